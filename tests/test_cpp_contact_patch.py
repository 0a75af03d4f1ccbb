"""Contact patches through the header-only C++ facade (tests/cpp/contact_patch_example.cpp): its host checks without a device, and on the
GPU a Panda with a config-13-like closed-loop force stack pressing a four-point plate on a table at B = 3; the example checks itself and
its numbers are those of the same case through the Python facade at (3, 64)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import workloads as W
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
SQUARE = np.array([[0.05, 0.05, 0.0], [-0.05, 0.05, 0.0], [-0.05, -0.05, 0.0], [0.05, -0.05, 0.0]])


def python_half(qf, pf, of, B, ld, K):
    """the same case through the Python facade: readout [20][B], summary [6][B], q, dq, torques [dof][B] written like the example's"""
    import sai_primitives_amd as sp
    n = 7
    q = np.fromfile(qf).reshape(n, B).T
    planes = np.fromfile(pf).reshape(1, 8, B).transpose(0, 2, 1)
    robot = sp.SaiModel("panda_arm", B, device=0)
    mf = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07))
    mf.disableInternalOtg()
    mf.parametrizeForceMotionSpaces(1, [0.0, 0.0, 1.0])
    mf.setForceControlGains(0.9, 12.0, 1.7)
    mf.setClosedLoopForceControl(True)
    mf.enablePassivity()
    jt = sp.JointTask(robot)
    jt.disableInternalOtg()
    ctrl = sp.RobotController(robot, [mf, jt], leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(np.zeros((B, n)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    mf.setGoalForce(np.broadcast_to((0.0, 0.0, -5.0), (B, 3)))
    ctrl.updateControllerTaskModels()
    mf.attachContactPatch(SQUARE, planes, sensor=True, per_instance=True)
    ctrl.rolloutAsync(K, 5e-4, 2, gravity=(0.0, 0.0, 0.0))
    ctrl.synchronize()
    want = np.empty((20 + 6, B))
    ctrl._call("saip_batch_contact_patch_readout_host", mf._id, want[:20].ctypes.data_as(C.POINTER(C.c_double)))
    ctrl._call("saip_batch_contact_patch_summary_host", mf._id, want[20:].ctypes.data_as(C.POINTER(C.c_double)))
    pq, pdq = ctrl.pullState()
    ptau = ctrl.getTorques()
    mf.detachContactPatch()
    np.concatenate([want, pq.T, pdq.T, ptau.T]).tofile(of)


def build_example(tmp_path):
    exe = str(tmp_path / "contact_patch_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "contact_patch_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_contact_patch_example_host_checks(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "CONTACT_PATCH_CFG_OK" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_cpp_plate_on_a_table_reproduces_the_python_numbers(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    B, ld, K, n = 3, 64, 40, 7
    d = W.make_inputs(13, B)
    q, model = d["q"], d["model"]
    # a table facing up, the plate's lowest corner 0.1 mm inside (placed with the host kinematics: both runs read the same file)
    R, o = W.fk(model, q)[model.link_index("end-effector")]
    pz = np.stack([(o + np.einsum("bij,j->bi", R, np.array([0, 0, 0.07]) + r))[:, 2] for r in SQUARE])
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, 2.0e4, 400.0, 0.3, 1e-3]
    planes[0, :, 3] = pz.min(axis=0) + 1e-4
    # the example first, in its own process, while this one has not touched the device
    qf, pf, of = tmp_path / "q.bin", tmp_path / "planes.bin", tmp_path / "out.bin"
    np.ascontiguousarray(q.T).tofile(qf)
    np.ascontiguousarray(planes.transpose(0, 2, 1)).tofile(pf)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(K), str(qf), str(pf), str(of)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "CONTACT_PATCH_RUN_OK" in out.stdout, out.stdout + out.stderr
    got = np.fromfile(of).reshape(26 + 3 * n, B)
    # the same stack through the Python facade, in a process of its own as well: this one must not load the engine, since a later test of
    # the suite imports torch, whose own HIP runtime has to be the first one loaded into a process
    wf = tmp_path / "want.bin"
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [x for x in (os.environ.get("PYTHONPATH"),) if x]))
    py = subprocess.run([sys.executable, os.path.abspath(__file__), str(qf), str(pf), str(wf), str(B), str(ld), str(K)], capture_output=True, text=True,
                        timeout=300, env=env)
    assert py.returncode == 0, py.stdout + py.stderr
    ref = np.fromfile(wf).reshape(26 + 3 * n, B)
    assert np.array_equal(got, ref)
    assert (ref[7] >= 1).all() and (ref[20 + 3] > 0).all()


if __name__ == "__main__":
    python_half(sys.argv[1], sys.argv[2], sys.argv[3], *(int(a) for a in sys.argv[4:7]))
