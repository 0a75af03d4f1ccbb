"""The inertia table through the header-only C++ facade (tests/cpp/inertia_example.cpp): its host checks without a device, and on the GPU a
Panda with the config-2 stack whose instances each simulate a robot of their own (scaled links, a box in the hand) for 50 periods under
gravity -- the table and the final state agree with the same calls made through Python (in a process of its own), bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import workloads as W
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")


def build_example(tmp_path):
    exe = str(tmp_path / "inertia_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "inertia_example.cpp"),
                           "-L" + PKG, "-lsaip", "-L/opt/rocm/lib", "-lamdhip64", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_inertia_example_host_checks(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "INERTIA_CFG_OK" in out.stdout, out.stdout + out.stderr


# The same calls through the Python facade, in a process of its own like the example (this file runs in front of the tests that hand the
# GPU to torch first, and leaves the test process without a device context as the other test_cpp_* files do).  argv: B K q.bin out.bin;
# example_parts of the example: s = 0.9 + 0.2 i / B on every body, a box of (0.5 + 2 i / B) kg
PYTHON_SIDE = """
import sys
import numpy as np
import sai_primitives_amd as sp
B, K, n = int(sys.argv[1]), int(sys.argv[2]), 7
q = np.fromfile(sys.argv[3]).reshape(n, B).T
robot = sp.SaiModel("panda_arm", B, device=0)
mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
mf.disableInternalOtg()
jt.disableInternalOtg()
ctrl = sp.RobotController(robot, [mf, jt])
robot.setQ(q)
robot.setDq(np.zeros((B, n)))
robot.updateModel()
ctrl.reinitializeTasks()
ctrl.updateControllerTaskModels()
ctrl.attachInertia(per_instance=True, payload_links=["end-effector"])
i = np.arange(B)
bodies = np.zeros((n, B, 4))
bodies[:, :, 0] = 0.9 + 0.2 * i / B
pay = np.tile([0.0, 0.0, 0.0, 0.1, 0.05, 0.04, 0.03], (1, B, 1))
pay[0, :, 0] = 0.5 + 2.0 * i / B
ctrl.setInertiaParts(bodies, pay)
rows = ctrl.inertiaRows()
ctrl.rolloutAsync(K, 5e-4, 2)
ctrl.synchronize()
q1, dq1 = ctrl.pullState()
ctrl.detachInertia()
np.concatenate([rows.transpose(0, 2, 1).ravel(), q1.T.ravel(), dq1.T.ravel()]).tofile(sys.argv[4])
"""


@pytest.mark.gpu
def test_cpp_inertia_run_agrees_with_python(tmp_path):
    import sai_primitives_amd as sp
    sp.build_library()
    exe = build_example(tmp_path)
    B, K, n = 70, 50, 7
    ld = (B + 31) // 32 * 32
    d = W.make_inputs(2, B)
    qf, of, pf = tmp_path / "q.bin", tmp_path / "out.bin", tmp_path / "py.bin"
    np.ascontiguousarray(d["q"].T).tofile(qf)
    out = subprocess.run([exe, _robot_file(tmp_path), "run", str(B), str(K), str(qf), str(of)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "INERTIA_RUN_OK" in out.stdout, out.stdout + out.stderr
    raw = np.fromfile(of)
    rows, dev, q, dq = np.split(raw, np.cumsum([n * 10 * B, n * 10 * ld, n * B]))
    rows, dev = rows.reshape(n, 10, B), dev.reshape(n * 10, ld)
    assert np.array_equal(dev[:, :B], rows.reshape(n * 10, B)) and not dev[:, B:].any()      # the padding columns were never written
    out = subprocess.run([sys.executable, "-c", PYTHON_SIDE, str(B), str(K), str(qf), str(pf)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout + out.stderr
    want_rows, want_q, want_dq = np.split(np.fromfile(pf), np.cumsum([n * 10 * B, n * B]))
    bits = lambda a: np.ascontiguousarray(a, np.float64).view(np.uint64)
    assert np.array_equal(bits(rows.ravel()), bits(want_rows))
    assert np.array_equal(bits(q), bits(want_q)) and np.array_equal(bits(dq), bits(want_dq))
    assert (np.diff(rows[6, 0]) > 0).all() and np.isfinite(q).all() and np.abs(dq).max() > 0  # every instance its own payload; the arms moved
