"""Task-space diagnostics of a motion-force task, host side (no GPU needed): the C-ABI entries are declared, exported and bound, every
getter refuses to run without a device, a joint task and a call before finalize are refused with the documented codes, and the C++
facade example compiles and passes its host checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
ENTRIES = ["saip_batch_get_task_diagnostics_host", "saip_batch_task_diagnostics_device"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def test_entries_declared_exported_and_bound(sp):
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L._declared
        assert getattr(L, name).restype is C.c_int


def _cfg_only(sp, B=4):
    robot = sp.SaiModel("panda_arm", B, device=-1)  # configuration-only batch: host logic without a device
    tasks = [sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)]
    ctrl = sp.RobotController(robot, tasks)
    robot.setQ(np.zeros((B, 7)))
    return robot, ctrl, tasks


def test_python_getters_need_a_device(sp):
    robot, ctrl, (mf, jt) = _cfg_only(sp)
    for fn in ["getTaskDiagnostics", "getPositionError", "getOrientationError", "getCurrentLinearVelocity", "getCurrentAngularVelocity",
               "getSensedForceControlWorldFrame", "getSensedMomentControlWorldFrame", "getUnitMassForce"]:
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            getattr(mf, fn)()


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot, ctrl, (mf, jt) = _cfg_only(sp)
    out = np.zeros(24 * 4)
    p = out.ctypes.data_as(C.POINTER(C.c_double))
    # joint task and out-of-range ids: the task-type error
    for tid in (jt._id, 7, -1):
        assert L.saip_batch_get_task_diagnostics_host(ctrl._h, tid, p) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert L.saip_batch_task_diagnostics_device(ctrl._h, tid, None) == capi.SAIP_ERR_INVALID_ARGUMENT
    # finalized batch without a device
    assert L.saip_batch_get_task_diagnostics_host(ctrl._h, mf._id, p) == capi.SAIP_ERR_NO_DEVICE
    assert b"no CPU path" in L.saip_last_error()
    assert L.saip_batch_task_diagnostics_device(ctrl._h, mf._id, None) == capi.SAIP_ERR_NO_DEVICE
    # before saip_batch_finalize: the call-order error
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == capi.SAIP_OK
    try:
        pos = (C.c_double * 3)(0, 0, 0.07)
        tid = C.c_int(-1)
        assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == capi.SAIP_OK
        assert L.saip_batch_get_task_diagnostics_host(b, tid.value, p) == capi.SAIP_ERR_ORDER
        assert L.saip_batch_task_diagnostics_device(b, tid.value, None) == capi.SAIP_ERR_ORDER
    finally:
        L.saip_batch_destroy(b)


def _robot_file(tmp_path):
    robot = tmp_path / "robot.txt"
    m = W.load_robot("panda_arm")
    jt = {"fixed": 0, "revolute": 1, "prismatic": 2}
    with open(robot, "w") as f:
        f.write(f"{len(m.links)}\n")
        for l in m.links:
            vals = l["origin_xyz"] + l["origin_rpy"] + l["axis"] + [l["mass"]] + l["com"] + l["inertia"] + \
                [l["q_lower"], l["q_upper"], l["velocity_limit"], l["effort_limit"]]
            f.write(f"{l['name']} {jt[l['joint_type']]} " + " ".join(repr(float(v)) for v in vals) + "\n")
    return str(robot)


def test_cpp_diagnostics_example_host_checks(sp, tmp_path):
    exe = str(tmp_path / "diagnostics_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "diagnostics_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "DIAG_CFG_OK" in out.stdout, out.stdout + out.stderr
