"""Rollout recorder, host side (no GPU needed): the C-ABI entries are declared, exported and bound, the argument and call-order errors
come back with the documented codes (before finalize, on a model-only batch, with bad arguments, without a recorder), valid arguments
reach the device check, and the C++ facade example compiles and passes its host checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_rollout_recorder_attach", "saip_batch_rollout_recorder_detach", "saip_batch_rollout_recorder_reset",
                  "saip_batch_rollout_log_info", "saip_batch_rollout_log_host", "saip_batch_rollout_summary_host"]
POINTER_ENTRIES = ["saip_batch_rollout_log_device", "saip_batch_rollout_summary_device"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    assert re.search(r"SAIP_RECORD_Q = 1, SAIP_RECORD_DQ = 2, SAIP_RECORD_TAU = 4, SAIP_RECORD_POSE = 8, SAIP_RECORD_ERROR = 16", hdr)
    assert re.search(r"#define SAIP_RECORD_SUMMARY_ROWS 8\b", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert (capi.SAIP_RECORD_Q, capi.SAIP_RECORD_DQ, capi.SAIP_RECORD_TAU, capi.SAIP_RECORD_POSE, capi.SAIP_RECORD_ERROR) == (1, 2, 4, 8, 16)
    assert capi.SAIP_RECORD_SUMMARY_ROWS == 8
    # the kernel is part of the library's sources
    assert "csrc/saip_rollout_record.hip" in capi.SOURCES


def _readers_refuse(L, b, code):
    n = C.c_int(7)
    buf = np.zeros(64)
    assert L.saip_batch_rollout_recorder_detach(b) == code
    assert L.saip_batch_rollout_recorder_reset(b) == code
    assert L.saip_batch_rollout_log_info(b, C.byref(n), None, None, None) == code
    assert L.saip_batch_rollout_log_host(b, _dp(buf), None) == code
    assert L.saip_batch_rollout_summary_host(b, _dp(buf)) == code
    assert L.saip_batch_rollout_log_device(b) is None and L.saip_batch_rollout_summary_device(b) is None
    assert n.value == 7  # nothing was written


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    # null batch
    assert L.saip_batch_rollout_recorder_attach(None, 4, 1, 7, -1, 0) == INVALID
    assert L.saip_batch_rollout_log_device(None) is None and L.saip_batch_rollout_summary_device(None) is None
    # before finalize: the call-order error, whatever the arguments
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
        assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
        assert L.saip_batch_add_joint_task(b, b"jt", None, 0, 0.001, C.byref(tid)) == 0
        assert L.saip_batch_rollout_recorder_attach(b, 4, 1, 7, -1, 0) == ORDER
        assert L.saip_batch_rollout_recorder_attach(b, 0, 0, 99, 5, 0) == ORDER
        _readers_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        # a controller batch (tasks: 0 motion-force, 1 joint): bad arguments
        for cap, stride, ch, task, sums in [(0, 1, 7, -1, 0), (-3, 1, 7, -1, 0), (4, 0, 7, -1, 0), (4, -1, 7, -1, 0), (4, 1, 32, -1, 0),
                                            (4, 1, 7 | 64, -1, 1), (4, 1, 0, -1, 0), (4, 1, 0, 0, 0), (4, 1, 8, -1, 0), (4, 1, 16, -1, 1),
                                            (4, 1, 24, 1, 0), (4, 1, 7, 1, 1), (4, 1, 7, 2, 0), (4, 1, 7, -2, 0)]:
            assert L.saip_batch_rollout_recorder_attach(b, cap, stride, ch, task, sums) == INVALID, (cap, stride, ch, task, sums)
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        assert L.saip_batch_rollout_recorder_attach(b, 4, 1, 7, -1, 0) == capi.SAIP_ERR_NO_DEVICE
        assert b"no CPU path" in L.saip_last_error()
        assert L.saip_batch_rollout_recorder_attach(b, 4, 3, 31, 0, 1) == capi.SAIP_ERR_NO_DEVICE
        assert L.saip_batch_rollout_recorder_attach(b, 4, 1, 0, -1, 1) == capi.SAIP_ERR_NO_DEVICE
        _readers_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_log_size_that_overflows_size_t_is_refused(sp):
    """capacity x rows x ld x 8 bytes past 2^64: a (configuration-only, so nothing is allocated) batch of 2^31 - 64 instances, 39 rows and
    2^31 - 1 samples is 1.4e21 bytes; one sample of it still fits and reaches the device check"""
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    B = 2**31 - 64
    assert L.saip_batch_create(robot._h, B, -1, C.byref(b)) == 0
    try:
        pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
        assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_batch_ld(b) == B
        assert L.saip_batch_rollout_recorder_attach(b, 2**31 - 1, 1, 31, 0, 1) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert b"too large" in L.saip_last_error()
        assert L.saip_batch_rollout_recorder_attach(b, 1, 1, 31, 0, 1) == capi.SAIP_ERR_NO_DEVICE
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_the_recorder(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_rollout_recorder_attach(b, 4, 1, 7, -1, 0) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _readers_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    other = sp.MotionForceTask(robot, "end-effector", task_name="elsewhere")
    with pytest.raises(ValueError, match="unknown channel"):
        ctrl.recordRollouts(4, channels=("q", "torque"))
    with pytest.raises(ValueError, match="does not belong"):
        ctrl.recordRollouts(4, channels=("error",), task=other)
    with pytest.raises(ValueError, match="not a MotionForceTask"):
        ctrl.recordRollouts(4, channels=("error",), task="joint_task")
    with pytest.raises(ValueError):
        ctrl.recordRollouts(0)
    with pytest.raises(ValueError):
        ctrl.recordRollouts(4, stride=0)
    with pytest.raises(ValueError):
        ctrl.recordRollouts(4, channels=())
    with pytest.raises(ValueError):
        ctrl.recordRollouts(4, channels=("pose",))
    with pytest.raises(ValueError):
        ctrl.recordRollouts(4, channels=("q",), task=jt)
    with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
        ctrl.recordRollouts(4, 2, ("q", "dq", "tau", "pose", "error"), task=mf, summaries=True)
    with pytest.raises(sp.SaipNoDevice):
        ctrl.recordRollouts(4, channels=(), summaries=True, task="motion_force_task")
    for fn in (ctrl.rolloutLog, ctrl.rolloutSummary, ctrl.resetRolloutRecorder, ctrl.stopRecordingRollouts):
        with pytest.raises(sp.SaipError, match="no rollout recorder"):
            fn()


def _robot_file(tmp_path, name="panda_arm"):
    robot = tmp_path / "robot.txt"
    m = W.load_robot(name)
    jt = {"fixed": 0, "revolute": 1, "prismatic": 2}
    with open(robot, "w") as f:
        f.write(f"{len(m.links)}\n")
        for l in m.links:
            vals = l["origin_xyz"] + l["origin_rpy"] + l["axis"] + [l["mass"]] + l["com"] + l["inertia"] + \
                [l["q_lower"], l["q_upper"], l["velocity_limit"], l["effort_limit"]]
            f.write(f"{l['name']} {jt[l['joint_type']]} " + " ".join(repr(float(v)) for v in vals) + "\n")
    return str(robot)


def build_example(tmp_path):
    exe = str(tmp_path / "rollout_record_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "rollout_record_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_rollout_record_example_host_checks(sp, tmp_path):
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "RECORD_CFG_OK" in out.stdout, out.stdout + out.stderr
