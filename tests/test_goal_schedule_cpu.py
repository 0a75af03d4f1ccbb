"""Goal schedules, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument and call-order errors come
back with the documented codes before the device is needed and valid arguments reach the device check; the NumPy restatement the GPU
tests compare against (tests/goal_schedule_ref.py) has the properties of the interpolation; the C++ example compiles and passes its
host checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import goal_schedule_ref as GS
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_goal_schedule_attach", "saip_batch_goal_schedule_detach", "saip_batch_goal_schedule_rewind",
                  "saip_batch_goal_schedule_info"]
POINTER_ENTRIES = ["saip_batch_goal_schedule_device"]
HOLD, LINEAR = 0, 1


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
    assert re.search(r"enum \{ SAIP_SCHEDULE_HOLD = 0, SAIP_SCHEDULE_LINEAR = 1 \};", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert (capi.SAIP_SCHEDULE_HOLD, capi.SAIP_SCHEDULE_LINEAR) == (0, 1)
    assert "csrc/saip_goal_schedule.hip" in capi.SOURCES      # the kernel is part of the library's sources


def _controller_batch(sp, L, B=4):
    """an unfinalized configuration-only batch with tasks 0 (motion-force, 36 goal rows) and 1 (joint, 21 goal rows)"""
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, B, -1, C.byref(b)) == 0
    pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
    assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
    assert L.saip_batch_add_joint_task(b, b"jt", None, 0, 0.001, C.byref(tid)) == 0
    return robot, b


def _others_refuse(L, b, code, task=0):
    n, p = C.c_int(7), C.c_longlong(7)
    assert L.saip_batch_goal_schedule_detach(b, task) == code
    assert L.saip_batch_goal_schedule_info(b, task, C.byref(n), None, None, None, None, C.byref(p)) == code
    assert L.saip_batch_goal_schedule_device(b, task) is None
    assert (n.value, p.value) == (7, 7)      # nothing was written


def _rot_keys(angles, B=None):
    """(K, 12) or (K, 12, B) keyframes: a position and a rotation about z by angles[k]"""
    K = len(angles)
    k = np.zeros((K, 12))
    k[:, 3:] = GS.exp_so3(np.outer(angles, [0.0, 0.0, 1.0])).reshape(K, 9)
    return k if B is None else np.ascontiguousarray(np.repeat(k[:, :, None], B, axis=2))


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    B = 4
    keys = np.zeros((3, 36, B))
    att = L.saip_batch_goal_schedule_attach
    # null batch
    assert att(None, 0, 0, 3, _dp(keys), 3, 1, HOLD, 1) == INVALID
    assert L.saip_batch_goal_schedule_detach(None, 0) == INVALID and L.saip_batch_goal_schedule_rewind(None) == INVALID
    assert L.saip_batch_goal_schedule_info(None, 0, None, None, None, None, None, None) == INVALID
    assert L.saip_batch_goal_schedule_device(None, 0) is None
    robot, b = _controller_batch(sp, L, B)
    try:
        # before finalize: the call-order error, whatever the arguments
        assert att(b, 0, 0, 3, _dp(keys), 3, 1, HOLD, 1) == ORDER
        assert att(b, 9, -1, 0, None, 0, 0, 5, 0) == ORDER
        assert L.saip_batch_goal_schedule_rewind(b) == ORDER
        assert L.saip_batch_goal_schedule_detach(b, -1) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_batch_goal_components(b, 0) == 36 and L.saip_batch_goal_components(b, 1) == 21
        # bad arguments: task, null keyframes, range, n_keyframes, stride, mode
        for task, first, count, K, stride, mode in [(-1, 0, 3, 3, 1, HOLD), (2, 0, 3, 3, 1, HOLD), (0, -1, 3, 3, 1, HOLD), (0, 0, 0, 3, 1, HOLD),
                                                    (0, 0, -2, 3, 1, HOLD), (0, 34, 3, 3, 1, HOLD), (0, 0, 37, 3, 1, HOLD), (0, 36, 1, 3, 1, HOLD),
                                                    (1, 15, 7, 3, 1, HOLD), (1, 0, 22, 3, 1, LINEAR), (0, 2**31 - 1, 2, 3, 1, HOLD),
                                                    (0, 0, 3, 0, 1, HOLD), (0, 0, 3, -1, 1, LINEAR), (0, 0, 3, 3, 0, HOLD), (0, 0, 3, 3, -4, LINEAR),
                                                    (0, 0, 3, 3, 1, 2), (0, 0, 3, 3, 1, -1)]:
            for per_instance in (0, 1):
                assert att(b, task, first, count, _dp(keys), K, stride, mode, per_instance) == INVALID, (task, first, count, K, stride, mode)
        assert att(b, 0, 0, 3, None, 3, 1, HOLD, 1) == INVALID and b"null keyframes" in L.saip_last_error()
        # LINEAR on a motion-force task: all of rows 3..11 or none of them
        rot = _rot_keys([0.0, 1.0, 2.0], B)
        for first, count in [(0, 4), (0, 11), (3, 8), (4, 8), (4, 9), (11, 1), (5, 2), (11, 10), (2, 2)]:
            assert att(b, 0, first, count, _dp(keys), 3, 1, LINEAR, 1) == INVALID, (first, count)
            assert b"all or none" in L.saip_last_error()
            assert att(b, 0, first, count, _dp(keys), 3, 1, HOLD, 1) == NO_DEVICE, (first, count)       # HOLD validates nothing
        # ... the same rows of a joint task are plain components
        assert att(b, 1, 2, 5, _dp(keys), 3, 1, LINEAR, 1) == NO_DEVICE
        # LINEAR over rows 3..11: every keyframe a rotation to 1e-6, consecutive keyframes at most pi - 1e-3 apart
        assert att(b, 0, 0, 12, _dp(rot), 3, 2, LINEAR, 1) == NO_DEVICE
        assert att(b, 0, 0, 12, _dp(_rot_keys([0.0, 1.0, 2.0])), 3, 2, LINEAR, 0) == NO_DEVICE
        assert att(b, 0, 3, 9, _dp(np.ascontiguousarray(rot[:, 3:])), 3, 2, LINEAR, 1) == NO_DEVICE
        assert att(b, 0, 0, 36, _dp(np.concatenate([rot, np.zeros((3, 24, B))], axis=1)), 3, 2, LINEAR, 1) == NO_DEVICE
        assert att(b, 0, 0, 12, _dp(keys), 3, 1, LINEAR, 1) == INVALID and b"orthonormal" in L.saip_last_error()     # R = 0
        skew = rot.copy()
        skew[1, 3 + 1, 2] += 3e-6                     # one entry of one instance's second keyframe
        assert att(b, 0, 0, 12, _dp(skew), 3, 1, LINEAR, 1) == INVALID and b"orthonormal" in L.saip_last_error()
        skew[1, 3 + 1, 2] = rot[1, 3 + 1, 2] + 1e-8   # inside the 1e-6 bound
        assert att(b, 0, 0, 12, _dp(skew), 3, 1, LINEAR, 1) == NO_DEVICE
        assert att(b, 0, 0, 12, _dp(skew), 3, 1, HOLD, 1) == NO_DEVICE
        far = _rot_keys([0.0, 1.0, 1.0 + np.pi - 5e-4], B)
        assert att(b, 0, 0, 12, _dp(far), 3, 1, LINEAR, 1) == INVALID and b"pi - 1e-3" in L.saip_last_error()
        assert att(b, 0, 0, 12, _dp(_rot_keys([0.0, 1.0, 1.0 + np.pi - 5e-4])), 3, 1, LINEAR, 0) == INVALID
        assert att(b, 0, 0, 12, _dp(_rot_keys([0.0, np.pi, 0.5])), 3, 1, LINEAR, 0) == INVALID
        assert att(b, 0, 0, 12, _dp(_rot_keys([0.0, 1.0, 1.0 + np.pi - 2e-3], B)), 3, 1, LINEAR, 1) == NO_DEVICE
        assert att(b, 0, 0, 12, _dp(far), 3, 1, HOLD, 1) == NO_DEVICE
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        assert att(b, 0, 0, 3, _dp(keys), 3, 1, HOLD, 1) == NO_DEVICE and b"no CPU path" in L.saip_last_error()
        assert att(b, 0, 30, 6, _dp(keys), 1, 5, LINEAR, 0) == NO_DEVICE      # the sensed force and moment rows
        assert att(b, 1, 0, 21, _dp(keys), 2, 1, LINEAR, 1) == NO_DEVICE
        _others_refuse(L, b, ORDER, 0)
        _others_refuse(L, b, ORDER, 1)
        _others_refuse(L, b, INVALID, 2)
        _others_refuse(L, b, INVALID, -3)
        assert L.saip_batch_goal_schedule_detach(b, -1) == 0      # all of none
        assert L.saip_batch_goal_schedule_rewind(b) == 0
    finally:
        L.saip_batch_destroy(b)


def test_keyframe_size_that_overflows_size_t_is_refused(sp):
    """n_keyframes x n_components x ld x 8 bytes past 2^64: a (configuration-only, so nothing is allocated or read) batch of 2^31 - 64
    instances, 36 rows and 2^31 - 1 keyframes is 1.3e21 bytes; one keyframe of it still fits and reaches the device check, and so do
    2^31 - 1 batch-uniform keyframes (6e11 bytes)"""
    from sai_primitives_amd import capi
    L = sp.lib()
    B = 2**31 - 64
    robot, b = _controller_batch(sp, L, B)
    try:
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_batch_ld(b) == B
        keys = np.zeros(64)
        assert L.saip_batch_goal_schedule_attach(b, 0, 0, 36, _dp(keys), 2**31 - 1, 1, HOLD, 1) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert b"too large" in L.saip_last_error()
        assert L.saip_batch_goal_schedule_attach(b, 0, 0, 36, _dp(keys), 1, 1, HOLD, 1) == capi.SAIP_ERR_NO_DEVICE
        assert L.saip_batch_goal_schedule_attach(b, 0, 0, 36, _dp(keys), 2**31 - 1, 1, HOLD, 0) == capi.SAIP_ERR_NO_DEVICE
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_schedules(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        keys = np.zeros((3, 3, 4))
        assert L.saip_batch_goal_schedule_attach(b, 0, 0, 3, _dp(keys), 3, 1, HOLD, 1) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        assert L.saip_batch_goal_schedule_rewind(b) == capi.SAIP_ERR_ORDER
        assert L.saip_batch_goal_schedule_detach(b, -1) == capi.SAIP_ERR_ORDER
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    with pytest.raises(ValueError, match="unknown field"):
        mf.setGoalSchedule("pose", np.zeros((3, 3)))
    with pytest.raises(ValueError, match="unknown field"):
        jt.setGoalSchedule("orientation", np.zeros((3, 9)))
    with pytest.raises(ValueError, match="unknown mode"):
        mf.setGoalSchedule("position", np.zeros((3, 3)), mode="cubic")
    for bad in (np.zeros((3, 4)), np.zeros((3, B + 1, 3)), np.zeros(3), np.zeros((3, 3, B))):
        with pytest.raises(ValueError, match="keyframes of shape"):
            mf.setGoalSchedule("position", bad)
    with pytest.raises(ValueError):
        mf.setGoalSchedule("position", np.zeros((3, 3)), stride=0)
    with pytest.raises(ValueError):
        mf.setGoalSchedule((30, 7), np.zeros((3, 7)))
    with pytest.raises(ValueError, match="all or none"):
        mf.setGoalSchedule((0, 6), np.zeros((3, 6)), mode="linear")
    with pytest.raises(ValueError, match="orthonormal"):
        mf.setGoalSchedule("orientation", np.zeros((3, B, 3, 3)), mode="linear")
    eye = np.broadcast_to(np.eye(3), (3, 3, 3))
    for task, field, keys, mode in [(mf, "position", np.zeros((3, 3)), "hold"), (mf, "orientation", eye, "linear"),
                                    (mf, "orientation", np.broadcast_to(np.eye(3), (3, B, 3, 3)), "linear"),
                                    (mf, "sensed_force", np.zeros((2, B, 3)), "linear"), (mf, (0, 12), np.zeros((3, B, 12)), "hold"),
                                    (jt, "position", np.zeros((3, 7)), "linear"), (jt, "acceleration", np.zeros((3, B, 7)), "hold")]:
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            task.setGoalSchedule(field, keys, stride=2, mode=mode)
    for fn in (mf.clearGoalSchedule, jt.clearGoalSchedule, mf.goalScheduleInfo):
        with pytest.raises(sp.SaipError, match="has no goal schedule"):
            fn()
    assert mf.goalScheduleDevice() is None
    ctrl.rewindGoalSchedules()


# ------------------------------------------------------------------ the NumPy restatement
def test_index_and_fraction_rule():
    K, stride = 3, 2
    got = [GS.index_fraction(c, K, stride) for c in range(7)]
    assert got == [(0, 0.0), (0, 0.5), (1, 0.0), (1, 0.5), (2, 0.0), (2, 0.0), (2, 0.0)]
    assert [GS.index_fraction(c, 1, 5) for c in range(3)] == [(0, 0.0)] * 3
    assert [GS.index_fraction(c, 4, 1) for c in range(5)] == [(0, 0.0), (1, 0.0), (2, 0.0), (3, 0.0), (3, 0.0)]
    assert GS.index_fraction(7, 4, 3) == (2, 1.0 / 3.0)


def _rotations(rng, shape, max_angle):
    axis = rng.normal(size=shape + (3,))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    return GS.exp_so3(axis * rng.uniform(0.0, max_angle, shape + (1,)))


def test_lerp_and_rows_reproduce_the_keyframes():
    rng = np.random.default_rng(5)
    keys = rng.normal(size=(3, 6, 4))
    a, b = keys[0], keys[1]
    assert np.array_equal(GS.lerp(a, b, 0.0), a)
    # a + 1 (b - a): the difference and the sum round once each, to half an ulp of numbers no larger than 2 max(|a|, |b|)
    assert (np.abs(GS.lerp(a, b, 1.0) - b) <= 2.0 ** -52 * 2.0 * np.maximum(np.abs(a), np.abs(b))).all()
    for mode in (GS.HOLD, GS.LINEAR):
        for k in range(3):
            assert np.array_equal(GS.rows(keys, 2 * k, 2, mode), keys[k])
        assert np.array_equal(GS.rows(keys, 9, 2, mode), keys[2])
    assert np.array_equal(GS.rows(keys, 3, 2, GS.HOLD), keys[1])
    assert np.array_equal(GS.rows(keys, 3, 2, GS.LINEAR), keys[1] + 0.5 * (keys[2] - keys[1]))


def test_slerp_properties():
    rng = np.random.default_rng(6)
    R0 = _rotations(rng, (200,), np.pi)
    step = _rotations(rng, (200,), 3.1)
    step[0] = np.eye(3)                       # the same orientation twice
    R1 = R0 @ step
    assert np.array_equal(GS.slerp(R0, R1, 0.0), R0)
    assert np.abs(GS.slerp(R0, R1, 1.0) - R1).max() <= 1e-13
    for s in (0.25, 0.5, 1.0 / 3.0, 0.9):
        R = GS.slerp(R0, R1, s)
        assert np.abs(np.swapaxes(R, -1, -2) @ R - np.eye(3)).max() <= 1e-14, s
        assert (np.linalg.det(R) > 0.999).all()
    half = np.swapaxes(R0, -1, -2) @ GS.slerp(R0, R1, 0.5)
    assert np.abs(half @ half - np.swapaxes(R0, -1, -2) @ R1).max() <= 1e-13
    assert np.array_equal(GS.slerp(R0[0], R1[0], 0.5), R0[0])
    # the rotation rows inside a range: rows() interpolates them on SO(3) and everything else component-wise
    keys = np.zeros((2, 200, 12))
    keys[:, :, :3] = rng.normal(size=(2, 200, 3))
    keys[0, :, 3:], keys[1, :, 3:] = R0.reshape(200, 9), R1.reshape(200, 9)
    r = GS.rows(keys, 1, 4, GS.LINEAR, rot_at=3)
    assert np.array_equal(r[:, :3], GS.lerp(keys[0, :, :3], keys[1, :, :3], 0.25))
    assert np.array_equal(r[:, 3:].reshape(200, 3, 3), GS.slerp(R0, R1, 0.25))


# ------------------------------------------------------------------ the C++ facade
def build_example(tmp_path):
    exe = str(tmp_path / "goal_schedule_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "goal_schedule_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_goal_schedule_example_host_checks(sp, tmp_path):
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "SCHEDULE_CFG_OK" in out.stdout, out.stdout + out.stderr
