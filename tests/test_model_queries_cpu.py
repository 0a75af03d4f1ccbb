"""Robot-model queries, host side (no GPU needed): the C-ABI entries are declared, exported and bound, every query refuses to run without
a device, argument errors and calls before finalize are refused with the documented codes, a model-only batch refuses every entry that
needs a task, and the C++ facade example compiles and passes its host checks."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
ENTRIES = ["saip_batch_set_robot_base", "saip_batch_get_robot_base", "saip_batch_model_frame_rows", "saip_batch_model_frames_host",
           "saip_batch_model_frames_device", "saip_batch_model_dynamics_host", "saip_batch_model_dynamics_device",
           "saip_batch_finalize_model_only"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entries_declared_exported_and_bound(sp):
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    assert re.search(r"#define SAIP_MAX_QUERY_FRAMES 8\b", hdr)
    assert re.search(r"SAIP_QUERY_JACOBIAN = 1, SAIP_QUERY_WORLD = 2", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    for name in ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name in L._declared
        assert getattr(L, name).restype is C.c_int
    assert (sp.SAIP_MAX_QUERY_FRAMES, sp.SAIP_QUERY_JACOBIAN, sp.SAIP_QUERY_WORLD) == (8, 1, 2)


def _batch(sp, robot, B=4, finalize="model"):
    L = sp.lib()
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, B, -1, C.byref(b)) == 0
    if finalize == "model":
        assert L.saip_batch_finalize_model_only(b) == 0
    return b


def test_frame_rows(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    for name, n in (("panda_arm", 7), ("panda_sliding_base", 8), ("chain30", 30)):
        robot = sp.SaiModel(name, 4, device=-1)
        b = _batch(sp, robot)
        try:
            assert L.saip_batch_model_frame_rows(b, 0) == 18
            assert L.saip_batch_model_frame_rows(b, capi.SAIP_QUERY_WORLD) == 18
            assert L.saip_batch_model_frame_rows(b, capi.SAIP_QUERY_JACOBIAN) == 18 + 6 * n
            assert L.saip_batch_model_frame_rows(b, 3) == 18 + 6 * n
            assert L.saip_batch_model_frame_rows(b, 4) == 0
            assert L.saip_batch_model_frame_rows(None, 0) == 0
        finally:
            L.saip_batch_destroy(b)


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_sliding_base", 4, device=-1)
    nl = len(robot.description["links"])
    out = np.zeros(8 * (18 + 6 * 8) * 4)
    M = np.zeros(64 * 4)
    links, pos = np.array([robot.linkIndex("end-effector"), 0], np.int32), np.zeros(6)
    # before finalize: the call-order error
    b = _batch(sp, robot, finalize=None)
    try:
        assert L.saip_batch_model_frames_host(b, 2, _ip(links), _dp(pos), 1, _dp(out)) == capi.SAIP_ERR_ORDER
        assert L.saip_batch_model_frames_device(b, 2, _ip(links), None, 0, None) == capi.SAIP_ERR_ORDER
        assert L.saip_batch_model_dynamics_host(b, _dp(M), None, None, None) == capi.SAIP_ERR_ORDER
        assert L.saip_batch_model_dynamics_device(b, None, None, None, None) == capi.SAIP_ERR_ORDER
    finally:
        L.saip_batch_destroy(b)
    b = _batch(sp, robot)
    try:
        bad = [(0, links, 0, out), (9, np.zeros(9, np.int32), 0, out), (1, np.array([nl], np.int32), 0, out),
               (1, np.array([-1], np.int32), 0, out), (1, links, 4, out), (1, links, -1, out), (1, None, 0, out), (1, links, 0, None)]
        for nf, lk, flags, o in bad:
            lp = None if lk is None else _ip(lk)
            assert L.saip_batch_model_frames_host(b, nf, lp, None, flags, None if o is None else _dp(o)) == capi.SAIP_ERR_INVALID_ARGUMENT
            assert L.saip_batch_model_frames_device(b, nf, lp, None, flags, None if o is None else 1) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert L.saip_batch_model_dynamics_host(b, None, None, None, None) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert L.saip_batch_model_dynamics_device(b, None, None, None, None) == capi.SAIP_ERR_INVALID_ARGUMENT
        # configuration-only batch: valid arguments reach the device check
        assert L.saip_batch_model_frames_host(b, 2, _ip(links), _dp(pos), 3, _dp(out)) == capi.SAIP_ERR_NO_DEVICE
        assert b"no CPU path" in L.saip_last_error()
        assert L.saip_batch_model_frames_device(b, 2, _ip(links), None, 0, 1) == capi.SAIP_ERR_NO_DEVICE
        assert L.saip_batch_model_dynamics_host(b, _dp(M), None, None, None) == capi.SAIP_ERR_NO_DEVICE
        assert L.saip_batch_model_dynamics_device(b, None, None, 1, None) == capi.SAIP_ERR_NO_DEVICE
        # the robot base: identity by default, round trip, null arguments
        R, p = np.zeros(9), np.ones(3)
        assert L.saip_batch_get_robot_base(b, _dp(R), _dp(p)) == 0
        assert np.array_equal(R, np.eye(3).ravel()) and np.array_equal(p, np.zeros(3))
        R2, p2 = np.array([0., -1, 0, 1, 0, 0, 0, 0, 1]), np.array([0.5, -0.25, 0.1])
        assert L.saip_batch_set_robot_base(b, _dp(R2), _dp(p2)) == 0
        assert L.saip_batch_get_robot_base(b, _dp(R), _dp(p)) == 0
        assert np.array_equal(R, R2) and np.array_equal(p, p2)
        assert L.saip_batch_set_robot_base(b, None, _dp(p2)) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert L.saip_batch_set_robot_base(None, _dp(R2), _dp(p2)) == capi.SAIP_ERR_INVALID_ARGUMENT
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_controller_entries(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = _batch(sp, robot, finalize=None)
    try:
        # saip_batch_finalize still refuses a batch without tasks
        assert L.saip_batch_finalize(b) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert L.saip_batch_finalize_model_only(b) == capi.SAIP_OK
        assert L.saip_batch_finalize_model_only(b) == capi.SAIP_OK
        buf = np.zeros(7 * 32 * 32)
        t, st = _dp(buf), buf.ctypes.data_as(C.POINTER(C.c_ubyte))
        ms = C.c_double()
        ORDER = capi.SAIP_ERR_ORDER
        assert L.saip_batch_step_async(b) == ORDER
        assert L.saip_batch_compute_control_torques(b, t, st) == ORDER
        assert L.saip_batch_update_task_models(b) == ORDER
        assert L.saip_batch_get_torques_host(b, t, st) == ORDER
        assert L.saip_batch_integrate(b, 0.001, 1, None, 0.0) == ORDER
        assert L.saip_batch_rollout_async(b, 1, 0.001, 1, None, 0.0) == ORDER
        assert L.saip_batch_set_torques_host(b, t) == ORDER
        assert L.saip_batch_time_steps(b, 2, 1, C.byref(ms)) == ORDER
        assert L.saip_batch_reinitialize_tasks(b) == ORDER
        for fn, args in [("saip_batch_get_current_pose_host", (0, t, t)), ("saip_batch_get_task_diagnostics_host", (0, t)),
                         ("saip_batch_task_update_model", (0, None)), ("saip_batch_get_goal_host", (0, t)),
                         ("saip_batch_set_goal_host", (0, t)), ("saip_batch_get_desired_host", (0, t)),
                         ("saip_batch_reinitialize_task", (0,)), ("saip_batch_reset_integrators", (0, 3))]:
            assert getattr(L, fn)(b, *args) == ORDER, fn
        # the state entries only need a device
        assert L.saip_batch_set_state_host(b, t, t) == capi.SAIP_ERR_NO_DEVICE
        assert L.saip_batch_get_state_host(b, t, t) == capi.SAIP_ERR_NO_DEVICE
        # a batch with tasks cannot be finalized for model queries only
        b2 = _batch(sp, robot, finalize=None)
        try:
            pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
            assert L.saip_batch_add_motion_force_task(b2, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
            assert L.saip_batch_finalize_model_only(b2) == capi.SAIP_ERR_INVALID_ARGUMENT
        finally:
            L.saip_batch_destroy(b2)
    finally:
        L.saip_batch_destroy(b)


def test_python_queries_need_a_device(sp):
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    robot.setQ(np.zeros((4, 7)))
    for fn, args in [("position", ("end-effector", (0, 0, 0.07))), ("rotation", ("link7",)), ("transform", ("end-effector",)),
                     ("linearVelocity", ("end-effector",)), ("angularVelocity", ("end-effector",)), ("J", ("end-effector",)),
                     ("Jv", ("end-effector",)), ("Jw", (3,)), ("positionInWorld", ("end-effector",)), ("rotationInWorld", ("link7",)),
                     ("transformInWorld", ("end-effector",)), ("linearVelocityInWorld", ("end-effector",)),
                     ("angularVelocityInWorld", ("end-effector",)), ("JWorldFrame", ("end-effector",)), ("M", ()), ("MInv", ()),
                     ("jointGravityVector", ()), ("coriolisForce", ())]:
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            getattr(robot, fn)(*args)
    with pytest.raises(ValueError, match="does not exist"):
        robot.position("no-such-link")
    tasks = [sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)]
    ctrl = sp.RobotController(robot, tasks)
    with pytest.raises(sp.SaipNoDevice):
        ctrl.getModelFrames(["end-effector", ("link3", (0.1, 0, 0))], jacobian=True, world=True)
    with pytest.raises(sp.SaipNoDevice):
        ctrl.getModelDynamics()
    with pytest.raises(ValueError):
        ctrl.getModelFrames([("end-effector", None)] * 9)


def test_python_robot_base_reaches_every_batch(sp):
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    T = np.eye(4)
    T[:3, :3] = [[0, -1, 0], [1, 0, 0], [0, 0, 1]]
    T[:3, 3] = [0.5, -0.25, 0.1]
    ctrl = sp.RobotController(robot, [sp.MotionForceTask(robot, "end-effector"), sp.JointTask(robot)])
    robot.setTRobotBase(T)
    assert np.array_equal(robot.TRobotBase(), T)
    ctrl2 = sp.RobotController(robot, [sp.JointTask(robot)])  # attached after the call
    with pytest.raises(sp.SaipNoDevice):
        robot.M()  # creates the model-only batch
    for h in (ctrl._h, ctrl2._h, robot._mq):
        R, p = np.zeros(9), np.zeros(3)
        assert L.saip_batch_get_robot_base(h, _dp(R), _dp(p)) == 0
        assert np.array_equal(R.reshape(3, 3), T[:3, :3]) and np.array_equal(p, T[:3, 3])
    with pytest.raises(ValueError):
        robot.setTRobotBase(np.eye(3))


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
    exe = str(tmp_path / "model_queries_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "model_queries_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    return exe


def test_cpp_model_queries_example_host_checks(sp, tmp_path):
    exe = build_example(tmp_path)
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "MQ_CFG_OK" in out.stdout, out.stdout + out.stderr
