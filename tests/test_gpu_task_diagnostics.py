"""MotionForceTask task-space diagnostics (saip_task_diag_kernel through saip_batch_get_task_diagnostics_host / _device and the Python
getters) against a NumPy expectation: workloads.fk / jacobian / mf_projection, the oracle's orientation_error / sigma_space and the F_um of
restatement.controller_step_single."""
import os
import subprocess

import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
TOL = 1e-9
ROWS = ["position_error", "orientation_error", "linear_velocity", "angular_velocity", "sensed_force", "sensed_moment", "unit_mass_force"]


def _close(a, b, tol=TOL):
    return np.all(np.abs(a - b) <= tol * (1.0 + np.abs(b)))


def _no_ki(tasks):
    out = []
    for t in tasks:
        t = dict(t)
        if t["type"] == "motion_force":
            t["ki_pos"], t["ki_ori"] = 0.0, 0.0
        else:
            t["ki"] = 0.0
        out.append(t)
    return out


def _controller(cfg, B, tasks=None, ld=None):
    from sai_primitives_amd.controller import controller_from_specs
    d = W.make_inputs(cfg, B)
    if tasks is not None:
        d["tasks"] = tasks
    robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, leading_dimension=ld)
    robot.setQ(d["q"])
    robot.setDq(d["dq"])
    robot.updateModel()
    ctrl.setGoals(d["goals"])
    return d, robot, ctrl, objs


def _expected(d, ti, fum_stride):
    """(B, 24) rows 0..17 for every instance; F_um rows 18..23 for every `fum_stride`-th instance (NaN elsewhere)"""
    from restatement import orientation_error, sigma_space, controller_step_single
    model, t, q, dq, g = d["model"], d["tasks"][ti], d["q"], d["dq"], d["goals"][ti]
    B = q.shape[0]
    frames = W.fk(model, q)
    li = model.link_index(t["link"])
    Rl, ol = frames[li]
    x = ol + Rl @ np.asarray(t["pos_in_link"])
    Rc = Rl @ np.asarray(t["rot_in_link"])
    P = W.mf_projection(t)[0]
    assert np.all(P[:3, 3:] == 0) and np.all(P[3:, :3] == 0)  # block-diagonal: TaskDev::Ppos / Pori carry all of it
    J = np.einsum("ij,bjk->bik", P, W.jacobian(model, frames, li, x))
    tw = np.einsum("bij,bj->bi", J, dq)
    out = np.full((B, 24), np.nan)
    for b in range(B):
        rot = Rc[b] if t["param_in_compliant_frame"] else np.eye(3)
        sf = sigma_space(P[:3, :3], t["force_dim"], t["force_axis"], rot)
        sm = sigma_space(P[3:, 3:], t["moment_dim"], t["moment_axis"], rot)
        sp_ = P[:3, :3] @ (np.eye(3) - sf) @ P[:3, :3].T
        so = P[3:, 3:] @ (np.eye(3) - sm) @ P[3:, 3:].T
        out[b, 0:3] = sp_ @ (g[b, 0:3] - x[b])
        out[b, 3:6] = so @ orientation_error(g[b, 3:12].reshape(3, 3), Rc[b])
        out[b, 6:12] = tw[b]
        out[b, 12:18] = 0.0
        if g.shape[1] >= 36:
            Rcs, tcs = np.asarray(t.get("Rcs", np.eye(3)), float), np.asarray(t.get("tcs", np.zeros(3)), float)
            fc = Rcs @ g[b, 30:33]
            mc = np.cross(tcs, fc) + Rcs @ g[b, 33:36]
            out[b, 12:15], out[b, 15:18] = Rc[b] @ fc, Rc[b] @ mc
        if b % fum_stride == 0:
            det = []
            controller_step_single(model, d["tasks"], q[b], dq[b], [gg[b] for gg in d["goals"]], details=det)
            out[b, 18:24] = det[ti]["F_um"]
    return out


def _diag(task):
    r = task.getTaskDiagnostics()
    return np.concatenate([r[k] for k in ROWS], axis=1)


@pytest.mark.parametrize("cfg,B,stride", [(2, 4096, 16), (3, 4096, 16), (9, 256, 1), (13, 256, 1), (5, 4096, 64)])
def test_diagnostics_match_numpy(cfg, B, stride):
    """config 2: full task (law_identity); 3: partial position task (P-projected velocity rows); 9: force space dim 1 + moment space
    dim 2 in the compliant frame; 13: closed-loop force / moment with a rotated / offset sensor; 5: 30-dof chain, two motion-force
    tasks.  F_um is compared on every `stride`-th instance (the oracle is a per-instance Python restatement)."""
    tasks = _no_ki(W.make_inputs(cfg, 1)["tasks"])
    d, robot, ctrl, objs = _controller(cfg, B, tasks)
    if cfg == 13:
        assert d["goals"][0].shape[1] == 36 and np.abs(d["goals"][0][:, 30:36]).max() > 0  # a sensed wrench is pushed through the goal block
    mf = [i for i, t in enumerate(d["tasks"]) if t["type"] == "motion_force"]
    assert len(mf) == (2 if cfg == 5 else 1)
    for ti in mf:
        got = _diag(objs[ti])
        exp = _expected(d, ti, stride)
        assert _close(got[:, :18], exp[:, :18]), (cfg, ti, np.abs(got[:, :18] - exp[:, :18]).max())
        sel = np.arange(0, B, stride)
        assert _close(got[sel, 18:], exp[sel, 18:]), (cfg, ti, np.abs(got[sel, 18:] - exp[sel, 18:]).max())
        if cfg == 3:
            P = W.mf_projection(d["tasks"][ti])[0]
            assert np.abs(P[3:, 3:]).max() == 0 and np.all(got[:, 9:12] == 0)  # angular rows projected away


def test_single_getters_and_pose_agreement():
    """the seven getters return the rows of getTaskDiagnostics(); with sigma = I the position error is goal - getCurrentPosition() bit for bit"""
    d, robot, ctrl, objs = _controller(2, 512)
    mf = objs[0]
    r = mf.getTaskDiagnostics()
    for k, fn in zip(ROWS, ["getPositionError", "getOrientationError", "getCurrentLinearVelocity", "getCurrentAngularVelocity",
                            "getSensedForceControlWorldFrame", "getSensedMomentControlWorldFrame", "getUnitMassForce"]):
        v = getattr(mf, fn)()
        assert v.shape == ((512, 6) if k == "unit_mass_force" else (512, 3))
        assert np.array_equal(v, r[k]), fn
    assert np.array_equal(r["position_error"], mf.getGoalPosition() - mf.getCurrentPosition())


def test_zero_velocity_gives_zero_twist():
    d, robot, ctrl, objs = _controller(5, 256)
    robot.setDq(np.zeros_like(d["dq"]))
    for t in (objs[0], objs[1]):
        r = t.getTaskDiagnostics()
        assert np.all(r["linear_velocity"] == 0.0) and np.all(r["angular_velocity"] == 0.0)


def _run_cycles(cfg, tasks, with_diag, n=5):
    d, robot, ctrl, objs = _controller(cfg, 256, tasks)
    taus = []
    for k in range(n):
        q = d["q"] + 1e-3 * k
        robot.setQ(q)
        robot.setDq(d["dq"])
        robot.updateModel()
        ctrl.updateControllerTaskModels()
        ctrl.setGoals(d["goals"])
        if with_diag:
            objs[0].getTaskDiagnostics()
        taus.append(ctrl.computeControlTorques().copy())
    after = objs[0].getTaskDiagnostics()["unit_mass_force"]  # depends on the integrators the five cycles left behind
    return np.array(taus), after, objs[0].getGoalPosition(), objs[0].getDesiredPosition()


@pytest.mark.parametrize("cfg", [2, 13])
def test_no_side_effects(cfg):
    """two identical controllers, one reading the diagnostics before every cycle: torques (which carry the integrators forward), goals and
    desired states stay bit-identical.  Config 2 runs with integral gains on."""
    tasks = W.make_inputs(cfg, 1)["tasks"]
    if cfg == 2:
        tasks = [dict(tasks[0], ki_pos=5.0, ki_ori=3.0), dict(tasks[1], ki=2.0)]
    a = _run_cycles(cfg, tasks, True)
    b = _run_cycles(cfg, tasks, False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("B", [1, 63, 65])
def test_odd_batch_sizes(B):
    d, robot, ctrl, objs = _controller(2, 256)
    full = _diag(objs[0])[:B]
    # the same first B instances in a batch of size B
    from sai_primitives_amd.controller import controller_from_specs
    robot2, ctrl2, objs2 = controller_from_specs(d["model"].name, d["tasks"], B, device=0)
    robot2.setQ(d["q"][:B])
    robot2.setDq(d["dq"][:B])
    robot2.updateModel()
    ctrl2.setGoals([g[:B] for g in d["goals"]])
    assert np.array_equal(_diag(objs2[0]), full)


def test_padded_leading_dimension_and_device_entry():
    """ld > B gives the same rows; the device entry writes [24][ld] into a caller buffer (allocated here through the HIP runtime the engine
    itself links) and agrees with the host entry without touching the padding columns"""
    import ctypes as C
    from sai_primitives_amd import capi
    d, robot, ctrl, objs = _controller(3, 200)
    ref = _diag(objs[0])
    d2, robot2, ctrl2, objs2 = _controller(3, 200, ld=320)
    assert capi.lib().saip_batch_ld(ctrl2._h) == 320
    assert np.array_equal(_diag(objs2[0]), ref)
    hip = C.CDLL("libamdhip64.so.7")
    nbytes = 24 * 320 * 8
    host = np.full((24, 320), np.nan)
    ptr = C.c_void_p()
    assert hip.hipMalloc(C.byref(ptr), C.c_size_t(nbytes)) == 0
    try:
        assert hip.hipMemcpy(ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(nbytes), 1) == 0   # hipMemcpyHostToDevice
        objs2[0].getTaskDiagnosticsDevice(ptr.value)
        ctrl2._call("saip_batch_synchronize")
        assert hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), ptr, C.c_size_t(nbytes), 2) == 0   # hipMemcpyDeviceToHost
    finally:
        hip.hipFree(ptr)
    assert np.array_equal(host[:, :200].T, ref)
    assert np.all(np.isnan(host[:, 200:]))  # the padding is not written


def test_cpp_facade_diagnostics(tmp_path):
    """tests/cpp/diagnostics_example.cpp runs one config-2 cycle through the C++ facade; its getters agree with the Python ones"""
    import sai_primitives_amd as sp
    sp.build_library()
    exe = str(tmp_path / "diagnostics_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "diagnostics_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    robot_file = _write_robot(tmp_path, "panda_arm")
    B = 128
    d, robot, ctrl, objs = _controller(2, B)
    blob = np.concatenate([d["q"].T, d["dq"].T, d["goals"][0].T, d["goals"][1].T], axis=0)
    inp, outp = tmp_path / "in.bin", tmp_path / "out.bin"
    np.ascontiguousarray(blob).tofile(inp)
    res = subprocess.run([exe, robot_file, "run", str(B), str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "DIAG_RUN_OK" in res.stdout, res.stdout + res.stderr
    got = np.fromfile(outp).reshape(-1, B)
    ctrl.updateControllerTaskModels()
    tau = ctrl.computeControlTorques()
    exp = _diag(objs[0]).T
    assert np.array_equal(got[:24], exp)                                   # getTaskDiagnostics
    assert np.array_equal(got[24:27], objs[0].getGoalPosition().T)          # getGoalPosition
    assert np.array_equal(got[27:30], objs[0].getDesiredPosition().T)       # getDesiredPosition
    reached = np.sqrt((exp[0:3] ** 2).sum(0)) < 0.05
    assert np.array_equal(got[30].astype(bool), reached)                   # goalPositionReached(0.05)
    assert np.array_equal(got[31:38], tau.T)                               # the cycle's torques


def _write_robot(tmp_path, name):
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
