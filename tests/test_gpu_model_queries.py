"""Robot-model queries (saip_model_frames_kernel / saip_model_dynamics_kernel through saip_batch_model_frames_* / saip_batch_model_dynamics_*,
the SaiModel accessors and RobotController.getModelFrames / getModelDynamics) against independent NumPy: workloads.fk / jacobian /
mass_matrix and oracle/restatement.gravity_vector / forward_dynamics."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOTS = ["panda_arm", "panda_sliding_base", "chain30"]
# per robot: (link, pos_in_link) frames of one call -- out of body order on purpose; the fixed end-effector links compose their transform
FRAMES = {"panda_arm": [("end-effector", (0.0, 0.0, 0.07)), ("link3", (0.1, -0.05, 0.02)), ("link1", None), ("end-effector", None)],
          "panda_sliding_base": [("link4", (0.03, 0.0, -0.1)), ("end-effector", (0.01, 0.02, 0.1)), ("link0", (0.2, 0.0, 0.0))],
          "chain30": [("link30", (0.0, 0.0, 0.1)), ("link7", None), ("link18", (0.05, 0.05, 0.0))]}
T_BASE = np.array([[0.0, -0.8, 0.6, 0.5], [1.0, 0.0, 0.0, -0.25], [0.0, 0.6, 0.8, 0.1], [0, 0, 0, 1]])


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _close(a, b, tol):
    scale = max(1.0, float(np.max(np.abs(b))))
    return float(np.max(np.abs(a - b))) <= tol * scale, float(np.max(np.abs(a - b))) / scale


def _state(name, B, seed=7, zero_dq=False):
    m = W.load_robot(name)
    rng = np.random.default_rng(seed)
    q = rng.uniform(np.maximum(m.q_lower, -2.5), np.minimum(m.q_upper, 2.5), size=(B, m.dof))
    dq = np.zeros((B, m.dof)) if zero_dq else rng.uniform(-1.0, 1.0, size=(B, m.dof))
    return m, q, dq


def _robot(sp, name, B, q, dq, desc=None):
    robot = sp.SaiModel(desc if desc is not None else name, B, device=0)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    return robot


def _expected_frame(m, frames, li, pos):
    R, o = frames[li]
    p = o + R @ np.zeros(3) if pos is None else o + R @ np.asarray(pos, float)
    return p, R, W.jacobian(m, frames, li, p)


@pytest.mark.parametrize("name", ROBOTS)
def test_frames_match_numpy(sp, name):
    B = 65
    m, q, dq = _state(name, B)
    robot = _robot(sp, name, B, q, dq)
    frames = W.fk(m, q)
    fr = FRAMES[name]
    out = robot._frames(fr, sp.SAIP_QUERY_JACOBIAN)
    assert out.shape == (len(fr), 18 + 6 * m.dof, B)
    for k, (link, pos) in enumerate(fr):
        p, R, J = _expected_frame(m, frames, m.link_index(link), pos)
        r = out[k]
        for got, want, what in [(r[0:3].T, p, "position"), (r[3:12].T.reshape(B, 3, 3), R, "rotation"),
                                (r[18:].T.reshape(B, 6, m.dof), J, "jacobian")]:
            ok, err = _close(got, want, 1e-12)
            assert ok, (name, link, what, err)
        Jg = r[18:].T.reshape(B, 6, m.dof)
        ok, err = _close(np.concatenate([r[12:15].T, r[15:18].T], 1), np.einsum("bij,bj->bi", Jg, dq), 1e-12)
        assert ok, (name, link, "twist", err)
    # the accessors are slices of the same rows; links by index as well
    link, pos = fr[0]
    li = m.link_index(link)
    assert np.array_equal(robot.position(link, pos), out[0, 0:3].T)
    assert np.array_equal(robot.position(li, pos), out[0, 0:3].T)
    assert np.array_equal(robot.rotation(link), out[0, 3:12].T.reshape(B, 3, 3))
    assert np.array_equal(robot.J(link, pos), out[0, 18:].T.reshape(B, 6, m.dof))
    assert np.array_equal(robot.Jv(link, pos), robot.J(link, pos)[:, :3])
    assert np.array_equal(robot.Jw(link), robot.J(link)[:, 3:])
    assert np.array_equal(robot.linearVelocity(link, pos), out[0, 12:15].T)
    assert np.array_equal(robot.angularVelocity(link), out[0, 15:18].T)
    T = robot.transform(link, pos)
    assert np.array_equal(T[:, :3, 3], out[0, 0:3].T) and np.array_equal(T[:, :3, :3], robot.rotation(link))
    assert np.all(T[:, 3] == [0, 0, 0, 1])


def test_link_welded_to_the_base(sp):
    desc = sp.load_robot_description("panda_arm")
    desc = dict(desc, links=[dict(desc["links"][0], name="mount", joint_type="fixed", mass=2.0, origin_xyz=[0.1, 0.0, 0.2],
                                  origin_rpy=[0.0, 0.0, 0.5])] + list(desc["links"]))
    m = W.RobotModel(desc)
    B = 33
    _, q, dq = _state("panda_arm", B)
    robot = _robot(sp, None, B, q, dq, desc=desc)
    out = robot._frames([("link2", (0, 0.1, 0)), ("mount", (0.0, 0.3, 0.0))], sp.SAIP_QUERY_JACOBIAN)
    frames = W.fk(m, q)
    p, R, J = _expected_frame(m, frames, 0, (0.0, 0.3, 0.0))
    assert np.all(J == 0) and np.all(out[1, 12:] == 0)  # constant pose, zero twist, all-zero Jacobian
    assert _close(out[1, 0:3].T, p, 1e-14)[0] and _close(out[1, 3:12].T.reshape(B, 3, 3), R, 1e-14)[0]
    p, R, J = _expected_frame(m, frames, 2, (0, 0.1, 0))
    assert _close(out[0, 0:3].T, p, 1e-12)[0] and _close(out[0, 18:].T.reshape(B, 6, 7), J, 1e-12)[0]


@pytest.mark.parametrize("name", ROBOTS)
def test_world_rows_are_mapped_base_rows(sp, name):
    B = 40
    m, q, dq = _state(name, B, seed=3)
    robot = _robot(sp, name, B, q, dq)
    fr = FRAMES[name]
    base = robot._frames(fr, sp.SAIP_QUERY_JACOBIAN)
    robot.setTRobotBase(T_BASE)
    assert np.array_equal(robot._frames(fr, sp.SAIP_QUERY_JACOBIAN), base)  # the base-frame rows ignore the base
    world = robot._frames(fr, sp.SAIP_QUERY_JACOBIAN | sp.SAIP_QUERY_WORLD)
    Rw, pw = T_BASE[:3, :3], T_BASE[:3, 3]
    n = m.dof
    for k in range(len(fr)):
        b, w = base[k], world[k]
        want = np.concatenate([Rw @ b[0:3] + pw[:, None], np.einsum("ik,kjb->ijb", Rw, b[3:12].reshape(3, 3, B)).reshape(9, B),
                               Rw @ b[12:15], Rw @ b[15:18], np.einsum("ik,kjb->ijb", Rw, b[18:18 + 3 * n].reshape(3, n, B)).reshape(3 * n, B),
                               np.einsum("ik,kjb->ijb", Rw, b[18 + 3 * n:].reshape(3, n, B)).reshape(3 * n, B)])
        ok, err = _close(w, want, 1e-12)
        assert ok, (name, k, err)
    link, pos = fr[0]
    assert np.array_equal(robot.positionInWorld(link, pos), world[0, 0:3].T)
    assert np.array_equal(robot.linearVelocityInWorld(link, pos), world[0, 12:15].T)
    assert np.array_equal(robot.JWorldFrame(link, pos), world[0, 18:].T.reshape(B, 6, n))
    assert np.array_equal(robot.transformInWorld(link, pos)[:, :3, 3], world[0, 0:3].T)


@pytest.mark.parametrize("name", ROBOTS)
def test_dynamics_match_numpy(sp, name):
    import restatement as RS
    B = 65 if name != "chain30" else 8
    m, q, dq = _state(name, B, seed=11)
    robot = _robot(sp, name, B, q, dq)
    frames = W.fk(m, q)
    M, Minv, g, b = robot.M(), robot.MInv(), robot.jointGravityVector(), robot.coriolisForce()
    Mref = W.mass_matrix(m, frames)
    assert _close(M, Mref, 1e-12)[0], _close(M, Mref, 1e-12)[1]
    ok, err = _close(np.einsum("bij,bjk->bik", M, Minv), np.broadcast_to(np.eye(m.dof), M.shape), 1e-10)
    assert ok, err
    gref = RS.gravity_vector(m, frames)
    assert _close(g, gref, 1e-12)[0], _close(g, gref, 1e-12)[1]
    # b = C(q, dq) dq: the Lagrangian expression of forward_dynamics with tau = 0 and no gravity is qdd = -M^-1 b
    qdd0 = RS.forward_dynamics(m, q, dq, np.zeros_like(q), g=(0.0, 0.0, 0.0))
    bref = -np.einsum("bij,bj->bi", Mref, qdd0)
    ok, err = _close(b, bref, 1e-8)
    assert ok, err
    # M^-1 (tau - b - g) is the forward dynamics
    tau = np.random.default_rng(5).uniform(-20, 20, size=q.shape)
    ok, err = _close(np.einsum("bij,bj->bi", Minv, tau - b - g), RS.forward_dynamics(m, q, dq, tau), 1e-8)
    assert ok, err
    # b vanishes exactly at rest
    robot.setDq(np.zeros_like(dq))
    robot.updateModel()
    assert np.all(robot.coriolisForce() == 0.0)
    assert np.array_equal(robot.jointGravityVector(), g) and np.array_equal(robot.M(), M)


def test_gravity_vector_is_what_gravity_compensation_adds(sp):
    from sai_primitives_amd.controller import controller_from_specs
    B = 64
    d = W.make_inputs(2, B)
    taus = []
    for gc in (False, True):
        robot, ctrl, _ = controller_from_specs(d["model"].name, d["tasks"], B, device=0)
        ctrl.enableGravityCompensation(gc)
        robot.setQ(d["q"])
        robot.setDq(d["dq"])
        robot.updateModel()
        ctrl.updateControllerTaskModels()
        ctrl.setGoals(d["goals"])
        taus.append(ctrl.computeControlTorques())
        assert ctrl.status.sum() == 0
    g = robot.jointGravityVector()
    ok, err = _close(taus[1] - taus[0], g, 1e-9)
    assert ok, err
    assert np.array_equal(ctrl.getModelDynamics()["g"], g)


def _run_cycles(ctrl, robot, d, k, between=None):
    res = []
    for i in range(k):
        ctrl.updateControllerTaskModels()
        tau = ctrl.computeControlTorques()
        res.append((tau, ctrl.status.copy()))
        if between:
            between()
        robot.setQ(d["q"] + 1e-3 * (i + 1))
        robot.updateModel()
    return res


@pytest.mark.parametrize("cfg,otg", [(2, False), (9, True)])
def test_queries_leave_the_cycle_unchanged(sp, cfg, otg):
    from sai_primitives_amd.controller import controller_from_specs
    B = 96
    d = W.make_inputs(cfg, B)
    runs = []
    for interleave in (False, True):
        robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, disable_otg=not otg)
        robot.setQ(d["q"])
        robot.setDq(d["dq"])
        robot.updateModel()
        ctrl.setGoals(d["goals"])
        if interleave:
            robot.setTRobotBase(T_BASE)  # no torque depends on the base

        def queries():
            ctrl.getModelFrames(["end-effector", ("link4", (0.1, 0, 0))], jacobian=True, world=True)
            ctrl.getModelDynamics()
            robot.M()
            robot.positionInWorld("end-effector")
        runs.append(_run_cycles(ctrl, robot, d, 4, queries if interleave else None))
    for (t0, s0), (t1, s1) in zip(*runs):
        assert np.array_equal(t0, t1, equal_nan=True) and np.array_equal(s0, s1)


def test_pose_bitwise_equal_to_the_pose_readback(sp):
    from sai_primitives_amd.controller import controller_from_specs
    B = 65
    d = W.make_inputs(2, B)
    robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0)
    robot.setQ(d["q"])
    robot.setDq(d["dq"])
    robot.updateModel()
    mf = [t for t in objs if t.getTaskType() == 3][0]
    spec = [t for t in d["tasks"] if t["type"] == "motion_force"][0]
    assert np.array_equal(np.asarray(spec["rot_in_link"]), np.eye(3))
    pos, rot = mf.getCurrentPosition(), mf.getCurrentOrientation()
    out = ctrl.getModelFrames([(spec["link"], tuple(spec["pos_in_link"]))], jacobian=True)
    assert np.array_equal(out[0, 0:3].T, pos) and np.array_equal(out[0, 3:12].T.reshape(B, 3, 3), rot)
    assert np.array_equal(robot.position(spec["link"], spec["pos_in_link"]), pos)


def test_resident_state_after_rollout(sp):
    from sai_primitives_amd.controller import controller_from_specs
    B = 64
    d = W.make_inputs(2, B)
    robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0)
    robot.setQ(d["q"])
    robot.setDq(d["dq"])
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    ctrl.setGoals(d["goals"])
    ctrl.rolloutAsync(5, 0.001)
    frames = ctrl.getModelFrames([("end-effector", (0, 0, 0.07))], jacobian=True)
    dyn = ctrl.getModelDynamics()
    n = d["model"].dof
    L = sp.lib()
    q, dq = np.empty((n, B)), np.empty((n, B))
    from sai_primitives_amd.controller import _dptr
    assert L.saip_batch_get_state_host(ctrl._h, _dptr(q), _dptr(dq)) == 0
    q, dq = q.T, dq.T
    assert not np.allclose(q, d["q"])  # the rollout moved the state
    m = d["model"]
    fr = W.fk(m, q)
    p, R, J = _expected_frame(m, fr, m.link_index("end-effector"), (0, 0, 0.07))
    assert _close(frames[0, 0:3].T, p, 1e-12)[0] and _close(frames[0, 18:].T.reshape(B, 6, n), J, 1e-12)[0]
    assert _close(frames[0, 12:18].T, np.einsum("bij,bj->bi", J, dq), 1e-12)[0]
    assert _close(dyn["M"], W.mass_matrix(m, fr), 1e-12)[0]


class _DevBuf:
    """a (rows, ld) float64 device array filled with 7.0 (hipMalloc through ctypes, as the engine's own runtime)"""
    def __init__(self, rows, ld):
        self.hip = C.CDLL("libamdhip64.so.7")
        self.shape = (rows, ld)
        self.nbytes = rows * ld * 8
        self.ptr = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(self.ptr), C.c_size_t(self.nbytes)) == 0
        host = np.full(self.shape, 7.0)
        assert self.hip.hipMemcpy(self.ptr, host.ctypes.data_as(C.c_void_p), C.c_size_t(self.nbytes), 1) == 0

    def numpy(self):
        host = np.empty(self.shape)
        assert self.hip.hipMemcpy(host.ctypes.data_as(C.c_void_p), self.ptr, C.c_size_t(self.nbytes), 2) == 0
        return host

    def free(self):
        self.hip.hipFree(self.ptr)


@pytest.mark.parametrize("B,ld", [(1, None), (63, None), (65, None), (65, 160)])
def test_sizes_and_device_flavours(sp, B, ld):
    from sai_primitives_amd.controller import controller_from_specs
    d = W.make_inputs(2, B)
    robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, leading_dimension=ld)
    robot.setQ(d["q"])
    robot.setDq(d["dq"])
    robot.updateModel()
    L = sp.lib()
    ldv = L.saip_batch_ld(ctrl._h)
    assert ld is None or ldv == ld
    n = d["model"].dof
    fr = [("end-effector", (0, 0, 0.07)), ("link2", None)]
    rows = 18 + 6 * n
    host = ctrl.getModelFrames(fr, jacobian=True, world=True)
    hd = ctrl.getModelDynamics()
    bufs = [_DevBuf(2 * rows, ldv)] + [_DevBuf(n * n if k in ("M", "M_inv") else n, ldv) for k in ("M", "M_inv", "g", "b", "g")]
    try:
        ctrl.getModelFrames(fr, jacobian=True, world=True, out=bufs[0].ptr.value)
        ctrl.getModelDynamics(out={k: bf.ptr.value for k, bf in zip(("M", "M_inv", "g", "b"), bufs[1:5])})
        ctrl.getModelDynamics(out={"g": bufs[5].ptr.value})  # only what is asked for is written
        assert L.saip_batch_synchronize(ctrl._h) == 0
        dv = bufs[0].numpy().reshape(2, rows, ldv)
        assert np.array_equal(dv[:, :, :B], host) and np.all(dv[:, :, B:] == 7.0)
        for k, bf in zip(("M", "M_inv", "g", "b", "g"), bufs[1:]):
            a = bf.numpy()
            assert np.array_equal(a[:, :B], hd[k].reshape(B, -1).T), k
            assert np.all(a[:, B:] == 7.0), k
    finally:
        for bf in bufs:
            bf.free()
    m = d["model"]
    p, R, J = _expected_frame(m, W.fk(m, d["q"]), m.link_index("end-effector"), (0, 0, 0.07))
    assert _close(host[0, 0:3].T, p, 1e-12)[0]  # identity base: the world rows are the base-frame rows


def test_facade_reflects_the_last_update_model(sp):
    B = 17
    m, q, dq = _state("panda_arm", B)
    robot = _robot(sp, "panda_arm", B, q, dq)
    p0, M0 = robot.position("end-effector"), robot.M()
    robot.setQ(q + 0.3)  # not followed by updateModel(): the queries keep answering for q
    assert np.array_equal(robot.position("end-effector"), p0) and np.array_equal(robot.M(), M0)
    robot.updateModel()
    p1 = robot.position("end-effector")
    want = _expected_frame(m, W.fk(m, q + 0.3), m.link_index("end-effector"), None)[0]
    assert _close(p1, want, 1e-12)[0] and not np.allclose(p1, p0)


def test_model_only_batch_on_the_device(sp):
    from sai_primitives_amd import capi
    robot = _robot(sp, "panda_arm", 8, *_state("panda_arm", 8)[1:])
    robot.M()
    L = sp.lib()
    h = robot._mq
    assert L.saip_batch_step_async(h) == capi.SAIP_ERR_ORDER
    assert L.saip_batch_integrate(h, 0.001, 1, None, 0.0) == capi.SAIP_ERR_ORDER
    assert L.saip_batch_rollout_async(h, 1, 0.001, 1, None, 0.0) == capi.SAIP_ERR_ORDER
    ms = C.c_double()
    assert L.saip_batch_time_steps(h, 2, 1, C.byref(ms)) == capi.SAIP_ERR_ORDER
    assert L.saip_batch_synchronize(h) == capi.SAIP_OK


def test_cpp_example_runs(sp, tmp_path):
    import test_model_queries_cpu as T
    exe = T.build_example(tmp_path)
    B = 65
    m, q, dq = _state("panda_arm", B, seed=2)
    inp = tmp_path / "in.bin"
    np.concatenate([q.T.ravel(), dq.T.ravel()]).tofile(inp)
    outp = tmp_path / "out.bin"
    r = subprocess.run([exe, T._robot_file(tmp_path), "run", str(B), str(inp), str(outp)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "MQ_RUN_OK" in r.stdout, r.stdout + r.stderr
    out = np.fromfile(outp).reshape(-1, B)
    n = m.dof
    p, R, J = _expected_frame(m, W.fk(m, q), m.link_index("end-effector"), (0, 0, 0.07))
    assert _close(out[0:3].T, p, 1e-12)[0] and _close(out[3:12].T.reshape(B, 3, 3), R, 1e-12)[0]
    assert _close(out[24:24 + 6 * n].T.reshape(B, 6, n), J, 1e-12)[0]
    assert _close(out[24 + 6 * n:24 + 6 * n + n * n].T.reshape(B, n, n), W.mass_matrix(m, W.fk(m, q)), 1e-12)[0]
    assert np.all(np.isfinite(out))
