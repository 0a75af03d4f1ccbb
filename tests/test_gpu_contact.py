"""Contact planes and the simulated force sensor on the device (csrc/saip_contact.hip, saip_batch_contact_*).  Oracles: the NumPy
restatement tests/contact_ref.py of the contact arithmetic, the engine's own model queries (pose, twist, Jacobian of the contact point),
the plain integrator given the same torques, and the host-driven loop { contactSense, cycle, integrate } for whole rollouts.

Batches B in {3, 65, 130} (a partial wavefront, a block edge, more than one block) at a padded leading dimension, torques in a
caller-bound buffer."""
import ctypes as C

import numpy as np
import pytest

import chains as CH
import contact_ref as CR
import trees as TR
import workloads as W
from test_gpu_batch_layout import _DevBuf, _d2h, _same_bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SHAPES = [(3, 64), (65, 128), (130, 192)]          # (B, leading dimension)
DT, SUB = 5e-4, 2
ZERO_G = (0.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _bind_tau(ctrl, n, ld, values=None):
    """a caller-owned torque buffer (n, ld), bound; the padding columns hold a sentinel nothing may touch"""
    host = np.full((n, ld), 6.02214076e23)
    B = ctrl.batch_size
    host[:, :B] = 0.0 if values is None else values.T
    buf = _DevBuf(host)
    ctrl.bindTauDevice(buf.ptr)
    return buf


def _tau_sim(ctrl, mf, n, ld):
    ctrl.synchronize()
    return _d2h(mf.contactTorquesDevice(), (n, ld))


# ------------------------------------------------------------------ 1. drop test
def _slider(mass):
    """a vertical slider (prismatic z) that carries a horizontal one (prismatic x): the smallest chain that can carry a motion-force task
    (the engine refuses rank-1 tasks, so a 1-dof chain has nothing to attach a contact to).  The horizontal joint stays at rest and the
    mass matrix is diagonal, so the vertical motion is that of one body of the total mass."""
    ine = [0.01, 0.01, 0.01, 0, 0, 0]
    return dict(name="slider2", links=[CH._link("link1", "prismatic", [0, 0, 0], [0, 0, 0], [0, 0, 1], 0.75 * mass, [0, 0, 0], ine, -5.0, 5.0, 1e3),
                                       CH._link("link2", "prismatic", [0, 0, 0], [0, 0, 0], [1, 0, 0], 0.25 * mass, [0, 0, 0], ine, -5.0, 5.0, 1e3)])


@pytest.mark.parametrize("B,ld", SHAPES)
def test_drop_on_a_plane(sp, B, ld):
    """a vertical slider of mass m released on z = 0 with critical damping c = 2 sqrt(k m): every period against the NumPy
    restatement of the same semi-implicit stepping, then the rest state d = -m g / k, f_n = m g"""
    from sai_primitives_amd.controller import controller_from_specs
    m, k, g = 2.0, 1.0e4, 9.81
    c = 2.0 * np.sqrt(k * m)
    om = np.sqrt(k / m)
    dts = DT / 2                                    # the substep
    tasks = [W.motion_force_task("tip", "link2", (0, 0, 0), dirs_trans=[[0, 0, 1], [1, 0, 0]], dirs_rot=None)]
    robot, ctrl, objs = controller_from_specs(_slider(m), tasks, B, device=0, leading_dimension=ld)
    h0 = np.linspace(0.0, 2e-3, B)                  # instance i starts h0[i] above the plane, at rest
    robot.setQ(np.column_stack([h0, np.zeros(B)]))
    robot.setDq(np.zeros((B, 2)))
    robot.updateModel()
    with _bind_tau(ctrl, 2, ld) as buf:             # commanded torque 0: free fall onto the plane
        objs[0].attachContactPlanes(CR.plane([0, 0, 1], 0.0, k, c, 0.5, 1e-3)[None], sensor=False)
        q, dq = h0.copy(), np.zeros(B)
        checked, total = 40, 840
        S = checked * SUB
        hist = []
        for period in range(checked):
            for _ in range(SUB):                    # the restatement: contact force at the state, then one semi-implicit Euler substep
                p = np.column_stack([np.zeros(B), np.zeros(B), q])
                v = np.column_stack([np.zeros(B), np.zeros(B), dq])
                f, fn, dmin, act = CR.plane_forces(CR.plane([0, 0, 1], 0.0, k, c, 0.5, 1e-3)[None], p, v)
                last = (f.copy(), p.copy(), dmin.copy(), act.copy())
                ddq = (f[:, 2] - m * g) / m
                dq = dq + dts * ddq
                q = q + dts * dq
                hist.append((np.abs(q).max(), np.abs(dq).max(), np.abs(ddq).max(), np.abs(f).max()))
            ctrl.integrate(dts, SUB)
            gq, gdq = ctrl.pullState()
            ro = objs[0].contactReadout()
            # per substep the device and the restatement differ by a few roundings: <= 8 eps on q, on dq and on dt * ddq.  In the energy
            # norm (om dq_err is to q_err what dq is to q) the contact dynamics do not amplify them, in free flight q_err grows by dt * dq_err
            # per step: after S substeps dq_err <= S inj, q_err <= S inj (1 / om + S dt)
            hq, hdq, hdd, hf = (max(h[i] for h in hist) for i in range(4))
            s = (period + 1) * SUB
            inj = 8 * EPS * (om * hq + hdq + dts * hdd)
            b_dq = s * inj
            b_q = s * inj * (1.0 / om + s * dts)
            assert np.abs(gq[:, 0] - q).max() <= b_q, (period, np.abs(gq[:, 0] - q).max(), b_q)
            assert np.abs(gdq[:, 0] - dq).max() <= b_dq, (period, np.abs(gdq[:, 0] - dq).max(), b_dq)
            # the readout is of the period's LAST contact launch (the state in front of the last substep)
            b_f = k * b_q + c * b_dq + 8 * EPS * hf
            edge = np.abs(last[2]) <= b_q           # an instance within rounding of d = 0 may be on either side
            assert (np.abs(ro["force"] - last[0]).max(axis=1)[~edge] <= b_f).all(), period
            assert np.abs(ro["point"] - last[1]).max() <= b_q and (np.abs(ro["distance"] - last[2]) <= b_q).all()
            assert np.array_equal(ro["active"][~edge], last[3][~edge])
        for _ in range(total - checked):
            ctrl.integrate(dts, SUB)
        gq, gdq = ctrl.pullState()
        ro, sm = objs[0].contactReadout(), objs[0].contactSummary()
        # critically damped: with a = om dt the semi-implicit step has the characteristic polynomial z^2 - (2 - 2a - a^2) z + (1 - 2a), whose
        # discriminant a^3 (a + 4) splits the double root of the continuous system into two real ones; the slow one is
        # 1 - a - a^2/2 + a^1.5 sqrt(1 + a/4) <= exp(-a (1 - 1.01 sqrt(a) - a)).  With two real roots z2 < z1 the residual after n steps is
        # at most z1^n (|x0| + n |x1 - z2 x0| / z1), and one step moves x by less than 2 a |x0| + dt |v0|: counted from a state no farther
        # than start = |h0| + 2 m g / k from rest with speeds below om * start, that is below 2 (1 + om T) z1^n start after the time T
        T = (total - checked) * SUB * dts
        a = om * dts
        start = 2e-3 + 2 * m * g / k
        resid = 2.0 * (1.0 + om * T) * np.exp(-om * T * (1.0 - 1.01 * np.sqrt(a) - a)) * start
        assert resid < 1e-9
        assert not gq[:, 1].any() and not gdq[:, 1].any()                                    # the horizontal joint never moved
        assert np.abs(gq[:, 0] + m * g / k).max() <= resid + b_q, np.abs(gq[:, 0] + m * g / k).max()
        assert np.abs(ro["force"][:, 2] - m * g).max() <= (k + c * om) * (resid + b_q) and not ro["force"][:, :2].any()
        assert (ro["active"] == 1).all() and (sm["substeps_in_contact"] > 0).all() and (sm["max_penetration"] >= m * g / k - (resid + b_q)).all()
        assert np.all(buf.get()[:, B:] == 6.02214076e23) and not buf.get()[:, :B].any()      # the commanded torques are never written
        objs[0].detachContactPlanes()


# ------------------------------------------------------------------ 2. torque path
def _model_case(name, B, ld, seed=5):
    """(robot, ctrl, task under contact, model, link, pos_in_link, the kernel family): a stack at a random state"""
    from sai_primitives_amd.controller import controller_from_specs
    rng = np.random.default_rng(seed)
    if name == "tree":
        desc = TR.dual_panda_torso()
        m = W.RobotModel(desc)
        specs, ti, link, pos = TR.dual_stack(m), 1, "right_link7", (0.0, 0.0, 0.1)      # the task on the second arm
    elif name == "puma6":
        desc = CH.puma_arm()
        m = W.RobotModel(desc)
        specs, ti, link, pos = [W.motion_force_task("hand", "link6", (0.05, 0.0, 0.02)), W.joint_task("posture")], 0, "link6", (0.05, 0.0, 0.02)
    else:
        cfg = {"panda_arm": 2, "chain30": 5}[name]
        d = W.make_inputs(cfg, B)
        desc, m, specs = d["model"].name, d["model"], d["tasks"]
        ti, link, pos = 0, specs[0]["link"], tuple(specs[0]["pos_in_link"])
    q = np.clip(rng.uniform(-1.2, 1.2, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    dq = rng.uniform(-0.5, 0.5, (B, m.dof))
    robot, ctrl, objs = controller_from_specs(desc, specs, B, device=0, leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    return robot, ctrl, objs[ti], m, link, pos


@pytest.mark.parametrize("name,B,ld", [("panda_arm", 65, 128), ("puma6", 3, 64), ("chain30", 130, 192), ("tree", 65, 128)])
def test_contact_torques_are_jacobian_transpose_times_force(sp, name, B, ld):
    robot, ctrl, mf, m, link, pos = _model_case(name, B, ld)
    n = m.dof
    rng = np.random.default_rng(9)
    rc = np.array([0.02, -0.01, 0.03])
    cp = tuple(np.asarray(pos) + rc)                  # the control frame is the link frame moved to `pos`: the contact point in the link
    p, v, Jv = robot.position(link, cp), robot.linearVelocity(link, cp), robot.Jv(link, cp)
    # two planes per instance through the neighbourhood of its point: instance i touches plane 0 when i % 3 != 2, plane 1 when i % 2
    nrm = rng.normal(size=(2, B, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    pen = np.stack([np.where(np.arange(B) % 3 != 2, 3e-3, -2e-3), np.where(np.arange(B) % 2 == 1, 1e-3, -5e-3)])
    planes = np.zeros((2, B, 8))
    planes[..., :3] = nrm
    planes[..., 3] = np.einsum("pbe,be->pb", nrm, p) + pen
    planes[..., 4:] = [1.0e3, 15.0, 0.6, 1e-2]
    tau_cmd = rng.uniform(-5, 5, (B, n))
    tau_cmd[B // 2] = np.nan                          # a flagged instance under the NaN policy
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    with _bind_tau(ctrl, n, ld, tau_cmd) as buf:
        mf.attachContactPlanes(planes, point=rc, sensor=False, per_instance=True)
        ctrl.integrate(DT, 1)
        sim = _tau_sim(ctrl, mf, n, ld)
        q1, dq1 = (a.copy() for a in ctrl.pullState())
        ro = mf.contactReadout()
        f, fn, dmin, act = CR.plane_forces(planes.transpose(1, 0, 2), p, v)
        assert np.array_equal(ro["active"], act) and set(act) == {0, 1, 2}
        want = np.einsum("bej,be->bj", Jv, f)
        scale = max(1.0, np.abs(want).max())
        base = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
        err = np.abs((sim[:, :B].T - base) - want).max() / scale
        print(f"{name}: max |tau_sim - tau_cmd - Jv^T f| = {err:.3e} of {scale:.3e}")
        assert err <= 1e-12                                              # the bound of test_gpu_model_queries.py on the Jacobians
        assert np.abs(ro["force"] - f).max() <= 1e-12 * max(1.0, np.abs(f).max()) and np.abs(ro["point"] - p).max() <= 1e-12
        assert not (sim[:, :B].T - base)[act == 0].any()                 # no plane acts: the torques pass through bit for bit
        assert not np.isnan(sim[:, :B]).any() and not sim[:, B:].any()   # columns B.. are never written (zero since the attach)
        if name == "tree":                                               # joints off the task's branch get no contact torque
            anc = np.zeros(n, bool)
            j = n - 1                                                    # right_link7 is the last movable body
            par = TR.joint_parents(m)
            while j >= 0:
                anc[j] = True
                j = par[j]
            assert anc.sum() == 8 and np.array_equal((sim[:, :B].T - base)[:, ~anc], np.zeros((B, (~anc).sum())))
            assert np.abs(want[:, ~anc]).max() == 0.0
        assert np.all(buf.get()[:, B:] == 6.02214076e23)
        mf.detachContactPlanes()
        # the same substep by the plain integrator given tau = tau_sim: the same bits
        robot.setQ(q0)
        robot.setDq(dq0)
        ctrl.bindTauDevice(0)
        ctrl.setTorques(sim[:, :B].T)
        ctrl.integrate(DT, 1)
        q2, dq2 = ctrl.pullState()
        assert _same_bits(q1, q2) and _same_bits(dq1, dq2)


# ------------------------------------------------------------------ config-13-like Panda stacks
def _cfg13(B, ld, otg, *, world_axis=False, goal_force=None):
    """config 13 (closed-loop force and moment control, passivity on) at rest; (robot, ctrl, objs)"""
    from sai_primitives_amd.controller import controller_from_specs
    d = W.make_inputs(13, B)
    specs = [dict(t) for t in d["tasks"]]
    if world_axis:
        specs[0].update(param_in_compliant_frame=False, force_axis=[0.0, 0.0, 1.0], moment_dim=0)
    robot, ctrl, objs = controller_from_specs(d["model"].name, specs, B, device=0, disable_otg=not otg, leading_dimension=ld)
    robot.setQ(d["q"])
    robot.setDq(np.zeros((B, 7)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    objs[0].enablePassivity()
    if goal_force is not None:
        objs[0].setGoalForce(np.broadcast_to(goal_force, (B, 3)))
        objs[0].setGoalMoment(np.zeros((B, 3)))
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs


def _table_under(robot, objs, depth, k=2.0e4, c=400.0, mu=0.3, rc=(0.0, 0.0, 0.0)):
    """per-instance planes z >= p_z + depth (normal +z): every instance starts `depth` inside"""
    B = robot.batch_size
    p = robot.position("end-effector", tuple(np.array([0, 0, 0.07]) + np.asarray(rc)))
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, k, c, mu, 1e-3]
    planes[0, :, 3] = p[:, 2] + depth
    return planes


def _final(ctrl, objs):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float), goals=[t._get_goal() for t in objs],
                summary=np.column_stack(list(objs[0].contactSummary().values())).astype(float),
                readout=np.column_stack([objs[0].contactReadout()[k].reshape(ctrl.batch_size, -1) for k in ("force", "point", "distance")]))


# ------------------------------------------------------------------ 3. sensor round trip
@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_sensor_round_trip(sp, B, ld):
    robot, ctrl, objs = _cfg13(B, ld, False)         # R_cs a rotation about z by 0.4 rad, t_cs = (0.01, -0.02, 0.05)
    mf = objs[0]
    rc = (0.01, 0.02, -0.015)
    with _bind_tau(ctrl, 7, ld):
        mf.attachContactPlanes(_table_under(robot, objs, 2e-3, rc=rc), point=rc, sensor=True, per_instance=True)
        ctrl.contactSense()
        ro = mf.contactReadout()
        xc = robot.position("end-effector", (0, 0, 0.07))
        F = -ro["force"]
        M = np.cross(ro["point"] - xc, F)
        assert (ro["active"] == 1).all() and (F[:, 2] < -30.0).all()          # k d = 40 N
        fw, mw = mf.getSensedForceControlWorldFrame(), mf.getSensedMomentControlWorldFrame()
        # two rotations there and two back, each orthonormal to a few eps, plus the lever arms: a few tens of eps of the magnitudes
        # (tests/test_contact_cpu.py derives 32 eps for the restatement; the device's x_c differs from the queried one by ~1e-16)
        assert np.abs(fw - F).max() <= 64 * EPS * np.abs(F).max()
        assert np.abs(mw - M).max() <= 64 * EPS * (np.abs(M).max() + 0.06 * np.abs(F).max())
        assert np.abs(M).max() > 0.1
        mf.detachContactPlanes()


# ------------------------------------------------------------------ 4. rollout vs host-driven loop
@pytest.mark.parametrize("otg,sched,rec,sub,B,ld", [(False, False, False, 2, 65, 128), (True, False, False, 2, 65, 128), (False, True, True, 1, 3, 64),
                                                    (True, True, True, 2, 130, 192), (False, False, True, 1, 130, 192)])
def test_rollout_equals_the_host_driven_loop(sp, otg, sched, rec, sub, B, ld):
    K = 20
    runs = []
    for host in (False, True):
        robot, ctrl, objs = _cfg13(B, ld, otg)
        mf = objs[0]
        buf = _bind_tau(ctrl, 7, ld)
        mf.attachContactPlanes(_table_under(robot, objs, 2e-3), sensor=True, per_instance=True)
        if sched:
            g = mf._get_goal()[:, :3]
            keys = g[None] + np.linspace(0.0, 0.01, 3)[:, None, None] * np.array([1.0, -1.0, 0.0])
            mf.setGoalSchedule((0, 3), keys, stride=4, mode="linear")
        if rec:
            ctrl.recordRollouts(K, 1, ("q", "tau"), task=mf, summaries=True)
        if not host:
            ctrl.rolloutAsync(K, DT, sub, gravity=ZERO_G)
        elif sched or rec:                           # schedules and the recorder act inside rollouts only: one period per call
            for _ in range(K):
                ctrl.rolloutAsync(1, DT, sub, gravity=ZERO_G)
        else:
            for _ in range(K):
                ctrl.contactSense()
                ctrl.stepAsync()
                ctrl.integrate(DT, sub, gravity=ZERO_G)
        out = _final(ctrl, objs)
        if rec:
            out["log"] = ctrl.rolloutLog()["tau"]
            out["rsum"] = ctrl.rolloutSummary()
        out["tau_buf"] = buf.get()
        runs.append(out)
        mf.detachContactPlanes()
        ctrl.bindTauDevice(0)
        buf.free()
    a, b = runs
    for key in a:
        if key == "goals":
            assert all(_same_bits(x, y) for x, y in zip(a[key], b[key]))
        else:
            assert _same_bits(np.asarray(a[key]), np.asarray(b[key])), key
    assert (a["summary"][:, 3] >= 1).all() and np.isfinite(a["q"]).all()            # every instance starts inside the table
    assert np.abs(a["goals"][0][:, 30:33]).max() > 1.0                               # the sensor wrote the sensed force
    if rec:
        assert _same_bits(a["log"][-1], a["tau"])                                    # the recorder logs the commanded torques


# ------------------------------------------------------------------ 5. per-instance planes
def test_per_instance_planes_and_flagged_instances(sp):
    res = {}
    for B, ld in [(3, 64), (130, 192)]:
        robot, ctrl, objs = _cfg13(B, ld, False)
        robot.setQ(np.broadcast_to(robot._q[0], (B, 7)).copy())      # the same posture everywhere: only the planes differ
        robot.updateModel()
        ctrl.reinitializeTasks()
        ctrl.updateControllerTaskModels()
        mf = objs[0]
        planes = _table_under(robot, objs, 2e-3)
        touch = np.arange(B) % 3 != 1                                # instance 1, 4, 7, ... have the table 5 cm below
        planes[0, ~touch, 3] -= 0.052
        tau = np.zeros((B, 7))
        tau[2] = np.nan                                              # instance 2 touches and carries NaN torques
        with _bind_tau(ctrl, 7, ld, tau):
            mf.attachContactPlanes(planes, sensor=False, per_instance=True)
            for _ in range(4):
                ctrl.integrate(DT, 1, gravity=ZERO_G)
            out = _final(ctrl, objs)
            mf.detachContactPlanes()
        ctrl.bindTauDevice(0)
        assert np.array_equal(out["summary"][:, 3] > 0, touch)
        assert not np.ptp(out["q"][~touch], axis=0).any() and not out["dq"][~touch].any()      # untouched, torque-free, no gravity: at rest
        vz = np.einsum("bej,bj->be", robot.Jv("end-effector", (0, 0, 0.07)), out["dq"])[:, 2]
        assert (vz[touch] > 0).all() and vz[2] > 0                   # pushed away from the plane, the NaN instance included
        res[B] = out
    for key in ("q", "dq", "summary", "readout"):
        assert _same_bits(res[3][key], res[130][key][:3]), key


# ------------------------------------------------------------------ 6. lifecycle
def test_lifecycle(sp):
    B, ld, K = 65, 128, 6
    robot, ctrl, objs = _cfg13(B, ld, True)
    mf, jt = objs
    planes = _table_under(robot, objs, 2e-3)
    with pytest.raises(ValueError, match="not a motion-force task"):
        ctrl._call("saip_batch_contact_attach", jt._id, None, 1, planes.ctypes.data_as(C.POINTER(C.c_double)), 1, 1)
    mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    with pytest.raises(sp.SaipError, match="already attached"):
        mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    with pytest.raises(sp.SaipError, match="written by the simulated sensor"):
        mf.setGoalSchedule("sensed_force", np.zeros((2, 3)))
    mf.setGoalSchedule("position", mf._get_goal()[None, :, :3])      # rows 0..2 do not collide
    mf.clearGoalSchedule()
    info = mf.contactInfo()
    assert (info["n_planes"], info["per_instance"], info["sensor"]) == (1, True, True)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    s1 = mf.contactSummary()
    assert (s1["substeps_in_contact"] >= 1).all() and (s1["impulse"] > 0).all() and (s1["max_penetration"] >= 2e-3 * (1 - 1e-9)).all()
    mf.resetContactSummary()
    lower = planes.copy()
    lower[0, :, 3] -= 0.5                                            # the table far below: nothing touches from the next period on
    mf.setContactPlanes(lower)
    ctrl.rolloutAsync(2, DT, SUB, gravity=ZERO_G)
    s2 = mf.contactSummary()
    assert not s2["substeps_in_contact"].any() and not s2["impulse"].any() and not s2["max_force"].any()
    assert not mf.contactReadout()["active"].any()
    mf.detachContactPlanes()
    assert mf.contactPlanesDevice() is None and mf.contactTorquesDevice() is None
    with pytest.raises(sp.SaipError, match="no contact planes are attached"):
        mf.contactReadout()
    # a schedule over the sensed rows first, then a sensor-writing contact: refused; without the sensor: fine
    mf.setGoalSchedule("sensed_force", np.zeros((2, 3)))
    with pytest.raises(sp.SaipError, match="covers sensed-wrench rows"):
        mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    mf.attachContactPlanes(planes, sensor=False, per_instance=True)
    with pytest.raises(sp.SaipError, match="without the simulated sensor"):
        ctrl.contactSense()
    mf.detachContactPlanes()
    mf.clearGoalSchedule()
    mf.attachContactPlanes(planes[:, 0], sensor=True)                # re-attach, batch-uniform this time
    assert mf.contactInfo()["per_instance"] is False
    mf.detachContactPlanes()
    # attach, detach, then a rollout: the bits of a batch that never had a contact
    ends = []
    for touched in (False, True):
        robot2, ctrl2, objs2 = _cfg13(B, ld, True)
        if touched:
            objs2[0].attachContactPlanes(planes, sensor=True, per_instance=True)
            objs2[0].detachContactPlanes()
        ctrl2.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        ctrl2.synchronize()
        q, dq = ctrl2.pullState()
        ends.append((q.copy(), dq.copy(), ctrl2.getTorques(), ctrl2.kernelName()))
    assert all(_same_bits(x, y) for x, y in zip(ends[0][:3], ends[1][:3])) and ends[0][3] == ends[1][3]


# ------------------------------------------------------------------ 7. behaviour
@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_force_task_presses_on_the_table(sp, B, ld):
    """goal force 5 N along the plane normal with config 13's closed-loop force gains: signs and inequalities only"""
    k = 2.0e4
    robot, ctrl, objs = _cfg13(B, ld, False, world_axis=True, goal_force=(0.0, 0.0, -5.0))      # the robot presses down on a table facing up
    mf = objs[0]
    mf.attachContactPlanes(_table_under(robot, objs, 1e-4, k=k), sensor=True, per_instance=True)
    ctrl.rolloutAsync(400, DT, SUB, gravity=ZERO_G)
    out = _final(ctrl, objs)
    ro, sm = mf.contactReadout(), mf.contactSummary()
    print("f_z min/max", ro["force"][:, 2].min(), ro["force"][:, 2].max(), "penetration max", -ro["distance"].min(), "status", out["status"].sum())
    assert (ro["active"] == 1).all()
    assert (ro["force"][:, 2] > 0).all()
    assert (-ro["distance"] < 2 * 5.0 / k).all()
    assert not out["status"].any()
    assert all(np.isfinite(out[key]).all() for key in ("q", "dq", "tau", "summary", "readout"))
    mf.detachContactPlanes()
