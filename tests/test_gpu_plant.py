"""The plant model of the resident simulator on the device (csrc/saip_plant.hip, saip_batch_plant_*).  Oracles: the NumPy restatement
tests/plant_ref.py of the joint arithmetic and of the random draw (bit for bit: no kinematics in them), the engine's own model queries
(Jacobian and rotation of the application site) for the wrenches, the plain integrator given the same torques, the NumPy restatement of
the semi-implicit stepping for a stop and for friction, and the host-driven loop { sense, cycle, integrate } for whole rollouts.

Batches B in {3, 65, 130} (a partial wavefront, a block edge, more than one block) at a padded leading dimension, torques in a
caller-bound buffer whose padding columns hold a sentinel."""
import numpy as np
import pytest

import chains as CH
import plant_ref as PL
import trees as TR
import workloads as W
from test_gpu_batch_layout import _DevBuf, _d2h, _same_bits

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
SENTINEL = 6.02214076e23
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
    host = np.full((n, ld), SENTINEL)
    B = ctrl.batch_size
    host[:, :B] = 0.0 if values is None else values.T
    buf = _DevBuf(host)
    ctrl.bindTauDevice(buf.ptr)
    return buf


def _tau_act(ctrl, n, ld):
    ctrl.synchronize()
    return _d2h(ctrl.plantTorquesDevice(), (n, ld))


def _summary(ctrl):
    return np.column_stack([np.asarray(v, float) for v in ctrl.plantSummary().values()])


def _model_case(name, B, ld, seed=5):
    """(robot, ctrl, task objects, model): a stack at a random state"""
    from sai_primitives_amd.controller import controller_from_specs
    rng = np.random.default_rng(seed)
    if name == "tree":
        desc = TR.dual_panda_torso()
        m = W.RobotModel(desc)
        specs = TR.dual_stack(m)
    elif name == "puma6":
        desc = CH.puma_arm()
        m = W.RobotModel(desc)
        specs = [W.motion_force_task("hand", "link6", (0.05, 0.0, 0.02)), W.joint_task("posture")]
    else:
        d = W.make_inputs({"panda_arm": 2, "chain30": 5}[name], B)
        desc, m, specs = d["model"].name, d["model"], d["tasks"]
    q = np.clip(rng.uniform(-1.2, 1.2, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    dq = rng.uniform(-0.5, 0.5, (B, m.dof))
    robot, ctrl, objs = controller_from_specs(desc, specs, B, device=0, leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    return robot, ctrl, objs, m


def _cfg2(B, ld, otg):
    """config 2 (full motion-force task, posture task behind) holding its pose, moving at the start; (robot, ctrl, objs, the inputs)"""
    from sai_primitives_amd.controller import controller_from_specs
    d = W.make_inputs(2, B)
    robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, disable_otg=not otg, leading_dimension=ld)
    robot.setQ(d["q"])
    robot.setDq(0.2 * d["dq"])
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, d


# ------------------------------------------------------------------ 1. the neutral plant changes nothing
@pytest.mark.parametrize("name,B,ld", [("panda_arm", 65, 128), ("chain30", 130, 192), ("tree", 65, 128)])
def test_neutral_plant_passes_the_torques_through(sp, name, B, ld):
    robot, ctrl, objs, m = _model_case(name, B, ld)
    n = m.dof
    rng = np.random.default_rng(3)
    tau_cmd = rng.uniform(-5, 5, (B, n))
    tau_cmd[B // 2] = np.nan                          # a flagged instance under the NaN policy
    tau_cmd[0, 0] = -0.0
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    ends = []
    with _bind_tau(ctrl, n, ld, tau_cmd) as buf:
        for attached in (False, True):
            robot.setQ(q0)
            robot.setDq(dq0)
            if attached:
                ctrl.attachPlant()
                assert ctrl.plantInfo() == dict(per_instance_joints=False, n_wrenches=0, per_instance_wrenches=False, period=0)
            ctrl.integrate(DT, 2)
            ends.append(tuple(a.copy() for a in ctrl.pullState()))
        act = _tau_act(ctrl, n, ld)
        assert np.array_equal(act[:, :B].T, np.where(np.isnan(tau_cmd), 0.0, tau_cmd))
        assert not act[:, B:].any()                                      # columns B.. are never written (zero since the attach)
        assert _same_bits(ends[0][0], ends[1][0]) and _same_bits(ends[0][1], ends[1][1])
        assert not _summary(ctrl).any() and ctrl.plantInfo()["period"] == 1
        got = buf.get()
        assert np.all(got[:, B:] == SENTINEL) and _same_bits(got[:, :B], np.ascontiguousarray(tau_cmd.T))    # the commanded torques are never written
        ctrl.detachPlant()
    ctrl.bindTauDevice(0)


@pytest.mark.parametrize("otg", [False, True])
def test_neutral_plant_leaves_a_rollout_bit_for_bit(sp, otg):
    B, ld, K = 65, 128, 5
    ends = []
    for attached in (False, True):
        robot, ctrl, objs, d = _cfg2(B, ld, otg)
        with _bind_tau(ctrl, 7, ld) as buf:
            if attached:
                ctrl.attachPlant()
            ctrl.rolloutAsync(K, DT, SUB)
            ctrl.synchronize()
            q, dq = ctrl.pullState()
            ends.append((q.copy(), dq.copy(), ctrl.getTorques(), ctrl.status.copy()))
            assert np.all(buf.get()[:, B:] == SENTINEL)
            if attached:
                assert ctrl.plantInfo()["period"] == K and not _summary(ctrl).any()
                ctrl.detachPlant()
        ctrl.bindTauDevice(0)
    assert all(_same_bits(np.asarray(x, float), np.asarray(y, float)) for x, y in zip(*ends))
    assert np.abs(ends[0][1]).max() > 1e-3


# ------------------------------------------------------------------ 2. the joint part against the restatement
def _joint_table(rng, m, B):
    """random per-instance rows (n, B, 10): every word away from its neutral value"""
    n = m.dof
    t = np.empty((n, B, 10))
    t[..., PL.GAIN], t[..., PL.BIAS] = rng.uniform(0.8, 1.2, (n, B)), rng.uniform(-0.5, 0.5, (n, B))
    t[..., PL.TAU_MAX] = rng.uniform(1.0, 6.0, (n, B))
    t[..., PL.FV], t[..., PL.FC], t[..., PL.VS] = rng.uniform(0.0, 0.3, (n, B)), rng.uniform(0.1, 1.0, (n, B)), rng.uniform(0.05, 0.3, (n, B))
    t[..., PL.Q_LO], t[..., PL.Q_HI] = rng.uniform(-1.0, -0.4, (n, B)), rng.uniform(0.4, 1.0, (n, B))
    t[..., PL.K_STOP], t[..., PL.C_STOP] = rng.uniform(50.0, 300.0, (n, B)), rng.uniform(0.0, 5.0, (n, B))
    return t


@pytest.mark.parametrize("name,B,ld", [("panda_arm", 65, 128), ("chain30", 130, 192)])
def test_joint_part_equals_the_restatement_bit_for_bit(sp, name, B, ld):
    robot, ctrl, objs, m = _model_case(name, B, ld)
    n = m.dof
    rng = np.random.default_rng(17)
    table = _joint_table(rng, m, B)
    tau_cmd = rng.uniform(-8, 8, (B, n))
    tau_cmd[1] = np.nan
    q = rng.uniform(-1.3, 1.3, (B, n))
    dq = rng.uniform(-0.5, 0.5, (B, n)) * rng.choice([0.1, 1.0], (B, n))
    dq[2, :] = 0.0
    robot.setQ(q)
    robot.setDq(dq)
    # every branch occurs in the batch
    _, fr, st, clip = PL.joint(table, tau_cmd, q, dq)
    u1 = table[..., PL.GAIN].T * np.where(np.isnan(tau_cmd), 0.0, tau_cmd) + table[..., PL.BIAS].T
    lo, hi, vs, tmax = (table[..., k].T for k in (PL.Q_LO, PL.Q_HI, PL.VS, PL.TAU_MAX))
    assert (u1 > tmax).any() and (u1 < -tmax).any() and (clip == 0).any()
    assert (q < lo).any() and (q > hi).any() and ((q >= lo) & (q <= hi)).any() and (st > 0).any() and (st < 0).any()
    assert (np.abs(dq) > vs).any() and (np.abs(dq) < vs).any() and (dq == 0).any()
    with _bind_tau(ctrl, n, ld, tau_cmd) as buf:
        ctrl.attachPlant(table, per_instance=True)
        s = np.zeros((B, 4))
        for steps in (1, 3):                          # one substep, then three more from where it ended
            for k in range(steps):
                qk, dqk = (a.copy() for a in ctrl.pullState()) if (steps, k) != (1, 0) else (q, dq)
                want, s = PL.apply(table, tau_cmd, qk, dqk, s, DT)
                ctrl.integrate(DT, 1)
                act = _tau_act(ctrl, n, ld)
                assert _same_bits(act[:, :B], np.ascontiguousarray(want.T)), (steps, k, np.nanmax(np.abs(act[:, :B].T - want)))
                assert not act[:, B:].any()
            assert _same_bits(_summary(ctrl), s), steps
        assert (s[:, 0] > 0).all() and (s[:, 1] > 0).any() and (s[:, 2] >= 1).any() and not s[:, 3].any()
        sm = _d2h(ctrl.plantSummaryDevice(), (4, ld))
        assert not sm[:, B:].any()
        assert np.all(buf.get()[:, B:] == SENTINEL)
        ctrl.detachPlant()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 3. wrenches are J^T w
def _tree_ancestors(m, body):
    anc = np.zeros(m.dof, bool)
    par = TR.joint_parents(m)
    j = body
    while j >= 0:
        anc[j] = True
        j = par[j]
    return anc


WRENCH_SITES = {"panda_arm": [("end-effector", (0.02, -0.01, 0.1)), ("link4", (0.0, 0.03, 0.01))],
                "puma6": [("link6", (0.05, 0.0, 0.02)), ("link3", (0.01, 0.02, -0.03))],
                "chain30": [("link30", (0.0, 0.01, 0.02)), ("link11", (0.02, 0.0, 0.0))],
                "tree": [("right_link7", (0.0, 0.0, 0.1)), ("left_link4", (0.01, -0.02, 0.03))]}


@pytest.mark.parametrize("name,B,ld", [("panda_arm", 65, 128), ("puma6", 3, 64), ("chain30", 130, 192), ("tree", 65, 128)])
def test_wrenches_are_jacobian_transpose_times_wrench(sp, name, B, ld):
    robot, ctrl, objs, m = _model_case(name, B, ld)
    n = m.dof
    rng = np.random.default_rng(23)
    sites = WRENCH_SITES[name]
    vals = np.zeros((2, B, 8))
    vals[..., :6] = rng.uniform(-20, 20, (2, B, 6))
    vals[..., 6:] = [[[10.0, 14.0]], [[-np.inf, np.inf]]]                # wrench 0 acts in periods 10..13, wrench 1 for ever
    frames = ["world", "link"]
    tau_cmd = rng.uniform(-5, 5, (B, n))
    tau_cmd[B // 2] = np.nan
    base = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    J = [robot.J(link, r) for link, r in sites]
    Rl = robot.rotation(sites[1][0])
    w_world = [vals[0, :, :6], np.concatenate([np.einsum("bij,bj->bi", Rl, vals[1, :, :3]), np.einsum("bij,bj->bi", Rl, vals[1, :, 3:6])], axis=1)]
    part = [np.einsum("bej,be->bj", J[k], w_world[k]) for k in range(2)]

    def run(period):
        robot.setQ(q0)
        robot.setDq(dq0)
        ctrl.setPlantPeriod(period)
        ctrl.integrate(DT, 1)
        assert ctrl.plantInfo()["period"] == period + 1
        return _tau_act(ctrl, n, ld)

    with _bind_tau(ctrl, n, ld, tau_cmd) as buf:
        ctrl.attachPlant(wrenches=[(sites[k][0], sites[k][1], frames[k], vals[k]) for k in range(2)], per_instance=True)
        both, only1 = run(10), run(9)
        for got, want in ((both, part[0] + part[1]), (only1, part[1])):
            scale = max(1.0, np.abs(want).max())
            err = np.abs((got[:, :B].T - base) - want).max() / scale
            print(f"{name}: max |tau_act - tau_cmd - J^T w| = {err:.3e} of {scale:.3e}")
            assert err <= 1e-12                                          # the bound of test_gpu_model_queries.py on the Jacobians
            assert not np.isnan(got[:, :B]).any() and not got[:, B:].any()
        if name == "tree":                                               # joints off the link's branch get exactly nothing
            a0, a1 = _tree_ancestors(m, n - 1), _tree_ancestors(m, 4)    # right_link7 is the last movable body, left_link4 body 4
            assert a0.sum() == 8 and a1.sum() == 5
            assert not (both[:, :B].T - base)[:, ~(a0 | a1)].any() and not (only1[:, :B].T - base)[:, ~a1].any()
            assert np.abs(part[0][:, ~a0]).max() == 0.0 and np.abs(part[1][:, ~a1]).max() == 0.0
        # the window of wrench 0: absent at p_start - 1 and p_end, present at p_start and p_end - 1, bit for bit
        assert _same_bits(run(13), both) and _same_bits(run(14), only1) and not _same_bits(both, only1)
        # external work: sum dt sum_j ext_j dq_j over the substeps so far (four, in periods 10, 9, 13 and 14)
        sm = _summary(ctrl)
        work = DT * (2 * np.einsum("bj,bj->b", part[0] + part[1], dq0) + 2 * np.einsum("bj,bj->b", part[1], dq0))
        assert np.abs(sm[:, 3] - work).max() <= 1e-11 * max(1.0, np.abs(work).max()) and not sm[:, :3].any()
        # a neutral run where the wrenches are absent: the commanded torques alone
        ctrl.setPlantWrenches(np.concatenate([vals[..., :6], np.broadcast_to([5.0, 5.0], (2, B, 2))], axis=-1))
        assert np.array_equal(run(5)[:, :B].T, base)
        assert np.all(buf.get()[:, B:] == SENTINEL)
        ctrl.detachPlant()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 4., 5. a stop and friction on a slider
def _slider(mass):
    """a vertical slider (prismatic z) that carries a horizontal one (prismatic x), as in the contact tests: the mass matrix is diagonal,
    the vertical joint moves the total mass, the horizontal one a quarter of it"""
    ine = [0.01, 0.01, 0.01, 0, 0, 0]
    return dict(name="slider2", links=[CH._link("link1", "prismatic", [0, 0, 0], [0, 0, 0], [0, 0, 1], 0.75 * mass, [0, 0, 0], ine, -5.0, 5.0, 1e3),
                                       CH._link("link2", "prismatic", [0, 0, 0], [0, 0, 0], [1, 0, 0], 0.25 * mass, [0, 0, 0], ine, -5.0, 5.0, 1e3)])


def _slider_stack(B, ld, mass):
    from sai_primitives_amd.controller import controller_from_specs
    tasks = [W.motion_force_task("tip", "link2", (0, 0, 0), dirs_trans=[[0, 0, 1], [1, 0, 0]], dirs_rot=None)]
    return controller_from_specs(_slider(mass), tasks, B, device=0, leading_dimension=ld)


@pytest.mark.parametrize("B,ld", SHAPES)
def test_drop_on_a_joint_stop(sp, B, ld):
    """the vertical slider of mass m released above a lower stop at q = 0 with critical damping c = 2 sqrt(k m): the oscillator of
    test_drop_on_a_plane.  Every checked period against the NumPy restatement of the same semi-implicit stepping, then the rest state
    q = q_lo - m g / k.  Per substep the device and the restatement differ by a few roundings: <= 8 eps on q, on dq and on dt * ddq.  In
    the energy norm (om dq_err is to q_err what dq is to q) the stop does not amplify them, in free flight q_err grows by dt * dq_err
    per step: after s substeps dq_err <= s inj, q_err <= s inj (1 / om + s dt), inj = 8 eps (om max|q| + max|dq| + dt max|ddq|)."""
    m, k, g = 2.0, 1.0e4, 9.81
    c = 2.0 * np.sqrt(k * m)
    om = np.sqrt(k / m)
    dts = DT / 2
    robot, ctrl, objs = _slider_stack(B, ld, m)
    h0 = np.linspace(0.0, 2e-3, B)                  # instance i starts h0[i] above the stop, at rest
    robot.setQ(np.column_stack([h0, np.zeros(B)]))
    robot.setDq(np.zeros((B, 2)))
    robot.updateModel()
    table = PL.neutral(2)
    table[0, [PL.Q_LO, PL.K_STOP, PL.C_STOP]] = [0.0, k, c]
    with _bind_tau(ctrl, 2, ld) as buf:             # commanded torque 0: free fall onto the stop
        ctrl.attachPlant(table)
        q, dq = h0.copy(), np.zeros(B)
        checked, total = 40, 840
        hist = []
        for period in range(checked):
            for _ in range(SUB):                    # the restatement: the stop at the state, then one semi-implicit Euler substep
                st = PL.joint(table[:1], np.zeros((B, 1)), q[:, None], dq[:, None])[2][:, 0]
                ddq = (st - m * g) / m
                dq = dq + dts * ddq
                q = q + dts * dq
                hist.append((np.abs(q).max(), np.abs(dq).max(), np.abs(ddq).max()))
            ctrl.integrate(dts, SUB)
            gq, gdq = ctrl.pullState()
            hq, hdq, hdd = (max(h[i] for h in hist) for i in range(3))
            s = (period + 1) * SUB
            inj = 8 * EPS * (om * hq + hdq + dts * hdd)
            b_dq = s * inj
            b_q = s * inj * (1.0 / om + s * dts)
            print(period, np.abs(gq[:, 0] - q).max(), b_q, np.abs(gdq[:, 0] - dq).max(), b_dq)
            assert np.abs(gq[:, 0] - q).max() <= b_q, (period, np.abs(gq[:, 0] - q).max(), b_q)
            assert np.abs(gdq[:, 0] - dq).max() <= b_dq, (period, np.abs(gdq[:, 0] - dq).max(), b_dq)
        for _ in range(total - checked):
            ctrl.integrate(dts, SUB)
        gq, gdq = ctrl.pullState()
        # the residual of the critically damped semi-implicit step after the time T: the derivation of test_drop_on_a_plane
        T = (total - checked) * SUB * dts
        a = om * dts
        start = 2e-3 + 2 * m * g / k
        resid = 2.0 * (1.0 + om * T) * np.exp(-om * T * (1.0 - 1.01 * np.sqrt(a) - a)) * start
        assert resid < 1e-9
        assert not gq[:, 1].any() and not gdq[:, 1].any()                                    # the horizontal joint never moved
        assert np.abs(gq[:, 0] + m * g / k).max() <= resid + b_q, np.abs(gq[:, 0] + m * g / k).max()
        act = _tau_act(ctrl, 2, ld)
        assert np.abs(act[0, :B] - m * g).max() <= (k + c * om) * (resid + b_q) and not act[1].any() and not act[:, B:].any()
        sm = ctrl.plantSummary()
        assert (sm["substeps_limited"] > 0).all() and not sm["max_clip"].any() and not sm["friction_loss"].any() and not sm["external_work"].any()
        assert ctrl.plantInfo()["period"] == total
        assert np.all(buf.get()[:, B:] == SENTINEL) and not buf.get()[:, :B].any()
        ctrl.detachPlant()
    ctrl.bindTauDevice(0)


@pytest.mark.parametrize("B,ld", SHAPES)
def test_coulomb_friction_stops_the_slider(sp, B, ld):
    """the horizontal slider (mass m2) at dq = v0 with Coulomb friction fc regularised below v_s, no gravity, no command, and
    dt fc / (m2 v_s) = 0.05.  While |dq| > v_s the friction is fc sign(dq) exactly and dq_k = v0 - k dt fc / m2; a substep computes
    dq + dt * (-(fc dq / |dq|) / m2) in a handful of roundings of dq and of the decrement: <= 8 eps (|v0| + dt fc / m2) each, k of them
    after k substeps.  Below v_s a substep multiplies dq by 1 - 0.05: |dq| decays, keeps its sign and the errors shrink with it.  The
    friction loss sum dt |fr dq| is checked against the same sum over the restated trajectory: a term is dt fc |dq| above v_s and
    dt fc dq^2 / v_s below, so an error e of dq changes it by at most 2 dt fc e, plus 8 eps of the term for its own roundings."""
    mass = 2.0
    m2 = 0.25 * mass
    fc, vs = 1.0, 0.01
    dt = 0.05 * m2 * vs / fc
    robot, ctrl, objs = _slider_stack(B, ld, mass)
    v0 = np.linspace(0.05, 0.1, B) * np.where(np.arange(B) % 2, -1.0, 1.0)
    robot.setQ(np.zeros((B, 2)))
    robot.setDq(np.column_stack([np.zeros(B), v0]))
    robot.updateModel()
    table = PL.neutral(2)
    table[1, [PL.FC, PL.VS]] = [fc, vs]
    step = dt * fc / m2
    with _bind_tau(ctrl, 2, ld) as buf:
        ctrl.attachPlant(table)
        dq = v0.copy()
        loss, b_loss, prev = np.zeros(B), np.zeros(B), np.abs(v0)
        K = int(np.ceil((np.abs(v0).max() - vs) / step)) + 120
        for k in range(1, K + 1):
            fr = PL.joint(table[1:], np.zeros((B, 1)), np.zeros((B, 1)), dq[:, None])[1][:, 0]
            term = dt * np.abs(fr * dq)
            loss = loss + term
            b_k = k * 8 * EPS * (np.abs(v0) + step)
            b_loss = b_loss + 2 * dt * fc * b_k + 8 * EPS * term
            dq = dq + dt * (-fr / m2)
            ctrl.integrate(dt, 1, gravity=ZERO_G)
            gq, gdq = ctrl.pullState()
            x = gdq[:, 1]
            closed = v0 - np.sign(v0) * (k * step)
            sliding = np.abs(v0) - (k - 1) * step > vs + b_k             # the substep started above v_s, whatever the rounding
            assert (np.abs(x - closed)[sliding] <= b_k[sliding]).all(), (k, np.abs(x - closed)[sliding].max())
            assert (np.abs(x) <= prev).all() and (np.sign(x) == np.sign(v0)).all()
            assert not gq[:, 0].any() and not gdq[:, 0].any()
            prev = np.abs(x)
        assert (prev < vs).all() and (prev > 0).all() and (np.abs(dq) < vs).all()
        sm = ctrl.plantSummary()
        print("friction loss", np.abs(sm["friction_loss"] - loss).max(), b_loss.max())
        assert (np.abs(sm["friction_loss"] - loss) <= b_loss).all()
        assert np.abs(sm["friction_loss"] - 0.5 * m2 * v0 ** 2).max() <= 0.05 * 0.5 * m2 * (v0 ** 2).max()  # it is the kinetic energy, to first order in dt
        assert not sm["max_clip"].any() and not sm["substeps_limited"].any() and not sm["external_work"].any()
        assert np.all(buf.get()[:, B:] == SENTINEL)
        ctrl.detachPlant()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 6. randomise
@pytest.mark.parametrize("B,ld", SHAPES)
def test_randomize_equals_the_restatement_bit_for_bit(sp, B, ld):
    robot, ctrl, objs, d = _cfg2(B, ld, False)
    n, seed = 7, 0xC0FFEE1234567
    jl, jh = PL.neutral(n, -2.0, 2.0), PL.neutral(n, -2.0, 2.0)
    jl[:, [PL.GAIN, PL.BIAS, PL.TAU_MAX, PL.FV, PL.FC, PL.VS, PL.K_STOP]] = [0.9, -0.3, 5.0, 0.0, 0.1, 0.01, 100.0]
    jh[:, [PL.GAIN, PL.BIAS, PL.TAU_MAX, PL.FV, PL.FC, PL.VS, PL.K_STOP]] = [1.1, 0.3, 50.0, 0.2, 0.8, 0.05, 900.0]
    jh[3] = jl[3]                                                        # a joint that is not randomised
    wl = np.array([[0, 0, -30.0, 0, 0, 0, 2.0, 20.0], [-5.0, -5.0, 0, -1.0, 0, 0, -np.inf, np.inf]])
    wh = np.array([[0, 0, -10.0, 0, 0, 0, 9.5, 40.0], [5.0, 5.0, 0, 1.0, 0, 0, -np.inf, np.inf]])
    sites = [("end-effector", (0, 0, 0.1), "world", np.zeros((B, 8))), ("link4", (0, 0, 0), "link", np.zeros((B, 8)))]
    ctrl.attachPlant(np.repeat(jl[:, None, :], B, axis=1), sites, per_instance=True)

    def tables():
        ctrl.synchronize()
        return _d2h(ctrl.plantJointsDevice(), (n, 10, ld)), _d2h(ctrl.plantWrenchesDevice(), (2, 8, ld))

    ctrl.randomizePlant(seed, 3, joints=(jl, jh), wrenches=(wl, wh))
    gj, gw = tables()
    wj, ww = PL.draw(seed, 3, PL.TABLE_JOINTS, B, jl, jh), PL.draw(seed, 3, PL.TABLE_WRENCHES, B, wl, wh)
    assert _same_bits(gj[..., :B], np.ascontiguousarray(wj.transpose(0, 2, 1))) and _same_bits(gw[..., :B], np.ascontiguousarray(ww.transpose(0, 2, 1)))
    assert not gj[..., B:].any() and not gw[..., B:].any()               # columns B.. are never written
    fixed_j, fixed_w = np.broadcast_to((jl == jh)[:, None, :], wj.shape), np.broadcast_to((wl == wh)[:, None, :], ww.shape)
    assert np.array_equal(wj[fixed_j], np.broadcast_to(jl[:, None, :], wj.shape)[fixed_j]) and np.array_equal(ww[fixed_w], np.broadcast_to(wl[:, None, :], ww.shape)[fixed_w])
    assert np.array_equal(ww[0, :, 6:], np.floor(ww[0, :, 6:])) and np.isinf(ww[1, :, 6:]).all()
    ctrl.randomizePlant(seed, 4, joints=(jl, jh), wrenches=(wl, wh))     # another round: every drawn word differs
    gj4, gw4 = tables()
    assert (gj4[..., :B].transpose(0, 2, 1) != wj)[~fixed_j].all()
    drawn_w = ~fixed_w
    drawn_w[0, :, 6:] = False                                            # (floored window words can repeat)
    assert (gw4[..., :B].transpose(0, 2, 1) != ww)[drawn_w].all()
    ctrl.randomizePlant(seed, 3, joints=(jl, jh))                        # the same seed and round reproduce; a null pair leaves its table alone
    gj3, gw3 = tables()
    assert _same_bits(gj3, gj) and _same_bits(gw3, gw4)
    ctrl.randomizePlant(seed, 3, wrenches=(wl, wh))
    assert _same_bits(tables()[1], gw)
    ctrl.integrate(DT, 1)                                                # the drawn plant runs
    assert np.isfinite(_tau_act(ctrl, n, ld)).all()
    ctrl.detachPlant()
    ctrl.attachPlant(jl, [s[:3] + (np.zeros(8),) for s in sites])        # batch-uniform tables are refused
    with pytest.raises(ValueError, match="joint table is batch-uniform"):
        ctrl.randomizePlant(seed, 0, joints=(jl, jh))
    with pytest.raises(ValueError, match="wrench table is batch-uniform"):
        ctrl.randomizePlant(seed, 0, wrenches=(wl, wh))
    ctrl.detachPlant()


# ------------------------------------------------------------------ 7. composition and equivalence
def _rough_plant(rng, B, lim):
    """a per-instance plant a config-2 rollout feels: tight actuators, friction, stops at the posture the rollout starts from"""
    t = np.repeat(PL.neutral(7)[:, None, :], B, axis=1)
    t[..., PL.GAIN], t[..., PL.BIAS] = rng.uniform(0.9, 1.1, (7, B)), rng.uniform(-0.2, 0.2, (7, B))
    t[..., PL.TAU_MAX] = rng.uniform(0.5, 30.0, (7, B))
    t[..., PL.FV], t[..., PL.FC], t[..., PL.VS] = rng.uniform(0.0, 0.5, (7, B)), rng.uniform(0.0, 0.5, (7, B)), 0.05
    t[..., PL.Q_LO], t[..., PL.Q_HI] = lim[0].T, lim[1].T
    t[..., PL.K_STOP], t[..., PL.C_STOP] = 200.0, 2.0
    return t


def _attach_rough(ctrl, d, B):
    rng = np.random.default_rng(41)
    q = d["q"]
    lo = q - rng.uniform(-0.01, 0.05, q.shape)                           # some instances start below a lower stop
    lim = (lo, lo + rng.uniform(0.02, 0.08, q.shape))                    # ... or above an upper one; q_lo < q_hi everywhere
    w = np.zeros((B, 8))
    w[:, :6] = rng.uniform(-10, 10, (B, 6))
    w[:, 6:] = [2.0, 4.0]                                                # a shove in periods 2 and 3
    pay = np.zeros((B, 8))
    pay[:, 2], pay[:, 6:] = -9.81 * rng.uniform(0.5, 2.0, B), [-np.inf, np.inf]
    ctrl.attachPlant(_rough_plant(rng, B, lim), [("end-effector", (0, 0, 0.1), "world", pay), ("link5", (0.0, 0.02, 0.0), "link", w)], per_instance=True)


def _table_under(robot, depth, k=2.0e4, c=400.0, mu=0.3):
    B = robot.batch_size
    p = robot.position("end-effector", (0, 0, 0.07))
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, k, c, mu, 1e-3]
    planes[0, :, 3] = p[:, 2] + depth
    return planes


@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_plant_composes_in_front_of_the_contact_planes(sp, B, ld):
    robot, ctrl, objs, d = _cfg2(B, ld, False)
    mf = objs[0]
    rng = np.random.default_rng(2)
    tau_cmd = rng.uniform(-20, 20, (B, 7))
    tau_cmd[5] = np.nan
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    planes = _table_under(robot, 2e-3)
    with _bind_tau(ctrl, 7, ld, tau_cmd) as buf:
        _attach_rough(ctrl, d, B)
        mf.attachContactPlanes(planes, sensor=False, per_instance=True)
        ctrl.integrate(DT, 1, gravity=ZERO_G)
        act = _tau_act(ctrl, 7, ld)
        sim = _d2h(mf.contactTorquesDevice(), (7, ld))
        q1, dq1 = (a.copy() for a in ctrl.pullState())
        assert (mf.contactReadout()["active"] == 1).all() and np.abs(sim[:, :B] - act[:, :B]).max() > 1.0
        assert np.abs(act[:, :B].T - np.where(np.isnan(tau_cmd), 0.0, tau_cmd)).max() > 1.0
        assert np.all(buf.get()[:, B:] == SENTINEL)
        ctrl.detachPlant()
    # the contact planes alone, commanded tau_act: the same contact buffer, hence the same contact contribution, bit for bit
    robot.setQ(q0)
    robot.setDq(dq0)
    with _bind_tau(ctrl, 7, ld, act[:, :B].T):
        ctrl.integrate(DT, 1, gravity=ZERO_G)
        ctrl.synchronize()
        sim2 = _d2h(mf.contactTorquesDevice(), (7, ld))
        q2, dq2 = (a.copy() for a in ctrl.pullState())
    assert _same_bits(sim, sim2) and _same_bits(sim[:, :B] - act[:, :B], sim2[:, :B] - act[:, :B])
    assert _same_bits(q1, q2) and _same_bits(dq1, dq2)
    mf.detachContactPlanes()
    # the plain integrator fed the final buffer: the same state bits
    robot.setQ(q0)
    robot.setDq(dq0)
    ctrl.bindTauDevice(0)
    ctrl.setTorques(sim[:, :B].T)
    ctrl.integrate(DT, 1, gravity=ZERO_G)
    q3, dq3 = ctrl.pullState()
    assert _same_bits(q1, q3) and _same_bits(dq1, dq3)


def _final(ctrl, objs, contact, ld=128):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    out = dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float), goals=[t._get_goal() for t in objs],
               plant=_summary(ctrl), act=_d2h(ctrl.plantTorquesDevice(), (7, ld)), period=np.array([float(ctrl.plantInfo()["period"])]))
    if contact:
        out["contact"] = np.column_stack(list(objs[0].contactSummary().values())).astype(float)
    return out


@pytest.mark.parametrize("otg,sched,rec,contact", [(False, False, False, False), (True, False, False, False), (False, True, True, False), (True, False, False, True),
                                                   (False, False, True, True)])
def test_rollout_equals_the_host_driven_loop(sp, otg, sched, rec, contact):
    B, ld, K = 65, 128, 6
    runs = []
    for host in (False, True):
        robot, ctrl, objs, d = _cfg2(B, ld, otg)
        mf = objs[0]
        buf = _bind_tau(ctrl, 7, ld)
        _attach_rough(ctrl, d, B)
        if contact:
            mf.attachContactPlanes(_table_under(robot, 1e-3), sensor=True, per_instance=True)
        if sched:
            g = mf._get_goal()[:, :3]
            keys = g[None] + np.linspace(0.0, 0.01, 3)[:, None, None] * np.array([1.0, -1.0, 0.0])
            mf.setGoalSchedule((0, 3), keys, stride=2, mode="linear")
        if rec:
            ctrl.recordRollouts(K, 1, ("q", "tau"), task=mf, summaries=True)
        if not host:
            ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        elif sched or rec:                           # schedules and the recorder act inside rollouts only: one period per call
            for _ in range(K):
                ctrl.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
        else:
            for _ in range(K):
                if contact:
                    ctrl.contactSense()
                ctrl.stepAsync()
                ctrl.integrate(DT, SUB, gravity=ZERO_G)
        out = _final(ctrl, objs, contact)
        if rec:
            out["log"] = ctrl.rolloutLog()["tau"]
            out["rsum"] = ctrl.rolloutSummary()
        out["tau_buf"] = buf.get()
        runs.append(out)
        if contact:
            mf.detachContactPlanes()
        ctrl.detachPlant()
        ctrl.bindTauDevice(0)
        buf.free()
    a, b = runs
    for key in a:
        if key == "goals":
            assert all(_same_bits(x, y) for x, y in zip(a[key], b[key]))
        else:
            assert _same_bits(np.asarray(a[key]), np.asarray(b[key])), key
    assert a["period"][0] == K and np.isfinite(a["q"]).all() and np.all(a["tau_buf"][:, B:] == SENTINEL) and not a["act"][:, B:].any()
    assert (a["plant"][:, 0] > 0).all() and (a["plant"][:, 1] > 0).any() and (a["plant"][:, 2] > 0).any() and (a["plant"][:, 3] != 0).all()
    if rec:
        assert _same_bits(a["log"][-1], a["tau"])                                    # the recorder logs the commanded torques
        assert not _same_bits(a["act"][:, :B].T, a["tau"])
    if contact:
        assert (a["contact"][:, 3] >= 1).all()


@pytest.mark.parametrize("otg", [False, True])
def test_snapshot_restore_reproduces_a_rollout(sp, otg):
    B, ld, K = 65, 128, 6
    robot, ctrl, objs, d = _cfg2(B, ld, otg)
    plain = ctrl.saveState()
    layout, nbytes = plain.segments(), plain.nbytes()
    with _bind_tau(ctrl, 7, ld) as buf:
        _attach_rough(ctrl, d, B)
        snap = ctrl.saveState()
        assert snap.segments() == layout and snap.nbytes() == nbytes     # the attachment is configuration: not part of a snapshot
        ctrl.setPlantPeriod(1)
        ends = []
        for _ in range(2):
            ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
            out = _final(ctrl, objs, False)
            out["tau_buf"] = buf.get()
            ends.append(out)
            assert ctrl.plantInfo()["period"] == 1 + K
            ctrl.restoreState(snap)
            ctrl.setPlantPeriod(1)
            ctrl.resetPlantSummary()
        for key in ends[0]:
            if key == "goals":
                assert all(_same_bits(x, y) for x, y in zip(ends[0][key], ends[1][key]))
            else:
                assert _same_bits(np.asarray(ends[0][key]), np.asarray(ends[1][key])), key
        assert (ends[0]["plant"][:, 3] != 0).all()
        ctrl.detachPlant()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 8. lifecycle
def test_lifecycle(sp):
    B, ld, K = 65, 128, 6
    robot, ctrl, objs, d = _cfg2(B, ld, True)
    assert ctrl.plantTorquesDevice() is None
    with pytest.raises(sp.SaipError, match="no plant model is attached"):
        ctrl.plantInfo()
    _attach_rough(ctrl, d, B)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachPlant()
    assert ctrl.plantInfo() == dict(per_instance_joints=True, n_wrenches=2, per_instance_wrenches=True, period=0)
    assert all(p is not None for p in (ctrl.plantTorquesDevice(), ctrl.plantJointsDevice(), ctrl.plantWrenchesDevice(), ctrl.plantSummaryDevice()))
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    s1 = ctrl.plantSummary()
    assert ctrl.plantInfo()["period"] == K and (s1["friction_loss"] > 0).all()
    ctrl.resetPlantSummary()
    ctrl.setPlantJoints(np.repeat(PL.neutral(7)[:, None, :], B, axis=1))
    ctrl.setPlantWrenches(np.zeros((2, B, 8)))                           # empty windows
    ctrl.rolloutAsync(2, DT, SUB, gravity=ZERO_G)
    assert not _summary(ctrl).any() and ctrl.plantInfo()["period"] == K + 2
    bad = np.repeat(PL.neutral(7)[:, None, :], B, axis=1)
    bad[2, B - 1, PL.TAU_MAX] = -1.0
    with pytest.raises(ValueError, match="joint 2 of instance 64: word tau_max"):
        ctrl.setPlantJoints(bad)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    ctrl.detachPlant()                                                   # with a rollout in flight: the detach waits for it
    assert ctrl.plantTorquesDevice() is None and ctrl.plantSummaryDevice() is None
    with pytest.raises(sp.SaipError, match="no plant model is attached"):
        ctrl.plantSummary()
    ctrl.attachPlant(wrenches=[("end-effector", (0, 0, 0.1), "world", [0, 0, -9.81, 0, 0, 0])])      # re-attach, batch-uniform this time
    assert ctrl.plantInfo() == dict(per_instance_joints=False, n_wrenches=1, per_instance_wrenches=False, period=0)
    ctrl.integrate(DT, SUB, gravity=ZERO_G)
    assert (ctrl.plantSummary()["external_work"] != 0).all()
    ctrl.detachPlant()
    # attach, detach, then a rollout: the bits of a batch that never had a plant; and a batch destroyed while attached
    ends = []
    for touched in (False, True):
        robot2, ctrl2, objs2, d2 = _cfg2(B, ld, True)
        if touched:
            _attach_rough(ctrl2, d2, B)
            ctrl2.detachPlant()
        ctrl2.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        ctrl2.synchronize()
        q, dq = ctrl2.pullState()
        ends.append((q.copy(), dq.copy(), ctrl2.getTorques(), ctrl2.kernelName()))
    assert all(_same_bits(x, y) for x, y in zip(ends[0][:3], ends[1][:3])) and ends[0][3] == ends[1][3]
    robot3, ctrl3, objs3, d3 = _cfg2(B, ld, False)
    _attach_rough(ctrl3, d3, B)
    ctrl3.rolloutAsync(2, DT, SUB, gravity=ZERO_G)
    ctrl3._release()                                                     # destroy while attached, a rollout in flight
