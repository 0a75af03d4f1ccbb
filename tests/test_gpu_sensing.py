"""The sensing model of the resident simulator on the device (csrc/saip_sense.hip, saip_batch_sensing_*).  Oracles: an unattached batch
(a neutral table changes nothing; offsets equal a shifted state), the NumPy restatement tests/sensing_ref.py (bit for bit without noise,
within min(64 x linear_bound, 1e-11) with it: the rule of tests/test_gpu_sampler.py), the clean simulated sensor of an unattached twin
passed through se_measure, the known fixed point of a joint task under an encoder offset, and the host-driven loop { measureState, cycle,
integrate } for whole rollouts.

Shapes: the Panda's config-2 stack with B = 70 at a padded leading dimension and B = 1, B = 300 for the draw, the 30-dof chain (wavefront
kernel) with B = 5, a 6-dof arm on the lane kernel, the dual-arm tree (general kernel) with B = 3."""
import numpy as np
import pytest

import sensing_ref as SE
import trees as TR
import workloads as W
from test_gpu_batch_layout import _build, _d2h, _h2d, _same_bits, _stack
from test_gpu_contact import _cfg13, _table_under
from test_gpu_rollout_record import _panda
from test_sampler_cpu import linear_bound

pytestmark = pytest.mark.gpu

SENTINEL = 6.02214076e23
DT, SUB = 5e-4, 2
ZERO_G = (0.0, 0.0, 0.0)
#          stack            B   ld    kernel forced    the kernel the cycle must run
KERNELS = {"panda": ("cfg2", 70, 128, None, "saip_cycle_oct"),
           "panda1": ("cfg2", 1, 32, None, "saip_cycle_oct"),
           "chain30": ("cfg5", 5, 64, 4, "saip_cycle_wave"),
           "arm6_lane": ("arm6", 70, 96, 2, "saip_cycle_lane"),
           "tree": ("tree", 3, 32, None, "saip_cycle_wg_tree<32,512>")}


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _case(name, otg=False):
    """(robot, ctrl, objs, q, dq, gravity): a fresh batch of the named stack at a moving state, goals away from it"""
    from sai_primitives_amd.controller import controller_from_specs
    stack, B, ld, kernel, _ = KERNELS[name]
    rng = np.random.default_rng(7)
    if stack == "tree":
        desc = TR.dual_panda_torso()
        m = W.RobotModel(desc)
        q = np.clip(rng.uniform(-0.8, 0.8, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
        robot, ctrl, objs = controller_from_specs(desc, TR.dual_stack(m), B, device=0, disable_otg=not otg, leading_dimension=ld)
        if otg:
            objs[2].disableInternalOtg()                                 # (as tests/test_gpu_rollout_record.py drives this stack)
        ctrl.setFlaggedTorquePolicy(True)
        ctrl.enableGravityCompensation(True)
        grav = None
    else:
        c = _stack(stack, B)
        robot, ctrl, objs = _build(c, B, ld, kernel, disable_otg=not otg)
        q, m, grav = c["q"], c["model"], ZERO_G
    dq = rng.uniform(-0.2, 0.2, q.shape)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.reinitializeTasks()
    objs[0].setGoalPosition(objs[0].getGoalPosition() + np.array([0.02, -0.01, 0.015]))
    objs[-1].setGoalPosition(q + 0.1)
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, q.copy(), dq.copy(), grav


def _finals(ctrl):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    return [q.copy(), dq.copy(), ctrl.getTorques(), ctrl.status.astype(np.float64)]


def _equal(a, b):
    return all(_same_bits(np.asarray(x, float), np.asarray(y, float)) for x, y in zip(a, b))


# ------------------------------------------------------------------ 1. neutral sensing changes nothing
@pytest.mark.parametrize("name,otg", [(k, o) for k in ("panda", "panda1", "chain30", "arm6_lane", "tree") for o in (False, True)])
def test_neutral_sensing_leaves_cycle_integrate_and_rollout_unchanged(sp, name, otg):
    K, runs = 5, []
    n = KERNELS[name]
    for attached in (False, True):
        robot, ctrl, objs, q, dq, grav = _case(name, otg)
        if attached:
            ctrl.attachSensing(seed=3)
            assert ctrl.sensingInfo() == dict(per_instance_joints=False, n_wrench_tasks=0, per_instance_wrenches=False, period=0)
        ctrl.recordRollouts(K, 1, ("q", "dq", "tau"))
        tau = ctrl.computeControlTorques()
        out = [tau, ctrl.status.astype(float)]
        assert ctrl.kernelName() == n[4]
        ctrl.integrate(DT, SUB, gravity=grav)
        out += _finals(ctrl)
        ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
        out += _finals(ctrl)
        log = ctrl.rolloutLog()
        out += [log[k] for k in ("q", "dq", "tau")] + [log["status"].astype(float)]
        if attached:
            assert ctrl.sensingInfo()["period"] == K + 1
            qm, dqm = ctrl.measuredState()                               # the measurement of the last period's state
            ctrl.measureState()
            qm, dqm = ctrl.measuredState()
            assert _same_bits(qm, out[6] + 0.0) and _same_bits(dqm, out[7] + 0.0)
        runs.append(out)
    assert _equal(*runs)
    assert np.abs(runs[0][7]).max() > 1e-3 and np.isfinite(runs[0][0]).any()


# ------------------------------------------------------------------ 2. the controller sees exactly the measured state
@pytest.mark.parametrize("name", ["panda", "panda1", "chain30", "arm6_lane", "tree"])
def test_offsets_equal_a_shifted_state(sp, name):
    _, B, ld, _, kernel = KERNELS[name]
    rng = np.random.default_rng(11)
    robot, ctrl, objs, q, dq, grav = _case(name)
    n = q.shape[1]
    qo, dqo = rng.uniform(-0.03, 0.03, n), rng.uniform(-0.05, 0.05, n)
    ctrl.attachSensing(dict(q_off=qo, dq_off=dqo))
    qp, dqp = ctrl.measuredStateDevice()
    _h2d(qp, np.full((n, ld), SENTINEL))
    _h2d(dqp, np.full((n, ld), SENTINEL))
    tau = ctrl.computeControlTorques()
    status = ctrl.status.copy()
    assert ctrl.kernelName() == kernel
    tq, tdq = ctrl.pullState()
    assert _same_bits(tq, q) and _same_bits(tdq, dq)                     # the true state keeps its bits
    for ptr, want in ((qp, q + qo), (dqp, dq + dqo)):
        got = _d2h(ptr, (n, ld))
        assert _same_bits(got[:, :B], np.ascontiguousarray(want.T)) and np.all(got[:, B:] == SENTINEL)
    qm, dqm = ctrl.measuredState()
    assert _same_bits(qm, q + qo) and _same_bits(dqm, dq + dqo)
    tau2 = ctrl.computeControlTorques()                                  # a second cycle at the same state: the same measurement
    assert _same_bits(tau2, tau)
    ctrl.detachSensing()
    # the unattached twin at the shifted state
    robot2, ctrl2, objs2, _, _, _ = _case(name)
    robot2.setQ(q + qo)
    robot2.setDq(dq + dqo)
    robot2.updateModel()
    ctrl2.updateControllerTaskModels()
    want = ctrl2.computeControlTorques()
    assert _same_bits(tau, want) and np.array_equal(status, ctrl2.status)
    robot3, ctrl3, _, _, _, _ = _case(name)
    assert not _same_bits(ctrl3.computeControlTorques(), want)           # (the offsets matter)


# ------------------------------------------------------------------ 3. quantisation, the draw and the noise against the restatement
def _random_joint_table(rng, n, shape, sigma):
    t = np.zeros((n,) + shape + (6,))
    sh = t.shape[:-1]
    t[..., 0], t[..., 3] = rng.uniform(-0.03, 0.03, sh), rng.uniform(-0.05, 0.05, sh)
    t[..., 1], t[..., 4] = rng.choice([2 * np.pi / 2 ** 14, 0.0, 0.125], sh), rng.choice([1e-2, 0.0, 2.0 ** -6], sh)
    t[..., 2], t[..., 5] = sigma * rng.uniform(0.5, 1.0, sh), sigma * rng.uniform(0.5, 1.0, sh)
    t[0] = 0.0
    return t


def test_quantisation_and_the_draw_equal_the_restatement_bit_for_bit(sp):
    B, ld, n = 300, 320, 7
    rng = np.random.default_rng(13)
    robot, ctrl, objs, mf, grav = _panda(B, False, ld=ld)
    q = rng.uniform(-2.5, 2.5, (B, n))
    q[::3, 2] = (rng.integers(-40, 40, len(q[::3])) + 0.5) * 0.125        # exactly on a half step of joint 2's resolution
    dq = rng.uniform(-1, 1, (B, n))
    q[5, 1], dq[6, 3], dq[7, 4] = np.nan, np.inf, -np.inf
    robot.setQ(q)
    robot.setDq(dq)
    table = _random_joint_table(rng, n, (B,), 0.0)
    table[2, :, :] = [0.0, 0.125, 0.0, 0.0, 2.0 ** -6, 0.0]
    ctrl.attachSensing(table, per_instance=True)
    ctrl.measureState()
    qm, dqm = ctrl.measuredState()
    wq, wdq = SE.joints(table, q, dq)
    assert _same_bits(qm, wq) and _same_bits(dqm, wdq)
    assert np.isnan(qm[5, 1]) and dqm[6, 3] == np.inf and dqm[7, 4] == -np.inf
    assert np.array_equal((qm[::3, 2] / 0.125) % 2, np.zeros(len(q[::3])))                   # half to even
    # the per-instance draw
    lo, hi = _random_joint_table(rng, n, (), 1e-3), _random_joint_table(rng, n, (), 1e-3)
    hi[:, ::3] = lo[:, ::3]
    ctrl.sensingRandomize(0xC0FFEE123456789, 4, joints=(lo, hi))
    ctrl.synchronize()
    got = _d2h(ctrl.sensingJointsDevice(), (n, 6, ld))
    want = SE.draw(0xC0FFEE123456789, 4, SE.TABLE_JOINTS, B, lo, hi)
    assert _same_bits(got[:, :, :B], np.ascontiguousarray(want.transpose(0, 2, 1))) and not got[:, :, B:].any()
    ctrl.measureState()
    qm2, dqm2 = ctrl.measuredState()
    w2 = SE.joints(want, q, dq, 0, 0, quantise=False)
    res_q, res_dq = want[..., 1].T, want[..., 4].T
    fin = np.isfinite(q) & np.isfinite(dq)
    for g, u, r, s in ((qm2, w2[0], res_q, want[..., 2].max()), (dqm2, w2[1], res_dq, want[..., 5].max())):
        bound = min(64 * linear_bound(s, 2.6), 1e-11)
        on = (r > 0) & fin
        assert np.array_equal(r[on] * np.rint(g[on] / r[on]), g[on])
        assert (np.abs(g[fin] - u[fin]) <= np.where(r > 0, r / 2 * (1 + 2.0 ** -50), 0.0)[fin] + bound).all()
    ctrl.detachSensing()


def test_noise_equals_the_restatement_and_is_keyed_by_seed_and_period(sp):
    _, B, ld, _, _ = KERNELS["panda"]
    rng = np.random.default_rng(17)
    robot, ctrl, objs, q, dq, grav = _case("panda")
    n, seed = 7, 0xFEEDFACE12345678
    table = _random_joint_table(rng, n, (), 5e-3)
    table[:, [1, 4]] = 0.0
    ctrl.attachSensing(table, seed=seed)
    bound = min(64 * linear_bound(5e-3, np.abs(q).max() + 0.05), 1e-11)

    def measured(period):
        ctrl.setSensingPeriod(period)
        ctrl.computeControlTorques()                                     # the cycle takes the measurement itself
        return ctrl.measuredState()
    a = measured(41)
    want = SE.joints(table, q, dq, seed, 41)
    assert np.abs(a[0] - want[0]).max() <= bound and np.abs(a[1] - want[1]).max() <= bound
    b = measured(42)
    assert (b[0] != a[0])[:, 1:].all() and (b[1] != a[1])[:, 1:].all()   # the next period differs in every noisy element
    assert _same_bits(b[0][:, 0], q[:, 0] + 0.0)                        # the neutral joint
    c = measured(41)
    assert _same_bits(c[0], a[0]) and _same_bits(c[1], a[1])             # equal (seed, period): equal bits
    ctrl.setSensingSeed(seed + 1)
    d = measured(41)
    assert (d[0] != a[0])[:, 1:].all()
    with pytest.raises(ValueError, match="0 <= period < 2\\^32"):
        ctrl.setSensingPeriod(2 ** 32)
    ctrl.setSensingPeriod(2 ** 32 - 1)
    ctrl.detachSensing()


# ------------------------------------------------------------------ 4. the sensed wrench
WRENCH = np.array([[0.5, 0.25, 0.0], [-0.3, 0.0, 0.0], [1.5, 0.01, 0.0], [0.02, 0.0, 0.0], [-0.01, 2.0 ** -10, 0.0], [0.0, 0.0, 0.0]])


@pytest.mark.parametrize("kind", ["planes", "patch"])
@pytest.mark.parametrize("sigma", [0.0, 0.3])
def test_sensed_wrench_is_the_clean_sensor_through_se_measure(sp, kind, sigma):
    B, ld, seed = 70, 128, 99
    table = WRENCH.copy()
    table[:, 2] = sigma * np.array([1, 1, 0, 0.1, 0, 0.1])
    rows = {}
    for attached in (False, True):
        robot, ctrl, objs = _cfg13(B, ld, False)
        mf = objs[0]
        planes = _table_under(robot, objs, 2e-3)
        if kind == "planes":
            mf.attachContactPlanes(planes, sensor=True, per_instance=True)
            sense = ctrl.contactSense
        else:
            mf.attachContactPatch(np.array([[0.02, 0.0, 0.0], [-0.02, 0.01, 0.0], [0.0, -0.02, 0.0]]), planes, sensor=True, per_instance=True)
            sense = ctrl.contactPatchSense
        if attached:
            ctrl.attachSensing(wrenches={mf: table}, seed=seed)
            ctrl.setSensingPeriod(7)
        sense()
        ctrl.synchronize()
        first = mf._get_goal()[:, 30:36].copy()
        sense()                                                          # a second call does not stack the perturbation
        ctrl.synchronize()
        assert _same_bits(mf._get_goal()[:, 30:36], first)
        if attached:
            ctrl.setSensingPeriod(0)
            ctrl.rolloutAsync(1, DT, 1, gravity=ZERO_G)                  # a rollout period writes the same rows (period 0) from the same state
            ctrl.synchronize()
            rows["rollout"] = mf._get_goal()[:, 30:36].copy()
            assert ctrl.sensingInfo()["period"] == 1
        rows[attached] = first
    clean = rows[False]
    assert np.abs(clean[:, :3]).max() > 1.0
    want = SE.wrench(table, clean, 0, seed, 7)
    want0 = SE.wrench(table, clean, 0, seed, 0)
    if sigma == 0.0:
        assert _same_bits(rows[True], want) and _same_bits(rows["rollout"], want0)
    else:
        u = SE.wrench(table, clean, 0, seed, 7, quantise=False)
        bound = min(64 * linear_bound(sigma, np.abs(clean).max() + 1.5), 1e-11)
        res = np.broadcast_to(table[:, 1], clean.shape)
        on = res > 0
        assert np.array_equal(res[on] * np.rint(rows[True][on] / res[on]), rows[True][on])
        assert (np.abs(rows[True] - u) <= np.where(on, res / 2 * (1 + 2.0 ** -50), 0.0) + bound).all()
        assert (rows[True] != want0)[:, 1].all()                         # another period: another draw (axis 1: noise without quantisation)
        u0 = SE.wrench(table, clean, 0, seed, 0, quantise=False)         # the rows a rollout period writes, period 0
        assert np.array_equal(res[on] * np.rint(rows["rollout"][on] / res[on]), rows["rollout"][on])
        assert (np.abs(rows["rollout"] - u0) <= np.where(on, res / 2 * (1 + 2.0 ** -50), 0.0) + bound).all()


def test_a_wrench_table_on_a_task_without_a_sensor_changes_nothing(sp):
    B, ld = 70, 128
    runs = []
    for attached in (False, True):
        robot, ctrl, objs = _cfg13(B, ld, False)
        mf = objs[0]
        mf.attachContactPlanes(_table_under(robot, objs, 2e-3), sensor=False, per_instance=True)
        if attached:
            ctrl.attachSensing(wrenches={mf: WRENCH}, seed=1)
        ctrl.rolloutAsync(3, DT, SUB, gravity=ZERO_G)
        runs.append(_finals(ctrl) + [mf._get_goal()])
    assert _equal(*runs) and not runs[1][4][:, 30:36].any()


# ------------------------------------------------------------------ 5. closed loop against a known answer
def test_a_joint_task_settles_at_the_goal_minus_the_encoder_offset(sp):
    """A joint task alone, gravity-free, kp 50 / kv 14: the controller drives the MEASURED q to the goal, so the true q settles at
    goal - c.  Tolerance: twice the residual the unattached run still has against its goal after the same 1500 periods."""
    from sai_primitives_amd.controller import controller_from_specs
    B, n, K = 3, 7, 1500
    d = W.make_inputs(2, B)
    c = np.array([0.02, -0.015, 0.01, 0.03, -0.02, 0.005, -0.01])
    ends = []
    for attached in (False, True):
        robot, ctrl, objs = controller_from_specs(d["model"].name, [W.joint_task("posture")], B, device=0, disable_otg=True)
        jt = objs[0]
        jt.setGains(50.0, 14.0, 0.0)
        robot.setQ(d["q"])
        robot.setDq(np.zeros((B, n)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        goal = d["q"] + 0.2
        jt.setGoalPosition(goal)
        ctrl.updateControllerTaskModels()
        if attached:
            ctrl.attachSensing(dict(q_off=c))
        ctrl.rolloutAsync(K, 1e-3, 1, gravity=ZERO_G)
        ctrl.synchronize()
        ends.append(ctrl.pullState()[0].copy())
    residual = np.abs(ends[0] - goal).max()
    print(f"unattached residual after {K} periods: {residual:.3e}; attached |q - (goal - c)|: {np.abs(ends[1] - (goal - c)).max():.3e}")
    assert residual < 1e-3                                               # the unattached run has settled
    assert np.abs(ends[1] - (goal - c)).max() <= 2 * residual


# ------------------------------------------------------------------ 6. rollout_async against the host-driven loop
@pytest.mark.parametrize("otg", [False, True])
@pytest.mark.parametrize("mode", ["plain", "contact", "all"])
def test_rollout_equals_the_host_driven_loop(sp, otg, mode):
    """plain: config 2, the host loop is { measureState, stepAsync, integrate }.  contact: config 13 with a plant and contact planes with the
    sensor and a wrench table, the host loop is { contactSense, measureState, stepAsync, integrate }.  all: goal schedule and recorder as
    well; those two act inside rollouts only, so the host loop is then one rollout period per call.  The period is set by hand."""
    B, ld, K, seed = 70, 128, 6, 5
    rng = np.random.default_rng(23)
    table = _random_joint_table(rng, 7, (), 2e-3)
    dq0 = 0.1 * rng.uniform(-1, 1, (B, 7))
    runs = []
    for host in (False, True):
        if mode == "plain":
            robot, ctrl, objs, mf, _ = _panda(B, otg, ld=ld)
            robot.setDq(dq0)
            ctrl.attachSensing(table, seed=seed)
        else:
            robot, ctrl, objs = _cfg13(B, ld, otg)
            mf = objs[0]
            mf.attachContactPlanes(_table_under(robot, objs, 2e-3), sensor=True, per_instance=True)
            ctrl.attachPlant(dict_plant(ctrl))
            if mode == "all":
                g = mf._get_goal()[:, :3]
                mf.setGoalSchedule((0, 3), g[None] + np.linspace(0.0, 0.01, 3)[:, None, None] * np.array([1.0, -1.0, 0.0]), stride=2, mode="linear")
                ctrl.recordRollouts(K, 1, ("q", "dq", "tau"), task=mf)
            ctrl.attachSensing(table, wrenches={mf: WRENCH + [0, 0, 0.05]}, seed=seed)
        if not host:
            ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        else:
            for k in range(K):
                ctrl.setSensingPeriod(k)
                if mode == "all":
                    ctrl.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
                    continue
                if mode == "contact":
                    ctrl.contactSense()
                ctrl.measureState()
                ctrl.stepAsync()
                ctrl.integrate(DT, SUB, gravity=ZERO_G)
        out = _finals(ctrl) + list(ctrl.measuredState())
        assert ctrl.sensingInfo()["period"] == K
        if mode != "plain":
            out += [mf._get_goal()]
            assert ctrl.plantInfo()["period"] == K
        if mode == "all":
            log = ctrl.rolloutLog()
            out += [log["q"], log["dq"], log["tau"]]
            assert _same_bits(log["q"][-1], out[0]) and not _same_bits(out[4], out[0])          # the recorder logs the true state
        runs.append(out)
    assert _equal(*runs)
    assert np.isfinite(runs[0][0]).all() and (runs[0][4] != runs[0][0]).any()
    if mode != "plain":
        sensed = runs[0][6][:, 30:36]
        assert np.abs(sensed[:, :3]).max() > 1.0 and np.array_equal(0.25 * np.rint(sensed[:, 0] / 0.25), sensed[:, 0])    # the perturbed wrench


def dict_plant(ctrl):
    t = ctrl.neutralPlantJoints()
    t[:, 3] = 0.05                                                        # viscous friction
    return t


# ------------------------------------------------------------------ 7. snapshots
def test_snapshot_restore_repeats_the_rollout(sp):
    B, ld, K = 70, 128, 5
    rng = np.random.default_rng(29)
    robot, ctrl, objs, mf, _ = _panda(B, True, ld=ld)
    table = _random_joint_table(rng, 7, (B,), 2e-3)
    ctrl.attachSensing(table, per_instance=True, seed=77)
    ctrl.setSensingPeriod(10)
    snap = ctrl.saveState()
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    first = _finals(ctrl) + list(ctrl.measuredState())
    ctrl.restoreState(snap)
    assert ctrl.sensingInfo()["period"] == 10 + K                        # the counter is not part of a snapshot
    got = _d2h(ctrl.sensingJointsDevice(), (7, 6, ld))
    assert _same_bits(got[:, :, :B], np.ascontiguousarray(table.transpose(0, 2, 1)))    # the per-instance table survives the restore
    ctrl.setSensingPeriod(10)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    again = _finals(ctrl) + list(ctrl.measuredState())
    assert _equal(first, again) and (first[4] != first[0]).any()
    ctrl.detachSensing()


# ------------------------------------------------------------------ 8. lifecycle
def test_lifecycle(sp):
    from sai_primitives_amd import capi
    B, ld, K = 70, 128, 4
    # attach before finalize is refused (a controller finalizes on construction: the C entry on a raw batch)
    import ctypes as C
    L = sp.lib()
    raw = C.c_void_p()
    m = sp.SaiModel("panda_arm", B, device=0)
    assert L.saip_batch_create(m._h, B, 0, C.byref(raw)) == 0
    assert L.saip_batch_sensing_attach(raw, None, 0, 0, None, None, 0, 0) == capi.SAIP_ERR_ORDER
    L.saip_batch_destroy(raw)
    robot, ctrl, objs, mf, _ = _panda(B, True, ld=ld)
    snap = ctrl.saveState()
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    plain = _finals(ctrl)
    ctrl.restoreState(snap)
    ctrl.attachSensing(dict(q_off=0.01, dq_sigma=1e-3), seed=1)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachSensing()
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    sensed = _finals(ctrl)
    assert not _same_bits(sensed[0], plain[0])
    ctrl.detachSensing()
    assert ctrl.measuredStateDevice() == (None, None)
    with pytest.raises(sp.SaipError, match="no sensing model is attached"):
        ctrl.measureState()
    ctrl.restoreState(snap)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)                        # after detach the launch sequence is the unattached one
    assert _equal(_finals(ctrl), plain)
    # another layout: per-instance joints and a wrench task
    ctrl.attachSensing(np.zeros((7, B, 6)), wrenches={mf: np.zeros((6, B, 3))}, per_instance=True)
    assert ctrl.sensingInfo() == dict(per_instance_joints=True, n_wrench_tasks=1, per_instance_wrenches=True, period=0)
    ctrl.restoreState(snap)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    assert _equal(_finals(ctrl), plain) and ctrl.sensingInfo()["period"] == K
    ctrl.detachSensing()
    # device memory returns to its level: a batch large enough for a leaked array to show in the free-memory figure
    import ctypes as C
    from test_gpu_batch_layout import _hip

    def free_bytes():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert _hip().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    Bb = 16384
    robot, ctrl, objs, mf, _ = _panda(Bb, False)
    zeros_j, zeros_w = np.zeros((7, Bb, 6)), np.zeros((6, Bb, 3))
    levels = []
    for k in range(21):
        ctrl.attachSensing(zeros_j, wrenches={mf: zeros_w}, per_instance=True)
        ctrl.stepAsync()
        ctrl.detachSensing()
        levels.append(free_bytes())
    assert levels[-1] == levels[0], levels                               # 20 more pairs after the first: nothing is left behind
