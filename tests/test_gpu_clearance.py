"""The clearance monitor on the device (csrc/saip_clearance.hip, saip_batch_clearance_*).  Oracles: the engine's own model queries for the
sphere centres, the NumPy restatement tests/clearance_ref.py for everything behind them, the host-driven loop { one period, evaluate } for
whole rollouts, a batch without the attachment for everything the monitor must not touch.

Batches (B, ld) in {(3, 64), (65, 128), (130, 192)}: a partial group block, a block edge, several blocks, at a padded leading dimension.
The padding columns of every output are pre-filled with a sentinel that must survive."""
import copy
import ctypes as C

import numpy as np
import pytest

import clearance_ref as CL
import trees as TR
import workloads as W
from test_gpu_batch_layout import _d2h, _h2d, _same_bits
from test_gpu_rollout_record import _panda

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64), (65, 128), (130, 192)]          # (B, leading dimension)
MODELS = ["panda_arm", "chain30w", "tree", "forest"]
SENTINEL = 6.02214076e23
DT, SUB = 5e-4, 2
GRAV = (0.0, 0.0, 0.0)
# 1e-12 m absolute on metre-scale models: <= 32 joints, each a handful of roundings of <= 2e-16 on lengths <= 1 m, and a factor of ten over
# that.  The walk of the clearance kernel and the walk of the model query are the same source (SAIP_FK_JOINT_STEP) in two kernels.
CENTRE_BOUND = 1e-12
WORST = {}


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


# ------------------------------------------------------------------ models, spheres, obstacles
def _chain30w():
    """chain30 with a bracket welded behind link12 (a rotated frame): link13 hangs off the bracket"""
    from sai_primitives_amd.controller import load_robot_description
    d = copy.deepcopy(load_robot_description("chain30"))
    d.pop("_source", None)
    d["name"] = "chain30w"
    bracket = dict(d["links"][11], name="bracket", joint_type="fixed", origin_xyz=[0.02, -0.03, 0.05], origin_rpy=[0.3, -0.2, 0.5], mass=0.3,
                   q_lower=0.0, q_upper=0.0, velocity_limit=0.0, effort_limit=0.0)
    d["links"].insert(12, bracket)
    return d


def _spheres(name, rng):
    """[(link, centre, radius)] and the self pairs of the model"""
    if name == "panda_arm":          # 9 spheres: more than one round of the eight lanes, the last one partial
        links = [f"link{i}" for i in range(1, 8)] + ["end-effector", "end-effector"]
        pairs = [(0, 4), (0, 5), (1, 6), (2, 8), (0, 7)]
    elif name == "chain30w":         # 32 spheres, two of them on the welded bracket
        links = [f"link{i}" for i in range(1, 31)] + ["bracket", "bracket"]
        pairs = [(i, i + 9) for i in range(20)]
    else:                            # 18 spheres; 8 x 8 = 64 pairs between the arms; the torso is the fixed base of the forest
        arm = [f"link{i}" for i in range(1, 8)] + ["end-effector"]
        links = ["left_" + l for l in arm] + ["right_" + l for l in arm] + ["torso", "shoulders" if name == "tree" else "torso"]
        pairs = [(i, 8 + j) for i in range(8) for j in range(8)]
    order = rng.permutation(len(links))              # not sorted by body: the engine sorts, the item numbers keep the caller's order
    inv = np.argsort(order)
    sph = [(links[i], rng.uniform(-0.04, 0.04, 3), float(rng.uniform(0.02, 0.07))) for i in order]
    return sph, np.array([(inv[a], inv[b]) for a, b in pairs], int)


def _case(name, B, ld, seed=3):
    """(robot, ctrl, spheres, pairs) at a random state"""
    from sai_primitives_amd.controller import controller_from_specs
    rng = np.random.default_rng(seed)
    if name in ("tree", "forest"):
        desc = TR.dual_panda_torso() if name == "tree" else TR.dual_panda_fixed_torso()
        m = W.RobotModel(desc)
        specs = TR.dual_stack(m)
    elif name == "chain30w":
        desc = _chain30w()
        m, specs = W.RobotModel(desc), W.make_inputs(5, B)["tasks"]
    else:
        d = W.make_inputs(2, B)
        desc, m, specs = d["model"].name, d["model"], d["tasks"]
    q = np.clip(rng.uniform(-1.2, 1.2, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    robot, ctrl, objs = controller_from_specs(desc, specs, B, device=0, leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(np.zeros((B, m.dof)))
    robot.updateModel()
    sph, pairs = _spheres(name, rng)
    return robot, ctrl, sph, pairs


def _query_centres(robot, sph):
    """(B, S, 3) from the engine's model queries, eight frames at a time"""
    out = np.empty((robot.batch_size, len(sph), 3))
    for i in range(0, len(sph), 8):
        fr = robot._frames([(l, tuple(c)) for l, c, _ in sph[i:i + 8]], 0)
        out[:, i:i + 8] = fr[:, 0:3].transpose(2, 0, 1)
    return out


def _obstacles(rng, centres, O, per_instance):
    """O obstacles of mixed kinds through the cloud of centres: (O, 8) or (O, B, 8)"""
    B = centres.shape[0]
    lo, hi = centres.reshape(-1, 3).min(axis=0), centres.reshape(-1, 3).max(axis=0)
    shape = (O, B) if per_instance else (O,)
    ob = np.zeros(shape + (8,))
    ob[..., 1:4] = rng.uniform(lo, hi, shape + (3,))
    ob[..., 4:7] = ob[..., 1:4] + rng.uniform(-0.3, 0.3, shape + (3,))
    ob[..., 7] = rng.uniform(0.0, 0.08, shape)
    kind = np.arange(O) % 4
    sel = np.broadcast_to((kind == 1).reshape((O,) + (1,) * (len(shape) - 1)), shape)          # every fourth a sphere (a == b)
    ob[..., 4:7] = np.where(sel[..., None], ob[..., 1:4], ob[..., 4:7])
    hs = np.broadcast_to((kind == 3).reshape((O,) + (1,) * (len(shape) - 1)), shape)           # every fourth a half-space
    n = rng.normal(size=shape + (3,))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    off = (n * rng.uniform(lo, hi, shape + (3,))).sum(axis=-1) - 0.3
    ob[..., 0] = hs
    ob[..., 1:4] = np.where(hs[..., None], n, ob[..., 1:4])
    ob[..., 4] = np.where(hs, off, ob[..., 4])
    return ob


def _ref_obst(ob, per_instance):
    return ob.transpose(1, 0, 2) if per_instance else ob


class _Outputs:
    """the device outputs of an attachment with the padding columns pre-filled with a sentinel"""

    def __init__(self, ctrl, S, ld, keep):
        from sai_primitives_amd import capi
        L = capi.lib()
        ctrl.synchronize()
        self.ctrl, self.B, self.ld = ctrl, ctrl.batch_size, ld
        self.bufs = dict(readout=(L.saip_batch_clearance_readout_device(ctrl._h), 8), summary=(L.saip_batch_clearance_summary_device(ctrl._h), 4))
        if keep:
            self.bufs["centres"] = (L.saip_batch_clearance_centres_device(ctrl._h), 3 * S)
        for ptr, rows in self.bufs.values():
            assert ptr
            a = _d2h(ptr, (rows, ld))
            a[:, self.B:] = SENTINEL
            _h2d(ptr, a)

    def get(self, key):
        self.ctrl.synchronize()
        ptr, rows = self.bufs[key]
        a = _d2h(ptr, (rows, self.ld))
        assert (a[:, self.B:] == SENTINEL).all(), key          # columns B..ld-1 are never written
        return a[:, :self.B]

    def centres(self):
        c = self.get("centres")
        return np.ascontiguousarray(c.T.reshape(self.B, -1, 3))

    def readout(self):
        return np.ascontiguousarray(self.get("readout").T)

    def summary(self):
        return np.ascontiguousarray(self.get("summary").T)


def _same(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


# ------------------------------------------------------------------ 1. centres against the engine's own FK
@pytest.mark.parametrize("name,B,ld", [(n, *SHAPES[i % 3]) for i, n in enumerate(MODELS)] + [("chain30w", 3, 64), ("tree", 3, 64)])
def test_centres_match_the_model_queries(sp, name, B, ld):
    robot, ctrl, sph, pairs = _case(name, B, ld)
    ctrl.attachClearance(sph, pairs=pairs, margin=0.05, keep_centres=True)
    out = _Outputs(ctrl, len(sph), ld, True)
    ctrl.evaluateClearance()
    got, want = out.centres(), _query_centres(robot, sph)
    worst = np.abs(got - want).max()
    WORST[(name, B)] = worst
    print(f"{name} B={B}: worst |centre - model query| = {worst:.3e} m over {len(sph)} spheres (largest coordinate {np.abs(want).max():.2f} m)")
    assert worst <= CENTRE_BOUND
    assert np.abs(want).max() > 0.3 and np.ptp(want[:, :, 2]) > 0.1         # the spheres are spread over the robot
    info = ctrl.clearanceInfo()
    assert (info["n_spheres"], info["n_obstacles"], info["n_pairs"], info["keep_centres"], info["period"]) == (len(sph), 0, len(pairs), True, 0)
    ctrl.detachClearance()


# ------------------------------------------------------------------ 2. the distance stage bit for bit
@pytest.mark.parametrize("name,B,ld", [(n, *SHAPES[(i + 1) % 3]) for i, n in enumerate(MODELS)] + [("panda_arm", 3, 64), ("tree", 65, 128)])
def test_distance_stage_bit_for_bit(sp, name, B, ld):
    robot, ctrl, sph, pairs = _case(name, B, ld, seed=4)
    radii = np.array([r for _, _, r in sph])
    rng = np.random.default_rng(17)
    cloud = _query_centres(robot, sph)
    for per in (False, True):
        ob = _obstacles(rng, cloud, 16, per)
        ctrl.attachClearance(sph, ob, pairs=pairs, margin=0.06, per_instance=per, keep_centres=True)
        out = _Outputs(ctrl, len(sph), ld, True)
        for again in (False, True):
            if again:
                ob = _obstacles(rng, cloud, 16, per)
                ctrl.setClearanceObstacles(ob)
            ctrl.evaluateClearance()
            ro, c = out.readout(), out.centres()
            want = CL.evaluate(c, radii, _ref_obst(ob, per), pairs, 0.06)
            assert _same(ro, want), (name, per, again, np.argwhere(ro != want)[:5])
            assert (ro[:, 3] > 0).any() and (ro[:, 0] < 0).any() and np.isfinite(ro).all()
            face = ctrl.clearanceReadout()
            assert _same(face["distance"], want[:, 0]) and _same(face["point"], want[:, 4:7]) and _same(face["pair_distance"], want[:, 7])
            assert face["closest"] == [CL.decode(k, len(sph), 16, pairs) for k in want[:, 1]]
        assert _same(out.summary(), CL.summary_reset(B))                       # evaluate leaves the summaries alone
        ctrl.detachClearance()


# ------------------------------------------------------------------ 3. end to end without keep_centres
@pytest.mark.parametrize("name,B,ld", [(n, *SHAPES[(i + 2) % 3]) for i, n in enumerate(MODELS)])
def test_end_to_end_against_the_model_queries(sp, name, B, ld):
    robot, ctrl, sph, pairs = _case(name, B, ld, seed=6)
    radii = np.array([r for _, _, r in sph])
    rng = np.random.default_rng(23)
    cloud = _query_centres(robot, sph)
    ob = _obstacles(rng, cloud, 16, True)
    # the index can only be compared where the minimum is not a near-tie: in the restatement alone, every instance's runner-up lies more
    # than 1e-9 behind its minimum (a thousand times the bound on the centres)
    d = np.sort(CL.item_distances(cloud, radii, _ref_obst(ob, True), pairs), axis=1)
    assert (d[:, 1] - d[:, 0] > 1e-9).all(), (d[:, 1] - d[:, 0]).min()
    want = CL.evaluate(cloud, radii, _ref_obst(ob, True), pairs, 0.06)
    ctrl.attachClearance(sph, ob, pairs=pairs, margin=0.06, per_instance=True)
    assert ctrl.clearanceCentresDevice() is None
    out = _Outputs(ctrl, len(sph), ld, False)
    ctrl.evaluateClearance()
    ro = out.readout()
    err = np.abs(ro[:, 0] - want[:, 0]).max()
    print(f"{name} B={B}: worst |dmin - restatement at the queried centres| = {err:.3e} m")
    assert err <= CENTRE_BOUND and np.array_equal(ro[:, 1], want[:, 1])
    assert np.abs(ro[:, 4:7] - want[:, 4:7]).max() <= CENTRE_BOUND
    ctrl.detachClearance()


# ------------------------------------------------------------------ 4. rollout
def _panda_monitored(B, ld, attach=True, margin=0.05, q=None):
    """config 2's stack on the Panda with five spheres and a floor placed so that a fifth of the instances start inside it"""
    robot, ctrl, objs, mf, grav = _panda(B, False, ld=ld, q=q)
    sph = [("link4", (0.0, 0.0, 0.0), 0.06), ("link5", (0.0, 0.02, -0.1), 0.05), ("link6", (0.0, 0.0, 0.0), 0.05), ("link7", (0.0, 0.0, 0.05), 0.04),
           ("end-effector", (0.0, 0.0, 0.03), 0.04)]
    good = np.isfinite(robot._q).all(axis=1)
    z = _query_centres(robot, sph)[good, 4, 2] - 0.04
    floor = np.array([[1, 0.0, 0.0, 1.0, np.quantile(z, 0.2), 0, 0, 0], [0, 0.3, 0.0, 0.9, 0.5, 0.0, 0.9, 0.02]])
    if attach:
        ctrl.attachClearance(sph, floor, pairs=[(0, 4)], margin=margin)
    return robot, ctrl, mf, sph, floor


@pytest.mark.parametrize("B,ld", SHAPES)
def test_rollout_summaries_equal_the_host_driven_loop(sp, B, ld):
    K, T, margin = 6, DT * SUB, 0.05
    # a: one call of K periods
    robot, ctrl, mf, sph, floor = _panda_monitored(B, ld)
    out = _Outputs(ctrl, len(sph), ld, False)
    ctrl.recordRollouts(K, 1, ("q", "tau"), task=mf, summaries=True)
    ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
    got = out.summary()
    assert ctrl.clearanceInfo()["period"] == K
    end_a = (ctrl.pullState()[0].copy(), ctrl.pullState()[1].copy(), ctrl.getTorques(), ctrl.rolloutLog(), ctrl.rolloutSummary())
    # b: K host-driven periods, each followed by an evaluation, folded by the restatement
    robot2, ctrl2, mf2, _, _ = _panda_monitored(B, ld)
    out2 = _Outputs(ctrl2, len(sph), ld, False)
    s = CL.summary_reset(B)
    radii = np.array([r for _, _, r in sph])
    entered = np.zeros(B, bool)
    for p in range(K):
        ctrl2.rolloutAsync(1, DT, SUB, gravity=GRAV)
        mon = out2.readout()                                                 # of the period's own launch
        ctrl2.evaluateClearance()
        ro = out2.readout()
        assert _same(ro, mon)
        s = CL.summary_advance(s, T, ro[:, 0], ro[:, 2], p)
        # the host-side recomputation from the state: the same minimum within the bound of the centres
        ctrl2.pullState()                                                    # (mirrors q and dq into the robot: nothing is pushed back)
        robot2.updateModel()
        rec = CL.evaluate(_query_centres(robot2, sph), radii, floor, [(0, 4)], margin)
        assert np.abs(rec[:, 0] - ro[:, 0]).max() <= CENTRE_BOUND
        entered |= rec[:, 0] < margin - CENTRE_BOUND
    hit = s[:, 0] < 0
    print(f"B={B}: {entered.sum()} instances under the margin, {hit.sum()} penetrate, first periods {sorted(set(s[:, 3].astype(int)))}")
    assert entered.any() and not entered.all() and hit.any() and (rec[:, 0] < -CENTRE_BOUND).any()
    assert np.array_equal(got[:, [0, 2, 3]], s[:, [0, 2, 3]]) and _same(got[:, 1], s[:, 1])
    assert _same(out2.summary(), got)
    assert (got[hit, 3] >= 0).all() and (got[~hit, 3] == -1).all() and (got[:, 1] > 0).any()
    face = ctrl.clearanceSummary()
    assert _same(face["min_distance"], got[:, 0]) and np.array_equal(face["first_collision"], got[:, 3].astype(int))
    # c: the same rollout without the attachment: torques, state and the recorder's log are the same bits
    robot3, ctrl3, mf3, _, _ = _panda_monitored(B, ld, attach=False)
    ctrl3.recordRollouts(K, 1, ("q", "tau"), task=mf3, summaries=True)
    ctrl3.rolloutAsync(K, DT, SUB, gravity=GRAV)
    ctrl3.synchronize()
    end_c = (ctrl3.pullState()[0], ctrl3.pullState()[1], ctrl3.getTorques(), ctrl3.rolloutLog(), ctrl3.rolloutSummary())
    assert _same_bits(end_a[0], end_c[0]) and _same_bits(end_a[1], end_c[1]) and _same_bits(end_a[2], end_c[2]) and _same_bits(end_a[4], end_c[4])
    for key in ("q", "tau"):
        assert _same_bits(end_a[3][key], end_c[3][key]), key
    assert np.array_equal(end_a[3]["status"], end_c[3]["status"])
    # reset
    ctrl.resetClearanceSummary()
    assert _same(out.summary(), CL.summary_reset(B)) and ctrl.clearanceInfo()["period"] == 0
    ctrl.rolloutAsync(1, DT, SUB, gravity=GRAV)
    assert set(out.summary()[:, 3]) <= {-1.0, 0.0}                              # the index counts from the reset


# ------------------------------------------------------------------ 5. sampler
@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_clearance_cost_and_the_sampler(sp, B, ld):
    K = 6
    for nan_col in (None, 5):
        q = W.make_inputs(2, B)["q"].copy()
        if nan_col is not None:
            q[nan_col, 2] = np.nan
        robot, ctrl, mf, sph, floor = _panda_monitored(B, ld, q=q)
        out = _Outputs(ctrl, len(sph), ld, False)
        good = np.isfinite(q).all(axis=1)
        p0 = mf._get_goal()[np.flatnonzero(good)[0], :3]
        nominal = np.tile(p0, (2, 1))                                          # every instance is sent to the first one's goal
        mf.setGoalSchedule("position", np.repeat(nominal[:, None], B, axis=1), stride=3, mode="linear")
        mf.attachSampler(0.01, nominal=nominal, exempt=0)
        ctrl.recordRollouts(K, 1, ("pose",), task=mf)
        ctrl.seedSampler(7)
        ctrl.perturbGoalSchedules()
        ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
        ctrl.rolloutCost(target=p0, final_weight=1.0)
        cost0 = ctrl.getRolloutCost()
        s = out.summary()
        if nan_col is not None:
            assert np.isnan(s[nan_col, 0]) and np.isnan(s[nan_col, 1]) and np.isfinite(s[good]).all()
        ctrl.clearanceCost(3.0, 50.0, 0.01)
        cost1 = ctrl.getRolloutCost()
        assert _same(cost1, CL.add_cost(cost0, s[:, 0], s[:, 1], 3.0, 50.0, 0.01))
        if nan_col is not None:
            assert np.isnan(cost1[nan_col]) and np.isfinite(cost1[good]).all()
            continue
        assert (cost1 > cost0).any() and (cost1 == cost0).any()
        # a hard constraint
        ctrl.setRolloutCost(cost0)
        ctrl.clearanceCost(0.0)
        cost2 = ctrl.getRolloutCost()
        hit = s[:, 0] < 0
        assert hit.any() and not hit.all() and np.isinf(cost2[hit]).all() and _same(cost2[~hit], cost0[~hit])
        ctrl.updateSampler(1e-3)
        res = ctrl.samplerResult()
        assert res["n_valid"] == B - hit.sum() and not hit[res["best"]] and res["best"] == int(np.argmin(np.where(hit, np.inf, cost0)))


# ------------------------------------------------------------------ 6. without an attachment
def test_without_an_attachment(sp):
    from sai_primitives_amd import capi
    robot, ctrl, objs, mf, grav = _panda(3, False)
    L = capi.lib()
    out = np.full(8 * 3, 7.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    for fn, args in (("detach", ()), ("info", (None,) * 7), ("set_obstacles_host", (dp,)), ("evaluate", ()), ("readout_host", (dp,)),
                     ("summary_host", (dp,)), ("summary_reset", ()), ("add_cost", (1.0, 1.0, 0.0))):
        assert getattr(L, "saip_batch_clearance_" + fn)(ctrl._h, *args) == capi.SAIP_ERR_ORDER, fn
        assert b"no clearance monitor is attached" in L.saip_last_error()
    for fn in ("obstacles", "readout", "summary", "centres"):
        assert getattr(L, f"saip_batch_clearance_{fn}_device")(ctrl._h) is None
    assert (out == 7.0).all()
    # attached, but no sampler: the cost has nowhere to go
    ctrl.attachClearance([("link4", (0, 0, 0), 0.05)], np.array([[1, 0, 0, 1.0, 0, 0, 0, 0]], float))
    with pytest.raises(sp.SaipError, match="no sampler is attached"):
        ctrl.clearanceCost(1.0)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachClearance([("link4", (0, 0, 0), 0.05)], np.array([[1, 0, 0, 1.0, 0, 0, 0, 0]], float))
    assert L.saip_batch_clearance_obstacles_device(ctrl._h) and L.saip_batch_clearance_centres_device(ctrl._h) is None
    ctrl.detachClearance()
    assert L.saip_batch_clearance_readout_device(ctrl._h) is None
