"""Scenario groups of the resident rollout sampler on the device (saip_batch_sampler_set_scenarios and its neighbours, csrc/saip_sampler.hip)
on the Panda stack of tests/test_gpu_sampler.py: a batch of B = C * M instances as M scenario blocks of C candidate plans.  (C, M) = (35, 2)
gives B = 70, no multiple of 64, with padding columns behind it; (300, 3) gives B = 900 and more candidates than the 256 lanes of the weights
kernel.  Everything is compared bit for bit: against the NumPy restatement tests/sampler_scenarios_ref.py where only sums, comparisons and one
division are involved (the group cost, the best map), and against an ungrouped controller of batch C, which runs the same kernels on the
same numbers, where a maths library is involved (keyframes, weights, nominal, result)."""
import gc

import numpy as np
import pytest

import inertia_ref as IR
import plant_chain_ref as PC
import plant_ref as PR
import sampler_ref as SR
import sampler_scenarios_ref as SS
import workloads as W
from test_gpu_batch_layout import _d2h, _h2d, _same_bits
from test_gpu_rollout_record import _panda
from test_gpu_sampler import DT, GRAV, K, SENTINEL, SUB, _attach, _fill_padding, _keys, _ld, _nominal

pytestmark = pytest.mark.gpu

SHAPES = [(35, 2), (300, 3)]
RISKS = [("mean", None), ("max", None), ("cvar", 0.6)]          # alpha = 0.6: the two worst scenarios of two and of three


@pytest.fixture(autouse=True)
def _release_device_memory():
    """a controller, its robot and its tasks refer to each other, so the batches of a test (B = 900 among them) are freed by the cycle
    collector only, whenever it next runs: later tests that compare free device memory would see them go.  Collect them here."""
    yield
    gc.collect()


def _lib():
    from sai_primitives_amd import capi
    return capi.lib()


def _blocks(a, Cn, M):
    """(..., C * M) -> (M, ..., C)"""
    return np.stack([a[..., s * Cn:(s + 1) * Cn] for s in range(M)])


# ------------------------------------------------------------------ 1. perturb
@pytest.mark.parametrize("Cn,M", SHAPES)
def test_perturb_keys_the_noise_by_the_candidate(Cn, M):
    B, exempt, seed = Cn * M, 2, 0xfeedc0de1234 + Cn
    rng = np.random.default_rng(41 + Cn)
    _, grouped, (mf, jt), _, _ = _panda(B, False)
    _, single, (mf1, jt1), _, _ = _panda(Cn, False)
    nom, sigma = _nominal(mf, rng, 12), rng.uniform(0.01, 0.1, 6)
    nomj, sigj = _nominal(jt, rng, 7), rng.uniform(0.01, 0.1, 7)
    for ctrl, a, b in ((grouped, mf, jt), (single, mf1, jt1)):
        _attach(a, ctrl, 0, 12, nom, sigma, exempt)
        _attach(b, ctrl, 0, 7, nomj, sigj, exempt)
        ctrl.seedSampler(seed)
        _fill_padding(a, ctrl, 12)
        _fill_padding(b, ctrl, 7)
    grouped.setSamplerScenarios(M, "max")
    assert grouped.samplerScenarios() == dict(n_scenarios=M, n_candidates=Cn, risk="max", tail=0)
    for ctrl in (grouped, single):
        ctrl.perturbGoalSchedules()
        ctrl.perturbGoalSchedules()                       # the keyframes are those of round 1
    for (tg, ts), cnt, nm in (((mf, mf1), 12, nom), ((jt, jt1), 7, nomj)):
        dev, ref = _keys(tg, grouped, cnt), _keys(ts, single, cnt)
        assert (dev[:, :, B:] == SENTINEL).all() and (ref[:, :, Cn:] == SENTINEL).all()
        blocks = _blocks(dev[:, :, :B], Cn, M)
        for s in range(M):
            assert _same_bits(blocks[s], blocks[0]), s                                   # every scenario block is block 0
            assert _same_bits(np.ascontiguousarray(blocks[s][:, :, :exempt]), np.ascontiguousarray(np.broadcast_to(nm[:, :, None], (K, cnt, exempt))))
        assert _same_bits(blocks[0], np.ascontiguousarray(ref[:, :, :Cn]))                # ... and the ungrouped batch of C
        assert np.abs(blocks[0][:, :, exempt:] - nm[:, :, None]).max() > 1e-3


# ------------------------------------------------------------------ 2. group cost and update from uploaded costs
def _costs(rng, Cn, M):
    v = rng.uniform(1.0, 3.0, (M, Cn))
    v[0, 3], v[M - 1, 5], v[0, 7] = np.inf, -np.inf, np.nan
    v[:, 9] = [np.nan, np.inf, -np.inf][:M]             # every scenario of one candidate
    v[:, 11] = 1.25
    v[:, 20] = rng.uniform(-2.0, -1.0, M)
    v[:, Cn - 2] = rng.uniform(-3.2, -3.1, M)           # the best sits in the last lanes' share
    return v.reshape(-1)


@pytest.mark.parametrize("Cn,M", SHAPES)
def test_group_cost_and_update_from_uploaded_costs(Cn, M):
    L = _lib()
    B = Cn * M
    rng = np.random.default_rng(43 + Cn)
    _, grouped, (mf, jt), _, _ = _panda(B, False)
    _, single, (mf1, jt1), _, _ = _panda(Cn, False)
    nom, sigma = _nominal(mf, rng, 12), rng.uniform(0.01, 0.1, 6)
    _attach(mf, grouped, 0, 12, nom, sigma, 1)
    grouped.setSamplerScenarios(M)
    grouped.seedSampler(9)
    grouped.perturbGoalSchedules()
    ld, ld1 = _ld(grouped), _ld(single)
    keys = _keys(mf, grouped, 12)[:, :, :B]                                # (K, 12, B)
    mf1.setGoalSchedule((0, 12), np.ascontiguousarray(keys[:, :, :Cn].transpose(0, 2, 1)))
    mf1.attachSampler(sigma, nominal=nom, exempt=1)
    h, h1 = grouped._h, single._h
    ptrs = dict(cost=L.saip_batch_sampler_cost_device(h), group=L.saip_batch_sampler_group_cost_device(h), w=L.saip_batch_sampler_weights_device(h),
                map=L.saip_batch_sampler_best_map_device(h))
    assert ptrs["group"] != ptrs["cost"] and L.saip_batch_sampler_group_cost_device(h1) == L.saip_batch_sampler_cost_device(h1)
    for name in ("cost", "group", "w"):
        _h2d(ptrs[name], np.full(ld, SENTINEL))
    _h2d(ptrs["map"], np.full(ld, 12345, np.int32))
    costs = _costs(rng, Cn, M)
    for (risk, alpha), T in [(r, T) for r in RISKS for T in (0.4, 1e-300)]:
        grouped.setSamplerScenarios(M, risk, alpha)
        tail = SS.tail_of(M, alpha) if risk == "cvar" else 0
        assert grouped.samplerScenarios() == dict(n_scenarios=M, n_candidates=Cn, risk=risk, tail=tail)
        mf.setSamplerNominal(nom)
        grouped.setRolloutCost(costs)
        grouped.updateSampler(T)
        g = grouped.samplerGroupCost()
        want = SS.group_cost(costs, Cn, M, risk, tail)
        assert _same_bits(g, want), (risk, g, want)
        assert np.isposinf(g[[3, 5, 7, 9]]).all() and np.isfinite(np.delete(g, [3, 5, 7, 9])).all()
        res = grouped.samplerResult()
        mf1.setSamplerNominal(nom)
        single.setRolloutCost(g)
        single.updateSampler(T)
        assert res == single.samplerResult() and res["best"] == Cn - 2 and res["n_valid"] == Cn - 4
        assert _same_bits(mf.samplerNominal(), mf1.samplerNominal()) and not _same_bits(mf.samplerNominal(), nom)
        w, w1 = _d2h(ptrs["w"], (ld,)), _d2h(L.saip_batch_sampler_weights_device(h1), (ld1,))
        assert _same_bits(w[:Cn], w1[:Cn]) and w[:Cn].max() == 1.0
        m = _d2h(ptrs["map"], (ld,), np.int32)
        assert np.array_equal(m[:B], SS.best_map(B, Cn, res["best"])) and np.array_equal(m[:B], (np.arange(B) // Cn) * Cn + res["best"])
        # the padding of cost, group cost, weights and map
        assert (_d2h(ptrs["cost"], (ld,))[B:] == SENTINEL).all() and (_d2h(ptrs["group"], (ld,))[Cn:] == SENTINEL).all()
        assert (w[Cn:] == SENTINEL).all() and (m[B:] == 12345).all()
        assert _same_bits(grouped.getRolloutCost(), costs)                 # the per-instance costs stay what they were
    # CVAR over one scenario is MAX
    out = {}
    for risk, alpha in (("max", None), ("cvar", 1e-6)):
        grouped.setSamplerScenarios(M, risk, alpha)
        mf.setSamplerNominal(nom)
        grouped.updateSampler(0.4)
        out[risk] = (grouped.samplerGroupCost(), mf.samplerNominal(), grouped.samplerResult())
    assert grouped.samplerScenarios()["tail"] == 1
    assert _same_bits(out["max"][0], out["cvar"][0]) and _same_bits(out["max"][1], out["cvar"][1]) and out["max"][2] == out["cvar"][2]
    # one bad scenario everywhere: no candidate is valid, nothing moves, the map holds -1
    bad = costs.reshape(M, Cn).copy()
    bad[M - 1] = np.nan
    mf.setSamplerNominal(nom)
    grouped.setRolloutCost(bad.reshape(-1))
    grouped.updateSampler(0.4)
    assert grouped.samplerResult() == dict(best=-1, n_valid=0, min_cost=0.0, sum_w=0.0, ess=0.0) and _same_bits(mf.samplerNominal(), nom)
    m = _d2h(ptrs["map"], (ld,), np.int32)
    assert (m[:B] == -1).all() and (m[B:] == 12345).all() and np.isposinf(grouped.samplerGroupCost()).all()


# ------------------------------------------------------------------ 3. one scenario is the ungrouped sampler
def test_one_scenario_is_the_ungrouped_sampler():
    L = _lib()
    B = 70
    rng = np.random.default_rng(45)
    out, nom = [], None
    for call_it in (False, True):
        _, ctrl, (mf, jt), _, _ = _panda(B, False)
        if nom is None:
            nom, sigma = _nominal(mf, rng, 12), rng.uniform(0.01, 0.05, 6)
            target = mf._get_goal()[0, :3] + np.array([0.03, -0.02, 0.04])
        _attach(mf, ctrl, 0, 12, nom, sigma, 1, mode="linear", stride=4)
        if call_it:
            ctrl.setSamplerScenarios(1)
            assert ctrl.samplerScenarios() == dict(n_scenarios=1, n_candidates=B, risk="mean", tail=0)
        ctrl.recordRollouts(4, 2, ("pose",), task=mf)
        ctrl.seedSampler(11)
        ctrl.perturbGoalSchedules()
        keys = _keys(mf, ctrl, 12)
        ctrl.rolloutAsync(8, DT, SUB, gravity=GRAV)
        ctrl.rolloutCost(target=target, path_weight=0.5, final_weight=1.0)
        ctrl.updateSampler(0.05)
        ctrl.synchronize()
        ld = _ld(ctrl)
        assert L.saip_batch_sampler_group_cost_device(ctrl._h) == L.saip_batch_sampler_cost_device(ctrl._h)
        assert _same_bits(ctrl.samplerGroupCost(), ctrl.getRolloutCost())
        out.append(dict(keys=keys, cost=ctrl.getRolloutCost(), nominal=mf.samplerNominal(), result=ctrl.samplerResult(),
                        map=_d2h(L.saip_batch_sampler_best_map_device(ctrl._h), (ld,), np.int32), w=_d2h(L.saip_batch_sampler_weights_device(ctrl._h), (ld,))))
    a, b = out
    assert a["result"] == b["result"] and a["result"]["n_valid"] == B and 1.0 < a["result"]["ess"] < B
    for name in ("cost", "nominal"):
        assert _same_bits(a[name], b[name]), name
    assert _same_bits(np.ascontiguousarray(a["keys"][:, :, :B]), np.ascontiguousarray(b["keys"][:, :, :B])) and _same_bits(a["w"][:B], b["w"][:B])
    assert np.array_equal(a["map"][:B], b["map"][:B]) and (a["map"][:B] == a["result"]["best"]).all()


# ------------------------------------------------------------------ 4. share tables
def _randomised(ctrl, B, sensing_chain_per_instance=True):
    """all five attachments, per instance, drawn on the device; dict name -> (device pointer, rows) of the arrays with an accessor"""
    n = 7
    ctrl.attachPlant(np.repeat(PR.neutral(n)[:, None], B, axis=1), wrenches=[("end-effector", (0, 0, 0.05), "world", np.zeros((B, 8)))], per_instance=True)
    ctrl.attachActuationChain(np.tile(PC.NEUTRAL, (n, B, 1)), per_instance=True, depth=2)
    ctrl.attachInertia(per_instance=True, payload_links=["end-effector"])
    ctrl.attachSensing(joints=dict(q_off=np.zeros((n, B))), per_instance=True)
    ctrl.attachSensingChain(dict(delay=np.zeros((n, B))) if sensing_chain_per_instance else dict(delay=1, a_q=0.25), per_instance=sensing_chain_per_instance, depth=2)
    lo, hi = PR.neutral(n), PR.neutral(n)
    lo[:, PR.GAIN], hi[:, PR.FV] = 0.5, 0.2
    ctrl.randomizePlant(71, 0, joints=(lo, hi), wrenches=(np.array([[-1.0] * 6 + [0.0, 50.0]]), np.array([[1.0] * 6 + [0.0, 50.0]])))
    ctrl.actuationChainRandomize(72, 0, np.tile([-0.4, 10.0, 0.0], (n, 1)), np.tile([2.4, 500.0, 0.01], (n, 1)))
    bl, bh = IR.neutral_bodies(n), IR.neutral_bodies(n)
    bl[:, 0], bh[:, 0] = 0.8, 1.2
    ctrl.randomizeInertia(73, 0, bodies=(bl, bh), payloads=(np.array([[0.0, 0, 0, 0, 0.01, 0.01, 0.01]]), np.array([[1.0, 0, 0, 0.05, 0.05, 0.05, 0.05]])))
    jl, jh = np.zeros((n, 6)), np.zeros((n, 6))
    jl[:, [0, 3]], jh[:, [0, 3]] = -1e-3, 1e-3
    ctrl.sensingRandomize(74, 0, joints=(jl, jh))
    if sensing_chain_per_instance:
        ctrl.sensingChainRandomize(75, 0, np.tile([-0.4, -0.4, 0.0, 0.0], (n, 1)), np.tile([2.4, 1.4, 0.5, 0.5], (n, 1)))
    tabs = dict(plant_joints=(ctrl.plantJointsDevice(), n * 10), plant_wrenches=(ctrl.plantWrenchesDevice(), 8), actuation_chain=(ctrl.actuationChainTableDevice(), n * 3),
                inertia_rows=(ctrl.inertiaRowsDevice(), n * 10), sensing_joints=(ctrl.sensingJointsDevice(), n * 6))
    if sensing_chain_per_instance:
        tabs["sensing_chain"] = (ctrl.sensingChainTableDevice(), n * 4)
    return tabs


def test_share_scenario_tables():
    Cn, M = 35, 2
    B = Cn * M
    rng = np.random.default_rng(47)
    _, ctrl, (mf, jt), _, _ = _panda(B, False)
    ld = _ld(ctrl)
    assert ld > B
    _attach(mf, ctrl, 0, 3, _nominal(mf, rng, 3), 0.02, 1)
    tabs = _randomised(ctrl, B)
    ctrl.synchronize()
    before = {}
    for name, (ptr, rows) in tabs.items():
        t = _d2h(ptr, (rows, ld))
        t[:, B:] = SENTINEL
        _h2d(ptr, t)
        before[name] = t
        assert (t[:, 1:B] != t[:, :1]).any(), name                          # the draw made the instances differ
    with pytest.raises(Exception, match="one scenario"):
        ctrl.shareScenarioTables()
    ctrl.setSamplerScenarios(M, "max")
    # the arrays touched: plant joints and wrenches, actuation chain, inertia part staging and composed rows, sensing joints, sensing chain
    assert ctrl.shareScenarioTables() == 7
    ctrl.synchronize()
    src = (np.arange(B) // Cn) * Cn
    for name, (ptr, rows) in tabs.items():
        t = _d2h(ptr, (rows, ld))
        assert _same_bits(np.ascontiguousarray(t[:, :B]), np.ascontiguousarray(before[name][:, src])), name      # column i is column (i // C) * C as it was
        assert (t[:, B:] == SENTINEL).all(), name
        assert not _same_bits(np.ascontiguousarray(t[:, 0]), np.ascontiguousarray(t[:, Cn])), name             # the scenarios still differ
    assert np.isfinite(ctrl.inertiaRows()).all()
    # the shared robots roll out: candidates of one scenario that hold the same plan move alike, the two scenarios do not
    ctrl.detachSensingChain()
    ctrl.detachSensing()                                                    # its noise and state stay per instance
    ctrl.rolloutAsync(4, DT, SUB, gravity=GRAV)
    ctrl.synchronize()
    q = ctrl.pullState()[0]
    assert np.isfinite(q).all()
    # a batch-uniform table is skipped and not counted
    ctrl.attachSensing(joints=dict(q_off=np.zeros((7, B))), per_instance=True)
    ctrl.attachSensingChain(dict(delay=1, a_q=0.25), depth=2)
    ctrl.synchronize()
    uniform = _d2h(ctrl.sensingChainTableDevice(), (7 * 4,))
    assert ctrl.shareScenarioTables() == 6
    ctrl.synchronize()
    assert _same_bits(_d2h(ctrl.sensingChainTableDevice(), (7 * 4,)), uniform)
    ctrl.detachPlant()                                                      # takes its chain along
    ctrl._call("saip_batch_sampler_share_scenario_tables", None)            # the count may be left out
    assert ctrl.shareScenarioTables() == 3                                   # inertia parts and rows, sensing joints


# ------------------------------------------------------------------ 5. the loop closes under randomisation
def test_the_planning_loop_closes_under_randomisation():
    Cn, M = 35, 2
    B, KL, STRIDE, PERIODS, ROUNDS = Cn * M, 4, 10, 40, 2
    rng = np.random.default_rng(49)
    q0 = np.repeat(W.make_inputs(2, B)["q"][:1], B, axis=0)                 # one measured state: the scenarios differ by their plant alone
    _, ctrl, (mf, jt), _, _ = _panda(B, False, q=q0)
    p0 = mf._get_goal()[0, :3] - np.array([0.04, -0.03, 0.05])
    target = p0 + np.array([0.03, -0.02, 0.04])
    stay = np.tile(p0, (KL, 1))
    mf.setGoalSchedule("position", np.repeat(stay[:, None], B, axis=1), stride=STRIDE, mode="linear")
    mf.attachSampler(0.02, nominal=stay, exempt=1)
    ctrl.setSamplerScenarios(M, "max")
    # a per-instance plant: every instance another actuator gain, scenario 0's source column the nominal gain 1, scenario 1's gain 0.5
    joints = np.repeat(PR.neutral(7)[:, None], B, axis=1)
    joints[:, :, PR.GAIN] = rng.uniform(0.3, 0.9, (7, B))
    joints[:, 0, PR.GAIN], joints[:, Cn, PR.GAIN] = 1.0, 0.5
    ctrl.attachPlant(joints, per_instance=True)
    assert ctrl.shareScenarioTables() == 1
    ctrl.recordRollouts(4, STRIDE, ("pose",), task=mf)
    ctrl.seedSampler(2027)
    src = ((np.arange(B) // Cn) * Cn).astype(np.int32)                       # every scenario block starts from its own instance 0
    s = ctrl.saveState()
    q_saved = ctrl.pullState()[0].copy()
    prev, worst = None, 0.0
    for r in range(ROUNDS):
        ctrl.restoreState(s, src)
        ctrl.rewindGoalSchedules()
        ctrl.resetRolloutRecorder()
        ctrl.setPlantPeriod(0)
        ctrl.perturbGoalSchedules()
        ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=GRAV)
        ctrl.rolloutCost(target=target, final_weight=1.0)
        cost = ctrl.getRolloutCost().reshape(M, Cn)
        ctrl.updateSampler(1e-300)
        res, g = ctrl.samplerResult(), ctrl.samplerGroupCost()
        best = res["best"]
        assert np.isfinite(cost).all() and res["n_valid"] == Cn
        assert _same_bits(g, 0.0 + cost.max(axis=0))                         # MAX: the larger of the two scenario costs ...
        assert g[best] == max(cost[0, best], cost[1, best]) == res["min_cost"] and best == int(np.argmin(g))    # ... also for the chosen candidate
        assert np.median(np.abs(cost[1] - cost[0])) > 1e-3 * cost.max()      # the weak actuators of scenario 1 are another robot
        if prev is not None:                                                 # candidate 0 ran the previous round's best plan in both scenarios
            diff = np.abs(cost[:, 0] - prev)
            worst = max(worst, diff.max())
            print(f"round {r}: cost of (s, 0) {cost[:, 0]}, cost of (s, best) the round before {prev}, worst difference {worst:.3g}")
            assert _same_bits(np.ascontiguousarray(cost[:, 0]), prev), (r, cost[:, 0], prev)
            assert res["min_cost"] <= prev.max()
        prev = np.ascontiguousarray(cost[:, best])
    m = _d2h(_lib().saip_batch_sampler_best_map_device(ctrl._h), (_ld(ctrl),), np.int32)[:B]
    assert np.array_equal(m, src + best)
    ctrl.restoreState(s, "best")                                             # every block takes its own copy of the best candidate
    ctrl.synchronize()
    assert _same_bits(ctrl.pullState()[0], np.ascontiguousarray(q_saved[src + best]))


# ------------------------------------------------------------------ 6. lifecycle
def test_lifecycle_and_an_idle_grouped_sampler():
    import sai_primitives_amd as sp
    Cn, M = 35, 2
    B = Cn * M
    rng = np.random.default_rng(51)
    logs, nom = [], None
    for sampled in (False, True):
        _, ctrl, (mf, jt), _, _ = _panda(B, False)
        if nom is None:
            nom = _nominal(mf, rng, 12)
            keys = SR.perturb(nom, np.full(6, 0.03), 3, 0, 0, B, 1, 3)
        mf.setGoalSchedule((0, 12), keys, stride=2, mode="linear")
        if sampled:
            mf.attachSampler(0.03, nominal=nom)
            ctrl.setSamplerScenarios(M, "cvar", 0.5)
        ctrl.recordRollouts(6, 1, ("q", "dq", "tau", "error"), task=mf)
        ctrl.rolloutAsync(6, DT, SUB, gravity=GRAV)
        ctrl.synchronize()
        logs.append(ctrl.rolloutLog())
    for name in ("q", "dq", "tau", "position_error", "orientation_error"):                # state, torque ...
        assert _same_bits(logs[0][name], logs[1][name]), name
    assert np.array_equal(logs[0]["status"], logs[1]["status"])                          # ... and status
    assert ctrl.samplerScenarios() == dict(n_scenarios=M, n_candidates=Cn, risk="cvar", tail=1)
    # exempt > C: refused by a later attach ...
    jt.setGoalSchedule("position", np.zeros((K, B, 7)))
    with pytest.raises(ValueError, match=f"exempt = {Cn + 1} outside 0 .. {Cn}"):
        jt.attachSampler(0.1, exempt=Cn + 1)
    jt.attachSampler(0.1, exempt=Cn)
    jt.detachSampler()
    # ... and by set_scenarios, which changes nothing then
    ctrl.setSamplerScenarios(1)
    jt.attachSampler(0.1, exempt=Cn + 1)
    with pytest.raises(ValueError, match=f"exempt = {Cn + 1}"):
        ctrl.setSamplerScenarios(M)
    assert ctrl.samplerScenarios() == dict(n_scenarios=1, n_candidates=B, risk="mean", tail=0)
    with pytest.raises(sp.SaipError, match="one scenario"):
        ctrl.shareScenarioTables()
    jt.detachSampler()
    ctrl.setSamplerScenarios(M, "max")
    # detaching the last sampler resets the setting
    mf.detachSampler()
    with pytest.raises(sp.SaipError, match="no sampler"):
        ctrl.samplerScenarios()
    mf.attachSampler(0.03, nominal=nom)
    assert ctrl.samplerScenarios() == dict(n_scenarios=1, n_candidates=B, risk="mean", tail=0)
    for bad in (0, 65, 4):                                                   # 70 instances are no multiple of 4
        with pytest.raises(ValueError, match=f"n_scenarios = {bad}"):
            ctrl.setSamplerScenarios(bad)
