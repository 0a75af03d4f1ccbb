"""Resident rollout sampler on the device (csrc/saip_sampler.hip, saip_batch_sampler_*) against the NumPy restatement tests/sampler_ref.py
on the Panda with the motion-force + joint stack of config 2 and per-instance goal schedules.  B = 70 is no multiple of 64 and its
leading dimension leaves a padding tail; B = 300 makes the 256-stride loops of the update run twice with a ragged second pass; B = 1 once.
The bounds are the derived ones of tests/test_sampler_cpu.py (kernel and restatement run the same operations in the same order and
differ by their maths libraries only); the device may use 64 x a derived bound and never more than 1e-11."""
import numpy as np
import pytest

import goal_schedule_ref as GS
import sampler_ref as SR
from test_gpu_batch_layout import _d2h, _h2d, _same_bits
from test_gpu_rollout_record import _panda
from test_sampler_cpu import linear_bound, mean_bound, perturbed_rotation_bound, rotation_mean_bound

pytestmark = pytest.mark.gpu

K = 3
SENTINEL = 6.02214076e23
CAP = 1e-11
DT, SUB = 5e-4, 2
GRAV = (0.0, 0.0, 0.0)


def _allowed(derived):
    return min(64 * derived, CAP)


def _ld(ctrl):
    return ctrl.devicePointers()["ld"]


def _nominal(task, rng, count, first=0):
    """(K, count) plan of goal rows [first, first + count) around instance 0's goal; the rotation (rows 3..11) moves 0.2 rad a keyframe"""
    g = task._get_goal()[0]
    nom = np.tile(g[first:first + count], (K, 1)) + rng.uniform(-0.02, 0.02, (K, count))
    if first == 0 and count >= 12:
        R = g[3:12].reshape(3, 3)
        for k in range(K):
            axis = rng.normal(size=3)
            R = R @ GS.exp_so3(axis / np.linalg.norm(axis) * 0.2)
            nom[k, 3:12] = R.reshape(9)
    return nom


def _attach(task, ctrl, first, count, nom, sigma, exempt, mode="hold", stride=1):
    B = ctrl.batch_size
    task.setGoalSchedule((first, count), np.repeat(nom[:, None], B, axis=1), stride=stride, mode=mode)
    task.attachSampler(sigma, nominal=nom, exempt=exempt)


def _keys(task, ctrl, count, Kf=K):
    """the resident keyframes (K, count, ld)"""
    ctrl.synchronize()
    return _d2h(task.goalScheduleDevice(), (Kf, count, _ld(ctrl)))


def _fill_padding(task, ctrl, count):
    B = ctrl.batch_size
    k = _keys(task, ctrl, count)
    k[:, :, B:] = SENTINEL
    _h2d(task.goalScheduleDevice(), k)


# ------------------------------------------------------------------ 1. perturb against the restatement
@pytest.mark.parametrize("B", [70, 300])
def test_perturb_matches_the_restatement(B):
    robot, ctrl, (mf, jt), _, _ = _panda(B, False)
    rng = np.random.default_rng(31 + B)
    seed, exempt = 0xfeedc0de1234 + B, 2
    worst = {}
    for first, count in [(0, 3), (0, 12), (12, 5)]:
        r_rot = 3 if count == 12 else None
        d = SR.dim(count, r_rot)
        nom, sigma = _nominal(mf, rng, count, first), rng.uniform(0.01, 0.1, d)
        nomj, sigj = _nominal(jt, rng, 7), rng.uniform(0.01, 0.1, 7)
        _attach(mf, ctrl, first, count, nom, sigma, exempt)
        _attach(jt, ctrl, 0, 7, nomj, sigj, exempt)
        info = mf.samplerInfo()
        assert (info["d"], info["exempt"]) == (d, exempt)
        ctrl.seedSampler(seed)
        _fill_padding(mf, ctrl, count)
        _fill_padding(jt, ctrl, 7)
        ctrl.perturbGoalSchedules()
        ctrl.perturbGoalSchedules()                       # the keyframes are those of the last round
        assert mf.samplerInfo()["round"] == 2 and mf.samplerInfo()["seed"] == seed
        for task, tid, cnt, nm, sg, rr in [(mf, 0, count, nom, sigma, r_rot), (jt, 1, 7, nomj, sigj, None)]:
            dev = _keys(task, ctrl, cnt)
            assert (dev[:, :, B:] == SENTINEL).all()
            got = dev[:, :, :B].transpose(0, 2, 1)
            ref = SR.perturb(nm, sg, seed, 1, tid, B, exempt, rr)
            assert _same_bits(got[:, :exempt], np.ascontiguousarray(np.broadcast_to(nm[:, None], (K, exempt, cnt))))
            rows, _ = SR.coords(cnt, rr)
            lin = np.abs(got[:, :, rows] - ref[:, :, rows]).max()
            worst[(tid, first, cnt, "linear")] = lin
            assert lin <= _allowed(linear_bound(sg.max(), np.abs(ref).max()))
            assert np.abs(got[:, exempt:, rows] - nm[:, None, rows]).max() > 1e-3
            if rr is not None:
                rot = np.abs(got[:, :, 3:12] - ref[:, :, 3:12]).max()
                worst[(tid, first, cnt, "rotation")] = rot
                assert rot <= _allowed(perturbed_rotation_bound(sg.max()))
                R = got[:, :, 3:12].reshape(K, B, 3, 3)
                assert np.abs(R.transpose(0, 1, 3, 2) @ R - np.eye(3)).max() <= 1e-12
        mf.clearGoalSchedule()
        jt.clearGoalSchedule()
    print(f"perturb B={B}: worst |device - NumPy| {worst}")


# ------------------------------------------------------------------ 2. the noise does not depend on the batch
def test_noise_does_not_depend_on_the_batch():
    rng = np.random.default_rng(32)
    out = {}
    nom = sigma = None
    for B in (70, 300):
        robot, ctrl, (mf, jt), _, _ = _panda(B, False)
        if nom is None:
            nom, sigma = _nominal(mf, rng, 12), rng.uniform(0.01, 0.1, 6)
        _attach(mf, ctrl, 0, 12, nom, sigma, 1)
        for name, seed, rounds in [("a", 77, 1), ("again", 77, 1), ("round", 77, 2), ("seed", 78, 1)]:
            ctrl.seedSampler(seed)
            for _ in range(rounds):
                ctrl.perturbGoalSchedules()
            out[(B, name)] = _keys(mf, ctrl, 12)[:, :, :B]
    assert _same_bits(out[(70, "a")], np.ascontiguousarray(out[(300, "a")][:, :, :70]))
    for B in (70, 300):
        assert _same_bits(out[(B, "a")], out[(B, "again")])
        assert not _same_bits(out[(B, "a")][:, :, 1:], out[(B, "round")][:, :, 1:]) and not _same_bits(out[(B, "a")][:, :, 1:], out[(B, "seed")][:, :, 1:])


# ------------------------------------------------------------------ 3. cost
def test_cost_equals_the_formula_bit_for_bit():
    B = 70
    robot, ctrl, (mf, jt), _, _ = _panda(B, False)
    rng = np.random.default_rng(33)
    ctrl.recordRollouts(4, 3, ("q", "pose"), task=mf, summaries=True)
    _attach(mf, ctrl, 0, 3, _nominal(mf, rng, 3), 0.02, 1)
    ctrl.seedSampler(5)
    ctrl.perturbGoalSchedules()
    from sai_primitives_amd import capi
    cost_ptr = capi.lib().saip_batch_sampler_cost_device(ctrl._h)
    ld = _ld(ctrl)
    with pytest.raises(Exception, match="at least one recorded sample"):
        ctrl.rolloutCost(target=np.zeros(3), final_weight=1.0)
    target = mf._get_goal()[0, :3] + np.array([0.03, -0.02, 0.04])
    w8 = np.array([0.5, 2.0, 0.0, 0.0, 1.0, 1e-3, 0.0, 10.0])
    for periods in (12, 3):                                # 4 samples fill the ring; 3 more periods wrap it
        ctrl.rolloutAsync(periods, DT, SUB, gravity=GRAV)
        ctrl.synchronize()
        _h2d(cost_ptr, np.full(ld, SENTINEL))
        S, pos = ctrl.rolloutSummary().T, ctrl.rolloutLog()["position"]
        assert pos.shape == (4, B, 3)
        for kw in [dict(summary_weights=w8), dict(target=target, path_weight=0.7, final_weight=3.0),
                   dict(summary_weights=w8, target=target, path_weight=0.7, final_weight=3.0), dict(target=target, final_weight=1.0)]:
            ctrl.rolloutCost(**kw)
            got = ctrl.getRolloutCost()
            want = SR.cost(B, S, kw.get("summary_weights"), pos, kw.get("target"), kw.get("path_weight", 0.0), kw.get("final_weight", 0.0))
            assert _same_bits(got, want), kw
            assert np.isfinite(got).all() and got.std() > 0
        assert (_d2h(cost_ptr, (ld,))[B:] == SENTINEL).all()


# ------------------------------------------------------------------ 4. update with uploaded costs
@pytest.mark.parametrize("B", [70, 300])
def test_update_with_uploaded_costs(B):
    from sai_primitives_amd import capi
    L = capi.lib()
    robot, ctrl, (mf, jt), _, _ = _panda(B, False)
    rng = np.random.default_rng(34 + B)
    nom, sigma = _nominal(mf, rng, 12), rng.uniform(0.01, 0.1, 6)
    _attach(mf, ctrl, 0, 12, nom, sigma, 1)
    ctrl.seedSampler(9)
    ctrl.perturbGoalSchedules()
    ld = _ld(ctrl)
    keys = _keys(mf, ctrl, 12)[:, :, :B].transpose(0, 2, 1)
    cost_ptr, map_ptr = L.saip_batch_sampler_cost_device(ctrl._h), L.saip_batch_sampler_best_map_device(ctrl._h)
    assert (_d2h(map_ptr, (ld,), np.int32) == -1).all()
    _h2d(cost_ptr, np.full(ld, SENTINEL))
    _h2d(map_ptr, np.full(ld, 12345, np.int32))

    def update(costs, temperature):
        mf.setSamplerNominal(nom)
        ctrl.setRolloutCost(costs)
        ctrl.updateSampler(temperature)
        res = ctrl.samplerResult()
        m = _d2h(map_ptr, (ld,), np.int32)
        assert (m[B:] == 12345).all() and (_d2h(cost_ptr, (ld,))[B:] == SENTINEL).all()      # padding
        assert (m[:B] == res["best"]).all()
        return res, mf.samplerNominal()

    j = B - 3
    costs = rng.uniform(1.0, 3.0, B)
    costs[j] = 0.5
    res, new = update(costs, 1e-300)                       # one-hot
    assert res == dict(best=j, n_valid=B, min_cost=0.5, sum_w=1.0, ess=1.0)
    assert _same_bits(new, np.ascontiguousarray(keys[:, j]))
    costs[7] = 0.5                                         # a tie: the lower index
    res, new = update(costs, 1e-300)
    assert (res["best"], res["sum_w"], res["ess"]) == (7, 2.0, 2.0)
    costs[7], costs[3], costs[11] = np.nan, -np.inf, np.inf          # invalid costs are excluded
    costs[40] = 0.25
    T = 0.4
    res, new = update(costs, T)                            # finite temperature
    w, ref = SR.weights(costs, T)
    assert (res["best"], res["n_valid"], res["min_cost"]) == (40, B - 3, 0.25) == (ref["best"], ref["n_valid"], ref["min_cost"])
    assert abs(res["sum_w"] - ref["sum_w"]) <= _allowed(mean_bound(B, 1.0)) * ref["sum_w"]
    assert abs(res["ess"] - ref["ess"]) <= 4 * _allowed(mean_bound(B, 1.0)) * ref["ess"] and 1.0 < res["ess"] < B
    want = SR.update(nom, keys, w, ref["best"], 3)
    lin = np.abs(new[:, :3] - want[:, :3]).max()
    rot = np.abs(new[:, 3:] - want[:, 3:]).max()
    lg = np.abs(SR.log_so3(nom[:, None, 3:].reshape(K, 1, 3, 3), keys[:, :, 3:].reshape(K, B, 3, 3))).max()
    print(f"update B={B}: worst |device - NumPy| linear {lin:.3g} rotation {rot:.3g}")
    assert lin <= _allowed(mean_bound(B, np.abs(keys[:, :, :3]).max())) and rot <= _allowed(rotation_mean_bound(B, lg))
    assert not _same_bits(new, nom)
    res, new = update(np.full(B, np.nan), T)               # no valid cost: nothing moves
    assert res == dict(best=-1, n_valid=0, min_cost=0.0, sum_w=0.0, ess=0.0) and _same_bits(new, nom)
    # refusals that need a sampler
    for bad in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="temperature"):
            ctrl.updateSampler(bad)
    with pytest.raises(ValueError, match="negative"):
        ctrl.shiftSampler(-1)
    with pytest.raises(Exception, match="already has a sampler"):
        mf.attachSampler(sigma)
    # orthonormality after 20 rounds
    mf.setSamplerNominal(nom)
    for r in range(20):
        ctrl.perturbGoalSchedules()
        ctrl.setRolloutCost(rng.uniform(0.0, 2.0, B))
        ctrl.updateSampler(0.3)
    R = mf.samplerNominal()[:, 3:].reshape(K, 3, 3)
    assert np.abs(R.transpose(0, 2, 1) @ R - np.eye(3)).max() <= 1e-12
    assert not _same_bits(mf.samplerNominal(), nom)


# ------------------------------------------------------------------ 5. shift, and one instance
def test_shift_and_a_single_exempt_instance():
    robot, ctrl, (mf, jt), _, _ = _panda(1, False)
    rng = np.random.default_rng(35)
    nom = _nominal(mf, rng, 12)
    _attach(mf, ctrl, 0, 12, nom, 0.05, 1)
    ctrl.seedSampler(1)
    ctrl.perturbGoalSchedules()
    ctrl.setRolloutCost(np.array([2.0]))
    ctrl.updateSampler(1.0)
    assert ctrl.samplerResult() == dict(best=0, n_valid=1, min_cost=2.0, sum_w=1.0, ess=1.0)
    assert _same_bits(mf.samplerNominal(), nom) and _same_bits(_keys(mf, ctrl, 12)[:, :, 0], nom)
    for n in (0, 1, 2, 5):
        mf.setSamplerNominal(nom)
        ctrl.shiftSampler(n)
        assert _same_bits(mf.samplerNominal(), SR.shift(nom, n)), n


# ------------------------------------------------------------------ 6. the loop closes
def test_the_planning_loop_closes():
    B, KL, STRIDE, PERIODS, ROUNDS, TOL = 70, 4, 10, 40, 5, 1e-5
    robot, ctrl, (mf, jt), _, _ = _panda(B, False)
    p0 = mf._get_goal()[0, :3] - np.array([0.04, -0.03, 0.05])       # instance 0's start position (_panda moved the goal by that much)
    target = p0 + np.array([0.03, -0.02, 0.04])
    stay = np.tile(p0, (KL, 1))
    mf.setGoalSchedule("position", np.repeat(stay[:, None], B, axis=1), stride=STRIDE, mode="linear")
    mf.attachSampler(0.02, nominal=stay, exempt=1)
    ctrl.recordRollouts(4, STRIDE, ("pose",), task=mf)
    ctrl.seedSampler(2026)
    s = ctrl.saveState()
    q_saved = ctrl.pullState()[0].copy()
    first_cost0, mins, worst = None, [], 0.0
    for r in range(ROUNDS):
        ctrl.restoreState(s, 0)
        ctrl.rewindGoalSchedules()
        ctrl.resetRolloutRecorder()
        ctrl.perturbGoalSchedules()
        ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=GRAV)
        ctrl.rolloutCost(target=target, final_weight=1.0)
        cost = ctrl.getRolloutCost()
        ctrl.updateSampler(1e-300)
        res = ctrl.samplerResult()
        assert res["n_valid"] == B and res["min_cost"] == cost.min() and res["best"] == int(np.argmin(cost))
        if r == 0:
            first_cost0 = cost[0]
        else:           # instance 0 ran the previous round's best keyframes from the same state
            rel = abs(cost[0] - mins[-1]) / mins[-1]
            worst = max(worst, rel)
            assert rel <= TOL, (r, cost[0], mins[-1])
            assert res["min_cost"] <= mins[-1] * (1 + TOL)
        mins.append(res["min_cost"])
    print(f"loop: cost[0] of round 0 {first_cost0:.6g}, minima {mins}, worst round-to-round relative difference {worst:.3g}")
    assert mins[-1] < first_cost0
    ctrl.restoreState(s, "best")
    ctrl.synchronize()
    q = ctrl.pullState()[0]
    assert _same_bits(q, np.ascontiguousarray(np.broadcast_to(q_saved[res["best"]], q.shape)))
    with pytest.raises(ValueError, match="unknown source"):
        ctrl.restoreState(s, "worst")


# ------------------------------------------------------------------ 7. nothing else moved
def test_an_idle_sampler_changes_nothing_and_the_lifecycle():
    B = 70
    rng = np.random.default_rng(37)
    logs, nom = [], None
    for sampled in (False, True):
        robot, ctrl, (mf, jt), _, _ = _panda(B, False)
        if nom is None:
            nom = _nominal(mf, rng, 12)
            keys = SR.perturb(nom, np.full(6, 0.03), 3, 0, 0, B, 1, 3)
        mf.setGoalSchedule((0, 12), keys, stride=2, mode="linear")
        if sampled:
            mf.attachSampler(0.03, nominal=nom)
        ctrl.recordRollouts(6, 1, ("q", "dq", "tau", "error"), task=mf)
        ctrl.rolloutAsync(6, DT, SUB, gravity=GRAV)
        ctrl.synchronize()
        logs.append(ctrl.rolloutLog())
    for name in ("q", "dq", "tau", "position_error", "orientation_error"):
        assert _same_bits(logs[0][name], logs[1][name]), name
    # refusals that need a schedule
    with pytest.raises(Exception, match="already has a sampler"):
        mf.attachSampler(0.03)
    jt.setGoalSchedule("position", np.zeros((K, 7)))                       # batch-uniform
    with pytest.raises(ValueError, match="batch-uniform"):
        jt.attachSampler(0.1)
    jt.clearGoalSchedule()
    jt.setGoalSchedule("position", np.zeros((K, B, 7)))                    # per-instance: only the exempt count is wrong
    for exempt in (-1, B + 1):
        with pytest.raises(ValueError, match="exempt"):
            jt.attachSampler(0.1, exempt=exempt)
    jt.clearGoalSchedule()
    # the schedule's detach takes the sampler along: every entry answers SAIP_ERR_ORDER, a later attach works again
    mf.clearGoalSchedule()
    import sai_primitives_amd as sp
    for fn in (ctrl.perturbGoalSchedules, lambda: ctrl.updateSampler(1.0), ctrl.samplerResult, ctrl.getRolloutCost, mf.detachSampler,
               lambda: ctrl.seedSampler(1), lambda: ctrl.shiftSampler(1), mf.samplerInfo, lambda: ctrl.setRolloutCost(np.zeros(B))):
        with pytest.raises(sp.SaipError, match="no sampler"):
            fn()
    assert not sp.capi.lib().saip_batch_sampler_cost_device(ctrl._h)
    mf.setGoalSchedule((0, 9), keys[:, :, :9])                             # rows 0..8: part of the rotation
    with pytest.raises(ValueError, match="all or none"):
        mf.attachSampler(0.1)
    mf.clearGoalSchedule()
    mf.setGoalSchedule("position", keys[:, :, :3])
    for bad in (-0.1, np.nan, np.inf):
        with pytest.raises(ValueError, match="negative or not finite"):
            mf.attachSampler(np.array([0.1, 0.1, bad]))
    mf.clearGoalSchedule()
    mf.setGoalSchedule((0, 12), keys)
    mf.attachSampler(0.03)                                                 # the nominal is instance 0's keyframes
    assert _same_bits(mf.samplerNominal(), np.ascontiguousarray(keys[:, 0]))
    ctrl.perturbGoalSchedules()
    got = _keys(mf, ctrl, 12)[:, :, :B].transpose(0, 2, 1)
    assert _same_bits(got[:, 0], np.ascontiguousarray(keys[:, 0])) and not _same_bits(got[:, 1:], np.ascontiguousarray(keys[:, 1:]))
    mf.detachSampler()
    assert mf.goalScheduleInfo()["count"] == 12                            # the schedule stays


# ------------------------------------------------------------------ 8. the row limit and the checks of the nominal plan
def test_row_limit_and_nominal_checks():
    from test_gpu_goal_schedule import _stack
    B = 5
    robot, ctrl, objs, _, _, _ = _stack("chain30", B)         # a 30-dof joint task: 90 goal rows
    jt = objs[2]
    rng = np.random.default_rng(38)
    jt.setGoalSchedule((0, 37), np.zeros((K, B, 37)))
    with pytest.raises(ValueError, match="at most 36"):
        jt.attachSampler(0.1)
    jt.clearGoalSchedule()
    nom = rng.uniform(-0.3, 0.3, (K, 36))                     # 36 rows are the most a sampler takes: every array of the kernels is full
    jt.setGoalSchedule((0, 36), np.repeat(nom[:, None], B, axis=1))
    sigma = rng.uniform(0.01, 0.1, 36)
    jt.attachSampler(sigma, nominal=nom, exempt=1)
    ctrl.seedSampler(4)
    ctrl.perturbGoalSchedules()
    keys = _keys(jt, ctrl, 36)[:, :, :B].transpose(0, 2, 1)
    ref = SR.perturb(nom, sigma, 4, 0, 2, B, 1)               # task id 2 is part of the counter
    assert _same_bits(keys[:, 0], nom) and np.abs(keys[:, 1:] - nom[:, None]).max() > 1e-3
    assert np.abs(keys - ref).max() <= _allowed(linear_bound(sigma.max(), np.abs(ref).max()))
    costs = np.array([3.0, 2.0, 0.5, np.nan, 1.0])
    ctrl.setRolloutCost(costs)
    ctrl.updateSampler(1e-300)
    assert ctrl.samplerResult() == dict(best=2, n_valid=4, min_cost=0.5, sum_w=1.0, ess=1.0)
    assert _same_bits(jt.samplerNominal(), np.ascontiguousarray(keys[:, 2]))
    ctrl.setRolloutCost(costs)
    ctrl.updateSampler(0.5)
    w, res = SR.weights(costs, 0.5)
    want = SR.update(keys[:, 2], keys, w, res["best"])
    assert np.abs(jt.samplerNominal() - want).max() <= _allowed(mean_bound(B, np.abs(keys).max()))
    before = jt.samplerNominal()
    ctrl.shiftSampler(1)
    assert _same_bits(jt.samplerNominal(), SR.shift(before, 1))
    # a LINEAR schedule over the rotation rows: the nominal plan is checked like the schedule's keyframes, at attach and later
    robot, ctrl, (mf, jt), _, _ = _panda(B, False)
    nom = _nominal(mf, rng, 12)
    mf.setGoalSchedule((0, 12), np.repeat(nom[:, None], B, axis=1), stride=2, mode="linear")
    bad = nom.copy()
    bad[1, 3:] = 0.0
    with pytest.raises(ValueError, match="orthonormal"):
        mf.attachSampler(0.05, nominal=bad)
    mf.attachSampler(0.05, nominal=nom)
    with pytest.raises(ValueError, match="orthonormal"):
        mf.setSamplerNominal(bad)
    assert _same_bits(mf.samplerNominal(), nom)               # a refused plan writes nothing
    mf.setSamplerNominal(nom[::-1].copy())
    assert _same_bits(mf.samplerNominal(), nom[::-1].copy())
