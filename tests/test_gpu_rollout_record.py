"""Rollout recorder (csrc/saip_rollout_record.hip, saip_batch_rollout_recorder_*): the per-period log and the running summaries of
rolloutAsync.  The oracle is the project's own call-by-call loop (the pattern of tests/test_gpu_dynamics.py::
test_rollout_with_fused_integrate_and_next_otg_equals_stepwise_loop): an identical batch driven stepAsync(); integrate() one period at a
time, read back through pullState(), getTorques(), status, getCurrentPosition / Orientation and getTaskDiagnostics() after every period.
Tolerance against that loop: |a - b| <= 1e-11 max(1, |b|), the fused-vs-separate-launch spread that test accepts for the same comparison;
the status must be equal.  Everything the recorder only copies, or that two runs of the same launches produce, is compared bit for bit."""
import functools

import numpy as np
import pytest

import trees as TR
import workloads as W
from test_gpu_batch_layout import _d2h, _same_bits

pytestmark = pytest.mark.gpu

B, K = 70, 11            # crosses one 64-lane block, not a multiple of 8
DT, SUB = 5e-4, 2
T = DT * SUB
ALL = ("q", "dq", "tau", "pose", "error")
KEYS = ("q", "dq", "tau", "position", "orientation", "position_error", "orientation_error")
#          B   kernel the case must run                 what it exercises
CASES = {"oct_fused": (B, "saip_cycle_oct"),          # config 2 without internal OTG: the cycle launch integrates in-kernel
         "otg_pair": (B, "saip_cycle_oct"),           # config 2 with both OTGs: integration fused with the next period's OTG step
         "wave": (9, "saip_cycle_wave"),              # config 5 (30-dof chain): wavefront kernel
         "tree": (B, "saip_cycle_wg_tree<32,512>")}   # dual-arm torso tree, the right arm's task selected: general tree kernel


def _flagging(spec):
    """the blended singularity strategies switched off: instances outside the non-singular branch are flagged (status 1)"""
    return [dict(t, singularity_strategies=False) if t["type"] == "motion_force" else t for t in spec]


def _panda(nb, otg, q=None, flagging=False, ld=None):
    from sai_primitives_amd.controller import controller_from_specs
    d = W.make_inputs(2, nb)
    q = d["q"] if q is None else q
    tasks = _flagging(d["tasks"]) if flagging else d["tasks"]
    robot, ctrl, objs = controller_from_specs(d["model"].name, tasks, nb, device=0, disable_otg=not otg, leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(np.zeros((nb, 7)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    mf, jt = objs
    mf.setGoalPosition(mf.getGoalPosition() + np.array([0.04, -0.03, 0.05]))
    qg = q.copy()
    qg[:, 0] += 0.3
    jt.setGoalPosition(qg)
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, mf, (0.0, 0.0, 0.0)


def _setup(case):
    """a fresh batch of the case, ready to roll: (robot, ctrl, task objects, the recorded motion-force task, gravity)"""
    from sai_primitives_amd.controller import controller_from_specs
    nb = CASES[case][0]
    if case in ("oct_fused", "otg_pair"):
        return _panda(nb, case == "otg_pair")
    if case == "wave":
        d = W.make_inputs(5, nb)
        robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], nb, device=0)
        ctrl.setKernel(4)
        robot.setQ(d["q"])
        robot.setDq(np.zeros((nb, 30)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        objs[0].setGoalPosition(objs[0].getGoalPosition() + np.array([0.02, -0.01, 0.015]))
        ctrl.updateControllerTaskModels()
        return robot, ctrl, objs, objs[0], (0.0, 0.0, 0.0)
    desc = TR.dual_panda_torso()       # the setting of tests/test_gpu_tree_paths.py::test_rollout_equals_stepwise_periods_on_tree
    m = W.RobotModel(desc)
    rng = np.random.default_rng(26)
    q = np.clip(rng.uniform(-0.8, 0.8, (nb, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    shift = rng.uniform(-0.04, 0.04, (nb, 3))
    robot, ctrl, objs = controller_from_specs(desc, TR.dual_stack(m), nb, device=0, disable_otg=False)
    objs[2].disableInternalOtg()
    ctrl.enableGravityCompensation(True)
    robot.setQ(q)
    robot.setDq(np.zeros((nb, m.dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    for t in objs[:2]:
        t.setGoalPosition(t.getGoalPosition() + shift)
    objs[2].setGoalPosition(q + 0.2)
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, objs[1], None


def _finals(ctrl, objs):
    """what a rollout leaves behind: state, torques, status, what every task tracks (the OTG output where one runs)"""
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    tau = ctrl.getTorques()
    return [q.copy(), dq.copy(), tau, ctrl.status.astype(np.float64)] + [t._desired_block() for t in objs]


@functools.lru_cache(maxsize=None)
def _recorded(case):
    """case 1's recorded run: stride 1, capacity K, all channels.  Shared, never modified."""
    robot, ctrl, objs, mf, grav = _setup(case)
    ctrl.recordRollouts(K, 1, ALL, task=mf)
    ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
    ctrl.synchronize()
    name = ctrl.kernelName()
    log = ctrl.rolloutLog()
    fin = _finals(ctrl, objs)
    return dict(log=log, finals=fin, kernel=name)


def _stepwise(case):
    robot, ctrl, objs, mf, grav = _setup(case)
    out = {k: [] for k in KEYS + ("status",)}
    for _ in range(K):
        ctrl.stepAsync()
        ctrl.integrate(DT, SUB, gravity=grav)
        ctrl.synchronize()
        q, dq = ctrl.pullState()
        out["q"].append(q.copy())
        out["dq"].append(dq.copy())
        out["tau"].append(ctrl.getTorques())
        out["status"].append(ctrl.status.copy())
        out["position"].append(mf.getCurrentPosition())
        out["orientation"].append(mf.getCurrentOrientation())
        diag = mf.getTaskDiagnostics()
        out["position_error"].append(diag["position_error"])
        out["orientation_error"].append(diag["orientation_error"])
    return {k: np.array(v) for k, v in out.items()}, ctrl.kernelName()


# ------------------------------------------------------------------ 1. every kernel path against the stepwise loop
@pytest.mark.parametrize("case", list(CASES))
def test_log_matches_the_stepwise_loop(case):
    nb, kernel = CASES[case]
    rec = _recorded(case)
    ref, ref_kernel = _stepwise(case)
    assert rec["kernel"] == kernel and ref_kernel == kernel
    log = rec["log"]
    assert np.array_equal(log["period"], np.arange(1, K + 1))
    assert np.array_equal(log["status"], ref["status"])
    for k in KEYS:
        a, b = log[k], ref[k]
        assert a.shape == b.shape and a.shape[:2] == (K, nb), k
        err = np.abs(a - b).max()
        print(case, k, "max |recorded - stepwise|", err, "scale", np.abs(b).max())
        assert err <= 1e-11 * max(1.0, np.abs(b).max()), (k, err)
    assert np.abs(log["q"][-1] - log["q"][0]).max() > 1e-5      # the robots did move
    assert np.abs(log["position_error"]).max() > 1e-3            # and the error channel is not trivially zero


# ------------------------------------------------------------------ 2. the last sample is a copy of what the rollout left
@pytest.mark.parametrize("case", list(CASES))
def test_last_sample_is_bit_equal_to_the_final_state(case):
    rec = _recorded(case)
    q, dq, tau, st = rec["finals"][:4]
    log = rec["log"]
    assert _same_bits(log["q"][-1], q) and _same_bits(log["dq"][-1], dq) and _same_bits(log["tau"][-1], tau)
    assert np.array_equal(log["status"][-1].astype(np.float64), st)


# ------------------------------------------------------------------ 3. recording changes nothing
@pytest.mark.parametrize("case", list(CASES))
def test_recorded_rollout_equals_the_unrecorded_one(case):
    robot, ctrl, objs, mf, grav = _setup(case)
    ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
    plain = _finals(ctrl, objs)
    assert ctrl.kernelName() == CASES[case][1]
    for i, (a, b) in enumerate(zip(_recorded(case)["finals"], plain)):
        assert _same_bits(a, b), i


# ------------------------------------------------------------------ 4. stride, ring, the counter across calls, reset
def test_stride_ring_counter_and_reset():
    from sai_primitives_amd import capi
    full = _recorded("oct_fused")["log"]
    robot, ctrl, objs, mf, grav = _setup("oct_fused")
    ctrl.recordRollouts(2, 3, ALL, task=mf)
    ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
    ctrl.synchronize()
    log = ctrl.rolloutLog()
    assert log["status"].shape == (2, B) and list(log["period"]) == [6, 9]
    for k in KEYS + ("status",):
        assert _same_bits(log[k].astype(np.float64), full[k][[5, 8]].astype(np.float64)), k
    ctrl.updateControllerTaskModels()
    ctrl.rolloutAsync(4, DT, SUB, gravity=grav)     # periods 12..15: the counter goes on
    ctrl.synchronize()
    log2 = ctrl.rolloutLog()
    assert list(log2["period"]) == [12, 15]
    q, _ = ctrl.pullState()
    assert _same_bits(log2["q"][-1], q) and not _same_bits(log2["q"][0], log["q"][1])
    ctrl.resetRolloutRecorder()
    empty = ctrl.rolloutLog()
    assert empty["status"].shape == (0, B) and empty["period"].shape == (0,) and empty["q"].shape == (0, B, 7)
    ctrl.rolloutAsync(4, DT, SUB, gravity=grav)     # periods 1..4 of a new count: one sample, period 3
    ctrl.synchronize()
    assert list(ctrl.rolloutLog()["period"]) == [3]
    # a second recorder needs the first one gone
    with pytest.raises(Exception, match="already attached"):
        ctrl.recordRollouts(2)
    ctrl.stopRecordingRollouts()
    assert capi.lib().saip_batch_rollout_log_device(ctrl._h) is None      # the log is freed
    ctrl.recordRollouts(3, channels=("tau",))
    ctrl.rolloutAsync(2, DT, SUB, gravity=grav)
    ctrl.synchronize()
    log3 = ctrl.rolloutLog()
    assert sorted(log3) == ["period", "status", "tau"] and list(log3["period"]) == [1, 2]
    assert _same_bits(log3["tau"][-1], ctrl.getTorques())


# ------------------------------------------------------------------ 5. running summaries
def _summary_reference(log):
    """the eight rows from the log of the same run, summed sequentially in period order (and joint order inside a period); squared
    norms as ((e0 e0 + e1 e1) + e2 e2), every operation rounded once -- what the kernel does for the rows that must be bit-equal"""
    n, nb, dof = log["tau"].shape
    s = np.zeros((nb, 8))
    tau0 = np.where(np.isnan(log["tau"]), 0.0, log["tau"])
    for k in range(n):
        tt = np.zeros(nb)
        for j in range(dof):
            tt = tt + tau0[k, :, j] * tau0[k, :, j]
        s[:, 0] += T * tt
        for row, key in ((1, "position_error"), (2, "orientation_error")):
            e = log[key][k]
            e2 = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            s[:, row] += T * e2
            s[:, row + 2] = np.fmax(s[:, row + 2], np.sqrt(e2))
        s[:, 5] = np.fmax(s[:, 5], np.abs(tau0[k]).max(axis=1))
        s[:, 6] = np.fmax(s[:, 6], np.fmax.reduce(np.abs(log["dq"][k]), axis=1))
    s[:, 7] = (log["status"] != 0).sum(axis=0)
    return s


def _check_summary(summ, log, dof):
    ref = _summary_reference(log)
    tol = (K + dof + 8) * 2.0 ** -53      # K + dof + 8 roundings on non-negative terms
    assert tol <= 1e-13
    for row in (0, 1, 2):
        rel = np.abs(summ[:, row] - ref[:, row]) / ref[:, row]
        print("summary row", row, "max relative difference", rel.max(), "bound", tol)
        assert (ref[:, row] > 0).all() and rel.max() <= tol, row
    for row in (3, 4, 5, 6):
        assert _same_bits(summ[:, row], ref[:, row]), row
    assert np.array_equal(summ[:, 7], ref[:, 7])


def test_summaries_equal_the_reduction_of_the_log():
    robot, ctrl, objs, mf, grav = _setup("otg_pair")
    ctrl.recordRollouts(K, 1, ALL, task=mf, summaries=True)
    ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
    ctrl.synchronize()
    log, summ = ctrl.rolloutLog(), ctrl.rolloutSummary()
    assert summ.shape == (B, 8) and log["status"].shape == (K, B)
    for k in KEYS + ("status",):     # summaries on or off, the log is the same
        assert _same_bits(log[k].astype(np.float64), _recorded("otg_pair")["log"][k].astype(np.float64)), k
    _check_summary(summ, log, 7)
    # summaries only: nothing is sampled, the summaries are the same
    robot2, ctrl2, objs2, mf2, _ = _setup("otg_pair")
    ctrl2.recordRollouts(K, 1, (), task=mf2, summaries=True)
    ctrl2.rolloutAsync(K, DT, SUB, gravity=grav)
    ctrl2.synchronize()
    log2 = ctrl2.rolloutLog()
    assert log2["status"].shape == (0, B) and sorted(log2) == ["period", "status"]
    assert _same_bits(ctrl2.rolloutSummary(), summ)
    # no task selected: rows 1..4 stay zero; a stride changes the log, not the summaries
    robot3, ctrl3, objs3, _, _ = _setup("otg_pair")
    ctrl3.recordRollouts(K, 4, ("q",), summaries=True)
    ctrl3.rolloutAsync(K, DT, SUB, gravity=grav)
    ctrl3.synchronize()
    s3 = ctrl3.rolloutSummary()
    assert list(ctrl3.rolloutLog()["period"]) == [4, 8]
    assert not s3[:, 1:5].any() and _same_bits(s3[:, [0, 5, 6, 7]], summ[:, [0, 5, 6, 7]])
    ctrl3.resetRolloutRecorder()
    assert not ctrl3.rolloutSummary().any()


def test_summaries_on_the_tree():
    robot, ctrl, objs, mf, grav = _setup("tree")
    ctrl.recordRollouts(K, 1, ALL, task=mf, summaries=True)
    ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
    ctrl.synchronize()
    _check_summary(ctrl.rolloutSummary(), ctrl.rolloutLog(), 15)


# ------------------------------------------------------------------ 6. an instance the engine refuses
def test_refused_instance_is_counted_and_isolated():
    """instance 5 sits at the elbow singularity (joint 4 nearly straight, as in tests/test_gpu_singularity_strategies.py) with the
    blended strategies off and the NaN torque policy: it is flagged in every period and coasts"""
    bad = 5
    runs = []
    for singular in (True, False):
        q = W.make_inputs(2, B)["q"].copy()
        if singular:
            q[bad, 3] = -0.08
        robot, ctrl, objs, mf, grav = _panda(B, False, q=q, flagging=True)
        ctrl.setFlaggedTorquePolicy(True)
        ctrl.recordRollouts(K, 1, ALL, task=mf, summaries=True)
        ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
        ctrl.synchronize()
        runs.append((ctrl.rolloutLog(), ctrl.rolloutSummary()))
    (log, summ), (log0, summ0) = runs
    print("status of the singular instance per period", log["status"][:, bad], "row 7", summ[bad, 7], "row 0", summ[bad, 0])
    assert (log["status"][:, bad] != 0).all() and summ[bad, 7] == K
    assert np.isnan(log["tau"][:, bad]).all()
    assert np.isfinite(summ[bad]).all() and summ[bad, 0] == 0.0 and summ[bad, 5] == 0.0
    assert (log0["status"] == 0).all() and not summ0[:, 7].any()
    others = np.arange(B) != bad
    for k in KEYS + ("status",):
        assert _same_bits(log[k][:, others].astype(np.float64), log0[k][:, others].astype(np.float64)), k
    assert _same_bits(summ[others], summ0[others])


# ------------------------------------------------------------------ 7. padded leading dimension
def test_padded_leading_dimension_keeps_its_padding():
    from sai_primitives_amd import capi
    L = capi.lib()
    ld, cap, steps = 160, 4, 6
    robot, ctrl, objs, mf, grav = _panda(B, False, ld=ld)
    assert L.saip_batch_ld(ctrl._h) == ld
    ctrl.recordRollouts(cap, 1, ALL, task=mf, summaries=True)
    ctrl.rolloutAsync(steps, DT, SUB, gravity=grav)
    ctrl.synchronize()
    log = ctrl.rolloutLog()
    rows = 3 * 7 + 18
    ring = _d2h(L.saip_batch_rollout_log_device(ctrl._h), (cap, rows, ld))
    summ = _d2h(L.saip_batch_rollout_summary_device(ctrl._h), (8, ld))
    assert not ring[:, :, B:].any() and not summ[:, B:].any()      # still the fill of attach: nothing stored past B
    assert list(log["period"]) == [3, 4, 5, 6]
    flat = np.concatenate([log["q"], log["dq"], log["tau"], log["position"], log["orientation"].reshape(cap, B, 9),
                           log["position_error"], log["orientation_error"]], axis=2).transpose(0, 2, 1)
    for i, p in enumerate(log["period"]):        # period p sits in slot (p - 1) % capacity
        assert _same_bits(ring[(p - 1) % cap][:, :B], flat[i]), p
    assert _same_bits(summ[:, :B].T, ctrl.rolloutSummary())
    full = _recorded("oct_fused")["log"]          # the same periods at the default leading dimension
    for k in KEYS + ("status",):
        assert _same_bits(log[k].astype(np.float64), full[k][2:6].astype(np.float64)), k
