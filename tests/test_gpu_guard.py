"""Resident guards on the device (csrc/saip_guard.hip, saip_batch_guard_*).  Oracles: the NumPy restatement tests/guard_ref.py fed with the
device's own readout (state and goal rows bit for bit in every period), the engine's pose getter and task diagnostics (the readout), the
host-driven loop { contactSense, evaluateGuards, stepAsync, integrate } for whole rollouts, the same rollout without guards (behaviour,
comparisons only), an unattached twin at the measured state (sensing), and the snapshot's source columns.

The Panda stack of config 2 at B = 70 (ld = 96: two blocks, the second ragged, 26 padded columns), 40 periods of 8 ms; a dual-arm tree at
B = 5 for the TREE instantiation.

The scene: every instance's tool starts at rest above its own table (per-instance contact planes with the simulated sensor) and a LINEAR
position schedule lowers the goal by 5 cm/s.  The table of instance i is `gap[i]` below the tool: -0.5 mm (the tool starts inside) to
1.5 mm, so that instances touch in different periods, and 5 cm for every seventh instance, which never touches.  The contact point sits a
few millimetres beside the control point, so the sensed moment is not zero."""
import ctypes as C

import numpy as np
import pytest

import goal_schedule_ref as GSR
import guard_ref as GR
import trees as TR
import workloads as W
from test_gpu_batch_layout import _d2h, _h2d, _same_bits

pytestmark = pytest.mark.gpu

B, LD, K = 70, 96, 40
DT, SUB = 1e-3, 8
ZERO_G = (0.0, 0.0, 0.0)
SPEED = 0.05                                                            # of the scheduled descent, m/s
NEVER = np.arange(B) % 7 == 3                                           # instances whose table is out of reach
GAP = np.where(NEVER, 0.05, np.linspace(-5e-4, 1.5e-3, B))
TOUCH = dict(signal="force", axis="norm", cmp=">=", threshold=1.0, hold=2)
# the last two never fire: they make every launch gather the sensed moment and the joint speeds, which the readout checks then cover
GUARDS = [{"from": 0, "to": 1, **TOUCH}, {"from": 1, "to": 2, "signal": "periods", "threshold": 5},
          {"from": 2, "to": 3, "signal": "pos_error", "cmp": "<=", "threshold": 5e-3, "hold": 3},
          {"from": 0, "to": 0, "signal": "moment", "axis": "norm", "threshold": 1e9}, {"from": 0, "to": 0, "signal": "joint_speed", "threshold": 1e9}]
POINT = (2e-3, 4e-3, 0.0)                                               # the contact point in the control frame
PHASES = [dict(mode="free"), dict(mode="hold"), dict(mode="offset", offset=(0.0, 0.0, 2e-3)), dict(mode="free")]
GUARD_ROWS = np.array([GR.guard(0, 1, GR.FORCE, 1.0, axis=3, hold=2), GR.guard(1, 2, GR.PERIODS, 5.0), GR.guard(2, 3, GR.POS_ERROR, 5e-3, cmp=GR.LE, hold=3),
                       GR.guard(0, 0, GR.MOMENT, 1e9, axis=3), GR.guard(0, 0, GR.JOINT_SPEED, 1e9)])
PHASE_ROWS = np.array([[GR.FREE, 0, 0, 0], [GR.HOLD_MODE, 0, 0, 0], [GR.OFFSET, 0, 0, 2e-3], [GR.FREE, 0, 0, 0]])


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _scene(otg=False, guards=GUARDS, phases=PHASES, schedule=False, per_instance=False):
    """(robot, ctrl, mf, keys): config 2 at rest, stiffer position gains, per-instance tables, guards attached (None: no guards)"""
    from sai_primitives_amd import capi
    from sai_primitives_amd.controller import controller_from_specs
    d = W.make_inputs(2, B)
    robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, disable_otg=not otg)
    assert capi.lib().saip_batch_ld(ctrl._h) == LD
    robot.setQ(d["q"])
    robot.setDq(np.zeros((B, 7)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    mf = objs[0]
    mf.setPosControlGains(400.0, 40.0, 0.0)
    ctrl.updateControllerTaskModels()
    p0 = mf.getCurrentPosition()
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, 2.0e4, 400.0, 0.3, 1e-3]
    planes[0, :, 3] = robot.position("end-effector", tuple(np.array([0, 0, 0.07]) + POINT))[:, 2] - GAP
    mf.attachContactPlanes(planes, point=POINT, sensor=True, per_instance=True)
    keys = np.stack([p0, p0 - np.array([0.0, 0.0, SPEED * K * DT * SUB])])
    if schedule:
        mf.setGoalSchedule("position", keys, stride=K, mode="linear")
    if guards is not None:
        mf.attachGuards(guards, phases, per_instance=per_instance)
    return robot, ctrl, mf, keys


def _finals(ctrl, mf, guards=True):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    out = dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), goal=mf._get_goal())
    if guards:
        out.update(ctrl.guardState())
    return out


def _same(a, b, keys=None):
    for k in (a if keys is None else keys):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x, y) if x.dtype.kind == "i" else _same_bits(x, y), k


def _pose_rows(mf):
    pos, rot = mf._current_pose()
    return np.concatenate([pos.T, rot.reshape(-1, 9).T])                 # (12, B)


def _host_loop(otg, check, periods=K):
    """the host-driven loop; check: every period against the restatement fed with the device's readout.  Returns (ctrl, mf, ref, finals)"""
    robot, ctrl, mf, keys = _scene(otg)
    ref = GR.Guards(GUARD_ROWS, PHASE_ROWS, B)
    moment = 0.0
    for c in range(periods):
        mf.setGoalPosition(GSR.rows(keys, c, K, "linear"))                # what the schedule of the rollout writes in period c
        ctrl.contactSense()
        if check:
            before, pose, diag = mf._get_goal().T.copy(), _pose_rows(mf), mf.getTaskDiagnostics()
            speed = np.abs(ctrl.pullState()[1]).max(axis=1)                # max_j |dq_j| of the resident state (no sensing model here)
        ctrl.evaluateGuards()
        if check:
            ro, st, goal = ctrl.guardReadout(), ctrl.guardState(), mf._get_goal().T
            # the readout: the pose getter, the task diagnostics, the sensed rows of the goal block
            assert _same_bits(ro["position"], pose[:3].T), c
            assert _same_bits(ro["pos_error"], GR.norm3(diag["position_error"])) and _same_bits(ro["ori_error"], GR.norm3(diag["orientation_error"])), c
            assert _same_bits(ro["force"], GR.norm3(before[30:33].T)) and _same_bits(ro["moment"], GR.norm3(before[33:36].T)), c
            assert _same_bits(ro["joint_speed"], speed), c
            moment = max(moment, np.abs(before[33:36]).max())
            want = before[:24].copy()
            ref.step(want, f=before[30:33].T, m=before[33:36].T, pos=ro["position"], ep=ro["pos_error"], eo=ro["ori_error"], speed=ro["joint_speed"], pose=pose)
            _same(st, ref.state())
            assert _same_bits(goal[:24], want) and _same_bits(goal[24:], before[24:]), c
        ctrl.stepAsync()
        ctrl.integrate(DT, SUB, gravity=ZERO_G)
    assert not check or (moment > 1e-3 and speed.max() > 1e-3)           # the moment and speed rows were checked on values that are not zero
    return ctrl, mf, ref, _finals(ctrl, mf)


# ------------------------------------------------------------------ 1. the host-driven loop against the restatement
def test_host_driven_loop_equals_the_restatement(sp):
    ctrl, mf, ref, fin = _host_loop(False, True)
    entry, phase = fin["entry"], fin["phase"]
    print("instances per final phase", np.bincount(phase, minlength=4), "entry periods into HOLD", np.unique(entry[1]))
    for p in range(1, 4):                                                # conditions, so that the test cannot pass vacuously
        assert (entry[p] >= 0).any(), p
    assert len(np.unique(entry[1][entry[1] >= 0])) >= 2
    assert (phase[NEVER] == 0).all() and NEVER.any() and (fin["fires"][:, NEVER] == 0).all()
    assert (fin["clock"] == K).all() and np.isfinite(fin["q"]).all()
    reached = entry[1] >= 0
    assert (np.abs(fin["latch"][:, reached]).max(axis=0) > 0).all() and not fin["latch"][:, ~reached].any()
    # the sampler's cost term on these entries: its formula bit for bit, the columns that never got there at w_miss = +inf
    mf.setGoalSchedule("position", np.repeat(mf._get_goal()[None, :, :3], 2, axis=0))
    mf.attachSampler(1e-3)
    c0 = np.random.default_rng(3).uniform(0.0, 4.0, B)
    for ph, w_time, w_miss in ((1, 0.25, np.inf), (3, 1.0 / 3.0, 7.5), (0, 2.0, np.inf)):
        ctrl.setRolloutCost(c0)
        ctrl.guardCost(ph, w_time, w_miss)
        got = ctrl.getRolloutCost()
        assert _same_bits(got, GR.cost(c0, ref.entry[ph], w_time, w_miss)), ph
    ctrl.setRolloutCost(c0)
    ctrl.guardCost(1, 0.25)
    got = ctrl.getRolloutCost()
    assert np.array_equal(np.isinf(got), ~reached) and np.isinf(got).any() and np.isfinite(got).any()
    # scenario groups M = 2: candidate c is instances c and 35 + c; one missed scenario invalidates the candidate
    ctrl.setSamplerScenarios(2, "mean")
    ctrl.updateSampler(1.0)
    missed = ~(reached[:35] & reached[35:])
    group = ctrl.samplerGroupCost()
    assert np.array_equal(np.isinf(group), missed) and missed.any() and not missed.all()
    assert ctrl.samplerResult()["n_valid"] == int((~missed).sum())
    with pytest.raises(ValueError, match="phase 4 outside the 4 phases"):
        ctrl.guardCost(4, 1.0)


def test_add_cost_needs_a_sampler(sp):
    robot, ctrl, mf, _ = _scene()
    with pytest.raises(sp.SaipError, match="no sampler is attached"):
        ctrl.guardCost(1, 1.0)
    with pytest.raises(sp.SaipError, match="already attached"):
        mf.attachGuards(GUARDS, PHASES)
    assert ctrl.guardInfo() == dict(task=0, n_guards=5, per_instance=False, n_phases=4, needs_pose=True)
    mf.detachGuards()
    with pytest.raises(sp.SaipError, match="no guards are attached"):
        ctrl.evaluateGuards()


# ------------------------------------------------------------------ 2. a rollout is the loop
@pytest.mark.parametrize("otg", [False, True])
def test_rollout_equals_the_host_driven_loop(sp, otg):
    _, _, _, loop = _host_loop(otg, False)
    robot, ctrl, mf, _ = _scene(otg, schedule=True)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    roll = _finals(ctrl, mf)
    _same(loop, roll)
    assert (roll["entry"][1] >= 0).any() and (roll["clock"] == K).all() and np.isfinite(roll["q"]).all()


# ------------------------------------------------------------------ 3. it does something
def test_a_guarded_descent_stops_at_the_table(sp):
    """FORCE -> HOLD only, against the same rollout without guards: comparisons, no absolute figure"""
    runs = {}
    for guarded in (True, False):
        robot, ctrl, mf, _ = _scene(False, guards=GUARDS[:1] if guarded else None, phases=PHASES[:2], schedule=True)
        ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        ctrl.synchronize()
        runs[guarded] = dict(peak=mf.contactSummary()["max_force"], pen=-mf.contactReadout()["distance"], pos=mf.getCurrentPosition(),
                             state=ctrl.guardState() if guarded else None)
    g, u = runs[True], runs[False]
    held = g["state"]["phase"] == 1
    latch = g["state"]["latch"][:3].T
    dg, du = np.linalg.norm(g["pos"] - latch, axis=1), np.linalg.norm(u["pos"] - latch, axis=1)
    print(f"{held.sum()} of {B} instances reached HOLD; peak force {g['peak'][held].max():.3g} N against {u['peak'][held].max():.3g} N unguarded; final penetration "
          f"{g['pen'][held].max():.3g} m against {u['pen'][held].max():.3g} m; distance from the latch {dg[held].max():.3g} m against {du[held].max():.3g} m")
    assert held.sum() >= B // 2 and not held[NEVER].any()
    # the peak of an instance that touches at speed is the impact itself, which both runs share up to the period the guard fires in: equal
    # there, never larger, and smaller where it counts, in the largest force over the instances
    assert (g["peak"][held] <= u["peak"][held]).all() and g["peak"][held].max() < u["peak"][held].max()
    assert (g["pen"][held] < u["pen"][held]).all()
    assert (dg[held] < du[held]).all()
    assert _same_bits(g["pos"][NEVER], u["pos"][NEVER])                  # an instance whose guard never fired is the unguarded one


# ------------------------------------------------------------------ 4. sensing attached
def test_the_guard_reads_what_the_controller_reads(sp):
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, mf, _ = _scene()
    table = np.zeros((7, 6))
    table[:, 0] = 0.02                                                   # an encoder offset on every joint
    ctrl.attachSensing(table, seed=1)
    ctrl.evaluateGuards()
    ro = ctrl.guardReadout()
    qm, _ = ctrl.measuredState()
    true = robot.position("end-effector", (0, 0, 0.07))
    assert np.linalg.norm(ro["position"] - true, axis=1).max() > 1e-3    # not the pose of q
    d = W.make_inputs(2, B)
    twin_robot, twin, tobjs = controller_from_specs(d["model"].name, d["tasks"], B, device=0)
    twin_robot.setQ(qm)
    twin_robot.setDq(np.zeros((B, 7)))
    twin_robot.updateModel()
    twin.updateControllerTaskModels()
    assert _same_bits(ro["position"], tobjs[0].getCurrentPosition())     # the pose of q_meas
    assert _same_bits(ro["position"], mf.getCurrentPosition())


def test_wrench_noise_is_repeatable_under_one_seed(sp):
    wrench = np.zeros((6, 3))
    wrench[:, 2] = 0.5                                                   # sigma on every axis of the sensed wrench
    outs = []
    for seed in (11, 11, 12):
        robot, ctrl, mf, _ = _scene(schedule=True)
        ctrl.attachSensing(wrenches={mf: wrench}, seed=seed)
        ctrl.rolloutAsync(12, DT, SUB, gravity=ZERO_G)
        outs.append(_finals(ctrl, mf))
    _same(outs[0], outs[1])
    assert not _same_bits(outs[0]["goal"][:, 30:33], outs[2]["goal"][:, 30:33])
    assert (outs[0]["entry"][1] >= 0).any()                              # the noisy sensor tripped guards


# ------------------------------------------------------------------ 5. the TREE instantiation
def test_a_tree_with_the_task_on_one_arm(sp):
    from sai_primitives_amd.controller import controller_from_specs
    nb = 5
    desc = TR.dual_panda_torso()
    m = W.RobotModel(desc)
    rng = np.random.default_rng(26)
    q = np.clip(rng.uniform(-0.8, 0.8, (nb, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    robot, ctrl, objs = controller_from_specs(desc, TR.dual_stack(m), nb, device=0)
    robot.setQ(q)
    robot.setDq(np.zeros((nb, m.dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    mf = objs[1]                                                         # the right arm: the walk skips the left arm's joints
    goal0 = mf._get_goal().T.copy()
    mf.attachGuards([{"from": 0, "to": 1, "signal": "periods", "threshold": 2}], [dict(mode="free"), dict(mode="hold")])
    assert ctrl.guardInfo()["task"] == 1
    ref, goal = GR.Guards([GR.guard(0, 1, GR.PERIODS, 2.0)], [[GR.FREE, 0, 0, 0], [GR.HOLD_MODE, 0, 0, 0]], nb), goal0[:24].copy()
    pose = _pose_rows(mf)
    for c in range(4):
        ctrl.evaluateGuards()
        ro = ctrl.guardReadout()
        assert _same_bits(ro["position"], pose[:3].T) and np.isnan(ro["pos_error"]).all() and np.isnan(ro["force"]).all()
        ref.step(goal, pos=ro["position"], pose=pose)
        _same(ctrl.guardState(), ref.state())
        assert _same_bits(mf._get_goal().T[:24], goal)
    st = ctrl.guardState()
    assert (st["phase"] == 1).all() and (st["entry"][1] == 2).all() and _same_bits(st["latch"], pose)
    assert _same_bits(mf._get_goal().T[:12], pose) and not mf._get_goal().T[12:24].any()
    assert np.isfinite(pose).all()


# ------------------------------------------------------------------ 5b. per-instance tables, and a replaced table
def test_per_instance_tables_and_a_replaced_table(sp):
    """thresholds and debounces that differ per column against the restatement; setGuards changes what the launches gather and keeps the state"""
    from sai_primitives_amd import capi
    robot, ctrl, mf, _ = _scene(guards=None)
    i = np.arange(B)
    first = [{"from": 0, "to": 1, "signal": "periods", "threshold": (i % 5).astype(float)},
             {"from": 1, "to": 1, "signal": "force", "axis": "norm", "threshold": np.full(B, 1e9)}]
    second = [first[0], {"from": 1, "to": 2, "signal": "joint_speed", "threshold": 0.0, "hold": 1 + i % 3}]
    phases = [dict(mode="free"), dict(mode="hold"), dict(mode="offset", offset=(1e-3, 0.0, 2e-3))]
    ones = np.ones(B)
    rows1 = np.stack([np.stack([0 * ones, ones, GR.PERIODS * ones, 0 * ones, 0 * ones, (i % 5).astype(float), ones, 0 * ones]),
                      np.stack([ones, ones, GR.FORCE * ones, 3 * ones, 0 * ones, 1e9 * ones, ones, 0 * ones])])
    rows2 = rows1.copy()
    rows2[1] = np.stack([ones, 2 * ones, GR.JOINT_SPEED * ones, 0 * ones, 0 * ones, 0 * ones, 1.0 + i % 3, 0 * ones])
    mf.attachGuards(first, phases, per_instance=True)
    assert ctrl.guardInfo()["per_instance"] is True
    ctrl.synchronize()
    got = _d2h(capi.lib().saip_batch_guard_guards_device(ctrl._h), (16, LD))
    assert _same_bits(got[:, :B], rows1.reshape(16, B)) and not got[:, B:].any()
    ref = GR.Guards(rows1, [[GR.FREE, 0, 0, 0], [GR.HOLD_MODE, 0, 0, 0], [GR.OFFSET, 1e-3, 0, 2e-3]], B)
    pose, goal = _pose_rows(mf), mf._get_goal().T.copy()
    for c in range(11):
        if c == 6:
            mf.setGuards(second)
            ref.table = rows2.copy()
        ctrl.evaluateGuards()
        ro, st = ctrl.guardReadout(), ctrl.guardState()
        if c < 6:                                                        # PERIODS and FORCE: the sensed force is gathered, the speeds are not
            assert _same_bits(ro["force"], GR.norm3(goal[30:33].T)) and np.isnan(ro["joint_speed"]).all(), c
        else:                                                            # PERIODS and JOINT_SPEED: the other way round (the robot is at rest)
            assert np.isnan(ro["force"]).all() and _same_bits(ro["joint_speed"], np.zeros(B)), c
        assert _same_bits(ro["position"], pose[:3].T), c
        ref.step(goal, f=goal[30:33].T, pos=ro["position"], speed=ro["joint_speed"], pose=pose)
        _same(st, ref.state())
        assert _same_bits(mf._get_goal().T, goal), c
    assert np.array_equal(st["entry"][1], i % 5) and np.array_equal(st["entry"][2], np.maximum(i % 5 + 1, 6) + i % 3)
    assert (st["phase"] == 2).all() and _same_bits(goal[:3], pose[:3] + np.array([[1e-3], [0.0], [2e-3]]))
    # any output of _state_host may be NULL
    ph = np.full(B, -7, np.int32)
    ctrl._call("saip_batch_guard_state_host", ph.ctypes.data_as(C.POINTER(C.c_int)), None, None, None, None, None, None)
    assert np.array_equal(ph, st["phase"])
    lt = np.empty((12, B))
    ctrl._call("saip_batch_guard_state_host", None, None, None, None, None, None, lt.ctypes.data_as(C.POINTER(C.c_double)))
    assert _same_bits(lt, st["latch"])
    ctrl._call("saip_batch_guard_state_host", None, None, None, None, None, None, None)


# ------------------------------------------------------------------ 6. snapshots
def test_snapshots_carry_the_guard_state(sp):
    robot, ctrl, mf, _ = _scene(schedule=False)
    mf.setGoalPosition(mf.getGoalPosition() - np.array([0.0, 0.0, 5e-3]))  # a constant goal 5 mm below: no schedule, whose counter no snapshot carries
    snap = ctrl.saveState()
    names = [s["name"] for s in snap.segments()]
    assert names[-7:] == ["guard.phase", "guard.since", "guard.clock", "guard.run", "guard.entry", "guard.fires", "guard.latch"]
    ctrl.rolloutAsync(12, DT, SUB, gravity=ZERO_G)
    ctrl.saveState(snap)
    mid = _finals(ctrl, mf)
    assert len(np.unique(mid["phase"])) >= 2                             # mid-rollout: the instances are in different phases
    ctrl.rolloutAsync(8, DT, SUB, gravity=ZERO_G)
    end = _finals(ctrl, mf)
    assert not np.array_equal(end["since"], mid["since"])
    # every instance its own: the continuation repeats
    ctrl.restoreState(snap)
    _same(_finals(ctrl, mf), mid)
    ctrl.rolloutAsync(8, DT, SUB, gravity=ZERO_G)
    _same(_finals(ctrl, mf), end)
    # a permutation and a broadcast: guard state and goal rows of the source columns
    perm = np.random.default_rng(5).permutation(B)
    src = int(np.flatnonzero(mid["phase"] > 0)[0])
    for source, cols in ((perm, perm), (src, np.full(B, src))):
        ctrl.restoreState(snap, source)
        got = _finals(ctrl, mf)
        for k in ("phase", "since", "clock"):
            assert np.array_equal(got[k], mid[k][cols]), k
        for k in ("run", "entry", "fires"):
            assert np.array_equal(got[k], mid[k][:, cols]), k
        assert _same_bits(got["latch"], mid["latch"][:, cols]) and _same_bits(got["goal"], mid["goal"][cols])
        ctrl.rolloutAsync(2, DT, SUB, gravity=ZERO_G)                    # ... and the batch rolls on from there
        assert (_finals(ctrl, mf)["clock"] == mid["clock"][cols] + 2).all()
    # a snapshot of another guard layout is refused, the segment named
    mf.detachGuards()
    with pytest.raises(sp.SaipError, match=r"\[guard\.phase\] is gone"):
        ctrl.restoreState(snap)
    bare = ctrl.saveState()
    mf.attachGuards(GUARDS, PHASES)
    with pytest.raises(sp.SaipError, match=r"\[guard\.phase\] is new"):
        ctrl.restoreState(bare)


# ------------------------------------------------------------------ 7. padding and no-op
def _ptr(p):
    return p.value if hasattr(p, "value") else p


def test_padding_columns_are_never_written(sp):
    from sai_primitives_amd import capi
    per = [dict(g, threshold=np.full(B, float(g["threshold"]))) for g in GUARDS]
    robot, ctrl, mf, _ = _scene(schedule=True, guards=per, per_instance=True)
    L = capi.lib()
    ptrs = [C.c_void_p() for _ in range(7)]
    ctrl._call("saip_batch_guard_state_device", *(C.byref(p) for p in ptrs))
    G, P = 5, 4
    arrays = [(p.value, (r, LD), np.int32, 0x5A5A5A5A) for p, r in zip(ptrs[:6], (1, 1, 1, G, P, G))]
    arrays += [(ptrs[6].value, (12, LD), np.float64, 6.02214076e23), (L.saip_batch_guard_readout_device(ctrl._h), (8, LD), np.float64, 6.02214076e23),
               (L.saip_batch_device_goal(ctrl._h, 0), (36, LD), np.float64, 6.02214076e23),
               (L.saip_batch_guard_guards_device(ctrl._h), (G * 8, LD), np.float64, 6.02214076e23)]
    ctrl.synchronize()
    table = _d2h(arrays[-1][0], (G * 8, LD))
    assert _same_bits(table[:, :B], np.repeat(GUARD_ROWS.reshape(-1, 1), B, axis=1)) and not table[:, B:].any()   # the upload wrote columns 0 .. B-1 only
    for ptr, shape, dt, fill in arrays:
        a = _d2h(ptr, shape, dt)
        a[:, B:] = fill
        _h2d(ptr, a)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    assert (ctrl.guardState()["entry"][1] >= 0).any()                    # the per-instance table is the table of the other tests
    mf.setGuards(per)                                                    # the upload of a replacement keeps to columns 0 .. B-1 too
    ctrl.resetGuards()
    ctrl.rolloutAsync(3, DT, SUB, gravity=ZERO_G)
    ctrl.synchronize()
    for ptr, shape, dt, fill in arrays:
        a = _d2h(ptr, shape, dt)
        assert (a[:, B:] == fill).all(), shape
    st = ctrl.guardState()
    assert (st["clock"] == 3).all()                                      # ... while the reset and the rollouts wrote columns 0 .. B-1


@pytest.mark.parametrize("otg", [False, True])
def test_a_guard_that_never_fires_changes_nothing(sp, otg):
    from test_gpu_rollout_record import _panda
    outs = []
    for attached in (False, True):
        robot, ctrl, objs, mf, grav = _panda(B, otg)
        if attached:
            mf.attachGuards([{"from": 0, "to": 0, "signal": "periods", "threshold": 1e9}], [dict(mode="free")])
            assert ctrl.guardInfo()["needs_pose"] is False
        ctrl.rolloutAsync(6, 5e-4, 2, gravity=grav)
        outs.append(_finals(ctrl, mf, guards=False))
        if attached:
            st, ro = ctrl.guardState(), ctrl.guardReadout()
            assert (st["clock"] == 6).all() and (st["since"] == 6).all() and not st["phase"].any() and not st["fires"].any()
            assert all(np.isnan(v).all() for v in ro.values())          # nothing was needed, nothing was computed
    _same(outs[0], outs[1])
    assert np.abs(outs[0]["dq"]).max() > 1e-3
