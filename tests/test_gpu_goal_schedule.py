"""Goal schedules (csrc/saip_goal_schedule.hip, saip_batch_goal_schedule_*): time-varying task goals inside rolloutAsync from keyframes
resident on the device.  The oracle is the project's own host-driven loop: an identical batch given the period's goal rows through
saip_batch_set_goal_field_host and rolled one period at a time, the rows coming from the NumPy restatement tests/goal_schedule_ref.py.
Both sides enqueue the same launches on the same inputs (no fused integrate + OTG launch on either side), so everything is compared bit
for bit; only the rows interpolated on SO(3) depend on the maths library and carry a measured bound.

Shapes: B = 70 on the Panda (two 64-lane blocks, the second ragged, ld = 96) and B = 33 at a padded leading dimension of 128; K = 3
keyframes at stride 2 run for 6 periods: keyframe periods 0, 2, 4, the periods in between, and the hold past the end."""
import numpy as np
import pytest

import goal_schedule_ref as GS
import trees as TR
import workloads as W
from test_gpu_batch_layout import _d2h, _h2d, _same_bits
from test_gpu_rollout_record import _panda

pytestmark = pytest.mark.gpu

K, STRIDE, PERIODS = 3, 2, 6
DT, SUB = 5e-4, 2
SHAPES = [(70, None), (33, 128)]          # (B, leading dimension)
REC = ("q", "dq", "tau", "error")
SENTINEL = 6.02214076e23
# worst |device - NumPy| entry of the SO(3)-interpolated goal rows over test_slerp_rows_match_the_restatement's inputs (consecutive
# keyframes up to 3.0 rad apart); the test allows 64 x that, and never more than 1e-11.  The MI355X figure has not been taken yet (None:
# DESIGN.md 4.9), so the worst is derived instead: kernel and restatement run the same operations in the same order and differ only in
# atan2, sin and cos (sqrt is correctly rounded on both sides).  At <= 2 ulp each, the angle s * atan2 (s <= 1/2, atan2 <= pi) differs by
# <= 4.4e-16, sin and cos of it by <= 4.4e-16 + 4.4e-16, an entry of Exp (|k| <= 1, two terms) by <= 1e-15, and an entry of R0 Exp (a
# row of R0 has 1-norm <= sqrt 3) by <= 2e-15
SLERP_WORST_MEASURED = None
SLERP_WORST_DERIVED = 2e-15
# worst relative torque difference (workloads.torque_error) of the closed loop on device-interpolated rows against the loop fed with
# NumPy's rows on the MI355X (None: not taken yet); the bound is the project's torque tolerance
CLOSED_LOOP_WORST_MEASURED = None
TORQUE_TOL = 1e-5


# ------------------------------------------------------------------ stacks
def _stack(name, B, ld=None):
    """(robot, ctrl, task objects, the motion-force task the recorder watches, gravity, kernel the stack must run)"""
    from sai_primitives_amd.controller import controller_from_specs
    if name in ("otg", "no_otg"):
        return _panda(B, name == "otg", ld=ld) + ("saip_cycle_oct",)
    if name == "chain30":                      # config 5, the wavefront kernel
        d = W.make_inputs(5, B)
        robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, leading_dimension=ld)
        ctrl.setKernel(4)
        robot.setQ(d["q"])
        robot.setDq(np.zeros((B, 30)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        ctrl.updateControllerTaskModels()
        return robot, ctrl, objs, objs[0], (0.0, 0.0, 0.0), "saip_cycle_wave"
    assert name == "tree"                      # 15-dof dual-arm torso tree, the general kernel
    desc = TR.dual_panda_torso()
    m = W.RobotModel(desc)
    rng = np.random.default_rng(26)
    q = np.clip(rng.uniform(-0.8, 0.8, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    robot, ctrl, objs = controller_from_specs(desc, TR.dual_stack(m), B, device=0, leading_dimension=ld)
    ctrl.enableGravityCompensation(True)
    robot.setQ(q)
    robot.setDq(np.zeros((B, m.dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    objs[2].setGoalPosition(q + 0.2)
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, objs[1], None, "saip_cycle_wg_tree<32,512>"


def _pose_keys(task, rng, B, max_angle, shift=0.04):
    """(K, B, 12) keyframes of goal rows 0..11 around the task's goal: positions within `shift`, every rotation up to max_angle away from
    the one before (instance 0 exactly max_angle each time)"""
    g = task._get_goal()
    keys = np.empty((K, B, 12))
    R = g[:, 3:12].reshape(B, 3, 3)
    for k in range(K):
        axis = rng.normal(size=(B, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        angle = rng.uniform(0.0, max_angle, (B, 1))
        angle[0] = max_angle
        R = R @ GS.exp_so3(axis * angle)
        keys[k, :, :3] = g[:, :3] + rng.uniform(-shift, shift, (B, 3))
        keys[k, :, 3:] = R.reshape(B, 9)
    return keys


def _joint_keys(task, rng, B):
    q = task._get_goal()[:, :task.getTaskDof()]
    return q[None] + rng.uniform(-0.3, 0.3, (K,) + q.shape)


class Plan:
    """one schedule: task index in the stack, goal rows [first, first + count), keyframes (K, B, count) or (K, count), mode"""

    def __init__(self, task, first, keys, mode, stride=STRIDE):
        self.task, self.first, self.keys, self.mode, self.stride = task, first, np.asarray(keys, float), mode, stride
        self.count = self.keys.shape[-1]
        self.rot_at = 3 - first if (mode == GS.LINEAR and first <= 3 and first + self.count >= 12) else None

    def rows(self, c, B):
        """(B, count) goal rows of period c from the NumPy restatement"""
        r = GS.rows(self.keys, c, self.stride, self.mode, self.rot_at)
        return np.ascontiguousarray(np.broadcast_to(r, (B, self.count)))

    def attach(self, objs):
        objs[self.task].setGoalSchedule((self.first, self.count), self.keys, stride=self.stride, mode=self.mode)


def _finals(ctrl, objs):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    tau = ctrl.getTorques()
    return dict(q=q.copy(), dq=dq.copy(), tau=tau, status=ctrl.status.astype(np.float64), goals=[t._get_goal() for t in objs],
                log=ctrl.rolloutLog(), kernel=ctrl.kernelName())


def _roll(ctrl, grav, steps):
    ctrl.rolloutAsync(steps, DT, SUB, gravity=grav)


def _scheduled(stack, plans, calls=(PERIODS,)):
    """the rollout under test: the schedules attached, then rolloutAsync per entry of `calls`"""
    robot, ctrl, objs, mf, grav, _ = stack
    ctrl.recordRollouts(sum(calls), 1, REC, task=mf)
    for p in plans:
        p.attach(objs)
    for steps in calls:
        _roll(ctrl, grav, steps)
    return _finals(ctrl, objs)


def _host_loop(stack, plans, periods=PERIODS):
    """the oracle: every period's rows written from the host, one period per rollout call"""
    robot, ctrl, objs, mf, grav, _ = stack
    ctrl.recordRollouts(periods, 1, REC, task=mf)
    for c in range(periods):
        for p in plans:
            objs[p.task]._set_field(p.first, p.count, p.rows(c, ctrl.batch_size), "goal rows")
        _roll(ctrl, grav, 1)
    return _finals(ctrl, objs)


def _assert_equal_runs(a, b, kernel):
    assert a["kernel"] == kernel and b["kernel"] == kernel
    for k in ("q", "dq", "tau", "status"):
        assert _same_bits(a[k], b[k]), k
    for t, (ga, gb) in enumerate(zip(a["goals"], b["goals"])):
        assert _same_bits(ga, gb), ("goal of task", t)
    assert np.array_equal(a["log"]["period"], b["log"]["period"]) and len(a["log"]["period"]) == PERIODS
    for k in ("q", "dq", "tau", "position_error", "orientation_error", "status"):
        assert _same_bits(a["log"][k].astype(np.float64), b["log"][k].astype(np.float64)), ("log", k)
    assert np.abs(a["log"]["q"][-1] - a["log"]["q"][0]).max() > 1e-5       # the robots moved
    assert np.abs(a["log"]["position_error"]).max() > 1e-3


def _plans(name, objs, B, mode, seed, max_angle=0.2):
    """the schedule of a named case: a per-instance position and orientation schedule (HOLD) / a position schedule, rows 0..2 (LINEAR)
    of the motion-force task, or a schedule on the q goals of the joint task"""
    rng = np.random.default_rng(seed)
    if name == "joint":
        return [Plan(1, 0, _joint_keys(objs[1], rng, B), mode)]
    if mode == GS.HOLD:
        return [Plan(0, 0, _pose_keys(objs[0], rng, B, max_angle), mode)]
    keys = _pose_keys(objs[0], rng, B, max_angle)[:, :, :3]      # rows 0..2: the position
    return [Plan(0, 0, keys, mode)]


CASES = [("otg", "otg"), ("no_otg", "no_otg"), ("joint", "no_otg")]     # (schedule, stack)


# ------------------------------------------------------------------ 1. HOLD equals the host loop
@pytest.mark.parametrize("B,ld", SHAPES)
@pytest.mark.parametrize("case,stack", CASES)
def test_hold_equals_the_host_loop(case, stack, B, ld):
    s1, s2 = _stack(stack, B, ld), _stack(stack, B, ld)
    plans = _plans(case, s1[2], B, GS.HOLD, 11)
    got, ref = _scheduled(s1, plans), _host_loop(s2, plans)
    _assert_equal_runs(got, ref, s1[5])
    p = plans[0]
    assert _same_bits(got["goals"][p.task][:, p.first:p.first + p.count], p.keys[K - 1])     # the last keyframe is held


# ------------------------------------------------------------------ 2. LINEAR on non-rotation rows
@pytest.mark.parametrize("B,ld", SHAPES)
@pytest.mark.parametrize("case,stack", CASES)
def test_linear_equals_the_host_loop_fed_with_the_restatement(case, stack, B, ld):
    s1, s2, s3 = _stack(stack, B, ld), _stack(stack, B, ld), _stack(stack, B, ld)
    plans = _plans(case, s1[2], B, GS.LINEAR, 12)
    _assert_equal_runs(_scheduled(s1, plans), _host_loop(s2, plans), s1[5])
    # the goal rows after each of 6 single-period rollouts: the restatement's bits (a contracted FMA would show here); the counter
    # continues across the calls, rewind restarts it
    robot, ctrl, objs, mf, grav, _ = s3
    p = plans[0]
    p.attach(objs)
    for c in list(range(PERIODS)) + [0, 1]:
        if c == 0:
            ctrl.rewindGoalSchedules()
        assert objs[p.task].goalScheduleInfo()["period"] == c
        _roll(ctrl, grav, 1)
        ctrl.synchronize()
        assert _same_bits(objs[p.task]._get_goal()[:, p.first:p.first + p.count], p.rows(c, B)), c
    info = objs[p.task].goalScheduleInfo()
    assert info == dict(first=p.first, count=p.count, n_keyframes=K, stride=STRIDE, mode="linear", period=2)


# ------------------------------------------------------------------ 3. slerp on the orientation rows
def test_slerp_rows_match_the_restatement():
    B = 70
    s1, s2 = _stack("no_otg", B), _stack("no_otg", B)
    rng = np.random.default_rng(13)
    plan = Plan(0, 0, _pose_keys(s1[2][0], rng, B, 3.0, shift=0.02), GS.LINEAR)
    assert plan.rot_at == 3
    R = plan.keys[:, :, 3:].reshape(K, B, 3, 3)
    apart = np.arccos(np.clip((np.einsum("kbij,kbij->kb", R[:-1], R[1:]) - 1.0) / 2.0, -1.0, 1.0))
    assert abs(apart[:, 0] - 3.0).max() < 1e-9 and apart.max() < 3.0 + 1e-9       # up to 3.0 rad between consecutive keyframes
    robot, ctrl, objs, mf, grav, kernel = s1
    ctrl.recordRollouts(PERIODS, 1, REC, task=mf)
    plan.attach(objs)
    worst = 0.0
    for c in range(PERIODS):
        _roll(ctrl, grav, 1)
        ctrl.synchronize()
        rows, ref = objs[0]._get_goal()[:, :12], plan.rows(c, B)
        assert _same_bits(rows[:, :3], ref[:, :3]), c                               # the position rows: component-wise, exact
        i, s = GS.index_fraction(c, K, STRIDE)
        if s == 0.0:
            assert _same_bits(rows, plan.keys[i]), c                               # on a keyframe: the keyframe exactly
        Rd = rows[:, 3:].reshape(B, 3, 3)
        assert np.abs(np.swapaxes(Rd, 1, 2) @ Rd - np.eye(3)).max() < 1e-13
        worst = max(worst, np.abs(rows[:, 3:] - ref[:, 3:]).max())
    bound = min(64.0 * (SLERP_WORST_DERIVED if SLERP_WORST_MEASURED is None else SLERP_WORST_MEASURED), 1e-11)
    print("slerp rows: worst |device - NumPy| entry", worst, "bound", bound)
    got = _finals(ctrl, objs)
    ref = _host_loop(s2, [plan])
    err = max(W.torque_error(got["log"]["tau"], ref["log"]["tau"]), W.torque_error(got["tau"], ref["tau"]))
    print("closed loop on slerp rows: worst relative torque difference", err, "bound", TORQUE_TOL, "recorded", CLOSED_LOOP_WORST_MEASURED)
    assert worst <= bound
    assert got["kernel"] == kernel and np.array_equal(got["status"], ref["status"])
    assert err < TORQUE_TOL


# ------------------------------------------------------------------ 4. broadcast equals per-instance
@pytest.mark.parametrize("mode", [GS.HOLD, GS.LINEAR])
def test_uniform_keyframes_equal_tiled_ones(mode):
    B = 70
    s1, s2 = _stack("otg", B), _stack("otg", B)
    rng = np.random.default_rng(14)
    one = _pose_keys(s1[2][0], rng, B, 0.3)[:, 5]                 # (K, 12): one instance's keyframes for everybody
    uniform, tiled = Plan(0, 0, one, mode), Plan(0, 0, np.repeat(one[:, None], B, axis=1), mode)
    assert uniform.keys.shape == (K, 12) and tiled.keys.shape == (K, B, 12)
    a, b = _scheduled(s1, [uniform]), _scheduled(s2, [tiled])
    _assert_equal_runs(a, b, s1[5])
    assert _same_bits(a["goals"][0][:, :12], np.broadcast_to(one[K - 1], (B, 12)))


# ------------------------------------------------------------------ 5. layout and isolation
def test_only_the_scheduled_rows_and_columns_are_written():
    from sai_primitives_amd import capi
    L = capi.lib()
    B, ld = 33, 128
    stack = _stack("no_otg", B, ld)
    robot, ctrl, objs, mf, grav, kernel = stack
    assert L.saip_batch_ld(ctrl._h) == ld
    rng = np.random.default_rng(15)
    before = []
    for t in (0, 1):       # a sentinel into columns B..ld-1 of every goal row
        comps, ptr = L.saip_batch_goal_components(ctrl._h, t), L.saip_batch_device_goal(ctrl._h, t)
        g = _d2h(ptr, (comps, ld))
        g[:, B:] = SENTINEL
        _h2d(ptr, g)
        before.append(g)
    # one task scheduled: rows 12..17 (linear and angular velocity) of the motion-force task
    vel = Plan(0, 12, rng.uniform(-0.05, 0.05, (K, B, 6)), GS.LINEAR)
    vel.attach(objs)
    _roll(ctrl, grav, 4)
    ctrl.synchronize()
    g0, g1 = (_d2h(L.saip_batch_device_goal(ctrl._h, t), before[t].shape) for t in (0, 1))
    assert _same_bits(g1, before[1])                                                   # the second task's goal is untouched
    assert _same_bits(g0[:12], before[0][:12]) and _same_bits(g0[18:], before[0][18:])   # rows outside the range
    assert _same_bits(g0[12:18, B:], before[0][12:18, B:])                             # padding columns of the scheduled rows
    assert _same_bits(g0[12:18, :B], vel.rows(3, B).T)      # period 3: half way from keyframe 1 to keyframe 2
    keys = _d2h(objs[0].goalScheduleDevice(), (K, 6, ld))                              # device layout [K][count][ld], padding zeroed
    assert _same_bits(keys[:, :, :B], vel.keys.transpose(0, 2, 1)) and not keys[:, :, B:].any()
    objs[0].clearGoalSchedule()
    assert objs[0].goalScheduleDevice() is None
    # two tasks scheduled at once (one launch serves both): each gets its own rows, and the run equals the host loop
    s1, s2 = _stack("no_otg", B, ld), _stack("no_otg", B, ld)
    plans = [Plan(0, 0, _pose_keys(s1[2][0], rng, B, 0.2)[:, :, :3], GS.LINEAR), Plan(1, 0, _joint_keys(s1[2][1], rng, B), GS.HOLD)]
    got = _scheduled(s1, plans)
    _assert_equal_runs(got, _host_loop(s2, plans), s1[5])
    assert _same_bits(got["goals"][0][:, :3], plans[0].keys[K - 1]) and _same_bits(got["goals"][1][:, :7], plans[1].keys[K - 1])


# ------------------------------------------------------------------ 6. not a chain-only feature
@pytest.mark.parametrize("name", ["chain30", "tree"])
def test_hold_on_the_wavefront_and_tree_kernels(name):
    B = 33
    s1, s2 = _stack(name, B), _stack(name, B)
    rng = np.random.default_rng(16)
    t = s1[2].index(s1[3])
    plans = [Plan(t, 0, _pose_keys(s1[3], rng, B, 0.1, shift=0.02), GS.HOLD)]
    _assert_equal_runs(_scheduled(s1, plans), _host_loop(s2, plans), s1[5])


# ------------------------------------------------------------------ 7. lifecycle
def test_detach_rewrite_and_the_counter():
    B = 70
    s1, s2 = _stack("otg", B), _stack("otg", B)
    rng = np.random.default_rng(17)
    plan = Plan(0, 0, _pose_keys(s1[2][0], rng, B, 0.2)[:, :, :3], GS.LINEAR)
    robot, ctrl, objs, mf, grav, kernel = s1
    plan.attach(objs)
    with pytest.raises(Exception, match="already has a goal schedule"):
        plan.attach(objs)
    _roll(ctrl, grav, 3)                           # periods 0..2: the goal stands at keyframe 1
    # cycles outside a rollout apply no schedule and leave the counter alone
    ctrl.stepAsync()
    ctrl.synchronize()
    assert objs[0].goalScheduleInfo()["period"] == 3
    assert _same_bits(objs[0]._get_goal()[:, :3], plan.keys[1])
    objs[0].clearGoalSchedule()                    # mid-sequence: the last goal stays in place
    assert _same_bits(objs[0]._get_goal()[:, :3], plan.keys[1])
    _roll(ctrl, grav, 4)
    got = _finals_plain(ctrl, objs)
    # ... and the later rollouts are those of a batch that never had a schedule and was given that goal
    robot2, ctrl2, objs2, _, _, _ = s2
    for c in range(3):
        objs2[0].setGoalPosition(plan.rows(c, B))
        _roll(ctrl2, grav, 1)
    ctrl2.stepAsync()
    _roll(ctrl2, grav, 4)                          # more than one period per call: the fused integrate + OTG launch is back
    ref = _finals_plain(ctrl2, objs2)
    for k in got:
        assert _same_bits(got[k], ref[k]), k
    # keyframes rewritten in place between rollouts take effect
    new = Plan(0, 0, plan.keys + rng.uniform(-0.01, 0.01, plan.keys.shape), GS.LINEAR)
    plan.attach(objs)
    ld = ctrl.devicePointers()["ld"]
    _roll(ctrl, grav, 1)
    ctrl.synchronize()
    assert _same_bits(objs[0]._get_goal()[:, :3], plan.keys[0])
    dev = np.zeros((K, 3, ld))
    dev[:, :, :B] = new.keys.transpose(0, 2, 1)
    _h2d(objs[0].goalScheduleDevice(), dev)
    _roll(ctrl, grav, 1)
    ctrl.synchronize()
    assert _same_bits(objs[0]._get_goal()[:, :3], new.rows(1, B)) and not _same_bits(new.rows(1, B), plan.rows(1, B))


def _finals_plain(ctrl, objs):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(np.float64), goal=objs[0]._get_goal(),
                desired=objs[0]._desired_block())
