"""Every tree entry point besides the plain cycle (robots and the NumPy tree oracle: tests/trees.py), on the 15-dof torso carrying two Pandas:
  * blended singularity strategies over several cycles of near-singular postures (the handler's perturbed-pose classification walks the
    tree) and closed-loop force control, against the restatement with the tree kinematics swapped in;
  * motion-force task diagnostics on branch links (a fixed link at the end of one arm, a middle link of the other) against NumPy;
  * the Cartesian OTG re-initialised on a tree: its output sits at the current pose of each control frame;
  * the per-task TemplateTask entry points driven by hand reproduce the controller;
  * rolloutAsync(K) equals K periods issued one call at a time; energy is conserved without torque, gravity and damping;
  * batch sizes 1, 63 and 65 and a padded leading dimension give the same per-instance results."""
import numpy as np
import pytest

import chains as CH
import trees as TR
import workloads as W

pytestmark = pytest.mark.gpu
DESC = TR.dual_panda_torso()


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _model():
    return W.RobotModel(DESC)


def _ctrl(tasks, B, opts=None, otg=False, ld=None):
    """controller on the torso tree; otg: motion-force tasks with their internal OTG on (joint tasks always off)"""
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(DESC, tasks, B, device=0, disable_otg=not otg, leading_dimension=ld)
    for t, spec in zip(objs, tasks):
        if otg and spec["type"] == "joint":
            t.disableInternalOtg()
    opts = opts or {}
    ctrl.enableGravityCompensation(bool(opts.get("gravity_comp")))
    ctrl.enableTorqueSaturation(bool(opts.get("torque_saturation")))
    ctrl.enableJointLimitAvoidance(bool(opts.get("joint_limit_avoidance")))
    return robot, ctrl, objs


def _cycle(robot, ctrl, q, dq, goals):
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    ctrl.setGoals(goals)
    return ctrl.computeControlTorques().copy(), ctrl.status.copy()


def _state(rng, m, B, spread=0.8):
    q = np.clip(rng.uniform(-spread, spread, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    return q, rng.uniform(-0.5, 0.5, (B, m.dof))


def _oracle_states(tasks, n, B):
    return [[dict(int_pos=np.zeros(3), int_ori=np.zeros(3)) if t["type"] == "motion_force" else dict(int_err=np.zeros(n)) for t in tasks]
            for _ in range(B)]


def test_blended_strategies_over_cycles_on_tree(sp):
    """both arms in config 12's postures (a third inside the blending region, elbow nearly straight), strategies on, five cycles of a
    drifting state: status words (8 = blended) and torques against the restatement carrying the handler state per instance"""
    m = _model()
    B = 36
    rng = np.random.default_rng(21)
    q0 = np.zeros((B, m.dof))
    q0[:, 0] = rng.uniform(-0.5, 0.5, B)
    q0[:, 1:8] = W.make_inputs(12, B)["q"]
    q0[:, 8:15] = W.make_inputs(12, B, shard=1)["q"]
    dq = rng.uniform(-0.2, 0.2, (B, m.dof))
    tasks = TR.dual_stack(m)
    goals = TR.tree_goals(rng, m, tasks, q0)
    robot, ctrl, _ = _ctrl(tasks, B)
    states = _oracle_states(tasks, m.dof, B)
    q = q0.copy()
    seen = 0
    with TR.tree_oracle() as RS:
        for cyc in range(5):
            tau, st = _cycle(robot, ctrl, q, dq, goals)
            ref, rst = np.zeros_like(q), np.zeros(B, np.uint8)
            for b in range(B):
                info = {}
                try:
                    ref[b] = RS.controller_step_single(m, tasks, q[b], dq[b], [g[b] for g in goals], state=states[b], info=info)
                    rst[b] = 8 if info.get("blended") else 0
                except RS.Singular:
                    rst[b] = 1
            assert np.array_equal(st, rst), (cyc, np.flatnonzero(st != rst)[:8], st[st != rst][:8], rst[st != rst][:8])
            ok = (rst & 1) == 0
            err = W.torque_error(tau[ok], ref[ok])
            print("cycle", cyc, "blended", int(((rst & 8) != 0).sum()), "of", B, "max rel error", err)
            assert err < 1e-8, (cyc, err)
            seen += int(((rst & 8) != 0).sum())
            q = q + 1e-3 * dq + 2e-3 * rng.standard_normal(q.shape)
    assert seen > 0  # the blended branch (and its perturbed-pose classification walk) did run


def test_closed_loop_force_on_tree(sp):
    m = _model()
    B = 48
    rng = np.random.default_rng(22)
    c, s_ = np.cos(0.4), np.sin(0.4)
    contact = W.motion_force_task("contact", "left_end-effector", (0, 0, 0.07), force_dim=1, force_axis=[0.0, 0.0, 1.0], moment_dim=2,
                                  moment_axis=[0.0, 0.0, 1.0], param_in_compliant_frame=True, cl_force=True, cl_moment=True, kp_force=0.9,
                                  kv_force=12.0, ki_force=1.7, kp_moment=0.6, kv_moment=8.0, ki_moment=1.1, kff_force=0.9, kff_moment=0.8,
                                  max_force_fb=4.0, max_moment_fb=0.5, Rcs=[[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], tcs=[0.01, -0.02, 0.05])
    tasks = [contact, W.motion_force_task("right", "right_link7", (0.0, 0.0, 0.1)), W.joint_task("posture")]
    opts = dict(gravity_comp=True)
    q, dq = _state(rng, m, B)
    goals = TR.tree_goals(rng, m, tasks, q)
    robot, ctrl, _ = _ctrl(tasks, B, opts)
    states = _oracle_states(tasks, m.dof, B)
    with TR.tree_oracle() as RS:
        for cyc in range(3):  # the force and moment integrators advance from cycle to cycle
            tau, st = _cycle(robot, ctrl, q, dq, goals)
            ref, rst = np.zeros_like(q), np.zeros(B, np.uint8)
            for b in range(B):
                info = {}
                try:
                    ref[b] = RS.controller_step_single(m, tasks, q[b], dq[b], [g[b] for g in goals], state=states[b], info=info, **opts)
                    rst[b] = 8 if info.get("blended") else 0
                except RS.Singular:
                    rst[b] = 1
            assert np.array_equal(st, rst), cyc
            ok = (rst & 1) == 0
            assert ok.sum() > B // 2
            err = W.torque_error(tau[ok], ref[ok])
            print("closed-loop force cycle", cyc, "max rel error", err)
            assert err < 1e-8, (cyc, err)


def test_task_diagnostics_on_branch_links(sp):
    """position / orientation error and current twist of a full task on a fixed link at the end of the left arm and of a position task on
    the right arm's link4, against NumPy (full task: sigma = I, P = I; position task: sigma_ori = 0, P_ori = 0)"""
    m = _model()
    B = 65
    rng = np.random.default_rng(23)
    q, dq = _state(rng, m, B)
    pos = np.array([0.01, -0.02, 0.05])
    tasks = [W.motion_force_task("left", "left_end-effector", pos), W.motion_force_task("right4", "right_link4", pos, dirs_trans=CH.XYZ, dirs_rot=None),
             W.joint_task("posture")]
    goals = TR.tree_goals(rng, m, tasks, q)
    robot, ctrl, objs = _ctrl(tasks, B)
    _cycle(robot, ctrl, q, dq, goals)
    fr = TR.tree_fk(m, q)
    for t, (obj, link, full) in enumerate(((objs[0], "left_end-effector", True), (objs[1], "right_link4", False))):
        li = m.link_index(link)
        R, o = fr[li]
        x = o + R @ pos
        J = TR.tree_jacobian(m, fr, li, x)
        v, w = np.einsum("bij,bj->bi", J[:, :3], dq), np.einsum("bij,bj->bi", J[:, 3:], dq)
        Rg = goals[t][:, 3:12].reshape(B, 3, 3)
        oe = -0.5 * np.cross(np.swapaxes(R, 1, 2), np.swapaxes(Rg, 1, 2)).sum(axis=1)
        assert np.abs(obj.getPositionError() - (goals[t][:, :3] - x)).max() < 1e-12, link
        assert np.abs(obj.getOrientationError() - (oe if full else 0.0)).max() < 1e-12, link
        assert np.abs(obj.getCurrentLinearVelocity() - v).max() < 1e-12, link
        assert np.abs(obj.getCurrentAngularVelocity() - (w if full else 0.0)).max() < 1e-12, link


def test_cartesian_otg_reinitialised_on_tree(sp):
    """reinitializeTasks with the Cartesian OTGs on: the trajectory starts, and with the goal at the current pose stays, at the pose of each
    control frame (the OTG's re-initialisation walks the tree)"""
    m = _model()
    B = 63
    rng = np.random.default_rng(24)
    q, _ = _state(rng, m, B)
    tasks = TR.dual_stack(m)
    robot, ctrl, objs = _ctrl(tasks, B, otg=True)
    robot.setQ(q)
    robot.setDq(np.zeros((B, m.dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    ctrl.computeControlTorques()
    fr = TR.tree_fk(m, q)
    for obj, link in ((objs[0], "left_link7"), (objs[1], "right_link7")):
        R, o = fr[m.link_index(link)]
        x = o + R @ np.array([0.0, 0.0, 0.1])
        assert np.abs(obj.getGoalPosition() - x).max() < 1e-12, link
        assert np.abs(obj.getDesiredPosition() - x).max() < 1e-12, link
        assert np.abs(obj.getDesiredOrientation() - R).max() < 1e-12, link


def _set_goal(task, spec, g):
    if spec["type"] == "motion_force":
        task.setGoalPosition(g[:, 0:3])
        task.setGoalOrientation(g[:, 3:12].reshape(-1, 3, 3))
        task.setGoalLinearVelocity(g[:, 12:15])
        task.setGoalAngularVelocity(g[:, 15:18])
        task.setGoalLinearAcceleration(g[:, 18:21])
        task.setGoalAngularAcceleration(g[:, 21:24])
    else:
        k = task.getTaskDof()
        task.setGoalPosition(g[:, :k])
        task.setGoalVelocity(g[:, k:2 * k])
        task.setGoalAcceleration(g[:, 2 * k:3 * k])


def test_per_task_entry_points_reproduce_the_controller(sp):
    """TemplateTask's updateTaskModel(N_prec) / getTaskAndPreviousNullspace / computeTorques(tau_prec) driven by hand (example 04) equal
    RobotController::computeControlTorques on the same tree and state"""
    from sai_primitives_amd.controller import tasks_from_specs
    m = _model()
    B = 64
    rng = np.random.default_rng(25)
    q, dq = _state(rng, m, B)
    tasks = TR.dual_stack(m)
    goals = TR.tree_goals(rng, m, tasks, q)
    robot, ctrl, _ = _ctrl(tasks, B)
    ref, st = _cycle(robot, ctrl, q, dq, goals)
    objs = tasks_from_specs(robot, tasks)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    N_prec = np.eye(m.dof)
    for t in objs:
        t.updateTaskModel(N_prec)
        N_prec = t.getTaskAndPreviousNullspace()
    total = np.zeros((B, m.dof))
    for t, spec, g in zip(objs, tasks, goals):
        _set_goal(t, spec, g)
        total = total + t.computeTorques(total)
    ok = (st & 1) == 0
    assert ok.sum() > B // 2
    assert W.torque_error(total[ok], ref[ok]) < 1e-10


def test_rollout_equals_stepwise_periods_on_tree(sp):
    m = _model()
    B = 40
    rng = np.random.default_rng(26)
    q, _ = _state(rng, m, B)
    tasks = TR.dual_stack(m)
    shift = rng.uniform(-0.04, 0.04, (B, 3))
    out = []
    for fused in (True, False):
        robot, ctrl, objs = _ctrl(tasks, B, dict(gravity_comp=True), otg=True)
        robot.setQ(q)
        robot.setDq(np.zeros((B, m.dof)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        for t in objs[:2]:
            t.setGoalPosition(t.getGoalPosition() + shift)
        objs[2].setGoalPosition(q + 0.2)
        ctrl.updateControllerTaskModels()
        K = 17
        if fused:
            ctrl.rolloutAsync(K, 5e-4, 2)
        else:
            for _ in range(K):
                ctrl.stepAsync()
                ctrl.integrate(5e-4, 2)
        ctrl.synchronize()
        q1, dq1 = ctrl.pullState()
        out.append((q1.copy(), dq1.copy(), ctrl.getTorques(), objs[0].getDesiredPosition(), objs[1].getDesiredPosition()))
        assert (ctrl.status & 1).sum() == 0
    for a, b in zip(*out):
        assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max()), np.abs(a - b).max()
    assert np.abs(out[0][0] - q).max() > 1e-4


def test_energy_is_conserved_on_tree(sp):
    m = _model()
    B = 16
    rng = np.random.default_rng(27)
    q, dq = _state(rng, m, B)
    robot, ctrl, _ = _ctrl([W.joint_task("posture")], B)
    ctrl.setTorques(np.zeros((B, m.dof)))
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.integrate(2e-5, 2500, gravity=(0.0, 0.0, 0.0))  # 0.05 s of free motion
    ctrl.synchronize()
    q1, dq1 = ctrl.pullState()
    with TR.tree_oracle() as RS:
        E0 = RS.total_energy(m, q, dq, g=(0.0, 0.0, 0.0))
        E1 = RS.total_energy(m, q1, dq1, g=(0.0, 0.0, 0.0))
    drift = np.abs(E1 - E0).max()
    print("energy drift", drift, "of", E0.min(), E0.max())
    assert np.abs(q1 - q).max() > 0.005 and drift < 1e-3 * max(1.0, E0.max())


def test_batch_layouts_on_tree(sp):
    """B = 1, 63, 65 and 65 at a padded leading dimension (128): every instance's torques and status equal those of the same instance in
    the 65-instance batch (one workgroup per instance: nothing couples them)"""
    m = _model()
    rng = np.random.default_rng(28)
    q, dq = _state(rng, m, 65)
    tasks = TR.dual_stack(m)
    goals = TR.tree_goals(rng, m, tasks, q)
    opts = dict(gravity_comp=True, torque_saturation=True)
    robot, ctrl, _ = _ctrl(tasks, 65, opts)
    ref, rst = _cycle(robot, ctrl, q, dq, goals)
    assert ((rst & 1) == 0).sum() > 32
    for B, ld in ((1, None), (63, None), (65, 128)):
        robot, ctrl, _ = _ctrl(tasks, B, opts, ld=ld)
        tau, st = _cycle(robot, ctrl, q[:B], dq[:B], [g[:B] for g in goals])
        assert np.array_equal(st, rst[:B]), B
        ok = (st & 1) == 0
        assert np.array_equal(tau[ok], ref[:B][ok]), B
