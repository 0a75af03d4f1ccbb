"""Kinematic trees on the device (robots and the NumPy tree oracle: tests/trees.py):
  * a chain written as a tree, and a Panda with fixed side frames, run exactly the serial code: same kernel, bit-identical torques, status,
    pose readback and model queries;
  * a forest (two arms on a fixed torso) decouples: over 20 closed-loop rollout periods with the Cartesian OTGs on, its state, torques,
    OTG output and status equal two serial single-arm batches on the fast kernels;
  * true trees (a torso carrying two arms, random trees) against the restatement with the tree kinematics swapped in: task stacks,
    the hierarchy property, model queries, one integration step, pose readback and re-initialisation."""
import numpy as np
import pytest

import chains as CH
import trees as TR
import workloads as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _ctrl(desc, tasks, B, opts=None, kernel=0):
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(desc, tasks, B, device=0)
    ctrl.setKernel(kernel)
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


def _state(rng, model, B, spread=1.0):
    q = np.clip(rng.uniform(-spread, spread, (B, model.dof)), model.q_lower + 0.1, model.q_upper - 0.1)
    return q, rng.uniform(-0.5, 0.5, (B, model.dof))


@pytest.mark.parametrize("name,link", [("panda_arm", "link7"), ("panda_sliding_base", None), ("chain30", None)])
def test_chain_written_as_tree_is_bit_identical(sp, name, link):
    desc = sp.load_robot_description(name)
    model = W.RobotModel(desc)
    tip = link or desc["links"][-1]["name"]
    tasks = [W.motion_force_task("hand", tip, (0.0, 0.0, 0.1)), W.joint_task("posture")]
    rng = np.random.default_rng(1)
    B = 96
    q, dq = _state(rng, model, B)
    goals = CH.goals(rng, model, tasks, q)
    out = []
    for d in (desc, TR.chain_as_tree(desc)):
        robot, ctrl, objs = _ctrl(d, tasks, B, dict(gravity_comp=True))
        tau, st = _cycle(robot, ctrl, q, dq, goals)
        pose = objs[0].getCurrentPosition().copy()
        out.append((tau, st, ctrl.kernelName(), pose, robot.M().copy(), robot.JWorldFrame(tip).copy(), robot.jointGravityVector().copy()))
    a, b = out
    assert a[2] == b[2]
    for x, y in zip(a, b):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_side_frames_are_bit_identical_to_the_chain(sp):
    panda = sp.load_robot_description("panda_arm")
    model = W.RobotModel(panda)
    tasks = [W.motion_force_task("hand", "link7", (0.0, 0.0, 0.1)), W.joint_task("posture")]
    rng = np.random.default_rng(2)
    B = 128
    q, dq = _state(rng, model, B)
    goals = CH.goals(rng, model, tasks, q)
    r1, c1, _ = _ctrl(panda, tasks, B, dict(gravity_comp=True))
    r2, c2, _ = _ctrl(TR.panda_with_side_frames(), tasks, B, dict(gravity_comp=True))
    t1, s1 = _cycle(r1, c1, q, dq, goals)
    t2, s2 = _cycle(r2, c2, q, dq, goals)
    assert c1.kernelName() == c2.kernelName()
    assert np.array_equal(t1, t2) and np.array_equal(s1, s2)
    # side frames as task links and query frames, against the tree oracle
    side = W.RobotModel(TR.panda_with_side_frames(True))
    r3, c3, objs = _ctrl(TR.panda_with_side_frames(True),
                         [W.motion_force_task("cam", "camera", (0.0, 0.0, 0.05)), W.joint_task("posture")], B)
    r3.setQ(q)
    r3.setDq(dq)
    r3.updateModel()
    fr = TR.tree_fk(side, q)
    for name in ("camera", "tool_side"):
        R, o = fr[side.link_index(name)]
        assert np.abs(r3.positionInWorld(name) - o).max() < 1e-12
        assert np.abs(r3.JWorldFrame(name) - TR.tree_jacobian(side, fr, side.link_index(name), o)).max() < 1e-12
    c3.updateControllerTaskModels()
    R, o = fr[side.link_index("camera")]
    assert np.abs(objs[0].getCurrentPosition() - (o + R @ np.array([0.0, 0.0, 0.05]))).max() < 1e-12


def _otg_ctrl(desc, tasks, B, opts):
    """motion-force tasks with their internal OTG on, joint tasks with it off"""
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(desc, tasks, B, device=0, disable_otg=False)
    for t, spec in zip(objs, tasks):
        if spec["type"] == "joint":
            t.disableInternalOtg()
    ctrl.enableGravityCompensation(bool(opts.get("gravity_comp")))
    ctrl.enableTorqueSaturation(bool(opts.get("torque_saturation")))
    ctrl.enableJointLimitAvoidance(bool(opts.get("joint_limit_avoidance")))
    return robot, ctrl, objs


def _arm_alone(side):
    """one arm of dual_panda_fixed_torso as a serial chain, mounted where the torso holds it"""
    arm = TR._arm("", None, *(([0.0, 0.25, 0.7], [-0.6, 0.0, 0.0]) if side == "left" else ([0.0, -0.25, 0.7], [0.6, 0.0, 0.0])))
    for l in arm:
        l.pop("parent")
    return dict(name=side, links=arm)


def test_forest_decouples_into_two_serial_batches(sp):
    """[MF left, MF right, full JointTask] on the forest, Cartesian OTGs on (their re-initialisation walks the tree), joint OTG off (Ruckig
    synchronises every dof of one joint task), over 20 closed-loop rollout periods: each arm equals a serial [MF, JointTask] batch of its own
    on the fast kernels -- state, torques, OTG output and status"""
    forest = TR.dual_panda_fixed_torso()
    fm = W.RobotModel(forest)
    opts = dict(gravity_comp=True, torque_saturation=True, joint_limit_avoidance=True)
    B = 64
    rng = np.random.default_rng(3)
    q, _ = _state(rng, fm, B, 0.8)
    tasks = TR.dual_stack(fm)
    K, sim_dt = 20, 5e-4
    robot, ctrl, objs = _otg_ctrl(forest, tasks, B, opts)
    robot.setQ(q)
    robot.setDq(np.zeros((B, 14)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    shift = rng.uniform(-0.05, 0.05, (B, 3))
    for t in objs[:2]:
        t.setGoalPosition(t.getGoalPosition() + shift)
    qg = q + rng.uniform(-0.2, 0.2, q.shape)
    objs[2].setGoalPosition(qg)
    ctrl.updateControllerTaskModels()
    ctrl.rolloutAsync(K, sim_dt, 2)
    ctrl.synchronize()
    assert ctrl.kernelName().startswith("saip_cycle_wg_tree")
    qf, dqf = ctrl.pullState()
    tau_f, st_f = ctrl.getTorques(), ctrl.status.copy()
    des_f = [t.getDesiredPosition().copy() for t in objs[:2]]
    assert np.abs(qf - q).max() > 1e-3  # the arms did move
    st_or = np.zeros(B, np.uint8)
    for side, sl, g in (("left", slice(0, 7), 0), ("right", slice(7, 14), 1)):
        st = [W.motion_force_task(side, "link7", (0.0, 0.0, 0.1)), W.joint_task("posture")]
        r, c_, o = _otg_ctrl(_arm_alone(side), st, B, opts)
        r.setQ(q[:, sl])
        r.setDq(np.zeros((B, 7)))
        r.updateModel()
        c_.reinitializeTasks()
        o[0].setGoalPosition(o[0].getGoalPosition() + shift)
        o[1].setGoalPosition(qg[:, sl])
        c_.updateControllerTaskModels()
        c_.rolloutAsync(K, sim_dt, 2)
        c_.synchronize()
        qa, dqa = c_.pullState()
        assert not c_.kernelName().startswith("saip_cycle_wg")  # the arm alone runs a fast kernel
        for a, b in ((qf[:, sl], qa), (dqf[:, sl], dqa), (tau_f[:, sl], c_.getTorques()), (des_f[g], o[0].getDesiredPosition())):
            assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max()), (side, np.abs(a - b).max())
        st_or |= c_.status
    assert np.array_equal(st_f, st_or)


def _tree_cases():
    return {"torso": TR.dual_panda_torso(), **{f"random{s}_{n}": TR.random_tree(s, n) for s, n in ((11, 4), (12, 9), (13, 20))}}


def _stacks(desc):
    m = W.RobotModel(desc)
    if desc["name"] == "dual_panda_torso":
        return {"full": (TR.dual_stack(m), dict(gravity_comp=True)),
                "partial": (TR.dual_stack(m, partial=True), dict(torque_saturation=True)),
                "bie": (TR.dual_stack(m, decoupling=W.BOUNDED_INERTIA_ESTIMATES), dict(gravity_comp=True)),
                "unhandled": ([W.motion_force_task("left", "left_link7", (0.0, 0.0, 0.1), singularity_handling=False), W.joint_task("posture")], {}),
                "joint_selection": ([W.joint_task("sel", S=CH._general_selection(m.dof), kp=40.0, kv=12.0)], dict(gravity_comp=True))}
    movable = [l["name"] for l in desc["links"] if l["joint_type"] != "fixed"]
    par = TR.parent_index(m)
    depth = [0] * m.nl
    for i in range(m.nl):
        depth[i] = (depth[par[i]] + 1) if par[i] >= 0 else 1
    tip = max(range(m.nl), key=lambda i: depth[i] * 100 + i)
    st = {"joint": ([W.joint_task("posture", ki=1.0)], dict(gravity_comp=True))}
    if m.dof >= 3:
        st["position_joint"] = ([W.motion_force_task("hand", desc["links"][tip]["name"], (0.0, 0.02, 0.1), dirs_trans=CH.XYZ, dirs_rot=None),
                                 W.joint_task("posture")], dict(gravity_comp=True, torque_saturation=True))
    assert movable
    return st


@pytest.mark.parametrize("case", sorted(_tree_cases()))
def test_tree_matches_tree_oracle(sp, case):
    desc = _tree_cases()[case]
    m = W.RobotModel(desc)
    B = 64
    rng = np.random.default_rng(5)
    for sname, (tasks, opts) in _stacks(desc).items():
        q, dq = _state(rng, m, B, 0.9)
        goals = TR.tree_goals(rng, m, tasks, q)
        robot, ctrl, _ = _ctrl(desc, tasks, B, opts)
        tau, st = _cycle(robot, ctrl, q, dq, goals)
        with TR.tree_oracle() as RS:
            ref, rst = RS.controller_step(m, tasks, q, dq, goals, **opts)
        ok = ((rst & 1) == 0) & ((st & 1) == 0)
        assert ok.sum() > B // 2, (case, sname, np.bincount(rst), np.bincount(st))
        assert np.array_equal(st[ok], rst[ok]), (case, sname)
        err = W.torque_error(tau[ok], ref[ok])
        print(case, sname, "max rel error", err)
        assert err < 1e-8, (case, sname, err)


def test_hierarchy_property_on_tree(sp):
    desc = TR.dual_panda_torso()
    m = W.RobotModel(desc)
    B = 32
    rng = np.random.default_rng(6)
    q, dq = _state(rng, m, B, 0.8)
    t1 = W.motion_force_task("left", "left_link7", (0.0, 0.0, 0.1))
    goals = TR.tree_goals(rng, m, [t1], q)
    robot, ctrl, _ = _ctrl(desc, [t1, W.joint_task("posture")], B)
    tau_all, st = _cycle(robot, ctrl, q, dq, goals + [np.concatenate([q + 0.3, np.zeros((B, 2 * m.dof))], axis=1)])
    tau_1, _ = _cycle(robot, ctrl, q, dq, goals + [np.concatenate([q, np.zeros((B, 2 * m.dof))], axis=1)])
    fr = TR.tree_fk(m, q)
    R, o = fr[m.link_index("left_link7")]
    J = TR.tree_jacobian(m, fr, m.link_index("left_link7"), o + R @ np.array([0.0, 0.0, 0.1]))
    M = TR.tree_mass_matrix(m, fr)
    acc = np.einsum("bij,bj->bi", J, np.linalg.solve(M, (tau_all - tau_1)[..., None])[..., 0])
    ok = (st & 1) == 0
    assert np.abs(acc[ok]).max() < 1e-8 * max(1.0, np.abs(tau_all).max())


@pytest.mark.parametrize("case", sorted(_tree_cases()))
def test_tree_model_queries_and_integrate(sp, case):
    desc = _tree_cases()[case]
    m = W.RobotModel(desc)
    B = 65
    rng = np.random.default_rng(7)
    q, dq = _state(rng, m, B, 0.9)
    robot, ctrl, _ = _ctrl(desc, [W.joint_task("posture")], B)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    fr = TR.tree_fk(m, q)
    for li in range(m.nl):
        name = m.links[li]["name"]
        R, o = fr[li]
        assert np.abs(robot.positionInWorld(name) - o).max() < 1e-12, name
        assert np.abs(robot.rotationInWorld(name) - R).max() < 1e-12, name
        assert np.abs(robot.JWorldFrame(name) - TR.tree_jacobian(m, fr, li, o)).max() < 1e-12, name
    M = TR.tree_mass_matrix(m, fr)
    assert np.abs(robot.M() - M).max() < 1e-10 * max(1.0, np.abs(M).max())
    assert np.abs(robot.MInv() - np.linalg.inv(M)).max() < 1e-7 * max(1.0, np.abs(np.linalg.inv(M)).max())
    with TR.tree_oracle() as RS:
        g = RS.gravity_vector(m, fr)
        assert np.abs(robot.jointGravityVector() - g).max() < 1e-10 * max(1.0, np.abs(g).max())
        qdd0 = RS.forward_dynamics(m, q, dq, np.zeros((B, m.dof)), g=(0.0, 0.0, 0.0))
        h = -np.einsum("bij,bj->bi", M, qdd0)   # C(q, dq) dq from the Lagrangian forward dynamics without gravity and torque
        assert np.abs(robot.coriolisForce() - h).max() < 1e-6 * max(1.0, np.abs(h).max())
        tau = rng.uniform(-5, 5, (B, m.dof))
        ctrl.setTorques(tau)
        dt = 1e-4
        ctrl.integrate(dt, 1)
        ctrl.synchronize()
        q1, dq1 = ctrl.pullState()
        ref = RS.forward_dynamics(m, q, dq, tau)
        qdd = (dq1 - dq) / dt
        assert np.abs(qdd - ref).max() / max(1.0, np.abs(ref).max()) < 1e-8


def test_tree_pose_and_reinit(sp):
    desc = TR.dual_panda_torso()
    m = W.RobotModel(desc)
    B = 63
    rng = np.random.default_rng(8)
    q, dq = _state(rng, m, B, 0.9)
    tasks = TR.dual_stack(m)
    robot, ctrl, objs = _ctrl(desc, tasks, B)
    goals = TR.tree_goals(rng, m, tasks, q)
    _cycle(robot, ctrl, q, dq, goals)
    fr = TR.tree_fk(m, q)
    for t, link in ((0, "left_link7"), (1, "right_link7")):
        R, o = fr[m.link_index(link)]
        x = o + R @ np.array([0.0, 0.0, 0.1])
        assert np.abs(objs[t].getCurrentPosition() - x).max() < 1e-12
        assert np.abs(objs[t].getCurrentOrientation() - R).max() < 1e-12
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    tau, st = ctrl.computeControlTorques().copy(), ctrl.status.copy()
    with TR.tree_oracle() as RS:
        g2 = []
        for t, link in ((0, "left_link7"), (1, "right_link7")):
            R, o = fr[m.link_index(link)]
            g2.append(np.concatenate([o + R @ np.array([0.0, 0.0, 0.1]), R.reshape(B, 9), np.zeros((B, 12))], axis=1))
        g2.append(np.concatenate([q, np.zeros((B, 2 * m.dof))], axis=1))
        ref, rst = RS.controller_step(m, tasks, q, dq, g2)
    ok = ((st & 1) == 0) & ((rst & 1) == 0)
    assert ok.sum() > B // 2
    assert W.torque_error(tau[ok], ref[ok]) < 1e-8
