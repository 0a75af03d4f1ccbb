"""Resident forward dynamics + semi-implicit Euler (the step after the path; csrc/saip_dynamics.hip).
The reference delegates this step to the external sai-simulation (examples/05-...cpp:225-231), so there is no reference arithmetic:
the oracle is the Lagrangian restatement oracle/restatement.forward_dynamics (finite-difference Christoffel terms, no recursion in common
with the kernel's Newton-Euler pass), plus energy conservation and the closed-loop behaviour of the reference's example 05."""
import numpy as np
import pytest

import workloads as W
import restatement as RS  # oracle/restatement.py: the NumPy restatement of the reference path (test infrastructure)

pytestmark = pytest.mark.gpu


def _engine(robot_name, tasks, B, **kw):
    from sai_primitives_amd.controller import controller_from_specs
    return controller_from_specs(robot_name, tasks, B, device=0, **kw)


@pytest.mark.parametrize("robot_name,cfg", [("panda_arm", 2), ("panda_sliding_base", 6), ("chain30", 5)])
def test_one_step_matches_lagrangian_oracle(robot_name, cfg):
    B = 48
    d = W.make_inputs(cfg, B)
    model = d["model"]
    n = model.dof
    rng = np.random.default_rng(4)
    robot, ctrl, tasks = _engine(model.name, d["tasks"], B)
    tau = rng.uniform(-5, 5, (B, n))
    ctrl.setTorques(tau)
    dq = rng.uniform(-1.0, 1.0, (B, n))
    robot.setQ(d["q"])
    robot.setDq(dq)
    robot.updateModel()
    dt = 1e-4
    for grav, damping in [((0.0, 0.0, -9.81), 0.0), ((0.0, 0.0, 0.0), 0.3)]:
        robot.setQ(d["q"])
        robot.setDq(dq)
        robot.updateModel()
        ctrl.integrate(dt, 1, gravity=grav, damping=damping)
        ctrl.synchronize()
        q1, dq1 = ctrl.pullState()
        qdd = (dq1 - dq) / dt
        ref = RS.forward_dynamics(model, d["q"], dq, tau, g=grav, damping=damping)
        err = np.abs(qdd - ref).max() / max(1.0, np.abs(ref).max())
        print(robot_name, "gravity", grav, "max rel qdd error", err)
        assert err < 1e-8
        assert np.abs(q1 - (d["q"] + dt * dq1)).max() < 1e-15   # semi-implicit: positions advance with the NEW velocities


def test_energy_is_conserved_without_torques():
    B = 32
    d = W.make_inputs(2, B)
    model = d["model"]
    robot, ctrl, _ = _engine(model.name, d["tasks"], B)
    ctrl.setTorques(np.zeros((B, 7)))
    dq = np.random.default_rng(1).uniform(-0.5, 0.5, (B, 7))
    robot.setQ(d["q"])
    robot.setDq(dq)
    robot.updateModel()
    E0 = RS.total_energy(model, d["q"], dq)
    ctrl.integrate(2e-5, 5000)      # 0.1 s of free motion under gravity
    ctrl.synchronize()
    q1, dq1 = ctrl.pullState()
    E1 = RS.total_energy(model, q1, dq1)
    drift = np.abs(E1 - E0).max()
    moved = np.abs(q1 - d["q"]).max()
    print("energy drift", drift, "J over 0.1 s; max joint motion", moved, "rad; E0 range", E0.min(), E0.max())
    assert moved > 0.02 and drift < 2e-3    # first-order symplectic scheme: bounded O(dt) energy error


def test_on_device_closed_loop_rollout_tracks_otg_trajectory():
    """examples/05 scenario, entirely on the device: internal OTGs -> control cycle -> dynamics, 1 kHz control / 2 kHz simulation
    (examples/05-...cpp:216-231), gravity-free world (world.urdf:3).  The end effector must follow the Cartesian OTG to its goal."""
    B = 64
    d = W.make_inputs(2, B)
    model = d["model"]
    robot, ctrl, tasks = _engine(model.name, d["tasks"], B, disable_otg=False)
    robot.setQ(d["q"])
    robot.setDq(np.zeros((B, 7)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    mf, jt = tasks
    x0 = mf.getGoalPosition()
    goal = x0 + np.array([0.05, -0.04, 0.03])
    mf.setGoalPosition(goal)
    ctrl.updateControllerTaskModels()
    ctrl.rolloutAsync(100, 5e-4, 2, gravity=(0.0, 0.0, 0.0))
    ctrl.synchronize()
    qm, _ = ctrl.pullState()
    frm = W.fk(model, qm)
    lim = model.link_index("end-effector")
    xm = frm[lim][1] + frm[lim][0] @ np.array([0.0, 0.0, 0.07])
    des = mf.getDesiredPosition()
    # after 0.1 s the end effector follows the OTG's acceleration-limited profile (<= 1/2 * 2 m/s^2 * (0.1 s)^2 = 1 cm per axis), not the raw goal
    assert np.abs(des - x0).max() <= 0.0101 and np.abs(xm - des).max() < 2e-3 and np.abs(xm - goal).max() > 0.02
    ctrl.updateControllerTaskModels()
    ctrl.rolloutAsync(1400, 5e-4, 2, gravity=(0.0, 0.0, 0.0))
    ctrl.synchronize()
    q1, dq1 = ctrl.pullState()
    fr = W.fk(model, q1)
    li = model.link_index("end-effector")
    x1 = fr[li][1] + fr[li][0] @ np.array([0.0, 0.0, 0.07])
    gr, fl, res = mf.getInternalOtgStatus()
    err = np.linalg.norm(x1 - goal, axis=1)
    print("rollout: OTG goal reached", int(gr.sum()), "of", B, "| max end-effector error", err.max(), "| max |dq|", np.abs(dq1).max())
    assert ctrl.getTorques() is not None and ctrl.status.sum() == 0
    assert gr.all()
    assert err.max() < 2e-3 and np.abs(dq1).max() < 0.05
    assert np.linalg.norm(x0 - goal, axis=1).min() > 0.06


def test_eight_lane_dynamics_substeps_ragged_batch_and_coasting():
    """saip_integrate_oct (7-dof chains): a batch that is not a multiple of the eight instances per wavefront, three substeps with the
    torque held against the same scheme stepped with the Lagrangian oracle, NaN torques coast as zero torque, one instance with a
    non-finite state does not disturb the instances that share its wavefront"""
    B = 1001
    d = W.make_inputs(2, B)
    model = d["model"]
    rng = np.random.default_rng(12)
    robot, ctrl, _ = _engine(model.name, d["tasks"], B)
    tau = rng.uniform(-5, 5, (B, 7))
    tau[5] = np.nan
    dq = rng.uniform(-1.0, 1.0, (B, 7))
    dt, damping, grav = 2e-4, 0.2, (0.0, 0.0, -9.81)
    ctrl.setTorques(tau)
    robot.setQ(d["q"])
    robot.setDq(dq)
    robot.updateModel()
    ctrl.integrate(dt, 3, gravity=grav, damping=damping)
    ctrl.synchronize()
    q1, dq1 = ctrl.pullState()
    tz = np.where(np.isnan(tau), 0.0, tau)
    q_ref, dq_ref = d["q"].copy(), dq.copy()
    for _ in range(3):
        qdd = RS.forward_dynamics(model, q_ref, dq_ref, tz, g=grav, damping=damping)
        dq_ref = dq_ref + dt * qdd
        q_ref = q_ref + dt * dq_ref
    err = np.abs(dq1 - dq_ref).max() / np.abs(dq_ref - dq).max()
    print("three substeps, B = 1001: velocity increment error", err)
    assert err < 1e-8 and np.abs(q1 - q_ref).max() < 1e-9
    # isolation
    qb = d["q"].copy()
    qb[42, 2] = np.nan
    robot.setQ(qb)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.setTorques(tau)
    ctrl.integrate(dt, 3, gravity=grav, damping=damping)
    ctrl.synchronize()
    q2, dq2 = ctrl.pullState()
    others = np.arange(B) != 42
    assert np.array_equal(dq2[others], dq1[others]) and np.array_equal(q2[others], q1[others])
    assert not np.isfinite(dq2[42]).all()


@pytest.mark.parametrize("otg", [True, False], ids=["internal_otg", "no_otg"])
def test_rollout_with_fused_integrate_and_next_otg_equals_stepwise_loop(otg):
    """saip_batch_rollout_async puts the integration of period k and the internal OTG step of period k + 1 into one launch (they are
    independent: the OTGs evolve their own state); without internal OTGs the cycle launch of the eight-lane kernel integrates the state
    itself (one launch per period).  The same periods issued one call at a time (stepAsync + integrate: separate OTG, cycle and
    integrate launches) must give the same robot state, OTG state and torques."""
    B = 200
    d = W.make_inputs(2, B)
    out = []
    for fused in (True, False):
        robot, ctrl, tasks = _engine(d["model"].name, d["tasks"], B, disable_otg=not otg)
        robot.setQ(d["q"])
        robot.setDq(np.zeros((B, 7)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        mf, jt = tasks
        mf.setGoalPosition(mf.getGoalPosition() + np.array([0.04, -0.03, 0.05]))
        qg = d["q"].copy()
        qg[:, 0] += 0.3
        jt.setGoalPosition(qg)
        ctrl.updateControllerTaskModels()
        K = 37
        if fused:
            ctrl.rolloutAsync(K, 5e-4, 2, gravity=(0.0, 0.0, 0.0))
        else:
            for _ in range(K):
                ctrl.stepAsync()
                ctrl.integrate(5e-4, 2, gravity=(0.0, 0.0, 0.0))
        ctrl.synchronize()
        q, dq = ctrl.pullState()
        out.append((q.copy(), dq.copy(), ctrl.getTorques(), mf.getDesiredPosition(), jt.getDesiredPosition()))
        assert (ctrl.status & 1).sum() == 0
    for a, b in zip(*out):
        assert np.abs(a - b).max() <= 1e-11 * max(1.0, np.abs(b).max()), np.abs(a - b).max()
    assert np.abs(out[0][0] - d["q"]).max() > 1e-3     # the arm did move
