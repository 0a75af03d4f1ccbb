"""Forward dynamics and every integrator path against the exact oracle tests/dynamics_ref.py (complex-step Lagrangian in long double; it
earns its place in tests/test_dynamics_ref_cpu.py).  What is asserted is dynamics_ref.residual_check: the backward error of one
semi-implicit Euler step, in units of n eps of a scale made of absolute sums.  It does not depend on the conditioning of M, so its bound
is derived and not tuned:

    BOUND = 8     Cholesky and two triangular solves leave at most about (n + 1) eps |L||L^T||a|; the depth-n recursions that form M
                  and h each add a few n eps of their absolute sums; the oracle's own double solve sits below 1.

Single steps: dt = 2^-6 (one step needs no stability, and a large power of two keeps the error of recovering the acceleration from two
stored velocities near 1e-14), |dq| <= 3 rad/s, tau uniform in +-5, and the two settings g = (1.3, -2.1, -9.0) undamped and g = 0 with
damping 0.3.  Every case also requires, so that it cannot pass vacuously: |a| above 1 rad/s^2 somewhere in the batch, H below 1e3 |h| for
every instance, no flagged (non-finite) instance, and the position update q1 = q0 + dt dq1 to 1 ulp.

Every case prints its measured residual, instance and row; DESIGN.md ("The exact dynamics oracle") keeps the table."""
import copy

import numpy as np
import pytest

import chains as CH
import dynamics_ref as DR
import inertia_ref as IR
import trees as TR
import workloads as W

pytestmark = pytest.mark.gpu

BOUND = 8.0
DT = 2.0 ** -6
G_TILTED = (1.3, -2.1, -9.0)
SETTINGS = [(G_TILTED, 0.0), ((0.0, 0.0, 0.0), 0.3)]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def panda_with_a_branch():
    """the Panda as a real tree of 8 dof: its camera side frame off link4 (tests/trees.panda_with_side_frames, massive) made a revolute
    joint.  A chain merely written with parents keeps is_tree = 0 and runs the chain code, so the Panda needs a branch to reach the tree
    instantiation: link5 no longer hangs off the body listed before it."""
    d = TR.panda_with_side_frames(True)
    cam = d["links"][[l["name"] for l in d["links"]].index("camera")]
    cam.update(joint_type="revolute", axis=[0.0, 1.0, 0.0], q_lower=-2.5, q_upper=2.5)
    return dict(name="panda_camera_joint", links=d["links"])


def _desc(name):
    if name in ("panda_arm", "panda_sliding_base", "chain30"):
        m = W.load_robot(name)
        return dict(name=m.name, links=copy.deepcopy(m.links))
    if name.startswith("chain"):
        return CH.small_chain(int(name[5:]), "random")
    return {"puma6": CH.puma_arm, "panda_branch": panda_with_a_branch, "random11_4": lambda: TR.random_tree(11, 4),
            "dual_panda_torso": TR.dual_panda_torso}[name]()


def _is_tree(m):
    return TR.joint_parents(m) != list(range(-1, m.dof - 1))


def _engine(desc, B, specs=None, **kw):
    from sai_primitives_amd.controller import controller_from_specs
    return controller_from_specs(desc, specs or [W.joint_task("posture")], B, device=0, **kw)


def _state(m, B, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(np.maximum(m.q_lower, -2.5), np.minimum(m.q_upper, 2.5), (B, m.dof))
    return q, rng.uniform(-3.0, 3.0, (B, m.dof)), rng.uniform(-5.0, 5.0, (B, m.dof))


def _ulp_apart(a, b):
    return np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))


def _check_step(tag, md, q0, dq0, q1, dq1, tau, dt, grav, damping, bound=BOUND):
    """the conditions of the module docstring and the residual of one step; returns the residual"""
    assert np.isfinite(q1).all() and np.isfinite(dq1).all(), tag                              # no instance is flagged
    assert _ulp_apart(q1, q0 + dt * dq1).max() <= 1.0, (tag, _ulp_apart(q1, q0 + dt * dq1).max())
    det = {}
    val, b, i = DR.residual_check(md, q0, dq0, dq1, tau, dt, grav, damping, details=det)
    ratio = (det["H"].max(axis=1) / np.maximum(np.abs(det["h"]).max(axis=1), 1e-300)).max() if det["H"].any() else 0.0
    print(f"{tag}: gravity {grav}, damping {damping}: residual {val:.3g} n eps (instance {b}, row {i}); max |a| {np.abs(det['a']).max():.3g}, "
          f"worst H / |h| {ratio:.3g}")
    assert np.abs(det["a"]).max() > 1.0, tag
    assert (det["H"].max(axis=1) <= 1e3 * np.abs(det["h"]).max(axis=1)).all(), (tag, ratio)
    assert val <= bound, (tag, val, b, i)
    return val


def _one_step(robot, ctrl, q, dq, tau, grav, damping, substeps=1):
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.setTorques(tau)
    ctrl.integrate(DT, substeps, gravity=grav, damping=damping)
    ctrl.synchronize()
    q1, dq1 = ctrl.pullState()
    return q1.copy(), dq1.copy()


# name -> (batch size, the instantiation launch_integrate takes for it)
PATHS = {"chain1": (70, "lane chain <8>"), "chain4": (70, "lane chain <8>"), "puma6": (70, "lane chain <8>"), "panda_sliding_base": (70, "lane chain <8>"),
         "chain9": (70, "lane chain <32>"), "chain30": (8, "lane chain <32>"),
         "panda_branch": (70, "lane tree <8>"), "random11_4": (70, "lane tree <8>"), "dual_panda_torso": (70, "lane tree <32>"),
         "panda_arm": (9, "eight-lane")}


@pytest.mark.parametrize("name", sorted(PATHS))
def test_single_step_residual(sp, name):
    """launch_integrate: a chain of 7 dof takes the eight-lane step (panda_arm; B = 9: two groups of eight, the second with one live
    instance); every other chain the lane kernel, NMAX = 8 up to 8 dof (chain1, chain4, the 6-dof PUMA layout, the sliding-base Panda with
    its prismatic joint) and NMAX = 32 above (chain9, chain30); a tree the TREE instantiation whatever its dof, NMAX = 8 (the Panda with a
    branch, a random tree of 4 dof) or 32 (dual_panda_torso, 15 dof).  B = 70 is ld = 96: two blocks, the second ragged."""
    B, path = PATHS[name]
    desc = _desc(name)
    m = W.RobotModel(desc)
    assert _is_tree(m) == ("tree" in path) and (m.dof == 7) == (path == "eight-lane") and (m.dof <= 8) == ("<32>" not in path)
    md = DR.Model(m)
    q, dq, tau = _state(m, B, 40 + m.dof)
    robot, ctrl, _ = _engine(desc, B)
    for grav, damping in SETTINGS:
        q1, dq1 = _one_step(robot, ctrl, q, dq, tau, grav, damping)
        _check_step(f"{name} ({path}, B = {B})", md, q, dq, q1, dq1, tau, DT, grav, damping)


# ------------------------------------------------------------------ the INERTIA instantiations
def _parts(rng, n, B=None):
    """s in [0.8, 1.2], |d| <= 0.02, one payload of 0.5 .. 3 kg on the last link; (n, 4) and (1, 7), or (n, B, 4) and (1, B, 7)"""
    sb, spay = ((n,), (1,)) if B is None else ((n, B), (1, B))
    bodies = np.concatenate([rng.uniform(0.8, 1.2, sb + (1,)), rng.uniform(-0.02, 0.02, sb + (3,))], axis=-1)
    pay = np.concatenate([rng.uniform(0.5, 3.0, spay + (1,)), rng.uniform(-0.05, 0.05, spay + (3,)), rng.uniform(0.01, 0.08, spay + (3,))], axis=-1)
    return bodies, pay


INERTIA = [("panda_sliding_base", 8, "lane chain <8>"), ("panda_sliding_base", 70, "lane chain <8>"), ("random11_4", 8, "lane tree <8>"),
           ("random11_4", 70, "lane tree <8>"), ("panda_arm", 8, "eight-lane"), ("panda_arm", 9, "eight-lane")]


@pytest.mark.parametrize("name,B,path", INERTIA, ids=[f"{n}-B{B}" for n, B, _ in INERTIA])
def test_single_step_residual_with_an_inertia_table(sp, name, B, path):
    """an attached table selects the INERTIA instantiation of whichever kernel the model takes (launch_integrate: S.inertia): the lane chain
    kernel (sliding-base Panda), the lane tree kernel (random tree) and the eight-lane step (Panda).  A batch-uniform table (stride 1),
    a per-instance table with a payload on the last link -- the oracle with every instance's own link parameters,
    inertia_ref.instance_description -- and after the detach the model's robot again."""
    desc = _desc(name)
    m = W.RobotModel(desc)
    assert _is_tree(m) == ("tree" in path)
    parents = TR.parent_index(m) if _is_tree(m) else None
    site = [[l["name"] for l in desc["links"] if l["joint_type"] != "fixed"][-1] if name.startswith("random") else "end-effector"]
    rng = np.random.default_rng(50 + B)
    q, dq, tau = _state(m, B, 60 + m.dof + B)
    robot, ctrl, _ = _engine(desc, B)
    # batch-uniform
    bodies, pay = _parts(rng, m.dof)
    ctrl.attachInertia(payload_links=site)
    ctrl.setInertiaParts(bodies, pay)
    assert ctrl.inertiaRows().shape == (m.dof, 10)
    md = DR.Model(W.RobotModel(IR.instance_description(desc, bodies, pay, site, parents)))
    for grav, damping in SETTINGS:
        q1, dq1 = _one_step(robot, ctrl, q, dq, tau, grav, damping)
        _check_step(f"{name} ({path}, INERTIA batch-uniform, B = {B})", md, q, dq, q1, dq1, tau, DT, grav, damping)
    ctrl.detachInertia()
    # per instance
    bodies, pay = _parts(rng, m.dof, B)
    ctrl.attachInertia(per_instance=True, payload_links=site)
    ctrl.setInertiaParts(bodies, pay)
    md = DR.Model([W.RobotModel(IR.instance_description(desc, bodies[:, i], pay[:, i], site, parents)) for i in range(B)])
    for grav, damping in SETTINGS:
        q1, dq1 = _one_step(robot, ctrl, q, dq, tau, grav, damping)
        _check_step(f"{name} ({path}, INERTIA per instance, B = {B})", md, q, dq, q1, dq1, tau, DT, grav, damping)
    ctrl.detachInertia()
    # detached: the model's robot
    md = DR.Model(m)
    for grav, damping in SETTINGS:
        q1, dq1 = _one_step(robot, ctrl, q, dq, tau, grav, damping)
        _check_step(f"{name} ({path}, detached, B = {B})", md, q, dq, q1, dq1, tau, DT, grav, damping)


# ------------------------------------------------------------------ the fused forms
@pytest.mark.parametrize("otg", [False, True], ids=["cycle_fused", "integrate_otg_pair"])
def test_fused_forms_residual_of_every_period(sp, otg):
    """panda_arm with config 2's stack, B = 9, 3 periods of 2^-9 s, one substep, the recorder logging q | dq | tau every period.  Without
    internal OTGs the cycle launch of the eight-lane kernel integrates the state itself (saip_batch_rollout_async: sim handed to
    launch_cycle); with them the integration of a period that another follows shares its launch with the next period's OTG step
    (launch_integrate_otg_pair; the last period takes the plain eight-lane step).  Every transition: the state of sample k - 1 (the start
    state for k = 0) advances to the state of sample k under the logged torque of sample k."""
    B, K, dt = 9, 3, 2.0 ** -9
    d = W.make_inputs(2, B)
    m = d["model"]
    md = DR.Model(m)
    dq0 = np.random.default_rng(70).uniform(-1.0, 1.0, (B, 7))
    for grav, damping in SETTINGS:
        robot, ctrl, tasks = _engine(m.name, B, d["tasks"], disable_otg=not otg)
        robot.setQ(d["q"])
        robot.setDq(dq0)
        robot.updateModel()
        ctrl.reinitializeTasks()
        mf, jt = tasks
        mf.setGoalPosition(mf.getGoalPosition() + np.array([0.04, -0.03, 0.05]))
        qg = d["q"].copy()
        qg[:, 0] += 0.3
        jt.setGoalPosition(qg)
        ctrl.updateControllerTaskModels()
        ctrl.recordRollouts(K, 1, ("q", "dq", "tau"))
        ctrl.rolloutAsync(K, dt, 1, gravity=grav, damping=damping)
        ctrl.synchronize()
        log = ctrl.rolloutLog()
        assert log["q"].shape == (K, B, 7) and list(log["period"]) == [1, 2, 3]
        assert (log["status"] & 1).sum() == 0 and np.isfinite(log["tau"]).all()              # no instance is flagged
        qs, dqs = [d["q"]] + list(log["q"]), [dq0] + list(log["dq"])
        for k in range(K):
            _check_step(f"panda_arm rollout {'with' if otg else 'without'} internal OTG, period {k + 1}", md, qs[k], dqs[k], qs[k + 1], dqs[k + 1],
                        log["tau"][k], dt, grav, damping)
        ctrl.stopRecordingRollouts()


# ------------------------------------------------------------------ the substep loop
SUBSTEP_PATHS = ["panda_sliding_base", "chain9", "random11_4", "dual_panda_torso", "panda_arm"]


@pytest.mark.parametrize("name", SUBSTEP_PATHS)
def test_three_substeps_equal_three_calls_bit_for_bit(sp, name):
    """integrate(dt, 3) holds the torque and repeats the arithmetic of integrate(dt, 1), with the state in registers in place of memory:
    the same bits on each of the five paths (lane chain <8> and <32>, lane tree <8> and <32>, eight-lane).  This carries the single-step
    residual over to the substep loop."""
    B, path = PATHS[name]
    desc = _desc(name)
    m = W.RobotModel(desc)
    q, dq, tau = _state(m, B, 80 + m.dof)
    robot, ctrl, _ = _engine(desc, B)
    grav, damping = G_TILTED, 0.3
    qa, dqa = _one_step(robot, ctrl, q, dq, tau, grav, damping, substeps=3)
    qb, dqb = q, dq
    for _ in range(3):
        qb, dqb = _one_step(robot, ctrl, qb, dqb, tau, grav, damping)
    assert np.isfinite(qa).all() and np.isfinite(dqa).all() and np.abs(qa - q).max() > 1e-3
    diff = max(np.abs(qa - qb).max(), np.abs(dqa - dqb).max())
    print(f"{name} ({path}): integrate(dt, 3) against three integrate(dt, 1): max abs difference {diff:.3g}")
    assert qa.tobytes() == qb.tobytes() and dqa.tobytes() == dqb.tobytes(), (name, diff)


# ------------------------------------------------------------------ the model queries at the same precision
# Explained rounding, the one constant above 8 (and at the cap of 64 such a constant may have): coriolisForce() on puma6, measured 20.8 n eps H
# (rows 0 and 5).  rnea() works in world coordinates.  It forms every body's force from the total acceleration of its centre of mass and takes
# moments with levers that are differences of world positions, so (row 0, the vertical waist) the moments of the centripetal forces that lie in
# the arm's plane cancel as r_x f_y - r_y f_x at eps |r||f| where the Lagrangian sum has no summand at all, and (row 5, the last wrist joint,
# H = 5e-4) the lever c - o of 3 cm is the difference of two positions 1.5 m from the origin.  The same algorithm in NumPy gives 20.5 in double
# and 0.008 in long double at these inputs: the arithmetic is right, the excess is rounding.  Every other case and query stays at 8.
QUERY_BOUND = {("puma6", "coriolisForce"): 64.0}


@pytest.mark.parametrize("name", ["panda_sliding_base", "puma6", "panda_branch", "dual_panda_torso"])
def test_model_queries_to_the_rounding_of_their_sums(sp, name):
    """coriolisForce() against the velocity part of h (bias with g = 0), jointGravityVector() against dU/dq (bias at rest, model gravity),
    each to 8 n eps H per row, H the absolute sum of that part; M() against the long-double Jacobian form to 8 n eps of the sum of its
    summands with their factors replaced by their norms (dynamics_ref.mass_matrix).  Chains and trees: the queries share saip_rbd.h with
    the lane kernel.  puma6 is the case that found the composite inertias summed about the world origin: its last wrist joint, M_66 =
    1.5e-4 kg m^2 at 1.5 m from the base, was 3e2 n eps off (and the step residual 215); about the joint origins it is within the bound.
    Its coriolisForce() carries the one raised constant, QUERY_BOUND."""
    B = 70
    desc = _desc(name)
    m = W.RobotModel(desc)
    n = m.dof
    md = DR.Model(m)
    q, dq, _ = _state(m, B, 90 + n)
    robot = sp.SaiModel(desc, B, device=0)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    hv, Hv = DR.bias(md, q, dq, (0.0, 0.0, 0.0), np.clongdouble)
    hg, Hg = DR.bias(md, q, np.zeros_like(dq), (0.0, 0.0, -9.81), np.clongdouble)
    Ml, Mabs = DR.mass_matrix(md, q, np.longdouble, with_abs=True)
    unit = n * DR.EPS
    worst = {}
    for what, got, want, scale in (("coriolisForce", robot.coriolisForce(), hv, Hv), ("jointGravityVector", robot.jointGravityVector(), hg, Hg),
                                   ("M", robot.M(), Ml, Mabs)):
        err = np.abs(got - want).astype(float)
        scale = scale.astype(float)
        assert np.isfinite(got).all() and np.abs(want).max() > 0.1, what
        assert (err[scale == 0] == 0).all(), what                                             # an exact zero of the oracle is one of the device
        worst[what] = float((err[scale > 0] / (unit * scale[scale > 0])).max())
    print(f"{name}: " + ", ".join(f"{k} {v:.3g} n eps" for k, v in worst.items()))
    for what, v in worst.items():
        assert v <= QUERY_BOUND.get((name, what), 8.0), (name, what, v)
