"""Launch words of the eight-lane kernels (CycleParams::lw, csrc/saip_device.h): the batch-uniform words of the model block and of the
motion-force task that saip_cycle_oct reads from its kernel arguments instead of the blocks.  The new risk is a word that disagrees
with its block or goes stale, so every case changes a word between steps and checks every step against the general kernel
(setKernel(1), which reads the blocks; same inputs, bench.py's cross-kernel bound 1e-7) and against the oracle (tests/test_gpu_oct.py's
1e-5, whole status words equal).

Shapes: B = 9 (two workgroups of the two-wavefront form, the second with one live instance and seven padding groups) and B = 4104 (the
first batch that takes the one-wavefront form); the lean stack (config 2's) and one FULL stack (config 9's: general control laws).

The C ABI has no setter that moves the control frame of a finalized batch (and this change exports none: tests/test_engine_units_cpu.py
pins the ABI), so the control-frame cases use what a process can do: controllers with different frames alive side by side, stepped
alternately -- a word kept per process instead of per batch shows there.  The other words change through their setters on one live
controller.  The oracle has no setters: a phase gets a fresh oracle with the phase's spec (the stacks here carry no integrator, and the
engine resets the handler states when the strategies are switched on, as a fresh SingularityHandler starts)."""
import numpy as np
import pytest

import chains as CH
import workloads as W

pytestmark = pytest.mark.gpu
TOL = 1e-5     # oracle: tests/test_gpu_oct.py
XTOL = 1e-7    # general kernel on the same inputs: bench.py's cross-kernel bound
OCT = "saip_cycle_oct"
SHAPES = [9, 4104]
ROT = np.array([[0.0, -1.0, 0.0], [0.6, 0.0, -0.8], [0.8, 0.0, 0.6]])  # a proper rotation that is no permutation


def _controller(desc, spec, B, kernel):
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(desc, spec, B, device=0)
    ctrl.setFlaggedTorquePolicy(True)  # an instance the engine refuses (status 1) shows as NaN, like in the oracle
    ctrl.setKernel(kernel)
    return robot, ctrl, objs


def _cycle(robot, ctrl, q, dq, goals):
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    ctrl.setGoals(goals)
    return ctrl.computeControlTorques().copy(), ctrl.status.copy(), ctrl.kernelName()


def _elbow(d, B, seed):
    """every second instance with the elbow nearly straight, as tests/test_gpu_singularity_strategies.py places them: inside the blending
    region of the full task, so that the handling words decide something"""
    q = d["q"].copy()
    q[::2, 3] = -0.07 - 0.25 * np.random.default_rng(seed).uniform(size=(B + 1) // 2)
    return q


def _check(tag, got, gen, ref):
    """got / gen: (tau, status, kernel) of the automatic choice and of the general kernel; ref: (tau, status) of the oracle"""
    tau, st, _ = got
    assert np.array_equal(st, ref[1]), (tag, "status vs oracle", np.flatnonzero(st != ref[1])[:8])
    assert np.array_equal(st, gen[1]), (tag, "status vs general kernel", np.flatnonzero(st != gen[1])[:8])
    ok = (st & 1) == 0
    assert ok.any() and np.isfinite(tau[ok]).all() and np.isnan(tau[~ok]).all(), tag
    xerr, err = W.torque_error(tau[ok], gen[0][ok]), W.torque_error(tau[ok], ref[0][ok])
    print(tag, "vs general kernel", xerr, "vs oracle", err, "flagged", int((~ok).sum()), "blended", int(((st & 8) > 0).sum()))
    assert xerr < XTOL, (tag, xerr)
    assert err < TOL, (tag, err)


def _phases(desc, model, phases, B, q, dq, goals, opts=None):
    """phases: [(name, oracle spec of the phase, setter(task objects) or None)], two cycles each, on ONE controller per kernel"""
    from oracle import Oracle
    opts = opts or {}
    runs = []
    for kernel in (0, 1):
        robot, ctrl, objs = _controller(desc, phases[0][1], B, kernel)
        ctrl.enableGravityCompensation(bool(opts.get("gravity_comp")))
        out = []
        for name, spec, setter in phases:
            if setter:
                setter(objs)
            out.append([_cycle(robot, ctrl, q + 1e-3 * c, dq, goals) for c in range(2)])
        runs.append(out)
    for p, (name, spec, _) in enumerate(phases):
        orc = Oracle(model, spec, **opts)
        for c in range(2):
            _check(f"B={B} {name} cycle {c}", runs[0][p][c], runs[1][p][c], orc.step(q + 1e-3 * c, dq, goals, nthreads=8))
    return runs[0]


def _with(spec, **kw):
    return [dict(t, **kw) if t["type"] == "motion_force" else t for t in spec]


@pytest.mark.parametrize("B", SHAPES)
def test_singularity_handling_off_then_on(B):
    """disableSingularityHandling() -> enableSingularityHandling() on a live controller: the handling word follows (the near-singular
    instances are reduced in the first phase and flagged in the second)"""
    d = W.make_inputs(2, B)
    q = _elbow(d, B, 3)
    base = _with(W.config_tasks(2), singularity_strategies=False)
    got = _phases(d["model"].name, d["model"], [("handling off", _with(base, singularity_handling=False), None),
                                                ("handling on", _with(base, singularity_handling=True), lambda o: o[0].enableSingularityHandling())],
                  B, q, d["dq"], d["goals"])
    assert got[1][0][2] == OCT
    assert not np.array_equal(got[0][0][1], got[1][0][1])  # the word decided something


@pytest.mark.parametrize("B", SHAPES)
def test_strategies_off_on_off_with_handler_state(B):
    """setSingularityStrategies off -> on (handler states allocated: the strategies word is set) -> off again (states still there: the word
    is cleared all the same)"""
    d = W.make_inputs(2, B)
    q = _elbow(d, B, 5)
    off, on = _with(W.config_tasks(2), singularity_strategies=False), _with(W.config_tasks(2), singularity_strategies=True)
    got = _phases(d["model"].name, d["model"], [("strategies off", off, None),
                                                ("strategies on", on, lambda o: o[0].setSingularityStrategies(True)),
                                                ("strategies off again", off, lambda o: o[0].setSingularityStrategies(False))],
                  B, q, d["dq"], d["goals"])
    for p in range(3):
        assert got[p][0][2] == OCT
    near = np.arange(B) % 2 == 0
    assert (got[0][0][1][near] == 1).sum() > near.sum() // 2 and (got[1][0][1][near] == 8).sum() > near.sum() // 2
    assert np.array_equal(got[0][0][1], got[2][0][1])


@pytest.mark.parametrize("B", SHAPES)
def test_full_stack_handling_off_then_on(B):
    """config 9's stack (general control laws: a FULL instantiation), its integral gains zeroed so that a fresh oracle per phase is the
    reference"""
    d = W.make_inputs(9, B)
    q = _elbow(d, B, 7)
    base = [dict(t, **{k: 0.0 for k in ("ki", "ki_pos", "ki_ori") if k in t}) for t in W.config_tasks(9)]
    _phases(d["model"].name, d["model"], [("cfg9 handling off", _with(base, singularity_handling=False), None),
                                          ("cfg9 handling on", _with(base, singularity_handling=True), lambda o: o[0].enableSingularityHandling())],
            B, q, d["dq"], d["goals"])


def _frame_specs(tip, other):
    """the headline stack on two control frames: the usual one, and another body with a new point and a new rotation"""
    a = [W.motion_force_task("motion_force_task", tip, (0, 0, 0.07)), W.joint_task("joint_task")]
    # (bounds of the singular region below the defaults: on this frame they leave 6 of 7 postures on the ordinary path, the rest blended)
    b = [W.motion_force_task("motion_force_task", other, (0.04, -0.03, 0.06), rot_in_link=ROT, s_min=1e-3, s_max=1e-2), W.joint_task("joint_task")]
    return a, b


def _side_by_side(desc, model, specs, B, q, dq):
    """one controller per spec and kernel, all alive at once, stepped alternately for two rounds"""
    from oracle import Oracle
    rng = np.random.default_rng(11)
    goals = [CH.goals(rng, model, s, q) for s in specs]
    ctl = [[_controller(desc, s, B, kernel) for kernel in (0, 1)] for s in specs]
    orc = [Oracle(model, s) for s in specs]  # (kept over the rounds: blended instances carry handler state)
    taus = []
    for rnd in range(2):
        for i, s in enumerate(specs):
            got, gen = [_cycle(r, c, q + 1e-3 * rnd, dq, goals[i]) for r, c, _ in ctl[i]]
            _check(f"B={B} frame {i} round {rnd}", got, gen, orc[i].step(q + 1e-3 * rnd, dq, goals[i], nthreads=8))
            assert got[2] == OCT
            taus.append(got[0])
    both = np.isfinite(taus[0]).all(axis=1) & np.isfinite(taus[1]).all(axis=1)
    assert W.torque_error(taus[0][both], taus[1][both]) > 1e-3  # the frames really differ


@pytest.mark.parametrize("B", SHAPES)
def test_control_frame_on_another_body_with_new_point_and_rotation(B):
    d = W.make_inputs(2, B)
    _side_by_side(d["model"].name, d["model"], _frame_specs("end-effector", "link6"), B, d["q"], d["dq"])


@pytest.mark.parametrize("B", SHAPES)
def test_chain_whose_axes_are_not_all_z_next_to_the_panda(B):
    """all_axis_z is a word of the model: a 7-dof chain with general joint axes and the Panda (all z), same controller type, alive side
    by side and stepped alternately"""
    from oracle import Oracle
    desc = CH.random_chain(np.random.default_rng(1007), 7, "chain7_general_axes", prismatic_share=0.0)
    cm = W.RobotModel(desc)
    assert any(l["axis"] != [0.0, 0.0, 1.0] for l in desc["links"])
    rng = np.random.default_rng(13)
    cq = CH.postures(rng, cm, "random", B)
    cdq = rng.uniform(-0.5, 0.5, (B, 7))
    cspec = [W.motion_force_task("motion_force_task", "link7", (0.0, 0.02, 0.1), s_min=1e-3, s_max=1e-2), W.joint_task("joint_task")]  # (7 of 8 postures ordinary)
    cgoals = CH.goals(rng, cm, cspec, cq)
    d = W.make_inputs(2, B)
    sides = [(desc, cm, cspec, cq, cdq, cgoals), (d["model"].name, d["model"], d["tasks"], d["q"], d["dq"], d["goals"])]
    ctl = [[_controller(s[0], s[2], B, kernel) for kernel in (0, 1)] for s in sides]
    orc = [Oracle(s[1], s[2]) for s in sides]  # (kept over the rounds: blended instances carry handler state)
    for rnd in range(2):
        for i, (_, model, spec, q, dq, goals) in enumerate(sides):
            got, gen = [_cycle(r, c, q + 1e-3 * rnd, dq, goals) for r, c, _ in ctl[i]]
            _check(f"B={B} {'chain' if i == 0 else 'panda'} round {rnd}", got, gen, orc[i].step(q + 1e-3 * rnd, dq, goals, nthreads=8))
            assert got[2] == OCT


def test_multi_launcher_two_batches_with_different_control_frames():
    """the path of `bench.py --launcher multi` (saip_multi_*: batches that the multi-device layer owns and steps): two of them in one
    process with different control frames give different, each correct, torques -- the words are per batch, not static"""
    from oracle import Oracle
    from sai_primitives_amd import sharding
    B = 9
    d = W.make_inputs(2, B)
    model = d["model"]
    specs = _frame_specs("end-effector", "link6")
    rng = np.random.default_rng(17)
    goals = [CH.goals(rng, model, s, d["q"]) for s in specs]
    mcs = [sharding.MultiController(model.name, s, B, [0]) for s in specs]
    try:
        for mc, g in zip(mcs, goals):
            mc.robots[0].setQ(d["q"])
            mc.robots[0].setDq(d["dq"])
            mc.robots[0].updateModel()
            mc.controllers[0].setGoals(g)
        taus = []
        orc = [Oracle(model, s) for s in specs]
        for rnd in range(2):
            for mc in mcs:
                mc.step_async()
            for mc in mcs:
                mc.synchronize()
            taus = [mc.controllers[0].getTorques().copy() for mc in mcs]
            for i, s in enumerate(specs):
                ref, st = orc[i].step(d["q"], d["dq"], goals[i], nthreads=4)
                assert mcs[i].controllers[0].kernelName() == OCT and np.array_equal(mcs[i].controllers[0].status, st)
                ok = (st & 1) == 0
                err = W.torque_error(taus[i][ok], ref[ok])
                print("multi batch", i, "round", rnd, "err", err, "flagged", int((~ok).sum()))
                assert ok.sum() > B // 2 and err < TOL
        assert W.torque_error(taus[0], taus[1]) > 1e-3
    finally:
        for mc in mcs:
            mc.close()
