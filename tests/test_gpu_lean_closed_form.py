"""Lean eight-lane cycle kernel, closed-form torques of the headline stack (no J M^-1 J^T on the ordinary path): against the CPU oracle,
against the general kernel, and independence of an ordinary instance from the instances that share its wavefront."""
import itertools

import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu
TOL = 1e-5      # against the oracle (tests/test_gpu_oct.py)
XTOL = 1e-7     # against the general kernel: the benchmark's cross-kernel bound
OCT, GENERAL = 3, 1
DECS = (W.FULL_DYNAMIC_DECOUPLING, W.BOUNDED_INERTIA_ESTIMATES, W.IMPEDANCE)


def _engine(model_name, tasks, B, kernel):
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(model_name, tasks, B, device=0)
    ctrl.setFlaggedTorquePolicy(True)
    ctrl.setKernel(kernel)
    return robot, ctrl, objs


def _cycle(robot, ctrl, q, dq, goals):
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    ctrl.setGoals(goals)
    return np.array(ctrl.computeControlTorques())


def _both_kernels(model, tasks, q, dq, goals):
    B = q.shape[0]
    robot, ctrl, _ = _engine(model.name, tasks, B, OCT)
    tau = _cycle(robot, ctrl, q, dq, goals)
    assert ctrl.kernelName() == "saip_cycle_oct"
    st = np.array(ctrl.status)
    robot_g, ctrl_g, _ = _engine(model.name, tasks, B, GENERAL)
    tau_g = _cycle(robot_g, ctrl_g, q, dq, goals)
    assert ctrl_g.kernelName() != "saip_cycle_oct"
    return tau, st, tau_g, np.array(ctrl_g.status)


@pytest.mark.parametrize("B", [8, 9, 4104])
def test_batch_sizes(B):
    """one full group; one group with a single live instance; the first size that runs one wavefront per group on 256 CUs"""
    from oracle import Oracle
    d = W.make_inputs(2, B)
    ref, st_ref = Oracle(d["model"], d["tasks"]).step(d["q"], d["dq"], d["goals"], nthreads=8)
    tau, st, tau_g, st_g = _both_kernels(d["model"], d["tasks"], d["q"], d["dq"], d["goals"])
    assert np.array_equal(st, st_ref) and np.array_equal(st_g, st_ref) and not st_ref.any()
    err, xerr = W.torque_error(tau, ref), W.torque_error(tau, tau_g)
    print("closed form B", B, "vs oracle", err, "vs general kernel", xerr)
    assert err < TOL
    assert xerr < XTOL


@pytest.mark.parametrize("thr", [0.0, 0.1, 1.0])
@pytest.mark.parametrize("mf_dec,jt_dec", list(itertools.product(DECS, DECS)))
def test_decoupling_combinations(mf_dec, jt_dec, thr):
    """0, 1 and several clamped diagonal entries of M on the Panda, every pair of decoupling types"""
    from oracle import Oracle
    B = 64
    d = W.make_inputs(2, B)
    tasks = W.config_tasks(2)
    tasks[0].update(decoupling=mf_dec, bie_threshold=thr)
    tasks[1].update(decoupling=jt_dec, bie_threshold=thr)
    ref, st_ref = Oracle(d["model"], tasks).step(d["q"], d["dq"], d["goals"], nthreads=8)
    tau, st, tau_g, st_g = _both_kernels(d["model"], tasks, d["q"], d["dq"], d["goals"])
    assert np.array_equal(st, st_ref) and np.array_equal(st_g, st_ref) and not st_ref.any()
    err, xerr = W.torque_error(tau, ref), W.torque_error(tau, tau_g)
    print("closed form decoupling", mf_dec, jt_dec, "threshold", thr, "vs oracle", err, "vs general kernel", xerr)
    assert err < TOL
    assert xerr < XTOL


def test_ordinary_instances_do_not_depend_on_their_neighbours():
    """config 14's stream mixes ordinary instances and instances inside the blended singularity strategies; an ordinary instance gets
    the same bits wherever it sits in its wavefront and whoever sits next to it"""
    from oracle import Oracle
    B = 24
    d = W.make_inputs(14, 256)
    q, dq, goals = d["q"][:B], d["dq"][:B], [g[:B] for g in d["goals"]]
    ref, st_ref = Oracle(d["model"], d["tasks"]).step(q, dq, goals, nthreads=8)
    assert "".join("B" if s == 8 else "." if s == 0 else "?" for s in st_ref) == "B..BB.B..BB.BB.B..BB.B.."
    robot, ctrl, _ = _engine(d["model"].name, d["tasks"], B, OCT)
    tau = _cycle(robot, ctrl, q, dq, goals)
    assert ctrl.kernelName() == "saip_cycle_oct"
    st = np.array(ctrl.status)
    rev = slice(None, None, -1)
    robot_r, ctrl_r, _ = _engine(d["model"].name, d["tasks"], B, OCT)
    tau_r = _cycle(robot_r, ctrl_r, q[rev].copy(), dq[rev].copy(), [g[rev].copy() for g in goals])[rev]
    st_r = np.array(ctrl_r.status)[rev]
    assert np.array_equal(st, st_ref) and np.array_equal(st_r, st_ref)
    plain, blended = st_ref == 0, st_ref == 8
    assert np.array_equal(tau[plain], tau_r[plain])
    berr = W.torque_error(tau[blended], tau_r[blended])
    err, err_r = W.torque_error(tau, ref), W.torque_error(tau_r, ref)
    print("stream order vs reversed: blended", berr, "vs oracle", err, err_r)
    assert berr < 1e-9
    assert err < TOL and err_r < TOL


def test_integrators_track_every_cycle():
    """the commit path sees what the control laws advanced: three cycles with every-cycle accumulation on, against the oracle's own state"""
    from oracle import Oracle
    B = 16
    d = W.make_inputs(2, B)
    tasks = W.config_tasks(2)
    tasks[0].update(ki_pos=5.0, ki_ori=7.0)
    tasks[1].update(ki=3.0)
    orc = Oracle(d["model"], tasks)
    robot, ctrl, _ = _engine(d["model"].name, tasks, B, OCT)
    ctrl.setIntegratorTracking(True)
    rng = np.random.default_rng(5)
    q = d["q"].copy()
    for c in range(3):
        tau = _cycle(robot, ctrl, q, d["dq"], d["goals"])
        assert ctrl.kernelName() == "saip_cycle_oct"
        ref, st_ref = orc.step(q, d["dq"], d["goals"], nthreads=4)
        assert np.array_equal(np.array(ctrl.status), st_ref) and not st_ref.any()
        err = W.torque_error(tau, ref)
        print("closed form integrators cycle", c, "err", err)
        assert err < TOL
        q = q + 1e-3 * rng.standard_normal(q.shape)
