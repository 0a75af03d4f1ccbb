"""Chains of 1 to 6 dof, and mid-chain fixed links, on every kernel family (robots and stacks: tests/chains.py; the oracle side of
every stack is pinned against the NumPy restatement in tests/test_small_chains_cpu.py):
  * n = 1..5: the automatic choice is the workgroup kernel saip_cycle_wg<8,64> (the lane, eight-lane and wavefront kernels need
    n >= 6); every stack against the oracle over three cycles at B = 1, 65, 1000 -- whole status words equal, torques of every
    instance the oracle does not refuse within 1e-5, blended (status 8) instances included;
  * n = 6, a PUMA-like arm with a third of its postures near the wrist singularity, a third near the elbow singularity: automatic,
    general, lane and eight-lane kernels (slow tail and list launch) against the oracle on every non-refused instance, and equal
    status words across kernels; blended strategies on, and singularity handling disabled;
  * model queries, dynamics and one integration step at n = 1, 2, 3, 4, 5, 6, 9, 32 and on a 7-dof chain with two massive fixed
    links mid-chain (the engine merges them into their parent body, the NumPy references treat every link as its own body);
  * task diagnostics on the planar 4R controller stack;
  * a motion-force task with more directions than the robot has dof is refused by the Python and C++ facades on a device."""
import subprocess

import numpy as np
import pytest

import chains as CH
import workloads as W

pytestmark = pytest.mark.gpu
TOL = 1e-5
WG = "saip_cycle_wg<8,64>"
SMALL = [(kind, n, s) for kind, ns in (("random", range(1, 6)), ("planar", range(2, 5))) for n in ns for s in sorted(CH.cycle_stacks(n, kind))]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _controller(desc, tasks, opts, B, kernel=0, on_list=False):
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(desc, tasks, B, device=0)
    ctrl.setKernel(kernel)
    ctrl.setFlaggedRecompute(on_list)
    ctrl.enableGravityCompensation(bool(opts.get("gravity_comp")))
    ctrl.enableTorqueSaturation(bool(opts.get("torque_saturation")))
    ctrl.enableJointLimitAvoidance(bool(opts.get("joint_limit_avoidance")))
    return robot, ctrl, objs


def _cycles(robot, ctrl, q, dq, goals, k=3):
    """k control cycles at q + 0.01 c: (tau (k, B, n), status (k, B), kernel names)"""
    taus, sts, names = [], [], set()
    ctrl.setGoals(goals)
    for c in range(k):
        robot.setQ(q + 0.01 * c)
        robot.setDq(dq)
        robot.updateModel()
        ctrl.updateControllerTaskModels()
        taus.append(ctrl.computeControlTorques().copy())
        sts.append(ctrl.status.copy())
        names.add(ctrl.kernelName())
    return np.array(taus), np.array(sts), names


def _oracle_cycles(model, tasks, opts, q, dq, goals, k=3):
    from oracle import Oracle
    orc = Oracle(model, tasks, **opts)
    out = [orc.step(q + 0.01 * c, dq, goals, nthreads=8) for c in range(k)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _compare(tag, tau, st, ref, rst):
    """whole status words equal; torques of every instance the oracle does not refuse within TOL; returns the worst error"""
    assert np.array_equal(st, rst), (tag, np.argwhere(st != rst)[:5], st[st != rst][:5], rst[st != rst][:5])
    worst = 0.0
    for c in range(tau.shape[0]):
        ok = (rst[c] & 1) == 0
        if ok.any():
            worst = max(worst, W.torque_error(tau[c][ok], ref[c][ok]))
    assert worst < TOL, (tag, worst)
    return worst


@pytest.mark.parametrize("B", [1, 65, 1000])
@pytest.mark.parametrize("kind,n,stack", SMALL, ids=[f"{k}{n}-{s}" for k, n, s in SMALL])
def test_small_chain_cycle_matches_oracle(sp, kind, n, stack, B):
    desc = CH.small_chain(n, kind)
    model = W.RobotModel(desc)
    tasks, opts = CH.cycle_stacks(n, kind)[stack]
    rng = np.random.default_rng(31 * n + B + len(stack))
    q = CH.postures(rng, model, kind, B)
    dq = rng.uniform(-0.5, 0.5, (B, n))
    goals = CH.goals(rng, model, tasks, q)
    robot, ctrl, _ = _controller(desc, tasks, opts, B)
    tau, st, names = _cycles(robot, ctrl, q, dq, goals)
    assert names == {WG}, names
    ref, rst = _oracle_cycles(model, tasks, opts, q, dq, goals)
    worst = _compare(f"{kind}{n}-{stack}-B{B}", tau, st, ref, rst)
    print(f"{kind} n={n} {stack} B={B}: {WG} worst torque err {worst:.2e}, statuses {sorted(set(rst.ravel().tolist()))}, "
          f"blended {int((rst & 8).astype(bool).sum())} of {rst.size}")


SIX = sorted(CH.cycle_stacks(6, "puma"))


@pytest.mark.parametrize("stack", SIX)
def test_puma_near_singular_postures_all_kernels(sp, stack):
    """kernels 0 (automatic), 1 (general), 2 (lane), 3 (eight-lane, slow tail and list launch) on the PUMA-like arm; the eight-lane kernel
    does not take a task whose singularity handling is disabled"""
    desc = CH.puma_arm()
    model = W.RobotModel(desc)
    tasks, opts = CH.cycle_stacks(6, "puma")[stack]
    B = 300
    rng = np.random.default_rng(66 + len(stack))
    q = CH.puma_postures(rng, B)
    dq = rng.uniform(-0.5, 0.5, (B, 6))
    goals = CH.goals(rng, model, tasks, q)
    ref, rst = _oracle_cycles(model, tasks, opts, q, dq, goals)
    handled = tasks[0].get("singularity_handling", True)
    assert (rst & (8 if handled else 2)).astype(bool).sum() > B // 3   # the postures do reach the handler's region
    runs = [(0, False), (1, False), (2, False), (2, True)] + ([(3, False), (3, True)] if handled else [])
    first = None
    for kernel, on_list in runs:
        robot, ctrl, _ = _controller(desc, tasks, opts, B, kernel, on_list)
        tau, st, names = _cycles(robot, ctrl, q, dq, goals)
        worst = _compare(f"puma {stack} kernel {kernel}{' list' if on_list else ''}", tau, st, ref, rst)
        print(f"puma {stack} kernel {kernel}{' (list launch)' if on_list else ''} {sorted(names)}: worst torque err {worst:.2e}, "
              f"statuses {sorted(set(rst.ravel().tolist()))}")
        if kernel == 3:
            assert names == {"saip_cycle_oct"}, names
        if kernel == 2:
            assert names == {"saip_cycle_lane"}, names
        if first is None:
            first = st
        assert np.array_equal(st, first)


# ---------------------------------------------------------------- model queries, dynamics, integration
QROBOTS = [1, 2, 3, 4, 5, 6, 9, 32, "7fixed"]


def _query_robot(key):
    if key == "7fixed":
        rng = np.random.default_rng(77)
        return CH.random_chain(rng, 7, "chain7_fixed", fixed_after=(2, 5), fixed_tip=True)
    return CH.small_chain(key, "random")   # n >= 2: a massive fixed link after link1 and one at the tip


def _frame_list(desc):
    m = W.RobotModel(desc)
    n = m.dof
    fixed = [l["name"] for l in desc["links"] if l["joint_type"] == "fixed"]
    base = [(f"link{n}", (0.0, 0.02, 0.1)), ("link1", None), (fixed[0], (0.03, -0.01, 0.05)), (fixed[-1], None),
            (f"link{max(1, n // 2)}", (0.1, 0.0, -0.02)), (fixed[0], None), (f"link{n}", None), ("link1", (0.0, 0.2, 0.0))]
    assert len(base) == 8
    return base


def _state(m, B, seed):
    rng = np.random.default_rng(seed)
    q = rng.uniform(np.maximum(m.q_lower, -2.5), np.minimum(m.q_upper, 2.5), size=(B, m.dof))
    return q, rng.uniform(-1.0, 1.0, size=(B, m.dof))


def _close(a, b, tol):
    scale = max(1.0, float(np.max(np.abs(b))))
    err = float(np.max(np.abs(a - b))) / scale
    return err <= tol, err


@pytest.mark.parametrize("B", [1, 65])
@pytest.mark.parametrize("key", QROBOTS, ids=[str(k) for k in QROBOTS])
def test_model_frames_small_and_fixed_link_chains(sp, key, B):
    desc = _query_robot(key)
    m = W.RobotModel(desc)
    n = m.dof
    q, dq = _state(m, B, 5 + n)
    robot = sp.SaiModel(desc, B, device=0)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    frames = W.fk(m, q)
    fr = _frame_list(desc)
    assert len(fr) == sp.SAIP_MAX_QUERY_FRAMES
    worst = 0.0
    for flags in (sp.SAIP_QUERY_JACOBIAN, 0, sp.SAIP_QUERY_JACOBIAN | sp.SAIP_QUERY_WORLD):
        out = robot._frames(fr, flags)
        assert out.shape == (len(fr), 18 + (6 * n if flags & sp.SAIP_QUERY_JACOBIAN else 0), B)
        for k, (link, pos) in enumerate(fr):
            li = m.link_index(link)
            R, o = frames[li]
            p = o + R @ (np.zeros(3) if pos is None else np.asarray(pos, float))
            J = W.jacobian(m, frames, li, p)
            r = out[k]
            checks = [(r[0:3].T, p, "position"), (r[3:12].T.reshape(B, 3, 3), R, "rotation"),
                      (np.concatenate([r[12:15].T, r[15:18].T], 1), np.einsum("bij,bj->bi", J, dq), "twist")]
            if flags & sp.SAIP_QUERY_JACOBIAN:
                checks.append((r[18:].T.reshape(B, 6, n), J, "jacobian"))
            for got, want, what in checks:   # the base is the identity: world rows equal base rows
                ok, err = _close(got, want, 1e-12)
                worst = max(worst, err)
                assert ok, (key, B, flags, link, what, err)
    print(f"frames n={n} ({key}) B={B}: worst err {worst:.2e}")


DYN = [(k, B) for k in QROBOTS for B in (1, 65)] + [(9, 200), (32, 200)]   # B = 200: the <32> dynamics query on several workgroups


@pytest.mark.parametrize("key,B", DYN, ids=[f"{k}-B{B}" for k, B in DYN])
def test_dynamics_and_integration_small_and_fixed_link_chains(sp, key, B):
    import restatement as RS
    from sai_primitives_amd.controller import controller_from_specs
    desc = _query_robot(key)
    m = W.RobotModel(desc)
    n = m.dof
    q, dq = _state(m, B, 11 + n)
    robot, ctrl, _ = controller_from_specs(desc, [W.joint_task("posture")], B, device=0)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    frames = W.fk(m, q)
    M, Minv, g, b = robot.M(), robot.MInv(), robot.jointGravityVector(), robot.coriolisForce()
    assert M.shape == Minv.shape == (B, n, n) and g.shape == b.shape == (B, n)   # (at n = 1 the vectors have as many rows as M)
    Mref = W.mass_matrix(m, frames)
    errs = {}
    for what, (ok, err) in [("M", _close(M, Mref, 1e-12)),
                            ("M Minv", _close(np.einsum("bij,bjk->bik", M, Minv), np.broadcast_to(np.eye(n), M.shape), 1e-10)),
                            ("g", _close(g, RS.gravity_vector(m, frames), 1e-12))]:
        errs[what] = err
        assert ok, (key, B, what, err)
    qdd0 = RS.forward_dynamics(m, q, dq, np.zeros_like(q), g=(0.0, 0.0, 0.0))
    ok, errs["b"] = _close(b, -np.einsum("bij,bj->bi", Mref, qdd0), 1e-7)
    assert ok, (key, B, "b", errs["b"])
    tau = np.random.default_rng(5).uniform(-20, 20, size=q.shape)
    ok, errs["fd"] = _close(np.einsum("bij,bj->bi", Minv, tau - b - g), RS.forward_dynamics(m, q, dq, tau), 1e-7)
    assert ok, (key, B, "forward dynamics", errs["fd"])
    dyn = ctrl.getModelDynamics()
    assert np.array_equal(dyn["M"], M) and np.array_equal(dyn["g"], g) and np.array_equal(dyn["b"], b)
    # one semi-implicit Euler step (the integrate kernel) against the Lagrangian forward dynamics
    dt = 1e-4
    tau = np.random.default_rng(4).uniform(-5, 5, (B, n))
    ctrl.setTorques(tau)
    for grav, damping in [((0.0, 0.0, -9.81), 0.0), ((0.0, 0.0, 0.0), 0.3)]:
        robot.setQ(q)
        robot.setDq(dq)
        robot.updateModel()
        ctrl.integrate(dt, 1, gravity=grav, damping=damping)
        ctrl.synchronize()
        q1, dq1 = ctrl.pullState()
        ref = RS.forward_dynamics(m, q, dq, tau, g=grav, damping=damping)
        err = np.abs((dq1 - dq) / dt - ref).max() / max(1.0, np.abs(ref).max())
        errs[f"qdd {'gravity' if damping == 0 else 'damped'}"] = err
        assert err < 1e-8, (key, B, grav, err)
        assert np.abs(q1 - (q + dt * dq1)).max() < 1e-15
    print(f"dynamics n={n} ({key}) B={B}: " + ", ".join(f"{k} {v:.1e}" for k, v in errs.items()))


def test_planar4_task_diagnostics(sp):
    """the diagnostics rows of the planar 4R controller's motion-force task (x, y, rotation about z at 0.5 m along link4) against the
    NumPy expectation of test_gpu_task_diagnostics; F_um on every instance outside the blending region"""
    from test_gpu_task_diagnostics import _diag, _expected, _close as _dclose
    from sai_primitives_amd.controller import controller_from_specs
    from oracle import Oracle
    desc = CH.planar_arm(4)
    model = W.RobotModel(desc)
    tasks, _ = CH.cycle_stacks(4, "planar")["planar4_controller"]
    B = 65
    rng = np.random.default_rng(44)
    q = CH.postures(rng, model, "planar", B)
    dq = rng.uniform(-0.5, 0.5, (B, 4))
    goals = CH.goals(rng, model, tasks, q)
    robot, ctrl, objs = controller_from_specs(desc, tasks, B, device=0)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.setGoals(goals)
    got = _diag(objs[0])
    exp = _expected(dict(model=model, tasks=tasks, q=q, dq=dq, goals=goals), 0, 1)
    _, st = Oracle(model, tasks).step(q, dq, goals)
    regular = st == 0
    assert regular.sum() > B // 2
    assert _dclose(got[:, :18], exp[:, :18]), np.abs(got[:, :18] - exp[:, :18]).max()
    assert _dclose(got[regular, 18:], exp[regular, 18:]), np.abs(got[regular, 18:] - exp[regular, 18:]).max()
    assert np.all(got[:, 2] == 0) and np.all(got[:, 3:5] == 0)   # z position and x / y rotation are not controlled
    print(f"planar 4R diagnostics: worst err {np.abs(got[:, :18] - exp[:, :18]).max():.2e}, F_um on {int(regular.sum())} of {B}")


def test_more_directions_than_dof_refused_on_device(sp, tmp_path):
    from sai_primitives_amd.controller import controller_from_specs, tasks_from_specs
    from test_small_chains_cpu import build_facade
    desc = CH.planar_arm(4)
    full = W.motion_force_task("full", "link4", (0.5, 0.0, 0.0))
    with pytest.raises(sp.SaipUnsupported, match="controls 6 directions but the robot has only 4 dof"):
        controller_from_specs(desc, [full, W.joint_task("posture")], 8, device=0)
    robot = sp.SaiModel(desc, 8, device=0)
    robot.setQ(np.zeros((8, 4)))
    robot.setDq(np.zeros((8, 4)))
    robot.updateModel()
    with pytest.raises(sp.SaipUnsupported, match="use a partial task"):
        tasks_from_specs(robot, [full])[0].updateTaskModel(np.eye(4))
    exe, rfile = build_facade(tmp_path, desc)
    out = subprocess.run([exe, rfile, "kgtn", "0", "link4"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "FACADE_KGTN_OK" in out.stdout, out.stdout + out.stderr
