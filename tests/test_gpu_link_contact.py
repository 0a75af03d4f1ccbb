"""Link contact on the device (csrc/saip_link_contact.hip, saip_batch_link_contact_*).  Oracles: the NumPy restatement
tests/link_contact_ref.py for the force stage (fed the kernel's own centres and velocities), the engine's model queries for centres,
velocities and Jacobians, the clearance monitor and the contact planes for two independent cross-checks, a batch without the attachment
for everything that must not change, the host-driven loop for rollouts.

Batches (B, ld) in {(3, 64), (65, 128), (130, 192)}: a partial group block, a block edge, several blocks, at a padded leading dimension.
The padding columns of every output are pre-filled with a sentinel that must survive.  Obstacles are placed from the restatement's own
forward kinematics so that between a quarter and three quarters of all items are active; every test with obstacles in reach asserts that
share (the two single-sphere tests, the drop and the comparison with the contact planes, assert instead that the one item is active in
part of the run and inactive in the rest).

The elbow test steps the Panda in NumPy (oracle/restatement.py: the joint controller and the forward dynamics; the restatement for the
contact torques), which takes a few seconds: it runs at B = 3 only."""
import ctypes as C

import numpy as np
import pytest

import chains as CH
import clearance_ref as CL
import contact_ref as CT
import link_contact_ref as LC
import plant_ref as PL
import trees as TR
import workloads as W
from test_gpu_batch_layout import _DevBuf, _d2h, _h2d, _same_bits
from test_gpu_clearance import _chain30w, _query_centres, _spheres
from test_gpu_guard import GUARDS, PHASES
from test_gpu_rollout_record import _panda

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64), (65, 128), (130, 192)]          # (B, leading dimension)
MODELS = ["panda_arm", "chain30w", "tree", "forest"]
SENTINEL = 6.02214076e23
EPS = 2.0 ** -52
DT, SUB = 5e-4, 2
GRAV = (0.0, 0.0, 0.0)
CENTRE_BOUND = 1e-12                               # the bound of tests/test_gpu_clearance.py on the same walk
FAR = np.array([[1, 0.0, 0.0, 1.0, -50.0, 0, 0, 0], [0, 40.0, 40.0, 40.0, 41.0, 40.0, 40.0, 0.5]])       # nothing of any robot is near these
FAR_MAT = np.array([[1e4, 10.0, 0.5, 1e-3], [1e4, 10.0, 0.0, 0.0]])


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


# ------------------------------------------------------------------ models, spheres, obstacles
def _slider1(mass):
    """one vertical prismatic joint carrying `mass`"""
    return dict(name="slider1", links=[CH._link("link1", "prismatic", [0, 0, 0], [0, 0, 0], [0, 0, 1], mass, [0, 0, 0], [0.01, 0.01, 0.01, 0, 0, 0], -5.0, 5.0, 1e3)])


def _case(name, B, ld, seed=3, dq_scale=0.5):
    """(robot, ctrl, task objects, the NumPy model, spheres) at a random moving state"""
    from sai_primitives_amd.controller import controller_from_specs
    rng = np.random.default_rng(seed)
    if name in ("tree", "forest"):
        desc = TR.dual_panda_torso() if name == "tree" else TR.dual_panda_fixed_torso()
        m = W.RobotModel(desc)
        specs = TR.dual_stack(m)
    elif name == "chain30w":
        desc = _chain30w()
        m, specs = W.RobotModel(desc), W.make_inputs(5, B)["tasks"]
    elif name == "slider1":
        desc = _slider1(2.0)
        m, specs = W.RobotModel(desc), [W.joint_task("posture")]
    else:
        d = W.make_inputs(2, B)
        desc, m, specs = d["model"].name, d["model"], d["tasks"]
    q = np.clip(rng.uniform(-1.2, 1.2, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    dq = dq_scale * rng.uniform(-1.0, 1.0, (B, m.dof))
    robot, ctrl, objs = controller_from_specs(desc, specs, B, device=0, leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    sph = [("link1", np.array([0.0, 0.01, 0.02]), 0.05)] if name == "slider1" else _spheres(name, rng)[0]
    return robot, ctrl, objs, m, sph


def _touching(rng, m, robot, sph, O, per):
    """O obstacles of mixed kinds (capsule, sphere, half-space in turn) and their materials, placed from the restatement's forward kinematics
    so that each is penetrated by 35 % .. 65 % of the (instance, sphere) pairs: (O, 8) or (O, B, 8), and (O, 4)"""
    c, _, _ = LC.sphere_state(m, robot._q, robot._dq, sph)
    B, S = c.shape[:2]
    flat, rs = c.reshape(-1, 3), np.tile([r for _, _, r in sph], B)
    ob = np.zeros((O, 8))
    for o in range(O):
        share = rng.uniform(0.35, 0.65)
        if o % 3 == 2:
            n = rng.normal(size=3)
            n /= np.linalg.norm(n)
            ob[o, 0], ob[o, 1:4], ob[o, 4] = 1, n, np.quantile(flat @ n - rs, share)
        else:
            a = flat[rng.integers(len(flat))] + rng.uniform(-0.05, 0.05, 3)
            b = a if o % 3 == 1 else a + rng.uniform(-0.3, 0.3, 3)
            d = CL.capsule_dist(np.broadcast_to(a, flat.shape), np.broadcast_to(b, flat.shape), 0.0, flat, rs)
            ob[o, 1:4], ob[o, 4:7], ob[o, 7] = a, b, max(0.0, np.quantile(d, share))
    mat = np.stack([rng.uniform(2e3, 3e4, O), rng.uniform(0.0, 100.0, O), rng.uniform(0.2, 0.9, O), 10.0 ** rng.uniform(-3, -0.5, O)], axis=1)
    mat[::4, 2], mat[::4, 3] = 0.0, 0.0                                  # every fourth obstacle is frictionless
    if per:                                                              # the same obstacles, shifted a little per instance
        ob = np.repeat(ob[:, None, :], B, axis=1)
        hs = ob[..., 0] == 1
        shift = rng.uniform(-0.01, 0.01, (O, B, 3))
        ob[..., 1:4] = np.where(hs[..., None], ob[..., 1:4], ob[..., 1:4] + shift)
        ob[..., 4:7] = np.where(hs[..., None], ob[..., 4:7], ob[..., 4:7] + shift)
        ob[..., 4] = np.where(hs, ob[..., 4] + shift[..., 0], ob[..., 4])
    return ob, mat


def _ref_obst(ob, per):
    return ob.transpose(1, 0, 2) if per else ob


def _share(ro, S, O):
    share = ro[:, 5].sum() / (ro.shape[0] * S * O)
    assert 0.25 <= share <= 0.75, share                                  # a condition of every test: something touches, not everything
    return share


class _Outputs:
    """the device outputs of an attachment with the padding columns pre-filled with a sentinel"""

    def __init__(self, ctrl, S, n, ld, keep):
        from sai_primitives_amd import capi
        L = capi.lib()
        ctrl.synchronize()
        self.ctrl, self.B, self.ld, self.S = ctrl, ctrl.batch_size, ld, S
        self.bufs = dict(readout=(L.saip_batch_link_contact_readout_device(ctrl._h), 8), summary=(L.saip_batch_link_contact_summary_device(ctrl._h), 4),
                         tau=(ctrl.linkContactTorquesDevice(), n))
        if keep:
            self.bufs["keep"] = (ctrl.linkContactKeepDevice(), 9 * S)
        for ptr, rows in self.bufs.values():
            assert ptr
            a = _d2h(ptr, (rows, ld))
            a[:, self.B:] = SENTINEL
            _h2d(ptr, a)

    def get(self, key):
        self.ctrl.synchronize()
        ptr, rows = self.bufs[key]
        a = _d2h(ptr, (rows, self.ld))
        assert (a[:, self.B:] == SENTINEL).all(), key          # columns B..ld-1 are never written
        return a[:, :self.B]

    def kept(self):
        """centres, velocities, sphere forces: (B, S, 3) each, in the caller's numbering"""
        k = self.get("keep")
        return tuple(np.ascontiguousarray(k[3 * self.S * i:3 * self.S * (i + 1)].T.reshape(self.B, self.S, 3)) for i in range(3))

    def readout(self):
        return np.ascontiguousarray(self.get("readout").T)

    def summary(self):
        return np.ascontiguousarray(self.get("summary").T)

    def tau(self):
        return np.ascontiguousarray(self.get("tau").T)


def _same(a, b):
    a, b = np.ascontiguousarray(a, float), np.ascontiguousarray(b, float)
    return a.shape == b.shape and bool(((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))).all())


def _bind_tau(ctrl, n, ld, values=None):
    """a caller-owned torque buffer (n, ld), bound; the padding columns hold a sentinel nothing may touch"""
    host = np.full((n, ld), SENTINEL)
    host[:, :ctrl.batch_size] = 0.0 if values is None else values.T
    buf = _DevBuf(host)
    ctrl.bindTauDevice(buf.ptr)
    return buf


# ------------------------------------------------------------------ 1. nothing touching is exact
@pytest.mark.parametrize("B,ld", SHAPES)
def test_nothing_touching_is_exact(sp, B, ld):
    K = 5
    ends = []
    sph = [("link4", (0.0, 0.0, 0.0), 0.06), ("link5", (0.0, 0.02, -0.1), 0.05), ("link7", (0.0, 0.0, 0.05), 0.04), ("end-effector", (0.0, 0.0, 0.03), 0.04)]
    for attached in (True, False):
        robot, ctrl, objs, mf, grav = _panda(B, False, ld=ld)
        if attached:
            ctrl.attachLinkContact(sph, FAR, FAR_MAT)
            out = _Outputs(ctrl, len(sph), 7, ld, False)
            assert ctrl.linkContactInfo() == dict(n_spheres=4, n_obstacles=2, per_instance=False, keep=False)
        ctrl.stepAsync()
        ctrl.integrate(DT, SUB, gravity=GRAV)
        first = tuple(a.copy() for a in ctrl.pullState())
        ctrl.recordRollouts(K, 1, ("q", "tau"), task=mf, summaries=True)
        ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
        ctrl.synchronize()
        ends.append((first[0], first[1], ctrl.pullState()[0].copy(), ctrl.pullState()[1].copy(), ctrl.getTorques(), ctrl.rolloutLog(), ctrl.rolloutSummary()))
        if attached:
            ro, s = out.readout(), out.summary()
            assert (ro[:, 5] == 0).all() and (ro[:, 3] > 10).all() and not ro[:, [0, 1, 2, 6, 7]].any() and not s.any()
            tau = ctrl.getTorques()
            assert _same(out.tau(), np.where(np.isnan(tau), 0.0, tau))   # tau_sim = u0: the commanded torques of the last period
            ctrl.detachLinkContact()
    a, c = ends
    for i in (0, 1, 2, 3, 4, 6):
        assert _same_bits(a[i], c[i]), i
    for key in ("q", "tau"):
        assert _same_bits(a[5][key], c[5][key]), key
    assert np.array_equal(a[5]["status"], c[5]["status"])


# ------------------------------------------------------------------ 2. the force stage bit for bit
@pytest.mark.parametrize("name,B,ld", [(n, *SHAPES[(i + 1) % 3]) for i, n in enumerate(MODELS)] + [("slider1", 3, 64), ("tree", 3, 64)])
def test_force_stage_bit_for_bit(sp, name, B, ld):
    robot, ctrl, objs, m, sph = _case(name, B, ld, seed=4)
    S, O = len(sph), 16 if name != "slider1" else 3
    radii = np.array([r for _, _, r in sph])
    order, _ = LC.sort_spheres(m, sph)
    rng = np.random.default_rng(17)
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    for per in (False, True):
        robot.setQ(q0)                                                   # the state of the case, for the second table too
        robot.setDq(dq0)
        ob, mat = _touching(rng, m, robot, sph, O, per)
        ctrl.attachLinkContact(sph, ob, mat, per_instance=per, keep=True)
        out = _Outputs(ctrl, S, m.dof, ld, True)
        for again in (False, True):
            if again:
                ob, mat = _touching(rng, m, robot, sph, O, per)
                ctrl.setLinkContactObstacles(ob)
                ctrl.setLinkContactMaterials(mat)
            ctrl.evaluateLinkContact()
            ro = out.readout()
            c, v, F = out.kept()
            want = LC.evaluate(c, v, radii, _ref_obst(ob, per), mat, order)
            assert _same(ro, want["readout"]), (name, per, again, np.argwhere(ro != want["readout"])[:5])
            assert _same(F, want["F"])
            print(f"{name} per={per}: share of active items {_share(ro, S, O):.2f}")
            face = ctrl.linkContactReadout()
            assert _same(face["force"], ro[:, 0:3]) and _same(face["distance"], ro[:, 3]) and _same(face["peak_force"], ro[:, 7])
            assert face["closest"] == [LC.decode(k, O) for k in ro[:, 4]] and np.array_equal(face["active"], ro[:, 5].astype(int))
        assert not out.summary().any()                                   # evaluate leaves the summaries alone
        # one APPLY substep at the same state: the same readout, the summaries advanced once from zero
        ctrl.integrate(DT, 1, gravity=GRAV)
        assert _same(out.readout(), ro) and _same(out.summary(), LC.summary_advance(np.zeros((B, 4)), DT, ro))
        face = ctrl.linkContactSummary()
        assert _same(face["impulse"], DT * ro[:, 6]) and np.array_equal(face["substeps_in_contact"], (ro[:, 5] > 0).astype(int))
        ctrl.detachLinkContact()


# ------------------------------------------------------------------ 3. centres and velocities against the model queries
@pytest.mark.parametrize("name,B,ld", [(n, *SHAPES[i % 3]) for i, n in enumerate(MODELS)])
def test_centres_and_velocities_match_the_model_queries(sp, name, B, ld):
    """The walk of this kernel and the walk of the model query are the same source (SAIP_FK_JOINT_STEP, SAIP_FK_TWIST_STEP) in two kernels:
    a centre differs by the contraction of the walk alone (CENTRE_BOUND).  A velocity is v = tv + tw x c - tc, at most 32 joints each adding
    a handful of roundings of <= 2e-16 relative to terms |dq_j| |o_j|, |dq_j| |c|: within 1e-12 of the scale sum_j |dq_j| x 2 m (no lever on
    these robots is longer), ten times over the count."""
    robot, ctrl, objs, m, sph = _case(name, B, ld)
    ctrl.attachLinkContact(sph, FAR, FAR_MAT, keep=True)
    out = _Outputs(ctrl, len(sph), m.dof, ld, True)
    ctrl.evaluateLinkContact()
    c, v, F = out.kept()
    want_c = _query_centres(robot, sph)
    want_v = np.stack([np.einsum("bij,bj->bi", robot.Jv(l, tuple(r)), robot._dq) for l, r, _ in sph], axis=1)
    worst = np.abs(c - want_c).max()
    scale = (np.abs(robot._dq).sum(axis=1) * 2.0).max()
    rel = np.abs(v - want_v).max() / scale
    print(f"{name} B={B}: worst |centre - model query| = {worst:.3e} m; worst |velocity - J_v dq| = {rel:.3e} of {scale:.3e} m/s")
    assert worst <= CENTRE_BOUND and rel <= 1e-12
    assert np.abs(want_v).max() > 0.1 and not F.any()
    if name == "forest":                                                 # the spheres on the fixed torso do not move
        base = [i for i, s in enumerate(sph) if s[0] == "torso"]
        assert len(base) == 2 and not v[:, base].any()
    ctrl.detachLinkContact()


# ------------------------------------------------------------------ 4., 8. torques end to end, on a caller-bound torque buffer
@pytest.mark.parametrize("name,B,ld", [(n, *SHAPES[(i + 2) % 3]) for i, n in enumerate(MODELS)])
def test_torques_are_jacobian_transpose_times_the_sphere_forces(sp, name, B, ld):
    robot, ctrl, objs, m, sph = _case(name, B, ld, seed=6)
    n, S, O = m.dof, len(sph), 16
    rng = np.random.default_rng(23)
    ob, mat = _touching(rng, m, robot, sph, O, True)
    tau_cmd = rng.uniform(-5, 5, (B, n))
    tau_cmd[B // 2] = np.nan
    base = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
    Jv = [robot.Jv(l, tuple(r)) for l, r, _ in sph]
    with _bind_tau(ctrl, n, ld, tau_cmd) as buf:
        ctrl.attachLinkContact(sph, ob, mat, per_instance=True, keep=True)
        out = _Outputs(ctrl, S, n, ld, True)
        ctrl.integrate(DT, 1, gravity=GRAV)
        got, (c, v, F), ro = out.tau(), out.kept(), out.readout()
        want = sum(np.einsum("bej,be->bj", Jv[s], F[:, s]) for s in range(S))
        scale = max(1.0, np.abs(want).max())
        err = np.abs((got - base) - want).max() / scale
        print(f"{name} B={B}: max |tau_sim - u0 - sum J_v^T F_s| = {err:.3e} of {scale:.3e}; share of active items {_share(ro, S, O):.2f}")
        assert err <= 1e-12 and not np.isnan(got).any()                  # the bound of the plant's wrenches
        quiet = ro[:, 5] == 0
        assert _same(got[quiet], base[quiet])                            # no active item: the commanded torques, bit for bit
        got_buf = buf.get()
        assert np.all(got_buf[:, B:] == SENTINEL) and _same(got_buf[:, :B], np.ascontiguousarray(tau_cmd.T))      # the commanded torques are never written
        ctrl.detachLinkContact()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 5. two cross-checks against code that already exists
@pytest.mark.parametrize("name,B,ld", [("panda_arm", 65, 128), ("chain30w", 3, 64), ("tree", 130, 192), ("forest", 65, 128)])
def test_smallest_distance_equals_the_clearance_monitor(sp, name, B, ld):
    robot, ctrl, objs, m, sph = _case(name, B, ld, seed=8)
    S, O = len(sph), 16
    rng = np.random.default_rng(31)
    for per in (False, True):
        ob, mat = _touching(rng, m, robot, sph, O, per)
        ctrl.attachClearance(sph, ob, margin=0.0, per_instance=per)
        ctrl.attachLinkContact(sph, ob, mat, per_instance=per)
        out = _Outputs(ctrl, S, m.dof, ld, False)
        ctrl.evaluateClearance()
        ctrl.evaluateLinkContact()
        ro, mon = out.readout(), ctrl.clearanceReadout()
        _share(ro, S, O)
        assert _same(ro[:, 3], mon["distance"]) and np.array_equal(ro[:, 4].astype(int), mon["item"])
        ctrl.detachLinkContact()
        ctrl.detachClearance()


@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_one_point_sphere_equals_the_contact_planes(sp, B, ld):
    """one radius-0 sphere at the motion-force task's control point against one half-space, and attachContactPlanes with the same plane and
    material: the two kernels walk the same chain with different roundings (contraction), so tau_sim agrees within 1e-12 relative"""
    robot, ctrl, objs, mf, grav = _panda(B, False, ld=ld)
    rng = np.random.default_rng(5)
    robot.setDq(0.3 * rng.uniform(-1, 1, (B, 7)))
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    link, pos = W.make_inputs(2, B)["tasks"][0]["link"], W.make_inputs(2, B)["tasks"][0]["pos_in_link"]
    p = robot.position(link, tuple(pos))
    n = np.array([0.0, 0.6, 0.8])
    off = np.quantile(p @ n, 0.5)                                        # half of the instances are inside the half-space's wall
    k, c, mu, vs = 2.0e4, 300.0, 0.4, 1e-3
    tau_cmd = rng.uniform(-20, 20, (B, 7))
    with _bind_tau(ctrl, 7, ld, tau_cmd):
        ctrl.attachLinkContact([(link, tuple(pos), 0.0)], np.array([[1, *n, off, 0, 0, 0]]), np.array([[k, c, mu, vs]]))
        out = _Outputs(ctrl, 1, 7, ld, False)
        ctrl.integrate(DT, 1, gravity=GRAV)
        got, ro = out.tau(), out.readout()
        ctrl.detachLinkContact()
        robot.setQ(q0)
        robot.setDq(dq0)
        mf.attachContactPlanes(np.array([[*n, off, k, c, mu, vs]]), sensor=False)
        ctrl.integrate(DT, 1, gravity=GRAV)
        ctrl.synchronize()
        want = _d2h(mf.contactTorquesDevice(), (7, ld))[:, :B].T
        face = mf.contactReadout()
        mf.detachContactPlanes()
    ctrl.bindTauDevice(0)
    active = ro[:, 5] == 1
    assert 0.25 <= active.mean() <= 0.75 and np.array_equal(active, face["active"] == 1)
    scale = max(1.0, np.abs(want - tau_cmd).max())
    err = np.abs(got - want).max() / scale
    print(f"worst |tau_sim (link contact) - tau_sim (contact planes)| = {err:.3e} of {scale:.3e}")
    assert err <= 1e-12 and scale > 10.0
    assert _same(got[~active], tau_cmd[~active]) and np.abs(ro[:, 0:3] - face["force"]).max() <= 1e-12 * max(1.0, np.abs(face["force"]).max())


# ------------------------------------------------------------------ 6. physics: a sphere dropped onto a half-space
@pytest.mark.parametrize("B,ld", SHAPES)
def test_drop_on_a_half_space(sp, B, ld):
    """The 1-dof slider of mass m carries a sphere of radius r released above the half-space z >= 0 under gravity, k = 1e4, critical damping
    c = 2 sqrt(k m), dt = 5e-4, 400 periods of one substep.  The first 40 periods are compared with the NumPy stepping of the restatement:
    the oscillator and the error propagation of test_drop_on_a_joint_stop (tests/test_gpu_plant.py) -- per substep a few roundings,
    <= 8 eps on q, on dq and on dt ddq; in the energy norm the wall does not amplify them, in free flight q_err grows by dt dq_err per
    step: after s substeps dq_err <= s inj, q_err <= s inj (1 / om + s dt), inj = 8 eps (om max|q| + max|dq| + dt max|ddq|).  Then the rest
    state: penetration m g / k, within the residual of the critically damped semi-implicit step after the remaining time (the derivation
    of test_drop_on_a_plane)."""
    from sai_primitives_amd.controller import controller_from_specs
    m, k, g, r = 2.0, 1.0e4, 9.81, 0.05
    c = 2.0 * np.sqrt(k * m)
    om = np.sqrt(k / m)
    robot, ctrl, objs = controller_from_specs(_slider1(m), [W.joint_task("posture")], B, device=0, leading_dimension=ld)
    h0 = np.linspace(0.0, 2e-3, B)                  # instance i starts with its sphere h0[i] above the wall, at rest
    robot.setQ((r + h0)[:, None])
    robot.setDq(np.zeros((B, 1)))
    robot.updateModel()
    floor, mat = np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]]), np.array([[k, c, 0.5, 1e-3]])
    sph = [("link1", (0.0, 0.0, 0.0), r)]
    with _bind_tau(ctrl, 1, ld) as buf:             # commanded torque 0: free fall onto the wall
        ctrl.attachLinkContact(sph, floor, mat)
        out = _Outputs(ctrl, 1, 1, ld, False)
        q, dq = r + h0, np.zeros(B)
        checked, total = 40, 400
        hist, touching = [], []
        for period in range(checked):
            cen, vel = np.zeros((B, 1, 3)), np.zeros((B, 1, 3))
            cen[:, 0, 2], vel[:, 0, 2] = q, dq
            ev = LC.evaluate(cen, vel, [r], floor, mat)
            touching.append(ev["readout"][:, 5].sum())
            ddq = (ev["F"][:, 0, 2] - m * g) / m
            dq = dq + DT * ddq
            q = q + DT * dq
            hist.append((np.abs(q).max(), np.abs(dq).max(), np.abs(ddq).max()))
            ctrl.integrate(DT, 1)
            gq, gdq = ctrl.pullState()
            hq, hdq, hdd = (max(h[i] for h in hist) for i in range(3))
            s = period + 1
            inj = 8 * EPS * (om * hq + hdq + DT * hdd)
            b_dq, b_q = s * inj, s * inj * (1.0 / om + s * DT)
            assert np.abs(gq[:, 0] - q).max() <= b_q, (period, np.abs(gq[:, 0] - q).max(), b_q)
            assert np.abs(gdq[:, 0] - dq).max() <= b_dq, (period, np.abs(gdq[:, 0] - dq).max(), b_dq)
        print(f"B={B}: after {checked} periods worst |q - restatement| = {np.abs(gq[:, 0] - q).max():.3e} (bound {b_q:.3e}), "
              f"|dq - restatement| = {np.abs(gdq[:, 0] - dq).max():.3e} (bound {b_dq:.3e})")
        assert touching[0] == 0 and touching[-1] > 0                     # the item is inactive at the start (h0 = 0: d == 0 exactly) and active later
        for _ in range(total - checked):
            ctrl.integrate(DT, 1)
        gq, gdq = ctrl.pullState()
        T = (total - checked) * DT
        a = om * DT
        start = 2e-3 + 2 * m * g / k
        resid = 2.0 * (1.0 + om * T) * np.exp(-om * T * (1.0 - 1.01 * np.sqrt(a) - a)) * start
        pen = r - gq[:, 0]
        print(f"B={B}: worst |penetration - m g / k| = {np.abs(pen - m * g / k).max():.3e} (m g / k = {m * g / k:.3e}, bound {resid + b_q:.3e})")
        assert resid < 0.05 * m * g / k
        assert np.abs(pen - m * g / k).max() <= resid + b_q
        sm = ctrl.linkContactSummary()
        assert (sm["substeps_in_contact"] > total - 60).all() and (sm["substeps_in_contact"] <= total).all() and (sm["max_penetration"] >= pen - resid).all()
        assert np.abs(out.tau()[:, 0] - m * g).max() <= (k + c * om) * (resid + b_q)          # the wall carries the weight
        assert np.all(buf.get()[:, B:] == SENTINEL) and not buf.get()[:, :B].any()
        ctrl.detachLinkContact()
    ctrl.bindTauDevice(0)


def test_panda_elbow_stops_on_the_table(sp):
    """A joint task (kp 900, kv 60, no internal OTG, no gravity) drives the Panda's shoulder 0.4 rad down: the elbow sphere would sink about
    10 cm below a table 1 cm under it.  160 periods of one substep at dt = 1e-3, k = 2e5 N/m (k dt^2 / m_eff ~ 0.05 at the elbow), near-
    critical damping.  Reference: the same loop in NumPy -- per period RS.controller_step, the contact torques of the restatement at the
    state, RS.forward_dynamics, semi-implicit Euler -- and its largest penetration over the states the summaries see.

    Margin: the reference and the device differ in the forward dynamics (the restatement's is finite-differenced; the existing tests hold
    it to 1e-7 relative of the acceleration) and in roundings.  With |ddq| <= ~500 rad/s^2 at the impact that is <= 5e-5 rad/s^2, over
    T = 0.16 s at most T^2 / 2 x 5e-5 = 6.4e-7 rad, x 0.32 m of lever = 2e-7 m at the elbow, and the damped wall does not amplify it
    (as in the drop test).  MARGIN = 1e-5 m is fifty times that, a thousandth of the penetration.  The difference of the two
    penetrations and of q at the end of the run are printed; the latter is not covered by this estimate and is not asserted.

    Stops: at the end the elbow stands no deeper than that bound, the wall pushes it upwards, and its vertical speed is under 5 % of the
    speed the same rollout without the attachment still has there (a stopped and a passing elbow differ by far more).  Goes through:
    without the attachment the elbow ends more than five times the bound below the table."""
    from sai_primitives_amd.controller import controller_from_specs
    import restatement as RS
    B, ld, K, dt, R, MARGIN = 3, 64, 160, 1e-3, 0.06, 1e-5
    m = W.load_robot("panda_arm")
    specs = [W.joint_task("posture", kp=900.0, kv=60.0)]
    q0 = np.tile(np.array([0.2, 1.0, -0.3, -1.6, 0.1, 1.8, 0.4]), (B, 1))
    q0[:, 1] += np.linspace(0.0, 0.06, B)
    dq0 = np.zeros((B, 7))
    qg = q0.copy()
    qg[:, 1] += 0.4
    sph = [("link4", (0.0, 0.0, 0.0), R), ("link3", (0.0, 0.0, 0.0), 0.05)]
    radii = [r for _, _, r in sph]
    c0 = LC.sphere_state(m, q0, dq0, sph)[0]
    table_z = c0[:, 0, 2].min() - R - 0.01
    floor, mat = np.array([[1, 0.0, 0.0, 1.0, table_z, 0, 0, 0]]), np.array([[2.0e5, 1500.0, 0.3, 1e-3]])
    # the reference stepping
    order, anc = LC.sort_spheres(m, sph)
    goals = [np.concatenate([qg, np.zeros((B, 14))], axis=1)]
    q, dq, pen_ref = q0.copy(), dq0.copy(), np.zeros(B)
    for _ in range(K):
        tau, status = RS.controller_step(m, specs, q, dq, goals)
        assert not status.any()
        cc, vv, (frames, jtype, aw, oj) = LC.sphere_state(m, q, dq, sph)
        ev = LC.evaluate(cc, vv, radii, floor, mat, order)
        pen_ref = np.maximum(pen_ref, np.maximum(0.0, -ev["readout"][:, 3]))
        ddq = RS.forward_dynamics(m, q, dq, LC.torques(ev, cc, order, anc, jtype, aw, oj, tau), g=GRAV)
        dq = dq + dt * ddq
        q = q + dt * dq
    bound = pen_ref + MARGIN

    def run(attach):
        robot, ctrl, objs = controller_from_specs("panda_arm", specs, B, device=0, disable_otg=True, leading_dimension=ld)
        robot.setQ(q0)
        robot.setDq(dq0)
        robot.updateModel()
        ctrl.reinitializeTasks()
        objs[0].setGoalPosition(qg)
        ctrl.updateControllerTaskModels()
        out = None
        if attach:
            ctrl.attachLinkContact(sph, floor, mat)
            out = _Outputs(ctrl, len(sph), 7, ld, False)
        ctrl.rolloutAsync(K, dt, 1, gravity=GRAV)
        gq, gdq = (a.copy() for a in ctrl.pullState())
        robot.updateModel()
        d = robot.position("link4")[:, 2] - R - table_z
        vz = np.einsum("bj,bj->b", robot.Jv("link4")[:, 2], gdq)
        return ctrl, out, gq, d, vz

    ctrl, out, gq, d, vz = run(True)
    ctrl.evaluateLinkContact()
    ro, sm = out.readout(), ctrl.linkContactSummary()
    ctrl2, _, gq2, d2, vz2 = run(False)
    print(f"largest penetration: summaries {sm['max_penetration']}, reference stepping {pen_ref}, worst difference "
          f"{np.abs(sm['max_penetration'] - pen_ref).max():.3e} m (margin {MARGIN:.0e} m); worst |q - reference| at the end {np.abs(gq - q).max():.3e} rad")
    print(f"final elbow clearance with the attachment {d} m at {vz} m/s; without it {d2} m at {vz2} m/s")
    assert (pen_ref > 1e-3).all() and (sm["substeps_in_contact"] > K // 2).all()
    assert (sm["max_penetration"] <= bound).all()
    assert (d >= -bound).all() and (ro[:, 2] > 0).all() and (ro[:, 5] == 1).all()          # it stands on the table, which pushes upwards
    assert (np.abs(vz) <= 0.05 * np.abs(vz2)).all()
    assert (d2 < -5.0 * bound).all() and (vz2 < 0).all()                                    # without the attachment it goes through
    ctrl.detachLinkContact()


# ------------------------------------------------------------------ 7. composition and rollouts
def _panda_in_contact(B, ld, otg=False, attach=True, keep=False, free=None):
    """config 2's stack on the Panda, moving, with five spheres and four obstacles through them; free: instances whose obstacles (a
    per-instance table then) are moved out of reach"""
    robot, ctrl, objs, mf, grav = _panda(B, otg, ld=ld)
    rng = np.random.default_rng(11)
    robot.setDq(0.2 * rng.uniform(-1, 1, (B, 7)))
    robot.updateModel()
    ctrl.updateControllerTaskModels()                                    # (pushes the state: stepAsync alone does not)
    sph = [("link4", (0.0, 0.0, 0.0), 0.06), ("link5", (0.0, 0.02, -0.1), 0.05), ("link6", (0.0, 0.0, 0.0), 0.05), ("link7", (0.0, 0.0, 0.05), 0.04),
           ("end-effector", (0.0, 0.0, 0.03), 0.04)]
    m = W.make_inputs(2, B)["model"]
    ob, mat = _touching(rng, m, robot, sph, 4, False)
    mat[:, 0] = np.minimum(mat[:, 0], 1e4)                               # k dt^2 / m_eff stays small at DT
    if free is not None:
        ob = np.repeat(ob[:, None, :], B, axis=1)
        hs = ob[..., 0] == 1
        ob[:, free, 1:7] += np.where(hs[:, free, None], 0.0, 50.0)       # capsules and spheres 50 m away in every coordinate ...
        ob[:, free, 4] -= np.where(hs[:, free], 50.0, 0.0)               # ... half-spaces 50 m below
    if attach:
        ctrl.attachLinkContact(sph, ob, mat, keep=keep, per_instance=free is not None)
    return robot, ctrl, objs, mf, m, sph, ob, mat


@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_plant_in_front_and_contact_planes_behind(sp, B, ld):
    """the three buffers chain: plant tau_act -> link contact tau_sim -> contact planes tau_sim -> integrator.  First against the three
    restatements applied in order (tests/plant_ref.py, tests/link_contact_ref.py fed the kernel's centres and velocities and the joint
    axes of the NumPy kinematics, tests/contact_ref.py at the control point of the model queries), within 1e-12 relative: the device
    walks differ from the NumPy kinematics in roundings only.  Then each stage alone, fed the buffer in front of it as commanded
    torques, reproduces its own buffer bit for bit, and the plain integrator fed the last buffer reaches the same state."""
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, attach=False)
    rng = np.random.default_rng(2)
    tau_cmd = rng.uniform(-20, 20, (B, 7))
    tau_cmd[5] = np.nan
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    p = robot.position("end-effector", (0, 0, 0.07))
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, 2.0e4, 400.0, 0.3, 1e-3]
    planes[0, :, 3] = p[:, 2] + 2e-3
    table = PL.neutral(7)
    table[:, PL.GAIN], table[:, PL.TAU_MAX], table[:, PL.FV] = 0.9, 15.0, 0.5

    def reset():
        robot.setQ(q0)
        robot.setDq(dq0)

    spec = W.make_inputs(2, B)["tasks"][0]
    pc = robot.position(spec["link"], tuple(spec["pos_in_link"]))        # the contact point is the task's control point
    Jc = robot.Jv(spec["link"], tuple(spec["pos_in_link"]))
    with _bind_tau(ctrl, 7, ld, tau_cmd) as buf:
        ctrl.attachPlant(table)
        ctrl.attachLinkContact(sph, ob, mat, keep=True)
        mf.attachContactPlanes(planes, sensor=False, per_instance=True)
        out = _Outputs(ctrl, len(sph), 7, ld, True)
        ctrl.integrate(DT, 1, gravity=GRAV)
        ctrl.synchronize()
        act = _d2h(ctrl.plantTorquesDevice(), (7, ld))[:, :B].T
        lsim, ro = out.tau(), out.readout()
        csim = _d2h(mf.contactTorquesDevice(), (7, ld))[:, :B].T
        q1, dq1 = (a.copy() for a in ctrl.pullState())
        _share(ro, len(sph), 4)
        assert np.abs(act - np.where(np.isnan(tau_cmd), 0.0, tau_cmd)).max() > 1.0 and np.abs(lsim - act).max() > 1.0 and np.abs(csim - lsim).max() > 1.0
        # the three restatements in order
        act_ref = PL.joint(table, tau_cmd, q0, dq0)[0]
        c, v, F = out.kept()
        order, anc = LC.sort_spheres(m, sph)
        ev = LC.evaluate(c, v, [r for _, _, r in sph], ob, mat, order)
        frames, jtype, aw, oj = LC.joints(m, q0)
        lsim_ref = LC.torques(ev, c, order, anc, jtype, aw, oj, act_ref)
        f_plane = CT.plane_forces(planes.transpose(1, 0, 2), pc, np.einsum("bij,bj->bi", Jc, dq0))[0]
        csim_ref = lsim_ref + np.einsum("bej,be->bj", Jc, f_plane)
        assert _same(F, ev["F"]) and _same(ro, ev["readout"])
        for what, got, want in (("plant", act, act_ref), ("link contact", lsim, lsim_ref), ("contact planes", csim, csim_ref)):
            err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
            print(f"{what}: worst |device - restatement chain| = {err:.3e} of {max(1.0, np.abs(want).max()):.3e}")
            assert err <= 1e-12, what
        assert np.abs(f_plane).max() > 1.0
        assert np.all(buf.get()[:, B:] == SENTINEL)
        mf.detachContactPlanes()
        ctrl.detachPlant()
    # link contact alone, commanded tau_act
    reset()
    with _bind_tau(ctrl, 7, ld, act):
        ctrl.integrate(DT, 1, gravity=GRAV)
        assert _same(out.tau(), lsim)
    ctrl.detachLinkContact()
    # the contact planes alone, commanded link contact's tau_sim
    reset()
    with _bind_tau(ctrl, 7, ld, lsim):
        mf.attachContactPlanes(planes, sensor=False, per_instance=True)
        ctrl.integrate(DT, 1, gravity=GRAV)
        ctrl.synchronize()
        assert _same(_d2h(mf.contactTorquesDevice(), (7, ld))[:, :B].T, csim)
        mf.detachContactPlanes()
    # the plain integrator fed the last buffer
    reset()
    ctrl.bindTauDevice(0)
    ctrl.setTorques(csim)
    ctrl.integrate(DT, 1, gravity=GRAV)
    q3, dq3 = ctrl.pullState()
    assert _same_bits(q1, q3) and _same_bits(dq1, dq3)


def _final(ctrl, objs, out):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float), goals=[t._get_goal() for t in objs],
                summary=out.summary(), readout=out.readout(), sim=out.tau())


def _equal_runs(a, b):
    for key in a:
        if key == "goals":
            assert all(_same_bits(x, y) for x, y in zip(a[key], b[key]))
        else:
            assert _same(np.asarray(a[key]), np.asarray(b[key])), key


@pytest.mark.parametrize("otg,B,ld", [(False, 65, 128), (True, 130, 192), (False, 3, 64)])
def test_rollout_equals_the_host_driven_loop(sp, otg, B, ld):
    K = 6
    runs = []
    for host in (False, True):
        robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, otg)
        out = _Outputs(ctrl, len(sph), 7, ld, False)
        if host:
            for _ in range(K):
                ctrl.stepAsync()
                ctrl.integrate(DT, SUB, gravity=GRAV)
        else:
            ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
        runs.append(_final(ctrl, objs, out))
        ctrl.detachLinkContact()
    _equal_runs(*runs)
    a = runs[0]
    assert np.isfinite(a["q"]).all() and (a["summary"][:, 3] > 0).any() and (a["summary"][:, 3] <= K * SUB).all() and (a["summary"][:, 0] > 0).any()
    # the same rollout without the attachment ends elsewhere: the obstacles pushed
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, otg, attach=False)
    ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
    touched = a["summary"][:, 3] > 0
    assert not _same_bits(ctrl.pullState()[0][touched], a["q"][touched])


def _stacked(B, ld, otg, K):
    """every stage of a period at once on the moving Panda in contact: a plant, link contact, contact planes with the simulated sensor under
    the tool (every instance starts 2 mm inside), a sensing model with a joint table and a wrench table, the guards of
    tests/test_gpu_guard.py on the sensed force, and the recorder"""
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, otg)
    table = PL.neutral(7)
    table[:, PL.GAIN], table[:, PL.TAU_MAX], table[:, PL.FV] = 0.9, 15.0, 0.5
    ctrl.attachPlant(table)
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, 2.0e4, 400.0, 0.3, 1e-3]
    planes[0, :, 3] = robot.position("end-effector", (0, 0, 0.07))[:, 2] + 2e-3
    mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    mf.attachGuards(GUARDS, PHASES)
    ctrl.recordRollouts(K, 1, ("q", "dq", "tau"), task=mf)
    joints = np.zeros((7, 6))
    joints[:, 0], joints[:, 1], joints[:, 2], joints[:, 5] = 0.01, 2 * np.pi / 2 ** 14, 1e-3, 1e-3       # offset, resolution, noise on q and dq
    wrench = np.zeros((6, 3))
    wrench[:, 0], wrench[:3, 1], wrench[:, 2] = 0.2, 0.25, 0.05
    ctrl.attachSensing(joints, wrenches={mf: wrench}, seed=5)
    return robot, ctrl, objs, mf, _Outputs(ctrl, len(sph), 7, ld, False)


def _stacked_final(ctrl, objs, mf, out, ld):
    """_final, and what every other attachment of _stacked has to show"""
    B = ctrl.batch_size
    a = _final(ctrl, objs, out)
    a["plant_act"] = _d2h(ctrl.plantTorquesDevice(), (7, ld))[:, :B].T
    a["planes_sim"] = _d2h(mf.contactTorquesDevice(), (7, ld))[:, :B].T
    a["q_meas"], a["dq_meas"] = ctrl.measuredState()
    for name, d in (("plant", ctrl.plantSummary()), ("planes", mf.contactReadout()), ("planes_sum", mf.contactSummary()), ("guard", ctrl.guardState()),
                    ("guard_ro", ctrl.guardReadout())):
        a.update({f"{name}.{k}": v for k, v in d.items()})
    a["periods"] = [ctrl.plantInfo()["period"], ctrl.sensingInfo()["period"]]
    return a


@pytest.mark.parametrize("B,ld", [(65, 128), (3, 64)])
@pytest.mark.parametrize("otg", [False, True])
def test_stacked_rollout_equals_the_host_driven_loop(sp, otg, B, ld):
    """plant + link contact + contact planes with the sensor + sensing model + guards + recorder: K periods in one rolloutAsync against the
    host-driven loop { contactSense, measureState, evaluateGuards, stepAsync, integrate }, bit for bit in the state, the torques, the goals,
    every attachment's buffer, readout and summary, the guard state and the two period counters.  The recorder acts inside rollouts only:
    its log is compared with what the host loop pulls after every integrate."""
    K = 6
    robot, ctrl, objs, mf, out = _stacked(B, ld, otg, K)
    ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
    roll, log = _stacked_final(ctrl, objs, mf, out, ld), ctrl.rolloutLog()
    robot, ctrl, objs, mf, out = _stacked(B, ld, otg, K)
    pulled = dict(q=[], dq=[], tau=[], status=[])
    for _ in range(K):
        ctrl.contactSense()
        ctrl.measureState()
        ctrl.evaluateGuards()
        ctrl.stepAsync()
        ctrl.integrate(DT, SUB, gravity=GRAV)
        ctrl.synchronize()
        for key, val in zip(("q", "dq", "tau", "status"), (*ctrl.pullState(), ctrl.getTorques(), ctrl.status)):
            pulled[key].append(np.array(val, float))
    _equal_runs(roll, _stacked_final(ctrl, objs, mf, out, ld))
    assert np.array_equal(log["period"], np.arange(1, K + 1))
    for key in pulled:
        assert _same(log[key], np.stack(pulled[key])), key
    # conditions, so that nothing above holds vacuously: every stage acted
    assert roll["periods"] == [K, K] and np.isfinite(roll["q"]).all()
    assert (roll["summary"][:, 3] > 0).any() and (roll["plant.friction_loss"] > 0).all() and (roll["planes_sum.max_force"] > 1.0).any()
    assert (roll["guard.entry"][1] >= 0).any() and (roll["guard.clock"] == K).all()
    assert not _same(roll["q_meas"], roll["q"]) and np.abs(roll["goals"][0][:, 30:33]).max() > 1.0
    assert not _same(roll["plant_act"], roll["sim"]) and not _same(roll["sim"], roll["planes_sim"])


@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_snapshot_restore_reproduces_a_rollout(sp, B, ld):
    K = 6
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, attach=False)
    plain = ctrl.saveState()
    layout, nbytes = plain.segments(), plain.nbytes()
    ctrl.attachLinkContact(sph, ob, mat)
    out = _Outputs(ctrl, len(sph), 7, ld, False)
    snap = ctrl.saveState()
    assert snap.segments() == layout and snap.nbytes() == nbytes         # the attachment is configuration: not part of a snapshot
    ends = []
    for _ in range(2):
        ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
        ends.append(_final(ctrl, objs, out))
        ctrl.restoreState(snap)
        ctrl.resetLinkContactSummary()
        assert not out.summary().any()
    _equal_runs(*ends)
    assert (ends[0]["summary"][:, 3] > 0).any()
    ctrl.detachLinkContact()


@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_link_contact_cost_and_the_sampler(sp, B, ld):
    K = 6
    free = np.arange(B) % 3 == 2                                         # every third instance has nothing in reach
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, free=free)
    out = _Outputs(ctrl, len(sph), 7, ld, False)
    ctrl.evaluateLinkContact()
    _share(out.readout(), len(sph), 4)
    with pytest.raises(sp.SaipError, match="no sampler is attached"):
        ctrl.linkContactCost(1.0)
    p0 = mf._get_goal()[0, :3]
    nominal = np.tile(p0, (2, 1))
    mf.setGoalSchedule("position", np.repeat(nominal[:, None], B, axis=1), stride=3, mode="linear")
    mf.attachSampler(0.01, nominal=nominal, exempt=0)
    ctrl.recordRollouts(K, 1, ("pose",), task=mf)
    ctrl.seedSampler(7)
    ctrl.perturbGoalSchedules()
    ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
    ctrl.rolloutCost(target=p0, final_weight=1.0)
    cost0 = ctrl.getRolloutCost()
    s = out.summary()
    ctrl.linkContactCost(3.0, 0.25)
    cost1 = ctrl.getRolloutCost()
    assert _same(cost1, LC.add_cost(cost0, s[:, 0], s[:, 1], 3.0, 0.25))
    touched = s[:, 3] > 0
    assert touched.any() and not touched[free].any() and (cost1[touched] > cost0[touched]).all() and _same(cost1[~touched], cost0[~touched])
    # an infinite weight makes touching a hard constraint for the update (0 x inf would be NaN for the others: w_peak stays 0)
    ctrl.setRolloutCost(cost0)
    ctrl.linkContactCost(1e300)
    cost2 = ctrl.getRolloutCost()
    ctrl.setRolloutCost(np.where(touched, np.inf, cost2))
    ctrl.updateSampler(1e-3)
    res = ctrl.samplerResult()
    assert res["n_valid"] == B - touched.sum() and not touched[res["best"]] and res["best"] == int(np.argmin(np.where(touched, np.inf, cost0)))
    # with the cost as link contact left it, the update prefers a sample that does not touch
    ctrl.setRolloutCost(cost2)
    ctrl.updateSampler(1e-3)
    assert not touched[ctrl.samplerResult()["best"]]
    ctrl.detachLinkContact()


# ------------------------------------------------------------------ without an attachment
def test_without_an_attachment(sp):
    from sai_primitives_amd import capi
    robot, ctrl, objs, mf, grav = _panda(3, False)
    L = capi.lib()
    out = np.full(8 * 3, 7.0)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    for fn, args in (("detach", ()), ("info", (None,) * 4), ("set_obstacles_host", (dp,)), ("set_materials_host", (dp,)), ("evaluate", ()), ("readout_host", (dp,)),
                     ("summary_host", (dp,)), ("summary_reset", ()), ("add_cost", (1.0, 1.0))):
        assert getattr(L, "saip_batch_link_contact_" + fn)(ctrl._h, *args) == capi.SAIP_ERR_ORDER, fn
        assert b"no link contact is attached" in L.saip_last_error()
    for fn in ("obstacles", "readout", "summary", "torques", "keep"):
        assert getattr(L, f"saip_batch_link_contact_{fn}_device")(ctrl._h) is None
    assert (out == 7.0).all()
    ctrl.attachLinkContact([("link4", (0, 0, 0), 0.05)], FAR, FAR_MAT)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachLinkContact([("link4", (0, 0, 0), 0.05)], FAR, FAR_MAT)
    assert L.saip_batch_link_contact_obstacles_device(ctrl._h) and ctrl.linkContactKeepDevice() is None
    ctrl.detachLinkContact()
    assert ctrl.linkContactTorquesDevice() is None
