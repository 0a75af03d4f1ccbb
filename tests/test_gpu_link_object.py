"""The pushed object of link contact on the device (saip_link_object_apply of csrc/saip_link_contact.hip, saip_batch_link_object_*).
Oracles: the NumPy restatement tests/link_object_ref.py for the force stage and the body's step (fed the kernel's own kept centres and
velocities of the robot spheres), the engine's model queries for the Jacobians, a batch with link contact alone for everything that must
not change, the host-driven loop for rollouts, the snapshot's own source columns.

Batches (B, ld) in {(9, 64), (70, 128)}: a block with a partly live group, a batch with a partly filled block, at a padded leading
dimension.  The padding columns of every output are pre-filled with a sentinel that must survive."""
import numpy as np
import pytest

import link_contact_ref as LC
import link_object_ref as LO
import workloads as W
from test_gpu_batch_layout import _d2h, _h2d, _same_bits
from test_gpu_link_contact import (DT, EPS, FAR, FAR_MAT, GRAV, SENTINEL, SUB, _bind_tau, _case, _equal_runs, _final, _Outputs, _panda_in_contact, _ref_obst, _same,
                                   _slider1, _touching)

pytestmark = pytest.mark.gpu

SHAPES = [(9, 64), (70, 128)]
G = np.array([0.0, 0.0, -9.81])
REST = np.r_[0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, np.zeros(6)]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


class _ObjOutputs:
    """the device arrays of the object with the padding columns pre-filled with a sentinel"""

    def __init__(self, ctrl, ld):
        from sai_primitives_amd import capi
        L = capi.lib()
        ctrl.synchronize()
        self.ctrl, self.B, self.ld = ctrl, ctrl.batch_size, ld
        self.bufs = dict(state=(L.saip_batch_link_object_state_device(ctrl._h), 13), readout=(L.saip_batch_link_object_readout_device(ctrl._h), 12),
                         summary=(L.saip_batch_link_object_summary_device(ctrl._h), 4))
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
        return np.ascontiguousarray(a[:, :self.B].T)


def _shape(rng, P):
    return [(rng.uniform(-0.05, 0.05, 3), float(rng.uniform(0.03, 0.07))) for _ in range(P)]


def _near(rng, centres, B):
    """object states (B, 13) with the origin near a robot sphere of the instance, turning and moving"""
    S = centres.shape[1]
    x = np.zeros((B, 13))
    x[:, 0:3] = centres[np.arange(B), rng.integers(S, size=B)] + rng.uniform(-0.06, 0.06, (B, 3))
    q = rng.normal(size=(B, 4))
    x[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    x[:, 7:10], x[:, 10:13] = 0.2 * rng.normal(size=(B, 3)), 2.0 * rng.normal(size=(B, 3))
    return x


def _inertial(rng, B, per):
    inr = np.stack([rng.uniform(0.2, 1.0, B), *(rng.uniform(5e-4, 5e-3, B) for _ in range(3))], axis=1)
    return inr if per else inr[0]


# ------------------------------------------------------------------ 1. an object out of reach changes nothing
@pytest.mark.parametrize("B,ld", SHAPES)
def test_far_object_changes_nothing(sp, B, ld):
    K, runs = 6, []
    for attached in (False, True):
        robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld)
        out = _Outputs(ctrl, len(sph), 7, ld, False)
        if attached:
            # far from the robot and from its obstacles: 50 m out on the free side of the half-spaces (the capsules and spheres are at the robot)
            hs = ob[ob[:, 0] == 1]
            away = hs[:, 1:4].sum(axis=0) / np.linalg.norm(hs[:, 1:4].sum(axis=0))
            x0 = np.tile(REST, (B, 1))
            x0[:, 0:3] = 50.0 * away + np.arange(B)[:, None] * 0.01
            assert len(hs) >= 1 and ((x0[:, 0:3] @ hs[:, 1:4].T - hs[:, 4]) > 10.0).all()
            ctrl.attachLinkObject(_shape(np.random.default_rng(1), 8), [1e4, 10.0, 0.5, 1e-3], [0.5, 1e-3, 2e-3, 3e-3], state=x0)
            oo = _ObjOutputs(ctrl, ld)
            assert ctrl.linkObjectInfo() == dict(n_spheres=8, per_instance=False)
        ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
        runs.append(_final(ctrl, objs, out))
        if attached:
            assert _same(oo.get("state"), x0) and not oo.get("summary").any()
            rq = oo.get("readout")
            assert not rq[:, 0:9].any() and (rq[:, 9] > 10).all() and not rq[:, 11].any()
        ctrl.detachLinkContact()
    _equal_runs(*runs)
    assert (runs[0]["summary"][:, 3] > 0).any()                          # the robot did touch its obstacles


# ------------------------------------------------------------------ 2., 3. the force stage and the body's step bit for bit; the torques
@pytest.mark.parametrize("name,B,ld,P,per", [("panda_arm", 70, 128, 8, True), ("slider1", 9, 64, 1, False), ("tree", 9, 64, 8, False), ("panda_arm", 9, 64, 1, True),
                                             ("slider1", 70, 128, 8, True)])
def test_force_stage_step_and_torques(sp, name, B, ld, P, per):
    """EVALUATE, then one APPLY substep at the same state, against the restatement fed the kernel's kept centres and velocities: both readouts,
    F_s, both summaries and the new object state bit for bit.  tau_sim - u0 against sum_s J_v(c_s)^T F_s of the model queries within 1e-12
    relative: the bound of tests/test_gpu_link_contact.py on the same torque loop."""
    robot, ctrl, objs, m, sph = _case(name, B, ld, seed=4)
    n, S, O = m.dof, len(sph), 3 if name == "slider1" else 4
    rng = np.random.default_rng(29 + P)
    radii = np.array([r for _, _, r in sph])
    order, _ = LC.sort_spheres(m, sph)
    ob, mat = _touching(rng, m, robot, sph, O, per)
    shape, omat, inr = _shape(rng, P), np.array([2e4, 40.0, 0.5, 1e-3]), _inertial(rng, B, per)
    x0 = _near(rng, LC.sphere_state(m, robot._q, robot._dq, sph)[0], B)
    tau_cmd = rng.uniform(-5, 5, (B, n))
    tau_cmd[B // 2] = np.nan
    base = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
    Jv = [robot.Jv(l, tuple(r)) for l, r, _ in sph]
    with _bind_tau(ctrl, n, ld, tau_cmd):
        ctrl.attachLinkContact(sph, ob, mat, per_instance=per, keep=True)
        ctrl.attachLinkObject(shape, omat, inr, per_instance=per, state=x0)
        out, oo = _Outputs(ctrl, S, n, ld, True), _ObjOutputs(ctrl, ld)
        x = oo.get("state")
        assert np.abs(x - x0).max() <= 4 * EPS and _same(ctrl.objectState(), x)          # (the quaternion was normalised once more on the host)
        ctrl.evaluateLinkContact()
        c, v, F = out.kept()
        st = LO.step(c, v, radii, _ref_obst(ob, per), mat, order, x, inr, np.array([r for r, _ in shape]), np.array([r for _, r in shape]), omat, G, DT)
        ro, rq = out.readout(), oo.get("readout")
        assert _same(ro, st["readout_lc"]) and _same(rq, st["readout"]), np.argwhere(rq != st["readout"])[:5]
        assert _same(F, st["F"]) and _same(oo.get("state"), x) and not oo.get("summary").any() and not out.summary().any()      # EVALUATE advances nothing
        ctrl.integrate(DT, 1, gravity=G)
        assert _same(out.readout(), ro) and _same(oo.get("readout"), rq) and _same(out.kept()[2], st["F"])
        assert _same(oo.get("state"), st["state"]), np.argwhere(oo.get("state") != st["state"])[:5]
        assert _same(oo.get("summary"), LO.summary_advance(np.zeros((B, 4)), DT, st)) and _same(out.summary(), LC.summary_advance(np.zeros((B, 4)), DT, ro))
        touching, resting = (rq[:, 11] > 0).mean(), (st["partial"]["wpen"] > 0).mean()
        print(f"{name} B={B} P={P}: instances with an active robot-object item {touching:.2f}, with object-world penetration {resting:.2f}")
        assert 0.2 <= touching and 0.1 <= resting and (st["state"] != x).any(axis=1).all()
        # the torques
        got = out.tau()
        want = sum(np.einsum("bej,be->bj", Jv[s], F[:, s]) for s in range(S))
        scale = max(1.0, np.abs(want).max())
        err = np.abs((got - base) - want).max() / scale
        print(f"{name} B={B} P={P}: max |tau_sim - u0 - sum J_v^T F_s| = {err:.3e} of {scale:.3e}")
        assert err <= 1e-12 and not np.isnan(got).any()
        quiet = (ro[:, 5] == 0) & (rq[:, 11] == 0)
        assert _same(got[quiet], base[quiet])
        # the facade speaks of the same arrays
        face, fs = ctrl.objectReadout(), ctrl.objectSummary()
        assert _same(face["raw"], rq) and face["closest"] == [LO.decode(k, P) for k in rq[:, 10]] and _same(fs["raw"], oo.get("summary"))
        assert _same(face["force"], rq[:, 0:3]) and _same(face["world_force"], rq[:, 6:9]) and np.array_equal(fs["substeps_in_contact"], (rq[:, 11] > 0).astype(int))
        ctrl.resetObjectSummary()
        assert not oo.get("summary").any()
        # an instance with a state that is not finite is invalid: tau_sim = u0, the state stays, the readout is NaN; its neighbours go on
        xb = oo.get("state")
        xb[0, 1], xb[B - 1, 12] = np.nan, np.inf
        ctrl.setObjectState(xb)
        keep = oo.get("state")
        ctrl.integrate(DT, 1, gravity=G)
        got, rq2, x2 = out.tau(), oo.get("readout"), oo.get("state")
        for i in (0, B - 1):
            assert np.isnan(rq2[i]).all() and _same(x2[i], keep[i]) and _same(got[i], base[i]) and np.isnan(oo.get("summary")[i, 0])
        assert np.isfinite(rq2[1:B - 1]).all() and np.isfinite(x2[1:B - 1]).all()
        ctrl.detachLinkObject()
        assert ctrl.objectStateDevice() is None
        ctrl.detachLinkContact()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 4. rollouts
def _panda_with_object(B, ld, otg, P=8, per=True):
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, otg)
    rng = np.random.default_rng(41)
    x0 = _near(rng, LC.sphere_state(m, robot._q, robot._dq, sph)[0], B)
    x0[:, 7:13] *= 0.1
    ctrl.attachLinkObject(_shape(rng, P), [8e3, 20.0, 0.4, 1e-3], _inertial(rng, B, per), per_instance=per, state=x0)
    return robot, ctrl, objs, _Outputs(ctrl, len(sph), 7, ld, False), _ObjOutputs(ctrl, ld)


def _final_with_object(ctrl, objs, out, oo):
    a = _final(ctrl, objs, out)
    a.update(obj_state=oo.get("state"), obj_readout=oo.get("readout"), obj_summary=oo.get("summary"))
    return a


@pytest.mark.parametrize("otg,B,ld", [(False, 70, 128), (True, 9, 64)])
def test_rollout_equals_the_host_driven_loop(sp, otg, B, ld):
    K, runs = 6, []
    for host in (False, True, None):
        robot, ctrl, objs, out, oo = _panda_with_object(B, ld, otg)
        if host is None:                                                 # substeps = 2 against two integrate calls of one substep
            for _ in range(K):
                ctrl.stepAsync()
                ctrl.integrate(DT, 1, gravity=G)
                ctrl.integrate(DT, 1, gravity=G)
        elif host:
            for _ in range(K):
                ctrl.stepAsync()
                ctrl.integrate(DT, SUB, gravity=G)
        else:
            ctrl.rolloutAsync(K, DT, SUB, gravity=G)
        runs.append(_final_with_object(ctrl, objs, out, oo))
        ctrl.detachLinkContact()
        assert ctrl.objectStateDevice() is None                          # detaching link contact detaches the object
    _equal_runs(runs[0], runs[1])
    _equal_runs(runs[0], runs[2])
    a = runs[0]
    assert np.isfinite(a["q"]).all() and np.isfinite(a["obj_state"]).all() and (a["obj_summary"][:, 3] > 0).mean() > 0.2 and (a["obj_summary"][:, 3] <= K * SUB).all()
    # the same rollout without the object ends elsewhere where it was touched
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld, otg)
    ctrl.rolloutAsync(K, DT, SUB, gravity=G)
    touched = a["obj_summary"][:, 3] > 0
    assert not _same_bits(ctrl.pullState()[0][touched], a["q"][touched])


# ------------------------------------------------------------------ 5. snapshots
@pytest.mark.parametrize("B,ld", SHAPES)
def test_snapshot_carries_the_object(sp, B, ld):
    from sai_primitives_amd.controller import StateSnapshot
    K = 4
    robot, ctrl, objs, mf, m, sph, ob, mat = _panda_in_contact(B, ld)
    plain = ctrl.saveState().segments()
    robot, ctrl, objs, out, oo = _panda_with_object(B, ld, False)
    snap = ctrl.saveState()
    segs = snap.segments()
    assert [s for s in segs if s["name"] != "link_object.state"] == [dict(s, offset=t["offset"]) for s, t in zip(plain, [s for s in segs if s["name"] != "link_object.state"])]
    seg = [s for s in segs if s["name"] == "link_object.state"]
    assert len(seg) == 1 and (seg[0]["rows"], seg[0]["elem_bytes"], seg[0]["kind"]) == (13, 8, "soa")
    x0 = oo.get("state")
    ctrl.rolloutAsync(K, DT, SUB, gravity=G)
    first = _final_with_object(ctrl, objs, out, oo)
    assert (first["obj_state"] != x0).any(axis=1).all()
    ctrl.restoreState(snap)
    assert _same(oo.get("state"), x0)
    ctrl.resetLinkContactSummary()
    ctrl.resetObjectSummary()
    ctrl.rolloutAsync(K, DT, SUB, gravity=G)
    _equal_runs(first, _final_with_object(ctrl, objs, out, oo))
    ctrl.restoreState(snap, 0)
    assert _same(oo.get("state"), np.tile(x0[0], (B, 1)))
    perm = np.random.default_rng(3).permutation(B)
    ctrl.restoreState(snap, perm)
    assert _same(oo.get("state"), x0[perm])
    blob = snap.tobytes()
    ctrl.rolloutAsync(1, DT, SUB, gravity=G)
    again = StateSnapshot.frombytes(ctrl, blob)
    ctrl.restoreState(again)
    assert _same(oo.get("state"), x0)
    # the layout follows the attachment: the old snapshot no longer fits, a new one has today's directory
    ctrl.detachLinkObject()
    with pytest.raises(sp.SaipError, match=r"segment \[link_object.state\] is gone"):
        ctrl.restoreState(snap)
    assert ctrl.saveState().segments() == plain
    ctrl.detachLinkContact()


# ------------------------------------------------------------------ 6. momentum
@pytest.mark.parametrize("B,ld", SHAPES)
def test_momentum_is_conserved_through_a_collision(sp, B, ld):
    """The slider of mass M runs into a one-sphere object of mass m at rest: no gravity, no damping, no friction, commanded torque 0.  The
    bound is the one tests/test_link_object_cpu.py derives: 8 eps sum |dt F| + K eps (M max|dq| + m max|v_z|); sum |dt F| is the object's
    impulse summary, and since both bodies move in +z throughout, M |dq| + m |v_z| is the momentum itself."""
    from sai_primitives_amd.controller import controller_from_specs
    M, mo, k, K, r = 2.0, 0.5, 2.0e4, 240, 0.05
    robot, ctrl, objs = controller_from_specs(_slider1(M), [W.joint_task("posture")], B, device=0, leading_dimension=ld)
    q0, dq0 = np.linspace(-0.13, -0.11, B), np.linspace(0.5, 1.1, B)
    robot.setQ(q0[:, None])
    robot.setDq(dq0[:, None])
    robot.updateModel()
    with _bind_tau(ctrl, 1, ld):
        ctrl.attachLinkContact([("link1", (0.0, 0.0, 0.0), r)], FAR, FAR_MAT)
        ctrl.attachLinkObject([((0.0, 0.0, 0.0), r)], [k, 0.0, 0.0, 0.0], [mo, 1e-3, 1e-3, 1e-3])
        oo = _ObjOutputs(ctrl, ld)
        for _ in range(K):
            ctrl.integrate(DT, 1, gravity=GRAV)
        q, dq = ctrl.pullState()
        x, sm = oo.get("state"), oo.get("summary")
        P0, P1 = M * dq0, M * dq[:, 0] + mo * x[:, 9]
        bound = 8 * EPS * sm[:, 0] + K * EPS * P0
        print(f"B={B}: worst |P_K - P_0| = {np.abs(P1 - P0).max():.3e} kg m/s (smallest bound {bound.min():.3e}); impulse {sm[:, 0].min():.3f} .. {sm[:, 0].max():.3f} N s")
        assert (np.abs(P1 - P0) <= bound).all() and (sm[:, 0] > 0.1).all() and (sm[:, 3] > 3).all()
        assert (x[:, 9] > dq[:, 0]).all() and (x[:, 2] - q[:, 0] > 2 * r).all() and not x[:, [0, 1, 7, 8, 10, 11, 12]].any()      # the object moves away, along the axis
        ctrl.detachLinkContact()
    ctrl.bindTauDevice(0)


# ------------------------------------------------------------------ 7. push: the Panda sweeps a forearm sphere into a puck on a table
def _push_case(B):
    """the Panda at rest, a joint task that swings joint 1 (the base yaw) by 0.25 .. 0.35 rad, a sphere on the forearm 1 cm above a table, and a
    one-sphere puck resting on the table 2.5 cm ahead of that sphere on its path"""
    R_S, R_P, MASS, K_T, dt = 0.03, 0.04, 0.3, 2.0e4, 1e-3
    m = W.load_robot("panda_arm")
    q0 = np.tile(np.array([0.2, 1.0, -0.3, -1.6, 0.1, 1.8, 0.4]), (B, 1))
    qg = q0.copy()
    qg[:, 0] += np.linspace(0.25, 0.35, B)
    sph = [("link5", (0.0, 0.0, 0.0), R_S)]
    c0 = LC.sphere_state(m, q0, np.zeros((B, 7)), sph)[0][:, 0]
    ahead = q0.copy()
    ahead[:, 0] += (R_S + R_P + 0.025) / np.linalg.norm(c0[0, 0:2])     # the yaw that carries the sphere's centre that far along its circle
    c1 = LC.sphere_state(m, ahead, np.zeros((B, 7)), sph)[0][:, 0]
    table_z = c0[0, 2] - R_P
    floor, mat = np.array([[1, 0.0, 0.0, 1.0, table_z, 0, 0, 0]]), np.array([[K_T, 2.0 * np.sqrt(K_T * MASS), 0.5, 1e-3]])
    x0 = np.tile(REST, (B, 1))
    x0[:, 0:2], x0[:, 2] = c1[:, 0:2], table_z + R_P - MASS * 9.81 / K_T  # at rest on the table: penetration m g / k
    return dict(m=m, q0=q0, qg=qg, sph=sph, floor=floor, mat=mat, x0=x0, dt=dt, radius=R_P, shape=[((0.0, 0.0, 0.0), R_P)], omat=np.array([2.0e4, 20.0, 0.3, 1e-3]),
                inr=np.array([MASS, 2e-4, 2e-4, 2e-4]), specs=[W.joint_task("posture", kp=900.0, kv=60.0)])


def test_panda_pushes_a_puck_across_the_table(sp):
    """A joint task (kp 900, kv 60, no internal OTG) swings the Panda's base joint by 0.25 .. 0.35 rad; a forearm sphere meets a puck (one
    sphere, 0.3 kg, friction 0.3 against the robot and 0.5 against the table it rests on) and pushes it across the table, under gravity,
    140 periods of one substep at dt = 1e-3.  Reference: the same loop in NumPy -- per period RS.controller_step, the restatement of the
    object stage at the state (robot-object and object-world items, the body's step), RS.forward_dynamics on its tau_sim, semi-implicit
    Euler -- and the puck's displacement at the end.

    Margin, as test_panda_elbow_stops_on_the_table of tests/test_gpu_link_contact.py derives it: the reference and the device differ in
    the forward dynamics (the restatement's is finite-differenced, held to 1e-7 relative of the acceleration) and in roundings.  With
    |ddq| <= ~500 rad/s^2 that is <= 5e-5 rad/s^2: after T = 0.14 s at most T x 5e-5 = 7e-6 rad/s and T^2 / 2 x 5e-5 = 4.9e-7 rad, x 0.5 m
    of lever = 3.5e-6 m/s and 2.5e-7 m at the sphere.  The contact is a spring between two bodies: what the puck takes away is at most
    twice the error of the approach speed, 7e-6 m/s, which over the remaining <= 0.14 s is <= 1e-6 m, plus the sphere's position error;
    the table's friction is regularised and does not amplify it.  MARGIN = 1e-5 m is eight times that sum.

    Moves: with the attachment the puck ends more than its own radius from where it started and stays on the table; without the object
    there is no object to move, and the arm ends elsewhere, because nothing pushed back."""
    from sai_primitives_amd.controller import controller_from_specs
    import restatement as RS
    B, ld, K, MARGIN = 9, 64, 140, 1e-5
    c = _push_case(B)
    m, dt, sph = c["m"], c["dt"], c["sph"]
    radii = [r for _, _, r in sph]
    shape_r, shape_radius = np.array([r for r, _ in c["shape"]]), np.array([r for _, r in c["shape"]])
    order, anc = LC.sort_spheres(m, sph)
    goals = [np.concatenate([c["qg"], np.zeros((B, 14))], axis=1)]
    q, dq, x, touched = c["q0"].copy(), np.zeros((B, 7)), c["x0"].copy(), np.zeros(B)
    for _ in range(K):
        tau, status = RS.controller_step(m, c["specs"], q, dq, goals)
        assert not status.any()
        cc, vv, (frames, jtype, aw, oj) = LC.sphere_state(m, q, dq, sph)
        st = LO.step(cc, vv, radii, c["floor"], c["mat"], order, x, c["inr"], shape_r, shape_radius, c["omat"], G, dt)
        touched += st["readout"][:, 11] > 0
        ddq = RS.forward_dynamics(m, q, dq, LO.torques(st, cc, order, anc, jtype, aw, oj, tau), g=tuple(G))
        dq = dq + dt * ddq
        q = q + dt * dq
        x = st["state"]
    moved_ref = np.linalg.norm(x[:, 0:3] - c["x0"][:, 0:3], axis=1)

    def run(attach):
        robot, ctrl, objs = controller_from_specs("panda_arm", c["specs"], B, device=0, disable_otg=True, leading_dimension=ld)
        robot.setQ(c["q0"])
        robot.setDq(np.zeros((B, 7)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        objs[0].setGoalPosition(c["qg"])
        ctrl.updateControllerTaskModels()
        ctrl.attachLinkContact(sph, c["floor"], c["mat"])
        if attach:
            ctrl.attachLinkObject(c["shape"], c["omat"], c["inr"], state=c["x0"])
        ctrl.rolloutAsync(K, dt, 1, gravity=G)
        return ctrl, ctrl.pullState()[0].copy()

    ctrl, gq = run(True)
    gx, sm = ctrl.objectState(), ctrl.objectSummary()
    moved = np.linalg.norm(gx[:, 0:3] - c["x0"][:, 0:3], axis=1)
    ctrl2, gq2 = run(False)
    print(f"puck displacement after {K} periods: device {moved}, reference stepping {moved_ref}, worst difference {np.abs(moved - moved_ref).max():.3e} m "
          f"(margin {MARGIN:.0e} m); worst |puck position - reference| {np.abs(gx[:, 0:3] - x[:, 0:3]).max():.3e} m, worst |q - reference| {np.abs(gq - q).max():.3e} rad")
    assert (touched > 3).all() and (sm["substeps_in_contact"] > 3).all() and (sm["max_world_penetration"] > 0).all()
    assert (np.abs(moved - moved_ref) <= MARGIN).all()
    assert (moved > c["radius"]).all() and (np.abs(gx[:, 2] - c["x0"][:, 2]) < 1e-3).all()         # pushed across the table, still on it
    assert ctrl2.objectStateDevice() is None and (np.abs(gq2 - gq).max(axis=1) > 1e-4).all()          # without the object nothing pushed back on the arm
    ctrl.detachLinkContact()
    ctrl2.detachLinkContact()


# ------------------------------------------------------------------ 8. the cost, and the error contract behind an attachment
@pytest.mark.parametrize("B,ld", [(9, 64)])
def test_object_cost_and_errors_behind_an_attachment(sp, B, ld):
    from test_gpu_rollout_record import _panda
    K = 6
    robot, ctrl, objs, mf, grav = _panda(B, False, ld=ld)
    q = np.tile(robot._q[0], (B, 1))
    q[1, 1] -= 0.6                                                       # instance 1 holds its arm elsewhere: it cannot reach the object
    robot.setQ(q)
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    ee = robot.position("end-effector", (0.0, 0.0, 0.03))
    assert np.linalg.norm(ee[1] - ee[0]) > 0.2
    sph = [("end-effector", (0.0, 0.0, 0.03), 0.04)]
    with pytest.raises(sp.SaipError, match="no link contact is attached"):
        ctrl.attachLinkObject([((0, 0, 0), 0.05)], [5e3, 5.0, 0.3, 1e-3], [0.5, 1e-3, 1e-3, 1e-3])
    ctrl.attachLinkContact(sph, FAR, FAR_MAT)
    x0 = np.tile(REST, (B, 1))
    x0[:, 0:3] = ee[0] + [0.07, 0.0, 0.0]                                # 2 cm inside the end-effector sphere of every arm that is there, on its +x side
    ctrl.attachLinkObject([((0, 0, 0), 0.05)], [5e3, 5.0, 0.3, 1e-3], [0.5, 1e-3, 1e-3, 1e-3], state=x0)
    oo = _ObjOutputs(ctrl, ld)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachLinkObject([((0, 0, 0), 0.05)], [5e3, 5.0, 0.3, 1e-3], [0.5, 1e-3, 1e-3, 1e-3])
    with pytest.raises(sp.SaipError, match="no sampler is attached"):
        ctrl.objectCost(ee[0], 1.0)
    # what is refused behind an attachment leaves the state and the inertial words as they are
    for bad in (0.0, np.nan, np.inf):
        xb = x0.copy()
        xb[B - 2, 3:7] = bad
        with pytest.raises(ValueError, match=f"instance {B - 2}: the quaternion is zero or not finite"):
            ctrl.setObjectState(xb)
        with pytest.raises(ValueError, match="the quaternion is zero or not finite"):
            ctrl.setObjectState(xb[B - 2])
    with pytest.raises(ValueError, match=r"inertial word 0 \(m\) = "):
        ctrl.setObjectInertial([0.0, 1e-3, 1e-3, 1e-3])
    assert _same(oo.get("state"), x0)
    ctrl.setObjectState(np.r_[1.0, 2.0, 3.0, 0.0, 3.0, 0.0, 4.0, np.zeros(6)])           # normalised on the host, every instance
    assert np.abs(oo.get("state") - np.r_[1.0, 2.0, 3.0, 0.0, 0.6, 0.0, 0.8, np.zeros(6)]).max() <= EPS
    ctrl.setObjectState(x0)
    # the cost
    p0 = mf._get_goal()[0, :3]
    nominal = np.tile(p0, (2, 1))
    mf.setGoalSchedule("position", np.repeat(nominal[:, None], B, axis=1), stride=3, mode="linear")
    mf.attachSampler(0.01, nominal=nominal, exempt=0)
    ctrl.rolloutAsync(K, DT, SUB, gravity=GRAV)
    x = oo.get("state")
    target = ee[0] + [0.3, 0.0, 0.0]
    rng = np.random.default_rng(9)
    for tq, w in ((None, 0.0), ((0.5, 0.5, 0.5, 0.5), 0.75), ((1.0, 0.0, 0.0, 0.0), 2.0)):
        cost0 = rng.normal(size=B)
        ctrl.setRolloutCost(cost0)
        ctrl.objectCost(target, 3.0, tq, w)
        assert _same(ctrl.getRolloutCost(), LO.add_cost(cost0, x, target, 3.0, tq, w)), tq
    ctrl.setRolloutCost(np.zeros(B))
    ctrl.objectCost(target, 1.0)
    cost = ctrl.getRolloutCost()
    sm = ctrl.objectSummary()
    print(f"cost of the pushing instance {cost[0]:.6f}, of the one out of reach {cost[1]:.6f} (0.23^2 = 0.0529: its object rests); the object moved {x[0, 0] - x0[0, 0]:.3e} m")
    assert sm["substeps_in_contact"][0] > 0 and sm["substeps_in_contact"][1] == 0 and _same(x[1], x0[1])
    assert cost[0] < cost[1] and cost[1] == LO.add_cost(np.zeros(1), x0[1:2], target, 1.0, None, 0.0)[0] and x[0, 0] > x0[0, 0]
    for bad, msg in (((np.nan, 0, 0), "target position is not finite"),):
        with pytest.raises(ValueError, match=msg):
            ctrl.objectCost(bad, 1.0)
    with pytest.raises(ValueError, match="a weight is NaN"):
        ctrl.objectCost(target, np.nan)
    with pytest.raises(ValueError, match="target quaternion is zero"):
        ctrl.objectCost(target, 1.0, (0, 0, 0, 0), 1.0)
    xb = x.copy()
    xb[2, 0] = np.nan
    ctrl.setObjectState(xb)
    ctrl.setRolloutCost(np.zeros(B))
    ctrl.objectCost(target, 1.0)
    assert ctrl.getRolloutCost()[2] == np.inf and np.isfinite(ctrl.getRolloutCost()[[0, 1, 3]]).all()
    ctrl.detachLinkContact()
