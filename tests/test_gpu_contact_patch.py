"""Contact patches on the device (csrc/saip_contact_patch.hip, saip_batch_contact_patch_*).  Oracles: the single-point attachment (one
point is the old kernel), the NumPy restatements tests/contact_ref.py and tests/contact_patch_ref.py, the engine's own model queries
(pose, velocity, Jacobian of every contact point), the plain integrator given the same torques, and the host-driven loop
{ contactPatchSense, cycle, integrate } for whole rollouts.

Batches B in {3, 65, 130}: a partial group row, a partial block (eight instances per block) and more than one wavefront, at a padded
leading dimension, torques in a caller-bound buffer."""
import ctypes as C

import numpy as np
import pytest

import chains as CH
import contact_ref as CR
import trees as TR
import workloads as W
from test_gpu_batch_layout import _DevBuf, _d2h, _same_bits
from test_gpu_contact import _bind_tau, _cfg13, _table_under

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
DT, SUB = 5e-4, 2
ZERO_G = (0.0, 0.0, 0.0)
SENTINEL = 6.02214076e23
SQUARE = np.array([[0.05, 0.05, 0.0], [-0.05, 0.05, 0.0], [-0.05, -0.05, 0.0], [0.05, -0.05, 0.0]])
EE, EE_POS = "end-effector", np.array([0.0, 0.0, 0.07])


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _patch_tau_sim(ctrl, mf, n, ld):
    ctrl.synchronize()
    return _d2h(mf.contactPatchTorquesDevice(), (n, ld))


def _floor(robot, link, pos, pts, depth, k=2.0e4, c=400.0, mu=0.3):
    """per-instance planes with normal +z whose deepest point of the patch starts `depth` inside"""
    B = robot.batch_size
    pz = np.stack([robot.position(link, tuple(np.asarray(pos) + r))[:, 2] for r in pts])
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 1, 0, k, c, mu, 1e-3]
    planes[0, :, 3] = pz.min(axis=0) + depth
    return planes


# ------------------------------------------------------------------ 1. one point is the old kernel
def test_one_point_is_the_single_point_kernel(sp):
    B, ld = 65, 128
    rc = (0.01, 0.02, -0.015)
    runs = []
    for patch in (False, True):
        robot, ctrl, objs = _cfg13(B, ld, False)
        mf = objs[0]
        buf = _bind_tau(ctrl, 7, ld)
        planes = _table_under(robot, objs, 2e-3, rc=rc)
        if patch:
            mf.attachContactPatch([rc], planes, sensor=True, per_instance=True)
        else:
            mf.attachContactPlanes(planes, point=rc, sensor=True, per_instance=True)
        out = {}
        for stage in ("integrate", "rollout"):
            if stage == "integrate":
                ctrl.integrate(DT, 1, gravity=ZERO_G)
            else:
                ctrl.rolloutAsync(6, DT, 2, gravity=ZERO_G)
            ctrl.synchronize()
            q, dq = ctrl.pullState()
            ro = mf.contactPatchReadout() if patch else mf.contactReadout()
            sm = mf.contactPatchSummary() if patch else mf.contactSummary()
            sim = _d2h(mf.contactPatchTorquesDevice() if patch else mf.contactTorquesDevice(), (7, ld))
            out[stage] = dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), tau_sim=sim, sensed=mf._get_goal()[:, 30:36], force=ro["force"],
                              dmin=ro["distance"], touching=ro["n_touch"] if patch else (ro["active"] > 0).astype(int),
                              summary=np.column_stack([sm[key] for key in ("impulse", "max_force", "max_penetration", "substeps_in_contact")]))
        runs.append(out)
        (mf.detachContactPatch if patch else mf.detachContactPlanes)()
        ctrl.bindTauDevice(0)
        buf.free()
    old, new = runs
    for stage in old:
        for key in old[stage]:
            assert np.array_equal(old[stage][key], new[stage][key]), (stage, key, np.abs(old[stage][key] - new[stage][key]).max())
    assert (old["rollout"]["summary"][:, 3] >= 1).all() and np.abs(old["rollout"]["sensed"]).max() > 1.0      # something was compared


# ------------------------------------------------------------------ 2. net wrench
def _model_case(name, B, ld, seed=5):
    """(robot, ctrl, objs, model, [(task index, link, pos_in_link)] of the patches): a stack at a random state"""
    from sai_primitives_amd.controller import controller_from_specs
    rng = np.random.default_rng(seed)
    if name == "tree":
        desc = TR.dual_panda_torso()
        m = W.RobotModel(desc)
        specs, where = TR.dual_stack(m), [(0, "left_link7", (0.0, 0.0, 0.1)), (1, "right_link7", (0.0, 0.0, 0.1))]
    elif name == "puma6":
        desc = CH.puma_arm()
        m = W.RobotModel(desc)
        specs, where = [W.motion_force_task("hand", "link6", (0.05, 0.0, 0.02)), W.joint_task("posture")], [(0, "link6", (0.05, 0.0, 0.02))]
    else:
        d = W.make_inputs({"panda_arm": 2, "chain30": 5}[name], B)
        desc, m, specs = d["model"].name, d["model"], d["tasks"]
        where = [(0, specs[0]["link"], tuple(specs[0]["pos_in_link"]))]
    q = np.clip(rng.uniform(-1.2, 1.2, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    dq = rng.uniform(-0.5, 0.5, (B, m.dof))
    robot, ctrl, objs = controller_from_specs(desc, specs, B, device=0, leading_dimension=ld)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    return robot, ctrl, objs, m, where


def _classed_planes(rng, p, cls):
    """two planes per instance around the points p (n, B, 3).  Class 0: every point 1..5 mm in front of both planes; class 1: every point
    1..5 mm behind plane 0 (odd instances: behind plane 1 too); class 2: plane 0 passes through the middle of the widest gap between the
    points along its normal (at least 1 mm from either neighbour), so some points touch and some do not"""
    n, B = p.shape[:2]
    nrm = rng.normal(size=(2, B, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    s = np.einsum("kbe,ibe->kib", nrm, p)                       # n_k . p_i
    pen = rng.uniform(1e-3, 5e-3, (2, B))
    free, full = s.min(axis=1) - pen, s.max(axis=1) + pen
    off = free.copy()
    srt = np.sort(s[0], axis=0)
    j = np.argmax(np.diff(srt, axis=0), axis=0)[None]
    mid = 0.5 * (np.take_along_axis(srt, j, axis=0) + np.take_along_axis(srt, j + 1, axis=0))[0]
    off[0] = np.where(cls == 1, full[0], np.where(cls == 2, mid, free[0]))
    off[1] = np.where((cls == 1) & (np.arange(B) % 2 == 1), full[1], free[1])
    planes = np.zeros((2, B, 8))
    planes[..., :3] = nrm
    planes[..., 3] = off
    planes[..., 4:] = [1.0e3, 15.0, 0.6, 1e-2]
    d = s - off[:, None, :]
    assert (np.abs(d) >= 1e-3 * (1 - 1e-9)).all()               # "active" cannot depend on rounding
    return planes


@pytest.mark.parametrize("name,B,ld,npts", [("panda_arm", 65, 128, (3,)), ("puma6", 3, 64, (8,)), ("chain30", 130, 192, (8,)), ("tree", 65, 128, (3, 8))])
def test_net_wrench_is_jacobian_transpose_times_forces(sp, name, B, ld, npts):
    robot, ctrl, objs, m, where = _model_case(name, B, ld)
    n = m.dof
    rng = np.random.default_rng(9)
    tau_cmd = rng.uniform(-5, 5, (B, n))
    tau_cmd[B // 2] = np.nan                                     # a flagged instance under the NaN policy
    base = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    want, patches = np.zeros((B, n)), []
    for k, ((ti, link, pos), npt) in enumerate(zip(where, npts)):
        pts = rng.uniform(-0.04, 0.04, (npt, 3))
        at = [tuple(np.asarray(pos) + r) for r in pts]           # the control frame is the link frame moved to `pos`
        p = np.stack([robot.position(link, a) for a in at])
        v = np.stack([robot.linearVelocity(link, a) for a in at])
        Jv = np.stack([robot.Jv(link, a) for a in at])
        xc = robot.position(link, pos)
        cls = (np.arange(B) // 3 ** k) % 3 if B > 3 else np.arange(B)
        planes = _classed_planes(rng, p, cls)
        res = [CR.plane_forces(planes.transpose(1, 0, 2), p[i], v[i]) for i in range(npt)]                    # f, fn_sum, dmin, active
        f, fn = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
        dm = np.stack([r[2:] for r in res])                                                                  # (npt, 2, B): dmin, active
        ext = np.einsum("ibej,ibe->bj", Jv, f)
        want += ext
        patches.append(dict(mf=objs[ti], pts=pts, planes=planes, F=f.sum(axis=0), M=np.cross(p - xc[None], f).sum(axis=0), xc=xc, ext=ext, fn=fn.T,
                            n_touch=(dm[:, 1] > 0).sum(axis=0).astype(int), i_deep=np.argmin(dm[:, 0], axis=0), dmin=dm[:, 0].min(axis=0), npt=npt))
    with _bind_tau(ctrl, n, ld, tau_cmd) as buf:
        for P in patches:
            P["mf"].attachContactPatch(P["pts"], P["planes"], sensor=False, per_instance=True)
        ctrl.integrate(DT, 1)
        sim = _patch_tau_sim(ctrl, patches[0]["mf"], n, ld)
        q1, dq1 = (a.copy() for a in ctrl.pullState())
        got = sim[:, :B].T - base
        scale = max(1.0, np.abs(want).max())
        err = np.abs(got - want).max() / scale
        print(f"{name}: max |tau_sim - tau_cmd - sum Jv(p_i)^T f_i| = {err:.3e} of {scale:.3e}")
        assert err <= 1e-12                                      # the bound of test_gpu_model_queries.py on the Jacobians
        touch = [P["n_touch"] > 0 for P in patches]
        for P in patches:
            ro = P["mf"].contactPatchReadout()
            seen = set(P["n_touch"])
            assert 0 in seen and P["npt"] in seen and any(0 < x < P["npt"] for x in seen), seen
            assert np.array_equal(ro["n_touch"], P["n_touch"]) and np.array_equal(ro["deepest"], P["i_deep"])
            for key, ref in (("force", P["F"]), ("moment", P["M"]), ("control_point", P["xc"])):
                e = np.abs(ro[key] - ref).max() / max(1.0, np.abs(ref).max())
                print(f"  {key}: {e:.3e}")
                assert e <= 1e-12, key
            assert np.abs(ro["distance"] - P["dmin"]).max() <= 1e-12
            assert not ro["normal_forces"][:, P["npt"]:].any()
            assert np.abs(ro["normal_forces"][:, :P["npt"]] - P["fn"]).max() <= 1e-12 * max(1.0, np.abs(P["fn"]).max())
            # columns B.. of the patch's own arrays are never written (zero since the attach)
            assert not _d2h(P["mf"].contactPatchReadoutDevice(), (20, ld))[:, B:].any()
            assert not _d2h(P["mf"].contactPatchSummaryDevice(), (6, ld))[:, B:].any()
        nothing = ~np.any(touch, axis=0)
        assert nothing.any() and _same_bits(sim[:, :B].T[nothing], base[nothing])      # nothing touches: the torques pass bit for bit
        assert not np.isnan(sim[:, :B]).any() and not sim[:, B:].any()
        if name == "tree":
            # joints off a patch's branch receive exactly nothing from it: an arm whose own patch is free keeps its commanded torques
            # bit for bit whatever the other arm touches, and the torso (the common trunk) carries both
            par = TR.joint_parents(m)
            arms = []
            for body in (7, 14):                                 # left_link7, right_link7
                anc = np.zeros(n, bool)
                j = body
                while j >= 0:
                    anc[j] = True
                    j = par[j]
                arms.append(anc)
            left_only, right_only = arms[0] & ~arms[1], arms[1] & ~arms[0]
            assert left_only.sum() == 7 and right_only.sum() == 7 and (arms[0] & arms[1]).sum() == 1
            sel = ~touch[0] & touch[1]
            assert sel.any() and _same_bits(sim[:, :B].T[sel][:, left_only], base[sel][:, left_only])
            sel = touch[0] & ~touch[1]
            assert sel.any() and _same_bits(sim[:, :B].T[sel][:, right_only], base[sel][:, right_only])
            assert np.abs(patches[0]["ext"][:, right_only]).max() == 0.0 and np.abs(patches[1]["ext"][:, left_only]).max() == 0.0
            both = touch[0] & touch[1]
            assert both.any() and np.abs(got[both][:, 0]).max() > 0
        assert np.all(buf.get()[:, B:] == SENTINEL)
        for P in patches:
            P["mf"].detachContactPatch()
        # the same substep by the plain integrator given tau = tau_sim: the same bits
        robot.setQ(q0)
        robot.setDq(dq0)
        ctrl.bindTauDevice(0)
        ctrl.setTorques(sim[:, :B].T)
        ctrl.integrate(DT, 1)
        q2, dq2 = ctrl.pullState()
        assert _same_bits(q1, q2) and _same_bits(dq1, dq2)


# ------------------------------------------------------------------ 3. rollout vs host-driven loop
def _dual(B, ld, otg):
    """the dual-arm tree with a motion-force task per flange, at rest at a random posture"""
    from sai_primitives_amd.controller import controller_from_specs
    desc = TR.dual_panda_torso()
    m = W.RobotModel(desc)
    rng = np.random.default_rng(21)
    robot, ctrl, objs = controller_from_specs(desc, TR.dual_stack(m), B, device=0, disable_otg=not otg, leading_dimension=ld)
    robot.setQ(np.clip(rng.uniform(-0.8, 0.8, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1))
    robot.setDq(np.zeros((B, m.dof)))
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, m.dof


def _final(ctrl, objs, mfs, ld):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    out = dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float))
    for i, t in enumerate(objs):
        out[f"goal{i}"] = t._get_goal()
    for i, mf in enumerate(mfs):
        out[f"readout{i}"] = _d2h(mf.contactPatchReadoutDevice(), (20, ld))
        out[f"summary{i}"] = _d2h(mf.contactPatchSummaryDevice(), (6, ld))
    return out


@pytest.mark.parametrize("otg,sched,rec,sub,B,ld,two", [(False, False, False, 2, 65, 128, False), (True, False, False, 1, 3, 64, False),
                                                        (False, True, True, 1, 3, 64, False), (True, True, True, 2, 65, 128, False),
                                                        (False, False, False, 2, 65, 128, True), (True, True, True, 1, 3, 64, True)])
def test_rollout_equals_the_host_driven_loop(sp, otg, sched, rec, sub, B, ld, two):
    K = 12
    runs = []
    for host in (False, True):
        if two:
            robot, ctrl, objs, n = _dual(B, ld, otg)
            mfs = objs[:2]
            specs = [(mfs[0], "left_link7", (0, 0, 0.1), SQUARE), (mfs[1], "right_link7", (0, 0, 0.1), np.vstack([SQUARE, 0.5 * SQUARE]))]
        else:
            robot, ctrl, objs = _cfg13(B, ld, otg)
            n, mfs = 7, objs[:1]
            specs = [(mfs[0], EE, EE_POS, SQUARE)]
        buf = _bind_tau(ctrl, n, ld)
        for mf, link, pos, pts in specs:
            mf.attachContactPatch(pts, _floor(robot, link, pos, pts, 2e-3), sensor=True, per_instance=True)
        mf = mfs[0]
        if sched:
            g = mf._get_goal()[:, :3]
            keys = g[None] + np.linspace(0.0, 0.01, 3)[:, None, None] * np.array([1.0, -1.0, 0.0])
            mf.setGoalSchedule((0, 3), keys, stride=4, mode="linear")
        if rec:
            ctrl.recordRollouts(K, 1, ("q", "tau"), task=mf, summaries=True)
        if not host:
            ctrl.rolloutAsync(K, DT, sub, gravity=ZERO_G)
        elif sched or rec:                           # schedules and the recorder act inside rollouts only: one period per call
            for _ in range(K):
                ctrl.rolloutAsync(1, DT, sub, gravity=ZERO_G)
        else:
            for _ in range(K):
                ctrl.contactPatchSense()
                ctrl.stepAsync()
                ctrl.integrate(DT, sub, gravity=ZERO_G)
        out = _final(ctrl, objs, mfs, ld)
        if rec:
            out["log"] = ctrl.rolloutLog()["tau"]
            out["rsum"] = ctrl.rolloutSummary()
        out["tau_buf"] = buf.get()
        out["tau_sim"] = _patch_tau_sim(ctrl, mf, n, ld)
        runs.append(out)
        ctrl._call("saip_batch_contact_patch_detach", -1)
        assert mf.contactPatchTorquesDevice() is None
        ctrl.bindTauDevice(0)
        buf.free()
    a, b = runs
    for key in a:
        assert _same_bits(np.asarray(a[key]), np.asarray(b[key])), key
    for i in range(len(mfs)):
        assert (a[f"summary{i}"][3, :B] >= 1).all()                                  # every instance starts inside the table
        assert two or np.abs(a[f"goal{i}"][:, 30:33]).max() > 1.0                    # the sensor wrote the sensed force (config 13 has the rows)
        assert not a[f"readout{i}"][:, B:].any() and not a[f"summary{i}"][:, B:].any()
    assert np.all(a["tau_buf"][:, B:] == SENTINEL)


# ------------------------------------------------------------------ 4. sensor round trip
def test_sensor_round_trip(sp):
    B, ld = 65, 128
    robot, ctrl, objs = _cfg13(B, ld, False)         # R_cs a rotation about z by 0.4 rad, t_cs = (0.01, -0.02, 0.05)
    mf = objs[0]
    pts = SQUARE + np.array([0.01, 0.02, -0.015])
    with _bind_tau(ctrl, 7, ld):
        mf.attachContactPatch(pts, _floor(robot, EE, EE_POS, pts, 2e-3), sensor=True, per_instance=True)
        ctrl.contactPatchSense()
        ro = mf.contactPatchReadout()
        F, M = -ro["force"], -ro["moment"]
        assert (ro["n_touch"] >= 1).all() and (F[:, 2] < -30.0).all()          # k d = 40 N on the deepest point alone
        assert np.abs(ro["control_point"] - robot.position(EE, tuple(EE_POS))).max() <= 1e-12
        fw, mw = mf.getSensedForceControlWorldFrame(), mf.getSensedMomentControlWorldFrame()
        # the bound of test_gpu_contact.py::test_sensor_round_trip: two rotations there and two back, plus the lever arm t_cs
        assert np.abs(fw - F).max() <= 64 * EPS * np.abs(F).max()
        assert np.abs(mw - M).max() <= 64 * EPS * (np.abs(M).max() + 0.06 * np.abs(F).max())
        assert np.abs(M).max() > 0.1
        mf.detachContactPatch()


# ------------------------------------------------------------------ 5. lifecycle and refusals
def test_lifecycle_and_refusals(sp):
    B, ld, K = 65, 128, 6
    robot, ctrl, objs, n = _dual(B, ld, True)
    left, right, jt = objs
    pl = _floor(robot, "left_link7", (0, 0, 0.1), SQUARE, 2e-3)
    pr = _floor(robot, "right_link7", (0, 0, 0.1), SQUARE[:3], 2e-3)      # the right patch gets three of the corners
    assert not hasattr(jt, "attachContactPatch")
    with pytest.raises(ValueError, match="not a motion-force task"):
        ctrl._call("saip_batch_contact_patch_attach", jt._id, 4, _dp(SQUARE), 1, _dp(np.ascontiguousarray(pl.transpose(0, 2, 1))), 1, 1)
    for bad_n in (np.zeros((0, 3)), np.zeros((9, 3))):
        with pytest.raises(ValueError, match="points required"):
            left.attachContactPatch(bad_n, pl, per_instance=True)
    with pytest.raises(ValueError, match="not finite"):
        left.attachContactPatch([[0.0, np.inf, 0.0]], pl, per_instance=True)
    with pytest.raises(ValueError, match="planes required"):
        left.attachContactPatch(SQUARE, np.tile(pl, (5, 1, 1)), per_instance=True)
    with pytest.raises(ValueError, match="k > 0"):
        bad = pl.copy()
        bad[0, B - 1, 4] = 0.0
        left.attachContactPatch(SQUARE, bad, per_instance=True)
    left.attachContactPatch(SQUARE, pl, sensor=True, per_instance=True)
    with pytest.raises(sp.SaipError, match="already carries a contact patch"):
        left.attachContactPatch(SQUARE, pl, sensor=True, per_instance=True)
    with pytest.raises(sp.SaipError, match="a contact patch is attached"):           # mutual exclusion, patch first
        right.attachContactPlanes(pr, sensor=True, per_instance=True)
    with pytest.raises(sp.SaipError, match="written by the simulated sensor"):       # the schedule-row conflict, patch first
        left.setGoalSchedule("sensed_force", np.zeros((2, 3)))
    right.setGoalSchedule("sensed_force", np.zeros((2, 3)))                          # the other task has no sensor yet
    with pytest.raises(sp.SaipError, match="covers sensed-wrench rows"):             # ... schedule first
        right.attachContactPatch(SQUARE, pr, sensor=True, per_instance=True)
    right.attachContactPatch(SQUARE[:3], pr, sensor=False, per_instance=True)        # without the sensor: fine
    right.clearGoalSchedule()
    with pytest.raises(sp.SaipError, match="patches are attached already"):              # a third patch
        left.attachContactPatch(SQUARE, pl, sensor=False, per_instance=True)
    il, ir = left.contactPatchInfo(), right.contactPatchInfo()
    assert (il["n_patches"], il["n_points"], il["sensor"], ir["n_points"], ir["sensor"]) == (2, 4, True, 3, False)
    assert np.array_equal(il["points"], SQUARE) and np.array_equal(ir["points"], SQUARE[:3])
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    sl, sr = left.contactPatchSummary(), right.contactPatchSummary()
    for s in (sl, sr):
        assert (s["substeps_in_contact"] >= 1).all() and (s["impulse"] > 0).all() and (s["max_penetration"] >= 2e-3 * (1 - 1e-9)).all()
        assert (s["substeps_in_full_contact"] <= s["substeps_in_contact"]).all() and (s["max_force"] > 0).all()
    left.resetContactPatchSummary()
    assert not left.contactPatchSummary()["impulse"].any() and right.contactPatchSummary()["impulse"].all()
    lower = pl.copy()
    lower[0, :, 3] -= 0.5                                            # the left table far below: nothing touches from the next period on
    left.setContactPatchPlanes(lower)
    ctrl.rolloutAsync(2, DT, SUB, gravity=ZERO_G)
    s2 = left.contactPatchSummary()
    assert not s2["substeps_in_contact"].any() and not s2["impulse"].any() and not s2["max_force"].any() and not s2["max_moment"].any()
    assert not left.contactPatchReadout()["n_touch"].any()
    # detaching one of two: the other stays, and moves to the front
    left.detachContactPatch()
    assert left.contactPatchPlanesDevice() is None and right.contactPatchPlanesDevice() is not None
    assert right.contactPatchInfo()["n_patches"] == 1
    with pytest.raises(sp.SaipError, match="carries no contact patch"):
        left.contactPatchReadout()
    with pytest.raises(sp.SaipError, match="no contact patch was attached with the simulated sensor"):
        ctrl.contactPatchSense()
    before = right.contactPatchSummary()
    ctrl.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
    after = right.contactPatchSummary()
    assert (after["impulse"] >= before["impulse"]).all() and (after["substeps_in_contact"] >= before["substeps_in_contact"]).all()
    right.detachContactPatch()
    assert right.contactPatchTorquesDevice() is None
    with pytest.raises(sp.SaipError, match="no contact patch is attached"):
        right.contactPatchReadout()
    # mutual exclusion, single point first
    left.attachContactPlanes(pl, sensor=True, per_instance=True)
    with pytest.raises(sp.SaipError, match="single-point contact planes are attached"):
        right.attachContactPatch(SQUARE, pr, per_instance=True)
    left.detachContactPlanes()
    # attach, detach, then a rollout: the bits of a batch that never had a patch
    ends = []
    for touched in (False, True):
        robot2, ctrl2, objs2, _ = _dual(B, ld, True)
        if touched:
            objs2[0].attachContactPatch(SQUARE, pl, sensor=True, per_instance=True)
            objs2[1].attachContactPatch(SQUARE, pr, sensor=True, per_instance=True)
            ctrl2._call("saip_batch_contact_patch_detach", -1)
        ctrl2.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        ctrl2.synchronize()
        q, dq = ctrl2.pullState()
        ends.append((q.copy(), dq.copy(), ctrl2.getTorques(), ctrl2.kernelName()))
    assert all(_same_bits(x, y) for x, y in zip(ends[0][:3], ends[1][:3])) and ends[0][3] == ends[1][3]


# ------------------------------------------------------------------ 6. surface alignment
def _tilted_table(robot, depth, k=2.0e4, c=400.0, mu=0.3, tilt_deg=3.0, pts=SQUARE):
    """per-instance table facing the plate (the control frame's x-y plane, pressed along +z_c), tilted about the in-plane axis x_c, the
    deepest edge `depth` inside.  Returns planes (1, B, 8), the table normal n (B, 3), x_c's and z_c's world directions"""
    B = robot.batch_size
    o = robot.position(EE, tuple(EE_POS))
    ex, ey, ez = (robot.position(EE, tuple(EE_POS + e)) - o for e in np.eye(3))      # the control frame's axes in the world
    a = np.deg2rad(tilt_deg)
    nrm = -(np.cos(a) * ez + np.sin(a) * ey)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    p = np.stack([robot.position(EE, tuple(EE_POS + r)) for r in pts])
    planes = np.zeros((1, B, 8))
    planes[0] = [0, 0, 0, 0, k, c, mu, 1e-3]
    planes[0, :, :3] = nrm
    planes[0, :, 3] = np.einsum("be,ibe->ib", nrm, p).min(axis=0) + depth
    return planes, nrm, ex, ey, ez


def test_surface_alignment(sp):
    """A square plate pressed on a table tilted by 3 degrees, config 13's force and moment loops closed on the simulated sensor.

    Asserted: the sensed moment about the tilt axis at the first SENSE is non-zero with the sign of r x F of the touching edge (a single
    point at the centre reports exactly 0), the rollout stays finite, and the angle between plate and table normal is smaller than at the
    start in every instance.  The final angle, the spread of the four normal forces and the share in full contact are printed."""
    B, ld = 65, 128
    robot, ctrl, objs = _cfg13(B, ld, False, goal_force=(0.0, 0.0, 5.0))             # compliant-frame axis z_c: press along the plate normal
    mf = objs[0]
    planes, nrm, ex, ey, ez = _tilted_table(robot, 1e-4)
    angle0 = np.degrees(np.arccos(np.clip(np.einsum("be,be->b", ez, -nrm), -1, 1)))
    assert np.abs(angle0 - 3.0).max() < 1e-6
    mf.attachContactPatch(SQUARE, planes, sensor=True, per_instance=True)
    ctrl.contactPatchSense()
    ro = mf.contactPatchReadout()
    assert (ro["n_touch"] == 2).all() and np.isin(ro["deepest"], (0, 1)).all()       # the +y_c edge: points 0 and 1
    mw = mf.getSensedMomentControlWorldFrame()
    edge = 0.05 * ey                                                                 # the middle of the touching edge from the control point
    want = np.einsum("be,be->b", np.cross(edge, -ro["force"]), ex)                   # r x F about the tilt axis, F the force on the table
    got = np.einsum("be,be->b", mw, ex)
    print("sensed moment about the tilt axis: min/max", got.min(), got.max(), "r x F", want.min(), want.max())
    assert (got != 0).all() and (np.sign(got) == np.sign(want)).all() and (want > 0).all()
    assert np.abs(mf._get_goal()[:, 33:36]).max(axis=1).min() > 0                    # MS itself, in the sensor frame
    # one point at the centre, pressed in until it touches: a force, and exactly no moment
    mf.detachContactPatch()
    centre, _, _, _, _ = _tilted_table(robot, 1e-4, pts=np.zeros((1, 3)))
    mf.attachContactPatch(np.zeros((1, 3)), centre, sensor=True, per_instance=True)
    ctrl.contactPatchSense()
    one = mf.contactPatchReadout()
    assert (one["n_touch"] == 1).all() and (np.abs(one["force"]).max(axis=1) > 0).all() and not one["moment"].any()
    # the same contrast where the moment loop reads it: M is exactly 0, so what comes back through the sensor frame (t_cs is not zero)
    # is the round trip's rounding alone, the bound of test_sensor_round_trip with M = 0
    got1 = np.einsum("be,be->b", mf.getSensedMomentControlWorldFrame(), ex)
    print("one point at the centre, sensed moment about the tilt axis: max |.|", np.abs(got1).max(), "patch: min |.|", np.abs(got).min())
    assert np.abs(got1).max() <= 64 * EPS * 0.06 * np.abs(one["force"]).max()
    assert np.abs(got).min() > 1e6 * np.abs(got1).max()
    mf.detachContactPatch()
    mf.attachContactPatch(SQUARE, planes, sensor=True, per_instance=True)
    ctrl.rolloutAsync(400, DT, SUB, gravity=ZERO_G)
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    ro, sm = mf.contactPatchReadout(), mf.contactPatchSummary()
    assert all(np.isfinite(a).all() for a in (q, dq, ctrl.getTorques(), ro["force"], ro["moment"], sm["impulse"], sm["max_moment"]))
    assert not ctrl.status.any()
    robot.setQ(q)
    robot.updateModel()
    o = robot.position(EE, tuple(EE_POS))
    ez1 = robot.position(EE, tuple(EE_POS + np.array([0.0, 0.0, 1.0]))) - o
    angle1 = np.degrees(np.arccos(np.clip(np.einsum("be,be->b", ez1, -nrm), -1, 1)))
    fn = ro["normal_forces"][:, :4]
    spread = (fn.max(axis=1) - fn.min(axis=1)) / np.maximum(fn.sum(axis=1), 1e-300)
    print(f"tilt after 400 periods: min {angle1.min():.4f} median {np.median(angle1):.4f} max {angle1.max():.4f} deg (start 3.0000)")
    print(f"normal-force spread (max - min) / sum: median {np.median(spread):.3f} max {spread.max():.3f}; net force median {np.median(fn.sum(axis=1)):.3f} N")
    print(f"full contact at the end: {(ro['n_touch'] == 4).mean():.3f} of the instances; n_touch counts {np.bincount(ro['n_touch'], minlength=5)}")
    assert (angle1 < angle0).all(), (angle1.max(), int((angle1 >= angle0).sum()))
    mf.detachContactPatch()
