"""The resident inertia table of the simulator on the device (csrc/saip_inertia.hip, the INERTIA instantiations of csrc/saip_dynamics.hip and
csrc/saip_dynamics_oct.hip, saip_batch_inertia_*).  Oracles: the Lagrangian restatement oracle/restatement.forward_dynamics on a robot
description of its own per instance (tests/inertia_ref.instance_description: link by link, nothing of the engine's merging repeated), the
NumPy restatement tests/inertia_ref.py of the composition and of the draw (bit for bit), the unattached integrator for the neutral table,
and the host-driven loop for whole rollouts.

Neutral table, measured on the MI355X (test_neutral_table_changes_nothing prints it): worst relative difference of q and dq 0.0 on the
Panda and on chain30 (NEUTRAL_MEASURED below)."""
import contextlib

import numpy as np
import pytest

import inertia_ref as IR
import trees as TR
import workloads as W
import restatement as RS
from test_gpu_batch_layout import _d2h, _same_bits

pytestmark = pytest.mark.gpu

DT, SUB = 5e-4, 2
ZERO_G = (0.0, 0.0, 0.0)
SETTINGS = [((0.0, 0.0, -9.81), 0.0), ((0.0, 0.0, 0.0), 0.3)]           # test_gpu_dynamics.py's: gravity on without damping, off with 0.3
# worst relative difference of q and dq between the neutral table and no table (integrate and a 5-period rollout, Panda and chain30) as
# measured on the MI355X: 0, the two instantiations gave the same bits in every case.  The assertion is 100 x this figure and never more than
# NEUTRAL_CAP (1e-9, three orders under the oracle tolerance): with the figure at 0 that is equality.
NEUTRAL_MEASURED = 0.0
NEUTRAL_CAP = 1e-9


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


@contextlib.contextmanager
def _oracle(tree):
    """the Lagrangian oracle (over trees when asked) with mass_matrix remembered per (model, state): forward_dynamics differentiates the
    same matrices again for every gravity / damping setting"""
    with (TR.tree_oracle() if tree else contextlib.nullcontext(RS)) as rs:
        inner, memo = rs.mass_matrix, {}

        def cached(model, frames):
            key = (id(model), b"".join(R.tobytes() + o.tobytes() for R, o in frames))
            if key not in memo:
                memo[key] = inner(model, frames)
            return memo[key]
        rs.mass_matrix = cached
        try:
            yield rs
        finally:
            rs.mass_matrix = inner


def _parts(rng, n, P, B, per_instance=True):
    """s in [0.8, 1.2], |d| <= 0.02, payloads of 0..3 kg (every third instance carries nothing in payload 0)"""
    sb, spay = ((n, B) if per_instance else (n,)), ((P, B) if per_instance else (P,))
    bodies = np.concatenate([rng.uniform(0.8, 1.2, sb + (1,)), rng.uniform(-0.02, 0.02, sb + (3,))], axis=-1)
    pay = np.concatenate([rng.uniform(0.0, 3.0, spay + (1,)), rng.uniform(-0.05, 0.05, spay + (3,)), rng.uniform(0.01, 0.08, spay + (3,))], axis=-1)
    if per_instance and P:
        pay[0, ::3, 0] = 0.0
    return bodies, pay


def _case(name):
    """(description, model, task specs, is a tree, payload sites)"""
    if name.startswith("random"):
        s, n = {"random11_4": (11, 4), "random12_9": (12, 9)}[name]
        desc = TR.random_tree(s, n)
        m = W.RobotModel(desc)
        movable = [l["name"] for l in desc["links"] if l["joint_type"] != "fixed"]
        fixed = [l["name"] for l, b in zip(desc["links"], IR.link_frames(desc["links"], TR.parent_index(m))) if l["joint_type"] == "fixed" and b[0] >= 0]
        return desc, m, [W.joint_task("posture")], True, [movable[-1]] + fixed[:1]
    d = W.make_inputs({"panda_arm": 2, "panda_sliding_base": 6, "chain30": 5}[name], 4)
    m = d["model"]
    sites = {"panda_arm": ["end-effector", "link4"], "panda_sliding_base": ["end-effector", "link0"], "chain30": [m.link_names[-1], m.link_names[3]]}[name]
    return dict(name=m.name, links=m.links), m, d["tasks"], False, sites


def _engine(desc, specs, B, ld=None, **kw):
    from sai_primitives_amd.controller import controller_from_specs
    return controller_from_specs(desc, specs, B, device=0, leading_dimension=ld, **kw)


def _state(rng, m, B):
    q = np.clip(rng.uniform(-1.2, 1.2, (B, m.dof)), m.q_lower + 0.1, m.q_upper - 0.1)
    return q, rng.uniform(-1.0, 1.0, (B, m.dof)), rng.uniform(-5, 5, (B, m.dof))


def _rel(a, b):
    """per instance: max |a - b| over the joints, against max(1, max |b|) over the batch (the scale of test_gpu_dynamics.py)"""
    return np.abs(a - b).max(axis=1) / max(1.0, np.abs(b).max())


def _one_step(robot, ctrl, q, dq, tau, grav, damping, dt=1e-4):
    ctrl.setTorques(tau)
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.integrate(dt, 1, gravity=grav, damping=damping)
    ctrl.synchronize()
    q1, dq1 = ctrl.pullState()
    assert np.abs(q1 - (q + dt * dq1)).max() < 1e-15
    return (dq1 - dq) / dt


# ------------------------------------------------------------------ 1. one step against the Lagrangian oracle, a robot per instance
# eight-lane kernel: two groups of eight, the second ragged, and a padded leading dimension; lane kernels NMAX 8 (a prismatic joint, across a
# 64-thread block) and 32; the tree kernels, NMAX 8 and 32
@pytest.mark.parametrize("name,B,ld", [("panda_arm", 13, None), ("panda_arm", 70, 128), ("panda_sliding_base", 65, None), ("chain30", 9, None),
                                       ("random11_4", 65, None), ("random12_9", 65, None)])
def test_one_step_matches_the_oracle_of_every_instance(sp, name, B, ld):
    desc, m, specs, tree, sites = _case(name)
    parents = TR.parent_index(m) if tree else None
    rng = np.random.default_rng(4)
    q, dq, tau = _state(rng, m, B)
    bodies, pay = _parts(rng, m.dof, len(sites), B)
    robot, ctrl, _ = _engine(desc, specs, B, ld)
    ctrl.attachInertia(per_instance=True, payload_links=sites)
    ctrl.setInertiaParts(bodies, pay)
    with _oracle(tree) as rs:
        models = [W.RobotModel(IR.instance_description(desc, bodies[:, i], pay[:, i], sites, parents)) for i in range(B)]
        for grav, damping in SETTINGS:
            qdd = _one_step(robot, ctrl, q, dq, tau, grav, damping)
            ref = np.concatenate([rs.forward_dynamics(models[i], q[i:i + 1], dq[i:i + 1], tau[i:i + 1], g=grav, damping=damping) for i in range(B)])
            err = np.abs(qdd - ref).max() / max(1.0, np.abs(ref).max())
            print(name, B, "gravity", grav, "max rel qdd error", err)
            assert err < 1e-8
    ctrl.detachInertia()


def test_one_step_with_a_batch_uniform_table(sp):
    desc, m, specs, tree, sites = _case("panda_arm")
    B = 13
    rng = np.random.default_rng(4)
    q, dq, tau = _state(rng, m, B)
    bodies, pay = _parts(rng, m.dof, len(sites), B, per_instance=False)
    robot, ctrl, _ = _engine(desc, specs, B)
    ctrl.attachInertia(payload_links=sites)
    ctrl.setInertiaParts(bodies, pay)
    assert ctrl.inertiaRows().shape == (7, 10)
    model = W.RobotModel(IR.instance_description(desc, bodies, pay, sites))
    for grav, damping in SETTINGS:
        qdd = _one_step(robot, ctrl, q, dq, tau, grav, damping)
        ref = RS.forward_dynamics(model, q, dq, tau, g=grav, damping=damping)
        err = np.abs(qdd - ref).max() / max(1.0, np.abs(ref).max())
        print("batch-uniform table, gravity", grav, "max rel qdd error", err)
        assert err < 1e-8


# ------------------------------------------------------------------ 2. the table is used
def test_a_payload_in_the_hand_changes_the_acceleration(sp):
    """config 2's inputs (B = 13, seed 4 as in test_gpu_dynamics.py) with a 2 kg box of half-extents 0.05 at (0, 0, 0.1) of the
    end-effector: the oracle with the payload is 2.9e-2 .. 1.2e-1 (relative, per instance) away from the oracle without, computed on
    the CPU for these inputs; the device follows the oracle with the payload"""
    B = 13
    d = W.make_inputs(2, B)
    model = d["model"]
    desc = dict(name=model.name, links=model.links)
    rng = np.random.default_rng(4)
    tau = rng.uniform(-5, 5, (B, 7))
    dq = rng.uniform(-1.0, 1.0, (B, 7))
    pay = np.array([[2.0, 0.0, 0.0, 0.1, 0.05, 0.05, 0.05]])
    robot, ctrl, _ = _engine(model.name, d["tasks"], B)
    ctrl.attachInertia(payload_links=["end-effector"])
    ctrl.setInertiaParts(None, pay)
    loaded = W.RobotModel(IR.instance_description(desc, IR.neutral_bodies(7), pay, ["end-effector"]))
    grav, damping = SETTINGS[0]
    qdd = _one_step(robot, ctrl, d["q"], dq, tau, grav, damping)
    ref = RS.forward_dynamics(loaded, d["q"], dq, tau, g=grav, damping=damping)
    bare = RS.forward_dynamics(model, d["q"], dq, tau, g=grav, damping=damping)
    apart = _rel(bare, ref)
    err = np.abs(qdd - ref).max() / max(1.0, np.abs(ref).max())
    print("payload oracle against bare oracle, per instance:", apart.min(), "..", apart.max(), "| device against the payload oracle", err)
    assert (apart > 1e-3).all()
    assert err < 1e-8
    ctrl.detachInertia()
    qdd0 = _one_step(robot, ctrl, d["q"], dq, tau, grav, damping)
    assert np.abs(qdd0 - bare).max() / max(1.0, np.abs(bare).max()) < 1e-8          # detached: the model's robot again


# ------------------------------------------------------------------ 3. the neutral table
def _cfg(name, B, otg, ld=None):
    d = W.make_inputs({"panda_arm": 2, "chain30": 5}[name], B)
    robot, ctrl, objs = _engine(d["model"].name, d["tasks"], B, ld, disable_otg=not otg)
    robot.setQ(d["q"])
    robot.setDq(0.2 * d["dq"])
    robot.updateModel()
    ctrl.reinitializeTasks()
    ctrl.updateControllerTaskModels()
    return robot, ctrl, objs, d


@pytest.mark.parametrize("name,B", [("panda_arm", 65), ("chain30", 9)])
def test_neutral_table_changes_nothing(sp, name, B):
    """attached with the model's own rows: integrate and a 5-period rollout against the same calls unattached (on the Panda the
    unattached rollout takes the fused launches, the attached one does not).  Not bit for bit: the compiler may contract the two
    instantiations differently."""
    worst = 0.0
    for otg in (False, True):
        ends = []
        for attached in (False, True):
            robot, ctrl, objs, d = _cfg(name, B, otg)
            if attached:
                ctrl.attachInertia()
            tau = np.random.default_rng(3).uniform(-5, 5, (B, d["model"].dof))
            ctrl.setTorques(tau)
            ctrl.integrate(DT, 2)
            a = tuple(x.copy() for x in ctrl.pullState())
            ctrl.updateControllerTaskModels()
            ctrl.rolloutAsync(5, DT, SUB)
            ctrl.synchronize()
            ends.append(a + tuple(x.copy() for x in ctrl.pullState()))
        for x, y in zip(*ends):
            worst = max(worst, np.abs(x - y).max() / max(1.0, np.abs(x).max()))
        assert np.abs(ends[0][3]).max() > 1e-3
    bound = NEUTRAL_CAP if NEUTRAL_MEASURED is None else min(NEUTRAL_CAP, 100 * NEUTRAL_MEASURED)
    print(name, "neutral table: worst relative difference of q and dq", worst, "| bound", bound)
    assert worst <= bound


# ------------------------------------------------------------------ 4. the composition kernel against the restatement
def _sites(ctrl):
    info = ctrl.inertiaInfo()
    return info["payload_bodies"], info["payload_positions"], info["payload_rotations"]


@pytest.mark.parametrize("name,B,ld", [("panda_arm", 70, 128), ("panda_arm", 300, None), ("random12_9", 65, None)])
def test_composition_equals_the_restatement_bit_for_bit(sp, name, B, ld):
    desc, m, specs, tree, sites = _case(name)
    n, P = m.dof, len(sites)
    robot, ctrl, _ = _engine(desc, specs, B, ld)
    ctrl.attachInertia()
    rows0 = ctrl.inertiaRows()                                           # the model's own rows, as the device holds them
    ctrl.detachInertia()
    assert np.abs(rows0 - IR.model_rows(desc["links"], TR.parent_index(m) if tree else None)).max() < 1e-14
    ctrl.attachInertia(per_instance=True, payload_links=sites)
    assert _same_bits(ctrl.inertiaRows(), np.ascontiguousarray(np.broadcast_to(rows0[:, None, :], (n, B, 10))))
    where = _sites(ctrl)
    frames = IR.link_frames(desc["links"], TR.parent_index(m) if tree else None)
    for p, s in enumerate(sites):
        body, R, pos = frames[m.link_index(s)]
        assert where[0][p] == body and np.abs(where[1][p] - pos).max() < 1e-15 and np.abs(where[2][p] - R).max() < 1e-15
    rng = np.random.default_rng(8)
    bodies, pay = _parts(rng, n, P, B)
    # from tables: per instance, batch-uniform, and each alone
    for bt, pt in ((bodies, pay), (bodies[:, 0], pay[:, 0]), (bodies, None), (None, pay)):
        ctrl.setInertiaParts(bt, pt)
        want = IR.compose(rows0, IR.neutral_bodies(n) if bt is None else bt, np.zeros((P, 7)) if pt is None else pt, *where, B)
        assert _same_bits(ctrl.inertiaRows(), want)
    ctrl.setInertiaParts()
    assert _same_bits(ctrl.inertiaRows(), np.ascontiguousarray(np.broadcast_to(rows0[:, None, :], (n, B, 10))))     # neutral parts: the model's words
    # from the draw
    bl, bh = IR.neutral_bodies(n), IR.neutral_bodies(n)
    bl[:, 0], bh[:, 0], bl[:, 1:], bh[:, 1:] = 0.8, 1.2, -0.02, 0.02
    bh[::2, 2] = bl[::2, 2]
    pl, ph = np.zeros((P, 7)), np.tile([3.0, 0.05, 0.05, 0.05, 0.08, 0.08, 0.08], (P, 1))
    ph[0, 5] = pl[0, 5] = 0.05
    seed, rnd = 0x9E3779B97F4A7C15, 7
    for bb, pb in (((bl, bh), (pl, ph)), ((bl, bh), None), (None, (pl, ph))):
        ctrl.randomizeInertia(seed, rnd, bodies=bb, payloads=pb)
        want, db, dp = IR.randomized(rows0, seed, rnd, B, bb, pb, *where)
        got = ctrl.inertiaRows()
        assert _same_bits(got, want)
    assert len(np.unique(got[where[0][0], :, 0])) == B                    # every instance its own payload
    ctrl.synchronize()
    ldim = ld or (B + 31) // 32 * 32
    raw = _d2h(ctrl.inertiaRowsDevice(), (n * 10, ldim))
    assert not raw[:, B:].any()                                          # columns B.. are never written (zero since the attach)
    # read-back equals what was set
    rows = np.ascontiguousarray(got[:, ::-1])
    ctrl.setInertiaRows(rows)
    assert _same_bits(ctrl.inertiaRows(), rows)
    ctrl.detachInertia()


def test_columns_do_not_depend_on_the_batch_size(sp):
    desc, m, specs, tree, sites = _case("panda_arm")
    out = []
    for B in (70, 300):
        robot, ctrl, _ = _engine(desc, specs, B)
        ctrl.attachInertia(per_instance=True, payload_links=sites)
        lo, hi = np.tile([0.8, -0.02, -0.02, -0.02], (7, 1)), np.tile([1.2, 0.02, 0.02, 0.02], (7, 1))
        ctrl.randomizeInertia(11, 2, bodies=(lo, hi), payloads=(np.zeros((2, 7)), np.tile([3.0, 0.05, 0.05, 0.05, 0.08, 0.08, 0.08], (2, 1))))
        out.append(ctrl.inertiaRows())
    assert _same_bits(np.ascontiguousarray(out[0]), np.ascontiguousarray(out[1][:, :70]))


def test_refusals_with_an_attachment(sp):
    desc, m, specs, tree, sites = _case("panda_arm")
    B = 5
    robot, ctrl, _ = _engine(desc, specs, B)
    ctrl.attachInertia(per_instance=True, payload_links=sites)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachInertia()
    before = ctrl.inertiaRows()
    nb, zp = IR.neutral_bodies(7), np.zeros((2, 7))
    perb, perp = np.repeat(nb[:, None, :], B, axis=1), np.repeat(zp[:, None, :], B, axis=1)
    for j, k, val, msg in [(2, 0, 0.0, "body 2 of instance 4: word s = 0 must be positive"), (3, 0, -1.0, "body 3 of instance 4: word s = -1 must be positive"),
                           (1, 2, np.nan, "body 1 of instance 4: word dy is not finite")]:
        t = perb.copy()
        t[j, B - 1, k] = val
        with pytest.raises(ValueError, match=msg):
            ctrl.setInertiaParts(t, perp)
    for p, k, val, msg in [(0, 0, -0.5, "payload 0 of instance 1: word m_p = -0.5 is below 0"), (1, 5, -1e-3, "payload 1 of instance 1: word hy = -0.001 is below 0"),
                           (1, 2, np.inf, r"payload 1 of instance 1: word c_p\[1\] is not finite")]:
        t = perp.copy()
        t[p, 1, k] = val
        with pytest.raises(ValueError, match=msg):
            ctrl.setInertiaParts(perb, t)
    bad = nb.copy()
    bad[4, 0] = 0.0
    with pytest.raises(ValueError, match="upper bound: body 4: word s = 0 must be positive"):
        ctrl.randomizeInertia(1, bodies=(nb, bad))
    bad = zp.copy()
    bad[1, 0] = -1.0
    with pytest.raises(ValueError, match="lower bound: payload 1: word m_p = -1 is below 0"):
        ctrl.randomizeInertia(1, payloads=(bad, zp))
    with pytest.raises(ValueError, match="nothing to draw"):
        ctrl.randomizeInertia(1)
    rows = before.copy()
    rows[5, 2, 4:7] = (-1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="body 5 of instance 2: words Ixx..Iyz"):
        ctrl.setInertiaRows(rows)
    assert _same_bits(ctrl.inertiaRows(), before)                        # nothing was written by any of them
    ctrl.detachInertia()
    ctrl.attachInertia(payload_links=sites)                              # batch-uniform: no draw, no per-instance parts
    with pytest.raises(ValueError, match="the table is batch-uniform"):
        ctrl.randomizeInertia(1, bodies=(nb, nb))
    with pytest.raises(ValueError, match="per-instance parts on a batch-uniform table"):
        ctrl.setInertiaParts(perb)
    ctrl.detachInertia()


# ------------------------------------------------------------------ 5. the engine around the table
def _attach_varied(ctrl, B, seed=21):
    rng = np.random.default_rng(seed)
    bodies, pay = _parts(rng, 7, 2, B)
    ctrl.attachInertia(per_instance=True, payload_links=["end-effector", "link4"])
    ctrl.setInertiaParts(bodies, pay)


def _final(ctrl, objs):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float), goals=[t._get_goal() for t in objs])


def _same(a, b):
    for key in a:
        if key == "goals":
            assert all(_same_bits(x, y) for x, y in zip(a[key], b[key]))
        else:
            assert _same_bits(np.asarray(a[key]), np.asarray(b[key])), key


@pytest.mark.parametrize("otg", [False, True])
def test_rollout_equals_the_host_driven_loop(sp, otg):
    B, K = 65, 6
    runs = []
    for host in (False, True):
        robot, ctrl, objs, d = _cfg("panda_arm", B, otg, 128)
        _attach_varied(ctrl, B)
        if host:
            for _ in range(K):
                ctrl.stepAsync()
                ctrl.integrate(DT, SUB, gravity=ZERO_G)
        else:
            ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        runs.append(_final(ctrl, objs))
    _same(*runs)
    # and the table was felt: the same rollout without it ends elsewhere
    robot, ctrl, objs, d = _cfg("panda_arm", B, otg, 128)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    assert np.abs(_final(ctrl, objs)["dq"] - runs[0]["dq"]).max() > 1e-4


def test_table_survives_snapshots(sp):
    B, K = 65, 4
    robot, ctrl, objs, d = _cfg("panda_arm", B, True)
    plain = ctrl.saveState()
    layout, nbytes = plain.segments(), plain.nbytes()
    _attach_varied(ctrl, B)
    rows = ctrl.inertiaRows()
    snap = ctrl.saveState()
    assert snap.segments() == layout and snap.nbytes() == nbytes         # the table is configuration: not part of a snapshot
    ends = []
    for _ in range(2):
        ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        ends.append(_final(ctrl, objs))
        ctrl.restoreState(snap)
        assert _same_bits(ctrl.inertiaRows(), rows)
    _same(*ends)
    # instance 0's state into all: every instance still integrates its own robot
    ctrl.restoreState(snap, 0)
    assert _same_bits(ctrl.inertiaRows(), rows)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    out = _final(ctrl, objs)
    assert _same_bits(out["q"][0], ends[0]["q"][0]) and np.abs(out["dq"] - out["dq"][0]).max(axis=1)[1:].min() > 0
    ctrl.detachInertia()


def test_table_composes_with_the_plant_and_contact_planes(sp):
    """with a plant model and contact planes attached as well, one integrate is { plant, contact APPLY, integrate with the table }: the
    plain integrator with the table, fed the torques the contact launch left on the device, gives the same bits"""
    from test_gpu_plant import _attach_rough, _table_under
    B, ld = 65, 128
    robot, ctrl, objs, d = _cfg("panda_arm", B, False, ld)
    mf = objs[0]
    ctrl.setTorques(np.random.default_rng(2).uniform(-20, 20, (B, 7)))
    q0, dq0 = robot._q.copy(), robot._dq.copy()
    _attach_varied(ctrl, B)
    _attach_rough(ctrl, d, B)
    mf.attachContactPlanes(_table_under(robot, 2e-3), sensor=False, per_instance=True)
    ctrl.integrate(DT, SUB, gravity=ZERO_G)
    ctrl.synchronize()
    q1, dq1 = (a.copy() for a in ctrl.pullState())
    mf.detachContactPlanes()
    ctrl.detachPlant()
    # the manual sequence: the same two substeps, one at a time, each with its own plant and contact launch
    robot.setQ(q0)
    robot.setDq(dq0)
    _attach_rough(ctrl, d, B)
    mf.attachContactPlanes(_table_under(robot, 2e-3), sensor=False, per_instance=True)
    sims = []
    for _ in range(SUB):
        ctrl.integrate(DT, 1, gravity=ZERO_G)
        ctrl.synchronize()
        sims.append(_d2h(mf.contactTorquesDevice(), (7, ld))[:, :B].T.copy())
        ctrl.setPlantPeriod(0)                                           # both substeps belong to the first period
    q2, dq2 = (a.copy() for a in ctrl.pullState())
    assert _same_bits(q1, q2) and _same_bits(dq1, dq2)
    mf.detachContactPlanes()
    ctrl.detachPlant()
    # ... and with nothing but the table attached, fed those torques
    robot.setQ(q0)
    robot.setDq(dq0)
    for s in sims:
        ctrl.setTorques(s)
        ctrl.integrate(DT, 1, gravity=ZERO_G)
    q3, dq3 = (a.copy() for a in ctrl.pullState())
    assert _same_bits(q1, q3) and _same_bits(dq1, dq3)
    # without the table the same torques move the arm elsewhere
    ctrl.detachInertia()
    robot.setQ(q0)
    robot.setDq(dq0)
    for s in sims:
        ctrl.setTorques(s)
        ctrl.integrate(DT, 1, gravity=ZERO_G)
    assert np.abs(ctrl.pullState()[1] - dq1).max() > 1e-6


@pytest.mark.parametrize("otg", [False, True])
def test_detach_restores_the_launch_sequence_and_the_torques_never_see_the_table(sp, otg):
    B, K = 65, 6
    ends = []
    for touched in (False, True):
        robot, ctrl, objs, d = _cfg("panda_arm", B, otg, 128)
        if touched:
            _attach_varied(ctrl, B)
        tau = np.asarray(ctrl.computeControlTorques(), float).copy()    # the cycle path keeps the model: the same bits, attached or not
        if touched:
            ctrl.detachInertia()
            assert ctrl.inertiaRowsDevice() is None
        ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        out = _final(ctrl, objs)
        out["first_tau"] = tau
        out["kernel"] = np.frombuffer(ctrl.kernelName().encode().ljust(16), np.uint8).astype(float)
        ends.append(out)
    _same(*ends)
    robot3, ctrl3, objs3, d3 = _cfg("panda_arm", B, otg)
    _attach_varied(ctrl3, B)
    ctrl3.rolloutAsync(2, DT, SUB, gravity=ZERO_G)
    ctrl3._release()                                                     # destroy while attached, a rollout in flight
