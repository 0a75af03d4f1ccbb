"""Link contact, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument and call-order errors come back
with the documented codes before the device is needed; the Python facade raises the same; the host build of csrc/saip_link_contact.h
(tests/cpp/link_contact_host.cpp, also under ASan/UBSan) matches the NumPy restatement tests/link_contact_ref.py bit for bit in tau_sim,
the readout, the sphere forces, the summaries and the cost; the restatement's force law has the properties of a contact force."""
import copy
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import link_contact_ref as LC
import trees as TR
import workloads as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_link_contact_" + n for n in ("attach", "detach", "info", "set_obstacles_host", "set_materials_host", "evaluate", "readout_host",
                                                           "summary_host", "summary_reset", "add_cost")]
POINTER_ENTRIES = ["saip_batch_link_contact_" + n + "_device" for n in ("torques", "obstacles", "readout", "summary", "keep")]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    src = open(os.path.join(PKG, "csrc", "saip_link_contact.h")).read()
    for name, val in [("MAX_SPHERES", 32), ("MAX_OBSTACLES", 16), ("OBSTACLE_WORDS", 8), ("MATERIAL_WORDS", 4), ("READOUT_ROWS", 8), ("SUMMARY_ROWS", 4)]:
        assert re.search(rf"#define SAIP_LINK_CONTACT_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_LINK_CONTACT_" + name) == val == getattr(LC, name)
        m = re.search(rf"LINK_CONTACT_{name} = (\w+)", src)
        assert m and (m.group(1) == str(val) or getattr(capi, "SAIP_" + m.group(1)) == val), name     # a number, or the clearance monitor's constant
    assert re.search(r"LINK_CONTACT_LANES = CLEARANCE_LANES", src) and LC.LANES == 8
    assert re.search(r"LINK_CONTACT_EVALUATE = 0, LINK_CONTACT_APPLY = 1", src) and (LC.EVALUATE, LC.APPLY) == (0, 1)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    for f in ("csrc/saip_link_contact.hip", "csrc/saip_engine_link_contact.cpp"):
        assert f in capi.SOURCES
    assert "csrc/saip_link_contact.h" in capi.HEADERS


def _controller_batch(sp, L, B=4):
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, B, -1, C.byref(b)) == 0
    pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
    assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
    assert L.saip_batch_add_joint_task(b, b"jt", None, 0, 0.001, C.byref(tid)) == 0
    return robot, b


def _others_refuse(L, b, code):
    v, out = C.c_int(7), np.full(8 * 4, 7.0)
    assert L.saip_batch_link_contact_detach(b) == code
    assert L.saip_batch_link_contact_info(b, C.byref(v), None, None, None) == code
    assert L.saip_batch_link_contact_set_obstacles_host(b, _dp(out)) == code
    assert L.saip_batch_link_contact_set_materials_host(b, _dp(out)) == code
    assert L.saip_batch_link_contact_evaluate(b) == code
    assert L.saip_batch_link_contact_readout_host(b, _dp(out)) == code
    assert L.saip_batch_link_contact_summary_host(b, _dp(out)) == code
    assert L.saip_batch_link_contact_summary_reset(b) == code
    assert L.saip_batch_link_contact_add_cost(b, 1.0, 0.0) == code
    for name in POINTER_ENTRIES:
        assert getattr(L, name)(b) is None
    assert v.value == 7 and (out == 7.0).all()      # nothing was written


OBST = np.array([[0, 0.4, 0.0, 0.3, 0.4, 0.2, 0.6, 0.05], [1, 0.0, 0.0, 1.0, 0.1, 9.0, 9.0, 9.0], [0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0]])
MAT = np.array([[1e4, 50.0, 0.5, 1e-3], [2e4, 0.0, 0.0, 0.0], [5e3, 10.0, 0.0, -1.0]])


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_link_contact_attach
    links = np.array([1, 3, 5], np.int32)
    cen = np.array([[0.0, 0.0, 0.05], [0.01, 0.0, 0.0], [0.0, 0.0, 0.0]])
    rad = np.array([0.08, 0.06, 0.0])

    def call(b, S=3, links=links, cen=cen, rad=rad, O=3, obst=OBST, mat=MAT, per=0, keep=0):
        return att(b, S, None if links is None else _ip(links), None if cen is None else _dp(cen), None if rad is None else _dp(rad), O,
                   None if obst is None else _dp(obst), None if mat is None else _dp(mat), per, keep)

    def refused(b, msg, **kw):
        assert call(b, **kw) == INVALID and msg in L.saip_last_error(), (kw, L.saip_last_error())

    assert call(None) == INVALID
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert call(b) == ORDER                                          # before finalize, whatever the arguments
        assert call(b, S=0) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for S in (0, -1, 33, 2**31 - 1):
            refused(b, b"spheres required", S=S)
        for O in (0, -1, 17):
            refused(b, b"obstacles required", O=O)
        refused(b, b"null links", links=None)
        refused(b, b"null links", cen=None)
        refused(b, b"null links", rad=None)
        refused(b, b"null obstacles", obst=None)
        refused(b, b"null materials", mat=None)
        for bad in (-1, 10_000):
            l2 = links.copy()
            l2[1] = bad
            refused(b, b"sphere 1: link index", links=l2)
        for bad in (np.nan, np.inf):
            c2 = cen.copy()
            c2[2, 1] = bad
            refused(b, b"sphere 2: the centre is not finite", cen=c2)
            r2 = rad.copy()
            r2[0] = bad
            refused(b, b"sphere 0: the radius is not finite", rad=r2)
        r2 = rad.copy()
        r2[1] = -1e-12
        refused(b, b"sphere 1: radius", rad=r2)
        per = np.ascontiguousarray(np.repeat(OBST[:, :, None], B, axis=2))
        cases = [(0, 2, np.nan, b"obstacle 0: word 2 is not finite"), (1, 7, np.inf, b"obstacle 1: word 7 is not finite"),
                 (0, 7, -0.01, b"obstacle 0: radius"), (2, 0, 2.0, b"obstacle 2: unknown kind"), (1, 3, 1.0 + 3e-6, b"obstacle 1: the half-space normal"),
                 (1, 3, 1.0 - 3e-6, b"obstacle 1: the half-space normal"), (1, 3, 0.0, b"obstacle 1: the half-space normal")]
        for o, word, val, msg in cases:
            o1 = OBST.copy()
            o1[o, word] = val
            refused(b, msg, obst=o1)
            o2 = per.copy()
            o2[o, word, B - 1] = val
            refused(b, msg.replace(b":", b" of instance 3:", 1), obst=o2, per=1)
        for o, word, val, msg in [(0, 0, -1.0, b"material 0: word 0 (k)"), (1, 0, np.inf, b"material 1: word 0 (k)"), (2, 1, -1e-9, b"material 2: word 1 (c)"),
                                  (0, 1, np.inf, b"material 0: word 1 (c)"), (0, 2, -0.1, b"material 0: word 2 (mu)"), (1, 2, np.inf, b"material 1: word 2 (mu)"),
                                  (0, 3, 0.0, b"material 0: word 3 (v_s)"), (0, 3, -1e-3, b"material 0: word 3 (v_s)"), (1, 0, np.nan, b"material 1: word 0 (k) is NaN"),
                                  (2, 3, np.nan, b"material 2: word 3 (v_s) is NaN"), (0, 2, np.nan, b"material 0: word 2 (mu) is NaN")]:
            m2 = MAT.copy()
            m2[o, word] = val
            refused(b, msg, mat=m2)
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        for kw in (dict(), dict(obst=per, per=1), dict(keep=1), dict(S=1), dict(O=1)):
            assert call(b, **kw) == NO_DEVICE and b"no CPU path" in L.saip_last_error(), kw
        S = 32
        big = (np.arange(S, dtype=np.int32) % 8, np.zeros((S, 3)), np.full(S, 0.01))
        assert call(b, S=S, links=big[0], cen=big[1], rad=big[2], O=16, obst=np.ascontiguousarray(np.tile(OBST, (6, 1))[:16]),
                    mat=np.ascontiguousarray(np.tile(MAT, (6, 1))[:16])) == NO_DEVICE
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_link_contact(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        links, cen, rad = np.array([1], np.int32), np.zeros((1, 3)), np.array([0.1])
        assert L.saip_batch_link_contact_attach(b, 1, _ip(links), _dp(cen), _dp(rad), 3, _dp(OBST), _dp(MAT), 0, 0) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    sph = [("link4", (0, 0, 0.02), 0.08), ("end-effector", (0, 0, 0), 0.05)]
    for bad in (np.zeros(8), np.zeros((2, 7)), np.zeros((2, B, 8))):
        with pytest.raises(ValueError, match="obstacles of shape"):
            ctrl.attachLinkContact(sph, bad, MAT)
    with pytest.raises(ValueError, match="per-instance obstacles of shape"):
        ctrl.attachLinkContact(sph, OBST, MAT, per_instance=True)
    with pytest.raises(ValueError, match="materials of shape"):
        ctrl.attachLinkContact(sph, OBST, MAT[:2])
    with pytest.raises(ValueError, match="unknown link"):
        ctrl.attachLinkContact([("no-such-link", (0, 0, 0), 0.1)], OBST, MAT)
    with pytest.raises(ValueError, match="centre of shape"):
        ctrl.attachLinkContact([("link4", (0, 0), 0.1)], OBST, MAT)
    with pytest.raises(ValueError, match="sphere 1: radius"):
        ctrl.attachLinkContact([sph[0], ("link5", (0, 0, 0), -0.1)], OBST, MAT)
    m2 = MAT.copy()
    m2[0, 3] = 0.0
    with pytest.raises(ValueError, match=r"material 0: word 3 \(v_s\)"):
        ctrl.attachLinkContact(sph, OBST, m2)
    for per in (False, True):
        ob = np.ascontiguousarray(np.repeat(OBST[:, None, :], B, axis=1)) if per else OBST
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            ctrl.attachLinkContact(sph, ob, MAT, per_instance=per, keep=True)
    for fn in (ctrl.detachLinkContact, ctrl.linkContactInfo, ctrl.evaluateLinkContact, ctrl.linkContactReadout, ctrl.linkContactSummary,
               ctrl.resetLinkContactSummary, lambda: ctrl.linkContactCost(1.0), lambda: ctrl.setLinkContactObstacles(OBST), lambda: ctrl.setLinkContactMaterials(MAT)):
        with pytest.raises(sp.SaipError, match="no link contact is attached"):
            fn()
    assert ctrl.linkContactKeepDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "link_contact_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("link_contact_host"), "link_contact_host", []),
            _build(tmp_path_factory.mktemp("link_contact_host_san"), "link_contact_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _chain30w():
    """chain30 with a bracket welded behind link12 (as tests/test_gpu_clearance.py builds it)"""
    from sai_primitives_amd.controller import load_robot_description
    d = copy.deepcopy(load_robot_description("chain30"))
    d.pop("_source", None)
    d["name"] = "chain30w"
    bracket = dict(d["links"][11], name="bracket", joint_type="fixed", origin_xyz=[0.02, -0.03, 0.05], origin_rpy=[0.3, -0.2, 0.5], mass=0.3,
                   q_lower=0.0, q_upper=0.0, velocity_limit=0.0, effort_limit=0.0)
    d["links"].insert(12, bracket)
    return d


def _model(name):
    if name == "panda_sliding_base":                  # prismatic and revolute joints on one chain
        return W.load_robot(name)
    if name == "chain30w":                            # 30 dof, a welded link
        return W.RobotModel(_chain30w())
    if name == "tree":                                # a tree ancestor mask
        return W.RobotModel(TR.dual_panda_torso())
    return W.RobotModel(TR.dual_panda_fixed_torso())  # forest: spheres on the fixed base


def _spheres(model, rng, S):
    names = [l["name"] for l in model.links]
    pick = rng.choice(len(names), S, replace=S > len(names))
    return [(names[i], rng.uniform(-0.04, 0.04, 3), float(rng.uniform(0.02, 0.07)) * (rng.random() < 0.85)) for i in pick]


def _obstacles(rng, centres, O, per):
    """mixed kinds through the cloud of centres, sized so that a good share of the items is active: (O, 8) or (N, O, 8)"""
    N = centres.shape[0]
    flat = centres[np.isfinite(centres).all(axis=(1, 2))].reshape(-1, 3)
    lo, hi = flat.min(axis=0), flat.max(axis=0)
    shape = (N, O) if per else (O,)
    ob = np.zeros(shape + (8,))
    ob[..., 1:4] = rng.uniform(lo, hi, shape + (3,))
    ob[..., 4:7] = ob[..., 1:4] + rng.uniform(-0.4, 0.4, shape + (3,))
    ob[..., 7] = rng.uniform(0.1, 0.5, shape)
    kind = np.broadcast_to(np.arange(O) % 3, shape)
    ob[..., 4:7] = np.where((kind == 1)[..., None], ob[..., 1:4], ob[..., 4:7])      # every third a sphere (a == b)
    hs = kind == 2                                                                    # every third a half-space through the cloud
    n = rng.normal(size=shape + (3,))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    off = (n * rng.uniform(lo, hi, shape + (3,))).sum(axis=-1)
    ob[..., 0] = hs
    ob[..., 1:4] = np.where(hs[..., None], n, ob[..., 1:4])
    ob[..., 4] = np.where(hs, off, ob[..., 4])
    return ob


def _materials(rng, O):
    m = np.stack([rng.uniform(1e3, 5e4, O), rng.uniform(0.0, 200.0, O), rng.uniform(0.1, 1.0, O), 10.0 ** rng.uniform(-4, 0, O)], axis=1)
    m[rng.random(O) < 0.3, 2] = 0.0                  # frictionless obstacles ...
    m[m[:, 2] == 0.0, 3] = 0.0                       # ... need no v_s
    m[rng.random(O) < 0.2, 1] = 0.0
    return m


def _case(name, seed, N, S, O, per):
    rng = np.random.default_rng(seed)
    model = _model(name)
    sph = _spheres(model, rng, S)
    q = rng.uniform(-1.0, 1.0, (N, model.dof))
    dq = rng.normal(size=(N, model.dof)) * rng.choice([0.0, 1e-4, 1.0], (N, 1))      # |v_t| on both sides of v_s, and at rest
    c, v, (frames, jtype, aw, oj) = LC.sphere_state(model, q, dq, sph)
    order, anc = LC.sort_spheres(model, sph)
    tau = rng.normal(size=(N, model.dof)) * 10
    tau[rng.random((N, model.dof)) < 0.1] = np.nan                                   # NaN commanded torques
    s = np.abs(rng.normal(size=(N, 4))) * (rng.random((N, 1)) < 0.6)
    return dict(N=N, S=S, O=O, n=model.dof, per=per, order=order, anc=anc, jtype=jtype, dt=5e-4, w=(3.0, 0.25), centres=c, vels=v,
                radii=np.array([r for _, _, r in sph]), obst=_obstacles(rng, c, O, per), mat=_materials(rng, O), aw=aw, oj=oj, tau=tau, summary=s,
                cost=rng.normal(size=N))


def _run(exe, c, tmp):
    N, S, n = c["N"], c["S"], c["n"]
    obst = np.ascontiguousarray(c["obst"].transpose(1, 2, 0)) if c["per"] else c["obst"]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, S, c["O"], n, int(c["per"])], np.int32).tobytes())
        f.write(np.asarray(c["order"], np.int32).tobytes())
        f.write(np.asarray(c["anc"], np.uint32).tobytes())
        f.write(np.asarray(c["jtype"], np.int32).tobytes())
        f.write(np.array([c["dt"], *c["w"]], float).tobytes())
        for a in (c["centres"], c["vels"], c["radii"], obst, c["mat"], c["aw"], c["oj"], c["tau"], np.ascontiguousarray(c["summary"].T), c["cost"]):
            f.write(np.ascontiguousarray(a, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    sizes = [8 * N, 3 * N * S, N * n, 4 * N, N]
    assert raw.size == sum(sizes)
    ro, F, tau, s, cost = np.split(raw, np.cumsum(sizes)[:-1])
    return dict(readout=ro.reshape(N, 8), F=F.reshape(N, S, 3), tau=tau.reshape(N, n), summary=s.reshape(4, N).T, cost=cost)


def _ref(c):
    ev = LC.evaluate(c["centres"], c["vels"], c["radii"], c["obst"], c["mat"], c["order"])
    s = LC.summary_advance(c["summary"], c["dt"], ev["readout"])
    return dict(readout=ev["readout"], F=ev["F"], tau=LC.torques(ev, c["centres"], c["order"], c["anc"], c["jtype"], c["aw"], c["oj"], c["tau"]), summary=s,
                cost=LC.add_cost(c["cost"], s[:, 0], s[:, 1], *c["w"]), ev=ev)


def _same_bits(got, ref, what):
    for key in got:
        a, b = np.ascontiguousarray(got[key], float), np.ascontiguousarray(ref[key], float)
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (what, key, np.argwhere(~same)[:4], a[~same][:4], b[~same][:4])


def _check(exes, c, tmp, what):
    ref = _ref(c)
    for exe in exes:
        _same_bits(_run(exe, c, tmp), ref, what)
    return ref


def test_host_build_matches_restatement_random(exes, tmp_path):
    """S in {1, 9, 32} x O in {1, 4, 16} over a chain with prismatic joints, a 30-dof chain with a welded link, a tree and a forest with
    spheres on the fixed base; batch-uniform and per-instance tables"""
    i = 0
    share = []
    for S in (1, 9, 32):
        for O in (1, 4, 16):
            for per in (False, True):
                name = ["panda_sliding_base", "chain30w", "tree", "forest"][i % 4]
                c = _case(name, 200 + i, 12, S, O, per)
                ref = _check(exes, c, tmp_path, (name, S, O, per))
                share.append(ref["readout"][:, 5].sum() / (12 * S * O))
                if S >= 9 and O >= 4:
                    assert np.abs(ref["tau"] - np.where(np.isnan(c["tau"]), 0.0, c["tau"])).max() > 1.0          # the obstacles push
                i += 1
    print("share of active items per case:", np.round(share, 2))
    assert 0.2 < np.mean(share) < 0.8
    # base spheres, a welded link, both joint types and NaN torques were in the cases
    assert any(m == 0 for m in _case("forest", 1, 2, 32, 1, False)["anc"]) and 2 in _case("panda_sliding_base", 1, 2, 1, 1, False)["jtype"]


def _blank(N=4, S=1, O=1):
    c = _case("panda_sliding_base", 9, N, S, O, False)
    c["summary"] = np.zeros((N, 4))
    c["vels"][:] = 0.0
    return c


def test_host_build_matches_restatement_edges(exes, tmp_path):
    floor = np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]], float)
    # d exactly 0 is inactive; radius 0; one ulp below is active
    c = _blank(3)
    c["obst"], c["mat"], c["radii"] = floor, np.array([[1e4, 0.0, 0.5, 1e-3]]), np.array([0.0])
    c["centres"][:, 0] = [[0.3, 0.1, 0.0], [0.3, 0.1, -2.0 ** -60], [0.3, 0.1, 0.25]]
    ref = _check(exes, c, tmp_path, "d == 0")
    ro = ref["readout"]
    assert ro[0, 3] == 0.0 and ro[0, 5] == 0 and (ro[0, 0:3] == 0).all() and ro[1, 5] == 1 and ro[1, 2] > 0 and ro[2, 5] == 0
    u0 = np.where(np.isnan(c["tau"]), 0.0, c["tau"])
    assert (ref["tau"][[0, 2]] == u0[[0, 2]]).all() and (ref["tau"][1] != u0[1]).any()
    # len == 0: the centre exactly on a capsule's axis (and at the centre of a sphere obstacle): no force, though d < 0 is the smallest distance
    c = _blank(3, 1, 2)
    c["obst"] = np.array([[0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.01], [0, 0.1, 0.2, 0.3, 0.1, 0.2, 0.3, 0.02]])
    c["mat"], c["radii"] = np.array([[1e4, 1.0, 0.5, 1e-3]] * 2), np.array([0.03])
    c["centres"][:, 0] = [[0.25, 0.0, 0.0], [0.1, 0.2, 0.3], [0.25, 0.0, 0.015]]
    ref = _check(exes, c, tmp_path, "len == 0")
    ro = ref["readout"]
    assert ro[0, 3] == -(0.03 + 0.01) and ro[0, 5] == 0 and ro[1, 3] == -(0.03 + 0.02) and ro[1, 5] == 0 and (ro[:2, 0:3] == 0).all()
    assert ro[2, 5] == 1 and ro[2, 2] > 0 and ro[2, 0] == 0 and ro[2, 1] == 0
    # mu == 0 (with v_s = 0 and v_s < 0): no tangential force, no NaN; |v_t| below, at and above v_s, and exactly 0
    c = _blank(5, 1, 1)
    c["obst"], c["radii"] = floor, np.array([0.05])
    c["centres"][:, 0] = [0.2, 0.0, 0.0]
    c["vels"][:, 0] = [[0, 0, 0], [5e-4, 0, 0], [1e-3, 0, 0], [0.3, 0.4, 0.0], [0.3, 0.4, -0.2]]
    for mu, vs in ((0.0, 0.0), (0.0, -1.0), (0.5, 1e-3)):
        c["mat"] = np.array([[1e4, 20.0, mu, vs]])
        ref = _check(exes, c, tmp_path, ("friction", mu, vs))
        F = ref["F"][:, 0]
        assert np.isfinite(F).all() and (F[:, 2] > 0).all()
        if mu == 0.0:
            assert (F[:, 0:2] == 0).all()
        else:
            ft = np.linalg.norm(F[:, 0:2], axis=1)
            assert ft[0] == 0 and np.isclose(ft[1], 0.5 * mu * F[1, 2]) and np.isclose(ft[2], mu * F[2, 2]) and np.isclose(ft[3], mu * F[3, 2])
            assert F[4, 2] == 1e4 * 0.05 + 20.0 * 0.2                                  # the damping term of an approaching sphere
    # a NaN / infinite centre: the instance is invalid, its neighbours are not
    for bad in (np.nan, np.inf, -np.inf):
        c = _case("tree", 11, 5, 9, 4, True)
        c["centres"][1, 8, 2] = bad
        c["centres"][3, 0, 0] = bad
        ref = _check(exes, c, tmp_path, ("invalid", bad))
        ro = ref["readout"]
        for i in (1, 3):
            assert np.isnan(ro[i, [0, 1, 2, 3, 6, 7]]).all() and ro[i, 4] == -1 and ro[i, 5] == 0
            assert np.isnan(ref["summary"][i, 0]) and np.isnan(ref["cost"][i]) and (ref["summary"][i, 1:] == c["summary"][i, 1:]).all()
            assert (ref["tau"][i] == np.where(np.isnan(c["tau"][i]), 0.0, c["tau"][i])).all()
        assert np.isfinite(ro[[0, 2, 4]]).all() and np.isfinite(ref["cost"][[0, 2, 4]]).all()
    # two items with the same distance: the lowest k in the caller's numbering wins, whatever the sorted order says
    c = _case("chain30w", 12, 2, 32, 1, False)
    c["obst"], c["radii"] = floor, np.zeros(32)
    c["centres"][:, :, 2] = 0.5 + 0.01 * np.arange(32)
    for ks in ((3, 11), (5, 10), (30, 2), (0, 31)):
        c["centres"][:, :, 2] = 0.5 + 0.01 * np.arange(32)
        for k in ks:
            c["centres"][:, k, 2] = 0.25
        ref = _check(exes, c, tmp_path, ("tie", ks))
        assert (ref["readout"][:, 4] == min(ks)).all() and (ref["readout"][:, 3] == 0.25).all()
    assert LC.decode(-1, 4) is None and LC.decode(4 * 7 + 2, 4) == (7, 2)


def _single_items(N, centres, vels, obst, mat, radius, summary=None, cost=None, per=True):
    """a case for the host build with one sphere and one obstacle per instance: F of the sphere is the item's force"""
    return dict(N=N, S=1, O=1, n=1, per=per, order=[0], anc=[0], jtype=[1], dt=0.5, w=(2.0, 0.5), centres=centres[:, None, :], vels=vels[:, None, :],
                radii=np.array([radius]), obst=obst, mat=mat[None, :], aw=np.zeros((N, 1, 3)), oj=np.zeros((N, 1, 3)), tau=np.zeros((N, 1)),
                summary=np.zeros((N, 4)) if summary is None else summary, cost=np.ones(N) if cost is None else cost)


def test_force_law_invariants(exes, tmp_path):
    """on random inputs, for the host build of the header (lc_item through lc_evaluate_host: its F of a single item, bit for bit the
    restatement's f) and for the terms the law itself forms: f . n >= 0, |f_t| <= mu f_n (1 + 4 ulp), f_t . v_t <= 0, nothing from an
    inactive item.  The dot products and the norm of the check are taken in extended precision, so that the roundings counted are the
    law's own: one in g v_t, one in the division, 1.5 in sqrt(v_t . v_t) -- under 4 ulp."""
    rng = np.random.default_rng(5)
    N = 4000
    c, v = rng.uniform(-0.5, 0.5, (N, 3)), rng.normal(size=(N, 3)) * rng.choice([0.0, 1e-4, 1.0], (N, 1))
    ob = _obstacles(rng, c[:, None, :], 1, True)[:, 0]
    eps = np.finfo(float).eps
    ld = np.longdouble
    for m in (np.array([2e4, 80.0, 0.7, 1e-3]), np.array([1e3, 0.0, 0.0, 0.0]), np.array([5e4, 500.0, 1.2, 0.5])):
        d, n, fn, ft, vt, f, act = LC.item_parts(ob, m, c, v, 0.05)
        d2, f2, fn2, act2 = LC.item(ob, m, c, v, 0.05)
        for exe in exes:                                                                               # the header's own item force
            got = _run(exe, _single_items(N, c, v, ob[:, None, :], m, 0.05), tmp_path)
            F = got["F"][:, 0]
            want = np.zeros_like(f2) + f2                                                               # F_s = (0, 0, 0) + f: a -0.0 component becomes +0.0
            same = F.view(np.uint64) == want.view(np.uint64)
            assert same.all(), (np.argwhere(~same)[:4], F[~same][:4], want[~same][:4])
            assert (F[~act] == 0).all() and ((F.astype(ld) * n.astype(ld)).sum(1)[act] >= 0).all()
            assert (got["readout"][:, 3].view(np.uint64) == d.view(np.uint64)).all() and (got["readout"][:, 5] == act).all()
            assert (got["readout"][:, 6].view(np.uint64) == fn2.view(np.uint64)).all()
        assert act.any() and not act.all() and (act == (d < 0)).all() and (act2 == act).all()
        assert (f2[~act] == 0).all() and (fn2[~act] == 0).all() and (f2[act] == f[act]).all()          # no force from an inactive item
        assert ((f.astype(ld) * n.astype(ld)).sum(1)[act] >= 0).all() and (fn[act] >= 0).all()
        norm_ft = np.sqrt((ft.astype(ld) ** 2).sum(1))
        assert (norm_ft[act] <= ld(m[2]) * fn[act].astype(ld) * (1 + 4 * ld(eps))).all()
        assert ((ft.astype(ld) * vt.astype(ld)).sum(1)[act] <= 0).all()
        if m[2] == 0.0:
            assert (ft == 0).all()
        else:
            assert (norm_ft[act & (fn > 0) & (np.linalg.norm(vt, axis=1) > m[3])] > 0).all()


def test_summary_and_cost_rules(exes, tmp_path):
    """lc_summary_advance and lc_add_cost of the host build over two substeps, against the restatement bit for bit and against the rules
    spelled out: sums, maxima, counts; NaN sticks in row 0 only and makes the cost NaN"""
    floor, mat = np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]]), np.array([1e3, 0.0, 0.0, 0.0])
    zs = np.array([[-0.01, 0.2, np.nan], [-0.002, -0.03, 0.1]])
    for exe in exes:
        s, ref = np.zeros((3, 4)), np.zeros((3, 4))
        for z in zs:
            cen = np.zeros((3, 3))
            cen[:, 2] = z
            c = _single_items(3, cen, np.zeros((3, 3)), floor, mat, 0.0, summary=s, per=False)
            got = _run(exe, c, tmp_path)
            ro = LC.evaluate(c["centres"], c["vels"], c["radii"], floor, c["mat"])["readout"]
            ref = LC.summary_advance(ref, 0.5, ro)
            _same_bits(dict(readout=got["readout"], summary=got["summary"], cost=got["cost"]),
                       dict(readout=ro, summary=ref, cost=LC.add_cost(c["cost"], ref[:, 0], ref[:, 1], *c["w"])), "summary rules")
            s = got["summary"]
        fn = 1e3 * np.array([0.01, 0.002, 0.03])
        assert s[0, 0] == 0.5 * fn[0] + 0.5 * fn[1] and s[0, 1] == fn[0] and s[0, 2] == 0.01 and s[0, 3] == 2.0
        assert s[1, 0] == 0.0 + 0.5 * fn[2] and s[1, 1] == fn[2] and s[1, 2] == 0.03 and s[1, 3] == 1.0
        assert np.isnan(s[2, 0]) and (s[2, 1:] == 0).all()                             # NaN is sticky in row 0 only
        assert got["cost"][0] == 1.0 + (2.0 * s[0, 0] + 0.5 * s[0, 1]) and np.isnan(got["cost"][2])
    assert np.isnan(LC.add_cost(np.ones(1), np.array([np.nan]), np.array([0.0]), 0.0, 0.0))[0]
