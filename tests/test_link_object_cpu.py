"""The pushed object of link contact, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument and
call-order errors come back with the documented codes before the device is needed; the Python facade raises the same; the host build of
csrc/saip_link_object.h (tests/cpp/link_object_host.cpp, also under ASan/UBSan) matches the NumPy restatement tests/link_object_ref.py bit
for bit in the state, tau_sim, both readouts, the sphere forces, both summaries and the cost; and the host build alone keeps the invariants
of a rigid body under contact: free fall, a constant angular velocity, action and reaction, a resting plate, momentum."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import link_contact_ref as LC
import link_object_ref as LO
import test_link_contact_cpu as TLC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_link_object_" + n for n in ("attach", "detach", "info", "set_state_host", "state_host", "set_inertial_host", "readout_host",
                                                          "summary_host", "summary_reset", "add_cost")]
POINTER_ENTRIES = ["saip_batch_link_object_" + n + "_device" for n in ("state", "readout", "summary")]
EPS = 2.0 ** -52
_dp, _ip = TLC._dp, TLC._ip


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    src = open(os.path.join(PKG, "csrc", "saip_link_object.h")).read()
    for name, val in [("MAX_SPHERES", 8), ("STATE_ROWS", 13), ("INERTIAL_WORDS", 4), ("READOUT_ROWS", 12), ("SUMMARY_ROWS", 4)]:
        assert re.search(rf"#define SAIP_LINK_OBJECT_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_LINK_OBJECT_" + name) == val == getattr(LO, name)
        assert re.search(rf"LINK_OBJECT_{name} = {val}\b", src), name
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert "csrc/saip_link_object.h" in capi.HEADERS


SHAPE_C = np.array([[0.02, 0.0, 0.0], [-0.02, 0.0, 0.01]])
SHAPE_R = np.array([0.03, 0.0])
OMAT = np.array([2e4, 30.0, 0.4, 1e-3])
INERTIAL = np.array([0.5, 1e-3, 2e-3, 3e-3])


def _others_refuse(L, b, code):
    v, out = C.c_int(7), np.full(13 * 4, 7.0)
    assert L.saip_batch_link_object_detach(b) == code
    assert L.saip_batch_link_object_info(b, C.byref(v), None) == code
    assert L.saip_batch_link_object_set_state_host(b, _dp(out), 0) == code
    assert L.saip_batch_link_object_state_host(b, _dp(out)) == code
    assert L.saip_batch_link_object_set_inertial_host(b, _dp(out)) == code
    assert L.saip_batch_link_object_readout_host(b, _dp(out)) == code
    assert L.saip_batch_link_object_summary_host(b, _dp(out)) == code
    assert L.saip_batch_link_object_summary_reset(b) == code
    assert L.saip_batch_link_object_add_cost(b, _dp(out), 1.0, None, 0.0) == code
    for name in POINTER_ENTRIES:
        assert getattr(L, name)(b) is None
    assert v.value == 7 and (out == 7.0).all()      # nothing was written


def test_c_abi_error_contract(sp):
    """what a batch without a device can reach: every argument error of _attach (they are reported before the order errors that need an
    attached link contact, which such a batch cannot hold), and the order errors of every entry.  The errors behind an attachment
    (_set_state_host, _set_inertial_host, _add_cost) are in tests/test_gpu_link_object.py."""
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    att = L.saip_batch_link_object_attach

    def call(b, P=2, cen=SHAPE_C, rad=SHAPE_R, mat=OMAT, inr=INERTIAL, per=0):
        return att(b, P, *(None if a is None else _dp(np.ascontiguousarray(a, float)) for a in (cen, rad, mat, inr)), per)

    def refused(b, msg, **kw):
        assert call(b, **kw) == INVALID and msg in L.saip_last_error(), (kw, L.saip_last_error())

    assert call(None) == INVALID
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = TLC._controller_batch(sp, L, B)
    try:
        assert call(b) == ORDER and call(b, P=0) == ORDER                # before finalize, whatever the arguments
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for P in (0, -1, 9, 2**31 - 1):
            refused(b, b"spheres required", P=P)
        refused(b, b"null centres", cen=None)
        refused(b, b"null centres", rad=None)
        refused(b, b"null material", mat=None)
        refused(b, b"null inertial", inr=None)
        for bad in (np.nan, np.inf):
            c2 = SHAPE_C.copy()
            c2[1, 2] = bad
            refused(b, b"sphere 1: the centre is not finite", cen=c2)
            r2 = SHAPE_R.copy()
            r2[0] = bad
            refused(b, b"sphere 0: the radius is not finite", rad=r2)
        refused(b, b"sphere 1: radius", rad=np.array([0.03, -1e-12]))
        for word, val, msg in [(0, -1.0, b"word 0 (k)"), (1, np.inf, b"word 1 (c)"), (2, -0.1, b"word 2 (mu)"), (3, 0.0, b"word 3 (v_s)"), (2, np.nan, b"word 2 (mu) is NaN")]:
            m2 = OMAT.copy()
            m2[word] = val
            refused(b, b"material 0: " + msg, mat=m2)
        per = np.ascontiguousarray(np.repeat(INERTIAL[:, None], B, axis=1))
        for word, name in enumerate((b"m", b"Ix", b"Iy", b"Iz")):
            for val in (0.0, -1.0, np.inf, np.nan):
                i2 = INERTIAL.copy()
                i2[word] = val
                refused(b, b"inertial word %d (%s) =" % (word, name), inr=i2)
                i3 = per.copy()
                i3[word, B - 1] = val
                refused(b, b"inertial word %d (%s) of instance 3" % (word, name), inr=i3, per=1)
        # valid arguments: the object is the second stage of a link contact this batch does not have
        for kw in (dict(), dict(inr=per, per=1), dict(P=1)):
            assert call(b, **kw) == ORDER and b"no link contact is attached" in L.saip_last_error(), kw
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert call(b) == ORDER and b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    ctrl = sp.RobotController(robot, [sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)])
    sph = [((0.02, 0, 0), 0.03), ((-0.02, 0, 0), 0.03)]
    with pytest.raises(ValueError, match=r"sphere 1: \(centre, radius\) expected"):
        ctrl.attachLinkObject([sph[0], ("link4", (0, 0, 0), 0.1)], OMAT, INERTIAL)
    with pytest.raises(ValueError, match="centre of shape"):
        ctrl.attachLinkObject([((0, 0), 0.1)], OMAT, INERTIAL)
    with pytest.raises(ValueError, match="material of shape"):
        ctrl.attachLinkObject(sph, np.zeros((1, 4)), INERTIAL)
    with pytest.raises(ValueError, match="inertial words of shape"):
        ctrl.attachLinkObject(sph, OMAT, np.zeros(3))
    with pytest.raises(ValueError, match="per-instance inertial words of shape"):
        ctrl.attachLinkObject(sph, OMAT, INERTIAL, per_instance=True)
    with pytest.raises(ValueError, match="state of shape"):
        ctrl.attachLinkObject(sph, OMAT, INERTIAL, state=np.zeros(12))
    with pytest.raises(ValueError, match="sphere 1: radius"):
        ctrl.attachLinkObject([sph[0], ((0, 0, 0), -0.1)], OMAT, INERTIAL)
    with pytest.raises(ValueError, match=r"inertial word 2 \(Iy\)"):
        ctrl.attachLinkObject(sph, OMAT, [1.0, 1.0, 0.0, 1.0])
    with pytest.raises(sp.SaipError, match="no link contact is attached"):
        ctrl.attachLinkObject(sph, OMAT, INERTIAL)
    for fn in (ctrl.detachLinkObject, ctrl.linkObjectInfo, ctrl.objectState, ctrl.objectReadout, ctrl.objectSummary, ctrl.resetObjectSummary,
               lambda: ctrl.objectCost((0, 0, 0), 1.0), lambda: ctrl.setObjectState(np.r_[0, 0, 0, 1, 0, 0, 0, np.zeros(6)]), lambda: ctrl.setObjectInertial(INERTIAL)):
        with pytest.raises(sp.SaipError, match="no link object is attached"):
            fn()
    for bad, msg in (((0, 0), "target position of shape"),):
        with pytest.raises(ValueError, match=msg):
            ctrl.objectCost(bad, 1.0)
    with pytest.raises(ValueError, match="target quaternion of shape"):
        ctrl.objectCost((0, 0, 0), 1.0, (1, 0, 0), 1.0)
    assert ctrl.objectStateDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "link_object_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("link_object_host"), "link_object_host", []),
            _build(tmp_path_factory.mktemp("link_object_host_san"), "link_object_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _quat(rng, N):
    q = rng.normal(size=(N, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _case(name, seed, N, S, O, per, P, per_in):
    """a link-contact case (tests/test_link_contact_cpu.py) and an object in the cloud of the robot's spheres: its origin near a sphere
    centre of the instance, so that a good share of the robot-object and of the object-world items is active"""
    c = TLC._case(name, seed, N, S, O, per)
    rng = np.random.default_rng(seed + 1000)
    x = np.zeros((N, 13))
    x[:, 0:3] = c["centres"][np.arange(N), rng.integers(S, size=N)] + rng.uniform(-0.06, 0.06, (N, 3))
    x[:, 3:7] = _quat(rng, N)
    x[:, 7:10] = rng.normal(size=(N, 3)) * rng.choice([0.0, 1e-4, 0.5], (N, 1))
    x[:, 10:13] = rng.normal(size=(N, 3)) * rng.choice([0.0, 2.0], (N, 1))
    inr = np.stack([rng.uniform(0.1, 2.0, N), *(rng.uniform(1e-4, 1e-2, N) for _ in range(3))], axis=1)
    c.update(P=P, per_in=per_in, state=x, inertial=inr if per_in else inr[0], shape_r=rng.uniform(-0.05, 0.05, (P, 3)),
             shape_radius=rng.uniform(0.02, 0.07, P) * (rng.random(P) < 0.85), omat=np.array([rng.uniform(1e3, 5e4), rng.uniform(0, 100.0), 0.5, 1e-3]),
             grav=np.array([0.0, 0.0, -9.81]), osummary=np.abs(rng.normal(size=(N, 4))) * (rng.random((N, 1)) < 0.6), tp=rng.uniform(-0.5, 0.5, 3),
             tq=_quat(rng, 1)[0] if seed % 2 else None, wo=(2.0, 0.75))
    return c


def _run(exe, c, tmp):
    N, S, n, P = c["N"], c["S"], c["n"], c["P"]
    obst = np.ascontiguousarray(c["obst"].transpose(1, 2, 0)) if c["per"] else c["obst"]
    tq = c.get("tq")
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, S, c["O"], n, int(c["per"]), P, int(c["per_in"])], np.int32).tobytes())
        f.write(np.asarray(c["order"], np.int32).tobytes())
        f.write(np.asarray(c["anc"], np.uint32).tobytes())
        f.write(np.asarray(c["jtype"], np.int32).tobytes())
        f.write(np.array([c["dt"], *c["grav"], *c["wo"], 0.0 if tq is None else 1.0, *c["tp"], *(np.zeros(4) if tq is None else tq)], float).tobytes())
        inr = np.ascontiguousarray(np.asarray(c["inertial"]).T) if c["per_in"] else c["inertial"]
        for a in (c["centres"], c["vels"], c["radii"], obst, c["mat"], c["aw"], c["oj"], c["tau"], np.ascontiguousarray(c["summary"].T),
                  np.ascontiguousarray(c["osummary"].T), c["cost"], c["shape_r"], c["shape_radius"], c["omat"], inr, np.ascontiguousarray(c["state"].T)):
            f.write(np.ascontiguousarray(a, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    sizes = [8 * N, 12 * N, 3 * N * S, N * n, 4 * N, 4 * N, 13 * N, N]
    assert raw.size == sum(sizes)
    ro, rq, F, tau, s, so, x, cost = np.split(raw, np.cumsum(sizes)[:-1])
    return dict(readout_lc=ro.reshape(N, 8), readout=rq.reshape(N, 12), F=F.reshape(N, S, 3), tau=tau.reshape(N, n), summary=s.reshape(4, N).T,
                osummary=so.reshape(4, N).T, state=x.reshape(13, N).T, cost=cost)


def _ref(c):
    st = LO.step(c["centres"], c["vels"], c["radii"], c["obst"], c["mat"], c["order"], c["state"], c["inertial"], c["shape_r"], c["shape_radius"], c["omat"],
                 c["grav"], c["dt"])
    return dict(readout_lc=st["readout_lc"], readout=st["readout"], F=st["F"], tau=LO.torques(st, c["centres"], c["order"], c["anc"], c["jtype"], c["aw"], c["oj"], c["tau"]),
                summary=LC.summary_advance(c["summary"], c["dt"], st["readout_lc"]), osummary=LO.summary_advance(c["osummary"], c["dt"], st),
                state=st["state"], cost=LO.add_cost(c["cost"], st["state"], c["tp"], c["wo"][0], c.get("tq"), c["wo"][1])), st


def _check(exes, c, tmp, what):
    ref, st = _ref(c)
    for exe in exes:
        TLC._same_bits(_run(exe, c, tmp), ref, what)
    return ref, st


def test_host_build_matches_restatement_random(exes, tmp_path):
    """S in {1, 9} x P in {1, 8} x O in {1, 4} x both inertial table forms over a chain with a prismatic joint (the slider), a 30-dof chain
    with a welded link and a tree; batch-uniform and per-instance obstacles in turn; NaN commanded torques come with the cases"""
    i, robot_share, world_share, moved = 0, [], [], 0
    for S in (1, 9):
        for P in (1, 8):
            for O in (1, 4):
                for per_in in (False, True):
                    name = ["panda_sliding_base", "chain30w", "tree"][i % 3]
                    c = _case(name, 300 + i, 10, S, O, bool((i // 2) % 2), P, per_in)
                    ref, st = _check(exes, c, tmp_path, (name, S, P, O, per_in))
                    robot_share.append(ref["readout"][:, 11].sum() / (10 * S * P))
                    world_share.append((st["partial"]["wpen"] > 0).mean())
                    moved += (ref["state"] != c["state"]).any(axis=1).sum()
                    assert np.isnan(c["tau"]).any() or S * O == 1
                    i += 1
    print("share of active robot-object items per case:", np.round(robot_share, 2), "instances with object-world penetration:", np.round(world_share, 2))
    assert 0.1 < np.mean(robot_share) < 0.9 and 0.1 < np.mean(world_share) < 0.95 and moved == 10 * i


def _blank(N, S=1, O=1, P=1):
    """robot spheres and one obstacle far from an object at the origin, everything at rest, no gravity"""
    c = _case("panda_sliding_base", 9, N, S, O, False, P, False)
    c["summary"], c["osummary"] = np.zeros((N, 4)), np.zeros((N, 4))
    c["vels"][:] = 0.0
    c["centres"][:] = 5.0 + np.arange(S)[None, :, None]
    c["obst"] = np.tile(np.array([[1, 0.0, 0.0, 1.0, -50.0, 0, 0, 0]]), (O, 1))
    c["mat"] = np.tile(np.array([[1e4, 0.0, 0.0, 0.0]]), (O, 1))
    c["state"] = np.tile(np.r_[0, 0, 0, 1, 0, 0, 0, np.zeros(6)], (N, 1)).astype(float)
    c["shape_r"], c["shape_radius"] = np.zeros((P, 3)), np.full(P, 0.05)
    c["grav"] = np.zeros(3)
    c["inertial"] = np.array([1.0, 1e-3, 1e-3, 1e-3])
    return c


def test_host_build_matches_restatement_edges(exes, tmp_path):
    # d exactly 0 is inactive; one ulp deeper is active; far away is inactive
    c = _blank(3)
    c["radii"], c["shape_radius"], c["omat"] = np.array([0.25]), np.array([0.0625]), np.array([1e4, 0.0, 0.5, 1e-3])
    c["centres"][:, 0] = [[0.0, 0.0, 0.3125], [0.0, 0.0, 0.3125 - 2.0 ** -54], [0.0, 0.0, 0.9]]
    ref, st = _check(exes, c, tmp_path, "d == 0")
    rq = ref["readout"]
    assert rq[0, 9] == 0.0 and rq[0, 11] == 0 and rq[1, 9] < 0 and rq[1, 11] == 1 and rq[1, 2] < 0 and rq[2, 11] == 0 and (rq[[0, 2], 0:9] == 0).all()
    u0 = np.where(np.isnan(c["tau"]), 0.0, c["tau"])
    assert (ref["tau"][[0, 2]] == u0[[0, 2]]).all() and (ref["tau"][1] != u0[1]).any()
    assert (ref["state"][[0, 2]] == c["state"][[0, 2]]).all() and ref["state"][1, 9] < 0        # the pushed body moves, the others rest
    # len == 0: the robot sphere's centre on the object sphere's centre: no direction, no force, though d < 0 is the smallest distance
    c = _blank(2)
    c["radii"] = np.array([0.03])
    c["centres"][:, 0] = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.05]]
    ref, st = _check(exes, c, tmp_path, "len == 0")
    rq = ref["readout"]
    assert rq[0, 9] == -(0.03 + 0.05) and rq[0, 11] == 0 and (rq[0, 0:9] == 0).all() and rq[1, 11] == 1 and rq[1, 2] < 0
    # mu == 0 (with v_s = 0): no tangential reaction and no NaN, against a sliding robot sphere
    c = _blank(3)
    c["radii"] = np.array([0.05])
    c["centres"][:, 0] = [0.0, 0.0, 0.08]
    c["vels"][:, 0] = [[0, 0, 0], [0.3, 0.4, 0.0], [0.3, 0.4, -0.2]]
    for mu, vs in ((0.0, 0.0), (0.5, 1e-3)):
        c["omat"] = np.array([1e4, 20.0, mu, vs])
        ref, st = _check(exes, c, tmp_path, ("friction", mu))
        rf = ref["readout"][:, 0:3]
        assert np.isfinite(ref["state"]).all() and (rf[:, 2] < 0).all()
        assert (rf[:, 0:2] == 0).all() if mu == 0.0 else (rf[0, 0:2] == 0).all() and (rf[1:, 0] > 0).all()          # friction drags the body along
        assert abs(ref["readout"][2, 2] + (1e4 * 0.02 + 20.0 * 0.2)) < 1e-9                # stiffness and the damping term of an approaching sphere
    # a state that is not finite, or a robot sphere centre that is not: the instance is invalid, its neighbours are not
    for bad in (np.nan, np.inf, -np.inf):
        c = _case("tree", 11, 6, 9, 4, True, 8, True)
        c["state"][1, 2] = bad
        c["state"][3, 11] = bad
        c["centres"][4, 8, 2] = bad
        ref, st = _check(exes, c, tmp_path, ("invalid", bad))
        for i in (1, 3, 4):
            assert np.isnan(ref["readout"][i]).all() and np.isnan(ref["osummary"][i, 0]) and (ref["osummary"][i, 1:] == c["osummary"][i, 1:]).all()
            assert (ref["tau"][i] == np.where(np.isnan(c["tau"][i]), 0.0, c["tau"][i])).all()
            assert TLC._same_bits(dict(x=ref["state"][i]), dict(x=c["state"][i]), "state kept") is None
        assert np.isinf(ref["cost"][[1, 3]]).all() and (ref["cost"][[1, 3]] > 0).all() and np.isfinite(ref["cost"][[0, 2, 4, 5]]).all()
        assert np.isfinite(ref["readout"][[0, 2, 5]]).all() and np.isnan(ref["readout_lc"][4, 3]) and np.isfinite(ref["readout_lc"][[1, 3]]).all()
    # two items with the same distance: the lowest s P + p in the caller's numbering wins, whatever the sorted order says
    c = _case("chain30w", 12, 2, 9, 1, False, 8, False)
    c["state"] = _blank(2)["state"]
    c["shape_r"], c["shape_radius"], c["radii"] = np.zeros((8, 3)), np.full(8, 0.01), np.zeros(9)
    c["shape_r"][:, 0] = 0.1 * np.arange(8)
    for pairs in (((3, 2), (7, 5)), ((8, 0), (1, 7)), ((6, 5), (5, 6))):
        c["centres"][:] = 9.0 + np.arange(9)[None, :, None]
        for s, p in pairs:
            c["centres"][:, s] = [0.1 * p, 0.0, 0.5]
        ref, st = _check(exes, c, tmp_path, ("tie", pairs))
        assert (ref["readout"][:, 10] == min(s * 8 + p for s, p in pairs)).all() and (ref["readout"][:, 9] == 0.5 - 0.01).all()
    assert LO.decode(-1, 8) is None and LO.decode(8 * 7 + 2, 8) == (7, 2)


# ------------------------------------------------------------------ invariants of the host build, without a reference
def _advance(exe, c, tmp, K):
    """K substeps of the host build with a robot that does not move; returns the outputs of every substep"""
    outs = []
    for _ in range(K):
        got = _run(exe, c, tmp)
        c["state"], c["summary"], c["osummary"] = got["state"], got["summary"], got["osummary"]
        outs.append(got)
    return outs


def test_free_fall_matches_the_closed_form_of_the_scheme(exes, tmp_path):
    """nothing touches: v_K = K dt g and p_K = p_0 + dt^2 g K (K + 1) / 2.  Per substep F = fl(m g), a = fl(F / m), inc = fl(dt a): three
    roundings, each <= u = eps / 2 relative, then one addition into v (<= u |v_k|, |v_k| <= K dt |g|): |v_K - K dt g| <= (3 + K) u K dt |g|
    =: E_v.  p adds fl(dt v_k) (u relative, on top of dt E_v) K times, each addition <= u |p_k|:
    with D = dt^2 |g| K (K + 1) / 2 the distance fallen, |p_K - exact| <= K dt E_v + u D + K u (|p_0| + D)."""
    K, dt, u = 60, 1e-3, EPS / 2
    g = np.array([0.3, -0.2, -9.81])
    for exe in exes:
        c = _blank(3, 1, 1, 8)
        c["grav"], c["dt"] = g, dt
        c["inertial"] = np.array([0.7, 1e-3, 2e-3, 3e-3])
        c["state"][:, 0:3] = [[0.0, 0.0, 1.0], [0.3, -0.2, 2.0], [1.0, 1.0, 1.0]]
        p0 = c["state"][:, 0:3].copy()
        x = _advance(exe, c, tmp_path, K)[-1]["state"]
        ld = np.longdouble
        v_exact = K * ld(dt) * g.astype(ld)
        p_exact = p0.astype(ld) + ld(dt) * ld(dt) * g.astype(ld) * (K * (K + 1) // 2)
        E_v = (3 + K) * u * K * dt * np.abs(g)
        D = dt * dt * np.abs(g) * (K * (K + 1) // 2)
        E_p = K * dt * E_v + u * D + K * u * (np.abs(p0) + D)
        ev, ep = np.abs(x[:, 7:10] - v_exact).astype(float), np.abs(x[:, 0:3] - p_exact).astype(float)
        print(f"free fall, {K} substeps: worst |v - K dt g| = {ev.max():.3e} (bound {E_v.max():.3e}), worst |p - closed form| = {ep.max():.3e} (bound {E_p.max():.3e})")
        assert (ev <= E_v).all() and (ep <= E_p).all() and (x[:, 3:7] == [1, 0, 0, 0]).all() and not x[:, 10:13].any()


def test_torque_free_body_with_equal_moments_keeps_omega(exes, tmp_path):
    rng = np.random.default_rng(3)
    for exe in exes:
        c = _blank(5, 1, 1, 8)
        c["grav"], c["inertial"], c["dt"] = np.array([0.0, 0.0, -9.81]), np.array([0.4, 2.5e-3, 2.5e-3, 2.5e-3]), 1e-2
        c["state"][:, 3:7], c["state"][:, 10:13] = _quat(rng, 5), rng.normal(size=(5, 3)) * 3.0
        om, q0 = c["state"][:, 10:13].copy(), c["state"][:, 3:7].copy()
        x = _advance(exe, c, tmp_path, 25)[-1]["state"]
        assert (x[:, 10:13].view(np.uint64) == om.view(np.uint64)).all()
        assert np.abs(np.linalg.norm(x[:, 3:7], axis=1) - 1.0).max() <= 4 * EPS and (np.abs((x[:, 3:7] * q0).sum(axis=1)) < 0.999).all()       # it turns, at unit length


def test_reaction_is_the_exact_negation_of_the_object_items(exes, tmp_path):
    """S = 8: every lane owns one robot sphere, no world obstacle is near, so F_s of lane l is the sum of its object items and the lane's
    reaction is its negation, item by item; the folded reaction is the negation of the F_s folded in the same shape (4, 2, 1)"""
    c = _case("tree", 21, 12, 8, 1, False, 8, True)
    c["obst"], c["mat"] = np.array([[1, 0.0, 0.0, 1.0, -50.0, 0, 0, 0]]), np.array([[1e4, 0.0, 0.0, 0.0]])
    for exe in exes:
        got = _run(exe, c, tmp_path)
        v = [got["F"][:, c["order"][l]] for l in range(8)]
        for off in (4, 2, 1):
            for l in range(off):
                v[l] = v[l] + v[l + off]
        assert (got["readout"][:, 0:3] == -v[0]).all() and (got["readout"][:, 11] > 0).sum() >= 6 and not got["readout_lc"][:, 5].any()


def test_plate_rests_on_a_half_space(exes, tmp_path):
    """A plate of four spheres on the half-space z >= 0, stiffness k per sphere, released at d = 0: the vertical oscillator m z'' = 4 k pen -
    4 c z' - m g, critically damped with c = sqrt(k m) per sphere (4 c = 2 sqrt(4 k m)); it rests at the penetration m g / (4 k).  The bound
    is the residual of the critically damped semi-implicit step after T = K dt from a start 2 m g / (4 k) away (the derivation of
    tests/test_gpu_link_contact.py::test_drop_on_a_half_space), plus 1e-12 m for the roundings of K substeps of millimetre-sized terms.
    K = 400 runs of the program, one per substep: the plain build only (the sanitizer build starts several times slower, and the bit-for-bit
    cases above already put every function of the header through it)."""
    m, k, g, r, a, dt, K = 0.8, 1.0e4, 9.81, 0.02, 0.05, 5e-4, 400
    cs, om = np.sqrt(k * m), np.sqrt(4 * k / m)
    c = _blank(2, 1, 1, 4)
    c["obst"], c["mat"] = np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]]), np.array([[k, cs, 0.5, 1e-3]])
    c["shape_r"], c["shape_radius"] = np.array([[a, a, 0.0], [-a, -a, 0.0], [a, -a, 0.0], [-a, a, 0.0]]), np.full(4, r)
    c["grav"], c["dt"], c["inertial"] = np.array([0.0, 0.0, -g]), dt, np.array([m, 1e-3, 1e-3, 2e-3])
    c["state"][:, 2] = r
    c["state"][1, 0:2] = [0.4, -0.3]
    outs = _advance(exes[0], c, tmp_path, K)
    x, rq = outs[-1]["state"], outs[-1]["readout"]
    T, al = K * dt, om * dt
    resid = 2.0 * (1.0 + om * T) * np.exp(-om * T * (1.0 - 1.01 * np.sqrt(al) - al)) * (2 * m * g / (4 * k))
    pen = r - x[:, 2]
    print(f"plate: worst |penetration - m g / (4 k)| = {np.abs(pen - m * g / (4 * k)).max():.3e} (m g / 4 k = {m * g / (4 * k):.3e}, bound {resid + 1e-12:.3e})")
    assert resid < 0.05 * m * g / (4 * k) and np.abs(pen - m * g / (4 * k)).max() <= resid + 1e-12
    assert np.abs(rq[:, 8] - m * g).max() <= (4 * k + 4 * cs * om) * (resid + 1e-12) and np.abs(x[:, 10:13]).max() < 1e-9        # the wall carries the weight, level
    assert (outs[-1]["osummary"][:, 2] >= pen - resid).all() and not outs[-1]["osummary"][:, [0, 1, 3]].any()


def test_momentum_is_conserved_through_a_collision(exes, tmp_path):
    """A slider of mass M (one prismatic joint along z, one sphere) runs into a one-sphere object of mass m at rest; no gravity, no damping,
    no friction.  Per substep the slider gains dt tau_sim / M with tau_sim = 0 + a . F_s = F_z and the object dt ((0 + 0) + (-F_z)) / m:
    the momentum M dq + m v_z changes only by roundings -- on each side the division, the product with dt and the addition, and the
    product with the mass when the momentum is formed: <= 4 eps |dt F| per side and substep, and eps of the momentum held, per substep:
    |P_K - P_0| <= 8 eps sum |dt F_k| + K eps (M max|dq| + m max|v_z|).  240 runs of the program: the plain build only, as for the plate."""
    M, m, k, dt, K, r = 2.0, 0.5, 2.0e4, 5e-4, 240, 0.05
    c = _blank(3, 1, 1, 1)
    c.update(n=1, anc=[1], jtype=[2], order=[0], aw=np.tile([0.0, 0.0, 1.0], (3, 1, 1)), oj=np.zeros((3, 1, 3)), tau=np.zeros((3, 1)))
    c["radii"], c["shape_radius"], c["omat"], c["dt"] = np.array([r]), np.array([r]), np.array([k, 0.0, 0.0, 0.0]), dt
    c["inertial"] = np.array([m, 1e-3, 1e-3, 1e-3])
    q, dq = np.array([-0.13, -0.12, -0.11]), np.array([0.5, 0.8, 1.1])
    P0 = M * dq
    sumF, hold = np.zeros(3), np.zeros(3)
    for _ in range(K):
        c["centres"][:, 0], c["vels"][:, 0] = np.stack([0 * q, 0 * q, q], axis=1), np.stack([0 * q, 0 * q, dq], axis=1)
        got = _run(exes[0], c, tmp_path)
        dq = dq + dt * (got["tau"][:, 0] / M)
        q = q + dt * dq
        c["state"], c["osummary"] = got["state"], got["osummary"]
        sumF += np.abs(dt * got["tau"][:, 0])
        hold = np.maximum(hold, M * np.abs(dq) + m * np.abs(c["state"][:, 9]))
    P = M * dq + m * c["state"][:, 9]
    bound = 8 * EPS * sumF + K * EPS * hold
    print(f"collision: worst |P_K - P_0| = {np.abs(P - P0).max():.3e} kg m/s (bound {bound.min():.3e}), impulse {sumF}")
    assert (np.abs(P - P0) <= bound).all() and (sumF > 0.1).all()
    assert (c["state"][:, 9] > dq).all() and (c["state"][:, 2] - q > 2 * r).all() and (c["osummary"][:, 3] > 3).all()          # the object moves away, after a real contact
