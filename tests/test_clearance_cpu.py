"""The clearance monitor, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument and call-order errors
come back with the documented codes before the device is needed; the Python facade raises the same; the host build of
csrc/saip_clearance.h (tests/cpp/clearance_host.cpp, also under ASan/UBSan) matches the NumPy restatement tests/clearance_ref.py bit for
bit in every output; the restatement has the properties of a signed distance."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import clearance_ref as CL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_clearance_attach", "saip_batch_clearance_detach", "saip_batch_clearance_info", "saip_batch_clearance_set_obstacles_host",
                  "saip_batch_clearance_evaluate", "saip_batch_clearance_readout_host", "saip_batch_clearance_summary_host",
                  "saip_batch_clearance_summary_reset", "saip_batch_clearance_add_cost"]
POINTER_ENTRIES = ["saip_batch_clearance_obstacles_device", "saip_batch_clearance_readout_device", "saip_batch_clearance_summary_device",
                   "saip_batch_clearance_centres_device"]


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
    for name, val in [("MAX_SPHERES", 32), ("MAX_OBSTACLES", 16), ("MAX_PAIRS", 64), ("OBSTACLE_WORDS", 8), ("READOUT_ROWS", 8), ("SUMMARY_ROWS", 4)]:
        assert re.search(rf"#define SAIP_CLEARANCE_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_CLEARANCE_" + name) == val == getattr(CL, name)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert "csrc/saip_clearance.hip" in capi.SOURCES and "csrc/saip_clearance.h" in capi.HEADERS


def _controller_batch(sp, L, B=4):
    """an unfinalized configuration-only batch with tasks 0 (motion-force) and 1 (joint)"""
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, B, -1, C.byref(b)) == 0
    pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
    assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
    assert L.saip_batch_add_joint_task(b, b"jt", None, 0, 0.001, C.byref(tid)) == 0
    return robot, b


def _others_refuse(L, b, code):
    v, out = C.c_int(7), np.full(8 * 4, 7.0)
    assert L.saip_batch_clearance_detach(b) == code
    assert L.saip_batch_clearance_info(b, C.byref(v), None, None, None, None, None, None) == code
    assert L.saip_batch_clearance_set_obstacles_host(b, _dp(out)) == code
    assert L.saip_batch_clearance_evaluate(b) == code
    assert L.saip_batch_clearance_readout_host(b, _dp(out)) == code
    assert L.saip_batch_clearance_summary_host(b, _dp(out)) == code
    assert L.saip_batch_clearance_summary_reset(b) == code
    assert L.saip_batch_clearance_add_cost(b, 1.0, np.inf, 0.0) == code
    for name in POINTER_ENTRIES:
        assert getattr(L, name)(b) is None
    assert v.value == 7 and (out == 7.0).all()      # nothing was written


OBST = np.array([[0, 0.4, 0.0, 0.3, 0.4, 0.2, 0.6, 0.05], [1, 0.0, 0.0, 1.0, 0.1, 9.0, 9.0, 9.0], [0, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.0]])


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_clearance_attach
    links = np.array([1, 3, 5], np.int32)
    cen = np.array([[0.0, 0.0, 0.05], [0.01, 0.0, 0.0], [0.0, 0.0, 0.0]])
    rad = np.array([0.08, 0.06, 0.0])
    pairs = np.array([[0, 2], [2, 1]], np.int32)

    def call(b, S=3, links=links, cen=cen, rad=rad, O=3, obst=OBST, per=0, P=2, pairs=pairs, margin=0.05, keep=0):
        return att(b, S, None if links is None else _ip(links), None if cen is None else _dp(cen), None if rad is None else _dp(rad), O,
                   None if obst is None else _dp(obst), per, P, None if pairs is None else _ip(pairs), margin, keep)

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
        for O in (-1, 17):
            refused(b, b"obstacles required", O=O)
        for P in (-1, 65):
            refused(b, b"pairs required", P=P)
        refused(b, b"0 obstacles and 0 pairs", O=0, P=0)
        refused(b, b"null links", links=None)
        refused(b, b"null links", cen=None)
        refused(b, b"null links", rad=None)
        refused(b, b"null obstacles", obst=None)
        refused(b, b"null pairs", pairs=None)
        for m in (-1e-9, np.nan, np.inf):
            refused(b, b"margin", margin=m)
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
        for bad, msg in (([0, 3], b"pair 1: sphere index"), ([-1, 0], b"pair 1: sphere index"), ([2, 2], b"pair 1: sphere 2 against itself")):
            p2 = pairs.copy()
            p2[1] = bad
            refused(b, msg, pairs=p2)
        # one bad word of one obstacle, batch-uniform and per instance (there: of one instance only)
        per = np.ascontiguousarray(np.repeat(OBST[:, :, None], B, axis=2))
        cases = [(0, 2, np.nan, b"obstacle 0: word 2 is not finite"), (1, 7, np.inf, b"obstacle 1: word 7 is not finite"),
                 (0, 7, -0.01, b"obstacle 0: radius"), (2, 0, 2.0, b"obstacle 2: unknown kind"), (2, 0, 0.5, b"obstacle 2: unknown kind"),
                 (2, 0, -1.0, b"obstacle 2: unknown kind"), (1, 3, 1.0 + 3e-6, b"obstacle 1: the half-space normal"),
                 (1, 3, 1.0 - 3e-6, b"obstacle 1: the half-space normal"), (1, 3, 0.0, b"obstacle 1: the half-space normal")]
        for o, word, val, msg in cases:
            o1 = OBST.copy()
            o1[o, word] = val
            refused(b, msg, obst=o1)
            o2 = per.copy()
            o2[o, word, B - 1] = val
            refused(b, msg.replace(b":", b" of instance 3:", 1), obst=o2, per=1)
        ok = OBST.copy()
        ok[1, 3] = 1.0 + 5e-7                                            # within 1e-6 of unit length
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        for kw in (dict(), dict(obst=ok), dict(obst=per, per=1), dict(O=0, obst=None), dict(P=0, pairs=None), dict(keep=1), dict(margin=0.0), dict(S=1, P=0)):
            assert call(b, **kw) == NO_DEVICE and b"no CPU path" in L.saip_last_error(), kw
        S, Pm = 32, 64
        big = (np.arange(S, dtype=np.int32) % 8, np.zeros((S, 3)), np.full(S, 0.01), np.array([[i % 32, (i + 1 + i // 32) % 32] for i in range(Pm)], np.int32))
        assert call(b, S=S, links=big[0], cen=big[1], rad=big[2], O=16, obst=np.ascontiguousarray(np.tile(OBST, (6, 1))[:16]), P=Pm, pairs=big[3]) == NO_DEVICE
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_clearance(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        links, cen, rad = np.array([1], np.int32), np.zeros((1, 3)), np.array([0.1])
        assert L.saip_batch_clearance_attach(b, 1, _ip(links), _dp(cen), _dp(rad), 3, _dp(OBST), 0, 0, None, 0.0, 0) == capi.SAIP_ERR_ORDER
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
            ctrl.attachClearance(sph, bad)
    for bad in (np.zeros((2, 8)), np.zeros((2, 8, B)), np.zeros((2, B + 1, 8))):
        with pytest.raises(ValueError, match="per-instance obstacles of shape"):
            ctrl.attachClearance(sph, bad, per_instance=True)
    with pytest.raises(ValueError, match="unknown link"):
        ctrl.attachClearance([("no-such-link", (0, 0, 0), 0.1)], OBST)
    with pytest.raises(ValueError, match="centre of shape"):
        ctrl.attachClearance([("link4", (0, 0), 0.1)], OBST)
    with pytest.raises(ValueError, match="pairs of shape"):
        ctrl.attachClearance(sph, OBST, pairs=[0, 1, 1])
    with pytest.raises(ValueError, match="sphere 1: radius"):
        ctrl.attachClearance([sph[0], ("link5", (0, 0, 0), -0.1)], OBST)
    with pytest.raises(ValueError, match="0 obstacles and 0 pairs"):
        ctrl.attachClearance(sph)
    with pytest.raises(ValueError, match="margin"):
        ctrl.attachClearance(sph, OBST, margin=-1.0)
    with pytest.raises(ValueError, match="against itself"):
        ctrl.attachClearance(sph, pairs=[(1, 1)])
    for per in (False, True):
        ob = np.ascontiguousarray(np.repeat(OBST[:, None, :], B, axis=1)) if per else OBST
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            ctrl.attachClearance(sph, ob, pairs=[(0, 1)], margin=0.05, per_instance=per, keep_centres=True)
    for fn in (ctrl.detachClearance, ctrl.clearanceInfo, ctrl.evaluateClearance, ctrl.clearanceReadout, ctrl.clearanceSummary, ctrl.resetClearanceSummary,
               lambda: ctrl.clearanceCost(1.0), lambda: ctrl.setClearanceObstacles(OBST)):
        with pytest.raises(sp.SaipError, match="no clearance monitor is attached"):
            fn()
    assert ctrl.clearanceCentresDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "clearance_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("clearance_host"), "clearance_host", []),
            _build(tmp_path_factory.mktemp("clearance_host_san"), "clearance_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _rotations(rng, N):
    Q = np.linalg.qr(rng.normal(size=(N, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q.reshape(N, 9)


def _obstacles(rng, shape):
    """mixed kinds: capsules (a quarter of them degenerate, a == b) and half-spaces through the cloud of centres"""
    ob = np.zeros(shape + (8,))
    ob[..., 1:7] = rng.uniform(-0.6, 0.6, shape + (6,))
    ob[..., 7] = rng.uniform(0.0, 0.1, shape)
    deg = rng.random(shape) < 0.25
    ob[..., 4:7] = np.where(deg[..., None], ob[..., 1:4], ob[..., 4:7])
    hs = rng.random(shape) < 0.35
    n = rng.normal(size=shape + (3,))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    ob[..., 0] = hs
    ob[..., 1:4] = np.where(hs[..., None], n, ob[..., 1:4])
    ob[..., 4] = np.where(hs, rng.uniform(-0.5, 0.1, shape), ob[..., 4])
    return ob


def _case(seed, N, S, O, P, per):
    rng = np.random.default_rng(seed)
    c = dict(N=N, S=S, O=O, P=P, per=per, margin=0.08, dt=2e-3, period=float(seed % 5), w=(3.0, 1e3, 0.01))
    c["centres"] = rng.uniform(-0.5, 0.5, (N, S, 3))
    c["radii"] = rng.uniform(0.0, 0.1, S) * (rng.random(S) < 0.9)
    c["obst"] = _obstacles(rng, (N, O) if per else (O,))
    if P:
        s1 = rng.integers(0, S, P)
        c["pairs"] = np.stack([s1, (s1 + rng.integers(1, S, P)) % S], axis=1)
    else:
        c["pairs"] = np.zeros((0, 2), int)
    s = CL.summary_reset(N)
    seen = rng.random(N) < 0.6                        # instances that have been monitored before, some of them in collision
    s[seen, 0] = rng.uniform(-0.05, 0.3, seen.sum())
    s[seen, 1] = np.abs(rng.normal(size=seen.sum())) * 1e-3
    hit = seen & (s[:, 0] < 0)
    s[hit, 2], s[hit, 3] = rng.integers(1, 4, hit.sum()), rng.integers(0, 3, hit.sum())
    c["summary"] = s
    c["cost"] = rng.normal(size=N)
    c["o"], c["R"], c["r"] = rng.uniform(-1, 1, (N, 3)), _rotations(rng, N), rng.uniform(-0.2, 0.2, (N, 3))
    return c


def _run(exe, c, tmp):
    N, S, O, P = c["N"], c["S"], c["O"], c["P"]
    obst = np.ascontiguousarray(c["obst"].transpose(1, 2, 0)) if c["per"] else c["obst"]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, S, O, P, int(c["per"])], np.int32).tobytes())
        f.write(np.ascontiguousarray(c["pairs"], np.int32).tobytes())
        f.write(np.array([c["margin"], c["dt"], c["period"], *c["w"]], float).tobytes())
        for a in (c["centres"], c["radii"], obst, np.ascontiguousarray(c["summary"].T), c["cost"], c["o"], c["R"], c["r"]):
            f.write(np.ascontiguousarray(a, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    assert raw.size == 8 * N + 4 * N + N + 3 * N
    return dict(readout=raw[:8 * N].reshape(N, 8), summary=raw[8 * N:12 * N].reshape(4, N).T, cost=raw[12 * N:13 * N], c=raw[13 * N:].reshape(N, 3))


def _ref(c):
    ro = CL.evaluate(c["centres"], c["radii"], c["obst"], c["pairs"], c["margin"])
    s = CL.summary_advance(c["summary"], c["dt"], ro[:, 0], ro[:, 2], c["period"])
    return dict(readout=ro, summary=s, cost=CL.add_cost(c["cost"], s[:, 0], s[:, 1], *c["w"]), c=CL.centre(c["o"], c["R"], c["r"]))


def _same_bits(got, ref, what):
    for key in ref:
        a, b = np.ascontiguousarray(got[key], float), np.ascontiguousarray(ref[key], float)
        same = (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
        assert same.all(), (what, key, np.argwhere(~same)[:4], a[~same][:4], b[~same][:4])


def _check(exes, c, tmp, what):
    ref = _ref(c)
    for exe in exes:
        _same_bits(_run(exe, c, tmp), ref, what)
    return ref


SHAPES = [(S, O, P) for S in (1, 7, 8, 9, 32) for O in (0, 1, 16) for P in (0, 1, 64) if (O or P) and (P == 0 or S > 1)]


def test_host_build_matches_restatement_random(exes, tmp_path):
    """S in {1, 7, 8, 9, 32} x O in {0, 1, 16} x P in {0, 1, 64}, O and P not both 0 (a pair needs two spheres: none at S = 1),
    batch-uniform and per-instance tables"""
    assert len(SHAPES) == 5 * 8 - 2 * 3
    for i, (S, O, P) in enumerate(SHAPES):
        for per in (False, True):
            c = _case(100 + i, 24, S, O, P, per)
            ref = _check(exes, c, tmp_path, (S, O, P, per))
            if O == 16 and S >= 7:
                assert (ref["readout"][:, 3] > 0).any() and (ref["readout"][:, 0] < 0).any()     # the cases reach the margin and penetrate


def _blank(N, S, O, P, margin=0.05):
    c = _case(7, N, S, O, P, False)
    c["margin"] = margin
    c["summary"] = CL.summary_reset(N)
    return c


def test_host_build_matches_restatement_edges(exes, tmp_path):
    # degenerate capsules (a == b), a centre exactly on a capsule axis, t clamped at both ends
    c = _blank(6, 2, 3, 0)
    c["obst"] = np.array([[0, 0.1, 0.2, 0.3, 0.1, 0.2, 0.3, 0.02], [0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.01], [0, -0.5, 0.0, 0.25, 0.5, 0.0, 0.25, 0.0]])
    c["radii"] = np.array([0.03, 0.0])
    c["centres"][:, 0] = [[0.1, 0.2, 0.3], [0.25, 0.0, 0.0], [-2.0, 0.5, 0.0], [3.0, -0.5, 0.0], [0.0, 0.0, 0.25], [0.5, 0.125, 0.0]]
    c["centres"][:, 1] = c["centres"][::-1, 0]
    ref = _check(exes, c, tmp_path, "capsule edges")
    d = CL.item_distances(c["centres"], c["radii"], c["obst"])
    assert d[0, 0] == -(0.03 + 0.02)                                  # at the centre of a point obstacle
    assert d[1, 1] == -(0.03 + 0.01) and d[4, 2] == -(0.03 + 0.0)     # on the axis
    assert d[2, 1] == np.sqrt(4.0 + 0.25) - (0.03 + 0.01)             # t clamped to 0 ...
    assert d[3, 1] == np.sqrt(4.0 + 0.25) - (0.03 + 0.01)             # ... and to 1
    assert (ref["readout"][:, 7] == np.inf).all()                     # no pairs
    # an item exactly at dist == margin: no penalty, not under the margin
    c = _blank(3, 1, 1, 0, margin=0.125)
    c["radii"], c["obst"] = np.array([0.125]), np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]])
    c["centres"][:, 0] = [[0.3, 0.1, 0.25], [0.3, 0.1, 0.25 - 2.0 ** -40], [0.3, 0.1, 0.5]]
    ref = _check(exes, c, tmp_path, "dist == margin")
    assert ref["readout"][0, 0] == 0.125 and ref["readout"][0, 2] == 0.0 and ref["readout"][0, 3] == 0
    assert ref["readout"][1, 2] > 0.0 and ref["readout"][1, 3] == 1 and ref["readout"][2, 3] == 0
    # two items with the same distance: the lower k wins, inside one lane (k = 3 and 11) and across lanes (k = 5 and 10; 2 and 7)
    for ks in ((3, 11), (5, 10), (2, 7), (0, 15), (9, 1)):
        c = _blank(2, 16, 1, 0)
        c["obst"], c["radii"] = np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]]), np.zeros(16)
        c["centres"][:, :, 2] = 0.5 + 0.01 * np.arange(16)
        for k in ks:
            c["centres"][:, k] = [0.1 * k, -0.2, 0.25]                # two spheres at the same height, the lowest of all
        ref = _check(exes, c, tmp_path, ("tie", ks))
        assert (ref["readout"][:, 1] == min(ks)).all() and (ref["readout"][:, 0] == 0.25).all()
        assert (ref["readout"][:, 4] == 0.1 * min(ks)).all()
    # ties among pairs, and between an obstacle item and a pair item
    c = _blank(2, 4, 1, 3)
    c["obst"], c["radii"] = np.array([[1, 0.0, 0.0, 1.0, 0.0, 0, 0, 0]]), np.zeros(4)
    c["centres"][:] = [[0, 0, 0.5], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0.5, 0.75]]
    c["pairs"] = np.array([[3, 2], [0, 1], [2, 0]])
    ref = _check(exes, c, tmp_path, "pair ties")
    assert (ref["readout"][:, 1] == 0).all() and (ref["readout"][:, 7] == 0.5).all()
    c["centres"][:, :, 2] += 1.0
    ref = _check(exes, c, tmp_path, "pair ties 2")
    assert (ref["readout"][:, 1] == 5).all() and (ref["readout"][:, 4:7] == [0, 0, 1.5]).all()       # pair (0, 1): k = 4 + 1, its first sphere
    # a NaN / infinite centre: the instance is invalid, its neighbours are not
    for bad in (np.nan, np.inf, -np.inf):
        c = _case(11, 5, 9, 2, 3, True)
        c["centres"][1, 8, 2] = bad
        c["centres"][3, 0, 0] = bad
        ref = _check(exes, c, tmp_path, ("invalid", bad))
        ro = ref["readout"]
        for i in (1, 3):
            assert np.isnan(ro[i, [0, 2, 4, 5, 6, 7]]).all() and ro[i, 1] == -1 and ro[i, 3] == 0
            assert np.isnan(ref["summary"][i, 0]) and np.isnan(ref["summary"][i, 1]) and np.isnan(ref["cost"][i])
        assert np.isfinite(ro[[0, 2, 4]]).all() and np.isfinite(ref["cost"][[0, 2, 4]]).all()


def test_summary_and_cost_rules():
    s = CL.summary_reset(5)
    assert (s == [np.inf, 0, 0, -1]).all()
    dmins = np.array([[0.2, 0.1, -0.1, np.nan, 0.3], [0.1, -0.2, 0.05, 0.1, 0.3], [0.3, -0.3, -0.2, 0.1, 0.3]])
    pens = np.array([[0.0, 0.1, 0.4, np.nan, 0.0], [0.1, 0.5, 0.2, 0.1, 0.0], [0.0, 0.6, 0.5, 0.1, 0.0]])
    for p in range(3):
        s = CL.summary_advance(s, 0.5, dmins[p], pens[p], p)
    assert (s[[0, 1, 2, 4], 0] == [0.1, -0.3, -0.2, 0.3]).all() and np.isnan(s[3, 0])          # NaN is sticky
    assert np.allclose(s[[0, 1, 2, 4], 1], [0.05, 0.6, 0.55, 0.0], rtol=1e-15, atol=0) and np.isnan(s[3, 1])
    assert (s[:, 2] == [0, 2, 2, 0, 0]).all() and (s[:, 3] == [-1, 1, 0, -1, -1]).all()
    cost = CL.add_cost(np.ones(5), s[:, 0], s[:, 1], 2.0, np.inf, 0.15)
    assert cost[0] == np.inf and cost[1] == np.inf and cost[2] == np.inf and np.isnan(cost[3]) and cost[4] == 1.0
    cost = CL.add_cost(np.ones(5), s[:, 0], s[:, 1], 2.0, 10.0, 0.0)
    assert np.allclose(cost[[0, 1, 2, 4]], [1.1, 12.2, 12.1, 1.0], rtol=1e-15, atol=0) and np.isnan(cost[3])
    assert np.isnan(CL.add_cost(np.ones(1), np.array([np.nan]), np.array([0.0]), 0.0, 0.0, 0.0))[0]


def test_restatement_properties():
    rng = np.random.default_rng(5)
    N, S, O, P = 64, 12, 7, 9
    c = _case(21, N, S, O, P, True)
    d = CL.item_distances(c["centres"], c["radii"], c["obst"], c["pairs"])
    ro = CL.evaluate(c["centres"], c["radii"], c["obst"], c["pairs"], c["margin"])
    # the minimum is the brute-force minimum over the items, at the first item that attains it
    assert (ro[:, 0] == d.min(axis=1)).all() and (ro[:, 1] == d.argmin(axis=1)).all()
    assert (ro[:, 7] == d[:, S * O:].min(axis=1)).all()
    assert (ro[:, 3] == (d < c["margin"]).sum(axis=1)).all()
    # the penalty is 0 iff nothing is under the margin
    for margin in (0.0, 0.02, 0.08, 0.5):
        r = CL.evaluate(c["centres"], c["radii"], c["obst"], c["pairs"], margin)
        assert ((r[:, 2] == 0.0) == (r[:, 3] == 0)).all() and (r[:, 2] >= 0).all()
    # the penalty is the plain sum within rounding
    pen = (np.maximum(0.0, c["margin"] - d) ** 2).sum(axis=1)
    assert np.allclose(ro[:, 2], pen, rtol=1e-13, atol=0)
    # translating everything leaves the distances within rounding: coordinates up to ~4 after the shift, a handful of roundings of 2^-53
    # relative each on values up to ~16 (the squares): 1e-14 absolute is a factor of ten over that
    t = rng.uniform(-3, 3, 3)
    ob = c["obst"].copy()
    hs = ob[..., 0] == 1
    ob[..., 1:4] = np.where(hs[..., None], ob[..., 1:4], ob[..., 1:4] + t)
    ob[..., 4:7] = np.where(hs[..., None], ob[..., 4:7], ob[..., 4:7] + t)
    ob[..., 4] = np.where(hs, c["obst"][..., 4] + c["obst"][..., 1:4] @ t, ob[..., 4])
    d2 = CL.item_distances(c["centres"] + t, c["radii"], ob, c["pairs"])
    assert np.abs(d2 - d).max() < 1e-14
    # a sphere obstacle is the pair formula
    a = rng.uniform(-1, 1, (N, 1, 3))
    sph = np.zeros((N, 1, 8))
    sph[:, 0, 1:4], sph[:, 0, 4:7], sph[:, 0, 7] = a[:, 0], a[:, 0], 0.07
    d3 = CL.item_distances(c["centres"][:, :1], c["radii"][:1], sph)
    assert (d3[:, 0] == CL.pair_dist(c["centres"][:, 0], c["radii"][0], a[:, 0], 0.07)).all()
    # decode
    assert CL.decode(-1, S, O, c["pairs"]) is None and CL.decode(O + 2, S, O, c["pairs"]) == ("obstacle", 1, 2)
    assert CL.decode(S * O + 3, S, O, c["pairs"]) == ("pair", int(c["pairs"][3, 0]), int(c["pairs"][3, 1]))
