"""Contact patches, host side (no GPU needed): the C-ABI entries are declared, exported and bound; argument and call-order errors come back
with the documented codes before the device is needed; the Python facade raises the same; the host build of csrc/saip_contact_patch.h
(tests/cpp/contact_patch_host.cpp, also under ASan/UBSan) matches the NumPy restatement tests/contact_patch_ref.py bit for bit in every
readout row, summary row, tau_sim entry and sensor row; a one-point patch gives what ct_plane_forces, ct_joint_torque and ct_sensor give."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contact_patch_ref as PR
import contact_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_contact_patch_attach", "saip_batch_contact_patch_detach", "saip_batch_contact_patch_info",
                  "saip_batch_contact_patch_set_planes_host", "saip_batch_contact_patch_sense", "saip_batch_contact_patch_readout_host",
                  "saip_batch_contact_patch_summary_host", "saip_batch_contact_patch_summary_reset"]
POINTER_ENTRIES = ["saip_batch_contact_patch_planes_device", "saip_batch_contact_patch_readout_device", "saip_batch_contact_patch_summary_device",
                   "saip_batch_contact_patch_torques_device"]
GOOD = np.array([[0.0, 0.0, 2.0, 0.1, 1e4, 50.0, 0.5, 1e-3], [1.0, 1.0, 0.0, -0.3, 2e3, 0.0, 0.0, 1e-2]])
SQUARE = np.array([[0.05, 0.05, 0.0], [-0.05, 0.05, 0.0], [-0.05, -0.05, 0.0], [0.05, -0.05, 0.0]])


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    for name, val in [("MAX_POINTS", 8), ("MAX", 2), ("READOUT_ROWS", 20), ("SUMMARY_ROWS", 6)]:
        assert re.search(rf"#define SAIP_CONTACT_PATCH_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_CONTACT_PATCH_" + name) == val
    assert (PR.MAX_POINTS, PR.MAX_PATCHES, PR.READOUT_ROWS, PR.SUMMARY_ROWS) == (8, 2, 20, 6)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert "csrc/saip_contact_patch.hip" in capi.SOURCES and "csrc/saip_contact_patch.h" in capi.HEADERS


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
    v, out = C.c_int(7), np.full(20 * 4, 7.0)
    for task in (-1, 0):
        assert L.saip_batch_contact_patch_detach(b, task) == code
        assert L.saip_batch_contact_patch_info(b, task, C.byref(v), None, None, None, None, None) == code
        assert L.saip_batch_contact_patch_set_planes_host(b, task, _dp(out)) == code
        assert L.saip_batch_contact_patch_readout_host(b, task, _dp(out)) == code
        assert L.saip_batch_contact_patch_summary_host(b, task, _dp(out)) == code
        assert L.saip_batch_contact_patch_summary_reset(b, task) == code
        for name in POINTER_ENTRIES[:3]:
            assert getattr(L, name)(b, task) is None
    assert L.saip_batch_contact_patch_sense(b) == code
    assert L.saip_batch_contact_patch_torques_device(b) is None
    assert v.value == 7 and (out == 7.0).all()      # nothing was written


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_contact_patch_attach
    pts = np.ascontiguousarray(SQUARE)
    assert att(None, 0, 4, _dp(pts), 2, _dp(GOOD), 0, 1) == INVALID
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert att(b, 0, 4, _dp(pts), 2, _dp(GOOD), 0, 1) == ORDER           # before finalize, whatever the arguments
        assert att(b, 9, 0, None, 0, None, 0, 0) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for task in (-1, 2, 7):
            assert att(b, task, 4, _dp(pts), 2, _dp(GOOD), 0, 1) == INVALID and b"out of range" in L.saip_last_error()
        assert att(b, 1, 4, _dp(pts), 2, _dp(GOOD), 0, 1) == INVALID and b"not a motion-force task" in L.saip_last_error()
        for n in (0, -1, 9, 2**31 - 1):
            assert att(b, 0, n, _dp(pts), 2, _dp(GOOD), 0, 1) == INVALID and b"points required" in L.saip_last_error()
        assert att(b, 0, 4, None, 2, _dp(GOOD), 0, 1) == INVALID and b"null points" in L.saip_last_error()
        for bad in (np.nan, np.inf, -np.inf):
            p2 = pts.copy()
            p2[3, 1] = bad                                                    # the last point only
            assert att(b, 0, 4, _dp(p2), 2, _dp(GOOD), 0, 1) == INVALID and b"not finite" in L.saip_last_error()
            assert att(b, 0, 3, _dp(p2), 2, _dp(GOOD), 0, 1) == NO_DEVICE    # ... which a three-point patch does not read
        for P in (0, -1, 5, 2**31 - 1):
            assert att(b, 0, 4, _dp(pts), P, _dp(GOOD), 0, 1) == INVALID and b"planes required" in L.saip_last_error()
        assert att(b, 0, 4, _dp(pts), 2, None, 0, 1) == INVALID and b"null planes" in L.saip_last_error()
        # the plane checks are those of saip_batch_contact_attach: one bad word of one plane, batch-uniform and per instance
        cases = [(0, np.nan, b"not finite"), (3, np.inf, b"not finite"), (4, 0.0, b"k > 0"), (5, -1e-9, b"c >= 0"), (6, -0.1, b"mu >= 0"),
                 (7, 0.0, b"v_s > 0")]
        per = np.ascontiguousarray(np.repeat(GOOD[:, :, None], B, axis=2))
        for word, val, msg in cases:
            p1 = GOOD.copy()
            p1[1, word] = val
            assert att(b, 0, 4, _dp(pts), 2, _dp(p1), 0, 1) == INVALID and msg in L.saip_last_error(), (word, val)
            p2 = per.copy()
            p2[1, word, B - 1] = val
            assert att(b, 0, 1, _dp(pts), 2, _dp(p2), 1, 0) == INVALID and msg in L.saip_last_error(), (word, val)
        z = GOOD.copy()
        z[0, :3] = 0.0
        assert att(b, 0, 4, _dp(pts), 2, _dp(z), 0, 1) == INVALID and b"normal is zero" in L.saip_last_error()
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        eight = np.ascontiguousarray(np.vstack([SQUARE, 0.5 * SQUARE]))
        for n, a in ((1, pts), (4, pts), (8, eight)):
            for sensor in (0, 1):
                assert att(b, 0, n, _dp(a), 2, _dp(GOOD), 0, sensor) == NO_DEVICE and b"no CPU path" in L.saip_last_error()
                assert att(b, 0, n, _dp(a), 2, _dp(per), 1, sensor) == NO_DEVICE
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_contact_attach(b, 0, None, 2, _dp(GOOD), 0, 1) == NO_DEVICE    # the single-point attach is not in the way
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_patches(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_contact_patch_attach(b, 0, 4, _dp(np.ascontiguousarray(SQUARE)), 2, _dp(GOOD), 0, 1) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    assert not hasattr(jt, "attachContactPatch")
    for bad in (np.zeros(3), np.zeros((4, 2)), np.zeros((2, 4, 3))):
        with pytest.raises(ValueError, match="points of shape"):
            mf.attachContactPatch(bad, GOOD)
    with pytest.raises(ValueError, match="planes of shape"):
        mf.attachContactPatch(SQUARE, np.zeros((2, 7)))
    with pytest.raises(ValueError, match="per-instance planes of shape"):
        mf.attachContactPatch(SQUARE, GOOD, per_instance=True)
    with pytest.raises(ValueError, match="points required"):
        mf.attachContactPatch(np.zeros((9, 3)), GOOD)
    with pytest.raises(ValueError, match="not finite"):
        mf.attachContactPatch([[0, np.nan, 0]], GOOD)
    with pytest.raises(ValueError, match="k > 0"):
        mf.attachContactPatch(SQUARE, np.array([[0, 0, 1, 0, 0, 0, 0, 1e-3]], float))
    for per in (False, True):
        planes = np.ascontiguousarray(np.repeat(GOOD[:, None, :], B, axis=1)) if per else GOOD
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            mf.attachContactPatch(SQUARE, planes, sensor=True, per_instance=per)
    for fn in (mf.detachContactPatch, mf.contactPatchReadout, mf.contactPatchSummary, mf.resetContactPatchSummary, mf.contactPatchInfo,
               ctrl.contactPatchSense, lambda: mf.setContactPatchPlanes(GOOD)):
        with pytest.raises(sp.SaipError, match="no contact patch is attached"):
            fn()
    assert mf.contactPatchPlanesDevice() is None and mf.contactPatchTorquesDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "contact_patch_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("contact_patch_host"), "contact_patch_host", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("contact_patch_host_san"), "contact_patch_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _rotations(rng, N):
    Q = np.linalg.qr(rng.normal(size=(N, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q.reshape(N, 9)


J = 9
# two bodies on different branches behind a common trunk (joints 0, 1); joint 8 is an ancestor of neither
ANC = [np.array([1, 1, 1, 1, 1, 0, 0, 0, 0], bool), np.array([1, 1, 0, 0, 0, 1, 1, 1, 0], bool)]


def _patch(rng, N, n_points, P, per):
    """one patch of N candidate cases: the control point within a few centimetres of a base point, the planes through its neighbourhood, so
    that instances with no, some and all points touching occur"""
    c = dict(n=n_points, P=P, per=per)
    c["points"] = rng.uniform(-0.06, 0.06, (n_points, 3))
    c["xc"] = rng.uniform(-0.5, 0.5, 3) + rng.uniform(-0.03, 0.03, (N, 3)) * (1.0 if per else 5.0)   # shared planes: the poses do the spreading
    near = rng.random((N, 1)) < 0.5                        # half the instances close to the identity: a patch that lies flat on a plane
    c["Rc"] = np.where(near, _rotations(rng, 1), _rotations(rng, N))
    c["Rcs"], c["tcs"] = _rotations(rng, N), rng.uniform(-0.1, 0.1, (N, 3))
    scale = 10.0 ** rng.uniform(-5, 0, (N, 1))
    c["tv"], c["tw"], c["tc"] = (rng.normal(size=(N, 3)) * scale for _ in range(3))
    M = N if per else 1
    nrm = rng.normal(size=(M, P, 3))
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    planes = np.zeros((M, P, 8))
    planes[..., :3] = nrm
    ref = c["xc"] if per else c["xc"].mean(axis=0, keepdims=True)
    planes[..., 3] = np.einsum("npe,ne->np", nrm, ref) + rng.uniform(-0.08, 0.05, (M, P))
    planes[..., 4] = 10.0 ** rng.uniform(2, 5, (M, P))
    planes[..., 5] = rng.uniform(0, 200, (M, P)) * (rng.random((M, P)) < 0.7)
    planes[..., 6] = rng.uniform(0, 1.2, (M, P)) * (rng.random((M, P)) < 0.8)
    planes[..., 7] = 10.0 ** rng.uniform(-4, -1, (M, P))
    c["planes"] = planes if per else planes[0]
    c["summary"] = np.abs(rng.normal(size=(N, 6))) * (rng.random((N, 1)) < 0.5)
    return c


def _clear_of_zero(c):
    """instances in which every signed distance of every point to every plane is at least 1e-3 m from 0: "active" cannot depend on rounding"""
    N = c["xc"].shape[0]
    ok = np.ones(N, bool)
    for r in c["points"]:
        p = CR.point(c["xc"], c["Rc"], np.broadcast_to(r, (N, 3)))
        pl = np.broadcast_to(c["planes"], (N,) + c["planes"].shape[-2:])
        d = np.einsum("npe,ne->np", pl[..., :3], p) - pl[..., 3]
        ok &= (np.abs(d) >= 1e-3).all(axis=1)
    return ok


PER_INSTANCE_KEYS = ("xc", "Rc", "Rcs", "tcs", "tv", "tw", "tc", "summary")


def _cases(seed, N, specs):
    """specs: [(n_points, P, per)] per patch.  Common: commanded torques with NaN instances, joint axes"""
    rng = np.random.default_rng(seed)
    c = dict(dt=5e-4, patches=[_patch(rng, N, *s) for s in specs])
    c["tau_cmd"] = rng.uniform(-5, 5, (N, J))
    c["tau_cmd"][rng.random(N) < 0.15] = np.nan               # a flagged instance under the NaN policy
    c["tau_cmd"][rng.random((N, J)) < 0.02] = np.nan
    c["rev"] = rng.random((N, J)) < 0.7
    aw = rng.normal(size=(N, J, 3))
    c["aw"] = aw / np.linalg.norm(aw, axis=-1, keepdims=True)
    c["oj"] = rng.uniform(-0.8, 0.8, (N, J, 3))
    keep = np.ones(N, bool)
    for pc in c["patches"]:
        keep &= _clear_of_zero(pc)
    for key in ("tau_cmd", "rev", "aw", "oj"):
        c[key] = c[key][keep]
    for pc in c["patches"]:
        for key in PER_INSTANCE_KEYS:
            pc[key] = pc[key][keep]
        if pc["per"]:
            pc["planes"] = pc["planes"][keep]
    c["N"] = int(keep.sum())
    return c


def _run(exe, c, tmp):
    N = c["N"]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, len(c["patches"]), J, 0], np.int32).tobytes())
        f.write(np.array([c["dt"]]).tobytes())
        for a in (c["tau_cmd"], c["rev"].astype(float), c["aw"], c["oj"]):
            f.write(np.ascontiguousarray(a, float).tobytes())
        for k, pc in enumerate(c["patches"]):
            f.write(np.array([pc["n"], pc["P"], int(pc["per"]), 0], np.int32).tobytes())
            planes = np.ascontiguousarray(pc["planes"].transpose(1, 2, 0)) if pc["per"] else pc["planes"]
            for a in (ANC[k].astype(float), pc["points"], planes, pc["xc"], pc["Rc"], pc["tv"], pc["tw"], pc["tc"], pc["Rcs"], pc["tcs"],
                      np.ascontiguousarray(pc["summary"].T)):
                f.write(np.ascontiguousarray(a, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    got, at = [], 0

    def take(shp):
        nonlocal at
        k = int(np.prod(shp))
        a = raw[at:at + k].reshape(shp)
        at += k
        return a
    for pc in c["patches"]:
        g = dict(readout=take((20, N)).T, FS=take((N, 3)), MS=take((N, 3)), summary=take((6, N)).T)
        if pc["n"] == 1:
            g["direct"] = dict(f=take((N, 3)), dmin=take((N,)), active=take((N,)), ext=take((N, J)), FS=take((N, 3)), MS=take((N, 3)))
        got.append(g)
    tau = take((N, J))
    assert at == raw.size
    return got, tau


def _reference(c):
    ref, ext = [], []
    for k, pc in enumerate(c["patches"]):
        s = PR.slots(pc["planes"], pc["xc"], pc["Rc"], pc["points"], pc["tv"], pc["tw"], pc["tc"])
        nt = PR.net(s)
        FS, MS = PR.sensor(nt["F"], nt["M"], pc["Rc"], pc["Rcs"], pc["tcs"])
        ref.append(dict(readout=PR.readout(s, nt, pc["xc"]), FS=FS, MS=MS, summary=PR.summary_advance(pc["summary"], c["dt"], nt, pc["n"]), net=nt, slots=s))
        ext.append((PR.joint_torques(s, c["rev"], c["aw"], c["oj"]), ANC[k], nt["n_touch"]))
    return ref, PR.tau_sim(c["tau_cmd"], ext)


def _compare(got, tau, ref, tau_ref):
    for g, r in zip(got, ref):
        for name in ("readout", "FS", "MS", "summary"):
            assert np.array_equal(g[name], r[name]), (name, np.abs(g[name] - r[name]).max())
    assert np.array_equal(tau, tau_ref), np.abs(tau - tau_ref).max()


@pytest.mark.parametrize("n,P,per", [(1, 1, False), (1, 4, True), (3, 1, True), (3, 4, False), (8, 1, False), (8, 4, True)])
def test_host_build_matches_the_restatement_bit_for_bit(exe, tmp_path, n, P, per):
    """contraction is off in every function of the header and the restatement performs the same operations in the same order, folds
    included, so every output is compared for equality: no tolerance anywhere"""
    c = _cases(200 + 10 * n + P, 2500, [(n, P, per)])
    (got,), tau = _run(exe, c, tmp_path)
    (ref,), tau_ref = _reference(c)
    nt = ref["net"]
    counts = np.bincount(nt["n_touch"], minlength=n + 1)
    assert c["N"] > 100 and counts[0] > 0 and counts[n] > 0 and (n < 3 or counts[1:n].sum() > 0), counts      # free, full and partial contact
    assert np.isnan(c["tau_cmd"]).any()
    _compare([got], tau, [ref], tau_ref)
    # no point touches: the torques pass through, bit for bit (a NaN as 0); unused slots hold exact zeros
    base = np.where(np.isnan(c["tau_cmd"]), 0.0, c["tau_cmd"])
    free = nt["n_touch"] == 0
    assert np.array_equal(tau[free].view(np.uint64), base[free].view(np.uint64))
    assert np.array_equal(tau[:, ~ANC[0]].view(np.uint64), base[:, ~ANC[0]].view(np.uint64))                   # not an ancestor: untouched
    assert (tau[~free][:, ANC[0]] != base[~free][:, ANC[0]]).any()
    assert not got["readout"][:, 12 + n:].any() and not got["readout"][free, :6].any()
    assert (got["readout"][:, 8] < n).all() and np.array_equal(got["readout"][:, 6], ref["slots"]["dcand"][:, :n].min(axis=1))
    assert np.array_equal(got["readout"][:, 8], np.argmin(ref["slots"]["dcand"], axis=1))                      # the lowest index that attains it
    if n == 1:
        # one point: what the single-point functions give, compared with == (so +0 and -0 are equal)
        d = got["direct"]
        assert np.array_equal(got["readout"][:, :3], d["f"]) and np.array_equal(got["readout"][:, 6], d["dmin"])
        assert np.array_equal(got["readout"][:, 7], (d["active"] > 0).astype(float))
        assert np.array_equal(got["FS"], d["FS"]) and np.array_equal(got["MS"], d["MS"])
        want = np.where(ANC[0][None, :] & (d["active"] > 0)[:, None], base + d["ext"], base)
        assert np.array_equal(tau, want)
        assert np.array_equal(got["readout"][:, 12], CR.plane_forces(c["patches"][0]["planes"], ref["slots"]["p"][:, 0],
                              CR.velocity(c["patches"][0]["tv"], c["patches"][0]["tw"], c["patches"][0]["tc"], ref["slots"]["p"][:, 0]))[1])


def test_equal_depths_pick_the_lower_index():
    """ties in the smallest-distance fold, in every pair of slots: the lower index wins whichever side of the fold it sits on"""
    for a in range(8):
        for b in range(a + 1, 8):
            d = np.full((1, 8), 0.5)
            d[0, a] = d[0, b] = -0.25
            dm, ix = PR.fold_min(d)
            assert dm[0] == -0.25 and ix[0] == a
    d = np.full((1, 8), np.inf)
    d[0, 0] = 3.0
    assert PR.fold_min(d) == (3.0, 0)                                   # unused slots are no candidates
    v = np.array([[1.0, 2.0 ** -53, 2.0 ** -53, 0.0, 0.0, 0.0, 2.0 ** -53, 0.0]])
    seq = 0.0
    for x in v[0]:
        seq = seq + x
    # ((1 + 0) + (2^-53 + 2^-53)) + ((2^-53 + 0) + 0) = (1 + 2^-52) + 2^-53 -> 1 + 2^-51 (ties to even); left to right every 2^-53 is lost
    assert PR.fold_sum(v)[0] == 1.0 + 2.0 ** -51 and seq == 1.0


def test_two_patches_on_a_branching_ancestor_set(exe, tmp_path):
    c = _cases(31, 4000, [(4, 2, True), (8, 1, False)])
    got, tau = _run(exe, c, tmp_path)
    ref, tau_ref = _reference(c)
    t0, t1 = ref[0]["net"]["n_touch"] > 0, ref[1]["net"]["n_touch"] > 0
    assert c["N"] > 100 and (t0 & t1).any() and (t0 & ~t1).any() and (~t0 & t1).any() and (~t0 & ~t1).any()
    _compare(got, tau, ref, tau_ref)
    base = np.where(np.isnan(c["tau_cmd"]), 0.0, c["tau_cmd"])
    same = lambda x, y: np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert same(tau[:, 8], base[:, 8])                                   # on neither branch
    assert same(tau[~t0][:, 2:5], base[~t0][:, 2:5]) and same(tau[~t1][:, 5:8], base[~t1][:, 5:8])
    assert same(tau[~t0 & ~t1], base[~t0 & ~t1])
    both = t0 & t1                                                       # the trunk carries both, the first patch added first
    e0 = PR.joint_torques(ref[0]["slots"], c["rev"], c["aw"], c["oj"])
    e1 = PR.joint_torques(ref[1]["slots"], c["rev"], c["aw"], c["oj"])
    assert np.array_equal(tau[both][:, :2], ((base + e0) + e1)[both][:, :2])
    assert np.array_equal(tau[t0][:, 2:5], (base + e0)[t0][:, 2:5]) and np.array_equal(tau[t1][:, 5:8], (base + e1)[t1][:, 5:8])


def test_host_build_under_sanitizers(exe_san, tmp_path):
    for specs in ([(1, 4, True)], [(3, 1, False)], [(8, 4, True), (3, 2, False)]):
        c = _cases(7 + specs[0][0], 1200, specs)
        got, tau = _run(exe_san, c, tmp_path)
        ref, tau_ref = _reference(c)
        assert c["N"] > 30
        _compare(got, tau, ref, tau_ref)


def test_a_tilted_plate_reports_a_moment_a_single_point_cannot():
    """the point of the feature, on the restatement: a square plate on a table tilted about x touches with one edge; the net moment about
    the control point is r x F of that edge, and the sensed moment about the tilt axis has its sign.  One point at the centre reports 0"""
    N = 1
    ang = np.deg2rad(3.0)
    nrm = np.array([0.0, -np.sin(ang), np.cos(ang)])                     # the table's normal, tilted about x: higher towards +y
    xc, eye = np.zeros((N, 3)), np.eye(3).reshape(1, 9)
    hi = nrm @ np.array([0.05, 0.05, 0.0])                               # n.p of the +y edge is the smallest: that edge is deepest
    assert hi < 0
    planes = np.array([[*nrm, hi + 1e-3, 2e4, 0.0, 0.0, 1e-3]])          # the +y edge 1e-3 m inside, the centre and the -y edge outside
    z = np.zeros((N, 3))
    s = PR.slots(planes, xc, eye, SQUARE, z, z, z)
    nt = PR.net(s)
    assert nt["n_touch"][0] == 2 and set(np.nonzero(s["active"][0])[0]) == {0, 1} and nt["i_deep"][0] == 0
    want = np.cross(SQUARE[0], s["f"][0, 0]) + np.cross(SQUARE[1], s["f"][0, 1])
    assert np.allclose(nt["M"][0], want, rtol=1e-14, atol=0) and nt["M"][0, 0] > 0   # +y edge pushed along +z: moment about +x
    FS, MS = PR.sensor(nt["F"], nt["M"], eye, eye, z)
    assert MS[0, 0] < 0 and np.array_equal(FS, -nt["F"])                 # the sensor reports the wrench on the environment
    one = PR.net(PR.slots(planes, xc, eye, np.zeros((1, 3)), z, z, z))
    assert one["n_touch"][0] == 0 and not one["M"].any()
    deep = planes.copy()
    deep[0, 3] += 0.01                                                   # pressed in until the centre touches too: still no moment from one point
    one = PR.net(PR.slots(deep, xc, eye, np.zeros((1, 3)), z, z, z))
    assert one["n_touch"][0] == 1 and not one["M"].any() and PR.net(PR.slots(deep, xc, eye, SQUARE, z, z, z))["M"][0, 0] > 0
