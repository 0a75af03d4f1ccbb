"""Contact planes and the simulated force sensor, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the
argument and call-order errors come back with the documented codes before the device is needed; the Python facade raises the same; the
host build of csrc/saip_contact.h (tests/cpp/contact_host.cpp, also under ASan/UBSan) matches the NumPy restatement tests/contact_ref.py
bit for bit; the restatement has the properties of a penalty contact with regularised Coulomb friction and of the sensor."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contact_ref as CR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_contact_attach", "saip_batch_contact_detach", "saip_batch_contact_info", "saip_batch_contact_set_planes_host",
                  "saip_batch_contact_sense", "saip_batch_contact_readout_host", "saip_batch_contact_summary_host",
                  "saip_batch_contact_summary_reset"]
POINTER_ENTRIES = ["saip_batch_contact_planes_device", "saip_batch_contact_readout_device", "saip_batch_contact_summary_device",
                   "saip_batch_contact_torques_device"]
EPS = 2.0 ** -52


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
    for name, val in [("MAX_PLANES", 4), ("PLANE_WORDS", 8), ("READOUT_ROWS", 8), ("SUMMARY_ROWS", 4)]:
        assert re.search(rf"#define SAIP_CONTACT_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_CONTACT_" + name) == val == getattr(CR, name)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert "csrc/saip_contact.hip" in capi.SOURCES and "csrc/saip_contact.h" in capi.HEADERS


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
    assert L.saip_batch_contact_detach(b) == code
    assert L.saip_batch_contact_info(b, C.byref(v), None, None, None, None) == code
    assert L.saip_batch_contact_set_planes_host(b, _dp(out)) == code
    assert L.saip_batch_contact_sense(b) == code
    assert L.saip_batch_contact_readout_host(b, _dp(out)) == code
    assert L.saip_batch_contact_summary_host(b, _dp(out)) == code
    assert L.saip_batch_contact_summary_reset(b) == code
    for name in POINTER_ENTRIES:
        assert getattr(L, name)(b) is None
    assert v.value == 7 and (out == 7.0).all()      # nothing was written


GOOD = np.array([[0.0, 0.0, 2.0, 0.1, 1e4, 50.0, 0.5, 1e-3], [1.0, 1.0, 0.0, -0.3, 2e3, 0.0, 0.0, 1e-2]])


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_contact_attach
    rc = np.array([0.0, 0.01, 0.05])
    assert att(None, 0, _dp(rc), 2, _dp(GOOD), 0, 1) == INVALID
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert att(b, 0, _dp(rc), 2, _dp(GOOD), 0, 1) == ORDER           # before finalize, whatever the arguments
        assert att(b, 9, None, 0, None, 0, 0) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for task in (-1, 2, 7):
            assert att(b, task, _dp(rc), 2, _dp(GOOD), 0, 1) == INVALID and b"out of range" in L.saip_last_error()
        assert att(b, 1, _dp(rc), 2, _dp(GOOD), 0, 1) == INVALID and b"not a motion-force task" in L.saip_last_error()
        for P in (0, -1, 5, 2**31 - 1):
            assert att(b, 0, _dp(rc), P, _dp(GOOD), 0, 1) == INVALID and b"planes required" in L.saip_last_error()
        assert att(b, 0, _dp(rc), 2, None, 0, 1) == INVALID and b"null planes" in L.saip_last_error()
        for bad in (np.nan, np.inf):
            r2 = rc.copy()
            r2[1] = bad
            assert att(b, 0, _dp(r2), 2, _dp(GOOD), 0, 1) == INVALID and b"not finite" in L.saip_last_error()
        # one bad word of one plane, batch-uniform and per instance (there: of one instance only)
        cases = [(0, np.nan, b"not finite"), (3, np.inf, b"not finite"), (7, -np.inf, b"not finite"), (4, 0.0, b"k > 0"), (4, -1.0, b"k > 0"),
                 (5, -1e-9, b"c >= 0"), (6, -0.1, b"mu >= 0"), (7, 0.0, b"v_s > 0"), (7, -1.0, b"v_s > 0")]
        per = np.ascontiguousarray(np.repeat(GOOD[:, :, None], B, axis=2))
        for word, val, msg in cases:
            p1 = GOOD.copy()
            p1[1, word] = val
            assert att(b, 0, _dp(rc), 2, _dp(p1), 0, 1) == INVALID and msg in L.saip_last_error(), (word, val)
            p2 = per.copy()
            p2[1, word, B - 1] = val
            assert att(b, 0, None, 2, _dp(p2), 1, 0) == INVALID and msg in L.saip_last_error(), (word, val)
        z = GOOD.copy()
        z[0, :3] = 0.0
        assert att(b, 0, _dp(rc), 2, _dp(z), 0, 1) == INVALID and b"normal is zero" in L.saip_last_error()
        zp = per.copy()
        zp[1, :3, 2] = 0.0
        assert att(b, 0, _dp(rc), 2, _dp(zp), 1, 1) == INVALID and b"normal is zero" in L.saip_last_error()
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        for P in (1, 2):
            for sensor in (0, 1):
                assert att(b, 0, _dp(rc), P, _dp(GOOD), 0, sensor) == NO_DEVICE and b"no CPU path" in L.saip_last_error()
                assert att(b, 0, None, P, _dp(per), 1, sensor) == NO_DEVICE
        four = np.ascontiguousarray(np.tile(GOOD, (2, 1)))
        assert att(b, 0, None, 4, _dp(four), 0, 1) == NO_DEVICE
        c0 = GOOD.copy()
        c0[:, 5:7] = 0.0                                                  # c = 0 and mu = 0 are allowed
        assert att(b, 0, None, 2, _dp(c0), 0, 1) == NO_DEVICE
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_largest_batch_overflows_nothing(sp):
    """the attachment's arrays are at most max(dof, 32) x ld doubles: with ld < 2^31 no byte count can pass 2^64, and the largest
    (configuration-only, so nothing is allocated) batch reaches the device check"""
    from sai_primitives_amd import capi
    L = sp.lib()
    Bb = 2**31 - 64
    robot, b = _controller_batch(sp, L, Bb)
    try:
        assert L.saip_batch_finalize(b) == 0 and L.saip_batch_ld(b) == Bb
        assert L.saip_batch_contact_attach(b, 0, None, 2, _dp(GOOD), 0, 1) == capi.SAIP_ERR_NO_DEVICE
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_contacts(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_contact_attach(b, 0, None, 2, _dp(GOOD), 0, 1) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    assert not hasattr(jt, "attachContactPlanes")          # a motion-force task carries the point
    for bad in (np.zeros(8), np.zeros((2, 7)), np.zeros((2, B, 8))):
        with pytest.raises(ValueError, match="planes of shape"):
            mf.attachContactPlanes(bad)
    for bad in (np.zeros((2, 8)), np.zeros((2, 8, B)), np.zeros((2, B + 1, 8))):
        with pytest.raises(ValueError, match="per-instance planes of shape"):
            mf.attachContactPlanes(bad, per_instance=True)
    with pytest.raises(ValueError, match="point of shape"):
        mf.attachContactPlanes(GOOD, point=(0, 0))
    with pytest.raises(ValueError, match="planes required"):
        mf.attachContactPlanes(np.tile(GOOD, (3, 1)))
    with pytest.raises(ValueError, match="k > 0"):
        mf.attachContactPlanes(np.array([[0, 0, 1, 0, 0, 0, 0, 1e-3]], float))
    with pytest.raises(ValueError, match="normal is zero"):
        mf.attachContactPlanes(np.array([[0, 0, 0, 0, 1e3, 0, 0, 1e-3]], float))
    with pytest.raises(ValueError, match="not finite"):
        mf.attachContactPlanes(GOOD, point=(0, np.nan, 0))
    for per in (False, True):
        planes = np.ascontiguousarray(np.repeat(GOOD[:, None, :], B, axis=1)) if per else GOOD
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            mf.attachContactPlanes(planes, point=(0, 0, 0.05), sensor=True, per_instance=per)
    for fn in (mf.detachContactPlanes, mf.contactReadout, mf.contactSummary, mf.resetContactSummary, mf.contactInfo, ctrl.contactSense,
               lambda: mf.setContactPlanes(GOOD)):
        with pytest.raises(sp.SaipError, match="no contact planes are attached"):
            fn()
    assert mf.contactPlanesDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "contact_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("contact_host"), "contact_host", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("contact_host_san"), "contact_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _rotations(rng, N):
    Q = np.linalg.qr(rng.normal(size=(N, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q.reshape(N, 9)


def _cases(seed, N, P, J, per):
    """random cases: the point within a few centimetres of the planes (so that every number of active planes occurs), speeds on both
    sides of v_s, revolute and prismatic joints"""
    rng = np.random.default_rng(seed)
    c = dict(N=N, P=P, J=J, per=per, dt=5e-4)
    c["xc"] = rng.uniform(-0.5, 0.5, (N, 3))
    c["Rc"], c["Rcs"] = _rotations(rng, N), _rotations(rng, N)
    c["rc"] = rng.uniform(-0.1, 0.1, (N, 3)) * (rng.random((N, 1)) < 0.8)
    c["tcs"] = rng.uniform(-0.1, 0.1, (N, 3))
    scale = 10.0 ** rng.uniform(-5, 0, (N, 1))
    c["tv"], c["tw"], c["tc"] = (rng.normal(size=(N, 3)) * scale for _ in range(3))
    p = CR.point(c["xc"], c["Rc"], c["rc"])
    n = rng.normal(size=(N if per else 1, P, 3))
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    planes = np.zeros((N if per else 1, P, 8))
    planes[..., :3] = n
    ref_p = p if per else p[:1]
    planes[..., 3] = np.einsum("npe,ne->np", n, ref_p) + rng.uniform(-0.02, 0.03, planes.shape[:2]) * (1.0 if per else 20.0)
    planes[..., 4] = 10.0 ** rng.uniform(2, 5, planes.shape[:2])
    planes[..., 5] = rng.uniform(0, 200, planes.shape[:2]) * (rng.random(planes.shape[:2]) < 0.7)
    planes[..., 6] = rng.uniform(0, 1.2, planes.shape[:2]) * (rng.random(planes.shape[:2]) < 0.8)
    planes[..., 7] = 10.0 ** rng.uniform(-4, -1, planes.shape[:2])
    c["planes"] = planes if per else planes[0]
    c["rev"] = rng.random((N, J)) < 0.7
    aw = rng.normal(size=(N, J, 3))
    c["aw"] = aw / np.linalg.norm(aw, axis=-1, keepdims=True)
    c["oj"] = rng.uniform(-0.8, 0.8, (N, J, 3))
    c["summary"] = np.abs(rng.normal(size=(N, 4))) * (rng.random((N, 1)) < 0.5)
    return c


def _run(exe, c, tmp):
    N, P, J = c["N"], c["P"], c["J"]
    planes = np.ascontiguousarray(c["planes"].transpose(1, 2, 0)) if c["per"] else c["planes"]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, P, J, int(c["per"])], np.int32).tobytes())
        f.write(np.array([c["dt"]]).tobytes())
        for a in (planes, c["xc"], c["Rc"], c["rc"], c["tv"], c["tw"], c["tc"], c["Rcs"], c["tcs"], c["rev"].astype(float), c["aw"], c["oj"],
                  np.ascontiguousarray(c["summary"].T)):
            f.write(np.ascontiguousarray(a, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    shapes = [("p", (N, 3)), ("v", (N, 3)), ("f", (N, 3)), ("fn_sum", (N,)), ("dmin", (N,)), ("active", (N,)), ("tau", (N, J)), ("FS", (N, 3)),
              ("MS", (N, 3)), ("summary", (4, N))]
    got, at = {}, 0
    for name, shp in shapes:
        k = int(np.prod(shp))
        got[name] = raw[at:at + k].reshape(shp)
        at += k
    assert at == raw.size
    got["summary"] = got["summary"].T
    return got


def _reference(c):
    p = CR.point(c["xc"], c["Rc"], c["rc"])
    v = CR.velocity(c["tv"], c["tw"], c["tc"], p)
    f, fn_sum, dmin, active = CR.plane_forces(c["planes"], p, v)
    FS, MS = CR.sensor(f, p, c["xc"], c["Rc"], c["Rcs"], c["tcs"])
    return dict(p=p, v=v, f=f, fn_sum=fn_sum, dmin=dmin, active=active.astype(float), tau=CR.joint_torque(c["rev"], c["aw"], c["oj"], p, f), FS=FS, MS=MS,
                summary=CR.summary_advance(c["summary"], c["dt"], f, fn_sum, dmin, active))


@pytest.mark.parametrize("P,per", [(1, False), (2, True), (3, False), (4, True)])
def test_host_build_matches_the_restatement_bit_for_bit(exe, tmp_path, P, per):
    """every function of the header has contraction off and the restatement performs the same operations in the same order, so every
    output is compared for equality: no tolerance anywhere"""
    c = _cases(100 + P, 600, P, 9, per)
    got, ref = _run(exe, c, tmp_path), _reference(c)
    counts = np.bincount(ref["active"].astype(int), minlength=P + 1)
    assert counts[0] > 0 and counts[1:].sum() > 100 and (P < 2 or counts[2:].sum() > 0), counts      # free, touching, several planes at once
    for name in ref:
        assert np.array_equal(got[name], ref[name]), (name, np.abs(got[name] - ref[name]).max())


def test_host_build_under_sanitizers(exe_san, tmp_path):
    for P, per in [(1, True), (4, False), (4, True)]:
        c = _cases(7 + P, 130, P, 32, per)
        got, ref = _run(exe_san, c, tmp_path), _reference(c)
        for name in ref:
            assert np.array_equal(got[name], ref[name]), name


# ------------------------------------------------------------------ properties of the restatement
def _state(rng, N):
    return rng.uniform(-0.3, 0.3, (N, 3)), rng.normal(size=(N, 3)) * 10.0 ** rng.uniform(-5, 0, (N, 1))


def test_sensor_is_the_inverse_of_the_laws_sensed_wrench():
    rng = np.random.default_rng(3)
    N = 2000
    f = rng.normal(size=(N, 3)) * 10.0 ** rng.uniform(-2, 3, (N, 1))
    xc, rc, tcs = rng.uniform(-1, 1, (N, 3)), rng.uniform(-0.2, 0.2, (N, 3)), rng.uniform(-0.2, 0.2, (N, 3))
    Rc, Rcs = _rotations(rng, N), _rotations(rng, N)
    p = CR.point(xc, Rc, rc)
    FS, MS = CR.sensor(f, p, xc, Rc, Rcs, tcs)
    fw, mw = CR.sensed_wrench(FS, MS, Rc, Rcs, tcs)
    F = -f
    m = np.cross(p - xc, F)
    nf, nm, nt = (np.linalg.norm(a, axis=1) for a in (F, m, tcs))
    # force: four products with rotations that are orthonormal to ~4 eps each (QR), three rounded terms per row: (4 * 3 + 4 * 4) eps |F|
    # < 32 eps |F|.  moment: the same on |m|, plus t_cs x fc subtracted and added back, each a rounded cross product (2 eps |t||F| each)
    # carried through two rotations: < 32 eps (|m| + |t_cs| |F|)
    assert (np.abs(fw - F).max(axis=1) <= 32 * EPS * nf).all()
    assert (np.abs(mw - m).max(axis=1) <= 32 * EPS * (nm + nt * nf)).all()
    # no lever arm, sensor frame = control frame = world: the sensor reports -f exactly and no moment
    eye = np.broadcast_to(np.eye(3).reshape(9), (N, 9))
    FS0, MS0 = CR.sensor(f, xc, xc, eye, eye, np.zeros((N, 3)))
    assert np.array_equal(FS0, -f) and not MS0.any()


def test_plane_force_properties():
    rng = np.random.default_rng(4)
    N = 4000
    p, v = _state(rng, N)
    n = rng.normal(size=(N, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    planes = np.zeros((N, 1, 8))
    planes[:, 0, :3] = n
    planes[:, 0, 3] = CR.dot(n, p) + rng.uniform(-0.01, 0.01, N)
    planes[:, 0, 4:] = np.stack([10.0 ** rng.uniform(2, 5, N), rng.uniform(0, 100, N), rng.uniform(0, 1.5, N), 10.0 ** rng.uniform(-4, -1, N)], axis=1)
    f, fn_sum, dmin, active = CR.plane_forces(planes, p, v)
    d = CR.dot(n, p) - planes[:, 0, 3]
    assert np.array_equal(dmin, d) and np.array_equal(active, (d < 0).astype(int))
    free = d >= 0
    assert free.any() and not f[free].any() and not fn_sum[free].any()                # d >= 0  =>  f = 0
    assert (fn_sum >= 0).all() and (fn_sum[~free] > 0).any()                             # f_n >= 0
    vn = CR.dot(n, v)
    vt = v - vn[:, None] * n
    ft = f - fn_sum[:, None] * n
    mu = planes[:, 0, 6]
    # |f_t| = mu f_n |v_t| / max(|v_t|, v_s) <= mu f_n up to the rounding of a handful of operations on numbers of size |f|
    slack = 16 * EPS * (np.linalg.norm(f, axis=1) + fn_sum)
    assert (np.linalg.norm(ft, axis=1) <= mu * fn_sum + slack).all()                     # |f_t| <= mu f_n
    assert (np.einsum("ne,ne->n", ft, vt) <= slack * np.linalg.norm(vt, axis=1)).all()   # f_t . v_t <= 0
    pushing = ~free & (fn_sum > 0) & (mu > 0)
    assert (np.einsum("ne,ne->n", ft, vt)[pushing] < 0).any()
    # a plane whose d < 0 but that is left fast enough pulls nothing: f_n is clamped at 0
    fast = planes.copy()
    fast[:, 0, 5] = 1e9
    f2, fn2, _, act2 = CR.plane_forces(fast, p, np.abs(vn)[:, None] * n + 1.0 * n)
    assert not f2.any() and not fn2.any() and np.array_equal(act2, active)


def test_friction_is_linear_in_the_slip_below_vs():
    rng = np.random.default_rng(5)
    N = 500
    n = np.array([0.0, 0.0, 1.0])
    planes = np.array([[0, 0, 1, 0.0, 1e4, 0.0, 0.7, 1e-2]])
    p = np.column_stack([rng.uniform(-1, 1, (N, 2)), -rng.uniform(1e-4, 1e-2, N)])
    t = rng.normal(size=(N, 2))
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    s = rng.uniform(1e-5, 4e-3, N)                            # 2 s stays below v_s = 1e-2
    v1 = np.column_stack([t * s[:, None], np.zeros(N)])
    f1 = CR.plane_forces(planes, p, v1)[0]
    f2 = CR.plane_forces(planes, p, 2.0 * v1)[0]
    fn = 1e4 * -p[:, 2]
    assert np.array_equal(f1[:, 2], fn) and np.array_equal(f2[:, 2], fn)        # c = 0: the normal force does not see the slip
    assert np.array_equal(f2[:, :2], 2.0 * f1[:, :2])                            # doubling is exact in binary: linear bit for bit
    assert np.allclose(f1[:, :2], -0.7 * fn[:, None] * v1[:, :2] / 1e-2, rtol=8 * EPS, atol=0)
    # above v_s the magnitude saturates at mu f_n
    f3 = CR.plane_forces(planes, p, v1 / s[:, None] * 0.5)[0]
    assert np.allclose(np.linalg.norm(f3[:, :2], axis=1), 0.7 * fn, rtol=8 * EPS, atol=0)
    assert n @ np.array([0, 0, 1.0]) == 1.0


def test_two_active_planes_superpose():
    rng = np.random.default_rng(6)
    N = 300
    p, v = _state(rng, N)
    a = CR.plane([0.3, -1.0, 2.0], 0.0, 3e3, 20.0, 0.4, 1e-3)
    b = CR.plane([1.0, 0.5, -0.2], 0.0, 8e3, 5.0, 0.9, 1e-2)
    a[3], b[3] = 1.0, 1.1                                      # both far in front of every p: always active
    fa, na, da, _ = CR.plane_forces(a[None], p, v)
    fb, nb, db, _ = CR.plane_forces(b[None], p, v)
    fab, nab, dab, act = CR.plane_forces(np.stack([a, b]), p, v)
    assert (act == 2).all()
    assert np.array_equal(fab, fa + fb) and np.array_equal(nab, na + nb) and np.array_equal(dab, np.minimum(da, db))
    # ... and an inactive plane next to an active one changes nothing but the smallest distance
    far = CR.plane([0, 0, 1.0], -5.0, 1e4)
    f1, n1, d1, act1 = CR.plane_forces(np.stack([far, a]), p, v)
    assert np.array_equal(f1, fa) and np.array_equal(n1, na) and (act1 == 1).all() and np.array_equal(d1, np.minimum(da, p[:, 2] + 5.0))
