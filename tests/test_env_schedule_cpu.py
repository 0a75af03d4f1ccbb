"""Environment schedules, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument and call-order errors
come back with the documented codes before the device is needed; the host build of csrc/saip_env_schedule.h and of the moving-surface
contact arithmetic (tests/cpp/env_schedule_host.cpp, also under ASan/UBSan) matches the NumPy restatement tests/env_schedule_ref.py bit for
bit in every table word, velocity word and force; interpolated normals stay unit to a derived bound.

A configuration-only batch (device -1) cannot carry a contact or clearance attachment, so the refusals that need the target's table --
keyframe contents against it -- are checked on the routine the attach entry calls for them (env_check_keyframes, through the host program)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import contact_patch_ref as CP
import contact_ref as CR
import env_schedule_ref as ES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_env_schedule_attach", "saip_batch_env_schedule_detach", "saip_batch_env_schedule_rewind", "saip_batch_env_schedule_info"]
POINTER_ENTRIES = ["saip_batch_env_schedule_keyframes_device", "saip_batch_env_schedule_velocity_device"]
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
    dev = open(os.path.join(PKG, "csrc", "saip_env_schedule.h")).read()
    for name, val, ref in [("MAX_SCHEDULES", 4, ES.MAX_SCHEDULES), ("PLANE_WORDS", 12, ES.PLANE_WORDS), ("TARGET_OBSTACLES", 0, ES.TARGET_OBSTACLES),
                           ("TARGET_PLANES", 1, ES.TARGET_PLANES), ("TARGET_PATCH", 2, ES.TARGET_PATCH), ("HOLD", 0, ES.HOLD), ("LINEAR", 1, ES.LINEAR)]:
        assert re.search(rf"#define SAIP_ENV_{name} {val}\b", hdr), name
        assert re.search(rf"\bENV_{name} = {val}\b", dev), name
        assert getattr(capi, "SAIP_ENV_" + name) == val == ref
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    for f in ("csrc/saip_env_schedule.hip", "csrc/saip_engine_env.cpp"):
        assert f in capi.SOURCES
    assert "csrc/saip_env_schedule.h" in capi.HEADERS


def _controller_batch(sp, L, B=4):
    robot = sp.SaiModel("panda_arm", B, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, B, -1, C.byref(b)) == 0
    pos, tid = (C.c_double * 3)(0, 0, 0.07), C.c_int(-1)
    assert L.saip_batch_add_motion_force_task(b, b"mf", b"end-effector", pos, None, None, -1, None, -1, 0.001, C.byref(tid)) == 0
    assert L.saip_batch_add_joint_task(b, b"jt", None, 0, 0.001, C.byref(tid)) == 0
    return robot, b


def _others_refuse(L, b, code):
    v, per = C.c_int(7), C.c_longlong(7)
    for target in (0, 1, 2):
        assert L.saip_batch_env_schedule_detach(b, target, -1) == code
        assert L.saip_batch_env_schedule_info(b, target, 0, C.byref(v), None, None, None, None, None, C.byref(per)) == code
        for name in POINTER_ENTRIES:
            assert getattr(L, name)(b, target, -1) is None
    assert v.value == 7 and per.value == 7          # nothing was written


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    att = L.saip_batch_env_schedule_attach
    key = np.zeros((2, 1, 12))
    key[:, 0, :8] = CR.plane([0, 0, 1.0], 0.1, 1e4)
    assert att(None, 1, 0, 0, 1, _dp(key), 2, 1, 0) == INVALID
    assert L.saip_batch_env_schedule_rewind(None, 0) == INVALID
    _others_refuse(L, None, INVALID)
    robot, b = _controller_batch(sp, L)
    try:
        assert att(b, 1, 0, 0, 1, _dp(key), 2, 1, 0) == ORDER            # before finalize, whatever the arguments
        assert att(b, 9, 0, 0, 1, _dp(key), 0, 0, 5) == ORDER
        assert L.saip_batch_env_schedule_rewind(b, 0) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for target in (-1, 3, 2 ** 31 - 1):
            assert att(b, target, 0, 0, 1, _dp(key), 2, 1, 0) == INVALID and b"unknown target" in L.saip_last_error()
        for mode in (-1, 2):
            assert att(b, 1, 0, 0, 1, _dp(key), 2, 1, mode) == INVALID and b"unknown mode" in L.saip_last_error()
        for K, stride in ((0, 1), (-3, 1), (2, 0), (2, -1)):
            assert att(b, 1, 0, 0, 1, _dp(key), K, stride, 0) == INVALID and b"n_keyframes >= 1 and stride >= 1" in L.saip_last_error()
        assert att(b, 1, 0, 0, 1, None, 2, 1, 0) == INVALID and b"null keyframes" in L.saip_last_error()
        # valid arguments, but the target is not attached (it cannot be on a configuration-only batch): the order error names it
        for target, msg in ((0, b"no clearance monitor is attached"), (1, b"no contact planes are attached"), (2, b"carries no contact patch")):
            assert att(b, target, 0, 0, 1, _dp(key), 2, 1, 1) == ORDER and msg in L.saip_last_error()
        assert L.saip_batch_env_schedule_detach(b, 5, 0) == INVALID and b"unknown target" in L.saip_last_error()
        assert L.saip_batch_env_schedule_detach(b, -1, -1) == 0           # all of none
        assert L.saip_batch_env_schedule_rewind(b, -1) == INVALID and b"below 0" in L.saip_last_error()
        assert L.saip_batch_env_schedule_rewind(b, 0) == 0 and L.saip_batch_env_schedule_rewind(b, 2 ** 40) == 0
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    with pytest.raises(sp.SaipError, match="no clearance monitor is attached"):
        ctrl.setObstacleSchedule(np.zeros((2, 1, 8)))
    with pytest.raises(sp.SaipError, match="neither contact planes nor a contact patch"):
        mf.setContactSchedule(np.zeros((2, 1, 12)))
    with pytest.raises(sp.SaipError, match="neither contact planes nor a contact patch"):
        mf.contactScheduleInfo()
    with pytest.raises(sp.SaipError, match="have no environment schedule"):
        ctrl.obstacleScheduleInfo()
    with pytest.raises(ValueError, match="unknown mode"):
        ctrl._env_schedule_attach("x", 0, -1, np.zeros((2, 1, 8)), 8, False, 1, "cubic", 0)
    for bad, per in ((np.zeros((2, 8)), False), (np.zeros((2, 1, 7)), False), (np.zeros((2, 1, B, 8)), False), (np.zeros((2, 1, 8)), True),
                     (np.zeros((2, 1, 8, B)), True), (np.zeros((2, 1, B + 1, 8)), True)):
        with pytest.raises(ValueError, match="keyframes of shape"):
            ctrl._env_schedule_attach("x", 0, -1, bad, 8, per, 1, "hold", 0)
    ctrl.rewindEnvironment(3)
    ctrl.clearEnvironmentSchedules()
    with pytest.raises(ValueError, match="below 0"):
        ctrl.rewindEnvironment(-2)


# ------------------------------------------------------------------ the host build of the headers against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "env_schedule_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("env_host"), "env_host", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("env_host_san"), "env_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _unit(rng, shape):
    n = rng.normal(size=shape + (3,))
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def _keyframes(rng, planes, K, n, B):
    """(K, n, W[, B]) keyframes as the engine keeps them: plane normals normalised its way; obstacles alternate capsule / half-space by item;
    consecutive normals less than a right angle apart"""
    cols = B if B else 1
    W = 12 if planes else 8
    key = rng.uniform(-0.5, 0.5, (K, n, W, cols))
    base = _unit(rng, (n, cols))
    for k in range(K):
        m = base + 0.3 * rng.normal(size=(n, cols, 3))              # within a right angle of the previous one
        base = m / np.linalg.norm(m, axis=-1, keepdims=True)
        n0 = 0 if planes else 1
        key[k, :, n0:n0 + 3, :] = base.transpose(0, 2, 1)
    if planes:
        key[:, :, 4] = 10.0 ** rng.uniform(2, 5, (K, n, cols))
        key[:, :, 5] = rng.uniform(0, 100, (K, n, cols))
        key[:, :, 6] = rng.uniform(0, 1, (K, n, cols))
        key[:, :, 7] = 10.0 ** rng.uniform(-4, -1, (K, n, cols))
        key[:, :, 11] = 0.0
        key = ES.normalise_plane_keys(key)
    else:
        key[:, :, 0] = (np.arange(n) % 2)[None, :, None]
        key[:, :, 7] = np.abs(key[:, :, 7])
    return key if B else key[..., 0]


def _run_schedule(exe, tmp, key, planes, B, first, items, stride, mode, periods, T, sentinel):
    K, n = key.shape[:2]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([planes, K, n, B, first, items, stride, mode, periods], np.int32).tobytes())
        f.write(np.array([T, sentinel]).tobytes())
        f.write(np.ascontiguousarray(key, float).tobytes())
    out = subprocess.run([exe, "schedule", str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    tail = (B,) if B else ()
    per = items * 8 * max(B, 1) + (items * 4 * max(B, 1) if planes else 0)
    assert raw.size == periods * per
    got = []
    for c in range(periods):
        r = raw[c * per:(c + 1) * per]
        table = r[:items * 8 * max(B, 1)].reshape((items, 8) + tail)
        vel = r[items * 8 * max(B, 1):].reshape((items, 4) + tail) if planes else None
        got.append((table, vel))
    return got


def _check_schedule(exe, tmp, seed, planes, K, stride, mode, B, first=1, extra=2):
    """periods 0 .. (K - 1) stride + 2: s == 0, true fractions and the held tail; the scheduled items sit at [first, first + n) of a table
    with `extra` more items, whose words (and the velocity rows) keep the sentinel"""
    rng = np.random.default_rng(seed)
    n, T, sentinel = 3, 2 * 5e-4, -7.25
    items, periods = n + extra, (K - 1) * stride + 3
    key = _keyframes(rng, planes, K, n, B)
    got = _run_schedule(exe, tmp, key, planes, B, first, items, stride, mode, periods, T, sentinel)
    fractions = set()
    for c, (table, vel) in enumerate(got):
        x = ES.period_index(c, planes)
        assert x == (c if planes else c + 1)                         # the alignment: contact sees c, clearance c + 1
        rt, rv = ES.rows(key, planes, x, stride, mode, T)
        fractions.add(ES.timing(x, K, stride, mode)[1:])
        assert np.array_equal(table[first:first + n], rt), (c, np.abs(table[first:first + n] - rt).max())
        rest = np.delete(table, np.s_[first:first + n], axis=0)
        assert rest.size and (rest == sentinel).all()
        if planes:
            assert np.array_equal(vel[first:first + n], rv), c
            assert (np.delete(vel, np.s_[first:first + n], axis=0) == sentinel).all()
            if mode == ES.HOLD or x >= (K - 1) * stride:
                assert not vel[first:first + n, 3].any() and np.array_equal(vel[first:first + n, :3], rt_u(key, x, K, stride))
    return fractions


def rt_u(key, x, K, stride):
    """HOLD and the held tail: v_p = u + 0 n, the keyframe's u up to the sign of a zero"""
    i = min(x // stride, K - 1)
    return key[i][:, 8:11] + 0.0


@pytest.mark.parametrize("planes", [0, 1])
@pytest.mark.parametrize("B", [0, 5])
def test_host_build_matches_the_restatement_bit_for_bit(exe, tmp_path, planes, B):
    seen = set()
    for mode in (ES.HOLD, ES.LINEAR):
        for K in (1, 2, 4):
            for stride in (1, 3):
                seen |= {(mode,) + f for f in _check_schedule(exe, tmp_path, 10 * K + stride + mode, planes, K, stride, mode, B)}
    assert (ES.LINEAR, 0.0, True) in seen and any(m == ES.LINEAR and 0 < s < 1 and mv for m, s, mv in seen) and (ES.LINEAR, 0.0, False) in seen


def test_alignment_of_contact_and_clearance_targets(exe, tmp_path):
    """the same keyframe values under both targets (an obstacle's eight words as the first eight of a plane): in rollout period c the
    clearance table holds what the contact table holds in period c + 1"""
    rng = np.random.default_rng(5)
    K, stride = 3, 2
    ko = _keyframes(rng, 0, K, 2, 0)
    ko[:, :, 0] = 0.0                                                   # capsules: every word interpolates plainly
    got = _run_schedule(exe, tmp_path, ko, 0, 0, 0, 2, stride, ES.LINEAR, 6, 1e-3, 0.0)
    for c in range(6):
        assert np.array_equal(got[c][0], ES.rows(ko, 0, c + 1, stride, ES.LINEAR, 1e-3)[0])
        if c > 0:
            assert not np.array_equal(got[c][0], ES.rows(ko, 0, c, stride, ES.LINEAR, 1e-3)[0]) or c + 1 > (K - 1) * stride


def test_host_build_under_sanitizers(exe_san, tmp_path):
    for planes, B, K, stride, mode in [(1, 4, 3, 2, ES.LINEAR), (0, 0, 2, 3, ES.LINEAR), (1, 0, 1, 1, ES.HOLD), (0, 3, 4, 1, ES.HOLD)]:
        _check_schedule(exe_san, tmp_path, 77, planes, K, stride, mode, B)
    for P, per, n_points in [(4, True, 0), (1, False, 8), (3, True, 5)]:
        _check_forces(exe_san, tmp_path, 9, 60, P, per, n_points, zero=False)


def test_interpolated_normals_stay_unit():
    """| |n|^2 - 1 | <= 4 * 2^-52 for n = m / sqrt(fl(m . m)), m = a + s (b - a).  With u = 2^-53 (one rounding):
      * fl(m . m) = ((p0 + p1) + p2) with p_e = fl(m_e m_e): every term is positive and passes through at most three roundings (its product
        and the two sums; p2 through two), so fl(m . m) = |m|^2 (1 + t), |t| <= 3 u + O(u^2);
      * r = fl(sqrt(.)) = |m| (1 + t)^(1/2) (1 + d), |d| <= u;
      * n_e = fl(m_e / r) = (m_e / r) (1 + d_e), |d_e| <= u.
    Hence |n|^2 = [sum_e (m_e^2 / |m|^2) (1 + d_e)^2] / [(1 + t) (1 + d)^2], a weighted mean of factors within 1 +- 2 u over a denominator
    within 1 +- (3 u + 2 u): | |n|^2 - 1 | <= 7 u + O(u^2) < 8 u = 4 * 2^-52.  |m|^2 >= 1/2 (the attach refuses n_a . n_b < 0) keeps
    everything far from underflow.  Summing |n|^2 in double would add roundings of its own, so it is taken in exact rational arithmetic."""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    N = 300
    a = _unit(rng, (N,))
    m = a + 0.9 * rng.normal(size=(N, 3))
    b = m / np.linalg.norm(m, axis=1, keepdims=True)
    b = np.where((CR.dot(a, b) < 0)[:, None], -b, b)
    bound = Fraction(4) * Fraction(2) ** -52
    key = np.zeros((2, N, 12))
    key[0, :, 0:3], key[1, :, 0:3] = a, b
    key[:, :, 4], key[:, :, 7] = 1e3, 1e-3
    for stride in (2, 3, 7):
        for x in range(1, stride):
            n = ES.rows(key, 1, x, stride, ES.LINEAR, 1e-3)[0][:, 0:3]
            assert not np.array_equal(n, a)
            for row in n:
                e = abs(sum(Fraction(float(v)) ** 2 for v in row) - 1)
                assert e <= bound, (float(e), float(bound))


# ------------------------------------------------------------------ moving-surface forces
def _rotations(rng, N):
    Q = np.linalg.qr(rng.normal(size=(N, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q.reshape(N, 9)


def _force_cases(seed, N, P, per, n_points, zero):
    rng = np.random.default_rng(seed)
    c = dict(N=N, P=P, per=per, n_points=n_points)
    c["xc"] = rng.uniform(-0.5, 0.5, (N, 3))
    c["Rc"] = _rotations(rng, N)
    c["r"] = rng.uniform(-0.05, 0.05, (max(n_points, 1), 3))
    scale = 10.0 ** rng.uniform(-5, 0, (N, 1))
    c["tv"], c["tw"], c["tc"] = (rng.normal(size=(N, 3)) * scale for _ in range(3))
    M = N if per else 1
    n = _unit(rng, (M, P))
    planes = np.zeros((M, P, 8))
    planes[..., :3] = n
    # inactive planes too: per instance around the instance's point, batch-uniform through the middle of the cloud of points
    planes[..., 3] = np.einsum("npe,ne->np", n, c["xc"]) + rng.uniform(-0.03, 0.04, (M, P)) if per else rng.uniform(-0.1, 0.1, (M, P))
    planes[..., 4] = 10.0 ** rng.uniform(2, 5, (M, P))
    planes[..., 5] = rng.uniform(0, 200, (M, P)) * (rng.random((M, P)) < 0.7)
    planes[..., 6] = rng.uniform(0, 1.2, (M, P)) * (rng.random((M, P)) < 0.8)
    planes[..., 7] = 10.0 ** rng.uniform(-4, -1, (M, P))
    vel = np.zeros((M, P, 4)) if zero else rng.normal(size=(M, P, 4)) * 10.0 ** rng.uniform(-4, 0, (M, P, 1))
    c["planes"], c["vel"] = (planes, vel) if per else (planes[0], vel[0])
    return c


def _run_forces(exe, tmp, c):
    N, P, n_points = c["N"], c["P"], c["n_points"]
    tr = (lambda a: np.ascontiguousarray(a.transpose(1, 2, 0))) if c["per"] else (lambda a: a)
    with open(tmp / "fin.bin", "wb") as f:
        f.write(np.array([N, P, int(c["per"]), n_points], np.int32).tobytes())
        for a in (tr(c["planes"]), tr(c["vel"]), c["xc"], c["Rc"], c["r"], c["tv"], c["tw"], c["tc"]):
            f.write(np.ascontiguousarray(a, float).tobytes())
    out = subprocess.run([exe, "forces", str(tmp / "fin.bin"), str(tmp / "fout.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "fout.bin")
    if n_points == 0:
        shapes = [("f", (N, 3)), ("fn_sum", (N,)), ("dmin", (N,)), ("active", (N,))]
    else:
        shapes = [("p", (N, 8, 3)), ("f", (N, 8, 3)), ("m", (N, 8, 3)), ("fn_sum", (N, 8)), ("dcand", (N, 8)), ("active", (N, 8)), ("F", (N, 3)), ("M", (N, 3))]
    res, at = [], 0
    for _ in range(2):                                                   # moving, then static
        got = {}
        for name, shp in shapes:
            k = int(np.prod(shp))
            got[name] = raw[at:at + k].reshape(shp)
            at += k
        res.append(got)
    assert at == raw.size
    return res


def _check_forces(exe, tmp, seed, N, P, per, n_points, zero):
    c = _force_cases(seed, N, P, per, n_points, zero)
    moving, static = _run_forces(exe, tmp, c)
    if n_points == 0:
        p = CR.point(c["xc"], c["Rc"], np.broadcast_to(c["r"][0], (N, 3)))
        v = CR.velocity(c["tv"], c["tw"], c["tc"], p)
        f, fn_sum, dmin, active = ES.plane_forces_moving(c["planes"], c["vel"], p, v)
        ref = dict(f=f, fn_sum=fn_sum, dmin=dmin, active=active.astype(float))
        f0, fn0, d0, a0 = CR.plane_forces(c["planes"], p, v)
        ref0 = dict(f=f0, fn_sum=fn0, dmin=d0, active=a0.astype(float))
    else:
        s = ES.slots_moving(c["planes"], c["vel"], c["xc"], c["Rc"], c["r"], c["tv"], c["tw"], c["tc"])
        nt = CP.net(s)
        ref = dict(p=s["p"], f=s["f"], m=s["m"], fn_sum=s["fn_sum"], dcand=s["dcand"], active=s["active"].astype(float), F=nt["F"], M=nt["M"])
        s0 = CP.slots(c["planes"], c["xc"], c["Rc"], c["r"], c["tv"], c["tw"], c["tc"])
        nt0 = CP.net(s0)
        ref0 = dict(p=s0["p"], f=s0["f"], m=s0["m"], fn_sum=s0["fn_sum"], dcand=s0["dcand"], active=s0["active"].astype(float), F=nt0["F"], M=nt0["M"])
    for name in ref:
        assert np.array_equal(moving[name], ref[name]), (name, np.abs(moving[name] - ref[name]).max())
        assert np.array_equal(static[name], ref0[name]), name
        if zero:                                                         # v_p = 0: ct_plane_forces in every output bit
            assert np.array_equal(moving[name].view(np.uint64), static[name].view(np.uint64)), name
    act = ref["active"]
    assert (act == 0).any() and (act > 0).sum() > N // 10                # inactive planes and touching ones
    if not zero:
        assert not np.array_equal(moving["f"], static["f"])
    return ref


@pytest.mark.parametrize("P,per", [(1, False), (4, True), (4, False), (1, True)])
@pytest.mark.parametrize("n_points", [0, 8])
@pytest.mark.parametrize("zero", [True, False])
def test_moving_forces_match_the_restatement_bit_for_bit(exe, tmp_path, P, per, n_points, zero):
    _check_forces(exe, tmp_path, 100 + P + n_points, 500, P, per, n_points, zero)


def test_a_belt_drags_along_its_velocity():
    """a point at rest pressed into a plane that slides along +x: the friction force points along +x (ct_plane_forces gives none)"""
    plane = CR.plane([0, 0, 1.0], 0.0, 1e4, 0.0, 0.5, 1e-3)
    vel = np.array([[0.2, 0.0, 0.0, 0.0]])
    p, v = np.array([[0.1, 0.2, -1e-3]]), np.zeros((1, 3))
    f = ES.plane_forces_moving(plane[None], vel, p, v)[0]
    assert f[0, 0] > 0 and f[0, 1] == 0 and f[0, 2] == 1e4 * 1e-3
    assert np.isclose(f[0, 0], 0.5 * 10.0, rtol=1e-12)
    assert not CR.plane_forces(plane[None], p, v)[0][0, :2].any()
    # a table rising at 0.1 m/s is damped against a resting point as if the point sank at 0.1 m/s
    pl = CR.plane([0, 0, 1.0], 0.0, 1e4, 50.0)
    up = ES.plane_forces_moving(pl[None], np.array([[0, 0, 0.1, 0.1]]), p, v)[0]
    assert np.array_equal(up, CR.plane_forces(pl[None], p, np.array([[0, 0, -0.1]]))[0])


# ------------------------------------------------------------------ the keyframe rules of the attach entry
def _check(exe, tmp, key, planes, mode):
    key = np.asarray(key, float)
    K, n = key.shape[:2]
    cols = key.shape[3] if key.ndim == 4 else 1
    with open(tmp / "cin.bin", "wb") as f:
        f.write(np.array([planes, K, n, cols, mode], np.int32).tobytes())
        f.write(np.ascontiguousarray(key).tobytes())
    out = subprocess.run([exe, "check", str(tmp / "cin.bin")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    return out.stdout.strip()


def test_keyframe_rules(exe, tmp_path):
    rng = np.random.default_rng(2)
    for planes in (0, 1):
        for B in (0, 3):
            good = _keyframes(rng, planes, 3, 2, B)
            assert _check(exe, tmp_path, good, planes, ES.LINEAR) == "ok"
            where = " of instance 2" if B else ""
            at = (lambda k, it, w: (k, it, w, 2)) if B else (lambda k, it, w: (k, it, w))
            what = "plane" if planes else "obstacle"
            for bad in (np.nan, np.inf):
                k2 = good.copy()
                k2[at(1, 1, 5)] = bad
                assert _check(exe, tmp_path, k2, planes, ES.HOLD) == f"keyframe 1, {what} 1{where}: word 5 is not finite"
            k2 = good.copy()
            n0 = 0 if planes else 1
            it = 0 if planes else 1                                     # (item 1 of the obstacle keyframes is a half-space)
            k2[2, it, n0:n0 + 3] = -k2[1, it, n0:n0 + 3]
            msg = _check(exe, tmp_path, k2, planes, ES.LINEAR)
            assert msg.startswith(f"keyframes 1 and 2, {what} {it}") and "n_a . n_b < 0" in msg
            assert _check(exe, tmp_path, k2, planes, ES.HOLD) == "ok"    # HOLD never interpolates
            if planes:
                k2 = good.copy()
                k2[at(0, 1, 11)] = 1e-300
                assert _check(exe, tmp_path, k2, 1, ES.HOLD) == f"keyframe 0, plane 1{where}: the reserved word 11 is not 0"
            else:
                k2 = good.copy()
                k2[at(2, 0, 0)] = 1.0
                assert "kind 1 differs from keyframe 0" in _check(exe, tmp_path, k2, 0, ES.HOLD)
                k2 = good.copy()
                k2[at(1, 0, 0)] = 2.0
                assert "unknown kind 2" in _check(exe, tmp_path, k2, 0, ES.HOLD)
                for scale in (1.0 + 3e-6, 1.0 - 3e-6, 0.0):
                    k2 = good.copy()
                    k2[1, 1, 1:4] *= scale
                    assert f"keyframe 1, obstacle 1{' of instance 0' if B else ''}: the half-space normal has length" in _check(exe, tmp_path, k2, 0, ES.HOLD)
                k2 = good.copy()
                k2[1, 1, 1:4] *= 1.0 + 5e-7                              # within 1e-6 of unit length
                assert _check(exe, tmp_path, k2, 0, ES.LINEAR) == "ok"
                k2 = good.copy()
                k2[at(0, 0, 7)] = -1e-9
                assert "radius" in _check(exe, tmp_path, k2, 0, ES.HOLD)
