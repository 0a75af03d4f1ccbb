"""The plant model of the resident simulator, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument
and call-order errors come back with the documented codes before the device is needed and write nothing; the Python facade raises the
same; the host build of csrc/saip_plant.h (tests/cpp/plant_host.cpp, also under ASan/UBSan) matches the NumPy restatement
tests/plant_ref.py bit for bit in every output; the restatement has the properties of friction, of a stop and of a bounded draw."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plant_ref as PL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_plant_attach", "saip_batch_plant_detach", "saip_batch_plant_info", "saip_batch_plant_set_joints_host",
                  "saip_batch_plant_set_wrenches_host", "saip_batch_plant_randomize", "saip_batch_plant_set_period", "saip_batch_plant_summary_host",
                  "saip_batch_plant_summary_reset"]
POINTER_ENTRIES = ["saip_batch_plant_joints_device", "saip_batch_plant_wrenches_device", "saip_batch_plant_torques_device", "saip_batch_plant_summary_device"]
WORDS = ["gain", "bias", "tau_max", "fv", "fc", "v_s", "q_lo", "q_hi", "k_stop", "c_stop"]


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
    src = open(os.path.join(PKG, "csrc", "saip_plant.h")).read()
    for name, val in [("JOINT_WORDS", 10), ("WRENCH_WORDS", 8), ("MAX_WRENCHES", 4), ("SUMMARY_ROWS", 4), ("FRAME_WORLD", 0), ("FRAME_LINK", 1)]:
        assert re.search(rf"#define SAIP_PLANT_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_PLANT_" + name) == val == getattr(PL, name)
        assert re.search(rf"\bPLANT_{name} = {val}\b", src), name
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    assert "csrc/saip_plant.hip" in capi.SOURCES and "csrc/saip_plant.h" in capi.HEADERS
    assert list(sp.RobotController.PLANT_JOINT_WORDS) == WORDS


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
    v, per, out = C.c_int(7), C.c_longlong(7), np.full(7 * 10 * 4, 7.0)
    assert L.saip_batch_plant_detach(b) == code
    assert L.saip_batch_plant_info(b, C.byref(v), None, None, C.byref(per)) == code
    assert L.saip_batch_plant_set_joints_host(b, _dp(out)) == code
    assert L.saip_batch_plant_set_wrenches_host(b, _dp(out)) == code
    assert L.saip_batch_plant_randomize(b, 1, 0, _dp(out), _dp(out), None, None) == code
    assert L.saip_batch_plant_set_period(b, 3) == code
    assert L.saip_batch_plant_summary_host(b, _dp(out)) == code
    assert L.saip_batch_plant_summary_reset(b) == code
    for name in POINTER_ENTRIES:
        assert getattr(L, name)(b) is None
    assert v.value == 7 and per.value == 7 and (out == 7.0).all()      # nothing was written


JOINTS = PL.neutral(7, -2.0, 2.0)
JOINTS[:, PL.TAU_MAX], JOINTS[:, PL.FV], JOINTS[:, PL.FC], JOINTS[:, PL.VS], JOINTS[:, PL.K_STOP], JOINTS[:, PL.C_STOP] = 50.0, 0.1, 0.5, 0.01, 1e3, 10.0
WRENCHES = np.array([[0.0, 0.0, -9.81, 0.0, 0.0, 0.0, 0.0, np.inf], [1.0, 0.0, 0.0, 0.0, 0.1, 0.0, 40.0, 45.0]])


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_plant_attach
    links, frames = np.array([7, 4], np.int32), np.array([0, 1], np.int32)
    points = np.array([[0.0, 0.0, 0.1], [0.01, 0.0, 0.0]])

    def call(b, joints=JOINTS, perj=0, W=2, links=links, points=points, frames=frames, wr=WRENCHES, perw=0):
        return att(b, None if joints is None else _dp(np.ascontiguousarray(joints)), perj, W, None if links is None else _ip(links),
                   None if points is None else _dp(points), None if frames is None else _ip(frames), None if wr is None else _dp(np.ascontiguousarray(wr)), perw)

    def refused(b, msg, **kw):
        assert call(b, **kw) == INVALID and msg in L.saip_last_error(), (kw, L.saip_last_error())
        assert L.saip_batch_plant_info(b, None, None, None, None) == ORDER            # nothing got attached

    assert call(None) == INVALID
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert call(b) == ORDER                                          # before finalize, whatever the arguments
        assert call(b, W=9) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for W in (-1, 5, 2**31 - 1):
            refused(b, b"wrenches required", W=W)
        for kw in (dict(links=None), dict(points=None), dict(frames=None), dict(wr=None)):
            refused(b, b"null links, points, frames or wrench table", **kw)
        for bad in (-1, 10_000):
            l2 = links.copy()
            l2[1] = bad
            refused(b, b"wrench 1: link index", links=l2)
        for bad in (np.nan, np.inf):
            p2 = points.copy()
            p2[0, 2] = bad
            refused(b, b"wrench 0: the point is not finite", points=p2)
        for bad in (-1, 2):
            f2 = frames.copy()
            f2[1] = bad
            refused(b, b"wrench 1: unknown frame", frames=f2)
        # one bad word of one joint, batch-uniform and per instance (there: of one instance only).  Every refusal of the issue's list:
        # NaN anywhere; tau_max, fv, fc, k_stop, c_stop below 0; fc > 0 with v_s <= 0; q_lo > q_hi
        per = np.ascontiguousarray(np.repeat(JOINTS[:, :, None], B, axis=2))
        cases = [(j % 7, k, np.nan, b"word %s is NaN" % WORDS[k].encode()) for j, k in enumerate(range(10))]
        cases += [(2, k, -1e-9, b"word %s = -1e-09 is below 0" % WORDS[k].encode()) for k in (PL.TAU_MAX, PL.FV, PL.FC, PL.K_STOP, PL.C_STOP)]
        cases += [(5, k, np.inf, b"word %s is not finite" % WORDS[k].encode()) for k in (PL.GAIN, PL.BIAS, PL.FV, PL.FC, PL.K_STOP, PL.C_STOP)]
        cases += [(6, PL.VS, 0.0, b"word v_s = 0 must be positive when fc > 0"), (6, PL.VS, -1.0, b"word v_s = -1 must be positive when fc > 0"),
                  (0, PL.Q_LO, 2.5, b"word q_lo = 2.5 is above q_hi = 2"), (1, PL.Q_HI, -np.inf, b"word q_lo = -2 is above q_hi = -inf")]
        for j, k, val, msg in cases:
            t1 = JOINTS.copy()
            t1[j, k] = val
            refused(b, b"joint %d: " % j + msg, joints=t1)
            t2 = per.copy()
            t2[j, k, B - 1] = val
            refused(b, b"joint %d of instance 3: " % j + msg, joints=t2, perj=1)
        perw = np.ascontiguousarray(np.repeat(WRENCHES[:, :, None], B, axis=2))
        for k, e, val, msg in [(0, 2, np.nan, b"word F[2]"), (1, 4, np.inf, b"word M[1]"), (1, 6, np.nan, b"word p_start"), (0, 7, np.nan, b"word p_end")]:
            w1 = WRENCHES.copy()
            w1[k, e] = val
            refused(b, b"wrench %d: " % k + msg + b" is not finite", wr=w1)
            w2 = perw.copy()
            w2[k, e, 1] = val
            refused(b, b"wrench %d of instance 1: " % k + msg, wr=w2, perw=1)
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached
        free = JOINTS.copy()
        free[:, PL.FC], free[:, PL.VS], free[:, PL.TAU_MAX], free[:, PL.Q_LO], free[:, PL.Q_HI] = 0.0, -3.0, 0.0, -np.inf, np.inf
        win = WRENCHES.copy()
        win[:, 6:] = [[-np.inf, np.inf], [5.0, 5.0]]
        for kw in (dict(), dict(joints=None), dict(joints=None, perj=1), dict(joints=per, perj=1), dict(wr=perw, perw=1), dict(W=0, links=None, points=None, frames=None, wr=None),
                   dict(joints=free), dict(wr=win), dict(joints=PL.neutral(7))):
            assert call(b, **kw) == NO_DEVICE and b"no CPU path" in L.saip_last_error(), kw
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_the_plant(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_plant_attach(b, None, 0, 0, None, None, None, None, 0) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    neutral = ctrl.neutralPlantJoints()
    lim = robot.jointLimits()
    assert neutral.shape == (7, 10) and np.array_equal(neutral[:, PL.Q_LO], lim["position_lower"]) and np.array_equal(neutral[:, PL.Q_HI], lim["position_upper"])
    assert np.array_equal(neutral[:, [0, 1, 2, 3, 4, 5, 8, 9]], np.tile([1, 0, np.inf, 0, 0, 0, 0, 0], (7, 1)))
    for bad in (np.zeros(10), np.zeros((6, 10)), np.zeros((7, B, 10))):
        with pytest.raises(ValueError, match="joints of shape"):
            ctrl.attachPlant(bad)
    for bad in (np.zeros((7, 10)), np.zeros((7, 10, B)), np.zeros((7, B + 1, 10))):
        with pytest.raises(ValueError, match="per-instance joints of shape"):
            ctrl.attachPlant(bad, per_instance=True)
    ok = ("end-effector", (0, 0, 0.1), "world", [0, 0, -9.81, 0, 0, 0])
    with pytest.raises(ValueError, match="unknown link"):
        ctrl.attachPlant(wrenches=[("no-such-link", (0, 0, 0), "world", np.zeros(8))])
    with pytest.raises(ValueError, match="point of shape"):
        ctrl.attachPlant(wrenches=[("link4", (0, 0), "world", np.zeros(8))])
    with pytest.raises(ValueError, match="frame 'world' or 'link'"):
        ctrl.attachPlant(wrenches=[("link4", (0, 0, 0), "tool", np.zeros(8))])
    with pytest.raises(ValueError, match="values of shape"):
        ctrl.attachPlant(wrenches=[("link4", (0, 0, 0), "link", np.zeros(7))])
    with pytest.raises(ValueError, match="values of shape"):
        ctrl.attachPlant(wrenches=[("link4", (0, 0, 0), "link", np.zeros(8))], per_instance=True)
    with pytest.raises(ValueError, match="wrenches required"):
        ctrl.attachPlant(wrenches=[ok] * 5)
    t = neutral.copy()
    t[3, PL.FC] = 1.0
    with pytest.raises(ValueError, match="joint 3: word v_s = 0 must be positive"):
        ctrl.attachPlant(t)
    for kw in (dict(), dict(joints=neutral), dict(wrenches=[ok]), dict(per_instance=True),
               dict(joints=np.repeat(neutral[:, None, :], B, axis=1), wrenches=[("link4", (0, 0, 0), "link", np.zeros((B, 6)))], per_instance=True)):
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            ctrl.attachPlant(**kw)
    for fn in (ctrl.detachPlant, ctrl.plantInfo, ctrl.plantSummary, ctrl.resetPlantSummary, lambda: ctrl.setPlantPeriod(3), lambda: ctrl.setPlantJoints(neutral),
               lambda: ctrl.setPlantWrenches(np.zeros((1, 8))), lambda: ctrl.randomizePlant(1, joints=(neutral, neutral))):
        with pytest.raises(sp.SaipError, match="no plant model is attached"):
            fn()
    assert ctrl.plantTorquesDevice() is None and ctrl.plantJointsDevice() is None and ctrl.plantWrenchesDevice() is None and ctrl.plantSummaryDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "plant_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("plant_host"), "plant_host", []),
            _build(tmp_path_factory.mktemp("plant_host_san"), "plant_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _rotations(rng, shape):
    Q = np.linalg.qr(rng.normal(size=shape + (3, 3)))[0]
    Q[..., :, 0] *= np.sign(np.linalg.det(Q))[..., None]
    return Q


def _joint_table(rng, n, shape):
    """random non-neutral rows of shape (n,) + shape + (10,), with a neutral row, a row with tau_max = 0 and one without Coulomb friction"""
    t = np.empty((n,) + shape + (10,))
    t[..., PL.GAIN], t[..., PL.BIAS] = rng.uniform(0.8, 1.2, t.shape[:-1]), rng.uniform(-0.5, 0.5, t.shape[:-1])
    t[..., PL.TAU_MAX] = rng.uniform(1.0, 6.0, t.shape[:-1])
    t[..., PL.FV], t[..., PL.FC], t[..., PL.VS] = rng.uniform(0, 0.3, t.shape[:-1]), rng.uniform(0.1, 1.0, t.shape[:-1]), rng.uniform(0.05, 0.2, t.shape[:-1])
    t[..., PL.Q_LO], t[..., PL.Q_HI] = rng.uniform(-1.0, -0.5, t.shape[:-1]), rng.uniform(0.5, 1.0, t.shape[:-1])
    t[..., PL.K_STOP], t[..., PL.C_STOP] = rng.uniform(100, 1000, t.shape[:-1]), rng.uniform(0, 20, t.shape[:-1])
    t[0] = PL.neutral(1)[0]
    if n > 1:
        t[1, ..., PL.TAU_MAX] = 0.0
    if n > 2:
        t[2, ..., PL.FC], t[2, ..., PL.VS] = 0.0, -1.0
    return t


def _case(seed, N, J, W, perj, perw, S=3):
    """S substeps of N instances: torques beyond and inside the limits and NaN, q on both sides of the limits, exactly at them and inside,
    dq on both sides of v_s and exactly 0; revolute and prismatic joints; wrenches in both frames whose windows are empty, half-open,
    infinite or cover some of the S periods"""
    rng = np.random.default_rng(seed)
    c = dict(N=N, J=J, W=W, perj=perj, perw=perw, S=S, p0=int(rng.integers(3, 9)), dt=5e-4)
    c["joints"] = _joint_table(rng, J, (N,) if perj else ())
    c["rev"] = (np.arange(J) + seed) % 3 != 0
    c["frames"] = [(w + seed) % 2 for w in range(W)]
    c["anc"] = [int(rng.integers(1, 2 ** J)) if w else 2 ** J - 1 for w in range(W)]
    if W > 2:
        c["anc"][2] = 0                                                  # a link welded to the base: the wrench moves nothing
    wr = rng.uniform(-20, 20, (W,) + ((N,) if perw else ()) + (8,))
    p0, inf = c["p0"], np.inf
    windows = [(-inf, inf), (p0 + 1, inf), (p0 + 1, p0 + 1), (-inf, p0 + 2)]
    for w in range(W):
        wr[w, ..., 6:] = windows[w]
    if perw and W:
        wr[0, ::2, 6:] = (p0 + 1, p0 + 2)
    c["wrenches"] = wr
    c["summary"] = np.abs(rng.normal(size=(N, 4)))
    steps = []
    for s in range(S):
        t = rng.uniform(-8, 8, (N, J))
        t[rng.random((N, J)) < 0.1] = np.nan
        q = rng.uniform(-1.3, 1.3, (N, J))
        lo = c["joints"][..., PL.Q_LO].T if perj else np.broadcast_to(c["joints"][:, PL.Q_LO], (N, J))
        hi = c["joints"][..., PL.Q_HI].T if perj else np.broadcast_to(c["joints"][:, PL.Q_HI], (N, J))
        at = rng.random((N, J))
        q = np.where((at < 0.1) & np.isfinite(lo), lo, np.where((at > 0.9) & np.isfinite(hi), hi, q))
        dq = rng.uniform(-0.4, 0.4, (N, J)) * rng.choice([0.1, 1.0], (N, J))
        dq[rng.random((N, J)) < 0.1] = 0.0
        aw = rng.normal(size=(N, J, 3))
        aw /= np.linalg.norm(aw, axis=-1, keepdims=True)
        steps.append(dict(t=t, q=q, dq=dq, aw=aw, oj=rng.uniform(-1, 1, (N, J, 3)), p=rng.uniform(-1, 1, (N, W, 3)), Rl=_rotations(rng, (N, W))))
    c["steps"] = steps
    c["seed"], c["round"] = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
    jl, jh = _joint_table(rng, J, ()), _joint_table(rng, J, ())
    jl[..., PL.Q_HI] += 1.0                                              # (any bounds do for the arithmetic; some equal, some reversed)
    jh[:, ::3] = jl[:, ::3]
    wl, wh = rng.uniform(-20, 0, (W, 8)), rng.uniform(0, 20, (W, 8))
    wl[:, 6:], wh[:, 6:] = (3.0, 50.0), (9.75, 50.0)
    wh[:, 1] = wl[:, 1]
    wl[:, 2], wh[:, 2] = wh[:, 2].copy(), wl[:, 2].copy()
    c["bounds"] = (jl, jh, wl, wh)
    return c


def _run(exe, tmp, c):
    N, J, W, S = c["N"], c["J"], c["W"], c["S"]
    T = lambda a: np.ascontiguousarray(np.moveaxis(np.asarray(a, float), 0, -1))       # instance-major -> instance last
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, J, W, c["perj"], c["perw"], S], np.int32).tobytes())
        f.write(np.array([c["p0"]], np.int64).tobytes())
        f.write(np.array([c["dt"]]).tobytes())
        f.write(np.asarray(c["rev"], np.int32).tobytes())
        f.write(np.asarray(c["frames"], np.int32).tobytes())
        f.write(np.asarray(c["anc"], np.uint32).tobytes())
        jt, wt = c["joints"], c["wrenches"]
        f.write(np.ascontiguousarray(jt.transpose(0, 2, 1) if c["perj"] else jt).tobytes())
        f.write(np.ascontiguousarray(wt.transpose(0, 2, 1) if c["perw"] else wt).tobytes())
        f.write(T(c["summary"]).tobytes())
        for st in c["steps"]:
            for k in ("t", "q", "dq", "aw", "oj", "p"):
                f.write(T(st[k]).tobytes())
            f.write(T(st["Rl"].reshape(N, W, 9)).tobytes())
        f.write(np.array([c["seed"]], np.uint64).tobytes())
        f.write(np.array([c["round"], 0], np.uint32).tobytes())
        for a in c["bounds"]:
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    got, at = {}, 0
    for name, shp in [("tau", (S, J, N)), ("summary", (4, N)), ("dj", (J, 10, N)), ("dw", (W, 8, N))]:
        k = int(np.prod(shp))
        got[name] = raw[at:at + k].reshape(shp)
        at += k
    assert at == raw.size
    return got


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


CASES = [(1, 67, 7, 2, 0, 0), (2, 5, 7, 4, 1, 1), (3, 64, 30, 3, 1, 0), (4, 33, 2, 1, 0, 1), (5, 9, 3, 0, 1, 0), (6, 1, 1, 4, 0, 0)]


@pytest.mark.parametrize("seed,N,J,W,perj,perw", CASES)
def test_host_build_matches_the_restatement_bit_for_bit(exes, tmp_path, seed, N, J, W, perj, perw):
    c = _case(seed, N, J, W, perj, perw)
    # what the cases must cover (over the whole list: asserted on the first, which is large enough to hit them all)
    want_tau, s = [], c["summary"]
    for k, st in enumerate(c["steps"]):
        tau, s = PL.apply(c["joints"], st["t"], st["q"], st["dq"], s, c["dt"], c["p0"] + k, c["wrenches"], c["frames"], c["anc"], c["rev"], st["aw"], st["oj"],
                          st["p"], st["Rl"])
        want_tau.append(tau.T)
    jl, jh, wl, wh = c["bounds"]
    dj, dw = PL.draw(c["seed"], c["round"], PL.TABLE_JOINTS, N, jl, jh), PL.draw(c["seed"], c["round"], PL.TABLE_WRENCHES, N, wl, wh)
    if seed == 1:
        st = c["steps"][0]
        _, fr, stp, clip = PL.joint(c["joints"], st["t"], st["q"], st["dq"])
        lo, hi, vs = c["joints"][:, PL.Q_LO], c["joints"][:, PL.Q_HI], c["joints"][:, PL.VS]
        assert np.isnan(st["t"]).any() and (clip[:, 3:] > 0).any() and (clip[:, 3:] == 0).any() and (clip[:, 1] > 0).any()
        assert (st["q"] == lo).any() and (st["q"] == hi).any() and (st["q"] < lo).any() and (st["q"] > hi).any()
        assert not stp[st["q"] == lo].any() and not stp[st["q"] == hi].any()                   # exactly at a limit: inside
        a = np.abs(st["dq"][:, 3:])
        assert (a > vs[3:]).any() and ((a < vs[3:]) & (a > 0)).any() and (a == 0).any()
        assert c["rev"].any() and not c["rev"].all() and set(c["frames"]) == {0, 1}
    for exe in exes:
        got = _run(exe, tmp_path, c)
        assert np.array_equal(_bits(got["tau"]), _bits(np.stack(want_tau))), np.abs(got["tau"] - np.stack(want_tau)).max()
        assert np.array_equal(_bits(got["summary"]), _bits(s.T))
        assert np.array_equal(_bits(got["dj"]), _bits(dj.transpose(0, 2, 1)))
        assert np.array_equal(_bits(got["dw"]), _bits(dw.transpose(0, 2, 1)))


def test_wrench_windows_of_the_cases():
    """the four windows of _case are what they are meant to be over its S periods: always, from the second period on, never, the first two"""
    c = _case(2, 4, 7, 4, 0, 0)
    acts = np.array([PL.wrench_acts(c["wrenches"], c["p0"] + k)[:, 0] for k in range(3)])
    assert acts.T.tolist() == [[True, True, True], [False, True, True], [False, False, False], [True, True, False]]


# ------------------------------------------------------------------ properties of the restatement
def test_friction_never_adds_energy_and_a_stop_never_pulls():
    rng = np.random.default_rng(11)
    N, J = 4000, 6
    table = _joint_table(rng, J, (N,))
    t, q = rng.uniform(-8, 8, (N, J)), rng.uniform(-1.5, 1.5, (N, J))
    dq = rng.uniform(-1, 1, (N, J)) * rng.choice([1e-6, 1e-2, 1.0], (N, J))
    dq[rng.random((N, J)) < 0.05] = 0.0
    tau, fr, st, clip = PL.joint(table, t, q, dq)
    assert (fr * dq >= 0).all() and (fr[dq == 0] == 0).all()
    lo, hi = table[..., PL.Q_LO].T, table[..., PL.Q_HI].T
    assert (st[q < lo] >= 0).all() and (st[q > hi] <= 0).all() and not st[(q >= lo) & (q <= hi)].any()
    assert (st[q < lo] > 0).any() and (st[q > hi] < 0).any()
    u2 = tau + fr - st
    assert (np.abs(u2) <= table[..., PL.TAU_MAX].T * (1 + 1e-12) + 1e-12).all() and (clip >= 0).all()
    # the neutral row passes the torque through (NaN -> 0), whatever the state
    t[::7] = np.nan
    tau = PL.joint(PL.neutral(J), t, q, dq)[0]
    assert np.array_equal(tau, np.where(np.isnan(t), 0.0, t))
    # tau_max = 0: the actuator is dead, what is left is friction and the stop
    dead = PL.neutral(J)
    dead[:, PL.TAU_MAX] = 0.0
    tau, fr, st, clip = PL.joint(dead, t, q, dq)
    assert not tau.any() and np.array_equal(clip, np.abs(np.where(np.isnan(t), 0.0, t)))


def test_the_draw_is_bounded_exact_and_reproducible():
    rng = np.random.default_rng(5)
    lo, hi = rng.uniform(-3, 3, (6, 10)), rng.uniform(-3, 3, (6, 10))
    hi[:, ::4] = lo[:, ::4]
    lo[2, 2] = hi[2, 2] = np.inf
    lo[3, 6], hi[3, 6] = -1000.3, 1e-3                                   # a wide interval: the roundings must not leave it
    d = PL.draw(0x123456789ABCDEF, 3, PL.TABLE_JOINTS, 500, lo, hi)
    assert d.shape == (6, 500, 10)
    mn, mx = np.minimum(lo, hi)[:, None, :], np.maximum(lo, hi)[:, None, :]
    assert ((d >= mn) & (d <= mx)).all()
    same = np.broadcast_to((lo == hi)[:, None, :], d.shape)
    assert np.array_equal(d[same], np.broadcast_to(lo[:, None, :], d.shape)[same])
    assert np.array_equal(d, PL.draw(0x123456789ABCDEF, 3, PL.TABLE_JOINTS, 500, lo, hi))
    for other in (PL.draw(0x123456789ABCDEF, 4, PL.TABLE_JOINTS, 500, lo, hi), PL.draw(0x123456789ABCDEE, 3, PL.TABLE_JOINTS, 500, lo, hi),
                  PL.draw(0x123456789ABCDEF, 3, PL.TABLE_WRENCHES, 500, lo, hi)[..., :6]):
        k = other.shape[-1]
        assert (other != d[..., :k])[~same[..., :k]].mean() > 0.999
    assert np.ptp(d[~same].reshape(-1)) > 1.0 and len(np.unique(d[0, :, 1])) == 500
    w = PL.draw(7, 0, PL.TABLE_WRENCHES, 200, np.array([[0, 0, 0, 0, 0, 0, 3.0, 10.0]]), np.array([[1, 1, 1, 1, 1, 1, 9.75, 10.0]]))
    assert np.array_equal(w[..., 6:], np.floor(w[..., 6:])) and set(w[0, :, 6]) == {3.0, 4.0, 5.0, 6.0, 7.0, 8.0, 9.0} and (w[..., 7] == 10.0).all()
    assert (w[..., :6] != np.floor(w[..., :6])).all()
