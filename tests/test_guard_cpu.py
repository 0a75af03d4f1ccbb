"""Resident guards, host side (no GPU needed): the C-ABI entries are declared, exported and bound and the constants agree everywhere; the
argument and call-order errors come back with the documented codes before the device is needed and write nothing; the Python facade raises
the same; the host build of csrc/saip_guard.h (tests/cpp/guard_host.cpp, also under ASan/UBSan) matches the NumPy restatement
tests/guard_ref.py bit for bit on random sequences; and both pass analytic checks of the debounce, the blanking time, the priority of the
lower guard, re-entry, one transition per period and the OFFSET mode."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import guard_ref as GR
from test_sensing_cpu import _controller_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_guard_attach", "saip_batch_guard_detach", "saip_batch_guard_info", "saip_batch_guard_set_guards_host", "saip_batch_guard_reset",
                  "saip_batch_guard_evaluate", "saip_batch_guard_state_host", "saip_batch_guard_state_device", "saip_batch_guard_readout_host",
                  "saip_batch_guard_add_cost"]
POINTER_ENTRIES = ["saip_batch_guard_guards_device", "saip_batch_guard_readout_device"]
WORDS = ["from", "to", "signal", "axis", "cmp", "threshold", "hold", "blank"]


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
    src = open(os.path.join(PKG, "csrc", "saip_guard.h")).read()
    consts = [("MAX_PHASES", 8, GR.MAX_PHASES, "GUARD_MAX_PHASES"), ("MAX_GUARDS", 8, GR.MAX_GUARDS, "GUARD_MAX_GUARDS"), ("WORDS", 8, GR.WORDS, "GUARD_WORDS"),
              ("PHASE_WORDS", 4, GR.PHASE_WORDS, "GUARD_PHASE_WORDS"), ("READOUT_ROWS", 8, GR.READOUT_ROWS, "GUARD_READOUT_ROWS")]
    for name, val, ref, srcname in consts:
        assert re.search(rf"#define SAIP_GUARD_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_GUARD_" + name) == val == ref
        assert re.search(rf"\b{srcname} = {val}\b", src), name
    # the enumerations: saip.h, capi, the restatement and the order of the header's enum lists
    signals = ["PERIODS", "FORCE", "MOMENT", "POSITION", "POS_ERROR", "ORI_ERROR", "JOINT_SPEED"]
    for k, name in enumerate(signals):
        assert re.search(rf"#define SAIP_GUARD_{name} {k}\b", hdr) and getattr(capi, "SAIP_GUARD_" + name) == k == getattr(GR, name)
    assert re.search(r"GUARD_SIGNAL_PERIODS = 0,\s+" + r",\s+".join("GUARD_SIGNAL_" + s for s in signals[1:]) + r",\s+GUARD_SIGNAL_COUNT", src)
    for k, (name, ref) in enumerate([("FREE", GR.FREE), ("HOLD", GR.HOLD_MODE), ("OFFSET", GR.OFFSET)]):
        assert re.search(rf"#define SAIP_GUARD_{name} {k}\b", hdr) and getattr(capi, "SAIP_GUARD_" + name) == k == ref
    assert "GUARD_MODE_FREE = 0, GUARD_MODE_HOLD, GUARD_MODE_OFFSET" in src
    for k, (name, ref) in enumerate([("GE", GR.GE), ("LE", GR.LE)]):
        assert re.search(rf"#define SAIP_GUARD_{name} {k}\b", hdr) and getattr(capi, "SAIP_GUARD_" + name) == k == ref
    assert "GUARD_FROM = 0, GUARD_TO, GUARD_SIGNAL, GUARD_AXIS, GUARD_CMP, GUARD_THRESHOLD, GUARD_HOLD, GUARD_BLANK" in src
    assert [GR.FROM, GR.TO, GR.SIGNAL, GR.AXIS, GR.CMP, GR.THRESHOLD, GR.HOLD, GR.BLANK] == list(range(8))
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    for f in ("csrc/saip_guard.hip", "csrc/saip_engine_guard.cpp"):
        assert f in capi.SOURCES
    assert "csrc/saip_guard.h" in capi.HEADERS
    assert "#pragma clang fp contract(off)" in src and "atomic" not in re.sub(r"//.*", "", src)
    for m in ("attachGuards", "detachGuards"):
        assert hasattr(sp.MotionForceTask, m)
    for m in ("evaluateGuards", "resetGuards", "guardState", "guardReadout", "guardCost"):
        assert hasattr(sp.RobotController, m)


def _others_refuse(L, b, code):
    v, out, ints = C.c_int(7), np.full(8 * 8 * 4, 7.0), np.full(8 * 4, 7, np.int32)
    assert L.saip_batch_guard_detach(b) == code
    assert L.saip_batch_guard_info(b, C.byref(v), C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == code
    assert L.saip_batch_guard_set_guards_host(b, _dp(out)) == code
    assert L.saip_batch_guard_reset(b) == code
    assert L.saip_batch_guard_evaluate(b) == code
    assert L.saip_batch_guard_state_host(b, _ip(ints), _ip(ints), _ip(ints), _ip(ints), _ip(ints), _ip(ints), _dp(out)) == code
    ptr = C.c_void_p(7)
    assert L.saip_batch_guard_state_device(b, *([C.byref(ptr)] * 7)) == code and ptr.value == 7
    assert L.saip_batch_guard_readout_host(b, _dp(out)) == code
    assert L.saip_batch_guard_add_cost(b, 0, 1.0, 2.0) == code
    assert L.saip_batch_guard_guards_device(b) is None and L.saip_batch_guard_readout_device(b) is None
    assert v.value == 7 and (out == 7.0).all() and (ints == 7).all()      # nothing was written


GUARDS = np.array([GR.guard(0, 1, GR.FORCE, 5.0, axis=3, hold=2), GR.guard(1, 2, GR.PERIODS, 5.0), GR.guard(2, 3, GR.POS_ERROR, 1e-3, cmp=GR.LE, hold=3, blank=2)], float)
PHASES = np.array([[GR.FREE, 0, 0, 0], [GR.HOLD_MODE, 0, 0, 0], [GR.OFFSET, 0, 0, 0.05], [GR.FREE, 0, 0, 0]], float)


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_guard_attach

    def call(b, task=0, guards=GUARDS, per=0, phases=PHASES, G=None, P=None):
        g, p = np.ascontiguousarray(guards, float), np.ascontiguousarray(phases, float)
        return att(b, task, g.shape[0] if G is None else G, _dp(g), per, p.shape[0] if P is None else P, _dp(p))

    def refused(b, msg, **kw):
        assert call(b, **kw) == INVALID and msg in L.saip_last_error(), (kw, L.saip_last_error())

    assert call(None) == INVALID and b"null batch" in L.saip_last_error()
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert call(b) == ORDER and b"saip_batch_finalize first" in L.saip_last_error()           # before finalize, whatever the arguments
        assert call(b, task=9, G=99) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        refused(b, b"task 2 is not a motion-force task", task=2)
        for t in (-1, 3):
            refused(b, b"task id %d out of range" % t, task=t)
        for n in (0, 9, -1):
            refused(b, b"1..8 guards required (got %d)" % n, G=n)
            refused(b, b"1..8 phases required (got %d)" % n, P=n)
        assert att(b, 0, 3, None, 0, 4, _dp(PHASES)) == INVALID and b"null guards or phases" in L.saip_last_error()
        assert att(b, 0, 3, _dp(GUARDS), 0, 4, None) == INVALID
        # one bad word of one guard, batch-uniform and per instance (there: of one instance only)
        per = np.ascontiguousarray(np.repeat(GUARDS[:, :, None], B, axis=2))
        cases = [(0, GR.FROM, 4.0, b"word from = 4 is outside the phases"), (1, GR.FROM, -1.0, b"word from = -1 is outside the phases"),
                 (2, GR.TO, 4.0, b"word to = 4 is outside the phases"), (0, GR.TO, 0.5, b"word to = 0.5 is not an integer"),
                 (0, GR.SIGNAL, 7.0, b"word signal = 7 is no signal"), (1, GR.SIGNAL, -1.0, b"word signal = -1 is no signal"),
                 (2, GR.SIGNAL, 1.5, b"word signal = 1.5 is not an integer"), (0, GR.AXIS, 4.0, b"word axis = 4 is no axis of the signal"),
                 (1, GR.AXIS, 1.0, b"word axis = 1 is no axis of the signal"), (2, GR.AXIS, -1.0, b"word axis = -1 is no axis of the signal"),
                 (0, GR.CMP, 2.0, b"word cmp = 2 is neither 0 (>=) nor 1 (<=)"), (0, GR.CMP, 0.5, b"word cmp = 0.5 is not an integer"),
                 (1, GR.THRESHOLD, np.nan, b"word threshold = nan is not finite"), (2, GR.THRESHOLD, np.inf, b"word threshold = inf is not finite"),
                 (0, GR.THRESHOLD, -np.inf, b"word threshold = -inf is not finite"), (0, GR.HOLD, 0.0, b"word hold = 0 is below 1"),
                 (1, GR.HOLD, 1.5, b"word hold = 1.5 is not an integer"), (2, GR.HOLD, np.nan, b"word hold = nan is not finite"),
                 (0, GR.BLANK, -1.0, b"word blank = -1 is below 0"), (1, GR.BLANK, 0.25, b"word blank = 0.25 is not an integer")]
        for g, k, val, msg in cases:
            t1 = GUARDS.copy()
            t1[g, k] = val
            refused(b, b"guard %d: " % g + msg, guards=t1)
            t2 = per.copy()
            t2[g, k, B - 1] = val
            refused(b, b"guard %d of instance 3: " % g + msg, guards=t2, per=1)
        # POSITION has axes 0..2 only, the wrench signals 0..3
        t1 = GUARDS.copy()
        t1[0, GR.SIGNAL], t1[0, GR.AXIS] = GR.POSITION, 3.0
        refused(b, b"guard 0: word axis = 3 is no axis of the signal", guards=t1)
        # the phases
        for p, k, val, msg in [(1, 0, 3.0, b"phase 1: word mode = 3 is no mode"), (2, 0, 0.5, b"phase 2: word mode = 0.5 is no mode"),
                               (3, 0, np.nan, b"phase 3: word mode = nan is no mode"), (0, 0, 1.0, b"phase 0: word mode = 1: phase 0 must be FREE"),
                               (0, 0, 2.0, b"phase 0 must be FREE"), (2, 1, np.nan, b"phase 2: word dx is not finite"), (2, 3, np.inf, b"phase 2: word dz is not finite"),
                               (1, 2, -np.inf, b"phase 1: word dy is not finite")]:
            t = PHASES.copy()
            t[p, k] = val
            refused(b, msg, phases=t)
        # a guard that points past a shorter phase table
        refused(b, b"guard 2: word to = 3 is outside the phases", P=3)
        # valid arguments reach the device check: a configuration-only batch has none
        for kw in (dict(), dict(task=1), dict(guards=per, per=1), dict(guards=GUARDS[:1], phases=PHASES[:2])):
            assert call(b, **kw) == NO_DEVICE, (kw, L.saip_last_error())
        _others_refuse(L, b, ORDER)
        assert b"no guards are attached (saip_batch_guard_attach)" in L.saip_last_error()
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_the_guards(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_guard_attach(b, 0, 3, _dp(GUARDS), 0, 4, _dp(PHASES)) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    task, joint = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [task, joint])
    touch = {"from": 0, "to": 1, "signal": "force", "axis": "norm", "cmp": ">=", "threshold": 5.0, "hold": 2}
    phases = [dict(mode="free"), dict(mode="hold"), dict(mode="offset", offset=(0, 0, 0.05))]
    assert not hasattr(joint, "attachGuards")
    with pytest.raises(ValueError, match="guard 0: unknown signal 'torque'"):
        task.attachGuards([dict(touch, signal="torque")], phases)
    with pytest.raises(ValueError, match="guard 0: unknown axis 'w'"):
        task.attachGuards([dict(touch, axis="w")], phases)
    with pytest.raises(ValueError, match="guard 0: unknown cmp '>'"):
        task.attachGuards([dict(touch, cmp=">")], phases)
    with pytest.raises(ValueError, match="guard 0: unknown keys"):
        task.attachGuards([dict(touch, debounce=2)], phases)
    with pytest.raises(ValueError, match=r"guard 0: key \[threshold\] is missing"):
        task.attachGuards([{k: v for k, v in touch.items() if k != "threshold"}], phases)
    with pytest.raises(ValueError, match="phase 1: unknown mode 'stop'"):
        task.attachGuards([touch], [dict(mode="free"), dict(mode="stop")])
    with pytest.raises(ValueError, match="phase 2: an offset of shape"):
        task.attachGuards([touch], [dict(mode="free"), dict(mode="hold"), dict(mode="offset", offset=(1, 2))])
    with pytest.raises(ValueError, match="a scalar expected for word 5"):
        task.attachGuards([dict(touch, threshold=np.ones(B))], phases)
    # the engine's refusals come through as ValueError with its message
    with pytest.raises(ValueError, match="guard 0: word hold = 0 is below 1"):
        task.attachGuards([dict(touch, hold=0)], phases)
    with pytest.raises(ValueError, match="guard 0: word to = 3 is outside the phases"):
        task.attachGuards([dict(touch, to=3)], phases)
    with pytest.raises(ValueError, match="guard 1 of instance 2: word threshold = nan is not finite"):
        thr = np.ones(B)
        thr[2] = np.nan
        task.attachGuards([touch, dict(touch, threshold=thr)], phases, per_instance=True)
    with pytest.raises(ValueError, match="phase 0 must be FREE"):
        task.attachGuards([touch], [dict(mode="hold"), dict(mode="free")])
    with pytest.raises(ValueError, match="1..8 guards required"):
        task.attachGuards([], phases)
    with pytest.raises(ValueError, match="1..8 phases required"):
        task.attachGuards([touch], [])
    with pytest.raises(sp.SaipNoDevice):
        task.attachGuards([touch, dict(touch, signal=GR.PERIODS, axis=0, **{"from": 1}, to=2)], phases)
    for fn in (task.detachGuards, ctrl.evaluateGuards, ctrl.resetGuards, ctrl.guardState, ctrl.guardReadout, ctrl.guardInfo, lambda: ctrl.guardCost(1, 1.0),
               lambda: task.setGuards([touch])):
        with pytest.raises(sp.SaipError, match="no guards are attached"):
            fn()


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "guard_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("guard_host"), "guard_host", []),
            _build(tmp_path_factory.mktemp("guard_host_san"), "guard_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


SIGNAL_KEYS = ("f", "m", "pos", "ep", "eo", "speed", "pose")


def _period(N, **kw):
    """the inputs of one evaluation, NaN where not given: f, m, pos (N, 3), ep, eo, speed (N,), pose (12, N)"""
    d = dict(f=np.full((N, 3), np.nan), m=np.full((N, 3), np.nan), pos=np.full((N, 3), np.nan), ep=np.full(N, np.nan), eo=np.full(N, np.nan),
             speed=np.full(N, np.nan), pose=np.full((12, N), np.nan))
    for k, v in kw.items():
        d[k] = np.broadcast_to(np.asarray(v, float), d[k].shape).copy()
    return d


def _run(exe, tmp, guards, phases, goal0, periods, have_pose=True, cost=None, w=(0.0, 0.0), cost_phase=0):
    guards, phases = np.asarray(guards, float), np.asarray(phases, float)
    N, G, P, K = goal0.shape[1], guards.shape[0], phases.shape[0], len(periods)
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, G, P, int(guards.ndim == 3), K, int(have_pose), 0, 0], np.int32).tobytes())
        f.write(np.ascontiguousarray(guards).tobytes())
        f.write(np.ascontiguousarray(phases).tobytes())
        f.write(np.ascontiguousarray(goal0[:24]).tobytes())
        for d in periods:
            for k in ("f", "m", "pos"):
                f.write(np.ascontiguousarray(d[k].T).tobytes())
            for k in ("ep", "eo", "speed", "pose"):
                f.write(np.ascontiguousarray(d[k]).tobytes())
        f.write(np.ascontiguousarray(np.zeros(N) if cost is None else cost, float).tobytes())
        f.write(np.array(w, np.float64).tobytes())
        f.write(np.array([cost_phase, 0], np.int32).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    rows = 3 + 2 * G + P + 12 + 24
    assert raw.size == K * rows * N + N
    per = raw[:K * rows * N].reshape(K, rows, N)
    res = []
    for k in range(K):
        a, at, d = per[k], 0, {}
        for name, r in (("phase", 1), ("since", 1), ("clock", 1), ("run", G), ("entry", P), ("fires", G)):
            d[name] = a[at:at + r].astype(np.int32).reshape((N,) if r == 1 and name in ("phase", "since", "clock") else (r, N))
            at += r
        d["latch"], d["goal"] = a[at:at + 12].copy(), a[at + 12:at + 36].copy()
        res.append(d)
    return res, raw[K * rows * N:]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ref(guards, phases, goal0, periods, have_pose=True):
    N = goal0.shape[1]
    gd, goal, res = GR.Guards(guards, phases, N), goal0[:24].copy(), []
    for d in periods:
        kw = {k: d[k] for k in SIGNAL_KEYS}
        if not have_pose:
            kw["pose"] = None
        gd.step(goal, **kw)
        s = gd.state()
        s["goal"] = goal.copy()
        res.append(s)
    return res, gd


def _same(a, b):
    for k in ("phase", "since", "clock", "run", "entry", "fires"):
        assert np.array_equal(a[k], b[k]), k
    for k in ("latch", "goal"):
        assert np.array_equal(_bits(a[k]), _bits(b[k])), k


def _both(exes, tmp_path, guards, phases, goal0, periods, have_pose=True):
    """the restatement's per-period results, asserted equal to both host builds'"""
    want, _ = _ref(guards, phases, goal0, periods, have_pose)
    for exe in exes:
        got, _ = _run(exe, tmp_path, guards, phases, goal0, periods, have_pose)
        for a, b in zip(got, want):
            _same(a, b)
    return want


def _random_case(seed, N, G, P, K, per):
    rng = np.random.default_rng(seed)
    sh = (G, N) if per else (G,)
    g = np.zeros((G, 8) + ((N,) if per else ()))
    sig = rng.integers(0, 7, sh)
    g[:, GR.FROM], g[:, GR.TO] = rng.integers(0, P, sh), rng.integers(0, P, sh)
    g[:, GR.SIGNAL] = sig
    g[:, GR.AXIS] = np.where((sig == GR.FORCE) | (sig == GR.MOMENT), rng.integers(0, 4, sh), np.where(sig == GR.POSITION, rng.integers(0, 3, sh), 0))
    g[:, GR.CMP] = rng.integers(0, 2, sh)
    g[:, GR.THRESHOLD] = np.where(sig == GR.PERIODS, rng.integers(0, 5, sh), rng.uniform(-0.5, 1.0, sh))
    g[:, GR.HOLD], g[:, GR.BLANK] = rng.integers(1, 4, sh), rng.integers(0, 4, sh)
    ph = np.zeros((P, 4))
    ph[1:, 0] = rng.integers(0, 3, P - 1)
    ph[:, 1:] = rng.uniform(-0.1, 0.1, (P, 3))
    periods = []
    for k in range(K):
        d = _period(N, f=rng.uniform(-1, 1, (N, 3)), m=rng.uniform(-1, 1, (N, 3)), pos=rng.uniform(-1, 1, (N, 3)), ep=rng.uniform(0, 1, N), eo=rng.uniform(0, 1, N),
                    speed=rng.uniform(0, 1, N), pose=rng.uniform(-1, 1, (12, N)))
        if k % 5 == 3:                                                   # non-finite signals: no special case anywhere
            for key, val in (("f", np.nan), ("m", np.inf), ("pos", -np.inf), ("ep", np.nan), ("eo", np.inf), ("speed", -np.inf)):
                d[key][rng.random(d[key].shape) < 0.2] = val
            d["pose"][rng.random((12, N)) < 0.05] = np.nan
        periods.append(d)
    return g, ph, rng.uniform(-1, 1, (24, N)), periods


@pytest.mark.parametrize("seed,N,G,P,K,per", [(1, 70, 8, 8, 40, 1), (2, 70, 8, 8, 40, 0), (3, 5, 3, 2, 12, 1), (4, 1, 1, 1, 6, 0)])
def test_host_build_matches_the_restatement_bit_for_bit(exes, tmp_path, seed, N, G, P, K, per):
    guards, phases, goal0, periods = _random_case(seed, N, G, P, K, per)
    want, gd = _ref(guards, phases, goal0, periods)
    cost0 = np.random.default_rng(seed).uniform(0, 3, N)
    if seed == 1:   # what the case must cover (the issue's case: B = 70, 40 periods, G = 8, P = 8, per-instance tables)
        assert guards.shape == (8, 8, 70) and len(phases) == 8 and len(periods) == 40
        assert set(np.unique(guards[:, GR.SIGNAL])) == set(range(7)) and set(phases[:, 0]) == {0.0, 1.0, 2.0}
        assert any(np.isnan(d["f"]).any() and np.isposinf(d["m"]).any() and np.isneginf(d["pos"]).any() for d in periods)
        assert (gd.fires.sum(axis=1) > 0).sum() >= 6 and len(np.unique(gd.phase)) >= 4 and (gd.entry[1:] >= 0).any() and (gd.entry < 0).any()
        assert not np.array_equal(_bits(want[-1]["goal"]), _bits(goal0))                         # HOLD / OFFSET phases wrote goals
    for exe in exes:
        for cp, w in ((P - 1, (0.25, np.inf)), (0, (3.0, -1.5))):
            got, cost = _run(exe, tmp_path, guards, phases, goal0, periods, cost=cost0, w=w, cost_phase=cp)
            assert np.array_equal(_bits(cost), _bits(GR.cost(cost0, gd.entry[cp], *w)))
        for a, b in zip(got, want):
            _same(a, b)
    # a launch that computed no pose leaves the latch as it is
    want = _both(exes, tmp_path, guards, phases, goal0, periods[:10], have_pose=False)
    assert all((w["latch"] == 0.0).all() for w in want)


# ------------------------------------------------------------------ analytic cases, on the restatement and both host builds
FREE4 = np.array([[GR.FREE, 0, 0, 0]] * 4, float)
GOAL0 = np.arange(24.0)[:, None] + np.zeros((24, 1))


def test_hold_is_a_debounce_over_consecutive_evaluations(exes, tmp_path):
    g = [GR.guard(0, 1, GR.JOINT_SPEED, 1.0, hold=3)]
    speed = [2, 2, 0, 2, 2, 2, 2]                                        # a false evaluation intervenes: fires on the third true one after it
    res = _both(exes, tmp_path, g, FREE4, GOAL0, [_period(1, speed=s) for s in speed])
    assert [int(r["phase"][0]) for r in res] == [0, 0, 0, 0, 0, 1, 1]
    assert [int(r["run"][0, 0]) for r in res] == [1, 2, 0, 1, 2, 0, 0]   # (every run is cleared by the transition; the guard is not of phase 1)
    assert res[-1]["entry"][1, 0] == 5 and res[-1]["fires"][0, 0] == 1
    res = _both(exes, tmp_path, g, FREE4, GOAL0, [_period(1, speed=2.0)] * 4)
    assert [int(r["phase"][0]) for r in res] == [0, 0, 1, 1]             # uninterrupted: on the third consecutive true evaluation


def test_blank_suppresses_a_condition_true_from_the_start(exes, tmp_path):
    g = [GR.guard(0, 1, GR.FORCE, -1.0, axis=2, cmp=GR.LE, blank=4), GR.guard(1, 2, GR.FORCE, -1.0, axis=2, cmp=GR.LE, blank=2, hold=2)]
    res = _both(exes, tmp_path, g, FREE4, GOAL0, [_period(1, f=(0, 0, -5.0))] * 10)
    # since = 0..3 are blanked: the guard is first evaluated at since = 4 (clock 4); in phase 1 since 0, 1 are blanked, then two evaluations
    assert [int(r["phase"][0]) for r in res] == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2]
    assert list(res[-1]["entry"][:3, 0]) == [0, 4, 8]
    assert [int(r["run"][1, 0]) for r in res[4:8]] == [0, 0, 0, 1]


def test_the_lower_guard_fires_and_only_one_transition_happens_per_period(exes, tmp_path):
    g = [GR.guard(0, 2, GR.PERIODS, 0.0), GR.guard(0, 1, GR.PERIODS, 0.0), GR.guard(2, 3, GR.PERIODS, 0.0), GR.guard(3, 0, GR.PERIODS, 0.0)]
    res = _both(exes, tmp_path, g, FREE4, GOAL0, [_period(1)] * 5)
    # guards 0 and 1 are both true in period 0: guard 0 wins; guard 2 (of the new phase, true at once) waits for the next period
    assert [int(r["phase"][0]) for r in res] == [2, 3, 0, 2, 3]
    assert list(res[0]["fires"][:, 0]) == [1, 0, 0, 0] and list(res[-1]["fires"][:, 0]) == [2, 0, 2, 1]
    assert all(int(r["since"][0]) == 0 for r in res) and [int(r["clock"][0]) for r in res] == [1, 2, 3, 4, 5]
    assert list(res[-1]["entry"][:, 0]) == [0, -1, 0, 1]                 # entry keeps the first time; phase 1 was never reached


def test_to_equal_from_reenters_the_phase(exes, tmp_path):
    g = [GR.guard(0, 1, GR.PERIODS, 1.0), GR.guard(1, 1, GR.PERIODS, 2.0)]
    ph = np.array([[GR.FREE, 0, 0, 0], [GR.HOLD_MODE, 0, 0, 0]], float)
    poses = [np.full((12, 1), 10.0 * k) + np.arange(12.0)[:, None] for k in range(8)]
    res = _both(exes, tmp_path, g, ph, GOAL0, [_period(1, pose=p) for p in poses])
    assert [int(r["phase"][0]) for r in res] == [0, 1, 1, 1, 1, 1, 1, 1]
    assert [int(r["since"][0]) for r in res] == [1, 0, 1, 2, 0, 1, 2, 0]  # since = 0 on every re-entry
    assert res[-1]["entry"][1, 0] == 1 and list(res[-1]["fires"][:, 0]) == [1, 2]
    for k, latched in ((1, 1), (3, 1), (4, 4), (6, 4), (7, 7)):           # the latch is retaken on re-entry, and HOLD writes it in every period
        assert np.array_equal(res[k]["latch"][:, 0], poses[latched][:, 0]) and np.array_equal(res[k]["goal"][:12, 0], poses[latched][:, 0])
        assert (res[k]["goal"][12:24, 0] == 0.0).all()
    assert np.array_equal(res[0]["goal"], GOAL0)                         # FREE wrote nothing


def test_offset_adds_to_the_latched_position_only(exes, tmp_path):
    g = [GR.guard(0, 1, GR.PERIODS, 0.0), GR.guard(1, 2, GR.PERIODS, 1.0), GR.guard(2, 3, GR.PERIODS, 1.0)]
    ph = np.array([[GR.FREE, 9, 9, 9], [GR.OFFSET, 0.1, -0.2, 0.05], [GR.HOLD_MODE, 7, 7, 7], [GR.FREE, 0, 0, 0]], float)
    pose = np.array([0.3, 0.1, 0.7, 1, 0, 0, 0, -1, 0, 0, 0, -1.0])[:, None]
    goal0 = np.full((24, 1), 5.0)
    res = _both(exes, tmp_path, g, ph, goal0, [_period(1, pose=pose + k) for k in range(6)])
    assert [int(r["phase"][0]) for r in res] == [1, 1, 2, 2, 3, 3]
    assert np.array_equal(res[0]["latch"], pose) and np.array_equal(res[1]["latch"], pose)
    want = pose[:, 0].copy()
    want[:3] = [0.3 + 0.1, 0.1 + -0.2, 0.7 + 0.05]                       # each sum rounded once
    assert np.array_equal(_bits(res[1]["goal"][:12, 0]), _bits(want)) and (res[1]["goal"][12:, 0] == 0.0).all()
    assert np.array_equal(res[1]["goal"][3:12], pose[3:12])              # the rotation is the latch, untouched
    assert np.array_equal(res[3]["goal"][:12], pose + 2)                 # HOLD ignores its offset words: the latch of period 2 itself
    assert np.array_equal(_bits(res[5]["goal"]), _bits(res[3]["goal"]))  # the final FREE phase leaves the rows as they stand


def test_a_nan_signal_satisfies_neither_comparison(exes, tmp_path):
    g = [GR.guard(0, 1, GR.POS_ERROR, 0.0, cmp=GR.GE), GR.guard(0, 1, GR.POS_ERROR, 0.0, cmp=GR.LE), GR.guard(0, 2, GR.MOMENT, 5.0, axis=3)]
    res = _both(exes, tmp_path, g, FREE4, GOAL0, [_period(1)] * 3 + [_period(1, m=(3.0, 0.0, 4.0))])
    assert [int(r["phase"][0]) for r in res] == [0, 0, 0, 2]             # sqrt((9 + 0) + 16) = 5 >= 5
    assert (res[2]["run"] == 0).all()
