"""The actuation chain of the resident simulator, host side (no GPU needed): the C-ABI entries are declared, exported and bound and the
constants agree everywhere; the argument and call-order errors come back with the documented codes before the device is needed and write
nothing; the Python facade raises the same; the host build of csrc/saip_plant_chain.h (tests/cpp/plant_chain_host.cpp, also under
ASan/UBSan) matches the NumPy restatement tests/plant_chain_ref.py bit for bit; and both pass analytic checks: the neutral row, a pure
delay, a rate-limited step, the step response of the lag, and taps that only a period's first substep moves."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import plant_chain_ref as PC
from test_plant_cpu import _controller_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_plant_chain_attach", "saip_batch_plant_chain_detach", "saip_batch_plant_chain_info", "saip_batch_plant_chain_set_table_host",
                  "saip_batch_plant_chain_randomize", "saip_batch_plant_chain_reset", "saip_batch_plant_chain_state_host", "saip_batch_plant_chain_state_device"]
POINTER_ENTRIES = ["saip_batch_plant_chain_table_device"]
WORDS = ["delay", "rate_max", "tau_lag"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    import plant_ref as PL
    import sensing_chain_ref as SC
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    src = open(os.path.join(PKG, "csrc", "saip_plant_chain.h")).read()
    hpp = open(os.path.join(ROOT, "include", "saip", "SaiPrimitivesBatched.hpp")).read()
    for name, val, ref, srcname in [("CHAIN_WORDS", 3, PC.WORDS, "PLANT_CHAIN_WORDS"), ("CHAIN_MAX_DEPTH", 8, PC.MAX_DEPTH, "PLANT_CHAIN_MAX_DEPTH"),
                                    ("TABLE_CHAIN", 9, PC.TABLE_CHAIN, "PLANT_TABLE_CHAIN")]:
        assert re.search(rf"#define SAIP_PLANT_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_PLANT_" + name) == val == ref
        assert re.search(rf"\b{srcname} = {val}\b", src), name
    assert "SAIP_PLANT_CHAIN_WORDS" in hpp and "SAIP_PLANT_CHAIN_MAX_DEPTH" in hpp
    # ids 0..8 are taken: the chain's table is the next free one
    assert (PL.TABLE_JOINTS, PL.TABLE_WRENCHES, SC.TABLE_CHAIN) == (0, 1, 8) and capi.SAIP_PLANT_JOINT_WORDS == 10
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    for f in ("csrc/saip_plant.hip", "csrc/saip_engine_plant.cpp"):
        assert f in capi.SOURCES
    assert "csrc/saip_plant_chain.h" in capi.HEADERS
    assert list(sp.RobotController.PLANT_CHAIN_WORDS) == WORDS
    for m in ("attachActuationChain", "detachActuationChain", "actuationChainInfo", "setActuationChainTable", "actuationChainRandomize", "resetActuationChain",
              "actuationChainState", "actuationChainStateDevice", "actuationChainTableDevice"):
        assert callable(getattr(sp.RobotController, m)) and re.search(r"\b" + m + r"\s*\(", hpp), m
    # the header includes the plant model (and through it the generator and the draw), it does not restate them; no transcendental function
    assert '#include "saip_plant.h"' in src and "philox" not in src.lower()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\b(exp|log|sin|cos|tan|pow|sqrt|atan2?|fmin|fmax)\s*\(", code)
    assert "#pragma clang fp contract(off)" in code and "pl_min(pl_max(" in code


def _others_refuse(L, b, code, info_code=None):
    v, nb, out, flags = C.c_int(7), C.c_size_t(7), np.full(7 * 4 * 4 * 16, 7.0), np.full(7 * 4, 7, np.int32)
    assert L.saip_batch_plant_chain_detach(b) == code
    assert L.saip_batch_plant_chain_info(b, C.byref(v), C.byref(v), C.byref(v), C.byref(nb)) == (code if info_code is None else info_code)
    assert L.saip_batch_plant_chain_set_table_host(b, _dp(out)) == code
    assert L.saip_batch_plant_chain_randomize(b, 1, 0, _dp(out), _dp(out)) == code
    assert L.saip_batch_plant_chain_reset(b) == code
    assert L.saip_batch_plant_chain_state_host(b, _dp(out), _dp(out), flags.ctypes.data_as(C.POINTER(C.c_int))) == code
    assert L.saip_batch_plant_chain_table_device(b) is None
    ptr = C.c_void_p(7)
    assert L.saip_batch_plant_chain_state_device(b, C.byref(ptr), C.byref(ptr), C.byref(ptr)) == code and ptr.value == 7
    assert v.value == 7 and nb.value == 7 and (out == 7.0).all() and (flags == 7).all()      # nothing was written


TABLE = np.tile([2.0, 50.0, 0.004], (7, 1))


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    att = L.saip_batch_plant_chain_attach

    def call(b, table=TABLE, per=0, depth=4):
        return att(b, None if table is None else _dp(np.ascontiguousarray(table)), per, depth)

    def refused(b, msg, **kw):
        assert call(b, **kw) == INVALID and msg in L.saip_last_error(), (kw, L.saip_last_error())

    assert call(None) == INVALID and b"null batch" in L.saip_last_error()
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert call(b) == ORDER and b"saip_batch_finalize first" in L.saip_last_error()           # before finalize, whatever the arguments
        assert call(b, depth=99) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for d in (-1, 9, 2 ** 31 - 1):
            refused(b, b"a depth of 0..8 required (got %d)" % d, depth=d)
        # one bad word of one joint, batch-uniform and per instance (there: of one instance only)
        per = np.ascontiguousarray(np.repeat(TABLE[:, :, None], B, axis=2))
        cases = [(k, k, np.nan, b"word %s is NaN" % WORDS[k].encode()) for k in range(3)]
        cases += [(6, k, s * np.inf, b"word %s is not finite" % WORDS[k].encode()) for k in (0, 2) for s in (1, -1)]
        cases += [(2, 0, 1.5, b"word delay = 1.5 is not an integer in 0..4"), (3, 0, 5.0, b"word delay = 5 is not an integer in 0..4"),
                  (0, 0, -1.0, b"word delay = -1 is not an integer in 0..4"), (1, 1, 0.0, b"word rate_max = 0 is not above 0"),
                  (5, 1, -3.0, b"word rate_max = -3 is not above 0"), (5, 1, -np.inf, b"word rate_max = -inf is not above 0"),
                  (4, 2, -1e-9, b"word tau_lag = -1e-09 is below 0")]
        for j, k, val, msg in cases:
            t1 = TABLE.copy()
            t1[j, k] = val
            refused(b, b"joint %d: " % j + msg, table=t1)
            t2 = per.copy()
            t2[j, k, B - 1] = val
            refused(b, b"joint %d of instance 3: " % j + msg, table=t2, per=1)
        refused(b, b"word delay = 2 is not an integer in 0..1", depth=1)
        # valid arguments reach the order check: a configuration-only batch has no device, so no plant model can be attached to carry a chain
        edge = TABLE.copy()
        edge[:, 0], edge[:, 1], edge[:, 2] = 4.0, np.inf, 0.0
        for kw in (dict(), dict(table=None), dict(table=None, per=1), dict(table=per, per=1), dict(table=PC.neutral(7), depth=0), dict(table=edge), dict(depth=8)):
            assert call(b, **kw) == ORDER and b"no plant model is attached" in L.saip_last_error(), kw
        assert L.saip_last_error() == b"saip_batch_plant_chain_attach: no plant model is attached (saip_batch_plant_attach; an all-neutral table is a valid carrier)"
        # several at once: the depth is checked first, then the table, then the call order
        bad = TABLE.copy()
        bad[0, 2] = -1.0
        refused(b, b"a depth of 0..8 required (got 9)", table=bad, depth=9)
        refused(b, b"joint 0: word tau_lag = -1 is below 0", table=bad)
        _others_refuse(L, b, ORDER)
        assert b"no plant model is attached" in L.saip_last_error()
    finally:
        L.saip_batch_destroy(b)


def chain_calls(L, b, stem, B=4):
    """every status entry of the chain `stem` ("plant", "sensing") behind its need-check, called with well-formed arguments:
    [(entry, status, message)]"""
    z, flags, p = np.zeros(7 * 4 * B), np.zeros(7 * B, np.int32), C.c_void_p()
    args = dict(detach=(), set_table_host=(_dp(z),), randomize=(1, 0, _dp(z), _dp(z)), reset=(),
                state_host=(_dp(z), _dp(z), flags.ctypes.data_as(C.POINTER(C.c_int))), state_device=(C.byref(p),) * 3)
    out = []
    for entry, a in args.items():
        fn = f"saip_batch_{stem}_chain_{entry}"
        out.append((fn, getattr(L, fn)(b, *a), L.saip_last_error().decode()))
    return out


def each_chain_answers_for_itself(sp, L, stems):
    """the two chains share their host code: on one batch every entry of either still names itself and its own carrier.  Without a device
    no carrier can be attached, so this is as far as the order checks go here; tests/test_gpu_plant_chain.py::test_both_chains_together
    has the "no ... chain is attached" half, with one chain attached and the other not."""
    from sai_primitives_amd import capi
    robot, b = _controller_batch(sp, L, 4)
    try:
        assert L.saip_batch_finalize(b) == 0
        for stem in stems + stems[::-1]:
            for fn, status, msg in chain_calls(L, b, stem):
                assert status == capi.SAIP_ERR_ORDER and msg == f"{fn}: no {stem} model is attached (saip_batch_{stem}_attach)", (fn, msg)
    finally:
        L.saip_batch_destroy(b)


def test_each_chain_answers_for_itself(sp):
    each_chain_answers_for_itself(sp, sp.lib(), ["plant", "sensing"])


def test_model_only_batch_refuses_the_chain(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_plant_chain_attach(b, None, 0, 0) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    ctrl = sp.RobotController(robot, [sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)])
    for bad in (np.zeros(3), np.zeros((3, 3)), np.zeros((7, B, 3))):
        with pytest.raises(ValueError, match="chain table of shape"):
            ctrl.attachActuationChain(bad, depth=2)
    with pytest.raises(ValueError, match="per-instance chain table of shape"):
        ctrl.attachActuationChain(np.zeros((7, 3)), per_instance=True, depth=2)
    with pytest.raises(ValueError, match="unknown chain table words"):
        ctrl.attachActuationChain(dict(a_q=1))
    with pytest.raises(ValueError, match="a depth of 0..8 required"):
        ctrl.attachActuationChain(depth=9)
    with pytest.raises(ValueError, match="joint 3: word delay = 3 is not an integer in 0..2"):
        ctrl.attachActuationChain(dict(delay=[0, 0, 0, 3, 0, 0, 0]), depth=2)
    with pytest.raises(ValueError, match="joint 0: word rate_max = 0 is not above 0"):
        ctrl.attachActuationChain(np.zeros((7, 3)), depth=2)                   # an all-zero array is not the neutral table
    with pytest.raises(ValueError, match="joint 6 of instance 2: word tau_lag is NaN"):
        t = np.tile(PC.neutral(7)[:, None, :], (1, B, 1))
        t[6, 2, 2] = np.nan
        ctrl.attachActuationChain(t, per_instance=True, depth=2)
    # a dict names only what differs from the neutral row: rate_max defaults to +inf
    for kw in (dict(), dict(table=dict(delay=2, tau_lag=0.003), depth=2), dict(table=dict(delay=np.ones((7, B)), rate_max=100.0), per_instance=True, depth=8)):
        with pytest.raises(sp.SaipError, match="no plant model is attached"):
            ctrl.attachActuationChain(**kw)
    z = PC.neutral(7)
    for fn in (ctrl.detachActuationChain, ctrl.actuationChainInfo, ctrl.resetActuationChain, ctrl.actuationChainState, ctrl.actuationChainStateDevice,
               lambda: ctrl.setActuationChainTable(z), lambda: ctrl.actuationChainRandomize(1, lo=z, hi=z)):
        with pytest.raises(sp.SaipError, match="no plant model is attached"):
            fn()
    assert ctrl.actuationChainTableDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "plant_chain_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("plant_chain_host"), "plant_chain_host", []),
            _build(tmp_path_factory.mktemp("plant_chain_host_san"), "plant_chain_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _run(exe, tmp, table, depth, dts, cmds, per, dseed=1, rnd=0, bounds=None):
    """table (J, 3) or (J, N, 3); dts the substeps' lengths; cmds [t (N, J)] one per period; returns out (P, S, N, J), taps (N, J, depth),
    filt (N, J, 3), primed (N, J), drawn (J, N, 3)"""
    table = np.asarray(table, float)
    N, J, P, S = cmds[0].shape[0], table.shape[0], len(cmds), len(dts)
    lo, hi = bounds if bounds is not None else (PC.neutral(J), PC.neutral(J))
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, J, depth, per, P, S], np.int32).tobytes())
        f.write(np.ascontiguousarray(table.transpose(0, 2, 1) if per else table).tobytes())
        f.write(np.asarray(dts, np.float64).tobytes())
        for t in cmds:
            f.write(np.ascontiguousarray(np.asarray(t, float).T).tobytes())
        f.write(np.array([dseed], np.uint64).tobytes())
        f.write(np.array([rnd, 0], np.uint32).tobytes())
        f.write(np.ascontiguousarray(lo, float).tobytes())
        f.write(np.ascontiguousarray(hi, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    got, at = [], 0
    for shp in [(P, S, J, N), (J, depth, N), (J, 3, N), (J, N), (J, 3, N)]:
        k = int(np.prod(shp))
        got.append(raw[at:at + k].reshape(shp))
        at += k
    assert at == raw.size
    o, taps, filt, primed, drawn = got
    return o.transpose(0, 1, 3, 2), taps.transpose(2, 0, 1), filt.transpose(2, 0, 1), primed.T.astype(np.int32), drawn.transpose(0, 2, 1)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ref(table, depth, dts, cmds):
    ch = PC.Chain(table, depth, cmds[0].shape[0])
    out = np.stack([np.stack([ch.step(t, dt, s == 0) for s, dt in enumerate(dts)]) for t in cmds])
    return out, ch


DT = 1e-3 / 3
DTS = [DT, 0.5 * DT, 1.5 * DT]                                             # unequal substeps of one period


def _table(rng, J, N, depth, per):
    """rows covering d in {0, 1, depth}, rate_max in {+inf, binding, never binding} and tau_lag in {0, dt, 10 dt}; row 0 neutral"""
    sh = (J, N) if per else (J,)
    t = np.zeros(sh + (3,))
    t[..., 0] = rng.choice(sorted({0, min(1, depth), depth}), sh)
    t[..., 1] = rng.choice([np.inf, 2e3, 1e9], sh)                         # commands are O(10): 2e3 / s binds at dt = 1/3 ms, 1e9 / s never
    t[..., 2] = rng.choice([0.0, DT, 10 * DT], sh)
    t[0] = PC.NEUTRAL
    if J > 3:
        t[1] = [depth, 2e3, 10 * DT]
        t[2] = [min(1, depth), 1e9, DT]
        t[3] = [0.0, np.inf, DT]
    return t


def _commands(rng, N, J, P=40, nonfinite=True):
    out = []
    for k in range(P):
        t = rng.uniform(-10, 10, (N, J))
        if nonfinite and k in (7, 8, 20):                                    # non-finite input: NaN is no torque, +-inf gets no special case
            t[rng.random((N, J)) < 0.05] = np.nan
            t[rng.random((N, J)) < 0.04] = np.inf
            t[rng.random((N, J)) < 0.03] = -np.inf
        out.append(t)
    return out


CASES = [(1, 67, 7, 8, 0), (2, 5, 7, 8, 1), (3, 64, 30, 3, 1), (4, 33, 2, 1, 0), (5, 9, 3, 0, 1), (6, 1, 1, 8, 0)]


@pytest.mark.parametrize("seed,N,J,depth,per", CASES)
def test_host_build_matches_the_restatement_bit_for_bit(exes, tmp_path, seed, N, J, depth, per):
    rng = np.random.default_rng(seed)
    table = _table(rng, J, N, depth, per)
    cmds = _commands(rng, N, J)
    want, ch = _ref(table, depth, DTS, cmds)
    lo, hi = np.tile([-0.4, 10.0, 0.0], (J, 1)), np.tile([depth + 0.4, 500.0, 0.01], (J, 1))
    lo[0], hi[0] = [1.0, np.inf, 0.002], [1.0, np.inf, 0.002]               # lo == hi: exact, +inf stays +inf
    drawn = PC.draw(0xABCDEF0123456789, 5, N, lo, hi, depth)
    if seed == 1:   # what the cases must cover (asserted on the first, which is large enough to hit them all)
        assert {0.0, 1.0, 8.0} <= set(table[:, 0]) and {np.inf, 2e3, 1e9} <= set(table[:, 1]) and {0.0, DT, 10 * DT} <= set(table[:, 2])
        assert np.isnan(cmds[7]).any() and np.isposinf(cmds[8]).any() and np.isneginf(cmds[20]).any()
        for k, t in enumerate(cmds):                                         # the neutral row returns the sanitised command's bits, every substep
            for s in range(3):
                assert np.array_equal(_bits(want[k, s][:, 0]), _bits(np.where(t[:, 0] == t[:, 0], t[:, 0], 0.0)))
        assert not np.isfinite(want[-1]).all()                               # what an infinite command left in a filter stays
        r, hit = PC.Chain(table, depth, N), {2e3: False, 1e9: False}          # 2e3 / s binds somewhere, 1e9 / s never
        for k, t in enumerate(cmds[:7]):
            for s, dt in enumerate(DTS):
                before = r.filt[..., PC.Y_RATE].copy()
                r.step(t, dt, s == 0)
                for rm in hit:
                    hit[rm] |= k > 0 and bool((np.abs(r.filt[..., PC.X_HELD] - before) > rm * dt)[:, table[:, 1] == rm].any())
        assert hit[2e3] and not hit[1e9]
        assert set(np.unique(drawn[1:, :, 0])) == set(range(9)) and (drawn[0] == [1.0, np.inf, 0.002]).all()
    for exe in exes:
        got, taps, filt, primed, dr = _run(exe, tmp_path, table, depth, DTS, cmds, per, 0xABCDEF0123456789, 5, (lo, hi))
        assert np.array_equal(_bits(got), _bits(want))
        assert np.array_equal(_bits(taps), _bits(ch.taps)) and np.array_equal(_bits(filt), _bits(ch.filt)) and np.array_equal(primed, ch.primed)
        assert np.array_equal(_bits(dr), _bits(drawn))
        assert ((dr[..., 0] >= 0) & (dr[..., 0] <= depth) & (dr[..., 0] == np.floor(dr[..., 0]))).all() and (dr[..., 1] >= 10.0).all()


def _both(exes, tmp_path, table, depth, dts, cmds):
    """the restatement's and the host build's outputs and final taps, asserted equal, returned once"""
    want, ch = _ref(table, depth, dts, cmds)
    got, taps = _run(exes[0], tmp_path, table, depth, dts, cmds, 0)[:2]
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(taps), _bits(ch.taps))
    return want, ch.taps


def test_the_neutral_row_returns_the_sanitised_command(exes, tmp_path):
    t = np.array([[0.0, -0.0, 1.5, -7.25e300, 5e-324, np.nan, np.inf, -np.inf]])
    for depth in (0, 8):
        out, _ = _both(exes, tmp_path, PC.neutral(t.shape[1]), depth, DTS, [t, t[:, ::-1].copy()])
        for k, c in enumerate((t, t[:, ::-1])):
            for s in range(3):
                assert np.array_equal(_bits(out[k, s]), _bits(np.where(c == c, c, 0.0)))      # -0 stays -0, NaN becomes +0


def test_a_pure_delay_returns_the_command_of_d_periods_earlier(exes, tmp_path):
    rng = np.random.default_rng(11)
    N, depth, P = 3, 8, 20
    table = PC.neutral(depth + 1)
    table[:, 0] = np.arange(depth + 1)                                       # joint j delays by j periods
    cmds = _commands(rng, N, depth + 1, P, nonfinite=False)
    out, _ = _both(exes, tmp_path, table, depth, DTS, cmds)
    for p in range(P):
        for d in range(depth + 1):
            src = max(p - d, 0)                                              # before that, the first command
            for s in range(3):                                               # held over all substeps
                assert np.array_equal(_bits(out[p, s][:, d]), _bits(cmds[src][:, d]))


def test_a_rate_limited_step_climbs_by_exact_increments(exes, tmp_path):
    """a step 0 -> T with rate_max dt exactly representable (dt = 2^-10, rate_max a small multiple of a power of two): after k substeps
    the output is min(k rate_max dt, T) exactly, whichever substep of a period it is"""
    dt, P, S = 2.0 ** -10, 12, 3
    rate = np.array([1024.0, 3 * 256.0, 5 * 64.0, 1e9 * 1024])
    T = np.array([7.5, 7.5, -3.0, 2.0])
    table = PC.neutral(4)
    table[:, 1] = rate
    cmds = [np.zeros((1, 4))] + [T[None, :].copy()] * P                      # the first period primes at 0
    out, _ = _both(exes, tmp_path, table, 0, [dt] * S, cmds)
    assert (out[0] == 0).all()
    for p in range(P):
        for s in range(S):
            k = p * S + s + 1
            want = np.sign(T) * np.minimum(k * rate * dt, np.abs(T))
            assert np.array_equal(out[p + 1, s][0], want), (p, s)


def test_the_step_response_of_the_lag(exes, tmp_path):
    """y_k = 1 - (tau / (tau + dt))^k for a unit step after a first period at 0 (which primes the filter at 0), within k ulp of 1.  Each of
    the k updates y + a (1 - y) rounds three times on values below 1 (a quarter ulp of 1 each at most), and the error of earlier steps is
    damped by 1 - a: at most 0.75 k ulp.  a = dt / (tau + dt) is rounded twice, a relative error of an ulp, which moves (1 - a)^k by
    k a (1 - a)^(k-1) ulp, below 0.7 ulp for every k.  The first update is exact but for a."""
    dt, P, S = 1e-3 / 3, 10, 3
    tau = np.array([dt, 10 * dt, 0.5 * dt, 0.02])
    table = PC.neutral(len(tau))
    table[:, 2] = tau
    cmds = [np.zeros((1, len(tau)))] + [np.ones((1, len(tau)))] * P
    out, _ = _both(exes, tmp_path, table, 0, [dt] * S, cmds)
    ulp = np.spacing(1.0)
    assert (out[0] == 0).all()
    for p in range(P):
        for s in range(S):
            k = p * S + s + 1
            want = np.array([float(1 - (Fraction(float(x)) / (Fraction(float(x)) + Fraction(dt))) ** k) for x in tau])      # exact in rationals, rounded once
            assert (np.abs(out[p + 1, s][0] - want) <= k * ulp).all(), k


def test_substeps_without_advance_never_touch_a_tap(exes, tmp_path):
    """the taps after P periods are the same bits whether a period has one substep or three, and in the restatement a substep with
    advance = 0 leaves them alone even when nothing is primed"""
    rng = np.random.default_rng(5)
    N, J, depth = 4, 5, 8
    table = _table(rng, J, N, depth, 0)
    table[:, 0] = [0, 1, 3, 8, 8]
    cmds = _commands(rng, N, J, 12)
    _, taps1 = _both(exes, tmp_path, table, depth, DTS[:1], cmds)
    _, taps3 = _both(exes, tmp_path, table, depth, DTS, cmds)
    assert np.array_equal(_bits(taps1), _bits(taps3))
    ch = PC.Chain(table, depth, N)
    ch.taps[:] = 7.0
    ch.step(cmds[0], DT, False)
    assert (ch.taps == 7.0).all() and (ch.primed == 0).all()
    ch.step(cmds[0], DT, True)
    mark = ch.taps.copy()
    ch.step(cmds[1], DT, False)
    assert np.array_equal(_bits(ch.taps), _bits(mark))
