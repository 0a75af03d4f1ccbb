"""The sensing chain of the resident simulator, host side (no GPU needed): the C-ABI entries are declared, exported and bound and the
constants agree everywhere; the argument and call-order errors come back with the documented codes before the device is needed and write
nothing; the Python facade raises the same; the host build of csrc/saip_sense_chain.h (tests/cpp/sensing_chain_host.cpp, also under
ASan/UBSan) matches the NumPy restatement tests/sensing_chain_ref.py bit for bit; and both pass analytic checks: a pure delay, the step
response of the low-pass, the finite difference of a ramp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sensing_chain_ref as SC
from test_sensing_cpu import _controller_batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_sensing_chain_attach", "saip_batch_sensing_chain_detach", "saip_batch_sensing_chain_info", "saip_batch_sensing_chain_set_table_host",
                  "saip_batch_sensing_chain_randomize", "saip_batch_sensing_chain_reset", "saip_batch_sensing_chain_state_host",
                  "saip_batch_sensing_chain_state_device"]
POINTER_ENTRIES = ["saip_batch_sensing_chain_table_device"]
WORDS = ["delay", "vel_mode", "a_q", "a_dq"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    import sensing_ref as SE
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    src = open(os.path.join(PKG, "csrc", "saip_sense_chain.h")).read()
    for name, val, ref, srcname in [("CHAIN_WORDS", 4, SC.WORDS, "SENSE_CHAIN_WORDS"), ("CHAIN_MAX_DEPTH", 8, SC.MAX_DEPTH, "SENSE_CHAIN_MAX_DEPTH"),
                                    ("TABLE_CHAIN", 8, SC.TABLE_CHAIN, "SENSE_TABLE_CHAIN")]:
        assert re.search(rf"#define SAIP_SENSE_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_SENSE_" + name) == val == ref
        assert re.search(rf"\b{srcname} = {val}\b", src), name
    # ids 0..7 are taken: the chain's table is the next free one; the sensing model's words stay six
    assert sorted([SE.TABLE_JOINTS, SE.TABLE_WRENCHES, SE.TABLE_JOINT_NOISE, SE.TABLE_WRENCH_NOISE]) == [4, 5, 6, 7] and capi.SAIP_SENSE_JOINT_WORDS == 6
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    for f in ("csrc/saip_sense_chain.hip", "csrc/saip_engine_sensing.cpp"):
        assert f in capi.SOURCES
    assert "csrc/saip_sense_chain.h" in capi.HEADERS
    assert list(sp.RobotController.SENSE_CHAIN_WORDS) == WORDS
    # the header includes the sensing model (and through it the generator and the draw), it does not restate them; no transcendental function
    assert '#include "saip_sense.h"' in src and "philox" not in src.lower()
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\b(exp|log|sin|cos|tan|pow|sqrt|atan2?)\s*\(", code)
    assert "#pragma clang fp contract(off)" in code
    assert sp.RobotController.sensingChainAlpha(50.0, 1e-3) == 1.0 - np.exp(-2.0 * np.pi * 50.0 * 1e-3) == SC.alpha(50.0, 1e-3)


def _others_refuse(L, b, code, info_code=None):
    v, T, nb, out, flags = C.c_int(7), C.c_double(7.0), C.c_size_t(7), np.full(7 * 4 * 4 * 16, 7.0), np.full(7 * 4, 7, np.int32)
    assert L.saip_batch_sensing_chain_detach(b) == code
    assert L.saip_batch_sensing_chain_info(b, C.byref(v), C.byref(v), C.byref(v), C.byref(T), C.byref(nb)) == (code if info_code is None else info_code)
    assert L.saip_batch_sensing_chain_set_table_host(b, _dp(out)) == code
    assert L.saip_batch_sensing_chain_randomize(b, 1, 0, _dp(out), _dp(out)) == code
    assert L.saip_batch_sensing_chain_reset(b) == code
    assert L.saip_batch_sensing_chain_state_host(b, _dp(out), _dp(out), flags.ctypes.data_as(C.POINTER(C.c_int))) == code
    assert L.saip_batch_sensing_chain_table_device(b) is None
    ptr = C.c_void_p(7)
    assert L.saip_batch_sensing_chain_state_device(b, C.byref(ptr), C.byref(ptr), C.byref(ptr)) == code and ptr.value == 7
    assert v.value == 7 and T.value == 7.0 and nb.value == 7 and (out == 7.0).all() and (flags == 7).all()      # nothing was written


TABLE = np.tile([2.0, 1.0, 0.25, 0.5], (7, 1))


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    att = L.saip_batch_sensing_chain_attach

    def call(b, table=TABLE, per=0, depth=4, T=1e-3):
        return att(b, None if table is None else _dp(np.ascontiguousarray(table)), per, depth, T)

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
        for T in (0.0, -1e-3, np.inf, np.nan):
            refused(b, b"a finite sample time > 0 required", T=T)
        # one bad word of one joint, batch-uniform and per instance (there: of one instance only)
        per = np.ascontiguousarray(np.repeat(TABLE[:, :, None], B, axis=2))
        cases = [(k, k, np.nan, b"word %s is NaN" % WORDS[k].encode()) for k in range(4)]
        cases += [(6, k, s * np.inf, b"word %s is not finite" % WORDS[k].encode()) for k in range(4) for s in (1, -1)]
        cases += [(2, 0, 1.5, b"word delay = 1.5 is not an integer in 0..4"), (3, 0, 5.0, b"word delay = 5 is not an integer in 0..4"),
                  (0, 0, -1.0, b"word delay = -1 is not an integer in 0..4"), (1, 1, 2.0, b"word vel_mode = 2 is neither 0 nor 1"),
                  (5, 1, 0.5, b"word vel_mode = 0.5 is neither 0 nor 1"), (4, 2, -1e-9, b"word a_q = -1e-09 is outside [0, 1]"),
                  (4, 3, 1.5, b"word a_dq = 1.5 is outside [0, 1]"), (6, 2, 1.0000001, b"word a_q = 1 is outside [0, 1]")]
        for j, k, val, msg in cases:
            t1 = TABLE.copy()
            t1[j, k] = val
            refused(b, b"joint %d: " % j + msg, table=t1)
            t2 = per.copy()
            t2[j, k, B - 1] = val
            refused(b, b"joint %d of instance 3: " % j + msg, table=t2, per=1)
        refused(b, b"word delay = 2 is not an integer in 0..1", depth=1)
        # valid arguments reach the order check: a configuration-only batch has no device, so no sensing model can be attached to carry a chain
        edge = TABLE.copy()
        edge[:, 0], edge[:, 2], edge[:, 3] = 4.0, 1.0, 0.0
        for kw in (dict(), dict(table=None), dict(table=None, per=1), dict(table=per, per=1), dict(table=np.zeros((7, 4)), depth=0), dict(table=edge), dict(depth=8),
                   dict(T=1e-300)):
            assert call(b, **kw) == ORDER and b"no sensing model is attached" in L.saip_last_error(), kw
        assert L.saip_last_error() == b"saip_batch_sensing_chain_attach: no sensing model is attached (saip_batch_sensing_attach; an all-zero table is a valid carrier)"
        # several at once: the depth is checked first, then the sample time, then the table, then the call order
        bad = TABLE.copy()
        bad[0, 2] = 2.0
        refused(b, b"a depth of 0..8 required (got 9)", table=bad, depth=9, T=0.0)
        refused(b, b"a finite sample time > 0 required (got 0)", table=bad, T=0.0)
        refused(b, b"joint 0: word a_q = 2 is outside [0, 1]", table=bad)
        _others_refuse(L, b, ORDER)
        assert b"no sensing model is attached" in L.saip_last_error()
    finally:
        L.saip_batch_destroy(b)


def test_each_chain_answers_for_itself(sp):
    from test_plant_chain_cpu import each_chain_answers_for_itself
    each_chain_answers_for_itself(sp, sp.lib(), ["sensing", "plant"])


def test_model_only_batch_refuses_the_chain(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_sensing_chain_attach(b, None, 0, 0, 1e-3) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    ctrl = sp.RobotController(robot, [sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)])
    for bad in (np.zeros(4), np.zeros((4, 4)), np.zeros((7, B, 4))):
        with pytest.raises(ValueError, match="chain table of shape"):
            ctrl.attachSensingChain(bad, depth=2)
    with pytest.raises(ValueError, match="per-instance chain table of shape"):
        ctrl.attachSensingChain(np.zeros((7, 4)), per_instance=True, depth=2)
    with pytest.raises(ValueError, match="unknown chain table words"):
        ctrl.attachSensingChain(dict(lag=1))
    with pytest.raises(ValueError, match="a depth of 0..8 required"):
        ctrl.attachSensingChain(depth=9)
    with pytest.raises(ValueError, match="a finite sample time > 0 required"):
        ctrl.attachSensingChain(depth=1, sample_time=0.0)
    with pytest.raises(ValueError, match="joint 3: word delay = 3 is not an integer in 0..2"):
        ctrl.attachSensingChain(dict(delay=[0, 0, 0, 3, 0, 0, 0]), depth=2)
    with pytest.raises(ValueError, match="joint 6 of instance 2: word a_dq is NaN"):
        t = np.zeros((7, B, 4))
        t[6, 2, 3] = np.nan
        ctrl.attachSensingChain(t, per_instance=True, depth=2)
    for kw in (dict(), dict(table=dict(delay=2, vel_mode=1, a_dq=0.3), depth=2), dict(table=dict(delay=np.ones((7, B))), per_instance=True, depth=8)):
        with pytest.raises(sp.SaipError, match="no sensing model is attached"):
            ctrl.attachSensingChain(**kw)
    z = np.zeros((7, 4))
    for fn in (ctrl.detachSensingChain, ctrl.sensingChainInfo, ctrl.resetSensingChain, ctrl.sensingChainState, lambda: ctrl.setSensingChainTable(z),
               lambda: ctrl.sensingChainRandomize(1, lo=z, hi=z)):
        with pytest.raises(sp.SaipError, match="no sensing model is attached"):
            fn()
    assert ctrl.sensingChainTableDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "sensing_chain_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("sensing_chain_host"), "sensing_chain_host", []),
            _build(tmp_path_factory.mktemp("sensing_chain_host_san"), "sensing_chain_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _run(exe, tmp, table, depth, T, samples, per, dseed=1, rnd=0, bounds=None):
    """table (J, 4) or (J, N, 4); samples [(q_m (N, J), dq_m)]; returns q, dq (P, N, J), taps (N, J, 2, depth), filt (N, J, 3), primed (N, J), drawn (J, N, 4)"""
    table = np.asarray(table, float)
    N, J, P = samples[0][0].shape[0], table.shape[0], len(samples)
    lo, hi = bounds if bounds is not None else (np.zeros((J, 4)), np.zeros((J, 4)))
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, J, depth, per, P, 0], np.int32).tobytes())
        f.write(np.array([T], np.float64).tobytes())
        f.write(np.ascontiguousarray(table.transpose(0, 2, 1) if per else table).tobytes())
        for q, dq in samples:
            f.write(np.ascontiguousarray(np.asarray(q, float).T).tobytes())
            f.write(np.ascontiguousarray(np.asarray(dq, float).T).tobytes())
        f.write(np.array([dseed], np.uint64).tobytes())
        f.write(np.array([rnd, 0], np.uint32).tobytes())
        f.write(np.ascontiguousarray(lo, float).tobytes())
        f.write(np.ascontiguousarray(hi, float).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    got, at = [], 0
    for shp in [(P, 2, J, N), (J, 2, depth, N), (J, 3, N), (J, N), (J, 4, N)]:
        k = int(np.prod(shp))
        got.append(raw[at:at + k].reshape(shp))
        at += k
    assert at == raw.size
    meas, taps, filt, primed, drawn = got
    return (meas[:, 0].transpose(0, 2, 1), meas[:, 1].transpose(0, 2, 1), taps.transpose(3, 0, 1, 2), filt.transpose(2, 0, 1), primed.T.astype(np.int32),
            drawn.transpose(0, 2, 1))


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _ref(table, depth, T, samples):
    N = samples[0][0].shape[0]
    ch = SC.Chain(table, depth, T, N)
    out = [ch.step(q, dq) for q, dq in samples]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), ch


def _table(rng, J, N, depth, per):
    """rows covering d = 0, 1, depth, both velocity modes and a in {0, 1, 0.25}; row 0 neutral"""
    sh = (J, N) if per else (J,)
    t = np.zeros(sh + (4,))
    t[..., 0] = rng.choice(sorted({0, min(1, depth), depth}), sh)
    t[..., 1] = rng.choice([0.0, 1.0], sh)
    t[..., 2], t[..., 3] = rng.choice([0.0, 1.0, 0.25], sh), rng.choice([0.0, 1.0, 0.25], sh)
    t[0] = 0.0
    if J > 3:
        t[1] = [depth, 1.0, 0.25, 0.25]
        t[2] = [min(1, depth), 0.0, 1.0, 0.0]
        t[3] = [0.0, 1.0, 0.0, 1.0]
    return t


def _samples(rng, N, J, P=40, nonfinite=True):
    out = []
    for k in range(P):
        q, dq = rng.uniform(-2.5, 2.5, (N, J)), rng.uniform(-1, 1, (N, J))
        if nonfinite and k in (7, 8, 20):                                # non-finite input: no special case anywhere
            q[rng.random((N, J)) < 0.05] = np.nan
            dq[rng.random((N, J)) < 0.05] = np.inf
            q[rng.random((N, J)) < 0.03] = -np.inf
        out.append((q, dq))
    return out


CASES = [(1, 67, 7, 8, 0), (2, 5, 7, 8, 1), (3, 64, 30, 3, 1), (4, 33, 2, 1, 0), (5, 9, 3, 0, 1), (6, 1, 1, 8, 0)]


@pytest.mark.parametrize("seed,N,J,depth,per", CASES)
def test_host_build_matches_the_restatement_bit_for_bit(exes, tmp_path, seed, N, J, depth, per):
    rng = np.random.default_rng(seed)
    table, T = _table(rng, J, N, depth, per), 1e-3
    samples = _samples(rng, N, J)
    wq, wdq, ch = _ref(table, depth, T, samples)
    lo, hi = np.tile([-0.4, -0.4, 0.0, 0.1], (J, 1)), np.tile([depth + 0.4, 1.4, 1.0, 0.1], (J, 1))
    lo[0], hi[0] = [1.0, 1.0, 0.3, 0.2], [1.0, 1.0, 0.3, 0.2]          # lo == hi: exact
    drawn = SC.draw(0xABCDEF0123456789, 5, N, lo, hi, depth)
    if seed == 1:   # what the cases must cover (asserted on the first, which is large enough to hit them all)
        assert {0.0, 1.0, 8.0} <= set(table[:, 0]) and {0.0, 1.0} <= set(table[:, 1]) and {0.0, 1.0, 0.25} <= set(table[:, 2]) | set(table[:, 3])
        assert np.isnan(samples[7][0]).any() and np.isposinf(samples[8][1]).any() and np.isneginf(samples[20][0]).any()
        for k, (q, dq) in enumerate(samples):                            # the neutral row returns its input bits
            assert np.array_equal(_bits(wq[k][:, 0]), _bits(q[:, 0])) and np.array_equal(_bits(wdq[k][:, 0]), _bits(dq[:, 0]))
        assert np.isnan(wq[-1]).any()                                    # a NaN that entered a filter stays
        d = drawn[1:, :, 0]
        assert set(np.unique(d)) == set(range(9)) and set(np.unique(drawn[1:, :, 1])) == {0.0, 1.0}
        assert (drawn[0] == [1.0, 1.0, 0.3, 0.2]).all()
    for exe in exes:
        q, dq, taps, filt, primed, dr = _run(exe, tmp_path, table, depth, T, samples, per, 0xABCDEF0123456789, 5, (lo, hi))
        assert np.array_equal(_bits(q), _bits(wq)) and np.array_equal(_bits(dq), _bits(wdq))
        assert np.array_equal(_bits(taps), _bits(ch.taps)) and np.array_equal(_bits(filt), _bits(ch.filt)) and np.array_equal(primed, ch.primed)
        assert np.array_equal(_bits(dr), _bits(drawn))
        assert ((dr[..., 0] >= 0) & (dr[..., 0] <= depth) & (dr[..., 0] == np.floor(dr[..., 0]))).all() and np.isin(dr[..., 1], (0.0, 1.0)).all()


def _both(exes, tmp_path, table, depth, T, samples):
    """the restatement's and the host build's outputs, asserted equal, returned once"""
    wq, wdq, _ = _ref(table, depth, T, samples)
    q, dq = _run(exes[0], tmp_path, table, depth, T, samples, 0)[:2]
    assert np.array_equal(_bits(q), _bits(wq)) and np.array_equal(_bits(dq), _bits(wdq))
    return wq, wdq


def test_a_pure_delay_returns_the_input_of_d_samples_earlier(exes, tmp_path):
    rng = np.random.default_rng(11)
    N, depth, P = 3, 8, 20
    table = np.zeros((depth + 1, 4))
    table[:, 0] = np.arange(depth + 1)                                   # joint j delays by j samples
    samples = _samples(rng, N, depth + 1, P, nonfinite=False)
    q, dq = _both(exes, tmp_path, table, depth, 1e-3, samples)
    for p in range(P):
        for d in range(depth + 1):
            src = max(p - d, 0)                                          # before that, the first sample
            assert np.array_equal(_bits(q[p][:, d]), _bits(samples[src][0][:, d])) and np.array_equal(_bits(dq[p][:, d]), _bits(samples[src][1][:, d]))


def test_the_step_response_of_the_low_pass(exes, tmp_path):
    """y_k = 1 - (1 - a)^k for a unit step after a first sample of 0 (which primes the filter at 0), within k ulp of 1: each of the k updates
    y + a (1 - y) rounds three times on values below 1, and the error of earlier steps is damped by (1 - a)"""
    P = 30
    a = np.array([0.25, 0.5, 0.1, 0.9, SC.alpha(50.0, 1e-3)])
    table = np.zeros((len(a), 4))
    table[:, 2], table[:, 3] = a, a
    samples = [(np.zeros((1, len(a))), np.zeros((1, len(a))))] + [(np.ones((1, len(a))), np.ones((1, len(a))))] * P
    q, dq = _both(exes, tmp_path, table, 0, 1e-3, samples)
    ulp = np.spacing(1.0)
    from fractions import Fraction
    for k in range(P + 1):
        want = np.array([float(1 - (1 - Fraction(float(x))) ** k) for x in a])          # exact in rationals, rounded once
        assert (np.abs(q[k][0] - want) <= k * ulp).all() and np.array_equal(_bits(q[k]), _bits(dq[k])), k


def test_the_finite_difference_of_a_ramp_is_exact(exes, tmp_path):
    """q_k = c k T with c T exactly representable (T = 2^-10, c a small multiple of 2^-6): every difference is c T exactly and the quotient
    by T (a power of two) is c exactly; the first sample gives 0; with a delay the ramp starts d samples late"""
    T, P = 2.0 ** -10, 24
    c = np.array([3.0, -0.75, 1.25 * 2 ** -3, 17.0])
    table = np.zeros((4, 4))
    table[:, 1] = 1.0
    table[:, 0] = [0, 0, 2, 5]
    samples = [((c * k * T)[None, :], np.full((1, 4), 99.0)) for k in range(P)]
    q, dq = _both(exes, tmp_path, table, 5, T, samples)
    for k in range(P):
        for j, d in enumerate([0, 0, 2, 5]):
            assert dq[k][0, j] == (c[j] if k - d >= 1 else 0.0), (k, j)
            assert q[k][0, j] == c[j] * max(k - d, 0) * T
