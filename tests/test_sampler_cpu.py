"""Resident rollout sampler, everything that needs no GPU: the per-element code of the kernels (csrc/saip_sampler.h) compiled for the host
as a stand-alone program (tests/cpp/sampler_host.cpp) against the NumPy restatement tests/sampler_ref.py -- Philox known answers, uniforms,
perturb / cost / update / shift over small arrays -- the same program under AddressSanitizer and UBSan, and the C-ABI and facade contract.

The bounds.  Program and restatement run the same operations in the same order (nothing is contracted), so they differ only by their
maths libraries.  u = 2^-53, an ulp of a value below 1 is <= 2u = 2.2e-16; every library function is taken to be within 2 ulp of the exact
result, so two libraries differ by <= 4 ulp; sqrt is correctly rounded on both sides.
  normals  z = r cos(a), r = sqrt(-2 ln u1), a = 2 pi u2.  u1, u2 and a have the same bits on both sides.  -2 ln u1 <= 2 * 53.7 ln 2 = 74.4
           differs by <= 4 ulp = 4.4e-16 relative, r <= 8.63 by half of that plus the rounding of sqrt = 3.3e-16 relative = 2.9e-15;
           cos(a), sin(a) by <= 4 ulp(1) = 4.4e-16; z by <= 8.63 * 4.4e-16 + 2.9e-15 + one rounding of |z| <= 8.63 (9.6e-16) < 8e-15.
  linear rows  nominal + sigma z: sigma * 8e-15, plus one rounding each of the product and the sum, 2.2e-16 max|row|.
  rotation rows  v = sigma o z differs by dv <= sigma (8e-15 + 1.1e-16 * 8.63) <= 9e-15 sigma.  ang = |v| by <= sqrt(3) dv; sin(ang) k_e
           = (sin(ang) / ang) v_e by <= dv + sqrt(3) dv + 1e-15 |v|; (1 - cos(ang)) k_a k_b (1 - cos <= ang^2 / 2, k = v / ang) by <=
           ang dv + 4.4e-16 + 2 dv; an entry of Exp by <= 6 dv + 2e-15 for ang <= 1, an entry of R_nom Exp (a row of R_nom has 1-norm
           <= sqrt(3), three roundings) by <= 11 dv + 4e-15.
  weighted means  sum w_i x_i / sum w_i, lane l adding instances l, l + 256, ... and a tree of depth 8 over the lanes: a path to the
           root has depth = ceil(B / 256) + 8 additions and one product, so numerator and denominator carry <= (depth + 1) u and depth u
           relative to sum w max|x| and sum w, the quotient one more u.  Both sides make the same roundings, but their weights differ by
           exp's 4 ulp = 4.4e-16 relative, which moves numerator and denominator by that much each.  Relative to max|x_i|:
           (2 depth + 3) u + 8.8e-16.  The rotation mean is taken over Log coordinates, each <= pi and different by atan2's 4 ulp(pi) =
           1.8e-15 plus 2e-15 of the roundings in front of it; its Exp then follows the rotation-row bound with dv = that difference."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sampler_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
NORMAL_DERIVED = 8e-15
SENTINEL = 6.02214076e23


def linear_bound(sigma_max, row_max):
    return sigma_max * NORMAL_DERIVED + 2 * 2 * U * row_max


def rotation_bound(dv):
    return 11 * dv + 4e-15


def perturbed_rotation_bound(sigma_max):
    return rotation_bound(9e-15 * sigma_max)


def mean_bound(B, x_max):
    depth = -(-B // SR.LANES) + 8
    return ((2 * depth + 3) * U + 8.8e-16) * x_max


def rotation_mean_bound(B, log_max):
    return rotation_bound(mean_bound(B, log_max) + 1.8e-15 + 2e-15)


KNOWN = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "sampler_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sampler_host"), "sampler_host", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("sampler_host_san"), "sampler_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _run(exe, *args):
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


# ------------------------------------------------------------------ random numbers
def test_philox_known_answers(exe):
    assert _run(exe, "philox").split("\n")[:3] == [k[2] for k in KNOWN]
    for ctr, key, words in KNOWN:
        w = SR.philox4x32_10(np.array(ctr, np.uint64), key)
        assert " ".join(f"{int(x):08x}" for x in w) == words


def test_uniforms_bit_for_bit(exe):
    for seed, rnd, task, i, k, p in [(0, 0, 0, 0, 0, 0), (0x123456789abcdef0, 7, 1, 69, 2, 3), (2**64 - 1, 2**32 - 1, 7, 299, 15, 14), (42, 1, 0, 4095, 0, 1)]:
        got = _run(exe, "uniforms", seed, rnd, task, i, k, p).split()
        w = SR.philox4x32_10(SR.counters(task, np.array(i), k, p, rnd), (seed & 0xFFFFFFFF, seed >> 32))
        u = SR.uniforms(seed, rnd, task, np.array(i), k, p)
        assert got[:4] == [f"{int(x):08x}" for x in w]
        assert got[4:] == [f"{struct.unpack('<Q', struct.pack('<d', float(x)))[0]:016x}" for x in u]
        assert all(0.0 < float(x) <= 1.0 for x in u)
    # the largest and the smallest words: (0, 1] without an overflow of the integer part
    top, zero = np.uint64(0xFFFFFFFF), np.uint64(0)
    assert SR.uniform(top, top) == 1.0 and SR.uniform(zero, zero) == 2.0 ** -54


# ------------------------------------------------------------------ perturb, cost, update, shift against the restatement
def _rot(rng, angle):
    import goal_schedule_ref as GS
    axis = rng.normal(size=3)
    return GS.exp_so3(axis / np.linalg.norm(axis) * angle)


def _case(B, count, seed=5):
    """inputs of one pass of the host program: count = 3 (position rows) or 12 (position + rotation)"""
    rng = np.random.default_rng(1000 * B + count + seed)
    K, ld = 3, -(-B // 32) * 32 + 32
    r_rot = 3 if count == 12 else None
    d = SR.dim(count, r_rot)
    nominal = rng.uniform(-0.5, 0.5, (K, count))
    if r_rot is not None:
        for k in range(K):
            nominal[k, 3:] = _rot(rng, 0.4 * (k + 1)).reshape(9)
    cap, rows, pose0, n_samples, first = 4, 19, 7, 4, 2
    costs = rng.uniform(1.0, 3.0, B)
    costs[[5, 17]] = np.nan, np.inf
    return dict(B=B, ld=ld, K=K, count=count, r_rot=r_rot, d=d, task=1, exempt=2, rnd=3, seed=0x5eed0000beef + B, nominal=nominal,
                sigma=rng.uniform(0.01, 0.1, d), summary=rng.uniform(0.0, 2.0, (8, ld)), log=rng.uniform(-1.0, 1.0, (cap, rows, ld)), cap=cap,
                rows=rows, pose0=pose0, n_samples=n_samples, first=first, w=np.array([0.5, 0.0, 2.0, 0.0, 0.0, 1e-3, 0.0, 10.0]),
                target=np.array([0.3, -0.1, 0.2]), w_path=0.7, w_final=3.0, temperature=0.25, costs=costs, shift=1)


def _pass(exe, c, tmp):
    """run the host program on case c: dict of its outputs"""
    B, ld, K, count = c["B"], c["ld"], c["K"], c["count"]
    head = np.array([B, ld, K, count, int(c["r_rot"] is not None), c["r_rot"] if c["r_rot"] is not None else count, c["task"], c["exempt"], c["rnd"], c["cap"],
                     c["first"], c["n_samples"], c["rows"], c["pose0"], 1, 1], np.int32)
    blob = head.tobytes() + struct.pack("<Qd", c["seed"], c["temperature"]) + c["w"].tobytes() + c["target"].tobytes() + struct.pack("<ddii", c["w_path"], c["w_final"], c["shift"], 0)
    blob += b"".join(np.ascontiguousarray(c[k], np.float64).tobytes() for k in ("nominal", "sigma", "summary", "log", "costs"))
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(blob)
    _run(exe, "run", fin, fout)
    out = np.frombuffer(fout.read_bytes(), np.float64)
    sizes = [("keys", K * count * ld), ("cost", ld), ("w", ld), ("map", ld), ("result", 5), ("updated", K * count), ("shifted", K * count)]
    assert out.size == sum(n for _, n in sizes)
    got, at = {}, 0
    for name, n in sizes:
        got[name] = out[at:at + n]
        at += n
    got["keys"] = got["keys"].reshape(K, count, ld)
    got["updated"], got["shifted"] = got["updated"].reshape(K, count), got["shifted"].reshape(K, count)
    return got


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _check_against_restatement(got, c):
    B, ld, K, count, r_rot = c["B"], c["ld"], c["K"], c["count"], c["r_rot"]
    rows, _ = SR.coords(count, r_rot)
    ref = SR.perturb(c["nominal"], c["sigma"], c["seed"], c["rnd"], c["task"], B, c["exempt"], r_rot)
    keys = got["keys"][:, :, :B].transpose(0, 2, 1)
    # exempt columns and the padding: bit for bit
    assert np.array_equal(_bits(keys[:, :c["exempt"]]), _bits(np.broadcast_to(c["nominal"][:, None], (K, c["exempt"], count))))
    assert (got["keys"][:, :, B:] == SENTINEL).all() and (got["cost"][B:] == SENTINEL).all() and (got["w"][B:] == SENTINEL).all()
    sig = c["sigma"].max()
    worst_lin = np.abs(keys[:, :, rows] - ref[:, :, rows]).max()
    assert worst_lin <= linear_bound(sig, np.abs(ref).max())
    assert np.abs(keys[:, c["exempt"]:, rows] - c["nominal"][:, None, rows]).max() > 1e-3        # ... and they were perturbed
    if r_rot is not None:
        assert np.abs(keys[:, :, 3:] - ref[:, :, 3:]).max() <= perturbed_rotation_bound(sig)
        R = keys[:, :, 3:].reshape(K, B, 3, 3)
        assert np.abs(R.transpose(0, 1, 3, 2) @ R - np.eye(3)).max() <= 1e-12
    # cost: bit for bit (slot order first, first + 1, ... around the ring)
    order = [(c["first"] + s) % c["cap"] for s in range(c["n_samples"])]
    pos = c["log"][order][:, c["pose0"]:c["pose0"] + 3, :B].transpose(0, 2, 1)
    want = SR.cost(B, c["summary"][:, :B], c["w"], pos, c["target"], c["w_path"], c["w_final"])
    assert np.array_equal(_bits(got["cost"][:B]), _bits(want))
    # weights and result
    w, res = SR.weights(c["costs"], c["temperature"])
    assert (got["result"][0], got["result"][1]) == (res["best"], res["n_valid"]) and got["result"][2] == res["min_cost"]
    assert (got["map"][:B] == res["best"]).all() and (got["map"][B:] == SENTINEL).all()
    assert np.abs(got["w"][:B] - w).max() <= 4 * 2 * U and got["w"][5] == 0.0 and got["w"][17] == 0.0
    assert abs(got["result"][3] - res["sum_w"]) <= mean_bound(B, 1.0) * res["sum_w"]
    assert abs(got["result"][4] - res["ess"]) <= 4 * mean_bound(B, 1.0) * res["ess"]
    # update: the program's own perturbed keyframes through the restatement
    new = SR.update(c["nominal"], keys, w, res["best"], r_rot)
    assert np.abs(got["updated"][:, rows] - new[:, rows]).max() <= mean_bound(B, np.abs(keys[:, :, rows]).max())
    if r_rot is not None:
        lg = np.abs(SR.log_so3(c["nominal"][:, None, 3:].reshape(K, 1, 3, 3), keys[:, :, 3:].reshape(K, B, 3, 3))).max()
        assert np.abs(got["updated"][:, 3:] - new[:, 3:]).max() <= rotation_mean_bound(B, lg)
        assert not np.array_equal(got["updated"][:, 3:], c["nominal"][:, 3:])
    assert np.array_equal(_bits(got["shifted"]), _bits(SR.shift(got["updated"], c["shift"])))


@pytest.mark.parametrize("B", [70, 300])
@pytest.mark.parametrize("count", [3, 12])
def test_host_build_matches_the_restatement(exe, tmp_path, B, count):
    c = _case(B, count)
    _check_against_restatement(_pass(exe, c, tmp_path), c)


def test_host_build_special_costs(exe, tmp_path):
    """one-hot temperature, a tie, and no finite cost at all"""
    c = _case(70, 12)
    c["temperature"] = 1e-300
    c["costs"][[40, 11]] = 0.5                     # two equal minima: the lower index is the best
    got = _pass(exe, c, tmp_path)
    assert got["result"][0] == 11 and got["result"][1] == 68 and got["result"][3] == 2.0 and got["result"][4] == 2.0
    c["costs"][40] = 0.75                          # one minimum: all the weight on it, the nominal is its keyframes bit for bit
    got = _pass(exe, c, tmp_path)
    assert got["result"][0] == 11 and got["result"][3] == 1.0 and got["result"][4] == 1.0
    assert np.array_equal(_bits(got["updated"]), _bits(got["keys"][:, :, 11]))
    c["costs"][:] = np.nan
    c["costs"][3] = -np.inf
    got = _pass(exe, c, tmp_path)
    assert list(got["result"]) == [-1.0, 0.0, 0.0, 0.0, 0.0] and (got["map"][:70] == -1).all() and not got["w"][:70].any()
    assert np.array_equal(_bits(got["updated"]), _bits(c["nominal"]))


def test_sanitizer_run(exe_san, tmp_path):
    """the stand-alone program under AddressSanitizer and UBSan (-fno-sanitize-recover: any report ends the run with an error)"""
    assert _run(exe_san, "philox").split("\n")[:3] == [k[2] for k in KNOWN]
    for B, count in [(70, 12), (300, 3), (257, 5)]:
        c = _case(B, count)
        _check_against_restatement(_pass(exe_san, c, tmp_path), c)
    c = _case(20, 12)                              # one instance, exempt: nothing to perturb, all the weight on it
    c.update(B=1, exempt=1, costs=np.array([1.5]))
    got = _pass(exe_san, c, tmp_path)
    assert np.array_equal(_bits(got["keys"][:, :, 0]), _bits(c["nominal"])) and np.array_equal(_bits(got["updated"]), _bits(c["nominal"]))


# ------------------------------------------------------------------ C-ABI contract
ENTRIES = ["attach", "detach", "seed", "perturb", "cost", "set_cost_host", "get_cost_host", "cost_device", "update", "shift", "result_host",
           "best_map_device", "get_nominal_host", "set_nominal_host", "info"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def test_entries_are_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    header = open(os.path.join(ROOT, "include", "saip.h")).read()
    L = sp.lib()
    for e in ENTRIES:
        name = "saip_batch_sampler_" + e
        assert re.search(r"\b" + name + r"\(saip_batch\*", header), name
        assert getattr(L, name).argtypes is not None, name       # bound with a signature in capi.lib()
    assert "csrc/saip_sampler.hip" in capi.SOURCES and "csrc/saip_sampler.h" in capi.HEADERS
    third = open(os.path.join(ROOT, "THIRD_PARTY.md")).read()
    assert "Philox" in third and "Random123" in third


def _all_refuse(L, b, want, probe):
    """every entry that needs a sampler answers `want` and leaves its outputs alone"""
    out, i0, i1 = np.full(8, SENTINEL), C.c_int(7), C.c_int(7)
    seed, rnd = C.c_ulonglong(7), C.c_longlong(7)
    w8, t3 = np.ones(8), np.zeros(3)
    calls = [L.saip_batch_sampler_detach(b, 0), L.saip_batch_sampler_detach(b, -1), L.saip_batch_sampler_seed(b, 1), L.saip_batch_sampler_perturb(b),
             L.saip_batch_sampler_cost(b, _dp(w8), _dp(t3), 1.0, 1.0), L.saip_batch_sampler_set_cost_host(b, _dp(probe)),
             L.saip_batch_sampler_get_cost_host(b, _dp(out)), L.saip_batch_sampler_update(b, 1.0), L.saip_batch_sampler_shift(b, 1),
             L.saip_batch_sampler_result_host(b, C.byref(i0), C.byref(i1), _dp(out), _dp(out[1:]), _dp(out[2:])),
             L.saip_batch_sampler_get_nominal_host(b, 0, _dp(out)), L.saip_batch_sampler_set_nominal_host(b, 0, _dp(probe)),
             L.saip_batch_sampler_info(b, 0, C.byref(i0), C.byref(i1), C.byref(seed), C.byref(rnd))]
    assert calls == [want] * len(calls), calls
    assert (out == SENTINEL).all() and (i0.value, i1.value) == (7, 7) and seed.value == 7 and rnd.value == 7
    assert not L.saip_batch_sampler_cost_device(b) and not L.saip_batch_sampler_best_map_device(b)


def test_c_abi_error_contract(sp):
    """a configuration-only batch: argument errors first, then the order errors.  No schedule can be attached without a device, so
    every sampler entry ends at SAIP_ERR_ORDER there; the refusals that need a schedule are checked on the GPU."""
    from sai_primitives_amd import capi
    from test_goal_schedule_cpu import _controller_batch
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    B = 4
    sigma, probe = np.full(36, 0.1), np.zeros(256)
    robot, b = _controller_batch(sp, L, B)
    try:
        assert L.saip_batch_sampler_attach(b, 0, _dp(sigma), None, 1) == ORDER and b"saip_batch_finalize" in L.saip_last_error()
        _all_refuse(L, b, ORDER, probe)                               # unfinalized
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_batch_sampler_attach(None, 0, _dp(sigma), None, 1) == INVALID
        for task in (-1, 2):
            assert L.saip_batch_sampler_attach(b, task, _dp(sigma), None, 1) == INVALID and b"out of range" in L.saip_last_error()
        assert L.saip_batch_sampler_attach(b, 0, None, None, 1) == INVALID and b"null sigma" in L.saip_last_error()
        for exempt in (-1, B + 1):
            assert L.saip_batch_sampler_attach(b, 0, _dp(sigma), None, exempt) == INVALID and b"exempt" in L.saip_last_error()
        assert L.saip_batch_sampler_attach(b, 0, _dp(sigma), None, B) == ORDER and b"no goal schedule" in L.saip_last_error()
        assert L.saip_batch_sampler_attach(b, 1, _dp(sigma), _dp(probe), 0) == ORDER
        _all_refuse(L, b, ORDER, probe)
        assert b"no sampler is attached" in L.saip_last_error()
        # the pure argument checks come before anything else is looked at
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert L.saip_batch_sampler_update(b, bad) == INVALID and b"temperature" in L.saip_last_error()
        assert L.saip_batch_sampler_shift(b, -1) == INVALID and b"negative" in L.saip_last_error()
        assert L.saip_batch_sampler_detach(b, -2) == INVALID and L.saip_batch_sampler_info(b, -1, None, None, None, None) == INVALID
        assert L.saip_batch_sampler_get_nominal_host(b, 5, _dp(probe)) == INVALID
        # nothing changed for a task without a sampler: the schedule's detach still answers as before
        assert L.saip_batch_goal_schedule_detach(b, 0) == ORDER and L.saip_batch_goal_schedule_detach(b, -1) == 0
    finally:
        L.saip_batch_destroy(b)
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_sampler_attach(b, 0, _dp(sigma), None, 1) == ORDER and b"model queries only" in L.saip_last_error()
        _all_refuse(L, b, ORDER, probe)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_checks_shapes(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    with pytest.raises(ValueError, match="8 summary weights"):
        ctrl.rolloutCost(summary_weights=np.ones(5))
    with pytest.raises(ValueError, match=r"target of shape \(3,\)"):
        ctrl.rolloutCost(target=np.zeros(4))
    with pytest.raises(ValueError, match="costs expected"):
        ctrl.setRolloutCost(np.zeros(B + 1))
    for fn in (lambda: ctrl.updateSampler(1.0), lambda: ctrl.shiftSampler(1), ctrl.perturbGoalSchedules, ctrl.samplerResult, ctrl.getRolloutCost,
               lambda: ctrl.seedSampler(3), lambda: ctrl.setRolloutCost(np.zeros(B)), lambda: ctrl.rolloutCost(target=np.zeros(3))):
        with pytest.raises(sp.SaipError, match="no sampler"):
            fn()
    with pytest.raises(sp.SaipError, match="no goal schedule"):
        mf.attachSampler(0.1)
    for fn in (jt.samplerNominal, lambda: jt.setSamplerNominal(np.zeros((3, 7)))):
        with pytest.raises(sp.SaipError, match="no sampler"):
            fn()
    with pytest.raises(sp.SaipError, match="no sampler"):
        mf.detachSampler()
