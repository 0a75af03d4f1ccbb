"""Scenario groups of the resident rollout sampler, everything that needs no GPU: the per-element code (csrc/saip_sampler.h) compiled for
the host as a stand-alone program (tests/cpp/sampler_scenarios_host.cpp) against the NumPy restatement tests/sampler_scenarios_ref.py --
grouped perturb, group cost under the three risk measures, weights, best map and update -- the same program under AddressSanitizer and
UBSan, and the C-ABI and facade contract of the five new entries.

Group cost, perturbed linear rows of exempt columns, the scenario blocks among themselves and the best map are compared bit for bit: sums,
comparisons and one division, the same on both sides.  Perturbed rows, weights and means differ by the two maths libraries only and stay
within the derived bounds of tests/test_sampler_cpu.py, taken for the C candidates the weights and the update run over."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import sampler_ref as SR
import sampler_scenarios_ref as SS
from test_sampler_cpu import SENTINEL, U, _bits, _dp, _rot, linear_bound, mean_bound, perturbed_rotation_bound, rotation_mean_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
SHAPES = [(35, 2), (300, 3), (70, 1)]
RISKS = [("mean", 0), ("max", 0), ("cvar", 1), ("cvar", 2)]
CASES = [(Cn, M, risk, tail) for Cn, M in SHAPES[:2] for risk, tail in RISKS] + [(70, 1, "mean", 0)]      # one scenario has no risk measure to choose


def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-ffp-contract=off"] + extra + ["-o", exe, os.path.join(ROOT, "tests", "cpp", "sampler_scenarios_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("scen_host"), "sampler_scenarios_host", [])


@pytest.fixture(scope="module")
def exe_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("scen_host_san"), "sampler_scenarios_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def _costs(rng, Cn, M):
    """(C * M,) costs: +inf, -inf and NaN in some scenarios of some candidates, every scenario of candidate 9 invalid, ties, signed zeros"""
    v = rng.uniform(1.0, 3.0, (M, Cn))
    v[0, 3], v[M - 1, 5], v[0, 7] = np.inf, -np.inf, np.nan
    v[:, 9] = [np.nan, np.inf, -np.inf][:M] if M <= 3 else np.nan
    v[:, 11] = 1.25                                   # all scenarios equal
    v[:, 13] = -0.0                                   # a largest value of -0.0
    v[0, 13] = 0.0 if M > 1 else -0.0
    v[:, 20] = rng.uniform(-2.0, -1.0, M)             # negative costs
    return v.reshape(-1)


def _case(Cn, M, count, risk="mean", tail=0, seed=7):
    rng = np.random.default_rng(1000 * Cn + 10 * M + count + seed)
    K, B = 3, Cn * M
    ld = -(-B // 32) * 32 + 32
    r_rot = 3 if count == 12 else None
    d = SR.dim(count, r_rot)
    nominal = rng.uniform(-0.5, 0.5, (K, count))
    if r_rot is not None:
        for k in range(K):
            nominal[k, 3:] = _rot(rng, 0.4 * (k + 1)).reshape(9)
    return dict(C=Cn, M=M, B=B, ld=ld, K=K, count=count, r_rot=r_rot, d=d, task=1, exempt=2, rnd=3, seed=0x5eed0000beef + B, nominal=nominal,
                sigma=rng.uniform(0.01, 0.1, d), costs=_costs(rng, Cn, M), risk=risk, tail=tail, temperature=0.25)


def _pass(exe, c, tmp):
    K, count, ld = c["K"], c["count"], c["ld"]
    head = np.array([c["C"], c["M"], ld, K, count, int(c["r_rot"] is not None), c["r_rot"] if c["r_rot"] is not None else count, c["task"], c["exempt"], c["rnd"],
                     SS.RISKS[c["risk"]], c["tail"]], np.int32)
    blob = head.tobytes() + struct.pack("<Qd", c["seed"], c["temperature"])
    blob += b"".join(np.ascontiguousarray(c[k], np.float64).tobytes() for k in ("nominal", "sigma", "costs"))
    fin, fout = tmp / "in.bin", tmp / "out.bin"
    fin.write_bytes(blob)
    out = subprocess.run([exe, "run", str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    out = np.frombuffer(fout.read_bytes(), np.float64)
    sizes = [("keys", K * count * ld), ("group", ld), ("w", ld), ("map", ld), ("result", 5), ("updated", K * count)]
    assert out.size == sum(n for _, n in sizes)
    got, at = {}, 0
    for name, n in sizes:
        got[name] = out[at:at + n]
        at += n
    got["keys"], got["updated"] = got["keys"].reshape(K, count, ld), got["updated"].reshape(K, count)
    return got


def _check(got, c):
    Cn, M, B, K, count, r_rot = c["C"], c["M"], c["B"], c["K"], c["count"], c["r_rot"]
    rows, _ = SR.coords(count, r_rot)
    keys = got["keys"][:, :, :B].transpose(0, 2, 1)
    # perturb: every block is block 0 bit for bit, exempt candidates hold the nominal in every block, the padding is untouched
    for s in range(M):
        assert np.array_equal(_bits(keys[:, s * Cn:(s + 1) * Cn]), _bits(keys[:, :Cn])), s
        assert np.array_equal(_bits(keys[:, s * Cn:s * Cn + c["exempt"]]), _bits(np.broadcast_to(c["nominal"][:, None], (K, c["exempt"], count))))
    assert (got["keys"][:, :, B:] == SENTINEL).all()
    ref = SS.perturb(c["nominal"], c["sigma"], c["seed"], c["rnd"], c["task"], Cn, M, c["exempt"], r_rot)
    sig = c["sigma"].max()
    assert np.abs(keys[:, :, rows] - ref[:, :, rows]).max() <= linear_bound(sig, np.abs(ref).max())
    assert np.abs(keys[:, c["exempt"]:Cn, rows] - c["nominal"][:, None, rows]).max() > 1e-3
    if r_rot is not None:
        assert np.abs(keys[:, :, 3:] - ref[:, :, 3:]).max() <= perturbed_rotation_bound(sig)
    # group cost: bit for bit, the invalid candidates included
    if M == 1:
        g = c["costs"]
        w, res = SR.weights(g, c["temperature"])
        bmap = np.full(B, res["best"])
    else:
        g, w, res, bmap = SS.weights(c["costs"], Cn, M, c["risk"], c["tail"], c["temperature"])
        assert np.isposinf(g[[3, 5, 7, 9]]).all() and np.isfinite(np.delete(g, [3, 5, 7, 9])).all()
        assert g[11] == 1.25 and _bits(g[13:14])[0] == 0           # +0.0 from signed zeros
    assert np.array_equal(_bits(got["group"][:Cn]), _bits(g))
    assert (got["group"][Cn:] == SENTINEL).all() and (got["w"][Cn:] == SENTINEL).all() and (got["map"][B:] == SENTINEL).all()
    # weights, result and best map over candidates
    assert (got["result"][0], got["result"][1]) == (res["best"], res["n_valid"]) and got["result"][2] == res["min_cost"]
    assert np.array_equal(got["map"][:B], bmap)
    assert np.abs(got["w"][:Cn] - w).max() <= 4 * 2 * U
    assert abs(got["result"][3] - res["sum_w"]) <= mean_bound(Cn, 1.0) * res["sum_w"]
    assert abs(got["result"][4] - res["ess"]) <= 4 * mean_bound(Cn, 1.0) * res["ess"]
    # update over block 0 with the candidates' weights
    new = SS.update(c["nominal"], keys, w, res["best"], Cn, r_rot)
    assert np.abs(got["updated"][:, rows] - new[:, rows]).max() <= mean_bound(Cn, np.abs(keys[:, :, rows]).max())
    if r_rot is not None:
        lg = np.abs(SR.log_so3(c["nominal"][:, None, 3:].reshape(K, 1, 3, 3), keys[:, :Cn, 3:].reshape(K, Cn, 3, 3))).max()
        assert np.abs(got["updated"][:, 3:] - new[:, 3:]).max() <= rotation_mean_bound(Cn, lg)
    assert not np.array_equal(got["updated"], c["nominal"])


@pytest.mark.parametrize("Cn,M,risk,tail", CASES)
def test_host_build_matches_the_restatement(exe, tmp_path, Cn, M, risk, tail):
    c = _case(Cn, M, 12, risk, tail)
    _check(_pass(exe, c, tmp_path), c)


def test_cvar_of_one_scenario_is_max_and_of_all_is_the_descending_mean(exe, tmp_path):
    for Cn, M in SHAPES[:2]:
        a, b = _case(Cn, M, 3, "max", 0), _case(Cn, M, 3, "cvar", 1)
        ga, gb = _pass(exe, a, tmp_path), _pass(exe, b, tmp_path)
        for name in ("group", "w", "map", "result", "updated"):
            assert np.array_equal(_bits(ga[name]), _bits(gb[name])), name
        full = _pass(exe, _case(Cn, M, 3, "cvar", M), tmp_path)["group"][:Cn]
        mean = _pass(exe, _case(Cn, M, 3, "mean", 0), tmp_path)["group"][:Cn]
        ok = np.isfinite(mean)
        assert np.abs(full[ok] - mean[ok]).max() <= 2 * M * U * np.abs(mean[ok]).max() + 1e-300      # the same values in another order
        assert (ga["group"][:Cn][ok] >= full[ok]).all()


def test_the_restatement_on_known_values():
    v = np.array([[1.0, 4.0, np.nan, -1.0], [3.0, 2.0, 1.0, -3.0], [2.0, 0.5, 1.0, -2.0]]).reshape(-1)        # M = 3 blocks of C = 4
    assert np.array_equal(SS.group_cost(v, 4, 3, "mean"), [2.0, 6.5 / 3.0, np.inf, -2.0])
    assert np.array_equal(SS.group_cost(v, 4, 3, "max"), [3.0, 4.0, np.inf, -1.0])
    assert np.array_equal(SS.group_cost(v, 4, 3, "cvar", 2), [2.5, 3.0, np.inf, -1.5])
    assert np.array_equal(SS.best_map(8, 4, 2), [2, 2, 2, 2, 6, 6, 6, 6]) and (SS.best_map(8, 4, -1) == -1).all()
    assert [SS.tail_of(M, a) for M, a in [(4, 0.25), (4, 0.26), (4, 1.0), (3, 1e-9), (64, 0.1)]] == [1, 2, 4, 1, 7]


def test_sanitizer_run(exe_san, tmp_path):
    """the stand-alone program under AddressSanitizer and UBSan (-fno-sanitize-recover: any report ends the run with an error)"""
    for (Cn, M), (risk, tail), count in [((35, 2), ("cvar", 2), 12), ((300, 3), ("max", 0), 3), ((300, 3), ("cvar", 2), 12), ((70, 1), ("mean", 0), 12), ((35, 2), ("mean", 0), 5)]:
        c = _case(Cn, M, count, risk, tail)
        _check(_pass(exe_san, c, tmp_path), c)
    c = _case(21, 64, 3, "cvar", 64)               # the most scenarios the ABI takes
    _check(_pass(exe_san, c, tmp_path), c)


# ------------------------------------------------------------------ C-ABI contract
ENTRIES = ["set_scenarios", "scenarios_info", "get_group_cost_host", "group_cost_device", "share_scenario_tables", "weights_device"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def test_entries_are_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    header = open(os.path.join(ROOT, "include", "saip.h")).read()
    L = sp.lib()
    exported = subprocess.run(["nm", "-D", "--defined-only", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for e in ENTRIES:
        name = "saip_batch_sampler_" + e
        assert re.search(r"\b" + name + r"\(saip_batch\*", header), name
        assert re.search(r" T " + name + r"\b", exported), name
        assert getattr(L, name).argtypes is not None, name
    for k, v in [("SAIP_SAMPLER_MAX_SCENARIOS", 64), ("SAIP_SAMPLER_RISK_MEAN", 0), ("SAIP_SAMPLER_RISK_MAX", 1), ("SAIP_SAMPLER_RISK_CVAR", 2)]:
        assert re.search(r"#define\s+" + k + r"\s+" + str(v) + r"\b", header) and getattr(capi, k) == v
    assert SS.MAX_SCENARIOS == capi.SAIP_SAMPLER_MAX_SCENARIOS and SS.RISKS == dict(mean=0, max=1, cvar=2)


def test_c_abi_error_contract(sp):
    """a configuration-only batch: the argument errors of _set_scenarios that are decided before the sampler is looked at, each naming the
    offending value; then SAIP_ERR_ORDER of all five entries (no sampler can be attached without a device)"""
    from sai_primitives_amd import capi
    from test_goal_schedule_cpu import _controller_batch
    L = sp.lib()
    ORDER, INVALID = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT
    MEAN, MAX, CVAR = capi.SAIP_SAMPLER_RISK_MEAN, capi.SAIP_SAMPLER_RISK_MAX, capi.SAIP_SAMPLER_RISK_CVAR
    B = 6
    robot, b = _controller_batch(sp, L, B)
    try:
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_batch_sampler_set_scenarios(None, 2, MEAN, 0) == INVALID and b"null batch" in L.saip_last_error()
        for M in (0, -3, 65):
            assert L.saip_batch_sampler_set_scenarios(b, M, MEAN, 0) == INVALID and f"n_scenarios = {M}".encode() in L.saip_last_error()
        for risk in (-1, 3, 99):
            assert L.saip_batch_sampler_set_scenarios(b, 2, risk, 0) == INVALID and f"risk measure {risk}".encode() in L.saip_last_error()
        for risk, tail in [(MEAN, 1), (MAX, 2), (MEAN, -1), (CVAR, 0), (CVAR, 3), (CVAR, -1)]:
            assert L.saip_batch_sampler_set_scenarios(b, 2, risk, tail) == INVALID and f"tail = {tail}".encode() in L.saip_last_error()
        for M in (4, 5, 64):
            assert L.saip_batch_sampler_set_scenarios(b, M, MEAN, 0) == INVALID
            assert f"n_scenarios = {M}".encode() in L.saip_last_error() and b"6 instances" in L.saip_last_error()
        # then the order errors, outputs left alone
        out, n = np.full(8, SENTINEL), [C.c_int(7) for _ in range(5)]
        calls = [L.saip_batch_sampler_set_scenarios(b, 2, MEAN, 0), L.saip_batch_sampler_set_scenarios(b, 3, CVAR, 2), L.saip_batch_sampler_set_scenarios(b, 1, MEAN, 0),
                 L.saip_batch_sampler_scenarios_info(b, C.byref(n[0]), C.byref(n[1]), C.byref(n[2]), C.byref(n[3])), L.saip_batch_sampler_scenarios_info(b, None, None, None, None),
                 L.saip_batch_sampler_get_group_cost_host(b, _dp(out)), L.saip_batch_sampler_get_group_cost_host(b, None),
                 L.saip_batch_sampler_share_scenario_tables(b, C.byref(n[4])), L.saip_batch_sampler_share_scenario_tables(b, None)]
        assert calls == [ORDER] * len(calls), calls
        assert b"no sampler is attached" in L.saip_last_error()
        assert (out == SENTINEL).all() and [x.value for x in n] == [7] * 5
        assert not L.saip_batch_sampler_group_cost_device(b) and not L.saip_batch_sampler_group_cost_device(None)
        assert not L.saip_batch_sampler_weights_device(b) and not L.saip_batch_sampler_weights_device(None)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_checks_risk_and_alpha(sp):
    B = 6
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    for risk in ("median", "MEAN", None, 1):
        with pytest.raises(ValueError, match="unknown risk"):
            ctrl.setSamplerScenarios(2, risk=risk)
    for alpha in (None, 0.0, -0.5, 1.0001, float("nan")):
        with pytest.raises(ValueError, match=r"alpha in \(0, 1\]"):
            ctrl.setSamplerScenarios(2, risk="cvar", alpha=alpha)
    for risk in ("mean", "max"):
        with pytest.raises(ValueError, match="applies to risk \"cvar\" only"):
            ctrl.setSamplerScenarios(2, risk=risk, alpha=0.5)
    with pytest.raises(ValueError, match="n_scenarios = 4"):              # the ABI's own argument errors arrive as ValueError
        ctrl.setSamplerScenarios(4)
    for fn in (lambda: ctrl.setSamplerScenarios(2), lambda: ctrl.setSamplerScenarios(3, "cvar", 0.5), lambda: ctrl.setSamplerScenarios(2, "max"),
               ctrl.samplerScenarios, ctrl.samplerGroupCost, ctrl.shareScenarioTables):
        with pytest.raises(sp.SaipError, match="no sampler"):
            fn()


def test_cpp_facade_host_checks(sp, tmp_path):
    from test_rollout_record_cpu import _robot_file
    exe = str(tmp_path / "sampler_scenarios_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sampler_scenarios_example.cpp"),
                           "-L" + PKG, "-lsaip", "-Wl,-rpath," + PKG, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe, _robot_file(tmp_path), "cfgonly"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "SCENARIOS_CFG_OK" in out.stdout, out.stdout + out.stderr
