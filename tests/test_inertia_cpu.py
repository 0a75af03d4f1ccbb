"""The resident inertia table of the simulator, host side (no GPU needed): the C-ABI entries are declared, exported and bound; the argument
and call-order errors come back with the documented codes before the device is needed and write nothing; the Python facade raises the
same; the host build of csrc/saip_inertia.h (tests/cpp/inertia_host.cpp, also under ASan/UBSan) matches the NumPy restatement
tests/inertia_ref.py bit for bit in the composed rows and in the draw; the restatement composes what rigid bodies compose to."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import inertia_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_inertia_attach", "saip_batch_inertia_detach", "saip_batch_inertia_info", "saip_batch_inertia_set_rows_host",
                  "saip_batch_inertia_set_parts_host", "saip_batch_inertia_randomize", "saip_batch_inertia_rows_host"]
POINTER_ENTRIES = ["saip_batch_inertia_rows_device"]
WORDS = ["m", "cx", "cy", "cz", "Ixx", "Iyy", "Izz", "Ixy", "Ixz", "Iyz"]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int))


def _links(name):
    with open(os.path.join(PKG, "robots", name + ".json")) as f:
        return json.load(f)["links"]


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    src = open(os.path.join(PKG, "csrc", "saip_inertia.h")).read()
    for name, val in [("ROW_WORDS", 10), ("BODY_WORDS", 4), ("PAYLOAD_WORDS", 7), ("MAX_PAYLOADS", 2)]:
        assert re.search(rf"#define SAIP_INERTIA_{name} {val}\b", hdr), name
        assert getattr(capi, "SAIP_INERTIA_" + name) == val == getattr(IR, name)
        assert re.search(rf"\bINERTIA_{name} = {val}\b", src), name
    for name, val in [("TABLE_BODIES", 2), ("TABLE_PAYLOADS", 3)]:
        assert re.search(rf"\bINERTIA_{name} = {val}\b", src) and getattr(IR, name) == val
    import plant_ref as PL
    assert {IR.TABLE_BODIES, IR.TABLE_PAYLOADS}.isdisjoint({PL.TABLE_JOINTS, PL.TABLE_WRENCHES})
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + POINTER_ENTRIES:
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else C.c_void_p)
    for f in ("csrc/saip_inertia.hip", "csrc/saip_engine_inertia.cpp"):
        assert f in capi.SOURCES
    assert "csrc/saip_inertia.h" in capi.HEADERS
    assert list(sp.RobotController.INERTIA_ROW_WORDS) == WORDS
    for m in ("attachInertia", "setInertiaRows", "setInertiaParts", "randomizeInertia", "inertiaRows", "inertiaRowsDevice", "detachInertia"):
        assert callable(getattr(sp.RobotController, m))
    hpp = open(os.path.join(ROOT, "include", "saip", "SaiPrimitivesBatched.hpp")).read()
    for m in ("attachInertia", "setInertiaRows", "setInertiaParts", "randomizeInertia", "inertiaRows", "inertiaRowsDevice", "detachInertia"):
        assert re.search(r"\b" + m + r"\s*\(", hpp), m


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
    v, out = C.c_int(7), np.full(7 * 10 * 4, 7.0)
    assert L.saip_batch_inertia_detach(b) == code
    assert L.saip_batch_inertia_info(b, C.byref(v), None, None, _dp(out)) == code
    assert L.saip_batch_inertia_set_rows_host(b, _dp(out)) == code
    assert L.saip_batch_inertia_set_parts_host(b, _dp(out), 0, _dp(out), 0) == code
    assert L.saip_batch_inertia_randomize(b, 1, 0, _dp(out), _dp(out), None, None) == code
    assert L.saip_batch_inertia_rows_host(b, _dp(out)) == code
    assert L.saip_batch_inertia_rows_device(b) is None
    assert v.value == 7 and (out == 7.0).all()                            # nothing was written


ROWS = IR.model_rows(_links("panda_arm"))


def test_c_abi_error_contract(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    att = L.saip_batch_inertia_attach
    links = np.array([7, 4], np.int32)                                    # end-effector (welded to link7), link5

    def call(b, rows=ROWS, per=0, P=2, links=links):
        return att(b, None if rows is None else _dp(np.ascontiguousarray(rows)), per, P, None if links is None else _ip(links))

    def refused(b, msg, **kw):
        assert call(b, **kw) == INVALID and msg in L.saip_last_error(), (kw, L.saip_last_error())
        assert L.saip_batch_inertia_info(b, None, None, None, None) == ORDER           # nothing got attached

    assert call(None) == INVALID
    _others_refuse(L, None, INVALID)
    B = 4
    robot, b = _controller_batch(sp, L, B)
    try:
        assert call(b) == ORDER                                          # before finalize, whatever the arguments
        assert call(b, P=9) == ORDER
        _others_refuse(L, b, ORDER)
        assert L.saip_batch_finalize(b) == 0
        for P in (-1, 3, 2**31 - 1):
            refused(b, b"payloads required", P=P)
        refused(b, b"null payload links", links=None)
        for bad in (-1, 10_000):
            l2 = links.copy()
            l2[1] = bad
            refused(b, b"payload 1: link index", links=l2)
        # one bad word of one body, batch-uniform and per instance (there: of one instance only): NaN or infinity anywhere, m < 0, an
        # inertia with a negative eigenvalue
        per = np.ascontiguousarray(np.repeat(ROWS[:, :, None], B, axis=2))
        cases = [(k % 7, k, bad, b"word %s is not finite" % WORDS[k].encode()) for k in range(10) for bad in (np.nan, np.inf, -np.inf)]
        cases += [(2, 0, -1e-9, b"word m = -1e-09 is below 0"), (3, 4, -1e-3, b"words Ixx..Iyz: the inertia has the eigenvalue"),
                  (5, 7, 1.0, b"words Ixx..Iyz: the inertia has the eigenvalue")]
        for j, k, val, msg in cases:
            t1 = ROWS.copy()
            t1[j, k] = val
            refused(b, b"body %d: " % j + msg, rows=t1)
            t2 = per.copy()
            t2[j, k, B - 1] = val
            refused(b, b"body %d of instance 3: " % j + msg, rows=t2, per=1)
        # valid arguments reach the device check (a configuration-only batch): nothing gets attached.  The triangle inequality is not
        # enforced, a massless body and an eigenvalue inside the tolerance pass
        odd = ROWS.copy()
        odd[1, 4:7], odd[2, 0], odd[3, 4:10] = (1.0, 0.1, 0.1), 0.0, (1.0, 1.0, -1e-13, 0.0, 0.0, 0.0)
        for kw in (dict(), dict(rows=None), dict(rows=None, per=1), dict(rows=per, per=1), dict(P=0, links=None), dict(rows=odd), dict(P=1)):
            assert call(b, **kw) == NO_DEVICE and b"no CPU path" in L.saip_last_error(), kw
        _others_refuse(L, b, ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_a_payload_on_the_fixed_base_is_refused(sp):
    from sai_primitives_amd import capi
    import chains as CH
    L = sp.lib()
    links = _links("panda_arm")
    stand = CH._link("stand", "fixed", [0.0, 0.0, 0.1], [0, 0, 0], [0, 0, 1], 5.0, [0.0, 0.0, 0.0], [0.1, 0.1, 0.1, 0.0, 0.0, 0.0], 0.0, 0.0, 0.0)
    robot = sp.SaiModel(dict(name="panda_on_stand", links=[stand] + links), 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        tid = C.c_int(-1)
        assert L.saip_batch_add_joint_task(b, b"jt", None, 0, 0.001, C.byref(tid)) == 0
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_batch_inertia_attach(b, None, 0, 1, _ip(np.array([0], np.int32))) == capi.SAIP_ERR_INVALID_ARGUMENT
        assert b"payload 0: link stand is welded to the fixed base" in L.saip_last_error()
    finally:
        L.saip_batch_destroy(b)


def test_model_only_batch_refuses_the_table(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        assert L.saip_batch_inertia_attach(b, None, 0, 0, None) == capi.SAIP_ERR_ORDER
        assert b"model queries only" in L.saip_last_error()
        _others_refuse(L, b, capi.SAIP_ERR_ORDER)
    finally:
        L.saip_batch_destroy(b)


def test_python_facade_without_a_device(sp):
    B = 4
    robot = sp.SaiModel("panda_arm", B, device=-1)
    mf, jt = sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)
    ctrl = sp.RobotController(robot, [mf, jt])
    for bad in (np.zeros(10), np.zeros((6, 10)), np.zeros((7, B, 10))):
        with pytest.raises(ValueError, match="rows of shape"):
            ctrl.attachInertia(bad)
    for bad in (np.zeros((7, 10)), np.zeros((7, 10, B)), np.zeros((7, B + 1, 10))):
        with pytest.raises(ValueError, match="per-instance rows of shape"):
            ctrl.attachInertia(bad, per_instance=True)
    with pytest.raises(ValueError, match="unknown link"):
        ctrl.attachInertia(payload_links=["no-such-link"])
    with pytest.raises(ValueError, match="payloads required"):
        ctrl.attachInertia(payload_links=["link4"] * 3)
    t = ROWS.copy()
    t[3, 0] = -1.0
    with pytest.raises(ValueError, match="body 3: word m = -1 is below 0"):
        ctrl.attachInertia(t)
    for kw in (dict(), dict(rows=ROWS), dict(payload_links=["end-effector", "link4"]), dict(per_instance=True),
               dict(rows=np.repeat(ROWS[:, None, :], B, axis=1), per_instance=True)):
        with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
            ctrl.attachInertia(**kw)
    nb = IR.neutral_bodies(7)
    for fn in (ctrl.detachInertia, ctrl.inertiaInfo, ctrl.inertiaRows, lambda: ctrl.setInertiaRows(ROWS), lambda: ctrl.setInertiaParts(nb),
               lambda: ctrl.randomizeInertia(1, bodies=(nb, nb))):
        with pytest.raises(sp.SaipError, match="no inertia table is attached"):
            fn()
    assert ctrl.inertiaRowsDevice() is None


# ------------------------------------------------------------------ the host build of the header against the restatement
def _build(tmp, name, extra):
    exe = str(tmp / name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off"] + extra +
                          ["-o", exe, os.path.join(ROOT, "tests", "cpp", "inertia_host.cpp")])
    return exe


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    return [_build(tmp_path_factory.mktemp("inertia_host"), "inertia_host", []),
            _build(tmp_path_factory.mktemp("inertia_host_san"), "inertia_host_san", ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])]


def _case(robot, payload_links, N, perb, perp, seed, zero_mass=False, equal_bounds=False):
    """parts of N instances on `robot`: s in [0.8, 1.2], |d| <= 0.02, payloads of 0..3 kg (some exactly 0)"""
    links = _links(robot)
    frames = IR.link_frames(links)
    names = [l["name"] for l in links]
    rows = IR.model_rows(links)
    n, P = rows.shape[0], len(payload_links)
    rng = np.random.default_rng(seed)
    c = dict(N=N, n=n, P=P, perb=perb, perp=perp, rows=rows, links=links, payload_links=payload_links)
    c["site_body"] = [frames[names.index(x)][0] for x in payload_links]
    c["site_rot"] = [frames[names.index(x)][1] for x in payload_links]
    c["site_pos"] = [frames[names.index(x)][2] for x in payload_links]
    shape_b, shape_p = ((n, N, 4) if perb else (n, 4)), ((P, N, 7) if perp else (P, 7))
    bodies = np.concatenate([rng.uniform(0.8, 1.2, shape_b[:-1] + (1,)), rng.uniform(-0.02, 0.02, shape_b[:-1] + (3,))], axis=-1)
    pay = np.concatenate([rng.uniform(0.0, 3.0, shape_p[:-1] + (1,)), rng.uniform(-0.1, 0.1, shape_p[:-1] + (3,)), rng.uniform(0.0, 0.08, shape_p[:-1] + (3,))], axis=-1)
    if P and perp:
        pay[0, ::3, 0] = 0.0                                             # m_p = 0 in some instances: the payload is not there
    if P and zero_mass:
        pay[..., 0] = 0.0
    c["bodies"], c["payloads"] = bodies, pay
    c["seed"], c["round"] = int(rng.integers(0, 2 ** 63)) * 2 + 1, int(rng.integers(0, 2 ** 32))
    bl, bh = IR.neutral_bodies(n), IR.neutral_bodies(n)
    bl[:, 0], bh[:, 0], bl[:, 1:], bh[:, 1:] = 0.8, 1.2, -0.02, 0.02
    bh[::2, 2] = bl[::2, 2]                                              # lo == hi on some words
    bl[1, 3], bh[1, 3] = bh[1, 3], bl[1, 3]                              # reversed on one
    pl, ph = np.zeros((P, 7)), np.tile([3.0, 0.1, 0.1, 0.1, 0.08, 0.08, 0.08], (P, 1))
    pl[:, 1:4] = -0.1
    if P:
        ph[0, 5] = pl[0, 5] = 0.05
    if equal_bounds:
        bh, ph = bl.copy(), pl.copy()
    c["bounds"] = (bl, bh, pl, ph)
    return c


def _run(exe, tmp, c):
    N, n, P = c["N"], c["n"], c["P"]
    with open(tmp / "in.bin", "wb") as f:
        f.write(np.array([N, n, P, c["perb"], c["perp"]], np.int32).tobytes())
        f.write(np.asarray(c["site_body"], np.int32).tobytes())
        f.write(np.ascontiguousarray(c["rows"]).tobytes())
        f.write(np.asarray(c["site_pos"], float).reshape(-1).tobytes())
        f.write(np.asarray(c["site_rot"], float).reshape(-1).tobytes())
        bt, pt = c["bodies"], c["payloads"]
        f.write(np.ascontiguousarray(bt.transpose(0, 2, 1) if c["perb"] else bt).tobytes())
        f.write(np.ascontiguousarray(pt.transpose(0, 2, 1) if c["perp"] else pt).tobytes())
        f.write(np.array([c["seed"]], np.uint64).tobytes())
        f.write(np.array([c["round"], 0], np.uint32).tobytes())
        for a in c["bounds"]:
            f.write(np.ascontiguousarray(a).tobytes())
    out = subprocess.run([exe, str(tmp / "in.bin"), str(tmp / "out.bin")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    raw = np.fromfile(tmp / "out.bin")
    got, at = {}, 0
    for name, shp in [("rows", (n, 10, N)), ("db", (n, 4, N)), ("dp", (P, 7, N)), ("rows2", (n, 10, N))]:
        k = int(np.prod(shp))
        got[name] = raw[at:at + k].reshape(shp).transpose(0, 2, 1)
        at += k
    assert at == raw.size
    return got


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _want(c, N=None):
    N = c["N"] if N is None else N
    sites = (c["site_body"], c["site_pos"], c["site_rot"])
    rows = IR.compose(c["rows"], c["bodies"], c["payloads"], *sites, N)
    bl, bh, pl, ph = c["bounds"]
    rows2, db, dp = IR.randomized(c["rows"], c["seed"], c["round"], N, (bl, bh), (pl, ph), *sites)
    return rows, db, dp, rows2


# robot, payload sites, instances, per-instance bodies / payloads: revolute and prismatic bodies; a payload on a movable link, on a welded
# link, two on one body (link7 and the end-effector welded to it); m_p = 0; lo == hi
CASES = [("panda_arm", ["link4"], 67, 1, 1, {}), ("panda_arm", ["end-effector"], 5, 1, 0, {}), ("panda_sliding_base", ["link7", "end-effector"], 64, 1, 1, {}),
         ("panda_sliding_base", ["link0", "link3"], 33, 0, 0, {}), ("chain30", [], 9, 1, 0, {}), ("panda_arm", ["end-effector", "link2"], 12, 1, 1, dict(zero_mass=True)),
         ("panda_arm", ["end-effector"], 7, 0, 1, dict(equal_bounds=True))]


@pytest.mark.parametrize("robot,sites,N,perb,perp,kw", CASES)
def test_host_build_matches_the_restatement_bit_for_bit(exes, tmp_path, robot, sites, N, perb, perp, kw):
    c = _case(robot, sites, N, perb, perp, seed=len(sites) + N, **kw)
    want = _want(c)
    if robot == "panda_sliding_base":
        assert c["links"][0]["joint_type"] == "prismatic"
    if sites == ["link7", "end-effector"]:
        assert c["site_body"] == [7, 7] and not np.allclose(c["site_pos"][1], 0)          # two payloads on one body, one through a weld
        assert (c["payloads"][0, :, 0] == 0).any() and (c["payloads"][:, :, 0] > 0).all(axis=0).any()
    if kw.get("equal_bounds"):
        bl, _, pl, _ = c["bounds"]
        assert np.array_equal(want[1], np.broadcast_to(bl[:, None, :], want[1].shape)) and np.array_equal(want[2], np.broadcast_to(pl[:, None, :], want[2].shape))
    if kw.get("zero_mass"):
        assert np.array_equal(want[0][:, :, 0], c["bodies"][:, :, 0] * c["rows"][:, None, 0])
    for exe in exes:
        got = _run(exe, tmp_path, c)
        for name, w in zip(("rows", "db", "dp", "rows2"), want):
            assert np.array_equal(_bits(got[name]), _bits(w)), (name, np.abs(got[name] - w).max())


def test_columns_do_not_depend_on_the_batch_size(exes, tmp_path):
    """columns 0..69 of B = 70 and of B = 300 are identical, in the host build and in the restatement"""
    out = []
    for N in (70, 300):
        c = _case("panda_arm", ["end-effector", "link4"], N, 0, 0, seed=3)
        got = _run(exes[0], tmp_path, c)
        want = _want(c)
        for name, w in zip(("rows", "db", "dp", "rows2"), want):
            assert np.array_equal(_bits(got[name]), _bits(w)), name
        out.append(got)
    for name in ("rows", "db", "dp", "rows2"):
        assert np.array_equal(_bits(out[0][name]), _bits(out[1][name][:, :70]))
    assert len(np.unique(out[1]["rows2"][6, :, 0])) == 300


# ------------------------------------------------------------------ properties of the restatement
def test_neutral_parts_return_the_models_rows_exactly():
    for robot, sites in (("panda_arm", ["end-effector", "link4"]), ("panda_sliding_base", []), ("chain30", [])):
        c = _case(robot, sites, 6, 0, 0, seed=1, zero_mass=True)
        rows = IR.compose(c["rows"], IR.neutral_bodies(c["n"]), c["payloads"], c["site_body"], c["site_pos"], c["site_rot"], 6)
        assert np.array_equal(_bits(rows), _bits(np.broadcast_to(c["rows"][:, None, :], rows.shape)))
        rows, _, _ = IR.randomized(c["rows"], 5, 0, 6, None, None, c["site_body"], c["site_pos"], c["site_rot"])
        assert np.array_equal(_bits(rows), _bits(np.broadcast_to(c["rows"][:, None, :], rows.shape)))


def test_mass_first_moment_and_inertia_compose_as_rigid_bodies_do():
    N = 200
    c = _case("panda_sliding_base", ["link7", "end-effector"], N, 1, 1, seed=9)
    rows = IR.compose(c["rows"], c["bodies"], c["payloads"], c["site_body"], c["site_pos"], c["site_rot"], N)
    m1 = c["bodies"][:, :, 0] * c["rows"][:, None, 0]
    c1 = c["rows"][:, None, 1:4] + c["bodies"][:, :, 1:4]
    mass, moment = m1.copy(), m1[:, :, None] * c1
    cp = []
    for p in range(c["P"]):
        mp = c["payloads"][p, :, 0]
        cp.append(c["site_pos"][p] + c["payloads"][p, :, 1:4] @ c["site_rot"][p].T)
        mass[c["site_body"][p]] += mp
        moment[c["site_body"][p]] += mp[:, None] * cp[p]
    assert np.array_equal(rows[:, :, 0], mass) or np.abs(rows[:, :, 0] - mass).max() <= 1e-15 * mass.max()
    got = rows[:, :, 0:1] * rows[:, :, 1:4]
    assert np.abs(got - moment).max() <= 1e-15 * max(1.0, np.abs(moment).max())
    # every composed inertia is positive semidefinite, and it is the sum of the parts' inertias about the common COM (in exact terms: here
    # against an independent sum of 3 x 3 matrices)
    lam = np.linalg.eigvalsh(IR.sym(rows[:, :, 4:10]))
    assert (lam >= -1e-15).all() and (lam[c["rows"][:, 0] > 0] > 0).all()
    j = 7
    for i in range(0, N, 17):
        com = rows[j, i, 1:4]
        I = c["bodies"][j, i, 0] * IR.sym(c["rows"][j, 4:10]) + m1[j, i] * IR.sym(IR.parallel_axis((c1[j, i] - com)[None])[0])
        for p in range(2):
            w = c["payloads"][p, i]
            if w[0] > 0:
                R = c["site_rot"][p]
                I = I + R @ IR.box_inertia(w[0], w[4:7]) @ R.T + w[0] * IR.sym(IR.parallel_axis((cp[p][i] - com)[None])[0])
        assert np.abs(IR.sym(rows[j, i, 4:10]) - I).max() <= 1e-14
    # a payload moves the COM towards itself and never lightens the body
    on = (c["payloads"][:, :, 0] > 0).any(axis=0)
    assert (rows[7, on, 0] > m1[7, on]).all() and np.array_equal(rows[7, ~on, 0], m1[7, ~on]) and np.array_equal(rows[:7, :, 0], m1[:7])


def test_the_merged_description_matches_the_composition():
    """instance_description (what the device tests hand to the per-link oracle) and compose agree on the merged bodies to rounding"""
    c = _case("panda_arm", ["end-effector", "link4"], 5, 1, 1, seed=2)
    rows = IR.compose(c["rows"], c["bodies"], c["payloads"], c["site_body"], c["site_pos"], c["site_rot"], 5)
    for i in range(5):
        d = IR.instance_description(dict(name="x", links=c["links"]), c["bodies"][:, i], c["payloads"][:, i], c["payload_links"])
        assert np.abs(IR.model_rows(d["links"]) - rows[:, i]).max() < 1e-14


def test_the_draw_is_bounded_exact_and_reproducible():
    rng = np.random.default_rng(5)
    lo, hi = rng.uniform(-3, 3, (6, 4)), rng.uniform(-3, 3, (6, 4))
    hi[:, ::3] = lo[:, ::3]
    lo[3, 2], hi[3, 2] = -1000.3, 1e-3                                   # a wide interval: the roundings must not leave it
    d = IR.draw(0x123456789ABCDEF, 3, IR.TABLE_BODIES, 500, lo, hi)
    assert d.shape == (6, 500, 4)
    mn, mx = np.minimum(lo, hi)[:, None, :], np.maximum(lo, hi)[:, None, :]
    assert ((d >= mn) & (d <= mx)).all()
    same = np.broadcast_to((lo == hi)[:, None, :], d.shape)
    assert np.array_equal(d[same], np.broadcast_to(lo[:, None, :], d.shape)[same])
    assert np.array_equal(d, IR.draw(0x123456789ABCDEF, 3, IR.TABLE_BODIES, 500, lo, hi))
    for other in (IR.draw(0x123456789ABCDEF, 4, IR.TABLE_BODIES, 500, lo, hi), IR.draw(0x123456789ABCDEE, 3, IR.TABLE_BODIES, 500, lo, hi),
                  IR.draw(0x123456789ABCDEF, 3, IR.TABLE_PAYLOADS, 500, lo, hi)):
        assert (other != d)[~same].mean() > 0.999
    assert np.ptp(d[~same].reshape(-1)) > 1.0 and len(np.unique(d[0, :, 1])) == 500
    # the plant's draw of the same counter under the plant's table ids is another stream
    import plant_ref as PL
    assert (PL.draw(0x123456789ABCDEF, 3, PL.TABLE_JOINTS, 500, lo, hi) != d)[~same].mean() > 0.999
