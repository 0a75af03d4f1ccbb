"""State snapshots, host side (no GPU needed): the C-ABI entries are declared, exported and bound; a configuration-only and an unfinalized
batch get the documented codes and nothing is written to the outputs; saip_snapshot_import_host refuses a short buffer, a bad magic,
another version and a wrong fingerprint before the device is needed; the indexing of the gather kernel, compiled for the host from the
header the kernel uses, equals a NumPy gather on the three layouts; the Python facade and the C++ example pass their host checks."""
import ctypes as C
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from test_goal_schedule_cpu import _controller_batch
from test_rollout_record_cpu import _robot_file

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "sai-primitives_amd")
STATUS_ENTRIES = ["saip_batch_snapshot_create", "saip_batch_snapshot_save", "saip_batch_snapshot_restore", "saip_batch_snapshot_restore_device",
                  "saip_snapshot_segment_info", "saip_snapshot_export_host", "saip_snapshot_import_host"]
OTHER_ENTRIES = {"saip_snapshot_destroy": None, "saip_snapshot_segments": C.c_int, "saip_snapshot_bytes": C.c_size_t}
HEADER_BYTES = 256


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    return sp


def test_entries_declared_exported_and_bound(sp):
    from sai_primitives_amd import capi
    hdr = open(os.path.join(ROOT, "include", "saip.h")).read()
    assert re.search(r"enum \{ SAIP_SNAPSHOT_SOA = 0, SAIP_SNAPSHOT_GROUPED = 1, SAIP_SNAPSHOT_AOS = 2 \};", hdr)
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    L = sp.lib()
    raw = C.CDLL(os.path.join(PKG, "libsaip.so"))
    for name in STATUS_ENTRIES + list(OTHER_ENTRIES):
        assert re.search(r"\b" + name + r"\s*\(", hdr), name
        assert hasattr(raw, name), name
        assert name in L._declared
        assert getattr(L, name).restype is (C.c_int if name in STATUS_ENTRIES else OTHER_ENTRIES[name])
    assert (capi.SAIP_SNAPSHOT_SOA, capi.SAIP_SNAPSHOT_GROUPED, capi.SAIP_SNAPSHOT_AOS) == (0, 1, 2)
    assert "csrc/saip_state_snapshot.hip" in capi.SOURCES and "csrc/saip_state_snapshot.h" in capi.HEADERS


def _all_refuse(L, b, code):
    """every entry that takes a batch, with otherwise plausible arguments: `code`, and the outputs stay as they were"""
    out = C.c_void_p(0x5a5a)
    assert L.saip_batch_snapshot_create(b, C.byref(out)) == code
    assert out.value == 0x5a5a
    fake = C.c_void_p(0)                       # no snapshot can exist without a device
    src = (C.c_int * 4)(0, 1, 2, 3)
    buf = (C.c_ubyte * 512)(*([7] * 512))
    for st in (L.saip_batch_snapshot_save(b, fake), L.saip_batch_snapshot_restore(b, fake, src), L.saip_batch_snapshot_restore(b, fake, None),
               L.saip_batch_snapshot_restore_device(b, fake, C.c_void_p(64)), L.saip_snapshot_export_host(b, fake, buf, 512)):
        assert st == code
    assert bytes(buf) == bytes([7] * 512)


def test_error_contract_without_a_device(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    ORDER, INVALID, NO_DEVICE = capi.SAIP_ERR_ORDER, capi.SAIP_ERR_INVALID_ARGUMENT, capi.SAIP_ERR_NO_DEVICE
    out = C.c_void_p(0x5a5a)
    assert L.saip_batch_snapshot_create(None, C.byref(out)) == INVALID and out.value == 0x5a5a
    assert L.saip_batch_snapshot_save(None, None) == INVALID and L.saip_batch_snapshot_restore(None, None, None) == INVALID
    assert L.saip_snapshot_import_host(None, None, None, 0) == INVALID and L.saip_snapshot_export_host(None, None, None, 0) == INVALID
    # entries on a snapshot alone
    assert L.saip_snapshot_segments(None) == 0 and L.saip_snapshot_bytes(None) == 0
    L.saip_snapshot_destroy(None)
    rows, name = C.c_int(7), C.c_char_p(b"x")
    assert L.saip_snapshot_segment_info(None, 0, C.byref(name), C.byref(rows), None, None, None, None) == INVALID
    assert (rows.value, name.value) == (7, b"x")
    robot, b = _controller_batch(sp, L, 4)
    try:
        _all_refuse(L, b, ORDER)                                  # before finalize: the call-order error, whatever the arguments
        assert L.saip_snapshot_import_host(b, None, (C.c_ubyte * 8)(), 8) == ORDER
        assert L.saip_batch_finalize(b) == 0
        # finalized, configuration-only: argument errors first, then the missing device
        out = C.c_void_p(0x5a5a)
        assert L.saip_batch_snapshot_create(b, None) == INVALID
        assert L.saip_batch_snapshot_create(b, C.byref(out)) == NO_DEVICE and out.value == 0x5a5a and b"no CPU path" in L.saip_last_error()
        assert L.saip_batch_snapshot_save(b, None) == INVALID and b"null snapshot" in L.saip_last_error()
        assert L.saip_batch_snapshot_restore(b, None, None) == INVALID
        assert L.saip_batch_snapshot_restore_device(b, None, None) == INVALID
        assert L.saip_snapshot_export_host(b, None, None, 0) == INVALID
    finally:
        L.saip_batch_destroy(b)
    # a batch finalized for model queries only
    b = C.c_void_p()
    assert L.saip_batch_create(robot._h, 4, -1, C.byref(b)) == 0
    try:
        assert L.saip_batch_finalize_model_only(b) == 0
        _all_refuse(L, b, ORDER)
        assert b"model queries only" in L.saip_last_error()
    finally:
        L.saip_batch_destroy(b)


def _header(magic=b"SAIPSNAP", version=1, nseg=10, fingerprint=0, total=0, ntasks=2):
    h = struct.pack("<8sIIQQii", magic, version, nseg, fingerprint, total, 0, ntasks) + struct.pack("<16i", *([0] * 16))
    assert len(h) == 104
    return h + bytes(HEADER_BYTES - len(h))


def test_import_refuses_bad_blobs_before_the_device(sp):
    from sai_primitives_amd import capi
    L = sp.lib()
    INVALID = capi.SAIP_ERR_INVALID_ARGUMENT
    robot, b = _controller_batch(sp, L, 4)

    def imp(blob, n=None):
        buf = (C.c_ubyte * max(len(blob), 1)).from_buffer_copy(blob or b"\0")
        return L.saip_snapshot_import_host(b, None, buf, len(blob) if n is None else n)
    try:
        assert L.saip_batch_finalize(b) == 0
        assert L.saip_snapshot_import_host(b, None, None, 1024) == INVALID and b"null buffer" in L.saip_last_error()
        for n in (0, 8, 103, HEADER_BYTES - 1):
            assert imp(_header(), n) == INVALID and b"short buffer" in L.saip_last_error(), n
        assert imp(_header(magic=b"SAIPSNAQ")) == INVALID and b"bad magic" in L.saip_last_error()
        assert imp(bytes(1024)) == INVALID and b"bad magic" in L.saip_last_error()
        assert imp(_header(version=2)) == INVALID and b"version" in L.saip_last_error()
        assert imp(_header(fingerprint=0x1234)) == INVALID and b"wrong fingerprint" in L.saip_last_error()
        # the layout of this batch (its fingerprint is in the message): q, dq, tau, status and goal / integ / integ_new of both tasks
        fp = int(re.search(rb"expected ([0-9a-f]{16})", L.saip_last_error()).group(1), 16)
        ld = L.saip_batch_ld(b)
        sizes = [7 * ld * 8] * 3 + [ld] + [36 * ld * 8, 12 * ld * 8, 12 * ld * 8] + [21 * ld * 8, 7 * ld * 8, 7 * ld * 8]
        total = HEADER_BYTES + sum((s + 255) // 256 * 256 for s in sizes)
        assert imp(_header(fingerprint=fp ^ 1, total=total)) == INVALID and b"wrong fingerprint" in L.saip_last_error()
        assert imp(_header(fingerprint=fp, total=total - 8)) == INVALID and b"inconsistent header" in L.saip_last_error()
        assert imp(_header(fingerprint=fp, total=total, nseg=9)) == INVALID and b"inconsistent header" in L.saip_last_error()
        good = _header(fingerprint=fp, total=total)
        assert imp(good) == INVALID and b"short buffer" in L.saip_last_error()
        assert imp(good + bytes(total - HEADER_BYTES - 1)) == INVALID and b"short buffer" in L.saip_last_error()
        # a well-formed blob of this layout passes every check of the blob and stops at the snapshot (none can exist without a device)
        assert imp(good + bytes(total - HEADER_BYTES)) == INVALID and b"null snapshot" in L.saip_last_error()
    finally:
        L.saip_batch_destroy(b)


# ------------------------------------------------------------------ the kernel's indexing, compiled for the host
@pytest.fixture(scope="module")
def gather(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gather") / "libstate_gather_host.so")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tests", "cpp", "state_gather_host.cpp")])
    fn = C.CDLL(so).saip_test_gather_segment
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    return fn


B, LD, GS, REC = 5, 32, 8, 488
# (kind, array shape in elements, dtype, row_stride in words, rows, words per instance, word bytes)
LAYOUTS = {
    "soa_f64": ((11, LD), np.float64, LD, 11, 1, 8),
    "soa_i32": ((1, LD), np.int32, LD, 1, 1, 4),
    "soa_u8": ((3, LD), np.uint8, LD, 3, 1, 1),
    "grouped": ((19, B * GS), np.float64, B * GS, 19, GS, 8),
    "aos": ((LD, REC), np.uint8, 0, 1, REC // 8, 8),
}
SOURCES = {"identity": None, "permutation": [3, 0, 4, 1, 2], "broadcast": [4] * 5, "repeats": [1, 1, 0, 3, 3], "holes": [2, -1, 5, 0, -7]}


def _per_instance(name, a):
    """(B, ...) view of the words each instance owns"""
    if name.startswith("soa"):
        return a[:, :B].T
    if name == "grouped":
        return a.reshape(a.shape[0], B, GS).transpose(1, 0, 2)
    return a[:B]


@pytest.mark.parametrize("src", list(SOURCES))
@pytest.mark.parametrize("name", list(LAYOUTS))
def test_gather_indexing_equals_numpy(gather, name, src):
    shape, dtype, stride, rows, wpi, wb = LAYOUTS[name]
    rng = np.random.default_rng(len(name) * 31 + len(src))
    snap = rng.integers(0, 200, shape).astype(dtype)
    live = rng.integers(0, 200, shape).astype(dtype)
    live0 = live.copy()
    m = SOURCES[src]
    mp = None if m is None else np.asarray(m, np.int32)
    units = gather(live.ctypes.data, snap.ctypes.data, stride, rows, wpi, wb, B, None if mp is None else mp.ctypes.data, 0)
    assert units == -(-B * wpi // 256) * -(-rows // 8)
    want = live0.copy()
    w, s0 = _per_instance(name, want), _per_instance(name, snap)
    for i in range(B):
        j = i if m is None else m[i]
        if 0 <= j < B:
            w[i] = s0[j]
    assert np.array_equal(live, want)
    if name != "grouped":                                             # the padding columns / records B .. ld-1 are never written
        pad = live[:, B:] if name.startswith("soa") else live[B:]
        assert np.array_equal(pad, live0[:, B:] if name.startswith("soa") else live0[B:])
    # save: the snapshot's columns 0 .. B-1 become the live ones, whatever the map
    snap2 = snap.copy()
    gather(live.ctypes.data, snap2.ctypes.data, stride, rows, wpi, wb, B, None if mp is None else mp.ctypes.data, 1)
    assert np.array_equal(_per_instance(name, snap2), _per_instance(name, live))
    if name != "grouped":
        assert np.array_equal(snap2[:, B:] if name.startswith("soa") else snap2[B:], snap[:, B:] if name.startswith("soa") else snap[B:])


def test_python_facade_without_a_device(sp):
    robot = sp.SaiModel("panda_arm", 4, device=-1)
    ctrl = sp.RobotController(robot, [sp.MotionForceTask(robot, "end-effector", (0, 0, 0.07)), sp.JointTask(robot)])
    with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
        ctrl.saveState()
    with pytest.raises(sp.SaipNoDevice, match="no CPU path"):
        sp.StateSnapshot(ctrl)
    with pytest.raises(ValueError, match="another controller"):
        ctrl.restoreState(None)
    with pytest.raises(sp.SaipNoDevice):                              # frombytes creates the snapshot first
        sp.StateSnapshot.frombytes(ctrl, bytes(1024))
    with pytest.raises(ValueError, match="bad magic"):
        ctrl._call("saip_snapshot_import_host", None, (C.c_ubyte * 1024)(), 1024)
