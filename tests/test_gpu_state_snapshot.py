"""State snapshots (csrc/saip_state_snapshot.hip, saip_batch_snapshot_*): the complete per-instance state saved on the device and
written back through a source index.  Panda, B = 70 at ld = 96 (a full and a partial wavefront plus padding columns).  The stack makes
every kind of segment exist and move: the closed-loop contact stack of config 13 (motion-force + joint task) with the passivity
controller, integral gains on both tasks, internal OTGs on both (acceleration- or jerk-limited), the blended singularity strategies
with every third instance's elbow nearly straight, and sensed-force rows that change every two periods.

A rollout of 6 periods is three calls of two periods, each behind new sensed forces; `src` tells which instance's forces an instance is
given, so that a permuted or broadcast batch is fed what its source instances were fed."""
import ctypes as C

import numpy as np
import pytest

import workloads as W
from test_gpu_batch_layout import _d2h, _h2d, _same_bits

pytestmark = pytest.mark.gpu

B, LD = 70, 96
DT, SUB = 5e-4, 2
CANARY = 6.02214076e23
TOL = 1e-5          # the project's parity tolerance, relative per joint (workloads.torque_error)
MODES = ["acc", "jerk"]


def _q0():
    d = W.make_inputs(13, B)
    q = d["q"].copy()
    q[::3, 3] = -0.07 - 0.28 * np.linspace(0.05, 0.95, len(q[::3]))      # elbow nearly straight: inside the singularity bounds
    return d, q


def _stack(mode):
    from sai_primitives_amd.controller import controller_from_specs
    d, q = _q0()
    spec = W.config_tasks(13)
    spec[0].update(passivity=True, ki_pos=5.0, ki_ori=3.0)
    spec[1].update(ki=2.0)
    robot, ctrl, objs = controller_from_specs(d["model"].name, spec, B, device=0, disable_otg=False)
    mf, jt = objs
    if mode == "jerk":
        mf.enableInternalOtgJerkLimited()
        jt.enableInternalOtgJerkLimited(np.pi / 3, 2 * np.pi, 10 * np.pi)
    robot.setQ(q)
    robot.setDq(0.2 * d["dq"])
    robot.updateModel()
    ctrl.reinitializeTasks()
    g0, g1 = d["goals"]
    mf.setGoalPosition(g0[:, 0:3])
    mf.setGoalOrientation(g0[:, 3:12].reshape(B, 3, 3))
    mf.setGoalForce(g0[:, 24:27])
    mf.setGoalMoment(g0[:, 27:30])
    jt.setGoalPosition(g1[:, 0:7])
    ctrl.updateControllerTaskModels()
    ctrl.recordRollouts(8, channels=("q", "dq", "tau"), summaries=True)
    assert ctrl.devicePointers()["ld"] == LD
    return robot, ctrl, mf, jt


def _forces(seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-6, 6, (3, B, 3)), rng.uniform(-1, 1, (3, B, 3))


def _roll(ctrl, mf, seed, src=None, periods=6):
    f, m = _forces(seed)
    src = np.arange(B) if src is None else np.asarray(src)
    for k in range(periods // 2):
        mf.updateSensedForceAndMoment(f[k][src], m[k][src])
        ctrl.rolloutAsync(2, DT, SUB, gravity=(0.0, 0.0, 0.0))


def _end(ctrl):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    log = ctrl.rolloutLog()
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(np.float64), log_q=log["q"], log_tau=log["tau"],
                summary=ctrl.rolloutSummary())


def _take(end, src):
    """what the run `end` looks like when instance i is instance src[i] of it"""
    return {k: (v[:, src] if k.startswith("log") else v[src]) for k, v in end.items()}


def _columns(snap, blob):
    """{segment name: (B, bytes per instance) uint8}: the bytes of every instance, padding columns left out"""
    raw = np.frombuffer(blob, np.uint8)
    out = {}
    for s in snap.segments():
        rows, eb, g, off = s["rows"], s["elem_bytes"], s["group"], s["offset"]
        if s["kind"] == "soa":
            a = raw[off:off + rows * LD * eb].reshape(rows, LD, eb)[:, :B]
            out[s["name"]] = a.transpose(1, 0, 2).reshape(B, rows * eb)
        elif s["kind"] == "grouped":
            a = raw[off:off + rows * B * g * eb].reshape(rows, B, g * eb)
            out[s["name"]] = a.transpose(1, 0, 2).reshape(B, rows * g * eb)
        else:
            out[s["name"]] = raw[off:off + LD * eb].reshape(LD, eb)[:B]
    return out


MAPS = {"identity": np.arange(B), "permutation": np.random.default_rng(3).permutation(B), "broadcast": np.full(B, 69),
        "repeats": np.random.default_rng(4).integers(0, 7, B)}


@pytest.fixture(scope="module", params=MODES)
def rolled(request):
    """a stack rolled 5 periods (OTGs initialised, integrators, handler and observer state in motion) with a snapshot S of that state"""
    robot, ctrl, mf, jt = _stack(request.param)
    f, m = _forces(1)
    for k in range(5):
        mf.updateSensedForceAndMoment(f[k % 3], m[k % 3])
        ctrl.rolloutAsync(1, DT, SUB, gravity=(0.0, 0.0, 0.0))
    snap = ctrl.saveState()
    return robot, ctrl, mf, jt, snap, snap.tobytes()


def test_directory(rolled):
    robot, ctrl, mf, jt, snap, blob = rolled
    names = [s["name"] for s in snap.segments()]
    want = ["q", "dq", "tau", "status"]
    for t in (0, 1):
        want += [f"task{t}.{n}" for n in ("goal", "integ", "integ_new", "desired", "otg.state", "otg.time", "otg.seen_epoch")]
    want += ["task0.sh", "task0.popc", "task0.otg.frame"]
    assert set(want) <= set(names), sorted(set(want) - set(names))
    assert len(blob) == snap.nbytes()
    kinds = {s["name"]: s["kind"] for s in snap.segments()}
    assert kinds["task0.otg.state"] == "grouped" and kinds["task0.sh"] == "aos" and kinds["q"] == "soa"
    # all zeros, legitimately: the status byte (no instance is refused), the OTG result (ruckig::Working = 0) and seen_epoch (the
    # limits were never changed after the first cycle: epoch 0 ... unless the jerk mode was switched on, which bumps it)
    zero_ok = {"status", "task0.otg.result", "task1.otg.result", "task0.otg.seen_epoch", "task1.otg.seen_epoch"}
    cols = _columns(snap, blob)
    for name, a in cols.items():
        if name not in zero_ok:
            assert a.any(), name
    assert cols["task0.sh"].any(axis=1).sum() >= B // 3 - 2      # the near-singular third has handler state


@pytest.mark.parametrize("which", list(MAPS))
def test_pure_data_movement_is_bitwise(rolled, which):
    robot, ctrl, mf, jt, snap, blob = rolled
    src = MAPS[which]
    _roll(ctrl, mf, 2, periods=2)
    ctrl.rolloutAsync(1, DT, SUB, gravity=(0.0, 0.0, 0.0))           # 3 more periods: every segment has moved on
    ctrl.synchronize()
    p = ctrl.devicePointers()
    goal_ptr = __import__("sai_primitives_amd").lib().saip_batch_device_goal(ctrl._h, mf._id)
    live_q, live_goal = _d2h(p["q"], (7, LD)), _d2h(goal_ptr, (36, LD))
    live_q[:, B:], live_goal[:, B:] = CANARY, -CANARY
    _h2d(p["q"], live_q)
    _h2d(goal_ptr, live_goal)
    ctrl.restoreState(snap, None if which == "identity" else (69 if which == "broadcast" else src))
    s2 = ctrl.saveState()
    a, b = _columns(snap, blob), _columns(s2, s2.tobytes())
    assert a.keys() == b.keys()
    for name in a:
        assert np.array_equal(b[name], a[name][src]), name
    assert (_d2h(p["q"], (7, LD))[:, B:] == CANARY).all() and (_d2h(goal_ptr, (36, LD))[:, B:] == -CANARY).all()
    assert snap.tobytes() == blob                                     # a restore reads the snapshot only
    s2.close()
    ctrl.restoreState(snap)


@pytest.fixture(scope="module", params=MODES)
def run_a(request):
    """save, 6 periods: the end state A of the first run"""
    robot, ctrl, mf, jt = _stack(request.param)
    _roll(ctrl, mf, 5, periods=4)
    snap = ctrl.saveState()
    ctrl.resetRolloutRecorder()
    _roll(ctrl, mf, 6)
    A = _end(ctrl)
    return request.param, ctrl, mf, snap, A


def _same(got, ref):
    for k in ref:
        assert _same_bits(got[k], ref[k]), k


def test_restore_is_deterministic(run_a):
    mode, ctrl, mf, snap, A = run_a
    # control: without the restore the same six periods end elsewhere
    ctrl.resetRolloutRecorder()
    _roll(ctrl, mf, 6)
    other = _end(ctrl)
    assert not _same_bits(other["q"], A["q"]) and not _same_bits(other["tau"], A["tau"])
    ctrl.restoreState(snap)
    ctrl.resetRolloutRecorder()
    _roll(ctrl, mf, 6)
    _same(_end(ctrl), A)


def _worst(got, ref):
    w = 0.0
    for k in ("q", "dq", "tau"):
        w = max(w, W.torque_error(got[k], ref[k]))
    return w


@pytest.mark.parametrize("which", ["permutation", "broadcast"])
def test_permutation_and_broadcast_behave(run_a, which):
    mode, ctrl, mf, snap, A = run_a
    src = MAPS[which]
    ctrl.restoreState(snap, 69 if which == "broadcast" else src)
    ctrl.resetRolloutRecorder()
    _roll(ctrl, mf, 6, src=src)
    got, ref = _end(ctrl), _take(A, src)
    worst = _worst(got, ref)
    print(f"snapshot {which} restore, {mode}: worst relative difference to the source columns {worst:.3e}")
    assert worst <= TOL
    assert np.array_equal(got["status"], ref["status"])


def test_device_map(run_a):
    import torch
    mode, ctrl, mf, snap, A = run_a
    src = MAPS["permutation"].astype(np.int32)
    ctrl.restoreState(snap, src)
    host = ctrl.saveState()
    want = _columns(host, host.tobytes())
    ctrl.restoreState(snap)
    ctrl.synchronize()
    ctrl.restoreState(snap, torch.from_numpy(src).to("cuda:0"))
    ctrl.saveState(host)
    got = _columns(host, host.tobytes())
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    # entries -1 and B leave exactly those instances as they are
    _roll(ctrl, mf, 7, periods=2)
    ctrl.saveState(host)
    before = _columns(host, host.tobytes())
    holes = src.copy()
    holes[[2, 64, 69]] = [-1, B, -1]
    dev = torch.from_numpy(holes).to("cuda:0")
    ctrl.restoreState(snap, dev)
    ctrl.saveState(host)
    after, ref = _columns(host, host.tobytes()), _columns(snap, snap.tobytes())
    keep = np.isin(np.arange(B), [2, 64, 69])
    for name in ref:
        assert np.array_equal(after[name][keep], before[name][keep]), name
        assert np.array_equal(after[name][~keep], ref[name][src[~keep]]), name
    host.close()
    ctrl.restoreState(snap)


def test_blob_round_trip(run_a):
    from sai_primitives_amd import StateSnapshot
    mode, ctrl, mf, snap, A = run_a
    robot2, ctrl2, mf2, jt2 = _stack(mode)
    s2 = StateSnapshot.frombytes(ctrl2, snap.tobytes())
    ctrl2.restoreState(s2)
    _roll(ctrl2, mf2, 6)
    _same(_end(ctrl2), A)


def test_refusals(run_a):
    import sai_primitives_amd as sp
    from sai_primitives_amd import capi
    mode, ctrl, mf, snap, A = run_a
    L = sp.lib()
    ctrl.restoreState(snap)
    ctrl.synchronize()
    before = ctrl.saveState()
    ref = before.tobytes()
    bad = np.arange(B, dtype=np.int32)
    bad[5] = B
    assert L.saip_batch_snapshot_restore(ctrl._h, snap._h, bad.ctypes.data_as(C.POINTER(C.c_int))) == capi.SAIP_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        ctrl.restoreState(snap, bad)
    ctrl.saveState(before)
    assert before.tobytes() == ref                                    # nothing moved
    # a snapshot of another batch
    robot2, ctrl2, mf2, jt2 = _stack(mode)
    other = ctrl2.saveState()
    assert L.saip_batch_snapshot_restore(ctrl._h, other._h, None) != 0 and b"another batch" in L.saip_last_error()
    assert L.saip_batch_snapshot_save(ctrl._h, other._h) != 0
    with pytest.raises(ValueError):
        ctrl.restoreState(other)
    # an internal OTG enabled for the first time after the snapshot was created
    from sai_primitives_amd.controller import controller_from_specs
    d, q = _q0()
    robot3, ctrl3, objs3 = controller_from_specs(d["model"].name, W.config_tasks(13), B, device=0, disable_otg=True)
    robot3.setQ(q)
    robot3.updateModel()
    ctrl3.reinitializeTasks()
    ctrl3.updateControllerTaskModels()
    s3 = ctrl3.saveState()
    assert not any("otg" in s["name"] for s in s3.segments())
    objs3[1].enableInternalOtgAccelerationLimited()
    for fn in (lambda: L.saip_batch_snapshot_save(ctrl3._h, s3._h), lambda: L.saip_batch_snapshot_restore(ctrl3._h, s3._h, None)):
        assert fn() == capi.SAIP_ERR_ORDER
        assert b"task1.desired" in L.saip_last_error()


def test_the_bare_path_is_unchanged():
    """a batch that has a snapshot taken rolls exactly like its twin that never saw one (and runs the same kernel)"""
    ends = []
    for with_snapshot in (False, True):
        robot, ctrl, mf, jt = _stack("acc")
        _roll(ctrl, mf, 5, periods=2)
        if with_snapshot:
            snap = ctrl.saveState()
        _roll(ctrl, mf, 6)
        ends.append((_end(ctrl), ctrl.kernelName()))
    _same(ends[1][0], ends[0][0])
    assert ends[0][1] == ends[1][1]
