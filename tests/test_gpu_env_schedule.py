"""Environment schedules on the device (csrc/saip_env_schedule.hip, the MOVING instantiations of the contact kernels,
saip_batch_env_schedule_*).  Oracles: the NumPy restatement tests/env_schedule_ref.py for every table and velocity word and for the
moving-surface force; for whole rollouts a twin controller WITHOUT a schedule whose table is uploaded with set_*_host in front of every
single-period rollout -- the code path as it was before schedules existed.

Batches (B, ld) in {(3, 64), (65, 128), (130, 192)}; every rollout is 6 periods of 2 substeps unless a test says otherwise.  The padding
columns of every table are pre-filled with a sentinel that must survive."""
import numpy as np
import pytest

import contact_patch_ref as CP
import contact_ref as CR
import env_schedule_ref as ES
from test_gpu_batch_layout import _d2h, _h2d, _same_bits
from test_gpu_clearance import _query_centres
from test_gpu_contact import _cfg13, _table_under
from test_gpu_contact_patch import EE, EE_POS, SQUARE, _dual, _floor
from test_gpu_rollout_record import _panda

pytestmark = pytest.mark.gpu

SHAPES = [(3, 64), (65, 128), (130, 192)]          # (B, leading dimension)
SENTINEL = 6.02214076e23
DT, SUB, PERIODS = 5e-4, 2, 6
T = DT * SUB
ZERO_G = (0.0, 0.0, 0.0)
MODES = {"hold": ES.HOLD, "linear": ES.LINEAR}
SPHERES = [("link4", (0.0, 0.0, 0.0), 0.06), ("link5", (0.0, 0.02, -0.1), 0.05), ("link6", (0.0, 0.0, 0.0), 0.05), ("link7", (0.0, 0.0, 0.05), 0.04),
           ("end-effector", (0.0, 0.0, 0.03), 0.04)]


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _lib():
    from sai_primitives_amd import capi
    return capi.lib()


# ------------------------------------------------------------------ keyframes (device layout: (K, n, W[, B]); the facade takes (K, n[, B], W))
def _facade(key):
    return key.transpose(0, 1, 3, 2) if key.ndim == 4 else key


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _obstacle_keys(rng, K, base, B):
    """K keyframes around the obstacle rows `base` (n, 8): capsules drift, half-spaces tilt a little and shift; (K, n, 8) or (K, n, 8, B)"""
    cols = B if B else 1
    n = base.shape[0]
    key = np.repeat(np.repeat(base[None, :, :, None], K, axis=0), cols, axis=3).astype(float)
    for k in range(1, K):
        step = rng.uniform(-0.03, 0.03, (n, 8, cols))
        step[:, 0] = 0.0
        key[k] = key[k - 1] + step
        key[k, :, 7] = np.abs(key[k, :, 7])
    hs = base[:, 0] == 1.0
    nrm = _unit(key[:, hs, 1:4].transpose(0, 1, 3, 2))                       # a half-space normal is unit in every keyframe
    key[:, hs, 1:4] = nrm.transpose(0, 1, 3, 2)
    return key if B else key[..., 0]


def _plane_keys(rng, K, base, B, u_scale=0.05, tilt=0.05):
    """K raw keyframes around the plane rows `base` (n, 8[, B]): offsets move, normals tilt (not normalised: the engine does that), u random;
    (K, n, 12) or (K, n, 12, B)"""
    cols = B if B else 1
    base = base if base.ndim == 3 else np.repeat(base[:, :, None], cols, axis=2)
    n = base.shape[0]
    key = np.zeros((K, n, 12, cols))
    key[:, :, :8] = base[None]
    for k in range(1, K):
        key[k, :, 0:3] = key[k - 1, :, 0:3] + tilt * rng.normal(size=(n, 3, cols))
        key[k, :, 3] = key[k - 1, :, 3] + rng.uniform(-2e-3, 2e-3, (n, cols))
    key[:, :, 8:11] = u_scale * rng.normal(size=(K, n, 3, cols))
    return key if B else key[..., 0]


class _Table:
    """a resident table [items][W][ld] or [items][W]: padding columns pre-filled with a sentinel, reads check that it survived"""

    def __init__(self, ctrl, ptr, items, W, ld, per):
        assert ptr
        ctrl.synchronize()
        self.ctrl, self.ptr, self.B, self.per = ctrl, ptr, ctrl.batch_size, per
        self.shape = (items, W, ld) if per else (items, W)
        if per:
            a = _d2h(ptr, self.shape)
            a[:, :, self.B:] = SENTINEL
            _h2d(ptr, a)

    def get(self):
        self.ctrl.synchronize()
        a = _d2h(self.ptr, self.shape)
        if self.per:
            assert (a[:, :, self.B:] == SENTINEL).all()                        # columns B..ld-1 are never written
            return a[:, :, :self.B]
        return a

    def put_rows(self, rows, value):
        """fill whole items with a marker (what an unscheduled item must keep)"""
        self.ctrl.synchronize()
        a = _d2h(self.ptr, self.shape)
        a[rows] = np.where(a[rows] == SENTINEL, SENTINEL, value)
        _h2d(self.ptr, a)


# ------------------------------------------------------------------ 1. tables and velocities, bit for bit
def _check_tables(ctrl, scheds, periods):
    """scheds: [(table, velocity table or None, device-layout keyframes as the engine keeps them, planes, first, stride, mode, frozen rows)]"""
    seen = set()
    for c in range(periods):
        ctrl.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
        for tab, vel, key, planes, first, stride, mode, frozen in scheds:
            x = ES.period_index(c, planes)
            rt, rv = ES.rows(key, planes, x, stride, mode, T)
            n = key.shape[1]
            got = tab.get()
            assert _same_bits(np.ascontiguousarray(got[first:first + n]), np.ascontiguousarray(rt)), (c, planes)
            for rows, want in frozen:
                assert _same_bits(np.ascontiguousarray(got[rows]), want), ("unscheduled item", c, rows)
            if planes:
                gv = vel.get()
                assert _same_bits(np.ascontiguousarray(gv[first:first + n]), np.ascontiguousarray(rv)), (c, "velocity")
                rest = np.delete(gv, np.s_[first:first + n], axis=0)
                assert (rest == 0.125).all()                                    # the velocity rows of unscheduled planes are never written
            seen.add((planes,) + ES.timing(x, key.shape[0], stride, mode)[1:])
    return seen


@pytest.mark.parametrize("mode", ["hold", "linear"])
@pytest.mark.parametrize("B,ld", SHAPES)
def test_tables_match_the_restatement(sp, B, ld, mode):
    """Panda, config 2's stack: per-instance obstacles (items 1..2 of 3 scheduled) and batch-uniform planes (items 0..1 of 3) for B = 65, the
    layouts swapped otherwise; 8 single-period rollouts over K = 3 keyframes of stride 3"""
    rng = np.random.default_rng(B)
    robot, ctrl, objs, mf, _ = _panda(B, False, ld=ld)
    per_o, per_p = (B == 65), (B != 65)
    cloud = _query_centres(robot, SPHERES)
    z = cloud[:, 4, 2].min() - 0.3
    obst = np.array([[0, 0.3, 0.0, 0.9, 0.5, 0.0, 0.9, 0.02], [1, 0.0, 0.0, 1.0, z, 0, 0, 0], [0, 0.6, 0.1, 0.4, 0.6, 0.1, 0.4, 0.05]])
    ctrl.attachClearance(SPHERES, np.repeat(obst[:, None], B, axis=1) if per_o else obst, margin=0.05, per_instance=per_o)
    planes = np.array([CR.plane([0, 0, 1.0], z, 2e4, 400.0, 0.3), CR.plane([0.1, 0, 1.0], z - 0.1, 1e4, 10.0, 0.5), CR.plane([0, 1.0, 0.0], -5.0, 1e3)])
    mf.attachContactPlanes(np.repeat(planes[:, None], B, axis=1) if per_p else planes, sensor=False, per_instance=per_p)
    K, stride = 3, 3
    ko = _obstacle_keys(rng, K, obst[1:3], B if per_o else 0)
    kp = _plane_keys(rng, K, planes[0:2], B if per_p else 0)
    ctrl.setObstacleSchedule(_facade(ko), stride=stride, mode=mode, first=1)
    mf.setContactSchedule(_facade(kp), stride=stride, mode=mode, first=0)
    info = ctrl.obstacleScheduleInfo()
    assert (info["first"], info["n_items"], info["n_keyframes"], info["stride"], info["mode"], info["per_instance"], info["period"]) == (1, 2, K, stride, mode, per_o, 0)
    assert mf.contactScheduleInfo()["n_items"] == 2 and mf.contactScheduleInfo()["per_instance"] == per_p
    L = _lib()
    to = _Table(ctrl, L.saip_batch_clearance_obstacles_device(ctrl._h), 3, 8, ld, per_o)
    tp = _Table(ctrl, mf.contactPlanesDevice(), 3, 8, ld, per_p)
    tv = _Table(ctrl, mf.contactVelocityDevice(), 3, 4, ld, per_p)
    tv.put_rows(np.s_[2:3], 0.125)
    frozen_o = [(np.s_[0:1], np.ascontiguousarray(to.get()[0:1]))]
    frozen_p = [(np.s_[2:3], np.ascontiguousarray(tp.get()[2:3]))]
    kp_kept = ES.normalise_plane_keys(kp)
    # the resident keyframes are the normalised ones
    kd = _d2h(L.saip_batch_env_schedule_keyframes_device(ctrl._h, ES.TARGET_PLANES, -1), (K, 2, 12, ld) if per_p else (K, 2, 12))
    assert _same_bits(np.ascontiguousarray(kd[..., :B] if per_p else kd), np.ascontiguousarray(kp_kept))
    seen = _check_tables(ctrl, [(to, None, ko, 0, 1, stride, MODES[mode], frozen_o), (tp, tv, kp_kept, 1, 0, stride, MODES[mode], frozen_p)], (K - 1) * stride + 2)
    if mode == "linear":
        assert (1, 0.0, True) in seen and (1, 0.0, False) in seen and any(p == 1 and 0 < s < 1 for p, s, _ in seen) and any(p == 0 and 0 < s < 1 for p, s, _ in seen)
    assert ctrl.obstacleScheduleInfo()["period"] == (K - 1) * stride + 2
    assert np.isfinite(ctrl.pullState()[0]).all()


@pytest.mark.parametrize("mode", ["hold", "linear"])
def test_tables_of_three_schedules_in_one_launch(sp, mode):
    """the dual-arm tree at B = 9 with a patch per arm: two plane schedules and one obstacle schedule, written by one launch per period"""
    B, ld = 9, 64
    rng = np.random.default_rng(4)
    robot, ctrl, objs, n = _dual(B, ld, False)
    mfs = objs[:2]
    specs = [(mfs[0], "left_link7", (0, 0, 0.1), SQUARE, True), (mfs[1], "right_link7", (0, 0, 0.1), np.vstack([SQUARE, 0.5 * SQUARE]), False)]
    K, stride = 2, 3
    scheds = []
    for mf, link, pos, pts, per in specs:
        fl = _floor(robot, link, pos, pts, -0.05)                                # (1, B, 8), 5 cm under the lowest point
        two = np.concatenate([fl, fl], axis=0)
        two[1, :, 3] -= 0.1
        base = two.transpose(0, 2, 1) if per else two[:, 0]
        mf.attachContactPatch(pts, two if per else two[:, 0], sensor=False, per_instance=per)
        kp = _plane_keys(rng, K, base[1:2], B if per else 0)
        mf.setContactSchedule(_facade(kp), stride=stride, mode=mode, first=1)
        tp = _Table(ctrl, mf.contactPatchPlanesDevice(), 2, 8, ld, per)
        tv = _Table(ctrl, mf.contactVelocityDevice(), 2, 4, ld, per)
        tv.put_rows(np.s_[0:1], 0.125)
        scheds.append((tp, tv, ES.normalise_plane_keys(kp), 1, 1, stride, MODES[mode], [(np.s_[0:1], np.ascontiguousarray(tp.get()[0:1]))]))
    sph = [("left_link7", (0, 0, 0.05), 0.05), ("right_link7", (0, 0, 0.05), 0.05), ("left_link4", (0, 0, 0), 0.06)]
    obst = np.array([[1, 0.0, 0.0, 1.0, -2.0, 0, 0, 0], [0, 0.5, 0.0, 0.5, 0.5, 0.2, 0.5, 0.03]])
    ctrl.attachClearance(sph, np.repeat(obst[:, None], B, axis=1), margin=0.05, per_instance=True)
    ko = _obstacle_keys(rng, K, obst, B)
    ctrl.setObstacleSchedule(_facade(ko), stride=stride, mode=mode)
    to = _Table(ctrl, _lib().saip_batch_clearance_obstacles_device(ctrl._h), 2, 8, ld, True)
    scheds.append((to, None, ko, 0, 0, stride, MODES[mode], []))
    _check_tables(ctrl, scheds, (K - 1) * stride + 2)
    assert mfs[0].contactScheduleInfo()["per_instance"] and not mfs[1].contactScheduleInfo()["per_instance"]
    ctrl.clearEnvironmentSchedules()
    assert mfs[0].contactVelocityDevice() is None and mfs[1].contactVelocityDevice() is None


# ------------------------------------------------------------------ 2. clearance against the unscheduled code path
def _monitored(B, ld, per, rng):
    robot, ctrl, objs, mf, _ = _panda(B, False, ld=ld)
    z = _query_centres(robot, SPHERES)[:, 4, 2] - 0.04
    obst = np.array([[1, 0.0, 0.0, 1.0, np.quantile(z, 0.2), 0, 0, 0], [0, 0.3, 0.0, 0.9, 0.5, 0.0, 0.9, 0.02]])
    ctrl.attachClearance(SPHERES, np.repeat(obst[:, None], B, axis=1) if per else obst, pairs=[(0, 4)], margin=0.05, per_instance=per)
    ctrl.recordRollouts(PERIODS, 1, ("q", "tau"), task=mf, summaries=True)
    return robot, ctrl, mf, obst


def _clearance_end(ctrl):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    log = ctrl.rolloutLog()
    s, r = ctrl.clearanceSummary(), ctrl.clearanceReadout()
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), log_q=log["q"], log_tau=log["tau"], log_status=log["status"].astype(float),
                rsum=ctrl.rolloutSummary(), summary=np.column_stack([s[k] for k in ("min_distance", "penalty", "periods_in_collision", "first_collision")]).astype(float),
                readout=np.column_stack([r["distance"], r["item"], r["penalty"], r["under_margin"], r["point"], r["pair_distance"]]).astype(float))


@pytest.mark.parametrize("mode", ["hold", "linear"])
@pytest.mark.parametrize("B,ld,per", [(3, 64, True), (65, 128, False), (130, 192, True), (65, 128, True), (3, 64, False)])
def test_clearance_rollout_equals_the_twin_with_uploaded_obstacles(sp, B, ld, per, mode):
    K, stride = 3, 2
    robot, ctrl, mf, obst = _monitored(B, ld, per, None)
    ko = _obstacle_keys(np.random.default_rng(7), K, obst, B if per else 0)
    ctrl.setObstacleSchedule(_facade(ko), stride=stride, mode=mode)
    ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
    a = _clearance_end(ctrl)
    robot2, ctrl2, mf2, _ = _monitored(B, ld, per, None)
    for c in range(PERIODS):
        rows = ES.rows(ko, 0, c + 1, stride, MODES[mode], T)[0]                  # the obstacles at the time of the state the monitor looks at
        ctrl2.setClearanceObstacles(rows.transpose(0, 2, 1) if per else rows)
        ctrl2.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
    b = _clearance_end(ctrl2)
    for key in a:
        assert _same_bits(np.asarray(a[key]), np.asarray(b[key])), key
    assert (a["summary"][:, 0] < 0.05).any() and np.isfinite(a["q"]).all()
    # the schedule mattered: the obstacles as attached give other summaries
    robot3, ctrl3, mf3, _ = _monitored(B, ld, per, None)
    ctrl3.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
    c3 = _clearance_end(ctrl3)
    assert not _same_bits(a["summary"], c3["summary"]) and _same_bits(a["q"], c3["q"]) and _same_bits(a["log_tau"], c3["log_tau"])


# ------------------------------------------------------------------ 3. contact against the static kernels
def _contact_case(B, ld, patch):
    robot, ctrl, objs = _cfg13(B, ld, False)
    mf = objs[0]
    if patch:
        planes = _floor(robot, EE, EE_POS, SQUARE, 2e-3)
        mf.attachContactPatch(SQUARE, planes, sensor=True, per_instance=True)
    else:
        planes = _table_under(robot, objs, 2e-3)
        mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    ctrl.recordRollouts(PERIODS, 1, ("q", "tau"), task=mf, summaries=True)
    return robot, ctrl, objs, mf, planes


def _contact_end(ctrl, objs, mf, patch):
    ctrl.synchronize()
    q, dq = ctrl.pullState()
    log = ctrl.rolloutLog()
    ro, sm = (mf.contactPatchReadout(), mf.contactPatchSummary()) if patch else (mf.contactReadout(), mf.contactSummary())
    B = ctrl.batch_size
    return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float), log_q=log["q"], log_tau=log["tau"],
                rsum=ctrl.rolloutSummary(), goal=mf._get_goal(), summary=np.column_stack([np.asarray(v, float) for v in sm.values()]),
                readout=np.column_stack([np.asarray(v, float).reshape(B, -1) for v in ro.values()]))


@pytest.mark.parametrize("patch,B,ld", [(False, 3, 64), (False, 65, 128), (True, 130, 192), (True, 65, 128), (False, 130, 192), (True, 3, 64)])
def test_contact_rollout_equals_the_twin_with_uploaded_planes(sp, patch, B, ld):
    """HOLD, u = 0, keyframes that differ: v_p is exactly zero, so the MOVING instantiation must give the bits of the static kernel the
    twin runs"""
    K, stride = 3, 2
    robot, ctrl, objs, mf, planes = _contact_case(B, ld, patch)
    key = np.zeros((K, 1, 12, B))
    key[:, 0, :8] = planes[0].T[None]
    key[:, 0, 3] += np.array([0.0, 1.5e-3, -1.0e-3])[:, None]                     # the table rises into the tool, then recedes
    key[1, 0, 6] = 0.6
    mf.setContactSchedule(_facade(key), stride=stride, mode="hold")
    ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
    a = _contact_end(ctrl, objs, mf, patch)
    vel = _d2h(mf.contactVelocityDevice(), (1, 4, ld))
    assert not vel.any()                                                          # +0 in every word
    robot2, ctrl2, objs2, mf2, _ = _contact_case(B, ld, patch)
    for c in range(PERIODS):
        rows = ES.rows(key, 1, c, stride, ES.HOLD, T)[0]                          # the planes of period c, held through its substeps
        (mf2.setContactPatchPlanes if patch else mf2.setContactPlanes)(rows.transpose(0, 2, 1))
        ctrl2.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
    b = _contact_end(ctrl2, objs2, mf2, patch)
    for k in a:
        assert _same_bits(np.asarray(a[k]), np.asarray(b[k])), k
    assert (a["summary"][:, 3] >= 1).all() and np.isfinite(a["q"]).all() and np.abs(a["goal"][:, 30:33]).max() > 1.0
    robot3, ctrl3, objs3, mf3, _ = _contact_case(B, ld, patch)                    # ... and the keyframes mattered
    ctrl3.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
    assert not _same_bits(a["q"], _contact_end(ctrl3, objs3, mf3, patch)["q"])


def test_a_scheduled_patch_next_to_a_static_one(sp):
    """the dual-arm tree, a patch per arm, a schedule on the SECOND patch only: inside the MOVING launch the first patch keeps the static
    arithmetic; HOLD and u = 0 again, so the twin with uploaded planes is the yardstick for both"""
    B, ld, K, stride = 9, 64, 3, 2
    ends = []
    for scheduled in (True, False):
        robot, ctrl, objs, n = _dual(B, ld, False)
        mfs = objs[:2]
        specs = [(mfs[0], "left_link7", (0, 0, 0.1), SQUARE), (mfs[1], "right_link7", (0, 0, 0.1), np.vstack([SQUARE, 0.5 * SQUARE]))]
        for mf, link, pos, pts in specs:
            fl = _floor(robot, link, pos, pts, 2e-3)
            mf.attachContactPatch(pts, fl, sensor=True, per_instance=True)
        key = np.zeros((K, 1, 12, B))
        key[:, 0, :8] = fl[0].T[None]
        key[:, 0, 3] += np.array([0.0, 1.0e-3, -1.0e-3])[:, None]
        if scheduled:
            mfs[1].setContactSchedule(_facade(key), stride=stride, mode="hold")
            ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
            assert mfs[1].contactVelocityDevice() and mfs[0].contactVelocityDevice() is None
        else:
            for c in range(PERIODS):
                mfs[1].setContactPatchPlanes(ES.rows(key, 1, c, stride, ES.HOLD, T)[0].transpose(0, 2, 1))
                ctrl.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
        ctrl.synchronize()
        q, dq = ctrl.pullState()
        out = dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), status=ctrl.status.astype(float))
        for i, mf in enumerate(mfs):
            out[f"readout{i}"] = np.column_stack([np.asarray(v, float).reshape(B, -1) for v in mf.contactPatchReadout().values()])
            out[f"summary{i}"] = np.column_stack([np.asarray(v, float) for v in mf.contactPatchSummary().values()])
        ends.append(out)
    for k in ends[0]:
        assert _same_bits(ends[0][k], ends[1][k]), k
    assert (ends[0]["summary0"][:, 3] >= 1).all() and (ends[0]["summary1"][:, 3] >= 1).all() and np.isfinite(ends[0]["q"]).all()


# ------------------------------------------------------------------ 4. the moving-surface force, bit for bit
@pytest.mark.parametrize("B,ld", SHAPES)
def test_moving_surface_force_single_point(sp, B, ld):
    """dq = 0, LINEAR with a rising offset and a belt velocity u, one period of one substep: the readout's force is ct_plane_forces_moving
    at the readout's own point with v = 0, against the table and velocity rows the schedule wrote"""
    robot, ctrl, objs = _cfg13(B, ld, False)
    mf = objs[0]
    planes = _table_under(robot, objs, 2e-3, c=150.0, mu=0.4)
    far = planes.copy()
    far[0, :, 3] -= 1.0                                                           # a second plane that never acts
    mf.attachContactPlanes(np.concatenate([planes, far]), sensor=True, per_instance=True)
    key = np.zeros((2, 2, 12, B))
    key[:, :, :8] = np.concatenate([planes, far]).transpose(0, 2, 1)[None]
    key[1, 0, 3] += 4e-4                                                          # rises 0.4 mm over two periods: w_n = 0.4 m/s at T = 0.5 ms
    key[:, 0, 8:11] = np.array([0.03, 0.0, 0.0])[None, :, None]
    key[:, 0, 8] += np.linspace(0.0, 0.01, B)[None, :]
    mf.setContactSchedule(_facade(key), stride=2, mode="linear")
    ctrl.rolloutAsync(1, DT, 1, gravity=ZERO_G)
    ro = mf.contactReadout()
    rt, rv = ES.rows(key, 1, 0, 2, ES.LINEAR, DT * 1)
    tab = _d2h(mf.contactPlanesDevice(), (2, 8, ld))[:, :, :B]
    vel = _d2h(mf.contactVelocityDevice(), (2, 4, ld))[:, :, :B]
    assert _same_bits(np.ascontiguousarray(tab), np.ascontiguousarray(rt)) and _same_bits(np.ascontiguousarray(vel), np.ascontiguousarray(rv))
    assert np.array_equal(rv[0, 3], (key[1, 0, 3] - key[0, 0, 3]) / (2.0 * DT)) and (rv[0, 3] > 0.3).all()
    f, fn_sum, dmin, active = ES.plane_forces_moving(rt.transpose(2, 0, 1), rv.transpose(2, 0, 1), ro["point"], np.zeros((B, 3)))
    assert _same_bits(ro["force"], f) and _same_bits(ro["distance"], dmin) and np.array_equal(ro["active"], active) and (active == 1).all()
    # a pressed point at rest on a belt that runs along +x is dragged along +x; the rising table is damped as if the point sank into it
    assert (f[:, 0] > 0).all() and not f[:, 1].any()
    static = CR.plane_forces(rt.transpose(2, 0, 1), ro["point"], np.zeros((B, 3)))[0]
    assert not static[:, :2].any() and (f[:, 2] > static[:, 2] + 50.0).all()      # c w_n = 150 x 0.4 = 60 N more than the static planes give
    assert (mf.contactSummary()["substeps_in_contact"] == 1).all()


@pytest.mark.parametrize("B,ld", SHAPES)
def test_moving_surface_force_patch(sp, B, ld):
    """the same for an eight-point patch.  The patch readout carries the per-slot normal forces but not the points, so the net force is
    rebuilt, bit for bit, from them: with one plane f_i = fn_i n + f_t(fn_i, v_r = 0 - v_p) has no other input, and F is the eight-lane fold"""
    pts = np.vstack([SQUARE, 0.5 * SQUARE])
    robot, ctrl, objs = _cfg13(B, ld, False)
    mf = objs[0]
    planes = _floor(robot, EE, EE_POS, pts, 2e-3, c=150.0, mu=0.4)
    mf.attachContactPatch(pts, planes, sensor=True, per_instance=True)
    key = np.zeros((2, 1, 12, B))
    key[:, 0, :8] = planes[0].T[None]
    key[1, 0, 3] += 4e-4
    key[:, 0, 8:11] = np.array([0.02, -0.03, 0.0])[None, :, None]
    mf.setContactSchedule(_facade(key), stride=2, mode="linear")
    ctrl.rolloutAsync(1, DT, 1, gravity=ZERO_G)
    ro = mf.contactPatchReadout()
    rt, rv = ES.rows(key, 1, 0, 2, ES.LINEAR, DT * 1)
    vel = _d2h(mf.contactVelocityDevice(), (1, 4, ld))[:, :, :B]
    assert _same_bits(np.ascontiguousarray(vel), np.ascontiguousarray(rv))
    w, vp = rt[0].T, rv[0].T                                                      # (B, 8), (B, 4)
    n, mu, vs = w[:, 0:3], w[:, 6], w[:, 7]
    fn = ro["normal_forces"]                                                      # (B, 8)
    vr = np.zeros((B, 3)) - vp[:, 0:3]
    vn = CR.dot(n, vr)
    vt = vr - vn[:, None] * n
    s = np.maximum(np.sqrt(CR.dot(vt, vt)), vs)
    f = np.zeros((B, 8, 3))
    for i in range(8):
        g = mu * fn[:, i]
        ft = -(g[:, None] * vt) / s[:, None]
        f[:, i] = np.where((fn[:, i] > 0)[:, None], np.zeros((B, 3)) + (fn[:, i, None] * n + ft), 0.0)
    F = CP.fold_sum(f.transpose(0, 2, 1))
    assert (ro["n_touch"] >= 1).all() and (fn > 0).sum() >= B
    assert _same_bits(ro["force"], F)
    assert (F[:, 0] > 0).all() and (F[:, 1] < 0).all()                            # dragged along +u
    # the normal forces carry the damping against the rising table: c w_n = 60 N per touching point over the static k d <= 2e4 x 2e-3 = 40 N
    assert (fn[fn > 0] > 55.0).all()


# ------------------------------------------------------------------ 5. behaviour
def test_a_rising_table_reaches_the_tool_or_stops_short(sp):
    B, ld = 65, 128
    robot, ctrl, objs = _cfg13(B, ld, False)
    mf = objs[0]
    under = _table_under(robot, objs, 0.0, k=5e3, c=10.0, mu=0.2)                 # the plane through the tool point
    even = np.arange(B) % 2 == 0
    start = under.copy()
    start[0, :, 3] -= np.where(even, 0.01, 0.03)
    mf.attachContactPlanes(start, sensor=True, per_instance=True)
    key = np.zeros((2, 1, 12, B))
    key[:, 0, :8] = start[0].T[None]
    key[1, 0, 3] += 0.02                                                          # 2 cm over 4 periods: through the point, or to 1 cm under it
    mf.setContactSchedule(_facade(key), stride=4, mode="linear")
    ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
    ctrl.synchronize()
    sm = mf.contactSummary()
    print("substeps in contact, even / odd:", sorted(set(sm["substeps_in_contact"][even])), sorted(set(sm["substeps_in_contact"][~even])))
    assert (sm["substeps_in_contact"][even] > 0).all() and (sm["substeps_in_contact"][~even] == 0).all()
    q, dq = ctrl.pullState()
    assert np.isfinite(q).all() and np.isfinite(dq).all() and np.isfinite(ctrl.getTorques()).all() and np.isfinite(sm["max_force"]).all()
    assert not ctrl.status.any()


# ------------------------------------------------------------------ 6. rewind to any period
def test_rewind_to_a_period_replays_the_tail(sp):
    B, ld, p = 65, 128, 2
    robot, ctrl, objs = _cfg13(B, ld, False)
    mf = objs[0]
    planes = _table_under(robot, objs, 2e-3)
    mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    key = _plane_keys(np.random.default_rng(1), 3, planes.transpose(0, 2, 1), B, tilt=0.01)
    mf.setContactSchedule(_facade(key), stride=2, mode="linear")
    ctrl.rolloutAsync(p, DT, SUB, gravity=ZERO_G)
    snap = ctrl.saveState()
    assert mf.contactScheduleInfo()["period"] == p
    ctrl.rolloutAsync(PERIODS - p, DT, SUB, gravity=ZERO_G)

    def end():
        ctrl.synchronize()
        q, dq = ctrl.pullState()
        return dict(q=q.copy(), dq=dq.copy(), tau=ctrl.getTorques(), goal=mf._get_goal(), force=mf.contactReadout()["force"],
                    planes=_d2h(mf.contactPlanesDevice(), (1, 8, ld)), vel=_d2h(mf.contactVelocityDevice(), (1, 4, ld)))

    a = end()
    ctrl.restoreState(snap)
    ctrl.rewindEnvironment(p)                                                     # what goes with the restore: tables are not state
    ctrl.rolloutAsync(PERIODS - p, DT, SUB, gravity=ZERO_G)
    b = end()
    for k in a:
        assert _same_bits(a[k], b[k]), k
    ctrl.restoreState(snap)
    ctrl.rewindEnvironment(0)                                                     # another period gives another tail
    ctrl.rolloutAsync(PERIODS - p, DT, SUB, gravity=ZERO_G)
    c = end()
    assert not _same_bits(a["planes"], c["planes"]) and not _same_bits(a["q"], c["q"])
    assert mf.contactScheduleInfo()["period"] == PERIODS - p


# ------------------------------------------------------------------ 7. rules and refusals
def test_rules_and_refusals(sp):
    B, ld = 3, 64
    robot, ctrl, objs = _cfg13(B, ld, False)
    mf = objs[0]
    planes = _table_under(robot, objs, 2e-3)
    with pytest.raises(sp.SaipError, match="neither contact planes nor a contact patch"):
        mf.setContactSchedule(np.zeros((1, 1, B, 12)))
    mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    key = np.zeros((2, 1, 12, B))
    key[:, 0, :8] = planes[0].T[None]
    with pytest.raises(ValueError, match=r"keyframes of shape \(K, n, 3, 12\)"):
        mf.setContactSchedule(key[..., 0])                                        # a batch-uniform layout against a per-instance table
    for first, n in ((1, 1), (-1, 1), (0, 2)):
        with pytest.raises(ValueError, match="outside the 1 items"):
            mf.setContactSchedule(_facade(np.repeat(key, n, axis=1)), first=first)
    bad = key.copy()
    bad[1, 0, 11, 2] = 1.0
    with pytest.raises(ValueError, match="keyframe 1, plane 0 of instance 2: the reserved word 11 is not 0"):
        mf.setContactSchedule(_facade(bad))
    bad = key.copy()
    bad[1, 0, 4, 0] = -1.0
    with pytest.raises(ValueError, match="keyframe 1: stiffness k > 0 required"):
        mf.setContactSchedule(_facade(bad))
    bad = key.copy()
    bad[0, 0, 9, 1] = np.inf
    with pytest.raises(ValueError, match="not finite"):
        mf.setContactSchedule(_facade(bad))
    bad = key.copy()
    bad[1, 0, 0:3] = -bad[0, 0, 0:3]
    with pytest.raises(ValueError, match="n_a . n_b < 0"):
        mf.setContactSchedule(_facade(bad), mode="linear")
    assert mf.contactVelocityDevice() is None                                     # nothing was attached by the refused calls
    mf.setContactSchedule(_facade(key))
    with pytest.raises(sp.SaipError, match="already have an environment schedule"):
        mf.setContactSchedule(_facade(key))
    with pytest.raises(sp.SaipError, match="written by an environment schedule"):
        mf.setContactPlanes(planes)
    mf.detachContactPlanes()                                                      # releases the schedule first
    L = _lib()
    assert L.saip_batch_env_schedule_keyframes_device(ctrl._h, ES.TARGET_PLANES, -1) is None
    mf.attachContactPlanes(planes, sensor=True, per_instance=True)
    mf.setContactPlanes(planes)                                                   # ... so the planes can be set again
    with pytest.raises(sp.SaipError, match="have no environment schedule"):
        mf.contactScheduleInfo()
    mf.detachContactPlanes()
    # the same for a patch and for the clearance monitor
    mf.attachContactPatch(SQUARE, _floor(robot, EE, EE_POS, SQUARE, 2e-3), sensor=True, per_instance=True)
    mf.setContactSchedule(_facade(key))
    with pytest.raises(sp.SaipError, match="written by an environment schedule"):
        mf.setContactPatchPlanes(planes)
    mf.detachContactPatch()
    assert L.saip_batch_env_schedule_keyframes_device(ctrl._h, ES.TARGET_PATCH, -1) is None
    obst = np.array([[1, 0.0, 0.0, 1.0, -1.0, 0, 0, 0], [0, 0.3, 0.0, 0.9, 0.5, 0.0, 0.9, 0.02]])
    ctrl.attachClearance(SPHERES, obst, margin=0.05)
    ko = np.repeat(obst[None], 2, axis=0)
    bad = ko.copy()
    bad[1, 0, 0] = 0.0
    with pytest.raises(ValueError, match="kind 0 differs from keyframe 0"):
        ctrl.setObstacleSchedule(bad)
    bad = ko.copy()
    bad[1, 0, 3] = 1.0 + 3e-6
    with pytest.raises(ValueError, match="the half-space normal has length"):
        ctrl.setObstacleSchedule(bad)
    ctrl.setObstacleSchedule(ko)
    with pytest.raises(sp.SaipError, match="written by an environment schedule"):
        ctrl.setClearanceObstacles(obst)
    assert L.saip_batch_env_schedule_velocity_device(ctrl._h, ES.TARGET_OBSTACLES, -1) is None      # obstacles have no velocity table
    ctrl.detachClearance()
    assert L.saip_batch_env_schedule_keyframes_device(ctrl._h, ES.TARGET_OBSTACLES, -1) is None
    with pytest.raises(sp.SaipError, match="have no environment schedule"):
        ctrl.obstacleScheduleInfo()


@pytest.mark.parametrize("B,ld", [(65, 128)])
def test_attach_and_detach_leaves_todays_rollout(sp, B, ld):
    """a controller that never had a schedule against a twin that attached one (contact planes and obstacles) and detached it before the
    first rollout: the same bits everywhere"""
    ends = []
    for touch in (False, True):
        robot, ctrl, objs = _cfg13(B, ld, False)
        mf = objs[0]
        planes = _table_under(robot, objs, 2e-3)
        mf.attachContactPlanes(planes, sensor=True, per_instance=True)
        obst = np.array([[1, 0.0, 0.0, 1.0, -1.0, 0, 0, 0], [0, 0.3, 0.0, 0.9, 0.5, 0.0, 0.9, 0.02]])
        ctrl.attachClearance(SPHERES, obst, margin=0.05)
        ctrl.recordRollouts(PERIODS, 1, ("q", "tau"), task=mf, summaries=True)
        if touch:
            key = np.zeros((2, 1, 12, B))
            key[:, 0, :8] = planes[0].T[None]
            key[1, 0, 3] += 0.01
            key[:, 0, 8] = 0.5
            mf.setContactSchedule(_facade(key), mode="linear")
            ko = np.repeat(obst[None], 2, axis=0)
            ko[1, 1, 1:7] += 0.2
            ctrl.setObstacleSchedule(ko, mode="linear")
            mf.clearContactSchedule()
            ctrl.clearObstacleSchedule()
        ctrl.rolloutAsync(PERIODS, DT, SUB, gravity=ZERO_G)
        out = _contact_end(ctrl, objs, mf, False)
        s = ctrl.clearanceSummary()
        out["clearance"] = np.column_stack([np.asarray(v, float) for v in s.values()])
        ends.append(out)
    for k in ends[0]:
        assert _same_bits(np.asarray(ends[0][k]), np.asarray(ends[1][k])), k
    assert (ends[0]["summary"][:, 3] >= 1).all()
