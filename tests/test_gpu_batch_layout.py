"""Batch layout: every device array is [rows][ld], and ld may exceed the batch rounded up to 32 (saip_batch_set_leading_dimension: the
common ld of uneven shards, sharding.shard_ld) or belong to the caller (saip_batch_bind_tau_device, saip_batch_set_state_device, the
per-task *_device entries).  Every kernel family at padded ld against the same inputs at the default ld (bitwise: grid, kernel choice and
per-instance arithmetic depend on B only, ld only moves addresses) and against the oracle; state carried across cycles; caller buffers
whose padding must stay untouched; padding columns that must never be read; uneven shards of one stream emulated on one GPU."""
import ctypes as C

import numpy as np
import pytest

import workloads as W

pytestmark = pytest.mark.gpu
TOL = 1e-5
SENTINEL = 6.02214076e23     # a distinctive finite value in caller-buffer padding
GARBAGE = 4.0e5              # scale of the finite garbage put into padding columns the kernels must not read

LANE, GENERAL = 2, 1      # setKernel selectors (0 = automatic choice)


# ------------------------------------------------------------------ helpers
def _r32(B):
    return (B + 31) // 32 * 32


def _lds(B):
    """the default ld, one column block more, and an ld of at least 2 B that is not a power of two"""
    big = _r32(2 * B)
    while big & (big - 1) == 0 or big == _r32(B) + 32:
        big += 32
    return [_r32(B), _r32(B) + 32, big]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


_HIP = None


def _hip():
    global _HIP
    if _HIP is None:
        h = C.CDLL("libamdhip64.so.7")
        h.hipMalloc.argtypes, h.hipMalloc.restype = [C.POINTER(C.c_void_p), C.c_size_t], C.c_int
        h.hipMemcpy.argtypes, h.hipMemcpy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        h.hipFree.argtypes, h.hipFree.restype = [C.c_void_p], C.c_int
        _HIP = h
    return _HIP


def _d2h(ptr, shape, dtype=np.float64):
    """a copy of device memory at `ptr` (the engine's own arrays or a caller buffer); the engine stream must be idle"""
    out = np.empty(shape, dtype)
    assert _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(out.nbytes), 2) == 0   # hipMemcpyDeviceToHost
    return out


def _h2d(ptr, host):
    host = np.ascontiguousarray(host)
    assert _hip().hipMemcpy(C.c_void_p(ptr), host.ctypes.data_as(C.c_void_p), C.c_size_t(host.nbytes), 1) == 0   # hipMemcpyHostToDevice


class _DevBuf:
    """a caller-owned device buffer from the HIP runtime the engine links"""

    def __init__(self, host):
        self.shape, self.nbytes = host.shape, host.nbytes
        p = C.c_void_p()
        assert _hip().hipMalloc(C.byref(p), C.c_size_t(self.nbytes)) == 0
        self.ptr = p.value
        _h2d(self.ptr, host)

    def get(self):
        return _d2h(self.ptr, self.shape)

    def free(self):
        if self.ptr:
            _hip().hipFree(C.c_void_p(self.ptr))
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


def _padded(cols, ld, B, fill):
    """[rows][ld]: cols (rows, B) in [0, B), `fill` (a scalar or a (rows, ld - B) array) in the padding"""
    out = np.empty((cols.shape[0], ld))
    out[:, :B] = cols
    out[:, B:] = fill
    return out


def _goals(model, tasks, q, rng):
    """goal blocks near the current pose for hand-built stacks (the generator of tests/test_gpu_oct.py)"""
    B, n = q.shape
    frames = W.fk(model, q)
    goals = []
    for t in tasks:
        if t["type"] == "motion_force":
            R, o = frames[model.link_index(t["link"])]
            x = o + np.einsum("bij,j->bi", R, np.asarray(t["pos_in_link"], float))
            Rg = W._expm_so3(rng.uniform(-0.2, 0.2, (B, 3))) @ (R @ np.asarray(t["rot_in_link"], float))
            goals.append(np.concatenate([x + rng.uniform(-0.05, 0.05, (B, 3)), Rg.reshape(B, 9), rng.uniform(-0.1, 0.1, (B, 6)),
                                         rng.uniform(-0.5, 0.5, (B, 6))], axis=1))
        else:
            S = W.joint_selection(t, n)
            m = S.shape[0]
            goals.append(np.concatenate([q @ S.T + rng.uniform(-0.3, 0.3, (B, m)), rng.uniform(-0.1, 0.1, (B, m)), rng.uniform(-0.5, 0.5, (B, m))], axis=1))
    return goals


def _flagging(spec):
    """engine extra: the blended singularity strategies switched off -> instances outside the non-singular branch are flagged (status 1)"""
    return [dict(t, singularity_strategies=False) if t["type"] == "motion_force" else t for t in spec]


def _stack(name, B):
    """inputs of one named stack: dict(desc, model, tasks, q, dq, goals, opts, on_list = setFlaggedRecompute(True))"""
    rng = np.random.default_rng(B + sum(map(ord, name)))
    opts, on_list = {}, False
    if name.startswith("cfg"):
        cfg = int(name[3:].split("_")[0])
        d = W.make_inputs(cfg, B)
        model, tasks, q, dq, goals = d["model"], d["tasks"], d["q"].copy(), d["dq"], d["goals"]
        if name == "cfg11_jla":
            opts = dict(joint_limit_avoidance=True, gravity_comp=True, torque_saturation=True)
        elif name == "cfg12_list":
            on_list = True
        elif name == "cfg13_passivity":
            tasks = [dict(tasks[0], passivity=True), tasks[1]]
        elif name == "cfg14_flagging":
            tasks = _flagging(tasks)
        elif name == "cfg5_postures":   # tests/test_gpu_wave.py: stretched-out instances and ones locked straight behind the elbow task
            q[0::4] = rng.uniform(-0.02, 0.02, q[0::4].shape)
            q[1::4, 15:] = rng.uniform(-1e-3, 1e-3, q[1::4, 15:].shape)
        elif name == "cfg6_flagging":   # elbow nearly straight in every third instance, blended strategies off
            tasks = _flagging(tasks)
            q[0::3, 4] = -0.07 - 0.25 * rng.uniform(size=q[0::3].shape[0])
        return dict(desc=model.name, model=model, tasks=tasks, q=q, dq=dq, goals=goals, opts=opts, on_list=on_list)
    if name == "arm6":
        from test_gpu_oct import _six_dof_chain
        desc = _six_dof_chain(np.random.default_rng(14))
        model = W.RobotModel(desc)
        q = rng.uniform(0.7 * model.q_lower, 0.7 * model.q_upper, (B, 6))
        dq = rng.uniform(-0.5, 0.5, (B, 6))
        tasks = [W.motion_force_task("hand", "link6", (0.02, 0.0, 0.1)), W.joint_task("posture")]
    else:
        base = W.make_inputs(15 if name.startswith("arm8") else 2, B)
        model, q, dq = base["model"], base["q"], base["dq"]
        ee, off = "end-effector", (0, 0, 0.07)
        pos, ori = [[1, 0, 0], [0, 1, 0], [0, 0, 1]], [[1, 0, 0], [0, 1, 0], [0, 0, 1]]
        tasks = {
            "pos_ori_joint": [W.motion_force_task("pos_task", ee, off, dirs_trans=pos, dirs_rot=None),
                              W.motion_force_task("ori_task", ee, off, dirs_trans=None, dirs_rot=ori), W.joint_task("joint_task")],
            "pos_velsat_joint4": [W.motion_force_task("pos_task", ee, off, dirs_trans=pos, dirs_rot=None, vel_sat=True, lin_sat=0.02),
                                  W.joint_task("partial_joint_task", S=[0, 2, 4, 6])],
            "joint2_pos": [W.joint_task("partial_joint_task", S=[0, 3]), W.motion_force_task("pos_task", ee, off, dirs_trans=pos, dirs_rot=None)],
            "rank2_joint": [W.motion_force_task("line_task", ee, off, dirs_trans=[[0, 0, 1]], dirs_rot=[[0, 0, 1]]), W.joint_task("joint_task")],
            "arm8_pos_joint": [W.motion_force_task("pos_task", ee, off, dirs_trans=pos, dirs_rot=None), W.joint_task("joint_task")],
        }[name]
        desc = model.name
    return dict(desc=desc, model=model, tasks=tasks, q=q, dq=dq, goals=_goals(model, tasks, q, rng), opts=opts, on_list=on_list)


def _build(c, B, ld=None, kernel=None, disable_otg=True):
    from sai_primitives_amd import capi
    from sai_primitives_amd.controller import controller_from_specs
    robot, ctrl, objs = controller_from_specs(c["desc"], c["tasks"], B, device=0, disable_otg=disable_otg, leading_dimension=ld)
    assert capi.lib().saip_batch_ld(ctrl._h) == (_r32(B) if ld is None else ld)
    ctrl.setFlaggedTorquePolicy(True)
    if kernel is not None:
        ctrl.setKernel(kernel)
    if c["on_list"]:
        ctrl.setFlaggedRecompute(True)
    ctrl.enableJointLimitAvoidance(c["opts"].get("joint_limit_avoidance", False))
    ctrl.enableGravityCompensation(c["opts"].get("gravity_comp", False))
    ctrl.enableTorqueSaturation(c["opts"].get("torque_saturation", False))
    return robot, ctrl, objs


def _cycle(robot, ctrl, q, dq, goals):
    robot.setQ(q)
    robot.setDq(dq)
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    ctrl.setGoals(goals)
    tau = ctrl.computeControlTorques()
    return tau, ctrl.status.copy()


def _sample(B, k=300):
    """all rows of small batches; first, last and a random sample of large ones"""
    if B <= 4096:
        return None
    return np.unique(np.concatenate([[0, B - 1], np.random.default_rng(B).choice(B, k, replace=False)]))


def _oracle(c, tau, status, rows=None, q=None, goals=None, orc=None):
    """status bits 0 and 3 and the torques of the instances the oracle does not refuse, on `rows` (None = all)"""
    from oracle import Oracle
    q = c["q"] if q is None else q
    goals = c["goals"] if goals is None else goals
    sel = slice(None) if rows is None else rows
    orc = Oracle(c["model"], c["tasks"], **c["opts"]) if orc is None else orc
    ref, st = orc.step(q[sel], c["dq"][sel], [g[sel] for g in goals], nthreads=8)
    assert np.array_equal(status[sel] & 9, st & 9)
    ok = st != 1
    err = W.torque_error(tau[sel][ok], ref[ok])
    assert err < TOL, err
    return st


# ------------------------------------------------------------------ A. kernel matrix at padded ld
MATRIX = [
    # saip_cycle_oct (eight lanes per instance)
    pytest.param("cfg2", 1001, 0, "saip_cycle_oct", id="oct-lean-cfg2"),                  # oct_general_joint 0, no JLA / general law: the lean instantiation
    pytest.param("cfg3", 203, 0, "saip_cycle_oct", id="oct-partial-cfg3"),                # partial task, 4-row joint task: oct_general_joint 1, partial_mf
    pytest.param("cfg12", 203, 0, "saip_cycle_oct", id="oct-reduced-cfg12-tail"),         # handling disabled: truncate path, status 2, in-kernel slow tail
    pytest.param("cfg14", 203, 0, "saip_cycle_oct", id="oct-blended-cfg14"),              # blended strategies in the kernel itself, status 8
    pytest.param("cfg11_jla", 203, 0, "saip_cycle_oct", id="oct-jla-cfg11"),              # joint limit avoidance + gravity + saturation
    pytest.param("cfg15", 203, 0, "saip_cycle_oct", id="oct-8dof-cfg15"),                 # 8-dof chain: the general instantiation with N = 8
    pytest.param("cfg2", 8197, 0, "saip_cycle_oct", id="oct-rounds-cfg2-B8197"),          # more instances than the chip holds at once: rounds
    pytest.param("cfg12_list", 203, 0, "saip_cycle_oct", id="oct-reduced-cfg12-list"),    # setFlaggedRecompute: wg_list behind instead of the tail
    # saip_cycle_octjf (joint task first)
    pytest.param("cfg6", 13, 0, "saip_cycle_octjf", id="octjf-cfg6-B13"),
    pytest.param("cfg6", 8193, 0, "saip_cycle_octjf", id="octjf-cfg6-B8193-tail"),       # rounds, slow tail
    # saip_cycle_lane: every branch of launch_cycle_lane
    pytest.param("cfg2", 203, LANE, "saip_cycle_lane", id="lane-7_1_MFJT-cfg2"),                      # <7,1,MF_JT>, no general law
    pytest.param("cfg10", 203, LANE, "saip_cycle_lane", id="lane-7_1_MFJT_GL-cfg10"),                 # <7,1,MF_JT> general law (force space, velocity saturation)
    pytest.param("pos_ori_joint", 203, LANE, "saip_cycle_lane", id="lane-7_1_GENERIC-three_tasks"),  # <7,1,GENERIC>: three tasks, joint rank bound 1
    pytest.param("cfg3", 203, LANE, "saip_cycle_lane", id="lane-7_4_MFJT-cfg3"),                      # <7,4,MF_JT>, no general law
    pytest.param("pos_velsat_joint4", 203, LANE, "saip_cycle_lane", id="lane-7_4_MFJT_GL-velsat"),    # <7,4,MF_JT> general law
    pytest.param("joint2_pos", 203, LANE, "saip_cycle_lane", id="lane-7_4_GENERIC-joint_first"),      # <7,4,GENERIC>: joint task first, rank 2
    pytest.param("rank2_joint", 203, LANE, "saip_cycle_lane", id="lane-7_7-rank2_task"),              # <7,7>: joint rank bound 5
    pytest.param("cfg15", 203, LANE, "saip_cycle_lane", id="lane-8_2-cfg15"),                         # <8,2>
    pytest.param("arm8_pos_joint", 203, LANE, "saip_cycle_lane", id="lane-8_8-position_task"),        # <8,8>: joint rank bound 5
    pytest.param("arm6", 203, LANE, "saip_cycle_lane", id="lane-6_6-arm6"),                           # <6,6> (most postures blended: wg_list)
    pytest.param("cfg2", 16389, LANE, "saip_cycle_lane", id="lane-lean-cfg2-B16389"),                 # launch_cycle_lane_lean: B > 64 * 256
    pytest.param("cfg12", 203, LANE, "saip_cycle_lane", id="lane-list-cfg12"),                        # non-empty slow-path list: saip_cycle_wg_list
    pytest.param("cfg14", 203, LANE, "saip_cycle_lane", id="lane-list-cfg14"),
    pytest.param("cfg13", 203, 0, "saip_cycle_lane", id="lane-closed_loop-cfg13"),                    # closed-loop force: <7,1,MF_JT> general law
    # saip_cycle_wave + its wg_list, the general kernel
    pytest.param("cfg5_postures", 65, 0, "saip_cycle_wave", id="wave-list-cfg5-B65"),
    pytest.param("cfg2", 203, GENERAL, "saip_cycle_wg<8,64>", id="wg8-cfg2"),
    pytest.param("cfg5_postures", 65, GENERAL, "saip_cycle_wg<32,512>", id="wg32-cfg5-B65"),
    pytest.param("cfg13_passivity", 203, 0, "saip_cycle_wg<8,64>", id="wg8-passivity-cfg13"),         # passivity controller: general kernel
]


@pytest.mark.parametrize("stack,B,kernel,expected", MATRIX)
def test_padded_ld_matches_default_ld_and_oracle(stack, B, kernel, expected):
    c = _stack(stack, B)
    runs = []
    for ld in _lds(B):
        robot, ctrl, _ = _build(c, B, ld, kernel)
        tau, st = _cycle(robot, ctrl, c["q"], c["dq"], c["goals"])
        assert ctrl.kernelName() == expected, ld
        runs.append((ld, tau, st))
        del robot, ctrl
    for ld, tau, st in runs[1:]:
        assert np.array_equal(st, runs[0][2]), ld
        assert _same_bits(tau, runs[0][1]), ld
    st = _oracle(c, runs[0][1], runs[0][2], _sample(B))
    print(stack, B, expected, "lds", [r[0] for r in runs], "status set", sorted(set(st.tolist())))


def test_oct_list_recompute_equals_in_kernel_tail():
    """the same flagged instances recomputed on the device-side list behind the eight-lane kernel and in the kernel's own tail, at padded ld"""
    B = 203
    ld = _lds(B)[2]
    out = []
    for name in ("cfg12", "cfg12_list"):
        c = _stack(name, B)
        robot, ctrl, _ = _build(c, B, ld)
        out.append(_cycle(robot, ctrl, c["q"], c["dq"], c["goals"]))
        assert ctrl.kernelName() == "saip_cycle_oct"
    assert (out[0][1] == 2).sum() > B // 8
    assert np.array_equal(out[0][1], out[1][1])
    assert _same_bits(out[0][0], out[1][0])


# ------------------------------------------------------------------ B. state carried across cycles
def _getters(tasks, otg):
    vals = []
    for t in tasks:
        vals.append(t._desired_block())
        vals.append(t.getTaskNullspace().reshape(t._robot.batch_size, -1))
        if otg:
            _, fl, res = t.getInternalOtgStatus()
            vals += [fl.astype(np.float64), res.astype(np.float64)]
    return vals


@pytest.mark.parametrize("case", [
    pytest.param("integrators", id="oct-integrators-cfg2"),      # ki on both tasks: integ / integ_new committed per instance
    pytest.param("blended", id="oct-blended_state-cfg14"),       # handler state of the blended strategies
    pytest.param("otg_pair", id="otg_pair-oct-cfg2"),            # both internal OTGs: launch_otg_pair, lane-major OTG state
    pytest.param("flag_parity", id="lane_list-wg-alternating-cfg12"),  # kernels 2, 1, 2, 2: flag-list parity and flag_clean
])
def test_state_across_cycles_at_padded_ld(case):
    from oracle import Oracle
    B = 203
    c = _stack({"integrators": "cfg2", "blended": "cfg14", "otg_pair": "cfg2", "flag_parity": "cfg12"}[case], B)
    if case == "integrators":
        c["tasks"] = [dict(c["tasks"][0], ki_pos=5.0, ki_ori=7.0), dict(c["tasks"][1], ki=3.0)]
    otg = case == "otg_pair"
    kernels = [LANE, GENERAL, LANE, LANE] if case == "flag_parity" else [0] * 4
    names = []
    runs = {}
    for ld in (None, _lds(B)[2]):
        robot, ctrl, tasks = _build(c, B, ld, disable_otg=not otg)
        orc = Oracle(c["model"], c["tasks"], **c["opts"])
        robot.setQ(c["q"])
        robot.setDq(c["dq"])
        robot.updateModel()
        if otg:
            ctrl.reinitializeTasks()
        ctrl.setGoals(c["goals"])
        out = []
        for k in range(4):
            ctrl.setKernel(kernels[k])
            q = c["q"] + 1e-3 * k * np.cos(np.arange(c["q"].shape[1]))   # a new state each cycle
            robot.setQ(q)
            robot.updateModel()
            ctrl.updateControllerTaskModels()
            tau = ctrl.computeControlTorques()
            st = ctrl.status.copy()
            if ld is None:
                names.append(ctrl.kernelName())
                des = [t._desired_block()[:, :g.shape[1]] for t, g in zip(tasks, c["goals"])] if otg else None
                _oracle(c, tau, st, q=q, goals=des, orc=orc)
            out.append([tau, st.astype(np.float64)] + _getters(tasks, otg))
        runs[ld] = out
        del robot, ctrl, tasks
    if case == "flag_parity":
        assert names == ["saip_cycle_lane", "saip_cycle_wg<8,64>", "saip_cycle_lane", "saip_cycle_lane"]
        assert (runs[None][0][1] == 2).sum() > B // 8
    else:
        assert names == ["saip_cycle_oct"] * 4
    for k in range(4):
        for i, (a, b) in enumerate(zip(runs[None][k], runs[_lds(B)[2]][k])):
            assert _same_bits(a, b), (k, i)


@pytest.mark.parametrize("on_list", [False, True], ids=["oct-tail", "oct-list"])
def test_last_instance_flagged_in_a_ragged_batch(on_list):
    """config 12 at B = 97: instance 96 is near-singular (every third is) and alone in the last group of eight lanes, whose dead lanes
    shadow it.  Integrators on the motion-force task must advance exactly once per cycle: three cycles against the oracle, bitwise the same
    at padded ld"""
    from oracle import Oracle
    B = 97
    c = _stack("cfg12_list" if on_list else "cfg12", B)
    c["tasks"] = [dict(c["tasks"][0], ki_pos=3.0, ki_ori=4.0), c["tasks"][1]]
    runs = []
    for ld in (None, _lds(B)[1], _lds(B)[2]):
        robot, ctrl, _ = _build(c, B, ld)
        orc = Oracle(c["model"], c["tasks"])
        out = []
        for cycle in range(3):
            q = c["q"] + 1e-3 * cycle
            tau, st = _cycle(robot, ctrl, q, c["dq"], c["goals"])
            assert ctrl.kernelName() == "saip_cycle_oct"
            assert st[B - 1] == 2 and st[B - 2] == 0
            if ld is None:
                _oracle(c, tau, st, q=q, orc=orc)
            out.append((tau, st))
        runs.append(out)
        del robot, ctrl
    for out in runs[1:]:
        for (t0, s0), (t1, s1) in zip(runs[0], out):
            assert np.array_equal(s0, s1) and _same_bits(t0, t1)


# ------------------------------------------------------------------ C. caller buffers and untouched padding
BOUND = [
    pytest.param("cfg14_flagging", 203, 0, "saip_cycle_oct", id="oct-cfg14_flagged"),
    pytest.param("cfg6_flagging", 203, 0, "saip_cycle_octjf", id="octjf-cfg6_flagged"),
    pytest.param("cfg14_flagging", 203, LANE, "saip_cycle_lane", id="lane-cfg14_flagged"),
    pytest.param("cfg14", 203, LANE, "saip_cycle_lane", id="lane-list-cfg14"),
    pytest.param("cfg5_postures", 65, 0, "saip_cycle_wave", id="wave-list-cfg5"),
    pytest.param("cfg14_flagging", 203, GENERAL, "saip_cycle_wg<8,64>", id="wg8-cfg14_flagged"),
]


@pytest.mark.parametrize("stack,B,kernel,expected", BOUND)
def test_bound_torque_buffer_keeps_its_padding(stack, B, kernel, expected):
    c = _stack(stack, B)
    n = c["q"].shape[1]
    states = [(c["q"] + 1e-3 * k, c["dq"]) for k in range(2)]
    robot, ctrl, _ = _build(c, B, None, kernel)
    ref = [_cycle(robot, ctrl, q, dq, c["goals"]) for q, dq in states]
    assert ctrl.kernelName() == expected
    assert any(((s & 1) != 0).any() or ((s & 8) != 0).any() for _, s in ref), "the scenario must contain singular instances"
    del robot, ctrl
    for ld in _lds(B)[1:]:
        with _DevBuf(np.full((n, ld), SENTINEL)) as buf:
            robot, ctrl, _ = _build(c, B, ld, kernel)
            ctrl.bindTauDevice(buf.ptr)
            assert ctrl.devicePointers()["tau"] == buf.ptr
            for (q, dq), (tau_ref, st_ref) in zip(states, ref):
                tau, st = _cycle(robot, ctrl, q, dq, c["goals"])
                assert ctrl.kernelName() == expected
                assert np.array_equal(st, st_ref) and _same_bits(tau, tau_ref)
                ctrl.synchronize()
                slab = buf.get()
                assert _same_bits(slab[:, :B].T, tau)
                assert _same_bits(ctrl.getTorques(), tau)
                assert np.all(_bits(slab[:, B:]) == _bits(np.float64(SENTINEL))), ld
            del robot, ctrl


def _engine_slabs(ctrl, n):
    p = ctrl.devicePointers()
    ld = p["ld"]
    return [_d2h(p[k], (n, ld)) for k in ("q", "dq", "tau")] + [_d2h(p["status"], (ld,), np.uint8)]


def _assert_padding_zero(slabs, B):
    for s in slabs:
        assert not s[..., B:].any()      # still the dev_alloc fill: no kernel stored past B


@pytest.mark.parametrize("stack,B", [pytest.param("cfg2", 203, id="integrate_oct-7dof"), pytest.param("cfg15", 203, id="integrate_kernel8-8dof"),
                                     pytest.param("cfg5", 65, id="integrate_kernel32-30dof")])
def test_integrate_leaves_padding_alone(stack, B):
    c = _stack(stack, B)
    n = c["q"].shape[1]
    final = {}
    for ld in (None, _lds(B)[2]):
        robot, ctrl, _ = _build(c, B, ld)
        robot.setQ(c["q"])
        robot.setDq(c["dq"])
        robot.updateModel()
        ctrl.setGoals(c["goals"])
        for _ in range(2):
            ctrl.updateControllerTaskModels()
            ctrl.computeControlTorques()
            ctrl.integrate(1e-3, 2)
        ctrl.synchronize()
        _assert_padding_zero(_engine_slabs(ctrl, n), B)
        q, dq = ctrl.pullState()
        assert np.isfinite(q).all() and np.isfinite(dq).all()
        final[ld] = (q.copy(), dq.copy())
        del robot, ctrl
    (q0, dq0), (q1, dq1) = final.values()
    assert _same_bits(q0, q1) and _same_bits(dq0, dq1)


@pytest.mark.parametrize("otg", [False, True], ids=["rollout-oct_fused_integration", "rollout-otg_pair_with_integration"])
def test_rollout_leaves_padding_alone(otg):
    """rolloutAsync without internal OTG (the eight-lane cycle integrates in-kernel) and with both OTGs (integration and the next period's
    trajectory step in one launch)"""
    B = 203
    c = _stack("cfg2", B)
    final = {}
    for ld in (None, _lds(B)[2]):
        robot, ctrl, tasks = _build(c, B, ld, disable_otg=not otg)
        robot.setQ(c["q"])
        robot.setDq(c["dq"])
        robot.updateModel()
        if otg:
            ctrl.reinitializeTasks()
        ctrl.setGoals(c["goals"])
        ctrl.rolloutAsync(4, 1e-3, 2)
        ctrl.synchronize()
        assert ctrl.kernelName() == "saip_cycle_oct"
        slabs = _engine_slabs(ctrl, 7)
        _assert_padding_zero(slabs, B)
        q, dq = ctrl.pullState()
        assert np.isfinite(q).all() and not np.array_equal(q, c["q"])
        final[ld] = [q.copy(), dq.copy(), slabs[2][:, :B].copy()] + [t._desired_block() for t in tasks]
        del robot, ctrl, tasks
    a, b = final.values()
    for i, (x, y) in enumerate(zip(a, b)):
        assert _same_bits(x, y), i


@pytest.mark.parametrize("stack,B,kernel", [pytest.param("cfg2", 203, 0, id="oct-cfg2"), pytest.param("cfg6", 203, 0, id="octjf-cfg6"),
                                            pytest.param("cfg14", 203, LANE, id="lane-list-cfg14"), pytest.param("cfg5_postures", 65, 0, id="wave-list-cfg5"),
                                            pytest.param("cfg2", 203, GENERAL, id="wg8-cfg2")])
def test_padding_columns_are_never_read(stack, B, kernel):
    """q, dq (saip_batch_set_state_device) and the goals with large finite garbage in their padding columns: torques and status bitwise
    equal to the same state and goals set from the host"""
    from sai_primitives_amd import capi
    c = _stack(stack, B)
    ld = _lds(B)[2]
    rng = np.random.default_rng(3)
    robot, ctrl, _ = _build(c, B, ld, kernel)
    tau_ref, st_ref = _cycle(robot, ctrl, c["q"], c["dq"], c["goals"])
    del robot, ctrl
    robot, ctrl, tasks = _build(c, B, ld, kernel)
    n = c["q"].shape[1]

    def junk(rows):
        return GARBAGE * rng.uniform(-1.0, 1.0, (rows, ld - B))

    with _DevBuf(_padded(c["q"].T, ld, B, junk(n))) as qb, _DevBuf(_padded(c["dq"].T, ld, B, junk(n))) as dqb:
        capi.check(capi.lib().saip_batch_set_state_device(ctrl._h, C.c_void_p(qb.ptr), C.c_void_p(dqb.ptr)))
        ctrl.synchronize()
        for t, g in zip(tasks, c["goals"]):
            gs = capi.lib().saip_batch_goal_components(ctrl._h, t._id)
            full = np.zeros((B, gs))
            full[:, :g.shape[1]] = g
            _h2d(capi.lib().saip_batch_device_goal(ctrl._h, t._id), _padded(full.T, ld, B, junk(gs)))
        ctrl._call("saip_batch_update_task_models")      # (not the Python wrapper: it would push the host mirror over the device state)
        tau = ctrl.computeControlTorques()
    assert np.array_equal(ctrl.status, st_ref) and _same_bits(tau, tau_ref)


def test_per_task_device_entries_at_padded_ld():
    """example 04's manual hierarchy inside a controller at padded ld: updateTaskModel from a device nullspace (the engine's own and a
    caller buffer with garbage padding) and computeTorques into caller buffers; host entries, both lds and the caller padding agree"""
    from oracle import Oracle
    from sai_primitives_amd import capi
    L = capi.lib()
    B = 203
    c = _stack("cfg2", B)
    n = 7
    rng = np.random.default_rng(8)
    out = {}
    for ld in (None, _lds(B)[2]):
        robot, ctrl, (mf, jt) = _build(c, B, ld)
        ldv = ctrl.devicePointers()["ld"]
        robot.setQ(c["q"])
        robot.setDq(c["dq"])
        robot.updateModel()
        ctrl.setGoals(c["goals"])
        mf.updateTaskModel(np.eye(n))
        Nt = mf.getTaskAndPreviousNullspace()                 # host copy (B, n, n)
        jt.updateTaskModel(Nt)
        tau_mf = mf.computeTorques()
        tau_jt = jt.computeTorques(tau_mf)
        N_jt = jt.getTaskNullspace()
        # the engine's device nullspace
        jt.updateTaskModel(mf.getTaskAndPreviousNullspace(device=True))
        assert _same_bits(jt.computeTorques(tau_mf), tau_jt) and _same_bits(jt.getTaskNullspace(), N_jt)
        # a caller N_prec [n*n][ld] with garbage padding
        with _DevBuf(_padded(Nt.reshape(B, n * n).T, ldv, B, GARBAGE * rng.uniform(-1, 1, (n * n, ldv - B)))) as nb:
            capi.check(L.saip_batch_task_update_model_device(ctrl._h, jt._id, C.c_void_p(nb.ptr)))
            assert _same_bits(jt.computeTorques(tau_mf), tau_jt) and _same_bits(jt.getTaskNullspace(), N_jt)
        # computeTorques(tau_prec) with caller tau_prec_dev (sentinel padding) and tau_dev
        prec_host = _padded(tau_mf.T, ldv, B, SENTINEL)
        with _DevBuf(prec_host) as pb, _DevBuf(np.full((n, ldv), SENTINEL)) as tb:
            capi.check(L.saip_batch_task_compute_torques_device(ctrl._h, jt._id, C.c_void_p(pb.ptr), C.c_void_p(tb.ptr)))
            ctrl.synchronize()
            got, prec_after = tb.get(), pb.get()
        assert _same_bits(got[:, :B].T, tau_jt)
        assert np.all(_bits(got[:, B:]) == _bits(np.float64(SENTINEL)))
        assert _same_bits(prec_after, prec_host)
        out[ld] = (tau_mf, tau_jt, N_jt)
        del robot, ctrl, mf, jt
    for a, b in zip(*out.values()):
        assert _same_bits(a, b)
    ref, st = Oracle(c["model"], c["tasks"]).step(c["q"], c["dq"], c["goals"], nthreads=8)
    assert st.sum() == 0 and W.torque_error(out[None][0] + out[None][1], ref) < TOL


# ------------------------------------------------------------------ D. uneven shards on one GPU
@pytest.mark.parametrize("cfg,total,world,same_family", [
    pytest.param(2, 961, 3, True, id="oct-cfg2-world3"),             # shards 321 / 320 / 320: ld 352 (the smaller ones alone: 320)
    pytest.param(14, 1123, 7, True, id="oct-blended-cfg14-world7"),  # shards 161 x 3, 160 x 4: ld 192 (160)
    pytest.param(6, 450, 7, True, id="octjf-cfg6-world7"),           # shards 65 x 2, 64 x 5: ld 96 (64)
    pytest.param(2, 24577, 3, False, id="lane_lean-vs-oct-cfg2-world3"),  # whole batch > 24576: lane (lean); shards 8193 / 8192 / 8192: oct, ld 8224
])
def test_uneven_shards_equal_the_whole_batch(cfg, total, world, same_family):
    """what a node does, on one GPU: rank r takes shard_range(total, world, r) of one stream, every rank the common shard_ld, and writes
    into its slot of the [world][dof][ld] slab the all-gather delivers.  Same kernel family: bitwise the single-batch run.  Across a
    dispatch threshold (the whole batch on the lane kernel, the shards on the eight-lane one) only the oracle is compared.  (At padded ld
    alone the grouping of instances into wavefronts does not change: there blended instances are bitwise too, see above.)"""
    from sai_primitives_amd.sharding import shard_ld, shard_range
    c = _stack(f"cfg{cfg}", total)
    n = c["q"].shape[1]
    robot, ctrl, _ = _build(c, total)
    tau_w, st_w = _cycle(robot, ctrl, c["q"], c["dq"], c["goals"])
    whole = ctrl.kernelName()
    del robot, ctrl
    ld = shard_ld(total, world)
    sizes = [hi - lo for lo, hi in (shard_range(total, world, r) for r in range(world))]
    assert len(set(sizes)) == 2 and _r32(min(sizes)) < ld     # the smaller shards run above their own default ld
    with _DevBuf(np.full((world, n, ld), SENTINEL)) as buf:
        names, stats = [], []
        for r in range(world):
            lo, hi = shard_range(total, world, r)
            sub = dict(c, q=c["q"][lo:hi], dq=c["dq"][lo:hi], goals=[g[lo:hi] for g in c["goals"]])
            rb, cs, _ = _build(sub, hi - lo, ld)
            cs.bindTauDevice(buf.ptr + r * n * ld * 8)
            _, st = _cycle(rb, cs, sub["q"], sub["dq"], sub["goals"])
            names.append(cs.kernelName())
            stats.append(st)
            del rb, cs
        slab = buf.get()
    tau = np.concatenate([slab[r][:, :sizes[r]].T for r in range(world)])
    st = np.concatenate(stats)
    for r in range(world):
        assert np.all(_bits(slab[r][:, sizes[r]:]) == _bits(np.float64(SENTINEL))), r
    assert np.array_equal(st, st_w)
    if same_family:
        assert set(names) == {whole}
        # The one neighbour dependence: the eight-lane kernels' Jacobi eigen-solve (oct_jacobi_n) sweeps until EVERY instance of the
        # wavefront has converged, so a blended instance (status 8) gets as many sweeps as the slowest of the eight instances it shares a
        # wavefront with.  Shards start at lo = r * (total // world) + ..., not a multiple of eight, and regroup the instances; the extra
        # sweeps move its torques by rounding only.  Every other instance is bitwise the single-batch run.
        blended = (st & 8) != 0
        assert _same_bits(tau[~blended], tau_w[~blended])
        if blended.any():
            diff = W.torque_error(tau[blended], tau_w[blended])
            print("blended instances", int(blended.sum()), "bitwise", int((_bits(tau[blended]) == _bits(tau_w[blended])).all(axis=1).sum()),
                  "max rel difference", diff)
            assert diff < 1e-9
    else:
        assert whole == "saip_cycle_lane" and set(names) == {"saip_cycle_oct"}
        _oracle(c, tau_w, st_w, _sample(total))
    _oracle(c, tau, st, _sample(total))
    print("cfg", cfg, "total", total, "world", world, "ld", ld, "whole", whole, "shards", sorted(set(names)))
