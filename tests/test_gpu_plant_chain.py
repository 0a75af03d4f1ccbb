"""The actuation chain of the resident simulator on the device (saip_plant_apply<*, true> in csrc/saip_plant.hip, saip_batch_plant_chain_*).
Oracles: the plant model alone (a neutral chain changes nothing, on every cycle kernel); a plant-only twin at the same prescribed state fed
the command of d periods earlier (a pure delay) or the output of the NumPy restatement tests/plant_chain_ref.py (the full chain), whose
state the device's state arrays match bit for bit; the host-driven loop { cycle, integrate } for whole rollouts; and the first continuation
of a rollout for everything a snapshot restores.

Shapes: B = 70 at ld = 128 (two wavefronts, one partial, padded) on the Panda; for the neutral chain also the 30-dof chain (wavefront
kernel), a 6-dof arm on the lane kernel and the dual-arm tree (general kernel, saip_plant_apply<true, true>); the tree and a 1-dof chain
for the pure delay; depths 0, 1 and 8; 1 and 3 substeps; 5 to 16 periods."""
import numpy as np
import pytest

import chains as CH
import plant_chain_ref as PC
import plant_ref as PL
import sensing_chain_ref as SC
import trees as TR
import workloads as W
from test_gpu_batch_layout import _DevBuf, _d2h, _h2d, _same_bits
from test_gpu_contact import _cfg13, _table_under
from test_gpu_plant import _joint_table, _summary
from test_gpu_rollout_record import _panda
from test_gpu_sensing import KERNELS, ZERO_G, _case, _equal, _finals, _random_joint_table, dict_plant

pytestmark = pytest.mark.gpu

SENTINEL, ISENTINEL = 6.02214076e23, 0x5A5A5A5A
B, LD, N = 70, 128, 7
DT, SUB = 5e-4, 3


@pytest.fixture(scope="module")
def sp():
    import sai_primitives_amd as sp
    sp.build_library()
    if sp.device_count() < 1:
        pytest.fail("no HIP device")
    return sp


def _chain_table(rng, depth, n=N, per=True):
    """per-instance rows: every delay 0..depth, the rate limit off, binding and loose, the lag off, one substep and ten substeps long; joint 0
    of every instance neutral"""
    sh = (n, B) if per else (n,)
    t = np.zeros(sh + (3,))
    t[..., 0] = rng.integers(0, depth + 1, sh)
    t[..., 1] = rng.choice([np.inf, 4e3, 1e9], sh)                        # commands of a few N m: 4e3 / s binds at 0.5 ms, 1e9 / s never
    t[..., 2] = rng.choice([0.0, DT, 10 * DT], sh)
    t[0] = PC.NEUTRAL
    return t


def _act(ctrl, n=N, ld=LD):
    ctrl.synchronize()
    return np.ascontiguousarray(_d2h(ctrl.plantTorquesDevice(), (n, ld))[:, :ctrl.batch_size].T)


def _state(ctrl):
    st = ctrl.actuationChainState()
    return [st["taps"], st["filt"], st["primed"].astype(float)]


def _bound(ctrl, n=N, ld=LD):
    """a caller-owned commanded-torque buffer (n, ld), bound, a sentinel in its padding columns; write(t) puts (B, n) commands into it"""
    host = np.full((n, ld), SENTINEL)
    host[:, :ctrl.batch_size] = 0.0
    buf = _DevBuf(host)
    ctrl.bindTauDevice(buf.ptr)

    def write(t):
        host[:, :ctrl.batch_size] = np.asarray(t, float).T
        _h2d(buf.ptr, host)
    return buf, write


def _period(robot, ctrl, write, q, dq, t, sub):
    """one period at a prescribed state under a prescribed command: (tau_act of the last substep, q, dq after it)"""
    robot.setQ(q)
    robot.setDq(dq)
    write(t)
    ctrl.integrate(DT, sub, gravity=ZERO_G)
    act = _act(ctrl, q.shape[1], LD)
    return [act] + [a.copy() for a in ctrl.pullState()]


def _commands(rng, P, n=N, nonfinite=True):
    out = [rng.uniform(-8, 8, (B, n)) for _ in range(P)]
    if nonfinite:
        out[2][3] = np.nan                                                # a flagged instance under the NaN policy: no torque
        out[4][5, n - 1] = np.nan
    return out


def _states(rng, P, q0):
    ph = rng.uniform(0, 6.28, q0.shape)
    return [(q0 + 0.05 * np.sin(ph + 0.4 * p), 0.3 * np.cos(ph + 0.4 * p)) for p in range(P)]


# ------------------------------------------------------------------ 1. a neutral chain changes nothing
@pytest.mark.parametrize("name,otg", [(k, o) for k in ("panda", "chain30", "arm6_lane", "tree") for o in (False, True)])
def test_neutral_chain_equals_the_plant_alone(sp, name, otg):
    K, runs = 5, []
    for depth in (None, 0, 8):
        robot, ctrl, objs, q, dq, grav = _case(name, otg)
        n, ld = q.shape[1], KERNELS[name][2]
        ctrl.attachPlant(dict_plant(ctrl))
        if depth is not None:
            ctrl.attachActuationChain(depth=depth)
            assert ctrl.actuationChainInfo() == dict(attached=True, per_instance=False, depth=depth, state_bytes=((depth + 3) * 8 + 4) * n * ld)
        else:
            assert ctrl.actuationChainInfo()["attached"] is False
        ctrl.recordRollouts(K, 1, ("q", "dq", "tau"))
        out = [ctrl.computeControlTorques(), ctrl.status.astype(float)]
        assert ctrl.kernelName() == KERNELS[name][4]
        ctrl.integrate(DT, SUB, gravity=grav)
        out += _finals(ctrl) + [_act(ctrl, n, ld)]
        ctrl.rolloutAsync(K, DT, SUB, gravity=grav)
        out += _finals(ctrl) + [_act(ctrl, n, ld), _summary(ctrl)]
        log = ctrl.rolloutLog()
        out += [log[k] for k in ("q", "dq", "tau")] + [log["status"].astype(float)]
        if depth is not None:
            assert (ctrl.actuationChainState()["primed"] == 1).all()
        runs.append(out)
        ctrl.detachPlant()
    assert _equal(runs[0], runs[1]) and _equal(runs[0], runs[2])
    assert np.abs(runs[0][8]).max() > 1e-3 and (runs[0][12][:, 0] > 0).all()           # moving, and the friction is on


# ------------------------------------------------------------------ 2. a pure delay
def _delay_case(robot_name):
    """(robot, ctrl, model): a batch of B instances at ld = LD whose cycle nobody runs; the plant is driven through a bound buffer"""
    from sai_primitives_amd.controller import controller_from_specs
    if robot_name == "panda":
        d = W.make_inputs(2, B)
        desc, m, specs = d["model"].name, d["model"], d["tasks"]
    elif robot_name == "tree":
        desc = TR.dual_panda_torso()
        m = W.RobotModel(desc)
        specs = TR.dual_stack(m)
    else:
        desc = CH.small_chain(1, "random")
        m = W.RobotModel(desc)
        specs = [W.joint_task("posture")]
    robot, ctrl, objs = controller_from_specs(desc, specs, B, device=0, leading_dimension=LD)
    return robot, ctrl, m


@pytest.mark.parametrize("robot_name,kind,sub", [("panda", "d1", 1), ("panda", "depth", 3), ("panda", "per_instance", 3), ("panda", "per_instance", 1),
                                                 ("tree", "per_instance", 3), ("dof1", "per_instance", 3), ("dof1", "d1_depth1", 1)])
def test_pure_delay_is_the_plant_fed_the_command_of_d_periods_earlier(sp, robot_name, kind, sub):
    depth, P = (1, 6) if kind == "d1_depth1" else (8, 12)
    robot, ctrl, m = _delay_case(robot_name)
    n = m.dof
    rng = np.random.default_rng(19)
    d = np.full((B, n), depth if kind == "depth" else 1)
    if kind == "per_instance":
        d = np.repeat((np.arange(B) % (depth + 1))[:, None], n, axis=1)
        table = np.tile(PC.NEUTRAL, (n, B, 1))
        table[..., 0] = d.T
    else:
        table = dict(delay=float(d[0, 0]))
    q0 = np.clip(rng.uniform(-1.0, 1.0, (B, n)), m.q_lower + 0.2, m.q_upper - 0.2)
    traj, cmds = _states(rng, P, q0), _commands(rng, P, n)
    buf, write = _bound(ctrl, n)
    ctrl.attachPlant(_joint_table(rng, m, B), per_instance=True)          # friction and stops: tau_act depends on the state
    # the twin: the plant alone at the prescribed state of period p, fed per (instance, joint) the command of period p - d
    want = []
    for p, (q, dq) in enumerate(traj):
        src = np.maximum(p - d, 0)
        want.append(_period(robot, ctrl, write, q, dq, np.take_along_axis(np.stack(cmds), src[None], 0)[0], sub))
    ctrl.attachActuationChain(table, per_instance=kind == "per_instance", depth=depth)
    for p, (q, dq) in enumerate(traj):
        got = _period(robot, ctrl, write, q, dq, cmds[p], sub)
        assert _equal(got, want[p]), p
    ctrl.detachActuationChain()
    plain = _period(robot, ctrl, write, traj[-1][0], traj[-1][1], cmds[-1], sub)
    assert not _same_bits(plain[0], want[-1][0])                          # (the delayed command is another command)
    got = buf.get()
    assert np.all(got[:, B:] == SENTINEL) and _same_bits(got[:, :B], np.ascontiguousarray(cmds[-1].T))    # tau_cmd is never written
    ctrl.detachPlant()
    ctrl.bindTauDevice(0)
    buf.free()


# ------------------------------------------------------------------ 3. the full chain against the restatement
def test_full_chain_equals_the_restatement_bit_for_bit(sp):
    depth, P, P1 = 8, 12, 4
    rng = np.random.default_rng(43)
    table = _chain_table(rng, depth)
    table[2, 7], table[3, 9] = [1.0, np.inf, DT], [0.0, np.inf, 10 * DT]  # the rows the two infinite commands below go through
    assert set(np.unique(table[..., 0])) == set(range(depth + 1)) and set(np.unique(table[1:, :, 1])) == {np.inf, 4e3, 1e9}
    d = W.make_inputs(2, B)
    traj, cmds = _states(rng, P + P1, d["q"]), _commands(rng, P + P1)
    cmds[6][7, 2], cmds[7][9, 3] = np.inf, -np.inf                        # no special case: what they leave in a filter stays
    # a plant whose rows do not look at the state (gain, offset, saturation): tau_act of a period's LAST substep is known without the states
    # its earlier substeps went through; and a rough one (friction, stops) for the periods of one substep, where a twin has the same state
    blind = np.repeat(PL.neutral(N)[:, None, :], B, axis=1)
    blind[..., PL.GAIN], blind[..., PL.BIAS], blind[..., PL.TAU_MAX] = rng.uniform(0.8, 1.2, (N, B)), rng.uniform(-0.5, 0.5, (N, B)), rng.uniform(2.0, 9.0, (N, B))
    rough = _joint_table(rng, d["model"], B)
    robot, ctrl, m = _delay_case("panda")
    twin_robot, twin, _ = _delay_case("panda")
    buf, write = _bound(ctrl)
    tbuf, twrite = _bound(twin)
    ctrl.attachPlant(blind, per_instance=True)
    twin.attachPlant(rough, per_instance=True)
    ctrl.attachActuationChain(table, per_instance=True, depth=depth)
    ctrl.synchronize()
    # a sentinel in the padding columns of tau_act, of the table and of every state array, through the device pointers
    tp, fp, pp = ctrl.actuationChainStateDevice()
    shapes = {ctrl.plantTorquesDevice(): (N, LD), tp: (depth * N, LD), fp: (3 * N, LD)}
    for ptr, shp in shapes.items():
        a = np.zeros(shp)
        a[:, B:] = SENTINEL
        _h2d(ptr, a)
    tab = _d2h(ctrl.actuationChainTableDevice(), (N * 3, LD))
    assert _same_bits(tab[:, :B], np.ascontiguousarray(table.transpose(0, 2, 1)).reshape(N * 3, B))       # the documented layout
    tab[:, B:] = SENTINEL
    _h2d(ctrl.actuationChainTableDevice(), tab)
    shapes[ctrl.actuationChainTableDevice()] = (N * 3, LD)
    a = np.zeros((N, LD), np.int32)
    a[:, B:] = ISENTINEL
    _h2d(pp, a)
    ref = PC.Chain(table, depth, B)
    for p in range(P + P1):
        q, dq = traj[p]
        if p == P:
            ctrl.setPlantJoints(rough)
        sub = SUB if p < P else 1
        act, q1, dq1 = _period(robot, ctrl, write, q, dq, cmds[p], sub)
        for s in range(sub):
            t1 = ref.step(cmds[p], DT, s == 0)
        if p < P:
            want = PL.joint(blind, t1, q1, dq1)[0]
            assert _same_bits(act, want), p
        else:
            # the twin: the plant alone at the same state, commanded what the restatement hands pl_joint; its tau_act and its next state
            # are the chained batch's: q and dq are written by the integrator alone
            assert _equal([act, q1, dq1], _period(twin_robot, twin, twrite, q, dq, t1, 1)), p
            assert _same_bits(act, PL.joint(rough, t1, q, dq)[0])
        st = ctrl.actuationChainState()
        assert _same_bits(st["taps"], ref.taps) and _same_bits(st["filt"], ref.filt) and np.array_equal(st["primed"], ref.primed), p
        got = buf.get()
        assert np.all(got[:, B:] == SENTINEL) and _same_bits(got[:, :B], np.ascontiguousarray(cmds[p].T))             # tau_cmd keeps its bits
    assert _same_bits(ref.filt[:, 0, PC.Y_LAG], np.where(np.isnan(cmds[-1][:, 0]), 0.0, cmds[-1][:, 0])) and not _same_bits(ref.filt[..., PC.Y_LAG], cmds[-1])
    assert not np.isfinite(ref.filt).all() and np.isfinite(ref.filt).sum() > 0.9 * ref.filt.size
    ctrl.synchronize()
    for ptr, shp in shapes.items():
        got = _d2h(ptr, shp)
        assert np.all(got[:, B:] == SENTINEL) and not np.any(got[:, :B] == SENTINEL)
    got = _d2h(pp, (N, LD), np.int32)
    assert np.all(got[:, B:] == ISENTINEL) and np.all(got[:, :B] == 1)
    assert _same_bits(_d2h(tp, (N, depth, LD))[..., :B], np.ascontiguousarray(ref.taps.transpose(1, 2, 0)))            # the documented layout
    for c, b_ in ((ctrl, buf), (twin, tbuf)):
        c.detachPlant()
        c.bindTauDevice(0)
        b_.free()


# ------------------------------------------------------------------ 4. the draw
def test_randomize_equals_the_restatement(sp):
    depth, seed = 8, 0xC0FFEE123456789
    robot, ctrl, objs, mf, _ = _panda(B, False, ld=LD)
    ctrl.attachPlant()
    ctrl.attachActuationChain(np.tile(PC.NEUTRAL, (N, B, 1)), per_instance=True, depth=depth)
    lo, hi = np.tile([-0.4, 10.0, 0.0], (N, 1)), np.tile([depth + 0.4, 500.0, 0.01], (N, 1))
    lo[2], hi[2] = [3.0, np.inf, 0.002], [3.0, np.inf, 0.002]             # lo == hi: exact, +inf stays +inf
    lo[3, 0], hi[3, 0] = -7.0, 30.0                                       # far outside: clamped
    ctrl.actuationChainRandomize(seed, 4, lo, hi)
    ctrl.synchronize()
    got = _d2h(ctrl.actuationChainTableDevice(), (N, 3, LD))
    want = PC.draw(seed, 4, B, lo, hi, depth)                             # (N, B, 3)
    assert _same_bits(got[:, :, :B], np.ascontiguousarray(want.transpose(0, 2, 1)))
    assert not got[:, :, B:].any()                                        # columns B.. are never written (zero since the attach)
    dl = got[:, 0, :B]
    assert (dl == np.floor(dl)).all() and set(np.unique(dl[[0, 1, 4, 5, 6]])) == set(range(depth + 1))
    assert (got[2, :, :B] == np.array([3.0, np.inf, 0.002])[:, None]).all()
    ctrl.actuationChainRandomize(seed, 5, lo, hi)
    ctrl.synchronize()
    assert not _same_bits(_d2h(ctrl.actuationChainTableDevice(), (N, 3, LD)), got)               # another round: another table
    ctrl.rolloutAsync(2, DT, SUB, gravity=ZERO_G)                         # every drawn table is a valid one
    assert np.isfinite(_finals(ctrl)[0]).all()
    for word, val, msg in ((1, 0.0, "upper bound: joint 1: word rate_max = 0 is not above 0"), (2, -1.0, "upper bound: joint 1: word tau_lag = -1 is below 0"),
                           (1, np.inf, "joint 1: word rate_max has an infinite bound on one side only")):
        with pytest.raises(ValueError, match=msg):
            bad = hi.copy()
            bad[1, word] = val
            ctrl.actuationChainRandomize(seed, 4, lo, bad)
    ctrl.detachActuationChain()
    ctrl.attachActuationChain(depth=2)
    with pytest.raises(ValueError, match="batch-uniform"):
        ctrl.actuationChainRandomize(seed, 4, lo, hi)
    ctrl.detachPlant()


# ------------------------------------------------------------------ 5. rollout_async against the host-driven loop
@pytest.mark.parametrize("otg", [False, True])
@pytest.mark.parametrize("mode", ["plain", "contact", "sensing", "all"])
def test_rollout_equals_the_host_driven_loop(sp, otg, mode):
    """plain: config 2 behind a rough plant, { stepAsync, integrate }; contact: config 13 with contact planes and their sensor,
    { contactSense, stepAsync, integrate }; sensing: config 2 with a sensing model and a sensing chain as well, { measureState, stepAsync,
    integrate }; all: config 13 with a goal schedule and the recorder, one rollout period per call.  Every one with a per-instance actuation
    chain of depth 8 in front of the plant."""
    K, depth = 6, 8
    rng = np.random.default_rng(23)
    chain = _chain_table(rng, depth)
    plant = np.repeat(PL.neutral(N)[:, None, :], B, axis=1)
    plant[..., PL.GAIN], plant[..., PL.TAU_MAX], plant[..., PL.FV] = rng.uniform(0.9, 1.1, (N, B)), rng.uniform(5.0, 60.0, (N, B)), rng.uniform(0.0, 0.3, (N, B))
    sense, schain = _random_joint_table(rng, N, (), 2e-3), np.zeros((N, B, 4))
    schain[..., 0], schain[..., 3] = rng.integers(0, 5, (N, B)), SC.alpha(50.0, DT)
    dq0 = 0.1 * rng.uniform(-1, 1, (B, N))
    runs = []
    for host in (False, True):
        if mode in ("plain", "sensing"):
            robot, ctrl, objs, mf, _ = _panda(B, otg, ld=LD)
            robot.setDq(dq0)
            robot.updateModel()                                          # (pushes the state: stepAsync does not)
            ctrl.updateControllerTaskModels()
        else:
            robot, ctrl, objs = _cfg13(B, LD, otg)
            mf = objs[0]
            mf.attachContactPlanes(_table_under(robot, objs, 2e-3), sensor=True, per_instance=True)
        ctrl.attachPlant(plant, per_instance=True)
        ctrl.attachActuationChain(chain, per_instance=True, depth=depth)
        if mode == "sensing":
            ctrl.attachSensing(sense, seed=5)
            ctrl.attachSensingChain(schain, per_instance=True, depth=4, sample_time=DT)
        if mode == "all":
            g = mf._get_goal()[:, :3]
            mf.setGoalSchedule((0, 3), g[None] + np.linspace(0.0, 0.01, 3)[:, None, None] * np.array([1.0, -1.0, 0.0]), stride=2, mode="linear")
            ctrl.recordRollouts(K, 1, ("q", "dq", "tau"), task=mf)
        if not host:
            ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
        else:
            for k in range(K):
                if mode == "all":
                    ctrl.rolloutAsync(1, DT, SUB, gravity=ZERO_G)
                    continue
                if mode == "contact":
                    ctrl.contactSense()
                if mode == "sensing":
                    ctrl.setSensingPeriod(k)
                    ctrl.measureState()
                ctrl.stepAsync()
                ctrl.integrate(DT, SUB, gravity=ZERO_G)
        out = _finals(ctrl) + _state(ctrl) + [_act(ctrl), _summary(ctrl)]
        if mode == "sensing":
            st = ctrl.sensingChainState()
            out += list(ctrl.measuredState()) + [st["taps"], st["filt"]]
        if mode in ("contact", "all"):
            out += [mf._get_goal()]
        if mode == "all":
            log = ctrl.rolloutLog()
            out += [log["q"], log["dq"], log["tau"]]
            assert _same_bits(log["tau"][-1], out[2]) and not _same_bits(out[7], out[2])        # the recorder logs the commanded torques
        runs.append(out)
        ctrl.detachPlant()
    assert _equal(*runs)
    assert np.isfinite(runs[0][0]).all() and (runs[0][6] == 1).all()


# ------------------------------------------------------------------ 6. snapshots
def _chained(per=True, depth=8, otg=True):
    rng = np.random.default_rng(29)
    robot, ctrl, objs, mf, _ = _panda(B, otg, ld=LD)
    plant = np.repeat(PL.neutral(N)[:, None, :], B, axis=1) if per else PL.neutral(N)
    plant[..., PL.FV] = 0.05
    ctrl.attachPlant(plant, per_instance=per)
    ctrl.attachActuationChain(_chain_table(rng, depth, per=per), per_instance=per, depth=depth)
    return robot, ctrl, mf


def _roll(ctrl, K):
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    return _finals(ctrl) + _state(ctrl) + [_act(ctrl)]


def _chain_bytes(depth):
    return (depth * N + 3 * N) * LD * 8 + N * LD * 4


def test_snapshot_lists_the_chain_state(sp):
    robot, ctrl, mf = _chained()
    with_chain = ctrl.saveState()
    segs = {s["name"]: s for s in with_chain.segments()}
    for name, rows, elem in (("plant.chain.taps", 8 * N, 8), ("plant.chain.filt", 3 * N, 8), ("plant.chain.primed", N, 4)):
        assert (segs[name]["rows"], segs[name]["elem_bytes"], segs[name]["kind"]) == (rows, elem, "soa"), name
    assert [s["name"] for s in with_chain.segments()][-3:] == ["plant.chain.taps", "plant.chain.filt", "plant.chain.primed"]
    ctrl.detachActuationChain()
    without = ctrl.saveState()
    assert not [s["name"] for s in without.segments() if s["name"].startswith("plant.")]
    assert with_chain.nbytes() - without.nbytes() == _chain_bytes(8) == ((8 + 3) * 8 + 4) * N * LD
    ctrl.attachActuationChain(depth=0)
    flat = ctrl.saveState()
    names = [s["name"] for s in flat.segments()]
    assert "plant.chain.taps" not in names and names[-2:] == ["plant.chain.filt", "plant.chain.primed"]
    assert flat.nbytes() - without.nbytes() == _chain_bytes(0) == ctrl.actuationChainInfo()["state_bytes"]
    # both chains: the sensing chain's segments first, then the actuation chain's
    ctrl.attachSensing()
    ctrl.attachSensingChain(depth=0)
    assert [s["name"] for s in ctrl.saveState().segments()][-4:] == ["sense.chain.filt", "sense.chain.primed", "plant.chain.filt", "plant.chain.primed"]
    ctrl.detachSensing()
    ctrl.detachPlant()
    assert not [s["name"] for s in ctrl.saveState().segments() if s["name"].startswith("plant.")]


def test_snapshot_restore_repeats_the_continuation(sp):
    from sai_primitives_amd import StateSnapshot
    K = 5
    robot, ctrl, mf = _chained()
    before = ctrl.saveState()                                             # no period run yet: primed is 0 everywhere
    _roll(ctrl, K)
    snap = ctrl.saveState()                                               # the chain after K periods, the robot after K integrations
    first = _roll(ctrl, K)
    ctrl.restoreState(snap)
    again = _roll(ctrl, K)
    assert _equal(first, again) and not _same_bits(first[7], first[2]) and np.isfinite(first[0]).all()
    # through a host blob
    blob = snap.tobytes()
    _roll(ctrl, 2)
    s2 = StateSnapshot.frombytes(ctrl, blob)
    ctrl.restoreState(s2)
    assert _equal(first, _roll(ctrl, K))
    # the snapshot of the unprimed chain restores too: the run from the start repeats
    ctrl.restoreState(before)
    assert (ctrl.actuationChainState()["primed"] == 0).all()
    _roll(ctrl, K)
    assert _equal(first, _roll(ctrl, K))
    ctrl.detachPlant()


def test_snapshot_of_another_chain_layout_is_refused(sp):
    robot, ctrl, mf = _chained()
    _roll(ctrl, 3)
    deep = ctrl.saveState()
    ctrl.detachActuationChain()
    bare = ctrl.saveState()
    ctrl.attachActuationChain(dict(delay=2.0, tau_lag=0.002), depth=4)
    _roll(ctrl, 3)
    ctrl.synchronize()
    live = _finals(ctrl) + _state(ctrl)
    for snap, what in ((bare, r"segment \[plant\.chain\.taps\] is new"), (deep, r"segment \[plant\.chain\.taps\] where the snapshot has \[plant\.chain\.taps\]")):
        with pytest.raises(sp.SaipError, match=what):
            ctrl.restoreState(snap)
        with pytest.raises(sp.SaipError, match=r"plant\.chain\."):
            ctrl.saveState(snap)
    # nothing was restored or saved: the live state is what it was
    assert _equal(_finals(ctrl) + _state(ctrl), live)
    ctrl.detachActuationChain()
    with pytest.raises(sp.SaipError, match=r"segment \[plant\.chain\.taps\] is gone"):
        ctrl.restoreState(deep)
    assert _equal(_finals(ctrl), live[:4])
    ctrl.restoreState(bare)                                               # the layout it was taken from: accepted again
    ctrl.detachPlant()


def test_broadcast_restore_gives_every_instance_the_sources_history(sp):
    """batch-uniform tables, so that instance 69's continuation is what every instance must repeat; the bound is the one of
    tests/test_gpu_state_snapshot.py::test_permutation_and_broadcast_behave (1e-5 relative per joint, workloads.torque_error)"""
    K, TOL = 5, 1e-5
    robot, ctrl, mf = _chained(per=False)
    ctrl.setActuationChainTable(dict(delay=3.0, rate_max=4e3, tau_lag=10 * DT))
    _roll(ctrl, K)
    snap = ctrl.saveState()
    ref = _roll(ctrl, K)
    ctrl.restoreState(snap, 69)
    st = ctrl.actuationChainState()
    assert (st["primed"] == 1).all() and _same_bits(st["taps"], np.repeat(st["taps"][69:70], B, axis=0))    # primed travels with the column: no re-priming
    got = _roll(ctrl, K)
    worst = 0.0
    for k in (0, 1, 2, 4, 5, 7):                                          # q, dq, tau, taps, filter state, tau_act
        g, r = got[k].reshape(B, -1), ref[k].reshape(B, -1)
        worst = max(worst, W.torque_error(g, np.repeat(r[69:70], B, axis=0)))
    print(f"broadcast restore with an actuation chain: worst relative difference to instance 69's continuation {worst:.3e}")
    assert worst <= TOL and np.array_equal(got[3], np.repeat(ref[3][69:70], B, axis=0))
    assert W.torque_error(ref[0], np.repeat(ref[0][69:70], B, axis=0)) > 1e-3                              # (the instances did differ)
    ctrl.detachPlant()


# ------------------------------------------------------------------ 7. lifecycle
def test_lifecycle(sp):
    K = 4
    robot, ctrl, objs, mf, _ = _panda(B, True, ld=LD)
    with pytest.raises(sp.SaipError, match="no plant model is attached"):
        ctrl.attachActuationChain(depth=2)
    ctrl.attachPlant(dict_plant(ctrl))
    with pytest.raises(sp.SaipError, match="no actuation chain is attached"):
        ctrl.resetActuationChain()
    snap = ctrl.saveState()
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    plain = _finals(ctrl) + [_act(ctrl), _summary(ctrl)]
    ctrl.restoreState(snap)
    ctrl.resetPlantSummary()
    ctrl.attachActuationChain(dict(delay=2.0, rate_max=4e3, tau_lag=0.002), depth=2)
    with pytest.raises(sp.SaipError, match="already attached"):
        ctrl.attachActuationChain(depth=1)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    assert not _same_bits(_finals(ctrl)[0], plain[0])
    # a reset: the next period primes again, so a pure delay hands the plant that very command; a new table keeps the state
    before = ctrl.actuationChainState()
    ctrl.setActuationChainTable(dict(delay=2.0))
    after = ctrl.actuationChainState()
    assert all(_same_bits(np.asarray(before[k], float), np.asarray(after[k], float)) for k in before)
    buf, write = _bound(ctrl)
    rng = np.random.default_rng(3)
    t5, t6 = rng.uniform(-3, 3, (B, N)), rng.uniform(-3, 3, (B, N))
    ctrl.resetActuationChain()
    assert (ctrl.actuationChainState()["primed"] == 0).all()
    write(t5)
    ctrl.integrate(DT, SUB, gravity=ZERO_G)
    st = ctrl.actuationChainState()
    assert (st["primed"] == 1).all() and _same_bits(st["taps"], np.repeat(t5[:, :, None], 2, axis=2)) and _same_bits(st["filt"], np.repeat(t5[:, :, None], 3, axis=2))
    write(t6)
    ctrl.integrate(DT, SUB, gravity=ZERO_G)
    assert _same_bits(ctrl.actuationChainState()["filt"][..., 2], t5)    # (primed: the delay holds the first command)
    ctrl.bindTauDevice(0)
    buf.free()
    # after detaching the chain the results are the plant-only ones
    ctrl.detachActuationChain()
    assert ctrl.actuationChainTableDevice() is None and ctrl.actuationChainInfo()["attached"] is False
    ctrl.restoreState(snap)
    ctrl.resetPlantSummary()
    ctrl.setPlantPeriod(0)
    ctrl.rolloutAsync(K, DT, SUB, gravity=ZERO_G)
    assert _equal(_finals(ctrl) + [_act(ctrl), _summary(ctrl)], plain)
    # detaching the plant model detaches the chain
    ctrl.attachActuationChain(depth=3)
    ctrl.rolloutAsync(2, DT, SUB, gravity=ZERO_G)
    ctrl.detachPlant()                                                   # with a rollout in flight: the detach waits for it
    assert ctrl.actuationChainTableDevice() is None
    with pytest.raises(sp.SaipError, match="no plant model is attached"):
        ctrl.actuationChainInfo()
    ctrl.attachPlant()
    assert ctrl.actuationChainInfo()["attached"] is False
    ctrl.detachPlant()
    # device memory returns to its level: a batch large enough for a leaked array to show in the free-memory figure
    import ctypes as C
    from test_gpu_batch_layout import _hip

    def free_bytes():
        free, total = C.c_size_t(0), C.c_size_t(0)
        assert _hip().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    import gc
    Bb = 16384
    robot, ctrl, objs, mf, _ = _panda(Bb, False)
    gc.collect()                                                          # batches of earlier tests go now, not in the middle of the loop
    ctrl.attachPlant()
    rows = np.tile(PC.NEUTRAL, (N, Bb, 1))
    levels = []
    for k in range(21):
        ctrl.attachActuationChain(rows, per_instance=True, depth=8)
        ctrl.stepAsync()
        ctrl.integrate(DT, 1, gravity=ZERO_G)
        if k % 2:
            ctrl.detachActuationChain()
        else:
            ctrl.detachPlant()                                           # the other way out
            ctrl.attachPlant()
        levels.append(free_bytes())
    print("free device memory after each attach / detach pair:", levels)
    assert levels[-1] == levels[0] and levels[-2] == levels[1], levels   # 20 more pairs after the first (each way out): nothing is left behind


# ------------------------------------------------------------------ 7b. both chains at once: neither entry reaches into the other's state
def test_both_chains_together(sp):
    """Config 2 on the Panda, B = 70 at its own ld = 96, a sensing chain of depth 2 (2 * 2 * 7 tap rows) and an actuation chain of depth 3
    (3 * 7), non-neutral per-instance tables.  Every assertion is an equality between runs of one build: the snapshot directory against the
    two info calls; a reset or a detach of one chain against the other's state arrays; a restored continuation against the first."""
    from sai_primitives_amd import capi
    ld, ds, da, K, sub = 96, 2, 3, 3, 2
    rng = np.random.default_rng(41)
    robot, ctrl, objs, mf, _ = _panda(B, True)
    assert capi.lib().saip_batch_ld(ctrl._h) == ld
    robot.setDq(0.1 * rng.uniform(-1, 1, (B, N)))
    robot.updateModel()
    ctrl.updateControllerTaskModels()
    plant = np.repeat(PL.neutral(N)[:, None, :], B, axis=1)
    plant[..., PL.GAIN], plant[..., PL.FV] = rng.uniform(0.9, 1.1, (N, B)), rng.uniform(0.0, 0.3, (N, B))
    schain = np.zeros((N, B, 4))
    schain[..., 0], schain[..., 1] = rng.integers(0, ds + 1, (N, B)), rng.integers(0, 2, (N, B))
    schain[..., 2], schain[..., 3] = rng.choice([0.0, SC.alpha(50.0, DT)], (N, B)), SC.alpha(80.0, DT)
    achain = _chain_table(rng, da)
    ctrl.attachPlant(plant, per_instance=True)
    ctrl.attachSensing(_random_joint_table(rng, N, (), 2e-3), seed=5)
    ctrl.attachSensingChain(schain, per_instance=True, depth=ds, sample_time=DT)
    ctrl.attachActuationChain(achain, per_instance=True, depth=da)

    def sense():
        st = ctrl.sensingChainState()
        return [st["taps"], st["filt"], st["primed"]]

    def roll():
        ctrl.rolloutAsync(K, DT, sub, gravity=ZERO_G)
        return _finals(ctrl)[:3] + sense() + _state(ctrl)

    def names():
        return [s["name"] for s in ctrl.saveState().segments()]

    def refuses(stem, noun):
        """with only the other chain attached, every entry of this one answers with its own message (and writes nothing)"""
        from test_plant_chain_cpu import chain_calls
        for fn, status, msg in chain_calls(capi.lib(), ctrl._h, stem, B):
            assert status == capi.SAIP_ERR_ORDER and msg == f"{fn}: no {noun} is attached (saip_batch_{stem}_chain_attach)", (fn, msg)

    # 1. the directory lists both chains' state, each at the size its own info call reports
    segs = {s["name"]: s for s in ctrl.saveState().segments()}
    for prefix, rows, info in (("sense.chain.", 2 * ds * N, ctrl.sensingChainInfo()), ("plant.chain.", da * N, ctrl.actuationChainInfo())):
        mine = [segs[prefix + k] for k in ("taps", "filt", "primed")]
        assert [s["rows"] for s in mine] == [rows, 3 * N, N] and [s["elem_bytes"] for s in mine] == [8, 8, 4], prefix
        assert sum(s["rows"] * ld * s["elem_bytes"] for s in mine) == info["state_bytes"], prefix
        assert info["attached"] and info["per_instance"] and info["depth"] == (ds if prefix[0] == "s" else da)
    assert len([n for n in segs if ".chain." in n]) == 6
    # 2. a reset zeroes the chain's own primed and nothing else of either chain
    roll()
    s0, a0 = sense(), _state(ctrl)
    assert (s0[2] == 1).all() and (a0[2] == 1).all() and not (s0[0] == 0).all() and not (a0[0] == 0).all()
    ctrl.resetSensingChain()
    s1 = sense()
    assert (s1[2] == 0).all() and _equal(s1[:2], s0[:2]) and _equal(_state(ctrl), a0)
    roll()                                                                # both primed again
    s0, a0 = sense(), _state(ctrl)
    assert (s0[2] == 1).all() and (a0[2] == 1).all()
    ctrl.resetActuationChain()
    a1 = _state(ctrl)
    assert (a1[2] == 0).all() and _equal(a1[:2], a0[:2]) and _equal(sense(), s0)
    roll()
    # 3. a restored continuation repeats the first (the two period counters are not part of a snapshot)
    snap, periods = ctrl.saveState(), (ctrl.sensingInfo()["period"], ctrl.plantInfo()["period"])
    first = roll()
    ctrl.restoreState(snap)
    ctrl.setSensingPeriod(periods[0])
    ctrl.setPlantPeriod(periods[1])
    assert _equal(first, roll()) and np.isfinite(first[0]).all()
    # 4. a detach takes the chain's own three segments and leaves the other chain's info and state alone
    every = names()
    info, a0 = ctrl.actuationChainInfo(), _state(ctrl)
    ctrl.detachSensingChain()
    assert ctrl.actuationChainInfo() == info and _equal(_state(ctrl), a0)
    assert names() == [n for n in every if not n.startswith("sense.chain.")] and len(names()) == len(every) - 3
    refuses("sensing", "sensing chain")
    ctrl.attachSensingChain(schain, per_instance=True, depth=ds, sample_time=DT)
    roll()
    assert names() == every
    info, s0 = ctrl.sensingChainInfo(), sense()
    ctrl.detachActuationChain()
    assert ctrl.sensingChainInfo() == info and _equal(sense(), s0)
    assert names() == [n for n in every if not n.startswith("plant.chain.")] and len(names()) == len(every) - 3
    refuses("plant", "actuation chain")
    assert ctrl.sensingChainInfo() == info and _equal(sense(), s0)
    ctrl.detachSensing()
    ctrl.detachPlant()


# ------------------------------------------------------------------ 8. one closed-loop figure (printed and recorded in DESIGN.md 4.19, not asserted)
def test_closed_loop_under_command_delay_stays_finite_and_the_neutral_row_is_the_plant(sp):
    """A joint task alone at config 1's gains (kp 100, kv 20), gravity-free, a 0.2 rad step on every joint, 300 periods of 1 ms.  Instance i
    has a command delay of (0, 2, 4, 8)[i % 5] periods and a torque lag of 2 ms; i % 5 == 4 is the neutral row.  The test prints, per
    delay, the peak overshoot in per cent of the step and the RMS error of the last 100 periods over all joints of the instances with that
    delay; DESIGN.md 4.19 records the figures.  Asserted: every instance stays finite, and the neutral-row instances are the plant-only
    run bit for bit."""
    from sai_primitives_amd.controller import controller_from_specs
    K, T, step = 300, 1e-3, 0.2
    d = W.make_inputs(1, B)
    q0 = np.ascontiguousarray(np.broadcast_to(d["q"], (B, N)))           # config 1 has one posture: every instance starts there
    delays = np.array([0, 2, 4, 8, 0])
    group = np.arange(B) % 5
    table = np.tile(PC.NEUTRAL, (N, B, 1))
    table[:, :, 0] = delays[group]
    table[:, group < 4, 2] = 2e-3
    logs = []
    for chained in (False, True):
        robot, ctrl, objs = controller_from_specs(d["model"].name, d["tasks"], B, device=0, disable_otg=True, leading_dimension=LD)
        robot.setQ(q0)
        robot.setDq(np.zeros((B, N)))
        robot.updateModel()
        ctrl.reinitializeTasks()
        goal = q0 + step
        objs[0].setGoalPosition(goal)
        ctrl.updateControllerTaskModels()
        ctrl.attachPlant()
        if chained:
            ctrl.attachActuationChain(table, per_instance=True, depth=8)
        ctrl.recordRollouts(K, 1, ("q", "tau"))
        ctrl.rolloutAsync(K, T, 1, gravity=ZERO_G)
        ctrl.synchronize()
        log = ctrl.rolloutLog()
        logs.append((log["q"], log["tau"]))
        ctrl.detachPlant()
    q, tau = logs[1]
    err = q - goal[None]                                                  # (K, B, N)
    for g in range(5):
        e = err[:, group == g]
        over = max(e.max(), 0.0) / step
        rms = np.sqrt(np.mean(e[-100:] ** 2))
        what = "neutral row" if g == 4 else "lag 2 ms"
        print(f"closed loop, command delay {delays[g]} periods ({what}): peak overshoot {100 * over:.2f} % of the step, RMS error of the last 100 periods {rms:.3e} rad")
    assert np.isfinite(q).all() and np.isfinite(tau).all()
    assert _same_bits(q[:, group == 4], logs[0][0][:, group == 4]) and _same_bits(tau[:, group == 4], logs[0][1][:, group == 4])
