"""NumPy restatement of the plant model of the resident simulator (csrc/saip_plant.h / .hip, saip_batch_plant_*): actuator gain, offset
and saturation, viscous and Coulomb friction, penalty joint stops, external wrenches through the joints' world axes and origins, the running
summaries and the random draw of the per-instance tables.  Every array operation of NumPy rounds once in double precision and none is
fused, which is what the header does too (contraction off): the restatement runs the header's operations in the header's order and
reproduces it bit for bit.  Shapes are those of the Python facade: states (B, n), joint tables (n, 10) or (n, B, 10), wrench values (W, 8)
or (W, B, 8)."""
import numpy as np

import sampler_ref as SR

JOINT_WORDS, WRENCH_WORDS, MAX_WRENCHES, SUMMARY_ROWS = 10, 8, 4, 4
FRAME_WORLD, FRAME_LINK = 0, 1
TABLE_JOINTS, TABLE_WRENCHES = 0, 1
GAIN, BIAS, TAU_MAX, FV, FC, VS, Q_LO, Q_HI, K_STOP, C_STOP = range(10)


def pl_max(a, b):
    """a < b ? b : a: the first argument on a tie and whenever the comparison fails"""
    return np.where(np.less(a, b), b, a)


def pl_min(a, b):
    return np.where(np.less(b, a), b, a)


def neutral(n, q_lo=-np.inf, q_hi=np.inf):
    t = np.zeros((n, JOINT_WORDS))
    t[:, GAIN], t[:, TAU_MAX], t[:, Q_LO], t[:, Q_HI] = 1.0, np.inf, q_lo, q_hi
    return t


def _words(table):
    """the ten (or eight) words as arrays that broadcast against (B, n): (n,) from a batch-uniform table, (B, n) from a per-instance one"""
    table = np.asarray(table, float)
    return [table[..., k] if table.ndim == 2 else table[..., k].T for k in range(table.shape[-1])]


def joint(table, t, q, dq):
    """(tau, fr, st, clip), each (B, n): pl_joint for every joint of every instance"""
    gain, bias, tau_max, fv, fc, vs, q_lo, q_hi, ks, cs = _words(table)
    t, q, dq = (np.asarray(a, float) for a in (t, q, dq))
    with np.errstate(all="ignore"):
        u0 = np.where(t == t, t, 0.0)
        u1 = gain * u0 + bias
        u2 = pl_min(pl_max(u1, -tau_max), tau_max)
        coul = np.where(fc > 0.0, (fc * dq) / pl_max(np.abs(dq), np.where(fc > 0.0, vs, 1.0)), 0.0)
        fr = fv * dq + coul
        below = pl_max(0.0, ks * (q_lo - q) - cs * dq)
        above = -pl_max(0.0, ks * (q - q_hi) + cs * dq)
        st = np.where(q < q_lo, below, np.where(q > q_hi, above, 0.0))
        tau = (u2 - fr) + st
        clip = np.abs(u1 - u2)
    return tau, fr, st, clip


def fold(fr, st, clip, dq):
    """(work_fr, clip_max, acted), each (B,): the joints folded in ascending order"""
    B, n = fr.shape
    work, cmax, acted = np.zeros(B), np.zeros(B), np.zeros(B, bool)
    for j in range(n):
        work = work + np.abs(fr[:, j] * dq[:, j])
        cmax = pl_max(cmax, clip[:, j])
        acted |= (clip[:, j] > 0.0) | (st[:, j] != 0.0)
    return work, cmax, acted


def wrench_acts(values, period):
    """(W, B) bool from values (W, 8) or (W, B, 8)"""
    v = np.asarray(values, float)
    p = float(period)
    a = (v[..., 6] <= p) & (p < v[..., 7])
    return a if v.ndim == 3 else a[:, None]


def wrench_world(vals, frame, Rl):
    """F, M (B, 3) of one wrench: vals (8,) or (B, 8), Rl (B, 3, 3) the link's world rotation"""
    vals = np.asarray(vals, float)
    B = Rl.shape[0]
    f, m = np.broadcast_to(vals[..., 0:3], (B, 3)), np.broadcast_to(vals[..., 3:6], (B, 3))
    if frame == FRAME_WORLD:
        return f.copy(), m.copy()
    F = np.stack([(Rl[:, i, 0] * f[:, 0] + Rl[:, i, 1] * f[:, 1]) + Rl[:, i, 2] * f[:, 2] for i in range(3)], axis=1)
    M = np.stack([(Rl[:, i, 0] * m[:, 0] + Rl[:, i, 1] * m[:, 1]) + Rl[:, i, 2] * m[:, 2] for i in range(3)], axis=1)
    return F, M


def wrench_torque(revolute, aw, oj, p, F, M):
    """(B,): aw . ((p - oj) x F + M) of a revolute joint, aw . F of a prismatic one"""
    if not revolute:
        return (aw[:, 0] * F[:, 0] + aw[:, 1] * F[:, 1]) + aw[:, 2] * F[:, 2]
    r = p - oj
    m0 = (r[:, 1] * F[:, 2] - r[:, 2] * F[:, 1]) + M[:, 0]
    m1 = (r[:, 2] * F[:, 0] - r[:, 0] * F[:, 2]) + M[:, 1]
    m2 = (r[:, 0] * F[:, 1] - r[:, 1] * F[:, 0]) + M[:, 2]
    return (aw[:, 0] * m0 + aw[:, 1] * m1) + aw[:, 2] * m2


def apply(joints, t, q, dq, summary, dt, period=0, wrenches=None, frames=(), anc=(), rev=None, aw=None, oj=None, p=None, Rl=None):
    """one substep: (tau_act (B, n), the advanced summary (B, 4)).  Wrenches need the kinematics: rev (n,) bool, aw and oj (B, n, 3) the
    joints' world axes and origins, anc[w] the bit mask of the ancestor joints of wrench w's link, p (B, W, 3), Rl (B, W, 3, 3)"""
    tau, fr, st, clip = joint(joints, t, q, dq)
    work_fr, cmax, acted = fold(fr, st, clip, dq)
    B, n = tau.shape
    work_ext = np.zeros(B)
    tau = tau.copy()
    if wrenches is not None and len(wrenches):
        wrenches = np.asarray(wrenches, float)
        acts = wrench_acts(wrenches, period)
        for w in range(wrenches.shape[0]):
            if anc[w] == 0:
                continue
            on = np.broadcast_to(acts[w], (B,))
            F, M = wrench_world(wrenches[w], frames[w], Rl[:, w])
            for j in range(n):
                if not (anc[w] >> j) & 1:
                    continue
                with np.errstate(all="ignore"):
                    x = wrench_torque(bool(rev[j]), aw[:, j], oj[:, j], p[:, w], F, M)
                    tau[:, j] = np.where(on, tau[:, j] + x, tau[:, j])
                    work_ext = np.where(on, work_ext + x * dq[:, j], work_ext)
    s = np.asarray(summary, float).copy()
    with np.errstate(all="ignore"):
        s[:, 0] = s[:, 0] + dt * work_fr
        s[:, 1] = pl_max(s[:, 1], cmax)
        s[:, 2] = s[:, 2] + np.where(acted, 1.0, 0.0)
        s[:, 3] = s[:, 3] + dt * work_ext
    return tau, s


def draw(seed, rnd, table, B, lo, hi):
    """(rows, B, words): word w = words * row + k of instance i is lo + u (hi - lo), clamped to the interval, u the first uniform of Philox
    counter (i, w, table, round); lo == hi gives lo; the window words of the wrench table are floored"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    rows, words = lo.shape
    out = np.empty((rows, B, words))
    i = np.arange(B, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for r in range(rows):
        for k in range(words):
            ctr = np.empty((B, 4), np.uint64)
            ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = i, r * words + k, table, rnd & 0xFFFFFFFF
            x = SR.philox4x32_10(ctr, key)
            u = SR.uniform(x[:, 0], x[:, 1])
            l, h = lo[r, k], hi[r, k]
            if l == h:
                v = np.full(B, l)
            else:
                with np.errstate(all="ignore"):
                    v = l + u * (h - l)
                v = pl_min(pl_max(v, min(l, h)), max(l, h))
            if table == TABLE_WRENCHES and k >= 6:
                v = np.floor(v)
            out[r, :, k] = v
    return out
