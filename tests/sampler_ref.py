"""NumPy restatement of the resident rollout sampler (csrc/saip_sampler.h / .hip, saip_batch_sampler_*): Philox4x32-10 and the uniforms
in integers and one exact scaling, Box-Muller, the perturbation of the keyframes (rotations on SO(3)), the cost formula and the softmin
update with the kernel's reduction shape.  Every array operation of NumPy rounds once in double precision and none is fused, which is
what the kernels do too (no FMA contraction): the restatement runs the kernel's operations in the kernel's order and differs from it only
by what log / sqrt / sin / cos / atan2 / exp of the two maths libraries differ."""
import numpy as np

LANES, WAVE = 256, 64
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------ random numbers
def philox4x32_10(ctr, key):
    """ctr (..., 4), key (2,) unsigned 32-bit -> (..., 4) words, held in uint64 (Random123's Philox4x32 with 10 rounds)"""
    c = [np.asarray(ctr)[..., j].astype(np.uint64) & MASK for j in range(4)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
    return np.stack(c, axis=-1)


def uniform(hi, lo):
    """(((hi >> 5) * 2^26 + (lo >> 6)) + 0.5) * 2^-53"""
    n = ((hi >> np.uint64(5)) << np.uint64(26)) + (lo >> np.uint64(6))
    return (n.astype(np.float64) + 0.5) * 2.0 ** -53


def counters(task, i, k, p, rnd):
    i = np.asarray(i, np.uint64)
    ctr = np.empty(i.shape + (4,), np.uint64)
    ctr[..., 0], ctr[..., 1], ctr[..., 2], ctr[..., 3] = i, k, (task << 16) | p, rnd & 0xFFFFFFFF
    return ctr


def uniforms(seed, rnd, task, i, k, p):
    w = philox4x32_10(counters(task, i, k, p, rnd), (seed & 0xFFFFFFFF, seed >> 32))
    return uniform(w[..., 0], w[..., 1]), uniform(w[..., 2], w[..., 3])


def noise(seed, rnd, task, B, K, d):
    """(K, B, d) standard normals: coordinates 2p, 2p + 1 of instance i, keyframe k from counter (i, k, (task << 16) | p, round)"""
    z = np.empty((K, B, d))
    i = np.arange(B)
    for k in range(K):
        for p in range((d + 1) // 2):
            u1, u2 = uniforms(seed, rnd, task, i, k, p)
            r, a = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
            z[k, :, 2 * p] = r * np.cos(a)
            if 2 * p + 1 < d:
                z[k, :, 2 * p + 1] = r * np.sin(a)
    return z


# ------------------------------------------------------------------ SO(3): the forms of goal_schedule_ref.slerp
def exp_apply(R0, v):
    """R0 Exp(v) for rotations (..., 3, 3) and rotation vectors (..., 3); v = 0 gives R0's bits"""
    R0, v = np.asarray(R0, float), np.asarray(v, float)
    shape = np.broadcast_shapes(R0.shape[:-2], v.shape[:-1])
    R0, v = np.broadcast_to(R0, shape + (3, 3)), np.broadcast_to(v, shape + (3,))
    ang = np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
    zero = ang == 0.0
    safe = np.where(zero, 1.0, ang)
    k = [v[..., 0] / safe, v[..., 1] / safe, v[..., 2] / safe]
    sa, ca = np.sin(ang), np.cos(ang)
    c1 = 1.0 - ca
    E = np.empty(shape + (3, 3))
    E[..., 0, 0] = (c1 * k[0]) * k[0] + ca
    E[..., 0, 1] = (c1 * k[0]) * k[1] - sa * k[2]
    E[..., 0, 2] = (c1 * k[0]) * k[2] + sa * k[1]
    E[..., 1, 0] = (c1 * k[1]) * k[0] + sa * k[2]
    E[..., 1, 1] = (c1 * k[1]) * k[1] + ca
    E[..., 1, 2] = (c1 * k[1]) * k[2] - sa * k[0]
    E[..., 2, 0] = (c1 * k[2]) * k[0] - sa * k[1]
    E[..., 2, 1] = (c1 * k[2]) * k[1] + sa * k[0]
    E[..., 2, 2] = (c1 * k[2]) * k[2] + ca
    out = np.empty(shape + (3, 3))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = (R0[..., i, 0] * E[..., 0, j] + R0[..., i, 1] * E[..., 1, j]) + R0[..., i, 2] * E[..., 2, j]
    out[zero] = R0[zero]
    return out


def log_so3(R0, R1):
    """Log(R0^T R1) as rotation vectors (..., 3)"""
    R0, R1 = np.asarray(R0, float), np.asarray(R1, float)
    M = np.empty(np.broadcast(R0, R1).shape)
    for i in range(3):
        for j in range(3):
            M[..., i, j] = (R0[..., 0, i] * R1[..., 0, j] + R0[..., 1, i] * R1[..., 1, j]) + R0[..., 2, i] * R1[..., 2, j]
    w = [0.5 * (M[..., 2, 1] - M[..., 1, 2]), 0.5 * (M[..., 0, 2] - M[..., 2, 0]), 0.5 * (M[..., 1, 0] - M[..., 0, 1])]
    sn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    cs = 0.5 * (((M[..., 0, 0] + M[..., 1, 1]) + M[..., 2, 2]) - 1.0)
    same = sn == 0.0
    safe = np.where(same, 1.0, sn)
    ang = np.arctan2(sn, cs)
    out = np.stack([ang * (w[e] / safe) for e in range(3)], axis=-1)
    out[same] = 0.0
    return out


def coords(count, r_rot):
    """(linear rows of the range, their sampler coordinates); r_rot: first of the nine rotation rows inside the range or None"""
    if r_rot is None:
        return np.arange(count), np.arange(count)
    rows = np.array([r for r in range(count) if not r_rot <= r < r_rot + 9])
    return rows, np.where(rows >= r_rot + 9, rows - 6, rows)


def dim(count, r_rot):
    return count if r_rot is None else count - 6


# ------------------------------------------------------------------ the three steps
def perturb(nominal, sigma, seed, rnd, task, B, exempt, r_rot=None, z=None):
    """keyframes (K, B, count) around the nominal plan (K, count); z: the normals (K, B, d) when they are given instead of drawn"""
    nominal, sigma = np.asarray(nominal, float), np.asarray(sigma, float)
    K, count = nominal.shape
    d = dim(count, r_rot)
    z = noise(seed, rnd, task, B, K, d) if z is None else z
    rows, js = coords(count, r_rot)
    keys = np.empty((K, B, count))
    keys[:, :, rows] = nominal[:, None, rows] + sigma[js] * z[:, :, js]
    if r_rot is not None:
        v = sigma[r_rot:r_rot + 3] * z[:, :, r_rot:r_rot + 3]
        keys[:, :, r_rot:r_rot + 9] = exp_apply(nominal[:, None, r_rot:r_rot + 9].reshape(K, 1, 3, 3), v).reshape(K, B, 9)
    keys[:, :exempt] = nominal[:, None]
    return keys


def cost(B, summary=None, w_summary=None, positions=None, target=None, w_path=0.0, w_final=0.0):
    """summary (8, B), positions (samples, B, 3) oldest first: the cost formula, left to right from 0"""
    c = np.zeros(B)
    if w_summary is not None:
        for r in range(8):
            if w_summary[r] != 0.0:
                c = c + w_summary[r] * summary[r]
    if target is not None:
        path, last = np.zeros(B), np.zeros(B)
        for p in positions:
            e = p - np.asarray(target, float)
            last = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
            path = path + last
        c = c + w_path * path
        c = c + w_final * last
    return c


def lane_sums(x):
    """x (B, ...) -> (256, ...): lane l adds instances l, l + 256, ... in that order, from 0"""
    x = np.asarray(x, float)
    acc = np.zeros((LANES,) + x.shape[1:])
    for m in range(0, x.shape[0], LANES):
        part = x[m:m + LANES]
        acc[:part.shape[0]] = acc[:part.shape[0]] + part
    return acc


def tree_sum(v):
    """(256, ...) lane values -> their sum in the kernel's shape: inside each group of 64 lanes v[l] += v[l + off] for off = 32 .. 1,
    then (g0 + g1) + (g2 + g3)"""
    v = np.array(v, float)
    for g in range(0, LANES, WAVE):
        off = WAVE // 2
        while off >= 1:
            v[g:g + off] = v[g:g + off] + v[g + off:g + 2 * off]
            off //= 2
    return (v[0] + v[WAVE]) + (v[2 * WAVE] + v[3 * WAVE])


def weights(costs, temperature):
    """(w (B,), result dict best, n_valid, min_cost, sum_w, ess)"""
    costs = np.asarray(costs, float)
    ok = np.isfinite(costs)
    n_valid = int(ok.sum())
    if n_valid == 0:
        return np.zeros(costs.shape), dict(best=-1, n_valid=0, min_cost=0.0, sum_w=0.0, ess=0.0)
    beta = costs[ok].min()
    best = int(np.flatnonzero(ok & (costs == beta))[0])
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.where(ok, np.exp(-((np.where(ok, costs, beta) - beta) / temperature)), 0.0)
    sw, sw2 = tree_sum(lane_sums(w)), tree_sum(lane_sums(w * w))
    return w, dict(best=best, n_valid=n_valid, min_cost=float(beta), sum_w=float(sw), ess=float((sw * sw) / sw2))


def update(nominal, keys, w, best, r_rot=None):
    """the new nominal plan (K, count) from keyframes (K, B, count) and weights (B,) with at least one finite cost behind them"""
    nominal, keys, w = np.array(nominal, float), np.asarray(keys, float), np.asarray(w, float)
    K, B, count = keys.shape
    sw, sw2 = tree_sum(lane_sums(w)), tree_sum(lane_sums(w * w))
    rows, _ = coords(count, r_rot)
    out = nominal.copy()
    for k in range(K):
        out[k, rows] = tree_sum(lane_sums(w[:, None] * keys[k][:, rows])) / sw
        if r_rot is not None:
            Rn = nominal[k, r_rot:r_rot + 9].reshape(3, 3)
            if sw == 1.0 and sw2 == 1.0:      # all the weight on one instance: its own rotation rows
                out[k, r_rot:r_rot + 9] = keys[k, best, r_rot:r_rot + 9]
            else:
                lg = log_so3(Rn, keys[k][:, r_rot:r_rot + 9].reshape(B, 3, 3))
                delta = tree_sum(lane_sums(w[:, None] * lg)) / sw
                out[k, r_rot:r_rot + 9] = exp_apply(Rn, delta).reshape(9)
    return out


def shift(nominal, n):
    nominal = np.asarray(nominal, float)
    K = nominal.shape[0]
    return nominal[np.minimum(np.arange(K) + n, K - 1)].copy()
