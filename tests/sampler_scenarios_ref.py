"""NumPy restatement of the sampler's scenario groups (csrc/saip_sampler.h: samp_perturb_candidate, samp_group_cost, samp_group_map): a
batch of B = C * M instances is M scenario blocks of C candidate plans, instance i = s * C + c.  Built on sampler_ref.py: the grouped
perturb is the ungrouped one of a batch of C tiled over the blocks, weights and update are the ungrouped ones over the C group costs and
block 0 of the keyframes.  Every operation rounds once and none is fused, as in the kernels."""
import numpy as np

import sampler_ref as SR

RISKS = {"mean": 0, "max": 1, "cvar": 2}
MAX_SCENARIOS = 64


def tail_of(M, alpha):
    """the scenarios CVAR averages: min(M, max(1, ceil(alpha * M)))"""
    return min(M, max(1, int(np.ceil(alpha * M))))


def perturb(nominal, sigma, seed, rnd, task, C, M, exempt, r_rot=None):
    """keyframes (K, C * M, count): the noise and the exempt test are keyed by the candidate, so every block is block 0"""
    block = SR.perturb(nominal, sigma, seed, rnd, task, C, exempt, r_rot)
    return np.ascontiguousarray(np.tile(block, (1, M, 1)))


def group_cost(costs, C, M, risk, tail=0):
    """(C,) group costs from the (C * M,) per-instance costs.  +inf where a scenario cost is not finite; "mean": added in scenario
    order from 0.0, / M; "max": the largest (as 0.0 + v); "cvar": the `tail` largest added in descending order from 0.0, / tail"""
    v = np.asarray(costs, float).reshape(M, C)
    bad = ~np.isfinite(v).all(axis=0)
    safe = np.where(bad[None], 0.0, v)
    if risk == "mean":
        acc = np.zeros(C)
        for s in range(M):
            acc = acc + safe[s]
        g = acc / float(M)
    elif risk == "max":
        g = 0.0 + safe.max(axis=0)
    elif risk == "cvar":
        assert 1 <= tail <= M
        order = -np.sort(-safe, axis=0)          # descending; equal values have equal bits but for the sign of zero, which 0.0 + v absorbs
        acc = np.zeros(C)
        for t in range(tail):
            acc = acc + order[t]
        g = acc / float(tail)
    else:
        raise ValueError(risk)
    return np.where(bad, np.inf, g)


def best_map(B, C, best):
    i = np.arange(B)
    return np.full(B, -1, np.int32) if best < 0 else ((i // C) * C + best).astype(np.int32)


def weights(costs, C, M, risk, tail, temperature):
    """(group cost (C,), w (C,), result dict over candidates, best map (C * M,))"""
    g = group_cost(costs, C, M, risk, tail)
    w, res = SR.weights(g, temperature)
    return g, w, res, best_map(C * M, C, res["best"])


def update(nominal, keys, w, best, C, r_rot=None):
    """the new nominal from block 0 of the keyframes (K, C * M, count) and the candidates' weights (C,)"""
    return SR.update(nominal, np.asarray(keys)[:, :C], w, best, r_rot)
