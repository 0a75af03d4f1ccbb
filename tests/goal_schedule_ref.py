"""NumPy restatement of the goal schedules (csrc/saip_goal_schedule.hip, saip_batch_goal_schedule_*): the index / fraction rule of a
period, the component-wise interpolation and the interpolation of the rotation rows on SO(3).  Every array operation of NumPy rounds
once in double precision and none is fused, which is what the kernel does too (no FMA contraction): `lerp` gives the kernel's bits; `slerp`
runs the kernel's operations in the kernel's order and differs from it only by what sqrt / atan2 / sin / cos of the two maths libraries
differ."""
import numpy as np

HOLD, LINEAR = "hold", "linear"


def index_fraction(c, n_keyframes, stride):
    """keyframe i and fraction s of period c: i = c // stride, s = (c % stride) / stride; the last keyframe is held"""
    if c >= (n_keyframes - 1) * stride:
        return n_keyframes - 1, 0.0
    return c // stride, (c % stride) / float(stride)


def lerp(a, b, s):
    return a + s * (b - a)


def slerp(R0, R1, s):
    """R0 Exp(s Log(R0^T R1)) for (..., 3, 3) rotations at most pi - 1e-3 apart"""
    R0, R1 = np.asarray(R0, float), np.asarray(R1, float)
    M = np.empty(np.broadcast(R0, R1).shape)
    for i in range(3):
        for j in range(3):
            M[..., i, j] = (R0[..., 0, i] * R1[..., 0, j] + R0[..., 1, i] * R1[..., 1, j]) + R0[..., 2, i] * R1[..., 2, j]
    w = [0.5 * (M[..., 2, 1] - M[..., 1, 2]), 0.5 * (M[..., 0, 2] - M[..., 2, 0]), 0.5 * (M[..., 1, 0] - M[..., 0, 1])]
    sn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    cs = 0.5 * (((M[..., 0, 0] + M[..., 1, 1]) + M[..., 2, 2]) - 1.0)
    ang = s * np.arctan2(sn, cs)
    same = sn == 0.0
    safe = np.where(same, 1.0, sn)
    k = [w[0] / safe, w[1] / safe, w[2] / safe]
    sa, ca = np.sin(ang), np.cos(ang)
    v = 1.0 - ca
    E = np.empty_like(M)
    E[..., 0, 0] = (v * k[0]) * k[0] + ca
    E[..., 0, 1] = (v * k[0]) * k[1] - sa * k[2]
    E[..., 0, 2] = (v * k[0]) * k[2] + sa * k[1]
    E[..., 1, 0] = (v * k[1]) * k[0] + sa * k[2]
    E[..., 1, 1] = (v * k[1]) * k[1] + ca
    E[..., 1, 2] = (v * k[1]) * k[2] - sa * k[0]
    E[..., 2, 0] = (v * k[2]) * k[0] - sa * k[1]
    E[..., 2, 1] = (v * k[2]) * k[1] + sa * k[0]
    E[..., 2, 2] = (v * k[2]) * k[2] + ca
    out = np.empty_like(M)
    for i in range(3):
        for j in range(3):
            out[..., i, j] = (R0[..., i, 0] * E[..., 0, j] + R0[..., i, 1] * E[..., 1, j]) + R0[..., i, 2] * E[..., 2, j]
    out[same] = np.broadcast_to(R0, M.shape)[same]
    return out


def rows(keyframes, c, stride, mode, rot_at=None):
    """the scheduled goal rows of period c: keyframes (K, ..., count) -> (..., count).  rot_at: index inside the range of the first of
    the nine rotation rows (3 - first for a linear schedule over rows 3..11 of a motion-force task), None: no rotation rows"""
    keyframes = np.asarray(keyframes, float)
    i, s = index_fraction(c, keyframes.shape[0], stride)
    if mode == HOLD or s == 0.0:
        return keyframes[i].copy()
    a, b = keyframes[i], keyframes[i + 1]
    out = lerp(a, b, s)
    if rot_at is not None:
        lead = a.shape[:-1]
        R = slerp(a[..., rot_at:rot_at + 9].reshape(lead + (3, 3)), b[..., rot_at:rot_at + 9].reshape(lead + (3, 3)), s)
        out[..., rot_at:rot_at + 9] = R.reshape(lead + (9,))
    return out


def exp_so3(w):
    """Rodrigues' formula for rotation vectors (..., 3) (test inputs)"""
    w = np.asarray(w, float)
    th = np.linalg.norm(w, axis=-1)[..., None, None]
    k = w / np.where(th[..., 0] == 0, 1.0, th[..., 0])
    K = np.zeros(w.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0], K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 2], k[..., 1], k[..., 2], -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)
