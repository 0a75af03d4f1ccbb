"""NumPy restatement of the environment schedules of sai-primitives_amd/csrc/saip_env_schedule.h and of the moving-surface contact
arithmetic of csrc/saip_contact.h / saip_contact_patch.h (ct_plane_forces_moving, cp_slot_eval_moving), on top of contact_ref.py and
contact_patch_ref.py.

Every product and every sum is one NumPy operation, in the order the headers write them.  Keyframes are (K, n_items, W) for a batch-uniform
table and (K, n_items, W, B) for a per-instance one: W = 8 for obstacles { kind, a[3], b[3], r }, W = 12 for planes
{ n[3], offset, k, c, mu, v_s, u[3], 0 }."""
import numpy as np

import contact_patch_ref as CP
import contact_ref as CR

MAX_SCHEDULES, OBSTACLE_WORDS, PLANE_WORDS, TABLE_WORDS, VELOCITY_WORDS = 4, 8, 12, 8, 4
TARGET_OBSTACLES, TARGET_PLANES, TARGET_PATCH = 0, 1, 2
HOLD, LINEAR = 0, 1
HALF_SPACE = 1.0


def timing(x, K, stride, mode):
    """keyframe index i, fraction s and whether the schedule is between two keyframes, for the period index x it sees"""
    past = x >= (K - 1) * stride
    i = K - 1 if past else x // stride
    s = 0.0 if past else float(x % stride) / float(stride)
    return i, s, (mode == LINEAR and not past)


def period_index(c, planes):
    """contact targets see the rollout period c, the clearance target c + 1"""
    return c if planes else c + 1


def lerp(a, b, s):
    return a + s * (b - a)


def rows(key, planes, x, stride, mode, T):
    """the table rows (n_items, 8[, B]) and, for planes, the velocity rows (n_items, 4[, B]) (else None) a schedule that sees the period
    index x writes; T: the length of a period"""
    key = np.asarray(key, float)
    K = key.shape[0]
    i, s, moving = timing(x, K, stride, mode)
    a = key[i]
    b = key[i + 1] if moving else a
    n0 = 0 if planes else 1
    w = a.copy()
    if moving and s != 0.0:
        w = lerp(a, b, s)
        if not planes:
            w[:, 0] = a[:, 0]
        m = w[:, n0:n0 + 3]
        nn = np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])
        unit = m / nn[:, None]
        normal = np.ones_like(nn, bool) if planes else (a[:, 0] == HALF_SPACE)
        w[:, n0:n0 + 3] = np.where(normal[:, None], unit, m)
    table = w[:, :TABLE_WORDS].copy()
    if not planes:
        return table, None
    span = float(stride) * T
    wn = (b[:, 3] - a[:, 3]) / span if moving else np.zeros_like(a[:, 3])
    vp = w[:, 8:11] + wn[:, None] * w[:, 0:3]
    return table, np.concatenate([vp, wn[:, None]], axis=1)


def plane_forces_moving(planes, vel, p, v):
    """contact_ref.plane_forces against planes that move with vel (N, P, 4) or (P, 4): v - v_p takes the place of v, per plane"""
    p, v = np.atleast_2d(np.asarray(p, float)), np.atleast_2d(np.asarray(v, float))
    N = p.shape[0]
    planes = np.broadcast_to(np.asarray(planes, float), (N,) + np.asarray(planes).shape[-2:])
    vel = np.broadcast_to(np.asarray(vel, float), (N,) + np.asarray(vel).shape[-2:])
    f, fn_sum, dmin, active = np.zeros((N, 3)), np.zeros(N), np.zeros(N), np.zeros(N, int)
    for k in range(planes.shape[1]):
        w = planes[:, k]
        n, off, ks, cd, mu, vs = w[:, 0:3], w[:, 3], w[:, 4], w[:, 5], w[:, 6], w[:, 7]
        d = CR.dot(n, p) - off
        dmin = d.copy() if k == 0 else np.where(d < dmin, d, dmin)
        on = d < 0.0
        vr = v - vel[:, k, 0:3]
        vn = CR.dot(n, vr)
        fn = np.maximum(0.0, -ks * d - cd * vn)
        vt = vr - vn[:, None] * n
        s = np.maximum(np.sqrt(CR.dot(vt, vt)), vs)
        g = mu * fn
        ft = -(g[:, None] * vt) / s[:, None]
        fk = f + (fn[:, None] * n + ft)
        f = np.where(on[:, None], fk, f)
        fn_sum = np.where(on, fn_sum + fn, fn_sum)
        active = active + on
    return f, fn_sum, dmin, active


def slots_moving(planes, vel, xc, Rc, points, tv, tw, tc):
    """contact_patch_ref.slots against moving planes"""
    N, n = xc.shape[0], len(points)
    out = dict(p=np.zeros((N, 8, 3)), f=np.zeros((N, 8, 3)), m=np.zeros((N, 8, 3)), fn_sum=np.zeros((N, 8)), dcand=np.full((N, 8), np.inf),
               active=np.zeros((N, 8), int))
    for i in range(n):
        r = np.broadcast_to(np.asarray(points[i], float), (N, 3))
        p = CR.point(xc, Rc, r)
        v = CR.velocity(tv, tw, tc, p)
        f, fn_sum, dmin, active = plane_forces_moving(planes, vel, p, v)
        out["p"][:, i], out["f"][:, i], out["m"][:, i] = p, f, CR.cross(p - xc, f)
        out["fn_sum"][:, i], out["dcand"][:, i], out["active"][:, i] = fn_sum, dmin, active
    return out


def plane_key(n, offset, k, c=0.0, mu=0.0, vs=1e-3, u=(0.0, 0.0, 0.0)):
    """one plane keyframe row, the normal normalised the way the engine does it"""
    return np.concatenate([CR.plane(n, offset, k, c, mu, vs), np.asarray(u, float), [0.0]])


def normalise_plane_keys(key):
    """plane keyframes (K, n, 12[, B]) as the engine keeps them: n / sqrt((n0 n0 + n1 n1) + n2 n2)"""
    key = np.array(key, float)
    n = key[:, :, 0:3]
    nn = np.sqrt(n[:, :, 0] * n[:, :, 0] + n[:, :, 1] * n[:, :, 1] + n[:, :, 2] * n[:, :, 2])
    key[:, :, 0:3] = n / nn[:, :, None]
    return key
