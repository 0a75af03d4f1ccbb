"""NumPy restatement of the resident inertia table of the simulator (csrc/saip_inertia.h / .hip, saip_batch_inertia_*): a movable body's
row { m, c (3), I (6: xx yy zz xy xz yz) } composed from the model's row scaled and shifted plus up to two box payloads, and the random
draw of the parts.  Every array operation of NumPy rounds once in double precision and none is fused, which is what the header does too
(contraction off): the restatement runs the header's operations in the header's order and reproduces it bit for bit.  Shapes are those of
the Python facade: rows (n, 10) or (n, B, 10), bodies (n, 4) or (n, B, 4), payloads (P, 7) or (P, B, 7).

Also what the tests need around it: the rows and link frames of a robot description merged in NumPy (model_rows), and a description with
one instance's inertial parameters for the per-link Lagrangian oracle (instance_description)."""
import copy

import numpy as np

import sampler_ref as SR

ROW_WORDS, BODY_WORDS, PAYLOAD_WORDS, MAX_PAYLOADS = 10, 4, 7, 2
TABLE_BODIES, TABLE_PAYLOADS = 2, 3
IJ = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]                      # the six inertia words as matrix entries


def neutral_bodies(n):
    t = np.zeros((n, BODY_WORDS))
    t[:, 0] = 1.0
    return t


def parallel_axis(d):
    """PA(d) = (d.d) 1 - d d^T as six words, d (B, 3) -> (B, 6)"""
    xx, yy, zz = d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2]
    dd = (xx + yy) + zz
    return np.stack([dd - xx, dd - yy, dd - zz, -(d[:, 0] * d[:, 1]), -(d[:, 0] * d[:, 2]), -(d[:, 1] * d[:, 2])], axis=1)


def _per_instance(t, B):
    """(rows, words) or (rows, B, words) -> (rows, B, words)"""
    t = np.asarray(t, float)
    return np.ascontiguousarray(np.broadcast_to(t[:, None, :], (t.shape[0], B, t.shape[1]))) if t.ndim == 2 else t


def compose(model_rows, bodies, payloads, site_body, site_pos, site_rot, B):
    """rows (n, B, 10): in_compose_row for every body of every instance"""
    model_rows = np.asarray(model_rows, float)
    n = model_rows.shape[0]
    bodies = _per_instance(bodies, B)
    P = len(site_body)
    payloads = _per_instance(payloads, B) if P else np.zeros((0, B, PAYLOAD_WORDS))
    out = np.empty((n, B, ROW_WORDS))
    # the payloads in their bodies' frames
    mp, cp, Ip = [], [], []
    for p in range(P):
        w, R, pos = payloads[p], np.asarray(site_rot[p], float), np.asarray(site_pos[p], float)
        m, cl, hx, hy, hz = w[:, 0], w[:, 1:4], w[:, 4], w[:, 5], w[:, 6]
        cp.append(np.stack([pos[i] + ((R[i, 0] * cl[:, 0] + R[i, 1] * cl[:, 1]) + R[i, 2] * cl[:, 2]) for i in range(3)], axis=1))
        a, xx, yy, zz = m / 3.0, hx * hx, hy * hy, hz * hz
        D = [a * (yy + zz), a * (xx + zz), a * (xx + yy)]
        Ip.append(np.stack([((R[i, 0] * D[0]) * R[k, 0] + (R[i, 1] * D[1]) * R[k, 1]) + (R[i, 2] * D[2]) * R[k, 2] for i, k in IJ], axis=1))
        mp.append(m)
    for j in range(n):
        s = bodies[j, :, 0]
        m1 = s * model_rows[j, 0]
        c1 = model_rows[j, 1:4] + bodies[j, :, 1:4]
        I1 = s[:, None] * model_rows[j, 4:10]
        on = [(mp[p] > 0.0) if site_body[p] == j else np.zeros(B, bool) for p in range(P)]
        m = m1
        for p in range(P):
            m = np.where(on[p], m + mp[p], m)
        h = m1[:, None] * c1
        for p in range(P):
            h = np.where(on[p][:, None], h + mp[p][:, None] * cp[p], h)
        with np.errstate(all="ignore"):
            c = h / m[:, None]
            I = I1 + m1[:, None] * parallel_axis(c1 - c)
            for p in range(P):
                I = np.where(on[p][:, None], I + (Ip[p] + mp[p][:, None] * parallel_axis(cp[p] - c)), I)
        some = np.zeros(B, bool)
        for p in range(P):
            some |= on[p]
        out[j, :, 0] = np.where(some, m, m1)
        out[j, :, 1:4] = np.where(some[:, None], c, c1)
        out[j, :, 4:10] = np.where(some[:, None], I, I1)
    return out


def draw(seed, rnd, table, B, lo, hi):
    """(rows, B, words): word w = words * row + k of instance i is lo + u (hi - lo), clamped to the interval, u the first uniform of Philox
    counter (i, w, table, round); lo == hi gives lo"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    rows, words = lo.shape
    out = np.empty((rows, B, words))
    i = np.arange(B, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    for r in range(rows):
        for k in range(words):
            l, h = lo[r, k], hi[r, k]
            if l == h:
                out[r, :, k] = l
                continue
            ctr = np.empty((B, 4), np.uint64)
            ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3] = i, r * words + k, table, rnd & 0xFFFFFFFF
            x = SR.philox4x32_10(ctr, key)
            u = SR.uniform(x[:, 0], x[:, 1])
            v = l + u * (h - l)
            a, b = min(l, h), max(l, h)
            v = np.where(v < a, a, v)
            out[r, :, k] = np.where(b < v, b, v)
    return out


def randomized(model_rows, seed, rnd, B, body_bounds, payload_bounds, site_body, site_pos, site_rot):
    """what saip_batch_inertia_randomize leaves in the table: (rows (n, B, 10), drawn bodies (n, B, 4), drawn payloads (P, B, 7))"""
    n, P = np.asarray(model_rows).shape[0], len(site_body)
    bl, bh = body_bounds if body_bounds is not None else (neutral_bodies(n), neutral_bodies(n))
    pl, ph = payload_bounds if payload_bounds is not None else (np.zeros((P, PAYLOAD_WORDS)), np.zeros((P, PAYLOAD_WORDS)))
    bodies = draw(seed, rnd, TABLE_BODIES, B, bl, bh)
    payloads = draw(seed, rnd, TABLE_PAYLOADS, B, pl, ph) if P else np.zeros((0, B, PAYLOAD_WORDS))
    return compose(model_rows, bodies, payloads, site_body, site_pos, site_rot, B), bodies, payloads


def sym(I6):
    """(..., 6) -> (..., 3, 3)"""
    I6 = np.asarray(I6, float)
    M = np.empty(I6.shape[:-1] + (3, 3))
    for e, (i, k) in enumerate(IJ):
        M[..., i, k] = M[..., k, i] = I6[..., e]
    return M


# ------------------------------------------------------------------ a robot description in NumPy
def _rot_rpy(rpy):
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return (np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]]) @ np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]]) @
            np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]]))


def link_frames(links, parents=None):
    """per link: (movable body or -1, R, p) -- the link's frame in its movable body (a movable link: identity, zero)"""
    out = []
    for li, l in enumerate(links):
        pa = (li - 1) if parents is None else parents[li]
        body, Rp, pp = (-1, np.eye(3), np.zeros(3)) if pa < 0 else out[pa]
        if l["joint_type"] == "fixed":
            out.append((body, Rp @ _rot_rpy(l["origin_rpy"]), pp + Rp @ np.asarray(l["origin_xyz"], float)))
        else:
            out.append((1 + max([b for b, _, _ in out], default=-1), np.eye(3), np.zeros(3)))
    return out


def model_rows(links, parents=None):
    """(n, 10): the rows of the movable bodies, every welded link merged into its body (to rounding what the engine's model holds)"""
    frames = link_frames(links, parents)
    n = 1 + max(b for b, _, _ in frames)
    rows = np.zeros((n, ROW_WORDS))
    for j in range(n):
        parts = []
        for l, (b, R, p) in zip(links, frames):
            if b == j:
                parts.append((l["mass"], p + R @ np.asarray(l["com"], float), R @ sym(l["inertia"]) @ R.T))
        m = sum(x[0] for x in parts)
        if m > 0:
            c = sum(x[0] * x[1] for x in parts) / m
            I = sum(x[2] + x[0] * sym(parallel_axis((x[1] - c)[None])[0]) for x in parts)
        else:
            c, I = parts[0][1], np.zeros((3, 3))
        rows[j, 0], rows[j, 1:4] = m, c
        rows[j, 4:10] = [I[i, k] for i, k in IJ]
    return rows


def box_inertia(m, h):
    return m / 3.0 * np.diag([h[1] ** 2 + h[2] ** 2, h[0] ** 2 + h[2] ** 2, h[0] ** 2 + h[1] ** 2])


def instance_description(desc, bodies, payloads, payload_links, parents=None):
    """a deep copy of the description `desc` whose links carry one instance's inertial parameters, link by link (nothing is merged here:
    the per-link oracle does its own sums).  bodies (n, 4): every link of body j has its mass and inertia scaled by s_j and its COM
    shifted by d_j (given in the body frame, so rotated into the link's own).  payloads (P, 7): the box joins the inertial of its site
    link, in that link's own frame."""
    d = copy.deepcopy(desc)
    links = d["links"]
    frames = link_frames(links, parents)
    for l, (b, R, _) in zip(links, frames):
        if b < 0:
            continue
        s, dj = bodies[b][0], np.asarray(bodies[b][1:4], float)
        l["mass"] = float(s * l["mass"])
        l["inertia"] = [float(s * x) for x in l["inertia"]]
        l["com"] = [float(x) for x in np.asarray(l["com"], float) + R.T @ dj]
    names = [l["name"] for l in links]
    for p, name in enumerate(payload_links):
        mp, cp, h = payloads[p][0], np.asarray(payloads[p][1:4], float), payloads[p][4:7]
        if not mp > 0:
            continue
        l = links[names.index(name)]
        m0, c0, I0 = l["mass"], np.asarray(l["com"], float), sym(l["inertia"])
        m = m0 + mp
        c = (m0 * c0 + mp * cp) / m
        I = I0 + m0 * sym(parallel_axis((c0 - c)[None])[0]) + box_inertia(mp, h) + mp * sym(parallel_axis((cp - c)[None])[0])
        l["mass"], l["com"], l["inertia"] = float(m), [float(x) for x in c], [float(I[i, k]) for i, k in IJ]
    return d
