"""NumPy restatement of the link-contact arithmetic of sai-primitives_amd/csrc/saip_link_contact.h, vectorised over a leading axis of instances.

Every product and every sum is one NumPy operation, in the order the header writes them, and the spheres are summed in the header's
eight-lane split and fold, so that the host build of the header (contraction off) and the kernel give the same bits.  Shapes: centres and
velocities (N, S, 3) and radii (S,) in the CALLER's sphere numbering, `order` the sorted list (order[i]: the caller's sphere at sorted
position i), obstacles (O, 8) or (N, O, 8) with rows { kind, a[3], b[3], r }, materials (O, 4) with rows { k, c, mu, v_s }.

The kinematics at the end (frames, joint axes, sphere centres and velocities from q and dq) are plain NumPy, not bit-exact: they choose
obstacles, feed the physics checks and supply the host build's inputs."""
import numpy as np

import clearance_ref as CL
import trees as TR

MAX_SPHERES, MAX_OBSTACLES, OBSTACLE_WORDS, MATERIAL_WORDS, READOUT_ROWS, SUMMARY_ROWS, LANES = 32, 16, 8, 4, 8, 4, 8
EVALUATE, APPLY = 0, 1
dot = CL.dot


def vmax(a, b):
    """lc_max: a < b ? b : a (the first argument on a tie and when the comparison fails)"""
    with np.errstate(invalid="ignore"):
        return np.where(a < b, b, a)


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def velocity(tv, tw, tc, p):
    """ct_velocity: (tv + tw x p) - tc"""
    return (tv + cross(tw, p)) - tc


def item_parts(w, m, c, v, rs):
    """the terms of lc_item for (N,) instances: w (N, 8), m (4,), c, v (N, 3) -> d (N,), n, f_n, f_t, v_t, f = f_n n + f_t, active; the
    force terms are what an ACTIVE item would have (garbage where it is not)"""
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a, b = w[:, 1:4], w[:, 4:7]
        hs = w[:, 0] == CL.HALF_SPACE
        d = np.where(hs, CL.half_space_dist(a, w[:, 4], c, rs), CL.capsule_dist(a, b, w[:, 7], c, rs))
        e, x = b - a, c - a
        L2 = dot(e, e)
        t = np.where(L2 > 0.0, np.fmin(np.fmax(dot(x, e) / L2, 0.0), 1.0), 0.0)
        u = x - t[:, None] * e
        ln = np.sqrt(dot(u, u))
        n = np.where(hs[:, None], a, u / ln[:, None])
        active = (d < 0.0) & (hs | (ln != 0.0))
        k, cd, mu, vs = m
        vn = dot(n, v)
        fn = vmax(0.0, (-k * d) - cd * vn)
        vt = v - vn[:, None] * n
        s = vmax(np.sqrt(dot(vt, vt)), vs)
        g = mu * fn
        ft = np.zeros_like(vt) if mu == 0.0 else -(g[:, None] * vt) / s[:, None]
        f = fn[:, None] * n + ft
    return d, n, fn, ft, vt, f, active


def item(w, m, c, v, rs):
    """lc_item: d (N,), f (N, 3), fn (N,), active (N,); an inactive item has f = 0 and fn = 0"""
    d, n, fn, ft, vt, f, active = item_parts(w, m, c, v, rs)
    return d, np.where(active[:, None], f, 0.0), np.where(active, fn, 0.0), active


def _fold(v, w):
    take = (w["dmin"] < v["dmin"]) | ((w["dmin"] == v["dmin"]) & (w["k"] < v["k"]))
    return dict(f=v["f"] + w["f"], fn_sum=v["fn_sum"] + w["fn_sum"], fmax=vmax(v["fmax"], w["fmax"]), active=v["active"] + w["active"],
                dmin=np.where(take, w["dmin"], v["dmin"]), k=np.where(take, w["k"], v["k"]))


def evaluate(centres, vels, radii, obstacles, materials, order=None):
    """lc_evaluate_host: dict readout (N, 8), F (N, S, 3) and act (N, S) in the caller's numbering, run (N,): the torque loop runs"""
    centres, vels = np.asarray(centres, float), np.asarray(vels, float)
    N, S = centres.shape[:2]
    radii, materials = np.asarray(radii, float), np.asarray(materials, float)
    obstacles = np.asarray(obstacles, float)
    ob = np.broadcast_to(obstacles, (N,) + obstacles.shape[-2:])
    O = ob.shape[1]
    order = np.arange(S) if order is None else np.asarray(order, int)
    F, act = np.zeros((N, S, 3)), np.zeros((N, S), bool)
    lanes = []
    for lane in range(LANES):
        p = dict(f=np.zeros((N, 3)), fn_sum=np.zeros(N), fmax=np.zeros(N), active=np.zeros(N, int), dmin=np.full(N, np.inf), k=np.full(N, -1))
        for i in range(lane, S, LANES):
            s = int(order[i])
            Fs, n_act = np.zeros((N, 3)), np.zeros(N, int)
            for o in range(O):
                d, f, fn, a = item(ob[:, o], materials[o], centres[:, s], vels[:, s], radii[s])
                k = s * O + o
                with np.errstate(invalid="ignore"):
                    take = (d < p["dmin"]) | ((d == p["dmin"]) & (k < p["k"]))
                p["dmin"], p["k"] = np.where(take, d, p["dmin"]), np.where(take, k, p["k"])
                with np.errstate(invalid="ignore", over="ignore"):
                    Fs = np.where(a[:, None], Fs + f, Fs)
                    p["fn_sum"] = np.where(a, p["fn_sum"] + fn, p["fn_sum"])
                    p["fmax"] = np.where(a, vmax(p["fmax"], np.sqrt(dot(f, f))), p["fmax"])
                n_act = n_act + a
            F[:, s], act[:, s] = Fs, n_act > 0
            with np.errstate(invalid="ignore", over="ignore"):
                p["f"] = p["f"] + Fs
            p["active"] = p["active"] + n_act
        lanes.append(p)
    off = LANES // 2
    while off >= 1:
        for lane in range(off):
            with np.errstate(invalid="ignore", over="ignore"):
                lanes[lane] = _fold(lanes[lane], lanes[lane + off])
        off //= 2
    v = lanes[0]
    bad = ~np.isfinite(centres).all(axis=(1, 2))
    ro = np.empty((N, READOUT_ROWS))
    ro[:, 0:3] = np.where(bad[:, None], np.nan, v["f"])
    ro[:, 3] = np.where(bad, np.nan, v["dmin"])
    ro[:, 4] = np.where(bad, -1, v["k"])
    ro[:, 5] = np.where(bad, 0, v["active"])
    ro[:, 6] = np.where(bad, np.nan, v["fn_sum"])
    ro[:, 7] = np.where(bad, np.nan, v["fmax"])
    return dict(readout=ro, F=F, act=act, run=~bad & (v["active"] > 0))


def joint_torque(revolute, aw, oj, p, f):
    """ct_joint_torque"""
    return dot(aw, cross(p - oj, f)) if revolute else dot(aw, f)


def torques(ev, centres, order, anc, jtype, aw, oj, tau_cmd):
    """tau_sim (N, n): anc[i] the ancestor mask of sorted position i, jtype (n,) 1 revolute 2 prismatic, aw, oj (N, n, 3), tau_cmd (N, n)"""
    tau_cmd = np.asarray(tau_cmd, float)
    N, n = tau_cmd.shape
    u0 = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
    out = u0.copy()
    for j in range(n):
        x = np.zeros(N)
        if jtype[j] in (1, 2):
            for i, s in enumerate(order):
                if not (int(anc[i]) >> j) & 1:
                    continue
                with np.errstate(invalid="ignore", over="ignore"):
                    x = np.where(ev["act"][:, s], x + joint_torque(jtype[j] == 1, aw[:, j], oj[:, j], centres[:, s], ev["F"][:, s]), x)
        with np.errstate(invalid="ignore", over="ignore"):
            out[:, j] = np.where(ev["run"], u0[:, j] + x, u0[:, j])
    return out


def summary_advance(s, dt, ro):
    """s (N, 4) after one APPLY substep of length dt with the readout ro (N, 8)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([s[:, 0] + dt * ro[:, 6], vmax(s[:, 1], ro[:, 7]), vmax(s[:, 2], vmax(0.0, -ro[:, 3])), s[:, 3] + np.where(ro[:, 5] > 0.0, 1.0, 0.0)], axis=-1)


def add_cost(cost, S0, S1, w_impulse, w_peak):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.isnan(S0), np.nan, cost + (w_impulse * S0 + w_peak * S1))


def decode(k, O):
    """item number -> (sphere, obstacle) / None"""
    k = int(k)
    return None if k < 0 else (k // O, k % O)


# ------------------------------------------------------------------ kinematics (plain NumPy)
def link_bodies(model):
    """movable body (dof index, -1: the fixed base) every link of a workloads.RobotModel is rigidly attached to"""
    par = TR.parent_index(model)
    body = []
    for i in range(model.nl):
        d = model.dof_of_link[i]
        body.append(d if d >= 0 else (body[par[i]] if par[i] >= 0 else -1))
    return body


def ancestor_masks(model):
    """per dof j: the mask of the joints that move body j (itself included)"""
    jp = TR.joint_parents(model)
    anc = []
    for j in range(model.dof):
        anc.append((anc[jp[j]] if jp[j] >= 0 else 0) | (1 << j))
    return anc


def sort_spheres(model, spheres):
    """order (sorted position -> caller's sphere, stable by body) and the ancestor mask of every sorted position"""
    body, masks = link_bodies(model), ancestor_masks(model)
    b = [body[model.link_index(s[0])] for s in spheres]
    order = sorted(range(len(spheres)), key=lambda s: b[s])
    return np.array(order, int), [masks[b[s]] if b[s] >= 0 else 0 for s in order]


def joints(model, q):
    """frames (per link), jtype (n,), world axes aw (N, n, 3) and origins oj (N, n, 3) of the joints at q (N, n)"""
    frames = TR.tree_fk(model, q)
    N = np.asarray(q).shape[0]
    jtype, aw, oj = np.zeros(model.dof, int), np.zeros((N, model.dof, 3)), np.zeros((N, model.dof, 3))
    for li, l in enumerate(model.links):
        d = model.dof_of_link[li]
        if d < 0:
            continue
        R, o = frames[li]
        a = np.asarray(l["axis"], float)
        jtype[d] = 1 if l["joint_type"] == "revolute" else 2
        aw[:, d], oj[:, d] = R @ (a / np.linalg.norm(a)), o
    return frames, jtype, aw, oj


def sphere_state(model, q, dq, spheres):
    """centres and velocities (N, S, 3) of [(link, centre in the link frame, radius)] at q, dq, and what joints() returns"""
    q, dq = np.asarray(q, float), np.asarray(dq, float)
    frames, jtype, aw, oj = joints(model, q)
    N, S = q.shape[0], len(spheres)
    c, v = np.zeros((N, S, 3)), np.zeros((N, S, 3))
    for s, (link, r, _) in enumerate(spheres):
        li = model.link_index(link)
        R, o = frames[li]
        c[:, s] = o + R @ np.asarray(r, float)
        Jv = TR.tree_jacobian(model, frames, li, c[:, s])[:, 0:3]
        v[:, s] = np.einsum("bij,bj->bi", Jv, dq)
    return c, v, (frames, jtype, aw, oj)
