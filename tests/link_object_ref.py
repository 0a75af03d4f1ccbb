"""NumPy restatement of the pushed-object arithmetic of sai-primitives_amd/csrc/saip_link_object.h, vectorised over a leading axis of instances.

Every product and every sum is one NumPy operation, in the order the header writes them, in the header's eight-lane split and fold, so
that the host build of the header (contraction off) and the kernel give the same bits.  Robot spheres as in link_contact_ref.py (centres and
velocities (N, S, 3), radii (S,), `order` the sorted list); the object: state x (N, 13) = p, quat (w, x, y, z), v, omega; inertial words (4,) or
(N, 4) = m, Ix, Iy, Iz; shape r (P, 3) and radius (P,) in the body frame; omat (4,) the robot-object material."""
import numpy as np

import link_contact_ref as LC

MAX_SPHERES, STATE_ROWS, INERTIAL_WORDS, READOUT_ROWS, SUMMARY_ROWS = 8, 13, 4, 12, 4
dot, cross, vmax = LC.dot, LC.cross, LC.vmax
_quiet = dict(invalid="ignore", over="ignore", divide="ignore")


def rotation(q):
    """lo_rotation: (N, 4) -> (N, 9) row-major"""
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    return np.stack([1.0 - 2.0 * (yy + zz), 2.0 * (xy - wz), 2.0 * (xz + wy), 2.0 * (xy + wz), 1.0 - 2.0 * (xx + zz), 2.0 * (yz - wx),
                     2.0 * (xz - wy), 2.0 * (yz + wx), 1.0 - 2.0 * (xx + yy)], axis=-1)


def sphere(x, R, r):
    """lo_sphere: centre and velocity (N, 3) of the object sphere at r (3,)"""
    c = np.stack([x[:, i] + ((R[:, 3 * i] * r[0] + R[:, 3 * i + 1] * r[1]) + R[:, 3 * i + 2] * r[2]) for i in range(3)], axis=-1)
    a = c - x[:, 0:3]
    return c, x[:, 7:10] + cross(x[:, 10:13], a)


def spheres(x, shape_r):
    """(N, P, 3) centres and velocities of the object spheres at the state x"""
    with np.errstate(**_quiet):
        R = rotation(x[:, 3:7])
        cv = [sphere(x, R, np.asarray(r, float)) for r in shape_r]
    return np.stack([c for c, _ in cv], axis=1), np.stack([v for _, v in cv], axis=1)


def _clear(N):
    z = lambda: np.zeros((N, 3))
    return dict(rf=z(), rm=z(), wf=z(), wm=z(), dmin=np.full(N, np.inf), fn_sum=np.zeros(N), wpen=np.zeros(N), k=np.full(N, -1), active=np.zeros(N, int))


def _fold(v, w):
    take = (w["dmin"] < v["dmin"]) | ((w["dmin"] == v["dmin"]) & (w["k"] < v["k"]))
    return dict(rf=v["rf"] + w["rf"], rm=v["rm"] + w["rm"], wf=v["wf"] + w["wf"], wm=v["wm"] + w["wm"], fn_sum=v["fn_sum"] + w["fn_sum"],
                wpen=vmax(v["wpen"], w["wpen"]), active=v["active"] + w["active"], dmin=np.where(take, w["dmin"], v["dmin"]), k=np.where(take, w["k"], v["k"]))


def integrate(x, inertial, grav, dt, v):
    """lo_integrate: the new state (N, 13)"""
    N = x.shape[0]
    inr = np.broadcast_to(np.asarray(inertial, float), (N, 4))
    grav = np.asarray(grav, float)
    with np.errstate(**_quiet):
        R = rotation(x[:, 3:7])
        xn = np.empty_like(x)
        F = (inr[:, 0:1] * grav[None, :] + v["wf"]) + v["rf"]
        T = v["wm"] + v["rm"]
        xn[:, 7:10] = x[:, 7:10] + dt * (F / inr[:, 0:1])
        om = x[:, 10:13]
        tb = np.stack([(R[:, i] * T[:, 0] + R[:, 3 + i] * T[:, 1]) + R[:, 6 + i] * T[:, 2] for i in range(3)], axis=-1)
        wb = np.stack([(R[:, i] * om[:, 0] + R[:, 3 + i] * om[:, 1]) + R[:, 6 + i] * om[:, 2] for i in range(3)], axis=-1)
        y = np.stack([(inr[:, 3] - inr[:, 2]) * (wb[:, 1] * wb[:, 2]), (inr[:, 1] - inr[:, 3]) * (wb[:, 2] * wb[:, 0]),
                      (inr[:, 2] - inr[:, 1]) * (wb[:, 0] * wb[:, 1])], axis=-1)
        db = dt * ((tb - y) / inr[:, 1:4])
        xn[:, 10:13] = np.stack([om[:, i] + ((R[:, 3 * i] * db[:, 0] + R[:, 3 * i + 1] * db[:, 1]) + R[:, 3 * i + 2] * db[:, 2]) for i in range(3)], axis=-1)
        xn[:, 0:3] = x[:, 0:3] + dt * xn[:, 7:10]
        qw, qx, qy, qz = x[:, 3], x[:, 4], x[:, 5], x[:, 6]
        ox, oy, oz = xn[:, 10], xn[:, 11], xn[:, 12]
        d = np.stack([-((ox * qx + oy * qy) + oz * qz), (ox * qw + oy * qz) - oz * qy, (oy * qw + oz * qx) - ox * qz, (oz * qw + ox * qy) - oy * qx], axis=-1)
        h = 0.5 * dt
        u = x[:, 3:7] + h * d
        ln = np.sqrt(((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]) + u[:, 3] * u[:, 3])
        xn[:, 3:7] = u / ln[:, None]
    return xn


def step(centres, vels, radii, obstacles, materials, order, x, inertial, shape_r, shape_radius, omat, grav, dt):
    """lo_step_host: dict readout_lc (N, 8), readout (N, 12), F (N, S, 3) and act (N, S) in the caller's numbering, run (N,), valid (N,),
    state (N, 13) the new state (the old one where the instance is invalid), partial: the folded object partial"""
    centres, vels, x = np.asarray(centres, float), np.asarray(vels, float), np.asarray(x, float)
    N, S = centres.shape[:2]
    radii, materials, omat = np.asarray(radii, float), np.asarray(materials, float), np.asarray(omat, float)
    obstacles = np.asarray(obstacles, float)
    ob = np.broadcast_to(obstacles, (N,) + obstacles.shape[-2:])
    O = ob.shape[1]
    shape_r, shape_radius = np.asarray(shape_r, float), np.asarray(shape_radius, float)
    P = shape_r.shape[0]
    order = np.arange(S) if order is None else np.asarray(order, int)
    OC, OV = spheres(x, shape_r)
    pos = x[:, 0:3]
    F, act = np.zeros((N, S, 3)), np.zeros((N, S), bool)
    lanes, objs = [], []
    for lane in range(LC.LANES):
        p = dict(f=np.zeros((N, 3)), fn_sum=np.zeros(N), fmax=np.zeros(N), active=np.zeros(N, int), dmin=np.full(N, np.inf), k=np.full(N, -1))
        q = _clear(N)
        for i in range(lane, S, LC.LANES):
            s = int(order[i])
            Fs, n_act = np.zeros((N, 3)), np.zeros(N, int)
            for o in range(O):
                d, f, fn, a = LC.item(ob[:, o], materials[o], centres[:, s], vels[:, s], radii[s])
                k = s * O + o
                with np.errstate(**_quiet):
                    take = (d < p["dmin"]) | ((d == p["dmin"]) & (k < p["k"]))
                    p["dmin"], p["k"] = np.where(take, d, p["dmin"]), np.where(take, k, p["k"])
                    Fs = np.where(a[:, None], Fs + f, Fs)
                    p["fn_sum"] = np.where(a, p["fn_sum"] + fn, p["fn_sum"])
                    p["fmax"] = np.where(a, vmax(p["fmax"], np.sqrt(dot(f, f))), p["fmax"])
                n_act = n_act + a
            with np.errstate(**_quiet):
                p["f"] = p["f"] + Fs
            p["active"] = p["active"] + n_act
            for t in range(P):
                cp = OC[:, t]
                w = np.concatenate([np.zeros((N, 1)), cp, cp, np.full((N, 1), shape_radius[t])], axis=1)
                with np.errstate(**_quiet):
                    d, f, fn, a = LC.item(w, omat, centres[:, s], vels[:, s] - OV[:, t], radii[s])
                    k = s * P + t
                    take = (d < q["dmin"]) | ((d == q["dmin"]) & (k < q["k"]))
                    q["dmin"], q["k"] = np.where(take, d, q["dmin"]), np.where(take, k, q["k"])
                    Fs = np.where(a[:, None], Fs + f, Fs)
                    nf = -f
                    m = cross(cp - pos, nf)
                    q["rf"] = np.where(a[:, None], q["rf"] + nf, q["rf"])
                    q["rm"] = np.where(a[:, None], q["rm"] + m, q["rm"])
                    q["fn_sum"] = np.where(a, q["fn_sum"] + fn, q["fn_sum"])
                n_act = n_act + a
                q["active"] = q["active"] + a
            F[:, s], act[:, s] = Fs, n_act > 0
        if lane < P:
            cp, vp = OC[:, lane], OV[:, lane]
            for o in range(O):
                with np.errstate(**_quiet):
                    d, f, fn, a = LC.item(ob[:, o], materials[o], cp, vp, shape_radius[lane])
                    q["wpen"] = vmax(q["wpen"], vmax(0.0, -d))
                    m = cross(cp - pos, f)
                    q["wf"] = np.where(a[:, None], q["wf"] + f, q["wf"])
                    q["wm"] = np.where(a[:, None], q["wm"] + m, q["wm"])
        lanes.append(p)
        objs.append(q)
    off = LC.LANES // 2
    while off >= 1:
        for lane in range(off):
            with np.errstate(**_quiet):
                lanes[lane] = LC._fold(lanes[lane], lanes[lane + off])
                objs[lane] = _fold(objs[lane], objs[lane + off])
        off //= 2
    v, q = lanes[0], objs[0]
    rbad = ~np.isfinite(centres).all(axis=(1, 2))
    ro = np.empty((N, LC.READOUT_ROWS))
    ro[:, 0:3] = np.where(rbad[:, None], np.nan, v["f"])
    ro[:, 3] = np.where(rbad, np.nan, v["dmin"])
    ro[:, 4] = np.where(rbad, -1, v["k"])
    ro[:, 5] = np.where(rbad, 0, v["active"])
    ro[:, 6] = np.where(rbad, np.nan, v["fn_sum"])
    ro[:, 7] = np.where(rbad, np.nan, v["fmax"])
    bad = rbad | ~np.isfinite(x).all(axis=1)
    rq = np.concatenate([q["rf"], q["rm"], q["wf"], q["dmin"][:, None], q["k"][:, None].astype(float), q["active"][:, None].astype(float)], axis=1)
    rq = np.where(bad[:, None], np.nan, rq)
    xn = np.where(bad[:, None], x, integrate(x, inertial, grav, dt, q))
    return dict(readout_lc=ro, readout=rq, F=F, act=act, run=~bad & (v["active"] + q["active"] > 0), valid=~bad, state=xn, partial=q)


def summary_advance(s, dt, st):
    """lo_summary_advance: s (N, 4) after one APPLY substep whose step() result is st"""
    q, bad = st["partial"], ~st["valid"]
    with np.errstate(**_quiet):
        s0 = s[:, 0] + dt * np.where(bad, np.nan, q["fn_sum"])
        s1 = np.where(bad, s[:, 1], vmax(s[:, 1], vmax(0.0, -q["dmin"])))
        s2 = np.where(bad, s[:, 2], vmax(s[:, 2], q["wpen"]))
        s3 = np.where(bad, s[:, 3], s[:, 3] + np.where(q["active"] > 0, 1.0, 0.0))
    return np.stack([s0, s1, s2, s3], axis=-1)


def add_cost(cost, x, tp, w_pos, tq, w_ori):
    """lo_add_cost: tq None or a unit quaternion (4,)"""
    x = np.asarray(x, float)
    with np.errstate(**_quiet):
        d = x[:, 0:3] - np.asarray(tp, float)
        c = w_pos * ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        if tq is not None:
            tq = np.asarray(tq, float)
            s = ((x[:, 3] * tq[0] + x[:, 4] * tq[1]) + x[:, 5] * tq[2]) + x[:, 6] * tq[3]
            c = c + w_ori * (1.0 - s * s)
        return np.where(np.isfinite(x).all(axis=1), cost + c, np.inf)


def torques(st, centres, order, anc, jtype, aw, oj, tau_cmd):
    """tau_sim (N, n) of a step() result: link_contact_ref.torques over F_s with the object items in them"""
    return LC.torques(dict(act=st["act"], F=st["F"], run=st["run"]), centres, order, anc, jtype, aw, oj, tau_cmd)


def decode(k, P):
    """item number -> (robot sphere, object sphere) / None"""
    return LC.decode(k, P)
