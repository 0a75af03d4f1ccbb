"""NumPy restatement of the contact-patch arithmetic of sai-primitives_amd/csrc/saip_contact_patch.h, vectorised over a leading axis of
cases, on top of contact_ref.py.

An instance has eight point slots; slot i >= n_points holds exact zeros and is no candidate for the smallest distance.  Every sum over the
slots has the shape v[i] += v[i + off] for off = 4, 2, 1, so the rounding order is that of the kernel's eight-lane fold."""
import numpy as np

import contact_ref as CR

MAX_POINTS, MAX_PATCHES, READOUT_ROWS, SUMMARY_ROWS = 8, 2, 20, 6


def fold_sum(v):
    """(..., 8) -> (...): ((v0 + v4) + (v2 + v6)) + ((v1 + v5) + (v3 + v7))"""
    a = v[..., :4] + v[..., 4:]
    b = a[..., :2] + a[..., 2:]
    return b[..., 0] + b[..., 1]


def fold_min(d):
    """(N, 8) candidates -> the smallest and the lowest index that attains it, by the kernel's pairwise fold"""
    ix = np.broadcast_to(np.arange(MAX_POINTS), d.shape)
    for off in (4, 2, 1):
        da, db, ia, ib = d[:, :off], d[:, off:2 * off], ix[:, :off], ix[:, off:2 * off]
        take = (db < da) | ((db == da) & (ib < ia))
        d, ix = np.where(take, db, da), np.where(take, ib, ia)
    return d[:, 0], ix[:, 0]


def slots(planes, xc, Rc, points, tv, tw, tc):
    """the eight slots of N instances: dict p, f, m (N, 8, 3), fn_sum, dcand (N, 8), active (N, 8) int.  points (n, 3)"""
    N, n = xc.shape[0], len(points)
    out = dict(p=np.zeros((N, 8, 3)), f=np.zeros((N, 8, 3)), m=np.zeros((N, 8, 3)), fn_sum=np.zeros((N, 8)), dcand=np.full((N, 8), np.inf),
               active=np.zeros((N, 8), int))
    for i in range(n):
        r = np.broadcast_to(np.asarray(points[i], float), (N, 3))
        p = CR.point(xc, Rc, r)
        v = CR.velocity(tv, tw, tc, p)
        f, fn_sum, dmin, active = CR.plane_forces(planes, p, v)
        out["p"][:, i], out["f"][:, i], out["m"][:, i] = p, f, CR.cross(p - xc, f)
        out["fn_sum"][:, i], out["dcand"][:, i], out["active"][:, i] = fn_sum, dmin, active
    return out


def net(s):
    """dict F, M (N, 3), fn_total, dmin (N,), i_deep, n_touch (N,) int"""
    dmin, i_deep = fold_min(s["dcand"])
    return dict(F=fold_sum(s["f"].transpose(0, 2, 1)), M=fold_sum(s["m"].transpose(0, 2, 1)), fn_total=fold_sum(s["fn_sum"]), dmin=dmin,
                i_deep=i_deep, n_touch=(s["active"] > 0).sum(axis=1))


def joint_torques(s, rev, aw, oj):
    """(N, J): sum over the slots of (active ? ct_joint_torque : 0.0)"""
    t = np.stack([np.where(s["active"][:, i, None] > 0, CR.joint_torque(rev, aw, oj, s["p"][:, i], s["f"][:, i]), 0.0) for i in range(8)], axis=-1)
    return fold_sum(t)


def tau_sim(tau_cmd, patches):
    """((tau_cmd or 0 when NaN) + ext_0) + ext_1.  patches: (ext (N, J), ancestors (J,) bool, n_touch (N,)) in attach order; a patch is
    skipped (not added as zero) on joints that are no ancestors of its body and in instances where none of its points touches"""
    t = np.where(np.isnan(tau_cmd), 0.0, tau_cmd)
    for ext, anc, n_touch in patches:
        t = np.where(np.asarray(anc, bool)[None, :] & (n_touch > 0)[:, None], t + ext, t)
    return t


def sensor(F, M, Rc, Rcs, tcs):
    """FS, MS in the sensor frame from the net force and moment on the robot"""
    fc, mc = CR.matT_vec(Rc, -F), CR.matT_vec(Rc, -M)
    y = mc - CR.cross(tcs, fc)
    return CR.matT_vec(Rcs, fc), CR.matT_vec(Rcs, y)


def readout(s, nt, xc):
    """(N, 20)"""
    return np.column_stack([nt["F"], nt["M"], nt["dmin"], nt["n_touch"].astype(float), nt["i_deep"].astype(float), xc, s["fn_sum"]])


def summary_advance(sm, dt, nt, n_points):
    """sm (N, 6) after one APPLY substep of length dt"""
    on = nt["n_touch"] > 0
    return np.stack([sm[:, 0] + dt * nt["fn_total"], np.maximum(sm[:, 1], np.sqrt(CR.dot(nt["F"], nt["F"]))),
                     np.maximum(sm[:, 2], np.where(on, -nt["dmin"], 0.0)), sm[:, 3] + np.where(on, 1.0, 0.0),
                     np.maximum(sm[:, 4], np.sqrt(CR.dot(nt["M"], nt["M"]))), sm[:, 5] + np.where(nt["n_touch"] == n_points, 1.0, 0.0)], axis=-1)
