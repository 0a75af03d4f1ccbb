"""An exact NumPy oracle of the robot dynamics M(q) qdd + h(q, dq) = tau - d dq for the resident integrator and the dynamics queries (a
helper module, not a conftest).  It shares nothing with the kernels: no recursion over velocities, no Newton-Euler pass, no composite
bodies.  The mass matrix is the Jacobian form M = sum_links m Jv^T Jv + Jw^T (R I R^T) Jw, the potential energy U = -sum_links m c.g, and

    h = Mdot dq - 1/2 grad_q(dq^T M dq) + dU/dq

with dM/dq_k and dU/dq_k by the complex step, Im f(q + i STEP e_k) / STEP: no subtraction, no step-size error (STEP^2 = 1e-60 is far below
the rounding of the real part).  Everything is written once for float64, longdouble, complex128 and clongdouble, for chains and trees
(parents from trees.parent_index; a chain is the tree with parent = li - 1), revolute and prismatic joints and welded links, and for one
set of inertial parameters per instance (the descriptions of inertia_ref.instance_description).

oracle/restatement.forward_dynamics is the same Lagrangian form with central differences (own error 4.5e-12 .. 1.3e-10); this one is exact
to the rounding of its dtype, which bias() reports as H: the same sum with every summand replaced by its absolute value.

residual_check() is what the device tests assert: the backward error of one semi-implicit Euler step, in units of n eps of a scale made of
absolute sums, so that it does not depend on the conditioning of M."""
import numpy as np

import trees as TR
import workloads as W

EPS = 2.0 ** -52
STEP = 1e-30
_REAL = {np.dtype(np.float64): np.float64, np.dtype(np.complex128): np.float64,
         np.dtype(np.longdouble): np.longdouble, np.dtype(np.clongdouble): np.longdouble}
_COMPLEX = {np.float64: np.complex128, np.longdouble: np.clongdouble}


def real_of(dtype):
    return _REAL[np.dtype(dtype)]


class Model:
    """the kinematic structure of a workloads.RobotModel plus the inertial parameters of every link, for one robot (shared by the batch) or
    for a list of robots of the same structure, one per instance"""

    def __init__(self, models):
        ms = list(models) if isinstance(models, (list, tuple)) else [models]
        ms = [m if isinstance(m, W.RobotModel) else W.RobotModel(m) for m in ms]
        m0 = ms[0]
        self.n, self.nl = m0.dof, m0.nl
        self.parent = TR.parent_index(m0)
        self.dof_of_link = list(m0.dof_of_link)
        self.joint_type = [l["joint_type"] for l in m0.links]
        ld = np.longdouble
        self.xyz = [np.asarray(l["origin_xyz"], ld) for l in m0.links]
        self.rpy = [np.asarray(l["origin_rpy"], ld) for l in m0.links]
        self.axis = [np.asarray(l["axis"], ld) for l in m0.links]
        for m in ms[1:]:
            assert m.nl == self.nl and TR.parent_index(m) == self.parent and [l["joint_type"] for l in m.links] == self.joint_type
        self.mass = np.array([[l["mass"] for l in m.links] for m in ms], ld)                 # (I, nl); I = 1 or the batch size
        self.com = np.array([[l["com"] for l in m.links] for m in ms], ld)                   # (I, nl, 3)
        ine = np.array([[l["inertia"] for l in m.links] for m in ms], ld)                    # xx yy zz xy xz yz
        self.inertia = np.empty(ine.shape[:2] + (3, 3), ld)
        for e, (i, k) in enumerate([(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]):
            self.inertia[:, :, i, k] = self.inertia[:, :, k, i] = ine[:, :, e]
        # the movable links a point of link li depends on
        self.path = []
        for li in range(self.nl):
            p, i = [], li
            while i >= 0:
                if self.dof_of_link[i] >= 0:
                    p.append(i)
                i = self.parent[i]
            self.path.append(p[::-1])


def as_model(model):
    return model if isinstance(model, Model) else Model(model)


def _rot_rpy(rpy, rdt):
    r, p, y = (rdt(x) for x in rpy)
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    o, z = rdt(1), rdt(0)
    Rx = np.array([[o, z, z], [z, cr, -sr], [z, sr, cr]], rdt)
    Ry = np.array([[cp, z, sp], [z, o, z], [-sp, z, cp]], rdt)
    Rz = np.array([[cy, -sy, z], [sy, cy, z], [z, z, o]], rdt)
    return Rz @ Ry @ Rx


def _unit(a, rdt):
    a = a.astype(rdt)
    return a / np.sqrt((a * a).sum())


def _skew(a):
    z = a.dtype.type(0)
    return np.array([[z, -a[2], a[1]], [a[2], z, -a[0]], [-a[1], a[0], z]], a.dtype)


def _mm(A, B):
    """batched matrix product without conjugation, any dtype"""
    return np.einsum("...ij,...jk->...ik", A, B)


def _mv(A, v):
    return np.einsum("...ij,...j->...i", A, v)


def fk(model, q, dtype=np.float64):
    """q (B, n) -> per link (R (B, 3, 3), o (B, 3)) in `dtype`"""
    md = as_model(model)
    rdt = real_of(dtype)
    q = np.asarray(q).astype(dtype)
    B = q.shape[0]
    eye = np.broadcast_to(np.eye(3, dtype=rdt), (B, 3, 3)).astype(dtype)
    out = []
    for li in range(md.nl):
        if md.parent[li] >= 0:
            R, o = out[md.parent[li]]
        else:
            R, o = eye, np.zeros((B, 3), dtype)
        o = o + _mv(R, md.xyz[li].astype(rdt))
        R = _mm(R, _rot_rpy(md.rpy[li], rdt))
        d = md.dof_of_link[li]
        if md.joint_type[li] == "revolute":
            K = _skew(_unit(md.axis[li], rdt))
            s, c = np.sin(q[:, d])[:, None, None], np.cos(q[:, d])[:, None, None]
            R = _mm(R, np.eye(3, dtype=rdt) + s * K + (1 - c) * (K @ K))
        elif md.joint_type[li] == "prismatic":
            o = o + _mv(R, _unit(md.axis[li], rdt)) * q[:, d][:, None]
        out.append((R, o))
    return out


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _mass_and_energy(md, q, g, dtype, with_abs=False):
    """M (B, n, n), the summands of U (B, nl, 3) and, when asked, the scales of M (see mass_matrix) and of dU/dq per unit of |g|:
    sum_links m |c - o_i| (B, n), 1 in place of the lever arm for a prismatic joint"""
    rdt = real_of(dtype)
    frames = fk(md, q, dtype)
    B, n = q.shape[0], md.n
    M = np.zeros((B, n, n), dtype)
    Mabs, Uarm = (np.zeros((B, n, n), rdt), np.zeros((B, n), rdt)) if with_abs else (None, None)
    Ut = np.zeros((B, md.nl, 3), dtype)
    gv = np.asarray(g, rdt)
    for li in range(md.nl):
        m, I = md.mass[:, li].astype(rdt), md.inertia[:, li].astype(rdt)
        if not m.any() and not I.any():
            continue
        R, o = frames[li]
        c = o + _mv(R, md.com[:, li].astype(rdt))
        Ut[:, li] = -(m[:, None] * c) * gv
        Jv, Jw = np.zeros((B, 3, n), dtype), np.zeros((B, 3, n), dtype)
        arm, turn = np.zeros((B, n), rdt), np.zeros((B, n), rdt)      # the norms the columns of Jv and Jw are bounded by
        for lj in md.path[li]:
            d = md.dof_of_link[lj]
            Rj, oj = frames[lj]
            z = _mv(Rj, _unit(md.axis[lj], rdt))
            if md.joint_type[lj] == "revolute":
                Jv[:, :, d] = _cross(z, c - oj)
                Jw[:, :, d] = z
                arm[:, d], turn[:, d] = np.sqrt((np.abs(c - oj) ** 2).sum(axis=1)), 1
            else:
                Jv[:, :, d] = z
                arm[:, d] = 1
        Iw = _mm(_mm(R, I), np.swapaxes(R, 1, 2))
        M += m[:, None, None] * np.einsum("bki,bkj->bij", Jv, Jv) + np.einsum("bki,bkl,blj->bij", Jw, Iw, Jw)
        if with_abs:
            Inorm = np.sqrt((I * I).sum(axis=(1, 2)))
            Mabs += np.abs(m)[:, None, None] * arm[:, :, None] * arm[:, None, :] + Inorm[:, None, None] * turn[:, :, None] * turn[:, None, :]
            Uarm += np.abs(m)[:, None] * arm
    return M, Ut, Mabs, Uarm


def mass_matrix(model, q, dtype=np.float64, with_abs=False):
    """Jacobian-form M (B, n, n) in `dtype`; with_abs: also the scale of its rounding, the sum over the links of every summand with its
    factors replaced by their norms: m |c - o_i| |c - o_j| + |I|_F for revolute joints i, j (1 in place of the lever arm for a prismatic
    joint, and no inertia term).  Norms and not entries: a rotation carries an absolute error of eps in every entry, so an entry of M
    that the geometry makes small is no more accurate than the others"""
    md = as_model(model)
    M, _, Mabs, _ = _mass_and_energy(md, np.asarray(q).astype(dtype), (0.0, 0.0, 0.0), dtype, with_abs)
    return (M, Mabs) if with_abs else M


def potential_energy(model, q, g, dtype=np.float64):
    """U (B,) = -sum_links m c.g"""
    md = as_model(model)
    return _mass_and_energy(md, np.asarray(q).astype(dtype), g, dtype)[1].sum(axis=(1, 2))


def bias(model, q, dq, g, dtype=np.complex128):
    """(h, H), both (B, n) in the real type of `dtype` (complex128 or clongdouble; a real dtype selects its complex twin):
    h = Mdot dq - 1/2 grad(dq^T M dq) + dU/dq by the complex step, H the same sum over |summands|: the scale of the rounding in h.
    The summands of the velocity part are the products dM_ij/dq_k dq_j dq_k.  Those of dU/dq_i are m g.(z_i x (c - o_i)), one per link, and
    the absolute value of one is taken over its factors, m |g| |c - o_i| (m |g| for a prismatic joint): the frames carry an absolute
    error of eps in every entry, so a gravity torque that the posture makes small is no more accurate than a large one.  (Measured on the
    CPU: with |summand| itself, complex128 misses clongdouble by up to 9.8 n eps H on the gravity vector of dual_panda_torso at rest.)"""
    md = as_model(model)
    rdt = real_of(dtype)
    cdt = _COMPLEX[rdt]
    q, dq = np.asarray(q), np.asarray(dq).astype(rdt)
    B, n = q.shape
    moving = bool(dq.any())
    dM = np.zeros((n, B, n, n), rdt)
    dU = np.zeros((n, B, md.nl, 3), rdt)
    for k in range(n):
        qk = q.astype(cdt)
        qk[:, k] += cdt(1j) * rdt(STEP)
        M, Ut, _, _ = _mass_and_energy(md, qk, g, cdt)
        if moving:
            dM[k] = M.imag / rdt(STEP)
        dU[k] = Ut.imag / rdt(STEP)
    a = np.einsum("kbij,bj,bk->bijk", dM, dq, dq)             # dM_ij/dq_k dq_j dq_k
    b = np.einsum("ibjk,bj,bk->bijk", dM, dq, dq) / 2         # 1/2 dM_jk/dq_i dq_j dq_k
    u = np.moveaxis(dU, 0, 1).reshape(B, n, -1)
    h = a.sum(axis=(2, 3)) - b.sum(axis=(2, 3)) + u.sum(axis=2)
    gv = np.asarray(g, rdt)
    Uarm = _mass_and_energy(md, q.astype(rdt), g, rdt, True)[3] if gv.any() else np.zeros((B, n), rdt)
    H = np.abs(a).sum(axis=(2, 3)) + np.abs(b).sum(axis=(2, 3)) + np.sqrt((gv * gv).sum()) * Uarm
    return h, H


def solve_spd(M, r):
    """x of M x = r, batched, by Cholesky in the dtype of M (NumPy's solvers stop at double)"""
    M, r = np.array(M), np.array(r)
    n = M.shape[-1]
    L = np.zeros_like(M)
    for k in range(n):
        L[:, k, k] = np.sqrt(M[:, k, k] - (L[:, k, :k] ** 2).sum(axis=1))
        for i in range(k + 1, n):
            L[:, i, k] = (M[:, i, k] - (L[:, i, :k] * L[:, k, :k]).sum(axis=1)) / L[:, k, k]
    y = np.zeros_like(r)
    for i in range(n):
        y[:, i] = (r[:, i] - (L[:, i, :i] * y[:, :i]).sum(axis=1)) / L[:, i, i]
    x = np.zeros_like(r)
    for i in range(n - 1, -1, -1):
        x[:, i] = (y[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    return x


def forward_dynamics(model, q, dq, tau, g=(0.0, 0.0, -9.81), damping=0.0, dtype=np.longdouble):
    """qdd (B, n) in the real type of `dtype`: M qdd = tau - h - damping dq, solved in that type"""
    md = as_model(model)
    rdt = real_of(dtype)
    h, _ = bias(md, q, dq, g, _COMPLEX[rdt])
    M = mass_matrix(md, q, rdt)
    rhs = np.asarray(tau).astype(rdt) - h - rdt(damping) * np.asarray(dq).astype(rdt)
    if rdt is np.float64:
        return np.linalg.solve(M, rhs[..., None])[..., 0]
    return solve_spd(M, rhs)


def residual_check(model, q0, dq0, dq1, tau, dt, g, damping, details=None):
    """the backward error of one step dq1 = dq0 + dt qdd of M(q0) qdd = tau - h(q0, dq0) - damping dq0, as stored in double:
    a = (dq1 - dq0) / dt, r = M a - (tau - h - d dq0) with M and h in long double; per row
      scale = |L||L^T||a| + |tau| + H + d |dq0|        (L the Cholesky factor of M)
      rec   = sum_j |M_ij| 2 eps max(|dq0_j|, |dq1_j|) / dt     (a is recovered from two stored velocities)
    returns (max_i (|r_i| - rec_i) / (n eps scale_i), instance, row): the residual in units of n eps.  details: a dict that receives a, h, H
    and the per-row values"""
    md = as_model(model)
    ld = np.longdouble
    q0, dq0, dq1, tau = (np.asarray(x, float) for x in (q0, dq0, dq1, tau))
    n = md.n
    a = (dq1.astype(ld) - dq0.astype(ld)) / ld(dt)
    M = mass_matrix(md, q0, ld)
    h, H = bias(md, q0, dq0, g, np.clongdouble)
    r = _mv(M, a) - (tau.astype(ld) - h - ld(damping) * dq0.astype(ld))
    L = np.abs(np.linalg.cholesky(M.astype(float)))
    scale = _mv(L, _mv(np.swapaxes(L, 1, 2), np.abs(a).astype(float))) + np.abs(tau) + H.astype(float) + damping * np.abs(dq0)
    rec = _mv(np.abs(M).astype(float), 2 * EPS * np.maximum(np.abs(dq0), np.abs(dq1)) / dt)
    val = (np.abs(r).astype(float) - rec) / (n * EPS * scale)
    if details is not None:
        details.update(a=a.astype(float), h=h.astype(float), H=H.astype(float), rows=val)
    b, i = np.unravel_index(np.argmax(val), val.shape)
    return float(val[b, i]), int(b), int(i)
