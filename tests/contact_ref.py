"""NumPy restatement of the contact arithmetic of sai-primitives_amd/csrc/saip_contact.h, vectorised over a leading axis of cases.

Every product and every sum is one NumPy operation, in the order the header writes them, so that the host build of the header (contraction
off) and the kernel give the same bits.  Shapes: vectors (N, 3), rotations (N, 9) row-major, planes (N, P, 8) or (P, 8) with rows
{ n[3], offset, k, c, mu, v_s }."""
import numpy as np

PLANE_WORDS, READOUT_ROWS, SUMMARY_ROWS, MAX_PLANES = 8, 8, 4, 4


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def mat_vec(R, v):
    return np.stack([(R[..., 3 * i] * v[..., 0] + R[..., 3 * i + 1] * v[..., 1]) + R[..., 3 * i + 2] * v[..., 2] for i in range(3)], axis=-1)


def matT_vec(R, v):
    return np.stack([(R[..., i] * v[..., 0] + R[..., 3 + i] * v[..., 1]) + R[..., 6 + i] * v[..., 2] for i in range(3)], axis=-1)


def point(xc, Rc, rc):
    """p = x_c + R_c r_c"""
    return xc + mat_vec(Rc, rc)


def velocity(tv, tw, tc, p):
    """v = (tv + tw x p) - tc"""
    return (tv + cross(tw, p)) - tc


def plane_forces(planes, p, v):
    """f (N, 3), fn_sum (N,), dmin (N,), active (N,) of the planes on the point p moving with v"""
    p, v = np.atleast_2d(np.asarray(p, float)), np.atleast_2d(np.asarray(v, float))
    N = p.shape[0]
    planes = np.broadcast_to(np.asarray(planes, float), (N,) + np.asarray(planes).shape[-2:])
    f, fn_sum, dmin, active = np.zeros((N, 3)), np.zeros(N), np.zeros(N), np.zeros(N, int)
    for k in range(planes.shape[1]):
        w = planes[:, k]
        n, off, ks, cd, mu, vs = w[:, 0:3], w[:, 3], w[:, 4], w[:, 5], w[:, 6], w[:, 7]
        d = dot(n, p) - off
        dmin = d.copy() if k == 0 else np.where(d < dmin, d, dmin)
        on = d < 0.0
        vn = dot(n, v)
        fn = np.maximum(0.0, -ks * d - cd * vn)
        vt = v - vn[:, None] * n
        s = np.maximum(np.sqrt(dot(vt, vt)), vs)
        g = mu * fn
        ft = -(g[:, None] * vt) / s[:, None]
        fk = f + (fn[:, None] * n + ft)
        f = np.where(on[:, None], fk, f)
        fn_sum = np.where(on, fn_sum + fn, fn_sum)
        active = active + on
    return f, fn_sum, dmin, active


def joint_torque(rev, aw, oj, p, f):
    """rev (N, J) bool, aw, oj (N, J, 3), p, f (N, 3) -> (N, J): aw . ((p - oj) x f) or aw . f"""
    r = p[:, None, :] - oj
    return np.where(rev, dot(aw, cross(r, f[:, None, :])), dot(aw, np.broadcast_to(f[:, None, :], aw.shape)))


def sensor(f, p, xc, Rc, Rcs, tcs):
    """FS, MS in the sensor frame: the inverse of sensed_wrench"""
    F = -f
    m = cross(p - xc, F)
    fc, mc = matT_vec(Rc, F), matT_vec(Rc, m)
    y = mc - cross(tcs, fc)
    return matT_vec(Rcs, fc), matT_vec(Rcs, y)


def sensed_wrench(FS, MS, Rc, Rcs, tcs):
    """LAW_SENSED_WRENCH of csrc/saip_law.h: sensor frame -> control frame -> world"""
    fc = mat_vec(Rcs, FS)
    mc = mat_vec(Rcs, MS) + cross(tcs, fc)
    return mat_vec(Rc, fc), mat_vec(Rc, mc)


def summary_advance(s, dt, f, fn_sum, dmin, active):
    """s (N, 4) after one APPLY substep of length dt"""
    on = active > 0
    return np.stack([s[:, 0] + dt * fn_sum, np.maximum(s[:, 1], np.sqrt(dot(f, f))), np.maximum(s[:, 2], np.where(on, -dmin, 0.0)),
                     s[:, 3] + np.where(on, 1.0, 0.0)], axis=-1)


def plane(n, offset, k, c=0.0, mu=0.0, vs=1e-3):
    """one row of a plane table, the normal normalised the way the engine does it (n / sqrt(n.n))"""
    n = np.asarray(n, float)
    n = n / np.sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2])
    return np.array([n[0], n[1], n[2], offset, k, c, mu, vs])
