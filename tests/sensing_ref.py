"""NumPy restatement of the sensing model of the resident simulator (csrc/saip_sense.h / .hip, saip_batch_sensing_*): offset, Gaussian
noise and quantisation on q, dq and the sensed wrench, the counters of the noise and the random draw of the per-instance tables.  Every
array operation of NumPy rounds once in double precision and none is fused, which is what the header does too (contraction off): with
every sigma 0 the restatement reproduces it bit for bit; with noise it differs by what log / sqrt / cos / sin of two maths libraries
differ.  Shapes are those of the Python facade: states (B, n), joint tables (n, 6) or (n, B, 6), wrench tables (6, 3) or (6, B, 3) per
task, sensed wrenches (B, 6)."""
import numpy as np

import plant_ref as PL
import sampler_ref as SR

JOINT_WORDS, AXIS_WORDS, WRENCH_WORDS, MAX_WRENCH_TASKS = 6, 3, 18, 2
TABLE_JOINTS, TABLE_WRENCHES, TABLE_JOINT_NOISE, TABLE_WRENCH_NOISE = 4, 5, 6, 7
Q_OFF, Q_RES, Q_SIGMA, DQ_OFF, DQ_RES, DQ_SIGMA = range(6)
OFF, RES, SIGMA = range(3)


def measure(x, off, res, sigma, z, quantise=True):
    """se_measure: m = x + off; sigma > 0: m = m + sigma z; res > 0: m = res rint(m / res) (np.rint rounds half to even)"""
    x, off, res, sigma, z = np.broadcast_arrays(*(np.asarray(a, float) for a in (x, off, res, sigma, z)))
    with np.errstate(all="ignore"):
        m = x + off
        m = np.where(sigma > 0.0, m + sigma * z, m)
        if quantise:
            m = np.where(res > 0.0, res * np.rint(m / np.where(res > 0.0, res, 1.0)), m)
    return m


def normals(seed, period, table, B, rows):
    """(rows, B, 2): the two standard normals of row r of instance i at counter (i, r, table << 16, period)"""
    z = SR.noise(int(seed), int(period), table, B, rows, 2)
    return z


def _words(table):
    """the words as arrays that broadcast against (B, rows): (rows,) from a batch-uniform table, (B, rows) from a per-instance one"""
    table = np.asarray(table, float)
    return [table[..., k] if table.ndim == 2 else table[..., k].T for k in range(table.shape[-1])]


def joints(table, q, dq, seed=0, period=0, quantise=True):
    """(q_meas, dq_meas), each (B, n)"""
    q, dq = np.asarray(q, float), np.asarray(dq, float)
    B, n = q.shape
    w = _words(table)
    z = normals(seed, period, TABLE_JOINT_NOISE, B, n)                  # (n, B, 2)
    return (measure(q, w[Q_OFF], w[Q_RES], w[Q_SIGMA], z[:, :, 0].T, quantise),
            measure(dq, w[DQ_OFF], w[DQ_RES], w[DQ_SIGMA], z[:, :, 1].T, quantise))


def wrench(table, f, slot=0, seed=0, period=0, quantise=True):
    """the perturbed sensed wrench (B, 6) of the task in slot `slot` from the clean one: axis a takes z[a % 2] of row 3 slot + a // 2"""
    f = np.asarray(f, float)
    B = f.shape[0]
    w = _words(table)
    z = normals(seed, period, TABLE_WRENCH_NOISE, B, 3 * (slot + 1))    # (rows, B, 2)
    zz = np.stack([z[3 * slot + a // 2, :, a % 2] for a in range(6)], axis=1)
    return measure(f, w[OFF], w[RES], w[SIGMA], zz, quantise)


def draw(seed, rnd, table, B, lo, hi):
    """(rows, B, words) from bounds (rows, words): pl_draw under the sensing tables' ids.  Joints: lo (n, 6), word index 6 j + k.  Wrenches:
    lo (S, 6, 3) or (S, 18), word index 18 s + 3 a + e; returned as (S, 6, B, 3) when the bounds were (S, 6, 3)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    if lo.ndim == 3:
        S = lo.shape[0]
        d = PL.draw(seed, rnd, table, B, lo.reshape(S, WRENCH_WORDS), hi.reshape(S, WRENCH_WORDS))  # (S, B, 18)
        return np.ascontiguousarray(d.reshape(S, B, 6, AXIS_WORDS).transpose(0, 2, 1, 3))
    return PL.draw(seed, rnd, table, B, lo, hi)
