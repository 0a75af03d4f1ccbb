"""NumPy restatement of the sensing chain of the resident simulator (csrc/saip_sense_chain.h / .hip, saip_batch_sensing_chain_*): per joint
a delay line, an optional finite-difference velocity and a first-order low-pass behind the sensing model's measured sample, and the draw of
the per-instance table.  Every array operation of NumPy rounds once in double precision and none is fused, which is what the header does
too (contraction off), and there is no transcendental function in it: the restatement reproduces the header bit for bit.  Shapes are those
of the Python facade: samples (B, n), tables (n, 4) or (n, B, 4), taps (B, n, 2, depth), filt (B, n, 3), primed (B, n)."""
import numpy as np

import plant_ref as PL

WORDS, MAX_DEPTH, TABLE_CHAIN = 4, 8, 8
DELAY, VEL_MODE, A_Q, A_DQ = range(4)
Q_PREV, Y_Q, Y_DQ = range(3)


def alpha(cutoff_hz, sample_time):
    """the facades' helper: 1 - exp(-2 pi f_c T)"""
    return 1.0 - np.exp(-2.0 * np.pi * np.asarray(cutoff_hz, float) * float(sample_time))


class Chain:
    """the state of B x n chains and sc_step over all of them"""

    def __init__(self, table, depth, sample_time, B):
        table = np.asarray(table, float)
        self.n, self.B, self.depth, self.T = table.shape[0], B, int(depth), float(sample_time)
        # the words as (B, n) arrays
        self.w = [np.ascontiguousarray(np.broadcast_to(table[..., k] if table.ndim == 2 else table[..., k].T, (B, self.n))) for k in range(WORDS)]
        self.taps = np.zeros((B, self.n, 2, self.depth))
        self.filt = np.zeros((B, self.n, 3))
        self.primed = np.zeros((B, self.n), np.int32)

    def copy(self):
        c = Chain.__new__(Chain)
        c.__dict__.update(self.__dict__)
        c.taps, c.filt, c.primed = self.taps.copy(), self.filt.copy(), self.primed.copy()
        return c

    def step(self, q_m, dq_m):
        """one sample: (q_meas, dq_meas), each (B, n); the state advances in place"""
        q_m, dq_m = np.asarray(q_m, float), np.asarray(dq_m, float)
        d = np.clip(np.nan_to_num(self.w[DELAY]), 0, self.depth).astype(int)
        new = self.primed == 0
        self.taps[:, :, 0, :] = np.where(new[..., None], q_m[..., None], self.taps[:, :, 0, :])
        self.taps[:, :, 1, :] = np.where(new[..., None], dq_m[..., None], self.taps[:, :, 1, :])
        q_prev = np.where(new, q_m, self.filt[..., Q_PREV])
        y_q = np.where(new, q_m, self.filt[..., Y_Q])
        y_dq = np.where(new, dq_m, self.filt[..., Y_DQ])
        self.primed[:] = 1
        x, v = q_m.copy(), dq_m.copy()
        for k in range(1, self.depth + 1):                              # the sample taken d samples ago: tap d - 1
            x = np.where(d == k, self.taps[:, :, 0, k - 1], x)
            v = np.where(d == k, self.taps[:, :, 1, k - 1], v)
        for k in range(self.depth - 1, 0, -1):                           # taps d-1 .. 1 take their predecessor
            self.taps[:, :, :, k] = np.where((d > k)[..., None], self.taps[:, :, :, k - 1], self.taps[:, :, :, k])
        if self.depth:
            self.taps[:, :, 0, 0] = np.where(d > 0, q_m, self.taps[:, :, 0, 0])
            self.taps[:, :, 1, 0] = np.where(d > 0, dq_m, self.taps[:, :, 1, 0])
        with np.errstate(all="ignore"):
            fd = self.w[VEL_MODE] == 1.0
            v = np.where(fd, (x - q_prev) / self.T, v)
            q_prev = np.where(fd, x, q_prev)
            a_q, a_dq = self.w[A_Q], self.w[A_DQ]
            y_q = np.where(a_q > 0.0, y_q + a_q * (x - y_q), x)
            y_dq = np.where(a_dq > 0.0, y_dq + a_dq * (v - y_dq), v)
        self.filt[..., Q_PREV], self.filt[..., Y_Q], self.filt[..., Y_DQ] = q_prev, y_q, y_dq
        return y_q.copy(), y_dq.copy()


def draw(seed, rnd, B, lo, hi, depth):
    """(n, B, 4) from bounds (n, 4): pl_draw under the chain's table id, word index 4 j + k; delay and vel_mode rounded with
    floor(x + 0.5) and clamped to 0..depth and 0..1"""
    t = PL.draw(seed, rnd, TABLE_CHAIN, B, lo, hi)
    t[..., DELAY] = np.clip(np.floor(t[..., DELAY] + 0.5), 0.0, float(depth))
    t[..., VEL_MODE] = np.clip(np.floor(t[..., VEL_MODE] + 0.5), 0.0, 1.0)
    return t
