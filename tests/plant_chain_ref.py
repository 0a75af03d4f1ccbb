"""NumPy restatement of the actuation chain of the resident simulator (csrc/saip_plant_chain.h, saip_batch_plant_chain_*): per joint a delay
line of whole control periods, a slew-rate limit and a first-order lag between the commanded torque and the plant's joint arithmetic, and
the draw of the per-instance table.  Every array operation of NumPy rounds once in double precision and none is fused, which is what the
header does too (contraction off), and there is no transcendental function in it: the restatement reproduces the header bit for bit.
Shapes are those of the Python facade: commands (B, n), tables (n, 3) or (n, B, 3), taps (B, n, depth), filt (B, n, 3), primed (B, n)."""
import numpy as np

import plant_ref as PL

WORDS, MAX_DEPTH, TABLE_CHAIN = 3, 8, 9
DELAY, RATE_MAX, TAU_LAG = range(3)
X_HELD, Y_RATE, Y_LAG = range(3)
NEUTRAL = (0.0, np.inf, 0.0)


def neutral(n):
    return np.tile(NEUTRAL, (n, 1))


class Chain:
    """the state of B x n chains and pc_step over all of them"""

    def __init__(self, table, depth, B):
        table = np.asarray(table, float)
        self.n, self.B, self.depth = table.shape[0], B, int(depth)
        # the words as (B, n) arrays
        self.w = [np.ascontiguousarray(np.broadcast_to(table[..., k] if table.ndim == 2 else table[..., k].T, (B, self.n))) for k in range(WORDS)]
        self.taps = np.zeros((B, self.n, self.depth))
        self.filt = np.zeros((B, self.n, 3))
        self.primed = np.zeros((B, self.n), np.int32)

    def copy(self):
        c = Chain.__new__(Chain)
        c.__dict__.update(self.__dict__)
        c.taps, c.filt, c.primed = self.taps.copy(), self.filt.copy(), self.primed.copy()
        return c

    def step(self, t, dt, advance):
        """one substep of length dt: what pl_joint gets in place of t, (B, n); the state advances in place"""
        t = np.asarray(t, float)
        x0 = np.where(t == t, t, 0.0)
        d = np.clip(np.nan_to_num(self.w[DELAY]), 0, self.depth).astype(int)
        x_held, y_rate, y_lag = (self.filt[..., k].copy() for k in range(3))
        if advance:
            new = self.primed == 0
            self.taps[:] = np.where(new[..., None], x0[..., None], self.taps)
            y_rate = np.where(new, x0, y_rate)
            y_lag = np.where(new, x0, y_lag)
            self.primed[:] = 1
            x_held = x0.copy()
            for k in range(1, self.depth + 1):                              # the command issued d periods ago: tap d - 1
                x_held = np.where(d == k, self.taps[:, :, k - 1], x_held)
            for k in range(self.depth - 1, 0, -1):                           # taps d-1 .. 1 take their predecessor
                self.taps[:, :, k] = np.where(d > k, self.taps[:, :, k - 1], self.taps[:, :, k])
            if self.depth:
                self.taps[:, :, 0] = np.where(d > 0, x0, self.taps[:, :, 0])
        rate_max, tau_lag = self.w[RATE_MAX], self.w[TAU_LAG]
        with np.errstate(all="ignore"):
            step = rate_max * dt
            y_rate = np.where(rate_max < np.inf, y_rate + PL.pl_min(PL.pl_max(x_held - y_rate, -step), step), x_held)
            y_lag = np.where(tau_lag > 0.0, y_lag + (dt / (tau_lag + dt)) * (y_rate - y_lag), y_rate)
        self.filt[..., X_HELD], self.filt[..., Y_RATE], self.filt[..., Y_LAG] = x_held, y_rate, y_lag
        return y_lag.copy()


def draw(seed, rnd, B, lo, hi, depth):
    """(n, B, 3) from bounds (n, 3): pl_draw under the chain's table id, word index 3 j + k; delay rounded with floor(x + 0.5) and clamped to
    0..depth"""
    t = PL.draw(seed, rnd, TABLE_CHAIN, B, lo, hi)
    t[..., DELAY] = np.clip(np.floor(t[..., DELAY] + 0.5), 0.0, float(depth))
    return t
