"""NumPy restatement of one evaluation of the resident guards (sai-primitives_amd/csrc/saip_guard.h), vectorised over the instances.
Every product and sum is one NumPy operation on doubles, hence rounded on its own, in the order the header writes them; the rest is
integer arithmetic.  The tests compare it bit for bit with the host build of the header and with the kernel."""
import numpy as np

MAX_PHASES, MAX_GUARDS, WORDS, PHASE_WORDS, READOUT_ROWS, LATCH_ROWS = 8, 8, 8, 4, 8, 12
FROM, TO, SIGNAL, AXIS, CMP, THRESHOLD, HOLD, BLANK = range(8)
PERIODS, FORCE, MOMENT, POSITION, POS_ERROR, ORI_ERROR, JOINT_SPEED = range(7)
GE, LE = 0, 1
FREE, HOLD_MODE, OFFSET = 0, 1, 2
READ_FORCE, READ_MOMENT, READ_POS_ERROR, READ_ORI_ERROR, READ_JOINT_SPEED, READ_POSITION = range(6)


def norm3(e):
    """sqrt((e0 e0 + e1 e1) + e2 e2) of (..., 3)"""
    e = np.asarray(e, float)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.sqrt((e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2])


def guard(frm, to, signal, threshold, axis=0, cmp=GE, hold=1, blank=0):
    return [frm, to, signal, axis, cmp, threshold, hold, blank]


class Guards:
    """guards: (G, 8), or (G, 8, N) per instance (the layout of the C ABI); phases: (P, 4); the state as _attach leaves it"""

    def __init__(self, guards, phases, N):
        g = np.asarray(guards, float)
        self.table = np.repeat(g[:, :, None], N, axis=2) if g.ndim == 2 else g.copy()
        self.phases = np.asarray(phases, float).reshape(-1, PHASE_WORDS)
        self.G, self.P, self.N = self.table.shape[0], self.phases.shape[0], N
        assert self.table.shape == (self.G, WORDS, N)
        self.reset()

    def reset(self):
        N = self.N
        self.phase, self.since, self.clock = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
        self.run, self.fires = np.zeros((self.G, N), np.int32), np.zeros((self.G, N), np.int32)
        self.entry = np.full((self.P, N), -1, np.int32)
        self.entry[0] = 0
        self.latch = np.zeros((LATCH_ROWS, N))

    def state(self):
        return dict(phase=self.phase.copy(), since=self.since.copy(), clock=self.clock.copy(), run=self.run.copy(), entry=self.entry.copy(), fires=self.fires.copy(),
                    latch=self.latch.copy())

    @staticmethod
    def signal(sig, axis, since, f, m, pos, ep, eo, speed):
        """sig, axis (N,) ints; f, m, pos (N, 3); ep, eo, speed (N,)"""
        nan = np.full(since.shape, np.nan)

        def wrench(w):
            return np.where(axis == 0, w[:, 0], np.where(axis == 1, w[:, 1], np.where(axis == 2, w[:, 2], norm3(w))))

        position = np.where(axis == 0, pos[:, 0], np.where(axis == 1, pos[:, 1], np.where(axis == 2, pos[:, 2], nan)))
        out = nan
        for code, val in ((PERIODS, since.astype(float)), (FORCE, wrench(f)), (MOMENT, wrench(m)), (POSITION, position), (POS_ERROR, ep), (ORI_ERROR, eo),
                          (JOINT_SPEED, speed)):
            out = np.where(sig == code, val, out)
        return out

    def step(self, goal, f=None, m=None, pos=None, ep=None, eo=None, speed=None, pose=None):
        """one evaluation of every instance.  goal: (>= 24, N), rows 0..23 written in place by HOLD / OFFSET phases; the signal inputs
        default to NaN (what a launch that did not need them feeds); pose: (12, N) or None (the launch computed none)"""
        N, idx = self.N, np.arange(self.N)
        nan3, nan1 = np.full((N, 3), np.nan), np.full(N, np.nan)
        f, m, pos = (nan3 if a is None else np.asarray(a, float) for a in (f, m, pos))
        ep, eo, speed = (nan1 if a is None else np.asarray(a, float) for a in (ep, eo, speed))
        p, sn = self.phase.copy(), self.since.copy()
        fired, to = np.full(N, -1), np.zeros(N, np.int64)
        for g in range(self.G):
            w = self.table[g]
            active = (w[FROM] == p) & ~(sn < w[BLANK])
            s = self.signal(w[SIGNAL].astype(np.int64), w[AXIS].astype(np.int64), sn, f, m, pos, ep, eo, speed)
            with np.errstate(invalid="ignore"):
                c = np.where(w[CMP] == LE, s <= w[THRESHOLD], s >= w[THRESHOLD])
            r = np.where(active & c, self.run[g] + 1, 0).astype(np.int32)
            hit = active & (fired < 0) & (r >= w[HOLD])
            fired[hit] = g
            t = w[TO]
            to[hit] = np.where(t >= 1.0, np.where(t < self.P, t, self.P - 1), 0)[hit].astype(np.int64)
            self.run[g] = r
        fd = fired >= 0
        self.fires[fired[fd], idx[fd]] += 1
        now = np.where(fd, to, p).astype(np.int32)
        self.phase = now
        self.since = np.where(fd, 0, sn + 1).astype(np.int32)
        self.run[:, fd] = 0
        first = fd & (self.entry[now, idx] < 0)
        self.entry[now[first], idx[first]] = self.clock[first]
        if pose is not None:
            self.latch[:, fd] = np.asarray(pose, float)[:, fd]
        ph = self.phases[np.clip(now, 0, self.P - 1)]
        writes, off = (ph[:, 0] == HOLD_MODE) | (ph[:, 0] == OFFSET), ph[:, 0] == OFFSET
        with np.errstate(invalid="ignore", over="ignore"):
            moved = self.latch[0:3] + ph[:, 1:4].T
        goal[0:3, writes] = np.where(off, moved, self.latch[0:3])[:, writes]
        goal[3:12, writes] = self.latch[3:12][:, writes]
        goal[12:24, writes] = 0.0
        self.clock = self.clock + 1
        return fired


def cost(cost, entry, w_time, w_miss):
    """saip_batch_guard_add_cost: cost + (entry >= 0 ? w_time (double)entry : w_miss)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(cost, float) + np.where(entry >= 0, w_time * entry.astype(float), w_miss)
