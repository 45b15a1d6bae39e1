"""A NumPy statement of the start-pose draw (include/f110.h f110_reset_sampler): every env owns
np.random.Generator(PCG64(SeedSequence(seed, spawn_key=(env_base + e,)))), every attempt consumes 1 + 2A uniforms in the
documented order, and x, y follow the documented operation order (bitwise comparable with the device); theta goes through
NumPy's arctan2 (the device's atan2 may differ by an ulp)."""
import numpy as np


class SlotModel(object):
    """what a draw reads of one map slot: the track's segment table and the slot's distance table"""

    def __init__(self, track, dt, res, origin):
        self.closed = bool(track.closed)
        a = track.xy
        b = np.roll(a, -1, axis=0) if self.closed else a[1:]
        a = a if self.closed else a[:-1]
        self.ax, self.ay = a[:, 0].copy(), a[:, 1].copy()
        self.dx, self.dy = b[:, 0] - a[:, 0], b[:, 1] - a[:, 1]
        self.len, self.cum, self.L = track.seg_len, track.cum, float(track.length)
        self.dt = np.asarray(dt, dtype=np.float64)
        self.res = float(res)
        self.ox, self.oy = float(origin[0]), float(origin[1])
        self.oc, self.os = np.cos(float(origin[2])), np.sin(float(origin[2]))
        self.H, self.W = self.dt.shape

    def rc(self, x, y):
        """xy_2_rc (laser_models.py:55-86)"""
        xt, yt = x - self.ox, y - self.oy
        xr = xt * self.oc + yt * self.os
        yr = -xt * self.os + yt * self.oc
        if xr < 0 or xr >= self.W * self.res or yr < 0 or yr >= self.H * self.res:
            return -1, -1
        return int(yr / self.res), int(xr / self.res)

    def segment(self, s):
        k = int(np.searchsorted(self.cum, s, side="right")) - 1
        return max(k, 0)


class SamplerModel(object):
    def __init__(self, seed, num_envs, num_agents, slots, env_slot=None, s_range=(0.0, 1.0), gap=1.0, lateral=0.0,
                 heading=0.0, clearance=0.0, attempts=16, env_base=0):
        self.E, self.A = int(num_envs), int(num_agents)
        self.slots = slots
        self.env_slot = np.zeros(self.E, dtype=np.int64) if env_slot is None else np.asarray(env_slot)
        self.s_lo, self.s_hi = float(s_range[0]), float(s_range[1])
        self.gap, self.lateral, self.heading = float(gap), float(lateral), float(heading)
        self.clearance, self.attempts = float(clearance), int(attempts)
        self.gens = [np.random.Generator(np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(int(env_base) + e,))))
                     for e in range(self.E)]
        self.uniforms = np.zeros(self.E, dtype=np.int64)   # uniforms each env's stream has handed out

    def _u(self, e):
        self.uniforms[e] += 1
        return self.gens[e].random()

    def attempt(self, e):
        """one attempt for env e: (poses [A][3], arc lengths [A], valid)"""
        m = self.slots[int(self.env_slot[e])]
        poses, ss = np.empty((self.A, 3)), np.empty(self.A)
        valid = True
        s0 = m.L * (self.s_lo + self._u(e) * (self.s_hi - self.s_lo))
        for j in range(self.A):
            s = s0 - float(j) * self.gap
            if m.closed:
                s = float(np.fmod(s, m.L))
                if s < 0.0:
                    s += m.L
            ul, uh = self._u(e), self._u(e)
            d = self.lateral * (2.0 * ul - 1.0)
            h = self.heading * (2.0 * uh - 1.0)
            k = m.segment(s)
            t = min(max((s - m.cum[k]) / m.len[k], 0.0), 1.0)
            x = (m.ax[k] + t * m.dx[k]) + d * (-m.dy[k] / m.len[k])
            y = (m.ay[k] + t * m.dy[k]) + d * (m.dx[k] / m.len[k])
            poses[j] = (x, y, np.arctan2(m.dy[k], m.dx[k]) + h)
            ss[j] = s
            r, c = m.rc(x, y)
            valid = valid and (m.closed or s >= 0.0) and r >= 0 and m.dt[r, c] >= self.clearance
        need = (2.0 * self.clearance) * (2.0 * self.clearance)
        for p in range(self.A):
            for q in range(p + 1, self.A):
                ddx, ddy = poses[p, 0] - poses[q, 0], poses[p, 1] - poses[q, 1]
                valid = valid and (ddx * ddx + ddy * ddy >= need)
        return poses, ss, valid

    def draw(self, e):
        """one draw for env e: (poses [A][3] or None for a fallback, winning attempt or -1)"""
        for att in range(self.attempts):
            poses, _, ok = self.attempt(e)
            if ok:
                return poses, att
        return None, -1

    def valid(self, e, poses):
        """the validity rule for given poses of env e (open tracks: the arc lengths are not known here; callers check s)"""
        m = self.slots[int(self.env_slot[e])]
        for x, y, _ in poses:
            r, c = m.rc(x, y)
            if r < 0 or not m.dt[r, c] >= self.clearance:
                return False
        need = (2.0 * self.clearance) ** 2
        for p in range(self.A):
            for q in range(p + 1, self.A):
                ddx, ddy = poses[p, 0] - poses[q, 0], poses[p, 1] - poses[q, 1]
                if not ddx * ddx + ddy * ddy >= need:
                    return False
        return True


def wrap_diff(a, b):
    """a - b wrapped into [-pi, pi)"""
    return np.mod(np.asarray(a) - np.asarray(b) + np.pi, 2 * np.pi) - np.pi
