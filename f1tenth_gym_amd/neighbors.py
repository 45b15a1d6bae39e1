"""Neighbors — each agent's K nearest opponents of its own env, in its own frame, computed on the device.

Not a reference type: overtaking, blocking and self-play setups built on the reference copy every pose back and run an all-pairs
search in NumPy.  Here one call (BatchSim.neighbors_device) turns the poses, speeds and arc lengths of the step just taken into
float32 [N][K][D] where they already are: per neighbour its position, distance, relative heading and velocity in the ego frame,
its gap along the track, a validity flag and its index.  This class holds and validates the settings (include/f110.h,
f110_neighbors), restates the rule in NumPy (compute) and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

# channel name -> bit number; the output holds the requested channels in this order whatever order they are asked for in
CHANNELS = ("dx", "dy", "dist", "cos_dth", "sin_dth", "v_x", "v_y", "gap_s", "valid", "index")
MAX_K = _ffi.NBR_MAX_K
MAX_AGENTS = _ffi.NBR_MAX_AGENTS


class Neighbors(object):
    """settings of the neighbour observation.  k: K slots per agent, 1 .. 8, filled with the nearest other agents of the same env
    by ascending squared distance (ties by ascending index).  channels: names from CHANNELS.  max_range: metres, > 0 (inf: no
    limit); an agent exactly max_range away still counts.  pad: what an empty slot holds in every channel but 'valid' (0.0 there),
    finite.  scale: {channel: divisor} (default 1.0), finite and non-zero.  The output is float32 [N][K][D], D = len(channels)."""

    def __init__(self, k=1, channels=('dx', 'dy'), max_range=np.inf, pad=0.0, scale=None):
        if not is_int(k) or not (1 <= k <= MAX_K):
            raise ValueError("k must be an integer in 1 .. %d, got %r" % (MAX_K, k))
        if isinstance(channels, str):
            channels = (channels,)
        channels = tuple(channels)
        for c in channels:
            if c not in CHANNELS:
                raise ValueError("unknown channel %r (known: %s)" % (c, ", ".join(CHANNELS)))
        if not channels:
            raise ValueError("neighbors need at least one channel")
        if len(set(channels)) != len(channels):
            raise ValueError("a channel is listed twice: %r" % (channels,))
        max_range, pad = float(max_range), float(pad)
        if not (max_range > 0.0):
            raise ValueError("max_range must be > 0 (inf is allowed), got %r" % (max_range,))
        if not np.isfinite(pad):
            raise ValueError("pad must be finite, got %r" % (pad,))
        scale = dict(scale or {})
        for key, v in scale.items():
            if key not in CHANNELS:
                raise ValueError("scale: unknown channel %r" % (key,))
            if key in channels and not (np.isfinite(float(v)) and float(v) != 0.0):
                raise ValueError("scale[%r] must be finite and non-zero, got %r" % (key, v))
        self.k, self.max_range, self.pad = int(k), max_range, pad
        self.channels = tuple(c for c in CHANNELS if c in channels)   # the fixed output order
        self.scale = {c: (float(scale[c]) if c in scale and c in channels else 1.0) for c in CHANNELS}
        self.dim = len(self.channels)

    @classmethod
    def coerce(cls, spec):
        """a Neighbors, or a dict of its keyword arguments"""
        return coerce(cls, spec, "neighbors")

    @property
    def channel_mask(self):
        return sum(1 << CHANNELS.index(c) for c in self.channels)

    @property
    def needs_track(self):
        """'gap_s' reads the track column s"""
        return "gap_s" in self.channels

    def shape(self, num_agents_total):
        """the output shape [N][K][D]"""
        return (int(num_agents_total), self.k, self.dim)

    def spec(self):
        """the C struct"""
        return _ffi.NeighborsSpec(self.k, self.channel_mask, 0, 0, self.max_range, self.pad,
                                  (_ffi.C.c_double * 10)(*[self.scale[c] for c in CHANNELS]))

    def settings(self):
        """the keyword arguments that rebuild these settings"""
        return dict(k=self.k, channels=self.channels, max_range=self.max_range, pad=self.pad, scale={c: self.scale[c] for c in self.channels})

    def compute(self, poses, v, s, A, track_L=0.0, raw=False, indices=False):
        """the rule of include/f110.h in NumPy: poses [m][3], v [m], s [m] (or None: zeros) in env-major order, m a multiple of A;
        track_L > 0 wraps 'gap_s' as a closed track of that length -> float32 [m][K][D]; with raw also float64 [m][K][10] (every
        channel before scaling; an empty slot pad, 'valid' 0.0), with indices also int32 [m][K] (-1: empty)"""
        p = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        m, A, K = p.shape[0], int(A), self.k
        if not (1 <= A <= MAX_AGENTS) or m % A:
            raise ValueError("A must be in 1 .. %d and divide the row count" % MAX_AGENTS)
        track_L = float(track_L)
        if not (np.isfinite(track_L) and track_L >= 0.0):
            raise ValueError("track_L must be finite and >= 0 (0: no wrap)")
        E = m // A
        col = lambda a: np.zeros((E, A)) if a is None else np.asarray(a, dtype=np.float64).reshape(E, A)   # noqa: E731
        x, y, th = p[:, 0].reshape(E, A), p[:, 1].reshape(E, A), p[:, 2].reshape(E, A)
        vv, ss = col(v), col(s)
        c, sn = np.cos(th), np.sin(th)
        R2 = np.float64(self.max_range) * np.float64(self.max_range)
        with np.errstate(invalid="ignore", over="ignore"):
            rx, ry = x[:, None, :] - x[:, :, None], y[:, None, :] - y[:, :, None]       # [e][a][b]: b as a sees it
            d2 = rx * rx + ry * ry
            ok = (d2 <= R2) & ~np.eye(A, dtype=bool)[None]
            # ascending d2 among the eligible, ties by ascending b, the ineligible behind them
            order = np.lexsort((np.broadcast_to(np.arange(A), d2.shape), np.where(ok, d2, 0.0), ~ok), axis=-1)
            count = ok.sum(axis=-1)
            idx = np.full((E, A, K), -1, dtype=np.int32)
            kk = min(K, A)
            idx[..., :kk] = np.where(np.arange(kk)[None, None, :] < count[..., None], order[..., :kk], -1)
            valid = idx >= 0
            b = np.where(valid, idx, 0).astype(np.int64)
            take = lambda q: np.take_along_axis(np.broadcast_to(q[:, None, :], (E, A, A)), b, axis=2)   # noqa: E731
            rxk, ryk = take(x) - x[..., None], take(y) - y[..., None]
            ca, sa, va = c[..., None], sn[..., None], vv[..., None]
            cb, sb, vb = take(c), take(sn), take(vv)
            cd, sd = cb * ca + sb * sa, sb * ca - cb * sa
            g = take(ss) - ss[..., None]
            if track_L > 0.0:
                half = 0.5 * track_L
                g = np.where(g > half, g - track_L, np.where(g <= -half, g + track_L, g))
            vals = [ca * rxk + sa * ryk, ca * ryk - sa * rxk, np.sqrt(rxk * rxk + ryk * ryk), cd, sd, vb * cd - va, vb * sd, g,
                    np.ones(b.shape), b.astype(np.float64)]
            rw = np.stack([np.where(valid, q, 0.0 if n == 8 else self.pad) for n, q in enumerate(vals)], axis=-1)
            bits = [CHANNELS.index(ch) for ch in self.channels]
            out = np.stack([np.where(valid, (vals[n] / np.float64(self.scale[CHANNELS[n]])).astype(np.float32),
                                     np.float32(0.0 if n == 8 else self.pad)) for n in bits], axis=-1).astype(np.float32)
        res = [out.reshape(m, K, self.dim)] + ([rw.reshape(m, K, 10)] if raw else []) + ([idx.reshape(m, K)] if indices else [])
        return res[0] if len(res) == 1 else tuple(res)

    def __repr__(self):
        return "Neighbors(k=%d, channels=%r, max_range=%r, pad=%r)" % (self.k, self.channels, self.max_range, self.pad)


__all__ = ["Neighbors", "CHANNELS"]
