"""Track — a raceline for progress tracking (f110_track_*): a polyline of M points (x, y) in map coordinates.

Not a reference type: racing RL setups built on the reference compute progress along a centreline or raceline on the host
(NumPy projection onto the waypoints).  Here the projection runs as part of the step (BatchSim.enable_track); this class
holds the points, validates them as the library does, and builds the segment lengths, their running sum `cum` and the total
length L on the host, in float64 — the same numbers f110_track_set uploads.

Semantics: segment k runs from p_k to p_{k+1}; a closed track (the default) adds p_{M-1} -> p_0.  A closed
track whose last point equals its first bitwise drops that repeat first.  Refused (ValueError): M < 2 (M < 3 closed),
non-finite points, any zero-length segment (the closing one included; also one whose squared length underflows to 0).

Per-point attributes: `attrs` is an [M][C] array or a {name: column} dict of 1 .. 4 finite float64 columns, one row
per point as given (a closed track drops the repeated last row together with the point).  The track preview interpolates them
linearly along a segment, value by value: pass kappa, vx or cos / sin columns, not an angle such as psi.
"""
import numpy as np


class Track(object):
    MAX_ATTRS = 4

    def __init__(self, xy, closed=True, attrs=None):
        xy = np.array(xy, dtype=np.float64, copy=True)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("a track is an [M][2] array of (x, y) points, got shape %s" % (xy.shape,))
        if xy.shape[0] < 2:
            raise ValueError("a track needs at least 2 points, got %d" % xy.shape[0])
        closed = bool(closed)
        names = None
        if attrs is not None:
            if isinstance(attrs, dict):
                names = tuple(str(k) for k in attrs)
                attrs = np.stack([np.asarray(v, dtype=np.float64).reshape(-1) for v in attrs.values()], axis=1) if attrs else np.zeros((xy.shape[0], 0))
            attrs = np.array(attrs, dtype=np.float64, copy=True)
            if attrs.ndim != 2 or attrs.shape[0] != xy.shape[0]:
                raise ValueError("a track's attributes are an [M][C] array with a row per point (M = %d), got shape %s" % (xy.shape[0], attrs.shape))
            if not (1 <= attrs.shape[1] <= self.MAX_ATTRS):
                raise ValueError("a track carries 1 .. %d attributes per point, got %d" % (self.MAX_ATTRS, attrs.shape[1]))
            if not np.all(np.isfinite(attrs)):
                raise ValueError("a track's attributes must be finite")
        if closed and xy[-1].tobytes() == xy[0].tobytes():   # a closed csv repeats its first point
            xy = xy[:-1]
            attrs = None if attrs is None else attrs[:-1]
        if closed and xy.shape[0] < 3:
            raise ValueError("a closed track needs at least 3 distinct points, got %d" % xy.shape[0])
        if not np.all(np.isfinite(xy)):
            raise ValueError("a track's points must be finite")
        b = np.roll(xy, -1, axis=0) if closed else xy[1:]
        a = xy if closed else xy[:-1]
        d = b - a
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        if not np.all(l2 > 0.0):
            k = int(np.flatnonzero(~(l2 > 0.0))[0])
            raise ValueError("segment %d -> %d of the track has zero length" % (k, (k + 1) % xy.shape[0]))
        self.xy = xy
        self.closed = closed
        self.attrs = attrs
        self.attr_names = names
        self.seg_len = np.sqrt(l2)
        cum = np.empty(self.seg_len.shape[0])
        acc = 0.0
        for k, v in enumerate(self.seg_len):   # the running float64 sum, in order (np.cumsum may pair terms)
            cum[k] = acc
            acc += float(v)
        self.cum = cum
        self.length = acc

    @classmethod
    def from_xy(cls, xy, closed=True):
        return cls(xy, closed=closed)

    @classmethod
    def from_csv(cls, path, xind=1, yind=2, delim=';', skiprows=3, closed=True, attrs=None):
        """the raceline file the way PurePursuitPlanner reads it (conf.wpt_path, wpt_delim, wpt_rowskip, wpt_xind, wpt_yind);
        attrs: {name: column index} of per-point attributes, e.g. {'kappa': 4, 'vx': 5} for the example raceline"""
        w = np.loadtxt(path, delimiter=delim, skiprows=skiprows)
        cols = None if attrs is None else {k: w[:, int(c)] for k, c in dict(attrs).items()}
        return cls(w[:, [int(xind), int(yind)]], closed=closed, attrs=cols)

    @classmethod
    def from_map(cls, sim, slot=0, **kw):
        """the centreline of a map slot, extracted on the device: BatchSim.centerline(slot, **kw) — seed, heading,
        spacing, smooth, max_passes.  sim: a BatchSim, or an env layer that holds one."""
        sim = getattr(sim, "sim", sim)        # F110Env / F110VecEnv -> their Simulator
        sim = getattr(sim, "batch", sim)      # Simulator -> its BatchSim
        return sim.centerline(slot, **kw)

    def raceline(self, sim, spec=None):
        """this track's racing line and speed profile, solved on the device: BatchSim.raceline(self, spec).  The track
        must be closed and carry a 'half_width' column.  sim: a BatchSim, or an env layer that holds one."""
        sim = getattr(sim, "sim", sim)
        sim = getattr(sim, "batch", sim)
        return sim.raceline(self, spec)

    @classmethod
    def coerce(cls, track):
        """a Track, an [M][2] array (closed) or a csv path (PurePursuitPlanner's defaults: x, y in columns 1, 2)"""
        if isinstance(track, Track):
            return track
        if isinstance(track, str):
            return cls.from_csv(track)
        return cls(track)

    @property
    def num_points(self):
        return int(self.xy.shape[0])

    @property
    def num_segments(self):
        return int(self.seg_len.shape[0])

    def points_closed(self):
        """the points the reference's nearest_point_on_trajectory sees for this track: p_0 appended when closed"""
        return np.vstack([self.xy, self.xy[:1]]) if self.closed else self.xy

    def point_at(self, s):
        """arc lengths s [m] (a closed track wraps them into [0, L), an open one clips them to [0, L]) -> (xy [m][2], unit
        tangent [m][2]) on the polyline.  Host work: what places obstacles per map slot (Obstacles.random_on_track)."""
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        L = self.length
        s = np.mod(s, L) if self.closed else np.clip(s, 0.0, L)
        k = np.clip(np.searchsorted(self.cum, s, side='right') - 1, 0, self.num_segments - 1)
        pts = self.points_closed()
        a, d = pts[:-1], pts[1:] - pts[:-1]
        t = np.clip((s - self.cum[k]) / self.seg_len[k], 0.0, 1.0)
        return a[k] + t[:, None] * d[k], d[k] / self.seg_len[k][:, None]

    def wrap_ds(self, ds):
        """progress of one step wrapped into (-L/2, L/2] on a closed track (open: unchanged)"""
        ds = np.array(ds, dtype=np.float64, copy=True)
        if self.closed:
            L = self.length
            ds = np.where(ds > 0.5 * L, ds - L, np.where(ds <= -0.5 * L, ds + L, ds))
        return ds

    def project(self, poses):
        """NumPy restatement of the device projection for host poses [m][3]: -> [m][5] = s, lateral, heading_error,
        segment, t.  The same per-segment arithmetic as nearest_point_on_trajectory (first minimum)."""
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        pts = self.points_closed()
        a, d = pts[:-1], pts[1:] - pts[:-1]
        l2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
        out = np.empty((poses.shape[0], 5))
        for r, (px, py, th) in enumerate(poses):
            t = ((px - a[:, 0]) * d[:, 0] + (py - a[:, 1]) * d[:, 1]) / l2
            t = np.clip(t, 0.0, 1.0)
            rx = px - (a[:, 0] + t * d[:, 0])
            ry = py - (a[:, 1] + t * d[:, 1])
            dist = np.sqrt(rx * rx + ry * ry)
            k = int(np.argmin(dist))
            tk = float(t[k])      # (a NaN pose: segment 0 with t and distance NaN, as the reference's np.clip leaves them)
            cross = d[k, 0] * ry[k] - d[k, 1] * rx[k]
            herr = np.mod(th - np.arctan2(d[k, 1], d[k, 0]) + np.pi, 2 * np.pi) - np.pi
            out[r] = (self.cum[k] + tk * self.seg_len[k], -dist[k] if cross < 0 else dist[k], herr, k, tk)
        return out

    @property
    def num_attrs(self):
        return 0 if self.attrs is None else int(self.attrs.shape[1])

    def preview(self, poses, s, preview, raw=False, segments=False):
        """NumPy restatement of the device preview (include/f110.h, f110_track_preview) for host poses [m][3] and their arc
        lengths s [m]: -> float32 [m][P][D] (and, asked for, raw float64 [m][P][8] before scaling with absent attributes 0.0,
        and the stations' segments int32 [m][P]).  It does not project: s is project()'s first column."""
        from .track_preview import TrackPreview, CHANNELS
        pv = TrackPreview.coerce(preview)
        pv.check_track(self)
        poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        s = np.asarray(s, dtype=np.float64).reshape(-1)
        if s.shape[0] != poses.shape[0]:
            raise ValueError("s must hold one arc length per pose")
        pts = self.points_closed()
        a, d = pts[:-1], pts[1:] - pts[:-1]
        L, n = self.length, self.num_segments
        dj = pv.offset + np.arange(pv.points, dtype=np.float64) * pv.spacing
        with np.errstate(invalid='ignore'):
            sj = s[:, None] + dj[None, :]
            if self.closed:
                sj = np.where(sj >= L, sj - L, sj)
            k = np.searchsorted(self.cum, sj, side='right') - 1     # the last segment with cum[k] <= s_j ...
            k = np.where(np.isnan(sj) | (k < 0), 0, k)               # ... 0 when there is none (NaN sorts behind everything)
            ln = self.seg_len[k]
            t = np.clip((sj - self.cum[k]) / ln, 0.0, 1.0)
            X, Y = a[k, 0] + t * d[k, 0], a[k, 1] + t * d[k, 1]
            ux, uy = d[k, 0] / ln, d[k, 1] / ln
            rawv = np.zeros(sj.shape + (8,))
            if pv.frame == 'world':
                rawv[..., 0], rawv[..., 1], rawv[..., 2], rawv[..., 3] = X, Y, ux, uy
            else:
                c, sn = np.cos(poses[:, 2])[:, None], np.sin(poses[:, 2])[:, None]
                rx, ry = X - poses[:, 0:1], Y - poses[:, 1:2]
                rawv[..., 0], rawv[..., 1] = c * rx + sn * ry, c * ry - sn * rx
                rawv[..., 2], rawv[..., 3] = c * ux + sn * uy, c * uy - sn * ux
            k1 = np.where(k + 1 == self.num_points, 0, k + 1)
            for q in range(self.num_attrs):
                col = self.attrs[:, q]
                rawv[..., 4 + q] = col[k] + t * (col[k1] - col[k])
            bits = [CHANNELS.index(ch) for ch in pv.channels]
            out = (rawv[..., bits] / np.array([pv.scale[CHANNELS[b]] for b in bits])).astype(np.float32)
        res = [out]
        if raw:
            res.append(rawv)
        if segments:
            res.append(k.astype(np.int32))
        return res[0] if len(res) == 1 else tuple(res)

    def __repr__(self):
        return "Track(%d points, %s, L=%.5f m)" % (self.num_points, "closed" if self.closed else "open", self.length)
