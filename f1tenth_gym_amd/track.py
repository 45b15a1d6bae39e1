"""Track — a raceline for progress tracking (f110_track_*): a polyline of M points (x, y) in map coordinates.

Not a reference type: racing RL setups built on the reference compute progress along a centreline or raceline on the host
(NumPy projection onto the waypoints).  Here the projection runs as part of the step (BatchSim.enable_track); this class
holds the points, validates them as the library does, and builds the segment lengths, their running sum `cum` and the total
length L on the host, in float64 — the same numbers f110_track_set uploads.

Semantics: segment k runs from p_k to p_{k+1}; a closed track (the default) adds p_{M-1} -> p_0.  A closed
track whose last point equals its first bitwise drops that repeat first.  Refused (ValueError): M < 2 (M < 3 closed),
non-finite points, any zero-length segment (the closing one included; also one whose squared length underflows to 0).
"""
import numpy as np


class Track(object):
    def __init__(self, xy, closed=True):
        xy = np.array(xy, dtype=np.float64, copy=True)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("a track is an [M][2] array of (x, y) points, got shape %s" % (xy.shape,))
        if xy.shape[0] < 2:
            raise ValueError("a track needs at least 2 points, got %d" % xy.shape[0])
        closed = bool(closed)
        if closed and xy[-1].tobytes() == xy[0].tobytes():   # a closed csv repeats its first point
            xy = xy[:-1]
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
    def from_csv(cls, path, xind=1, yind=2, delim=';', skiprows=3, closed=True):
        """the raceline file the way PurePursuitPlanner reads it (conf.wpt_path, wpt_delim, wpt_rowskip, wpt_xind, wpt_yind)"""
        w = np.loadtxt(path, delimiter=delim, skiprows=skiprows)
        return cls(w[:, [int(xind), int(yind)]], closed=closed)

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

    def __repr__(self):
        return "Track(%d points, %s, L=%.5f m)" % (self.num_points, "closed" if self.closed else "open", self.length)
