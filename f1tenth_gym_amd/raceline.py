"""Raceline — a racing line and a speed profile for a closed track, computed on the device (f110_raceline_batch).

Not a reference type: racing stacks built on the reference take this step offline, with host programs that solve a minimum-curvature
problem per map.  Here a centreline with half widths (Track.from_map, random_track) goes in and a line that uses the corridor's width
comes out, with a speed per point: one workgroup per line, so a batch of re-carved slots costs what one does.

The rule is stated in include/f110.h and restated in NumPy in tests/raceline_ref.py; this module holds and validates the settings,
places the stations, builds the momentum table the device reads and needs no GPU.  The result is an approximation by design: nested
iteration with a fixed count and no convergence test.
"""
import math

import numpy as np

from ._spec import coerce, is_int
from .centerline import resample_closed
from .track import Track

MAX_POINTS = 4096    # F110_RACELINE_MAX_POINTS
MAX_LEVELS = 6
MAX_ITERS = 4096


def momentum(iters):
    """the table beta[k] = (t_k - 1) / t_{k+1}, t_0 = 1, t_{k+1} = (1 + sqrt(1 + 4 t_k^2)) / 2, float64 [iters]"""
    beta = np.empty(int(iters), dtype=np.float64)
    t = 1.0
    for k in range(int(iters)):
        t1 = (1.0 + math.sqrt(1.0 + 4.0 * (t * t))) / 2.0
        beta[k] = (t - 1.0) / t1
        t = t1
    return beta


class Raceline(object):
    """settings of the raceline.  spacing: metres between stations, > 0.  levels: 0 .. 6 coarsenings of the coarse-to-fine solve.
    iters: 0 .. 4096 iterations per level (0: the centreline itself).  margin: metres kept from either wall, >= 0 (the car's half
    width and then some).  v_max [m/s], a_lat, a_accel, a_brake [m/s^2]: the limits of the speed profile, > 0."""

    def __init__(self, spacing=0.4, levels=4, iters=200, margin=0.3, v_max=8.0, a_lat=7.0, a_accel=7.0, a_brake=8.0):
        if not is_int(levels) or not (0 <= levels <= MAX_LEVELS):
            raise ValueError("levels must be an integer in 0 .. %d, got %r" % (MAX_LEVELS, levels))
        if not is_int(iters) or not (0 <= iters <= MAX_ITERS):
            raise ValueError("iters must be an integer in 0 .. %d, got %r" % (MAX_ITERS, iters))
        for name, v in (("spacing", spacing), ("v_max", v_max), ("a_lat", a_lat), ("a_accel", a_accel), ("a_brake", a_brake)):
            if not (np.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError("%s must be finite and > 0, got %r" % (name, v))
        if not (np.isfinite(float(margin)) and float(margin) >= 0.0):
            raise ValueError("margin must be finite and >= 0, got %r" % (margin,))
        self.spacing, self.levels, self.iters, self.margin = float(spacing), int(levels), int(iters), float(margin)
        self.v_max, self.a_lat, self.a_accel, self.a_brake = float(v_max), float(a_lat), float(a_accel), float(a_brake)

    @classmethod
    def coerce(cls, spec):
        """a Raceline, a dict of its keyword arguments, or None for the defaults"""
        return cls() if spec is None else coerce(cls, spec, "raceline")

    def settings(self):
        """the keyword arguments that rebuild these settings"""
        return dict(spacing=self.spacing, levels=self.levels, iters=self.iters, margin=self.margin, v_max=self.v_max, a_lat=self.a_lat,
                    a_accel=self.a_accel, a_brake=self.a_brake)

    def station_count(self, length):
        """M = 2^levels * max(8, floor(L / (spacing * 2^levels) + 0.5))"""
        unit = 1 << self.levels
        return unit * max(8, int(math.floor(float(length) / (self.spacing * unit) + 0.5)))

    def stations(self, track):
        """a closed Track with a 'half_width' column -> (points [M][2], half widths [M]) at M uniform stations
        (centerline.resample_closed), M a multiple of 2^levels with at least 8 stations on the coarsest level"""
        track = Track.coerce(track)
        if not track.closed:
            raise ValueError("raceline: the track must be closed (open tracks have no lap)")
        if 'half_width' not in (track.attr_names or ()):
            raise ValueError("raceline: the track needs a 'half_width' attribute column (Track.from_map and random_track make one)")
        M = self.station_count(track.length)
        if M > MAX_POINTS:
            raise ValueError("raceline: %d stations, at most %d are solved: raise spacing (%g m) above %g m" % (M, MAX_POINTS, self.spacing, track.length / MAX_POINTS))
        col = track.attrs[:, track.attr_names.index('half_width')]
        q, w, _, _ = resample_closed(track.xy, col, track.length / M)
        if q.shape[0] != M:   # (L / (L / M) rounds to M for every M <= 4096)
            raise ValueError("raceline: %d stations came back for %d" % (q.shape[0], M))
        return np.ascontiguousarray(q), np.ascontiguousarray(w)

    def momentum(self):
        return momentum(self.iters)

    def __repr__(self):
        return "Raceline(%s)" % ", ".join("%s=%r" % kv for kv in self.settings().items())


def assemble(spec, stations, out):
    """the Tracks of BatchSim.raceline from the stations [(q, w), ...] and the call's outputs for the lines (raceline_0, centre_0,
    raceline_1, centre_1, ...): (alpha, xy, kappa, vx) rows one line after the other, length and lap_time per line"""
    alpha, xy, kappa, vx, length, lap = out
    tracks, o = [], 0
    for t, (q, w) in enumerate(stations):
        M = q.shape[0]
        a = slice(o, o + M)
        tr = Track(xy[a], closed=True, attrs={'kappa': kappa[a], 'vx': vx[a], 'offset': alpha[a]})
        tr.lap_time = float(lap[2 * t])
        tr.center = Track(q, closed=True, attrs={'half_width': w, 'kappa': kappa[o + M:o + 2 * M], 'vx': vx[o + M:o + 2 * M]})
        tr.center_lap_time = tr.center.lap_time = float(lap[2 * t + 1])
        tr.spec = spec
        tracks.append(tr)
        o += 2 * M
    return tracks


__all__ = ["Raceline", "momentum", "MAX_POINTS"]
