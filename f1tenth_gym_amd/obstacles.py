"""Obstacles — static boxes and discs stamped into a map slot on the device (f110_add_map_obstacles).

Not a reference type: with the reference an obstacle is drawn into the map image and the map is loaded again.  Here a DERIVED map
slot takes a list of shapes; the library stamps them into the slot's distance table (BatchSim.add_obstacle_map / set_obstacles),
and the scan, the wall check, the reset sampler, the rollout and the render see them because they read that table.

An Obstacles object is an immutable list of shapes, validated by the library's rules (include/f110.h): at most 256 shapes, finite
fields, half extents >= 0.  A box is (x, y, yaw, length, width) — full extents, as a car's; a disc (x, y, radius).  The cosine and
sine of the yaw are computed HERE (NumPy) and handed to the device as numbers, so the stamp rule involves no device trigonometry.
"""
import numpy as np

from . import _ffi

BOX, DISC = _ffi.OBST_BOX, _ffi.OBST_DISC
MAX_OBSTACLES = _ffi.MAX_OBSTACLES
FIELDS = ("shape", "x", "y", "c", "s", "half_length", "half_width")


class Obstacles(object):
    __slots__ = ("_rows",)

    def __init__(self, rows=()):
        """rows [n][7] = shape, x, y, cos(yaw), sin(yaw), half_length, half_width (the struct's fields; see boxes / discs)"""
        rows = np.array(rows, dtype=np.float64, copy=True).reshape(-1, 7) if np.size(rows) else np.zeros((0, 7))
        if rows.shape[0] > MAX_OBSTACLES:
            raise ValueError("a map slot takes at most %d obstacles, got %d" % (MAX_OBSTACLES, rows.shape[0]))
        if not np.all(np.isfinite(rows)):
            raise ValueError("an obstacle has a non-finite field")
        if not np.all((rows[:, 0] == BOX) | (rows[:, 0] == DISC)):
            raise ValueError("unknown obstacle shape (0 = box, 1 = disc)")
        if np.any(rows[:, 5] < 0) or np.any(rows[:, 6] < 0):
            raise ValueError("an obstacle has a negative half extent")
        rows.setflags(write=False)
        object.__setattr__(self, "_rows", rows)

    def __setattr__(self, *a):
        raise AttributeError("Obstacles is immutable")

    @staticmethod
    def _column(v, n, what):
        v = np.asarray(v, dtype=np.float64)
        if v.ndim == 0:
            return np.full(n, float(v))
        if v.shape != (n,):
            raise ValueError("%s must be a number or one per obstacle (%d), got shape %s" % (what, n, v.shape))
        return v

    @classmethod
    def boxes(cls, xy, yaw, length, width):
        """boxes centred on xy [n][2] (or one (x, y)) with yaw, full length (along the yaw) and full width: numbers or [n]"""
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        yaw = cls._column(yaw, n, "yaw")
        rows = np.column_stack([np.full(n, float(BOX)), xy[:, 0], xy[:, 1], np.cos(yaw), np.sin(yaw),
                                0.5 * cls._column(length, n, "length"), 0.5 * cls._column(width, n, "width")])
        return cls(rows)

    @classmethod
    def discs(cls, xy, radius):
        xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
        n = xy.shape[0]
        rows = np.column_stack([np.full(n, float(DISC)), xy[:, 0], xy[:, 1], np.ones(n), np.zeros(n), cls._column(radius, n, "radius"), np.zeros(n)])
        return cls(rows)

    @classmethod
    def coerce(cls, obstacles):
        """an Obstacles, None (no obstacle) or an [n][7] array of rows"""
        if isinstance(obstacles, Obstacles):
            return obstacles
        if obstacles is None:
            return cls()
        return cls(obstacles)

    def __add__(self, other):
        if not isinstance(other, Obstacles):
            return NotImplemented
        return Obstacles(np.vstack([self._rows, other._rows]))

    def __len__(self):
        return int(self._rows.shape[0])

    def __eq__(self, other):
        return isinstance(other, Obstacles) and self._rows.shape == other._rows.shape and self._rows.tobytes() == other._rows.tobytes()

    def __hash__(self):
        return hash(self._rows.tobytes())

    @property
    def rows(self):
        """[n][7] read-only: shape, x, y, cos(yaw), sin(yaw), half_length, half_width"""
        return self._rows

    @property
    def xy(self):
        return self._rows[:, 1:3]

    def structs(self):
        """the list as a ctypes array of struct f110_obstacle (None when empty)"""
        n = len(self)
        if n == 0:
            return None
        arr = (_ffi.Obstacle * n)()
        for i, r in enumerate(self._rows):
            arr[i].shape = int(r[0])
            arr[i].x, arr[i].y, arr[i].c, arr[i].s, arr[i].half_length, arr[i].half_width = (float(v) for v in r[1:])
        return arr

    @classmethod
    def random_on_track(cls, track, n, seed, s_range=(0.0, 1.0), lateral=0.3, length=(0.3, 0.5), width=(0.2, 0.4), radius=(0.1, 0.2),
                        disc_fraction=0.5, yaw=np.pi, keep_clear=(), min_gap=1.0, return_s=False):
        """n obstacles along a Track, drawn on the host with np.random.default_rng(seed): deterministic for a seed.

        Arc lengths are drawn in s_range (fractions of the track's length L) outside every keep_clear stretch [(s0, s1), ...]
        (fractions too; s0 > s1 wraps through the start of a closed track), sorted, and thinned so that consecutive obstacles (on
        a closed track also the last and the first) are at least min_gap metres of arc length apart; the draw repeats until n are
        placed and raises ValueError after 64 rounds.  Each centre is the track's point at s moved along the left normal by a
        uniform offset in [-lateral, lateral]; a box's yaw is the tangent's plus a uniform angle in [-yaw / 2, yaw / 2].  length,
        width and radius are numbers or (lo, hi) ranges; disc_fraction is the probability of a disc.  return_s: also the arc
        lengths [n] (metres, ascending) the centres were placed at."""
        from .track import Track
        track = Track.coerce(track)
        n = int(n)
        if n < 0 or n > MAX_OBSTACLES:
            raise ValueError("n must be in 0..%d, got %d" % (MAX_OBSTACLES, n))
        lo, hi = float(s_range[0]), float(s_range[1])
        if not (0.0 <= lo < hi <= 1.0):
            raise ValueError("s_range must satisfy 0 <= lo < hi <= 1")
        lateral, min_gap, disc_fraction = float(lateral), float(min_gap), float(disc_fraction)
        if not (lateral >= 0 and min_gap >= 0 and 0.0 <= disc_fraction <= 1.0 and np.isfinite(lateral) and np.isfinite(min_gap)):
            raise ValueError("lateral and min_gap must be finite and >= 0, disc_fraction in [0, 1]")
        clear = [(float(a), float(b)) for a, b in keep_clear]

        def span(v, what):
            v = np.asarray(v, dtype=np.float64).reshape(-1)
            a, b = (float(v[0]), float(v[0])) if v.size == 1 else (float(v[0]), float(v[1]))
            if not (0.0 <= a <= b and np.isfinite(b)):
                raise ValueError("%s must be a number or a (lo, hi) range with 0 <= lo <= hi" % what)
            return a, b
        length, width, radius = span(length, "length"), span(width, "width"), span(radius, "radius")
        L = track.length
        rng = np.random.default_rng(seed)

        def is_clear(f):
            for a, b in clear:
                if (a <= f <= b) if a <= b else (f >= a or f <= b):
                    return False
            return True

        kept = []
        for _ in range(64):
            if len(kept) >= n:
                break
            cand = sorted(kept + [float(f) * L for f in rng.uniform(lo, hi, size=max(2 * n, 8)) if is_clear(float(f))])
            kept = []
            for s in cand:
                if not kept or s - kept[-1] >= min_gap:
                    kept.append(s)
            while track.closed and len(kept) > 1 and kept[0] + L - kept[-1] < min_gap:
                kept.pop()
            if len(kept) > n:   # an even pick over the sorted candidates keeps every gap
                kept = [kept[i] for i in sorted(rng.choice(len(kept), size=n, replace=False))]
        if len(kept) < n:
            raise ValueError("could not place %d obstacles %g m apart on %g m of track" % (n, min_gap, (hi - lo) * L))
        s = np.array(kept, dtype=np.float64)
        p, tan = track.point_at(s)
        off = rng.uniform(-lateral, lateral, size=n)
        xy = p + off[:, None] * np.column_stack([-tan[:, 1], tan[:, 0]])
        is_disc = rng.uniform(size=n) < disc_fraction
        yaws = np.arctan2(tan[:, 1], tan[:, 0]) + rng.uniform(-0.5 * float(yaw), 0.5 * float(yaw), size=n)
        ln, wd, rd = rng.uniform(*length, size=n), rng.uniform(*width, size=n), rng.uniform(*radius, size=n)
        rows = np.column_stack([np.where(is_disc, float(DISC), float(BOX)), xy[:, 0], xy[:, 1], np.where(is_disc, 1.0, np.cos(yaws)),
                                np.where(is_disc, 0.0, np.sin(yaws)), np.where(is_disc, rd, 0.5 * ln), np.where(is_disc, 0.0, 0.5 * wd)])
        return (cls(rows), s) if return_s else cls(rows)

    def __repr__(self):
        nd = int(np.sum(self._rows[:, 0] == DISC))
        return "Obstacles(%d boxes, %d discs)" % (len(self) - nd, nd)
