"""Track generation — random closed lines, and the raster frame a line is carved into (f110_add_map_corridor).

Not a reference type: the reference's generator draws a track into an image with cv2, shapely and matplotlib, and the image is
loaded like any map.  Here a line (a Track) plus a half width per segment IS the map: the library carves the corridor into a slot's
distance table on the device (BatchSim.add_track_map / set_track_map).  Everything in this module is NumPy on a few hundred points.

TrackMap holds a line and its frame; it is immutable.  random_track draws a line, float64, deterministic per seed, in these steps:

1. The draw.  rng = np.random.default_rng(seed), once per call.  A try draws a = rng.uniform(-amplitude, amplitude, harmonics) and
   then p = rng.uniform(0, 2 pi, harmonics), in this order; try n + 1 continues the same stream.
2. The star-shaped line.  At phi_i = 2 pi i / 2048, i = 0 .. 2047:
       r(phi) = radius * (1 + sum_k a_k / (k - 1) * cos(k * phi + p_k)),  k = 2 .. harmonics + 1   (a_k, p_k the draws in order)
   and the points (r cos phi, r sin phi): counter-clockwise, since phi grows.  A try with min r <= 0 is rejected.
3. Resampling, uniform in arc length: centerline.resample_closed at `spacing` (M = max(3, floor(L / spacing + 0.5)) stations; more
   than 16384 stations are refused: raise spacing).
4. kappa: centerline.curvature_closed of the resampled points.
5. Acceptance.  With D = 2 * half_width + wall_gap a try is rejected when
       max |kappa| * half_width >= tightness               (the corridor's inner wall would fold), or
       two stations more than D of arc apart (the shorter way round) are closer than D   (two arms would merge).
6. The first accepted try is returned as a closed Track with the attribute columns ('half_width', 'kappa'), half_width constant;
   after max_tries rejections ValueError.
"""
import numpy as np

from .centerline import curvature_closed, resample_closed
from .track import Track

MAX_CORRIDOR_POINTS = 65536   # F110_MAX_CORRIDOR_POINTS
MAX_SIDE = 16384              # cells, as f110_add_map_image asks
STAR_SAMPLES = 2048
MAX_STATIONS = 16384           # random_track's own limit: its pairwise test is quadratic in the stations


def _frozen(a):
    a = np.array(a, dtype=np.float64, copy=True)
    a.setflags(write=False)
    return a


class TrackMap(object):
    """a line (Track) with one half width per segment and the raster frame it is carved into: `shape` (H, W) cells of `resolution`
    metres, `origin` (x, y, yaw) the map position of the corner of cell (0, 0).

    half_width: a number, an [S] array (S = the track's segments) or None = the track's 'half_width' attribute column averaged over
    each segment's two ends.  The default frame has yaw 0 and is the line's bounding box grown by the largest half width plus
    `margin` on every side, rounded up to whole cells; `origin` and / or `shape` replace it (a shape alone is measured from the
    default origin, an origin alone gets the shape that covers the grown box in its frame)."""
    __slots__ = ("track", "resolution", "margin", "_hw", "_shape", "_origin")

    def __init__(self, track, half_width=None, resolution=0.0625, margin=1.0, shape=None, origin=None):
        track = Track.coerce(track)
        S, M = track.num_segments, track.num_points
        if M > MAX_CORRIDOR_POINTS:
            raise ValueError("a corridor takes at most %d points, got %d" % (MAX_CORRIDOR_POINTS, M))
        if half_width is None:
            names = track.attr_names or ()
            if 'half_width' not in names:
                raise ValueError("half_width=None needs a track with a 'half_width' attribute column")
            col = track.attrs[:, names.index('half_width')]
            nxt = np.roll(col, -1) if track.closed else col[1:]
            hw = 0.5 * (col[:S] + nxt[:S])
        else:
            hw = np.asarray(half_width, dtype=np.float64)
            if hw.ndim == 0:
                hw = np.full(S, float(hw))
            elif hw.shape != (S,):
                raise ValueError("half_width must be a number or one per segment (%d), got shape %s" % (S, hw.shape))
        if not np.all(np.isfinite(hw)) or np.any(hw < 0.0):
            raise ValueError("half widths must be finite and >= 0")
        res, margin = float(resolution), float(margin)
        if not (np.isfinite(res) and res > 0.0):
            raise ValueError("resolution must be finite and > 0, got %r" % (resolution,))
        if not (np.isfinite(margin) and margin >= 0.0):
            raise ValueError("margin must be finite and >= 0, got %r" % (margin,))
        grow = float(hw.max()) + margin
        xy = track.xy
        if origin is None:
            org = (float(xy[:, 0].min()) - grow, float(xy[:, 1].min()) - grow, 0.0)
        else:
            org = tuple(float(v) for v in origin)
            if len(org) != 3 or not np.all(np.isfinite(org)):
                raise ValueError("origin must be three finite numbers (x, y, yaw), got %r" % (origin,))
        if shape is None:
            c, s = np.cos(org[2]), np.sin(org[2])
            xt, yt = xy[:, 0] - org[0], xy[:, 1] - org[1]
            xr, yr = xt * c + yt * s, -xt * s + yt * c      # the line in the frame's axes (the centreline rule's inverse transform)
            shp = (int(np.ceil((float(yr.max()) + grow) / res)), int(np.ceil((float(xr.max()) + grow) / res)))
        else:
            shp = tuple(shape)
            if len(shp) != 2 or any(int(v) != v for v in shp):
                raise ValueError("shape must be two whole numbers (H, W), got %r" % (shape,))
            shp = (int(shp[0]), int(shp[1]))
        if not (1 <= shp[0] <= MAX_SIDE and 1 <= shp[1] <= MAX_SIDE):
            raise ValueError("a frame has 1 .. %d cells a side, got %r" % (MAX_SIDE, shp))
        set_ = object.__setattr__
        set_(self, "track", track)
        set_(self, "resolution", res)
        set_(self, "margin", margin)
        set_(self, "_hw", _frozen(hw))
        set_(self, "_shape", shp)
        set_(self, "_origin", org)

    def __setattr__(self, name, value):
        raise AttributeError("a TrackMap is immutable")

    def __delattr__(self, name):
        raise AttributeError("a TrackMap is immutable")

    @classmethod
    def coerce(cls, tm):
        """a TrackMap, a Track (its 'half_width' column, the default frame) or a dict of random_track's keyword arguments"""
        if isinstance(tm, TrackMap):
            return tm
        if isinstance(tm, dict):
            return cls(random_track(**tm))
        return cls(tm)

    @property
    def shape(self):
        return self._shape

    @property
    def origin(self):
        return self._origin

    def widths(self):
        """the half width per segment, [S] (read-only)"""
        return self._hw

    def points(self):
        """the line's points, [M][2] float64, contiguous"""
        return np.ascontiguousarray(self.track.xy, dtype=np.float64)

    def carved_line(self):
        """the closed line as a Track whose 'half_width' column is what was CARVED around each point: the smaller half width of the
        point's two segments (the track's own column, if it has one, plays no part: `half_width=` may have overridden it, and a
        varying column is carved at each segment's mean).  What a raceline on the carved slot is solved from."""
        if not self.track.closed:
            raise ValueError("a carved line with half widths per point needs a closed track")
        hw = np.asarray(self._hw)
        return Track(self.track.xy, closed=True, attrs={'half_width': np.minimum(hw, np.roll(hw, 1))})

    def same_frame(self, other):
        return (isinstance(other, TrackMap) and self._shape == other._shape and self.resolution == other.resolution
                and self._origin == other._origin)

    def frame(self):
        """(res, ox, oy, oc, os) as the library holds them for this map (f110_slot_frame)"""
        return (self.resolution, self._origin[0], self._origin[1], float(np.cos(self._origin[2])), float(np.sin(self._origin[2])))

    def __repr__(self):
        return "TrackMap(%r, %d x %d cells of %g m at %r)" % (self.track, self._shape[0], self._shape[1], self.resolution, self._origin)


def star_line(a, p, radius):
    """step 2: the amplitudes and phases of the harmonics k = 2 .. -> (points [2048][2], min r)"""
    phi = 2.0 * np.pi * np.arange(STAR_SAMPLES, dtype=np.float64) / STAR_SAMPLES
    rel = np.ones(STAR_SAMPLES)
    for j in range(len(a)):
        k = j + 2
        rel = rel + (float(a[j]) / (k - 1)) * np.cos(k * phi + float(p[j]))
    r = float(radius) * rel
    return np.stack([r * np.cos(phi), r * np.sin(phi)], axis=1), float(r.min())


def acceptance(q, kappa, half_width, wall_gap):
    """step 5's two figures of a resampled closed line: (max |kappa| * half_width, the smallest distance between two stations more
    than D = 2 * half_width + wall_gap of arc apart — inf when there are none)"""
    D = 2.0 * float(half_width) + float(wall_gap)
    d = np.roll(q, -1, axis=0) - q
    ln = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    s = np.concatenate([[0.0], np.cumsum(ln)[:-1]])
    L = float(ln.sum())
    near = float('inf')
    for i0 in range(0, q.shape[0], 512):      # 512 stations against all at a time: memory stays at 512 x M
        rows = slice(i0, i0 + 512)
        gap = np.abs(s[rows, None] - s[None, :])
        far = np.minimum(gap, L - gap) > D
        if far.any():
            ex, ey = q[rows, 0][:, None] - q[None, :, 0], q[rows, 1][:, None] - q[None, :, 1]
            near = min(near, float(np.sqrt(ex * ex + ey * ey)[far].min()))
    return float(np.max(np.abs(kappa)) * float(half_width)), near


def random_track(seed, radius=8.0, half_width=1.0, harmonics=4, amplitude=0.3, spacing=0.2, tightness=0.9, wall_gap=0.5, max_tries=64):
    """a random closed star-shaped line as a Track (counter-clockwise, attribute columns 'half_width' and 'kappa'), deterministic per
    seed: the steps at the top of this module"""
    harmonics, max_tries = int(harmonics), int(max_tries)
    for name, v in (("radius", radius), ("spacing", spacing), ("tightness", tightness)):
        if not (np.isfinite(v) and v > 0.0):
            raise ValueError("random_track: %s must be finite and > 0, got %r" % (name, v))
    for name, v in (("half_width", half_width), ("amplitude", amplitude), ("wall_gap", wall_gap)):
        if not (np.isfinite(v) and v >= 0.0):
            raise ValueError("random_track: %s must be finite and >= 0, got %r" % (name, v))
    if harmonics < 0 or max_tries < 1:
        raise ValueError("random_track: harmonics must be >= 0 and max_tries >= 1")
    rng = np.random.default_rng(seed)
    D = 2.0 * float(half_width) + float(wall_gap)
    for _ in range(max_tries):
        a = rng.uniform(-float(amplitude), float(amplitude), harmonics)
        p = rng.uniform(0.0, 2.0 * np.pi, harmonics)
        pts, rmin = star_line(a, p, radius)
        if not rmin > 0.0:
            continue
        q, _, _, _ = resample_closed(pts, np.zeros(pts.shape[0]), spacing)
        if q.shape[0] > MAX_STATIONS:
            raise ValueError("random_track: %d stations, at most %d are drawn (raise spacing)" % (q.shape[0], MAX_STATIONS))
        kappa = curvature_closed(q)
        tight, near = acceptance(q, kappa, half_width, wall_gap)
        if tight >= float(tightness) or near < D:
            continue
        return Track(q, closed=True, attrs={'half_width': np.full(q.shape[0], float(half_width)), 'kappa': kappa})
    raise ValueError("random_track: no acceptable line in %d tries (seed %r): lower amplitude or half_width, or raise radius or tightness" % (max_tries, seed))
