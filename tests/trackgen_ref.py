"""NumPy model of the corridor carve (include/f110.h, f110_add_map_corridor) and the fixtures of its tests.

The rule is restated verbatim from the header, on whole arrays: the cell centres by the stamp rule's formula, the capsule test of
every segment on EVERY cell (no culling of any kind), the border ring, res * distance_transform_edt.  A line is (xy [M][2], half
widths [S], closed); a frame is (res, ox, oy, oc, os) as the library holds it."""
import functools

import numpy as np
from scipy.ndimage import distance_transform_edt

from f1tenth_gym_amd import Track, TrackMap
from f1tenth_gym_amd.centerline import curvature_closed, resample_closed

TILE_H, TILE_W = 16, 64   # kCorrTileH, kCorrTileW (f110_math.hpp); the harness reports them too
CAP = 256                 # kCorrCap

# The largest distance of a centreline cell's centre from the generating line, in cells, measured on the model (the figures of
# DESIGN §6o); the test allows each its own figure plus 0.25 cell, the margin tests/test_centerline_host.py uses for such figures.
ROUND_TRIP_CELLS = {"star31": 1.4380, "star57": 1.4197, "star90": 1.7821, "star120": 2.1418, "star160": 1.6022, "star200": 1.6248}


def frame_of(res, origin):
    """(res, ox, oy, oc, os) of a resolution and an origin (x, y, yaw)"""
    return (float(res), float(origin[0]), float(origin[1]), float(np.cos(origin[2])), float(np.sin(origin[2])))


def cell_world(H, W, frame):
    """(wx, wy) [H][W]: the centre of every table cell (row 0 at the bottom) in map coordinates"""
    res, ox, oy, oc, os_ = frame
    c = np.arange(W, dtype=np.float64)[None, :]
    r = np.arange(H, dtype=np.float64)[:, None]
    px = np.broadcast_to((c + 0.5) * res, (H, W))
    py = np.broadcast_to((r + 0.5) * res, (H, W))
    return ox + (px * oc - py * os_), oy + (px * os_ + py * oc)


def segments(xy, closed):
    """(a [S][2], b [S][2])"""
    xy = np.asarray(xy, dtype=np.float64)
    return (xy, np.roll(xy, -1, axis=0)) if closed else (xy[:-1], xy[1:])


def segment_hits(wx, wy, a, b, hw):
    """the rule for one segment on arrays of cell centres"""
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    with np.errstate(over="ignore", invalid="ignore"):
        ux, uy = wx - ax, wy - ay
        dx, dy = bx - ax, by - ay
        t = ux * dx + uy * dy
        L2 = dx * dx + dy * dy
        h2 = hw * hw
        near = ux * ux + uy * uy <= h2
        vx, vy = wx - bx, wy - by
        far = vx * vx + vy * vy <= h2
        cr = ux * dy - uy * dx
        mid = cr * cr <= h2 * L2
        return np.where(t <= 0.0, near, np.where(t >= L2, far, mid))


def ring(H, W):
    m = np.zeros((H, W), dtype=bool)
    m[0, :] = m[H - 1, :] = True
    m[:, 0] = m[:, W - 1] = True
    return m


def corridor_mask(xy, hw, closed, H, W, frame, with_ring=True):
    """bool [H][W]: the carved cells — every segment against every cell"""
    wx, wy = cell_world(H, W, frame)
    a, b = segments(xy, closed)
    m = np.zeros((H, W), dtype=bool)
    for i in range(a.shape[0]):
        m |= segment_hits(wx, wy, a[i], b[i], float(hw[i]))
    if with_ring:
        m &= ~ring(H, W)
    return m


def corridor_table(mask, res):
    """the slot's table of a carved mask: res * EDT to the nearest cell that is not carved"""
    return res * distance_transform_edt(mask)


def image_of(mask):
    """the image a user of the reference would load: carved cells 255, all others 0, top row first"""
    return np.ascontiguousarray(np.flipud(np.where(mask, 255, 0).astype(np.uint8)))


def free_from_image(img_top_first):
    """laser_models.py:398-404: flip, then > 128 is free"""
    return np.flipud(np.asarray(img_top_first)) > 128


def point_segment_distance(px, py, a, b):
    """brute force, with a division and a square root: arrays of points against one segment"""
    ax, ay, bx, by = float(a[0]), float(a[1]), float(b[0]), float(b[1])
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    t = np.zeros_like(px) if L2 == 0.0 else np.clip(((px - ax) * dx + (py - ay) * dy) / L2, 0.0, 1.0)
    ex, ey = px - (ax + t * dx), py - (ay + t * dy)
    return np.sqrt(ex * ex + ey * ey)


def polyline_distance(points, xy, closed=True):
    """[n]: the distance of every point to the polyline, brute force over the segments"""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 2)
    a, b = segments(xy, closed)
    best = np.full(points.shape[0], np.inf)
    for i in range(a.shape[0]):
        best = np.minimum(best, point_segment_distance(points[:, 0], points[:, 1], a[i], b[i]))
    return best


def boundary_margin(xy, hw, closed, H, W, frame):
    """the smallest distance [m] of any cell centre to any capsule's boundary: above 1e-9, no cell's test hangs on the last bits"""
    wx, wy = cell_world(H, W, frame)
    a, b = segments(xy, closed)
    best = np.inf
    for i in range(a.shape[0]):
        if not np.isfinite(hw[i]) or hw[i] > 1e100:
            continue   # (a capsule whose boundary is nowhere near the table)
        best = min(best, float(np.min(np.abs(point_segment_distance(wx, wy, a[i], b[i]) - float(hw[i])))))
    return best


def tile_need(xy, hw, closed, H, W, frame):
    """int [tile rows][tile columns]: how many segments carve at least one cell centre of each tile (ring cells included: they are
    centres of the tile too) — what any culling must keep at the least"""
    wx, wy = cell_world(H, W, frame)
    a, b = segments(xy, closed)
    th, tw = -(-H // TILE_H), -(-W // TILE_W)
    need = np.zeros((th, tw), dtype=np.int64)
    for i in range(a.shape[0]):
        hit = segment_hits(wx, wy, a[i], b[i], float(hw[i]))
        pad = np.zeros((th * TILE_H, tw * TILE_W), dtype=bool)
        pad[:H, :W] = hit
        need += pad.reshape(th, TILE_H, tw, TILE_W).any(axis=(1, 3))
    return need


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
class Fx(object):
    """a line, its half widths and its frame; .tm is the TrackMap of it (None for a line Track refuses, e.g. a repeated point)"""

    def __init__(self, name, xy, hw, closed, H, W, res, origin, inside=True, track_ok=True):
        self.name, self.closed, self.H, self.W, self.res, self.origin = name, bool(closed), int(H), int(W), float(res), tuple(float(v) for v in origin)
        self.xy = np.ascontiguousarray(xy, dtype=np.float64)
        S = self.xy.shape[0] if closed else self.xy.shape[0] - 1
        self.hw = np.full(S, float(hw)) if np.ndim(hw) == 0 else np.ascontiguousarray(hw, dtype=np.float64)
        assert self.hw.shape == (S,)
        self.inside = inside   # the fixture says: the corridor stays inside the ring
        self.frame = frame_of(res, origin)
        self.tm = TrackMap(Track(self.xy, closed=self.closed), self.hw, resolution=res, shape=(H, W), origin=self.origin) if track_ok else None

    @functools.lru_cache(maxsize=None)
    def mask(self):
        m = corridor_mask(self.xy, self.hw, self.closed, self.H, self.W, self.frame)
        m.setflags(write=False)
        return m

    @functools.lru_cache(maxsize=None)
    def table(self):
        t = corridor_table(self.mask(), self.res)
        t.setflags(write=False)
        return t

    def margin(self):
        return boundary_margin(self.xy, self.hw, self.closed, self.H, self.W, self.frame)

    def cell_xy(self, r, c):
        """world coordinates of a point given in (fractional) cell-centre units: (r, c) whole = the centre of cell (r, c)"""
        res, ox, oy, oc, os_ = self.frame
        px, py = (c + 0.5) * res, (r + 0.5) * res
        return (ox + (px * oc - py * os_), oy + (px * os_ + py * oc))


def star_points(n, radius, k, amp, phase, centre):
    """n points of r(phi) = radius * (1 + amp * cos(k phi + phase)) around centre, uniform in arc length, counter-clockwise"""
    phi = 2.0 * np.pi * np.arange(4096, dtype=np.float64) / 4096
    r = radius * (1.0 + amp * np.cos(k * phi + phase))
    pts = np.stack([centre[0] + r * np.cos(phi), centre[1] + r * np.sin(phi)], axis=1)
    L = float(np.sum(np.sqrt(np.sum((np.roll(pts, -1, axis=0) - pts) ** 2, axis=1))))
    q, _, _, _ = resample_closed(pts, np.zeros(4096), L / n)
    return q


def max_kappa(xy):
    return float(np.max(np.abs(curvature_closed(np.asarray(xy, dtype=np.float64)))))


@functools.lru_cache(maxsize=None)
def star_fixtures():
    """six closed star-shaped lines, 31 .. 200 points, on 96 x 130 .. 256 x 320 tables (one frame turned by 0.3): the round-trip
    fixtures.  (name, n, radius [m], k, amp, phase, half width [m], H, W, res, yaw)"""
    rows = [("star31", 31, 1.6, 2, 0.10, 0.3, 0.52, 96, 130, 0.05, 0.0),
            ("star57", 57, 2.3, 3, 0.08, 1.1, 0.47, 128, 150, 0.05, 0.0),
            ("star90", 90, 2.7, 2, 0.18, 2.0, 0.61, 160, 200, 0.05, 0.0),
            ("star120", 120, 3.6, 3, 0.10, 0.7, 0.83, 200, 256, 0.05, 0.3),
            ("star160", 160, 5.2, 4, 0.05, 4.0, 0.72, 256, 320, 0.05, 0.0),
            ("star200", 200, 4.9, 5, 0.04, 5.1, 0.66, 250, 300, 0.05, 0.0)]
    out = []
    for name, n, radius, k, amp, phase, hw, H, W, res, yaw in rows:
        c, s = np.cos(yaw), np.sin(yaw)
        px, py = 0.5 * W * res + 0.013, 0.5 * H * res - 0.017   # the table's middle, a little off the cell grid
        origin = (-1.7, 0.9, yaw)
        centre = (origin[0] + (px * c - py * s), origin[1] + (px * s + py * c))
        out.append(Fx(name, star_points(n, radius, k, amp, phase, centre), hw, True, H, W, res, origin))
    return out


def tight_fixture():
    """the negative fixture of the generator's check: |kappa| * hw = 1.8 where a six-pointed star turns tightest (the inner wall
    folds there; the corridor is still a ring)"""
    res, H, W = 0.05, 280, 280
    xy = star_points(150, 4.0, 6, 0.1, 0.4, (7.0 + 0.011, 7.0 - 0.007))
    hw = 1.8 / max_kappa(xy)
    return Fx("tight", xy, hw, True, H, W, res, (0.0, 0.0, 0.0))


def wound_line(M, centre, pitch, length):
    """M points of a boustrophedon: rows `pitch` apart, `length` long, so that a small region holds hundreds of segments"""
    per = 8
    pts = []
    for i in range(M):
        row, k = divmod(i, per)
        x = (k if row % 2 == 0 else per - 1 - k) * (length / (per - 1))
        pts.append((centre[0] + x, centre[1] + row * pitch))
    return np.array(pts)


def wound_fixture(M):
    """an open line of M points wound inside ONE tile (rows 16 .. 31, columns 64 .. 127 of a 48 x 160 table at 0.05 m): the tile's
    cells lie within 0.8 m x 3.2 m, the line's rows are 0.0111 m apart, so every segment carves cells of that tile"""
    res = 0.05
    fx0 = Fx("w", [(0, 0), (1, 1)], 0.0, False, 48, 160, res, (0.3, -0.2, 0.0))
    x0, y0 = fx0.cell_xy(16.37, 70.21)
    xy = wound_line(M, (x0, y0), 0.6 / max(1, (M + 7) // 8), 2.313)
    return Fx("wound%d" % M, xy, 0.0721, False, 48, 160, res, (0.3, -0.2, 0.0), track_ok=True)


def _line_fx(name, cells, hw, closed, H, W, res=0.05, origin=(-0.4, 0.7, 0.0), inside=True, track_ok=True):
    fx0 = Fx("f", [(0, 0), (1, 1)], 0.0, False, H, W, res, origin)
    return Fx(name, [fx0.cell_xy(r, c) for r, c in cells], hw, closed, H, W, res, origin, inside=inside, track_ok=track_ok)


@functools.lru_cache(maxsize=None)
def edge_fixtures():
    """the smallest shapes where the kernel can go wrong (the issue's edge list); cell coordinates are (row, column), fractional"""
    out = []
    loop = [(8.3, 9.2), (8.6, 40.4), (30.2, 52.7), (36.4, 30.1), (33.7, 8.8)]
    for W in (63, 64, 65, 127, 129):   # widths around the tile's, with a height (45) that is no multiple of the tile's rows
        sx = (W - 12.0) / 55.0
        out.append(_line_fx("w%d" % W, [(r, 4.0 + (c - 8.0) * sx) for r, c in loop], 0.137, True, 45, W))
    out.append(_line_fx("one_segment", [(5.2, 6.3), (20.7, 50.1)], 0.171, False, 30, 70))
    out.append(_line_fx("triangle", [(6.2, 7.3), (9.7, 55.1), (31.4, 28.6)], 0.121, True, 40, 66))
    out.append(_line_fx("repeated_point", [(6.2, 7.3), (20.4, 30.6), (20.4, 30.6), (8.1, 50.2)], 0.153, False, 33, 70, track_ok=False))
    out.append(_line_fx("segment_outside", [(10.3, 8.2), (22.6, 41.7), (300.2, 500.4), (320.8, 520.1)], [0.162, 0.0, 0.162], False, 35, 67, inside=False))
    out.append(_line_fx("crosses_border", [(12.3, -20.4), (14.8, 30.2), (60.7, 33.9)], 0.211, False, 38, 72, inside=False))
    out.append(_line_fx("yaw", [(8.3, 9.2), (8.6, 48.4), (36.4, 50.1), (33.7, 8.8)], 0.143, True, 47, 80, origin=(1.3, -2.1, 0.3)))
    out.append(_line_fx("widths", loop, [0.06, 0.211, 0.0, 0.137, 0.093], True, 45, 70))
    out.append(_line_fx("all_free", [(10.2, 11.3), (20.4, 30.1)], [1e3], False, 37, 90, inside=False))
    for M in (CAP - 1, CAP, CAP + 1, 2 * CAP + 3):
        out.append(wound_fixture(M))
    return out


def fixture(name):
    for fx in list(star_fixtures()) + list(edge_fixtures()):
        if fx.name == name:
            return fx
    raise KeyError(name)


EDGE_NAMES = ["w63", "w64", "w65", "w127", "w129", "one_segment", "triangle", "repeated_point", "segment_outside", "crosses_border", "yaw", "widths",
              "all_free", "wound%d" % (CAP - 1), "wound%d" % CAP, "wound%d" % (CAP + 1), "wound%d" % (2 * CAP + 3)]
STAR_NAMES = ["star31", "star57", "star90", "star120", "star160", "star200"]


def no_carve_line():
    """all widths 0 on a line between cell centres of a 30 x 40 table: nothing is carved"""
    return _line_fx("no_carve", [(5.5, 6.5), (5.5, 30.5), (20.5, 30.5)], 0.0, False, 30, 40)


@functools.lru_cache(maxsize=None)
def inplace_fixtures():
    """three closed lines of 57 points each in ONE frame (star57's): what set_track_map re-carves a slot with"""
    base = fixture("star57")
    centre = base.cell_xy(0.5 * base.H - 0.84, 0.5 * base.W - 0.24)
    out = [base]
    for name, radius, k, amp, phase, hw in (("inplace_b", 2.0, 2, 0.15, 0.9, 0.41), ("inplace_c", 2.2, 4, 0.06, 2.3, 0.55)):
        out.append(Fx(name, star_points(57, radius, k, amp, phase, centre), hw, True, base.H, base.W, base.res, base.origin))
    return out
