"""The model of the track preview (include/f110.h, f110_track_preview): plain NumPy / Python float64, one IEEE
operation per step in the order the header states, a loop per row and per station.  The segment of a station comes from a
bisection over a Python list (the last segment with cum[k] <= s_j, 0 when there is none, 0 for a NaN), not from np.searchsorted.
Shared by the CPU tests (tests/test_track_preview_host.py) and the GPU tests (tests/test_gpu_track_preview.py)."""
import bisect
import os

import numpy as np

from _util import MAPS

CHANNELS = ("x", "y", "tan_x", "tan_y", "attr0", "attr1", "attr2", "attr3")
EPS = 2.0 ** -52
GRID_P = (1, 5, 16, 32)


def settings(**kw):
    s = dict(points=8, offset=0.5, spacing=0.5, channels=("x", "y"), frame="ego", scale={})
    s.update(kw)
    return s


class Tables(object):
    """a track the way f110_track_set stores it: points [M][2] (a closed track's repeated last point dropped), attributes
    [M][C] or None -> ax, ay, dx, dy, len, cum, L in float64, the running sum in order"""

    def __init__(self, xy, closed=True, attrs=None):
        xy = np.array(xy, dtype=np.float64)
        attrs = None if attrs is None else np.array(attrs, dtype=np.float64).reshape(xy.shape[0], -1)
        if closed and xy[-1].tobytes() == xy[0].tobytes():
            xy = xy[:-1]
            attrs = None if attrs is None else attrs[:-1]
        self.xy, self.closed, self.attrs = xy, bool(closed), attrs
        m = xy.shape[0]
        self.npts = m
        self.nseg = m if closed else m - 1
        self.ax, self.ay, self.dx, self.dy, self.len, self.cum = ([0.0] * self.nseg for _ in range(6))
        acc = 0.0
        for k in range(self.nseg):
            k1 = 0 if k + 1 == m else k + 1
            ax, ay = float(xy[k, 0]), float(xy[k, 1])
            dx, dy = float(xy[k1, 0]) - ax, float(xy[k1, 1]) - ay
            ln = float(np.sqrt(np.float64(dx * dx + dy * dy)))
            self.ax[k], self.ay[k], self.dx[k], self.dy[k], self.len[k], self.cum[k] = ax, ay, dx, dy, ln, acc
            acc = acc + ln
        self.L = acc
        self.C = 0 if attrs is None else attrs.shape[1]


def segment_of(tab, sj):
    if sj != sj:
        return 0
    k = bisect.bisect_right(tab.cum, sj) - 1
    return k if k > 0 else 0


def clip01(t):
    """np.clip(t, 0, 1): NaN passes"""
    return 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)


def preview(tab, s, poses, arc):
    """poses [m][3], arc [m] -> (out float32 [m][P][D], raw float64 [m][P][8], seg int32 [m][P])"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    arc = np.asarray(arc, dtype=np.float64).reshape(-1)
    P = int(s["points"])
    bits = [b for b, c in enumerate(CHANNELS) if c in s["channels"]]
    scale = [float(s["scale"].get(CHANNELS[b], 1.0)) for b in range(8)]
    offset, spacing = float(s["offset"]), float(s["spacing"])
    m = poses.shape[0]
    out = np.zeros((m, P, len(bits)), dtype=np.float32)
    raw = np.zeros((m, P, 8))
    seg = np.zeros((m, P), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for r in range(m):
            px, py, th = (float(v) for v in poses[r])
            c, sn = float(np.cos(np.float64(th))), float(np.sin(np.float64(th)))
            for j in range(P):
                d = offset + float(j) * spacing
                sj = float(arc[r]) + d
                if tab.closed and sj >= tab.L:
                    sj = sj - tab.L
                k = segment_of(tab, sj)
                ln = tab.len[k]
                t = clip01((sj - tab.cum[k]) / ln)
                X, Y = tab.ax[k] + t * tab.dx[k], tab.ay[k] + t * tab.dy[k]
                ux, uy = tab.dx[k] / ln, tab.dy[k] / ln
                v = [0.0] * 8
                if s["frame"] == "world":
                    v[:4] = X, Y, ux, uy
                else:
                    rx, ry = X - px, Y - py
                    v[:4] = c * rx + sn * ry, c * ry - sn * rx, c * ux + sn * uy, c * uy - sn * ux
                k1 = 0 if k + 1 == tab.npts else k + 1
                for q in range(tab.C):
                    a0, a1 = float(tab.attrs[k, q]), float(tab.attrs[k1, q])
                    v[4 + q] = a0 + t * (a1 - a0)
                raw[r, j] = v
                seg[r, j] = k
                out[r, j] = [np.float32(np.float64(v[b]) / np.float64(scale[b])) for b in bits]
    return out, raw, seg


def ego_offsets(tab, s, poses, arc, seg):
    """|rx| + |ry| per station [m][P], the size the EGO position channels' bound scales with"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    w = dict(s, frame="world")
    _, raw, _ = preview(tab, w, poses, arc)
    return np.abs(raw[..., 0] - poses[:, None, 0]) + np.abs(raw[..., 1] - poses[:, None, 1])


# ---- the comparison the issue states ------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def f32_steps(a, b):
    """how many float32 values apart two float32 arrays are, element by element (0 = the same value; NaN against NaN 0)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def compare(tab, s, poses, arc, got, what=""):
    """got = (out, raw, seg) of the code under test against the model: WORLD bit for bit; EGO: segments and attribute channels
    bit for bit, |raw - model| <= 8 eps (|rx| + |ry|) for the position channels and 8 eps for the tangent channels, every float32
    output the model's or its float32 neighbour, at most 1 in 1000 different at all.  -> how many float32 values differed"""
    want = preview(tab, s, poses, arc)
    out, raw, seg = got
    assert np.array_equal(seg, want[2]), "%s: segments differ" % what
    if s["frame"] == "world":
        assert np.array_equal(bits(raw), bits(want[1])), "%s: WORLD raw values differ" % what
        assert np.array_equal(bits(out), bits(want[0])), "%s: WORLD outputs differ" % what
        return 0
    assert np.array_equal(bits(raw[..., 4:]), bits(want[1][..., 4:])), "%s: attribute channels differ" % what
    size = ego_offsets(tab, s, poses, arc, seg)
    with np.errstate(invalid="ignore"):
        err = np.abs(raw[..., :4] - want[1][..., :4])
        same_nan = np.isnan(raw[..., :4]) & np.isnan(want[1][..., :4])
        bound = np.stack([8 * EPS * size, 8 * EPS * size, np.full(size.shape, 8 * EPS), np.full(size.shape, 8 * EPS)], axis=-1)
        ok = same_nan | (err <= bound)
    assert np.all(ok), "%s: EGO raw values beyond the bound: worst excess %r" % (what, float(np.nanmax(np.where(ok, 0.0, err - bound))))
    steps = f32_steps(out, want[0])
    assert steps.max(initial=0) <= 1, "%s: a float32 output is %d values away from the model's" % (what, int(steps.max()))
    differ = int(np.count_nonzero(steps))
    assert differ * 1000 <= out.size, "%s: %d of %d float32 outputs differ from the model's" % (what, differ, out.size)
    return differ


# ---- tracks and poses -----------------------------------------------------------------------------------------------------------------
def unit_square(closed=True, attrs=1):
    """(0,0) (1,0) (1,1) (0,1): cum = 0, 1, 2, 3 and, closed, L = 4; attribute q of point k is 10 (q + 1) + k"""
    xy = np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]])
    a = None if attrs == 0 else np.array([[10.0 * (q + 1) + k for q in range(attrs)] for k in range(4)])
    return Tables(xy, closed, a), xy, a


def example_raceline(closed=True, attrs=4):
    """the example raceline (782 segments closed): attributes kappa, vx, cos psi, sin psi"""
    w = np.loadtxt(os.path.join(MAPS, "example_waypoints.csv"), delimiter=';', skiprows=3)
    a = np.column_stack([w[:, 4], w[:, 5], np.cos(w[:, 3]), np.sin(w[:, 3])])[:, :attrs] if attrs else None
    xy = w[:, 1:3]
    if not closed:        # an open track keeps every row; drop the repeated last one so that no segment has zero length
        xy, a = xy[:-1], (None if a is None else a[:-1])
    return Tables(xy, closed, a), xy, a


def circle(n=1500, radius=30.0, closed=True, attrs=1):
    """n points on a circle (n segments closed, n - 1 open).  The kernel stages `cum` of a track of at most STAGED_SEGS segments
    in LDS: the 1500 segments of the default are staged (they are more than the projection kernel stages, 1024)"""
    ang = 2.0 * np.pi * np.arange(n) / n
    xy = np.column_stack([radius * np.cos(ang) + 3.0, radius * np.sin(ang) - 2.0])
    a = None if attrs == 0 else np.column_stack([np.sin(3.0 * ang), 2.0 + np.cos(ang), ang * 0.0 + 1.5, np.cos(5.0 * ang)])[:, :attrs]
    return Tables(xy, closed, a), xy, a


STAGED_SEGS = 2048    # kPreviewLdsSegs (f110_kernels.hpp): a longer track's `cum` is probed in L2


def circle_2048(closed=True, attrs=1):
    """2048 segments, closed or open: the longest track whose `cum` is staged"""
    return circle(2048 if closed else 2049, closed=closed, attrs=attrs)


def circle_2049(closed=True, attrs=1):
    """2049 segments, closed or open: the shortest track whose `cum` is not staged"""
    return circle(2049 if closed else 2050, closed=closed, attrs=attrs)


def poses_near(tab, rng, m, spread=0.4):
    """m random poses near the track and their arc lengths by a float64 projection (first minimum), as Track.project does"""
    k = rng.integers(0, tab.nseg, size=m)
    t = rng.random(m)
    ax, ay, dx, dy = (np.array(v) for v in (tab.ax, tab.ay, tab.dx, tab.dy))
    x = ax[k] + t * dx[k] + rng.uniform(-spread, spread, m)
    y = ay[k] + t * dy[k] + rng.uniform(-spread, spread, m)
    th = np.arctan2(dy[k], dx[k]) + rng.uniform(-0.6, 0.6, m)
    poses = np.column_stack([x, y, th])
    return poses, project_s(tab, poses)


def project_s(tab, poses):
    ax, ay, dx, dy, ln, cum = (np.array(v) for v in (tab.ax, tab.ay, tab.dx, tab.dy, tab.len, tab.cum))
    l2 = dx * dx + dy * dy
    s = np.empty(len(poses))
    for r, (px, py, _) in enumerate(poses):
        t = np.clip(((px - ax) * dx + (py - ay) * dy) / l2, 0.0, 1.0)
        rx, ry = px - (ax + t * dx), py - (ay + t * dy)
        k = int(np.argmin(np.sqrt(rx * rx + ry * ry)))
        s[r] = cum[k] + t[k] * ln[k]
    return s


def unit_grid():
    """(name, track builder, closed, attrs, P, frame, channels) of the CPU / unit-form grid"""
    chans = {0: ("x", "y", "tan_x", "tan_y"), 1: ("x", "y", "tan_x", "tan_y", "attr0"), 4: CHANNELS}
    out = []
    for name, make in (("square", unit_square), ("raceline", example_raceline), ("circle", circle)):
        for ci, closed in enumerate((True, False)):
            for ai, attrs in enumerate((0, 1, 4)):
                for pi, P in enumerate(GRID_P):
                    if (ci + ai + pi) % 2 and name != "square":     # half the grid on the long tracks: the model is a Python loop
                        continue
                    for frame in ("world", "ego"):
                        out.append((name, make, closed, attrs, P, frame, chans[attrs]))
    # either side of the staging boundary (appended: the cases above keep their place in the tests' random streams)
    for name, make in (("circle_2048", circle_2048), ("circle_2049", circle_2049)):
        for closed in (True, False):
            for attrs in (0, 4):
                for P in (1, 32):
                    for frame in ("world", "ego"):
                        out.append((name, make, closed, attrs, P, frame, chans[attrs]))
    return out


def grid_settings(name, tab, P, frame, channels, k):
    """a preview that fits the track: the square is 4 m (closed) long"""
    if name == "square":
        spacing = 0.5 if P <= 5 else 3.4 / P
        s = settings(points=P, offset=0.25 * (k % 2), spacing=spacing, channels=channels, frame=frame)
    else:
        s = settings(points=P, offset=(0.0, 0.5, 1.3)[k % 3], spacing=(0.5, 0.31, 1.7)[k % 3], channels=channels, frame=frame)
    if k % 2:
        s["scale"] = {"x": 10.0, "y": -4.0, "tan_x": 0.5, "attr0": 3.0, "attr3": 7.0}
    return s
