"""Centreline — from the loop of table cells f110_map_centerline extracts on the device to a Track.

The device does the heavy part (thinning millions of cells); what is left is a few thousand points, and all of it is NumPy in
float64, deterministic, in exactly these steps (tests/centerline_ref.py restates them):

1. World points.  Cell (r, c) -> its centre by the stamp rule's formula (include/f110.h), with the slot's resolution res, origin
   (ox, oy) and origin cosine / sine (oc, os) as the library holds them (f110_slot_frame):
       px = (c + 0.5) * res, py = (r + 0.5) * res;  wx = ox + (px * oc - py * os), wy = oy + (px * os + py * oc)
2. Smoothing.  A periodic moving average over `smooth` metres of arc: with L0 the length of the closed polyline through the n
   points and m = floor(0.5 * smooth * n / L0 + 0.5) points to either side (at most (n - 1) // 2), point i becomes the mean of
   points i - m .. i + m (indices modulo n), the 2 m + 1 terms added in that order, then divided.  smooth = 0 changes nothing.
3. Resampling.  With L the length of the smoothed closed polyline and cum its running sum (Track's), M = max(3, floor(L / spacing
   + 0.5)) stations s_j = j * (L / M): station j lies on segment k = the last with cum[k] <= s_j at t = (s_j - cum[k]) / len_k,
   and is p_k + t * (p_{k+1} - p_k).  Uniform in the arc length of the smoothed line; the closing segment is one more L / M.
4. half_width.  The gathered table values (T at the cell: the distance to the nearest wall), NOT smoothed, interpolated at the
   same (k, t): w_k + t * (w_{k+1} - w_k).
5. kappa.  The signed curvature of the circle through the resampled points a = q_{j-1}, b = q_j, c = q_{j+1} (indices modulo M):
       2 * ((bx - ax) * (cy - by) - (by - ay) * (cx - bx)) / (|b - a| * |c - b| * |c - a|),   positive to the left.
The Track is closed and carries the attribute columns ('half_width', 'kappa').
"""
import numpy as np

from .track import Track

DEFAULTS = dict(seed=(0.0, 0.0), heading=None, spacing=0.2, smooth=1.0, max_passes=None)


def cell_centres(cells, frame):
    """step 1: cells int [n][2] (r, c), frame = (res, ox, oy, oc, os) -> world points [n][2]"""
    res, ox, oy, oc, os_ = (float(v) for v in frame)
    cells = np.asarray(cells)
    px = (cells[:, 1].astype(np.float64) + 0.5) * res
    py = (cells[:, 0].astype(np.float64) + 0.5) * res
    return np.stack([ox + (px * oc - py * os_), oy + (px * os_ + py * oc)], axis=1)


def _closed_lengths(p):
    d = np.roll(p, -1, axis=0) - p
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])


def _running(v):
    """(cum [n] with cum[0] = 0, total): the running float64 sum in order, as Track builds it"""
    cum = np.empty(v.shape[0])
    acc = 0.0
    for k, x in enumerate(v):
        cum[k] = acc
        acc += float(x)
    return cum, acc


def smooth_closed(p, smooth):
    """step 2"""
    n = p.shape[0]
    _, L0 = _running(_closed_lengths(p))
    m = min(int(np.floor(0.5 * float(smooth) * n / L0 + 0.5)), (n - 1) // 2)
    if m <= 0:
        return p.copy(), 0
    acc = np.zeros_like(p)
    for o in range(-m, m + 1):
        acc = acc + np.roll(p, -o, axis=0)   # row i of roll(p, -o) is p[i + o]
    return acc / float(2 * m + 1), m


def resample_closed(p, values, spacing):
    """steps 3 and 4 -> (points [M][2], values [M], stations [M], L)"""
    ln = _closed_lengths(p)
    cum, L = _running(ln)
    M = max(3, int(np.floor(L / float(spacing) + 0.5)))
    s = np.arange(M, dtype=np.float64) * (L / M)
    k = np.clip(np.searchsorted(cum, s, side='right') - 1, 0, p.shape[0] - 1)
    t = (s - cum[k]) / ln[k]
    k1 = np.where(k + 1 == p.shape[0], 0, k + 1)
    q = p[k] + t[:, None] * (p[k1] - p[k])
    v = values[k] + t * (values[k1] - values[k])
    return q, v, s, L


def curvature_closed(q):
    """step 5"""
    a, c = np.roll(q, 1, axis=0), np.roll(q, -1, axis=0)
    ab, bc, ac = q - a, c - q, c - a
    cross = ab[:, 0] * bc[:, 1] - ab[:, 1] * bc[:, 0]
    den = np.sqrt(ab[:, 0] * ab[:, 0] + ab[:, 1] * ab[:, 1]) * np.sqrt(bc[:, 0] * bc[:, 0] + bc[:, 1] * bc[:, 1]) * np.sqrt(ac[:, 0] * ac[:, 0] + ac[:, 1] * ac[:, 1])
    return 2.0 * cross / den


def track_from_cells(cells, half_width, frame, spacing=0.2, smooth=1.0, details=False):
    """the steps above: ordered loop cells [n][2] and T at each -> Track (and, asked for, a dict of the intermediate arrays)"""
    if not (float(spacing) > 0.0 and np.isfinite(spacing)):
        raise ValueError("centerline: spacing must be finite and > 0, got %r" % (spacing,))
    if not (float(smooth) >= 0.0 and np.isfinite(smooth)):
        raise ValueError("centerline: smooth must be finite and >= 0, got %r" % (smooth,))
    cells = np.asarray(cells, dtype=np.int32).reshape(-1, 2)
    hw = np.asarray(half_width, dtype=np.float64).reshape(-1)
    if cells.shape[0] < 3 or hw.shape[0] != cells.shape[0]:
        raise ValueError("centerline: a loop needs at least 3 cells and one half width per cell")
    raw = cell_centres(cells, frame)
    sm, m = smooth_closed(raw, smooth)
    q, w, s, L = resample_closed(sm, hw, spacing)
    track = Track(q, closed=True, attrs={'half_width': w, 'kappa': curvature_closed(q)})
    if details:
        return track, dict(raw=raw, smoothed=sm, window=m, stations=s, length=L)
    return track


def coerce_params(centerline):
    """the centerline=dict(...) of the env layers -> the keyword arguments of BatchSim.centerline"""
    kw = dict(DEFAULTS)
    if centerline:
        bad = sorted(set(centerline) - set(kw))
        if bad:
            raise ValueError("centerline: unknown parameter(s) %s (known: %s)" % (", ".join(bad), ", ".join(sorted(kw))))
        kw.update(centerline)
    return kw
