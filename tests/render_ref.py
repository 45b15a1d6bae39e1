"""A NumPy statement of the render's class rules (include/f110.h f110_render_device) in float64, with the margin of
every pixel's decision: how far (metres) the deciding quantity is from flipping it.  Device trigonometry (the camera angle of
FOLLOW / EGO views, box corners, the lidar offset) may differ from NumPy's by an ulp, so comparisons skip pixels whose margin
is below MARGIN and require everything else to be equal."""
import numpy as np

MARGIN = 1e-9
VIEWS = {"world": 0, "follow": 1, "ego": 2}
LAYER = {"map": 1, "track": 2, "scan": 4, "cars": 8}


def box_vertices(x, y, th, length, width):
    """get_vertices (collision_models.py:218-260): [4][2], [rl, rr, fr, fl]"""
    c, s = np.cos(th), np.sin(th)
    hx, hy = length / 2, width / 2
    bx, by = np.array([-hx, -hx, hx, hx]), np.array([hy, -hy, -hy, hy])
    return np.stack([((c * bx + (-s) * by) + 0.) + x, ((s * bx + c * by) + 0.) + y], axis=1)


class Scene(object):
    """what a render reads.  poses [N][3] (agent_poses), scans [N][B], lengths / widths [N] (each agent's params),
    maps: list per slot of dict(dt=[H][W], res, origin=(ox, oy, yaw) or oc / os, track=[M][2] or None), env_slot [E] or None,
    fov, theta_dis, max_range, lidar_dist; verts [N][4][2] optional (the device's get_vertices)"""

    def __init__(self, poses, scans, A, maps, lengths, widths, env_slot=None, fov=4.7, theta_dis=2000, max_range=30.0,
                 lidar_dist=0.0, verts=None):
        self.poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
        self.N = self.poses.shape[0]
        self.scans = np.asarray(scans, dtype=np.float64).reshape(self.N, -1)
        self.A = int(A)
        self.maps = maps
        self.lengths, self.widths = np.broadcast_to(lengths, (self.N,)), np.broadcast_to(widths, (self.N,))
        self.env_slot = None if env_slot is None else np.asarray(env_slot)
        self.fov, self.theta_dis, self.max_range, self.lidar_dist = fov, int(theta_dis), max_range, lidar_dist
        self.verts = verts
        theta = np.linspace(0.0, 2 * np.pi, num=self.theta_dis)
        self.sines, self.cosines = np.sin(theta), np.cos(theta)


def _map_fields(m):
    if "oc" in m:
        oc, os_ = m["oc"], m["os"]
    else:
        oc, os_ = np.cos(m["origin"][2]), np.sin(m["origin"][2])
    return m["dt"], float(m["res"]), float(m["origin"][0]), float(m["origin"][1]), oc, os_


def track_points(xy, closed=True):
    xy = np.asarray(xy, dtype=np.float64)
    if closed and xy.shape[0] > 1 and xy[0].tobytes() == xy[-1].tobytes():
        xy = xy[:-1]
    return xy


def scan_points(sc, n):
    """(x, y) of the lidar hits of agent n (range < max_range): the scan pose plus r times the trig-table direction of the
    beam's theta_index (laser_models.py get_scan / trace_ray)"""
    x, y, th = sc.poses[n]
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(th)):
        return np.zeros((0, 2))
    if sc.lidar_dist == 0.0 and abs(th) < 1e300 and not (x == 0.0 and np.signbit(x)) and not (y == 0.0 and np.signbit(y)):
        sx, sy = x, y
    else:
        sx, sy = x + sc.lidar_dist * np.cos(th), y + sc.lidar_dist * np.sin(th)
    B = sc.scans.shape[1]
    inc = sc.theta_dis * (sc.fov / (B - 1)) / (2. * np.pi)
    ti = sc.theta_dis * (th - sc.fov / 2.) / (2. * np.pi)
    ti = np.fmod(ti, sc.theta_dis)
    while ti < 0:
        ti += sc.theta_dis
    idx = np.empty(B, dtype=np.int64)
    for b in range(B):
        idx[b] = min(int(ti), sc.theta_dis - 1)
        ti += inc
        while ti >= sc.theta_dis:
            ti -= sc.theta_dis
    r = sc.scans[n]
    hit = r < sc.max_range
    return np.stack([sx + r[hit] * sc.cosines[idx[hit]], sy + r[hit] * sc.sines[idx[hit]]], axis=1)


def camera(sc, n, view, center=(0.0, 0.0), angle=0.0, fwd_offset=0.0):
    """(cx, cy, c, s, valid)"""
    if view == "world":
        return float(center[0]), float(center[1]), np.cos(angle), np.sin(angle), True
    x, y, th = sc.poses[n]
    cx, cy = x + fwd_offset * np.cos(th), y + fwd_offset * np.sin(th)
    c, s = (1.0, 0.0) if view == "follow" else (np.cos(th - np.pi / 2), np.sin(th - np.pi / 2))
    return cx, cy, c, s, bool(np.isfinite(x) and np.isfinite(y) and np.isfinite(th))


def _edge_frac_margin(q):
    return np.minimum(q - np.floor(q), np.floor(q) + 1.0 - q)


def render_frame(sc, n, width=64, height=64, view="ego", m_per_px=0.05, center=(0.0, 0.0), angle=0.0, fwd_offset=0.0,
                 layers=("map", "cars"), car_size=None, tracks_closed=True):
    """-> (classes [H][W] uint8, margin [H][W] metres) of camera agent n"""
    H, W, mpp = int(height), int(width), float(m_per_px)
    bits = sum(LAYER[k] for k in (LAYER if layers == "all" else layers))
    cls = np.zeros((H, W), dtype=np.uint8)
    margin = np.full((H, W), np.inf)
    cx, cy, c, s, valid = camera(sc, n, view, center, angle, fwd_offset)
    if not valid:
        return cls, margin
    e = n // sc.A
    slot = 0 if sc.env_slot is None else int(sc.env_slot[e])
    i = np.arange(H, dtype=np.float64)[:, None]
    j = np.arange(W, dtype=np.float64)[None, :]
    u = ((j + 0.5) - W * 0.5) * mpp
    v = (H * 0.5 - (i + 0.5)) * mpp
    x = cx + (u * c - v * s)
    y = cy + (u * s + v * c)
    if bits & LAYER["map"]:
        dt, res, ox, oy, oc, os_ = _map_fields(sc.maps[slot])
        mh, mw = dt.shape
        xt, yt = x - ox, y - oy
        xr = xt * oc + yt * os_
        yr = -xt * os_ + yt * oc
        w_res, h_res = mw * res, mh * res
        inside = (xr >= 0) & (xr < w_res) & (yr >= 0) & (yr < h_res)
        margin = np.minimum(margin, np.minimum(np.minimum(np.abs(xr), np.abs(xr - w_res)), np.minimum(np.abs(yr), np.abs(yr - h_res))))
        col = np.clip(np.where(inside, xr / res, 0).astype(np.int64), 0, mw - 1)
        row = np.clip(np.where(inside, yr / res, 0).astype(np.int64), 0, mh - 1)
        cell_m = np.minimum(_edge_frac_margin(xr / res), _edge_frac_margin(yr / res)) * res
        margin = np.where(inside, np.minimum(margin, cell_m), margin)
        cls[...] = np.where(inside, np.where(dt[row, col] == 0.0, 2, 1), 0)
    else:
        cls[...] = 1
    if bits & LAYER["cars"]:
        for a in range(sc.A):
            m = e * sc.A + a
            px, py, pth = sc.poses[m]
            if not (np.isfinite(px) and np.isfinite(py) and np.isfinite(pth)):
                continue
            if sc.verts is not None and car_size is None:
                vtx = np.asarray(sc.verts[m]).reshape(4, 2)
            else:
                L, Wd = (car_size if car_size is not None else (sc.lengths[m], sc.widths[m]))
                vtx = box_vertices(px, py, pth, L, Wd)
            crs, dist = [], []
            for q in range(4):
                ax, ay = vtx[q]
                bx, by = vtx[(q + 1) % 4]
                cr = (bx - ax) * (y - ay) - (by - ay) * (x - ax)
                crs.append(cr >= 0.0)
                dist.append(cr / np.hypot(bx - ax, by - ay))
            inside = crs[0] & crs[1] & crs[2] & crs[3]
            d = np.stack(dist)
            m_in = np.min(d, axis=0)
            m_out = np.max(np.where(d < 0, -d, 0.0), axis=0)
            margin = np.minimum(margin, np.where(inside, m_in, m_out))
            k = 6 if m == n else 5
            cls = np.where(inside & (cls < k), k, cls).astype(np.uint8)

    def points(pts, k):
        nonlocal cls, margin
        if len(pts) == 0:
            return
        dx, dy = pts[:, 0] - cx, pts[:, 1] - cy
        up, vp = dx * c + dy * s, -dx * s + dy * c
        qi, qj = H * 0.5 - vp / mpp, up / mpp + W * 0.5
        fi, fj = np.floor(qi), np.floor(qj)
        pm = np.minimum(_edge_frac_margin(qi), _edge_frac_margin(qj)) * mpp
        ok = np.isfinite(fi) & np.isfinite(fj)
        for a, b, pmar in zip(fi[ok], fj[ok], pm[ok]):
            a, b = int(a), int(b)
            if pmar < MARGIN:   # the point may land in a neighbour: both sides are undecided
                margin[max(a - 1, 0):max(a + 2, 0), max(b - 1, 0):max(b + 2, 0)] = 0.0
            if 0 <= a < H and 0 <= b < W and cls[a, b] < k:
                cls[a, b] = k

    if bits & LAYER["track"]:
        t = sc.maps[slot].get("track")
        if t is not None:
            points(track_points(t, tracks_closed), 3)
    if bits & LAYER["scan"]:
        points(scan_points(sc, n), 4)
    return cls, margin


def render(sc, agents, **spec):
    """-> (classes [F][H][W], margin [F][H][W])"""
    out = [render_frame(sc, int(n), **spec) for n in agents]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def compare(got, want, margin, max_share=1e-3, what=""):
    """every pixel with margin >= MARGIN equal; the excluded share <= max_share"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    decided = margin >= MARGIN
    share = 1.0 - decided.mean()
    assert share <= max_share, "%s: %.4f%% of the pixels are undecided" % (what, 100 * share)
    bad = decided & (got != want)
    if bad.any():
        idx = np.argwhere(bad)[:5]
        raise AssertionError("%s: %d pixels differ, e.g. %s: got %s want %s" % (
            what, int(bad.sum()), idx.tolist(), [int(got[tuple(q)]) for q in idx], [int(want[tuple(q)]) for q in idx]))
