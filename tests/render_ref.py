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
                 layers=("map", "cars"), car_size=None, tracks_closed=True, map_slip=None):
    """-> (classes [H][W] uint8, margin [H][W] metres) of camera agent n.  map_slip ('col', 'row' or 'swap') reads the table
    one column on, one row on, or transposed: the wrong renders a fixture has to tell from the right one"""
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
        if map_slip == "col":
            col = np.minimum(col + 1, mw - 1)
        elif map_slip == "row":
            row = np.minimum(row + 1, mh - 1)
        elif map_slip == "swap":
            row, col = np.minimum(col, mh - 1), np.minimum(row, mw - 1)
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
        mi, mj = _edge_frac_margin(qi) * mpp, _edge_frac_margin(qj) * mpp
        ok = np.isfinite(fi) & np.isfinite(fj)
        for a, b, ma, mb in zip(fi[ok], fj[ok], mi[ok], mj[ok]):
            a, b = int(a), int(b)
            if ma < MARGIN or mb < MARGIN:
                # the point may land in a neighbour along the axis it is on an edge of: both sides are undecided, except
                # pixels that already hold a class the point cannot overwrite (they are the same wherever it lands)
                da, db = (1 if ma < MARGIN else 0), (1 if mb < MARGIN else 0)
                ra, rb = slice(max(a - da, 0), max(a + da + 1, 0)), slice(max(b - db, 0), max(b + db + 1, 0))
                margin[ra, rb] = np.where(cls[ra, rb] < k, 0.0, margin[ra, rb])
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


# ---- the fixture and the case table of the edge tests (tests/test_gpu_render_edges.py on the device, tests/test_render_host.py
# for the model alone): one place, so both sides walk the same cases ----------------------------------------------------------
BOARD_SHAPE, BOARD_RES, BOARD_ORIGIN, BOARD_MPP = (37, 53), 0.0537, (-1.3, -0.7, 0.37), 0.0179   # a pixel is a third of a cell
BOARD_E, BOARD_A, BOARD_BEAMS, BOARD_LIDAR = 2, 3, 61, 0.275
CAMERA_AGENTS = [5, 0, 0, 3]            # unsorted, with a duplicate
CORNER_OFFSET = (0.00713, -0.00391)
# (W, H): below one word and one wave; words_per_frame 255 / 256 / 257 as a column and as a row; one staged row; the limits
FRAME_SHAPES = [(1, 1), (2, 1), (3, 2), (5, 3), (7, 1), (13, 79), (16, 64), (4, 255), (4, 256), (4, 257), (1020, 1), (1024, 1),
                (1028, 1), (1021, 1), (1023, 1), (4096, 1), (1, 4096)]
LAYER_SETS = ["all", ("map",), ("track",), ("scan",), ("cars",)]


def board_dt(plain=False):
    """the checkerboard table [37][53]: 0 (a wall) where r + c + [r > c] is even, else res.  plain = True leaves the [r > c]
    term out: that board is its own transpose (dt[c, r] == dt[r, c]), so a kernel that swapped row and column would pass on
    it; the term flips the colours below the diagonal, and a transposed read then differs at every cell off it."""
    r, c = np.indices(BOARD_SHAPE)
    return np.where((r + c + (0 if plain else (r > c))) % 2 == 0, 0.0, BOARD_RES)


def board_world(xr, yr):
    """map-frame metres (xr along the columns, yr along the rows) -> world"""
    ox, oy, yaw = BOARD_ORIGIN
    c, s = np.cos(yaw), np.sin(yaw)
    return ox + xr * c - yr * s, oy + xr * s + yr * c


def board_map(track=True):
    return {"dt": board_dt(), "res": BOARD_RES, "origin": BOARD_ORIGIN, "track": board_track() if track else None}


def board_poses(seed=7):
    """BOARD_E * BOARD_A seeded poses inside the board, 0.4 m or more from its rim, each moved along the columns until its
    lidar stands in a free cell (from a wall cell every range is 0.0 and all hits coincide on the EGO frame's centre line)"""
    rng = np.random.default_rng(seed)
    n = BOARD_E * BOARD_A
    h, w = BOARD_SHAPE[0] * BOARD_RES, BOARD_SHAPE[1] * BOARD_RES
    xr, yr, th = rng.uniform(0.4, w - 0.8, n), rng.uniform(0.4, h - 0.4, n), rng.uniform(-np.pi, np.pi, n)
    dt, yaw = board_dt(), BOARD_ORIGIN[2]
    for k in range(n):
        lx, ly = BOARD_LIDAR * np.cos(th[k] - yaw), BOARD_LIDAR * np.sin(th[k] - yaw)   # the lidar offset in the map frame
        while dt[int((yr[k] + ly) / BOARD_RES), int((xr[k] + lx) / BOARD_RES)] == 0.0:
            xr[k] += BOARD_RES
    x, y = board_world(xr, yr)
    return np.stack([x, y, th], axis=1)


def board_track(m=23):
    """a closed track of m distinct points on an ellipse inside the board"""
    h, w = BOARD_SHAPE[0] * BOARD_RES, BOARD_SHAPE[1] * BOARD_RES
    t = 0.113 + 2 * np.pi * np.arange(m) / m
    x, y = board_world(w / 2 + 0.0131 + 0.91 * np.cos(t), h / 2 - 0.0071 + 0.63 * np.sin(t))
    return np.stack([x, y], axis=1)


def board_cameras():
    """[(name, spec keywords)]: WORLD on the four map corners at two angles, wholly outside, inside one cell; FOLLOW; EGO"""
    h, w = BOARD_SHAPE[0] * BOARD_RES, BOARD_SHAPE[1] * BOARD_RES
    cams = []
    for q, (xr, yr) in enumerate([(0.0, 0.0), (w, 0.0), (w, h), (0.0, h)]):
        x, y = board_world(xr, yr)
        for angle in (0.3, -1.1):
            cams.append(("corner%d@%g" % (q, angle), dict(view="world", m_per_px=BOARD_MPP, angle=angle,
                                                         center=(float(x + CORNER_OFFSET[0]), float(y + CORNER_OFFSET[1])))))
    cams.append(("outside", dict(view="world", m_per_px=BOARD_MPP, angle=0.3, center=(140.00713, -125.00391))))
    cams.append(("one cell", one_cell_camera()))
    cams.append(("follow", dict(view="follow", m_per_px=BOARD_MPP, fwd_offset=0.137)))
    cams.append(("ego", dict(view="ego", m_per_px=BOARD_MPP)))
    return cams


def one_cell_camera(row=18, col=26):
    """WORLD on the middle of a cell at res / 50 per pixel: a 5 x 5 frame lies wholly inside the cell"""
    x, y = board_world((col + 0.5) * BOARD_RES + 0.00013, (row + 0.5) * BOARD_RES - 0.00007)
    return dict(view="world", m_per_px=BOARD_RES / 50, angle=-1.1, center=(float(x), float(y)))


def board_scene(poses, scans, **kw):
    kw.setdefault("lidar_dist", BOARD_LIDAR)
    return Scene(poses, scans, BOARD_A, [board_map()], 0.58, 0.31, **kw)


def max_share_of(width, height):
    """the undecided share a comparison may leave out: none of a frame under 1000 pixels (one pixel of a 1 x 1 frame is the
    whole frame), 0.1 % of a larger one"""
    return 0.0 if int(width) * int(height) < 1000 else 1e-3


# SCAN geometry (one env of two cars on the board): headings outside +-pi, a -0.0 coordinate, crafted ranges
SCAN_POSES = np.array([[0.3, 0.2, 7.1], [-0.0, 0.45, -9.3]])
SCAN_FRAMES = [dict(view="ego", width=64, height=64, m_per_px=0.05, fwd_offset=0.00713),
               dict(view="world", width=96, height=80, m_per_px=0.8, center=(0.15713, 0.32109), angle=0.3)]


def scan_case_ranges(B, max_range=30.0, seed=11):
    """[2][B]: short seeded ranges, and on fixed beams exactly max_range (not a hit), the largest double below it (a hit, in
    the wide WORLD frame), 0.0 (on the lidar), hits far outside the EGO frame, and a NaN"""
    r = np.random.default_rng(seed).uniform(0.2, 3.0, (2, int(B)))
    for n in range(2):
        k = 3 + n
        r[n, k], r[n, k + 7], r[n, k + 14] = max_range, np.nextafter(max_range, 0.0), 0.0
        r[n, k + 21], r[n, k + 28], r[n, k + 35] = 25.0, 29.75, np.nan
        r[n, B - 1 - n] = np.nextafter(max_range, 0.0)
    return r


# the requests of the reused-buffers sequence (one handle, in this order; each also on a fresh handle): staged, tiny, F > N,
# direct, and the first again
REUSE_PALETTE = (np.arange(21).reshape(7, 3) * 11 + 3).astype(np.uint8)
REUSE = [dict(agents=[5, 0, 0, 3, 1], width=199, height=31, view="follow", m_per_px=BOARD_MPP, fwd_offset=0.137, layers="all"),
         dict(agents=[4], width=3, height=2, view="ego", m_per_px=BOARD_MPP * 5, layers="all", rgb=True, palette=REUSE_PALETTE),
         dict(agents=[5, 0, 0, 3, 1, 4, 2], width=5, height=3, view="ego", m_per_px=BOARD_MPP * 7, layers=("map", "scan", "cars")),
         dict(agents=[1, 1, 4, 2], width=8, height=4, view="follow", m_per_px=BOARD_MPP * 5, layers="all", rgb=True),
         dict(agents=[5, 0, 0, 3, 1], width=199, height=31, view="follow", m_per_px=BOARD_MPP, fwd_offset=0.137, layers="all")]
# every agent (agents=None) and more frames than agents, with repeats
COUNTS_SPEC = dict(width=7, height=5, view="ego", m_per_px=BOARD_MPP * 6, layers="all")
COUNTS_AGENTS = [5, 0, 0, 3, 1, 1, 2, 4, 4, 4, 0, 5, 3]
