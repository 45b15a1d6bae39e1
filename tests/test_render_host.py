"""CPU: the render's class rules as tests/render_ref.py states them (hand-computed cases), the f110_render_spec binding, the
argument checks that run before the library is called, F110Env.render's default camera, and the edge tests' fixture and case
table (render_ref.board_*) walked with the model alone: nothing undecided, and a slipped or transposed map read shows."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import render_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene(poses, A, maps=None, lengths=0.58, widths=0.31, scans=None, **kw):
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 3)
    if scans is None:
        scans = np.full((poses.shape[0], 4), 30.0)
    return R.Scene(poses, scans, A, maps or [], lengths, widths, **kw)


def test_car_on_a_pixel_corner_covers_14_by_8_pixels():
    # 0.58 x 0.31 m at heading 0, centred on a pixel corner at 0.04 m/px: centres at +-0.02, +-0.06, ... -> 7 + 7 along, 4 + 4 across
    sc = _scene([[1.0, 2.0, 0.0], [50.0, 50.0, 0.0]], A=2)
    cls, margin = R.render_frame(sc, 0, width=40, height=30, view="world", m_per_px=0.04, center=(1.0, 2.0), layers=("cars",))
    assert np.count_nonzero(cls == 6) == 14 * 8
    rows, cols = np.nonzero(cls == 6)
    assert (rows.min(), rows.max(), cols.min(), cols.max()) == (11, 18, 13, 26)
    assert np.all(cls[cls != 6] == 1)          # map off: FREE everywhere else
    assert margin.min() > 1e-3                 # no centre near an edge
    # the same car seen from another agent's camera is a CAR
    sc2 = _scene([[1.0, 2.0, 0.0], [1.0, 2.0, 0.0]], A=2)
    cls2, _ = R.render_frame(sc2, 1, width=40, height=30, view="world", m_per_px=0.04, center=(1.0, 2.0), layers=("cars",))
    assert np.count_nonzero(cls2 == 6) == 14 * 8   # SELF (6) beats CAR (5) on the shared pixels


def _xy_2_rc(x, y, ox, oy, oc, os_, res, h, w):
    """laser_models.py:55-86, literally"""
    x_trans, y_trans = x - ox, y - oy
    x_rot = x_trans * oc + y_trans * os_
    y_rot = -x_trans * os_ + y_trans * oc
    if x_rot < 0 or x_rot >= w * res or y_rot < 0 or y_rot >= h * res:
        return -1, -1
    return int(y_rot / res), int(x_rot / res)


def test_wall_free_outside_on_a_yawed_origin():
    dt = np.array([[0.0, 0.5, 1.0, 0.5, 0.0],
                   [0.5, 1.0, 0.0, 1.0, 0.5],
                   [0.0, 0.0, 0.5, 0.5, 0.5],
                   [1.5, 0.0, 1.0, 0.0, 2.0]])
    res, origin = 0.3, (1.0, -2.0, 0.4)
    sc = _scene([[0.0, 0.0, 0.0]], A=1, maps=[{"dt": dt, "res": res, "origin": origin}])
    H, W, mpp, ctr = 24, 32, 0.07, (1.6, -1.2)
    cls, margin = R.render_frame(sc, 0, width=W, height=H, view="world", m_per_px=mpp, center=ctr, layers=("map",))
    oc, os_ = math.cos(origin[2]), math.sin(origin[2])
    for i in range(H):
        for j in range(W):
            x = ctr[0] + (((j + 0.5) - W / 2) * mpp * 1.0 - (H / 2 - (i + 0.5)) * mpp * 0.0)
            y = ctr[1] + (((j + 0.5) - W / 2) * mpp * 0.0 + (H / 2 - (i + 0.5)) * mpp * 1.0)
            r, c = _xy_2_rc(x, y, origin[0], origin[1], oc, os_, res, *dt.shape)
            want = 0 if r < 0 else (2 if dt[r, c] == 0.0 else 1)
            assert cls[i, j] == want, (i, j, cls[i, j], want)
    assert {0, 1, 2} <= set(np.unique(cls).tolist())
    assert (margin < R.MARGIN).mean() <= 1e-3


def test_highest_class_wins():
    dt = np.zeros((40, 40))                    # all wall
    track = np.array([[1.0, 1.0], [1.3, 1.0], [1.3, 1.3], [5.0, 5.0]])
    scans = np.array([[0.4, 30.0, 30.0, 30.0]])
    sc = _scene([[1.0, 1.0, 0.0], [5.0, 5.0, 0.0]], A=2, maps=[{"dt": dt, "res": 0.1, "origin": (0.0, 0.0, 0.0), "track": track}],
                scans=np.vstack([scans, scans]))
    cls, _ = R.render_frame(sc, 0, width=100, height=100, view="world", m_per_px=0.05, center=(3.0, 3.0), layers="all",
                            tracks_closed=False)

    def px(x, y):
        return int(math.floor(50 - (y - 3.0) / 0.05)), int(math.floor((x - 3.0) / 0.05 + 50))
    assert cls[px(1.0, 1.0)] == 6              # a track point inside the camera car: SELF
    assert cls[px(5.0, 5.0)] == 5              # ... inside another car: CAR
    assert cls[px(1.3, 1.3)] == 3              # on a wall: TRACK
    assert cls[px(3.52, 3.52)] == 2              # wall only
    assert np.count_nonzero(cls == 4) == 1     # the one hit (0.4 m) of the camera agent's scan


def test_render_spec_layout_matches_header():
    from f1tenth_gym_amd import render
    S = render.RenderSpec
    assert C.sizeof(S) == 4 * 4 + 7 * 8
    assert (S.m_per_px.offset, S.center_x.offset, S.angle.offset, S.car_width.offset) == (16, 24, 40, 64)
    hdr = open(os.path.join(ROOT, "include", "f110.h")).read()
    body = re.search(r"typedef struct f110_render_spec \{(.*?)\} f110_render_spec;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"([a-z_]+)\s*[,;]", body)
    assert names == [f for f, _ in S._fields_]
    for name, val in (("F110_VIEW_EGO", 2), ("F110_LAYER_CARS", 8), ("F110_CLASS_SELF", 6)):
        assert re.search(r"\b%s = %d\b" % (name, val), hdr), name


@pytest.mark.parametrize("kw", [dict(width=0), dict(height=4097), dict(width=2.5), dict(m_per_px=0.0), dict(m_per_px=float("nan")),
                                dict(m_per_px=float("inf")), dict(view="top"), dict(layers=("map", "lidar")), dict(layers=16),
                                dict(center=(0.0, float("nan"))), dict(car_size=(0.5, 0.0)), dict(angle=float("inf"))])
def test_bad_specs_raise_value_error_without_a_gpu(kw):
    from f1tenth_gym_amd import render
    with pytest.raises(ValueError):
        render.make_spec(**kw)


def test_bad_agents_and_palettes_raise_value_error():
    from f1tenth_gym_amd import render
    spec = render.make_spec(width=64, height=64)
    for bad in ([-1], [8], [], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            render.check_agents(bad, 8, spec)
    assert render.check_agents(None, 8, spec).tolist() == list(range(8))
    big = render.make_spec(width=4096, height=4096)
    with pytest.raises(ValueError):
        render.check_agents(np.zeros(129, dtype=np.int32), 8, big)   # 129 * 2^24 > 2^31
    render.check_agents(np.zeros(128, dtype=np.int32), 8, big)
    for bad in (np.zeros((6, 3)), np.full((7, 3), 256), np.full((7, 3), -1)):
        with pytest.raises(ValueError):
            render.check_palette(bad)


def test_env_render_defaults_and_validation():
    from f1tenth_gym_amd import env, F110Env
    d = env.RENDER_DEFAULTS
    assert (d["width"], d["height"], d["view"], d["m_per_px"], tuple(d["center"]), d["angle"]) == (1000, 800, "world", 0.024, (0.0, 0.0), 0.0)
    assert abs(d["m_per_px"] - 1.0 / (50 * 1.2 / 1.44)) < 1e-15 or d["m_per_px"] == 0.024
    assert d["layers"] is None                 # every layer that has data
    assert 'rgb_array' in F110Env.metadata['render.modes'] and 'human' in F110Env.metadata['render.modes']
    with pytest.raises(ValueError):
        env._render_spec(d, {"view": "sideways"})
    with pytest.raises(ValueError):
        env._render_spec(d, {"zoom": 2})
    assert env._render_spec(d, {"view": "follow"})["view"] == "follow"


def test_palette_of_classes():
    from f1tenth_gym_amd import render
    cls = np.arange(7, dtype=np.uint8).reshape(1, 7)
    rgb = render.colorize(cls)
    assert rgb.shape == (1, 7, 3) and rgb.dtype == np.uint8
    assert rgb[0].tolist() == [[9, 32, 87], [9, 32, 87], [183, 193, 222], [183, 193, 222], [255, 190, 0], [99, 52, 94], [172, 97, 185]]
    pal = np.arange(21).reshape(7, 3)
    assert np.array_equal(render.colorize(cls, pal)[0], pal)


# ---- the edge tests' fixture and case table (render_ref.board_*, FRAME_SHAPES), with the model alone ---------------------------
def _board_scene():
    """the fixture's poses with the oracle's scans of the checkerboard from their lidar poses"""
    from oracle import orc
    poses = R.board_poses()
    so = orc.ScanOracle(R.BOARD_BEAMS, 4.7)
    so.set_map_dt(R.board_dt(), R.BOARD_RES, R.BOARD_ORIGIN)
    lidar = poses + R.BOARD_LIDAR * np.stack([np.cos(poses[:, 2]), np.sin(poses[:, 2]), 0 * poses[:, 2]], axis=1)
    return R.board_scene(poses, np.stack([so.scan(p) for p in lidar]))


@pytest.fixture(scope="module")
def board():
    return _board_scene()


@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=lambda s: "%dx%d" % s)
def test_case_table_leaves_nothing_undecided(board, shape):
    """every camera, every layer set, the four frames of CAMERA_AGENTS: no undecided pixel in a frame under 1000 pixels, at
    most 0.1 % of a larger one (what the GPU comparisons of the same cases are held to)"""
    W, H = shape
    for name, cam in R.board_cameras():
        for layers in R.LAYER_SETS:
            _, margin = R.render(board, R.CAMERA_AGENTS, width=W, height=H, layers=layers, **cam)
            for f in range(len(R.CAMERA_AGENTS)):
                share = float((margin[f] < R.MARGIN).mean())
                assert share <= R.max_share_of(W, H), (name, layers, f, share)


def test_reuse_and_count_requests_leave_nothing_undecided(board):
    for req in R.REUSE + [dict(R.COUNTS_SPEC, agents=R.COUNTS_AGENTS)]:
        spec = {k: v for k, v in req.items() if k not in ("agents", "rgb", "palette")}
        _, margin = R.render(board, req["agents"], **spec)
        share = (margin < R.MARGIN).mean(axis=(1, 2)).max()
        assert share <= R.max_share_of(spec["width"], spec["height"]), (spec, share)


def test_scan_cases_stay_under_the_cap():
    for lidar in (0.0, 0.275):
        for B in (61, 1080, 4096):
            for fov in (4.7, 6.0):
                sc = R.Scene(R.SCAN_POSES, R.scan_case_ranges(B), 2, [R.board_map()], 0.58, 0.31, fov=fov, lidar_dist=lidar)
                for spec in R.SCAN_FRAMES:
                    for layers in (("scan",), "all"):
                        cls, margin = R.render(sc, [0, 1], layers=layers, **spec)
                        assert float((margin < R.MARGIN).mean(axis=(1, 2)).max()) <= 1e-3, (lidar, B, fov, spec["view"], layers)
                        assert (cls == 4).any()


@pytest.mark.parametrize("slip", ["col", "row", "swap"])
def test_checkerboard_tells_a_slip_of_one_cell_or_a_transposition(board, slip):
    """reading the table one column on, one row on or transposed changes more than half of the in-map pixels of the fixture's
    frames.  (On the plain parity board, r + c even, the transposed read would change only the clamped cells: dt[c, r] ==
    dt[r, c]; board_dt's [r > c] term is there for that.)"""
    changed = inmap = 0
    for W, H in [(5, 3), (13, 79), (16, 64), (4, 255), (1020, 1)]:
        for name, cam in R.board_cameras():
            good, _ = R.render(board, R.CAMERA_AGENTS, width=W, height=H, layers=("map",), **cam)
            bad, _ = R.render(board, R.CAMERA_AGENTS, width=W, height=H, layers=("map",), map_slip=slip, **cam)
            inmap += int((good != 0).sum())
            changed += int((good != bad).sum())
            assert ((good == 0) == (bad == 0)).all()
    assert inmap > 20000 and changed > 0.5 * inmap, (slip, changed, inmap)
    if slip == "swap":   # why the board is not the plain one
        plain = R.board_dt(plain=True)
        r, c = np.indices(plain.shape)
        same = plain[np.minimum(c, plain.shape[0] - 1), np.minimum(r, plain.shape[1] - 1)] == plain
        assert same.mean() > 0.8


def test_one_cell_camera_sees_one_class():
    sc = R.board_scene(R.board_poses(), np.full((6, R.BOARD_BEAMS), 30.0))
    cls, margin = R.render(sc, [0], width=5, height=5, layers=("map",), **R.one_cell_camera(18, 26))
    assert margin.min() > 0.3 * R.BOARD_RES and np.unique(cls).tolist() == [1 if R.board_dt()[18, 26] else 2]


def test_scan_point_with_an_offset_lidar_at_heading_half_pi():
    # the lidar sits 0.275 m along +y; beam 0 of 3 over fov pi points along theta - pi/2 = 0, i.e. +x, table index 0
    scans = np.array([[0.5, 30.0, 30.0]])
    sc = _scene([[1.0, 2.0, math.pi / 2]], A=1, scans=scans, fov=math.pi, lidar_dist=0.275)
    pts = R.scan_points(sc, 0)
    assert pts.shape == (1, 2) and abs(pts[0, 0] - 1.5) < 1e-12 and abs(pts[0, 1] - 2.275) < 1e-12
    cls, _ = R.render_frame(sc, 0, width=21, height=21, view="world", m_per_px=0.1, center=(1.0, 2.0), layers=("scan",))
    assert np.argwhere(cls == 4).tolist() == [[10 - 3, 10 + 5]]   # 0.275 up (2.75 px above the centre row's middle), 0.5 right


def test_scan_indices_match_the_oracle_on_wrapped_headings():
    from oracle import orc
    for B, fov in ((61, 4.7), (1080, 6.0), (4096, 6.0), (4096, 4.7)):
        so = orc.ScanOracle(B, fov)
        for th in (7.1, -9.3, 0.0, 3.0):
            r = np.arange(B) * 1e-3 + 1.0
            sc = _scene([[0.0, 0.0, th]], A=1, scans=r[None, :], fov=fov)
            idx = so.beam_dir_indices(th)
            want = np.stack([r * sc.cosines[idx], r * sc.sines[idx]], axis=1)
            np.testing.assert_array_equal(R.scan_points(sc, 0), want)


def test_minus_zero_takes_the_lidar_offset_branch():
    # x = -0.0 leaves the on-axle shortcut: the scan pose is x + 0 * cos, which is +0.0; the hit is the same point either way
    scans = np.array([[0.7, 30.0, 30.0]])
    a = R.scan_points(_scene([[-0.0, 0.45, -9.3]], A=1, scans=scans), 0)
    b = R.scan_points(_scene([[0.0, 0.45, -9.3]], A=1, scans=scans), 0)
    np.testing.assert_array_equal(a, b)
    c = R.scan_points(_scene([[-0.0, 0.45, -9.3]], A=1, scans=scans, lidar_dist=0.275), 0)
    want = a[0] + 0.275 * np.array([np.cos(-9.3), np.sin(-9.3)])
    assert a.shape == (1, 2) and np.abs(c[0] - want).max() < 1e-15


def test_range_at_max_range_is_not_a_hit():
    below = np.nextafter(30.0, 0.0)
    sc = _scene([[0.0, 0.0, 0.0]], A=1, scans=np.array([[30.0, below, np.nan, 0.0]]))
    pts = R.scan_points(sc, 0)
    assert pts.shape == (2, 2)                      # the largest double below max_range and 0.0
    assert abs(np.hypot(*pts[0]) - below) < 1e-9 and pts[1].tolist() == [0.0, 0.0]
    cls, _ = R.render_frame(sc, 0, width=9, height=9, view="world", m_per_px=0.1, center=(0.013, 0.017), layers=("scan", "cars"))
    assert not (cls == 4).any() and cls[4, 4] == 6  # 0.0 lands on the lidar, under SELF; the far hit is out of frame


def test_a_repeated_camera_agent_gives_identical_frames():
    sc = _board_scene()
    cls, margin = R.render(sc, R.CAMERA_AGENTS, width=43, height=37, view="ego", m_per_px=R.BOARD_MPP, layers="all")
    assert R.CAMERA_AGENTS[1] == R.CAMERA_AGENTS[2]
    np.testing.assert_array_equal(cls[1], cls[2])
    np.testing.assert_array_equal(margin[1], margin[2])
    assert not np.array_equal(cls[0], cls[1])


def test_a_one_point_track_is_one_pixel():
    dt = np.ones((10, 10))
    sc = _scene([[9.0, 9.0, 0.0]], A=1, maps=[{"dt": dt, "res": 0.1, "origin": (0.0, 0.0, 0.0), "track": np.array([[0.52, 0.33]])}])
    cls, _ = R.render_frame(sc, 0, width=10, height=10, view="world", m_per_px=0.1, center=(0.5, 0.5), layers=("map", "track"))
    assert np.argwhere(cls == 3).tolist() == [[6, 5]] and np.count_nonzero(cls == 1) == 99
