"""The renderer (k_render_setup, k_render_raster, k_render_points<TRACK|SCAN>, k_render_finish, k_render_occ) at the
shapes where its launch arithmetic changes form, against tests/render_ref.py on the checkerboard fixture (render_ref.board_*):
frames below one 32-bit word and one wave, words_per_frame either side of a workgroup, the limits, the direct and the staged
form with guard bytes around both outputs, unaligned class pointers, the handle's render buffers reused across differently shaped
requests, F > N and N > 256, the SCAN layer's geometry branches and culls, 4 .. 64 cars per env, and track point counts either
side of a workgroup.  Every pixel whose decision is 1e-9 m or more from flipping is equal; a frame under 1000 pixels leaves
nothing out.  RGB and the reuse comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

import render_ref as R
from f1tenth_gym_amd import workload

pytestmark = pytest.mark.gpu

GUARD, FILL = 64, 0xAB
AGENTS = R.CAMERA_AGENTS
PALETTE = R.REUSE_PALETTE


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _board_sim(amd, poses=None, E=R.BOARD_E, A=R.BOARD_A, B=R.BOARD_BEAMS, lidar=R.BOARD_LIDAR, fov=4.7, track=True):
    """a handle on the checkerboard, reset to `poses` (the fixture's) and stepped once at rest, so that it holds scans"""
    sim = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, fov=fov, lidar_dist=lidar)
    sim.set_map_dt(R.board_dt(), R.BOARD_RES, R.BOARD_ORIGIN)
    if track:
        sim.set_track(R.board_track())
    sim.reset(R.board_poses() if poses is None else poses)
    sim.step(np.zeros((E * A, 2)))
    return sim


def _scene(sim, maps=None, **kw):
    o = sim.get("agent_poses", "scans")
    kw.setdefault("lengths", sim.params["length"])
    kw.setdefault("widths", sim.params["width"])
    return R.Scene(o["agent_poses"], o["scans"], sim.A, [R.board_map()] if maps is None else maps, fov=sim.fov,
                   theta_dis=sim.theta_dis, **kw)


@pytest.fixture(scope="module")
def board(amd):
    sim = _board_sim(amd)
    sc = _scene(sim, lidar_dist=R.BOARD_LIDAR)
    assert np.isfinite(sc.scans).all() and (sc.scans > 0).all() and (sc.scans < 30.0).any()
    yield sim, sc
    sim.close()


def _render_guarded(sim, agents, rgb=False, palette=None, shift=0, **spec):
    """f110_render_device through ctypes into pointers GUARD (+ shift) bytes inside larger buffers filled with 0xAB; the GUARD
    bytes before and after each output must still hold 0xAB -> classes [F][H][W] or (classes, rgb [F][H][W][3])"""
    from f1tenth_gym_amd import _ffi, render
    sp = render.make_spec(**spec)
    a = render.check_agents(agents, sim.N, sp)
    shape = (a.size, sp.height, sp.width)
    n = int(np.prod(shape))
    bufs = []
    for nbytes in [n] + ([3 * n] if rgb else []):
        buf = sim.device_array((GUARD + shift + nbytes + GUARD,), np.uint8)
        buf.upload(np.full(buf.shape, FILL, dtype=np.uint8))
        bufs.append((buf, nbytes))
    pal = None if palette is None else render.check_palette(palette)
    try:
        rc = _ffi.lib().f110_render_device(sim._h, C.byref(sp), None if agents is None else a.ctypes.data_as(_ffi._i32p), a.size,
                                           bufs[0][0].ptr + GUARD + shift, bufs[1][0].ptr + GUARD + shift if rgb else None,
                                           None if pal is None else pal.ctypes.data_as(_ffi._u8p))
        assert rc == _ffi.OK, _ffi.last_error(sim._h)
        out = []
        for (buf, nbytes), shp in zip(bufs, (shape, shape + (3,))):
            host = buf.download()
            lo, body, hi = host[:GUARD + shift], host[GUARD + shift:GUARD + shift + nbytes], host[GUARD + shift + nbytes:]
            assert hi.size == GUARD and (lo == FILL).all() and (hi == FILL).all(), \
                ("guard bytes overwritten", spec, np.flatnonzero(lo != FILL)[:4].tolist(), np.flatnonzero(hi != FILL)[:4].tolist())
            out.append(body.reshape(shp).copy())
    finally:
        for buf, _ in bufs:
            buf.free()
    return tuple(out) if rgb else out[0]


def _compare(got, want, margin, what):
    """render_ref.compare frame by frame, with the frame size's cap on the undecided share"""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    cap = R.max_share_of(got.shape[2], got.shape[1])
    for f in range(got.shape[0]):
        R.compare(got[f], want[f], margin[f], max_share=cap, what="%s frame %d" % (what, f))


def _check(sim, sc, agents, what, rgb=False, palette=None, shift=0, **spec):
    got = _render_guarded(sim, agents, rgb=rgb, palette=palette, shift=shift, **spec)
    cls = got[0] if rgb else got
    idx = np.arange(sc.N) if agents is None else agents
    _compare(cls, *R.render(sc, idx, **spec), what=what)
    if rgb:
        from f1tenth_gym_amd import render
        np.testing.assert_array_equal(got[1], render.colorize(cls, palette), err_msg=what)
    return cls


# ---- a. frame shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.FRAME_SHAPES, ids=lambda s: "%dx%d" % s)
def test_frame_shapes(board, shape):
    sim, sc = board
    W, H = shape
    seen = set()
    for q, (name, cam) in enumerate(R.board_cameras()):
        every = None
        for layers in R.LAYER_SETS:
            got = _check(sim, sc, AGENTS, "%dx%d %s %s" % (W, H, name, layers), width=W, height=H, layers=layers, **cam)
            np.testing.assert_array_equal(got[1], got[2])      # the repeated camera agent
            every = got if layers == "all" else every
            seen.update(np.unique(got).tolist())
        # with RGB: a custom palette on every staged shape and every other camera of the direct ones
        pal = PALETTE if (W % 4 or q % 2) else None
        again = _check(sim, sc, AGENTS, "%dx%d %s rgb" % (W, H, name), rgb=True, palette=pal, width=W, height=H, layers="all", **cam)
        np.testing.assert_array_equal(again, every)
    assert seen >= ({0, 1, 2, 6} if W * H >= 16 else {0, 6}), seen


def test_one_cell_camera_is_uniform(board):
    sim, sc = board
    got = _check(sim, sc, AGENTS, "one cell", width=5, height=5, layers=("map",), **R.one_cell_camera(18, 26))
    assert np.unique(got).tolist() == [1 if R.board_dt()[18, 26] else 2]
    wall = _check(sim, sc, AGENTS, "the next cell", width=5, height=5, layers=("map",), **R.one_cell_camera(18, 27))
    assert np.unique(wall).tolist() != np.unique(got).tolist()


# ---- b. unaligned class pointer --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rgb", [False, True])
def test_unaligned_class_pointer(board, rgb):
    sim, sc = board
    spec = dict(width=16, height=8, view="follow", m_per_px=R.BOARD_MPP * 3, fwd_offset=0.137, layers="all")
    base = _render_guarded(sim, AGENTS, rgb=rgb, palette=PALETTE, **spec)
    _compare(base[0] if rgb else base, *R.render(sc, AGENTS, **spec), what="aligned 16x8")
    for shift in (1, 2, 3):
        got = _render_guarded(sim, AGENTS, rgb=rgb, palette=PALETTE, shift=shift, **spec)
        for g, b in zip(got if rgb else (got,), base if rgb else (base,)):
            np.testing.assert_array_equal(g, b, err_msg="class pointer + %d" % shift)


# ---- c. the handle's render buffers, reused ------------------------------------------------------------------------------------------
def test_reused_buffers(amd, board):
    _, sc = board
    assert len(R.REUSE[2]["agents"]) > sc.N
    one = _board_sim(amd)
    for q, req in enumerate(R.REUSE):
        req = dict(req)
        agents = req.pop("agents")
        fresh = _board_sim(amd)
        for k, v in fresh.get("agent_poses", "scans").items():
            np.testing.assert_array_equal(v, one.get(k)[k])
        want = _render_guarded(fresh, agents, **req)
        fresh.close()
        got = _render_guarded(one, agents, **req)
        for g, w in zip(got if req.get("rgb") else (got,), want if req.get("rgb") else (want,)):
            np.testing.assert_array_equal(g, w, err_msg="request %d on the reused handle" % q)
        model = {k: v for k, v in req.items() if k not in ("rgb", "palette")}
        _compare(got[0] if req.get("rgb") else got, *R.render(sc, agents, **model), what="reused, request %d" % q)
    one.close()


# ---- d. frame and agent counts ---------------------------------------------------------------------------------------------------------
def test_every_agent_and_more_frames_than_agents(board):
    sim, sc = board
    spec = R.COUNTS_SPEC
    every = _check(sim, sc, None, "agents=None", **spec)
    assert every.shape[0] == sc.N == 6
    many = R.COUNTS_AGENTS
    got = _check(sim, sc, many, "F = 13 > N", rgb=True, **spec)
    np.testing.assert_array_equal(got, every[many])


def test_agents_beyond_the_first_workgroup_of_car_records(amd):
    E, A = 130, 2
    e = np.arange(E)
    xr, yr = 0.5 + (e % 13) * 0.137, 0.5 + (e // 13) * 0.093
    x0, y0 = R.board_world(xr, yr)
    x1, y1 = R.board_world(xr + 0.21, yr + 0.13)
    poses = np.stack([np.stack([x0, y0, 0.1 * e], axis=1), np.stack([x1, y1, 0.3 - 0.07 * e], axis=1)], axis=1).reshape(E * A, 3)
    sim = _board_sim(amd, poses, E=E, A=A, track=False)
    sc = _scene(sim, [R.board_map(track=False)], lidar_dist=R.BOARD_LIDAR)
    spec = dict(width=8, height=8, view="ego", m_per_px=0.1, layers=("map", "cars"))
    got = _render_guarded(sim, None, **spec)
    assert got.shape == (260, 8, 8)
    last = np.arange(250, 260)
    _compare(got[last], *R.render(sc, last, **spec), what="frames 250 .. 259 of 260")
    for f in last:
        assert (got[f] == 6).any() and (got[f] == 5).any(), f     # the last envs' cars, the camera's marked SELF
    sim.close()


# ---- e. SCAN geometry ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fov", [4.7, 6.0])
@pytest.mark.parametrize("B", [61, 1080, 4096])
@pytest.mark.parametrize("lidar", [0.0, 0.275])
def test_scan_geometry(amd, lidar, B, fov):
    sim = _board_sim(amd, np.array([[0.3, 0.2, 0.5], [0.1, 0.45, -0.7]]), E=1, A=2, B=B, lidar=lidar, fov=fov)
    views = sim.device_views()
    views["agent_poses"].upload(np.ascontiguousarray(R.SCAN_POSES.T))
    views["scans"].upload(R.scan_case_ranges(B))
    sc = _scene(sim, lidar_dist=lidar)
    assert sc.poses[0, 2] == 7.1 and sc.poses[1, 2] == -9.3 and sc.poses[1, 0] == 0.0 and np.signbit(sc.poses[1, 0])
    assert (sc.scans == 30.0).sum() == 2 and np.isnan(sc.scans).sum() == 2 and (sc.scans == 0.0).sum() == 2
    for spec in R.SCAN_FRAMES:
        for layers in (("scan",), "all"):
            got = _check(sim, sc, [0, 1], "lidar %g B %d fov %g %s %s" % (lidar, B, fov, spec["view"], layers), layers=layers, **spec)
            assert (got[0] == 4).any() and (got[1] == 4).any()
            if spec["view"] == "ego" and layers == "all":
                assert (got == 6).any()
    sim.close()


# ---- f. many cars per env --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def example_dt(amd):
    img, res, origin = workload.load_map_image("example_map")
    sim = amd.BatchSim(num_envs=1, num_agents=1, num_beams=8)
    sim.set_map_image(img, res, origin)
    dt = sim.get_map_dt()
    sim.close()
    return img, res, origin, dt


@pytest.mark.parametrize("A", [4, 16, 17, 64])
def test_many_cars_per_env(amd, example_dt, A):
    img, res, origin, dt = example_dt
    E = 2
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map_image(img, res, origin)
    rng = np.random.default_rng(A)
    pv = np.tile(np.array([sim.params[k] for k in amd._ffi.PARAM_KEYS]), (E * A, 1))
    pv[:, 17] = rng.uniform(0.3, 1.2, E * A)   # length
    pv[:, 16] = rng.uniform(0.2, 0.6, E * A)   # width
    pv[A - 2:A, 17], pv[A - 2:A, 16] = (1.13, 0.41), (0.27, 0.53)   # env 0's last two: long and narrow, short and wide
    sim.set_params_batch(pv)
    sim.reset(workload.bench_start_poses(E, A, gap_wp=2))      # 0.4 m apart: neighbours overlap
    sim.step(np.tile([0.0, 1.0], (E * A, 1)))
    maps = [{"dt": dt, "res": res, "origin": origin, "track": None}]
    sc = _scene(sim, maps, lengths=pv[:, 17], widths=pv[:, 16])
    cx, cy = sc.poses[:A, 0].mean() + 0.00713, sc.poses[:A, 1].mean() - 0.00391
    world = _check(sim, sc, [A // 2, A], "A=%d world" % A, width=320, height=240, view="world", m_per_px=0.1, center=(cx, cy),
                   angle=0.3, layers="all")
    assert (world[0] == 6).any() and (world[0] == 5).any()
    cams = [0, A // 2, A - 1, A, A + A // 2, 2 * A - 1]
    ego = _check(sim, sc, cams, "A=%d ego" % A, width=64, height=64, view="ego", m_per_px=0.05, layers="all")
    for f in range(len(cams)):
        assert (ego[f] == 6).any() and (ego[f] == 5).any(), f
    # two cars on one pose: the camera's own box is SELF on the shared pixels, whichever of the two it is
    ap = sim.device_views()["agent_poses"]
    host = ap.download()
    host[:, A - 1] = host[:, A - 2]
    ap.upload(host)
    sc = _scene(sim, maps, lengths=pv[:, 17], widths=pv[:, 16])
    spec = dict(width=48, height=48, view="world", m_per_px=0.03, center=(host[0, A - 1] + 0.00713, host[1, A - 1] - 0.00391),
                layers=("map", "cars"))
    pair = _check(sim, sc, [A - 2, A - 1], "A=%d two cars on one pose" % A, **spec)
    np.testing.assert_array_equal(pair[0] >= 5, pair[1] >= 5)   # the same cars cover the same pixels in both frames
    both = (pair[0] == 6) & (pair[1] == 6)                      # the two boxes' intersection: SELF in both
    assert both.any() and both[24, 24] and ((pair[0] == 6) & (pair[1] == 5)).any() and ((pair[0] == 5) & (pair[1] == 6)).any()
    sim.close()


# ---- g. TRACK points ----------------------------------------------------------------------------------------------------------------------------
def _ring(m, rx, ry, phase):
    t = phase + 2 * np.pi * np.arange(m) / m
    return np.stack([0.31 + rx * np.cos(t), 0.22 + ry * np.sin(t)], axis=1)


def _two_slots(amd, tracks):
    """2 envs x 2 cars, env 0 on the board and env 1 on the board upside down (slot 1); tracks = [slot 0's, slot 1's] or None"""
    from f1tenth_gym_amd.track import Track
    poses = np.array([[0.3, 0.2, 0.5], [0.1, 0.45, -0.7], [0.35, 0.1, 2.5], [0.2, 0.5, -2.1]])
    sim = amd.BatchSim(num_envs=2, num_agents=2, num_beams=R.BOARD_BEAMS, lidar_dist=R.BOARD_LIDAR)
    sim.set_map_dt(R.board_dt(), R.BOARD_RES, R.BOARD_ORIGIN)
    flipped = np.ascontiguousarray(R.board_dt()[::-1])
    assert sim.add_map_dt(flipped, R.BOARD_RES, R.BOARD_ORIGIN) == 1
    sim.set_env_maps(np.array([0, 1], dtype=np.int32))
    maps = [R.board_map(track=False), dict(R.board_map(track=False), dt=flipped)]

    def put(tracks):
        for slot, t in enumerate(tracks):
            if t is not None:
                sim.set_track(Track(t, closed=len(t) > 2), slot)
                maps[slot]["track"] = t
    put(tracks)
    sim.reset(poses)
    sim.step(np.zeros((4, 2)))
    return sim, maps, put


TRACK_SPEC = dict(width=48, height=40, view="follow", m_per_px=0.05, fwd_offset=0.137)


def _check_tracks(sim, maps, what, counts):
    sc = _scene(sim, maps, env_slot=np.array([0, 1]), lidar_dist=R.BOARD_LIDAR)
    got = _check(sim, sc, [3, 0, 2, 1], what, layers="all", **TRACK_SPEC)
    only = _check(sim, sc, [3, 0, 2, 1], what + " alone", layers=("track",), **TRACK_SPEC)
    for f, n in enumerate([3, 0, 2, 1]):
        m = counts[n // 2]
        assert (only[f] == 3).any() == (m > 0) and (only[f] == 3).sum() <= m, (what, f, m)
    return got


def test_track_point_counts(amd):
    sim, maps, put = _two_slots(amd, [_ring(4, 0.8, 0.6, 0.1), _ring(257, 0.9, 0.7, 0.2)])
    _check_tracks(sim, maps, "4 and 257 points", (4, 257))
    # a one-point track does not exist on the device (f110_track_set needs two points): the smallest one beside 256
    with pytest.raises(ValueError):
        sim.set_track(np.array([[0.31, 0.22]]), 1)
    put([_ring(256, 0.9, 0.7, 0.3), np.array([[0.33, 0.27], [0.21, 0.14]])])
    _check_tracks(sim, maps, "256 and 2 points", (256, 2))
    sim.close()


@pytest.mark.parametrize("which", [0, 1])
def test_a_slot_without_a_track_beside_one_with(amd, which):
    tracks = [None, None]
    tracks[which] = _ring(40, 0.8, 0.6, 0.4)
    sim, maps, _ = _two_slots(amd, tracks)
    counts = [0, 0]
    counts[which] = 40
    _check_tracks(sim, maps, "a track on slot %d only" % which, counts)
    sim.close()


def test_track_layer_without_any_track(amd):
    sim, maps, _ = _two_slots(amd, [None, None])
    got = _check_tracks(sim, maps, "no track anywhere", (0, 0))
    np.testing.assert_array_equal(got, _render_guarded(sim, [3, 0, 2, 1], layers=("map", "scan", "cars"), **TRACK_SPEC))
    sim.close()
