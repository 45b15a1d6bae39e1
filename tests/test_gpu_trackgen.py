"""The corridor carve on the device (f110_add_map_corridor / f110_set_map_corridor / f110_corridor_mask_batch) against
the NumPy model (tests/trackgen_ref.py; tests/test_trackgen_host.py holds the fixtures' conditions on the CPU).

(1) the edge list: mask, carved count and table equal to the model, cell for cell; the slot's frame equal to the request.
(2) refusals leave outputs, the slot count and the device allocations as they were, "no cell carved" included.
(3) re-carving in place: the address and the allocations stay, the table follows, a step right behind two-block steps scans the
    new walls.
(4) a carved slot steps like a slot made from its own table.
(5) composition: the centreline of a carved slot, obstacles derived from it, the reset sampler, the render, the env layers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import centerline_ref as cref
import obstacles_ref as oref
import trackgen_ref as ref
from f1tenth_gym_amd.centerline import cell_centres

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = os.path.join(ROOT, "tests", "golden", "maps")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _sim(amd, E=1, A=1, **kw):
    """a handle whose slot 0 is the obstacle tests' small image (96 x 128)"""
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(oref.small_image(), oref.SMALL_RES, list(oref.SMALL_ORIGIN))
    return s


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _raw_line(fx):
    return _dp(fx.xy), _dp(fx.hw), int(fx.xy.shape[0]), int(fx.closed)


def _mask(s, fx):
    """(mask, carved) through BatchSim.corridor_mask, or through the ABI for a line a Track does not take"""
    from f1tenth_gym_amd import _ffi
    if fx.tm is not None:
        return s.corridor_mask(fx.tm)
    mask, carved = np.zeros((fx.H, fx.W), dtype=np.uint8), np.zeros(1, dtype=np.int64)
    _ffi.check(_ffi.lib().f110_corridor_mask_batch(s._h, *_raw_line(fx), fx.H, fx.W, *fx.frame, mask.ctypes.data_as(_ffi._u8p),
                                                   carved.ctypes.data_as(_ffi._i64p)), s._h)
    return mask, int(carved[0])


def _add(s, fx):
    from f1tenth_gym_amd import _ffi
    if fx.tm is not None:
        return s.add_track_map(fx.tm)
    slot = C.c_int32(0)
    _ffi.check(_ffi.lib().f110_add_map_corridor(s._h, *_raw_line(fx), fx.H, fx.W, fx.res, fx.origin[0], fx.origin[1], fx.origin[2], C.byref(slot)), s._h)
    return int(slot.value)


def _obs(s):
    o = s.get("state", "scans", "collisions", "in_collision")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def _same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s %s differs" % (what, k)


def _pose_on(fx, i, offset=0.0):
    """a pose on point i of the fixture's line, heading along it"""
    a, b = fx.xy[i % len(fx.xy)], fx.xy[(i + 1) % len(fx.xy)]
    return [a[0], a[1], float(np.arctan2(b[1] - a[1], b[0] - a[0])) + offset]


# ---- 1. the edge list ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.EDGE_NAMES + ref.STAR_NAMES)
def test_mask_count_table_and_frame_equal_the_model(amd, name):
    fx = ref.fixture(name)
    want_mask, want_table = fx.mask(), fx.table()
    s = _sim(amd)
    mask, carved = _mask(s, fx)
    assert mask.shape == (fx.H, fx.W) and np.array_equal(mask, want_mask.astype(np.uint8)), "%s: %d cells of the mask differ" % (name, int((mask != want_mask).sum()))
    assert carved == int(want_mask.sum())
    slot = _add(s, fx)
    assert slot == 1
    got = s.get_map_dt(slot)
    assert got.shape == (fx.H, fx.W) and np.array_equal(got, want_table), "%s: %d cells of the table differ" % (name, int((got != want_table).sum()))
    assert s.slot_frame(slot) == fx.frame
    # ... and the image a user of the reference would have loaded gives the same slot
    twin = s.add_map_image(ref.image_of(want_mask), fx.res, list(fx.origin))
    assert np.array_equal(s.get_map_dt(twin), got)
    assert np.array_equal(s.get_map_dt(0), oref.table_from_bitmap(oref.free_from_image(oref.small_image()), oref.SMALL_RES))
    if fx.tm is not None:
        assert s.tracks[slot] is fx.tm.track and s.track_maps[slot] is fx.tm
    s.close()


# ---- 2. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(amd):
    from f1tenth_gym_amd import _ffi
    L = _ffi.lib()
    fx = ref.fixture("triangle")
    s = _sim(amd)
    plain = s.add_map_image(oref.small_image(), oref.SMALL_RES, list(oref.SMALL_ORIGIN))
    assert plain == 1
    xy, hw = fx.xy.copy(), fx.hw.copy()
    slot = C.c_int32(-5)
    mask, carved = np.full((fx.H, fx.W), 9, dtype=np.uint8), np.full(1, -7, dtype=np.int64)
    mp, cp = mask.ctypes.data_as(_ffi._u8p), carved.ctypes.data_as(_ffi._i64p)
    big = np.zeros((65537, 2))
    big[:, 0] = np.arange(65537) * 1e-3
    bigw = np.full(65537, 0.1)
    none = ref.no_carve_line()

    def bad(i, v, width=False):
        a, w = xy.copy(), hw.copy()
        (w if width else a.reshape(-1))[i] = v
        return a, w
    frame = (fx.H, fx.W, fx.res, fx.origin[0], fx.origin[1], fx.origin[2])

    def add(a, w, M=3, closed=1, fr=frame, h=s._h, sl=C.byref(slot)):
        return L.f110_add_map_corridor(h, None if a is None else _dp(a), None if w is None else _dp(w), M, closed, *fr, sl)

    def msk(a, w, M=3, closed=1, fr=(fx.H, fx.W) + fx.frame, h=s._h, m=mp, c=cp):
        return L.f110_corridor_mask_batch(h, None if a is None else _dp(a), None if w is None else _dp(w), M, closed, *fr, m, c)
    lines = [("M < 3 closed", (xy, hw, 2, 1)), ("M < 2 open", (xy, hw, 1, 0)), ("M = 0", (xy, hw, 0, 0)), ("M < 0", (xy, hw, -3, 1)),
             ("M > 65536", (big, bigw, 65537, 1)), ("nan point", bad(2, float("nan")) + (3, 1)), ("inf point", bad(5, float("inf")) + (3, 1)),
             ("nan width", bad(1, float("nan"), True) + (3, 1)), ("inf width", bad(0, float("inf"), True) + (3, 1)),
             ("negative width", bad(2, -1e-9, True) + (3, 1)), ("null points", (None, hw, 3, 1)), ("null widths", (xy, None, 3, 1))]
    calls = [("null handle add", lambda: add(xy, hw, h=None)), ("null slot pointer", lambda: add(xy, hw, sl=None)),
             ("null handle mask", lambda: msk(xy, hw, h=None)), ("null mask", lambda: msk(xy, hw, m=None)), ("null count", lambda: msk(xy, hw, c=None)),
             ("null handle set", lambda: L.f110_set_map_corridor(None, 1, _dp(xy), _dp(hw), 3, 1))]
    for what, (a, w, M, closed) in lines:
        calls.append((what + " add", lambda a=a, w=w, M=M, closed=closed: add(a, w, M, closed)))
        calls.append((what + " mask", lambda a=a, w=w, M=M, closed=closed: msk(a, w, M, closed)))
        calls.append((what + " set", lambda a=a, w=w, M=M, closed=closed: L.f110_set_map_corridor(s._h, 2, None if a is None else _dp(a), None if w is None else _dp(w), M, closed)))
    for what, fr in [("H = 0", (0, fx.W)), ("W = 0", (fx.H, 0)), ("H < 0", (-4, fx.W)), ("W > 16384", (fx.H, 16385)), ("H > 16384", (16385, fx.W))]:
        calls.append((what + " add", lambda fr=fr: add(xy, hw, fr=fr + frame[2:])))
        calls.append((what + " mask", lambda fr=fr: msk(xy, hw, fr=fr + fx.frame)))
    for what, res in [("res = 0", 0.0), ("res < 0", -0.05), ("res nan", float("nan")), ("res inf", float("inf"))]:
        calls.append((what + " add", lambda res=res: add(xy, hw, fr=(fx.H, fx.W, res) + frame[3:])))
        calls.append((what + " mask", lambda res=res: msk(xy, hw, fr=(fx.H, fx.W, res) + fx.frame[1:])))
    calls.append(("origin nan add", lambda: add(xy, hw, fr=frame[:3] + (float("nan"), 0.0, 0.0))))
    calls.append(("yaw inf add", lambda: add(xy, hw, fr=frame[:5] + (float("inf"),))))
    calls.append(("oc nan mask", lambda: msk(xy, hw, fr=(fx.H, fx.W) + fx.frame[:3] + (float("nan"), 0.0))))
    # a border of 30 m / 1e-4 m = 300 000 cells: no 16-bit cell coordinates
    calls.append(("does not fit the padded layout", lambda: add(xy, hw, fr=(fx.H, fx.W, 1e-4) + frame[3:])))
    calls.append(("no cell carved add", lambda: add(none.xy, none.hw, 3, 0, fr=(none.H, none.W, none.res) + none.origin)))
    calls.append(("set on slot 0", lambda: L.f110_set_map_corridor(s._h, 0, _dp(xy), _dp(hw), 3, 1)))
    calls.append(("set on a slot that was not carved", lambda: L.f110_set_map_corridor(s._h, plain, _dp(xy), _dp(hw), 3, 1)))
    calls.append(("set out of range", lambda: L.f110_set_map_corridor(s._h, 9, _dp(xy), _dp(hw), 3, 1)))
    calls.append(("set negative slot", lambda: L.f110_set_map_corridor(s._h, -1, _dp(xy), _dp(hw), 3, 1)))
    # (the "set" forms of the bad lines name slot 2, the carved slot registered now: only the line is wrong with them)
    carved_slot = s.add_track_map(fx.tm)
    assert carved_slot == 2
    table, addr = s.get_map_dt(carved_slot), s.map_table_address(carved_slot)
    calls.append(("no cell carved set", lambda: L.f110_set_map_corridor(s._h, carved_slot, _dp(none.xy), _dp(none.hw), 3, 0)))
    s.sync()
    allocs = amd.device_allocs()
    for what, call in calls:
        rc = call()
        assert rc == _ffi.ERR_INVALID, (what, rc)
        assert _ffi.last_error(None if "null handle" in what else s._h), what
        assert amd.device_allocs() == allocs, what
    assert "no cell carved" in _ffi.last_error(s._h)
    assert slot.value == -5 and np.all(mask == 9) and carved[0] == -7
    assert np.array_equal(s.get_map_dt(carved_slot), table) and s.map_table_address(carved_slot) == addr
    assert np.array_equal(s.get_map_dt(plain), s.get_map_dt(0))
    with pytest.raises(ValueError):
        s.set_track_map(plain, fx.tm)
    with pytest.raises(ValueError, match="frame"):
        s.set_track_map(carved_slot, ref.fixture("w63").tm)
    assert amd.device_allocs() == allocs
    # the mask of nothing is a result, not a refusal
    m0, c0 = _mask(s, none)
    assert c0 == 0 and not m0.any()
    # the next slot number shows that no refused call registered anything
    assert s.add_track_map(fx.tm) == carved_slot + 1
    s.close()
    # "no cell carved" on a fresh handle, whose scratch the call itself had to make: the allocations are as they were
    s = _sim(amd)
    s.sync()
    allocs = amd.device_allocs()
    assert L.f110_add_map_corridor(s._h, _dp(none.xy), _dp(none.hw), 3, 0, none.H, none.W, none.res, *none.origin, C.byref(slot)) == _ffi.ERR_INVALID
    assert amd.device_allocs() == allocs and slot.value == -5
    assert s.add_track_map(fx.tm) == 1
    s.close()
    # a layout other than the padded one
    s = _sim(amd, map_layout=_ffi.MAP_ROWMAJOR_F64)
    s.sync()
    allocs = amd.device_allocs()
    assert L.f110_add_map_corridor(s._h, _dp(xy), _dp(hw), 3, 1, *frame, C.byref(slot)) == _ffi.ERR_STATE
    assert "F110_MAP_PADDED_F64" in _ffi.last_error(s._h) and amd.device_allocs() == allocs and slot.value == -5
    s.close()


# ---- 3. in place --------------------------------------------------------------------------------------------------------------
def test_recarve_in_place(amd):
    lines = ref.inplace_fixtures()
    base = lines[0]
    E, A = 4, 2
    s = _sim(amd, E, A)
    slot = s.add_track_map(base.tm)
    twins = [s.add_map_dt(fx.table(), fx.res, list(fx.origin)) for fx in lines]
    s.set_env_maps([slot] + twins)
    view = dict(agents=[0], width=150, height=128, view="world", m_per_px=base.res, center=base.cell_xy(63.5, 74.5), angle=0.0, layers=("map",))
    s.set_track_map(slot, lines[1].tm)      # (the line's scratch and the track's buffers have their size now: every line has 57 points)
    s.sync()
    addr = s.map_table_address(slot)
    for k in (0, 2, 1):
        fx = lines[k]
        allocs = amd.device_allocs()
        s.set_track_map(slot, fx.tm)
        assert s.map_table_address(slot) == addr and amd.device_allocs() == allocs, k
        got = s.get_map_dt(slot)
        assert np.array_equal(got, fx.table()), "line %d: %d cells differ" % (k, int((got != fx.table()).sum()))
        assert s.tracks[slot] is fx.tm.track
        # env 0 on the carved slot and env 1 + k on the slot made from line k's table: a car on the line, and one outside the
        # table whose every sample reads the out-of-bounds value T[H-1][W-1]
        outside = list(fx.cell_xy(-40.0, 20.0)) + [0.7]
        poses = np.array([[_pose_on(fx, 5 + e), outside] for e in range(E)])
        poses[1 + k] = poses[0]
        s.reset(poses.reshape(E * A, 3))
        s.step(np.tile([0.05, 1.5], (E * A, 1)))
        o = {key: v.reshape((E, A) + v.shape[1:]) for key, v in _obs(s).items()}
        for key, v in o.items():
            assert np.array_equal(v[0], v[1 + k], equal_nan=True), "line %d: %s differs between the carved slot and its table's twin" % (k, key)
        assert fx.table()[fx.H - 1, fx.W - 1] == 0.0 and np.all(o["scans"][0, 1] == o["scans"][1 + k, 1])
        assert 0.0 < o["scans"][0, 0].max() < 30.0
        # the render's occupancy follows (the cached grid was marked stale)
        cls = s.render(**view)
        s.set_env_maps([twins[k]] + twins)
        assert np.array_equal(s.render(**view), cls) and len(np.unique(cls)) >= 2
        s.set_env_maps([slot] + twins)
    s.close()


def test_corridor_times_bracket_the_last_carve(amd):
    from f1tenth_gym_amd import _ffi
    fx, none = ref.fixture("star90"), ref.no_carve_line()
    s = _sim(amd)
    assert s.corridor_times() == dict(mask=0.0, edt=0.0)
    slot = s.add_track_map(fx.tm)
    t = s.corridor_times()
    assert 0.0 < t["mask"] < 100.0 and 0.0 < t["edt"] < 100.0
    s.set_track_map(slot, fx.tm)
    t = s.corridor_times()
    assert 0.0 < t["mask"] < 100.0 and 0.0 < t["edt"] < 100.0
    # a call refused for carving nothing ran the mask kernel and no distance transform
    assert _ffi.lib().f110_set_map_corridor(s._h, slot, _dp(none.xy), _dp(none.hw), 3, 0) == _ffi.ERR_INVALID
    t = s.corridor_times()
    assert t["mask"] > 0.0 and t["edt"] == 0.0
    assert np.array_equal(s.get_map_dt(slot), fx.table())
    assert _ffi.lib().f110_map_corridor_times(s._h, None) == _ffi.ERR_INVALID and _ffi.lib().f110_map_corridor_times(None, None) == _ffi.ERR_INVALID
    s.close()


def test_recarve_is_ordered_between_two_block_steps(amd):
    lines = ref.inplace_fixtures()
    E, A = 256, 2
    rng = np.random.default_rng(2)
    poses = np.array([[_pose_on(lines[0], i), _pose_on(lines[0], i + 20, 0.05)] for i in rng.integers(0, 57, E)]).reshape(E * A, 3)
    acts = np.stack([rng.uniform(-0.2, 0.2, E * A), rng.uniform(0.5, 3.0, E * A)], axis=1)
    out = []
    for synced in (False, True):
        s = _sim(amd, E, A, step_groups=2)
        d = s.add_track_map(lines[0].tm)
        s.set_env_maps([d if e % 2 else 0 for e in range(E)])
        s.reset(poses)
        d_act = s.device_array((E * A, 2))
        d_act.upload(acts)
        s.step_device(d_act)          # (the first step after a reset forks from the main stream)
        s.step_device(d_act)
        if synced:
            s.sync()
        assert s.step_groups()[2] == 2
        s.set_track_map(d, lines[1].tm)
        if synced:
            s.sync()
        s.step_device(d_act)
        assert s.step_groups()[2] == 2
        out.append(_obs(s))
        assert np.array_equal(s.get_map_dt(d), lines[1].table())
        d_act.free()
        s.close()
    _same(out[0], out[1], "unsynchronised against synchronised:")
    # and the re-carve mattered: the same sequence without it ends elsewhere
    s = _sim(amd, E, A, step_groups=2)
    d = s.add_track_map(lines[0].tm)
    s.set_env_maps([d if e % 2 else 0 for e in range(E)])
    s.reset(poses)
    for _ in range(3):
        s.step(acts)
    assert not np.array_equal(_obs(s)["scans"], out[0]["scans"])
    s.close()


# ---- 4. a carved slot is a slot like any other --------------------------------------------------------------------------------
def test_stepping_on_a_carved_slot_and_on_a_slot_of_its_table_is_identical(amd):
    fx = ref.fixture("star120")      # (the frame turned by 0.3)
    E, A, T = 2, 3, 20
    s = _sim(amd, E, A)
    slot = s.add_track_map(fx.tm)
    twin = s.add_map_dt(s.get_map_dt(slot), fx.res, list(fx.origin))
    s.set_env_maps([slot, twin])
    half = np.array([_pose_on(fx, 3), _pose_on(fx, 60, 0.2), list(fx.cell_xy(-30.0, 300.0)) + [2.0]])   # two on the line, one outside the table
    s.reset(np.concatenate([half, half]))
    rng = np.random.default_rng(5)
    moved = False
    for t in range(T):
        a = np.stack([rng.uniform(-0.2, 0.2, A), rng.uniform(0.5, 3.0, A)], axis=1)
        s.step(np.concatenate([a, a]))
        o = _obs(s)
        for k, v in o.items():
            v = v.reshape((E, A) + v.shape[1:])
            assert np.array_equal(v[0], v[1], equal_nan=True), "step %d: %s differs" % (t, k)
        moved = moved or float(o["scans"].reshape(E, A, -1)[0, 0].max()) > 1.0
    assert moved
    s.close()


# ---- 5. composition -----------------------------------------------------------------------------------------------------------
def test_centerline_of_a_carved_slot(amd):
    for name in ("star57", "star120"):
        fx = ref.fixture(name)
        s = _sim(amd)
        slot = s.add_track_map(fx.tm)
        cells, hw, deleted = s.centerline_cells(slot, seed=tuple(fx.xy[0]))
        T = fx.table()
        wc, whw, wdel, _ = cref.centerline(T > 0, T, fx.res, fx.origin, seed=tuple(fx.xy[0]))
        assert np.array_equal(cells, wc) and np.array_equal(hw, whw) and np.array_equal(deleted, wdel)
        dev = float(np.max(ref.polyline_distance(cell_centres(cells, s.slot_frame(slot)), fx.xy))) / fx.res
        assert dev <= ref.ROUND_TRIP_CELLS[name] + 0.25, (name, dev)
        t = s.centerline(slot, seed=tuple(fx.xy[0]))
        assert t.closed and float(np.max(ref.polyline_distance(t.xy, fx.xy))) / fx.res <= ref.ROUND_TRIP_CELLS[name] + 0.25
        s.close()


def test_obstacles_derived_from_a_carved_slot(amd):
    from f1tenth_gym_amd import Obstacles
    fx = ref.fixture("star90")
    p, q = fx.xy[7], fx.xy[50]
    ob = Obstacles(np.vstack([Obstacles.boxes([p[0] + 0.0113, p[1] - 0.0071], 0.4, 0.31, 0.23).rows, Obstacles.discs([q[0] - 0.0091, q[1] + 0.0037], 0.137).rows]))
    assert oref.boundary_margin(ob, fx.H, fx.W, fx.res, fx.origin) > 1e-9
    want, stamped = oref.derived_table(fx.table(), ob, fx.res, fx.origin)
    assert stamped.sum() > 10 and int((want != fx.table()).sum()) > 20
    s = _sim(amd)
    slot = s.add_track_map(fx.tm)
    d = s.add_obstacle_map(ob, base=slot)
    assert np.array_equal(s.get_map_dt(d), want) and s.tracks[d] is fx.tm.track
    # a derived slot of a re-carved base keeps its old contents until it is re-stamped
    other = ref.Fx("other", ref.star_points(90, 2.5, 3, 0.1, 0.2, fx.cell_xy(79.3, 99.6)), 0.5, True, fx.H, fx.W, fx.res, fx.origin)
    s.set_track_map(slot, other.tm)
    assert np.array_equal(s.get_map_dt(d), want) and np.array_equal(s.get_map_dt(slot), other.table())
    s.set_obstacles(d, ob)
    assert np.array_equal(s.get_map_dt(d), oref.derived_table(other.table(), ob, fx.res, fx.origin)[0])
    s.close()


def test_reset_sampler_places_cars_on_the_generating_line(amd):
    fx = ref.fixture("star160")
    E, A, clear = 64, 2, 0.3
    s = _sim(amd, E, A)
    slot = s.add_track_map(fx.tm)
    s.set_env_maps([slot] * E)
    s.set_reset_sampler(seed=11, gap=1.0, clearance=clear)
    s.sample_reset()
    poses = s.reset_sampler_poses().reshape(-1, 3)
    assert s.reset_sampler_stats()["fallbacks"] == 0
    assert float(np.max(ref.polyline_distance(poses[:, :2], fx.xy))) < 1e-9
    T, (res, ox, oy, oc, os_) = fx.table(), fx.frame
    xt, yt = poses[:, 0] - ox, poses[:, 1] - oy
    c, r = ((xt * oc + yt * os_) / res).astype(int), ((-xt * os_ + yt * oc) / res).astype(int)
    assert np.all(T[r, c] >= clear)
    s.close()


def test_render_shows_the_corridor(amd):
    from f1tenth_gym_amd import render as R
    fx = ref.fixture("w129")
    s = _sim(amd, 2, 1)
    slot = s.add_track_map(fx.tm)
    twin = s.add_map_image(ref.image_of(fx.mask()), fx.res, list(fx.origin))
    s.set_env_maps([slot, twin])
    s.reset(np.array([_pose_on(fx, 0), _pose_on(fx, 0)]))
    # one pixel per cell, pixel centres on cell centres: the frame's FREE pixels are the mask
    view = dict(width=fx.W, height=fx.H, view="world", m_per_px=fx.res, center=fx.cell_xy(0.5 * (fx.H - 1), 0.5 * (fx.W - 1)), angle=0.0, layers=("map",))
    dev = s.render_device([0, 1], **view)
    cls = dev.download()
    dev.free()
    assert np.array_equal(cls[0], cls[1])
    free = cls[0] == R.CLASSES.index("free")
    assert int(free.sum()) == int(fx.mask().sum())
    assert np.array_equal(free, fx.mask()) or np.array_equal(free, np.flipud(fx.mask()))
    s.close()


def _kw():
    return dict(map=os.path.join(MAPS, "example_map"), map_ext=".png", num_agents=2)


def test_env_layers_against_the_batchsim_form(amd):
    lines = ref.inplace_fixtures()
    tm, tm2 = lines[0].tm, lines[2].tm
    E, A, T = 4, 2, 12
    env_map = [1, 1, 0, 1]
    poses = np.array([[_pose_on(lines[0], 4 + 9 * e), _pose_on(lines[0], 30 + 5 * e, 0.1)] for e in range(E)])
    rng = np.random.default_rng(1)
    acts = np.stack([rng.uniform(-0.1, 0.1, (T, E, A)), rng.uniform(0.5, 2.0, (T, E, A))], axis=3)
    keys = ("scans", "poses_x", "poses_y", "poses_theta", "collisions", "progress", "lateral_offset")

    def run(env, recarve):
        rows = []
        o, r, _, _ = env.reset(poses)
        rows.append(dict({k: np.array(o[k], copy=True) for k in keys}, reward=np.array(r, copy=True)))
        for t in range(T):
            if t == 6:
                recarve(env)
            o, r, _, _ = env.step(acts[t])
            rows.append(dict({k: np.array(o[k], copy=True) for k in keys}, reward=np.array(r, copy=True)))
        return rows
    a = amd.F110VecEnv(E, device_logic=True, track_maps=[tm], env_map=env_map, reward='progress', track=tm.track, **_kw())
    assert a.track_maps == {1: tm} and a.tracks[1] is tm.track
    ra = run(a, lambda env: env.set_track_map(1, tm2))
    assert a.tracks[1] is tm2.track and np.array_equal(a.sim.batch.get_map_dt(1), lines[2].table())
    a.sim.batch.close()
    b = amd.F110VecEnv(E, device_logic=True, reward='progress', track=tm.track, **_kw())
    assert b.sim.batch.add_track_map(tm) == 1
    b.set_env_maps(env_map)
    rb = run(b, lambda env: env.sim.batch.set_track_map(1, tm2))
    b.sim.batch.close()
    for t, (x, y) in enumerate(zip(ra, rb)):
        _same(x, y, "vec env, step %d:" % t)
    assert np.any(ra[-1]["reward"] != 0.0)
    sh = amd.ShardedVecEnv(E, devices=[0, 0], track_maps=[tm], env_map=env_map, reward='progress', track=tm.track, **_kw())
    rs = run(sh, lambda env: env.set_track_map(1, tm2))
    assert all(np.array_equal(k.sim.batch.get_map_dt(1), lines[2].table()) for k in sh.shards)
    sh.close()
    for t, (x, y) in enumerate(zip(ra, rs)):
        _same(x, y, "sharded env, step %d:" % t)
    # obstacles derive from carved slots: track_maps come before obstacle_maps
    c = amd.F110VecEnv(2, device_logic=True, track_maps=[tm, dict(seed=3, radius=3.0, half_width=0.5)], obstacle_maps=[(2, None)], env_map=[2, 3], **_kw())
    assert sorted(c.track_maps) == [1, 2] and c.obstacle_slots == {3: 2} and c.tracks[3] is c.tracks[2]
    assert np.array_equal(c.sim.batch.get_map_dt(3), c.sim.batch.get_map_dt(2))
    c.sim.batch.close()


def test_single_env_on_a_carved_track(amd):
    fx = ref.inplace_fixtures()[0]
    kw = dict(map=os.path.join(MAPS, "example_map"), map_ext=".png", num_agents=1)
    start = np.array([_pose_on(fx, 9)])
    e = amd.F110Env(track_map=fx.tm, **kw)
    assert e.map_slot == 1 and e.track is fx.tm.track
    assert np.array_equal(e.sim.batch.get_map_dt(1), fx.table())
    o1 = e.reset(start)[0]
    p = amd.F110Env(track=fx.tm.track, **kw)
    assert p.sim.batch.add_track_map(fx.tm) == 1
    p.sim.batch.set_env_maps([1])
    o2 = p.reset(start)[0]
    for k in ("scans", "poses_x", "poses_y", "progress", "lateral_offset"):
        assert np.array_equal(np.asarray(o1[k]), np.asarray(o2[k])), k
    assert 0.0 < np.max(o1["scans"]) < 30.0 and abs(float(np.asarray(o1["lateral_offset"])[0])) < 0.05
    e.sim.batch.close()
    p.sim.batch.close()


def test_example_runs():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "random_tracks.py"), "--envs", "64", "--steps", "60", "--redraw", "25"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout[-3000:]
    assert "re-drawn" in proc.stdout
