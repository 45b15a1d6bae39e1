"""A map slot's centreline loop extracted on the device (f110_map_centerline / f110_map_skeleton) against the NumPy
reference tests/centerline_ref.py: the final mask cell for cell, the ordered cells, the half widths and the three deletion totals on
the fixtures of tests/test_centerline_host.py, on berlin and example_map, at the widths around the word size, on a one-cell
corridor and on a derived obstacle slot; every refusal, the scratch memory, calls behind steps in flight, and the env layers."""
import os

import numpy as np
import pytest

import centerline_ref as ref
from _util import MAPS, bench_start_poses, load_map_image, oracle_map_dt
from test_centerline_host import LOOPS, REFUSED

pytestmark = pytest.mark.gpu

FIX = ref.fixtures()
MESSAGES = {"not_simple": "not a simple loop", "no_loop": "no loop is reachable"}


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def world(amd):
    """one handle with every fixture registered through add_map_image: (sim, {fixture: slot})"""
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(FIX["annulus_w10"], ref.RES, list(ref.ORIGIN))
    slots = {name: s.add_map_image(img, ref.RES, list(ref.ORIGIN)) for name, img in sorted(FIX.items())}
    yield s, slots
    s.close()


_ref_cache = {}


def reference(name):
    """(free, T, (cells, half_width, deleted, final) or the Refused, (skeleton mask, deleted)) of a fixture: computed once, shared"""
    if name not in _ref_cache:
        free = ref.free_from_image(FIX[name])
        T = ref.edt_table(free, ref.RES)
        try:
            res = ref.centerline(free, T, ref.RES, ref.ORIGIN, ref.fixture_seed(name))
        except ref.Refused as ex:
            res = ex
        _ref_cache[name] = (free, T, res, ref.skeleton(free)[:2])
    return _ref_cache[name]


def lib_error(amd):
    return amd._ffi.F110LibraryError


def raw_call(amd, s, slot, seed, cap=4096, heading=None, max_passes=0, cells=True, hw=True, n=True, deleted=True):
    """f110_map_centerline itself: -> (rc, n, cells, half_width, deleted) with the outputs pre-filled with a pattern"""
    import ctypes as C
    f = amd._ffi
    c = np.full((max(cap, 1), 2), -7, dtype=np.int32)
    w = np.full(max(cap, 1), -7.0)
    d = np.full(3, -7, dtype=np.int64)
    cnt = C.c_int32(-7)
    rc = f.lib().f110_map_centerline(s._h, slot, float(seed[0]), float(seed[1]), int(heading is not None), 0.0 if heading is None else float(heading),
                                     max_passes, f.i32ptr(c) if cells else None, f.dptr(w) if hw else None, cap, C.byref(cnt) if n else None,
                                     d.ctypes.data_as(f._i64p) if deleted else None)
    return rc, cnt.value, c, w, d


@pytest.mark.parametrize("name", sorted(FIX))
def test_fixtures(amd, world, name):
    s, slots = world
    free, T, want, (mask_ref, deleted_ref) = reference(name)
    assert np.array_equal(s.get_map_dt(slots[name]), T)
    mask, deleted = s.map_skeleton(slots[name])
    assert np.array_equal(mask.astype(bool), mask_ref) and np.array_equal(deleted, deleted_ref)
    if name in LOOPS:
        cells, hw, deleted = s.centerline_cells(slots[name], ref.fixture_seed(name))
        assert len(cells) == LOOPS[name]
        assert np.array_equal(cells, want[0]) and np.array_equal(hw, want[1]) and np.array_equal(deleted, want[2])
    else:
        with pytest.raises(lib_error(amd), match=MESSAGES[REFUSED[name]]):
            s.centerline_cells(slots[name], ref.fixture_seed(name))
        if name == "annulus_spur_diamond":
            with pytest.raises(lib_error(amd), match="5 of the 177 cells"):
                s.centerline_cells(slots[name], ref.fixture_seed(name))


def test_heading_and_track(amd, world):
    s, slots = world
    name = "annulus_w13"
    free, T, want, _ = reference(name)
    seed = ref.fixture_seed(name)
    for heading in (-0.5 * np.pi, 0.5 * np.pi, 0.0, 3.0):
        cells = s.centerline_cells(slots[name], seed, heading=heading)[0]
        assert np.array_equal(cells, ref.centerline(free, T, ref.RES, ref.ORIGIN, seed, heading=heading)[0]), heading
    up = s.centerline_cells(slots[name], seed, heading=0.5 * np.pi)[0]
    assert np.array_equal(up[0], want[0][0]) and np.array_equal(up[1:], want[0][1:][::-1])
    # the Track: the package's post-processing on the device's cells is the restatement's
    track, cells, hw, _ = s.centerline(slots[name], seed, spacing=0.15, smooth=0.6, return_cells=True)
    assert s.slot_frame(slots[name]) == (ref.RES, ref.ORIGIN[0], ref.ORIGIN[1], 1.0, 0.0)
    pts, w, kappa, _, _ = ref.post_process(cells, hw, s.slot_frame(slots[name]), 0.15, 0.6)
    assert track.closed and track.attr_names == ('half_width', 'kappa')
    assert np.allclose(track.xy, pts, rtol=0, atol=1e-12) and np.allclose(track.attrs[:, 0], w, rtol=0, atol=1e-12)
    assert np.allclose(track.attrs[:, 1], kappa, rtol=1e-9, atol=1e-9)
    t2 = amd.Track.from_map(s, slots[name], seed=seed, spacing=0.15, smooth=0.6)
    assert np.array_equal(t2.xy, track.xy) and np.array_equal(t2.attrs, track.attrs)


def test_berlin(amd):
    img, res, origin = load_map_image("berlin")
    T = oracle_map_dt("berlin")[0]
    free = ref.free_from_image(img)
    want = ref.centerline(free, T, res, origin)
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(img, res, origin)
    mask, deleted = s.map_skeleton(0)
    cells, hw, deleted2 = s.centerline_cells(0)
    s.close()
    assert len(cells) == 1297
    assert np.array_equal(mask.astype(bool), want[3]) and np.array_equal(deleted, want[2]) and np.array_equal(deleted2, want[2])
    assert np.array_equal(cells, want[0]) and np.array_equal(hw, want[1])


def test_example_map(amd):
    img, res, origin = load_map_image("example_map")
    free = ref.free_from_image(img)
    want = ref.centerline(free, free, res, origin, whole=False)[0]     # (the seed's component alone: the same loop, quickly)
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(img, res, origin)
    cells = s.centerline_cells(0)[0]
    s.close()
    assert len(cells) == 2397 and np.array_equal(cells, want)


@pytest.mark.parametrize("W", (64, 65, 127))
def test_word_size_widths_and_one_cell_corridor(amd, W):
    """rings that touch every border of a 40 x W table, and loops whose corridor is one cell wide"""
    wide = ref.rect_ring(0, 39, 0, W - 1, 5, H=40, W=W)
    narrow = ref.rect_ring(3, 36, 2, W - 3, 1, H=40, W=W)
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(wide, ref.RES, list(ref.ORIGIN))
    slot = s.add_map_image(narrow, ref.RES, list(ref.ORIGIN))
    for k, img, seed in ((0, wide, ref.cell_world(20, 2)), (slot, narrow, ref.cell_world(20, 2))):
        free = ref.free_from_image(img)
        T = ref.edt_table(free, ref.RES)
        want = ref.centerline(free, T, ref.RES, ref.ORIGIN, seed)
        mask, deleted = s.map_skeleton(k)
        cells, hw, deleted2 = s.centerline_cells(k, seed)
        assert np.array_equal(mask.astype(bool), want[3]) and np.array_equal(deleted, want[2]) and np.array_equal(deleted2, want[2])
        assert np.array_equal(cells, want[0]) and np.array_equal(hw, want[1])
        if k:
            assert deleted[0] == 0 and deleted[2] == 0 and len(cells) == 2 * (34 + W - 4) - 4 - 4     # only the four corners go
    s.close()


def test_derived_obstacle_slot(amd, world):
    s, slots = world
    base = slots["rect_w12"]
    seed = ref.fixture_seed("rect_w12")
    want = reference("rect_w12")[2]

    def box(r0, r1, c0, c1):
        """a box over the table cells rows r0 .. r1 - 1, columns c0 .. c1 - 1, its edges on cell boundaries"""
        return amd.Obstacles.boxes([(ref.ORIGIN[0] + 0.5 * (c0 + c1) * ref.RES, ref.ORIGIN[1] + 0.5 * (r0 + r1) * ref.RES)], 0.0, (c1 - c0) * ref.RES, (r1 - r0) * ref.RES)
    flush, mid = box(5, 11, 55, 75), box(9, 13, 60, 70)
    d = s.add_obstacle_map(flush, base)
    T = s.get_map_dt(d)
    assert np.array_equal(T[5:11, 55:75] > 0, np.zeros((6, 20), dtype=bool)) and (T > 0).sum() == (reference("rect_w12")[0]).sum() - 120
    got = s.centerline_cells(d, seed)
    exp = ref.centerline(T > 0, T, ref.RES, ref.ORIGIN, seed)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    assert np.array_equal(s.map_skeleton(d)[0].astype(bool), exp[3])
    rows = {int(c): int(r) for r, c in got[0] if r < 30}
    rows0 = {int(c): int(r) for r, c in want[0] if r < 30}
    assert all(rows[c] >= rows0[c] + 2 for c in range(58, 72))        # the line moved inward where the box narrows the corridor
    s.set_obstacles(d, mid)                                            # an island: two loops
    with pytest.raises(lib_error(amd), match="not a simple loop"):
        s.centerline_cells(d, seed)
    T = s.get_map_dt(d)
    with pytest.raises(ref.Refused) as ei:
        ref.centerline(T > 0, T, ref.RES, ref.ORIGIN, seed)
    assert ei.value.kind == 'not_simple'
    s.set_obstacles(d, None)
    back = s.centerline_cells(d, seed)
    for a, b in zip(back, want[:3]):
        assert np.array_equal(a, b)


def test_refusals_write_nothing_and_allocate_nothing(amd):
    f = amd._ffi
    img = FIX["annulus_w10"]
    seed = ref.fixture_seed("annulus_w10")
    live0 = amd.device_allocs()
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(img, ref.RES, list(ref.ORIGIN))
    eight = s.add_map_image(FIX["figure_eight"], ref.RES, list(ref.ORIGIN))
    straight = s.add_map_image(FIX["straight"], ref.RES, list(ref.ORIGIN))
    fresh = amd.device_allocs()

    def untouched(out, n_written=0):
        rc, n, c, w, d = out
        assert n == n_written and np.all(c == -7) and np.all(w == -7.0) and np.all(d == -7)
        return rc
    # refused up front: nothing launched, nothing allocated
    assert untouched(raw_call(amd, s, 0, seed, cells=False)) == f.ERR_INVALID and "null argument" in f.last_error(s._h)
    assert untouched(raw_call(amd, s, 0, seed, hw=False)) == f.ERR_INVALID
    assert untouched(raw_call(amd, s, 0, seed, deleted=False)) == f.ERR_INVALID
    assert untouched(raw_call(amd, s, 0, seed, n=False), -7) == f.ERR_INVALID
    assert f.lib().f110_map_centerline(None, 0, 0.0, 0.0, 0, 0.0, 0, None, None, 0, None, None) == f.ERR_INVALID
    for slot in (-1, 3, 99):
        assert untouched(raw_call(amd, s, slot, seed)) == f.ERR_INVALID and "maps are registered" in f.last_error(s._h)
    for bad in ((np.nan, 0.0), (0.0, np.inf), (-np.inf, 0.0)):
        assert untouched(raw_call(amd, s, 0, bad)) == f.ERR_INVALID and "not finite" in f.last_error(s._h)
    assert untouched(raw_call(amd, s, 0, seed, heading=np.nan)) == f.ERR_INVALID
    for outside in ((-3.0 - 1e-9, 0.0), (-3.0 + 130 * ref.RES, 0.0), (0.0, 100.0)):
        assert untouched(raw_call(amd, s, 0, outside)) == f.ERR_INVALID and "outside" in f.last_error(s._h)
    for occupied in (ref.cell_world(48, 64), ref.cell_world(2, 2)):
        assert untouched(raw_call(amd, s, 0, occupied)) == f.ERR_INVALID and "not free" in f.last_error(s._h)
    assert untouched(raw_call(amd, s, 0, seed, cap=-1)) == f.ERR_INVALID
    assert amd.device_allocs() == fresh
    with pytest.raises(ValueError, match="not free"):
        s.centerline_cells(0, ref.cell_world(48, 64))
    with pytest.raises(ValueError):
        s.map_skeleton(7)
    # a good call allocates the scratch once
    rc, n, c, w, d = raw_call(amd, s, 0, seed)
    assert rc == f.OK and n == 170
    warm = amd.device_allocs()
    assert warm[0] > fresh[0]
    # refused after the passes: nothing written but n, nothing allocated that a good call does not hold
    assert untouched(raw_call(amd, s, eight, ref.fixture_seed("figure_eight"))) == f.ERR_STATE and "not a simple loop" in f.last_error(s._h)
    assert untouched(raw_call(amd, s, straight, ref.fixture_seed("straight"))) == f.ERR_STATE and "no loop is reachable" in f.last_error(s._h)
    passes = ref.skeleton(ref.free_from_image(img))[2]
    assert untouched(raw_call(amd, s, 0, seed, max_passes=passes[0] - 1)) == f.ERR_STATE and "thinning has not converged" in f.last_error(s._h)
    assert raw_call(amd, s, 0, seed, max_passes=passes[0])[0] == f.OK       # the pass that deletes nothing included
    assert untouched(raw_call(amd, s, 0, seed, cap=169), 170) == f.ERR_INVALID and "cap = 169" in f.last_error(s._h)
    assert raw_call(amd, s, 0, seed, cap=170)[:2] == (f.OK, 170)
    assert amd.device_allocs() == warm
    # a second call on the same slot allocates nothing new, and gives the same answer
    again = raw_call(amd, s, 0, seed)
    assert amd.device_allocs() == warm
    assert np.array_equal(again[2], c) and np.array_equal(again[3], w) and np.array_equal(again[4], d)
    s.close()
    assert amd.device_allocs() == live0


def test_behind_steps_in_flight_on_both_env_blocks(amd):
    E, A = 4, 2
    img, res, origin = load_map_image("example_map")
    poses = bench_start_poses(E, A)
    rng = np.random.default_rng(3)
    acts = np.stack([rng.uniform(-0.2, 0.2, E * A), rng.uniform(0.5, 3.0, E * A)], axis=1)
    seed = ref.fixture_seed("annulus_w10")
    out = []
    for call in (False, True):
        s = amd.BatchSim(num_envs=E, num_agents=A, step_groups=2)
        s.set_map_image(img, res, origin)
        slot = s.add_map_image(FIX["annulus_w10"], ref.RES, list(ref.ORIGIN))
        idle = s.centerline_cells(slot, seed)
        s.reset(poses)
        d_act = s.device_array((E * A, 2))
        d_act.upload(acts)
        s.step_device(d_act)
        s.step_device(d_act)
        assert s.step_groups()[2] == 2
        if call:
            busy = s.centerline_cells(slot, seed)       # no sync in between: ordered behind both blocks by the library
            for a, b in zip(busy, idle):
                assert np.array_equal(a, b)
            assert np.array_equal(busy[0], reference("annulus_w10")[2][0])
        s.step_device(d_act)
        s.step_device(d_act)
        o = s.get("state", "scans", "collisions", "in_collision", "step_count")
        out.append({k: np.array(v, copy=True) for k, v in o.items()})
        d_act.free()
        s.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k      # nothing on the step path changed


def test_env_layers(amd):
    """track='centerline' on berlin: the progress of F110VecEnv equals that of the same env given Track.from_map's line; a 3-shard
    ShardedVecEnv equals one handle; F110Env takes it too"""
    E, A, T = 3, 1, 6
    stem = os.path.join(MAPS, "berlin")
    kw = dict(map=stem, map_ext=".png", num_agents=A, reward='progress')
    cl = dict(spacing=0.25, smooth=0.8)
    a = amd.F110VecEnv(E, device_logic=True, track='centerline', centerline=cl, **kw)
    track = a.tracks[0]
    line = amd.Track.from_map(a, 0, **cl)
    assert np.array_equal(line.xy, track.xy) and np.array_equal(line.attrs, track.attrs) and track.attr_names == ('half_width', 'kappa')
    assert track.closed and abs(track.length / track.num_points - 0.25) < 1e-3
    xy, tan = track.point_at(np.array([1.0, 20.0, 40.0]))
    poses = np.column_stack([xy, np.arctan2(tan[:, 1], tan[:, 0])]).reshape(E, A, 3)
    rng = np.random.default_rng(2)
    acts = np.stack([rng.uniform(-0.05, 0.05, (T, E, A)), rng.uniform(1.0, 4.0, (T, E, A))], axis=3)

    def run(env):
        rows = [np.array(env.reset(poses)[0]["progress"], copy=True)]
        rew = []
        for t in range(T):
            o, r = env.step(acts[t])[:2]
            rows.append(np.array(o["progress"], copy=True))
            rew.append(np.array(r, copy=True))
        return np.array(rows), np.array(rew)
    pa, ra = run(a)
    a.sim.batch.close()
    assert np.all(np.diff(pa[:, :, 0], axis=0) > 0) and np.all(ra[1:] > 0)          # the cars drive along the line, forwards
    assert np.allclose(pa[0, :, 0], [1.0, 20.0, 40.0], rtol=0, atol=1e-9)
    b = amd.F110VecEnv(E, device_logic=True, track=line, **kw)
    pb, rb = run(b)
    b.sim.batch.close()
    assert np.max(np.abs(pa - pb)) <= 1e-12 and np.max(np.abs(ra - rb)) <= 1e-12
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], track='centerline', centerline=cl, **kw)
    ps, rs = run(sh)
    sh.close()
    assert np.array_equal(ps, pa) and np.array_equal(rs, ra)
    with pytest.raises(ValueError, match="unknown parameter"):
        amd.F110VecEnv(E, device_logic=True, track='centerline', centerline=dict(sed=1), **kw)
    # a derived obstacle slot takes its own line (here: no obstacles, so the base's), an added map too
    two = amd.F110VecEnv(E, device_logic=True, extra_maps=[(stem + ".yaml", ".png")], obstacle_maps=[amd.Obstacles()], tracks={0: 'centerline', 1: 'centerline', 2: 'centerline'},
                         centerline=cl, **kw)
    assert two.obstacle_slots == {2: 0} and sorted(two.tracks) == [0, 1, 2]
    for k in (1, 2):
        assert two.tracks[k] is not two.tracks[0] and np.array_equal(two.tracks[k].xy, track.xy) and np.array_equal(two.tracks[k].attrs, track.attrs)
    two.sim.batch.close()
    one = amd.F110Env(map=stem, map_ext=".png", num_agents=1, track='centerline', centerline=cl, reward='progress')
    assert np.array_equal(one.track.xy, track.xy)
    one.sim.batch.close()
