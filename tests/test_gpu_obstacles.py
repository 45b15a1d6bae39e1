"""Static obstacles stamped into a derived map slot on the device (f110_add_map_obstacles / f110_set_map_obstacles)
against the NumPy model tests/obstacles_ref.py: the tables bit for bit (and against a slot made from the image with the stamped cells
blacked out), stepping on both kinds of slot, the in-place re-stamp, its ordering behind and in front of two-block steps, the reset
sampler on a derived slot, an untouched step path, every refusal, and the env layers."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import obstacles_ref as ref
from _util import MAPS, bench_start_poses, load_map_image
from reset_sampler_ref import SamplerModel, SlotModel

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSV = os.path.join(MAPS, "example_waypoints.csv")
CLEAR = float(np.sqrt(0.58 ** 2 + 0.31 ** 2) / 2)   # the sampler's default clearance: half a car's diagonal


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _fixture(name):
    """(image, resolution, origin, obstacle lists) of the small or the large fixture"""
    if name == "small":
        return ref.small_image(), ref.SMALL_RES, list(ref.SMALL_ORIGIN), [ref.small_obstacles(0), ref.small_obstacles(1)]
    img, res, origin = load_map_image("example_map")
    return img, res, origin, [ref.large_obstacles(), ref.large_obstacles(seed=4)]


_model_cache = {}


def _model(name, which):
    """(model table, stamp mask, base table) — computed once per fixture and list, shared, never written to"""
    key = (name, which)
    if key not in _model_cache:
        img, res, origin, lists = _fixture(name)
        base = ref.table_from_bitmap(ref.free_from_image(img), res)
        t, m = ref.derived_table(base, lists[which], res, origin)
        for a in (t, m, base):
            a.setflags(write=False)
        _model_cache[key] = (t, m, base)
    return _model_cache[key]


def _sim(amd, name, E=1, A=2, **kw):
    img, res, origin, _ = _fixture(name)
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(img, res, origin)
    return s


def _obs(s):
    o = s.get("state", "scans", "collisions", "in_collision", "step_count")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def _same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s %s differs" % (what, k)


# ---- 1. tables -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "example_map"])
def test_tables_equal_model_and_image_made_slot(amd, name):
    img, res, origin, lists = _fixture(name)
    H, W = img.shape
    ob = lists[0]
    assert ref.boundary_margin(ob, H, W, res, origin) > 1e-9
    want, mask, base = _model(name, 0)
    s = _sim(amd, name)
    base_dev = s.get_map_dt()
    assert np.array_equal(base_dev, base)
    other = s.add_map_image(np.flipud(img), res, origin)          # an unrelated slot that must stay as it is
    other_dt = s.get_map_dt(other)
    d = s.add_obstacle_map(ob)
    im = s.add_map_image(ref.image_with_stamps(img, mask), res, origin)
    copy = s.add_obstacle_map(None, base=other)                   # n = 0: a copy of its base
    assert (other, d, im, copy) == (1, 2, 3, 4)
    got = s.get_map_dt(d)
    assert got.shape == (H, W) and np.array_equal(got, want)
    assert np.array_equal(got, s.get_map_dt(im))
    assert int((got != base).sum()) > 200
    assert np.array_equal(s.get_map_dt(copy), other_dt)
    assert np.array_equal(s.get_map_dt(0), base_dev) and np.array_equal(s.get_map_dt(), base_dev) and np.array_equal(s.get_map_dt(other), other_dt)
    if name == "small":   # the far corner cell is stamped: the out-of-bounds value changed with it
        assert got[H - 1, W - 1] == 0.0 and base[H - 1, W - 1] > 0.0
    s.close()


# ---- 2. stepping ------------------------------------------------------------------------------------------------------------
def _corridor_pose(phi, heading_offset=0.0):
    """a pose on the small fixture's corridor at ring angle phi, heading along the ring (counter-clockwise in the table)"""
    r, c = 48.0 + 26.3 * np.sin(phi), 64.0 + 38.0 * np.cos(phi)
    x, y = ref.small_cell_xy(r, c)
    th = np.arctan2(26.3 * np.cos(phi), -38.0 * np.sin(phi)) + ref.SMALL_ORIGIN[2]   # d(c, r)/dphi, rotated into the world
    return [x, y, th + heading_offset]


def _small_poses():
    """[4][2][3]: env 0 holds the car that drives into obstacle 0 (the box at cell (50.3, 26.2)) and the car in the corner patch
    whose rays leave the map; the others sit on the corridor"""
    yaw = ref.SMALL_ORIGIN[2]
    hx, hy = ref.small_cell_xy(38.0, 26.5)
    kx, ky = ref.small_cell_xy(89.0, 119.0)
    poses = np.empty((4, 2, 3))
    poses[0, 0] = (hx, hy, yaw + np.pi / 2)          # towards +row: the box is 12 cells ahead
    poses[0, 1] = (kx, ky, yaw + np.pi / 4)          # towards the far corner: every ray leaves the table
    for e in range(1, 4):
        poses[e, 0] = _corridor_pose(0.9 * e + 0.2)
        poses[e, 1] = _corridor_pose(0.9 * e + 3.4, 0.1)
    return poses


def test_stepping_on_derived_and_image_made_slots_is_identical(amd):
    img, res, origin, lists = _fixture("small")
    _, mask, _ = _model("small", 0)
    E, A, T = 8, 2, 40
    s = _sim(amd, "small", E, A)
    d = s.add_obstacle_map(lists[0])
    im = s.add_map_image(ref.image_with_stamps(img, mask), res, origin)
    s.set_env_maps([d] * 4 + [im] * 4)
    poses = np.concatenate([_small_poses(), _small_poses()]).reshape(E * A, 3)
    s.reset(poses)
    rng = np.random.default_rng(5)
    hit = False
    for t in range(T):
        half = np.stack([rng.uniform(-0.2, 0.2, (4, A)), rng.uniform(0.5, 2.0, (4, A))], axis=2)
        half[0, 0] = (0.0, 3.0)      # straight into the box
        half[0, 1] = (0.0, 0.0)
        s.step(np.concatenate([half, half]).reshape(E * A, 2))
        o = _obs(s)
        for k, v in o.items():
            v = v.reshape((E, A) + v.shape[1:])
            assert np.array_equal(v[:4], v[4:], equal_nan=True), "step %d: %s differs between the derived and the image-made slot" % (t, k)
        hit = hit or bool(o["collisions"].reshape(E, A)[0, 0] > 0)
        if t == 0:   # the corner car's rays leave the table; the stamped corner cell makes the out-of-bounds value 0, so they end there
            sc = o["scans"].reshape(E, A, -1)[0, 1]
            assert sc.max() < 2.0
    assert hit, "the car that drives into the box never raised its collision flag"
    # the same car on the base slot drives through: the box is what stopped it
    b = _sim(amd, "small", 4, A)
    b.reset(_small_poses().reshape(4 * A, 3))
    rng = np.random.default_rng(5)
    free_run = False
    for t in range(T):
        half = np.stack([rng.uniform(-0.2, 0.2, (4, A)), rng.uniform(0.5, 2.0, (4, A))], axis=2)
        half[0, 0] = (0.0, 3.0)
        half[0, 1] = (0.0, 0.0)
        b.step(half.reshape(4 * A, 2))
        free_run = free_run or bool(b.get("collisions")["collisions"].reshape(4, A)[0, 0] > 0)
    assert not free_run
    s.close()
    b.close()


# ---- 3. re-stamp ------------------------------------------------------------------------------------------------------------
def test_restamp_in_place(amd):
    img, res, origin, lists = _fixture("small")
    E, A = 2, 2
    s = _sim(amd, "small", E, A)
    d = s.add_obstacle_map(lists[0])
    s.set_env_maps([d, d])
    s.reset(_small_poses()[:2].reshape(E * A, 3))
    s.step(np.zeros((E * A, 2)))
    addr = s.map_table_address(d)
    view = dict(agents=[0, 1], width=96, height=96, view="world", m_per_px=0.08, center=ref.small_cell_xy(48.0, 64.0), angle=0.0, layers=("map",))
    before = s.render(**view)
    want1, mask1, base = _model("small", 1)
    s.set_obstacles(d, lists[1])
    assert np.array_equal(s.get_map_dt(d), want1)
    assert s.map_table_address(d) == addr
    after = s.render(**view)
    assert not np.array_equal(before, after)
    im = s.add_map_image(ref.image_with_stamps(img, mask1), res, origin)
    s.set_env_maps([im, im])
    assert np.array_equal(s.render(**view), after)
    s.set_env_maps([d, d])
    for _ in range(3):   # again and again: the same table, the same address
        s.set_obstacles(d, lists[0])
        s.set_obstacles(d, lists[1])
    assert np.array_equal(s.get_map_dt(d), want1) and s.map_table_address(d) == addr
    s.set_obstacles(d, None)
    assert np.array_equal(s.get_map_dt(d), base) and s.map_table_address(d) == addr
    assert np.array_equal(s.get_map_dt(0), base)
    s.set_env_maps([0, 0])
    plain = s.render(**view)
    s.set_env_maps([d, d])
    assert np.array_equal(s.render(**view), plain)
    s.close()


# ---- 4. ordering ------------------------------------------------------------------------------------------------------------
def test_restamp_is_ordered_between_two_block_steps(amd):
    img, res, origin, lists = _fixture("small")
    E, A = 256, 2
    rng = np.random.default_rng(2)
    poses = np.array([[_corridor_pose(p), _corridor_pose(p + 0.6, 0.05)] for p in rng.uniform(0, 2 * np.pi, E)]).reshape(E * A, 3)
    acts = np.stack([rng.uniform(-0.2, 0.2, E * A), rng.uniform(0.5, 3.0, E * A)], axis=1)
    out = []
    for synced in (False, True):
        s = _sim(amd, "small", E, A, step_groups=2)
        d = s.add_obstacle_map(lists[0])
        s.set_env_maps([d if e % 2 else 0 for e in range(E)])
        s.reset(poses)
        d_act = s.device_array((E * A, 2))
        d_act.upload(acts)
        s.step_device(d_act)          # (the first step after a reset forks from the main stream)
        s.step_device(d_act)
        if synced:
            s.sync()
        assert s.step_groups()[2] == 2
        s.set_obstacles(d, lists[1])
        if synced:
            s.sync()
        s.step_device(d_act)
        assert s.step_groups()[2] == 2
        if synced:
            s.sync()
        s.set_obstacles(d, lists[0])
        s.step_device(d_act)
        out.append(_obs(s))
        assert np.array_equal(s.get_map_dt(d), _model("small", 0)[0])
        d_act.free()
        s.close()
    _same(out[0], out[1], "unsynchronised against synchronised:")
    # and the re-stamp mattered: the same sequence without it ends elsewhere
    s = _sim(amd, "small", E, A, step_groups=2)
    d = s.add_obstacle_map(lists[1])
    s.set_env_maps([d if e % 2 else 0 for e in range(E)])
    s.reset(poses)
    for _ in range(4):
        s.step(acts)
    assert not np.array_equal(_obs(s)["scans"], out[0]["scans"])
    s.close()


# ---- 5. reset sampler -------------------------------------------------------------------------------------------------------
def test_reset_sampler_reads_the_derived_table(amd):
    img, res, origin, lists = _fixture("example_map")
    want, _, base = _model("example_map", 0)
    track = ref.example_track()
    E, A = 256, 1
    base_slot, der_slot = SlotModel(track, base, res, origin), SlotModel(track, want, res, origin)

    def clearances(slot, poses):
        return np.array([slot.dt[slot.rc(x, y)] for x, y, _ in poses.reshape(-1, 3)])
    # a seed (found on the CPU model) whose draws on the BASE slot put at least one start where the derived table is too close
    for seed in range(100):
        m = SamplerModel(seed, E, A, [base_slot], clearance=CLEAR)
        on_base = np.array([m.draw(e)[0] for e in range(E)])
        if np.any(clearances(der_slot, on_base) < CLEAR):
            break
    else:
        raise AssertionError("no seed below 100 draws a start on an obstacle")
    s = _sim(amd, "example_map", E, A)
    s.set_track(track)
    d = s.add_obstacle_map(lists[0])
    s.set_reset_sampler(seed=seed)
    s.sample_reset()
    p0 = s.reset_sampler_poses()
    assert s.reset_sampler_stats()["fallbacks"] == 0
    assert np.array_equal(p0.reshape(-1, 3)[:, :2], on_base.reshape(-1, 3)[:, :2])
    assert np.any(clearances(der_slot, p0) < CLEAR) and np.all(clearances(base_slot, p0) >= CLEAR)
    s.set_env_maps([d] * E)
    s.set_reset_sampler(seed=seed)
    s.sample_reset()
    p1 = s.reset_sampler_poses()
    assert s.reset_sampler_stats()["fallbacks"] == 0
    assert np.all(clearances(der_slot, p1) >= CLEAR)
    md = SamplerModel(seed, E, A, [der_slot], clearance=CLEAR)
    assert np.array_equal(p1.reshape(-1, 3)[:, :2], np.array([md.draw(e)[0] for e in range(E)]).reshape(-1, 3)[:, :2])
    s.close()


# ---- 6. untouched step path ---------------------------------------------------------------------------------------------------
def _blob_payload(raw, N, B):
    """the defined bytes of a whole-handle blob with the agent columns, a shared noise stream and the scans (include/f110.h: a
    256-byte header, then one section per column, each 256-byte aligned): the header and every section without the alignment
    padding behind it, which the format leaves unspecified"""
    widths = [8] * 7 + [8] * 2 + [4] + [8] * 3 + [8, 8, 4, 4] + [16] + [8 * B]   # state, steer FIFO, count, agent_poses, flags, step_count, stream, scans
    parts, off = [raw[:256]], 256
    for w in widths:
        parts.append(raw[off:off + N * w])
        off += (N * w + 255) // 256 * 256
    assert off == len(raw), "the blob has sections this test does not know"
    return b"".join(parts)


@pytest.mark.parametrize("E", [1, 48])
def test_unused_derived_slot_changes_nothing(amd, E):
    A, T = 2, 100
    sims = [_sim(amd, "example_map", E, A) for _ in range(2)]
    sims[1].add_obstacle_map(ref.large_obstacles())
    poses = bench_start_poses(E, A)
    rng = np.random.default_rng(8)
    acts = np.stack([rng.uniform(-0.3, 0.3, (T, E * A)), rng.uniform(1.0, 6.0, (T, E * A))], axis=2)
    for s in sims:
        s.set_noise_rng(4242, 0.01)
        s.reset(poses)
    for t in range(T):
        for s in sims:
            s.step(acts[t])
        assert sims[0].step_launches() == sims[1].step_launches()
        if t % 10 == 9:
            _same(_obs(sims[0]), _obs(sims[1]), "step %d" % t)
    blobs = [_blob_payload(s.save_state().to_bytes(), E * A, 1080) for s in sims]
    assert blobs[0] == blobs[1], "the state blobs differ"
    for s in sims:
        s.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(amd):
    from f1tenth_gym_amd import _ffi
    L = _ffi.lib()
    img, res, origin, lists = _fixture("small")
    s = _sim(amd, "small", 1, 2)
    plain = s.add_map_image(img, res, origin)
    d = s.add_obstacle_map(lists[0])
    want = s.get_map_dt(d)
    assert np.array_equal(want, _model("small", 0)[0])
    slot = C.c_int32(-5)
    good = lists[1].structs()
    n = len(lists[1])

    def one(**kw):
        arr = (_ffi.Obstacle * 1)()
        arr[0].shape, arr[0].x, arr[0].y, arr[0].c, arr[0].s, arr[0].half_length, arr[0].half_width = 0, 0.5, 0.5, 1.0, 0.0, 0.2, 0.1
        for k, v in kw.items():
            setattr(arr[0], k, v)
        return arr
    bad_lists = [one(shape=2), one(shape=-1), one(x=float("nan")), one(y=float("inf")), one(c=float("nan")), one(s=float("-inf")),
                 one(half_length=float("nan")), one(half_width=float("inf")), one(half_length=-0.1), one(half_width=-1e-9)]
    calls = [("null handle add", lambda: L.f110_add_map_obstacles(None, 0, good, n, C.byref(slot))),
             ("null slot pointer", lambda: L.f110_add_map_obstacles(s._h, 0, good, n, None)),
             ("null list add", lambda: L.f110_add_map_obstacles(s._h, 0, None, 3, C.byref(slot))),
             ("null handle set", lambda: L.f110_set_map_obstacles(None, d, good, n)),
             ("null list set", lambda: L.f110_set_map_obstacles(s._h, d, None, 3)),
             ("base out of range", lambda: L.f110_add_map_obstacles(s._h, 9, good, n, C.byref(slot))),
             ("base negative", lambda: L.f110_add_map_obstacles(s._h, -1, good, n, C.byref(slot))),
             ("derived base", lambda: L.f110_add_map_obstacles(s._h, d, good, n, C.byref(slot))),
             ("set on slot 0", lambda: L.f110_set_map_obstacles(s._h, 0, good, n)),
             ("set on a plain slot", lambda: L.f110_set_map_obstacles(s._h, plain, good, n)),
             ("set out of range", lambda: L.f110_set_map_obstacles(s._h, 9, good, n)),
             ("set negative slot", lambda: L.f110_set_map_obstacles(s._h, -1, good, n)),
             ("n < 0 add", lambda: L.f110_add_map_obstacles(s._h, 0, good, -1, C.byref(slot))),
             ("n < 0 set", lambda: L.f110_set_map_obstacles(s._h, d, good, -1)),
             ("n > 256 add", lambda: L.f110_add_map_obstacles(s._h, 0, good, 257, C.byref(slot))),
             ("n > 256 set", lambda: L.f110_set_map_obstacles(s._h, d, good, 257)),
             ("get null", lambda: L.f110_get_slot_dt(s._h, d, None)),
             ("get out of range", lambda: L.f110_get_slot_dt(s._h, 9, want.ctypes.data_as(_ffi._dp))),
             ("shape out of range", lambda: L.f110_slot_shape(s._h, 9, None, None))]
    for i, arr in enumerate(bad_lists):
        calls.append(("bad field %d add" % i, lambda arr=arr: L.f110_add_map_obstacles(s._h, 0, arr, 1, C.byref(slot))))
        calls.append(("bad field %d set" % i, lambda arr=arr: L.f110_set_map_obstacles(s._h, d, arr, 1)))
    keep = want.copy()
    for what, call in calls:
        rc = call()
        assert rc == _ffi.ERR_INVALID, (what, rc)
        assert _ffi.last_error(None if "null handle" in what else s._h), what
    assert slot.value == -5 and np.array_equal(want, keep)
    assert np.array_equal(s.get_map_dt(d), want) and np.array_equal(s.get_map_dt(plain), s.get_map_dt(0))
    with pytest.raises(ValueError):
        s.add_obstacle_map(lists[0], base=d)
    with pytest.raises(ValueError):
        s.set_obstacles(plain, lists[0])
    # the next slot number shows that no refused call registered anything
    assert s.add_obstacle_map(None) == d + 1
    # a base whose shape no longer matches: slot 0 re-set to another map since
    s.set_map_image(np.full((40, 50), 255, dtype=np.uint8), res, origin)
    rc = L.f110_set_map_obstacles(s._h, d, good, n)
    assert rc == _ffi.ERR_STATE and "derived from a 96 x 128 base" in _ffi.last_error(s._h)
    assert np.array_equal(s.get_map_dt(d), want)
    s.close()


# ---- 8. env layers ----------------------------------------------------------------------------------------------------------
def _pose_before(ob, i, dist=2.0):
    """a pose on the example raceline `dist` metres before obstacle i, heading along the track: the obstacle is in its scan"""
    track = ref.example_track()
    s = float(track.project(np.array([[ob.xy[i, 0], ob.xy[i, 1], 0.0]]))[0, 0])
    p, tan = track.point_at([s - dist])
    return (p[0, 0], p[0, 1], np.arctan2(tan[0, 1], tan[0, 0]))


def _vec_kwargs():
    return dict(map=os.path.join(MAPS, "example_map"), map_ext=".png", num_agents=2, track=CSV)


def test_vec_env_and_sharded_env_against_batchsim_level(amd):
    E, A, T = 4, 2, 20
    ob, ob2 = ref.large_obstacles(), ref.large_obstacles(seed=4)
    env_map = [1, 1, 0, 1]
    poses = bench_start_poses(E, A).reshape(E, A, 3)
    poses[0, 0] = _pose_before(ob, 0)   # env 0's ego just in front of the first obstacle
    rng = np.random.default_rng(1)
    acts = np.stack([rng.uniform(-0.1, 0.1, (T, E, A)), rng.uniform(1.0, 5.0, (T, E, A))], axis=3)
    keys = ("scans", "poses_x", "poses_y", "poses_theta", "collisions", "progress")

    def run(env, restamp):
        rows = []
        o = env.reset(poses)[0]
        rows.append({k: np.array(o[k], copy=True) for k in keys})
        for t in range(T):
            if t == 10:
                restamp(env)
            o = env.step(acts[t])[0]
            rows.append({k: np.array(o[k], copy=True) for k in keys})
        return rows
    a = amd.F110VecEnv(E, device_logic=True, obstacle_maps=[ob], env_map=env_map, **_vec_kwargs())
    assert a.obstacle_slots == {1: 0} and a.tracks[1] is a.tracks[0]
    ra = run(a, lambda env: env.set_obstacles(1, ob2))
    a.sim.batch.close()
    b = amd.F110VecEnv(E, device_logic=True, **_vec_kwargs())
    assert b.sim.batch.add_obstacle_map(ob) == 1
    b.set_env_maps(env_map)
    rb = run(b, lambda env: env.sim.batch.set_obstacles(1, ob2))
    b.sim.batch.close()
    for t, (x, y) in enumerate(zip(ra, rb)):
        _same(x, y, "vec env, step %d:" % t)
    plain = amd.F110VecEnv(E, device_logic=True, **_vec_kwargs())
    rp = run(plain, lambda env: None)
    plain.sim.batch.close()
    assert not np.array_equal(rp[-1]["scans"], ra[-1]["scans"])
    sh = amd.ShardedVecEnv(E, devices=[0, 0], obstacle_maps=[ob], env_map=env_map, **_vec_kwargs())
    rs = run(sh, lambda env: env.set_obstacles(1, ob2))
    sh.close()
    for t, (x, y) in enumerate(zip(ra, rs)):
        _same(x, y, "sharded env, step %d:" % t)


def test_single_env_with_obstacles(amd):
    ob = ref.large_obstacles()
    kw = dict(map=os.path.join(MAPS, "example_map"), map_ext=".png", num_agents=1)
    start = np.array([_pose_before(ob, 0)])
    e = amd.F110Env(obstacles=ob, **kw)
    assert e.obstacle_slot == 1
    assert np.array_equal(e.sim.batch.get_map_dt(1), _model("example_map", 0)[0])
    o1 = e.reset(start)[0]
    e.set_obstacles(None)
    o2 = e.reset(start)[0]
    p = amd.F110Env(**kw)
    o3 = p.reset(start)[0]
    assert np.array_equal(o2["scans"], o3["scans"]) and not np.array_equal(o1["scans"], o3["scans"])
    p.set_obstacles(ob)
    assert np.array_equal(p.reset(start)[0]["scans"], o1["scans"])
    e.sim.batch.close()
    p.sim.batch.close()


def test_example_runs():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "obstacles.py"), "--envs", "64", "--steps", "50", "--redraw", "20"],
                          stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout
    assert "collisions per lap" in proc.stdout
