"""Who owns device memory: every buffer a handle allocates is given back by close(), by the call that replaces it and by
the call that disarms its feature, a refused call allocates nothing that stays, and a unit call holds nothing once it has returned.  Held to f110_device_allocs, the process-wide
count of the library's live device allocations and their bytes: each test creates no handle but its own and compares readings it
took itself.  Memory the caller owns (DeviceArrays) is not counted.  Nothing here makes an allocation fail: the failure paths are
the CPU program's (tests/host_harness/devmem_harness.cpp)."""
import ctypes as C
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, A, B = 2, 2, 64
N = E * A
RES, ORIGIN = 0.25, (-6.0, -6.0, 0.0)
MPPI = dict(k=8, horizon=4)                                        # (w_progress is set by default: the planner projects onto the track)
PF = dict(particles=16, n_beams=8, beam_first=0, beam_stride=8)    # beams 0, 8 .. 56 of the 64


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _image(n=48):
    img = np.full((n, n), 255, dtype=np.uint8)   # free inside a wall of one cell
    img[0, :] = img[-1, :] = img[:, 0] = img[:, -1] = 0
    return img


def _track(amd, radius=3.0, attrs=True):
    th = np.arange(16) * (2.0 * np.pi / 16)
    xy = np.column_stack([radius * np.cos(th), radius * np.sin(th)])
    return amd.Track(xy, closed=True, attrs=np.column_stack([np.full(16, 1.0 / radius), np.full(16, 2.0)]) if attrs else None)


def _poses(radius=3.0):
    th = np.array([0.0, 0.6, 2.0, 2.6])   # two cars per env, a few metres apart on the circle, heading along it
    return np.column_stack([radius * np.cos(th), radius * np.sin(th), th + np.pi / 2])


def _obstacles(amd, x=0.0):
    return amd.Obstacles.boxes([[x, 0.0], [x, 1.0]], 0.3, 0.6, 0.4)


def _sim(amd):
    gc.collect()
    before = amd.device_allocs()
    return before, amd.BatchSim(num_envs=E, num_agents=A, num_beams=B)


def _with_map(amd):
    """a handle with the map, a second slot and the track on both"""
    before, b = _sim(amd)
    b.set_map_image(_image(), RES, ORIGIN)
    slot = b.add_map_image(_image(), RES, ORIGIN)
    b.set_track(_track(amd))
    b.set_track(_track(amd), slot=slot)
    b.reset(_poses())
    return before, b, slot


# ---- (a) everything armed, then close() ---------------------------------------------------------------------------------------------
def test_close_gives_back_every_allocation(amd):
    before, b, slot = _with_map(amd)
    assert amd.device_allocs()[0] > before[0] and amd.device_allocs()[1] > before[1]
    derived = b.add_obstacle_map(_obstacles(amd), base=0)   # (takes slot 0's track with it)
    b.set_env_maps([derived, slot])
    rng = np.random.default_rng(5)
    b.set_noise_table(rng.normal(0.0, 0.01, (32, B)))
    b.set_noise_rng(7, cache_rows=64)
    b.noise_prepare(64)
    b.set_noise_rng(None, per_agent_seeds=[11, 12, 13, 14])
    b.set_track_attrs(slot, np.ones((16, 1)))
    b.enable_track(True)
    b.episode_init(0)
    b.episode_reset(_poses())
    b.set_reset_sampler(3, gap=1.5)
    b.sample_reset()
    b.set_controllers([[0, -1], [0, -1]], [amd.GapFollower()])
    b.set_mppi(MPPI, agents=[1, 3], seed=9)
    b.set_particle_filter(PF, agents=[0, 2], seed=10)
    actions = np.tile([0.05, 1.5], (N, 1))
    b.step(actions)
    frames = b.render(width=16, height=16, layers="all")
    assert frames.shape == (N, 16, 16)
    summary = b.rollout(dict(k=4, horizon=4, channels=("alive", "progress")), np.tile([0.0, 1.0], (4, 4, 1)))
    assert summary.shape == (N, 4, 2) and np.all(np.isfinite(summary))
    blob = b.save_state(scans=True)
    b.step(actions)
    b.load_state(blob)
    assert b.mppi(actions).shape == (N, 2)
    pose, _ = b.localize()
    assert np.all(np.isfinite(pose[[0, 2]]))
    hb = b.host_block(("state", "scans", "done"))
    for _ in range(3):
        b.step(actions)
    b.step_host(hb, actions, scripted=True)
    assert np.all(np.isfinite(hb.views["scans"]))
    armed = amd.device_allocs()
    assert armed[0] > before[0] + 60, armed   # (the features above are several dozen buffers)
    b.close()
    del hb
    assert amd.device_allocs() == before


# ---- (b) a replacing call replaces, a disarming call gives back ---------------------------------------------------------------------------
def test_replacing_calls_do_not_accumulate_and_disarming_gives_back(amd):
    before, b, slot = _with_map(amd)
    live = lambda: amd.device_allocs()[0]

    def twice(call, what):
        call()
        once = amd.device_allocs()
        call()
        assert amd.device_allocs() == once, what
        return once

    twice(lambda: b.set_map_image(_image(), RES, ORIGIN), "set_map_image")
    b.reset(_poses())
    twice(lambda: b.set_track(_track(amd)), "set_track")
    twice(lambda: b.set_track_attrs(0, np.ones((16, 2))), "set_track_attrs")
    base = live()
    b.set_track_attrs(0, None)
    assert live() == base - 1
    derived = b.add_obstacle_map(_obstacles(amd), base=0)
    twice(lambda: b.set_obstacles(derived, _obstacles(amd, 0.5)), "set_obstacles")
    for arm, disarm, what in (
            (lambda: b.set_mppi(MPPI, agents=[1, 3]), b.clear_mppi, "set_mppi"),
            (lambda: b.set_particle_filter(PF, agents=[0, 2]), b.clear_particle_filter, "set_particle_filter"),
            (lambda: b.set_controllers([[0, -1], [0, -1]], [amd.GapFollower()]), b.clear_controllers, "set_controllers"),
            (lambda: b.set_reset_sampler(3), b.clear_reset_sampler, "set_reset_sampler"),
            (lambda: b.set_noise_rng(7, cache_rows=64), b.set_noise_off, "set_noise_rng")):
        arm()         # (the first arming of a planner or a filter also builds its jump constants, which stay)
        disarm()
        base = amd.device_allocs()
        assert twice(arm, what)[0] > base[0], what
        disarm()
        assert amd.device_allocs() == base, what
    b.close()
    assert amd.device_allocs() == before


# ---- (c) grow-only buffers grow in place ------------------------------------------------------------------------------------------------
def test_grow_only_buffers_grow_in_bytes_not_in_number(amd):
    before, b, slot = _with_map(amd)
    b.step(np.tile([0.0, 1.0], (N, 1)))

    def grows(small, big, what, bytes_grow=True):
        """small, big, small: the big call adds no buffer, only bytes, and the small one after it changes nothing"""
        small()
        first = amd.device_allocs()
        big()
        second = amd.device_allocs()
        assert second[0] == first[0] and (second[1] > first[1] if bytes_grow else second[1] == first[1]), (what, first, second)
        small()
        assert amd.device_allocs() == second, what

    # every agent's frame into rows that take 32-bit stores: the handle's own buffers hold per-frame records, not pixels
    grows(lambda: b.render(width=16, height=16), lambda: b.render(width=32, height=32), "render", bytes_grow=False)
    # an odd width renders through the staging copy, a list of agents through the agent list: both grow with the frames
    grows(lambda: b.render(agents=[0, 1], width=15, height=16), lambda: b.render(agents=[0, 1, 2, 3], width=31, height=32), "render, staged")
    # a subset's blob is the caller's memory, the handle allocates nothing for it; the whole handle's goes through the handle's own
    grows(lambda: b.save_envs([0]), lambda: b.save_envs([0, 1]), "save_envs", bytes_grow=False)
    grows(lambda: b.save_state(scans=False), lambda: b.save_state(scans=True), "save_state")
    roll = lambda k: b.rollout(dict(k=k, horizon=2, channels=("progress",)), np.tile([0.0, 1.0], (k, 2, 1)))
    grows(lambda: roll(2), lambda: roll(8), "rollout")
    b.close()
    assert amd.device_allocs() == before


# ---- (d) a refused call leaves nothing behind -----------------------------------------------------------------------------------------------
def test_refused_calls_do_not_leak(amd):
    from f1tenth_gym_amd import _ffi
    from f1tenth_gym_amd.reset_sampler import stream_words
    before, b, slot = _with_map(amd)
    b.set_mppi(MPPI, agents=[1, 3])
    b.set_particle_filter(PF, agents=[0, 2])
    armed = amd.device_allocs()
    L = _ffi.lib()
    words = np.ascontiguousarray(stream_words(0, 2, 0), dtype=np.uint64)
    wp = words.ctypes.data_as(_ffi._u64p)
    down = np.array([3, 1], dtype=np.int32)
    with pytest.raises(ValueError):
        b.set_mppi(MPPI, agents=down)
    msp = amd.Mppi(**MPPI).spec()
    assert L.f110_mppi_set(b._h, C.byref(msp), down.ctypes.data_as(_ffi._i32p), 2, wp) == _ffi.ERR_INVALID
    assert "ascending" in _ffi.last_error(b._h)
    with pytest.raises(ValueError):
        b.set_particle_filter(dict(PF, beam_first=60), agents=[0, 2])
    psp = amd.ParticleFilter(**dict(PF, beam_first=60)).spec()   # beam 60 + 7 * 8 of a scan of 64
    up = np.array([0, 2], dtype=np.int32)
    assert L.f110_pf_set(b._h, C.byref(psp), up.ctypes.data_as(_ffi._i32p), 2, wp) == _ffi.ERR_INVALID
    with pytest.raises(ValueError):
        b.add_map_image(np.zeros((0, 48), dtype=np.uint8), RES, ORIGIN)
    with pytest.raises(ValueError):
        b.add_map_image(_image(), 0.0, ORIGIN)
    assert amd.device_allocs() == armed
    assert b.get_mppi_state() is not None and b.localize()[0].shape == (N, 3)   # what was armed is as it was
    b.close()
    assert amd.device_allocs() == before


# ---- (e) a unit call holds nothing once it has returned -------------------------------------------------------------------------------------
def _unit_poses(m):
    th = np.linspace(0.3, 2.3, m)   # on the circle track, heading along it
    return np.column_stack([3.0 * np.cos(th), 3.0 * np.sin(th), th + np.pi / 2])


def _unit_forms(amd, b, m):
    """(name, call) for every unit form of the Python layer on m rows; each call returns the form's mandatory output"""
    from f1tenth_gym_amd import _ffi
    from f1tenth_gym_amd.reset_sampler import stream_words
    rng = np.random.default_rng(m)
    poses = _unit_poses(m)
    scans = rng.uniform(0.5, 8.0, (m, B))
    verts = np.array([[0.8, 0.15], [0.8, -0.15], [0.2, -0.15], [0.2, 0.15]])   # a car's corners ahead of the origin
    start = np.zeros((m, 10))
    start[:, 0], start[:, 1], start[:, 3], start[:, 4] = poses[:, 0], poses[:, 1], 1.0, poses[:, 2]
    first = lambda r: r[0] if isinstance(r, tuple) else r
    ro = amd.Rollout(k=4, horizon=4, channels=("alive", "progress"))
    acts = np.zeros(ro.actions_shape(m))
    acts[..., 1] = 1.0
    mp, pf = amd.Mppi(**MPPI), amd.ParticleFilter(**PF)
    words = np.ascontiguousarray(stream_words(3, max(m, 1))[:m], dtype=np.uint64)
    opp = np.tile([0.0, 3.0, 1.0, np.pi], (m, 1, 1))   # one opponent per row: x, y, v, theta
    cloud = poses[:, None, :] + rng.normal(0.0, 0.05, pf.cloud_shape(m))
    enc = amd.ObsEncoder(sectors=8, frames=2)
    wp = np.column_stack([_track(amd).xy, np.full(16, 2.0)])
    forms = [("scan_batch hits=%d lookups=%d" % (hits, lk), lambda hits=hits, lk=lk: first(b.scan_batch(poses, want_hits=hits, want_lookups=lk)))
             for hits in (False, True) for lk in (False, True)]
    forms += [
        ("pure_pursuit_batch", lambda: b.pure_pursuit_batch(wp, poses, 1.0, 1.0, 0.33)),
        ("noise_rows_batch", lambda: b.noise_rows_batch(7, max(m, 1))[0]),
        ("obs_encode_batch", lambda: b.obs_encode_batch(enc, scans, np.ones((m, 8)), np.arange(m), np.zeros(enc.shape(m), dtype=np.float32))),
        ("follow_gap", lambda: b.follow_gap(scans)),
        ("follow_gap info", lambda: b.follow_gap(scans, info=True)[0]),
        ("beam_dir_index_batch", lambda: b.beam_dir_index_batch(poses[:, 2])),
        ("dynamics_batch", lambda: b.dynamics_batch(np.ones((m, 7)), np.ones((m, 2)), amd.DEFAULT_PARAMS)[0]),
        ("pid_batch", lambda: b.pid_batch(np.ones((m, 4)), amd.DEFAULT_PARAMS)),
        ("update_pose_batch", lambda: b.update_pose_batch(np.ones((m, 7)), np.zeros((m, 2)), np.zeros(m, dtype=np.int32), np.ones((m, 2)),
                                                          amd.DEFAULT_PARAMS, 0.01, 1, 0.0)[0]),
        ("get_vertices_batch", lambda: b.get_vertices_batch(poses, 0.58, 0.31)),
        ("gjk_batch", lambda: b.gjk_batch(np.tile(verts, (m, 1, 1)), np.tile(verts + 0.1, (m, 1, 1)))),
        ("collision_multiple_batch", lambda: b.collision_multiple_batch(np.tile(verts, (m, 2, 1, 1)))[0]),
        ("ttc_batch", lambda: b.ttc_batch(scans, np.ones(m))),
        ("raycast_batch", lambda: first(b.raycast_batch(np.zeros((m, 3)), np.tile(verts, (m, 1, 1)), scans))),
        ("get_range_batch", lambda: b.get_range_batch(np.tile([0.0, 0.0, 0.1, 1.0, -1.0, 1.0, 1.0, 0.0], (m, 1)))),
        ("helper_batch, a map op", lambda: b.helper_batch(_ffi.OP_DISTANCE_TRANSFORM, poses[:, :2])),
        ("helper_batch, a body op", lambda: b.helper_batch(_ffi.OP_AVG_POINT, np.tile(verts.reshape(1, 8), (m, 1)), n=4)),
        ("track_project_batch", lambda: b.track_project_batch(poses)),
        ("track_preview", lambda: b.track_preview(poses, np.zeros(m), amd.TrackPreview(points=4))),
        ("neighbors", lambda: b.neighbors(np.column_stack([poses, np.ones(m), np.zeros(m)]), amd.Neighbors(k=2), m if m else 1)),
        ("rollout_rows", lambda: b.rollout_rows(ro, start, acts)),
        ("rollout_rows raw", lambda: b.rollout_rows(ro, start, acts, raw=True)[0]),
        ("rollout_opp_rows", lambda: b.rollout_opp_rows(ro, amd.Opponents(), start, acts, opp)["out"]),
        ("mppi_rows", lambda: b.mppi_rows(mp, start, mp.fresh_nominal(m), words)["actions"]),
        ("mppi_opp_rows", lambda: b.mppi_opp_rows(mp, amd.Opponents(), 1.0, 1.0, 0.5, start, mp.fresh_nominal(m), words, opp)["actions"]),
        ("localize_rows", lambda: b.localize_rows(pf, poses, scans, cloud, np.full((m, pf.particles), 1.0 / pf.particles), poses, words)["pose"]),
    ]
    if m:   # (an image has no empty form)
        forms += [("dt_from_bitmap", lambda: b.dt_from_bitmap(_image(8 * m), RES)), ("edt_sq", lambda: b.edt_sq(_image(8 * m) != 0))]
    return forms


def test_unit_calls_hold_nothing_once_returned(amd):
    from f1tenth_gym_amd import _ffi
    before, b, slot = _with_map(amd)
    bare = b.add_map_image(_image(), RES, ORIGIN)   # a slot without a track
    forms = _unit_forms(amd, b, 3)
    for name, call in forms:   # grow-only handle buffers and the planner's and the filter's jump constants settle
        call()
    held = amd.device_allocs()
    got = {}
    for name, call in forms:
        got[name] = call()
        assert amd.device_allocs() == held, name
    # the optional outputs do not change the mandatory ones
    same = lambda x, y: x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes()
    for name in ("scan_batch hits=0 lookups=1", "scan_batch hits=1 lookups=0", "scan_batch hits=1 lookups=1"):
        assert same(got[name], got["scan_batch hits=0 lookups=0"]), name
    assert same(got["follow_gap info"], got["follow_gap"])
    assert same(got["rollout_rows raw"], got["rollout_rows"])
    # an empty batch returns empty and allocates nothing
    for name, call in _unit_forms(amd, b, 0):
        if name.split()[0] in ("scan_batch", "dynamics_batch", "track_project_batch", "rollout_rows"):
            assert call().shape[0] == 0 and amd.device_allocs() == held, name
    # a call refused behind the handle's entry leaves nothing behind, and the handle works as before
    poses = _poses()[:3]
    with pytest.raises(SyntaxError):
        b.update_pose_batch(np.ones((3, 7)), np.zeros((3, 2)), np.zeros(3, dtype=np.int32), np.ones((3, 2)), amd.DEFAULT_PARAMS, 0.01, 99, 0.0)
    assert amd.device_allocs() == held
    rows, out = np.ones((3, 2)), np.zeros((3, 2))
    assert _ffi.lib().f110_helper_batch(b._h, 9999, _ffi.dptr(rows), 3, 4, _ffi.dptr(out)) == _ffi.ERR_INVALID
    assert "unknown op" in _ffi.last_error(b._h) and amd.device_allocs() == held
    with pytest.raises(_ffi.F110LibraryError, match="has no track"):
        b.track_project_batch(poses, slot=bare)
    assert amd.device_allocs() == held
    assert same(b.scan_batch(_unit_poses(3)), got["scan_batch hits=0 lookups=0"])
    assert amd.device_allocs() == held
    b.close()
    assert amd.device_allocs() == before
