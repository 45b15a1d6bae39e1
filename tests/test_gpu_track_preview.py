"""The track preview on the device (f110_track_set_attrs, f110_track_preview_*) against the NumPy model
tests/track_preview_ref.py with the assertions of the host tests (ref.compare): WORLD frame bit for bit; EGO frame the segments and
attribute channels bit for bit, the rotated channels within 8 eps (|rx| + |ry|) resp. 8 eps, every float32 output the model's or
its neighbour and at most 1 in 1000 different.  The unit form over the grid of the host tests, the device form through noisy steps
with in-step re-seats, two map slots, env blocks, no effect on the step, the refusals, the pinned copy, DLPack, the env layers.

The pose a preview belongs to is the observation's (agent_poses, the one no in-step re-seat overwrites, the pose `s` was computed
from); the poses_x / poses_y / poses_theta columns read the live state and equal it for every agent that was not re-seated in the
step, but for the heading of a car that hit a wall in it (check_ttc zeroes state[3:] behind the observation), which the device-form
test also holds."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import track_preview_ref as ref
from _util import MAPS, bench_start_poses, load_map_image, map_stem

pytestmark = pytest.mark.gpu

SEED, STD = 4242, 0.01
CSV = os.path.join(MAPS, "example_waypoints.csv")
ALL8 = ref.CHANNELS
SCALE = {"x": 10.0, "y": -4.0, "tan_x": 0.5, "attr0": 3.0, "attr3": 7.0}


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def race():
    """the example raceline with 4 attributes: the model's tables, the points and the attribute rows as given"""
    return ref.example_raceline(True, 4)


def _track(amd, xy, closed, attrs):
    return amd.Track(xy, closed=closed, attrs=attrs)


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs hit the walls within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


def _sim(amd, E, A, track, noise=True, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    if noise:
        s.set_noise_rng(SEED, STD)
    if track is not None:
        s.set_track(track)
        s.enable_track()
    return s


def _armed(s, E, A):
    start = bench_start_poses(E, A)
    s.reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    s.set_auto_reseat(d_start, 0)
    d_act = s.device_array((E * A, 2))
    s._keep = (d_start, d_act)   # (the armed re-seat reads d_start: it lives with the handle)
    return d_act


def _pose_and_s(s):
    return np.array(s.get("agent_poses")["agent_poses"], copy=True), np.array(s.get_track()["s"], copy=True)


def _model_settings(p):
    return ref.settings(**p.settings())


def _check_device(tab, p, poses, arc, out, what):
    """the device form has no raw values: WORLD bit for bit; EGO the float32 outputs the model's or its neighbour, at most 1 in
    1000 different, attribute channels bit for bit"""
    s = _model_settings(p)
    want, raw, _ = ref.preview(tab, s, poses, arc)
    if p.frame == "world":
        assert np.array_equal(ref.bits(out), ref.bits(want)), "%s: WORLD outputs differ" % what
        return 0
    cols = [i for i, c in enumerate(p.channels) if c.startswith("attr")]
    assert np.array_equal(ref.bits(out[..., cols]), ref.bits(want[..., cols])), "%s: attribute channels differ" % what
    steps = ref.f32_steps(out, want)
    assert steps.max(initial=0) <= 1, "%s: a float32 output is %d values away from the model's" % (what, int(steps.max()))
    return int(np.count_nonzero(steps))


# ---- the unit form over the grid -----------------------------------------------------------------------------------------------
def test_unit_form_matches_model_over_the_grid(amd):
    rng = np.random.default_rng(32)
    s = amd.BatchSim(num_envs=1, num_agents=1)        # (no map: a unit entry point)
    total = differ = 0
    last = None
    for k, case in enumerate(ref.unit_grid()):
        name, make, closed, attrs, P, frame, channels = case
        tab, xy, a = make(closed=closed, attrs=attrs)
        st = ref.grid_settings(name, tab, P, frame, channels, k)
        poses, arc = ref.poses_near(tab, rng, 8, spread=0.2 if name == "square" else 0.4)
        if k % 5 == 0:
            poses[0], arc[0] = np.nan, np.nan
        if last != (name, closed, attrs):
            s.set_track(_track(amd, xy, closed, a))
            last = (name, closed, attrs)
        got = s.track_preview(poses, arc, amd.TrackPreview(**st), raw=True, segments=True)
        differ += ref.compare(tab, st, poses, arc, got, "%s closed=%r attrs=%d %r" % (name, closed, attrs, st))
        total += got[0].size
    assert total > 30000 and differ * 1000 <= total, (total, differ)
    # more rows than a workgroup holds groups, P = 32 and P = 1, without raw and segments
    tab, xy, a = ref.example_raceline(True, 2)
    s.set_track(_track(amd, xy, True, a))
    poses, arc = ref.poses_near(tab, rng, 70)
    for P in (32, 1):
        p = amd.TrackPreview(points=P, channels=("x", "y", "attr1"), frame="world")
        out = s.track_preview(poses, arc, p)
        assert np.array_equal(ref.bits(out), ref.bits(ref.preview(tab, _model_settings(p), poses, arc)[0])), P
    s.close()


# ---- the device form through noisy steps with in-step re-seats -----------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 3])
def test_device_form_follows_model_through_reseats(amd, race, A):
    tab, xy, attrs = race
    E, T = 64, 150
    N = E * A
    s = _sim(amd, E, A, _track(amd, xy, True, attrs))
    d_act = _armed(s, E, A)
    acts = _crash_actions(T, N)
    world = amd.TrackPreview(points=8, offset=0.5, spacing=0.5, channels=ALL8, frame="world", scale=SCALE)
    ego = amd.TrackPreview(points=5, offset=0.0, spacing=0.8, channels=ALL8, frame="ego", scale=SCALE)
    bufs = {}
    fresh = total = differ = reseat_steps = 0
    for t in range(T):
        d_act.upload(acts[t])
        s.step_device(d_act)
        # the sample: every tenth step, the last one, and the first six steps in which some env was re-seated
        o = s.get("poses_x", "poses_y", "poses_theta", "step_count", "in_collision")
        seated = o["step_count"] == 0                         # re-seated inside this step: the live state is the new start pose
        hit = o["in_collision"] != 0                          # a wall hit: check_ttc zeroed the live heading behind the observation's
        take_reseat = bool(seated.any()) and reseat_steps < 6
        if not (t % 10 == 3 or t == T - 1 or take_reseat):
            continue
        reseat_steps += int(take_reseat)
        for p in (world, ego):
            bufs[p] = s.track_preview_device(p, bufs.get(p))
        poses, arc = _pose_and_s(s)
        live = np.column_stack([o["poses_x"], o["poses_y"], o["poses_theta"]])
        assert np.array_equal(live[~seated, :2], poses[~seated, :2])
        assert np.array_equal(live[~seated & ~hit, 2], poses[~seated & ~hit, 2]) and not live[~seated & hit, 2].any()
        fresh += int(np.sum(seated))
        for p in (world, ego):
            differ += _check_device(tab, p, poses, arc, bufs[p].download(), "A=%d step %d %s" % (A, t, p.frame))
        total += N * ego.points * ego.dim
    assert fresh >= A, "no env was re-seated in a sampled step (%d agents)" % fresh
    assert differ * 1000 <= total, (differ, total)
    s.close()


# ---- two map slots ------------------------------------------------------------------------------------------------------------------
def test_every_agent_gets_its_own_slots_stations(amd, race):
    _two_slots(amd, race, "race", "circle_1500")


@pytest.mark.parametrize("first,second", [("race", "circle_2049"), ("circle_2049", "race"), ("circle_2048", "race")])
def test_two_slots_either_side_of_the_staging_boundary(amd, race, first, second):
    _two_slots(amd, race, first, second)


def _two_slots(amd, race, first, second):
    """slot 0 / slot 1.  The kernel stages `cum` of the slot of the workgroup's first agent when that track has at most
    ref.STAGED_SEGS = 2048 segments; every other lane probes its own slot's column in L2.  The 1500-segment circle is staged
    where it comes first; the 2049-segment one never is: on slot 0 a workgroup that starts on it stages nothing, on slot 1 behind
    the 782-segment raceline its lanes probe L2 next to staged ones.  The three assignments put either slot first in a workgroup
    (16 envs a workgroup with P = 8, 32 with P = 3: envs 0, 16, 32, ... start one)."""
    made = {"race": lambda: race, "circle_1500": lambda: ref.circle(1500, radius=30.0, attrs=4),
            "circle_2049": lambda: ref.circle_2049(True, 4), "circle_2048": lambda: ref.circle_2048(True, 4)}
    (tab0, xy0, a0), (tab1, xy1, a1) = made[first](), made[second]()
    assert (tab0.nseg, tab1.nseg) == tuple({"race": 782, "circle_1500": 1500, "circle_2049": 2049, "circle_2048": 2048}[n] for n in (first, second))
    E, A = 70, 2
    N = E * A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.add_map_image(*load_map_image("example_map"))
    s.set_track(_track(amd, xy0, True, a0), 0)
    s.set_track(_track(amd, xy1, True, a1), 1)
    env_maps = (np.arange(E) % 2, (np.arange(E) + 1) % 2, (np.arange(E) // 3) % 2)   # either slot first in a workgroup
    for step in (16, 32):                              # the first envs of the workgroups: all slot 0, all slot 1, mixed
        assert [{int(m[e]) for e in range(0, E, step)} for m in env_maps] == [{0}, {1}, {0, 1}], step
    for env_map in env_maps:
        s.set_env_maps(env_map)
        s.enable_track()
        s.reset(bench_start_poses(E, A))
        s.step(np.tile([0.05, 2.0], (N, 1)))
        slot = np.repeat(env_map, A)
        poses, arc = _pose_and_s(s)
        for p in (amd.TrackPreview(points=8, channels=ALL8, frame="world"), amd.TrackPreview(points=3, spacing=2.0, channels=ALL8, frame="ego")):
            assert p.reach < min(tab0.L, tab1.L)
            out = s.track_preview_device(p).download()
            for m, tab in ((0, tab0), (1, tab1)):
                _check_device(tab, p, poses[slot == m], arc[slot == m], out[slot == m], "slot %d %s" % (m, p.frame))
    s.close()


# ---- env blocks -------------------------------------------------------------------------------------------------------------------
def test_two_blocks_equal_one(amd, race):
    tab, xy, attrs = race
    E, A, T = 512, 2, 12
    N = E * A
    p = amd.TrackPreview(points=8, channels=ALL8, frame="ego")
    res = []
    for groups in (1, 2):
        s = _sim(amd, E, A, _track(amd, xy, True, attrs), step_groups=groups)
        d_act = _armed(s, E, A)
        acts = _crash_actions(T, N)
        buf = s.device_array(p.shape(N), np.float32)
        pin = s.pinned_empty(p.shape(N), np.float32)
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            s.track_preview_device(p, buf, pinned=pin)
            s.step_device(d_act)                       # a step right behind the preview keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            s.track_preview_device(p, buf, pinned=pin)
        s.sync()
        out = buf.download()
        assert np.array_equal(ref.bits(np.array(pin)), ref.bits(out)), "the pinned copy differs from the download"
        poses, arc = _pose_and_s(s)
        _check_device(tab, p, poses[:64], arc[:64], out[:64], "groups=%d" % groups)
        res.append(out)
        s.close()
    assert np.array_equal(ref.bits(res[0]), ref.bits(res[1])), "two blocks against one"


# ---- no effect on the step --------------------------------------------------------------------------------------------------------
def test_preview_calls_change_no_step(amd, race):
    tab, xy, attrs = race
    E, A, T = 32, 2, 100
    N = E * A
    acts = _crash_actions(T, N, seed=5)
    p = amd.TrackPreview(points=8, channels=ALL8)
    res = []
    for use in (False, True):
        s = _sim(amd, E, A, _track(amd, xy, True, attrs))
        d_act = _armed(s, E, A)
        launches = []
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            launches.append(s.step_launches())
            if use:
                s.track_preview_device(p)
        o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
        trk = s.get_track()
        res.append((launches, {k: np.array(v, copy=True) for k, v in list(o.items()) + list(trk.items())}, s.save_state().to_bytes()))
        s.close()
    assert res[0][0] == res[1][0], "f110_step_launches changed"
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k
    assert res[0][2] == res[1][2], "the state blobs differ"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_write_nothing(amd, race):
    from f1tenth_gym_amd import _ffi
    tab, xy, attrs = race
    E, A = 8, 2
    N = E * A
    s = _sim(amd, E, A, None)
    L = _ffi.lib()
    good = amd.TrackPreview(points=8, channels=("x", "y", "attr0"))
    shape = good.shape(N)
    d_out = s.device_array(shape, np.float32)
    sentinel = np.random.default_rng(1).normal(size=shape).astype(np.float32)
    d_out.upload(sentinel)
    pin = s.pinned_empty(shape, np.float32)
    pin[...] = sentinel

    def call(ptr=None, pinned=None, **fields):
        sp = good.spec()
        for k, v in fields.items():
            if k == "scale":
                sp.scale[v[0]] = v[1]
            else:
                setattr(sp, k, v)
        return L.f110_track_preview_device(s._h, C.byref(sp), d_out.ptr if ptr is None else ptr, pinned)

    # attributes: no track on the slot yet, then the wrong shapes
    a = np.ascontiguousarray(attrs[:-1])
    assert L.f110_track_set_attrs(s._h, 0, _ffi.dptr(a), a.shape[0], a.shape[1]) == _ffi.ERR_INVALID
    assert call() == _ffi.ERR_STATE                                                   # tracking is off (and there is no track)
    s.set_track(amd.Track(xy))                                                        # a track without attributes
    assert call() == _ffi.ERR_STATE                                                   # tracking is still off
    s.enable_track()
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    assert call() == _ffi.ERR_STATE and "attribute" in _ffi.last_error(s._h)          # attr0 is not there
    bad_attr = a.copy()
    bad_attr[5, 1] = np.inf
    for arr, M, Cn in ((a, a.shape[0] - 1, 4), (a, a.shape[0] + 1, 4), (a, a.shape[0], 0), (a, a.shape[0], 5), (bad_attr, a.shape[0], 4)):
        assert L.f110_track_set_attrs(s._h, 0, _ffi.dptr(arr), M, Cn) == _ffi.ERR_INVALID, (M, Cn)
    assert L.f110_track_set_attrs(s._h, 0, None, a.shape[0], 4) == _ffi.ERR_INVALID
    assert L.f110_track_set_attrs(s._h, 1, _ffi.dptr(a), a.shape[0], 4) == _ffi.ERR_INVALID    # no such slot
    assert call() == _ffi.ERR_STATE                                                   # refused attributes changed nothing
    s.set_track_attrs(0, a[:, :1])
    inf, nan = float("inf"), float("nan")
    bad = [dict(points=0), dict(points=33), dict(points=-1), dict(channels=0), dict(channels=256 | 1), dict(channels=-1), dict(frame=2), dict(frame=-1),
           dict(flags=1), dict(offset=-0.5), dict(offset=inf), dict(offset=nan), dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=inf),
           dict(spacing=nan), dict(points=1, spacing=0.0), dict(scale=(0, 0.0)), dict(scale=(1, nan)), dict(scale=(4, inf)),
           dict(ptr=0), dict(ptr=d_out.ptr + 4), dict(ptr=d_out.ptr + 8)]
    for f in bad:
        assert call(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
    heap = np.zeros(shape, dtype=np.float32)
    assert call(pinned=heap.ctypes.data) == _ffi.ERR_INVALID                          # not f110_host_alloc memory
    small = s.pinned_empty((N, 8, 2), np.float32)
    assert call(pinned=small.ctypes.data) == _ffi.ERR_INVALID                         # too small for [N][P][D]
    assert call(channels=1 | 2 | 32) == _ffi.ERR_STATE                                # attr1 of a one-attribute track
    assert call(points=32, spacing=6.0) == _ffi.ERR_STATE and "reach" in _ffi.last_error(s._h)   # the closed track is shorter
    s.set_track_attrs(0, None)
    assert call() == _ffi.ERR_STATE                                                   # cleared
    s.set_track_attrs(0, a)
    s.set_track(amd.Track(xy))                                                        # a new track clears the slot's attributes
    assert call() == _ffi.ERR_STATE
    s.sync()
    assert np.array_equal(ref.bits(d_out.download()), ref.bits(sentinel)), "a refused call wrote d_out"
    assert np.array_equal(ref.bits(np.array(pin)), ref.bits(sentinel))
    # the unit form refuses the same way and leaves the caller's arrays alone
    rows = np.zeros((N, 4))
    out = sentinel.copy()
    sp = good.spec()
    assert L.f110_track_preview_batch(s._h, C.byref(sp), 0, _ffi.dptr(rows), N, out.ctypes.data, None, None) == _ffi.ERR_STATE    # attr0
    sp = amd.TrackPreview().spec()
    sp.points = 40
    assert L.f110_track_preview_batch(s._h, C.byref(sp), 0, _ffi.dptr(rows), N, out.ctypes.data, None, None) == _ffi.ERR_INVALID
    sp = amd.TrackPreview().spec()
    assert L.f110_track_preview_batch(s._h, C.byref(sp), 1, _ffi.dptr(rows), N, out.ctypes.data, None, None) == _ffi.ERR_STATE    # no track there
    assert np.array_equal(ref.bits(out), ref.bits(sentinel))
    with pytest.raises(ValueError):
        s.track_preview_device(good, s.device_array((N, 8, 2), np.float32))
    with pytest.raises(ValueError):
        s.track_preview_device(good, pinned=heap[:, :4])
    # and the good spec goes through, into the pinned block as well
    s.set_track_attrs(0, a)
    assert call(pinned=pin.ctypes.data) == _ffi.OK
    s.sync()
    got = d_out.download()
    assert not np.array_equal(got, sentinel) and np.array_equal(ref.bits(np.array(pin)), ref.bits(got))
    poses, arc = _pose_and_s(s)
    _check_device(tab, good, poses, arc, got, "after the refusals")
    s.close()


# ---- DLPack: a torch consumer in a fresh process ------------------------------------------------------------------------------------
def test_torch_consumer_in_a_fresh_process():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "track_preview_torch_worker.py")
    r = subprocess.run([sys.executable, worker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    if "SKIP" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert "TRACK PREVIEW TORCH OK" in r.stdout, r.stdout[-3000:]


# ---- the env layers -------------------------------------------------------------------------------------------------------------------
def _assert_same_step(a, b, what, skip=()):
    for k in b[0]:
        if k not in skip:
            assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), "%s: obs[%r]" % (what, k)
    assert np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and np.array_equal(a[2], b[2]), what
    for k in b[3]:
        assert np.array_equal(a[3][k], b[3][k]), "%s: info[%r]" % (what, k)


def _check_obs(tab, p, obs, what, batch=None):
    """batch: also hold the pose fields to the observation's pose.  They differ from it in one place: poses_theta of a car that
    hit a wall in the step is 0 (check_ttc zeroes state[3:] behind the observation), where the preview, like `progress` and
    `heading_error`, keeps the heading the car arrived with."""
    E, A = obs["poses_x"].shape
    poses = np.stack([obs["poses_x"], obs["poses_y"], obs["poses_theta"]], axis=2).reshape(-1, 3)
    if batch is not None:
        snap = batch.get("agent_poses")["agent_poses"]
        zeroed = poses[:, 2] != snap[:, 2]
        assert np.array_equal(poses[:, :2], snap[:, :2]) and not poses[zeroed, 2].any(), what
        assert np.asarray(obs["collisions"]).reshape(-1)[zeroed].all(), what
        poses = snap
    out = np.asarray(obs["track_preview"])
    assert out.shape == (E, A, p.points, p.dim) and out.dtype == np.float32
    return _check_device(tab, p, poses, np.asarray(obs["progress"]).reshape(-1), out.reshape((E * A,) + out.shape[2:]), what)


def test_vec_env_preview_belongs_to_the_steps_observation(amd, race):
    tab, xy, attrs = race
    E, A, T = 32, 2, 100
    p = amd.TrackPreview(points=6, offset=0.3, spacing=0.7, channels=("x", "y", "tan_x", "tan_y", "attr1"), frame="ego", scale={"attr1": 8.0})
    kw = dict(auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png", track=_track(amd, xy, True, attrs))
    env, env2, plain = amd.F110VecEnv(E, track_preview=p, **kw), amd.F110VecEnv(E, track_preview=p.settings(), **kw), amd.F110VecEnv(E, **kw)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    first = env.reset(start)
    env2.reset(start)
    _assert_same_step(first, plain.reset(start), "reset")
    assert sorted(first[0]) == sorted(list(plain._last[0]) + ["track_preview"])
    differ = _check_obs(tab, p, first[0], "reset", env.sim.batch)
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    dones = 0
    for t in range(T):
        a, b = env.step(acts[t]), plain.step(acts[t])
        _assert_same_step(a, b, "step %d" % t)
        differ += _check_obs(tab, p, a[0], "step %d" % t, env.sim.batch)
        env2.step_async(acts[t])
        c = env2.step_wait()
        _assert_same_step(c, b, "step_async / step_wait, step %d" % t)
        assert np.array_equal(ref.bits(np.asarray(c[0]["track_preview"])), ref.bits(np.asarray(a[0]["track_preview"])))
        dones += int(np.sum(b[2]))
    assert dones > 5 and differ * 1000 <= (T + 1) * E * A * p.points * p.dim, (dones, differ)
    again = env.reset(start)                                  # also valid after reset()
    _check_obs(tab, p, again[0], "second reset", env.sim.batch)


def test_sharded_equals_one_handle(amd, race):
    tab, xy, attrs = race
    E, A, T = 30, 2, 40
    p = dict(points=4, channels=("x", "y", "attr0", "attr3"), frame="world")
    kw = dict(auto_reset=True, map=map_stem("example_map"), map_ext=".png", track=_track(amd, xy, True, attrs), track_preview=p)
    one = amd.F110VecEnv(E, device_logic=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], shard_sizes=[7, 12, 11], **kw)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    a, b = sh.reset(start), one.reset(start)
    _assert_same_step(a, b, "reset")
    assert a[0]["track_preview"].shape == (E, A, 4, 4)
    acts = _crash_actions(T, E * A, seed=10).reshape(T, E, A, 2)
    for t in range(T):
        _assert_same_step(sh.step(acts[t]), one.step(acts[t]), "step %d" % t)
    _check_obs(tab, amd.TrackPreview(**p), one._last[0], "one handle")
    sh.close()


def test_single_env_carries_the_key(amd, race):
    tab, xy, attrs = race
    p = amd.TrackPreview(points=5, channels=("x", "y", "attr1"), frame="ego")
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, track=_track(amd, xy, True, attrs), track_preview=p)
    plain = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, track=_track(amd, xy, True, attrs))
    start = bench_start_poses(1, 2)
    obs, obs0 = env.reset(start)[0], plain.reset(start)[0]
    for t in range(5):
        obs, obs0 = env.step(np.array([[0.1, 3.0], [-0.1, 2.0]]))[0], plain.step(np.array([[0.1, 3.0], [-0.1, 2.0]]))[0]
    assert sorted(obs) == sorted(list(obs0) + ["track_preview"])
    for k in obs0:
        assert np.array_equal(np.asarray(obs[k]), np.asarray(obs0[k]), equal_nan=True), k
    poses = np.column_stack([obs["poses_x"], obs["poses_y"], obs["poses_theta"]])
    assert obs["track_preview"].shape == (2, 5, 3)
    _check_device(tab, p, poses, np.asarray(obs["progress"]), obs["track_preview"], "F110Env")
    with pytest.raises(ValueError):
        amd.F110Env(map=map_stem("example_map"), map_ext=".png", track_preview=p)
