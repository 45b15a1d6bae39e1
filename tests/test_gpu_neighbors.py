"""The neighbour observation on the device (f110_neighbors_*) against the Python model tests/neighbors_ref.py with the
assertions of the host tests (ref.compare): the indices, VALID, INDEX, DIST and GAP_S bit for bit, the rotated channels within
8 eps of their size, every float32 output the model's or its neighbour and at most 1 in 1000 different.  The unit form over the
grid of the host tests, the device form through noisy steps with in-step re-seats, env blocks, no effect on the step, the
refusals, the pinned copy, DLPack, the env layers.

The pose a neighbour call reads is the observation's (agent_poses, the one no in-step re-seat overwrites, the pose `s` was computed
from); the speed is the live state[3], which an in-step re-seat has zeroed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import neighbors_ref as ref
from _util import MAPS, bench_start_poses, load_map_image, map_stem

pytestmark = pytest.mark.gpu

SEED, STD = 4242, 0.01
CSV = os.path.join(MAPS, "example_waypoints.csv")
ALL10 = ref.CHANNELS
NO_GAP = tuple(c for c in ALL10 if c != "gap_s")
SCALE = {"dx": 10.0, "dy": -4.0, "dist": 3.0, "v_x": 0.5, "gap_s": 25.0}


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def track(amd):
    return amd.Track.from_csv(CSV)


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


def _rows(s, with_track=True):
    """what a neighbour call reads: the observation's pose, the live speed, the s column"""
    poses = np.array(s.get("agent_poses")["agent_poses"], copy=True)
    v = np.array(s.get("state")["state"], copy=True)[:, 3]
    arc = np.array(s.get_track()["s"], copy=True) if with_track else np.zeros(len(v))
    return np.ascontiguousarray(np.column_stack([poses, v, arc]))


def _check_device(p, rows, A, L, out, what):
    """the device form has no raw values: the float32 outputs as ref.compare_out holds them -> how many differ"""
    s = ref.settings(**p.settings())
    return ref.compare_out(s, ref.neighbors(s, rows, A, L)[0], out, what)


# ---- the unit form over the grid -----------------------------------------------------------------------------------------------
def test_unit_form_matches_model_over_the_grid(amd):
    s = amd.BatchSim(num_envs=1, num_agents=1)        # (no map: a unit entry point; A is the call's, not the handle's)
    total = differ = 0
    for case in ref.unit_grid():
        st, rows, L, want = ref.grid_case(case)
        got = s.neighbors(rows, amd.Neighbors(**st), case[1], L, raw=True, indices=True)
        differ += ref.compare(st, rows, case[1], want, got, "%r" % (case[:4],))
        total += want[0].size
    # more envs than a workgroup holds groups (128 at A = 2), without raw and indices
    rows = ref.cars("scatter", 2, 130, 77)
    for st in (ref.settings(k=1, channels=("dx", "dy", "dist", "valid")), ref.settings(k=8, channels=ALL10, max_range=2.0, pad=-1.0, scale=SCALE)):
        out = s.neighbors(rows, amd.Neighbors(**st), 2, ref.TRACK_L)
        differ += ref.compare_out(st, ref.neighbors(st, rows, 2, ref.TRACK_L)[0], out, "130 envs of 2")
        total += out.size
    assert total > 30000 and differ * 1000 <= total, (total, differ)
    s.close()


# ---- the device form through noisy steps with in-step re-seats -----------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 4])
def test_device_form_follows_model_through_reseats(amd, track, A):
    E, T = 64, 150
    N = E * A
    s = _sim(amd, E, A, track)
    d_act = _armed(s, E, A)
    acts = _crash_actions(T, N)
    near = amd.Neighbors(k=1, channels=("dx", "dy", "dist", "valid"), max_range=3.0, pad=-1.0)
    full = amd.Neighbors(k=8 if A == 4 else 3, channels=ALL10, scale=SCALE)
    bufs = {}
    fresh = total = differ = reseat_steps = moving = 0
    for t in range(T):
        d_act.upload(acts[t])
        s.step_device(d_act)
        # the sample: every tenth step, the last one, and the first six steps in which some env was re-seated
        seated = s.get("step_count")["step_count"] == 0      # re-seated inside this step: the live speed is 0, the pose the old one
        take_reseat = bool(seated.any()) and reseat_steps < 6
        if not (t % 10 == 3 or t == T - 1 or take_reseat):
            continue
        reseat_steps += int(take_reseat)
        for p in (near, full):
            bufs[p] = s.neighbors_device(p, bufs.get(p))
        rows = _rows(s)
        assert not rows[seated, 3].any()
        fresh += int(np.sum(seated))
        moving += int(np.sum(rows[:, 3] != 0.0))
        for p in (near, full):
            differ += _check_device(p, rows, A, track.length, bufs[p].download(), "A=%d step %d k=%d" % (A, t, p.k))
            total += N * p.k * p.dim
    assert fresh >= A, "no env was re-seated in a sampled step (%d agents)" % fresh
    assert moving > N and differ * 1000 <= total, (moving, differ, total)
    s.close()


# ---- env blocks -------------------------------------------------------------------------------------------------------------------
def test_two_blocks_equal_one(amd, track):
    E, A, T = 512, 2, 12
    N = E * A
    p = amd.Neighbors(k=2, channels=ALL10, pad=-2.0)
    res = []
    for groups in (1, 2):
        s = _sim(amd, E, A, track, step_groups=groups)
        d_act = _armed(s, E, A)
        acts = _crash_actions(T, N)
        buf = s.device_array(p.shape(N), np.float32)
        pin = s.pinned_empty(p.shape(N), np.float32)
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            s.neighbors_device(p, buf, pinned=pin)
            s.step_device(d_act)                       # a step right behind the call keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            s.neighbors_device(p, buf, pinned=pin)
        s.sync()
        out = buf.download()
        assert np.array_equal(ref.bits(np.array(pin)), ref.bits(out)), "the pinned copy differs from the download"
        rows = _rows(s)
        _check_device(p, rows[:64], A, track.length, out[:64], "groups=%d" % groups)
        _check_device(p, rows[-64:], A, track.length, out[-64:], "groups=%d, the last envs" % groups)
        res.append(out)
        s.close()
    assert np.array_equal(ref.bits(res[0]), ref.bits(res[1])), "two blocks against one"


# ---- no effect on the step --------------------------------------------------------------------------------------------------------
def test_neighbor_calls_change_no_step(amd, track):
    E, A, T = 32, 2, 100
    N = E * A
    acts = _crash_actions(T, N, seed=5)
    p = amd.Neighbors(k=3, channels=ALL10)
    res = []
    for use in (False, True):
        s = _sim(amd, E, A, track)
        d_act = _armed(s, E, A)
        launches = []
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            launches.append(s.step_launches())
            if use:
                s.neighbors_device(p)
        o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
        trk = s.get_track()
        res.append((launches, {k: np.array(v, copy=True) for k, v in list(o.items()) + list(trk.items())}, s.save_state().to_bytes()))
        s.close()
    assert res[0][0] == res[1][0], "f110_step_launches changed"
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k
    assert res[0][2] == res[1][2], "the state blobs differ"


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_write_nothing(amd, track):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    s = _sim(amd, E, A, None)
    L = _ffi.lib()
    good = amd.Neighbors(k=3, channels=("dx", "dy", "valid"))
    gap = amd.Neighbors(k=3, channels=("dx", "gap_s", "valid"))
    shape = good.shape(N)
    d_out = s.device_array(shape, np.float32)
    sentinel = np.random.default_rng(1).normal(size=shape).astype(np.float32)
    d_out.upload(sentinel)
    pin = s.pinned_empty(shape, np.float32)
    pin[...] = sentinel

    def call(ptr=None, pinned=None, base=good, **fields):
        sp = base.spec()
        for k, v in fields.items():
            if k == "scale":
                sp.scale[v[0]] = v[1]
            else:
                setattr(sp, k, v)
        return L.f110_neighbors_device(s._h, C.byref(sp), d_out.ptr if ptr is None else ptr, pinned)

    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    inf, nan = float("inf"), float("nan")
    bad = [dict(k=0), dict(k=9), dict(k=-1), dict(channels=0), dict(channels=1024 | 1), dict(channels=-1), dict(flags=1), dict(flags=-1),
           dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=nan), dict(max_range=-inf), dict(pad=inf), dict(pad=-inf), dict(pad=nan),
           dict(scale=(0, 0.0)), dict(scale=(1, nan)), dict(scale=(8, inf)), dict(ptr=0), dict(ptr=d_out.ptr + 4), dict(ptr=d_out.ptr + 8)]
    for f in bad:
        assert call(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
    assert call(scale=(2, 0.0)) == _ffi.OK                                            # (a clear bit's scale is ignored)
    d_out.upload(sentinel)
    heap = np.zeros(shape, dtype=np.float32)
    assert call(pinned=heap.ctypes.data) == _ffi.ERR_INVALID                          # not f110_host_alloc memory
    small = s.pinned_empty((N, 3, 2), np.float32)
    assert call(pinned=small.ctypes.data) == _ffi.ERR_INVALID                         # too small for [N][K][D]
    assert call(base=gap) == _ffi.ERR_STATE and "tracking is off" in _ffi.last_error(s._h)
    s.set_track(track)
    s.enable_track()
    s.add_map_image(*load_map_image("example_map"))
    s.set_env_maps(np.arange(E) % 2)                                                  # tracking is on, and slot 1, now in use, has no track
    assert call(base=gap) == _ffi.ERR_STATE and "no track" in _ffi.last_error(s._h)
    assert call() == _ffi.OK                                                          # (without 'gap_s' no track is asked for)
    d_out.upload(sentinel)
    many = amd.BatchSim(num_envs=1, num_agents=257)                                   # more cars per env than a workgroup has lanes
    big = many.device_array(good.shape(257), np.float32)
    sp = good.spec()
    assert L.f110_neighbors_device(many._h, C.byref(sp), big.ptr, None) == _ffi.ERR_STATE and "257" in _ffi.last_error(many._h)
    many.close()
    s.sync()
    assert np.array_equal(ref.bits(d_out.download()), ref.bits(sentinel)), "a refused call wrote d_out"
    assert np.array_equal(ref.bits(np.array(pin)), ref.bits(sentinel))
    # the unit form refuses the same way and leaves the caller's arrays alone
    rows = np.zeros((N, 5))
    out = sentinel.copy()
    for sp, An, Lt, m in ((good.spec(), 0, 0.0, N), (good.spec(), 257, 0.0, 257 * 2), (good.spec(), 3, 0.0, N), (good.spec(), 2, -1.0, N),
                          (good.spec(), 2, nan, N), (good.spec(), 2, inf, N)):
        assert L.f110_neighbors_batch(s._h, C.byref(sp), An, Lt, _ffi.dptr(rows), m, out.ctypes.data, None, None) == _ffi.ERR_INVALID, (An, Lt, m)
    sp = good.spec()
    sp.k = 9
    assert L.f110_neighbors_batch(s._h, C.byref(sp), 2, 0.0, _ffi.dptr(rows), N, out.ctypes.data, None, None) == _ffi.ERR_INVALID
    assert np.array_equal(ref.bits(out), ref.bits(sentinel))
    with pytest.raises(ValueError):
        s.neighbors_device(good, s.device_array((N, 3, 2), np.float32))
    with pytest.raises(ValueError):
        s.neighbors_device(good, pinned=heap[:, :2])
    with pytest.raises(ValueError):
        s.neighbors(np.zeros((N, 4)), good, 2)
    # and the good spec goes through, into the pinned block as well
    assert call(pinned=pin.ctypes.data) == _ffi.OK
    s.sync()
    got = d_out.download()
    assert not np.array_equal(got, sentinel) and np.array_equal(ref.bits(np.array(pin)), ref.bits(got))
    _check_device(good, _rows(s, with_track=False), A, 0.0, got, "after the refusals")
    s.close()


# ---- DLPack: a torch consumer in a fresh process ------------------------------------------------------------------------------------
def test_torch_consumer_in_a_fresh_process():
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "neighbors_torch_worker.py")
    r = subprocess.run([sys.executable, worker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    if "SKIP" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert "NEIGHBORS TORCH OK" in r.stdout, r.stdout[-3000:]


# ---- the env layers -------------------------------------------------------------------------------------------------------------------
def _assert_same_step(a, b, what, skip=()):
    for k in b[0]:
        if k not in skip:
            assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), "%s: obs[%r]" % (what, k)
    assert np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and np.array_equal(a[2], b[2]), what
    for k in b[3]:
        assert np.array_equal(a[3][k], b[3][k]), "%s: info[%r]" % (what, k)


def _check_obs(p, obs, batch, L, what):
    """the observation's neighbours against the model from the handle's own columns (the observation's pose, the live speed);
    the observation's progress is the s column"""
    E, A = obs["poses_x"].shape
    rows = _rows(batch, with_track=p.needs_track)
    if p.needs_track:
        assert np.array_equal(rows[:, 4], np.asarray(obs["progress"]).reshape(-1), equal_nan=True), what
    assert np.array_equal(rows[:, 0], np.asarray(obs["poses_x"]).reshape(-1)) and np.array_equal(rows[:, 1], np.asarray(obs["poses_y"]).reshape(-1)), what
    out = np.asarray(obs["neighbors"])
    assert out.shape == (E, A, p.k, p.dim) and out.dtype == np.float32
    return _check_device(p, rows, A, L, out.reshape((E * A,) + out.shape[2:]), what)


def test_vec_env_neighbors_belong_to_the_steps_observation(amd, track):
    E, A, T = 32, 2, 100
    p = amd.Neighbors(k=2, channels=("dx", "dy", "dist", "v_x", "gap_s", "valid"), max_range=6.0, pad=-1.0, scale={"gap_s": 8.0})
    kw = dict(auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png", track=track)
    env, env2, plain = amd.F110VecEnv(E, neighbors=p, **kw), amd.F110VecEnv(E, neighbors=p.settings(), **kw), amd.F110VecEnv(E, **kw)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    first = env.reset(start)
    env2.reset(start)
    _assert_same_step(first, plain.reset(start), "reset")
    assert sorted(first[0]) == sorted(list(plain._last[0]) + ["neighbors"])
    differ = _check_obs(p, first[0], env.sim.batch, track.length, "reset")
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    dones = 0
    for t in range(T):
        a, b = env.step(acts[t]), plain.step(acts[t])
        _assert_same_step(a, b, "step %d" % t)
        differ += _check_obs(p, a[0], env.sim.batch, track.length, "step %d" % t)
        env2.step_async(acts[t])
        c = env2.step_wait()
        _assert_same_step(c, b, "step_async / step_wait, step %d" % t)
        assert np.array_equal(ref.bits(np.asarray(c[0]["neighbors"])), ref.bits(np.asarray(a[0]["neighbors"])))
        dones += int(np.sum(b[2]))
    assert dones > 5 and differ * 1000 <= (T + 1) * E * A * p.k * p.dim, (dones, differ)
    again = env.reset(start)                                  # also valid after reset()
    _check_obs(p, again[0], env.sim.batch, track.length, "second reset")
    # without 'gap_s' no track is needed
    q = amd.Neighbors(k=1, channels=("dist", "index"))
    bare = amd.F110VecEnv(4, neighbors=q, auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png")
    o = bare.reset(bench_start_poses(4, A).reshape(4, A, 3))[0]
    _check_obs(q, o, bare.sim.batch, 0.0, "no track")


def test_sharded_equals_one_handle(amd, track):
    E, A, T = 30, 2, 40
    p = dict(k=2, channels=("dx", "dy", "gap_s", "index"))
    kw = dict(auto_reset=True, map=map_stem("example_map"), map_ext=".png", track=track, neighbors=p)
    one = amd.F110VecEnv(E, device_logic=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], shard_sizes=[7, 12, 11], **kw)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    a, b = sh.reset(start), one.reset(start)
    _assert_same_step(a, b, "reset")
    assert a[0]["neighbors"].shape == (E, A, 2, 4)
    acts = _crash_actions(T, E * A, seed=10).reshape(T, E, A, 2)
    for t in range(T):
        _assert_same_step(sh.step(acts[t]), one.step(acts[t]), "step %d" % t)
    _check_obs(amd.Neighbors(**p), one._last[0], one.sim.batch, track.length, "one handle")
    sh.close()


def test_single_env_carries_the_key(amd, track):
    p = amd.Neighbors(k=2, channels=("dx", "dy", "gap_s", "valid"), pad=-1.0)
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=3, track=track, neighbors=p)
    plain = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=3, track=track)
    start = bench_start_poses(1, 3)
    act = np.array([[0.1, 3.0], [-0.1, 2.0], [0.0, 1.0]])
    obs, obs0 = env.reset(start)[0], plain.reset(start)[0]
    for t in range(5):
        obs, obs0 = env.step(act)[0], plain.step(act)[0]
    assert sorted(obs) == sorted(list(obs0) + ["neighbors"])
    for k in obs0:
        assert np.array_equal(np.asarray(obs[k]), np.asarray(obs0[k]), equal_nan=True), k
    assert obs["neighbors"].shape == (3, 2, 4)
    rows = np.column_stack([obs["poses_x"], obs["poses_y"], obs["poses_theta"], obs["linear_vels_x"], np.asarray(obs["progress"])])
    _check_device(p, rows, 3, track.length, obs["neighbors"], "F110Env")
    with pytest.raises(ValueError):
        amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, neighbors=dict(channels=("gap_s",)))
