"""Exact snapshot, restore and clone of simulator state (include/f110.h f110_state_*, BatchSim.save_state / load_state /
save_envs / load_envs / clone_envs, snapshot() / restore() of the env layers): a restored or cloned env continues bit for bit
as the original did."""
import numpy as np
import pytest

from _util import bench_start_poses, load_map_image, map_stem, oracle_map_dt, rel_err

pytestmark = pytest.mark.gpu

SEED, STD = 12345, 0.01
ALL = ("scans", "state", "agent_poses", "collisions", "collision_idx", "in_collision", "step_count")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _sim(amd, E, A=2, noise=True, cache_rows=0, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    if noise:
        s.set_noise_rng(SEED, STD, cache_rows=cache_rows)
    return s


def _actions(T, E, A, seed=7):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.4, 0.4, (T, E * A)), rng.uniform(2.0, 8.0, (T, E * A))], axis=2)


def _record(s, episode):
    o = s.get(*ALL)
    if episode:
        o.update({"ep_" + k: v for k, v in s.episode_get().items()})
    return o


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), "%s%s differs" % (what, k)


class _Episodic(object):
    """E envs of 2 cars with the device episode logic, auto re-seat armed, shared device noise (the issue's item 1 setup)"""

    def __init__(self, amd, E, cache_rows=0):
        self.s = s = _sim(amd, E, cache_rows=cache_rows)
        s.episode_init(0)
        self.poses = bench_start_poses(E, 2, gap_wp=6)
        s.episode_reset(self.poses)
        self.d_start = s.device_array((E * 2, 3))
        self.d_start.upload(self.poses)
        self.d_count = s.device_array((1,), np.int32)
        self.d_count.upload(np.zeros(1, np.int32))
        s.set_auto_reseat(self.d_start, 0, self.d_count)
        self.d_act = s.device_array((E * 2, 2))

    def run(self, acts, record=False):
        out = []
        for a in acts:
            self.d_act.upload(a)
            self.s.episode_step_device(self.d_act)
            if record:
                out.append(_record(self.s, True))
        return out


@pytest.fixture(scope="module")
def episodic(amd):
    """150 steps, a save, 150 more recorded: shared by items 1 and 2"""
    E = 64
    acts = _actions(300, E, 2)
    run = _Episodic(amd, E)
    run.run(acts[:150])
    blob = run.s.save_state()
    rec = run.run(acts[150:], record=True)
    resets = int(run.d_count.download()[0])
    yield run, blob, acts, rec, resets
    run.s.close()


def test_round_trip_on_one_handle(amd, episodic):
    run, blob, acts, rec, resets = episodic
    assert resets > 0, "the run is meant to re-seat envs along the way"
    assert blob.header["scans"] and "episode" in blob.header["columns"] and blob.header["max_step"] == 300 - 150
    run.s.load_state(blob)
    again = run.run(acts[150:], record=True)
    for t, (a, b) in enumerate(zip(rec, again)):
        _same(a, b, "step %d: " % t)


def test_restore_into_a_fresh_handle_with_a_small_row_cache(amd, episodic):
    """cache_rows = 64: the restored episodes (> 64 steps) run past the row cache, whose positions the blob carries"""
    run, blob, acts, rec, _ = episodic
    fresh = _Episodic(amd, 64, cache_rows=64)
    fresh.s.load_state(blob)
    again = fresh.run(acts[150:], record=True)
    for t, (a, b) in enumerate(zip(rec, again)):
        _same(a, b, "step %d: " % t)
    fresh.s.close()


def test_restored_slice_matches_the_oracle(amd):
    """32 envs saved after 80 steps, restored into a fresh handle (row cache of 64 rows), 40 steps more: the oracle run
    uninterrupted for 120 steps with the same actions and NumPy's noise rows agrees (flags exact, floats <= 1e-5)"""
    from oracle import orc
    E, A, T0, T1 = 32, 2, 80, 40
    img, res, origin = load_map_image("example_map")
    dt, _, _ = oracle_map_dt("example_map")
    acts = _actions(T0 + T1, E, A, seed=3)
    acts[:, :, 1] = np.clip(acts[:, :, 1], 1.0, 4.0)
    poses = bench_start_poses(E, A, gap_wp=6)
    s = _sim(amd, E)
    s.reset(poses)
    for t in range(T0):
        s.step(acts[t])
    blob = s.save_state(scans=False)
    s.close()
    f = _sim(amd, E, cache_rows=64)
    f.load_state(blob)
    for t in range(T0, T0 + T1):
        f.step(acts[t])
    o = f.get("scans", "state", "collisions", "in_collision")
    f.close()
    ref = orc.SimOracle(E, A)
    ref.set_map_dt(dt, res, origin)
    ref.set_noise(np.random.default_rng(SEED).normal(0., STD, size=(T0 + T1 + 1, 1080)))
    ref.reset(poses)
    for t in range(T0 + T1):
        ref.step(acts[t])
    assert np.array_equal(o["collisions"], ref.collisions) and np.array_equal(o["in_collision"], ref.in_collision)
    assert rel_err(o["state"], ref.state) < 1e-5 and rel_err(o["scans"], ref.scans) < 1e-5


def test_tiny_step_save_restore_through_f110env(amd):
    """item 1 again on the one-launch step (k_step_tiny: one env of two cars behind F110Env)"""
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2)
    poses = bench_start_poses(1, 2, gap_wp=6)
    env.reset(poses)
    acts = _actions(120, 1, 2, seed=5).reshape(120, 2, 2)
    for t in range(60):
        env.step(acts[t])
    assert env.sim.batch.step_launches() == 1
    snap = env.snapshot()
    first = [env.step(acts[t]) for t in range(60, 120)]
    back = env.restore(snap)
    assert np.array_equal(back[0]["scans"][0], snap["host"][7][0]["scans"][0])
    second = [env.step(acts[t]) for t in range(60, 120)]
    for (o1, r1, d1, i1), (o2, r2, d2, i2) in zip(first, second):
        for k in ("scans", "poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions", "lap_times", "lap_counts"):
            assert np.array_equal(np.asarray(o1[k]), np.asarray(o2[k])), k
        assert r1 == r2 and d1 == d2 and np.array_equal(i1["checkpoint_done"], i2["checkpoint_done"])
    env.close() if hasattr(env, "close") else None


def test_per_agent_noise_subset_into_another_handle(amd):
    E, A, T = 48, 2, 60
    seeds = list(range(1000, 1000 + E * A))
    a = _sim(amd, E, noise=False)
    a.set_noise_rng(None, STD, per_agent_seeds=seeds)
    a.reset(bench_start_poses(E, A, gap_wp=4))
    acts = _actions(2 * T, E, A, seed=11)
    for t in range(T):
        a.step(acts[t])
    pick = [3, 17, 40]
    blob = a.save_envs(pick)
    assert blob.num_envs == 3 and "rng_seed" in blob.header["columns"] and not blob.header["scans"]
    want = []
    rows = np.concatenate([np.arange(e * A, e * A + A) for e in pick])
    for t in range(T, 2 * T):
        a.step(acts[t])
        want.append({k: v[rows] for k, v in a.get(*ALL).items()})
    a.close()

    E2 = 12
    b = _sim(amd, E2, noise=False)
    b.set_noise_rng(None, STD, per_agent_seeds=list(range(7, 7 + E2 * A)))
    b.reset(bench_start_poses(E2, A, gap_wp=5))
    for t in range(5):
        b.step(_actions(1, E2, A, seed=100 + t)[0])
    before = b.get(*ALL)
    dst = [5, 6, 7]
    b.load_envs(blob, [0, 1, 2], dst)
    after = b.get(*ALL)
    rows_b = np.concatenate([np.arange(e * A, e * A + A) for e in dst])
    others = np.setdiff1d(np.arange(E2 * A), rows_b)
    for k in ALL:
        assert np.array_equal(after[k][others], before[k][others]), k
    assert np.array_equal(after["step_count"][rows_b], np.full(6, T))
    act_b = _actions(T, E2, A, seed=12)
    for t in range(T):
        act_b[t].reshape(E2, A, 2)[dst] = acts[T + t].reshape(E, A, 2)[pick]
        b.step(act_b[t])
        got = b.get(*ALL)
        for k in ALL:
            assert np.array_equal(got[k][rows_b], want[t][k]), "step %d: %s" % (t, k)
    b.close()


def test_clone_one_env_into_32(amd):
    E, A, T = 48, 2, 300
    s = _sim(amd, E)
    poses = bench_start_poses(E, A, gap_wp=4)
    s.reset(poses)
    d_start = s.device_array((E * A, 3))
    d_start.upload(poses)
    d_count = s.device_array((1,), np.int32)
    d_count.upload(np.zeros(1, np.int32))
    s.set_auto_reseat(d_start, 0, d_count)
    acts = _actions(T + 20, E, A, seed=21)
    for t in range(20):
        s.step(acts[t])
    group = [3] + list(range(10, 42))
    s.clone_envs([3] * 32, list(range(10, 42)))
    # the re-seat poses are the caller's configuration, not env state: the clones re-seat where env 3 does
    start = poses.reshape(E, A, 3).copy()
    start[group] = start[3]
    d_start.upload(start.reshape(E * A, 3))
    rows = lambda e: slice(e * A, e * A + A)   # noqa: E731
    o = s.get(*ALL)
    for e in group[1:]:
        for k in ALL:
            assert np.array_equal(o[k][rows(e)], o[k][rows(3)]), (e, k)
    collided = 0
    for t in range(20, T + 20):
        a = acts[t].reshape(E, A, 2)
        a[group] = a[3]
        s.step(acts[t])
        o = s.get(*ALL)
        collided += int(o["collisions"][rows(3)][0] != 0)
        for e in group[1:]:
            for k in ALL:
                assert np.array_equal(o[k][rows(e)], o[k][rows(3)]), (t, e, k)
    assert collided > 0, "the cloned env is meant to collide and be re-seated"
    # host index lists are checked
    with pytest.raises(ValueError, match="overlap"):
        s.clone_envs([3, 4], [4, 5])
    with pytest.raises(ValueError, match="more than once"):
        s.clone_envs([1, 2], [5, 5])
    with pytest.raises(ValueError, match="indices must lie"):
        s.clone_envs([1], [E])
    with pytest.raises(ValueError, match="indices must lie"):
        s.clone_envs([-1], [2])
    # device index lists: out-of-range entries are skipped and counted, the rest is copied
    before = s.get(*ALL)
    d_src = s.device_array((3,), np.int32)
    d_dst = s.device_array((3,), np.int32)
    d_src.upload(np.array([0, 99, 1], np.int32))
    d_dst.upload(np.array([44, 45, -3], np.int32))
    d_status = s.device_array((1,), np.int32)
    d_status.upload(np.zeros(1, np.int32))
    s.clone_envs(d_src, d_dst, d_status)
    assert int(d_status.download()[0]) == 2
    after = s.get(*ALL)
    for k in ALL:
        assert np.array_equal(after[k][rows(44)], before[k][rows(0)]), k
        keep = np.setdiff1d(np.arange(E * A), np.arange(44 * A, 45 * A))
        assert np.array_equal(after[k][keep], before[k][keep]), k
    # the device form of save / load counts the same way
    blob = s.save_envs(d_src, device=True)
    d_status.upload(np.zeros(1, np.int32))
    d_src.upload(np.array([0, 2, 2], np.int32))   # (entry 1 of the blob was skipped: nothing loads it)
    d_dst.upload(np.array([46, 47, 1000], np.int32))
    s.load_envs(blob, d_src, d_dst, d_status)
    assert int(d_status.download()[0]) == 1
    s.close()


def test_refusals(amd):
    s = _sim(amd, 4)
    s.reset(bench_start_poses(4, 2))
    blob = s.save_state()
    o = _sim(amd, 4, A=1)
    with pytest.raises(ValueError, match="agents per env"):
        o.load_state(blob)
    o.close()
    o = amd.BatchSim(num_envs=4, num_agents=2, num_beams=540)
    o.set_map_image(*load_map_image("example_map")); o.set_noise_rng(SEED, STD)
    with pytest.raises(ValueError, match="beams"):
        o.load_state(blob)
    o.close()
    o = _sim(amd, 4, noise=False)
    o.set_noise_rng(SEED + 1, STD)
    with pytest.raises(ValueError, match="different noise seed"):
        o.load_state(blob)
    o.close()
    o = _sim(amd, 4, noise=False)
    with pytest.raises(ValueError, match="noise"):
        o.load_state(blob)
    o.close()
    s.episode_init(0)
    s.episode_reset(bench_start_poses(4, 2))
    ep_blob = s.save_state(scans=False)
    o = _sim(amd, 4)
    with pytest.raises(ValueError, match="episode"):
        o.load_state(ep_blob)
    with pytest.raises(ValueError, match="episode"):
        o.load_envs(ep_blob, [0], [1])
    o.close()
    bad = ep_blob.data.copy()
    bad[0] = ord("X")
    with pytest.raises(ValueError, match="bad magic"):
        s.load_state(bad)
    blob2 = s.save_state()
    blob2.data[8] = 9   # the version, after the StateBlob was validated: the library refuses it too
    with pytest.raises(ValueError, match="format version 9"):
        s.load_state(blob2)
    with pytest.raises(ValueError, match="version"):
        s.load_envs(blob2, [0], [0])
    s.close()


def _tuples_equal(t1, t2, what):
    o1, r1, d1, i1 = t1
    o2, r2, d2, i2 = t2
    assert r1 == r2, what
    assert np.array_equal(np.asarray(d1), np.asarray(d2)), what + " done"
    for k in o1:
        if k == "ego_idx":
            continue
        assert np.array_equal(np.asarray(o1[k]), np.asarray(o2[k])), "%s obs %s" % (what, k)
    for k in i1:
        assert np.array_equal(np.asarray(i1[k]), np.asarray(i2[k])), "%s info %s" % (what, k)


def _copy(t):
    import copy
    return copy.deepcopy(t)


@pytest.mark.parametrize("kind", ["vec_host", "vec_device", "sharded"])
def test_env_layers_snapshot_restore(amd, kind):
    E, A, T = 7, 2, 100
    kw = dict(map=map_stem("example_map"), map_ext=".png", num_agents=A, auto_reset=True)
    if kind == "sharded":
        env = amd.ShardedVecEnv(E, devices=[0, 0, 0], device_logic=True, **kw)
    else:
        env = amd.F110VecEnv(E, device_logic=(kind == "vec_device"), **kw)
    poses = bench_start_poses(E, A, gap_wp=4).reshape(E, A, 3)
    env.reset(poses)
    acts = _actions(2 * T, E, A, seed=31).reshape(2 * T, E, A, 2)
    for t in range(T // 2):
        last = _copy(env.step(acts[t]))
    snap = env.snapshot()
    first = [_copy(env.step(acts[t])) for t in range(T // 2, T // 2 + T)]
    back = env.restore(snap)
    _tuples_equal(back, last, "%s restore" % kind)
    second = [_copy(env.step(acts[t])) for t in range(T // 2, T // 2 + T)]
    for t, (a, b) in enumerate(zip(first, second)):
        _tuples_equal(a, b, "%s step %d" % (kind, t))
    if hasattr(env, "close"):
        env.close()
