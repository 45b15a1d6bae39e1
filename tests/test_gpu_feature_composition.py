"""The observation features together: one env with the reset sampler, the progress reward, a scripted car, the
observation encoder, the track preview and the neighbours all on, held bitwise to envs that turn on one of them (or none), and each
block held to its model by the rules of its own test file (imported from there: encoded bit for bit, preview and neighbours the
model's value or its float32 neighbour with the exact channels bit for bit, at most 1 in 1000 different).  Then the same through
snapshot / restore, shards, the single env, and the device-resident loop that issues all five calls back to back behind a
two-block step.

Comparisons between device runs are made on the bytes (`_bits`): NaN payloads and the sign of zero count."""
import numpy as np
import pytest

import gap_follower_ref as gap_ref
import obs_encoder_ref as enc_ref
import track_preview_ref as prv_ref
from _util import bench_start_poses, load_map_image, map_stem
from test_gpu_neighbors import _check_device as nbr_check_device
from test_gpu_neighbors import _check_obs as nbr_check_obs
from test_gpu_neighbors import _rows as nbr_rows
from test_gpu_obs_encoder import _columns as enc_columns
from test_gpu_obs_encoder import _same_bits as enc_same_bits
from test_gpu_track_preview import _check_device as prv_check_device
from test_gpu_track_preview import _check_obs as prv_check_obs
from test_gpu_track_preview import _pose_and_s

pytestmark = pytest.mark.gpu

SEED, STD = 4242, 0.01
SCALES = {"vx": 8.0, "steer": 0.4189, "yaw_rate": 3.2, "slip": -0.7, "collision": 1.0, "lateral": 1.5, "heading_error": 3.0, "ds": 0.2}
ENC = dict(sectors=36, pool="min", features=enc_ref.FEATURES, frames=4, scales=SCALES)
PRV = dict(points=6, offset=0.3, spacing=0.7, channels=("x", "y", "tan_x", "tan_y", "attr0", "attr1"), frame="ego", scale={"attr1": 8.0})
NBR = dict(k=2, channels=("dx", "dy", "dist", "v_x", "gap_s", "valid", "index"), max_range=6.0, pad=-1.0, scale={"gap_s": 8.0})
SAMPLER = dict(seed=31, lateral=0.2, heading=0.1)
OPTIONS = {"encoded": "obs_encoder", "track_preview": "track_preview", "neighbors": "neighbors"}   # obs key -> constructor option


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def race():
    """the example raceline with two attribute columns (kappa, vx): the model's tables, the points, the attribute rows"""
    return prv_ref.example_raceline(True, 2)


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs hit the walls within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.dtype.str, a.shape, a.tobytes()


def _same(a, b, what):
    assert _bits(a) == _bits(b), "%s differs" % what


def _same_step(a, b, what, keys=None):
    """every field of the (obs, reward, done, info) tuple `b` (or the obs keys named) is in `a` with the same bytes"""
    for k in (b[0] if keys is None else keys):
        _same(a[0][k], b[0][k], "%s: obs[%r]" % (what, k))
    if keys is None:
        _same(a[1], b[1], "%s: reward" % what)
        _same(a[2], b[2], "%s: done" % what)
        for k in b[3]:
            _same(a[3][k], b[3][k], "%s: info[%r]" % (what, k))


def _copy_step(r):
    cp = lambda v: np.array(v, copy=True) if isinstance(v, np.ndarray) else v
    return ({k: cp(v) for k, v in r[0].items()}, cp(r[1]), cp(r[2]), {k: cp(v) for k, v in r[3].items()})


def _env_kw(amd, race, A):
    tab, xy, attrs = race
    return dict(auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png", num_agents=A,
                track=amd.Track(xy, closed=True, attrs=attrs), reward="progress", random_start=dict(SAMPLER),
                scripted={1: amd.GapFollower()})


def _all_on(amd):
    return dict(obs_encoder=amd.ObsEncoder(**ENC), track_preview=amd.TrackPreview(**PRV), neighbors=amd.Neighbors(**NBR))


# ---- 1. F110VecEnv with everything on against each option alone ------------------------------------------------------------------
@pytest.mark.parametrize("E,A", [(64, 2), (48, 3)])
def test_vec_env_all_options_equal_each_option_alone(amd, race, E, A):
    tab = race[0]
    T = 150
    opts = _all_on(amd)
    enc, prv, nbr = opts["obs_encoder"], opts["track_preview"], opts["neighbors"]
    kw = _env_kw(amd, race, A)
    full = amd.F110VecEnv(E, **dict(kw, **opts))
    plain = amd.F110VecEnv(E, **kw)
    alone = {key: amd.F110VecEnv(E, **dict(kw, **{opt: opts[opt]})) for key, opt in OPTIONS.items()}
    others = [plain] + list(alone.values())
    b = full.sim.batch
    L = full.tracks[0].length
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    state = {"stack": np.zeros(enc.shape(E * A), np.float32), "fill": True, "prev_sc": None}
    count = {"zeros": 0, "ones_after_zero": 0, "dones": 0, "prv": 0, "nbr": 0, "sampled": 0}

    def check(got, rest, what, models):
        assert sorted(got[0]) == sorted(list(rest[0][0]) + list(OPTIONS))
        _same_step(got, rest[0], what + ", against the plain env")
        for key, r in zip(OPTIONS, rest[1:]):
            assert sorted(r[0]) == sorted(list(rest[0][0]) + [key])
            _same_step(got, r, what + ", against the env with %s alone" % OPTIONS[key])
        # the encoder's model follows every step (its stack is state); it is compared where the other two are
        scans, cols, sc = enc_columns(b, True)
        state["stack"] = enc_ref.encode(enc, scans, cols, sc, state["stack"], fill=state["fill"])
        state["fill"] = False
        count["zeros"] += int(np.sum(sc == 0))
        if state["prev_sc"] is not None:
            count["ones_after_zero"] += int(np.sum((state["prev_sc"] == 0) & (sc == 1)))
        state["prev_sc"] = sc
        count["dones"] += int(np.sum(got[2]))
        if models:
            enc_same_bits(np.asarray(got[0]["encoded"]).reshape(state["stack"].shape), state["stack"], what + ": encoded")
            count["prv"] += prv_check_obs(tab, prv, got[0], what + ": track_preview", b)
            count["nbr"] += nbr_check_obs(nbr, got[0], b, L, what + ": neighbors")
            count["sampled"] += 1

    check(full.reset(start), [e.reset(start) for e in others], "reset", True)
    for t in range(T):
        if t == 70:      # a reset() without poses in mid-run: every env draws its start poses
            check(full.reset(), [e.reset() for e in others], "reset() at step %d" % t, True)
        if t % 3 == 2:
            full.step_async(acts[t])
            got = full.step_wait()
        else:
            got = full.step(acts[t])
        check(got, [e.step(acts[t]) for e in others], "step %d%s" % (t, " (step_async / step_wait)" if t % 3 == 2 else ""), t % 10 == 9)
    assert count["zeros"] >= 20 and count["ones_after_zero"] >= 20, "too few re-seats to test the composition where it matters: %r" % (count,)
    assert count["dones"] > 5 and count["sampled"] == 17
    N = E * A
    assert count["prv"] * 1000 <= count["sampled"] * N * prv.points * prv.dim and count["nbr"] * 1000 <= count["sampled"] * N * nbr.k * nbr.dim, count


# ---- 2. snapshot and restore ---------------------------------------------------------------------------------------------------------
def test_vec_env_all_options_snapshot_restore(amd, race):
    E, A = 32, 2
    env = amd.F110VecEnv(E, **dict(_env_kw(amd, race, A), **_all_on(amd)))
    acts = _crash_actions(50, E * A, seed=9).reshape(50, E, A, 2)
    env.reset()
    for t in range(20):
        at_snap = _copy_step(env.step(acts[t]))
    snap = env.snapshot()
    first = [_copy_step(env.step(acts[20 + t])) for t in range(30)]
    assert any(_bits(first[-1][0][k]) != _bits(at_snap[0][k]) for k in OPTIONS)      # (the views have moved on)
    back = env.restore(snap)
    _same_step(back, at_snap, "right after restore()")                               # the three blocks are back in the views
    _same(env.encoded_stack.download(), at_snap[0]["encoded"].reshape(env.encoded_stack.shape), "the restored device stack")
    for t in range(30):
        _same_step(env.step(acts[20 + t]), first[t], "step %d after restore()" % t)
    assert sum(int(np.sum(r[2])) for r in first) >= 1


# ---- 3. shards ---------------------------------------------------------------------------------------------------------------------------
def test_sharded_all_options_equal_one_handle(amd, race):
    E, A, T = 31, 2, 60
    kw = dict(_env_kw(amd, race, A), **_all_on(amd))
    one = amd.F110VecEnv(E, **kw)
    del kw["device_logic"]
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], **kw)
    assert sh.shard_sizes == [11, 10, 10]
    mask = np.zeros(E, dtype=bool)
    mask[11:21] = True                                     # exactly the second shard
    acts = _crash_actions(T, E * A, seed=10).reshape(T, E, A, 2)
    _same_step(sh.reset(), one.reset(), "reset")
    assert sh.reset()[0]["encoded"].shape == one.reset()[0]["encoded"].shape == (E, A, 4, 44)
    for t in range(T):
        if t == 30:
            _same_step(sh.reset(env_mask=mask), one.reset(env_mask=mask), "partial reset")
        a, b = sh.step(acts[t]), one.step(acts[t])
        assert sorted(a[0]) == sorted(b[0])
        _same_step(a, b, "step %d" % t)
    sh.close()


# ---- 4. the single env ---------------------------------------------------------------------------------------------------------------------
def test_single_env_preview_and_neighbors_together(amd, race):
    tab, xy, attrs = race
    prv, nbr = amd.TrackPreview(**PRV), amd.Neighbors(**NBR)
    mk = lambda **kw: amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, track=amd.Track(xy, closed=True, attrs=attrs), **kw)
    both, plain = mk(track_preview=prv, neighbors=nbr), mk()
    alone = {"track_preview": mk(track_preview=prv), "neighbors": mk(neighbors=nbr)}
    start = bench_start_poses(1, 2)
    acts = _crash_actions(100, 2, seed=4) * np.array([1.0, 0.5])
    outs = [e.reset(start) for e in [both, plain] + list(alone.values())]
    for t in range(101):
        got, base = outs[0], outs[1]
        assert sorted(got[0]) == sorted(list(base[0]) + ["neighbors", "track_preview"])
        for k in base[0]:
            _same(np.asarray(got[0][k]), np.asarray(base[0][k]), "step %d: obs[%r]" % (t, k))
        assert got[1] == base[1] and got[2] == base[2]
        for key, o in zip(alone, outs[2:]):
            _same(got[0][key], o[0][key], "step %d: %s against the env with it alone" % (t, key))
        # the one-launch step (k_step_tiny; with a track its projection runs in front of and behind it) still applies with both
        # calls behind it: f110_step_launches is 0 for the per-kernel form
        assert both.sim.batch.step_launches() == plain.sim.batch.step_launches() >= 1, t
        if t < 100:
            outs = [e.step(acts[t]) for e in [both, plain] + list(alone.values())]
    # the observation's pose (agent_poses: the heading a car that hit a wall arrived with, which obs['poses_theta'] shows as 0)
    obs = outs[0][0]
    poses, arc = _pose_and_s(both.sim.batch)
    _same(arc, np.asarray(obs["progress"]), "progress")
    prv_check_device(tab, prv, poses, arc, obs["track_preview"], "F110Env")
    nbr_check_device(nbr, nbr_rows(both.sim.batch), 2, both.track.length, obs["neighbors"], "F110Env")


# ---- 5. the device-resident loop behind a two-block step -------------------------------------------------------------------------------
def _loop_handle(amd, race, E, A, groups):
    tab, xy, attrs = race
    s = amd.BatchSim(num_envs=E, num_agents=A, step_groups=groups)
    s.set_map_image(*load_map_image("example_map"))
    s.set_noise_rng(SEED, STD)
    s.set_track(amd.Track(xy, closed=True, attrs=attrs))
    s.enable_track()
    s.set_reset_sampler(**SAMPLER)
    start = bench_start_poses(E, A)
    s.episode_init(0)
    s.episode_reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    s.set_auto_reseat(d_start, 0)
    d_act = s.device_array((E * A, 2))
    s._keep = (d_start, d_act)   # (the armed re-seat reads d_start: it lives with the handle)
    return s, d_act


def _loop_state(s):
    o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
    o.update({"track_" + k: v for k, v in s.get_track().items()})
    o.update({"episode_" + k: v for k, v in s.episode_get().items()})
    o = {k: np.array(v, copy=True) for k, v in o.items()}
    o["blob"] = np.frombuffer(s.save_state(scans=True).to_bytes(), dtype=np.uint8)
    return o


def test_device_loop_all_calls_behind_two_blocks(amd, race):
    """follow_gap_device, episode_step_device, encode_obs_device, track_preview_device, neighbors_device back to back, 60 times,
    one sync() at the end: with step_groups=2 every call rides the blocks' streams and the step stays two blocks; the results are
    those of one block.  A third handle takes the same 60 steps with none of the four follow-up calls: its scripted rows come
    from the unit form of the controller on the downloaded scans (a sample of them held to the model), and it supplies the
    columns the encoder's model is fed step by step."""
    tab = race[0]
    E, A, T = 512, 2, 60
    N = E * A
    enc, prv, nbr = amd.ObsEncoder(**ENC), amd.TrackPreview(**PRV), amd.Neighbors(**NBR)
    g = amd.GapFollower()
    assign = np.tile([-1, 0], E).astype(np.int32)            # slot 1 of every env drives itself
    ext = np.random.default_rng(3)                           # the external rows: written once, hard steering at speed
    acts = np.stack([ext.uniform(-0.42, 0.42, N), ext.uniform(4.0, 12.0, N)], axis=1)
    res = {}
    for groups in (1, 2):
        s, d_act = _loop_handle(amd, race, E, A, groups)
        s.set_controllers(assign, [g])
        out = {"encoded": s.device_array(enc.shape(N), np.float32), "track_preview": s.device_array(prv.shape(N), np.float32),
               "neighbors": s.device_array(nbr.shape(N), np.float32)}
        pin = {k: s.pinned_empty(v.shape, np.float32) for k, v in out.items()}
        for p in pin.values():
            p[...] = 0.0
        d_act.upload(acts)
        blocks, launches = [], set()
        for t in range(T):
            s.follow_gap_device(d_act)
            s.episode_step_device(d_act)
            blocks.append(s.step_groups()[2])
            launches.add(s.step_launches())
            s.encode_obs_device(enc, out["encoded"], fill=(t == 0), pinned=pin["encoded"])
            s.track_preview_device(prv, out["track_preview"], pinned=pin["track_preview"])
            s.neighbors_device(nbr, out["neighbors"], pinned=pin["neighbors"])
        assert s.step_groups()[0] == groups and s.step_groups()[2] == groups, "the handle reports %r after the loop" % (s.step_groups(),)
        s.sync()
        assert all(n == groups for n in blocks), "a step went out as another number of blocks: %r" % (blocks,)
        r = _loop_state(s)
        r["actions"] = d_act.download()
        for k in out:
            r[k] = out[k].download()
            _same(np.array(pin[k]), r[k], "groups=%d: the pinned copy of %s" % (groups, k))
        r["rows"], r["pose_s"] = nbr_rows(s), _pose_and_s(s)
        res[groups] = (r, blocks, launches)
        s.close()
    one, two = res[1][0], res[2][0]
    for k in one:
        if k not in ("rows", "pose_s"):
            _same(two[k], one[k], "two blocks against one: %s" % k)
    # f110_step_launches counts the one-launch form only: both handles took the per-kernel form, in one block and in two
    assert res[1][2] == res[2][2] == {0}
    # the third handle: no follow-up call at all
    s, d_act = _loop_handle(amd, race, E, A, 1)
    unit = amd.BatchSim(num_envs=1, num_agents=1)            # (the controller's unit form: no map, its own handle)
    model = gap_ref.settings(**g.settings())
    stack = np.zeros(enc.shape(N), np.float32)
    scripted = np.flatnonzero(assign >= 0)
    rng = np.random.default_rng(17)
    reseats = first_steps = 0
    prev_sc = None
    for t in range(T):
        o = s.get("scans", "step_count")
        a = acts.copy()
        a[scripted] = unit.follow_gap(o["scans"][scripted], g, o["step_count"][scripted])
        pick = np.concatenate([rng.choice(E // 2, 4, replace=False), E // 2 + rng.choice(E // 2, 4, replace=False)]) * A + 1
        want = gap_ref.follow(model, o["scans"][pick], o["step_count"][pick])[0]
        assert _bits(a[pick]) == _bits(want), "step %d: the unit form differs from the controller's model" % t
        d_act.upload(a)
        s.episode_step_device(d_act)
        scans, cols, sc = enc_columns(s, True)
        stack = enc_ref.encode(enc, scans, cols, sc, stack, fill=(t == 0))
        reseats += int(np.sum(sc == 0))
        if prev_sc is not None:
            first_steps += int(np.sum((prev_sc == 0) & (sc == 1)))
        prev_sc = sc
    bare = _loop_state(s)
    bare["actions"] = d_act.download()
    s.close()
    unit.close()
    for k in bare:
        _same(one[k], bare[k], "the loop with every follow-up call against the loop with none: %s" % k)
    assert reseats >= 20 and first_steps >= 20, "too few re-seats in the loop (%d, %d)" % (reseats, first_steps)
    # the three outputs of the final step against the models
    enc_same_bits(one["encoded"], stack, "the device loop's final stack")
    poses, arc = one["pose_s"]
    differ = total = 0
    differ += prv_check_device(tab, prv, poses, arc, one["track_preview"], "the final preview")      # every agent of both blocks
    differ += nbr_check_device(nbr, one["rows"], A, tab.L, one["neighbors"], "the final neighbours")
    total += N * (prv.points * prv.dim + nbr.k * nbr.dim)
    assert differ * 1000 <= total, (differ, total)
