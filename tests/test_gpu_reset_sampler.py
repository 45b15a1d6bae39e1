"""Randomised start poses on the device (f110_reset_sampler_*) against the NumPy model tests/reset_sampler_ref.py:
explicit draws bit for bit, drawn resets as real resets, in-step draws on every re-seat path, env blocks, shards, snapshots and
clones, per-slot tracks, the device episode logic, and nothing changed with the sampler off."""
import os

import numpy as np
import pytest

from _util import MAPS, bench_start_poses, load_map_image, map_stem, oracle_map_dt, raceline
from reset_sampler_ref import SamplerModel, SlotModel, wrap_diff

pytestmark = pytest.mark.gpu

CSV = os.path.join(MAPS, "example_waypoints.csv")
SEED, STD = 4242, 0.01
CLEAR = float(np.sqrt(0.58 ** 2 + 0.31 ** 2) / 2)


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _track(amd, xy=None):
    return amd.Track.from_xy(raceline()[:, 1:3] if xy is None else xy)


def _slot(amd, xy=None):
    dt, res, origin = oracle_map_dt("example_map")
    return SlotModel(_track(amd, xy), dt, res, origin)


def _sim(amd, E, A=2, sampler=None, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    s.set_noise_rng(SEED, STD)
    s.set_track(_track(amd))
    if sampler is not None:
        s.set_reset_sampler(**sampler)
    return s


def _obs(s):
    o = s.get("state", "scans", "collisions", "in_collision", "step_count")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def _same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s %s differs" % (what, k)


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs crash within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


def _within_ulp(got, want):
    """|got - want| at most one ulp of the larger magnitude, elementwise"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.all(np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want))))


def _check_poses(got, want, what):
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    np.testing.assert_array_equal(got[:, :2], want[:, :2], err_msg=what + " x, y")
    assert np.all(np.abs(wrap_diff(got[:, 2], want[:, 2])) <= 1e-15), what + " theta"


@pytest.mark.parametrize("A", [1, 2, 3])
def test_sample_reset_matches_model_bitwise(amd, A):
    E = 512
    cfg = dict(seed=SEED, lateral=0.3, heading=0.2)
    s = _sim(amd, E, A, sampler=cfg)
    s.sample_reset()
    st = s.reset_sampler_stats(attempts=True)
    got = s.get("state")["state"]
    m = SamplerModel(SEED, E, A, [_slot(amd)], lateral=0.3, heading=0.2, clearance=CLEAR)
    want, att = np.zeros((E, A, 3)), np.empty(E, dtype=np.int64)
    for e in range(E):
        p, att[e] = m.draw(e)
        if p is not None:
            want[e] = p
    np.testing.assert_array_equal(st["attempt"], att)
    assert st["draws"] == E and st["fallbacks"] == int(np.sum(att < 0))
    pose = np.stack([got[:, 0], got[:, 1], got[:, 4]], axis=1)
    _check_poses(pose, want, "A=%d" % A)
    _check_poses(s.reset_sampler_poses(), want, "fallback buffer")
    # a second draw continues each env's stream
    s.sample_reset(np.arange(E) % 2 == 0)
    got2 = s.get("state")["state"]
    for e in range(0, E, 2):
        p, _ = m.draw(e)
        if p is not None:
            _check_poses(np.stack([got2[e * A:(e + 1) * A, 0], got2[e * A:(e + 1) * A, 1], got2[e * A:(e + 1) * A, 4]], 1), p, "2nd")
    s.close()


def test_drawn_reset_is_a_real_reset(amd):
    E, A = 64, 2
    s1 = _sim(amd, E, A, sampler=dict(seed=9, lateral=0.2, heading=0.1))
    s1.sample_reset()
    poses = s1.reset_sampler_poses()
    s2 = _sim(amd, E, A)
    s2.reset(poses)
    acts = _crash_actions(50, E * A, seed=5) * np.array([0.5, 0.5])
    for t in range(50):
        s1.step(acts[t])
        s2.step(acts[t])
        _same(_obs(s1), _obs(s2), "step %d" % t)
    s1.close()
    s2.close()


def _episode_model(amd, E, A, seed):
    return SamplerModel(seed, E, A, [_slot(amd)], clearance=CLEAR)


def _run_in_step(amd, form, E=256, A=2, T=300, step_groups=0):
    """the start poses each env receives over T crashing steps, per env a list; and the handle + a twin without sampler"""
    s = _sim(amd, E, A, sampler=dict(seed=77), step_groups=step_groups)
    twin = _sim(amd, E, A, step_groups=step_groups)
    start = bench_start_poses(E, A)
    for h in (s, twin):
        if form in ("episode", "host_block", "episode_host"):
            h.episode_init(0)
            h.episode_reset(start)
        else:
            h.reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    d_start2 = twin.device_array((E * A, 3))
    d_start2.upload(start)
    if form == "auto":
        s.set_auto_reseat(d_start, 0)
        twin.set_auto_reseat(d_start2, 0)
    d_act = s.device_array((E * A, 2))
    d_act2 = twin.device_array((E * A, 2))
    s._keep, twin._keep = (d_start, d_act), (d_start2, d_act2)   # (the armed re-seat reads d_start: it lives with the handle)
    acts = _crash_actions(T, E * A)
    received = [[] for _ in range(E)]
    reseated = np.zeros(E, dtype=bool)
    hb = s.host_block(["state", "done"]) if form == "host_block" else None
    if form == "episode_host":
        act_pin = s.pinned_empty((E * A, 2))
        packed = s.pinned_empty((s.packed_bytes(),), np.uint8)
    for t in range(T):
        d_act.upload(acts[t])
        d_act2.upload(acts[t])
        if form == "auto":
            s.step_device(d_act)
            twin.step_device(d_act2)
        elif form == "collided":
            s.step_device(d_act)
            twin.step_device(d_act2)
            s.reset_collided_device(d_start, 0)
            twin.reset_collided_device(d_start2, 0)
        elif form == "episode":
            s.episode_step_device(d_act)
            twin.episode_step_device(d_act2)
            s.episode_reset_done_device()
            twin.episode_reset_done_device()
        elif form == "episode_host":
            act_pin[...] = acts[t]
            s.episode_step_host(act_pin, packed, auto_reset=True)
        else:
            hb.actions[...] = acts[t]
            s.step_host(hb, None, auto_reset=True)
        o = s.get("state", "step_count")
        sc = o["step_count"].reshape(E, A)[:, 0]
        for e in np.flatnonzero(sc == 0):
            st = o["state"][e * A:(e + 1) * A]
            received[e].append(np.stack([st[:, 0], st[:, 1], st[:, 4]], axis=1))
            reseated[e] = True
        if form not in ("host_block", "episode_host"):   # (the twin of these two forms is not stepped)
            a, b = _obs(s), _obs(twin)
            fresh = np.repeat(~reseated, A)
            for k in ("state", "scans", "collisions"):
                assert np.array_equal(a[k][fresh], b[k][fresh]), "%s: env not yet re-seated differs (%s, step %d)" % (form, k, t)
    return s, twin, received


@pytest.mark.parametrize("form", ["auto", "collided", "episode", "host_block", "episode_host"])
def test_in_step_draws_follow_the_model(amd, form):
    E, A = 256, 2
    s, twin, received = _run_in_step(amd, form, E, A)
    m = _episode_model(amd, E, A, 77)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    n = 0
    for e in range(E):
        prev = start[e]
        for got in received[e]:
            p, _ = m.draw(e)
            want = prev if p is None else p
            _check_poses(got, want, "%s env %d" % (form, e))
            if form in ("episode", "host_block", "episode_host"):
                prev = want
            n += 1
    assert n >= 50, "the policy crashed too rarely (%d re-seats)" % n
    if form in ("episode", "host_block", "episode_host"):   # start_poses / start_rot of the episode logic follow the draws
        v = s.episode_device_views()
        sp = v["start_poses"].download().reshape(E, A, 3)
        rot = v["start_rot"].download()
        for e in range(E):
            want = received[e][-1] if received[e] else start[e]
            _check_poses(sp[e], want, "start_poses")
            th = -sp[e, 0, 2]
            assert _within_ulp(rot[e], [np.cos(th), -np.sin(th), np.sin(th), np.cos(th)]), "start_rot of env %d" % e
    s.close()
    twin.close()


@pytest.mark.parametrize("form", ["auto", "episode"])
def test_step_groups_two_blocks_equal_one(amd, form):
    """the in-step draw behind a two-block step (f110_step_device with f110_set_auto_reseat, f110_episode_step_device +
    f110_episode_reset_done_device) draws in every block what one block draws"""
    s1, t1, r1 = _run_in_step(amd, form, 512, 2, T=120, step_groups=1)
    s2, t2, r2 = _run_in_step(amd, form, 512, 2, T=120, step_groups=2)
    assert s1.step_groups()[2] == 1 and s2.step_groups()[2] == 2   # (blocks of the most recent step)
    _same(_obs(s1), _obs(s2), "two blocks")
    assert sum(len(a) for a in r1) >= 50
    for a, b in zip(r1, r2):
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
    for h in (s1, t1, s2, t2):
        h.close()


def _vec(amd, E, device_logic, **kw):
    return amd.F110VecEnv(E, auto_reset=True, device_logic=device_logic, map=map_stem("example_map"), map_ext=".png",
                          track=CSV, random_start=dict(seed=31, lateral=0.2, heading=0.1), **kw)


def test_vec_env_paths_and_shards_agree(amd):
    E, A, T = 96, 2, 200
    envs = [_vec(amd, E, True), _vec(amd, E, False),
            amd.ShardedVecEnv(E, devices=[0, 0], shard_sizes=[37, 59], auto_reset=True, map=map_stem("example_map"),
                              map_ext=".png", track=CSV, random_start=dict(seed=31, lateral=0.2, heading=0.1))]
    first = [env.reset()[0] for env in envs]
    m = SamplerModel(31, E, A, [_slot(amd)], lateral=0.2, heading=0.1, clearance=CLEAR)
    want0 = np.stack([m.draw(e)[0] for e in range(E)])
    _check_poses(envs[0].sim.batch.reset_sampler_poses(), want0, "first draw")
    for o in first[1:]:
        np.testing.assert_array_equal(o["poses_x"], first[0]["poses_x"])
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    dones = 0
    for t in range(T):
        outs = [env.step(acts[t]) for env in envs]
        for o, r, d, i in outs[1:]:
            np.testing.assert_array_equal(o["poses_x"], outs[0][0]["poses_x"])
            np.testing.assert_array_equal(o["poses_y"], outs[0][0]["poses_y"])
            np.testing.assert_array_equal(d, outs[0][2])
        dones += int(np.sum(outs[0][2]))
    assert dones > 20
    envs[2].close()


def test_snapshot_restore_and_clone_continue_draws(amd):
    E, A = 128, 2
    s, twin, _ = _run_in_step(amd, "auto", E, A, T=60)
    blob = s.save_state()
    d_act = s.device_array((E * A, 2))
    acts = _crash_actions(80, E * A, seed=12)
    seq = []
    for t in range(80):
        d_act.upload(acts[t])
        s.step_device(d_act)
        seq.append(_obs(s))
    s.load_state(blob)
    for t in range(80):
        d_act.upload(acts[t])
        s.step_device(d_act)
        _same(_obs(s), seq[t], "restored step %d" % t)
    # a blob with the sampler column is refused without a sampler, and the other way round
    with pytest.raises(ValueError, match="reset sampler"):
        twin.load_state(blob)
    with pytest.raises(ValueError, match="reset sampler"):
        s.load_state(twin.save_state())
    # clones draw what their source draws
    s.clone_envs(list(range(0, 64)), list(range(64, 128)))
    s.sample_reset()
    p = s.reset_sampler_poses().reshape(E, A, 3)
    np.testing.assert_array_equal(p[:64], p[64:])
    s.close()
    twin.close()


def test_two_slots_draw_on_their_own_tracks(amd):
    """slot 1 is example_map moved by `off` with the raceline moved along: a draw that read slot 0's table (or track) for
    an env of slot 1 would test other cells, and the winning attempts would differ"""
    E, A = 256, 2
    off = np.array([3.0, -2.0])
    img, res, origin = load_map_image("example_map")
    origin1 = [origin[0] + off[0], origin[1] + off[1], origin[2]]
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(img, res, origin)
    s.add_map_image(img, res, origin1)
    s.set_track(_track(amd))
    env_slot = np.arange(E) % 2
    s.set_env_maps(env_slot)
    with pytest.raises(amd._ffi.F110LibraryError, match="no track"):   # slot 1 has no track: F110_ERR_STATE
        s.set_reset_sampler(5)
    xy1 = raceline()[:, 1:3] + off
    s.set_track(_track(amd, xy1), slot=1)
    cfg = dict(lateral=1.2, heading=0.2, clearance=0.45)
    s.set_reset_sampler(5, **cfg)
    s.sample_reset()
    st = s.reset_sampler_stats(attempts=True)
    got = s.get("state")["state"]
    dt, _, _ = oracle_map_dt("example_map")
    slots = [_slot(amd), SlotModel(_track(amd, xy1), dt, res, origin1)]
    m = SamplerModel(5, E, A, slots, env_slot=env_slot, **cfg)
    wrong = SamplerModel(5, E, A, [slots[0], SlotModel(_track(amd, xy1), dt, res, origin)], env_slot=env_slot, **cfg)
    att = np.empty(E, dtype=np.int64)
    differs = 0
    for e in range(E):
        p, att[e] = m.draw(e)
        differs += int(wrong.draw(e)[1] != att[e])
        if p is not None:
            _check_poses(np.stack([got[e * A:(e + 1) * A, 0], got[e * A:(e + 1) * A, 1], got[e * A:(e + 1) * A, 4]], 1), p,
                         "slot %d" % env_slot[e])
    np.testing.assert_array_equal(st["attempt"], att)
    assert differs > 0 and np.any(att[env_slot == 1] > 0)   # (the table decides attempts here: the check has teeth)
    s.close()


def test_sampler_off_and_cleared_change_nothing(amd):
    E, A = 64, 2
    a, b = _sim(amd, E, A), _sim(amd, E, A, sampler=dict(seed=1))
    b.clear_reset_sampler()
    start = bench_start_poses(E, A)
    for h in (a, b):
        h.episode_init(0)
        h.episode_reset(start)
    hbs = [h.host_block(["state", "done"]) for h in (a, b)]
    acts = _crash_actions(60, E * A, seed=2)
    for t in range(60):
        for h, hb in zip((a, b), hbs):
            hb.actions[...] = acts[t]
            h.step_host(hb, None, auto_reset=True)
        assert a.step_launches() == b.step_launches()
        _same(_obs(a), _obs(b), "cleared step %d" % t)
    assert len(a.save_state().to_bytes()) == len(b.save_state().to_bytes())
    a.close()
    b.close()


def test_f110env_random_start(amd):
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, track=CSV, random_start=dict(seed=21))
    obs, _, _, _ = env.reset()
    m = SamplerModel(21, 1, 2, [_slot(amd)], clearance=CLEAR)
    p, _ = m.draw(0)
    _check_poses(env.sim.batch.reset_sampler_poses(), p, "F110Env")
    np.testing.assert_array_equal(env.start_xs, p[:, 0])
    poses = bench_start_poses(1, 2)
    ref = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, track=CSV)
    o1, _, _, _ = env.reset(poses)
    o2, _, _, _ = ref.reset(poses)
    np.testing.assert_array_equal(o1["poses_x"], o2["poses_x"])
    np.testing.assert_array_equal(o1["scans"], o2["scans"])


@pytest.mark.parametrize("form", ["collided", "episode"])
def test_standalone_reseat_right_after_host_reset_draws_only_its_envs(amd, form):
    """f110_reset_collided_device / f110_episode_reset_done_device with no step since a host reset: the host-reset envs
    (step_count 0 too) must not draw; only the envs the call itself re-seats do"""
    E, A = 128, 2
    s = _sim(amd, E, A, sampler=dict(seed=55))
    start = bench_start_poses(E, A)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    if form == "episode":
        s.episode_init(0)
        s.episode_reset(start)
    else:
        s.reset(start)

    def standalone():
        if form == "collided":
            s.reset_collided_device(d_start, 0)
        else:
            s.episode_reset_done_device()

    def poses():
        st = s.get("state")["state"]
        return np.stack([st[:, 0], st[:, 1], st[:, 4]], axis=1).reshape(E, A, 3)

    standalone()   # 1) right after a full host reset nothing is re-seated, nothing draws
    assert s.reset_sampler_stats()["draws"] == 0
    np.testing.assert_array_equal(poses(), start.reshape(E, A, 3))
    # 2) step until some envs are flagged, host-reset the others, then the standalone call with no step in between
    d_act = s.device_array((E * A, 2))
    acts = _crash_actions(200, E * A, seed=6)
    flagged = np.zeros(E, dtype=bool)
    for t in range(200):
        d_act.upload(acts[t])
        if form == "collided":
            s.step_device(d_act)
            flagged = s.get("collisions")["collisions"].reshape(E, A)[:, 0] != 0
        else:
            s.episode_step_device(d_act)
            flagged = s.episode_get()["done"] != 0
        if flagged.sum() >= 8:
            break
    assert 0 < flagged.sum() < E
    if form == "collided":
        s.reset(start, ~flagged)
    else:
        s.episode_reset(start, ~flagged)
    before = poses()
    s.reset_sampler_stats(clear=True)
    standalone()
    st = s.reset_sampler_stats(attempts=True)
    assert st["draws"] == int(flagged.sum())
    after = poses()
    np.testing.assert_array_equal(after[~flagged], start.reshape(E, A, 3)[~flagged])
    np.testing.assert_array_equal(before[~flagged], after[~flagged])
    m = SamplerModel(55, E, A, [_slot(amd)], clearance=CLEAR)
    for e in np.flatnonzero(flagged):
        p, a = m.draw(e)
        assert st["attempt"][e] == a
        _check_poses(after[e], start.reshape(E, A, 3)[e] if p is None else p, "env %d" % e)
    s.close()


def _lap_margin(lap, px, py):
    """per env, the smallest |dist2 - 0.1| over its agents of the update lap.update(px, py, ...) is about to make"""
    px = np.asarray(px).reshape(lap.E, lap.A) - lap.start_xs
    py = np.asarray(py).reshape(lap.E, lap.A) - lap.start_ys
    c, s = lap.rot_c[:, None], lap.rot_s[:, None]
    dx = c * px + (-s) * py
    ty = s * px + c * py
    ty = np.where(ty > 2, ty - 2, np.where(ty < -2, -2 - ty, 0.0))
    return np.min(np.abs(dx ** 2 + ty ** 2 - 0.1), axis=1)


def test_device_episode_logic_after_draws_matches_lap_logic(amd):
    """done and the toggles of the device episode logic, across in-step draws, against the host _LapLogic fed the same start
    poses (start_rot there is NumPy's); a step whose dist2 <= 0.1 decision is within 1e-12 is skipped and re-synced"""
    from f1tenth_gym_amd.env import _LapLogic
    E, A, T = 128, 2, 400
    s = _sim(amd, E, A, sampler=dict(seed=66, lateral=0.2, heading=0.1))
    start = bench_start_poses(E, A)
    s.episode_init(0)
    s.episode_reset(start)
    lap = _LapLogic(E, A, 0)
    lap.reset(start.reshape(E, A, 3))
    d_act = s.device_array((E * A, 2))
    rng = np.random.default_rng(9)
    acts = np.stack([rng.uniform(-0.3, 0.3, (T, E * A)), rng.uniform(2.0, 7.0, (T, E * A))], axis=2)
    compared = draws = skipped = 0
    for t in range(T):
        d_act.upload(acts[t])
        s.episode_step_device(d_act)
        o = s.get("state", "collisions")
        ep = s.episode_get()
        margin = _lap_margin(lap, o["state"][:, 0], o["state"][:, 1])
        done_h, _ = lap.update(o["state"][:, 0], o["state"][:, 1], o["collisions"], 0.01)
        done_d = ep["done"] != 0
        tog_d = ep["toggles"].reshape(E, A)
        ok = margin >= 1e-12
        np.testing.assert_array_equal(done_d[ok], done_h[ok], err_msg="done, step %d" % t)
        np.testing.assert_array_equal(tog_d[ok], lap.toggle_list[ok], err_msg="toggles, step %d" % t)
        for e in np.flatnonzero(~ok):   # (too close to call: take the device's bookkeeping)
            lap.toggle_list[e] = tog_d[e]
            lap.near_starts[e] = ep["near_starts"].reshape(E, A)[e] != 0
            skipped += 1
        compared += int(ok.sum())
        s.episode_reset_done_device()
        if done_d.any():
            sp = s.episode_device_views()["start_poses"].download().reshape(E, A, 3)
            lap.reset(sp, done_d)
            draws += int(done_d.sum())
    assert draws >= 20 and compared > 0.99 * E * T
    assert np.max(lap.toggle_list) >= 1
    s.close()


def test_every_state_column_with_the_sampler(amd):
    """save with scans, load and clone with every optional column active (per-agent noise streams, episode, per-agent params,
    env maps, the sampler): the column table's largest configuration"""
    E, A = 16, 2
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.add_map_image(*load_map_image("example_map"))
    s.set_noise_rng(None, STD, per_agent_seeds=list(range(E * A)))
    s.set_track(_track(amd))
    s.set_track(_track(amd), slot=1)
    s.set_env_maps(np.arange(E) % 2)
    s.set_params_batch(np.tile(amd._ffi.params_vector(s.params), (E * A, 1)))
    s.episode_init(0)
    s.episode_reset(bench_start_poses(E, A))
    s.set_reset_sampler(8, lateral=0.2)
    cols = set(amd.core.STATE_COLUMNS)
    blob = s.save_state(scans=True)
    assert set(blob.header["columns"]) == cols
    d_act = s.device_array((E * A, 2))
    acts = _crash_actions(40, E * A, seed=1)
    seq = []
    for t in range(40):
        d_act.upload(acts[t])
        s.episode_step_device(d_act)
        s.episode_reset_done_device()
        seq.append(_obs(s))
    s.load_state(blob)
    for t in range(40):
        d_act.upload(acts[t])
        s.episode_step_device(d_act)
        s.episode_reset_done_device()
        _same(_obs(s), seq[t], "restored step %d" % t)
    s.clone_envs(list(range(0, 8)), list(range(8, 16)))
    a = _obs(s)
    for k in a:
        v = a[k].reshape(E, -1)   # (every column is agent-major: env e's agents are rows e*A .. e*A + A - 1)
        assert np.array_equal(v[:8], v[8:], equal_nan=True), k
    s.sample_reset()
    p = s.reset_sampler_poses().reshape(E, A, 3)
    np.testing.assert_array_equal(p[:8], p[8:])
    s.close()
