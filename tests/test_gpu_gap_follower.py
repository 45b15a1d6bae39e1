"""The follow-the-gap controller on the device (f110_controllers_set, f110_follow_gap_*, F110_STEP_SCRIPTED) against
the NumPy model tests/gap_follower_ref.py, bit for bit on the uint64 view of the actions: the unit form over the grid of the host
tests, the device form through noisy steps with in-step re-seats and mixed assignments, env blocks, the vector envs, shards, no
effect without the flag, the refusals, and the controller driving cars around example_map without a collision."""
import ctypes as C

import numpy as np
import pytest

import gap_follower_ref as ref
from _util import bench_start_poses, load_map_image, map_stem

pytestmark = pytest.mark.gpu

SEED, STD = 4242, 0.01
OTHER = dict(beams=(100, 1000), smooth=9, range_clip=6.0, bubble_radius=0.3, gap_threshold=0.8, target="furthest", steer_gain=0.7, v_hi=6.5,
             d_ref=5.0, steer_slow=0.1)


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _model(g):
    """the model's settings of a GapFollower"""
    return ref.settings(**g.settings())


def _same_bits(got, want, what):
    g, w = ref.bits(got), ref.bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r want %r" % (
            what, len(bad), g.size, bad[0].tolist(), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])]))


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs hit the walls within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


def _sim(amd, E, A=2, B=1080, noise=True, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, **kw)
    s.set_map_image(*load_map_image("example_map"))
    if noise:
        s.set_noise_rng(SEED, STD)
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


def _scans(s):
    o = s.get("scans", "step_count")
    return np.array(o["scans"], copy=True), np.array(o["step_count"], copy=True)


# ---- the unit form over the grid ---------------------------------------------------------------------------------------------
def test_unit_form_matches_model_over_the_grid(amd):
    rng = np.random.default_rng(21)
    sims = {B: amd.BatchSim(num_envs=1, num_agents=1, num_beams=B) for B in ref.GRID_B}   # (no map: a unit entry point)
    orc_rows = {B: ref.oracle_scans(B) for B in ref.GRID_B}
    n = free = 0
    for k, (B, beams, S, target) in enumerate(ref.unit_grid()):
        kw = dict(beams=beams, smooth=S, target=target)
        if k % 3 == 1:
            kw.update(range_clip=6.0, bubble_radius=0.3, gap_threshold=0.8, steer_gain=0.7, v_hi=6.5, d_ref=5.0, steer_slow=0.1)
        g = amd.GapFollower(num_beams=B, **kw)
        rows = np.concatenate([ref.random_rows(rng, 8, B), orc_rows[B][(k % 3)::3]])
        sc = (np.arange(len(rows)) % 5 != 3).astype(np.int32) * (1 + np.arange(len(rows)))
        want = ref.follow(_model(g), rows, sc)
        act, info = sims[B].follow_gap(rows, g, sc, info=True)
        what = "B=%d beams=%r S=%d %s" % (B, beams, S, target)
        assert np.array_equal(info, want[1]), "%s: the integers differ\n%r\n%r" % (what, info, want[1])
        _same_bits(act, want[0], what)
        n += len(rows)
        free += int(np.sum(want[1][:, 4] >= 0))
    assert n >= 300 and free >= n // 3, (n, free)
    s = sims[61]
    for name, st, row, info in ref.hand_rows():
        act, got = s.follow_gap(row[None, :], amd.GapFollower(**st), info=True)
        assert tuple(got[0]) == info, name
        _same_bits(act, ref.follow(st, row[None, :])[0], name)
    # more rows than a workgroup holds waves, without step_count and without info
    rows = ref.random_rows(rng, 133, 1080)
    _same_bits(sims[1080].follow_gap(rows), ref.follow(ref.settings(), rows)[0], "133 rows")
    for b in sims.values():
        b.close()


# ---- the device form through noisy steps with in-step re-seats ---------------------------------------------------------------
@pytest.mark.parametrize("A", [2, 3])
def test_device_form_follows_model_with_mixed_assignments(amd, A):
    E, T = 64, 150
    N = E * A
    s = _sim(amd, E, A)
    d_act = _armed(s, E, A)
    ctrls = [amd.GapFollower(), amd.GapFollower(**OTHER)]
    assign = np.random.default_rng(5).choice([-1, 0, 1], size=N, p=[0.4, 0.3, 0.3]).astype(np.int32)
    assign[:3] = [-1, 0, 1]
    s.set_controllers(assign, ctrls)
    models = [_model(c) for c in ctrls]
    acts = _crash_actions(T, N)
    ext = assign < 0
    fresh = moving = 0
    for t in range(T):
        scans, sc = _scans(s)                        # downloaded before the call
        d_act.upload(acts[t])
        s.follow_gap_device(d_act)
        got = d_act.download()
        want = ref.follow_assigned(models, assign, scans, sc, acts[t])
        _same_bits(got[~ext], want[~ext], "A=%d step %d, scripted rows" % (A, t))
        _same_bits(got[ext], acts[t][ext], "A=%d step %d, external rows" % (A, t))
        z = (sc == 0) & ~ext
        assert np.all(got[z] == 0.0)
        fresh += int(np.sum(z))
        moving += int(np.sum(got[~ext][:, 1] > 0.5))
        s.step_device(d_act)
    assert fresh >= 10, "too few re-seated scripted agents to test the zero action (%d)" % fresh
    assert moving > T * np.sum(~ext) // 2
    s.clear_controllers()
    with pytest.raises(Exception):
        s.follow_gap_device(d_act)
    s.close()


# ---- env blocks ------------------------------------------------------------------------------------------------------------------
def _everything(s):
    o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def test_two_blocks_equal_one_and_stay_two(amd):
    E, A, T = 512, 2, 40
    N = E * A
    assign = np.tile([-1, 0], E).astype(np.int32)
    assign[N // 2:] = np.tile([1, -1], E // 2)
    res = []
    for groups in (1, 2):
        s = _sim(amd, E, A, step_groups=groups)
        d_act = _armed(s, E, A)
        s.set_controllers(assign, [amd.GapFollower(), amd.GapFollower(**OTHER)])
        acts = _crash_actions(T, N)
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            s.follow_gap_device(d_act)
            s.step_device(d_act)                       # a step right behind the controllers keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            s.follow_gap_device(d_act)
        res.append((d_act.download(), _everything(s)))
        s.close()
    _same_bits(res[0][0], res[1][0], "two blocks against one")
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k


# ---- the flag: nothing changes without it, the host step with it ------------------------------------------------------------------
def _host_loop(amd, E, A, T, acts, controllers=None, scripted=False, model=None):
    s = _sim(amd, E, A)
    s.episode_init(0)
    s.episode_reset(bench_start_poses(E, A))
    hb = s.host_block(["state", "scans", "done"])
    if controllers is not None:
        s.set_controllers(*controllers)
    out = []
    for t in range(T):
        a = acts[t]
        if model is not None:                          # the host feeds the model's actions
            a = ref.follow_assigned(model[1], model[0].reshape(-1), *_scans(s), a)
        hb.actions[...] = a
        s.step_host(hb, None, auto_reset=True, scripted=scripted)
        out.append({k: np.array(hb.views[k], copy=True) for k in ("state", "scans", "done")})
    o = _everything(s)
    s.close()
    return out, o


def test_armed_controllers_change_nothing_without_the_flag(amd):
    E, A, T = 64, 2, 100
    acts = _crash_actions(T, E * A)
    assign = np.tile([-1, 0], E).astype(np.int32)
    plain = _host_loop(amd, E, A, T, acts)
    armed = _host_loop(amd, E, A, T, acts, controllers=(assign, [amd.GapFollower()]))
    for t in range(T):
        for k in plain[0][t]:
            assert np.array_equal(plain[0][t][k], armed[0][t][k], equal_nan=True), "step %d: %s differs with controllers armed" % (t, k)
    for k in plain[1]:
        assert np.array_equal(plain[1][k], armed[1][k], equal_nan=True), k


@pytest.mark.parametrize("E", [2, 64])      # (2 envs: a batch that otherwise takes the one-launch form)
def test_scripted_host_step_equals_the_model_fed_by_the_host(amd, E):
    A, T = 2, 100
    acts = _crash_actions(T, E * A, seed=6)
    assign = np.tile([-1, 0], E).astype(np.int32)
    g = amd.GapFollower()
    dev = _host_loop(amd, E, A, T, acts, controllers=(assign, [g]), scripted=True)
    host = _host_loop(amd, E, A, T, acts, model=(assign, [_model(g)]))
    for t in range(T):
        for k in dev[0][t]:
            assert np.array_equal(dev[0][t][k], host[0][t][k], equal_nan=True), "step %d: %s" % (t, k)
    assert sum(int(o["done"].sum()) for o in dev[0]) >= 1


# ---- the vector envs -----------------------------------------------------------------------------------------------------------
def _vec(amd, E, **kw):
    return amd.F110VecEnv(E, auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png", **kw)


def _assert_same_step(a, b, what):
    for k in a[0]:
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), "%s: obs[%r]" % (what, k)
    assert np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and np.array_equal(a[2], b[2]), what
    for k in a[3]:
        assert np.array_equal(a[3][k], b[3][k]), "%s: info[%r]" % (what, k)


def test_vec_env_scripted_equals_host_fed_model(amd):
    E, A, T = 32, 2, 150
    g = amd.GapFollower()
    env, env2, plain = _vec(amd, E, scripted={1: g}), _vec(amd, E, scripted={1: g.settings()}), _vec(amd, E)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    first = env.reset(start)
    env2.reset(start)
    _assert_same_step(first, plain.reset(start), "reset")
    assert sorted(first[0]) == sorted(plain._last[0])
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    assign = np.tile([-1, 0], E).astype(np.int32)
    dones = 0
    for t in range(T):
        fed = ref.follow_assigned([_model(g)], assign, *_scans(plain.sim.batch), acts[t].reshape(-1, 2)).reshape(E, A, 2)
        junk = acts[t].copy()
        junk[:, 1] = 99.0                               # a scripted car's row is ignored
        a, b = env.step(junk), plain.step(fed)
        _assert_same_step(a, b, "step %d" % t)
        env2.step_async(acts[t])
        _assert_same_step(env2.step_wait(), b, "step_async / step_wait, step %d" % t)
        dones += int(np.sum(b[2]))
    assert dones > 5
    assert sorted(env.snapshot()) == sorted(plain.snapshot())      # controllers hold no state: snapshots keep their keys


def test_sharded_equals_one_handle(amd):
    E, A, T = 30, 2, 60
    assign = np.random.default_rng(9).choice([-1, 0, 1], size=(E, A)).astype(np.int32)
    scripted = (assign, [amd.GapFollower(), OTHER])
    kw = dict(auto_reset=True, map=map_stem("example_map"), map_ext=".png", scripted=scripted)
    one = amd.F110VecEnv(E, device_logic=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], shard_sizes=[7, 12, 11], **kw)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    _assert_same_step(sh.reset(start), one.reset(start), "reset")
    acts = _crash_actions(T, E * A, seed=10).reshape(T, E, A, 2)
    for t in range(T):
        _assert_same_step(sh.step(acts[t]), one.step(acts[t]), "step %d" % t)
    sh.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_write_nothing(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    s = _sim(amd, E, A)
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    L = _ffi.lib()
    good = amd.GapFollower()
    d_act = s.device_array((N, 2))
    sentinel = np.random.default_rng(1).normal(size=(N, 2))
    d_act.upload(sentinel)
    assign = np.zeros(N, dtype=np.int32)
    assert L.f110_follow_gap_device(s._h, d_act.ptr) == _ffi.ERR_STATE                      # nothing armed
    hb = s.host_block(["state"])
    assert L.f110_step_host(s._h, hb.actions_ptr, hb.struct_ref, _ffi.STEP_SCRIPTED) == _ffi.ERR_STATE

    def arm(a=assign, n=1, **fields):
        sp = good.spec(1080)
        for k, v in fields.items():
            setattr(sp, k, v)
        arr = (_ffi.GapFollowerSpec * 2)(sp, good.spec(1080))
        return L.f110_controllers_set(s._h, arr, n, _ffi.i32ptr(a))

    inf, nan = float("inf"), float("nan")
    bad = [dict(beam_lo=-1, beam_hi=100), dict(beam_lo=0, beam_hi=1081), dict(beam_lo=500, beam_hi=500), dict(beam_lo=600, beam_hi=200),
           dict(smooth=4), dict(smooth=0), dict(smooth=65), dict(smooth=-1), dict(beam_lo=10, beam_hi=15, smooth=7),
           dict(target=2), dict(target=-1),
           dict(range_clip=0.0), dict(range_clip=-1.0), dict(range_clip=nan), dict(range_clip=inf), dict(d_ref=0.0), dict(d_ref=nan),
           dict(bubble_radius=-0.1), dict(bubble_radius=inf), dict(gap_threshold=-0.5), dict(gap_threshold=nan), dict(steer_gain=inf),
           dict(steer_max=-0.1), dict(steer_max=nan), dict(steer_slow=-1.0), dict(v_lo=5.0, v_hi=4.0), dict(v_lo=nan), dict(v_hi=inf),
           dict(v_turn=nan), dict(v_blocked=inf)]
    for f in bad:
        assert arm(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
        assert L.f110_follow_gap_device(s._h, d_act.ptr) == _ffi.ERR_STATE, f              # a refused spec arms nothing
    for a in (np.full(N, 1, np.int32), np.full(N, -2, np.int32), np.r_[np.zeros(N - 1, np.int32), np.int32(2)].astype(np.int32)):
        assert arm(a) == _ffi.ERR_INVALID
    assert arm(n=0) == _ffi.ERR_INVALID and arm(n=9) == _ffi.ERR_INVALID
    assert L.f110_controllers_set(s._h, None, 1, _ffi.i32ptr(assign)) == _ffi.ERR_INVALID
    s.sync()
    assert np.array_equal(ref.bits(d_act.download()), ref.bits(sentinel)), "a refused call wrote the actions"
    # the unit form refuses the same way and leaves the caller's arrays alone
    sp = good.spec(1080)
    sp.smooth = 2
    scans = _scans(s)[0]
    act = sentinel.copy()
    assert L.f110_follow_gap_batch(s._h, C.byref(sp), _ffi.dptr(scans), None, N, _ffi.dptr(act), None) == _ffi.ERR_INVALID
    assert np.array_equal(ref.bits(act), ref.bits(sentinel))
    with pytest.raises(ValueError):
        s.set_controllers(assign[:-1], [good])
    with pytest.raises(ValueError):
        s.set_controllers(assign, [amd.GapFollower(beams=(0, 2000))])
    # and the good spec goes through; two of two specs, the second unused; misaligned and null buffers are refused
    assert arm(np.where(np.arange(N) % 2, 1, -1).astype(np.int32), n=2) == _ffi.OK
    assert L.f110_follow_gap_device(s._h, None) == _ffi.ERR_INVALID and L.f110_follow_gap_device(s._h, d_act.ptr + 8) == _ffi.ERR_INVALID
    assert L.f110_follow_gap_device(s._h, d_act.ptr) == _ffi.OK
    got = d_act.download()
    assert np.array_equal(ref.bits(got[0::2]), ref.bits(sentinel[0::2])) and not np.array_equal(got[1::2], sentinel[1::2])
    assert L.f110_controllers_set(s._h, None, 0, None) == _ffi.OK
    assert L.f110_follow_gap_device(s._h, d_act.ptr) == _ffi.ERR_STATE
    s.close()


# ---- the controller drives ------------------------------------------------------------------------------------------------------
def drive_on_device(amd, E, A, steps, noise=False, target="center"):
    """every car driven by the default controller on the device; -> (collision flags seen, metres driven per car)"""
    s = _sim(amd, E, A, noise=noise)
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((E * A, 2)))                    # the zero-action step of the reference's reset()
    s.set_controllers(np.zeros(E * A, dtype=np.int32), [amd.GapFollower(target=target)])
    d_act = s.device_array((E * A, 2))
    hits, dist = 0, np.zeros(E * A)
    for t in range(steps):
        s.follow_gap_device(d_act)
        s.step_device(d_act)
        o = s.get("collisions", "in_collision", "state")
        hits += int(np.sum(o["collisions"] != 0)) + int(np.sum(o["in_collision"] != 0))
        dist += np.abs(np.asarray(o["state"]).reshape(-1, 7)[:, 3]) * 0.01
    s.close()
    return hits, dist


def test_controller_drives_single_cars_without_a_collision(amd):
    hits, dist = drive_on_device(amd, 8, 1, 2500)
    assert hits == 0, "%d collision flags" % hits
    assert dist.min() > 40.0, dist


def test_controller_drives_two_scripted_cars_per_env_without_a_collision(amd):
    hits, dist = drive_on_device(amd, 4, 2, 1500)
    assert hits == 0, "%d collision flags" % hits
    assert dist.min() > 20.0, dist
