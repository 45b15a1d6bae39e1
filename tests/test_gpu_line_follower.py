"""The line follower on the device (f110_line_followers_set, f110_follow_line_*, F110_STEP_SCRIPTED) against the NumPy
restatement tests/line_follower_ref.py under the two rules of ref.compare: the speed and the raw columns ld, s_t, k, X, Y, Tx, Ty,
vref, lim and the pre-clamp speed bit for bit; lx, ly and steer, which sit behind cos_sin and atan, rel_err <= 1e-9 where the
model's d2 >= 0.25 (ly's error is a few ulp of |rx| + |ry| <= 2 look_max and d steer / d ly <= 2 wheelbase / d2: about 2e-14
absolute, some 400 times under the gate).

The unit form over the grid of the host tests (five tracks, A up to 256), the device form through noisy steps with in-step re-seats
on two slots next to gap followers, agent counts that fill neither a wave nor a workgroup, env blocks, the scripted host step, the
stream order, no effect on the step, the refusals and the memory, the env layers, and the follower driving berlin's raceline.

Measured on an MI355X (DESIGN §6q has the table): the largest |device - model| over the unit grid, the lap times of the lap test
and the smallest gap of the two-car test are printed by the tests that measure them."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import line_follower_ref as ref
from _util import bench_start_poses, load_map_image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = os.path.join(ROOT, "tests", "golden", "maps")
SEED, STD = 4242, 0.01
INFO = [ref.RAW.index(c) for c in ("ld", "vref", "k", "lim")]


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def race():
    """berlin's raceline with the attributes kappa, vx: the model's tables, the points and the attribute rows"""
    return ref.example_raceline(True, 2)


@pytest.fixture(scope="module")
def ring():
    """a second track for a second slot: a circle of 300 segments around the map"""
    return ref.ring(300, radius=12.0)


def _model(f):
    return ref.settings(**f.settings())


def _same_bits(got, want, what):
    g, w = ref.bits(got), ref.bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r want %r" % (
            what, len(bad), g.size, bad[0].tolist(), np.asarray(got)[tuple(bad[0])], np.asarray(want)[tuple(bad[0])]))


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs hit the walls within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


def _sim(amd, E, A, tracks, env_map=None, noise=True, **kw):
    """example_map on every slot, tracks[m] = (tab, xy, attrs) on slot m, tracking on"""
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    for _ in tracks[1:]:
        s.add_map_image(*load_map_image("example_map"))
    if noise:
        s.set_noise_rng(SEED, STD)
    for m, (tab, xy, attrs) in enumerate(tracks):
        s.set_track(amd.Track(xy, closed=tab.closed, attrs=attrs), m)
    if env_map is not None:
        s.set_env_maps(np.asarray(env_map, dtype=np.int32))
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


def _inputs(s):
    """rows [N][7] = x, y, theta, v, s, lateral, step_count as the follower reads them"""
    o = s.get("agent_poses", "state", "step_count")
    trk = s.get_track()
    return np.column_stack([np.asarray(o["agent_poses"]).reshape(-1, 3), np.asarray(o["state"]).reshape(-1, 7)[:, 3], trk["s"], trk["lateral"],
                            np.asarray(o["step_count"]).astype(np.float64)])


def _model_rows(tabs, env_map, models, assign, rows, A):
    """the model over a whole handle: per slot and spec the envs of that slot, the rows of that spec -> (actions, raw, armed)"""
    N = rows.shape[0]
    act, raw = np.zeros((N, 2)), np.zeros((N, 12))
    slot = np.repeat(np.asarray(env_map), A)
    for m, tab in enumerate(tabs):
        on = slot == m
        if not on.any():
            continue
        for k, S in enumerate(models):
            pick = on & (assign == k)
            if not pick.any():
                continue
            a, r = ref.follow(tab, S, rows[on], A)
            act[pick], raw[pick] = a[pick[on]], r[pick[on]]
    return act, raw, assign >= 0


def _check_device(act, info, want_act, want_raw, armed, rows, what):
    """the two rules on the armed rows of the device form: speed and info bit for bit, steer by rel_err where d2 >= 0.25"""
    _same_bits(act[armed, 1], want_act[armed, 1], what + ", speed")
    if info is not None:
        _same_bits(info[armed], want_raw[armed][:, INFO], what + ", info")
    lx, ly = want_raw[:, 7], want_raw[:, 8]
    far = armed & (rows[:, 6] != 0.0) & (lx * lx + ly * ly >= 0.25)
    e = ref.rel_err(act[far, 0], want_act[far, 0])
    assert np.all(e <= 1e-9), "%s: steer rel_err %r" % (what, float(e.max()))
    fresh = armed & (rows[:, 6] == 0.0)
    assert np.all(act[fresh] == 0.0), what
    return int(far.sum()), int(fresh.sum())


# ---- the unit form over the grid ---------------------------------------------------------------------------------------------------
def test_unit_form_matches_model_over_the_grid(amd):
    rng = np.random.default_rng(2)
    s = amd.BatchSim(num_envs=1, num_agents=1)        # (no map: a unit entry point)
    worst, n, decided = 0.0, 0, 0
    for name, tab, xy, attrs in ref.unit_tracks():
        s.set_track(amd.Track(xy, closed=tab.closed, attrs=attrs))
        for k, A in enumerate(ref.UNIT_A):
            S = ref.unit_settings(name, k)
            rows, first = ref.unit_rows(tab, S, A, rng)
            got = s.follow_line(rows, amd.LineFollower(**S), A=A, raw=True)
            worst = max(worst, ref.compare(tab, S, rows, A, got, "%s A=%d" % (name, A)))
            decided += ref.boundary_check(tab, S, A, rows, first, got[1], "%s A=%d" % (name, A))
            n += rows.shape[0]
            _same_bits(s.follow_line(rows, S, A=A), got[0], "%s A=%d without raw" % (name, A))
    print("unit grid: %d rows, largest |device - model| in lx, ly, steer: %.3g" % (n, worst))
    assert n > 5000 and decided >= 5 * 12     # (per track: ten boundary cars at A = 2, the car at follow_range exactly at A = 3 and 5)
    s.close()


# ---- the device form through noisy steps with in-step re-seats ---------------------------------------------------------------------
def test_device_form_follows_model_next_to_gap_followers(amd, race, ring):
    E, A, T = 24, 3, 120
    N = E * A
    env_map = (np.arange(E) // 2) % 2
    s = _sim(amd, E, A, [race, ring], env_map)
    d_act = _armed(s, E, A)
    d_gap = s.device_array((N, 2))
    d_info = s.device_array((N, 4))
    followers = [amd.LineFollower(), amd.LineFollower(lane_offset=0.3, vgain=1.0, follow_range=3.0, look_gain=0.4, speed_attr=-1)]
    rng = np.random.default_rng(5)
    kind = rng.choice([-1, 0, 1, 2], size=N, p=[0.25, 0.3, 0.3, 0.15])     # 2: a gap follower
    kind[:4] = [-1, 0, 1, 2]
    assign = np.where(kind == 2, -1, kind).astype(np.int32)
    s.set_controllers(np.where(kind == 2, 0, -1).astype(np.int32), [amd.GapFollower()])
    s.set_line_followers(assign, followers)
    models = [_model(f) for f in followers]
    acts = _crash_actions(T, N)
    sentinel = np.full((N, 4), -7.5)
    far = fresh = limited = reseat_steps = 0
    for t in range(T):
        d_act.upload(acts[t])
        rows = _inputs(s)
        take_reseat = bool(np.any(rows[:, 6] == 0.0)) and t > 0 and reseat_steps < 6
        if t % 10 == 3 or t == T - 1 or take_reseat:
            reseat_steps += int(take_reseat)
            d_gap.upload(acts[t])
            s.follow_gap_device(d_gap)
            d_info.upload(sentinel)
            s.follow_gap_device(d_act)
            s.follow_line_device(d_act, d_info)
            got, info, gap = d_act.download(), d_info.download(), d_gap.download()
            want_act, want_raw, armed = _model_rows([race[0], ring[0]], env_map, models, assign, rows, A)
            a, b = _check_device(got, info, want_act, want_raw, armed, rows, "step %d" % t)
            far, fresh = far + a, fresh + b
            limited += int(np.sum(want_raw[armed, 10] >= 0))
            _same_bits(got[~armed], gap[~armed], "step %d: rows without a line follower" % t)
            _same_bits(gap[kind == -1], acts[t][kind == -1], "step %d: the caller's rows" % t)
            _same_bits(info[~armed], sentinel[~armed], "step %d: info rows without a line follower" % t)
        else:
            s.follow_gap_device(d_act)
            s.follow_line_device(d_act)
        s.step_device(d_act)
    assert far > 200 and fresh >= 1 and limited >= 1, (far, fresh, limited)
    s.close()


@pytest.mark.parametrize("N", [1, 63, 65, 257])
def test_agent_counts_that_fill_neither_a_wave_nor_a_workgroup(amd, race, N):
    s = _sim(amd, N, 1, [race], noise=False)
    f = amd.LineFollower()
    assign = np.zeros(N, dtype=np.int32)
    if N > 1:
        assign[N // 2] = -1   # (N = 1: the one agent is armed)
    assign[64:128] = -1          # (257: the second wave of the first workgroup holds no follower and leaves; the other three stage cum)
    s.set_line_followers(assign, [f])
    s.reset(bench_start_poses(N, 1))
    for _ in range(2):
        s.step(np.tile([0.1, 3.0], (N, 1)))
    rows = _inputs(s)
    sentinel = np.random.default_rng(N).normal(size=(N, 2))
    d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4))
    d_act.upload(sentinel)
    d_info.upload(np.full((N, 4), 3.25))
    s.follow_line_device(d_act, d_info)
    got, info = d_act.download(), d_info.download()
    want_act, want_raw, armed = _model_rows([race[0]], np.zeros(N, dtype=int), [_model(f)], assign, rows, 1)
    _check_device(got, info, want_act, want_raw, armed, rows, "N=%d" % N)
    _same_bits(got[~armed], sentinel[~armed], "N=%d: the unarmed row" % N)
    assert np.all(info[~armed] == 3.25)
    s.close()


# ---- launch forms and purity --------------------------------------------------------------------------------------------------------
def _everything(s):
    o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
    out = {k: np.array(v, copy=True) for k, v in o.items()}
    out.update({"track_" + k: np.array(v, copy=True) for k, v in s.get_track().items()})
    return out


def _block_run(amd, race, groups, sync):
    E, A, T = 512, 2, 10
    N = E * A
    s = _sim(amd, E, A, [race], step_groups=groups)
    d_act = _armed(s, E, A)
    d_info = s.device_array((N, 4))
    d_info.upload(np.zeros((N, 4)))
    assign = np.tile([-1, 0], E).astype(np.int32)
    assign[N // 2:] = np.tile([1, -1], E // 2)
    s.set_line_followers(assign, [amd.LineFollower(), amd.LineFollower(follow_range=0.0, vgain=0.6)])
    acts = _crash_actions(T, N)
    wait = s.sync if sync else (lambda: None)
    for t in range(T):
        d_act.upload(acts[t])
        s.step_device(d_act)
        wait()
        s.step_device(d_act)                       # back to back: the second may go out as two blocks
        wait()
        s.follow_line_device(d_act, d_info)        # right behind the blocks, on their streams
        wait()
        s.step_device(d_act)                       # a step right behind the followers keeps its blocks
        if not sync:
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
        wait()
        s.follow_line_device(d_act, d_info)
    res = (d_act.download(), d_info.download(), _everything(s))
    s.close()
    return res


def test_two_blocks_equal_one_in_stream_order(amd, race):
    one, two, two_sync = _block_run(amd, race, 1, False), _block_run(amd, race, 2, False), _block_run(amd, race, 2, True)
    for other, what in ((two, "two blocks against one"), (two_sync, "the synchronised sequence against the enqueued one")):
        _same_bits(one[0], other[0], what + ": actions")
        _same_bits(one[1], other[1], what + ": info")
        for k in one[2]:
            assert np.array_equal(one[2][k], other[2][k], equal_nan=True), "%s: %s" % (what, k)
    assert np.any(one[1][:, 0] > 0.0)


def _host_loop(amd, race, E, A, T, acts, followers=None, mode="plain"):
    """mode 'plain': step_host with the caller's actions; 'scripted': step_host(scripted=True); 'device': follow_line_device on
    the staged actions, downloaded and fed to a plain step_host"""
    s = _sim(amd, E, A, [race])
    s.episode_init(0)
    s.episode_reset(bench_start_poses(E, A))
    hb = s.host_block(["state", "scans", "done"])
    if followers is not None:
        s.set_line_followers(*followers)
    d_act = s.device_array((E * A, 2))
    out = []
    for t in range(T):
        a = acts[t]
        if mode == "device":
            d_act.upload(a)
            s.follow_line_device(d_act)
            a = d_act.download()
        hb.actions[...] = a
        s.step_host(hb, None, auto_reset=True, scripted=(mode == "scripted"))
        out.append({k: np.array(hb.views[k], copy=True) for k in ("state", "scans", "done")})
    o = _everything(s)
    s.close()
    return out, o


@pytest.mark.parametrize("E", [2, 64])      # (2 envs: a batch that otherwise takes the one-launch form)
def test_scripted_host_step_equals_follow_then_step(amd, race, E):
    A, T = 2, 60
    acts = _crash_actions(T, E * A, seed=6)
    followers = (np.tile([-1, 0], E).astype(np.int32), [amd.LineFollower()])
    dev = _host_loop(amd, race, E, A, T, acts, followers, "scripted")
    host = _host_loop(amd, race, E, A, T, acts, followers, "device")
    for t in range(T):
        for k in dev[0][t]:
            assert np.array_equal(dev[0][t][k], host[0][t][k], equal_nan=True), "step %d: %s" % (t, k)
    for k in dev[1]:
        assert np.array_equal(dev[1][k], host[1][k], equal_nan=True), k
    speed = np.abs(dev[1]["state"].reshape(-1, 7)[1::2, 3])
    assert np.max(speed) > 1.0, "no scripted car drives: %r" % speed


def test_armed_followers_change_nothing_without_a_call(amd, race):
    E, A, T = 32, 2, 50
    acts = _crash_actions(T, E * A)
    plain = _host_loop(amd, race, E, A, T, acts)
    armed = _host_loop(amd, race, E, A, T, acts, (np.tile([-1, 0], E).astype(np.int32), [amd.LineFollower()]))
    for t in range(T):
        for k in plain[0][t]:
            assert np.array_equal(plain[0][t][k], armed[0][t][k], equal_nan=True), "step %d: %s differs with line followers armed" % (t, k)
    for k in plain[1]:
        assert np.array_equal(plain[1][k], armed[1][k], equal_nan=True), k


# ---- refusals and memory --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_write_nothing(amd, race):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    tab, xy, attrs = race
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    L = _ffi.lib()
    good = amd.LineFollower()
    d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4))
    sentinel, sent_info = np.random.default_rng(1).normal(size=(N, 2)), np.random.default_rng(2).normal(size=(N, 4))
    d_act.upload(sentinel)
    d_info.upload(sent_info)
    assign = np.zeros(N, dtype=np.int32)

    def call(a=None, i=None):
        return L.f110_follow_line_device(s._h, d_act.ptr if a is None else a, d_info.ptr if i is None else i)

    def arm(a=assign, n=1, **fields):
        sp = good.spec()
        for k, v in fields.items():
            setattr(sp, k, v)
        arr = (_ffi.LineFollowerSpec * 9)(sp, *[good.spec() for _ in range(8)])
        return L.f110_line_followers_set(s._h, arr, n, _ffi.i32ptr(a))

    assert call() == _ffi.ERR_STATE                                                   # nothing armed
    hb = s.host_block(["state"])
    assert L.f110_step_host(s._h, hb.actions_ptr, hb.struct_ref, _ffi.STEP_SCRIPTED) == _ffi.ERR_STATE
    base = _ffi.device_allocs()
    inf, nan = float("inf"), float("nan")
    bad = [{k: v} for k in _ffi.LINE_FLOATS for v in (nan, inf)]
    bad += [dict(look_min=0.0), dict(look_min=-0.5), dict(look_min=4.0), dict(look_base=-0.1), dict(look_gain=-0.1), dict(speed_look=-0.1),
            dict(wheelbase=0.0), dict(wheelbase=-1.0), dict(steer_max=-0.1), dict(v_min=-0.1), dict(v_min=21.0), dict(follow_range=-0.1),
            dict(lane_width=-0.1), dict(lat_slow=-0.1), dict(speed_attr=-2), dict(speed_attr=4)]
    for f in bad:
        assert arm(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
        assert call() == _ffi.ERR_STATE, f                                            # a refused spec arms nothing
    for a in (np.full(N, 1, np.int32), np.full(N, -2, np.int32), np.r_[np.zeros(N - 1, np.int32), np.int32(2)].astype(np.int32)):
        assert arm(a) == _ffi.ERR_INVALID
    assert arm(n=0) == _ffi.ERR_INVALID and arm(n=9) == _ffi.ERR_INVALID
    assert L.f110_line_followers_set(s._h, None, 1, _ffi.i32ptr(assign)) == _ffi.ERR_INVALID
    assert _ffi.device_allocs() == base
    with pytest.raises(ValueError):
        s.set_line_followers(assign[:-1], [good])
    with pytest.raises(ValueError):
        s.set_line_followers(assign, [good] * 9)
    # armed, but the handle cannot run them: tracking off, no track, no attribute column, a track too short
    assert arm() == _ffi.OK
    assert _ffi.device_allocs()[0] == base[0] + 2                                     # the specs and the assignment
    assert call() == _ffi.ERR_STATE and "tracking is off" in _ffi.last_error(s._h)
    assert L.f110_step_host(s._h, hb.actions_ptr, hb.struct_ref, _ffi.STEP_SCRIPTED) == _ffi.ERR_STATE
    s.set_track(amd.Track(xy))                                                        # a track without attributes
    s.enable_track()
    s.step(np.zeros((N, 2)))
    assert call() == _ffi.ERR_STATE and "speed_attr" in _ffi.last_error(s._h)
    s.set_track_attrs(0, tab.attrs[:, :1])                                              # kappa only: column 1 is missing
    assert call() == _ffi.ERR_STATE and "speed_attr" in _ffi.last_error(s._h)
    s.set_track_attrs(0, tab.attrs)
    assert call(a=0) == _ffi.ERR_INVALID and call(a=d_act.ptr + 8) == _ffi.ERR_INVALID and call(i=d_info.ptr + 8) == _ffi.ERR_INVALID
    short, sxy, sattrs = ref.closed_8()                                               # about 25 m: longer than look_max, not than 2 * follow_range = 30
    s.set_track(amd.Track(sxy, attrs=sattrs))
    s.step(np.zeros((N, 2)))
    armed_allocs = _ffi.device_allocs()
    assert arm(follow_range=15.0) == _ffi.OK
    assert call() == _ffi.ERR_STATE and "twice follow_range" in _ffi.last_error(s._h)
    assert arm(look_max=30.0) == _ffi.OK
    assert call() == _ffi.ERR_STATE and "reach" in _ffi.last_error(s._h)
    assert arm(speed_look=30.0) == _ffi.OK
    assert call() == _ffi.ERR_STATE and "reach" in _ffi.last_error(s._h)
    assert L.f110_step_host(s._h, hb.actions_ptr, hb.struct_ref, _ffi.STEP_SCRIPTED) == _ffi.ERR_STATE
    s.sync()
    _same_bits(d_act.download(), sentinel, "a refused call wrote the actions")
    _same_bits(d_info.download(), sent_info, "a refused call wrote the info")
    assert _ffi.device_allocs() == armed_allocs
    # the unit form refuses the same way and leaves the caller's arrays alone
    rows = np.tile([0.0, 0.0, 0.0, 1.0, 1.0, 0.0, 1.0], (N, 1))
    act = sentinel.copy()
    sp = good.spec()
    sp.look_min = 0.0
    assert L.f110_follow_line_batch(s._h, C.byref(sp), 0, 1, _ffi.dptr(rows), N, _ffi.dptr(act), None) == _ffi.ERR_INVALID
    sp = good.spec()
    for slot, A_, m in ((1, 1, N), (0, 0, N), (0, 257, N), (0, 3, N)):
        assert L.f110_follow_line_batch(s._h, C.byref(sp), slot, A_, _ffi.dptr(rows), m, _ffi.dptr(act), None) != _ffi.OK, (slot, A_, m)
    sp.speed_attr = 2
    assert L.f110_follow_line_batch(s._h, C.byref(sp), 0, 1, _ffi.dptr(rows), N, _ffi.dptr(act), None) == _ffi.ERR_STATE
    _same_bits(act, sentinel, "a refused unit call wrote the actions")
    # the good spec goes through; disarming returns the allocations
    s.set_track(amd.Track(xy, attrs=attrs))
    s.step(np.zeros((N, 2)))
    assert arm(np.where(np.arange(N) % 2, 1, -1).astype(np.int32), n=2) == _ffi.OK
    assert call() == _ffi.OK
    got = d_act.download()
    _same_bits(got[0::2], sentinel[0::2], "the unarmed rows")
    assert not np.array_equal(got[1::2], sentinel[1::2])
    live = _ffi.device_allocs()[0]
    assert L.f110_line_followers_set(s._h, None, 0, None) == _ffi.OK
    assert _ffi.device_allocs()[0] == live - 2
    assert call() == _ffi.ERR_STATE
    s.close()


def test_arming_and_disarming_returns_the_allocations(amd, race):
    from f1tenth_gym_amd import _ffi
    s = _sim(amd, 4, 2, [race], noise=False)
    s.reset(bench_start_poses(4, 2))
    s.step(np.zeros((8, 2)))
    d_act = s.device_array((8, 2))
    before = _ffi.device_allocs()
    for _ in range(3):
        s.set_line_followers(np.tile([0, -1], 4), [amd.LineFollower()])
        s.follow_line_device(d_act)
        s.set_line_followers(np.tile([-1, 1], 4), [amd.LineFollower(), amd.LineFollower(vgain=0.5)])   # re-arming reuses the buffers
        assert _ffi.device_allocs()[0] == before[0] + 2
        s.clear_line_followers()
        assert _ffi.device_allocs() == before
    s.close()


@pytest.mark.parametrize("A,car", [(100, 64), (200, 128)])
def test_one_armed_car_in_an_env_of_several_waves(amd, race, A, car):
    """more than 64 lanes per env (128 and 256) and one follower per env: the env's waves without an armed agent stay, because the
    armed car walks their (s, lat, v) columns; the workgroup's other env (A = 100) has none and its waves leave"""
    E = 3
    N = E * A
    s = _sim(amd, E, A, [race], noise=False)
    f = amd.LineFollower()
    assign = np.full((E, A), -1, dtype=np.int32)
    assign[0, car] = assign[2, car] = 0
    assign = assign.reshape(-1)
    s.set_line_followers(assign, [f])
    s.reset(bench_start_poses(E, A, gap_wp=1000 // A))
    for _ in range(3):
        s.step(np.tile([0.0, 1.0], (N, 1)))
    rows = _inputs(s)
    sentinel = np.random.default_rng(A).normal(size=(N, 2))
    d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4))
    d_act.upload(sentinel)
    d_info.upload(np.full((N, 4), 3.25))
    s.follow_line_device(d_act, d_info)
    got, info = d_act.download(), d_info.download()
    want_act, want_raw, armed = _model_rows([race[0]], np.zeros(E, dtype=int), [_model(f)], assign, rows, A)
    _check_device(got, info, want_act, want_raw, armed, rows, "A=%d" % A)
    lim = want_raw[armed, 10].astype(int)
    assert armed.sum() == 2 and np.all(lim >= 0) and np.all(lim >> 6 != car >> 6), "a car of another wave is to limit the armed one: %r" % lim
    _same_bits(got[~armed], sentinel[~armed], "A=%d: the unarmed rows" % A)
    assert np.all(info[~armed] == 3.25)
    s.close()


def test_more_cars_per_env_than_the_car_ahead_term_serves(amd):
    """num_agents = 257: arming with follow_range > 0 is refused (F110_ERR_STATE) with the allocations and the buffers as they
    were; with follow_range = 0 it goes through"""
    from f1tenth_gym_amd import _ffi
    A = 257
    s = amd.BatchSim(num_envs=1, num_agents=A)
    L = _ffi.lib()
    d_act, d_info = s.device_array((A, 2)), s.device_array((A, 4))
    sentinel, sent_info = np.random.default_rng(3).normal(size=(A, 2)), np.random.default_rng(4).normal(size=(A, 4))
    d_act.upload(sentinel)
    d_info.upload(sent_info)
    assign = np.zeros(A, dtype=np.int32)
    before = _ffi.device_allocs()
    sp = (_ffi.LineFollowerSpec * 1)(amd.LineFollower().spec())
    assert L.f110_line_followers_set(s._h, sp, 1, _ffi.i32ptr(assign)) == _ffi.ERR_STATE and "257 agents per env" in _ffi.last_error(s._h)
    assert _ffi.device_allocs() == before
    assert L.f110_follow_line_device(s._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE          # nothing was armed
    with pytest.raises(Exception, match="257 agents per env"):
        s.set_line_followers(assign, [amd.LineFollower(), amd.LineFollower(follow_range=0.0)])   # one spec with the term is enough
    s.sync()
    _same_bits(d_act.download(), sentinel, "a refused arming wrote the actions")
    _same_bits(d_info.download(), sent_info, "a refused arming wrote the info")
    assert _ffi.device_allocs() == before
    s.set_line_followers(assign, [amd.LineFollower(follow_range=0.0)])
    assert _ffi.device_allocs()[0] == before[0] + 2
    s.clear_line_followers()
    assert _ffi.device_allocs() == before
    s.close()
    with pytest.raises(ValueError, match="at most 256 cars per env"):
        amd.F110VecEnv(1, device_logic=True, num_agents=A, scripted={0: amd.LineFollower()}, track='raceline',
                       map=os.path.join(MAPS, "berlin"), map_ext=".png")


def test_an_armed_agents_slot_without_a_track_is_refused(amd, race):
    """device form: envs moved to a slot that has no track behind the arming; only the slots of armed agents count"""
    from f1tenth_gym_amd import _ffi
    E, A = 4, 2
    N = E * A
    s = _sim(amd, E, A, [race], noise=False)
    s.add_map_image(*load_map_image("example_map"))        # slot 1: a map, no track
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4))
    sentinel, sent_info = np.random.default_rng(5).normal(size=(N, 2)), np.random.default_rng(6).normal(size=(N, 4))
    d_act.upload(sentinel)
    d_info.upload(sent_info)
    assign = np.full(N, -1, dtype=np.int32)
    assign[:A] = 0                                          # env 0's cars only
    s.set_line_followers(assign, [amd.LineFollower()])
    s.follow_line_device(d_act, d_info)
    d_act.upload(sentinel)
    d_info.upload(sent_info)
    s.set_env_maps(np.array([1, 0, 0, 0], dtype=np.int32))  # the armed env on the slot without a track
    before = _ffi.device_allocs()
    L = _ffi.lib()
    assert L.f110_follow_line_device(s._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE and "map slot 1 has no track" in _ffi.last_error(s._h)
    hb = s.host_block(["state"])
    assert L.f110_step_host(s._h, hb.actions_ptr, hb.struct_ref, _ffi.STEP_SCRIPTED) == _ffi.ERR_STATE
    s.sync()
    _same_bits(d_act.download(), sentinel, "a refused call wrote the actions")
    _same_bits(d_info.download(), sent_info, "a refused call wrote the info")
    s.set_env_maps(np.array([0, 1, 1, 1], dtype=np.int32))  # unarmed envs there: no objection from the followers
    assert L.f110_follow_line_device(s._h, d_act.ptr, d_info.ptr) == _ffi.OK
    got = d_act.download()
    _same_bits(got[A:], sentinel[A:], "the unarmed rows")
    assert not np.array_equal(got[:A], sentinel[:A])
    s.close()


def test_three_way_exclusivity_in_both_orders(amd, race):
    E, A = 4, 3
    N = E * A
    s = _sim(amd, E, A, [race], noise=False)
    line, gap, plan = np.tile([0, -1, -1], E), np.tile([-1, 0, -1], E), np.arange(E) * A + 2
    lf, gf, mp = amd.LineFollower(), amd.GapFollower(), amd.Mppi(k=64, horizon=8)
    # side by side on different cars
    s.set_line_followers(line, [lf])
    s.set_controllers(gap, [gf])
    s.set_mppi(mp, plan, seed=1)
    # the other calls refuse a line follower's car and name the call
    with pytest.raises(Exception, match="f110_line_followers_set"):
        s.set_controllers(np.tile([0, 0, -1], E), [gf])
    with pytest.raises(Exception, match="f110_line_followers_set"):
        s.set_mppi(mp, np.arange(E) * A, seed=1)
    # and the line followers refuse theirs
    with pytest.raises(Exception, match="f110_controllers_set"):
        s.set_line_followers(np.tile([0, 0, -1], E), [lf])
    with pytest.raises(Exception, match="f110_mppi_set"):
        s.set_line_followers(np.tile([0, -1, 0], E), [lf])
    assert np.array_equal(s.line_follower_assign, line)
    # the other order: disarmed, the cars are free again
    s.clear_line_followers()
    s.set_controllers(np.tile([0, 0, -1], E), [gf])
    with pytest.raises(Exception, match="f110_controllers_set"):
        s.set_line_followers(line, [lf])
    s.clear_controllers()
    s.set_line_followers(np.tile([0, 0, -1], E), [lf])
    s.close()


# ---- the env layers -------------------------------------------------------------------------------------------------------------------
def _kw(name="berlin", agents=1):
    return dict(map=os.path.join(MAPS, name), map_ext=".png", num_agents=agents)


def _assert_same_step(a, b, what):
    for k in a[0]:
        assert np.array_equal(np.asarray(a[0][k]), np.asarray(b[0][k]), equal_nan=True), "%s: obs[%r]" % (what, k)
    assert np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and np.array_equal(a[2], b[2]), what


def _line_poses(track, s0, lat=0.0):
    xy, tan = track.point_at(np.asarray(s0, dtype=np.float64))
    return np.column_stack([xy[:, 0] - lat * tan[:, 1], xy[:, 1] + lat * tan[:, 0], np.arctan2(tan[:, 1], tan[:, 0])])


RS = dict(iters=100, margin=0.45)     # the raceline examples/raceline.py drives on berlin


def test_vec_env_scripted_equals_hand_armed_handle(amd):
    E, A, T = 4, 2, 80
    f = amd.LineFollower()
    kw = dict(device_logic=True, auto_reset=True, track='raceline', raceline=RS, **_kw(agents=A))
    env, plain = amd.F110VecEnv(E, scripted={1: f}, **kw), amd.F110VecEnv(E, **kw)
    assert env.line_followers is not None and env.scripted is None
    rl = env.tracks[0]
    s0 = np.arange(E) * rl.length / E + 1.0
    start = np.stack([_line_poses(rl, s0 + 3.0), _line_poses(rl, s0)], axis=1)
    _assert_same_step(env.reset(start), plain.reset(start), "reset")
    b = plain.sim.batch
    b.set_line_followers(np.tile([-1, 0], E), [f])
    d_act = b.device_array((E * A, 2))
    acts = np.tile([0.0, 1.5], (T, E, A, 1))
    for t in range(T):
        d_act.upload(acts[t].reshape(-1, 2))
        b.follow_line_device(d_act)
        fed = d_act.download().reshape(E, A, 2)
        junk = acts[t].copy()
        junk[:, 1] = 99.0                               # a scripted car's row is ignored
        _assert_same_step(env.step(junk), plain.step(fed), "step %d" % t)
    assert np.all(np.asarray(env._last[0]["linear_vels_x"]).reshape(E, A)[:, 1] > 1.0)
    env.sim.batch.close()
    plain.sim.batch.close()
    with pytest.raises(ValueError, match="needs a track"):
        amd.F110VecEnv(E, device_logic=True, scripted={1: f}, **_kw(agents=A))


def test_sharded_equals_one_handle(amd):
    E, A, T = 6, 2, 40
    scripted = ([[0, 1]] * 3 + [[1, -1]] * 3, [amd.LineFollower(), amd.GapFollower()])
    kw = dict(auto_reset=True, track='raceline', raceline=RS, scripted=scripted, **_kw(agents=A))
    one = amd.F110VecEnv(E, device_logic=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=[0, 0], **kw)
    rl = one.tracks[0]
    s0 = np.arange(E) * rl.length / E + 1.0
    start = np.stack([_line_poses(rl, s0 + 3.0), _line_poses(rl, s0)], axis=1)
    _assert_same_step(sh.reset(start), one.reset(start), "reset")
    acts = np.tile([0.05, 2.0], (E, A, 1))
    for t in range(T):
        _assert_same_step(sh.step(acts), one.step(acts), "step %d" % t)
    sh.close()
    one.sim.batch.close()


def test_set_track_map_hands_the_follower_the_new_line(amd):
    from f1tenth_gym_amd import random_track, TrackMap
    frame = dict(origin=(-15.0, -15.0, 0.0), shape=(480, 480))
    tms = [TrackMap(random_track(seed), **frame) for seed in (1, 2)]
    f = amd.LineFollower()
    env = amd.F110VecEnv(2, device_logic=True, track_maps=tms[:1], tracks={1: 'raceline'}, env_map=[1, 1], scripted={0: f},
                         map=os.path.join(MAPS, "example_map"), map_ext=".png", num_agents=1)
    b = env.sim.batch

    def drive(steps):
        rl = env.tracks[1]
        env.reset(_line_poses(rl, [1.0, 0.5 * rl.length]).reshape(2, 1, 3))
        for _ in range(steps):
            obs = env.step(np.zeros((2, 1, 2)))[0]
        tab = ref.Tables(rl.xy, True, rl.attrs)
        rows = _inputs(b)
        d_act = b.device_array((2, 2))
        b.follow_line_device(d_act)
        want_act, want_raw, armed = _model_rows([None, tab], [1, 1], [_model(f)], np.zeros(2, dtype=np.int32), rows, 1)
        _check_device(d_act.download(), None, want_act, want_raw, armed, rows, "on %r" % rl)
        assert not np.asarray(obs["collisions"]).any() and np.all(np.asarray(obs["linear_vels_x"]) > 0.5)
        assert np.all(np.abs(np.asarray(obs["lateral_offset"])) < 0.3)
        return rl

    first = drive(60)
    env.set_track_map(1, tms[1])
    second = drive(60)                                    # the follower drives the new line from the next step on
    assert second.num_points != first.num_points or not np.array_equal(second.xy, first.xy)
    b.close()


# ---- the follower drives ----------------------------------------------------------------------------------------------------------------
def test_every_car_completes_a_lap_of_berlin_at_the_defaults(amd):
    E = 4
    f = amd.LineFollower()
    env = amd.F110VecEnv(E, device_logic=True, track='raceline', raceline=RS, scripted={0: f}, reward='progress', **_kw())
    rl = env.tracks[0]
    cap = int(np.ceil(2.0 * rl.lap_time / f.vgain / env.timestep))     # a liveness cap, not a performance claim
    env.reset(_line_poses(rl, np.arange(E) * rl.length / E + 1.0).reshape(E, 1, 3))
    travelled, lap_step, hit = np.zeros(E), np.full(E, -1), False
    acts = np.zeros((E, 1, 2))
    for t in range(cap):
        obs, reward, _, _ = env.step(acts)
        travelled += np.asarray(reward).reshape(E)
        lap_step = np.where((lap_step < 0) & (travelled >= rl.length), t + 1, lap_step)
        hit = bool(np.asarray(obs["collisions"]).any())
        if hit or np.all(lap_step >= 0):
            break
    print("berlin, %r: lap times %s s (the profile's %.2f s / vgain = %.2f s), cap %d steps, hit %r" % (
        f, (lap_step * env.timestep).round(2).tolist(), rl.lap_time, rl.lap_time / f.vgain, cap, hit))
    env.sim.batch.close()
    assert not hit, "a collision after %d steps, %r m of %.1f m travelled" % (t + 1, travelled.round(1).tolist(), rl.length)
    assert np.all(lap_step >= 0), "no lap within %d steps: %r m of %.1f m travelled" % (cap, travelled.round(1).tolist(), rl.length)


def test_a_faster_follower_stays_behind_a_slower_one(amd):
    rear, front = amd.LineFollower(vgain=0.9), amd.LineFollower(vgain=0.5)
    env = amd.F110VecEnv(2, device_logic=True, track='raceline', raceline=RS, scripted={0: rear, 1: front}, reward='progress', **_kw(agents=2))
    rl = env.tracks[0]
    s0 = np.array([1.0, 0.5 * rl.length])
    env.reset(np.stack([_line_poses(rl, s0), _line_poses(rl, s0 + 4.0)], axis=1))
    steps = int(np.ceil(rl.lap_time / front.vgain / env.timestep)) + 200
    gap_min, hit, travelled = np.inf, False, np.zeros(2)
    acts = np.zeros((2, 2, 2))
    for t in range(steps):
        obs, reward, _, _ = env.step(acts)
        s = np.asarray(obs["progress"]).reshape(2, 2)
        g = np.array([ref.gap(s[e, 0], s[e, 1], rl.length) for e in range(2)])
        if t > 0:
            gap_min = min(gap_min, float(g.min()))
        travelled += np.asarray(reward).reshape(2)
        hit = hit or bool(np.asarray(obs["collisions"]).any())
        if hit or np.all(travelled >= rl.length):
            break
    print("two followers on berlin's raceline (vgain 0.9 behind 0.5, 4 m apart at the start): smallest gap %.3f m over %d steps, hit %r" % (gap_min, t + 1, hit))
    env.sim.batch.close()
    assert not hit, "a collision after %d steps" % (t + 1)
    assert gap_min > 0.0 and np.all(travelled >= rl.length), (gap_min, travelled)


def test_example_runs_in_a_fresh_process():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "line_followers.py"), "--envs", "2"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=120)
    assert proc.returncode == 0 and "smallest gap" in proc.stdout, proc.stdout[-3000:]
