"""The rollout on the device (f110_rollout_*).

(a) the unit form against the Python model tests/rollout_ref.py over the grid of the host tests and on 45 envs x 2 cars x K = 3 (270
    lanes: agents straddle waves and a workgroup): raw float64 values under the project's parity gate rel_err < 1e-5,
    every float32 output exactly (float)(raw / scale) of the device's own raw value, ALIVE exact except for candidates whose model
    clearance comes within 1e-9 m of the margin at a visited step (left out, at most 1 %; the model alone is held to that too).
    Measured on an MI355X: 26 304 + 540 candidates, none left out, the largest rel_err 0.0 beyond rel_err's 1e-12 absolute floor.
(b) the rollout is the simulator: 16 x 2 cars on example_map, 15 warm-up steps, the 8 x 8 candidates of default_rng(7) held 3 steps;
    the handle, restored from the state blob and stepped 24 times with a candidate, passes through the rollout's trajectory rows
    exactly and raises no collision flag.
(c) two env blocks against one with the pinned copy, two map slots with different tracks and per-agent parameter rows, no effect on
    the step, the refusals, a torch consumer through DLPack, the example planner."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import rollout_ref as ref
from _util import MAPS, bench_start_poses, load_map_image, rel_err

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(MAPS, "example_waypoints.csv")
ALL10 = ref.CHANNELS


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _two_maps(amd, E=1, A=1, **kw):
    """slot 0: example_map with its raceline; slot 1: berlin with the grid's open polyline"""
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    assert s.add_map_image(*load_map_image("berlin")) == 1
    s.set_track(ref.grid_track("example_map"), 0)
    s.set_track(ref.grid_track("berlin"), 1)
    return s


def _check_unit(s, flown, want, got, what, stats):
    """got = (out, traj, raw, traj_raw) of rollout_rows against the model's (out, raw, traj, traj_raw)"""
    out, traj, raw, traw = got
    w_raw, w_traw = want[1], want[3]
    keep = flown[4] >= 1e-9                     # the model's clearance stays 1e-9 m away from the margin at every visited step
    stats["left_out"] += int(np.count_nonzero(~keep))
    stats["candidates"] += keep.size
    assert np.array_equal(raw[..., ref.ALIVE][keep], w_raw[..., ref.ALIVE][keep]), "%s: ALIVE differs" % (what,)
    err = max(rel_err(raw[keep], w_raw[keep]), rel_err(traw[keep], w_traw[keep]))
    stats["rel_err"] = max(stats["rel_err"], err)
    assert err < 1e-5, "%s: rel_err %.3e" % (what, err)
    scale = np.array([float(s["scale"].get(c, 1.0)) for c in ref.CHANNELS])
    bits = [b for b, c in enumerate(ref.CHANNELS) if c in s["channels"]]
    with np.errstate(over="ignore", invalid="ignore"):
        own = (raw[..., bits] / scale[bits]).astype(np.float32)
        own_traj = (traw / scale[:4]).astype(np.float32)
    assert np.array_equal(ref.bits(out), ref.bits(own)), "%s: a float32 output is not (float)(raw / scale)" % (what,)
    assert np.array_equal(ref.bits(traj), ref.bits(own_traj)), "%s: a float32 trajectory value is not (float)(raw / scale)" % (what,)


# ---- (a) the unit form against the model -----------------------------------------------------------------------------------------------
def test_unit_form_matches_model_over_the_grid(amd):
    sims = {integ: _two_maps(amd, integrator=integ) for integ in (1, 2)}
    stats = {"left_out": 0, "candidates": 0, "rel_err": 0.0}
    for case in ref.grid_cases():
        map_name, K, H, repeat, integrator, per_agent = case
        start, params = ref.grid_rows(map_name)
        flown, track = ref.grid_flown(case), ref.grid_track(map_name)
        for frame in ("map", "ego"):
            s = ref.grid_settings(case, frame)
            got = sims[integrator].rollout_rows(amd.Rollout(**s), start, ref.grid_actions(K, H, per_agent), slot=ref.GRID_MAPS.index(map_name),
                                                params=params, raw=True)
            _check_unit(s, flown, ref.render(s, start, flown, track), got, (case, frame), stats)
    print("rollout unit grid: %(candidates)d candidates, %(left_out)d left out, largest rel_err %(rel_err).3e" % stats)
    assert stats["left_out"] * 100 <= stats["candidates"], stats
    for s in sims.values():
        s.close()


def test_unit_form_270_lanes_across_waves_and_a_workgroup(amd):
    E, A, K, H, repeat = 45, 2, 3, 5, 3
    poses = bench_start_poses(E, A)
    m = E * A
    rng = np.random.default_rng(45)
    start = np.zeros((m, 10))
    start[:, [0, 1, 4]] = poses
    start[:, 3] = rng.uniform(0.0, 5.0, m)
    start[:, 7:9] = rng.uniform(-0.2, 0.2, (m, 2))
    start[:, 9] = rng.integers(0, 3, m)
    params = np.tile(ref.orc.params_vec(), (m, 1))
    actions = np.stack([rng.uniform(-0.4, 0.4, (m, K, H)), rng.uniform(0.0, 7.0, (m, K, H))], axis=-1)
    so, track = ref.scan_oracle("example_map"), ref.grid_track("example_map")
    flown = ref.fly(so, start, params, actions, True, repeat, ref.GRID_MARGIN, 1)
    sim = _two_maps(amd)
    stats = {"left_out": 0, "candidates": 0, "rel_err": 0.0}
    for frame in ("map", "ego"):
        s = ref.settings(k=K, horizon=H, repeat=repeat, margin=ref.GRID_MARGIN, frame=frame, layout="per_agent", scale={"end_x": 3.0, "progress": 5.0})
        got = sim.rollout_rows(amd.Rollout(**s), start, actions, params=params, raw=True)
        _check_unit(s, flown, ref.render(s, start, flown, track), got, ("270 lanes", frame), stats)
    # the handle's own parameter row of agent slot 0 when none is given, and without raw values or a trajectory
    s = ref.settings(k=K, horizon=H, repeat=repeat, margin=ref.GRID_MARGIN, layout="per_agent", traj=False, channels=("end_x", "alive", "progress"))
    out = sim.rollout_rows(amd.Rollout(**s), start, actions)
    want = ref.render(s, start, flown, track)[0]
    assert out.shape == (m, K, 3) and rel_err(out, want, atol=1e-6) < 1e-5
    print("rollout 270 lanes: %(candidates)d candidates, %(left_out)d left out, largest rel_err %(rel_err).3e" % stats)
    assert stats["left_out"] * 100 <= stats["candidates"], stats
    sim.close()


def test_walls_unit_form(amd):
    """candidates that die: ALIVE and the frozen poses as the model has them"""
    start, params, actions, flown = ref.wall_case()
    sim = _two_maps(amd)
    stats = {"left_out": 0, "candidates": 0, "rel_err": 0.0}
    s = ref.settings(k=2, horizon=60, repeat=1, margin=ref.GRID_MARGIN, frame="ego", scale={"alive": 60.0})
    got = sim.rollout_rows(amd.Rollout(**s), start, actions, params=params, raw=True)
    _check_unit(s, flown, ref.render(s, start, flown, ref.grid_track("example_map")), got, "walls", stats)
    assert stats["left_out"] == 0 and np.count_nonzero(got[2][..., ref.ALIVE] < 60) * 4 >= flown[1].size
    sim.close()


# ---- (b) the rollout is the simulator ---------------------------------------------------------------------------------------------------
def test_rollout_is_the_simulator(amd):
    E, A, K, H, repeat = 16, 2, 8, 8, 3
    N = E * A
    rng = np.random.default_rng(7)
    steer = rng.uniform(-0.3, 0.3, (K, H))
    speed = rng.uniform(1.0, 5.0, (K, H))
    cand = np.stack([steer, speed], axis=-1)
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map_image(*load_map_image("example_map"))
    sim.reset(bench_start_poses(E, A))
    for _ in range(15):
        sim.step(np.tile([0.05, 3.0], (N, 1)))
    blob = sim.save_state()
    p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=("end_v", "end_yaw_rate", "alive", "min_clear"), margin=0.3, frame="map", traj=True)
    out, traj = sim.rollout(p, cand)
    f32 = lambda a: np.asarray(a, dtype=np.float64).astype(np.float32)   # noqa: E731
    assert np.all(out[..., 2] == 24.0), "a candidate left the track: ALIVE %r" % (out[..., 2].min(),)
    assert out[..., 3].min() > 0.3
    for k in range(K):
        sim.load_state(blob)
        for t in range(H * repeat):
            sim.step(np.tile(cand[k, t // repeat], (N, 1)))
            o = sim.get("state", "collisions", "in_collision")
            assert not o["collisions"].any() and not o["in_collision"].any(), "candidate %d: a collision flag at step %d" % (k, t)
            if t % repeat == repeat - 1:
                st = o["state"]
                want = np.stack([f32(st[:, 0]), f32(st[:, 1]), f32(np.cos(st[:, 4])), f32(np.sin(st[:, 4]))], axis=-1)
                assert np.array_equal(ref.bits(traj[:, k, t // repeat]), ref.bits(want)), "candidate %d, step %d" % (k, t)
        assert np.array_equal(ref.bits(out[:, k, 0]), ref.bits(f32(st[:, 3]))) and np.array_equal(ref.bits(out[:, k, 1]), ref.bits(f32(st[:, 5]))), k
    sim.close()


# ---- (c) env blocks ---------------------------------------------------------------------------------------------------------------------
def test_two_blocks_equal_one(amd):
    E, A, T = 512, 2, 6
    N = E * A
    p = amd.Rollout(k=8, horizon=4, repeat=2, channels=ALL10, margin=0.3, frame="ego", traj=True, layout="per_agent")
    rng = np.random.default_rng(11)
    cand = np.stack([rng.uniform(-0.4, 0.4, p.actions_shape(N)[:-1]), rng.uniform(1.0, 7.0, p.actions_shape(N)[:-1])], axis=-1)
    res = []
    for groups in (1, 2):
        s = amd.BatchSim(num_envs=E, num_agents=A, step_groups=groups)
        s.set_map_image(*load_map_image("example_map"))
        s.set_noise_rng(4242, 0.01)
        s.set_track(CSV)
        s.reset(bench_start_poses(E, A))
        d_act = s.device_array((N, 2))
        d_act.upload(np.tile([0.05, 3.0], (N, 1)))
        d_cand = s.device_array(cand.shape)
        d_cand.upload(cand)
        buf, tr = s.device_array(p.shape(N), np.float32), s.device_array(p.traj_shape(N), np.float32)
        pin = s.pinned_empty(p.shape(N), np.float32)
        for t in range(T):
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            s.rollout_device(p, d_cand, buf, tr, pinned=pin)
            s.step_device(d_act)                       # a step right behind the call keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            s.rollout_device(p, d_cand, buf, tr, pinned=pin)
        s.sync()
        out = buf.download()
        assert np.array_equal(ref.bits(np.array(pin)), ref.bits(out)), "the pinned copy differs from the download"
        assert np.all(out[..., ref.ALIVE] <= 8.0) and np.all(out[..., ref.MIN_CLEAR] > 0.0) and np.all(np.abs(out[..., ref.PROGRESS]) < 1.0)
        res.append((out, tr.download()))
        s.close()
    assert np.array_equal(ref.bits(res[0][0]), ref.bits(res[1][0])) and np.array_equal(ref.bits(res[0][1]), ref.bits(res[1][1])), "two blocks against one"


# ---- (c) two map slots, two tracks, a parameter row per agent -------------------------------------------------------------------------------
def test_two_map_slots_and_per_agent_parameters(amd):
    E, A, K, H, repeat = 6, 2, 64, 5, 3
    N = E * A
    sim = _two_maps(amd, E, A)
    env_map = np.arange(E) % 2
    sim.set_env_maps(env_map)
    rows = {mp: ref.grid_rows(mp) for mp in ref.GRID_MAPS}
    start, params = np.zeros((N, 10)), np.zeros((N, 18))
    for e in range(E):
        for a in range(A):
            q = (e // 2) * A + a
            start[e * A + a], params[e * A + a] = rows[ref.GRID_MAPS[env_map[e]]][0][q], rows[ref.GRID_MAPS[env_map[e]]][1][q]
    sim.set_params_batch(params)
    sim.reset(np.ascontiguousarray(start[:, [0, 1, 4]]))
    sim.set_state(start[:, :7], start[:, 7:9], start[:, 9].astype(np.int32))
    actions = ref.grid_actions(K, H, True, m=N)
    p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=ref.GRID_MARGIN, frame="ego", layout="per_agent", traj=True,
                    scale={"end_x": 2.0, "progress": 4.0})
    out, traj = sim.rollout(p, actions)
    s = ref.settings(**p.settings())
    for slot, mp in enumerate(ref.GRID_MAPS):
        idx = np.flatnonzero(np.repeat(env_map, A) == slot)
        flown = ref.fly(ref.scan_oracle(mp), start[idx], params[idx], actions[idx], True, repeat, ref.GRID_MARGIN, 1)
        w_out, _, w_traj, _ = ref.render(s, start[idx], flown, ref.grid_track(mp))
        keep = flown[4] >= 1e-9
        assert np.all(keep) and np.array_equal(out[idx][..., ref.ALIVE], flown[1].astype(np.float32)), mp
        assert rel_err(out[idx], w_out, atol=1e-6) < 1e-5 and rel_err(traj[idx], w_traj, atol=1e-6) < 1e-5, mp
    # the same rows through the unit form of each slot: the device form's floats bit for bit
    for slot in (0, 1):
        idx = np.flatnonzero(np.repeat(env_map, A) == slot)
        u_out, u_traj = sim.rollout_rows(p, start[idx], actions[idx], slot=slot, params=params[idx])
        assert np.array_equal(ref.bits(u_out), ref.bits(out[idx])) and np.array_equal(ref.bits(u_traj), ref.bits(traj[idx])), slot
    sim.close()


# ---- (c) no effect on the step -----------------------------------------------------------------------------------------------------------
def test_rollout_calls_change_no_step(amd):
    E, A, T = 32, 2, 100
    N = E * A
    rng = np.random.default_rng(5)
    acts = np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)
    p = amd.Rollout(k=8, horizon=3, repeat=2, channels=ALL10, margin=0.3, traj=True)
    cand = np.stack([rng.uniform(-0.4, 0.4, (8, 3)), rng.uniform(1.0, 7.0, (8, 3))], axis=-1)
    res = []
    for use in (False, True):
        s = amd.BatchSim(num_envs=E, num_agents=A)
        s.set_map_image(*load_map_image("example_map"))
        s.set_noise_rng(4242, 0.01)
        s.set_track(CSV)
        s.enable_track()
        start = bench_start_poses(E, A)
        s.reset(start)
        d_start = s.device_array((N, 3))
        d_start.upload(start)
        s.set_auto_reseat(d_start, 0)
        d_act, d_cand = s.device_array((N, 2)), s.device_array(cand.shape)
        d_cand.upload(cand)
        launches, bufs = [], None
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            launches.append(s.step_launches())
            if use:
                bufs = s.rollout_device(p, d_cand, *(bufs or ()))
        o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
        trk = s.get_track()
        res.append((launches, {k: np.array(v, copy=True) for k, v in list(o.items()) + list(trk.items())}, s.save_state().to_bytes()))
        s.close()
    assert res[0][0] == res[1][0], "f110_step_launches changed"
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k
    assert res[0][2] == res[1][2], "the state blobs differ"


# ---- (c) refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals_launch_and_write_nothing(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    L = _ffi.lib()
    good = amd.Rollout(k=3, horizon=2, repeat=2, channels=("end_x", "alive", "min_clear"), margin=0.2, traj=True)
    tracked = amd.Rollout(k=3, horizon=2, repeat=2, channels=("end_x", "progress"), traj=True)
    shape, tshape = good.shape(N), good.traj_shape(N)
    d_out, d_traj = s.device_array(shape, np.float32), s.device_array(tshape, np.float32)
    rng = np.random.default_rng(1)
    sentinel, tsentinel = rng.normal(size=shape).astype(np.float32), rng.normal(size=tshape).astype(np.float32)
    d_out.upload(sentinel)
    d_traj.upload(tsentinel)
    pin = s.pinned_empty(shape, np.float32)
    pin[...] = sentinel
    cand = np.tile([0.0, 2.0], (3, 2, 1))
    d_cand = s.device_array(cand.shape)
    d_cand.upload(cand)

    def call(base=good, p_act=None, p_out=None, p_traj=None, pinned=None, **fields):
        """f110_rollout_device with fields of the spec replaced; p_* = 0 passes a null pointer"""
        sp = base.spec()
        for k, v in fields.items():
            if k == "scale":
                sp.scale[v[0]] = v[1]
            else:
                setattr(sp, k, v)
        ptr = lambda given, mine: mine if given is None else (given or None)   # noqa: E731
        return L.f110_rollout_device(s._h, C.byref(sp), ptr(p_act, d_cand.ptr), ptr(p_out, d_out.ptr), ptr(p_traj, d_traj.ptr), pinned)

    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    inf, nan = float("inf"), float("nan")
    bad = [dict(k=0), dict(k=257), dict(k=-1), dict(horizon=0), dict(horizon=65), dict(repeat=0), dict(repeat=17), dict(layout=2), dict(layout=-1),
           dict(frame=2), dict(frame=-1), dict(channels=0), dict(channels=1024 | 1), dict(channels=-1), dict(traj=2), dict(traj=-1), dict(margin=nan),
           dict(scale=(0, 0.0)), dict(scale=(0, -1.0)), dict(scale=(6, nan)), dict(scale=(7, inf)), dict(scale=(1, 0.0)),   # (END_Y: read by the trajectory)
           dict(p_act=0), dict(p_out=0), dict(p_traj=0), dict(p_traj=d_traj.ptr + 8)]
    for f in bad:
        assert call(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
    assert call(scale=(4, 0.0)) == _ffi.OK                                            # (a clear bit's scale is ignored)
    d_out.upload(sentinel)
    d_traj.upload(tsentinel)
    heap = np.zeros(shape, dtype=np.float32)
    assert call(pinned=heap.ctypes.data) == _ffi.ERR_INVALID                          # not f110_host_alloc memory
    small = s.pinned_empty((N, 3, 2), np.float32)
    assert call(pinned=small.ctypes.data) == _ffi.ERR_INVALID                         # too small for [N][K][D]
    assert call(base=tracked) == _ffi.ERR_STATE and "no track" in _ffi.last_error(s._h)
    s.set_track(CSV)
    s.add_map_image(*load_map_image("example_map"))
    s.set_env_maps(np.arange(E) % 2)                                                  # slot 1, now in use, has no track
    assert call(base=tracked) == _ffi.ERR_STATE and "slot 1" in _ffi.last_error(s._h)
    nomap = amd.BatchSim(num_envs=1, num_agents=1)
    sp = amd.Rollout(k=1, horizon=1, channels=("alive",)).spec()
    tiny = nomap.device_array((1, 1, 2))
    assert L.f110_rollout_device(nomap._h, C.byref(sp), tiny.ptr, tiny.ptr, None, None) != _ffi.OK   # no map
    nomap.close()
    s.sync()
    assert np.array_equal(ref.bits(d_out.download()), ref.bits(sentinel)), "a refused call wrote d_out"
    assert np.array_equal(ref.bits(d_traj.download()), ref.bits(tsentinel)), "a refused call wrote d_traj"
    assert np.array_equal(ref.bits(np.array(pin)), ref.bits(sentinel))
    # the unit form refuses the same way and leaves the caller's arrays alone
    rows = np.zeros((N, 10))
    rows[:, [0, 1, 4]] = bench_start_poses(E, A)
    out, tr = sentinel.copy(), tsentinel.copy()
    dp = _ffi.dptr

    def unit(sp, slot=0, start=rows, m=N):
        return L.f110_rollout_batch(s._h, C.byref(sp), slot, dp(start), None, dp(cand), m, out.ctypes.data, None, tr.ctypes.data, None)

    sp = good.spec()
    sp.k = 257
    assert unit(sp) == _ffi.ERR_INVALID
    assert unit(good.spec(), slot=2) == _ffi.ERR_INVALID and unit(good.spec(), slot=-1) == _ffi.ERR_INVALID and unit(good.spec(), m=-1) == _ffi.ERR_INVALID
    assert unit(tracked.spec(), slot=1) == _ffi.ERR_STATE
    fill = rows.copy()
    fill[3, 9] = 3.0
    assert unit(good.spec(), start=fill) == _ffi.ERR_INVALID
    sp = good.spec()
    assert L.f110_rollout_batch(s._h, C.byref(sp), 0, dp(rows), None, dp(cand), N, out.ctypes.data, None, None, None) == _ffi.ERR_INVALID   # traj = 1, no h_traj
    assert np.array_equal(ref.bits(out), ref.bits(sentinel)) and np.array_equal(ref.bits(tr), ref.bits(tsentinel))
    with pytest.raises(ValueError):
        s.rollout_device(good, d_cand, s.device_array((N, 3, 2), np.float32))
    with pytest.raises(ValueError):
        s.rollout_device(good, s.device_array((3, 2, 3)))
    with pytest.raises(ValueError):
        s.rollout_device(amd.Rollout(k=3, horizon=2, channels=("alive",)), d_cand, traj=d_traj)
    with pytest.raises(ValueError):
        s.rollout(good, np.zeros((3, 3, 2)))
    with pytest.raises(ValueError):
        s.rollout_rows(good, np.zeros((N, 9)), cand)
    # and the good spec goes through, into the pinned block as well
    assert call(pinned=pin.ctypes.data) == _ffi.OK
    s.sync()
    got = d_out.download()
    assert not np.array_equal(got, sentinel) and np.array_equal(ref.bits(np.array(pin)), ref.bits(got))
    assert np.all(got[..., 1] == 4.0) and not np.array_equal(d_traj.download(), tsentinel)
    s.close()


# ---- (c) DLPack: a torch consumer in a fresh process ---------------------------------------------------------------------------------------
def test_torch_consumer_in_a_fresh_process():
    worker = os.path.join(HERE, "rollout_torch_worker.py")
    r = subprocess.run([sys.executable, worker], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    if "SKIP" in r.stdout:
        pytest.skip(r.stdout.strip().splitlines()[-1])
    assert "ROLLOUT TORCH OK" in r.stdout, r.stdout[-3000:]


# ---- (c) the example planner ---------------------------------------------------------------------------------------------------------------
def test_example_planner_runs():
    example = os.path.join(os.path.dirname(HERE), "examples", "rollout_planner.py")
    r = subprocess.run([sys.executable, example, "--envs", "8", "--steps", "50"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "steps" in r.stdout, r.stdout[-3000:]
