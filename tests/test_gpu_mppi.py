"""The MPPI planner on the device (f110_mppi_*), held to the Python model tests/mppi_ref.py.

(a) the unit form over the full cross K in {1, 2, 63, 64, 65, 256} x H in {1, 5} x repeat in {1, 3} x both integrators x both maps
    (example_map with its closed raceline, berlin with an open polyline; one test per map), six rows with their own parameter rows,
    and H = 64 at K = 3 under both integrators on both maps: the candidates V and the stream positions bit for bit; costs, weights,
    actions, nominal and info under the project's gate rel_err < 1e-5, finite exactly where the model's value is.
    A row whose model clearance comes within 1e-9 m of the margin at a visited step is left out (its ALIVE may differ by a step),
    and `best` is compared only where the model's two lowest costs differ by more than 1e-9 * max(1, |beta|); at most 1 % of the
    rows may be left out.  One kind of tie is not left out but compared: the grid's Euler cases with one sim step (and a few of
    three, where the speed command saturates the brake) give every candidate the same motion, because a step's position does
    not depend on that step's action; the tied candidates' ALIVE, MIN_CLEAR, PROGRESS and END_LAT are then the same bits in the
    model, the device computes one cost from one rollout as well, and `best` must be the model's first index.
(b) the device form on 45 envs x 2 cars at K = 3 (agents straddle waves and a workgroup) with every agent, every other agent and
    only the last agent armed: the armed rows against the model evaluated on the device's own state, the others untouched.
(c) ten consecutive plan-and-step calls with an env re-seated in mid-run; (d) two env blocks against one, two map slots with
    different tracks, get / put and a state blob; (e) no effect on the step; (f) the refusals and the env layers (a planner alone and
    beside gap followers against loops written by hand); (g) the example.
The kernels' lane groupings, limits and edge costs: tests/test_gpu_mppi_edges.py; the helpers both files share: tests/mppi_ref.py."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mppi_ref as ref
import rollout_ref as rr
from _util import MAPS, bench_start_poses, load_map_image, map_stem
from mppi_ref import check_rows, grid_settings, mppi_of, nominal_for, pin_fifo, same_bits, streams_for, two_maps, warm_sim

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(MAPS, "example_waypoints.csv")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


# ---- (a) the unit form against the model -----------------------------------------------------------------------------------------------
GRID_K = (1, 2, 63, 64, 65, 256)


def grid_cases(map_name):
    """every (K, H, repeat, integrator) on the map, and H = 64 at K = 3 under both integrators; q numbers the cases across both maps
    (it picks the seeds, the shift, the temperature and the lateral weight)"""
    cases, q = [], 100 * rr.GRID_MAPS.index(map_name)
    for K, H, repeat in [(K, H, repeat) for K in GRID_K for H in (1, 5) for repeat in (1, 3)] + [(3, 64, 1)]:
        for integrator in (1, 2):
            cases.append((map_name, K, H, repeat, integrator, q))
            q += 1
    return cases


GRID_FRESH = np.array([3, 0, 0, 7, 1, 2], dtype=np.int32)      # rows 1 and 2 (0.3 and 0.49 m/s) are fresh: they plan around v_init


def grid_inputs(case):
    """(settings, start, params, nominal, streams): the nominal speeds lie within 0.3 m/s of the row's own speed"""
    map_name, K, H, repeat, integrator, q = case
    s = grid_settings(case)
    start, params = rr.grid_rows(map_name)
    rng = np.random.default_rng(40 + q)
    nom = np.stack([rng.uniform(-0.2, 0.2, (6, H)), start[:, 3:4] + rng.uniform(-0.3, 0.3, (6, H))], axis=-1)
    return s, start, params, nom, streams_for(1000 + q, range(6))


@pytest.mark.parametrize("grid_map", rr.GRID_MAPS)
def test_unit_form_matches_model_over_the_grid(amd, grid_map):
    sims = {integ: two_maps(amd, integrator=integ) for integ in (1, 2)}
    stats = {"rows": 0, "left_out": 0, "rel_err": 0.0}
    steps = 0
    for case in grid_cases(grid_map):
        map_name, K, H, repeat, integrator, q = case
        s, start, params, nom, words = grid_inputs(case)
        fresh = GRID_FRESH
        want = ref.plan(s, rr.scan_oracle(map_name), start, params, nom, words, integrator, fresh, rr.grid_track(map_name))
        got = sims[integrator].mppi_rows(mppi_of(amd, s), start, nom, words, slot=rr.GRID_MAPS.index(map_name), params=params, fresh=fresh)
        check_rows(s, want, got, case, stats)
        steps += 6 * K * H * repeat
    print("mppi unit grid on %s: %d rows, %d left out, %d candidate-steps, largest rel_err %.3e" % (grid_map, stats["rows"], stats["left_out"], steps, stats["rel_err"]))
    assert stats["left_out"] * 100 <= stats["rows"], stats
    for sim in sims.values():
        sim.close()


# ---- (b) the device form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("armed", ["all", "every_other", "last"])
def test_device_form_45_envs_of_2_cars(amd, armed):
    E, A, seed = 45, 2, 321
    N = E * A
    sim, start = warm_sim(amd, E, A)
    agents = {"all": np.arange(N), "every_other": np.arange(0, N, 2), "last": np.array([N - 1])}[armed]
    s = ref.settings(k=3, horizon=5, repeat=3, w_progress=3.0, w_lat=0.5, margin=0.25)
    sim.set_mppi(mppi_of(amd, s), agents, seed=seed)
    rng = np.random.default_rng(9)
    poison_a, poison_i = rng.normal(size=(N, 2)), rng.normal(size=(N, 4)).astype(np.float32)
    d_act, d_info = sim.device_array((N, 2)), sim.device_array((N, 4), np.float32)
    d_act.upload(poison_a)
    d_info.upload(poison_i)
    sim.mppi_device(d_act, d_info)
    act, info = d_act.download(), d_info.download()
    nom, words = sim.get_mppi_state()
    other = np.setdiff1d(np.arange(N), agents)
    assert same_bits(act[other], poison_a[other]) and same_bits(info[other], poison_i[other]), "a row of an agent that is not armed was written"
    params = np.tile(rr.orc.params_vec(), (len(agents), 1))
    mp = mppi_of(amd, s)
    want = ref.plan(s, rr.scan_oracle("example_map"), start[agents], params, mp.fresh_nominal(len(agents)), streams_for(seed, agents), 1,
                    sim.get("step_count")["step_count"][agents], rr.grid_track("example_map"))
    stats = {"rows": 0, "left_out": 0, "rel_err": 0.0}
    check_rows(s, want, dict(actions=act[agents], info=info[agents], nominal=nom, streams=words), armed, stats)
    assert stats["left_out"] * 100 <= stats["rows"], stats
    # the step takes the planner's actions as they are
    sim.step_device(d_act)
    sim.sync()
    sim.close()


# ---- (c) ten consecutive plan-and-step calls -----------------------------------------------------------------------------------------------
def test_ten_plan_and_step_calls_with_a_reseat(amd):
    E, A, seed = 4, 2, 77
    N = E * A
    sim, start = warm_sim(amd, E, A, steps=5)
    s = ref.settings(k=5, horizon=4, repeat=2, w_progress=3.0, margin=0.25, lam=0.6)
    sim.set_mppi(mppi_of(amd, s), None, seed=seed)
    so, track = rr.scan_oracle("example_map"), rr.grid_track("example_map")
    params = np.tile(rr.orc.params_vec(), (N, 1))
    d_act = sim.device_array((N, 2))
    first = streams_for(seed, range(N))
    rng = np.random.default_rng(3)
    poses0 = bench_start_poses(E, A)
    stats = {"rows": 0, "left_out": 0, "rel_err": 0.0}
    fresh_seen = 0
    for t in range(10):
        if t == 5:   # env 1 is re-seated: its cars' step_count is 0, their rows are fresh
            sim.reset(poses0, np.array([0, 1, 0, 0], dtype=np.uint8))
            start = pin_fifo(sim, rng, np.where(np.arange(N)[:, None] // A == 1, 0.0, start[:, 7:9]), np.where(np.arange(N) // A == 1, 0, 2).astype(np.int32))
        nom, words = sim.get_mppi_state()
        count = sim.get("step_count")["step_count"]
        fresh_seen += int(np.count_nonzero(count == 0))
        assert same_bits(words, np.stack([ref.words_of(ref.generator(first[n], t << 28)) for n in range(N)])), "call %d: the streams' positions" % t
        want = ref.plan(s, so, start, params, nom, words, 1, count, track)
        sim.mppi_device(d_act)
        act = d_act.download()
        nom1, words1 = sim.get_mppi_state()
        check_rows(s, want, dict(actions=act, info=want["info"], nominal=nom1, streams=words1), "call %d" % t, stats)
        if t == 5:
            assert np.all(count[2:4] == 0) and np.all(want["candidates"][2:4, 0, :, 0] == 0.0) and np.all(want["candidates"][2:4, 0, :, 1] == s["v_init"])
        sim.step_device(d_act)
        start = pin_fifo(sim, rng, np.stack([act[:, 0], start[:, 7]], axis=1), np.minimum(start[:, 9] + 1, 2).astype(np.int32))
    assert fresh_seen == 2 and stats["left_out"] * 100 <= stats["rows"], (fresh_seen, stats)
    sim.close()


# ---- (d) two env blocks against one, two map slots, get / put and a state blob ---------------------------------------------------------------
def test_two_env_blocks_against_one(amd):
    E, A, T = 512, 2, 4
    N = E * A
    mp = amd.Mppi(k=8, horizon=4, repeat=2, w_progress=3.0, w_lat=0.2, margin=0.3)
    agents = np.arange(1, N, 2)
    res = []
    for groups in (1, 2):
        s = amd.BatchSim(num_envs=E, num_agents=A, step_groups=groups)
        s.set_map_image(*load_map_image("example_map"))
        s.set_noise_rng(4242, 0.01)
        s.set_track(CSV)
        s.reset(bench_start_poses(E, A))
        s.set_mppi(mp, agents, seed=5)
        d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4), np.float32)
        d_act.upload(np.tile([0.05, 3.0], (N, 1)))
        d_info.upload(np.zeros((N, 4), dtype=np.float32))
        for t in range(T):
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            s.mppi_device(d_act, d_info)
            s.step_device(d_act)                       # a step right behind the call keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            s.mppi_device(d_act, d_info)
        s.sync()
        res.append((d_act.download(), d_info.download()) + s.get_mppi_state() + (s.get("state")["state"],))
        s.close()
    for a, b in zip(*res):
        assert same_bits(a, b), "two blocks against one"
    assert not np.array_equal(res[0][0][agents], np.tile([0.05, 3.0], (len(agents), 1))) and np.all(res[0][0][::2] == [0.05, 3.0])


def test_two_map_slots_with_different_tracks(amd):
    E, A = 6, 2
    N = E * A
    sim = two_maps(amd, E, A)
    env_map = np.arange(E) % 2
    sim.set_env_maps(env_map)
    rows = {mp: rr.grid_rows(mp) for mp in rr.GRID_MAPS}
    start, params = np.zeros((N, 10)), np.zeros((N, 18))
    for e in range(E):
        for a in range(A):
            q = (e // 2) * A + a
            start[e * A + a], params[e * A + a] = rows[rr.GRID_MAPS[env_map[e]]][0][q], rows[rr.GRID_MAPS[env_map[e]]][1][q]
    sim.set_params_batch(params)
    sim.reset(np.ascontiguousarray(start[:, [0, 1, 4]]))
    sim.set_state(start[:, :7], start[:, 7:9], start[:, 9].astype(np.int32))
    sim.step(np.tile([0.05, 2.0], (N, 1)))                        # (one step: no row is fresh, the seeded nominal is what the call draws around)
    start = pin_fifo(sim, np.random.default_rng(6))
    s = ref.settings(k=64, horizon=5, repeat=3, w_progress=3.0, w_lat=0.5, margin=rr.GRID_MARGIN)
    mp = mppi_of(amd, s)
    sim.set_mppi(mp, None, seed=8)
    nom0 = nominal_for(s, N, 2)
    sim.set_mppi_state(nominal=nom0)
    got_nom, words0 = sim.get_mppi_state()
    assert same_bits(got_nom, nom0) and same_bits(words0, streams_for(8, range(N)))
    act, info = sim.mppi(np.zeros((N, 2)), info=True)
    nom1, words1 = sim.get_mppi_state()
    count = sim.get("step_count")["step_count"]
    assert np.all(count == 1)
    stats = {"rows": 0, "left_out": 0, "rel_err": 0.0}
    for slot, name in enumerate(rr.GRID_MAPS):
        idx = np.flatnonzero(np.repeat(env_map, A) == slot)
        want = ref.plan(s, rr.scan_oracle(name), start[idx], params[idx], nom0[idx], words0[idx], 1, count[idx], rr.grid_track(name))
        check_rows(s, want, dict(actions=act[idx], info=info[idx], nominal=nom1[idx], streams=words1[idx]), name, stats)
        # the same rows through the unit form of the slot: the device form's numbers bit for bit
        unit = sim.mppi_rows(mp, start[idx], nom0[idx], words0[idx], slot=slot, params=params[idx], fresh=count[idx])
        for key, mine in (("actions", act), ("info", info), ("nominal", nom1), ("streams", words1)):
            assert same_bits(unit[key], mine[idx]), (name, key)
    assert stats["left_out"] * 100 <= stats["rows"], stats
    sim.close()


def test_get_put_and_a_state_blob_reproduce_the_next_action(amd):
    E, A = 8, 2
    N = E * A
    sim, _ = warm_sim(amd, E, A, steps=6)
    sim.set_noise_rng(99, 0.01)
    mp = amd.Mppi(k=16, horizon=6, repeat=2, w_progress=3.0, margin=0.3)
    sim.set_mppi(mp, np.arange(0, N, 3), seed=4)
    d_act = sim.device_array((N, 2))
    d_act.upload(np.tile([0.0, 2.0], (N, 1)))
    for _ in range(3):
        sim.mppi_device(d_act)
        sim.step_device(d_act)
    blob, planner = sim.save_state(), sim.get_mppi_state()
    seq = []
    for _ in range(3):
        sim.mppi_device(d_act)
        seq.append(d_act.download())
        sim.step_device(d_act)
    after = sim.get_mppi_state()
    assert not same_bits(after[0], planner[0]) and not same_bits(after[1], planner[1])
    sim.load_state(blob)                            # the blob does not hold the planner: its state is still the later one
    assert same_bits(sim.get_mppi_state()[1], after[1])
    sim.set_mppi_state(*planner)
    d_act.upload(np.tile([0.0, 2.0], (N, 1)))
    for t in range(3):
        sim.mppi_device(d_act)
        assert same_bits(d_act.download(), seq[t]), "call %d after the restore" % t
        sim.step_device(d_act)
    for a, b in zip(sim.get_mppi_state(), after):
        assert same_bits(a, b)
    sim.close()


# ---- (e) no effect on the step -----------------------------------------------------------------------------------------------------------
def test_planner_calls_change_no_step(amd):
    E, A, T = 32, 2, 100
    N = E * A
    rng = np.random.default_rng(5)
    acts = np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)
    mp = amd.Mppi(k=8, horizon=3, repeat=2, w_progress=3.0, w_lat=0.3, margin=0.3)
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
        d_act, d_plan, d_info = s.device_array((N, 2)), s.device_array((N, 2)), s.device_array((N, 4), np.float32)
        if use:
            s.set_mppi(mp, None, seed=1)
        launches = []
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            launches.append(s.step_launches())
            if use:
                s.mppi_device(d_plan, d_info)       # (into a buffer of its own: the step's actions are the same in both runs)
        o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
        trk = s.get_track()
        res.append((launches, {k: np.array(v, copy=True) for k, v in list(o.items()) + list(trk.items())}, s.save_state().to_bytes()))
        s.close()
    assert res[0][0] == res[1][0], "f110_step_launches changed"
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k
    assert res[0][2] == res[1][2], "the state blobs differ"


# ---- (f) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_planner_alone(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    L = _ffi.lib()
    u64 = _ffi._u64p
    good = amd.Mppi(k=4, horizon=3, repeat=2, w_progress=0.0, w_lat=0.0)
    tracked = amd.Mppi(k=4, horizon=3, repeat=2, w_progress=1.0)
    agents = np.arange(0, N, 2, dtype=np.int32)
    words = np.ascontiguousarray(streams_for(1, agents))
    rng = np.random.default_rng(1)
    poison_a, poison_i = rng.normal(size=(N, 2)), rng.normal(size=(N, 4)).astype(np.float32)
    d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4), np.float32)
    d_act.upload(poison_a)
    d_info.upload(poison_i)
    assert L.f110_mppi_device(s._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE and "armed" in _ffi.last_error(s._h)      # nothing armed
    assert L.f110_mppi_get(s._h, None, None) == _ffi.ERR_STATE and L.f110_mppi_put(s._h, None, None) == _ffi.ERR_STATE
    s.set_mppi(good, agents, seed=1)
    before = s.get_mppi_state()

    def arm(base=good, ag=agents, m=None, w=words, **fields):
        sp = base.spec()
        for k, v in fields.items():
            setattr(sp, k, v)
        ag = np.ascontiguousarray(ag, dtype=np.int32)
        return L.f110_mppi_set(s._h, C.byref(sp), _ffi.i32ptr(ag), len(ag) if m is None else m, w.ctypes.data_as(u64))

    inf, nan = float("inf"), float("nan")
    bad = [dict(k=0), dict(k=257), dict(k=-1), dict(horizon=0), dict(horizon=65), dict(repeat=0), dict(repeat=17), dict(shift=2), dict(shift=-1),
           dict(margin=nan), dict(sigma_steer=-1.0), dict(sigma_speed=-0.1), dict(sigma_steer=inf), dict(steer_min=1.0), dict(speed_min=100.0),
           dict(lambda_=0.0), dict(lambda_=-1.0), dict(lambda_=nan), dict(w_dead=-1.0), dict(w_clear=-1.0), dict(w_progress=-1.0), dict(w_lat=-1.0),
           dict(w_dead=inf), dict(clear_ref=nan), dict(v_init=0.0), dict(v_init=100.0), dict(v_init=nan),
           dict(ag=[3, 3]), dict(ag=[5, 2]), dict(ag=[-1, 2]), dict(ag=[0, N]), dict(m=0), dict(m=N + 1)]
    for f in bad:
        assert arm(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
    sp = good.spec()
    assert L.f110_mppi_set(s._h, C.byref(sp), None, 3, words.ctypes.data_as(u64)) == _ffi.ERR_INVALID
    assert L.f110_mppi_set(s._h, C.byref(sp), _ffi.i32ptr(agents), len(agents), None) == _ffi.ERR_INVALID
    assert L.f110_mppi_device(s._h, None, None) == _ffi.ERR_INVALID
    # an agent cannot have a follow-the-gap controller and the planner, whichever comes second
    assign = np.full(N, -1, dtype=np.int32)
    assign[2] = 0
    with pytest.raises(ValueError):
        s.set_controllers(assign, [amd.GapFollower()])
    assign[:] = -1
    assign[1] = 0
    s.set_controllers(assign, [amd.GapFollower()])
    assert arm(ag=[0, 1]) == _ffi.ERR_INVALID and "follow-the-gap" in _ffi.last_error(s._h)
    s.clear_controllers()
    # put: values that are not finite or outside the bounds
    for value, where in ((nan, (0, 0, 0)), (inf, (1, 2, 1)), (good.steer_max + 0.1, (0, 1, 0)), (good.speed_min - 0.1, (2, 0, 1))):
        nom = before[0].copy()
        nom[where] = value
        with pytest.raises(ValueError):
            s.set_mppi_state(nominal=nom)
    with pytest.raises(ValueError):
        s.set_mppi_state(nominal=np.zeros((3, 3, 2)))
    with pytest.raises(ValueError):
        s.mppi_device(d_act, s.device_array((N, 3), np.float32))
    # every refusal so far changed nothing: the planner is the one armed first, the outputs hold their pattern
    for a, b in zip(s.get_mppi_state(), before):
        assert same_bits(a, b)
    s.sync()
    assert same_bits(d_act.download(), poison_a) and same_bits(d_info.download(), poison_i), "a refused call wrote an output"
    # a track weight without a track, and on a slot in use without one
    s.set_mppi(tracked, agents, seed=1)
    assert L.f110_mppi_device(s._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE and "no track" in _ffi.last_error(s._h)
    s.set_track(CSV)
    s.add_map_image(*load_map_image("example_map"))
    s.set_env_maps(np.arange(E) % 2)
    assert L.f110_mppi_device(s._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE and "slot 1" in _ffi.last_error(s._h)
    assert same_bits(d_act.download(), poison_a) and same_bits(d_info.download(), poison_i)
    # the unit form refuses the same way and leaves the caller's arrays alone
    rows = np.zeros((4, 10))
    rows[:, [0, 1, 4]] = bench_start_poses(4, 1)
    nom, w4 = good.fresh_nominal(4), np.ascontiguousarray(streams_for(2, range(4)))
    act = poison_a[:4].copy()

    def unit(sp, slot=0, start=rows, m=4, nominal=nom):
        return L.f110_mppi_batch(s._h, C.byref(sp), slot, _ffi.dptr(start), None, None, m, _ffi.dptr(nominal), w4.ctypes.data_as(u64), _ffi.dptr(act),
                                 None, None, None, None)

    sp = good.spec()
    sp.k = 257
    assert unit(sp) == _ffi.ERR_INVALID
    assert unit(good.spec(), slot=2) == _ffi.ERR_INVALID and unit(good.spec(), slot=-1) == _ffi.ERR_INVALID and unit(good.spec(), m=-1) == _ffi.ERR_INVALID
    assert unit(tracked.spec(), slot=1) == _ffi.ERR_STATE
    fill = rows.copy()
    fill[3, 9] = 3.0
    assert unit(good.spec(), start=fill) == _ffi.ERR_INVALID
    wild = nom.copy()
    wild[1, 1, 0] = nan
    assert unit(good.spec(), nominal=wild) == _ffi.ERR_INVALID
    assert same_bits(act, poison_a[:4]) and same_bits(w4, streams_for(2, range(4))) and same_bits(nom, good.fresh_nominal(4))
    assert unit(good.spec()) == _ffi.OK and not same_bits(act, poison_a[:4])
    # disarmed: the call is refused again, and the scripted step with nothing armed as well
    s.clear_mppi()
    assert L.f110_mppi_device(s._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE
    nomap = amd.BatchSim(num_envs=1, num_agents=1)
    nomap.set_mppi(good, None, seed=0)
    tiny = nomap.device_array((1, 2))
    assert L.f110_mppi_device(nomap._h, tiny.ptr, None) == _ffi.ERR_STATE and "map" in _ffi.last_error(nomap._h)
    nomap.close()
    s.close()


# ---- (f) the env layers ---------------------------------------------------------------------------------------------------------------------
ENV_KW = dict(num_agents=2, map=map_stem("example_map"), map_ext=".png", seed=31, device_logic=True, auto_reset=True,
              obs_fields=("poses_x", "poses_y", "poses_theta", "linear_vels_x", "collisions"))


def env_planner(amd):
    return amd.Mppi(k=8, horizon=4, repeat=3, w_progress=4.0, margin=0.3, speed_max=5.0)


def run_env(env, E, T=20):
    rng = np.random.default_rng(2)
    out = [env.reset(bench_start_poses(E, 2).reshape(E, 2, 3))[0]]
    out = [{k: np.array(v, copy=True) for k, v in out[0].items() if isinstance(v, np.ndarray)}]
    for _ in range(T):
        act = np.stack([rng.uniform(-0.1, 0.1, (E, 2)), rng.uniform(1.0, 3.0, (E, 2))], axis=-1)
        obs = env.step(act)[0]
        out.append({k: np.array(v, copy=True) for k, v in obs.items() if isinstance(v, np.ndarray)})
    return out


def test_vec_env_scripted_planner_is_the_hand_written_loop(amd):
    E = 6
    track = amd.Track.from_csv(CSV)
    env = amd.F110VecEnv(E, scripted={1: env_planner(amd)}, track=track, **ENV_KW)
    mine = run_env(env, E)
    env.sim.batch.close()
    # by hand: the planner armed on the handle of an env without scripted cars, its action read back and handed to step()
    hand = amd.F110VecEnv(E, track=track, **ENV_KW)
    b = hand.sim.batch
    b.set_mppi(env_planner(amd), np.arange(E) * 2 + 1, seed=ENV_KW["seed"])
    d_act = b.device_array((2 * E, 2))

    class ByHand(object):
        def reset(self, poses):
            b.episode_reset(poses.reshape(-1, 3))
            hand._start_poses = poses.copy()
            hand.sim._steps_since_full_reset = 0
            return self.step(np.zeros((E, 2, 2)))

        def step(self, act):
            d_act.upload(np.ascontiguousarray(act.reshape(-1, 2)))
            b.mppi_device(d_act)
            return hand.step(d_act.download().reshape(E, 2, 2))

    theirs = run_env(ByHand(), E)
    b.close()
    for t, (x, y) in enumerate(zip(mine, theirs)):
        for k in x:
            assert same_bits(x[k], y[k]), (t, k)
    assert mine[-1]["linear_vels_x"][:, 1].min() > 0.5, "the planner's cars do not move"
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, scripted={1: env_planner(amd)}, track=track, **dict(ENV_KW, device_logic=False))
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, scripted={0: env_planner(amd), 1: env_planner(amd)}, track=track, **ENV_KW)
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, scripted={1: env_planner(amd)}, **ENV_KW)               # a track weight without a track


def test_vec_env_gap_followers_and_planner_are_the_hand_written_loop(amd):
    """car 0 of every env follows the gap, car 1 plans: the scripted step against a loop written by hand on a plain env's handle —
    the controllers' device call, then the planner's, then the step — every observation bit for bit"""
    from f1tenth_gym_amd.gap_follower import coerce_scripted
    E = 6
    track = amd.Track.from_csv(CSV)
    env = amd.F110VecEnv(E, scripted={0: amd.GapFollower(), 1: env_planner(amd)}, track=track, **ENV_KW)
    mine = run_env(env, E)
    env.sim.batch.close()
    hand = amd.F110VecEnv(E, track=track, **ENV_KW)
    b = hand.sim.batch
    b.set_controllers(*coerce_scripted({0: amd.GapFollower()}, E, 2))
    b.set_mppi(env_planner(amd), np.arange(E) * 2 + 1, seed=ENV_KW["seed"])
    d_act = b.device_array((2 * E, 2))
    seen = []

    class ByHand(object):
        def reset(self, poses):
            b.episode_reset(poses.reshape(-1, 3))
            hand._start_poses = poses.copy()
            hand.sim._steps_since_full_reset = 0
            return self.step(np.zeros((E, 2, 2)))

        def step(self, act):
            d_act.upload(np.ascontiguousarray(act.reshape(-1, 2)))
            b.follow_gap_device(d_act)
            b.mppi_device(d_act)
            seen.append((act.reshape(-1, 2).copy(), d_act.download()))
            return hand.step(seen[-1][1].reshape(E, 2, 2))

    theirs = run_env(ByHand(), E)
    b.close()
    for t, (x, y) in enumerate(zip(mine, theirs)):
        for k in x:
            assert same_bits(x[k], y[k]), (t, k)
    # both kinds of scripted car replaced their rows (after the reset's own step), and both drive
    assert all(np.all(given != taken) for given, taken in seen[2:])
    assert mine[-1]["linear_vels_x"][:, 1].min() > 0.5 and mine[-1]["linear_vels_x"][:, 0].max() > 0.0, "the scripted cars do not move"


def test_sharded_env_draws_the_numbers_of_one_handle(amd):
    E = 6
    track = amd.Track.from_csv(CSV)
    one = amd.F110VecEnv(E, scripted={0: amd.GapFollower(), 1: env_planner(amd)}, track=track, **ENV_KW)
    a = run_env(one, E, T=12)
    one.sim.batch.close()
    two = amd.ShardedVecEnv(E, devices=[0, 0], scripted={0: amd.GapFollower(), 1: env_planner(amd)}, track=track, **ENV_KW)
    b = run_env(two, E, T=12)
    two.close()
    for t, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert same_bits(np.asarray(x[k]), np.asarray(y[k])), (t, k)


# ---- (g) the example ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("obstacles", [0, 6])
def test_example_planner_drives(obstacles):
    example = os.path.join(os.path.dirname(HERE), "examples", "mppi_planner.py")
    r = subprocess.run([sys.executable, example, "--envs", "8", "--steps", "300", "--obstacles", str(obstacles)], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert not res["nan"] and res["progress_min"] > 0.0, res
