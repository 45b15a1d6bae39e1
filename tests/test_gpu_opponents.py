"""The opponent term on the device (f110_rollout_opp_*, f110_mppi_set_opponents, f110_mppi_opp_batch), held to the
Python model tests/opponents_ref.py.

(a) the unit form over both maps x K in {1, 63, 64, 65} x H in {1, 2, 8} x repeat in {1, 3} x Ao in {0, 1, 2, 4} x both modes, three
    rows: the predictions under the project's gate rel_err < 1e-5, finite exactly where the model's are; (OPP_MIN,
    OPP_FREE) against the model evaluated on the device's own trajectory and predictions: OPP_FREE exactly, OPP_MIN under the gate.
    A candidate with a sample within 1e-9 * radius of the radius may be left out, at most 1 % (tests/test_opponents_host.py shows
    that the model's own motion leaves none out on this grid).
(b) the device form on 45 envs x 2 cars and 20 envs x 3 cars: d_opp bit for bit the unit form on the state fetched before it,
    d_out and d_traj bit for bit f110_rollout_device's.
(c) the planner with the term on every, every other and only the last agent: bit for bit the unit form, the costs against the model
    on the device's own rollout values; zero weights and A = 1 are the detached call; a car parked ahead changes the plan.
(d) env blocks, two map slots (one a derived obstacle slot) in TRACK mode, the scripted step, the env layers.
(e) no effect on the step; the refusals; the device allocations.  (f) the example."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import mppi_ref as mr
import opponents_ref as ref
import rollout_ref as rr
from _util import MAPS, bench_start_poses, load_map_image, map_stem
from mppi_ref import gated, mppi_of, pin_fifo, same_bits, streams_for, two_maps, warm_sim
from opponents_ref import live_opponents

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSV = os.path.join(MAPS, "example_waypoints.csv")
GATE = 1e-5
INF, NAN = float("inf"), float("nan")
ALL10 = rr.CHANNELS


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def opp_of(amd, s):
    return amd.Opponents(**s)


# ---- (a) the unit form against the model -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("grid_map", rr.GRID_MAPS)
def test_unit_form_matches_model_over_the_grid(amd, grid_map, mode):
    sim = two_maps(amd)
    slot, track = rr.GRID_MAPS.index(grid_map), rr.grid_track(grid_map)
    cands = left = 0
    worst = 0.0
    for case in ref.gpu_cases((grid_map,), (mode,)):
        _, K, H, repeat, _, Ao = case
        s = ref.grid_settings(mode, Ao)
        start, params, actions, opp = ref.gpu_inputs(case)
        p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=rr.GRID_MARGIN, frame="ego", traj=True)
        got = sim.rollout_opp_rows(p, opp_of(amd, s), start, actions, opp, slot=slot, params=params)
        # d_out and the trajectory are the plain rollout's, bit for bit
        plain = sim.rollout_rows(p, start, actions, slot=slot, params=params, raw=True)
        for a, b in zip((got["out"], got["traj"], got["raw"], got["traj_raw"]), plain):
            assert same_bits(a, b), (case, "the rollout's own outputs changed")
        want_pred = np.stack([ref.predict(s, start[n, 0], start[n, 1], opp[n], H, repeat, track=track) for n in range(len(start))]) \
            if Ao else np.zeros((len(start), 0, H, 2))
        err = gated(got["pred"], want_pred, (case, "pred"))
        assert err < GATE, (case, "pred rel_err %.3e" % err)
        worst = max(worst, err)
        # the samples on the device's OWN positions and predictions.  The trajectory is in the ego frame here (the term reads the map
        # frame whatever the spec says), so the positions are the map-frame ones of a second call
        pm = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=rr.GRID_MARGIN, frame="map", traj=True)
        gm = sim.rollout_opp_rows(pm, opp_of(amd, s), start, actions, opp, slot=slot, params=params)
        assert same_bits(gm["opp_raw"], got["opp_raw"]) and same_bits(gm["pred"], got["pred"]), (case, "the spec's frame changed the term")
        want_raw, near = ref.sample_rows(s, gm["traj_raw"], got["pred"])
        keep = ~ref.left_out(near, s["radius"])
        cands += keep.size
        left += int(np.count_nonzero(~keep))
        assert np.array_equal(got["opp_raw"][..., 1][keep], want_raw[..., 1][keep]), (case, "OPP_FREE")
        err = gated(got["opp_raw"][..., 0][keep], want_raw[..., 0][keep], (case, "OPP_MIN"))
        assert err < GATE, (case, "OPP_MIN rel_err %.3e" % err)
        worst = max(worst, err)
        assert same_bits(got["opp"], got["opp_raw"].astype(np.float32)), (case, "the float32 output")
        if Ao == 0:
            assert np.all(got["opp_raw"][..., 0] == INF) and np.all(got["opp_raw"][..., 1] == H)
    print("opponents unit grid on %s, %s: %d candidates, %d left out, largest rel_err %.3e" % (grid_map, mode, cands, left, worst))
    assert left * 100 <= cands
    sim.close()


# ---- (b) the device form -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,A", [(45, 2), (20, 3)])
@pytest.mark.parametrize("mode", ref.MODES)
def test_device_form_is_the_unit_form(amd, E, A, mode):
    N = E * A
    sim, start = warm_sim(amd, E, A)
    K, H, repeat = 5, 6, 3
    p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=0.25, frame="ego", traj=True, layout="per_agent")
    op = amd.Opponents(mode=mode, radius=2.0, max_range=3.0)         # the cars of an env start 10 waypoints (2 m) apart; a third one is out of range
    actions = rr.grid_actions(K, H, True, m=N)
    d_act = sim.device_array(actions.shape)
    d_act.upload(actions)
    out0, traj0 = sim.rollout_device(p, d_act)
    out, traj, opp = sim.rollout_opp_device(p, op, d_act)
    sim.sync()
    assert same_bits(out.download(), out0.download()) and same_bits(traj.download(), traj0.download()), "d_out / d_traj are not f110_rollout_device's"
    unit = sim.rollout_opp_rows(p, op, start, actions, live_opponents(start[:, :7], A))
    got = opp.download()
    assert same_bits(got, unit["opp"]), "d_opp is not the unit form's"
    assert same_bits(out.download(), unit["out"])
    assert np.all(np.isfinite(got[..., 0])) and np.all((got[..., 1] >= 0) & (got[..., 1] <= H)), "every agent has an opponent in range"
    print("device form %d x %d, %s: %d of %d candidates come within the radius" % (E, A, mode, np.count_nonzero(got[..., 1] < H), got[..., 1].size))
    host = sim.rollout_opp(p, op, actions)
    assert same_bits(host[2], got) and same_bits(host[0], out.download())
    sim.close()


# ---- (c) the planner ---------------------------------------------------------------------------------------------------------------------
W = (3.0, 1.5, 2.5)      # w_hit, w_near, near_ref: the cars of an env are about 2 m apart, so both terms act


@pytest.mark.parametrize("armed", ["all", "every_other", "last"])
def test_planner_device_form_45_envs_of_2_cars(amd, armed):
    E, A, seed = 45, 2, 321
    N = E * A
    sim, start = warm_sim(amd, E, A)
    agents = {"all": np.arange(N), "every_other": np.arange(0, N, 2), "last": np.array([N - 1])}[armed]
    s = mr.settings(k=3, horizon=5, repeat=3, w_progress=3.0, w_lat=0.5, margin=0.25)
    os_ = ref.settings(mode="track", radius=2.0, max_range=8.0)
    mp, op = mppi_of(amd, s), opp_of(amd, os_)
    sim.set_mppi(mp, agents, seed=seed)
    sim.set_mppi_opponents(op, *W)
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
    fresh = sim.get("step_count")["step_count"][agents]
    opp = live_opponents(start[:, :7], A)[agents]
    unit = sim.mppi_opp_rows(mp, op, W[0], W[1], W[2], start[agents], mp.fresh_nominal(len(agents)), streams_for(seed, agents), opp, params=params, fresh=fresh)
    for key, mine in (("actions", act[agents]), ("info", info[agents]), ("nominal", nom), ("streams", words)):
        assert same_bits(unit[key], mine), (armed, key)
    # the costs against the model on the device's own rollout values: the candidates rolled by the plain rollout's unit form
    ro = amd.Rollout(k=s["k"], horizon=s["horizon"], repeat=s["repeat"], channels=ALL10, margin=s["margin"], frame="map", traj=True, layout="per_agent")
    rolled = sim.rollout_opp_rows(ro, op, start[agents], unit["candidates"], opp, params=params)
    raw4 = rolled["raw"][..., [rr.ALIVE, rr.MIN_CLEAR, rr.PROGRESS, rr.END_LAT]]
    want = ref.costs(s, W[0], W[1], W[2], raw4, unit["opp_raw"])
    err = gated(unit["cost"], want, (armed, "cost"))
    assert err < GATE, err
    assert np.any(unit["opp_raw"][..., 0] < W[2]) and np.any(unit["opp_raw"][..., 1] < s["horizon"]), "no candidate comes near an opponent: the case shows nothing"
    sim.step_device(d_act)
    sim.sync()
    sim.close()


def test_zero_weights_and_one_car_are_the_detached_call(amd):
    res = {}
    for A in (2, 1):
        E = 12
        N = E * A
        for attach in (False, True):
            sim, _ = warm_sim(amd, E, A, steps=8)
            sim.set_mppi(amd.Mppi(k=64 if A == 1 else 7, horizon=4, repeat=2, w_progress=3.0, w_lat=0.3, margin=0.3), None, seed=3)
            if attach:
                sim.set_mppi_opponents(amd.Opponents(mode="track", radius=0.7), 0.0 if A == 2 else 5.0, 0.0 if A == 2 else 2.0, 1.0)
            d_act, d_info = sim.device_array((N, 2)), sim.device_array((N, 4), np.float32)
            d_act.upload(np.zeros((N, 2)))
            d_info.upload(np.zeros((N, 4), dtype=np.float32))
            for _ in range(3):
                sim.mppi_device(d_act, d_info)
                sim.step_device(d_act)
            res[A, attach] = (d_act.download(), d_info.download()) + sim.get_mppi_state()
            sim.close()
        for a, b in zip(res[A, False], res[A, True]):
            assert same_bits(a, b), "A = %d: the attached call differs from the detached one" % A


def test_a_car_parked_ahead_changes_the_plan(amd):
    """the ego at rest on the raceline, a car parked 1.5 m ahead on its heading, w_hit > 0: every candidate that comes within the
    radius costs exactly w_hit * (H - free) more than in the detached call, and the planned steer differs"""
    E, A, K, H = 1, 2, 64, 10
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map_image(*load_map_image("example_map"))
    x, y, th = bench_start_poses(1, 1)[0]
    poses = np.array([[x, y, th], [x + 1.5 * math.cos(th), y + 1.5 * math.sin(th), th]])
    sim.reset(poses)
    state = sim.get("state")["state"]
    state[0, 3] = 3.0                                                     # the ego drives at 3 m/s, the other car stands
    sim.set_state(state, np.zeros((2, 2)), np.full(2, 2, dtype=np.int32))
    mp = amd.Mppi(k=K, horizon=H, repeat=5, shift=False, margin=0.2, sigma_steer=0.15, sigma_speed=0.3, speed_min=2.0, speed_max=4.0, lam=0.3, w_dead=10.0,
                  w_clear=5.0, w_progress=0.0, w_lat=0.0, clear_ref=0.5, v_init=3.0)
    op, w_hit = amd.Opponents(mode="cv", radius=0.5), 7.0
    sim.step(np.array([[0.0, 3.0], [0.0, 0.0]]))                          # (a step: the rows are not fresh)
    start = pin_fifo(sim, np.random.default_rng(1))
    nom = np.tile([0.0, 3.0], (1, H, 1))
    words = streams_for(17, [0])
    opp = live_opponents(start[:, :7], A)[:1]
    plain = sim.mppi_rows(mp, start[:1], nom, words)
    seen = sim.mppi_opp_rows(mp, op, w_hit, 0.0, 0.0, start[:1], nom, words, opp)
    assert same_bits(plain["candidates"], seen["candidates"])
    free = seen["opp_raw"][0, :, 1]
    hit = free < H
    assert hit[0] and len(set(free[hit].tolist())) > 1, "the nominal drives straight into the parked car; the others meet it at different actions"
    assert np.array_equal(seen["cost"][0], plain["cost"][0] + w_hit * (float(H) - free)), "the hit candidates do not cost w_hit * (H - free) more"
    assert np.array_equal(seen["cost"][0][~hit], plain["cost"][0][~hit])
    assert seen["actions"][0, 0] != plain["actions"][0, 0], "the planned steer is the blind one"
    # the armed planner on the handle says the same
    sim.set_mppi(mp, np.array([0]), seed=17)
    sim.set_mppi_state(nominal=nom)
    a0 = sim.mppi(np.zeros((2, 2)))
    sim.set_mppi(mp, np.array([0]), seed=17)
    sim.set_mppi_state(nominal=nom)
    sim.set_mppi_opponents(op, w_hit, 0.0, 0.0)
    a1 = sim.mppi(np.zeros((2, 2)))
    assert same_bits(a0[0], plain["actions"][0]) and same_bits(a1[0], seen["actions"][0]) and a0[0, 0] != a1[0, 0]
    sim.close()


# ---- (d) blocks, slots, the scripted step, the env layers ---------------------------------------------------------------------------------
def test_two_env_blocks_against_one(amd):
    """130 envs as blocks of 128 and 2 against a one-block handle: the planner with the term and the rollout with it, bit for bit"""
    E, A, T = 130, 2, 3
    N = E * A
    mp = amd.Mppi(k=8, horizon=4, repeat=2, w_progress=3.0, w_lat=0.2, margin=0.3)
    op = amd.Opponents(mode="track", radius=2.0, max_range=10.0)
    p = amd.Rollout(k=8, horizon=4, repeat=2, channels=ALL10, margin=0.3, traj=True)
    cand = rr.grid_actions(8, 4, False)
    agents = np.arange(1, N, 2)
    res = []
    for groups in (1, 2):
        s = amd.BatchSim(num_envs=E, num_agents=A, step_groups=groups)
        s.set_map_image(*load_map_image("example_map"))
        s.set_noise_rng(4242, 0.01)
        s.set_track(CSV)
        s.reset(bench_start_poses(E, A))
        s.set_mppi(mp, agents, seed=5)
        s.set_mppi_opponents(op, *W)
        d_act, d_info, d_cand = s.device_array((N, 2)), s.device_array((N, 4), np.float32), s.device_array(cand.shape)
        d_act.upload(np.tile([0.05, 3.0], (N, 1)))
        d_info.upload(np.zeros((N, 4), dtype=np.float32))
        d_cand.upload(cand)
        bufs = None
        for t in range(T):
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            s.mppi_device(d_act, d_info)
            bufs = s.rollout_opp_device(p, op, d_cand, *(bufs or ()))
            s.step_device(d_act)                       # a step right behind the calls keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            s.mppi_device(d_act, d_info)
            bufs = s.rollout_opp_device(p, op, d_cand, *bufs)
        s.sync()
        res.append((d_act.download(), d_info.download()) + s.get_mppi_state() + tuple(b.download() for b in bufs) + (s.get("state")["state"],))
        s.close()
    for a, b in zip(*res):
        assert same_bits(a, b), "two blocks against one"
    assert np.all(np.isfinite(res[0][6][..., 0])), "every agent has its opponent in range"


def test_track_mode_on_two_map_slots_one_of_them_derived(amd):
    """slot 0 the example map, slot 1 an obstacle slot derived from it (the same raceline attached): TRACK on both; the device form's
    planner is the unit form of each env's slot; without a track on the derived slot the attach and the call are refused"""
    from f1tenth_gym_amd import _ffi
    E, A = 6, 2
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map_image(*load_map_image("example_map"))
    track = amd.Track.from_csv(CSV)
    sim.set_track(track)
    obstacles = amd.Obstacles.random_on_track(track, 4, 3, lateral=0.5, min_gap=6.0, length=(0.3, 0.5), width=(0.2, 0.4), radius=(0.1, 0.2))
    slot = sim.add_obstacle_map(obstacles)
    env_map = (np.arange(E) % 2) * slot
    sim.set_env_maps(env_map.astype(np.int32))
    sim.reset(bench_start_poses(E, A))
    rng = np.random.default_rng(4)
    for _ in range(10):
        sim.step(np.stack([rng.uniform(-0.1, 0.1, N), rng.uniform(2.0, 4.0, N)], axis=1))
    start = pin_fifo(sim, rng)
    s = mr.settings(k=64, horizon=5, repeat=3, w_progress=3.0, w_lat=0.5, margin=0.3)
    mp, op = mppi_of(amd, s), amd.Opponents(mode="track", radius=2.0)
    sim.set_mppi(mp, None, seed=8)
    sim.set_mppi_opponents(op, *W)
    words0 = sim.get_mppi_state()[1]
    act, info = sim.mppi(np.zeros((N, 2)), info=True)
    nom1, words1 = sim.get_mppi_state()
    count = sim.get("step_count")["step_count"]
    opp = live_opponents(start[:, :7], A)
    for sl in (0, slot):
        idx = np.flatnonzero(np.repeat(env_map, A) == sl)
        unit = sim.mppi_opp_rows(mp, op, W[0], W[1], W[2], start[idx], mp.fresh_nominal(len(idx)), words0[idx], opp[idx], slot=sl, fresh=count[idx])
        for key, mine in (("actions", act), ("info", info), ("nominal", nom1), ("streams", words1)):
            assert same_bits(unit[key], mine[idx]), (sl, key)
        want = np.stack([ref.predict(ref.settings(mode="track", radius=2.0), start[n, 0], start[n, 1], opp[n], 5, 3, track=rr.grid_track("example_map")) for n in idx])
        ro = amd.Rollout(k=64, horizon=5, repeat=3, channels=("alive",), margin=0.3, layout="per_agent")
        pred = sim.rollout_opp_rows(ro, op, start[idx], unit["candidates"], opp[idx], slot=sl)["pred"]
        assert gated(pred, want, (sl, "pred")) < GATE
    sim.close()
    # a second plain map in use without a track: TRACK is refused when attaching and, attached first, at the call
    s2 = amd.BatchSim(num_envs=2, num_agents=2)
    s2.set_map_image(*load_map_image("example_map"))
    s2.set_track(CSV)
    s2.reset(bench_start_poses(2, 2))
    s2.step(np.zeros((4, 2)))
    s2.set_mppi(amd.Mppi(k=4, horizon=3, w_progress=0.0, w_lat=0.0), None, seed=1)
    s2.set_mppi_opponents(op, 1.0, 0.0, 0.0)
    s2.add_map_image(*load_map_image("example_map"))
    s2.set_env_maps(np.array([0, 1], dtype=np.int32))
    d_act = s2.device_array((4, 2))
    assert _ffi.lib().f110_mppi_device(s2._h, d_act.ptr, None) == _ffi.ERR_STATE and "slot 1" in _ffi.last_error(s2._h)
    s2.clear_mppi_opponents()
    sp = op.spec()
    assert _ffi.lib().f110_mppi_set_opponents(s2._h, C.byref(sp), 1.0, 0.0, 0.0) == _ffi.ERR_STATE and "slot 1" in _ffi.last_error(s2._h)
    s2.close()


ENV_KW = dict(num_agents=2, map=map_stem("example_map"), map_ext=".png", seed=31, device_logic=True, auto_reset=True,
              obs_fields=("poses_x", "poses_y", "poses_theta", "linear_vels_x", "collisions"))


def env_planner(amd):
    return amd.Mppi(k=8, horizon=4, repeat=3, w_progress=4.0, margin=0.3, speed_max=5.0)


def env_opponents(amd):
    return dict(opponents=amd.Opponents(mode="track", radius=2.0, max_range=12.0), w_hit=3.0, w_near=2.0, near_ref=3.0)


def run_env(env, E, T=20):
    rng = np.random.default_rng(2)
    out = [env.reset(bench_start_poses(E, 2).reshape(E, 2, 3))[0]]
    out = [{k: np.array(v, copy=True) for k, v in out[0].items() if isinstance(v, np.ndarray)}]
    for _ in range(T):
        act = np.stack([rng.uniform(-0.1, 0.1, (E, 2)), rng.uniform(1.0, 3.0, (E, 2))], axis=-1)
        obs = env.step(act)[0]
        out.append({k: np.array(v, copy=True) for k, v in obs.items() if isinstance(v, np.ndarray)})
    return out


def test_scripted_step_and_env_layers_against_the_hand_fed_loop(amd):
    """F110VecEnv(mppi_opponents=...) — a F110_STEP_SCRIPTED step with the term attached — against a loop written by hand on a plain
    env's handle (the controllers' call, the planner's call with the term, the step), and ShardedVecEnv on two handles of one device
    against the one handle: every observation bit for bit; and the term matters (the blind env's run differs)"""
    from f1tenth_gym_amd.gap_follower import coerce_scripted
    E = 6
    track = amd.Track.from_csv(CSV)
    scripted = {0: amd.GapFollower(), 1: env_planner(amd)}
    env = amd.F110VecEnv(E, scripted=scripted, mppi_opponents=env_opponents(amd), track=track, **ENV_KW)
    assert env.sim.batch.mppi_opponents[0].mode == "track"
    mine = run_env(env, E)
    env.sim.batch.close()
    hand = amd.F110VecEnv(E, track=track, **ENV_KW)
    b = hand.sim.batch
    b.set_controllers(*coerce_scripted({0: amd.GapFollower()}, E, 2))
    b.set_mppi(env_planner(amd), np.arange(E) * 2 + 1, seed=ENV_KW["seed"])
    kw = env_opponents(amd)
    b.set_mppi_opponents(kw["opponents"], kw["w_hit"], kw["w_near"], kw["near_ref"])
    d_act = b.device_array((2 * E, 2))

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
            return hand.step(d_act.download().reshape(E, 2, 2))

    theirs = run_env(ByHand(), E)
    b.close()
    for t, (x, y) in enumerate(zip(mine, theirs)):
        for k in x:
            assert same_bits(x[k], y[k]), (t, k)
    two = amd.ShardedVecEnv(E, devices=[0, 0], scripted=scripted, mppi_opponents=env_opponents(amd), track=track, **ENV_KW)
    sharded = run_env(two, E)
    two.close()
    for t, (x, y) in enumerate(zip(mine, sharded)):
        for k in x:
            assert same_bits(np.asarray(x[k]), np.asarray(y[k])), ("sharded", t, k)
    blind = amd.F110VecEnv(E, scripted=scripted, track=track, **ENV_KW)
    other = run_env(blind, E)
    blind.sim.batch.close()
    assert not same_bits(other[-1]["poses_x"], mine[-1]["poses_x"]), "the term changed nothing: the cars are 10 waypoints apart, within its reach"
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, mppi_opponents=env_opponents(amd), track=track, **ENV_KW)                     # no planner
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, scripted={1: amd.Mppi(w_progress=0.0)}, mppi_opponents=env_opponents(amd), **ENV_KW)   # 'track' without a track


# ---- (e) no side effects ----------------------------------------------------------------------------------------------------------------------
def test_rollout_opp_calls_change_no_step(amd):
    E, A, T = 32, 2, 100
    N = E * A
    rng = np.random.default_rng(5)
    acts = np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)
    p = amd.Rollout(k=8, horizon=3, repeat=2, channels=ALL10, margin=0.3, traj=True)
    op = amd.Opponents(mode="track", radius=0.6)
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
                bufs = s.rollout_opp_device(p, op, d_cand, *(bufs or ()))
        o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
        trk = s.get_track()
        res.append((launches, {k: np.array(v, copy=True) for k, v in list(o.items()) + list(trk.items())}, s.save_state().to_bytes()))
        s.close()
    assert res[0][0] == res[1][0], "f110_step_launches changed"
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k
    assert res[0][2] == res[1][2], "the state blobs differ"


def test_refusals_and_device_allocations(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    L = _ffi.lib()
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    good = amd.Rollout(k=3, horizon=2, repeat=2, channels=("end_x", "alive"), margin=0.2, traj=True)
    op = amd.Opponents(radius=0.5)
    shape, tshape = good.shape(N), good.traj_shape(N)
    d_out, d_traj, d_opp = s.device_array(shape, np.float32), s.device_array(tshape, np.float32), s.device_array((N, 3, 2), np.float32)
    rng = np.random.default_rng(1)
    sent = [rng.normal(size=sh).astype(np.float32) for sh in (shape, tshape, (N, 3, 2))]
    for d, v in zip((d_out, d_traj, d_opp), sent):
        d.upload(v)
    cand = np.tile([0.0, 2.0], (3, 2, 1))
    d_cand = s.device_array(cand.shape)
    d_cand.upload(cand)
    mp = amd.Mppi(k=4, horizon=3, repeat=2, w_progress=0.0, w_lat=0.0)
    poison_a = rng.normal(size=(N, 2))
    d_act = s.device_array((N, 2))
    d_act.upload(poison_a)
    s.set_mppi(mp, None, seed=0)          # (the candidates' jump table stays with the handle from its first arming on)
    s.clear_mppi()
    s.sync()
    base = amd.device_allocs()[0]

    def roll(p_opp=None, **fields):
        sp, osp = good.spec(), op.spec()
        for k, v in fields.items():
            setattr(osp, k, v)
        return L.f110_rollout_opp_device(s._h, C.byref(sp), C.byref(osp), d_cand.ptr, d_out.ptr, d_traj.ptr, d_opp.ptr if p_opp is None else p_opp, None)

    def attach(w=(1.0, 1.0, 1.0), **fields):
        osp = op.spec()
        for k, v in fields.items():
            setattr(osp, k, v)
        return L.f110_mppi_set_opponents(s._h, C.byref(osp), C.c_double(w[0]), C.c_double(w[1]), C.c_double(w[2]))

    bad_spec = [dict(mode=2), dict(mode=-1), dict(radius=0.0), dict(radius=-1.0), dict(radius=INF), dict(radius=NAN), dict(max_range=0.0),
                dict(max_range=-2.0), dict(max_range=NAN)]
    for f in bad_spec:
        assert roll(**f) == _ffi.ERR_INVALID and _ffi.last_error(s._h), f
    assert roll(p_opp=0) == _ffi.ERR_INVALID
    sp = good.spec()
    assert L.f110_rollout_opp_device(s._h, C.byref(sp), None, d_cand.ptr, d_out.ptr, d_traj.ptr, d_opp.ptr, None) == _ffi.ERR_INVALID
    sp.k = 257
    osp = op.spec()
    assert L.f110_rollout_opp_device(s._h, C.byref(sp), C.byref(osp), d_cand.ptr, d_out.ptr, d_traj.ptr, d_opp.ptr, None) == _ffi.ERR_INVALID
    assert roll(mode=_ffi.OPP_TRACK) == _ffi.ERR_STATE and "no track" in _ffi.last_error(s._h)
    assert attach() == _ffi.ERR_STATE and "armed" in _ffi.last_error(s._h)                       # no planner armed
    s.sync()
    for d, v in zip((d_out, d_traj, d_opp), sent):
        assert same_bits(d.download(), v), "a refused call wrote an output"
    assert amd.device_allocs()[0] == base, "a refused call kept device memory"
    # the unit forms: Ao outside 0 .. 31, a null row array, TRACK on a slot without a track
    rows = np.zeros((2, 10))
    rows[:, [0, 1, 4]] = bench_start_poses(2, 1)
    orows = np.zeros((2, 32, 4))
    out, tr = sent[0][:2].copy(), sent[1][:2].copy()
    dp = _ffi.dptr

    def unit(Ao, null_rows=False, mode=_ffi.OPP_CV):
        sp, osp = good.spec(), op.spec()
        osp.mode = mode
        return L.f110_rollout_opp_batch(s._h, C.byref(sp), C.byref(osp), 0, dp(rows), None, dp(cand), None if null_rows else dp(orows), Ao, 2,
                                        out.ctypes.data, None, tr.ctypes.data, None, None, None, None)

    assert unit(32) == _ffi.ERR_INVALID and unit(-1) == _ffi.ERR_INVALID and unit(1, null_rows=True) == _ffi.ERR_INVALID
    assert unit(1, mode=_ffi.OPP_TRACK) == _ffi.ERR_STATE
    assert same_bits(out, sent[0][:2]) and same_bits(tr, sent[1][:2])
    assert unit(31) == _ffi.OK and not same_bits(out, sent[0][:2])
    assert amd.device_allocs()[0] == base, "a unit call kept device memory"
    # the planner: every refusal leaves the planner, its outputs and the allocations alone
    s.set_mppi(mp, np.arange(0, N, 2), seed=1)
    armed = amd.device_allocs()[0]
    before = s.get_mppi_state()
    for f in bad_spec:
        assert attach(**f) == _ffi.ERR_INVALID, f
    for w in ((-1.0, 0.0, 0.0), (0.0, -1.0, 0.0), (INF, 0.0, 0.0), (0.0, NAN, 0.0), (0.0, 0.0, INF), (0.0, 0.0, NAN)):
        assert attach(w=w) == _ffi.ERR_INVALID, w
    assert attach(mode=_ffi.OPP_TRACK) == _ffi.ERR_STATE and "no track" in _ffi.last_error(s._h)
    assert amd.device_allocs()[0] == armed
    for a, b in zip(s.get_mppi_state(), before):
        assert same_bits(a, b)
    assert same_bits(d_act.download(), poison_a)
    # attach, detach, re-arm, disarm: the allocations come and go with them
    s.set_mppi_opponents(op, 1.0, 1.0, 1.0)
    assert amd.device_allocs()[0] == armed + 2 and s.mppi_opponents[1:] == (1.0, 1.0, 1.0)
    s.set_mppi_opponents(dict(mode="cv", radius=0.3), 2.0, 0.0, 0.0)                            # replaces what was attached
    assert amd.device_allocs()[0] == armed + 2
    s.mppi_device(d_act)
    s.clear_mppi_opponents()
    assert amd.device_allocs()[0] == armed and s.mppi_opponents is None
    s.clear_mppi_opponents()                                                                   # (nothing attached: nothing to do)
    s.set_mppi_opponents(op, 1.0, 1.0, 1.0)
    s.set_mppi(mp, np.arange(0, N, 2), seed=1)                                                  # arming anew drops the term
    assert amd.device_allocs()[0] == armed and s.mppi_opponents is None
    s.set_mppi_opponents(op, 1.0, 1.0, 1.0)
    s.clear_mppi()
    assert amd.device_allocs()[0] == base and s.mppi_opponents is None
    with pytest.raises(ValueError):
        s.set_mppi_opponents(op, -1.0, 0.0, 0.0)
    with pytest.raises(ValueError):
        s.rollout_opp_rows(good, op, rows, cand, np.zeros((2, 3, 5)))
    with pytest.raises(ValueError):
        s.rollout_opp_device(good, op, d_cand, opp=s.device_array((N, 3, 3), np.float32))
    # the device form's own buffers stay with the handle until it closes
    assert roll() == _ffi.OK
    s.sync()
    assert not same_bits(d_opp.download(), sent[2])
    s.set_mppi(mp, None, seed=2)
    s.set_mppi_opponents(op, 1.0, 0.0, 0.0)
    start = amd.device_allocs()[0]
    assert start > base
    s.close()
    assert amd.device_allocs()[0] < base


# ---- (f) the example -------------------------------------------------------------------------------------------------------------------------
def test_example_overtake_runs():
    example = os.path.join(os.path.dirname(HERE), "examples", "overtake.py")
    r = subprocess.run([sys.executable, example, "--envs", "8", "--steps", "200"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert not res["nan"] and math.isfinite(res["planner_progress_mean"]) and math.isfinite(res["closest_approach_min"]) and math.isfinite(res["ms_per_step"])
