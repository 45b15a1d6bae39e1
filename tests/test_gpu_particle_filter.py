"""The particle filter on the device (f110_pf_*), held to the Python model tests/particle_filter_ref.py stage by stage,
each stage on the device's own input to it (particle_filter_ref.check_stages): the draws and the streams bit for bit; the ancestors
against the model on the same input weights; the moved particles against the model with the device's ancestors; the expected ranges
against ScanOracle at the device's own moved poses; L against the model on the device's expected ranges (bit for bit: the header
claims it); weights, estimate and info against the model on the device's L.  Everything that is not bitwise is under the project's
gate rel_err < 1e-5, finite exactly where the model is.  Left out: a slot whose t_i lies within 1e-9 * C_{P-1} of a
cumulative boundary, a row whose ESS lies within 1e-9 * P of the threshold; at most 1 % of either (tests/test_particle_filter_host.py
checks on the CPU that the model leaves none out for the seeds used here).

(a) the unit form on both maps, three rows with distinct poses: P in {1, 2, 63, 64, 65} x B' in {1, 7, 64, 65, 128}, P = 1024 at
    B' in {7, 128}, stride 1 and the largest that fits, a fresh row among them, both resampling outcomes.
(b) the device form on 45 envs x 2 cars at P = 65, B' = 7 with every, every other and only the last agent armed: bit for bit the unit
    form on the device's own state, which is held to the model; the other rows' poison untouched.
(c) ten step-and-localise calls with an env re-seated in mid-run, each held against the model on the state fetched before it.
(d) 130 envs as blocks of 128 and 2 with lists straddling the bound against a one-block handle; two map slots, one of them a derived
    obstacle slot; get / put beside a state blob.  (e) dead reckoning.  (f) no effect on the step.  (g) the refusals and the env
    layers.  (h) the example."""
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import particle_filter_ref as ref
import rollout_ref as rr
from _util import bench_start_poses, load_map_image, map_stem
from mppi_ref import two_maps, warm_sim
from particle_filter_ref import STATE_KEYS, check_stages, filter_of, live_rows, localize_and_check, poisoned, same_bits, seed_clouds, streams_for

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def unit_sim(amd):
    sim = two_maps(amd)      # slot 0: example_map, slot 1: berlin
    yield sim
    sim.close()


def report(what, stats):
    print("%s: %d rows (%d left out), %d slots (%d left out), largest rel_err %.3e" % (what, stats["rows"], stats["rows_left_out"], stats["slots"],
                                                                                      stats["slots_left_out"], stats["rel_err"]))
    assert ref.leave_outs_ok(stats), stats


def run_unit(amd, sim, s, inp, slot):
    poses, scans, X, W, last, words, fresh = inp
    return sim.localize_rows(filter_of(amd, s), poses, scans, X, W, last, words, slot=slot, fresh=fresh)


# ---- (a) the unit form against the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("map_name", rr.GRID_MAPS)
@pytest.mark.parametrize("P", ref.UNIT_P)
def test_unit_form_matches_model(amd, unit_sim, map_name, P):
    so, slot = rr.scan_oracle(map_name), rr.GRID_MAPS.index(map_name)
    stats, outcomes = ref.new_stats(), set()
    for q, (Bp, big) in enumerate(itertools.product(ref.UNIT_B, (False, True))):
        s, inp = ref.unit_case(map_name, P, Bp, big, q)
        got = run_unit(amd, unit_sim, s, inp, slot)
        check_stages(s, so, inp, got, (map_name, P, Bp, s["beam_stride"]), stats)
        outcomes |= set(got["info"][[0, 2], 3].tolist())
    assert outcomes == {0.0, 1.0}, "both resampling outcomes"
    report("pf unit grid on %s, P = %d" % (map_name, P), stats)


@pytest.mark.parametrize("map_name", rr.GRID_MAPS)
@pytest.mark.parametrize("Bp", [7, 128])
def test_unit_form_matches_model_at_1024_particles(amd, unit_sim, map_name, Bp):
    so, slot = rr.scan_oracle(map_name), rr.GRID_MAPS.index(map_name)
    stats = ref.new_stats()
    for q, big in enumerate((False, True)):
        s, inp = ref.unit_case(map_name, 1024, Bp, big, q)
        got = run_unit(amd, unit_sim, s, inp, slot)
        check_stages(s, so, inp, got, (map_name, 1024, Bp, s["beam_stride"]), stats)
    report("pf unit form on %s, P = 1024, B' = %d" % (map_name, Bp), stats)


# ---- (b) the device form ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("armed", ["all", "every_other", "last"])
def test_device_form_45_envs_of_2_cars(amd, armed):
    E, A, seed = 45, 2, 321
    N = E * A
    sim, _ = warm_sim(amd, E, A)
    agents = {"all": np.arange(N), "every_other": np.arange(0, N, 2), "last": np.array([N - 1])}[armed]
    s = ref.settings(particles=65, n_beams=7, beam_first=11, beam_stride=150)
    sim.set_particle_filter(filter_of(amd, s), agents, seed=seed)
    assert same_bits(sim.get_pf_state()[3], streams_for(seed, agents))
    seed_clouds(sim, s, agents, 5)
    d_pose, d_info, pa, pi = poisoned(sim, 9)
    stats = ref.new_stats()
    _, info, _ = localize_and_check(amd, sim, s, rr.scan_oracle("example_map"), agents, d_pose, d_info, armed, stats)
    other = np.setdiff1d(np.arange(N), agents)
    assert same_bits(d_pose.download()[other], pa[other]) and same_bits(info[other], pi[other]), "a row of an agent that is not armed was written"
    if armed == "all":
        assert set(info[:, 3].tolist()) == {0.0, 1.0}
    report("pf device form, %s" % armed, stats)
    sim.close()


# ---- (c) ten step-and-localise calls -----------------------------------------------------------------------------------------------------
def test_ten_step_and_localise_calls_with_a_reseat(amd):
    E, A, seed = 4, 2, 77
    N = E * A
    sim, _ = warm_sim(amd, E, A, steps=5)
    sim.set_noise_rng(4242, 0.01)
    s = ref.settings(particles=33, n_beams=9, beam_first=0, beam_stride=130, resample_frac=0.9)
    sim.set_particle_filter(filter_of(amd, s), None, seed=seed)
    so = rr.scan_oracle("example_map")
    first = streams_for(seed, range(N))
    d_pose, d_info, _, _ = poisoned(sim, 3)
    rng = np.random.default_rng(3)
    poses0 = bench_start_poses(E, A)
    stats, fresh_seen, resampled = ref.new_stats(), 0, 0
    for t in range(10):
        if t == 5:   # env 1 is re-seated: its cars' step_count is 0, their rows are fresh
            sim.reset(poses0, np.array([0, 1, 0, 0], dtype=np.uint8))
        else:
            sim.step(np.stack([rng.uniform(-0.1, 0.1, N), rng.uniform(2.0, 4.0, N)], axis=1))
        assert same_bits(sim.get_pf_state()[3], np.stack([ref.words_of(ref.generator(first[n], t << 28)) for n in range(N)])), "call %d: the streams' positions" % t
        pose, info, count = localize_and_check(amd, sim, s, so, np.arange(N), d_pose, d_info, "call %d" % t, stats)
        fresh_seen += int(np.count_nonzero(count == 0))
        resampled += int(info[:, 3].sum())
        if t == 5:
            assert np.all(count[2:4] == 0) and np.all(info[2:4, 3] == 0.0)
        if t >= 6:   # the clouds have found their cars
            assert np.all(info[:, 2] < 0.5), "call %d: err_xy %s" % (t, info[:, 2])
    assert fresh_seen == 2 and resampled > 0, (fresh_seen, resampled)
    report("pf ten calls", stats)
    sim.close()


# ---- (d) blocks, slots and state -------------------------------------------------------------------------------------------------------------
BLOCK_E, BLOCK_A = 130, 2      # group_envs: ceil(130 / 2) = 65 -> 128 envs and 2: agents 0..255 and 256..259


@pytest.fixture(scope="module")
def block_sims(amd):
    """the same 130 x 2 cars on a handle that submits two env blocks and on one that submits one, each with its constant actions"""
    sims = {}
    for groups in (2, 1):
        sim, _ = warm_sim(amd, BLOCK_E, BLOCK_A, steps=5, step_groups=groups)
        d_const = sim.device_array((sim.N, 2))
        d_const.upload(np.tile([0.05, 3.0], (sim.N, 1)))
        sims[groups] = (sim, d_const)
    yield sims
    for sim, _ in sims.values():
        sim.close()


@pytest.mark.parametrize("armed", [[0, 255, 256, 259], [257, 258], [3], [255, 256]], ids=["straddle", "first_empty", "second_empty", "at_the_bound"])
def test_armed_list_across_unequal_env_blocks(amd, block_sims, armed):
    """two device steps back to back, then two calls right behind them: on the two-block handle they ride the blocks (armed indices
    [i0, i0 + count) per block, i0 != 0 or count == 0 in one of them); every output and the filter's state bit for bit the
    one-block handle's"""
    agents = np.array(armed)
    s = ref.settings(particles=65, n_beams=7, beam_first=5, beam_stride=170)
    res = {}
    for groups in (2, 1):
        sim, d_const = block_sims[groups]
        sim.set_particle_filter(filter_of(amd, s), agents, seed=40)
        seed_clouds(sim, s, agents, 8)
        d_pose, d_info, pa, pi = poisoned(sim, 11)
        sim.step_device(d_const)
        sim.step_device(d_const)
        sim.localize_device(d_pose, d_info)
        sim.step_device(d_const)
        assert sim.step_groups()[2] == groups, "the steps went out as %d block(s)" % sim.step_groups()[2]
        sim.localize_device(d_pose, d_info)
        pose, info = d_pose.download(), d_info.download()
        other = np.setdiff1d(np.arange(sim.N), agents)
        assert same_bits(pose[other], pa[other]) and same_bits(info[other], pi[other]), "%d block(s): a row of an agent that is not armed was written" % groups
        res[groups] = (pose, info) + sim.get_pf_state() + (sim.get("state")["state"],)
        d_pose.free()
        d_info.free()
    for a, b in zip(res[2], res[1]):
        assert same_bits(a, b), "two blocks against one"
    assert np.all(res[2][1][agents, 2] < 1.0)


def test_two_map_slots_one_of_them_with_obstacles(amd):
    """even envs on example_map, odd envs on a slot derived from it with a disc ahead of every car: each slot's rows against the model
    on that slot's own table, and bit for bit the unit form of the slot"""
    E, A = 6, 1
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    img, res, origin = load_map_image("example_map")
    sim.set_map_image(img, res, origin)
    poses = bench_start_poses(E, A)
    ahead = poses[:, :2] + 2.5 * np.column_stack([np.cos(poses[:, 2]), np.sin(poses[:, 2])])
    slot = sim.add_obstacle_map(amd.Obstacles.discs(ahead, np.full(E, 0.25)))
    env_map = np.arange(E) % 2 * slot
    sim.set_env_maps(env_map)
    sim.reset(poses)
    sim.step(np.tile([0.0, 1.0], (E, 1)))
    s = ref.settings(particles=64, n_beams=64, beam_first=8, beam_stride=16, resample_frac=2.0)
    sim.set_particle_filter(filter_of(amd, s), None, seed=12)
    seed_clouds(sim, s, np.arange(E), 21)
    d_pose, d_info, _, _ = poisoned(sim, 2)
    poses_l, scans, count, (X, W, last, words) = live_rows(sim, np.arange(E))
    sim.localize_device(d_pose, d_info)
    pose, info = d_pose.download(), d_info.download()
    after = dict(zip(STATE_KEYS, sim.get_pf_state()))
    stats = ref.new_stats()
    expect = {}
    for sl in (0, slot):
        idx = np.flatnonzero(env_map == sl)
        so = ref.orc.ScanOracle(ref.NUM_BEAMS, ref.FOV)
        so.set_map_dt(sim.get_map_dt(sl), res, origin)
        unit = sim.localize_rows(filter_of(amd, s), poses_l[idx], scans[idx], X[idx], W[idx], last[idx], words[idx], slot=sl, fresh=count[idx])
        assert same_bits(pose[idx], unit["pose"]) and same_bits(info[idx], unit["info"]), sl
        for key in STATE_KEYS:
            assert same_bits(after[key][idx], unit[key]), (sl, key)
        check_stages(s, so, (poses_l[idx], scans[idx], X[idx], W[idx], last[idx], words[idx], count[idx]), unit, "slot %d" % sl, stats)
        expect[sl] = unit["expected"]
    # the obstacle shows in the expected ranges of the derived slot: the same particles on the base slot see further somewhere
    base_view = sim.localize_rows(filter_of(amd, s), poses_l[1::2], scans[1::2], X[1::2], W[1::2], last[1::2], words[1::2], slot=0, fresh=count[1::2])["expected"]
    assert np.any(base_view > expect[slot] + 0.1)
    report("pf two slots", stats)
    sim.close()


def test_get_put_and_a_state_blob_reproduce_the_next_estimate(amd):
    E, A = 8, 2
    N = E * A
    sim, _ = warm_sim(amd, E, A, steps=6)
    sim.set_noise_rng(99, 0.01)
    pf = amd.ParticleFilter(particles=48, n_beams=12, beam_stride=90, resample_frac=0.7)
    sim.set_particle_filter(pf, np.arange(0, N, 3), seed=4)
    d_act, d_pose = sim.device_array((N, 2)), sim.device_array((N, 3))
    d_act.upload(np.tile([0.03, 2.0], (N, 1)))
    d_pose.upload(np.zeros((N, 3)))
    for _ in range(3):
        sim.step_device(d_act)
        sim.localize_device(d_pose)
    blob, state = sim.save_state(), sim.get_pf_state()
    seq = []
    for _ in range(3):
        sim.step_device(d_act)
        sim.localize_device(d_pose)
        seq.append(d_pose.download())
    after = sim.get_pf_state()
    assert not any(same_bits(a, b) for a, b in zip(after, state))
    sim.load_state(blob)                            # the blob does not hold the filter: its state is still the later one
    for a, b in zip(sim.get_pf_state(), after):
        assert same_bits(a, b)
    sim.set_pf_state(*state)
    for t in range(3):
        sim.step_device(d_act)
        sim.localize_device(d_pose)
        assert same_bits(d_pose.download(), seq[t]), "call %d after the restore" % t
    for a, b in zip(sim.get_pf_state(), after):
        assert same_bits(a, b)
    sim.close()


# ---- (e) dead reckoning ------------------------------------------------------------------------------------------------------------------------
def test_dead_reckoning_follows_the_true_pose(amd):
    """every sigma and init sigma 0, no resampling: the odometry delta is the filter's only input to the motion, and the estimate stays
    on the true pose for 50 steps under gap followers (the first call, right after the reset, draws the fresh cloud)"""
    E, A = 8, 2
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map_image(*load_map_image("example_map"))
    sim.set_noise_rng(7, 0.01)
    sim.set_controllers(np.zeros(N, dtype=np.int32), [amd.GapFollower()])
    pf = amd.ParticleFilter(particles=16, n_beams=8, beam_stride=100, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, init_x=0.0, init_y=0.0, init_theta=0.0,
                            resample_frac=0.0)
    sim.set_particle_filter(pf, None, seed=1)
    sim.reset(bench_start_poses(E, A))
    d_act, d_pose, d_info = sim.device_array((N, 2)), sim.device_array((N, 3)), sim.device_array((N, 4), np.float32)
    d_act.upload(np.zeros((N, 2)))
    sim.localize_device(d_pose, d_info)
    assert np.all(sim.get("step_count")["step_count"] == 0) and np.all(d_info.download()[:, 3] == 0.0)
    worst, moved = 0.0, 0.0
    start = None
    for t in range(50):
        sim.step_device(d_act)
        sim.follow_gap_device(d_act)
        sim.localize_device(d_pose, d_info)
        true, est = sim.get("agent_poses")["agent_poses"], d_pose.download()
        start = true.copy() if start is None else start
        err = np.abs(est - true)
        err[:, 2] = np.abs(np.remainder(err[:, 2] + np.pi, 2.0 * np.pi) - np.pi)
        worst = max(worst, float(err.max()))
        assert err.max() < 1e-9, "step %d: |estimate - true pose| = %.3e" % (t, err.max())
        moved = max(moved, float(np.abs(true[:, :2] - start[:, :2]).max()))
    print("dead reckoning: worst |estimate - true pose| %.3e over 50 steps, the cars moved up to %.2f m" % (worst, moved))
    assert moved > 0.5
    sim.close()


# ---- (f) no effect on the step -----------------------------------------------------------------------------------------------------------
def test_filter_calls_change_no_step(amd):
    E, A, T = 32, 2, 100
    N = E * A
    rng = np.random.default_rng(5)
    acts = np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)
    pf = amd.ParticleFilter(particles=32, n_beams=8, beam_stride=100)
    res = []
    for use in (False, True):
        s = amd.BatchSim(num_envs=E, num_agents=A)
        s.set_map_image(*load_map_image("example_map"))
        s.set_noise_rng(4242, 0.01)
        start = bench_start_poses(E, A)
        s.reset(start)
        d_start = s.device_array((N, 3))
        d_start.upload(start)
        s.set_auto_reseat(d_start, 0)
        d_act, d_pose, d_info = s.device_array((N, 2)), s.device_array((N, 3)), s.device_array((N, 4), np.float32)
        if use:
            s.set_particle_filter(pf, None, seed=1)
        launches = []
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            launches.append(s.step_launches())
            if use:
                s.localize_device(d_pose, d_info)
        o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
        res.append((launches, {k: np.array(v, copy=True) for k, v in o.items()}, s.save_state().to_bytes()))
        if use:
            assert np.all(np.isfinite(d_pose.download())) and np.all(np.isfinite(d_info.download()))
        s.close()
    assert res[0][0] == res[1][0], "f110_step_launches changed"
    for k in res[0][1]:
        assert np.array_equal(res[0][1][k], res[1][1][k], equal_nan=True), k
    assert res[0][2] == res[1][2], "the state blobs differ"


# ---- (g) refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_and_filter_alone(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    L = _ffi.lib()
    u64 = _ffi._u64p
    good = amd.ParticleFilter(particles=8, n_beams=4, beam_first=1, beam_stride=300)
    agents = np.arange(0, N, 2, dtype=np.int32)
    words = np.ascontiguousarray(streams_for(1, agents))
    d_pose, d_info, pa, pi = poisoned(s, 1)
    assert L.f110_pf_device(s._h, d_pose.ptr, d_info.ptr) == _ffi.ERR_STATE and "armed" in _ffi.last_error(s._h)      # nothing armed
    assert L.f110_pf_get(s._h, None, None, None, None) == _ffi.ERR_STATE and L.f110_pf_put(s._h, None, None, None, None) == _ffi.ERR_STATE
    s.set_particle_filter(good, agents, seed=1)
    seed_clouds(s, ref.settings(particles=8), agents, 3)
    before = s.get_pf_state()

    def arm(ag=agents, m=None, w=words, **fields):
        sp = good.spec()
        for k, v in fields.items():
            setattr(sp, k, v)
        ag = np.ascontiguousarray(ag, dtype=np.int32)
        return L.f110_pf_set(s._h, C.byref(sp), _ffi.i32ptr(ag), len(ag) if m is None else m, w.ctypes.data_as(u64))

    inf, nan = float("inf"), float("nan")
    bad = [dict(particles=0), dict(particles=1025), dict(particles=-1), dict(n_beams=0), dict(n_beams=129), dict(beam_first=-1), dict(beam_stride=0),
           dict(beam_first=180), dict(beam_stride=360), dict(n_beams=128, beam_stride=9),
           dict(sigma_x=-1.0), dict(sigma_y=-0.1), dict(sigma_theta=-0.1), dict(init_x=-1.0), dict(init_y=-1.0), dict(init_theta=-1.0),
           dict(sigma_x=inf), dict(sigma_theta=nan), dict(init_y=inf), dict(init_x=nan),
           dict(sigma_hit=0.0), dict(sigma_hit=-1.0), dict(sigma_hit=inf), dict(sigma_hit=nan), dict(clip=0.0), dict(clip=-inf), dict(clip=nan),
           dict(squash=0.0), dict(squash=inf), dict(squash=nan), dict(resample_frac=-0.5), dict(resample_frac=inf), dict(resample_frac=nan),
           dict(ag=[3, 3]), dict(ag=[5, 2]), dict(ag=[-1, 2]), dict(ag=[0, N]), dict(m=0), dict(m=N + 1)]
    for f in bad:
        assert arm(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
    sp = good.spec()
    assert L.f110_pf_set(s._h, C.byref(sp), None, 3, words.ctypes.data_as(u64)) == _ffi.ERR_INVALID
    assert L.f110_pf_set(s._h, C.byref(sp), _ffi.i32ptr(agents), len(agents), None) == _ffi.ERR_INVALID
    assert L.f110_pf_device(s._h, None, None) == _ffi.ERR_INVALID
    big = amd.BatchSim(num_envs=1024, num_agents=16, num_beams=128)          # M * P * B' = 2^14 * 2^10 * 2^7 = 2^31
    sp_big = amd.ParticleFilter(particles=1024, n_beams=128, beam_stride=1).spec()
    ag_big, w_big = np.arange(big.N, dtype=np.int32), np.zeros((big.N, 4), dtype=np.uint64)
    assert L.f110_pf_set(big._h, C.byref(sp_big), _ffi.i32ptr(ag_big), big.N, w_big.ctypes.data_as(u64)) == _ffi.ERR_INVALID and "31 bits" in _ffi.last_error(big._h)
    big.close()
    # clip = +inf is a setting, not a refusal
    assert arm(clip=inf) == _ffi.OK
    s.set_particle_filter(good, agents, seed=1)
    s.set_pf_state(*before)
    # put: a particle that is not finite, a weight that is negative or not finite, a row that sums to nothing
    for key, value, where in ((0, nan, (0, 0, 0)), (0, inf, (1, 2, 1)), (1, -0.1, (0, 1)), (1, nan, (2, 0)), (1, inf, (3, 7))):
        arrs = [a.copy() for a in before]
        arrs[key][where] = value
        with pytest.raises(ValueError):
            s.set_pf_state(*arrs)
    zero = before[1].copy()
    zero[1] = 0.0
    with pytest.raises(ValueError):
        s.set_pf_state(weights=zero)
    with pytest.raises(ValueError):
        s.set_pf_state(particles=np.zeros((3, 8, 3)))
    with pytest.raises(ValueError):
        s.localize_device(d_pose, s.device_array((N, 3), np.float32))
    with pytest.raises(ValueError):
        s.localize_device(s.device_array((N, 2)), d_info)
    # every refusal so far changed nothing: the filter is the one armed first, the outputs hold their pattern
    for a, b in zip(s.get_pf_state(), before):
        assert same_bits(a, b)
    s.sync()
    assert same_bits(d_pose.download(), pa) and same_bits(d_info.download(), pi), "a refused call wrote an output"
    # the unit form refuses the same way and leaves the caller's arrays alone
    poses = np.ascontiguousarray(bench_start_poses(4, 1))
    scans = np.ones((4, s.B))
    X, W = ref.cloud_around(poses, 8, 4)
    last, w4 = poses.copy(), np.ascontiguousarray(streams_for(2, range(4)))
    keep = [a.copy() for a in (X, W, last, w4)]
    pose = pa[:4].copy()

    def unit(sp, slot=0, m=4, particles=X, weights=W):
        return L.f110_pf_batch(s._h, C.byref(sp), slot, _ffi.dptr(poses), _ffi.dptr(scans), None, m, _ffi.dptr(particles), _ffi.dptr(weights), _ffi.dptr(last),
                               w4.ctypes.data_as(u64), _ffi.dptr(pose), None, None, None, None, None)

    sp = good.spec()
    sp.particles = 1025
    assert unit(sp) == _ffi.ERR_INVALID
    assert unit(good.spec(), slot=1) == _ffi.ERR_INVALID and unit(good.spec(), slot=-1) == _ffi.ERR_INVALID and unit(good.spec(), m=-1) == _ffi.ERR_INVALID
    wild = X.copy()
    wild[1, 1, 0] = nan
    assert unit(good.spec(), particles=wild) == _ffi.ERR_INVALID
    neg = W.copy()
    neg[2, 3] = -1e-3
    assert unit(good.spec(), weights=neg) == _ffi.ERR_INVALID
    for a, b in zip((X, W, last, w4), keep):
        assert same_bits(a, b)
    assert same_bits(pose, pa[:4])
    assert unit(good.spec()) == _ffi.OK and not same_bits(pose, pa[:4]) and not same_bits(w4, keep[3])
    for a, b in zip(s.get_pf_state(), before):                     # the unit form does not touch the armed filter
        assert same_bits(a, b)
    # disarmed: the call is refused again; and without a map
    s.clear_particle_filter()
    assert L.f110_pf_device(s._h, d_pose.ptr, d_info.ptr) == _ffi.ERR_STATE
    nomap = amd.BatchSim(num_envs=1, num_agents=1)
    nomap.set_particle_filter(good, None, seed=0)
    tiny = nomap.device_array((1, 3))
    assert L.f110_pf_device(nomap._h, tiny.ptr, None) == _ffi.ERR_STATE and "map" in _ffi.last_error(nomap._h)
    nomap.close()
    s.close()


# ---- (g) the env layers ---------------------------------------------------------------------------------------------------------------------
ENV_KW = dict(num_agents=2, map=map_stem("example_map"), map_ext=".png", seed=31, device_logic=True, auto_reset=True,
              obs_fields=("poses_x", "poses_y", "poses_theta", "linear_vels_x", "collisions"))


def env_filter(amd):
    return amd.ParticleFilter(particles=40, n_beams=10, beam_stride=100, resample_frac=0.6)


def run_env(env, E, T=20):
    rng = np.random.default_rng(2)
    out = []
    obs = env.reset(bench_start_poses(E, 2).reshape(E, 2, 3))[0]
    for t in range(T + 1):
        out.append({k: np.array(v, copy=True) for k, v in obs.items() if isinstance(v, np.ndarray)})
        act = np.stack([rng.uniform(-0.1, 0.1, (E, 2)), rng.uniform(4.0, 9.0, (E, 2))], axis=-1)     # fast enough for a crash and a re-seat
        obs = env.step(act)[0]
    return out


def test_vec_env_filter_is_the_hand_fed_loop(amd):
    E = 6
    env = amd.F110VecEnv(E, particle_filter={0: env_filter(amd)}, **ENV_KW)
    mine = run_env(env, E, T=60)
    env.sim.batch.close()
    # by hand: the filter armed on the handle of an env without one, called after every step
    hand = amd.F110VecEnv(E, **ENV_KW)
    b = hand.sim.batch
    b.set_particle_filter(env_filter(amd), np.arange(E) * 2, seed=ENV_KW["seed"])
    d_pose, d_info = b.device_array((2 * E, 3)), b.device_array((2 * E, 4), np.float32)
    d_pose.upload(np.full((2 * E, 3), np.nan))
    d_info.upload(np.full((2 * E, 4), np.nan, dtype=np.float32))

    class ByHand(object):
        def _with(self, ret):
            b.localize_device(d_pose, d_info)
            obs = dict(ret[0])
            obs["pose_estimate"], obs["pf_info"] = d_pose.download().reshape(E, 2, 3), d_info.download().reshape(E, 2, 4)
            return (obs,) + tuple(ret[1:])

        def reset(self, poses):
            return self._with(hand.reset(poses))

        def step(self, act):
            return self._with(hand.step(act))

    theirs = run_env(ByHand(), E, T=60)
    b.close()
    assert "pose_estimate" in mine[0] and mine[0]["pose_estimate"].shape == (E, 2, 3) and mine[0]["pf_info"].shape == (E, 2, 4)
    for t, (x, y) in enumerate(zip(mine, theirs)):
        assert set(x) == set(y)
        for k in x:
            assert same_bits(x[k], y[k]), (t, k)
    last = mine[-1]
    assert np.all(np.isnan(last["pose_estimate"][:, 1])) and np.all(np.isnan(last["pf_info"][:, 1])) and np.all(np.isfinite(last["pose_estimate"][:, 0]))
    assert np.all(last["pf_info"][:, 0, 2] < 0.5), "the clouds lost their cars: err_xy %s" % (last["pf_info"][:, 0, 2],)
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, particle_filter={0: env_filter(amd)}, **dict(ENV_KW, device_logic=False))
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, particle_filter={0: env_filter(amd), 1: env_filter(amd)}, **ENV_KW)
    with pytest.raises(ValueError):
        amd.F110VecEnv(2, particle_filter={2: env_filter(amd)}, **ENV_KW)


def test_sharded_env_draws_the_numbers_of_one_handle(amd):
    E = 6
    one = amd.F110VecEnv(E, particle_filter={1: env_filter(amd)}, **ENV_KW)
    a = run_env(one, E, T=12)
    one.sim.batch.close()
    two = amd.ShardedVecEnv(E, devices=[0, 0], particle_filter={1: env_filter(amd)}, **ENV_KW)
    b = run_env(two, E, T=12)
    two.close()
    for t, (x, y) in enumerate(zip(a, b)):
        assert set(x) == set(y)
        for k in x:
            assert same_bits(np.asarray(x[k]), np.asarray(y[k])), (t, k)
    assert np.all(np.isfinite(a[-1]["pose_estimate"][:, 1]))


# ---- (h) the example ------------------------------------------------------------------------------------------------------------------------
def test_example_localises_and_drives():
    example = os.path.join(os.path.dirname(HERE), "examples", "particle_filter.py")
    r = subprocess.run([sys.executable, example, "--envs", "8", "--steps", "300"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["finite"], res
