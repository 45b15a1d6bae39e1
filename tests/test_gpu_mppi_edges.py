"""The MPPI planner's kernels (k_mppi_roll, k_mppi_track, k_mppi_update) where tests/test_gpu_mppi.py does not reach:
the model, the gate and the leave-out rule are that file's (tests/mppi_ref.py: check_rows; rel_err < 1e-5, at most 1 % of a test's
rows left out, the candidates V and the stream words bit for bit).

(a) every lane grouping of k_mppi_update — GS = 16, 32, 64, 128, set by K and by 2 H, K = 2 H = GS, K above GS with a short last
    stride, an idle group beside a live one, both limits (K = 256 with H = 64; repeat = 16) — in the unit form against the model,
    on both grid maps under both integrators (mppi_ref.LANE_CASES).
(b) one case per GS through the device form: a strict subset armed whose count leaves idle groups, the other rows poisoned.
(c) the armed list cut at the bounds of two unequal env blocks (128 and 2 envs of 2 cars), K = 64 (k_mppi_roll<UNI> with i0 != 0)
    and K = 65: lists that straddle the bound, that leave the first or the second block empty, against the model and against a
    one-block handle.
(d) the cases tests/test_mppi_host.py works out by hand, on the device, in a workgroup shared with healthy rows: every candidate
    dead, a NaN pose, a cold and a hot temperature, both clamps binding, the ziggurat's wedge and tail.
(e) re-arming one handle with other shapes (d_end comes and goes), with and without host synchronisation between the calls."""
import math

import numpy as np
import pytest

import mppi_ref as ref
import rollout_ref as rr
from mppi_ref import check_rows, mppi_of, nominal_for, same_bits, streams_for, two_maps, warm_sim

pytestmark = pytest.mark.gpu

INF = float("inf")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def new_stats():
    return {"rows": 0, "left_out": 0, "rel_err": 0.0}


def report(what, stats):
    print("%s: %d rows, %d left out, largest rel_err %.3e" % (what, stats["rows"], stats["left_out"], stats["rel_err"]))
    assert stats["left_out"] * 100 <= stats["rows"], (what, stats)


def poisoned(sim, seed):
    """(d_actions, d_info, their host patterns): output buffers that hold a pattern no call writes"""
    rng = np.random.default_rng(seed)
    pa, pi = rng.normal(size=(sim.N, 2)), rng.normal(size=(sim.N, 4)).astype(np.float32)
    d_act, d_info = sim.device_array((sim.N, 2)), sim.device_array((sim.N, 4), np.float32)
    d_act.upload(pa)
    d_info.upload(pi)
    return d_act, d_info, pa, pi


# ---- (a) every lane grouping, unit form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("integrator", [1, 2])
@pytest.mark.parametrize("grid_map", rr.GRID_MAPS)
def test_unit_form_at_every_lane_grouping(amd, grid_map, integrator):
    sim = two_maps(amd, integrator=integrator)
    so, track, slot = rr.scan_oracle(grid_map), rr.grid_track(grid_map), rr.GRID_MAPS.index(grid_map)
    stats = new_stats()
    for q, (K, H, M, GS, per, repeat) in enumerate(ref.LANE_CASES):
        assert ref.group_lanes(K, H) == GS and 256 // GS == per, "the table is stale: mppi_group_lanes(%d, %d)" % (K, H)
        s, start, params, nom, words, fresh = ref.lane_inputs(grid_map, integrator, q)
        assert start.shape[0] == M and (s["k"], s["horizon"], s["repeat"]) == (K, H, repeat)
        want = ref.plan(s, so, start, params, nom, words, integrator, fresh, track)
        got = sim.mppi_rows(mppi_of(amd, s), start, nom, words, slot=slot, params=params, fresh=fresh)
        check_rows(s, want, got, (grid_map, integrator, K, H, "GS %d" % GS), stats)
    report("lane groupings on %s, integrator %d" % (grid_map, integrator), stats)
    sim.close()


# ---- (b) the groupings through the device form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,H", [(17, 2), (5, 9), (33, 3), (3, 33)])
def test_device_form_at_every_group_size(amd, K, H):
    """12 envs x 2 cars; per + 3 of the 24 agents are armed (per = 256 / GS agents fill a workgroup): the last workgroup holds three
    live groups (per = 2: one) beside idle ones, which shadow the last agent; a write of theirs lands in a poisoned row or changes an
    armed one"""
    E, A, seed = 12, 2, 500 + K
    N = E * A
    per = 256 // ref.group_lanes(K, H)
    count = per + 3
    assert count < N and count % per != 0
    sim, start = warm_sim(amd, E, A)
    agents = np.sort(np.random.default_rng(K).choice(N, count, replace=False))
    s = ref.settings(k=K, horizon=H, repeat=2, w_progress=3.0, w_lat=0.5, margin=0.25)
    sim.set_mppi(mppi_of(amd, s), agents, seed=seed)
    d_act, d_info, poison_a, poison_i = poisoned(sim, 9)
    sim.mppi_device(d_act, d_info)
    act, info = d_act.download(), d_info.download()
    nom, words = sim.get_mppi_state()
    other = np.setdiff1d(np.arange(N), agents)
    assert same_bits(act[other], poison_a[other]) and same_bits(info[other], poison_i[other]), "a row of an agent that is not armed was written"
    params = np.tile(rr.orc.params_vec(), (count, 1))
    want = ref.plan(s, rr.scan_oracle("example_map"), start[agents], params, mppi_of(amd, s).fresh_nominal(count), streams_for(seed, agents), 1,
                    sim.get("step_count")["step_count"][agents], rr.grid_track("example_map"))
    stats = new_stats()
    check_rows(s, want, dict(actions=act[agents], info=info[agents], nominal=nom, streams=words), (K, H), stats)
    report("device form K = %d, H = %d (%d agents a workgroup, %d armed)" % (K, H, per, count), stats)
    sim.close()


# ---- (c) the armed list across unequal env blocks ------------------------------------------------------------------------------------------
BLOCK_E, BLOCK_A, BLOCK_STEER = 130, 2, 0.05      # group_envs: ceil(130 / 2) = 65 -> 128 envs and 2: agents 0..255 and 256..259


@pytest.fixture(scope="module")
def block_sims(amd):
    """the same 130 x 2 cars on a handle that submits two env blocks and on one that submits one, each with its constant actions"""
    sims = {}
    for groups in (2, 1):
        sim, _ = warm_sim(amd, BLOCK_E, BLOCK_A, steps=5, step_groups=groups)
        d_const = sim.device_array((sim.N, 2))
        d_const.upload(np.tile([BLOCK_STEER, 3.0], (sim.N, 1)))
        sims[groups] = (sim, d_const)
    yield sims
    for sim, _ in sims.values():
        sim.close()


@pytest.mark.parametrize("armed", [[0, 255, 256, 259], [257, 258], [3], [255, 256]], ids=["straddle", "first_empty", "second_empty", "at_the_bound"])
@pytest.mark.parametrize("K", [64, 65])
def test_armed_list_across_unequal_env_blocks(amd, block_sims, K, armed):
    """two device steps back to back, then the call right behind them: on the two-block handle it rides the blocks (armed indices
    [i0, i0 + count) per block, i0 != 0 or count == 0 in one of them).  The planner changes no state, so the state read back after the
    call is the one it planned from; two steps with one steering command leave the FIFO full of it."""
    agents = np.array(armed)
    s = ref.settings(k=K, horizon=5, repeat=2, w_progress=3.0, w_lat=0.5, margin=0.25)
    seed = 40 + K
    res = {}
    for groups in (2, 1):
        sim, d_const = block_sims[groups]
        N = sim.N
        sim.set_mppi(mppi_of(amd, s), agents, seed=seed)
        d_act, d_info, poison_a, poison_i = poisoned(sim, 11)
        sim.step_device(d_const)
        sim.step_device(d_const)
        sim.mppi_device(d_act, d_info)
        assert sim.step_groups()[2] == groups, "the steps went out as %d block(s)" % sim.step_groups()[2]
        act, info = d_act.download(), d_info.download()
        nom, words = sim.get_mppi_state()
        o = sim.get("state", "step_count")
        other = np.setdiff1d(np.arange(N), agents)
        assert same_bits(act[other], poison_a[other]) and same_bits(info[other], poison_i[other]), "%d block(s): a row of an agent that is not armed was written" % groups
        res[groups] = (act, info, nom, words, o["state"])
        d_act.free()
        d_info.free()
    for a, b in zip(res[2], res[1]):
        assert same_bits(a, b), "two blocks against one"
    act, info, nom, words, state = res[2]
    m = len(agents)
    start = np.concatenate([state, np.full((state.shape[0], 2), BLOCK_STEER), np.full((state.shape[0], 1), 2.0)], axis=1)[agents]
    want = ref.plan(s, rr.scan_oracle("example_map"), start, np.tile(rr.orc.params_vec(), (m, 1)), mppi_of(amd, s).fresh_nominal(m), streams_for(seed, agents), 1,
                    None, rr.grid_track("example_map"))
    stats = new_stats()
    check_rows(s, want, dict(actions=act[agents], info=info[agents], nominal=nom, streams=words), (K, armed), stats)
    report("blocks of 128 and 2 envs, K = %d, armed %s" % (K, armed), stats)


# ---- (d) the hand cases on the device -------------------------------------------------------------------------------------------------------
SPECIAL = 2      # the special row, between healthy ones: its LDS slice and its lanes lie inside a workgroup that serves all six


def six_rows(map_name="example_map"):
    start, params = rr.grid_rows(map_name)
    return start.copy(), params.copy()


def test_hand_every_candidate_dead_at_its_first_step(amd):
    """a start far outside the table reads the out-of-bounds value at every step; with the margin 1.0 above it (not AT it: that is a
    tie at the margin) the candidates die at their first step: one cost, weights of exactly 1.0, the plain ascending mean.  On berlin
    (out-of-bounds value 0.0, margin 1.0) the healthy rows beside it keep some candidates alive and lose others."""
    so = rr.scan_oracle("berlin")
    oob = float(so.dt[-1, -1])
    K, H, repeat = 6, 3, 2
    s = ref.settings(k=K, horizon=H, repeat=repeat, margin=oob + 1.0, clear_ref=0.0)
    start, params = six_rows("berlin")
    start[SPECIAL, [0, 1, 4]] = [-500.0, 900.0, 0.3]
    nom, words = nominal_for(s, 6), streams_for(11, range(6))
    sim = two_maps(amd)
    got = sim.mppi_rows(mppi_of(amd, s), start, nom, words, slot=1, params=params)
    want = ref.plan(s, so, start, params, nom, words, 1)
    stats = new_stats()
    check_rows(s, want, got, "every candidate dead", stats)
    report("every candidate dead", stats)
    assert stats["left_out"] == 0
    c = s["w_dead"] * float(H * repeat)
    assert np.all(got["cost"][SPECIAL] == c) and np.all(got["weight"][SPECIAL] == 1.0)
    assert got["info"][SPECIAL].tolist() == [np.float32(c), np.float32(c), float(K), 0.0]
    mean = np.zeros((H, 2))
    for k in range(K):
        mean = mean + got["candidates"][SPECIAL, k]
    mean = mean / float(K)
    assert same_bits(got["actions"][SPECIAL], mean[0]), "the action is not the plain ascending mean"
    assert same_bits(got["nominal"][SPECIAL], ref.shifted(s, mean))
    healthy = np.delete(np.arange(6), SPECIAL)
    assert len(np.unique(want["cost"][healthy])) > 1, "the healthy rows all cost what the dead row costs: they test no slice"
    sim.close()


def test_hand_a_nan_pose_keeps_the_nominal(amd):
    """a NaN x reads the out-of-bounds value (sample_distance's `inside` is false for it) and projects to a NaN arc length through
    roll_search16's no-winner path: every cost NaN -> +inf, w = (1, 0, 0), the nominal stays.  K = 3: the NaN row's 16-lane
    projection groups share a wave with row 1's and row 3's.  The model cannot take the NaN row (its clearance lookup raises): it is
    evaluated on the five healthy rows."""
    so, track = rr.scan_oracle("example_map"), rr.grid_track("example_map")
    s = ref.settings(k=3, horizon=3, repeat=1, shift=0, w_progress=2.0)
    start, params = six_rows()
    start[SPECIAL, 0] = float("nan")
    nom, words = nominal_for(s, 6), streams_for(12, range(6))
    sim = two_maps(amd)
    got = sim.mppi_rows(mppi_of(amd, s), start, nom, words, slot=0, params=params)
    g = got
    assert np.all(g["cost"][SPECIAL] == INF) and g["weight"][SPECIAL].tolist() == [1.0, 0.0, 0.0]
    assert same_bits(g["nominal"][SPECIAL], nom[SPECIAL]) and same_bits(g["actions"][SPECIAL], nom[SPECIAL, 0])
    assert g["info"][SPECIAL].tolist() == [INF, INF, 1.0, 0.0]
    assert same_bits(g["streams"][SPECIAL], ref.words_of(ref.generator(words[SPECIAL], 1 << 28)))
    assert same_bits(g["candidates"][SPECIAL], ref.candidates(s, nom[SPECIAL], words[SPECIAL]))
    healthy = np.delete(np.arange(6), SPECIAL)
    want = ref.plan(s, so, start[healthy], params[healthy], nom[healthy], words[healthy], 1, None, track)
    stats = new_stats()
    check_rows(s, want, {k: v[healthy] for k, v in got.items()}, "beside a NaN pose", stats)
    report("beside a NaN pose", stats)
    assert stats["left_out"] == 0
    sim.close()


@pytest.mark.parametrize("lam", [1e-3, 1e6], ids=["cold", "hot"])
def test_hand_cold_and_hot_temperatures(amd, lam):
    """the device's exp at both ends.  Against the model under the gate, and — what isolates the exp from the 1 / lambda amplification
    of the costs' rounding — the device's weights against float64 exp(-(c - min c) / lambda) of the device's own costs."""
    so, track = rr.scan_oracle("example_map"), rr.grid_track("example_map")
    s = ref.settings(k=16, horizon=5, repeat=3, lam=lam, w_progress=10.0)
    start, params = six_rows()
    nom, words = nominal_for(ref.settings(horizon=5), 6), streams_for(13, range(6))
    sim = two_maps(amd)
    got = sim.mppi_rows(mppi_of(amd, s), start, nom, words, slot=0, params=params)
    want = ref.plan(s, so, start, params, nom, words, 1, None, track)
    cost = got["cost"]
    own = np.array([[math.exp(-(c - row.min()) / lam) for c in row] for row in cost])
    err_own = ref.gated(got["weight"], own, "weights from the device's own costs")
    amp = float(np.max(np.abs(cost - want["cost"])) / lam)
    print("lambda %g: weights against exp of the device's own costs rel_err %.3e; largest |delta cost| / lambda %.3e" % (lam, err_own, amp))
    assert err_own < ref.GATE
    if lam < 1.0:
        assert np.any(cost - cost.min(axis=1, keepdims=True) > 1.0)
        for n in range(6):      # whoever costs 1 more than the winner has weight exp(-1000) = 0
            far = cost[n] - cost[n].min() > 1.0
            assert np.all(got["weight"][n][far] == 0.0) and got["weight"][n][int(np.argmin(cost[n]))] == 1.0
    else:
        assert np.all(got["info"][:, 2] > 15.99)
        assert np.allclose(got["actions"], got["candidates"][:, :, 0].mean(axis=1), rtol=1e-3, atol=1e-6)
    stats = new_stats()
    check_rows(s, want, got, "lambda %g" % lam, stats)
    report("lambda %g" % lam, stats)
    assert stats["left_out"] == 0
    sim.close()


def test_hand_both_clamps_bind(amd):
    so = rr.scan_oracle("example_map")
    s = ref.settings(k=64, horizon=5, repeat=1, sigma_steer=50.0, sigma_speed=500.0)
    start, params = six_rows()
    nom, words = nominal_for(s, 6), streams_for(14, range(6))
    sim = two_maps(amd)
    got = sim.mppi_rows(mppi_of(amd, s), start, nom, words, slot=0, params=params)
    want = ref.plan(s, so, start, params, nom, words, 1)
    assert same_bits(got["candidates"], want["candidates"])
    V = got["candidates"][:, 1:]
    for c, lo, hi in ((0, s["steer_min"], s["steer_max"]), (1, s["speed_min"], s["speed_max"])):
        assert np.any(V[..., c] == lo) and np.any(V[..., c] == hi) and np.all((V[..., c] >= lo) & (V[..., c] <= hi))
    stats = new_stats()
    check_rows(s, want, got, "both clamps", stats)
    report("both clamps", stats)
    assert stats["left_out"] == 0
    sim.close()


def test_hand_draws_through_the_wedge_and_the_tail(amd):
    """row 0 draws from the stored seed's first stream, whose K = 64, H = 5 draws take the ziggurat's wedge test and its tail loop
    (tests/test_mppi_host.py holds the seed to that): V and the streams are NumPy's, and a draw from beyond the base layer is there"""
    so = rr.scan_oracle("example_map")
    s = ref.zig_settings()
    start, params = six_rows()
    nom, words = nominal_for(s, 6), streams_for(ref.ZIG_SEED, range(6))
    sim = two_maps(amd)
    got = sim.mppi_rows(mppi_of(amd, s), start, nom, words, slot=0, params=params)
    want = ref.plan(s, so, start, params, nom, words, 1)
    assert same_bits(got["candidates"], want["candidates"]) and same_bits(got["streams"], want["streams"])
    speed = (got["candidates"][0, 1:, :, 1] - nom[0, None, :, 1]) / s["sigma_speed"]
    steer = (got["candidates"][0, 1:, :, 0] - nom[0, None, :, 0]) / s["sigma_steer"]
    assert max(np.abs(speed).max(), np.abs(steer).max()) > ref.ZIG_BASE - 1e-6
    stats = new_stats()
    check_rows(s, want, got, "wedge and tail", stats)
    report("wedge and tail", stats)
    assert stats["left_out"] == 0
    sim.close()


# ---- (e) re-arming --------------------------------------------------------------------------------------------------------------------------
REARM_E, REARM_A, REARM_STEER = 8, 2, 0.03
REARM = (      # (settings, agents, seed): d_end is allocated, goes away, comes back; the buffers change size every time
    (dict(k=64, horizon=5, repeat=2, w_progress=3.0, w_lat=0.5, margin=0.25), np.arange(0, 16, 2), 61),
    (dict(k=3, horizon=33, repeat=2, w_progress=0.0, w_lat=0.0, margin=0.25, clear_ref=5.0), np.arange(0, 16, 2), 62),      # (every clearance counts:
    # with the default clear_ref = 0.6 and no track term, candidates that keep 0.6 m clear all cost 0.0 and tie from different rollouts)
    (dict(k=17, horizon=2, repeat=2, w_progress=3.0, w_lat=0.25, margin=0.25), np.array([1, 2, 3, 7, 8, 14, 15]), 63),
)


def rearm_run(amd, groups, sync, stats=None):
    """arm, one step, one call — three times, then disarm.  sync: the handle is synchronised after every call and the call is held
    to the model (the planner is fresh after each arming: nominal (0, v_init), the streams of the seed).  Without: nothing waits on
    the host between a call and the re-arm behind it; the outputs are read at the end.  -> the outputs' arrays"""
    from f1tenth_gym_amd import _ffi
    sim, start = warm_sim(amd, REARM_E, REARM_A, steps=5, step_groups=groups)
    N = sim.N
    d_const = sim.device_array((N, 2))
    d_const.upload(np.tile([REARM_STEER, 2.5], (N, 1)))
    bufs = [poisoned(sim, 20 + t) for t in range(len(REARM) + 1)]
    fifo = start[:, 7:9]
    out = []
    for t, (kw, agents, seed) in enumerate(REARM):
        s = ref.settings(**kw)
        d_act, d_info, poison_a, poison_i = bufs[t]
        sim.set_mppi(mppi_of(amd, s), agents, seed=seed)
        sim.step_device(d_const)
        sim.mppi_device(d_act, d_info)
        assert sim.step_groups()[2] == groups
        fifo = np.stack([np.full(N, REARM_STEER), fifo[:, 0]], axis=1)
        if not sync:
            continue
        sim.sync()
        act, info = d_act.download(), d_info.download()
        nom, words = sim.get_mppi_state()
        o = sim.get("state", "step_count")
        other = np.setdiff1d(np.arange(N), agents)
        assert same_bits(act[other], poison_a[other]) and same_bits(info[other], poison_i[other]), "arming %d: a row of an agent that is not armed was written" % t
        out += [nom, words]
        if stats is not None:
            m = len(agents)
            rows = np.concatenate([o["state"], fifo, np.full((N, 1), 2.0)], axis=1)[agents]
            want = ref.plan(s, rr.scan_oracle("example_map"), rows, np.tile(rr.orc.params_vec(), (m, 1)), mppi_of(amd, s).fresh_nominal(m),
                            streams_for(seed, agents), 1, o["step_count"][agents], rr.grid_track("example_map") if mppi_of(amd, s).needs_track else None)
            check_rows(s, want, dict(actions=act[agents], info=info[agents], nominal=nom, streams=words), "arming %d (K = %d, H = %d)" % (t, s["k"], s["horizon"]), stats)
            print("arming %d: %d rows so far, %d left out" % (t, stats["rows"], stats["left_out"]))
    # disarmed: the call is refused with the state error and writes nothing
    d_act, d_info, poison_a, poison_i = bufs[-1]
    sim.clear_mppi()
    assert _ffi.lib().f110_mppi_device(sim._h, d_act.ptr, d_info.ptr) == _ffi.ERR_STATE and "armed" in _ffi.last_error(sim._h)
    sim.sync()
    assert same_bits(d_act.download(), poison_a) and same_bits(d_info.download(), poison_i), "the refused call wrote an output"
    res = [a.download() for b in bufs[:-1] for a in b[:2]] + [sim.get("state")["state"]]
    sim.close()
    return res, out


def test_rearm_with_other_shapes_then_disarm(amd):
    stats = new_stats()
    rearm_run(amd, 1, True, stats)
    report("re-arming on one block", stats)


def test_rearm_behind_two_block_calls_without_a_wait(amd):
    stats = new_stats()
    waited, _ = rearm_run(amd, 2, True, stats)
    report("re-arming on two blocks", stats)
    rushed, _ = rearm_run(amd, 2, False)
    for t, (a, b) in enumerate(zip(rushed, waited)):
        assert same_bits(a, b), "output %d differs between the run that never waits and the one that waits after every call" % t
