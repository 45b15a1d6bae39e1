"""The opponent term's kernels (k_opp_predict, k_rollout_opp, k_mppi_roll_opp) where tests/test_gpu_opponents.py does not
reach: the model, the gate and the leave-out rule are that file's (tests/opponents_ref.py; rel_err < 1e-5, finite exactly where the
model is, a candidate with a sample within 1e-9 * radius of the radius may be left out, at most 1 %).

(a) the unit form at long horizons and many opponents (opponents_ref.EDGE_CASES): H = 15, 16, 17, 32, 33 and 64 — the end of the first,
    the second and the last lap of k_opp_predict's stride loop (lane `sub` writes the actions sub, sub + 16, ...) —, repeat up to 16,
    Ao = 5, 16 and 31 (15, 48 and 93 groups of 16 lanes: an idle group that shadows the last one, three full workgroups, a ragged last
    workgroup; 31 is the limit), and a finite max_range that leaves ignored opponents between predicted ones.
(b) the cases tests/test_opponents_host.py works out by hand, on the device, each in a call shared with two healthy rows whose results
    must not change: parked on the path, max_range and NaN rows, a NaN heading, a dead candidate, the closed track's seam crossed in the
    stride loop's second lap in both directions, an opponent beyond 2 L, the open track's end.
(c) the device form with 5, 17 and 32 cars per env (Ao = 4, 16, 31 from the live columns, agents in the middle of their env): d_opp
    bit for bit the unit form on the env's other cars in ascending slot; 33 cars are refused.
(d) the planner with the term across two unequal env blocks at K = 64 (k_mppi_roll_opp<UNI> with i0 != 0) and K = 65, and with 5 cars
    per env (prediction rows indexed by the armed list, Ao = 4)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import mppi_ref as mr
import opponents_ref as ref
import rollout_ref as rr
from _util import bench_start_poses, load_map_image, rel_err, track_oracle
from mppi_ref import gated, mppi_of, same_bits, streams_for, two_maps, warm_sim
from opponents_ref import live_opponents

pytestmark = pytest.mark.gpu

GATE = 1e-5
INF, NAN = float("inf"), float("nan")
ALL10 = rr.CHANNELS
OUT_KEYS = ("out", "raw", "traj", "traj_raw", "pred", "opp_raw", "opp")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def unit_sim(amd):
    sim = two_maps(amd)      # slot 0: example_map with its closed raceline, slot 1: berlin with the grid's open polyline
    yield sim
    sim.close()


def check_samples(s, got, what):
    """(OPP_MIN, OPP_FREE) of a map-frame unit call against the model on the device's own trajectory and predictions: OPP_FREE exactly,
    OPP_MIN under the gate, the float32 output the cast of the raw one -> (keep [m][K], rel_err)"""
    want_raw, near = ref.sample_rows(s, got["traj_raw"], got["pred"])
    keep = ~ref.left_out(near, s["radius"])
    assert np.array_equal(got["opp_raw"][..., 1][keep], want_raw[..., 1][keep]), (what, "OPP_FREE")
    err = gated(got["opp_raw"][..., 0][keep], want_raw[..., 0][keep], (what, "OPP_MIN"))
    assert err < GATE, (what, "OPP_MIN rel_err %.3e" % err)
    assert same_bits(got["opp"], got["opp_raw"].astype(np.float32)), (what, "the float32 output")
    return keep, err


# ---- (a) long horizons and many opponents, unit form ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ref.MODES)
@pytest.mark.parametrize("grid_map", rr.GRID_MAPS)
def test_unit_form_at_long_horizons_and_many_opponents(amd, unit_sim, grid_map, mode):
    sim, slot = unit_sim, rr.GRID_MAPS.index(grid_map)
    cands = left = hits = 0
    worst = 0.0
    seen = set()
    for case in ref.edge_cases((grid_map,), (mode,)):
        _, K, H, repeat, _, Ao, max_range, _ = case
        s = ref.edge_settings(case)
        start, params, actions, opp = ref.edge_inputs(case)
        p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=rr.GRID_MARGIN, frame="ego", traj=True)
        got = sim.rollout_opp_rows(p, amd.Opponents(**s), start, actions, opp, slot=slot, params=params)
        plain = sim.rollout_rows(p, start, actions, slot=slot, params=params, raw=True)
        for a, b in zip((got["out"], got["traj"], got["raw"], got["traj_raw"]), plain):
            assert same_bits(a, b), (case, "the rollout's own outputs changed")
        want_pred = ref.edge_pred(case)
        err = gated(got["pred"], want_pred, (case, "pred"))
        assert err < GATE, (case, "pred rel_err %.3e" % err)
        worst = max(worst, err)
        if max_range != INF:
            assert ref.nan_rows_between_finite(got["pred"]), (case, "no ignored opponent between two predicted ones")
        # the samples on the device's own map-frame positions (the term reads the map frame whatever the spec says) and predictions
        pm = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=rr.GRID_MARGIN, frame="map", traj=True)
        gm = sim.rollout_opp_rows(pm, amd.Opponents(**s), start, actions, opp, slot=slot, params=params)
        assert same_bits(gm["opp_raw"], got["opp_raw"]) and same_bits(gm["pred"], got["pred"]), (case, "the spec's frame changed the term")
        assert same_bits(got["opp"], got["opp_raw"].astype(np.float32)), (case, "the float32 output")
        keep, err = check_samples(s, gm, case)
        worst = max(worst, err)
        cands += keep.size
        left += int(np.count_nonzero(~keep))
        hits += int(np.count_nonzero(got["opp_raw"][..., 1] < H))
        seen.add((H, Ao))
    assert {h for h, _ in seen} == {15, 16, 17, 32, 33, 64} and {a for _, a in seen} == set(ref.EDGE_AO)
    print("opponents edge grid on %s, %s: %d candidates, %d left out, %d hit, largest rel_err %.3e" % (grid_map, mode, cands, left, hits, worst))
    assert left * 100 <= cands and hits > 0


# ---- (b) the hand cases on the device --------------------------------------------------------------------------------------------------------
P1 = rr.orc.params_vec()[None, :]
FREE = tuple(rr.grid_rows("example_map")[0][0, [0, 1, 4]])       # on the example raceline
HAND = 1                                                       # the hand row, between the two healthy ones


def hand_call(amd, sim, s, hand_start, hand_opp, H=6, repeat=5, v=2.0, margin=-INF, map_name="example_map", on_radius=False):
    """the hand row (one candidate: zero steer at the commanded speed v) between the grid's rows 0 and 2 with their own opponents, in
    one call: the healthy rows bit for bit a call without it; every row's predictions against the model under the gate and its samples
    against the model on the device's own trajectory and predictions (on_radius: the hand case has a sample about a radius away, and
    the leave-out rule may apply to it too).  -> the three-row dict (map frame)"""
    slot, track = rr.GRID_MAPS.index(map_name), rr.grid_track(map_name)
    hand_opp = np.asarray(hand_opp, dtype=np.float64).reshape(-1, 4)
    Ao = hand_opp.shape[0]
    g_start, g_params = rr.grid_rows(map_name)
    g_opp = ref.grid_opponents(map_name, Ao)
    start = np.concatenate([g_start[0:1], hand_start, g_start[2:3]])
    params = np.concatenate([g_params[0:1], P1, g_params[2:3]])
    opp = np.stack([g_opp[0], hand_opp, g_opp[2]])
    actions = np.zeros((1, H, 2))
    actions[..., 1] = v
    p = amd.Rollout(k=1, horizon=H, repeat=repeat, channels=ALL10, margin=margin, frame="map", traj=True)
    got = sim.rollout_opp_rows(p, amd.Opponents(**s), start, actions, opp, slot=slot, params=params)
    healthy = [0, 2]
    alone = sim.rollout_opp_rows(p, amd.Opponents(**s), start[healthy], actions, opp[healthy], slot=slot, params=params[healthy])
    for key in OUT_KEYS:
        assert same_bits(got[key][healthy], alone[key]), "the hand row changed a healthy row's %s" % key
    want = np.stack([ref.predict(s, start[n, 0], start[n, 1], opp[n], H, repeat, track=track) for n in range(3)]) if Ao else np.zeros((3, 0, H, 2))
    err = gated(got["pred"], want, "pred")
    assert err < GATE, "pred rel_err %.3e" % err
    keep, err2 = check_samples(s, got, "hand")
    assert on_radius or keep[HAND].all(), "the hand case itself lies on the radius"
    print("hand call on %s, Ao = %d: pred rel_err %.3e, OPP_MIN rel_err %.3e, %d healthy candidates left out" % (map_name, Ao, err, err2, np.count_nonzero(~keep)))
    return got


def ahead(r, v=0.0, theta=0.0):
    return [FREE[0] + r * math.cos(FREE[2]), FREE[1] + r * math.sin(FREE[2]), v, theta]


def free_row(v=2.0):
    return ref.hand_row(FREE[0], FREE[1], FREE[2], v=v)


def test_hand_parked_on_the_path(amd, unit_sim):
    """an opponent parked 0.35 m ahead on the heading, the car covers 0.1 m per action: distances 0.25, 0.15, 0.05, 0.05, 0.15, 0.25"""
    opp = ahead(0.35, theta=1.0)
    got = hand_call(amd, unit_sim, ref.settings(radius=0.2), free_row(), opp)
    assert got["opp_raw"][HAND, 0, 1] == 1.0 and abs(got["opp_raw"][HAND, 0, 0] - 0.05) < 1e-6
    assert np.all(got["pred"][HAND, 0] == np.array(opp[:2])), "v = 0: parked, whatever its heading"
    d = np.hypot(*(got["traj_raw"][HAND, 0, :, :2] - np.array(opp[:2])).T)
    assert np.allclose(d, [0.25, 0.15, 0.05, 0.05, 0.15, 0.25], atol=1e-6)
    never = hand_call(amd, unit_sim, ref.settings(radius=0.04), free_row(), opp)["opp_raw"][HAND, 0]
    assert never.tolist() == [got["opp_raw"][HAND, 0, 0], 6.0], "never within 4 cm"
    assert hand_call(amd, unit_sim, ref.settings(radius=0.26), free_row(), opp)["opp_raw"][HAND, 0, 1] == 0.0
    moving = hand_call(amd, unit_sim, ref.settings(radius=0.2), free_row(), ahead(0.35, v=2.0, theta=FREE[2]))
    assert moving["opp_raw"][HAND, 0, 1] == 6.0 and abs(moving["opp_raw"][HAND, 0, 0] - 0.35) < 1e-6, "at the car's own speed it stays 0.35 m away"


def test_hand_max_range_and_nan_rows(amd, unit_sim):
    """(0.4 and 0.6 m ahead at 0.1 m per action: a sample lies about the radius of 0.2 m away, so these cases assert no action)"""
    hand_call = functools.partial(globals()["hand_call"], on_radius=True)
    inside, outside = ahead(0.4), ahead(0.6)
    s, wide = ref.settings(radius=0.2, max_range=0.5), ref.settings(radius=0.2)
    g_in, g_out = (hand_call(amd, unit_sim, s, free_row(), o) for o in (inside, outside))
    assert np.all(np.isfinite(g_in["pred"][HAND])) and g_in["opp_raw"][HAND, 0, 1] < 6.0
    assert np.all(np.isnan(g_out["pred"][HAND])) and g_out["opp_raw"][HAND, 0].tolist() == [INF, 6.0]
    assert hand_call(amd, unit_sim, wide, free_row(), outside)["opp_raw"][HAND, 0, 1] < 6.0, "seen without the limit"
    # exactly on the limit counts (<=)
    edge = [FREE[0] + 0.5, FREE[1], 0.0, 0.0]
    assert np.all(np.isfinite(hand_call(amd, unit_sim, ref.settings(radius=0.2, max_range=edge[0] - FREE[0]), free_row(), edge)["pred"][HAND]))
    # a NaN opponent beside a real one, on either side of it: its row is NaN and it changes nothing
    one = hand_call(amd, unit_sim, wide, free_row(), inside)
    both = hand_call(amd, unit_sim, wide, free_row(), [inside, [NAN, 0.0, 1.0, 0.0]])
    assert np.all(np.isnan(both["pred"][HAND, 1])) and same_bits(both["pred"][HAND, 0], one["pred"][HAND, 0])
    assert same_bits(both["opp_raw"][HAND], one["opp_raw"][HAND])
    swapped = hand_call(amd, unit_sim, wide, free_row(), [[0.0, NAN, 1.0, 0.0], inside])
    assert np.all(np.isnan(swapped["pred"][HAND, 0])) and same_bits(swapped["opp_raw"][HAND], one["opp_raw"][HAND])
    # a NaN heading with a position in range: CV's predictions are NaN through the device's cos_sin, and measure nothing
    nanth = hand_call(amd, unit_sim, wide, free_row(), [inside[0], inside[1], 1.0, NAN])
    assert np.all(np.isnan(nanth["pred"][HAND])) and nanth["opp_raw"][HAND, 0].tolist() == [INF, 6.0]
    # no opponents at all
    none = hand_call(amd, unit_sim, wide, free_row(), np.zeros((0, 4)))
    assert none["opp_raw"][HAND, 0].tolist() == [INF, 6.0] and none["opp"][HAND, 0].tolist() == [INF, 6.0]


def test_hand_a_dead_candidate_stays_where_it_died(amd, unit_sim):
    """a margin above every clearance kills the candidate at its first step: it is frozen one step from the start while the opponent
    drives by from behind; 0.42, 0.32, 0.22, 0.12, 0.02, 0.08 m from the pose 0.02 m along"""
    got = hand_call(amd, unit_sim, ref.settings(radius=0.15), free_row(), ahead(-0.5, v=2.0, theta=FREE[2]), margin=INF)
    assert got["raw"][HAND, 0, rr.ALIVE] == 0.0
    xy = got["traj_raw"][HAND, 0, :, :2]
    assert same_bits(xy, np.tile(xy[0], (6, 1))), "frozen"
    d = np.hypot(*(got["pred"][HAND, 0] - xy[0]).T)
    assert got["opp_raw"][HAND, 0, 1] == 3.0 == float(np.argmax(d < 0.15)) and abs(got["opp_raw"][HAND, 0, 0] - 0.02) < 1e-6
    assert abs(got["opp_raw"][HAND, 0, 0] - d.min()) <= 1e-12


def test_hand_track_mode_across_the_seam_in_the_second_lap(amd, unit_sim):
    """TRACK on the closed example raceline, H = 20 actions of 5 steps: one opponent crosses the seam forward and one backward at an
    action >= 16, which the second lap of k_opp_predict's stride loop writes; a third lies beyond 2 L at the last action, where the
    rule's one subtraction leaves s >= L (the station is the track's end point).  The lateral offsets are kept."""
    track = rr.grid_track("example_map")
    cols, L, H, repeat = ref.track_cols(track), track.length, 20, 5
    opp = ref.seam_opponents(track)
    fwd, back, fast = (ref.stations_of(track, o, H, repeat) for o in opp)
    assert 16 <= int(np.argmax(fwd >= L)) < H and not np.any(fwd[:16] >= L), "the forward opponent does not cross in the second lap"
    assert 16 <= int(np.argmax(back < 0.0)) < H and not np.any(back[:16] < 0.0), "the backward opponent does not cross in the second lap"
    assert fast[-1] > 2.0 * L and fast[-1] - L >= L
    st = ref.hand_row(cols[0][0], cols[1][0], 0.0, v=1.0)
    got = hand_call(amd, unit_sim, ref.settings(mode="track", radius=0.2), st, opp, H=H, repeat=repeat, v=1.0)
    pred = got["pred"][HAND]
    assert np.all(np.isfinite(pred))
    proj = lambda o: np.array([track_oracle(track, np.array([[p[0], p[1], 0.0]]))[0, :2] for p in pred[o]])
    pf, pb = proj(0), proj(1)
    assert pf[0, 0] > 0.9 * L and pf[-1, 0] < 0.1 * L and pb[0, 0] < 0.1 * L and pb[-1, 0] > 0.9 * L
    assert np.all(pf[:16, 0] > 0.9 * L) and np.all(pb[:16, 0] < 0.1 * L), "a crossing before action 16"
    assert np.allclose(pf[:, 1], 0.2, atol=0.02) and np.allclose(pb[:, 1], -0.1, atol=0.02)
    want = ref.predict(ref.settings(mode="track", radius=0.2), st[0, 0], st[0, 1], opp[2:3], H, repeat, track=track)[0, -1]
    assert np.all(np.isfinite(pred[2, -1])) and rel_err(pred[2, -1], want) < GATE, "beyond 2 L: the device's station is not the model's"


def test_hand_track_mode_at_the_open_track_s_end(amd, unit_sim):
    """berlin's open polyline does not wrap: an opponent at its last point driving on at 50 m/s stays at the end point (t clipped)"""
    otr = rr.grid_track("berlin")
    ocols = ref.track_cols(otr)
    e = otr.num_segments - 1
    tip = [ocols[0][e] + ocols[2][e], ocols[1][e] + ocols[3][e], 50.0, 0.0]
    g_start = rr.grid_rows("berlin")[0]
    st = ref.hand_row(g_start[3, 0], g_start[3, 1], g_start[3, 4], v=1.0)
    got = hand_call(amd, unit_sim, ref.settings(mode="track"), st, tip, H=3, repeat=5, v=1.0, map_name="berlin")
    p = got["pred"][HAND, 0]
    assert same_bits(p, np.tile(p[0], (3, 1))) and np.allclose(p[0], tip[:2], atol=1e-9)


# ---- (c) many cars per env, device form ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E,A", [(5, 5), (4, 17), (3, 32)])
@pytest.mark.parametrize("mode", ref.MODES)
def test_device_form_with_many_cars_per_env(amd, E, A, mode):
    N = E * A
    sim, start = warm_sim(amd, E, A)
    K, H, repeat = 3, 17, 2
    p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ALL10, margin=0.25, frame="ego", traj=True, layout="per_agent")
    op = amd.Opponents(mode=mode, radius=2.0, max_range=5.0)         # the cars of an env start 10 waypoints (2 m) apart: two on either side are in range
    actions = rr.grid_actions(K, H, True, m=N)
    d_act = sim.device_array(actions.shape)
    d_act.upload(actions)
    opp_rows = live_opponents(start[:, :7], A)                       # the state fetched before the call (warm_sim)
    out0, traj0 = sim.rollout_device(p, d_act)
    out, traj, opp = sim.rollout_opp_device(p, op, d_act)
    sim.sync()
    assert same_bits(out.download(), out0.download()) and same_bits(traj.download(), traj0.download()), "d_out / d_traj are not f110_rollout_device's"
    unit = sim.rollout_opp_rows(p, op, start, actions, opp_rows)
    got = opp.download()
    assert same_bits(got, unit["opp"]), "d_opp is not the unit form's on the env's other cars in ascending slot"
    assert same_bits(out.download(), unit["out"])
    # an agent in the middle of its env: opponents from both sides of its own slot, with distinct predictions, so that the order shows
    n = 1 * A + A // 2
    a = n % A
    assert 0 < a < A - 1
    below, above = unit["pred"][n, a - 1], unit["pred"][n, a]         # the cars in the slots a - 1 and a + 1
    assert np.all(np.isfinite(below)) and np.all(np.isfinite(above)) and not np.any(np.all(below == above, axis=-1))
    assert np.array_equal(opp_rows[n, a - 1], start[n - 1, [0, 1, 3, 4]]) and np.array_equal(opp_rows[n, a], start[n + 1, [0, 1, 3, 4]])
    swapped = opp_rows.copy()
    swapped[n, [a - 1, a]] = opp_rows[n, [a, a - 1]]
    pred_s = sim.rollout_opp_rows(p, op, start, actions, swapped)["pred"]
    assert same_bits(pred_s[n, a - 1], above) and same_bits(pred_s[n, a], below) and not same_bits(pred_s[n], unit["pred"][n])
    # leaving the upper neighbour out for the agent itself (an off-by-one in the live columns) would show in d_opp
    wrong = opp_rows.copy()
    wrong[n, a] = start[n, [0, 1, 3, 4]]
    assert not same_bits(sim.rollout_opp_rows(p, op, start, actions, wrong)["opp"][n], got[n]), "the case cannot tell the agent from its neighbour"
    print("device form %d x %d, %s: %d of %d candidates come within the radius" % (E, A, mode, np.count_nonzero(got[..., 1] < H), got[..., 1].size))
    sim.close()


def test_33_cars_per_env_are_refused(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 1, 33
    L = _ffi.lib()
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((A, 2)))
    good = amd.Rollout(k=3, horizon=2, repeat=2, channels=("end_x", "alive"), margin=0.2, traj=True)
    op = amd.Opponents(radius=0.5)
    shapes = (good.shape(A), good.traj_shape(A), (A, 3, 2))
    rng = np.random.default_rng(1)
    sent = [rng.normal(size=sh).astype(np.float32) for sh in shapes]
    bufs = [s.device_array(sh, np.float32) for sh in shapes]
    for d, v in zip(bufs, sent):
        d.upload(v)
    cand = np.tile([0.0, 2.0], (3, 2, 1))
    d_cand = s.device_array(cand.shape)
    d_cand.upload(cand)
    sp, osp = good.spec(), op.spec()
    assert L.f110_rollout_opp_device(s._h, C.byref(sp), C.byref(osp), d_cand.ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, None) == _ffi.ERR_INVALID
    assert "32 opponents" in _ffi.last_error(s._h)
    assert L.f110_rollout_device(s._h, C.byref(sp), d_cand.ptr, bufs[0].ptr, bufs[1].ptr, None) == _ffi.OK        # (the plain rollout takes 33 cars)
    s.sync()
    plain = [b.download() for b in bufs]
    assert not same_bits(plain[0], sent[0]) and same_bits(plain[2], sent[2])
    for d, v in zip(bufs, sent):
        d.upload(v)
    mp = amd.Mppi(k=4, horizon=3, repeat=2, w_progress=0.0, w_lat=0.0)
    s.set_mppi(mp, None, seed=1)
    before = s.get_mppi_state()
    assert L.f110_mppi_set_opponents(s._h, C.byref(osp), C.c_double(1.0), C.c_double(1.0), C.c_double(1.0)) == _ffi.ERR_INVALID
    assert "32 opponents" in _ffi.last_error(s._h)
    with pytest.raises(ValueError):
        s.set_mppi_opponents(op, 1.0, 1.0, 1.0)
    assert s.mppi_opponents is None
    with pytest.raises(ValueError):
        s.rollout_opp_device(good, op, d_cand, *bufs)
    s.sync()
    for d, v in zip(bufs, sent):
        assert same_bits(d.download(), v), "a refused call wrote an output"
    for x, y in zip(s.get_mppi_state(), before):
        assert same_bits(x, y)
    s.close()


# ---- (d) the planner ---------------------------------------------------------------------------------------------------------------------------
W = (3.0, 1.5, 2.5)      # w_hit, w_near, near_ref: the cars of an env are about 2 m apart, so both terms act
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


def planner_against_unit_form(amd, sim, mp, op, s, agents, seed, start, act, info, nom, words, what, fresh=None):
    """the device form's armed rows bit for bit mppi_opp_rows on `start`; the unit form's costs against the model on the device's own
    rollout values, its predictions against the model"""
    A, m = sim.A, len(agents)
    params = np.tile(rr.orc.params_vec(), (m, 1))
    opp = live_opponents(start[:, :7], A)[agents]
    unit = sim.mppi_opp_rows(mp, op, W[0], W[1], W[2], start[agents], mp.fresh_nominal(m), streams_for(seed, agents), opp, params=params, fresh=fresh)
    for key, mine in (("actions", act[agents]), ("info", info[agents]), ("nominal", nom), ("streams", words)):
        assert same_bits(unit[key], mine), (what, key, "the device form against the unit form")
    ro = amd.Rollout(k=s["k"], horizon=s["horizon"], repeat=s["repeat"], channels=ALL10, margin=s["margin"], frame="map", traj=True, layout="per_agent")
    rolled = sim.rollout_opp_rows(ro, op, start[agents], unit["candidates"], opp, params=params)
    os_ = dict(mode=op.mode, radius=op.radius, max_range=op.max_range)
    track = rr.grid_track("example_map")
    want_pred = np.stack([ref.predict(os_, start[n, 0], start[n, 1], opp[i], s["horizon"], s["repeat"], track=track) for i, n in enumerate(agents)])
    err_p = gated(rolled["pred"], want_pred, (what, "pred"))
    raw4 = rolled["raw"][..., [rr.ALIVE, rr.MIN_CLEAR, rr.PROGRESS, rr.END_LAT]]
    err_c = gated(unit["cost"], ref.costs(s, W[0], W[1], W[2], raw4, unit["opp_raw"]), (what, "cost"))
    print("%s: pred rel_err %.3e, cost rel_err %.3e, %d of %d candidates hit" % (what, err_p, err_c, np.count_nonzero(unit["opp_raw"][..., 1] < s["horizon"]),
                                                                           unit["opp_raw"][..., 1].size))
    assert err_p < GATE and err_c < GATE
    return unit


@pytest.mark.parametrize("armed", [[0, 255, 256, 259], [257, 258], [3]], ids=["straddle", "first_empty", "second_empty"])
@pytest.mark.parametrize("K", [64, 65])
def test_planner_armed_list_across_unequal_env_blocks(amd, block_sims, K, armed):
    """two device steps back to back, then the call right behind them: on the two-block handle it rides the blocks (armed indices
    [i0, i0 + count) per block, i0 != 0 or count == 0 in one of them; K = 64 is k_mppi_roll_opp<UNI>).  The planner changes no state,
    so the state read back after the call is the one it planned from; two steps with one steering command leave the FIFO full of it."""
    agents = np.array(armed)
    s = mr.settings(k=K, horizon=5, repeat=2, w_progress=3.0, w_lat=0.5, margin=0.25)
    mp, op = mppi_of(amd, s), amd.Opponents(mode="track", radius=2.0, max_range=10.0)
    seed = 70 + K
    res = {}
    for groups in (2, 1):
        sim, d_const = block_sims[groups]
        N = sim.N
        rng = np.random.default_rng(11)              # (the same poison on both handles)
        sim.set_mppi(mp, agents, seed=seed)
        sim.set_mppi_opponents(op, *W)
        poison_a, poison_i = rng.normal(size=(N, 2)), rng.normal(size=(N, 4)).astype(np.float32)
        d_act, d_info = sim.device_array((N, 2)), sim.device_array((N, 4), np.float32)
        d_act.upload(poison_a)
        d_info.upload(poison_i)
        sim.step_device(d_const)
        sim.step_device(d_const)
        sim.mppi_device(d_act, d_info)
        assert sim.step_groups()[2] == groups, "the steps went out as %d block(s)" % sim.step_groups()[2]
        act, info = d_act.download(), d_info.download()
        nom, words = sim.get_mppi_state()
        other = np.setdiff1d(np.arange(N), agents)
        assert same_bits(act[other], poison_a[other]) and same_bits(info[other], poison_i[other]), "%d block(s): a row of an agent that is not armed was written" % groups
        res[groups] = (act, info, nom, words, sim.get("state")["state"])
        d_act.free()
        d_info.free()
        sim.clear_mppi()
    for a, b in zip(res[2], res[1]):
        assert same_bits(a, b), "two blocks against one"
    act, info, nom, words, state = res[2]
    start = np.concatenate([state, np.full((state.shape[0], 2), BLOCK_STEER), np.full((state.shape[0], 1), 2.0)], axis=1)
    unit = planner_against_unit_form(amd, block_sims[2][0], mp, op, s, agents, seed, start, act, info, nom, words, "blocks of 128 and 2 envs, K = %d, armed %s" % (K, armed))
    assert np.all(np.isfinite(unit["opp_raw"][..., 0])), "every armed agent has its opponent in range"


def test_planner_with_five_cars_per_env(amd):
    """6 envs x 5 cars, armed agents in every slot of an env: the prediction rows are indexed by the armed list, four opponents each
    from the live columns"""
    E, A, seed = 6, 5, 91
    N = E * A
    sim, start = warm_sim(amd, E, A)
    agents = np.array([1, 5, 7, 8, 14, 22, 29])
    assert set(agents % A) == set(range(A))
    s = mr.settings(k=7, horizon=5, repeat=3, w_progress=3.0, w_lat=0.5, margin=0.25)
    mp, op = mppi_of(amd, s), amd.Opponents(mode="track", radius=2.0, max_range=5.0)
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
    fresh = sim.get("step_count")["step_count"][agents]
    unit = planner_against_unit_form(amd, sim, mp, op, s, agents, seed, start, act, info, nom, words, "5 cars per env", fresh=fresh)
    assert np.any(unit["opp_raw"][..., 0] < W[2]) and np.any(unit["opp_raw"][..., 1] < s["horizon"]), "no candidate comes near an opponent: the case shows nothing"
    sim.close()
