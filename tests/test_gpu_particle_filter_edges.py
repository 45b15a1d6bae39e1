"""The particle filter's kernels (k_pf_plan / _move / _sense / _update) where tests/test_gpu_particle_filter.py does not
reach: the model, the stage-by-stage comparison, the gate and the leave-out rule are that file's (tests/particle_filter_ref.py:
check_stages; rel_err < 1e-5, the draws, the streams and L bit for bit, at most 1 % of the rows and of the slots left out).

(a) every lane grouping of k_pf_update in the unit form: P = 16 | 17, 32 | 33, 128 | 129 on both sides of the bounds between GS = 16,
    32, 64 and 256 (33 is GS = 64, 128 is GS = 128), 256 | 257 where GS = 256 goes from one pass to two; B' = 7 and 64, stride 1 and
    the largest that fits, both maps, a fresh row among the three, both resampling outcomes.
(b) one device-form case per GS (P = 16, 24, 64, 100, 200): seven of 22 agents armed, so that the last workgroup holds live groups
    beside idle ones, the other rows poisoned, two calls in a row.
(c) the cases tests/test_particle_filter_host.py works out by hand, on the device, each in a call (and, at P <= 16, a k_pf_update
    workgroup) shared with two healthy rows whose outputs must not change: a particle outside the map, a NaN scan value under a finite
    and an infinite clip, one surviving weight, the underflow fall-back to uniform weights, a heading change across the yaw wrap in
    both directions, one particle."""
import numpy as np
import pytest

import particle_filter_ref as ref
import rollout_ref as rr
from mppi_ref import two_maps, warm_sim
from particle_filter_ref import check_stages, filter_of, localize_and_check, poisoned, same_bits, seed_clouds

pytestmark = pytest.mark.gpu

INF, NAN = float("inf"), float("nan")
OUT_KEYS = ("pose", "info", "noise", "ancestors", "expected", "logw", "particles", "weights", "last", "streams")


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


def run_unit(amd, sim, s, inp, slot=0):
    poses, scans, X, W, last, words, fresh = inp
    return sim.localize_rows(filter_of(amd, s), poses, scans, X, W, last, words, slot=slot, fresh=fresh)


# ---- (a) every lane grouping, unit form ----------------------------------------------------------------------------------------------------
def test_the_grid_reaches_every_lane_grouping():
    assert {ref.group_lanes(P) for P in ref.EDGE_P} == {16, 32, 64, 128, 256}
    assert [ref.group_lanes(P) for P in ref.EDGE_P] == [16, 32, 32, 64, 128, 256, 256, 256]
    assert [-(-P // ref.group_lanes(P)) for P in ref.EDGE_P] == [1, 1, 1, 1, 1, 1, 1, 2], "the passes a lane takes over its particles"


@pytest.mark.parametrize("map_name", rr.GRID_MAPS)
@pytest.mark.parametrize("P", ref.EDGE_P)
def test_unit_form_at_every_lane_grouping(amd, unit_sim, map_name, P):
    so, slot = rr.scan_oracle(map_name), rr.GRID_MAPS.index(map_name)
    stats, outcomes = ref.new_stats(), set()
    cases = ref.edge_cases((map_name,), (P,))
    assert [c[2:] for c in cases] == [(7, False, 0), (7, True, 1), (64, False, 2), (64, True, 3)]
    for _, _, Bp, big, q in cases:
        s, inp = ref.unit_case(map_name, P, Bp, big, q)
        got = run_unit(amd, unit_sim, s, inp, slot)
        check_stages(s, so, inp, got, (map_name, P, Bp, s["beam_stride"], "GS %d" % ref.group_lanes(P)), stats)
        outcomes |= set(got["info"][[0, 2], 3].tolist())
    assert outcomes == {0.0, 1.0}, "both resampling outcomes"
    report("pf lane groupings on %s, P = %d (GS %d)" % (map_name, P, ref.group_lanes(P)), stats)


# ---- (b) one device-form case per GS -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [16, 24, 64, 100, 200])
def test_device_form_at_every_group_size(amd, P):
    """11 envs x 2 cars, seven agents armed: 256 / GS = 16, 8, 4, 2 agents fill a workgroup (GS = 256: one), so the last workgroup
    holds live groups beside idle ones, which shadow the last agent; a write of theirs lands in a poisoned row or changes an armed one"""
    E, A, seed = 11, 2, 600 + P
    N = E * A
    gs = ref.group_lanes(P)
    per = 256 // gs
    assert gs == {16: 16, 24: 32, 64: 64, 100: 128, 200: 256}[P]
    sim, _ = warm_sim(amd, E, A)
    agents = np.sort(np.random.default_rng(P).choice(N, 7, replace=False))
    assert len(agents) < N and (per == 1 or len(agents) % per != 0)
    s = ref.settings(particles=P, n_beams=7, beam_first=11, beam_stride=150)
    sim.set_particle_filter(filter_of(amd, s), agents, seed=seed)
    seed_clouds(sim, s, agents, 5)
    d_pose, d_info, pa, pi = poisoned(sim, 9)
    so, stats = rr.scan_oracle("example_map"), ref.new_stats()
    other = np.setdiff1d(np.arange(N), agents)
    rng = np.random.default_rng(P)
    seen = set()
    for call in range(2):
        _, info, _ = localize_and_check(amd, sim, s, so, agents, d_pose, d_info, "P = %d, call %d" % (P, call), stats)
        assert same_bits(d_pose.download()[other], pa[other]) and same_bits(info[other], pi[other]), "a row of an agent that is not armed was written"
        seen |= set(info[agents, 3].tolist())
        sim.step(np.stack([rng.uniform(-0.1, 0.1, N), rng.uniform(2.0, 4.0, N)], axis=1))
    report("pf device form, P = %d (GS %d, %d agents a workgroup, 7 armed), resampling outcomes %s" % (P, gs, per, sorted(seen)), stats)
    sim.close()


# ---- (c) the hand cases on the device ------------------------------------------------------------------------------------------------------
HAND = 1      # the hand row, between the two healthy ones


def one_row(**kw):
    """tests/test_particle_filter_host.py's hand row: (settings, poses [1][3], scans, particles, weights, last, streams)"""
    s = ref.settings(**kw)
    _, poses, scans, X, W, last, words = ref.rows_for("example_map", s["particles"], m=1, seed=77)
    return s, poses, scans, X, W, last, words


def hand_call(amd, sim, s, hand, what, stats):
    """the hand row (poses, scans, particles, weights, last, streams of one row) between two healthy rows of rows_for, in one call: the
    healthy rows bit for bit a call without it, all three held to the model by check_stages -> the three-row dict"""
    so, poses, scans, X, W, last, words = ref.rows_for("example_map", s["particles"], m=3, seed=55)
    inp = [a.copy() for a in (poses, scans, X, W, last, words)]
    for a, h in zip(inp, hand):
        a[HAND] = h[0]
    got = run_unit(amd, sim, s, tuple(inp) + (None,))
    healthy = [0, 2]
    alone = run_unit(amd, sim, s, tuple(a[healthy] for a in inp) + (None,))
    for key in OUT_KEYS:
        assert same_bits(got[key][healthy], alone[key]), "%s: the hand row changed a healthy row's %s" % (what, key)
    check_stages(s, so, tuple(inp) + (None,), got, what, stats)
    return got


def test_hand_a_particle_outside_the_map(amd, unit_sim):
    s, poses, scans, X, W, last, words = one_row(particles=2, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, resample_frac=0.0)
    X[0, 1] = (-500.0, 300.0, 1.0)
    stats = ref.new_stats()
    got = hand_call(amd, unit_sim, s, (poses, scans, X, W, poses.copy(), words), "outside", stats)
    assert same_bits(got["particles"][HAND, 1, :2], np.array([-500.0, 300.0])), "no move, no noise: the particle stays outside"
    assert np.all(np.isfinite(got["expected"][HAND])) and np.all(np.isfinite(got["pose"][HAND])) and got["weights"][HAND, 1] < got["weights"][HAND, 0]
    report("pf hand: a particle outside the map", stats)


@pytest.mark.parametrize("clip", [2.0, INF])
def test_hand_a_nan_scan_value_takes_the_clip_or_counts_as_nothing(amd, unit_sim, clip):
    s, poses, scans, X, W, last, words = one_row(particles=2, n_beams=3, clip=clip, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, resample_frac=0.0)
    stats = ref.new_stats()
    clean = hand_call(amd, unit_sim, s, (poses, scans, X, W, poses.copy(), words), ("clean", clip), stats)
    scans = scans.copy()
    idx = ref.beams(s)
    scans[0, idx[1]] = NAN
    got = hand_call(amd, unit_sim, s, (poses, scans, X, W, poses.copy(), words), ("nan", clip), stats)
    assert np.all(np.isfinite(got["logw"][HAND])) and same_bits(clean["expected"], got["expected"])
    for p in range(2):
        terms = [min(((z - r) / s["sigma_hit"]) ** 2, clip * clip) for z, r in zip(scans[0, idx], got["expected"][HAND, p])]
        terms[1] = clip * clip if clip != INF else 0.0
        assert got["logw"][HAND, p] == -(0.5 / s["squash"]) * ((0.0 + terms[0]) + terms[1] + terms[2]), "L is not the formula on the device's expected ranges"
    report("pf hand: a NaN scan value, clip %s" % clip, stats)


def test_hand_one_surviving_weight_is_every_ancestor(amd, unit_sim):
    s, poses, scans, X, W, last, words = one_row(particles=7, resample_frac=0.5)
    W = np.zeros((1, 7))
    W[0, 4] = 1.0
    stats = ref.new_stats()
    got = hand_call(amd, unit_sim, s, (poses, scans, X, W, last, words), "survivor", stats)
    assert np.all(got["ancestors"][HAND] == 4) and got["info"][HAND, 3] == 1.0
    report("pf hand: one surviving weight", stats)
    assert stats["rows_left_out"] == 0


def test_hand_underflow_falls_back_to_uniform_weights(amd, unit_sim):
    """a scan far from every expectation without truncation: the device's exp underflows for all but the best particle, which the
    prior gives no weight; eta is 0 and the weights become uniform.  `best` comes from the device's own L in a probe call."""
    s, poses, scans, X, W, last, words = one_row(particles=7, clip=INF, sigma_hit=1e-3, squash=1e-3, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0,
                                                 resample_frac=0.0)
    stats = ref.new_stats()
    probe = hand_call(amd, unit_sim, s, (poses, scans, X, W, poses.copy(), words), "underflow probe", stats)
    best = int(np.argmax(probe["logw"][HAND]))
    rest = np.delete(probe["logw"][HAND], best)
    assert np.all(rest - probe["logw"][HAND, best] < -800.0), "the other particles' exp does not underflow: the case shows nothing"
    W = np.full((1, 7), 1.0 / 6.0)
    W[0, best] = 0.0
    got = hand_call(amd, unit_sim, s, (poses, scans, X, W, poses.copy(), words), "underflow", stats)
    assert same_bits(got["logw"][HAND], probe["logw"][HAND])
    assert np.all(got["weights"][HAND] == 1.0 / 7.0) and got["info"][HAND, 0] == np.float32(1.0 / (7.0 * (1.0 / 7.0) ** 2)) == np.float32(7.0)
    report("pf hand: underflow", stats)


@pytest.mark.parametrize("th0,th1,want_d", [(6.25, 0.02, 0.02 - 6.25 + ref.TWO_PI), (0.01, 6.27, 6.27 - 0.01 - ref.TWO_PI)])
def test_hand_heading_change_across_the_yaw_wrap(amd, unit_sim, th0, th1, want_d):
    s, poses, scans, X, W, last, words = one_row(particles=2, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, resample_frac=0.0)
    last, poses = poses.copy(), poses.copy()
    last[0, 2], poses[0, 2] = th0, th1
    X = np.repeat(last[:, None, :], 2, axis=1)
    assert ref.odometry(last[0], poses[0])[2] == want_d
    stats = ref.new_stats()
    got = hand_call(amd, unit_sim, s, (poses, scans, X, W, last, words), ("wrap", th0), stats)
    assert np.all(np.abs(got["particles"][HAND, :, 2] - th1) < 1e-12), "the moved heading is not the true one"
    report("pf hand: the yaw wrap from %.2f" % th0, stats)


def test_hand_one_particle_is_the_estimate(amd, unit_sim):
    """P = 1: three rows of one particle share a k_pf_update workgroup of 16 groups; the estimate is the particle"""
    s, poses, scans, X, W, last, words = one_row(particles=1, resample_frac=2.0)
    stats = ref.new_stats()
    got = hand_call(amd, unit_sim, s, (poses, scans, X, W, last, words), "P = 1", stats)
    turn = got["pose"][:, 2] - got["particles"][:, 0, 2]          # (the estimate's heading lies in (-pi, pi], a particle's in [0, 2 pi])
    assert same_bits(got["pose"][:, :2], got["particles"][:, 0, :2]) and np.all(np.abs(np.remainder(turn + np.pi, ref.TWO_PI) - np.pi) < 1e-12)
    assert np.all(got["weights"] == 1.0) and np.all(got["info"][:, 0] == 1.0)
    assert same_bits(got["streams"][HAND], ref.words_of(ref.generator(words[0], 1 << 28)))
    report("pf hand: one particle", stats)
