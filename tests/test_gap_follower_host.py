"""CPU checks of the follow-the-gap controller: the settings' validation, the NumPy model
(tests/gap_follower_ref.py) on rows worked out by hand, the host instantiation of f110_math.hpp's gap_* functions
(tests/host_harness/gap_harness.hip) against the model bit for bit, and the model driving the oracle's simulator around
example_map without a collision.  The GPU tests (tests/test_gpu_gap_follower.py) hold the kernel to the same model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import gap_follower_ref as ref
from _util import bench_start_poses, oracle_map_dt
from f1tenth_gym_amd import GapFollower, _ffi
from f1tenth_gym_amd import gap_follower as gf

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
FLOATS = ("range_clip", "bubble_radius", "gap_threshold", "steer_gain", "steer_max", "v_lo", "v_hi", "d_ref", "steer_slow", "v_turn", "v_blocked")


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(beams=(5, 5)), dict(beams=(-1, 10)), dict(beams=(10, 5)), dict(beams=(0, 2000), num_beams=1080), dict(beams=(0, 5000)),   # a bad window
    dict(smooth=4), dict(smooth=0), dict(smooth=65), dict(smooth=-3), dict(smooth=2.5), dict(smooth=7, beams=(10, 15)),            # S
    dict(smooth=63, num_beams=61, beams=(0, 0)), dict(smooth=63, num_beams=90),                                                     # S > W
    dict(target="left"), dict(target=2),
    dict(range_clip=0.0), dict(range_clip=-1.0), dict(range_clip=np.inf), dict(range_clip=np.nan),
    dict(d_ref=0.0), dict(d_ref=np.nan), dict(bubble_radius=-0.1), dict(bubble_radius=np.inf), dict(gap_threshold=-1.0),
    dict(gap_threshold=np.nan), dict(steer_gain=np.inf), dict(steer_max=-0.1), dict(steer_max=np.nan), dict(steer_slow=-0.1),
    dict(v_lo=5.0, v_hi=4.0), dict(v_lo=np.nan), dict(v_hi=np.inf), dict(v_turn=np.nan), dict(v_blocked=np.inf),
])
def test_validation_refuses(kw):
    with pytest.raises(ValueError):
        GapFollower(**kw)


def test_defaults_struct_and_coerce():
    g = GapFollower()
    assert g.window(1080) == (180, 900) and g.window(61) == (10, 51) and GapFollower(beams=(0, 0)).window(1080) == (0, 1080)
    sp = g.spec(1080)
    assert (sp.beam_lo, sp.beam_hi, sp.smooth, sp.target) == (180, 900, 5, _ffi.GAP_TARGET_CENTER == 0 and 0)
    assert [getattr(sp, k) for k in FLOATS] == [10.0, 0.6, 1.5, 1.0, 0.4189, 1.5, 4.0, 8.0, 0.2, 2.5, 0.5]
    assert GapFollower(target="furthest").spec(1080).target == _ffi.GAP_TARGET_FURTHEST == 1
    assert C.sizeof(_ffi.GapFollowerSpec) == 4 * 4 + 11 * 8 and _ffi.STEP_SCRIPTED == 64
    assert GapFollower.coerce(dict(smooth=7)).smooth == 7 and GapFollower.coerce(g) is g
    assert GapFollower(**g.settings()).settings() == g.settings()
    with pytest.raises(TypeError):
        GapFollower.coerce(7)
    for k, v in ref.DEFAULTS.items():      # the model's defaults are the class's
        assert g.settings()[k] == v, k


def test_scripted_argument_forms():
    a, c = gf.coerce_scripted({1: dict(smooth=7)}, 3, 2)
    assert a.tolist() == [[-1, 0]] * 3 and len(c) == 1 and c[0].smooth == 7
    a, c = gf.coerce_scripted({0: GapFollower(), 2: GapFollower(target="furthest")}, 2, 3)
    assert a.tolist() == [[0, -1, 1]] * 2 and c[1].target == "furthest"
    a, c = gf.coerce_scripted(([[0, -1], [1, 1]], [GapFollower(), dict(smooth=3)]), 2, 2)
    assert a.dtype == np.int32 and a.tolist() == [[0, -1], [1, 1]] and c[1].smooth == 3
    for bad in ({2: GapFollower()}, {-1: GapFollower()}, ([[0, 2], [0, 0]], [GapFollower(), GapFollower()]), ([[0, -2], [0, 0]], [GapFollower()]),
                ([[0, 0]], [GapFollower()]), ([[0, 0], [0, 0]], []), ([[0, 0], [0, 0]], [GapFollower()] * 9)):
        with pytest.raises(ValueError):
            gf.coerce_scripted(bad, 2, 2)
    with pytest.raises(TypeError):
        gf.coerce_scripted(5, 2, 2)


def test_vec_env_needs_device_logic():
    """raised before a simulator is made; the message names the call other loops use"""
    from f1tenth_gym_amd import F110VecEnv
    with pytest.raises(ValueError, match="follow_gap_device"):
        F110VecEnv(2, scripted={1: GapFollower()}, map="example_map")


# ---- the model on rows worked out by hand ---------------------------------------------------------------------------------------
def _expected_action(s, row, info):
    """the action that belongs to hand-derived integers, by the rule's last step alone"""
    c, half, g0, g1, t = info
    if t < 0:
        return 0.0, s["v_blocked"]
    B = len(row)
    angle = -4.7 / 2. + (4.7 / (B - 1)) * t
    steer = min(max(s["steer_gain"] * angle, -s["steer_max"]), s["steer_max"])
    rt = min(row[t], s["range_clip"])
    speed = s["v_lo"] + (s["v_hi"] - s["v_lo"]) * min(rt / s["d_ref"], 1.0)
    return steer, (min(speed, s["v_turn"]) if abs(steer) > s["steer_slow"] else speed)


@pytest.mark.parametrize("case", ref.hand_rows(), ids=lambda c: c[0])
def test_model_on_hand_built_rows(case):
    name, s, row, info = case
    act, got = ref.follow_row(s, row)
    assert tuple(got) == info, name
    assert act == _expected_action(s, row, info), name


def test_model_smoothing_and_step_count():
    v = np.array([[1.0, 2.0, 4.0, 8.0, 16.0, 32.0]])
    assert ref.smooth_rows(v, 3).tolist() == [[1.5, 7.0 / 3.0, 14.0 / 3.0, 28.0 / 3.0, 56.0 / 3.0, 24.0]]
    assert ref.smooth_rows(v, 1).tolist() == v.tolist()
    assert ref.smooth_rows(v, 5)[0, 0] == 7.0 / 3.0 and ref.smooth_rows(v, 5)[0, 2] == 31.0 / 5.0
    # ascending adds, each window on its own: (1e16 + 1) + 1 differs from 1e16 + (1 + 1)
    w = np.array([[1e16, 1.0, 1.0, -1e16, 0.0]])
    assert ref.smooth_rows(w, 3)[0, 1] == ((0.0 + 1e16) + 1.0 + 1.0) / 3.0 and ref.smooth_rows(w, 3)[0, 2] == ((0.0 + 1.0) + 1.0 - 1e16) / 3.0
    assert ref.longest_run([0, 1, 1, 0, 1, 1, 0]) == (1, 3) and ref.longest_run([1, 0, 1, 1]) == (2, 4) and ref.longest_run([0, 0]) is None
    rows = np.full((3, 61), 5.0)
    act, info = ref.follow(ref.settings(), rows, np.array([0, 1, 7]))
    assert act[0].tolist() == [0.0, 0.0] and info[0].tolist() == [-1] * 5 and np.array_equal(act[1], act[2]) and act[1, 1] > 0


# ---- the host instantiation of f110_math.hpp's gap_* against the model ---------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "gap_harness.hip")
    lib = str(tmp_path_factory.mktemp("gap_harness") / "libgap_harness.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness_follow(hh, s, scans, step_count=None, fov=ref.FOV):
    scans = np.ascontiguousarray(scans, dtype=np.float64)
    m, B = scans.shape
    lo, hi = ref.window(s, B)
    d = np.array([s[k] for k in FLOATS], dtype=np.float64)
    act, info = np.zeros((m, 2)), np.zeros((m, 5), dtype=np.int32)
    sc = None if step_count is None else np.ascontiguousarray(step_count, dtype=np.int32)
    hh.hh_gap_follow(lo, hi, int(s["smooth"]), 0 if s["target"] == "center" else 1, d.ctypes.data_as(_dp), C.c_double(fov),
                     scans.ctypes.data_as(_dp), B, None if sc is None else sc.ctypes.data_as(_ip), m, act.ctypes.data_as(_dp),
                     info.ctypes.data_as(_ip))
    return act, info


def same(got, want, what):
    assert np.array_equal(got[1], want[1]), "%s: the integers differ\n%r\n%r" % (what, got[1], want[1])
    assert np.array_equal(ref.bits(got[0]), ref.bits(want[0])), "%s: the actions differ\n%r\n%r" % (what, got[0], want[0])


@needs_hipcc
def test_harness_matches_model_over_the_grid(hh):
    rng = np.random.default_rng(21)
    orc_rows = {B: ref.oracle_scans(B) for B in ref.GRID_B}
    n = free = 0
    for k, (B, beams, S, target) in enumerate(ref.unit_grid()):
        s = ref.settings(beams=beams, smooth=S, target=target)
        if k % 3 == 1:
            s.update(range_clip=6.0, bubble_radius=0.3, gap_threshold=0.8, steer_gain=0.7, v_hi=6.5, d_ref=5.0, steer_slow=0.1)
        rows = np.concatenate([ref.random_rows(rng, 8, B), orc_rows[B][(k % 3)::3]])
        sc = (np.arange(len(rows)) % 5 != 3).astype(np.int32) * (1 + np.arange(len(rows)))
        want = ref.follow(s, rows, sc)
        same(harness_follow(hh, s, rows, sc), want, "B=%d beams=%r S=%d %s" % (B, beams, S, target))
        n += len(rows)
        free += int(np.sum(want[1][:, 4] >= 0))
    assert n >= 300 and free >= n // 3, (n, free)


@needs_hipcc
def test_harness_on_hand_built_rows(hh):
    for name, s, row, info in ref.hand_rows():
        got = harness_follow(hh, s, row[None, :])
        assert tuple(got[1][0]) == info, name
        same(got, ref.follow(s, row[None, :]), name)


@needs_hipcc
def test_run_merge_is_the_longest_run_however_the_beams_are_cut(hh):
    rng = np.random.default_rng(22)
    for trial in range(400):
        n = int(rng.integers(1, 400))
        free = (rng.random(n) < rng.choice([0.1, 0.5, 0.9, 1.0])).astype(np.uint8)
        if trial % 7 == 0:
            free[:] = trial % 2
        cuts = [0]
        while cuts[-1] < n:
            cuts.append(min(n, cuts[-1] + int(rng.integers(0, 65))))    # chunks of 0..64 beams, empty ones among them
        cuts = np.array(cuts[1:-1], dtype=np.int32)
        out = np.zeros(4, dtype=np.int32)
        hh.hh_gap_runs(free.ctypes.data_as(C.POINTER(C.c_ubyte)), n, cuts.ctypes.data_as(_ip), len(cuts), out.ctypes.data_as(_ip))
        run = ref.longest_run(free)
        want = (0, None) if run is None else (run[1] - run[0], run[0])
        for best, start in (out[:2], out[2:]):
            assert best == want[0] and (want[1] is None or start == want[1]), (trial, n, cuts.tolist(), out.tolist(), want)


# ---- the model drives the oracle's simulator -------------------------------------------------------------------------------------
def drive(E, A, steps, target="center"):
    """every car of E envs x A cars driven by the model with the default settings, noise off; -> (collisions seen, metres driven)"""
    from oracle import orc
    dt, res, origin = oracle_map_dt("example_map")
    o = orc.SimOracle(E, A)
    o.set_map_dt(dt, res, origin)
    o.reset(bench_start_poses(E, A))
    o.step(np.zeros((E * A, 2)))                 # the zero-action step of the reference's reset()
    s = ref.settings(target=target)
    hits, dist = 0, np.zeros(E * A)
    for t in range(steps):
        act, _ = ref.follow(s, o.scans)
        o.step(act)
        hits += int(np.sum(o.collisions != 0)) + int(np.sum(o.in_collision != 0))
        dist += np.abs(o.state[:, 3]) * 0.01
    return hits, dist


def test_model_drives_single_cars_without_a_collision():
    hits, dist = drive(8, 1, 2500)
    assert hits == 0, "%d collision flags" % hits
    assert dist.min() > 40.0, dist          # they drive: 2500 steps at 1.5 .. 4 m/s


def test_model_drives_two_scripted_cars_per_env_without_a_collision():
    hits, dist = drive(4, 2, 1500)
    assert hits == 0, "%d collision flags" % hits
    assert dist.min() > 20.0, dist
