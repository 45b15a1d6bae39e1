"""CPU checks of the observation encoder: the settings' validation, the NumPy model (tests/obs_encoder_ref.py)
against itself, and the host instantiation of f110_math.hpp's obs_* functions (tests/host_harness/obs_harness.hip) against
the model, bit for bit.  The GPU tests (tests/test_gpu_obs_encoder.py) hold the kernel to the same model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import obs_encoder_ref as ref
from f1tenth_gym_amd import ObsEncoder, _ffi
from f1tenth_gym_amd import obs_encoder as oe

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(beams=(5, 5)), dict(beams=(-1, 10)), dict(beams=(10, 5)), dict(beams=(0, 2000), num_beams=1080),      # a bad beam range
    dict(sectors=11, beams=(0, 10)), dict(sectors=1081, num_beams=1080), dict(sectors=-1),                      # K > W, K < 0
    dict(pool="max"), dict(features=("vx", "jerk")), dict(features=("vx", "vx")),                              # unknown pool / feature
    dict(frames=0), dict(frames=17), dict(frames=2.5),                                                          # F out of range
    dict(range_clip=0.0), dict(range_clip=-1.0), dict(range_clip=np.inf), dict(range_clip=np.nan),
    dict(range_scale=0.0), dict(range_scale=np.inf), dict(range_scale=np.nan),
    dict(scales={"vx": 0.0}), dict(scales={"vx": np.inf}), dict(scales={"steer": np.nan}), dict(scales={"jerk": 1.0}),
    dict(sectors=0, features=()),                                                                               # D = 0
    dict(sectors=1080, frames=8),                                                                               # F * D above the bound
])
def test_validation_refuses(kw):
    with pytest.raises(ValueError):
        ObsEncoder(**kw)


def test_dim_shape_order_and_struct():
    enc = ObsEncoder(sectors=108, pool="mean", beams=(100, 980), features=("collision", "vx", "heading_error", "steer"), frames=4,
                     range_clip=20.0, range_scale=10.0, scales={"vx": 8.0, "heading_error": -2.0})
    assert enc.features == ("vx", "steer", "collision", "heading_error")   # the fixed order, whatever order was asked for
    assert enc.dim == 112 and enc.shape(10) == (10, 4, 112) and enc.needs_track
    assert enc.feature_mask == 1 | 2 | 16 | 64
    sp = enc.spec(fill=True)
    assert (sp.beam_lo, sp.beam_hi, sp.sectors, sp.pool, sp.features, sp.frames, sp.flags) == (100, 980, 108, _ffi.OBS_POOL_MEAN, 83, 4, _ffi.OBS_FILL)
    assert (sp.range_clip, sp.range_scale) == (20.0, 10.0) and list(sp.feat_scale) == [8.0, 1.0, 1.0, 1.0, 1.0, 1.0, -2.0, 1.0]
    assert enc.spec().flags == 0 and ObsEncoder(beams=None).spec().beam_hi == 0
    assert C.sizeof(_ffi.ObsSpec) == 8 * 4 + 10 * 8
    assert not ObsEncoder(features=("vx",)).needs_track
    assert ObsEncoder.coerce(dict(sectors=4, frames=2)).shape(3) == (3, 2, 9) and ObsEncoder.coerce(enc) is enc
    with pytest.raises(TypeError):
        ObsEncoder.coerce(7)
    assert oe.FEATURES == ref.FEATURES
    with pytest.raises(ValueError):
        ObsEncoder(sectors=108).check_beams(61)
    assert ObsEncoder(sectors=0, features=("vx",)).dim == 1


def test_vec_env_argument_checks():
    """refusals that need no device: they are raised before a simulator is made"""
    from f1tenth_gym_amd import F110VecEnv
    with pytest.raises(ValueError, match="device_logic"):
        F110VecEnv(2, obs_encoder=ObsEncoder(sectors=8), map="example_map")
    with pytest.raises(ValueError, match="obs_encoder"):
        F110VecEnv(2, device_logic=True, obs_fields=("encoded",), map="example_map")
    with pytest.raises(ValueError, match="track"):
        F110VecEnv(2, device_logic=True, obs_encoder=ObsEncoder(sectors=8, features=("ds",)), map="example_map")


# ---- the model against itself ------------------------------------------------------------------------------------------------
def test_model_min_le_mean_and_center_identity():
    rng = np.random.default_rng(5)
    scans = rng.uniform(0.1, 40.0, size=(9, 1080))
    cols = np.zeros((9, 8))
    for K in (1, 7, 108, 1080):
        a = ref.new_frame(scans, cols, K, "min", None, (), 30.0, 30.0, {})
        b = ref.new_frame(scans, cols, K, "mean", None, (), 30.0, 30.0, {})
        assert a.shape == (9, K) and np.all(a <= b)
    for beams in (None, (13, 977)):
        lo, hi = beams or (0, 1080)
        c = ref.new_frame(scans, cols, hi - lo, "center", beams, (), 30.0, 30.0, {})
        assert np.array_equal(ref.bits(c), ref.bits((np.minimum(scans[:, lo:hi], 30.0) / 30.0).astype(np.float32)))
    assert ref.sector_bounds(61, 7, 3) == [(3, 11), (11, 20), (20, 29), (29, 37), (37, 46), (46, 55), (55, 64)]


def test_model_fill_then_shift():
    rng = np.random.default_rng(6)
    F, D, m = 4, 5, 3
    stack = rng.normal(size=(m, F, D)).astype(np.float32)
    first = rng.normal(size=(m, D)).astype(np.float32)
    s = ref.update_stack(stack, first, np.full(m, 7), True)
    assert all(np.array_equal(s[:, f], first) for f in range(F))
    frames = [first]
    for t in range(F - 1):
        frames.append(rng.normal(size=(m, D)).astype(np.float32))
        s = ref.update_stack(s, frames[-1], np.full(m, 2 + t), False)
    assert np.array_equal(s[:, 0], first) and all(np.array_equal(s[:, f], frames[f]) for f in range(F))
    # step_count 1 refills that agent only; step_count 0 shifts like any other agent
    new = rng.normal(size=(m, D)).astype(np.float32)
    s2 = ref.update_stack(s, new, np.array([0, 1, 2]), False)
    assert np.array_equal(s2[0, :-1], s[0, 1:]) and np.array_equal(s2[2, :-1], s[2, 1:]) and np.array_equal(s2[0, -1], new[0])
    assert all(np.array_equal(s2[1, f], new[1]) for f in range(F))


# ---- the host instantiation of f110_math.hpp's obs_* against the model ---------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "obs_harness.hip")
    lib = str(tmp_path_factory.mktemp("obs_harness") / "libobs_harness.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness_encode(hh, enc, scans, cols, step_count, stack, fill):
    B = scans.shape[1]
    lo, hi = enc.beams if enc.beams is not None else (0, B)
    scans, cols = np.ascontiguousarray(scans), np.ascontiguousarray(cols)
    sc = np.ascontiguousarray(step_count, dtype=np.int32)
    out = np.array(stack, dtype=np.float32, order="C")
    fs = np.array([enc.scales[f] for f in ref.FEATURES])
    D = hh.hh_obs_encode(lo, hi, enc.sectors, oe.POOLS[enc.pool], enc.feature_mask, fs.ctypes.data_as(_dp), C.c_double(enc.range_clip),
                         C.c_double(enc.range_scale), enc.frames, int(bool(fill)), scans.ctypes.data_as(_dp), B, cols.ctypes.data_as(_dp),
                         sc.ctypes.data_as(C.POINTER(C.c_int)), scans.shape[0], out.ctypes.data_as(C.c_void_p))
    assert D == enc.dim
    return out


GRID_SCALES = {"vx": 8.0, "steer": 0.4189, "yaw_rate": 3.2, "slip": -0.7, "collision": 1.0, "lateral": 1.5, "heading_error": 3.0, "ds": 0.2}


@needs_hipcc
def test_harness_matches_model_over_the_grid(hh):
    rng = np.random.default_rng(11)
    n = 0
    for B, beams, K, pool, F, fill in ref.unit_grid():
        feats = ref.FEATURES if n % 3 == 0 else (("vx", "steer", "yaw_rate", "slip", "collision") if n % 3 == 1 else ("steer", "ds"))
        enc = ObsEncoder(sectors=K, pool=pool, beams=beams, features=feats, frames=F, range_clip=30.0, range_scale=30.0 if n % 2 else 7.0,
                         scales=GRID_SCALES, num_beams=B)
        scans, cols, sc, stack = ref.random_inputs(rng, 7, B, F, enc.dim)
        want = ref.encode(enc, scans, cols, sc, stack, fill)
        got = harness_encode(hh, enc, scans, cols, sc, stack, fill)
        assert np.array_equal(ref.bits(got), ref.bits(want)), (B, beams, K, pool, F, fill)
        n += 1
    assert n > 300


@needs_hipcc
def test_harness_features_only_and_subnormal_results(hh):
    rng = np.random.default_rng(12)
    enc = ObsEncoder(sectors=0, features=ref.FEATURES, frames=3, scales=GRID_SCALES)
    scans, cols, sc, stack = ref.random_inputs(rng, 9, 61, 3, enc.dim)
    assert np.array_equal(ref.bits(harness_encode(hh, enc, scans, cols, sc, stack, False)), ref.bits(ref.encode(enc, scans, cols, sc, stack, False)))
    # results below float32's normal range: the float64 -> float32 conversion must round into the subnormals, not flush
    enc = ObsEncoder(sectors=61, pool="center", features=("vx",), frames=1)
    scans = np.full((2, 61), 1.0)
    scans[0, :] = 30.0 * 2.0 ** -130 * np.arange(1, 62)
    scans[1, :5] = [30.0 * 2.0 ** -149, 30.0 * 2.0 ** -150, 30.0 * 2.0 ** -151, 30.0 * 1.5 * 2.0 ** -149, 0.0]
    cols = np.zeros((2, 8))
    cols[:, 0] = [1e-41, -3e-45]
    got = harness_encode(hh, enc, scans, cols, np.array([2, 2]), np.zeros((2, 1, 62), np.float32), False)
    want = ref.encode(enc, scans, cols, np.array([2, 2]), np.zeros((2, 1, 62), np.float32), False)
    assert np.array_equal(ref.bits(got), ref.bits(want)) and np.count_nonzero((np.abs(want) < 1.1754944e-38) & (want != 0)) >= 19


# ---- the launch forms the host chooses: the staging rule's boundaries, F above 4, F * D at the cap ---------------------------------
def test_launch_form_grid_sits_on_both_sides_of_the_staging_rule():
    """the rule restated in the model file gives every row the side written next to it, so the grid cannot drift to one side;
    both kinds of row that ask for exactly 64 KiB are present, and the products an encoder cannot have are named"""
    rows = ref.launch_form_grid()
    unstaged = exact = 0
    seen_F, starts = set(), set()
    for row in rows:
        B, beams, K, pool, F, fill, feats, staged = row
        enc = ref.launch_form_encoder(ObsEncoder, row, GRID_SCALES)
        W = B if beams is None else beams[1] - beams[0]
        assert enc.dim == K + len(feats) and ref.planned_staged(W, F, enc.dim) is staged, row
        unstaged += not staged
        exact += staged and ref.planned_lds(W, F, enc.dim) == ref.LDS_BYTES
        seen_F.add(F)
        if not staged and beams is not None and beams[0] != 0:
            starts.add(pool)
    assert unstaged >= 6 and exact >= 4 and {5, 8, 16} <= seen_F and starts == {"min", "mean", "center"}
    windows = {(r[0] if r[1] is None else r[1][1] - r[1][0], r[4] * (r[2] + len(r[6]))) for r in rows}
    assert {(8190, 1), (8191, 1), (8192, 1), (4096, 8188), (4096, 8190), (4096, 8192)} <= windows
    # the rule itself at the boundary no encoder reaches: 8189 is the last staged product of a 4096-beam row, 8190 the first unstaged
    assert ref.planned_staged(4096, 1, 8189) and ref.planned_lds(4096, 1, 8189) == 65536 and not ref.planned_staged(4096, 1, 8190)
    assert ref.planned_staged(8190, 1, 1) and ref.planned_lds(8190, 1, 1) == 65536 and not ref.planned_staged(8191, 1, 1)
    assert all(8189 % F or 8189 // F > 4096 + 8 for F in range(1, 17))
    # every phase of the aligned store occurs among the staged everyday rows and among the unstaged ones
    for staged in (True, False):
        phases = {(i * r[4] * (r[2] + len(r[6]))) % 4 for r in rows if r[7] is staged for i in range(7)}
        assert phases == {0, 1, 2, 3}, staged


@needs_hipcc
def test_harness_matches_model_over_the_launch_form_grid(hh):
    rng = np.random.default_rng(13)
    for row in ref.launch_form_grid():
        B, beams, K, pool, F, fill, feats, staged = row
        enc = ref.launch_form_encoder(ObsEncoder, row, GRID_SCALES)
        scans, cols, sc, stack = ref.launch_form_inputs(rng, 7, row, enc.dim)
        assert set(sc) == {0, 1, 2} and np.isnan(scans).any() and np.isinf(scans).any()
        want = ref.encode(enc, scans, cols, sc, stack, fill)
        got = harness_encode(hh, enc, scans, cols, sc, stack, fill)
        assert np.array_equal(ref.bits(got), ref.bits(want)), row
