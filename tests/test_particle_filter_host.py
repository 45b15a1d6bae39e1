"""CPU checks of the particle filter: the settings' validation, the struct layout against the header, the host
instantiation of the pf_* functions (tests/host_harness/pf_harness.hip) against the Python model (tests/particle_filter_ref.py), bit
for bit in every output, and cases worked out by hand.  The GPU tests (tests/test_gpu_particle_filter.py) hold the kernels to the
same model."""
import ctypes as C
import itertools
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import particle_filter_ref as ref
import rollout_ref as rr
from f1tenth_gym_amd import ParticleFilter, _ffi
from f1tenth_gym_amd import particle_filter as pfm
from particle_filter_ref import same_bits

HERE = os.path.dirname(os.path.abspath(__file__))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
NAN, INF = float("nan"), float("inf")
KEYS = ("noise", "ancestors", "particles", "expected", "logw", "weights", "pose", "info", "last", "streams")


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(particles=0), dict(particles=1025), dict(particles=-1), dict(particles=2.5), dict(particles=True),
    dict(n_beams=0), dict(n_beams=129), dict(n_beams=1.0),
    dict(beam_first=-1), dict(beam_first=0.5), dict(beam_stride=0), dict(beam_stride=-3), dict(beam_stride=False),
    dict(beam_first=2 ** 31 - 2, n_beams=2, beam_stride=2),
    dict(sigma_x=-0.1), dict(sigma_y=-1.0), dict(sigma_theta=-1e-9), dict(sigma_x=INF), dict(sigma_y=NAN), dict(sigma_theta="wide"),
    dict(init_x=-0.1), dict(init_y=-0.1), dict(init_theta=-0.1), dict(init_x=INF), dict(init_theta=NAN),
    dict(sigma_hit=0.0), dict(sigma_hit=-1.0), dict(sigma_hit=INF), dict(sigma_hit=NAN),
    dict(clip=0.0), dict(clip=-1.0), dict(clip=-INF), dict(clip=NAN),
    dict(squash=0.0), dict(squash=-2.0), dict(squash=INF), dict(squash=NAN),
    dict(resample_frac=-0.1), dict(resample_frac=INF), dict(resample_frac=NAN), dict(resample_frac=True),
])
def test_particle_filter_validation_refuses(kw):
    with pytest.raises(ValueError):
        ParticleFilter(**kw)


def test_particle_filter_defaults_struct_and_coerce():
    p = ParticleFilter()
    assert (p.particles, p.n_beams, p.beam_first, p.beam_stride, p.last_beam) == (256, 54, 0, 20, 1060)
    p.check_beams(1080)
    with pytest.raises(ValueError):
        p.check_beams(1060)
    q = ParticleFilter(particles=1024, n_beams=128, beam_first=7, beam_stride=8, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, init_x=0.0, init_y=0.0,
                       init_theta=0.0, sigma_hit=1e-3, clip=INF, squash=1.0, resample_frac=0.0)
    sp = q.spec()
    assert (sp.particles, sp.n_beams, sp.beam_first, sp.beam_stride, sp.sigma_hit, sp.clip, sp.squash, sp.resample_frac) == (1024, 128, 7, 8, 1e-3, INF, 1.0, 0.0)
    assert q.cloud_shape(3) == (3, 1024, 3) and np.array_equal(q.beams, 7 + 8 * np.arange(128))
    S = _ffi.PfSpec
    assert C.sizeof(S) == 96 == 4 * 4 + 10 * 8
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12] + [16 + 8 * i for i in range(10)]
    assert ParticleFilter.coerce(dict(particles=3)).particles == 3 and ParticleFilter.coerce(p) is p
    assert ParticleFilter(**q.settings()).settings() == q.settings() and repr(q).startswith("ParticleFilter(particles=1024, ")
    with pytest.raises(TypeError):
        ParticleFilter.coerce(7)
    assert pfm.split_filter(None) is None and pfm.split_filter({1: p}) == (1, p) and pfm.split_filter({0: dict(particles=2)})[1].particles == 2
    for bad in ({0: p, 1: q}, {}, p, {"0": p}):
        with pytest.raises(ValueError):
            pfm.split_filter(bad)


def test_struct_and_constants_match_the_header():
    """the struct's fields in the header's order and types, and the limits, read from include/f110.h"""
    with open(os.path.join(os.path.dirname(HERE), "include", "f110.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct f110_pf \{(.*?)\} f110_pf;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"(int32_t|double)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    mirror = _ffi.PfSpec._fields_
    assert [n for _, n in fields] == [n for n, _ in mirror] == list(ref.SPEC_INTS + ref.SPEC_FLOATS)
    assert all(ct is ctype[t] for (t, _), (_, ct) in zip(fields, mirror))
    enums = dict(re.findall(r"(F110_PF_[A-Z_]+) = (\d+)", src))
    assert int(enums["F110_PF_MAX_P"]) == _ffi.PF_MAX_P == pfm.MAX_P == 1024
    assert int(enums["F110_PF_MAX_BEAMS"]) == _ffi.PF_MAX_BEAMS == pfm.MAX_BEAMS == 128
    for name in ("f110_pf_set", "f110_pf_device", "f110_pf_get", "f110_pf_put", "f110_pf_batch"):
        assert name in _ffi.PROTOTYPES and re.search(r"\bint %s\(" % name, src), name


# ---- the host instantiation ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "pf_harness.hip")
    lib = str(tmp_path_factory.mktemp("pf_harness") / "libpf_harness.so")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness(hh, s, so, poses, scans, particles, weights, last, streams, fresh=None, lidar_dist=0.0):
    """the host instantiation's call for settings s (particle_filter_ref.settings): the model's dict (without near and ess_gap)"""
    c = so.cfg
    poses, scans = np.ascontiguousarray(poses, dtype=np.float64), np.ascontiguousarray(scans, dtype=np.float64)
    m, P, Bp = poses.shape[0], s["particles"], s["n_beams"]
    ints = np.array([s[k] for k in ref.SPEC_INTS], dtype=np.intc)
    dbl = np.array([s[k] for k in ref.SPEC_FLOATS], dtype=np.float64)
    o = dict(particles=np.array(particles, dtype=np.float64), weights=np.array(weights, dtype=np.float64), last=np.array(last, dtype=np.float64),
             streams=np.array(streams, dtype=np.uint64), pose=np.zeros((m, 3)), info=np.zeros((m, 4), dtype=np.float32), noise=np.zeros((m, P, 3)),
             ancestors=np.zeros((m, P), dtype=np.int32), expected=np.zeros((m, P, Bp)), logw=np.zeros((m, P)))
    fr = None if fresh is None else np.ascontiguousarray(fresh, dtype=np.intc)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    hh.hh_pf(p(so.dt), C.c_int(c.height), C.c_int(c.width), C.c_double(c.resolution), C.c_double(c.orig_x), C.c_double(c.orig_y), C.c_double(c.orig_c),
             C.c_double(c.orig_s), p(so.sines), p(so.cosines), C.c_int(c.theta_dis), C.c_int(c.num_beams), C.c_double(c.fov), C.c_double(c.eps),
             C.c_double(c.max_range), p(ints), p(dbl), C.c_double(lidar_dist), p(poses), p(scans), None if fr is None else p(fr), C.c_int(m),
             p(o["particles"]), p(o["weights"]), p(o["last"]), p(o["streams"]), p(o["pose"]), p(o["info"]), p(o["noise"]), p(o["ancestors"]),
             p(o["expected"]), p(o["logw"]))
    return o


def assert_same(got, want, what):
    for key in KEYS:
        assert same_bits(got[key], want[key].astype(got[key].dtype)), "%s: %s" % (what, key)


@needs_hipcc
@pytest.mark.parametrize("map_name", rr.GRID_MAPS)
@pytest.mark.parametrize("P", [1, 2, 7, 65])
@pytest.mark.parametrize("Bp", [1, 7, 65])
def test_host_instantiation_is_the_model(hh, map_name, P, Bp):
    """two calls in a row per (stride, resample_frac): the first with a fresh row among the three, the second without one, on the
    state the first one left; every output bit for bit"""
    so, poses, scans, X0, W0, last0, words0 = ref.rows_for(map_name, P, seed=P + Bp)
    for stride in (1, 18):
        if 3 + (Bp - 1) * stride >= ref.NUM_BEAMS:
            stride = ref.largest_stride(ref.settings(n_beams=Bp))
        for frac in (0.0, 0.5, 2.0):
            s = ref.settings(particles=P, n_beams=Bp, beam_stride=stride, resample_frac=frac)
            X, W, last, words = X0, W0, last0, words0
            for call, fresh in enumerate((np.array([3, 0, 5]), None)):
                lidar = 0.275 * call
                want = ref.call(s, so, poses, scans, X, W, last, words, fresh, lidar)
                got = harness(hh, s, so, poses, scans, X, W, last, words, fresh, lidar)
                assert_same(got, want, (map_name, P, Bp, stride, frac, call))
                if frac == 0.0:                       # never resampled; always (ESS <= P < 2 P) unless the row is fresh
                    assert np.all(want["info"][:, 3] == 0.0)
                if frac == 2.0:
                    assert np.array_equal(want["info"][:, 3], [1.0, 0.0, 1.0] if call == 0 else [1.0, 1.0, 1.0])
                X, W, last, words = got["particles"], got["weights"], got["last"], got["streams"]
                poses = poses + np.column_stack([0.03 * np.cos(poses[:, 2]), 0.03 * np.sin(poses[:, 2]), np.zeros(3)])


# ---- cases worked out by hand --------------------------------------------------------------------------------------------------------
def one_row(map_name="example_map", **kw):
    s = ref.settings(**kw)
    so, poses, scans, X, W, last, words = ref.rows_for(map_name, s["particles"], m=1, seed=77)
    return s, so, poses, scans, X, W, last, words


@needs_hipcc
def test_one_particle_is_the_estimate_and_the_stream_moves_on(hh):
    s, so, poses, scans, X, W, last, words = one_row(particles=1, resample_frac=2.0)
    for call in (harness(hh, s, so, poses, scans, X, W, last, words), ref.call(s, so, poses, scans, X, W, last, words)):
        assert call["pose"][0, 0] == call["particles"][0, 0, 0] and call["pose"][0, 1] == call["particles"][0, 0, 1]
        assert abs(call["pose"][0, 2] - call["particles"][0, 0, 2]) < 1e-15 and call["weights"][0, 0] == 1.0 and call["info"][0, 0] == 1.0
        assert same_bits(call["streams"], ref.words_of(ref.generator(words[0], 1 << 28))[None])
    s64 = ref.settings(particles=65)
    so, poses, scans, X, W, last, words = ref.rows_for("example_map", 65, m=1, seed=78)
    assert same_bits(harness(hh, s64, so, poses, scans, X, W, last, words)["streams"], ref.words_of(ref.generator(words[0], 1 << 28))[None])


@needs_hipcc
def test_without_noise_the_estimate_follows_the_true_pose(hh):
    """every sigma 0 and a cloud on the true pose: the odometry delta alone moves it, the estimate stays on the car"""
    s = ref.settings(particles=7, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, init_x=0.0, init_y=0.0, init_theta=0.0, resample_frac=0.0)
    so, poses, scans, _, W, _, words = ref.rows_for("example_map", 7, m=1, seed=79)
    X, last = np.repeat(poses[:, None, :], 7, axis=1), poses.copy()
    for step in range(20):
        poses = poses + np.array([[0.05 * math.cos(poses[0, 2]), 0.05 * math.sin(poses[0, 2]), 0.03]])
        poses[0, 2] = ref.wrap(poses[0, 2])
        got = harness(hh, s, so, poses, scans, X, W, last, words)
        assert np.max(np.abs(got["pose"][0, :2] - poses[0, :2])) < 1e-12 and abs(math.remainder(got["pose"][0, 2] - poses[0, 2], ref.TWO_PI)) < 1e-12
        assert got["info"][0, 2] < 1e-12
        X, W, last, words = got["particles"], got["weights"], got["last"], got["streams"]


@needs_hipcc
def test_a_particle_outside_the_map(hh):
    s, so, poses, scans, X, W, last, words = one_row(particles=2, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, resample_frac=0.0)
    X[0, 1] = (-500.0, 300.0, 1.0)
    last = poses.copy()
    got, want = harness(hh, s, so, poses, scans, X, W, last, words), ref.call(s, so, poses, scans, X, W, last, words)
    assert_same(got, want, "outside")
    assert np.all(np.isfinite(got["expected"])) and np.all(np.isfinite(got["pose"])) and got["weights"][0, 1] < got["weights"][0, 0]


@needs_hipcc
def test_a_nan_scan_value_takes_the_clip_or_counts_as_nothing(hh):
    for clip in (2.0, INF):
        s, so, poses, scans, X, W, last, words = one_row(particles=2, n_beams=3, clip=clip, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, resample_frac=0.0)
        last = poses.copy()
        clean = harness(hh, s, so, poses, scans, X, W, last, words)
        scans = scans.copy()
        b = ref.beams(s)[1]
        scans[0, b] = NAN
        got, want = harness(hh, s, so, poses, scans, X, W, last, words), ref.call(s, so, poses, scans, X, W, last, words)
        assert_same(got, want, ("nan", clip))
        assert np.all(np.isfinite(got["logw"]))
        for p in range(2):
            terms = [min(((clean_z - r) / s["sigma_hit"]) ** 2, clip * clip) for clean_z, r in zip(scans[0, ref.beams(s)], got["expected"][0, p])]
            terms[1] = clip * clip if clip != INF else 0.0
            assert got["logw"][0, p] == -(0.5 / s["squash"]) * ((0.0 + terms[0]) + terms[1] + terms[2])
        assert np.array_equal(clean["expected"], got["expected"])


@needs_hipcc
def test_one_surviving_weight_is_every_ancestor(hh):
    s, so, poses, scans, X, W, last, words = one_row(particles=7, resample_frac=0.5)
    W = np.zeros((1, 7))
    W[0, 4] = 1.0
    got, want = harness(hh, s, so, poses, scans, X, W, last, words), ref.call(s, so, poses, scans, X, W, last, words)
    assert_same(got, want, "survivor")
    assert np.all(got["ancestors"] == 4) and got["info"][0, 3] == 1.0


@needs_hipcc
def test_underflow_falls_back_to_uniform_weights(hh):
    """a scan far from every expectation without truncation: exp underflows for all but the best particle when the prior puts no
    weight on it, eta is 0 and the weights become uniform"""
    s, so, poses, scans, X, W, last, words = one_row(particles=7, clip=INF, sigma_hit=1e-3, squash=1e-3, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0,
                                                     resample_frac=0.0)
    last = poses.copy()
    probe = ref.call(s, so, poses, scans, X, W, last, words)
    best = int(np.argmax(probe["logw"][0]))
    W = np.full((1, 7), 1.0 / 6.0)
    W[0, best] = 0.0
    got, want = harness(hh, s, so, poses, scans, X, W, last, words), ref.call(s, so, poses, scans, X, W, last, words)
    assert_same(got, want, "underflow")
    assert np.all(got["weights"] == 1.0 / 7.0) and got["info"][0, 0] == np.float32(1.0 / (7.0 * (1.0 / 7.0) ** 2))


@needs_hipcc
def test_heading_change_across_the_yaw_wrap(hh):
    s, so, poses, scans, X, W, last, words = one_row(particles=2, sigma_x=0.0, sigma_y=0.0, sigma_theta=0.0, resample_frac=0.0)
    for th0, th1, want_d in ((6.25, 0.02, 0.02 - 6.25 + ref.TWO_PI), (0.01, 6.27, 6.27 - 0.01 - ref.TWO_PI)):
        last, poses = poses.copy(), poses.copy()
        last[0, 2], poses[0, 2] = th0, th1
        X = np.repeat(last[:, None, :], 2, axis=1)
        got, want = harness(hh, s, so, poses, scans, X, W, last, words), ref.call(s, so, poses, scans, X, W, last, words)
        assert_same(got, want, ("wrap", th0))
        assert ref.odometry(last[0], poses[0])[2] == want_d and abs(got["particles"][0, 0, 2] - th1) < 1e-12


def test_the_model_leaves_nothing_out_on_the_gpu_tests_unit_grid():
    """the GPU tests leave out a row whose ESS lies within 1e-9 * P of the threshold and a slot within 1e-9 * C of a cumulative
    boundary: for the seeds of their unit grid the model itself has neither"""
    cases = [(mp, P, Bp, big, q) for mp in rr.GRID_MAPS for P in ref.UNIT_P for q, (Bp, big) in enumerate(itertools.product(ref.UNIT_B, (False, True)))]
    cases += [(mp, 1024, Bp, big, q) for mp in rr.GRID_MAPS for Bp in (7, 128) for q, big in enumerate((False, True))]
    rows = 0
    for mp, P, Bp, big, q in cases:
        s, (poses, scans, X, W, last, words, fresh) = ref.unit_case(mp, P, Bp, big, q)
        assert ref.beams(s)[-1] < ref.NUM_BEAMS and (not big or ref.beams(s)[-1] + s["n_beams"] - 1 >= ref.NUM_BEAMS or Bp == 1)
        for n in np.flatnonzero(fresh != 0):
            u = float(np.random.Generator(ref.generator(words[n], 0)).random())
            res, anc, ess, near = ref.resampling(s, W[n], u)
            assert abs(ess - s["resample_frac"] * P) > 1e-9 * P and np.all(near > 1e-9), (mp, P, Bp, big, q, n)
            rows += 1
    assert rows == 2 * len(cases)


def test_the_model_leaves_nothing_out_on_the_gpu_tests_edge_grid():
    """the same for tests/test_gpu_particle_filter_edges.py's grid (particle_filter_ref.edge_cases: P on both sides of every bound
    of k_pf_update's lane grouping), whose P reach every grouping"""
    cases = ref.edge_cases()
    assert {ref.group_lanes(P) for P in ref.EDGE_P} == {16, 32, 64, 128, 256} and len(cases) == 2 * len(ref.EDGE_P) * 4
    assert [ref.group_lanes(P) for P in (1, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 1024)] == [16, 16, 32, 32, 64, 64, 128, 128, 256, 256, 256, 256]
    rows, outcomes = 0, {}
    for mp, P, Bp, big, q in cases:
        s, (poses, scans, X, W, last, words, fresh) = ref.unit_case(mp, P, Bp, big, q)
        assert ref.beams(s)[-1] < ref.NUM_BEAMS and (not big or ref.beams(s)[-1] + s["n_beams"] - 1 >= ref.NUM_BEAMS)
        for n in np.flatnonzero(fresh != 0):
            u = float(np.random.Generator(ref.generator(words[n], 0)).random())
            res, anc, ess, near = ref.resampling(s, W[n], u)
            assert abs(ess - s["resample_frac"] * P) > 1e-9 * P and np.all(near > 1e-9), (mp, P, Bp, big, q, n)
            outcomes.setdefault((mp, P), set()).add(res)
            rows += 1
    assert rows == 128 and all(v == {False, True} for v in outcomes.values()), "both resampling outcomes per P"


# ---- the sanitizers --------------------------------------------------------------------------------------------------------------------
@needs_hipcc
def test_harness_program_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program (its own main) under the address and undefined-behaviour sanitizers: host code only"""
    src = os.path.join(HERE, "host_harness", "pf_harness.hip")
    exe = str(tmp_path / "pf_harness_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DPF_HARNESS_MAIN",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout.startswith("pf harness: ok"), proc.stdout
