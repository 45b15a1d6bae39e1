"""CPU checks of the opponent term: the settings' validation, the struct layout against the header, the host
instantiation of the opp_* functions (tests/host_harness/opp_harness.hip) against the Python model (tests/opponents_ref.py) and
cases worked out by hand.  The GPU tests (tests/test_gpu_opponents.py) hold the kernels to the same model."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import mppi_ref as mr
import opponents_ref as ref
import rollout_ref as rr
from f1tenth_gym_amd import Opponents, _ffi
from f1tenth_gym_amd import opponents as opm
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
NAN, INF = float("nan"), float("inf")


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ---- validation and layout ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(mode="ctra"), dict(mode=0), dict(mode=None), dict(mode="CV"),
    dict(radius=0.0), dict(radius=-0.1), dict(radius=INF), dict(radius=NAN), dict(radius="wide"), dict(radius=True),
    dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=NAN), dict(max_range=None), dict(max_range=False),
])
def test_opponents_validation_refuses(kw):
    with pytest.raises(ValueError):
        Opponents(**kw)


@pytest.mark.parametrize("w", [(-1.0, 0.0, 0.0), (0.0, -1e-9, 0.0), (INF, 0.0, 0.0), (0.0, NAN, 0.0), (0.0, 0.0, INF), (0.0, 0.0, NAN), ("a", 0.0, 0.0)])
def test_weights_validation_refuses(w):
    with pytest.raises(ValueError):
        opm.check_weights(*w)


def test_defaults_struct_and_coerce():
    p = Opponents()
    assert (p.mode, p.radius, p.max_range, p.needs_track) == ("cv", 0.4, INF, False)
    q = Opponents(mode="track", radius=1e-3, max_range=12.5)
    sp = q.spec()
    assert (sp.mode, sp.radius, sp.max_range, q.needs_track) == (_ffi.OPP_TRACK, 1e-3, 12.5, True)
    S = _ffi.OpponentsSpec
    assert C.sizeof(S) == 24 and [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 16]
    assert Opponents.coerce(dict(radius=0.3)).radius == 0.3 and Opponents.coerce(p) is p
    assert Opponents(**q.settings()).settings() == q.settings()
    with pytest.raises(TypeError):
        Opponents.coerce(3)
    assert opm.check_weights(1, 2, -3) == (1.0, 2.0, -3.0)
    got = opm.split_mppi_opponents(dict(opponents=dict(mode="track"), w_hit=2.0, near_ref=1.0))
    assert got[0].mode == "track" and got[1:] == (2.0, 0.0, 1.0) and opm.split_mppi_opponents(None) is None
    for bad in (7, dict(w_hit=1.0), dict(opponents=p, w_miss=1.0)):
        with pytest.raises(TypeError):
            opm.split_mppi_opponents(bad)


def test_struct_and_constants_match_the_header():
    """the struct's fields in the header's order and types, the enum values and the four entry points, read from include/f110.h"""
    with open(os.path.join(os.path.dirname(HERE), "include", "f110.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct f110_opponents \{(.*?)\} f110_opponents;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"(int32_t|double)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    mirror = _ffi.OpponentsSpec._fields_
    assert [n for _, n in fields] == [n for n, _ in mirror] == ["mode", "pad_", "radius", "max_range"]
    assert all(ct is ctype[t] for (t, _), (_, ct) in zip(fields, mirror))
    enums = dict(re.findall(r"(F110_OPP_[A-Z_]+) = (\d+)", src))
    assert (int(enums["F110_OPP_CV"]), int(enums["F110_OPP_TRACK"]), int(enums["F110_OPP_MAX"])) == (_ffi.OPP_CV, _ffi.OPP_TRACK, _ffi.OPP_MAX) == (0, 1, 31)
    assert opm.MODES == {"cv": 0, "track": 1} and opm.MAX_OPPONENTS == 31
    for name in ("f110_rollout_opp_device", "f110_rollout_opp_batch", "f110_mppi_set_opponents", "f110_mppi_opp_batch"):
        assert name in _ffi.PROTOTYPES and re.search(r"\bint %s\(" % name, src), name
    # the rollout's and the planner's "Not offered" lists no longer name them
    roll = src[src.index("---- rollout"):src.index("typedef struct f110_rollout")]
    plan = src[src.index("---- MPPI planner"):src.index("typedef struct f110_mppi")]
    for text in (roll, plan):
        assert not re.search(r"[,:] opponents,", text[text.index("Not offered"):])


# ---- the host instantiation -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "opp_harness.hip")
    lib = str(tmp_path_factory.mktemp("opp_harness") / "libopp_harness.so")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def _map_args(so, track):
    c = so.cfg
    cols = None if track is None else ref.track_cols(track)
    return cols, (so.dt.ctypes.data_as(_dp), c.height, c.width, C.c_double(c.resolution), C.c_double(c.orig_x), C.c_double(c.orig_y),
                  C.c_double(c.orig_c), C.c_double(c.orig_s), None if cols is None else cols.ctypes.data_as(_dp),
                  0 if track is None else track.num_segments, int(track is not None and track.closed), C.c_double(0.0 if track is None else track.length))


def _opp_args(s, w=(0.0, 0.0, 0.0)):
    oi = np.array([opm.MODES[s["mode"]]], dtype=np.int32)
    od = np.array([s["radius"], s["max_range"], w[0], w[1], w[2]], dtype=np.float64)
    return oi, od


def h_rollout(hh, s, so, start, params, actions, per_agent, opp, K, H, repeat, margin, integrator, track=None, lidar_dist=0.0):
    start, params, actions = (np.ascontiguousarray(a, dtype=np.float64) for a in (start, params, actions))
    opp = np.ascontiguousarray(opp, dtype=np.float64)
    m, Ao = start.shape[0], opp.shape[1]
    cols, margs = _map_args(so, track)
    ri = np.array([K, H, repeat, int(per_agent), integrator], dtype=np.int32)
    oi, od = _opp_args(s)
    o = dict(pred=np.zeros((m, Ao, H, 2)), opp_raw=np.zeros((m, K, 2)), opp=np.zeros((m, K, 2), dtype=np.float32), xy=np.zeros((m, K, H, 2)),
             roll=np.zeros((m, K, 2)))
    hh.hh_opp_rollout(*margs, ri.ctypes.data_as(C.c_void_p), C.c_double(margin), oi.ctypes.data_as(C.c_void_p), od.ctypes.data_as(_dp),
                      C.c_double(rr.TIME_STEP), C.c_double(lidar_dist), start.ctypes.data_as(_dp), params.ctypes.data_as(_dp), actions.ctypes.data_as(_dp),
                      opp.ctypes.data_as(_dp), Ao, m, o["pred"].ctypes.data_as(_dp), o["opp_raw"].ctypes.data_as(_dp), o["opp"].ctypes.data_as(C.c_void_p),
                      o["xy"].ctypes.data_as(_dp), o["roll"].ctypes.data_as(_dp))
    return o


def h_mppi(hh, ms, s, w, so, start, params, nominal, streams, opp, integrator, fresh=None, track=None, lidar_dist=0.0):
    K, H = int(ms["k"]), int(ms["horizon"])
    start, params = (np.ascontiguousarray(a, dtype=np.float64) for a in (start, params))
    opp = np.ascontiguousarray(opp, dtype=np.float64)
    m, Ao = start.shape[0], opp.shape[1]
    nom = np.array(nominal, dtype=np.float64, order="C").reshape(m, H, 2)
    words = np.array(streams, dtype=np.uint64, order="C").reshape(m, 4)
    ints = np.array([ms[n] for n in mr.SPEC_INTS], dtype=np.int32)
    dbl = np.array([ms[n] for n in mr.SPEC_FLOATS], dtype=np.float64)
    fr = None if fresh is None else np.ascontiguousarray(fresh, dtype=np.int32)
    cols, margs = _map_args(so, track)
    oi, od = _opp_args(s, w)
    o = dict(actions=np.zeros((m, 2)), info=np.zeros((m, 4), dtype=np.float32), candidates=np.zeros((m, K, H, 2)), cost=np.zeros((m, K)),
             weight=np.zeros((m, K)), raw=np.zeros((m, K, 4)), opp_raw=np.zeros((m, K, 2)), pred=np.zeros((m, Ao, H, 2)))
    hh.hh_opp_mppi(*margs, ints.ctypes.data_as(C.c_void_p), dbl.ctypes.data_as(_dp), oi.ctypes.data_as(C.c_void_p), od.ctypes.data_as(_dp),
                   C.c_double(rr.TIME_STEP), int(integrator), C.c_double(lidar_dist), start.ctypes.data_as(_dp), params.ctypes.data_as(_dp),
                   None if fr is None else fr.ctypes.data_as(C.c_void_p), opp.ctypes.data_as(_dp), Ao, m, nom.ctypes.data_as(_dp),
                   words.ctypes.data_as(C.c_void_p), o["actions"].ctypes.data_as(_dp), o["info"].ctypes.data_as(C.c_void_p),
                   o["candidates"].ctypes.data_as(_dp), o["cost"].ctypes.data_as(_dp), o["weight"].ctypes.data_as(_dp), o["raw"].ctypes.data_as(_dp),
                   o["opp_raw"].ctypes.data_as(_dp), o["pred"].ctypes.data_as(_dp))
    o["nominal"], o["streams"] = nom, words
    return o


def same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), "%s differs from the model" % (what,)


def streams_for(seed, m):
    return np.stack([mr.stream_of(seed, n) for n in range(m)])


@needs_hipcc
@pytest.mark.parametrize("map_name", ["example_map", "berlin"])
def test_harness_matches_model_over_a_grid(hh, map_name):
    """CV / TRACK, Ao in {0, 1, 2, 4}, K in {1, 7, 65}, H in {1, 2, 9}, repeat in {1, 3}: the predictions and (OPP_MIN, OPP_FREE) bit
    for bit (the motion is flown once per shape; the harness and the model share the oracle's arithmetic and glibc's cos / sin); the
    planner's costs and weights bit for bit against the model fed the harness's own rollout values"""
    so, track = rr.scan_oracle(map_name), rr.grid_track(map_name)
    start, params = (a[:ref.GRID_ROWS] for a in rr.grid_rows(map_name))
    q = 0
    for K in (1, 7, 65):
        for H in (1, 2, 9):
            for repeat in (1, 3):
                integrator, per_agent = 1 + q % 2, q // 2 % 2 == 1
                actions = rr.grid_actions(K, H, per_agent, ref.GRID_ROWS)
                flown = rr.fly(so, start, params, actions, per_agent, repeat, rr.GRID_MARGIN, integrator)
                ms = mr.settings(k=K, horizon=H, repeat=repeat, shift=q % 2, margin=rr.GRID_MARGIN, w_progress=3.0 if q % 3 else 0.0, w_lat=0.5 if q % 3 else 0.0)
                nom, words = mr.nominal_for(ms, ref.GRID_ROWS, q), streams_for(300 + q, ref.GRID_ROWS)
                for mode in ref.MODES:
                    for Ao in ref.GRID_AO:
                        what = (map_name, mode, Ao, K, H, repeat)
                        s, opp = ref.grid_settings(mode, Ao), ref.grid_opponents(map_name, Ao)
                        got = h_rollout(hh, s, so, start, params, actions, per_agent, opp, K, H, repeat, rr.GRID_MARGIN, integrator, track)
                        pred = np.stack([ref.predict(s, start[n, 0], start[n, 1], opp[n], H, repeat, track=track) for n in range(ref.GRID_ROWS)]) \
                            if Ao else np.zeros((ref.GRID_ROWS, 0, H, 2))
                        raw, _ = ref.sample_rows(s, flown[3], pred)
                        same(got["xy"], flown[3][..., :2], (what, "positions"))
                        same(got["pred"], pred, (what, "pred"))
                        same(got["opp_raw"], raw, (what, "opp_raw"))
                        same(got["opp"], raw.astype(np.float32), (what, "opp"))
                        if Ao == 0:
                            assert np.all(raw[..., 0] == INF) and np.all(raw[..., 1] == H)
                        if Ao == 4:
                            assert np.all(np.isnan(pred[:, 3])) and np.all(np.isfinite(pred[:, :3]))      # the far one is ignored
                        w = (2.0 + q % 3, 1.5, 1.0)
                        gm = h_mppi(hh, ms, s, w, so, start, params, nom, words, opp, integrator, None, track)
                        cost = ref.costs(ms, w[0], w[1], w[2], gm["raw"], gm["opp_raw"])
                        same(gm["cost"], cost, (what, "cost"))
                        same(gm["pred"], pred, (what, "mppi pred"))
                        for n in range(ref.GRID_ROWS):
                            wts, Un, _, _, _, _ = mr.update(ms, gm["candidates"][n], [float(c) for c in cost[n]])
                            same(gm["weight"][n], np.array(wts), (what, "weight"))
                            same(gm["actions"][n], Un[0], (what, "actions"))
                q += 1


@needs_hipcc
def test_whole_plan_matches_the_model(hh):
    """the planner end to end against the model's own rollout (not fed the harness's values), both modes, on the closed track"""
    so, track = rr.scan_oracle("example_map"), rr.grid_track("example_map")
    start, params = (a[:ref.GRID_ROWS] for a in rr.grid_rows("example_map"))
    for q, mode in enumerate(ref.MODES):
        ms = mr.settings(k=7, horizon=4, repeat=2, margin=rr.GRID_MARGIN, w_progress=3.0, w_lat=0.5)
        s, opp = ref.grid_settings(mode, 2), ref.grid_opponents("example_map", 2)
        nom, words = mr.nominal_for(ms, ref.GRID_ROWS, q), streams_for(40 + q, ref.GRID_ROWS)
        want = ref.plan(ms, s, 3.0, 1.5, 1.0, so, start, params, nom, words, opp, 1, np.array([1, 0, 2]), track)
        got = h_mppi(hh, ms, s, (3.0, 1.5, 1.0), so, start, params, nom, words, opp, 1, np.array([1, 0, 2]), track)
        for key in ("candidates", "streams", "raw", "opp_raw", "pred", "cost", "weight", "actions", "nominal", "info"):
            same(got[key], want[key], (mode, key))


# ---- the GPU grid's seeds ---------------------------------------------------------------------------------------------------------------
def test_the_gpu_grid_leaves_no_candidate_out():
    """tests/test_gpu_opponents.py may leave out a candidate whose |d - radius| is below 1e-9 * radius; on the model's own motion
    its grid (opponents_ref.gpu_cases) has none, so what the GPU test leaves out is the device's own doing"""
    total = 0
    for case in ref.gpu_cases():
        map_name, K, H, repeat, mode, Ao = case
        s, (start, params, actions, opp), track = ref.grid_settings(mode, Ao), ref.gpu_inputs(case), rr.grid_track(map_name)
        flown = ref.gpu_flown(map_name, K, H, repeat)
        pred = np.stack([ref.predict(s, start[n, 0], start[n, 1], opp[n], H, repeat, track=track) for n in range(len(start))]) \
            if Ao else np.zeros((len(start), 0, H, 2))
        _, near = ref.sample_rows(s, flown[3], pred)
        assert not np.any(ref.left_out(near, s["radius"])), case
        total += near.size
    assert total > 10000


def test_the_edge_grid_leaves_no_candidate_out_and_some_hit():
    """the same for tests/test_gpu_opponents_edges.py's grid (opponents_ref.EDGE_CASES: H up to 64, repeat up to 16, 5, 16 and 31
    opponents): no candidate of the model's own motion is within 1e-9 * radius of flipping, candidates hit under every (K, H, repeat),
    and the case with a finite max_range ignores opponents that lie between predicted ones"""
    total, hits, by_shape, ranged = 0, 0, {}, 0
    for case in ref.EDGE_CASES:
        map_name, K, H, repeat, mode, Ao, max_range, _ = case
        s = ref.edge_settings(case)
        pred = ref.edge_pred(case)
        assert pred.shape == (ref.GRID_ROWS, Ao, H, 2)
        if max_range == INF:
            assert np.all(np.isfinite(pred)), case
        else:
            assert ref.nan_rows_between_finite(pred), (case, "no ignored opponent between two predicted ones")
            ranged += 1
        raw, near = ref.sample_rows(s, ref.gpu_flown(map_name, K, H, repeat)[3], pred)
        assert not np.any(ref.left_out(near, s["radius"])), case
        total += near.size
        hit = int(np.count_nonzero(raw[..., 1] < H))
        hits += hit
        by_shape[K, H, repeat] = by_shape.get((K, H, repeat), 0) + hit
    print("edge grid: %d candidates, none left out, %d hit" % (total, hits))
    assert ranged == len(ref.MODES) and all(by_shape.values()), by_shape
    assert set(by_shape) == set(ref.EDGE_KHR) | {ref.EDGE_LIMITS[1:4]} and {c[5] for c in ref.EDGE_CASES} == set(ref.EDGE_AO)
    assert {c[0] for c in ref.EDGE_CASES} == set(rr.GRID_MAPS) and {c[4] for c in ref.EDGE_CASES} == set(ref.MODES)


# ---- cases by hand ----------------------------------------------------------------------------------------------------------------------
P1 = orc.params_vec()[None, :]
FREE = (rr.grid_rows("example_map")[0][0, 0], rr.grid_rows("example_map")[0][0, 1], rr.grid_rows("example_map")[0][0, 4])   # on the example raceline


def row(x, y, theta, v=0.0, fill=2):
    return np.array([[x, y, 0.0, v, theta, 0.0, 0.0, 0.0, 0.0, float(fill)]])


def straight(hh, s, opp, H=6, repeat=5, v=2.0, margin=-INF, start=None, track=None, K=1):
    """one car from FREE along its heading at the commanded speed v (it starts at v: no acceleration), zero steer"""
    so = rr.scan_oracle("example_map")
    st = row(FREE[0], FREE[1], FREE[2], v=v) if start is None else start
    actions = np.zeros((K, H, 2))
    actions[..., 1] = v
    return h_rollout(hh, s, so, st, P1, actions, False, np.asarray(opp, dtype=np.float64).reshape(1, -1, 4), K, H, repeat, margin, 1, track), st


@needs_hipcc
def test_hand_parked_on_the_path(hh):
    """an opponent parked 0.35 m ahead on the heading; the car covers 0.1 m per action (2 m/s, 5 steps of 0.01 s).  After action h it
    is 0.1 (h + 1) m along: distances 0.25, 0.15, 0.05, 0.05, 0.15, 0.25.  radius 0.2: the first hit is action 1; the minimum is the
    0.05 of action 2 (the first of the two, up to the rounding of the motion)"""
    c, sn = math.cos(FREE[2]), math.sin(FREE[2])
    opp = [FREE[0] + 0.35 * c, FREE[1] + 0.35 * sn, 0.0, 1.0]
    got, _ = straight(hh, ref.settings(radius=0.2), opp)
    assert got["opp_raw"][0, 0, 1] == 1.0 and abs(got["opp_raw"][0, 0, 0] - 0.05) < 1e-6
    assert np.all(got["pred"][0, 0] == np.array(opp[:2]))                    # v = 0: parked, whatever its heading
    d = np.hypot(*(got["xy"][0, 0] - np.array(opp[:2])).T)
    assert np.allclose(d, [0.25, 0.15, 0.05, 0.05, 0.15, 0.25], atol=1e-6)
    assert straight(hh, ref.settings(radius=0.04), opp)[0]["opp_raw"][0, 0].tolist() == [got["opp_raw"][0, 0, 0], 6.0]       # never within 4 cm
    assert straight(hh, ref.settings(radius=0.26), opp)[0]["opp_raw"][0, 0, 1] == 0.0
    # the same opponent driving ahead at the car's own speed stays 0.35 m away
    moving = [opp[0], opp[1], 2.0, FREE[2]]
    g2, _ = straight(hh, ref.settings(radius=0.2), moving)
    assert g2["opp_raw"][0, 0, 1] == 6.0 and abs(g2["opp_raw"][0, 0, 0] - 0.35) < 1e-6


@needs_hipcc
def test_hand_max_range_and_nan_rows(hh):
    c, sn = math.cos(FREE[2]), math.sin(FREE[2])
    at = lambda r: [FREE[0] + r * c, FREE[1] + r * sn, 0.0, 0.0]
    inside, outside = at(0.4), at(0.6)
    s = ref.settings(radius=0.2, max_range=0.5)
    g_in, g_out = straight(hh, s, inside)[0], straight(hh, s, outside)[0]
    assert np.all(np.isfinite(g_in["pred"])) and g_in["opp_raw"][0, 0, 1] < 6.0
    assert np.all(np.isnan(g_out["pred"])) and g_out["opp_raw"][0, 0].tolist() == [INF, 6.0]
    assert straight(hh, ref.settings(radius=0.2), outside)[0]["opp_raw"][0, 0, 1] < 6.0         # seen without the limit
    # exactly on the limit counts (<=)
    edge = [FREE[0] + 0.5, FREE[1], 0.0, 0.0]
    dx = edge[0] - FREE[0]
    assert np.all(np.isfinite(straight(hh, ref.settings(radius=0.2, max_range=dx), edge)[0]["pred"]))
    # a NaN opponent beside a real one: its row is NaN and it changes nothing
    both = straight(hh, ref.settings(radius=0.2), [inside, [NAN, 0.0, 1.0, 0.0]])[0]
    assert np.all(np.isnan(both["pred"][0, 1])) and np.array_equal(both["opp_raw"], straight(hh, ref.settings(radius=0.2), inside)[0]["opp_raw"])
    swapped = straight(hh, ref.settings(radius=0.2), [[0.0, NAN, 1.0, 0.0], inside])[0]
    assert np.array_equal(swapped["opp_raw"], both["opp_raw"])
    # a NaN heading with a position in range: CV's predictions are NaN through the cos, and measure nothing
    nanth = straight(hh, ref.settings(radius=0.2), [inside[0], inside[1], 1.0, NAN])[0]
    assert np.all(np.isnan(nanth["pred"])) and nanth["opp_raw"][0, 0].tolist() == [INF, 6.0]
    # no opponents at all
    none = straight(hh, ref.settings(radius=0.2), np.zeros((0, 4)))[0]
    assert none["opp_raw"][0, 0].tolist() == [INF, 6.0] and none["opp"][0, 0].tolist() == [INF, 6.0]


@needs_hipcc
def test_hand_a_dead_candidate_stays_where_it_died(hh):
    """a margin above every clearance kills the candidate at its first step: it is frozen one step from the start while the opponent
    drives by from behind — the distances are those to the frozen pose"""
    c, sn = math.cos(FREE[2]), math.sin(FREE[2])
    opp = [FREE[0] - 0.5 * c, FREE[1] - 0.5 * sn, 2.0, FREE[2]]             # 0.5 m behind, 0.1 m per action
    got, _ = straight(hh, ref.settings(radius=0.15), opp, margin=INF)
    assert got["roll"][0, 0, 0] == 0.0
    assert np.all(got["xy"][0, 0] == got["xy"][0, 0, 0])                      # frozen
    frozen = got["xy"][0, 0, 0]
    d = np.hypot(*(got["pred"][0, 0] - frozen).T)
    want_m, want_free, _ = ref.sample(0.15, got["xy"][0, 0], got["pred"][0])
    assert got["opp_raw"][0, 0].tolist() == [want_m, float(want_free)] == [d.min(), float(np.argmax(d < 0.15))]
    assert want_free == 3 and abs(d.min() - 0.02) < 1e-6                      # 0.42, 0.32, 0.22, 0.12, 0.02, 0.08 m from the pose 0.02 m along


@needs_hipcc
def test_hand_track_mode_across_the_seam(hh):
    """TRACK on the closed example raceline: an opponent just before the seam driving forward wraps to small s; one just behind it
    driving backward (v < 0) wraps to s near L (0.05 m per action, half a segment of about 0.2 m from the seam); the lateral offset
    is kept"""
    track = rr.grid_track("example_map")
    cols, L = ref.track_cols(track), track.length
    last = track.num_segments - 1
    ux, uy = cols[2][last] / cols[5][last], cols[3][last] / cols[5][last]
    near_end = [cols[0][last] + 0.5 * cols[2][last] - 0.2 * uy, cols[1][last] + 0.5 * cols[3][last] + 0.2 * ux, 1.0, 0.0]   # 0.2 m left of the last segment
    u0x, u0y = cols[2][0] / cols[5][0], cols[3][0] / cols[5][0]
    near_start = [cols[0][0] + 0.5 * cols[2][0] + 0.1 * u0y, cols[1][0] + 0.5 * cols[3][0] - 0.1 * u0x, -1.0, 0.0]           # 0.1 m right of segment 0
    s = ref.settings(mode="track", radius=0.2)
    st = row(cols[0][0], cols[1][0], 0.0, v=1.0)
    got, _ = straight(hh, s, [near_end, near_start], H=8, repeat=5, start=st, track=track)
    want = ref.predict(s, st[0, 0], st[0, 1], [near_end, near_start], 8, 5, track=track)
    same(got["pred"][0], want, "pred")
    s_of = lambda p: float(orc_project(track, p)[0])
    fwd, back = [s_of(p) for p in got["pred"][0, 0]], [s_of(p) for p in got["pred"][0, 1]]
    assert fwd[0] > 0.9 * L and fwd[-1] < 0.1 * L and back[0] < 0.1 * L and back[-1] > 0.9 * L
    lat_f, lat_b = [float(orc_project(track, p)[1]) for p in got["pred"][0, 0]], [float(orc_project(track, p)[1]) for p in got["pred"][0, 1]]
    assert np.allclose(lat_f, 0.2, atol=0.02) and np.allclose(lat_b, -0.1, atol=0.02)
    # an open track does not wrap: beyond its end the station is the end point (t clipped)
    otr = rr.grid_track("berlin")
    ocols = ref.track_cols(otr)
    e = otr.num_segments - 1
    tip = [ocols[0][e] + ocols[2][e], ocols[1][e] + ocols[3][e], 50.0, 0.0]
    p = ref.predict(ref.settings(mode="track"), tip[0], tip[1], [tip], 3, 5, track=otr)
    assert np.all(p[0] == p[0][0]) and np.allclose(p[0][0], tip[:2], atol=1e-9)


@needs_hipcc
def test_hand_track_mode_wraps_late_and_beyond_two_laps(hh):
    """opponents_ref.seam_opponents, the rows tests/test_gpu_opponents_edges.py sends through the kernel: the two slow ones cross the
    seam at an action >= 16 (the second lap of the kernel's stride loop), the fast one lies beyond 2 L at the last action, where the
    rule's single subtraction leaves s >= L: the station is the track's end point, finite; all bit for bit the model's"""
    track = rr.grid_track("example_map")
    cols, L, H, repeat = ref.track_cols(track), track.length, 20, 5
    opp = ref.seam_opponents(track)
    s = ref.settings(mode="track", radius=0.2)
    st = row(cols[0][0], cols[1][0], 0.0, v=1.0)
    got, _ = straight(hh, s, opp, H=H, repeat=repeat, start=st, track=track)
    want = ref.predict(s, st[0, 0], st[0, 1], opp, H, repeat, track=track)
    same(got["pred"][0], want, "pred")
    assert np.all(np.isfinite(want))
    fwd, back, fast = (ref.stations_of(track, o, H, repeat) for o in opp)
    assert 16 <= int(np.argmax(fwd >= L)) < H and not np.any(fwd[:16] >= L) and 16 <= int(np.argmax(back < 0.0)) < H and not np.any(back[:16] < 0.0)
    assert fast[-1] > 2.0 * L and fast[-1] - L >= L
    end = np.array([cols[0][-1] + cols[2][-1], cols[1][-1] + cols[3][-1]])
    lat_o = float(orc_project(track, opp[2])[1])
    assert abs(lat_o - 0.2) < 0.02 and np.allclose(want[2, -1], end + lat_o * np.array([-cols[3][-1], cols[2][-1]]) / cols[5][-1], atol=1e-9)


def orc_project(track, p):
    from _util import track_oracle
    return track_oracle(track, np.array([[p[0], p[1], 0.0]]))[0]


@needs_hipcc
def test_hand_zero_weights_are_the_parent_s_costs(hh):
    """w_hit = w_near = 0: the planner's outputs are mppi_ref.plan's (the parent's rule) bit for bit, opponents or not"""
    so, track = rr.scan_oracle("example_map"), rr.grid_track("example_map")
    start, params = (a[:ref.GRID_ROWS] for a in rr.grid_rows("example_map"))
    ms = mr.settings(k=9, horizon=4, repeat=2, margin=rr.GRID_MARGIN, w_progress=3.0, w_lat=0.5)
    nom, words = mr.nominal_for(ms, ref.GRID_ROWS), streams_for(21, ref.GRID_ROWS)
    want = mr.plan(ms, so, start, params, nom, words, 1, None, track)
    for mode in ref.MODES:
        got = h_mppi(hh, ms, ref.grid_settings(mode, 2), (0.0, 0.0, 0.7), so, start, params, nom, words, ref.grid_opponents("example_map", 2), 1, None, track)
        for key in ("candidates", "streams", "raw", "cost", "weight", "actions", "nominal", "info"):
            same(got[key], want[key], (mode, key))
    # and with a weight the hit candidates cost exactly w_hit * (H - free) more (w_near = 0, no track term)
    ms0 = mr.settings(k=9, horizon=4, repeat=2, margin=rr.GRID_MARGIN)
    base = mr.plan(ms0, so, start, params, nom, words, 1)
    got = h_mppi(hh, ms0, ref.grid_settings("cv", 2), (4.0, 0.0, 0.0), so, start, params, nom, words, ref.grid_opponents("example_map", 2), 1)
    assert np.array_equal(got["cost"], base["cost"] + 4.0 * (4.0 - got["opp_raw"][..., 1]))


@needs_hipcc
def test_harness_standalone_under_host_sanitizers(tmp_path):
    """the term's arithmetic as a stand-alone program (its own main) built for the HOST with the address and undefined-behaviour
    sanitizers; nothing is loaded into Python"""
    src = os.path.join(HERE, "host_harness", "opp_harness.hip")
    exe = str(tmp_path / "opp_harness_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DOPP_HARNESS_MAIN",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout.startswith("opp harness: ok"), proc.stdout
