"""CPU checks of the rollout: the settings' validation, the struct layout against the header, cases worked out by hand
and the host instantiation of f110_math.hpp's roll_* functions (tests/host_harness/rollout_harness.hip) against the Python model
(tests/rollout_ref.py) over the grid and on candidates that drive into walls.  The GPU tests (tests/test_gpu_rollout.py) hold the
kernels to the same model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import rollout_ref as ref
from _util import raceline
from f1tenth_gym_amd import Rollout, Track, _ffi
from f1tenth_gym_amd import rollout as rom
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
NAN, INF = float("nan"), float("inf")


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(k=0), dict(k=257), dict(k=-1), dict(k=2.5), dict(k=True),
    dict(horizon=0), dict(horizon=65), dict(horizon=1.0),
    dict(repeat=0), dict(repeat=17), dict(repeat=False),
    dict(channels=()), dict(channels=("alive", "speed")), dict(channels=("alive", "alive")),
    dict(frame="world"), dict(frame=0), dict(layout="each"), dict(layout=1), dict(traj=2), dict(traj="yes"),
    dict(margin=NAN),
    dict(scale={"alive": 0.0}), dict(scale={"alive": -1.0}), dict(scale={"alive": INF}), dict(scale={"alive": NAN}), dict(scale={"speed": 1.0}),
    dict(traj=True, scale={"end_x": 0.0}), dict(traj=True, channels=("alive",), scale={"end_sin": -2.0}),
])
def test_rollout_validation_refuses(kw):
    with pytest.raises(ValueError):
        Rollout(**kw)


def test_rollout_defaults_struct_and_coerce():
    p = Rollout()
    assert (p.k, p.horizon, p.repeat, p.channels, p.margin, p.frame, p.layout, p.traj, p.dim) == (8, 8, 1, ("alive", "min_clear"), 0.0, "ego", "shared", False, 2)
    assert p.shape(6) == (6, 8, 2) and p.traj_shape(6) == (6, 8, 8, 4) and p.actions_shape(6) == (8, 8, 2) and not p.needs_track and p.steps == 8
    sp = p.spec()
    assert (sp.k, sp.horizon, sp.repeat, sp.layout, sp.frame, sp.channels, sp.traj, sp.margin) == (8, 8, 1, 0, 0, 64 | 128, 0, 0.0)
    assert list(sp.scale) == [1.0] * 10
    q = Rollout(k=256, horizon=64, repeat=16, channels=("end_lat", "progress", "end_x"), margin=-INF, frame="map", layout="per_agent", traj=True,
                scale={"end_x": 10.0, "progress": 2.0, "end_y": 4.0, "alive": 0.0})
    assert q.channels == ("end_x", "progress", "end_lat") and q.channel_mask == 1 | 256 | 512 and q.needs_track   # (a clear bit's scale is ignored ...)
    assert list(q.spec().scale) == [10.0, 4.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 2.0, 1.0]                                # (... but not end_y's with traj)
    assert q.actions_shape(3) == (3, 256, 64, 2) and q.spec().frame == 1 and q.spec().layout == 1 and q.spec().traj == 1 and q.steps == 1024
    assert Rollout(channels=("alive",), scale={"end_x": 0.0}).scale["end_x"] == 1.0
    S = _ffi.RolloutSpec
    assert C.sizeof(S) == 8 * 4 + 8 + 10 * 8
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 40]
    assert Rollout.coerce(dict(k=3)).k == 3 and Rollout.coerce(p) is p
    assert Rollout(**q.settings()).settings() == q.settings()
    assert rom.CHANNELS == ref.CHANNELS
    with pytest.raises(TypeError):
        Rollout.coerce(7)


def test_struct_and_enums_match_the_header():
    """the struct's fields in the header's order and types, and the enum values, read from include/f110.h"""
    with open(os.path.join(os.path.dirname(HERE), "include", "f110.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct f110_rollout \{(.*?)\} f110_rollout;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(int32_t|double)\s+(\w+)(?:\[\w+\])?;", body)]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    mirror = _ffi.RolloutSpec._fields_
    assert [n for _, n in fields] == [n for n, _ in mirror]
    for (t, n), (_, ct) in zip(fields, mirror):
        assert ct is ctype[t] or (n == "scale" and ct._type_ is C.c_double and ct._length_ == 10), n
    enums = dict(re.findall(r"(F110_ROLL_[A-Z_]+) = (\d+)", src))
    names = ["END_X", "END_Y", "END_COS", "END_SIN", "END_V", "END_YAW_RATE", "ALIVE", "MIN_CLEAR", "PROGRESS", "END_LAT"]
    assert [int(enums["F110_ROLL_" + n]) for n in names] == [1 << b for b in range(10)]
    assert [getattr(_ffi, "ROLL_" + n) for n in names] == [1 << b for b in range(10)]
    for n in ("NCHANNELS", "SHARED", "PER_AGENT", "FRAME_EGO", "FRAME_MAP", "MAX_K", "MAX_H", "MAX_REPEAT"):
        assert int(enums["F110_ROLL_" + n]) == getattr(_ffi, "ROLL_" + n), n
    assert (rom.MAX_K, rom.MAX_H, rom.MAX_REPEAT) == (256, 64, 16)


# ---- the host instantiation ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "rollout_harness.hip")
    lib = str(tmp_path_factory.mktemp("rollout_harness") / "librollout_harness.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def track_cols(track):
    """the seven segment columns f110_track_set uploads: ax, ay, dx, dy, l2, len, cum"""
    pts = track.points_closed()
    a, d = pts[:-1], pts[1:] - pts[:-1]
    return np.ascontiguousarray(np.stack([a[:, 0], a[:, 1], d[:, 0], d[:, 1], d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1], track.seg_len, track.cum]))


def harness(hh, s, so, start, params, actions, integrator, track=None, lidar_dist=0.0):
    """(out, raw, traj, traj_raw) of the host instantiation for settings s (tests/rollout_ref.settings)"""
    K, H = int(s["k"]), int(s["horizon"])
    mask = sum(1 << b for b, c in enumerate(ref.CHANNELS) if c in s["channels"])
    scale = np.array([float(s["scale"].get(c, 1.0)) for c in ref.CHANNELS])
    start, params, actions = (np.ascontiguousarray(a, dtype=np.float64) for a in (start, params, actions))
    m = start.shape[0]
    assert actions.shape == ((m,) if s["layout"] == "per_agent" else ()) + (K, H, 2)
    out, raw = np.zeros((m, K, bin(mask).count("1")), dtype=np.float32), np.zeros((m, K, 10))
    traj, traw = np.zeros((m, K, H, 4), dtype=np.float32), np.zeros((m, K, H, 4))
    cols = None if track is None else track_cols(track)
    c = so.cfg
    hh.hh_rollout(so.dt.ctypes.data_as(_dp), c.height, c.width, C.c_double(c.resolution), C.c_double(c.orig_x), C.c_double(c.orig_y),
                  C.c_double(c.orig_c), C.c_double(c.orig_s), None if cols is None else cols.ctypes.data_as(_dp),
                  0 if track is None else track.num_segments, int(track is not None and track.closed), C.c_double(0.0 if track is None else track.length),
                  K, H, int(s["repeat"]), int(s["layout"] == "per_agent"), int(s["frame"] == "map"), mask, int(bool(s["traj"])), C.c_double(s["margin"]),
                  scale.ctypes.data_as(_dp), C.c_double(ref.TIME_STEP), int(integrator), C.c_double(lidar_dist), start.ctypes.data_as(_dp),
                  params.ctypes.data_as(_dp), actions.ctypes.data_as(_dp), m, out.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(_dp),
                  traj.ctypes.data_as(C.c_void_p), traw.ctypes.data_as(_dp))
    return out, raw, traj, traw


def row(x, y, theta, v=0.0, steer=0.0, fifo=(0.0, 0.0), fill=2):
    return np.array([[x, y, steer, v, theta, 0.0, 0.0, fifo[0], fifo[1], float(fill)]])


P1 = orc.params_vec()[None, :]
FREE = (ref.grid_rows("example_map")[0][0, 0], ref.grid_rows("example_map")[0][0, 1])   # a point on the example raceline


@needs_hipcc
def test_hand_car_at_rest_stays_where_it_is(hh):
    so = ref.scan_oracle("example_map")
    s = ref.settings(k=2, horizon=4, repeat=3, margin=0.1)
    st = row(FREE[0], FREE[1], 1.25)
    out, raw, traj, traw = harness(hh, s, so, st, P1, np.zeros((2, 4, 2)), 1)
    for k in range(2):
        assert raw[0, k, :2].tolist() == [FREE[0], FREE[1]] and raw[0, k, ref.END_V] == 0.0 and raw[0, k, ref.END_YAW_RATE] == 0.0
        assert raw[0, k, ref.ALIVE] == 12.0 and raw[0, k, ref.MIN_CLEAR] == ref.clearance(so, *FREE)
        assert np.all(traw[0, k, :, 0] == FREE[0]) and np.all(traw[0, k, :, 1] == FREE[1])
    assert np.allclose(raw[0, :, 2:4], [np.cos(1.25), np.sin(1.25)], atol=8 * ref.EPS, rtol=0.0)
    # in its own frame the car sits at the origin looking along x
    _, rawe, _, trawe = harness(hh, dict(s, frame="ego"), so, st, P1, np.zeros((2, 4, 2)), 1)
    assert rawe[0, 0, :2].tolist() == [0.0, 0.0] and np.allclose(rawe[0, 0, 2:4], [1.0, 0.0], atol=8 * ref.EPS, rtol=0.0)
    assert np.all(trawe[0, :, :, :2] == 0.0)


@needs_hipcc
def test_hand_margin_above_the_start_clearance_freezes_the_first_step(hh):
    so = ref.scan_oracle("example_map")
    st = row(FREE[0], FREE[1], 0.7, v=3.0, steer=0.05, fifo=(0.1, -0.1))
    act = np.array([[[0.2, 5.0], [0.3, 6.0], [-0.3, 1.0]]])
    s = ref.settings(k=1, horizon=3, repeat=2, margin=ref.clearance(so, *FREE) + 1.0)
    out, raw, traj, traw = harness(hh, s, so, st, P1, act, 1)
    one, _, _, _ = orc.update_pose(st[0, :7], st[0, 7:9], 2, 0.2, 5.0, P1[0], ref.TIME_STEP, 1, 0.0)
    assert raw[0, 0, ref.ALIVE] == 0.0 and raw[0, 0, ref.MIN_CLEAR] == ref.clearance(so, one[0], one[1])
    assert raw[0, 0, [ref.END_X, ref.END_Y, ref.END_V, ref.END_YAW_RATE]].tolist() == [one[0], one[1], one[3], one[5]]
    assert np.all(traw[0, 0, :, 0] == one[0]) and np.all(traw[0, 0, :, 1] == one[1])      # a dead candidate repeats its frozen pose
    # -inf: nothing dies of its clearance
    _, raw2, _, _ = harness(hh, dict(s, margin=-INF), so, st, P1, act, 1)
    assert raw2[0, 0, ref.ALIVE] == 6.0


@needs_hipcc
def test_hand_nan_state_dies_at_step_0_and_a_start_outside_the_map_reads_the_last_cell(hh):
    so = ref.scan_oracle("example_map")
    oob = float(so.dt[-1, -1])
    assert oob > 1.0
    s = ref.settings(k=1, horizon=2, repeat=2, margin=0.5)
    act = np.array([[[0.0, 1.0], [0.0, 1.0]]])
    for st in (row(NAN, FREE[1], 0.0), row(FREE[0], NAN, 0.0), row(FREE[0], FREE[1], NAN, v=1.0)):
        _, raw, _, _ = harness(hh, s, so, st, P1, act, 1)
        assert raw[0, 0, ref.ALIVE] == 0.0, st
    _, raw, _, _ = harness(hh, s, so, row(-500.0, 900.0, 0.3, v=1.0), P1, act, 1)
    assert raw[0, 0, ref.ALIVE] == 4.0 and raw[0, 0, ref.MIN_CLEAR] == oob
    _, raw, _, _ = harness(hh, dict(s, margin=oob), so, row(-500.0, 900.0, 0.3, v=1.0), P1, act, 1)
    assert raw[0, 0, ref.ALIVE] == 0.0 and raw[0, 0, ref.MIN_CLEAR] == oob                    # alive needs d > margin, not >=


@needs_hipcc
def test_hand_the_last_two_steer_commands_never_arrive(hh):
    """the two-step steering delay: with repeat = 1 the commands of the last two steps are still in the FIFO at the end"""
    so = ref.scan_oracle("example_map")
    rng = np.random.default_rng(3)
    act = np.stack([rng.uniform(-0.4, 0.4, (2, 6)), rng.uniform(2.0, 6.0, (2, 6))], axis=-1)
    act[1] = act[0]
    act[1, 4:, 0] = [0.4, -0.4]
    st = row(FREE[0], FREE[1], 0.7, v=2.0, fifo=(0.1, -0.2))
    s = ref.settings(k=2, horizon=6, repeat=1, margin=-INF)
    for integrator in (1, 2):
        _, raw, _, traw = harness(hh, s, so, st, P1, act, integrator)
        assert np.array_equal(ref.bits(raw[0, 0]), ref.bits(raw[0, 1])) and np.array_equal(ref.bits(traw[0, 0]), ref.bits(traw[0, 1]))
    _, raw, _, _ = harness(hh, dict(s, repeat=2), so, st, P1, act, 1)                       # held two steps, the fifth command arrives
    assert not np.array_equal(ref.bits(raw[0, 0]), ref.bits(raw[0, 1]))


@needs_hipcc
def test_hand_progress_across_the_closing_segment_and_at_half_the_length(hh):
    hh.hh_roll_progress.restype = C.c_double
    hh.hh_roll_progress.argtypes = [C.c_double, C.c_double, C.c_int, C.c_double]
    # L = 8: exactly +L/2 stays, exactly -L/2 wraps to +L/2; an open track never wraps
    for s0, s1, closed, opened in ((0.0, 4.0, 4.0, 4.0), (4.0, 0.0, 4.0, -4.0), (0.0, 5.0, -3.0, 5.0), (5.0, 0.0, 3.0, -5.0), (1.0, 4.0, 3.0, 3.0), (7.5, 0.25, 0.75, -7.25)):
        assert hh.hh_roll_progress(s0, s1, 1, 8.0) == closed and hh.hh_roll_progress(s0, s1, 0, 8.0) == opened, (s0, s1)
    # a car 0.3 m before the example raceline's first point drives over it: s falls by almost L, the progress is the metres driven
    w = raceline()
    track = Track(w[:, 1:3])
    so = ref.scan_oracle("example_map")
    th = float(np.arctan2(w[1, 2] - w[0, 2], w[1, 1] - w[0, 1]))
    st = row(w[0, 1] - 0.3 * np.cos(th), w[0, 2] - 0.3 * np.sin(th), th, v=4.0)
    act = np.array([[[0.0, 4.0]]])
    s = ref.settings(k=1, horizon=1, repeat=16, margin=0.0)
    got = harness(hh, s, so, st, P1, act, 1, track)
    want = ref.render(s, st, ref.fly(so, st, P1, act, False, 16, 0.0, 1), track)
    assert got[1][0, 0, ref.ALIVE] == 16.0 and np.array_equal(ref.bits(got[1][..., ref.EXACT]), ref.bits(want[1][..., ref.EXACT]))
    assert 0.5 < got[1][0, 0, ref.PROGRESS] < 0.7 and abs(got[1][0, 0, ref.END_LAT]) < 0.05
    open_track = Track(w[:-1, 1:3], closed=False)
    assert harness(hh, s, so, st, P1, act, 1, open_track)[1][0, 0, ref.PROGRESS] < -0.5 * track.length


def compare(s, start, flown, want, got, what):
    """the harness's (out, raw, traj, traj_raw) against the model's: the map-frame values, ALIVE, MIN_CLEAR, PROGRESS and END_LAT bit
    for bit; the ego-frame positions within 8 eps (|rx| + |ry|) and every cos / sin value within 8 eps (the model's cos and sin are
    NumPy's, the harness's libm's; a rotation is two products and a sum of operands of that size); every float32 the model's or its
    neighbour.  -> (float32 values compared, float32 values that differ)"""
    out, raw, traj, traw = got
    w_out, w_raw, w_traj, w_traw = want
    ego = s["frame"] == "ego"
    exact = [b for b in ref.EXACT if not (ego and b in (ref.END_X, ref.END_Y))]
    assert np.array_equal(ref.bits(raw[..., exact]), ref.bits(w_raw[..., exact])), "%s: exact channels differ" % (what,)
    with np.errstate(invalid="ignore"):
        if not ego:
            assert np.array_equal(ref.bits(traw[..., :2]), ref.bits(w_traw[..., :2])), "%s: map-frame trajectory differs" % (what,)
        else:
            end, poses = flown[0], flown[3]
            size = np.abs(end[..., 0] - start[:, None, 0]) + np.abs(end[..., 1] - start[:, None, 1])
            tsize = np.abs(poses[..., 0] - start[:, None, None, 0]) + np.abs(poses[..., 1] - start[:, None, None, 1])
            assert np.all(np.abs(raw[..., :2] - w_raw[..., :2]) <= 8 * ref.EPS * size[..., None]), "%s: ego end position" % (what,)
            assert np.all(np.abs(traw[..., :2] - w_traw[..., :2]) <= 8 * ref.EPS * tsize[..., None]), "%s: ego trajectory" % (what,)
        assert np.all(np.abs(raw[..., 2:4] - w_raw[..., 2:4]) <= 8 * ref.EPS) and np.all(np.abs(traw[..., 2:] - w_traw[..., 2:]) <= 8 * ref.EPS), "%s: cos / sin" % (what,)
    return out.size + traj.size, ref.float32_neighbours(out, w_out) + ref.float32_neighbours(traj, w_traj)


@needs_hipcc
def test_harness_matches_model_over_the_grid(hh):
    total = differ = cases = 0
    seen = set()
    for case in ref.grid_cases():
        map_name, K, H, repeat, integrator, per_agent = case
        start, params = ref.grid_rows(map_name)
        so, track = ref.scan_oracle(map_name), ref.grid_track(map_name)
        flown = ref.grid_flown(case)
        for frame in ("map", "ego"):
            s = ref.grid_settings(case, frame)
            got = harness(hh, s, so, start, params, ref.grid_actions(K, H, per_agent), integrator, track)
            n, d = compare(s, start, flown, ref.render(s, start, flown, track), got, (case, frame))
            total, differ, cases = total + n, differ + d, cases + 1
        seen.add((K, H, repeat, integrator, per_agent))
    assert len(seen) == 4 * 2 * 2 * 2 * 2 and cases == 2 * len(ref.grid_cases())
    assert total > 100000 and differ * 1000 <= total, (total, differ)
    fills, v = ref.grid_rows("berlin")[0][:, 9], np.abs(ref.grid_rows("berlin")[0][:, 3])
    assert set(fills.tolist()) == {0.0, 1.0, 2.0} and np.any(v < 0.5) and np.any(v > 0.5)


@needs_hipcc
def test_harness_a_subset_of_channels_and_a_lidar_offset(hh):
    """the channels come in bit order whatever order they are asked for in; the lidar offset does not move the clearance sample"""
    case = ("example_map", 3, 5, 3, 1, True)
    start, params = ref.grid_rows("example_map")
    so, track = ref.scan_oracle("example_map"), ref.grid_track("example_map")
    s = dict(ref.grid_settings(case, "ego"), channels=("end_lat", "alive", "end_x"), traj=False)
    want = ref.render(s, start, ref.grid_flown(case), track)
    got = harness(hh, s, so, start, params, ref.grid_actions(3, 5, True), 1, track)
    assert got[0].shape == (6, 3, 3) and ref.float32_neighbours(got[0], want[0]) <= 1 and np.all(got[2] == 0.0)
    assert np.array_equal(ref.bits(got[0][..., 1:]), ref.bits(want[0][..., 1:]))
    moved = harness(hh, s, so, start, params, ref.grid_actions(3, 5, True), 1, track, lidar_dist=0.275)
    assert np.array_equal(ref.bits(moved[1]), ref.bits(got[1]))


@needs_hipcc
def test_candidates_that_drive_into_walls(hh):
    start, params, actions, flown = ref.wall_case()
    alive = flown[1]
    died = alive < 60
    assert 4 * np.count_nonzero(died) >= died.size and 4 * np.count_nonzero(~died) >= died.size, (int(died.sum()), died.size)
    assert np.all(flown[2][died] <= ref.GRID_MARGIN) and np.all(flown[2][~died] > ref.GRID_MARGIN)
    so, track = ref.scan_oracle("example_map"), ref.grid_track("example_map")
    for frame in ("map", "ego"):
        s = ref.settings(k=2, horizon=60, repeat=1, margin=ref.GRID_MARGIN, frame=frame, scale={"alive": 60.0, "end_x": 2.0})
        got = harness(hh, s, so, start, params, actions, 1, track)
        n, d = compare(s, start, flown, ref.render(s, start, flown, track), got, ("walls", frame))
        assert d * 1000 <= n
        assert np.array_equal(got[1][..., ref.ALIVE], alive.astype(np.float64))
        # a dead candidate's trajectory repeats the pose it froze at
        k_dead = np.argwhere(died)
        for n_, k_ in k_dead[:8]:
            a = int(alive[n_, k_])
            assert np.all(got[3][n_, k_, a:] == got[3][n_, k_, a])
