"""CPU checks of the line follower (include/f110.h, f110_line_follower): the settings' validation, the coercion of a
mixed `scripted=` argument, the NumPy restatement (tests/line_follower_ref.py) against the rule's own properties, and the host
instantiation of f110_math.hpp's line_* functions (tests/host_harness/line_follower_main.hip, a stand-alone program built with the
address and undefined-behaviour sanitizers; nothing is loaded into Python) against the restatement on the unit grid."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import line_follower_ref as ref
import raceline_ref
import track_preview_ref as pref
from f1tenth_gym_amd import GapFollower, LineFollower, random_track
from f1tenth_gym_amd.gap_follower import coerce_scripted
from f1tenth_gym_amd.line_follower import coerce_scripted_mixed, has_line_follower, mixed_scripted

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT_A = ref.UNIT_A[:-1]   # (256 cars per env on the GPU only: the harness and the model are both serial)


# ---- the settings ---------------------------------------------------------------------------------------------------------------------
def test_settings_validation():
    f = LineFollower()
    assert f.settings() == ref.DEFAULTS
    nan, inf = float("nan"), float("inf")
    for k in ref.DEFAULTS:
        if k != "speed_attr":
            for bad in (nan, inf, -inf):
                with pytest.raises(ValueError):
                    LineFollower(**{k: bad})
    for bad in (dict(look_min=0.0), dict(look_min=-1.0), dict(look_min=4.0), dict(look_base=-0.1), dict(look_gain=-0.1), dict(speed_look=-0.1),
                dict(wheelbase=0.0), dict(wheelbase=-0.3), dict(steer_max=-0.1), dict(v_min=-0.1), dict(v_min=21.0), dict(follow_range=-1.0),
                dict(lane_width=-0.1), dict(lat_slow=-0.1), dict(speed_attr=-2), dict(speed_attr=4), dict(speed_attr=1.0), dict(speed_attr=True)):
        with pytest.raises(ValueError):
            LineFollower(**bad)
    for ok in (dict(look_min=3.9), dict(look_base=0.0, look_gain=0.0), dict(steer_max=0.0), dict(v_min=20.0), dict(follow_range=0.0), dict(speed_attr=-1),
               dict(speed_attr=3), dict(lane_offset=-1.0), dict(follow_gap=-1.0), dict(v_recover=-1.0)):
        LineFollower(**ok)
    assert LineFollower.coerce(f) is f and LineFollower.coerce(dict(vgain=0.5)).settings() == dict(ref.DEFAULTS, vgain=0.5)
    with pytest.raises(TypeError):
        LineFollower.coerce(3)
    with pytest.raises(TypeError):
        LineFollower.coerce(dict(vgian=1.0))
    assert eval(repr(LineFollower(vgain=0.9, speed_attr=-1))).settings() == LineFollower(vgain=0.9, speed_attr=-1).settings()
    sp = LineFollower(lane_offset=0.3, speed_attr=2).spec()
    assert sp.lane_offset == 0.3 and sp.speed_attr == 2 and sp.v_max == 20.0 and sp.look_base == 0.8


# ---- scripted= --------------------------------------------------------------------------------------------------------------------
def test_mixed_scripted_coercion():
    lf, lf2, gf = LineFollower(), LineFollower(vgain=0.5), GapFollower()
    gap, line = coerce_scripted_mixed({1: lf, 0: gf, 3: lf2}, 2, 4)
    assert np.array_equal(gap[0], [[0, -1, -1, -1]] * 2) and gap[1] == [gf]
    assert np.array_equal(line[0], [[-1, 0, -1, 1]] * 2) and line[1] == [lf, lf2]
    assert gap[0].dtype == line[0].dtype == np.int32
    gap, line = coerce_scripted_mixed({2: lf}, 3, 3)
    assert gap is None and np.array_equal(line[0], [[-1, -1, 0]] * 3)
    # the tuple form: assign indexes the mixed list; a dict in it is a GapFollower's settings, as before
    gap, line = coerce_scripted_mixed(([[0, 1, 2], [2, -1, 0]], [lf, dict(smooth=3), lf2]), 2, 3)
    assert np.array_equal(gap[0], [[-1, 0, -1], [-1, -1, -1]]) and gap[1][0].smooth == 3
    assert np.array_equal(line[0], [[0, -1, 1], [1, -1, 0]]) and line[1] == [lf, lf2]
    gap, line = coerce_scripted_mixed(([[1, -1]], [gf, lf]), 1, 2)   # a class nobody is assigned to drops out
    assert gap is None and np.array_equal(line[0], [[0, -1]])
    assign, ctrls = mixed_scripted({0: lf, 1: gf}, 2, 2)
    assert np.array_equal(assign, [[0, 1]] * 2) and ctrls == [lf, gf]
    for bad in (({5: lf}, 1, 2), (([[0, 2]], [lf, gf]), 1, 2), (([[0]], [lf]), 1, 2), (([[-2, 0]], [lf]), 1, 2), (([[0, 0]], [lf] * 9 + [gf]), 1, 2)):
        with pytest.raises(ValueError):
            coerce_scripted_mixed(*bad)
    with pytest.raises(TypeError):
        coerce_scripted_mixed(3, 1, 2)
    with pytest.raises(TypeError):
        coerce_scripted_mixed({0: lf, 1: 7}, 1, 2)
    assert has_line_follower({0: gf, 1: lf}) and has_line_follower(([[0]], [lf])) and not has_line_follower({0: gf}) and not has_line_follower(([[0]], [{}]))
    assert not has_line_follower(3)


def test_gap_only_inputs_are_unchanged():
    """what coerce_scripted accepted before keeps its result, and the env layer still routes it there"""
    gf = GapFollower(smooth=7)
    for scripted in ({1: gf}, {0: dict(smooth=3), 1: gf}, ([[0, -1], [-1, 0]], [gf])):
        assert not has_line_follower(scripted)
        a, c = coerce_scripted(scripted, 2, 2)
        gap, line = coerce_scripted_mixed(scripted, 2, 2)
        assert line is None and np.array_equal(gap[0], a) and [x.settings() for x in gap[1]] == [x.settings() for x in c]


def test_one_car_cannot_have_two_drivers():
    """an agent has one entry in `assign`, so one controller; the planner's slot is checked against both controller classes"""
    from f1tenth_gym_amd import F110VecEnv, Mppi
    with pytest.raises(ValueError, match="both a line follower and the planner"):
        F110VecEnv(2, num_agents=2, device_logic=True, scripted={1: LineFollower(), }, planner=(1, Mppi()), track='raceline')
    with pytest.raises(ValueError, match="needs a track"):
        F110VecEnv(2, num_agents=2, device_logic=True, scripted={1: LineFollower()})
    with pytest.raises(ValueError, match="at most 256 cars per env"):
        F110VecEnv(1, num_agents=257, device_logic=True, scripted={0: LineFollower()}, track='raceline')


# ---- the model's own properties -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def property_tracks():
    tr = random_track(1, 8.0, 1.0)
    q, w = raceline_ref.stations(tr)
    r = raceline_ref.raceline(q, w)
    attrs = np.column_stack([r["kappa"], r["vx"], r["alpha"]])
    return [("stadium",) + ref.stadium(), ("raceline", ref.Tables(r["xy"], True, attrs), r["xy"], attrs)]


def test_model_bounds(property_tracks):
    rng = np.random.default_rng(5)
    for name, tab, _, _ in property_tracks:
        for S in (ref.settings(), ref.settings(v_min=1.0, v_max=2.5, steer_max=0.2, lane_offset=0.3), ref.settings(speed_attr=-1, follow_range=0.0)):
            for A in (1, 4):
                m = 40 * A
                s = rng.uniform(0.0, tab.L, m)
                lat = rng.uniform(-1.0, 1.0, m)
                rows = np.array([[*ref.on_line(tab, s[r], lat[r], rng.uniform(-1.0, 1.0)), rng.uniform(-1.0, 9.0), s[r], lat[r], 1.0] for r in range(m)])
                act, raw = ref.follow(tab, S, rows, A)
                assert np.all(np.abs(act[:, 0]) <= S["steer_max"]) and np.all((act[:, 1] >= S["v_min"]) & (act[:, 1] <= S["v_max"])), name
                assert np.all((raw[:, 0] >= S["look_min"]) & (raw[:, 0] <= S["look_max"]))


def test_model_steers_into_the_bend(property_tracks):
    """a car on the line with the line's heading steers towards the inside of the bend: the sign of the curvature attribute,
    wherever the curvature keeps one sign from the car to its target; zero on an exact straight"""
    S = ref.settings()
    checked = 0
    for name, tab, _, attrs in property_tracks:
        kappa = attrs[:, 0]
        for s in np.linspace(0.0, tab.L, 97, endpoint=False):
            x, y, th = ref.on_line(tab, s)
            act, raw = ref.follow(tab, S, [[x, y, th, 2.0, s, 0.0, 1.0]])
            k0, k1 = pref.segment_of(tab, s), int(raw[0, 2])
            span = kappa[np.arange(k0, k0 + (k1 - k0) % tab.nseg + 2) % tab.npts]
            if np.all(span > 0.02):
                assert act[0, 0] > 0.0, (name, s)
            elif np.all(span < -0.02):
                assert act[0, 0] < 0.0, (name, s)
            elif name == "stadium" and np.all(span == 0.0) and k1 + 1 < 10:
                assert act[0, 0] == 0.0, (name, s)
            else:
                continue
            checked += 1
    assert checked > 60


def test_model_limit_is_the_nearest_eligible_car(property_tracks):
    rng = np.random.default_rng(11)
    S = ref.settings(vgain=2.0)   # (fast enough for every eligible car to cap it)
    for name, tab, _, _ in property_tracks:
        for A in (2, 5, 16):
            for _ in range(20):
                s = rng.uniform(0.0, tab.L, A)
                lat = rng.uniform(-0.5, 0.5, A)
                rows = np.array([[*ref.on_line(tab, s[a], lat[a]), 1.0, s[a], lat[a], 1.0] for a in range(A)])
                _, raw = ref.follow(tab, S, rows, A)
                for a in range(A):
                    g = np.array([ref.gap(s[a], s[b], tab.L) for b in range(A)])
                    ok = (g > 0.0) & (g <= S["follow_range"]) & (np.abs(lat - lat[a]) <= S["lane_width"])
                    ok[a] = False
                    capped = ok & (1.0 + (g - 1.0) < raw[a, 9] * S["vgain"])
                    want = -1 if not capped.any() else int(np.flatnonzero(capped)[np.argmin(g[capped])])
                    assert int(raw[a, 10]) == want, (name, A, a)


# ---- the arithmetic, compiled for the host ---------------------------------------------------------------------------------------------
def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


needs_hipcc = pytest.mark.skipif(not os.path.isfile(hipcc()), reason="hipcc not installed")
SRC = os.path.join(HERE, "host_harness", "line_follower_main.hip")
ORDER = ("look_base", "look_gain", "look_min", "look_max", "lane_offset", "wheelbase", "steer_max", "v_const", "vgain", "speed_look", "lat_slow",
         "v_recover", "follow_range", "follow_gap", "follow_gain", "lane_width", "v_min", "v_max")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """the stand-alone program, built for the HOST with the address and undefined-behaviour sanitizers"""
    exe = str(tmp_path_factory.mktemp("line_follower_main") / "line_follower_main")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return exe


def run_program(exe, tmp, cases):
    """cases [(tab, xy, attrs, S, A, rows)] -> [(actions, raw)]"""
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(cases)], dtype=np.int32).tobytes())
        for tab, S, A, rows in cases:
            f.write(np.array([tab.closed, tab.npts, tab.C, A, rows.shape[0], S["speed_attr"]], dtype=np.int32).tobytes())
            f.write(np.array([S[k] for k in ORDER], dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(tab.xy, dtype=np.float64).tobytes() + np.ascontiguousarray(tab.attrs, dtype=np.float64).tobytes())
            f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
    proc = subprocess.run([exe, src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0, proc.stdout
    raw, pos, out = np.fromfile(dst, dtype=np.float64), 0, []
    for tab, S, A, rows in cases:
        m = rows.shape[0]
        out.append((raw[pos:pos + 2 * m].reshape(m, 2), raw[pos + 2 * m:pos + 14 * m].reshape(m, 12)))
        pos += 14 * m
    assert pos == raw.size
    return out


@needs_hipcc
def test_host_program_self_check(program):
    proc = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout.startswith("ok: 4 rows"), proc.stdout


@needs_hipcc
def test_host_program_equals_reference_on_the_unit_grid(program, tmp_path):
    rng = np.random.default_rng(2)
    cases, firsts = [], []
    for name, tab, _, _ in ref.unit_tracks():
        for k, A in enumerate(UNIT_A):
            S = ref.unit_settings(name, k)
            rows, first = ref.unit_rows(tab, S, A, rng)
            cases.append((tab, S, A, rows))
            firsts.append(first)
    got = run_program(program, tmp_path, cases)
    decided = 0
    for (tab, S, A, rows), first, g in zip(cases, firsts, got):
        what = "A = %d, %d segments" % (A, tab.nseg)
        ref.compare(tab, S, rows, A, g, what)
        decided += ref.boundary_check(tab, S, A, rows, first, g[1], what)
    assert decided >= 5 * 12      # per track: ten boundary cars at A = 2, the car at follow_range exactly at A = 3 and 5


def test_the_grid_notices_an_off_by_one_compare():
    """the boundary cars decide: the model with `g <= follow_range` read as `<`, with `<= lane_width` read as `<`, or with either
    bound moved one ulp outwards, changes `lim` on the grid of every track at A = 2"""
    rng = np.random.default_rng(2)
    for name, tab, _, _ in ref.unit_tracks():
        S = ref.unit_settings(name, 1)
        rows, first = ref.unit_rows(tab, S, 2, rng)
        want = ref.follow(tab, S, rows, 2)[1][:, 10]
        for key in ("follow_range", "lane_width"):
            for moved in (math.nextafter(S[key], 0.0), math.nextafter(S[key], math.inf)):
                assert not np.array_equal(ref.follow(tab, dict(S, **{key: moved}), rows, 2)[1][:, 10], want), (name, key, moved)
