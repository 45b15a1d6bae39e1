"""CPU checks of the track preview: the settings' and the attributes' validation, the struct layout, the NumPy model
(tests/track_preview_ref.py) on stations worked out by hand on a unit square, Track.preview against the model, and the host
instantiation of f110_math.hpp's preview_* functions (tests/host_harness/preview_harness.hip) against the model over the grid.
The GPU tests (tests/test_gpu_track_preview.py) hold the kernel to the same model."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import track_preview_ref as ref
from _util import MAPS
from f1tenth_gym_amd import Track, TrackPreview, _ffi
from f1tenth_gym_amd import track_preview as tp

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
CSV = os.path.join(MAPS, "example_waypoints.csv")
NAN = float("nan")


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(points=0), dict(points=33), dict(points=-1), dict(points=2.5), dict(points=True),
    dict(channels=()), dict(channels=("x", "speed")), dict(channels=("x", "x")), dict(channels=("attr4",)),
    dict(frame="car"), dict(frame=2),
    dict(offset=-0.1), dict(offset=np.inf), dict(offset=np.nan),
    dict(spacing=0.0), dict(spacing=-1.0), dict(spacing=np.inf), dict(spacing=np.nan), dict(points=1, spacing=0.0),
    dict(scale={"x": 0.0}), dict(scale={"y": np.inf}, channels=("y",)), dict(scale={"x": np.nan}), dict(scale={"speed": 1.0}),
])
def test_preview_validation_refuses(kw):
    with pytest.raises(ValueError):
        TrackPreview(**kw)


def test_preview_defaults_struct_and_coerce():
    p = TrackPreview()
    assert (p.points, p.offset, p.spacing, p.channels, p.frame, p.dim) == (8, 0.5, 0.5, ("x", "y"), "ego", 2)
    assert p.shape(6) == (6, 8, 2) and p.reach == 4.0 and p.num_attrs == 0
    sp = p.spec()
    assert (sp.points, sp.channels, sp.frame, sp.flags, sp.offset, sp.spacing) == (8, 3, _ffi.PREVIEW_FRAME_EGO, 0, 0.5, 0.5)
    assert list(sp.scale) == [1.0] * 8
    q = TrackPreview(points=32, channels=("attr2", "tan_y", "x"), frame="world", scale={"x": 10.0, "attr2": -2.0, "y": 0.0})
    assert q.channels == ("x", "tan_y", "attr2") and q.channel_mask == 1 | 8 | 64 and q.num_attrs == 3   # (a clear bit's scale is ignored)
    assert list(q.spec().scale) == [10.0, 1.0, 1.0, 1.0, 1.0, 1.0, -2.0, 1.0] and q.spec().frame == _ffi.PREVIEW_FRAME_WORLD == 1
    # struct f110_track_preview: 4 int32, 2 double, 8 double
    S = _ffi.TrackPreviewSpec
    assert C.sizeof(S) == 4 * 4 + 2 * 8 + 8 * 8
    assert (S.points.offset, S.channels.offset, S.frame.offset, S.flags.offset, S.offset.offset, S.spacing.offset, S.scale.offset) == (0, 4, 8, 12, 16, 24, 32)
    assert [_ffi.PREVIEW_X, _ffi.PREVIEW_Y, _ffi.PREVIEW_TAN_X, _ffi.PREVIEW_TAN_Y, _ffi.PREVIEW_ATTR0, _ffi.PREVIEW_ATTR3] == [1, 2, 4, 8, 16, 128]
    assert (_ffi.PREVIEW_NCHANNELS, _ffi.PREVIEW_MAX_POINTS, _ffi.TRACK_MAX_ATTRS) == (8, 32, 4) and tp.CHANNELS == ref.CHANNELS
    assert TrackPreview.coerce(dict(points=3)).points == 3 and TrackPreview.coerce(p) is p
    assert TrackPreview(**q.settings()).settings() == q.settings()
    with pytest.raises(TypeError):
        TrackPreview.coerce(7)


SQ = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]


@pytest.mark.parametrize("attrs", [
    np.zeros((3, 1)), np.zeros((4, 5)), np.zeros((4, 0)), np.zeros(4), np.array([[0.0], [np.nan], [0.0], [0.0]]),
    np.array([[0.0], [np.inf], [0.0], [0.0]]), {"a": [1.0, 2.0, 3.0]}, {k: [0.0] * 4 for k in "abcde"}, {},
])
def test_track_attrs_refused(attrs):
    with pytest.raises(ValueError):
        Track(SQ, attrs=attrs)


def test_track_attrs_forms():
    assert Track(SQ).attrs is None and Track(SQ).num_attrs == 0             # existing calls behave as before
    t = Track(SQ, attrs={"kappa": [1.0, 2.0, 3.0, 4.0], "vx": [5.0, 6.0, 7.0, 8.0]})
    assert t.attr_names == ("kappa", "vx") and t.attrs.tolist() == [[1.0, 5.0], [2.0, 6.0], [3.0, 7.0], [4.0, 8.0]] and t.num_attrs == 2
    rep = SQ + [SQ[0]]                                                        # a closed track drops the repeated last row with the point
    t = Track(rep, attrs=np.arange(5.0)[:, None])
    assert t.num_points == 4 and t.attrs[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0]
    t = Track(rep, closed=False, attrs=np.arange(5.0)[:, None])
    assert t.num_points == 5 and t.attrs.shape == (5, 1)
    with pytest.raises(ValueError):
        Track(rep, attrs=np.zeros((4, 1)))                                    # a row per point as given
    w = np.loadtxt(CSV, delimiter=';', skiprows=3)
    t = Track.from_csv(CSV, attrs={'kappa': 4, 'vx': 5})
    assert t.num_segments == 782 and t.attr_names == ("kappa", "vx")
    assert np.array_equal(t.attrs, w[:-1, 4:6]) and np.array_equal(Track.from_csv(CSV).xy, t.xy)
    with pytest.raises(ValueError):
        TrackPreview(channels=("attr2",)).check_track(t)
    with pytest.raises(ValueError):
        TrackPreview(points=9, offset=0.0, spacing=0.5).check_track(Track(SQ))   # reach 4.0 = L: one subtraction is not enough
    TrackPreview(points=8, offset=0.0, spacing=0.5).check_track(Track(SQ))
    TrackPreview(points=32, spacing=5.0).check_track(Track(SQ, closed=False))


def test_vec_env_argument_checks():
    """raised before a simulator is made"""
    from f1tenth_gym_amd import F110VecEnv
    with pytest.raises(ValueError, match="track_preview_device"):
        F110VecEnv(2, track_preview=TrackPreview(), track=CSV, map="example_map")
    with pytest.raises(ValueError, match="needs a track"):
        F110VecEnv(2, track_preview=TrackPreview(), device_logic=True, map="example_map")
    with pytest.raises(ValueError, match="attribute"):
        F110VecEnv(2, track_preview=dict(channels=("x", "attr0")), device_logic=True, track=CSV, map="example_map")
    with pytest.raises(ValueError, match="reach"):
        F110VecEnv(2, track_preview=dict(points=32, spacing=6.0), device_logic=True, track=CSV, map="example_map")
    with pytest.raises(ValueError):
        F110VecEnv(2, track_preview=dict(points=0), device_logic=True, track=CSV, map="example_map")
    with pytest.raises(TypeError):
        F110VecEnv(2, track_preview=3, device_logic=True, track=CSV, map="example_map")


# ---- stations worked out by hand on the unit square ---------------------------------------------------------------------------
ALL5 = ("x", "y", "tan_x", "tan_y", "attr0")


def hand_cases():
    """(name, closed, settings, pose, s, segments, raw rows [P][5] = X, Y, ux, uy, attr0 in the WORLD frame)"""
    w = dict(channels=ALL5, frame="world")
    return [
        # s = 0.5, spacing 0.5: stations 1.0, 1.5, 2.0, 2.5, 3.0 sit on cum[k]: the new segment wins with t = 0
        ("on_cum", True, ref.settings(points=5, offset=0.5, spacing=0.5, **w), (0.5, 0.1, 0.0), 0.5, [1, 1, 2, 2, 3],
         [[1.0, 0.0, 0.0, 1.0, 11.0], [1.0, 0.5, 0.0, 1.0, 11.5], [1.0, 1.0, -1.0, 0.0, 12.0], [0.5, 1.0, -1.0, 0.0, 12.5], [0.0, 1.0, 0.0, -1.0, 13.0]]),
        # s_j == L exactly: it wraps to 0, segment 0
        ("wrap_at_L", True, ref.settings(points=2, offset=0.5, spacing=0.25, **w), (0.0, 0.5, 0.0), 3.5, [0, 0],
         [[0.0, 0.0, 1.0, 0.0, 10.0], [0.25, 0.0, 1.0, 0.0, 10.25]]),
        # the closing segment interpolates the attribute towards point 0: 13 + 0.5 (10 - 13)
        ("closing", True, ref.settings(points=2, offset=0.5, spacing=0.25, **w), (0.0, 1.0, 0.0), 3.0, [3, 3],
         [[0.0, 0.5, 0.0, -1.0, 11.5], [0.0, 0.25, 0.0, -1.0, 10.75]]),
        ("one_station", True, ref.settings(points=1, offset=0.0, spacing=0.5, **w), (0.25, 0.0, 0.0), 0.25, [0],
         [[0.25, 0.0, 1.0, 0.0, 10.25]]),
        # open: cum = 0, 1, 2 and L = 3; stations 3.0, 3.5, 4.0 are at and beyond the end and repeat the last point
        ("open_end", False, ref.settings(points=3, offset=0.5, spacing=0.5, **w), (0.5, 1.0, 0.0), 2.5, [2, 2, 2],
         [[0.0, 1.0, -1.0, 0.0, 13.0]] * 3),
        # open, before the start there is nothing to find: s_j < cum[0] cannot happen with s >= 0, but a negative s clips to point 0
        ("open_before", False, ref.settings(points=1, offset=0.0, spacing=0.5, **w), (0.0, 0.0, 0.0), -0.5, [0],
         [[0.0, 0.0, 1.0, 0.0, 10.0]]),
    ]


@pytest.mark.parametrize("case", hand_cases(), ids=lambda c: c[0])
def test_model_and_track_on_hand_built_stations(case):
    name, closed, s, pose, arc, segs, rows = case
    tab, xy, attrs = ref.unit_square(closed, attrs=1)
    assert tab.cum == ([0.0, 1.0, 2.0, 3.0] if closed else [0.0, 1.0, 2.0]) and tab.L == (4.0 if closed else 3.0)
    out, raw, seg = ref.preview(tab, s, [pose], [arc])
    assert seg[0].tolist() == segs and raw[0][:, :5].tolist() == rows and out[0].tolist() == rows and np.all(raw[0][:, 5:] == 0.0)
    t = Track(xy, closed=closed, attrs=attrs)
    got = t.preview([pose], [arc], TrackPreview(**s), raw=True, segments=True)
    assert got[2][0].tolist() == segs and got[1][0][:, :5].tolist() == rows and got[0][0].tolist() == rows


def test_model_ego_frame_scale_and_nan():
    tab, xy, attrs = ref.unit_square(True, attrs=1)
    # a car at (0.5, 0) heading +y: the station at (1, 0.5) is 0.5 ahead and 0.5 to the right; the tangent (0, 1) points ahead
    s = ref.settings(points=1, offset=1.0, spacing=0.5, channels=ALL5, frame="ego", scale={"x": 0.5, "y": -0.25, "attr0": 2.0})
    out, raw, seg = ref.preview(tab, s, [(0.5, 0.0, np.pi / 2)], [0.5])
    assert seg.tolist() == [[1]] and np.allclose(raw[0, 0, :5], [0.5, -0.5, 1.0, 0.0, 11.5], atol=1e-15)
    assert np.allclose(out[0, 0], [1.0, 2.0, 1.0, 0.0, 5.75], atol=1e-6) and out.dtype == np.float32
    # the channels come in bit order whatever order they are asked for in; float32 is the rounded float64 quotient
    s2 = ref.settings(points=1, offset=1.0, spacing=0.5, channels=("attr0", "x"), frame="world", scale={"attr0": 3.0})
    out2, _, _ = ref.preview(tab, s2, [(0.5, 0.0, 0.0)], [0.5])
    assert out2[0, 0].tolist() == [1.0, float(np.float32(11.5 / 3.0))]
    # a NaN pose (and the NaN s its projection gives): segment 0, NaN outputs
    out3, raw3, seg3 = ref.preview(tab, ref.settings(points=3, channels=ALL5), [(NAN, NAN, NAN)], [NAN])
    assert seg3.tolist() == [[0, 0, 0]] and np.all(np.isnan(out3)) and np.all(np.isnan(raw3[..., :5]))
    got = Track(xy, attrs=attrs).preview([(NAN, NAN, NAN)], [NAN], TrackPreview(points=3, channels=ALL5), segments=True)
    assert got[1].tolist() == [[0, 0, 0]] and np.all(np.isnan(got[0]))


def grid_case(k, case, rng, m=6):
    name, make, closed, attrs, P, frame, channels = case
    tab, xy, a = make(closed=closed, attrs=attrs)
    s = ref.grid_settings(name, tab, P, frame, channels, k)
    poses, arc = ref.poses_near(tab, rng, m, spread=0.2 if name == "square" else 0.4)
    if k % 5 == 0:
        poses[0], arc[0] = NAN, NAN
    return tab, xy, a, s, poses, arc


def test_grid_holds_both_sides_of_the_staging_boundary():
    """the circles named after their segment counts have them, closed and open; the default circle is on the staged side"""
    for closed in (True, False):
        assert ref.circle_2048(closed, 0)[0].nseg == ref.STAGED_SEGS and ref.circle_2049(closed, 4)[0].nseg == ref.STAGED_SEGS + 1
    assert ref.circle(closed=True)[0].nseg == 1500 <= ref.STAGED_SEGS
    names = [c[0] for c in ref.unit_grid()]
    assert names.count("circle_2048") == 16 and names.count("circle_2049") == 16
    assert {(c[2], c[3], c[4]) for c in ref.unit_grid() if c[0] == "circle_2049"} == {(cl, a, P) for cl in (True, False) for a in (0, 4) for P in (1, 32)}


def test_track_preview_method_matches_model_over_the_grid():
    """Track.preview (vectorised NumPy) against the model; the condition of the EGO bound: with NumPy's cos / sin on both sides
    no float32 output differs at all"""
    rng = np.random.default_rng(31)
    n = 0
    for k, case in enumerate(ref.unit_grid()):
        tab, xy, a, s, poses, arc = grid_case(k, case, rng)
        t = Track(xy, closed=case[2], attrs=a)
        assert t.num_segments == tab.nseg and np.array_equal(t.cum, np.array(tab.cum)) and t.length == tab.L
        got = t.preview(poses, arc, TrackPreview(**s), raw=True, segments=True)
        assert ref.compare(tab, s, poses, arc, got, "%s %r" % (case[0], s)) == 0
        assert ref.compare(tab, s, poses, arc, ref.preview(tab, s, poses, arc), "model") == 0
        n += got[0].size
    assert n > 20000


# ---- the host instantiation of f110_math.hpp's preview_* against the model ------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "preview_harness.hip")
    lib = str(tmp_path_factory.mktemp("preview_harness") / "libpreview_harness.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness_preview(hh, tab, s, poses, arc):
    n = tab.nseg
    dx, dy = np.array(tab.dx), np.array(tab.dy)
    cols = np.ascontiguousarray(np.stack([tab.ax, tab.ay, dx, dy, dx * dx + dy * dy, tab.len, tab.cum]), dtype=np.float64)
    attr = None if tab.attrs is None else np.ascontiguousarray(tab.attrs.T)
    P = int(s["points"])
    bits = [b for b, c in enumerate(ref.CHANNELS) if c in s["channels"]]
    scale = np.array([float(s["scale"].get(c, 1.0)) for c in ref.CHANNELS])
    rows = np.ascontiguousarray(np.column_stack([np.asarray(poses, dtype=np.float64).reshape(-1, 3), np.asarray(arc, dtype=np.float64)]))
    m = rows.shape[0]
    out, raw, seg = np.zeros((m, P, len(bits)), dtype=np.float32), np.zeros((m, P, 8)), np.zeros((m, P), dtype=np.int32)
    hh.hh_track_preview(cols.ctypes.data_as(_dp), n, int(tab.closed), C.c_double(tab.L), None if attr is None else attr.ctypes.data_as(_dp),
                        tab.C, tab.npts, P, sum(1 << b for b in bits), 1 if s["frame"] == "world" else 0, C.c_double(s["offset"]),
                        C.c_double(s["spacing"]), scale.ctypes.data_as(_dp), rows.ctypes.data_as(_dp), m, out.ctypes.data_as(C.c_void_p),
                        raw.ctypes.data_as(_dp), seg.ctypes.data_as(C.POINTER(C.c_int)))
    return out, raw, seg


@needs_hipcc
def test_harness_matches_model_over_the_grid(hh):
    rng = np.random.default_rng(32)
    total = differ = wrapped = clipped = 0
    for k, case in enumerate(ref.unit_grid()):
        tab, xy, a, s, poses, arc = grid_case(k, case, rng, m=8)
        differ += ref.compare(tab, s, poses, arc, harness_preview(hh, tab, s, poses, arc), "%s closed=%r attrs=%d %r" % (case[0], case[2], case[3], s))
        total += len(poses) * s["points"] * len(s["channels"])
        reach = s["offset"] + (s["points"] - 1) * s["spacing"]
        with np.errstate(invalid="ignore"):
            wrapped += int(np.sum(arc + reach >= tab.L)) if tab.closed else 0
            clipped += int(np.sum(arc + reach >= tab.L)) if not tab.closed else 0
    assert total > 30000 and differ * 1000 <= total, (total, differ)
    assert wrapped > 20 and clipped > 5, (wrapped, clipped)     # the wrap and the open end are on the grid


@needs_hipcc
def test_harness_on_hand_built_stations(hh):
    for name, closed, s, pose, arc, segs, rows in hand_cases():
        tab, _, _ = ref.unit_square(closed, attrs=1)
        out, raw, seg = harness_preview(hh, tab, s, [pose], [arc])
        assert seg[0].tolist() == segs and raw[0][:, :5].tolist() == rows and out[0].tolist() == rows, name
