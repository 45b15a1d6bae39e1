"""The corridor carve (f110_add_map_corridor) and the track generator without a GPU: the fixtures' conditions, the NumPy
model (tests/trackgen_ref.py) against the reference pipeline on the carved image, the round trip line -> table -> centreline on
the model, random_track, TrackMap, and the host instantiation of the kernel's decision and tile-and-cull walk
(tests/host_harness/corridor_harness.hip) against the model, cell for cell."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
from scipy.ndimage import distance_transform_edt

import centerline_ref as cref
import trackgen_ref as ref
from f1tenth_gym_amd import Track, TrackMap, random_track, trackgen
from f1tenth_gym_amd.centerline import cell_centres

HERE = os.path.dirname(os.path.abspath(__file__))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")

ROUND_TRIP_CELLS = ref.ROUND_TRIP_CELLS


def all_fixtures():
    return list(ref.star_fixtures()) + list(ref.edge_fixtures())


# ---- the fixtures and the model ------------------------------------------------------------------------------------------------
def test_fixture_conditions():
    """no cell centre within 1e-9 m of a capsule's boundary, on any fixture: no cell is left out of any comparison; the star
    fixtures turn gently enough for the corridor not to fold; the corridor stays inside the ring where the fixture says so"""
    names = [fx.name for fx in all_fixtures()]
    assert names == ref.STAR_NAMES + ref.EDGE_NAMES and len(set(names)) == len(names)
    for fx in all_fixtures() + [ref.tight_fixture(), ref.no_carve_line()]:
        assert fx.margin() > 1e-9, (fx.name, fx.margin())
        assert fx.H <= 280 and fx.W <= 320
        touched = bool((ref.corridor_mask(fx.xy, fx.hw, fx.closed, fx.H, fx.W, fx.frame, with_ring=False) & ref.ring(fx.H, fx.W)).any())
        if fx.inside:
            assert not touched, fx.name
        assert not (fx.mask() & ref.ring(fx.H, fx.W)).any()
    for fx in ref.star_fixtures():
        assert 31 <= fx.xy.shape[0] <= 200 and ref.max_kappa(fx.xy) * fx.hw.max() < 0.95, fx.name
    assert abs(ref.max_kappa(ref.tight_fixture().xy) * ref.tight_fixture().hw.max() - 1.8) < 1e-9
    assert ref.fixture("crosses_border").mask().any() and (ref.corridor_mask(*_line(ref.fixture("crosses_border")), with_ring=False) & ref.ring(38, 72)).any()
    assert ref.fixture("all_free").mask().sum() == 35 * 88                     # everything but the ring
    assert ref.fixture("yaw").origin[2] == 0.3 and ref.fixture("star120").origin[2] == 0.3
    assert (ref.fixture("widths").hw == 0.0).sum() == 1 and len(set(ref.fixture("widths").hw)) == 5
    assert ref.fixture("repeated_point").xy[1].tobytes() == ref.fixture("repeated_point").xy[2].tobytes()
    assert not ref.no_carve_line().mask().any()
    assert 45 % ref.TILE_H != 0


def _line(fx):
    return fx.xy, fx.hw, fx.closed, fx.H, fx.W, fx.frame


def test_wound_fixtures_fill_one_tile_past_the_list():
    """M = C - 1, C, C + 1 and 2 C + 3 points whose segments ALL carve cells of one tile: what any culling must keep there is S,
    below, at and (2 C + 2) above the list's capacity C"""
    for M in (ref.CAP - 1, ref.CAP, ref.CAP + 1, 2 * ref.CAP + 3):
        fx = ref.fixture("wound%d" % M)
        need = ref.tile_need(*_line(fx))
        assert need.max() == M - 1 and need[1, 1] == M - 1, (M, need)
    assert 2 * ref.CAP + 2 > ref.CAP


def test_model_equals_the_reference_pipeline_on_the_carved_image():
    """flip, > 128, resolution * distance_transform_edt on the image with the carved cells white"""
    for fx in all_fixtures():
        img = ref.image_of(fx.mask())
        assert img.dtype == np.uint8 and set(np.unique(img)) <= {0, 255}
        free = ref.free_from_image(img)
        assert np.array_equal(free, fx.mask()), fx.name
        want = fx.res * distance_transform_edt(free)
        assert np.array_equal(fx.table(), want), fx.name
        assert fx.table()[fx.H - 1, fx.W - 1] == 0.0 and np.array_equal(fx.table() > 0, fx.mask())


def _round_trip(fx):
    T = fx.table()
    cells, hw, _, final = cref.centerline(T > 0, T, fx.res, fx.origin, seed=tuple(fx.xy[0]))
    nb = sum(cref.shifted(final, dr, dc).astype(np.int32) for dr, dc in cref.NBR)
    assert np.all(nb[cells[:, 0], cells[:, 1]] == 2), "not a simple loop"
    dev = ref.polyline_distance(cell_centres(cells, fx.frame), fx.xy) / fx.res
    return cells, float(dev.max())


@pytest.mark.parametrize("name", ref.STAR_NAMES)
def test_round_trip_line_table_centerline(name):
    """the centreline of the model's table is a simple loop that stays within the measured distance of the line it was carved
    around (measured: ROUND_TRIP_CELLS, 1.42 .. 2.14 cells)"""
    fx = ref.fixture(name)
    cells, dev = _round_trip(fx)
    print("%s: %d loop cells, largest distance from the line %.4f cells" % (name, len(cells), dev))
    assert len(cells) >= fx.xy.shape[0]
    assert dev <= ROUND_TRIP_CELLS[name] + 0.25, (name, dev)


def test_round_trip_breaks_where_the_corridor_folds():
    """|kappa| * hw = 1.8: the corridor is still a ring and has a centreline, but it leaves the line by several cells (measured:
    9.84) — what random_track's tightness check keeps out"""
    cells, dev = _round_trip(ref.tight_fixture())
    print("tight: largest distance from the line %.4f cells" % dev)
    assert dev > 4.0 > max(ROUND_TRIP_CELLS.values()) + 0.25


# ---- random_track ---------------------------------------------------------------------------------------------------------------
def test_random_track_is_deterministic_per_seed():
    a, b, c = random_track(7), random_track(7), random_track(8)
    assert a.xy.tobytes() == b.xy.tobytes() and a.attrs.tobytes() == b.attrs.tobytes()
    assert a.xy.tobytes() != c.xy.tobytes()
    assert a.closed and a.attr_names == ('half_width', 'kappa')


def test_random_tracks_satisfy_the_acceptance_conditions_and_fit_their_frames():
    for seed in range(32):
        t = random_track(seed)
        hw, gap = 1.0, 0.5
        tight, near = trackgen.acceptance(t.xy, t.attrs[:, 1], hw, gap)
        assert tight < 0.9 and near >= 2 * hw + gap, (seed, tight, near)
        assert np.array_equal(t.attrs[:, 0], np.full(t.num_points, hw))
        assert np.allclose(t.seg_len, t.seg_len[0], rtol=1e-3) and abs(t.seg_len[0] - 0.2) < 0.01     # uniform in arc length
        assert 0.5 * float(np.sum(t.xy[:, 0] * np.roll(t.xy[:, 1], -1) - np.roll(t.xy[:, 0], -1) * t.xy[:, 1])) > 0.0   # counter-clockwise
        # the brute-force restatement of the second condition
        s = t.cum
        for i in range(0, t.num_points, 7):
            arc = np.abs(s - s[i])
            arc = np.minimum(arc, t.length - arc)
            dist = np.sqrt(np.sum((t.xy - t.xy[i]) ** 2, axis=1))
            assert not np.any((arc > 2 * hw + gap) & (dist < 2 * hw + gap)), seed
        # the default frame holds the corridor inside the ring, with the margin (checked on a coarse raster of the same frame rule)
        tm = TrackMap(t, resolution=0.25)
        H, W = tm.shape
        assert H <= 16384 // 4 and TrackMap(t).shape[0] in (4 * H, 4 * H - 1, 4 * H - 2, 4 * H - 3)
        m = ref.corridor_mask(tm.points(), tm.widths(), True, H, W, tm.frame(), with_ring=False)
        assert m.any() and not (m & ref.ring(H, W)).any(), seed
        assert not m[:3].any() and not m[:, :3].any() and not m[-3:].any() and not m[:, -3:].any()   # margin 1 m = 4 cells, less one of rounding
    # ... and on the real default frame (0.0625 m): the corridor's outermost carved cells lie the margin inside, 1 m = 16 cells, less
    # the cell the frame's rounding up and a cell centre's half cell can take
    for seed in (0, 13, 31):
        tm = TrackMap(random_track(seed))
        H, W = tm.shape
        assert tm.resolution == 0.0625 and tm.origin[2] == 0.0
        m = ref.corridor_mask(tm.points(), tm.widths(), True, H, W, tm.frame(), with_ring=False)
        rows, cols = np.flatnonzero(m.any(axis=1)), np.flatnonzero(m.any(axis=0))
        assert 15 <= rows[0] <= 16 and 15 <= cols[0] <= 16 and 15 <= H - 1 - rows[-1] <= 17 and 15 <= W - 1 - cols[-1] <= 17, (seed, rows[[0, -1]], cols[[0, -1]], H, W)


def test_random_track_rejects_and_gives_up():
    with pytest.raises(ValueError, match="no acceptable line in 3 tries"):
        random_track(1, tightness=1e-6, max_tries=3)
    with pytest.raises(ValueError, match="no acceptable line in 64 tries"):
        random_track(1, radius=1.0, half_width=0.5, wall_gap=0.9)     # D = 1.9 m: opposite sides of a 1 m star are closer than that
    # a rejected draw is passed over: seed 3's first accepted line under a tightness its first draws miss is a later draw of the
    # same stream
    rng = np.random.default_rng(3)
    a, p = rng.uniform(-0.3, 0.3, 4), rng.uniform(0.0, 2.0 * np.pi, 4)
    q, _, _, _ = trackgen.resample_closed(trackgen.star_line(a, p, 8.0)[0], np.zeros(trackgen.STAR_SAMPLES), 0.2)
    first, near = trackgen.acceptance(q, trackgen.curvature_closed(q), 0.5, 0.1)
    assert near >= 1.1
    t = random_track(3, half_width=0.5, wall_gap=0.1, tightness=first * 0.999, max_tries=4096)
    assert t.xy.tobytes() != q.tobytes() and np.max(np.abs(t.attrs[:, 1])) * 0.5 < first * 0.999
    assert random_track(3, half_width=0.5, wall_gap=0.1, tightness=first * 1.001).xy.tobytes() == q.tobytes()
    with pytest.raises(ValueError, match="stations"):
        random_track(0, radius=400.0, spacing=0.1)
    for bad in (dict(radius=0.0), dict(spacing=-1.0), dict(half_width=float('nan')), dict(max_tries=0), dict(amplitude=-0.1)):
        with pytest.raises(ValueError):
            random_track(0, **bad)


# ---- TrackMap -------------------------------------------------------------------------------------------------------------------
def test_trackmap_frames_widths_and_refusals():
    t = random_track(5)
    tm = TrackMap(t)
    assert tm.origin[2] == 0.0 and tm.resolution == 0.0625 and tm.widths().shape == (t.num_segments,)
    assert np.array_equal(tm.widths(), np.ones(t.num_segments))
    lo, hi = t.xy.min(axis=0), t.xy.max(axis=0)
    assert tm.origin[0] == lo[0] - 2.0 and tm.origin[1] == lo[1] - 2.0                        # the largest half width plus the margin
    assert tm.shape == (int(np.ceil((hi[1] - lo[1] + 4.0) / 0.0625)), int(np.ceil((hi[0] - lo[0] + 4.0) / 0.0625)))
    assert tm.frame() == (0.0625, tm.origin[0], tm.origin[1], 1.0, 0.0)
    # half widths: a number, one per segment, the attribute column averaged over a segment's ends
    w = np.linspace(0.5, 1.5, t.num_points)
    tw = Track(t.xy, attrs={'half_width': w})
    assert np.array_equal(TrackMap(tw).widths(), 0.5 * (w + np.roll(w, -1)))
    op = Track(t.xy[:20], closed=False, attrs={'half_width': w[:20]})
    assert np.array_equal(TrackMap(op).widths(), 0.5 * (w[:19] + w[1:20]))
    assert np.array_equal(TrackMap(t, 0.7).widths(), np.full(t.num_segments, 0.7))
    assert np.array_equal(TrackMap(t, w).widths(), w)
    # same_frame
    assert tm.same_frame(TrackMap(t, 0.7, shape=tm.shape, origin=tm.origin)) and not tm.same_frame(TrackMap(t, 0.7))
    assert not tm.same_frame(TrackMap(t, resolution=0.05, shape=tm.shape, origin=tm.origin)) and not tm.same_frame(None)
    yawed = TrackMap(t, origin=(lo[0] - 5.0, lo[1] - 12.0, 0.3))
    m = ref.corridor_mask(yawed.points(), yawed.widths(), True, yawed.shape[0], yawed.shape[1], yawed.frame(), with_ring=False)
    assert m.any() and not m[-8:].any() and not m[:, -8:].any()                               # the shape covers the grown box in the turned frame
    # immutable
    with pytest.raises(AttributeError):
        tm.resolution = 0.1
    with pytest.raises(AttributeError):
        tm._shape = (1, 1)
    with pytest.raises(AttributeError):
        del tm.track
    with pytest.raises(ValueError):
        tm.widths()[0] = 2.0
    # refusals
    for kw in (dict(half_width=-0.1), dict(half_width=float('inf')), dict(half_width=np.ones(3)), dict(resolution=0.0), dict(resolution=float('nan')),
               dict(margin=-1.0), dict(shape=(0, 10)), dict(shape=(10, 16385)), dict(shape=(10.5, 10)), dict(origin=(0.0, 0.0)),
               dict(origin=(0.0, float('nan'), 0.0))):
        with pytest.raises(ValueError):
            TrackMap(t, **kw)
    with pytest.raises(ValueError, match="half_width"):
        TrackMap(Track(t.xy))
    assert TrackMap.coerce(tm) is tm and isinstance(TrackMap.coerce(t), TrackMap)
    assert TrackMap.coerce(dict(seed=5)).track.xy.tobytes() == t.xy.tobytes()


def test_abi_signatures_are_struct_free():
    from f1tenth_gym_amd import _ffi
    P = _ffi.PROTOTYPES
    i32, f64 = C.c_int32, C.c_double
    assert P["f110_add_map_corridor"] == (C.c_int, [C.c_void_p, _ffi._dp, _ffi._dp, i32, i32, i32, i32, f64, f64, f64, f64, _ffi._i32p])
    assert P["f110_set_map_corridor"] == (C.c_int, [C.c_void_p, i32, _ffi._dp, _ffi._dp, i32, i32])
    assert P["f110_corridor_mask_batch"] == (C.c_int, [C.c_void_p, _ffi._dp, _ffi._dp, i32, i32, i32, i32, f64, f64, f64, f64, f64, _ffi._u8p, _ffi._i64p])
    assert P["f110_map_corridor_times"] == (C.c_int, [C.c_void_p, _ffi._dp])
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "f110.h")).read()
    for name in ("f110_add_map_corridor", "f110_set_map_corridor", "f110_corridor_mask_batch", "f110_map_corridor_times", "F110_MAX_CORRIDOR_POINTS = 65536"):
        assert name in hdr
    assert trackgen.MAX_CORRIDOR_POINTS == 65536


# ---- the host instantiation of the kernel's decision and walk -------------------------------------------------------------------
def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "corridor_harness.hip")
    lib = str(tmp_path_factory.mktemp("corridor_harness") / "libcorridor_harness.so")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness_mask(hh, fx, cull=True):
    """-> (mask uint8 [H][W], carved, the largest per-tile kept count, rounds, cell tests)"""
    mask = np.full((fx.H, fx.W), 9, dtype=np.uint8)
    carved, rounds, tests, kept = C.c_longlong(-1), C.c_longlong(-1), C.c_longlong(-1), C.c_int(-1)
    dp = C.POINTER(C.c_double)
    hh.hh_corridor_mask(fx.xy.ctypes.data_as(dp), fx.hw.ctypes.data_as(dp), C.c_int(fx.xy.shape[0]), C.c_int(int(fx.closed)), C.c_int(fx.H), C.c_int(fx.W),
                        *[C.c_double(v) for v in fx.frame], C.c_int(int(cull)), mask.ctypes.data_as(C.POINTER(C.c_ubyte)), C.byref(carved), C.byref(kept),
                        C.byref(rounds), C.byref(tests))
    return mask, int(carved.value), int(kept.value), int(rounds.value), int(tests.value)


@needs_hipcc
def test_harness_constants_are_the_models(hh):
    out = (C.c_int * 4)()
    hh.hh_corridor_consts(out)
    assert tuple(out) == (ref.TILE_H, ref.TILE_W, 256, ref.CAP) and ref.CAP >= 256


@needs_hipcc
@pytest.mark.parametrize("name", ref.STAR_NAMES + ref.EDGE_NAMES)
def test_harness_mask_equals_model(hh, name):
    """the kernel's decision and its tile-and-cull walk on the host: mask and carved count equal to the model's, with and without
    culling; no tile keeps fewer segments than carve cells of it; a tile that keeps nothing runs no cell test"""
    fx = ref.fixture(name)
    want = fx.mask()
    got, carved, kept, rounds, tests = harness_mask(hh, fx)
    assert np.array_equal(got, want.astype(np.uint8)), "%s: %d cells differ" % (name, int((got != want).sum()))
    assert carved == int(want.sum())
    whole, carved_w, kept_w, _, tests_w = harness_mask(hh, fx, cull=False)
    assert np.array_equal(whole, got) and carved_w == carved and kept_w == fx.hw.shape[0]
    need = int(ref.tile_need(*_line(fx)).max())
    assert need <= kept <= fx.hw.shape[0]
    assert tests <= tests_w
    if name.startswith("wound"):
        M = fx.xy.shape[0]
        assert kept == M - 1 and (rounds >= 1 if M - 1 > ref.CAP else rounds == 0), (kept, rounds)   # (a round per tile whose list overflows)
        if M == 2 * ref.CAP + 3:
            assert need > ref.CAP     # one tile really keeps more than the list holds
    if name in ("star160", "star200"):
        # a tile's circle (1.7 m) plus the half width reaches about 5 m of these 30 m lines: no tile keeps a quarter of the segments
        assert kept * 4 <= fx.hw.shape[0] and tests * 4 < tests_w


@needs_hipcc
def test_harness_nothing_carved(hh):
    fx = ref.no_carve_line()
    got, carved, _, _, _ = harness_mask(hh, fx)
    assert carved == 0 and not got.any()


@needs_hipcc
def test_harness_standalone_under_host_sanitizers(tmp_path):
    """the same text as a stand-alone program (its own main: lines inside, across and far outside a table under a turned frame that
    is no rotation, sizes up to 1e300, a wound line past the list's capacity) built for the HOST with the address and undefined-
    behaviour sanitizers; nothing is loaded into Python"""
    src = os.path.join(HERE, "host_harness", "corridor_harness.hip")
    exe = str(tmp_path / "corridor_harness_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DCORR_HARNESS_MAIN",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout.startswith("ok:"), proc.stdout[-2000:]
