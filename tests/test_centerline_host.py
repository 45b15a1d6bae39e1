"""CPU-only checks of the centreline extraction (include/f110.h, f110_map_centerline): the NumPy reference
(tests/centerline_ref.py) on fixtures built here as 96 x 130 images — the width no multiple of 64, every corridor across columns
63 / 64 — the host post-processing (f1tenth_gym_amd/centerline.py) against its restatement, and the host instantiation of
f110_math.hpp's per-word decisions (tests/host_harness/centerline_main.hip, a stand-alone program) against the reference, cell for cell.

The loop lengths below are what the reference gives on these fixtures.  Measured on the three annuli, the largest radial distance
of a loop cell centre from the mid circle is 1.147, 0.880 and 0.996 cells (widths 9, 10, 13, centred on and off half-cell
positions); the test asserts the measured value plus 0.25 cell — the margin for a differently centred, equally valid fixture —
and never more than 2 cells."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import centerline_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = ref.fixtures()

# fixture -> loop cells; None: refused
LOOPS = {"annulus_w9": 169, "annulus_w10": 170, "annulus_w13": 170, "annulus_spur": 170, "annulus_spurs3": 170, "annulus_blob": 170,
         "rect_w12": 319, "rect_w11_12": 322, "border_ring": 399}
REFUSED = {"figure_eight": "not_simple", "annulus_spur_diamond": "not_simple", "straight": "no_loop"}
# the largest radial distance from the mid circle the reference measured here, in cells (the module docstring)
RADIAL = {"annulus_w9": 1.147, "annulus_w10": 0.880, "annulus_w13": 0.996}


@pytest.fixture(scope="module")
def results():
    """the reference's answer on every fixture, computed once: name -> (cells, half_width, deleted, final, T) or a Refused"""
    out = {}
    for name, img in FIX.items():
        free = ref.free_from_image(img)
        T = ref.edt_table(free, ref.RES)
        try:
            out[name] = ref.centerline(free, T, ref.RES, ref.ORIGIN, ref.fixture_seed(name)) + (T,)
        except ref.Refused as ex:
            out[name] = ex
    return out


def degrees(final):
    return np.array([len(ref.set_neighbours(final, r, c)) for r, c in np.argwhere(final)])


def test_fixture_shapes():
    assert set(LOOPS) | set(REFUSED) == set(FIX)
    for name, img in FIX.items():
        assert img.shape == (96, 130) and img.dtype == np.uint8, name
        free = ref.free_from_image(img)
        assert free[:, 63].any() and free[:, 64].any(), name    # the corridor crosses the word boundary
        cell = ref.seed_cell(ref.fixture_seed(name), 96, 130, ref.RES, ref.ORIGIN)
        assert cell is not None and free[cell], name
    b = ref.free_from_image(FIX["border_ring"])
    assert b[0].all() and b[-1].all() and b[:, 0].all() and b[:, -1].all()


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_loops(results, name):
    cells, hw, deleted, final, T = results[name]
    assert len(cells) == LOOPS[name]
    assert int(final.sum()) == LOOPS[name]                    # spurs and blobs erase to nothing: the loop is all that is left
    assert np.all(degrees(final) == 2)
    assert len({(int(r), int(c)) for r, c in cells}) == len(cells) and np.all(final[cells[:, 0], cells[:, 1]])
    step = np.abs(np.roll(cells, -1, axis=0) - cells).max(axis=1)
    assert np.all(step == 1)                                   # consecutive cells are 8-neighbours, the closing step included
    free = ref.free_from_image(FIX[name])
    assert int(free.sum()) - int(deleted.sum()) == int(final.sum())
    assert np.array_equal(hw, T[cells[:, 0], cells[:, 1]]) and np.all(hw > 0)      # half_width IS T at the cell
    area2 = sum(int(c0) * int(r1) - int(c1) * int(r0) for (r0, c0), (r1, c1) in zip(cells, np.roll(cells, -1, axis=0)))
    assert area2 > 0                                           # counter-clockwise without a heading


def test_spurs_and_blob_leave_the_annulus_loop(results):
    base = results["annulus_w10"][0]
    for name in ("annulus_spur", "annulus_spurs3", "annulus_blob"):
        assert len(results[name][0]) == len(base), name
    assert np.array_equal(results["annulus_blob"][0], base) and np.array_equal(results["annulus_blob"][3], results["annulus_w10"][3])
    assert results["annulus_blob"][2][2] == 1                  # the blob thins to one cell, which pruning erases


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused(results, name):
    assert isinstance(results[name], ref.Refused) and results[name].kind == REFUSED[name], results[name]
    if name == "straight":
        free = ref.free_from_image(FIX[name])
        assert not ref.skeleton(free)[0].any()                 # pruned to nothing
    if name == "annulus_spur_diamond":
        assert results[name].info == dict(branching=5, members=177)


def test_bad_seeds_and_max_passes():
    free = ref.free_from_image(FIX["annulus_w10"])
    T = free.astype(np.float64)
    for seed in (ref.cell_world(48, 64), ref.cell_world(2, 2), (-3.0 - 1e-9, 0.0), (-3.0 + 130 * ref.RES, 0.0), (0.0, 100.0), (np.nan, 0.0), (0.0, np.inf)):
        with pytest.raises(ref.Refused) as ei:
            ref.centerline(free, T, ref.RES, ref.ORIGIN, seed)
        assert ei.value.kind == 'seed', seed
    _, _, passes = ref.skeleton(free)
    with pytest.raises(ref.Refused) as ei:
        ref.skeleton(free, max_passes=passes[0] - 1)
    assert ei.value.kind == 'not_converged'
    assert np.array_equal(ref.skeleton(free, max_passes=max(passes))[0], ref.skeleton(free)[0])


def test_component_only_gives_the_same_loop(results):
    name = "annulus_blob"
    free = ref.free_from_image(FIX[name])
    cells = ref.centerline(free, results[name][4], ref.RES, ref.ORIGIN, ref.fixture_seed(name), whole=False)[0]
    assert np.array_equal(cells, results[name][0])


def test_heading_reverses_the_order(results):
    name = "annulus_w10"
    free, T = ref.free_from_image(FIX[name]), results[name][4]
    ccw = results[name][0]
    a = ref.centerline(free, T, ref.RES, ref.ORIGIN, ref.fixture_seed(name), heading=-0.5 * np.pi)[0]   # down the left arm: counter-clockwise
    b = ref.centerline(free, T, ref.RES, ref.ORIGIN, ref.fixture_seed(name), heading=0.5 * np.pi)[0]
    assert np.array_equal(a, ccw)
    assert np.array_equal(b[0], ccw[0]) and np.array_equal(b[1:], ccw[1:][::-1])
    rot = (ref.ORIGIN[0], ref.ORIGIN[1], 0.5 * np.pi)          # a rotated origin turns the heading with it
    seed = ref.cell_world(47, 34, origin=rot)
    c = ref.centerline(free, T, ref.RES, rot, seed, heading=0.0)[0]
    assert np.array_equal(c, ccw)


@pytest.mark.parametrize("name, width, centre", ref.ANNULI)
def test_radial_quality(results, name, width, centre):
    cells = results[name][0]
    # the image's centre in table coordinates: row H - centre_row (cell centres at + 0.5)
    rc, cc = 96 - centre[0], centre[1]
    d = np.sqrt((cells[:, 0] + 0.5 - rc) ** 2 + (cells[:, 1] + 0.5 - cc) ** 2)
    worst = float(np.abs(d - 30.0).max())
    print("%s: largest radial distance from the mid circle %.3f cells" % (name, worst))
    assert worst <= min(RADIAL[name] + 0.25, 2.0)


# ---- the host post-processing ---------------------------------------------------------------------------------------------------
def test_track_from_cells_matches_the_restatement(results):
    from f1tenth_gym_amd.centerline import track_from_cells
    for name, spacing, smooth, yaw in (("annulus_w10", 0.2, 1.0, 0.0), ("rect_w12", 0.13, 0.4, 0.3), ("border_ring", 0.5, 0.0, -1.1)):
        cells, hw = results[name][0], results[name][1]
        frame = (ref.RES, ref.ORIGIN[0], ref.ORIGIN[1], float(np.cos(yaw)), float(np.sin(yaw)))
        track, det = track_from_cells(cells, hw, frame, spacing=spacing, smooth=smooth, details=True)
        pts, w, kappa, st, L = ref.post_process(cells, hw, frame, spacing, smooth)
        assert track.closed and track.attr_names == ('half_width', 'kappa') and track.num_points == len(pts)
        assert np.allclose(track.xy, pts, rtol=0, atol=1e-12) and np.allclose(track.attrs[:, 0], w, rtol=0, atol=1e-12)
        assert np.allclose(track.attrs[:, 1], kappa, rtol=1e-9, atol=1e-9)
        # uniform in the arc length of the smoothed line, and it closes: M steps of L / M
        ds = np.diff(np.append(det["stations"], det["length"]))
        assert np.all(np.abs(ds - ds[0]) <= 1e-9 * ds[0]) and abs(ds[0] * len(ds) - L) <= 1e-9 * L
        assert abs(ds[0] - spacing) <= 0.5 * spacing * spacing / L + 1e-12     # L / round(L / spacing)
        assert np.allclose(det["stations"], st, rtol=0, atol=1e-12)
        assert np.all(track.seg_len <= ds[0] * (1 + 1e-12)) and np.all(track.seg_len >= 0.7 * ds[0])   # chords of equal arcs
        assert np.all(w > 0) and w.min() >= hw.min() and w.max() <= hw.max()
        if smooth == 0.0:
            assert det["window"] == 0 and np.array_equal(det["smoothed"], det["raw"])
    # a circle's curvature: the annulus, smoothed, turns left at about 1 / (30 cells)
    cells, hw = results["annulus_w10"][0], results["annulus_w10"][1]
    track = track_from_cells(cells, hw, (ref.RES, 0.0, 0.0, 1.0, 0.0), spacing=0.2, smooth=1.0)
    assert abs(float(np.mean(track.attrs[:, 1])) - 1.0 / (30 * ref.RES)) < 0.05 / (30 * ref.RES)


def test_track_from_cells_refuses():
    from f1tenth_gym_amd.centerline import track_from_cells, coerce_params
    cells = np.array([[0, 0], [0, 1], [1, 1], [1, 0]])
    fr = (0.1, 0.0, 0.0, 1.0, 0.0)
    for kw in (dict(spacing=0.0), dict(spacing=np.nan), dict(smooth=-1.0)):
        with pytest.raises(ValueError):
            track_from_cells(cells, np.ones(4), fr, **kw)
    with pytest.raises(ValueError):
        track_from_cells(cells[:2], np.ones(2), fr)
    with pytest.raises(ValueError):
        coerce_params(dict(sed=(0, 0)))
    assert coerce_params(dict(spacing=0.5))["spacing"] == 0.5 and coerce_params(None)["seed"] == (0.0, 0.0)


# ---- the per-word decisions, compiled for the host ------------------------------------------------------------------------------
def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


needs_hipcc = pytest.mark.skipif(not os.path.isfile(hipcc()), reason="hipcc not installed")
SRC = os.path.join(HERE, "host_harness", "centerline_main.hip")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("centerline_main") / "centerline_main")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", SRC, "-o", exe], stdout=subprocess.DEVNULL,
                          stderr=subprocess.DEVNULL)
    return exe


def run_program(exe, tmp, free, max_passes=0):
    H, W = free.shape
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([H, W, max_passes], dtype=np.int32).tobytes() + np.ascontiguousarray(free, dtype=np.uint8).tobytes())
    subprocess.check_call([exe, src, dst])
    raw = open(dst, "rb").read()
    head = np.frombuffer(raw[:32], dtype=np.int64)
    return np.frombuffer(raw[32:], dtype=np.uint8).reshape(H, W).astype(bool), head[:3], bool(head[3])


@needs_hipcc
def test_host_program_equals_reference(program, tmp_path):
    rng = np.random.default_rng(5)
    cases = [(name, ref.free_from_image(img)) for name, img in sorted(FIX.items())]
    for W in (1, 63, 64, 65, 127, 128, 129):                   # random blobs at the widths around the word size
        cases.append(("random %d" % W, rng.random((37, W)) < 0.7))
    cases.append(("full", np.ones((40, 130), dtype=bool)))
    cases.append(("empty", np.zeros((5, 70), dtype=bool)))
    for name, free in cases:
        want, deleted, _ = ref.skeleton(free)
        got, d, ok = run_program(program, tmp_path, free)
        assert ok and np.array_equal(got, want), name
        assert np.array_equal(d, deleted), name
    free = ref.free_from_image(FIX["annulus_w13"])
    passes = ref.skeleton(free)[2]
    assert run_program(program, tmp_path, free, passes[0])[2] and not run_program(program, tmp_path, free, passes[0] - 1)[2]


@needs_hipcc
def test_host_program_under_host_sanitizers(tmp_path):
    """the program's self-check (rings at the widths around the word size) built for the HOST with the address and
    undefined-behaviour sanitizers; nothing is loaded into Python"""
    exe = str(tmp_path / "centerline_main_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", SRC, "-o", exe], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout.startswith("ok: 7 rings"), proc.stdout
