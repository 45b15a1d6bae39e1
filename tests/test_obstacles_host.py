"""CPU checks of the static obstacles: Obstacles' validation, the struct layout against the header, random_on_track,
the NumPy model (tests/obstacles_ref.py) — its min identity against a full rebuild of the table on both fixtures — and the host
instantiation of f110_math.hpp's obstacle_hit / obstacle_cell_box (tests/host_harness/obstacles_harness.hip) against the model's
mask, bit for bit.  The GPU tests (tests/test_gpu_obstacles.py) hold the kernels to the same model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import obstacles_ref as ref
from _util import load_map_image
from f1tenth_gym_amd import Obstacles, Track, _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
NAN, INF = float("nan"), float("inf")
ROW = [0.0, 1.0, 2.0, 1.0, 0.0, 0.3, 0.2]


def row(**kw):
    r = list(ROW)
    for k, v in kw.items():
        r[("shape", "x", "y", "c", "s", "half_length", "half_width").index(k)] = v
    return [r]


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [
    row(shape=2.0), row(shape=-1.0), row(shape=0.5), row(x=NAN), row(y=INF), row(c=NAN), row(s=-INF), row(half_length=NAN),
    row(half_width=INF), row(half_length=-0.1), row(half_width=-1e-300), [ROW] * 257,
])
def test_obstacles_refuses(rows):
    with pytest.raises(ValueError):
        Obstacles(rows)


def test_obstacles_constructors_and_immutability():
    with pytest.raises(ValueError):
        Obstacles.boxes([[0, 0], [1, 1]], [0.1, 0.2, 0.3], 0.4, 0.2)
    with pytest.raises(ValueError):
        Obstacles.discs([[0, 0]], -0.1)
    with pytest.raises(ValueError):
        Obstacles.boxes([[0, 0]] * 200, 0.0, 0.1, 0.1) + Obstacles.discs([[0, 0]] * 57, 0.1)
    with pytest.raises(TypeError):
        Obstacles() + 3
    b = Obstacles.boxes([[1.0, 2.0], [3.0, 4.0]], [0.0, 0.5], 0.6, [0.2, 0.4])
    assert b.rows.tolist() == [[0.0, 1.0, 2.0, 1.0, 0.0, 0.3, 0.1], [0.0, 3.0, 4.0, float(np.cos(0.5)), float(np.sin(0.5)), 0.3, 0.2]]
    d = Obstacles.discs([5.0, 6.0], 0.25)
    assert d.rows.tolist() == [[1.0, 5.0, 6.0, 1.0, 0.0, 0.25, 0.0]]
    both = b + d
    assert len(both) == 3 and len(Obstacles()) == 0 and both == Obstacles(both.rows) and both != b and Obstacles.coerce(None) == Obstacles()
    assert Obstacles.coerce(both) is both and Obstacles().structs() is None
    with pytest.raises(AttributeError):
        both.extra = 1
    with pytest.raises(ValueError):
        both.rows[0, 1] = 9.0
    st = both.structs()
    assert len(st) == 3 and (st[1].shape, st[1].x, st[1].y, st[1].half_width) == (0, 3.0, 4.0, 0.2) and (st[2].shape, st[2].half_length) == (1, 0.25)
    assert len(Obstacles([ROW] * 256)) == 256


def test_struct_and_enums_match_the_header():
    with open(os.path.join(os.path.dirname(HERE), "include", "f110.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct f110_obstacle \{(.*?)\} f110_obstacle;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for t, names in re.findall(r"(int32_t|double)\s+([\w\s,]+);", body):
        fields += [(t, n.strip()) for n in names.split(",")]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    S = _ffi.Obstacle
    assert [(n, ctype[t]) for t, n in fields] == list(S._fields_)
    assert C.sizeof(S) == 56
    assert [getattr(S, n).offset for n, _ in S._fields_] == [0, 4, 8, 16, 24, 32, 40, 48]
    enums = dict(re.findall(r"(F110_OBST_BOX|F110_OBST_DISC|F110_MAX_OBSTACLES) = (\d+)", src))
    assert (int(enums["F110_OBST_BOX"]), int(enums["F110_OBST_DISC"]), int(enums["F110_MAX_OBSTACLES"])) == (_ffi.OBST_BOX, _ffi.OBST_DISC, _ffi.MAX_OBSTACLES) == (0, 1, 256)


# ---- random_on_track ---------------------------------------------------------------------------------------------------------
def test_track_point_at():
    t = Track([[0.0, 0.0], [4.0, 0.0], [4.0, 3.0]])   # closed: 4 + 3 + 5
    p, tan = t.point_at([0.0, 1.0, 4.0, 5.5, 7.0, 9.5, 12.0, 13.0, -1.0])
    assert t.length == 12.0
    np.testing.assert_allclose(p, [[0, 0], [1, 0], [4, 0], [4, 1.5], [4, 3], [2, 1.5], [0, 0], [1, 0], [0.8, 0.6]], atol=1e-12)
    np.testing.assert_allclose(tan[[0, 3, 5]], [[1, 0], [0, 1], [-0.8, -0.6]], atol=1e-12)
    o = Track([[0.0, 0.0], [4.0, 0.0]], closed=False)
    assert o.point_at([-1.0, 2.0, 9.0])[0].tolist() == [[0.0, 0.0], [2.0, 0.0], [4.0, 0.0]]


def test_random_on_track():
    track = ref.example_track()
    L = track.length
    kw = dict(s_range=(0.1, 0.9), lateral=0.4, keep_clear=[(0.3, 0.45), (0.7, 0.72)], min_gap=5.0)
    a, sa = Obstacles.random_on_track(track, 14, 11, return_s=True, **kw)
    b, sb = Obstacles.random_on_track(track, 14, 11, return_s=True, **kw)
    c = Obstacles.random_on_track(track, 14, 12, **kw)
    assert a == b and sa.tolist() == sb.tolist() and a != c and len(a) == 14
    assert a == Obstacles.random_on_track(track, 14, 11, **kw)
    f = sa / L
    assert np.all((f >= 0.1) & (f <= 0.9)) and not np.any((f >= 0.3) & (f <= 0.45)) and not np.any((f >= 0.7) & (f <= 0.72))
    assert np.all(np.diff(sa) >= 5.0)
    # every centre lies within the lateral bound of the track's point at its s, hence of the track
    p, tan = track.point_at(sa)
    off = a.xy - p
    assert np.all(np.abs(off[:, 0] * tan[:, 0] + off[:, 1] * tan[:, 1]) < 1e-9)
    assert np.all(np.hypot(off[:, 0], off[:, 1]) <= 0.4 + 1e-9)
    assert np.all(np.abs(track.project(np.column_stack([a.xy, np.zeros(14)]))[:, 1]) <= 0.4 + 1e-9)
    # a wrapped keep_clear stretch and the closing gap of a closed track
    w, sw = Obstacles.random_on_track(track, 10, 5, keep_clear=[(0.9, 0.1)], min_gap=8.0, return_s=True)
    assert np.all((sw / L > 0.1) & (sw / L < 0.9)) and np.all(np.diff(sw) >= 8.0) and sw[0] + L - sw[-1] >= 8.0
    # shapes: all discs / all boxes, sizes inside their ranges
    d = Obstacles.random_on_track(track, 6, 1, disc_fraction=1.0, radius=(0.1, 0.2))
    assert np.all(d.rows[:, 0] == 1) and np.all((d.rows[:, 5] >= 0.1) & (d.rows[:, 5] <= 0.2))
    bx = Obstacles.random_on_track(track, 6, 1, disc_fraction=0.0, length=0.5, width=(0.2, 0.3))
    assert np.all(bx.rows[:, 0] == 0) and np.all(bx.rows[:, 5] == 0.25) and np.all((bx.rows[:, 6] >= 0.1) & (bx.rows[:, 6] <= 0.15))
    assert len(Obstacles.random_on_track(track, 0, 1)) == 0
    for bad in (dict(n=300), dict(n=5, s_range=(0.5, 0.5)), dict(n=5, lateral=-1.0), dict(n=5, disc_fraction=1.5), dict(n=5, radius=(0.2, 0.1)),
                dict(n=200, min_gap=10.0)):
        with pytest.raises(ValueError):
            Obstacles.random_on_track(track, seed=1, **bad)


# ---- the model ---------------------------------------------------------------------------------------------------------------
def fixtures():
    """(name, image, resolution, origin, [obstacle lists])"""
    img, res, origin = load_map_image("example_map")
    return [("small", ref.small_image(), ref.SMALL_RES, ref.SMALL_ORIGIN, [ref.small_obstacles(0), ref.small_obstacles(1)]),
            ("example_map", img, res, origin, [ref.large_obstacles()])]


def test_fixture_conditions():
    """what the issue asks of the fixtures: no cell centre within 1e-9 m of a shape's boundary; the small one stamps the far corner
    cell, has a shape partly and one wholly outside the table"""
    for name, img, res, origin, lists in fixtures():
        H, W = img.shape
        for ob in lists:
            assert ref.boundary_margin(ob, H, W, res, origin) > 1e-9, name
    H, W = ref.SMALL_H, ref.SMALL_W
    ob = ref.small_obstacles(0)
    assert len(ob) == 10 and ref.free_from_image(ref.small_image())[H - 1, W - 1]
    m = ref.stamp_mask(ob, H, W, ref.SMALL_RES, ref.SMALL_ORIGIN)
    assert m[H - 1, W - 1]
    per = [int(ref.stamp_mask(Obstacles(ob.rows[i:i + 1]), H, W, ref.SMALL_RES, ref.SMALL_ORIGIN).sum()) for i in range(len(ob))]
    assert per[6] == 0 and 0 < per[5] < per[0]
    assert len(ref.large_obstacles()) == 12


def test_model_min_identity_equals_full_rebuild():
    for name, img, res, origin, lists in fixtures():
        free = ref.free_from_image(img)
        base = ref.table_from_bitmap(free, res)
        for ob in lists:
            t, m = ref.derived_table(base, ob, res, origin)
            full = ref.table_from_bitmap(ref.free_from_image(ref.image_with_stamps(img, m)), res)
            assert np.array_equal(t, full), name
            assert (t != base).sum() > 200 and t[-1, -1] == full[-1, -1]
        t, m = ref.derived_table(base, Obstacles(), res, origin)
        assert not m.any() and np.array_equal(t, base)


# ---- the host instantiation of the stamp ----------------------------------------------------------------------------------------
def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "obstacles_harness.hip")
    lib = str(tmp_path_factory.mktemp("obstacles_harness") / "libobstacles_harness.so")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness_mask(hh, ob, H, W, res, origin, whole=False):
    mask = np.empty((H, W), dtype=np.uint8)
    boxes = np.full((max(len(ob), 1), 4), -7, dtype=np.int32)
    hh.hh_obstacles_stamp.restype = None
    hh.hh_obstacles_stamp.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_double] * 5 + [C.c_int, C.c_void_p, C.c_void_p]
    hh.hh_obstacles_stamp(ob.structs(), len(ob), H, W, float(res), float(origin[0]), float(origin[1]), float(np.cos(origin[2])), float(np.sin(origin[2])),
                          int(whole), mask.ctypes.data, boxes.ctypes.data)
    return mask, boxes


@needs_hipcc
def test_harness_stamp_equals_model_mask(hh):
    for name, img, res, origin, lists in fixtures():
        H, W = img.shape
        for ob in lists:
            want = ref.stamp_mask(ob, H, W, res, origin)
            got, boxes = harness_mask(hh, ob, H, W, res, origin)
            assert np.array_equal(got.astype(bool), want), name
            assert np.array_equal(harness_mask(hh, ob, H, W, res, origin, whole=True)[0], got), name
            # the cell boxes stay inside the table and are tight enough to be worth having
            live = boxes[boxes[:, 0] <= boxes[:, 1]]
            assert np.all(live[:, 0] >= 0) and np.all(live[:, 1] <= W - 1) and np.all(live[:, 2] >= 0) and np.all(live[:, 3] <= H - 1)
            cols = np.zeros(W, dtype=bool)
            for c0, c1, r0, r1 in live:
                if r0 <= r1:
                    cols[c0:c1 + 1] = True
            assert np.all(cols[want.any(axis=0)]) and cols.sum() <= want.any(axis=0).sum() + 8 * len(ob)


@needs_hipcc
def test_harness_standalone_under_host_sanitizers(tmp_path):
    """the stamp and the cell box as a stand-alone program (its own main: boxes and discs inside, across and far outside a table,
    extreme sizes included) built for the HOST with the address and undefined-behaviour sanitizers; nothing is loaded into Python"""
    src = os.path.join(HERE, "host_harness", "obstacles_harness.hip")
    exe = str(tmp_path / "obstacles_harness_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-DOBST_HARNESS_MAIN",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout.startswith("ok: 1000 obstacles"), proc.stdout


# ---- the fixtures for the kernels' edges (tests/test_gpu_obstacles_edges.py runs them on the device) ----------------------------
def edge_cases():
    """(fixture name, image, resolution, origin, list label, Obstacles, promised stamped-column count) of every new table and list"""
    return [(name, img, res, origin, label, ob, cols) for name, img, res, origin, lists in ref.edge_fixtures() for label, ob, cols in lists]


def promised(cols, n):
    return True if cols is None else (n == cols if isinstance(cols, int) else cols[0] <= n <= cols[1])


def test_edge_fixture_conditions():
    """the margin of every list, the stamped-column counts the kernels' paths hang on, and what each table is there for"""
    seen = {}
    for name, img, res, origin, label, ob, cols in edge_cases():
        H, W = img.shape
        if label != "1e200 disc" and len(ob):   # (that disc's boundary is nowhere near the table)
            assert ref.boundary_margin(ob, H, W, res, origin) > 1e-9, (name, label)
        m = ref.stamp_mask(ob, H, W, res, origin)
        n = ref.stamped_columns(m)
        assert promised(cols, n), (name, label, n, cols)
        seen[(name, label)] = (m, n)
        free = ref.free_from_image(img)
        assert free[H - 1, W - 1] and (H * W == 1 or not free.all()), name   # a base with occupied cells: the minimum with it matters
    # three chunks of 2048 active columns, 17 strides of 256 and 66 workgroups of 64; exactly one chunk, and one more column
    assert seen[("bar4200", "bar and discs")][1] == 4200 == 2 * 2048 + 104 and -(-4200 // 256) == 17 and -(-4200 // 64) == 66
    assert seen[("bar2048", "bar and discs")][1] == 2048 and seen[("bar2049", "bar and discs")][1] == 2049
    assert 300 <= seen[("mid", "mid")][1] <= 1500 and seen[("mid", "mid")][1] < 1500 - 300   # several strides, one short chunk, free columns left
    m = seen[("tall", "tall")][0]
    assert m[:6].any() and m[-6:].any() and not m[6:-6].any() and m.shape[0] > 2048
    # the edge widths: computed from the border's formula for every max_range the device test constructs
    borders = [ref.pad_border(mr, ref.EDGE_RES) for mr in ref.EDGE_MAX_RANGES]
    assert sorted(b % 256 for b in borders) == [0, 186, 255]
    for mr, b in zip(ref.EDGE_MAX_RANGES, borders):
        ws = ref.edge_widths(mr)
        assert [(b + w) % 256 for w in ws] == [0, 1, 255, 0] and (b + ws[3] - 1) // 256 - b // 256 >= 2
        for w in ws:
            m = seen[("edge%d" % w, "edge")][0]
            assert m[:, 0].any() and m[:, w - 1].any() and not m[-1, -1], w
    assert ref.edge_fixture(70)[3][2] != 0.0 and all(f[3][2] != 0.0 for f in ref.tiny_fixtures())
    # the tiny tables and the lists on the small one
    assert seen[("tiny1x1", "stamps")][0].all() and seen[("tiny1x300", "stamps")][1] > 0 and seen[("tiny300x1", "stamps")][0].sum() > 1
    assert [len(ob) for _, ob, _ in ref.small_lists()[:4]] == [256, 255, 1, 0]
    assert seen[("small", "256")][0].sum() > 3000 and seen[("small", "1")][0].any() and seen[("small", "1e200 disc")][0].all()
    each = sum(int(ref.stamp_mask(Obstacles(ref.small_lists()[0][1].rows[i:i + 1]), ref.SMALL_H, ref.SMALL_W, ref.SMALL_RES, ref.SMALL_ORIGIN).sum()) for i in range(256))
    assert each > 1.25 * seen[("small", "256")][0].sum()   # many overlap: the shapes' own cell counts add up to more than 1.25 times their union
    for label in ("0", "zero box", "outside"):
        assert not seen[("small", label)][0].any()
    assert np.all(ref.small_lists()[4][1].rows[0, 5:] == 0.0)


def test_edge_model_min_identity_equals_full_rebuild():
    for name, img, res, origin, label, ob, cols in edge_cases():
        base = ref.table_from_bitmap(ref.free_from_image(img), res)
        t, m = ref.derived_table(base, ob, res, origin)
        full = ref.table_from_bitmap(ref.free_from_image(ref.image_with_stamps(img, m)), res)
        assert np.array_equal(t, full), (name, label)
        assert (m.any() and not np.array_equal(t, base)) or (not m.any() and np.array_equal(t, base)), (name, label)
    assert ref.derived_table(base, ref.small_lists()[5][1], res, origin)[0].max() == 0.0   # the 1e200 disc: all zeros, out-of-bounds value 0


@needs_hipcc
def test_harness_stamp_equals_model_mask_on_edge_fixtures(hh):
    """the host instantiation's mask against the model's on every new table and list, and the ACTIVE column count Wa (the union of
    the non-empty cell boxes' column ranges, as obstacles_stamp forms it): W on the bar tables and under the 1e200 disc (the `wild`
    branch: the whole table), 0 for the empty list and for shapes that all lie outside, above 0 where a cell box reaches the table
    and nothing is stamped"""
    wa = {}
    for name, img, res, origin, label, ob, cols in edge_cases():
        H, W = img.shape
        want = ref.stamp_mask(ob, H, W, res, origin)
        got, boxes = harness_mask(hh, ob, H, W, res, origin)
        assert np.array_equal(got.astype(bool), want), (name, label)
        assert np.array_equal(harness_mask(hh, ob, H, W, res, origin, whole=True)[0], got), (name, label)
        live = boxes[:len(ob)]
        live = live[(live[:, 0] <= live[:, 1]) & (live[:, 2] <= live[:, 3])]
        assert np.all(live[:, 0] >= 0) and np.all(live[:, 1] <= W - 1) and np.all(live[:, 2] >= 0) and np.all(live[:, 3] <= H - 1)
        active = np.zeros(W, dtype=bool)
        for c0, c1, r0, r1 in live:
            active[c0:c1 + 1] = True
        assert np.all(active[want.any(axis=0)]), (name, label)
        wa[(name, label)] = int(active.sum())
    assert (wa[("bar4200", "bar and discs")], wa[("bar2048", "bar and discs")], wa[("bar2049", "bar and discs")]) == (4200, 2048, 2049)
    assert 256 < wa[("mid", "mid")] < 1500 and 0 < wa[("bar4200", "discs only")] < 256
    assert wa[("small", "1e200 disc")] == ref.SMALL_W and wa[("small", "0")] == wa[("small", "outside")] == 0
    assert wa[("small", "zero box")] > 0 and wa[("tiny1x300", "stamps none")] > 0 and wa[("tiny300x1", "stamps none")] == 1


def test_rollout_case_on_the_derived_slot():
    """the candidates of the rollout tests (tests/test_gpu_obstacles_edges.py), on the model alone: none comes within 1e-9 m of the
    margin; some die in list 0's shapes, some pass where list 1 has one, and those that leave the table die with list 0 (whose
    out-of-bounds value is 0.0) and survive with list 1 (0.7000000000000001)"""
    assert ref.rollout_table(0)[-1, -1] == 0.0 and ref.rollout_table(1)[-1, -1] == 0.7000000000000001 == ref.rollout_table("base")[-1, -1]
    assert 0.0 < ref.ROLL_MARGIN < 0.7
    steps = ref.ROLL_H * ref.ROLL_REPEAT
    alive = {w: ref.rollout_flown(w)[1] for w in ("base", 0, 1)}
    for w in ("base", 0, 1):
        assert np.all(ref.rollout_flown(w)[4] >= 1e-9), w                      # the model leaves out no candidate
    corridor = np.arange(13)
    assert np.count_nonzero(alive[0][corridor] < alive["base"][corridor]) >= 16     # die in one of list 0's shapes
    assert np.count_nonzero((alive[1][corridor] < alive["base"][corridor]) & (alive[0][corridor] == alive["base"][corridor])) >= 8   # pass where list 1 has one
    assert np.count_nonzero((alive[0][corridor] < alive["base"][corridor]) & (alive[1][corridor] == alive["base"][corridor])) >= 8
    assert np.count_nonzero(alive["base"] == steps) >= 16 and np.count_nonzero(alive["base"][corridor] < steps) >= 16
    out = ref.rollout_left_table(1)
    assert np.count_nonzero(out) >= 20 and not out[corridor].any() and out[list(ref.ROLL_LEAVERS)].sum() == out.sum()
    assert np.all(alive[1][out] == steps) and np.all(alive["base"][out] == steps) and np.all(alive[0][out] < steps)
