"""CPU checks of the neighbour observation: the settings' validation, the struct layout, the Python model
(tests/neighbors_ref.py) on cases worked out by hand on integer coordinates, Neighbors.compute (NumPy) against the model, and the
host instantiation of f110_math.hpp's nbr_* functions (tests/host_harness/neighbors_harness.hip) against the model over the grid.
The GPU tests (tests/test_gpu_neighbors.py) hold the kernel to the same model."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import neighbors_ref as ref
from f1tenth_gym_amd import Neighbors, _ffi
from f1tenth_gym_amd import neighbors as nbm

HERE = os.path.dirname(os.path.abspath(__file__))
_dp = C.POINTER(C.c_double)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")
NAN, INF = float("nan"), float("inf")
ALL10 = ref.CHANNELS


# ---- validation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(k=0), dict(k=9), dict(k=-1), dict(k=2.5), dict(k=True),
    dict(channels=()), dict(channels=("dx", "speed")), dict(channels=("dx", "dx")), dict(channels=("attr0",)),
    dict(max_range=0.0), dict(max_range=-1.0), dict(max_range=np.nan), dict(max_range=-np.inf),
    dict(pad=np.inf), dict(pad=np.nan), dict(pad=-np.inf),
    dict(scale={"dx": 0.0}), dict(scale={"dy": np.inf}), dict(scale={"dx": np.nan}), dict(scale={"speed": 1.0}),
])
def test_neighbors_validation_refuses(kw):
    with pytest.raises(ValueError):
        Neighbors(**kw)


def test_neighbors_defaults_struct_and_coerce():
    p = Neighbors()
    assert (p.k, p.channels, p.max_range, p.pad, p.dim) == (1, ("dx", "dy"), INF, 0.0, 2)
    assert p.shape(6) == (6, 1, 2) and not p.needs_track
    sp = p.spec()
    assert (sp.k, sp.channels, sp.flags, sp.max_range, sp.pad) == (1, 3, 0, INF, 0.0) and list(sp.scale) == [1.0] * 10
    q = Neighbors(k=8, channels=("index", "gap_s", "dx"), max_range=12.5, pad=-1.0, scale={"dx": 10.0, "gap_s": -2.0, "dy": 0.0})
    assert q.channels == ("dx", "gap_s", "index") and q.channel_mask == 1 | 128 | 512 and q.needs_track   # (a clear bit's scale is ignored)
    assert list(q.spec().scale) == [10.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, -2.0, 1.0, 1.0] and q.spec().max_range == 12.5 and q.spec().pad == -1.0
    # struct f110_neighbors: 4 int32, 2 double, 10 double
    S = _ffi.NeighborsSpec
    assert C.sizeof(S) == 4 * 4 + 2 * 8 + 10 * 8
    assert (S.k.offset, S.channels.offset, S.flags.offset, S.pad_.offset, S.max_range.offset, S.pad.offset, S.scale.offset) == (0, 4, 8, 12, 16, 24, 32)
    assert [_ffi.NBR_DX, _ffi.NBR_DY, _ffi.NBR_DIST, _ffi.NBR_COS_DTH, _ffi.NBR_SIN_DTH, _ffi.NBR_V_X, _ffi.NBR_V_Y, _ffi.NBR_GAP_S,
            _ffi.NBR_VALID, _ffi.NBR_INDEX] == [1 << b for b in range(10)]
    assert (_ffi.NBR_NCHANNELS, _ffi.NBR_MAX_K) == (10, 8) and nbm.CHANNELS == ref.CHANNELS
    assert Neighbors.coerce(dict(k=3)).k == 3 and Neighbors.coerce(p) is p
    assert Neighbors(**q.settings()).settings() == q.settings()
    with pytest.raises(TypeError):
        Neighbors.coerce(7)


def test_struct_and_enums_match_the_header():
    """the struct's fields in the header's order and types, and the enum values, read from include/f110.h"""
    with open(os.path.join(os.path.dirname(HERE), "include", "f110.h")) as f:
        src = f.read()
    body = re.search(r"typedef struct f110_neighbors \{(.*?)\} f110_neighbors;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [(t, n) for t, n in re.findall(r"(int32_t|double)\s+(\w+)(?:\[\w+\])?;", body)]
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    mirror = _ffi.NeighborsSpec._fields_
    assert [n for _, n in fields] == [n for n, _ in mirror]
    for (t, n), (_, ct) in zip(fields, mirror):
        assert ct is ctype[t] or (n == "scale" and ct._type_ is C.c_double and ct._length_ == 10), n
    enums = dict(re.findall(r"(F110_NBR_[A-Z_]+) = (\d+)", src))
    names = ["DX", "DY", "DIST", "COS_DTH", "SIN_DTH", "V_X", "V_Y", "GAP_S", "VALID", "INDEX"]
    assert [int(enums["F110_NBR_" + n]) for n in names] == [1 << b for b in range(10)]
    assert (int(enums["F110_NBR_NCHANNELS"]), int(enums["F110_NBR_MAX_K"])) == (10, 8)


def test_vec_env_argument_checks():
    """raised before a simulator is made"""
    from f1tenth_gym_amd import F110VecEnv
    from _util import MAPS
    csv = os.path.join(MAPS, "example_waypoints.csv")
    with pytest.raises(ValueError, match="neighbors_device"):
        F110VecEnv(2, neighbors=Neighbors(), map="example_map")
    with pytest.raises(ValueError, match="needs a track"):
        F110VecEnv(2, neighbors=dict(channels=("dx", "gap_s")), device_logic=True, map="example_map")
    with pytest.raises(ValueError):
        F110VecEnv(2, neighbors=dict(k=0), device_logic=True, track=csv, map="example_map")
    with pytest.raises(TypeError):
        F110VecEnv(2, neighbors=3, device_logic=True, map="example_map")


# ---- cases worked out by hand on integer coordinates --------------------------------------------------------------------------
def rows_of(xy, theta=0.0, v=0.0, s=0.0):
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    n = xy.shape[0]
    col = lambda q: np.broadcast_to(np.asarray(q, dtype=np.float64), (n,))   # noqa: E731
    return np.ascontiguousarray(np.column_stack([xy, col(theta), col(v), col(s)]))


SQUARE = [[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 1.0]]


def both(s, rows, A, L=0.0):
    """the model's and Neighbors.compute's (out, raw, idx), after holding them to each other bit for bit"""
    want = ref.neighbors(s, rows, A, L)
    got = Neighbors(**s).compute(rows[:, :3], rows[:, 3], rows[:, 4], A, L, raw=True, indices=True)
    for w, g in zip(want, got):
        assert w.shape == g.shape and w.dtype == g.dtype and np.ascontiguousarray(w).tobytes() == np.ascontiguousarray(g).tobytes()
    return want


def test_hand_unit_square_ties_go_to_the_lower_index():
    s = ref.settings(k=3, channels=ALL10)
    rows = rows_of(SQUARE, v=[1.0, 2.0, 3.0, 4.0], s=[0.0, 1.0, 2.0, 3.0])
    out, raw, idx = both(s, rows, 4)
    # every corner has two neighbours at d2 = 1 (the lower index first) and the opposite corner at d2 = 2
    assert idx.tolist() == [[1, 3, 2], [0, 2, 3], [1, 3, 0], [0, 2, 1]]
    assert raw[..., ref.DIST].tolist() == [[1.0, 1.0, np.sqrt(2.0)]] * 4
    # car 0 at the origin heading +x: car 1 is 1 m ahead, car 3 1 m to the left, car 2 ahead and to the left
    assert raw[0, :, ref.DX].tolist() == [1.0, 0.0, 1.0] and raw[0, :, ref.DY].tolist() == [0.0, 1.0, 1.0]
    assert raw[0, :, ref.COS_DTH].tolist() == [1.0] * 3 and raw[0, :, ref.SIN_DTH].tolist() == [0.0] * 3
    assert raw[0, :, ref.V_X].tolist() == [1.0, 3.0, 2.0] and raw[0, :, ref.V_Y].tolist() == [0.0] * 3
    assert raw[0, :, ref.GAP_S].tolist() == [1.0, 3.0, 2.0] and raw[0, :, ref.VALID].tolist() == [1.0] * 3 and raw[0, :, ref.INDEX].tolist() == [1.0, 3.0, 2.0]
    assert out.dtype == np.float32 and np.array_equal(out, raw.astype(np.float32))
    # two envs of two cars: nobody sees the other env
    _, _, idx2 = both(ref.settings(k=2, channels=ALL10), rows, 2)
    assert idx2.tolist() == [[1, -1], [0, -1], [1, -1], [0, -1]]


def test_hand_heading_rotates_the_frame_and_scales_divide():
    # car 0 at the origin heading +y at 2 m/s, car 1 at (3, 4) heading -x at 1 m/s
    rows = rows_of([[0.0, 0.0], [3.0, 4.0]], theta=[np.pi / 2, np.pi], v=[2.0, 1.0])
    s = ref.settings(k=1, channels=ALL10, scale={"dist": 2.0, "dx": -4.0})
    out, raw, idx = both(s, rows, 2)
    assert idx.tolist() == [[1], [0]] and raw[:, 0, ref.DIST].tolist() == [5.0, 5.0]
    assert np.allclose(raw[0, 0, :7], [4.0, -3.0, 5.0, 0.0, 1.0, -2.0, 1.0], atol=1e-15)    # ahead 4, right 3; it drives to my left
    assert out[0, 0, ref.DIST] == np.float32(2.5) and np.isclose(out[0, 0, ref.DX], -1.0)
    # the channels come in bit order whatever order they are asked for in
    out2, _, _ = both(ref.settings(k=1, channels=("index", "dist")), rows, 2)
    assert out2.tolist() == [[[5.0, 1.0]], [[5.0, 0.0]]]


def test_hand_coincident_cars_and_the_range_on_a_distance():
    rows = rows_of([[2.0, 1.0], [2.0, 1.0], [5.0, 5.0]])
    out, raw, idx = both(ref.settings(k=2, channels=("dist", "valid", "index"), max_range=5.0), rows, 3)
    # d2 = 0 for the coincident pair; (2, 1) to (5, 5) is exactly 5 m: eligible
    assert idx.tolist() == [[1, 2], [0, 2], [0, 1]]
    assert out.tolist() == [[[0.0, 1.0, 1.0], [5.0, 1.0, 2.0]], [[0.0, 1.0, 0.0], [5.0, 1.0, 2.0]], [[5.0, 1.0, 0.0], [5.0, 1.0, 1.0]]]
    _, _, idx = both(ref.settings(k=2, channels=("dist",), max_range=np.nextafter(5.0, 0.0)), rows, 3)
    assert idx.tolist() == [[1, -1], [0, -1], [-1, -1]]


def test_hand_padding_valid_and_one_car():
    rows = rows_of([[0.0, 0.0], [0.0, 2.0], [7.0, 7.0]])
    s = ref.settings(k=4, channels=("dist", "valid", "index"), pad=-1.0, scale={"dist": 2.0, "valid": 4.0})
    out, raw, idx = both(s, rows, 3)
    assert idx[0].tolist() == [1, 2, -1, -1]
    # a filled slot is scaled, an empty one holds the pad unscaled and VALID 0
    assert out[0, 0].tolist() == [1.0, 0.25, 1.0] and out[0, 2].tolist() == [-1.0, 0.0, -1.0] and out[0, 3].tolist() == [-1.0, 0.0, -1.0]
    assert raw[0, 3].tolist() == [-1.0] * 8 + [0.0, -1.0]
    out1, raw1, idx1 = both(s, rows, 1)                         # A = 1: every slot is empty
    assert np.all(idx1 == -1) and out1.tolist() == [[[-1.0, 0.0, -1.0]] * 4] * 3


def test_hand_nan_row_has_no_neighbours_and_is_nobodys():
    rows = rows_of([[0.0, 0.0], [NAN, NAN], [3.0, 0.0]], theta=[0.0, NAN, 0.0])
    out, raw, idx = both(ref.settings(k=2, channels=("dx", "valid")), rows, 3)
    assert idx.tolist() == [[2, -1], [-1, -1], [0, -1]]
    assert out.tolist() == [[[3.0, 1.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 0.0]], [[-3.0, 1.0], [0.0, 0.0]]]


def test_hand_gap_at_half_the_length():
    # L = 8: gaps of +4, -4, +5, -5, +3 from s = 0, 4, ... ; exactly +L/2 stays, exactly -L/2 wraps to +L/2
    s = ref.settings(k=1, channels=("gap_s",))
    for sa, sb, closed, opened in ((0.0, 4.0, 4.0, 4.0), (4.0, 0.0, 4.0, -4.0), (0.0, 5.0, -3.0, 5.0), (5.0, 0.0, 3.0, -5.0), (1.0, 4.0, 3.0, 3.0)):
        rows = rows_of([[0.0, 0.0], [1.0, 0.0]], s=[sa, sb])
        out, _, _ = both(s, rows, 2, 8.0)
        assert out[0, 0, 0] == closed, (sa, sb)
        out, _, _ = both(s, rows, 2, 0.0)
        assert out[0, 0, 0] == opened, (sa, sb)


# ---- Neighbors.compute (NumPy) against the model over the grid: no float32 output differs -----------------------------------------
def test_compute_matches_model_over_the_grid():
    n = 0
    for case in ref.unit_grid():
        s, rows, L, want = ref.grid_case(case)
        got = Neighbors(**s).compute(rows[:, :3], rows[:, 3], rows[:, 4], case[1], L, raw=True, indices=True)
        assert ref.compare(s, rows, case[1], want, got, "%r" % (case[:4],)) == 0
        assert np.array_equal(ref.bits(got[1]), ref.bits(want[1]))
        n += got[0].size
    assert n > 30000


def test_grid_does_what_it_says():
    """the middle range leaves some agents short of K and fills others, the small one leaves every slot empty, the lattice has ties"""
    for layout in ("scatter", "lattice"):
        for A in ref.GRID_A:
            rows, _, _, raw8, idx8 = ref.grid_search(layout, A, "mid")
            if A >= 17:
                n = (idx8 >= 0).sum(axis=1)
                assert n.min() < 8 and n.max() >= 1, (layout, A)
            assert np.all(ref.grid_search(layout, A, "small")[4] == -1), (layout, A)
            assert A == 1 or np.all(ref.grid_search(layout, A, "inf")[4][:, 0] >= 0)
    d = ref.grid_search("lattice", 64, "inf")[3][..., ref.DIST]
    assert np.any(d[:, 1:] == d[:, :-1])


# ---- the host instantiation of f110_math.hpp's nbr_* against the model -----------------------------------------------------------
@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "neighbors_harness.hip")
    lib = str(tmp_path_factory.mktemp("neighbors_harness") / "libneighbors_harness.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def harness_neighbors(hh, s, rows, A, L):
    K = int(s["k"])
    bits = [b for b, c in enumerate(ref.CHANNELS) if c in s["channels"]]
    scale = np.array([float(s["scale"].get(c, 1.0)) for c in ref.CHANNELS])
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    m = rows.shape[0]
    out, raw, idx = np.zeros((m, K, len(bits)), dtype=np.float32), np.zeros((m, K, 10)), np.zeros((m, K), dtype=np.int32)
    hh.hh_neighbors(A, K, sum(1 << b for b in bits), C.c_double(s["max_range"]), C.c_double(s["pad"]), scale.ctypes.data_as(_dp), C.c_double(L),
                    rows.ctypes.data_as(_dp), m, out.ctypes.data_as(C.c_void_p), raw.ctypes.data_as(_dp), idx.ctypes.data_as(C.POINTER(C.c_int)))
    return out, raw, idx


@needs_hipcc
def test_harness_matches_model_over_the_grid(hh):
    total = differ = 0
    for case in ref.unit_grid():
        s, rows, L, want = ref.grid_case(case)
        differ += ref.compare(s, rows, case[1], want, harness_neighbors(hh, s, rows, case[1], L), "%r" % (case[:4],))
        total += want[0].size
    assert total > 30000 and differ * 1000 <= total, (total, differ)


@needs_hipcc
def test_harness_on_hand_built_cases(hh):
    rows = rows_of(SQUARE, v=[1.0, 2.0, 3.0, 4.0], s=[0.0, 1.0, 2.0, 3.0])
    out, raw, idx = harness_neighbors(hh, ref.settings(k=3, channels=ALL10), rows, 4, 0.0)
    assert idx.tolist() == [[1, 3, 2], [0, 2, 3], [1, 3, 0], [0, 2, 1]] and raw[0, :, ref.DX].tolist() == [1.0, 0.0, 1.0]
    assert raw[..., ref.DIST].tolist() == [[1.0, 1.0, np.sqrt(2.0)]] * 4 and raw[0, :, ref.V_X].tolist() == [1.0, 3.0, 2.0]
    rows = rows_of([[2.0, 1.0], [2.0, 1.0], [5.0, 5.0], [NAN, 0.0]], theta=[0.0, 0.0, 0.0, NAN])
    s = ref.settings(k=4, channels=("dist", "valid", "index"), max_range=5.0, pad=-1.0)
    got = harness_neighbors(hh, s, rows, 4, 0.0)
    assert got[2].tolist() == [[1, 2, -1, -1], [0, 2, -1, -1], [0, 1, -1, -1], [-1, -1, -1, -1]]
    assert ref.compare(s, rows, 4, ref.neighbors(s, rows, 4), got) == 0
    assert got[0][0].tolist() == [[0.0, 1.0, 1.0], [5.0, 1.0, 2.0], [-1.0, 0.0, -1.0], [-1.0, 0.0, -1.0]]
    g = ref.settings(k=1, channels=("gap_s",))
    for sa, sb, closed, opened in ((0.0, 4.0, 4.0, 4.0), (4.0, 0.0, 4.0, -4.0), (0.0, 5.0, -3.0, 5.0), (5.0, 0.0, 3.0, -5.0)):
        rows = rows_of([[0.0, 0.0], [1.0, 0.0]], s=[sa, sb])
        assert harness_neighbors(hh, g, rows, 2, 8.0)[0][0, 0, 0] == closed and harness_neighbors(hh, g, rows, 2, 0.0)[0][0, 0, 0] == opened
    one = harness_neighbors(hh, ref.settings(k=2, channels=("dx", "valid"), pad=3.0), rows_of([[1.0, 1.0]]), 1, 0.0)
    assert one[0].tolist() == [[[3.0, 0.0], [3.0, 0.0]]] and one[2].tolist() == [[-1, -1]]
