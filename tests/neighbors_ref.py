"""The model of the neighbour observation (include/f110.h, f110_neighbors): plain Python float64, one IEEE operation
per step in the order the header states, a loop per env, per agent and per candidate, the K best kept by an insertion into a
Python list (no argsort).  The search (search) keeps all of MAX_K slots and every channel once per (rows, A, L, max_range); a
spec's output (render) is its first K slots, its channels, its padding and its scaling.  Shared by the CPU tests
(tests/test_neighbors_host.py) and the GPU tests (tests/test_gpu_neighbors.py)."""
import functools
import math

import numpy as np

CHANNELS = ("dx", "dy", "dist", "cos_dth", "sin_dth", "v_x", "v_y", "gap_s", "valid", "index")
DX, DY, DIST, COS_DTH, SIN_DTH, V_X, V_Y, GAP_S, VALID, INDEX = range(10)
EXACT = (DIST, GAP_S, VALID, INDEX)
MAX_K = 8
EPS = 2.0 ** -52
INF = float("inf")
GRID_A = (1, 2, 3, 4, 5, 17, 64, 65, 256)
GRID_K = (1, 3, 8)


def settings(**kw):
    s = dict(k=1, channels=("dx", "dy"), max_range=INF, pad=0.0, scale={})
    s.update(kw)
    return s


def gap(sa, sb, L):
    g = sb - sa
    if L > 0.0:
        if g > 0.5 * L:
            g = g - L
        elif g <= -0.5 * L:
            g = g + L
    return g


def search(rows, A, L=0.0, max_range=INF):
    """rows [m][5] = x, y, theta, v, s, env-major -> (raw float64 [m][8][10], idx int32 [m][8]): the 8 nearest eligible opponents
    of every row and all ten channel values of each; an empty slot has idx -1 and NaN values (render pads them)"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    m = rows.shape[0]
    assert m % A == 0
    R2 = float(max_range) * float(max_range)
    raw = np.full((m, MAX_K, 10), np.nan)
    idx = np.full((m, MAX_K), -1, dtype=np.int32)
    cs = [(float(np.cos(np.float64(t))), float(np.sin(np.float64(t)))) for t in rows[:, 2]]
    R = rows.tolist()
    for e in range(m // A):
        env = R[e * A:(e + 1) * A]
        trig = cs[e * A:(e + 1) * A]
        for a in range(A):
            xa, ya, _, va, sa = env[a]
            ca, sna = trig[a]
            best = []                                 # (d2, b), ascending d2, equal d2 in ascending b
            for b in range(A):
                if b == a:
                    continue
                rx, ry = env[b][0] - xa, env[b][1] - ya
                d2 = rx * rx + ry * ry
                if not d2 <= R2:                      # (a NaN d2 is never eligible)
                    continue
                pos = len(best)
                while pos > 0 and d2 < best[pos - 1][0]:
                    pos -= 1
                if pos < MAX_K:
                    best.insert(pos, (d2, b))
                    del best[MAX_K:]
            for k, (d2, b) in enumerate(best):
                xb, yb, _, vb, sb = env[b]
                cb, snb = trig[b]
                rx, ry = xb - xa, yb - ya
                cd, sd = cb * ca + snb * sna, snb * ca - cb * sna
                raw[e * A + a, k] = [ca * rx + sna * ry, ca * ry - sna * rx, math.sqrt(d2), cd, sd, vb * cd - va, vb * sd,
                                     gap(sa, sb, L), 1.0, float(b)]
                idx[e * A + a, k] = b
    return raw, idx


def render(s, raw8, idx8):
    """a spec's (out float32 [m][K][D], raw float64 [m][K][10], idx int32 [m][K]) from the search's result"""
    K = int(s["k"])
    bits = [b for b, c in enumerate(CHANNELS) if c in s["channels"]]
    idx = np.ascontiguousarray(idx8[:, :K])
    valid = idx >= 0
    padrow = np.full(10, float(s["pad"]))
    padrow[VALID] = 0.0
    raw = np.where(valid[..., None], raw8[:, :K], padrow)
    scale = np.array([float(s["scale"].get(c, 1.0)) for c in CHANNELS])
    with np.errstate(invalid="ignore", over="ignore"):
        scaled = (raw / scale).astype(np.float32)
    out = np.where(valid[..., None], scaled, padrow.astype(np.float32))[..., bits]
    return np.ascontiguousarray(out, dtype=np.float32), raw, idx


def neighbors(s, rows, A, L=0.0):
    return render(s, *search(rows, A, L, s["max_range"]))


# ---- the comparison the issue states ------------------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def f32_steps(a, b):
    """how many float32 values apart two float32 arrays are, element by element (0 = the same value; NaN against NaN 0)"""
    def key(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(key(a) - key(b))
    return np.where(np.isnan(a) & np.isnan(b), 0, d)


def compare_out(s, want_out, out, what=""):
    """float32 outputs: the exact channels (dist, gap_s, valid, index) bit for bit, every other one the model's or its float32
    neighbour -> how many differ (the caller holds the sum over its grid to 1 in 1000)"""
    assert out.shape == want_out.shape and out.dtype == np.float32, "%s: shape %r, dtype %r" % (what, out.shape, out.dtype)
    names = [c for c in CHANNELS if c in s["channels"]]
    exact = [i for i, c in enumerate(names) if CHANNELS.index(c) in EXACT]
    assert np.array_equal(bits(out[..., exact]), bits(want_out[..., exact])), "%s: dist / gap_s / valid / index outputs differ" % what
    steps = f32_steps(out, want_out)
    assert steps.max(initial=0) <= 1, "%s: a float32 output is %d values away from the model's" % (what, int(steps.max()))
    return int(np.count_nonzero(steps))


def compare(s, rows, A, want, got, what=""):
    """got = (out, raw, idx) of the code under test against the model's want: idx, VALID, INDEX, DIST and GAP_S bit for bit on the
    raw values (and every value of an empty slot); DX, DY within 8 eps (|rx| + |ry|), COS_DTH, SIN_DTH within 8 eps, V_X within
    8 eps (|v_a| + |v_b|), V_Y within 8 eps |v_b|; the float32 outputs as compare_out holds them -> how many of them differ"""
    out, raw, idx = got
    w_out, w_raw, w_idx = want
    assert np.array_equal(idx, w_idx), "%s: the neighbour indices differ" % what
    for ch in EXACT:
        assert np.array_equal(bits(raw[..., ch]), bits(w_raw[..., ch])), "%s: raw %s differs" % (what, CHANNELS[ch])
    empty = w_idx < 0
    assert np.array_equal(bits(raw[empty]), bits(w_raw[empty])), "%s: an empty slot's raw values differ" % what
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 5)
    m, K = w_idx.shape
    me = np.arange(m)[:, None]
    other = (me // A) * A + np.where(empty, 0, w_idx)
    with np.errstate(invalid="ignore"):
        size = np.abs(rows[other, 0] - rows[me, 0]) + np.abs(rows[other, 1] - rows[me, 1])
        va, vb = np.abs(rows[me, 3]) + 0.0 * size, np.abs(rows[other, 3])
        one = np.ones(size.shape)
        bound = {DX: size, DY: size, COS_DTH: one, SIN_DTH: one, V_X: va + vb, V_Y: vb}
        for ch, b in bound.items():
            err = np.abs(raw[..., ch] - w_raw[..., ch])
            ok = empty | (np.isnan(raw[..., ch]) & np.isnan(w_raw[..., ch])) | (err <= 8 * EPS * b)
            assert np.all(ok), "%s: raw %s beyond the bound: worst excess %r" % (what, CHANNELS[ch], float(np.nanmax(np.where(ok, 0.0, err - 8 * EPS * b))))
    return compare_out(s, w_out, out, what)


# ---- cars and the grid ------------------------------------------------------------------------------------------------------------------
TRACK_L = 50.0
MID_RANGE, SMALL_RANGE = {"scatter": 2.0, "lattice": 1.0}, {"scatter": 1e-4, "lattice": 0.5}


def envs_of(A):
    """how many envs a grid case has: several workgroups' worth at the small sizes, two envs at the large ones"""
    return {1: 5, 2: 9, 3: 7, 4: 6, 5: 5, 17: 3}.get(A, 2)


def cars(layout, A, E, seed):
    """rows [E * A][5].  scatter: cars uniform in a square of side 2 sqrt(A) + 1 (about 0.25 cars per square metre at any A), random
    headings, speeds in -1 .. 8 and arc lengths in 0 .. TRACK_L.  lattice: distinct integer points of a square lattice about twice
    as large as the env needs, so that many squared distances are equal, and speeds and arc lengths in quarters"""
    rng = np.random.default_rng(seed)
    rows = np.empty((E, A, 5))
    if layout == "scatter":
        side = 2.0 * np.sqrt(A) + 1.0
        rows[..., 0:2] = rng.uniform(-0.5 * side, 0.5 * side, (E, A, 2))
        rows[..., 2] = rng.uniform(-np.pi, np.pi, (E, A))
        rows[..., 3] = rng.uniform(-1.0, 8.0, (E, A))
        rows[..., 4] = rng.uniform(0.0, TRACK_L, (E, A))
    else:
        w = int(np.ceil(np.sqrt(2.0 * A)))
        for e in range(E):
            cell = rng.choice(w * w, size=A, replace=False)
            rows[e, :, 0], rows[e, :, 1] = cell % w - w // 2, cell // w - w // 2
        rows[..., 2] = rng.integers(-4, 5, (E, A)) * (np.pi / 4.0)
        rows[..., 3] = rng.integers(-4, 33, (E, A)) * 0.25
        rows[..., 4] = rng.integers(0, 200, (E, A)) * 0.25
    return np.ascontiguousarray(rows.reshape(E * A, 5))


@functools.lru_cache(maxsize=None)
def grid_search(layout, A, which):
    """(rows, L, max_range, raw8, idx8) of one (layout, A, range) of the grid; the model runs once per process for each"""
    E = envs_of(A)
    rows = cars(layout, A, E, 1000 * A + (7 if layout == "lattice" else 0))
    max_range = {"inf": INF, "mid": MID_RANGE[layout], "small": SMALL_RANGE[layout]}[which]
    L = TRACK_L if (A + len(which)) % 2 else 0.0          # half the grid wraps the gap, half does not
    raw8, idx8 = search(rows, A, L, max_range)
    for a in (rows, raw8, idx8):
        a.setflags(write=False)
    return rows, L, max_range, raw8, idx8


GRID_CHANNELS = (CHANNELS, ("dx", "dy", "dist", "valid"), ("cos_dth", "sin_dth", "v_x", "v_y", "gap_s", "index"), ("dist",))
GRID_SCALE = {"dx": 10.0, "dy": -4.0, "dist": 3.0, "v_x": 0.5, "gap_s": 25.0, "index": 256.0, "valid": 2.0}


def unit_grid():
    """(layout, A, K, which range, settings) of the CPU / unit-form grid: every A x K x range x layout; the channel set, the scales
    and the pad vary with the case number"""
    out = []
    n = 0
    for layout in ("scatter", "lattice"):
        for A in GRID_A:
            for K in GRID_K:
                for which in ("inf", "mid", "small"):
                    s = settings(k=K, channels=GRID_CHANNELS[n % 4], pad=(0.0, -1.0, 99.5)[n % 3], scale=GRID_SCALE if n % 2 else {})
                    out.append((layout, A, K, which, s))
                    n += 1
    return out


def grid_case(case):
    """-> (settings with the range filled in, rows, L, the model's (out, raw, idx))"""
    layout, A, K, which, s = case
    rows, L, max_range, raw8, idx8 = grid_search(layout, A, which)
    s = dict(s, max_range=max_range)
    return s, rows, L, render(s, raw8, idx8)
