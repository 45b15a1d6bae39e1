"""The follow-the-gap rule (include/f110.h, f110_gap_follower) in NumPy float64.

This is the model every device result is held to bit for bit (tests/test_gap_follower_host.py, tests/test_gpu_gap_follower.py).
It is written from the rule, not from the kernel: one row at a time, the window sums as explicit ascending adds (np.sum adds
pairwise, which rounds differently), the runs of free beams found from the edges of the free flags.
"""
import numpy as np

CENTER, FURTHEST = 0, 1

DEFAULTS = dict(beams=None, smooth=5, range_clip=10.0, bubble_radius=0.6, gap_threshold=1.5, target="center", steer_gain=1.0,
                steer_max=0.4189, v_lo=1.5, v_hi=4.0, d_ref=8.0, steer_slow=0.2, v_turn=2.5, v_blocked=0.5)
FOV = 4.7


def settings(**kw):
    """the defaults of the issue with overrides, as a plain dict (what the model reads)"""
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def window(s, B):
    """[lo, hi) of the settings `s` at B beams: None = the default B/6 .. B - B/6, (0, 0) = all beams"""
    beams = s["beams"]
    if beams is None:
        return B // 6, B - B // 6
    if tuple(beams) == (0, 0):
        return 0, B
    return int(beams[0]), int(beams[1])


def smooth_rows(v, S):
    """p[:, i] = (v[:, a] + ... + v[:, b - 1]) / (b - a), a = max(0, i - S // 2), b = min(W, i + S // 2 + 1); the adds run in
    ascending order from 0.0 + v[a], every window on its own (vectorised over rows and beams, a loop over the window)"""
    m, W = v.shape
    h = S // 2
    idx = np.arange(W)
    acc = np.zeros((m, W))
    for d in range(-h, h + 1):
        k = idx + d
        ok = (k >= 0) & (k < W)
        term = v[:, np.clip(k, 0, W - 1)]
        acc = np.where(ok[None, :], acc + term, acc)
    a = np.maximum(0, idx - h)
    b = np.minimum(W, idx + h + 1)
    return acc / (b - a).astype(np.float64)[None, :]


def longest_run(free):
    """(g0, g1) of the longest run of True, the lowest g0 on equal length; None without a True"""
    f = np.concatenate([[False], np.asarray(free, dtype=bool), [False]])
    edges = np.flatnonzero(f[1:] != f[:-1])
    starts, ends = edges[0::2], edges[1::2]
    if len(starts) == 0:
        return None
    k = int(np.argmax(ends - starts))        # the first maximum: the lowest start
    return int(starts[k]), int(ends[k])


def follow_row(s, row, fov=FOV):
    """one scan row [B] -> ((steer, speed), (c, half, g0, g1, t)); the five integers are -1 where the row is blocked"""
    row = np.asarray(row, dtype=np.float64)
    B = row.shape[0]
    lo, hi = window(s, B)
    W = hi - lo
    inc = np.float64(fov) / np.float64(B - 1)
    clip = np.float64(s["range_clip"])
    r = row[lo:hi]
    with np.errstate(all="ignore"):
        v = np.where(r < clip, r, clip)
        v = np.where(np.isnan(r), 0.0, v)
        p = smooth_rows(v[None, :], int(s["smooth"]))[0]
        c = int(np.argmin(p))
        den = p[c] * inc
        kb = np.float64(s["bubble_radius"]) / den if den > 0 else np.inf
    half = W if not (kb < W) else int(np.ceil(kb))
    q = p.copy()
    q[max(0, c - half):min(W, c + half + 1)] = 0.0
    gap = longest_run(q > np.float64(s["gap_threshold"]))
    if gap is None:
        return (0.0, float(s["v_blocked"])), (c, half, -1, -1, -1)
    g0, g1 = gap
    if s["target"] in ("center", CENTER):
        t = (g0 + g1 - 1) >> 1
    else:
        t = g0 + int(np.argmax(q[g0:g1]))
    angle = -np.float64(fov) / 2. + inc * np.float64(lo + t)
    steer = np.float64(s["steer_gain"]) * angle
    sm = np.float64(s["steer_max"])
    steer = sm if steer > sm else (-sm if steer < -sm else steer)
    f = p[t] / np.float64(s["d_ref"])
    speed = np.float64(s["v_lo"]) + (np.float64(s["v_hi"]) - np.float64(s["v_lo"])) * (f if f < 1 else np.float64(1.0))
    if abs(steer) > s["steer_slow"]:
        speed = min(speed, np.float64(s["v_turn"]))
    return (float(steer), float(speed)), (c, half, g0, g1, t)


def follow(s, scans, step_count=None, fov=FOV):
    """scans [m][B] -> actions float64 [m][2], info int32 [m][5].  A row whose step_count is 0 gets (0, 0) and -1s."""
    scans = np.asarray(scans, dtype=np.float64)
    m = scans.shape[0]
    act = np.zeros((m, 2))
    info = np.full((m, 5), -1, dtype=np.int32)
    for i in range(m):
        if step_count is not None and step_count[i] == 0:
            continue
        act[i], info[i] = follow_row(s, scans[i], fov)
    return act, info


def follow_assigned(specs, assign, scans, step_count, actions, fov=FOV):
    """the device form: rows of `actions` [N][2] whose assign is >= 0 are replaced by their controller's action, the others
    are left as they are (a new array)"""
    out = np.array(actions, dtype=np.float64, copy=True)
    for i, k in enumerate(assign):
        if k >= 0:
            out[i] = follow(specs[k], scans[i:i + 1], None if step_count is None else step_count[i:i + 1], fov)[0][0]
    return out


def bits(a):
    """the uint64 view the comparisons are made on"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the unit grid both test files walk (host harness and GPU unit form) ----
GRID_B = (61, 1080, 4096)
GRID_S = (1, 5, 63)


def grid_windows(B):
    """several windows per B: all beams, the default, an off-centre one, a narrow one (at least 63 beams wide where B allows)"""
    return ((0, 0), None, (B // 7, B - B // 5), (B // 3, min(B, B // 3 + max(7, B // 9))))


def unit_grid():
    """(B, beams, S, target) with S kept where it does not exceed the window (the rule refuses the rest)"""
    for B in GRID_B:
        for beams in grid_windows(B):
            lo, hi = window(dict(beams=beams), B)
            for S in GRID_S:
                if S > hi - lo:
                    continue
                for target in ("center", "furthest"):
                    yield B, beams, S, target


def random_rows(rng, m, B, clip=10.0):
    """rows that exercise every branch: corridor-like rows (a smooth profile with walls close on both sides), uniform noise,
    +inf and NaN sprinkled in, an all-near row (blocked), an all-far row (one gap edge to edge), a row of equal ranges (ties)"""
    x = np.linspace(-1.0, 1.0, B)
    rows = np.empty((m, B))
    for i in range(m):
        kind = i % 4
        if kind == 0:
            rows[i] = rng.uniform(0.05, 1.5 * clip, size=B)
        elif kind == 1:      # a few wide lobes
            centres, widths = rng.uniform(-1, 1, 3), rng.uniform(0.05, 0.5, 3)
            rows[i] = 0.4 + sum(rng.uniform(2, 14) * np.exp(-((x - c) / w) ** 2) for c, w in zip(centres, widths)) + rng.normal(0, 0.01, B)
        elif kind == 2:      # plateaus of equal value: ties in argmin, argmax and in run length
            rows[i] = np.repeat(rng.choice([0.5, 2.0, 2.0, 6.0, 12.0], size=B // 16 + 1), 16)[:B]
        else:
            rows[i] = rng.uniform(1.0, 4.0, size=B)
    rows[rng.random((m, B)) < 0.004] = np.inf
    rows[rng.random((m, B)) < 0.004] = np.nan
    if m >= 4:
        rows[0] = rng.uniform(0.05, 1.4, size=B)         # nothing above the default threshold: blocked
        rows[1] = 20.0                                    # everything at the clip: the bubble leaves one side
        rows[2] = 3.0                                     # all equal below the clip
    return rows


def oracle_scans(B, steps=6, E=3, A=2):
    """scan rows of the oracle's simulator on example_map at B beams: E x A cars, a few steps apart"""
    from oracle import orc
    from _util import bench_start_poses, oracle_map_dt
    dt, res, origin = oracle_map_dt("example_map")
    o = orc.SimOracle(E, A, num_beams=B)
    o.set_map_dt(dt, res, origin)
    o.reset(bench_start_poses(E, A))
    rows = []
    for t in range(steps):
        o.step(np.tile([0.05 * (t % 3 - 1), 2.0 + t], (E * A, 1)))
        if t % 2 == 1:
            rows.append(np.array(o.scans, copy=True))
    return np.concatenate(rows)


def hand_rows():
    """(name, settings, row [61], (c, half, g0, g1, t)) worked out by hand: 61 beams, all of them in the window, no smoothing,
    inc = 4.7 / 60, so a closest point at 1.0 m has kb = 0.6 / (1.0 * 4.7 / 60) = 7.66 and a bubble of 8 beams either side"""
    B = 61
    out = []

    def case(name, row, info, **kw):
        out.append((name, settings(beams=(0, 0), smooth=1, **kw), np.asarray(row, dtype=np.float64), info))

    r = np.full(B, 5.0)
    r[30] = 1.0
    case("two gaps of 22 beams: the lower one wins, its centre", r, (30, 8, 0, 22, 10))
    case("equal ranges in the gap: the first is the furthest", r, (30, 8, 0, 22, 0), target="furthest")
    r = np.full(B, 5.0)
    r[30] = 1.0
    r[5] = 7.0
    r[9] = 7.0
    case("furthest: the first of two equal maxima", r, (30, 8, 0, 22, 5), target="furthest")
    r = np.full(B, 5.0)
    r[[20, 40]] = 1.0
    case("two equal minima: the first is the closest point; gap to the upper edge", r, (20, 8, 41, 61, 50))
    r = np.full(B, 5.0)
    r[50] = 1.0
    r[:10] = 1.2
    case("gap between a blocked stretch and the bubble", r, (50, 8, 10, 42, 25))
    r = np.full(B, 5.0)
    r[0] = 1.0
    case("closest point on the lower edge: the gap runs to the upper edge", r, (0, 8, 9, 61, 34))
    case("nothing above the threshold: blocked", np.full(B, 1.0), (0, 8, -1, -1, -1))
    r = np.full(B, 5.0)
    r[10] = np.nan
    case("a NaN beam is an obstacle at the car: the bubble covers the window", r, (10, 61, -1, -1, -1))
    r = np.full(B, 5.0)
    r[10] = 0.0
    case("a zero range: den = 0, the bubble covers the window", r, (10, 61, -1, -1, -1))
    r = np.full(B, 5.0)
    r[30] = 0.1
    case("a bubble wider than the window (kb = 76.6)", r, (30, 61, -1, -1, -1))
    r = np.full(B, np.inf)
    r[30] = 1.0
    case("inf beams are clipped: free", r, (30, 8, 0, 22, 10))
    r = np.full(B, np.inf)
    case("all inf: the first beam is the closest, kb = 0.6 / (10 * 4.7 / 60) = 0.766 -> 1", r, (0, 1, 2, 61, 31))
    r = np.full(B, 1.0)
    r[40:45] = 3.0
    r[50:55] = 3.0
    r[0] = 0.9
    case("two gaps of five: the lower one", r, (0, 9, 40, 45, 42))
    return out
