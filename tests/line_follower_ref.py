"""The model of the line follower (include/f110.h, f110_line_follower): plain Python float64, one IEEE operation per
step in the order the header states, a loop per row, on top of tests/track_preview_ref.py's station functions (Tables,
segment_of, clip01).  Shared by the CPU tests (tests/test_line_follower_host.py) and the GPU tests
(tests/test_gpu_line_follower.py)."""
import math

import numpy as np

from track_preview_ref import Tables, bits, clip01, example_raceline, segment_of, STAGED_SEGS   # noqa: F401

RAW = ("ld", "s_t", "k", "X", "Y", "Tx", "Ty", "lx", "ly", "vref", "lim", "speed")
EXACT = [RAW.index(c) for c in ("ld", "s_t", "k", "X", "Y", "Tx", "Ty", "vref", "lim", "speed")]
DEFAULTS = dict(look_base=0.8, look_gain=0.25, look_min=0.6, look_max=3.9, lane_offset=0.0, wheelbase=0.3302, steer_max=0.4189,
                speed_attr=1, v_const=2.0, vgain=0.8, speed_look=0.6, lat_slow=0.5, v_recover=1.5, follow_range=6.0, follow_gap=1.0,
                follow_gain=1.0, lane_width=0.6, v_min=0.0, v_max=20.0)


def settings(**kw):
    s = dict(DEFAULTS)
    s.update(kw)
    return s


def lookahead(S, v):
    ld = S["look_base"] + S["look_gain"] * abs(v)
    if not (ld >= S["look_min"]):
        ld = S["look_min"]
    elif ld > S["look_max"]:
        ld = S["look_max"]
    return ld


def ahead(tab, s, d):
    q = s + d
    if tab.closed and q >= tab.L:
        q = q - tab.L
    return q


def station(tab, sj):
    """k, t, (X, Y), (ux, uy) by the preview's station rule"""
    k = segment_of(tab, sj)
    ln = tab.len[k]
    t = clip01((sj - tab.cum[k]) / ln)
    return k, t, tab.ax[k] + t * tab.dx[k], tab.ay[k] + t * tab.dy[k], tab.dx[k] / ln, tab.dy[k] / ln


def attribute(tab, c, sj):
    k, t = station(tab, sj)[:2]
    k1 = 0 if k + 1 == tab.npts else k + 1
    a0, a1 = float(tab.attrs[k, c]), float(tab.attrs[k1, c])
    return a0 + t * (a1 - a0)


def gap(sa, sb, L):
    """the neighbours' GAP_S rule; L == 0: no wrap"""
    g = sb - sa
    if L > 0.0:
        half = 0.5 * L
        if g > half:
            g = g - L
        elif g <= -half:
            g = g + L
    return g


def follow(tab, S, rows, A=1):
    """rows [m][7] = x, y, theta, v, s, lateral, step_count, env-major with A cars per env -> (actions [m][2], raw [m][12])"""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 7)
    m = rows.shape[0]
    assert m % A == 0
    act, raw = np.zeros((m, 2)), np.zeros((m, 12))
    Lw = tab.L if tab.closed else 0.0
    R = rows.tolist()
    for r in range(m):
        px, py, th, v, s, lat, cnt = R[r]
        if cnt == 0.0:
            raw[r, RAW.index("k")] = raw[r, RAW.index("lim")] = -1.0
            continue
        ld = lookahead(S, v)
        s_t = ahead(tab, s, ld)
        k, _, X, Y, ux, uy = station(tab, s_t)
        Tx, Ty = X - S["lane_offset"] * uy, Y + S["lane_offset"] * ux
        c, sn = float(np.cos(np.float64(th))), float(np.sin(np.float64(th)))
        rx, ry = Tx - px, Ty - py
        lx, ly = c * rx + sn * ry, c * ry - sn * rx
        d2 = lx * lx + ly * ly
        steer = float(np.arctan(np.float64(2.0 * S["wheelbase"] * ly / d2))) if d2 > 0.0 else 0.0
        if steer > S["steer_max"]:
            steer = S["steer_max"]
        elif steer < -S["steer_max"]:
            steer = -S["steer_max"]
        s_v = ahead(tab, s, S["speed_look"])
        vref = attribute(tab, S["speed_attr"], s_v) if S["speed_attr"] >= 0 else S["v_const"]
        speed = S["vgain"] * vref
        if abs(lat - S["lane_offset"]) > S["lat_slow"] and S["v_recover"] < speed:
            speed = S["v_recover"]
        lim = -1
        if S["follow_range"] > 0.0 and A > 1:
            e0, a = r - r % A, r % A
            for b in range(A):
                if b == a:
                    continue
                vb, sb, latb = R[e0 + b][3], R[e0 + b][4], R[e0 + b][5]
                g = gap(s, sb, Lw)
                if g > 0.0 and g <= S["follow_range"] and abs(latb - lat) <= S["lane_width"]:
                    cap = vb + S["follow_gain"] * (g - S["follow_gap"])
                    if cap < speed:
                        speed, lim = cap, b
        pre = speed
        if speed < S["v_min"]:
            speed = S["v_min"]
        if speed > S["v_max"]:
            speed = S["v_max"]
        act[r] = steer, speed
        raw[r] = ld, s_t, float(k), X, Y, Tx, Ty, lx, ly, vref, float(lim), pre
    return act, raw


def rel_err(got, want):
    """|got - want| / max(|want|, 1e-12), NaN against NaN 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        e = np.abs(got - want) / np.maximum(np.abs(want), 1e-12)
    return np.where(np.isnan(got) & np.isnan(want), 0.0, e)


def compare(tab, S, rows, A, got, what="", need_d2=True):
    """got = (actions, raw) of the code under test against the model: speed and the raw columns ld, s_t, k, X, Y, Tx, Ty, vref, lim
    and the pre-clamp speed bit for bit; lx, ly and steer, which sit behind cos_sin and atan, rel_err <= 1e-9 on the rows where the
    model's d2 >= 0.25.  need_d2: every row but the fresh ones and those with d2 == 0 must be such a row.  -> the largest
    absolute difference seen in (lx, ly, steer)"""
    want_act, want_raw = follow(tab, S, rows, A)
    act, raw = got
    assert np.array_equal(bits(act[:, 1]), bits(want_act[:, 1])), "%s: speeds differ" % what
    assert np.array_equal(bits(raw[:, EXACT]), bits(want_raw[:, EXACT])), "%s: exact raw columns differ in %r" % (
        what, [RAW[EXACT[c]] for c in np.nonzero(np.any(bits(raw[:, EXACT]) != bits(want_raw[:, EXACT]), axis=0))[0]])
    lx, ly = want_raw[:, RAW.index("lx")], want_raw[:, RAW.index("ly")]
    d2 = lx * lx + ly * ly
    fresh = np.asarray(rows).reshape(-1, 7)[:, 6] == 0.0
    zero = ~fresh & (d2 == 0.0)
    assert np.all(act[zero, 0] == 0.0) and not np.any(np.signbit(act[zero, 0])), "%s: d2 == 0 must steer 0.0" % what
    assert np.array_equal(bits(act[fresh]), bits(want_act[fresh])), "%s: fresh rows differ" % what
    far = ~fresh & (d2 >= 0.25)
    if need_d2:
        assert np.all(far | zero | fresh), "%s: %d rows have 0 < d2 < 0.25" % (what, int(np.count_nonzero(~(far | zero | fresh))))
    worst = 0.0
    for g, w in ((raw[:, 7], want_raw[:, 7]), (raw[:, 8], want_raw[:, 8]), (act[:, 0], want_act[:, 0])):
        e = rel_err(g[far], w[far])
        assert np.all(e <= 1e-9), "%s: rel_err %r beyond 1e-9" % (what, float(e.max()))
        if np.any(far):
            worst = max(worst, float(np.nanmax(np.abs(g[far] - w[far]), initial=0.0)))
    return worst


# ---- tracks -------------------------------------------------------------------------------------------------------------------------
def stadium(n_arc=24, straight=20.0, radius=6.0):
    """two exact straights along y = 0 and y = 2 r (zero curvature) joined by half circles; attributes kappa, vx"""
    pts = []
    n_st = 10
    for q in range(n_st):
        pts.append((straight * q / n_st, 0.0, 0.0))
    for q in range(n_arc):
        a = -0.5 * math.pi + math.pi * q / n_arc
        pts.append((straight + radius * math.cos(a), radius + radius * math.sin(a), 1.0 / radius))
    for q in range(n_st):
        pts.append((straight - straight * q / n_st, 2.0 * radius, 0.0))
    for q in range(n_arc):
        a = 0.5 * math.pi + math.pi * q / n_arc
        pts.append((radius * math.cos(a), radius + radius * math.sin(a), 1.0 / radius))
    p = np.array(pts)
    attrs = np.column_stack([p[:, 2], np.where(p[:, 2] > 0.0, 3.0, 6.0)])
    return Tables(p[:, :2], True, attrs), p[:, :2], attrs


def closed_8():
    """a closed line of 8 points (an irregular octagon, 26 m or so); attributes kappa (a stand-in), vx"""
    ang = 2.0 * np.pi * np.arange(8) / 8
    r = np.array([4.0, 4.5, 3.8, 4.2, 4.0, 4.6, 3.9, 4.1])
    xy = np.column_stack([r * np.cos(ang) + 1.0, r * np.sin(ang) - 0.5])
    attrs = np.column_stack([1.0 / r, 2.0 + 0.25 * np.arange(8)])
    return Tables(xy, True, attrs), xy, attrs


def open_2():
    """an open line of 2 points, 12.5 m; attributes kappa, vx"""
    xy = np.array([[0.5, -1.0], [8.0, 9.0]])
    attrs = np.array([[0.0, 2.0], [0.0, 5.0]])
    return Tables(xy, False, attrs), xy, attrs


def ring(nseg, radius=40.0):
    """a closed circle of nseg segments; attributes kappa, vx"""
    ang = 2.0 * np.pi * np.arange(nseg) / nseg
    xy = np.column_stack([radius * np.cos(ang) - 1.0, radius * np.sin(ang) + 2.0])
    attrs = np.column_stack([np.full(nseg, 1.0 / radius), 4.0 + np.cos(3.0 * ang)])
    return Tables(xy, True, attrs), xy, attrs


def on_line(tab, s, lat=0.0, dth=0.0, back=0.0):
    """the pose lat metres to the left of and `back` metres behind the line's point at arc length s, heading along the line plus dth"""
    _, _, X, Y, ux, uy = station(tab, s)
    return X - lat * uy - back * ux, Y + lat * ux - back * uy, math.atan2(uy, ux) + dth


def boundary_cars(S, L):
    """the scripted cars ahead as (gap from car 0, lateral offset from car 0, v_b).  With car 0 at s = 0 and lat = 0 the sums are
    exact, so the car sits bitwise on the compare it is named after.  Every v_b but the NaN one is low enough to cap any speed,
    so an eligible car shows as `lim` and in the pre-clamp speed."""
    fr, lw, inf = S["follow_range"], S["lane_width"], float("inf")
    return [(fr, 0.0, -20.0),                          # 0  g = follow_range exactly: eligible
            (math.nextafter(fr, inf), 0.0, -20.0),     # 1  one ulp beyond: not
            (1.5, lw, -20.0),                          # 2  |lat_b - lat| = lane_width exactly: eligible
            (1.5, math.nextafter(lw, inf), -20.0),     # 3  one ulp beyond: not
            (0.0, 0.0, -20.0),                         # 4  g = 0: not
            (0.5 * L, 0.0, -20.0),                     # 5  g = L / 2 exactly (out of range whichever way the wrap goes)
            (1.5, -lw, float("nan")),                  # 6  eligible, but a NaN cap never wins
            (-2.0, 0.1, -20.0),                        # 7  behind
            (0.5 * fr, 0.1, 0.2),                      # 8  an ordinary car ahead
            (math.nextafter(fr, 0.0), -lw, -20.0)]     # 9  just inside both
BOUNDARY_LIMITS = (True, False, True, False, False, False, False, False, True, True)


def grid_rows(tab, S, A, rng, vs=(-1.0, 0.0, 3.0, 40.0, float("nan"))):
    """the unit grid's rows for one track, settings and A: envs of A cars -> (rows, first: the row of car 0 of the first boundary
    env).  Car 0 of each env runs through the s / v cases; behind them come len(boundary_cars) envs with car 0 at s = 0, lat = 0
    and v = 3, env j's car b being boundary car (b - 1 + j) mod 10, so that at A = 2 every boundary car is once the only other
    car.  In the other envs car b is boundary car (b - 1 + n) mod 10; from b = 11 on the cars sit at random places.  The unit form
    does not project, so a pose need not match its s: every pose lies 0.6 m behind its point of the line, look_min or more short
    of its target even where an open track's station clips to the last point, so that d2 >= 0.25 on every row but the one
    placed on its target bitwise."""
    L = tab.L
    cars = boundary_cars(S, L)
    T = len(cars)
    rows = []
    s_cases = []
    for v in vs:
        ld = lookahead(S, v)
        edge = L - ld
        s_cases += [(0.0, v), (math.nextafter(L, 0.0), v), (edge, v), (math.nextafter(edge, 0.0), v), (math.nextafter(edge, L), v),
                    (float(rng.uniform(0.0, L)), v)]
    first = len(s_cases) * A
    s_cases += [(0.0, 3.0)] * T
    for n, (s, v) in enumerate(s_cases):
        edge_env = n * A >= first
        lat = 0.0 if edge_env else (0.0, 0.3, -0.7)[n % 3]
        env = [[*on_line(tab, s, lat, (0.0, 0.2, -0.3)[n % 3], 0.6), v, s, lat, float(1 + n)]]
        rot = n - first // A if edge_env else n
        for b in range(1, A):
            if b <= T:
                d, dlat, vb = cars[(b - 1 + rot) % T]
            else:
                d, dlat, vb = float(rng.uniform(-0.5 * L, 0.5 * L)), float(rng.uniform(-1.0, 1.0)), (1.0, 2.5, float("nan"), 0.2)[b % 4]
            sb = s + d
            if tab.closed:
                sb = sb - L if sb >= L else (sb + L if sb < 0.0 else sb)
            else:
                sb = min(max(sb, 0.0), L)
            latb = lat + dlat
            env.append([*on_line(tab, sb, latb, 0.1, 0.6), vb, sb, latb, 3.0])
        rows += env
    rows = np.array(rows)
    rows[A, 6] = 0.0              # a fresh row ...
    if A > 1:
        rows[2 * A + 1, 6] = 0.0   # ... and a fresh car ahead, which still counts as a car
    # one row bitwise on its target: d2 == 0
    r = 3 * A
    ld = lookahead(S, rows[r, 3])
    _, _, X, Y, ux, uy = station(tab, ahead(tab, rows[r, 4], ld))
    rows[r, 0], rows[r, 1] = X - S["lane_offset"] * uy, Y + S["lane_offset"] * ux
    return rows, first


def boundary_check(tab, S, A, rows, first, raw, what=""):
    """the boundary envs of grid_rows in `raw` (the code under test's, already held to the model bit for bit): at A = 2 env j's
    only other car limits exactly when BOUNDARY_LIMITS[j] says so, with the cap as the pre-clamp speed; at A = 3 and 5 the car at
    g = follow_range exactly limits env 0 (at 5 the nearer car on the lane's edge, cars[2], caps lower and limits instead)."""
    if A < 2:
        return 0
    cars = boundary_cars(S, tab.L)
    lim, pre = raw[:, RAW.index("lim")], raw[:, RAW.index("speed")]
    if A == 2:
        for j, (d, dlat, vb) in enumerate(cars):
            r = first + j * A
            assert lim[r] == (1.0 if BOUNDARY_LIMITS[j] else -1.0), "%s: boundary car %d: lim = %r" % (what, j, lim[r])
            if BOUNDARY_LIMITS[j]:
                assert pre[r] == vb + S["follow_gain"] * (d - S["follow_gap"]), "%s: boundary car %d: cap %r" % (what, j, pre[r])
        return len(cars)
    if A in (3, 5):
        assert lim[first] == (1.0 if A == 3 else 3.0), "%s: the car at follow_range exactly: lim = %r" % (what, lim[first])
        return 1
    return 0


# ---- the unit grid --------------------------------------------------------------------------------------------------------------------
UNIT_A = (1, 2, 3, 5, 33, 256)


def unit_tracks():
    """(name, tables, xy, attrs): a stadium with exact straights, a closed line of 8 points, an open line of 2 points, berlin's
    raceline (782 segments) and a closed line one segment longer than the kernel stages in LDS"""
    return [("stadium",) + stadium(), ("closed_8",) + closed_8(), ("open_2",) + open_2(), ("berlin",) + example_raceline(True, 2),
            ("ring_%d" % (STAGED_SEGS + 1),) + ring(STAGED_SEGS + 1)]


def unit_settings(name, k):
    """settings that fit the track: the 8-point line is about 25 m long, the open one 12.5 m"""
    S = settings(lane_offset=(0.0, 0.4, -0.25)[k % 3], vgain=(0.8, 1.0)[k % 2])
    if name in ("closed_8", "open_2"):
        S.update(follow_range=4.0, look_max=3.0)
    if k % 4 == 3:
        S.update(speed_attr=-1, v_const=3.5, v_min=1.0, v_max=3.0)
    return S


def unit_rows(tab, S, A, rng):
    """grid_rows -> (rows, first); from 33 cars per env on at one speed only (the model is a Python loop over the pairs)"""
    return grid_rows(tab, S, A, rng) if A < 33 else grid_rows(tab, S, A, rng, vs=(3.0,))
