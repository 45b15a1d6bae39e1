"""The model of the opponent term (include/f110.h, f110_opponents): plain Python loops over `math` functions on top of
the rollout's and the planner's models (tests/rollout_ref.py fly, tests/mppi_ref.py candidates / update; tests/_util.track_oracle
for the projection).  Its stages are functions of their own: predict (where the opponents will be), sample (a candidate's poses
against the predictions), cost (the planner's two terms).  math.cos / math.sin are the libm calls the host instantiation makes, so
the host harness agrees bit for bit; the device's differ by its own sincos.  Shared by tests/test_opponents_host.py,
tests/test_gpu_opponents.py and tests/test_gpu_opponents_edges.py."""
import functools
import math

import numpy as np

import mppi_ref as mr
import rollout_ref as rr
from _util import track_oracle

INF, NAN = float("inf"), float("nan")
MODES = ("cv", "track")


def settings(**kw):
    s = dict(mode="cv", radius=0.4, max_range=INF)
    s.update(kw)
    return s


def track_cols(track):
    """the seven segment columns f110_track_set uploads: ax, ay, dx, dy, l2, len, cum"""
    pts = track.points_closed()
    a, d = pts[:-1], pts[1:] - pts[:-1]
    return np.ascontiguousarray(np.stack([a[:, 0], a[:, 1], d[:, 0], d[:, 1], d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1], track.seg_len, track.cum]))


def tau(h, repeat, time_step):
    return float((h + 1) * repeat) * time_step


def in_range(x, y, ox, oy, max_range):
    dx, dy = ox - x, oy - y
    return dx * dx + dy * dy <= max_range * max_range


def segment_of(cum, s):
    """the last segment with cum[k] <= s, 0 when there is none (the preview's binary search)"""
    lo, hi = 0, len(cum) - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if cum[mid] <= s:
            lo = mid
        else:
            hi = mid - 1
    return lo


def station(cols, s):
    """(X, Y, ux, uy) of the preview's station at arc length s, in the map frame"""
    k = segment_of(cols[6], s)
    ax, ay, dx, dy, ln, cum = (float(cols[c][k]) for c in (0, 1, 2, 3, 5, 6))
    t = (s - cum) / ln
    t = 0.0 if t < 0.0 else (1.0 if t > 1.0 else t)
    return ax + t * dx, ay + t * dy, dx / ln, dy / ln


def predict(s, x, y, opp, H, repeat, time_step=rr.TIME_STEP, track=None):
    """one agent at (x, y): opp [Ao][4] = x, y, v, theta -> p [Ao][H][2]; an opponent out of range (or NaN): NaN"""
    opp = np.asarray(opp, dtype=np.float64).reshape(-1, 4)
    p = np.full((opp.shape[0], H, 2), NAN)
    cols = None if track is None else track_cols(track)
    for o, (ox, oy, v, th) in enumerate(opp.tolist()):
        if not in_range(x, y, ox, oy, s["max_range"]):
            continue
        if s["mode"] == "cv":
            c, sn = math.cos(th), math.sin(th)
            for h in range(H):
                d = v * tau(h, repeat, time_step)
                p[o, h] = (ox + d * c, oy + d * sn)
        else:
            s_o, lat_o = (float(q) for q in track_oracle(track, np.array([[ox, oy, 0.0]]))[0, :2])
            for h in range(H):
                sh = s_o + v * tau(h, repeat, time_step)
                if track.closed:
                    if sh >= track.length:
                        sh = sh - track.length
                    elif sh < 0.0:
                        sh = sh + track.length
                X, Y, ux, uy = station(cols, sh)
                p[o, h] = (X - lat_o * uy, Y + lat_o * ux)
    return p


def sample(radius, xy, pred):
    """one candidate: xy [H][2] its map-frame positions after each action, pred [Ao][H][2] -> (OPP_MIN, OPP_FREE, near): near is
    the smallest |d - radius| over the samples (inf without one)"""
    H = len(xy)
    m, free, hit, near = INF, H, False, INF
    for h in range(H):
        x, y = float(xy[h][0]), float(xy[h][1])
        for o in range(len(pred)):
            dx, dy = x - float(pred[o][h][0]), y - float(pred[o][h][1])
            d = math.sqrt(dx * dx + dy * dy)   # (a NaN passes through)
            if d < m:
                m = d
            if not hit and d < radius:
                hit, free = True, h
            if d == d:
                near = min(near, abs(d - radius))
    return m, free, near


def sample_rows(s, poses, pred):
    """poses [m][K][H][>=2] (the rollout's map-frame poses), pred [m][Ao][H][2] -> raw float64 [m][K][2], near [m][K]"""
    m, K = poses.shape[:2]
    raw, near = np.zeros((m, K, 2)), np.zeros((m, K))
    for n in range(m):
        for k in range(K):
            mn, free, nr = sample(s["radius"], poses[n, k], pred[n])
            raw[n, k], near[n, k] = (mn, float(free)), nr
    return raw, near


def cost_of(ms, w_hit, w_near, near_ref, alive, min_clear, opp_min, opp_free, progress, end_lat):
    """the planner's cost with the two opponent terms between the map's and the track's"""
    H = ms["horizon"]
    c = ms["w_dead"] * float(H * ms["repeat"] - alive)
    c = c + ms["w_clear"] * (ms["clear_ref"] - min_clear if min_clear < ms["clear_ref"] else 0.0)
    c = c + w_hit * float(H - opp_free)
    c = c + w_near * (near_ref - opp_min if opp_min < near_ref else 0.0)
    c = c - ms["w_progress"] * progress
    c = c + ms["w_lat"] * abs(end_lat)
    return INF if c != c else c


def costs(ms, w_hit, w_near, near_ref, raw4, opp_raw):
    """raw4 [m][K][4] = ALIVE, MIN_CLEAR, PROGRESS, END_LAT and opp_raw [m][K][2] -> cost [m][K]"""
    m, K = raw4.shape[:2]
    out = np.zeros((m, K))
    for n in range(m):
        for k in range(K):
            a, mc, pr, lat = (float(v) for v in raw4[n, k])
            out[n, k] = cost_of(ms, w_hit, w_near, near_ref, int(a), mc, float(opp_raw[n, k, 0]), int(opp_raw[n, k, 1]), pr, lat)
    return out


def rollout(s, so, start, params, actions, per_agent, opp, H, repeat, margin, integrator, track=None, lidar_dist=0.0, time_step=rr.TIME_STEP):
    """the rollout's model with the term: (flown, pred [m][Ao][H][2], raw [m][K][2], near [m][K])"""
    flown = rr.fly(so, start, params, actions, per_agent, repeat, margin, integrator, lidar_dist, time_step)
    pred = np.stack([predict(s, float(start[n][0]), float(start[n][1]), opp[n], H, repeat, time_step, track) for n in range(len(start))])
    raw, near = sample_rows(s, flown[3], pred)
    return flown, pred, raw, near


def plan(ms, s, w_hit, w_near, near_ref, so, start, params, nominal, streams, opp, integrator, fresh=None, track=None, lidar_dist=0.0,
         time_step=rr.TIME_STEP):
    """mppi_ref.plan with the term: the same dict, plus opp_raw [m][K][2], pred and opp_near [m][K]"""
    start, params = np.asarray(start, dtype=np.float64), np.asarray(params, dtype=np.float64)
    m, K, H = start.shape[0], ms["k"], ms["horizon"]
    need_track = ms["w_progress"] != 0.0 or ms["w_lat"] != 0.0
    o = dict(candidates=np.zeros((m, K, H, 2)), raw=np.zeros((m, K, 4)), cost=np.zeros((m, K)), weight=np.zeros((m, K)), actions=np.zeros((m, 2)),
             info=np.zeros((m, 4), dtype=np.float32), nominal=np.zeros((m, H, 2)), streams=np.zeros((m, 4), dtype=np.uint64), near=np.zeros((m, K)),
             gap=np.zeros(m), beta=np.zeros(m), best=np.zeros(m, dtype=np.int64), opp_raw=np.zeros((m, K, 2)), opp_near=np.zeros((m, K)),
             pred=np.zeros((m, np.asarray(opp).shape[1], H, 2)))
    for n in range(m):
        U = np.array(nominal[n], dtype=np.float64)
        if fresh is not None and int(fresh[n]) == 0:
            U[:, 0], U[:, 1] = 0.0, ms["v_init"]
        V = mr.candidates(ms, U, streams[n])
        end, alive, mc, poses, near = rr.fly(so, start[n:n + 1], params[n:n + 1], V[None], True, ms["repeat"], ms["margin"], integrator, lidar_dist, time_step)
        pred = predict(s, float(start[n, 0]), float(start[n, 1]), opp[n], H, ms["repeat"], time_step, track)
        oraw, onear = sample_rows(s, poses, pred[None])
        prog, lat = np.zeros(K), np.zeros(K)
        if need_track:
            s0 = track_oracle(track, start[n:n + 1, [0, 1, 4]])
            s1 = track_oracle(track, end[0][:, [0, 1, 4]])
            for k in range(K):
                prog[k] = rr.wrap(float(s1[k, 0]) - float(s0[0, 0]), track.closed, track.length)
                lat[k] = s1[k, 1]
        raw4 = np.stack([alive[0].astype(np.float64), mc[0], prog, lat], axis=-1)
        cost = [float(c) for c in costs(ms, w_hit, w_near, near_ref, raw4[None], oraw)[0]]
        w, Un, beta, best, eta, q = mr.update(ms, V, cost)
        o["candidates"][n], o["cost"][n], o["weight"][n], o["actions"][n], o["nominal"][n] = V, cost, w, Un[0], mr.shifted(ms, Un)
        o["raw"][n], o["opp_raw"][n], o["opp_near"][n], o["pred"][n] = raw4, oraw[0], onear[0], pred
        with np.errstate(over="ignore", invalid="ignore"):
            o["info"][n] = np.array([beta, cost[0], eta * eta / q, float(best)]).astype(np.float32)
        o["streams"][n] = mr.words_of(mr.generator(streams[n], 1 << 28))
        o["near"][n], o["beta"][n], o["best"][n] = near[0], beta, best
        rest = sorted(cost)
        o["gap"][n] = rest[1] - rest[0] if K > 1 and math.isfinite(rest[0]) else INF
    return o


# ---- the grid both test files walk ------------------------------------------------------------------------------------------------------
GRID_AO = (0, 1, 2, 4)
GRID_ROWS = 3
RADIUS = 0.45


@functools.lru_cache(maxsize=None)
def grid_opponents(map_name, Ao, seed=0):
    """[3][Ao][4]: opponents around the grid's first three rows, 0.3 .. 2.5 m away, speeds of both signs; the last one of four is
    far away (outside the finite max_range the track cases use)"""
    start = rr.grid_rows(map_name)[0][:GRID_ROWS]
    rng = np.random.default_rng(77 + seed + 10 * Ao + len(map_name))
    opp = np.zeros((GRID_ROWS, Ao, 4))
    for n in range(GRID_ROWS):
        for o in range(Ao):
            r, phi = rng.uniform(0.3, 2.5), rng.uniform(-math.pi, math.pi)
            opp[n, o] = (start[n, 0] + r * math.cos(phi), start[n, 1] + r * math.sin(phi), rng.uniform(-1.0, 4.0), start[n, 4] + rng.uniform(-0.5, 0.5))
        if Ao == 4:
            opp[n, 3, :2] += 40.0
    return opp


def grid_settings(mode, Ao):
    return settings(mode=mode, radius=RADIUS, max_range=30.0 if Ao == 4 else INF)


def left_out(near, radius):
    """the candidates whose decisive comparison d < radius is within 1e-9 * radius of flipping"""
    return near < 1e-9 * radius


# ---- the GPU test's grid (tests/test_gpu_opponents.py; tests/test_opponents_host.py holds its seeds to the leave-out rule) ---------------
GPU_K = (1, 63, 64, 65)
GPU_H = (1, 2, 8)
GPU_REPEAT = (1, 3)


def gpu_cases(map_names=rr.GRID_MAPS, modes=MODES):
    return [(mp, K, H, repeat, mode, Ao) for mp in map_names for mode in modes for K in GPU_K for H in GPU_H for repeat in GPU_REPEAT for Ao in GRID_AO]


def gpu_inputs(case):
    """(start [3][10], params [3][18], actions [K][H][2] shared, opp [3][Ao][4])"""
    map_name, K, H, _, _, Ao = case
    start, params = (a[:GRID_ROWS] for a in rr.grid_rows(map_name))
    return start, params, rr.grid_actions(K, H, False), grid_opponents(map_name, Ao)


@functools.lru_cache(maxsize=None)
def gpu_flown(map_name, K, H, repeat):
    start, params = (a[:GRID_ROWS] for a in rr.grid_rows(map_name))
    return rr.fly(rr.scan_oracle(map_name), start, params, rr.grid_actions(K, H, False), False, repeat, rr.GRID_MARGIN, 1)


def live_opponents(state, A):
    """[N][A - 1][4] = x, y, v, theta of every agent's opponents: the env's other agents in ascending slot"""
    N = state.shape[0]
    out = np.zeros((N, A - 1, 4))
    for n in range(N):
        e, a = divmod(n, A)
        for o in range(A - 1):
            nb = e * A + (o if o < a else o + 1)
            out[n, o] = state[nb, [0, 1, 3, 4]]
    return out


# ---- the edge grid (tests/test_gpu_opponents_edges.py; tests/test_opponents_host.py holds it to the leave-out rule) ----------------------
# k_opp_predict gives a (row, opponent) 16 lanes, lane `sub` writes the actions sub, sub + 16, ...: H = 15, 16, 17 lie around the end
# of the first lap, 32 and 33 around the end of the second, 64 is the limit (four laps).  Three rows x Ao in {5, 16, 31} are 15, 48 and
# 93 groups of 16 lanes in workgroups of 16 groups: one idle group, three full workgroups, a ragged last one; 31 is the limit.
EDGE_KHR = ((5, 15, 1), (5, 16, 1), (5, 17, 1), (5, 32, 2), (5, 33, 1), (64, 64, 1))
EDGE_AO = (5, 16, 31)
EDGE_LIMITS = ("example_map", 5, 64, 16, 5)      # (map, K, H, repeat, Ao): both limits of the horizon at once
EDGE_RANGED = ("berlin", 5, 33, 1, 31)           # the same with a finite max_range: some of the 31 are not looked at
EDGE_MAX_RANGE = 1.5                             # grid_opponents places them 0.3 .. 2.5 m from the row's start


def edge_cases(map_names=rr.GRID_MAPS, modes=MODES):
    """(map, K, H, repeat, mode, Ao, max_range, seed) — seed is grid_opponents' (0 unless a case had to move off a leave-out)"""
    cases = [(mp, K, H, repeat, mode, Ao, INF, 0) for mp in map_names for mode in modes for K, H, repeat in EDGE_KHR for Ao in EDGE_AO]
    for (mp, K, H, repeat, Ao), max_range in ((EDGE_LIMITS, INF), (EDGE_RANGED, EDGE_MAX_RANGE)):
        cases += [(mp, K, H, repeat, mode, Ao, max_range, 0) for mode in modes if mp in map_names]
    return cases


EDGE_CASES = tuple(edge_cases())


def edge_settings(case):
    return settings(mode=case[4], radius=RADIUS, max_range=case[6])


def edge_inputs(case):
    """(start [3][10], params [3][18], actions [K][H][2] shared, opp [3][Ao][4])"""
    map_name, K, H, _, _, Ao, _, seed = case
    start, params = (a[:GRID_ROWS] for a in rr.grid_rows(map_name))
    return start, params, rr.grid_actions(K, H, False), grid_opponents(map_name, Ao, seed)


def edge_pred(case):
    """the model's predictions of a case [3][Ao][H][2]"""
    map_name, _, H, repeat = case[:4]
    s, (start, _, _, opp), track = edge_settings(case), edge_inputs(case), rr.grid_track(map_name)
    return np.stack([predict(s, start[n, 0], start[n, 1], opp[n], H, repeat, track=track) for n in range(len(start))])


def nan_rows_between_finite(pred):
    """does every row of pred [m][Ao][H][2] hold an ignored opponent (all NaN) with a predicted one on either side of it?"""
    gone = np.all(np.isnan(pred), axis=(2, 3))
    assert np.array_equal(gone, np.any(np.isnan(pred), axis=(2, 3))), "an opponent is ignored at some actions only"
    return all(any(row[o] and not row[:o].all() and not row[o + 1:].all() for o in range(1, len(row) - 1)) for row in gone)


# ---- the hand cases both test files work out (tests/test_opponents_host.py on the host harness, tests/test_gpu_opponents_edges.py) -------
def hand_row(x, y, theta, v=0.0, fill=2):
    return np.array([[x, y, 0.0, v, theta, 0.0, 0.0, 0.0, 0.0, float(fill)]])


def seam_opponents(track, lap_at=0.875, lat=(0.2, -0.1), tau_last=1.0):
    """three opponents on a closed track [3][4]: one `lap_at` metres before the seam driving forward at 1 m/s, `lat[0]` m left of the
    line; one `lap_at` metres behind the seam driving backward at 1 m/s, -lat[1] m right of it; one at the first fast enough
    that s_o + v tau_last lies beyond 2 L (a single subtraction leaves s >= L)"""
    cols, L = track_cols(track), track.length
    out = []
    for s_at, l, v in ((L - lap_at, lat[0], 1.0), (lap_at, lat[1], -1.0), (L - lap_at, lat[0], 2.5 * L / tau_last)):
        X, Y, ux, uy = station(cols, s_at)
        out.append([X - l * uy, Y + l * ux, v, 0.0])
    return np.array(out)


def stations_of(track, opp_row, H, repeat, time_step=rr.TIME_STEP):
    """s_o + v tau_h before the wrap, per action: what the model's TRACK rule hands to its one subtraction"""
    s_o = float(track_oracle(track, np.array([[opp_row[0], opp_row[1], 0.0]]))[0, 0])
    return np.array([s_o + float(opp_row[2]) * tau(h, repeat, time_step) for h in range(H)])
