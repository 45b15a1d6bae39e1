"""The model of the MPPI planner (include/f110.h, f110_mppi): plain Python loops on top of the rollout's model
(tests/rollout_ref.py: fly, the oracle's update_pose and clearance; tests/_util.track_oracle) and NumPy's own generator — a
candidate's draws are PCG64 with the agent's state, .advance(k << 20), then Generator.standard_normal() draw by draw.  The
exponential is math.exp (np.exp differs from it by an ulp here, and only math.exp can be bit-equal to a host build); the sums are
loops in ascending k from 0.0.  Shared by the CPU tests (tests/test_mppi_host.py) and the GPU tests (tests/test_gpu_mppi.py,
tests/test_gpu_mppi_edges.py), whose common helpers (the gate, the leave-out rule, the warm handle) are at the end."""
import math
import os

import numpy as np

import rollout_ref as rr
from _util import MAPS, bench_start_poses, load_map_image, rel_err, track_oracle

INF = float("inf")
MASK64 = (1 << 64) - 1
SPEC_INTS = ("k", "horizon", "repeat", "shift")
SPEC_FLOATS = ("margin", "sigma_steer", "sigma_speed", "steer_min", "steer_max", "speed_min", "speed_max", "lam", "w_dead", "w_clear",
               "w_progress", "w_lat", "clear_ref", "v_init")


def settings(**kw):
    s = dict(k=4, horizon=3, repeat=1, shift=1, margin=0.3, sigma_steer=0.15, sigma_speed=1.0, steer_min=-0.4, steer_max=0.4, speed_min=0.5,
             speed_max=7.0, lam=1.0, w_dead=10.0, w_clear=20.0, w_progress=0.0, w_lat=0.0, clear_ref=0.6, v_init=2.0)
    s.update(kw)
    return s


def stream_of(seed, key):
    """the words {state.hi, state.lo, inc.hi, inc.lo} of PCG64(SeedSequence(seed, spawn_key=(key,)))"""
    st = np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(int(key),))).state["state"]
    return np.array([st["state"] >> 64, st["state"] & MASK64, st["inc"] >> 64, st["inc"] & MASK64], dtype=np.uint64)


def generator(words, advance):
    bg = np.random.PCG64()
    w = [int(v) for v in words]
    bg.state = {"bit_generator": "PCG64", "state": {"state": (w[0] << 64) | w[1], "inc": (w[2] << 64) | w[3]}, "has_uint32": 0, "uinteger": 0}
    bg.advance(advance)
    return bg


def words_of(bg):
    st = bg.state["state"]
    return np.array([st["state"] >> 64, st["state"] & MASK64, st["inc"] >> 64, st["inc"] & MASK64], dtype=np.uint64)


def clamp(x, lo, hi):
    return lo if x < lo else (hi if x > hi else x)


def candidates(s, U, words):
    """V [K][H][2] around the nominal U [H][2] for one agent"""
    K, H = s["k"], s["horizon"]
    V = np.zeros((K, H, 2))
    V[0] = U
    for k in range(1, K):
        gen = np.random.Generator(generator(words, k << 20))
        for h in range(H):
            e_s = float(gen.standard_normal())
            e_v = float(gen.standard_normal())
            V[k, h, 0] = clamp(float(U[h, 0]) + s["sigma_steer"] * e_s, s["steer_min"], s["steer_max"])
            V[k, h, 1] = clamp(float(U[h, 1]) + s["sigma_speed"] * e_v, s["speed_min"], s["speed_max"])
    return V


def cost_of(s, alive, min_clear, progress, end_lat):
    c = s["w_dead"] * float(s["horizon"] * s["repeat"] - alive)
    c = c + s["w_clear"] * (s["clear_ref"] - min_clear if min_clear < s["clear_ref"] else 0.0)
    c = c - s["w_progress"] * progress
    c = c + s["w_lat"] * abs(end_lat)
    return INF if c != c else c


def update(s, V, cost):
    """(weights [K], U' [H][2], beta, best, eta, q) from the candidates and their costs"""
    K, H = s["k"], s["horizon"]
    beta, best = cost[0], 0
    for k in range(1, K):
        if cost[k] < beta:
            beta, best = cost[k], k
    if not math.isfinite(beta):
        w = [1.0] + [0.0] * (K - 1)
    else:
        w = [math.exp(-(cost[k] - beta) / s["lam"]) for k in range(K)]
    eta = q = 0.0
    for k in range(K):
        eta = eta + w[k]
        q = q + w[k] * w[k]
    Un = np.zeros((H, 2))
    for h in range(H):
        for c in range(2):
            num = 0.0
            for k in range(K):
                num = num + w[k] * float(V[k, h, c])
            Un[h, c] = num / eta
    return w, Un, beta, best, eta, q


def shifted(s, Un):
    if not s["shift"]:
        return Un.copy()
    out = Un.copy()
    out[:-1] = Un[1:]
    return out


def plan(s, so, start, params, nominal, streams, integrator, fresh=None, track=None, lidar_dist=0.0, time_step=rr.TIME_STEP):
    """one call on m rows: start [m][10], params [m][18], nominal [m][H][2], streams uint64 [m][4], fresh [m] step counts or None.
    -> dict: candidates [m][K][H][2], raw [m][K][4] (ALIVE, MIN_CLEAR, PROGRESS, END_LAT), cost, weight [m][K], actions [m][2],
    info float32 [m][4], nominal and streams after the call, near [m][K] (the smallest |d - margin| the candidate saw), gap [m] (the
    second lowest cost minus the lowest, inf with one candidate), beta, best [m]"""
    start, params = np.asarray(start, dtype=np.float64), np.asarray(params, dtype=np.float64)
    m, K, H = start.shape[0], s["k"], s["horizon"]
    need_track = s["w_progress"] != 0.0 or s["w_lat"] != 0.0
    assert not need_track or track is not None
    o = dict(candidates=np.zeros((m, K, H, 2)), raw=np.zeros((m, K, 4)), cost=np.zeros((m, K)), weight=np.zeros((m, K)), actions=np.zeros((m, 2)),
             info=np.zeros((m, 4), dtype=np.float32), nominal=np.zeros((m, H, 2)), streams=np.zeros((m, 4), dtype=np.uint64), near=np.zeros((m, K)),
             gap=np.zeros(m), beta=np.zeros(m), best=np.zeros(m, dtype=np.int64))
    for n in range(m):
        U = np.array(nominal[n], dtype=np.float64)
        if fresh is not None and int(fresh[n]) == 0:
            U[:, 0], U[:, 1] = 0.0, s["v_init"]
        V = candidates(s, U, streams[n])
        end, alive, mc, _, near = rr.fly(so, start[n:n + 1], params[n:n + 1], V[None], True, s["repeat"], s["margin"], integrator, lidar_dist, time_step)
        prog, lat = np.zeros(K), np.zeros(K)
        if need_track:
            s0 = track_oracle(track, start[n:n + 1, [0, 1, 4]])
            s1 = track_oracle(track, end[0][:, [0, 1, 4]])
            for k in range(K):
                prog[k] = rr.wrap(float(s1[k, 0]) - float(s0[0, 0]), track.closed, track.length)
                lat[k] = s1[k, 1]
        cost = [cost_of(s, int(alive[0, k]), float(mc[0, k]), float(prog[k]), float(lat[k])) for k in range(K)]
        w, Un, beta, best, eta, q = update(s, V, cost)
        o["candidates"][n], o["cost"][n], o["weight"][n], o["actions"][n], o["nominal"][n] = V, cost, w, Un[0], shifted(s, Un)
        o["raw"][n] = np.stack([alive[0].astype(np.float64), mc[0], prog, lat], axis=-1)
        with np.errstate(over="ignore", invalid="ignore"):
            o["info"][n] = np.array([beta, cost[0], eta * eta / q, float(best)]).astype(np.float32)
        o["streams"][n] = words_of(generator(streams[n], 1 << 28))
        o["near"][n], o["beta"][n], o["best"][n] = near[0], beta, best
        rest = sorted(cost)
        o["gap"][n] = rest[1] - rest[0] if K > 1 and math.isfinite(rest[0]) else INF
    return o


def bits(a):
    return rr.bits(a)


# ---- what the GPU tests share (tests/test_gpu_mppi.py, tests/test_gpu_mppi_edges.py, tests/test_gpu_obstacles_edges.py) --------------------
CSV = os.path.join(MAPS, "example_waypoints.csv")
GATE = 1e-5      # the project's gate


def mppi_of(amd, s):
    kw = {k: v for k, v in s.items()}
    kw["shift"] = bool(kw["shift"])
    return amd.Mppi(**kw)


def streams_for(seed, agents):
    return np.stack([stream_of(seed, g) for g in agents])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def gated(got, want, what, atol=1e-12):
    """rel_err of got against want, after what rel_err cannot see (a NaN or an infinity gives it an excess that is not > 0): the
    device's value is finite exactly where the model's is, and elsewhere it is the model's value itself (+inf, -inf or NaN)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin), "%s: the device's value is not finite where the model's is (or the other way round)" % (what,)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), "%s: a value that is not finite differs from the model's" % (what,)
    return rel_err(got[fin], want[fin], atol=atol)


def check_rows(s, want, got, what, stats):
    """got: the device's dict (actions, info, nominal, streams, and from the unit form candidates, cost, weight) against the model's"""
    assert same_bits(got["streams"], want["streams"]), "%s: stream positions" % (what,)
    if "candidates" in got:
        assert same_bits(got["candidates"], want["candidates"]), "%s: the candidates V" % (what,)
    m = want["actions"].shape[0]
    keep = np.all(want["near"] >= 1e-9, axis=1)                                       # the model's clearance stays 1e-9 m away from the margin
    sure = want["gap"] > 1e-9 * np.maximum(1.0, np.abs(want["beta"]))                 # the model's two lowest costs are apart ...
    for n in np.flatnonzero(want["gap"] == 0.0):                                      # ... or the very same number from the very same rollout
        tied = want["raw"][n][want["cost"][n] == want["beta"][n]]
        sure[n] = bool(np.all(tied.view(np.uint64) == tied[0].view(np.uint64)))
    stats["rows"] += m
    stats["left_out"] += int(np.count_nonzero(~(keep & sure)))
    for key in ("cost", "weight", "actions", "nominal"):
        if key in got:
            err = gated(got[key][keep], want[key][keep], (what, key))
            print("%s: %s rel_err %.3e" % (what, key, err))
            stats["rel_err"] = max(stats["rel_err"], err)
            assert err < GATE, "%s: %s rel_err %.3e" % (what, key, err)
    err = gated(got["info"][keep][:, :3], want["info"][keep][:, :3], (what, "info"), atol=1e-6)
    print("%s: info rel_err %.3e" % (what, err))
    assert err < GATE, "%s: info rel_err %.3e" % (what, err)
    assert np.all(np.isfinite(got["info"][keep][:, 3])), "%s: best is not a number" % (what,)
    assert np.array_equal(got["info"][keep & sure][:, 3], want["info"][keep & sure][:, 3]), "%s: best" % (what,)


def warm_sim(amd, E, A, steps=15, **kw):
    """E x A cars on example_map with its raceline after `steps` steps; the FIFO is then set to known values next to the state read
    back (f110_set_state leaves step_count alone): (sim, start [N][10])"""
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    sim.set_map_image(*load_map_image("example_map"))
    sim.set_track(CSV)
    sim.reset(bench_start_poses(E, A))
    rng = np.random.default_rng(E)
    for _ in range(steps):
        sim.step(np.stack([rng.uniform(-0.1, 0.1, N), rng.uniform(2.0, 4.0, N)], axis=1))
    return sim, pin_fifo(sim, rng)


def pin_fifo(sim, rng, fifo=None, cnt=None):
    """the live state as the model's start rows, with the FIFO set on the device to the values returned"""
    N = sim.N
    state = sim.get("state")["state"]
    fifo = rng.uniform(-0.1, 0.1, (N, 2)) if fifo is None else fifo
    cnt = np.full(N, 2, dtype=np.int32) if cnt is None else cnt
    sim.set_state(state, fifo, cnt)
    return np.concatenate([state, fifo, cnt[:, None].astype(np.float64)], axis=1)


def two_maps(amd, E=1, A=1, **kw):
    """slot 0: example_map with its raceline; slot 1: berlin with the grid's open polyline"""
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    assert s.add_map_image(*load_map_image("berlin")) == 1
    s.set_track(rr.grid_track("example_map"), 0)
    s.set_track(rr.grid_track("berlin"), 1)
    return s


def nominal_for(s, m, seed=5):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(0.5 * s["steer_min"], 0.5 * s["steer_max"], (m, s["horizon"])),
                     rng.uniform(s["speed_min"], s["speed_max"], (m, s["horizon"]))], axis=-1)


def grid_settings(case):
    """the track weights are always on and the speed noise is small: two candidates whose speed commands both saturate the
    acceleration move alike for as long as their own steering has not left the two-step delay, and would tie for the lowest cost"""
    _, K, H, repeat, _, q = case
    return settings(k=K, horizon=H, repeat=repeat, shift=q // 2 % 2, margin=rr.GRID_MARGIN, w_progress=3.0, w_lat=0.25 * (1 + q % 3), lam=0.5 + 0.25 * (q % 3),
                    sigma_steer=0.1, sigma_speed=0.3, speed_min=-2.0, v_init=1.0)


# ---- the update kernel's lane groupings (tests/test_gpu_mppi_edges.py) -------------------------------------------------------------------
def group_lanes(K, H):
    """a Python copy of mppi_group_lanes (f110_kernels.hpp): the lanes k_mppi_update gives an agent — the power of two
    >= max(2 H, min(K, 64)), at least 16; a workgroup of 256 lanes then holds 256 / GS agents"""
    need = max(2 * H, min(K, 64))
    gs = 16
    while gs < need:
        gs <<= 1
    return gs


# (K, H, rows, GS, agents per workgroup, repeat): every grouping, K on both sides of GS, GS set by K and by 2 H, both limits
LANE_CASES = ((16, 8, 17, 16, 16, 2), (17, 2, 9, 32, 8, 2), (32, 16, 9, 32, 8, 2), (5, 9, 9, 32, 8, 2), (33, 3, 5, 64, 4, 2), (7, 32, 5, 64, 4, 2),
              (255, 1, 5, 64, 4, 2), (3, 33, 3, 128, 2, 2), (256, 64, 3, 128, 2, 1), (2, 1, 17, 16, 16, 16))


def lane_inputs(map_name, integrator, q):
    """row q of LANE_CASES on a grid map: (settings, start, params, nominal, streams, fresh).  Row n is the grid's row n % 6, so the
    rows of one workgroup differ only in their stream; every fifth row is fresh; the nominal speeds lie within 0.3 m/s of the row's
    own speed, clipped into the spec"""
    K, H, M, _, _, repeat = LANE_CASES[q]
    s = grid_settings((map_name, K, H, repeat, integrator, q))
    start, params = rr.grid_rows(map_name)
    idx = np.arange(M) % 6
    start, params = start[idx], params[idx]
    rng = np.random.default_rng(400 + q)
    steer = rng.uniform(-0.2, 0.2, (M, H))
    speed = np.clip(start[:, 3:4] + rng.uniform(-0.3, 0.3, (M, H)), s["speed_min"], s["speed_max"])
    words = streams_for(2000 + q + 100 * rr.GRID_MAPS.index(map_name), range(M))
    return s, start, params, np.stack([steer, speed], axis=-1), words, (np.arange(M) % 5).astype(np.int32)


# a seed whose first stream's draws (K = 64, H = 5) take the ziggurat's wedge test and its tail loop: found once with the host harness's
# hh_mppi_branches, which tests/test_mppi_host.py holds it to
ZIG_SEED = 1
ZIG_BASE = 3.6541528853610088      # the ziggurat's base layer ends here: a larger draw came through the tail


def zig_settings():
    """wide clamps: the draws themselves show in V"""
    return settings(k=64, horizon=5, repeat=1, sigma_steer=0.05, sigma_speed=0.4, steer_min=-10.0, steer_max=10.0, speed_min=-50.0, speed_max=50.0)
