"""The model of the MPPI planner (include/f110.h, f110_mppi): plain Python loops on top of the rollout's model
(tests/rollout_ref.py: fly, the oracle's update_pose and clearance; tests/_util.track_oracle) and NumPy's own generator — a
candidate's draws are PCG64 with the agent's state, .advance(k << 20), then Generator.standard_normal() draw by draw.  The
exponential is math.exp (np.exp differs from it by an ulp here, and only math.exp can be bit-equal to a host build); the sums are
loops in ascending k from 0.0.  Shared by the CPU tests (tests/test_mppi_host.py) and the GPU tests (tests/test_gpu_mppi.py)."""
import math

import numpy as np

import rollout_ref as rr
from _util import track_oracle

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
