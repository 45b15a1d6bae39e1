"""The model of the particle filter (include/f110.h, f110_pf): plain Python loops over NumPy's own generator — a
sub-stream is PCG64 with the agent's state, .advance(q << 16), then Generator.random() or Generator.standard_normal() draw by draw —
the oracle's scan (ScanOracle.scan(pose)[b_j]) for the expected ranges, and math functions; every sum is a loop over ascending indices
from 0.0.  The stages are functions of their own, so that the GPU tests (tests/test_gpu_particle_filter.py, tests/test_gpu_particle_filter_edges.py) can hold each stage of
the device to the model on the device's own input to it; the CPU tests (tests/test_particle_filter_host.py) chain them (`call`)."""
import bisect
import math

import numpy as np

from _util import oracle_map_dt
from mppi_ref import GATE, gated, generator, same_bits, stream_of, streams_for, words_of   # noqa: F401  (shared with the GPU tests)
from oracle import orc

INF, NAN = float("inf"), float("nan")
TWO_PI = 2.0 * math.pi
SPEC_INTS = ("particles", "n_beams", "beam_first", "beam_stride")
SPEC_FLOATS = ("sigma_x", "sigma_y", "sigma_theta", "init_x", "init_y", "init_theta", "sigma_hit", "clip", "squash", "resample_frac")
NUM_BEAMS, FOV = 1080, 4.7


def settings(**kw):
    s = dict(particles=7, n_beams=7, beam_first=3, beam_stride=18, sigma_x=0.05, sigma_y=0.02, sigma_theta=0.02, init_x=0.1, init_y=0.1,
             init_theta=0.05, sigma_hit=0.1, clip=3.0, squash=2.0, resample_frac=0.5)
    s.update(kw)
    return s


def largest_stride(s, num_beams=NUM_BEAMS):
    return max(1, (num_beams - 1 - s["beam_first"]) // max(1, s["n_beams"] - 1))


def scan_oracle(name, num_beams=NUM_BEAMS, fov=FOV):
    so = orc.ScanOracle(num_beams, fov)
    dt, res, origin = oracle_map_dt(name)
    so.set_map_dt(dt, res, origin)
    return so


def wrap(th):
    if th > TWO_PI:
        return th - TWO_PI
    if th < 0:
        return th + TWO_PI
    return th


# ---- the stages ------------------------------------------------------------------------------------------------------------------
def draws(s, words):
    """(u, noise [P][3], the stream's words after the call)"""
    P = s["particles"]
    u = float(np.random.Generator(generator(words, 0)).random())
    noise = np.zeros((P, 3))
    for p in range(P):
        gen = np.random.Generator(generator(words, (p + 1) << 16))
        for c in range(3):
            noise[p, c] = float(gen.standard_normal())
    return u, noise, words_of(generator(words, 1 << 28))


def resampling(s, W, u):
    """(resampled, ancestors [P], ess, near [P]: slot i's smallest |t_i - C_j| / C_{P-1} over the boundaries, inf without resampling)
    from the stored weights.  The least j with C_j > t_i is found by bisection in the list C, which does not decrease."""
    P = s["particles"]
    q = 0.0
    for p in range(P):
        q = q + float(W[p]) * float(W[p])
    ess = 1.0 / q
    if not ess < s["resample_frac"] * float(P):
        return False, np.arange(P, dtype=np.int32), ess, np.full(P, INF)
    C, c = [], 0.0
    for p in range(P):
        c = c + float(W[p])
        C.append(c)
    anc, near, Ca = np.zeros(P, dtype=np.int32), np.zeros(P), np.array(C)
    for i in range(P):
        t = (float(i) + u) / float(P) * C[P - 1]
        anc[i] = min(bisect.bisect_right(C, t), P - 1)
        near[i] = float(np.min(np.abs(Ca - t))) / C[P - 1]
    return True, anc, ess, near


def odometry(last, pose):
    x, y, th = (float(v) for v in pose)
    dx, dy = x - float(last[0]), y - float(last[1])
    c, sn = math.cos(float(last[2])), math.sin(float(last[2]))
    a = c * dx + sn * dy
    b = -sn * dx + c * dy
    dth = th - float(last[2])
    if dth > math.pi:
        dth = dth - TWO_PI
    elif dth <= -math.pi:
        dth = dth + TWO_PI
    return a, b, dth


def moved(s, X, anc, noise, pose, last, fresh):
    """the cloud after the fresh or the motion rule: [P][3]"""
    P = s["particles"]
    x, y, th = (float(v) for v in pose)
    out = np.zeros((P, 3))
    if fresh:
        for p in range(P):
            e = [float(v) for v in noise[p]]
            out[p] = (x + s["init_x"] * e[0], y + s["init_y"] * e[1], wrap(th + s["init_theta"] * e[2]))
        return out
    a, b, dth = odometry(last, pose)
    for p in range(P):
        e = [float(v) for v in noise[p]]
        sx, sy, sth = (float(v) for v in X[int(anc[p])])
        fa, fb = a + s["sigma_x"] * e[0], b + s["sigma_y"] * e[1]
        c, sn = math.cos(sth), math.sin(sth)
        out[p] = (sx + (c * fa - sn * fb), sy + (sn * fa + c * fb), wrap(sth + dth + s["sigma_theta"] * e[2]))
    return out


def beams(s):
    return [s["beam_first"] + j * s["beam_stride"] for j in range(s["n_beams"])]


def expected(s, so, X, lidar_dist=0.0):
    """the noise-free ranges of the compared beams at every particle's lidar pose: [P][B']"""
    P, idx = s["particles"], beams(s)
    out = np.zeros((P, len(idx)))
    for p in range(P):
        x, y, th = (float(v) for v in X[p])
        if lidar_dist != 0.0:
            x, y = x + lidar_dist * math.cos(th), y + lidar_dist * math.sin(th)
        out[p] = so.scan(np.array([x, y, th]))[idx]
    return out


def logw(s, z, r):
    """L [P] from the scan row z [B] and the expected ranges r [P][B']"""
    P, idx = s["particles"], beams(s)
    c2 = s["clip"] * s["clip"]
    L = np.zeros(P)
    for p in range(P):
        acc = 0.0
        for j, b in enumerate(idx):
            e = (float(z[b]) - float(r[p, j])) / s["sigma_hit"]
            e2 = e * e
            if e2 < c2:
                t = e2
            elif e2 != e2 and c2 == INF:
                t = 0.0
            else:
                t = c2
            acc = acc + t
        L[p] = -(0.5 / s["squash"]) * acc
    return L


def exp_(x):
    try:
        return math.exp(x)
    except OverflowError:
        return INF


def update(s, Wprior, L, X, pose, resampled):
    """(W' [P], estimate [3], info float32 [4]) from the prior weights, L and the moved cloud"""
    P = s["particles"]
    x, y, _ = (float(v) for v in pose)
    Lmax = float(L[0])
    for p in range(1, P):
        if float(L[p]) > Lmax:
            Lmax = float(L[p])
    w, eta = [], 0.0
    for p in range(P):
        d = float(L[p]) - Lmax
        w.append(float(Wprior[p]) * (d if d != d else exp_(d)))
        eta = eta + w[p]
    Wn = [w[p] / eta for p in range(P)] if eta > 0 else [1.0 / float(P)] * P
    xh = yh = sn = cs = q = 0.0
    for p in range(P):
        xh = xh + Wn[p] * float(X[p, 0])
        yh = yh + Wn[p] * float(X[p, 1])
        sn = sn + Wn[p] * math.sin(float(X[p, 2]))
        cs = cs + Wn[p] * math.cos(float(X[p, 2]))
        q = q + Wn[p] * Wn[p]
    spread = 0.0
    for p in range(P):
        dx, dy = float(X[p, 0]) - xh, float(X[p, 1]) - yh
        spread = spread + Wn[p] * (dx * dx + dy * dy)
    info = np.array([1.0 / q, math.sqrt(spread), math.hypot(xh - x, yh - y), 1.0 if resampled else 0.0], dtype=np.float32)
    return np.array(Wn), np.array([xh, yh, math.atan2(sn, cs)]), info


# ---- one call on m rows ------------------------------------------------------------------------------------------------------------
def call(s, so, poses, scans, particles, weights, last, streams, fresh=None, lidar_dist=0.0):
    """-> dict: pose [m][3], info float32 [m][4], noise [m][P][3], ancestors [m][P], expected [m][P][B'], logw [m][P], particles,
    weights, last and streams after the call, near [m] (resampling's smallest slot-to-boundary distance, relative) and ess_gap [m]
    (|ess - resample_frac * P| / P)"""
    poses = np.asarray(poses, dtype=np.float64)
    m, P, Bp = poses.shape[0], s["particles"], s["n_beams"]
    o = dict(pose=np.zeros((m, 3)), info=np.zeros((m, 4), dtype=np.float32), noise=np.zeros((m, P, 3)), ancestors=np.zeros((m, P), dtype=np.int32),
             expected=np.zeros((m, P, Bp)), logw=np.zeros((m, P)), particles=np.zeros((m, P, 3)), weights=np.zeros((m, P)), last=np.zeros((m, 3)),
             streams=np.zeros((m, 4), dtype=np.uint64), near=np.full(m, INF), ess_gap=np.full(m, INF))
    for n in range(m):
        is_fresh = fresh is not None and int(fresh[n]) == 0
        u, noise, words = draws(s, streams[n])
        res, anc = False, np.arange(P, dtype=np.int32)
        if not is_fresh:
            res, anc, ess, near = resampling(s, weights[n], u)
            o["near"][n], o["ess_gap"][n] = float(np.min(near)), abs(ess - s["resample_frac"] * float(P)) / float(P)
        X = moved(s, particles[n], anc, noise, poses[n], last[n], is_fresh)
        r = expected(s, so, X, lidar_dist)
        L = logw(s, scans[n], r)
        prior = [1.0 / float(P)] * P if (is_fresh or res) else weights[n]
        Wn, est, info = update(s, prior, L, X, poses[n], res)
        o["pose"][n], o["info"][n], o["noise"][n], o["ancestors"][n], o["expected"][n], o["logw"][n] = est, info, noise, anc, r, L
        o["particles"][n], o["weights"][n], o["last"][n], o["streams"][n] = X, Wn, poses[n], words
    return o


def rows_for(map_name, P, m=3, seed=0):
    """m rows with distinct poses on a fixture map (rollout_ref.grid_rows): (so, poses [m][3], scans [m][B] = the oracle's scan plus
    1 cm of noise, particles, weights, last = the pose a short move earlier, streams)"""
    import rollout_ref as rr
    so = rr.scan_oracle(map_name)
    poses = np.ascontiguousarray(rr.grid_rows(map_name)[0][np.arange(m) % 6][:, [0, 1, 4]])
    poses[:, 2] = np.mod(poses[:, 2], TWO_PI)
    rng = np.random.default_rng(9000 + seed)
    scans = np.stack([so.scan(p) for p in poses]) + rng.normal(0.0, 0.01, (m, NUM_BEAMS))
    X, W = cloud_around(poses, P, 100 + seed)
    last = poses - np.column_stack([0.04 * np.cos(poses[:, 2]), 0.04 * np.sin(poses[:, 2]), rng.uniform(-0.02, 0.02, m)])
    last[:, 2] = np.mod(last[:, 2], TWO_PI)
    return so, poses, scans, X, W, last, streams_for(4000 + seed, range(m))


UNIT_P = (1, 2, 63, 64, 65)
UNIT_B = (1, 7, 64, 65, 128)
UNIT_FRESH = np.array([4, 0, 9], dtype=np.int32)      # row 1 is fresh


def unit_case(map_name, P, Bp, big_stride, q):
    """case q of the GPU tests' unit grid: (settings, (poses, scans, particles, weights, last, streams, fresh)).  Three rows with
    distinct poses: row 0 holds uniform weights (resampled only when resample_frac is 2), row 1 is fresh, row 2 holds uneven ones;
    resample_frac and the truncation alternate with q"""
    s = settings(particles=P, n_beams=Bp, beam_first=2, beam_stride=1, resample_frac=(0.5, 2.0)[q % 2], clip=(3.0, INF)[q // 2 % 2])
    if big_stride:
        s["beam_stride"] = largest_stride(s)
    so, poses, scans, X, W, last, words = rows_for(map_name, P, seed=300 + q)
    W[0] = 1.0 / float(P)
    return s, (poses, scans, X, W, last, words, UNIT_FRESH)


def filter_of(amd, s):
    return amd.ParticleFilter(**s)


# ---- the update kernel's lane groupings (tests/test_gpu_particle_filter_edges.py) -------------------------------------------------------
def group_lanes(P):
    """a Python copy of pf_group_lanes (f110_kernels.hpp): the lanes k_pf_update gives an agent — the power of two >= min(P, 256), at
    least 16; a workgroup of 256 lanes then holds 256 / GS agents, and a lane walks its particles in ceil(P / GS) passes"""
    need = min(P, 256)
    gs = 16
    while gs < need:
        gs <<= 1
    return gs


# P on both sides of every bound of the grouping: 16 | 17 (GS 16 -> 32), 32 | 33 (-> 64), 128 | 129 (-> 256), and 256 | 257, where GS
# stays 256 and the lanes take a second pass
EDGE_P = (16, 17, 32, 33, 128, 129, 256, 257)
EDGE_B = (7, 64)


def edge_cases(map_names=("example_map", "berlin"), Ps=EDGE_P):
    """(map, P, B', the largest stride?, q) in unit_case's terms: q = 0 .. 3 in itertools.product(EDGE_B, (False, True)) order"""
    return [(mp, P, Bp, big, q) for mp in map_names for P in Ps for q, (Bp, big) in enumerate((b, g) for b in EDGE_B for g in (False, True))]


def cloud_around(poses, P, seed, spread=(0.15, 0.15, 0.08)):
    """a stored cloud [m][P][3] around the poses, with weights [m][P] of uneven size (normalised)"""
    rng = np.random.default_rng(seed)
    poses = np.asarray(poses, dtype=np.float64)
    X = poses[:, None, :] + rng.normal(0.0, 1.0, (poses.shape[0], P, 3)) * np.asarray(spread)
    X[..., 2] = np.mod(X[..., 2], TWO_PI)
    W = rng.uniform(0.05, 1.0, (poses.shape[0], P)) ** 3
    return X, W / W.sum(axis=1, keepdims=True)


# ---- what the GPU tests share (tests/test_gpu_particle_filter.py) ---------------------------------------------------------------------
def new_stats():
    return {"rows": 0, "rows_left_out": 0, "slots": 0, "slots_left_out": 0, "rel_err": 0.0}


def leave_outs_ok(stats):
    return stats["rows_left_out"] * 100 <= stats["rows"] and stats["slots_left_out"] * 100 <= max(stats["slots"], 1)


def _gate(got, want, what, stats, atol=1e-12):
    err = gated(got, want, what, atol=atol)
    stats["rel_err"] = max(stats["rel_err"], err)
    assert err < GATE, "%s: rel_err %.3e" % (what, err)


def check_stages(s, so, inp, got, what, stats, lidar_dist=0.0):
    """the device's unit-form dict `got` against the model, stage by stage, each stage on the device's own input to it.
    inp = (poses, scans, particles, weights, last, streams, fresh) as they went in.  Left out: a row whose ESS lies within 1e-9 * P
    of the threshold (its decision, and everything behind it, is not compared), a slot whose t_i lies within 1e-9 * C_{P-1} of a
    cumulative boundary (its ancestor is not compared)."""
    poses, scans, X0, W0, last0, words0, fresh = inp
    m, P = np.asarray(poses).shape[0], s["particles"]
    for n in range(m):
        w = "%s row %d" % (what, n)
        is_fresh = fresh is not None and int(fresh[n]) == 0
        u, noise, words = draws(s, words0[n])
        assert same_bits(got["noise"][n], noise), "%s: the draws" % w
        assert same_bits(got["streams"][n], words), "%s: the stream's position" % w
        stats["rows"] += 1
        res_dev = bool(got["info"][n, 3] == 1.0)
        assert got["info"][n, 3] in (0.0, 1.0), w
        if is_fresh:
            assert not res_dev and np.array_equal(got["ancestors"][n], np.arange(P)), "%s: a fresh row resampled" % w
        else:
            res, anc, ess, near = resampling(s, W0[n], u)
            if abs(ess - s["resample_frac"] * float(P)) <= 1e-9 * P:
                stats["rows_left_out"] += 1
            else:
                assert res_dev == res, "%s: the resampling decision (ess %.17g)" % (w, ess)
                keep = near > 1e-9
                stats["slots"] += P
                stats["slots_left_out"] += int(np.count_nonzero(~keep))
                assert np.array_equal(got["ancestors"][n][keep], anc[keep]), "%s: the ancestors" % w
            assert np.all((got["ancestors"][n] >= 0) & (got["ancestors"][n] < P)), w
        X = moved(s, X0[n], got["ancestors"][n], got["noise"][n], poses[n], last0[n], is_fresh)
        _gate(got["particles"][n], X, (w, "moved particles"), stats)
        r = expected(s, so, got["particles"][n], lidar_dist)
        _gate(got["expected"][n], r, (w, "expected ranges"), stats)
        L = logw(s, scans[n], got["expected"][n])
        assert same_bits(got["logw"][n], L), "%s: L given the device's expected ranges" % w
        prior = np.full(P, 1.0 / float(P)) if (is_fresh or res_dev) else W0[n]
        Wn, est, info = update(s, prior, got["logw"][n], got["particles"][n], poses[n], res_dev)
        _gate(got["weights"][n], Wn, (w, "weights"), stats)
        _gate(got["pose"][n], est, (w, "estimate"), stats)
        _gate(got["info"][n, :3], info[:3], (w, "info"), stats, atol=1e-6)
        assert same_bits(got["last"][n], np.asarray(poses[n], dtype=np.float64)), "%s: last" % w


# ---- the device form's inputs and outputs ---------------------------------------------------------------------------------------------
STATE_KEYS = ("particles", "weights", "last", "streams")


def live_rows(sim, agents):
    """the device's own inputs of the armed rows: (poses, scans, step_count) of the observation, and the filter's state"""
    o = sim.get("agent_poses", "scans", "step_count")
    return o["agent_poses"][agents], o["scans"][agents], o["step_count"][agents].astype(np.int32), sim.get_pf_state()


def poisoned(sim, seed):
    rng = np.random.default_rng(seed)
    pa, pi = rng.normal(size=(sim.N, 3)), rng.normal(size=(sim.N, 4)).astype(np.float32)
    d_pose, d_info = sim.device_array((sim.N, 3)), sim.device_array((sim.N, 4), np.float32)
    d_pose.upload(pa)
    d_info.upload(pi)
    return d_pose, d_info, pa, pi


def localize_and_check(amd, sim, s, so, agents, d_pose, d_info, what, stats, slot=0):
    """one device call held to the unit form on the state fetched before it (bit for bit), and the unit form to the model"""
    poses, scans, count, (X, W, last, words) = live_rows(sim, agents)
    sim.localize_device(d_pose, d_info)
    pose, info = d_pose.download(), d_info.download()
    after = dict(zip(STATE_KEYS, sim.get_pf_state()))
    unit = sim.localize_rows(filter_of(amd, s), poses, scans, X, W, last, words, slot=slot, fresh=count)
    assert same_bits(pose[agents], unit["pose"]) and same_bits(info[agents], unit["info"]), "%s: the device form against the unit form" % (what,)
    for key in STATE_KEYS:
        assert same_bits(after[key], unit[key]), "%s: %s, the device form against the unit form" % (what, key)
    check_stages(s, so, (poses, scans, X, W, last, words, count), unit, what, stats)
    return pose, info, count


def seed_clouds(sim, s, agents, seed):
    """clouds around the live poses with uneven weights, and the last poses a short move earlier"""
    poses = sim.get("agent_poses")["agent_poses"][agents]
    X, W = cloud_around(poses, s["particles"], seed)
    last = poses - np.column_stack([0.03 * np.cos(poses[:, 2]), 0.03 * np.sin(poses[:, 2]), np.full(len(agents), 0.01)])
    last[:, 2] = np.mod(last[:, 2], TWO_PI)
    W[::2] = 1.0 / s["particles"]                     # every other row holds uniform weights: it is not resampled
    sim.set_pf_state(X, W, last)
