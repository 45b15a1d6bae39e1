"""Randomised fuzzing of exact snapshot / restore / clone (k_state_pack, k_state_unpack, k_clone_envs) and of the env layers'
equivalence under partial resets.

run(seed): a configuration drawn together — E envs of A agents, 1..3 map slots with a random env_map, a vehicle parameter set per
agent or per slot, the integrator, shared-stream device noise with a random row cache (0 included) or a stream per agent, tracking
on or off, device_logic (the episode arrays) on or off, re-seats armed or not, a step entry point drawn per step.  T1 steps, a save
(save_state or save_envs; all envs or a subset; host or device blob; with or without scans), T2 more steps recorded (state, poses,
scans, collision flags, step counters, episode arrays, track columns), then the same T2 steps replayed, bit for bit, after a restore
(a) into the same handle, (b) into a fresh handle with another row cache, (c) of a subset blob into other env indices of a handle
with another env count.  Then one env cloned into others, all stepped with its actions: every clone equals it at every step.  The
restored run (b) is also held against the CPU oracle (SimOracle, 1e-9) for envs the run never re-seated (shared-stream noise).

run_env(seed): ShardedVecEnv (1..5 shards of random sizes, all on device 0) against one F110VecEnv of the same E, device_logic on or
off, tracking with reward='progress', random partial reset masks (one per seed covers exactly one whole shard), snapshot() / restore()
in between: every returned array bit-equal at every step.

1 000 seeds of each (0 .. 999) run by hand on one MI355X without a mismatch.
    python tools/debug/fuzz_snapshot.py 0 40          # run(), seeds 0..39
    python tools/debug/fuzz_snapshot.py 0 40 env      # run_env()
"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from _util import MAPS, bench_start_poses, load_map_image, map_stem, oracle_map_dt, raceline, rel_err
from oracle import orc
import f1tenth_gym_amd as amd

SEED, STD = 12345, 0.01
ALL = ("scans", "state", "agent_poses", "collisions", "collision_idx", "in_collision", "step_count")
CSV = os.path.join(MAPS, "example_waypoints.csv")


def _loop(n, r=10.0):
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    rr = r + 0.7 * np.sin(7 * a)
    return np.column_stack([rr * np.cos(a), rr * np.sin(a)])


def _params(rng):
    p = dict(amd.DEFAULT_PARAMS)
    p.update({'mu': rng.uniform(0.6, 1.2), 'm': rng.uniform(3.0, 4.2), 'lf': rng.uniform(0.147, 0.17), 'C_Sf': rng.uniform(4.0, 5.5),
              'a_max': rng.uniform(7.0, 10.0), 'v_max': rng.uniform(12.0, 22.0), 'length': rng.uniform(0.5, 0.62),
              'width': rng.uniform(0.27, 0.34)})
    return p


class Cfg(object):
    pass


def _make(c, E, rows, env_map, start, params, seeds):
    """a handle of E envs with c's configuration; start [E*A][3] the poses it is reset to (and re-seats to)"""
    A = c.A
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=c.B, integrator=c.integ)
    img = load_map_image("example_map")
    s.set_map_image(*img)
    for _ in range(1, c.K):
        s.add_map_image(*img)
    if c.K > 1:
        s.set_env_maps(env_map)
    if c.per_agent:
        s.set_params_batch(params)
    else:
        for a in range(A):
            s.set_params(params[a], a)
    if c.noise == "shared":
        s.set_noise_rng(SEED, STD, cache_rows=rows)
    elif c.noise == "per_agent":
        s.set_noise_rng(None, STD, per_agent_seeds=seeds)
    if c.track:
        for k, t in enumerate(c.tracks):
            s.set_track(t, k)
        s.enable_track()
    h = Cfg()
    h.s = s
    h.d_act = s.device_array((E * A, 2))
    h.hb = s.host_block(("state", "agent_poses"))
    h.d_start = s.device_array((E * A, 3)); h.d_start.upload(start)
    h.d_cnt = s.device_array((1,), np.int32); h.d_cnt.upload(np.zeros(1, np.int32))
    if c.device_logic:
        s.episode_init(0)
        s.episode_reset(start)
    else:
        s.reset(start)
    if c.reseat:
        s.set_auto_reseat(h.d_start, 0, h.d_cnt)
    return h


def _step(c, h, path, act):
    s = h.s
    if path == "step":
        s.step(act)
    elif path in ("step_device", "episode_step_device"):
        h.d_act.upload(act)
        (s.episode_step_device if path == "episode_step_device" else s.step_device)(h.d_act)
    else:
        s.step_host(h.hb, act, fuse=path != "step_host_no_fuse")


def _record(c, h):
    o = h.s.get(*ALL)
    if c.device_logic:
        o.update({"ep_" + k: np.array(v) for k, v in h.s.episode_get().items()})
    if c.track:
        o.update({"trk_" + k: v for k, v in h.s.get_track().items()})
    return o


def _rows(o, envs, A, E):
    """the rows of envs (per-agent columns) or the envs themselves (per-env columns)"""
    ag = np.concatenate([np.arange(e * A, e * A + A) for e in envs])
    return {k: (v[ag] if v.shape[0] == E * A else v[np.asarray(envs)]) for k, v in o.items()}


def _diff(a, b):
    for k in a:
        if not np.array_equal(a[k], b[k], equal_nan=True):
            return k
    return None


def run(seed, verbose=True):
    rng = np.random.default_rng(500000 + seed)
    c = Cfg()
    E = int(rng.choice([int(rng.integers(1, 5)), int(rng.integers(2, 65))]))
    c.A = A = int(rng.choice([1, 2, 2, 3, 4]))
    c.K = int(rng.integers(1, 4))
    c.B = int(rng.choice([1080, 64, 271]))
    c.integ = int(rng.choice([1, 1, 2]))
    c.noise = str(rng.choice(["shared", "shared", "per_agent"]))
    c.per_agent = bool(rng.random() < 0.5)
    c.track = bool(rng.random() < 0.6)
    c.device_logic = bool(rng.random() < 0.5)
    c.reseat = bool(rng.random() < 0.6)
    c.tracks = [amd.Track.from_xy(raceline()[:, 1:3]), amd.Track.from_xy(raceline()[::-1, 1:3]), amd.Track.from_xy(_loop(1500))][:c.K]
    T1, T2 = int(rng.integers(3, 40)), int(rng.integers(3, 30))
    rows = int(rng.choice([0, 7, 64, T1 + T2 + 2]))
    paths = ["episode_step_device", "step_host", "step_host_no_fuse"] if c.device_logic else ["step", "step_device", "step_host", "step_host_no_fuse"]
    path_of = [str(rng.choice(paths)) for _ in range(T1 + T2)]
    N = E * A
    env_map = rng.integers(0, c.K, E) if c.K > 1 else np.zeros(E, np.int64)
    params = [_params(rng) for _ in range(N)] if c.per_agent else [_params(rng) if rng.random() < 0.5 else dict(amd.DEFAULT_PARAMS) for _ in range(A)]
    seeds = [int(v) for v in rng.integers(0, 1 << 31, N)]
    start = bench_start_poses(E, A, gap_wp=int(rng.integers(3, 8)))
    acts = np.empty((T1 + T2 + 40, N, 2))
    for t in range(acts.shape[0]):   # calm, held actions (fuzz_envs.py): the oracle check stays within 1e-9
        if t % 9 == 0:
            a = np.stack([rng.uniform(-0.25, 0.25, N), rng.uniform(0.5, 6.0 if rng.random() < 0.7 else 12.0, N)], axis=1)
        acts[t] = a
    save_kind = str(rng.choice(["save_state", "save_envs"]))
    subset = np.sort(rng.choice(E, int(rng.integers(1, E + 1)), replace=False)) if save_kind == "save_envs" and rng.random() < 0.6 else np.arange(E)
    scans, device = bool(rng.random() < 0.5), bool(rng.random() < 0.5)
    tag = "seed %d E%d A%d K%d B%d integ%d noise %s rows %d params %s track %s logic %s reseat %s T1 %d T2 %d save %s %d envs%s%s" % (
        seed, E, A, c.K, c.B, c.integ, c.noise, rows, "per-agent" if c.per_agent else "per-slot", c.track, c.device_logic, c.reseat, T1, T2,
        save_kind, subset.size, " scans" if scans else "", " device" if device else "")

    def fail(what, t, key):
        print("MISMATCH", tag, what, "step", t, "column", key)
        return False

    h = _make(c, E, rows, env_map, start, params, seeds)
    handles = [h]
    try:
        for t in range(T1):
            _step(c, h, path_of[t], acts[t])
        if save_kind == "save_state":
            blob = h.s.save_state(scans=scans)
        else:
            blob = h.s.save_envs(subset, scans=scans, device=device)
        sub = blob if save_kind == "save_envs" else h.s.save_envs(subset, scans=scans, device=device)
        rec = []
        for t in range(T1, T1 + T2):
            _step(c, h, path_of[t], acts[t])
            rec.append(_rows(_record(c, h), subset, A, E))
        # (a) the same handle
        if save_kind == "save_state":
            h.s.load_state(blob)
        else:
            h.s.load_envs(blob, np.arange(subset.size), subset)
        for j, t in enumerate(range(T1, T1 + T2)):
            _step(c, h, path_of[t], acts[t])
            k = _diff(_rows(_record(c, h), subset, A, E), rec[j])
            if k:
                return fail("(a) same handle", j, k)
        # (b) a fresh handle, another row cache
        rows_b = int(rng.choice([r for r in (0, 5, 64, 300) if r != rows]))
        hb = _make(c, E, rows_b, env_map, start, params, seeds)
        handles.append(hb)
        for t in range(int(rng.integers(0, 4))):   # a fresh handle that has stepped a little first
            _step(c, hb, path_of[t], acts[-1 - t])
        if save_kind == "save_state":
            hb.s.load_state(blob)
        else:
            hb.s.load_envs(blob, np.arange(subset.size), subset)
        b_rec = []
        for j, t in enumerate(range(T1, T1 + T2)):
            _step(c, hb, path_of[t], acts[t])
            o = _record(c, hb)
            b_rec.append(o)
            k = _diff(_rows(o, subset, A, E), rec[j])
            if k:
                return fail("(b) fresh handle, %d cache rows" % rows_b, j, k)
        # (c) the subset blob into other env indices of a handle with another E
        E2 = int(rng.integers(subset.size, subset.size + 40))
        dst = np.sort(rng.choice(E2, subset.size, replace=False))
        env_map2 = rng.integers(0, c.K, E2) if c.K > 1 else np.zeros(E2, np.int64)
        start2 = bench_start_poses(E2, A, gap_wp=5).reshape(E2, A, 3)
        start2[dst] = start.reshape(E, A, 3)[subset]   # (the re-seat poses are configuration, not env state)
        params2 = [_params(rng) for _ in range(E2 * A)] if c.per_agent else params
        hc = _make(c, E2, int(rng.choice([0, 9, 64])), env_map2, start2.reshape(-1, 3), params2, [int(v) for v in rng.integers(0, 1 << 31, E2 * A)])
        handles.append(hc)
        hc.s.load_envs(sub, np.arange(subset.size), dst)
        for j, t in enumerate(range(T1, T1 + T2)):
            a2 = np.stack([rng.uniform(-0.3, 0.3, E2 * A), rng.uniform(0.5, 6.0, E2 * A)], axis=1).reshape(E2, A, 2)
            a2[dst] = acts[t].reshape(E, A, 2)[subset]
            _step(c, hc, path_of[t], a2.reshape(-1, 2))
            k = _diff(_rows(_record(c, hc), dst, A, E2), rec[j])
            if k:
                return fail("(c) %d envs into E=%d at %s" % (subset.size, E2, dst[:8].tolist()), j, k)
        # clone one env into others, step them all with its actions
        if E > 1:
            src = int(rng.integers(0, E))
            group = np.sort(rng.choice(np.delete(np.arange(E), src), int(rng.integers(1, E)), replace=False))
            st = start.reshape(E, A, 3).copy()
            st[group] = st[src]
            h.d_start.upload(st.reshape(-1, 3))
            h.s.clone_envs(np.full(group.size, src), group)
            for j in range(int(rng.integers(5, 40))):
                a = acts[j % acts.shape[0]].reshape(E, A, 2).copy()
                a[group] = a[src]
                _step(c, h, path_of[j % len(path_of)], a.reshape(-1, 2))
                o = _record(c, h)
                want = _rows(o, [src], A, E)
                for e in group:
                    k = _diff(_rows(o, [e], A, E), want)
                    if k:
                        return fail("clone %d -> %d" % (src, e), j, k)
        # the restored run (b) against the oracle, for envs the run never re-seated (shared-stream noise: NumPy's rows)
        checked = 0
        if c.noise == "shared":
            dt, res, origin = oracle_map_dt("example_map")
            noise = np.random.default_rng(SEED).normal(0., STD, size=(T1 + T2 + 1, c.B))
            sc = np.stack([o["step_count"] for o in b_rec])   # [T2][N]
            for e in subset[:4]:
                ag = np.arange(e * A, e * A + A)
                if not np.array_equal(sc[:, ag], np.repeat(np.arange(T1 + 1, T1 + T2 + 1)[:, None], A, axis=1)):
                    continue   # re-seated somewhere: its episode restarted
                r = orc.SimOracle(1, A, num_beams=c.B, integrator=c.integ)
                r.set_map_dt(dt, res, origin)
                r.set_noise(noise)
                for a in range(A):
                    r.set_params(params[e * A + a] if c.per_agent else params[a], a)
                r.reset(start[ag])
                for t in range(T1 + T2):
                    r.step(acts[t][ag])
                    if max(np.abs(r.state).max(), 0) > 1e6:
                        break
                    if t >= T1:
                        o = b_rec[t - T1]
                        flags = np.array_equal(o["collisions"][ag], r.collisions) and np.array_equal(o["in_collision"][ag], r.in_collision)
                        es, er = rel_err(o["state"][ag], r.state), rel_err(o["scans"][ag], r.scans)
                        if not (flags and es < 1e-9 and er < 1e-9):
                            print("MISMATCH", tag, "oracle env", e, "step", t, "flags", flags, "state", es, "scan", er)
                            return False
                checked += 1
    finally:
        for x in handles:
            x.s.close()
    print("ok", tag, "oracle envs %d" % checked)
    return True


# ------------------------------------------------------------------ the env layers
def _same_tuple(a, b):
    """(obs, reward, done, info) of one F110VecEnv and of a ShardedVecEnv: None or the first key that differs"""
    for name in a[0]:
        if isinstance(a[0][name], np.ndarray) and not np.array_equal(a[0][name], b[0][name], equal_nan=True):
            return "obs " + name
    if not np.array_equal(np.asarray(a[1]), np.asarray(b[1]), equal_nan=True):
        return "reward"
    if not np.array_equal(a[2], b[2]):
        return "done"
    for name in a[3]:
        if not np.array_equal(a[3][name], b[3][name]):
            return "info " + name
    return None


def run_env(seed, verbose=True):
    rng = np.random.default_rng(700000 + seed)
    K = int(rng.integers(1, 6))
    sizes = [int(rng.choice([1, int(rng.integers(1, 5)), int(rng.integers(1, 17))])) for _ in range(K)]
    E = sum(sizes)
    A = int(rng.choice([1, 2, 2, 3]))
    device_logic = bool(rng.random() < 0.5)
    auto_reset = bool(rng.random() < 0.5)
    T = int(rng.integers(20, 60))
    tag = "env seed %d shards %s A%d device_logic %s auto_reset %s T%d" % (seed, sizes, A, device_logic, auto_reset, T)
    kw = dict(map=map_stem("example_map"), map_ext=".png", num_agents=A, track=CSV, reward='progress', device_logic=device_logic,
              auto_reset=auto_reset)
    one = amd.F110VecEnv(E, copy_obs=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=[0] * K, shard_sizes=sizes, **kw)
    bounds = np.concatenate([[0], np.cumsum(sizes)])
    whole_at = int(rng.integers(1, T))   # the step before which a mask covers exactly one whole shard
    snaps = None
    try:
        poses = bench_start_poses(E, A, gap_wp=int(rng.integers(3, 7))).reshape(E, A, 3)
        a, b = one.reset(poses), sh.reset(poses)
        k = _same_tuple(a, b)
        if k:
            print("MISMATCH", tag, "first reset", k)
            return False
        for t in range(T):
            what = "step"
            if t == whole_at or rng.random() < 0.15:
                q = int(rng.integers(0, K))
                if t == whole_at or rng.random() < 0.4:
                    mask = np.zeros(E, bool)
                    mask[bounds[q]:bounds[q + 1]] = True          # exactly shard q
                else:
                    mask = rng.random(E) < 0.3
                what = "reset mask %s" % "".join("1" if m else "0" for m in mask)
                p2 = bench_start_poses(E, A, gap_wp=int(rng.integers(3, 7))).reshape(E, A, 3)
                a, b = one.reset(p2, mask), sh.reset(p2, mask)
            elif snaps is None and rng.random() < 0.1:
                snaps = (one.snapshot(), sh.snapshot(), t)
                continue
            elif snaps is not None and rng.random() < 0.15:
                what = "restore of step %d" % snaps[2]
                a, b = one.restore(snaps[0]), sh.restore(snaps[1])
                snaps = None
                if a is None or b is None:
                    if (a is None) != (b is None):
                        print("MISMATCH", tag, "step", t, what, "one side returned None")
                        return False
                    continue
            else:
                act = np.stack([rng.uniform(-0.4, 0.4, (E, A)), rng.uniform(1.0, 9.0, (E, A))], axis=2)
                a, b = one.step(act), sh.step(act)
            k = _same_tuple(a, b)
            if k:
                print("MISMATCH", tag, "step", t, what, "differs in", k)
                return False
    finally:
        sh.close()
        one.sim.batch.close()
    print("ok", tag)
    return True


if __name__ == "__main__":
    lo, hi = int(sys.argv[1]), int(sys.argv[2])
    fn = run_env if len(sys.argv) > 3 and sys.argv[3] == "env" else run
    bad = [sd for sd in range(lo, hi) if not fn(sd)]
    print("failed seeds:", bad)
