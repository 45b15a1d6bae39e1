"""Randomised parity fuzzing of track progress (k_track_project: head, post-step and unit forms) against the oracle's
nearest_on_trajectory.  Per seed: 1..300 envs of 1..4 agents on 1..3 map slots with a random env_map (slot changes inside the
16-agent workgroups), one track per slot (the shipped raceline, wiggly loops of 3 .. 5000 segments on both sides of the 1024-segment
LDS limit, polylines with segment lengths from 1 mm to 50 m, hairpins, self-crossing figure-eights), and a step entry point drawn per
step (step, step_device, step_host fused or not; the one-launch k_step_tiny step where it applies).  Between steps, events that leave
the pruning seed (the agent's last winning segment) stale: set_state teleports, masked resets, reset_collided_device re-seats,
save_envs / load_envs, clone_envs, set_track on a slot mid-run, enable_track(False) / (True).
At every step, for every agent: segment, s and lateral bit-equal to the oracle on the device's own post-step pose, heading_error to
1e-12, ds bit-equal to s(post) - s(pre) wrapped as on the device; on a sample of agents the winner is also held against an
extended-precision search over every segment (within 1e-9 m of the true minimum).
1 200 seeds (0 .. 1199) run by hand on one MI355X without a mismatch.
    python tools/debug/fuzz_track.py 0 40      # seeds 0..39
"""
import os
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from _util import check_track_winner, load_map_image, raceline, track_oracle
import f1tenth_gym_amd as amd

LDS_SEGS = 1024          # kTrackLdsSegs
WIGGLY = [3, 5, 15, 16, 17, 1023, 1024, 1025, 2048, 5000]
PATHS = ["step", "step_device", "step_host", "step_host_no_fuse"]


def wiggly_loop(n, rng):
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    r = 10.0 + rng.uniform(0.2, 1.5) * np.sin(int(rng.integers(2, 9)) * a) + 0.3 * np.cos(13 * a)
    return np.column_stack([r * np.cos(a), r * np.sin(a)])


def mixed_polyline(rng, n):
    ln = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n))
    ang = np.cumsum(rng.uniform(-2.0, 2.0, n))
    xy = np.vstack([[0.0, 0.0], np.cumsum(np.column_stack([ln * np.cos(ang), ln * np.sin(ang)]), axis=0)])
    return xy - xy.mean(axis=0)


def hairpin(rng, n):
    """two parallel straights 0.2 .. 1 m apart joined by a half circle: points of one leg are near-ties with the other"""
    w, L = rng.uniform(0.2, 1.0), rng.uniform(5.0, 30.0)
    m = max(n // 3, 2)
    leg = np.linspace(0.0, L, m, endpoint=False)
    a = np.linspace(-np.pi / 2, np.pi / 2, m, endpoint=False)
    turn = np.column_stack([L + 0.5 * w * np.cos(a), 0.5 * w * np.sin(a)])
    return np.vstack([np.column_stack([leg, np.full(m, -0.5 * w)]), turn, np.column_stack([L - leg, np.full(m, 0.5 * w)])])


def figure_eight(rng, n):
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    s = rng.uniform(4.0, 15.0)
    return np.column_stack([s * np.sin(a), s * np.sin(a) * np.cos(a)])


def draw_track(rng, kind):
    if kind == "raceline":
        return amd.Track.from_xy(raceline()[:, 1:3], closed=bool(rng.random() < 0.8))
    if kind == "big":
        return amd.Track.from_xy(wiggly_loop(int(rng.choice([1025, 2048, 5000])), rng))
    if kind == "small":
        return amd.Track.from_xy(wiggly_loop(int(rng.choice([3, 5, 15, 16, 17, 300, 1023, 1024])), rng))
    if kind == "wiggly":
        return amd.Track.from_xy(wiggly_loop(int(rng.choice(WIGGLY)), rng))
    if kind == "mixed":
        closed = bool(rng.random() < 0.5)
        xy = mixed_polyline(rng, int(rng.integers(2, 1500)))
        return amd.Track.from_xy(xy[:-1] if closed and xy.shape[0] > 3 else xy, closed=closed and xy.shape[0] > 3)
    if kind == "hairpin":
        return amd.Track.from_xy(hairpin(rng, int(rng.integers(6, 1200))), closed=bool(rng.random() < 0.3))
    return amd.Track.from_xy(figure_eight(rng, int(rng.choice([16, 17, 400, 1024, 1025, 3000]))))


def start_on(t, rng, n, jitter=0.0):
    k = rng.integers(0, t.num_segments, n)
    pts = t.points_closed()
    d = pts[k + 1] - pts[k]
    w = rng.uniform(0.0, 1.0, (n, 1))
    xy = pts[k] + w * d + rng.normal(0.0, jitter, (n, 2)) if jitter else pts[k]
    return np.column_stack([xy, np.arctan2(d[:, 1], d[:, 0])])


def run(seed, verbose=True, sample=48):
    rng = np.random.default_rng(300000 + seed)
    E = int(rng.choice([int(rng.integers(1, 5)), int(rng.integers(1, 40)), int(rng.integers(1, 301))]))
    A = int(rng.integers(1, 5))
    K = int(rng.integers(1, 4))
    if seed % 4 == 0:   # every chunk of seeds: one slot past the LDS limit next to one within it (staged / not staged first agents)
        K = max(K, 2)
        kinds = ["big", "small"] if rng.random() < 0.5 else ["small", "big"]
        kinds += [str(rng.choice(["raceline", "wiggly", "mixed", "hairpin", "eight"])) for _ in range(K - 2)]
    else:
        kinds = [str(rng.choice(["raceline", "wiggly", "wiggly", "mixed", "hairpin", "eight"])) for _ in range(K)]
    tracks = [draw_track(rng, kd) for kd in kinds]
    u = rng.random()
    if u < 0.4:
        env_map = rng.integers(0, K, E)
    elif u < 0.8:   # runs of 1..9 envs: slot changes at random places inside the workgroups
        env_map = np.repeat(rng.integers(0, K, E), rng.integers(1, 10, E))[:E]
    else:
        env_map = (np.arange(E) * K) // E
    T = int(rng.integers(6, 18))
    tag = "seed %d E%d A%d slots %s env_map %s T%d" % (seed, E, A, ",".join("%s:%d%s" % (kd, t.num_segments, "c" if t.closed else "o")
                                                                            for kd, t in zip(kinds, tracks)),
                                                     "".join(str(int(m)) for m in env_map[:48]), T)
    N = E * A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    img = load_map_image("example_map")
    s.set_map_image(*img)
    for k in range(1, K):
        s.add_map_image(*img)
    s.set_noise_rng(seed, 0.01)
    if K > 1:
        s.set_env_maps(env_map)
    else:
        env_map = np.zeros(E, dtype=np.int64)
    env_map = np.array(env_map, dtype=np.int64)
    for k, t in enumerate(tracks):
        s.set_track(t, k)
    s.enable_track()
    slot = np.repeat(env_map, A)
    on = True

    def starts():
        p = np.empty((N, 3))
        for k in range(K):
            m = slot == k
            if m.any():
                p[m] = start_on(tracks[k], rng, int(m.sum()), jitter=float(rng.choice([0.0, 0.05, 2.0])))
        return p

    start = starts()
    s.reset(start)
    d_act = s.device_array((N, 2))
    d_start = s.device_array((N, 3)); d_start.upload(start)
    d_cnt = s.device_array((1,), np.int32); d_cnt.upload(np.zeros(1, np.int32))
    hb = s.host_block(("state", "agent_poses"))
    events = []
    try:
        for step in range(T):
            # ---- an event between steps (each one leaves the seed of some agents stale)
            ev = str(rng.choice(["none", "none", "teleport", "reset", "reseat", "load", "clone", "set_track", "toggle"]))
            if ev == "teleport":
                st = s.get("state")["state"].copy()
                seg = s.get_track()["segment"].astype(np.int64)
                who = np.nonzero(rng.random(N) < 0.5)[0]
                for i in who:
                    t = tracks[slot[i]]
                    pts = t.points_closed()
                    if rng.random() < 0.5 and on:   # the point of the track farthest along it from the last winner
                        j = (min(max(seg[i], 0), t.num_segments - 1) + t.num_segments // 2) % t.num_segments
                        st[i, 0:2] = 0.5 * (pts[j] + pts[j + 1])
                    else:
                        j = int(rng.integers(0, t.num_segments))
                        st[i, 0:2] = pts[j] + rng.normal(0.0, float(rng.choice([1e-9, 0.3, 5.0])), 2)
                s.set_state(st)
            elif ev == "reset":
                mask = (rng.random(E) < 0.4).astype(np.uint8)
                s.reset(starts(), mask)
            elif ev == "reseat":
                s.reset_collided_device(d_start, int(rng.integers(0, A)), d_cnt)
            elif ev == "load":
                src = rng.choice(E, int(rng.integers(1, E + 1)), replace=False)
                blob = s.save_envs(src, scans=bool(rng.random() < 0.3), device=bool(rng.random() < 0.5))
                dst = rng.choice(E, src.size, replace=False)
                s.load_envs(blob, np.arange(src.size), dst)
                env_map[dst] = env_map[src]          # (a blob of a multi-slot handle carries each env's slot)
                ev += " %d" % src.size
            elif ev == "clone" and E > 1:
                src = int(rng.integers(0, E))
                dst = rng.choice(np.delete(np.arange(E), src), int(rng.integers(1, E)), replace=False)
                s.clone_envs(np.full(dst.size, src), dst)
                env_map[dst] = env_map[src]
            elif ev == "set_track":
                k = int(rng.integers(0, K))
                tracks[k] = draw_track(rng, str(rng.choice(["raceline", "wiggly", "big", "small", "mixed", "hairpin", "eight"])))
                s.set_track(tracks[k], k)
                ev += " %d:%d" % (k, tracks[k].num_segments)
            elif ev == "toggle":
                on = not on
                s.enable_track(on)
            events.append(ev)
            slot = np.repeat(env_map, A)
            # ---- the step
            path = str(rng.choice(PATHS))
            act = np.stack([rng.uniform(-0.4, 0.4, N), rng.uniform(0.5, 9.0, N)], axis=1)
            pre = s.get("state")["state"][:, [0, 1, 4]]
            if path == "step":
                s.step(act)
            elif path == "step_device":
                d_act.upload(act)
                s.step_device(d_act)
            else:
                s.step_host(hb, act, fuse=path != "step_host_no_fuse")
            if not on:
                continue
            tr = s.get_track()
            post = s.get("agent_poses")["agent_poses"]
            for k in range(K):
                rows = np.nonzero(slot == k)[0]
                if rows.size == 0:
                    continue
                t = tracks[k]
                want = track_oracle(t, post[rows])
                got = np.column_stack([tr["s"][rows], tr["lateral"][rows], tr["heading_error"][rows], tr["segment"][rows]])
                ds = t.wrap_ds(want[:, 0] - track_oracle(t, pre[rows])[:, 0])
                dh = np.abs(np.mod(got[:, 2] - want[:, 2] + np.pi, 2 * np.pi) - np.pi)
                bad = ~((got[:, 3] == want[:, 3]) & (got[:, 0] == want[:, 0]) & (got[:, 1] == want[:, 1])
                        & (dh <= 1e-12 * np.maximum(1.0, np.abs(want[:, 2]))) & (tr["ds"][rows] == ds))
                msg = None
                if bad.any():
                    r = int(np.nonzero(bad)[0][0])
                    i = int(rows[r])
                    msg = "agent %d (env %d slot %d): got seg %d s %r lat %r herr %r ds %r, oracle seg %d s %r lat %r herr %r ds %r; pose %r pre %r" % (
                        i, i // A, k, got[r, 3], got[r, 0], got[r, 1], got[r, 2], tr["ds"][i], want[r, 3], want[r, 0], want[r, 1],
                        want[r, 2], ds[r], post[i].tolist(), pre[i].tolist())
                else:
                    pick = rows if rows.size <= sample else rng.choice(rows, sample, replace=False)
                    msg = check_track_winner(t, post[pick], tr["segment"][pick])
                if msg is not None:
                    print("MISMATCH", tag, "step %d path %s events %s:" % (step, path, events), msg)
                    return False
            events.append(path)
    finally:
        s.close()
    print("ok", tag, "events", ",".join(e for e in events if e not in PATHS))
    return True


if __name__ == "__main__":
    a, b = int(sys.argv[1]), int(sys.argv[2])
    bad = [sd for sd in range(a, b) if not run(sd)]
    print("failed seeds:", bad)
