#!/usr/bin/env python3
"""What the line followers (f110_follow_line_device) cost: envs of A cars on example_map with its raceline as the
track, 1080 beams, device noise, workload.action_sets, a few steps taken first.

    python tools/line_follower_bench.py [--blocks 6] [--reps 200] [--warmup 20] [--vec-steps 200] [--skip-host] [--out FILE]

Kernel side, HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within
one process: f110_follow_line_device with every agent armed, at 4096 and 65 536 agents, A = 2 and 16 cars per env, with the
car-ahead term (follow_range = 6) and without it (follow_range = 0); the median of the blocks' means, their least and greatest.
Host side: F110VecEnv(device_logic=True, auto_reset=True) milliseconds per step (host wall clock, every step ends in its wait) at
2048 envs of 2 cars with scripted={1: LineFollower()}, with scripted={1: GapFollower()} and without scripted cars, in alternating
rounds.
Prints one line per case and --out writes them to a file (profiles/line_follower_bench.txt), the sources' hash first.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEAN = ("poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions")


def timed(sim, fn, reps):
    sim.sync()
    sim.timer_begin()
    for _ in range(reps):
        fn()
    return sim.timer_end_ms() / reps


def kernel_side(amd, workload, track, args):
    sims, calls, names = {}, {}, []
    for agents in (4096, 65536):
        for A in (2, 16):
            for follow in (True, False):
                E = agents // A
                s = amd.BatchSim(num_envs=E, num_agents=A)
                s.set_map_image(*workload.load_map_image("example_map"))
                s.set_noise_rng(12345, 0.01)
                s.set_track(track)
                s.enable_track()
                s.reset(workload.bench_start_poses(E, A))
                for acts in workload.action_sets(5, E * A, 1):
                    s.step(acts)
                s.set_line_followers(np.zeros(E * A, dtype=np.int32), [amd.LineFollower(follow_range=6.0 if follow else 0.0)])
                d_act = s.device_array((E * A, 2))
                d_act.upload(np.zeros((E * A, 2)))
                name = "follow_line_device  agents %6d  A %2d  car-ahead %s" % (agents, A, "on " if follow else "off")
                names.append(name)
                sims[name] = s
                calls[name] = (lambda s=s, d=d_act: s.follow_line_device(d))
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.blocks):          # alternating blocks: every case sees the same drift of the box
        for k, fn in calls.items():
            times[k].append(timed(sims[k], fn, args.reps))
    for s in sims.values():
        s.close()
    return ["%s  median %.2f us  (blocks %.2f .. %.2f us)" % (k, 1e3 * np.median(times[k]), 1e3 * min(times[k]), 1e3 * max(times[k])) for k in names]


def host_side(amd, workload, track, E, steps, warmup):
    A = 2
    forms = {"line followers": dict(scripted={1: amd.LineFollower()}), "gap followers": dict(scripted={1: amd.GapFollower()}), "no scripted cars": {}}
    acts = [a.reshape(E, A, 2) for a in workload.action_sets(4, E * A, 1)]
    envs = {k: amd.F110VecEnv(E, auto_reset=True, device_logic=True, map=workload.map_stem("example_map"), map_ext=".png", track=track,
                              episode_fields=(), obs_fields=LEAN, **kw) for k, kw in forms.items()}
    for env in envs.values():
        env.reset(workload.bench_start_poses(E, A).reshape(E, A, 3))
        for t in range(warmup):
            env.step(acts[t % 4])
    rounds = {k: [] for k in envs}
    for _ in range(3):                     # alternating rounds
        for k, env in envs.items():
            t0 = time.perf_counter()
            for t in range(steps):
                env.step(acts[(t // 20) % 4])
            rounds[k].append((time.perf_counter() - t0) * 1e3 / steps)
    for env in envs.values():
        env.sim.batch.close()
    return ["scripted step  %d envs x %d cars  %-16s  median %.4f ms per step  (rounds %s)" % (E, A, k, np.median(v), ", ".join("%.4f" % x for x in v))
            for k, v in rounds.items()]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--vec-steps", type=int, default=200)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, build, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    w = workload.raceline()
    track = amd.Track(w[:, 1:3], closed=True, attrs=np.column_stack([w[:, 4], w[:, 5]]))
    lines = ["sources %s  %s  reps %d  warmup %d  blocks %d" % (build.src_hash(), _ffi.lib().f110_build_info().decode(), args.reps, args.warmup, args.blocks)]
    lines += kernel_side(amd, workload, track, args)
    if not args.skip_host:
        lines += host_side(amd, workload, track, 2048, args.vec_steps, 20)
    print("\n".join(lines))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
