#!/usr/bin/env python3
"""What the neighbour observation (f110_neighbors_device) costs at 65 536 agents, as 32 768 x 2, 16 384 x 4, 2048 x 32
and 256 x 256 cars per env on example_map (device noise, the example raceline, a few steps taken first).

    python tools/neighbors_bench.py [--blocks 8] [--reps 200] [--warmup 20] [--agents 65536] [--cars 2,4,32,256] [--out FILE]

HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within one
process and per shape:  (a) K = 1 with four channels (dx, dy, dist, valid)  (b) K = 8 with all ten  (c) f110_track_preview_device
with P = 8 and four channels on the same handle, the yardstick: a per-agent kernel with the same kind of output.  The expectation
(not a gate): at 2 and 4 cars per env a neighbour call costs about what the preview costs; the 256-car shape shows what the
all-pairs walk costs.  Reports median and min .. max of the blocks for each.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(sim, fn, reps):
    sim.sync()
    sim.timer_begin()
    for _ in range(reps):
        fn()
    return sim.timer_end_ms() / reps


def shape_side(amd, workload, agents, A, args):
    E = agents // A
    N = E * A
    w = workload.raceline()
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(amd.Track(w[:, 1:3], attrs={"kappa": w[:, 4], "vx": w[:, 5]}))
    s.enable_track()
    s.reset(workload.bench_start_poses(E, A, gap_wp=max(1, min(10, 780 // A))))   # (an env's cars fit on the raceline's 783 points)
    for acts in workload.action_sets(args.steps, N, 1):
        s.step(acts)
    small = amd.Neighbors(k=1, channels=("dx", "dy", "dist", "valid"))
    big = amd.Neighbors(k=8, channels=amd.neighbors.CHANNELS)
    pv = amd.TrackPreview(points=8, channels=("x", "y", "attr0", "attr1"))
    bufs = {p: s.device_array(p.shape(N), np.float32) for p in (small, big, pv)}
    calls = {"preview_p8_d4": lambda: s.track_preview_device(pv, bufs[pv]),
             "neighbors_k1_d4": lambda: s.neighbors_device(small, bufs[small]),
             "neighbors_k8_d10": lambda: s.neighbors_device(big, bufs[big])}
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.blocks):          # alternating blocks: every kernel sees the same drift of the machine
        for k, fn in calls.items():
            times[k].append(timed(s, fn, args.reps))
    res = {"envs": E, "cars": A, "agents": N}
    for k, v in times.items():
        t = np.array(v)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "blocks": [round(x, 5) for x in t]}
    for k in ("neighbors_k1_d4", "neighbors_k8_d10"):
        res[k]["over_preview"] = round(res[k]["median_ms"] / res["preview_p8_d4"]["median_ms"], 3)
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=3, help="steps taken before the measurement")
    ap.add_argument("--agents", type=int, default=65536)
    ap.add_argument("--cars", default="2,4,32,256", help="cars per env, one shape each (a kernel trace wants one per run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for A in (int(v) for v in args.cars.split(",") if v):
        res["cars_%d" % A] = shape_side(amd, workload, args.agents, A, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
