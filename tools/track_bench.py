#!/usr/bin/env python3
"""What track progress (f110_track_*) adds to a step, timed with HIP events (f110_timer_*).

    python tools/track_bench.py [--steps K] [--warmup W] [--out FILE]

For each case one handle steps bench.py's workload shape (envs of 2 cars on example_map, device noise, the actions of
workload.action_sets, step_device back to back) in pairs of K-step blocks: the state is saved, the block runs with tracking
off, the state is restored and the same block runs with tracking on.  Reported: the median step time of each mode and the
median over the pairs of the difference, the added microseconds per step.  Cases: the
783-row example raceline (782 segments) at 4096 and 65 536 agents, and a 5000-point track (streamed from global / L2, the
LDS holds 1024 segments) at 65 536 agents.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wiggly_loop(n):
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    r = 10.0 + 0.7 * np.sin(7 * a) + 0.3 * np.cos(13 * a)
    return np.column_stack([r * np.cos(a), r * np.sin(a)])


def run_case(amd, workload, agents, track, steps, warmup, blocks):
    A = 2
    E = agents // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(track)
    s.reset(workload.bench_start_poses(E, A))
    sets = workload.action_sets(8, E * A, 1)
    d_act = [s.device_array((E * A, 2)) for _ in sets]
    for d, a in zip(d_act, sets):
        d.upload(a)
    ms = {False: [], True: []}
    k = 0
    for b in range(blocks + 1):
        # a pair of blocks from the same saved state with the same actions: off and on time the very same steps
        blob = s.save_state(scans=False)
        for on in (False, True):
            s.load_state(blob)
            s.enable_track(on)
            for w in range(warmup):
                s.step_device(d_act[(k + w) % len(d_act)])
            s.timer_begin()
            for t in range(steps):
                s.step_device(d_act[(k + warmup + t) % len(d_act)])
            if b > 0:                    # the first pair warms both modes up
                ms[on].append(s.timer_end_ms() / steps)
            else:
                s.timer_end_ms()
        k += warmup + steps
    s.close()
    off, on = float(np.median(ms[False])), float(np.median(ms[True]))
    diff = [1e3 * (b - a) for a, b in zip(ms[False], ms[True])]
    return {"agents": agents, "segments": int(track.num_segments), "step_us_off": 1e3 * off, "step_us_on": 1e3 * on,
            "added_us": float(np.median(diff)), "added_pct": 100.0 * float(np.median(diff)) / (1e3 * off),
            "pairs_added_us": diff, "blocks_us_off": [1e3 * v for v in ms[False]], "blocks_us_on": [1e3 * v for v in ms[True]]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    if amd._ffi.device_count() < 1:
        raise SystemExit("track_bench: no MI355X visible (HIP events need the GPU; there is no CPU timing)")
    rl = amd.Track.from_xy(workload.raceline()[:, 1:3])
    big = amd.Track.from_xy(wiggly_loop(5000))
    cases = [(4096, rl), (65536, rl), (65536, big)]
    res = [run_case(amd, workload, n, t, args.steps, args.warmup, args.blocks) for n, t in cases]
    line = json.dumps({"tool": "track_bench", "steps": args.steps, "cases": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
