#!/usr/bin/env python3
"""What the start-pose sampler (f110_reset_sampler_*) adds to a step, timed with HIP events (f110_timer_*).

    python tools/reset_sampler_bench.py [--steps K] [--warmup W] [--blocks P] [--out FILE]

One handle steps bench.py's workload shape (32 768 envs of 2 cars on example_map, device noise, the actions of
workload.action_sets, step_device back to back) with the in-step re-seat armed (f110_set_auto_reseat at the bench start
poses), in pairs of K-step blocks from one saved state: the block runs with no sampler, the state is restored, the sampler is
armed and the same block runs again.  Reported: the median step time of each mode, the median over the pairs of the difference
(the added microseconds per step), the draws per step, and the time of one explicit draw of every env
(f110_reset_sample_device).  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(amd, workload, agents, steps, warmup, blocks):
    A = 2
    E = agents // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(amd.Track.from_xy(workload.raceline()[:, 1:3]))
    start = workload.bench_start_poses(E, A)
    s.reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    s.set_auto_reseat(d_start, 0)
    sets = workload.action_sets(8, E * A, 1)
    d_act = [s.device_array((E * A, 2)) for _ in sets]
    for d, a in zip(d_act, sets):
        d.upload(a)
    rs = amd.ResetSampler(7, lateral=0.3, heading=0.2)
    for w in range(300):   # into the steady regime (envs crash and re-seat every step)
        s.step_device(d_act[w % len(d_act)])
    ms = {False: [], True: []}
    draws = []
    k = 0
    for b in range(blocks + 1):
        blob = s.save_state(scans=False)   # (without a sampler: the blob has no sampler column)
        for on in (False, True):
            s.load_state(blob)
            if on:
                s.set_reset_sampler(rs)
            for w in range(warmup):
                s.step_device(d_act[(k + w) % len(d_act)])
            if on:
                s.reset_sampler_stats(clear=True)
            s.timer_begin()
            for t in range(steps):
                s.step_device(d_act[(k + warmup + t) % len(d_act)])
            v = s.timer_end_ms()
            if b > 0:                    # the first pair warms both modes up
                ms[on].append(v / steps)
                if on:
                    draws.append(s.reset_sampler_stats()["draws"] / steps)
            if on:
                s.clear_reset_sampler()
        k += warmup + steps
    # one explicit draw of every env
    s.set_reset_sampler(rs)
    full = []
    for r in range(6):
        s.timer_begin()
        s.sample_reset_device()
        v = s.timer_end_ms()
        if r > 0:
            full.append(1e3 * v)
    s.close()
    off, on = float(np.median(ms[False])), float(np.median(ms[True]))
    diff = [1e3 * (b - a) for a, b in zip(ms[False], ms[True])]
    return {"agents": agents, "step_us_off": 1e3 * off, "step_us_on": 1e3 * on, "added_us": float(np.median(diff)),
            "added_pct": 100.0 * float(np.median(diff)) / (1e3 * off), "draws_per_step": float(np.median(draws)),
            "full_draw_us": float(np.median(full)), "pairs_added_us": diff, "full_draw_runs_us": full}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--agents", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    if amd._ffi.device_count() < 1:
        raise SystemExit("reset_sampler_bench: no MI355X visible (HIP events need the GPU; there is no CPU timing)")
    res = run(amd, workload, args.agents, args.steps, args.warmup, args.blocks)
    line = json.dumps({"tool": "reset_sampler_bench", "steps": args.steps, "case": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
