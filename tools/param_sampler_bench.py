#!/usr/bin/env python3
"""What the parameter sampler (f110_param_sampler_*) adds to a step, timed with HIP events (f110_timer_*).

    python tools/param_sampler_bench.py [--steps K] [--warmup W] [--blocks P] [--out FILE]

tools/reset_sampler_bench.py's method, so the two launches can be put next to each other: one handle steps bench.py's workload
shape (32 768 envs of 2 cars on example_map, device noise, the actions of workload.action_sets, step_device back to back) with
the in-step re-seat armed (f110_set_auto_reseat at the bench start poses), in pairs of K-step blocks from one saved state: the
block runs with no sampler, again with the per-agent rows of set_params_batch (the nominal values: what the step's kernels pay for
reading a row per agent instead of one per agent slot), and again with the sampler armed, each from the restored state.  Two cases: one drawn
slot (mu ~ U(0.5, 1.1) per env) and all sixteen (+-10 % of the nominal, uniform and clipped normal alternating, per agent).
Reported per case: the median step time of each mode, the median over the blocks of sampler minus rows (the added microseconds
per step of the draw launch) and of rows minus off, the draws per step, and the time of one explicit draw of every env (f110_param_sample_device).  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def samplers(amd):
    from f1tenth_gym_amd.param_sampler import normal, uniform
    keys = amd._ffi.PARAM_KEYS[:16]
    every = {k: (uniform(0.9, 1.1, relative=True) if i % 2 == 0 else normal(1.0, 0.05, 0.9, 1.1, relative=True)) for i, k in enumerate(keys)}
    return {"one_slot": amd.ParamSampler(7, mu=uniform(0.5, 1.1, scope="env")), "sixteen_slots": amd.ParamSampler(7, **every)}


def run(amd, workload, agents, steps, warmup, blocks, ps):
    A = 2
    E = agents // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    start = workload.bench_start_poses(E, A)
    s.reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    s.set_auto_reseat(d_start, 0)
    sets = workload.action_sets(8, E * A, 1)
    d_act = [s.device_array((E * A, 2)) for _ in sets]
    for d, a in zip(d_act, sets):
        d.upload(a)
    for w in range(300):   # into the steady regime (envs crash and re-seat every step)
        s.step_device(d_act[w % len(d_act)])
    ms = {"off": [], "rows": [], "on": []}
    draws = []
    k = 0
    nominal = np.tile(s.agent_params_rows(), (E, 1))
    for b in range(blocks + 1):
        blob = s.save_state(scans=False)   # (without a sampler: the blob has neither the rows nor the stream column)
        for mode in ("off", "rows", "on"):
            on = mode == "on"
            s.load_state(blob)
            if on:
                s.set_param_sampler(ps)
            elif mode == "rows":
                s.set_params_batch(nominal)
            for w in range(warmup):
                s.step_device(d_act[(k + w) % len(d_act)])
            if on:
                s.param_sampler_stats(clear=True)
            s.timer_begin()
            for t in range(steps):
                s.step_device(d_act[(k + warmup + t) % len(d_act)])
            v = s.timer_end_ms()
            if b > 0:                    # the first pair warms both modes up
                ms[mode].append(v / steps)
                if on:
                    draws.append(s.param_sampler_stats()["draws"] / steps)
            if on:
                s.clear_param_sampler()
            elif mode == "rows":
                s.set_params_batch(None)
        k += warmup + steps
    # one explicit draw of every env
    s.set_param_sampler(ps)
    full = []
    for r in range(6):
        s.timer_begin()
        s.sample_params_device()
        v = s.timer_end_ms()
        if r > 0:
            full.append(1e3 * v)
    s.close()
    off, rows, on = (float(np.median(ms[m])) for m in ("off", "rows", "on"))
    diff = [1e3 * (b - a) for a, b in zip(ms["rows"], ms["on"])]
    rows_diff = [1e3 * (b - a) for a, b in zip(ms["off"], ms["rows"])]
    return {"agents": agents, "drawn_slots": len(ps.drawn), "step_us_off": 1e3 * off, "step_us_rows": 1e3 * rows, "step_us_on": 1e3 * on,
            "added_us": float(np.median(diff)), "added_pct": 100.0 * float(np.median(diff)) / (1e3 * off),
            "rows_added_us": float(np.median(rows_diff)), "draws_per_step": float(np.median(draws)),
            "full_draw_us": float(np.median(full)), "blocks_added_us": diff, "blocks_rows_added_us": rows_diff, "full_draw_runs_us": full}


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
        raise SystemExit("param_sampler_bench: no MI355X visible (HIP events need the GPU; there is no CPU timing)")
    cases = {name: run(amd, workload, args.agents, args.steps, args.warmup, args.blocks, ps) for name, ps in samplers(amd).items()}
    line = json.dumps({"tool": "param_sampler_bench", "steps": args.steps, "cases": cases})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
