#!/usr/bin/env python3
"""What the opponent term (f110_mppi_set_opponents) adds to a planning call: f110_mppi_device with the term attached
against the same handle's detached call, at the shapes of profiles/mppi_bench.txt (M x K x H x repeat = 4096 x 64 x 8 x 3 and
65 536 x 8 x 8 x 3, every agent armed, track weights 0) with A = 2 and A = 4 cars per env, in both modes.

    python tools/opponents_bench.py [--blocks 6] [--reps 100] [--warmup 5] [--shapes 4096x64,65536x8] [--agents 2,4] [--out FILE]

HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within one process:
detached, cv, track, detached, ...  Before every block the planner is armed afresh with the same seed and the term attached (or not)
outside the timed region; the simulator does not step, so every block starts from the same planner state and the same opponents.
The term adds one k_opp_predict launch (16 lanes per agent and opponent) and (A - 1) * H distance samples per candidate to
H * repeat integrations of about 1900 instructions each, so the expectation (not a gate) is a ratio close to 1.

Reports the median and min .. max of the blocks for each variant and the ratios of the medians.  Prints one JSON line; --out also
writes it to a file.
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


def shape_side(amd, workload, N, K, A, args):
    H, repeat = args.horizon, args.repeat
    E = N // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(amd.Track(workload.raceline()[:, 1:3]))
    s.reset(workload.bench_start_poses(E, A))
    for acts in workload.action_sets(args.steps, E * A, 1):
        s.step(acts)
    d_act, d_info = s.device_array((E * A, 2)), s.device_array((E * A, 4), np.float32)
    planner = amd.Mppi(k=K, horizon=H, repeat=repeat, margin=0.3, w_progress=0.0, w_lat=0.0)
    variants = {"detached": None, "cv": amd.Opponents(mode="cv", radius=0.6, max_range=10.0),
                "track": amd.Opponents(mode="track", radius=0.6, max_range=10.0)}
    times = {k: [] for k in variants}
    for _ in range(args.blocks):               # alternating blocks: every variant sees the same drift of the machine
        for name, op in variants.items():
            s.set_mppi(planner, None, seed=3)  # (outside the timed region)
            if op is not None:
                s.set_mppi_opponents(op, 5.0, 2.0, 1.5)
            for _ in range(args.warmup):
                s.mppi_device(d_act, d_info)
            times[name].append(timed(s, lambda: s.mppi_device(d_act, d_info), args.reps))
    res = {"agents": E * A, "cars_per_env": A, "K": K, "H": H, "repeat": repeat}
    for k, v in times.items():
        t = np.array(v)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "blocks": [round(x, 5) for x in t]}
    res["ratio_cv"] = res["cv"]["median_ms"] / res["detached"]["median_ms"]
    res["ratio_track"] = res["track"]["median_ms"] / res["detached"]["median_ms"]
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15, help="steps taken before the measurement")
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", default="4096x64,65536x8", help="agents x candidates, one shape each")
    ap.add_argument("--agents", default="2,4", help="cars per env")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for shape in (v for v in args.shapes.split(",") if v):
        N, K = (int(q) for q in shape.split("x"))
        for A in (int(v) for v in args.agents.split(",") if v):
            res["n%d_k%d_a%d" % (N, K, A)] = shape_side(amd, workload, N, K, A, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
