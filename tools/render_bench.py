#!/usr/bin/env python3
"""What a render (f110_render_device) costs, on bench.py's workload (envs of 2 cars on example_map with the example
raceline, device noise, workload.action_sets, a few steps taken first).

    python tools/render_bench.py [--reps R] [--warmup W] [--out FILE]

(a) F110Env.render('rgb_array') end to end: the 1000 x 800 RGB frame, its download included (host wall clock, the call
    synchronises);  (b) 64 FOLLOW frames of 256 x 256 with RGB, every layer;  (c) 64 x 64 EGO class crops of all 65 536 agents,
    every layer.  (b) and (c) are timed with HIP events on the handle's stream around R back-to-back renders into reused
    buffers, after W warm-up renders.  Prints one JSON line (milliseconds per render); --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(sim, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    sim.sync()
    sim.timer_begin()
    for _ in range(reps):
        fn()
    return sim.timer_end_ms() / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--agents", type=int, default=65536)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload

    res = {"reps": args.reps, "warmup": args.warmup}
    # (a) the gym frame
    env = amd.F110Env(map=workload.map_stem("example_map"), map_ext=".png", num_agents=2, track=workload.raceline()[:, 1:3])
    env.reset(workload.bench_start_poses(1, 2))
    for _ in range(5):
        env.step(np.array([[0.0, 3.0], [0.0, 3.0]]))
    for _ in range(args.warmup):
        env.render('rgb_array')
    t0 = time.perf_counter()
    for _ in range(args.reps):
        frame = env.render('rgb_array')
    res["env_rgb_array_ms"] = (time.perf_counter() - t0) * 1e3 / args.reps
    assert frame.shape == (800, 1000, 3)
    env.sim.batch.close()

    # (b), (c) on bench.py's workload
    A = 2
    E = args.agents // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(workload.raceline()[:, 1:3])
    s.reset(workload.bench_start_poses(E, A))
    for acts in workload.action_sets(5, E * A, 1):
        s.step(acts)
    s.sync()
    agents = np.arange(64) * (E * A // 64)
    out_b = s.render_device(agents, width=256, height=256, view="follow", m_per_px=0.05, layers="all", rgb=True)
    res["follow_64x256x256_rgb_ms"] = timed(s, lambda: s.render_device(agents, width=256, height=256, view="follow", m_per_px=0.05,
                                                                       layers="all", rgb=True, out=out_b), args.reps, args.warmup)
    out_c = s.render_device(None, width=64, height=64, view="ego", m_per_px=0.05, layers="all")
    res["ego_crops_all_agents_64x64_ms"] = timed(s, lambda: s.render_device(None, width=64, height=64, view="ego", m_per_px=0.05,
                                                                            layers="all", out=out_c), args.reps, args.warmup)
    out_m = s.render_device(None, width=64, height=64, view="ego", m_per_px=0.05, layers=("map", "cars"))
    res["ego_crops_all_agents_64x64_map_cars_ms"] = timed(s, lambda: s.render_device(None, width=64, height=64, view="ego",
                                                                                      m_per_px=0.05, layers=("map", "cars"), out=out_m),
                                                          args.reps, args.warmup)
    res["agents"] = E * A
    s.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
