#!/usr/bin/env python3
"""What the track preview (f110_track_preview_device) costs, on bench.py's workload (envs of 2 cars on example_map,
1080 beams, device noise, workload.action_sets, a few steps taken first), the example raceline with 2 attributes (kappa, vx).

    python tools/track_preview_bench.py [--blocks 8] [--reps 200] [--warmup 20] [--sizes 65536,4096] [--out FILE]

HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within one
process:  (a) the preview with P = 8 and 4 channels  (b) the preview with P = 32 and 8 channels  (c) f110_pure_pursuit_device on
the same raceline, the existing per-agent waypoint kernel and the yardstick: it scans every waypoint where the preview searches
logarithmically, so the expectation (not a gate) is that a preview takes no longer than it at the same N.  Reports median and
min .. max of the blocks for each and met / missed.  Prints one JSON line; --out also writes it to a file.
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


def kernel_side(amd, workload, agents, args):
    A = 2
    E = agents // A
    N = E * A
    w = workload.raceline()
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(amd.Track(w[:, 1:3], attrs={"kappa": w[:, 4], "vx": w[:, 5]}))
    s.enable_track()
    s.reset(workload.bench_start_poses(E, A))
    for acts in workload.action_sets(5, N, 1):
        s.step(acts)
    d_act = s.device_array((N, 2))
    d_act.upload(np.zeros((N, 2)))
    d_wp = s.device_array((len(w), 3))
    d_wp.upload(np.ascontiguousarray(w[:, [1, 2, 5]]))
    small = amd.TrackPreview(points=8, channels=("x", "y", "attr0", "attr1"))
    big = amd.TrackPreview(points=32, spacing=0.25, channels=("x", "y", "tan_x", "tan_y", "attr0", "attr1"), frame="ego")
    # (the track carries 2 attributes: the 8-channel case of a 4-attribute track is measured with the 6 channels it has)
    if args.four_attrs:
        s.set_track_attrs(0, np.column_stack([w[:-1, 4], w[:-1, 5], np.cos(w[:-1, 3]), np.sin(w[:-1, 3])]))
        big = amd.TrackPreview(points=32, spacing=0.25, channels=amd.track_preview.CHANNELS, frame="ego")
    bufs = {p: s.device_array(p.shape(N), np.float32) for p in (small, big)}
    calls = {"pure_pursuit": lambda: s.pure_pursuit_device(d_wp, len(w), d_act, 0.82461887897713965, 0.5, 0.17145 + 0.15875),
             "preview_p8_d4": lambda: s.track_preview_device(small, bufs[small]),
             "preview_p32_d%d" % big.dim: lambda: s.track_preview_device(big, bufs[big])}
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.blocks):          # alternating blocks: every kernel sees the same drift of the machine
        for k, fn in calls.items():
            times[k].append(timed(s, fn, args.reps))
    res = {"agents": N, "segments": 782}
    pp = np.array(times["pure_pursuit"])
    for k, v in times.items():
        t = np.array(v)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()), "blocks": [round(x, 5) for x in t]}
        if k != "pure_pursuit":
            res[k]["meets_expectation"] = bool(np.median(t) <= np.median(pp))
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sizes", default="65536,4096", help="agent counts (a kernel trace wants one size per run)")
    ap.add_argument("--two-attrs", dest="four_attrs", action="store_false", help="keep the track at 2 attributes: the big preview then has 6 channels")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for n in (int(v) for v in args.sizes.split(",") if v):
        res["agents_%d" % n] = kernel_side(amd, workload, n, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
