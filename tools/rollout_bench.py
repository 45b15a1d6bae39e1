#!/usr/bin/env python3
"""What a rollout (f110_rollout_device) costs at N x K x H x repeat = 4096 x 64 x 8 x 3 and 65 536 x 8 x 8 x 3 on
example_map (device noise, the example raceline, a few steps taken first), next to the step's own integration kernel.

    python tools/rollout_bench.py [--blocks 8] [--reps 100] [--warmup 5] [--shapes 4096x64,65536x8] [--out FILE]

HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within one
process and per shape:  shared and per-agent candidate actions, each (a) the summary without the track pass (six channels)
(b) with PROGRESS and END_LAT (c) with them and the trajectory.  Reports median and min .. max of the blocks for each, the
vehicle-steps per second (N * K * H * repeat over the call time) and, from f110_profile_kernels on the unchanged step of the same
handle, k_integrate's agent-steps per second.  The expectation (not a gate): a rollout's rate per vehicle-step is at least
k_integrate's, because its state stays in registers between steps.  Prints one JSON line; --out also writes it to a file.
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


def shape_side(amd, workload, N, K, args):
    A, H, repeat = 2, args.horizon, args.repeat
    E = N // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.set_track(amd.Track(workload.raceline()[:, 1:3]))
    s.reset(workload.bench_start_poses(E, A))
    for acts in workload.action_sets(args.steps, N, 1):
        s.step(acts)
    # the step's integration kernel on this handle: agent-steps per second
    d_act = s.device_array((N, 2))
    d_act.upload(np.tile([0.05, 3.0], (N, 1)))
    blob = s.save_state()
    s.profile_kernels(True)
    for _ in range(args.profile_steps):
        s.step_device(d_act)
    s.sync()
    n, _, dyn_ms, _ = s.profile_read()
    s.profile_kernels(False)
    s.load_state(blob)
    res = {"agents": N, "K": K, "H": H, "repeat": repeat,
           "k_integrate": {"ms": dyn_ms / max(n, 1), "agent_steps_per_s": N / (dyn_ms / max(n, 1) * 1e-3) if n and dyn_ms > 0 else None, "steps": n}}
    rng = np.random.default_rng(1)
    six = ("end_x", "end_y", "end_v", "end_yaw_rate", "alive", "min_clear")
    work = float(N) * K * H * repeat
    calls, keep = {}, []
    for layout in ("shared", "per_agent"):
        shape = ((N,) if layout == "per_agent" else ()) + (K, H)
        cand = np.stack([rng.uniform(-0.3, 0.3, shape), rng.uniform(1.0, 5.0, shape)], axis=-1)
        d_cand = s.device_array(cand.shape)
        d_cand.upload(cand)
        for name, ch, traj in (("summary", six, False), ("track", six + ("progress", "end_lat"), False), ("track_traj", six + ("progress", "end_lat"), True)):
            p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ch, margin=0.3, layout=layout, traj=traj)
            out = s.device_array(p.shape(N), np.float32)
            tr = s.device_array(p.traj_shape(N), np.float32) if traj else None
            keep.append((d_cand, out, tr))
            calls["%s_%s" % (layout, name)] = (lambda p=p, c=d_cand, o=out, t=tr: s.rollout_device(p, c, o, t))
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.blocks):          # alternating blocks: every variant sees the same drift of the machine
        for k, fn in calls.items():
            times[k].append(timed(s, fn, args.reps))
    for k, v in times.items():
        t = np.array(v)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                  "vehicle_steps_per_s": work / (float(np.median(t)) * 1e-3), "blocks": [round(x, 5) for x in t]}
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15, help="steps taken before the measurement")
    ap.add_argument("--profile-steps", type=int, default=50, help="steps of the k_integrate measurement")
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shapes", default="4096x64,65536x8", help="agents x candidates, one shape each")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for shape in (v for v in args.shapes.split(",") if v):
        N, K = (int(q) for q in shape.split("x"))
        res["n%d_k%d" % (N, K)] = shape_side(amd, workload, N, K, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
