#!/usr/bin/env python3
"""What a localisation call (f110_pf_device) costs at M x P x B' = 4096 x 256 x 54 and 65 536 x 64 x 54 on example_map
(device noise, a few steps taken first, every agent armed), next to the step's own scan kernel at the same agent count.

    python tools/pf_bench.py [--blocks 4] [--reps 100] [--warmup 5] [--shapes 4096x256x54,65536x64x54] [--out FILE]

HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within one process
and per shape: the filter, and the yardstick — `reps` device steps with the scan kernel's own event pair switched on
(f110_profile_kernels), whose scan time per step over N x num_beams rays is the step's ray rate in the same session.  The filter is
armed afresh with the same seed before each of its blocks (outside the timed region): the simulator does not step inside a block,
so the clouds would otherwise diffuse from block to block and the rays would be other rays.

Reports median and min .. max of the blocks for each, the rays per second of a whole call (M P B' over the call's time) and of the
step's scan kernel, and their ratio.  k_pf_sense's own share of a call comes from a kernel trace of this tool with --blocks 1
--reps 20 in a run of its own.  Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shape_side(amd, workload, M, P, Bp, args):
    A = 2
    E = M // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.reset(workload.bench_start_poses(E, A))
    acts = workload.action_sets(args.steps, M, 1)
    for a in acts:
        s.step(a)
    pf = amd.ParticleFilter(particles=P, n_beams=Bp, beam_first=0, beam_stride=(s.B - 1) // max(Bp - 1, 1), resample_frac=0.5)
    d_pose, d_info, d_act = s.device_array((M, 3)), s.device_array((M, 4), np.float32), s.device_array((M, 2))
    d_act.upload(np.ascontiguousarray(acts[-1]))
    res = {"agents": M, "P": P, "beams": Bp, "num_beams": s.B}

    def arm():
        s.set_particle_filter(pf, None, seed=3)
        for _ in range(args.warmup):
            s.localize_device(d_pose, d_info)

    def time_filter():
        arm()
        s.sync()
        s.timer_begin()
        for _ in range(args.reps):
            s.localize_device(d_pose, d_info)
        return s.timer_end_ms() / args.reps

    def time_scan():
        for _ in range(args.warmup):
            s.step_device(d_act)
        s.sync()
        s.profile_kernels(True)
        for _ in range(args.reps):
            s.step_device(d_act)
        s.sync()
        n, scan_ms, _, _ = s.profile_read()
        s.profile_kernels(False)
        return scan_ms / max(n, 1)

    times = {"pf_call": [], "step_scan": []}
    for _ in range(args.blocks):           # alternating blocks: both see the same drift of the machine
        times["pf_call"].append(time_filter())
        times["step_scan"].append(time_scan())
    rays = {"pf_call": float(M) * P * Bp, "step_scan": float(M) * s.B}
    for k, v in times.items():
        t = np.array(v)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                  "rays_per_s": rays[k] / (float(np.median(t)) * 1e-3), "blocks": [round(x, 5) for x in t]}
    res["call_rate_over_scan_rate"] = res["pf_call"]["rays_per_s"] / res["step_scan"]["rays_per_s"]
    info = d_info.download()
    res["err_xy_mean"], res["effective_samples_mean"] = float(info[:, 2].mean()), float(info[:, 0].mean())
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=4)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15, help="steps taken before the measurement")
    ap.add_argument("--shapes", default="4096x256x54,65536x64x54", help="agents x particles x beams, one shape each")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for shape in (v for v in args.shapes.split(",") if v):
        M, P, Bp = (int(q) for q in shape.split("x"))
        res["m%d_p%d_b%d" % (M, P, Bp)] = shape_side(amd, workload, M, P, Bp, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
