#!/usr/bin/env python3
"""What an observation encode (f110_obs_encode_device) costs, on bench.py's workload (envs of 2 cars on example_map,
1080 beams, device noise, workload.action_sets, a few steps taken first).

    python tools/obs_encoder_bench.py [--blocks 8] [--reps 200] [--warmup 20] [--vec-steps 200] [--sizes 65536,4096] [--skip-host] [--out FILE]

Kernel side, HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks
within one process:  (a) the encode call  (b) f110_scan_policy_device, which reads the same scans and is the yardstick.
The expectation (not a gate): encode <= policy * (8 W + 4 D (2F - 1)) / (8 B + 16) + the spread of the policy's own block times,
i.e. the extra bytes priced at the rate the existing kernel achieves.  Headline: 65 536 agents, K = 108, MIN, five features,
F = 4; also 4096 agents, F = 1 and K = 1080.
Host side: F110VecEnv(device_logic=True, auto_reset=True) steps per second (host wall clock, every step ends in its wait) at
2048 and 32 768 envs with obs['encoded'], with 'scans' in obs_fields, and with neither.
Prints one JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIVE = ("vx", "steer", "yaw_rate", "slip", "collision")
LEAN = ("poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions")


def timed(sim, fn, reps):
    sim.sync()
    sim.timer_begin()
    for _ in range(reps):
        fn()
    return sim.timer_end_ms() / reps


def kernel_side(amd, workload, agents, variants, args):
    A = 2
    E = agents // A
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*workload.load_map_image("example_map"))
    s.set_noise_rng(12345, 0.01)
    s.reset(workload.bench_start_poses(E, A))
    for acts in workload.action_sets(5, E * A, 1):
        s.step(acts)
    d_act = s.device_array((E * A, 2))
    B = s.B
    res = {"agents": E * A, "beams": B, "policy_bytes_per_agent": 8 * B + 16}
    calls = {"policy": lambda: s.scan_policy_device(d_act)}
    for name, kw in variants.items():
        enc = amd.ObsEncoder(features=FIVE, range_clip=30.0, range_scale=30.0, **kw)
        out = s.encode_obs_device(enc)
        calls[name] = (lambda enc=enc, out=out: s.encode_obs_device(enc, out))
        W, D, F = B, enc.dim, enc.frames
        res[name] = {"D": D, "F": F, "bytes_per_agent": 8 * W + 4 * D * (2 * F - 1)}
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.blocks):          # alternating blocks: every variant sees the same drift of the box
        for k, fn in calls.items():
            times[k].append(timed(s, fn, args.reps))
    pol = np.array(times["policy"])
    res["policy_ms"] = {"median": float(np.median(pol)), "min": float(pol.min()), "max": float(pol.max()), "blocks": [round(v, 5) for v in pol]}
    res["policy_gbps"] = res["agents"] * res["policy_bytes_per_agent"] / np.median(pol) / 1e6
    for name in variants:
        t = np.array(times[name])
        r = res[name]
        ratio = r["bytes_per_agent"] / res["policy_bytes_per_agent"]
        r.update(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), blocks=[round(v, 5) for v in t],
                 gbps=res["agents"] * r["bytes_per_agent"] / float(np.median(t)) / 1e6, byte_ratio=ratio,
                 expected_ms=float(np.median(pol)) * ratio + float(pol.max() - pol.min()))
        r["meets_expectation"] = bool(r["median_ms"] <= r["expected_ms"])
    s.close()
    return res


def host_side(amd, workload, E, steps, warmup):
    A = 2
    out = {}
    enc = dict(sectors=108, pool="min", features=FIVE, frames=4, range_clip=30.0, range_scale=30.0)
    forms = {"encoded": dict(obs_encoder=enc, obs_fields=LEAN + ("encoded",)), "scans": dict(obs_fields=LEAN + ("scans",)),
             "neither": dict(obs_fields=LEAN)}
    acts = [a.reshape(E, A, 2) for a in workload.action_sets(4, E * A, 1)]
    envs = {k: amd.F110VecEnv(E, auto_reset=True, device_logic=True, map=workload.map_stem("example_map"), map_ext=".png",
                              episode_fields=(), **kw) for k, kw in forms.items()}
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
    for k, v in rounds.items():
        out[k + "_ms_per_step"] = {"median": float(np.median(v)), "rounds": [round(x, 4) for x in v]}
    for env in envs.values():
        env.sim.batch.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--vec-steps", type=int, default=200)
    ap.add_argument("--skip-host", action="store_true")
    ap.add_argument("--sizes", default="65536,4096", help="agent counts of the kernel side (a kernel trace wants one size per run)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import _ffi, workload
    if _ffi.device_count() < 1:
        raise SystemExit("no GPU visible: nothing to measure (there is no CPU fallback)")
    variants = {"k108_min_f4": dict(sectors=108, pool="min", frames=4), "k108_min_f1": dict(sectors=108, pool="min", frames=1),
                "k108_mean_f4": dict(sectors=108, pool="mean", frames=4), "k1080_center_f1": dict(sectors=1080, pool="center", frames=1)}
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for n in (int(v) for v in args.sizes.split(",") if v):
        res["agents_%d" % n] = kernel_side(amd, workload, n, variants if n >= 65536 else {"k108_min_f4": variants["k108_min_f4"]}, args)
    if not args.skip_host:
        res["vec_env_2048"] = host_side(amd, workload, 2048, args.vec_steps, 20)
        res["vec_env_32768"] = host_side(amd, workload, 32768, max(20, args.vec_steps // 4), 5)
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
