#!/usr/bin/env python3
"""What the follow-the-gap controllers (f110_follow_gap_device) cost, on bench.py's workload (envs of 2 cars on
example_map, 1080 beams, device noise, workload.action_sets, a few steps taken first).

    python tools/gap_follower_bench.py [--blocks 8] [--reps 200] [--warmup 20] [--vec-steps 200] [--sizes 65536,4096] [--skip-host] [--out FILE]

Kernel side, HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks
within one process:  (a) the controller call  (b) f110_scan_policy_device, which reads the same scans and is the yardstick
(8 B + 16 = 8656 bytes per agent at 1080 beams).  Cases: every agent scripted, one slot of two scripted, and 4096 agents.
The expectation (not a gate): case <= policy * (bytes the case moves / bytes the policy moves) + the spread of the policy's own
block times, i.e. the case's bytes priced at the rate the existing kernel achieves.  A scripted agent moves 8 W + 4 + 4 + 16 bytes
(window, assignment, step_count, action), an external one its 4-byte assignment.
Host side: F110VecEnv(device_logic=True, auto_reset=True) steps per second (host wall clock, every step ends in its wait) at 2048
and 32 768 envs with and without scripted={1: GapFollower()}.
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

LEAN = ("poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "collisions")


def timed(sim, fn, reps):
    sim.sync()
    sim.timer_begin()
    for _ in range(reps):
        fn()
    return sim.timer_end_ms() / reps


def kernel_side(amd, workload, agents, cases, args):
    A = 2
    E = agents // A
    res = {"agents": E * A}
    sims = {}
    calls = {}
    g = amd.GapFollower()
    for name, assign in [("policy", None)] + [(k, v(E)) for k, v in cases.items()]:
        s = amd.BatchSim(num_envs=E, num_agents=A)     # one handle per case: each has its own assignment armed
        s.set_map_image(*workload.load_map_image("example_map"))
        s.set_noise_rng(12345, 0.01)
        s.reset(workload.bench_start_poses(E, A))
        for acts in workload.action_sets(5, E * A, 1):
            s.step(acts)
        d_act = s.device_array((E * A, 2))
        d_act.upload(np.zeros((E * A, 2)))
        sims[name] = s
        B = s.B
        if assign is None:
            res.update(beams=B, policy_bytes_per_agent=8 * B + 16)
            calls[name] = (lambda s=s, d=d_act: s.scan_policy_device(d))
        else:
            s.set_controllers(assign, [g])
            lo, hi = g.window(B)
            n_scr = int(np.sum(assign >= 0))
            res[name] = {"scripted": n_scr, "window": hi - lo,
                         "bytes_per_agent": (n_scr * (8 * (hi - lo) + 24) + (E * A - n_scr) * 4) / float(E * A)}
            calls[name] = (lambda s=s, d=d_act: s.follow_gap_device(d))
    for fn in calls.values():
        for _ in range(args.warmup):
            fn()
    times = {k: [] for k in calls}
    for _ in range(args.blocks):          # alternating blocks: every case sees the same drift of the box
        for k, fn in calls.items():
            times[k].append(timed(sims[k], fn, args.reps))
    pol = np.array(times["policy"])
    res["policy_ms"] = {"median": float(np.median(pol)), "min": float(pol.min()), "max": float(pol.max()), "blocks": [round(v, 5) for v in pol]}
    res["policy_gbps"] = res["agents"] * res["policy_bytes_per_agent"] / np.median(pol) / 1e6
    for name in cases:
        t = np.array(times[name])
        r = res[name]
        ratio = r["bytes_per_agent"] / res["policy_bytes_per_agent"]
        r.update(median_ms=float(np.median(t)), min_ms=float(t.min()), max_ms=float(t.max()), blocks=[round(v, 5) for v in t],
                 gbps=res["agents"] * r["bytes_per_agent"] / float(np.median(t)) / 1e6, byte_ratio=ratio,
                 expected_ms=float(np.median(pol)) * ratio + float(pol.max() - pol.min()))
        r["meets_expectation"] = bool(r["median_ms"] <= r["expected_ms"])
    for s in sims.values():
        s.close()
    return res


def host_side(amd, workload, E, steps, warmup):
    A = 2
    out = {}
    forms = {"scripted": dict(scripted={1: amd.GapFollower()}), "plain": {}}
    acts = [a.reshape(E, A, 2) for a in workload.action_sets(4, E * A, 1)]
    envs = {k: amd.F110VecEnv(E, auto_reset=True, device_logic=True, map=workload.map_stem("example_map"), map_ext=".png",
                              episode_fields=(), obs_fields=LEAN, **kw) for k, kw in forms.items()}
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
    cases = {"all_scripted": lambda E: np.zeros(2 * E, dtype=np.int32),
             "one_slot": lambda E: np.tile(np.array([-1, 0], dtype=np.int32), E)}
    res = {"reps": args.reps, "warmup": args.warmup, "blocks": args.blocks, "build": _ffi.lib().f110_build_info().decode()}
    for n in (int(v) for v in args.sizes.split(",") if v):
        res["agents_%d" % n] = kernel_side(amd, workload, n, cases if n >= 65536 else {"all_scripted": cases["all_scripted"]}, args)
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
