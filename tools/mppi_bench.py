#!/usr/bin/env python3
"""What a planning call (f110_mppi_device) costs at M x K x H x repeat = 4096 x 64 x 8 x 3 and 65 536 x 8 x 8 x 3 on
example_map (device noise, the example raceline, a few steps taken first, every agent armed), next to the rollout it is built on.

    python tools/mppi_bench.py [--blocks 8] [--reps 100] [--warmup 5] [--shapes 4096x64,65536x8] [--out FILE]

HIP events on the handle's stream around `reps` back-to-back calls, after `warmup` calls, in alternating blocks within one
process and per shape:  the planner without and with the track weights, and the yardstick, f110_rollout_device with PER_AGENT
candidates and the same channels (ALIVE, MIN_CLEAR; with PROGRESS and END_LAT) on the same handle: what a caller had before, who
then still had to draw the candidates and do the update elsewhere.

The yardstick rolls the planner's OWN candidates, because a dead candidate skips its integration and other candidates would be
other work: in every block the planner is armed afresh with the same seed (outside the timed region; the simulator does not
step, so the block starts from the same planner state every time) and called `warmup` times; the candidates V of its next call —
a function of the stored nominal, the streams and the spec alone — are computed once with the unit form and uploaded as the
rollout's actions.  The planner's later calls of a block draw around the nominal as it moves on, which the yardstick cannot follow;
`alive_first` and `alive_last` report the mean share of H * repeat steps survived by the candidates of the first timed call and of
the call after the last one, so that a drift of the rollout work inside a block is visible.

Reports median and min .. max of the blocks for each and the ratio planner / rollout of the medians.  The expectation (not a
gate): the ratio is close to 1 — a lane adds 2 H draws and the update 2 H K multiply-adds per agent to ~1900 H repeat instructions
of rollout per lane.  Prints one JSON line; --out also writes it to a file.  (The split by kernel comes from a kernel trace of this
tool with --blocks 1 --reps 20.)
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
    res = {"agents": N, "K": K, "H": H, "repeat": repeat}
    d_act, d_info = s.device_array((N, 2)), s.device_array((N, 4), np.float32)
    planners = {"mppi": amd.Mppi(k=K, horizon=H, repeat=repeat, margin=0.3, w_progress=0.0, w_lat=0.0),
                "mppi_track": amd.Mppi(k=K, horizon=H, repeat=repeat, margin=0.3, w_progress=8.0, w_lat=0.5)}
    yardstick = {"mppi": ("rollout", ("alive", "min_clear")), "mppi_track": ("rollout_track", ("alive", "min_clear", "progress", "end_lat"))}
    rows = np.zeros((N, 10))               # V does not depend on the start rows: any rows on the map do for the unit form
    rows[:, [0, 1, 4]] = workload.bench_start_poses(E, A)

    def arm(name):
        """the planner `name` as every one of its blocks starts: armed afresh, `warmup` calls made"""
        s.set_mppi(planners[name], None, seed=3)
        for _ in range(args.warmup):
            s.mppi_device(d_act, d_info)

    def next_candidates(name):
        """V of the armed planner's next call, as a device array"""
        nom, words = s.get_mppi_state()
        cand = s.mppi_rows(planners[name], rows, nom, words, fresh=np.ones(N, dtype=np.int32))["candidates"]
        d = s.device_array(cand.shape)
        d.upload(cand)
        return d

    def alive_share(name, d_cand):
        p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=("alive",), margin=0.3, layout="per_agent", frame="map")
        out = s.rollout_device(p, d_cand)
        share = float(out.download().mean()) / (H * repeat)
        out.free()
        return share

    calls, keep = {}, [d_act, d_info]
    for name in planners:                  # the yardsticks' candidates, once: every block of the planner starts from this state
        arm(name)
        d_cand = next_candidates(name)
        res.setdefault("alive_first", {})[name] = alive_share(name, d_cand)
        roll_name, ch = yardstick[name]
        p = amd.Rollout(k=K, horizon=H, repeat=repeat, channels=ch, margin=0.3, layout="per_agent", frame="map")
        out = s.device_array(p.shape(N), np.float32)
        keep += [d_cand, out]
        calls[roll_name] = (None, lambda p=p, c=d_cand, o=out: s.rollout_device(p, c, o))
        calls[name] = (name, lambda: s.mppi_device(d_act, d_info))
    times = {k: [] for k in calls}
    for b in range(args.blocks):           # alternating blocks: every variant sees the same drift of the machine
        for k, (planner, fn) in calls.items():
            if planner is not None:
                arm(planner)               # (outside the timed region, whatever --warmup is)
            else:
                for _ in range(args.warmup):
                    fn()
            times[k].append(timed(s, fn, args.reps))
            if planner is not None and b == args.blocks - 1:
                d_last = next_candidates(planner)
                res.setdefault("alive_last", {})[planner] = alive_share(planner, d_last)
                d_last.free()
    work = float(N) * K * H * repeat
    for k, v in times.items():
        t = np.array(v)
        res[k] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max()),
                  "vehicle_steps_per_s": work / (float(np.median(t)) * 1e-3), "blocks": [round(x, 5) for x in t]}
    res["ratio"] = res["mppi"]["median_ms"] / res["rollout"]["median_ms"]
    res["ratio_track"] = res["mppi_track"]["median_ms"] / res["rollout_track"]["median_ms"]
    s.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=15, help="steps taken before the measurement")
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
