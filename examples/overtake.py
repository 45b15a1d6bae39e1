#!/usr/bin/env python3
"""Overtaking on the device: an MPPI car that sees the car in front.

    scans (HBM) --follow_gap_device--> actions[:, 0]  (the slow car ahead)
    state, map, track, the other car's live state (HBM) --mppi_device--> actions[:, 1]  --step_device--> ...

Every env holds two cars on the example map.  Car 0 follows the gap at a modest speed; car 1 starts ten waypoints behind it and plans
with MPPI.  With the opponent term attached (BatchSim.set_mppi_opponents) the planner predicts car 0 over its horizon, along the
raceline with its lateral offset kept ('track') or at constant velocity ('cv'), and every candidate pays for coming within `radius`
of a prediction and for passing closer than `near_ref`.  With --blind the term is left off and the planner is the map-only one.
Nothing crosses PCIe inside the loop and the host never waits.

    python examples/overtake.py [--envs 64] [--steps 1500] [--mode track|cv] [--blind]

Prints, as one JSON line, the cars' closest approach over the run (sampled every 25 steps into device memory and read at the end),
the cars in collision at the last step and both cars' progress along the track.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--mode", choices=("track", "cv"), default="track")
    ap.add_argument("--blind", action="store_true", help="leave the opponent term off")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    E, A = args.envs, 2
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    track = amd.Track.from_csv(os.path.join(workload.PKG_MAPS, "example_waypoints.csv"))
    sim.set_track(track)
    sim.enable_track()
    sim.reset(workload.bench_start_poses(E, A))        # car 1 starts ten waypoints behind car 0
    assign = np.tile(np.array([0, -1], dtype=np.int32), E)
    sim.set_controllers(assign, [amd.GapFollower(v_lo=1.0, v_hi=2.5, v_turn=1.5)])
    planner = amd.Mppi(k=args.k, horizon=args.horizon, repeat=args.repeat, shift=True, margin=0.3, sigma_steer=0.12, sigma_speed=0.8,
                       speed_min=1.0, speed_max=6.0, lam=0.5, w_dead=4.0, w_clear=30.0, w_progress=8.0, w_lat=0.0, clear_ref=0.7, v_init=2.0)
    sim.set_mppi(planner, np.arange(1, N, 2), seed=args.seed)
    if not args.blind:
        sim.set_mppi_opponents(amd.Opponents(mode=args.mode, radius=0.6, max_range=15.0), w_hit=6.0, w_near=10.0, near_ref=1.0)
    actions = sim.device_array((N, 2))
    actions.upload(np.zeros((N, 2)))
    sim.step_device(actions)                           # the observation of the first plan
    s0 = np.array(sim.get_track()["s"], copy=True)
    nb = amd.Neighbors(k=1, channels=("dist",))        # the gap between the two cars, sampled every 25 steps into device memory
    samples = [sim.device_array((N, 1, 1), np.float32) for _ in range(max(args.steps // 25, 1))]
    t0 = time.perf_counter()
    for t in range(args.steps):                        # observe -> both controllers -> step, enqueued back to back: no host wait
        sim.follow_gap_device(actions)
        sim.mppi_device(actions)
        sim.step_device(actions)
        if t % 25 == 24:
            sim.neighbors_device(nb, samples[t // 25])
    sim.sync()
    dt = time.perf_counter() - t0
    o = sim.get("state", "collisions")
    s1 = sim.get_track()["s"]
    gain = np.array([_wrap(float(b) - float(a), track.length) for a, b in zip(s0, s1)])
    dist = np.array([b.download()[1::2, 0, 0] for b in samples[:max(args.steps // 25, 0)]] or [np.full(E, np.nan)])
    hits = int(np.sum(o["collisions"] > 0))
    print(json.dumps({"envs": E, "steps": args.steps, "mode": "blind" if args.blind else args.mode, "ms_per_step": dt / max(args.steps, 1) * 1e3,
                      "closest_approach_min": float(np.nanmin(dist)), "closest_approach_mean": float(np.nanmean(np.nanmin(dist, axis=0))),
                      "in_collision_at_the_end": hits,"planner_progress_mean": float(gain[1::2].mean()), "leader_progress_mean": float(gain[0::2].mean()),
                      "nan": bool(np.isnan(o["state"]).any() or np.isnan(actions.download()).any())}))
    sim.close()


def _wrap(g, length):
    if g > 0.5 * length:
        g -= length
    elif g <= -0.5 * length:
        g += length
    return g


if __name__ == "__main__":
    main()
