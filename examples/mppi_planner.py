#!/usr/bin/env python3
"""MPPI on the device: every car plans its own next action from its live state, entirely in device memory.

    state, FIFO, params, map, track (HBM) --mppi_device--> the action buffer [N][2] --step_device--> ...

Each call draws K noisy action sequences around the car's nominal one (NumPy's PCG64 and ziggurat, a stream per car), rolls them
ahead with the step's own integration, weights them by exp(-cost / lambda) and writes the weighted mean's first action into the
step's action buffer; the rest of the mean is the next call's nominal.  The cost trades the metres gained along the raceline against
the clearance kept and the steps a candidate did not survive.  Nothing crosses PCIe inside the loop and the host never waits.
With --obstacles the cars drive on a slot with random boxes and discs on the racing line: the rollout reads that
slot's distance table, so the planner sees them without being told.

    python examples/mppi_planner.py [--envs 256] [--steps 1000] [--k 64] [--horizon 8] [--repeat 5] [--obstacles 0]

Prints the progress made along the track and the collisions as one JSON line.
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
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=1000, help="less than half a lap, or the progress printed wraps")
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--obstacles", type=int, default=0, help="random obstacles on the racing line (0: the plain track)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    E = args.envs
    sim = amd.BatchSim(num_envs=E, num_agents=1)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    track = amd.Track.from_csv(os.path.join(workload.PKG_MAPS, "example_waypoints.csv"))
    sim.set_track(track)
    if args.obstacles > 0:                         # a slot derived from the track's map, the same raceline on it, every env on it
        obstacles = amd.Obstacles.random_on_track(track, args.obstacles, args.seed, lateral=0.5, min_gap=6.0, length=(0.3, 0.5),
                                                  width=(0.2, 0.4), radius=(0.1, 0.2))
        slot = sim.add_obstacle_map(obstacles)
        sim.set_track(track, slot)
        sim.set_env_maps(np.full(E, slot, dtype=np.int32))
    sim.enable_track()
    sim.reset(workload.bench_start_poses(E, 1))
    planner = amd.Mppi(k=args.k, horizon=args.horizon, repeat=args.repeat, shift=True, margin=0.3, sigma_steer=0.12, sigma_speed=0.8,
                       speed_min=1.0, speed_max=6.0, lam=0.5, w_dead=4.0, w_clear=30.0, w_progress=8.0, w_lat=0.0, clear_ref=0.7, v_init=2.0)
    sim.set_mppi(planner, seed=args.seed)
    actions = sim.device_array((E, 2))
    actions.upload(np.zeros((E, 2)))
    info = sim.device_array((E, 4), np.float32)
    sim.step_device(actions)                       # the observation of the first plan
    s0 = np.array(sim.get_track()["s"], copy=True)
    t0 = time.perf_counter()
    for _ in range(args.steps):                    # observe -> plan -> step, enqueued back to back
        sim.mppi_device(actions, info)
        sim.step_device(actions)
    sim.sync()
    dt = time.perf_counter() - t0
    o = sim.get("state", "collisions")
    trk = sim.get_track()
    progress = np.array([workload_wrap(float(b) - float(a), track.length) for a, b in zip(s0, trk["s"])])
    inf = info.download()
    print(json.dumps({"envs": E, "steps": args.steps, "k": planner.k, "horizon": planner.horizon, "repeat": planner.repeat,
                      "obstacles": args.obstacles, "ms_per_step": dt / max(args.steps, 1) * 1e3, "progress_min": float(progress.min()),
                      "progress_mean": float(progress.mean()), "collisions": int(np.sum(o["collisions"] > 0)),   # cars in collision at the last step
                      "nan": bool(np.isnan(o["state"]).any() or np.isnan(actions.download()).any()),
                      "effective_samples_mean": float(inf[:, 2].mean())}))
    sim.close()


def workload_wrap(g, length):
    """s(end) - s(start) on the closed raceline, for less than half a lap"""
    if g > 0.5 * length:
        g -= length
    elif g <= -0.5 * length:
        g += length
    return g


if __name__ == "__main__":
    main()
