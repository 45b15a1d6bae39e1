#!/usr/bin/env python3
"""Scripted opponents: slot 0 of every env is "the learner" (here the built-in scan policy, or pure pursuit on the raceline),
slot 1 drives itself with a follow-the-gap controller on the device and reacts to what its lidar sees.

    scans (HBM) --ego policy--> actions[:, 0]   --follow_gap_device--> actions[:, 1]   --episode_step_device--> scans ...

Nothing crosses PCIe inside the loop.  Prints laps and contacts.

    python examples/scripted_opponents.py [--envs 256] [--steps 3000] [--ego scan|pursuit] [--target center|furthest]

The same through the vector env: F110VecEnv(E, device_logic=True, scripted={1: GapFollower()}) and step(actions) as before; the
rows of slot 1 are ignored and replaced on the device.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import f1tenth_gym_amd as amd  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--ego", choices=("scan", "pursuit"), default="scan")
    ap.add_argument("--target", choices=("center", "furthest"), default="center")
    args = ap.parse_args(argv)
    E, A = args.envs, 2
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    sim.episode_init(0)
    sim.episode_reset(workload.bench_start_poses(E, A))
    actions = sim.device_array((N, 2))
    actions.upload(np.zeros((N, 2)))
    assign = np.tile(np.array([-1, 0], dtype=np.int32), E)          # slot 0: external, slot 1: controller 0
    sim.set_controllers(assign, [amd.GapFollower(target=args.target)])
    d_resets = sim.device_array((1,), np.int32)
    d_resets.upload(np.zeros(1, np.int32))
    if args.ego == "pursuit":
        wp = np.loadtxt(os.path.join(os.path.dirname(amd.__file__), "maps", "example_waypoints.csv"), delimiter=";", skiprows=3)
        d_wp = sim.device_array((len(wp), 3))
        d_wp.upload(np.ascontiguousarray(wp[:, [1, 2, 5]]))

        def ego():
            sim.pure_pursuit_device(d_wp, len(wp), actions, 0.82461887897713965, 0.5, 0.17145 + 0.15875)
    else:
        def ego():
            sim.scan_policy_device(actions, v_hi=4.0)
    sim.episode_step_device(actions)          # the first observation (zero actions)
    contacts = np.zeros(N)
    t0 = time.perf_counter()
    for t in range(args.steps):
        ego()                                 # writes every row ...
        sim.follow_gap_device(actions)        # ... and the controllers overwrite slot 1's
        sim.episode_step_device(actions)
        if t % 100 == 99:                     # a look at the collision flags now and then (the only host reads)
            contacts += sim.get("collisions")["collisions"]
        sim.episode_reset_done_device(d_resets)
    sim.sync()
    dt = time.perf_counter() - t0
    laps = sim.episode_device_views()["lap_counts"].download().reshape(E, A)
    print("%d envs x 2 cars, %d steps, %.3f ms per step: %d env resets; ego (%s) max lap count %.0f, gap follower (%s) max lap count %.0f; "
          "contacts seen at the sampled steps: ego %d, gap follower %d"
          % (E, args.steps, dt / args.steps * 1e3, int(d_resets.download()[0]), args.ego, laps[:, 0].max(), args.target, laps[:, 1].max(),
             int(contacts.reshape(E, A)[:, 0].sum()), int(contacts.reshape(E, A)[:, 1].sum())))
    sim.close()


if __name__ == "__main__":
    main()
