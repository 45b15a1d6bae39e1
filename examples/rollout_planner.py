#!/usr/bin/env python3
"""A sampling planner entirely in device memory: every car rolls a shared library of motion primitives ahead from its live state,
scores them in torch through DLPack and drives the first action of the best one.

    state, FIFO, params (HBM) --rollout_device--> [N][K][2] float32 (alive, progress)
        --torch: progress - w * (steps - alive), argmax--> the winner's first action --step_device--> ...

The library is K = steers x speeds primitives of H actions, each held `--repeat` sim steps: a constant steering angle at a constant
speed.  A primitive that comes closer than `--margin` metres to a wall stops counting steps (alive); the score trades the metres
gained along the raceline against the steps it did not survive.  Nothing crosses PCIe inside the loop and the host never waits.
Prints the progress made and the collisions at the end.

    python examples/rollout_planner.py [--envs 256] [--agents 1] [--steps 2000] [--steers 9] [--speeds 4] [--horizon 8] [--repeat 5]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--agents", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--steers", type=int, default=9)
    ap.add_argument("--speeds", type=int, default=4)
    ap.add_argument("--horizon", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--margin", type=float, default=0.35, help="metres of clearance a primitive must keep")
    ap.add_argument("--weight", type=float, default=0.5, help="metres of progress a step not survived costs")
    args = ap.parse_args(argv)
    import torch                                   # (torch first, then the simulator's library)
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    E, A = args.envs, args.agents
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    csv = os.path.join(os.path.dirname(amd.__file__), "maps", "example_waypoints.csv")
    sim.set_track(amd.Track.from_csv(csv))
    sim.enable_track()
    sim.reset(workload.bench_start_poses(E, A))
    # the library: every steering angle at every speed, held for the whole horizon
    steers, speeds = np.linspace(-0.35, 0.35, args.steers), np.linspace(1.5, 6.0, args.speeds)
    lib = np.array([[[st, v]] * args.horizon for st in steers for v in speeds])          # [K][H][2]
    plan = amd.Rollout(k=len(lib), horizon=args.horizon, repeat=args.repeat, channels=("alive", "progress"), margin=args.margin)   # (the output holds them in this order)
    d_lib = sim.device_array(lib.shape)
    d_lib.upload(lib)
    summary = sim.device_array(plan.shape(N), np.float32)
    actions = sim.device_array((N, 2))
    actions.upload(np.zeros((N, 2)))
    stream = torch.cuda.ExternalStream(sim.device_views()["stream"], device=torch.device("cuda", sim.device_id))
    hits = 0.0
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):                # torch's kernels on the simulator's stream: ordered with its own, no host wait
        first = torch.from_dlpack(d_lib)[:, 0, :]  # float64 [K, 2]: each primitive's first action
        res = torch.from_dlpack(summary)           # float32 [N, K, 2] over the summary's memory
        act = torch.from_dlpack(actions)           # float64 [N, 2] over the action buffer
        for t in range(args.steps):
            sim.rollout_device(plan, d_lib, summary)
            sim.fence()                            # a two-block step's rollout ran on two streams: both in front of torch, the step behind it
            score = res[:, :, 1] - args.weight * (float(plan.steps) - res[:, :, 0])
            act.copy_(first[score.argmax(dim=1)])
            sim.fence()
            sim.step_device(actions)
            if t % 100 == 99:                      # a look at the flags now and then (the only host reads)
                hits += float(sim.get("collisions")["collisions"].sum())
    sim.sync()
    dt = time.perf_counter() - t0
    del first, res, act, score                     # the tensors view the simulator's memory: they go before close()
    trk = sim.get_track()
    print("%d envs x %d cars, K = %d primitives x %d steps ahead, %d steps, %.3f ms per step: mean progress of the last step %.4f m, collisions at the sampled steps: %d"
          % (E, A, plan.k, plan.steps, args.steps, dt / args.steps * 1e3, float(np.mean(trk["ds"])), int(hits)))
    sim.close()


if __name__ == "__main__":
    main()
