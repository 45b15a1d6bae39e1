#!/usr/bin/env python3
"""Track preview: every car steers towards a station of its raceline preview and takes the raceline's speed there, with the
preview, the steering rule (torch, through DLPack) and the step all in device memory.

    s, pose (HBM) --track_preview_device--> [N][P][3] float32 --torch: pure-pursuit-like rule--> actions --episode_step_device--> ...

The example raceline's vx column is attribute 0 of the track.  Nothing crosses PCIe inside the loop.  Prints laps and collisions.

    python examples/track_preview.py [--envs 256] [--steps 3000] [--station 3] [--vgain 0.5]

The same through the vector env: F110VecEnv(E, device_logic=True, track=track, track_preview=TrackPreview(...)) adds
obs['track_preview'], float32 [E][A][P][D].
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
    ap.add_argument("--steps", type=int, default=3000)
    ap.add_argument("--station", type=int, default=3, help="which of the 8 stations (0.5 m apart, the first 0.5 m ahead) to steer at")
    ap.add_argument("--vgain", type=float, default=0.5)
    args = ap.parse_args(argv)
    import torch                                   # (torch first, then the simulator's library)
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    E, A = args.envs, 1
    N = E * A
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    csv = os.path.join(os.path.dirname(amd.__file__), "maps", "example_waypoints.csv")
    sim.set_track(amd.Track.from_csv(csv, attrs={"vx": 5}))
    sim.enable_track()
    sim.episode_init(0)
    sim.episode_reset(workload.bench_start_poses(E, A))
    preview = amd.TrackPreview(points=8, offset=0.5, spacing=0.5, channels=("x", "y", "attr0"), frame="ego")
    buf = sim.device_array(preview.shape(N), np.float32)
    actions = sim.device_array((N, 2))
    actions.upload(np.zeros((N, 2)))
    d_resets = sim.device_array((1,), np.int32)
    d_resets.upload(np.zeros(1, np.int32))
    stream = torch.cuda.ExternalStream(sim.device_views()["stream"], device=torch.device("cuda", sim.device_id))
    wheelbase = 0.17145 + 0.15875
    sim.episode_step_device(actions)               # the first observation (zero actions)
    hits = 0.0
    t0 = time.perf_counter()
    with torch.cuda.stream(stream):                # torch's kernels on the simulator's stream: ordered with its own, no host wait
        pv = torch.from_dlpack(buf)                # float32 [N, 8, 3] over the preview's memory
        act = torch.from_dlpack(actions)           # float64 [N, 2] over the action buffer
        for t in range(args.steps):
            sim.track_preview_device(preview, buf)
            look = pv[:, args.station]
            d2 = look[:, 0] ** 2 + look[:, 1] ** 2
            act[:, 0] = torch.atan(2.0 * wheelbase * look[:, 1] / d2).clamp(-0.4189, 0.4189).double()
            act[:, 1] = look[:, 2].double() * args.vgain
            sim.episode_step_device(actions)
            if t % 100 == 99:                      # a look at the collision flags now and then (the only host reads)
                hits += float(sim.get("collisions")["collisions"].sum())
            sim.episode_reset_done_device(d_resets)
    sim.sync()
    dt = time.perf_counter() - t0
    del pv, act, look, d2                          # the tensors view the simulator's memory: they go before close()
    laps = sim.episode_device_views()["lap_counts"].download()
    print("%d cars, %d steps, %.3f ms per step: max lap count %.0f, %d env resets, collisions seen at the sampled steps: %d"
          % (E, args.steps, dt / args.steps * 1e3, laps.max(), int(d_resets.download()[0]), int(hits)))
    sim.close()


if __name__ == "__main__":
    main()
