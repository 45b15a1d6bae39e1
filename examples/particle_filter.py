#!/usr/bin/env python3
"""Localise, then drive: every car follows the raceline by pure pursuit on its particle filter's ESTIMATE of its pose, never on
the simulator's true pose, entirely in device memory.

    scan, pose delta (HBM) --localize_device--> estimate [N][3] --pure_pursuit_poses_device--> actions [N][2] --step_device--> ...

Each call moves the car's cloud of P particles by the pose's move since the last call plus noise, casts B' rays per particle against
the map's distance table (the scan's own ray march), weights the particles by how well those ranges explain the car's live scan,
and writes the weighted mean pose next to the observation.  The planner reads that estimate where it lies.  Nothing crosses PCIe
inside the loop and the host never waits; every step's info row goes into a history buffer on the device that is read once at
the end.

    python examples/particle_filter.py [--envs 256] [--steps 1000] [--particles 256] [--beams 54]

Prints the mean and the worst distance between estimate and true pose as one JSON line.
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
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--particles", type=int, default=256)
    ap.add_argument("--beams", type=int, default=54)
    ap.add_argument("--vgain", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import DeviceArray, workload
    E, T = args.envs, args.steps
    sim = amd.BatchSim(num_envs=E, num_agents=1)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    wp = np.loadtxt(os.path.join(workload.PKG_MAPS, "example_waypoints.csv"), delimiter=";", skiprows=3)
    d_wp = sim.device_array((len(wp), 3))
    d_wp.upload(np.ascontiguousarray(wp[:, [1, 2, 5]]))
    sim.reset(workload.bench_start_poses(E, 1))
    pf = amd.ParticleFilter(particles=args.particles, n_beams=args.beams, beam_first=0, beam_stride=(sim.B - 1) // max(args.beams - 1, 1),
                            sigma_x=0.03, sigma_y=0.015, sigma_theta=0.01, init_x=0.1, init_y=0.1, init_theta=0.05, sigma_hit=0.1, clip=3.0,
                            squash=float(args.beams) / 6.0, resample_frac=0.5)
    sim.set_particle_filter(pf, seed=args.seed)
    actions = sim.device_array((E, 2))
    actions.upload(np.zeros((E, 2)))
    pose = sim.device_array((E, 3))
    history = sim.device_array((T, E, 4), np.float32)      # every call's info rows, read once at the end
    rows = [DeviceArray(sim, (E, 4), np.float32, ptr=history.ptr + t * E * 16) for t in range(T)]
    sim.localize_device(pose)                              # right after the reset: a fresh cloud per car
    sim.step_device(actions)                               # the first observation
    t0 = time.perf_counter()
    for t in range(T):                                     # observe -> localise -> plan on the estimate -> step, enqueued back to back
        sim.localize_device(pose, rows[t])
        sim.pure_pursuit_poses_device(d_wp, len(wp), pose, actions, 0.82461887897713965, args.vgain, 0.17145 + 0.15875)
        sim.step_device(actions)
    sim.sync()
    dt = time.perf_counter() - t0
    info = history.download()
    o = sim.get("state", "collisions")
    est = pose.download()
    print(json.dumps({"envs": E, "steps": T, "particles": pf.particles, "beams": pf.n_beams, "ms_per_step": dt / max(T, 1) * 1e3,
                      "err_xy_mean": float(info[:, :, 2].mean()), "err_xy_worst": float(info[:, :, 2].max()),
                      "effective_samples_mean": float(info[:, :, 0].mean()), "resampled_share": float(info[:, :, 3].mean()),
                      "speed_mean": float(o["state"][:, 3].mean()), "collisions": int(np.sum(o["collisions"] > 0)),
                      "finite": bool(np.isfinite(info).all() and np.isfinite(est).all() and np.isfinite(o["state"]).all())}))
    sim.close()


if __name__ == "__main__":
    main()
