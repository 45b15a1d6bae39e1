#!/usr/bin/env python3
"""Randomised vehicle parameters: every env draws its surface friction mu ~ U(0.5, 1.1) (one value per env: friction belongs to
the track) and every car its mass within +-15 % of the nominal, on the device.  Both cars of every env drive
themselves with the follow-the-gap controller; the progress along the raceline is accumulated on the device.

    reset --sample_params--> rows [N][18] (HBM) ... scans --follow_gap_device--> actions --episode_step_device--> scans, ds ...

The true parameters are read the way a policy or critic would read them as privileged input: params_view() through DLPack
(torch when it is installed, else a host copy), no copy of the rows.  Prints the spread of the progress per friction bin.

    python examples/random_params.py [--envs 1024] [--steps 1500] [--bins 6]

The same through the vector env: F110VecEnv(E, device_logic=True, auto_reset=True, random_params=sampler) draws at reset() and
at every auto re-seat inside the step.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import f1tenth_gym_amd as amd  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402
from f1tenth_gym_amd.param_sampler import uniform  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=1500)
    ap.add_argument("--bins", type=int, default=6)
    args = ap.parse_args(argv)
    E, A = args.envs, 2
    N = E * A
    try:
        import torch
    except ImportError:
        torch = None
    sim = amd.BatchSim(num_envs=E, num_agents=A)
    sim.set_map(workload.map_stem("example_map") + ".yaml", ".png")
    sim.set_noise_rng(12345, 0.01)
    sim.set_track(amd.Track.from_xy(workload.raceline()[:, 1:3]))
    sim.enable_track()
    sampler = amd.ParamSampler(7, mu=uniform(0.5, 1.1, scope="env"), m=uniform(0.85, 1.15, relative=True))
    sim.set_param_sampler(sampler)
    sim.sample_params()                       # the draw in front of the reset
    sim.episode_init(0)
    sim.episode_reset(workload.bench_start_poses(E, A))
    sim.set_controllers(np.zeros(N, dtype=np.int32), [amd.GapFollower()])
    actions = sim.device_array((N, 2))
    actions.upload(np.zeros((N, 2)))
    rows_view, ds_view = sim.params_view(), sim.track_views()["ds"]
    if torch is not None:
        rows, ds = torch.from_dlpack(rows_view), torch.from_dlpack(ds_view)
        progress = torch.zeros_like(ds)
    else:
        progress = np.zeros(N)
    sim.episode_step_device(actions)          # the first observation (zero actions)
    for t in range(args.steps):
        sim.follow_gap_device(actions)
        sim.episode_step_device(actions)
        if torch is not None:
            sim.sync()                        # (this example orders its torch work by waiting on both sides; a training loop would use fence())
            progress += ds
            torch.cuda.synchronize()
        else:
            progress += ds_view.download()
    sim.sync()
    if torch is not None:
        mu, mass, progress = rows[:, 0].cpu().numpy(), rows[:, 6].cpu().numpy(), progress.cpu().numpy()
        del rows, ds                          # the DLPack consumers go before the handle
    else:
        host = rows_view.download()
        mu, mass = host[:, 0], host[:, 6]
    crashed = sim.get("collisions")["collisions"] != 0
    print("%d envs x %d cars, %d steps; parameters through %s" % (E, A, args.steps, "torch.from_dlpack(params_view())" if torch is not None else "a host copy (torch is not installed)"))
    print("mu in [%.3f, %.3f] (one value per env: %s), mass in [%.3f, %.3f] kg" % (mu.min(), mu.max(), bool(np.all(mu[0::2] == mu[1::2])), mass.min(), mass.max()))
    edges = np.linspace(0.5, 1.1, args.bins + 1)
    for lo, hi in zip(edges[:-1], edges[1:]):
        sel = (mu >= lo) & (mu < hi)
        if sel.any():
            p = progress[sel]
            print("mu %.2f .. %.2f: %5d cars, progress mean %7.2f m, std %6.2f, min %7.2f, max %7.2f, crashed %4.1f %%"
                  % (lo, hi, int(sel.sum()), p.mean(), p.std(), p.min(), p.max(), 100.0 * crashed[sel].mean()))
    sim.close()


if __name__ == "__main__":
    main()
