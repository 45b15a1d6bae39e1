"""Randomised start poses: F110VecEnv(random_start=...) draws every env's start poses on the example raceline, at reset() and at
every auto re-seat, on the device.  A crash-prone random policy shows where the episodes start.

    python examples/random_starts.py [--envs 1024] [--steps 400]

Prints how many episodes started, how many draws fell back, and a histogram of the starts over the track's length.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from f1tenth_gym_amd import F110VecEnv, ResetSampler  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=400)
    args = ap.parse_args()
    csv = os.path.join(workload.PKG_MAPS, "example_waypoints.csv")
    sampler = ResetSampler(seed=7, gap=1.5, lateral=0.3, heading=0.15)
    env = F110VecEnv(args.envs, auto_reset=True, device_logic=True, map=workload.map_stem("example_map"), map_ext=".png",
                     track=csv, random_start=sampler, obs_fields=("poses_x", "poses_y", "progress"))
    obs, _, _, _ = env.reset()            # no poses: every env draws its own
    starts = [obs["progress"][:, 0].copy()]
    rng = np.random.default_rng(0)
    episodes = 0
    for _ in range(args.steps):
        acts = np.stack([rng.uniform(-0.4, 0.4, (args.envs, 2)), rng.uniform(3.0, 8.0, (args.envs, 2))], axis=2)
        obs, _, done, _ = env.step(acts)
        episodes += int(done.sum())       # a finished env is re-seated at a fresh draw inside the step
    stats = env.sim.batch.reset_sampler_stats()
    L = env.tracks[0].length
    hist, _ = np.histogram(starts[0], bins=10, range=(0.0, L))
    print("%d envs, %d steps: %d episodes ended and were re-seated at fresh draws" % (args.envs, args.steps, episodes))
    print("draws %d, fallbacks %d" % (stats["draws"], stats["fallbacks"]))
    print("first starts over the track (10 bins of %.1f m): %s" % (L / 10, hist.tolist()))
    env.sim.batch.close()


if __name__ == "__main__":
    main()
