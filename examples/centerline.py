"""A track without a csv: F110VecEnv(track='centerline') extracts berlin's centreline loop from the map's distance table on the
device, and everything that needs a Track — here the progress reward and randomised starts — runs on it.

    python examples/centerline.py [--map berlin] [--envs 256] [--steps 300]

Prints the extracted line, then the summed progress reward of a slow random policy started at random poses along it.
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
    ap.add_argument("--map", default="berlin")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=300)
    args = ap.parse_args()
    env = F110VecEnv(args.envs, auto_reset=True, device_logic=True, map=workload.map_stem(args.map), map_ext=".png", num_agents=1,
                     track='centerline', centerline=dict(seed=(0.0, 0.0), spacing=0.2, smooth=1.0), reward='progress',
                     random_start=ResetSampler(seed=3, lateral=0.1, heading=0.05), obs_fields=("poses_x", "poses_y", "progress", "lateral_offset"))
    track = env.tracks[0]
    hw, kappa = track.attrs[:, 0], track.attrs[:, 1]
    print("%s: %r, half width %.2f .. %.2f m, |kappa| up to %.2f 1/m" % (args.map, track, hw.min(), hw.max(), np.abs(kappa).max()))
    obs, _, _, _ = env.reset()            # no poses: every env draws its own on the extracted line
    hist, _ = np.histogram(obs["progress"][:, 0], bins=8, range=(0.0, track.length))
    print("starts over the line (8 bins of %.1f m): %s" % (track.length / 8, hist.tolist()))
    rng = np.random.default_rng(0)
    total, episodes = np.zeros(args.envs), 0
    for _ in range(args.steps):
        acts = np.stack([rng.uniform(-0.05, 0.05, (args.envs, 1)), rng.uniform(1.0, 2.5, (args.envs, 1))], axis=2)
        obs, reward, done, _ = env.step(acts)
        total += reward
        episodes += int(done.sum())
    print("%d envs x %d steps: mean progress %.2f m (%.2f m/s), largest |lateral offset| now %.2f m, %d episodes re-seated"
          % (args.envs, args.steps, total.mean(), total.mean() / (args.steps * env.timestep), np.abs(obs["lateral_offset"]).max(), episodes))
    env.sim.batch.close()


if __name__ == "__main__":
    main()
