"""Obstacle avoidance: follow-the-gap cars on the example track with boxes and discs on the racing line.

Eight map slots are derived from the track's map, each with its own random obstacles stamped into its distance table on the
device; every env runs on one of them.  Every few hundred steps the obstacles of all eight slots are drawn again and stamped in
place (F110VecEnv.set_obstacles): no image edit, no upload of a map, no new table.  Random starts are on: the sampler's clearance
test reads the slot's table, so no car starts inside an obstacle.

    python examples/obstacles.py [--envs 256] [--steps 2000] [--redraw 500] [--obstacles 10]

Prints the collisions per lap driven.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from f1tenth_gym_amd import F110VecEnv, GapFollower, Obstacles, ResetSampler, Track  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402

SLOTS = 8


def draw(track, n, seed):
    return Obstacles.random_on_track(track, n, seed, lateral=0.5, min_gap=6.0, length=(0.3, 0.5), width=(0.2, 0.4), radius=(0.1, 0.2))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--redraw", type=int, default=500, help="steps between two draws of the obstacles")
    ap.add_argument("--obstacles", type=int, default=10, help="obstacles per slot")
    args = ap.parse_args()
    E = args.envs
    track = Track.from_csv(os.path.join(workload.PKG_MAPS, "example_waypoints.csv"))
    env = F110VecEnv(E, auto_reset=True, device_logic=True, num_agents=1, map=workload.map_stem("example_map"), map_ext=".png",
                     track=track, random_start=ResetSampler(seed=7, lateral=0.2, heading=0.1), scripted={0: GapFollower()},
                     obstacle_maps=[draw(track, args.obstacles, k) for k in range(SLOTS)], env_map=1 + np.arange(E) % SLOTS,
                     obs_fields=("collisions", "progress_delta"))
    env.reset()                                   # no poses: every env draws its own, clear of its slot's obstacles
    actions = np.zeros((E, 1, 2))                 # the scripted car's rows are replaced on the device
    crashes, metres, draws = 0, 0.0, 1
    for t in range(args.steps):
        if t and t % args.redraw == 0:            # new obstacles on every slot, in place, behind the step in flight
            for k in range(SLOTS):
                env.set_obstacles(1 + k, draw(track, args.obstacles, draws * SLOTS + k))
            draws += 1
        obs, _, done, _ = env.step(actions)
        crashes += int(np.sum(done & (obs["collisions"][:, 0] > 0)))
        metres += float(np.sum(obs["progress_delta"][:, 0]))
    laps = metres / track.length
    print("%d envs on %d obstacle slots (%d obstacles each, drawn %d times), %d steps: %d crashes over %.1f laps driven: %.2f collisions per lap"
          % (E, SLOTS, args.obstacles, draws, args.steps, crashes, laps, crashes / max(laps, 1e-9)))
    env.sim.batch.close()


if __name__ == "__main__":
    main()
