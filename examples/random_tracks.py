"""Random tracks: follow-the-gap cars on eight tracks that exist nowhere but on the device.

Eight map slots are carved around random closed lines (random_track): a line plus a half width becomes the slot's distance table on
the device, and the line is the slot's track for the progress reward and the random starts.  Every few hundred steps one slot is
re-drawn in place with a fresh line (F110VecEnv.set_track_map: same frame, same table, no image, no upload of a map) and its envs
start again on it.  No map is ever made on the host or uploaded; per step only `done`, the collision flags and the progress reward
come back, for the printed summary.

    python examples/random_tracks.py [--envs 256] [--steps 2000] [--redraw 400] [--radius 8.0]

Prints the collisions per lap driven.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from f1tenth_gym_amd import F110VecEnv, GapFollower, ResetSampler, TrackMap, random_track  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402

SLOTS = 8
HALF_WIDTH = 1.0


def draw(seed, radius):
    """a random line in the ONE frame every slot shares, so that any slot can be re-carved with any later line: the star's largest
    radius is radius * (1 + 0.3 * (1 + 1/2 + 1/3 + 1/4)), plus the half width and a metre of wall"""
    reach = radius * 1.625 + HALF_WIDTH + 1.0
    side = int(np.ceil(2.0 * reach / 0.0625))
    return TrackMap(random_track(seed, radius=radius, half_width=HALF_WIDTH), shape=(side, side), origin=(-reach, -reach, 0.0))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--redraw", type=int, default=400, help="steps between two re-draws of one slot")
    ap.add_argument("--radius", type=float, default=8.0)
    args = ap.parse_args()
    E = args.envs
    maps = [draw(k, args.radius) for k in range(SLOTS)]
    env_map = 1 + np.arange(E) % SLOTS
    env = F110VecEnv(E, auto_reset=True, device_logic=True, num_agents=1, map=workload.map_stem("example_map"), map_ext=".png",
                     track_maps=maps, env_map=env_map, reward='progress', random_start=ResetSampler(seed=7, lateral=0.2, heading=0.1),
                     scripted={0: GapFollower()}, obs_fields=("collisions", "progress_delta"))
    env.reset()                                   # no poses: every env draws its own on its slot's line
    actions = np.zeros((E, 1, 2))                 # the scripted car's rows are replaced on the device
    crashes, metres, draws = 0, 0.0, 0
    for t in range(args.steps):
        if t and t % args.redraw == 0:            # one slot gets a new track, in place, behind the step in flight; its envs start again
            slot = 1 + draws % SLOTS
            env.set_track_map(slot, draw(SLOTS + draws, args.radius))
            env.reset(env_mask=env_map == slot)
            draws += 1
        obs, reward, done, _ = env.step(actions)
        crashes += int(np.sum(done & (obs["collisions"][:, 0] > 0)))
        metres += float(np.sum(reward))
    mean_lap = float(np.mean([tm.track.length for tm in env.track_maps.values()]))
    laps = metres / mean_lap
    print("%d envs on %d carved tracks (%d x %d cells each, %d slots re-drawn in place), %d steps: %d crashes over %.1f laps driven: %.2f collisions per lap"
          % (E, SLOTS, maps[0].shape[0], maps[0].shape[1], draws, args.steps, crashes, laps, crashes / max(laps, 1e-9)))
    env.sim.batch.close()


if __name__ == "__main__":
    main()
