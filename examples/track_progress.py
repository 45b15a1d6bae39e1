"""Lap progress along the example raceline: F110Env with track= and reward='progress', driven by the reference's pure-pursuit
planner (examples/waypoint_follow.py's PurePursuitPlanner, evaluated on the GPU through BatchSim.pure_pursuit_batch).

    python examples/track_progress.py [--laps 2]

Prints, every second of simulated time, the ego's arc length along the track, its lateral offset and heading error, and the
summed reward (metres of progress); at the end the total against laps x the track's length.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from f1tenth_gym_amd import F110Env  # noqa: E402
from f1tenth_gym_amd import workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--laps", type=int, default=2, help="the env ends an episode after 2 laps (the reference's rule)")
    args = ap.parse_args()
    csv = os.path.join(workload.PKG_MAPS, "example_waypoints.csv")
    env = F110Env(map=workload.map_stem("example_map"), map_ext=".png", num_agents=1, track=csv, reward='progress')
    w = workload.raceline()
    wp = np.ascontiguousarray(w[:, [1, 2, 5]])                         # x, y, speed
    lookahead, vgain, wheelbase = 0.82461887897713965, 0.90338203837889, 0.17145 + 0.15875   # config_example_map.yaml
    obs, total, done, _ = env.reset(np.array([[w[0, 1], w[0, 2], w[0, 3] + np.pi / 2]]))
    print("track: %d segments, L = %.5f m" % (env.track.num_segments, env.track.length))
    step = 0
    while not done and obs['lap_counts'][0] < args.laps:
        pose = np.array([[obs['poses_x'][0], obs['poses_y'][0], obs['poses_theta'][0]]])
        obs, r, done, _ = env.step(env.sim.batch.pure_pursuit_batch(wp, pose, lookahead, vgain, wheelbase))
        total += r
        step += 1
        if step % 100 == 0:
            print("t=%6.2f s  s=%8.3f m  lateral=%+.3f m  heading_error=%+.3f rad  progress=%8.3f m  laps=%d"
                  % (step * env.timestep, obs['progress'][0], obs['lateral_offset'][0], obs['heading_error'][0], total,
                     obs['lap_counts'][0]))
    print("done after %d steps: progress %.3f m, %d x L = %.3f m" % (step, total, args.laps, args.laps * env.track.length))
    env.sim.batch.close()


if __name__ == "__main__":
    main()
