#!/usr/bin/env python3
"""Scripted cars that drive the racing line: F110VecEnv(track='raceline') solves berlin's raceline and speed profile on the device
 and four LineFollowers per env drive it — pure pursuit on the line of the env's map slot, the speed from
the profile, slower behind a car ahead on the same lane.  No policy and no host in the loop: the step's actions are ignored, one
kernel writes every car's action from the track columns of the last step.

    map (HBM) --centerline--> Track --raceline--> kappa, vx, offset --set_track--> s, lateral per agent --k_follow_line--> actions

The four cars differ in vgain and lane_offset, so the faster ones catch the slower ones and queue behind them.

    python examples/line_followers.py [--map berlin] [--envs 2] [--laps 1] [--iters 100] [--margin 0.45]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CARS = (dict(vgain=0.85, lane_offset=0.0), dict(vgain=0.7, lane_offset=0.15), dict(vgain=0.6, lane_offset=-0.15), dict(vgain=0.5, lane_offset=0.0))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--map", default="berlin")
    ap.add_argument("--envs", type=int, default=2)
    ap.add_argument("--laps", type=int, default=1)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--margin", type=float, default=0.45)
    ap.add_argument("--max-steps", type=int, default=20000)
    args = ap.parse_args(argv)
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    E, A = args.envs, len(CARS)
    followers = {a: amd.LineFollower(**kw) for a, kw in enumerate(CARS)}
    env = amd.F110VecEnv(E, device_logic=True, map=workload.map_stem(args.map), map_ext=".png", num_agents=A, track='raceline',
                         raceline=dict(iters=args.iters, margin=args.margin), scripted=followers)
    rl = env.tracks[0]
    print("%s: %r, lap time of the profile %.2f s; %d envs x %d line followers: %s" % (
        args.map, rl, rl.lap_time, E, A, ", ".join("vgain %.2f offset %+.2f" % (c["vgain"], c["lane_offset"]) for c in CARS)))
    # the fastest car at the back, 5 m between cars, the envs spread around the lap
    s0 = (np.arange(E) * rl.length / E)[:, None] + 1.0 + 5.0 * np.arange(A)[None, :]
    xy, tan = rl.point_at(s0.reshape(-1))
    env.reset(np.column_stack([xy, np.arctan2(tan[:, 1], tan[:, 0])]).reshape(E, A, 3))
    travelled, lap_step, gap_min, hit = np.zeros((E, A)), np.full((E, A), -1), np.inf, False
    acts = np.zeros((E, A, 2))                           # ignored: every car is scripted
    for t in range(args.max_steps):
        obs = env.step(acts)[0]
        travelled += np.asarray(obs["progress_delta"]).reshape(E, A)
        lap_step = np.where((lap_step < 0) & (travelled >= args.laps * rl.length), t + 1, lap_step)
        s = np.asarray(obs["progress"]).reshape(E, A)
        g = np.abs((s[:, :, None] - s[:, None, :] + 0.5 * rl.length) % rl.length - 0.5 * rl.length) + np.where(np.eye(A, dtype=bool), np.inf, 0.0)
        if t > 0:
            gap_min = min(gap_min, float(g.min()))
        hit = bool(np.asarray(obs["collisions"]).any())
        if hit or np.all(lap_step >= 0):
            break
    env.sim.batch.close()
    if hit or np.any(lap_step < 0):
        print("no lap: %s after %d steps, %.1f .. %.1f m travelled" % ("a collision" if hit else "out of steps", t + 1, travelled.min(), travelled.max()))
        return 1
    for a, c in enumerate(CARS):
        print("car %d (vgain %.2f): %d lap(s) in %.2f .. %.2f s" % (a, c["vgain"], args.laps, lap_step[:, a].min() * env.timestep, lap_step[:, a].max() * env.timestep))
    print("smallest gap between two cars of an env along the line: %.2f m" % gap_min)
    return 0


if __name__ == "__main__":
    sys.exit(main())
