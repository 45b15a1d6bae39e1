#!/usr/bin/env python3
"""A racing line without a csv: F110VecEnv(track='raceline') extracts berlin's centreline from the map's distance table, solves a
raceline and a speed profile from it on the device and makes it the track.  A pure-pursuit rule then drives on the
track preview — a station ahead for the steering, the raceline's vx (attribute 1) for the speed — until every car has done a lap.

    map (HBM) --centerline--> Track --raceline--> Track with kappa, vx, offset --set_track--> obs['track_preview'] --rule--> actions

The rule runs in torch on the preview's device buffer (through DLPack, no type of this package on torch's side) when torch sees the
GPU, otherwise in NumPy on the observation.

    python examples/raceline.py [--map berlin] [--envs 4] [--iters 200] [--margin 0.45] [--vgain 0.8] [--numpy]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

POINTS, OFFSET, SPACING = 12, 0.3, 0.3       # the preview: stations 0.3, 0.6, ... 3.6 m ahead of the car's projection
WHEELBASE, STEER_MAX = 0.17145 + 0.15875, 0.4189


def rule(xp, pv, v, vgain):
    """pure pursuit on the preview [N][P][3] = (x, y, vx) in the car's frame, v [N] the car's speed -> (steer [N], speed [N]);
    xp is numpy or torch: the same lines serve both"""
    look = xp.clip(xp.round((0.8 + 0.25 * v - OFFSET) / SPACING), 1, POINTS - 1)
    if xp is np:
        at = pv[np.arange(pv.shape[0]), look.astype(np.int64)]
    else:
        at = pv[xp.arange(pv.shape[0], device=pv.device), look.long()]
    d2 = at[:, 0] ** 2 + at[:, 1] ** 2
    steer = xp.clip(xp.arctan(2.0 * WHEELBASE * at[:, 1] / d2), -STEER_MAX, STEER_MAX)
    return steer, vgain * pv[:, 1, 2]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--map", default="berlin")
    ap.add_argument("--envs", type=int, default=4)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--margin", type=float, default=0.45)
    ap.add_argument("--vgain", type=float, default=0.8)
    ap.add_argument("--max-steps", type=int, default=30000)
    ap.add_argument("--numpy", action="store_true", help="the rule in NumPy even when torch sees the GPU")
    args = ap.parse_args(argv)
    torch = None
    if not args.numpy:
        try:
            import torch                               # (torch first, then the simulator's library)
            if not torch.cuda.is_available():
                torch = None
        except ImportError:
            torch = None
    import f1tenth_gym_amd as amd
    from f1tenth_gym_amd import workload
    E = args.envs
    preview = amd.TrackPreview(points=POINTS, offset=OFFSET, spacing=SPACING, channels=("x", "y", "attr1"), frame="ego")
    env = amd.F110VecEnv(E, device_logic=True, map=workload.map_stem(args.map), map_ext=".png", num_agents=1, track='raceline',
                         raceline=dict(iters=args.iters, margin=args.margin), track_preview=preview, reward='progress')
    rl = env.tracks[0]
    kappa, vx, offset = rl.attrs[:, 0], rl.attrs[:, 1], rl.attrs[:, 2]
    print("%s: %r from %d stations; offset %.2f .. %.2f m, |kappa| up to %.2f 1/m (centre %.2f), vx %.2f .. %.2f m/s"
          % (args.map, rl, rl.num_points, offset.min(), offset.max(), np.abs(kappa).max(), np.abs(rl.center.attrs[:, 1]).max(), vx.min(), vx.max()))
    print("lap time of the profile: %.2f s on the raceline, %.2f s on the centreline (%.1f %% less)"
          % (rl.lap_time, rl.center_lap_time, 100.0 * (1.0 - rl.lap_time / rl.center_lap_time)))
    s0 = np.arange(E) * rl.length / E + 1.0
    xy, tan = rl.point_at(s0)
    obs = env.reset(np.column_stack([xy, np.arctan2(tan[:, 1], tan[:, 0])]).reshape(E, 1, 3))[0]
    pv_t = None
    if torch is not None:
        stream = torch.cuda.ExternalStream(env.sim.batch.device_views()["stream"], device=torch.device("cuda", env.sim.batch.device_id))
        pv_t = torch.from_dlpack(env.preview_buffer).reshape(E, POINTS, 3)     # float32 over the preview's own memory
    travelled, lap_step, hit = np.zeros(E), np.full(E, -1), False
    acts = np.zeros((E, 1, 2))
    for t in range(args.max_steps):
        v = np.asarray(obs["linear_vels_x"]).reshape(E)
        if pv_t is not None:
            with torch.cuda.stream(stream):
                steer, speed = rule(torch, pv_t, torch.as_tensor(v, dtype=torch.float32, device=pv_t.device), args.vgain)
                steer, speed = steer.cpu().numpy(), speed.cpu().numpy()
        else:
            steer, speed = rule(np, np.asarray(obs["track_preview"]).reshape(E, POINTS, 3), v.astype(np.float32), args.vgain)
        acts[:, 0, 0], acts[:, 0, 1] = steer, speed
        obs, reward, _, _ = env.step(acts)
        travelled += np.asarray(reward).reshape(E)
        lap_step = np.where((lap_step < 0) & (travelled >= rl.length), t + 1, lap_step)
        hit = bool(np.asarray(obs["collisions"]).any())
        if hit or np.all(lap_step >= 0):
            break
    lat = np.abs(np.asarray(obs["lateral_offset"])).max()
    del pv_t                                             # the tensor views the simulator's memory: it goes before close()
    if torch is not None:
        torch.cuda.synchronize()
    env.sim.batch.close()
    if hit or np.any(lap_step < 0):
        print("no lap: %s after %d steps, %.1f .. %.1f m of %.1f m travelled" % ("a collision" if hit else "out of steps", t + 1, travelled.min(), travelled.max(), rl.length))
        return 1
    print("lap completed by %d car(s) in %.2f .. %.2f s at vgain %.2f (the profile's %.2f s / vgain = %.2f s), rule in %s; |lateral offset| at the end <= %.2f m"
          % (E, lap_step.min() * env.timestep, lap_step.max() * env.timestep, args.vgain, rl.lap_time, rl.lap_time / args.vgain, "torch via DLPack" if torch is not None else "NumPy", lat))
    return 0


if __name__ == "__main__":
    sys.exit(main())
