#!/usr/bin/env python3
"""Time the in-place obstacle re-stamp (f110_set_map_obstacles) against what it replaces.

    python tools/obstacles_bench.py [--calls 50] [--out profiles/obstacles_bench.txt]

On example_map, with 8 and with 64 obstacles on the raceline: `calls` back-to-back BatchSim.set_obstacles between two HIP events
on the handle's stream (f110_timer_begin / f110_timer_end_ms), and the same number of BatchSim.add_map_image calls on the image with
the stamped cells blacked out, timed the same way — the existing pipeline (upload, flip, threshold, full exact EDT, padded copy, a new
table per call) and what a user would run today.  Wall-clock times are printed next to the event times.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import f1tenth_gym_amd as amd  # noqa: E402
from f1tenth_gym_amd import build, workload  # noqa: E402


def stamped_image(img, ob, res, origin):
    """the image with the cells of `ob` set to 0, by the header's stamp rule (NumPy)"""
    H, W = img.shape
    oc, os_ = float(np.cos(origin[2])), float(np.sin(origin[2]))
    px = np.broadcast_to((np.arange(W, dtype=np.float64)[None, :] + 0.5) * res, (H, W))
    py = np.broadcast_to((np.arange(H, dtype=np.float64)[:, None] + 0.5) * res, (H, W))
    wx, wy = origin[0] + (px * oc - py * os_), origin[1] + (px * os_ + py * oc)
    m = np.zeros((H, W), dtype=bool)
    for shape, x, y, c, s, hl, hw in ob.rows:
        dx, dy = wx - x, wy - y
        if int(shape) == 1:
            m |= dx * dx + dy * dy <= hl * hl
        else:
            m |= (np.abs(dx * c + dy * s) <= hl) & (np.abs(-dx * s + dy * c) <= hw)
    out = img.copy()
    out[np.flipud(m)] = 0
    return out, int(m.sum()), int(m.any(axis=0).sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obstacles_bench.txt"))
    args = ap.parse_args()
    img, res, origin = workload.load_map_image("example_map")
    track = amd.Track(workload.raceline()[:, 1:3])
    lines = ["obstacles_bench: example_map %d x %d, %d calls each, src %s" % (img.shape[0], img.shape[1], args.calls, build.src_hash())]
    for n in (8, 64):
        lists = [amd.Obstacles.random_on_track(track, n, seed, lateral=0.4, min_gap=2.0) for seed in (1, 2)]
        images = [stamped_image(img, ob, res, origin) for ob in lists]
        sim = amd.BatchSim(num_envs=1, num_agents=1)
        sim.set_map_image(img, res, origin)
        slot = sim.add_obstacle_map(lists[0])
        for ob in lists:                      # warm: scratch sized, kernels loaded
            sim.set_obstacles(slot, ob)
        sim.sync()
        t0 = time.perf_counter()
        sim.timer_begin()
        for k in range(args.calls):
            sim.set_obstacles(slot, lists[k % 2])
        ev_set = sim.timer_end_ms()
        wall_set = (time.perf_counter() - t0) * 1e3
        sim.add_map_image(images[0][0], res, origin)   # warm
        sim.sync()
        t0 = time.perf_counter()
        sim.timer_begin()
        for k in range(args.calls):
            sim.add_map_image(images[k % 2][0], res, origin)
        ev_add = sim.timer_end_ms()
        wall_add = (time.perf_counter() - t0) * 1e3
        sim.close()
        lines.append("%2d obstacles (%d stamped cells, %d of %d columns active): set_obstacles %.3f ms per call (events; %.3f wall), "
                     "add_map_image %.3f ms per call (events; %.3f wall): %.1f x"
                     % (n, images[0][1], images[0][2], img.shape[1], ev_set / args.calls, wall_set / args.calls, ev_add / args.calls,
                        wall_add / args.calls, ev_add / max(ev_set, 1e-9)))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
