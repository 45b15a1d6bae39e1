#!/usr/bin/env python3
"""Time the corridor carve (f110_add_map_corridor / f110_set_map_corridor) against what a user did before it.

    python tools/trackgen_bench.py [--calls 5] [--out profiles/trackgen_bench.txt]

Two frames at 0.0625 m: 1600 x 1600 cells around a random line of radius 25 m (about 800 segments) and 600 x 600 around one of
radius 8 m.  Per frame, `calls` back-to-back calls between two HIP events on the handle's stream (f110_timer_begin /
f110_timer_end_ms) and by the wall clock, each after one warm call: BatchSim.add_track_map, BatchSim.set_track_map (both include
set_track of the line); the mask kernel ALONE and the two passes of the distance transform, by the events the library records
around them inside a carve (f110_map_corridor_times: the line already on the device, the mask staying there), as the mean over the
set_track_map calls; BatchSim.corridor_mask, the unit call (the kernel plus the line's upload and the mask's download); and, for
comparison, the host's way: the rule in NumPy, each segment on the window of cells its capsule can reach (the cheapest form the
host has; it must give the device's mask), plus BatchSim.add_map_image of that image.  A record, not a gate.
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


def segment_hits(wx, wy, a, b, hw):
    """the rule of include/f110.h for one segment on arrays of cell centres"""
    ux, uy = wx - a[0], wy - a[1]
    dx, dy = b[0] - a[0], b[1] - a[1]
    t, L2, h2 = ux * dx + uy * dy, dx * dx + dy * dy, hw * hw
    vx, vy = wx - b[0], wy - b[1]
    cr = ux * dy - uy * dx
    return np.where(t <= 0.0, ux * ux + uy * uy <= h2, np.where(t >= L2, vx * vx + vy * vy <= h2, cr * cr <= h2 * L2))


def host_mask(tm):
    """the rule in NumPy on each segment's window of cells (yaw 0 frames), the border ring cleared: bool [H][W]"""
    H, W = tm.shape
    res, ox, oy, oc, os_ = tm.frame()
    assert oc == 1.0 and os_ == 0.0
    xy, hw = tm.points(), tm.widths()
    a, b = (xy, np.roll(xy, -1, axis=0)) if tm.track.closed else (xy[:-1], xy[1:])
    m = np.zeros((H, W), dtype=bool)
    for i in range(a.shape[0]):
        lo = np.minimum(a[i], b[i]) - hw[i]
        hi = np.maximum(a[i], b[i]) + hw[i]
        c0, c1 = max(0, int((lo[0] - ox) / res) - 2), min(W, int((hi[0] - ox) / res) + 3)
        r0, r1 = max(0, int((lo[1] - oy) / res) - 2), min(H, int((hi[1] - oy) / res) + 3)
        if c0 >= c1 or r0 >= r1:
            continue
        wx = np.broadcast_to(ox + (np.arange(c0, c1, dtype=np.float64)[None, :] + 0.5) * res, (r1 - r0, c1 - c0))
        wy = np.broadcast_to(oy + (np.arange(r0, r1, dtype=np.float64)[:, None] + 0.5) * res, (r1 - r0, c1 - c0))
        m[r0:r1, c0:c1] |= segment_hits(wx, wy, a[i], b[i], float(hw[i]))
    m[0, :] = m[H - 1, :] = False
    m[:, 0] = m[:, W - 1] = False
    return m


def timed(sim, calls, fn):
    fn()            # warm: scratch sized, kernels loaded
    sim.sync()
    t0 = time.perf_counter()
    sim.timer_begin()
    for _ in range(calls):
        fn()
    ev = sim.timer_end_ms() / calls
    return ev, (time.perf_counter() - t0) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trackgen_bench.txt"))
    args = ap.parse_args()
    lines = ["trackgen_bench: 0.0625 m per cell, half width 1 m, %d calls each after one warm call, src %s" % (args.calls, build.src_hash())]
    for side, radius, seed in ((1600, 25.0, 5), (600, 8.0, 5)):
        half = 0.5 * side * 0.0625
        tms = [amd.TrackMap(amd.random_track(seed + k, radius=radius), shape=(side, side), origin=(-half, -half, 0.0)) for k in range(2)]
        tm = tms[0]
        img0, res0, origin0 = workload.load_map_image("example_map")
        sim = amd.BatchSim(num_envs=1, num_agents=1)
        sim.set_map_image(img0, res0, origin0)
        ev_add, wall_add = timed(sim, args.calls, lambda: sim.add_track_map(tm))
        slot = sim.add_track_map(tm)
        flip = [0]

        stages = []

        def recarve():
            flip[0] ^= 1
            sim.set_track_map(slot, tms[flip[0]])
            stages.append(sim.corridor_times())
        ev_set, wall_set = timed(sim, args.calls, recarve)
        k_mask = float(np.mean([st["mask"] for st in stages[1:]]))
        k_edt = float(np.mean([st["edt"] for st in stages[1:]]))
        ev_mask, wall_mask = timed(sim, args.calls, lambda: sim.corridor_mask(tm))
        mask, carved = sim.corridor_mask(tm)
        t0 = time.perf_counter()
        hm = host_mask(tm)
        host_s = time.perf_counter() - t0
        same = np.array_equal(hm, mask.astype(bool))
        img = np.ascontiguousarray(np.flipud(np.where(hm, 255, 0).astype(np.uint8)))   # carved cells white, top row first
        ev_img, wall_img = timed(sim, args.calls, lambda: sim.add_map_image(img, tm.resolution, list(tm.origin)))
        sim.set_track_map(slot, tm)
        table_same = np.array_equal(sim.get_map_dt(slot), sim.get_map_dt(sim.add_map_image(img, tm.resolution, list(tm.origin))))
        sim.close()
        lines.append("%4d x %4d, %4d segments, %7d cells carved (%.1f %%): add_track_map %.3f ms per call (events; %.3f wall); set_track_map %.3f (%.3f wall); "
                     "inside a carve the mask kernel alone %.3f and the distance transform %.3f; corridor_mask with its copies %.3f (%.3f wall); the host's way: NumPy mask on segment windows %.1f ms (%s mask) + add_map_image %.3f "
                     "(%.3f wall) = %.1f ms (%s table)"
                     % (side, side, tm.widths().shape[0], carved, 100.0 * carved / (side * side), ev_add, wall_add, ev_set, wall_set, k_mask, k_edt, ev_mask, wall_mask,
                        host_s * 1e3, "the same" if same else "ANOTHER", ev_img, wall_img, host_s * 1e3 + wall_img, "the same" if table_same else "ANOTHER"))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
