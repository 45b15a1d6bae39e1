#!/usr/bin/env python3
"""Time the centreline extraction (f110_map_centerline) against the map pipeline and the NumPy reference.

    python tools/centerline_bench.py [--calls 5] [--maps example_map berlin vegas] [--no-numpy] [--out profiles/centerline_bench.txt]

Per map, seed (0, 0): `calls` back-to-back BatchSim.centerline_cells between two HIP events on the handle's stream (f110_timer_begin
/ f110_timer_end_ms) and by the wall clock, the last call's time per stage (f110_map_centerline_times: the host's clock between the
waits that end the stages), the same number of BatchSim.add_map_image calls of the same image timed the same way — the project's
existing map pipeline, the natural yardstick — and one run of the NumPy restatement of the rule (tests/centerline_ref.py) on the
seed's free component inside its bounding box, the cheapest form the host has (the device thins the whole mask), which must give
the same loop.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f1tenth_gym_amd as amd  # noqa: E402
from f1tenth_gym_amd import build, workload  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--maps", nargs="+", default=["example_map", "berlin", "vegas"])
    ap.add_argument("--no-numpy", action="store_true", help="skip the NumPy reference (tens of seconds on the large maps)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "centerline_bench.txt"))
    args = ap.parse_args()
    lines = ["centerline_bench: seed (0, 0), %d calls each, src %s" % (args.calls, build.src_hash())]
    for name in args.maps:
        img, res, origin = workload.load_map_image(name)
        sim = amd.BatchSim(num_envs=1, num_agents=1)
        sim.set_map_image(img, res, origin)
        cells, hw, deleted = sim.centerline_cells(0)          # warm: scratch sized, kernels loaded
        sim.sync()
        t0 = time.perf_counter()
        sim.timer_begin()
        for _ in range(args.calls):
            sim.centerline_cells(0)
        ev = sim.timer_end_ms() / args.calls
        wall = (time.perf_counter() - t0) * 1e3 / args.calls
        st = sim.centerline_times()
        sim.add_map_image(img, res, origin)                   # warm
        sim.sync()
        t0 = time.perf_counter()
        sim.timer_begin()
        for _ in range(args.calls):
            sim.add_map_image(img, res, origin)
        ev_add = sim.timer_end_ms() / args.calls
        wall_add = (time.perf_counter() - t0) * 1e3 / args.calls
        sim.close()
        ref_txt = "NumPy not run"
        if not args.no_numpy:
            import centerline_ref as ref
            free = ref.free_from_image(img)
            t0 = time.perf_counter()
            want = ref.centerline(free, free, res, origin, whole=False)
            ref_txt = "NumPy on the seed's component %.2f s (%s loop)" % (time.perf_counter() - t0, "the same" if np.array_equal(want[0], cells) else "ANOTHER")
        lines.append("%-12s %4d x %4d: loop %5d cells, deleted %d / %d / %d; centerline %.3f ms per call (events; %.3f wall) = thinning %.3f + staircase "
                     "%.3f + pruning %.3f + planes back, pick, trace, gather %.3f; add_map_image %.3f ms per call (events; %.3f wall): centerline / "
                     "add_map_image = %.2f; %s"
                     % (name, img.shape[0], img.shape[1], len(cells), deleted[0], deleted[1], deleted[2], ev, wall, st["thinning"], st["staircase"],
                        st["pruning"], st["host"], ev_add, wall_add, wall / max(wall_add, 1e-9), ref_txt))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
