#!/usr/bin/env python3
"""Time the raceline solve (f110_raceline_batch) against its NumPy restatement.

    python tools/raceline_bench.py [--calls 5] [--out profiles/raceline_bench.txt] [--resources]

T = 1, 8, 64, 256 copies of one line in one call, at M = 688 stations (random_track(3, 40, 1.5) at the default spacing) and at
M = 4096 (the same track at the spacing that gives the most stations the kernel takes), default settings (4 levels, 200 iterations
each).  Per case, `calls` back-to-back BatchSim.raceline_batch calls between two HIP events on the handle's stream (f110_timer_begin /
f110_timer_end_ms) and by the wall clock, after one warm call: the kernel plus the lines' upload, the results' download and the
call's one wait.  Beside it the restatement (tests/raceline_ref.py), timed on one line and multiplied by T: it has no batch form.
--resources compiles the library once more with the compiler's resource remarks and reports the four instantiations of k_raceline
(needs no GPU).  A record, not a gate.
"""
import argparse
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import f1tenth_gym_amd as amd  # noqa: E402
from f1tenth_gym_amd import _ffi, build, workload  # noqa: E402
import raceline_ref as ref  # noqa: E402


def kernel_resources():
    """the compiler's figures for every k_raceline instantiation: [(name, vgprs, lds bytes, scratch bytes, waves per SIMD)]"""
    cmd = [build.find_hipcc()] + build.HIPCC_FLAGS + ["-Rpass-analysis=kernel-resource-usage", build.SRC, "-o", os.devnull]
    text = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True).stdout
    rows = []
    for m in re.finditer(r"Function Name: (\S*k_raceline\S*)(.*?)LDS Size \[bytes/block\]: (\d+)", text, flags=re.S):
        body = m.group(2)
        grab = lambda key: int(re.search(re.escape(key) + r": (\d+)", body).group(1))   # noqa: E731
        lanes, beta = re.search(r"ILi(\d+)ELi(\d+)E", m.group(1)).groups()
        rows.append(("k_raceline<%s, %s>" % (lanes, beta), grab("VGPRs"), int(m.group(3)), grab("ScratchSize [bytes/lane]"), grab("Occupancy [waves/SIMD]")))
    return rows


def timed(sim, calls, fn):
    fn()            # warm: the kernel loaded
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "raceline_bench.txt"))
    ap.add_argument("--resources", action="store_true")
    args = ap.parse_args()
    lines = []
    if args.resources:
        for name, vgpr, lds, scratch, occ in kernel_resources():
            lines.append("%s: %d VGPRs, %d bytes of LDS per workgroup, %d bytes of scratch per lane, occupancy %d waves per SIMD (the compiler's figure)" % (name, vgpr, lds, scratch, occ))
    if _ffi.device_count() >= 1:
        lines.append("raceline_bench: default settings (levels 4, iters 200), %d calls each after one warm call, src %s" % (args.calls, build.src_hash()))
        track = amd.random_track(3, 40.0, 1.5)
        img, res, origin = workload.load_map_image("example_map")
        sim = amd.BatchSim(num_envs=1, num_agents=1)
        sim.set_map_image(img, res, origin)
        for spacing in (0.4, track.length / 4096):
            sp = amd.Raceline(spacing=spacing)
            q, w = sp.stations(track)
            t0 = time.perf_counter()
            for _ in range(3):
                want = ref.raceline(q, w)
            host_ms = (time.perf_counter() - t0) * 1e3 / 3
            for T in (1, 8, 64, 256):
                batch = [(q, w)] * T
                ev, wall = timed(sim, args.calls, lambda: sim.raceline_batch(batch, sp))
                ev0, _ = timed(sim, args.calls, lambda: sim.raceline_batch(batch, sp, [0] * T))   # the same call without the iteration loop
                out = sim.raceline_batch(batch, sp)
                same = all(np.array_equal(out[0][t * q.shape[0]:(t + 1) * q.shape[0]], want['alpha']) for t in range(T)) and np.all(out[5] == want['lap_time'])
                lines.append("M = %4d, T = %3d: %8.3f ms per call (events; %8.3f wall; %8.3f with no iterations: allocation, copies, profile), %7.3f ms per line; "
                             "NumPy %7.1f ms per line, x T = %9.1f ms (%s result)"
                             % (q.shape[0], T, ev, wall, ev0, ev / T, host_ms, host_ms * T, "the same" if same else "ANOTHER"))
        sim.close()
    else:
        lines.append("raceline_bench: no GPU visible, nothing timed")
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if args.out:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
