#!/usr/bin/env python3
"""How much of each kernel runs under the OTHER env block's scan?

Reads the kernel trace of one `bench.py --only-headline` run,

    rocprofv3 --kernel-trace -d DIR -o NAME -- python bench.py --only-headline [--groups 2] ...

(the program after `--`, no `--pmc` in the same run), and prints per kernel name, over the last STEPS steps (default 300):
the number of launches, the mean duration, and the share of the kernel's own wall interval that lies inside a scan launch of
another stream.  A step that runs as one block shows 0 % everywhere; with two env blocks the share says how far a kernel of
one block is hidden under the other block's scan ("Env blocks").

    python tools/blocks_overlap.py DIR/NAME_kernel_trace.csv [--steps 300] [--scan k_scan]
"""
import argparse
import bisect
import collections
import csv
import sys


def short(name):
    return name.split("(")[0].replace("void ", "").strip()


def family(name):
    """the kernel without its template arguments (k_finalize_pair_roles<32, false> -> k_finalize_pair_roles)"""
    return short(name).split("<")[0]


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            stream = r.get("Stream_Id") or r.get("Queue_Id") or "?"
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), family(r["Kernel_Name"]), stream))
    rows.sort()
    return rows


def covered(lo, hi, starts, ends):
    """length of [lo, hi) inside the sorted, pairwise disjoint intervals [starts[k], ends[k])"""
    total = 0
    k = max(bisect.bisect_right(starts, lo) - 1, 0)
    while k < len(starts) and starts[k] < hi:
        total += max(0, min(hi, ends[k]) - max(lo, starts[k]))
        k += 1
    return total


def summarize(rows, steps, scan_key):
    scans = collections.defaultdict(list)   # stream -> its scan launches, in time order (one stream runs them one after the other)
    for s, e, name, stream in rows:
        if scan_key in name:
            scans[stream].append((s, e))
    if not scans:
        raise SystemExit("no kernel whose name contains '%s' in the trace" % scan_key)
    # the last `steps` steps: every stream that steps launches one scan per step
    cut = min(v[-min(steps, len(v))][0] for v in scans.values() if len(v) >= max(1, steps // 4))
    by_stream = {st: ([a for a, _ in v], [b for _, b in v]) for st, v in scans.items()}
    acc = collections.OrderedDict()
    for s, e, name, stream in rows:
        if s < cut:
            continue
        n, dur, hid = acc.get(name, (0, 0, 0))
        under = sum(covered(s, e, *by_stream[o]) for o in by_stream if o != stream)
        acc[name] = (n + 1, dur + (e - s), hid + min(under, e - s))
    return len(scans), cut, acc


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("trace", help="rocprofv3 kernel trace (CSV)")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--scan", default="k_scan", help="substring that names the scan kernels")
    args = ap.parse_args()
    rows = load(args.trace)
    n_streams, cut, acc = summarize(rows, args.steps, args.scan)
    span = max(e for _, e, _, _ in rows) - cut
    print("# %d kernel launches after the cut, %d stream(s) with scan launches, %.1f us of wall time (%.1f us per step over %d steps)"
          % (sum(v[0] for v in acc.values()), n_streams, span / 1e3, span / 1e3 / args.steps, args.steps))
    print("# %-28s %8s %12s %22s" % ("kernel", "launches", "mean us", "under the other scan"))
    for name, (n, dur, hid) in sorted(acc.items(), key=lambda kv: -kv[1][1]):
        print("  %-28s %8d %12.1f %20.1f %%" % (name, n, dur / n / 1e3, 100.0 * hid / dur if dur else 0.0))
    return 0


if __name__ == "__main__":
    sys.exit(main())
