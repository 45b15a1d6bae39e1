"""tools/blocks_overlap.py on a hand-made kernel trace: durations and the share of a kernel under the other stream's scan"""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("blocks_overlap", os.path.join(ROOT, "tools", "blocks_overlap.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _trace(path, steps):
    """two streams half a step (100 ns) apart; per step k and stream, from t = 200 k (+ 100 on stream 2): integrate [t, t + 10),
    scan [t + 10, t + 110), finalize [t + 110, t + 150).  So the scans of the two streams follow each other end to start, and
    every integrate and every finalize lies inside the other stream's scan"""
    rows = ["Kind,Agent_Id,Queue_Id,Stream_Id,Kernel_Name,Start_Timestamp,End_Timestamp"]
    for k in range(steps):
        for stream, off in ((1, 0), (2, 100)):
            t = 200 * k + off
            rows.append("KERNEL_DISPATCH,0,%d,%d,\"k_integrate_duo(AgentArrays, ScanConst, double const*)\",%d,%d" % (stream, stream, t, t + 10))
            rows.append("KERNEL_DISPATCH,0,%d,%d,\"void k_scan_rays_agent<false, true, false>(RayJob)\",%d,%d" % (stream, stream, t + 10, t + 110))
            rows.append("KERNEL_DISPATCH,0,%d,%d,\"void k_finalize_pair_wave<12>(AgentArrays, int)\",%d,%d" % (stream, stream, t + 110, t + 150))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")


def test_overlap_shares(tmp_path):
    m = _tool()
    p = str(tmp_path / "t_kernel_trace.csv")
    _trace(p, 50)
    rows = m.load(p)
    assert len(rows) == 300 and rows[0][2] == "k_integrate_duo" and rows[1][2] == "k_scan_rays_agent"
    n_streams, cut, acc = m.summarize(rows, 20, "k_scan")
    assert n_streams == 2 and cut == 200 * 30 + 10
    # after the cut (6010): stream 1's steps 30 .. 49 without the integrate at 6000, stream 2's steps 30 .. 49 and the finalize of
    # its step 29 at 6010; stream 2's last finalize has no scan of a step 50 above it
    assert acc["k_finalize_pair_wave"] == (41, 41 * 40, 40 * 40)
    assert acc["k_scan_rays_agent"] == (40, 40 * 100, 0)
    assert acc["k_integrate_duo"] == (39, 39 * 10, 39 * 10)


def test_one_stream_shows_nothing_hidden(tmp_path):
    m = _tool()
    p = str(tmp_path / "t_kernel_trace.csv")
    _trace(p, 10)
    rows = [r for r in m.load(p) if r[3] == "1"]
    n_streams, _, acc = m.summarize(rows, 5, "k_scan")
    assert n_streams == 1 and all(hid == 0 for _, _, hid in acc.values())
