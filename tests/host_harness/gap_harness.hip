// tests/host_harness/gap_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the gap follower's per-row arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp, gap_*), for
// tests/test_gap_follower_host.py: clip, window mean, closest point, bubble, the run summaries and their merge operator, target
// and action are compared with the NumPy model without a GPU.  The GPU tests hold the device instantiation (and the kernel around
// it) to the same model.
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

extern "C" {

// scans [m][B], step_count [m] or null, actions [m][2], info [m][5] or null; d = range_clip, bubble_radius, gap_threshold,
// steer_gain, steer_max, v_lo, v_hi, d_ref, steer_slow, v_turn, v_blocked.  The caller has validated the settings.
void hh_gap_follow(int beam_lo, int beam_hi, int smooth, int target, const double *d, double fov, const double *scans, int B,
                   const int *step_count, int m, double *actions, int *info)
{
    GapSpec s{};
    s.lo = beam_lo;
    s.W = beam_hi - beam_lo;
    s.S = smooth;
    s.target = target;
    s.clip = d[0], s.bubble = d[1], s.thresh = d[2], s.steer_gain = d[3], s.steer_max = d[4], s.v_lo = d[5], s.v_hi = d[6];
    s.d_ref = d[7], s.steer_slow = d[8], s.v_turn = d[9], s.v_blocked = d[10];
    std::vector<double> v(s.W), p(s.W);
    for (int i = 0; i < m; ++i)
        gap_follow_row(s, scans + (size_t)i * B, B, fov, step_count ? step_count[i] : 1, v.data(), p.data(), actions + 2 * (size_t)i,
                       info ? info + 5 * (size_t)i : nullptr);
}

// the merge operator on its own: the free flags [n] cut into chunks at `cuts` [ncuts] (ascending, within 0..n; chunks of at most
// 64 beams), each summarised, then folded left to right and as a balanced tree (the wave's order).  out = best, best_start of
// the fold, then of the tree.
void hh_gap_runs(const unsigned char *free_, int n, const int *cuts, int ncuts, int *out)
{
    std::vector<GapRun> runs;
    int a = 0;
    for (int k = 0; k <= ncuts; ++k) {
        const int b = k < ncuts ? cuts[k] : n;
        unsigned long long m = 0;
        for (int i = a; i < b; ++i) m |= (unsigned long long)(free_[i] != 0) << (i - a);
        runs.push_back(gap_run_of_mask(m, a, b - a));
        a = b;
    }
    GapRun fold{};
    for (const GapRun &r : runs) fold = gap_run_merge(fold, r);
    out[0] = fold.best, out[1] = fold.best_start;
    while (runs.size() > 1) {
        std::vector<GapRun> next;
        for (size_t k = 0; k < runs.size(); k += 2) next.push_back(k + 1 < runs.size() ? gap_run_merge(runs[k], runs[k + 1]) : runs[k]);
        runs.swap(next);
    }
    out[2] = runs[0].best, out[3] = runs[0].best_start;
}

}
