// tests/host_harness/line_follower_main.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the line follower's arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp: line_lookahead .. line_env), as a
// stand-alone program for tests/test_line_follower_host.py: what k_follow_line computes with a lane per agent, on the CPU, one
// env after the other.  The track columns are built the way f110_track_set builds them.
//   line_follower_main IN OUT   IN: int32 cases, then per case int32 closed, npts, C, A, m, speed_attr, double [18] the settings
//                               in f110_line_follower's order, xy [npts][2], attrs [npts][C], rows [m][7];
//                               OUT per case: actions [m][2], raw [m][12]
//   line_follower_main          a self-check on a square (also what a sanitizer build runs)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

struct Case {
    int32_t closed = 0, npts = 0, C = 0, A = 1, m = 0;
    LineSpec sp{};
    std::vector<double> xy, attrs, rows;   // [npts][2], [npts][C], [m][7]
    std::vector<double> actions, raw;      // [m][2], [m][12]
};

static void run(Case &c)
{
    const int m = c.npts, nseg = c.closed ? m : m - 1;
    std::vector<double> cols(7 * (size_t)nseg), attr((size_t)c.C * m);
    double cum = 0.0;
    for (int k = 0; k < nseg; ++k) {
        const int k1 = k + 1 == m ? 0 : k + 1;
        const double ax = c.xy[2 * (size_t)k], ay = c.xy[2 * (size_t)k + 1];
        const double dx = c.xy[2 * (size_t)k1] - ax, dy = c.xy[2 * (size_t)k1 + 1] - ay;
        const double l2 = dx * dx + dy * dy;
        cols[(size_t)k] = ax;
        cols[(size_t)nseg + k] = ay;
        cols[2 * (size_t)nseg + k] = dx;
        cols[3 * (size_t)nseg + k] = dy;
        cols[4 * (size_t)nseg + k] = l2;
        cols[5 * (size_t)nseg + k] = std::sqrt(l2);
        cols[6 * (size_t)nseg + k] = cum;
        cum += std::sqrt(l2);
    }
    for (int k = 0; k < m; ++k)
        for (int q = 0; q < c.C; ++q) attr[(size_t)q * m + k] = c.attrs[(size_t)k * c.C + q];
    PreviewTrack tr;
    tr.cols = cols.data();
    tr.attr = c.C ? attr.data() : nullptr;
    tr.nseg = nseg;
    tr.closed = c.closed;
    tr.C = c.C;
    tr.npts = m;
    tr.L = cum;
    c.actions.assign(2 * (size_t)c.m, 0.0);
    c.raw.assign((size_t)LINE_NRAW * c.m, 0.0);
    for (int e = 0; e < c.m / c.A; ++e)
        line_env(c.sp, tr, c.rows.data() + 7 * (size_t)e * c.A, c.A, c.actions.data() + 2 * (size_t)e * c.A, c.raw.data() + (size_t)LINE_NRAW * e * c.A);
}

static LineSpec spec_of(const double *d, int32_t speed_attr)
{
    LineSpec o{};
    o.look_base = d[0], o.look_gain = d[1], o.look_min = d[2], o.look_max = d[3], o.lane_offset = d[4], o.wheelbase = d[5], o.steer_max = d[6];
    o.v_const = d[7], o.vgain = d[8], o.speed_look = d[9], o.lat_slow = d[10], o.v_recover = d[11];
    o.follow_range = d[12], o.follow_gap = d[13], o.follow_gain = d[14], o.lane_width = d[15], o.v_min = d[16], o.v_max = d[17];
    o.speed_attr = speed_attr;
    return o;
}

template <typename T>
static bool get(FILE *f, T *p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }

static int self_check()
{
    Case c;
    c.closed = 1, c.npts = 4, c.C = 2, c.A = 2, c.m = 4;
    c.xy = {0, 0, 10, 0, 10, 10, 0, 10};
    c.attrs = {0, 2, 0, 3, 0, 4, 0, 5};
    const double d[18] = {0.8, 0.25, 0.6, 3.9, 0.0, 0.3302, 0.4189, 2.0, 0.8, 0.6, 0.5, 1.5, 6.0, 1.0, 1.0, 0.6, 0.0, 20.0};
    c.sp = spec_of(d, 1);
    // env 0: a car left of the first side with a standing car 1 m ahead; env 1: a fresh car and one just short of the wrap
    c.rows = {1, 0.1, 0, 2, 1, 0.1, 5, 2, 0, 0, 0, 2, 0, 5, 0, 5, 0, 1, 30, 0, 0, 0.2, 8.5, -1.57, 3, 38.5, 0.2, 9};
    run(c);
    const double *a = c.actions.data(), *r = c.raw.data();
    bool ok = r[LINE_RAW_LD] == 0.8 + 0.25 * 2.0 && r[LINE_RAW_K] == 0.0 && r[LINE_RAW_LIM] == 1.0 && a[1] == 0.0;   // stopped by the car ahead
    ok = ok && a[0] < 0.0 && a[0] > -0.4189;                                                                       // back to the line from its left
    ok = ok && a[4] == 0.0 && a[5] == 0.0 && r[2 * LINE_NRAW + LINE_RAW_K] == -1.0;                                  // fresh
    ok = ok && r[3 * LINE_NRAW + LINE_RAW_K] == 0.0 && r[3 * LINE_NRAW + LINE_RAW_ST] == (38.5 + (0.8 + 0.25 * 3.0)) - 40.0;   // wrapped
    if (!ok) {
        std::printf("self-check failed: %.17g %.17g %.17g %.17g\n", a[0], a[1], r[LINE_RAW_LD], r[3 * LINE_NRAW + LINE_RAW_ST]);
        return 1;
    }
    std::printf("ok: 4 rows\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 1) return self_check();
    if (argc != 3) return 2;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n = 0;
    if (!get(f, &n, 1) || n < 0) return 2;
    std::vector<Case> cases((size_t)n);
    for (Case &c : cases) {
        int32_t hd[6];
        double d[18];
        if (!get(f, hd, 6) || !get(f, d, 18)) return 2;
        c.closed = hd[0], c.npts = hd[1], c.C = hd[2], c.A = hd[3], c.m = hd[4];
        if (c.npts < 2 || c.C < 0 || c.C > PREVIEW_MAX_ATTRS || c.A < 1 || c.m < 0 || c.m % c.A || hd[5] < -1 || hd[5] >= c.C) return 2;
        c.sp = spec_of(d, hd[5]);
        c.xy.resize(2 * (size_t)c.npts);
        c.attrs.resize((size_t)c.npts * c.C);
        c.rows.resize(7 * (size_t)c.m);
        if (!get(f, c.xy.data(), c.xy.size()) || !get(f, c.attrs.data(), c.attrs.size()) || !get(f, c.rows.data(), c.rows.size())) return 2;
    }
    std::fclose(f);
    FILE *g = std::fopen(argv[2], "wb");
    if (!g) return 2;
    for (Case &c : cases) {
        run(c);
        std::fwrite(c.actions.data(), sizeof(double), c.actions.size(), g);
        std::fwrite(c.raw.data(), sizeof(double), c.raw.size(), g);
    }
    std::fclose(g);
    return 0;
}
