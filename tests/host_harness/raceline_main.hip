// tests/host_harness/raceline_main.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the raceline rule's per-point arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp: rl_frame .. rl_lap_term),
// as a stand-alone program for tests/test_raceline_host.py: the walk k_raceline makes over a line — frame, the coarse-to-fine
// Jacobi iteration between two copies of p, curvature, the running sums, the four minima, the profile — on the CPU, one point
// after the other.
//   raceline_main IN OUT    IN: int32 T, then per line int32 M, levels, iters, double margin, v_max, a_lat, a_accel, a_brake,
//                           q [M][2], w [M];  OUT per line: int32 status (0 = ok, 1 = refused), and when ok alpha [M], xy [M][2],
//                           kappa [M], vx [M], length, lap_time
//   raceline_main           a self-check on ellipses (also run under the host sanitizers)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

struct Line {
    RacelineSpec sp;
    std::vector<double> q, w;   // [M][2], [M]
    std::vector<double> alpha, xy, kappa, vx;
    double length = 0.0, lap_time = 0.0;
};

static std::vector<double> momentum(int iters)
{
    std::vector<double> beta((size_t)iters);
    double t = 1.0;
    for (int k = 0; k < iters; ++k) {
        const double t1 = (1.0 + std::sqrt(1.0 + 4.0 * (t * t))) / 2.0;
        beta[(size_t)k] = (t - 1.0) / t1;
        t = t1;
    }
    return beta;
}

static bool spec_ok(const RacelineSpec &sp, int M)
{
    if (sp.levels < 0 || sp.levels > kRacelineMaxLevels || sp.iters < 0 || sp.iters > kRacelineMaxIters) return false;
    if (M < 1 || M > kRacelineMaxPoints || M % (1 << sp.levels) || M / (1 << sp.levels) < 8) return false;
    for (double v : {sp.v_max, sp.a_lat, sp.a_accel, sp.a_brake})
        if (!(std::isfinite(v) && v > 0.0)) return false;
    return std::isfinite(sp.margin) && sp.margin >= 0.0;
}

// false: refused
static bool solve(Line &ln)
{
    const int M = (int)ln.w.size();
    const RacelineSpec &sp = ln.sp;
    if (!spec_ok(sp, M)) return false;
    for (double v : ln.q)
        if (!std::isfinite(v)) return false;
    for (double v : ln.w)
        if (!std::isfinite(v)) return false;
    const double *q = ln.q.data();
    std::vector<double> nx((size_t)M), ny((size_t)M), b((size_t)M), alpha((size_t)M, 0.0), y((size_t)M, 0.0);
    for (int i = 0; i < M; ++i) {
        const int im = (i + M - 1) % M, ip = (i + 1) % M;
        if (!(rl_frame(q[2 * im], q[2 * im + 1], q[2 * ip], q[2 * ip + 1], ln.w[(size_t)i], sp.margin, nx[(size_t)i], ny[(size_t)i], b[(size_t)i]) > 0.0)) return false;
    }
    const std::vector<double> beta = momentum(sp.iters);
    std::vector<double> px((size_t)M), py((size_t)M), nxt((size_t)M);
    for (int lv = sp.levels; lv >= 0; --lv) {
        const int s = 1 << lv;
        if (lv < sp.levels) {
            nxt = alpha;
            for (int i = s; i < M; i += 2 * s) nxt[(size_t)i] = rl_prolong(alpha[(size_t)(i - s)], alpha[(size_t)((i + s) % M)], b[(size_t)i]);
            alpha = nxt;
        }
        for (int i = 0; i < M; i += s) y[(size_t)i] = alpha[(size_t)i];
        for (int k = 0; k < sp.iters; ++k) {
            for (int j = 0; j < M; j += s) rl_point(q[2 * j], q[2 * j + 1], y[(size_t)j], nx[(size_t)j], ny[(size_t)j], px[(size_t)j], py[(size_t)j]);
            for (int j = 0; j < M; j += s) {   // (read-old / write-new: p is this iteration's, y and alpha are the point's own)
                double sx[5], sy[5];
                for (int m = 0; m < 5; ++m) {
                    const int jj = ((j + (m - 2) * s) % M + M) % M;
                    sx[m] = px[(size_t)jj];
                    sy[m] = py[(size_t)jj];
                }
                rl_update(sx, sy, nx[(size_t)j], ny[(size_t)j], b[(size_t)j], beta[(size_t)k], y[(size_t)j], alpha[(size_t)j]);
            }
        }
    }
    for (int i = 0; i < M; ++i) rl_point(q[2 * i], q[2 * i + 1], alpha[(size_t)i], nx[(size_t)i], ny[(size_t)i], px[(size_t)i], py[(size_t)i]);
    std::vector<double> len((size_t)M), cum((size_t)M), kappa((size_t)M), c((size_t)M);
    for (int i = 0; i < M; ++i) {
        const int im = (i + M - 1) % M, ip = (i + 1) % M;
        len[(size_t)i] = rl_length(px[(size_t)i], py[(size_t)i], px[(size_t)ip], py[(size_t)ip]);
        kappa[(size_t)i] = rl_curvature(px[(size_t)im], py[(size_t)im], px[(size_t)i], py[(size_t)i], px[(size_t)ip], py[(size_t)ip]);
        if (rl_degenerate(len[(size_t)i], kappa[(size_t)i])) return false;
        c[(size_t)i] = rl_ceiling(kappa[(size_t)i], sp.v_max, sp.a_lat);
    }
    double L = 0.0;
    for (int i = 0; i < M; ++i) {
        cum[(size_t)i] = L;
        L += len[(size_t)i];
    }
    const double inf = std::numeric_limits<double>::infinity();
    std::vector<double> pre_f((size_t)M), suf_f((size_t)M), suf_g((size_t)M), pre_g((size_t)M), vx((size_t)M);
    double m = inf, g = inf;
    for (int i = 0; i < M; ++i) {
        pre_g[(size_t)i] = g;
        m = rl_min(m, rl_F(c[(size_t)i], cum[(size_t)i], sp.a_accel));
        g = rl_min(g, rl_G(c[(size_t)i], cum[(size_t)i], sp.a_brake));
        pre_f[(size_t)i] = m;
    }
    m = g = inf;
    for (int i = M - 1; i >= 0; --i) {
        suf_f[(size_t)i] = m;
        m = rl_min(m, rl_F(c[(size_t)i], cum[(size_t)i], sp.a_accel));
        g = rl_min(g, rl_G(c[(size_t)i], cum[(size_t)i], sp.a_brake));
        suf_g[(size_t)i] = g;
    }
    for (int i = 0; i < M; ++i)
        vx[(size_t)i] = rl_speed(c[(size_t)i], cum[(size_t)i], L, sp.a_accel, sp.a_brake, pre_f[(size_t)i], suf_f[(size_t)i], suf_g[(size_t)i], pre_g[(size_t)i]);
    double lap = 0.0;
    for (int i = 0; i < M; ++i) lap += rl_lap_term(len[(size_t)i], vx[(size_t)i], vx[(size_t)((i + 1) % M)]);
    ln.alpha = alpha;
    ln.xy.resize(2 * (size_t)M);
    for (int i = 0; i < M; ++i) {
        ln.xy[2 * (size_t)i] = px[(size_t)i];
        ln.xy[2 * (size_t)i + 1] = py[(size_t)i];
    }
    ln.kappa = kappa;
    ln.vx = vx;
    ln.length = L;
    ln.lap_time = lap;
    return true;
}

static Line ellipse(int M, int levels, int iters, double w)
{
    Line ln;
    ln.sp = RacelineSpec{levels, iters, 0.3, 8.0, 7.0, 7.0, 8.0};
    for (int i = 0; i < M; ++i) {
        const double phi = 6.283185307179586 * i / M, r = 1.0 + 0.2 * std::cos(3.0 * phi + 0.5);
        ln.q.push_back(12.0 * r * std::cos(phi));
        ln.q.push_back(7.0 * r * std::sin(phi));
        ln.w.push_back(w);
    }
    return ln;
}

static int self_check()
{
    const int sizes[][2] = {{8, 0}, {63, 0}, {64, 0}, {65, 0}, {32, 2}, {128, 4}, {512, 6}};
    double laps = 0.0;
    int n = 0;
    for (const auto &sz : sizes) {
        Line ln = ellipse(sz[0], sz[1], 20, 1.0), mid = ellipse(sz[0], sz[1], 0, 1.0), shut = ellipse(sz[0], sz[1], 20, 0.2);
        if (!solve(ln) || !solve(mid) || !solve(shut)) {
            std::printf("M %d: refused\n", sz[0]);
            return 1;
        }
        for (int i = 0; i < sz[0]; ++i) {
            if (!(std::fabs(ln.alpha[(size_t)i]) <= 0.7) || !(ln.vx[(size_t)i] > 0.0 && ln.vx[(size_t)i] <= 8.0) || !std::isfinite(ln.kappa[(size_t)i])) {
                std::printf("M %d: point %d out of its bounds\n", sz[0], i);
                return 1;
            }
            if (mid.alpha[(size_t)i] != 0.0 || shut.alpha[(size_t)i] != 0.0 || shut.xy[2 * (size_t)i] != shut.q[2 * (size_t)i] || shut.vx[(size_t)i] != mid.vx[(size_t)i]) {
                std::printf("M %d: point %d moved without room or iterations\n", sz[0], i);
                return 1;
            }
        }
        if (sz[0] >= 32 && !(ln.lap_time < mid.lap_time)) {
            std::printf("M %d: lap time %.6f, centre %.6f\n", sz[0], ln.lap_time, mid.lap_time);
            return 1;
        }
        laps += ln.lap_time;
        ++n;
    }
    Line bad = ellipse(36, 2, 5, 1.0);   // 36 / 4 = 9 stations, but 36 + 2 is no multiple of 4
    bad.q.push_back(0.0), bad.q.push_back(0.0), bad.w.push_back(1.0);
    bad.q.push_back(1.0), bad.q.push_back(0.0), bad.w.push_back(1.0);
    if (solve(bad)) {
        std::printf("a line of 38 points at levels 2 was not refused\n");
        return 1;
    }
    const double inf = std::numeric_limits<double>::infinity(), qnan = std::numeric_limits<double>::quiet_NaN();
    if (rl_degenerate(1.0, 0.0) || rl_degenerate(5e-324, -1.7976931348623157e308) || !rl_degenerate(0.0, 1.0) || !rl_degenerate(qnan, 1.0) || !rl_degenerate(1.0, qnan) ||
        !rl_degenerate(1.0, inf) || !rl_degenerate(1.0, -inf) || !rl_degenerate(1.0, rl_curvature(0.0, 0.0, 1.0, 0.0, 0.0, 0.0))) {
        std::printf("rl_degenerate: a wrong answer\n");   // (the last: p_{i+1} = p_{i-1}, kappa = 0 / 0)
        return 1;
    }
    std::printf("ok: %d lines, %.6f s\n", n, laps);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3) return self_check();
    std::FILE *f = std::fopen(argv[1], "rb"), *o = std::fopen(argv[2], "wb");
    int32_t T = 0;
    if (!f || !o || std::fread(&T, sizeof T, 1, f) != 1 || T < 0) return 2;
    for (int t = 0; t < T; ++t) {
        int32_t hdr[3];
        double sp[5];
        if (std::fread(hdr, sizeof hdr, 1, f) != 1 || std::fread(sp, sizeof sp, 1, f) != 1 || hdr[0] < 0 || hdr[0] > (1 << 20)) return 2;
        Line ln;
        ln.sp = RacelineSpec{hdr[1], hdr[2], sp[0], sp[1], sp[2], sp[3], sp[4]};
        const size_t M = (size_t)hdr[0];
        ln.q.resize(2 * M);
        ln.w.resize(M);
        if (M && (std::fread(ln.q.data(), sizeof(double), 2 * M, f) != 2 * M || std::fread(ln.w.data(), sizeof(double), M, f) != M)) return 2;
        const int32_t status = solve(ln) ? 0 : 1;
        if (std::fwrite(&status, sizeof status, 1, o) != 1) return 2;
        if (status) continue;
        const double tail[2] = {ln.length, ln.lap_time};
        if (std::fwrite(ln.alpha.data(), sizeof(double), M, o) != M || std::fwrite(ln.xy.data(), sizeof(double), 2 * M, o) != 2 * M ||
            std::fwrite(ln.kappa.data(), sizeof(double), M, o) != M || std::fwrite(ln.vx.data(), sizeof(double), M, o) != M || std::fwrite(tail, sizeof tail, 1, o) != 1)
            return 2;
    }
    std::fclose(f);
    return std::fclose(o) == 0 ? 0 : 2;
}
