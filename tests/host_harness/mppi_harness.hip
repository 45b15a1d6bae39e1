// tests/host_harness/mppi_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the planner's arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp and f110_rng.hpp, mppi_*), for
// tests/test_mppi_host.py: the jump of a candidate's generator, its draws, the clamp, roll_candidate as it is, the two projections,
// the cost, the weights and the update are compared with the Python model (tests/mppi_ref.py) without a GPU.  The GPU tests hold the
// device instantiation (and the kernels around it) to the same model.  With -DMPPI_HARNESS_MAIN the file is a stand-alone program
// that plans for a few cars on a synthetic map and track (what the address and undefined-behaviour sanitizers are run on).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_rng.hpp"

using namespace f110;

extern "C" {

// map: dt [Hm][W] with the yaml's resolution and origin (cos, sin of its yaw).  track: cols [7][nseg], or null (then both track
// weights are 0).  ints = k, horizon, repeat, shift; dbl = margin, sigma_steer, sigma_speed, steer_min, steer_max, speed_min,
// speed_max, lambda, w_dead, w_clear, w_progress, w_lat, clear_ref, v_init.  start [m][10], params [m][18], fresh [m] (step counts)
// or null; nominal [m][H][2] and streams [m][4] in and out; actions [m][2], info [m][4], cand [m][K][H][2], cost [m][K], weight
// [m][K], raw [m][K][4] = ALIVE, MIN_CLEAR, PROGRESS, END_LAT.  The caller has validated the settings.
void hh_mppi(const double *dt, int Hm, int W, double res, double ox, double oy, double oc, double os, const double *cols, int nseg, int closed,
             double L, const int *ints, const double *dbl, double time_step, int integrator, double lidar_dist, const double *start,
             const double *params, const int *fresh, int m, double *nominal, uint64_t *streams, double *actions, float *info, double *cand,
             double *cost, double *weight, double *raw)
{
    ScanConst k{};
    k.table = dt;
    k.table_rm = dt;
    k.height = Hm;
    k.width = W;
    k.row_bytes = W * 8;
    k.res = res;
    k.inv_res = 1.0 / res;
    k.orig_x = ox;
    k.orig_y = oy;
    k.orig_c = oc;
    k.orig_s = os;
    k.w_res = W * res;
    k.h_res = Hm * res;
    k.oob_value = dt[(size_t)Hm * W - 1];
    MppiSpec sp{};
    sp.K = ints[0], sp.H = ints[1], sp.repeat = ints[2], sp.shift = ints[3];
    sp.margin = dbl[0], sp.sigma_steer = dbl[1], sp.sigma_speed = dbl[2], sp.steer_min = dbl[3], sp.steer_max = dbl[4];
    sp.speed_min = dbl[5], sp.speed_max = dbl[6], sp.lambda = dbl[7], sp.w_dead = dbl[8], sp.w_clear = dbl[9], sp.w_progress = dbl[10];
    sp.w_lat = dbl[11], sp.clear_ref = dbl[12], sp.v_init = dbl[13];
    const int K = sp.K, H = sp.H;
    const bool track = cols && mppi_needs_track(sp);
    const RollSpec rs = mppi_roll_spec(sp);
    const ZigTables zt = {kZigK, kZigW, kZigF};
    std::vector<U128> ja(kMppiJumps), jg(kMppiJumps);
    mppi_jump_table(ja.data(), jg.data());
    std::vector<double> w(K), u(2 * (size_t)H);
    for (int n = 0; n < m; ++n) {
        VehicleParams vp;
        for (int q = 0; q < NPARAMS; ++q) vp.v[q] = params[(size_t)n * NPARAMS + q];
        const double *s = start + 10 * (size_t)n;
        double *U = nominal + (size_t)n * H * 2, *V = cand + (size_t)n * K * H * 2, *c = cost + (size_t)n * K;
        uint64_t *st = streams + 4 * (size_t)n;
        double s0 = 0.0, lat0 = 0.0;
        if (track) roll_project(cols, nseg, s[0], s[1], s0, lat0);
        for (int kk = 0; kk < K; ++kk) {
            double *row = V + (size_t)kk * H * 2;
            mppi_sample_row(sp, U, fresh && fresh[n] == 0, kk, st, ja[kk], jg[kk], zt, row);
            RollCar car;
            for (int q = 0; q < 7; ++q) car.st[q] = s[q];
            car.b0 = s[7];
            car.b1 = s[8];
            car.cnt = (int)s[9];
            int alive;
            double min_clear, progress = 0.0, lat = 0.0;
            RollFrame fr{};
            roll_candidate(rs, k, vp, time_step, integrator, lidar_dist, car, row, fr, alive, min_clear, RollEmitNone());
            if (track) {
                double s1;
                roll_project(cols, nseg, car.st[0], car.st[1], s1, lat);
                progress = roll_progress(s0, s1, closed, L);
            }
            c[kk] = mppi_cost(sp, alive, min_clear, progress, lat);
            double *r = raw + ((size_t)n * K + kk) * 4;
            r[0] = (double)alive, r[1] = min_clear, r[2] = progress, r[3] = lat;
        }
        double beta, eta, q2;
        int best;
        mppi_min(c, K, beta, best);
        for (int kk = 0; kk < K; ++kk) weight[(size_t)n * K + kk] = w[kk] = mppi_weight(sp, c[kk], beta, kk);
        mppi_norms(w.data(), K, eta, q2);
        for (int t = 0; t < 2 * H; ++t) u[t] = mppi_blend(w.data(), V, K, H, t, eta);
        for (int t = 0; t < 2 * H; ++t) mppi_store_nominal(sp, U, t, u[t]);
        actions[2 * (size_t)n] = u[0];
        actions[2 * (size_t)n + 1] = u[1];
        mppi_info(beta, c[0], eta, q2, best, info + 4 * (size_t)n);
        const U128 s1 = pcg_jump(U128{st[0], st[1]}, U128{st[2], st[3]}, ja[kMppiJumps - 1], jg[kMppiJumps - 1]);
        st[0] = s1.hi;
        st[1] = s1.lo;
    }
}

// how many of the n draws from the stream {state.hi, state.lo, inc.hi, inc.lo} took the wedge test (out[0]) and the tail loop
// (out[1]): what the test uses to find a seed whose draws reach both
void hh_mppi_branches(const uint64_t *stream, int n, int *out)
{
    const ZigTables zt = {kZigK, kZigW, kZigF};
    const U128 inc = {stream[2], stream[3]};
    U128 st = {stream[0], stream[1]};
    out[0] = out[1] = 0;
    for (int d = 0; d < n; ++d) {
        for (;;) {
            st = pcg_step(st, inc);
            const uint64_t r = pcg_output(st);
            const ZigAttempt z = zig_attempt(r, st, inc, zt);
            const int idx = (int)(r & 0xff);
            const uint64_t rabs = (r >> 9) & 0x000fffffffffffffULL;
            if (rabs >= zt.k[idx]) out[idx == 0 ? 1 : 0] += 1;
            for (int q = 1; q < z.len; ++q) st = pcg_step(st, inc);
            if (z.emit) break;
        }
    }
}

}

#ifdef MPPI_HARNESS_MAIN
// a 40 x 60 cell room whose clearance is the distance to the nearest wall, a square track inside it, three cars (one starts outside
// the map, one with a NaN state), K = 1, 5 and 70 candidates of H = 1 and 6 actions held 3 steps, with and without the track weights,
// shift 0 and 1, both integrators, three calls in a row
int main()
{
    const int Hm = 40, W = 60;
    const double res = 0.1;
    std::vector<double> dt((size_t)Hm * W);
    for (int r = 0; r < Hm; ++r)
        for (int c = 0; c < W; ++c) {
            const int e = std::min(std::min(r, Hm - 1 - r), std::min(c, W - 1 - c));
            dt[(size_t)r * W + c] = e * res;
        }
    const double px[4] = {1.0, 5.0, 5.0, 1.0}, py[4] = {1.0, 1.0, 3.0, 3.0};
    const int nseg = 4;
    std::vector<double> cols(7 * (size_t)nseg);
    double cum = 0.0;
    for (int q = 0; q < nseg; ++q) {
        const double dx = px[(q + 1) % 4] - px[q], dy = py[(q + 1) % 4] - py[q], l2 = dx * dx + dy * dy, len = sqrt(l2);
        const double v[7] = {px[q], py[q], dx, dy, l2, len, cum};
        for (int c = 0; c < 7; ++c) cols[(size_t)c * nseg + q] = v[c];
        cum += len;
    }
    const double P[NPARAMS] = {1.0489, 4.718, 5.4562, 0.15875, 0.17145, 0.074, 3.74, 0.04712, -0.4189, 0.4189, -3.2, 3.2, 7.319, 9.51, -5.0, 20.0, 0.31, 0.58};
    const int m = 3;
    std::vector<double> start(10 * (size_t)m, 0.0), params(NPARAMS * (size_t)m);
    for (int n = 0; n < m; ++n)
        for (int q = 0; q < NPARAMS; ++q) params[(size_t)n * NPARAMS + q] = P[q];
    start[0] = 1.0, start[1] = 1.0, start[3] = 2.0, start[9] = 2.0;
    start[10] = -3.0, start[11] = 9.0, start[13] = 0.2, start[19] = 1.0;
    start[20] = NAN, start[21] = 2.0;
    double moved = 0.0;
    for (int variant = 0; variant < 24; ++variant) {
        const int Ks[3] = {1, 5, 70};
        const int K = Ks[variant % 3], H = (variant / 3 & 1) ? 6 : 1, shift = variant / 6 & 1, with_track = variant / 12 & 1;
        const int ints[4] = {K, H, 3, shift};
        const double dbl[14] = {0.15, 0.2, 1.5, -0.4, 0.4, 0.5, 6.0, 0.7, 1.0, 5.0, with_track ? 3.0 : 0.0, with_track ? 0.5 : 0.0, 0.6, 2.0};
        std::vector<double> nominal((size_t)m * H * 2), actions(2 * (size_t)m), cand((size_t)m * K * H * 2), cost((size_t)m * K), weight((size_t)m * K), raw((size_t)m * K * 4);
        for (size_t q = 0; q < nominal.size(); ++q) nominal[q] = (q & 1) ? 2.0 : 0.0;
        std::vector<uint64_t> streams(4 * (size_t)m);
        for (int n = 0; n < m; ++n) pcg64_seed_from_u64(1000 + (uint64_t)n, &streams[4 * (size_t)n]);
        std::vector<float> info(4 * (size_t)m);
        const int fresh[3] = {1, 0, 1};
        for (int call = 0; call < 3; ++call) {
            hh_mppi(dt.data(), Hm, W, res, -0.5, -0.25, 1.0, 0.0, cols.data(), nseg, 1, cum, ints, dbl, 0.01, 1 + (variant & 1), 0.275, start.data(),
                    params.data(), call == 0 ? fresh : nullptr, m, nominal.data(), streams.data(), actions.data(), info.data(), cand.data(),
                    cost.data(), weight.data(), raw.data());
            for (int n = 0; n < m; ++n) {
                double sum = 0.0;
                for (int kk = 0; kk < K; ++kk) sum += weight[(size_t)n * K + kk];
                if (!(sum >= 1.0 && sum <= (double)K)) return 1;                                 // the winner's weight is exp(0) = 1
                if (!(actions[2 * n] >= -0.4 && actions[2 * n] <= 0.4 && actions[2 * n + 1] >= 0.5 && actions[2 * n + 1] <= 6.0)) return 2;
                if (!(info[4 * n + 3] >= 0.0f && info[4 * n + 3] < (float)K)) return 3;
            }
            if (weight[(size_t)2 * K] != 1.0) return 4;                                          // the NaN car keeps its nominal: w = (1, 0, ...)
            moved = std::max(moved, std::fabs(actions[0]));
        }
    }
    printf("mppi harness: ok (largest steer %g)\n", moved);
    return moved > 0.0 ? 0 : 5;
}
#endif
