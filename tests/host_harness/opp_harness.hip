// tests/host_harness/opp_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the opponent term's arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp, opp_* and mppi_cost_opp), for
// tests/test_opponents_host.py: the predictions, a candidate's samples through roll_candidate's xy hook and the planner's cost with
// the two terms are compared with the Python model (tests/opponents_ref.py) without a GPU.  The GPU tests hold the device
// instantiation (and the kernels around it) to the same model.  With -DOPP_HARNESS_MAIN the file is a stand-alone program that rolls
// and plans a few cars among opponents on a synthetic map and track (what the address and undefined-behaviour sanitizers are run on).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_rng.hpp"

using namespace f110;

namespace {

ScanConst map_of(const double *dt, int Hm, int W, double res, double ox, double oy, double oc, double os)
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
    return k;
}

// roll_candidate's xy hook on the host: the sample, and the position itself for the test
struct HostOppEmit {
    static constexpr bool kOn = false, kXY = true;
    const double *rows;
    const OppSpec *sp;
    int Ao, H;
    double *xy_out;   // [H][2] or null
    mutable double m;
    mutable int free;
    void operator()(int, const double *) const {}
    void xy(int h, double x, double y) const
    {
        opp_sample(rows, Ao, H, h, x, y, *sp, m, free);
        if (xy_out) {
            xy_out[2 * h] = x;
            xy_out[2 * h + 1] = y;
        }
    }
};

RollCar car_of(const double *s)
{
    RollCar car;
    for (int q = 0; q < 7; ++q) car.st[q] = s[q];
    car.b0 = s[7];
    car.b1 = s[8];
    car.cnt = (int)s[9];
    return car;
}

OppSpec opp_of(const int *oi, const double *od)
{
    OppSpec o{};
    o.mode = oi[0];
    o.radius = od[0], o.max_range = od[1], o.w_hit = od[2], o.w_near = od[3], o.near_ref = od[4];
    return o;
}

void predict_rows(const OppSpec &os, const double *cols, int nseg, int closed, double L, const double *start, const double *opp, int Ao, int m, int H,
                  int repeat, double dt, double *pred)
{
    for (int n = 0; n < m; ++n)
        for (int o = 0; o < Ao; ++o)
            opp_predict_row(os, cols, nseg, closed, L, start[10 * (size_t)n], start[10 * (size_t)n + 1], opp + ((size_t)n * Ao + o) * 4, H, repeat, dt,
                            pred + ((size_t)n * Ao + o) * H * 2);
}

}   // namespace

extern "C" {

// the rollout with the term.  map / track as mppi_harness.hip takes them (cols null: CV only).  ri = K, H, repeat, per_agent,
// integrator; oi = mode; od = radius, max_range, w_hit, w_near, near_ref.  start [m][10], params [m][18], actions [K][H][2] or
// [m][K][H][2], opp [m][Ao][4].  Out: pred [m][Ao][H][2], opp_raw [m][K][2], opp32 [m][K][2], xy [m][K][H][2], roll [m][K][2] = ALIVE,
// MIN_CLEAR.
void hh_opp_rollout(const double *dt, int Hm, int W, double res, double ox, double oy, double oc, double os, const double *cols, int nseg, int closed,
                    double L, const int *ri, double margin, const int *oi, const double *od, double time_step, double lidar_dist, const double *start,
                    const double *params, const double *actions, const double *opp, int Ao, int m, double *pred, double *opp_raw, float *opp32,
                    double *xy, double *roll)
{
    const ScanConst k = map_of(dt, Hm, W, res, ox, oy, oc, os);
    const int K = ri[0], H = ri[1], repeat = ri[2], per_agent = ri[3], integrator = ri[4];
    RollSpec rs{};
    rs.K = K, rs.H = H, rs.repeat = repeat, rs.layout = per_agent ? ROLL_PER_AGENT : ROLL_SHARED, rs.frame = ROLL_FRAME_EGO, rs.margin = margin;
    const OppSpec osp = opp_of(oi, od);
    predict_rows(osp, cols, nseg, closed, L, start, opp, Ao, m, H, repeat, time_step, pred);
    for (int n = 0; n < m; ++n) {
        VehicleParams vp;
        for (int q = 0; q < NPARAMS; ++q) vp.v[q] = params[(size_t)n * NPARAMS + q];
        for (int kk = 0; kk < K; ++kk) {
            const size_t G = (size_t)n * K + kk;
            RollCar car = car_of(start + 10 * (size_t)n);
            const double *act = actions + (per_agent ? G : (size_t)kk) * H * 2;
            int alive;
            double min_clear;
            RollFrame fr{};
            const HostOppEmit emit{pred + (size_t)n * Ao * H * 2, &osp, Ao, H, xy + G * H * 2, INFINITY, H};
            roll_candidate(rs, k, vp, time_step, integrator, lidar_dist, car, act, fr, alive, min_clear, emit);
            opp_raw[2 * G] = emit.m, opp_raw[2 * G + 1] = (double)emit.free;
            opp32[2 * G] = (float)emit.m, opp32[2 * G + 1] = (float)emit.free;
            roll[2 * G] = (double)alive, roll[2 * G + 1] = min_clear;
        }
    }
}

// the planner with the term: mppi_harness.hip's hh_mppi plus oi / od and opp [m][Ao][4]; also opp_raw [m][K][2] and pred
void hh_opp_mppi(const double *dt, int Hm, int W, double res, double ox, double oy, double oc, double os, const double *cols, int nseg, int closed, double L,
                 const int *ints, const double *dbl, const int *oi, const double *od, double time_step, int integrator, double lidar_dist,
                 const double *start, const double *params, const int *fresh, const double *opp, int Ao, int m, double *nominal, uint64_t *streams,
                 double *actions, float *info, double *cand, double *cost, double *weight, double *raw, double *opp_raw, double *pred)
{
    const ScanConst k = map_of(dt, Hm, W, res, ox, oy, oc, os);
    MppiSpec sp{};
    sp.K = ints[0], sp.H = ints[1], sp.repeat = ints[2], sp.shift = ints[3];
    sp.margin = dbl[0], sp.sigma_steer = dbl[1], sp.sigma_speed = dbl[2], sp.steer_min = dbl[3], sp.steer_max = dbl[4];
    sp.speed_min = dbl[5], sp.speed_max = dbl[6], sp.lambda = dbl[7], sp.w_dead = dbl[8], sp.w_clear = dbl[9], sp.w_progress = dbl[10];
    sp.w_lat = dbl[11], sp.clear_ref = dbl[12], sp.v_init = dbl[13];
    const OppSpec osp = opp_of(oi, od);
    const int K = sp.K, H = sp.H;
    const bool track = cols && mppi_needs_track(sp);
    const RollSpec rs = mppi_roll_spec(sp);
    const ZigTables zt = {kZigK, kZigW, kZigF};
    std::vector<U128> ja(kMppiJumps), jg(kMppiJumps);
    mppi_jump_table(ja.data(), jg.data());
    std::vector<double> w(K), u(2 * (size_t)H);
    predict_rows(osp, cols, nseg, closed, L, start, opp, Ao, m, H, sp.repeat, time_step, pred);
    for (int n = 0; n < m; ++n) {
        VehicleParams vp;
        for (int q = 0; q < NPARAMS; ++q) vp.v[q] = params[(size_t)n * NPARAMS + q];
        const double *s = start + 10 * (size_t)n;
        double *U = nominal + (size_t)n * H * 2, *V = cand + (size_t)n * K * H * 2, *c = cost + (size_t)n * K;
        uint64_t *st = streams + 4 * (size_t)n;
        double s0 = 0.0, lat0 = 0.0;
        if (track) roll_project(cols, nseg, s[0], s[1], s0, lat0);
        for (int kk = 0; kk < K; ++kk) {
            const size_t G = (size_t)n * K + kk;
            double *row = V + (size_t)kk * H * 2;
            mppi_sample_row(sp, U, fresh && fresh[n] == 0, kk, st, ja[kk], jg[kk], zt, row);
            RollCar car = car_of(s);
            int alive;
            double min_clear, progress = 0.0, lat = 0.0;
            RollFrame fr{};
            const HostOppEmit emit{pred + (size_t)n * Ao * H * 2, &osp, Ao, H, nullptr, INFINITY, H};
            roll_candidate(rs, k, vp, time_step, integrator, lidar_dist, car, row, fr, alive, min_clear, emit);
            if (track) {
                double s1;
                roll_project(cols, nseg, car.st[0], car.st[1], s1, lat);
                progress = roll_progress(s0, s1, closed, L);
            }
            // the kernels' two parts: the rollout's lane leaves the map's and the opponents' terms, the track's follow
            c[kk] = mppi_cost_track(sp, mppi_cost_opp(osp, mppi_cost_map(sp, alive, min_clear), H, emit.free, emit.m), progress, lat);
            double *r = raw + G * 4;
            r[0] = (double)alive, r[1] = min_clear, r[2] = progress, r[3] = lat;
            opp_raw[2 * G] = emit.m, opp_raw[2 * G + 1] = (double)emit.free;
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

}

#ifdef OPP_HARNESS_MAIN
// mppi_harness.hip's room and square track; two cars (one with a NaN state) among 0, 1 and 3 opponents (one parked ahead of the first
// car, one NaN, one out of range), both modes, K = 1, 5 and 70, H = 1 and 6, repeat 3: a parked opponent ahead must be hit
int main()
{
    const int Hm = 40, W = 60;
    const double res = 0.1;
    std::vector<double> dt((size_t)Hm * W);
    for (int r = 0; r < Hm; ++r)
        for (int c = 0; c < W; ++c) dt[(size_t)r * W + c] = std::min(std::min(r, Hm - 1 - r), std::min(c, W - 1 - c)) * res;
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
    const int m = 2;
    std::vector<double> start(10 * (size_t)m, 0.0), params(NPARAMS * (size_t)m);
    for (int n = 0; n < m; ++n)
        for (int q = 0; q < NPARAMS; ++q) params[(size_t)n * NPARAMS + q] = P[q];
    start[0] = 1.0, start[1] = 1.0, start[3] = 2.0, start[9] = 2.0;
    start[10] = NAN, start[11] = 2.0;
    int hits = 0;
    for (int variant = 0; variant < 36; ++variant) {
        const int Ks[3] = {1, 5, 70}, Aos[3] = {0, 1, 3};
        const int K = Ks[variant % 3], H = (variant / 3 & 1) ? 6 : 1, mode = variant / 6 & 1, Ao = Aos[variant / 12];
        std::vector<double> opp((size_t)m * std::max(Ao, 1) * 4, 0.0);
        for (int n = 0; n < m; ++n) {
            double *o = opp.data() + (size_t)n * Ao * 4;
            if (Ao >= 1) o[0] = 1.3, o[1] = 1.0, o[2] = 0.0, o[3] = 0.0;           // parked 0.3 m ahead of car 0
            if (Ao >= 3) {
                o[4] = NAN, o[5] = 1.0, o[6] = 1.0;
                o[8] = 30.0, o[9] = 2.0, o[10] = -2.0, o[11] = 1.0;                // beyond max_range
            }
        }
        const int oi[1] = {mode};
        const double od[5] = {0.4, 10.0, 2.0, 1.5, 1.0};
        {
            const int ri[5] = {K, H, 3, 0, 1 + (variant & 1)};
            std::vector<double> actions((size_t)K * H * 2), pred((size_t)m * std::max(Ao, 1) * H * 2), oraw((size_t)m * K * 2), xy((size_t)m * K * H * 2), roll((size_t)m * K * 2);
            std::vector<float> o32((size_t)m * K * 2);
            for (size_t q = 0; q < actions.size(); ++q) actions[q] = (q & 1) ? 2.0 : 0.02 * (double)(q % 7) - 0.06;
            hh_opp_rollout(dt.data(), Hm, W, res, -0.5, -0.25, 1.0, 0.0, cols.data(), nseg, 1, cum, ri, 0.15, oi, od, 0.01, 0.275, start.data(),
                           params.data(), actions.data(), opp.data(), Ao, m, pred.data(), oraw.data(), o32.data(), xy.data(), roll.data());
            for (int kk = 0; kk < K; ++kk) {
                if (Ao == 0 && !(oraw[2 * kk] == INFINITY && oraw[2 * kk + 1] == (double)H)) return 1;
                if (Ao >= 1 && !(oraw[2 * kk] < 0.4 && oraw[2 * kk + 1] == 0.0)) return 2;        // 0.3 m away at most from the first sample on
                if (!(oraw[2 * ((size_t)K + kk)] == INFINITY)) return 3;                          // the NaN car measures nothing
                hits += Ao >= 1;
            }
            if (Ao >= 3 && !(pred[(size_t)1 * H * 2] != pred[(size_t)1 * H * 2] && pred[(size_t)2 * H * 2] != pred[(size_t)2 * H * 2])) return 4;
        }
        {
            const int ints[4] = {K, H, 3, variant & 1};
            const double dbl[14] = {0.15, 0.2, 1.5, -0.4, 0.4, 0.5, 6.0, 0.7, 1.0, 5.0, mode ? 3.0 : 0.0, mode ? 0.5 : 0.0, 0.6, 2.0};
            std::vector<double> nominal((size_t)m * H * 2), actions(2 * (size_t)m), cand((size_t)m * K * H * 2), cost((size_t)m * K), weight((size_t)m * K),
                raw((size_t)m * K * 4), oraw((size_t)m * K * 2), pred((size_t)m * std::max(Ao, 1) * H * 2);
            for (size_t q = 0; q < nominal.size(); ++q) nominal[q] = (q & 1) ? 2.0 : 0.0;
            std::vector<uint64_t> streams(4 * (size_t)m);
            for (int n = 0; n < m; ++n) pcg64_seed_from_u64(2000 + (uint64_t)n, &streams[4 * (size_t)n]);
            std::vector<float> info(4 * (size_t)m);
            hh_opp_mppi(dt.data(), Hm, W, res, -0.5, -0.25, 1.0, 0.0, cols.data(), nseg, 1, cum, ints, dbl, oi, od, 0.01, 1, 0.275, start.data(), params.data(),
                        nullptr, opp.data(), Ao, m, nominal.data(), streams.data(), actions.data(), info.data(), cand.data(), cost.data(), weight.data(),
                        raw.data(), oraw.data(), pred.data());
            for (int kk = 0; kk < K; ++kk)
                if (Ao >= 1 && !(cost[kk] >= 2.0 * (double)H)) return 5;                          // w_hit * (H - 0) at least
            if (!(actions[0] >= -0.4 && actions[0] <= 0.4 && actions[1] >= 0.5 && actions[1] <= 6.0)) return 6;
        }
    }
    printf("opp harness: ok (%d hits)\n", hits);
    return hits > 0 ? 0 : 7;
}
#endif
