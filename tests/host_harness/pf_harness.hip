// tests/host_harness/pf_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the particle filter's arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp and f110_rng.hpp, pf_*), for
// tests/test_particle_filter_host.py: the sub-streams' jumps and draws, the resampling, the motion, the scan's ray march at every
// particle's lidar pose, the beam terms, the weights and the estimate are compared with the Python model
// (tests/particle_filter_ref.py) without a GPU.  The stages are chained the way k_pf_plan, k_pf_move, k_pf_sense and k_pf_update
// chain them.  The GPU tests hold the device instantiation (and the kernels around it) to the same model.  With -DPF_HARNESS_MAIN
// the file is a stand-alone program that localises a few cars in a synthetic room (what the address and undefined-behaviour
// sanitizers are run on).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_rng.hpp"

using namespace f110;

extern "C" {

// map: dt [Hm][W] with the yaml's resolution and origin (cos, sin of its yaw); the scan's tables and constants as hh_scan takes them.
// ints = particles, n_beams, beam_first, beam_stride; dbl = sigma_x, sigma_y, sigma_theta, init_x, init_y, init_theta, sigma_hit,
// clip, squash, resample_frac.  poses [m][3], scans [m][B], fresh [m] (step counts) or null; particles [m][P][3], weights [m][P],
// last [m][3] and streams [m][4] in and out; pose [m][3], info [m][4], noise [m][P][3], anc [m][P], expect [m][P][B'], logw [m][P].
// The caller has validated the settings.
void hh_pf(const double *dt, int Hm, int W, double res, double ox, double oy, double oc, double os, const double *sines, const double *cosines,
           int theta_dis, int B, double fov, double eps, double max_range, const int *ints, const double *dbl, double lidar_dist,
           const double *poses, const double *scans, const int *fresh, int m, double *particles, double *weights, double *last, uint64_t *streams,
           double *pose, float *info, double *noise, int *anc, double *expect, double *logw)
{
    ScanConst k{};
    std::vector<double2> cs(theta_dis);
    for (int i = 0; i < theta_dis; ++i) cs[i] = make_double2(cosines[i], sines[i]);
    k.cs = cs.data();
    k.table = dt;
    k.table_rm = dt;
    k.height = Hm;
    k.width = W;
    k.row_bytes = W * 8;
    k.theta_dis = theta_dis;
    k.num_beams = B;
    k.res = res;
    k.inv_res = 1.0 / res;
    k.orig_x = ox;
    k.orig_y = oy;
    k.orig_c = oc;
    k.orig_s = os;
    k.w_res = W * res;
    k.h_res = Hm * res;
    k.oob_value = dt[(size_t)Hm * W - 1];
    k.eps = eps;
    k.max_range = max_range;
    k.fov = fov;
    k.theta_inc = theta_dis * (fov / (B - 1)) / (2. * kPi);
    const double g = 64.0 * (double)B * 2.2737367544323206e-13;
    k.dir_guard = g > 1e-8 ? g : 1e-8;
    k.inv_theta_dis = 1.0 / (double)theta_dis;
    PfSpec sp{};
    sp.P = ints[0], sp.B = ints[1], sp.beam_first = ints[2], sp.beam_stride = ints[3];
    sp.sigma_x = dbl[0], sp.sigma_y = dbl[1], sp.sigma_theta = dbl[2], sp.init_x = dbl[3], sp.init_y = dbl[4], sp.init_theta = dbl[5];
    sp.sigma_hit = dbl[6], sp.clip = dbl[7], sp.squash = dbl[8], sp.resample_frac = dbl[9];
    const int P = sp.P, Bp = sp.B;
    const ZigTables zt = {kZigK, kZigW, kZigF};
    std::vector<U128> ja(kPfJumps), jg(kPfJumps);
    pf_jump_table(ja.data(), jg.data());
    std::vector<double> C(P), Xn(3 * (size_t)P), term(Bp), w(P), prod(5 * (size_t)P);
    for (int n = 0; n < m; ++n) {
        double *X = particles + (size_t)n * P * 3, *Wn = weights + (size_t)n * P, *la = last + 3 * (size_t)n;
        uint64_t *st = streams + 4 * (size_t)n;
        const double x = poses[3 * (size_t)n], y = poses[3 * (size_t)n + 1], th = poses[3 * (size_t)n + 2];
        // k_pf_plan
        PfPlan pl;
        pl.fresh = (fresh && fresh[n] == 0) ? 1 : 0;
        pl.u = pf_uniform(st);
        pl.resample = (!pl.fresh && pf_decide(sp, pf_ess(Wn, P))) ? 1 : 0;
        pf_cumulate(Wn, P, C.data());
        pl.ctot = C[P - 1];
        pf_odometry(la, x, y, th, pl.a, pl.b, pl.dth);
        // k_pf_move and k_pf_sense
        for (int p = 0; p < P; ++p) {
            const size_t G = (size_t)n * P + p;
            double *e = noise + 3 * G, *Xp = Xn.data() + 3 * (size_t)p;
            pf_normals(st, ja[p + 1], jg[p + 1], zt, e);
            int a = p;
            if (pl.fresh) {
                pf_fresh(sp, x, y, th, e, Xp);
            } else {
                if (pl.resample) a = pf_ancestor(C.data(), P, p, pl.u, pl.ctot);
                pf_move(sp, pl.a, pl.b, pl.dth, X + 3 * (size_t)a, e, Xp);
            }
            anc[G] = a;
            double lp[3];
            pf_lidar_pose(Xp, lidar_dist, lp);
            const double start = scan_start_index(k, lp[2]);
            int r0, c0, nl;
            const double d0 = sample_distance<LAYOUT_ROWMAJOR, false, false>(k, nullptr, lp[0], lp[1], r0, c0);
            for (int jb = 0; jb < Bp; ++jb) {
                const int beam = sp.beam_first + jb * sp.beam_stride;
                const double2 d = cs[beam_dir_index(k, start, beam)];
                const double r = march_from_first<LAYOUT_ROWMAJOR, false, false>(k, nullptr, lp[0], lp[1], d.x, d.y, d0, r0, c0, nl);
                expect[G * Bp + jb] = r;
                term[jb] = pf_term(sp, scans[(size_t)n * B + beam], r);
            }
            logw[G] = pf_logw(sp, term.data(), Bp);
        }
        if (pl.fresh | pl.resample)
            for (int p = 0; p < P; ++p) Wn[p] = 1.0 / (double)P;
        std::copy(Xn.begin(), Xn.end(), X);
        // k_pf_update
        const double *L = logw + (size_t)n * P;
        const double Lmax = pf_max(L, P);
        for (int p = 0; p < P; ++p) w[p] = pf_unnorm(Wn[p], L[p], Lmax);
        const double eta = pf_sum(w.data(), P);
        double *sx = prod.data(), *sy = sx + P, *ss = sy + P, *sc = ss + P, *sq = sc + P;
        for (int p = 0; p < P; ++p) {
            const double v = pf_norm(w[p], eta, P);
            double c, s;
            cos_sin(X[3 * p + 2], c, s);
            Wn[p] = v;
            sx[p] = v * X[3 * p];
            sy[p] = v * X[3 * p + 1];
            ss[p] = v * s;
            sc[p] = v * c;
            sq[p] = v * v;
        }
        const double xh = pf_sum(sx, P), yh = pf_sum(sy, P), S = pf_sum(ss, P), Cc = pf_sum(sc, P), q = pf_sum(sq, P);
        for (int p = 0; p < P; ++p) sx[p] = pf_spread_term(Wn[p], X[3 * p], X[3 * p + 1], xh, yh);
        const double spread = pf_sum(sx, P);
        pose[3 * (size_t)n] = xh;
        pose[3 * (size_t)n + 1] = yh;
        pose[3 * (size_t)n + 2] = atan2(S, Cc);
        pf_info(q, spread, xh, yh, x, y, pl.resample, info + 4 * (size_t)n);
        la[0] = x;
        la[1] = y;
        la[2] = th;
        pf_stream_advance(st, ja[kPfJumps - 1], jg[kPfJumps - 1]);
    }
}

}

#ifdef PF_HARNESS_MAIN
// a 40 x 60 cell room whose clearance is the distance to the nearest wall, three cars (one whose cloud starts outside the map), P = 1,
// 7 and 70 particles of B' = 1, 5 and 33 beams, with and without truncation, every resampling outcome, four calls in a row with the
// cars moving (the first one fresh), a NaN in one scan
int main()
{
    const int Hm = 40, W = 60, theta_dis = 2000, B = 108;
    const double res = 0.1, fov = 4.7;
    std::vector<double> dt((size_t)Hm * W);
    for (int r = 0; r < Hm; ++r)
        for (int c = 0; c < W; ++c) {
            const int e = std::min(std::min(r, Hm - 1 - r), std::min(c, W - 1 - c));
            dt[(size_t)r * W + c] = e * res;
        }
    std::vector<double> sines(theta_dis), cosines(theta_dis);
    for (int i = 0; i < theta_dis; ++i) {
        const double a = 2.0 * kPi * i / (theta_dis - 1);
        sines[i] = sin(a);
        cosines[i] = cos(a);
    }
    const int m = 3;
    double worst = 0.0;
    for (int variant = 0; variant < 18; ++variant) {
        const int Ps[3] = {1, 7, 70}, Bs[3] = {1, 5, 33};
        const int P = Ps[variant % 3], Bp = Bs[variant / 3 % 3];
        const int ints[4] = {P, Bp, 2, Bp > 1 ? (B - 3) / (Bp - 1) : 1};
        const double fracs[3] = {0.0, 0.5, 2.0};
        const double dbl[10] = {0.03, 0.02, 0.01, 0.1, 0.1, 0.05, 0.1, variant / 9 ? INFINITY : 3.0, 2.0, fracs[variant % 3]};
        std::vector<double> poses(3 * (size_t)m), scans((size_t)m * B, 1.0), particles(3 * (size_t)m * P, 0.0), weights((size_t)m * P, 1.0 / P), last(3 * (size_t)m, 0.0);
        std::vector<double> pose(3 * (size_t)m), noise(3 * (size_t)m * P), expect((size_t)m * P * Bp), logw((size_t)m * P);
        std::vector<int> anc((size_t)m * P);
        std::vector<float> info(4 * (size_t)m);
        std::vector<uint64_t> streams(4 * (size_t)m);
        for (int n = 0; n < m; ++n) pcg64_seed_from_u64(2000 + (uint64_t)n, &streams[4 * (size_t)n]);
        for (int call = 0; call < 4; ++call) {
            for (int n = 0; n < m; ++n) {
                poses[3 * n] = (n == 2 ? -4.0 : 1.0 + n) + 0.05 * call;
                poses[3 * n + 1] = 1.0 + 0.5 * n;
                poses[3 * n + 2] = n == 1 ? 6.2 + 0.05 * call : 0.3 * call;   // car 1 turns across the yaw wrap
                if (poses[3 * n + 2] > kTwoPi) poses[3 * n + 2] -= kTwoPi;
            }
            scans[5] = call == 2 ? NAN : 1.0;
            const int fresh[3] = {0, 0, 0};
            hh_pf(dt.data(), Hm, W, res, -0.5, -0.25, 1.0, 0.0, sines.data(), cosines.data(), theta_dis, B, fov, 1e-4, 30.0, ints, dbl, 0.275, poses.data(),
                  scans.data(), call == 0 ? fresh : nullptr, m, particles.data(), weights.data(), last.data(), streams.data(), pose.data(), info.data(),
                  noise.data(), anc.data(), expect.data(), logw.data());
            for (int n = 0; n < m; ++n) {
                double sum = 0.0;
                for (int p = 0; p < P; ++p) sum += weights[(size_t)n * P + p];
                if (!(fabs(sum - 1.0) < 1e-9)) return 1;
                if (!(info[4 * n] >= 0.999f && info[4 * n] <= (float)P * 1.001f)) return 2;
                for (int p = 0; p < P; ++p)
                    if (anc[(size_t)n * P + p] < 0 || anc[(size_t)n * P + p] >= P) return 3;
                if (!(pose[3 * n] == pose[3 * n] && pose[3 * n + 1] == pose[3 * n + 1] && pose[3 * n + 2] == pose[3 * n + 2])) return 4;
                worst = std::max(worst, (double)info[4 * n + 2]);
            }
        }
    }
    printf("pf harness: ok (largest err_xy %g)\n", worst);
    return worst > 0.0 && worst < 1.0 ? 0 : 5;
}
#endif
