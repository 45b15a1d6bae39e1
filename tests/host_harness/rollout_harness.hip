// tests/host_harness/rollout_harness.hip — TEST TOOLING, not part of the product.
//
// The HOST instantiation of the rollout arithmetic (f1tenth_gym_amd/csrc/f110_math.hpp, roll_*), for tests/test_rollout_host.py:
// the chain of advance_vehicle and sample_distance calls, the alive rule, the minimum, the frame, the scaling and the two track
// projections are compared with the Python model without a GPU.  The GPU tests hold the device instantiation (and the kernels
// around it) to the same model.  With -DROLLOUT_HARNESS_MAIN the file is a stand-alone program that rolls a few candidates on a
// synthetic map and track (what the address and undefined-behaviour sanitizers are run on).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <vector>

#include "../../f1tenth_gym_amd/csrc/f110_math.hpp"

using namespace f110;

namespace {

// roll_candidate's emit on the host: action h's pose into the candidate's rows
struct EmitRows {
    static constexpr bool kOn = true;
    const RollSpec *sp;
    float *row;     // [H][4] or null
    double *raw;    // [H][4] or null
    void operator()(int h, const double *v) const
    {
        for (int q = 0; q < 4; ++q) {
            if (raw) raw[4 * h + q] = v[q];
            if (row) row[4 * h + q] = roll_scaled(v[q], sp->scale[q]);
        }
    }
};

}  // namespace

extern "C" {

// map: dt [Hm][W] with the yaml's resolution and origin (cos, sin of its yaw).  track: cols [7][nseg] or null.  start [m][10] =
// state7, FIFO newest, FIFO older, fill; params [m][18]; actions in the layout's shape.  out [m][K][D], raw [m][K][10], traj
// [m][K][H][4] float32 and traj_raw float64 (both may be null when traj == 0).  The caller has validated the settings.
void hh_rollout(const double *dt, int Hm, int W, double res, double ox, double oy, double oc, double os, const double *cols, int nseg,
                int closed, double L, int K, int H, int repeat, int layout, int frame, int channels, int traj, double margin,
                const double *scale, double time_step, int integrator, double lidar_dist, const double *start, const double *params,
                const double *actions, int m, float *out, double *raw, float *traj_out, double *traj_raw)
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
    RollSpec sp{};
    sp.K = K;
    sp.H = H;
    sp.repeat = repeat;
    sp.layout = layout;
    sp.frame = frame;
    sp.channels = channels;
    sp.traj = traj;
    sp.margin = margin;
    for (int b = 0; b < ROLL_NCHANNELS; ++b) {
        sp.scale[b] = scale[b];
        sp.D += channels >> b & 1;
    }
    const int32_t all = (1 << ROLL_NCHANNELS) - 1;
    for (int n = 0; n < m; ++n) {
        VehicleParams vp;
        for (int q = 0; q < NPARAMS; ++q) vp.v[q] = params[(size_t)n * NPARAMS + q];
        const double *s = start + 10 * (size_t)n;
        const RollFrame fr = roll_frame(frame, s[0], s[1], s[4]);
        double s0 = 0.0, lat0 = 0.0;
        if (cols) roll_project(cols, nseg, s[0], s[1], s0, lat0);
        for (int c = 0; c < K; ++c) {
            const size_t G = (size_t)n * K + c;
            RollCar car;
            for (int q = 0; q < 7; ++q) car.st[q] = s[q];
            car.b0 = s[7];
            car.b1 = s[8];
            car.cnt = (int)s[9];
            const double *act = actions + (layout == ROLL_PER_AGENT ? G : (size_t)c) * H * 2;
            int alive;
            double min_clear;
            if (traj) {
                const EmitRows emit{&sp, traj_out ? traj_out + G * H * 4 : nullptr, traj_raw ? traj_raw + G * H * 4 : nullptr};
                roll_candidate(sp, k, vp, time_step, integrator, lidar_dist, car, act, fr, alive, min_clear, emit);
            } else {
                roll_candidate(sp, k, vp, time_step, integrator, lidar_dist, car, act, fr, alive, min_clear, RollEmitNone());
            }
            double v[ROLL_NCHANNELS];
            roll_values(fr, car, alive, min_clear, all, v);
            for (int b = 0; b < ROLL_NCHANNELS; ++b) raw[G * ROLL_NCHANNELS + b] = 0.0;
            roll_store(sp, v, all & ~kRollTrackBits, out + G * sp.D, raw + G * ROLL_NCHANNELS);
            if (cols) {
                double s1, lat1;
                roll_project(cols, nseg, car.st[0], car.st[1], s1, lat1);
                roll_store_track(sp, roll_progress(s0, s1, closed, L), lat1, out + G * sp.D, raw + G * ROLL_NCHANNELS);
            }
        }
    }
}

double hh_roll_progress(double s_start, double s_end, int closed, double L) { return roll_progress(s_start, s_end, closed, L); }

}

#ifdef ROLLOUT_HARNESS_MAIN
// a 40 x 60 cell room whose clearance is the distance to the nearest wall, a square track inside it, three cars (one starts outside
// the map, one with a NaN state), K = 5 candidates of H = 6 actions held 3 steps, every channel and the trajectory, both frames,
// layouts and integrators
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
    const int m = 3, K = 5, H = 6, repeat = 3;
    std::vector<double> start(10 * (size_t)m, 0.0), params(NPARAMS * (size_t)m), scale(ROLL_NCHANNELS, 2.0);
    for (int n = 0; n < m; ++n)
        for (int q = 0; q < NPARAMS; ++q) params[(size_t)n * NPARAMS + q] = P[q];
    start[0] = 1.0, start[1] = 1.0, start[3] = 2.0, start[9] = 2.0;
    start[10] = -3.0, start[11] = 9.0, start[13] = 0.2, start[19] = 1.0;
    start[20] = NAN, start[21] = 2.0;
    double worst = 0.0;
    for (int variant = 0; variant < 8; ++variant) {
        const int layout = variant & 1, frame = variant >> 1 & 1, integrator = variant >> 2 & 1;
        std::vector<double> act((size_t)(layout ? m : 1) * K * H * 2);
        for (size_t q = 0; q < act.size(); q += 2) {
            act[q] = 0.4 * (double)((int)(q * 7 % 11) - 5) / 5.0;
            act[q + 1] = 1.0 + (double)(q % 9);
        }
        const size_t cands = (size_t)m * K;
        std::vector<float> out(cands * ROLL_NCHANNELS), tr(cands * H * 4);
        std::vector<double> raw(cands * ROLL_NCHANNELS), traw(cands * H * 4);
        hh_rollout(dt.data(), Hm, W, res, -0.5, -0.25, 1.0, 0.0, cols.data(), nseg, 1, cum, K, H, repeat, layout, frame, (1 << ROLL_NCHANNELS) - 1, 1,
                   0.15, scale.data(), 0.01, integrator, 0.275, start.data(), params.data(), act.data(), m, out.data(), raw.data(), tr.data(),
                   traw.data());
        for (size_t g = 0; g < cands; ++g) {
            const double alive = raw[g * ROLL_NCHANNELS + ROLL_ALIVE];
            if (!(alive >= 0.0 && alive <= (double)(H * repeat))) return 1;
            if (g >= 2 * (size_t)K && alive != 0.0) return 2;   // the NaN car dies at once
            worst = alive > worst ? alive : worst;
        }
    }
    printf("rollout harness: ok (longest life %g steps)\n", worst);
    return worst > 0.0 ? 0 : 3;
}
#endif
