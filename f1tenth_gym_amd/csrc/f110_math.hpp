// f110_math.hpp — scalar float64 building blocks of the env.step() hot path for gfx950.
//
// Every function is `__host__ __device__` so the very same code that the HIP kernels inline can
// be exercised on the build container's CPU by tests/host_harness (there is no GPU there);
// the product only ever runs the __device__ instantiations (f110_hip.hip).
//
// Bit-parity discipline: IEEE float64, the reference's operation order, and
// the translation unit is compiled with -ffp-contract=off so `a*b + c` never becomes an FMA.
// Reference citations are gym/f110_gym/envs/<file>:<line> of f1tenth_gym v0.2.1.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#define F110_HD __host__ __device__ __forceinline__

namespace f110 {

constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 2.0 * kPi;

// vehicle parameter slots, key order of f110_env.py:130
enum { P_MU = 0, P_CSF, P_CSR, P_LF, P_LR, P_H, P_M, P_I, P_SMIN, P_SMAX, P_SVMIN, P_SVMAX,
       P_VSWITCH, P_AMAX, P_VMIN, P_VMAX, P_WIDTH, P_LENGTH, NPARAMS };

struct VehicleParams {
    double v[NPARAMS];
};

// cos and sin of ONE angle.  On the device a single argument reduction serves both (ocml's sincos returns what its
// sin and its cos return — the ray-cast has relied on that since round 1); the host instantiation (tests/host_harness)
// makes the two libm calls the oracle makes.  A float64 sin or cos is ~250 dependent instructions of a kernel that is
// a dependent chain (k_integrate) or bound by its vector-ALU work (the finalize kernels): one call instead of two.
F110_HD void cos_sin(double a, double &c, double &s)
{
#if defined(__HIP_DEVICE_COMPILE__)
    sincos(a, &s, &c);
#else
    c = cos(a);
    s = sin(a);
#endif
}

// ------------------------------------------------------------------ dynamic_models.py
// accl_constraints :29-60
F110_HD double clamp_accel(double vel, double accl, const VehicleParams &p)
{
    const double a_max = p.v[P_AMAX];
    const double pos_limit = (vel > p.v[P_VSWITCH]) ? a_max * p.v[P_VSWITCH] / vel : a_max;
    if ((vel <= p.v[P_VMIN] && accl <= 0) || (vel >= p.v[P_VMAX] && accl >= 0)) return 0.;
    if (accl <= -a_max) return -a_max;
    if (accl >= pos_limit) return pos_limit;
    return accl;
}

// steering_constraint :62-87
F110_HD double clamp_steer_rate(double steer_angle, double sv, const VehicleParams &p)
{
    if ((steer_angle <= p.v[P_SMIN] && sv <= 0) || (steer_angle >= p.v[P_SMAX] && sv >= 0)) return 0.;
    if (sv <= p.v[P_SVMIN]) return p.v[P_SVMIN];
    if (sv >= p.v[P_SVMAX]) return p.v[P_SVMAX];
    return sv;
}

// vehicle_dynamics_ks :90-121 — x[0..4], raw inputs (sv, accl); f[0..4]
F110_HD void rhs_kinematic(const double *x, double sv_in, double accl_in, const VehicleParams &p, double *f)
{
    const double lwb = p.v[P_LF] + p.v[P_LR];
    const double u0 = clamp_steer_rate(x[2], sv_in, p);
    const double u1 = clamp_accel(x[3], accl_in, p);
    double c4, s4;
    cos_sin(x[4], c4, s4);
    f[0] = x[3] * c4;
    f[1] = x[3] * s4;
    f[2] = u0;
    f[3] = u1;
    f[4] = x[3] / lwb * tan(x[2]);
}

// Where the low-speed branch's tan(steer) and cos(steer) come from: computed in place (everywhere but k_integrate), or
// handed over by the kernel's second wave, which runs one stage ahead (LowTrigShared in f110_kernels.hpp).
struct LowTrigDirect {
    F110_HD void begin_stage(int /*stage*/) const {}   // (called by every lane at the top of every stage)
    F110_HD void operator()(int /*stage*/, double steer, double &tn, double &cd) const
    {
        tn = tan(steer);
        cd = cos(steer);
    }
};

// vehicle_dynamics_st :123-176 — x[0..6] = (x, y, steer, v, yaw, yaw_rate, slip)
template <class LowTrig>
F110_HD void rhs_single_track_with(const double *x, double sv_in, double accl_in, const VehicleParams &p, double *f, int stage,
                                   const LowTrig &low_trig)
{
    const double g = 9.81;
    const double u0 = clamp_steer_rate(x[2], sv_in, p);
    const double u1 = clamp_accel(x[3], accl_in, p);
    // :152-160 low-speed kinematic branch (the reference feeds the constrained inputs through
    // vehicle_dynamics_ks, which constrains them once more) or the single-track model proper.  Both start with
    // velocity * (cos, sin) of ONE angle — the heading, or heading + slip — so a wave with lanes on either
    // side (every wave of a batch that re-seats crashed cars: they restart at v = 0) evaluates ONE cos_sin for
    // both instead of one per branch: the same operations per lane, ~150 instructions off every RK4 stage of a
    // kernel that is a dependent chain.
    const bool low = fabs(x[3]) < 0.5;
    double ca, sa;
    cos_sin(low ? x[4] : x[6] + x[4], ca, sa);
    f[0] = x[3] * ca;
    f[1] = x[3] * sa;
    if (low) {
        const double lwb = p.v[P_LF] + p.v[P_LR];
        double tn, cd;
        low_trig(stage, x[2], tn, cd);
        f[2] = clamp_steer_rate(x[2], u0, p);   // vehicle_dynamics_ks :108-109 on the already constrained inputs
        f[3] = clamp_accel(x[3], u1, p);
        f[4] = x[3] / lwb * tn;
        f[5] = u1 / lwb * tn + x[3] / (lwb * (cd * cd)) * u0;
        f[6] = 0.;
        return;
    }
    const double mu = p.v[P_MU], csf = p.v[P_CSF], csr = p.v[P_CSR], lf = p.v[P_LF], lr = p.v[P_LR];
    const double h = p.v[P_H], m = p.v[P_M], iz = p.v[P_I];
    const double rear = g * lr - u1 * h;   // (g*lr - u[1]*h)
    const double front = g * lf + u1 * h;  // (g*lf + u[1]*h)
    const double wb = lr + lf;
    f[2] = u0;
    f[3] = u1;
    f[4] = x[5];
    // :169-171
    const double t1 = -mu * m / (x[3] * iz * wb) * ((lf * lf) * csf * rear + (lr * lr) * csr * front) * x[5];
    const double t2 = mu * m / (iz * wb) * (lr * csr * front - lf * csf * rear) * x[6];
    const double t3 = mu * m / (iz * wb) * lf * csf * rear * x[2];
    f[5] = t1 + t2 + t3;
    // :172-174
    const double s1 = (mu / ((x[3] * x[3]) * wb) * (csr * front * lr - csf * rear * lf) - 1) * x[5];
    const double s2 = mu / (x[3] * wb) * (csr * front + csf * rear) * x[6];
    const double s3 = mu / (x[3] * wb) * (csf * rear) * x[2];
    f[6] = s1 - s2 + s3;
}

F110_HD void rhs_single_track(const double *x, double sv_in, double accl_in, const VehicleParams &p, double *f)
{
    rhs_single_track_with(x, sv_in, accl_in, p, f, 0, LowTrigDirect());
}

// pid :178-221
F110_HD void speed_steer_controller(double speed, double steer, double cur_speed, double cur_steer,
                                    const VehicleParams &p, double &accl, double &sv)
{
    const double steer_diff = steer - cur_steer;
    sv = (fabs(steer_diff) > 1e-4) ? (steer_diff / fabs(steer_diff)) * p.v[P_SVMAX] : 0.0;
    const double vel_diff = speed - cur_speed;
    double kp;
    if (cur_speed > 0.)
        kp = (vel_diff > 0) ? 10.0 * p.v[P_AMAX] / p.v[P_VMAX] : 10.0 * p.v[P_AMAX] / (-p.v[P_VMIN]);
    else
        kp = (vel_diff > 0) ? 2.0 * p.v[P_AMAX] / p.v[P_VMAX] : 2.0 * p.v[P_AMAX] / (-p.v[P_VMIN]);
    accl = kp * vel_diff;
}

// ------------------------------------------------------------------ base_classes.py
// RaceCar.update_pose :256-409 minus the scan.  buf[0] = newest delayed steer command.
template <class LowTrig>
F110_HD void advance_vehicle_with(double *st, double &buf0, double &buf1, int &buf_cnt, double raw_steer,
                                  double speed_cmd, const VehicleParams &p, double dt, int integrator,
                                  double lidar_dist, double *scan_pose, const LowTrig &low_trig)
{
    // :271-278 two-step steering delay
    double steer = 0.;
    if (buf_cnt < 2) {
        buf_cnt += 1;
    } else {
        steer = buf1;
    }
    buf1 = buf0;
    buf0 = raw_steer;

    double accl, sv;
    speed_steer_controller(speed_cmd, steer, st[3], st[2], p, accl, sv);  // :282

    {
        // Integrator.RK4 :284-373 (k1..k4, state + dt/6 * (k1 + 2 k2 + 2 k3 + k4)) and Integrator.Euler
        // :375-395 as ONE loop over the stages, not unrolled: the right-hand side is the bulk of this
        // kernel's code, and a kernel that runs one wave per SIMD pays for every instruction byte it
        // has to fetch.  Same operations in the same order as the reference's straight-line code:
        // acc = ((k1 + 2*k2) + 2*k3) + 1*k4, stage inputs st + dt*(k/2), st + dt*(k/2), st + dt*k.
        const int stages = (integrator == 1) ? 4 : 1;
        double acc[7], tmp[7], kk[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) tmp[i] = st[i];
#pragma unroll 1
        for (int sidx = 0; sidx < stages; ++sidx) {
            low_trig.begin_stage(sidx);
            rhs_single_track_with(tmp, sv, accl, p, kk, sidx, low_trig);
            const double wgt = (sidx == 1 || sidx == 2) ? 2.0 : 1.0;
#pragma unroll
            for (int i = 0; i < 7; ++i) {
                acc[i] = (sidx == 0) ? kk[i] : acc[i] + wgt * kk[i];
                const double h = (sidx < 2) ? kk[i] / 2 : kk[i];
                tmp[i] = st[i] + dt * h;
            }
        }
        const double w = (integrator == 1) ? dt * (1. / 6.) : dt;
#pragma unroll
        for (int i = 0; i < 7; ++i) st[i] = st[i] + w * acc[i];
    }
    // :400-404
    if (st[4] > kTwoPi)
        st[4] = st[4] - kTwoPi;
    else if (st[4] < 0)
        st[4] = st[4] + kTwoPi;
    // :407-409.  With the lidar on the reference point (lidar_dist == 0., the default of F110Env) the products are
    // +-0. and x + (+-0.) == x for every x except -0. — the two trig calls are skipped exactly then (finite heading,
    // no negative zero among the coordinates): the same bits, ~500 instructions off k_integrate's chain
    const bool on_axle = lidar_dist == 0.0 && fabs(st[4]) < 1e300 && !(st[0] == 0.0 && signbit(st[0])) && !(st[1] == 0.0 && signbit(st[1]));
    if (on_axle) {
        scan_pose[0] = st[0];
        scan_pose[1] = st[1];
    } else {
        double ch, sh;
        cos_sin(st[4], ch, sh);
        scan_pose[0] = st[0] + lidar_dist * ch;
        scan_pose[1] = st[1] + lidar_dist * sh;
    }
    scan_pose[2] = st[4];
}

F110_HD void advance_vehicle(double *st, double &buf0, double &buf1, int &buf_cnt, double raw_steer,
                             double speed_cmd, const VehicleParams &p, double dt, int integrator,
                             double lidar_dist, double *scan_pose)
{
    advance_vehicle_with(st, buf0, buf1, buf_cnt, raw_steer, speed_cmd, p, dt, integrator, lidar_dist, scan_pose, LowTrigDirect());
}

// The steering angle and the velocity through the RK4 stages, on their own: their derivatives — the constrained
// steering rate and acceleration, constrained a second time inside the low-speed branch (:152-160 -> :108-109) —
// depend on nothing else, so a second wave can walk (x[2], x[3]) ahead of the integration and have the low-speed
// branch's tan / cos ready (k_integrate).  Same operations in the same order as advance_vehicle_with's loop.
// emit(stage, tan, cos) is called by the lanes whose stage takes the low-speed branch, emit.end_stage(stage) by all.
template <class Emit>
F110_HD void low_speed_trig_ahead(double steer0, double vel0, double buf1, int buf_cnt, double speed_cmd, const VehicleParams &p,
                                  double dt, int integrator, const Emit &emit)
{
    const double steer = (buf_cnt < 2) ? 0. : buf1;   // :271-278 (the command that leaves the delay buffer this step)
    double accl, sv;
    speed_steer_controller(speed_cmd, steer, vel0, steer0, p, accl, sv);
    const int stages = (integrator == 1) ? 4 : 1;
    double x2 = steer0, x3 = vel0;
    for (int sidx = 0; sidx < stages; ++sidx) {
        const bool low = fabs(x3) < 0.5;
        if (low) emit(sidx, tan(x2), cos(x2));
        emit.end_stage(sidx);   // (every lane, every stage)
        const double u0 = clamp_steer_rate(x2, sv, p), u1 = clamp_accel(x3, accl, p);
        const double f2 = low ? clamp_steer_rate(x2, u0, p) : u0;
        const double f3 = low ? clamp_accel(x3, u1, p) : u1;
        const double h2 = (sidx < 2) ? f2 / 2 : f2, h3 = (sidx < 2) ? f3 / 2 : f3;
        x2 = steer0 + dt * h2;
        x3 = vel0 + dt * h3;
    }
}

// ---- the RK4 step taken apart by what depends on what (k_integrate_fan, round 4) --------------------------------
// advance_vehicle_with is one dependent chain of ~1900 instructions per agent: four stages, each a cos / sin of the
// heading, the low-speed branch's tan / cos of the steering angle or the single-track branch's three divisions by the
// velocity, and the stage update.  Its dataflow is much shallower than that:
//   * (steer, velocity) walk through the stages on their own (their derivatives are the constrained inputs);
//   * the low-speed branch's f4, f5 and the single-track branch's coefficients of (yaw rate, slip) in f5, f6 depend on
//     that walk only;
//   * given those, (yaw, yaw rate, slip) advance by a handful of multiply-adds per stage;
//   * the position derivatives — velocity x (cos, sin)(heading) — feed nothing but the position itself.
// So: one wave per (role, stage) computes the expensive piece it owns (fan_low, fan_dyn, fan_pos), the main wave
// chains the cheap recurrence (fan_main) and combines.  Every operation of advance_vehicle_with is executed once, on
// the same operands, in the same order within each expression: bit-identical (tests/test_host_math.py).
struct FanWalk {   // (steer, velocity) and their constrained rates at one stage
    double x2, x3, u0, u1;
    bool low;
};
// the pid of :282 — (accl, sv) — from what every role reads of the agent: raw state, delay buffer, speed command
F110_HD void fan_inputs(double steer0, double vel0, double buf1, int buf_cnt, double speed_cmd, const VehicleParams &p, double &accl, double &sv)
{
    const double steer = (buf_cnt < 2) ? 0. : buf1;   // :271-278 (the command that leaves the delay buffer this step)
    speed_steer_controller(speed_cmd, steer, vel0, steer0, p, accl, sv);
}
// the walk up to `stage` (0..3): same operations as low_speed_trig_ahead / advance_vehicle_with's loop for x[2], x[3]
F110_HD FanWalk fan_walk(double steer0, double vel0, double accl, double sv, const VehicleParams &p, double dt, int stage)
{
    FanWalk w;
    w.x2 = steer0;
    w.x3 = vel0;
    for (int sidx = 0;; ++sidx) {
        w.low = fabs(w.x3) < 0.5;
        w.u0 = clamp_steer_rate(w.x2, sv, p);
        w.u1 = clamp_accel(w.x3, accl, p);
        if (sidx == stage) return w;
        const double f2 = w.low ? clamp_steer_rate(w.x2, w.u0, p) : w.u0;
        const double f3 = w.low ? clamp_accel(w.x3, w.u1, p) : w.u1;
        const double h2 = (sidx < 2) ? f2 / 2 : f2, h3 = (sidx < 2) ? f3 / 2 : f3;
        w.x2 = steer0 + dt * h2;
        w.x3 = vel0 + dt * h3;
    }
}
// low-speed branch (:152-160): f[4], f[5] of rhs_single_track_with
F110_HD void fan_low(const FanWalk &w, const VehicleParams &p, double &f4, double &f5)
{
    const double lwb = p.v[P_LF] + p.v[P_LR];
    const double tn = tan(w.x2), cd = cos(w.x2);
    f4 = w.x3 / lwb * tn;
    f5 = w.u1 / lwb * tn + w.x3 / (lwb * (cd * cd)) * w.u0;
}
// single-track branch (:164-174): f5 = (k[0] * yaw_rate + k[1] * slip) + k[2], f6 = (k[3] * yaw_rate - k[4] * slip) + k[5]
F110_HD void fan_dyn(const FanWalk &w, const VehicleParams &p, double *k)
{
    const double g = 9.81;
    const double mu = p.v[P_MU], csf = p.v[P_CSF], csr = p.v[P_CSR], lf = p.v[P_LF], lr = p.v[P_LR];
    const double h = p.v[P_H], m = p.v[P_M], iz = p.v[P_I];
    const double rear = g * lr - w.u1 * h;
    const double front = g * lf + w.u1 * h;
    const double wb = lr + lf;
    k[0] = -mu * m / (w.x3 * iz * wb) * ((lf * lf) * csf * rear + (lr * lr) * csr * front);
    k[1] = mu * m / (iz * wb) * (lr * csr * front - lf * csf * rear);
    k[2] = mu * m / (iz * wb) * lf * csf * rear * w.x2;
    k[3] = mu / ((w.x3 * w.x3) * wb) * (csr * front * lr - csf * rear * lf) - 1;
    k[4] = mu / (w.x3 * wb) * (csr * front + csf * rear);
    k[5] = mu / (w.x3 * wb) * (csf * rear) * w.x2;
}
// position derivatives of one stage: velocity x (cos, sin)(angle), angle = heading (low speed) or heading + slip
F110_HD void fan_pos(double angle, double vel, double &f0, double &f1)
{
    double ca, sa;
    cos_sin(angle, ca, sa);
    f0 = vel * ca;
    f1 = vel * sa;
}
// The main chain.  take_low(stage, f4, f5) / take_dyn(stage, k6) fetch what fan_low / fan_dyn produced for the stages that
// took that branch; emit_angle(stage, angle, vel) hands the stage's position-derivative operands on.  st[2..6] are
// advanced to the end of the step here (st[0], st[1] by fan_combine_position); returns nothing else.
template <class TakeLow, class TakeDyn, class EmitAngle>
F110_HD void fan_main(double *st, double accl, double sv, const VehicleParams &p, double dt, const TakeLow &take_low, const TakeDyn &take_dyn,
                      const EmitAngle &emit_angle)
{
    double acc[5], tmp[5], kk[5];   // components 2..6
#pragma unroll
    for (int i = 0; i < 5; ++i) tmp[i] = st[2 + i];
#pragma unroll 1
    for (int sidx = 0; sidx < 4; ++sidx) {
        const double x2 = tmp[0], x3 = tmp[1], x4 = tmp[2], x5 = tmp[3], x6 = tmp[4];
        const double u0 = clamp_steer_rate(x2, sv, p);
        const double u1 = clamp_accel(x3, accl, p);
        const bool low = fabs(x3) < 0.5;
        emit_angle(sidx, low ? x4 : x6 + x4, x3);
        if (low) {
            kk[0] = clamp_steer_rate(x2, u0, p);
            kk[1] = clamp_accel(x3, u1, p);
            take_low(sidx, kk[2], kk[3]);
            kk[4] = 0.;
        } else {
            double k[6];
            take_dyn(sidx, k);
            kk[0] = u0;
            kk[1] = u1;
            kk[2] = x5;
            kk[3] = (k[0] * x5 + k[1] * x6) + k[2];
            kk[4] = (k[3] * x5 - k[4] * x6) + k[5];
        }
        const double wgt = (sidx == 1 || sidx == 2) ? 2.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            acc[i] = (sidx == 0) ? kk[i] : acc[i] + wgt * kk[i];
            const double h = (sidx < 2) ? kk[i] / 2 : kk[i];
            tmp[i] = st[2 + i] + dt * h;
        }
    }
    const double w = dt * (1. / 6.);
#pragma unroll
    for (int i = 0; i < 5; ++i) st[2 + i] = st[2 + i] + w * acc[i];
}
// x, y: the four stages' derivatives combined as advance_vehicle_with combines them
F110_HD double fan_combine(double x, double dt, double k1, double k2, double k3, double k4)
{
    double acc = k1;
    acc = acc + 2.0 * k2;
    acc = acc + 2.0 * k3;
    acc = acc + 1.0 * k4;
    return x + (dt * (1. / 6.)) * acc;
}
// what follows the integration in advance_vehicle_with: yaw wrap :400-404 and the lidar pose :407-409
F110_HD void fan_finish(double *st, double lidar_dist, double *scan_pose)
{
    if (st[4] > kTwoPi)
        st[4] = st[4] - kTwoPi;
    else if (st[4] < 0)
        st[4] = st[4] + kTwoPi;
    const bool on_axle = lidar_dist == 0.0 && fabs(st[4]) < 1e300 && !(st[0] == 0.0 && signbit(st[0])) && !(st[1] == 0.0 && signbit(st[1]));
    if (on_axle) {
        scan_pose[0] = st[0];
        scan_pose[1] = st[1];
    } else {
        double ch, sh;
        cos_sin(st[4], ch, sh);
        scan_pose[0] = st[0] + lidar_dist * ch;
        scan_pose[1] = st[1] + lidar_dist * sh;
    }
    scan_pose[2] = st[4];
}

// ------------------------------------------------------------------ laser_models.py
enum { LAYOUT_ROWMAJOR = 0, LAYOUT_PADDED = 3 };   // (1 = 4x4 tiles and 2 = byte codes + LUT: retired in round 5)

struct ScanConst {
    const double *table;   // the distance table dt[r][c] (PADDED: the interior of the padded copy, its row pitch)
    const double *table_rm;  // the same (a separate row-major original only while a map too large for PADDED is loaded)
    const double *reserved_pad_t; // (rounds 5-6: a tiled / row-pair copy of the PADDED table; retired — the field keeps the kernel-argument layout)
    const void *reserved_lut;
    const double2 *cs;     // (cos, sin) of linspace(0, 2pi, theta_dis), interleaved
    int32_t height, width, pad_tiles, theta_dis;
    int32_t num_beams, res_pow2, ident_rot, row_bytes;  // row_bytes = width * 8
    int32_t reserved_pad_t_row_bytes, pad1;
    double res, inv_res, orig_x, orig_y, orig_c, orig_s;
    double w_res, h_res;   // width*resolution, height*resolution (xy_2_rc :79)
    double oob_value;      // dt[-1,-1]: what an out-of-bounds sample reads (:80-81,:103)
    double eps, max_range, fov, theta_inc, dir_guard, inv_theta_dis;
    // PADDED: the row-major table surrounded by `pad_border` cells of oob_value on every side,
    // addressed in fixed point (see march_padded).  pad == nullptr: not available for this map.
    const double *pad;
    int32_t pad_border, pad_row_bytes, pad_width, pad_height;
    double pad_lo, pad_hi_x, pad_hi_y;  // lidar positions (padded cell units) whose rays stay inside
    double pad_cx, pad_cy;              // padded_position: u = x*axx + y*axy + cx  (IDENT: axx = inv_res, axy = 0)
    double pad_axx, pad_axy, pad_ayx, pad_ayy;
    int32_t pad_max_samples, pad_reserved;  // samples per ray the fixed-point error bound covers
};

// The PADDED fast path keeps a ray's position in padded-table cell units u (approximate on
// purpose: it differs from the reference's float64 position by less than kPadGuard / 4 cells,
// setup_padded) and reads the cell as the integer part of the fixed-point word that adding
// kFixBig = 1.5 * 2^36 leaves in the low mantissa bits (ulp = 2^-16 cells):
//   lo32(u + kFixBig) = round(u * 65536),  cell = word >> 16,  fraction = word & 0xffff.
// The addition rounds to nearest, so only a position within 2^-17 cells of a cell boundary can
// come out with fraction == 0; for those (1 sample in 30 000) the distance to the boundary is
// looked at in full precision: further than kPadGuard = 2^-27 cells -> the cell is floor(u), the
// same cell the reference's int(x_rot / resolution) and range tests (laser_models.py:79-84) pick,
// because everything that differs from the reference is smaller than kPadGuard / 4; closer -> the
// ray is re-marched with the reference's arithmetic (about one ray in 10^7).  Out-of-range
// samples need no test at all: the border cells hold the value the reference reads for them.
constexpr double kFixBig = 103079215104.0;  // 1.5 * 2^36
constexpr int kFixFracBits = 16;
constexpr int kPadSlack = 64;               // extra border cells so a lidar slightly outside the map stays fast
constexpr double kPadGuard = 7.450580596923828e-09;  // 2^-27 cells: closer to a cell boundary than this -> exact march

F110_HD uint32_t low_word(double v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__double2loint(v);
#else
    uint64_t b;
    __builtin_memcpy(&b, &v, 8);
    return (uint32_t)b;
#endif
}

// border width in cells for a map: rays sample at most max_range (+ rounding) away from the lidar
F110_HD int padded_border_cells(double max_range, double inv_res)
{
    return (int)ceil(max_range * inv_res) + 2 + kPadSlack;
}

// fills the PADDED constants of k (k.pad itself is set by the caller); false when the map is too
// large for 16-bit cell coordinates / 32-bit byte offsets and the exact path must be used
F110_HD bool setup_padded(ScanConst &k)
{
    const int b = padded_border_cells(k.max_range, k.inv_res);
    const long long wp = (long long)k.width + 2 * b, hp = (long long)k.height + 2 * b;
    k.pad = nullptr;
    k.pad_border = b;
    if (wp >= 65536 || hp >= 65536 || wp * 8 >= (1 << 24) || wp * hp * 8 >= (1ll << 32)) return false;
    k.pad_width = (int)wp;
    k.pad_height = (int)hp;
    k.pad_row_bytes = (int)(wp * 8);
    const double reach = ceil(k.max_range * k.inv_res) + 2.0;
    k.pad_lo = reach + 1.0;
    k.pad_hi_x = (double)wp - reach - 2.0;
    k.pad_hi_y = (double)hp - reach - 2.0;
    k.pad_axx = k.orig_c * k.inv_res;
    k.pad_axy = k.orig_s * k.inv_res;
    k.pad_ayx = -k.orig_s * k.inv_res;
    k.pad_ayy = k.orig_c * k.inv_res;
    k.pad_cx = (double)b - (k.orig_x * k.orig_c + k.orig_y * k.orig_s) * k.inv_res;
    k.pad_cy = (double)b - (k.orig_y * k.orig_c - k.orig_x * k.orig_s) * k.inv_res;
    // Error budget of march_padded against the reference's float64 positions, in cells.  Per
    // sample: the reference rounds x += d*c (<= 1 ulp of the largest coordinate), the fixed-point
    // side rounds one fma (<= 1/2 ulp of the padded width) and carries the 2^-52 relative error of
    // cu.  Once: the start position, the offsets, the rotation and the final division.
    const double xmax = fabs(k.orig_x) + fabs(k.orig_y) + ((double)k.width + (double)k.height) * k.res + 2.0 * k.max_range + 1.0;
    const double ulp_x = xmax * 2.220446049250313e-16, ulp_u = (double)(wp > hp ? wp : hp) * 2.220446049250313e-16;
    const double per_sample = ulp_x * k.inv_res + ulp_u + 4.0 * 2.220446049250313e-16 * k.max_range * k.inv_res;
    const double once = 8.0 * (ulp_x * k.inv_res + ulp_u);
    const double n_max = floor((0.25 * kPadGuard - once) / per_sample);
    if (!(n_max >= 256.0)) return false;  // coordinates too large for the bound to be useful
    k.pad_max_samples = n_max > 1e6 ? 1000000 : (int)n_max;
    return true;
}

// 24-bit multiply (v_mul_u32_u24 / v_mad_u32_u24 are full-rate; the 32-bit v_mul_lo_u32 is not).
// Rows, columns and row pitches of any realistic map are far below 2^24.
F110_HD uint32_t mul24(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul24(a, b);
#else
    return a * b;
#endif
}

// what march_padded does with every byte offset it is about to load from: nothing, unless a host test program defines it
// to check the offset against the table it built (tests/host_harness/march_chain_main.hip)
#ifndef F110_MARCH_OFFSET_HOOK
#define F110_MARCH_OFFSET_HOOK(off) ((void)0)
#endif

// true when the condition holds in any active lane of the wave (host: in this one "lane")
F110_HD bool any_lane(bool c)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ballot(c) != 0ull;
#else
    return c;
#endif
}

// One table value.  (Rounds 1-4 also had a 4x4-tiled float64 layout and a 1-byte-code + exact-value-LUT layout behind this
// function — bit-identical, measured slower, retired in round 5: DESIGN_HISTORY.md.  `lut` is that layout's parameter.)
template <int LAYOUT>
F110_HD double table_fetch(const ScanConst &k, int r, int c, const double *lut)
{
    static_assert(LAYOUT == LAYOUT_ROWMAJOR || LAYOUT == LAYOUT_PADDED, "row-major or padded");
    (void)lut;
    // 32-bit BYTE offset from the (wave-uniform) table base: lets the compiler use the
    // scalar-base + 32-bit-VGPR-offset form of global_load (tables are < 4 GiB, checked on upload).
    // PADDED: k.table is the plain table here (the exact path)
    const uint32_t off = mul24((uint32_t)r, (uint32_t)k.row_bytes) + ((uint32_t)c << 3);
    return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(k.table) + off);
}

// int(v / resolution) of xy_2_rc :83-84 for v in [0, extent).  When the resolution is a power
// of two the reciprocal multiply is exact; otherwise the multiply decides unless the quotient
// lands within 1e-9 of a cell boundary, where the true IEEE division is evaluated.
template <bool POW2>
F110_HD int cell_index(double v, const ScanConst &k)
{
    const double q = v * k.inv_res;
    int ci = (int)q;
    if (!POW2) {
        const double fr = q - (double)ci;
        if (fr < 1e-9 || fr > 1.0 - 1e-9) ci = (int)(v / k.res);
    }
    return ci;
}

// xy_2_rc :55-86 + distance_transform :88-104.  rc = (-1,-1) when out of bounds.
template <int LAYOUT, bool POW2, bool IDENT>
F110_HD double sample_distance(const ScanConst &k, const double *lut, double x, double y, int &r, int &c)
{
    const double xt = x - k.orig_x;
    const double yt = y - k.orig_y;
    double xr, yr;
    if (IDENT) {  // origin yaw == 0: x_trans*1 + y_trans*0 == x_trans for finite values
        xr = xt;
        yr = yt;
    } else {
        xr = xt * k.orig_c + yt * k.orig_s;
        yr = -xt * k.orig_s + yt * k.orig_c;
    }
    // one combined predicate (bitwise &, no short-circuit) -> a single divergent region per
    // sample.  The reference's "x_rot < 0 or x_rot >= w*res or ..." (:79) is its complement
    // for every non-NaN position.
    const bool inside = (xr >= 0) & (xr < k.w_res) & (yr >= 0) & (yr < k.h_res);
    double d = k.oob_value;
    r = -1;
    c = -1;
    if (inside) {
        c = cell_index<POW2>(xr, k);
        r = cell_index<POW2>(yr, k);
        d = table_fetch<LAYOUT>(k, r, c, lut);
    }
    return d;
}

// trace_ray :133-146 — the marching loop, entered with the first sample (:129-130) already taken.
// Every ray of one scan starts at the same lidar position, so that first sample is shared by
// all beams of an agent: the step kernel receives it from k_integrate instead of gathering it
// once per ray.
template <int LAYOUT, bool POW2, bool IDENT>
F110_HD double march_from_first(const ScanConst &k, const double *lut, double x, double y, double c, double s,
                                double d, int &hit_r, int &hit_c, int &lookups)
{
    double total = d;
    int n = 1;
    while (d > k.eps && total <= k.max_range) {
        x += d * c;
        y += d * s;
        d = sample_distance<LAYOUT, POW2, IDENT>(k, lut, x, y, hit_r, hit_c);
        total += d;
        ++n;
    }
    lookups = n;
    return (total > k.max_range) ? k.max_range : total;
}

// trace_ray :106-146 (sphere tracing over the distance table)
template <int LAYOUT, bool POW2, bool IDENT>
F110_HD double march_ray(const ScanConst &k, const double *lut, double x, double y, double c, double s,
                         int &hit_r, int &hit_c, int &lookups)
{
    const double d = sample_distance<LAYOUT, POW2, IDENT>(k, lut, x, y, hit_r, hit_c);
    return march_from_first<LAYOUT, POW2, IDENT>(k, lut, x, y, c, s, d, hit_r, hit_c, lookups);
}

// ---- PADDED fast path ---------------------------------------------------------------------
// world position -> padded-table cell units (xy_2_rc :68-77 then / resolution, + border), with
// the rotation, the 1/resolution and the offsets folded into six constants (setup_padded)
template <bool IDENT>
F110_HD void padded_position(const ScanConst &k, double x, double y, double &ux, double &uy)
{
    if (IDENT) {
        ux = fma(x, k.inv_res, k.pad_cx);
        uy = fma(y, k.inv_res, k.pad_cy);
    } else {
        ux = fma(x, k.pad_axx, fma(y, k.pad_axy, k.pad_cx));
        uy = fma(y, k.pad_ayy, fma(x, k.pad_ayx, k.pad_cy));
    }
}

// ray direction -> padded cells advanced per metre of range
template <bool IDENT>
F110_HD void padded_rate(const ScanConst &k, double c, double s, double &cux, double &cuy)
{
    if (IDENT) {
        cux = c * k.inv_res;
        cuy = s * k.inv_res;
    } else {
        cux = fma(c, k.pad_axx, s * k.pad_axy);
        cuy = fma(s, k.pad_ayy, c * k.pad_ayx);
    }
}

// true when every sample of every ray from this lidar position lands inside the padded table
// (false for NaN): samples are taken at most max_range (+ rounding) from the lidar
F110_HD bool padded_start_ok(const ScanConst &k, double ux, double uy)
{
    return (ux >= k.pad_lo) & (ux <= k.pad_hi_x) & (uy >= k.pad_lo) & (uy <= k.pad_hi_y);
}

// trace_ray :133-146 on the padded table, entered with the first sample d taken.  (ux, uy) is
// the lidar in padded cell units and (cux, cuy) the cells advanced per metre, so sample n is at
// u_n = u_0 + (d_0 + ... + d_{n-1}) * cu: the same point as the reference's x_n of :140-141 up to
// rounding, |u_n - reference| < kPadGuard / 4 for n <= k.pad_max_samples (setup_padded).
// Returns false when the ray must be re-marched with the reference's arithmetic: a sample within
// kPadGuard of a cell boundary, or more samples than the error bound covers (about one ray in
// 10^7); the outputs are then meaningless.
// r/c: cell of the last sample in the reference's convention (-1,-1 out of bounds); untouched when
// the loop takes no sample.
// (Rounds 5-6 also marched a 4x4-tiled copy and a row-pair copy — 2 rows x 8 cells per 128-byte line — of this table behind this
// function: bit-identical, fewer distinct lines per 64-ray gather (11.4 -> 8.6 / 9.1), paid for in integer operations per sample
// (+6 / +2); tiles lost 2-3 % at every size, row pairs were neutral from 8192 agents up and -2.5 % below 2048 agents.  Retired in
// round 6 under the pre-registered stop rule: DESIGN.md §8, profiles/r05_tiled_table.txt, profiles/r06_rowpair*.txt.)
template <bool WANT_CELL>
F110_HD bool march_padded(const ScanConst &k, double ux, double uy, double cux, double cuy, double d, double &range,
                          int &hit_r, int &hit_c, int &lookups)
{
    double total = d;
    int n = 1;
    // The give-up decision is a per-lane range limit, not a flag: a flag that is live across the back edge and part of
    // the loop condition is carried as lane masks (five scalar mask instructions per sample on gfx950, for a decision
    // taken on one sample in 10^7).  lim = -1 ends the loop at its next test, after the same load, total and n as the
    // flag did: the loop only goes on past a d > eps, so where it would go on total > 0 > lim.
    double lim = k.max_range;
    const char *base = reinterpret_cast<const char *>(k.pad);
    while ((d > k.eps) & (total <= lim)) {
        ux = fma(d, cux, ux);
        uy = fma(d, cuy, uy);
        const uint32_t wx = low_word(ux + kFixBig);
        const uint32_t wy = low_word(uy + kFixBig);
        uint32_t off = mul24(wy >> kFixFracBits, (uint32_t)k.pad_row_bytes) + ((wx >> kFixFracBits) << 3);
        if (WANT_CELL) {
            hit_c = (int)(wx >> kFixFracBits);
            hit_r = (int)(wy >> kFixFracBits);
        }
        // one compare for "either fraction is zero": the product of the two 16-bit fractions; and one wave-uniform
        // branch around the rare block for the (usual) wave that has no such lane, instead of an exec save / restore
        const bool edge = mul24(wx & 0xffffu, wy & 0xffffu) == 0u;
        if (__builtin_expect(any_lane(edge), 0)) {
            // within 2^-17 of a cell boundary, where the word (rounded to nearest) may name the
            // cell above: take the floor, and give the ray up if it is closer than kPadGuard.
            // (Evaluated by every lane of such a wave and selected per lane: the selects keep the block free of a second,
            // divergent branch.  With one sample in 30 000 per lane, above, that is at most one wave-sample in 470.)
            const bool near = (fabs(ux - rint(ux)) < kPadGuard) | (fabs(uy - rint(uy)) < kPadGuard);
            lim = (edge & near) ? -1.0 : lim;
            const int fc = (int)floor(ux), fr = (int)floor(uy);
            const uint32_t off_floor = mul24((uint32_t)fr, (uint32_t)k.pad_row_bytes) + ((uint32_t)fc << 3);
            off = edge ? off_floor : off;
            if (WANT_CELL) {
                hit_c = edge ? fc : hit_c;
                hit_r = edge ? fr : hit_r;
            }
        }
        F110_MARCH_OFFSET_HOOK(off);
        d = *reinterpret_cast<const double *>(base + off);
        total += d;
        ++n;
    }
    if (WANT_CELL && n > 1) {
        hit_c -= k.pad_border;
        hit_r -= k.pad_border;
        if (hit_c < 0 || hit_c >= k.width || hit_r < 0 || hit_r >= k.height) {
            hit_r = -1;
            hit_c = -1;
        }
    }
    lookups = n;
    range = (total > k.max_range) ? k.max_range : total;
    return !((lim < 0.0) | (n > k.pad_max_samples));
}

// (Round 5 also had march_padded_spec here — the tail of a long ray two samples per memory round trip where the table value
// repeats, bit-identical — measured slower at every setting and retired in round 6: DESIGN.md §8, profiles/r05_spec_march.txt.)

// The exact march for the rays march_padded gives up on, written to keep the fast kernel's
// register footprint: its constants are fetched from the HBM copy of ScanConst when (if ever) it
// runs, and it uses the reference's own arithmetic (true divisions, width*resolution formed from
// the integers as laser_models.py:79 does) on the plain row-major table.
template <bool IDENT>
F110_HD double march_exact_cold(const ScanConst *kc_in, double x, double y, double c, double s, double d, int &hit_r,
                                int &hit_c, int &lookups)
{
    // volatile: every constant is re-read where it is used instead of living in a register for the
    // whole loop; this path runs for about one ray in 10^7, its footprint matters, its speed does not
    const volatile ScanConst *kc = kc_in;
    double total = d;
    int n = 1;
    while (d > kc->eps && total <= kc->max_range) {
        x += d * c;
        y += d * s;
        const double xt = x - kc->orig_x, yt = y - kc->orig_y;
        double xr = xt, yr = yt;
        if (!IDENT) {
            const double oc = kc->orig_c, os = kc->orig_s;
            xr = xt * oc + yt * os;
            yr = -xt * os + yt * oc;
        }
        const double res = kc->res;
        hit_r = -1;
        hit_c = -1;
        d = kc->oob_value;
        if ((xr >= 0) & (xr < (double)kc->width * res) & (yr >= 0) & (yr < (double)kc->height * res)) {
            hit_c = (int)(xr / res);
            hit_r = (int)(yr / res);
            const char *base = reinterpret_cast<const char *>(kc->table_rm);
            d = *reinterpret_cast<const double *>(base + (mul24((uint32_t)hit_r, (uint32_t)kc->row_bytes) + ((uint32_t)hit_c << 3)));
        }
        total += d;
        ++n;
    }
    lookups = n;
    const double max_range = kc->max_range;
    return (total > max_range) ? max_range : total;
}

// get_scan :166-172
F110_HD double scan_start_index(const ScanConst &k, double pose_theta)
{
    double ti = k.theta_dis * (pose_theta - k.fov / 2.) / (2. * kPi);
    // fmod(x, y) == x whenever |x| < |y| (exactly): with the yaw wrapped to [0, 2 pi] that is every call, and the
    // library fmod is a loop of a few hundred dependent instructions on k_integrate's chain
    if (!(fabs(ti) < (double)k.theta_dis)) ti = fmod(ti, (double)k.theta_dis);
    while (ti < 0) ti += k.theta_dis;
    return ti;
}

// int(theta_index) of beam i (:124 with the running index of :177-184).  The reference adds
// theta_index_increment i times in floating point; start + i*inc reproduces that to ~1e-10, so
// the truncation is decided in closed form unless the value is within dir_guard of an integer,
// in which case the sequential additions are replayed exactly.
F110_HD int beam_dir_index(const ScanConst &k, double start, int i)
{
    const double td = (double)k.theta_dis;
    // closed form (approximate on purpose: explicit FMAs, reciprocal instead of a division);
    // any value that lands within dir_guard of an integer — which includes the wrap points 0 and
    // theta_dis — is recomputed exactly below
    double t = fma((double)i, k.theta_inc, start);
    t = fma(-floor(t * k.inv_theta_dis), td, t);
    const double fr = t - floor(t);
    if (!(fabs(fr - 0.5) < 0.5 - k.dir_guard)) {
        double ti = start;
        for (int j = 0; j < i; ++j) {
            ti += k.theta_inc;
            while (ti >= td) ti -= td;
        }
        t = ti;
    }
    int idx = (int)t;
    // theta_index == theta_dis can only arise from start + theta_dis rounding (:172); the
    // reference would then index one past the table — clamp instead of reading out of bounds.
    return idx >= k.theta_dis ? k.theta_dis - 1 : idx;
}

// The agent-aligned scan's task order (k_scan_rays_agent without a per-env order): task id -> (agent of the launch, 64-beam
// sector of its scan), walking an env's agents sector by sector: env = task / (tpa * A), sector = (task % (tpa * A)) / A,
// agent in env = task % A (tpa * A is a multiple of A).  Consecutive tasks are then the SAME 64 beams of one env's cars, which
// share their noise row.  A = 1 is the agent-major order (agent = task / tpa, sector = task % tpa).  A bijection from
// [0, E * A * tpa) onto [0, E * A) x [0, tpa).
// One division, as the agent-major order had: the small remainder is divided by A through a reciprocal the host passes,
// inv_A = scan_task_inv(A) = floor(2^32 / A) + 1 (0 for A = 1: nothing to divide).  With inv_A * A = 2^32 + e, 0 < e <= A,
// umulhi(rem, inv_A) == rem / A whenever rem * e < 2^32, and rem < tpa * A: exact for tpa * A * A <= 2^32 (scan_task_inv_ok;
// a launch beyond that walks agent-major, A = 1).
F110_HD uint32_t scan_task_inv(uint32_t A) { return A > 1u ? (uint32_t)(0x100000000ull / A) + 1u : 0u; }
F110_HD bool scan_task_inv_ok(uint32_t tpa, uint32_t A) { return (unsigned long long)tpa * A * A <= 0x100000000ull; }
F110_HD void scan_task_agent(uint32_t task, uint32_t tpa, uint32_t A, uint32_t inv_A, uint32_t &agent, uint32_t &sector)
{
    const uint32_t tpe = tpa * A, env = task / tpe, rem = task - env * tpe;
    sector = inv_A ? (uint32_t)(((unsigned long long)rem * inv_A) >> 32) : rem;
    agent = env * A + (rem - sector * A);
}

// check_ttc_jit :188-217 — one beam's predicate
F110_HD bool ttc_beam_hit(double range, double side_distance, double vel, double beam_cos, double thresh)
{
    // ttc = (scan[i] - side_distances[i]) / (vel*cosines[i]);  hit <=> 0 <= ttc < thresh.
    // Decided without the float64 division unless |num| is within 1e-12 (relative) of
    // thresh*|den| — there, and for NaN / 0/0, the reference expression itself is evaluated.
    const double proj_vel = vel * beam_cos;
    const double num = range - side_distance;
    const double a = fabs(num), b = fabs(proj_vel);
    if (a < (thresh * (1.0 - 1e-12)) * b) return (num == 0.0) || ((num > 0.0) == (proj_vel > 0.0));
    if (a > (thresh * (1.0 + 1e-12)) * b) return false;
    const double ttc = num / proj_vel;
    return (ttc < thresh) && (ttc >= 0.0);
}

// get_range :249-280 with v3 = (cos, sin)(beam_theta + pi/2) supplied by the caller
F110_HD double edge_range(double ox, double oy, double v3x, double v3y, double vax, double vay,
                          double vbx, double vby)
{
    const double v1x = ox - vax, v1y = oy - vay;
    const double v2x = vbx - vax, v2y = vby - vay;
    const double denom = v2x * v3x + v2y * v3y;
    double distance = INFINITY;
    if (fabs(denom) > 0.0) {
        // (round 4 tried deciding hit / miss on the numerators and dividing only for an edge that is hit — bit-identical,
        // tests/test_host_math.py keeps the equivalence test — and lost at every size: 65 536 x 2 agents 95.7 -> 94.6 M
        // agent-steps/s, 16 cars per env 70.6 -> 64.2: the divisions pipeline across the four edges, the branches do not)
        const double d1 = (v2x * v1y - v2y * v1x) / denom;
        const double d2 = (v1x * v3x + v1y * v3y) / denom;
        if (d1 >= 0.0 && d2 >= 0.0 && d2 <= 1.0) distance = d1;
    } else {
        // are_collinear(o, va, vb) :232-247
        const double bax = vax - ox, bay = vay - oy;
        const double cax = ox - vbx, cay = oy - vby;
        if (fabs(bax * cay - bay * cax) < 1e-8) {
            const double da = sqrt(bax * bax + bay * bay);
            const double dbx = vbx - ox, dby = vby - oy;
            const double db = sqrt(dbx * dbx + dby * dby);
            distance = da < db ? da : db;
        }
    }
    return distance;
}

// first index minimising |scan_angles[i] - a| (np.argmin, :310-313).  scan_angles is strictly
// increasing (base_classes.py:133-134), so the minimum sits next to the closed-form estimate;
// a +-3 neighbourhood is scanned with the reference's own comparison.
F110_HD int nearest_beam(const double *scan_angles, int num_beams, double angle_inc, double a)
{
    double est = (a - scan_angles[0]) / angle_inc;
    int i0 = est < 0 ? 0 : (est > (double)(num_beams - 1) ? num_beams - 1 : (int)est);
    int lo = i0 - 3 < 0 ? 0 : i0 - 3;
    int hi = i0 + 3 > num_beams - 1 ? num_beams - 1 : i0 + 3;
    int best = lo;
    double bv = fabs(scan_angles[lo] - a);
    for (int i = lo + 1; i <= hi; ++i) {
        const double v = fabs(scan_angles[i] - a);
        if (v < bv) {
            bv = v;
            best = i;
        }
    }
    return best;
}

// np.argmin(np.abs(scan_angles - a)) as the reference evaluates it (:310-313): every entry, first minimum wins (a NaN entry
// wins over every number, as in NumPy).  For tables that are not the uniform ramp of base_classes.py:133-134 — the free
// functions ray_cast / check_ttc_jit accept any scan_angles array (unit entry points only: f110_raycast_batch).
F110_HD int nearest_beam_full(const double *scan_angles, int num_beams, double a)
{
    int best = 0;
    double bv = fabs(scan_angles[0] - a);
    for (int i = 1; i < num_beams; ++i) {
        const double v = fabs(scan_angles[i] - a);
        if (v < bv || (v != v && bv == bv)) {
            bv = v;
            best = i;
        }
    }
    return best;
}

// the angle get_blocked_view_indices looks up for one vertex (:296-309): -(heading - direction), wrapped once
F110_HD double vertex_view_angle(double ex, double ey, double etheta, double vx, double vy)
{
    const double dx = vx - ex, dy = vy - ey;
    const double norm = sqrt(dx * dx + dy * dy);
    const double ux = dx / norm, uy = dy / norm;
    double ce, se;
    cos_sin(etheta, ce, se);
    double angle = atan2(se, ce) - atan2(uy, ux);
    if (angle > kPi)
        angle = angle - 2 * kPi;
    else if (angle < -kPi)
        angle = angle + 2 * kPi;
    return -angle;
}

// one vertex's beam index of get_blocked_view_indices :282-315
// get_blocked_view_indices :296-311 for one vertex, with its two arc tangents supplied:
// head = atan2(sin(etheta), cos(etheta)), dir = atan2(uy, ux) of the normalised lidar -> vertex vector
F110_HD int vertex_beam_from_angles(double head, double dir, const double *scan_angles, int num_beams, double angle_inc)
{
    double angle = head - dir;
    if (angle > kPi)
        angle = angle - 2 * kPi;
    else if (angle < -kPi)
        angle = angle + 2 * kPi;
    return nearest_beam(scan_angles, num_beams, angle_inc, -angle);
}

F110_HD int vertex_beam_index(double ex, double ey, double etheta, double vx, double vy,
                              const double *scan_angles, int num_beams, double angle_inc)
{
    const double dx = vx - ex, dy = vy - ey;
    const double norm = sqrt(dx * dx + dy * dy);
    const double ux = dx / norm, uy = dy / norm;
    double ce, se;
    cos_sin(etheta, ce, se);
    return vertex_beam_from_angles(atan2(se, ce), atan2(uy, ux), scan_angles, num_beams, angle_inc);
}

// Conservative beam-index range whose rays can touch a disc (centre c, radius R) seen from the
// ego at (ex, ey, eth).  ray_cast (:338-345) evaluates every beam of [min_ind, max_ind] against
// the opponent's four edges, but a beam whose ray misses the box's circumscribed disc returns
// inf from all four get_range calls and leaves the scan untouched — skipping it is
// result-preserving.  (When the opponent straddles the rear +-pi direction the reference window
// degenerates to all B beams although none of them can hit: this cull removes that work.)
// Beams are sa[0] + b*inc to within rounding; the range is padded by 3 beams + 1e-6 rad.
// disc_beam_range with dist = |centre - lidar|, dir = atan2(dy, dx) and head = atan2(sin(eth), cos(eth)) supplied
F110_HD void disc_beam_range_from(double dist, double eth, double dir, double head, double R, const double *scan_angles, int num_beams,
                                  double angle_inc, int &cl, int &ch)
{
    // No cull when the lidar is inside / on the disc (or anything is NaN), and none when the
    // heading is astronomically large: the reference wraps yaw by a single 2*pi per step
    // (base_classes.py:400-404), so a diverged yaw rate leaves |yaw| ~ 1e15, where
    // pose[2] + scan_angles[i] (:343) is rounded to a grid coarser than the beam spacing and the
    // beams no longer point where their index says.  Below 1e6 that rounding is < 1e-10 rad.
    if (!(dist > R * 1.000001 + 1e-9) || !(fabs(eth) < 1e6)) {
        cl = 0;
        ch = num_beams - 1;
        return;
    }
    double phi = dir - head;
    phi -= kTwoPi * rint(phi / kTwoPi);  // (-pi, pi]
    const double psi = asin(R / dist) + 3.0 * angle_inc + 1e-6;
    const double sa0 = scan_angles[0];
    const double last = (double)(num_beams - 1);
    cl = num_beams;
    ch = -1;
#pragma unroll
    for (int k = -1; k <= 1; ++k) {
        double lo = ceil((phi + kTwoPi * k - psi - sa0) / angle_inc);
        double hi = floor((phi + kTwoPi * k + psi - sa0) / angle_inc);
        lo = lo < 0.0 ? 0.0 : lo;
        hi = hi > last ? last : hi;
        if (lo <= hi) {
            cl = (int)lo < cl ? (int)lo : cl;
            ch = (int)hi > ch ? (int)hi : ch;
        }
    }
}

F110_HD void disc_beam_range(double ex, double ey, double eth, double cx, double cy, double R,
                             const double *scan_angles, int num_beams, double angle_inc, int &cl, int &ch)
{
    const double dx = cx - ex, dy = cy - ey;
    const double dist = sqrt(dx * dx + dy * dy);
    if (!(dist > R * 1.000001 + 1e-9) || !(fabs(eth) < 1e6)) {   // before any trigonometry, as it always was
        cl = 0;
        ch = num_beams - 1;
        return;
    }
    double ce, se;
    cos_sin(eth, ce, se);
    disc_beam_range_from(dist, eth, atan2(dy, dx), atan2(se, ce), R, scan_angles, num_beams, angle_inc, cl, ch);
}

// get_blocked_view_indices :282-315 (min/max of the four vertex beam indices) intersected with
// the disc cull above.  Returns an empty range (hi < lo) when no beam of the window can hit.
F110_HD void opponent_beam_window(double ex, double ey, double eth, const double *v, double cx, double cy,
                                  double R, const double *scan_angles, int num_beams, double angle_inc,
                                  int &ref_lo, int &ref_hi, int &lo, int &hi)
{
    const int i0 = vertex_beam_index(ex, ey, eth, v[0], v[1], scan_angles, num_beams, angle_inc);
    const int i1 = vertex_beam_index(ex, ey, eth, v[2], v[3], scan_angles, num_beams, angle_inc);
    const int i2 = vertex_beam_index(ex, ey, eth, v[4], v[5], scan_angles, num_beams, angle_inc);
    const int i3 = vertex_beam_index(ex, ey, eth, v[6], v[7], scan_angles, num_beams, angle_inc);
    int a = i0 < i1 ? i0 : i1, b = i2 < i3 ? i2 : i3;
    ref_lo = a < b ? a : b;
    a = i0 > i1 ? i0 : i1;
    b = i2 > i3 ? i2 : i3;
    ref_hi = a > b ? a : b;
    int cl, ch;
    disc_beam_range(ex, ey, eth, cx, cy, R, scan_angles, num_beams, angle_inc, cl, ch);
    lo = ref_lo > cl ? ref_lo : cl;
    hi = ref_hi < ch ? ref_hi : ch;
}

// the four get_range calls of ray_cast's inner loop (:341-345) for one beam
// (V: const double * — or a volatile pointer into LDS: every corner read where its edge uses it, see finalize_pair_wave_body)
template <typename V>
F110_HD double box_range_from(double ex, double ey, double v3x, double v3y, V v, double r)
{
    double rr = edge_range(ex, ey, v3x, v3y, v[0], v[1], v[2], v[3]);
    if (rr < r) r = rr;
    rr = edge_range(ex, ey, v3x, v3y, v[2], v[3], v[4], v[5]);
    if (rr < r) r = rr;
    rr = edge_range(ex, ey, v3x, v3y, v[4], v[5], v[6], v[7]);
    if (rr < r) r = rr;
    rr = edge_range(ex, ey, v3x, v3y, v[6], v[7], v[0], v[1]);
    if (rr < r) r = rr;
    return r;
}

F110_HD double box_range(double ex, double ey, double v3x, double v3y, const double *v, double r)
{
    return box_range_from<const double *>(ex, ey, v3x, v3y, v, r);
}

// ------------------------------------------------------------------ collision_models.py
// get_vertices :218-260 — order [rl, rr, fr, fl]; v[2*i], v[2*i+1]
F110_HD void box_vertices(double x, double y, double th, double length, double width, double *v)
{
    double c, s;
    cos_sin(th, c, s);
    const double hx = length / 2, hy = width / 2;
    const double bx[4] = {-hx, -hx, hx, hx};
    const double by[4] = {hy, -hy, -hy, hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = ((c * bx[i] + (-s) * by[i]) + 0.) + x;
        v[2 * i + 1] = ((s * bx[i] + c * by[i]) + 0.) + y;
    }
}

// the same with cos / sin of the heading supplied (computed once per agent by the caller)
F110_HD void box_vertices_cs(double x, double y, double c, double s, double length, double width, double *v)
{
    const double hx = length / 2, hy = width / 2;
    const double bx[4] = {-hx, -hx, hx, hx};
    const double by[4] = {hy, -hy, -hy, hy};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[2 * i] = ((c * bx[i] + (-s) * by[i]) + 0.) + x;
        v[2 * i + 1] = ((s * bx[i] + c * by[i]) + 0.) + y;
    }
}

// (V: const double * — or a volatile pointer into LDS: every vertex read where it is used, see finalize_pair_wave_body)
template <typename V>
F110_HD int furthest_vertex(V v, double dx, double dy)
{
    int best = 0;
    double bv = v[0] * dx + v[1] * dy;
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const double val = v[2 * i] * dx + v[2 * i + 1] * dy;
        if (val > bv) {
            bv = val;
            best = i;
        }
    }
    return best;
}

template <typename V>
F110_HD void minkowski_support(V v1, V v2, double dx, double dy, double &ax, double &ay)
{
    const int i = furthest_vertex(v1, dx, dy);
    const int j = furthest_vertex(v2, -dx, -dy);
    ax = v1[2 * i] - v2[2 * j];
    ay = v1[2 * i + 1] - v2[2 * j + 1];
}

// tripleProduct(a, b, c) = b*(a.c) - a*(b.c)  :51-64
F110_HD void triple_product(double ax, double ay, double bx, double by, double cx, double cy, double &ox, double &oy)
{
    const double ac = ax * cx + ay * cy;
    const double bc = bx * cx + by * cy;
    ox = bx * ac - ax * bc;
    oy = by * ac - ay * bc;
}

// collision (GJK) :113-182 on two 4-vertex convex bodies
template <typename V>
F110_HD bool gjk_overlap_from(V v1, V v2)
{
    // simplex slots kept in scalars (no runtime-indexed arrays -> no scratch on gfx950)
    double s0x, s0y, s1x = 0, s1y = 0;
    double dx = (((v1[0] + v1[2]) + v1[4]) + v1[6]) / 4 - (((v2[0] + v2[2]) + v2[4]) + v2[6]) / 4;
    double dy = (((v1[1] + v1[3]) + v1[5]) + v1[7]) / 4 - (((v2[1] + v2[3]) + v2[5]) + v2[7]) / 4;
    if (dx == 0 && dy == 0) dx = 1.0;
    double ax, ay;
    minkowski_support(v1, v2, dx, dy, ax, ay);
    s0x = ax;
    s0y = ay;
    if (dx * ax + dy * ay <= 0) return false;
    dx = -ax;
    dy = -ay;
    int index = 0;
    for (int iter = 0; iter < 1000;) {
        minkowski_support(v1, v2, dx, dy, ax, ay);
        index += 1;
        if (dx * ax + dy * ay <= 0) return false;
        const double aox = -ax, aoy = -ay;
        if (index < 2) {
            // line case: new point becomes simplex[1]
            s1x = ax;
            s1y = ay;
            const double abx = s0x - ax, aby = s0y - ay;
            triple_product(abx, aby, aox, aoy, abx, aby, dx, dy);
            if (sqrt(dx * dx + dy * dy) < 1e-10) {  // perpendicular(ab) :34-48
                dx = aby;
                dy = -1 * abx;
            }
            continue;
        }
        // triangle case: a = simplex[2], b = simplex[1], c = simplex[0]
        const double abx = s1x - ax, aby = s1y - ay;
        const double acx = s0x - ax, acy = s0y - ay;
        double px, py;
        triple_product(abx, aby, acx, acy, acx, acy, px, py);  // acperp
        if (px * aox + py * aoy >= 0) {
            dx = px;
            dy = py;
        } else {
            triple_product(acx, acy, abx, aby, abx, aby, px, py);  // abperp
            if (px * aox + py * aoy < 0) return true;
            s0x = s1x;
            s0y = s1y;
            dx = px;
            dy = py;
        }
        s1x = ax;
        s1y = ay;
        index -= 1;
        ++iter;
    }
    return false;
}

F110_HD bool gjk_overlap(const double *v1, const double *v2) { return gjk_overlap_from<const double *>(v1, v2); }

// ------------------------------------------------------------------ examples/waypoint_follow.py
// The reference's example policy (PurePursuitPlanner), so a closed loop can stay on the GPU.
// waypoints [M][3] = (x, y, speed).

// nearest_point_on_trajectory :15-50: projection on every segment, parameter clipped to [0,1],
// first segment with the smallest distance (np.argmin)
F110_HD int nearest_on_trajectory(const double *wp, int M, double px, double py, double &dist, double &t_best)
{
    int best = 0;
    dist = INFINITY;
    t_best = 0.0;
    for (int k = 0; k + 1 < M; ++k) {
        const double ax = wp[3 * k], ay = wp[3 * k + 1];
        const double dx = wp[3 * k + 3] - ax, dy = wp[3 * k + 4] - ay;
        double t = ((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy);
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double rx = px - (ax + t * dx), ry = py - (ay + t * dy);
        const double d = sqrt(rx * rx + ry * ry);
        if (d < dist) {
            dist = d;
            t_best = t;
            best = k;
        }
    }
    return best;
}

// does the look-ahead circle cut the segment s -> e (+1e-6 on e, :70)?  In the segment the search
// starts in only parameters >= t_min count (:86-96); elsewhere t_min = 0.
F110_HD bool lookahead_cuts(double sx, double sy, double ex, double ey, double px, double py, double radius, double t_min)
{
    const double vx = (ex + 1e-6) - sx, vy = (ey + 1e-6) - sy;
    const double a = vx * vx + vy * vy;
    const double b = 2.0 * (vx * (sx - px) + vy * (sy - py));
    const double c = (sx * sx + sy * sy) + (px * px + py * py) - 2.0 * (sx * px + sy * py) - radius * radius;
    const double disc = b * b - 4 * a * c;
    if (disc < 0) return false;
    const double root = sqrt(disc);
    const double t1 = (-b - root) / (2.0 * a), t2 = (-b + root) / (2.0 * a);
    return (t1 >= 0.0 && t1 <= 1.0 && t1 >= t_min) || (t2 >= 0.0 && t2 <= 1.0 && t2 >= t_min);
}

// first_point_on_trajectory_intersecting_circle :52-132 (wrap=True) -> index of the waypoint the
// planner then steers to (the segment's first waypoint; M-1 for the closing segment, which the
// reference reaches as wpts[-1]), or -1
F110_HD int first_waypoint_on_circle(const double *wp, int M, double px, double py, double radius, double start)
{
    const int start_i = (int)start;
    const double start_t = fmod(start, 1.0);
    for (int i = start_i; i + 1 < M; ++i)
        if (lookahead_cuts(wp[3 * i], wp[3 * i + 1], wp[3 * i + 3], wp[3 * i + 4], px, py, radius, i == start_i ? start_t : 0.0))
            return i;
    for (int i = -1; i < start_i; ++i) {
        const int k0 = i < 0 ? M - 1 : i, k1 = i + 1;   // i in [-1, M-2]: Python's (i % M), ((i+1) % M)
        if (lookahead_cuts(wp[3 * k0], wp[3 * k0 + 1], wp[3 * k1], wp[3 * k1 + 1], px, py, radius, 0.0)) return k0;
    }
    return -1;
}

// PurePursuitPlanner.plan :203-217 with _get_current_waypoint :183-201 and get_actuation :134-145
F110_HD void pure_pursuit_plan(const double *wp, int M, double px, double py, double theta, double lookahead, double vgain,
                               double wheelbase, double max_reacquire, double &steer, double &speed)
{
    steer = 0.0;
    speed = 4.0;  // "no waypoint" action :213-214
    double dist, t;
    const int i = nearest_on_trajectory(wp, M, px, py, dist, t);
    int goal = i;
    if (dist < lookahead) {
        goal = first_waypoint_on_circle(wp, M, px, py, lookahead, (double)i + t);
        if (goal < 0) return;
    } else if (!(dist < max_reacquire)) {
        return;
    }
    // steer to the WAYPOINT `goal` (:193) at the speed of the NEAREST index (:195)
    const double wy = sin(-theta) * (wp[3 * goal] - px) + cos(-theta) * (wp[3 * goal + 1] - py);
    speed = vgain * wp[3 * i + 2];
    if (fabs(wy) < 1e-6) return;
    const double radius = 1 / (2.0 * wy / (lookahead * lookahead));
    steer = atan(wheelbase / radius);
}

// ------------------------------------------------------------------ compact observations (include/f110.h, f110_obs_spec)
// No reference counterpart.  Compares, float64 adds and divides, one float64 -> float32 conversion: no libm, nothing to contract.
constexpr int kObsFeatures = 8;
enum { OBS_POOL_MIN = 0, OBS_POOL_MEAN = 1, OBS_POOL_CENTER = 2 };

struct ObsRowSpec {
    int32_t W, K;         // beams used, sectors (the row pointer handed to obs_element starts at beam_lo)
    int32_t pool, D;      // D = K + nfeat
    int32_t nfeat;
    int32_t feat[kObsFeatures];          // feature j (in output order) reads source column feat[j]
    double clip, scale;
    double feat_scale[kObsFeatures];     // divisor of feature j (output order)
};

// np.minimum(v, clip): a NaN operand is the result
F110_HD double obs_minimum(double v, double clip) { return v != v ? v : (v < clip ? v : clip); }

// the lidar value of beams [b0, b1) of a row (relative to beam_lo): pooling, clip / scale / cast
F110_HD float obs_pool(const ObsRowSpec &s, const double *row, int b0, int b1)
{
    double v;
    if (s.pool == OBS_POOL_CENTER) {
        v = row[(b0 + b1 - 1) >> 1];
    } else if (s.pool == OBS_POOL_MEAN) {
        v = row[b0];
        for (int b = b0 + 1; b < b1; ++b) v = v + row[b];
        v = v / (double)(b1 - b0);
    } else {
        v = row[b0];
        for (int b = b0 + 1; b < b1; ++b) {
            const double r = row[b];
            v = (r < v || r != r) ? r : v;   // a NaN sticks: nothing compares below it and it is not replaced
        }
    }
    return (float)(obs_minimum(v, s.clip) / s.scale);
}

// lidar value k of a row: sector k covers beams floor(k W / K) .. floor((k + 1) W / K) exclusive
F110_HD float obs_sector(const ObsRowSpec &s, const double *row, int k)
{
    return obs_pool(s, row, (int)(((long long)k * s.W) / s.K), (int)(((long long)(k + 1) * s.W) / s.K));
}

F110_HD float obs_feature(double x, double divisor) { return (float)(x / divisor); }

// element j of the new frame: the K lidar values, then the features in bit order.  cols[c * stride] = source column c
F110_HD float obs_element(const ObsRowSpec &s, const double *row, const double *cols, size_t stride, int j)
{
    if (j < s.K) return obs_sector(s, row, j);
    const int f = j - s.K;
    return obs_feature(cols[(size_t)s.feat[f] * stride], s.feat_scale[f]);
}

// does this agent's stack start over (all frames = the new frame)?
F110_HD bool obs_episode_start(int step_count, int fill) { return fill != 0 || step_count == 1; }

// the whole update of one agent's stack [F][D], serially (the kernel spreads obs_element over a wave and moves the frames
// through LDS; this is the same rule in one place, and what the unit harness runs)
F110_HD void obs_update_stack(const ObsRowSpec &s, const double *row, const double *cols, size_t stride, int step_count, int fill,
                              int F, float *stack)
{
    const int D = s.D;
    if (obs_episode_start(step_count, fill)) {
        for (int j = 0; j < D; ++j) {
            const float v = obs_element(s, row, cols, stride, j);
            for (int f = 0; f < F; ++f) stack[(size_t)f * D + j] = v;
        }
        return;
    }
    for (size_t t = 0; t + D < (size_t)F * D; ++t) stack[t] = stack[t + D];
    for (int j = 0; j < D; ++j) stack[(size_t)(F - 1) * D + j] = obs_element(s, row, cols, stride, j);
}

// ------------------------------------------------------------------ follow the gap (include/f110.h, f110_gap_follower)
// No reference counterpart.  Compares, float64 adds, multiplies and divides, one ceil: no libm, nothing to contract.
enum { GAP_TARGET_CENTER = 0, GAP_TARGET_FURTHEST = 1 };

struct GapSpec {
    int32_t lo, W;        // first beam of the window, beams in it
    int32_t S, target;    // smoothing length (odd), GAP_TARGET_*
    double clip, bubble, thresh;
    double steer_gain, steer_max, v_lo, v_hi, d_ref, steer_slow, v_turn, v_blocked;
};

// step 1: the clipped range; a NaN beam counts as an obstacle at the car
F110_HD double gap_clip(double r, double clip) { return r != r ? 0.0 : (r < clip ? r : clip); }

// step 2: the mean of the clipped ranges v[a .. b) around beam i, every window summed on its own in ascending order
F110_HD double gap_window_mean(const double *v, int W, int S, int i)
{
    const int h = S >> 1;
    const int a = i - h > 0 ? i - h : 0, b = i + h + 1 < W ? i + h + 1 : W;
    double sum = 0.0;
    for (int k = a; k < b; ++k) sum = sum + v[k];
    return sum / (double)(b - a);
}

// step 4: the bubble's half-width in beams around the closest point (smoothed range pc)
F110_HD int gap_bubble_half(double pc, double inc, double radius, int W)
{
    const double den = pc * inc;
    const double kb = den > 0.0 ? radius / den : INFINITY;
    if (!(kb < (double)W)) return W;
    return (int)ceil(kb);
}

// step 5: is beam i (smoothed range pi) free?
F110_HD bool gap_free(double pi, int i, int c, int half, double thresh)
{
    const int d = i > c ? i - c : c - i;
    return d > half && pi > thresh;
}

// the runs of free beams of a contiguous chunk [start, start + len): the run at its lower end, the run at its upper end and its
// longest run (lowest start on equal length).  lead == len says every beam is free.  An empty chunk (len 0) is the identity.
struct GapRun {
    int32_t start, len, lead, trail, best, best_start;
};

// a chunk of up to 64 beams from its free bits (bit k = beam start + k; bits at and above len are clear)
F110_HD GapRun gap_run_of_mask(unsigned long long m, int start, int len)
{
    GapRun r;
    r.start = start;
    r.len = len;
    r.lead = ~m ? (int)__builtin_ctzll(~m) : 64;
    const unsigned long long top = len > 0 ? (m << (64 - len)) : 0ull;   // the chunk's last beam in bit 63
    r.trail = ~top ? (int)__builtin_clzll(~top) : 64;
    if (len == 0) r.lead = r.trail = 0;
    // x keeps the positions from which at least `best` free bits run upwards
    unsigned long long x = m;
    int best = 0, pos = 0;
    while (x) {
        ++best;
        pos = (int)__builtin_ctzll(x);
        x &= x >> 1;
    }
    r.best = best;
    r.best_start = start + pos;
    return r;
}

// a followed directly by b (a.start + a.len == b.start): associative.  The candidates for the longest run come in ascending
// start order (a's, the run across the seam, b's), so a later one wins only when it is strictly longer.
F110_HD GapRun gap_run_merge(const GapRun &a, const GapRun &b)
{
    GapRun r;
    r.start = a.start;
    r.len = a.len + b.len;
    r.lead = a.lead == a.len ? a.len + b.lead : a.lead;
    r.trail = b.trail == b.len ? b.len + a.trail : b.trail;
    r.best = a.best;
    r.best_start = a.best_start;
    const int seam = a.trail + b.lead;
    if (seam > r.best) {
        r.best = seam;
        r.best_start = b.start - a.trail;
    }
    if (b.best > r.best) {
        r.best = b.best;
        r.best_start = b.best_start;
    }
    return r;
}

F110_HD double gap_beam_angle(double fov, int B, int beam)
{
    const double inc = fov / (double)(B - 1);
    return -fov / 2. + inc * (double)beam;
}

// step 7: the action from the target beam's angle and its smoothed range
F110_HD void gap_action(const GapSpec &s, double angle, double pt, double &steer, double &speed)
{
    steer = s.steer_gain * angle;
    steer = steer > s.steer_max ? s.steer_max : (steer < -s.steer_max ? -s.steer_max : steer);
    const double f = pt / s.d_ref;
    speed = s.v_lo + (s.v_hi - s.v_lo) * (f < 1. ? f : 1.);
    if (fabs(steer) > s.steer_slow) speed = speed < s.v_turn ? speed : s.v_turn;
}

// one agent's whole rule, serially (the kernel spreads the same pieces over a wave; this is what the unit harness runs).
// row = the agent's B ranges; v, p: scratch of W doubles each; info (or null) = c, half-width, g0, g1, t (-1s when blocked or
// when step_count is 0)
F110_HD void gap_follow_row(const GapSpec &s, const double *row, int B, double fov, int step_count, double *v, double *p,
                            double *action, int32_t *info)
{
    if (info)
        for (int k = 0; k < 5; ++k) info[k] = -1;
    if (step_count == 0) {
        action[0] = 0.0;
        action[1] = 0.0;
        return;
    }
    const int W = s.W;
    for (int i = 0; i < W; ++i) v[i] = gap_clip(row[s.lo + i], s.clip);
    int c = 0;
    for (int i = 0; i < W; ++i) {
        p[i] = gap_window_mean(v, W, s.S, i);
        if (p[i] < p[c]) c = i;
    }
    const int half = gap_bubble_half(p[c], fov / (double)(B - 1), s.bubble, W);
    GapRun all{};
    for (int i0 = 0; i0 < W; i0 += 64) {
        const int len = W - i0 < 64 ? W - i0 : 64;
        unsigned long long m = 0;
        for (int k = 0; k < len; ++k) m |= (unsigned long long)gap_free(p[i0 + k], i0 + k, c, half, s.thresh) << k;
        all = gap_run_merge(all, gap_run_of_mask(m, i0, len));
    }
    if (info) info[0] = c, info[1] = half;
    if (all.best == 0) {
        action[0] = 0.0;
        action[1] = s.v_blocked;
        return;
    }
    const int g0 = all.best_start, g1 = g0 + all.best;
    int t = (g0 + g1 - 1) >> 1;
    if (s.target == GAP_TARGET_FURTHEST) {
        t = g0;
        for (int i = g0 + 1; i < g1; ++i)
            if (p[i] > p[t]) t = i;
    }
    if (info) info[2] = g0, info[3] = g1, info[4] = t;
    gap_action(s, gap_beam_angle(fov, B, s.lo + t), p[t], action[0], action[1]);
}

// ------------------------------------------------------------------ track preview (include/f110.h, f110_track_preview)
// No reference counterpart.  Float64 adds, multiplies, divides and compares, nothing to contract; the EGO frame's one cos_sin is
// the only libm call.
enum { PREVIEW_FRAME_EGO = 0, PREVIEW_FRAME_WORLD = 1 };
enum { PREVIEW_NCHANNELS = 8, PREVIEW_MAX_ATTRS = 4 };

struct PreviewSpec {
    int32_t P, channels;   // stations; channel bits
    int32_t frame, D;      // PREVIEW_FRAME_*; popcount(channels)
    double offset, spacing;
    double scale[PREVIEW_NCHANNELS];
};

// a track as the preview reads it: the segment columns [7][nseg] (ax, ay, dx, dy, l2, len, cum) and the attributes [C][npts]
struct PreviewTrack {
    const double *cols;
    const double *attr;   // or null (C == 0)
    int32_t nseg, closed, C, npts;
    double L;
};

// station j's arc length: one wrap on a closed track
F110_HD double preview_station_s(double s, double offset, double spacing, int j, int closed, double L)
{
    const double d = offset + (double)j * spacing;
    double sj = s + d;
    if (closed && sj >= L) sj = sj - L;
    return sj;
}

// the last segment with cum[k] <= s, 0 when there is none (a NaN s: 0)
F110_HD int preview_segment(const double *cum, int nseg, double s)
{
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (cum[mid] <= s) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// np.clip(t, 0, 1): NaN passes
F110_HD double preview_clip01(double t) { return t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t); }

// the eight channel values of the station at arc length sj in segment k, before scaling; (c, sn) = cos, sin of the pose's heading
// (read in the EGO frame only); an absent attribute is 0.0
F110_HD void preview_station(const PreviewTrack &tr, int k, double sj, int frame, double px, double py, double c, double sn, double *v)
{
    const size_t n = (size_t)tr.nseg;
    const double *q = tr.cols;
    const double ax = q[k], ay = q[n + k], dx = q[2 * n + k], dy = q[3 * n + k], len = q[5 * n + k], cum = q[6 * n + k];
    const double t = preview_clip01((sj - cum) / len);
    const double X = ax + t * dx, Y = ay + t * dy;
    const double ux = dx / len, uy = dy / len;
    if (frame == PREVIEW_FRAME_WORLD) {
        v[0] = X;
        v[1] = Y;
        v[2] = ux;
        v[3] = uy;
    } else {
        const double rx = X - px, ry = Y - py;
        v[0] = c * rx + sn * ry;
        v[1] = c * ry - sn * rx;
        v[2] = c * ux + sn * uy;
        v[3] = c * uy - sn * ux;
    }
    const int k1 = k + 1 == tr.npts ? 0 : k + 1;   // (only a closed track's last segment ends at point 0)
#pragma unroll
    for (int a = 0; a < PREVIEW_MAX_ATTRS; ++a) {
        double w = 0.0;
        if (a < tr.C) {
            const double a0 = tr.attr[(size_t)a * tr.npts + k], a1 = tr.attr[(size_t)a * tr.npts + k1];
            w = a0 + t * (a1 - a0);
        }
        v[4 + a] = w;
    }
}

// one output element: a float64 divide, then the conversion (round to nearest even)
F110_HD float preview_scaled(double v, double scale) { return (float)(v / scale); }

// one row's whole preview, serially (the kernel gives every station a lane; this is what the unit harness runs).
// out [P][D], raw [P][8] or null, seg [P] or null
F110_HD void preview_row(const PreviewSpec &sp, const PreviewTrack &tr, double px, double py, double theta, double s, float *out,
                         double *raw, int32_t *seg)
{
    double c = 1.0, sn = 0.0;
    if (sp.frame == PREVIEW_FRAME_EGO) cos_sin(theta, c, sn);
    const double *cum = tr.cols + 6 * (size_t)tr.nseg;
    for (int j = 0; j < sp.P; ++j) {
        const double sj = preview_station_s(s, sp.offset, sp.spacing, j, tr.closed, tr.L);
        const int k = preview_segment(cum, tr.nseg, sj);
        double v[PREVIEW_NCHANNELS];
        preview_station(tr, k, sj, sp.frame, px, py, c, sn, v);
        float *o = out + (size_t)j * sp.D;
        for (int b = 0; b < PREVIEW_NCHANNELS; ++b) {
            if (raw) raw[(size_t)j * PREVIEW_NCHANNELS + b] = v[b];
            if (sp.channels >> b & 1) *o++ = preview_scaled(v[b], sp.scale[b]);
        }
        if (seg) seg[j] = k;
    }
}

// ------------------------------------------------------------------ neighbours (include/f110.h, f110_neighbors)
// No reference counterpart.  Float64 adds, multiplies, divides, compares and one sqrt, nothing to contract; the one cos_sin per
// agent is the only libm call.
enum { NBR_DX = 0, NBR_DY, NBR_DIST, NBR_COS_DTH, NBR_SIN_DTH, NBR_V_X, NBR_V_Y, NBR_GAP_S, NBR_VALID, NBR_INDEX, NBR_NCHANNELS };
enum { NBR_MAX_K = 8, NBR_MAX_AGENTS = 256 };

struct NbrSpec {
    int32_t K, channels;   // slots; channel bits
    int32_t D, KT;         // popcount(channels); the kept list's length: the power of two >= K
    double R2, pad;        // max_range * max_range; what an empty slot holds
    double scale[NBR_NCHANNELS];
};

// one agent as its env's other agents see it
struct NbrAgent {
    double x, y, c, sn, v, s;
};

F110_HD double nbr_d2(double xa, double ya, double xb, double yb)
{
    const double rx = xb - xa, ry = yb - ya;
    return rx * rx + ry * ry;
}

// the KT best (d2, b) so far, ascending; idx < 0 marks an empty slot.  The candidates arrive in ascending b, so a strict compare
// leaves equal d2 in ascending b.  Fully unrolled over constant indices: d and idx live in named registers.
template <int KT>
struct NbrBest {
    double d[KT];
    int32_t idx[KT];
    F110_HD void clear()
    {
#pragma unroll
        for (int q = 0; q < KT; ++q) d[q] = 0.0, idx[q] = -1;
    }
    // candidate b at d2, already found eligible
    F110_HD void insert(double d2, int32_t b)
    {
#pragma unroll
        for (int q = KT - 1; q >= 0; --q) {
            const bool before = idx[q] < 0 || d2 < d[q];
            if (q + 1 < KT) {
                d[q + 1] = before ? d[q] : d[q + 1];
                idx[q + 1] = before ? idx[q] : idx[q + 1];
            }
            d[q] = before ? d2 : d[q];
            idx[q] = before ? b : idx[q];
        }
    }
    // candidate b of agent a: the eligibility rule, then the insertion (a NaN d2 fails the compare)
    F110_HD void offer(double d2, int32_t b, int32_t a, double R2)
    {
        if (b != a && d2 <= R2) insert(d2, b);
    }
};

// g = s_b - s_a, wrapped once on a closed track of length L (L == 0: no wrap)
F110_HD double nbr_gap(double sa, double sb, double L)
{
    double g = sb - sa;
    if (L > 0.0) {
        const double half = 0.5 * L;
        if (g > half) g = g - L;
        else if (g <= -half) g = g + L;
    }
    return g;
}

// the ten channel values of neighbour b (index ib) as a sees it, before scaling; only the bits of `mask` are evaluated, the rest 0.0
F110_HD void nbr_values(const NbrAgent &a, const NbrAgent &b, int32_t ib, double L, int32_t mask, double *v)
{
    const double rx = b.x - a.x, ry = b.y - a.y;
    const double cd = b.c * a.c + b.sn * a.sn, sd = b.sn * a.c - b.c * a.sn;
    v[NBR_DX] = a.c * rx + a.sn * ry;
    v[NBR_DY] = a.c * ry - a.sn * rx;
    v[NBR_DIST] = (mask >> NBR_DIST & 1) ? sqrt(rx * rx + ry * ry) : 0.0;
    v[NBR_COS_DTH] = cd;
    v[NBR_SIN_DTH] = sd;
    v[NBR_V_X] = b.v * cd - a.v;
    v[NBR_V_Y] = b.v * sd;
    v[NBR_GAP_S] = (mask >> NBR_GAP_S & 1) ? nbr_gap(a.s, b.s, L) : 0.0;
    v[NBR_VALID] = 1.0;
    v[NBR_INDEX] = (double)ib;
}

// one output element of a filled slot: a float64 divide, then the conversion (round to nearest even)
F110_HD float nbr_scaled(double v, double scale) { return (float)(v / scale); }
// ... and of an empty one
F110_HD float nbr_empty(int bit, double pad) { return bit == NBR_VALID ? 0.0f : (float)pad; }

// slot k's D floats at o (and its ten raw values and its index) from the winner b with index ib (< 0: none, b is not read)
F110_HD void nbr_slot(const NbrSpec &sp, const NbrAgent &a, const NbrAgent &b, int32_t ib, double L, float *o, double *raw, int32_t *idx)
{
    double v[NBR_NCHANNELS] = {};
    if (ib >= 0) nbr_values(a, b, ib, L, raw ? (1 << NBR_NCHANNELS) - 1 : sp.channels, v);
#pragma unroll
    for (int bit = 0; bit < NBR_NCHANNELS; ++bit) {
        if (raw) raw[bit] = ib >= 0 ? v[bit] : (bit == NBR_VALID ? 0.0 : sp.pad);
        if (sp.channels >> bit & 1) *o++ = ib >= 0 ? nbr_scaled(v[bit], sp.scale[bit]) : nbr_empty(bit, sp.pad);
    }
    if (idx) *idx = ib;
}

// one env, serially (the kernel gives every agent a lane; this is what the unit harness runs): rows [A][5] = x, y, theta, v, s;
// out [A][K][D], raw [A][K][10] or null, idx [A][K] or null
template <int KT>
F110_HD void nbr_env(const NbrSpec &sp, const double *rows, int A, double L, NbrAgent *env, float *out, double *raw, int32_t *idx)
{
    for (int a = 0; a < A; ++a) {
        const double *r = rows + 5 * (size_t)a;
        env[a].x = r[0];
        env[a].y = r[1];
        cos_sin(r[2], env[a].c, env[a].sn);
        env[a].v = r[3];
        env[a].s = r[4];
    }
    for (int a = 0; a < A; ++a) {
        NbrBest<KT> best;
        best.clear();
        for (int b = 0; b < A; ++b) best.offer(nbr_d2(env[a].x, env[a].y, env[b].x, env[b].y), b, a, sp.R2);
#pragma unroll
        for (int k = 0; k < KT; ++k) {
            if (k >= sp.K) break;
            const size_t slot = (size_t)a * sp.K + k;
            const int32_t ib = best.idx[k];
            nbr_slot(sp, env[a], env[ib >= 0 ? ib : a], ib, L, out + slot * sp.D, raw ? raw + slot * NBR_NCHANNELS : nullptr, idx ? idx + slot : nullptr);
        }
    }
}

// ------------------------------------------------------------------ line follower (include/f110.h, f110_line_follower)
// No reference counterpart.  Pure pursuit on the track of the agent's map slot, the speed from a track attribute, slower behind a
// car ahead.  Float64 adds, multiplies, divides and compares, nothing to contract; cos_sin and atan are the only libm calls and
// only lx, ly and steer sit behind them: no branch and no part of the speed does.
enum { LINE_MAX_SPECS = 8, LINE_MAX_AGENTS = 256, LINE_NRAW = 12, LINE_NINFO = 4 };
enum { LINE_RAW_LD = 0, LINE_RAW_ST, LINE_RAW_K, LINE_RAW_X, LINE_RAW_Y, LINE_RAW_TX, LINE_RAW_TY, LINE_RAW_LX, LINE_RAW_LY, LINE_RAW_VREF,
       LINE_RAW_LIM, LINE_RAW_SPEED };

struct LineSpec {
    double look_base, look_gain, look_min, look_max;
    double lane_offset, wheelbase, steer_max;
    double v_const, vgain, speed_look, lat_slow, v_recover;
    double follow_range, follow_gap, follow_gain, lane_width;
    double v_min, v_max;
    int32_t speed_attr, pad_;   // -1: v_const
};

// step 1: the lookahead distance; a NaN v gives look_min
F110_HD double line_lookahead(const LineSpec &sp, double v)
{
    double ld = sp.look_base + sp.look_gain * fabs(v);
    if (!(ld >= sp.look_min)) ld = sp.look_min;
    else if (ld > sp.look_max) ld = sp.look_max;
    return ld;
}

// steps 2 and 4: the arc length d ahead of s, the preview's station rule (one wrap on a closed track)
F110_HD double line_ahead(double s, double d, int closed, double L) { return preview_station_s(s, d, 0.0, 0, closed, L); }

// step 2: the station (X, Y) at arc length s_t in segment k, by the preview's station rule, and the target lane_offset to its left
F110_HD void line_target(const PreviewTrack &tr, int k, double s_t, double lane_offset, double &X, double &Y, double &Tx, double &Ty)
{
    PreviewTrack geo = tr;
    geo.C = 0;   // (the geometry channels only)
    double w[PREVIEW_NCHANNELS];
    preview_station(geo, k, s_t, PREVIEW_FRAME_WORLD, 0.0, 0.0, 1.0, 0.0, w);
    X = w[0];
    Y = w[1];
    Tx = X - lane_offset * w[3];
    Ty = Y + lane_offset * w[2];
}

// step 3: the target in the car's frame and the pure-pursuit steer, clamped
F110_HD double line_steer(const LineSpec &sp, double c, double sn, double px, double py, double Tx, double Ty, double &lx, double &ly)
{
    const double rx = Tx - px, ry = Ty - py;
    lx = c * rx + sn * ry;
    ly = c * ry - sn * rx;
    const double d2 = lx * lx + ly * ly;
    double steer = d2 > 0.0 ? atan(2.0 * sp.wheelbase * ly / d2) : 0.0;
    if (steer > sp.steer_max) steer = sp.steer_max;
    else if (steer < -sp.steer_max) steer = -sp.steer_max;
    return steer;
}

// step 4: attribute column c at arc length s in segment k, by the preview's attribute rule
F110_HD double line_attr(const PreviewTrack &tr, int c, int k, double s)
{
    const size_t n = (size_t)tr.nseg;
    const double len = tr.cols[5 * n + k], cum = tr.cols[6 * n + k];
    const double t = preview_clip01((s - cum) / len);
    const int k1 = k + 1 == tr.npts ? 0 : k + 1;
    const double a0 = tr.attr[(size_t)c * tr.npts + k], a1 = tr.attr[(size_t)c * tr.npts + k1];
    return a0 + t * (a1 - a0);
}

// step 4: the line's speed, or the recovery speed away from the lane
F110_HD double line_speed(const LineSpec &sp, double vref, double lat)
{
    double speed = sp.vgain * vref;
    if (fabs(lat - sp.lane_offset) > sp.lat_slow && sp.v_recover < speed) speed = sp.v_recover;
    return speed;
}

// step 5: car b (s_b, lat_b, v_b) as the car at (s, lat) sees it; L: the wrap length (0: none).  A NaN cap never wins.
F110_HD void line_offer(const LineSpec &sp, double s, double lat, double sb, double latb, double vb, double L, int b, double &speed, int &lim)
{
    const double g = nbr_gap(s, sb, L);
    if (g > 0.0 && g <= sp.follow_range && fabs(latb - lat) <= sp.lane_width) {
        const double cap = vb + sp.follow_gain * (g - sp.follow_gap);
        if (cap < speed) {
            speed = cap;
            lim = b;
        }
    }
}

// step 6
F110_HD double line_clamp(const LineSpec &sp, double speed)
{
    if (speed < sp.v_min) speed = sp.v_min;
    if (speed > sp.v_max) speed = sp.v_max;
    return speed;
}

// a row whose step_count is 0: the action (0, 0); raw (or null) all 0.0 but k and lim, which are -1.0
F110_HD void line_fresh(double *action, double *raw)
{
    action[0] = 0.0;
    action[1] = 0.0;
    if (raw) {
        for (int q = 0; q < LINE_NRAW; ++q) raw[q] = 0.0;
        raw[LINE_RAW_K] = -1.0;
        raw[LINE_RAW_LIM] = -1.0;
    }
}

// one env, serially (the kernel gives every agent a lane; this is what the unit harness runs): rows [A][7] = x, y, theta, v, s,
// lateral, step_count; actions [A][2], raw [A][12] or null
F110_HD void line_env(const LineSpec &sp, const PreviewTrack &tr, const double *rows, int A, double *actions, double *raw)
{
    const double *cum = tr.cols + 6 * (size_t)tr.nseg;
    const double Lw = tr.closed ? tr.L : 0.0;
    for (int a = 0; a < A; ++a) {
        const double *r = rows + 7 * (size_t)a;
        double *act = actions + 2 * (size_t)a, *rw = raw ? raw + (size_t)LINE_NRAW * a : nullptr;
        if (r[6] == 0.0) {
            line_fresh(act, rw);
            continue;
        }
        const double px = r[0], py = r[1], v = r[3], s = r[4], lat = r[5];
        const double ld = line_lookahead(sp, v);
        const double s_t = line_ahead(s, ld, tr.closed, tr.L);
        const int k = preview_segment(cum, tr.nseg, s_t);
        double X, Y, Tx, Ty, lx, ly, c, sn;
        line_target(tr, k, s_t, sp.lane_offset, X, Y, Tx, Ty);
        cos_sin(r[2], c, sn);
        const double steer = line_steer(sp, c, sn, px, py, Tx, Ty, lx, ly);
        const double s_v = line_ahead(s, sp.speed_look, tr.closed, tr.L);
        const double vref = sp.speed_attr >= 0 ? line_attr(tr, sp.speed_attr, preview_segment(cum, tr.nseg, s_v), s_v) : sp.v_const;
        double speed = line_speed(sp, vref, lat);
        int lim = -1;
        if (sp.follow_range > 0.0 && A > 1)
            for (int b = 0; b < A; ++b)
                if (b != a) line_offer(sp, s, lat, rows[7 * (size_t)b + 4], rows[7 * (size_t)b + 5], rows[7 * (size_t)b + 3], Lw, b, speed, lim);
        act[0] = steer;
        act[1] = line_clamp(sp, speed);
        if (rw) {
            rw[LINE_RAW_LD] = ld, rw[LINE_RAW_ST] = s_t, rw[LINE_RAW_K] = (double)k, rw[LINE_RAW_X] = X, rw[LINE_RAW_Y] = Y;
            rw[LINE_RAW_TX] = Tx, rw[LINE_RAW_TY] = Ty, rw[LINE_RAW_LX] = lx, rw[LINE_RAW_LY] = ly, rw[LINE_RAW_VREF] = vref;
            rw[LINE_RAW_LIM] = (double)lim, rw[LINE_RAW_SPEED] = speed;
        }
    }
}

// ------------------------------------------------------------------ rollout (include/f110.h, f110_rollout)
// No reference counterpart of its own: a candidate's motion is advance_vehicle (RaceCar.update_pose) called H * repeat times and its
// clearance sample_distance (xy_2_rc + the table) at the reference point, both called as they are.  What is added here is the
// bookkeeping around them (alive, the minimum, the frame, the scaling) and the projection of two poses on the track.
enum { ROLL_END_X = 0, ROLL_END_Y, ROLL_END_COS, ROLL_END_SIN, ROLL_END_V, ROLL_END_YAW_RATE, ROLL_ALIVE, ROLL_MIN_CLEAR, ROLL_PROGRESS,
       ROLL_END_LAT, ROLL_NCHANNELS };
enum { ROLL_SHARED = 0, ROLL_PER_AGENT = 1 };
enum { ROLL_FRAME_EGO = 0, ROLL_FRAME_WORLD = 1 };
enum { ROLL_MAX_K = 256, ROLL_MAX_H = 64, ROLL_MAX_REPEAT = 16 };
constexpr int32_t kRollTrackBits = 1 << ROLL_PROGRESS | 1 << ROLL_END_LAT;

struct RollSpec {
    int32_t K, H, repeat;       // candidates per agent; actions per candidate; sim steps an action is held
    int32_t layout, frame;      // ROLL_SHARED / ROLL_PER_AGENT; ROLL_FRAME_*
    int32_t channels, traj, D;  // channel bits; 1: the trajectory is written too; popcount(channels)
    double margin;
    double scale[ROLL_NCHANNELS];
};

// what a candidate starts from and carries: the agent's state, the steering FIFO (b0 the newest entry) and its fill
struct RollCar {
    double st[7], b0, b1;
    int cnt;
};

// the frame the poses are reported in: the start pose's (one cos_sin per agent) or the map's
struct RollFrame {
    double x0, y0, c0, s0;
    int ego;
};

F110_HD RollFrame roll_frame(int frame, double x, double y, double theta)
{
    RollFrame f{x, y, 1.0, 0.0, frame == ROLL_FRAME_EGO};
    if (f.ego) cos_sin(theta, f.c0, f.s0);
    return f;
}

// (x, y, cos, sin) of a pose in the frame; with_cs false leaves the heading's two values 0.0 (and its cos_sin out)
F110_HD void roll_pose(const RollFrame &f, double x, double y, double theta, bool with_cs, double *v)
{
    double c = 0.0, s = 0.0;
    if (with_cs) cos_sin(theta, c, s);
    if (!f.ego) {
        v[0] = x;
        v[1] = y;
        v[2] = c;
        v[3] = s;
        return;
    }
    const double rx = x - f.x0, ry = y - f.y0;
    v[0] = f.c0 * rx + f.s0 * ry;
    v[1] = f.c0 * ry - f.s0 * rx;
    v[2] = with_cs ? c * f.c0 + s * f.s0 : 0.0;
    v[3] = with_cs ? s * f.c0 - c * f.s0 : 0.0;
}

// one output element: a float64 divide, then the conversion (round to nearest even)
F110_HD float roll_scaled(double v, double scale) { return (float)(v / scale); }

// One candidate: H actions (steer, speed) at act[2 * h], each held `repeat` sim steps.  A step integrates, samples the clearance at
// the reference point and keeps the minimum; the first sample that is not above the margin (or a NaN position, which reads
// oob_value as every position outside the table does) kills the candidate: its state stays as that step left it.  The two loops are
// not unrolled: advance_vehicle is ~1900 dependent instructions and appears once.  With Emit::kOn, emit(h, v) receives the pose
// after action h's last repeat in the frame `fr` (read only then); every lane of a workgroup reaches every emit (a dead candidate
// repeats its pose).  An Emit that declares kXY = true also has emit.xy(h, x, y), which receives the same instant's MAP-frame
// position behind it, whatever `fr` is (the opponent term).
struct RollEmitNone {
    static constexpr bool kOn = false;
    F110_HD void operator()(int, const double *) const {}
};

template <class Emit, class = void>
struct RollEmitXY {
    static constexpr bool value = false;
};
template <class Emit>
struct RollEmitXY<Emit, decltype((void)Emit::kXY)> {
    static constexpr bool value = Emit::kXY;
};

template <class Emit>
F110_HD void roll_candidate(const RollSpec &sp, const ScanConst &k, const VehicleParams &vp, double dt, int integrator, double lidar_dist,
                            RollCar &car, const double *act, const RollFrame &fr, int &alive, double &min_clear, const Emit &emit)
{
    bool live = true;
    alive = 0;
    min_clear = INFINITY;
#pragma unroll 1
    for (int h = 0; h < sp.H; ++h) {
        const double steer = act[2 * h], speed = act[2 * h + 1];
#pragma unroll 1
        for (int r = 0; r < sp.repeat; ++r) {
            if (!live) continue;
            double scan_pose[3];
            advance_vehicle(car.st, car.b0, car.b1, car.cnt, steer, speed, vp, dt, integrator, lidar_dist, scan_pose);
            int row, col;
            const double d = sample_distance<LAYOUT_ROWMAJOR, false, false>(k, nullptr, car.st[0], car.st[1], row, col);
            if (!(d >= min_clear)) min_clear = d;
            live = d > sp.margin && car.st[0] == car.st[0] && car.st[1] == car.st[1];
            alive += live ? 1 : 0;
        }
        if (Emit::kOn) {
            double v[4];
            roll_pose(fr, car.st[0], car.st[1], car.st[4], true, v);
            emit(h, v);
        }
        if constexpr (RollEmitXY<Emit>::value) emit.xy(h, car.st[0], car.st[1]);
    }
}

// the channel values of a finished candidate before scaling; PROGRESS and END_LAT are the track pass's (0.0 here).  Only the bits
// of `mask` decide whether the end heading's cos_sin is taken.
F110_HD void roll_values(const RollFrame &fr, const RollCar &car, int alive, double min_clear, int32_t mask, double *v)
{
    roll_pose(fr, car.st[0], car.st[1], car.st[4], (mask & (1 << ROLL_END_COS | 1 << ROLL_END_SIN)) != 0, v);
    v[ROLL_END_V] = car.st[3];
    v[ROLL_END_YAW_RATE] = car.st[5];
    v[ROLL_ALIVE] = (double)alive;
    v[ROLL_MIN_CLEAR] = min_clear;
    v[ROLL_PROGRESS] = 0.0;
    v[ROLL_END_LAT] = 0.0;
}

// a candidate's row of the summary (and of the raw values): the bits of `which` are written, the other requested ones skipped
F110_HD void roll_store(const RollSpec &sp, const double *v, int32_t which, float *o, double *raw)
{
#pragma unroll
    for (int bit = 0; bit < ROLL_NCHANNELS; ++bit) {
        const bool mine = (which >> bit & 1) != 0;
        if (raw && mine) raw[bit] = v[bit];
        if (sp.channels >> bit & 1) {
            if (mine) *o = roll_scaled(v[bit], sp.scale[bit]);
            ++o;
        }
    }
}

// nearest_point_on_trajectory's arithmetic for segment k of the track columns [7][.] (ax, ay, dx, dy, l2, len, cum; `cs` apart):
// the clipped parameter and the distance, as k_track_project computes them
F110_HD double track_seg_dist(const double *cols, size_t cs, int k, double px, double py, double &t)
{
    const double ax = cols[k], ay = cols[cs + k], dx = cols[2 * cs + k], dy = cols[3 * cs + k], l2 = cols[4 * cs + k];
    t = ((px - ax) * dx + (py - ay) * dy) / l2;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double rx = px - (ax + t * dx), ry = py - (ay + t * dy);
    return sqrt(rx * rx + ry * ry);
}

// arc length and signed lateral offset (left of the segment's direction is positive) of the winner (best, t, dist)
F110_HD void track_winner(const double *cols, size_t cs, int best, double t, double dist, double px, double py, double &s, double &lat)
{
    const double ax = cols[best], ay = cols[cs + best], dx = cols[2 * cs + best], dy = cols[3 * cs + best];
    s = cols[6 * cs + best] + t * cols[5 * cs + best];
    const double rx = px - (ax + t * dx), ry = py - (ay + t * dy);
    const double cross = dx * ry - dy * rx;
    lat = cross < 0.0 ? -dist : dist;
}

// the projection serially (the kernel gives a pose 16 lanes; this is what the unit harness runs): the first minimum over every
// segment; when no distance is below +inf (a NaN pose) segment 0 with its own t and distance, as np.argmin returns it
F110_HD void roll_project(const double *cols, int nseg, double px, double py, double &s, double &lat)
{
    double dist = INFINITY, tb = 0.0;
    int best = 0x7fffffff;
    for (int k = 0; k < nseg; ++k) {
        double t;
        const double d = track_seg_dist(cols, (size_t)nseg, k, px, py, t);
        if (d < dist) {
            dist = d;
            tb = t;
            best = k;
        }
    }
    if (best == 0x7fffffff) {
        best = 0;
        dist = track_seg_dist(cols, (size_t)nseg, 0, px, py, tb);
    }
    track_winner(cols, (size_t)nseg, best, tb, dist, px, py, s, lat);
}

// s(end) - s(start), wrapped once into (-L/2, L/2] on a closed track
F110_HD double roll_progress(double s_start, double s_end, int closed, double L) { return nbr_gap(s_start, s_end, closed ? L : 0.0); }

// the track pass's two values into a candidate's row
F110_HD void roll_store_track(const RollSpec &sp, double progress, double lat, float *o, double *raw)
{
    double v[ROLL_NCHANNELS] = {};
    v[ROLL_PROGRESS] = progress;
    v[ROLL_END_LAT] = lat;
    roll_store(sp, v, kRollTrackBits, o, raw);
}

// ------------------------------------------------------------------ static obstacles (f110_add_map_obstacles)
enum { OBST_BOX = 0, OBST_DISC = 1 };
constexpr int kMaxObstacles = 256;

// struct f110_obstacle of include/f110.h, field for field
struct Obstacle {
    int32_t shape, reserved;
    double x, y, c, s, half_length, half_width;
};

// the map fields the hit test reads (a slot's resolution and origin)
struct ObstFrame {
    double res, ox, oy, oc, os;
};

// Is the centre of table cell (r, col) inside the shape?  include/f110.h states the rule; float64 in exactly this order, no
// contraction, no trigonometry: the NumPy model (tests/obstacles_ref.py) evaluates the same expressions and agrees bit for bit.
// the centre of table cell (r, col) in map coordinates: the stamp rule's px, py, wx, wy (the corridor rule's too)
F110_HD void cell_centre(const ObstFrame &f, int r, int col, double &wx, double &wy)
{
    const double px = ((double)col + 0.5) * f.res, py = ((double)r + 0.5) * f.res;
    wx = f.ox + (px * f.oc - py * f.os);
    wy = f.oy + (px * f.os + py * f.oc);
}

F110_HD bool obstacle_hit(const Obstacle &o, const ObstFrame &f, int r, int col)
{
    double wx, wy;
    cell_centre(f, r, col, wx, wy);
    const double dx = wx - o.x, dy = wy - o.y;
    if (o.shape == OBST_DISC) return dx * dx + dy * dy <= o.half_length * o.half_length;
    const double u = dx * o.c + dy * o.s, v = -dx * o.s + dy * o.c;
    return fabs(u) <= o.half_length && fabs(v) <= o.half_width;
}

// A conservative cell box [c0, c1] x [r0, r1] around the shape, clamped to the table (empty: c0 > c1 or r0 > r1).  The shape lies
// inside the circle of radius hypot(half_length, half_width) (a disc: half_length) around its centre; two cells of margin cover
// the rounding of this arithmetic against obstacle_hit's ...
F110_HD void obstacle_cell_box(const Obstacle &o, const ObstFrame &f, int H, int W, int &c0, int &c1, int &r0, int &r1)
{
    const double R = o.shape == OBST_DISC ? o.half_length : sqrt(o.half_length * o.half_length + o.half_width * o.half_width);
    const double dx = o.x - f.ox, dy = o.y - f.oy;
    const double inv = 1.0 / f.res;
    const double tx = (dx * f.oc + dy * f.os) * inv - 0.5, ty = (-dx * f.os + dy * f.oc) * inv - 0.5;   // centre in cell-centre units
    // ... and 1e-12 of the coordinates' magnitude covers it where they are huge; beyond 1e150 (squares overflow: inf <= inf is a
    // hit by the rule) the box is the whole table
    const double mag = fabs(o.x) + fabs(o.y) + fabs(f.ox) + fabs(f.oy) + ((double)W + (double)H) * f.res;
    const bool wild = !(R <= 1e150) || !(mag <= 1e150);
    const double m = R * inv * (1.0 + 1e-9) + 2.0 + 1e-12 * mag * inv;
    // clamp in float64 BEFORE the conversion: a far-away centre must not overflow an int
    const double lo_c = floor(tx - m), hi_c = ceil(tx + m), lo_r = floor(ty - m), hi_r = ceil(ty + m);
    c0 = lo_c > 0.0 ? (lo_c < (double)W ? (int)lo_c : W) : 0;
    c1 = hi_c < (double)(W - 1) ? (hi_c >= 0.0 ? (int)hi_c : -1) : W - 1;
    r0 = lo_r > 0.0 ? (lo_r < (double)H ? (int)lo_r : H) : 0;
    r1 = hi_r < (double)(H - 1) ? (hi_r >= 0.0 ? (int)hi_r : -1) : H - 1;
    if (wild) {
        c0 = r0 = 0;
        c1 = W - 1;
        r1 = H - 1;
    }
}

// ------------------------------------------------------------------ corridors (f110_add_map_corridor)
// One text for k_corridor_mask and the host harness (tests/host_harness/corridor_harness.hip).
constexpr int kMaxCorridorPoints = 65536;
constexpr int kCorrTileW = 64, kCorrTileH = 16;   // a workgroup's tile of cells: a wave's lanes are 64 columns of one row
constexpr int kCorrChunk = 256;                   // segments per cooperative step of the cull walk: one per lane of the workgroup
constexpr int kCorrCap = 256;                     // segments the kept list holds (16 KiB of LDS, >= a chunk); a tile that keeps more works in rounds

// a segment as the rule reads it: the ends and what the rule forms from them once (the same expressions, so the same bits)
struct CorridorSeg {
    double ax, ay, bx, by, dx, dy, L2, h2;
};

F110_HD CorridorSeg corridor_seg(double ax, double ay, double bx, double by, double hw)
{
    const double dx = bx - ax, dy = by - ay;
    return CorridorSeg{ax, ay, bx, by, dx, dy, dx * dx + dy * dy, hw * hw};
}

// Is the point (wx, wy) — a cell centre — in the segment's capsule?  include/f110.h states the rule; float64 in exactly this order,
// no contraction, no division, no square root: the NumPy model (tests/trackgen_ref.py) agrees bit for bit.
F110_HD bool corridor_hit(const CorridorSeg &s, double wx, double wy)
{
    const double ux = wx - s.ax, uy = wy - s.ay;
    const double t = ux * s.dx + uy * s.dy;
    if (t <= 0.0) return ux * ux + uy * uy <= s.h2;
    if (t >= s.L2) {
        const double vx = wx - s.bx, vy = wy - s.by;
        return vx * vx + vy * vy <= s.h2;
    }
    const double cr = ux * s.dy - uy * s.dx;
    return cr * cr <= s.h2 * s.L2;
}

// the circle around the centres of the cells [r0, r1] x [c0, c1] of a tile (map coordinates), and the size of its numbers
struct CorridorTile {
    double cx, cy, rad, mag;
};

// The frame's map is affine, so the centres of a tile's cells lie in the parallelogram of its four corner cells' centres, and the
// corner farthest from the parallelogram's centre bounds them all (whatever oc, os are: they need not be a rotation).
F110_HD CorridorTile corridor_tile(const ObstFrame &f, int r0, int c0, int r1, int c1)
{
    double x[4], y[4];
    cell_centre(f, r0, c0, x[0], y[0]);
    cell_centre(f, r0, c1, x[1], y[1]);
    cell_centre(f, r1, c0, x[2], y[2]);
    cell_centre(f, r1, c1, x[3], y[3]);
    CorridorTile t;
    t.cx = 0.25 * x[0] + 0.25 * x[1] + 0.25 * x[2] + 0.25 * x[3];
    t.cy = 0.25 * y[0] + 0.25 * y[1] + 0.25 * y[2] + 0.25 * y[3];
    double far2 = 0.0;
    t.mag = 0.0;
    for (int i = 0; i < 4; ++i) {
        const double ex = x[i] - t.cx, ey = y[i] - t.cy, d2 = ex * ex + ey * ey;
        far2 = d2 > far2 ? d2 : far2;
        const double m = fabs(x[i]) + fabs(y[i]);
        t.mag = m > t.mag ? m : t.mag;   // (a NaN corner: the comparisons drop it; corridor_reaches then sees rad or d2 NaN and keeps)
    }
    t.rad = sqrt(far2);
    return t;
}

// Can the capsule of segment a -> b with half width hw reach a cell centre of the tile?  Conservative: the capsule lies in the
// circle of radius |b - a| / 2 + hw around the segment's middle, and the two circles are compared with a margin of 1e-9 of their
// radii plus 1e-9 of the magnitude of the numbers involved — many orders above the rounding of this arithmetic and of
// corridor_hit's, so rounding can only keep too many.  Numbers whose squares may overflow (beyond 1e150), and anything that
// compares as NaN, keep the segment: corridor_hit decides then.
F110_HD bool corridor_reaches(double ax, double ay, double bx, double by, double hw, const CorridorTile &t)
{
    const double mag = fabs(ax) + fabs(ay) + fabs(bx) + fabs(by) + hw + t.mag + t.rad;
    if (!(mag <= 1e150)) return true;
    const double mx = 0.5 * ax + 0.5 * bx, my = 0.5 * ay + 0.5 * by;
    const double ex = bx - ax, ey = by - ay;
    const double R = (0.5 * sqrt(ex * ex + ey * ey) + hw + t.rad) * (1.0 + 1e-9) + 1e-9 * mag;
    const double qx = t.cx - mx, qy = t.cy - my;
    return !(qx * qx + qy * qy > R * R);
}

// The walk's bookkeeping, shared so that the kernel and the host harness cannot drift apart: a chunk's kept segments take the list
// positions n, n + 1, ... in segment order; the list is swept against the tile's cells when it is full (a round) and the rest of
// the chunk starts the next list.  pos: where a kept segment of this chunk goes, before (first) or after (!first) the round.
F110_HD int corridor_list_slot(int pos, bool first) { return first ? (pos < kCorrCap ? pos : -1) : (pos >= kCorrCap ? pos - kCorrCap : -1); }

// ------------------------------------------------------------------ MPPI planner (include/f110.h, f110_mppi)
// The planner's own arithmetic around roll_candidate: the clamp of a sampled action, the cost of a rolled candidate, the weights and
// the weighted update.  One text for the kernels (k_mppi_*) and the host harness (tests/host_harness/mppi_harness.hip); the draws
// themselves are f110_rng.hpp's (mppi_normal, mppi_sample_row), which builds on this header.
enum { MPPI_MAX_K = 256, MPPI_MAX_H = 64, MPPI_MAX_REPEAT = 16 };

struct MppiSpec {
    int32_t K, H, repeat, shift;
    double margin, sigma_steer, sigma_speed, steer_min, steer_max, speed_min, speed_max, lambda;
    double w_dead, w_clear, w_progress, w_lat, clear_ref, v_init;
};

// the rollout's spec of a planner's candidates: per-agent rows of V, no output channels of its own
F110_HD RollSpec mppi_roll_spec(const MppiSpec &s)
{
    RollSpec r{};
    r.K = s.K;
    r.H = s.H;
    r.repeat = s.repeat;
    r.layout = ROLL_PER_AGENT;
    r.frame = ROLL_FRAME_WORLD;
    r.margin = s.margin;
    for (int b = 0; b < ROLL_NCHANNELS; ++b) r.scale[b] = 1.0;
    return r;
}

F110_HD bool mppi_needs_track(const MppiSpec &s) { return s.w_progress != 0.0 || s.w_lat != 0.0; }

F110_HD double mppi_clamp(double x, double lo, double hi) { return x < lo ? lo : (x > hi ? hi : x); }

// the nominal a candidate is drawn around: the stored one, or (0, v_init) on a fresh row; c = 0 steer, 1 speed
F110_HD double mppi_nominal(const MppiSpec &s, const double *U, bool fresh, int h, int c) { return fresh ? (c ? s.v_init : 0.0) : U[2 * h + c]; }

// one action of candidate k >= 1 from its two draws
F110_HD void mppi_perturb(const MppiSpec &s, double u_steer, double u_speed, double e_s, double e_v, double *v)
{
    v[0] = mppi_clamp(u_steer + s.sigma_steer * e_s, s.steer_min, s.steer_max);
    v[1] = mppi_clamp(u_speed + s.sigma_speed * e_v, s.speed_min, s.speed_max);
}

// the cost of a rolled candidate, accumulated in the header's order.  The kernels take it in two parts where the projection is a
// pass of its own (the rollout's lane leaves the first two terms, the projection's lane adds the track's); the operations and their
// order are the same.  Without a track pass progress = end_lat = 0.0.
F110_HD double mppi_cost_map(const MppiSpec &s, int alive, double min_clear)
{
    double c = s.w_dead * (double)(s.H * s.repeat - alive);
    c = c + s.w_clear * (min_clear < s.clear_ref ? s.clear_ref - min_clear : 0.0);
    return c;
}

F110_HD double mppi_cost_track(const MppiSpec &s, double c, double progress, double end_lat)
{
    c = c - s.w_progress * progress;
    c = c + s.w_lat * fabs(end_lat);
    return c != c ? INFINITY : c;
}

F110_HD double mppi_cost(const MppiSpec &s, int alive, double min_clear, double progress, double end_lat)
{
    return mppi_cost_track(s, mppi_cost_map(s, alive, min_clear), progress, end_lat);
}

// the minimum of the K costs (none is NaN) and its first index
F110_HD void mppi_min(const double *cost, int K, double &beta, int &best)
{
    beta = cost[0];
    best = 0;
    for (int k = 1; k < K; ++k)
        if (cost[k] < beta) {
            beta = cost[k];
            best = k;
        }
}

F110_HD bool mppi_finite(double x) { return x - x == 0.0; }

// candidate k's weight; a beta that is not finite leaves the nominal alone: w = (1, 0, ...)
F110_HD double mppi_weight(const MppiSpec &s, double cost, double beta, int k)
{
    if (!mppi_finite(beta)) return k == 0 ? 1.0 : 0.0;
    return exp(-(cost - beta) / s.lambda);
}

// eta = sum w, q = sum w * w over ascending k from 0.0
F110_HD void mppi_norms(const double *w, int K, double &eta, double &q)
{
    eta = 0.0;
    q = 0.0;
    for (int k = 0; k < K; ++k) {
        eta = eta + w[k];
        q = q + w[k] * w[k];
    }
}

// U'[t] for element t = 2 * h + c of the sequence: V is the agent's [K][H][2], the sum over ascending k from 0.0
F110_HD double mppi_blend(const double *w, const double *V, int K, int H, int t, double eta)
{
    double num = 0.0;
    for (int k = 0; k < K; ++k) num = num + w[k] * V[(size_t)k * 2 * H + t];
    return num / eta;
}

// element t of U' into the stored nominal: in place, or moved one action ahead with the last action kept
F110_HD void mppi_store_nominal(const MppiSpec &s, double *U, int t, double u)
{
    if (!s.shift) {
        U[t] = u;
        return;
    }
    if (t >= 2) U[t - 2] = u;
    if (t >= 2 * s.H - 2) U[t] = u;
}

F110_HD void mppi_info(double beta, double c0, double eta, double q, int best, float *o)
{
    o[0] = (float)beta;
    o[1] = (float)c0;
    o[2] = (float)(eta * eta / q);
    o[3] = (float)best;
}

// ------------------------------------------------------------------ opponents (include/f110.h, f110_opponents)
// The other cars of an agent's env predicted over the horizon, and a candidate's distance to the predictions.  No reference
// counterpart.  Float64 adds, multiplies, divides, compares and one sqrt per sample; one cos_sin per CV opponent.  One text for the
// kernels (k_opp_predict, the OPP lanes of k_rollout_opp / k_mppi_roll_opp) and the host harness (tests/host_harness/opp_harness.hip).
enum { OPP_CV = 0, OPP_TRACK = 1 };
enum { OPP_MAX = 31 };

// struct f110_opponents, then the planner's two weights and reference (0.0 where only the rollout asks)
struct OppSpec {
    int32_t mode, pad_;
    double radius, max_range;
    double w_hit, w_near, near_ref;
};

// the instant of the pose behind action h's last repeat
F110_HD double opp_tau(int h, int repeat, double dt) { return (double)((h + 1) * repeat) * dt; }

// is the opponent at (ox, oy) looked at by the agent that starts at (x, y)?  Written so that a NaN is not.
F110_HD bool opp_in_range(double x, double y, double ox, double oy, double max_range)
{
    const double dx = ox - x, dy = oy - y;
    return dx * dx + dy * dy <= max_range * max_range;
}

// constant velocity along the heading (c, s) = cos_sin(theta_o), taken once per opponent
F110_HD void opp_predict_cv(double ox, double oy, double v, double c, double s, double tau, double *p)
{
    const double d = v * tau;
    p[0] = ox + d * c;
    p[1] = oy + d * s;
}

// along the raceline from the projection (s_o, lat_o), the lateral offset kept: the preview's station at s_o + v * tau
F110_HD void opp_predict_track(const PreviewTrack &tr, double s_o, double lat_o, double v, double tau, double *p)
{
    double s = s_o + v * tau;
    if (tr.closed) {
        if (s >= tr.L) s = s - tr.L;
        else if (s < 0.0) s = s + tr.L;
    }
    const int k = preview_segment(tr.cols + 6 * (size_t)tr.nseg, tr.nseg, s);
    double w[PREVIEW_NCHANNELS];
    preview_station(tr, k, s, PREVIEW_FRAME_WORLD, 0.0, 0.0, 1.0, 0.0, w);
    p[0] = w[0] - lat_o * w[3];
    p[1] = w[1] + lat_o * w[2];
}

// one opponent's whole row p[H][2] serially (the kernel gives an opponent 16 lanes; this is what the unit harness runs).  `cols`
// [7][nseg] (TRACK only).  An opponent out of range: NaN.
F110_HD void opp_predict_row(const OppSpec &sp, const double *cols, int nseg, int closed, double L, double x, double y, const double *o, int H,
                             int repeat, double dt, double *p)
{
    const bool seen = opp_in_range(x, y, o[0], o[1], sp.max_range);
    double a = 0.0, b = 0.0;   // CV: cos, sin; TRACK: s_o, lat_o
    if (seen && sp.mode == OPP_CV) cos_sin(o[3], a, b);
    if (seen && sp.mode == OPP_TRACK) roll_project(cols, nseg, o[0], o[1], a, b);
    const PreviewTrack tr{cols, nullptr, nseg, closed, 0, 0, L};
    for (int h = 0; h < H; ++h) {
        const double tau = opp_tau(h, repeat, dt);
        if (!seen) p[2 * h] = p[2 * h + 1] = NAN;
        else if (sp.mode == OPP_CV) opp_predict_cv(o[0], o[1], o[2], a, b, tau, p + 2 * h);
        else opp_predict_track(tr, a, b, o[2], tau, p + 2 * h);
    }
}

// the candidate's position behind action h against the agent's rows [Ao][H][2]: the running minimum m (from +inf) and the first
// action with a sample inside the radius, `free` (from H: no hit yet).  A NaN distance does neither.  The radius is read from `sp`
// at the sample (on the device: from memory, so that it is not held in a register across the step loop).
F110_HD void opp_sample(const double *rows, int Ao, int H, int h, double x, double y, const OppSpec &sp, double &m, int &free)
{
#pragma unroll 1
    for (int o = 0; o < Ao; ++o) {
        const double *p = rows + ((size_t)o * H + h) * 2;
        const double dx = x - p[0], dy = y - p[1];
        const double d = sqrt(dx * dx + dy * dy);
        if (d < m) m = d;
        if (free == H && d < sp.radius) free = h;
    }
}

// the planner's two opponent terms, between the map's and the track's
F110_HD double mppi_cost_opp(const OppSpec &o, double c, int H, int free, double m)
{
    c = c + o.w_hit * (double)(H - free);
    c = c + o.w_near * (m < o.near_ref ? o.near_ref - m : 0.0);
    return c;
}

// ------------------------------------------------------------------ particle filter (include/f110.h, f110_pf)
// Monte-Carlo localisation's own arithmetic around the scan's ray march: the fresh cloud, systematic resampling, the odometry motion,
// the beam term, the weights and the estimate.  One text for the kernels (k_pf_*) and the host harness
// (tests/host_harness/pf_harness.hip); the draws are f110_rng.hpp's (pf_uniform, pf_normals).  Every sum here runs over ascending
// indices from 0.0, on the device too (one lane walks it): the header's rule bit for bit given the terms.
enum { PF_MAX_P = 1024, PF_MAX_BEAMS = 128 };

struct PfSpec {
    int32_t P, B, beam_first, beam_stride;
    double sigma_x, sigma_y, sigma_theta, init_x, init_y, init_theta, sigma_hit, clip, squash, resample_frac;
};

// what k_pf_plan leaves per armed agent for k_pf_move and k_pf_update
struct PfPlan {
    double u, ctot;        // the resampling draw; C[P - 1]
    double a, b, dth;      // the odometry delta in the last pose's frame
    int32_t resample, fresh;
};

// what k_pf_move leaves per particle for k_pf_sense: the lidar position, the scan's start index, the first sample (shared by the
// particle's beams) and whether every sample stays inside the padded table
struct PfHdr {
    double x, y, start, d0;
    int32_t fast, pad_;
};

// the step's own yaw wrap (advance_vehicle_with)
F110_HD double pf_wrap(double th)
{
    if (th > kTwoPi)
        th = th - kTwoPi;
    else if (th < 0)
        th = th + kTwoPi;
    return th;
}

F110_HD double pf_sum(const double *v, int n)
{
    double s = 0.0;
    for (int q = 0; q < n; ++q) s = s + v[q];
    return s;
}

// 1 / sum W^2
F110_HD double pf_ess(const double *W, int P)
{
    double q = 0.0;
    for (int p = 0; p < P; ++p) q = q + W[p] * W[p];
    return 1.0 / q;
}

F110_HD bool pf_decide(const PfSpec &s, double ess) { return ess < s.resample_frac * (double)s.P; }

// C[j] = sum of W[0 .. j]; C may be W
F110_HD void pf_cumulate(const double *W, int P, double *C)
{
    double c = 0.0;
    for (int p = 0; p < P; ++p) {
        c = c + W[p];
        C[p] = c;
    }
}

// slot i's ancestor: the least j with C[j] > t_i (P - 1 if none); C does not decrease, so a bisection finds it
F110_HD int pf_ancestor(const double *C, int P, int i, double u, double ctot)
{
    const double t = ((double)i + u) / (double)P * ctot;
    int lo = 0, hi = P - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (C[mid] > t)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// the true pose's move since the last call, in the last pose's frame
F110_HD void pf_odometry(const double *last, double x, double y, double th, double &a, double &b, double &dth)
{
    const double dx = x - last[0], dy = y - last[1];
    double c, s;
    cos_sin(last[2], c, s);
    a = c * dx + s * dy;
    b = -s * dx + c * dy;
    dth = th - last[2];
    if (dth > kPi)
        dth = dth - kTwoPi;
    else if (dth <= -kPi)
        dth = dth + kTwoPi;
}

F110_HD void pf_fresh(const PfSpec &s, double x, double y, double th, const double *e, double *X)
{
    X[0] = x + s.init_x * e[0];
    X[1] = y + s.init_y * e[1];
    X[2] = pf_wrap(th + s.init_theta * e[2]);
}

// one particle's motion from its ancestor `src`
F110_HD void pf_move(const PfSpec &s, double a, double b, double dth, const double *src, const double *e, double *X)
{
    const double fa = a + s.sigma_x * e[0], fb = b + s.sigma_y * e[1];
    double c, sn;
    cos_sin(src[2], c, sn);
    X[0] = src[0] + (c * fa - sn * fb);
    X[1] = src[1] + (sn * fa + c * fb);
    X[2] = pf_wrap(src[2] + dth + s.sigma_theta * e[2]);
}

// the lidar pose of a particle: advance_vehicle_with's rule for scan_pose (the heading is wrapped already)
F110_HD void pf_lidar_pose(const double *X, double lidar_dist, double *lp)
{
    const bool on_axle = lidar_dist == 0.0 && fabs(X[2]) < 1e300 && !(X[0] == 0.0 && signbit(X[0])) && !(X[1] == 0.0 && signbit(X[1]));
    if (on_axle) {
        lp[0] = X[0];
        lp[1] = X[1];
    } else {
        double ch, sh;
        cos_sin(X[2], ch, sh);
        lp[0] = X[0] + lidar_dist * ch;
        lp[1] = X[1] + lidar_dist * sh;
    }
    lp[2] = X[2];
}

// one beam's term: the squared error in sigmas, truncated at clip^2; a NaN takes the clip, or counts as 0 without truncation
F110_HD double pf_term(const PfSpec &s, double z, double expect)
{
    const double e = (z - expect) / s.sigma_hit, e2 = e * e, c2 = s.clip * s.clip;
    if (e2 < c2) return e2;
    return (e2 != e2 && !(c2 < INFINITY)) ? 0.0 : c2;
}

F110_HD double pf_logw(const PfSpec &s, const double *t, int B) { return -(0.5 / s.squash) * pf_sum(t, B); }

F110_HD double pf_max(const double *L, int P)
{
    double m = L[0];
    for (int p = 1; p < P; ++p)
        if (L[p] > m) m = L[p];
    return m;
}

F110_HD double pf_unnorm(double W, double L, double Lmax) { return W * exp(L - Lmax); }

F110_HD double pf_norm(double w, double eta, int P) { return eta > 0 ? w / eta : 1.0 / (double)P; }

F110_HD double pf_spread_term(double w, double x, double y, double xh, double yh) { return w * ((x - xh) * (x - xh) + (y - yh) * (y - yh)); }

F110_HD void pf_info(double q, double spread, double xh, double yh, double x, double y, int resampled, float *o)
{
    o[0] = (float)(1.0 / q);
    o[1] = (float)sqrt(spread);
    o[2] = (float)hypot(xh - x, yh - y);
    o[3] = resampled ? 1.0f : 0.0f;
}

// ------------------------------------------------------------------ centreline extraction (f110_map_centerline)
// The per-word decisions of the thinning rule include/f110.h states.  The mask is a bit plane: bit b of word w of a row is the cell
// of column 64 w + b, so one 64-bit word decides 64 cells of a row at once, in bit-sliced boolean logic.  One text for the kernels
// (k_cl_*) and the host program (tests/host_harness/centerline_main.hip).
struct ClNbr {
    uint64_t p2, p3, p4, p5, p6, p7, p8, p9;   // the eight neighbour planes of a word, aligned to its bits
};

// lo / mid / hi: rows r-1 / r / r+1 around word w, each as the words (w-1, w, w+1); a word or a row outside the plane is 0
F110_HD ClNbr cl_neighbours(const uint64_t *lo, const uint64_t *mid, const uint64_t *hi)
{
    ClNbr n;
    n.p2 = lo[1];
    n.p3 = (lo[1] >> 1) | (lo[2] << 63);
    n.p4 = (mid[1] >> 1) | (mid[2] << 63);
    n.p5 = (hi[1] >> 1) | (hi[2] << 63);
    n.p6 = hi[1];
    n.p7 = (hi[1] << 1) | (hi[0] >> 63);
    n.p8 = (mid[1] << 1) | (mid[0] >> 63);
    n.p9 = (lo[1] << 1) | (lo[0] >> 63);
    return n;
}

// A, the 0 -> 1 transitions around P2 .. P9, P2, as two planes: `any` A >= 1, `many` A >= 2
F110_HD void cl_transitions(const ClNbr &n, uint64_t &any, uint64_t &many)
{
    const uint64_t p[9] = {n.p2, n.p3, n.p4, n.p5, n.p6, n.p7, n.p8, n.p9, n.p2};
    any = many = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t t = ~p[i] & p[i + 1];
        many |= any & t;
        any |= t;
    }
}

// 2 <= B <= 6: the eight planes summed by full adders into the four bit planes of B
F110_HD uint64_t cl_count_2_to_6(const ClNbr &n)
{
    const uint64_t s0 = n.p2 ^ n.p3 ^ n.p4, c0 = (n.p2 & n.p3) | (n.p4 & (n.p2 ^ n.p3));
    const uint64_t s1 = n.p5 ^ n.p6 ^ n.p7, c1 = (n.p5 & n.p6) | (n.p7 & (n.p5 ^ n.p6));
    const uint64_t s2 = n.p8 ^ n.p9, c2 = n.p8 & n.p9;
    const uint64_t b0 = s0 ^ s1 ^ s2, c3 = (s0 & s1) | (s2 & (s0 ^ s1));     // ones
    const uint64_t t = c0 ^ c1 ^ c2, c4 = (c0 & c1) | (c2 & (c0 ^ c1));      // twos: c0 + c1 + c2 + c3
    const uint64_t b1 = t ^ c3, c5 = t & c3;
    const uint64_t b2 = c4 ^ c5, b3 = c4 & c5;                               // fours, eights
    return (b1 | b2 | b3) & ~b3 & ~(b2 & b1 & b0);
}

// the cells of `cur` that thinning sub-pass `sub` (0: the first, 1: the second) deletes
F110_HD uint64_t cl_thin_word(int sub, uint64_t cur, const ClNbr &n)
{
    uint64_t any, many;
    cl_transitions(n, any, many);
    const uint64_t keep = sub == 0 ? (n.p2 & n.p4 & n.p6) | (n.p4 & n.p6 & n.p8) : (n.p2 & n.p4 & n.p8) | (n.p2 & n.p6 & n.p8);
    return cur & cl_count_2_to_6(n) & any & ~many & ~keep;
}

// ... that staircase pass k (0 .. 3, in the rule's order) deletes
F110_HD uint64_t cl_stair_word(int k, uint64_t cur, const ClNbr &n)
{
    switch (k) {
    case 0: return cur & n.p2 & n.p4 & ~(n.p6 | n.p7 | n.p8);
    case 1: return cur & n.p4 & n.p6 & ~(n.p8 | n.p9 | n.p2);
    case 2: return cur & n.p6 & n.p8 & ~(n.p2 | n.p3 | n.p4);
    default: return cur & n.p8 & n.p2 & ~(n.p4 | n.p5 | n.p6);
    }
}

// ... that a prune pass deletes: A <= 1
F110_HD uint64_t cl_prune_word(uint64_t cur, const ClNbr &n)
{
    uint64_t any, many;
    cl_transitions(n, any, many);
    return cur & ~many;
}

// One pass over a plane on the CPU or by one lane per word: op 0 / 1 the thinning sub-passes, 2 .. 5 the staircase passes, 6 prune.
// Returns the word's deletions; `out` is the word after the pass.
F110_HD uint64_t cl_pass_word(int op, const uint64_t *plane, int H, int Ww, int r, int w, uint64_t &out)
{
    const uint64_t cur = plane[(size_t)r * Ww + w];
    out = cur;
    if (cur == 0) return 0;
    uint64_t rows[3][3];
    for (int dr = -1; dr <= 1; ++dr) {
        const int rr = r + dr;
        for (int dw = -1; dw <= 1; ++dw) {
            const int ww = w + dw;
            rows[dr + 1][dw + 1] = (rr >= 0 && rr < H && ww >= 0 && ww < Ww) ? plane[(size_t)rr * Ww + ww] : 0;
        }
    }
    const ClNbr n = cl_neighbours(rows[0], rows[1], rows[2]);
    const uint64_t del = op < 2 ? cl_thin_word(op, cur, n) : (op < 6 ? cl_stair_word(op - 2, cur, n) : cl_prune_word(cur, n));
    out = cur & ~del;
    return del;
}

// the seed's table cell: the inverse of the stamp rule's transform, with xy_2_rc's bounds test and true division.  false: outside.
F110_HD bool cl_seed_cell(double x, double y, double res, double ox, double oy, double oc, double os, int H, int W, int &r, int &c)
{
    const double xt = x - ox, yt = y - oy;
    const double xr = xt * oc + yt * os, yr = -xt * os + yt * oc;
    if (!((xr >= 0) & (xr < (double)W * res) & (yr >= 0) & (yr < (double)H * res))) return false;
    c = (int)(xr / res);
    r = (int)(yr / res);
    if (c > W - 1) c = W - 1;
    if (r > H - 1) r = H - 1;
    return true;
}

// ------------------------------------------------------------------ raceline and speed profile (f110_raceline_batch)
// The per-point arithmetic of the rule include/f110.h states: float64 in exactly this order, never contracted.  One text for
// k_raceline and the host program (tests/host_harness/raceline_main.hip); the NumPy restatement (tests/raceline_ref.py) agrees bit
// for bit.
constexpr int kRacelineMaxPoints = 4096;
constexpr int kRacelineMaxLevels = 6, kRacelineMaxIters = 4096;
constexpr int kRacelinePerLane = 4;   // points of a line per lane of its workgroup: point i is lane i % lanes, slot i / lanes

struct RacelineSpec {
    int32_t levels, iters;
    double margin, v_max, a_lat, a_accel, a_brake;
};

// min(max(x, lo), hi) for numbers that are no NaN
F110_HD double rl_clamp(double x, double lo, double hi)
{
    const double m = x > lo ? x : lo;
    return m < hi ? m : hi;
}

F110_HD double rl_min(double a, double b) { return b < a ? b : a; }

// step 1: the normal and the bound of a point from its two neighbours; returns l = |q_{i+1} - q_{i-1}| (0: the line is refused)
F110_HD double rl_frame(double qmx, double qmy, double qpx, double qpy, double w, double margin, double &nx, double &ny, double &b)
{
    const double dx = qpx - qmx, dy = qpy - qmy;
    const double l = sqrt(dx * dx + dy * dy);
    nx = -dy / l;
    ny = dx / l;
    const double d = w - margin;
    b = d > 0.0 ? d : 0.0;
    return l;
}

// step 2, prolong: a point between two points of the coarser level
F110_HD double rl_prolong(double am, double ap, double b) { return rl_clamp(0.5 * (am + ap), -b, b); }

// p = q + y * n, per component
F110_HD void rl_point(double qx, double qy, double y, double nx, double ny, double &px, double &py)
{
    px = qx + y * nx;
    py = qy + y * ny;
}

// step 2, one point's iteration: p[0 .. 4] = p_{j-2s} .. p_{j+2s} (x and y), the point's normal and bound, beta[k]; y and alpha are
// the point's state, read and replaced
F110_HD void rl_update(const double px[5], const double py[5], double nx, double ny, double b, double beta, double &y, double &alpha)
{
    double rx[3], ry[3];
    for (int m = 0; m < 3; ++m) {
        rx[m] = (px[m] - 2.0 * px[m + 1]) + px[m + 2];
        ry[m] = (py[m] - 2.0 * py[m + 1]) + py[m + 2];
    }
    const double gx = (rx[0] - 2.0 * rx[1]) + rx[2], gy = (ry[0] - 2.0 * ry[1]) + ry[2];
    const double gg = 2.0 * (nx * gx + ny * gy);
    const double nw = rl_clamp(y - 0.03125 * gg, -b, b);
    y = nw + beta * (nw - alpha);
    alpha = nw;
}

// step 3: the signed curvature of the circle through a, b, c (centerline.curvature_closed's operation order)
F110_HD double rl_curvature(double ax, double ay, double bx, double by, double cx, double cy)
{
    const double abx = bx - ax, aby = by - ay, bcx = cx - bx, bcy = cy - by, acx = cx - ax, acy = cy - ay;
    const double cross = abx * bcy - aby * bcx;
    const double den = sqrt(abx * abx + aby * aby) * sqrt(bcx * bcx + bcy * bcy) * sqrt(acx * acx + acy * acy);
    return 2.0 * cross / den;
}

F110_HD double rl_length(double ax, double ay, double bx, double by)
{
    const double dx = bx - ax, dy = by - ay;
    return sqrt(dx * dx + dy * dy);
}

// the refusal after the solve: a raceline segment of zero length, or a curvature that is no finite number (p_{i+1} = p_{i-1}, or
// lengths whose product underflows: 0 / 0 or x / 0).  With these out of the way no NaN reaches a minimum below, so which operand
// a minimum returns for a NaN is never asked.
F110_HD bool rl_degenerate(double len, double kappa) { return !(len > 0.0) || !(fabs(kappa) <= 1.7976931348623157e308); }

// step 4: the ceiling of v^2 (a zero curvature: a_lat / 0 = inf, then v_max^2)
F110_HD double rl_ceiling(double kappa, double v_max, double a_lat) { return rl_min(v_max * v_max, a_lat / fabs(kappa)); }

// step 4: vx from the ceiling, the arc length and the four minima: pre_f = min_{j<=i} F, suf_f = min_{j>i} F, suf_g = min_{j>=i} G,
// pre_g = min_{j<i} G (an empty one +inf)
F110_HD double rl_F(double c, double cum, double a_accel) { return c - (2.0 * a_accel) * cum; }
F110_HD double rl_G(double c, double cum, double a_brake) { return c + (2.0 * a_brake) * cum; }
F110_HD double rl_speed(double c, double cum, double L, double a_accel, double a_brake, double pre_f, double suf_f, double suf_g, double pre_g)
{
    const double ka = 2.0 * a_accel, kb = 2.0 * a_brake;
    const double A = ka * cum, B = kb * cum;
    const double up = rl_min(A + pre_f, (A + ka * L) + suf_f);
    const double um = rl_min(suf_g - B, (pre_g + kb * L) - B);
    return sqrt(rl_min(c, rl_min(up, um)));
}

// a term of the lap time
F110_HD double rl_lap_term(double len, double vx, double vx_next) { return (2.0 * len) / (vx + vx_next); }

}  // namespace f110
