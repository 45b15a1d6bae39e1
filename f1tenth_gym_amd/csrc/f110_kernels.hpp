// f110_kernels.hpp — the gfx950 kernels of the batched F1TENTH env.step() hot path.
//
// Included by f110_hip.hip (which owns the handle, the launches and the C ABI).  One step is
//   k_integrate   1 lane / agent   pid + steering delay + RK4|Euler + yaw wrap + lidar pose
//                                  (base_classes.py:256-409) + the per-agent ray header
//   k_collide     1 lane / agent   get_vertices + GJK inside each env (collision_models.py:113-260,
//                                  base_classes.py:536-550) + opponent beam windows; side stream
//   k_scan_rays   1 lane / ray, a wave holds 64 consecutive beams: sphere-trace the distance table
//                                  (laser_models.py:106-186), noise row (:450-452), iTTC predicate
//                                  (:188-217), one coalesced store.  Lean on purpose: 8 waves/SIMD.
//   (k_expand_beams: second pass when beams outnumber table directions)
//   k_finalize    1 wave / agent   wall-hit side effects (base_classes.py:246-249), collision OR
//                                  (:588-589), opponent ray-cast on the culled window (:206-227)
//   (k_finalize_pair: two-agent envs — k_collide's work done at the top of k_finalize, no side stream)
//   (k_noise_cache / k_noise_rows: the scan noise, NumPy's PCG64 + ziggurat stream, f110_rng.hpp)
// plus reset / episode-logic kernels, the unit kernels behind the parity entry points, and the
// map pipeline (flip + threshold + exact EDT + dt = res*sqrt(d2)).
// Compiled with -ffp-contract=off: float64, reference operation order, no FMA contraction.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "f110_math.hpp"
#include "f110_rng.hpp"

using namespace f110;

// What one ray needs to know about its agent, written by k_integrate: read through the scalar
// cache by k_scan_rays (a wave's 64 consecutive rays belong to at most two agents).
struct RayHdr {
    double x, y;        // lidar position (base_classes.py:407-408)
    double start;       // wrapped theta_index of beam 0 (laser_models.py:166-172)
    double vel;         // post-integration longitudinal velocity (iTTC)
    double d0;          // first table sample, shared by every beam of the scan (:129)
    int32_t noise_row;  // row of the noise table / row cache for this step; -1 = no noise; -2 = this step's
                        // noise row was generated into the agent's own scans[] row (k_noise_rows)
    int32_t map_slot;   // which registered map this agent's env runs on (0 unless f110_set_env_maps)
    int32_t pad_hdr;
    int32_t i0;         // table index of beam 0
    int32_t n_dirs;     // distinct table indices the scan's beams use (dedupe mode), else 0
    int32_t fast;       // PADDED: every sample of every ray of this scan lands inside the padded table
};
static_assert(sizeof(RayHdr) == 64, "RayHdr is read as 16-byte scalar loads");

struct AgentArrays {
    int32_t n_agents_total;  // N
    int32_t agents_per_env;  // A
    int32_t agent_begin, agent_count;  // the agents this launch covers (an env-aligned group; all: 0, N)
    double *state;           // [7][N]
    double *steer_buf;       // [2][N]
    int32_t *buf_cnt;        // [N]
    double *scan_pose;       // [3][N]  lidar pose after integration
    double *snap_pose;       // [3][N]  Simulator.agent_poses (:574)
    double *dir_start;       // [N]     wrapped theta_index of beam 0
    RayHdr *ray_hdr;         // [N]     per-agent constants of this step's scan
    double *scans;           // [N][B]
    double *collisions;      // [N]
    double *collision_idx;   // [N]
    int32_t *in_collision;   // [N]
    int32_t *step_count;     // [N]
    unsigned long long *path_stats;  // diagnostics or nullptr: rays of fast scans [0] / of exact scans [2]
    // a different track per env (f110_set_env_maps), else both nullptr
    const ScanConst *maps_full;      // [n_maps] every field of every registered map (exact paths)
    const int32_t *env_map;          // [num_envs] slot of each env
    // armed by f110_set_auto_reseat: k_finalize ends with the in-place re-seat of finished envs
    const double *reseat_poses;      // [N][3] or nullptr
    int32_t *reseat_count;           // device counter or nullptr
    int32_t reseat_ego, pad_reseat;
    uint32_t *sched_count_zero;  // longest-first scan order: this step's list counter, zeroed here (or nullptr)
    int32_t *opp_window;     // [N][A][4] beam range each opponent can occupy: {lo, hi} for the live
                             //           heading and {lo0, hi0} for heading 0 (after a wall hit)
    double *opp_verts;       // [N][A][8] the opponent's box drawn with the ego's length/width
    const double *params;    // [A][18] per agent slot, or [N][18] per agent (params_per_agent)
    int32_t params_per_agent, pad_params;
    const double *noise;     // [noise_rows][B] or nullptr: the uploaded table, or the device-generated row cache
    // device RNG (f110_set_noise_rng): 0 off / table, 1 one stream shared by every agent (the reference),
    // 2 a stream per agent.  Rows below noise_rows come from the cache in shared mode; later rows and
    // per-agent streams are generated into scans[] by k_noise_rows from the agent's carried state.
    int32_t noise_rng, pad_rng;
    U128 *rng_state;              // [N] state after the agent's last generated row
    const U128 *rng_seed;         // per-agent mode: [N][2] = {state at reset, inc}
    const U128 *rng_rowstate;     // shared mode: [noise_rows + 1] state at the start of every cached row
    U128 rng_inc;                 // shared mode: the stream's increment
    const double *scan_angles, *beam_cos, *side_dist;  // [B]
    int32_t noise_rows, integrator;
    double time_step, lidar_dist, ttc_thresh, angle_inc;
    double box_length, box_width;  // Simulator.params used by check_collision (:549)
    const struct FusedHost *fused_host;   // f110_step_host, A = 2: the finalize kernel ends with the episode logic + host block (or nullptr)
    unsigned long long fused_seq;         // ... and signals this sequence number (F110_STEP_SPIN_WAIT), 0 = no signal
};

__device__ __forceinline__ VehicleParams load_params(const double *p)
{
    VehicleParams vp;
#pragma unroll
    for (int i = 0; i < NPARAMS; ++i) vp.v[i] = p[i];
    return vp;
}

// ---- episode logic + host block (f110_episode_*, f110_step_host): the structs live here because the A = 2 finalize
// kernel can carry both as its epilogue (FusedHost) ------------------------------------------------------------------
// F110Env._check_done (f110_env.py:204-246): start/finish-zone toggles, lap counts and times, done
// = ego collided or every agent has 4 toggles.
struct EpisodeArrays {
    int32_t ego_idx, pad;
    double timestep;
    double *start_poses;   // [N][3]
    double *rot;           // [E][4] start_rot row-major (f110_env.py:331), computed by the host
    double *current_time;  // [E]
    uint8_t *near_start;   // [N]
    double *toggle;        // [N]
    double *lap_count;     // [N]
    double *lap_time;      // [N]
    uint8_t *done;         // [E]
    uint8_t *checkpoint;   // [N] toggle >= 4
};

// f110_step_host: what a host-driven loop reads after a step (see k_host_block).  Any pointer may be nullptr.
struct HostBlock {
    double *state;          // [7][N]
    double *collisions;     // [N]
    double *collision_idx;  // [N]
    double *agent_poses;    // [3][N]
    double *lap_time, *lap_count, *toggle;  // [N]
    double *current_time;   // [E]
    int32_t *in_collision;  // [N]
    uint8_t *near_start, *checkpoint;  // [N]
    uint8_t *done;          // [E]
    // completion word (F110_STEP_SPIN_WAIT): the workgroup that finishes last stores `seq` here, after every
    // workgroup's stores have been fenced at system scope — the host polls it instead of entering the runtime
    unsigned long long *seq_host;   // page-locked
    unsigned int *blocks_done;      // device counter, returns to 0
    unsigned long long seq;
    // small batches: the scans too are stored by the kernel (a DMA copy of 17 KB costs ~36 us of latency on this
    // runtime, a kernel's stores ~2); nullptr: the caller copies them (big batches: one DMA copy at link rate)
    double *scans;                  // [N][num_beams] page-locked, or nullptr
    int32_t num_beams, pad_beams;
    // f110_track_host_block: the step's track columns (device [4][N] s, ds, lateral, heading_error + [N] segment, written by
    // k_track_project before this kernel runs) into page-locked memory; trk_src nullptr = none
    const double *trk_src;
    const int32_t *trk_seg_src;
    double *trk_s, *trk_ds, *trk_lat, *trk_head;
    int32_t *trk_seg;
};

// rows [first, first + count) of the device scans into the host block, by every thread of the workgroup
__device__ __forceinline__ void host_block_copy_scans(const HostBlock &hb, const double *__restrict__ scans, size_t first, size_t count)
{
    const size_t B = (size_t)hb.num_beams, n = count * B;
    const double *__restrict__ src = scans + first * B;
    double *__restrict__ dst = hb.scans + first * B;
    // four independent loads in flight per lane, then the four stores (a dependent load -> store per iteration would
    // walk the rows one memory round trip at a time)
    size_t q = threadIdx.x;
    for (; q + 3 * (size_t)blockDim.x < n; q += 4 * (size_t)blockDim.x) {
        const double v0 = src[q], v1 = src[q + blockDim.x], v2 = src[q + 2 * (size_t)blockDim.x], v3 = src[q + 3 * (size_t)blockDim.x];
        dst[q] = v0;
        dst[q + blockDim.x] = v1;
        dst[q + 2 * (size_t)blockDim.x] = v2;
        dst[q + 3 * (size_t)blockDim.x] = v3;
    }
    for (; q < n; q += blockDim.x) dst[q] = src[q];
}

// last statement of a workgroup of k_host_block: publish the block's host stores, count, and let the last one signal
__device__ __forceinline__ void host_block_signal(const HostBlock &hb)
{
    if (!hb.seq_host) return;
    __builtin_amdgcn_s_waitcnt(0); // every wave's stores into the host block have been acknowledged (a workgroup barrier alone does not wait for them) ...
    __syncthreads();               // ... in every wave of the workgroup
    if (threadIdx.x == 0) {
        __threadfence_system();    // ... and visible system-wide before the count
        const unsigned int prev = __hip_atomic_fetch_add(hb.blocks_done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == gridDim.x - 1) {
            __hip_atomic_store(hb.blocks_done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(hb.seq_host, hb.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}


// f110_step_host with the pair kernel: episode logic + host block as k_finalize_pair_roles' epilogue (one launch and one
// drain less per step than k_host_block behind it).  Lives in device memory (the handle rewrites it when the caller's
// block changes); the completion word's sequence number travels by value in AgentArrays (it changes every step).
struct FusedHost {
    EpisodeArrays ep;
    HostBlock hb;
    int32_t episode, auto_reset;
};

// ---- K1b body: pairwise body collisions inside each env + opponent beam windows ---------------
// collision_multiple visits pairs (i<j) ascending and overwrites collision_idx, so an agent's
// final index is the largest colliding partner; flags are symmetric.  Each lane evaluates the
// GJK of its pairs in the reference's (lower, higher) argument order.
// AF = 0: any number of agents per env, partner poses through pose_of(j) from memory;
// AF = 2 / 4: exactly that many, loop unrolled so pose_of(j) can index registers.
template <int AF, typename PoseOf>
__device__ __forceinline__ void collide_agent(const AgentArrays &a, int32_t B, int i, double mx, double my, double mth, PoseOf pose_of)
{
    const int A = AF ? AF : a.agents_per_env;
    const int env = i / A, me = i - env * A;
    double mine[8];
    box_vertices(mx, my, mth, a.box_length, a.box_width, mine);
    // bodies whose centres are further apart than a box diagonal (+1 mm) cannot overlap
    const double reach = sqrt(a.box_length * a.box_length + a.box_width * a.box_width) + 1e-3;
    // RaceCar.ray_cast_agents draws the opponents with the EGO's length/width (:223)
    const size_t prow = (size_t)(a.params_per_agent ? i : me) * NPARAMS;
    const double blen = a.params[prow + P_LENGTH];
    const double bwid = a.params[prow + P_WIDTH];
    const double disc_r = 0.5 * sqrt(blen * blen + bwid * bwid);
    bool hit = false;
    int partner = -1;
#pragma unroll
    for (int j = 0; j < A; ++j) {
        if (j == me) continue;
        double ox, oy, oth;
        pose_of(j, ox, oy, oth);
        const double dx = ox - mx, dy = oy - my;
        double other[8];
        if (dx * dx + dy * dy <= reach * reach) {
            box_vertices(ox, oy, oth, a.box_length, a.box_width, other);
            const bool c = (me < j) ? gjk_overlap(mine, other) : gjk_overlap(other, mine);
            if (c) {
                hit = true;
                partner = j;  // j ascending -> ends at the largest colliding index
            }
        }
        // beam window this opponent can occupy in my scan: once for my post-integration heading
        // (no wall hit) and once for heading 0 (RaceCar.check_ttc zeroes it on a wall hit, and the
        // ray-cast reads the live state, base_classes.py:225,246-249); k_finalize picks one.
        int ref_lo, ref_hi, lo, hi;
        box_vertices(ox, oy, oth, blen, bwid, other);
        int32_t *win = a.opp_window + ((size_t)i * A + j) * 4;
        opponent_beam_window(mx, my, mth, other, ox, oy, disc_r, a.scan_angles, B, a.angle_inc, ref_lo, ref_hi, lo, hi);
        win[0] = lo;
        win[1] = hi;
        opponent_beam_window(mx, my, 0.0, other, ox, oy, disc_r, a.scan_angles, B, a.angle_inc, ref_lo, ref_hi, lo, hi);
        win[2] = lo;
        win[3] = hi;
        double *ov = a.opp_verts + ((size_t)i * A + j) * 8;
#pragma unroll
        for (int c = 0; c < 8; ++c) ov[c] = other[c];
    }
    a.collisions[i] = hit ? 1.0 : 0.0;
    a.collision_idx[i] = (double)partner;
}

// what k_integrate leaves behind for one agent: state, delay buffer, lidar pose, pose snapshot, the ray header
// everything the ray kernel needs per agent, incl. the first table sample that all beams share (trace_ray :129 evaluated at the
// lidar position; generic exact path)
__device__ __forceinline__ RayHdr make_ray_hdr(const AgentArrays &a, const ScanConst &k, int i, const double *st, const double *sp, double start)
{
    RayHdr hd;
    ScanConst kr = k;
    kr.table = k.table_rm;
    hd.x = sp[0];
    hd.y = sp[1];
    hd.start = start;
    hd.vel = st[3];
    // a different track per env (f110_set_env_maps): this agent's map constants come from the
    // registered slot instead of the kernel argument
    hd.map_slot = a.env_map ? a.env_map[i / a.agents_per_env] : 0;
    hd.pad_hdr = 0;
    const ScanConst *km = a.env_map ? a.maps_full + hd.map_slot : &kr;
    int r0, c0;
    hd.d0 = sample_distance<LAYOUT_ROWMAJOR, false, false>(*km, nullptr, sp[0], sp[1], r0, c0);
    int row = -1;
    if (a.noise_rng) {
        // k-th scan after reset adds the k-th B-sample draw of the stream (base_classes.py:204,
        // laser_models.py:450-452): from the row cache, or generated by k_noise_rows (-2)
        row = a.step_count[i];
        if (a.noise_rng == 2 || row >= a.noise_rows) row = -2;
    } else if (a.noise_rows > 0) {
        row = a.step_count[i];
        if (row >= a.noise_rows) row %= a.noise_rows;
    }
    hd.noise_row = row;
    hd.i0 = beam_dir_index(k, start, 0);
    hd.fast = 0;
    if (km->pad) {
        double ux, uy;
        padded_position<false>(*km, sp[0], sp[1], ux, uy);
        hd.fast = padded_start_ok(*km, ux, uy) ? 1 : 0;
    }
    hd.n_dirs = 0;
    if (k.theta_inc < 1.0) {  // consecutive beams advance the table index by 0 or 1 (mod theta_dis)
        int span = beam_dir_index(k, start, k.num_beams - 1) - hd.i0;
        if (span < 0) span += k.theta_dis;
        hd.n_dirs = span + 1;
    }
    return hd;
}

// what the integration leaves in HBM for one agent (every column but the ray header)
__device__ __forceinline__ void integrate_store_columns(const AgentArrays &a, int i, int N, const double *st, double b0, double b1, int cnt, const double *sp,
                                                        double start)
{
#pragma unroll
    for (int c = 0; c < 7; ++c) a.state[(size_t)c * N + i] = st[c];
    a.steer_buf[i] = b0;
    a.steer_buf[(size_t)N + i] = b1;
    a.buf_cnt[i] = cnt;
    a.scan_pose[i] = sp[0];
    a.scan_pose[(size_t)N + i] = sp[1];
    a.scan_pose[2 * (size_t)N + i] = sp[2];
    a.snap_pose[i] = st[0];
    a.snap_pose[(size_t)N + i] = st[1];
    a.snap_pose[2 * (size_t)N + i] = st[4];
    a.dir_start[i] = start;
}

__device__ __forceinline__ void integrate_store(const AgentArrays &a, const ScanConst &k, int i, int N, const double *st, double b0, double b1,
                                                int cnt, const double *sp)
{
    const double start = scan_start_index(k, sp[2]);
    integrate_store_columns(a, i, N, st, b0, b1, cnt, sp, start);
    const RayHdr hd = make_ray_hdr(a, k, i, st, sp, start);
    if (a.path_stats) atomicAdd(&a.path_stats[hd.fast ? 0 : 2], (unsigned long long)k.num_beams);
    a.ray_hdr[i] = hd;
    a.in_collision[i] = 0;  // raised by k_scan_rays when any beam's iTTC is under the threshold
    if (a.sched_count_zero && i == a.agent_begin) {
        a.sched_count_zero[0] = 0u;   // this step's task list (TaskSched::count_w)
    }
}

// ---- K1: integrate every agent one time step ------------------------------------------
// AF = 0: integration only (k_collide follows on a side stream, hidden under the scan).
// AF = 2 / 4 (agents per env): the pair tests run in the same lane right after the integration,
// the partners' post-integration poses (the :574 snapshot) arriving by lane shuffle — the agents
// of an env are neighbouring lanes of one wave.  Used when the step runs as several env groups on
// their own streams: one launch and no event fork/join per group, and the longer dependent chain
// hides under the other groups' scans.
template <int AF>
__global__ void __launch_bounds__(AF ? 64 : 256) k_integrate(AgentArrays a, ScanConst k, const double *__restrict__ actions)
{
    const int i = a.agent_begin + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = a.n_agents_total;
    if (i >= a.agent_begin + a.agent_count) return;
    const VehicleParams vp = load_params(a.params + (size_t)(a.params_per_agent ? i : i % a.agents_per_env) * NPARAMS);
    double st[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) st[c] = a.state[(size_t)c * N + i];
    double b0 = a.steer_buf[i], b1 = a.steer_buf[(size_t)N + i];
    int cnt = a.buf_cnt[i];
    const double2 act = reinterpret_cast<const double2 *>(actions)[i];
    double sp[3];
    advance_vehicle(st, b0, b1, cnt, act.x, act.y, vp, a.time_step, a.integrator, a.lidar_dist, sp);
    integrate_store(a, k, i, N, st, b0, b1, cnt, sp);
    if constexpr (AF != 0) {
        // groups are env-aligned and AF divides 64: the AF lanes of an env are all here, in one wave.
        // Every lane takes part in every shuffle (a lane masked off would read as zero).
        const int lane = (int)(threadIdx.x & 63u), me = i % AF;
        double px[AF], py[AF], pth[AF];
#pragma unroll
        for (int jj = 0; jj < AF; ++jj) {
            px[jj] = __shfl(st[0], lane - me + jj);
            py[jj] = __shfl(st[1], lane - me + jj);
            pth[jj] = __shfl(st[4], lane - me + jj);
        }
        collide_agent<AF>(a, k.num_beams, i, st[0], st[1], st[4], [&](int jj, double &ox, double &oy, double &oth) {
            ox = px[jj];
            oy = py[jj];
            oth = pth[jj];
        });
    }
}

// ---- K1 in two waves (round 3; what the product launches when the pair tests are not fused in) ---------------
// k_integrate is one dependent float64 chain per wave (one wave per SIMD at every batch size: its time is its
// instruction count, ~12 cycles each).  The low-speed branch of the right-hand side — tan and cos of the steering
// angle, a quarter of a stage's instructions in a wave that has lanes on both sides of |v| = 0.5, which is nearly
// every wave of a batch that re-seats crashed cars — depends on (steer, v) only, and THEIR derivatives depend on
// nothing else (low_speed_trig_ahead).  So a second wave of the workgroup walks (steer, v) through the stages on its
// own, one stage ahead of the integration, and leaves tan / cos in LDS; the first wave picks them up behind one
// workgroup barrier per stage.  Same operations on the same values: bit-identical to k_integrate<0>.
struct LowTrigShared {
    double (*tn)[64];
    double (*cd)[64];
    int lane;
    __device__ __forceinline__ void begin_stage(int) const { __syncthreads(); }
    __device__ __forceinline__ void operator()(int stage, double, double &t, double &c) const
    {
        t = tn[stage][lane];
        c = cd[stage][lane];
    }
};
struct LowTrigEmit {
    double (*tn)[64];
    double (*cd)[64];
    int lane;
    __device__ __forceinline__ void operator()(int stage, double t, double c) const
    {
        tn[stage][lane] = t;
        cd[stage][lane] = c;
    }
    __device__ __forceinline__ void end_stage(int) const { __syncthreads(); }
};

__global__ void __launch_bounds__(128) k_integrate_duo(AgentArrays a, ScanConst k, const double *__restrict__ actions)
{
    __shared__ double s_tn[4][64], s_cd[4][64];
    const int lane = (int)(threadIdx.x & 63u);
    const bool ahead = threadIdx.x >= 64u;   // wave 1: the low-speed branch's trigonometry; wave 0: everything else
    const int N = a.n_agents_total;
    const int i_raw = a.agent_begin + (int)(blockIdx.x * 64u) + lane;
    const bool live = i_raw < a.agent_begin + a.agent_count;
    const int i = live ? i_raw : a.agent_begin;   // (lanes past the end shadow the first agent: every lane meets every barrier)
    const VehicleParams vp = load_params(a.params + (size_t)(a.params_per_agent ? i : i % a.agents_per_env) * NPARAMS);
    const double2 act = reinterpret_cast<const double2 *>(actions)[i];
    if (ahead) {
        low_speed_trig_ahead(a.state[(size_t)2 * N + i], a.state[(size_t)3 * N + i], a.steer_buf[(size_t)N + i], a.buf_cnt[i], act.y, vp,
                             a.time_step, a.integrator, LowTrigEmit{s_tn, s_cd, lane});
        return;
    }
    double st[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) st[c] = a.state[(size_t)c * N + i];
    double b0 = a.steer_buf[i], b1 = a.steer_buf[(size_t)N + i];
    int cnt = a.buf_cnt[i];
    double sp[3];
    advance_vehicle_with(st, b0, b1, cnt, act.x, act.y, vp, a.time_step, a.integrator, a.lidar_dist, sp, LowTrigShared{s_tn, s_cd, lane});
    if (!live) return;
    integrate_store(a, k, i, N, st, b0, b1, cnt, sp);
}

// ---- K1 fanned out over thirteen waves (round 4; RK4) -------------------------------------------------------------
// k_integrate_duo still runs one ~1900-instruction chain per wave; at 4096 agents that chain IS the kernel's 9.4 us
// (one wave per SIMD: ~10 cycles per dependent instruction).  The step's dataflow is much shallower (f110_math.hpp,
// "the RK4 step taken apart"): a workgroup of 13 waves serves 64 agents —
//   wave 0        the main chain: loads, delay buffer, fan_main (a handful of multiply-adds per stage), combine, store;
//   waves 1-4     stage s's low-speed branch (tan / cos of the steering angle -> f4, f5), lanes that take it;
//   waves 5-8     stage s's single-track coefficients (the three divisions by the velocity), lanes that take it;
//   waves 9-12    stage s's position derivatives (cos / sin of the heading) once the main chain has the headings —
// three workgroup barriers in all.  Same operations on the same operands as k_integrate<0>: bit-identical
// (tests/test_host_math.py test_fan_integration_*, test_integrate_fan_is_invisible).
constexpr int kFanWaves = 13;
constexpr int kFanMaxAgents = 24576;   // measured (profiles/r04_fan_sweep.txt): pays up to 16 384 agents (-1 us per step), loses from 32 768
__global__ void __launch_bounds__(64 * kFanWaves) k_integrate_fan(AgentArrays a, ScanConst k, const double *__restrict__ actions)
{
    __shared__ double s_l4[4][64], s_l5[4][64], s_k[4][6][64], s_ang[4][64], s_vel[4][64], s_f0[4][64], s_f1[4][64];
    const int lane = (int)(threadIdx.x & 63u);
    const int role = (int)(threadIdx.x >> 6);
    const int N = a.n_agents_total;
    const int i_raw = a.agent_begin + (int)(blockIdx.x * 64u) + lane;
    const bool live = i_raw < a.agent_begin + a.agent_count;
    const int i = live ? i_raw : a.agent_begin;   // (lanes past the end shadow the first agent: every lane meets every barrier)
    const VehicleParams vp = load_params(a.params + (size_t)(a.params_per_agent ? i : i % a.agents_per_env) * NPARAMS);
    const double2 act = reinterpret_cast<const double2 *>(actions)[i];
    const double steer0 = a.state[(size_t)2 * N + i], vel0 = a.state[(size_t)3 * N + i];
    const double buf1_in = a.steer_buf[(size_t)N + i];
    const int cnt_in = a.buf_cnt[i];
    double accl, sv;
    fan_inputs(steer0, vel0, buf1_in, cnt_in, act.y, vp, accl, sv);
    double st[7];
    double b0 = 0., b1 = 0.;
    int cnt = 0;
    if (role == 0) {
#pragma unroll
        for (int c = 0; c < 7; ++c) st[c] = a.state[(size_t)c * N + i];
        b0 = a.steer_buf[i];
        b1 = buf1_in;
        cnt = cnt_in;
        if (cnt < 2) cnt += 1;   // :271-278 two-step steering delay
        b1 = b0;
        b0 = act.x;
    } else if (role <= 4) {
        const int s = role - 1;
        const FanWalk w = fan_walk(steer0, vel0, accl, sv, vp, a.time_step, s);
        if (w.low) {
            double f4, f5;
            fan_low(w, vp, f4, f5);
            s_l4[s][lane] = f4;
            s_l5[s][lane] = f5;
        }
    } else if (role <= 8) {
        const int s = role - 5;
        const FanWalk w = fan_walk(steer0, vel0, accl, sv, vp, a.time_step, s);
        if (!w.low) {
            double kk[6];
            fan_dyn(w, vp, kk);
#pragma unroll
            for (int c = 0; c < 6; ++c) s_k[s][c][lane] = kk[c];
        }
    }
    __syncthreads();
    const double x0 = st[0], y0 = st[1];
    if (role == 0) {
        fan_main(st, accl, sv, vp, a.time_step,
                 [&](int s, double &f4, double &f5) {
                     f4 = s_l4[s][lane];
                     f5 = s_l5[s][lane];
                 },
                 [&](int s, double *kk) {
#pragma unroll
                     for (int c = 0; c < 6; ++c) kk[c] = s_k[s][c][lane];
                 },
                 [&](int s, double ang, double v) {
                     s_ang[s][lane] = ang;
                     s_vel[s][lane] = v;
                 });
    }
    __syncthreads();
    if (role >= 9) {
        const int s = role - 9;
        double f0, f1;
        fan_pos(s_ang[s][lane], s_vel[s][lane], f0, f1);
        s_f0[s][lane] = f0;
        s_f1[s][lane] = f1;
    }
    __syncthreads();
    if (role != 0) return;
    st[0] = fan_combine(x0, a.time_step, s_f0[0][lane], s_f0[1][lane], s_f0[2][lane], s_f0[3][lane]);
    st[1] = fan_combine(y0, a.time_step, s_f1[0][lane], s_f1[1][lane], s_f1[2][lane], s_f1[3][lane]);
    double sp[3];
    fan_finish(st, a.lidar_dist, sp);
    if (!live) return;
    integrate_store(a, k, i, N, st, b0, b1, cnt, sp);
}

// ---- K1b: pairwise body collisions inside each env (separate launch, side stream) ------------
__global__ void __launch_bounds__(256) k_collide(AgentArrays a, int32_t B)
{
    const int i = a.agent_begin + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = a.n_agents_total, A = a.agents_per_env;
    if (i >= a.agent_begin + a.agent_count) return;
    const int env = i / A;
    collide_agent<0>(a, B, i, a.snap_pose[i], a.snap_pose[(size_t)N + i], a.snap_pose[2 * (size_t)N + i],
                     [&](int jj, double &ox, double &oy, double &oth) {
                         const int o = env * A + jj;
                         ox = a.snap_pose[o];
                         oy = a.snap_pose[(size_t)N + o];
                         oth = a.snap_pose[2 * (size_t)N + o];
                     });
}

// ---- K2: ray march -------------------------------------------------------------------------
// Rays are numbered ray = pose*B + beam, one lane per ray, so the 64 lanes of a wave are
// consecutive beams of (almost always) one pose: neighbouring beams touch neighbouring cells and
// have correlated lengths.  STEP=true is the env.step() form (SoA poses written by
// k_integrate, noise row, iTTC predicate); STEP=false is ScanSimulator2D.scan for the unit
// entry point (also reports terminating cells and lookup counts).
// Longest-first dispatch of the step's scan tasks, for SMALL batches.  With few agents the scan kernel
// ends when its longest ray ends, and a 64-ray task whose longest ray takes 300 samples may
// only be STARTED in the last of the launch's eight-odd rounds of waves.  Ray lengths barely change from
// one step to the next and workgroups start in block order: a task whose longest ray exceeded `thr`
// lookups in the PREVIOUS step is put on a list, and the list is served by the first blocks of this step's
// launch.  flags_r[task] == epoch_r marks "on the list" (the normal blocks skip those tasks); this step's
// long tasks go to list_w / flags_w for the next step (stamped epoch_w; stale stamps never match again, so
// nothing is ever cleared).  Stale or missing entries only cost speed: every task is marched exactly once.

struct TaskSched {
    const uint32_t *flags_r;
    uint32_t *flags_w;
    const uint32_t *list_r;
    uint32_t *list_w;
    const uint32_t *count_r;
    uint32_t *count_w;   // zeroed by k_integrate of the same step
    uint32_t cap, thr;
    // Reserved words here and in RayJob keep the kernel-argument layout the scan kernels were tuned on: the retired ray pass /
    // two-pass / LDS-window fields used to sit there, and taking them out moved the hot fields across the boundaries of the
    // compiler's wide scalar loads — 4096 agents 46.3 -> 44.6 M agent-steps/s, back to 46.7 with the padding (round 5, A/B of
    // three builds in one session).  Asking for all arguments in ONE batch of scalar loads at the top of the kernel (nine
    // dependent round trips -> two) is no cure either: 46.7 -> 44.7 M at 4096 agents, no change at 2048 / 8192 / 16 384.
    const void *reserved_r[8];
    uint32_t reserved_rcap, reserved_rthr;
};

struct RayJob {
    uint32_t n_rays;          // poses * B
    uint32_t n_tasks;         // ceil(n_rays / 64): one task = 64 consecutive rays
    uint32_t tasks_per_wave;  // consecutive tasks each wave walks
    int32_t n_poses;
    uint32_t div_magic, div_shift;  // ray / B == umulhi(ray, magic) >> shift (0: plain division)
    int32_t pad_dir, dir_stride;    // k_scan_dirs_agent: distinct directions per agent, rounded up to whole 64-direction tasks
    const void *reserved_dir_ranges;
    uint32_t first_pose, agents_per_env; // k_scan_rays_agent: the launch covers agents first_pose .. (env group); agents_per_env (in a
                                         // formerly reserved word: the layout stays) = the A of scan_task_agent, 1 = agent-major order
    unsigned long long *lookups_total;  // COUNT variants: table lookups of every marched ray, summed (or nullptr)
    // longest-first task order (k_scan_rays_agent<.., SCHED>): see TaskSched
    TaskSched sched;   // by value: the kernel argument segment is the one read a wave never waits long for
    uint32_t epoch_r, epoch_w, long_blocks, agents_inv;   // agents_inv (a formerly reserved word) = scan_task_inv(agents_per_env)
    // fusion-feasibility probe (experimental build): per-env count of finished scan tasks, reset by the last arriver
    uint32_t *env_done;
    uint32_t tasks_per_env, long_prio;
    uint32_t long_rev, pad_rev;   // 1: the long pass walks last step's list from its newest entry (the tasks that finished last)
    // timeline probe (experimental build, k_scan_rays_agent): [launch waves][8] = {begin, end (100 MHz clock), HW_ID | XCC_ID << 32,
    // lock-step samples marched | long pass << 32, task loop entered, first task's stamp + header arrived, its direction /
    // noise operands arrived (march begins), last march done} written by every wave that reaches the end of the kernel; nullptr = off
    unsigned long long *trace;
    // per-env maps: the order the scan walks the agents in — sorted by map slot, so that the XCD-contiguous
    // block order hands each XCD's L2 the agents of as few tracks as possible however the caller interleaved
    // them (nullptr: agent order)
    const uint32_t *order;
    const void *reserved_win[2];
    uint32_t reserved_win_pitch, pad_win;
    const double *pose_x, *pose_y, *dir_start;  // [n_poses] (unit path)
    double *ranges;           // [n_poses][B]
    // STEP only
    const RayHdr *hdr;        // [n_poses] written by k_integrate
    const double *noise;      // [noise_rows][B] or nullptr
    const double *beam_cos, *side_dist;
    int32_t *wall_flag;       // [n_poses], zeroed by k_integrate
    double ttc_thresh;
    double ttc_side_max, ttc_k;  // r > ttc_side_max + ttc_k*|v| cannot satisfy the iTTC predicate
    // unit only
    int32_t *hit_rc;                 // [n_poses][B][2] or nullptr
    unsigned long long *lookups;     // [n_poses] or nullptr
    // diagnostics (unit form; the step form counts per scan in k_integrate), nullptr unless enabled:
    // rays marched {fixed-point only, given up and re-marched exactly, exact throughout}
    unsigned long long *path_stats;
    // HBM copy of the ScanConst the kernel also receives by value: the (very rare) exact re-march of
    // the PADDED layout reads its constants from here, so they cost the fast kernel no registers
    const ScanConst *k_cold;
};

__device__ __forceinline__ int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform_f64(double v)
{
    const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    return __hiloint2double(hi, lo);
}

// Per-agent ray constants for the lane's agent p.  A wave holds 64 consecutive rays, so with >= 64
// rays per agent all its lanes belong to one agent except in the one wave per agent that
// straddles a boundary (1 in 17 at 1080 beams).  Uniform wave: the 64-byte header comes through
// the scalar cache (no vector-memory instruction, no per-lane select); uniform_*() pins the
// fields to SGPRs so the compiler does not turn them back into a divergent vector load.
// Straddling wave: plain per-lane loads.
struct LaneHdr {
    double x, y, start, vel, d0;
    int row, map_slot, i0, n_dirs, fast;
};

__device__ __forceinline__ LaneHdr load_lane_hdr(const RayHdr *hdr, uint32_t p)
{
    LaneHdr o;
    const uint32_t p0 = __builtin_amdgcn_readfirstlane(p);
    if (__ballot(p != p0) == 0ull) {  // wave-uniform branch
        typedef const __attribute__((address_space(4))) RayHdr *chdr_t;
        const chdr_t h0 = (chdr_t)(hdr) + p0;
        o.x = uniform_f64(h0->x);
        o.y = uniform_f64(h0->y);
        o.start = uniform_f64(h0->start);
        o.vel = uniform_f64(h0->vel);
        o.d0 = uniform_f64(h0->d0);
        o.row = uniform_i32(h0->noise_row);
        o.map_slot = uniform_i32(h0->map_slot);
        o.i0 = uniform_i32(h0->i0);
        o.n_dirs = uniform_i32(h0->n_dirs);
        o.fast = uniform_i32(h0->fast);
    } else {
        const RayHdr hd = hdr[p];
        o.x = hd.x; o.y = hd.y; o.start = hd.start; o.vel = hd.vel; o.d0 = hd.d0; o.row = hd.noise_row;
        o.map_slot = hd.map_slot; o.i0 = hd.i0; o.n_dirs = hd.n_dirs;
        o.fast = hd.fast;
    }
    return o;
}

// noise + iTTC + store for one beam (k_scan_rays, k_scan_dirs_agent).
// check_ttc_jit is an any-over-beams: every hitting lane raises the agent's flag.
// r > max(side) + thresh*(1+1e-9)*max|cos|*|v| implies r - side_distances[b] >
// thresh*(1+1e-12)*|v*cosines[b]|, i.e. the "no hit" branch of ttc_beam_hit, so the per-beam
// tables are only read for the few beams that are that close.
struct RayJob;
__device__ __forceinline__ void finish_beam(const RayJob &j, uint32_t B, uint32_t p, int b, uint32_t ray, double r,
                                            int row, double vel);
__device__ __forceinline__ void finish_beam_with(const RayJob &j, uint32_t p, int b, uint32_t ray, double r, double vel);

// all 64 lanes (reconverged after the task loop): sum the per-lane lookup counts, one atomic per wave
__device__ __forceinline__ void wave_add_lookups(unsigned long long *total, uint32_t mine)
{
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63u) == 0u) atomicAdd(total, (unsigned long long)mine);
}

// One ray from its (shared) first sample d0 on.  path: 0 fixed-point march, 1 fixed-point march
// given up and re-marched exactly, 2 exact arithmetic throughout.
template <int LAYOUT, bool POW2, bool IDENT, bool WANT_CELL>
__device__ __forceinline__ double trace_from_first(const ScanConst &k, const ScanConst *k_cold, const double *lut, double x, double y,
                                                   bool fast, double c, double s, double d0, int &hr, int &hc, int &nl,
                                                   int &path)
{
    if (LAYOUT == LAYOUT_PADDED) {
        double r = 0.;
        bool exact = !fast;
        if (fast) {
            double ux, uy, cux, cuy;
            padded_position<IDENT>(k, x, y, ux, uy);
            padded_rate<IDENT>(k, c, s, cux, cuy);
            exact = !march_padded<WANT_CELL>(k, ux, uy, cux, cuy, d0, r, hr, hc, nl);
        }
        path = fast ? (exact ? 1 : 0) : 2;
        if (exact) r = march_exact_cold<IDENT>(k_cold, x, y, c, s, d0, hr, hc, nl);
        return r;
    }
    path = 2;
    return march_from_first<LAYOUT, POW2, IDENT>(k, lut, x, y, c, s, d0, hr, hc, nl);
}

template <int LAYOUT, bool POW2, bool IDENT, bool STEP>
__global__ void __launch_bounds__(256) k_scan_rays(RayJob j, ScanConst k)
{
    const double *lut_lds = nullptr;   // (the byte-code layout's value table: retired in round 5)
    const uint32_t B = (uint32_t)k.num_beams;
    const uint32_t tpw = j.tasks_per_wave;
    const uint32_t lane = threadIdx.x & 63u;
    // Workgroup b is dispatched to XCD b % 8 (observed, MI355X_MICROARCH.md).  Re-map so that each
    // XCD walks one contiguous eighth of the rays: all beams of an agent, and agents that are
    // neighbours in the batch, then share one XCD's L2 instead of being spread over all eight.
    uint32_t blk = blockIdx.x;
    {
        const uint32_t nb = gridDim.x, q = nb >> 3, rem = nb & 7u, x = blk & 7u, i = blk >> 3;
        blk = (x < rem ? x * (q + 1u) : rem * (q + 1u) + (x - rem) * q) + i;  // bijective for any nb
    }
    const uint32_t wave = (blk * blockDim.x + threadIdx.x) >> 6;
    uint32_t nl_acc = 0;   // STEP: table lookups of this lane's rays (summed per wave when counting is on)
    for (uint32_t t = 0; t < tpw; ++t) {
        const uint32_t task = wave * tpw + t;
        if (task >= j.n_tasks) break;  // wave-uniform
        const uint32_t ray = task * 64u + lane;
        if (ray >= j.n_rays) break;
        const uint32_t p = j.div_magic ? (__umulhi(ray, j.div_magic) >> j.div_shift) : ray / B;
        const int b = (int)(ray - p * B);
        int hr, hc, nl, path;
        double r;
        if (STEP) {
            const LaneHdr hd = load_lane_hdr(j.hdr, p);
            hr = -1;
            hc = -1;
            const double2 cs = k.cs[beam_dir_index(k, hd.start, b)];
            r = trace_from_first<LAYOUT, POW2, IDENT, false>(k, j.k_cold, lut_lds, hd.x, hd.y, hd.fast != 0, cs.x, cs.y, hd.d0, hr, hc, nl, path);
            nl_acc += (uint32_t)nl;
            finish_beam(j, B, p, b, ray, r, hd.row, hd.vel);
            continue;
        } else {
            const double2 cs = k.cs[beam_dir_index(k, j.dir_start[p], b)];
            const double x = j.pose_x[p], y = j.pose_y[p];
            const double d0 = sample_distance<LAYOUT, POW2, IDENT>(k, lut_lds, x, y, hr, hc);
            bool fast = false;
            if (LAYOUT == LAYOUT_PADDED) {
                double ux, uy;
                padded_position<IDENT>(k, x, y, ux, uy);
                fast = padded_start_ok(k, ux, uy);
            }
            r = trace_from_first<LAYOUT, POW2, IDENT, true>(k, j.k_cold, lut_lds, x, y, fast, cs.x, cs.y, d0, hr, hc, nl, path);
            if (j.path_stats) atomicAdd(&j.path_stats[path], 1ull);
            if (j.hit_rc) {
                j.hit_rc[(size_t)ray * 2] = hr;
                j.hit_rc[(size_t)ray * 2 + 1] = hc;
            }
            if (j.lookups) atomicAdd(&j.lookups[p], (unsigned long long)nl);
        }
        j.ranges[ray] = r;
    }
    if (STEP && j.lookups_total) wave_add_lookups(j.lookups_total, nl_acc);
}

// ---- K2a: the step's ray march, agent-aligned ----------------------------------------------------
// Same march as k_scan_rays<LAYOUT_PADDED, ..., STEP>, with every agent's beams laid out on whole
// 64-ray tasks (ceil(B/64) tasks per agent, the last one partly idle: 0.7 % of the lanes at 1080
// beams).  A wave then always belongs to ONE agent: the header is scalar in every wave (no per-lane
// header path, no per-lane ray -> (agent, beam) division, lidar position and first sample stay in
// SGPRs) — and the agent's map can be a per-env property (f110_set_env_maps): its constants, one
// 64-byte MapFast record, arrive through the scalar cache next to the header and the loop runs
// with scalar constants exactly as with one map.
struct MapFast {
    const double *pad;                       // the map's padded table
    double pad_cx, pad_cy;                   // padded_position constants (general, rotated form)
    double pad_axx, pad_axy, pad_ayx, pad_ayy;
    uint32_t pad_row_bytes;
    int32_t pad_max_samples;
};
static_assert(sizeof(MapFast) == 64, "MapFast is read as one 64-byte scalar load");

// the per-env map's constants through the scalar cache (one 64-byte record), pinned to SGPRs
__device__ __forceinline__ void load_map_fast(ScanConst &km, const MapFast *__restrict__ maps_fast, int slot)
{
    typedef const __attribute__((address_space(4))) MapFast *cmap_t;
    const cmap_t m0 = (cmap_t)(maps_fast) + slot;
    const uint64_t pa = (uint64_t)m0->pad;
    km.pad = (const double *)(((uint64_t)(uint32_t)uniform_i32((int)(pa >> 32)) << 32) | (uint32_t)uniform_i32((int)pa));
    km.pad_cx = uniform_f64(m0->pad_cx);
    km.pad_cy = uniform_f64(m0->pad_cy);
    km.pad_axx = uniform_f64(m0->pad_axx);
    km.pad_axy = uniform_f64(m0->pad_axy);
    km.pad_ayx = uniform_f64(m0->pad_ayx);
    km.pad_ayy = uniform_f64(m0->pad_ayy);
    km.pad_row_bytes = uniform_i32((int)m0->pad_row_bytes);
    km.pad_max_samples = uniform_i32(m0->pad_max_samples);
}

#ifndef F110_SCAN_WAVES_EXPR
#define F110_SCAN_WAVES_EXPR 8
#endif
// ENV_ORDER: the tasks walk an env's agents sector by sector (scan_task_agent) and the wave keeps its noise samples across them; chosen
// by the host where it was measured to pay (f110_create) or where the caller sets the tasks per wave, never with a per-env order
template <bool PER_ENV_MAP, bool IDENT, bool COUNT, bool SCHED = false, bool ENVCNT = false, bool ENV_ORDER = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(F110_SCAN_WAVES_EXPR))) k_scan_rays_agent(RayJob j, ScanConst k, const MapFast *__restrict__ maps_fast,
                                                          const ScanConst *__restrict__ maps_full, uint32_t tasks_per_agent)
{
    static_assert(!(ENV_ORDER && PER_ENV_MAP), "a per-env order and the env order exclude each other");
    const uint32_t B = (uint32_t)k.num_beams;
    uint32_t tpw = j.tasks_per_wave;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t blk = blockIdx.x;
    typedef const __attribute__((address_space(4))) uint32_t *cu32_t;
    bool long_pass = false;
    uint32_t long_task = 0;
#ifdef F110_EXPERIMENTAL
    const unsigned long long trace_begin = j.trace ? wall_clock64() : 0ull;
    unsigned long long trace_loop = 0ull, trace_hdr = 0ull, trace_ops = 0ull, trace_marched = 0ull;
    uint32_t trace_samples = 0;
#endif
    if (SCHED) {
        if (blk < j.long_blocks) {   // the first blocks of the launch serve last step's long tasks, one per wave
            const TaskSched &sc = j.sched;
            const uint32_t wl = __builtin_amdgcn_readfirstlane((blk * blockDim.x + threadIdx.x) >> 6);
            uint32_t cnt = *(cu32_t)sc.count_r;
            cnt = cnt < sc.cap ? cnt : sc.cap;
            if (wl >= cnt) return;
            long_pass = true;
            long_task = ((cu32_t)sc.list_r)[j.long_rev ? cnt - 1u - wl : wl];
            tpw = 1u;
            if (j.long_prio) __builtin_amdgcn_s_setprio(3);   // (experiment: instruction-issue priority for the waves the launch waits for)
        } else {
            blk -= j.long_blocks;
        }
    }
    if (!long_pass) {
        const uint32_t nb = gridDim.x - (SCHED ? j.long_blocks : 0u), q = nb >> 3, rem = nb & 7u, x = blk & 7u, i = blk >> 3;
        blk = (x < rem ? x * (q + 1u) : rem * (q + 1u) + (x - rem) * q) + i;  // XCD-contiguous, as k_scan_rays
    }
    const uint32_t wave = (blk * blockDim.x + threadIdx.x) >> 6;
    uint32_t nl_acc = 0;
    // PER_ENV_MAP: the map record is (re)loaded only when the slot changes — the wave's consecutive tasks belong to
    // one or two agents, and the scan order groups the agents by slot (f110_set_env_maps)
    ScanConst km = k;
    const ScanConst *cold = j.k_cold;
    int cur_slot = -1;
    // ENV_ORDER: the tasks walk an env's agents sector by sector (scan_task_agent): the wave's consecutive tasks are
    // the same 64 beams of the env's cars, and all agents of an env are on the same noise row (they are reset together; the
    // reference gives every car a generator of the same seed) — the lane's sample stays in `held` while the wave-uniform key
    // (row, sector) stays the same.  held_row < 0: nothing held.  A task on last step's long list is skipped before the key is
    // touched, so it never leaves a key that the held sample does not match.
    double held = 0.0;
    int held_row = -1;
    uint32_t held_sec = 0;
#ifdef F110_EXPERIMENTAL
    if (j.trace) trace_loop = wall_clock64();
#endif
    for (uint32_t t = 0; t < tpw; ++t) {
        const uint32_t task = __builtin_amdgcn_readfirstlane(long_pass ? long_task : wave * tpw + t);
        if (task >= j.n_tasks) break;
        uint32_t pl, sec = 0;                                       // scalar
        if (!ENV_ORDER) pl = task / tasks_per_agent;
        else scan_task_agent(task, tasks_per_agent, j.agents_per_env, j.agents_inv, pl, sec);
        const uint32_t p = (PER_ENV_MAP && j.order) ? ((cu32_t)j.order)[pl] : j.first_pose + pl;
        // the task's two cold words — its stamp on last step's long list and its agent's header, both written by
        // other kernels on other XCDs — are requested together: one memory round trip, not two in a row (a small
        // batch is bound by its per-task latency chain: tools/debug/scan_timeline.py).  Measured and NOT done: keeping
        // the header in SGPRs while consecutive tasks belong to one agent (65 536 agents 92.1 -> 86.9 M agent-steps/s:
        // the loop-carried scalars cost more than the scalar-cache hit they save), and requesting the next task's
        // direction / noise operands before this task's march (92.1 -> 91.7).
        const uint32_t stamp = (SCHED && !long_pass) ? ((cu32_t)j.sched.flags_r)[task] : 0u;
        typedef const __attribute__((address_space(4))) RayHdr *chdr_t;
        const chdr_t h0 = (chdr_t)(j.hdr) + p;
        const double x = uniform_f64(h0->x), y = uniform_f64(h0->y), start = uniform_f64(h0->start);
        const double vel = uniform_f64(h0->vel), d0 = uniform_f64(h0->d0);
        const int row = uniform_i32(h0->noise_row), slot = uniform_i32(h0->map_slot), fast = uniform_i32(h0->fast);
#ifdef F110_EXPERIMENTAL
        if (j.trace && trace_hdr == 0ull) trace_hdr = wall_clock64();   // (reading the clock waits for the scalar loads above)
#endif
        if (SCHED && !long_pass && stamp == j.epoch_r) continue;   // served by the long pass
        // (decided here, where the wave is still whole, so that the key lives in SGPRs.  The lanes that leave at b >= B below
        // miss the load under a key that says "held" — and hold no beam in any task of that key: b depends on sector and lane only)
        const bool load_nz = !ENV_ORDER || row < 0 || row != held_row || sec != held_sec;   // row -2 is the agent's own row: never shared
        if (ENV_ORDER) {
            held_row = row;
            held_sec = sec;
        }
        const int b = (int)((ENV_ORDER ? sec : task - pl * tasks_per_agent) * 64u + lane);
        if (b >= (int)B) continue;
        if (PER_ENV_MAP && slot != cur_slot) {   // wave-uniform
            cold = maps_full + slot;
            load_map_fast(km, maps_fast, slot);
            cur_slot = slot;
        }
        // the beam's noise sample is requested before the march so that its latency hides under it:
        // row of the table / row cache, or (row -2) the row k_noise_rows left in this agent's scans[]
        const double *nrow = row >= 0 ? j.noise + (size_t)row * B : j.ranges + (size_t)p * B;   // scalar
        if (ENV_ORDER && load_nz) held = row != -1 ? nrow[b] : 0.0;   // wave-uniform
        const double nz = ENV_ORDER ? held : (row != -1 ? nrow[b] : 0.0);
        double2 cs = k.cs[beam_dir_index(k, start, b)];
#ifdef F110_EXPERIMENTAL
        if (j.trace && trace_ops == 0ull) {
            asm volatile("" : "+v"(cs.x), "+v"(cs.y));   // (the direction has arrived)
            trace_ops = wall_clock64();
        }
#endif
        int hr = -1, hc = -1, nl = 0;
        double r = 0.;
        bool exact = fast == 0;
        if (fast) {
            double ux, uy, cux, cuy;
            padded_position<IDENT>(km, x, y, ux, uy);
            padded_rate<IDENT>(km, cs.x, cs.y, cux, cuy);
            exact = !march_padded<false>(km, ux, uy, cux, cuy, d0, r, hr, hc, nl);
        }
        if (exact) r = march_exact_cold<IDENT>(cold, x, y, cs.x, cs.y, d0, hr, hc, nl);
        if (COUNT) nl_acc += (uint32_t)nl;   // measurement variant only (bench.py's L-bar)
#ifdef F110_EXPERIMENTAL
        if (j.trace) {
            asm volatile("" : "+v"(r));
            trace_marched = wall_clock64();
        }
        if (j.trace) {   // the task's lock-step length = its longest ray
            int m = 0;   // max over the lanes that hold a beam, bit by bit (ten compares; a cheap probe distorts least)
            for (int bit = 1 << 10; bit; bit >>= 1)
                if (__ballot(nl >= (m | bit)) != 0ull) m |= bit;
            trace_samples += (uint32_t)m;
        }
#endif
        if (SCHED) {
            const TaskSched &sc = j.sched;
            if (__ballot(nl > (int)sc.thr) != 0ull && lane == 0u) {
                // lane 0 (beam task*64, always a valid beam) appends the task for the next step
                const uint32_t pos = atomicAdd(sc.count_w, 1u);
                if (pos < sc.cap) {
                    sc.list_w[pos] = task;
                    sc.flags_w[task] = j.epoch_w;
                }
            }
        }
        finish_beam_with(j, p, b, p * B + (uint32_t)b, row != -1 ? r + nz : r, vel);
        if (ENVCNT && lane == 0u) {
            // probe: what a per-env completion counter costs (one returning agent-scope atomic per task; the
            // arrival that completes the env resets the counter, as a fused finalize would before it runs)
            const uint32_t env = p / (j.tasks_per_env / tasks_per_agent);
            const uint32_t old = __hip_atomic_fetch_add(j.env_done + env, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (old + 1u == j.tasks_per_env) __hip_atomic_store(j.env_done + env, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (COUNT) wave_add_lookups(j.lookups_total, nl_acc);
#ifdef F110_EXPERIMENTAL
    if (j.trace && lane == 0u) {
        uint32_t hw_id, xcc_id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
        unsigned long long *rec = j.trace + 8ull * ((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
        rec[0] = trace_begin;
        rec[1] = wall_clock64();
        rec[2] = (unsigned long long)hw_id | ((unsigned long long)xcc_id << 32);
        rec[3] = (unsigned long long)trace_samples | ((unsigned long long)(long_pass ? 1u : 0u) << 32);
        rec[4] = trace_loop;
        rec[5] = trace_hdr;
        rec[6] = trace_ops;
        rec[7] = trace_marched;
    }
#endif
}

// (Round 5 built k_scan_stream_agent here — "survivor compaction": a wave owns an agent's whole scan as a queue and re-fills finished
// lanes; 0.65-0.79 of the wave-level gathers, bit-identical — and measured it 7-20 % slower at every setting: the re-filled wave's rays
// share fewer lines, and the scan is bound by line traffic, not by instruction count.  Retired in round 6 under the pre-registered
// stop rule: DESIGN.md §8, profiles/r05_stream_scan.txt, r05_pmc_stream_vs_base.json.)

// iTTC + store for one beam whose noise sample has been added already
__device__ __forceinline__ void finish_beam_with(const RayJob &j, uint32_t p, int b, uint32_t ray, double r, double vel)
{
    if (vel != 0.0 && !(r > j.ttc_side_max + j.ttc_k * fabs(vel)) &&
        ttc_beam_hit(r, j.side_dist[b], vel, j.beam_cos[b], j.ttc_thresh))
        j.wall_flag[p] = 1;
    // (round 6 measured non-temporal range stores here for small batches — does the table stay in L2 when 35 MB of range writes per
    // step bypass it? — no change at any size, +-0.2 %: profiles/r06_nt_store.txt)
    j.ranges[ray] = r;
}

__device__ __forceinline__ void finish_beam(const RayJob &j, uint32_t B, uint32_t p, int b, uint32_t ray, double r,
                                            int row, double vel)
{
    if (row >= 0)
        r += j.noise[(size_t)row * B + b];
    else if (row == -2)
        r += j.ranges[ray];   // this step's noise row, left in the agent's scans[] by k_noise_rows
    finish_beam_with(j, p, b, ray, r, vel);
}

// ---- K2d: more beams than table directions, one pass -----------------------------------------------
// BASELINE config 5 (4096 beams, theta_dis = 2000 -> 1497 distinct directions per scan).  Agent-aligned
// like k_scan_rays_agent, but a task is 64 consecutive DISTINCT directions of one agent: each lane
// marches one direction once, then the wave writes the ~175 consecutive beams that use those 64
// directions in coalesced passes of 64 — beam b takes its range from lane rel(b) - s0 by shuffle and
// gets its own noise sample and iTTC test.  Replaces the (march to a [N][dir_stride] buffer,
// k_expand_beams) pair: one launch less and no 1.6 GB round trip of intermediate ranges per step.
// Bit-identical to marching every beam (beams that share a table index from one origin are one ray).
#ifndef F110_DIRS_WAVES_EXPR
#define F110_DIRS_WAVES_EXPR 8
#endif
template <bool PER_ENV_MAP, bool IDENT, bool COUNT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(F110_DIRS_WAVES_EXPR))) k_scan_dirs_agent(RayJob j, ScanConst k, const MapFast *__restrict__ maps_fast,
                                                          const ScanConst *__restrict__ maps_full, uint32_t tasks_per_agent)
{
    const uint32_t B = (uint32_t)k.num_beams;
    const uint32_t tpw = j.tasks_per_wave;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t blk = blockIdx.x;
    {
        const uint32_t nb = gridDim.x, q = nb >> 3, rem = nb & 7u, x = blk & 7u, i = blk >> 3;
        blk = (x < rem ? x * (q + 1u) : rem * (q + 1u) + (x - rem) * q) + i;  // XCD-contiguous, as k_scan_rays
    }
    const uint32_t wave = (blk * blockDim.x + threadIdx.x) >> 6;
    uint32_t nl_acc = 0;
    ScanConst km = k;   // PER_ENV_MAP: this agent's track (f110_set_env_maps), reloaded when the slot changes
    const ScanConst *cold = j.k_cold;
    int cur_slot = -1;
    for (uint32_t t = 0; t < tpw; ++t) {
        const uint32_t task = __builtin_amdgcn_readfirstlane(wave * tpw + t);
        if (task >= j.n_tasks) break;
        const uint32_t pl = task / tasks_per_agent;
        typedef const __attribute__((address_space(4))) uint32_t *cu32_t;
        const uint32_t p = (PER_ENV_MAP && j.order) ? ((cu32_t)j.order)[pl] : j.first_pose + pl;
        const int s0 = (int)((task - pl * tasks_per_agent) * 64u);
        typedef const __attribute__((address_space(4))) RayHdr *chdr_t;
        const chdr_t h0 = (chdr_t)(j.hdr) + p;
        const int n_dirs = uniform_i32(h0->n_dirs);
        if (s0 >= n_dirs) continue;   // wave-uniform: the padding tasks of dir_stride
        const double x = uniform_f64(h0->x), y = uniform_f64(h0->y), start = uniform_f64(h0->start);
        const double vel = uniform_f64(h0->vel), d0 = uniform_f64(h0->d0);
        const int row = uniform_i32(h0->noise_row), fast = uniform_i32(h0->fast), i0 = uniform_i32(h0->i0);
        if (PER_ENV_MAP) {
            const int slot = uniform_i32(h0->map_slot);
            if (slot != cur_slot) {   // wave-uniform
                cold = maps_full + slot;
                load_map_fast(km, maps_fast, slot);
                cur_slot = slot;
            }
        }
        // first beam whose table index is direction s0 (relative indices never decrease with the beam):
        // closed-form estimate, then the exact index function decides
        auto rel_of = [&](int b) {
            int rr = beam_dir_index(k, start, b) - i0;
            return rr < 0 ? rr + k.theta_dis : rr;
        };
        int b0 = 0;
        if (s0 > 0) {
            b0 = (int)ceil(((double)s0 - (start - floor(start))) / k.theta_inc) - 2;
            b0 = b0 < 0 ? 0 : (b0 >= (int)B ? (int)B - 1 : b0);
            b0 = __builtin_amdgcn_readfirstlane(b0);
            while (b0 > 0 && rel_of(b0 - 1) >= s0) --b0;
            while (b0 < (int)B && rel_of(b0) < s0) ++b0;
        }
        // Which beams this task writes, which lane's direction each of them takes and its noise sample are all known BEFORE the
        // march: the first kPre passes of 64 beams (~175 beams per task at 4096 beams on 2000 directions: three passes) ask for
        // their noise here, so that the loads fly under the march instead of forming a dependent load -> store round trip per
        // pass behind it (round 5: the kernel is a latency chain per task — 9 dependent gathers, then three such round trips)
        constexpr int kPre = 3;
        const double *nrow = row >= 0 ? j.noise + (size_t)row * B : j.ranges + (size_t)p * B;   // (row -2: this step's noise row, left in the agent's scans[] by k_noise_rows)
        bool pre_in[kPre];
        int pre_src[kPre];
        double pre_nz[kPre];
#pragma unroll
        for (int q = 0; q < kPre; ++q) {
            const int b = b0 + (int)lane + 64 * q;
            bool in = b < (int)B;
            int src = 0;
            if (in) {
                src = rel_of(b) - s0;
                in = src < 64;
            }
            pre_in[q] = in;
            pre_src[q] = src;
            pre_nz[q] = (in && row != -1) ? nrow[b] : 0.0;
        }
        double r_dir = 0.;
        if (s0 + (int)lane < n_dirs) {
            int didx = i0 + s0 + (int)lane;
            if (didx >= k.theta_dis) didx -= k.theta_dis;
            const double2 cs = k.cs[didx];
            int hr = -1, hc = -1, nl;
            bool exact = fast == 0;
            if (fast) {
                double ux, uy, cux, cuy;
                padded_position<IDENT>(km, x, y, ux, uy);
                padded_rate<IDENT>(km, cs.x, cs.y, cux, cuy);
                exact = !march_padded<false>(km, ux, uy, cux, cuy, d0, r_dir, hr, hc, nl);
            }
            if (exact) r_dir = march_exact_cold<IDENT>(cold, x, y, cs.x, cs.y, d0, hr, hc, nl);
            if (COUNT) nl_acc += (uint32_t)nl;
        }
        // the write passes (every lane takes part in every shuffle); the indices are monotone: the first pass with an idle lane is the last
        bool more = true;
#pragma unroll
        for (int q = 0; q < kPre; ++q) {
            if (more) {
                const int b = b0 + (int)lane + 64 * q;
                const double r = __shfl(r_dir, pre_in[q] ? pre_src[q] : 0);
                if (pre_in[q]) finish_beam_with(j, p, b, p * B + (uint32_t)b, row != -1 ? r + pre_nz[q] : r, vel);
                if (__ballot(!pre_in[q]) != 0ull) more = false;
            }
        }
        for (int b = b0 + (int)lane + 64 * kPre; more; b += 64) {   // (more beams per direction than kPre passes cover: load, then store)
            bool in = b < (int)B;
            int src = 0;
            if (in) {
                src = rel_of(b) - s0;
                in = src < 64;
            }
            const double r = __shfl(r_dir, in ? src : 0);
            if (in) finish_beam(j, B, p, b, p * B + (uint32_t)b, r, row, vel);
            if (__ballot(!in) != 0ull) more = false;
        }
    }
    if (COUNT) wave_add_lookups(j.lookups_total, nl_acc);
}


// ---- scan noise generated on the device --------------------------------------------
// rng.normal(0., std, num_beams) of laser_models.py:450-452 — NumPy's PCG64 + ziggurat, restated in
// f110_rng.hpp.  One wave produces one row of B samples: lane l evaluates the attempt that would
// start at draw l of the current 64-draw chunk (its generator state comes from the jump constants:
// A^(l+1) * s + G_(l+1) * inc), the few attempts that consume more than one draw decide which
// positions really start an attempt (zig_chain_starts), and the accepted values are packed in order.
struct NoiseGen {
    const uint64_t *zk;   // ziggurat tables (device copies)
    const double *zw, *zf;
    const U128 *ja, *jg;  // PcgJump (device copy): [65] each
    double scale;         // std_dev of the noise (loc = 0.)
};

// `state` (wave-uniform): stream position at the start of the row in, at its end out
__device__ __forceinline__ void noise_row_wave(const NoiseGen &g, U128 &state, const U128 inc, double *__restrict__ out, int B)
{
    const int lane = (int)(threadIdx.x & 63u);
    const ZigTables zt = {g.zk, g.zw, g.zf};
    const U128 aj = g.ja[lane + 1];
    const U128 gi = mul128(g.jg[lane + 1], inc);
    const uint64_t below = (1ull << lane) - 1ull;
    int produced = 0, skip = 0;
    U128 s = state;
    for (;;) {
        const U128 st = add128(mul128(aj, s), gi);
        const ZigAttempt z = zig_attempt(pcg_output(st), st, inc, zt);
        const uint64_t multi = __ballot(z.len > 1);
        int skip_out;
        const uint64_t starts = zig_chain_starts(multi, skip, [&](int p) { return __builtin_amdgcn_readlane(z.len, p); }, skip_out);
        const uint64_t em = starts & __ballot(z.emit);
        const int idx = produced + popc_u64(em & below);
        if (((em >> lane) & 1ull) && idx < B) out[idx] = 0.0 + g.scale * z.val;  // loc + scale * z (random_normal)
        const int cnt = popc_u64(em);
        if (produced + cnt >= B) {
            const int e = nth_set_bit(em, B - produced - 1);
            state = pcg_advance(s, inc, g.ja, g.jg, e + __builtin_amdgcn_readlane(z.len, e));
            return;
        }
        produced += cnt;
        skip = skip_out;
        s = pcg_advance(s, inc, g.ja, g.jg, 64);
    }
}

__device__ __forceinline__ U128 uniform_u128(U128 v)
{
    U128 o;
    o.hi = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v.hi >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v.hi);
    o.lo = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(v.lo >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)v.lo);
    return o;
}

// rows [row0, row1) of the shared stream into the row cache, one after the other (a row's start
// depends on how many draws the previous rows consumed); rowstate[r] = stream position at row r.
__global__ void __launch_bounds__(64) k_noise_cache(NoiseGen g, U128 inc, U128 *__restrict__ rowstate, double *__restrict__ cache, int row0,
                                                    int row1, int B)
{
    U128 state = uniform_u128(rowstate[row0]);
    for (int r = row0; r < row1; ++r) {
        noise_row_wave(g, state, inc, cache + (size_t)r * B, B);
        if ((threadIdx.x & 63u) == 0u) rowstate[r + 1] = state;
    }
}

// this step's noise row of every agent the row cache cannot serve (per-agent streams; episodes
// longer than the cache), generated into the agent's own scans[] row where the scan kernel picks it up
// (RayHdr::noise_row == -2).  A 256-thread workgroup first checks `agents_per_block` agents one lane each
// and lists the ones that need a row; its four waves then generate the listed rows, a wave per row.  In
// the shared-stream mode the list is almost always empty, and a launch of N / 256 workgroups that look
// and leave costs a couple of microseconds — the host cannot know the longest live episode without a
// round trip (re-seats happen on the device), so the launch is unconditional once the steps since the
// last full reset exceed the cache.
__global__ void __launch_bounds__(256) k_noise_rows(AgentArrays a, NoiseGen g, int B, int agents_per_block)
{
    __shared__ int list[256];
    __shared__ int n_listed;
    if (threadIdx.x == 0) n_listed = 0;
    __syncthreads();
    const int end = a.agent_begin + a.agent_count;
    const int i = a.agent_begin + (int)blockIdx.x * agents_per_block + (int)threadIdx.x;
    if ((int)threadIdx.x < agents_per_block && i < end && (a.noise_rng == 2 || a.step_count[i] >= a.noise_rows))
        list[atomicAdd(&n_listed, 1)] = i;
    __syncthreads();
    const int n = n_listed;
    for (int q = (int)(threadIdx.x >> 6); q < n; q += 4) {
        const int ag = __builtin_amdgcn_readfirstlane(list[q]);
        const int k = __builtin_amdgcn_readfirstlane(a.step_count[ag]);
        U128 state, inc;
        if (a.noise_rng == 2) {
            inc = uniform_u128(a.rng_seed[2 * (size_t)ag + 1]);
            state = uniform_u128(k == 0 ? a.rng_seed[2 * (size_t)ag] : a.rng_state[ag]);
        } else {
            inc = a.rng_inc;
            state = uniform_u128(k == a.noise_rows ? a.rng_rowstate[a.noise_rows] : a.rng_state[ag]);
        }
        noise_row_wave(g, state, inc, a.scans + (size_t)ag * B, B);
        if ((threadIdx.x & 63u) == 0u) a.rng_state[ag] = state;
    }
}

// In-place re-seat of one agent of a finished env (f110_reset_collided_device / auto re-seat): what
// k_reset does for a masked env.  collisions[] keeps the step's value, as Simulator.collisions does,
// and so does in_collision[] here (k_integrate clears it at the next step; other waves of this
// kernel may still be reading the ego's flag).
__device__ __forceinline__ void reseat_agent(const AgentArrays &a, int i, bool count)
{
    const int N = a.n_agents_total;
#pragma unroll
    for (int c = 0; c < 7; ++c) a.state[(size_t)c * N + i] = 0.;
    a.state[i] = a.reseat_poses[3 * (size_t)i];
    a.state[(size_t)N + i] = a.reseat_poses[3 * (size_t)i + 1];
    a.state[4 * (size_t)N + i] = a.reseat_poses[3 * (size_t)i + 2];
    a.steer_buf[i] = 0.;
    a.steer_buf[(size_t)N + i] = 0.;
    a.buf_cnt[i] = 0;
    a.step_count[i] = 0;
    if (count && a.reseat_count) atomicAdd(a.reseat_count, 1);
}

// ---- K3: finalize ---------------------------------------------------------------------------
// kFinalizeLanes lanes per agent.  A typical opponent window is ~36 beams and what one agent costs
// is a chain of memory round trips and float64 latencies, not throughput: with many agents, 16
// lanes each (four agents per wave) means a quarter of the waves for the same chains; with few
// agents the whole wave per agent (one pass over the window) is the shorter chain.
// RaceCar.check_ttc's side effects (:246-252), Simulator's collision OR (:588-589), then
// RaceCar.ray_cast_agents (:206-227): opponents from the :574 snapshot, ego pose = live state
// (heading already zeroed on a wall hit), box = the ego's own params.
template <int kFinalizeLanes>
__global__ void __launch_bounds__(256) k_finalize(AgentArrays a, int32_t B)
{
    constexpr int kFinalizeAgents = 256 / kFinalizeLanes;   // per 256-thread workgroup
    const int i = a.agent_begin + (int)(blockIdx.x * kFinalizeAgents + threadIdx.x / kFinalizeLanes), tid = threadIdx.x & (kFinalizeLanes - 1);
    const int N = a.n_agents_total, A = a.agents_per_env;
    if (i >= a.agent_begin + a.agent_count) return;
    // everything the wave may need is requested up front (one round trip), not behind the flag
    const int wall = a.in_collision[i];
    const double ex = a.state[i], ey = a.state[(size_t)N + i];
    const double th_live = a.state[4 * (size_t)N + i];
    const int me = i % A;
    const double eth = wall ? 0.0 : th_live;
    if (tid == 0) {
        if (wall) {
            a.state[3 * (size_t)N + i] = 0.;
            a.state[4 * (size_t)N + i] = 0.;
            a.state[5 * (size_t)N + i] = 0.;
            a.state[6 * (size_t)N + i] = 0.;
            a.collisions[i] = 1.0;
        }
        a.step_count[i] += 1;
    }
    double *sc = a.scans + (size_t)i * B;
    for (int jj = 0; jj < A; ++jj) {
        if (jj == me) continue;
        const int4 w4 = *reinterpret_cast<const int4 *>(a.opp_window + ((size_t)i * A + jj) * 4);
        const double *ov = a.opp_verts + ((size_t)i * A + jj) * 8;
        double v[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) v[c] = ov[c];
        const int lo = wall ? w4.z : w4.x, hi = wall ? w4.w : w4.y;
        if (hi < lo) continue;  // nothing of this opponent can be hit
        for (int b = lo + tid; b <= hi; b += kFinalizeLanes) {
            const double bt = eth + a.scan_angles[b];
            const double r0 = sc[b];
            double v3x, v3y;
            sincos(bt + kPi / 2., &v3y, &v3x);  // one argument reduction for both (get_range :259-260)
            const double r = box_range(ex, ey, v3x, v3y, v, r0);
            if (r < r0) sc[b] = r;
        }
        // the next opponent may touch the same beams: make this wave's stores visible to it
        __threadfence_block();
    }
    if (a.reseat_poses && tid == 0) {
        // the ego's collisions value of this step = pair test (k_collide, complete) OR its wall flag
        // (k_scan_rays, complete); neither input is written by this kernel's re-seat
        const int ego = (i / A) * A + a.reseat_ego;
        if (a.collisions[ego] != 0.0 || a.in_collision[ego] != 0) reseat_agent(a, i, i == ego);
    }
}

// ---- f110_step_host's work as the pair kernel's epilogue (round 4) -----------------------------------------------
// What k_host_block does in a launch of its own, done by the agent threads of k_finalize_pair_roles (lanes t < AG of
// wave 0; the two agents of an env are lanes t, t ^ 1) once the kernel's own work is finished: the agent's columns into
// the caller's page-locked block, F110Env._check_done for the env, the in-place re-seat.  Same arithmetic as
// k_host_block / k_episode (tests: the VecEnv forms agree, the reference's 2-agent episodes).
__device__ __forceinline__ void pair_host_epilogue_with(const AgentArrays &a, const EpisodeArrays &ep, const HostBlock &hb, const int episode, const int auto_reset,
                                                        bool agent_thread, int i)
{
    const size_t N = (size_t)a.n_agents_total;
    double col = 0.;
    int running = 0;
    double ct = 0.;
    if (agent_thread) {
        const size_t iu = (size_t)i;
        const double x = a.state[iu], y = a.state[N + iu];
        if (hb.state) {
            hb.state[iu] = x;
            hb.state[N + iu] = y;
#pragma unroll
            for (int c = 2; c < 7; ++c) hb.state[c * N + iu] = a.state[c * N + iu];
        }
        col = a.collisions[iu];
        if (hb.collisions) hb.collisions[iu] = col;
        if (hb.collision_idx) hb.collision_idx[iu] = a.collision_idx[iu];
        if (hb.in_collision) hb.in_collision[iu] = a.in_collision[iu];
        if (hb.agent_poses) {
#pragma unroll
            for (int c = 0; c < 3; ++c) hb.agent_poses[c * N + iu] = a.snap_pose[c * N + iu];
        }
        if (episode) {
            const int e = i >> 1;
            ct = ep.current_time[e] + ep.timestep;  // f110_env.py:295 (written back by the env's even lane below)
            const double r00 = ep.rot[4 * e], r01 = ep.rot[4 * e + 1], r10 = ep.rot[4 * e + 2], r11 = ep.rot[4 * e + 3];
            const double left_t = 2, right_t = 2;
            const double px = x - ep.start_poses[3 * iu];
            const double py = y - ep.start_poses[3 * iu + 1];
            const double dx = r00 * px + r01 * py;  // np.dot(start_rot, [px; py]) :223
            double ty = r10 * px + r11 * py;
            if (ty > left_t)
                ty -= left_t;
            else if (ty < -right_t)
                ty = -right_t - ty;
            else
                ty = 0;
            const double dist2 = dx * dx + ty * ty;
            const bool closes = dist2 <= 0.1;
            bool near = ep.near_start[iu] != 0;
            double tog = ep.toggle[iu];
            if (closes && !near) {
                near = true;
                tog += 1;
            } else if (!closes && near) {
                near = false;
                tog += 1;
            }
            const double laps = floor(tog / 2);  // toggle_list // 2
            ep.near_start[iu] = near ? 1 : 0;
            ep.toggle[iu] = tog;
            ep.lap_count[iu] = laps;
            double lt = ep.lap_time[iu];
            if (tog < 4) {
                lt = ct;
                ep.lap_time[iu] = ct;
                running = 1;
            }
            ep.checkpoint[iu] = tog >= 4 ? 1 : 0;
            if (hb.lap_time) hb.lap_time[iu] = lt;
            if (hb.lap_count) hb.lap_count[iu] = laps;
            if (hb.toggle) hb.toggle[iu] = tog;
            if (hb.near_start) hb.near_start[iu] = near ? 1 : 0;
            if (hb.checkpoint) hb.checkpoint[iu] = tog >= 4 ? 1 : 0;
        }
    }
    // the env's other agent is the neighbouring lane (every lane of the wave takes part in the shuffles)
    const double col_o = __shfl_xor(col, 1);
    const int run_o = __shfl_xor(running, 1);
    if (episode && agent_thread) {
        const size_t iu = (size_t)i;
        const int me = i & 1, e = i >> 1;
        const double ego_col = (me == ep.ego_idx) ? col : col_o;
        const bool done = ego_col != 0.0 || (running == 0 && run_o == 0);  // :244
        const bool reseat = auto_reset && done;
        if (me == 0) {
            if (hb.current_time) hb.current_time[e] = ct;
            if (hb.done) hb.done[e] = done ? 1 : 0;
            ep.done[e] = (done && !reseat) ? 1 : 0;
            ep.current_time[e] = reseat ? 0. : ct;
        }
        if (reseat) {   // F110Env.reset :319-334 without its zero-action step
#pragma unroll
            for (int c = 0; c < 7; ++c) a.state[c * N + iu] = 0.;
            a.state[iu] = ep.start_poses[3 * iu];
            a.state[N + iu] = ep.start_poses[3 * iu + 1];
            a.state[4 * N + iu] = ep.start_poses[3 * iu + 2];
            a.steer_buf[iu] = 0.;
            a.steer_buf[N + iu] = 0.;
            a.buf_cnt[iu] = 0;
            a.in_collision[iu] = 0;
            a.step_count[iu] = 0;
            ep.near_start[iu] = 1;
            ep.toggle[iu] = 0.;
        }
    }
}

// ... with the parameters where the launcher left them in device memory (k_finalize_pair_roles; k_step_tiny's general body)
__device__ __forceinline__ void pair_host_epilogue(const AgentArrays &a, bool agent_thread, int i)
{
    const FusedHost *fp = a.fused_host;
    const EpisodeArrays ep = fp->ep;
    const HostBlock hb = fp->hb;
    pair_host_epilogue_with(a, ep, hb, fp->episode, fp->auto_reset, agent_thread, i);
}

// ---- K3r: finalize for two-agent envs — pair test, opponent window and ray-cast in one kernel (rounds 2-3) ----------
// What k_collide prepares for k_finalize — the GJK flag of the env's one pair and the beam window the opponent can
// occupy — costs a second stream and an event fork/join per step (14 us); with two agents per env it sits at the top of
// the finalize kernel instead.  The workgroup's threads are dealt by ROLE: the 4 AG box corners (-> beam indices) fill
// waves 0-1, the AG disc culls sit in wave 2, the AG / 2 pair tests (ONE per env: both agents' calls are the same
// gjk_overlap(box(2e), box(2e + 1)) on the same numbers) in wave 3; each wave runs only its own piece, the pieces run side
// by side on the CU's four SIMDs, results meet in LDS.  Then the opponent windows of the workgroup's AG agents are
// flattened into one item list (a crashed pair sees windows of up to all beams; fixed lanes per agent serialise there).
// Same functions on the same operands as k_collide + k_finalize: bit-identical.  (The earlier forms — fixed lanes per
// agent, the prologue dealt by agent — were measured slower in round 3 and retired in round 5: DESIGN_HISTORY.md.)
// (Round 5 also ran this body as one-wave workgroups at 8 waves per SIMD, NT = 64, the three roles as branches of the one wave, so
// that a second env block's finalize fits under the first block's scan: it hid, and cost what it hid (profiles/r05_finalize_wave.txt).
// The one-wave form a two-block step launches today is K3w below, finalize_pair_wave_body, with the roles merged.)
// The body is a device function of a 256-thread workgroup over the AG agents [first, first + AG) (round 6): k_finalize_pair_roles
// runs it once per workgroup; k_step_tiny — the whole step of a tiny batch as ONE launch — runs it in its last workgroup.
template <int AG, bool HOST>
__device__ __forceinline__ void finalize_pair_body(const AgentArrays &a, int32_t B, const int first, const int end)
{
    constexpr int NT = 256;
    static_assert((AG & (AG - 1)) == 0 && AG >= 2 && 4 * AG <= NT / 2, "AG is a power of two, 2..32");
    constexpr int R1 = 128, R2 = 192;   // first thread of the cull / the pair-test role
    static_assert(R2 + AG / 2 <= NT, "the three roles fit the workgroup");
    __shared__ double s_rec[AG][12];   // ex, ey, eth, the opponent's box (8), pad
    __shared__ int s_idx[AG][4], s_cl[AG], s_ch[AG], s_hit[AG / 2];
    __shared__ int s_lo[AG], s_cnt[AG], s_off[AG + 1];
    const int t = (int)threadIdx.x;
    const int N = a.n_agents_total;
    int role = -1, slot = 0, sub = 0;
    if (t < 4 * AG) {                        // waves 0-1: box corner `sub` of agent `slot`'s opponent -> beam index
        role = 0; slot = t >> 2; sub = t & 3;
    } else if (t >= R1 && t < R1 + AG) {   // wave 2: disc cull of agent `slot`
        role = 1; slot = t - R1;
    } else if (t >= R2 && t < R2 + AG / 2) {   // wave 3: the pair test of env (slot, slot + 1)
        role = 2; slot = 2 * (t - R2);
    }
    if (role >= 0 && first + slot < end) {
        const int i = first + slot, me = i & 1, o = i ^ 1;
        const double ex = a.state[i], ey = a.state[(size_t)N + i];
        const double th_live = a.state[4 * (size_t)N + i];   // == the :574 snapshot heading: nothing has zeroed it yet
        const double ox = a.snap_pose[o], oy = a.snap_pose[(size_t)N + o], oth = a.snap_pose[2 * (size_t)N + o];
        if (role == 2) {
            // collision_multiple on the env's one pair, boxes with the Simulator's length / width (:549); i is the
            // even agent: gjk_overlap(mine, other) here is gjk_overlap(other, mine) of the odd agent's call
            int hit = 0;
            const double reach = sqrt(a.box_length * a.box_length + a.box_width * a.box_width) + 1e-3;
            const double cdx = ox - ex, cdy = oy - ey;
            if (cdx * cdx + cdy * cdy <= reach * reach) {
                double mine[8], other[8];
                box_vertices(ex, ey, th_live, a.box_length, a.box_width, mine);
                box_vertices(ox, oy, oth, a.box_length, a.box_width, other);
                hit = gjk_overlap(mine, other) ? 1 : 0;
            }
            s_hit[slot >> 1] = hit;
        } else {
            const int wall = a.in_collision[i];
            const double eth = wall ? 0.0 : th_live;
            const size_t prow = (size_t)(a.params_per_agent ? i : me) * NPARAMS;
            const double blen = a.params[prow + P_LENGTH], bwid = a.params[prow + P_WIDTH];
            double v[8];   // the opponent drawn with MY length / width (RaceCar.ray_cast_agents :223)
            box_vertices(ox, oy, oth, blen, bwid, v);
            double ce_, se_;
        cos_sin(eth, ce_, se_);
        const double head = atan2(se_, ce_);
            const double px = role == 1 ? ox : (sub == 0 ? v[0] : (sub == 1 ? v[2] : (sub == 2 ? v[4] : v[6])));
            const double py = role == 1 ? oy : (sub == 0 ? v[1] : (sub == 1 ? v[3] : (sub == 2 ? v[5] : v[7])));
            const double dx = px - ex, dy = py - ey;
            const double norm = sqrt(dx * dx + dy * dy);
            const double qx = role == 0 ? dx / norm : dx, qy = role == 0 ? dy / norm : dy;
            const double dir = atan2(qy, qx);
            if (role == 0) {
                s_idx[slot][sub] = vertex_beam_from_angles(head, dir, a.scan_angles, B, a.angle_inc);
                if (sub == 0) {
                    s_rec[slot][0] = ex;
                    s_rec[slot][1] = ey;
                    s_rec[slot][2] = eth;
#pragma unroll
                    for (int c = 0; c < 8; ++c) s_rec[slot][3 + c] = v[c];
                }
            } else {
                int cl, ch;
                disc_beam_range_from(norm, eth, dir, head, 0.5 * sqrt(blen * blen + bwid * bwid), a.scan_angles, B, a.angle_inc, cl, ch);
                s_cl[slot] = cl;
                s_ch[slot] = ch;
            }
        }
    }
    __syncthreads();
    int my_hit = 0;
    const bool agent_thread = t < AG && first + t < end;
    if (t < AG) {
        int lo = 0, cnt = 0;
        if (agent_thread) {
            const int i = first + t, me = i & 1;
            const int i0 = s_idx[t][0], i1 = s_idx[t][1], i2 = s_idx[t][2], i3 = s_idx[t][3];
            const int cl = s_cl[t], ch = s_ch[t];
            my_hit = s_hit[t >> 1];
            int ref_lo = i0 < i1 ? i0 : i1, t2 = i2 < i3 ? i2 : i3;
            ref_lo = ref_lo < t2 ? ref_lo : t2;
            int ref_hi = i0 > i1 ? i0 : i1;
            t2 = i2 > i3 ? i2 : i3;
            ref_hi = ref_hi > t2 ? ref_hi : t2;
            lo = ref_lo > cl ? ref_lo : cl;
            const int hi = ref_hi < ch ? ref_hi : ch;
            cnt = hi >= lo ? hi - lo + 1 : 0;
            const int wall = a.in_collision[i];
            if (wall) {
                a.state[3 * (size_t)N + i] = 0.;
                a.state[4 * (size_t)N + i] = 0.;
                a.state[5 * (size_t)N + i] = 0.;
                a.state[6 * (size_t)N + i] = 0.;
            }
            a.collisions[i] = (my_hit || wall) ? 1.0 : 0.0;
            a.collision_idx[i] = my_hit ? (double)(1 - me) : -1.0;
            a.step_count[i] += 1;
        }
        s_lo[t] = lo;
        s_cnt[t] = cnt;
    }
    __syncthreads();
    if (t < 64) {   // exclusive scan of the AG window lengths (AG <= 32: one wave)
        int c = t < AG ? s_cnt[t] : 0;
#pragma unroll
        for (int d = 1; d < AG; d <<= 1) {
            const int up = __shfl_up(c, d);
            if (t >= d) c += up;
        }
        if (t < AG) s_off[t + 1] = c;
        if (t == 0) s_off[0] = 0;
    }
    __syncthreads();
    const int total = s_off[AG];
    for (int item = t; item < total; item += NT) {
        int ag = 0;   // the largest ag with s_off[ag] <= item (its window is not empty: item < s_off[ag + 1])
#pragma unroll
        for (int st = AG / 2; st; st >>= 1)
            if (s_off[ag + st] <= item) ag += st;
        const int b = s_lo[ag] + (item - s_off[ag]);
        const double bex = s_rec[ag][0], bey = s_rec[ag][1], beth = s_rec[ag][2];
        double bv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) bv[c] = s_rec[ag][3 + c];
        double *sc = a.scans + (size_t)(first + ag) * B;
        const double bt = beth + a.scan_angles[b];
        const double r0 = sc[b];
        double v3x, v3y;
        sincos(bt + kPi / 2., &v3y, &v3x);
        const double r = box_range(bex, bey, v3x, v3y, bv, r0);
        if (r < r0) sc[b] = r;
    }
    if (HOST) {   // f110_step_host: the host block, the episode logic and its re-seat, right here (a.fused_host is set by the launcher)
        if (a.fused_host->hb.scans) {   // small batches: this workgroup's agents' scans, final once every item above is done
            __syncthreads();
            const int live_agents = (end - first) < AG ? (end - first) : AG;
            host_block_copy_scans(a.fused_host->hb, a.scans, (size_t)first, (size_t)(live_agents > 0 ? live_agents : 0));
        }
        if (t < 64) pair_host_epilogue(a, agent_thread, first + t);
    } else if (a.reseat_poses && agent_thread) {
        const int i = first + t, ego = (i & ~1) + a.reseat_ego;
        if (my_hit || a.in_collision[ego] != 0) reseat_agent(a, i, i == ego);
    }
}

// finalize_pair_body for ONE env of two agents that is the whole batch (k_step_tiny, N = 2): the same functions on the same operands,
// without the machinery for 32 agents per workgroup — the window lengths need no prefix scan (each half of the workgroup takes one
// agent's window), the agent's own columns are finished by the lane that runs its host epilogue (no barrier between the two), and the
// scans go into the host block EARLY: wave 1, which has no role, copies the 2 x B ranges while the role lanes do their trigonometry,
// and the beams the opponent shortens follow as they are found — instead of a 17 KB copy at the end of the chain.  (Storing them from
// the scan waves was tried first: their release then waits for the stores' acknowledgements over PCIe, +2.4 us where -2.6 were saved.)
// Three barriers instead of six on the step's critical path (profiles/r06_launch_latency.txt: the tail was 9.4 of the kernel's 32 us).
template <bool HOST>
__device__ __forceinline__ void finalize_duo_tiny(const AgentArrays &a, int32_t B, double *__restrict__ host_scans, const FusedHost &fh)
{
    __shared__ double d_rec[2][12];   // ex, ey, eth, the opponent's box (8), pad
    __shared__ int d_idx[2][4], d_cl[2], d_ch[2], d_hit;
    const int t = (int)threadIdx.x;
    constexpr int N = 2;
    int role = -1, slot = 0, sub = 0;
    if (t < 8) {                        // box corner `sub` of agent `slot`'s opponent -> beam index
        role = 0; slot = t >> 2; sub = t & 3;
    } else if (t >= 128 && t < 130) {   // wave 2: disc cull of agent `slot`
        role = 1; slot = t - 128;
    } else if (t == 192) {              // wave 3: the pair test
        role = 2;
    }
    if (HOST && host_scans && t >= 64 && t < 128) {
        const size_t n = (size_t)N * (size_t)B;
        size_t q = (size_t)(t - 64);
        for (; q + 192 < n; q += 256) {   // four independent loads in flight per lane, then the four stores
            const double v0 = a.scans[q], v1 = a.scans[q + 64], v2 = a.scans[q + 128], v3 = a.scans[q + 192];
            host_scans[q] = v0;
            host_scans[q + 64] = v1;
            host_scans[q + 128] = v2;
            host_scans[q + 192] = v3;
        }
        for (; q < n; q += 64) host_scans[q] = a.scans[q];
        __builtin_amdgcn_s_waitcnt(0);   // acknowledged before a window lane may store a shortened beam over one of them
    }
    if (role >= 0) {
        const int i = slot, me = i & 1, o = i ^ 1;
        const double ex = a.state[i], ey = a.state[(size_t)N + i];
        const double th_live = a.state[4 * (size_t)N + i];
        const double ox = a.snap_pose[o], oy = a.snap_pose[(size_t)N + o], oth = a.snap_pose[2 * (size_t)N + o];
        if (role == 2) {
            int hit = 0;
            const double reach = sqrt(a.box_length * a.box_length + a.box_width * a.box_width) + 1e-3;
            const double cdx = ox - ex, cdy = oy - ey;
            if (cdx * cdx + cdy * cdy <= reach * reach) {
                double mine[8], other[8];
                box_vertices(ex, ey, th_live, a.box_length, a.box_width, mine);
                box_vertices(ox, oy, oth, a.box_length, a.box_width, other);
                hit = gjk_overlap(mine, other) ? 1 : 0;
            }
            d_hit = hit;
        } else {
            const int wall = a.in_collision[i];
            const double eth = wall ? 0.0 : th_live;
            const size_t prow = (size_t)(a.params_per_agent ? i : me) * NPARAMS;
            const double blen = a.params[prow + P_LENGTH], bwid = a.params[prow + P_WIDTH];
            double v[8];
            box_vertices(ox, oy, oth, blen, bwid, v);
            double ce_, se_;
            cos_sin(eth, ce_, se_);
            const double head = atan2(se_, ce_);
            const double px = role == 1 ? ox : (sub == 0 ? v[0] : (sub == 1 ? v[2] : (sub == 2 ? v[4] : v[6])));
            const double py = role == 1 ? oy : (sub == 0 ? v[1] : (sub == 1 ? v[3] : (sub == 2 ? v[5] : v[7])));
            const double dx = px - ex, dy = py - ey;
            const double norm = sqrt(dx * dx + dy * dy);
            const double qx = role == 0 ? dx / norm : dx, qy = role == 0 ? dy / norm : dy;
            const double dir = atan2(qy, qx);
            if (role == 0) {
                d_idx[slot][sub] = vertex_beam_from_angles(head, dir, a.scan_angles, B, a.angle_inc);
                if (sub == 0) {
                    d_rec[slot][0] = ex;
                    d_rec[slot][1] = ey;
                    d_rec[slot][2] = eth;
#pragma unroll
                    for (int c = 0; c < 8; ++c) d_rec[slot][3 + c] = v[c];
                }
            } else {
                int cl, ch;
                disc_beam_range_from(norm, eth, dir, head, 0.5 * sqrt(blen * blen + bwid * bwid), a.scan_angles, B, a.angle_inc, cl, ch);
                d_cl[slot] = cl;
                d_ch[slot] = ch;
            }
        }
    }
    __syncthreads();
    // agent t's own columns, by lane t of wave 0 — the lane that runs its host epilogue below
    const bool agent_thread = t < N;
    const int my_hit = d_hit;
    if (agent_thread) {
        const int i = t, me = i & 1;
        const int wall = a.in_collision[i];
        if (wall) {
            a.state[3 * (size_t)N + i] = 0.;
            a.state[4 * (size_t)N + i] = 0.;
            a.state[5 * (size_t)N + i] = 0.;
            a.state[6 * (size_t)N + i] = 0.;
        }
        a.collisions[i] = (my_hit || wall) ? 1.0 : 0.0;
        a.collision_idx[i] = my_hit ? (double)(1 - me) : -1.0;
        a.step_count[i] += 1;
    }
    {   // agent `ag`'s opponent window, by its half of the workgroup
        const int ag = t >> 7, tt = t & 127;
        const int i0 = d_idx[ag][0], i1 = d_idx[ag][1], i2 = d_idx[ag][2], i3 = d_idx[ag][3];
        const int cl = d_cl[ag], ch = d_ch[ag];
        int ref_lo = i0 < i1 ? i0 : i1, t2 = i2 < i3 ? i2 : i3;
        ref_lo = ref_lo < t2 ? ref_lo : t2;
        int ref_hi = i0 > i1 ? i0 : i1;
        t2 = i2 > i3 ? i2 : i3;
        ref_hi = ref_hi > t2 ? ref_hi : t2;
        const int lo = ref_lo > cl ? ref_lo : cl;
        const int hi = ref_hi < ch ? ref_hi : ch;
        const int cnt = hi >= lo ? hi - lo + 1 : 0;
        const double bex = d_rec[ag][0], bey = d_rec[ag][1], beth = d_rec[ag][2];
        double bv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) bv[c] = d_rec[ag][3 + c];
        double *sc = a.scans + (size_t)ag * B;
        for (int item = tt; item < cnt; item += 128) {
            const int b = lo + item;
            const double bt = beth + a.scan_angles[b];
            const double r0 = sc[b];
            double v3x, v3y;
            sincos(bt + kPi / 2., &v3y, &v3x);
            const double r = box_range(bex, bey, v3x, v3y, bv, r0);
            if (r < r0) {
                sc[b] = r;
                if (HOST && host_scans) host_scans[(size_t)ag * B + b] = r;
            }
        }
    }
    if (HOST) {   // (fh: the epilogue's parameters as kernel arguments — a.fused_host holds the same in device memory, a load behind every barrier here)
        if (fh.hb.scans && !host_scans) {   // (not copied early: the copy, once every window is done)
            __syncthreads();
            host_block_copy_scans(fh.hb, a.scans, 0, (size_t)N);
        }
        if (t < 64) pair_host_epilogue_with(a, fh.ep, fh.hb, fh.episode, fh.auto_reset, agent_thread, t);
    } else if (a.reseat_poses && agent_thread) {
        const int i = t, ego = a.reseat_ego;
        if (my_hit || a.in_collision[ego] != 0) reseat_agent(a, i, i == ego);
    }
}

// HOST (round 6): the f110_step_host epilogue is a TEMPLATE parameter, not a run-time branch — the instantiation f110_step_device
// launches does not carry the epilogue's registers; the HOST instantiation (small, host-synchronised batches) runs at 4 waves per SIMD.
#ifndef F110_FIN_WAVES
#define F110_FIN_WAVES 5   // 5 waves per SIMD = up to 96 VGPRs: the body needs 82 and keeps nothing in scratch (at 6 = 80 VGPRs it kept 80 bytes per lane
                           // there for the epilogue it never ran; 35.9 us per launch at 65 536 agents at 4, 5 and 6 waves alike: profiles/r06_finalize_waves.txt)
#endif
template <int AG, bool HOST = false>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(HOST ? 4 : F110_FIN_WAVES))) k_finalize_pair_roles(AgentArrays a, int32_t B)
{
    finalize_pair_body<AG, HOST>(a, B, a.agent_begin + (int)blockIdx.x * AG, a.agent_begin + a.agent_count);
    if (HOST && a.fused_seq) {   // F110_STEP_SPIN_WAIT: the completion word, by the last workgroup to get here
        HostBlock sig = a.fused_host->hb;
        sig.seq = a.fused_seq;
        host_block_signal(sig);
    }
}

// ---- K3w: finalize_pair_body as ONE-WAVE workgroups, for a step that runs as two env blocks ---------------------------------------
// A 256-thread workgroup of the other block's finalize waits until this block's scan runs out of workgroups; a one-wave workgroup
// at 8 waves per SIMD fits the single slot a retiring scan wave frees, and its vector-ALU and latency work then runs under the scan's
// texture-bound march (DESIGN.md §4 "Env blocks").  Round 5's one-wave form dealt the three roles as divergent branches of the wave
// (+30 us alone).  Here the roles are MERGED: the 4 AG corner lanes and the AG cull lanes share one pass through the prologue — loads,
// the opponent's box, cos_sin, both atan2, the square root — the point under a lane select, and part only at the last call
// (vertex_beam_from_angles / disc_beam_range_from).  The pair test of env (slot, slot + 1) sits on the cull lane of its even agent,
// behind a wave-uniform skip: cars within reach of each other are rare, and the wave that holds such a pair pays a second pass.
// AG = 12: 48 + 12 = 60 lanes of the wave in the prologue, and window items (about half the agents see the opponent, up to ~31 beams)
// that mostly fill their passes of 64.  Same functions on the same operands as finalize_pair_body: bit-identical.  No HOST form: a
// host-synchronised step never runs as two blocks.
template <int AG>
__device__ __forceinline__ void finalize_pair_wave_body(const AgentArrays &a, int32_t B, const int first, const int end)
{
    constexpr int NT = 64;
    constexpr int AGP = AG <= 2 ? 2 : (AG <= 4 ? 4 : (AG <= 8 ? 8 : 16));   // the prefix scan and the item search run over a power of two
    static_assert(AG >= 2 && (AG & 1) == 0 && 5 * AG <= NT && AG <= AGP, "whole envs, and 4 AG corner + AG cull lanes fit the wave");
    constexpr int R1 = 4 * AG;   // first lane of the cull role
    // 64 VGPRs: GJK and box_range read a box's coordinates from LDS where they use them (volatile: not held in registers throughout)
    typedef const volatile __attribute__((address_space(3))) double *LdsBox;
    __shared__ double s_rec[AG][12];   // ex, ey, eth, the opponent's box (8), pad
    __shared__ int s_idx[AG][4], s_cl[AG], s_ch[AG], s_hit[AG / 2];
    __shared__ int s_lo[AG], s_cnt[AG], s_off[AGP + 1];
    __shared__ double s_box[AG / 2][16];   // the pair test's two boxes
    __shared__ int s_ab[NT][2];            // the item loop: each lane's (agent, beam) across its sincos
    const int t = (int)threadIdx.x;
    const int N = a.n_agents_total;
    const int role = t < R1 ? 0 : (t < R1 + AG ? 1 : -1);
    const int slot = role == 0 ? t >> 2 : t - R1, sub = t & 3;
    bool near = false;   // cull lane of an even agent whose opponent's centre is within reach: the pair test below
    if (role >= 0 && first + slot < end) {
        const int i = first + slot, me = i & 1, o = i ^ 1;
        const double ex = a.state[i], ey = a.state[(size_t)N + i];
        const double th_live = a.state[4 * (size_t)N + i];   // == the :574 snapshot heading: nothing has zeroed it yet
        const double ox = a.snap_pose[o], oy = a.snap_pose[(size_t)N + o], oth = a.snap_pose[2 * (size_t)N + o];
        const int wall = a.in_collision[i];
        const double eth = wall ? 0.0 : th_live;
        const size_t prow = (size_t)(a.params_per_agent ? i : me) * NPARAMS;
        const double blen = a.params[prow + P_LENGTH], bwid = a.params[prow + P_WIDTH];
        double v[8];   // the opponent drawn with MY length / width (RaceCar.ray_cast_agents :223)
        box_vertices(ox, oy, oth, blen, bwid, v);
        double ce_, se_;
        cos_sin(eth, ce_, se_);
        const double head = atan2(se_, ce_);
        const double px = role == 1 ? ox : (sub == 0 ? v[0] : (sub == 1 ? v[2] : (sub == 2 ? v[4] : v[6])));
        const double py = role == 1 ? oy : (sub == 0 ? v[1] : (sub == 1 ? v[3] : (sub == 2 ? v[5] : v[7])));
        const double dx = px - ex, dy = py - ey;
        const double d2 = dx * dx + dy * dy;   // (cull lanes: the centre distance the pair test's reach check takes)
        const double norm = sqrt(d2);
        const double qx = role == 0 ? dx / norm : dx, qy = role == 0 ? dy / norm : dy;
        const double dir = atan2(qy, qx);
        if (role == 0) {
            s_idx[slot][sub] = vertex_beam_from_angles(head, dir, a.scan_angles, B, a.angle_inc);
            if (sub == 0) {
                s_rec[slot][0] = ex;
                s_rec[slot][1] = ey;
                s_rec[slot][2] = eth;
#pragma unroll
                for (int c = 0; c < 8; ++c) s_rec[slot][3 + c] = v[c];
            }
        } else {
            int cl, ch;
            disc_beam_range_from(norm, eth, dir, head, 0.5 * sqrt(blen * blen + bwid * bwid), a.scan_angles, B, a.angle_inc, cl, ch);
            s_cl[slot] = cl;
            s_ch[slot] = ch;
            const double reach = sqrt(a.box_length * a.box_length + a.box_width * a.box_width) + 1e-3;
            near = me == 0 && d2 <= reach * reach;
        }
    }
    int hit = 0;
    if (__ballot(near) != 0) {   // wave-uniform: almost never taken
        if (near) {
            // collision_multiple on the env's one pair, boxes with the Simulator's length / width (:549); i is the
            // even agent: gjk_overlap(mine, other) here is gjk_overlap(other, mine) of the odd agent's call
            const int i = first + slot, o = i ^ 1;   // (loaded again: nothing is kept live across the prologue for the rare case)
            double *mine = s_box[slot >> 1], *other = mine + 8;
            box_vertices(a.state[i], a.state[(size_t)N + i], a.state[4 * (size_t)N + i], a.box_length, a.box_width, mine);
            box_vertices(a.snap_pose[o], a.snap_pose[(size_t)N + o], a.snap_pose[2 * (size_t)N + o], a.box_length, a.box_width, other);
            hit = gjk_overlap_from<LdsBox>((LdsBox)mine, (LdsBox)other) ? 1 : 0;
        }
    }
    if (role == 1 && (slot & 1) == 0) s_hit[slot >> 1] = hit;
    __syncthreads();
    if (t < AG) {
        int lo = 0, cnt = 0;
        if (first + t < end) {
            const int i = first + t, me = i & 1;
            const int i0 = s_idx[t][0], i1 = s_idx[t][1], i2 = s_idx[t][2], i3 = s_idx[t][3];
            const int cl = s_cl[t], ch = s_ch[t];
            const int my_hit = s_hit[t >> 1];
            int ref_lo = i0 < i1 ? i0 : i1, t2 = i2 < i3 ? i2 : i3;
            ref_lo = ref_lo < t2 ? ref_lo : t2;
            int ref_hi = i0 > i1 ? i0 : i1;
            t2 = i2 > i3 ? i2 : i3;
            ref_hi = ref_hi > t2 ? ref_hi : t2;
            lo = ref_lo > cl ? ref_lo : cl;
            const int hi = ref_hi < ch ? ref_hi : ch;
            cnt = hi >= lo ? hi - lo + 1 : 0;
            const int wall = a.in_collision[i];
            if (wall) {
                a.state[3 * (size_t)N + i] = 0.;
                a.state[4 * (size_t)N + i] = 0.;
                a.state[5 * (size_t)N + i] = 0.;
                a.state[6 * (size_t)N + i] = 0.;
            }
            a.collisions[i] = (my_hit || wall) ? 1.0 : 0.0;
            a.collision_idx[i] = my_hit ? (double)(1 - me) : -1.0;
            a.step_count[i] += 1;
        }
        s_lo[t] = lo;
        s_cnt[t] = cnt;
    }
    __syncthreads();
    {   // exclusive scan of the AG window lengths, padded to AGP (the entries past AG repeat the total: the search never lands there)
        int c = t < AG ? s_cnt[t] : 0;
#pragma unroll
        for (int d = 1; d < AGP; d <<= 1) {
            const int up = __shfl_up(c, d);
            if (t >= d) c += up;
        }
        if (t < AGP) s_off[t + 1] = c;
        if (t == 0) s_off[0] = 0;
    }
    __syncthreads();
    for (int item = t; item < s_off[AG]; item += NT) {   // (the total is read again every pass, not kept in a register)
        int ag = 0;   // the largest ag with s_off[ag] <= item (its window is not empty: item < s_off[ag + 1])
#pragma unroll
        for (int st = AGP / 2; st; st >>= 1)
            if (s_off[ag + st] <= item) ag += st;
        int b = s_lo[ag] + (item - s_off[ag]);
        const double bt = s_rec[ag][2] + a.scan_angles[b];
        // 64 VGPRs: nothing but the angle is held in registers across the sincos — the item's agent and beam wait in LDS, the
        // record's other ten doubles and the beam's address are read / formed behind it
        s_ab[item & (NT - 1)][0] = ag;
        s_ab[item & (NT - 1)][1] = b;
        double v3x, v3y;
        sincos(bt + kPi / 2., &v3y, &v3x);
        __asm__ volatile("" ::: "memory");
        ag = s_ab[item & (NT - 1)][0];
        b = s_ab[item & (NT - 1)][1];
        double *sc = a.scans + (size_t)(first + ag) * B;
        const double r0 = sc[b];
        const double r = box_range_from<LdsBox>(s_rec[ag][0], s_rec[ag][1], v3x, v3y, (LdsBox)&s_rec[ag][3], r0);   // (each edge's corners from LDS where the edge needs them)
        if (r < r0) sc[b] = r;
    }
    const int te = (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));   // == t: one wave (formed again, not kept across the item loop)
    if (a.reseat_poses && te < AG && first + te < end) {
        const int i = first + te, ego = (i & ~1) + a.reseat_ego;
        if (s_hit[te >> 1] || a.in_collision[ego] != 0) reseat_agent(a, i, i == ego);
    }
}

constexpr int kFinalizeWaveAgents = 12;   // agents per one-wave workgroup (the launcher's grid follows it)
template <int AG>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8))) k_finalize_pair_wave(AgentArrays a, int32_t B)   // 8 waves per SIMD = 64 VGPRs
{
    finalize_pair_wave_body<AG>(a, B, a.agent_begin + (int)blockIdx.x * AG, a.agent_begin + a.agent_count);
}

// ---- K3m: the same for envs of MORE than two agents (round 3) ---------------------------------------------
// k_finalize_pair_roles generalised: a workgroup holds G whole envs of A agents.  What k_collide + k_finalize did
// with one lane per agent (a serial loop over the A - 1 opponents: box, GJK, two beam windows, 80 bytes of windows
// and boxes through HBM per ordered pair, a side stream with an event fork / join around the scan) becomes one
// kernel behind the scan:
//   agents    (round 4) what a record needs of its two agents, once per agent into LDS (MultiAgentLds);
//   records   every ORDERED pair (agent i, opponent o) of the workgroup's envs, R = G A (A - 1) <= MAXREC (64 for A <= 8,
//             256 with one env per workgroup for A <= 16): the four
//             corners of o's box (drawn with i's length / width, RaceCar.ray_cast_agents :223) -> beam indices on
//             threads 0-191 (four per record), the disc cull on threads 192-255 (one per record);
//   pairs     every UNORDERED pair (p < q) of an env, P = G A (A - 1) / 2: collision_multiple's GJK in the reference's
//             (lower, higher) argument order on threads 192-255 behind the culls — once, not once per side;
//   agents    flags (Simulator's collision OR :588-589; collision_idx = the LARGEST colliding partner, the reference's
//             last writer), check_ttc's side effects, step count, re-seat: thread a of the first G A;
//   windows   all records' beam windows flattened into one item list over the 256 threads, as in the pair kernel.  Two
//             opponents of one agent may cover the same beam; the reference takes them one after the other, each
//             keeping the smaller range (:206-227), i.e. the minimum — ranges are non-negative doubles, whose bit
//             patterns order like unsigned integers, so the items settle it with atomicMin on the pattern: no rounds,
//             no order, the same value.
// Same functions on the same operands as collide_agent / k_finalize: bit-identical (test_finalize_multi_*).
constexpr int kMaxRec = 64;      // A <= 8: a workgroup's record table
constexpr int kMaxRecBig = 256;  // 9 <= A <= 16: one env per workgroup, up to 240 records
// phase 1 of k_finalize_multi: 4 R corner tasks (an atan2, a square root, two divisions each) on the first three waves, R disc
// culls and then R / 2 pair tests on the fourth (round 4; round 3: corners on two waves, 7.5 rounds of them at 16 cars).
// What a task needs of its two AGENTS — ray-cast heading, atan2(sin, cos) of it, cos / sin of the opponent's snapshot
// heading — is computed once per agent in a phase of its own (MultiAgentLds), not 4 (A - 1) times (doubling probes at 16
// cars, round 4: corners 77 us, culls 17, pair tests 5, window items 135 of the kernel's 250).
constexpr int kMultiCornerThreads = 192;
struct MultiAgentLds {   // one per agent of the workgroup
    double ex, ey, eth, head;      // live position, ray-cast heading, atan2(sin(eth), cos(eth))
    double ox, oy, co, so;         // :574 snapshot position, cos / sin of the snapshot heading
    double blen, bwid, rad;        // the box this agent draws around its opponents (RaceCar.ray_cast_agents :223: its OWN length / width), half its diagonal
};
template <int MAXREC>
__global__ void __launch_bounds__(256) k_finalize_multi(AgentArrays a, int32_t B, int G)
{
    static_assert(MAXREC == 64 || MAXREC == 256, "record table sizes");
    __shared__ double s_rec[MAXREC][12];   // ex, ey, eth, the opponent's box (8), pad
    __shared__ int s_idx[MAXREC][4], s_cl[MAXREC], s_ch[MAXREC], s_hit[MAXREC];
    __shared__ int s_lo[MAXREC], s_off[MAXREC + 1], s_agent[MAXREC], s_ahit[MAXREC], s_wsum[4];
    constexpr int MAXAG = MAXREC == 64 ? 32 : 16;   // agents per workgroup: G A (A - 1) <= 64 -> G A <= 32; the 256-record table takes ONE env of <= 16
    __shared__ MultiAgentLds s_ag[MAXAG];
    const int t = (int)threadIdx.x;
    const int A = a.agents_per_env, N = a.n_agents_total;
    const int per_env = A * (A - 1), pairs_env = per_env / 2;
    const int first = a.agent_begin + (int)blockIdx.x * G * A, end = a.agent_begin + a.agent_count;
    int envs = (end - first) / A;
    envs = envs < G ? envs : G;                 // (whole envs only: ranges are env-aligned)
    const int R = envs * per_env, P = envs * pairs_env, AGN = envs * A;
    if (t < AGN) {   // everything that is per agent, once
        const int i = first + t;
        MultiAgentLds m;
        m.ex = a.state[i];
        m.ey = a.state[(size_t)N + i];
        const double th_live = a.state[4 * (size_t)N + i];   // == the :574 snapshot heading: nothing has zeroed it yet
        m.eth = a.in_collision[i] ? 0.0 : th_live;
        double ce_, se_;
        cos_sin(m.eth, ce_, se_);
        m.head = atan2(se_, ce_);
        m.ox = a.snap_pose[i];
        m.oy = a.snap_pose[(size_t)N + i];
        cos_sin(a.snap_pose[2 * (size_t)N + i], m.co, m.so);
        const size_t prow = (size_t)(a.params_per_agent ? i : t % A) * NPARAMS;
        m.blen = a.params[prow + P_LENGTH];
        m.bwid = a.params[prow + P_WIDTH];
        m.rad = 0.5 * sqrt(m.blen * m.blen + m.bwid * m.bwid);
        s_ag[t] = m;
    }
    __syncthreads();
    if (t < kMultiCornerThreads) {
        // corner `sub` of record `rec`'s opponent box -> beam index
        for (int q = t; q < 4 * R; q += kMultiCornerThreads) {
            const int rec = q >> 2, sub = q & 3;
            const int e = rec / per_env, w = rec - e * per_env, me = w / (A - 1), k = w - me * (A - 1), oj = k < me ? k : k + 1;
            const MultiAgentLds &mm = s_ag[e * A + me], &mo = s_ag[e * A + oj];
            const double ex = mm.ex, ey = mm.ey, eth = mm.eth, head = mm.head;
            double v[8];
            box_vertices_cs(mo.ox, mo.oy, mo.co, mo.so, mm.blen, mm.bwid, v);
            const double px = sub == 0 ? v[0] : (sub == 1 ? v[2] : (sub == 2 ? v[4] : v[6]));
            const double py = sub == 0 ? v[1] : (sub == 1 ? v[3] : (sub == 2 ? v[5] : v[7]));
            const double dx = px - ex, dy = py - ey;
            const double norm = sqrt(dx * dx + dy * dy);
            const double dir = atan2(dy / norm, dx / norm);
            s_idx[rec][sub] = vertex_beam_from_angles(head, dir, a.scan_angles, B, a.angle_inc);
            if (sub == 0) {
                s_rec[rec][0] = ex;
                s_rec[rec][1] = ey;
                s_rec[rec][2] = eth;
#pragma unroll
                for (int c = 0; c < 8; ++c) s_rec[rec][3 + c] = v[c];
                s_agent[rec] = e * A + me;
            }
        }
    } else {
        // the disc cull of record `rec`
        for (int rec = t - kMultiCornerThreads; rec < R; rec += 256 - kMultiCornerThreads) {
            const int e = rec / per_env, w = rec - e * per_env, me = w / (A - 1), k = w - me * (A - 1), oj = k < me ? k : k + 1;
            const MultiAgentLds &mm = s_ag[e * A + me], &mo = s_ag[e * A + oj];
            const double eth = mm.eth, head = mm.head;
            const double dx = mo.ox - mm.ex, dy = mo.oy - mm.ey;
            const double norm = sqrt(dx * dx + dy * dy);
            const double dir = atan2(dy, dx);
            int cl, ch;
            disc_beam_range_from(norm, eth, dir, head, mm.rad, a.scan_angles, B, a.angle_inc, cl, ch);
            s_cl[rec] = cl;
            s_ch[rec] = ch;
        }
        // collision_multiple's pair (p < q) of env e, boxes with the Simulator's length / width (:549)
        const double reach = sqrt(a.box_length * a.box_length + a.box_width * a.box_width) + 1e-3;
        for (int pr = t - kMultiCornerThreads; pr < P; pr += 256 - kMultiCornerThreads) {
            const int e = pr / pairs_env;
            int w = pr - e * pairs_env, p = 0;
            while (w >= A - 1 - p) { w -= A - 1 - p; ++p; }   // row p of the upper triangle holds A - 1 - p pairs
            const int q = p + 1 + w;
            const MultiAgentLds &mp = s_ag[e * A + p], &mq = s_ag[e * A + q];
            int hit = 0;
            const double cdx = mq.ox - mp.ox, cdy = mq.oy - mp.oy;
            if (cdx * cdx + cdy * cdy <= reach * reach) {
                double lower[8], higher[8];
                box_vertices_cs(mp.ox, mp.oy, mp.co, mp.so, a.box_length, a.box_width, lower);
                box_vertices_cs(mq.ox, mq.oy, mq.co, mq.so, a.box_length, a.box_width, higher);
                hit = gjk_overlap(lower, higher) ? 1 : 0;
            }
            s_hit[pr] = hit;
        }
    }
    __syncthreads();
    int my_hit = 0;
    const bool agent_thread = t < AGN;
    if (agent_thread) {
        const int e = t / A, me = t - e * A, i = first + t;
        int partner = -1;
        for (int j = 0; j < A; ++j) {   // ascending: ends at the largest colliding index
            if (j == me) continue;
            const int p = me < j ? me : j, q = me < j ? j : me;
            const int pr = e * pairs_env + p * (A - 1) - (p * (p - 1)) / 2 + (q - p - 1);   // rows 0..p-1 hold p (A - 1) - p (p - 1) / 2 pairs
            if (s_hit[pr]) partner = j;
        }
        my_hit = partner >= 0;
        const int wall = a.in_collision[i];
        if (wall) {
            a.state[3 * (size_t)N + i] = 0.;
            a.state[4 * (size_t)N + i] = 0.;
            a.state[5 * (size_t)N + i] = 0.;
            a.state[6 * (size_t)N + i] = 0.;
        }
        a.collisions[i] = (my_hit || wall) ? 1.0 : 0.0;
        a.collision_idx[i] = (double)partner;
        a.step_count[i] += 1;
        s_ahit[t] = my_hit;
    }
    const int wrec = MAXREC == 64 ? t - 64 : t;   // 64 records: wave 1 (beside the agents' wave); 256: every thread one record
    if (wrec >= 0 && wrec < MAXREC) {   // every record's window = corner hull clipped by the disc cull
        const int rec = wrec;
        int lo = 0, cnt = 0;
        if (rec < R) {
            const int i0 = s_idx[rec][0], i1 = s_idx[rec][1], i2 = s_idx[rec][2], i3 = s_idx[rec][3];
            int ref_lo = i0 < i1 ? i0 : i1, t2 = i2 < i3 ? i2 : i3;
            ref_lo = ref_lo < t2 ? ref_lo : t2;
            int ref_hi = i0 > i1 ? i0 : i1;
            t2 = i2 > i3 ? i2 : i3;
            ref_hi = ref_hi > t2 ? ref_hi : t2;
            const int cl = s_cl[rec], ch = s_ch[rec];
            lo = ref_lo > cl ? ref_lo : cl;
            const int hi = ref_hi < ch ? ref_hi : ch;
            cnt = hi >= lo ? hi - lo + 1 : 0;
        }
        s_lo[rec] = lo;
        int c = cnt;   // inclusive scan over the wave's 64 records
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(c, d);
            if ((rec & 63) >= d) c += up;
        }
        s_off[rec + 1] = c;
        if (rec == 0) s_off[0] = 0;
        if (MAXREC > 64 && (rec & 63) == 63) s_wsum[rec >> 6] = c;
    }
    __syncthreads();
    if (MAXREC > 64) {   // the later waves' records start behind the earlier waves' totals
        if (t >= 64 && t < MAXREC) {
            int base = 0;
            for (int w = 0; w < (t >> 6); ++w) base += s_wsum[w];
            s_off[t + 1] += base;
        }
        __syncthreads();
    }
    const int total = s_off[MAXREC];
    for (int item = t; item < total; item += 256) {
        int rec = 0;   // the largest rec with s_off[rec] <= item (its window is not empty: item < s_off[rec + 1])
#pragma unroll
        for (int st = MAXREC / 2; st; st >>= 1)
            if (s_off[rec + st] <= item) rec += st;
        const int b = s_lo[rec] + (item - s_off[rec]);
        const double bex = s_rec[rec][0], bey = s_rec[rec][1], beth = s_rec[rec][2];
        double bv[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) bv[c] = s_rec[rec][3 + c];
        double *sc = a.scans + (size_t)(first + s_agent[rec]) * B;
        const double bt = beth + a.scan_angles[b];
        const double r0 = sc[b];   // (possibly already lowered by another opponent's item: the minimum does not care)
        double v3x, v3y;
        sincos(bt + kPi / 2., &v3y, &v3x);
        const double r = box_range(bex, bey, v3x, v3y, bv, r0);
        if (r < r0) atomicMin(reinterpret_cast<unsigned long long *>(sc + b), (unsigned long long)__double_as_longlong(r));
    }
    if (a.reseat_poses && agent_thread) {
        const int e = t / A, i = first + t, ego_t = e * A + a.reseat_ego, ego = first + ego_t;
        if (s_ahit[ego_t] || a.in_collision[ego] != 0) reseat_agent(a, i, i == ego);
    }
}

// ---- K3t: envs of MORE than sixteen agents (round 4) — k_finalize_multi with the env's ordered pairs in TILES -------
// k_finalize_multi for any number of agents per env (17 ... 256; it also runs 3 ... 16, where k_finalize_multi's role-parallel
// form is faster: A = 8 75.7 against 79.3 M agent-steps/s, 16: equal): a workgroup holds G whole envs of A agents.  What k_collide + k_finalize did with one lane per agent (a serial loop over the A - 1 opponents: box, GJK, two
// beam windows, 80 bytes of windows and boxes through HBM per ordered pair, a side stream with an event fork / join
// around the scan) is one kernel behind the scan:
//   agents    once per agent, into LDS: the live pose and the heading the ray cast uses (0 after a wall hit, :246-249),
//             head = atan2(sin, cos) of it (get_blocked_view_indices :296-297), and cos / sin of the agent's :574
//             snapshot heading (what every box drawn around it needs) — per AGENT, not per ordered pair (round 4: the
//             record threads of round 3 recomputed them 4 (A - 1) times);
//   pairs     every UNORDERED pair (p < q) of an env: collision_multiple's GJK in the reference's (lower, higher)
//             argument order behind a conservative reject (centres further apart than the boxes' diagonal: the
//             prune north_star asks for; SURVEY a15: flag-preserving) — the largest colliding partner per agent by
//             atomicMax (collision_multiple's last writer, :199-210);
//   records   every ORDERED pair (agent i, opponent o), in tiles of at most MAXREC: first the disc cull (beams whose
//             ray can touch the disc around o's box), then — only for records the cull leaves a window — the four
//             corners of o's box (drawn with i's length / width, RaceCar.ray_cast_agents :223) -> beam indices, four
//             threads per record;
//   windows   a tile's beam windows flattened into one item list over the 256 threads.  An item whose map range is
//             already shorter than the distance to the nearest point of o's disc is finished (every edge distance is
//             at least that far: the minimum keeps the map range).  Two opponents of one agent may cover the same
//             beam; the reference takes them one after the other, each keeping the smaller range (:206-227), i.e. the
//             minimum — ranges are non-negative doubles, whose bit patterns order like unsigned integers, so the items
//             settle it with atomicMin on the pattern: no rounds, no order, the same value — also across tiles.
//   flags     Simulator's collision OR (:588-589), check_ttc's side effects, step count, re-seat: one thread per agent.
// Same functions on the same operands as collide_agent / k_finalize: bit-identical (test_finalize_multi_*,
// tests/golden/sim_rollout_multi.npz = the reference itself at A = 3, 4, 8).
constexpr int kMaxAgentsMulti = 256;   // agents per env this kernel takes (its per-agent LDS table)
// (MultiAgentLds: above, shared with k_finalize_multi)
// dynamic LDS of k_finalize_multi for `agents` agents per workgroup (host and device agree through this one function):
// the agent table, a tile's boxes / near distances, a tile's int tables, the scan offsets, the partners
__host__ __device__ inline size_t multi_lds_bytes(int agents, int maxrec)
{
    return sizeof(MultiAgentLds) * (size_t)agents + (size_t)maxrec * 9 * sizeof(double) + sizeof(int) * ((size_t)maxrec * 8 + (size_t)maxrec + 1 + 4 + (size_t)agents) + 16;
}

template <int MAXREC>
__global__ void __launch_bounds__(256) k_finalize_multi_tiled(AgentArrays a, int32_t B, int G)
{
    static_assert(MAXREC == 64 || MAXREC == 256, "record tile sizes");
    extern __shared__ __align__(16) unsigned char s_raw[];
    const int t = (int)threadIdx.x;
    const int A = a.agents_per_env, N = a.n_agents_total;
    const int per_env = A * (A - 1), pairs_env = per_env / 2;
    const int first = a.agent_begin + (int)blockIdx.x * G * A, end = a.agent_begin + a.agent_count;
    int envs = (end - first) / A;
    envs = envs < G ? envs : G;                 // (whole envs only: ranges are env-aligned)
    const int R = envs * per_env, P = envs * pairs_env, AGN = envs * A;
    // LDS carve-up (dynamic: sized by the launch for G * A agents, multi_lds_bytes)
    MultiAgentLds *s_ag = reinterpret_cast<MultiAgentLds *>(s_raw);
    double (*s_box)[8] = reinterpret_cast<double (*)[8]>(s_ag + G * A);   // a record's opponent box
    double *s_near = reinterpret_cast<double *>(s_box + MAXREC);          // a map range below this cannot be lowered by the record
    int (*s_idx)[4] = reinterpret_cast<int (*)[4]>(s_near + MAXREC);
    int *s_cl = reinterpret_cast<int *>(s_idx + MAXREC), *s_ch = s_cl + MAXREC, *s_lo = s_ch + MAXREC, *s_agent = s_lo + MAXREC;
    int *s_off = s_agent + MAXREC;      // [MAXREC + 1]
    int *s_wsum = s_off + MAXREC + 1;   // [4]
    int *s_partner = s_wsum + 4;        // [G * A] largest colliding partner (slot index) or -1

    // ---- agents: everything that is per agent, once
    for (int ag = t; ag < AGN; ag += 256) {
        const int i = first + ag;
        MultiAgentLds m;
        m.ex = a.state[i];
        m.ey = a.state[(size_t)N + i];
        const double th_live = a.state[4 * (size_t)N + i];   // == the :574 snapshot heading: nothing has zeroed it yet
        m.eth = a.in_collision[i] ? 0.0 : th_live;
        double ce_, se_;
        cos_sin(m.eth, ce_, se_);
        m.head = atan2(se_, ce_);
        m.ox = a.snap_pose[i];
        m.oy = a.snap_pose[(size_t)N + i];
        cos_sin(a.snap_pose[2 * (size_t)N + i], m.co, m.so);
        const size_t prow = (size_t)(a.params_per_agent ? i : ag % A) * NPARAMS;
        m.blen = a.params[prow + P_LENGTH];
        m.bwid = a.params[prow + P_WIDTH];
        m.rad = 0.5 * sqrt(m.blen * m.blen + m.bwid * m.bwid);
        s_ag[ag] = m;
        s_partner[ag] = -1;
    }
    __syncthreads();

    // ---- pairs: collision_multiple's pair (p < q) of the env, boxes with the Simulator's length / width (:549)
    {
        const double reach = sqrt(a.box_length * a.box_length + a.box_width * a.box_width) + 1e-3;
        for (int pr = t; pr < P; pr += 256) {
            const int e = pr / pairs_env;
            int w = pr - e * pairs_env, p = 0;
            while (w >= A - 1 - p) { w -= A - 1 - p; ++p; }   // row p of the upper triangle holds A - 1 - p pairs
            const int q = p + 1 + w;
            const MultiAgentLds &mp = s_ag[e * A + p], &mq = s_ag[e * A + q];
            const double cdx = mq.ox - mp.ox, cdy = mq.oy - mp.oy;
            if (cdx * cdx + cdy * cdy <= reach * reach) {
                double lower[8], higher[8];
                box_vertices_cs(mp.ox, mp.oy, mp.co, mp.so, a.box_length, a.box_width, lower);
                box_vertices_cs(mq.ox, mq.oy, mq.co, mq.so, a.box_length, a.box_width, higher);
                if (gjk_overlap(lower, higher)) {
                    atomicMax(&s_partner[e * A + p], q);
                    atomicMax(&s_partner[e * A + q], p);
                }
            }
        }
    }

    // ---- records, tile by tile
    for (int tile = 0; tile < R; tile += MAXREC) {
        const int RT = (R - tile) < MAXREC ? (R - tile) : MAXREC;   // records of this tile
        // the disc cull of record `rec` (and who it is)
        for (int rec = t; rec < RT; rec += 256) {
            const int gr = tile + rec;
            const int e = gr / per_env, w = gr - e * per_env, me = w / (A - 1), k = w - me * (A - 1), oj = k < me ? k : k + 1;
            const int ia = e * A + me;
            const MultiAgentLds &mm = s_ag[ia], &mo = s_ag[e * A + oj];
            const double blen = mm.blen, bwid = mm.bwid, rad = mm.rad;
            const double dx = mo.ox - mm.ex, dy = mo.oy - mm.ey;
            const double norm = sqrt(dx * dx + dy * dy);
            const double dir = atan2(dy, dx);
            int cl, ch;
            disc_beam_range_from(norm, mm.eth, dir, mm.head, rad, a.scan_angles, B, a.angle_inc, cl, ch);
            s_cl[rec] = cl;
            s_ch[rec] = ch;
            s_agent[rec] = ia;
            s_near[rec] = norm - rad * 1.000001 - 1e-9;   // no point of the box is nearer than this
            if (cl <= ch) box_vertices_cs(mo.ox, mo.oy, mo.co, mo.so, blen, bwid, s_box[rec]);
        }
        __syncthreads();
        // corner `sub` of record `rec`'s opponent box -> beam index (records with an empty cull are skipped)
        for (int q = t; q < 4 * RT; q += 256) {
            const int rec = q >> 2, sub = q & 3;
            if (s_cl[rec] > s_ch[rec]) continue;
            const MultiAgentLds &mm = s_ag[s_agent[rec]];
            const double px = s_box[rec][2 * sub], py = s_box[rec][2 * sub + 1];
            const double dx = px - mm.ex, dy = py - mm.ey;
            const double norm = sqrt(dx * dx + dy * dy);
            const double dir = atan2(dy / norm, dx / norm);
            s_idx[rec][sub] = vertex_beam_from_angles(mm.head, dir, a.scan_angles, B, a.angle_inc);
        }
        __syncthreads();
        if (t < MAXREC) {   // every record's window = corner hull clipped by the disc cull
            const int rec = t;
            int lo = 0, cnt = 0;
            if (rec < RT && s_cl[rec] <= s_ch[rec]) {
                const int i0 = s_idx[rec][0], i1 = s_idx[rec][1], i2 = s_idx[rec][2], i3 = s_idx[rec][3];
                int ref_lo = i0 < i1 ? i0 : i1, t2 = i2 < i3 ? i2 : i3;
                ref_lo = ref_lo < t2 ? ref_lo : t2;
                int ref_hi = i0 > i1 ? i0 : i1;
                t2 = i2 > i3 ? i2 : i3;
                ref_hi = ref_hi > t2 ? ref_hi : t2;
                const int cl = s_cl[rec], ch = s_ch[rec];
                lo = ref_lo > cl ? ref_lo : cl;
                const int hi = ref_hi < ch ? ref_hi : ch;
                cnt = hi >= lo ? hi - lo + 1 : 0;
            }
            s_lo[rec] = lo;
            int c = cnt;   // inclusive scan over the wave's 64 records
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int up = __shfl_up(c, d);
                if ((rec & 63) >= d) c += up;
            }
            s_off[rec + 1] = c;
            if (rec == 0) s_off[0] = 0;
            if (MAXREC > 64 && (rec & 63) == 63) s_wsum[rec >> 6] = c;
        }
        __syncthreads();
        if (MAXREC > 64) {   // the later waves' records start behind the earlier waves' totals
            if (t >= 64 && t < MAXREC) {
                int base = 0;
                for (int w = 0; w < (t >> 6); ++w) base += s_wsum[w];
                s_off[t + 1] += base;
            }
            __syncthreads();
        }
        const int total = s_off[MAXREC];
        for (int item = t; item < total; item += 256) {
            int rec = 0;   // the largest rec with s_off[rec] <= item (its window is not empty: item < s_off[rec + 1])
#pragma unroll
            for (int st = MAXREC / 2; st; st >>= 1)
                if (s_off[rec + st] <= item) rec += st;
            const int b = s_lo[rec] + (item - s_off[rec]);
            const int ia = s_agent[rec];
            double *sc = a.scans + (size_t)(first + ia) * B;
            const double r0 = sc[b];   // (possibly already lowered by another opponent's item: the minimum does not care)
            if (r0 < s_near[rec]) continue;   // the wall is nearer than any point of this opponent
            const MultiAgentLds &mm = s_ag[ia];
            double bv[8];
#pragma unroll
            for (int c = 0; c < 8; ++c) bv[c] = s_box[rec][c];
            const double bt = mm.eth + a.scan_angles[b];
            double v3x, v3y;
            sincos(bt + kPi / 2., &v3y, &v3x);
            const double r = box_range(mm.ex, mm.ey, v3x, v3y, bv, r0);
            if (r < r0) atomicMin(reinterpret_cast<unsigned long long *>(sc + b), (unsigned long long)__double_as_longlong(r));
        }
        __syncthreads();   // the next tile overwrites the record tables
    }

    // ---- flags, check_ttc's side effects, step count, re-seat
    __syncthreads();
    for (int ag = t; ag < AGN; ag += 256) {
        const int i = first + ag;
        const int partner = s_partner[ag];
        const int wall = a.in_collision[i];
        if (wall) {
            a.state[3 * (size_t)N + i] = 0.;
            a.state[4 * (size_t)N + i] = 0.;
            a.state[5 * (size_t)N + i] = 0.;
            a.state[6 * (size_t)N + i] = 0.;
        }
        a.collisions[i] = (partner >= 0 || wall) ? 1.0 : 0.0;
        a.collision_idx[i] = (double)partner;
        a.step_count[i] += 1;
    }
    if (a.reseat_poses) {
        for (int ag = t; ag < AGN; ag += 256) {
            const int e = ag / A, i = first + ag, ego_t = e * A + a.reseat_ego, ego = first + ego_t;
            if (s_partner[ego_t] >= 0 || a.in_collision[ego] != 0) reseat_agent(a, i, i == ego);
        }
    }
}

// single-agent envs: no opponents, one lane per agent is enough
__device__ __forceinline__ void finalize_solo_agent(const AgentArrays &a, int i)
{
    const int N = a.n_agents_total;
    const int wall = a.in_collision[i];
    if (wall) {
        a.state[3 * (size_t)N + i] = 0.;
        a.state[4 * (size_t)N + i] = 0.;
        a.state[5 * (size_t)N + i] = 0.;
        a.state[6 * (size_t)N + i] = 0.;
    }
    // collision_multiple on a single body returns zeros every step (collision_models.py:196-197);
    // k_collide is not launched for A = 1, so the flag is (re)written here
    a.collisions[i] = wall ? 1.0 : 0.0;
    a.step_count[i] += 1;
    if (a.reseat_poses && wall) reseat_agent(a, i, true);
}

__global__ void __launch_bounds__(256) k_finalize_solo(AgentArrays a)
{
    const int i = a.agent_begin + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= a.agent_begin + a.agent_count) return;
    finalize_solo_agent(a, i);
}

// unit-path helper: AoS poses [M][3] -> pose_x, pose_y, dir_start
__global__ void k_prepare_poses(ScanConst k, const double *__restrict__ poses, int m, double *__restrict__ px,
                                double *__restrict__ py, double *__restrict__ start)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    px[i] = poses[3 * i];
    py[i] = poses[3 * i + 1];
    start[i] = scan_start_index(k, poses[3 * i + 2]);
}

// ---- reset ------------------------------------------------------------------------------
__global__ void k_reset(AgentArrays a, const double *__restrict__ poses, const uint8_t *__restrict__ env_mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.n_agents_total;
    if (i >= N) return;
    if (env_mask && !env_mask[i / a.agents_per_env]) return;
#pragma unroll
    for (int c = 0; c < 7; ++c) a.state[(size_t)c * N + i] = 0.;
    a.state[i] = poses[3 * (size_t)i];
    a.state[(size_t)N + i] = poses[3 * (size_t)i + 1];
    a.state[4 * (size_t)N + i] = poses[3 * (size_t)i + 2];
    a.steer_buf[i] = 0.;
    a.steer_buf[(size_t)N + i] = 0.;
    a.buf_cnt[i] = 0;
    a.in_collision[i] = 0;
    a.step_count[i] = 0;
}

// in-place re-seat of finished environments (SURVEY §8d "mask reset"): an env whose ego agent
// has collisions != 0 is reset to its start poses, exactly as k_reset would with that env masked.
__global__ void k_reset_collided(AgentArrays a, const double *__restrict__ start_poses, int ego_idx,
                                 int32_t *__restrict__ n_reset)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.n_agents_total, A = a.agents_per_env;
    if (i >= N) return;
    const int env = i / A;
    if (a.collisions[env * A + ego_idx] == 0.0) return;
    // every lane of the env reads the ego flag before any lane of the env can have cleared it:
    // collisions[] is not written here (it keeps the step's value, as Simulator.collisions does)
#pragma unroll
    for (int c = 0; c < 7; ++c) a.state[(size_t)c * N + i] = 0.;
    a.state[i] = start_poses[3 * (size_t)i];
    a.state[(size_t)N + i] = start_poses[3 * (size_t)i + 1];
    a.state[4 * (size_t)N + i] = start_poses[3 * (size_t)i + 2];
    a.steer_buf[i] = 0.;
    a.steer_buf[(size_t)N + i] = 0.;
    a.buf_cnt[i] = 0;
    a.in_collision[i] = 0;
    a.step_count[i] = 0;
    if (n_reset && i - env * A == ego_idx) atomicAdd(n_reset, 1);
}

// ---- episode logic on the device ------------------------------------------------
// F110Env._check_done (f110_env.py:204-246): start/finish-zone toggles, lap counts and times, done
// = ego collided or every agent has 4 toggles — one lane per env, so an RL loop that keeps its
// policy on the GPU never has to read poses back to decide `done`.
// (struct EpisodeArrays: defined next to AgentArrays, the finalize kernels take it too)

// (envs env0 .. env0 + num_envs - 1: the whole batch, or one env block on that block's stream)
__global__ void __launch_bounds__(256) k_episode(AgentArrays a, EpisodeArrays ep, int num_envs, int env0 = 0)
{
    const int e = env0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e >= env0 + num_envs) return;
    const int N = a.n_agents_total, A = a.agents_per_env;
    const double ct = ep.current_time[e] + ep.timestep;  // f110_env.py:295
    ep.current_time[e] = ct;
    const double r00 = ep.rot[4 * e], r01 = ep.rot[4 * e + 1], r10 = ep.rot[4 * e + 2], r11 = ep.rot[4 * e + 3];
    const double left_t = 2, right_t = 2;
    bool all4 = true;
    for (int s = 0; s < A; ++s) {
        const int i = e * A + s;
        const double px = a.state[i] - ep.start_poses[3 * (size_t)i];
        const double py = a.state[(size_t)N + i] - ep.start_poses[3 * (size_t)i + 1];
        const double dx = r00 * px + r01 * py;  // np.dot(start_rot, [px; py]) :223
        double ty = r10 * px + r11 * py;
        if (ty > left_t)
            ty -= left_t;
        else if (ty < -right_t)
            ty = -right_t - ty;
        else
            ty = 0;
        const double dist2 = dx * dx + ty * ty;
        const bool closes = dist2 <= 0.1;
        bool near = ep.near_start[i] != 0;
        double tog = ep.toggle[i];
        if (closes && !near) {
            near = true;
            tog += 1;
        } else if (!closes && near) {
            near = false;
            tog += 1;
        }
        ep.near_start[i] = near ? 1 : 0;
        ep.toggle[i] = tog;
        ep.lap_count[i] = floor(tog / 2);  // toggle_list // 2
        if (tog < 4) ep.lap_time[i] = ct;
        ep.checkpoint[i] = tog >= 4 ? 1 : 0;
        all4 = all4 && (tog >= 4);
    }
    ep.done[e] = (a.collisions[e * A + ep.ego_idx] != 0.0 || all4) ? 1 : 0;  // :244
}

// every per-agent / per-env scalar a host-side RL loop reads per step, packed into one block so that
// it crosses PCIe in one copy (f110_episode_step_host): 9 double columns [N], current_time [E], then
// the byte flags near_starts [N], checkpoint_done [N], done [E]
__global__ void __launch_bounds__(256) k_pack_episode(AgentArrays a, EpisodeArrays ep, int num_envs, double *__restrict__ cols, uint8_t *__restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.n_agents_total;
    if (i < N) {
        cols[i] = a.state[i];
        cols[(size_t)N + i] = a.state[(size_t)N + i];
        cols[2 * (size_t)N + i] = a.state[4 * (size_t)N + i];
        cols[3 * (size_t)N + i] = a.state[3 * (size_t)N + i];
        cols[4 * (size_t)N + i] = a.state[5 * (size_t)N + i];
        cols[5 * (size_t)N + i] = a.collisions[i];
        cols[6 * (size_t)N + i] = ep.lap_time[i];
        cols[7 * (size_t)N + i] = ep.lap_count[i];
        cols[8 * (size_t)N + i] = ep.toggle[i];
        flags[i] = ep.near_start[i];
        flags[(size_t)N + i] = ep.checkpoint[i];
    }
    if (i < num_envs) {
        cols[9 * (size_t)N + i] = ep.current_time[i];
        flags[2 * (size_t)N + i] = ep.done[i];
    }
}

// f110_step_host: what a host-driven loop reads after a step, written by ONE kernel straight into the caller's
// page-locked block (the pointers are device-visible host memory: the stores cross PCIe as posted writes, no
// staging buffer and no copy command behind the kernel).  With the episode logic on (f110_episode_init) the
// same kernel is F110Env._check_done (k_episode's arithmetic, f110_env.py:204-246) and, with auto_reset, the
// in-place re-seat of finished envs (k_episode_reset_done) AFTER their terminal observation has been written.
// A workgroup owns whole envs (envs_per_block of them): phase 1 per agent (toggles + the agent's columns),
// phase 2 per env (done, current_time), phase 3 per agent (re-seat).  Any pointer may be nullptr.
// (struct HostBlock, host_block_signal: defined next to AgentArrays)
// the completion word of a launch whose LAST workgroup runs the host block by itself (k_step_tiny): no counting
__device__ __forceinline__ void host_block_signal_single(const HostBlock &hb)
{
    if (!hb.seq_host) return;
    __builtin_amdgcn_s_waitcnt(0); // every wave's stores into the host block have been acknowledged ...
    __syncthreads();               // ... in every wave of the workgroup
    if (threadIdx.x == 0) {
        __threadfence_system();    // ... and visible system-wide before the word
        __hip_atomic_store(hb.seq_host, hb.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The body of k_host_block for the envs [e0, e0 + ne) of a 256-thread workgroup.  SINGLE: the workgroup is the only one that runs
// it in its launch (k_step_tiny's last workgroup) and signals by itself.
template <bool SINGLE>
__device__ __forceinline__ void host_block_body(const AgentArrays &a, const EpisodeArrays &ep, const HostBlock &hb, const int e0, const int ne, int episode,
                                                int auto_reset)
{
    __shared__ int s_running[256];    // per local env: agents with fewer than 4 toggles
    __shared__ uint8_t s_done[256];
    const int A = a.agents_per_env, tid = threadIdx.x;
    const size_t N = (size_t)a.n_agents_total;
    if (episode) {
        for (int le = tid; le < ne; le += 256) s_running[le] = 0;
        __syncthreads();
    }
    const int items = ne * A;
    for (int idx = tid; idx < items; idx += 256) {
        const int le = idx / A;
        const size_t i = (size_t)e0 * A + idx;
        const double x = a.state[i], y = a.state[N + i];
        if (hb.state) {
            hb.state[i] = x;
            hb.state[N + i] = y;
#pragma unroll
            for (int c = 2; c < 7; ++c) hb.state[c * N + i] = a.state[c * N + i];
        }
        if (hb.collisions) hb.collisions[i] = a.collisions[i];
        if (hb.collision_idx) hb.collision_idx[i] = a.collision_idx[i];
        if (hb.in_collision) hb.in_collision[i] = a.in_collision[i];
        if (hb.agent_poses) {
#pragma unroll
            for (int c = 0; c < 3; ++c) hb.agent_poses[c * N + i] = a.snap_pose[c * N + i];
        }
        if (hb.trk_src) {
            if (hb.trk_s) hb.trk_s[i] = hb.trk_src[i];
            if (hb.trk_ds) hb.trk_ds[i] = hb.trk_src[N + i];
            if (hb.trk_lat) hb.trk_lat[i] = hb.trk_src[2 * N + i];
            if (hb.trk_head) hb.trk_head[i] = hb.trk_src[3 * N + i];
            if (hb.trk_seg) hb.trk_seg[i] = hb.trk_seg_src[i];
        }
        if (episode) {
            const int e = e0 + le;
            const double ct = ep.current_time[e] + ep.timestep;  // f110_env.py:295 (written back in phase 2)
            const double r00 = ep.rot[4 * e], r01 = ep.rot[4 * e + 1], r10 = ep.rot[4 * e + 2], r11 = ep.rot[4 * e + 3];
            const double left_t = 2, right_t = 2;
            const double px = x - ep.start_poses[3 * i];
            const double py = y - ep.start_poses[3 * i + 1];
            const double dx = r00 * px + r01 * py;  // np.dot(start_rot, [px; py]) :223
            double ty = r10 * px + r11 * py;
            if (ty > left_t)
                ty -= left_t;
            else if (ty < -right_t)
                ty = -right_t - ty;
            else
                ty = 0;
            const double dist2 = dx * dx + ty * ty;
            const bool closes = dist2 <= 0.1;
            bool near = ep.near_start[i] != 0;
            double tog = ep.toggle[i];
            if (closes && !near) {
                near = true;
                tog += 1;
            } else if (!closes && near) {
                near = false;
                tog += 1;
            }
            const double laps = floor(tog / 2);  // toggle_list // 2
            ep.near_start[i] = near ? 1 : 0;
            ep.toggle[i] = tog;
            ep.lap_count[i] = laps;
            double lt = ep.lap_time[i];
            if (tog < 4) {
                lt = ct;
                ep.lap_time[i] = ct;
                atomicAdd(&s_running[le], 1);
            }
            ep.checkpoint[i] = tog >= 4 ? 1 : 0;
            if (hb.lap_time) hb.lap_time[i] = lt;
            if (hb.lap_count) hb.lap_count[i] = laps;
            if (hb.toggle) hb.toggle[i] = tog;
            if (hb.near_start) hb.near_start[i] = near ? 1 : 0;
            if (hb.checkpoint) hb.checkpoint[i] = tog >= 4 ? 1 : 0;
        }
    }
    if (hb.scans) host_block_copy_scans(hb, a.scans, (size_t)e0 * A, (size_t)items);
    if (!episode) {
        if (SINGLE) host_block_signal_single(hb);
        else host_block_signal(hb);
        return;
    }
    __syncthreads();
    for (int le = tid; le < ne; le += 256) {
        const int e = e0 + le;
        const bool done = a.collisions[(size_t)e * A + ep.ego_idx] != 0.0 || s_running[le] == 0;  // :244
        const double ct = ep.current_time[e] + ep.timestep;
        if (hb.current_time) hb.current_time[e] = ct;
        if (hb.done) hb.done[e] = done ? 1 : 0;
        s_done[le] = done ? 1 : 0;
        const bool reseat = auto_reset && done;
        ep.done[e] = (done && !reseat) ? 1 : 0;
        ep.current_time[e] = reseat ? 0. : ct;
    }
    if (SINGLE) host_block_signal_single(hb);   // the host block is complete here; the re-seat below touches device memory only
    else host_block_signal(hb);
    if (!auto_reset) return;
    __syncthreads();         // s_done
    for (int idx = tid; idx < items; idx += 256) {
        if (!s_done[idx / A]) continue;
        const size_t i = (size_t)e0 * A + idx;   // F110Env.reset :319-334 without its zero-action step
#pragma unroll
        for (int c = 0; c < 7; ++c) a.state[c * N + i] = 0.;
        a.state[i] = ep.start_poses[3 * i];
        a.state[N + i] = ep.start_poses[3 * i + 1];
        a.state[4 * N + i] = ep.start_poses[3 * i + 2];
        a.steer_buf[i] = 0.;
        a.steer_buf[N + i] = 0.;
        a.buf_cnt[i] = 0;
        a.in_collision[i] = 0;
        a.step_count[i] = 0;
        ep.near_start[i] = 1;
        ep.toggle[i] = 0.;
    }
}

__global__ void __launch_bounds__(256) k_host_block(AgentArrays a, EpisodeArrays ep, HostBlock hb, int num_envs, int envs_per_block,
                                                    int episode, int auto_reset)
{
    const int e0 = blockIdx.x * envs_per_block;
    host_block_body<false>(a, ep, hb, e0, min(envs_per_block, num_envs - e0), episode, auto_reset);   // ne >= 1: the grid is ceil(num_envs / envs_per_block)
}

// ---- K0: the WHOLE step of a tiny batch as one launch (round 6) ------------------------------------------------------------
// The reference's own shape — F110Env(num_agents = 2).step, one env — is launch- and sync-bound on the GPU: three kernels of 9 + 14 + 9
// us are reported after ~60 us (profiles/r06_f110env_breakdown.txt).  For a host-synchronised step of N <= kTinyMaxAgents agents, 1 or 2 per env, this
// kernel is the step: Simulator.step (base_classes.py:553-612) — update_pose for every agent, the scans, the iTTC test, the pair test,
// the opponent ray-cast — and, under f110_step_host, F110Env._check_done (f110_env.py:204-246) + the observation block in the caller's
// page-locked memory + the completion word the host polls.  Same device functions on the same operands as the three kernels: bit-identical
// (tests/test_gpu_round6.py).
//   scan phase    one wave per 64-beam task, four per workgroup.  A wave needs its agent's lidar pose and ray header, i.e. the agent's
//                 INTEGRATION: every lane computes it (advance_vehicle + make_ray_hdr: the same instructions one lane would run), so
//                 no kernel boundary and no HBM round trip separates integrate from scan.  Nothing live is overwritten meanwhile: the
//                 wave of an agent's FIRST task stores the new state / delay buffer / poses / header into SHADOW columns, the wall
//                 flags of the iTTC test go to a flag column of their own.
//   last block    workgroups count themselves done (one release per workgroup, acquire by the last, at agent scope); the one that arrives
//                 last runs the finalize body (finalize_duo_tiny / finalize_pair_body / finalize_solo_agent) and the host epilogue ON the
//                 shadow columns, stores the completion word, and only then copies the shadow columns over the live ones.
struct TinyCtl {
    unsigned int *done;      // workgroups finished this launch (left at 0 by the last one)
    int32_t *wall;           // [N] this step's iTTC flags (left at 0 by the last workgroup)
    double *state;           // shadow of AgentArrays: [7][N]
    double *steer_buf;       // [2][N]
    int32_t *buf_cnt;        // [N]
    double *scan_pose;       // [3][N]
    double *snap_pose;       // [3][N]
    double *dir_start;       // [N]
    RayHdr *ray_hdr;         // [N]
    uint32_t tasks_per_agent, pad_;
    unsigned long long *trace;   // lab timeline probe: [workgroups][16] stamps of the 100 MHz clock (nullptr = off)
    double *host_scans;          // N = 2: the caller's page-locked scans [2][B] (device view) — finalize_duo_tiny copies the ranges there while its
                                 // role lanes work, and the beams the opponent shortens as they are found (nullptr: no scans in the block)
    FusedHost fh;                // N = 2 under f110_step_host: the host epilogue's parameters (what a.fused_host points at), by value
    int act_inline;              // 1: the actions are `act` below (f110_step_host copied them into the launch: no read over PCIe inside the step)
    int skip;                    // lab (2 = N == 2 takes finalize_pair_body instead of finalize_duo_tiny: the A/B of the tail); 1 = the launch only reports start and completion (what does the dispatch itself cost?)
    double act[8];               // [kTinyMaxAgents][2] (steer, velocity)
    unsigned long long *start_word, start_seq;   // lab: a word in page-locked host memory the first workgroup stores start_seq to as it starts
};
static_assert(sizeof(TinyCtl::act) == 8 * sizeof(double), "TinyCtl::act holds kTinyMaxAgents actions");
constexpr int kTinyMaxAgents = 4;   // (measured: beyond a handful of agents the per-kernel form wins, f110_hip.hip tiny_applies)

template <bool PAIR, bool IDENT, bool HOST>
__global__ void __launch_bounds__(256) k_step_tiny(AgentArrays a, ScanConst k, RayJob j, const double *__restrict__ actions, TinyCtl ctl, EpisodeArrays ep,
                                                   HostBlock hb, int episode, int auto_reset)
{
    __shared__ int s_last;
    const int N = a.n_agents_total, B = k.num_beams;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t task = blockIdx.x * 4u + wave;
#ifdef F110_EXPERIMENTAL
#define TINY_STAMP(slot)                                                                                         \
    do {                                                                                                         \
        if (ctl.trace && threadIdx.x == 0) ctl.trace[16ull * blockIdx.x + (slot)] = wall_clock64();             \
    } while (0)
#else
#define TINY_STAMP(slot) do { } while (0)
#endif
    TINY_STAMP(0);   // the workgroup's first wave is running
#ifdef F110_EXPERIMENTAL
    if (ctl.start_word && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(ctl.start_word, ctl.start_seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (ctl.skip == 1) {   // the dispatch alone: start word, completion word, nothing else
        if (ctl.start_word && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(ctl.start_word - 1, ctl.start_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
#endif
    AgentArrays sh = a;      // the step's view: what integration produces and the tail works on
    sh.state = ctl.state; sh.steer_buf = ctl.steer_buf; sh.buf_cnt = ctl.buf_cnt; sh.scan_pose = ctl.scan_pose;
    sh.snap_pose = ctl.snap_pose; sh.dir_start = ctl.dir_start; sh.ray_hdr = ctl.ray_hdr; sh.in_collision = ctl.wall;
    if (task < (uint32_t)N * ctl.tasks_per_agent) {
        const int i = (int)(task / ctl.tasks_per_agent);
        const uint32_t sub = task - (uint32_t)i * ctl.tasks_per_agent;
        // RaceCar.update_pose for agent i, by every lane of the wave (k_integrate's body)
        const VehicleParams vp = load_params(a.params + (size_t)(a.params_per_agent ? i : i % a.agents_per_env) * NPARAMS);
        double st[7];
#pragma unroll
        for (int c = 0; c < 7; ++c) st[c] = a.state[(size_t)c * N + i];
        double b0 = a.steer_buf[i], b1 = a.steer_buf[(size_t)N + i];
        int cnt = a.buf_cnt[i];
        double2 act;
        if (ctl.act_inline) {   // (i < 4: selects on kernel arguments)
            act.x = i == 0 ? ctl.act[0] : i == 1 ? ctl.act[2] : i == 2 ? ctl.act[4] : ctl.act[6];
            act.y = i == 0 ? ctl.act[1] : i == 1 ? ctl.act[3] : i == 2 ? ctl.act[5] : ctl.act[7];
        } else {
            act = reinterpret_cast<const double2 *>(actions)[i];
        }
        double sp[3];
        advance_vehicle(st, b0, b1, cnt, act.x, act.y, vp, a.time_step, a.integrator, a.lidar_dist, sp);
        const double start = scan_start_index(k, sp[2]);
        const RayHdr hd = make_ray_hdr(a, k, i, st, sp, start);
#ifdef F110_EXPERIMENTAL
        if (ctl.trace) {
            double probe = hd.d0;
            asm volatile("" : "+v"(probe));   // (the header's table sample has arrived)
        }
#endif
        TINY_STAMP(1);   // integration + ray header done (wave 0 of the workgroup)
        if (sub == 0u && lane == 0u) {   // the agent's new columns, into the shadow (the live ones are still being read)
            integrate_store_columns(sh, i, N, st, b0, b1, cnt, sp, start);
            sh.ray_hdr[i] = hd;
        }
        // get_scan for the task's 64 beams (k_scan_rays_agent's body)
        const int b = (int)(sub * 64u + lane);
        if (b < B) {
            const int row = hd.noise_row;
            const double nz = row >= 0 ? j.noise[(size_t)row * B + b] : 0.0;
            const double2 cs = k.cs[beam_dir_index(k, start, b)];
            int hr = -1, hc = -1, nl = 0;
            double r = 0.;
            bool exact = hd.fast == 0;
            if (hd.fast) {
                double ux, uy, cux, cuy;
                padded_position<IDENT>(k, hd.x, hd.y, ux, uy);
                padded_rate<IDENT>(k, cs.x, cs.y, cux, cuy);
                exact = !march_padded<false>(k, ux, uy, cux, cuy, hd.d0, r, hr, hc, nl);
            }
            if (exact) r = march_exact_cold<IDENT>(j.k_cold, hd.x, hd.y, cs.x, cs.y, hd.d0, hr, hc, nl);
            if (row != -1) r += nz;
            // check_ttc_jit's predicate for this beam (finish_beam_with), the flag into the step's own column
            if (hd.vel != 0.0 && !(r > j.ttc_side_max + j.ttc_k * fabs(hd.vel)) && ttc_beam_hit(r, j.side_dist[b], hd.vel, j.beam_cos[b], j.ttc_thresh))
                sh.in_collision[i] = 1;
            a.scans[(size_t)i * B + b] = r;
        }
    }
    TINY_STAMP(2);   // wave 0's beams marched and stored
    // ---- who is last?
    // Release, once per workgroup: every wave waits for its own stores to be in L2 (vmcnt 0), the barrier collects the waves, and ONE
    // lane writes the L2 back at agent scope before it counts the workgroup done (a fence by every wave is 34 L2 write-backs where 9 do).
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    TINY_STAMP(3);   // every wave of the workgroup has its stores in L2
    if (threadIdx.x == 0) {
        __threadfence();     // this workgroup's rows, flags and shadow columns are visible device-wide (other XCDs' L2s included)
        const unsigned int prev = __hip_atomic_fetch_add(ctl.done, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        s_last = prev == gridDim.x - 1u ? 1 : 0;
        if (s_last) __hip_atomic_store(ctl.done, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();     // acquire: what the other workgroups released
    TINY_STAMP(4);   // the last workgroup knows it is the last
    // ---- the last workgroup: Simulator.step's tail ON the shadow columns (sh; its in_collision is the step's flag column), the host
    //      block and the completion word — and only then shadow -> live, which nobody waits for
    TINY_STAMP(5);
    if (PAIR) {
        if (N == 2 && ctl.skip != 2) {   // the reference's own shape: one env of two cars  (skip 2: lab A/B, the general body)
            finalize_duo_tiny<HOST>(sh, B, HOST ? ctl.host_scans : nullptr, ctl.fh);
            TINY_STAMP(6);
            if (HOST && a.fused_seq) {
                HostBlock sig = ctl.fh.hb;
                sig.seq = a.fused_seq;
                host_block_signal_single(sig);
            }
            TINY_STAMP(7);
        } else {
            constexpr int AG = 4;
            for (int first = 0; first < N; first += AG) {
                finalize_pair_body<AG, HOST>(sh, B, first, N);
                __syncthreads();   // the body's LDS is reused by the next group
            }
            TINY_STAMP(6);   // finalize + host block stores issued
            if (HOST && a.fused_seq) {
                HostBlock sig = a.fused_host->hb;
                sig.seq = a.fused_seq;
                host_block_signal_single(sig);
            }
            TINY_STAMP(7);   // completion word stored
        }
    } else {
        for (int i = (int)threadIdx.x; i < N; i += 256) finalize_solo_agent(sh, i);
        if (HOST) {
            __syncthreads();
            host_block_body<true>(sh, ep, hb, 0, N, episode, auto_reset);   // one agent per env: N envs, all in this workgroup (N <= 64)
        }
        TINY_STAMP(7);
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < N; i += 256) {
#pragma unroll
        for (int c = 0; c < 7; ++c) a.state[(size_t)c * N + i] = sh.state[(size_t)c * N + i];
        a.steer_buf[i] = sh.steer_buf[i];
        a.steer_buf[(size_t)N + i] = sh.steer_buf[(size_t)N + i];
        a.buf_cnt[i] = sh.buf_cnt[i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            a.scan_pose[(size_t)c * N + i] = sh.scan_pose[(size_t)c * N + i];
            a.snap_pose[(size_t)c * N + i] = sh.snap_pose[(size_t)c * N + i];
        }
        a.dir_start[i] = sh.dir_start[i];
        a.ray_hdr[i] = sh.ray_hdr[i];
        a.in_collision[i] = sh.in_collision[i];
        sh.in_collision[i] = 0;      // (the flag column is left clear for the next launch)
    }
#undef TINY_STAMP
}

// The scalar part of Simulator.step's observation (base_classes.py:594-610), packed for the RCCL
// observation gather: [7][N] = poses_x, poses_y, poses_theta, linear_vels_x, linear_vels_y (always 0.,
// :603), ang_vels_z, collisions.  Next to the scans it is what a consumer on another GPU needs.
constexpr int kObsScalars = 7;
__global__ void __launch_bounds__(256) k_pack_obs(AgentArrays a, double *__restrict__ cols)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N = (size_t)a.n_agents_total;
    if (i >= a.n_agents_total) return;
    cols[i] = a.state[i];
    cols[N + i] = a.state[N + i];
    cols[2 * N + i] = a.state[4 * N + i];
    cols[3 * N + i] = a.state[3 * N + i];
    cols[4 * N + i] = 0.;
    cols[5 * N + i] = a.state[5 * N + i];
    cols[6 * N + i] = a.collisions[i];
}

// ---- do two streams make progress independently of each other? ------------------------------------------------------
// ROCm maps HIP streams onto a few hardware queues; two streams on ONE queue run their kernels one after the other, and
// env groups (f110_step_device) then cost time instead of saving it.  The mapping cannot be queried, but it can be
// observed: a kernel on stream a waits (bounded: `ticks` of the 100 MHz clock) for a flag that a kernel enqueued
// afterwards on stream b sets.  It sees the flag only if b's kernel ran while it was waiting.
__global__ void k_probe_wait(unsigned *flag, unsigned *seen_out, unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    unsigned seen = 0;
    while ((seen = __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0u && wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(16);
    *seen_out = seen;
}
__global__ void k_probe_set(unsigned *flag) { __hip_atomic_store(flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// float32 transport of the observation gather (f110_comm_gather_obs, F110_GATHER_F32): round-to-nearest of every range
__global__ void __launch_bounds__(256) k_scans_to_f32(const double *__restrict__ src, float *__restrict__ dst, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = (float)src[i];
}

// re-seat every env whose done flag is set (F110Env.reset :319-334 without its zero-action step)
// (agents i0 .. i0 + count - 1; count < 0: all)
__global__ void __launch_bounds__(256) k_episode_reset_done(AgentArrays a, EpisodeArrays ep, int32_t *__restrict__ n_reset, int i0 = 0, int count = -1)
{
    const int i = i0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = a.n_agents_total, A = a.agents_per_env;
    if (i >= (count < 0 ? N : i0 + count)) return;
    const int e = i / A;
    if (!ep.done[e]) return;
#pragma unroll
    for (int c = 0; c < 7; ++c) a.state[(size_t)c * N + i] = 0.;
    a.state[i] = ep.start_poses[3 * (size_t)i];
    a.state[(size_t)N + i] = ep.start_poses[3 * (size_t)i + 1];
    a.state[4 * (size_t)N + i] = ep.start_poses[3 * (size_t)i + 2];
    a.steer_buf[i] = 0.;
    a.steer_buf[(size_t)N + i] = 0.;
    a.buf_cnt[i] = 0;
    a.in_collision[i] = 0;
    a.step_count[i] = 0;
    ep.near_start[i] = 1;
    ep.toggle[i] = 0.;
    if (i - e * A == 0) {
        ep.current_time[e] = 0.;
        if (n_reset) atomicAdd(n_reset, 1);
    }
}

// done[] is read by every lane of the env above and cleared here, in a separate launch
__global__ void k_episode_clear_done(EpisodeArrays ep, int num_envs, int env0 = 0)
{
    const int e = env0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (e < env0 + num_envs) ep.done[e] = 0;
}

__global__ void k_episode_reset(AgentArrays a, EpisodeArrays ep, const double *__restrict__ poses,
                                const double *__restrict__ rot, const uint8_t *__restrict__ env_mask)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int N = a.n_agents_total, A = a.agents_per_env;
    if (i >= N) return;
    const int e = i / A;
    if (env_mask && !env_mask[e]) return;
    ep.start_poses[3 * (size_t)i] = poses[3 * (size_t)i];
    ep.start_poses[3 * (size_t)i + 1] = poses[3 * (size_t)i + 1];
    ep.start_poses[3 * (size_t)i + 2] = poses[3 * (size_t)i + 2];
    ep.near_start[i] = 1;
    ep.toggle[i] = 0.;
    ep.checkpoint[i] = 0;
    if (i - e * A == 0) {
        ep.current_time[e] = 0.;
        ep.done[e] = 0;
#pragma unroll
        for (int c = 0; c < 4; ++c) ep.rot[4 * e + c] = rot[4 * e + c];
    }
}

// ---- unit kernels (one per reference function; parity tests) ------------------------------
__global__ void k_dir_index_unit(ScanConst k, const double *__restrict__ thetas, int m, int32_t *__restrict__ idx)
{
    const int p = blockIdx.x;
    const double start = scan_start_index(k, thetas[p]);
    for (int b = threadIdx.x; b < k.num_beams; b += blockDim.x) idx[(size_t)p * k.num_beams + b] = beam_dir_index(k, start, b);
}

__global__ void k_dynamics_unit(const double *__restrict__ x, const double *__restrict__ u, const double *__restrict__ params,
                                int m, double *__restrict__ f_st, double *__restrict__ f_ks)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const VehicleParams vp = load_params(params);
    double xs[7], f[7];
#pragma unroll
    for (int c = 0; c < 7; ++c) xs[c] = x[7 * (size_t)i + c];
    rhs_single_track(xs, u[2 * i], u[2 * i + 1], vp, f);
#pragma unroll
    for (int c = 0; c < 7; ++c) f_st[7 * (size_t)i + c] = f[c];
    rhs_kinematic(xs, u[2 * i], u[2 * i + 1], vp, f);
#pragma unroll
    for (int c = 0; c < 5; ++c) f_ks[5 * (size_t)i + c] = f[c];
}

__global__ void k_pid_unit(const double *__restrict__ in, const double *__restrict__ params, int m, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const VehicleParams vp = load_params(params);
    double accl, sv;
    speed_steer_controller(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3], vp, accl, sv);
    out[2 * i] = accl;
    out[2 * i + 1] = sv;
}

__global__ void k_update_pose_unit(const double *__restrict__ s0, const double *__restrict__ buf0, const int32_t *__restrict__ cnt0,
                                   const double *__restrict__ act, const double *__restrict__ params, double dt, int integ,
                                   double lidar_dist, int m, double *__restrict__ s1, double *__restrict__ buf1,
                                   int32_t *__restrict__ cnt1, double *__restrict__ spose)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const VehicleParams vp = load_params(params);
    double st[7], sp[3];
#pragma unroll
    for (int c = 0; c < 7; ++c) st[c] = s0[7 * (size_t)i + c];
    double b0 = buf0[2 * i], b1 = buf0[2 * i + 1];
    int cnt = cnt0[i];
    advance_vehicle(st, b0, b1, cnt, act[2 * i], act[2 * i + 1], vp, dt, integ, lidar_dist, sp);
#pragma unroll
    for (int c = 0; c < 7; ++c) s1[7 * (size_t)i + c] = st[c];
    buf1[2 * i] = b0;
    buf1[2 * i + 1] = b1;
    cnt1[i] = cnt;
    spose[3 * i] = sp[0];
    spose[3 * i + 1] = sp[1];
    spose[3 * i + 2] = sp[2];
}

__global__ void k_vertices_unit(const double *__restrict__ poses, double length, double width, int m, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double v[8];
    box_vertices(poses[3 * i], poses[3 * i + 1], poses[3 * i + 2], length, width, v);
#pragma unroll
    for (int c = 0; c < 8; ++c) out[8 * (size_t)i + c] = v[c];
}

__global__ void k_gjk_unit(const double *__restrict__ va, const double *__restrict__ vb, int m, int32_t *__restrict__ flags)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double a[8], b[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        a[c] = va[8 * (size_t)i + c];
        b[c] = vb[8 * (size_t)i + c];
    }
    flags[i] = gjk_overlap(a, b) ? 1 : 0;
}

// collision_multiple :184-212 — one lane per body, same last-writer rule as k_collide
__global__ void k_collision_multiple_unit(const double *__restrict__ verts, int groups, int n, double *__restrict__ col,
                                          double *__restrict__ idx)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= groups * n) return;
    const int g = t / n, me = t - g * n;
    double mine[8], other[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) mine[c] = verts[8 * (size_t)t + c];
    bool hit = false;
    int partner = -1;
    for (int j = 0; j < n; ++j) {
        if (j == me) continue;
#pragma unroll
        for (int c = 0; c < 8; ++c) other[c] = verts[8 * ((size_t)g * n + j) + c];
        const bool cc = (me < j) ? gjk_overlap(mine, other) : gjk_overlap(other, mine);
        if (cc) {
            hit = true;
            partner = j;
        }
    }
    col[t] = hit ? 1.0 : 0.0;
    idx[t] = (double)partner;
}

__global__ void k_ttc_unit(const double *__restrict__ scans, const double *__restrict__ vels, int m, int B,
                           const double *__restrict__ beam_cos, const double *__restrict__ side, double thresh,
                           int32_t *__restrict__ flags)
{
    const int p = blockIdx.x;
    const double vel = vels[p];
    int hit = 0;
    if (vel != 0.0)
        for (int b = threadIdx.x; b < B; b += blockDim.x)
            if (ttc_beam_hit(scans[(size_t)p * B + b], side[b], vel, beam_cos[b], thresh)) hit = 1;
    const int any = __syncthreads_or(hit);
    if (threadIdx.x == 0) flags[p] = any;
}

__global__ void k_raycast_unit(const double *__restrict__ ego, const double *__restrict__ verts, int m, int B,
                               const double *__restrict__ scan_angles, double angle_inc, int uniform, double *__restrict__ scans,
                               int32_t *__restrict__ minmax)
{
    const int p = blockIdx.x, tid = threadIdx.x;
    const double ex = ego[3 * p], ey = ego[3 * p + 1], eth = ego[3 * p + 2];
    double v[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = verts[8 * (size_t)p + c];
    int ref_lo, ref_hi, lo, hi;
    if (uniform) {
        // circumscribed disc of the quadrilateral: centroid + largest vertex distance
        const double cx = (((v[0] + v[2]) + v[4]) + v[6]) / 4, cy = (((v[1] + v[3]) + v[5]) + v[7]) / 4;
        double r2 = 0.0;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const double dx = v[2 * c] - cx, dy = v[2 * c + 1] - cy;
            r2 = fmax(r2, dx * dx + dy * dy);
        }
        opponent_beam_window(ex, ey, eth, v, cx, cy, sqrt(r2) * 1.000001, scan_angles, B, angle_inc, ref_lo, ref_hi, lo, hi);
    } else {
        // a scan_angles table that is not the uniform ramp (the free function ray_cast takes any array, laser_models.py:318):
        // the reference's own full argmin per vertex (:310-313), no closed-form estimate, no disc cull — every beam of the window
        __shared__ int vidx[4];
        if (tid < 4) vidx[tid] = nearest_beam_full(scan_angles, B, vertex_view_angle(ex, ey, eth, v[2 * tid], v[2 * tid + 1]));
        __syncthreads();
        ref_lo = min(min(vidx[0], vidx[1]), min(vidx[2], vidx[3]));
        ref_hi = max(max(vidx[0], vidx[1]), max(vidx[2], vidx[3]));
        lo = ref_lo;
        hi = ref_hi;
    }
    if (minmax && tid == 0) {
        minmax[2 * p] = ref_lo;
        minmax[2 * p + 1] = ref_hi;
    }
    double *sc = scans + (size_t)p * B;
    for (int b = lo + tid; b <= hi; b += blockDim.x) {
        const double bt = eth + scan_angles[b];
        const double r0 = sc[b];
        const double r = box_range(ex, ey, cos(bt + kPi / 2.), sin(bt + kPi / 2.), v, r0);
        if (r < r0) sc[b] = r;
    }
}

__global__ void k_get_range_unit(const double *__restrict__ in, int m, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double *r = in + 8 * (size_t)i;
    const double bt = r[3];
    out[i] = edge_range(r[0], r[1], cos(bt + kPi / 2.), sin(bt + kPi / 2.), r[4], r[5], r[6], r[7]);
}

// ---- f110_helper_batch: the small functions `from f110_gym.envs import *` also exposes in the reference, one item per thread.
// Each case is the reference function's own expression order (the same device functions the step kernels inline).
__global__ void k_helper_unit(int op, const double *__restrict__ in, int m, int n, int in_w, int out_w, double *__restrict__ out, ScanConst k)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const double *a = in + (size_t)in_w * i;
    double *o = out + (size_t)out_w * i;
    switch (op) {
    case F110_OP_ACCL_CONSTRAINTS: {   // dynamic_models.py:29-60  (vel, accl, v_switch, a_max, v_min, v_max)
        VehicleParams p;
        p.v[P_VSWITCH] = a[2]; p.v[P_AMAX] = a[3]; p.v[P_VMIN] = a[4]; p.v[P_VMAX] = a[5];
        o[0] = clamp_accel(a[0], a[1], p);
        break;
    }
    case F110_OP_STEERING_CONSTRAINT: {   // :62-87  (steering_angle, steering_velocity, s_min, s_max, sv_min, sv_max)
        VehicleParams p;
        p.v[P_SMIN] = a[2]; p.v[P_SMAX] = a[3]; p.v[P_SVMIN] = a[4]; p.v[P_SVMAX] = a[5];
        o[0] = clamp_steer_rate(a[0], a[1], p);
        break;
    }
    case F110_OP_CROSS:   // laser_models.py:219-230
        o[0] = a[0] * a[3] - a[1] * a[2];
        break;
    case F110_OP_ARE_COLLINEAR: {   // :232-247  (pt_a, pt_b, pt_c)
        const double bax = a[2] - a[0], bay = a[3] - a[1];
        const double cax = a[0] - a[4], cay = a[1] - a[5];
        o[0] = fabs(bax * cay - bay * cax) < 1e-8 ? 1.0 : 0.0;
        break;
    }
    case F110_OP_PERPENDICULAR:   // collision_models.py:34-48
        o[0] = a[1];
        o[1] = -1 * a[0];
        break;
    case F110_OP_TRIPLE_PRODUCT:   // :51-64  (a, b, c)
        triple_product(a[0], a[1], a[2], a[3], a[4], a[5], o[0], o[1]);
        break;
    case F110_OP_AVG_POINT: {   // :67-78  np.sum(vertices, axis=0) / n: the rows are added in order
        double sx = a[0], sy = a[1];
        for (int q = 1; q < n; ++q) {
            sx += a[2 * q];
            sy += a[2 * q + 1];
        }
        o[0] = sx / n;
        o[1] = sy / n;
        break;
    }
    case F110_OP_FURTHEST_POINT: {   // :81-92  np.argmax(vertices.dot(d)): first maximum wins  (vertices [n][2], d)
        const double dx = a[2 * n], dy = a[2 * n + 1];
        int best = 0;
        double bv = a[0] * dx + a[1] * dy;
        for (int q = 1; q < n; ++q) {
            const double val = a[2 * q] * dx + a[2 * q + 1] * dy;
            if (val > bv) {
                bv = val;
                best = q;
            }
        }
        o[0] = (double)best;
        break;
    }
    case F110_OP_SUPPORT: {   // :95-110  (vertices1 [n][2], vertices2 [n][2], d)
        const double *v1 = a, *v2 = a + 2 * n;
        const double dx = a[4 * n], dy = a[4 * n + 1];
        int bi = 0, bj = 0;
        double vi = v1[0] * dx + v1[1] * dy, vj = v2[0] * -dx + v2[1] * -dy;
        for (int q = 1; q < n; ++q) {
            const double t1 = v1[2 * q] * dx + v1[2 * q + 1] * dy, t2 = v2[2 * q] * -dx + v2[2 * q + 1] * -dy;
            if (t1 > vi) {
                vi = t1;
                bi = q;
            }
            if (t2 > vj) {
                vj = t2;
                bj = q;
            }
        }
        o[0] = v1[2 * bi] - v2[2 * bj];
        o[1] = v1[2 * bi + 1] - v2[2 * bj + 1];
        break;
    }
    case F110_OP_GET_TRMTX: {   // :218-235  H [4][4] row-major
        double c, s;
        cos_sin(a[2], c, s);
        const double H[16] = {c, -s, 0., a[0], s, c, 0., a[1], 0., 0., 1., 0., 0., 0., 0., 1.};
        for (int q = 0; q < 16; ++q) o[q] = H[q];
        break;
    }
    case F110_OP_XY_2_RC: {   // laser_models.py:55-86  (x, y, orig_x, orig_y, orig_c, orig_s, height, width, resolution) -> (r, c)
        const double xt = a[0] - a[2], yt = a[1] - a[3];
        const double xr = xt * a[4] + yt * a[5];
        const double yr = -xt * a[5] + yt * a[4];
        const double res = a[8];
        double r = -1., c = -1.;
        if (!(xr < 0 || xr >= a[7] * res || yr < 0 || yr >= a[6] * res)) {
            c = (double)(int)(xr / res);
            r = (double)(int)(yr / res);
        }
        o[0] = r;
        o[1] = c;
        break;
    }
    case F110_OP_DISTANCE_TRANSFORM: {   // :88-104 on the handle's map  (x, y) -> dt[r, c]
        int r, c;
        o[0] = sample_distance<LAYOUT_ROWMAJOR, false, false>(k, nullptr, a[0], a[1], r, c);
        break;
    }
    case F110_OP_TRACE_RAY: {   // :106-146 on the handle's map and (cos, sin) table  (x, y, theta_index) -> range
        const int ti = (int)a[2];   // int(theta_index) :124; like NumPy, a negative index counts from the table's end
        const double2 cs = k.cs[ti < 0 ? ti + k.theta_dis : ti];
        int r, c, nl;
        o[0] = march_ray<LAYOUT_ROWMAJOR, false, false>(k, nullptr, a[0], a[1], cs.x, cs.y, r, c, nl);
        break;
    }
    default:
        break;
    }
}

// ---- map pipeline: flip + threshold + exact EDT + dt = res*sqrt(d2) ------------------------
// laser_models.py:398-404
__global__ void k_flip_threshold(const uint8_t *__restrict__ img_top_first, int H, int W, uint8_t *__restrict__ bin)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)H * W) return;
    const int r = (int)(t / W), c = (int)(t - (size_t)r * W);
    bin[t] = img_top_first[(size_t)(H - 1 - r) * W + c] > 128 ? 1 : 0;
}

constexpr uint32_t kEdtInf = 0x00007FFFu;  // "no obstacle in this column": larger than any map side

// phase 1: per column, distance to the nearest obstacle cell in that column (lane = column)
__global__ void k_edt_columns(const uint8_t *__restrict__ bin, int H, int W, uint32_t *__restrict__ g)
{
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= W) return;
    uint32_t run = kEdtInf;
    for (int y = 0; y < H; ++y) {
        run = bin[(size_t)y * W + x] ? (run >= kEdtInf ? kEdtInf : run + 1) : 0;
        g[(size_t)y * W + x] = run;
    }
    run = kEdtInf;
    for (int y = H - 1; y >= 0; --y) {
        const uint32_t cur = g[(size_t)y * W + x];
        run = (cur == 0) ? 0 : (run >= kEdtInf ? kEdtInf : run + 1);
        if (run < cur) g[(size_t)y * W + x] = run;
    }
}

// phase 2: per row, d2[u] = min_i (u-i)^2 + g[i]^2 — exact integer lower envelope by brute
// force; the row of g^2 is staged in LDS and every lane walks it (LDS broadcast reads).
__global__ void __launch_bounds__(256) k_edt_rows(const uint32_t *__restrict__ g, int H, int W, uint32_t *__restrict__ d2)
{
    extern __shared__ uint32_t g2[];
    const int y = blockIdx.x;
    for (int i = threadIdx.x; i < W; i += blockDim.x) {
        const uint32_t v = g[(size_t)y * W + i];
        g2[i] = v * v;  // <= 0x7FFF^2 < 2^30
    }
    __syncthreads();
    for (int u = threadIdx.x; u < W; u += blockDim.x) {
        uint32_t best = 0xFFFFFFFFu;
        for (int i = 0; i < W; ++i) {
            const int d = u - i;
            const uint32_t cand = (uint32_t)(d * d) + g2[i];
            best = cand < best ? cand : best;
        }
        d2[(size_t)y * W + u] = best;
    }
}

__global__ void k_dt_from_d2(const uint32_t *__restrict__ d2, size_t n, double res, double *__restrict__ dt)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) dt[t] = res * sqrt((double)d2[t]);  // laser_models.py:52
}

// PADDED layout: the table inside a border of `b` cells that read dt[-1,-1], what the reference
// returns for any out-of-bounds sample (laser_models.py:80-81,103)
__global__ void k_build_padded(const double *__restrict__ rowmajor, int H, int W, int b, int Wp, int Hp, double *__restrict__ pad)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Wp * Hp) return;
    const int r = (int)(i / Wp) - b, c = (int)(i % Wp) - b;
    const bool inside = (r >= 0) & (r < H) & (c >= 0) & (c < W);
    pad[i] = inside ? rowmajor[(size_t)r * W + c] : rowmajor[(size_t)H * W - 1];
}

// ---- static obstacles stamped into a derived map slot (f110_add_map_obstacles / f110_set_map_obstacles) --------
// The slot's table is min(base table, res * sqrt(d2 to the nearest stamped cell)): the EDT of a union is the minimum of the EDTs.
// Only the columns some obstacle's cell box touches (the ACTIVE columns, listed by the host) can hold a stamped cell, so the column
// pass runs over those and the row pass takes its minimum over them: H * W * W_active instead of k_edt_rows' H * W * W.
struct ObstBox {
    Obstacle o;
    int32_t c0, c1, r0, r1;   // obstacle_cell_box: non-empty (the host drops the others)
};

// blockIdx.y = obstacle, the x axis walks its cell box row by row.  mask [H][W] was zeroed on the stream; lanes of different
// obstacles may store the same 1 to the same byte.
__global__ void __launch_bounds__(256) k_obst_stamp(const ObstBox *__restrict__ boxes, ObstFrame f, int W, uint8_t *__restrict__ mask)
{
    const ObstBox b = boxes[blockIdx.y];
    const uint32_t bw = (uint32_t)(b.c1 - b.c0 + 1), bh = (uint32_t)(b.r1 - b.r0 + 1);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= bw * bh) return;   // (bw * bh <= 16384^2 < 2^32: f110_add_map_obstacles checks the shape)
    const uint32_t dr = t / bw;
    const int r = b.r0 + (int)dr, c = b.c0 + (int)(t - dr * bw);
    if (obstacle_hit(b.o, f, r, c)) mask[(size_t)r * W + c] = 1;
}

// k_edt_columns over the active columns: lane = active column a (table column cols[a]); g [H][Wa].  A column without a stamped
// cell carries kEdtInf in every row.
__global__ void k_obst_columns(const uint8_t *__restrict__ mask, const int32_t *__restrict__ cols, int H, int W, int Wa, uint32_t *__restrict__ g)
{
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= Wa) return;
    const int x = cols[a];
    uint32_t run = kEdtInf;
    for (int y = 0; y < H; ++y) {
        run = mask[(size_t)y * W + x] ? 0 : (run >= kEdtInf ? kEdtInf : run + 1);
        g[(size_t)y * Wa + a] = run;
    }
    run = kEdtInf;
    for (int y = H - 1; y >= 0; --y) {
        const uint32_t cur = g[(size_t)y * Wa + a];
        run = (cur == 0) ? 0 : (run >= kEdtInf ? kEdtInf : run + 1);
        if (run < cur) g[(size_t)y * Wa + a] = run;
    }
}

// a d2 made of kEdtInf columns only (or of none) means "nothing stamped": any real one is below (W^2 + H^2 <= 2^29)
constexpr uint32_t kObstNone = kEdtInf * kEdtInf;

__device__ __forceinline__ double obst_value(double base, uint32_t d2, double res)
{
    if (d2 >= kObstNone) return base;
    const double v = res * sqrt((double)d2);   // k_dt_from_d2's expression
    return v < base ? v : base;
}

// The slot's out-of-bounds value T'[H-1][W-1], before the row pass needs it for the border: one workgroup reduces the corner
// cell's candidates.  Written to *oob (the row pass and the host read it) and, when the env-map tables are on the device, into the
// slot's ScanConst there.
__global__ void __launch_bounds__(256) k_obst_corner(const uint32_t *__restrict__ g, const int32_t *__restrict__ cols, int Wa, const double *__restrict__ base,
                                                     int base_row_bytes, int H, int W, double res, double *__restrict__ oob, double *__restrict__ oob_dev)
{
    __shared__ uint32_t part[256];
    uint32_t best = 0xFFFFFFFFu;
    for (int a = threadIdx.x; a < Wa; a += 256) {
        const int d = W - 1 - cols[a];
        const uint32_t v = g[(size_t)(H - 1) * Wa + a];
        const uint32_t cand = (uint32_t)(d * d) + v * v;
        best = cand < best ? cand : best;
    }
    part[threadIdx.x] = best;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] = part[threadIdx.x + s] < part[threadIdx.x] ? part[threadIdx.x + s] : part[threadIdx.x];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double b = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + (size_t)(H - 1) * (size_t)base_row_bytes + (size_t)(W - 1) * 8);
        const double v = obst_value(b, part[0], res);
        *oob = v;
        if (oob_dev) *oob_dev = v;
    }
}

// The row pass, the minimum with the base and res * sqrt in one kernel, writing the slot's padded copy: blockIdx.y = padded row,
// each lane one padded column.  A workgroup of an interior row stages the active columns' (index, g^2) in LDS, kObstChunk at a
// time, and every lane walks them (broadcast reads); border cells (and whole border workgroups, before any barrier) store *oob.
constexpr int kObstChunk = 2048;   // 16 KiB of LDS
__global__ void __launch_bounds__(256) k_obst_rows(const uint32_t *__restrict__ g, const int32_t *__restrict__ cols, int Wa, const double *__restrict__ base,
                                                   int base_row_bytes, int H, int W, int b, int Wp, double res, const double *__restrict__ oob,
                                                   double *__restrict__ pad)
{
    __shared__ uint2 act[kObstChunk];
    const int pr = blockIdx.y, pc0 = blockIdx.x * 256, pc = pc0 + (int)threadIdx.x;
    const int r = pr - b, c = pc - b;
    double *const out = pad + (size_t)pr * Wp + pc;
    if (r < 0 || r >= H || pc0 - b >= W || pc0 + 255 - b < 0) {   // workgroup-uniform: nothing but border
        if (pc < Wp) *out = *oob;
        return;
    }
    uint32_t best = 0xFFFFFFFFu;
    for (int a0 = 0; a0 < Wa; a0 += kObstChunk) {
        const int n = Wa - a0 < kObstChunk ? Wa - a0 : kObstChunk;
        if (a0) __syncthreads();   // the previous chunk has been read
        for (int i = threadIdx.x; i < n; i += 256) {
            const uint32_t v = g[(size_t)r * Wa + a0 + i];
            act[i] = make_uint2((uint32_t)cols[a0 + i], v * v);   // v <= kEdtInf: v^2 < 2^30
        }
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            const uint2 e = act[i];
            const int d = c - (int)e.x;   // |d| < 2^15: d^2 + g^2 < 2^31
            const uint32_t cand = (uint32_t)(d * d) + e.y;
            best = cand < best ? cand : best;
        }
    }
    if (pc >= Wp) return;
    if (c < 0 || c >= W) {
        *out = *oob;
        return;
    }
    const double bv = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base) + (size_t)r * (size_t)base_row_bytes + (size_t)c * 8);
    *out = obst_value(bv, best, res);
}

// ---- a corridor carved into a map slot (f110_add_map_corridor / f110_set_map_corridor) ----------------------------
// The carved mask [H][W], 1 = carved, in the bitmap convention k_edt_columns reads (row 0 = bottom, non-zero = free), the border
// ring already 0.  A workgroup of four waves takes a tile of kCorrTileH x kCorrTileW cells: lane = column, wave w the rows w, w + 4,
// w + 8, w + 12 of the tile.  It first walks the S segments kCorrChunk at a time, one per lane, and keeps in LDS those whose capsule
// can reach the tile (corridor_reaches: conservative); a list that fills up is swept against the tile's cells at once (a round) and
// started again, so no kept segment is dropped.  A cell leaves a sweep at its first hit and is not tested again; a tile that keeps
// nothing stores zeros without a cell test.  The carved cells are counted by ballot per row and one atomic per wave.
__global__ void __launch_bounds__(kCorrChunk) k_corridor_mask(const double *__restrict__ xy, const double *__restrict__ hw, int M, int S, ObstFrame f, int H, int W,
                                                              uint8_t *__restrict__ mask, unsigned long long *__restrict__ carved)
{
    static_assert(kCorrChunk == 256 && kCorrTileW == 64 && kCorrTileH == 16 && kCorrCap >= kCorrChunk,
                  "four waves, a lane per column, four rows per wave; what a chunk leaves behind a round fits the list");
    __shared__ CorridorSeg list[kCorrCap];
    __shared__ int wave_kept[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c0 = (int)blockIdx.x * kCorrTileW, r0 = (int)blockIdx.y * kCorrTileH;   // (the grid covers the table: c0 < W, r0 < H)
    const int c1 = (c0 + kCorrTileW < W ? c0 + kCorrTileW : W) - 1, r1 = (r0 + kCorrTileH < H ? r0 + kCorrTileH : H) - 1;
    const CorridorTile tile = corridor_tile(f, r0, c0, r1, c1);
    const int c = c0 + lane;
    double wx[4], wy[4];
    unsigned live = 0, hit = 0;   // bit q: the cell of row r0 + wave + 4 q is still undecided / is carved
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + wave + 4 * q;
        wx[q] = wy[q] = 0.0;
        if (r > 0 && r < H - 1 && c > 0 && c < W - 1) {   // inside the ring
            live |= 1u << q;
            cell_centre(f, r, c, wx[q], wy[q]);
        }
    }
    const auto sweep = [&](int count) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (!((live >> q) & 1u)) continue;
            for (int i = 0; i < count; ++i)
                if (corridor_hit(list[i], wx[q], wy[q])) {
                    hit |= 1u << q;
                    live &= ~(1u << q);
                    break;
                }
        }
    };
    int n = 0;   // the list's length (the same in every lane)
    for (int s0 = 0; s0 < S; s0 += kCorrChunk) {
        const int s = s0 + tid;
        bool keep = false;
        double ax = 0.0, ay = 0.0, bx = 0.0, by = 0.0, w = 0.0;
        if (s < S) {
            const int e = s + 1 == M ? 0 : s + 1;
            ax = xy[2 * s];
            ay = xy[2 * s + 1];
            bx = xy[2 * e];
            by = xy[2 * e + 1];
            w = hw[s];
            keep = corridor_reaches(ax, ay, bx, by, w, tile);
        }
        const unsigned long long kept = __ballot(keep);
        if (lane == 0) wave_kept[wave] = __popcll(kept);
        __syncthreads();
        int before = 0, total = 0;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const int k = wave_kept[v];
            before += v < wave ? k : 0;
            total += k;
        }
        const int pos = n + before + __popcll(kept & ((1ull << lane) - 1ull));
        int slot = keep ? corridor_list_slot(pos, true) : -1;
        if (slot >= 0) list[slot] = corridor_seg(ax, ay, bx, by, w);
        if (n + total > kCorrCap) {   // workgroup-uniform: the list is full, the chunk has more
            __syncthreads();
            sweep(kCorrCap);
            __syncthreads();
            slot = keep ? corridor_list_slot(pos, false) : -1;
            if (slot >= 0) list[slot] = corridor_seg(ax, ay, bx, by, w);
            n += total - kCorrCap;
        } else {
            n += total;
        }
        __syncthreads();   // the list is written, and wave_kept has been read before the next chunk writes it
    }
    sweep(n);
    unsigned mine = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = r0 + wave + 4 * q;
        const bool on = (hit >> q) & 1u;
        if (c < W && r < H) mask[(size_t)r * W + c] = on ? 1 : 0;
        mine += (unsigned)__popcll(__ballot(on));
    }
    if (lane == 0 && mine) atomicAdd(carved, (unsigned long long)mine);
}

// The slot's padded copy straight from the squared distances: res * sqrt(d2) (k_dt_from_d2's expression) inside, the value of cell
// [H-1][W-1] in the border (k_build_padded's rule), which also goes into the slot's ScanConst on the device when there is one.
__global__ void __launch_bounds__(256) k_corridor_table(const uint32_t *__restrict__ d2, int H, int W, int b, int Wp, int Hp, double res, double *__restrict__ pad,
                                                        double *__restrict__ oob_dev)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)Wp * Hp) return;
    const int r = (int)(i / Wp) - b, c = (int)(i % Wp) - b;
    const bool inside = (r >= 0) & (r < H) & (c >= 0) & (c < W);
    const double v = res * sqrt((double)d2[inside ? (size_t)r * W + c : (size_t)H * W - 1]);
    pad[i] = v;
    if (i == 0 && oob_dev) *oob_dev = v;   // (cell 0 of the padded copy is a border cell, or with b = 0 a ring cell: the same value)
}

// ---- raceline and speed profile (include/f110.h, f110_raceline_batch) ---------------------------------------------
// One workgroup per line (the batch is the grid), NT lanes, point i of the line in lane i % NT as its slot i / NT (at most
// kRacelinePerLane slots): q, n, b, alpha and y of a point stay in its lane's registers for the whole solve, p lives in LDS in two
// copies (read-old / write-new, so an iteration costs ONE barrier), beta in LDS too: the iteration loop touches no global memory
// and no atomics, and workgroups never talk.  On a coarse level only the lanes whose points are active work; nothing is compacted.
// The per-point arithmetic is f110_math.hpp's rl_*.
struct RacelineJob {
    const double *xy, *hw;        // the lines one after the other: [sum M][2], [sum M]
    const int32_t *off;           // [T + 1]: line t is rows off[t] .. off[t + 1]
    const int32_t *line_iters;    // [T]: the line's iteration count per level (<= sp.iters)
    const double *beta;           // [sp.iters]
    RacelineSpec sp;
    double *alpha, *out_xy, *kappa, *vx;   // rows as xy / hw
    double *length, *lap_time;             // [T]
    int32_t *status;                       // [T]: 0, or 1 = rl_degenerate: a raceline segment of zero length or a curvature that is not finite (nothing else written for the line)
};

// inclusive running minimum of a[0 .. M) (reverse: from the far end) by doubling between a and b, a barrier per round; the caller
// wrote a and has not synchronised.  Returns where the result lies; the caller synchronises before it writes either buffer again.
template <int NT>
__device__ const double *rl_scan_min(double *a, double *b, int M, int tid, bool reverse)
{
    __syncthreads();
    for (int d = 1; d < M; d <<= 1) {
#pragma unroll
        for (int e = 0; e < kRacelinePerLane; ++e) {
            const int i = tid + e * NT;
            if (i >= M) continue;
            const int j = reverse ? i + d : i - d;
            double v = a[i];
            if (j >= 0 && j < M) v = rl_min(v, a[j]);
            b[i] = v;
        }
        __syncthreads();
        double *const t = a;
        a = b;
        b = t;
    }
    return a;
}

// NT lanes take lines of up to NT * kRacelinePerLane points, NB is the capacity of the beta table: LDS is 128 NT + 8 NB bytes
// (NT = 1024, NB = 4096: all 160 KiB of the CU).
template <int NT, int NB>
__global__ void __launch_bounds__(NT) k_raceline(RacelineJob job)
{
    constexpr int CAP = NT * kRacelinePerLane;
    __shared__ __attribute__((aligned(16))) double lds[4 * CAP];
    __shared__ double s_beta[NB];
    const int t = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int o = job.off[t], M = job.off[t + 1] - o;
    const int iters = job.line_iters[t], levels = job.sp.levels;
    double2 *cur = reinterpret_cast<double2 *>(lds), *nxt = reinterpret_cast<double2 *>(lds + 2 * CAP);
    for (int k = tid; k < iters; k += NT) s_beta[k] = job.beta[k];

    // step 1
    double qx[kRacelinePerLane], qy[kRacelinePerLane], nx[kRacelinePerLane], ny[kRacelinePerLane], b[kRacelinePerLane], al[kRacelinePerLane], y[kRacelinePerLane];
#pragma unroll
    for (int e = 0; e < kRacelinePerLane; ++e) {
        const int i = tid + e * NT;
        qx[e] = qy[e] = nx[e] = ny[e] = b[e] = al[e] = y[e] = 0.0;
        if (i >= M) continue;
        const int im = i == 0 ? M - 1 : i - 1, ip = i + 1 == M ? 0 : i + 1;
        qx[e] = job.xy[2 * (size_t)(o + i)];
        qy[e] = job.xy[2 * (size_t)(o + i) + 1];
        (void)rl_frame(job.xy[2 * (size_t)(o + im)], job.xy[2 * (size_t)(o + im) + 1], job.xy[2 * (size_t)(o + ip)], job.xy[2 * (size_t)(o + ip) + 1], job.hw[o + i],
                       job.sp.margin, nx[e], ny[e], b[e]);
    }

    // step 2 (the first barrier below also publishes s_beta)
    for (int lv = levels; lv >= 0; --lv) {
        const int s = 1 << lv;
        if (lv < levels) {   // prolong: the coarser level's alpha through LDS, then the points between
            double *const a_lds = lds;
#pragma unroll
            for (int e = 0; e < kRacelinePerLane; ++e) {
                const int i = tid + e * NT;
                if (i < M && (i & (2 * s - 1)) == 0) a_lds[i] = al[e];
            }
            __syncthreads();
#pragma unroll
            for (int e = 0; e < kRacelinePerLane; ++e) {
                const int i = tid + e * NT;
                if (i < M && (i & (2 * s - 1)) == s) al[e] = rl_prolong(a_lds[i - s], a_lds[i + s == M ? 0 : i + s], b[e]);   // (2 s divides M: i + s <= M)
            }
            __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < kRacelinePerLane; ++e) {
            const int i = tid + e * NT;
            if (i >= M || (i & (s - 1))) continue;
            y[e] = al[e];
            double px, py;
            rl_point(qx[e], qy[e], y[e], nx[e], ny[e], px, py);
            cur[i] = make_double2(px, py);
        }
        __syncthreads();
        for (int k = 0; k < iters; ++k) {
            const double beta = s_beta[k];
#pragma unroll
            for (int e = 0; e < kRacelinePerLane; ++e) {
                const int i = tid + e * NT;
                if (i >= M || (i & (s - 1))) continue;
                double px[5], py[5];
#pragma unroll
                for (int m = 0; m < 5; ++m) {   // (M / s >= 8: one wrap at most)
                    int j = i + (m - 2) * s;
                    j = j < 0 ? j + M : (j >= M ? j - M : j);
                    const double2 p = cur[j];
                    px[m] = p.x;
                    py[m] = p.y;
                }
                rl_update(px, py, nx[e], ny[e], b[e], beta, y[e], al[e]);
                double wx, wy;
                rl_point(qx[e], qy[e], y[e], nx[e], ny[e], wx, wy);
                nxt[i] = make_double2(wx, wy);
            }
            __syncthreads();
            double2 *const sw = cur;
            cur = nxt;
            nxt = sw;
        }
    }

    // step 3: the line in LDS, curvature and segment lengths per point, the running sum by one lane
    double2 *const P = reinterpret_cast<double2 *>(lds);
    double *const r0 = lds, *const r1 = lds + CAP, *const r2 = lds + 2 * CAP, *const r3 = lds + 3 * CAP;
    double px[kRacelinePerLane], py[kRacelinePerLane], len[kRacelinePerLane], kap[kRacelinePerLane];
#pragma unroll
    for (int e = 0; e < kRacelinePerLane; ++e) {
        const int i = tid + e * NT;
        px[e] = py[e] = len[e] = kap[e] = 0.0;
        if (i >= M) continue;
        rl_point(qx[e], qy[e], al[e], nx[e], ny[e], px[e], py[e]);
        P[i] = make_double2(px[e], py[e]);
    }
    if (tid == 0) r3[0] = 0.0;   // the line's refusal flag (r3[1]: its length)
    __syncthreads();
    bool bad = false;
#pragma unroll
    for (int e = 0; e < kRacelinePerLane; ++e) {
        const int i = tid + e * NT;
        if (i >= M) continue;
        const double2 a = P[i == 0 ? M - 1 : i - 1], c = P[i + 1 == M ? 0 : i + 1];
        len[e] = rl_length(px[e], py[e], c.x, c.y);
        kap[e] = rl_curvature(a.x, a.y, px[e], py[e], c.x, c.y);
        bad |= rl_degenerate(len[e], kap[e]);
        r2[i] = len[e];
    }
    if (bad) r3[0] = 1.0;
    __syncthreads();
    if (r3[0] != 0.0) {   // (the same answer in every lane)
        if (tid == 0) job.status[t] = 1;
        return;
    }
    if (tid == 0) {
        double acc = 0.0;
        for (int i = 0; i < M; ++i) {
            const double l = r2[i];
            r2[i] = acc;
            acc += l;
        }
        r3[1] = acc;
    }
    __syncthreads();
    const double L = r3[1];
    const double inf = __longlong_as_double(0x7ff0000000000000ll);

    // step 4: the ceiling, the four minima as scans between r0 and r1, the profile, the lap time by one lane
    double cum[kRacelinePerLane], cl[kRacelinePerLane], mn[4][kRacelinePerLane];
#pragma unroll
    for (int e = 0; e < kRacelinePerLane; ++e) {
        const int i = tid + e * NT;
        cum[e] = cl[e] = 0.0;
        if (i >= M) continue;
        cum[e] = r2[i];
        cl[e] = rl_ceiling(kap[e], job.sp.v_max, job.sp.a_lat);
    }
#pragma unroll
    for (int pass = 0; pass < 4; ++pass) {   // pre_f (j <= i), suf_f (j > i), suf_g (j >= i), pre_g (j < i)
        const bool is_g = pass >= 2, reverse = pass == 1 || pass == 2, exclusive = pass == 1 || pass == 3;
#pragma unroll
        for (int e = 0; e < kRacelinePerLane; ++e) {
            const int i = tid + e * NT;
            if (i < M) r0[i] = is_g ? rl_G(cl[e], cum[e], job.sp.a_brake) : rl_F(cl[e], cum[e], job.sp.a_accel);
        }
        const double *const res = rl_scan_min<NT>(r0, r1, M, tid, reverse);
#pragma unroll
        for (int e = 0; e < kRacelinePerLane; ++e) {
            const int i = tid + e * NT;
            mn[pass][e] = inf;
            if (i >= M) continue;
            const int j = exclusive ? (reverse ? i + 1 : i - 1) : i;
            if (j >= 0 && j < M) mn[pass][e] = res[j];
        }
        __syncthreads();
    }
    double v[kRacelinePerLane];
#pragma unroll
    for (int e = 0; e < kRacelinePerLane; ++e) {
        const int i = tid + e * NT;
        v[e] = 0.0;
        if (i >= M) continue;
        v[e] = rl_speed(cl[e], cum[e], L, job.sp.a_accel, job.sp.a_brake, mn[0][e], mn[1][e], mn[2][e], mn[3][e]);
        r3[i] = v[e];
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < kRacelinePerLane; ++e) {
        const int i = tid + e * NT;
        if (i >= M) continue;
        r2[i] = rl_lap_term(len[e], v[e], r3[i + 1 == M ? 0 : i + 1]);
        job.alpha[o + i] = al[e];
        job.out_xy[2 * (size_t)(o + i)] = px[e];
        job.out_xy[2 * (size_t)(o + i) + 1] = py[e];
        job.kappa[o + i] = kap[e];
        job.vx[o + i] = v[e];
    }
    __syncthreads();
    if (tid == 0) {
        double lap = 0.0;
        for (int i = 0; i < M; ++i) lap += r2[i];
        job.length[t] = L;
        job.lap_time[t] = lap;
        job.status[t] = 0;
    }
}

// ---- centreline extraction (include/f110.h, f110_map_centerline) --------------------------------------------------
// The mask is a bit plane [H][Ww] of 64-bit words, Ww = ceil(W / 64): bit b of word w is column 64 w + b, bits from column W on
// are 0 in every plane.  The per-word decisions are f110_math.hpp's cl_*.

// The free mask of a slot's table: one wave per word, lane b tests T[r][64 w + b] > 0 and the wave's ballot IS the word.
// blockIdx.y = row, a workgroup of four waves takes four consecutive words.
__global__ void __launch_bounds__(256) k_cl_free(const double *__restrict__ table, int row_bytes, int H, int W, int Ww, uint64_t *__restrict__ plane)
{
    const int r = blockIdx.y, w = blockIdx.x * 4 + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    const int c = w * 64 + lane;
    bool free_cell = false;
    if (w < Ww && c < W) free_cell = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(table) + (size_t)r * (size_t)row_bytes + (size_t)c * 8) > 0.0;
    const uint64_t word = __ballot(free_cell);
    if (lane == 0 && w < Ww) plane[(size_t)r * Ww + w] = word;
}

// One pass, src -> dst (never the same plane: every decision reads the mask as it was before the pass): a lane per word.  op as
// cl_pass_word takes it.  The pass's deletions are added to *deleted, one atomic per wave that deleted anything.
__device__ __forceinline__ void cl_pass(int op, const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int H, int Ww, unsigned long long *__restrict__ deleted)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t mine = 0;
    if (t < (size_t)H * Ww) {
        const int r = (int)(t / (size_t)Ww), w = (int)(t - (size_t)r * Ww);
        uint64_t out;
        mine = (uint32_t)__popcll(cl_pass_word(op, src, H, Ww, r, w, out));
        dst[t] = out;
    }
    for (int off = 32; off; off >>= 1) mine += __shfl_xor(mine, off);
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(deleted, (unsigned long long)mine);
}

__global__ void __launch_bounds__(256) k_cl_thin(int sub, const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int H, int Ww,
                                                 unsigned long long *__restrict__ deleted)
{
    cl_pass(sub, src, dst, H, Ww, deleted);
}

__global__ void __launch_bounds__(256) k_cl_stair(int k, const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int H, int Ww,
                                                  unsigned long long *__restrict__ deleted)
{
    cl_pass(2 + k, src, dst, H, Ww, deleted);
}

__global__ void __launch_bounds__(256) k_cl_prune(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, int H, int Ww, unsigned long long *__restrict__ deleted)
{
    cl_pass(6, src, dst, H, Ww, deleted);
}

// T at a list of cells (r, c), all inside the table (the host traced them on the mask): the loop's half widths
__global__ void __launch_bounds__(256) k_cl_gather(const double *__restrict__ table, int row_bytes, const int32_t *__restrict__ cells, int n, double *__restrict__ out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = cells[2 * i], c = cells[2 * i + 1];
    out[i] = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(table) + (size_t)r * (size_t)row_bytes + (size_t)c * 8);
}


// A reactive policy that CONSUMES the scans where the scan kernel left them (round 5; not a reference function — the stand-in
// for an RL policy in a device-resident loop: examples/rl_loop_device.py, bench.py's "scans consumed on device" leg).  One wave
// per agent: the B beams are cut into 64 sectors, sector s = beams [ceil(s B / 64), ceil((s + 1) B / 64)); each lane takes the
// mean range of its sector (beams added in ascending order).  Steer towards the centre of the sector with the largest mean
// among those within `sector_limit` rad of straight ahead (first maximum), speed from the shortest range of the eight middle
// sectors.  actions [n][2] = (steer, speed).
__global__ void __launch_bounds__(256) k_scan_policy(const double *__restrict__ scans, int B, double fov, int i0, int n, double steer_gain, double steer_max,
                                                     double sector_limit, double v_lo, double v_hi, double d_ref, double *__restrict__ actions)
{
    // the agent's row goes through LDS: 64 consecutive ranges per load instruction (4 lines), then every lane walks its own
    // sector there (reading the sectors straight from HBM touches 64 lines per instruction, 16 x the traffic)
    extern __shared__ double lds_rows[];   // [4 waves][B]
    const int a = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    if (a >= n) return;
    const int lane = (int)(threadIdx.x & 63u);
    const double *row = scans + (size_t)(i0 + a) * (size_t)B;
    double *mine = lds_rows + (size_t)(threadIdx.x >> 6) * (size_t)B;
    for (int b = lane; b < B; b += 64) mine[b] = row[b];
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS writes are in order; the barrier only pins the compiler)
    const int b0 = (lane * B + 63) / 64, b1 = ((lane + 1) * B + 63) / 64;
    double sum = 0., lo = INFINITY;
    for (int b = b0; b < b1; ++b) {
        const double r = mine[b];
        sum += r;
        lo = r < lo ? r : lo;
    }
    const double inc = fov / (double)(B - 1);
    const double centre = -fov / 2. + inc * (0.5 * (double)(b0 + b1 - 1));
    double best = (b1 > b0 && fabs(centre) <= sector_limit) ? sum / (double)(b1 - b0) : -INFINITY;
    int best_lane = lane;
    double front = (lane >= 28 && lane < 36) ? lo : INFINITY;
    for (int off = 32; off; off >>= 1) {
        const double ob = __shfl_xor(best, off);
        const int ol = __shfl_xor(best_lane, off);
        if (ob > best || (ob == best && ol < best_lane)) {
            best = ob;
            best_lane = ol;
        }
        const double of = __shfl_xor(front, off);
        front = of < front ? of : front;
    }
    const double best_centre = __shfl(centre, best_lane);
    if (lane == 0) {
        // no eligible sector (none within sector_limit, or every eligible mean is NaN): straight ahead, not the tie-break's lane 0
        double steer = best > -INFINITY ? steer_gain * best_centre : 0.0;
        steer = steer > steer_max ? steer_max : (steer < -steer_max ? -steer_max : steer);
        const double f = front / d_ref;
        actions[2 * (size_t)(i0 + a)] = steer;
        actions[2 * (size_t)(i0 + a) + 1] = v_lo + (v_hi - v_lo) * (f < 1. ? f : 1.);
    }
}

// examples/waypoint_follow.py: PurePursuitPlanner.plan, 16 lanes per pose (4 poses per wave).  The
// lanes of a group split the segments of the waypoint polyline: the nearest-point search is a
// per-lane first-minimum followed by a (distance, index) lexicographic min across the group — the
// same winner as np.argmin's first minimum — and the look-ahead search tests 16 segments at a
// time and takes the lowest hit.  Per-segment arithmetic is f110_math.hpp's, unchanged.
// actions [n][2] = (steer, speed).
constexpr int kPlanLanes = 16;

__global__ void __launch_bounds__(256) k_pure_pursuit(const double *__restrict__ wp, int M, const double *__restrict__ px_,
                                                      const double *__restrict__ py_, const double *__restrict__ pth_, int stride, int n,
                                                      double lookahead, double vgain, double wheelbase, double max_reacquire,
                                                      double *__restrict__ actions)
{
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / kPlanLanes;   // pose
    const int sub = threadIdx.x & (kPlanLanes - 1);
    const int grp_shift = (threadIdx.x & 63) & ~(kPlanLanes - 1);            // first lane of my group in the wave
    const bool live = gid < n;
    const int g = live ? gid : n - 1;   // idle groups shadow the last pose so the wave stays convergent
    const double px = px_[(size_t)g * stride], py = py_[(size_t)g * stride], theta = pth_[(size_t)g * stride];
    // ---- nearest_point_on_trajectory :15-50
    double dist = INFINITY, tb = 0.0;
    int best = 0x7fffffff;
    for (int k = sub; k + 1 < M; k += kPlanLanes) {
        const double ax = wp[3 * k], ay = wp[3 * k + 1];
        const double dx = wp[3 * k + 3] - ax, dy = wp[3 * k + 4] - ay;
        double t = ((px - ax) * dx + (py - ay) * dy) / (dx * dx + dy * dy);
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double rx = px - (ax + t * dx), ry = py - (ay + t * dy);
        const double d = sqrt(rx * rx + ry * ry);
        if (d < dist) {
            dist = d;
            tb = t;
            best = k;
        }
    }
#pragma unroll
    for (int m = 1; m < kPlanLanes; m <<= 1) {
        const double od = __shfl_xor(dist, m, kPlanLanes), ot = __shfl_xor(tb, m, kPlanLanes);
        const int ob = __shfl_xor(best, m, kPlanLanes);
        if (od < dist || (od == dist && ob < best)) {
            dist = od;
            tb = ot;
            best = ob;
        }
    }
    if (best == 0x7fffffff) best = 0;   // all distances NaN: np.argmin -> 0
    // ---- _get_current_waypoint :183-201
    int goal = best;
    bool have = true;
    if (dist < lookahead) {
        // first_point_on_trajectory_intersecting_circle :52-132, wrap=True
        const double start = (double)best + tb;
        const int start_i = (int)start;
        const double start_t = fmod(start, 1.0);
        goal = -1;
        for (int base = start_i; base + 1 < M && goal < 0; base += kPlanLanes) {
            const int i = base + sub;
            const bool hit = (i + 1 < M) &&
                             lookahead_cuts(wp[3 * i], wp[3 * i + 1], wp[3 * i + 3], wp[3 * i + 4], px, py, lookahead, i == start_i ? start_t : 0.0);
            const unsigned m16 = (unsigned)((__ballot(hit) >> grp_shift) & 0xffffull);
            if (m16) goal = base + __ffs(m16) - 1;
        }
        for (int base = -1; base < start_i && goal < 0; base += kPlanLanes) {
            const int i = base + sub;
            bool hit = false;
            if (i < start_i) {
                const int k0 = i < 0 ? M - 1 : i, k1 = i + 1;
                hit = lookahead_cuts(wp[3 * k0], wp[3 * k0 + 1], wp[3 * k1], wp[3 * k1 + 1], px, py, lookahead, 0.0);
            }
            const unsigned m16 = (unsigned)((__ballot(hit) >> grp_shift) & 0xffffull);
            if (m16) {
                const int i0 = base + __ffs(m16) - 1;
                goal = i0 < 0 ? M - 1 : i0;
            }
        }
        have = goal >= 0;
    } else if (!(dist < max_reacquire)) {
        have = false;
    }
    if (sub != 0 || !live) return;
    // ---- get_actuation :134-145, plan :203-217
    double steer = 0.0, speed = 4.0;
    if (have) {
        const double wy = sin(-theta) * (wp[3 * goal] - px) + cos(-theta) * (wp[3 * goal + 1] - py);
        speed = vgain * wp[3 * best + 2];
        if (!(fabs(wy) < 1e-6)) {
            const double radius = 1 / (2.0 * wy / (lookahead * lookahead));
            steer = atan(wheelbase / radius);
        }
    }
    reinterpret_cast<double2 *>(actions)[gid] = make_double2(steer, speed);
}

__global__ void k_interleave_cs(const double *__restrict__ sines, const double *__restrict__ cosines, int n, double2 *__restrict__ cs)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) cs[i] = make_double2(cosines[i], sines[i]);
}

// ---- track progress (f110_track_*): per-agent projection on the raceline of the env's map slot ------------------------------
// A track is a polyline of nseg segments, stored per slot as seven SoA columns [7][nseg]: ax, ay, dx, dy, l2 = dx²+dy², len =
// sqrt(l2), cum (float64 running sum of len, built on the host).  The search is nearest_on_trajectory's (f110_math.hpp) with
// k_pure_pursuit's split: the 16 lanes of a group take every 16th segment, keep their first minimum, and a lexicographic
// (dist, index) min across the group picks np.argmin's winner.
// Pruning: the group first measures the segment that won this agent's last projection (any segment's distance is an upper bound
// of the minimum), and a lane skips segment k when |p - mid_k| - len_k / 2 — a lower bound of its true distance — exceeds the
// smaller of that bound and the lane's running minimum by more than kTrackPruneMargin (1 um, far above the float64 rounding of
// either side at any map size).  A skipped segment's computed distance is then strictly larger than the minimum: it can neither
// win nor tie, so the winner is the full first-minimum search's, bit for bit.
struct TrackDesc {
    const double *cols;   // [7][nseg] or nullptr (the slot has no track)
    int32_t nseg, closed;
    double L;             // total length (the closing segment included when closed)
};
enum TrackCol { kTrkAx = 0, kTrkAy, kTrkDx, kTrkDy, kTrkL2, kTrkLen, kTrkCum };

// what one projection pass reads and writes.  Step forms: agents [begin, begin + count), slot = env_map[i / A] (slot 0 when
// env_map is nullptr).  Unit form: poses [count][3], the track `unit_slot`, out [count][5].
struct TrackJob {
    const TrackDesc *tracks;
    const int32_t *env_map;
    int32_t A, begin, count, unit_slot;
    const double *px, *py, *pth;   // pose columns, `stride` apart per agent
    int32_t stride, pad_;
    double *s, *ds, *lat, *head;   // [N] (post-step form)
    int32_t *seg;                  // [N]
    double *c_s, *c_x, *c_y;       // [N] cache: s and the pose it belongs to
    int32_t *c_ok;                 // [N] the cache entry is valid (cleared by f110_track_set / f110_set_env_maps / state loads)
    const int32_t *hint;           // [N] segment of the agent's last projection (a pruning seed, any value is safe), or nullptr
    double *unit_out;              // [count][5]: s, lateral, heading_error, segment, t
};
enum TrackMode { kTrackHead = 0, kTrackPost = 1, kTrackUnit = 2 };
constexpr int kTrackLanes = 16;
constexpr int kTrackLdsSegs = 1024;   // 48 KB of LDS: ax, ay, dx, dy, l2, len per segment
constexpr int kTrackLdsCols = 6;
constexpr double kTrackPruneMargin = 1e-6;

__device__ __forceinline__ uint64_t track_bits(double v) { return (uint64_t)__double_as_longlong(v); }

// wrap(theta - atan2(dy, dx)) into [-pi, pi)
__device__ __forceinline__ double track_wrap_angle(double e)
{
    const double two_pi = 2.0 * M_PI;
    double w = fmod(e + M_PI, two_pi);
    if (w < 0.0) w += two_pi;
    if (w >= two_pi) w -= two_pi;
    return w - M_PI;
}

template <int MODE, bool LDS>
__global__ void __launch_bounds__(256) k_track_project(TrackJob j)
{
    __shared__ double s_tab[LDS ? kTrackLdsCols * kTrackLdsSegs : 1];
    __shared__ int s_slot, s_staged;
    const int gid = (blockIdx.x * blockDim.x + threadIdx.x) / kTrackLanes;
    const int sub = threadIdx.x & (kTrackLanes - 1);
    const bool live = gid < j.count;
    const int g = live ? gid : j.count - 1;   // idle groups shadow the last agent so the wave stays convergent
    const int i = MODE == kTrackUnit ? g : j.begin + g;
    const int slot = MODE == kTrackUnit ? j.unit_slot : (j.env_map ? j.env_map[i / j.A] : 0);
    const TrackDesc td = j.tracks[slot];
    const double px = j.px[(size_t)i * j.stride], py = j.py[(size_t)i * j.stride];
    // the head pass re-projects only agents whose pose changed bitwise since their cached s
    bool work = live && td.nseg > 0;
    if (MODE == kTrackHead && work)
        work = !(j.c_ok[i] && track_bits(j.c_x[i]) == track_bits(px) && track_bits(j.c_y[i]) == track_bits(py));
    if (LDS) {
        // stage the track of the workgroup's first agent when it fits (and, in the head pass, when somebody needs it)
        if (threadIdx.x == 0) s_slot = slot;
        const int any = __syncthreads_or(work ? 1 : 0);
        const TrackDesc t0 = j.tracks[s_slot];
        const bool stage = any && t0.nseg > 0 && t0.nseg <= kTrackLdsSegs;
        if (stage) {
            for (int q = threadIdx.x; q < kTrackLdsCols * t0.nseg; q += blockDim.x) {
                const int c = q / t0.nseg, k = q - c * t0.nseg;
                s_tab[c * kTrackLdsSegs + k] = t0.cols[(size_t)c * t0.nseg + k];
            }
        }
        if (threadIdx.x == 0) s_staged = stage ? 1 : 0;
        __syncthreads();
    }
    if (!work) {
        if (MODE == kTrackPost && live && sub == 0) {   // (no track on this slot: f110_step refuses it, so this is never read)
            j.s[i] = j.ds[i] = j.lat[i] = j.head[i] = NAN;
            j.seg[i] = -1;
        }
        return;
    }
    const bool from_lds = LDS && s_staged && slot == s_slot;
    const double *src = td.cols;
    size_t cs = (size_t)td.nseg;
    if (LDS && from_lds) {
        src = s_tab;
        cs = kTrackLdsSegs;
    }
    // ---- nearest_point_on_trajectory (examples/waypoint_follow.py:15-50), f110_math.hpp's arithmetic
    double dist = INFINITY, tb = 0.0, seed = INFINITY;
    int best = 0x7fffffff;
    if (j.hint) {   // the last winner's distance: an upper bound of the minimum (NaN for a NaN pose: then nothing is skipped)
        int k = j.hint[i];
        k = k < 0 ? 0 : (k >= td.nseg ? td.nseg - 1 : k);
        const double ax = src[k], ay = src[cs + k], dx = src[2 * cs + k], dy = src[3 * cs + k], l2 = src[4 * cs + k];
        double t = ((px - ax) * dx + (py - ay) * dy) / l2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double rx = px - (ax + t * dx), ry = py - (ay + t * dy);
        seed = sqrt(rx * rx + ry * ry);
    }
    for (int k = sub; k < td.nseg; k += kTrackLanes) {
        const double ax = src[k], ay = src[cs + k], dx = src[2 * cs + k], dy = src[3 * cs + k];
        const double mx = px - (ax + 0.5 * dx), my = py - (ay + 0.5 * dy);
        const double reach = (seed < dist ? seed : dist) + 0.5 * src[5 * cs + k] + kTrackPruneMargin;
        if (mx * mx + my * my > reach * reach) continue;
        const double l2 = src[4 * cs + k];
        double t = ((px - ax) * dx + (py - ay) * dy) / l2;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double rx = px - (ax + t * dx), ry = py - (ay + t * dy);
        const double d = sqrt(rx * rx + ry * ry);
        if (d < dist) {
            dist = d;
            tb = t;
            best = k;
        }
    }
#pragma unroll
    for (int m = 1; m < kTrackLanes; m <<= 1) {
        const double od = __shfl_xor(dist, m, kTrackLanes), ot = __shfl_xor(tb, m, kTrackLanes);
        const int ob = __shfl_xor(best, m, kTrackLanes);
        if (od < dist || (od == dist && ob < best)) {
            dist = od;
            tb = ot;
            best = ob;
        }
    }
    if (sub != 0) return;
    const size_t n = (size_t)td.nseg;
    const double *c = td.cols;
    if (best == 0x7fffffff) {   // no distance below +inf (every one NaN for a NaN pose): np.argmin -> 0, with segment 0's own t and
        best = 0;               // distance, as the reference returns them (its clip passes NaN through)
        const double dx = c[2 * n], dy = c[3 * n];
        double t = ((px - c[0]) * dx + (py - c[n]) * dy) / c[4 * n];
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
        const double rx = px - (c[0] + t * dx), ry = py - (c[n] + t * dy);
        tb = t;
        dist = sqrt(rx * rx + ry * ry);
    }
    const double ax = c[best], ay = c[n + best], dx = c[2 * n + best], dy = c[3 * n + best];
    const double s = c[6 * n + best] + tb * c[5 * n + best];
    if (MODE == kTrackHead) {
        j.c_s[i] = s;
        j.c_x[i] = px;
        j.c_y[i] = py;
        j.c_ok[i] = 1;
        return;
    }
    const double rx = px - (ax + tb * dx), ry = py - (ay + tb * dy);
    const double cross = dx * ry - dy * rx;
    const double lat = cross < 0.0 ? -dist : dist;
    const double theta = j.pth[(size_t)i * j.stride];
    const double herr = track_wrap_angle(theta - atan2(dy, dx));
    if (MODE == kTrackUnit) {
        double *o = j.unit_out + 5 * (size_t)i;
        o[0] = s;
        o[1] = lat;
        o[2] = herr;
        o[3] = (double)best;
        o[4] = tb;
        return;
    }
    double d = s - j.c_s[i];   // the head pass left the cache valid for the pose this step started from
    if (td.closed) {
        const double half = 0.5 * td.L;
        if (d > half) d -= td.L;
        else if (d <= -half) d += td.L;
    }
    j.s[i] = s;
    j.ds[i] = d;
    j.lat[i] = lat;
    j.head[i] = herr;
    j.seg[i] = best;
    j.c_s[i] = s;
    j.c_x[i] = px;
    j.c_y[i] = py;
    j.c_ok[i] = 1;
}


// ---- exact snapshot / restore / clone of the simulator state (f110_state_*, f110_clone_envs_device) ----------------------------
// The host lists every column a step or the episode logic reads (StateCols, built by state_columns in f110_hip.hip).  A column is
// items of `bytes` bytes, `per_env` items per env (A: a per-agent column, 1: a per-env one), item i of the live column at
// live + i * bytes.  In a blob each column is one section [k * per_env][bytes] starting at `off`, so the threads of a wave move
// consecutive items (or consecutive 16-byte words of one wide item, the scans) — coalesced on both sides.  One routine serves
// the three directions: live env -> blob entry (pack), blob entry -> live env (unpack), live env -> live env (clone).
constexpr int kStateMaxCols = 40;   // (StateCols is a kernel argument: 40 x 32 bytes; state_columns uses at most 33)
constexpr uint32_t kStateColRngShared = 1;   // rng_state in the shared-stream mode (see k_state_pack)
struct StateCol {
    char *live;
    uint64_t off;
    uint32_t bytes, per_env;
    uint32_t kind, pad;
};
struct StateCols {
    StateCol c[kStateMaxCols];
    int32_t n, num_envs;
    const int32_t *step_count;   // kStateColRngShared: the live step counters ...
    const U128 *rowstate;        // ... the row cache's start states [noise_rows + 1] ...
    int32_t noise_rows, pad;     // ... and its capacity
};

// the 256 bytes at the start of every blob (include/f110.h documents the fields; f1tenth_gym_amd/core.py StateBlob parses them)
struct StateHeader {
    char magic[8];          // "F110SNAP"
    uint32_t version;
    int32_t k, A, B, flags;
    uint32_t cols;          // F110_STATE_COL_* present
    int32_t noise_mode, noise_rows, n_maps, ego_idx;
    int64_t max_step;       // upper bound of every step_count in the blob
    uint64_t noise_id[4];
    double std_dev;
    uint64_t total_bytes;
    uint64_t reserved[19];
};
static_assert(sizeof(StateHeader) == 256, "the blob header is 256 bytes");

template <bool SRC_LIVE, bool DST_LIVE>
__device__ __forceinline__ void state_copy(const StateCols &cols, const char *__restrict__ blob_src, char *__restrict__ blob_dst,
                                           const int32_t *__restrict__ src_idx, const int32_t *__restrict__ dst_idx, int k, int src_lim,
                                           int32_t *status)
{
    const int ci = (int)blockIdx.y;
    if (ci >= cols.n) return;
    const StateCol c = cols.c[ci];
    const uint32_t unit = (c.bytes & 15u) == 0u ? 16u : ((c.bytes & 7u) == 0u ? 8u : ((c.bytes & 3u) == 0u ? 4u : 1u));
    const uint32_t upi = c.bytes / unit;                 // units per item
    const uint64_t upe = (uint64_t)upi * c.per_env;      // units per index-list entry
    const uint64_t total = upe * (uint64_t)k;
    const int E = cols.num_envs;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < total; u += (uint64_t)gridDim.x * blockDim.x) {
        const int j = (int)(u / upe);
        const uint64_t r = u - (uint64_t)j * upe;
        const uint32_t s = (uint32_t)(r / upi), w = (uint32_t)(r - (uint64_t)s * upi);
        const int se = src_idx ? src_idx[j] : j;
        const int de = dst_idx ? dst_idx[j] : j;
        const bool ok = se >= 0 && se < src_lim && (!DST_LIVE || (de >= 0 && de < E));
        if (!ok) {   // skipped, counted once per entry
            if (ci == 0 && r == 0 && status) atomicAdd(status, 1);
            continue;
        }
        const uint64_t si = (uint64_t)se * c.per_env + s, di = (uint64_t)de * c.per_env + s;
        const char *src = SRC_LIVE ? c.live + si * c.bytes : blob_src + c.off + si * c.bytes;
        char *dst = DST_LIVE ? c.live + di * c.bytes : blob_dst + c.off + di * c.bytes;
        src += (uint64_t)w * unit;
        dst += (uint64_t)w * unit;
        if (SRC_LIVE && !DST_LIVE && c.kind == kStateColRngShared) {
            // the shared stream: an agent still inside the row cache never advanced its own state, so the blob gets the stream
            // position of its next row from the cache's start states — a canonical value whatever cache size the target has
            const int32_t n = cols.step_count[si];
            if (n >= 0 && n <= cols.noise_rows) src = reinterpret_cast<const char *>(cols.rowstate + n);
        }
        switch (unit) {
        case 16: *reinterpret_cast<uint4 *>(dst) = *reinterpret_cast<const uint4 *>(src); break;
        case 8: *reinterpret_cast<uint2 *>(dst) = *reinterpret_cast<const uint2 *>(src); break;
        case 4: *reinterpret_cast<uint32_t *>(dst) = *reinterpret_cast<const uint32_t *>(src); break;
        default: *dst = *src; break;
        }
    }
}

// live env env_idx[j] (env j when env_idx is null) -> blob entry j; the first workgroup also stores the header
__global__ void __launch_bounds__(256) k_state_pack(StateCols cols, StateHeader hdr, const int32_t *__restrict__ env_idx, int k, char *__restrict__ blob,
                                                    int32_t *status)
{
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < sizeof(StateHeader) / 8)
        reinterpret_cast<uint64_t *>(blob)[threadIdx.x] = reinterpret_cast<const uint64_t *>(&hdr)[threadIdx.x];
    state_copy<true, false>(cols, nullptr, blob, env_idx, nullptr, k, cols.num_envs, status);
}

// blob entry src[j] (j when src is null) -> live env dst[j]; several dst may name one src
__global__ void __launch_bounds__(256) k_state_unpack(StateCols cols, const char *__restrict__ blob, int blob_k, const int32_t *__restrict__ src,
                                                      const int32_t *__restrict__ dst, int k, int32_t *status)
{
    state_copy<false, true>(cols, blob, nullptr, src, dst, k, blob_k, status);
}

// live env src[j] -> live env dst[j] in one launch (src and dst disjoint, no dst twice: the host checks host-side index lists)
__global__ void __launch_bounds__(256) k_clone_envs(StateCols cols, const int32_t *__restrict__ src, const int32_t *__restrict__ dst, int k,
                                                    int32_t *status)
{
    state_copy<true, true>(cols, nullptr, nullptr, src, dst, k, cols.num_envs, status);
}

// ---- rendering (f110_render_device) -----------------------------------------------------------------------------------------
// rendering.py's scene (map points, one quad per car) as a class image, one uint8 per pixel; include/f110.h states the rules.
// k_render_setup turns the spec into one record per frame (centre, cos / sin of the camera angle, env, slot) and one per agent
// (get_vertices' corners and their bounding box), so no pixel evaluates trigonometry.  k_render_raster classifies MAP and CARS:
// one workgroup covers part of one frame (the records are wave-uniform: scalar loads), each lane 4 adjacent pixels of a row, one
// 32-bit store.  The map test reads a per-slot byte grid (1 where dt == 0), 8x smaller than the float64 table.  k_render_points
// then scatters TRACK points and SCAN hits (two ordered launches); a point overwrites only a lower class, so the only concurrent
// writes to one byte store the same value.  k_render_finish writes the palette image (and the caller's class buffer when the
// raster wrote into an aligned staging copy).
struct RenderSlot {
    const uint8_t *occ;    // [height][width] 1 where the distance table is 0
    const double *pts;     // [npts][2] the slot's track points (nullptr: no track)
    int32_t height, width, npts, pad_;
    double res, inv_res, orig_x, orig_y, orig_c, orig_s, w_res, h_res;
};
struct RenderFrame {
    double cx, cy, c, s;
    int32_t env, slot, self, valid;   // valid = 0: a FOLLOW / EGO camera on an agent with a non-finite pose (all OUTSIDE)
};
struct RenderCar {
    double v[8];      // box_vertices: [rl, rr, fr, fl] (x, y)
    double bb[4];     // xmin, xmax, ymin, ymax, widened by kRenderBoxSlack
    int32_t draw, pad_[3];
};
constexpr double kRenderBoxSlack = 1e-6;   // the box test proper decides; the bounding box only skips cars far from a pixel

struct RenderJob {
    const double *snap;         // [3][N] Simulator.agent_poses
    const double *params;       // [A][18] or [N][18]
    const int32_t *env_map;     // [E] or nullptr (every env on slot 0)
    const RenderSlot *slots;
    const int32_t *agents;      // [F] camera agents, or nullptr (frame f = agent f)
    RenderFrame *frames;        // [F]
    RenderCar *cars;            // [N]
    uint8_t *cls;               // [F][H][pitch]
    const double *scans;        // [N][B]
    int32_t F, N, A, W, H, pitch, view, layers, params_per_agent, B;
    uint32_t words_per_frame, blocks_per_frame;   // raster: pitch / 4 * H, its workgroups
    double mpp, center_x, center_y, angle, fwd, car_len, car_wid, lidar_dist;
    double cull_r;   // the frame's half-diagonal plus a pixel and 1 %: a point farther from the centre lands in no pixel
};

__device__ __forceinline__ bool render_finite(double x, double y, double t) { return isfinite(x) && isfinite(y) && isfinite(t); }

// lanes [0, F): the frame records; lanes [0, N): the car records
__global__ void __launch_bounds__(256) k_render_setup(RenderJob j)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N = (size_t)j.N;
    if (t < j.F) {
        const int n = j.agents ? j.agents[t] : t;
        const int e = n / j.A;
        RenderFrame fr;
        fr.env = e;
        fr.slot = j.env_map ? j.env_map[e] : 0;
        fr.self = n;
        fr.valid = 1;
        const double x = j.snap[n], y = j.snap[N + n], th = j.snap[2 * N + n];
        if (j.view == 0) {
            fr.cx = j.center_x;
            fr.cy = j.center_y;
            cos_sin(j.angle, fr.c, fr.s);
        } else {
            double ch, sh;
            cos_sin(th, ch, sh);
            fr.cx = x + j.fwd * ch;
            fr.cy = y + j.fwd * sh;
            if (j.view == 1) {
                fr.c = 1.0;
                fr.s = 0.0;
            } else {
                cos_sin(th - kPi / 2, fr.c, fr.s);
            }
            if (!render_finite(x, y, th)) fr.valid = 0;
        }
        j.frames[t] = fr;
    }
    if (t < j.N) {
        RenderCar car;
        const double x = j.snap[t], y = j.snap[N + t], th = j.snap[2 * N + t];
        const double *p = j.params + (size_t)(j.params_per_agent ? t : t % j.A) * NPARAMS;
        const bool over = j.car_len > 0.0 && j.car_wid > 0.0;
        box_vertices(x, y, th, over ? j.car_len : p[P_LENGTH], over ? j.car_wid : p[P_WIDTH], car.v);
        car.draw = render_finite(x, y, th) ? 1 : 0;
        double x0 = car.v[0], x1 = car.v[0], y0 = car.v[1], y1 = car.v[1];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            x0 = fmin(x0, car.v[2 * q]);
            x1 = fmax(x1, car.v[2 * q]);
            y0 = fmin(y0, car.v[2 * q + 1]);
            y1 = fmax(y1, car.v[2 * q + 1]);
        }
        car.bb[0] = x0 - kRenderBoxSlack;
        car.bb[1] = x1 + kRenderBoxSlack;
        car.bb[2] = y0 - kRenderBoxSlack;
        car.bb[3] = y1 + kRenderBoxSlack;
        car.pad_[0] = car.pad_[1] = car.pad_[2] = 0;
        j.cars[t] = car;
    }
}

// int(v / res) of xy_2_rc :83-84 (cell_index's rule: the reciprocal decides unless the quotient is within 1e-9 of an integer)
__device__ __forceinline__ int render_cell(double v, double res, double inv_res, int n)
{
    const double q = v * inv_res;
    int ci = (int)q;
    const double fr = q - (double)ci;
    if (fr < 1e-9 || fr > 1.0 - 1e-9) ci = (int)(v / res);
    return ci < n ? ci : n - 1;   // (v < n * res rounded can still divide to n)
}

__device__ __forceinline__ int render_pixel(const RenderJob &j, const RenderFrame &fr, const RenderSlot &ms, double x, double y)
{
    int cls = 1;   // FREE (also what MAP off leaves)
    if (j.layers & F110_LAYER_MAP) {
        const double xt = x - ms.orig_x, yt = y - ms.orig_y;
        const double xr = xt * ms.orig_c + yt * ms.orig_s;
        const double yr = -xt * ms.orig_s + yt * ms.orig_c;
        const bool inside = (xr >= 0) & (xr < ms.w_res) & (yr >= 0) & (yr < ms.h_res);
        cls = 0;
        if (inside) {
            const int c = render_cell(xr, ms.res, ms.inv_res, ms.width), r = render_cell(yr, ms.res, ms.inv_res, ms.height);
            cls = ms.occ[(size_t)r * ms.width + c] ? 2 : 1;
        }
    }
    if (j.layers & F110_LAYER_CARS) {
        const int a0 = fr.env * j.A;
        for (int a = 0; a < j.A; ++a) {
            const RenderCar &car = j.cars[a0 + a];
            if (!car.draw || x < car.bb[0] || x > car.bb[1] || y < car.bb[2] || y > car.bb[3]) continue;
            bool in = true;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int q1 = (q + 1) & 3;
                const double ax = car.v[2 * q], ay = car.v[2 * q + 1], bx = car.v[2 * q1], by = car.v[2 * q1 + 1];
                in = in && ((bx - ax) * (y - ay) - (by - ay) * (x - ax) >= 0.0);
            }
            if (in) {
                const int k = (a0 + a == fr.self) ? 6 : 5;
                cls = k > cls ? k : cls;
            }
        }
    }
    return cls;
}

// MAP and CARS: lane = 4 adjacent pixels of one row of one frame (pitch % 4 == 0; pixels j >= W are padding, left 0)
__global__ void __launch_bounds__(256) k_render_raster(RenderJob j)
{
    const uint32_t f = blockIdx.x / j.blocks_per_frame;
    const uint32_t w = (blockIdx.x - f * j.blocks_per_frame) * blockDim.x + threadIdx.x;
    if (w >= j.words_per_frame) return;
    const uint32_t wpr = (uint32_t)j.pitch >> 2;
    const int i = (int)(w / wpr), j0 = (int)(w - (uint32_t)i * wpr) * 4;
    const RenderFrame fr = j.frames[f];
    uint32_t word = 0;
    if (fr.valid) {
        const RenderSlot ms = j.slots[fr.slot];
        const double v = ((double)j.H * 0.5 - ((double)i + 0.5)) * j.mpp;
        const double vs = v * fr.s, vc = v * fr.c;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (j0 + q >= j.W) break;
            const double u = (((double)(j0 + q) + 0.5) - (double)j.W * 0.5) * j.mpp;
            const double x = fr.cx + (u * fr.c - vs);
            const double y = fr.cy + (u * fr.s + vc);
            word |= (uint32_t)render_pixel(j, fr, ms, x, y) << (8 * q);
        }
    }
    *reinterpret_cast<uint32_t *>(j.cls + ((size_t)f * j.H + i) * j.pitch + j0) = word;
}

// TRACK (SCAN = false: lane = (frame, track point)) or SCAN (lane = (frame, beam)) points into the class image
template <bool SCAN>
__global__ void __launch_bounds__(256) k_render_points(RenderJob j, ScanConst k, uint32_t per_frame)
{
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)j.F * per_frame) return;
    const int f = (int)(t / per_frame), p = (int)(t - (size_t)f * per_frame);
    const RenderFrame fr = j.frames[f];
    if (!fr.valid) return;
    double px, py;
    if (SCAN) {
        const size_t N = (size_t)j.N;
        const int n = fr.self;
        const double r = j.scans[(size_t)n * j.B + p];
        if (!(r < k.max_range)) return;
        double st[5] = {j.snap[n], j.snap[N + n], 0.0, 0.0, j.snap[2 * N + n]};
        double sp[3];
        const bool on_axle = j.lidar_dist == 0.0 && fabs(st[4]) < 1e300 && !(st[0] == 0.0 && signbit(st[0])) && !(st[1] == 0.0 && signbit(st[1]));
        if (on_axle) {   // fan_finish's lidar pose (base_classes.py:407-409)
            sp[0] = st[0];
            sp[1] = st[1];
        } else {
            double ch, sh;
            cos_sin(st[4], ch, sh);
            sp[0] = st[0] + j.lidar_dist * ch;
            sp[1] = st[1] + j.lidar_dist * sh;
        }
        sp[2] = st[4];
        if (!render_finite(sp[0], sp[1], sp[2])) return;
        const double ox = sp[0] - fr.cx, oy = sp[1] - fr.cy;
        if (!(r <= sqrt(ox * ox + oy * oy) + j.cull_r)) return;   // the hit is beyond the frame whatever the beam's direction
        const double2 cs = k.cs[beam_dir_index(k, scan_start_index(k, sp[2]), p)];
        px = sp[0] + r * cs.x;
        py = sp[1] + r * cs.y;
    } else {
        const RenderSlot ms = j.slots[fr.slot];
        if (p >= ms.npts) return;
        px = ms.pts[2 * p];
        py = ms.pts[2 * p + 1];
    }
    const double dx = px - fr.cx, dy = py - fr.cy;
    if (!(dx * dx + dy * dy <= j.cull_r * j.cull_r)) return;   // (NaN included) before the divisions
    const double up = dx * fr.c + dy * fr.s, vp = -dx * fr.s + dy * fr.c;
    const double fi = floor((double)j.H * 0.5 - vp / j.mpp), fj = floor(up / j.mpp + (double)j.W * 0.5);
    if (!(fi >= 0.0 && fi < (double)j.H && fj >= 0.0 && fj < (double)j.W)) return;
    uint8_t *dst = j.cls + ((size_t)f * j.H + (size_t)fi) * j.pitch + (size_t)fj;
    const uint8_t cls = SCAN ? 4 : 3;
    if (*dst < cls) *dst = cls;
}

struct RenderPalette {
    uint8_t rgb[F110_NCLASSES * 3];
    uint8_t pad_[11];
};

// pixel -> rgb = palette[class] (rgb != nullptr), and the staged classes (row pitch `pitch`) into the caller's dense buffer
__global__ void __launch_bounds__(256) k_render_finish(const uint8_t *__restrict__ staged, int pitch, int W, int H, size_t total,
                                                       uint8_t *__restrict__ cls, uint8_t *__restrict__ rgb, RenderPalette pal)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= total) return;
    const size_t row = q / (size_t)W, col = q - row * (size_t)W;
    uint8_t c = staged[row * (size_t)pitch + col];
    if (c >= F110_NCLASSES) c = 0;
    if (cls) cls[q] = c;
    if (rgb) {
        rgb[3 * q] = pal.rgb[3 * c];
        rgb[3 * q + 1] = pal.rgb[3 * c + 1];
        rgb[3 * q + 2] = pal.rgb[3 * c + 2];
    }
    (void)H;
}

// the per-slot occupancy grid: 1 where the distance table holds 0 (the cells rays stop in)
__global__ void __launch_bounds__(256) k_render_occ(const double *__restrict__ table, int row_bytes, int H, int W, uint8_t *__restrict__ occ)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= (size_t)H * W) return;
    const size_t r = q / (size_t)W, c = q - r * (size_t)W;
    const double d = *reinterpret_cast<const double *>(reinterpret_cast<const char *>(table) + r * (size_t)row_bytes + c * 8);
    occ[q] = d == 0.0 ? 1 : 0;
}

// ---- randomised start poses (f110_reset_sampler_*) -----------------------------------------------------------
// One lane per env.  Env e owns the PCG64 stream {state, inc} = stream[2e], stream[2e + 1]; a uniform is NumPy's
// Generator.random() (pcg_to_double of the next output).  An attempt draws s0 = L (s_lo + u (s_hi - s_lo)) and, per agent j,
// (u_l, u_h): agent j sits j gap behind s0, d = lateral (2 u_l - 1) to the left of its segment, heading jitter h = heading (2 u_h - 1).
// The candidate poses are staged in cand [N][3]; the attempt is valid when every agent is on the track (open: s >= 0), in
// bounds of its slot's table with dt >= clearance, and every pair of agents is 2 clearance apart.  Which envs draw is the mode:
enum SampleMode {
    kSampleExplicit = 0,   // f110_reset_sample: envs of `mask` (nullptr: all); the result goes to out_poses / out_rot for k_reset
    kSampleMarker = 1,     // behind a step that re-seats: envs whose first agent has step_count 0 (only a re-seat sets it there)
    kSampleCollided = 2,   // behind f110_reset_collided_device: envs whose ego (`ego`) has collisions != 0
    kSampleDone = 3        // behind k_episode_reset_done: envs whose done flag is still set
};
struct SamplerJob {
    const TrackDesc *tracks;   // [slots] (f110_track_set)
    const int32_t *env_map;    // [E] or nullptr (slot 0)
    const ScanConst *maps;     // [slots] with env_map, else [1]
    U128 *stream;              // [E][2] {state, inc}
    double *last;              // [N][3] poses of the env's last reset (host or drawn): the explicit fallback
    double *cand;              // [N][3] scratch
    double *out_poses;         // [N][3] explicit: what the reset gets
    double *out_rot;           // [E][4] explicit: start_rot of the ego's pose
    int32_t *attempt;          // [E] winning attempt of the env's last draw, -1 = fallback
    unsigned long long *counters;   // [2] draws, fallbacks
    const uint8_t *mask;       // kSampleExplicit: [E] or nullptr
    double s_lo, s_hi, gap, lateral, heading, clearance;
    int32_t attempts, A, ego, mode;
};

__device__ __forceinline__ double sampler_uniform(U128 &st, U128 inc)
{
    st = pcg_step(st, inc);
    return pcg_to_double(pcg_output(st));
}

// start_rot (f110_env.py:331) of heading theta, row-major
__device__ __forceinline__ void sampler_rot(double theta, double *r)
{
    const double c = cos(-theta), s = sin(-theta);
    r[0] = c;
    r[1] = -s;
    r[2] = s;
    r[3] = c;
}

// envs [e0, e0 + count)
__global__ void __launch_bounds__(256) k_reset_sample(SamplerJob j, AgentArrays a, EpisodeArrays ep, int has_ep, int e0, int count)
{
    const int e = e0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    const int N = a.n_agents_total, A = j.A;
    const bool live = e < e0 + count;
    bool drew = false, fell = false;
    if (live) {
        const int i0 = e * A;
        if (j.mode == kSampleExplicit) drew = !j.mask || j.mask[e];
        else if (j.mode == kSampleMarker) drew = a.step_count[i0] == 0;
        else if (j.mode == kSampleCollided) drew = a.collisions[i0 + j.ego] != 0.0;
        else drew = ep.done[e] != 0;
    }
    if (drew) {
        const int i0 = e * A;
        const int slot = j.env_map ? j.env_map[e] : 0;
        const TrackDesc td = j.tracks[slot];
        const ScanConst &k = j.maps[j.env_map ? slot : 0];
        const int nseg = td.nseg;
        const double *ax = td.cols + (size_t)kTrkAx * nseg, *ay = td.cols + (size_t)kTrkAy * nseg;
        const double *dxs = td.cols + (size_t)kTrkDx * nseg, *dys = td.cols + (size_t)kTrkDy * nseg;
        const double *len = td.cols + (size_t)kTrkLen * nseg, *cum = td.cols + (size_t)kTrkCum * nseg;
        const double L = td.L, need2 = (2.0 * j.clearance) * (2.0 * j.clearance);
        U128 st = j.stream[2 * (size_t)e];
        const U128 inc = j.stream[2 * (size_t)e + 1];
        int won = -1;
        for (int att = 0; att < j.attempts && won < 0; ++att) {
            const double s0 = L * (j.s_lo + sampler_uniform(st, inc) * (j.s_hi - j.s_lo));
            bool ok = true;
            for (int q = 0; q < A; ++q) {
                double s = s0 - (double)q * j.gap;
                if (td.closed) {
                    s = fmod(s, L);
                    if (s < 0.0) s += L;
                }
                const double ul = sampler_uniform(st, inc), uh = sampler_uniform(st, inc);
                const double d = j.lateral * (2.0 * ul - 1.0), hj = j.heading * (2.0 * uh - 1.0);
                int lo = 0, hi = nseg - 1;   // the last segment with cum[k] <= s (0 when none)
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (cum[mid] <= s) lo = mid;
                    else hi = mid - 1;
                }
                const int sk = lo;
                double t = (s - cum[sk]) / len[sk];
                t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
                const double sdx = dxs[sk], sdy = dys[sk], sl = len[sk];
                const double x = (ax[sk] + t * sdx) + d * (-sdy / sl);
                const double y = (ay[sk] + t * sdy) + d * (sdx / sl);
                const double th = atan2(sdy, sdx) + hj;
                const size_t i = (size_t)i0 + q;
                j.cand[3 * i] = x;
                j.cand[3 * i + 1] = y;
                j.cand[3 * i + 2] = th;
                int r, c;
                const double dist = sample_distance<LAYOUT_ROWMAJOR, false, false>(k, nullptr, x, y, r, c);
                ok = ok && (td.closed || s >= 0.0) && r >= 0 && dist >= j.clearance;
            }
            for (int p = 0; p < A && ok; ++p)
                for (int q = p + 1; q < A && ok; ++q) {
                    const size_t ip = (size_t)i0 + p, iq = (size_t)i0 + q;
                    const double ddx = j.cand[3 * ip] - j.cand[3 * iq], ddy = j.cand[3 * ip + 1] - j.cand[3 * iq + 1];
                    ok = ddx * ddx + ddy * ddy >= need2;
                }
            if (ok) won = att;
        }
        j.stream[2 * (size_t)e] = st;
        j.attempt[e] = won;
        fell = won < 0;
        if (j.mode == kSampleExplicit) {
            // the reset gets the drawn poses, or (fallback) the poses of the env's last reset
            const double *src = fell ? j.last : j.cand;
            for (int q = 0; q < A; ++q) {
                const size_t i = (size_t)i0 + q;
                for (int c = 0; c < 3; ++c) j.out_poses[3 * i + c] = src[3 * i + c];
                if (!fell)
                    for (int c = 0; c < 3; ++c) j.last[3 * i + c] = j.cand[3 * i + c];
            }
            sampler_rot(src[3 * ((size_t)i0 + ep.ego_idx) + 2], j.out_rot + 4 * (size_t)e);
        } else if (!fell) {
            // the re-seat already zeroed the state: its pose columns become the drawn poses
            for (int q = 0; q < A; ++q) {
                const size_t i = (size_t)i0 + q;
                const double x = j.cand[3 * i], y = j.cand[3 * i + 1], th = j.cand[3 * i + 2];
                a.state[i] = x;
                a.state[(size_t)N + i] = y;
                a.state[4 * (size_t)N + i] = th;
                j.last[3 * i] = x;
                j.last[3 * i + 1] = y;
                j.last[3 * i + 2] = th;
                if (has_ep) {
                    ep.start_poses[3 * i] = x;
                    ep.start_poses[3 * i + 1] = y;
                    ep.start_poses[3 * i + 2] = th;
                }
            }
            if (has_ep) sampler_rot(j.cand[3 * ((size_t)i0 + ep.ego_idx) + 2], ep.rot + 4 * (size_t)e);
        }
    }
    const unsigned long long bd = __ballot(drew), bf = __ballot(fell);
    if ((threadIdx.x & 63u) == 0u && bd) {
        atomicAdd(&j.counters[0], (unsigned long long)__popcll(bd));
        if (bf) atomicAdd(&j.counters[1], (unsigned long long)__popcll(bf));
    }
}

// host resets while a sampler is armed: the masked envs' poses become their explicit-draw fallback
__global__ void k_sampler_keep(double *__restrict__ last, const double *__restrict__ poses, const uint8_t *__restrict__ env_mask, int N, int A)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N || (env_mask && !env_mask[i / A])) return;
    for (int c = 0; c < 3; ++c) last[3 * (size_t)i + c] = poses[3 * (size_t)i + c];
}

// ---- randomised vehicle parameters (f110_param_sampler_*; include/f110.h states the draw, f110_rng.hpp param_draw_env is it) ----
// One lane per env, k_reset_sample's pattern and its SampleMode selection.  Env e owns the PCG64 stream {state, inc} = stream[2e],
// stream[2e + 1] and the rows [e A, (e + 1) A) of the per-agent block; only drawn slots are written.  The 18 entries travel in the
// arguments; the nominal rows [A][18] (needed by relative slots only) are staged in LDS once per workgroup.
constexpr int kParamMaxAgents = 256;   // the nominal rows of an env fit LDS (36 KB)
struct ParamJob {
    ParamDist d[NPARAMS];
    const double *nominal;          // [A][18] the agent slots' sets as of arming
    double *rows;                   // [.][18] the per-agent block
    U128 *stream;                   // [E][2] {state, inc}
    unsigned long long *counter;    // envs drawn
    const uint8_t *mask;            // kSampleExplicit: [E] or nullptr
    const int32_t *step_count;      // kSampleMarker
    const double *collisions;       // kSampleCollided
    const uint8_t *done;            // kSampleDone
    const uint64_t *zk;             // the ziggurat tables
    const double *zw, *zf;
    int32_t A, ego, mode, relative;   // relative: some drawn slot multiplies the nominal
};

// envs [e0, e0 + count)
__global__ void __launch_bounds__(256) k_param_sample(ParamJob j, int e0, int count)
{
    extern __shared__ double param_nominal[];   // [A][18] when j.relative
    const int A = j.A;
    if (j.relative) {
        for (int q = (int)threadIdx.x; q < A * NPARAMS; q += (int)blockDim.x) param_nominal[q] = j.nominal[q];
        __syncthreads();
    }
    const int e = e0 + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    bool drew = false;
    if (e < e0 + count) {
        const size_t i0 = (size_t)e * A;
        if (j.mode == kSampleExplicit) drew = !j.mask || j.mask[e];
        else if (j.mode == kSampleMarker) drew = j.step_count[i0] == 0;
        else if (j.mode == kSampleCollided) drew = j.collisions[i0 + j.ego] != 0.0;
        else drew = j.done[e] != 0;
    }
    if (drew) {
        const ZigTables zt = {j.zk, j.zw, j.zf};
        U128 st = j.stream[2 * (size_t)e];
        const U128 inc = j.stream[2 * (size_t)e + 1];
        param_draw_env(j.d, param_nominal, A, st, inc, zt, j.rows + (size_t)e * A * NPARAMS);
        j.stream[2 * (size_t)e] = st;
    }
    const unsigned long long bd = __ballot(drew);
    if ((threadIdx.x & 63u) == 0u && bd) atomicAdd(j.counter, (unsigned long long)__popcll(bd));
}

// ---- compact observations (f110_obs_encode_*; include/f110.h states the rule, f110_math.hpp obs_* is the per-row arithmetic) ----
// One wave per agent, k_scan_policy's pattern: the W beams of the row go through LDS with 64-lane coalesced loads (walking the
// sectors straight from HBM touches 64 lines per instruction), then lane l takes elements l, l + 64, ... of the new frame (K above
// or below 64).  The agent's stack [F][D] is assembled in LDS as well: frames 1..F-1 are LOADED into the places of frames 0..F-2
// before anything is stored (one wave owns the agent: no race, no second buffer), the new frame goes behind them (or into all F
// places at an episode start), and the image leaves as 16-byte stores: the image sits in LDS at the agent's phase (first float
// of the stack modulo 4), so an aligned global float4 is an aligned LDS float4 whatever F * D is.
// HBM traffic per agent: 8 W (row) + 4 D (F - 1) (old frames) + 4 D F (stack) bytes.  Every load a wave needs (row, old frames,
// its lanes' features, step_count) is issued before anything waits: the old frames are fetched whether or not the agent turns out
// to start an episode (a start overwrites them in LDS), so a wave makes one trip to memory, not one per dependency.
struct ObsJob {
    ObsRowSpec rs;
    const double *scans;                 // [.][B]
    const double *fptr[kObsFeatures];    // feature j (output order) of agent i = fptr[j][i * col_stride]
    size_t col_stride;
    const int32_t *step_count;           // [.]
    float *out;                          // [.][F][D]
    int32_t B, beam_lo, F, fill;
    int32_t i0, n;                       // agents [i0, i0 + n)
    int32_t waves, wave_bytes, row_bytes;   // waves per workgroup; LDS per wave; of which the row (0: not staged)
};

template <bool STAGED>
__global__ void __launch_bounds__(256) k_obs_encode(ObsJob j)
{
    extern __shared__ double obs_lds[];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int a = (int)blockIdx.x * j.waves + wave;
    if (a >= j.n) return;
    const size_t i = (size_t)j.i0 + (size_t)a;
    const ObsRowSpec &s = j.rs;
    const int W = s.W, K = s.K, D = s.D, F = j.F;
    char *base = reinterpret_cast<char *>(obs_lds) + (size_t)wave * (size_t)j.wave_bytes;
    double *mine = reinterpret_cast<double *>(base);
    const size_t g0 = i * (size_t)F * (size_t)D;          // first float of the agent's stack
    const int phase = (int)(g0 & 3u);
    float *img = reinterpret_cast<float *>(base + j.row_bytes) + phase;
    const double *row = j.scans + i * (size_t)j.B + j.beam_lo;
    float *stack = j.out + g0;
    const bool start = obs_episode_start(j.step_count[i], j.fill);
    const int keep = (F - 1) * D;
    if (STAGED && K > 0) {
        // 16 loads in flight per lane, and the next round's loads issued before this round's LDS stores: a 1080-beam row is one
        // memory round trip (a small batch has few waves per SIMD to hide a second one behind)
        constexpr int U = 16;
        double cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = lane + 64 * u < W ? row[lane + 64 * u] : 0.;
        for (int b = lane; b < W; b += 64 * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = b + 64 * (U + u) < W ? row[b + 64 * (U + u)] : 0.;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (b + 64 * u < W) mine[b + 64 * u] = cur[u];
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }
    // frames 1..F-1 into the places of frames 0..F-2, without waiting for step_count (an episode start overwrites them below)
    if (!j.fill)
        for (int t = lane; t < keep; t += 64) img[t] = stack[t + D];
    // the lane's feature (at most one: fewer than 64 of them), loaded up front with the row, not behind the pooling
    const int ef = K + ((lane - K) & 63);
    double fx = 0., fdiv = 1.;
    if (ef < D) {
        const int f = ef - K;
        const double *p = j.fptr[0];
        fdiv = s.feat_scale[0];
#pragma unroll
        for (int c = 1; c < kObsFeatures; ++c) {   // (static indices: the job lives in kernel-argument registers)
            p = f == c ? j.fptr[c] : p;
            fdiv = f == c ? s.feat_scale[c] : fdiv;
        }
        fx = p[i * j.col_stride];
    }
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS accesses are in order; the barrier only pins the compiler)
    // the bounds of sector e = lane, lane + 64, ...: k W = q K + r, stepped by 64 W = dq K + dr per round (no division in the loop)
    int q0 = 0, r0 = 0, q1 = 0, r1 = 0, dq = 0, dr = 0;
    if (K > 0 && W < (1 << 25)) {   // (64 W fits 32 bits: the short division)
        const uint32_t w0 = (uint32_t)lane * (uint32_t)W, w1 = w0 + (uint32_t)W, ws = 64u * (uint32_t)W, k = (uint32_t)K;
        q0 = (int)(w0 / k), r0 = (int)(w0 % k), q1 = (int)(w1 / k), r1 = (int)(w1 % k), dq = (int)(ws / k), dr = (int)(ws % k);
    } else if (K > 0) {
        const long long w0 = (long long)lane * W, w1 = w0 + W, ws = 64ll * W;
        q0 = (int)(w0 / K), r0 = (int)(w0 % K), q1 = (int)(w1 / K), r1 = (int)(w1 % K), dq = (int)(ws / K), dr = (int)(ws % K);
    }
    for (int e = lane; e < D; e += 64) {
        float v;
        if (e < K) {
            v = STAGED ? obs_pool(s, mine, q0, q1) : obs_pool(s, row, q0, q1);
            q0 += dq, r0 += dr, q1 += dq, r1 += dr;
            if (r0 >= K) ++q0, r0 -= K;
            if (r1 >= K) ++q1, r1 -= K;
        } else {
            v = obs_feature(fx, fdiv);
        }
        if (start) {
            for (int f = 0; f < F; ++f) img[f * D + e] = v;
        } else {
            img[keep + e] = v;
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int total = F * D;
    int head = (4 - phase) & 3;
    head = head < total ? head : total;
    if (lane < head) stack[lane] = img[lane];
    const int nvec = (total - head) >> 2;
    for (int q = lane; q < nvec; q += 64)
        *reinterpret_cast<float4 *>(stack + head + 4 * q) = *reinterpret_cast<const float4 *>(img + head + 4 * q);
    const int tail = head + 4 * nvec;
    if (tail + lane < total) stack[tail + lane] = img[tail + lane];
}

// ---- follow the gap (f110_controllers_set / f110_follow_gap_*; include/f110.h states the rule, f110_math.hpp gap_* the arithmetic) ----
// One wave per scripted agent, k_scan_policy's pattern.  A wave whose agent is external leaves after one 4-byte load.  The W beams
// of the window go through LDS with 64-lane coalesced loads, 12 in flight per lane and the next round's issued before this
// round's LDS stores, clipped on the way in (v).  From there every pass gives lane l the beams l, l + 64, ...: consecutive lanes
// read consecutive doubles (ds_read_b64, no bank conflict), and nobody walks the window alone.
//   smooth + closest point: lane-local first minimum of p = the window mean, kept in LDS next to v; a lexicographic
//     (value, index) minimum across the wave picks np.argmin's winner
//   gap: round r's free flags are one ballot; lane r keeps it, so lane r holds the 64 beams [64 r, 64 r + 64) as a bit mask
//     (W <= 4096 = 64 lanes x 64 bits).  Its summary (runs at either end, longest run) costs as many steps as its longest run, and
//     gap_run_merge folds the 64 summaries in lane order (xor butterfly: the lane with the bit clear is the left operand)
//   target FURTHEST: the same (value, index) reduction over the gap's beams, largest value, lowest index
// LDS per wave: 16 W bytes (v and p), so the workgroup size (1..4 waves) is chosen per launch for the most waves per CU.
// HBM traffic per scripted agent: 8 W (window) + 4 (assignment) + 4 (step_count) + 16 (action) bytes, plus the spec (cached).
constexpr int kGapMaxWindow = 4096;
constexpr int kGapMaxSpecs = 8;

struct GapJob {
    const GapSpec *specs;        // device memory
    const int32_t *assign;       // [.] -1 = external, else the spec; null: spec 0 for every agent (unit form)
    const double *scans;         // [.][B]
    const int32_t *step_count;   // [.] or null (no agent is fresh)
    double *actions;             // [.][2]
    int32_t *info;               // [.][5] or null
    double fov;
    int32_t B, i0, n;            // agents [i0, i0 + n)
    int32_t waves, wave_bytes;   // waves per workgroup; LDS per wave (>= 16 W of every spec)
};

__global__ void __launch_bounds__(256) k_follow_gap(GapJob j)
{
    extern __shared__ double gap_lds[];
    const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63u);
    const int a = (int)blockIdx.x * j.waves + wave;
    if (a >= j.n) return;
    const size_t i = (size_t)j.i0 + (size_t)a;
    int k = j.assign ? j.assign[i] : 0;
    if (k < 0) return;                       // external: nothing loaded, nothing written
    k = __builtin_amdgcn_readfirstlane(k);   // (one agent per wave: the spec is read with scalar loads)
    const GapSpec s = j.specs[k];
    const int sc = j.step_count ? j.step_count[i] : 1;
    const int W = s.W;
    const double *row = j.scans + i * (size_t)j.B + s.lo;
    double *v = reinterpret_cast<double *>(reinterpret_cast<char *>(gap_lds) + (size_t)wave * (size_t)j.wave_bytes);
    double *p = v + W;
    double2 *act = reinterpret_cast<double2 *>(j.actions) + i;
    int32_t *info = j.info ? j.info + 5 * i : nullptr;
    if (sc == 0) {   // re-seated inside the step just taken: the scans are the finished episode's
        if (lane == 0) *act = make_double2(0.0, 0.0);
        if (info && lane < 5) info[lane] = -1;
        return;
    }
    {
        constexpr int U = 12;
        double cur[U], nxt[U];
#pragma unroll
        for (int u = 0; u < U; ++u) cur[u] = lane + 64 * u < W ? row[lane + 64 * u] : 0.;
        for (int b = lane; b < W; b += 64 * U) {
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[u] = b + 64 * (U + u) < W ? row[b + 64 * (U + u)] : 0.;
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (b + 64 * u < W) v[b + 64 * u] = gap_clip(cur[u], s.clip);
#pragma unroll
            for (int u = 0; u < U; ++u) cur[u] = nxt[u];
        }
    }
    __builtin_amdgcn_wave_barrier();   // (one wave: its LDS accesses are in order; the barrier only pins the compiler)
    // ---- smooth, closest point
    double best = INFINITY;
    int c = 0x7fffffff;
    for (int b = lane; b < W; b += 64) {
        const double pb = gap_window_mean(v, W, s.S, b);
        p[b] = pb;
        if (pb < best || c == 0x7fffffff) {
            best = pb;
            c = b;
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double ob = __shfl_xor(best, off);
        const int oc = __shfl_xor(c, off);
        if (ob < best || (ob == best && oc < c)) {
            best = ob;
            c = oc;
        }
    }
    const int half = gap_bubble_half(best, j.fov / (double)(j.B - 1), s.bubble, W);
    // ---- free beams: lane r keeps round r's ballot
    unsigned long long mask = 0;
    const int rounds = (W + 63) >> 6;
    for (int r = 0; r < rounds; ++r) {
        const int b = 64 * r + lane;
        const bool fr = b < W && gap_free(p[b < W ? b : 0], b, c, half, s.thresh);
        const unsigned long long m = __ballot(fr);
        if (lane == r) mask = m;
    }
    const int left = W - 64 * lane;
    GapRun run = gap_run_of_mask(mask, 64 * lane, left < 0 ? 0 : (left < 64 ? left : 64));
    if (left <= 0) run.start = W;   // (empty chunks sit at the window's end: a seam's start is read off the right operand)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        GapRun o;
        o.start = __shfl_xor(run.start, off);
        o.len = __shfl_xor(run.len, off);
        o.lead = __shfl_xor(run.lead, off);
        o.trail = __shfl_xor(run.trail, off);
        o.best = __shfl_xor(run.best, off);
        o.best_start = __shfl_xor(run.best_start, off);
        run = (lane & off) ? gap_run_merge(o, run) : gap_run_merge(run, o);
    }
    if (info && lane == 0) info[0] = c, info[1] = half;
    if (run.best == 0) {
        if (lane == 0) *act = make_double2(0.0, s.v_blocked);
        if (info && lane >= 2 && lane < 5) info[lane] = -1;
        return;
    }
    const int g0 = run.best_start, g1 = g0 + run.best;
    int t = (g0 + g1 - 1) >> 1;
    __builtin_amdgcn_wave_barrier();
    if (s.target == GAP_TARGET_FURTHEST) {
        double far = -INFINITY;
        t = 0x7fffffff;
        for (int b = g0 + lane; b < g1; b += 64) {
            const double pb = p[b];
            if (pb > far || t == 0x7fffffff) {
                far = pb;
                t = b;
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double of = __shfl_xor(far, off);
            const int ot = __shfl_xor(t, off);
            if (ot != 0x7fffffff && (t == 0x7fffffff || of > far || (of == far && ot < t))) {
                far = of;
                t = ot;
            }
        }
    }
    if (lane == 0) {
        double steer, speed;
        gap_action(s, gap_beam_angle(j.fov, j.B, s.lo + t), p[t], steer, speed);
        *act = make_double2(steer, speed);
        if (info) info[2] = g0, info[3] = g1, info[4] = t;
    }
}

// ---- track preview (f110_track_preview_*; include/f110.h states the rule, f110_math.hpp preview_* the arithmetic) ----------------
// A group of G lanes per agent, G the next power of two >= P (1..32), one station per lane; 256 / G agents per workgroup.  What a
// station costs is its dependent chain: the agent's s and pose, then ~log2(nseg) probes of the binary search on cum, then one
// round of independent loads of the winning segment's columns and attributes.  The probes are the long part, so cum — and only
// cum, 8 bytes per segment — of the workgroup's first agent's slot is staged in LDS when it has at most kPreviewLdsSegs segments
// (16 KiB; the example raceline's 782 take 6 KiB); a lane whose agent sits on another slot, or on a longer track, probes the same
// column in L2.  The rule defines k uniquely, so where the probes were served does not show.  The other columns are read once
// per station from L2, where neighbouring stations share lines.
// The agent's [P][D] floats go through LDS: lane j leaves its D values at j * D, then the group's lanes store the P * D floats in
// order, consecutive lanes consecutive floats.  The channel loop is unrolled over the eight bits, so the values stay in named
// registers (no private array indexed at run time) and the scales come from the kernel arguments.
// LDS: 16 KiB (cum) + 8 KiB (outputs) per workgroup of 4 waves.  Idle groups shadow the last agent and idle lanes the last
// station, so every lane reaches both barriers; they store nothing.
constexpr int kPreviewLdsSegs = 2048;

struct PreviewAttr {
    const double *a;   // [C][npts] or nullptr
    int32_t C, npts;
};

// device form: agents [begin, begin + count), slot = env_map[i / A] (slot 0 when env_map is nullptr), unit_slot = -1.
// unit form: rows [0, count) on the track `unit_slot`.
struct PreviewJob {
    const TrackDesc *tracks;
    const PreviewAttr *attrs;
    const int32_t *env_map;
    int32_t A, begin, count, unit_slot;
    const double *px, *py, *pth, *ps;   // pose and s columns, `stride` apart per agent
    int32_t stride, shift;              // lanes per agent = 1 << shift
    float *out;                         // [.][P][D]
    double *raw;                        // [.][P][8] or nullptr
    int32_t *seg;                       // [.][P] or nullptr
    PreviewSpec sp;
};

__global__ void __launch_bounds__(256) k_track_preview(PreviewJob j)
{
    __shared__ double s_cum[kPreviewLdsSegs];
    __shared__ float s_out[256 * PREVIEW_NCHANNELS];
    __shared__ int s_slot;
    const int P = j.sp.P, D = j.sp.D, G = 1 << j.shift;
    const int gid = (int)((blockIdx.x * 256u + threadIdx.x) >> j.shift);
    const int sub = (int)threadIdx.x & (G - 1);
    const bool live = gid < j.count;
    const int i = j.begin + (live ? gid : j.count - 1);
    const int slot = j.unit_slot >= 0 ? j.unit_slot : (j.env_map ? j.env_map[i / j.A] : 0);
    if (threadIdx.x == 0) s_slot = slot;
    __syncthreads();
    const int slot0 = s_slot;
    const TrackDesc t0 = j.tracks[slot0];
    const bool staged = t0.nseg > 0 && t0.nseg <= kPreviewLdsSegs;
    if (staged) {
        const double *cum0 = t0.cols + (size_t)kTrkCum * t0.nseg;
        for (int q = (int)threadIdx.x; q < t0.nseg; q += 256) s_cum[q] = cum0[q];
    }
    __syncthreads();
    const TrackDesc td = j.tracks[slot];
    const PreviewAttr at = j.attrs[slot];
    const bool work = live && td.nseg > 0;   // (a slot without a track is refused on the host)
    const int st = sub < P ? sub : P - 1;
    float *mine = s_out + ((int)threadIdx.x - sub) * PREVIEW_NCHANNELS;
    if (td.nseg > 0) {
        PreviewTrack tr;
        tr.cols = td.cols;
        tr.attr = at.a;
        tr.nseg = td.nseg;
        tr.closed = td.closed;
        tr.C = at.a ? at.C : 0;
        tr.npts = td.closed ? td.nseg : td.nseg + 1;
        tr.L = td.L;
        const size_t r = (size_t)i * j.stride;
        const double px = j.px[r], py = j.py[r], s = j.ps[r];
        double c = 1.0, sn = 0.0;
        if (j.sp.frame == PREVIEW_FRAME_EGO) cos_sin(j.pth[r], c, sn);
        const double sj = preview_station_s(s, j.sp.offset, j.sp.spacing, st, td.closed, td.L);
        const int k = (staged && slot == slot0) ? preview_segment(s_cum, td.nseg, sj)
                                                : preview_segment(td.cols + (size_t)kTrkCum * td.nseg, td.nseg, sj);
        double v[PREVIEW_NCHANNELS];
        preview_station(tr, k, sj, j.sp.frame, px, py, c, sn, v);
        if (work && sub < P) {
            float *o = mine + sub * D;
            int n = 0;
#pragma unroll
            for (int b = 0; b < PREVIEW_NCHANNELS; ++b)
                if (j.sp.channels >> b & 1) o[n++] = preview_scaled(v[b], j.sp.scale[b]);
            const size_t row = (size_t)i * P + sub;
            if (j.raw) {
#pragma unroll
                for (int b = 0; b < PREVIEW_NCHANNELS; ++b) j.raw[row * PREVIEW_NCHANNELS + b] = v[b];
            }
            if (j.seg) j.seg[row] = k;
        }
    }
    __syncthreads();
    if (work) {
        float *dst = j.out + (size_t)i * P * D;
        for (int q = sub; q < P * D; q += G) dst[q] = mine[q];
    }
}

// ---- neighbours (f110_neighbors_*; include/f110.h states the rule, f110_math.hpp nbr_* the arithmetic) ---------------------------
// One lane per agent, a group of G lanes per env, G the next power of two >= A (1..256); 256 / G envs per workgroup.
//  1. every lane loads its agent's columns, takes the one cos_sin and leaves (x, y, c, sn, v, s) in LDS, one column each (SoA,
//     6 x 256 doubles = 12 KiB), so that a walk over b reads consecutive doubles of one column.
//  2. every lane walks b = 0 .. A - 1 of its group: all lanes of a group read the same LDS address at the same time, which the LDS
//     serves as a broadcast; the groups of a 32-lane half read doubles G apart, on different banks.  The KT best (d2, b) stay
//     sorted in named registers (NbrBest<KT>, KT the power of two >= K: four instantiations, no register array indexed at run
//     time).
//  3. every lane re-reads its K winners' rows from LDS and evaluates the requested channels (unrolled over the ten bits, scales
//     from the kernel arguments) into an LDS stage at its agent's place in the workgroup's output, which is one contiguous region
//     of global memory (the live agents of a workgroup are consecutive); then all 256 lanes store the stage, consecutive lanes
//     consecutive floats.  An agent's row of the stage has the odd pitch K * D | 1: at a pitch of 32 or 80 floats the lanes'
//     writes would all meet on one or two banks.  The stage is 24 KiB: with the 12 KiB of columns a workgroup holds 36 KiB and
//     four of them fit a CU's 160 KiB.  A workgroup's output can be 80 KiB (256 agents x 8 slots x 10 channels), so it goes out
//     in pieces of whole agents (at most four); only the lanes of the piece evaluate, the others wait at the barrier.
// Idle lanes (G > A) shadow the env's last agent and idle groups the workgroup's last env: they reach every barrier, write their
// own LDS column slots only and store nothing.
constexpr int kNbrStageFloats = 6144;

// device form: envs [env0, env0 + envs), agent columns `stride` = 1 apart; the wrap length of GAP_S from tracks[env_map[e]] (slot 0
// when env_map is nullptr), tracks == nullptr when GAP_S is not asked for.  unit form: rows [m][5], stride 5, env0 = 0, the wrap
// length unit_L.
struct NbrJob {
    const TrackDesc *tracks;
    const int32_t *env_map;
    int32_t A, shift;                        // cars per env; lanes per env = 1 << shift
    int32_t env0, envs;
    const double *px, *py, *pth, *pv, *ps;   // ps == nullptr: s is not read (0.0)
    int32_t stride;
    double unit_L;
    float *out;                              // [.][K][D]
    double *raw;                             // [.][K][10] or nullptr
    int32_t *idx;                            // [.][K] or nullptr
    NbrSpec sp;
};

template <int KT>
__global__ void __launch_bounds__(256) k_neighbors(NbrJob j)
{
    __shared__ double s_col[6][256];
    __shared__ float s_out[kNbrStageFloats];
    const int A = j.A, G = 1 << j.shift, K = j.sp.K, D = j.sp.D, KD = K * D;
    const int tid = (int)threadIdx.x, sub = tid & (G - 1), grp = tid >> j.shift;
    const int epw = 256 >> j.shift;
    const int e_first = (int)blockIdx.x * epw;
    const int e_here = min(epw, j.envs - e_first);   // >= 1 by the grid
    const bool live = grp < e_here && sub < A;
    const int e = j.env0 + e_first + (grp < e_here ? grp : e_here - 1);
    const int a = sub < A ? sub : A - 1;
    const size_t i = (size_t)e * A + a, r = i * j.stride;
    NbrAgent me;
    me.x = j.px[r];
    me.y = j.py[r];
    cos_sin(j.pth[r], me.c, me.sn);
    me.v = j.pv[r];
    me.s = j.ps ? j.ps[r] : 0.0;
    double L = j.unit_L;
    if (j.tracks) {
        const TrackDesc td = j.tracks[j.env_map ? j.env_map[e] : 0];
        L = td.closed ? td.L : 0.0;
    }
    s_col[0][tid] = me.x;
    s_col[1][tid] = me.y;
    s_col[2][tid] = me.c;
    s_col[3][tid] = me.sn;
    s_col[4][tid] = me.v;
    s_col[5][tid] = me.s;
    __syncthreads();
    const int base = tid - sub;
    NbrBest<KT> best;
    best.clear();
    for (int b = 0; b < A; ++b) best.offer(nbr_d2(me.x, me.y, s_col[0][base + b], s_col[1][base + b]), b, a, j.sp.R2);
    const int n_live = e_here * A, w = grp * A + sub;   // the workgroup's live agents are consecutive; w: this one's place
    const int KDp = KD | 1;                             // the stage's row pitch: odd, so the lanes' rows start on different banks
    const int per = kNbrStageFloats / KDp;              // agents per piece (>= 75)
    const int step_w = 256 / KD, step_c = 256 - step_w * KD;   // what 256 floats further on means in (agent, float of the agent)
    float *dst = j.out + (size_t)(j.env0 + e_first) * A * KD;
    for (int p0 = 0; p0 < n_live; p0 += per) {
        if (live && w >= p0 && w < p0 + per) {
            float *o = s_out + (w - p0) * KDp;
#pragma unroll
            for (int k = 0; k < KT; ++k) {
                if (k < K) {
                    const int ib = best.idx[k];
                    const int q = base + (ib >= 0 ? ib : sub);
                    NbrAgent nb;
                    nb.x = s_col[0][q];
                    nb.y = s_col[1][q];
                    nb.c = s_col[2][q];
                    nb.sn = s_col[3][q];
                    nb.v = s_col[4][q];
                    nb.s = s_col[5][q];
                    const size_t slot = i * K + k;
                    nbr_slot(j.sp, me, nb, ib, L, o + k * D, j.raw ? j.raw + slot * NBR_NCHANNELS : nullptr, j.idx ? j.idx + slot : nullptr);
                }
            }
        }
        __syncthreads();
        const int nf = min(per, n_live - p0) * KD;
        int qw = tid / KD, qc = tid - qw * KD;
        for (int q = tid; q < nf; q += 256) {
            dst[(size_t)p0 * KD + q] = s_out[qw * KDp + qc];
            qw += step_w;
            qc += step_c;
            if (qc >= KD) qc -= KD, ++qw;
        }
        __syncthreads();
    }
}

// ---- line follower (f110_follow_line_*; include/f110.h states the rule, f110_math.hpp line_* the arithmetic) ---------------------
// One lane per agent.  kFollow = false (no armed spec looks for a car ahead, or one car per env): the lanes are the agents in
// order, GA = 1.  kFollow = true: a group of G lanes per env, G the power of two >= A = GA (as in k_neighbors), 256 / G envs per
// workgroup; every lane leaves (s, lat, v) of its agent in three LDS columns (6 KiB) and an armed lane walks b = 0 .. A - 1 of its
// group, which all lanes of a group read at the same address at the same time: a broadcast.
// What an agent costs without the car-ahead term is one dependent chain: its columns, then ~log2(nseg) probes of cum for each of
// the two stations (the steering station and the speed station, independent of each other), then one round of segment and
// attribute loads.  cum of the workgroup's first agent's slot is staged in LDS when it has at most kPreviewLdsSegs segments, as
// k_track_preview does; a lane on another slot, or on a longer track, probes L2.  The rule defines k uniquely, so where a probe
// was served does not show.
// The early exit comes before the kernel's one barrier: every wave reads the assignment of the workgroup's 256 lanes (four
// coalesced loads) and so knows which waves hold an armed agent.  A wave without one leaves before it loads anything else — with
// G > 64 only when no wave of its env holds one, since the env's armed cars need its columns.  The waves that stay share the
// staging of cum among themselves.  Behind the barrier a lane without a line follower leaves.  Idle lanes (G > A, or past the last
// group) shadow the last live agent and store nothing.  No atomics, no scratch.
struct LineJob {
    const LineSpec *specs;         // device memory
    const int32_t *assign;         // [.] -1 = no line follower, else the spec; null: spec 0 for every row (unit form)
    const TrackDesc *tracks;
    const PreviewAttr *attrs;
    const int32_t *env_map;        // or null: slot 0
    int32_t A, GA, shift, unit_slot;   // cars per env; agents per lane group (A or 1); lanes per group = 1 << shift; -1 or the unit form's slot
    int32_t i0, groups;            // agents [i0, i0 + groups * GA)
    int32_t stride, pad_;
    const double *px, *py, *pth, *pv, *ps, *plat;   // `stride` apart per agent
    const int32_t *cnt;            // step_count [.] (device form) ...
    const double *cnt_f;           // ... or the unit form's column, `stride` apart
    double *actions;               // [.][2]
    double *info;                  // [.][4] or null
    double *raw;                   // [.][12] or null
};

template <bool kFollow>
__global__ void __launch_bounds__(256) k_follow_line(LineJob j)
{
    __shared__ double s_cum[kPreviewLdsSegs];
    __shared__ double s_col[kFollow ? 3 * 256 : 1];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int G = 1 << j.shift, GA = j.GA;
    const int gpw = 256 >> j.shift;
    const int g_first = (int)blockIdx.x * gpw;
    const int g_here = min(gpw, j.groups - g_first);   // >= 1 by the grid
    const size_t i_first = (size_t)j.i0 + (size_t)g_first * GA;
    // which waves hold an armed agent, and which stay
    int armed_waves = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int t = w * 64 + lane, tg = t >> j.shift, ts = t & (G - 1);
        bool on = tg < g_here && ts < GA;
        if (on && j.assign) on = j.assign[i_first + (size_t)tg * GA + ts] >= 0;
        if (__ballot(on) != 0ull) armed_waves |= 1 << w;
    }
    const int gsh = kFollow && j.shift > 6 ? j.shift - 6 : 0;   // waves per env = 1 << gsh
    int stay = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
        if (armed_waves & (((1 << (1 << gsh)) - 1) << (w >> gsh << gsh))) stay |= 1 << w;
    stay = __builtin_amdgcn_readfirstlane(stay);
    if (!(stay >> wave & 1)) return;   // before the barrier: nothing but the assignment was loaded
    const int n_stay = __popc(stay), rank = __popc(stay & ((1 << wave) - 1));

    const int grp = tid >> j.shift, sub = tid & (G - 1);
    const bool live = grp < g_here && sub < GA;
    const int a = sub < GA ? sub : GA - 1;
    const size_t i = i_first + (size_t)(grp < g_here ? grp : g_here - 1) * GA + a, r = i * j.stride;
    const int ks = j.assign ? j.assign[i] : 0;
    const bool armed = live && ks >= 0;
    const int slot0 = j.unit_slot >= 0 ? j.unit_slot : (j.env_map ? j.env_map[i_first / j.A] : 0);
    const TrackDesc t0 = j.tracks[slot0];
    const bool staged = t0.nseg > 0 && t0.nseg <= kPreviewLdsSegs;
    if (staged) {
        const double *cum0 = t0.cols + (size_t)kTrkCum * t0.nseg;
        for (int q = rank * 64 + lane; q < t0.nseg; q += 64 * n_stay) s_cum[q] = cum0[q];
    }
    const double s = j.ps[r], lat = j.plat[r], v = j.pv[r];
    if (kFollow) {
        s_col[tid] = s;
        s_col[256 + tid] = lat;
        s_col[512 + tid] = v;
    }
    __syncthreads();
    if (!armed) return;

    const LineSpec sp = j.specs[ks];
    double2 *act = reinterpret_cast<double2 *>(j.actions) + i;
    double2 *info = j.info ? reinterpret_cast<double2 *>(j.info) + 2 * i : nullptr;
    double *raw = j.raw ? j.raw + (size_t)LINE_NRAW * i : nullptr;
    if (j.cnt ? j.cnt[i] == 0 : j.cnt_f[r] == 0.0) {   // re-seated inside the step just taken
        double z[2];
        line_fresh(z, raw);
        *act = make_double2(0.0, 0.0);
        if (info) info[0] = make_double2(0.0, 0.0), info[1] = make_double2(-1.0, -1.0);
        return;
    }
    const int slot = j.unit_slot >= 0 ? j.unit_slot : (j.env_map ? j.env_map[i / j.A] : 0);
    const TrackDesc td = j.tracks[slot];
    const PreviewAttr at = j.attrs[slot];
    PreviewTrack tr;
    tr.cols = td.cols;
    tr.attr = at.a;
    tr.nseg = td.nseg;
    tr.closed = td.closed;
    tr.C = at.a ? at.C : 0;
    tr.npts = td.closed ? td.nseg : td.nseg + 1;
    tr.L = td.L;
    const bool in_lds = staged && slot == slot0;
    const double *gcum = td.cols + (size_t)kTrkCum * td.nseg;
    const double ld = line_lookahead(sp, v);
    const double s_t = line_ahead(s, ld, td.closed, td.L);
    const double s_v = line_ahead(s, sp.speed_look, td.closed, td.L);
    const int k = in_lds ? preview_segment(s_cum, td.nseg, s_t) : preview_segment(gcum, td.nseg, s_t);
    double vref = sp.v_const;
    if (sp.speed_attr >= 0) {   // (a slot without the column is refused on the host)
        const int kv = in_lds ? preview_segment(s_cum, td.nseg, s_v) : preview_segment(gcum, td.nseg, s_v);
        vref = line_attr(tr, sp.speed_attr, kv, s_v);
    }
    double X, Y, Tx, Ty, lx, ly, c, sn;
    line_target(tr, k, s_t, sp.lane_offset, X, Y, Tx, Ty);
    cos_sin(j.pth[r], c, sn);
    const double steer = line_steer(sp, c, sn, j.px[r], j.py[r], Tx, Ty, lx, ly);
    double speed = line_speed(sp, vref, lat);
    int lim = -1;
    if (kFollow && sp.follow_range > 0.0) {
        const int base = tid - sub;
        const double Lw = td.closed ? td.L : 0.0;
        for (int b = 0; b < GA; ++b)
            if (b != a) line_offer(sp, s, lat, s_col[base + b], s_col[256 + base + b], s_col[512 + base + b], Lw, b, speed, lim);
    }
    *act = make_double2(steer, line_clamp(sp, speed));
    if (info) info[0] = make_double2(ld, vref), info[1] = make_double2((double)k, (double)lim);
    if (raw) {
        raw[LINE_RAW_LD] = ld, raw[LINE_RAW_ST] = s_t, raw[LINE_RAW_K] = (double)k, raw[LINE_RAW_X] = X, raw[LINE_RAW_Y] = Y;
        raw[LINE_RAW_TX] = Tx, raw[LINE_RAW_TY] = Ty, raw[LINE_RAW_LX] = lx, raw[LINE_RAW_LY] = ly, raw[LINE_RAW_VREF] = vref;
        raw[LINE_RAW_LIM] = (double)lim, raw[LINE_RAW_SPEED] = speed;
    }
}

// ---- rollout (f110_rollout_*; include/f110.h states the rule, f110_math.hpp roll_* the arithmetic) -------------------------------
// k_rollout: one lane per (agent, candidate), candidate-minor, so an agent's K candidates are consecutive lanes; 256-lane workgroups
// over the flat index.  A lane is one float64 dependent chain of H * repeat * ~1900 instructions with 16 bytes of action read per
// ~1900 * repeat of them: what matters is waves per SIMD (registers), not memory.
//  * the start state, the FIFO and the parameter row are loaded once per agent.  UNI (K a multiple of 64): every wave lies inside one
//    agent, the agent index goes through readfirstlane and those loads are scalar; the parameters then stay in SGPRs.
//  * TRAJ: a lane's trajectory row is H * 16 bytes, so the lanes of a store would be H * 16 bytes apart.  Each lane leaves its pose
//    (one float4) in an LDS stage instead, kRollChunk actions deep with a row pitch of kRollChunk + 1 float4 (an even pitch would
//    put every lane's write on the same banks); after every kRollChunk-th action (and the last) the workgroup stores the stage,
//    consecutive lanes consecutive float4 of a row: 128 contiguous bytes per row and flush, the whole region contiguous when
//    H <= kRollChunk.  The loops of roll_candidate have the same trip counts in every lane (a dead candidate idles through them), so
//    the barriers of the flush are reached by all.
//  * idle lanes (past count * K) shadow the last live one through every barrier and store nothing.
//  * the summary row is D <= 10 floats per lane, rows consecutive: the lanes of one store are D * 4 bytes apart and the workgroup's
//    region contiguous; once per candidate.
// k_rollout_track (only when PROGRESS or END_LAT is asked for): 16 lanes per candidate project the agent's start position and then
// the candidate's end position (k_rollout left it in end_xy) with k_track_project's search — every 16th segment per lane, the same
// pruning rule (the end's seed is the start's winner), a lexicographic (distance, index) minimum across the group — and lane 0
// writes the two values into the candidate's row.
constexpr int kRollChunk = 8;
constexpr int kRollPitch = kRollChunk + 1;

// agents [begin, begin + count) of columns with N entries each (the live ones, or the unit form's uploaded rows).  The map of agent
// n is maps[env_map ? env_map[n / A] : 0]; its track tracks[unit_slot >= 0 ? unit_slot : that slot].
struct RollJob {
    const ScanConst *maps;
    const int32_t *env_map;
    const TrackDesc *tracks;
    int32_t unit_slot, A;
    int32_t begin, count, N, params_per_agent;
    const double *state;      // [7][N]
    const double *steer_buf;  // [2][N]
    const int32_t *buf_cnt;   // [N]
    const double *params;     // [A][18] or [N][18] (params_per_agent)
    int32_t integrator, pad_;
    double time_step, lidar_dist;
    const double *actions;    // [K][H][2] or [N][K][H][2]
    float *out;               // [N][K][D]
    double *raw;              // [N][K][10] or nullptr
    float *traj;              // [N][K][H][4] or nullptr
    double *traj_raw;         // [N][K][H][4] or nullptr
    double *end_xy;           // [N][K][2] or nullptr: the end positions for k_rollout_track
    RollSpec sp;
};

// roll_candidate's emit on the device: the pose of action h into the lane's row of the stage, and the flush
struct RollEmitLds {
    static constexpr bool kOn = true;
    float4 *stage;       // the workgroup's stage [256][kRollPitch]
    float4 *traj;        // the workgroup's first row of the output, or nullptr
    double *raw_row;     // this lane's row of traj_raw, or nullptr
    int rows, H;         // live lanes of this workgroup
    double sx, sy, sc, ss;
    __device__ __forceinline__ void operator()(int h, const double *v) const
    {
        if (raw_row) {
#pragma unroll
            for (int q = 0; q < 4; ++q) raw_row[4 * h + q] = v[q];
        }
        if (!traj) return;
        const int tid = (int)threadIdx.x, slot = h % kRollChunk;
        stage[tid * kRollPitch + slot] = make_float4(roll_scaled(v[0], sx), roll_scaled(v[1], sy), roll_scaled(v[2], sc), roll_scaled(v[3], ss));
        if (slot != kRollChunk - 1 && h != H - 1) return;
        __syncthreads();
        const int cn = slot + 1, h0 = h - slot;
        for (int q = tid; q < rows * cn; q += 256) {
            const int row = q / cn, a = q - row * cn;
            traj[(size_t)row * H + h0 + a] = stage[row * kRollPitch + a];
        }
        __syncthreads();
    }
};

// ---- opponents (f110_rollout_opp_*, f110_mppi_set_opponents; f110_math.hpp opp_* the arithmetic) -------------------------
// k_opp_predict: 16 lanes per (row, opponent), row = an agent of the rollout or an armed index of the planner.  The group reads the
// opponent (the live columns of the env's other agent in ascending slot, or the unit form's uploaded row), TRACK: projects it with
// roll_search16 (every lane takes part; idle groups shadow the last one), then lane `sub` writes the predictions of the actions
// h = sub, sub + 16, ... into the table [row][Ao][H][2].  The OPP lanes of the two rollout kernels read the agent's rows back once
// per action: Ao * 16 bytes, wave-uniform when K % 64 == 0.  A lane carries only the minimum and the first hit across the step
// loop; the radius is read from device memory at every sample and the weights behind the loop (see sp_dev in k_mppi_roll).
__device__ __forceinline__ void roll_search16(const TrackDesc &td, double px, double py, int hint, int sub, int &best, double &s, double &lat);   // (below)

struct OppJob {
    const TrackDesc *tracks;
    const int32_t *env_map;
    int32_t unit_slot, A;
    int32_t r0, count, N, Ao;   // rows [r0, r0 + count); columns of N entries; opponents per row
    const int32_t *agents;      // [.] row -> agent, or nullptr: row r is agent r
    const double *state;        // [7][N]
    const double *opp_rows;     // [.][Ao][4] (x, y, v, theta) per row, or nullptr: the live columns
    int32_t H, repeat;
    double time_step;
    OppSpec *sp_out;            // or nullptr: where the first lane leaves sp for the lanes that sample
    double *table;              // [.][Ao][H][2]
    OppSpec sp;
};

__global__ void __launch_bounds__(256) k_opp_predict(OppJob j)
{
    const long long total = (long long)j.count * j.Ao;
    const long long gid = ((long long)blockIdx.x * 256 + (int)threadIdx.x) / kTrackLanes;
    const int sub = (int)threadIdx.x & (kTrackLanes - 1);
    const bool live = gid < total;
    const long long g = live ? gid : total - 1;
    if (j.sp_out && blockIdx.x == 0 && threadIdx.x == 0) *j.sp_out = j.sp;
    const int r = j.r0 + (int)(g / j.Ao), o = (int)(g % j.Ao);
    const int n = j.agents ? j.agents[r] : r;
    const size_t N = (size_t)j.N;
    double ov[4];
    if (j.opp_rows) {
#pragma unroll
        for (int q = 0; q < 4; ++q) ov[q] = j.opp_rows[((size_t)r * j.Ao + o) * 4 + q];
    } else {
        const int a = n % j.A, nb = n - a + (o < a ? o : o + 1);
        ov[0] = j.state[nb];
        ov[1] = j.state[N + nb];
        ov[2] = j.state[3 * N + nb];
        ov[3] = j.state[4 * N + nb];
    }
    const bool seen = opp_in_range(j.state[n], j.state[N + n], ov[0], ov[1], j.sp.max_range);
    double a = 0.0, b = 0.0;   // CV: cos, sin; TRACK: s_o, lat_o
    PreviewTrack tr{};
    if (j.sp.mode == OPP_TRACK) {
        const TrackDesc td = j.tracks[j.unit_slot >= 0 ? j.unit_slot : (j.env_map ? j.env_map[n / j.A] : 0)];
        int seg;
        roll_search16(td, ov[0], ov[1], -1, sub, seg, a, b);
        tr = PreviewTrack{td.cols, nullptr, td.nseg, td.closed, 0, 0, td.L};
    } else if (seen) {
        cos_sin(ov[3], a, b);
    }
    if (!live) return;
    double *p = j.table + ((size_t)r * j.Ao + o) * j.H * 2;
    for (int h = sub; h < j.H; h += kTrackLanes) {
        const double tau = opp_tau(h, j.repeat, j.time_step);
        if (!seen) p[2 * h] = p[2 * h + 1] = NAN;
        else if (j.sp.mode == OPP_CV) opp_predict_cv(ov[0], ov[1], ov[2], a, b, tau, p + 2 * h);
        else opp_predict_track(tr, a, b, ov[2], tau, p + 2 * h);
    }
}

// what a lane of k_rollout_opp / k_mppi_roll_opp reads and leaves
struct OppLane {
    const double *table;     // k_opp_predict's [.][Ao][H][2]: the row of agent n (rollout) or of armed index i (planner)
    const OppSpec *sp_dev;   // the settings in device memory
    float *out;              // [.][K][2] ((float)OPP_MIN, (float)OPP_FREE) per candidate, or nullptr
    double *raw;             // [.][K][2] the same before the conversion, or nullptr
    int32_t Ao, pad_;
};

// roll_candidate's xy hook: the candidate's position behind action h against its agent's rows
struct OppEmit {
    const double *rows;
    const OppSpec *sp;
    int Ao, H;
    mutable double m;
    mutable int free;
    __device__ __forceinline__ void xy(int h, double x, double y) const { opp_sample(rows, Ao, H, h, x, y, *sp, m, free); }
};

__device__ __forceinline__ OppEmit opp_emit(const OppLane &o, size_t row, int H)
{
    return OppEmit{o.table + row * o.Ao * H * 2, o.sp_dev, o.Ao, H, INFINITY, H};
}

__device__ __forceinline__ void opp_store(const OppLane &o, size_t G, double m, int free)
{
    if (o.out) {
        o.out[2 * G] = (float)m;
        o.out[2 * G + 1] = (float)free;
    }
    if (o.raw) {
        o.raw[2 * G] = m;
        o.raw[2 * G + 1] = (double)free;
    }
}

// an emit of the rollout with the opponent term's hook beside it
template <class Base>
struct RollEmitWithOpp : Base {
    static constexpr bool kXY = true;
    OppEmit opp;
    __device__ __forceinline__ void xy(int h, double x, double y) const { opp.xy(h, x, y); }
};

template <bool UNI, bool TRAJ>
__global__ void __launch_bounds__(256) k_rollout(RollJob j)
{
    __shared__ float4 s_stage[TRAJ ? 256 * kRollPitch : 1];
    const int K = j.sp.K, H = j.sp.H;
    const long long total = (long long)j.count * K;
    const long long g0 = (long long)blockIdx.x * 256, g_lane = g0 + (int)threadIdx.x;
    const bool live = g_lane < total;
    const long long g = live ? g_lane : total - 1;
    int a = (int)(g / K);
    const int kk = (int)(g - (long long)a * K);
    if (UNI) a = __builtin_amdgcn_readfirstlane(a);
    const int n = j.begin + a;
    const size_t N = (size_t)j.N;
    const size_t G = (size_t)j.begin * K + (size_t)g;   // the candidate's row in every output
    const VehicleParams vp = load_params(j.params + (size_t)(j.params_per_agent ? n : n % j.A) * NPARAMS);
    RollCar car;
#pragma unroll
    for (int c = 0; c < 7; ++c) car.st[c] = j.state[(size_t)c * N + n];
    car.b0 = j.steer_buf[n];
    car.b1 = j.steer_buf[N + n];
    car.cnt = j.buf_cnt[n];
    const ScanConst &k = j.maps[j.env_map ? j.env_map[n / j.A] : 0];
    const double *act = j.actions + (j.sp.layout == ROLL_PER_AGENT ? G : (size_t)kk) * H * 2;
    int alive;
    double min_clear;
    RollFrame fr;
    if constexpr (TRAJ) {
        fr = roll_frame(j.sp.frame, car.st[0], car.st[1], car.st[4]);
        RollEmitLds emit;
        emit.stage = s_stage;
        emit.traj = j.traj ? reinterpret_cast<float4 *>(j.traj) + ((size_t)j.begin * K + (size_t)g0) * H : nullptr;
        emit.raw_row = j.traj_raw && live ? j.traj_raw + G * H * 4 : nullptr;
        emit.rows = (int)(total - g0 < 256 ? total - g0 : 256);
        emit.H = H;
        emit.sx = j.sp.scale[ROLL_END_X];
        emit.sy = j.sp.scale[ROLL_END_Y];
        emit.sc = j.sp.scale[ROLL_END_COS];
        emit.ss = j.sp.scale[ROLL_END_SIN];
        roll_candidate(j.sp, k, vp, j.time_step, j.integrator, j.lidar_dist, car, act, fr, alive, min_clear, emit);
    } else {
        roll_candidate(j.sp, k, vp, j.time_step, j.integrator, j.lidar_dist, car, act, fr, alive, min_clear, RollEmitNone());
        // the frame only now, from the start pose read again: four doubles fewer are live across the loop
        fr = roll_frame(j.sp.frame, j.state[n], j.state[N + n], j.state[4 * N + n]);
    }
    if (!live) return;
    double v[ROLL_NCHANNELS];
    const int32_t all = (1 << ROLL_NCHANNELS) - 1;
    roll_values(fr, car, alive, min_clear, j.raw ? all : j.sp.channels, v);
    roll_store(j.sp, v, all & ~kRollTrackBits, j.out + G * j.sp.D, j.raw ? j.raw + G * ROLL_NCHANNELS : nullptr);
    if (j.end_xy) {
        j.end_xy[2 * G] = car.st[0];
        j.end_xy[2 * G + 1] = car.st[1];
    }
}

// k_rollout with the opponent term: the same lane with roll_candidate's xy hook sampling the agent's rows of k_opp_predict's table,
// and d_opp written beside the summary.  A kernel of its own beside k_rollout, not a third template parameter of it: routing
// k_rollout's lane through a shared function moved its register allocation (its SGPR spill counts), and the existing instantiations
// stay exactly what they were.
template <bool UNI, bool TRAJ>
__global__ void __launch_bounds__(256) k_rollout_opp(RollJob j, OppLane o)
{
    __shared__ float4 s_stage[TRAJ ? 256 * kRollPitch : 1];
    const int K = j.sp.K, H = j.sp.H;
    const long long total = (long long)j.count * K;
    const long long g0 = (long long)blockIdx.x * 256, g_lane = g0 + (int)threadIdx.x;
    const bool live = g_lane < total;
    const long long g = live ? g_lane : total - 1;
    int a = (int)(g / K);
    const int kk = (int)(g - (long long)a * K);
    if (UNI) a = __builtin_amdgcn_readfirstlane(a);
    const int n = j.begin + a;
    const size_t N = (size_t)j.N;
    const size_t G = (size_t)j.begin * K + (size_t)g;
    const VehicleParams vp = load_params(j.params + (size_t)(j.params_per_agent ? n : n % j.A) * NPARAMS);
    RollCar car;
#pragma unroll
    for (int c = 0; c < 7; ++c) car.st[c] = j.state[(size_t)c * N + n];
    car.b0 = j.steer_buf[n];
    car.b1 = j.steer_buf[N + n];
    car.cnt = j.buf_cnt[n];
    const ScanConst &k = j.maps[j.env_map ? j.env_map[n / j.A] : 0];
    const double *act = j.actions + (j.sp.layout == ROLL_PER_AGENT ? G : (size_t)kk) * H * 2;
    int alive;
    double min_clear, opp_m;
    int opp_free;
    RollFrame fr;
    if constexpr (TRAJ) {
        fr = roll_frame(j.sp.frame, car.st[0], car.st[1], car.st[4]);
        RollEmitWithOpp<RollEmitLds> emit;
        emit.opp = opp_emit(o, (size_t)n, H);
        emit.stage = s_stage;
        emit.traj = j.traj ? reinterpret_cast<float4 *>(j.traj) + ((size_t)j.begin * K + (size_t)g0) * H : nullptr;
        emit.raw_row = j.traj_raw && live ? j.traj_raw + G * H * 4 : nullptr;
        emit.rows = (int)(total - g0 < 256 ? total - g0 : 256);
        emit.H = H;
        emit.sx = j.sp.scale[ROLL_END_X];
        emit.sy = j.sp.scale[ROLL_END_Y];
        emit.sc = j.sp.scale[ROLL_END_COS];
        emit.ss = j.sp.scale[ROLL_END_SIN];
        roll_candidate(j.sp, k, vp, j.time_step, j.integrator, j.lidar_dist, car, act, fr, alive, min_clear, emit);
        opp_m = emit.opp.m, opp_free = emit.opp.free;
    } else {
        RollEmitWithOpp<RollEmitNone> emit;
        emit.opp = opp_emit(o, (size_t)n, H);
        roll_candidate(j.sp, k, vp, j.time_step, j.integrator, j.lidar_dist, car, act, fr, alive, min_clear, emit);
        opp_m = emit.opp.m, opp_free = emit.opp.free;
        fr = roll_frame(j.sp.frame, j.state[n], j.state[N + n], j.state[4 * N + n]);
    }
    if (!live) return;
    opp_store(o, G, opp_m, opp_free);
    double v[ROLL_NCHANNELS];
    const int32_t all = (1 << ROLL_NCHANNELS) - 1;
    roll_values(fr, car, alive, min_clear, j.raw ? all : j.sp.channels, v);
    roll_store(j.sp, v, all & ~kRollTrackBits, j.out + G * j.sp.D, j.raw ? j.raw + G * ROLL_NCHANNELS : nullptr);
    if (j.end_xy) {
        j.end_xy[2 * G] = car.st[0];
        j.end_xy[2 * G + 1] = car.st[1];
    }
}

// k_track_project's search for one pose by the 16 lanes of a group: lane `sub` takes every 16th segment and keeps its first minimum;
// a segment is skipped when a lower bound of its distance exceeds the smaller of the seed segment's distance (hint < 0: no seed)
// and the lane's running minimum by more than kTrackPruneMargin, so it can neither win nor tie; every lane returns the group's
// winner
__device__ __forceinline__ void roll_search16(const TrackDesc &td, double px, double py, int hint, int sub, int &best, double &s, double &lat)
{
    const double *src = td.cols;
    const size_t cs = (size_t)td.nseg;
    double dist = INFINITY, tb = 0.0, seed = INFINITY;
    best = 0x7fffffff;
    if (hint >= 0) {
        double t;
        seed = track_seg_dist(src, cs, hint < td.nseg ? hint : td.nseg - 1, px, py, t);
    }
    for (int k = sub; k < td.nseg; k += kTrackLanes) {
        const double ax = src[k], ay = src[cs + k], dx = src[2 * cs + k], dy = src[3 * cs + k];
        const double mx = px - (ax + 0.5 * dx), my = py - (ay + 0.5 * dy);
        const double reach = (seed < dist ? seed : dist) + 0.5 * src[5 * cs + k] + kTrackPruneMargin;
        if (mx * mx + my * my > reach * reach) continue;
        double t;
        const double d = track_seg_dist(src, cs, k, px, py, t);
        if (d < dist) {
            dist = d;
            tb = t;
            best = k;
        }
    }
#pragma unroll
    for (int m = 1; m < kTrackLanes; m <<= 1) {
        const double od = __shfl_xor(dist, m, kTrackLanes), ot = __shfl_xor(tb, m, kTrackLanes);
        const int ob = __shfl_xor(best, m, kTrackLanes);
        if (od < dist || (od == dist && ob < best)) {
            dist = od;
            tb = ot;
            best = ob;
        }
    }
    if (best == 0x7fffffff) {   // no distance below +inf (a NaN pose): np.argmin -> 0, with segment 0's own t and distance
        best = 0;
        dist = track_seg_dist(src, cs, 0, px, py, tb);
    }
    track_winner(src, cs, best, tb, dist, px, py, s, lat);
}

__global__ void __launch_bounds__(256) k_rollout_track(RollJob j)
{
    const int K = j.sp.K;
    const long long total = (long long)j.count * K;
    const long long gid = ((long long)blockIdx.x * 256 + (int)threadIdx.x) / kTrackLanes;
    const int sub = (int)threadIdx.x & (kTrackLanes - 1);
    const bool live = gid < total;
    const long long g = live ? gid : total - 1;   // idle groups shadow the last candidate: every lane takes part in every shuffle
    const int n = j.begin + (int)(g / K);
    const size_t G = (size_t)j.begin * K + (size_t)g;
    const TrackDesc td = j.tracks[j.unit_slot >= 0 ? j.unit_slot : (j.env_map ? j.env_map[n / j.A] : 0)];
    int seg0, seg1;
    double s0, lat0, s1, lat1;
    roll_search16(td, j.state[n], j.state[(size_t)j.N + n], -1, sub, seg0, s0, lat0);
    roll_search16(td, j.end_xy[2 * G], j.end_xy[2 * G + 1], seg0, sub, seg1, s1, lat1);
    if (sub != 0 || !live) return;
    roll_store_track(j.sp, roll_progress(s0, s1, td.closed, td.L), lat1, j.out + G * j.sp.D, j.raw ? j.raw + G * ROLL_NCHANNELS : nullptr);
}

// ---- MPPI planner (f110_mppi_*; include/f110.h states the rule, f110_math.hpp / f110_rng.hpp mppi_* the arithmetic) ----
// k_mppi_roll: one lane per (armed index, candidate), candidate-minor, 256-lane workgroups over the flat index, as k_rollout.  A lane
//  * jumps the agent's generator by k * 2^20 steps with entry k of the jump table (two 128-bit multiplies), draws its 2 H normals
//    one after the other and writes its row of V [M][K][H][2]: a prologue, so that the generator's registers are dead inside
//    roll_candidate's ~1900-instruction step loop, which reads the row back (H * 16 bytes, the lane's own);
//  * rolls the row with roll_candidate as it is and leaves the cost: complete without a track pass, else its first two terms
//    and the end position for k_mppi_track.
//  UNI (K a multiple of 64): a wave lies inside one agent, the agent goes through readfirstlane and its loads are scalar.
// k_mppi_track (only when w_progress or w_lat is non-zero): k_rollout_track's scheme through the armed list: 16 lanes per candidate
//  project the agent's start and the candidate's end; lane 0 adds the two track terms to the cost.
// k_mppi_update: a group of GS lanes per armed agent, 256 / GS agents per workgroup; GS is the power of two >= max(2 H, min(K, 64)),
//  at least 16 — with K = 8, H = 8 a workgroup serves 16 agents instead of one.  The costs go into LDS; every lane walks them for
//  the minimum and its first index (LDS broadcasts; the same walk in every lane, so no reduction order to argue about); exp is
//  taken once per candidate; lanes t < 2 H walk k = 0 .. K - 1 over V[i][k][t] (16 H contiguous bytes per k: coalesced), each with
//  its own numerator; eta and q are summed by every lane in the same ascending order.  Idle groups shadow the last agent through
//  the barriers and store nothing.
struct MppiJob {
    const ScanConst *maps;
    const int32_t *env_map;
    const TrackDesc *tracks;
    int32_t unit_slot, A;
    int32_t i0, count, N, params_per_agent;   // armed indices [i0, i0 + count); columns of N entries
    const int32_t *agents;       // [M] the armed list, or nullptr: armed index i is row i (the unit form)
    const double *state;         // [7][N]
    const double *steer_buf;     // [2][N]
    const int32_t *buf_cnt;      // [N]
    const int32_t *step_count;   // [N] or nullptr (no row is fresh)
    const double *params;        // [A][18] or [N][18]
    int32_t integrator, pad_;
    double time_step, lidar_dist;
    const uint64_t *zk;          // the ziggurat's tables
    const double *zw, *zf;
    const U128 *jump_a, *jump_g; // [kMppiJumps]
    double *nominal;             // [M][H][2]
    uint64_t *streams;           // [M][4]
    double *V;                   // [M][K][H][2]
    double *cost;                // [M][K]
    double *end_xy;              // [M][K][2] or nullptr: the end positions for k_mppi_track
    double *weight;              // [M][K] or nullptr (the unit form's output)
    double *actions;             // [N][2]
    float *info;                 // [N][4] or nullptr
    const MppiSpec *sp_dev;      // sp in device memory: what k_mppi_roll's epilogue reads, so that the cost's settings are not held in
                                 // SGPRs across the step loop (they were spilled there)
    MppiSpec sp;
};

// a lane of k_mppi_roll (OPP false: `o` is not read) and of k_mppi_roll_opp
template <bool UNI, bool OPP>
__device__ __forceinline__ void mppi_roll_lane(const MppiJob &j, const OppLane &o)
{
    const int K = j.sp.K, H = j.sp.H;
    const long long total = (long long)j.count * K;
    const long long g = (long long)blockIdx.x * 256 + (int)threadIdx.x;
    if (g >= total) return;
    int a = (int)(g / K);
    const int kk = (int)(g - (long long)a * K);
    if (UNI) a = __builtin_amdgcn_readfirstlane(a);
    const int i = j.i0 + a;
    const int n = j.agents ? j.agents[i] : i;
    const size_t N = (size_t)j.N;
    const size_t G = (size_t)i * K + (size_t)kk;
    double *row = j.V + G * H * 2;
    {
        const bool fresh = j.step_count && j.step_count[n] == 0;
        const ZigTables zt = {j.zk, j.zw, j.zf};
        mppi_sample_row(j.sp, j.nominal + (size_t)i * H * 2, fresh, kk, j.streams + 4 * (size_t)i, j.jump_a[kk], j.jump_g[kk], zt, row);
    }
    const VehicleParams vp = load_params(j.params + (size_t)(j.params_per_agent ? n : n % j.A) * NPARAMS);
    RollCar car;
#pragma unroll
    for (int c = 0; c < 7; ++c) car.st[c] = j.state[(size_t)c * N + n];
    car.b0 = j.steer_buf[n];
    car.b1 = j.steer_buf[N + n];
    car.cnt = j.buf_cnt[n];
    const ScanConst &k = j.maps[j.env_map ? j.env_map[n / j.A] : 0];
    const RollSpec rs = mppi_roll_spec(j.sp);
    int alive;
    double min_clear;
    RollFrame fr;
    [[maybe_unused]] double opp_m;
    [[maybe_unused]] int opp_free;
    if constexpr (OPP) {
        RollEmitWithOpp<RollEmitNone> emit;
        emit.opp = opp_emit(o, (size_t)i, H);
        roll_candidate(rs, k, vp, j.time_step, j.integrator, j.lidar_dist, car, row, fr, alive, min_clear, emit);
        opp_m = emit.opp.m, opp_free = emit.opp.free;
    } else {
        roll_candidate(rs, k, vp, j.time_step, j.integrator, j.lidar_dist, car, row, fr, alive, min_clear, RollEmitNone());
    }
    // The cost's settings come from the spec's copy in device memory, NOT from j.sp: read from the kernel's arguments they are
    // loaded at entry and held in SGPRs across the step loop, and the spill slots of that gave <UNI = false> a private segment of
    // 20 bytes (§6i rules scratch out).  Keep every use of the spec behind the loop on `sp`.
    const MppiSpec &sp = *j.sp_dev;
    if constexpr (OPP) {
        // the opponent terms go between the map's and the track's, their weights read here from device memory for the same reason
        const double c = mppi_cost_opp(*o.sp_dev, mppi_cost_map(sp, alive, min_clear), sp.H, opp_free, opp_m);
        opp_store(o, G, opp_m, opp_free);
        if (j.end_xy) {
            j.cost[G] = c;
            j.end_xy[2 * G] = car.st[0];
            j.end_xy[2 * G + 1] = car.st[1];
        } else {
            j.cost[G] = mppi_cost_track(sp, c, 0.0, 0.0);
        }
    } else if (j.end_xy) {
        j.cost[G] = mppi_cost_map(sp, alive, min_clear);
        j.end_xy[2 * G] = car.st[0];
        j.end_xy[2 * G + 1] = car.st[1];
    } else {
        j.cost[G] = mppi_cost(sp, alive, min_clear, 0.0, 0.0);
    }
}

template <bool UNI>
__global__ void __launch_bounds__(256) k_mppi_roll(MppiJob j)
{
    mppi_roll_lane<UNI, false>(j, OppLane{});
}

template <bool UNI>
__global__ void __launch_bounds__(256) k_mppi_roll_opp(MppiJob j, OppLane o)
{
    mppi_roll_lane<UNI, true>(j, o);
}

__global__ void __launch_bounds__(256) k_mppi_track(MppiJob j)
{
    const int K = j.sp.K;
    const long long total = (long long)j.count * K;
    const long long gid = ((long long)blockIdx.x * 256 + (int)threadIdx.x) / kTrackLanes;
    const int sub = (int)threadIdx.x & (kTrackLanes - 1);
    const bool live = gid < total;
    const long long g = live ? gid : total - 1;   // idle groups shadow the last candidate: every lane takes part in every shuffle
    const int i = j.i0 + (int)(g / K);
    const int n = j.agents ? j.agents[i] : i;
    const size_t G = (size_t)j.i0 * K + (size_t)g;
    const TrackDesc td = j.tracks[j.unit_slot >= 0 ? j.unit_slot : (j.env_map ? j.env_map[n / j.A] : 0)];
    int seg0, seg1;
    double s0, lat0, s1, lat1;
    roll_search16(td, j.state[n], j.state[(size_t)j.N + n], -1, sub, seg0, s0, lat0);
    roll_search16(td, j.end_xy[2 * G], j.end_xy[2 * G + 1], seg0, sub, seg1, s1, lat1);
    if (sub != 0 || !live) return;
    j.cost[G] = mppi_cost_track(j.sp, j.cost[G], roll_progress(s0, s1, td.closed, td.L), lat1);
}

constexpr int kMppiLdsCosts = 1024;   // (256 / GS) * K at its largest: GS = 64, K = 256

// the lanes per agent of k_mppi_update
inline int mppi_group_lanes(int K, int H)
{
    const int need = 2 * H > (K < 64 ? K : 64) ? 2 * H : (K < 64 ? K : 64);
    int gs = 16;
    while (gs < need) gs <<= 1;
    return gs;
}

__global__ void __launch_bounds__(256) k_mppi_update(MppiJob j, int GS)
{
    __shared__ double s_cost[kMppiLdsCosts], s_w[kMppiLdsCosts];
    const int K = j.sp.K, H = j.sp.H;
    const int per = 256 / GS, grp = (int)threadIdx.x / GS, t = (int)threadIdx.x - grp * GS;
    const long long a_raw = (long long)blockIdx.x * per + grp;
    const bool live = a_raw < j.count;
    const int i = j.i0 + (int)(live ? a_raw : j.count - 1);
    const int n = j.agents ? j.agents[i] : i;
    double *sc = s_cost + grp * K, *sw = s_w + grp * K;
    const double *cost = j.cost + (size_t)i * K;
    for (int k = t; k < K; k += GS) sc[k] = cost[k];
    __syncthreads();
    double beta;
    int best;
    mppi_min(sc, K, beta, best);
    for (int k = t; k < K; k += GS) {
        const double w = mppi_weight(j.sp, sc[k], beta, k);
        sw[k] = w;
        if (j.weight && live) j.weight[(size_t)i * K + k] = w;
    }
    __syncthreads();
    double eta, q;
    mppi_norms(sw, K, eta, q);
    if (t < 2 * H) {
        const double u = mppi_blend(sw, j.V + (size_t)i * K * H * 2, K, H, t, eta);
        if (live) {
            mppi_store_nominal(j.sp, j.nominal + (size_t)i * H * 2, t, u);
            if (t < 2) j.actions[2 * (size_t)n + t] = u;
        }
    }
    if (t != 0 || !live) return;
    if (j.info) mppi_info(beta, sc[0], eta, q, best, j.info + 4 * (size_t)n);
    uint64_t *st = j.streams + 4 * (size_t)i;
    const U128 s1 = pcg_jump(U128{st[0], st[1]}, U128{st[2], st[3]}, j.jump_a[kMppiJumps - 1], j.jump_g[kMppiJumps - 1]);
    st[0] = s1.hi;
    st[1] = s1.lo;
}

// ---- particle filter (f110_pf_*; include/f110.h states the rule, f110_math.hpp / f110_rng.hpp pf_* the arithmetic) ----
// Four kernels, one behind the other on a stream, over the armed indices [i0, i0 + count):
// k_pf_plan: a wave per armed agent, four agents per workgroup.  The stored weights go into LDS; lane 0 sums their squares (the ESS),
//  takes the decision, turns them into their cumulative sums in place and draws u from sub-stream 0; the wave stores the sums.  Lane 0
//  also forms the odometry delta, once per agent instead of once per particle.
// k_pf_move: one lane per (armed index, particle), particle-minor.  A lane jumps the agent's generator to its sub-stream with entry
//  p + 1 of the jump table, draws its three normals, finds its ancestor by bisection in the cumulative sums, applies the fresh or the
//  motion rule and writes into the OTHER cloud buffer (a lane reads its ancestor's row, which another lane would overwrite).  It also
//  leaves the particle's ray header: the lidar position, the scan's start index and the first sample, which the particle's beams share.
// k_pf_sense, the hot path of count * P * B' rays: lanes are (particle, beam), beam-minor; a workgroup holds as many whole particles
//  as fit 256 lanes (ppw = 256 / B'), so one particle's beams sit in adjacent lanes and walk neighbouring cells, as a scan task's 64
//  beams do, and no particle straddles a workgroup.  The ray is the scan's: beam_dir_index, the handle's trig table, the slot's table
//  through trace_from_first (the fixed-point march with its exact fall-back) or, without a padded copy, march_from_first.  The B'
//  terms go through LDS and the particle's first lane sums them ascending.
// k_pf_update: a group of GS lanes per armed agent (the power of two >= min(P, 256), at least 16), 256 / GS agents per workgroup.
//  Lanes spread over the particles for everything per particle (one exp, one sincos, the products); the sums are each walked ascending
//  by ONE lane of the group over LDS — eta by lane 0, then the five sums of the estimate by lanes 0 .. 4 side by side, then the
//  spread by lane 0 — and handed on through an LDS slot.  Idle groups shadow the last agent through the barriers and store nothing.
struct PfJob {
    const ScanConst *maps;       // [slots] (or one: the unit form's slot)
    const int32_t *env_map;      // [E] or nullptr
    int32_t A, num_beams;
    int32_t i0, count, N, pad_;
    const int32_t *agents;       // [M] the armed list, or nullptr: armed index i is row i (the unit form)
    const double *px, *py, *pth; // [N] the true poses
    const double *scans;         // [N][num_beams]
    const int32_t *step_count;   // [N] or nullptr (no row is fresh)
    double lidar_dist;
    const uint64_t *zk;          // the ziggurat's tables
    const double *zw, *zf;
    const U128 *jump_a, *jump_g; // [kPfJumps]
    uint64_t *streams;           // [M][4]
    const double *X_in;          // [M][P][3] the stored cloud
    double *X_out;               // [M][P][3] the moved cloud (the stored one after the call)
    double *W;                   // [M][P]
    double *last;                // [M][3]
    double *cum;                 // [M][P]
    PfPlan *plan;                // [M]
    PfHdr *hdr;                  // [M][P]
    double *logw;                // [M][P]
    double *noise;               // [M][P][3] or nullptr (the unit form's outputs)
    int32_t *anc;                // [M][P] or nullptr
    double *expect;              // [M][P][B'] or nullptr
    double *pose;                // [N][3]
    float *info;                 // [N][4] or nullptr
    PfSpec sp;
};

__global__ void __launch_bounds__(256) k_pf_plan(PfJob j)
{
    extern __shared__ double s_pf_plan[];   // [4][P]
    const int P = j.sp.P;
    const int grp = (int)threadIdx.x >> 6, t = (int)threadIdx.x & 63;
    const long long a_raw = (long long)blockIdx.x * 4 + grp;
    const bool live = a_raw < j.count;
    const int i = j.i0 + (int)(live ? a_raw : j.count - 1);
    const int n = j.agents ? j.agents[i] : i;
    double *c = s_pf_plan + (size_t)grp * P;
    const double *W = j.W + (size_t)i * P;
    for (int p = t; p < P; p += 64) c[p] = W[p];
    __syncthreads();
    if (t == 0 && live) {
        PfPlan pl;
        pl.fresh = (j.step_count && j.step_count[n] == 0) ? 1 : 0;
        pl.u = pf_uniform(j.streams + 4 * (size_t)i);
        pl.resample = (!pl.fresh && pf_decide(j.sp, pf_ess(c, P))) ? 1 : 0;
        pf_cumulate(c, P, c);
        pl.ctot = c[P - 1];
        pf_odometry(j.last + 3 * (size_t)i, j.px[n], j.py[n], j.pth[n], pl.a, pl.b, pl.dth);
        j.plan[i] = pl;
    }
    __syncthreads();
    if (!live) return;
    double *cum = j.cum + (size_t)i * P;
    for (int p = t; p < P; p += 64) cum[p] = c[p];
}

__global__ void __launch_bounds__(256) k_pf_move(PfJob j, ScanConst k)
{
    const int P = j.sp.P;
    const long long total = (long long)j.count * P;
    const long long g = (long long)blockIdx.x * 256 + (int)threadIdx.x;
    if (g >= total) return;
    const int a = (int)(g / P), p = (int)(g - (long long)a * P);
    const int i = j.i0 + a;
    const int n = j.agents ? j.agents[i] : i;
    const size_t G = (size_t)i * P + (size_t)p;
    const PfPlan pl = j.plan[i];
    double e[3];
    {
        const ZigTables zt = {j.zk, j.zw, j.zf};
        pf_normals(j.streams + 4 * (size_t)i, j.jump_a[p + 1], j.jump_g[p + 1], zt, e);
    }
    if (j.noise) {
#pragma unroll
        for (int q = 0; q < 3; ++q) j.noise[3 * G + q] = e[q];
    }
    double X[3];
    int anc = p;
    if (pl.fresh) {
        pf_fresh(j.sp, j.px[n], j.py[n], j.pth[n], e, X);
    } else {
        if (pl.resample) anc = pf_ancestor(j.cum + (size_t)i * P, P, p, pl.u, pl.ctot);
        pf_move(j.sp, pl.a, pl.b, pl.dth, j.X_in + ((size_t)i * P + (size_t)anc) * 3, e, X);
    }
    if (pl.fresh | pl.resample) j.W[G] = 1.0 / (double)P;
    if (j.anc) j.anc[G] = anc;
#pragma unroll
    for (int q = 0; q < 3; ++q) j.X_out[3 * G + q] = X[q];
    const ScanConst &km = j.maps[j.env_map ? j.env_map[n / j.A] : 0];
    double lp[3];
    pf_lidar_pose(X, j.lidar_dist, lp);
    PfHdr hd;
    hd.x = lp[0];
    hd.y = lp[1];
    hd.start = scan_start_index(k, lp[2]);
    int r0, c0;
    hd.d0 = sample_distance<LAYOUT_ROWMAJOR, false, false>(km, nullptr, lp[0], lp[1], r0, c0);
    hd.fast = 0;
    hd.pad_ = 0;
    if (km.pad) {
        double ux, uy;
        padded_position<false>(km, lp[0], lp[1], ux, uy);
        hd.fast = padded_start_ok(km, ux, uy) ? 1 : 0;
    }
    j.hdr[G] = hd;
}

// a workgroup's whole particles
inline int pf_particles_per_group(int B) { return 256 / B; }

__global__ void __launch_bounds__(256) k_pf_sense(PfJob j, ScanConst k, int ppw)
{
    __shared__ double s_term[256];
    const int P = j.sp.P, B = j.sp.B;
    const int tid = (int)threadIdx.x, q = tid / B, jb = tid - q * B;
    const long long total = (long long)j.count * P;
    const long long gp = (long long)blockIdx.x * ppw + q;
    const bool live = q < ppw && gp < total;
    const size_t G = (size_t)j.i0 * P + (size_t)(live ? gp : 0);
    double term = 0.0;
    if (live) {
        const int i = j.i0 + (int)(gp / P);
        const int n = j.agents ? j.agents[i] : i;
        const PfHdr hd = j.hdr[G];
        const int beam = j.sp.beam_first + jb * j.sp.beam_stride;
        const double z = j.scans[(size_t)n * j.num_beams + beam];
        const ScanConst *cold = j.maps + (j.env_map ? j.env_map[n / j.A] : 0);
        const ScanConst km = *cold;
        int di = beam_dir_index(k, hd.start, beam);
        di = di < 0 ? 0 : di;   // (a NaN heading)
        const double2 cs = k.cs[di];
        int hr = -1, hc = -1, nl, path;
        double r;
        if (km.pad)
            r = trace_from_first<LAYOUT_PADDED, false, false, false>(km, cold, nullptr, hd.x, hd.y, hd.fast != 0, cs.x, cs.y, hd.d0, hr, hc, nl, path);
        else
            r = march_from_first<LAYOUT_ROWMAJOR, false, false>(km, nullptr, hd.x, hd.y, cs.x, cs.y, hd.d0, hr, hc, nl);
        if (j.expect) j.expect[G * B + jb] = r;
        term = pf_term(j.sp, z, r);
    }
    s_term[tid] = term;
    __syncthreads();
    if (live && jb == 0) j.logw[G] = pf_logw(j.sp, s_term + tid, B);
}

// the lanes per agent of k_pf_update
inline int pf_group_lanes(int P)
{
    const int need = P < 256 ? P : 256;
    int gs = 16;
    while (gs < need) gs <<= 1;
    return gs;
}

constexpr int kPfSlots = 8;   // Lmax, eta, x, y, sin, cos, q

__global__ void __launch_bounds__(256) k_pf_update(PfJob j, int GS)
{
    extern __shared__ double s_pf_upd[];    // [256 / GS][6][P]
    __shared__ double s_slot[16][kPfSlots];
    const int P = j.sp.P;
    const int per = 256 / GS, grp = (int)threadIdx.x / GS, t = (int)threadIdx.x - grp * GS;
    const long long a_raw = (long long)blockIdx.x * per + grp;
    const bool live = a_raw < j.count;
    const int i = j.i0 + (int)(live ? a_raw : j.count - 1);
    const int n = j.agents ? j.agents[i] : i;
    double *sw = s_pf_upd + (size_t)grp * 6 * P, *sx = sw + P, *sy = sx + P, *ss = sy + P, *sc = ss + P, *sq = sc + P;
    double *slot = s_slot[grp];
    const double *L = j.logw + (size_t)i * P, *X = j.X_out + (size_t)i * P * 3;
    double *W = j.W + (size_t)i * P;
    for (int p = t; p < P; p += GS) sq[p] = L[p];
    __syncthreads();
    if (t == 0) slot[0] = pf_max(sq, P);
    __syncthreads();
    for (int p = t; p < P; p += GS) sw[p] = pf_unnorm(W[p], sq[p], slot[0]);
    __syncthreads();
    if (t == 0) slot[1] = pf_sum(sw, P);
    __syncthreads();
    for (int p = t; p < P; p += GS) {
        const double w = pf_norm(sw[p], slot[1], P);
        if (live) W[p] = w;
        double c, s;
        cos_sin(X[3 * p + 2], c, s);
        sw[p] = w;
        sx[p] = w * X[3 * p];
        sy[p] = w * X[3 * p + 1];
        ss[p] = w * s;
        sc[p] = w * c;
        sq[p] = w * w;
    }
    __syncthreads();
    if (t < 5) slot[2 + t] = pf_sum(sx + (size_t)t * P, P);   // sx, sy, ss, sc, sq lie one behind the other
    __syncthreads();
    const double xh = slot[2], yh = slot[3];
    for (int p = t; p < P; p += GS) sx[p] = pf_spread_term(sw[p], X[3 * p], X[3 * p + 1], xh, yh);
    __syncthreads();
    if (t != 0 || !live) return;
    const double spread = pf_sum(sx, P);
    const double x = j.px[n], y = j.py[n], th = j.pth[n];
    double *o = j.pose + 3 * (size_t)n;
    o[0] = xh;
    o[1] = yh;
    o[2] = atan2(slot[4], slot[5]);
    if (j.info) pf_info(slot[6], spread, xh, yh, x, y, j.plan[i].resample, j.info + 4 * (size_t)n);
    double *last = j.last + 3 * (size_t)i;
    last[0] = x;
    last[1] = y;
    last[2] = th;
    pf_stream_advance(j.streams + 4 * (size_t)i, j.jump_a[kPfJumps - 1], j.jump_g[kPfJumps - 1]);
}
