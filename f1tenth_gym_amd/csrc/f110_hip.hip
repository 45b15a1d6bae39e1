// f110_hip.hip — host side of libf110_hip.so: the handle (one MI355X, one HIP stream + a side
// stream), device-memory ownership, kernel launches and the C ABI declared in include/f110.h.
// The kernels live in f110_kernels.hpp, the scalar float64 building blocks in f110_math.hpp.
// A step is integrate -> scan -> finalize on one stream, the pair tests inside the finalize kernel (k_finalize_pair_roles
// for two-agent envs, k_finalize_multi up to 256 agents per env); beyond that k_collide runs on the side stream, under the
// scan.  A tiny host-synchronised batch is one launch (k_step_tiny).  The table of forms stands above step_range.
// Compiled with -ffp-contract=off.  There is no CPU fallback in this library.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <set>
#include <string>
#include <vector>

#include "../../include/f110.h"
#include "f110_kernels.hpp"
#include "f110_devmem.hpp"

using devmem::DevArena;
using devmem::DevBuf;


// ============================================================================ host side

// Two builds of this file: libf110_hip.so (the product: ONE step dispatch per (agents per env, beams) case,
// the row-major and PADDED table layouts, no environment variables read anywhere) and, with
// -DF110_EXPERIMENTAL, libf110_hip_exp.so, which adds everything that was built, measured and not adopted
// (tiled / byte-code / LDS-window layouts, env groups, the HIP-graph step, other places
// for the pair tests, two-pass dedupe) plus f110_exp_set, the switchboard the A/B tests and profiles use.
#ifdef F110_EXPERIMENTAL
constexpr bool kExperimental = true;
#else
constexpr bool kExperimental = false;
#endif

// f110_exp_set keys (experimental build; the product keeps the defaults)
struct ExpSwitches {
    int scan_flat = 0;         // 1: the flat ray kernel instead of the agent-aligned one
    int long_prio = 0;         // 1: the longest-first pass's waves raise their issue priority (s_setprio 3)
    int scan_occupancy = 0;    // 4: run the step's scan kernel at 4 waves/SIMD (fusion feasibility A/B)
    int scan_env_counter = 0;  // 1: the scan kernel also counts finished tasks per env (fusion feasibility A/B)
    int integrate_duo = -1;    // 0: k_integrate<0> (one wave per 64 agents), 1: k_integrate_duo, -1 = default (duo)
    int group_split = 0;       // two env groups: percent of the envs in the first (0 = even)
    int integrate_fan = -1;    // 0 / 1: k_integrate_fan (thirteen waves per 64 agents, RK4) off / on at every size, -1 = default (small batches)
    int tiny_general_tail = 0;
    int pair_wave = -1;        // A = 2: k_finalize_pair_wave (one-wave workgroups) 0 = never, 1 = in every step; -1 = default (in a step of two env blocks: from 24 576 agents, or when step_groups = 2 asks for the blocks)
    int tiny_start_probe = 0;  // k_step_tiny tells the host when its first workgroup starts (f110_step_host times launch -> start -> done)
    long probe_calls = 0;
    double probe_us[3] = {0, 0, 0};
    uint64_t tiny_trace = 0;   // device address of a caller-owned [workgroups][16] uint64 buffer: k_step_tiny's phase stamps (0 = off)
    uint64_t scan_trace = 0;   // device address of a caller-owned [waves][8] uint64 buffer: clock stamps, hardware id, samples of every scan wave (0 = off)
};

// the device forms that copy a per-agent float32 output into a caller's page-locked block (env_blocks_output)
enum PinnedDst { kPinnedObs, kPinnedPreview, kPinnedNeighbors, kPinnedRollout, kPinnedCount };

// the agents a feature is armed on (f110_mppi_set, f110_pf_set; the armed_* helpers below): m == 0: disarmed
struct ArmedList {
    int m = 0;
    std::vector<int32_t> agents;     // the armed list, ascending
    DevBuf<int32_t> d_agents;        // [m]
    DevBuf<uint64_t> d_streams;      // [m][4] each agent's generator
};

struct f110_sim {
    f110_config cfg{};
    int N = 0;
    hipStream_t stream = nullptr;
    hipStream_t side_stream = nullptr;          // k_collide runs here, concurrently with k_scan_rays
    hipEvent_t ev_integrated = nullptr, ev_collided = nullptr;
    DevArena mem;       // what f110_create allocates for the handle's life: dev's columns (but the scans), the parameter / beam / trig tables, the staging columns, the noise generator's constants
    AgentArrays dev{};
    ScanConst k{};
    bool has_map = false;
    uint32_t step_magic = 0, step_shift = 0;  // ray -> agent division constants of the step launch
    int scan_tasks_per_wave = 1, num_cus = 256;  // consecutive 64-ray tasks per wave
    int scan_tasks_agent = 1;                    // ... of k_scan_rays_agent in its env order (ENV_ORDER), whose waves share noise samples between an env's agents
    bool scan_env_order = false;                 // k_scan_rays_agent<.., ENV_ORDER> where the launch allows it
    bool scan_tasks_auto = false;                // chosen by batch size (f110_config.scan_tasks_per_wave = 0)
    double ttc_side_max = INFINITY, ttc_cos_max = INFINITY;  // see f110_set_beam_tables
    int dir_stride = 0;              // > 0: dedupe enabled
    int scan_block = 64;
    DevBuf<double> d_params_all;   // [N][18] when f110_set_params_batch is active
    DevBuf<double> d_noise;        // the noise table, or the row cache's current block
    double *d_params = nullptr, *d_scan_angles = nullptr, *d_beam_cos = nullptr, *d_side = nullptr;   // (mem)
    // a different track per env: slot 0 is the map of f110_set_map_*, further slots come from
    // f110_add_map_*; f110_set_env_maps assigns them and builds the device tables
    struct MapSlot {
        DevBuf<double> d_dt_row, d_dt_pad;
        ScanConst k{};
        DevBuf<uint8_t> d_occ;      // f110_render_device's occupancy grid, built on first use
        bool occ_stale = false;     // ... and again after f110_set_map_obstacles re-stamped the table (the allocation stays)
        int base = -1;              // >= 0: a DERIVED slot (f110_add_map_obstacles), stamped from this base slot's table
        bool carved = false;        // a base slot of f110_add_map_corridor: f110_set_map_corridor may re-carve it in place
    };
    std::vector<MapSlot> extra_maps;
    DevBuf<MapFast> d_maps_fast;
    DevBuf<ScanConst> d_maps_full;
    int n_maps_dev = 0;                 // slots d_maps_full holds
    // f110_*_map_obstacles: the byte mask, the active columns' distances and list, the boxes, the out-of-bounds value (grow-only)
    struct ObstScratch {
        DevBuf<uint8_t> mask;
        DevBuf<uint32_t> g;
        DevBuf<int32_t> cols;
        DevBuf<ObstBox> boxes;
        DevBuf<double> oob;
    } obst;
    // f110_*_map_corridor: the line, the carved mask, the column distances and the squared distances, the carved count (grow-only)
    struct CorridorScratch {
        DevBuf<double> line;   // [M][2] points, then [S] half widths
        DevBuf<uint8_t> mask;
        DevBuf<uint32_t> g, d2;
        DevBuf<unsigned long long> carved;
        hipEvent_t ev[3] = {nullptr, nullptr, nullptr};   // before the mask kernel, behind it, behind the EDT (f110_map_corridor_times)
        double mask_ms = 0.0;                             // the last carve's mask kernel, read at the call's wait
        bool timed = false;                               // ev[1], ev[2] bracket an EDT
    } corr;
    // f110_map_centerline / f110_map_skeleton: the free mask and the two planes the passes ping-pong between ([H][ceil(W / 64)]
    // words each), the per-pass deletion counters, the loop's cells and their table values (grow-only)
    struct CenterlineScratch {
        DevBuf<uint64_t> free_plane, a, b;
        DevBuf<unsigned long long> deleted;
        DevBuf<int32_t> cells;
        DevBuf<double> values;
        double stage_ms[5] = {0, 0, 0, 0, 0};   // the last call's host time per stage (f110_map_centerline_times)
    } cl;
    DevBuf<int32_t> d_env_map;
    DevBuf<uint32_t> d_scan_order;      // [N] agents sorted by map slot (nullptr while every env is on one slot)
    bool multi_map = false;
    DevBuf<ScanConst> d_k;     // HBM copy of k (RayJob::k_cold), refreshed by cold_consts()
    ScanConst k_uploaded{};
    DevBuf<unsigned long long> d_path_stats;     // [3], see f110_scan_path_stats
    bool path_stats_on = false;
    DevBuf<double> d_dt_row, d_dt_pad;
    double *d_actions = nullptr, *d_poses = nullptr;   // (mem)
    double2 *d_cs = nullptr;
    uint8_t *d_mask = nullptr;
    // env groups: the step of G > 1 independent env blocks runs on G streams of its own (no event
    // between the kernels of a group, no dependency between groups; see f110_step_device)
    int groups = 1;
    std::vector<hipStream_t> gstreams;   // two groups: the main stream and the side stream (borrowed); more: streams of their own
    std::vector<hipStream_t> gowned;
    std::vector<hipEvent_t> gevents;
    hipEvent_t ev_main = nullptr;
    bool groups_auto = true;    // cfg.step_groups == 0: two blocks only for steps that come back to back, at the sizes where it pays
    bool touched = true;        // something other than f110_step_device went through the handle since the last step
    int last_blocks = 0;        // env blocks the most recent f110_step_device was submitted as
    int group_probes = 0;       // candidates the two-group form probed for a stream that runs next to the main stream
    bool groups_busy = false;   // group streams hold work the main stream has not been joined with
    bool main_dirty = true;     // the main stream holds work the group streams have not waited for
    // device RNG for the scan noise (f110_set_noise_rng)
    NoiseGen noise_gen{};
    uint64_t *d_zig_k = nullptr;     // (mem, like the next three)
    double *d_zig_w = nullptr, *d_zig_f = nullptr;
    U128 *d_jump = nullptr;          // [2][65]
    DevBuf<U128> d_rng_state, d_rng_seed, d_rng_rowstate;
    int noise_rows_ready = 0;        // rows of the row cache generated so far
    int noise_rows_alloc = 0;        // rows the row cache has memory for (grows on demand up to dev.noise_rows)
    // the next rows are generated AHEAD of need on a stream of their own (noise_start_ahead): a row is 12.8 us of one wave, the rows of a
    // stream come one after the other, and a step that waits for them pays that in full (measured, F110Env: +13 us on every step of a first episode)
    hipStream_t noise_stream = nullptr;
    hipEvent_t ev_noise = nullptr, ev_noise_src = nullptr;
    bool noise_ahead = false;        // rows [noise_rows_ready, noise_ahead_upto) are being generated into noise_ahead_block
    int noise_ahead_upto = 0, noise_ahead_alloc = 0;
    DevBuf<double> noise_ahead_block;
    std::vector<DevBuf<double>> noise_retired;   // earlier, smaller blocks of the cache (steps in flight may read them): freed with the cache
    long long noise_ub = 0;          // upper bound of any agent's step_count (steps since the last full reset)
    // identity of the noise source, for the state blobs (0 off, 1 table, 2 shared stream, 3 a stream per agent): the table's
    // FNV-1a hash / rows / beams, or the shared stream's PCG64 words
    int noise_src = 0;
    uint64_t noise_src_id[4] = {0, 0, 0, 0};
    DevBuf<unsigned char> d_state_blob;   // f110_state_save / _load: the device side of the whole-handle blob (grows on demand)
    unsigned long long *d_lookups = nullptr;  // f110_scan_lookup_count (mem)
    bool lookups_on = false;
    int collide_mode = 0;        // where the pair tests run: 0 side stream, 1 fused into k_integrate, 2 in line, 3 inside k_finalize (A = 2)
    // longest-first order of the scan tasks (TaskSched, small batches): double-buffered flags / lists / counters
    bool task_order = false;
    DevArena sched_mem;              // the five buffers below
    uint32_t *d_tflags[2] = {nullptr, nullptr}, *d_tlist[2] = {nullptr, nullptr}, *d_tcount = nullptr;
    TaskSched tsched[2]{};           // [parity], passed to the scan by value
    bool sched_allocated = false;
    uint32_t task_cap_alloc = 0;
    uint32_t task_epoch = 2, task_cap = 0, task_thr = 96;   // epochs start above the flags' initial 0
    uint32_t task_cap_div = 32, task_rev = 0;                // list capacity = tasks / task_cap_div; 1 = newest list entries first
    ExpSwitches exp;
    DevBuf<uint32_t> d_env_done;      // [num_envs] scan_env_counter probe
    ncclComm_t comm = nullptr;   // optional RCCL communicator for the observation gather
    bool beams_uniform = true;   // f110_set_beam_tables: scan_angles is (to a quarter of a spacing) the ramp base_classes.py:133-134 builds
    int comm_ranks = 0;
    // overlapped gather (f110_comm_set_overlap): scans are double-buffered, the all-gather of step t
    // runs on comm_stream while step t+1 fills the other buffer
    bool comm_overlap = false, comm_swap_next = false, comm_inflight = false;
    DevBuf<double> scan_bufs[2];                // the scans' owner: [0] from f110_create on, [1] with the overlapped gather; dev.scans is a view of one of them
    DevBuf<double> obs_scal[2];                 // [7][N] scalar observation block(s) of the observation gather
    DevBuf<float> scan_f32[2];                  // [N][B] float32 copies of the scans (F110_GATHER_F32 transport)
    int comm_rank = -1;
    bool comm_send_scalars = false;
    int scans_cur = 0;
    bool gather_pending[2] = {false, false};
    hipStream_t comm_stream = nullptr;
    hipEvent_t ev_step_done = nullptr, ev_gather_done[2] = {nullptr, nullptr};
    DevArena ep_mem;            // ep's columns and d_rot_stage
    EpisodeArrays ep{};
    bool has_episode = false;
    double *d_rot_stage = nullptr;
    DevBuf<unsigned char> d_packed;   // f110_episode_step_host's packed block
    // f110_step_host: the caller's block as last validated, and its device-side pointers
    bool hb_valid = false;
    f110_host_block hb_host{};
    HostBlock hb_dev{};
    const double *hb_actions_host = nullptr, *hb_actions_dev = nullptr;
    bool hb_scans_by_kernel = false;             // the validated block's scans are stored by the kernel (small batch, page-locked)
    unsigned long long *hb_seq_host = nullptr;   // page-locked completion word (F110_STEP_SPIN_WAIT)
    DevBuf<unsigned int> hb_blocks_done;
    unsigned long long hb_seq = 0;
    double hs_enqueue_us = 0, hs_wait_us = 0;    // f110_step_host_stats
    DevBuf<FusedHost> d_fused;                   // device copy of {episode arrays, host block, flags} for the pair kernel's epilogue
    FusedHost fused_host_copy{};                 // what d_fused holds
    bool fused_valid = false;
    long long hs_calls = 0;
    // the whole step of a tiny batch as ONE launch (k_step_tiny): counters + shadow columns, allocated on first use
    TinyCtl tiny{};
    DevBuf<unsigned char> tiny_mem;
    int tiny_off = 0;                 // lab A/B (f110_exp_set "step_tiny" = 0): the three-kernel form also for tiny batches
    int last_launches = 0;            // kernels the most recent step submitted its work as (f110_step_launches)
    // track progress (f110_track_*): a polyline per map slot, the step's columns, the per-agent cache of s
    struct TrackSlot {
        DevBuf<double> d_cols;      // [7][nseg] (TrackCol)
        DevBuf<double> d_pts;       // [npts][2] the points (after the closed-track dedupe), what a render draws
        DevBuf<double> d_attr;      // [nattr][npts] per-point attributes (f110_track_set_attrs), or null
        int32_t nattr = 0;
        int32_t nseg = 0, closed = 0, npts = 0;
        double L = 0.0;
    };
    std::vector<TrackSlot> tracks;        // indexed by map slot (shorter than the slot list: the rest have no track)
    DevBuf<TrackDesc> d_tracks;           // [n_tracks_dev] what the kernels read
    DevBuf<PreviewAttr> d_track_attrs;    // [n_tracks_dev] the slots' attribute columns (k_track_preview), uploaded with d_tracks
    int n_tracks_dev = 0;
    bool tracks_dirty = true;             // d_tracks does not reflect `tracks` / the slot count
    bool track_lds = false;               // some track fits the LDS-staged form
    bool track_on = false, track_checked = false;   // f110_track_enable; every env's slot has a track (checked since the last change)
    std::vector<int32_t> env_map_host;    // f110_set_env_maps' assignment (meaningful while multi_map)
    DevBuf<double> d_trk;                 // [4][N] s, ds, lateral, heading_error
    DevBuf<int32_t> d_trk_seg;            // [N]
    DevBuf<double> d_trk_cache;           // [3][N] cached s, x, y
    DevBuf<int32_t> d_trk_ok;             // [N]
    f110_track_host trk_pinned{};         // f110_track_host_block, host pointers ...
    HostBlock trk_hb{};                   // ... and their device views (the trk_* fields)
    bool trk_pinned_on = false;
    const float *pinned_dst[kPinnedCount] = {};   // per device form: the page-locked block its last copy went to (f110_host_free)
    DevBuf<double> d_roll_end;               // f110_rollout_device: the candidates' end positions between its two kernels (grows on demand)
    // scripted cars (f110_controllers_set): the specs and the per-agent assignment in device memory; gap_specs == 0: disarmed
    DevBuf<GapSpec> d_gap_specs;
    DevBuf<int32_t> d_gap_assign;
    int gap_specs = 0, gap_max_w = 0;
    std::vector<int32_t> gap_assign_host;   // the armed assignment (empty while disarmed): what f110_mppi_set checks its agents against
    // line followers (f110_line_followers_set): the same shape; line_specs == 0: disarmed
    DevBuf<LineSpec> d_line_specs;
    DevBuf<int32_t> d_line_assign;
    int line_specs = 0;
    bool line_follow = false;                // some armed spec looks for a car ahead (follow_range > 0 and A > 1)
    bool line_checked = false;               // line_ready's slot checks hold (since the last change of the tracks, the env maps or the arming)
    LineSpec line_specs_host[LINE_MAX_SPECS] = {};
    std::vector<int32_t> line_assign_host;   // (empty while disarmed): what f110_controllers_set and f110_mppi_set check against
    // MPPI planner (f110_mppi_set): on.m == 0: disarmed.  The nominal sequences and the streams are the planner's own memory.
    struct Mppi {
        MppiSpec sp{};
        ArmedList on;
        DevBuf<MppiSpec> d_spec;         // sp, for the kernels
        DevBuf<double> d_nominal;        // [m][H][2]
        DevBuf<double> d_V;              // [m][K][H][2] the candidates of the last call
        DevBuf<double> d_cost;           // [m][K]
        DevBuf<double> d_end;            // [m][K][2] (only with a track weight)
        // the opponent term (f110_mppi_set_opponents): attached while opp_on; it goes with the planner
        bool opp_on = false;
        OppSpec opp{};
        DevBuf<OppSpec> d_opp_spec;      // opp, for the kernels
        DevBuf<double> d_opp_table;      // [m][A - 1][H][2] the predictions of the last call
    } mppi;
    DevBuf<double> d_roll_opp;           // f110_rollout_opp_device: the predictions [N][A - 1][H][2] (grows on demand)
    DevBuf<OppSpec> d_roll_opp_spec;     // ... and its settings, one copy per env block, written by the block's own k_opp_predict
    DevBuf<U128> d_mppi_jump;            // [2][kMppiJumps] the candidates' jump constants (from the first arming on)
    // particle filter (f110_pf_set): on.m == 0: disarmed.  The clouds, the weights, the last poses and the streams are the filter's own memory.
    struct Pf {
        PfSpec sp{};
        ArmedList on;
        int cur = 0;                     // d_X[cur] is the stored cloud; a call moves it into d_X[cur ^ 1] and flips
        DevBuf<double> d_X[2];           // [m][P][3]
        DevBuf<double> d_W;              // [m][P]
        DevBuf<double> d_last;           // [m][3]
        DevBuf<double> d_cum;            // [m][P]
        DevBuf<double> d_logw;           // [m][P]
        DevBuf<PfPlan> d_plan;           // [m]
        DevBuf<PfHdr> d_hdr;             // [m][P]
    } pf;
    DevBuf<U128> d_pf_jump;              // [2][kPfJumps] the sub-streams' jump constants (from the first arming on)
    // rendering (f110_render_device): slot 0's occupancy grid, the slot table as last uploaded, per-frame / per-agent records
    DevBuf<uint8_t> d_occ0;
    std::vector<RenderSlot> render_slots;
    DevBuf<RenderSlot> d_render_slots;      // (this and the next three grow on demand)
    DevBuf<RenderFrame> d_render_frames;
    DevBuf<RenderCar> d_render_cars;
    DevBuf<int32_t> d_render_agents;
    DevBuf<uint8_t> d_render_stage;      // [F][H][pitch] when the caller's buffer cannot take 32-bit stores
    // randomised start poses (f110_reset_sampler_*): the settings, each env's stream, the explicit fallback poses, the counters
    struct ResetSampler {
        bool on = false;
        DevArena mem;                // job's device buffers
        SamplerJob job{};            // settings + device buffers; tracks / maps / mode are filled per launch
    } rs;
    // randomised vehicle parameters (f110_param_sampler_*): the entries, the nominal rows, each env's stream, the counter.  The
    // rows it draws are d_params_all, the block of f110_set_params_batch (the two refuse each other: the rows have one owner).
    struct ParamSampler {
        bool on = false;
        bool owns_rows = false;      // arming allocated d_params_all: disarming frees it
        DevArena mem;                // job's nominal, stream and counter
        ParamJob job{};              // entries + device buffers; the mode and what it selects by are filled per launch
    } ps;
    // timing
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    bool profiling = false;
    std::vector<hipEvent_t> prof_events;  // per step: before integrate, before scan, after scan, after finalize
    size_t prof_used = 0;
    char err[512] = {0};
};

// What one step is asked to do beyond a plain f110_step_device (the default-constructed request).  Built on the stack of
// f110_step_host / f110_episode_step_*, handed down to step_range / step_tiny, gone when the call returns.
struct StepRequest {
    bool tiny = false;                      // this step is ONE k_step_tiny launch (f110_step_host decided: tiny_applies)
    const double *tiny_actions = nullptr;   // ... whose arguments carry the caller's [N][2] actions (host memory)
    bool fuse = false;                      // A = 2: host block + episode logic ride in the pair kernel / the last workgroup (d_fused)
    unsigned long long seq = 0;             // ... with this completion number (0: nobody spins on the word)
    const HostBlock *hb = nullptr;          // one car per env, one launch: what k_host_block would be handed ...
    int episode = 0, auto_reset = 0;        // ... (block, episode logic on, re-seat finished envs)
    bool defer_draw = false;                // the caller launches the reset sampler's draw itself, behind its own last kernel
    bool env_blocks = false;                // step_submit: this step goes out as several env blocks, each on its own stream
};

static thread_local char g_err[512] = {0};

static int fail(f110_sim *h, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    snprintf(g_err, sizeof g_err, "%s", buf);
    if (h) snprintf(h->err, sizeof h->err, "%s", buf);
    return code;
}

#define HIPCHK(h, call)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(h, F110_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

// device memory comes from one of the two owners of f110_devmem.hpp: a buffer of its own (replaced: what it held is freed
// first) or one more allocation of an arena, whose pointer lands in *p
template <typename T>
static int dmalloc(f110_sim *h, DevBuf<T> *buf, size_t count)
{
    HIPCHK(h, buf->alloc(count));
    return F110_OK;
}

template <typename T>
static int dmalloc(f110_sim *h, DevArena &arena, T **p, size_t count)
{
    HIPCHK(h, arena.alloc(p, count));
    return F110_OK;
}

// grow-only buffers (DevBuf::grow): a regrow frees the old allocation, and hipFree waits for the work in flight that reads it
template <typename T>
static int dgrow(f110_sim *h, DevBuf<T> &buf, size_t count)
{
    HIPCHK(h, buf.grow(count));
    return F110_OK;
}

// a scratch buffer back at the capacity it had when the call began (a refusal leaves the device allocations as it found them)
template <typename T>
static int dshrink(f110_sim *h, DevBuf<T> &buf, size_t was)
{
    if (buf.capacity() == was) return F110_OK;
    if (!was) {
        buf.reset();
        return F110_OK;
    }
    HIPCHK(h, buf.alloc(was));
    return F110_OK;
}

#define TRY(expr)              \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != F110_OK) return rc_; \
    } while (0)

// The group streams' outstanding work becomes a dependency of the main stream (stream-ordered, no
// host wait).  Every entry point except the step itself starts with it, so the env groups are an
// internal detail: anything enqueued or read through the handle sees completed steps.
static int join_groups(f110_sim *h)
{
    if (h->comm_inflight) {   // an overlapped gather: whatever follows on the main stream sees its result
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gather_done[0], 0));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gather_done[1], 0));
        h->comm_inflight = false;
    }
    if (!h->groups_busy) return F110_OK;
    for (size_t g = 0; g < h->gstreams.size(); ++g) {
        if (h->gstreams[g] == h->stream) continue;
        HIPCHK(h, hipEventRecord(h->gevents[g], h->gstreams[g]));
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->gevents[g], 0));
    }
    h->groups_busy = false;
    return F110_OK;
}

// first statement (after the null check) of every entry point that takes a handle: calls may come
// from any thread, so the handle's device is made current; group streams are joined; whatever the
// call enqueues on the main stream must be waited for by the next step's groups.
#define ENTER(h)                                          \
    do {                                                  \
        HIPCHK(h, hipSetDevice((h)->cfg.device_id));      \
        TRY(join_groups(h));                              \
        (h)->main_dirty = true;                           \
        (h)->touched = true;                              \
    } while (0)

static int track_invalidate(f110_sim *h);     // (below, with the track entry points)
static int track_prepare(f110_sim *h);
static int track_launch(f110_sim *h, hipStream_t st, int mode, int begin, int count);
static bool tiny_applies(const f110_sim *h);   // (below, with the step)
static void noise_release(f110_sim *h);        // (below, with the noise entry points)
static void sampler_release(f110_sim *h);      // (below, with the reset sampler)
static int sampler_launch(f110_sim *h, hipStream_t st, int mode, int e0, int count, const uint8_t *d_mask, int ego);
static int reseat_launch(f110_sim *h, hipStream_t st, int mode, int e0, int count, int ego);   // (below, with the parameter sampler)
// does anything draw behind a re-seat?  (a reset sampler, a parameter sampler, or both)
static inline bool reseat_draws(const f110_sim *h) { return h->rs.on || h->ps.on; }
// the step behind f110_step_device, f110_step_host and f110_episode_step_* (below, with step_range); host_written: the step's
// own kernel wrote the caller's host block (rq.fuse / rq.hb were honoured)
static int step_submit(f110_sim *h, const double *d_actions, const StepRequest &rq, bool &host_written);

// ---- env blocks: on which streams, over which env ranges, does a call launch? -------------------------------
constexpr int kMaxEnvBlocks = 16;
struct EnvBlock { hipStream_t stream; int e0, count; };   // envs [e0, e0 + count) on `stream`
static void gap_launch_armed(f110_sim *h, const EnvBlock &b, double *d_actions);   // (below, with the controllers)
static int line_ready(f110_sim *h);                                                   // (below, with the line followers)
static void line_launch_armed(f110_sim *h, const EnvBlock &b, double *d_actions, double *d_info);
static int track_upload(f110_sim *h);
static int mppi_ready(f110_sim *h);                                                   // (below, with the planner)
static int mppi_launch_armed(f110_sim *h, const EnvBlock &b, double *d_actions, float *d_info);
static int mppi_upload_tracks(f110_sim *h);
struct EnvBlocks {
    EnvBlock b[kMaxEnvBlocks];
    int n = 0;
    const EnvBlock *begin() const { return b; }
    const EnvBlock *end() const { return b + n; }
};

// how the env axis is cut into `groups` blocks: whole envs, whole 64-agent waves where possible
static int group_envs(const f110_sim *h)
{
    const int E = h->cfg.num_envs, G = h->groups;
    int per = (E + G - 1) / G;
#ifdef F110_EXPERIMENTAL
    if (G == 2 && h->exp.group_split > 0) per = std::max(1, (int)((long long)E * h->exp.group_split / 100));   // probe: uneven halves
#endif
    if (per >= 64) per = (per + 63) / 64 * 64;
    return per;
}

// submit: every env block on its own stream (a grouped step, and the sampler draw behind it); empty blocks are dropped
static EnvBlocks env_blocks_submit(const f110_sim *h)
{
    EnvBlocks w;
    const int per = group_envs(h), E = h->cfg.num_envs;
    for (int g = 0; g < h->groups && g * per < E; ++g) w.b[w.n++] = EnvBlock{h->gstreams[g], g * per, std::min(per, E - g * per)};
    return w;
}

// the whole batch on the main stream
static EnvBlocks env_blocks_main(const f110_sim *h)
{
    EnvBlocks w;
    w.b[w.n++] = EnvBlock{h->stream, 0, h->cfg.num_envs};
    return w;
}

// follow: a device-resident call behind the step.  Right behind a two-block step (nothing else through the handle since) it
// rides the two blocks, each on the block's own stream, without a join; otherwise it is an ordinary entry point (ENTER) on
// the main stream.  A caller whose work reads per env / per agent only ends with `h->touched = false`: the next step may
// split again (it forks from what the call left on the main stream: main_dirty); behind the blocks touched is false already.
static int env_blocks_follow(f110_sim *h, EnvBlocks &w)
{
    if (h->last_blocks == 2 && h->groups_busy && !h->touched) {   // (two blocks went out: groups == 2)
        HIPCHK(h, hipSetDevice(h->cfg.device_id));
        w = env_blocks_submit(h);
        return F110_OK;
    }
    ENTER(h);
    w = env_blocks_main(h);
    return F110_OK;
}

// A device form with a per-agent float32 output d_out [N][per_agent], over the blocks env_blocks_follow gave it: launch(b) per
// block, then (h_pinned set) the block's slice into the caller's page-locked copy on the block's stream, remembered for
// f110_host_free.  Ends the call the way `follow` asks.  A new form of this kind is a spec check, a job fill, a launcher and
// an enumerator of PinnedDst.
template <typename Launch>
static int env_blocks_output(f110_sim *h, const EnvBlocks &w, PinnedDst who, size_t per_agent, const float *d_out, float *h_pinned, Launch launch)
{
    const size_t A = (size_t)h->cfg.num_agents;
    for (const EnvBlock &b : w) {
        launch(b);
        const size_t i0 = b.e0 * A * per_agent, n = b.count * A * per_agent;
        if (h_pinned) HIPCHK(h, hipMemcpyAsync(h_pinned + i0, d_out + i0, n * sizeof(float), hipMemcpyDeviceToHost, b.stream));
    }
    HIPCHK(h, hipGetLastError());
    if (h_pinned) h->pinned_dst[who] = h_pinned;
    h->touched = false;
    return F110_OK;
}

// RAII scratch for the unit entry points: the device buffers of one call, what has to come back from them, and the call's one
// synchronise.  Each operation returns the device pointer, so the job's field is assigned where its buffer is made.  A null host
// pointer is an optional input or output: nullptr comes back and nothing is allocated.  The first failed allocation or copy is
// reported (fail(), under the entry point's name) and kept; whatever is asked afterwards returns nullptr and does nothing.  So
// every function that owns or is handed a Scratch calls TRY(s.ready()) once, behind its last allocation and before its first
// launch, memset or other device-side use of a scratch pointer: no kernel is ever handed a pointer of a failed call.  A new unit
// form is a spec check, in / out lines that fill the job, ready, a launcher and finish.  Host memory that `in` read or that
// finish() writes must live until finish() has returned.
struct Scratch {
    struct Back { void *host; const void *dev; size_t bytes; };
    f110_sim *h;
    const char *who;
    DevArena mem;
    std::vector<Back> back;   // the device-to-host copies finish() makes, in the order they were asked for
    int rc = F110_OK;
    explicit Scratch(f110_sim *hh, const char *name = __builtin_FUNCTION()) : h(hh), who(name) {}

    // allocation only
    template <typename T>
    T *tmp(size_t count)
    {
        T *p = nullptr;
        if (rc != F110_OK) return nullptr;
        const hipError_t e = mem.alloc(&p, count);
        if (e != hipSuccess) rc = fail(h, F110_ERR_HIP, "%s: a scratch allocation of %zu bytes failed: %s", who, count * sizeof(T), hipGetErrorString(e));
        return p;
    }
    // allocation and the host rows into it, on the handle's stream
    template <typename T>
    T *in(const T *host, size_t count)
    {
        T *p = host ? tmp<T>(count) : nullptr;
        if (!p) return nullptr;
        const hipError_t e = hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) rc = fail(h, F110_ERR_HIP, "%s: a copy to scratch memory failed: %s", who, hipGetErrorString(e));
        return rc == F110_OK ? p : nullptr;
    }
    // allocation that finish() copies into the host rows
    template <typename T>
    T *out(T *host, size_t count)
    {
        T *p = host ? tmp<T>(count) : nullptr;
        later(host, p, count);
        return p;
    }
    // in and out of the same host rows
    template <typename T>
    T *inout(T *host, size_t count)
    {
        T *p = in(host, count);
        later(host, p, count);
        return p;
    }
    // finish() copies `dev`, a buffer that exists anyway, into the host rows (none: nothing)
    template <typename T>
    void later(T *host, const T *dev, size_t count)
    {
        if (host && dev && rc == F110_OK) back.push_back(Back{host, dev, count * sizeof(T)});
    }
    int ready() const { return rc; }
    // behind the last launch: the launches' status, the copies back and the call's one synchronise
    int finish()
    {
        TRY(rc);
        HIPCHK(h, hipGetLastError());
        for (const Back &b : back) HIPCHK(h, hipMemcpyAsync(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return F110_OK;
    }
};

static inline bool padded_family(int layout) { return layout == F110_MAP_PADDED_F64; }

static inline dim3 grid1d(size_t n, int block) { return dim3((unsigned)((n + block - 1) / block)); }

// the kernel families of the step, by signature (the pickers below return these)
typedef void (*scan_rays_fn)(RayJob, ScanConst);
typedef void (*scan_agent_fn)(RayJob, ScanConst, const MapFast *, const ScanConst *, uint32_t);   // k_scan_rays_agent, k_scan_dirs_agent
typedef void (*finalize_fn)(AgentArrays, int32_t);
typedef void (*finalize_multi_fn)(AgentArrays, int32_t, int);
typedef void (*step_tiny_fn)(AgentArrays, ScanConst, RayJob, const double *, TinyCtl, EpisodeArrays, HostBlock, int, int);
static int copy_col(f110_sim *h, double *dst, const double *src, size_t n);

// ray / B by multiply-high: find (magic, shift) with umulhi(x, magic) >> shift == x / B for every
// x < n (verified at every multiple of B and its predecessor, which is sufficient because both
// sides are monotone step functions of x).  Returns false when no 32-bit magic works.
static bool find_div_magic(uint32_t B, uint32_t n, uint32_t *magic, uint32_t *shift)
{
    if (B < 2) return false;
    for (uint32_t s = 0; s < 32; ++s) {
        const unsigned long long m = ((1ull << (32 + s)) + B - 1) / B;  // ceil(2^(32+s) / B)
        if (m >> 32) break;
        bool ok = true;
        for (unsigned long long x = B; ok && x <= (unsigned long long)n + B; x += B) {
            const unsigned long long xs[2] = {x - 1, x};
            for (unsigned long long v : xs) {
                if (v >= n) continue;
                if ((((v * m) >> 32) >> s) != v / B) ok = false;
            }
        }
        if (ok) {
            *magic = (uint32_t)m;
            *shift = s;
            return true;
        }
    }
    return false;
}

static void set_div_magic(RayJob &j, uint32_t B)
{
    uint32_t m = 0, s = 0;
    if (find_div_magic(B, j.n_rays, &m, &s)) {
        j.div_magic = m;
        j.div_shift = s;
    } else {
        j.div_magic = 0;
        j.div_shift = 0;
    }
}


// the device copy of h->k, brought up to date (stream-ordered) if any field changed
static const ScanConst *cold_consts(f110_sim *h)
{
    if (!h->d_k && h->d_k.alloc(1) != hipSuccess) return nullptr;
    if (std::memcmp(&h->k, &h->k_uploaded, sizeof(ScanConst)) != 0) {
        std::memcpy(&h->k_uploaded, &h->k, sizeof(ScanConst));
        if (hipMemcpyAsync(h->d_k, &h->k_uploaded, sizeof(ScanConst), hipMemcpyHostToDevice, h->stream) != hipSuccess) return nullptr;
    }
    return h->d_k;
}

// the RayJob fields that every form of the step sets alike (step_scan, step_tiny)
static int ray_job_step_fields(f110_sim *h, RayJob &j)
{
    j.noise = h->dev.noise;
    j.ttc_side_max = h->ttc_side_max;
    j.ttc_k = h->dev.ttc_thresh * (1.0 + 1e-9) * h->ttc_cos_max;
    j.beam_cos = h->dev.beam_cos;
    j.side_dist = h->dev.side_dist;
    j.ttc_thresh = h->dev.ttc_thresh;
    j.k_cold = cold_consts(h);
    if (!j.k_cold) return fail(h, F110_ERR_HIP, "f110_step_device: constant upload failed");
    return F110_OK;
}

// The step's scan runs agent-aligned (k_scan_rays_agent) with the PADDED layout unless that would
// leave more than 3 % of the lanes idle (few beams); exp.scan_flat forces the flat kernel (A/B).
static bool agent_aligned(const f110_sim *h)
{
    if (h->exp.scan_flat || !padded_family(h->cfg.map_layout) || !h->k.pad || h->dir_stride > 0) return false;
    const int B = h->k.num_beams, lanes = (B + 63) / 64 * 64;
    return (lanes - B) * 100 <= 3 * B;
}

template <bool STEP>
static scan_rays_fn pick_rays(const ScanConst &k, int layout)
{
#define SEL(L) (k.res_pow2 ? (k.ident_rot ? k_scan_rays<L, true, true, STEP> : k_scan_rays<L, true, false, STEP>) \
                           : (k.ident_rot ? k_scan_rays<L, false, true, STEP> : k_scan_rays<L, false, false, STEP>))
    if (padded_family(layout) && k.pad) return SEL(LAYOUT_PADDED);
    return SEL(LAYOUT_ROWMAJOR);
#undef SEL
}

static dim3 rays_grid(RayJob &j, int block, int tasks_per_wave)
{
    j.n_tasks = (j.n_rays + 63u) / 64u;
    j.tasks_per_wave = tasks_per_wave > 0 ? (uint32_t)tasks_per_wave : 1u;
    const uint32_t waves = (j.n_tasks + j.tasks_per_wave - 1) / j.tasks_per_wave;
    const uint32_t wpb = (uint32_t)block / 64u;
    return dim3((waves + wpb - 1) / wpb);
}

// longest-first order of the step's scan tasks (TaskSched): buffers on first use, then on / off
static int task_order_setup(f110_sim *h, bool on)
{
    const size_t n_tasks = (size_t)h->N * (((size_t)h->cfg.num_beams + 63) / 64);
    if (!on || n_tasks >= 0x7fffffffu) {
        h->task_order = false;
        return F110_OK;
    }
    if (!h->sched_allocated) {
        h->sched_mem.clear();   // (an earlier attempt that ran out of memory half-way)
        h->task_cap_alloc = (uint32_t)std::max<size_t>(64, kExperimental ? n_tasks : n_tasks / h->task_cap_div);
        for (int q = 0; q < 2; ++q) {
            TRY(dmalloc(h, h->sched_mem, &h->d_tflags[q], n_tasks));
            TRY(dmalloc(h, h->sched_mem, &h->d_tlist[q], (size_t)h->task_cap_alloc));
            HIPCHK(h, hipMemsetAsync(h->d_tflags[q], 0, sizeof(uint32_t) * n_tasks, h->stream));
        }
        TRY(dmalloc(h, h->sched_mem, &h->d_tcount, 4));   // {task count of parity 0, of parity 1, spare, spare}
        HIPCHK(h, hipMemsetAsync(h->d_tcount, 0, 4 * sizeof(uint32_t), h->stream));
        h->sched_allocated = true;
    }
    h->task_cap = std::min<uint32_t>(h->task_cap_alloc, (uint32_t)std::max<size_t>(64, n_tasks / h->task_cap_div));
    for (int q = 0; q < 2; ++q)   // struct q is used at steps of parity q: it reads what parity q^1 wrote
        h->tsched[q] = TaskSched{h->d_tflags[q ^ 1], h->d_tflags[q], h->d_tlist[q ^ 1], h->d_tlist[q], h->d_tcount + (q ^ 1), h->d_tcount + q, h->task_cap, h->task_thr, {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, 0u, 0u};
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->task_order = true;
    return F110_OK;
}

static int finish_map(f110_sim *h, int H, int W, double res, double ox, double oy, double oc, double os);   // (below, with the map)

// Slot 0's table is replaced by a fresh row-major one of n cells, which fill(table) enqueues the contents of.  Once the old
// table is gone, a failure leaves the handle WITHOUT a map: it refuses a step ("Map is not set") instead of reading freed memory.
template <typename Fill>
static int replace_map(f110_sim *h, size_t n, int H, int W, double res, double ox, double oy, double oc, double os, Fill fill)
{
    const auto unset = [h](int rc) {
        h->has_map = false;
        h->k.table = h->k.table_rm = nullptr;
        h->k.pad = nullptr;
        return rc;
    };
    const bool freed = h->d_dt_row != nullptr;
    int rc = dmalloc(h, &h->d_dt_row, n);
    if (rc != F110_OK) return freed ? unset(rc) : rc;
    rc = fill(h->d_dt_row.get());
    if (rc == F110_OK) rc = finish_map(h, H, W, res, ox, oy, oc, os);
    return rc == F110_OK ? rc : unset(rc);
}

extern "C" {

const char *f110_last_error(const f110_sim *h) { return (h && h->err[0]) ? h->err : g_err; }
int f110_abi_version(void) { return F110_ABI_VERSION; }

int f110_device_allocs(int64_t *live, int64_t *bytes)
{
    if (live) *live = devmem::g_live.load();
    if (bytes) *bytes = devmem::g_bytes.load();
    return F110_OK;
}

int f110_device_count(int *count)
{
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        if (count) *count = 0;
        return fail(nullptr, F110_ERR_HIP, "hipGetDeviceCount failed: %s", hipGetErrorString(e));
    }
    if (count) *count = n;
    return F110_OK;
}

int f110_device_pci_bus_id(int32_t device, char *out, int32_t len)
{
    if (!out || len < 16) return fail(nullptr, F110_ERR_INVALID, "f110_device_pci_bus_id: buffer of at least 16 bytes required");
    const hipError_t e = hipDeviceGetPCIBusId(out, len, device);
    if (e != hipSuccess) return fail(nullptr, F110_ERR_HIP, "hipDeviceGetPCIBusId(%d) failed: %s", device, hipGetErrorString(e));
    return F110_OK;
}

#ifndef F110_SRC_HASH
#define F110_SRC_HASH "unknown"
#endif
const char *f110_build_info(void) { return "csrc=" F110_SRC_HASH; }

int f110_is_experimental(void) { return kExperimental ? 1 : 0; }

int f110_exp_set(f110_sim *h, const char *key, int32_t value)
{
    if (!h || !key) return fail(h, F110_ERR_INVALID, "null argument");
    if (!kExperimental) return fail(h, F110_ERR_STATE, "f110_exp_set(%s) is available in the experimental build only (libf110_hip_exp.so)", key);
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const std::string k(key);
    if (k == "scan_flat") h->exp.scan_flat = value;
    else if (k == "long_prio") h->exp.long_prio = value;
    else if (k == "scan_occupancy") h->exp.scan_occupancy = value;
    else if (k == "scan_env_counter") h->exp.scan_env_counter = value;
    else if (k == "integrate_duo") h->exp.integrate_duo = value;
    else if (k == "integrate_fan") h->exp.integrate_fan = value;
    else if (k == "group_split") h->exp.group_split = value;
    else if (k == "step_tiny") h->tiny_off = value == 0 ? 1 : 0;
    else if (k == "tiny_start_probe") {   // 1: k_step_tiny's first workgroup reports its start to the host; 0: print launch -> start -> word and stop
        if (!value && h->exp.tiny_start_probe && h->exp.probe_calls)
            std::fprintf(stderr, "[tiny_start_probe] %ld steps: call -> launched %.2f us, launched -> first wave seen %.2f us, first wave seen -> completion word seen %.2f us\n",
                         h->exp.probe_calls, h->exp.probe_us[0] / h->exp.probe_calls, h->exp.probe_us[1] / h->exp.probe_calls, h->exp.probe_us[2] / h->exp.probe_calls);
        h->exp.tiny_start_probe = value;
        h->exp.probe_calls = 0;
        h->exp.probe_us[0] = h->exp.probe_us[1] = h->exp.probe_us[2] = 0;
    }
    else if (k == "pair_wave") h->exp.pair_wave = value;
    else if (k == "tiny_general_tail") h->exp.tiny_general_tail = value;   // 1: one env of two cars finishes in finalize_pair_body (the tail before finalize_duo_tiny)
    else if (k == "tiny_trace_hi") h->exp.tiny_trace = (h->exp.tiny_trace & 0xffffffffull) | ((uint64_t)(uint32_t)value << 32);
    else if (k == "tiny_trace_lo") h->exp.tiny_trace = (h->exp.tiny_trace & ~0xffffffffull) | (uint64_t)(uint32_t)value;
    else if (k == "scan_trace_hi") h->exp.scan_trace = (h->exp.scan_trace & 0xffffffffull) | ((uint64_t)(uint32_t)value << 32);
    else if (k == "scan_trace_lo") h->exp.scan_trace = (h->exp.scan_trace & ~0xffffffffull) | (uint64_t)(uint32_t)value;
    else if (k == "collide_mode") {
        if (value < 0 || value > 3) return fail(h, F110_ERR_INVALID, "collide_mode must be 0..3");
        h->collide_mode = value;
    }
    else if (k == "task_order") return task_order_setup(h, value != 0);
    else if (k == "task_cap_div" || k == "task_rev") {
        if (k == "task_rev") h->task_rev = value != 0;
        else h->task_cap_div = (uint32_t)std::max(1, value);
        if (h->task_order) return task_order_setup(h, true);
    } else if (k == "task_thr") {
        h->task_thr = (uint32_t)value;
        if (h->task_order) return task_order_setup(h, true);
    }
    else if (k == "pad_tiled" || k == "scan_nt" || k == "finalize_wave" || k == "spec_from" || k == "scan_stream" || k == "stream_refill" || k == "stream_block" ||
             k == "stream_grid")
        return fail(h, F110_ERR_INVALID, "f110_exp_set: '%s' was retired in round 6 with the variant it switched (DESIGN.md section 8)", key);
    else
        return fail(h, F110_ERR_INVALID, "f110_exp_set: unknown key '%s'", key);
    return F110_OK;
}

static void default_beam_tables(const f110_config &c, std::vector<double> &sa, std::vector<double> &co, std::vector<double> &sd)
{
    // base_classes.py:125-158 (the Python host normally overrides these with NumPy's values)
    const int B = c.num_beams;
    const double incr = c.fov / (B - 1);
    const double dist_sides = c.params[F110_P_WIDTH] / 2., dist_fr = (c.params[F110_P_LF] + c.params[F110_P_LR]) / 2.;
    sa.resize(B); co.resize(B); sd.resize(B);
    for (int i = 0; i < B; ++i) {
        const double angle = -c.fov / 2. + i * incr;
        double to_side, to_fr;
        sa[i] = angle;
        co[i] = std::cos(angle);
        if (angle > 0) {
            if (angle < kPi / 2) { to_side = dist_sides / std::sin(angle); to_fr = dist_fr / std::cos(angle); }
            else { to_side = dist_sides / std::cos(angle - kPi / 2.); to_fr = dist_fr / std::sin(angle - kPi / 2.); }
        } else {
            if (angle > -kPi / 2) { to_side = dist_sides / std::sin(-angle); to_fr = dist_fr / std::cos(-angle); }
            else { to_side = dist_sides / std::cos(-angle - kPi / 2); to_fr = dist_fr / std::sin(-angle - kPi / 2); }
        }
        sd[i] = to_side < to_fr ? to_side : to_fr;
    }
}

// f110_kernels.hpp "do two streams make progress independently of each other?"; *yes is false whenever in doubt
static hipError_t streams_concurrent(hipStream_t a, hipStream_t b, bool *yes)
{
    *yes = false;
    DevBuf<unsigned> d;
    unsigned hres[2] = {0u, 0u};
    hipError_t e = d.alloc(2);
    if (e != hipSuccess) return e;
    do {
        if ((e = hipMemsetAsync(d, 0, 2 * sizeof(unsigned), a)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(a)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(b)) != hipSuccess) break;
        hipLaunchKernelGGL(k_probe_wait, dim3(1), dim3(1), 0, a, d, d + 1, 30000ull);   // at most 300 us
        hipLaunchKernelGGL(k_probe_set, dim3(1), dim3(1), 0, b, d);
        if ((e = hipStreamSynchronize(a)) != hipSuccess) break;
        if ((e = hipStreamSynchronize(b)) != hipSuccess) break;
        if ((e = hipMemcpy(hres, d, sizeof hres, hipMemcpyDeviceToHost)) != hipSuccess) break;
        *yes = hres[1] != 0u;
    } while (0);
    return e;
}

// live handles and page-locked blocks: f110_step_host caches the device view of the host block it validated, keyed by
// host pointers — a block that is freed must drop every handle's cache of it, or a later allocation at the same addresses would
// be stepped into through stale device pointers
static std::mutex g_registry_mu;
static std::set<f110_sim *> g_handles;
static std::map<const char *, size_t> g_host_blocks;

// does ONE f110_host_alloc block (the one that starts at or below p) hold all of [p, p + bytes)?
static bool pinned_block_holds(const void *p, size_t bytes)
{
    std::lock_guard<std::mutex> lk(g_registry_mu);
    const char *q = static_cast<const char *>(p);
    auto it = g_host_blocks.upper_bound(q);
    if (it == g_host_blocks.begin()) return false;
    --it;
    return q + bytes <= it->first + it->second;
}

int f110_create(const f110_config *cfg, f110_sim **out)
{
    if (!cfg || !out) return fail(nullptr, F110_ERR_INVALID, "f110_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != F110_ABI_VERSION) return fail(nullptr, F110_ERR_INVALID, "ABI version mismatch (%d vs %d)", cfg->abi_version, F110_ABI_VERSION);
    if (cfg->num_envs < 1 || cfg->num_agents < 1 || cfg->num_beams < 2 || cfg->theta_dis < 2)
        return fail(nullptr, F110_ERR_INVALID, "f110_create: num_envs/num_agents >= 1, num_beams/theta_dis >= 2 required");
    if (cfg->integrator != F110_INTEGRATOR_RK4 && cfg->integrator != F110_INTEGRATOR_EULER)
        return fail(nullptr, F110_ERR_INVALID, "Invalid Integrator Specified. Please choose RK4 or Euler");
    if (cfg->map_layout == F110_MAP_TILED_F64 || cfg->map_layout == F110_MAP_CODE8 || cfg->map_layout == F110_MAP_WINDOW_LDS)
        return fail(nullptr, F110_ERR_INVALID, "map_layout %d (4x4 tiles / byte codes + LUT / LDS window) was measured slower in rounds 1-4 and retired in round 5: "
                    "use F110_MAP_PADDED_F64 (3) or F110_MAP_ROWMAJOR_F64 (0)", cfg->map_layout);
    if (cfg->map_layout != F110_MAP_ROWMAJOR_F64 && cfg->map_layout != F110_MAP_PADDED_F64)
        return fail(nullptr, F110_ERR_INVALID, "unknown map_layout %d", cfg->map_layout);
    if (cfg->step_graph != 0)
        return fail(nullptr, F110_ERR_INVALID, "step_graph (the step as one captured HIP graph) was measured slower (graph launch ~250 us on ROCm 7.2) and retired in round 5");
    if (!kExperimental && cfg->step_groups > 2)
        return fail(nullptr, F110_ERR_STATE, "step_groups > 2 is available in the experimental build only (libf110_hip_exp.so)");
    if ((long long)cfg->num_envs * cfg->num_agents * (long long)cfg->num_beams > 0xFFFFFF00LL) return fail(nullptr, F110_ERR_INVALID, "num_envs*num_agents*num_beams must stay below 2^32");
    int ndev = 0;
    {
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev < 1)
            return fail(nullptr, F110_ERR_HIP, "no usable HIP device (%s); libf110_hip has no CPU fallback",
                        e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    }
    if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, F110_ERR_INVALID, "device_id %d out of range (%d devices)", cfg->device_id, ndev);
    f110_sim *h = new (std::nothrow) f110_sim();
    if (!h) return fail(nullptr, F110_ERR_NOMEM, "out of host memory");
    h->cfg = *cfg;
    h->N = cfg->num_envs * cfg->num_agents;
    const int N = h->N, B = cfg->num_beams;
    h->scan_block = cfg->scan_block > 0 ? cfg->scan_block : 64;
    if (cfg->scan_block <= 0 && cfg->map_layout == F110_MAP_CODE8) h->scan_block = 256;
    if (h->scan_block % 64 != 0 || h->scan_block > 256) { delete h; return fail(nullptr, F110_ERR_INVALID, "scan_block must be 64, 128, 192 or 256"); }
#define CK(expr) do { int rc_ = (expr); if (rc_ != F110_OK) { snprintf(g_err, sizeof g_err, "%s", h->err); f110_destroy(h); return rc_; } } while (0)
#define CKH(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { fail(nullptr, F110_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); f110_destroy(h); return F110_ERR_HIP; } } while (0)
    CKH(hipSetDevice(cfg->device_id));
    {
        hipDeviceProp_t prop;
        CKH(hipGetDeviceProperties(&prop, cfg->device_id));
        h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    if (cfg->scan_tasks_per_wave > 0) {
        h->scan_tasks_per_wave = cfg->scan_tasks_per_wave;
        h->scan_tasks_agent = cfg->scan_tasks_per_wave;
        h->scan_env_order = cfg->scan_tasks_per_wave > 1 && cfg->num_agents > 1;   // the caller groups tasks: the grouping that can share
    } else {
        // default: 3 consecutive tasks per wave once the batch fills every wave slot ~8 times over
        // (amortises the per-wave set-up); small batches are bound by their longest rays and want
        // the finer granularity (4096 agents: +5 %, 1024: +12 % with 1 task per wave).  Round 3, 3 / 4 / 6 / 8 / 17
        // tasks per wave: 65 536 agents 95.7 / 95.2 / 95.1 / 94.3 / 88.4 M agent-steps/s, 32 768: 87.6 / 86.2 / 85.9 / 83.3 / 77.9
        const size_t tasks = ((size_t)N * (size_t)B + 63) / 64, slots = (size_t)h->num_cus * 32;
        const size_t t = tasks / (slots * 8);
        h->scan_tasks_per_wave = t < 1 ? 1 : (t > 3 ? 3 : (int)t);
        h->scan_tasks_auto = true;
        // k_scan_rays_agent<.., ENV_ORDER> (an env's agents sector by sector, the noise sample kept while the key stays): two cars per
        // env, from the size at which waves take several tasks; an even count, so that no pair is split between two waves.
        // 2 / 3 / 4 tasks per wave in env order, ms per step (profiles/env_order_bench.txt; agent-major with 3 per wave in brackets):
        // 65 536 agents 0.6230 / 0.6358 / 0.6206 (0.6313), 49 152: 0.4963 / 0.5079 / 0.5001, 32 768: 0.3411 / 0.3504 / 0.3456 (0.3481),
        // 16 384: 0.1882 / 0.1908 / 0.1911 (0.1909).  Four cars per env LOSE in env order — 65 536 agents 0.7092 / 0.7280 / 0.7214
        // against 0.7062: a wave that walks four cars' same sector no longer walks one car's neighbouring sectors, whose rays
        // start in the same cells — so every other count keeps the agent-major order unless the caller sets the tasks per wave.
        h->scan_tasks_agent = h->scan_tasks_per_wave;
        if (cfg->num_agents == 2 && t >= 3) {
            h->scan_env_order = true;
            h->scan_tasks_agent = t >= 16 ? 4 : 2;
        }
    }
    CKH(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    CKH(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
    CKH(hipEventCreateWithFlags(&h->ev_integrated, hipEventDisableTiming));
    CKH(hipEventCreateWithFlags(&h->ev_collided, hipEventDisableTiming));
    CKH(hipEventCreate(&h->ev_begin));
    CKH(hipEventCreate(&h->ev_end));
    CKH(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
    {
        // env groups: envs are independent of each other, so two halves of the batch need not run in lockstep.
        // Steps that the caller enqueues back to back (f110_step_device, nothing else through the handle in between)
        // are submitted as two env blocks on two streams: one block's latency-bound kernels, tails and the VALU-bound
        // finalize run under the other block's texture-bound scan, and the blocks drift apart over consecutive steps.
        // 0 = automatic (two blocks when steps come back to back AND the size is one where it pays: env_blocks_pay),
        // 1 = always one block, 2 = always two (a caller that synchronises every
        // step pays ~25 us of fork / join for it), > 2 = experimental build.
        int G = cfg->step_groups;
        h->groups_auto = G <= 0;
        if (G <= 0) G = 2;
        G = std::min(std::min(G, kMaxEnvBlocks), cfg->num_envs);
        h->groups = G;
        // pair tests + opponent windows inside the finalize kernel: A = 2 (k_finalize_pair_roles) and every A up to
        // kMaxAgentsMulti = 256 (k_finalize_multi up to 16, k_finalize_multi_tiled above: an env's ordered pairs in tiles of a
        // workgroup's record table); above
        // that — no use case known — the round-1 form (k_collide on the side stream + k_finalize)
        h->collide_mode = (cfg->num_agents >= 2 && cfg->num_agents <= kMaxAgentsMulti) ? 3 : 0;
        // two groups: the main stream and ONE more stream that provably runs next to it.  Which hardware queue a stream
        // lands on depends on what else the process created before; a second stream on the main stream's queue turns
        // the gain (+2 .. +23 %) into a loss (-9 .. -50 %), so candidates are probed (k_probe_wait) — the side stream
        // first (unused by the in-kernel pair tests), then up to six fresh ones; with none, the step stays one block.
        const bool duo = G == 2 && (h->collide_mode == 3 || cfg->num_agents == 1);   // (the older forms launch k_collide on the side stream)
        if (h->groups_auto && !duo) G = h->groups = 1;
        if (duo) {
            hipStream_t second = nullptr;
            std::vector<hipStream_t> rejected;
            for (int attempt = 0; attempt < 7 && !second; ++attempt) {
                hipStream_t cand = h->side_stream;
                if (attempt > 0 && hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) {
                    (void)hipGetLastError();   // no more streams to be had: the search ends, the step stays one block
                    break;
                }
                bool yes = false;
                const hipError_t ep = streams_concurrent(h->stream, cand, &yes);
                if (ep == hipSuccess && yes) {
                    second = cand;
                    if (attempt > 0) h->gowned.push_back(cand);
                } else if (attempt > 0) {
                    rejected.push_back(cand);   // kept until the search ends, so that the next candidate lands elsewhere
                }
                h->group_probes = attempt + 1;
                if (ep != hipSuccess) break;
            }
            for (hipStream_t r : rejected) (void)hipStreamDestroy(r);
            if (!second) G = h->groups = 1;
            else {
                hipEvent_t ge = nullptr;
                h->gstreams.push_back(h->stream);
                h->gevents.push_back(nullptr);
                h->gstreams.push_back(second);
                CKH(hipEventCreateWithFlags(&ge, hipEventDisableTiming));
                h->gevents.push_back(ge);
            }
        }
        for (int g = 0; g < G && G > 1 && !duo; ++g) {
            hipStream_t gs = nullptr;
            hipEvent_t ge = nullptr;
            CKH(hipStreamCreateWithFlags(&gs, hipStreamNonBlocking));
            h->gowned.push_back(gs);
            h->gstreams.push_back(gs);
            CKH(hipEventCreateWithFlags(&ge, hipEventDisableTiming));
            h->gevents.push_back(ge);
        }
    }
    AgentArrays &d = h->dev;
    d.n_agents_total = N;
    d.agents_per_env = cfg->num_agents;
    d.agent_begin = 0;
    d.agent_count = N;
    CK(dmalloc(h, h->mem, &d.state, (size_t)7 * N));
    CK(dmalloc(h, h->mem, &d.steer_buf, (size_t)2 * N));
    CK(dmalloc(h, h->mem, &d.buf_cnt, (size_t)N));
    CK(dmalloc(h, h->mem, &d.scan_pose, (size_t)3 * N));
    CK(dmalloc(h, h->mem, &d.snap_pose, (size_t)3 * N));
    CK(dmalloc(h, h->mem, &d.dir_start, (size_t)N));
    CK(dmalloc(h, h->mem, &d.ray_hdr, (size_t)N));
    CK(dmalloc(h, &h->scan_bufs[0], (size_t)N * B));
    d.scans = h->scan_bufs[0];
    CK(dmalloc(h, h->mem, &d.collisions, (size_t)N));
    CK(dmalloc(h, h->mem, &d.collision_idx, (size_t)N));
    CK(dmalloc(h, h->mem, &d.in_collision, (size_t)N));
    CK(dmalloc(h, h->mem, &d.step_count, (size_t)N));
    CK(dmalloc(h, h->mem, &d.opp_window, (size_t)N * cfg->num_agents * 4));
    CK(dmalloc(h, h->mem, &d.opp_verts, (size_t)N * cfg->num_agents * 8));
    CK(dmalloc(h, h->mem, &h->d_params, (size_t)cfg->num_agents * NPARAMS));
    CK(dmalloc(h, h->mem, &h->d_scan_angles, (size_t)B));
    CK(dmalloc(h, h->mem, &h->d_beam_cos, (size_t)B));
    CK(dmalloc(h, h->mem, &h->d_side, (size_t)B));
    CK(dmalloc(h, h->mem, &h->d_cs, (size_t)cfg->theta_dis));
    CK(dmalloc(h, h->mem, &h->d_actions, (size_t)2 * N));
    CK(dmalloc(h, h->mem, &h->d_poses, (size_t)3 * N));
    CK(dmalloc(h, h->mem, &h->d_mask, (size_t)cfg->num_envs));
    {
        // constants of the device noise generator (f110_rng.hpp): NumPy's ziggurat tables and the
        // PCG64 jump constants, 8 KB in all
        PcgJump jt;
        pcg_jump_table(jt);
        CK(dmalloc(h, h->mem, &h->d_zig_k, 256));
        CK(dmalloc(h, h->mem, &h->d_zig_w, 256));
        CK(dmalloc(h, h->mem, &h->d_zig_f, 256));
        CK(dmalloc(h, h->mem, &h->d_jump, 2 * 65));
        CK(dmalloc(h, h->mem, &h->d_lookups, 2));
        CKH(hipMemcpy(h->d_zig_k, kZigK, sizeof kZigK, hipMemcpyHostToDevice));
        CKH(hipMemcpy(h->d_zig_w, kZigW, sizeof kZigW, hipMemcpyHostToDevice));
        CKH(hipMemcpy(h->d_zig_f, kZigF, sizeof kZigF, hipMemcpyHostToDevice));
        CKH(hipMemcpy(h->d_jump, jt.a, sizeof jt.a, hipMemcpyHostToDevice));
        CKH(hipMemcpy(h->d_jump + 65, jt.g, sizeof jt.g, hipMemcpyHostToDevice));
        CKH(hipMemsetAsync(h->d_lookups, 0, 2 * sizeof(unsigned long long), h->stream));
        h->noise_gen = NoiseGen{h->d_zig_k, h->d_zig_w, h->d_zig_f, h->d_jump, h->d_jump + 65, 0.0};
    }
    {
        // longest-first task order: for batches whose scan ends with its longest rays.  Window re-measured in round 3
        // with both kernels at 8 waves per SIMD (product kernel, list on / off): 512 agents 8.50 / 8.68 M agent-steps/s,
        // 1024: 15.4 / 15.2, 2048: 27.5 / 26.1, 4096: 43.7 / 39.9, 8192: 60.9 / 57.8, 12 288: 69.7 / 67.4,
        // 16 384: 75.2 / 73.6, 24 576: 81.0 / 83.0, 32 768: 82.6 / 86.3
        const size_t n_tasks = (size_t)N * (((size_t)B + 63) / 64);
#ifndef F110_TASK_ORDER_MAX_TASKS
#define F110_TASK_ORDER_MAX_TASKS 340000
#endif
        if (n_tasks >= 12000 && n_tasks < F110_TASK_ORDER_MAX_TASKS) CK(task_order_setup(h, true));
    }
    CKH(hipMemsetAsync(d.state, 0, sizeof(double) * 7 * N, h->stream));
    CKH(hipMemsetAsync(d.steer_buf, 0, sizeof(double) * 2 * N, h->stream));
    CKH(hipMemsetAsync(d.buf_cnt, 0, sizeof(int32_t) * N, h->stream));
    CKH(hipMemsetAsync(d.scan_pose, 0, sizeof(double) * 3 * N, h->stream));
    CKH(hipMemsetAsync(d.snap_pose, 0, sizeof(double) * 3 * N, h->stream));
    CKH(hipMemsetAsync(d.dir_start, 0, sizeof(double) * N, h->stream));
    CKH(hipMemsetAsync(d.scans, 0, sizeof(double) * (size_t)N * B, h->stream));
    CKH(hipMemsetAsync(d.collisions, 0, sizeof(double) * N, h->stream));
    CKH(hipMemsetAsync(d.in_collision, 0, sizeof(int32_t) * N, h->stream));
    CKH(hipMemsetAsync(d.step_count, 0, sizeof(int32_t) * N, h->stream));
    {
        std::vector<double> minus1(N, -1.0);  // collision_idx = -1 (base_classes.py:488)
        CKH(hipMemcpy(d.collision_idx, minus1.data(), sizeof(double) * N, hipMemcpyHostToDevice));
    }
    d.params = h->d_params;
    d.noise = nullptr;
    d.noise_rows = 0;
    d.scan_angles = h->d_scan_angles;
    d.beam_cos = h->d_beam_cos;
    d.side_dist = h->d_side;
    d.integrator = cfg->integrator;
    d.time_step = cfg->time_step;
    d.lidar_dist = cfg->lidar_dist;
    d.ttc_thresh = cfg->ttc_thresh;
    d.angle_inc = cfg->fov / (B - 1);  // laser_models.py:367
    d.box_length = cfg->params[F110_P_LENGTH];
    d.box_width = cfg->params[F110_P_WIDTH];
    // scan constants that do not depend on the map
    ScanConst &k = h->k;
    k.cs = h->d_cs;
    k.theta_dis = cfg->theta_dis;
    k.num_beams = B;
    k.eps = cfg->eps;
    k.max_range = cfg->max_range;
    k.fov = cfg->fov;
    k.theta_inc = cfg->theta_dis * d.angle_inc / (2. * kPi);  // :368
    k.inv_theta_dis = 1.0 / (double)cfg->theta_dis;
    {
        RayJob tmp{};
        tmp.n_rays = (uint32_t)N * (uint32_t)B;
        set_div_magic(tmp, (uint32_t)B);
        h->step_magic = tmp.div_magic;
        h->step_shift = tmp.div_shift;
    }
    {
        const double g = 64.0 * (double)B * 2.2737367544323206e-13;  // 64 * B * 2^-42
        k.dir_guard = g > 1e-8 ? g : 1e-8;
    }
    if (k.theta_inc < 1.0 && B >= 64) {
        // more beams than table directions: march each distinct direction once (k_scan_dirs_agent)
        int stride = (int)std::ceil((B - 1) * k.theta_inc) + 2;
        // The direction kernel walks an agent's beams in order of their table index RELATIVE to beam 0's, which must not wrap:
        // a scan that spans the whole table — fov close to a full turn, e.g. 6.28 with 1000 directions: (B - 1) theta_inc =
        // 999.5, plus the start's fraction — ends on beam 0's directions again and those beams were left unwritten (found by
        // round 5's fuzz over constructor arguments).  Such scans march every beam (k_scan_rays_agent).
        const bool wraps = (B - 1) * k.theta_inc + 1.0 >= (double)cfg->theta_dis;
        stride = std::min(stride, cfg->theta_dis);
        stride = (stride + 63) / 64 * 64;
        if (!wraps && stride < B && (long long)N * stride < 0xFFFFFF00LL) {
            h->dir_stride = stride;
        }
    }
    CK(f110_set_params(h, -1, cfg->params));
    {
        std::vector<double> s(cfg->theta_dis), c(cfg->theta_dis);
        for (int i = 0; i < cfg->theta_dis; ++i) {  // np.linspace(0, 2pi, theta_dis), laser_models.py:379
            const double th = i * (kTwoPi / (cfg->theta_dis - 1));
            s[i] = std::sin(th);
            c[i] = std::cos(th);
        }
        CK(f110_set_trig_tables(h, s.data(), c.data(), cfg->theta_dis));
        std::vector<double> sa, co, sd;
        default_beam_tables(*cfg, sa, co, sd);
        CK(f110_set_beam_tables(h, sa.data(), co.data(), sd.data(), B));
    }
    CKH(hipStreamSynchronize(h->stream));
#undef CK
#undef CKH
    {
        std::lock_guard<std::mutex> lk(g_registry_mu);
        g_handles.insert(h);
    }
    *out = h;
    return F110_OK;
}

void f110_destroy(f110_sim *h)
{
    if (!h) return;
    {   // first: no f110_host_free on another thread may look at this handle (or drain its streams) any more
        std::lock_guard<std::mutex> lk(g_registry_mu);
        g_handles.erase(h);
    }
    (void)hipSetDevice(h->cfg.device_id);
    for (hipStream_t gs : h->gstreams) (void)hipStreamSynchronize(gs);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    if (h->side_stream) (void)hipStreamSynchronize(h->side_stream);
    (void)f110_comm_destroy(h);
    h->comm_inflight = false;
    if (h->comm_stream) { (void)hipStreamSynchronize(h->comm_stream); (void)hipStreamDestroy(h->comm_stream); h->comm_stream = nullptr; }
    for (hipEvent_t e : {h->ev_step_done, h->ev_gather_done[0], h->ev_gather_done[1]})
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t gs : h->gowned) (void)hipStreamDestroy(gs);
    for (hipEvent_t ge : h->gevents)
        if (ge) (void)hipEventDestroy(ge);
    if (h->ev_main) (void)hipEventDestroy(h->ev_main);
    if (h->noise_stream) {   // rows generated ahead of need may still be in flight
        (void)hipStreamSynchronize(h->noise_stream);
        (void)hipStreamDestroy(h->noise_stream);
    }
    if (h->ev_noise) (void)hipEventDestroy(h->ev_noise);
    for (hipEvent_t e : h->corr.ev)
        if (e) (void)hipEventDestroy(e);
    if (h->ev_noise_src) (void)hipEventDestroy(h->ev_noise_src);
    if (h->hb_seq_host) (void)hipHostFree(h->hb_seq_host);
    for (hipEvent_t e : h->prof_events) (void)hipEventDestroy(e);
    if (h->ev_integrated) (void)hipEventDestroy(h->ev_integrated);
    if (h->ev_collided) (void)hipEventDestroy(h->ev_collided);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->ev_begin) (void)hipEventDestroy(h->ev_begin);
    if (h->ev_end) (void)hipEventDestroy(h->ev_end);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    // the device memory goes with the handle: every buffer is a DevBuf or sits in a DevArena (f110_devmem.hpp), so a feature
    // that adds one adds no line here.  All streams were synchronised above and this thread's device is the handle's.
    delete h;
}

int f110_sync(f110_sim *h)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

// ---- map ---------------------------------------------------------------------------------
// the per-map fields of ScanConst that do not involve device memory
static void fill_map_fields(ScanConst &k, int H, int W, double res, double ox, double oy, double oc, double os)
{
    k.height = H;
    k.width = W;
    k.row_bytes = W * 8;
    k.res = res;
    k.inv_res = 1.0 / res;
    {
        int e = 0;
        const double mant = std::frexp(res, &e);
        k.res_pow2 = (mant == 0.5) ? 1 : 0;
    }
    k.orig_x = ox;
    k.orig_y = oy;
    k.orig_c = oc;
    k.orig_s = os;
    k.ident_rot = (oc == 1.0 && os == 0.0) ? 1 : 0;
    k.w_res = W * res;  // width * resolution, laser_models.py:79
    k.h_res = H * res;
}

static int finish_map(f110_sim *h, int H, int W, double res, double ox, double oy, double oc, double os)
{
    ScanConst &k = h->k;
    h->multi_map = false;       // slot 0 changed: f110_set_env_maps has to be called again
    TRY(track_invalidate(h));
    h->dev.maps_full = nullptr;
    h->dev.env_map = nullptr;
    h->d_occ0.reset();   // a render rebuilds it from the new table
    fill_map_fields(k, H, W, res, ox, oy, oc, os);
    HIPCHK(h, hipMemcpyAsync(&k.oob_value, h->d_dt_row + ((size_t)H * W - 1), sizeof(double), hipMemcpyDeviceToHost, h->stream));
    k.table = h->d_dt_row;
    k.table_rm = h->d_dt_row;
    k.pad = nullptr;
    h->d_dt_pad.reset();
    if (padded_family(h->cfg.map_layout) && setup_padded(k)) {
        // the table again with a border of out-of-bounds cells wide enough for any ray of a lidar
        // that is on (or within kPadSlack cells of) the map; maps too large for 16-bit cell
        // coordinates keep k.pad == nullptr and run the plain row-major kernel
        const size_t total = (size_t)k.pad_width * k.pad_height;
        TRY(dmalloc(h, &h->d_dt_pad, total));
        hipLaunchKernelGGL(k_build_padded, grid1d(total, 256), dim3(256), 0, h->stream, h->d_dt_row, H, W, k.pad_border, k.pad_width, k.pad_height,
                           h->d_dt_pad);
        HIPCHK(h, hipGetLastError());
        k.pad = h->d_dt_pad;
        if (h->cfg.map_layout == F110_MAP_PADDED_F64) {
            // ONE table per map: the exact paths (k_integrate's first sample, the cold re-march, the unit
            // kernels) address dt[r][c] as table_rm + r * row_bytes + 8 c — point them at the interior of
            // the padded copy (its row pitch) and give the row-major original back (20.5 MB on example_map,
            // and the first sample now touches lines the march keeps hot)
            HIPCHK(h, hipStreamSynchronize(h->stream));
            k.table = k.table_rm = h->d_dt_pad + (size_t)k.pad_border * k.pad_width + k.pad_border;
            k.row_bytes = k.pad_row_bytes;
            h->d_dt_row.reset();
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->has_map = true;
    return F110_OK;
}

// The exact-EDT pipeline on a host image [H][W]: the image and the intermediates into scratch memory, then k_flip_threshold
// (threshold: a raw image, else a bitmap already), k_edt_columns, k_edt_rows and, with a table, k_dt_from_d2 at `res` into it.
// h_d2: the squared distances come back with the caller's finish().
static int edt_launch(Scratch &s, const uint8_t *h_img, int H, int W, bool threshold, uint32_t *h_d2, double res, double *table)
{
    f110_sim *h = s.h;
    const size_t n = (size_t)H * W;
    const uint8_t *d_img = s.in(h_img, n);
    uint8_t *d_bin = threshold ? s.tmp<uint8_t>(n) : nullptr;
    uint32_t *d_g = s.tmp<uint32_t>(n), *d_d2 = s.tmp<uint32_t>(n);
    s.later(h_d2, d_d2, n);
    TRY(s.ready());
    if (threshold) hipLaunchKernelGGL(k_flip_threshold, grid1d(n, 256), dim3(256), 0, h->stream, d_img, H, W, d_bin);
    hipLaunchKernelGGL(k_edt_columns, grid1d(W, 64), dim3(64), 0, h->stream, threshold ? d_bin : d_img, H, W, d_g);
    hipLaunchKernelGGL(k_edt_rows, dim3(H), dim3(256), (size_t)W * sizeof(uint32_t), h->stream, d_g, H, W, d_d2);
    if (table) hipLaunchKernelGGL(k_dt_from_d2, grid1d(n, 256), dim3(256), 0, h->stream, d_d2, n, res, table);
    return F110_OK;
}

int f110_set_map_image(f110_sim *h, const uint8_t *h_img, int32_t H, int32_t W, double res, double ox, double oy, double oyaw)
{
    if (!h || !h_img) return fail(h, F110_ERR_INVALID, "f110_set_map_image: null argument");
    ENTER(h);
    if (H < 1 || W < 1 || H > 16384 || W > 16384 || !(res > 0)) return fail(h, F110_ERR_INVALID, "f110_set_map_image: bad shape %dx%d or resolution", H, W);
    Scratch s(h);   // (lives until finish_map has synchronised)
    return replace_map(h, (size_t)H * W, H, W, res, ox, oy, std::cos(oyaw), std::sin(oyaw), [&](double *table) {  // :421-422
        TRY(edt_launch(s, h_img, H, W, true, nullptr, res, table));
        HIPCHK(h, hipGetLastError());
        return (int)F110_OK;
    });
}

int f110_set_map_dt(f110_sim *h, const double *h_dt, int32_t H, int32_t W, double res, double ox, double oy, double oc, double os)
{
    if (!h || !h_dt) return fail(h, F110_ERR_INVALID, "f110_set_map_dt: null argument");
    ENTER(h);
    if (H < 1 || W < 1 || !(res > 0)) return fail(h, F110_ERR_INVALID, "f110_set_map_dt: bad shape or resolution");
    if ((unsigned long long)(H + 3) * (unsigned long long)(W + 3) * 8ull >= 0xFFFFFFFFull) return fail(h, F110_ERR_INVALID, "distance table must stay below 4 GiB");
    const size_t n = (size_t)H * W;
    return replace_map(h, n, H, W, res, ox, oy, oc, os, [&](double *table) {
        HIPCHK(h, hipMemcpyAsync(table, h_dt, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
        return (int)F110_OK;
    });
}

// ---- a different track per env ---------------------------------------------------------------------
// the exact-EDT pipeline of f110_set_map_image into a fresh row-major table
static int edt_table_from_image(f110_sim *h, const uint8_t *h_img, int H, int W, double res, DevBuf<double> &d_dt_row)
{
    Scratch s(h);
    TRY(dmalloc(h, &d_dt_row, (size_t)H * W));
    TRY(edt_launch(s, h_img, H, W, true, nullptr, res, d_dt_row.get()));
    return s.finish();
}

// the row-major table becomes a slot: whatever fails, the table (and the slot's padded copy) go with the locals that own them
static int add_map_slot(f110_sim *h, DevBuf<double> &&table, int H, int W, double res, double ox, double oy, double oc, double os, int32_t *slot)
{
    f110_sim::MapSlot ms;
    ms.d_dt_row = std::move(table);
    double *const d_dt_row = ms.d_dt_row;
    ms.k = h->k;   // beam / trig / range constants are shared; the map fields follow
    fill_map_fields(ms.k, H, W, res, ox, oy, oc, os);
    ms.k.table = ms.k.table_rm = d_dt_row;
    HIPCHK(h, hipMemcpyAsync(&ms.k.oob_value, d_dt_row + ((size_t)H * W - 1), sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!setup_padded(ms.k)) return fail(h, F110_ERR_INVALID, "f110_add_map: a per-env map must fit the padded layout (16-bit cell coordinates, < 4 GiB)");
    const size_t total = (size_t)ms.k.pad_width * ms.k.pad_height;
    if (dmalloc(h, &ms.d_dt_pad, total) != F110_OK) return F110_ERR_NOMEM;
    hipLaunchKernelGGL(k_build_padded, grid1d(total, 256), dim3(256), 0, h->stream, d_dt_row, H, W, ms.k.pad_border, ms.k.pad_width,
                       ms.k.pad_height, ms.d_dt_pad);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ms.k.pad = ms.d_dt_pad;
    // one table per track (see finish_map): the exact paths read the padded copy's interior
    ms.k.table = ms.k.table_rm = ms.d_dt_pad + (size_t)ms.k.pad_border * ms.k.pad_width + ms.k.pad_border;
    ms.k.row_bytes = ms.k.pad_row_bytes;
    ms.d_dt_row.reset();
    h->extra_maps.push_back(std::move(ms));
    if (slot) *slot = (int32_t)h->extra_maps.size();   // slot 0 is the map of f110_set_map_*
    return F110_OK;
}

int f110_add_map_image(f110_sim *h, const uint8_t *h_img, int32_t H, int32_t W, double res, double ox, double oy, double oyaw, int32_t *slot)
{
    if (!h || !h_img) return fail(h, F110_ERR_INVALID, "f110_add_map_image: null argument");
    ENTER(h);
    if (H < 1 || W < 1 || H > 16384 || W > 16384 || !(res > 0)) return fail(h, F110_ERR_INVALID, "f110_add_map_image: bad shape %dx%d or resolution", H, W);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    DevBuf<double> d_dt_row;
    TRY(edt_table_from_image(h, h_img, H, W, res, d_dt_row));
    return add_map_slot(h, std::move(d_dt_row), H, W, res, ox, oy, std::cos(oyaw), std::sin(oyaw), slot);
}

int f110_add_map_dt(f110_sim *h, const double *h_dt, int32_t H, int32_t W, double res, double ox, double oy, double oc, double os, int32_t *slot)
{
    if (!h || !h_dt) return fail(h, F110_ERR_INVALID, "f110_add_map_dt: null argument");
    ENTER(h);
    if (H < 1 || W < 1 || !(res > 0)) return fail(h, F110_ERR_INVALID, "f110_add_map_dt: bad shape or resolution");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    DevBuf<double> d_dt_row;
    TRY(dmalloc(h, &d_dt_row, (size_t)H * W));
    HIPCHK(h, hipMemcpyAsync(d_dt_row, h_dt, (size_t)H * W * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return add_map_slot(h, std::move(d_dt_row), H, W, res, ox, oy, oc, os, slot);
}

int f110_set_env_maps(f110_sim *h, const int32_t *h_env_map)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    TRY(track_invalidate(h));   // the slots change under the cached s
    if (!h_env_map) {   // back to one map for everybody
        h->multi_map = false;
        h->dev.maps_full = nullptr;
        h->dev.env_map = nullptr;
        return F110_OK;
    }
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (!padded_family(h->cfg.map_layout) || !h->k.pad)
        return fail(h, F110_ERR_STATE, "f110_set_env_maps needs map_layout = F110_MAP_PADDED_F64 and a slot-0 map that fits it");
    const int E = h->cfg.num_envs, M = 1 + (int)h->extra_maps.size();
    for (int e = 0; e < E; ++e)
        if (h_env_map[e] < 0 || h_env_map[e] >= M) return fail(h, F110_ERR_INVALID, "f110_set_env_maps: env %d -> slot %d, but %d maps are registered", e, h_env_map[e], M);
    std::vector<ScanConst> full(M);
    std::vector<MapFast> fast(M);
    for (int m = 0; m < M; ++m) {
        full[m] = m == 0 ? h->k : h->extra_maps[m - 1].k;
        // constants that may have changed since a slot was added (trig / beam tables) are global
        full[m].cs = h->k.cs;
        fast[m].pad = full[m].pad;
        fast[m].pad_cx = full[m].pad_cx;
        fast[m].pad_cy = full[m].pad_cy;
        fast[m].pad_axx = full[m].pad_axx;
        fast[m].pad_axy = full[m].pad_axy;
        fast[m].pad_ayx = full[m].pad_ayx;
        fast[m].pad_ayy = full[m].pad_ayy;
        fast[m].pad_row_bytes = (uint32_t)full[m].pad_row_bytes;
        fast[m].pad_max_samples = full[m].pad_max_samples;
    }
    h->d_maps_fast.reset();
    h->d_maps_full.reset();
    if (!h->d_env_map) TRY(dmalloc(h, &h->d_env_map, (size_t)E));
    TRY(dmalloc(h, &h->d_maps_fast, (size_t)M));
    h->n_maps_dev = 0;
    TRY(dmalloc(h, &h->d_maps_full, (size_t)M));
    h->n_maps_dev = M;
    HIPCHK(h, hipMemcpyAsync(h->d_maps_fast, fast.data(), sizeof(MapFast) * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_maps_full, full.data(), sizeof(ScanConst) * M, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_env_map, h_env_map, sizeof(int32_t) * E, hipMemcpyHostToDevice, h->stream));
    {
        // the scan's agent order: by map slot (stable), so each XCD's contiguous share of the launch touches as few
        // tables as possible — interleaved assignments then cost what grouped ones do (measured, 8 tracks x 65 536
        // agents: interleaved 1.075 ms per step in agent order, grouped 0.738)
        const int A = h->cfg.num_agents;
        std::vector<uint32_t> order((size_t)h->N);
        for (int i = 0; i < h->N; ++i) order[i] = (uint32_t)i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return h_env_map[a / A] < h_env_map[b / A]; });
        bool identity = true;
        for (int i = 0; i < h->N && identity; ++i) identity = order[i] == (uint32_t)i;
        h->d_scan_order.reset();
        if (!identity) {
            TRY(dmalloc(h, &h->d_scan_order, (size_t)h->N));
            HIPCHK(h, hipMemcpyAsync(h->d_scan_order, order.data(), sizeof(uint32_t) * h->N, hipMemcpyHostToDevice, h->stream));
        }
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->dev.maps_full = h->d_maps_full;
    h->dev.env_map = h->d_env_map;
    h->multi_map = true;
    h->env_map_host.assign(h_env_map, h_env_map + E);
    return F110_OK;
}

int f110_get_map_dt(f110_sim *h, double *out)
{
    if (!h || !out) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    const size_t row = (size_t)h->k.width * sizeof(double);
    if (h->d_dt_row)
        HIPCHK(h, hipMemcpyAsync(out, h->d_dt_row, (size_t)h->k.height * row, hipMemcpyDeviceToHost, h->stream));
    else   // the table lives inside its padded copy only
        HIPCHK(h, hipMemcpy2DAsync(out, row, h->k.table_rm, (size_t)h->k.row_bytes, row, (size_t)h->k.height, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_map_shape(f110_sim *h, int32_t *H, int32_t *W)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (H) *H = h->k.height;
    if (W) *W = h->k.width;
    return F110_OK;
}

// ---- static obstacles in a derived map slot (include/f110.h) -------------------------------------------------
static_assert(sizeof(f110_obstacle) == sizeof(Obstacle) && sizeof(Obstacle) == 56, "f110_obstacle and f110::Obstacle are one layout");
static_assert((int)F110_OBST_BOX == (int)OBST_BOX && (int)F110_OBST_DISC == (int)OBST_DISC && (int)F110_MAX_OBSTACLES == kMaxObstacles, "obstacle enums");

static const ScanConst &slot_consts(const f110_sim *h, int slot) { return slot == 0 ? h->k : h->extra_maps[slot - 1].k; }

// the refusals that concern the list alone
static int obstacles_check(f110_sim *h, const char *who, const f110_obstacle *obs, int n)
{
    if (n < 0 || n > F110_MAX_OBSTACLES) return fail(h, F110_ERR_INVALID, "%s: n = %d obstacles, 0..%d are allowed", who, n, (int)F110_MAX_OBSTACLES);
    if (n > 0 && !obs) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    for (int i = 0; i < n; ++i) {
        const f110_obstacle &o = obs[i];
        if (o.shape != F110_OBST_BOX && o.shape != F110_OBST_DISC) return fail(h, F110_ERR_INVALID, "%s: obstacle %d: unknown shape %d", who, i, o.shape);
        const double v[6] = {o.x, o.y, o.c, o.s, o.half_length, o.half_width};
        for (double x : v)
            if (!std::isfinite(x)) return fail(h, F110_ERR_INVALID, "%s: obstacle %d has a non-finite field", who, i);
        if (o.half_length < 0 || o.half_width < 0) return fail(h, F110_ERR_INVALID, "%s: obstacle %d has a negative half extent", who, i);
    }
    return F110_OK;
}

// Stamp `obs` into derived slot m (>= 1) from its base's table: everything on the main stream (the caller went through ENTER, so
// steps in flight on the env blocks come first and the next step's blocks fork from behind this), then one wait for the new
// out-of-bounds value.  The list has been checked.
static int obstacles_stamp(f110_sim *h, const char *who, int m, const f110_obstacle *obs, int n)
{
    f110_sim::MapSlot &ms = h->extra_maps[m - 1];
    const ScanConst &kb = slot_consts(h, ms.base);
    const int H = ms.k.height, W = ms.k.width;
    if (kb.height != H || kb.width != W)
        return fail(h, F110_ERR_STATE, "%s: slot %d was derived from a %d x %d base, slot %d is %d x %d now", who, m, H, W, ms.base, kb.height, kb.width);
    const ObstFrame fr{ms.k.res, ms.k.orig_x, ms.k.orig_y, ms.k.orig_c, ms.k.orig_s};
    // the boxes that reach the table, and the union of their column ranges
    std::vector<ObstBox> boxes;
    std::vector<char> active((size_t)W, 0);
    size_t max_cells = 0;
    for (int i = 0; i < n; ++i) {
        ObstBox b;
        std::memcpy(&b.o, &obs[i], sizeof(Obstacle));
        obstacle_cell_box(b.o, fr, H, W, b.c0, b.c1, b.r0, b.r1);
        if (b.c0 > b.c1 || b.r0 > b.r1) continue;
        for (int c = b.c0; c <= b.c1; ++c) active[c] = 1;
        max_cells = std::max(max_cells, (size_t)(b.c1 - b.c0 + 1) * (size_t)(b.r1 - b.r0 + 1));
        boxes.push_back(b);
    }
    std::vector<int32_t> cols;
    for (int c = 0; c < W; ++c)
        if (active[c]) cols.push_back(c);
    const int Wa = (int)cols.size();
    f110_sim::ObstScratch &sc = h->obst;
    if (!sc.oob) TRY(dmalloc(h, &sc.oob, 1));
    if (!sc.boxes) TRY(dmalloc(h, &sc.boxes, (size_t)F110_MAX_OBSTACLES));
    if (Wa > 0) {
        TRY(dgrow(h, sc.mask, (size_t)H * W));
        TRY(dgrow(h, sc.g, (size_t)H * Wa));
        TRY(dgrow(h, sc.cols, (size_t)W));
        HIPCHK(h, hipMemsetAsync(sc.mask, 0, (size_t)H * W, h->stream));
        HIPCHK(h, hipMemcpyAsync(sc.boxes, boxes.data(), boxes.size() * sizeof(ObstBox), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(sc.cols, cols.data(), (size_t)Wa * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
        hipLaunchKernelGGL(k_obst_stamp, dim3((unsigned)((max_cells + 255) / 256), (unsigned)boxes.size()), dim3(256), 0, h->stream, sc.boxes, fr, W, sc.mask);
        hipLaunchKernelGGL(k_obst_columns, grid1d((size_t)Wa, 64), dim3(64), 0, h->stream, sc.mask, sc.cols, H, W, Wa, sc.g);
    }
    double *oob_dev = (h->d_maps_full && m < h->n_maps_dev) ? &h->d_maps_full[m].oob_value : nullptr;
    hipLaunchKernelGGL(k_obst_corner, dim3(1), dim3(256), 0, h->stream, sc.g, sc.cols, Wa, kb.table_rm, kb.row_bytes, H, W, ms.k.res, sc.oob, oob_dev);
    hipLaunchKernelGGL(k_obst_rows, dim3((unsigned)((ms.k.pad_width + 255) / 256), (unsigned)ms.k.pad_height), dim3(256), 0, h->stream, sc.g, sc.cols, Wa,
                       kb.table_rm, kb.row_bytes, H, W, ms.k.pad_border, ms.k.pad_width, ms.k.res, sc.oob, ms.d_dt_pad);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(&ms.k.oob_value, sc.oob, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ms.occ_stale = true;
    return F110_OK;
}

int f110_add_map_obstacles(f110_sim *h, int32_t base_slot, const f110_obstacle *h_obs, int32_t n, int32_t *slot)
{
    static const char *const who = "f110_add_map_obstacles";
    if (!h || !slot) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    TRY(obstacles_check(h, who, h_obs, n));
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (base_slot < 0 || base_slot > (int)h->extra_maps.size())
        return fail(h, F110_ERR_INVALID, "%s: base slot %d, but %d maps are registered", who, base_slot, 1 + (int)h->extra_maps.size());
    if (base_slot > 0 && h->extra_maps[base_slot - 1].base >= 0) return fail(h, F110_ERR_INVALID, "%s: slot %d is itself derived; derive from its base, slot %d", who, base_slot, h->extra_maps[base_slot - 1].base);
    if (!padded_family(h->cfg.map_layout)) return fail(h, F110_ERR_STATE, "%s needs map_layout = F110_MAP_PADDED_F64", who);
    const ScanConst kb = slot_consts(h, base_slot);
    if (kb.height > 16384 || kb.width > 16384) return fail(h, F110_ERR_INVALID, "%s: the base is %d x %d cells, at most 16384 a side are supported", who, kb.height, kb.width);
    ENTER(h);
    f110_sim::MapSlot ms;
    ms.k = h->k;   // beam / trig / range constants are shared; the map fields are the base's
    fill_map_fields(ms.k, kb.height, kb.width, kb.res, kb.orig_x, kb.orig_y, kb.orig_c, kb.orig_s);
    if (!setup_padded(ms.k)) return fail(h, F110_ERR_INVALID, "f110_add_map: a per-env map must fit the padded layout (16-bit cell coordinates, < 4 GiB)");
    TRY(dmalloc(h, &ms.d_dt_pad, (size_t)ms.k.pad_width * ms.k.pad_height));
    ms.k.pad = ms.d_dt_pad;
    ms.k.table = ms.k.table_rm = ms.d_dt_pad + (size_t)ms.k.pad_border * ms.k.pad_width + ms.k.pad_border;
    ms.k.row_bytes = ms.k.pad_row_bytes;
    ms.base = base_slot;
    h->extra_maps.push_back(std::move(ms));
    const int m = (int)h->extra_maps.size();
    const int rc = obstacles_stamp(h, who, m, h_obs, n);
    if (rc != F110_OK) {
        (void)hipStreamSynchronize(h->stream);
        h->extra_maps.pop_back();   // (and its table with it)
        return rc;
    }
    *slot = m;
    return F110_OK;
}

int f110_set_map_obstacles(f110_sim *h, int32_t slot, const f110_obstacle *h_obs, int32_t n)
{
    static const char *const who = "f110_set_map_obstacles";
    if (!h) return fail(nullptr, F110_ERR_INVALID, "%s: null argument", who);
    TRY(obstacles_check(h, who, h_obs, n));
    if (slot < 0 || slot > (int)h->extra_maps.size())
        return fail(h, F110_ERR_INVALID, "%s: slot %d, but %d maps are registered", who, slot, 1 + (int)h->extra_maps.size());
    if (slot == 0 || h->extra_maps[slot - 1].base < 0) return fail(h, F110_ERR_INVALID, "%s: slot %d is not a derived slot (f110_add_map_obstacles makes one)", who, slot);
    {
        const f110_sim::MapSlot &ms = h->extra_maps[slot - 1];
        const ScanConst &kb = slot_consts(h, ms.base);
        if (!h->has_map || kb.height != ms.k.height || kb.width != ms.k.width)
            return fail(h, F110_ERR_STATE, "%s: slot %d was derived from a %d x %d base, slot %d is %d x %d now", who, slot, ms.k.height, ms.k.width, ms.base,
                        kb.height, kb.width);
    }
    ENTER(h);
    return obstacles_stamp(h, who, slot, h_obs, n);
}

// ---- a corridor carved into a map slot (include/f110.h) -------------------------------------------------------
static_assert((int)F110_MAX_CORRIDOR_POINTS == kMaxCorridorPoints, "corridor limits");

// the refusals that concern the line alone
static int corridor_check(f110_sim *h, const char *who, const double *xy, const double *hw, int M, int closed)
{
    if (!xy || !hw) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    if (M < (closed ? 3 : 2)) return fail(h, F110_ERR_INVALID, "%s: M = %d points, %s corridor needs at least %d", who, M, closed ? "a closed" : "an open", closed ? 3 : 2);
    if (M > F110_MAX_CORRIDOR_POINTS) return fail(h, F110_ERR_INVALID, "%s: M = %d points, at most %d are allowed", who, M, (int)F110_MAX_CORRIDOR_POINTS);
    for (int i = 0; i < 2 * M; ++i)
        if (!std::isfinite(xy[i])) return fail(h, F110_ERR_INVALID, "%s: point %d is not finite", who, i / 2);
    const int S = closed ? M : M - 1;
    for (int i = 0; i < S; ++i) {
        if (!std::isfinite(hw[i])) return fail(h, F110_ERR_INVALID, "%s: the half width of segment %d is not finite", who, i);
        if (hw[i] < 0) return fail(h, F110_ERR_INVALID, "%s: the half width of segment %d is negative", who, i);
    }
    return F110_OK;
}

// ... and the frame
static int corridor_frame_check(f110_sim *h, const char *who, int H, int W, double res, double ox, double oy, double oc, double os)
{
    if (H < 1 || W < 1 || H > 16384 || W > 16384 || !(res > 0) || !std::isfinite(res)) return fail(h, F110_ERR_INVALID, "%s: bad shape %dx%d or resolution", who, H, W);
    if (!std::isfinite(ox) || !std::isfinite(oy) || !std::isfinite(oc) || !std::isfinite(os)) return fail(h, F110_ERR_INVALID, "%s: the origin is not finite", who);
    return F110_OK;
}

static void corridor_mask_launch(f110_sim *h, const double *d_xy, const double *d_hw, int M, int closed, const ObstFrame &fr, int H, int W, uint8_t *d_mask,
                                 unsigned long long *d_carved)
{
    const dim3 grid((unsigned)((W + kCorrTileW - 1) / kCorrTileW), (unsigned)((H + kCorrTileH - 1) / kCorrTileH));   // (H <= 16384: at most 1024 rows of tiles)
    hipLaunchKernelGGL(k_corridor_mask, grid, dim3(kCorrChunk), 0, h->stream, d_xy, d_hw, M, closed ? M : M - 1, fr, H, W, d_mask, d_carved);
}

// The mask of a checked line into the handle's scratch on the main stream (the caller went through ENTER), then the call's one
// wait, for the carved count.  No cell carved: refused there, with the scratch as large as it was; the planes of the distance
// transform have not been asked for yet.  Otherwise the two EDT passes follow on the stream, without a further wait.  Three
// events bracket the mask kernel and the EDT for f110_map_corridor_times.
static int corridor_carve(f110_sim *h, const char *who, const ObstFrame &fr, int H, int W, const double *xy, const double *hw, int M, int closed)
{
    f110_sim::CorridorScratch &sc = h->corr;
    const size_t n = (size_t)H * W, S = (size_t)(closed ? M : M - 1);
    const size_t was[3] = {sc.line.capacity(), sc.mask.capacity(), sc.carved.capacity()};
    for (hipEvent_t &e : sc.ev)
        if (!e) HIPCHK(h, hipEventCreate(&e));
    sc.timed = false;
    TRY(dgrow(h, sc.line, 2 * (size_t)M + S));
    TRY(dgrow(h, sc.mask, n));
    TRY(dgrow(h, sc.carved, 1));
    double *const d_hw = sc.line + 2 * (size_t)M;
    HIPCHK(h, hipMemcpyAsync(sc.line, xy, 2 * (size_t)M * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_hw, hw, S * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(sc.carved, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipEventRecord(sc.ev[0], h->stream));
    corridor_mask_launch(h, sc.line, d_hw, M, closed, fr, H, W, sc.mask, sc.carved);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(sc.ev[1], h->stream));
    unsigned long long carved = 0;
    HIPCHK(h, hipMemcpyAsync(&carved, sc.carved, sizeof carved, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    {
        float ms = 0.f;
        HIPCHK(h, hipEventElapsedTime(&ms, sc.ev[0], sc.ev[1]));
        sc.mask_ms = ms;
    }
    if (carved == 0) {
        TRY(dshrink(h, sc.line, was[0]));
        TRY(dshrink(h, sc.mask, was[1]));
        TRY(dshrink(h, sc.carved, was[2]));
        return fail(h, F110_ERR_INVALID, "%s: no cell carved (every half width 0 between cell centres, or the line misses the table's interior)", who);
    }
    TRY(dgrow(h, sc.g, n));
    TRY(dgrow(h, sc.d2, n));
    HIPCHK(h, hipEventRecord(sc.ev[1], h->stream));   // (again: the EDT's interval begins behind the wait)
    hipLaunchKernelGGL(k_edt_columns, grid1d(W, 64), dim3(64), 0, h->stream, sc.mask, H, W, sc.g);
    hipLaunchKernelGGL(k_edt_rows, dim3(H), dim3(256), (size_t)W * sizeof(uint32_t), h->stream, sc.g, H, W, sc.d2);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(sc.ev[2], h->stream));
    sc.timed = true;
    return F110_OK;
}

// the slot's padded copy from the scratch's squared distances, behind corridor_carve on the main stream (no wait: the out-of-bounds
// value is that of cell [H-1][W-1], a ring cell, so d2 = 0 there and res * sqrt(0) is 0.0 for every finite res > 0)
static int corridor_table(f110_sim *h, f110_sim::MapSlot &ms, double *oob_dev)
{
    const size_t total = (size_t)ms.k.pad_width * ms.k.pad_height;
    hipLaunchKernelGGL(k_corridor_table, grid1d(total, 256), dim3(256), 0, h->stream, h->corr.d2, ms.k.height, ms.k.width, ms.k.pad_border, ms.k.pad_width,
                       ms.k.pad_height, ms.k.res, ms.d_dt_pad, oob_dev);
    HIPCHK(h, hipGetLastError());
    ms.k.oob_value = 0.0;
    return F110_OK;
}

int f110_add_map_corridor(f110_sim *h, const double *h_xy, const double *h_hw, int32_t M, int32_t closed, int32_t H, int32_t W, double res, double ox, double oy,
                          double oyaw, int32_t *slot)
{
    static const char *const who = "f110_add_map_corridor";
    if (!h || !slot) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    TRY(corridor_check(h, who, h_xy, h_hw, M, closed));
    TRY(corridor_frame_check(h, who, H, W, res, ox, oy, std::cos(oyaw), std::sin(oyaw)));
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (!padded_family(h->cfg.map_layout)) return fail(h, F110_ERR_STATE, "%s needs map_layout = F110_MAP_PADDED_F64", who);
    f110_sim::MapSlot ms;
    ms.k = h->k;   // beam / trig / range constants are shared; the map fields follow
    fill_map_fields(ms.k, H, W, res, ox, oy, std::cos(oyaw), std::sin(oyaw));
    if (!setup_padded(ms.k)) return fail(h, F110_ERR_INVALID, "%s: a per-env map must fit the padded layout (16-bit cell coordinates, < 4 GiB)", who);
    ENTER(h);
    TRY(corridor_carve(h, who, ObstFrame{ms.k.res, ms.k.orig_x, ms.k.orig_y, ms.k.orig_c, ms.k.orig_s}, H, W, h_xy, h_hw, M, closed));
    TRY(dmalloc(h, &ms.d_dt_pad, (size_t)ms.k.pad_width * ms.k.pad_height));
    ms.k.pad = ms.d_dt_pad;
    ms.k.table = ms.k.table_rm = ms.d_dt_pad + (size_t)ms.k.pad_border * ms.k.pad_width + ms.k.pad_border;
    ms.k.row_bytes = ms.k.pad_row_bytes;
    ms.carved = true;
    TRY(corridor_table(h, ms, nullptr));
    h->extra_maps.push_back(std::move(ms));
    *slot = (int32_t)h->extra_maps.size();
    return F110_OK;
}

int f110_set_map_corridor(f110_sim *h, int32_t slot, const double *h_xy, const double *h_hw, int32_t M, int32_t closed)
{
    static const char *const who = "f110_set_map_corridor";
    if (!h) return fail(nullptr, F110_ERR_INVALID, "%s: null argument", who);
    TRY(corridor_check(h, who, h_xy, h_hw, M, closed));
    if (slot < 0 || slot > (int)h->extra_maps.size())
        return fail(h, F110_ERR_INVALID, "%s: slot %d, but %d maps are registered", who, slot, 1 + (int)h->extra_maps.size());
    if (slot == 0 || !h->extra_maps[slot - 1].carved) return fail(h, F110_ERR_INVALID, "%s: slot %d was not carved (f110_add_map_corridor makes one)", who, slot);
    ENTER(h);
    f110_sim::MapSlot &ms = h->extra_maps[slot - 1];
    TRY(corridor_carve(h, who, ObstFrame{ms.k.res, ms.k.orig_x, ms.k.orig_y, ms.k.orig_c, ms.k.orig_s}, ms.k.height, ms.k.width, h_xy, h_hw, M, closed));
    TRY(corridor_table(h, ms, (h->d_maps_full && slot < h->n_maps_dev) ? &h->d_maps_full[slot].oob_value : nullptr));
    ms.occ_stale = true;
    return F110_OK;
}

int f110_map_corridor_times(f110_sim *h, double *ms)
{
    if (!h || !ms) return fail(h, F110_ERR_INVALID, "f110_map_corridor_times: null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    f110_sim::CorridorScratch &sc = h->corr;
    ms[0] = sc.mask_ms;
    ms[1] = 0.0;
    if (sc.timed) {
        float edt = 0.f;
        HIPCHK(h, hipEventSynchronize(sc.ev[2]));
        HIPCHK(h, hipEventElapsedTime(&edt, sc.ev[1], sc.ev[2]));
        ms[1] = edt;
    }
    return F110_OK;
}

int f110_corridor_mask_batch(f110_sim *h, const double *h_xy, const double *h_hw, int32_t M, int32_t closed, int32_t H, int32_t W, double res, double ox, double oy,
                             double oc, double os, uint8_t *h_mask, int64_t *h_carved)
{
    static const char *const who = "f110_corridor_mask_batch";
    if (!h || !h_mask || !h_carved) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    TRY(corridor_check(h, who, h_xy, h_hw, M, closed));
    TRY(corridor_frame_check(h, who, H, W, res, ox, oy, oc, os));
    ENTER(h);
    Scratch s(h);
    const double *d_xy = s.in(h_xy, 2 * (size_t)M), *d_hw = s.in(h_hw, (size_t)(closed ? M : M - 1));
    uint8_t *d_mask = s.out(h_mask, (size_t)H * W);
    unsigned long long *d_carved = s.out(reinterpret_cast<unsigned long long *>(h_carved), 1);
    TRY(s.ready());
    HIPCHK(h, hipMemsetAsync(d_carved, 0, sizeof(unsigned long long), h->stream));
    corridor_mask_launch(h, d_xy, d_hw, M, closed, ObstFrame{res, ox, oy, oc, os}, H, W, d_mask, d_carved);
    return s.finish();
}

// ---- raceline and speed profile (include/f110.h) ---------------------------------------------------------------
static_assert((int)F110_RACELINE_MAX_POINTS == kRacelineMaxPoints, "raceline limits");

// the refusals that can be decided before the solve; max_M: the longest line
static int raceline_check(f110_sim *h, const char *who, const double *xy, const double *hw, const int32_t *off, int T, const RacelineSpec &sp, const double *beta,
                          const int32_t *line_iters, int &max_M)
{
    if (T < 1) return fail(h, F110_ERR_INVALID, "%s: T = %d lines", who, T);
    if (sp.levels < 0 || sp.levels > kRacelineMaxLevels) return fail(h, F110_ERR_INVALID, "%s: levels = %d, 0 .. %d are allowed", who, sp.levels, kRacelineMaxLevels);
    if (sp.iters < 0 || sp.iters > kRacelineMaxIters) return fail(h, F110_ERR_INVALID, "%s: iters = %d, 0 .. %d are allowed", who, sp.iters, kRacelineMaxIters);
    const double pos[4] = {sp.v_max, sp.a_lat, sp.a_accel, sp.a_brake};
    for (double v : pos)
        if (!(std::isfinite(v) && v > 0.0)) return fail(h, F110_ERR_INVALID, "%s: v_max, a_lat, a_accel and a_brake must be finite and > 0", who);
    if (!(std::isfinite(sp.margin) && sp.margin >= 0.0)) return fail(h, F110_ERR_INVALID, "%s: margin must be finite and >= 0", who);
    if (sp.iters > 0 && !beta) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    for (int k = 0; k < sp.iters; ++k)
        if (!std::isfinite(beta[k])) return fail(h, F110_ERR_INVALID, "%s: beta[%d] is not finite", who, k);
    if (off[0] != 0) return fail(h, F110_ERR_INVALID, "%s: offsets[0] must be 0", who);
    max_M = 0;
    const int unit = 1 << sp.levels;
    for (int t = 0; t < T; ++t) {
        const long long M = (long long)off[t + 1] - off[t];
        if (M > kRacelineMaxPoints) return fail(h, F110_ERR_INVALID, "%s: line %d has %lld points, at most %d are allowed", who, t, M, kRacelineMaxPoints);
        if (M < 1 || M % unit) return fail(h, F110_ERR_INVALID, "%s: line %d has %lld points, not a multiple of 2^levels = %d", who, t, M, unit);
        if (M / unit < 8) return fail(h, F110_ERR_INVALID, "%s: line %d has %lld points, fewer than 8 on the coarsest level (2^levels = %d)", who, t, M, unit);
        if (line_iters && (line_iters[t] < 0 || line_iters[t] > sp.iters))
            return fail(h, F110_ERR_INVALID, "%s: line %d asks for %d iterations, 0 .. iters = %d are allowed", who, t, line_iters[t], sp.iters);
        const double *q = xy + 2 * (size_t)off[t], *w = hw + off[t];
        for (int i = 0; i < (int)M; ++i)
            if (!std::isfinite(q[2 * i]) || !std::isfinite(q[2 * i + 1]) || !std::isfinite(w[i])) return fail(h, F110_ERR_INVALID, "%s: point %d of line %d is not finite", who, i, t);
        for (int i = 0; i < (int)M; ++i) {
            const int im = i == 0 ? (int)M - 1 : i - 1, ip = i + 1 == (int)M ? 0 : i + 1;
            double nx, ny, b;
            if (!(rl_frame(q[2 * im], q[2 * im + 1], q[2 * ip], q[2 * ip + 1], w[i], sp.margin, nx, ny, b) > 0.0))
                return fail(h, F110_ERR_INVALID, "%s: points %d and %d of line %d coincide: point %d has no normal", who, im, ip, t, i);
        }
        max_M = std::max(max_M, (int)M);
    }
    return F110_OK;
}

// one workgroup per line; the kernel's lanes by the longest line, its beta table by the iteration count
static void raceline_launch(f110_sim *h, const RacelineJob &job, int T, int max_M)
{
    const bool small = max_M <= 256 * kRacelinePerLane, few = job.sp.iters <= 512;
    if (small && few) hipLaunchKernelGGL((k_raceline<256, 512>), dim3(T), dim3(256), 0, h->stream, job);
    else if (small) hipLaunchKernelGGL((k_raceline<256, kRacelineMaxIters>), dim3(T), dim3(256), 0, h->stream, job);
    else if (few) hipLaunchKernelGGL((k_raceline<1024, 512>), dim3(T), dim3(1024), 0, h->stream, job);
    else hipLaunchKernelGGL((k_raceline<1024, kRacelineMaxIters>), dim3(T), dim3(1024), 0, h->stream, job);
}

int f110_raceline_batch(f110_sim *h, const double *h_xy, const double *h_hw, const int32_t *h_off, int32_t T, int32_t levels, int32_t iters, double margin, double v_max,
                        double a_lat, double a_accel, double a_brake, const double *h_beta, const int32_t *h_line_iters, double *h_alpha, double *h_out_xy,
                        double *h_kappa, double *h_vx, double *h_length, double *h_lap_time)
{
    static const char *const who = "f110_raceline_batch";
    if (!h || !h_xy || !h_hw || !h_off || !h_alpha || !h_out_xy || !h_kappa || !h_vx || !h_length || !h_lap_time) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    RacelineJob job{};
    job.sp = RacelineSpec{levels, iters, margin, v_max, a_lat, a_accel, a_brake};
    int max_M = 0;
    TRY(raceline_check(h, who, h_xy, h_hw, h_off, T, job.sp, h_beta, h_line_iters, max_M));
    const size_t n = (size_t)h_off[T];
    // the outputs land in host rows of the call's own first: a line may still be refused once the solve has run
    std::vector<double> rows(5 * n + 2 * (size_t)T);
    std::vector<int32_t> status((size_t)T, 0), ints(h_off, h_off + T + 1);   // offsets [T + 1], then the lines' iteration counts [T]
    if (h_line_iters) ints.insert(ints.end(), h_line_iters, h_line_iters + T);
    else ints.insert(ints.end(), (size_t)T, iters);
    const double no_beta = 0.0;   // iters = 0: the kernel reads no entry, the row exists
    ENTER(h);
    Scratch s(h);   // (few lines: an allocation costs more than these rows' copies)
    job.xy = s.in(h_xy, 2 * n);
    job.hw = s.in(h_hw, n);
    job.off = s.in(ints.data(), ints.size());
    job.beta = s.in(iters > 0 ? h_beta : &no_beta, (size_t)std::max(iters, 1));
    double *const d_rows = s.out(rows.data(), rows.size());
    job.status = s.out(status.data(), (size_t)T);
    TRY(s.ready());
    job.line_iters = job.off + T + 1;
    job.alpha = d_rows;
    job.out_xy = d_rows + n;
    job.kappa = d_rows + 3 * n;
    job.vx = d_rows + 4 * n;
    job.length = d_rows + 5 * n;
    job.lap_time = d_rows + 5 * n + T;
    raceline_launch(h, job, T, max_M);
    TRY(s.finish());
    for (int t = 0; t < T; ++t)
        if (status[(size_t)t]) return fail(h, F110_ERR_INVALID, "%s: the raceline of line %d has a segment of zero length or a curvature that is not finite", who, t);
    std::memcpy(h_alpha, rows.data(), n * sizeof(double));
    std::memcpy(h_out_xy, rows.data() + n, 2 * n * sizeof(double));
    std::memcpy(h_kappa, rows.data() + 3 * n, n * sizeof(double));
    std::memcpy(h_vx, rows.data() + 4 * n, n * sizeof(double));
    std::memcpy(h_length, rows.data() + 5 * n, (size_t)T * sizeof(double));
    std::memcpy(h_lap_time, rows.data() + 5 * n + T, (size_t)T * sizeof(double));
    return F110_OK;
}

int f110_slot_shape(f110_sim *h, int32_t slot, int32_t *H, int32_t *W)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (slot < 0 || slot > (int)h->extra_maps.size()) return fail(h, F110_ERR_INVALID, "f110_slot_shape: slot %d, but %d maps are registered", slot, 1 + (int)h->extra_maps.size());
    const ScanConst &k = slot_consts(h, slot);
    if (H) *H = k.height;
    if (W) *W = k.width;
    return F110_OK;
}

int f110_slot_table(f110_sim *h, int32_t slot, const double **d_table, int32_t *row_bytes)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (slot < 0 || slot > (int)h->extra_maps.size()) return fail(h, F110_ERR_INVALID, "f110_slot_table: slot %d, but %d maps are registered", slot, 1 + (int)h->extra_maps.size());
    const ScanConst &k = slot_consts(h, slot);
    if (d_table) *d_table = k.table_rm;
    if (row_bytes) *row_bytes = k.row_bytes;
    return F110_OK;
}

int f110_get_slot_dt(f110_sim *h, int32_t slot, double *out)
{
    if (!h || !out) return fail(h, F110_ERR_INVALID, "null argument");
    if (slot == 0) return f110_get_map_dt(h, out);
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (slot < 0 || slot > (int)h->extra_maps.size()) return fail(h, F110_ERR_INVALID, "f110_get_slot_dt: slot %d, but %d maps are registered", slot, 1 + (int)h->extra_maps.size());
    ENTER(h);
    const ScanConst &k = h->extra_maps[slot - 1].k;
    const size_t row = (size_t)k.width * sizeof(double);
    HIPCHK(h, hipMemcpy2DAsync(out, row, k.table_rm, (size_t)k.row_bytes, row, (size_t)k.height, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

// ---- centreline extraction (include/f110.h) ----------------------------------------------------------------------
constexpr int kClPoll = 16;   // passes between two looks at the deletion counters (the result does not depend on it)

static int centerline_slot_check(f110_sim *h, const char *who, int slot)
{
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (slot < 0 || slot > (int)h->extra_maps.size()) return fail(h, F110_ERR_INVALID, "%s: slot %d, but %d maps are registered", who, slot, 1 + (int)h->extra_maps.size());
    const ScanConst &k = slot_consts(h, slot);
    if (k.height > 16384 || k.width > 16384) return fail(h, F110_ERR_INVALID, "%s: the map is %d x %d cells, at most 16384 a side are supported", who, k.height, k.width);
    return F110_OK;
}

// Steps 1 - 3 of the rule on the whole free mask of the slot, everything on the main stream (the caller went through ENTER).  On
// success the final mask is h->cl.a or .b (*final_plane), the free mask h->cl.free_plane, and deleted [3] holds the cells each
// stage deleted.  Every pass adds to the counter of its place in the current group of kClPoll passes; the host reads a group's
// counters at once: the first pass that deleted nothing ends the stage, the passes behind it in the group changed nothing.
static int centerline_thin(f110_sim *h, const char *who, int slot, int max_passes, int64_t *deleted, const uint64_t **final_plane)
{
    const ScanConst &k = slot_consts(h, slot);
    const int H = k.height, W = k.width, Ww = (W + 63) / 64;
    const size_t nw = (size_t)H * Ww;
    if (max_passes <= 0) max_passes = 4 * (H + W);
    f110_sim::CenterlineScratch &sc = h->cl;
    TRY(dgrow(h, sc.free_plane, nw));
    TRY(dgrow(h, sc.a, nw));
    TRY(dgrow(h, sc.b, nw));
    TRY(dgrow(h, sc.deleted, (size_t)kClPoll));
    hipLaunchKernelGGL(k_cl_free, dim3((unsigned)((Ww + 3) / 4), (unsigned)H), dim3(256), 0, h->stream, k.table_rm, k.row_bytes, H, W, Ww, sc.free_plane.get());
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(sc.a, sc.free_plane, nw * sizeof(uint64_t), hipMemcpyDeviceToDevice, h->stream));
    uint64_t *cur = sc.a, *oth = sc.b;
    const dim3 grid = grid1d(nw, 256);
    // every stage ends with a wait for its counters: the host's clock between the waits is what the stage cost the caller
    auto t_prev = std::chrono::steady_clock::now();
    auto lap = [&](int i) {
        const auto t = std::chrono::steady_clock::now();
        sc.stage_ms[i] = std::chrono::duration<double, std::milli>(t - t_prev).count();
        t_prev = t;
    };
    for (double &v : sc.stage_ms) v = 0.0;
    unsigned long long cnt[kClPoll];
    int64_t del[3] = {0, 0, 0};
    // stage 0: thinning, a pass = the pair of sub-passes (cur -> oth -> cur); stage 2: pruning, a pass swaps the planes
    for (int stage = 0; stage < 3; ++stage) {
        if (stage == 1) {   // the four staircase passes, once each
            HIPCHK(h, hipMemsetAsync(sc.deleted, 0, sizeof(unsigned long long), h->stream));
            for (int q = 0; q < 4; ++q) {
                hipLaunchKernelGGL(k_cl_stair, grid, dim3(256), 0, h->stream, q, (const uint64_t *)cur, oth, H, Ww, sc.deleted.get());
                std::swap(cur, oth);
            }
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(cnt, sc.deleted, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            del[1] = (int64_t)cnt[0];
            lap(2);
            continue;
        }
        bool done = false;
        for (int used = 0; !done;) {
            if (used == max_passes)
                return fail(h, F110_ERR_STATE, "%s: %s has not converged within max_passes = %d on the %d x %d map of slot %d", who, stage == 0 ? "thinning" : "pruning",
                            max_passes, H, W, slot);
            const int m = std::min(kClPoll, max_passes - used);
            HIPCHK(h, hipMemsetAsync(sc.deleted, 0, (size_t)m * sizeof(unsigned long long), h->stream));
            for (int j = 0; j < m; ++j) {
                if (stage == 0) {
                    hipLaunchKernelGGL(k_cl_thin, grid, dim3(256), 0, h->stream, 0, (const uint64_t *)cur, oth, H, Ww, sc.deleted.get() + j);
                    hipLaunchKernelGGL(k_cl_thin, grid, dim3(256), 0, h->stream, 1, (const uint64_t *)oth, cur, H, Ww, sc.deleted.get() + j);
                } else {
                    hipLaunchKernelGGL(k_cl_prune, grid, dim3(256), 0, h->stream, (const uint64_t *)cur, oth, H, Ww, sc.deleted.get() + j);
                    std::swap(cur, oth);
                }
            }
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, hipMemcpyAsync(cnt, sc.deleted, (size_t)m * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            for (int j = 0; j < m && !done; ++j) {
                del[stage] += (int64_t)cnt[j];
                done = cnt[j] == 0;
            }
            used += m;
        }
        lap(stage == 0 ? 1 : 3);   // (thinning's figure includes the free mask's kernel and copy in front of it)
    }
    for (int i = 0; i < 3; ++i) deleted[i] = del[i];
    *final_plane = cur;
    return F110_OK;
}

// the neighbours P2 .. P9 of the rule as (row, column) offsets
static const int kClDr[8] = {-1, -1, 0, 1, 1, 1, 0, -1}, kClDc[8] = {0, 1, 1, 1, 0, -1, -1, -1};

struct ClPlane {
    std::vector<uint64_t> words;
    int H = 0, W = 0, Ww = 0;
    bool at(int r, int c) const { return r >= 0 && r < H && c >= 0 && c < W && ((words[(size_t)r * Ww + (c >> 6)] >> (c & 63)) & 1u); }
    void set(int r, int c) { words[(size_t)r * Ww + (c >> 6)] |= 1ull << (c & 63); }
};

// Steps 4 and 5 of the rule on the host.  cells: the ordered loop as (r, c) pairs.  0 ok, 1 no loop reachable, 2 not a simple
// loop (`members` cells are connected to the start cell (sr, sc), `branching` of them have more than two neighbours).
static int centerline_trace(const ClPlane &free_mask, const ClPlane &fin, int seed_r, int seed_c, bool has_heading, double hx, double hy, std::vector<int32_t> &cells,
                            int &sr, int &sc, size_t &members, size_t &branching)
{
    const int H = fin.H, W = fin.W;
    ClPlane seen;
    seen.H = H, seen.W = W, seen.Ww = fin.Ww;
    seen.words.assign(fin.words.size(), 0);
    std::vector<int32_t> queue;
    queue.push_back(seed_r * W + seed_c);
    seen.set(seed_r, seed_c);
    sr = sc = -1;
    for (size_t q = 0; q < queue.size(); ++q) {
        const int r = queue[q] / W, c = queue[q] % W;
        if (fin.at(r, c)) {
            sr = r, sc = c;
            break;
        }
        for (int i = 0; i < 8; ++i) {
            const int rr = r + kClDr[i], cc = c + kClDc[i];
            if (free_mask.at(rr, cc) && !seen.at(rr, cc)) {
                seen.set(rr, cc);
                queue.push_back(rr * W + cc);
            }
        }
    }
    if (sr < 0) return 1;
    // the set cells connected to the start, and how many neighbours each has
    seen.words.assign(fin.words.size(), 0);
    queue.clear();
    queue.push_back(sr * W + sc);
    seen.set(sr, sc);
    branching = 0;
    bool simple = true;
    for (size_t q = 0; q < queue.size(); ++q) {
        const int r = queue[q] / W, c = queue[q] % W;
        int deg = 0;
        for (int i = 0; i < 8; ++i) {
            const int rr = r + kClDr[i], cc = c + kClDc[i];
            if (!fin.at(rr, cc)) continue;
            ++deg;
            if (!seen.at(rr, cc)) {
                seen.set(rr, cc);
                queue.push_back(rr * W + cc);
            }
        }
        if (deg > 2) ++branching;
        if (deg != 2) simple = false;
    }
    members = queue.size();
    if (!simple) return 2;
    int first = -1, second = -1;
    for (int i = 0; i < 8; ++i)
        if (fin.at(sr + kClDr[i], sc + kClDc[i])) (first < 0 ? first : second) = i;
    if (has_heading) {
        const double d1 = (double)kClDc[first] * hx + (double)kClDr[first] * hy, d2 = (double)kClDc[second] * hx + (double)kClDr[second] * hy;
        if (d2 > d1) first = second;
    }
    cells.clear();
    cells.push_back(sr);
    cells.push_back(sc);
    int pr = sr, pc = sc, r = sr + kClDr[first], c = sc + kClDc[first];
    while (!(r == sr && c == sc)) {
        if (cells.size() / 2 >= members) return 2;   // (cannot happen on cells of degree two; never walk on)
        cells.push_back(r);
        cells.push_back(c);
        int nr = -1, nc = -1;
        for (int i = 0; i < 8; ++i) {
            const int rr = r + kClDr[i], cc = c + kClDc[i];
            if (fin.at(rr, cc) && !(rr == pr && cc == pc)) {
                nr = rr, nc = cc;
                break;
            }
        }
        pr = r, pc = c, r = nr, c = nc;
    }
    if (cells.size() / 2 != members) return 2;
    if (!has_heading) {   // counter-clockwise: the signed area in (column, row) has the sign of the world's, the frame being a rotation
        const size_t n = members;
        long long area2 = 0;
        for (size_t i = 0; i < n; ++i) {
            const size_t j = i + 1 == n ? 0 : i + 1;
            area2 += (long long)cells[2 * i + 1] * cells[2 * j] - (long long)cells[2 * j + 1] * cells[2 * i];
        }
        if (area2 < 0)
            for (size_t i = 1, j = n - 1; i < j; ++i, --j) {
                std::swap(cells[2 * i], cells[2 * j]);
                std::swap(cells[2 * i + 1], cells[2 * j + 1]);
            }
    }
    return 0;
}

static int centerline_fetch(f110_sim *h, const uint64_t *d_plane, const ScanConst &k, ClPlane &out)
{
    out.H = k.height, out.W = k.width, out.Ww = (k.width + 63) / 64;
    out.words.resize((size_t)out.H * out.Ww);
    HIPCHK(h, hipMemcpyAsync(out.words.data(), d_plane, out.words.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    return F110_OK;
}

int f110_map_centerline(f110_sim *h, int32_t slot, double seed_x, double seed_y, int32_t has_heading, double seed_theta, int32_t max_passes, int32_t *h_cells,
                        double *h_half_width, int32_t cap, int32_t *n, int64_t *h_deleted)
{
    static const char *const who = "f110_map_centerline";
    if (n) *n = 0;
    if (!h || !h_cells || !h_half_width || !n || !h_deleted) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    if (cap < 0) return fail(h, F110_ERR_INVALID, "%s: cap = %d", who, cap);
    TRY(centerline_slot_check(h, who, slot));
    if (!std::isfinite(seed_x) || !std::isfinite(seed_y) || (has_heading && !std::isfinite(seed_theta)))
        return fail(h, F110_ERR_INVALID, "%s: the seed (%g, %g%s) is not finite", who, seed_x, seed_y, has_heading ? ", heading" : "");
    const ScanConst &k = slot_consts(h, slot);
    int seed_r = 0, seed_c = 0;
    if (!cl_seed_cell(seed_x, seed_y, k.res, k.orig_x, k.orig_y, k.orig_c, k.orig_s, k.height, k.width, seed_r, seed_c))
        return fail(h, F110_ERR_INVALID, "%s: the seed (%g, %g) lies outside the %d x %d table of slot %d", who, seed_x, seed_y, k.height, k.width, slot);
    ENTER(h);
    double seed_t = 0.0;   // one table value comes back before anything is launched or allocated
    HIPCHK(h, hipMemcpyAsync(&seed_t, reinterpret_cast<const char *>(k.table_rm) + (size_t)seed_r * (size_t)k.row_bytes + (size_t)seed_c * 8, sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (!(seed_t > 0.0)) return fail(h, F110_ERR_INVALID, "%s: the seed (%g, %g) is cell (%d, %d) of slot %d, which is not free", who, seed_x, seed_y, seed_r, seed_c, slot);
    int64_t deleted[3];
    const uint64_t *d_final = nullptr;
    TRY(centerline_thin(h, who, slot, max_passes, deleted, &d_final));
    const auto t_host = std::chrono::steady_clock::now();
    ClPlane free_mask, fin;
    TRY(centerline_fetch(h, h->cl.free_plane, k, free_mask));
    TRY(centerline_fetch(h, d_final, k, fin));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> cells;
    int sr, sc;
    size_t members = 0, branching = 0;
    double hx = 0.0, hy = 0.0;
    if (has_heading) {   // the heading rotated into the table frame
        const double ct = std::cos(seed_theta), st = std::sin(seed_theta);
        hx = ct * k.orig_c + st * k.orig_s;
        hy = -ct * k.orig_s + st * k.orig_c;
    }
    const int what = centerline_trace(free_mask, fin, seed_r, seed_c, has_heading != 0, hx, hy, cells, sr, sc, members, branching);
    if (what == 1) return fail(h, F110_ERR_STATE, "%s: no loop is reachable from the seed (%g, %g) on slot %d: its free region thins to nothing", who, seed_x, seed_y, slot);
    if (what == 2)
        return fail(h, F110_ERR_STATE, "%s: not a simple loop: %zu of the %zu cells connected to the start cell (%d, %d) have more than two neighbours (islands and "
                    "several loops are not supported)", who, branching, members, sr, sc);
    const int32_t count = (int32_t)(cells.size() / 2);
    *n = count;
    if (count > cap) return fail(h, F110_ERR_INVALID, "%s: the loop has %d cells, cap = %d", who, count, cap);
    TRY(dgrow(h, h->cl.cells, cells.size()));
    TRY(dgrow(h, h->cl.values, (size_t)count));
    HIPCHK(h, hipMemcpyAsync(h->cl.cells, cells.data(), cells.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_cl_gather, grid1d((size_t)count, 256), dim3(256), 0, h->stream, k.table_rm, k.row_bytes, (const int32_t *)h->cl.cells.get(), count, h->cl.values.get());
    HIPCHK(h, hipGetLastError());
    std::vector<double> values((size_t)count);
    HIPCHK(h, hipMemcpyAsync(values.data(), h->cl.values, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::memcpy(h_cells, cells.data(), cells.size() * sizeof(int32_t));
    std::memcpy(h_half_width, values.data(), values.size() * sizeof(double));
    for (int i = 0; i < 3; ++i) h_deleted[i] = deleted[i];
    h->cl.stage_ms[4] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_host).count();
    return F110_OK;
}

int f110_map_centerline_times(f110_sim *h, double *ms)
{
    if (!h || !ms) return fail(h, F110_ERR_INVALID, "f110_map_centerline_times: null argument");
    std::memcpy(ms, h->cl.stage_ms, sizeof h->cl.stage_ms);
    return F110_OK;
}

int f110_slot_frame(f110_sim *h, int32_t slot, double *frame)
{
    if (!h || !frame) return fail(h, F110_ERR_INVALID, "f110_slot_frame: null argument");
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (slot < 0 || slot > (int)h->extra_maps.size()) return fail(h, F110_ERR_INVALID, "f110_slot_frame: slot %d, but %d maps are registered", slot, 1 + (int)h->extra_maps.size());
    const ScanConst &k = slot_consts(h, slot);
    const double v[5] = {k.res, k.orig_x, k.orig_y, k.orig_c, k.orig_s};
    std::memcpy(frame, v, sizeof v);
    return F110_OK;
}

int f110_map_skeleton(f110_sim *h, int32_t slot, int32_t max_passes, uint8_t *h_mask, int64_t *h_deleted)
{
    static const char *const who = "f110_map_skeleton";
    if (!h || !h_mask) return fail(h, F110_ERR_INVALID, "%s: null argument", who);
    TRY(centerline_slot_check(h, who, slot));
    ENTER(h);
    const ScanConst &k = slot_consts(h, slot);
    int64_t deleted[3];
    const uint64_t *d_final = nullptr;
    TRY(centerline_thin(h, who, slot, max_passes, deleted, &d_final));
    ClPlane fin;
    TRY(centerline_fetch(h, d_final, k, fin));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (int r = 0; r < fin.H; ++r)
        for (int c = 0; c < fin.W; ++c) h_mask[(size_t)r * fin.W + c] = fin.at(r, c) ? 1 : 0;
    if (h_deleted)
        for (int i = 0; i < 3; ++i) h_deleted[i] = deleted[i];
    return F110_OK;
}

int f110_set_trig_tables(f110_sim *h, const double *s, const double *c, int32_t n)
{
    if (!h || !s || !c) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (n != h->cfg.theta_dis) return fail(h, F110_ERR_INVALID, "trig tables must have theta_dis=%d entries (got %d)", h->cfg.theta_dis, n);
    Scratch sc(h);
    const double *ds = sc.in(s, (size_t)n), *dc = sc.in(c, (size_t)n);
    TRY(sc.ready());
    hipLaunchKernelGGL(k_interleave_cs, grid1d(n, 256), dim3(256), 0, h->stream, ds, dc, n, h->d_cs);
    return sc.finish();
}

static const char *const kBeamsMsg = "the beam tables (f110_set_beam_tables) are not the uniform ramp scan_angles[i] = scan_angles[0] + i*inc of base_classes.py:133-134: "
                                     "the step's opponent ray-cast assumes it; such tables are served by f110_raycast_batch / f110_ttc_batch only";

// what every stepping entry point asks before it enqueues anything (args: its pointer arguments are all there)
static int check_step(f110_sim *h, bool args)
{
    if (!h || !args) return fail(h, F110_ERR_INVALID, "null argument");
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (!h->beams_uniform) return fail(h, F110_ERR_STATE, kBeamsMsg);
    return F110_OK;
}

int f110_set_beam_tables(f110_sim *h, const double *sa, const double *co, const double *sd, int32_t B)
{
    if (!h || !sa || !co || !sd) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (B != h->cfg.num_beams) return fail(h, F110_ERR_INVALID, "beam tables must have num_beams=%d entries (got %d)", h->cfg.num_beams, B);
    HIPCHK(h, hipMemcpyAsync(h->d_scan_angles, sa, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_beam_cos, co, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_side, sd, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // beam spacing of THIS table (seed of the nearest-beam search in the opponent ray-cast)
    h->dev.angle_inc = (sa[B - 1] - sa[0]) / (B - 1);
    // The step's opponent ray-cast finds a vertex's beam next to a closed-form estimate (nearest_beam: +-3 entries) and culls by a
    // disc — both assume the table is the increasing ramp sa[0] + i*inc that RaceCar builds (base_classes.py:133-134).  A table
    // within a quarter of a beam spacing of that ramp keeps the true argmin inside the searched neighbourhood; anything else
    // (the free functions ray_cast / check_ttc_jit accept ANY array) is served by the unit entry points only, with the
    // reference's full argmin (k_raycast_unit), and refused by the step (beams_must_be_uniform).
    {
        const double inc = h->dev.angle_inc;
        bool uni = B >= 2 && inc > 0.0 && inc == inc;
        for (int i = 0; uni && i < B; ++i) uni = std::fabs(sa[i] - (sa[0] + (double)i * inc)) <= 0.25 * inc;
        h->beams_uniform = uni;
    }
    // iTTC early-out of k_scan_rays: with s = max|side|, c = max|cos|, a beam with
    // r > s + thresh*(1+1e-9)*c*|v| has (r - side_b) > thresh*(1+1e-12)*|v*cos_b| and cannot hit.
    {
        double smax = 0.0, cmax = 0.0;
        bool finite = true;
        for (int i = 0; i < B; ++i) {
            if (!(sd[i] == sd[i]) || !(co[i] == co[i])) finite = false;
            smax = std::max(smax, std::fabs(sd[i]));
            cmax = std::max(cmax, std::fabs(co[i]));
        }
        h->ttc_side_max = finite ? smax : INFINITY;
        h->ttc_cos_max = finite ? cmax : INFINITY;
    }
    return F110_OK;
}

int f110_set_params_batch(f110_sim *h, const double *h_params)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (h->ps.on) return fail(h, F110_ERR_STATE, "a parameter sampler is armed (f110_param_sampler_set) and owns the per-agent rows; disarm it first");
    if (!h_params) {   // back to one parameter set per agent slot
        h->dev.params = h->d_params;
        h->dev.params_per_agent = 0;
        return F110_OK;
    }
    const size_t n = (size_t)h->N * NPARAMS;
    if (!h->d_params_all) TRY(dmalloc(h, &h->d_params_all, n));
    HIPCHK(h, hipMemcpyAsync(h->d_params_all, h_params, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->dev.params = h->d_params_all;
    h->dev.params_per_agent = 1;
    return F110_OK;
}

int f110_set_params(f110_sim *h, int32_t agent_idx, const double *p)
{
    if (!h || !p) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (h->ps.on) return fail(h, F110_ERR_STATE, "a parameter sampler is armed (f110_param_sampler_set) and owns the per-agent rows; disarm it first");
    if (h->dev.params_per_agent) return fail(h, F110_ERR_STATE, "per-agent parameters are active (f110_set_params_batch); clear them first");
    const int A = h->cfg.num_agents;
    if (agent_idx >= A) return fail(h, F110_ERR_INVALID, "Index given is out of bounds for list of agents.");
    for (int a = 0; a < A; ++a)
        if (agent_idx < 0 || agent_idx == a)
            HIPCHK(h, hipMemcpyAsync(h->d_params + (size_t)a * NPARAMS, p, sizeof(double) * NPARAMS, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

static int noise_cache_extend(f110_sim *h, int upto);
static int noise_adopt(f110_sim *h);

static void noise_release(f110_sim *h)
{
    if (h->noise_stream) (void)hipStreamSynchronize(h->noise_stream);
    h->noise_ahead = false;
    h->noise_ahead_block.reset();
    h->noise_retired.clear();
    h->d_noise.reset();
    h->d_rng_state.reset();
    h->d_rng_seed.reset();
    h->d_rng_rowstate.reset();
    h->dev.noise = nullptr;
    h->dev.noise_rows = 0;
    h->dev.noise_rng = 0;
    h->dev.rng_state = nullptr;
    h->dev.rng_seed = nullptr;
    h->dev.rng_rowstate = nullptr;
    h->noise_rows_ready = 0;
    h->noise_rows_alloc = 0;
    h->noise_src = 0;
    for (uint64_t &w : h->noise_src_id) w = 0;
}

int f110_set_noise_table(f110_sim *h, const double *noise, int32_t rows, int32_t B)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    noise_release(h);
    if (!noise || rows <= 0) return F110_OK;
    if (B != h->cfg.num_beams) return fail(h, F110_ERR_INVALID, "noise table must have num_beams=%d columns (got %d)", h->cfg.num_beams, B);
    TRY(dmalloc(h, &h->d_noise, (size_t)rows * B));
    HIPCHK(h, hipMemcpyAsync(h->d_noise, noise, sizeof(double) * (size_t)rows * B, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->dev.noise = h->d_noise;
    h->dev.noise_rows = rows;
    uint64_t fnv = 0xcbf29ce484222325ull;   // FNV-1a 64 of the table's bytes
    const unsigned char *bytes = reinterpret_cast<const unsigned char *>(noise);
    for (size_t i = 0, n = sizeof(double) * (size_t)rows * B; i < n; ++i) fnv = (fnv ^ bytes[i]) * 0x100000001b3ull;
    h->noise_src = 1;
    h->noise_src_id[0] = fnv;
    h->noise_src_id[1] = (uint64_t)rows;
    h->noise_src_id[2] = (uint64_t)B;
    return F110_OK;
}

int f110_pcg64_seed(uint64_t seed, uint64_t *out_state_inc)
{
    if (!out_state_inc) return fail(nullptr, F110_ERR_INVALID, "null argument");
    pcg64_seed_from_u64(seed, out_state_inc);
    return F110_OK;
}

int f110_set_noise_rng(f110_sim *h, const uint64_t *state_inc, int32_t per_agent, double std_dev, int32_t cache_rows)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    noise_release(h);
    if (!state_inc) return F110_OK;
    if (!(std_dev >= 0.0)) return fail(h, F110_ERR_INVALID, "noise std_dev must be >= 0");
    const int B = h->cfg.num_beams;
    const size_t N = (size_t)h->N;
    h->noise_gen.scale = std_dev;
    TRY(dmalloc(h, &h->d_rng_state, N));
    HIPCHK(h, hipMemsetAsync(h->d_rng_state, 0, sizeof(U128) * N, h->stream));
    h->dev.rng_state = h->d_rng_state;
    if (per_agent) {
        // h_state_inc [N][4]: two U128 {hi, lo} per agent — the layout of rng_seed
        TRY(dmalloc(h, &h->d_rng_seed, 2 * N));
        HIPCHK(h, hipMemcpy(h->d_rng_seed, state_inc, sizeof(U128) * 2 * N, hipMemcpyHostToDevice));
        h->dev.rng_seed = h->d_rng_seed;
        h->dev.noise_rng = 2;
        h->noise_src = 3;
        return F110_OK;
    }
    // capacity: 164 s of simulated time by default.  Rows are generated on demand, and the memory behind
    // them grows on demand too (noise_cache_extend): a short-lived Simulator pays for the rows it uses
    // (8.6 KB each at 1080 beams), not for the capacity (141 MB)
    int rows = cache_rows > 0 ? cache_rows : 16384;
    if ((size_t)rows * B * sizeof(double) > (size_t)1 << 31) rows = (int)(((size_t)1 << 31) / ((size_t)B * sizeof(double)));
    h->noise_rows_alloc = std::min(rows, 512);
    TRY(dmalloc(h, &h->d_noise, (size_t)h->noise_rows_alloc * B));
    TRY(dmalloc(h, &h->d_rng_rowstate, (size_t)rows + 1));
    const U128 st0 = {state_inc[0], state_inc[1]};
    HIPCHK(h, hipMemcpy(h->d_rng_rowstate, &st0, sizeof st0, hipMemcpyHostToDevice));
    h->dev.rng_inc = U128{state_inc[2], state_inc[3]};
    h->dev.rng_rowstate = h->d_rng_rowstate;
    h->dev.noise = h->d_noise;
    h->dev.noise_rows = rows;
    h->dev.noise_rng = 1;
    h->noise_rows_ready = 0;
    h->noise_src = 2;
    for (int w = 0; w < 4; ++w) h->noise_src_id[w] = state_inc[w];
    return noise_cache_extend(h, std::min(rows, 256));
}

int f110_noise_prepare(f110_sim *h, int32_t rows)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (h->dev.noise_rng != 1) return F110_OK;
    TRY(noise_adopt(h));
    return noise_cache_extend(h, rows);
}

int f110_noise_rows_batch(f110_sim *h, const uint64_t *state_inc, double std_dev, int32_t rows, int32_t num_beams, double *h_out,
                          uint64_t *h_state_out)
{
    if (!h || !state_inc || !h_out || rows < 1 || num_beams < 1) return fail(h, F110_ERR_INVALID, "f110_noise_rows_batch: bad argument");
    ENTER(h);
    Scratch s(h);
    U128 last{};
    U128 *d_rs = s.tmp<U128>((size_t)rows + 1);
    double *d_out = s.out(h_out, (size_t)rows * num_beams);
    TRY(s.ready());
    s.later(&last, d_rs + rows, 1);   // the state behind the last row
    const U128 st0 = {state_inc[0], state_inc[1]}, inc = {state_inc[2], state_inc[3]};
    HIPCHK(h, hipMemcpyAsync(d_rs, &st0, sizeof st0, hipMemcpyHostToDevice, h->stream));
    NoiseGen g = h->noise_gen;
    g.scale = std_dev;
    hipLaunchKernelGGL(k_noise_cache, dim3(1), dim3(64), 0, h->stream, g, inc, d_rs, d_out, 0, rows, num_beams);
    TRY(s.finish());
    if (h_state_out) {
        h_state_out[0] = last.hi;
        h_state_out[1] = last.lo;
    }
    return F110_OK;
}

int f110_scan_lookup_count(f110_sim *h, int32_t enable, int64_t *out_total)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (out_total) {
        unsigned long long v[2] = {0, 0};
        HIPCHK(h, hipMemcpyAsync(v, h->d_lookups, sizeof v, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_lookups, 0, sizeof v, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        out_total[0] = (int64_t)v[0];
        out_total[1] = (int64_t)v[1];
    }
    if (enable >= 0) h->lookups_on = enable != 0;
    return F110_OK;
}

// ---- reset / step ------------------------------------------------------------------------
int f110_reset_device(f110_sim *h, const double *d_poses, const uint8_t *d_env_mask)
{
    if (!h || !d_poses) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!d_env_mask) h->noise_ub = 0;   // every agent's step_count is 0 again
    hipLaunchKernelGGL(k_reset, grid1d(h->N, 256), dim3(256), 0, h->stream, h->dev, d_poses, d_env_mask);
    if (h->rs.on)
        hipLaunchKernelGGL(k_sampler_keep, grid1d(h->N, 256), dim3(256), 0, h->stream, h->rs.job.last, d_poses, d_env_mask, h->N, h->cfg.num_agents);
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

int f110_set_auto_reseat(f110_sim *h, const double *d_start_poses, int32_t ego_idx, int32_t *d_count)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (d_start_poses && (ego_idx < 0 || ego_idx >= h->cfg.num_agents))
        return fail(h, F110_ERR_INVALID, "Index given is out of bounds for list of agents.");
    h->dev.reseat_poses = d_start_poses;
    h->dev.reseat_ego = d_start_poses ? ego_idx : 0;
    h->dev.reseat_count = d_start_poses ? d_count : nullptr;
    return F110_OK;
}

int f110_reset_collided_device(f110_sim *h, const double *d_start_poses, int32_t ego_idx, int32_t *d_count)
{
    if (!h || !d_start_poses) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (ego_idx < 0 || ego_idx >= h->cfg.num_agents) return fail(h, F110_ERR_INVALID, "Index given is out of bounds for list of agents.");
    if (h->rs.on) TRY(track_prepare(h));
    hipLaunchKernelGGL(k_reset_collided, grid1d(h->N, 256), dim3(256), 0, h->stream, h->dev, d_start_poses, ego_idx, d_count);
    HIPCHK(h, hipGetLastError());
    if (reseat_draws(h)) TRY(reseat_launch(h, h->stream, kSampleCollided, 0, h->cfg.num_envs, ego_idx));
    return F110_OK;
}

// ---- randomised start poses (f110_reset_sampler_*) ------------------------------------------------------------
static void sampler_release(f110_sim *h)
{
    h->rs.mem.clear();
    h->rs.job = SamplerJob{};
    h->rs.on = false;
}

// one k_reset_sample over envs [e0, e0 + count) on stream st (track_prepare has run)
static int sampler_launch(f110_sim *h, hipStream_t st, int mode, int e0, int count, const uint8_t *d_mask, int ego)
{
    if (count <= 0) return F110_OK;
    SamplerJob j = h->rs.job;
    j.tracks = h->d_tracks;
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.maps = h->multi_map ? h->d_maps_full : cold_consts(h);
    if (!j.maps) return fail(h, F110_ERR_HIP, "f110_reset_sample: constant upload failed");
    j.mode = mode;
    j.mask = d_mask;
    j.ego = ego;
    hipLaunchKernelGGL(k_reset_sample, grid1d(count, 256), dim3(256), 0, st, j, h->dev, h->ep, h->has_episode ? 1 : 0, e0, count);
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

// the draw behind a call that may have re-seated envs in-step, where that call's last kernel ran (the main stream, or per env block)
static int sampler_after_step(f110_sim *h, const EnvBlocks &where)
{
    for (const EnvBlock &b : where) TRY(reseat_launch(h, b.stream, kSampleMarker, b.e0, b.count, 0));
    if (h->last_launches > 0) h->last_launches += (h->rs.on ? 1 : 0) + (h->ps.on ? 1 : 0);   // (the one-launch step is two launches with a draw behind it)
    return F110_OK;
}

int f110_pcg64_seed_spawn(const uint32_t *h_entropy, int32_t n_words, uint64_t e0, int32_t n, uint64_t *h_out)
{
    if (!h_entropy || !h_out || n_words < 1 || n_words > 1 << 20 || n < 0) return fail(nullptr, F110_ERR_INVALID, "f110_pcg64_seed_spawn: bad argument");
    for (int32_t q = 0; q < n; ++q) pcg64_seed_spawn(h_entropy, n_words, e0 + (uint64_t)q, h_out + 4 * (size_t)q);
    return F110_OK;
}

int f110_reset_sampler_set(f110_sim *h, const f110_reset_sampler *spec, const uint64_t *h_streams)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!spec) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        sampler_release(h);
        return F110_OK;
    }
    if (!h_streams) return fail(h, F110_ERR_INVALID, "f110_reset_sampler_set: null stream words");
    const f110_reset_sampler &c = *spec;
    if (!(c.s_lo >= 0.0 && c.s_lo < c.s_hi && c.s_hi <= 1.0)) return fail(h, F110_ERR_INVALID, "reset sampler: need 0 <= s_lo < s_hi <= 1, got %g, %g", c.s_lo, c.s_hi);
    if (!(c.gap > 0.0 && std::isfinite(c.gap))) return fail(h, F110_ERR_INVALID, "reset sampler: gap must be finite and > 0, got %g", c.gap);
    if (!(c.lateral >= 0.0 && std::isfinite(c.lateral))) return fail(h, F110_ERR_INVALID, "reset sampler: lateral must be finite and >= 0, got %g", c.lateral);
    if (!(c.heading >= 0.0 && std::isfinite(c.heading))) return fail(h, F110_ERR_INVALID, "reset sampler: heading must be finite and >= 0, got %g", c.heading);
    if (!(c.clearance >= 0.0 && std::isfinite(c.clearance))) return fail(h, F110_ERR_INVALID, "reset sampler: clearance must be finite and >= 0, got %g", c.clearance);
    if (c.attempts < 1 || c.attempts > 1024) return fail(h, F110_ERR_INVALID, "reset sampler: attempts must be in 1 .. 1024, got %d", c.attempts);
    TRY(track_prepare(h));   // every env's slot has a track (F110_ERR_STATE otherwise)
    HIPCHK(h, hipStreamSynchronize(h->stream));
    sampler_release(h);
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs;
    SamplerJob &j = h->rs.job;
    TRY(dmalloc(h, h->rs.mem, &j.stream, 2 * E));
    TRY(dmalloc(h, h->rs.mem, &j.last, 3 * N));
    TRY(dmalloc(h, h->rs.mem, &j.cand, 3 * N));
    TRY(dmalloc(h, h->rs.mem, &j.out_poses, 3 * N));
    TRY(dmalloc(h, h->rs.mem, &j.out_rot, 4 * E));
    TRY(dmalloc(h, h->rs.mem, &j.attempt, E));
    TRY(dmalloc(h, h->rs.mem, &j.counters, 2));
    // {state.hi, state.lo, inc.hi, inc.lo} per env is the layout of two U128 {hi, lo}
    HIPCHK(h, hipMemcpy(j.stream, h_streams, sizeof(U128) * 2 * E, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(j.last, 0, sizeof(double) * 3 * N));
    HIPCHK(h, hipMemset(j.attempt, 0xff, sizeof(int32_t) * E));
    HIPCHK(h, hipMemset(j.counters, 0, 2 * sizeof(unsigned long long)));
    j.s_lo = c.s_lo;
    j.s_hi = c.s_hi;
    j.gap = c.gap;
    j.lateral = c.lateral;
    j.heading = c.heading;
    j.clearance = c.clearance;
    j.attempts = c.attempts;
    j.A = h->cfg.num_agents;
    h->rs.on = true;
    return F110_OK;
}

int f110_reset_sample_device(f110_sim *h, const uint8_t *d_env_mask)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->rs.on) return fail(h, F110_ERR_STATE, "f110_reset_sample: no reset sampler is armed (f110_reset_sampler_set)");
    TRY(track_prepare(h));
    const SamplerJob &j = h->rs.job;
    TRY(sampler_launch(h, h->stream, kSampleExplicit, 0, h->cfg.num_envs, d_env_mask, 0));
    if (!d_env_mask) h->noise_ub = 0;
    if (h->has_episode)
        hipLaunchKernelGGL(k_episode_reset, grid1d(h->N, 256), dim3(256), 0, h->stream, h->dev, h->ep, j.out_poses, j.out_rot, d_env_mask);
    hipLaunchKernelGGL(k_reset, grid1d(h->N, 256), dim3(256), 0, h->stream, h->dev, j.out_poses, d_env_mask);
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

int f110_reset_sample(f110_sim *h, const uint8_t *h_env_mask)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (h_env_mask) HIPCHK(h, hipMemcpyAsync(h->d_mask, h_env_mask, (size_t)h->cfg.num_envs, hipMemcpyHostToDevice, h->stream));
    TRY(f110_reset_sample_device(h, h_env_mask ? h->d_mask : nullptr));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the host mask is consumed on return
    return F110_OK;
}

int f110_reset_sampler_stats(f110_sim *h, uint64_t *out2, int32_t *h_attempt, int32_t clear)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->rs.on) return fail(h, F110_ERR_STATE, "no reset sampler is armed (f110_reset_sampler_set)");
    const SamplerJob &j = h->rs.job;
    unsigned long long v[2] = {0, 0};
    HIPCHK(h, hipMemcpyAsync(v, j.counters, sizeof v, hipMemcpyDeviceToHost, h->stream));
    if (h_attempt) HIPCHK(h, hipMemcpyAsync(h_attempt, j.attempt, sizeof(int32_t) * h->cfg.num_envs, hipMemcpyDeviceToHost, h->stream));
    if (clear) HIPCHK(h, hipMemsetAsync(j.counters, 0, sizeof v, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (out2) {
        out2[0] = v[0];
        out2[1] = v[1];
    }
    return F110_OK;
}

int f110_reset_sampler_poses(f110_sim *h, double *h_poses)
{
    if (!h || !h_poses) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!h->rs.on) return fail(h, F110_ERR_STATE, "no reset sampler is armed (f110_reset_sampler_set)");
    HIPCHK(h, hipMemcpyAsync(h_poses, h->rs.job.last, sizeof(double) * 3 * h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

// ---- randomised vehicle parameters (f110_param_sampler_*) ------------------------------------------------------
static_assert(sizeof(ParamDist) == sizeof(f110_param_dist) && offsetof(ParamDist, relative) == offsetof(f110_param_dist, relative),
              "ParamDist restates f110_param_dist");

static void param_release(f110_sim *h)
{
    if (h->ps.on) {   // back to the per-slot sets
        h->dev.params = h->d_params;
        h->dev.params_per_agent = 0;
    }
    if (h->ps.owns_rows) h->d_params_all.reset();
    h->ps.mem.clear();
    h->ps.job = ParamJob{};
    h->ps.owns_rows = false;
    h->ps.on = false;
}

// the entries as the kernel takes them; `relative`: some drawn slot multiplies the nominal
static void param_entries(const f110_param_dist *entries, ParamJob &j)
{
    j.relative = 0;
    for (int p = 0; p < NPARAMS; ++p) {
        const f110_param_dist &e = entries[p];
        j.d[p] = ParamDist{e.kind, e.scope, e.a, e.b, e.lo, e.hi, e.relative ? 1 : 0, 0};
        if (e.kind != F110_PARAM_FIXED && e.relative) j.relative = 1;
    }
}

// one k_param_sample over envs [e0, e0 + count) on stream st
static int param_launch(f110_sim *h, hipStream_t st, ParamJob j, int mode, int e0, int count, const uint8_t *d_mask, int ego)
{
    if (count <= 0) return F110_OK;
    j.mode = mode;
    j.mask = d_mask;
    j.ego = ego;
    j.zk = h->d_zig_k, j.zw = h->d_zig_w, j.zf = h->d_zig_f;
    const size_t lds = j.relative ? sizeof(double) * NPARAMS * (size_t)j.A : 0;
    hipLaunchKernelGGL(k_param_sample, grid1d(count, 256), dim3(256), lds, st, j, e0, count);
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

// what runs behind a re-seat of envs [e0, e0 + count) on stream st: the draw of every armed sampler (their streams and their
// outputs are disjoint, so the order does not matter); the reset sampler needs track_prepare to have run
static int reseat_launch(f110_sim *h, hipStream_t st, int mode, int e0, int count, int ego)
{
    if (h->rs.on) TRY(sampler_launch(h, st, mode, e0, count, nullptr, ego));
    if (h->ps.on) {
        ParamJob j = h->ps.job;
        j.step_count = h->dev.step_count;
        j.collisions = h->dev.collisions;
        j.done = h->ep.done;
        TRY(param_launch(h, st, j, mode, e0, count, nullptr, ego));
    }
    return F110_OK;
}

int f110_param_sampler_set(f110_sim *h, const f110_param_dist *entries18, const uint64_t *h_streams)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!entries18) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        param_release(h);
        return F110_OK;
    }
    if (!h_streams) return fail(h, F110_ERR_INVALID, "f110_param_sampler_set: null stream words");
    if (!h->ps.on && h->dev.params_per_agent)
        return fail(h, F110_ERR_STATE, "per-agent parameters are active (f110_set_params_batch) and own the rows; clear them first");
    const int A = h->cfg.num_agents;
    if (A > kParamMaxAgents) return fail(h, F110_ERR_INVALID, "f110_param_sampler_set: at most %d agents per env, this handle has %d", kParamMaxAgents, A);
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs;
    std::vector<double> nominal((size_t)A * NPARAMS);
    HIPCHK(h, hipMemcpyAsync(nominal.data(), h->d_params, sizeof(double) * nominal.size(), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ParamJob fresh{};
    param_entries(entries18, fresh);
    char why[256];
    if (param_dists_check(fresh.d, nominal.data(), A, why, sizeof why)) return fail(h, F110_ERR_INVALID, "f110_param_sampler_set: %s", why);
    param_release(h);
    ParamJob &j = h->ps.job;
    j = fresh;
    if (!h->d_params_all) {
        TRY(dmalloc(h, &h->d_params_all, N * NPARAMS));
        h->ps.owns_rows = true;
    }
    TRY(dmalloc(h, h->ps.mem, &j.stream, 2 * E));
    TRY(dmalloc(h, h->ps.mem, &j.counter, 1));
    double *d_nominal = nullptr;
    TRY(dmalloc(h, h->ps.mem, &d_nominal, nominal.size()));
    std::vector<double> rows(N * NPARAMS);
    for (size_t i = 0; i < N; ++i) std::memcpy(&rows[i * NPARAMS], &nominal[(i % A) * NPARAMS], sizeof(double) * NPARAMS);
    HIPCHK(h, hipMemcpy(h->d_params_all, rows.data(), sizeof(double) * rows.size(), hipMemcpyHostToDevice));
    HIPCHK(h, hipMemcpy(d_nominal, nominal.data(), sizeof(double) * nominal.size(), hipMemcpyHostToDevice));
    // {state.hi, state.lo, inc.hi, inc.lo} per env is the layout of two U128 {hi, lo}
    HIPCHK(h, hipMemcpy(j.stream, h_streams, sizeof(U128) * 2 * E, hipMemcpyHostToDevice));
    HIPCHK(h, hipMemset(j.counter, 0, sizeof(unsigned long long)));
    j.nominal = d_nominal;
    j.rows = h->d_params_all;
    j.A = A;
    h->dev.params = h->d_params_all;
    h->dev.params_per_agent = 1;
    h->ps.on = true;
    return F110_OK;
}

int f110_param_sample_device(f110_sim *h, const uint8_t *d_env_mask)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->ps.on) return fail(h, F110_ERR_STATE, "f110_param_sample: no parameter sampler is armed (f110_param_sampler_set)");
    return param_launch(h, h->stream, h->ps.job, kSampleExplicit, 0, h->cfg.num_envs, d_env_mask, 0);
}

int f110_param_sample(f110_sim *h, const uint8_t *h_env_mask)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->ps.on) return fail(h, F110_ERR_STATE, "f110_param_sample: no parameter sampler is armed (f110_param_sampler_set)");
    if (h_env_mask) HIPCHK(h, hipMemcpyAsync(h->d_mask, h_env_mask, (size_t)h->cfg.num_envs, hipMemcpyHostToDevice, h->stream));
    TRY(f110_param_sample_device(h, h_env_mask ? h->d_mask : nullptr));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the host mask is consumed on return
    return F110_OK;
}

int f110_param_sampler_stats(f110_sim *h, uint64_t *draws, int32_t clear)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->ps.on) return fail(h, F110_ERR_STATE, "no parameter sampler is armed (f110_param_sampler_set)");
    unsigned long long v = 0;
    HIPCHK(h, hipMemcpyAsync(&v, h->ps.job.counter, sizeof v, hipMemcpyDeviceToHost, h->stream));
    if (clear) HIPCHK(h, hipMemsetAsync(h->ps.job.counter, 0, sizeof v, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (draws) *draws = v;
    return F110_OK;
}

int f110_params_get(f110_sim *h, double *h_out)
{
    if (!h || !h_out) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!h->dev.params_per_agent) return fail(h, F110_ERR_STATE, "no per-agent parameter rows are active (f110_param_sampler_set, f110_set_params_batch)");
    HIPCHK(h, hipMemcpyAsync(h_out, h->d_params_all, sizeof(double) * NPARAMS * (size_t)h->N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_params_view(f110_sim *h, const double **d_rows)
{
    if (!h || !d_rows) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    *d_rows = nullptr;
    if (!h->dev.params_per_agent) return fail(h, F110_ERR_STATE, "no per-agent parameter rows are active (f110_param_sampler_set, f110_set_params_batch)");
    *d_rows = h->d_params_all;
    return F110_OK;
}

int f110_param_sample_batch(f110_sim *h, const f110_param_dist *entries18, const double *h_nominal, int32_t A, const uint64_t *h_streams,
                            int32_t m, int32_t rounds, double *h_out, uint64_t *h_streams_out)
{
    if (!h || !entries18 || !h_nominal || !h_streams || !h_out) return fail(h, F110_ERR_INVALID, "f110_param_sample_batch: null argument");
    ENTER(h);
    if (A < 1 || A > kParamMaxAgents || m < 1 || rounds < 1 || (size_t)m * A * rounds > ((size_t)1 << 28))
        return fail(h, F110_ERR_INVALID, "f110_param_sample_batch: A = %d (1 .. %d), m = %d, rounds = %d", A, kParamMaxAgents, m, rounds);
    ParamJob j{};
    param_entries(entries18, j);
    char why[256];
    if (param_dists_check(j.d, h_nominal, A, why, sizeof why)) return fail(h, F110_ERR_INVALID, "f110_param_sample_batch: %s", why);
    const size_t per_round = (size_t)m * A * NPARAMS;
    std::vector<double> rows0(per_round);   // every round starts from the rows before it: round 0 from the nominal ones
    for (size_t i = 0; i < (size_t)m * A; ++i) std::memcpy(&rows0[i * NPARAMS], h_nominal + (i % A) * NPARAMS, sizeof(double) * NPARAMS);
    Scratch s(h);
    j.nominal = s.in(h_nominal, (size_t)A * NPARAMS);
    uint64_t *d_streams = s.in(h_streams, 4 * (size_t)m);   // {state.hi, state.lo, inc.hi, inc.lo} per env: two U128 {hi, lo}
    s.later(h_streams_out, static_cast<const uint64_t *>(d_streams), 4 * (size_t)m);
    j.stream = reinterpret_cast<U128 *>(d_streams);
    double *d_out = s.out(h_out, per_round * rounds);
    j.counter = s.tmp<unsigned long long>(1);
    TRY(s.ready());
    HIPCHK(h, hipMemsetAsync(j.counter, 0, sizeof(unsigned long long), h->stream));
    HIPCHK(h, hipMemcpyAsync(d_out, rows0.data(), sizeof(double) * per_round, hipMemcpyHostToDevice, h->stream));
    j.A = A;
    for (int r = 0; r < rounds; ++r) {
        j.rows = d_out + per_round * r;
        if (r > 0) HIPCHK(h, hipMemcpyAsync(j.rows, j.rows - per_round, sizeof(double) * per_round, hipMemcpyDeviceToDevice, h->stream));
        TRY(param_launch(h, h->stream, j, kSampleExplicit, 0, m, nullptr, 0));
    }
    TRY(s.finish());   // (rows0 lives until here)
    return F110_OK;
}

// ---- optional observation gather over RCCL / xGMI (BASELINE config 4) ---------------------------
// The step path has no collective: environments never interact and each rank's policy consumes
// its observations on the owning GPU.  For consumers that want every rank's scans on every GPU,
// this all-gathers them; RCCL is resolved at run time (dlopen) so the library has no link-time
// dependency on it and, inside a process that already loaded torch's RCCL, shares that copy.
namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;   // optional: gather to a root
    ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int *) = nullptr;
    ncclResult_t (*CommUserRank)(const ncclComm_t, int *) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};

RcclApi *rccl_api()
{
    static RcclApi api;
    static bool tried = false;
    if (!tried) {
        tried = true;
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) {
            api.lib = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (api.lib) break;
        }
        if (api.lib) {
            api.GetUniqueId = reinterpret_cast<decltype(api.GetUniqueId)>(dlsym(api.lib, "ncclGetUniqueId"));
            api.CommInitRank = reinterpret_cast<decltype(api.CommInitRank)>(dlsym(api.lib, "ncclCommInitRank"));
            api.AllGather = reinterpret_cast<decltype(api.AllGather)>(dlsym(api.lib, "ncclAllGather"));
            api.CommDestroy = reinterpret_cast<decltype(api.CommDestroy)>(dlsym(api.lib, "ncclCommDestroy"));
            api.GetErrorString = reinterpret_cast<decltype(api.GetErrorString)>(dlsym(api.lib, "ncclGetErrorString"));
            api.GroupStart = reinterpret_cast<decltype(api.GroupStart)>(dlsym(api.lib, "ncclGroupStart"));
            api.GroupEnd = reinterpret_cast<decltype(api.GroupEnd)>(dlsym(api.lib, "ncclGroupEnd"));
            api.CommCount = reinterpret_cast<decltype(api.CommCount)>(dlsym(api.lib, "ncclCommCount"));
            api.CommUserRank = reinterpret_cast<decltype(api.CommUserRank)>(dlsym(api.lib, "ncclCommUserRank"));
            api.Send = reinterpret_cast<decltype(api.Send)>(dlsym(api.lib, "ncclSend"));
            api.Recv = reinterpret_cast<decltype(api.Recv)>(dlsym(api.lib, "ncclRecv"));
        }
    }
    const bool ok = api.lib && api.GetUniqueId && api.CommInitRank && api.AllGather && api.CommDestroy && api.GetErrorString &&
                    api.GroupStart && api.GroupEnd && api.CommCount && api.CommUserRank;
    return ok ? &api : nullptr;
}
}  // namespace

int f110_comm_unique_id(void *out_id128)
{
    if (!out_id128) return fail(nullptr, F110_ERR_INVALID, "null argument");
    RcclApi *r = rccl_api();
    if (!r) return fail(nullptr, F110_ERR_STATE, "RCCL (librccl.so) could not be loaded");
    ncclUniqueId id;
    const ncclResult_t rc = r->GetUniqueId(&id);
    if (rc != ncclSuccess) return fail(nullptr, F110_ERR_HIP, "ncclGetUniqueId failed: %s", r->GetErrorString(rc));
    static_assert(sizeof(id) == F110_COMM_ID_BYTES, "ncclUniqueId size");
    memcpy(out_id128, &id, sizeof(id));
    return F110_OK;
}

int f110_comm_init(f110_sim *h, int32_t n_ranks, int32_t rank, const void *id128)
{
    if (!h || !id128 || n_ranks < 1 || rank < 0 || rank >= n_ranks) return fail(h, F110_ERR_INVALID, "f110_comm_init: bad argument");
    ENTER(h);
    RcclApi *r = rccl_api();
    if (!r) return fail(h, F110_ERR_STATE, "RCCL (librccl.so) could not be loaded");
    if (h->comm) return fail(h, F110_ERR_STATE, "communicator already initialised");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    const ncclResult_t rc = r->CommInitRank(&h->comm, n_ranks, id, rank);
    if (rc != ncclSuccess) {
        h->comm = nullptr;
        return fail(h, F110_ERR_HIP, "ncclCommInitRank failed: %s", r->GetErrorString(rc));
    }
    h->comm_ranks = n_ranks;
    h->comm_rank = rank;
    return F110_OK;
}

int f110_comm_set_overlap(f110_sim *h, int32_t enable)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (enable && !h->comm_overlap) {
        const size_t count = (size_t)h->N * h->cfg.num_beams;
        if (!h->scan_bufs[1]) {
            TRY(dmalloc(h, &h->scan_bufs[1], count));
            HIPCHK(h, hipMemsetAsync(h->scan_bufs[1], 0, sizeof(double) * count, h->stream));
            HIPCHK(h, hipStreamCreateWithFlags(&h->comm_stream, hipStreamNonBlocking));
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_step_done, hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_gather_done[0], hipEventDisableTiming));
            HIPCHK(h, hipEventCreateWithFlags(&h->ev_gather_done[1], hipEventDisableTiming));
        }
        h->scans_cur = 0;   // (dev.scans is scan_bufs[0] whenever the overlap is off)
        h->gather_pending[0] = h->gather_pending[1] = false;
        h->comm_swap_next = false;
        h->comm_overlap = true;
    } else if (!enable && h->comm_overlap) {
        if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
        if (h->scans_cur != 0) {   // back on the buffer the handle owns by name
            HIPCHK(h, hipMemcpyAsync(h->scan_bufs[0], h->scan_bufs[1], sizeof(double) * (size_t)h->N * h->cfg.num_beams, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipStreamSynchronize(h->stream));
            h->scans_cur = 0;
        }
        h->dev.scans = h->scan_bufs[0];
        h->comm_overlap = false;
    }
    return F110_OK;
}

// scans (+ the [7][N] scalar block when d_recv_scal != nullptr) of every rank to every rank.  The two
// ncclAllGather calls are one group (ncclGroupStart / End): RCCL fuses them into one launch per rank.
// transport F110_GATHER_F32: the scans cross the links as float32 (a conversion kernel in front of the collective; the
// receive buffer then holds floats) — half the bytes of the one leg that is link-bound.  root >= 0: only
// that rank receives (grouped ncclSend / ncclRecv: every peer's block rides its one direct xGMI link to the root; the
// other ranks receive nothing, 1 / n_ranks of the all-gather's receive volume per rank).
static int comm_gather(f110_sim *h, void *d_recv_scans, void *d_recv_scal, int transport = F110_GATHER_F64, int root = -1)
{
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (!h->comm) return fail(h, F110_ERR_STATE, "f110_comm_init has not been called");
    RcclApi *r = rccl_api();
    if (root >= h->comm_ranks) return fail(h, F110_ERR_INVALID, "f110_comm_gather_obs: root %d of %d ranks", root, h->comm_ranks);
    if (root >= 0 && (!r->Send || !r->Recv)) return fail(h, F110_ERR_STATE, "this RCCL has no ncclSend / ncclRecv: gather to a root is not available");
    const bool f32 = transport == F110_GATHER_F32;
    const bool i_receive = root < 0 || root == h->comm_rank;
    if (i_receive && !d_recv_scans) return fail(h, F110_ERR_INVALID, "null receive buffer on a receiving rank");
    const size_t N = (size_t)h->N, count = N * h->cfg.num_beams, scount = N * kObsScalars;
    const int cur = h->comm_overlap ? h->scans_cur : 0;
    const bool scal = d_recv_scal != nullptr || (root >= 0 && !i_receive && h->comm_send_scalars);
    if (scal && !h->obs_scal[cur]) {
        TRY(dmalloc(h, &h->obs_scal[cur], scount));   // (k_pack_obs writes every element before the gather reads it)
    }
    if (f32 && !h->scan_f32[cur]) TRY(dmalloc(h, &h->scan_f32[cur], count));
    auto gather_on = [&](hipStream_t st, const double *scans) -> int {
        const void *send = scans;
        const ncclDataType_t ty = f32 ? ncclFloat32 : ncclFloat64;
        const size_t esz = f32 ? sizeof(float) : sizeof(double);
        if (f32) {
            hipLaunchKernelGGL(k_scans_to_f32, grid1d(count, 256), dim3(256), 0, st, scans, h->scan_f32[cur], count);
            send = h->scan_f32[cur];
        }
        ncclResult_t rc = r->GroupStart();
        if (root < 0) {
            if (rc == ncclSuccess) rc = r->AllGather(send, d_recv_scans, count, ty, h->comm, st);
            if (rc == ncclSuccess && d_recv_scal) rc = r->AllGather(h->obs_scal[cur], d_recv_scal, scount, ncclFloat64, h->comm, st);
        } else {
            if (rc == ncclSuccess) rc = r->Send(send, count, ty, root, h->comm, st);
            if (rc == ncclSuccess && scal) rc = r->Send(h->obs_scal[cur], scount, ncclFloat64, root, h->comm, st);
            if (i_receive) {
                for (int p = 0; p < h->comm_ranks && rc == ncclSuccess; ++p) {
                    rc = r->Recv(static_cast<char *>(d_recv_scans) + (size_t)p * count * esz, count, ty, p, h->comm, st);
                    if (rc == ncclSuccess && d_recv_scal)
                        rc = r->Recv(static_cast<double *>(d_recv_scal) + (size_t)p * scount, scount, ncclFloat64, p, h->comm, st);
                }
            }
        }
        const ncclResult_t re = r->GroupEnd();
        if (rc == ncclSuccess) rc = re;
        if (rc != ncclSuccess) return fail(h, F110_ERR_HIP, "RCCL gather failed: %s", r->GetErrorString(rc));
        return F110_OK;
    };
    if (!h->comm_overlap) {
        ENTER(h);
        if (scal) hipLaunchKernelGGL(k_pack_obs, grid1d(N, 256), dim3(256), 0, h->stream, h->dev, h->obs_scal[0]);
        return gather_on(h->stream, h->dev.scans);
    }
    // overlapped: the gather waits for the step that produced this buffer and runs beside the next one,
    // which writes the other buffer; the step after that waits for this gather before reusing the buffer
    {
        const bool inflight = h->comm_inflight;   // join the groups, not earlier gathers (they stay asynchronous)
        h->comm_inflight = false;
        const int rj = join_groups(h);
        h->comm_inflight = inflight;
        if (rj != F110_OK) return rj;
    }
    // the scalar block is packed on the main stream, behind the step and before anything (a re-seat, the
    // next step) can change the state it reads; obs_scal[cur] was last read by the gather of two steps ago,
    // which the step that just ran has waited for
    if (scal) {
        hipLaunchKernelGGL(k_pack_obs, grid1d(N, 256), dim3(256), 0, h->stream, h->dev, h->obs_scal[cur]);
        // k_pack_obs READS state[] on the main stream: a next step that goes out as two env blocks must fork from it
        // (its second block's k_integrate would otherwise overwrite the state under the pack) — ADVICE r4
        h->main_dirty = true;
    }
    HIPCHK(h, hipEventRecord(h->ev_step_done, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->comm_stream, h->ev_step_done, 0));
    TRY(gather_on(h->comm_stream, h->scan_bufs[cur]));
    HIPCHK(h, hipEventRecord(h->ev_gather_done[cur], h->comm_stream));
    h->gather_pending[cur] = true;
    h->comm_swap_next = true;
    h->comm_inflight = true;
    return F110_OK;
}

int f110_comm_all_gather_scans(f110_sim *h, void *d_recv)
{
    if (!h || !d_recv) return fail(h, F110_ERR_INVALID, "null argument");
    return comm_gather(h, d_recv, nullptr);
}

int f110_comm_all_gather_obs(f110_sim *h, void *d_recv_scans, void *d_recv_scalars)
{
    if (!h || !d_recv_scans || !d_recv_scalars) return fail(h, F110_ERR_INVALID, "null argument");
    return comm_gather(h, d_recv_scans, d_recv_scalars);
}

int f110_comm_gather_obs(f110_sim *h, void *d_recv_scans, void *d_recv_scalars, int32_t transport, int32_t root)
{
    if (!h) return fail(h, F110_ERR_INVALID, "null handle");
    if (transport != F110_GATHER_F64 && transport != F110_GATHER_F32) return fail(h, F110_ERR_INVALID, "f110_comm_gather_obs: unknown transport %d", transport);
    // a rank that is not the root sends its scalar block exactly when the root asked for one: the ranks agree on that
    // through this flag's convention — a sender passes a non-null d_recv_scalars (never written) to say "with scalars"
    h->comm_send_scalars = d_recv_scalars != nullptr;
    return comm_gather(h, d_recv_scans, d_recv_scalars, transport, root);
}

int f110_comm_info(f110_sim *h, int32_t *n_ranks, int32_t *rank)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!h->comm) return fail(h, F110_ERR_STATE, "f110_comm_init has not been called");
    RcclApi *r = rccl_api();
    int n = 0, me = -1;
    ncclResult_t rc = r->CommCount(h->comm, &n);
    if (rc == ncclSuccess) rc = r->CommUserRank(h->comm, &me);
    if (rc != ncclSuccess) return fail(h, F110_ERR_HIP, "ncclCommCount / ncclCommUserRank failed: %s", r->GetErrorString(rc));
    if (n_ranks) *n_ranks = n;
    if (rank) *rank = me;
    return F110_OK;
}

int f110_comm_destroy(f110_sim *h)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (h->comm) {
        if (h->comm_stream) HIPCHK(h, hipStreamSynchronize(h->comm_stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        RcclApi *r = rccl_api();
        if (r) (void)r->CommDestroy(h->comm);
        h->comm = nullptr;
        h->comm_ranks = 0;
    }
    return F110_OK;
}

// ---- episode logic (f110_env.py:204-246,306-338) -----------------------------------------------
int f110_episode_init(f110_sim *h, int32_t ego_idx)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (ego_idx < 0 || ego_idx >= h->cfg.num_agents) return fail(h, F110_ERR_INVALID, "Index given is out of bounds for list of agents.");
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs;
    EpisodeArrays &ep = h->ep;
    if (!h->has_episode) {
        h->ep_mem.clear();   // (an earlier attempt that ran out of memory half-way)
        TRY(dmalloc(h, h->ep_mem, &ep.start_poses, 3 * N));
        TRY(dmalloc(h, h->ep_mem, &ep.rot, 4 * E));
        TRY(dmalloc(h, h->ep_mem, &ep.current_time, E));
        TRY(dmalloc(h, h->ep_mem, &ep.near_start, N));
        TRY(dmalloc(h, h->ep_mem, &ep.toggle, N));
        TRY(dmalloc(h, h->ep_mem, &ep.lap_count, N));
        TRY(dmalloc(h, h->ep_mem, &ep.lap_time, N));
        TRY(dmalloc(h, h->ep_mem, &ep.done, E));
        TRY(dmalloc(h, h->ep_mem, &ep.checkpoint, N));
        TRY(dmalloc(h, h->ep_mem, &h->d_rot_stage, 4 * E));
        HIPCHK(h, hipMemsetAsync(ep.start_poses, 0, 3 * N * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(ep.rot, 0, 4 * E * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(ep.current_time, 0, E * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(ep.near_start, 1, N, h->stream));
        HIPCHK(h, hipMemsetAsync(ep.toggle, 0, N * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(ep.lap_count, 0, N * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(ep.lap_time, 0, N * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(ep.done, 0, E, h->stream));
        HIPCHK(h, hipMemsetAsync(ep.checkpoint, 0, N, h->stream));
        h->has_episode = true;
    }
    ep.ego_idx = ego_idx;
    ep.timestep = h->cfg.time_step;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_episode_reset(f110_sim *h, const double *poses, const double *rot, const uint8_t *env_mask)
{
    if (!h || !poses || !rot) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    HIPCHK(h, hipMemcpyAsync(h->d_poses, poses, sizeof(double) * 3 * h->N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_rot_stage, rot, sizeof(double) * 4 * h->cfg.num_envs, hipMemcpyHostToDevice, h->stream));
    if (env_mask) HIPCHK(h, hipMemcpyAsync(h->d_mask, env_mask, (size_t)h->cfg.num_envs, hipMemcpyHostToDevice, h->stream));
    const uint8_t *dm = env_mask ? h->d_mask : nullptr;
    if (!dm) h->noise_ub = 0;
    hipLaunchKernelGGL(k_episode_reset, grid1d(h->N, 256), dim3(256), 0, h->stream, h->dev, h->ep, h->d_poses, h->d_rot_stage, dm);
    hipLaunchKernelGGL(k_reset, grid1d(h->N, 256), dim3(256), 0, h->stream, h->dev, h->d_poses, dm);
    if (h->rs.on)
        hipLaunchKernelGGL(k_sampler_keep, grid1d(h->N, 256), dim3(256), 0, h->stream, h->rs.job.last, h->d_poses, dm, h->N, h->cfg.num_agents);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_episode_step_device(f110_sim *h, const double *d_actions)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    TRY(check_step(h, d_actions != nullptr));
    StepRequest rq;
    rq.defer_draw = true;
    bool host_written = false;
    TRY(step_submit(h, d_actions, rq, host_written));
    // _check_done behind the step: after a two-block step on each block's own stream (an env's lap bookkeeping reads that env's
    // agents only), no join — the device-resident loop stays two independent halves.  (Right after a successful step `touched`
    // is false, so the follow rule's `!touched` changes nothing here.)
    EnvBlocks w;
    TRY(env_blocks_follow(h, w));
    for (const EnvBlock &b : w) hipLaunchKernelGGL(k_episode, grid1d(b.count, 256), dim3(256), 0, b.stream, h->dev, h->ep, b.count, b.e0);
    HIPCHK(h, hipGetLastError());
    if (reseat_draws(h) && h->dev.reseat_poses) TRY(sampler_after_step(h, w));
    h->touched = false;
    return F110_OK;
}

int f110_episode_reset_done_device(f110_sim *h, int32_t *d_count)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    if (h->rs.on && (h->tracks_dirty || !h->track_checked)) {   // (the slot table is current behind any step of an armed sampler)
        HIPCHK(h, hipSetDevice(h->cfg.device_id));
        TRY(track_prepare(h));
    }
    EnvBlocks w;   // behind a two-block f110_episode_step_device: per block, no join (a re-seat touches the finished env's own agents only)
    TRY(env_blocks_follow(h, w));
    const int A = h->cfg.num_agents;
    for (const EnvBlock &b : w) {
        hipLaunchKernelGGL(k_episode_reset_done, grid1d(b.count * A, 256), dim3(256), 0, b.stream, h->dev, h->ep, d_count, b.e0 * A, b.count * A);
        if (reseat_draws(h)) TRY(reseat_launch(h, b.stream, kSampleDone, b.e0, b.count, 0));   // (done[] is still set)
        hipLaunchKernelGGL(k_episode_clear_done, grid1d(b.count, 256), dim3(256), 0, b.stream, h->ep, b.count, b.e0);
    }
    HIPCHK(h, hipGetLastError());
    h->touched = false;   // (the loop step / reset_done / step / ... may split from its second round on)
    return F110_OK;
}

size_t f110_episode_packed_bytes(const f110_sim *h)
{
    if (!h) return 0;
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs;
    return (9 * N + E) * sizeof(double) + 2 * N + E;
}

int f110_host_alloc(f110_sim *h, size_t bytes, void **out)
{
    if (!h || !out) return fail(h, F110_ERR_INVALID, "null argument");
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipHostMalloc(out, bytes > 0 ? bytes : 8, hipHostMallocDefault));
    std::lock_guard<std::mutex> lk(g_registry_mu);
    g_host_blocks[static_cast<const char *>(*out)] = bytes > 0 ? bytes : 8;
    return F110_OK;
}

int f110_host_free(f110_sim *h, void *p)
{
    if (!p) return F110_OK;
    if (h) {   // the handle's stream may still be copying from / into the block
        ENTER(h);
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    {
        // every live handle forgets what it cached about this block; a handle with an F110_STEP_NO_SYNC step still storing
        // into it is drained first (the caller may pass h = NULL: the block outlives the handle that allocated it)
        std::lock_guard<std::mutex> lk(g_registry_mu);
        const char *lo = static_cast<const char *>(p);
        const auto it = g_host_blocks.find(lo);
        const char *hi = lo + (it != g_host_blocks.end() ? it->second : 1);
        auto inside = [&](const void *q) { return q && static_cast<const char *>(q) >= lo && static_cast<const char *>(q) < hi; };
        for (f110_sim *o : g_handles) {
            if (o->trk_pinned_on) {
                const f110_track_host &t = o->trk_pinned;
                const void *tp[] = {t.s, t.ds, t.lateral, t.heading_error, t.segment};
                bool thit = false;
                for (const void *q : tp) thit = thit || inside(q);
                if (thit) {
                    if (o != h) {
                        (void)hipSetDevice(o->cfg.device_id);
                        (void)hipStreamSynchronize(o->stream);
                    }
                    o->trk_pinned_on = false;
                    o->trk_pinned = f110_track_host{};
                }
            }
            bool drained = false;
            for (const float *&dst : o->pinned_dst) {
                if (!inside(dst)) continue;
                if (!drained) {   // a device form's copy (on the env blocks' streams) may still be on its way into the block
                    (void)hipSetDevice(o->cfg.device_id);
                    for (hipStream_t gs : o->gstreams) (void)hipStreamSynchronize(gs);
                    (void)hipStreamSynchronize(o->stream);
                    drained = true;
                }
                dst = nullptr;
            }
            if (!o->hb_valid && !o->fused_valid) continue;
            const f110_host_block &b = o->hb_host;
            const void *ptrs[] = {b.scans, b.state, b.agent_poses, b.collisions, b.collision_idx, b.in_collision, b.lap_times, b.lap_counts, b.toggles,
                                  b.current_time, b.near_starts, b.done, b.checkpoint_done, o->hb_actions_host};
            bool hit = false;
            for (const void *q : ptrs) hit = hit || inside(q);
            if (!hit) continue;
            if (o != h) {
                (void)hipSetDevice(o->cfg.device_id);
                (void)hipStreamSynchronize(o->stream);
            }
            o->hb_valid = false;
            o->fused_valid = false;
        }
        if (it != g_host_blocks.end()) g_host_blocks.erase(it);
    }
    HIPCHK(h, hipHostFree(p));
    return F110_OK;
}

int f110_episode_step_host(f110_sim *h, const double *h_actions, int32_t auto_reset, void *h_packed)
{
    if (!h || !h_actions || !h_packed) return fail(h, F110_ERR_INVALID, "null argument");
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    TRY(check_step(h, true));
    ENTER(h);
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs, bytes = f110_episode_packed_bytes(h);
    if (!h->d_packed) TRY(dmalloc(h, &h->d_packed, bytes));
    HIPCHK(h, hipMemcpyAsync(h->d_actions, h_actions, sizeof(double) * 2 * N, hipMemcpyHostToDevice, h->stream));
    StepRequest rq;
    rq.defer_draw = true;
    bool host_written = false;
    TRY(step_submit(h, h->d_actions, rq, host_written));
    ENTER(h);
    hipLaunchKernelGGL(k_episode, grid1d(E, 256), dim3(256), 0, h->stream, h->dev, h->ep, (int)E);
    double *cols = reinterpret_cast<double *>(h->d_packed.get());
    uint8_t *flags = reinterpret_cast<uint8_t *>(cols + 9 * N + E);
    hipLaunchKernelGGL(k_pack_episode, grid1d(N > E ? N : E, 256), dim3(256), 0, h->stream, h->dev, h->ep, (int)E, cols, flags);
    HIPCHK(h, hipMemcpyAsync(h_packed, h->d_packed, bytes, hipMemcpyDeviceToHost, h->stream));
    if (auto_reset) {   // the packed block holds the terminal observation; the re-seat follows it
        hipLaunchKernelGGL(k_episode_reset_done, grid1d(N, 256), dim3(256), 0, h->stream, h->dev, h->ep, (int32_t *)nullptr);
        hipLaunchKernelGGL(k_episode_clear_done, grid1d(E, 256), dim3(256), 0, h->stream, h->ep, (int)E);
    }
    HIPCHK(h, hipGetLastError());
    if (reseat_draws(h) && (auto_reset || h->dev.reseat_poses)) TRY(sampler_after_step(h, env_blocks_main(h)));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

// One entry per env.step() of a host-driven loop (f110.h).  Every pointer of `out` and — with
// F110_STEP_ACTIONS_MAPPED — h_actions must be page-locked memory of f110_host_alloc: the kernels read / write
// it in place.  The (struct, actions) pair is validated once (hipHostGetDevicePointer) and remembered.
constexpr size_t kScansByKernelBytes = 8u << 20;   // scans up to this size ride in the host-block kernel instead of a DMA copy

static int map_host_ptr(f110_sim *h, const void *host, void **dev, const char *what)
{
    *dev = nullptr;
    if (!host) return F110_OK;
    if (hipHostGetDevicePointer(dev, const_cast<void *>(host), 0) != hipSuccess || !*dev) {
        (void)hipGetLastError();
        return fail(h, F110_ERR_INVALID, "f110_step_host: %s is not page-locked memory of f110_host_alloc", what);
    }
    return F110_OK;
}

// the device view of the caller's block (and of its actions, when they are read in place): kept until either changes
static int host_block_bind(f110_sim *h, const double *h_actions, const f110_host_block *out, bool mapped_actions)
{
    if (h->hb_valid && std::memcmp(&h->hb_host, out, sizeof *out) == 0 && h->hb_actions_host == (mapped_actions ? h_actions : nullptr)) return F110_OK;
    const size_t N = (size_t)h->N;
    HostBlock d{};
    void *p = nullptr;
#define MAP_FIELD(dst, src, name)                     \
    do {                                              \
        TRY(map_host_ptr(h, out->src, &p, name));     \
        d.dst = reinterpret_cast<decltype(d.dst)>(p); \
    } while (0)
    MAP_FIELD(state, state, "state");
    MAP_FIELD(collisions, collisions, "collisions");
    MAP_FIELD(collision_idx, collision_idx, "collision_idx");
    MAP_FIELD(agent_poses, agent_poses, "agent_poses");
    MAP_FIELD(lap_time, lap_times, "lap_times");
    MAP_FIELD(lap_count, lap_counts, "lap_counts");
    MAP_FIELD(toggle, toggles, "toggles");
    MAP_FIELD(current_time, current_time, "current_time");
    MAP_FIELD(in_collision, in_collision, "in_collision");
    MAP_FIELD(near_start, near_starts, "near_starts");
    MAP_FIELD(checkpoint, checkpoint_done, "checkpoint_done");
    MAP_FIELD(done, done, "done");
#undef MAP_FIELD
    // scans of a small batch: stored by the kernel too (needs page-locked memory; else, and for big batches, the DMA copy)
    d.scans = nullptr;
    d.num_beams = h->cfg.num_beams;
    h->hb_scans_by_kernel = false;
    if (out->scans && N * (size_t)h->cfg.num_beams * sizeof(double) <= kScansByKernelBytes) {
        void *ps = nullptr;
        if (hipHostGetDevicePointer(&ps, out->scans, 0) == hipSuccess && ps) {
            d.scans = reinterpret_cast<double *>(ps);
            h->hb_scans_by_kernel = true;
        } else {
            (void)hipGetLastError();
        }
    }
    TRY(map_host_ptr(h, mapped_actions ? h_actions : nullptr, &p, "h_actions"));
    h->hb_actions_dev = reinterpret_cast<const double *>(p);
    h->hb_actions_host = mapped_actions ? h_actions : nullptr;
    h->hb_dev = d;
    h->hb_host = *out;
    h->hb_valid = true;
    return F110_OK;
}

typedef std::chrono::steady_clock::time_point host_time;

// f110_step_host's way out: the completion word (spin), the bounded poll of the stream, or the runtime's wait
static int host_step_wait(f110_sim *h, int32_t flags, bool spin, bool tiny, host_time t_in, host_time t_enq)
{
    if (spin) {
        // poll the completion word the last workgroup stores (no runtime call on the way out); a kernel that
        // never signals (a device fault) is caught by the runtime after the spin budget
        const unsigned long long want = h->hb_seq;
        const volatile unsigned long long *w = h->hb_seq_host;
        bool seen = false;
        if (kExperimental && h->exp.tiny_start_probe && tiny && h->tiny.start_word) {
            for (long it = 0; it < 200000000L && __atomic_load_n(w + 1, __ATOMIC_ACQUIRE) != want; ++it) __builtin_ia32_pause();
            const auto t_start = std::chrono::steady_clock::now();
            for (long it = 0; it < 200000000L && __atomic_load_n(w, __ATOMIC_ACQUIRE) != want; ++it) __builtin_ia32_pause();
            const auto t_done = std::chrono::steady_clock::now();
            h->exp.probe_calls += 1;
            h->exp.probe_us[0] += std::chrono::duration<double, std::micro>(t_enq - t_in).count();
            h->exp.probe_us[1] += std::chrono::duration<double, std::micro>(t_start - t_enq).count();
            h->exp.probe_us[2] += std::chrono::duration<double, std::micro>(t_done - t_start).count();
        }
        for (long it = 0; it < 2000000000L; ++it) {
            if (__atomic_load_n(w, __ATOMIC_ACQUIRE) == want) {
                seen = true;
                break;
            }
            __builtin_ia32_pause();
            if ((it & 0xfffff) == 0xfffff &&
                std::chrono::duration<double>(std::chrono::steady_clock::now() - t_enq).count() > 5.0) break;
        }
        if (!seen) HIPCHK(h, hipStreamSynchronize(h->stream));
    } else if (!(flags & F110_STEP_NO_SYNC)) {
        if (flags & F110_STEP_POLL) {
            // hipStreamSynchronize wakes up in coarse quanta once a wait has lasted ~30 us (measured: a 40 us step is
            // reported after 67 us); polling the stream costs a core for the step's duration and returns within ~1 us
            // ... so the poll is BOUNDED: a step that has not finished after kPollBudgetUs hands the core back and
            // sleeps in hipStreamSynchronize — the coarse wake-up is then a few per cent of a long wait, and ranks that share a
            // CPU quota (8 ranks on 16 cores on the bench box) do not spin against their own policy threads
            constexpr double kPollBudgetUs = 250.0;
            hipError_t q;
            uint32_t it = 0;
            while ((q = hipStreamQuery(h->stream)) == hipErrorNotReady) {
                __builtin_ia32_pause();
                if ((++it & 0x3fu) == 0u && std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_enq).count() > kPollBudgetUs) break;
            }
            if (q == hipErrorNotReady) HIPCHK(h, hipStreamSynchronize(h->stream));
            else if (q != hipSuccess) return fail(h, F110_ERR_HIP, "hipStreamQuery failed: %s", hipGetErrorString(q));
        } else {
            HIPCHK(h, hipStreamSynchronize(h->stream));
        }
    }
    return F110_OK;
}

int f110_step_host(f110_sim *h, const double *h_actions, const f110_host_block *out, int32_t flags)
{
    TRY(check_step(h, h_actions && out));
    const bool episode = h->has_episode;
    if (!episode && (out->lap_times || out->lap_counts || out->toggles || out->current_time || out->near_starts ||
                     out->checkpoint_done || out->done || (flags & F110_STEP_AUTO_RESET)))
        return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    const bool scripted = (flags & F110_STEP_SCRIPTED) != 0;
    if (scripted && h->gap_specs == 0 && h->line_specs == 0 && h->mppi.on.m == 0)
        return fail(h, F110_ERR_STATE, "f110_step_host: F110_STEP_SCRIPTED without controllers (f110_controllers_set), line followers (f110_line_followers_set) or a planner (f110_mppi_set)");
    if (scripted && h->line_specs > 0) TRY(line_ready(h));
    if (scripted && h->mppi.on.m > 0) TRY(mppi_ready(h));
    ENTER(h);
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs;
    // scripted cars: the actions always go through the staging buffer, where the controllers overwrite their agents' rows
    const bool mapped_actions = (flags & F110_STEP_ACTIONS_MAPPED) != 0 && !scripted;
    TRY(host_block_bind(h, h_actions, out, mapped_actions));
    const auto t_in = std::chrono::steady_clock::now();
    // a tiny batch is one launch whose last workgroup writes the block (k_step_tiny): its completion is ONE word stored by one
    // workgroup, so the host always waits on that word (no runtime call on the way out)
    const bool tiny = tiny_applies(h) && !(flags & (F110_STEP_NO_FUSE | F110_STEP_NO_SYNC | F110_STEP_SCRIPTED)) && !h->dev.reseat_poses;
    const bool spin = ((flags & F110_STEP_SPIN_WAIT) || tiny) && !(flags & F110_STEP_NO_SYNC) && (!out->scans || (h->hb_valid && h->hb_scans_by_kernel));
    if (spin && !h->hb_seq_host) {
        HIPCHK(h, hipHostMalloc(reinterpret_cast<void **>(&h->hb_seq_host), 64, hipHostMallocDefault));
        *h->hb_seq_host = 0;
        TRY(dmalloc(h, &h->hb_blocks_done, 1));
        HIPCHK(h, hipMemsetAsync(h->hb_blocks_done, 0, sizeof(unsigned int), h->stream));
    }
    const double *d_act = h->d_actions;
    if (mapped_actions)
        d_act = h->hb_actions_dev;   // k_integrate reads the [N][2] block over PCIe, once, coalesced
    else if (!tiny)                  // (k_step_tiny gets the actions as kernel arguments)
        HIPCHK(h, hipMemcpyAsync(h->d_actions, h_actions, sizeof(double) * 2 * N, hipMemcpyHostToDevice, h->stream));
    if (scripted) {   // the scans are the last step's, the staged rows of scripted agents are replaced, external rows stay
        if (h->gap_specs > 0) gap_launch_armed(h, EnvBlock{h->stream, 0, h->cfg.num_envs}, h->d_actions);
        if (h->line_specs > 0) {   // the line followers: their agents' rows, from the track columns of the last step
            TRY(track_upload(h));
            line_launch_armed(h, EnvBlock{h->stream, 0, h->cfg.num_envs}, h->d_actions, nullptr);
        }
        if (h->mppi.on.m > 0) {   // the planner behind the controllers: its agents' rows, from the live state
            TRY(mppi_upload_tracks(h));
            TRY(mppi_launch_armed(h, EnvBlock{h->stream, 0, h->cfg.num_envs}, h->d_actions, nullptr));
        }
        HIPCHK(h, hipGetLastError());
    }
    const int A = h->cfg.num_agents;
    StepRequest rq;
    rq.tiny = tiny;
    rq.tiny_actions = tiny ? h_actions : nullptr;
    rq.episode = episode ? 1 : 0;
    rq.auto_reset = (flags & F110_STEP_AUTO_RESET) ? 1 : 0;
    rq.defer_draw = true;   // (the draw follows the host block, below)
    HostBlock hbk = h->hb_dev;
    if (spin) {
        void *p = nullptr;
        TRY(map_host_ptr(h, h->hb_seq_host, &p, "completion word"));
        hbk.seq_host = reinterpret_cast<unsigned long long *>(p);
        hbk.blocks_done = h->hb_blocks_done;
        hbk.seq = ++h->hb_seq;
    }
    // A = 2: the pair kernel can carry the host block and the episode logic as its epilogue (one launch and one drain
    // less per step); its parameters live in device memory and are rewritten only when they change
    // (not with F110_STEP_SPIN_WAIT: the completion word needs a system-scope release per workgroup, and the pair kernel
    // has N / 32 of them with the scan's dirty lines still in L2 — measured 0.657 -> 0.767 ms at 32 768 envs)
    // tracking: the track columns are computed behind the step's last kernel, so the host block is k_host_block (no epilogue)
    rq.fuse = A == 2 && !(flags & F110_STEP_NO_FUSE) && (!spin || tiny) && !h->track_on;
    if (h->track_on && h->trk_pinned_on) {
        hbk.trk_src = h->d_trk;
        hbk.trk_seg_src = h->d_trk_seg;
        hbk.trk_s = h->trk_hb.trk_s;
        hbk.trk_ds = h->trk_hb.trk_ds;
        hbk.trk_lat = h->trk_hb.trk_lat;
        hbk.trk_head = h->trk_hb.trk_head;
        hbk.trk_seg = h->trk_hb.trk_seg;
    }
    if (rq.fuse) {
        FusedHost fh{};
        if (episode) fh.ep = h->ep;
        fh.hb = hbk;
        fh.hb.seq = 0;   // (the sequence number travels in the kernel arguments: rq.seq)
        fh.episode = rq.episode;
        fh.auto_reset = rq.auto_reset;
        if (!h->d_fused) TRY(dmalloc(h, &h->d_fused, 1));
        if (!h->fused_valid || std::memcmp(&fh, &h->fused_host_copy, sizeof fh) != 0) {
            h->fused_host_copy = fh;
            HIPCHK(h, hipMemcpyAsync(h->d_fused, &h->fused_host_copy, sizeof fh, hipMemcpyHostToDevice, h->stream));
            h->fused_valid = true;
        }
    }
    rq.seq = spin ? hbk.seq : 0;
    if (tiny && A == 1 && !h->track_on) rq.hb = &hbk;
    bool host_written = false;
    TRY(step_submit(h, d_act, rq, host_written));
    ENTER(h);
    if (!host_written) {
        const int epb = A >= 256 ? 1 : 256 / A;
        hipLaunchKernelGGL(k_host_block, dim3((unsigned)((E + epb - 1) / epb)), dim3(256), 0, h->stream, h->dev, h->ep, hbk, (int)E, epb,
                           rq.episode, rq.auto_reset);
    }
    // the scans are contiguous in HBM already: a DMA copy, behind the kernel (the re-seat leaves scans alone)
    if (out->scans && !h->hb_scans_by_kernel) HIPCHK(h, hipMemcpyAsync(out->scans, h->dev.scans, sizeof(double) * N * (size_t)h->cfg.num_beams, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipGetLastError());
    // a re-seat inside this call (auto reset, or an armed f110_set_auto_reseat): the draw, behind the block (which keeps the
    // terminal observation), stream-ordered in front of the next step
    if (reseat_draws(h) && (rq.auto_reset || h->dev.reseat_poses)) TRY(sampler_after_step(h, env_blocks_main(h)));
    const auto t_enq = std::chrono::steady_clock::now();
    TRY(host_step_wait(h, flags, spin, tiny, t_in, t_enq));
    const auto t_out = std::chrono::steady_clock::now();
    h->hs_enqueue_us += std::chrono::duration<double, std::micro>(t_enq - t_in).count();
    h->hs_wait_us += std::chrono::duration<double, std::micro>(t_out - t_enq).count();
    h->hs_calls += 1;
    return F110_OK;
}

int f110_step_host_stats(f110_sim *h, double *out3)
{
    if (!h || !out3) return fail(h, F110_ERR_INVALID, "null argument");
    out3[0] = (double)h->hs_calls;
    out3[1] = h->hs_enqueue_us;
    out3[2] = h->hs_wait_us;
    h->hs_calls = 0;
    h->hs_enqueue_us = h->hs_wait_us = 0;
    return F110_OK;
}

int f110_episode_get(f110_sim *h, const f110_episode_host *o)
{
    if (!h || !o) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    const size_t N = (size_t)h->N, E = (size_t)h->cfg.num_envs;
    const EpisodeArrays &ep = h->ep;
    TRY(copy_col(h, o->lap_times, ep.lap_time, N));
    TRY(copy_col(h, o->lap_counts, ep.lap_count, N));
    TRY(copy_col(h, o->toggles, ep.toggle, N));
    TRY(copy_col(h, o->current_time, ep.current_time, E));
    if (o->near_starts) HIPCHK(h, hipMemcpyAsync(o->near_starts, ep.near_start, N, hipMemcpyDeviceToHost, h->stream));
    if (o->done) HIPCHK(h, hipMemcpyAsync(o->done, ep.done, E, hipMemcpyDeviceToHost, h->stream));
    if (o->checkpoint_done) HIPCHK(h, hipMemcpyAsync(o->checkpoint_done, ep.checkpoint, N, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_episode_device_views(f110_sim *h, f110_episode_views *v)
{
    if (!h || !v) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    v->done = h->ep.done;
    v->checkpoint_done = h->ep.checkpoint;
    v->lap_times = h->ep.lap_time;
    v->lap_counts = h->ep.lap_count;
    v->toggles = h->ep.toggle;
    v->current_time = h->ep.current_time;
    return F110_OK;
}

int f110_episode_start_views(f110_sim *h, double **d_start_poses, double **d_start_rot)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (!h->has_episode) return fail(h, F110_ERR_STATE, "f110_episode_init has not been called");
    if (d_start_poses) *d_start_poses = h->ep.start_poses;
    if (d_start_rot) *d_start_rot = h->ep.rot;
    return F110_OK;
}

int f110_reset(f110_sim *h, const double *poses, const uint8_t *env_mask)
{
    if (!h || !poses) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    HIPCHK(h, hipMemcpyAsync(h->d_poses, poses, sizeof(double) * 3 * h->N, hipMemcpyHostToDevice, h->stream));
    if (env_mask) HIPCHK(h, hipMemcpyAsync(h->d_mask, env_mask, (size_t)h->cfg.num_envs, hipMemcpyHostToDevice, h->stream));
    TRY(f110_reset_device(h, h->d_poses, env_mask ? h->d_mask : nullptr));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // host buffers are consumed on return
    return F110_OK;
}

static hipEvent_t prof_event(f110_sim *h)
{
    if (h->prof_used == h->prof_events.size()) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        h->prof_events.push_back(e);
    }
    return h->prof_events[h->prof_used++];
}

// rows [noise_rows_ready, upto) of the shared stream into the row cache (stream-ordered on the main stream)
static int noise_cache_extend(f110_sim *h, int upto)
{
    const int cap = h->dev.noise_rows;
    if (upto > cap) upto = cap;
    if (upto <= h->noise_rows_ready) return F110_OK;
    if (upto > h->noise_rows_alloc) {
        // grow the cache's memory (doubling, capped): the rows generated so far move to the new block
        const size_t B = (size_t)h->cfg.num_beams;
        const int want = std::min(cap, std::max(2 * h->noise_rows_alloc, upto));
        DevBuf<double> bigger;
        TRY(dmalloc(h, &bigger, (size_t)want * B));
        HIPCHK(h, hipMemcpyAsync(bigger, h->d_noise, sizeof(double) * (size_t)h->noise_rows_ready * B, hipMemcpyDeviceToDevice, h->stream));
        h->noise_retired.push_back(std::move(h->d_noise));   // earlier steps (env blocks on their own streams) may still read the old block
        h->d_noise = std::move(bigger);
        h->dev.noise = h->d_noise;
        h->noise_rows_alloc = want;
    }
    hipLaunchKernelGGL(k_noise_cache, dim3(1), dim3(64), 0, h->stream, h->noise_gen, h->dev.rng_inc, h->d_rng_rowstate, h->d_noise, h->noise_rows_ready, upto,
                       h->cfg.num_beams);
    HIPCHK(h, hipGetLastError());
    h->noise_rows_ready = upto;
    h->main_dirty = true;
    return F110_OK;
}

// The next doubling of the row cache, started on the noise stream when HALF of the rows there are have been used: generation (12.8 us a
// row) is faster than any step loop uses rows (a step of one env takes 30 us and more), so the rows are there when the episode reaches
// them and no step waits.  The rows so far are immutable; a cache that outgrows its memory continues in a new block (old rows copied
// on the same stream), which becomes THE cache at adoption — kernels get the block's address with every launch.
static int noise_start_ahead(f110_sim *h)
{
    const int cap = h->dev.noise_rows, ready = h->noise_rows_ready;
    const int upto = (int)std::min<long long>(cap, 2LL * ready);
    if (h->noise_ahead || upto <= ready) return F110_OK;
    if (!h->noise_stream) {
        HIPCHK(h, hipStreamCreateWithFlags(&h->noise_stream, hipStreamNonBlocking));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_noise, hipEventDisableTiming));
        HIPCHK(h, hipEventCreateWithFlags(&h->ev_noise_src, hipEventDisableTiming));
    }
    const size_t B = (size_t)h->cfg.num_beams;
    // behind whatever produced the rows so far (the main stream: f110_set_noise_rng, a step that could not wait; or this stream)
    HIPCHK(h, hipEventRecord(h->ev_noise_src, h->stream));
    HIPCHK(h, hipStreamWaitEvent(h->noise_stream, h->ev_noise_src, 0));
    double *block = h->d_noise;   // the rows fit the cache's block, or they go into a new one that noise_ahead_block owns until adoption
    int alloc = h->noise_rows_alloc;
    if (upto > alloc) {
        alloc = std::min(cap, std::max(2 * alloc, upto));
        TRY(dmalloc(h, &h->noise_ahead_block, (size_t)alloc * B));
        block = h->noise_ahead_block;
        HIPCHK(h, hipMemcpyAsync(block, h->d_noise, sizeof(double) * (size_t)ready * B, hipMemcpyDeviceToDevice, h->noise_stream));
    }
    hipLaunchKernelGGL(k_noise_cache, dim3(1), dim3(64), 0, h->noise_stream, h->noise_gen, h->dev.rng_inc, h->d_rng_rowstate, block, ready, upto, h->cfg.num_beams);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev_noise, h->noise_stream));
    h->noise_ahead = true;
    h->noise_ahead_upto = upto;
    h->noise_ahead_alloc = alloc;
    return F110_OK;
}

// ... and taken over by the main stream (which waits for them, if they are not there yet)
static int noise_adopt(f110_sim *h)
{
    if (!h->noise_ahead) return F110_OK;
    HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_noise, 0));
    if (h->noise_ahead_block) {
        h->noise_retired.push_back(std::move(h->d_noise));
        h->d_noise = std::move(h->noise_ahead_block);
        h->dev.noise = h->d_noise;
        h->noise_rows_alloc = h->noise_ahead_alloc;
    }
    h->noise_rows_ready = h->noise_ahead_upto;
    h->noise_ahead = false;
    h->main_dirty = true;
    return F110_OK;
}

// ---- the whole step of a tiny batch as ONE launch (k_step_tiny) ----------------------------------------------------------
// When: a HOST-SYNCHRONISED step (f110_step_host that waits: F110Env.step, F110VecEnv.step) of at most kTinyMaxAgents = 4 agents, one or
// two per env — the reference's own shape — with the agent-aligned scan on one PADDED map, this step's noise row in the table / row cache
// (or no noise), nothing that brackets or counts inside the step.  Measured where it was tried beyond that (profiles/r06_tiny_ab.txt, one
// launch against three kernels): F110Env with 2 cars 73.5 -> 69.5 us per step, with 1 car 69.3 -> 58.4 us; but 16 agents 79 -> 99 us and 64
// agents 86 -> 197 us (the last workgroup finalizes every agent by itself), and a device-resident loop of one env 53.1 -> 56.4 us (nothing
// waits between its steps, so the longer single kernel is all it sees).  Everything else takes the per-kernel form.
static bool tiny_applies(const f110_sim *h)
{
    const int A = h->cfg.num_agents;
    if (h->tiny_off || h->N > kTinyMaxAgents || (A != 1 && A != 2)) return false;
    if (A == 2 && h->collide_mode != 3) return false;
    if (h->multi_map || !agent_aligned(h) || h->lookups_on || h->path_stats_on || h->profiling) return false;
    if (h->dev.noise_rng && (h->dev.noise_rng == 2 || h->noise_ub >= (long long)h->dev.noise_rows)) return false;   // k_noise_rows would have to run first
    if (kExperimental && (h->exp.scan_env_counter || h->exp.scan_trace || h->exp.scan_occupancy)) return false;
    if (!h->groups_auto && h->groups > 1) return false;   // step_groups = 2 forced: the caller asked for env blocks
    return true;
}

static int tiny_setup(f110_sim *h)
{
    if (h->tiny_mem) return F110_OK;
    const size_t N = (size_t)h->N;
    // one allocation: [done + pad | wall N | buf_cnt N] int32 then the double columns, then the headers
    const size_t ints = 16 + 2 * N, dbls = (7 + 2 + 3 + 3 + 1) * N;
    const size_t bytes = ((ints * 4 + 63) / 64) * 64 + dbls * 8 + N * sizeof(RayHdr);
    TRY(dmalloc(h, &h->tiny_mem, bytes));
    HIPCHK(h, hipMemsetAsync(h->tiny_mem, 0, bytes, h->stream));
    char *base = reinterpret_cast<char *>(h->tiny_mem.get());
    TinyCtl &t = h->tiny;
    t.done = reinterpret_cast<unsigned int *>(base);
    t.wall = reinterpret_cast<int32_t *>(base) + 16;
    t.buf_cnt = t.wall + N;
    double *d = reinterpret_cast<double *>(base + ((ints * 4 + 63) / 64) * 64);
    t.state = d;            d += 7 * N;
    t.steer_buf = d;        d += 2 * N;
    t.scan_pose = d;        d += 3 * N;
    t.snap_pose = d;        d += 3 * N;
    t.dir_start = d;        d += N;
    t.ray_hdr = reinterpret_cast<RayHdr *>(d);
    t.tasks_per_agent = ((uint32_t)h->k.num_beams + 63u) / 64u;
    return F110_OK;
}

// One picker per kernel family of the step, each above the stage that launches it.  A picker names every instantiation the
// library holds and no other (taking a kernel's address instantiates it) — and in the order the code object has always had
// them: the device code stays byte for byte what it was (profiles/step_stage_split_device_code.txt).

// k_step_tiny<PAIR, IDENT, HOST>: two cars per env / the map's rotation is the identity / the f110_step_host epilogue
static step_tiny_fn pick_step_tiny(bool pair, bool ident, bool host)
{
    if (pair) {
        if (host) return ident ? k_step_tiny<true, true, true> : k_step_tiny<true, false, true>;
        return ident ? k_step_tiny<true, true, false> : k_step_tiny<true, false, false>;
    }
    if (host) return ident ? k_step_tiny<false, true, true> : k_step_tiny<false, false, true>;
    return ident ? k_step_tiny<false, true, false> : k_step_tiny<false, false, false>;
}

static int step_tiny(f110_sim *h, hipStream_t st, const double *d_actions, const StepRequest &rq, bool &host_written)
{
    TRY(tiny_setup(h));
    const int N = h->N, A = h->cfg.num_agents;
    AgentArrays dev = h->dev;
    dev.agent_begin = 0;
    dev.agent_count = N;
    dev.sched_count_zero = nullptr;
    RayJob j{};
    TRY(ray_job_step_fields(h, j));
    h->tiny.tasks_per_agent = ((uint32_t)h->k.num_beams + 63u) / 64u;
    h->tiny.trace = kExperimental ? reinterpret_cast<unsigned long long *>(h->exp.tiny_trace) : nullptr;
    h->tiny.act_inline = 0;
    if (rq.tiny_actions && N <= kTinyMaxAgents) {   // f110_step_host: the caller's actions travel with the launch
        std::memcpy(h->tiny.act, rq.tiny_actions, sizeof(double) * 2 * (size_t)N);
        h->tiny.act_inline = 1;
    }
    h->tiny.start_word = nullptr;
    h->tiny.skip = kExperimental ? (h->exp.tiny_start_probe == 2 ? 1 : (h->exp.tiny_general_tail ? 2 : 0)) : 0;
    if (kExperimental && h->exp.tiny_start_probe && h->hb_seq_host && rq.seq) {
        void *p = nullptr;
        TRY(map_host_ptr(h, h->hb_seq_host, &p, "completion word"));
        h->tiny.start_word = reinterpret_cast<unsigned long long *>(p) + 1;
        h->tiny.start_seq = h->hb_seq;
    }
    const dim3 grid(((unsigned)N * h->tiny.tasks_per_agent + 3u) / 4u), block(256);
    // f110_step_host: host block + episode logic as the last workgroup's epilogue; two cars per env read them from d_fused,
    // one car per env (solo) gets them as kernel arguments
    const bool host = !dev.reseat_poses && (A == 2 ? rq.fuse : rq.hb != nullptr), solo = host && A != 2;
    host_written = host;
    if (host && A == 2) {
        dev.fused_host = h->d_fused;
        dev.fused_seq = rq.seq;
        h->tiny.fh = h->fused_host_copy;   // (what d_fused holds: f110_step_host keeps the two equal)
    }
    const EpisodeArrays ep = solo ? h->ep : EpisodeArrays{};
    const HostBlock hb = solo ? *rq.hb : HostBlock{};
    const int episode = solo ? rq.episode : 0, auto_reset = solo ? rq.auto_reset : 0;
    // one env of two cars: finalize_duo_tiny puts the scans into the caller's block early (its idle wave copies, the window lanes follow)
    h->tiny.host_scans = (host && h->hb_valid && h->hb_scans_by_kernel && A == 2 && N == 2 && !(kExperimental && h->exp.tiny_general_tail)) ? h->hb_dev.scans : nullptr;
    if (h->track_on) TRY(track_launch(h, st, kTrackHead, 0, N));
    hipLaunchKernelGGL(pick_step_tiny(A == 2, h->k.ident_rot != 0, host), grid, block, 0, st, dev, h->k, j, d_actions, h->tiny, ep, hb, episode, auto_reset);
    h->last_launches = 1;
    if (h->track_on) {   // (f110_step_host runs the host block as k_host_block behind this: no host epilogue while tracking)
        TRY(track_launch(h, st, kTrackPost, 0, N));
        h->last_launches += 2;
    }
    return F110_OK;
}

// ---- one step of an env-aligned block, stage by stage (step_range puts them in order) ----------------------------------------

// the scan kernel family of a step
enum ScanKind { SCAN_FLAT, SCAN_AGENT, SCAN_AGENT_SCHED, SCAN_DIRS };

static ScanKind pick_scan(const f110_sim *h, int begin, int count)
{
    const bool padded = padded_family(h->cfg.map_layout) && h->k.pad;
    if (h->dir_stride > 0) return padded ? SCAN_DIRS : SCAN_FLAT;   // (no PADDED table: every beam is marched)
    if (!(h->multi_map || agent_aligned(h))) return SCAN_FLAT;
    if (h->task_order && !h->multi_map && !h->lookups_on && begin == 0 && count == h->N && !h->exp.scan_env_counter) return SCAN_AGENT_SCHED;
    return SCAN_AGENT;
}

// where the pair tests (car against car) and the opponent windows of a step run
enum PairTests {
    PAIRS_NONE,               // one car per env
    PAIRS_IN_INTEGRATE,       // lab, collide_mode 1: fused into k_integrate<2|4>
    PAIRS_IN_FINALIZE_PAIR,   // A = 2: inside k_finalize_pair_roles / _wave
    PAIRS_IN_FINALIZE_MULTI,  // A = 3 .. kMaxAgentsMulti, whole envs: inside k_finalize_multi / _tiled
    PAIRS_COLLIDE_SIDE,       // k_collide on the side stream, under the scan
    PAIRS_COLLIDE_IN_LINE     // lab, collide_mode 2: k_collide on the step's stream
};

// A = 2 inside the finalize kernel: one stream, no events.  (Round 2 kept the side-stream form for big batches stepped without the
// in-step re-seat — crashed cars pile up, their windows grow to all beams, and fixed lanes per agent then serialise — the flattened
// window loop balances that inside the workgroup: 65 536 parked cars 0.624 -> 0.579 ms, crashed cars piling up 0.899 -> 0.852.)
static PairTests pair_tests_place(int A, int collide_mode, int begin, int count)
{
    if (A <= 1) return PAIRS_NONE;
    if (kExperimental && collide_mode == 1 && (A == 2 || A == 4)) return PAIRS_IN_INTEGRATE;
    if (collide_mode == 3 && A == 2 && begin % 2 == 0) return PAIRS_IN_FINALIZE_PAIR;
    if (collide_mode == 3 && A > 2 && A <= kMaxAgentsMulti && begin % A == 0 && count % A == 0) return PAIRS_IN_FINALIZE_MULTI;
    return (kExperimental && collide_mode == 2) ? PAIRS_COLLIDE_IN_LINE : PAIRS_COLLIDE_SIDE;
}

enum IntegrateForm { INTEGRATE_FAN, INTEGRATE_DUO, INTEGRATE_WAVE };

// Two waves per 64 agents (k_integrate_duo); RK4: thirteen (k_integrate_fan) up to kFanMaxAgents agents — the kernel is a latency
// chain there; big batches are throughput-bound and keep the two-wave form.  force_*: the lab's switches (-1 = this rule).
static IntegrateForm integrate_form(int integrator, int count, int force_duo, int force_fan)
{
    const bool rk4 = integrator == F110_INTEGRATOR_RK4;
    if (force_fan >= 0 ? (force_fan != 0 && rk4) : (rk4 && count <= kFanMaxAgents)) return INTEGRATE_FAN;
    return force_duo == 0 ? INTEGRATE_WAVE : INTEGRATE_DUO;   // (k_integrate<0>, one wave per 64 agents: lab only)
}

// Lanes per agent in the finalize kernel.  With the pair test inside (A = 2): more agents per workgroup = fewer prologue waves and a
// better-balanced item list; small batches want the workgroups many (measured: 65 536 agents AG 32 / 16 / 4: 0.726 / 0.738 / 0.815 ms;
// 4096 agents AG 16 / 4: 0.1047 / 0.1053).  (Rounds 2-3's forms — fixed lanes per agent, the prologue dealt by agent — were retired in
// round 5.)  Behind k_collide: few lanes per agent pay off when opponent windows are short (~36 beams); cars that have crashed into
// each other see windows of up to all beams, so the narrow forms are used only when finished envs are re-seated inside the step
// (narrow: f110_set_auto_reseat armed).
static int finalize_lanes(bool narrow, int N, bool pair)
{
    if (pair) return N >= 32768 ? 8 : (N >= 4096 ? 16 : 64);
    return narrow && N >= 131072 ? 8 : (narrow && N >= 32768 ? 16 : 64);
}

// k_finalize_pair_wave in a step of two env blocks: from 24 576 agents in the automatic mode, where the other block's scan fills the
// GPU and the 256-thread form waits for its tail (two blocks, 256-thread / one-wave form, lab build, ms per step: 8192 agents 0.1235 /
// 0.1333, 16 384: 0.1964 / 0.1987, 24 576: 0.2754 / 0.2747, 32 768: 0.3637 / 0.3586, 49 152: 0.5278 / 0.5218, 65 536: 0.6799 / 0.6515 —
// profiles/two_block_pair_sweep.txt).  step_groups = 2, two blocks on request, takes it at every size: that keeps the form reachable
// for small batches in the product build, where the tests hold it against the one-block step bit for bit.
// One-wave workgroups fit the slots the OTHER block's scan frees wave by wave (a 256-thread workgroup waits for that scan's tail).
// Alone it is the slower form — one block at 65 536 agents 0.6933 -> 0.7032 ms with the lab switch pair_wave = 1 — so one block keeps
// the 256-thread form.  Priced in the bench's regime, re-seats armed; with re-seats off crashed pairs stay and their windows grow
// towards all B beams: there it still led, 1.159 -> 1.097 ms (same file).
static bool pair_wave_pays(bool env_blocks, bool groups_auto, int N)
{
    return env_blocks && (!groups_auto || N >= 24576);
}

static int step_noise_rows(f110_sim *h, hipStream_t st, const AgentArrays &dev, int count)
{
    if (dev.noise_rng && (dev.noise_rng == 2 || h->noise_ub >= (long long)dev.noise_rows)) {
        const int apb = dev.noise_rng == 2 ? 16 : 64;   // per-agent streams: every agent needs a row, keep the waves many
        hipLaunchKernelGGL(k_noise_rows, dim3((count + apb - 1) / apb), dim3(256), 0, st, dev, h->noise_gen, h->k.num_beams, apb);
    }
    return F110_OK;
}

static int step_integrate(f110_sim *h, hipStream_t st, const AgentArrays &dev, int count, const double *d_actions, PairTests pairs)
{
#ifdef F110_EXPERIMENTAL
    if (pairs == PAIRS_IN_INTEGRATE) {
        if (h->cfg.num_agents == 2) hipLaunchKernelGGL(k_integrate<2>, grid1d(count, 64), dim3(64), 0, st, dev, h->k, d_actions);
        else hipLaunchKernelGGL(k_integrate<4>, grid1d(count, 64), dim3(64), 0, st, dev, h->k, d_actions);
        return F110_OK;
    }
#endif
    (void)pairs;
    switch (integrate_form(h->dev.integrator, count, kExperimental ? h->exp.integrate_duo : -1, kExperimental ? h->exp.integrate_fan : -1)) {
    case INTEGRATE_FAN: hipLaunchKernelGGL(k_integrate_fan, grid1d(count, 64), dim3(64 * kFanWaves), 0, st, dev, h->k, d_actions); break;
    case INTEGRATE_DUO: hipLaunchKernelGGL(k_integrate_duo, grid1d(count, 64), dim3(128), 0, st, dev, h->k, d_actions); break;
    case INTEGRATE_WAVE:
#ifdef F110_EXPERIMENTAL
        hipLaunchKernelGGL(k_integrate<0>, grid1d(count, 256), dim3(256), 0, st, dev, h->k, d_actions);
#endif
        break;
    }
    return F110_OK;
}

// k_collide only feeds k_finalize, the scan only needs k_integrate: run the two side by side (second stream, event fork here,
// join in step_range behind the scan) so the pair test + window set-up hides under the scan
static int step_collide(f110_sim *h, hipStream_t st, const AgentArrays &dev, int count, PairTests pairs)
{
    if (pairs == PAIRS_COLLIDE_SIDE) {
        HIPCHK(h, hipEventRecord(h->ev_integrated, st));
        HIPCHK(h, hipStreamWaitEvent(h->side_stream, h->ev_integrated, 0));
        hipLaunchKernelGGL(k_collide, grid1d(count, 64), dim3(64), 0, h->side_stream, dev, h->k.num_beams);
        HIPCHK(h, hipEventRecord(h->ev_collided, h->side_stream));
    } else if (pairs == PAIRS_COLLIDE_IN_LINE) {
        hipLaunchKernelGGL(k_collide, grid1d(count, 64), dim3(64), 0, st, dev, h->k.num_beams);
    }
    return F110_OK;
}

// k_scan_dirs_agent<PER_ENV_MAP, IDENT, COUNT> (per-env maps carry their own rotation: IDENT never applies)
static scan_agent_fn pick_dirs_agent(bool per_env_map, bool ident, bool count)
{
    if (per_env_map) return count ? k_scan_dirs_agent<true, false, true> : k_scan_dirs_agent<true, false, false>;
    if (ident) return count ? k_scan_dirs_agent<false, true, true> : k_scan_dirs_agent<false, true, false>;
    return count ? k_scan_dirs_agent<false, false, true> : k_scan_dirs_agent<false, false, false>;
}

// Which k_scan_rays_agent<PER_ENV_MAP, IDENT, COUNT, SCHED, ENVCNT, ENV_ORDER> a launch takes; a combination the library does not
// hold gets nullptr.
struct ScanAgentForm {
    bool per_env_map = false;     // every env marches its own map (its own rotation: IDENT never applies)
    bool ident = false;           // the one map's rotation is the identity
    bool count = false;           // table lookups are counted (f110_count_lookups)
    bool longest_first = false;   // SCAN_AGENT_SCHED (pick_scan: never with a count or per-env maps)
    bool env_order = false;       // an env's agents sector by sector (never with per-env maps: the kernel's static_assert)
    bool env_counter = false;     // lab: finished tasks counted per env (alone: no count, no order)
};

static scan_agent_fn pick_rays_agent(const ScanAgentForm &f)
{
    if (f.longest_first) {
        if (f.count || f.per_env_map || f.env_counter) return nullptr;
        if (f.env_order) return f.ident ? k_scan_rays_agent<false, true, false, true, false, true> : k_scan_rays_agent<false, false, false, true, false, true>;
        return f.ident ? k_scan_rays_agent<false, true, false, true> : k_scan_rays_agent<false, false, false, true>;
    }
    if (f.env_counter) {
#ifdef F110_EXPERIMENTAL
        if (!f.count && !f.per_env_map) return f.ident ? k_scan_rays_agent<false, true, false, false, true> : k_scan_rays_agent<false, false, false, false, true>;
#endif
        return nullptr;
    }
    if (f.per_env_map) {
        if (f.env_order) return nullptr;
        return f.count ? k_scan_rays_agent<true, false, true> : k_scan_rays_agent<true, false, false>;
    }
    if (f.env_order) {
        if (f.ident) return f.count ? k_scan_rays_agent<false, true, true, false, false, true> : k_scan_rays_agent<false, true, false, false, false, true>;
        return f.count ? k_scan_rays_agent<false, false, true, false, false, true> : k_scan_rays_agent<false, false, false, false, false, true>;
    }
    if (f.ident) return f.count ? k_scan_rays_agent<false, true, true> : k_scan_rays_agent<false, true, false>;
    return f.count ? k_scan_rays_agent<false, false, true> : k_scan_rays_agent<false, false, false>;
}

// Agent-aligned launch geometry: whole 64-ray tasks per agent (tpa of them), so every wave belongs to one agent (and one map).
// Fills the job's task fields and returns the grid.
static dim3 scan_agent_grid(const f110_sim *h, RayJob &j, int begin, int count, uint32_t tpa, int tasks_per_wave, bool env_order)
{
    const int A = h->cfg.num_agents;
    (void)rays_grid(j, h->scan_block, tasks_per_wave);   // (for j.tasks_per_wave; the task count is the block's)
    j.n_tasks = (uint32_t)count * tpa;
    j.first_pose = (uint32_t)begin;
    // k_scan_rays_agent<.., ENV_ORDER> walks an env's agents sector by sector (scan_task_agent): the launch must cover whole envs
    j.agents_per_env = (env_order && A > 1 && begin % A == 0 && count % A == 0 && scan_task_inv_ok(tpa, (uint32_t)A)) ? (uint32_t)A : 1u;
    j.agents_inv = scan_task_inv(j.agents_per_env);
    const uint32_t wpb = (uint32_t)h->scan_block / 64u;
    const uint32_t waves = (j.n_tasks + j.tasks_per_wave - 1) / j.tasks_per_wave;
    return dim3((waves + wpb - 1) / wpb);
}

static int step_scan(f110_sim *h, hipStream_t st, int begin, int count, ScanKind scan)
{
    const int N = h->N, B = h->k.num_beams;
    RayJob j{};
    j.n_rays = (uint32_t)N * (uint32_t)B;
    j.n_poses = N;
    j.pose_x = h->dev.scan_pose;
    j.pose_y = h->dev.scan_pose + N;
    j.dir_start = h->dev.dir_start;
    j.ranges = h->dev.scans;
    j.hdr = h->dev.ray_hdr;
    j.wall_flag = h->dev.in_collision;
    j.div_magic = h->step_magic;
    j.div_shift = h->step_shift;
    j.lookups_total = h->lookups_on ? h->d_lookups : nullptr;
    j.path_stats = h->path_stats_on ? h->d_path_stats : nullptr;   // (step form: only the ray pass counts here)
#ifdef F110_EXPERIMENTAL
    j.trace = reinterpret_cast<unsigned long long *>(h->exp.scan_trace);
#endif
    TRY(ray_job_step_fields(h, j));
    j.order = (h->multi_map && begin == 0 && count == N) ? h->d_scan_order : nullptr;
    const dim3 block(h->scan_block);
    if (scan == SCAN_FLAT) {   // ray = agent * B + beam (row-major table, few beams, or — product build — beams beyond the table
                               // directions on a map the PADDED layout cannot hold)
        const dim3 fgrid = rays_grid(j, h->scan_block, h->scan_tasks_per_wave);
        hipLaunchKernelGGL(pick_rays<true>(h->k, h->cfg.map_layout), fgrid, block, 0, st, j, h->k);
        return F110_OK;
    }
    const bool count_lookups = j.lookups_total != nullptr, ident = h->k.ident_rot != 0;
    scan_agent_fn fn = nullptr;
    dim3 grid;
    uint32_t tpa = 0;
    size_t lds = 0;
    if (scan == SCAN_DIRS) {
        // more beams than table directions, PADDED table: march each distinct direction once and write
        // the beams that share it from the same wave (k_scan_dirs_agent)
        tpa = (uint32_t)h->dir_stride / 64u;
        // (a direction task ends with ~3 coalesced write passes: four per wave, where the beam kernel wants three —
        // BASELINE configs[4] 42.8 M agent-steps/s at 3, 45.2 M at 4)
        grid = scan_agent_grid(h, j, begin, count, tpa, h->scan_tasks_auto && h->scan_tasks_per_wave == 3 ? 4 : h->scan_tasks_per_wave, false);
        fn = pick_dirs_agent(h->multi_map, ident, count_lookups);
    } else {   // SCAN_AGENT, SCAN_AGENT_SCHED
        const bool env_order = h->scan_env_order && !h->multi_map;
        tpa = ((uint32_t)B + 63u) / 64u;
        grid = scan_agent_grid(h, j, begin, count, tpa, env_order ? h->scan_tasks_agent : h->scan_tasks_per_wave, env_order);
        ScanAgentForm f;
        f.per_env_map = h->multi_map;
        f.ident = ident;
        f.count = count_lookups;
        f.longest_first = scan == SCAN_AGENT_SCHED;
        f.env_order = j.agents_per_env > 1;
        if (f.longest_first) {   // last step's long tasks are served by the first blocks of the launch
            const uint32_t wpb = (uint32_t)h->scan_block / 64u;
            j.sched = h->tsched[h->task_epoch & 1u];
            j.epoch_r = h->task_epoch - 1u;
            j.epoch_w = h->task_epoch;
            j.long_blocks = (h->task_cap + wpb - 1) / wpb;
            j.long_prio = (uint32_t)h->exp.long_prio;
            j.long_rev = h->task_rev;
            h->task_epoch += 1u;
            grid = dim3(grid.x + j.long_blocks);
        }
#ifdef F110_EXPERIMENTAL
        // probes.  Fewer waves per SIMD (an LDS reservation per one-wave workgroup): the occupancy a kernel with the pair
        // finalize's 118 VGPRs would run at (fusion feasibility), and whether last step's long tasks, which start
        // first, march at the idle chip's latency — does the shorter chain beat the lost throughput?
        if (h->exp.scan_occupancy > 0 && h->scan_block == 64) lds = (size_t)(160 * 1024 / (4 * h->exp.scan_occupancy)) & ~(size_t)255;
        // ... and the price of a per-env completion counter (its kernel has neither the lookup count nor the env order)
        if (scan == SCAN_AGENT && h->exp.scan_env_counter && !h->multi_map && !count_lookups) {
            if (!h->d_env_done) {
                TRY(dmalloc(h, &h->d_env_done, (size_t)h->cfg.num_envs));
                HIPCHK(h, hipMemsetAsync(h->d_env_done, 0, sizeof(uint32_t) * h->cfg.num_envs, st));
            }
            j.env_done = h->d_env_done;
            j.tasks_per_env = tpa * (uint32_t)h->cfg.num_agents;
            f.env_counter = true;
            f.env_order = false;
        }
#endif
        fn = pick_rays_agent(f);
    }
    if (!fn) return fail(h, F110_ERR_STATE, "f110_step_device: no scan kernel for this combination of switches");
    hipLaunchKernelGGL(fn, grid, block, lds, st, j, h->k, h->d_maps_fast, h->d_maps_full, tpa);
    return F110_OK;
}

// A finalize kernel and how many agents one of its workgroups takes (the grid follows)
struct FinalizeKernel { finalize_fn fn; int agents, threads; };

// A = 2, the pair test inside the kernel.  k_finalize_pair_roles<AG, HOST>: the window loop flattened over the workgroup, AG agents
// per 256 threads (lanes per agent = 256 / AG), the prologue dealt by role; HOST carries the f110_step_host epilogue and goes first.
// k_finalize_pair_wave: one-wave workgroups (when: pair_wave_pays).
static FinalizeKernel pick_finalize_pair(int lanes, bool host, bool wave)
{
    if (host) {
        if (lanes <= 8) return {k_finalize_pair_roles<32, true>, 32, 256};
        if (lanes == 16) return {k_finalize_pair_roles<16, true>, 16, 256};
        return {k_finalize_pair_roles<4, true>, 4, 256};
    }
    if (wave) return {k_finalize_pair_wave<kFinalizeWaveAgents>, kFinalizeWaveAgents, 64};
    if (lanes <= 8) return {k_finalize_pair_roles<32>, 32, 256};
    if (lanes == 16) return {k_finalize_pair_roles<16>, 16, 256};
    return {k_finalize_pair_roles<4>, 4, 256};
}

// A = 3 .. kMaxAgentsMulti, every ordered pair of an env inside the kernel: whole envs per 256-thread workgroup
struct FinalizeMultiKernel { finalize_multi_fn fn; int envs; size_t lds; };

static FinalizeMultiKernel pick_finalize_multi(int A)
{
    const int pairs = A * (A - 1);
    if (pairs <= kMaxRec) return {k_finalize_multi<kMaxRec>, kMaxRec / pairs, 0};
    if (pairs <= kMaxRecBig) return {k_finalize_multi<kMaxRecBig>, 1, 0};
    return {k_finalize_multi_tiled<kMaxRecBig>, 1, multi_lds_bytes(A, kMaxRecBig)};   // more than 16 agents: the env's records in tiles of 256
}

// the pair tests done before it (k_collide, or the lab's fused integration): k_finalize<lanes per agent>
static FinalizeKernel pick_finalize(int lanes)
{
    if (lanes == 8) return {k_finalize<8>, 32, 256};
    if (lanes == 16) return {k_finalize<16>, 16, 256};
    return {k_finalize<64>, 4, 256};
}

static int step_finalize(f110_sim *h, hipStream_t st, AgentArrays &dev, int begin, int count, PairTests pairs, const StepRequest &rq, bool &host_written)
{
    const int N = h->N, A = h->cfg.num_agents, B = h->k.num_beams;
    const bool narrow = h->dev.reseat_poses != nullptr;
    switch (pairs) {
    case PAIRS_NONE:
        hipLaunchKernelGGL(k_finalize_solo, grid1d(count, 256), dim3(256), 0, st, dev);
        break;
    case PAIRS_IN_FINALIZE_PAIR: {
        bool pair_wave = pair_wave_pays(rq.env_blocks, h->groups_auto, N);
#ifdef F110_EXPERIMENTAL
        if (h->exp.pair_wave >= 0) pair_wave = h->exp.pair_wave != 0;
#endif
        if (rq.fuse && begin == 0 && count == N && !dev.reseat_poses) {   // f110_step_host: host block + episode logic as this kernel's epilogue
            dev.fused_host = h->d_fused;
            dev.fused_seq = rq.seq;
            host_written = true;
        }
        const FinalizeKernel k = pick_finalize_pair(finalize_lanes(narrow, N, true), dev.fused_host != nullptr, pair_wave);
        hipLaunchKernelGGL(k.fn, grid1d(count, k.agents), dim3(k.threads), 0, st, dev, B);
        break;
    }
    case PAIRS_IN_FINALIZE_MULTI: {
        const FinalizeMultiKernel k = pick_finalize_multi(A);
        hipLaunchKernelGGL(k.fn, grid1d(count / A, k.envs), dim3(256), k.lds, st, dev, B, k.envs);
        break;
    }
    default: {   // the pair tests are done (k_collide, or the lab's fused integration)
        const FinalizeKernel k = pick_finalize(finalize_lanes(narrow, N, false));
        hipLaunchKernelGGL(k.fn, grid1d(count, k.agents), dim3(k.threads), 0, st, dev, B);
        break;
    }
    }
    return F110_OK;
}

// One step of the agents [begin, begin + count) (an env-aligned block) on stream `st`: the stages above, in order.
// Product build, by agents per env (pair_tests_place):
//   A = 1          k_integrate_duo|fan -> scan -> k_finalize_solo
//   A = 2          k_integrate_duo|fan -> scan -> k_finalize_pair_roles<32|16|4>   (pair test + window inside the last kernel; <.., HOST>
//                                                                                  carries f110_step_host's block as its epilogue)
//                                        ... -> k_finalize_pair_wave   in a step of two env blocks (pair_wave_pays): one-wave
//                                                                      workgroups, which fit under the other block's scan
//   A = 3 .. 16    k_integrate_duo|fan -> scan -> k_finalize_multi         (the same for every ordered pair of an env)
//   A = 17 .. 256  k_integrate_duo|fan -> scan -> k_finalize_multi_tiled   (the env's ordered pairs in tiles of 256 records)
//   A > 256        k_integrate_duo|fan -> { scan || k_collide on the side stream } -> join -> k_finalize<64|16|8>
// (a block that does not cover whole envs of A = 3 .. 256 takes the last row), k_noise_rows in front when the step's noise rows are
// not in the table / row cache, the two track passes around it all when tracking is on; and the scan by table / beam count (pick_scan):
//   SCAN_AGENT        k_scan_rays_agent: PADDED table, every wave one agent's; in env order (an env's agents sector by sector)
//                     where f110_create measured it to pay; per-env maps
//   SCAN_AGENT_SCHED  ... last step's longest tasks first: the whole batch on one map, task order on (small batches)
//   SCAN_DIRS         k_scan_dirs_agent: more beams than table directions, each distinct direction marched once
//   SCAN_FLAT         k_scan_rays (pick_rays): row-major table, few beams, or beams beyond the directions without a PADDED table
// A tiny host-synchronised batch does not come here at all: step_tiny, one launch.
// The experimental build adds collide_mode 1 (pair tests fused into k_integrate<2|4>) / 2 (k_collide in line), k_integrate<0>,
// the scan's env counter and occupancy probes and the forced choices of f110_exp_set.
// ev[0..3] (or nullptr): profiling events before integrate / before scan / after scan / after finalize.
static int step_range(f110_sim *h, hipStream_t st, int begin, int count, const double *d_actions, int collide_mode, hipEvent_t *ev, const StepRequest &rq,
                      bool &host_written)
{
    AgentArrays dev = h->dev;
    dev.agent_begin = begin;
    dev.agent_count = count;
    // the scan kernel of this step, decided ONCE: the scan stage and what k_integrate prepares for it
    // (the longest-first list counter, of the parity the scan stage then moves on) follow the same answer
    const ScanKind scan = pick_scan(h, begin, count);
    const PairTests pairs = pair_tests_place(h->cfg.num_agents, collide_mode, begin, count);
    if (h->track_on) TRY(track_launch(h, st, kTrackHead, begin, count));   // s of the pose this step starts from (cache misses only)
    dev.sched_count_zero = scan == SCAN_AGENT_SCHED ? h->d_tcount + (h->task_epoch & 1u) : nullptr;
    TRY(step_noise_rows(h, st, dev, count));
    if (ev) HIPCHK(h, hipEventRecord(ev[0], st));
    TRY(step_integrate(h, st, dev, count, d_actions, pairs));
    TRY(step_collide(h, st, dev, count, pairs));
    if (ev) HIPCHK(h, hipEventRecord(ev[1], st));
    TRY(step_scan(h, st, begin, count, scan));
    if (ev) HIPCHK(h, hipEventRecord(ev[2], st));
    if (pairs == PAIRS_COLLIDE_SIDE) HIPCHK(h, hipStreamWaitEvent(st, h->ev_collided, 0));
    TRY(step_finalize(h, st, dev, begin, count, pairs, rq, host_written));
    if (ev) HIPCHK(h, hipEventRecord(ev[3], st));
    // the track columns of the observation: from snap_pose, the post-step pose no re-seat overwrites (k_host_block runs behind)
    if (h->track_on) TRY(track_launch(h, st, kTrackPost, begin, count));
    return F110_OK;
}

// step_groups = 0: do two env blocks pay for N agents, A per env?  bench.py's steady-regime workload, one block -> two blocks
// (profiles/r04_groups_bench_sweep.txt, ms per step):  A = 2:  1024 +2.8 %, 2048 +0.6 %, 3072 -1.6 %, 4096 -1.3 %, 6144 +1.7 %,
// 8192 +5.8 %, 16 384 +9.5 %, 32 768 +3.7 %, 65 536 +1.7 %;  A = 1 / 4 / 8 at 16 384: +7.2 / +6.9 / +10.3 %, at 65 536: +5.7 / +4.1 / +4.4 %,
// at 4096: -0.9 / -0.1 / +3.8 %.  Around 3000 .. 5000 agents the step IS its longest ray's chain of dependent samples: two
// blocks have two such chains side by side and nothing to hide under them (a heavier finalize, A >= 8, changes that).
// A = 2 above 32 768 agents stayed one block until the two-car finalize got its one-wave form (k_finalize_pair_wave, step_range),
// which the second block runs under the first block's scan.  With it, one block -> the automatic mode's two blocks, A = 2
// (profiles/two_block_pair_sweep.txt): see the table there; 65 536 agents 0.6851 -> 0.6414 ms (two_block_pair_bench.txt).
static bool env_blocks_pay(int N, int A)
{
    if (A <= 4 && N >= 2560 && N <= 5120) return false;
    return true;
}

int f110_step_groups(f110_sim *h, int32_t *groups, int32_t *probes, int32_t *last)
{
    if (!h) return fail(h, F110_ERR_INVALID, "null argument");
    if (groups) *groups = h->groups;
    if (probes) *probes = h->group_probes;
    if (last) *last = h->last_blocks;
    return F110_OK;
}

int f110_step_launches(f110_sim *h, int32_t *launches)
{
    if (!h || !launches) return fail(h, F110_ERR_INVALID, "null argument");
    *launches = h->last_launches;
    return F110_OK;
}

static int step_submit(f110_sim *h, const double *d_actions, const StepRequest &rq, bool &host_written)
{
    host_written = false;
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (h->track_on || h->rs.on) TRY(track_prepare(h));
    const int N = h->N, A = h->cfg.num_agents;
    h->dev.path_stats = h->path_stats_on ? h->d_path_stats : nullptr;
    if (h->comm_overlap && h->comm_swap_next) {
        // the previous step's scans are being gathered: this step fills the other buffer, once the
        // gather that last read THAT buffer (two steps ago) is done
        h->scans_cur ^= 1;
        h->dev.scans = h->scan_bufs[h->scans_cur];
        if (h->gather_pending[h->scans_cur]) {
            const bool inflight = h->comm_inflight;
            h->comm_inflight = false;
            const int rj = join_groups(h);
            h->comm_inflight = inflight;
            if (rj != F110_OK) return rj;
            HIPCHK(h, hipStreamWaitEvent(h->stream, h->ev_gather_done[h->scans_cur], 0));
            h->gather_pending[h->scans_cur] = false;
            h->main_dirty = true;
        }
        h->comm_swap_next = false;
    }
    // shared noise stream: the row cache must reach the longest live episode (or its capacity)
    if (h->dev.noise_rng == 1 && h->noise_rows_ready < h->dev.noise_rows) {
        if (h->noise_ub >= h->noise_rows_ready) {
            TRY(join_groups(h));
            TRY(noise_adopt(h));   // the rows generated ahead
            if (h->noise_ub >= h->noise_rows_ready && h->noise_rows_ready < h->dev.noise_rows) {   // (not enough: in line, this step waits)
                const long long want = std::max<long long>(2LL * h->noise_rows_ready, h->noise_ub + 1);
                TRY(noise_cache_extend(h, (int)std::min<long long>(want, h->dev.noise_rows)));
            }
        }
        if (!h->noise_ahead && 2 * (h->noise_ub + 1) >= h->noise_rows_ready) TRY(noise_start_ahead(h));
    }
    const bool prof = h->profiling && h->prof_used + 4 <= 4 * 65536;
    // the env groups need the agent-aligned scan (a launch per agent range); per-kernel profiling
    // brackets the kernels of ONE stream, so a profiled step runs as one block on the main stream
    // (two groups borrow the side stream, which the older collide forms use themselves)
    // a tiny batch (the reference's own shape: one env of two cars) is ONE launch: integrate, scan, finalize and — under
    // f110_step_host — the observation block and the completion word, in k_step_tiny
    const bool tiny = rq.tiny && !prof;   // (f110_step_host decided: tiny_applies)
    const bool grouped = !tiny && h->groups > 1 && !prof && (h->multi_map || agent_aligned(h)) && h->dir_stride == 0 &&
                         !(h->gstreams[0] == h->stream && h->collide_mode != 3 && A > 1) &&
                         (!h->groups_auto || (!h->touched && env_blocks_pay(N, A)));
    h->last_launches = 0;
    const EnvBlocks w = grouped ? env_blocks_submit(h) : env_blocks_main(h);
    if (!grouped) {
        TRY(join_groups(h));
        h->main_dirty = true;
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        if (prof) {
            for (int i = 0; i < 4; ++i)
                if (!(ev[i] = prof_event(h))) return fail(h, F110_ERR_HIP, "hipEventCreate failed");
        }
        if (tiny) TRY(step_tiny(h, h->stream, d_actions, rq, host_written));
        else TRY(step_range(h, h->stream, 0, N, d_actions, h->collide_mode, prof ? ev : nullptr, rq, host_written));
    } else {
        if (h->main_dirty) {
            HIPCHK(h, hipEventRecord(h->ev_main, h->stream));
            for (hipStream_t gs : h->gstreams)
                if (gs != h->stream) HIPCHK(h, hipStreamWaitEvent(gs, h->ev_main, 0));
            h->main_dirty = false;
        }
        const int mode = h->collide_mode == 3 ? 3 : ((A == 2 || A == 4) ? 1 : 2);
        StepRequest rb = rq;
        rb.env_blocks = true;
        for (const EnvBlock &b : w) TRY(step_range(h, b.stream, b.e0 * A, b.count * A, d_actions, mode, nullptr, rb, host_written));
        h->groups_busy = true;
    }
    // an in-step re-seat armed (f110_set_auto_reseat): the draw for the envs it re-seated, behind the step (per env block);
    // f110_step_host / f110_episode_step* launch it after their own last kernel instead (rq.defer_draw)
    if (reseat_draws(h) && h->dev.reseat_poses && !rq.defer_draw) TRY(sampler_after_step(h, w));
    h->touched = false;
    h->last_blocks = grouped ? h->groups : 1;
    h->noise_ub += 1;
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

int f110_step_device(f110_sim *h, const double *d_actions)
{
    TRY(check_step(h, d_actions != nullptr));
    bool host_written = false;
    return step_submit(h, d_actions, StepRequest{}, host_written);
}

int f110_stream_fence(f110_sim *h)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);   // joins the env blocks into the main stream; main_dirty + touched: the next step is one block behind the caller's work
    return F110_OK;
}

int f110_step(f110_sim *h, const double *actions)
{
    TRY(check_step(h, actions != nullptr));
    ENTER(h);   // the previous step (possibly still running on the group streams) reads d_actions
    HIPCHK(h, hipMemcpyAsync(h->d_actions, actions, sizeof(double) * 2 * h->N, hipMemcpyHostToDevice, h->stream));
    TRY(f110_step_device(h, h->d_actions));
    HIPCHK(h, hipStreamSynchronize(h->stream));  // pageable host buffer: consumed on return
    return F110_OK;
}

// ---- read-back ---------------------------------------------------------------------------
static int copy_col(f110_sim *h, double *dst, const double *src, size_t n)
{
    if (dst) HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    return F110_OK;
}

int f110_get_obs(f110_sim *h, const f110_obs_host *o)
{
    if (!h || !o) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    const size_t N = (size_t)h->N;
    const AgentArrays &d = h->dev;
    TRY(copy_col(h, o->scans, d.scans, N * h->cfg.num_beams));
    TRY(copy_col(h, o->poses_x, d.state, N));
    TRY(copy_col(h, o->poses_y, d.state + N, N));
    TRY(copy_col(h, o->poses_theta, d.state + 4 * N, N));
    TRY(copy_col(h, o->linear_vels_x, d.state + 3 * N, N));
    TRY(copy_col(h, o->ang_vels_z, d.state + 5 * N, N));
    TRY(copy_col(h, o->collisions, d.collisions, N));
    TRY(copy_col(h, o->collision_idx, d.collision_idx, N));
    std::vector<double> soa, poses;
    if (o->state) {
        soa.resize(7 * N);
        HIPCHK(h, hipMemcpyAsync(soa.data(), d.state, 7 * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if (o->agent_poses) {
        poses.resize(3 * N);
        HIPCHK(h, hipMemcpyAsync(poses.data(), d.snap_pose, 3 * N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    }
    if (o->in_collision) HIPCHK(h, hipMemcpyAsync(o->in_collision, d.in_collision, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (o->step_count) HIPCHK(h, hipMemcpyAsync(o->step_count, d.step_count, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (o->state)
        for (size_t i = 0; i < N; ++i)
            for (int c = 0; c < 7; ++c) o->state[7 * i + c] = soa[(size_t)c * N + i];
    if (o->agent_poses)
        for (size_t i = 0; i < N; ++i)
            for (int c = 0; c < 3; ++c) o->agent_poses[3 * i + c] = poses[(size_t)c * N + i];
    return F110_OK;
}

int f110_set_state(f110_sim *h, const double *state7, const double *steer_buf, const int32_t *buf_count)
{
    if (!h || !state7) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    const size_t N = (size_t)h->N;
    std::vector<double> soa(7 * N);
    for (size_t i = 0; i < N; ++i)
        for (int c = 0; c < 7; ++c) soa[(size_t)c * N + i] = state7[7 * i + c];
    HIPCHK(h, hipMemcpyAsync(h->dev.state, soa.data(), 7 * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    std::vector<double> sb;
    if (steer_buf) {
        sb.resize(2 * N);
        for (size_t i = 0; i < N; ++i) {
            sb[i] = steer_buf[2 * i];
            sb[N + i] = steer_buf[2 * i + 1];
        }
        HIPCHK(h, hipMemcpyAsync(h->dev.steer_buf, sb.data(), 2 * N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    if (buf_count) HIPCHK(h, hipMemcpyAsync(h->dev.buf_cnt, buf_count, N * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

// ---- exact snapshot / restore / clone (include/f110.h f110_state_*) ------------------------------------------------------
// The columns a blob carries are the ones active on the handle: the per-agent core always, device-noise positions / seeds,
// the episode arrays, per-agent params and the env-map slot while those exist.  Everything else a step reads (scan_pose,
// dir_start, ray_hdr, opp_window, opp_verts, the tiny step's shadow columns, the iTTC flags) is rewritten by every step form
// before it is read, so it is not state.
static uint32_t state_col_set(const f110_sim *h)
{
    uint32_t c = F110_STATE_COL_AGENT;
    if (h->dev.noise_rng) c |= F110_STATE_COL_RNG;
    if (h->dev.noise_rng == 2) c |= F110_STATE_COL_RNG_SEED;
    if (h->has_episode) c |= F110_STATE_COL_EPISODE;
    if (h->dev.params_per_agent) c |= F110_STATE_COL_PARAMS;
    if (h->multi_map) c |= F110_STATE_COL_ENV_MAP;
    if (h->rs.on) c |= F110_STATE_COL_RESET_RNG;
    if (h->ps.on) c |= F110_STATE_COL_PARAM_RNG;
    return c;
}

// the column table of a blob of k envs with column set `cols` (fixed order: the layout depends on cols, k, A and B only);
// returns the blob's total bytes
// the most columns state_columns adds: the agent core 17, noise 2, episode 9, params 1, env map 1, reset sampler 2, parameter sampler 1, scans 1
constexpr int kStateColsUsed = 17 + 2 + 9 + 1 + 1 + 2 + 1 + 1;
static_assert(kStateColsUsed <= kStateMaxCols, "StateCols::c cannot hold every column state_columns may add");

static size_t state_columns(const f110_sim *h, uint32_t cols, int k, StateCols *out)
{
    StateCols t{};
    const size_t N = (size_t)h->N;
    const uint32_t A = (uint32_t)h->cfg.num_agents, B = (uint32_t)h->cfg.num_beams;
    size_t off = F110_STATE_HEADER_BYTES;
    bool overflow = false;
    auto add = [&](void *live, uint32_t bytes, uint32_t per_env, uint32_t kind = 0) {
        if (t.n >= kStateMaxCols) {   // (kStateColsUsed rules this out; never index past the table)
            overflow = true;
            return;
        }
        StateCol &c = t.c[t.n++];
        c.live = static_cast<char *>(live);
        c.bytes = bytes;
        c.per_env = per_env;
        c.kind = kind;
        c.off = off;
        off += (((size_t)k * per_env * bytes) + 255) / 256 * 256;
    };
    for (int r = 0; r < 7; ++r) add(h->dev.state + r * N, 8, A);
    for (int r = 0; r < 2; ++r) add(h->dev.steer_buf + r * N, 8, A);
    add(h->dev.buf_cnt, 4, A);
    for (int r = 0; r < 3; ++r) add(h->dev.snap_pose + r * N, 8, A);
    add(h->dev.collisions, 8, A);
    add(h->dev.collision_idx, 8, A);
    add(h->dev.in_collision, 4, A);
    add(h->dev.step_count, 4, A);
    if (cols & F110_STATE_COL_RNG) add(h->d_rng_state, sizeof(U128), A, h->dev.noise_rng == 1 ? kStateColRngShared : 0);
    if (cols & F110_STATE_COL_RNG_SEED) add(h->d_rng_seed, 2 * sizeof(U128), A);
    if (cols & F110_STATE_COL_EPISODE) {
        const EpisodeArrays &ep = h->ep;
        add(ep.start_poses, 24, A);
        add(ep.near_start, 1, A);
        add(ep.toggle, 8, A);
        add(ep.lap_count, 8, A);
        add(ep.lap_time, 8, A);
        add(ep.checkpoint, 1, A);
        add(ep.rot, 32, 1);
        add(ep.current_time, 8, 1);
        add(ep.done, 1, 1);
    }
    if (cols & F110_STATE_COL_PARAMS) add(h->d_params_all, NPARAMS * 8, A);
    if (cols & F110_STATE_COL_ENV_MAP) add(h->d_env_map, 4, 1);
    if (cols & F110_STATE_COL_RESET_RNG) {
        add(h->rs.job.stream, 2 * sizeof(U128), 1);   // the env's sampler stream {state, inc}
        add(h->rs.job.last, 24, A);                   // ... and its explicit-draw fallback poses
    }
    if (cols & F110_STATE_COL_PARAM_RNG) add(h->ps.job.stream, 2 * sizeof(U128), 1);   // the env's parameter stream {state, inc}
    if (cols & F110_STATE_COL_SCANS) add(h->dev.scans, B * 8, A);   // last: launched on its own (state_launch)
    t.num_envs = h->cfg.num_envs;
    t.step_count = h->dev.step_count;
    t.rowstate = h->d_rng_rowstate;
    t.noise_rows = h->dev.noise_rows;
    if (overflow) t.n = -1;   // state_launch refuses the table
    if (out) *out = t;
    return overflow ? 0 : off;
}

enum StateDir { STATE_PACK, STATE_UNPACK, STATE_CLONE };

// the copy as launches on the main stream: the small columns in one (a workgroup row per column), the scans in a second launch
// sized for them, so neither waits on the other's grid
static int state_launch(f110_sim *h, StateDir dir, const StateCols &all, const StateHeader *hdr, char *blob, int blob_k,
                        const int32_t *src, const int32_t *dst, int k, int32_t *status)
{
    if (all.n < 1 || all.n > kStateMaxCols) return fail(h, F110_ERR_STATE, "state columns: %d columns do not fit the column table", all.n);
    if (k <= 0) return F110_OK;
    StateCols parts[2] = {all, all};
    parts[0].n = 0;
    parts[1].n = 0;
    for (int i = 0; i < all.n; ++i) {
        StateCols &p = parts[all.c[i].bytes > 1024 ? 1 : 0];
        p.c[p.n++] = all.c[i];
    }
    for (int part = 0; part < 2; ++part) {
        const StateCols &p = parts[part];
        if (p.n == 0) continue;
        uint64_t units = 0;
        for (int i = 0; i < p.n; ++i) {
            const uint32_t b = p.c[i].bytes, unit = (b & 15u) == 0u ? 16u : ((b & 7u) == 0u ? 8u : ((b & 3u) == 0u ? 4u : 1u));
            units = std::max<uint64_t>(units, (uint64_t)(b / unit) * p.c[i].per_env * (uint64_t)k);
        }
        const dim3 grid((unsigned)std::min<uint64_t>((units + 255) / 256, part == 0 ? 2048u : 8192u), (unsigned)p.n), block(256);
        int32_t *st = part == 0 ? status : nullptr;   // an entry is counted once, by the first launch
        if (dir == STATE_PACK) {   // (both launches store the same header)
            hipLaunchKernelGGL(k_state_pack, grid, block, 0, h->stream, p, *hdr, src, k, blob, st);
        } else if (dir == STATE_UNPACK) {
            hipLaunchKernelGGL(k_state_unpack, grid, block, 0, h->stream, p, blob, blob_k, src, dst, k, st);
        } else {
            hipLaunchKernelGGL(k_clone_envs, grid, block, 0, h->stream, p, src, dst, k, st);
        }
        HIPCHK(h, hipGetLastError());
    }
    return F110_OK;
}

size_t f110_state_bytes(const f110_sim *h, int32_t n_envs, int32_t flags)
{
    if (!h || n_envs < 0) return 0;
    return state_columns(h, state_col_set(h) | ((flags & F110_STATE_SCANS) ? F110_STATE_COL_SCANS : 0u), n_envs, nullptr);
}

static StateHeader state_header(const f110_sim *h, int k, int32_t flags, uint32_t cols, size_t bytes)
{
    StateHeader hd{};
    std::memcpy(hd.magic, "F110SNAP", 8);
    hd.version = F110_STATE_VERSION;
    hd.k = k;
    hd.A = h->cfg.num_agents;
    hd.B = h->cfg.num_beams;
    hd.flags = flags & F110_STATE_SCANS;
    hd.cols = cols;
    hd.noise_mode = h->noise_src;
    hd.noise_rows = h->dev.noise_rows;
    hd.n_maps = h->multi_map ? 1 + (int32_t)h->extra_maps.size() : 0;
    hd.ego_idx = h->has_episode ? h->ep.ego_idx : -1;
    hd.max_step = h->noise_ub;   // the host's bound on every agent's step_count
    for (int w = 0; w < 4; ++w) hd.noise_id[w] = h->noise_src_id[w];
    hd.std_dev = h->dev.noise_rng ? h->noise_gen.scale : 0.0;
    hd.total_bytes = bytes;
    return hd;
}

static const char *state_col_name(uint32_t bit)
{
    switch (bit) {
    case F110_STATE_COL_RNG: return "device-noise stream positions";
    case F110_STATE_COL_RNG_SEED: return "per-agent noise seeds";
    case F110_STATE_COL_EPISODE: return "episode (f110_episode_init)";
    case F110_STATE_COL_PARAMS: return "per-agent params (f110_set_params_batch)";
    case F110_STATE_COL_ENV_MAP: return "env map slots (f110_set_env_maps)";
    case F110_STATE_COL_RESET_RNG: return "reset sampler (f110_reset_sampler_set)";
    case F110_STATE_COL_PARAM_RNG: return "parameter sampler (f110_param_sampler_set)";
    default: return "agent";
    }
}

// may the blob with header hd go into h?  (F110_ERR_STATE with a message when not)
static int state_check(f110_sim *h, const StateHeader &hd)
{
    if (std::memcmp(hd.magic, "F110SNAP", 8) != 0) return fail(h, F110_ERR_STATE, "not a simulator state blob (bad magic)");
    if (hd.version != F110_STATE_VERSION)
        return fail(h, F110_ERR_STATE, "state blob format version %u, this library reads version %d", hd.version, F110_STATE_VERSION);
    if (hd.A != h->cfg.num_agents || hd.B != h->cfg.num_beams)
        return fail(h, F110_ERR_STATE, "state blob of %d agents per env x %d beams, this handle has %d x %d", hd.A, hd.B, h->cfg.num_agents,
                    h->cfg.num_beams);
    if (hd.k < 0) return fail(h, F110_ERR_STATE, "state blob with a negative env count");
    static const char *modes[] = {"no noise", "a noise table", "the shared device noise stream", "per-agent device noise streams"};
    const int mb = hd.noise_mode, mh = h->noise_src;
    if (mb < 0 || mb > 3) return fail(h, F110_ERR_STATE, "state blob with an unknown noise mode %d", mb);
    if (mb != mh) return fail(h, F110_ERR_STATE, "state blob saved with %s, this handle has %s", modes[mb], modes[mh]);
    if ((mb == 1 || mb == 2) && std::memcmp(hd.noise_id, h->noise_src_id, sizeof hd.noise_id) != 0)
        return fail(h, F110_ERR_STATE, "state blob saved with a different %s (%s)", mb == 1 ? "noise table" : "noise seed",
                    mb == 1 ? "table contents" : "PCG64 state");
    if (mb >= 2 && hd.std_dev != h->noise_gen.scale)
        return fail(h, F110_ERR_STATE, "state blob saved with noise std_dev %g, this handle has %g", hd.std_dev, h->noise_gen.scale);
    const uint32_t want = state_col_set(h), have = hd.cols & ~(uint32_t)F110_STATE_COL_SCANS;
    for (uint32_t bit = F110_STATE_COL_RNG; bit <= F110_STATE_COL_PARAM_RNG; bit <<= 1) {
        if ((have & bit) && !(want & bit))
            return fail(h, F110_ERR_STATE, "state blob holds %s columns, which are not active on this handle", state_col_name(bit));
        if (!(have & bit) && (want & bit))
            return fail(h, F110_ERR_STATE, "state blob has no %s columns, which are active on this handle", state_col_name(bit));
    }
    if (!(have & F110_STATE_COL_AGENT) || (hd.cols & ~0x1ffu)) return fail(h, F110_ERR_STATE, "state blob with an unknown column set 0x%x", hd.cols);
    if ((hd.cols & F110_STATE_COL_SCANS) != ((hd.flags & F110_STATE_SCANS) ? (uint32_t)F110_STATE_COL_SCANS : 0u))
        return fail(h, F110_ERR_STATE, "state blob header is inconsistent (flags / columns)");
    if ((have & F110_STATE_COL_ENV_MAP) && hd.n_maps > 1 + (int)h->extra_maps.size())
        return fail(h, F110_ERR_STATE, "state blob uses %d map slots, this handle has %d", hd.n_maps, 1 + (int)h->extra_maps.size());
    if (hd.total_bytes != state_columns(h, hd.cols, hd.k, nullptr)) return fail(h, F110_ERR_STATE, "state blob size does not match its header");
    if (hd.max_step < 0) return fail(h, F110_ERR_STATE, "state blob with a negative step bound");
    return F110_OK;
}

// host invariants after restored / cloned entries landed (stream-ordered on the main stream)
static int state_after_load(f110_sim *h, long long max_step, bool whole)
{
    h->noise_ub = whole ? max_step : std::max(h->noise_ub, max_step);   // the row cache grows to it at the next step (f110_step_device)
    if (h->multi_map) {   // the slots changed under the scan order: rebuild it from the restored assignment
        std::vector<int32_t> em((size_t)h->cfg.num_envs);
        HIPCHK(h, hipMemcpyAsync(em.data(), h->d_env_map, sizeof(int32_t) * em.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        TRY(f110_set_env_maps(h, em.data()));
    }
    return F110_OK;
}

int f110_state_save_device(f110_sim *h, const int32_t *d_env_idx, int32_t k, void *d_blob, int32_t flags)
{
    if (!h || !d_blob) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (k < 0 || (!d_env_idx && k != h->cfg.num_envs))
        return fail(h, F110_ERR_INVALID, "f110_state_save_device: k = %d (without an index list k must be num_envs = %d)", k, h->cfg.num_envs);
    if (reinterpret_cast<uintptr_t>(d_blob) & 15u) return fail(h, F110_ERR_INVALID, "f110_state_save_device: the blob must be 16-byte aligned");
    const uint32_t cols = state_col_set(h) | ((flags & F110_STATE_SCANS) ? F110_STATE_COL_SCANS : 0u);
    StateCols t;
    const size_t bytes = state_columns(h, cols, k, &t);
    const StateHeader hd = state_header(h, k, flags, cols, bytes);
    if (k == 0) {
        HIPCHK(h, hipMemcpyAsync(d_blob, &hd, sizeof hd, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        return F110_OK;
    }
    return state_launch(h, STATE_PACK, t, &hd, static_cast<char *>(d_blob), 0, d_env_idx, nullptr, k, nullptr);
}

static int state_load_blob(f110_sim *h, const StateHeader &hd, const void *d_blob, const int32_t *d_src, const int32_t *d_dst, int32_t k,
                           int32_t *d_status, bool whole)
{
    TRY(state_check(h, hd));
    StateCols t;
    (void)state_columns(h, hd.cols, hd.k, &t);   // the blob's sections (the scans only when it has them)
    TRY(state_launch(h, STATE_UNPACK, t, nullptr, static_cast<char *>(const_cast<void *>(d_blob)), hd.k, d_src, d_dst, k, d_status));
    return state_after_load(h, hd.max_step, whole);
}

int f110_state_load_device(f110_sim *h, const void *d_blob, const int32_t *d_src, const int32_t *d_dst, int32_t k, int32_t *d_status)
{
    if (!h || !d_blob) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (k < 0) return fail(h, F110_ERR_INVALID, "f110_state_load_device: k = %d", k);
    if (reinterpret_cast<uintptr_t>(d_blob) & 15u) return fail(h, F110_ERR_INVALID, "f110_state_load_device: the blob must be 16-byte aligned");
    StateHeader hd{};
    HIPCHK(h, hipMemcpyAsync(&hd, d_blob, sizeof hd, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return state_load_blob(h, hd, d_blob, d_src, d_dst, k, d_status, false);
}

int f110_clone_envs_device(f110_sim *h, const int32_t *d_src, const int32_t *d_dst, int32_t k, int32_t *d_status)
{
    if (!h || !d_src || !d_dst) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (k < 0) return fail(h, F110_ERR_INVALID, "f110_clone_envs_device: k = %d", k);
    StateCols t;
    (void)state_columns(h, state_col_set(h) | F110_STATE_COL_SCANS, k, &t);   // the observation travels with the state
    TRY(state_launch(h, STATE_CLONE, t, nullptr, nullptr, 0, d_src, d_dst, k, d_status));
    return state_after_load(h, h->noise_ub, false);   // (clones are copies of envs of this handle: the step bound holds)
}

static int state_scratch(f110_sim *h, size_t bytes)
{
    if (bytes <= h->d_state_blob.capacity()) return F110_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return dgrow(h, h->d_state_blob, bytes);
}

int f110_state_save(f110_sim *h, void *h_blob, int32_t flags)
{
    if (!h || !h_blob) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    const int E = h->cfg.num_envs;
    const uint32_t cols = state_col_set(h) | ((flags & F110_STATE_SCANS) ? F110_STATE_COL_SCANS : 0u);
    StateCols t;
    const size_t bytes = state_columns(h, cols, E, &t);
    TRY(state_scratch(h, bytes));
    const StateHeader hd = state_header(h, E, flags, cols, bytes);
    TRY(state_launch(h, STATE_PACK, t, &hd, reinterpret_cast<char *>(h->d_state_blob.get()), 0, nullptr, nullptr, E, nullptr));
    HIPCHK(h, hipMemcpyAsync(h_blob, h->d_state_blob, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_state_load(f110_sim *h, const void *h_blob)
{
    if (!h || !h_blob) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    StateHeader hd;
    std::memcpy(&hd, h_blob, sizeof hd);
    TRY(state_check(h, hd));
    if (hd.k != h->cfg.num_envs)
        return fail(h, F110_ERR_STATE, "state blob of %d envs, this handle has %d (f110_state_load_device takes index lists)", hd.k, h->cfg.num_envs);
    TRY(state_scratch(h, hd.total_bytes));
    HIPCHK(h, hipMemcpyAsync(h->d_state_blob, h_blob, hd.total_bytes, hipMemcpyHostToDevice, h->stream));
    TRY(state_load_blob(h, hd, h->d_state_blob, nullptr, nullptr, hd.k, nullptr, true));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // the caller's buffer is consumed on return
    return F110_OK;
}

int f110_get_device_views(f110_sim *h, f110_device_views *v)
{
    if (!h || !v) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    v->scans = h->dev.scans;
    v->state = h->dev.state;
    v->agent_poses = h->dev.snap_pose;
    v->collisions = h->dev.collisions;
    v->collision_idx = h->dev.collision_idx;
    v->in_collision = h->dev.in_collision;
    v->step_count = h->dev.step_count;
    v->stream = (void *)h->stream;
    return F110_OK;
}

int f110_device_mem_info(f110_sim *h, size_t *free_bytes, size_t *total_bytes)
{
    if (!h || !free_bytes || !total_bytes) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemGetInfo(free_bytes, total_bytes));
    return F110_OK;
}

int f110_device_alloc(f110_sim *h, size_t bytes, void **out)
{
    if (!h || !out) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    HIPCHK(h, hipMalloc(out, bytes ? bytes : 8));
    return F110_OK;
}

int f110_device_free(f110_sim *h, void *p)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (p) {
        HIPCHK(h, hipStreamSynchronize(h->stream));
        HIPCHK(h, hipFree(p));
    }
    return F110_OK;
}

int f110_memcpy_h2d(f110_sim *h, void *dst, const void *src, size_t bytes)
{
    if (!h || !dst || !src) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_memcpy_d2h(f110_sim *h, void *dst, const void *src, size_t bytes)
{
    if (!h || !dst || !src) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

// ---- timing ------------------------------------------------------------------------------
int f110_timer_begin(f110_sim *h)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipEventRecord(h->ev_begin, h->stream));
    return F110_OK;
}

int f110_timer_end_ms(f110_sim *h, double *ms)
{
    if (!h || !ms) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    HIPCHK(h, hipEventRecord(h->ev_end, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev_end));
    float f = 0.f;
    HIPCHK(h, hipEventElapsedTime(&f, h->ev_begin, h->ev_end));
    *ms = (double)f;
    return F110_OK;
}

int f110_profile_kernels(f110_sim *h, int32_t enable)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->profiling = enable != 0;
    h->prof_used = 0;
    return F110_OK;
}

int f110_profile_read(f110_sim *h, int32_t *n_launches, double *scan_ms, double *dyn_ms, double *fin_ms)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    double s = 0, dsum = 0, fsum = 0;
    int n = 0;
    for (size_t i = 0; i + 4 <= h->prof_used; i += 4) {
        float a = 0.f, b = 0.f, c = 0.f;
        HIPCHK(h, hipEventElapsedTime(&a, h->prof_events[i], h->prof_events[i + 1]));
        HIPCHK(h, hipEventElapsedTime(&b, h->prof_events[i + 1], h->prof_events[i + 2]));
        HIPCHK(h, hipEventElapsedTime(&c, h->prof_events[i + 2], h->prof_events[i + 3]));
        dsum += a;
        s += b;
        fsum += c;
        ++n;
    }
    if (fin_ms) *fin_ms = fsum;
    if (n_launches) *n_launches = n;
    if (scan_ms) *scan_ms = s;
    if (dyn_ms) *dyn_ms = dsum;
    return F110_OK;
}

// ---- unit entry points ---------------------------------------------------------------------
int f110_scan_batch(f110_sim *h, const double *poses, int32_t m, double *ranges, int32_t *hit_rc, int64_t *lookups)
{
    if (!h || !poses || !ranges || m < 0) return fail(h, F110_ERR_INVALID, "f110_scan_batch: bad argument");
    ENTER(h);
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (m == 0) return F110_OK;
    const size_t B = (size_t)h->cfg.num_beams;
    Scratch s(h);
    RayJob j{};
    const double *dp = s.in(poses, (size_t)3 * m);
    j.ranges = s.out(ranges, (size_t)m * B);
    j.hit_rc = s.out(hit_rc, (size_t)m * B * 2);
    j.lookups = s.out(reinterpret_cast<unsigned long long *>(lookups), (size_t)m);
    double *dpx = s.tmp<double>((size_t)m), *dpy = s.tmp<double>((size_t)m), *dst = s.tmp<double>((size_t)m);
    TRY(s.ready());
    if (j.lookups) HIPCHK(h, hipMemsetAsync(j.lookups, 0, sizeof(unsigned long long) * m, h->stream));
    hipLaunchKernelGGL(k_prepare_poses, grid1d(m, 128), dim3(128), 0, h->stream, h->k, dp, m, dpx, dpy, dst);
    j.n_rays = (uint32_t)m * (uint32_t)B;
    j.n_poses = m;
    j.pose_x = dpx;
    j.pose_y = dpy;
    j.dir_start = dst;
    j.path_stats = h->path_stats_on ? h->d_path_stats : nullptr;
    j.k_cold = cold_consts(h);
    if (!j.k_cold) return fail(h, F110_ERR_HIP, "f110_scan_batch: constant upload failed");
    set_div_magic(j, (uint32_t)B);
    scan_rays_fn fn = pick_rays<false>(h->k, h->cfg.map_layout);
    const dim3 grid = rays_grid(j, h->scan_block, h->scan_tasks_per_wave);
    hipLaunchKernelGGL(fn, grid, dim3(h->scan_block), 0, h->stream, j, h->k);
    return s.finish();
}

// ---- the reference's example policy (examples/waypoint_follow.py) -----------------------------
static int check_planner_args(f110_sim *h, const void *wp, int32_t M, double lookahead)
{
    if (!h || !wp) return fail(h, F110_ERR_INVALID, "pure pursuit: null argument");
    if (M < 2) return fail(h, F110_ERR_INVALID, "pure pursuit: need at least 2 waypoints (got %d)", M);
    if (!(lookahead > 0)) return fail(h, F110_ERR_INVALID, "pure pursuit: lookahead distance must be positive");
    return F110_OK;
}

int f110_pure_pursuit_batch(f110_sim *h, const double *h_waypoints, int32_t M, const double *h_poses, int32_t m, double lookahead,
                            double vgain, double wheelbase, double max_reacquire, double *h_actions)
{
    TRY(check_planner_args(h, h_waypoints, M, lookahead));
    if (!h_poses || !h_actions || m < 0) return fail(h, F110_ERR_INVALID, "pure pursuit: bad argument");
    if (m == 0) return F110_OK;
    ENTER(h);
    Scratch s(h);
    const double *dw = s.in(h_waypoints, (size_t)3 * M), *dp = s.in(h_poses, (size_t)3 * m);
    double *da = s.out(h_actions, (size_t)2 * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_pure_pursuit, grid1d((size_t)m * kPlanLanes, 256), dim3(256), 0, h->stream, dw, M, dp, dp + 1, dp + 2, 3, m, lookahead, vgain, wheelbase,
                       max_reacquire, da);
    return s.finish();
}

int f110_pure_pursuit_device(f110_sim *h, const double *d_waypoints, int32_t M, double lookahead, double vgain, double wheelbase,
                             double max_reacquire, double *d_actions)
{
    TRY(check_planner_args(h, d_waypoints, M, lookahead));
    if (!d_actions) return fail(h, F110_ERR_INVALID, "pure pursuit: null actions buffer");
    const int N = h->N;
    const double *st = h->dev.state;
    // a closed device-side loop (plan, step, plan, ...) behind a two-block step: each block's agents are planned for on the
    // block's own stream (a pose in, an action out, per agent), so the two halves of the batch stay independent
    EnvBlocks w;
    TRY(env_blocks_follow(h, w));
    const int A = h->cfg.num_agents;
    for (const EnvBlock &b : w) {
        const size_t i0 = (size_t)b.e0 * A;
        const int n = b.count * A;
        hipLaunchKernelGGL(k_pure_pursuit, grid1d((size_t)n * kPlanLanes, 256), dim3(256), 0, b.stream, d_waypoints, M, st + i0, st + N + i0,
                           st + 4 * (size_t)N + i0, 1, n, lookahead, vgain, wheelbase, max_reacquire, d_actions + 2 * i0);
    }
    HIPCHK(h, hipGetLastError());
    h->touched = false;
    return F110_OK;
}

int f110_scan_policy_device(f110_sim *h, double steer_gain, double steer_max, double sector_limit, double v_lo, double v_hi, double d_ref, double *d_actions)
{
    if (!h || !d_actions) return fail(h, F110_ERR_INVALID, "scan policy: null argument");
    if (!(d_ref > 0.) || !(steer_max >= 0.)) return fail(h, F110_ERR_INVALID, "scan policy: d_ref must be > 0 and steer_max >= 0");
    if (h->cfg.num_beams > 2048) return fail(h, F110_ERR_INVALID, "scan policy: at most 2048 beams (the rows are staged in LDS)");
    if (h->cfg.num_beams < 64) return fail(h, F110_ERR_INVALID, "scan policy: needs at least 64 beams (one per sector)");
    if (!(sector_limit >= h->cfg.fov / 128.)) return fail(h, F110_ERR_INVALID, "scan policy: sector_limit must be at least fov/128 (half a sector), else no sector is eligible");
    EnvBlocks w;   // behind a two-block step: each block's agents on the block's own stream (an agent reads its own scan row only)
    TRY(env_blocks_follow(h, w));
    const int A = h->cfg.num_agents, B = h->cfg.num_beams;
    for (const EnvBlock &b : w) {
        const int n = b.count * A;
        hipLaunchKernelGGL(k_scan_policy, grid1d((size_t)n * 64, 256), dim3(256), (size_t)4 * B * sizeof(double), b.stream, h->dev.scans, B, h->cfg.fov, b.e0 * A, n, steer_gain, steer_max,
                           sector_limit, v_lo, v_hi, d_ref, d_actions);
    }
    HIPCHK(h, hipGetLastError());
    h->touched = false;
    return F110_OK;
}

// ---- what the per-agent features' specs and launch plans share ------------------------------------------------------------------
// a spec's beam window: 0, 0 is every beam, otherwise [lo, hi) must lie within the handle's beams; on success its first beam and width
static int beam_window(f110_sim *h, const char *who, int lo, int hi, int *lo_out, int *W)
{
    const int B = h->cfg.num_beams, end = (lo == 0 && hi == 0) ? B : hi;
    if (lo < 0 || end > B || lo >= end) return fail(h, F110_ERR_INVALID, "%s: beams [%d, %d) are not a range within the %d beams", who, lo, hi, B);
    *lo_out = lo;
    *W = end - lo;
    return F110_OK;
}

// one wave per agent with wave_bytes of LDS: the workgroup size of 1..4 waves (within 64 KiB) that packs the most waves into a CU's 160 KiB
static int plan_waves(int wave_bytes)
{
    int best = 1, best_waves = 0;
    for (int w = 1; w <= 4; ++w) {
        if ((long long)w * wave_bytes > 65536) break;
        const int per_cu = std::min(32, (int)(163840 / ((long long)w * wave_bytes)) * w);
        if (per_cu >= best_waves) {
            best_waves = per_cu;
            best = w;
        }
    }
    return best;
}

// ---- compact observations (include/f110.h) ----------------------------------------------------------------------------------
// the spec's refusals; on success the kernel's row spec, W's first beam and F.  unit: the eight sources come from the caller
static int obs_check_spec(f110_sim *h, const f110_obs_spec *spec, const void *out, bool unit, ObsRowSpec &rs, int &beam_lo)
{
    if (!spec || !out) return fail(h, F110_ERR_INVALID, "obs encode: spec and the output buffer are required");
    const f110_obs_spec &sp = *spec;
    int lo = 0, W = 0;
    TRY(beam_window(h, "obs encode", sp.beam_lo, sp.beam_hi, &lo, &W));
    const int K = sp.sectors;
    if (K < 0 || K > W) return fail(h, F110_ERR_INVALID, "obs encode: sectors = %d is outside 0..%d (the beams used)", K, W);
    if (sp.pool < F110_OBS_POOL_MIN || sp.pool > F110_OBS_POOL_CENTER) return fail(h, F110_ERR_INVALID, "obs encode: unknown pool %d", sp.pool);
    if (sp.features & ~F110_OBS_ALL_FEATURES) return fail(h, F110_ERR_INVALID, "obs encode: unknown feature bits 0x%x", sp.features);
    if (sp.flags & ~F110_OBS_FILL) return fail(h, F110_ERR_INVALID, "obs encode: unknown flags 0x%x", sp.flags);
    if (sp.frames < 1 || sp.frames > F110_OBS_MAX_FRAMES) return fail(h, F110_ERR_INVALID, "obs encode: frames = %d is outside 1..%d", sp.frames, F110_OBS_MAX_FRAMES);
    if (K > 0 && !(std::isfinite(sp.range_clip) && sp.range_clip > 0 && std::isfinite(sp.range_scale) && sp.range_scale > 0))
        return fail(h, F110_ERR_INVALID, "obs encode: range_clip and range_scale must be finite and > 0");
    rs = ObsRowSpec{};
    for (int c = 0; c < F110_OBS_NFEATURES; ++c) {
        if (!(sp.features >> c & 1)) continue;
        if (!(std::isfinite(sp.feat_scale[c]) && sp.feat_scale[c] != 0.0)) return fail(h, F110_ERR_INVALID, "obs encode: feat_scale[%d] must be finite and non-zero", c);
        rs.feat[rs.nfeat] = c;
        rs.feat_scale[rs.nfeat++] = sp.feat_scale[c];
    }
    for (int c = rs.nfeat; c < F110_OBS_NFEATURES; ++c) rs.feat_scale[c] = 1.0;
    const int D = K + rs.nfeat;
    if (D == 0) return fail(h, F110_ERR_INVALID, "obs encode: no sectors and no features (D = 0)");
    if ((long long)sp.frames * D > F110_OBS_MAX_STACK)
        return fail(h, F110_ERR_INVALID, "obs encode: frames * D = %lld exceeds %d", (long long)sp.frames * D, (int)F110_OBS_MAX_STACK);
    if (reinterpret_cast<uintptr_t>(out) % (unit ? 4 : 16) != 0) return fail(h, F110_ERR_INVALID, "obs encode: the output buffer is not %d-byte aligned", unit ? 4 : 16);
    if (!unit && (sp.features & F110_OBS_TRACK_FEATURES) && !h->track_on)
        return fail(h, F110_ERR_STATE, "obs encode: LATERAL / HEADING_ERROR / DS need tracking (f110_track_enable)");
    rs.W = W;
    rs.K = K;
    rs.pool = sp.pool;
    rs.D = D;
    rs.clip = sp.range_clip;
    rs.scale = sp.range_scale;
    beam_lo = lo;
    return F110_OK;
}

// LDS per wave and waves per workgroup: the row (when it fits next to the stack image in 64 KiB) and the image [F * D + 3]
static void obs_plan_lds(ObsJob &j)
{
    const int img = ((j.F * j.rs.D + 3) * 4 + 15) & ~15;
    const int row = j.rs.K > 0 ? (j.rs.W * 8 + 15) & ~15 : 0;
    j.row_bytes = (row > 0 && row + img <= 65536) ? row : 0;
    j.wave_bytes = j.row_bytes + img;
    j.waves = plan_waves(j.wave_bytes);
}

static void obs_launch(const ObsJob &j, hipStream_t st)
{
    const dim3 grid((unsigned)((j.n + j.waves - 1) / j.waves)), block((unsigned)(64 * j.waves));
    const size_t lds = (size_t)j.waves * j.wave_bytes;
    if (j.row_bytes > 0 || j.rs.K == 0) hipLaunchKernelGGL(k_obs_encode<true>, grid, block, lds, st, j);
    else hipLaunchKernelGGL(k_obs_encode<false>, grid, block, lds, st, j);   // a row too long for LDS: the sectors are walked in HBM
}

int f110_obs_encode_device(f110_sim *h, const f110_obs_spec *spec, float *d_out, float *h_pinned)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ObsJob j{};
    TRY(obs_check_spec(h, spec, d_out, false, j.rs, j.beam_lo));
    const size_t N = (size_t)h->N;
    const size_t per_agent = (size_t)spec->frames * j.rs.D;
    if (h_pinned && !pinned_block_holds(h_pinned, N * per_agent * sizeof(float)))
        return fail(h, F110_ERR_INVALID, "obs encode: h_pinned is not [N][F][D] floats of f110_host_alloc memory");
    EnvBlocks w;   // behind a two-block step: each block's agents on the block's own stream (an agent reads and writes its own rows only)
    TRY(env_blocks_follow(h, w));
    const double *st = h->dev.state;
    const double *src[F110_OBS_NFEATURES] = {st + 3 * N, st + 2 * N, st + 5 * N, st + 6 * N, h->dev.collisions,
                                             h->d_trk ? h->d_trk + 2 * N : nullptr, h->d_trk ? h->d_trk + 3 * N : nullptr, h->d_trk ? h->d_trk + N : nullptr};
    for (int f = 0; f < F110_OBS_NFEATURES; ++f) j.fptr[f] = src[f < j.rs.nfeat ? j.rs.feat[f] : 0];
    j.col_stride = 1;
    j.scans = h->dev.scans;
    j.step_count = h->dev.step_count;
    j.out = d_out;
    j.B = h->cfg.num_beams;
    j.F = spec->frames;
    j.fill = (spec->flags & F110_OBS_FILL) ? 1 : 0;
    obs_plan_lds(j);
    const int A = h->cfg.num_agents;
    return env_blocks_output(h, w, kPinnedObs, per_agent, d_out, h_pinned, [&](const EnvBlock &b) {
        j.i0 = b.e0 * A;
        j.n = b.count * A;
        obs_launch(j, b.stream);
    });
}

int f110_obs_encode_batch(f110_sim *h, const f110_obs_spec *spec, const double *h_scans, const double *h_cols, const int32_t *h_step_count,
                          int32_t m, float *h_inout)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ObsJob j{};
    TRY(obs_check_spec(h, spec, h_inout, true, j.rs, j.beam_lo));
    if (!h_scans || !h_cols || !h_step_count || m < 0) return fail(h, F110_ERR_INVALID, "obs encode: bad argument");
    if (m == 0) return F110_OK;
    ENTER(h);
    Scratch s(h);
    const size_t B = (size_t)h->cfg.num_beams, per_agent = (size_t)spec->frames * j.rs.D;
    j.scans = s.in(h_scans, (size_t)m * B);
    const double *dc = s.in(h_cols, (size_t)m * F110_OBS_NFEATURES);
    j.step_count = s.in(h_step_count, (size_t)m);
    j.out = s.inout(h_inout, (size_t)m * per_agent);
    TRY(s.ready());
    for (int f = 0; f < F110_OBS_NFEATURES; ++f) j.fptr[f] = dc + (f < j.rs.nfeat ? j.rs.feat[f] : 0);
    j.col_stride = F110_OBS_NFEATURES;
    j.B = (int)B;
    j.F = spec->frames;
    j.fill = (spec->flags & F110_OBS_FILL) ? 1 : 0;
    j.i0 = 0;
    j.n = m;
    obs_plan_lds(j);
    obs_launch(j, h->stream);
    return s.finish();
}

// ---- scripted cars: follow the gap (include/f110.h) --------------------------------------------------------------------------
// the spec's refusals; on success the kernel's spec
static int gap_check_spec(f110_sim *h, const f110_gap_follower *g, GapSpec &o)
{
    if (!g) return fail(h, F110_ERR_INVALID, "gap follower: null spec");
    const int B = h->cfg.num_beams;
    int lo = 0, W = 0;
    TRY(beam_window(h, "gap follower", g->beam_lo, g->beam_hi, &lo, &W));
    if (W > kGapMaxWindow) return fail(h, F110_ERR_INVALID, "gap follower: a window of %d beams exceeds %d", W, kGapMaxWindow);
    if (B < 2) return fail(h, F110_ERR_INVALID, "gap follower: needs at least 2 beams (the angle increment)");
    if (g->smooth < 1 || g->smooth > F110_GAP_MAX_SMOOTH || !(g->smooth & 1) || g->smooth > W)
        return fail(h, F110_ERR_INVALID, "gap follower: smooth = %d must be odd, within 1..%d and at most the %d beams of the window", g->smooth, (int)F110_GAP_MAX_SMOOTH, W);
    if (g->target != F110_GAP_TARGET_CENTER && g->target != F110_GAP_TARGET_FURTHEST) return fail(h, F110_ERR_INVALID, "gap follower: unknown target %d", g->target);
    const double d[] = {g->range_clip, g->bubble_radius, g->gap_threshold, g->steer_gain, g->steer_max, g->v_lo, g->v_hi, g->d_ref, g->steer_slow, g->v_turn, g->v_blocked};
    for (double x : d)
        if (!std::isfinite(x)) return fail(h, F110_ERR_INVALID, "gap follower: every setting must be finite");
    if (!(g->range_clip > 0) || !(g->d_ref > 0)) return fail(h, F110_ERR_INVALID, "gap follower: range_clip and d_ref must be > 0");
    if (g->bubble_radius < 0 || g->gap_threshold < 0 || g->steer_slow < 0) return fail(h, F110_ERR_INVALID, "gap follower: bubble_radius, gap_threshold and steer_slow must be >= 0");
    if (g->steer_max < 0) return fail(h, F110_ERR_INVALID, "gap follower: steer_max must be >= 0");
    if (g->v_lo > g->v_hi) return fail(h, F110_ERR_INVALID, "gap follower: v_lo exceeds v_hi");
    o = GapSpec{};
    o.lo = lo, o.W = W, o.S = g->smooth, o.target = g->target;
    o.clip = g->range_clip, o.bubble = g->bubble_radius, o.thresh = g->gap_threshold;
    o.steer_gain = g->steer_gain, o.steer_max = g->steer_max, o.v_lo = g->v_lo, o.v_hi = g->v_hi, o.d_ref = g->d_ref;
    o.steer_slow = g->steer_slow, o.v_turn = g->v_turn, o.v_blocked = g->v_blocked;
    return F110_OK;
}

// LDS per wave (v and p of the widest window) and waves per workgroup
static void gap_plan_lds(GapJob &j, int max_w)
{
    j.wave_bytes = (2 * max_w * 8 + 15) & ~15;
    j.waves = plan_waves(j.wave_bytes);
}

static void gap_launch(const GapJob &j, hipStream_t st)
{
    if (j.n <= 0) return;
    hipLaunchKernelGGL(k_follow_gap, dim3((unsigned)((j.n + j.waves - 1) / j.waves)), dim3((unsigned)(64 * j.waves)), (size_t)j.waves * j.wave_bytes, st, j);
}

// the armed controllers over the agents of one env block, into d_actions [N][2]
static void gap_launch_armed(f110_sim *h, const EnvBlock &b, double *d_actions)
{
    GapJob j{};
    j.specs = h->d_gap_specs;
    j.assign = h->d_gap_assign;
    j.scans = h->dev.scans;
    j.step_count = h->dev.step_count;
    j.actions = d_actions;
    j.fov = h->cfg.fov;
    j.B = h->cfg.num_beams;
    j.i0 = b.e0 * h->cfg.num_agents;
    j.n = b.count * h->cfg.num_agents;
    gap_plan_lds(j, h->gap_max_w);
    gap_launch(j, b.stream);
}

int f110_controllers_set(f110_sim *h, const f110_gap_follower *specs, int32_t n_specs, const int32_t *h_assign)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (n_specs == 0 && !specs && !h_assign) {   // disarm
        ENTER(h);
        h->gap_specs = 0;
        h->gap_assign_host.clear();
        h->d_gap_specs.reset();   // (hipFree waits for the calls in flight that read them)
        h->d_gap_assign.reset();
        return F110_OK;
    }
    if (!specs || !h_assign || n_specs < 1 || n_specs > F110_GAP_MAX_SPECS)
        return fail(h, F110_ERR_INVALID, "controllers: 1..%d specs and an assignment, or NULL, 0, NULL", (int)F110_GAP_MAX_SPECS);
    GapSpec gs[kGapMaxSpecs];
    int max_w = 0;
    for (int k = 0; k < n_specs; ++k) {
        TRY(gap_check_spec(h, specs + k, gs[k]));
        max_w = std::max(max_w, (int)gs[k].W);
    }
    const size_t N = (size_t)h->N;
    for (size_t i = 0; i < N; ++i)
        if (h_assign[i] < -1 || h_assign[i] >= n_specs) return fail(h, F110_ERR_INVALID, "controllers: assignment[%zu] = %d is outside -1..%d", i, h_assign[i], n_specs - 1);
    for (int32_t n : h->mppi.on.agents)
        if (h_assign[n] != -1) return fail(h, F110_ERR_INVALID, "controllers: agent %d is driven by the armed planner (f110_mppi_set)", n);
    if (!h->line_assign_host.empty())
        for (size_t i = 0; i < N; ++i)
            if (h_assign[i] != -1 && h->line_assign_host[i] != -1)
                return fail(h, F110_ERR_INVALID, "controllers: agent %zu has a line follower (f110_line_followers_set)", i);
    ENTER(h);
    if (!h->d_gap_specs) TRY(dmalloc(h, &h->d_gap_specs, (size_t)kGapMaxSpecs));
    if (!h->d_gap_assign) TRY(dmalloc(h, &h->d_gap_assign, N));
    HIPCHK(h, hipMemcpyAsync(h->d_gap_specs, gs, sizeof(GapSpec) * n_specs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_gap_assign, h_assign, sizeof(int32_t) * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (the sources are the caller's and this function's stack)
    h->gap_specs = n_specs;
    h->gap_max_w = max_w;
    h->gap_assign_host.assign(h_assign, h_assign + N);
    return F110_OK;
}

int f110_follow_gap_device(f110_sim *h, double *d_actions)
{
    if (!h || !d_actions) return fail(h, F110_ERR_INVALID, "follow gap: null argument");
    if (reinterpret_cast<uintptr_t>(d_actions) % 16 != 0) return fail(h, F110_ERR_INVALID, "follow gap: the actions buffer is not 16-byte aligned");
    if (h->gap_specs == 0) return fail(h, F110_ERR_STATE, "follow gap: no controllers are armed (f110_controllers_set)");
    EnvBlocks w;   // behind a two-block step: each block's agents on the block's own stream (an agent reads its own scan row only)
    TRY(env_blocks_follow(h, w));
    for (const EnvBlock &b : w) gap_launch_armed(h, b, d_actions);
    HIPCHK(h, hipGetLastError());
    h->touched = false;
    return F110_OK;
}

int f110_follow_gap_batch(f110_sim *h, const f110_gap_follower *spec, const double *h_scans, const int32_t *h_step_count, int32_t m,
                          double *h_actions, int32_t *h_info)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    GapSpec gs;
    TRY(gap_check_spec(h, spec, gs));
    if (!h_scans || !h_actions || m < 0) return fail(h, F110_ERR_INVALID, "follow gap: bad argument");
    if (m == 0) return F110_OK;
    ENTER(h);
    Scratch s(h);
    const size_t B = (size_t)h->cfg.num_beams;
    GapJob j{};
    j.specs = s.in(&gs, 1);
    j.scans = s.in(h_scans, (size_t)m * B);
    j.step_count = s.in(h_step_count, (size_t)m);
    j.actions = s.out(h_actions, (size_t)m * 2);
    j.info = s.out(h_info, (size_t)m * 5);
    TRY(s.ready());
    j.fov = h->cfg.fov;
    j.B = (int)B;
    j.n = m;
    gap_plan_lds(j, gs.W);
    gap_launch(j, h->stream);
    return s.finish();
}

int f110_scan_path_stats(f110_sim *h, int32_t enable, int64_t *out3)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipSetDevice(h->cfg.device_id));
    if (!h->d_path_stats) {
        TRY(dmalloc(h, &h->d_path_stats, 3));
        HIPCHK(h, hipMemsetAsync(h->d_path_stats, 0, 3 * sizeof(unsigned long long), h->stream));
    }
    if (out3) {
        HIPCHK(h, hipMemcpyAsync(out3, h->d_path_stats, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemsetAsync(h->d_path_stats, 0, 3 * sizeof(unsigned long long), h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    if (enable >= 0) h->path_stats_on = enable != 0;
    return F110_OK;
}

int f110_beam_dir_index_batch(f110_sim *h, const double *thetas, int32_t m, int32_t *idx)
{
    if (!h || !thetas || !idx || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *dt = s.in(thetas, (size_t)m);
    int32_t *di = s.out(idx, (size_t)m * h->cfg.num_beams);
    TRY(s.ready());
    hipLaunchKernelGGL(k_dir_index_unit, dim3(m), dim3(128), 0, h->stream, h->k, dt, m, di);
    return s.finish();
}

int f110_dynamics_batch(f110_sim *h, const double *x, const double *u, const double *params, int32_t m, double *f_st, double *f_ks)
{
    if (!h || !x || !u || !params || !f_st || !f_ks || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *dx = s.in(x, (size_t)7 * m), *du = s.in(u, (size_t)2 * m), *dp = s.in(params, (size_t)NPARAMS);
    double *dfs = s.out(f_st, (size_t)7 * m), *dfk = s.out(f_ks, (size_t)5 * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_dynamics_unit, grid1d(m, 128), dim3(128), 0, h->stream, dx, du, dp, m, dfs, dfk);
    return s.finish();
}

int f110_pid_batch(f110_sim *h, const double *in, const double *params, int32_t m, double *out)
{
    if (!h || !in || !params || !out || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *di = s.in(in, (size_t)4 * m), *dp = s.in(params, (size_t)NPARAMS);
    double *dout = s.out(out, (size_t)2 * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_pid_unit, grid1d(m, 128), dim3(128), 0, h->stream, di, dp, m, dout);
    return s.finish();
}

int f110_update_pose_batch(f110_sim *h, const double *s0, const double *b0, const int32_t *c0, const double *act,
                           const double *params, double dt, int32_t integ, double lidar_dist, int32_t m, double *s1,
                           double *b1, int32_t *c1, double *spose)
{
    if (!h || !s0 || !b0 || !c0 || !act || !params || !s1 || !b1 || !c1 || !spose || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (integ != F110_INTEGRATOR_RK4 && integ != F110_INTEGRATOR_EULER) return fail(h, F110_ERR_INVALID, "Invalid Integrator Specified. Please choose RK4 or Euler");
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *ds0 = s.in(s0, (size_t)7 * m), *db0 = s.in(b0, (size_t)2 * m);
    const int32_t *dc0 = s.in(c0, (size_t)m);
    const double *dact = s.in(act, (size_t)2 * m), *dp = s.in(params, (size_t)NPARAMS);
    double *ds1 = s.out(s1, (size_t)7 * m), *db1 = s.out(b1, (size_t)2 * m);
    int32_t *dc1 = s.out(c1, (size_t)m);
    double *dsp = s.out(spose, (size_t)3 * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_update_pose_unit, grid1d(m, 128), dim3(128), 0, h->stream, ds0, db0, dc0, dact, dp, dt, integ, lidar_dist, m, ds1, db1, dc1, dsp);
    return s.finish();
}

int f110_get_vertices_batch(f110_sim *h, const double *poses, double length, double width, int32_t m, double *verts)
{
    if (!h || !poses || !verts || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *dp = s.in(poses, (size_t)3 * m);
    double *dv = s.out(verts, (size_t)8 * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_vertices_unit, grid1d(m, 128), dim3(128), 0, h->stream, dp, length, width, m, dv);
    return s.finish();
}

int f110_gjk_batch(f110_sim *h, const double *va, const double *vb, int32_t m, int32_t *flags)
{
    if (!h || !va || !vb || !flags || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *da = s.in(va, (size_t)8 * m), *db = s.in(vb, (size_t)8 * m);
    int32_t *df = s.out(flags, (size_t)m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_gjk_unit, grid1d(m, 128), dim3(128), 0, h->stream, da, db, m, df);
    return s.finish();
}

int f110_collision_multiple_batch(f110_sim *h, const double *verts, int32_t groups, int32_t n, double *col, double *idx)
{
    if (!h || !verts || !col || !idx || groups < 0 || n < 1) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (groups == 0) return F110_OK;
    const size_t t = (size_t)groups * n;
    Scratch s(h);
    const double *dv = s.in(verts, 8 * t);
    double *dc = s.out(col, t), *di = s.out(idx, t);
    TRY(s.ready());
    hipLaunchKernelGGL(k_collision_multiple_unit, grid1d(t, 128), dim3(128), 0, h->stream, dv, groups, n, dc, di);
    return s.finish();
}

int f110_ttc_batch(f110_sim *h, const double *scans, const double *vels, int32_t m, double thresh, int32_t *flags)
{
    if (!h || !scans || !vels || !flags || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    const size_t B = (size_t)h->cfg.num_beams;
    Scratch s(h);
    const double *ds = s.in(scans, (size_t)m * B), *dv = s.in(vels, (size_t)m);
    int32_t *df = s.out(flags, (size_t)m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_ttc_unit, dim3(m), dim3(128), 0, h->stream, ds, dv, m, (int)B, h->d_beam_cos, h->d_side, thresh, df);
    return s.finish();
}

int f110_raycast_batch(f110_sim *h, const double *ego, const double *verts, int32_t m, double *scans, int32_t *minmax)
{
    if (!h || !ego || !verts || !scans || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    const size_t B = (size_t)h->cfg.num_beams;
    Scratch s(h);
    const double *de = s.in(ego, (size_t)3 * m), *dv = s.in(verts, (size_t)8 * m);
    double *ds = s.inout(scans, (size_t)m * B);
    int32_t *dm = s.out(minmax, (size_t)2 * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_raycast_unit, dim3(m), dim3(128), 0, h->stream, de, dv, m, (int)B, h->d_scan_angles, h->dev.angle_inc, h->beams_uniform ? 1 : 0, ds, dm);
    return s.finish();
}

int f110_get_range_batch(f110_sim *h, const double *in, int32_t m, double *out)
{
    if (!h || !in || !out || m < 0) return fail(h, F110_ERR_INVALID, "bad argument");
    ENTER(h);
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *di = s.in(in, (size_t)8 * m);
    double *dout = s.out(out, (size_t)m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_get_range_unit, grid1d(m, 128), dim3(128), 0, h->stream, di, m, dout);
    return s.finish();
}

int f110_edt_sq(f110_sim *h, const uint8_t *img, int32_t H, int32_t W, uint32_t *d2)
{
    if (!h || !img || !d2) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(h, F110_ERR_INVALID, "f110_edt_sq: bad shape %dx%d", H, W);
    Scratch s(h);
    TRY(edt_launch(s, img, H, W, false, d2, 0.0, nullptr));
    return s.finish();
}

int f110_dt_from_bitmap(f110_sim *h, const uint8_t *img, int32_t H, int32_t W, double resolution, double *dt)
{
    if (!h || !img || !dt) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (H < 1 || W < 1 || H > 16384 || W > 16384) return fail(h, F110_ERR_INVALID, "f110_dt_from_bitmap: bad shape %dx%d", H, W);
    Scratch s(h);
    double *ddt = s.out(dt, (size_t)H * W);
    TRY(s.ready());
    TRY(edt_launch(s, img, H, W, false, nullptr, resolution, ddt));
    return s.finish();
}

int f110_helper_batch(f110_sim *h, int32_t op, const double *in, int32_t m, int32_t n, double *out)
{
    if (!h || !in || !out || m < 0) return fail(h, F110_ERR_INVALID, "f110_helper_batch: bad argument");
    ENTER(h);
    int in_w = 0, out_w = 0;
    bool bodies = false, needs_map = false;
    switch (op) {
    case F110_OP_ACCL_CONSTRAINTS: case F110_OP_STEERING_CONSTRAINT: in_w = 6; out_w = 1; break;
    case F110_OP_CROSS: in_w = 4; out_w = 1; break;
    case F110_OP_ARE_COLLINEAR: in_w = 6; out_w = 1; break;
    case F110_OP_PERPENDICULAR: in_w = 2; out_w = 2; break;
    case F110_OP_TRIPLE_PRODUCT: in_w = 6; out_w = 2; break;
    case F110_OP_AVG_POINT: bodies = true; in_w = 2 * n; out_w = 2; break;
    case F110_OP_FURTHEST_POINT: bodies = true; in_w = 2 * n + 2; out_w = 1; break;
    case F110_OP_SUPPORT: bodies = true; in_w = 4 * n + 2; out_w = 2; break;
    case F110_OP_GET_TRMTX: in_w = 3; out_w = 16; break;
    case F110_OP_XY_2_RC: in_w = 9; out_w = 2; break;
    case F110_OP_DISTANCE_TRANSFORM: needs_map = true; in_w = 2; out_w = 1; break;
    case F110_OP_TRACE_RAY: needs_map = true; in_w = 3; out_w = 1; break;
    default: return fail(h, F110_ERR_INVALID, "f110_helper_batch: unknown op %d", op);
    }
    if (bodies && (n < 1 || n > 4096)) return fail(h, F110_ERR_INVALID, "f110_helper_batch: a body needs 1..4096 vertices (got %d)", n);
    if (needs_map && !h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    if (m == 0) return F110_OK;
    Scratch s(h);
    const double *di = s.in(in, (size_t)in_w * m);
    double *dout = s.out(out, (size_t)out_w * m);
    TRY(s.ready());
    hipLaunchKernelGGL(k_helper_unit, grid1d(m, 128), dim3(128), 0, h->stream, op, di, m, n, in_w, out_w, dout, h->k);
    return s.finish();
}

}  // extern "C"

// ---- track progress (f110_track_*) ---------------------------------------------------------------------------------------------
static int track_alloc(f110_sim *h)
{
    if (h->d_trk) return F110_OK;
    const size_t N = (size_t)h->N;
    TRY(dmalloc(h, &h->d_trk, 4 * N));
    TRY(dmalloc(h, &h->d_trk_seg, N));
    TRY(dmalloc(h, &h->d_trk_cache, 3 * N));
    TRY(dmalloc(h, &h->d_trk_ok, N));
    HIPCHK(h, hipMemsetAsync(h->d_trk, 0, 4 * N * sizeof(double), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_trk_seg, 0, N * sizeof(int32_t), h->stream));
    HIPCHK(h, hipMemsetAsync(h->d_trk_ok, 0, N * sizeof(int32_t), h->stream));
    return F110_OK;
}

// the cached s no longer belongs to the slots / tracks: every agent is re-projected at the head of its next step
static int track_invalidate(f110_sim *h)
{
    h->track_checked = false;
    h->line_checked = false;
    if (h->d_trk_ok) HIPCHK(h, hipMemsetAsync(h->d_trk_ok, 0, (size_t)h->N * sizeof(int32_t), h->stream));
    return F110_OK;
}

// the kernels' slot table, one entry per registered map slot (slots without a track: nseg = 0)
static int track_upload(f110_sim *h)
{
    const int slots = 1 + (int)h->extra_maps.size();
    if (!h->tracks_dirty && h->n_tracks_dev == slots) return F110_OK;
    std::vector<TrackDesc> desc((size_t)slots);
    std::vector<PreviewAttr> attrs((size_t)slots);
    h->track_lds = false;
    for (int m = 0; m < slots; ++m) {
        desc[m] = TrackDesc{nullptr, 0, 0, 0.0};
        attrs[m] = PreviewAttr{nullptr, 0, 0};
        if (m < (int)h->tracks.size() && h->tracks[m].nseg > 0) {
            const f110_sim::TrackSlot &ts = h->tracks[m];
            desc[m] = TrackDesc{ts.d_cols, ts.nseg, ts.closed, ts.L};
            attrs[m] = PreviewAttr{ts.d_attr, ts.nattr, ts.npts};
            h->track_lds = h->track_lds || ts.nseg <= kTrackLdsSegs;
        }
    }
    if (h->n_tracks_dev != slots) {
        h->d_tracks.reset();
        h->d_track_attrs.reset();
        h->n_tracks_dev = 0;
        TRY(dmalloc(h, &h->d_tracks, (size_t)slots));
        TRY(dmalloc(h, &h->d_track_attrs, (size_t)slots));
        h->n_tracks_dev = slots;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_tracks, desc.data(), sizeof(TrackDesc) * slots, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_track_attrs, attrs.data(), sizeof(PreviewAttr) * slots, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (desc is a local; rare: only after a change)
    h->tracks_dirty = false;
    return F110_OK;
}

static bool track_has(const f110_sim *h, int slot) { return slot >= 0 && slot < (int)h->tracks.size() && h->tracks[slot].nseg > 0; }

// every map slot in use has a track: slot 0, or under f110_set_env_maps the slot of every env (agents set: of the envs that
// hold one of this ascending list of agents).  Refused as "<prefix>, but map slot %d has no track (f110_track_set)".
static int tracks_in_use(f110_sim *h, const char *prefix, const std::vector<int32_t> *agents = nullptr)
{
    auto need = [&](int32_t slot) {
        return track_has(h, slot) ? F110_OK : fail(h, F110_ERR_STATE, "%s, but map slot %d has no track (f110_track_set)", prefix, slot);
    };
    if (!h->multi_map) return need(0);
    if (!agents) {
        for (int32_t m : h->env_map_host) TRY(need(m));
        return F110_OK;
    }
    const int A = h->cfg.num_agents;
    int last = -1;
    for (int32_t n : *agents) {
        const int e = n / A;
        if (e == last) continue;
        last = e;
        TRY(need(h->env_map_host[e]));
    }
    return F110_OK;
}

// the kernels' slot table reflects `tracks` and the slot count.  After a change the upload is an ordinary entry point on the
// main stream (ENTER); the step (entry = false) joins its groups without becoming one.
static int tracks_current(f110_sim *h, bool entry = true)
{
    if (!h->tracks_dirty && h->n_tracks_dev == 1 + (int)h->extra_maps.size()) return F110_OK;
    if (entry) {
        ENTER(h);
    } else {
        TRY(join_groups(h));
        h->main_dirty = true;
    }
    return track_upload(h);
}

static int track_check(f110_sim *h)
{
    if (h->track_checked) return F110_OK;
    if (!h->multi_map) {
        if (!track_has(h, 0)) return fail(h, F110_ERR_STATE, "track progress: map slot 0 has no track (f110_track_set)");
    } else {
        for (size_t e = 0; e < h->env_map_host.size(); ++e)
            if (!track_has(h, h->env_map_host[e]))
                return fail(h, F110_ERR_STATE, "track progress: env %d is on map slot %d, which has no track (f110_track_set)", (int)e, h->env_map_host[e]);
    }
    h->track_checked = true;
    return F110_OK;
}

// f110_step_device, tracking on: the slot table is current and every env's slot has a track
static int track_prepare(f110_sim *h)
{
    TRY(track_check(h));
    return tracks_current(h, false);
}

// one projection pass of the step over agents [begin, begin + count) on stream st
static int track_launch(f110_sim *h, hipStream_t st, int mode, int begin, int count)
{
    if (count <= 0) return F110_OK;
    const size_t N = (size_t)h->N;
    TrackJob j{};
    j.tracks = h->d_tracks;
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.A = h->cfg.num_agents;
    j.begin = begin;
    j.count = count;
    j.stride = 1;
    if (mode == kTrackHead) {
        j.px = h->dev.state;        // x, y of the live state (what the last writer left)
        j.py = h->dev.state + N;
        j.pth = h->dev.state + 4 * N;
    } else {
        j.px = h->dev.snap_pose;    // the post-step pose of the observation
        j.py = h->dev.snap_pose + N;
        j.pth = h->dev.snap_pose + 2 * N;
    }
    j.s = h->d_trk;
    j.ds = h->d_trk + N;
    j.lat = h->d_trk + 2 * N;
    j.head = h->d_trk + 3 * N;
    j.seg = h->d_trk_seg;
    j.c_s = h->d_trk_cache;
    j.c_x = h->d_trk_cache + N;
    j.c_y = h->d_trk_cache + 2 * N;
    j.c_ok = h->d_trk_ok;
    j.hint = h->d_trk_seg;   // (the head pass reads it before the post pass of the same block rewrites it: stream order)
    const dim3 grid = grid1d((size_t)count * kTrackLanes, 256);
    if (mode == kTrackHead) {
        if (h->track_lds) hipLaunchKernelGGL((k_track_project<kTrackHead, true>), grid, dim3(256), 0, st, j);
        else hipLaunchKernelGGL((k_track_project<kTrackHead, false>), grid, dim3(256), 0, st, j);
    } else {
        if (h->track_lds) hipLaunchKernelGGL((k_track_project<kTrackPost, true>), grid, dim3(256), 0, st, j);
        else hipLaunchKernelGGL((k_track_project<kTrackPost, false>), grid, dim3(256), 0, st, j);
    }
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

int f110_track_set(f110_sim *h, int32_t slot, const double *h_xy, int32_t M, int32_t closed)
{
    if (!h || !h_xy) return fail(h, F110_ERR_INVALID, "f110_track_set: null argument");
    ENTER(h);
    const int slots = 1 + (int)h->extra_maps.size();
    if (slot < 0 || slot >= slots) return fail(h, F110_ERR_INVALID, "f110_track_set: slot %d, but %d map slots are registered", slot, slots);
    if (M < 2 || M > (1 << 24)) return fail(h, F110_ERR_INVALID, "f110_track_set: a track needs 2 .. 2^24 points, got %d", M);
    int m = M;
    if (closed && std::memcmp(h_xy, h_xy + 2 * (size_t)(M - 1), 2 * sizeof(double)) == 0) m -= 1;   // a closed csv repeats its first point
    if (closed && m < 3) return fail(h, F110_ERR_INVALID, "f110_track_set: a closed track needs 3 distinct points, got %d", m);
    for (size_t q = 0; q < 2 * (size_t)m; ++q)
        if (!std::isfinite(h_xy[q])) return fail(h, F110_ERR_INVALID, "f110_track_set: point %d is not finite", (int)(q / 2));
    const int nseg = closed ? m : m - 1;
    std::vector<double> cols(7 * (size_t)nseg);
    double cum = 0.0;
    for (int k = 0; k < nseg; ++k) {
        const int k1 = k + 1 == m ? 0 : k + 1;
        const double ax = h_xy[2 * k], ay = h_xy[2 * k + 1];
        const double dx = h_xy[2 * k1] - ax, dy = h_xy[2 * k1 + 1] - ay;
        const double l2 = dx * dx + dy * dy;
        if (!(l2 > 0.0)) return fail(h, F110_ERR_INVALID, "f110_track_set: segment %d -> %d has zero length", k, k1);
        const double len = std::sqrt(l2);
        cols[k] = ax;
        cols[(size_t)nseg + k] = ay;
        cols[2 * (size_t)nseg + k] = dx;
        cols[3 * (size_t)nseg + k] = dy;
        cols[4 * (size_t)nseg + k] = l2;
        cols[5 * (size_t)nseg + k] = len;
        cols[6 * (size_t)nseg + k] = cum;
        cum += len;
    }
    DevBuf<double> d_cols, d_pts;   // built aside: a failure drops them, success moves them into the slot
    TRY(dmalloc(h, &d_cols, cols.size()));
    if (dmalloc(h, &d_pts, 2 * (size_t)m) != F110_OK) return F110_ERR_NOMEM;
    hipError_t e = hipMemcpyAsync(d_cols, cols.data(), cols.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_pts, h_xy, 2 * (size_t)m * sizeof(double), hipMemcpyHostToDevice, h->stream);
    if (e != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, F110_ERR_HIP, "f110_track_set: upload failed: %s", hipGetErrorString(e));
    if ((int)h->tracks.size() <= slot) h->tracks.resize((size_t)slot + 1);
    f110_sim::TrackSlot &ts = h->tracks[slot];
    ts.d_cols = std::move(d_cols);   // (synchronised above: no step reads the old table any more)
    ts.d_pts = std::move(d_pts);
    ts.d_attr.reset();               // a new track: the old one's attributes go with it
    ts.nattr = 0;
    ts.npts = m;
    ts.nseg = nseg;
    ts.closed = closed ? 1 : 0;
    ts.L = cum;
    h->tracks_dirty = true;
    TRY(track_alloc(h));
    return track_invalidate(h);
}

int f110_track_enable(f110_sim *h, int32_t on)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    if (on) {
        TRY(track_alloc(h));
        h->track_checked = false;
        TRY(track_check(h));
        TRY(track_upload(h));
    }
    h->track_on = on != 0;
    return F110_OK;
}

int f110_track_views(f110_sim *h, struct f110_track_views *out)
{
    if (!h || !out) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    TRY(track_alloc(h));
    const size_t N = (size_t)h->N;
    out->s = h->d_trk;
    out->ds = h->d_trk + N;
    out->lateral = h->d_trk + 2 * N;
    out->heading_error = h->d_trk + 3 * N;
    out->segment = h->d_trk_seg;
    return F110_OK;
}

int f110_track_get(f110_sim *h, const f110_track_host *out)
{
    if (!h || !out) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    TRY(track_alloc(h));
    const size_t N = (size_t)h->N;
    TRY(copy_col(h, out->s, h->d_trk, N));
    TRY(copy_col(h, out->ds, h->d_trk + N, N));
    TRY(copy_col(h, out->lateral, h->d_trk + 2 * N, N));
    TRY(copy_col(h, out->heading_error, h->d_trk + 3 * N, N));
    if (out->segment) HIPCHK(h, hipMemcpyAsync(out->segment, h->d_trk_seg, N * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return F110_OK;
}

int f110_track_host_block(f110_sim *h, const f110_track_host *pinned)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));   // a F110_STEP_NO_SYNC step may still be storing into the previous block
    h->trk_pinned_on = false;
    h->trk_pinned = f110_track_host{};
    h->trk_hb = HostBlock{};
    if (!pinned || !(pinned->s || pinned->ds || pinned->lateral || pinned->heading_error || pinned->segment)) return F110_OK;
    HostBlock d{};
    void *p = nullptr;
    TRY(map_host_ptr(h, pinned->s, &p, "track s"));
    d.trk_s = static_cast<double *>(p);
    TRY(map_host_ptr(h, pinned->ds, &p, "track ds"));
    d.trk_ds = static_cast<double *>(p);
    TRY(map_host_ptr(h, pinned->lateral, &p, "track lateral"));
    d.trk_lat = static_cast<double *>(p);
    TRY(map_host_ptr(h, pinned->heading_error, &p, "track heading_error"));
    d.trk_head = static_cast<double *>(p);
    TRY(map_host_ptr(h, pinned->segment, &p, "track segment"));
    d.trk_seg = static_cast<int32_t *>(p);
    TRY(track_alloc(h));
    h->trk_hb = d;
    h->trk_pinned = *pinned;
    h->trk_pinned_on = true;
    return F110_OK;
}

int f110_track_project_batch(f110_sim *h, int32_t slot, const double *h_poses, int32_t m, double *h_out)
{
    if (!h || (m > 0 && (!h_poses || !h_out))) return fail(h, F110_ERR_INVALID, "null argument");
    ENTER(h);
    if (m < 0) return fail(h, F110_ERR_INVALID, "f110_track_project_batch: m = %d", m);
    if (!track_has(h, slot)) return fail(h, F110_ERR_STATE, "f110_track_project_batch: map slot %d has no track (f110_track_set)", slot);
    if (m == 0) return F110_OK;
    TRY(track_upload(h));
    Scratch sc(h);
    TrackJob j{};
    const double *dp = sc.in(h_poses, 3 * (size_t)m);
    j.unit_out = sc.out(h_out, 5 * (size_t)m);
    TRY(sc.ready());
    j.tracks = h->d_tracks;
    j.A = 1;
    j.count = m;
    j.unit_slot = slot;
    j.px = dp;
    j.py = dp + 1;
    j.pth = dp + 2;
    j.stride = 3;
    const dim3 grid = grid1d((size_t)m * kTrackLanes, 256);
    if (h->tracks[slot].nseg <= kTrackLdsSegs) hipLaunchKernelGGL((k_track_project<kTrackUnit, true>), grid, dim3(256), 0, h->stream, j);
    else hipLaunchKernelGGL((k_track_project<kTrackUnit, false>), grid, dim3(256), 0, h->stream, j);
    return sc.finish();
}

// ---- track preview (f110_track_set_attrs / f110_track_preview_*, include/f110.h) ------------------------------------------------
int f110_track_set_attrs(f110_sim *h, int32_t slot, const double *h_attr, int32_t M, int32_t C)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!track_has(h, slot)) return fail(h, F110_ERR_INVALID, "f110_track_set_attrs: map slot %d has no track (f110_track_set)", slot);
    f110_sim::TrackSlot &ts = h->tracks[slot];
    const bool clear = !h_attr && M == 0 && C == 0;
    std::vector<double> cols;
    if (!clear) {
        if (!h_attr) return fail(h, F110_ERR_INVALID, "f110_track_set_attrs: null attributes (NULL, 0, 0 clears them)");
        if (M != ts.npts) return fail(h, F110_ERR_INVALID, "f110_track_set_attrs: %d rows, but the track on slot %d has %d points", M, slot, ts.npts);
        if (C < 1 || C > F110_TRACK_MAX_ATTRS) return fail(h, F110_ERR_INVALID, "f110_track_set_attrs: 1..%d attributes per point, got %d", (int)F110_TRACK_MAX_ATTRS, C);
        cols.resize((size_t)M * C);
        for (int k = 0; k < M; ++k)
            for (int c = 0; c < C; ++c) {
                const double v = h_attr[(size_t)k * C + c];
                if (!std::isfinite(v)) return fail(h, F110_ERR_INVALID, "f110_track_set_attrs: attribute %d of point %d is not finite", c, k);
                cols[(size_t)c * M + k] = v;   // [C][M]: a station reads one column at k and k + 1
            }
    }
    ENTER(h);
    DevBuf<double> d_attr;
    if (!clear) {
        TRY(dmalloc(h, &d_attr, cols.size()));
        const hipError_t e = hipMemcpyAsync(d_attr, cols.data(), cols.size() * sizeof(double), hipMemcpyHostToDevice, h->stream);
        if (e != hipSuccess) return fail(h, F110_ERR_HIP, "f110_track_set_attrs: upload failed: %s", hipGetErrorString(e));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (the source is a local; no preview reads the old columns any more)
    ts.d_attr = std::move(d_attr);
    ts.nattr = clear ? 0 : C;
    h->tracks_dirty = true;
    h->line_checked = false;
    return F110_OK;
}

// the spec's refusals; on success the kernel's spec
static int preview_check_spec(f110_sim *h, const f110_track_preview *p, PreviewSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "track preview: null spec");
    if (p->points < 1 || p->points > F110_PREVIEW_MAX_POINTS) return fail(h, F110_ERR_INVALID, "track preview: points = %d is outside 1..%d", p->points, (int)F110_PREVIEW_MAX_POINTS);
    if (p->channels == 0 || (p->channels & ~((1 << F110_PREVIEW_NCHANNELS) - 1))) return fail(h, F110_ERR_INVALID, "track preview: channels = 0x%x is empty or has an unknown bit", p->channels);
    if (p->frame != F110_PREVIEW_FRAME_EGO && p->frame != F110_PREVIEW_FRAME_WORLD) return fail(h, F110_ERR_INVALID, "track preview: unknown frame %d", p->frame);
    if (p->flags != 0) return fail(h, F110_ERR_INVALID, "track preview: flags = %d must be 0", p->flags);
    if (!(std::isfinite(p->offset) && p->offset >= 0.0)) return fail(h, F110_ERR_INVALID, "track preview: offset must be finite and >= 0");
    if (!(std::isfinite(p->spacing) && p->spacing > 0.0)) return fail(h, F110_ERR_INVALID, "track preview: spacing must be finite and > 0");
    o = PreviewSpec{};
    for (int b = 0; b < F110_PREVIEW_NCHANNELS; ++b) {
        o.scale[b] = 1.0;
        if (!(p->channels >> b & 1)) continue;
        if (!(std::isfinite(p->scale[b]) && p->scale[b] != 0.0)) return fail(h, F110_ERR_INVALID, "track preview: scale[%d] must be finite and non-zero", b);
        o.scale[b] = p->scale[b];
        o.D += 1;
    }
    o.P = p->points;
    o.channels = p->channels;
    o.frame = p->frame;
    o.offset = p->offset;
    o.spacing = p->spacing;
    return F110_OK;
}

// what a slot in use must offer: a track, the requested attribute columns, and on a closed track more length than the reach
static int preview_check_slot(f110_sim *h, const PreviewSpec &sp, int slot)
{
    if (!track_has(h, slot)) return fail(h, F110_ERR_STATE, "track preview: map slot %d has no track (f110_track_set)", slot);
    const f110_sim::TrackSlot &ts = h->tracks[slot];
    for (int a = 0; a < F110_TRACK_MAX_ATTRS; ++a)
        if ((sp.channels >> (4 + a) & 1) && a >= ts.nattr)
            return fail(h, F110_ERR_STATE, "track preview: attribute %d is requested, but the track on slot %d has %d (f110_track_set_attrs)", a, slot, ts.nattr);
    const double reach = sp.offset + (double)(sp.P - 1) * sp.spacing;
    if (ts.closed && !(ts.L > reach))
        return fail(h, F110_ERR_STATE, "track preview: the closed track on slot %d is %.6g m long, not longer than the preview's reach of %.6g m", slot, ts.L, reach);
    return F110_OK;
}

static void preview_launch(PreviewJob &j, hipStream_t st)
{
    if (j.count <= 0) return;
    j.shift = 0;
    while ((1 << j.shift) < j.sp.P) ++j.shift;
    hipLaunchKernelGGL(k_track_preview, grid1d((size_t)j.count << j.shift, 256), dim3(256), 0, st, j);
}

int f110_track_preview_device(f110_sim *h, const f110_track_preview *spec, float *d_out, float *h_pinned)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    PreviewJob j{};
    TRY(preview_check_spec(h, spec, j.sp));
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return fail(h, F110_ERR_INVALID, "track preview: d_out is null or not 16-byte aligned");
    const size_t N = (size_t)h->N, per_agent = (size_t)j.sp.P * j.sp.D;
    if (h_pinned && !pinned_block_holds(h_pinned, N * per_agent * sizeof(float)))
        return fail(h, F110_ERR_INVALID, "track preview: h_pinned is not [N][P][D] floats of f110_host_alloc memory");
    if (!h->track_on) return fail(h, F110_ERR_STATE, "track preview: tracking is off (f110_track_enable)");
    if (!h->multi_map) TRY(preview_check_slot(h, j.sp, 0));
    else {
        std::vector<char> seen(1 + h->extra_maps.size(), 0);
        for (int32_t m : h->env_map_host) {
            if (m >= 0 && m < (int)seen.size() && seen[m]) continue;
            TRY(preview_check_slot(h, j.sp, m));
            seen[m] = 1;
        }
    }
    TRY(tracks_current(h));   // (attributes set since the last step)
    EnvBlocks w;   // behind a two-block step: each block's agents on the block's own stream (an agent reads its own rows and writes its own block)
    TRY(env_blocks_follow(h, w));
    j.tracks = h->d_tracks;
    j.attrs = h->d_track_attrs;
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.A = h->cfg.num_agents;
    j.unit_slot = -1;
    j.px = h->dev.snap_pose;   // the post-step pose of the observation, the one s was computed from
    j.py = h->dev.snap_pose + N;
    j.pth = h->dev.snap_pose + 2 * N;
    j.ps = h->d_trk;
    j.stride = 1;
    j.out = d_out;
    return env_blocks_output(h, w, kPinnedPreview, per_agent, d_out, h_pinned, [&](const EnvBlock &b) {
        j.begin = b.e0 * j.A;
        j.count = b.count * j.A;
        preview_launch(j, b.stream);
    });
}

int f110_track_preview_batch(f110_sim *h, const f110_track_preview *spec, int32_t slot, const double *h_in, int32_t m, float *h_out,
                             double *h_raw, int32_t *h_seg)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    PreviewJob j{};
    TRY(preview_check_spec(h, spec, j.sp));
    if (m < 0 || (m > 0 && (!h_in || !h_out))) return fail(h, F110_ERR_INVALID, "track preview: bad argument");
    TRY(preview_check_slot(h, j.sp, slot));
    if (m == 0) return F110_OK;
    ENTER(h);
    TRY(track_upload(h));
    Scratch sc(h);
    const size_t rows = (size_t)m * j.sp.P;
    const double *din = sc.in(h_in, 4 * (size_t)m);
    j.out = sc.out(h_out, rows * j.sp.D);
    j.raw = sc.out(h_raw, rows * F110_PREVIEW_NCHANNELS);
    j.seg = sc.out(h_seg, rows);
    TRY(sc.ready());
    j.tracks = h->d_tracks;
    j.attrs = h->d_track_attrs;
    j.A = 1;
    j.count = m;
    j.unit_slot = slot;
    j.px = din;
    j.py = din + 1;
    j.pth = din + 2;
    j.ps = din + 3;
    j.stride = 4;
    preview_launch(j, h->stream);
    return sc.finish();
}

// ---- neighbours (f110_neighbors_*, include/f110.h) --------------------------------------------------------------------------------
// the spec's refusals; on success the kernel's spec
static int nbr_check_spec(f110_sim *h, const f110_neighbors *p, NbrSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "neighbors: null spec");
    if (p->k < 1 || p->k > F110_NBR_MAX_K) return fail(h, F110_ERR_INVALID, "neighbors: k = %d is outside 1..%d", p->k, (int)F110_NBR_MAX_K);
    if (p->channels == 0 || (p->channels & ~((1 << F110_NBR_NCHANNELS) - 1))) return fail(h, F110_ERR_INVALID, "neighbors: channels = 0x%x is empty or has an unknown bit", p->channels);
    if (p->flags != 0) return fail(h, F110_ERR_INVALID, "neighbors: flags = %d must be 0", p->flags);
    if (!(p->max_range > 0.0)) return fail(h, F110_ERR_INVALID, "neighbors: max_range must be > 0 (+inf is allowed)");
    if (!std::isfinite(p->pad)) return fail(h, F110_ERR_INVALID, "neighbors: pad must be finite");
    o = NbrSpec{};
    for (int b = 0; b < F110_NBR_NCHANNELS; ++b) {
        o.scale[b] = 1.0;
        if (!(p->channels >> b & 1)) continue;
        if (!(std::isfinite(p->scale[b]) && p->scale[b] != 0.0)) return fail(h, F110_ERR_INVALID, "neighbors: scale[%d] must be finite and non-zero", b);
        o.scale[b] = p->scale[b];
        o.D += 1;
    }
    o.K = p->k;
    o.KT = 1;
    while (o.KT < o.K) o.KT *= 2;
    o.channels = p->channels;
    o.R2 = p->max_range * p->max_range;
    o.pad = p->pad;
    return F110_OK;
}

static void nbr_launch(NbrJob &j, hipStream_t st)
{
    if (j.envs <= 0) return;
    j.shift = 0;
    while ((1 << j.shift) < j.A) ++j.shift;
    const dim3 grid = grid1d((size_t)j.envs, 256 >> j.shift), block(256);
    switch (j.sp.KT) {
    case 1: hipLaunchKernelGGL(k_neighbors<1>, grid, block, 0, st, j); break;
    case 2: hipLaunchKernelGGL(k_neighbors<2>, grid, block, 0, st, j); break;
    case 4: hipLaunchKernelGGL(k_neighbors<4>, grid, block, 0, st, j); break;
    default: hipLaunchKernelGGL(k_neighbors<8>, grid, block, 0, st, j); break;
    }
}

int f110_neighbors_device(f110_sim *h, const f110_neighbors *spec, float *d_out, float *h_pinned)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    NbrJob j{};
    TRY(nbr_check_spec(h, spec, j.sp));
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return fail(h, F110_ERR_INVALID, "neighbors: d_out is null or not 16-byte aligned");
    const size_t N = (size_t)h->N, per_agent = (size_t)j.sp.K * j.sp.D;
    if (h_pinned && !pinned_block_holds(h_pinned, N * per_agent * sizeof(float)))
        return fail(h, F110_ERR_INVALID, "neighbors: h_pinned is not [N][K][D] floats of f110_host_alloc memory");
    const bool gap = (j.sp.channels & F110_NBR_GAP_S) != 0;
    if (h->cfg.num_agents > F110_NBR_MAX_AGENTS) return fail(h, F110_ERR_STATE, "neighbors: %d agents per env, more than %d", h->cfg.num_agents, (int)F110_NBR_MAX_AGENTS);
    if (gap) {
        if (!h->track_on) return fail(h, F110_ERR_STATE, "neighbors: GAP_S is requested, but tracking is off (f110_track_enable)");
        TRY(tracks_in_use(h, "neighbors: GAP_S is requested"));
        TRY(tracks_current(h));
    }
    EnvBlocks w;   // behind a two-block step: each block's envs on the block's own stream (an agent reads its own env's rows and writes its own block)
    TRY(env_blocks_follow(h, w));
    j.tracks = gap ? h->d_tracks : nullptr;
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.A = h->cfg.num_agents;
    j.px = h->dev.snap_pose;   // the post-step pose of the observation, the one s was computed from
    j.py = h->dev.snap_pose + N;
    j.pth = h->dev.snap_pose + 2 * N;
    j.pv = h->dev.state + 3 * N;   // the live longitudinal speed (0 for an env re-seated inside the step)
    j.ps = gap ? h->d_trk : nullptr;
    j.stride = 1;
    j.unit_L = 0.0;
    j.out = d_out;
    return env_blocks_output(h, w, kPinnedNeighbors, per_agent, d_out, h_pinned, [&](const EnvBlock &b) {
        j.env0 = b.e0;
        j.envs = b.count;
        nbr_launch(j, b.stream);
    });
}

int f110_neighbors_batch(f110_sim *h, const f110_neighbors *spec, int32_t A, double track_L, const double *h_in, int32_t m, float *h_out,
                         double *h_raw, int32_t *h_idx)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    NbrJob j{};
    TRY(nbr_check_spec(h, spec, j.sp));
    if (A < 1 || A > F110_NBR_MAX_AGENTS) return fail(h, F110_ERR_INVALID, "neighbors: A = %d is outside 1..%d", A, (int)F110_NBR_MAX_AGENTS);
    if (!(track_L >= 0.0 && std::isfinite(track_L))) return fail(h, F110_ERR_INVALID, "neighbors: track_L must be finite and >= 0 (0: no wrap)");
    if (m < 0 || m % A != 0 || (m > 0 && (!h_in || !h_out))) return fail(h, F110_ERR_INVALID, "neighbors: bad argument (m must be a multiple of A)");
    if (m == 0) return F110_OK;
    ENTER(h);
    Scratch sc(h);
    const size_t slots = (size_t)m * j.sp.K;
    const double *din = sc.in(h_in, 5 * (size_t)m);
    j.out = sc.out(h_out, slots * j.sp.D);
    j.raw = sc.out(h_raw, slots * F110_NBR_NCHANNELS);
    j.idx = sc.out(h_idx, slots);
    TRY(sc.ready());
    j.A = A;
    j.env0 = 0;
    j.envs = m / A;
    j.px = din;
    j.py = din + 1;
    j.pth = din + 2;
    j.pv = din + 3;
    j.ps = din + 4;
    j.stride = 5;
    j.unit_L = track_L;
    nbr_launch(j, h->stream);
    return sc.finish();
}

// ---- scripted cars: line followers (f110_line_followers_set / f110_follow_line_*, include/f110.h) -----------------------------------
// the spec's refusals; on success the kernel's spec
static int line_check_spec(f110_sim *h, const f110_line_follower *p, LineSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "line follower: null spec");
    const double d[] = {p->look_base, p->look_gain, p->look_min, p->look_max, p->lane_offset, p->wheelbase, p->steer_max, p->v_const, p->vgain,
                        p->speed_look, p->lat_slow, p->v_recover, p->follow_range, p->follow_gap, p->follow_gain, p->lane_width, p->v_min, p->v_max};
    for (double x : d)
        if (!std::isfinite(x)) return fail(h, F110_ERR_INVALID, "line follower: every setting must be finite");
    if (!(p->look_min > 0) || p->look_min > p->look_max) return fail(h, F110_ERR_INVALID, "line follower: 0 < look_min <= look_max is required");
    if (p->look_base < 0 || p->look_gain < 0 || p->speed_look < 0) return fail(h, F110_ERR_INVALID, "line follower: look_base, look_gain and speed_look must be >= 0");
    if (!(p->wheelbase > 0)) return fail(h, F110_ERR_INVALID, "line follower: wheelbase must be > 0");
    if (p->steer_max < 0) return fail(h, F110_ERR_INVALID, "line follower: steer_max must be >= 0");
    if (p->v_min < 0 || p->v_min > p->v_max) return fail(h, F110_ERR_INVALID, "line follower: 0 <= v_min <= v_max is required");
    if (p->follow_range < 0 || p->lane_width < 0 || p->lat_slow < 0) return fail(h, F110_ERR_INVALID, "line follower: follow_range, lane_width and lat_slow must be >= 0");
    if (p->speed_attr < -1 || p->speed_attr >= F110_TRACK_MAX_ATTRS)
        return fail(h, F110_ERR_INVALID, "line follower: speed_attr = %d is outside -1..%d", p->speed_attr, (int)F110_TRACK_MAX_ATTRS - 1);
    o = LineSpec{};
    o.look_base = p->look_base, o.look_gain = p->look_gain, o.look_min = p->look_min, o.look_max = p->look_max;
    o.lane_offset = p->lane_offset, o.wheelbase = p->wheelbase, o.steer_max = p->steer_max;
    o.v_const = p->v_const, o.vgain = p->vgain, o.speed_look = p->speed_look, o.lat_slow = p->lat_slow, o.v_recover = p->v_recover;
    o.follow_range = p->follow_range, o.follow_gap = p->follow_gap, o.follow_gain = p->follow_gain, o.lane_width = p->lane_width;
    o.v_min = p->v_min, o.v_max = p->v_max;
    o.speed_attr = p->speed_attr;
    return F110_OK;
}

// what a slot must offer a spec: a track, the speed's attribute column, and on a closed track more length than the spec reaches
static int line_check_slot(f110_sim *h, const LineSpec &sp, int slot)
{
    if (!track_has(h, slot)) return fail(h, F110_ERR_STATE, "line follower: map slot %d has no track (f110_track_set)", slot);
    const f110_sim::TrackSlot &ts = h->tracks[slot];
    if (sp.speed_attr >= ts.nattr)
        return fail(h, F110_ERR_STATE, "line follower: speed_attr = %d, but the track on slot %d has %d attributes (f110_track_set_attrs)", sp.speed_attr, slot, ts.nattr);
    const double reach = std::max(sp.look_max, sp.speed_look);
    if (ts.closed && !(ts.L > reach))
        return fail(h, F110_ERR_STATE, "line follower: the closed track on slot %d is %.6g m long, not longer than the reach of %.6g m", slot, ts.L, reach);
    if (ts.closed && !(ts.L > 2.0 * sp.follow_range))
        return fail(h, F110_ERR_STATE, "line follower: the closed track on slot %d is %.6g m long, not longer than twice follow_range = %.6g m", slot, ts.L, sp.follow_range);
    return F110_OK;
}

// can the armed line followers run?  The refusals of a call, nothing launched.  The slot checks are remembered until the tracks,
// the env maps or the arming change.
static int line_ready(f110_sim *h)
{
    if (h->line_specs == 0) return fail(h, F110_ERR_STATE, "follow line: no line followers are armed (f110_line_followers_set)");
    if (!h->track_on) return fail(h, F110_ERR_STATE, "follow line: tracking is off (f110_track_enable)");
    if (h->line_checked) return F110_OK;
    const int A = h->cfg.num_agents, slots = 1 + (int)h->extra_maps.size();
    std::vector<char> seen((size_t)slots * LINE_MAX_SPECS, 0);
    for (size_t n = 0; n < h->line_assign_host.size(); ++n) {
        const int k = h->line_assign_host[n];
        if (k < 0) continue;
        const int slot = h->multi_map ? h->env_map_host[n / A] : 0;
        char &s = seen[(size_t)slot * LINE_MAX_SPECS + k];
        if (s) continue;
        TRY(line_check_slot(h, h->line_specs_host[k], slot));
        s = 1;
    }
    h->line_checked = true;
    return F110_OK;
}

static void line_launch(LineJob &j, hipStream_t st, bool follow)
{
    if (j.groups <= 0) return;
    j.shift = 0;
    while ((1 << j.shift) < j.GA) ++j.shift;
    const dim3 grid = grid1d((size_t)j.groups, 256 >> j.shift), block(256);
    if (follow) hipLaunchKernelGGL(k_follow_line<true>, grid, block, 0, st, j);
    else hipLaunchKernelGGL(k_follow_line<false>, grid, block, 0, st, j);
}

// the armed line followers over the agents of one env block, into d_actions [N][2] (and d_info [N][4] or null)
static void line_launch_armed(f110_sim *h, const EnvBlock &b, double *d_actions, double *d_info)
{
    const size_t N = (size_t)h->N;
    const int A = h->cfg.num_agents;
    LineJob j{};
    j.specs = h->d_line_specs;
    j.assign = h->d_line_assign;
    j.tracks = h->d_tracks;
    j.attrs = h->d_track_attrs;
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.A = A;
    j.unit_slot = -1;
    j.GA = h->line_follow ? A : 1;
    j.i0 = b.e0 * A;
    j.groups = h->line_follow ? b.count : b.count * A;
    j.stride = 1;
    j.px = h->dev.snap_pose;   // the post-step pose of the observation, the one s was computed from
    j.py = h->dev.snap_pose + N;
    j.pth = h->dev.snap_pose + 2 * N;
    j.pv = h->dev.state + 3 * N;   // the live longitudinal speed (0 for an env re-seated inside the step)
    j.ps = h->d_trk;
    j.plat = h->d_trk + 2 * N;
    j.cnt = h->dev.step_count;
    j.actions = d_actions;
    j.info = d_info;
    line_launch(j, b.stream, h->line_follow);
}

int f110_line_followers_set(f110_sim *h, const f110_line_follower *specs, int32_t n_specs, const int32_t *h_assign)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (n_specs == 0 && !specs && !h_assign) {   // disarm
        ENTER(h);
        h->line_specs = 0;
        h->line_follow = false;
        h->line_checked = false;
        h->line_assign_host.clear();
        h->d_line_specs.reset();   // (hipFree waits for the calls in flight that read them)
        h->d_line_assign.reset();
        return F110_OK;
    }
    if (!specs || !h_assign || n_specs < 1 || n_specs > F110_LINE_MAX_SPECS)
        return fail(h, F110_ERR_INVALID, "line followers: 1..%d specs and an assignment, or NULL, 0, NULL", (int)F110_LINE_MAX_SPECS);
    LineSpec ls[LINE_MAX_SPECS] = {};
    bool follow = false;
    for (int k = 0; k < n_specs; ++k) {
        TRY(line_check_spec(h, specs + k, ls[k]));
        follow = follow || (ls[k].follow_range > 0.0 && h->cfg.num_agents > 1);
    }
    const size_t N = (size_t)h->N;
    for (size_t i = 0; i < N; ++i) {
        if (h_assign[i] < -1 || h_assign[i] >= n_specs) return fail(h, F110_ERR_INVALID, "line followers: assignment[%zu] = %d is outside -1..%d", i, h_assign[i], n_specs - 1);
        if (h_assign[i] != -1 && !h->gap_assign_host.empty() && h->gap_assign_host[i] != -1)
            return fail(h, F110_ERR_INVALID, "line followers: agent %zu has a follow-the-gap controller (f110_controllers_set)", i);
    }
    for (int32_t n : h->mppi.on.agents)
        if (h_assign[n] != -1) return fail(h, F110_ERR_INVALID, "line followers: agent %d is driven by the armed planner (f110_mppi_set)", n);
    if (follow && h->cfg.num_agents > F110_LINE_MAX_AGENTS)
        return fail(h, F110_ERR_STATE, "line followers: follow_range > 0 with %d agents per env, more than %d", h->cfg.num_agents, (int)F110_LINE_MAX_AGENTS);
    ENTER(h);
    if (!h->d_line_specs) TRY(dmalloc(h, &h->d_line_specs, (size_t)LINE_MAX_SPECS));
    if (!h->d_line_assign) TRY(dmalloc(h, &h->d_line_assign, N));
    HIPCHK(h, hipMemcpyAsync(h->d_line_specs, ls, sizeof(LineSpec) * n_specs, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->d_line_assign, h_assign, sizeof(int32_t) * N, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (the sources are the caller's and this function's stack)
    h->line_specs = n_specs;
    h->line_follow = follow;
    h->line_checked = false;
    std::copy(ls, ls + LINE_MAX_SPECS, h->line_specs_host);
    h->line_assign_host.assign(h_assign, h_assign + N);
    return F110_OK;
}

int f110_follow_line_device(f110_sim *h, double *d_actions, double *d_info)
{
    if (!h || !d_actions) return fail(h, F110_ERR_INVALID, "follow line: null argument");
    if (reinterpret_cast<uintptr_t>(d_actions) % 16 != 0 || reinterpret_cast<uintptr_t>(d_info) % 16 != 0)
        return fail(h, F110_ERR_INVALID, "follow line: the actions or the info buffer is not 16-byte aligned");
    TRY(line_ready(h));
    TRY(tracks_current(h));   // (tracks or attributes set since the last step)
    EnvBlocks w;   // behind a two-block step: each block's envs on the block's own stream (an agent reads its own env's rows and writes its own)
    TRY(env_blocks_follow(h, w));
    for (const EnvBlock &b : w) line_launch_armed(h, b, d_actions, d_info);
    HIPCHK(h, hipGetLastError());
    h->touched = false;
    return F110_OK;
}

int f110_follow_line_batch(f110_sim *h, const f110_line_follower *spec, int32_t slot, int32_t A, const double *h_in, int32_t m, double *h_actions,
                           double *h_raw)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    LineSpec ls;
    TRY(line_check_spec(h, spec, ls));
    if (A < 1 || A > F110_LINE_MAX_AGENTS) return fail(h, F110_ERR_INVALID, "follow line: A = %d is outside 1..%d", A, (int)F110_LINE_MAX_AGENTS);
    if (m < 0 || m % A != 0 || (m > 0 && (!h_in || !h_actions))) return fail(h, F110_ERR_INVALID, "follow line: bad argument (m must be a multiple of A)");
    TRY(line_check_slot(h, ls, slot));
    if (m == 0) return F110_OK;
    ENTER(h);
    TRY(track_upload(h));
    Scratch sc(h);
    const bool follow = ls.follow_range > 0.0 && A > 1;
    LineJob j{};
    j.specs = sc.in(&ls, 1);
    const double *din = sc.in(h_in, 7 * (size_t)m);
    j.actions = sc.out(h_actions, 2 * (size_t)m);
    j.raw = sc.out(h_raw, (size_t)LINE_NRAW * m);
    TRY(sc.ready());
    j.tracks = h->d_tracks;
    j.attrs = h->d_track_attrs;
    j.A = A;
    j.unit_slot = slot;
    j.GA = follow ? A : 1;
    j.groups = follow ? m / A : m;
    j.stride = 7;
    j.px = din;
    j.py = din + 1;
    j.pth = din + 2;
    j.pv = din + 3;
    j.ps = din + 4;
    j.plat = din + 5;
    j.cnt_f = din + 6;
    line_launch(j, h->stream, follow);
    return sc.finish();
}

// ---- rendering --------------------------------------------------------------------------------------------------------------
// rendering.py's clear colour (OUTSIDE, FREE), its map points and waypoint_follow.py's waypoints (WALL, TRACK), then SCAN, CAR, SELF
static const uint8_t kDefaultPalette[F110_NCLASSES * 3] = {9, 32, 87, 9, 32, 87, 183, 193, 222, 183, 193, 222, 255, 190, 0, 99, 52, 94, 172, 97, 185};

// the occupancy grid of a slot's table, built the first time a render reads the slot
static int render_occ(f110_sim *h, const ScanConst &k, DevBuf<uint8_t> *occ, bool *stale)
{
    if (*occ && !(stale && *stale)) return F110_OK;
    const size_t n = (size_t)k.height * k.width;
    if (!*occ) TRY(dmalloc(h, occ, n));
    if (stale) *stale = false;
    hipLaunchKernelGGL(k_render_occ, grid1d(n, 256), dim3(256), 0, h->stream, k.table, k.row_bytes, k.height, k.width, occ->get());
    HIPCHK(h, hipGetLastError());
    return F110_OK;
}

int f110_render_device(f110_sim *h, const f110_render_spec *spec, const int32_t *h_agents, int32_t n_frames, uint8_t *d_classes,
                       uint8_t *d_rgb, const uint8_t *h_palette)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    if (!spec || !d_classes) return fail(h, F110_ERR_INVALID, "f110_render_device: spec and d_classes are required");
    const f110_render_spec sp = *spec;
    const int W = sp.width, H = sp.height, N = h->N, A = h->cfg.num_agents;
    if (W < 1 || W > 4096 || H < 1 || H > 4096) return fail(h, F110_ERR_INVALID, "f110_render_device: width and height must be in 1..4096 (got %d x %d)", W, H);
    if (!(std::isfinite(sp.m_per_px) && sp.m_per_px > 0)) return fail(h, F110_ERR_INVALID, "f110_render_device: m_per_px must be finite and > 0");
    if (sp.view < F110_VIEW_WORLD || sp.view > F110_VIEW_EGO) return fail(h, F110_ERR_INVALID, "f110_render_device: unknown view %d", sp.view);
    if (sp.layers & ~F110_LAYER_ALL) return fail(h, F110_ERR_INVALID, "f110_render_device: unknown layer bits 0x%x", sp.layers);
    if (n_frames < 1) return fail(h, F110_ERR_INVALID, "f110_render_device: n_frames = %d", n_frames);
    if (!h_agents && n_frames != N) return fail(h, F110_ERR_INVALID, "f110_render_device: without an agent list n_frames must be N = %d (got %d)", N, n_frames);
    if (h_agents)
        for (int f = 0; f < n_frames; ++f)
            if (h_agents[f] < 0 || h_agents[f] >= N) return fail(h, F110_ERR_INVALID, "f110_render_device: frame %d: agent %d is outside [0, %d)", f, h_agents[f], N);
    if ((unsigned long long)n_frames * (unsigned long long)H * (unsigned long long)W > (1ull << 31))
        return fail(h, F110_ERR_INVALID, "f110_render_device: %d frames of %d x %d pixels exceed 2^31", n_frames, H, W);
    if (sp.view == F110_VIEW_WORLD && !(std::isfinite(sp.center_x) && std::isfinite(sp.center_y) && std::isfinite(sp.angle)))
        return fail(h, F110_ERR_INVALID, "f110_render_device: the WORLD camera needs a finite centre and angle");
    if (sp.view != F110_VIEW_WORLD && !std::isfinite(sp.fwd_offset)) return fail(h, F110_ERR_INVALID, "f110_render_device: fwd_offset is not finite");
    ENTER(h);
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    const int F = n_frames;
    const int slots = 1 + (int)h->extra_maps.size();
    // the slot table: the map fields, the occupancy grid when MAP is drawn, the track points
    std::vector<RenderSlot> rs((size_t)slots);
    for (int m = 0; m < slots; ++m) {
        const ScanConst &k = m == 0 ? h->k : h->extra_maps[m - 1].k;
        RenderSlot &r = rs[m];
        r = RenderSlot{};
        if (sp.layers & F110_LAYER_MAP) TRY(render_occ(h, k, m == 0 ? &h->d_occ0 : &h->extra_maps[m - 1].d_occ, m == 0 ? nullptr : &h->extra_maps[m - 1].occ_stale));
        r.occ = m == 0 ? h->d_occ0.get() : h->extra_maps[m - 1].d_occ.get();
        if ((sp.layers & F110_LAYER_TRACK) && m < (int)h->tracks.size() && h->tracks[m].d_pts) {
            r.pts = h->tracks[m].d_pts;
            r.npts = h->tracks[m].npts;
        }
        r.height = k.height;
        r.width = k.width;
        r.res = k.res;
        r.inv_res = k.inv_res;
        r.orig_x = k.orig_x;
        r.orig_y = k.orig_y;
        r.orig_c = k.orig_c;
        r.orig_s = k.orig_s;
        r.w_res = k.w_res;
        r.h_res = k.h_res;
    }
    if (h->render_slots.size() != rs.size() || std::memcmp(h->render_slots.data(), rs.data(), rs.size() * sizeof(RenderSlot)) != 0) {
        TRY(dgrow(h, h->d_render_slots, rs.size()));
        h->render_slots = rs;   // (a pageable source: consumed before the call returns)
        HIPCHK(h, hipMemcpyAsync(h->d_render_slots, h->render_slots.data(), rs.size() * sizeof(RenderSlot), hipMemcpyHostToDevice, h->stream));
    }
    TRY(dgrow(h, h->d_render_frames, (size_t)F));
    if (!h->d_render_cars) TRY(dmalloc(h, &h->d_render_cars, (size_t)N));
    if (h_agents) {
        TRY(dgrow(h, h->d_render_agents, (size_t)F));
        HIPCHK(h, hipMemcpyAsync(h->d_render_agents, h_agents, (size_t)F * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    }
    // 32-bit stores straight into the caller's buffer when its rows allow them, else into an aligned copy with padded rows
    const bool direct = (W % 4 == 0) && (reinterpret_cast<uintptr_t>(d_classes) % 4 == 0);
    const int pitch = (W + 3) & ~3;
    uint8_t *target = d_classes;
    if (!direct) {
        TRY(dgrow(h, h->d_render_stage, (size_t)F * H * pitch));
        target = h->d_render_stage;
    }
    RenderJob j{};
    j.snap = h->dev.snap_pose;
    j.params = h->dev.params;
    j.params_per_agent = h->dev.params_per_agent;
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.slots = h->d_render_slots;
    j.agents = h_agents ? h->d_render_agents : nullptr;
    j.frames = h->d_render_frames;
    j.cars = h->d_render_cars;
    j.cls = target;
    j.scans = h->dev.scans;
    j.F = F;
    j.N = N;
    j.A = A;
    j.W = W;
    j.H = H;
    j.pitch = pitch;
    j.view = sp.view;
    j.layers = sp.layers;
    j.B = h->cfg.num_beams;
    j.words_per_frame = (uint32_t)(pitch / 4) * (uint32_t)H;
    j.blocks_per_frame = (j.words_per_frame + 255) / 256;
    j.mpp = sp.m_per_px;
    j.center_x = sp.center_x;
    j.center_y = sp.center_y;
    j.angle = sp.angle;
    j.fwd = sp.fwd_offset;
    j.car_len = sp.car_length;
    j.car_wid = sp.car_width;
    j.lidar_dist = h->cfg.lidar_dist;
    j.cull_r = (0.5 * std::hypot((double)W, (double)H) + 1.0) * sp.m_per_px * 1.01;
    hipLaunchKernelGGL(k_render_setup, grid1d((size_t)std::max(F, N), 256), dim3(256), 0, h->stream, j);
    hipLaunchKernelGGL(k_render_raster, dim3((unsigned)((size_t)F * j.blocks_per_frame)), dim3(256), 0, h->stream, j);
    HIPCHK(h, hipGetLastError());
    if (sp.layers & F110_LAYER_TRACK) {
        uint32_t most = 0;
        for (const RenderSlot &r : rs) most = std::max(most, (uint32_t)r.npts);
        if (most > 0) hipLaunchKernelGGL(k_render_points<false>, grid1d((size_t)F * most, 256), dim3(256), 0, h->stream, j, h->k, most);
    }
    if (sp.layers & F110_LAYER_SCAN)
        hipLaunchKernelGGL(k_render_points<true>, grid1d((size_t)F * j.B, 256), dim3(256), 0, h->stream, j, h->k, (uint32_t)j.B);
    HIPCHK(h, hipGetLastError());
    if (!direct || d_rgb) {
        RenderPalette pal{};
        std::memcpy(pal.rgb, h_palette ? h_palette : kDefaultPalette, sizeof pal.rgb);
        const size_t total = (size_t)F * H * W;
        hipLaunchKernelGGL(k_render_finish, grid1d(total, 256), dim3(256), 0, h->stream, target, direct ? W : pitch, W, H, total,
                           direct ? nullptr : d_classes, d_rgb, pal);
        HIPCHK(h, hipGetLastError());
    }
    return F110_OK;
}

// ---- where the rollout's and the planner's candidates start (RollJob and MppiJob name these fields alike) ------------------------------
template <typename Job>
static void job_step_consts(const f110_sim *h, Job &j)
{
    j.integrator = h->dev.integrator;
    j.time_step = h->dev.time_step;
    j.lidar_dist = h->dev.lidar_dist;
}

// the live source: every agent's state, FIFO and parameter row, its env's map and (track) track
template <typename Job>
static int job_live_source(f110_sim *h, const char *who, bool track, Job &j)
{
    j.maps = h->multi_map ? h->d_maps_full : cold_consts(h);
    if (!j.maps) return fail(h, F110_ERR_HIP, "%s: constant upload failed", who);
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.tracks = track ? h->d_tracks : nullptr;
    j.unit_slot = -1;
    j.A = h->cfg.num_agents;
    j.N = h->N;
    j.params_per_agent = h->dev.params_per_agent;
    j.state = h->dev.state;
    j.steer_buf = h->dev.steer_buf;
    j.buf_cnt = h->dev.buf_cnt;
    j.params = h->dev.params;
    job_step_consts(h, j);
    return F110_OK;
}

// the unit source: the caller's m start rows [m][10] on one map slot, kept here until the call has synchronised
struct UnitRows {
    std::vector<double> cols;    // as the live columns are laid out: state [7][m], the FIFO [2][m]
    std::vector<int32_t> cnt;    // the FIFO's fill [m]
    ScanConst kc{};              // the slot's constants
};

static int unit_slot_check(f110_sim *h, const char *who, int slot)
{
    if (slot < 0 || slot > (int)h->extra_maps.size()) return fail(h, F110_ERR_INVALID, "%s: map slot %d, but %d maps are registered", who, slot, 1 + (int)h->extra_maps.size());
    return F110_OK;
}

// the rows into columns; refuses a fill count other than 0, 1, 2.  Host memory only: nothing is enqueued.
static int unit_rows(f110_sim *h, const char *who, const double *h_start, size_t M, UnitRows &u)
{
    u.cols.resize(9 * M);
    u.cnt.resize(M);
    for (size_t r = 0; r < M; ++r) {
        for (int c = 0; c < 9; ++c) u.cols[(size_t)c * M + r] = h_start[10 * r + c];
        const double f = h_start[10 * r + 9];
        if (!(f == 0.0 || f == 1.0 || f == 2.0)) return fail(h, F110_ERR_INVALID, "%s: row %zu has a FIFO fill count of %g, not 0, 1 or 2", who, r, f);
        u.cnt[r] = (int32_t)f;
    }
    return F110_OK;
}

// the columns, the slot's constants and the parameter rows (none: the handle's row of agent slot 0) into scratch memory, and the job's view of them
template <typename Job>
static int job_unit_source(f110_sim *h, Scratch &sc, int slot, bool track, UnitRows &u, const double *h_params, Job &j)
{
    const size_t M = u.cnt.size();
    u.kc = slot_consts(h, slot);
    double *dcols = sc.in(u.cols.data(), u.cols.size());
    j.buf_cnt = sc.in(u.cnt.data(), u.cnt.size());
    j.maps = sc.in(&u.kc, 1);
    j.params = h_params ? sc.in(h_params, M * NPARAMS) : h->d_params;
    TRY(sc.ready());
    j.tracks = track ? h->d_tracks : nullptr;
    j.unit_slot = slot;
    j.A = 1;
    j.count = (int)M;
    j.N = (int)M;
    j.params_per_agent = h_params ? 1 : 0;
    j.state = dcols;
    j.steer_buf = dcols + 7 * M;
    job_step_consts(h, j);
    return F110_OK;
}

// ---- rollout (f110_rollout_*, include/f110.h) ---------------------------------------------------------------------------------------
// the spec's refusals; on success the kernel's spec
static int roll_check_spec(f110_sim *h, const f110_rollout *p, RollSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "rollout: null spec");
    if (p->k < 1 || p->k > F110_ROLL_MAX_K) return fail(h, F110_ERR_INVALID, "rollout: k = %d is outside 1..%d", p->k, (int)F110_ROLL_MAX_K);
    if (p->horizon < 1 || p->horizon > F110_ROLL_MAX_H) return fail(h, F110_ERR_INVALID, "rollout: horizon = %d is outside 1..%d", p->horizon, (int)F110_ROLL_MAX_H);
    if (p->repeat < 1 || p->repeat > F110_ROLL_MAX_REPEAT) return fail(h, F110_ERR_INVALID, "rollout: repeat = %d is outside 1..%d", p->repeat, (int)F110_ROLL_MAX_REPEAT);
    if (p->layout != F110_ROLL_SHARED && p->layout != F110_ROLL_PER_AGENT) return fail(h, F110_ERR_INVALID, "rollout: unknown layout %d", p->layout);
    if (p->frame != F110_ROLL_FRAME_EGO && p->frame != F110_ROLL_FRAME_MAP) return fail(h, F110_ERR_INVALID, "rollout: unknown frame %d", p->frame);
    if (p->channels == 0 || (p->channels & ~((1 << F110_ROLL_NCHANNELS) - 1))) return fail(h, F110_ERR_INVALID, "rollout: channels = 0x%x is empty or has an unknown bit", p->channels);
    if (p->traj != 0 && p->traj != 1) return fail(h, F110_ERR_INVALID, "rollout: traj = %d must be 0 or 1", p->traj);
    if (p->margin != p->margin) return fail(h, F110_ERR_INVALID, "rollout: margin is NaN");
    o = RollSpec{};
    for (int b = 0; b < F110_ROLL_NCHANNELS; ++b) {
        o.scale[b] = 1.0;
        const bool set = (p->channels >> b & 1) != 0;
        if (set) o.D += 1;
        if (!set && !(p->traj && b < 4)) continue;
        if (!(std::isfinite(p->scale[b]) && p->scale[b] > 0.0)) return fail(h, F110_ERR_INVALID, "rollout: scale[%d] must be finite and > 0", b);
        o.scale[b] = p->scale[b];
    }
    o.K = p->k;
    o.H = p->horizon;
    o.repeat = p->repeat;
    o.layout = p->layout;
    o.frame = p->frame;
    o.channels = p->channels;
    o.traj = p->traj;
    o.margin = p->margin;
    return F110_OK;
}

// agents [j.begin, j.begin + j.count): the candidates, then (track set) the two projections behind them on the same stream
static void roll_launch(const RollJob &j, bool track, hipStream_t st, const OppLane *opp = nullptr)
{
    if (j.count <= 0) return;
    const size_t lanes = (size_t)j.count * j.sp.K;
    const dim3 grid = grid1d(lanes, 256), block(256);
    const bool uni = j.sp.K % 64 == 0;
    if (opp) {   // the same lanes with the opponent term's sampling (its predictions are on `st` already)
        if (j.sp.traj) {
            if (uni) hipLaunchKernelGGL((k_rollout_opp<true, true>), grid, block, 0, st, j, *opp);
            else hipLaunchKernelGGL((k_rollout_opp<false, true>), grid, block, 0, st, j, *opp);
        } else {
            if (uni) hipLaunchKernelGGL((k_rollout_opp<true, false>), grid, block, 0, st, j, *opp);
            else hipLaunchKernelGGL((k_rollout_opp<false, false>), grid, block, 0, st, j, *opp);
        }
    } else if (j.sp.traj) {
        if (uni) hipLaunchKernelGGL((k_rollout<true, true>), grid, block, 0, st, j);
        else hipLaunchKernelGGL((k_rollout<false, true>), grid, block, 0, st, j);
    } else {
        if (uni) hipLaunchKernelGGL((k_rollout<true, false>), grid, block, 0, st, j);
        else hipLaunchKernelGGL((k_rollout<false, false>), grid, block, 0, st, j);
    }
    if (track) hipLaunchKernelGGL(k_rollout_track, grid1d(lanes * kTrackLanes, 256), block, 0, st, j);
}

int f110_rollout_device(f110_sim *h, const f110_rollout *spec, const double *d_actions, float *d_out, float *d_traj, float *h_pinned)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    RollJob j{};
    TRY(roll_check_spec(h, spec, j.sp));
    if (!d_actions || !d_out) return fail(h, F110_ERR_INVALID, "rollout: d_actions or d_out is null");
    if (j.sp.traj && (!d_traj || reinterpret_cast<uintptr_t>(d_traj) % 16 != 0)) return fail(h, F110_ERR_INVALID, "rollout: traj = 1, but d_traj is null or not 16-byte aligned");
    const size_t N = (size_t)h->N, per_agent = (size_t)j.sp.K * j.sp.D;
    if (N * j.sp.K >= (size_t)1 << 31) return fail(h, F110_ERR_INVALID, "rollout: %zu agents x %d candidates do not fit 31 bits", N, j.sp.K);
    if (h_pinned && !pinned_block_holds(h_pinned, N * per_agent * sizeof(float)))
        return fail(h, F110_ERR_INVALID, "rollout: h_pinned is not [N][K][D] floats of f110_host_alloc memory");
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    const bool track = (j.sp.channels & kRollTrackBits) != 0;
    if (track) {
        TRY(tracks_in_use(h, "rollout: PROGRESS or END_LAT is requested"));
        TRY(tracks_current(h));
        if (h->d_roll_end.capacity() < 2 * N * j.sp.K) {
            ENTER(h);
            TRY(dgrow(h, h->d_roll_end, 2 * N * j.sp.K));
        }
    }
    EnvBlocks w;   // behind a two-block step: each block's agents on the block's own stream (a candidate reads its own agent's rows and writes its own)
    TRY(env_blocks_follow(h, w));
    TRY(job_live_source(h, "rollout", track, j));
    j.actions = d_actions;
    j.out = d_out;
    j.traj = j.sp.traj ? d_traj : nullptr;
    j.end_xy = track ? h->d_roll_end.get() : nullptr;
    return env_blocks_output(h, w, kPinnedRollout, per_agent, d_out, h_pinned, [&](const EnvBlock &b) {
        j.begin = b.e0 * j.A;
        j.count = b.count * j.A;
        roll_launch(j, track, b.stream);
    });
}

// ---- opponents (f110_rollout_opp_*, f110_mppi_set_opponents, f110_mppi_opp_batch; include/f110.h) -------------------------------------
// the settings' refusals; on success the kernels' settings (the planner's weights 0.0)
static int opp_check_spec(f110_sim *h, const char *who, const f110_opponents *p, OppSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "%s: null opponents", who);
    if (p->mode != F110_OPP_CV && p->mode != F110_OPP_TRACK) return fail(h, F110_ERR_INVALID, "%s: unknown opponents mode %d", who, p->mode);
    if (!(std::isfinite(p->radius) && p->radius > 0.0)) return fail(h, F110_ERR_INVALID, "%s: the opponents' radius must be finite and > 0", who);
    if (!(p->max_range > 0.0)) return fail(h, F110_ERR_INVALID, "%s: the opponents' max_range must be > 0 and not NaN", who);
    o = OppSpec{};
    o.mode = p->mode;
    o.radius = p->radius;
    o.max_range = p->max_range;
    return F110_OK;
}

static int opp_check_weights(f110_sim *h, double w_hit, double w_near, double near_ref, OppSpec &o)
{
    if (!(std::isfinite(w_hit) && w_hit >= 0.0) || !(std::isfinite(w_near) && w_near >= 0.0))
        return fail(h, F110_ERR_INVALID, "mppi: w_hit and w_near must be finite and >= 0");
    if (!std::isfinite(near_ref)) return fail(h, F110_ERR_INVALID, "mppi: near_ref must be finite");
    o.w_hit = w_hit;
    o.w_near = w_near;
    o.near_ref = near_ref;
    return F110_OK;
}

// what a unit form adds for the opponent term: the settings, the caller's opponent rows and its three outputs
struct OppUnit {
    OppSpec sp;
    const double *h_rows;   // [m][Ao][4]
    int Ao;
    double *h_pred;         // [m][Ao][H][2] or null
    double *h_raw;          // [m][K][2] or null
    float *h_out;           // [m][K][2] or null
};

static int opp_unit_check(f110_sim *h, const char *who, const OppUnit &u, int m, int slot)
{
    if (u.Ao < 0 || u.Ao > OPP_MAX) return fail(h, F110_ERR_INVALID, "%s: %d opponents per row are outside 0..%d", who, u.Ao, (int)OPP_MAX);
    if (m > 0 && u.Ao > 0 && !u.h_rows) return fail(h, F110_ERR_INVALID, "%s: h_opp_rows is null", who);
    if (u.sp.mode == OPP_TRACK && h->has_map && slot >= 0 && slot <= (int)h->extra_maps.size() && !track_has(h, slot))
        return fail(h, F110_ERR_STATE, "%s: the opponents follow the track, but map slot %d has no track (f110_track_set)", who, slot);
    return F110_OK;
}

// the predictions of rows [r0, r0 + count) of a rollout's or a planner's job into `table`, on `st`
template <typename Job>
static void opp_predict_launch(const f110_sim *h, const Job &j, const OppSpec &sp, int H, int repeat, int r0, int count, int Ao, const int32_t *agents,
                               const double *d_rows, OppSpec *sp_out, double *table, hipStream_t st)
{
    if (count <= 0 || Ao <= 0) return;
    OppJob o{};
    o.tracks = h->d_tracks.get();
    o.env_map = j.env_map;
    o.unit_slot = j.unit_slot;
    o.A = j.A;
    o.r0 = r0;
    o.count = count;
    o.N = j.N;
    o.Ao = Ao;
    o.agents = agents;
    o.state = j.state;
    o.opp_rows = d_rows;
    o.H = H;
    o.repeat = repeat;
    o.time_step = j.time_step;
    o.sp_out = sp_out;
    o.table = table;
    o.sp = sp;
    hipLaunchKernelGGL(k_opp_predict, grid1d((size_t)count * Ao * kTrackLanes, 256), dim3(256), 0, st, o);
}

// a unit form's side of the term: the opponent rows, the settings and the buffers into scratch memory, the predictions on the
// handle's stream, the lanes' view, and what of it the caller asked back
template <typename Job>
static int opp_unit_prepare(f110_sim *h, Scratch &sc, const Job &j, const OppUnit &u, int K, int H, int repeat, OppLane &lane)
{
    const size_t M = (size_t)j.count;
    const OppSpec *dspec = sc.in(&u.sp, 1);
    const double *drows = u.Ao > 0 ? sc.in(u.h_rows, M * u.Ao * 4) : nullptr;
    double *dtable = u.Ao > 0 ? sc.tmp<double>(M * u.Ao * H * 2) : nullptr;
    double *draw = sc.tmp<double>(M * K * 2);
    float *dout = sc.tmp<float>(M * K * 2);
    TRY(sc.ready());
    opp_predict_launch(h, j, u.sp, H, repeat, 0, (int)M, u.Ao, nullptr, drows, nullptr, dtable, h->stream);
    lane = OppLane{dtable, dspec, dout, draw, u.Ao, 0};
    sc.later(u.h_pred, dtable, M * u.Ao * H * 2);
    sc.later(u.h_raw, draw, M * K * 2);
    sc.later(u.h_out, dout, M * K * 2);
    return F110_OK;
}

// f110_rollout_batch, and with `ou` f110_rollout_opp_batch
static int roll_batch(f110_sim *h, const f110_rollout *spec, int32_t slot, const double *h_start, const double *h_params, const double *h_actions,
                      int32_t m, float *h_out, double *h_raw, float *h_traj, double *h_traj_raw, const OppUnit *ou)
{
    RollJob j{};
    TRY(roll_check_spec(h, spec, j.sp));
    if (m < 0 || (m > 0 && (!h_start || !h_actions || !h_out))) return fail(h, F110_ERR_INVALID, "rollout: bad argument");
    if (ou) TRY(opp_unit_check(h, "rollout", *ou, m, slot));
    if (j.sp.traj && m > 0 && !h_traj) return fail(h, F110_ERR_INVALID, "rollout: traj = 1, but h_traj is null");
    if ((size_t)m * j.sp.K >= (size_t)1 << 31) return fail(h, F110_ERR_INVALID, "rollout: %d rows x %d candidates do not fit 31 bits", m, j.sp.K);
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    TRY(unit_slot_check(h, "rollout", slot));
    const bool want_track = (j.sp.channels & kRollTrackBits) != 0;
    if (want_track && !track_has(h, slot)) return fail(h, F110_ERR_STATE, "rollout: PROGRESS or END_LAT is requested, but map slot %d has no track (f110_track_set)", slot);
    const bool track = want_track || (h_raw && track_has(h, slot));
    if (m == 0) return F110_OK;
    const size_t M = (size_t)m, cands = M * j.sp.K, steps = cands * j.sp.H;
    UnitRows rows;
    TRY(unit_rows(h, "rollout", h_start, M, rows));
    ENTER(h);
    if (track || (ou && ou->sp.mode == OPP_TRACK)) TRY(track_upload(h));
    Scratch sc(h);
    TRY(job_unit_source(h, sc, slot, track, rows, h_params, j));
    j.actions = sc.in(h_actions, (j.sp.layout == F110_ROLL_PER_AGENT ? steps : (size_t)j.sp.K * j.sp.H) * 2);
    j.out = sc.out(h_out, cands * j.sp.D);
    j.raw = sc.out(h_raw, cands * F110_ROLL_NCHANNELS);
    j.traj = j.sp.traj ? sc.out(h_traj, steps * 4) : nullptr;
    j.traj_raw = j.sp.traj ? sc.out(h_traj_raw, steps * 4) : nullptr;
    j.end_xy = track ? sc.tmp<double>(cands * 2) : nullptr;
    TRY(sc.ready());
    if (j.raw) HIPCHK(h, hipMemsetAsync(j.raw, 0, cands * F110_ROLL_NCHANNELS * sizeof(double), h->stream));
    OppLane lane{};
    if (ou) TRY(opp_unit_prepare(h, sc, j, *ou, j.sp.K, j.sp.H, j.sp.repeat, lane));
    roll_launch(j, track, h->stream, ou ? &lane : nullptr);
    return sc.finish();
}

int f110_rollout_batch(f110_sim *h, const f110_rollout *spec, int32_t slot, const double *h_start, const double *h_params, const double *h_actions,
                       int32_t m, float *h_out, double *h_raw, float *h_traj, double *h_traj_raw)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    return roll_batch(h, spec, slot, h_start, h_params, h_actions, m, h_out, h_raw, h_traj, h_traj_raw, nullptr);
}

int f110_rollout_opp_batch(f110_sim *h, const f110_rollout *spec, const f110_opponents *opp, int32_t slot, const double *h_start, const double *h_params,
                           const double *h_actions, const double *h_opp_rows, int32_t Ao, int32_t m, float *h_out, double *h_raw, float *h_traj,
                           double *h_traj_raw, double *h_pred, double *h_opp_raw, float *h_opp)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    OppUnit u{};
    TRY(opp_check_spec(h, "rollout", opp, u.sp));
    u.h_rows = h_opp_rows;
    u.Ao = Ao;
    u.h_pred = h_pred;
    u.h_raw = h_opp_raw;
    u.h_out = h_opp;
    return roll_batch(h, spec, slot, h_start, h_params, h_actions, m, h_out, h_raw, h_traj, h_traj_raw, &u);
}

int f110_rollout_opp_device(f110_sim *h, const f110_rollout *spec, const f110_opponents *opp, const double *d_actions, float *d_out, float *d_traj,
                            float *d_opp, float *h_pinned)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    RollJob j{};
    OppSpec os;
    TRY(roll_check_spec(h, spec, j.sp));
    TRY(opp_check_spec(h, "rollout", opp, os));
    if (!d_actions || !d_out || !d_opp) return fail(h, F110_ERR_INVALID, "rollout: d_actions, d_out or d_opp is null");
    if (j.sp.traj && (!d_traj || reinterpret_cast<uintptr_t>(d_traj) % 16 != 0)) return fail(h, F110_ERR_INVALID, "rollout: traj = 1, but d_traj is null or not 16-byte aligned");
    const size_t N = (size_t)h->N, per_agent = (size_t)j.sp.K * j.sp.D;
    if (N * j.sp.K >= (size_t)1 << 31) return fail(h, F110_ERR_INVALID, "rollout: %zu agents x %d candidates do not fit 31 bits", N, j.sp.K);
    if (h_pinned && !pinned_block_holds(h_pinned, N * per_agent * sizeof(float)))
        return fail(h, F110_ERR_INVALID, "rollout: h_pinned is not [N][K][D] floats of f110_host_alloc memory");
    if (!h->has_map) return fail(h, F110_ERR_NO_MAP, "Map is not set for scan simulator.");
    const bool track = (j.sp.channels & kRollTrackBits) != 0, opp_track = os.mode == OPP_TRACK;
    const int Ao = h->cfg.num_agents - 1;
    if (Ao > OPP_MAX) return fail(h, F110_ERR_INVALID, "rollout: %d opponents per agent, at most %d", Ao, (int)OPP_MAX);
    if (track) TRY(tracks_in_use(h, "rollout: PROGRESS or END_LAT is requested"));
    if (opp_track) TRY(tracks_in_use(h, "rollout: the opponents follow the track"));
    if (track || opp_track) TRY(tracks_current(h));
    const size_t table = N * (size_t)Ao * j.sp.H * 2;
    if ((track && h->d_roll_end.capacity() < 2 * N * j.sp.K) || h->d_roll_opp.capacity() < table || !h->d_roll_opp_spec) {
        ENTER(h);
        if (track) TRY(dgrow(h, h->d_roll_end, 2 * N * j.sp.K));
        if (table > 0) TRY(dgrow(h, h->d_roll_opp, table));
        TRY(dgrow(h, h->d_roll_opp_spec, (size_t)kMaxEnvBlocks));
    }
    EnvBlocks w;   // as f110_rollout_device; an env's cars are in one block, so a block's predictions read the block's own agents
    TRY(env_blocks_follow(h, w));
    TRY(job_live_source(h, "rollout", track, j));
    j.actions = d_actions;
    j.out = d_out;
    j.traj = j.sp.traj ? d_traj : nullptr;
    j.end_xy = track ? h->d_roll_end.get() : nullptr;
    return env_blocks_output(h, w, kPinnedRollout, per_agent, d_out, h_pinned, [&](const EnvBlock &b) {
        j.begin = b.e0 * j.A;
        j.count = b.count * j.A;
        // the block's own copy of the settings, written by its prediction kernel on its own stream.  Without opponents (one car per
        // env) nothing is predicted and no lane reads the settings.
        OppSpec *spec_b = h->d_roll_opp_spec.get() + (&b - w.begin());
        opp_predict_launch(h, j, os, j.sp.H, j.sp.repeat, j.begin, j.count, Ao, nullptr, nullptr, spec_b, h->d_roll_opp.get(), b.stream);
        const OppLane lane{h->d_roll_opp.get(), spec_b, d_opp, nullptr, Ao, 0};
        roll_launch(j, track, b.stream, &lane);
    });
}

// ---- the armed list (ArmedList): what f110_mppi_* and f110_pf_* share; `who` is "mppi" / "pf" -----------------------------------------
// the arguments of f110_<who>_set: all present arms (F110_OK), anything less is refused, but for the disarm form: kArmedDisarm, and
// the handle is entered for the caller to drop its feature (hipFree waits for the calls in flight that read its memory)
constexpr int kArmedDisarm = 1;
static int armed_form(f110_sim *h, const char *who, const void *spec, const int32_t *h_agents, int32_t m, const uint64_t *h_streams)
{
    if (spec && h_agents && h_streams) return F110_OK;
    if (spec || h_agents || m != 0 || h_streams) return fail(h, F110_ERR_INVALID, "%s: a spec, the agents and their streams, or NULL, NULL, 0, NULL", who);
    ENTER(h);
    return kArmedDisarm;
}

// the list's refusals, the first bad index decides: 1 .. N indices within 0 .. N - 1, strictly ascending, and with `drives` (the planner's) none with a controller
static int armed_check_list(f110_sim *h, const char *who, const int32_t *h_agents, int32_t m, bool drives)
{
    if (m < 1 || m > h->N) return fail(h, F110_ERR_INVALID, "%s: %d armed agents, but the handle has 1..%d", who, m, h->N);
    for (int32_t i = 0; i < m; ++i) {
        if (h_agents[i] < 0 || h_agents[i] >= h->N) return fail(h, F110_ERR_INVALID, "%s: agents[%d] = %d is outside 0..%d", who, i, h_agents[i], h->N - 1);
        if (i > 0 && h_agents[i] <= h_agents[i - 1]) return fail(h, F110_ERR_INVALID, "%s: the agents are not strictly ascending at [%d]", who, i);
        if (drives && !h->gap_assign_host.empty() && h->gap_assign_host[h_agents[i]] != -1)
            return fail(h, F110_ERR_INVALID, "%s: agent %d has a follow-the-gap controller (f110_controllers_set)", who, h_agents[i]);
        if (drives && !h->line_assign_host.empty() && h->line_assign_host[h_agents[i]] != -1)
            return fail(h, F110_ERR_INVALID, "%s: agent %d has a line follower (f110_line_followers_set)", who, h_agents[i]);
    }
    return F110_OK;
}

// a checked list into `a`, which the caller builds aside and moves in on success
static int armed_upload(f110_sim *h, const char *who, ArmedList &a, const int32_t *h_agents, size_t M, const uint64_t *h_streams)
{
    TRY(dmalloc(h, &a.d_agents, M));
    TRY(dmalloc(h, &a.d_streams, 4 * M));
    if (hipMemcpy(a.d_agents, h_agents, M * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(a.d_streams, h_streams, 4 * M * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        return fail(h, F110_ERR_HIP, "%s: the upload failed", who);
    a.agents.assign(h_agents, h_agents + M);
    a.m = (int)M;
    return F110_OK;
}

// the armed indices [i0, i0 + count) of one env block: the ascending list is split at the block's bounds
static void armed_split(const ArmedList &a, int A, const EnvBlock &b, int32_t &i0, int32_t &count)
{
    const int32_t n0 = b.e0 * A, n1 = (b.e0 + b.count) * A;
    i0 = (int32_t)(std::lower_bound(a.agents.begin(), a.agents.end(), n0) - a.agents.begin());
    count = (int32_t)(std::lower_bound(a.agents.begin(), a.agents.end(), n1) - a.agents.begin()) - i0;
}

// the refusals that begin a call on an armed feature: it (`noun`: "planner" / "filter") is armed, and with `map` the map is set
static int armed_ready(f110_sim *h, const char *who, const char *noun, const ArmedList &a, bool map)
{
    if (a.m == 0) return fail(h, F110_ERR_STATE, "%s: no %s is armed (f110_%s_set)", who, noun, who);
    if (map && !h->has_map) return fail(h, F110_ERR_STATE, "%s: the map is not set", who);
    return F110_OK;
}

// f110_<who>_get (put false: the host side is written) / _put: once the handle's work so far is done, every part the caller
// asks for (host != null) and then the streams' words [m][4] are copied
struct ArmedPart { const void *host; void *dev; size_t bytes; };
static int armed_transfer(f110_sim *h, const ArmedList &a, bool put, const uint64_t *h_streams, std::initializer_list<ArmedPart> parts)
{
    ENTER(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    std::vector<ArmedPart> all(parts);
    all.push_back({h_streams, a.d_streams, 4 * (size_t)a.m * sizeof(uint64_t)});
    for (const ArmedPart &q : all)
        if (q.host) HIPCHK(h, put ? hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) : hipMemcpy(const_cast<void *>(q.host), q.dev, q.bytes, hipMemcpyDeviceToHost));
    return F110_OK;
}

// what every job of a feature that draws shares: the generator's tables and the feature's jump constants [2][count]
template <typename Job>
static void job_rng_tables(const f110_sim *h, Job &j, const U128 *jump, int count)
{
    j.zk = h->d_zig_k, j.zw = h->d_zig_w, j.zf = h->d_zig_f;
    j.jump_a = jump, j.jump_g = jump + count;
}

// ---- MPPI planner (f110_mppi_*, include/f110.h) -------------------------------------------------------------------------------------
// the spec's refusals; on success the kernels' spec
static int mppi_check_spec(f110_sim *h, const f110_mppi *p, MppiSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "mppi: null spec");
    if (p->k < 1 || p->k > F110_MPPI_MAX_K) return fail(h, F110_ERR_INVALID, "mppi: k = %d is outside 1..%d", p->k, (int)F110_MPPI_MAX_K);
    if (p->horizon < 1 || p->horizon > F110_MPPI_MAX_H) return fail(h, F110_ERR_INVALID, "mppi: horizon = %d is outside 1..%d", p->horizon, (int)F110_MPPI_MAX_H);
    if (p->repeat < 1 || p->repeat > F110_MPPI_MAX_REPEAT) return fail(h, F110_ERR_INVALID, "mppi: repeat = %d is outside 1..%d", p->repeat, (int)F110_MPPI_MAX_REPEAT);
    if (p->shift != 0 && p->shift != 1) return fail(h, F110_ERR_INVALID, "mppi: shift = %d must be 0 or 1", p->shift);
    if (p->margin != p->margin) return fail(h, F110_ERR_INVALID, "mppi: margin is NaN");
    const double d[] = {p->sigma_steer, p->sigma_speed, p->steer_min, p->steer_max, p->speed_min, p->speed_max, p->lambda,
                        p->w_dead, p->w_clear, p->w_progress, p->w_lat, p->clear_ref, p->v_init};
    for (double x : d)
        if (!std::isfinite(x)) return fail(h, F110_ERR_INVALID, "mppi: every setting but the margin must be finite");
    if (p->sigma_steer < 0 || p->sigma_speed < 0) return fail(h, F110_ERR_INVALID, "mppi: sigma_steer and sigma_speed must be >= 0");
    if (p->steer_min > p->steer_max || p->speed_min > p->speed_max) return fail(h, F110_ERR_INVALID, "mppi: steer_min exceeds steer_max or speed_min exceeds speed_max");
    if (!(p->lambda > 0)) return fail(h, F110_ERR_INVALID, "mppi: lambda must be > 0");
    if (p->w_dead < 0 || p->w_clear < 0 || p->w_progress < 0 || p->w_lat < 0) return fail(h, F110_ERR_INVALID, "mppi: the weights must be >= 0");
    if (p->v_init < p->speed_min || p->v_init > p->speed_max) return fail(h, F110_ERR_INVALID, "mppi: v_init is outside [speed_min, speed_max]");
    o = MppiSpec{};
    o.K = p->k, o.H = p->horizon, o.repeat = p->repeat, o.shift = p->shift;
    o.margin = p->margin, o.sigma_steer = p->sigma_steer, o.sigma_speed = p->sigma_speed;
    o.steer_min = p->steer_min, o.steer_max = p->steer_max, o.speed_min = p->speed_min, o.speed_max = p->speed_max, o.lambda = p->lambda;
    o.w_dead = p->w_dead, o.w_clear = p->w_clear, o.w_progress = p->w_progress, o.w_lat = p->w_lat, o.clear_ref = p->clear_ref, o.v_init = p->v_init;
    return F110_OK;
}

// a feature's jump constants in device memory, [2][count], from its first arming on: build fills the two halves
static int jump_ensure(f110_sim *h, DevBuf<U128> &buf, void (*build)(U128 *, U128 *), int count)
{
    if (buf) return F110_OK;
    std::vector<U128> t(2 * (size_t)count);
    build(t.data(), t.data() + count);
    TRY(dmalloc(h, &buf, t.size()));
    HIPCHK(h, hipMemcpy(buf, t.data(), t.size() * sizeof(U128), hipMemcpyHostToDevice));
    return F110_OK;
}

// the tracks the armed planner's projection reads (nothing to do without a track weight)
static bool mppi_reads_tracks(const f110_sim::Mppi &p) { return mppi_needs_track(p.sp) || (p.opp_on && p.opp.mode == OPP_TRACK); }

static int mppi_upload_tracks(f110_sim *h)
{
    if (h->mppi.on.m > 0 && mppi_reads_tracks(h->mppi)) TRY(track_upload(h));
    return F110_OK;
}

// can the armed planner run?  The refusals of a call, nothing launched.
static int mppi_ready(f110_sim *h)
{
    const f110_sim::Mppi &p = h->mppi;
    TRY(armed_ready(h, "mppi", "planner", p.on, true));
    if (mppi_needs_track(p.sp)) TRY(tracks_in_use(h, "mppi: w_progress or w_lat is set", &p.on.agents));   // (only the envs of the armed agents)
    if (p.opp_on && p.opp.mode == OPP_TRACK) TRY(tracks_in_use(h, "mppi: the opponents follow the track", &p.on.agents));
    return F110_OK;
}

// armed indices [j.i0, j.i0 + j.count): the candidates, (track) the projections, the update, one behind the other on `st`
static void mppi_launch(const MppiJob &j, hipStream_t st, const OppLane *opp = nullptr)
{
    if (j.count <= 0) return;
    const size_t lanes = (size_t)j.count * j.sp.K;
    const dim3 block(256);
    if (opp) {   // the same lanes with the opponent term's sampling and its two cost terms (the predictions are on `st` already)
        if (j.sp.K % 64 == 0) hipLaunchKernelGGL((k_mppi_roll_opp<true>), grid1d(lanes, 256), block, 0, st, j, *opp);
        else hipLaunchKernelGGL((k_mppi_roll_opp<false>), grid1d(lanes, 256), block, 0, st, j, *opp);
    } else if (j.sp.K % 64 == 0) hipLaunchKernelGGL((k_mppi_roll<true>), grid1d(lanes, 256), block, 0, st, j);
    else hipLaunchKernelGGL((k_mppi_roll<false>), grid1d(lanes, 256), block, 0, st, j);
    if (j.end_xy) hipLaunchKernelGGL(k_mppi_track, grid1d(lanes * kTrackLanes, 256), block, 0, st, j);
    const int gs = mppi_group_lanes(j.sp.K, j.sp.H);
    hipLaunchKernelGGL(k_mppi_update, grid1d((size_t)j.count, 256 / gs), block, 0, st, j, gs);
}

// the armed planner over the agents of one env block
static int mppi_launch_armed(f110_sim *h, const EnvBlock &b, double *d_actions, float *d_info)
{
    const f110_sim::Mppi &p = h->mppi;
    const int A = h->cfg.num_agents;
    const bool track = mppi_needs_track(p.sp);
    MppiJob j{};
    TRY(job_live_source(h, "mppi", track, j));
    j.agents = p.on.d_agents;
    j.step_count = h->dev.step_count;
    job_rng_tables(h, j, h->d_mppi_jump, kMppiJumps);
    j.nominal = p.d_nominal;
    j.streams = p.on.d_streams;
    j.V = p.d_V;
    j.cost = p.d_cost;
    j.end_xy = track ? p.d_end : nullptr;
    j.actions = d_actions;
    j.info = d_info;
    j.sp_dev = p.d_spec;
    j.sp = p.sp;
    armed_split(p.on, A, b, j.i0, j.count);
    if (!p.opp_on) {
        mppi_launch(j, b.stream);
        return F110_OK;
    }
    // the opponent term: the block's armed agents' predictions from the live columns first (an env's cars are in one block)
    opp_predict_launch(h, j, p.opp, p.sp.H, p.sp.repeat, j.i0, j.count, A - 1, p.on.d_agents.get(), nullptr, nullptr, p.d_opp_table.get(), b.stream);
    const OppLane lane{p.d_opp_table.get(), p.d_opp_spec.get(), nullptr, nullptr, A - 1, 0};
    mppi_launch(j, b.stream, &lane);
    return F110_OK;
}

int f110_mppi_set(f110_sim *h, const f110_mppi *spec, const int32_t *h_agents, int32_t m, const uint64_t *h_streams)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    const int form = armed_form(h, "mppi", spec, h_agents, m, h_streams);
    if (form == kArmedDisarm) h->mppi = {};
    if (form != F110_OK) return form == kArmedDisarm ? F110_OK : form;
    MppiSpec sp;
    TRY(mppi_check_spec(h, spec, sp));
    TRY(armed_check_list(h, "mppi", h_agents, m, true));
    if ((size_t)m * sp.K >= (size_t)1 << 31) return fail(h, F110_ERR_INVALID, "mppi: %d agents x %d candidates do not fit 31 bits", m, sp.K);
    ENTER(h);
    TRY(jump_ensure(h, h->d_mppi_jump, mppi_jump_table, kMppiJumps));
    f110_sim::Mppi p;   // built aside: a failure below leaves the planner that is armed (if any) as it is
    const size_t M = (size_t)m, seq = (size_t)sp.H * 2, cands = M * sp.K;
    std::vector<double> nominal(M * seq);
    for (size_t q = 0; q < nominal.size(); ++q) nominal[q] = (q & 1) ? sp.v_init : 0.0;
    TRY(dmalloc(h, &p.d_spec, 1));
    TRY(dmalloc(h, &p.d_nominal, M * seq));
    TRY(dmalloc(h, &p.d_V, cands * seq));
    TRY(dmalloc(h, &p.d_cost, cands));
    if (mppi_needs_track(sp)) TRY(dmalloc(h, &p.d_end, 2 * cands));
    if (hipMemcpy(p.d_spec, &sp, sizeof sp, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p.d_nominal, nominal.data(), nominal.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess)
        return fail(h, F110_ERR_HIP, "mppi: the upload failed");
    p.sp = sp;
    TRY(armed_upload(h, "mppi", p.on, h_agents, M, h_streams));
    h->mppi = std::move(p);   // (the planner armed so far goes: hipFree waits for the calls in flight that read its memory)
    return F110_OK;
}

int f110_mppi_device(f110_sim *h, double *d_actions, float *d_info)
{
    if (!h || !d_actions) return fail(h, F110_ERR_INVALID, "mppi: null argument");
    TRY(mppi_ready(h));
    if (mppi_reads_tracks(h->mppi)) TRY(tracks_current(h));
    EnvBlocks w;   // behind a two-block step: each block's armed agents on the block's own stream (an agent reads and writes its own rows)
    TRY(env_blocks_follow(h, w));
    for (const EnvBlock &b : w) TRY(mppi_launch_armed(h, b, d_actions, d_info));
    HIPCHK(h, hipGetLastError());
    h->touched = false;
    return F110_OK;
}

// a caller's nominal: finite and within the spec's bounds
static int mppi_check_nominal(f110_sim *h, const MppiSpec &sp, const double *nominal, size_t rows)
{
    for (size_t q = 0; q < rows * sp.H * 2; ++q) {
        const double x = nominal[q], lo = (q & 1) ? sp.speed_min : sp.steer_min, hi = (q & 1) ? sp.speed_max : sp.steer_max;
        if (!std::isfinite(x) || x < lo || x > hi)
            return fail(h, F110_ERR_INVALID, "mppi: nominal[%zu][%zu][%d] = %g is not finite or outside [%g, %g]", q / (2 * (size_t)sp.H), q / 2 % sp.H, (int)(q & 1), x, lo, hi);
    }
    return F110_OK;
}

// f110_mppi_get / f110_mppi_put
static int mppi_state(f110_sim *h, const double *h_nominal, const uint64_t *h_streams, bool put)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    const f110_sim::Mppi &p = h->mppi;
    TRY(armed_ready(h, "mppi", "planner", p.on, false));
    const size_t M = (size_t)p.on.m;
    if (put && h_nominal) TRY(mppi_check_nominal(h, p.sp, h_nominal, M));
    return armed_transfer(h, p.on, put, h_streams, {{h_nominal, p.d_nominal, M * p.sp.H * 2 * sizeof(double)}});
}

int f110_mppi_get(f110_sim *h, double *h_nominal, uint64_t *h_streams) { return mppi_state(h, h_nominal, h_streams, false); }
int f110_mppi_put(f110_sim *h, const double *h_nominal, const uint64_t *h_streams) { return mppi_state(h, h_nominal, h_streams, true); }

// f110_mppi_batch, and with `ou` f110_mppi_opp_batch
static int mppi_batch(f110_sim *h, const f110_mppi *spec, int32_t slot, const double *h_start, const double *h_params, const int32_t *h_fresh, int32_t m,
                      double *h_nominal, uint64_t *h_streams, double *h_actions, float *h_info, double *h_cand, double *h_cost, double *h_weight,
                      const OppUnit *ou)
{
    MppiJob j{};
    TRY(mppi_check_spec(h, spec, j.sp));
    if (m < 0 || (m > 0 && (!h_start || !h_nominal || !h_streams))) return fail(h, F110_ERR_INVALID, "mppi: bad argument");
    if (ou) TRY(opp_unit_check(h, "mppi", *ou, m, slot));
    if ((size_t)m * j.sp.K >= (size_t)1 << 31) return fail(h, F110_ERR_INVALID, "mppi: %d rows x %d candidates do not fit 31 bits", m, j.sp.K);
    if (!h->has_map) return fail(h, F110_ERR_STATE, "mppi: the map is not set");
    TRY(unit_slot_check(h, "mppi", slot));
    const bool track = mppi_needs_track(j.sp);
    if (track && !track_has(h, slot)) return fail(h, F110_ERR_STATE, "mppi: w_progress or w_lat is set, but map slot %d has no track (f110_track_set)", slot);
    if (m == 0) return F110_OK;
    const size_t M = (size_t)m, seq = (size_t)j.sp.H * 2, cands = M * j.sp.K;
    TRY(mppi_check_nominal(h, j.sp, h_nominal, M));
    UnitRows rows;
    TRY(unit_rows(h, "mppi", h_start, M, rows));
    ENTER(h);
    TRY(jump_ensure(h, h->d_mppi_jump, mppi_jump_table, kMppiJumps));
    if (track || (ou && ou->sp.mode == OPP_TRACK)) TRY(track_upload(h));
    Scratch sc(h);
    TRY(job_unit_source(h, sc, slot, track, rows, h_params, j));
    j.step_count = sc.in(h_fresh, M);
    j.sp_dev = sc.in(&j.sp, 1);
    j.nominal = sc.inout(h_nominal, M * seq);
    j.streams = sc.inout(h_streams, 4 * M);
    j.V = sc.tmp<double>(cands * seq);
    j.cost = sc.tmp<double>(cands);
    j.weight = sc.tmp<double>(cands);
    j.actions = sc.tmp<double>(2 * M);
    j.info = sc.tmp<float>(4 * M);
    j.end_xy = track ? sc.tmp<double>(2 * cands) : nullptr;
    TRY(sc.ready());
    sc.later(h_actions, j.actions, 2 * M);
    sc.later(h_info, j.info, 4 * M);
    sc.later(h_cand, j.V, cands * seq);
    sc.later(h_cost, j.cost, cands);
    sc.later(h_weight, j.weight, cands);
    job_rng_tables(h, j, h->d_mppi_jump, kMppiJumps);
    OppLane lane{};
    if (ou) TRY(opp_unit_prepare(h, sc, j, *ou, j.sp.K, j.sp.H, j.sp.repeat, lane));
    mppi_launch(j, h->stream, ou ? &lane : nullptr);
    return sc.finish();
}

int f110_mppi_batch(f110_sim *h, const f110_mppi *spec, int32_t slot, const double *h_start, const double *h_params, const int32_t *h_fresh, int32_t m,
                    double *h_nominal, uint64_t *h_streams, double *h_actions, float *h_info, double *h_cand, double *h_cost, double *h_weight)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    return mppi_batch(h, spec, slot, h_start, h_params, h_fresh, m, h_nominal, h_streams, h_actions, h_info, h_cand, h_cost, h_weight, nullptr);
}

int f110_mppi_opp_batch(f110_sim *h, const f110_mppi *spec, const f110_opponents *opp, double w_hit, double w_near, double near_ref, int32_t slot,
                        const double *h_start, const double *h_params, const int32_t *h_fresh, const double *h_opp_rows, int32_t Ao, int32_t m,
                        double *h_nominal, uint64_t *h_streams, double *h_actions, float *h_info, double *h_cand, double *h_cost, double *h_weight,
                        double *h_opp_raw)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    OppUnit u{};
    TRY(opp_check_spec(h, "mppi", opp, u.sp));
    TRY(opp_check_weights(h, w_hit, w_near, near_ref, u.sp));
    u.h_rows = h_opp_rows;
    u.Ao = Ao;
    u.h_raw = h_opp_raw;
    return mppi_batch(h, spec, slot, h_start, h_params, h_fresh, m, h_nominal, h_streams, h_actions, h_info, h_cand, h_cost, h_weight, &u);
}

int f110_mppi_set_opponents(f110_sim *h, const f110_opponents *opp, double w_hit, double w_near, double near_ref)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    f110_sim::Mppi &p = h->mppi;
    if (!opp) {   // detach (nothing to do while nothing is attached)
        if (!p.opp_on) return F110_OK;
        ENTER(h);
        p.opp_on = false;
        p.opp = OppSpec{};
        p.d_opp_spec.reset();    // (hipFree waits for the calls in flight that read them)
        p.d_opp_table.reset();
        return F110_OK;
    }
    OppSpec os;
    TRY(opp_check_spec(h, "mppi", opp, os));
    TRY(opp_check_weights(h, w_hit, w_near, near_ref, os));
    const int Ao = h->cfg.num_agents - 1;
    if (Ao > OPP_MAX) return fail(h, F110_ERR_INVALID, "mppi: %d opponents per agent, at most %d", Ao, (int)OPP_MAX);
    TRY(armed_ready(h, "mppi", "planner", p.on, true));
    if (os.mode == OPP_TRACK) TRY(tracks_in_use(h, "mppi: the opponents follow the track", &p.on.agents));
    ENTER(h);
    DevBuf<OppSpec> dspec;   // built aside: a failure leaves what is attached (if anything) as it is
    DevBuf<double> dtable;
    TRY(dmalloc(h, &dspec, 1));
    if (Ao > 0) TRY(dmalloc(h, &dtable, (size_t)p.on.m * Ao * p.sp.H * 2));
    HIPCHK(h, hipMemcpy(dspec, &os, sizeof os, hipMemcpyHostToDevice));
    p.d_opp_spec = std::move(dspec);
    p.d_opp_table = std::move(dtable);
    p.opp = os;
    p.opp_on = true;
    return F110_OK;
}

// ---- particle filter (f110_pf_*, include/f110.h) ------------------------------------------------------------------------------------
// the spec's refusals; on success the kernels' spec
static int pf_check_spec(f110_sim *h, const f110_pf *p, PfSpec &o)
{
    if (!p) return fail(h, F110_ERR_INVALID, "pf: null spec");
    if (p->particles < 1 || p->particles > F110_PF_MAX_P) return fail(h, F110_ERR_INVALID, "pf: particles = %d is outside 1..%d", p->particles, (int)F110_PF_MAX_P);
    if (p->n_beams < 1 || p->n_beams > F110_PF_MAX_BEAMS) return fail(h, F110_ERR_INVALID, "pf: n_beams = %d is outside 1..%d", p->n_beams, (int)F110_PF_MAX_BEAMS);
    if (p->beam_first < 0 || p->beam_stride < 1) return fail(h, F110_ERR_INVALID, "pf: beam_first = %d must be >= 0 and beam_stride = %d >= 1", p->beam_first, p->beam_stride);
    if ((long long)p->beam_first + (long long)(p->n_beams - 1) * p->beam_stride >= (long long)h->cfg.num_beams)
        return fail(h, F110_ERR_INVALID, "pf: beam %lld is past the scan's %d beams", (long long)p->beam_first + (long long)(p->n_beams - 1) * p->beam_stride, h->cfg.num_beams);
    const double d[] = {p->sigma_x, p->sigma_y, p->sigma_theta, p->init_x, p->init_y, p->init_theta, p->sigma_hit, p->squash, p->resample_frac};
    for (double x : d)
        if (!std::isfinite(x)) return fail(h, F110_ERR_INVALID, "pf: every setting but the clip must be finite");
    if (p->clip != p->clip) return fail(h, F110_ERR_INVALID, "pf: clip is NaN");
    if (p->sigma_x < 0 || p->sigma_y < 0 || p->sigma_theta < 0 || p->init_x < 0 || p->init_y < 0 || p->init_theta < 0)
        return fail(h, F110_ERR_INVALID, "pf: the sigmas must be >= 0");
    if (!(p->sigma_hit > 0) || !(p->clip > 0) || !(p->squash > 0)) return fail(h, F110_ERR_INVALID, "pf: sigma_hit, clip and squash must be > 0");
    if (p->resample_frac < 0) return fail(h, F110_ERR_INVALID, "pf: resample_frac must be >= 0");
    o = PfSpec{};
    o.P = p->particles, o.B = p->n_beams, o.beam_first = p->beam_first, o.beam_stride = p->beam_stride;
    o.sigma_x = p->sigma_x, o.sigma_y = p->sigma_y, o.sigma_theta = p->sigma_theta;
    o.init_x = p->init_x, o.init_y = p->init_y, o.init_theta = p->init_theta;
    o.sigma_hit = p->sigma_hit, o.clip = p->clip, o.squash = p->squash, o.resample_frac = p->resample_frac;
    return F110_OK;
}

static int pf_check_count(f110_sim *h, const PfSpec &sp, int m)
{
    if ((size_t)m * sp.P * sp.B >= (size_t)1 << 31) return fail(h, F110_ERR_INVALID, "pf: %d agents x %d particles x %d beams do not fit 31 bits", m, sp.P, sp.B);
    return F110_OK;
}

// a caller's cloud and weights: finite particles; weight rows that are finite, >= 0 and sum to more than 0
static int pf_check_cloud(f110_sim *h, const PfSpec &sp, const double *particles, const double *weights, size_t rows)
{
    if (particles)
        for (size_t q = 0; q < rows * sp.P * 3; ++q)
            if (!std::isfinite(particles[q])) return fail(h, F110_ERR_INVALID, "pf: particles[%zu][%zu][%d] is not finite", q / (3 * (size_t)sp.P), q / 3 % sp.P, (int)(q % 3));
    if (weights)
        for (size_t r = 0; r < rows; ++r) {
            double sum = 0.0;
            for (int p = 0; p < sp.P; ++p) {
                const double w = weights[r * sp.P + p];
                if (!std::isfinite(w) || w < 0) return fail(h, F110_ERR_INVALID, "pf: weights[%zu][%d] = %g is negative or not finite", r, p, w);
                sum += w;
            }
            if (!(sum > 0)) return fail(h, F110_ERR_INVALID, "pf: the weights of row %zu do not sum to more than 0", r);
        }
    return F110_OK;
}

// armed indices [j.i0, j.i0 + j.count): the plan, the move, the rays, the update, one behind the other on `st`
static void pf_launch(const PfJob &j, const ScanConst &k, hipStream_t st)
{
    if (j.count <= 0) return;
    const int P = j.sp.P;
    const size_t parts = (size_t)j.count * P;
    const dim3 block(256);
    hipLaunchKernelGGL(k_pf_plan, grid1d((size_t)j.count, 4), block, (size_t)4 * P * sizeof(double), st, j);
    hipLaunchKernelGGL(k_pf_move, grid1d(parts, 256), block, 0, st, j, k);
    const int ppw = pf_particles_per_group(j.sp.B);
    hipLaunchKernelGGL(k_pf_sense, grid1d(parts, ppw), block, 0, st, j, k, ppw);
    const int gs = pf_group_lanes(P), per = 256 / gs;
    hipLaunchKernelGGL(k_pf_update, grid1d((size_t)j.count, per), block, (size_t)per * 6 * P * sizeof(double), st, j, gs);
}

// what every job of this handle shares: the generator's tables, the lidar's offset, the scan's width
static void pf_job_common(f110_sim *h, PfJob &j)
{
    job_rng_tables(h, j, h->d_pf_jump, kPfJumps);
    j.lidar_dist = h->dev.lidar_dist;
    j.num_beams = h->cfg.num_beams;
}

// the armed filter over the agents of one env block
static int pf_launch_armed(f110_sim *h, const EnvBlock &b, double *d_pose, float *d_info)
{
    const f110_sim::Pf &p = h->pf;
    const int A = h->cfg.num_agents;
    const size_t N = (size_t)h->N;
    PfJob j{};
    j.maps = h->multi_map ? h->d_maps_full : cold_consts(h);
    if (!j.maps) return fail(h, F110_ERR_HIP, "pf: constant upload failed");
    j.env_map = h->multi_map ? h->d_env_map : nullptr;
    j.A = A;
    j.N = h->N;
    j.agents = p.on.d_agents;
    j.px = h->dev.snap_pose;   // the post-step pose of the observation
    j.py = h->dev.snap_pose + N;
    j.pth = h->dev.snap_pose + 2 * N;
    j.scans = h->dev.scans;
    j.step_count = h->dev.step_count;
    pf_job_common(h, j);
    j.streams = p.on.d_streams;
    j.X_in = p.d_X[p.cur];
    j.X_out = p.d_X[p.cur ^ 1];
    j.W = p.d_W;
    j.last = p.d_last;
    j.cum = p.d_cum;
    j.plan = p.d_plan;
    j.hdr = p.d_hdr;
    j.logw = p.d_logw;
    j.pose = d_pose;
    j.info = d_info;
    j.sp = p.sp;
    armed_split(p.on, A, b, j.i0, j.count);
    pf_launch(j, h->k, b.stream);
    return F110_OK;
}

int f110_pf_set(f110_sim *h, const f110_pf *spec, const int32_t *h_agents, int32_t m, const uint64_t *h_streams)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    const int form = armed_form(h, "pf", spec, h_agents, m, h_streams);
    if (form == kArmedDisarm) h->pf = {};
    if (form != F110_OK) return form == kArmedDisarm ? F110_OK : form;
    PfSpec sp;
    TRY(pf_check_spec(h, spec, sp));
    TRY(armed_check_list(h, "pf", h_agents, m, false));   // (the filter drives nothing: a scripted car may be localised)
    TRY(pf_check_count(h, sp, m));
    ENTER(h);
    TRY(jump_ensure(h, h->d_pf_jump, pf_jump_table, kPfJumps));
    f110_sim::Pf p;   // built aside: a failure below leaves the filter that is armed (if any) as it is
    const size_t M = (size_t)m, parts = M * sp.P;
    std::vector<double> w(parts, 1.0 / (double)sp.P);
    TRY(dmalloc(h, &p.d_X[0], 3 * parts));
    TRY(dmalloc(h, &p.d_X[1], 3 * parts));
    TRY(dmalloc(h, &p.d_W, parts));
    TRY(dmalloc(h, &p.d_last, 3 * M));
    TRY(dmalloc(h, &p.d_cum, parts));
    TRY(dmalloc(h, &p.d_logw, parts));
    TRY(dmalloc(h, &p.d_plan, M));
    TRY(dmalloc(h, &p.d_hdr, parts));
    if (hipMemcpy(p.d_W, w.data(), parts * sizeof(double), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(p.d_X[0], 0, 3 * parts * sizeof(double)) != hipSuccess ||
        hipMemset(p.d_X[1], 0, 3 * parts * sizeof(double)) != hipSuccess ||
        hipMemset(p.d_last, 0, 3 * M * sizeof(double)) != hipSuccess)
        return fail(h, F110_ERR_HIP, "pf: the upload failed");
    p.sp = sp;
    TRY(armed_upload(h, "pf", p.on, h_agents, M, h_streams));
    h->pf = std::move(p);   // (the filter armed so far goes: hipFree waits for the calls in flight that read its memory)
    return F110_OK;
}

int f110_pf_device(f110_sim *h, double *d_pose, float *d_info)
{
    if (!h || !d_pose) return fail(h, F110_ERR_INVALID, "pf: null argument");
    TRY(armed_ready(h, "pf", "filter", h->pf.on, true));
    EnvBlocks w;   // behind a two-block step: each block's armed agents on the block's own stream (an agent reads and writes its own rows)
    TRY(env_blocks_follow(h, w));
    for (const EnvBlock &b : w) TRY(pf_launch_armed(h, b, d_pose, d_info));
    HIPCHK(h, hipGetLastError());
    h->pf.cur ^= 1;
    h->touched = false;
    return F110_OK;
}

// f110_pf_get / f110_pf_put
static int pf_state(f110_sim *h, const double *h_particles, const double *h_weights, const double *h_last, const uint64_t *h_streams, bool put)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    const f110_sim::Pf &p = h->pf;
    TRY(armed_ready(h, "pf", "filter", p.on, false));
    const size_t M = (size_t)p.on.m, cloud = M * p.sp.P * sizeof(double);
    if (put) TRY(pf_check_cloud(h, p.sp, h_particles, h_weights, M));
    return armed_transfer(h, p.on, put, h_streams, {{h_particles, p.d_X[p.cur], 3 * cloud}, {h_weights, p.d_W, cloud}, {h_last, p.d_last, 3 * M * sizeof(double)}});
}

int f110_pf_get(f110_sim *h, double *h_particles, double *h_weights, double *h_last, uint64_t *h_streams) { return pf_state(h, h_particles, h_weights, h_last, h_streams, false); }
int f110_pf_put(f110_sim *h, const double *h_particles, const double *h_weights, const double *h_last, const uint64_t *h_streams) { return pf_state(h, h_particles, h_weights, h_last, h_streams, true); }

int f110_pf_batch(f110_sim *h, const f110_pf *spec, int32_t slot, const double *h_poses, const double *h_scans, const int32_t *h_fresh, int32_t m,
                  double *h_particles, double *h_weights, double *h_last, uint64_t *h_streams, double *h_pose, float *h_info, double *h_noise,
                  int32_t *h_anc, double *h_expect, double *h_logw)
{
    if (!h) return fail(nullptr, F110_ERR_INVALID, "null handle");
    PfJob j{};
    TRY(pf_check_spec(h, spec, j.sp));
    if (m < 0 || (m > 0 && (!h_poses || !h_scans || !h_particles || !h_weights || !h_last || !h_streams))) return fail(h, F110_ERR_INVALID, "pf: bad argument");
    TRY(pf_check_count(h, j.sp, m));
    if (!h->has_map) return fail(h, F110_ERR_STATE, "pf: the map is not set");
    TRY(unit_slot_check(h, "pf", slot));
    if (m == 0) return F110_OK;
    const size_t M = (size_t)m, P = (size_t)j.sp.P, parts = M * P, B = (size_t)h->cfg.num_beams;
    TRY(pf_check_cloud(h, j.sp, h_particles, h_weights, M));
    std::vector<double> cols(3 * M);
    for (size_t r = 0; r < M; ++r)
        for (int c = 0; c < 3; ++c) cols[(size_t)c * M + r] = h_poses[3 * r + c];
    ScanConst kc = slot_consts(h, slot);
    ENTER(h);
    TRY(jump_ensure(h, h->d_pf_jump, pf_jump_table, kPfJumps));
    Scratch sc(h);
    const double *dcols = sc.in(cols.data(), cols.size());
    j.scans = sc.in(h_scans, M * B);
    j.maps = sc.in(&kc, 1);
    j.step_count = sc.in(h_fresh, M);
    j.X_in = sc.in(h_particles, 3 * parts);
    j.X_out = sc.tmp<double>(3 * parts);
    j.W = sc.inout(h_weights, parts);
    j.last = sc.inout(h_last, 3 * M);
    j.streams = sc.inout(h_streams, 4 * M);
    j.cum = sc.tmp<double>(parts);
    j.logw = sc.tmp<double>(parts);
    j.plan = sc.tmp<PfPlan>(M);
    j.hdr = sc.tmp<PfHdr>(parts);
    j.pose = sc.tmp<double>(3 * M);
    j.info = sc.tmp<float>(4 * M);
    j.noise = sc.out(h_noise, 3 * parts);
    j.anc = sc.out(h_anc, parts);
    j.expect = sc.out(h_expect, parts * j.sp.B);
    TRY(sc.ready());
    sc.later(h_particles, j.X_out, 3 * parts);
    sc.later(h_pose, j.pose, 3 * M);
    sc.later(h_info, j.info, 4 * M);
    sc.later(h_logw, j.logw, parts);
    j.A = 1;
    j.N = m;
    j.count = m;
    j.px = dcols;
    j.py = dcols + M;
    j.pth = dcols + 2 * M;
    pf_job_common(h, j);
    pf_launch(j, h->k, h->stream);
    return sc.finish();
}

// the example policy on poses the caller holds in device memory (the filter's estimates): f110_pure_pursuit_device's launch per env
// block, reading d_poses [N][3] instead of the live state
int f110_pure_pursuit_poses_device(f110_sim *h, const double *d_waypoints, int32_t M, const double *d_poses, double lookahead, double vgain,
                                   double wheelbase, double max_reacquire, double *d_actions)
{
    TRY(check_planner_args(h, d_waypoints, M, lookahead));
    if (!d_poses || !d_actions) return fail(h, F110_ERR_INVALID, "pure pursuit: null poses or actions buffer");
    EnvBlocks w;
    TRY(env_blocks_follow(h, w));
    const int A = h->cfg.num_agents;
    for (const EnvBlock &b : w) {
        const size_t i0 = (size_t)b.e0 * A;
        const int n = b.count * A;
        const double *p = d_poses + 3 * i0;
        hipLaunchKernelGGL(k_pure_pursuit, grid1d((size_t)n * kPlanLanes, 256), dim3(256), 0, b.stream, d_waypoints, M, p, p + 1, p + 2, 3, n, lookahead, vgain,
                           wheelbase, max_reacquire, d_actions + 2 * i0);
    }
    HIPCHK(h, hipGetLastError());
    h->touched = false;
    return F110_OK;
}
