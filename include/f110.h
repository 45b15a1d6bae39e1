/*
 * f110.h — C ABI of libf110_hip.so: the MI355X (gfx950) batched F1TENTH env.step() hot path.
 *
 * The reference (f1tenth/f1tenth_gym v0.2.1) has no FFI: its operator boundary is the set of
 * Python call sites where RaceCar/Simulator call the @njit kernels.  Each entry point below
 * names the reference interface it replaces (paths relative to gym/f110_gym/envs/).  The
 * Python host package f1tenth_gym_amd binds exactly these symbols with ctypes
 * (f1tenth_gym_amd/_ffi.py); INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; every call returns 0 (F110_OK) or a negative code and
 *     leaves a message retrievable with f110_last_error() (handle may be NULL for create).
 *   - "h_" pointers are host memory owned by the caller, consumed before the call returns
 *     (or before f110_sync for *_async variants); "d_" pointers are device memory.
 *   - one handle = one GPU + one HIP stream; calls on one handle must be serialised by the
 *     caller, different handles may be driven from different threads / processes.
 *   - agents are indexed i = env * num_agents + agent  (N = num_envs * num_agents);
 *     all arithmetic is IEEE float64 in the reference's operation order (no FMA contraction).
 *   - there is NO CPU fallback: without a usable HIP device every compute call fails.
 */
#ifndef F110_H
#define F110_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define F110_ABI_VERSION 1

enum {
    F110_OK = 0,
    F110_ERR_INVALID = -1,   /* bad argument (ValueError / IndexError on the Python side) */
    F110_ERR_NO_MAP = -2,    /* scan/step before a map is set (laser_models.py:445-446) */
    F110_ERR_HIP = -3,       /* HIP runtime / device error */
    F110_ERR_STATE = -4,     /* call not valid in the handle's current state */
    F110_ERR_NOMEM = -5
};

/* vehicle parameter vector: key order of f110_env.py:130 */
enum {
    F110_P_MU = 0, F110_P_CSF, F110_P_CSR, F110_P_LF, F110_P_LR, F110_P_H, F110_P_M, F110_P_I,
    F110_P_SMIN, F110_P_SMAX, F110_P_SVMIN, F110_P_SVMAX, F110_P_VSWITCH, F110_P_AMAX,
    F110_P_VMIN, F110_P_VMAX, F110_P_WIDTH, F110_P_LENGTH, F110_NPARAMS
};

enum { F110_INTEGRATOR_RK4 = 1, F110_INTEGRATOR_EULER = 2 }; /* base_classes.py:40-42 */

/* distance-table layouts in HBM.  Values 1 (4x4-cell tiles), 2 (1-byte codes + exact value LUT in LDS) and
 * 4 (a 128x128-cell window of byte codes per agent in LDS) existed in the experimental build through round 4 — bit-identical,
 * measured slower (DESIGN_HISTORY.md) — and were retired in round 5: f110_create refuses them (F110_ERR_INVALID). */
enum {
    F110_MAP_ROWMAJOR_F64 = 0, /* dt[r][c] as the reference stores it */
    F110_MAP_TILED_F64 = 1,    /* retired */
    F110_MAP_CODE8 = 2,        /* retired */
    F110_MAP_PADDED_F64 = 3,   /* dt[r][c] inside a border of out-of-bounds cells (max_range wide), so
                                  the march loop needs no range test, with fixed-point cell addressing
                                  and an exact re-march for samples in the guard band (the fastest
                                  layout; maps too large for it run as F110_MAP_ROWMAJOR_F64) */
    F110_MAP_WINDOW_LDS = 4    /* retired */
};

/* Simulator(params, num_agents, seed, time_step, ego_idx, integrator, lidar_dist)
 * base_classes.py:465 + RaceCar(num_beams=1080, fov=4.7) :69 + ScanSimulator2D(eps, theta_dis,
 * max_range) laser_models.py:360 + ttc_thresh base_classes.py:115.  */
typedef struct f110_config {
    int32_t abi_version;   /* F110_ABI_VERSION */
    int32_t num_envs;      /* E independent environments (extension; reference has 1) */
    int32_t num_agents;    /* A agents per environment */
    int32_t num_beams;     /* B */
    int32_t theta_dis;
    int32_t integrator;
    int32_t device_id;     /* HIP device ordinal */
    int32_t map_layout;    /* F110_MAP_* */
    int32_t scan_block;    /* threads per scan workgroup (0 = default) */
    int32_t scan_tasks_per_wave; /* consecutive 64-ray tasks each wave walks (0 = default) */
    int32_t step_groups;   /* env blocks per step: 0 = automatic (f110_step_device calls that come back to back are submitted as
                              two halves of the envs on two streams, at the batch sizes where that pays; anything else in one
                              block), 1 = always one block, 2 = always two, > 2 = experimental build.  Results do not depend on it. */
    int32_t step_graph;    /* must be 0 (the step as one captured HIP graph: measured slower, retired in round 5; the field keeps the struct layout) */
    double fov, eps, max_range;
    double time_step, lidar_dist, ttc_thresh;
    double params[F110_NPARAMS]; /* initial vehicle params for every agent slot */
} f110_config;

typedef struct f110_sim f110_sim;

const char *f110_last_error(const f110_sim *h);
int f110_abi_version(void);
int f110_device_count(int *count);
/* "dddd:bb:dd.f" of HIP device `device` (hipDeviceGetPCIBusId): lets the launcher pin each rank's host
 * threads to the NUMA node its GPU hangs off (f1tenth_gym_amd/numa.py); out: >= 16 bytes */
int f110_device_pci_bus_id(int32_t device, char *out, int32_t len);
/* "csrc=<sha256 prefix of the kernel sources this library was built from>": profiles/ entries and
 * bench.py's roofline record carry the same hash, so a reader can tie a number to the code */
const char *f110_build_info(void);
/* Device allocations the library's handles own at this moment, process-wide: their count and their bytes (either pointer
 * may be NULL).  Takes no handle, so that it can be read after f110_destroy: a handle that is gone has given everything
 * back.  Caller-owned memory (f110_device_alloc) and page-locked host memory are not counted. */
int f110_device_allocs(int64_t *live, int64_t *bytes);

/* 1 for libf110_hip_exp.so (-DF110_EXPERIMENTAL), 0 for the product library */
int f110_is_experimental(void);
/* The switchboard of the experimental build — every variant that was measured against the default and not
 * adopted, for the A/B tests and the profiles.  The product library refuses every key
 * (F110_ERR_STATE) and reads no environment variable; a step of the product has ONE dispatch per (agents per
 * env, beams) case.  Keys: scan_flat, collide_mode (0 side stream | 1 fused into k_integrate | 2 in line | 3 inside k_finalize),
 * task_order, task_thr, task_cap_div (list capacity = tasks / div), task_rev (walk the list from its newest entry), long_prio,
 * scan_occupancy, scan_env_counter (fusion probes), integrate_duo (-1|0|1: k_integrate in one wave or two per 64 agents),
 * integrate_fan (-1|0|1), group_split, pair_wave (-1|0|1: the A = 2 finalize as one-wave workgroups never / in every step; -1 = in a step of two env blocks, from 24 576 agents or under step_groups = 2),
 * step_tiny (0: tiny batches through the three kernels too — the A/B of k_step_tiny), scan_trace_hi / scan_trace_lo (the two halves of the device address of a caller-owned
 * [launch waves][8] uint64 buffer that every wave of the step's scan kernel stamps with its begin / end clock, CU and samples:
 * tools/debug/scan_timeline.py; 0 = off).  Retired with the code they switched (numbers in DESIGN.md section 8 / DESIGN_HISTORY.md) — round 5:
 * dedupe_two_pass, no_window, finalize_lanes / _flat / _roles, pair_always, step_graph, ray_pass / ray_thr / ray_waves; round 6 (the
 * pre-registered stop rule for march variants): scan_stream / stream_refill / stream_block / stream_grid (the lane-refill scan),
 * spec_from (the speculative tail march), finalize_wave (the A = 2 finalize as one-wave workgroups), pad_tiled (the step's march on a
 * 4x4-tiled or a row-pair copy of the PADDED table), scan_nt (non-temporal range stores): F110_ERR_INVALID. */
int f110_exp_set(f110_sim *h, const char *key, int32_t value);

int f110_create(const f110_config *cfg, f110_sim **out);
void f110_destroy(f110_sim *h);
int f110_sync(f110_sim *h);

/* ---- ScanSimulator2D.set_map  laser_models.py:383-427 ----
 * image: h_img [height][width] uint8, top row first as PIL decodes it; the library does the
 * FLIP_TOP_BOTTOM (:399), the <=128 threshold (:403-404), the exact EDT (:425,:40-53) and
 * dt = resolution*sqrt(d2) on the device.  origin = yaml 'origin' (x, y, yaw). */
int f110_set_map_image(f110_sim *h, const uint8_t *h_img, int32_t height, int32_t width,
                       double resolution, double origin_x, double origin_y, double origin_yaw);
/* same, from a caller-supplied distance table (row 0 = bottom of the picture). */
int f110_set_map_dt(f110_sim *h, const double *h_dt, int32_t height, int32_t width,
                    double resolution, double origin_x, double origin_y, double origin_c,
                    double origin_s);
int f110_get_map_dt(f110_sim *h, double *h_dt_out); /* row-major [height][width] */
int f110_map_shape(f110_sim *h, int32_t *height, int32_t *width);

/* sines/cosines = sin/cos(linspace(0, 2pi, theta_dis))  laser_models.py:379-381 (host-computed
 * so they are bit-identical to NumPy's). */
int f110_set_trig_tables(f110_sim *h, const double *h_sines, const double *h_cosines, int32_t n);
/* RaceCar class-level per-beam tables, base_classes.py:125-158 */
int f110_set_beam_tables(f110_sim *h, const double *h_scan_angles, const double *h_cosines,
                         const double *h_side_distances, int32_t num_beams);
/* Extension (domain randomisation): a different track per env.  The map of
 * f110_set_map_* is slot 0; f110_add_map_* registers further maps (same arguments, same exact-EDT
 * pipeline) and returns their slot; f110_set_env_maps assigns a slot to every env (h_env_map
 * [num_envs]; NULL = everybody back on slot 0).  Needs map_layout = F110_MAP_PADDED_F64 with every
 * map fitting it (any beam count).  Changing slot 0 or adding maps takes
 * effect at the next f110_set_env_maps.  Unit entry points (f110_scan_batch ...) keep using slot 0. */
int f110_add_map_image(f110_sim *h, const uint8_t *h_img, int32_t height, int32_t width,
                       double resolution, double origin_x, double origin_y, double origin_yaw,
                       int32_t *slot);
int f110_add_map_dt(f110_sim *h, const double *h_dt, int32_t height, int32_t width,
                    double resolution, double origin_x, double origin_y, double origin_c,
                    double origin_s, int32_t *slot);
int f110_set_env_maps(f110_sim *h, const int32_t *h_env_map);

/* Extension (obstacle avoidance): static obstacles stamped into a map slot ON THE DEVICE.  A DERIVED slot has its
 * base slot's geometry and a padded table of its own; everything that reads a slot's table (the scan, the iTTC wall check, the
 * reset sampler's clearance test, the rollout's clearance sample, the render's occupancy grid) sees the obstacles with no change
 * of its own.  Obstacles are per SLOT, not per env: memory is one padded table per derived slot.
 *
 * An obstacle: (x, y) its centre in map (world) coordinates; (c, s) the cosine and sine of its yaw AS THE CALLER COMPUTED THEM
 * (the device calls no trigonometric function here); a box has half extents half_length (along its yaw) and half_width, a disc
 * the radius half_length (c, s, half_width are then ignored but must be finite, half_width >= 0).  At most F110_MAX_OBSTACLES per slot.
 *
 * Table cell (r, c) — row 0 at the bottom, as the table is indexed — is STAMPED when its centre lies in a shape; float64 in
 * exactly this order, never contracted, with the slot's resolution res, origin (ox, oy) and origin cosine / sine (oc, os):
 *   px = ((double)c + 0.5) * res,  py = ((double)r + 0.5) * res
 *   wx = ox + (px * oc - py * os), wy = oy + (px * os + py * oc)
 *   dx = wx - x,  dy = wy - y
 *   box:  u = dx * c + dy * s,  v = -dx * s + dy * c,  stamped iff fabs(u) <= half_length && fabs(v) <= half_width
 *   disc: stamped iff dx * dx + dy * dy <= half_length * half_length
 * Parts of a shape outside the table are ignored.  The slot's table is
 *   T'[r][c] = min(T_base[r][c], res * sqrt((double)d2[r][c])),
 * d2 the exact squared Euclidean distance, in cells, to the nearest stamped cell; where nothing is stamped inside the table
 * T' = T_base.  For a base that came from an image this equals the reference pipeline (flip, threshold, resolution *
 * distance_transform_edt) run on the image with the stamped cells blacked out, bit for bit: the EDT of a union of occupied sets is
 * the elementwise minimum of the EDTs, and res * sqrt is monotone.  The slot's out-of-bounds value is T'[H-1][W-1]; the border of
 * its padded copy holds that value.
 *
 * f110_add_map_obstacles registers a new slot derived from base_slot (slot 0 or a slot of f110_add_map_*, not a derived slot;
 * n = 0: a copy of the base; h_obs may then be NULL).  Same preconditions as f110_add_map_*: the padded layout and a map that fits
 * it (and sides of at most 16384 cells, as f110_add_map_image asks).  Takes effect at the next f110_set_env_maps.
 * f110_set_map_obstacles re-stamps a derived slot IN PLACE from its base (not from its previous contents): the slot's table keeps
 * its allocation and address, scratch (a byte mask, the active columns' distances) grows with the map, never with the number of
 * calls.  The update is ordered behind every step in flight (on either env block) and in front of the next one, so the caller
 * needs no synchronisation of its own; the call returns once the new out-of-bounds value has been read back.  It refreshes that
 * value in the handle's constants and in the device-side slot table of f110_set_env_maps, marks the slot's cached render occupancy
 * grid stale (the next render rebuilds it) and leaves track data alone.
 * Refused (an error code, a message, nothing launched or written): null arguments, a slot out of range, a derived slot as base,
 * f110_set_map_obstacles on a slot that is not derived, n < 0 or n > F110_MAX_OBSTACLES, an unknown shape, a non-finite field, a
 * negative half extent, a base whose shape no longer matches (slot 0 re-set to another map since).
 * f110_get_slot_dt / f110_slot_shape: f110_get_map_dt / f110_map_shape for any slot (the row-major table out of its padded copy).
 * f110_slot_table: the device address of the slot's table cell [0][0] and its row pitch in bytes (what the kernels read). */
enum { F110_OBST_BOX = 0, F110_OBST_DISC = 1 };
enum { F110_MAX_OBSTACLES = 256 };
typedef struct f110_obstacle {
    int32_t shape;      /* F110_OBST_BOX / F110_OBST_DISC */
    int32_t reserved;   /* alignment; ignored */
    double x, y;        /* centre, map coordinates */
    double c, s;        /* cos(yaw), sin(yaw) */
    double half_length; /* >= 0; a disc's radius */
    double half_width;  /* >= 0 */
} f110_obstacle;
int f110_add_map_obstacles(f110_sim *h, int32_t base_slot, const f110_obstacle *h_obs, int32_t n, int32_t *slot);
int f110_set_map_obstacles(f110_sim *h, int32_t slot, const f110_obstacle *h_obs, int32_t n);
int f110_get_slot_dt(f110_sim *h, int32_t slot, double *h_dt_out); /* row-major [height][width] */
int f110_slot_shape(f110_sim *h, int32_t slot, int32_t *height, int32_t *width);
int f110_slot_table(f110_sim *h, int32_t slot, const double **d_table, int32_t *row_bytes);

/* Extension: a CORRIDOR carved into a map slot ON THE DEVICE — the step from a line to a distance table.
 *
 * A corridor: points xy [M][2] in map (world) coordinates, a `closed` flag, S = closed ? M : M - 1 segments, segment i from point i
 * to point (i + 1) % M, and one half width hw[i] >= 0 per segment.  Table cell (r, c) — row 0 at the bottom — is CARVED (free) iff
 * its centre lies in the capsule of some segment; float64 in exactly this order, never contracted, the cell centre (wx, wy) by the
 * stamp rule's formula above (px, py, wx, wy from res, ox, oy, oc, os), segment a -> b with half width hw:
 *   ux = wx - ax, uy = wy - ay;  dx = bx - ax, dy = by - ay
 *   t  = ux*dx + uy*dy;          L2 = dx*dx + dy*dy;      h2 = hw*hw
 *   t <= 0   : carved iff ux*ux + uy*uy <= h2               (also the whole rule when a == b)
 *   t >= L2  : vx = wx - bx, vy = wy - by;  carved iff vx*vx + vy*vy <= h2
 *   else     : cr = ux*dy - uy*dx;          carved iff cr*cr <= h2*L2
 * No division, no square root, no trigonometric function.  The BORDER RING (row 0, row H-1, column 0, column W-1) is never carved,
 * so a corridor that leaves the table is still closed by a wall; parts of a corridor outside the table are ignored.  The slot's
 * table is T[r][c] = res * sqrt((double)d2[r][c]), d2 the exact squared Euclidean distance, in cells, to the nearest cell that is
 * not carved: the reference pipeline (flip, > 128, resolution * distance_transform_edt), bit for bit, on the image that has the
 * carved cells at 255 and all others at 0.  Out-of-bounds value and padded border as for every slot: T[H-1][W-1], 0 by the ring.
 *
 * f110_add_map_corridor registers a new BASE slot (not a derived one: obstacle slots may be derived from it) with a padded table of
 * its own, in the frame (res, ox, oy, oyaw); preconditions and size limits as f110_add_map_image; takes effect at the next
 * f110_set_env_maps.  f110_set_map_corridor re-carves such a slot IN PLACE: same frame, same allocation and address; scratch (the
 * line, the byte mask, the two planes of the distance transform, the carved count) belongs to the handle and grows with the map,
 * never with the number of calls.  The update is ordered behind every step in flight (on either env block) and in front of the next
 * one; it refreshes the out-of-bounds value in the handle's constants and in the device-side slot table of f110_set_env_maps, marks
 * the slot's cached render occupancy grid stale and leaves track data alone.  A derived obstacle slot of a re-carved base KEEPS ITS
 * OLD CONTENTS until it is re-stamped (f110_set_map_obstacles stamps from the base's table as it is then).
 * f110_corridor_mask_batch: the mask alone, for any frame (oc, os as the caller computed them), h_mask [H][W] 1 = carved, *h_carved
 * their number: what the tests compare cell for cell.
 * Refused (an error code, a message; nothing launched, nothing written, the slot list and the device allocations unchanged): null
 * arguments, M < 2 (M < 3 closed), M > F110_MAX_CORRIDOR_POINTS, a non-finite point or width, a negative width, a bad shape (sides
 * 1 .. 16384) or resolution or a non-finite origin, a map that does not fit the padded layout, a layout other than the padded one,
 * f110_set_map_corridor on a slot that was not carved.  Decided once the mask exists, before the distance transform runs or any table
 * is written: NO CELL CARVED (F110_ERR_INVALID; the count is reduced on the device and comes back with the call's one wait). */
enum { F110_MAX_CORRIDOR_POINTS = 65536 };
int f110_add_map_corridor(f110_sim *h, const double *h_xy, const double *h_half_width /* [S] */, int32_t M, int32_t closed,
                          int32_t H, int32_t W, double res, double ox, double oy, double oyaw, int32_t *slot);
int f110_set_map_corridor(f110_sim *h, int32_t slot, const double *h_xy, const double *h_half_width, int32_t M, int32_t closed);
int f110_corridor_mask_batch(f110_sim *h, const double *h_xy, const double *h_half_width, int32_t M, int32_t closed,
                             int32_t H, int32_t W, double res, double ox, double oy, double oc, double os,
                             uint8_t *h_mask /* [H][W], 1 = carved */, int64_t *h_carved);
/* the handle's last f110_add_map_corridor / f110_set_map_corridor by HIP events on its stream, milliseconds: ms [2] = the mask kernel
 * alone (the line already on the device, the mask staying there), the two passes of the distance transform (0 after a call that was
 * refused for carving nothing).  Waits for that call's distance transform (tools/trackgen_bench.py). */
int f110_map_corridor_times(f110_sim *h, double *ms /* [2] */);

/* Extension: a RACELINE AND SPEED PROFILE per closed line, ON THE DEVICE — the step from a centreline with half widths to
 * what a racing stack drives on.  Stateless unit form: T lines in one call, one workgroup per line, nothing kept in the handle.
 *
 * A line: M points q_i (indices modulo M) with a half width w_i >= 0 each.  The lines lie one after the other: xy [sum M][2],
 * half_width [sum M], offsets [T + 1] with offsets[0] = 0 and line t in rows offsets[t] .. offsets[t + 1].  float64 throughout, in
 * exactly this order, never contracted; clamp(x, lo, hi) = min(max(x, lo), hi).
 *   1. Frame.    d = q_{i+1} - q_{i-1};  l = sqrt(dx*dx + dy*dy);  n_i = (-dy / l, dx / l);  b_i = max(w_i - margin, 0).
 *   2. Offsets.  alpha = 0.  For lv = levels .. 0, s = 2^lv, the ACTIVE points are i = 0 (mod s):
 *        prolong (lv < levels only): for i = s (mod 2 s)   alpha_i = clamp(0.5 * (alpha_{i-s} + alpha_{i+s}), -b_i, b_i)
 *        y = alpha; then for k = 0 .. iters - 1 on the active points, every point from the values of the iteration before (Jacobi):
 *          p_j = q_j + y_j * n_j                                (per component)
 *          r_j = (p_{j-s} - 2 * p_j) + p_{j+s};   g_j = (r_{j-s} - 2 * r_j) + r_{j+s}
 *          gg  = 2 * (nx * gx + ny * gy);         new = clamp(y_j - 0.03125 * gg, -b_j, b_j)
 *          y_j = new + beta[k] * (new - alpha_j);  alpha_j = new
 *      Accelerated projected gradient on sum |r_j|^2, a box-constrained quadratic programme in alpha; the step 1/32 is 1 / (2 * 16):
 *      the Hessian is 2 N' D2' D2 N with |D2|^2 <= 16 and unit normals.  beta[k] = (t_k - 1) / t_{k+1}, t_0 = 1,
 *      t_{k+1} = (1 + sqrt(1 + 4 * t_k * t_k)) / 2 is the CALLER'S table (the device takes no square root in the loop); every level
 *      restarts at beta[0].  line_iters [T] (or NULL: iters for every line) gives a line fewer iterations; 0 leaves alpha = 0, the
 *      profile of the centreline itself.
 *   3. Line.     p_i = q_i + alpha_i * n_i.  kappa_i with a = p_{i-1}, b = p_i, c = p_{i+1}:
 *                  ab = b - a, bc = c - b, ac = c - a;  cross = abx * bcy - aby * bcx
 *                  kappa = 2 * cross / (sqrt(ab.ab) * sqrt(bc.bc) * sqrt(ac.ac))          (x.x = xx*xx + xy*xy; products left to right)
 *                len_i = |p_{i+1} - p_i|;  cum_0 = 0, cum_{i+1} = cum_i + len_i, L = cum_M: the running sum in order.
 *   4. Speed.    c_i = min(v_max * v_max, a_lat / |kappa_i|)                               (kappa = 0: inf, then v_max^2)
 *                ka = 2 * a_accel;  A_i = ka * cum_i;  F_i = c_i - A_i
 *                up_i = min(A_i + min_{j<=i} F_j, (A_i + ka * L) + min_{j>i} F_j)
 *                kb = 2 * a_brake;  B_i = kb * cum_i;  G_i = c_i + B_i
 *                um_i = min((min_{j>=i} G_j) - B_i, ((min_{j<i} G_j) + kb * L) - B_i)          (an empty minimum is +inf)
 *                vx_i = sqrt(min(c_i, min(up_i, um_i)))
 *                lap_time = sum of (2 * len_i) / (vx_i + vx_{i+1}), added in order.
 *      The forward / backward pass in v^2 once round the closed line, as prefix and suffix minima: exact under any evaluation order.
 * Outputs, written only when the whole call succeeds: alpha [sum M], xy [sum M][2] (the p_i), kappa, vx [sum M], length [T] (L),
 * lap_time [T].  Refused (F110_ERR_INVALID, a message; outputs untouched, the device allocations as they were): null arguments,
 * T < 1, offsets[0] != 0, levels outside 0 .. 6, iters outside 0 .. 4096, a line_iters entry outside 0 .. iters, a non-finite point,
 * half width or beta, v_max / a_lat / a_accel / a_brake not finite and > 0, margin not finite or < 0, and per line: M not a multiple
 * of 2^levels, M / 2^levels < 8 (the five-point stencil must not alias on the coarsest level), M > F110_RACELINE_MAX_POINTS, a
 * zero-length q_{i+1} - q_{i-1}; and, decided on the device once the solve has run, a raceline segment of zero length or a kappa_i
 * that is no finite number (p_{i+1} = p_{i-1}, or lengths whose product underflows).  So no NaN ever reaches a minimum of step 4:
 * min(a, b) there is the smaller of two numbers, and which operand an implementation returns for a NaN is not part of the rule.
 * Ordered behind every step in flight; one wait, at the end. */
enum { F110_RACELINE_MAX_POINTS = 4096 };
int f110_raceline_batch(f110_sim *h, const double *h_xy, const double *h_half_width, const int32_t *h_offsets /* [T + 1] */, int32_t T,
                        int32_t levels, int32_t iters, double margin, double v_max, double a_lat, double a_accel, double a_brake,
                        const double *h_beta /* [iters] */, const int32_t *h_line_iters /* [T] or NULL */,
                        double *h_alpha, double *h_out_xy, double *h_kappa, double *h_vx, double *h_length /* [T] */, double *h_lap_time /* [T] */);

/* Extension: a map slot's CENTRELINE LOOP, extracted ON THE DEVICE from the slot's distance table T (slot 0, an added
 * slot or a derived obstacle slot), as an ordered cycle of table cells with T at each: what a Track is made of (Track.from_map).
 *
 * The rule, in table coordinates (row 0 at the bottom, as the table is indexed).  Cell (r, c) is FREE iff T[r][c] > 0; cells
 * outside the table count as not free and not set.  The neighbours of (r, c):
 *   P2 = (r-1, c)  P3 = (r-1, c+1)  P4 = (r, c+1)  P5 = (r+1, c+1)  P6 = (r+1, c)  P7 = (r+1, c-1)  P8 = (r, c-1)  P9 = (r-1, c-1)
 * B = the number of set neighbours; A = the number of 0 -> 1 transitions in the cyclic sequence P2, P3, ..., P9, P2.  Every pass
 * is PARALLEL: all decisions of a pass read the mask as it was before that pass.
 *   1. Thinning (Zhang-Suen).  Start from the free mask; repeat the pair of sub-passes until a full pair deletes nothing.
 *      Sub-pass 1 deletes a set cell with 2 <= B <= 6, A == 1, P2*P4*P6 == 0 and P4*P6*P8 == 0; sub-pass 2 is the same with
 *      P2*P4*P8 == 0 and P2*P6*P8 == 0.
 *   2. Staircase removal.  Four passes, once each, in this order; each deletes the set cells that match its pattern:
 *      P2 & P4 set with P6, P7, P8 clear;  P4 & P6 set with P8, P9, P2 clear;  P6 & P8 set with P2, P3, P4 clear;
 *      P8 & P2 set with P4, P5, P6 clear.
 *   3. Spur pruning.  Repeat until a pass deletes nothing: delete every set cell with A <= 1 (dead ends down to their last stub,
 *      isolated cells, everything that is not on a cycle).
 *   4. The start, on the host, from the final mask and the free mask.  The seed is a world point (x, y); with the slot's resolution
 *      res, origin (ox, oy) and origin cosine / sine (oc, os), float64 in this order (the inverse of the stamp rule's transform):
 *        xt = x - ox, yt = y - oy;  xr = xt * oc + yt * os, yr = -xt * os + yt * oc
 *        inside iff xr >= 0 && xr < W * res && yr >= 0 && yr < H * res;  c = (int)(xr / res), r = (int)(yr / res)
 *      The seed cell must be free.  A breadth-first search from it over free cells, 8-connected, neighbours taken in the order
 *      P2 .. P9, visits cells in the order it reached them; the first set cell it visits is START.  A search that exhausts the
 *      seed's free component found no loop.
 *   5. The trace.  The set cells 8-connected to START must each have exactly two set neighbours, else the call is refused; they are
 *      walked into a cycle that begins at START.  With a heading theta the first step goes to the neighbour whose offset (dr, dc)
 *      has the larger dc * hx + dr * hy, (hx, hy) = (cos(theta) * oc + sin(theta) * os, -cos(theta) * os + sin(theta) * oc), a tie
 *      to the earlier neighbour in P2 .. P9; without one, in the direction that makes the cycle's signed area positive in world
 *      coordinates (counter-clockwise).
 * Components do not influence each other under this rule; the library thins the WHOLE free mask.  The loop's cell centres in world
 * coordinates are the stamp rule's (px, py) -> (wx, wy) above.
 *
 * max_passes <= 0: 4 * (H + W).  Thinning may take at most max_passes pairs of sub-passes and pruning at most max_passes passes,
 * the one that deletes nothing included.  h_deleted [3]: the cells thinning, staircase removal and pruning deleted (how often the
 * host looks at the counters does not show in them, nor anywhere else).  h_cells [cap][2] = (r, c), h_half_width [cap] = T at the
 * cell, in metres; *n (always written: 0 where the loop was not reached) the loop's length.  The call runs on the handle's main
 * stream behind every step in flight (on either env block) and returns when its results are on the host; scratch (three bit
 * planes of ceil(W / 64) * H words, the loop's cells and values) grows with the map, never with the number of calls, and only the
 * free mask's and the final mask's planes and the loop's values come back from the device.
 * Refused up front, with nothing launched, allocated or written but *n = 0 (F110_ERR_INVALID): null arguments, cap < 0, a slot out
 * of range, a side above 16384 cells, a non-finite seed or heading, a seed outside the table or on a cell that is not free (one
 * table value is read back for that).  Refused after the passes, with nothing written to h_cells, h_half_width and h_deleted:
 * thinning or pruning not converged within max_passes, no loop reachable from the seed, not a simple loop — the message carries
 * the number of cells with more than two neighbours (a map with islands has several loops that share cells: not supported)
 * (F110_ERR_STATE each); cap smaller than the loop (F110_ERR_INVALID, *n = the length needed).
 * f110_map_skeleton: the final mask of steps 1 - 3, h_mask [H][W] one byte per cell (1 set), and the three totals (h_deleted may be
 * NULL): what the tests compare cell for cell.
 * f110_slot_frame: frame [5] = res, ox, oy, oc, os of a slot as the library holds them (what turns the loop's cells into points). */
int f110_map_centerline(f110_sim *h, int32_t slot, double seed_x, double seed_y, int32_t has_heading, double seed_theta, int32_t max_passes,
                        int32_t *h_cells /* [cap][2] r, c */, double *h_half_width /* [cap] */, int32_t cap, int32_t *n, int64_t *h_deleted /* [3] */);
int f110_map_skeleton(f110_sim *h, int32_t slot, int32_t max_passes, uint8_t *h_mask /* [H][W] */, int64_t *h_deleted /* [3] or NULL */);
int f110_slot_frame(f110_sim *h, int32_t slot, double *frame /* [5] */);
/* the host's clock over the stages of the handle's last f110_map_centerline / f110_map_skeleton, milliseconds: ms [5] = (unused),
 * the free mask and thinning, staircase removal, pruning, and what follows the passes in f110_map_centerline (the two planes back,
 * the loop pick, the trace, the gather).  Every stage ends with a wait for its counters, so this is what the stage cost the caller
 * (tools/centerline_bench.py). */
int f110_map_centerline_times(f110_sim *h, double *ms /* [5] */);

/* Simulator.update_params base_classes.py:514-534 (agent_idx<0: all slots) */
int f110_set_params(f110_sim *h, int32_t agent_idx, const double *h_params18);
/* Extension (domain randomisation over vehicle dynamics): one parameter set per AGENT, h_params
 * [N][18] in the order of f110_config.params; NULL returns to the per-slot sets of f110_set_params
 * (which is refused while this is active).  As in the reference, the collision boxes keep the
 * constructor's length/width (base_classes.py:549) and the iTTC tables those of the first car. */
int f110_set_params_batch(f110_sim *h, const double *h_params);
/* scan noise, laser_models.py:450-452 with base_classes.py:204: row k is added to every
 * agent's scan on its k-th step after reset (rows wrap modulo n_rows).  n_rows=0: no noise. */
int f110_set_noise_table(f110_sim *h, const double *h_noise, int32_t n_rows, int32_t num_beams);
/* The same noise generated ON THE DEVICE: np.random.default_rng(seed).normal(0.,
 * std_dev, num_beams) per scan, laser_models.py:450-452 — NumPy's PCG64 stream through NumPy's
 * ziggurat, bit for bit — re-started for an agent whenever it is reset (base_classes.py:204).
 * Nothing is uploaded and memory stays flat however long the run is.
 *   h_state_inc, per_agent = 0: [4] = {state.hi, state.lo, inc.hi, inc.lo} of np.random.PCG64(seed)
 *       (f110_pcg64_seed computes them): one stream shared by every agent, as in the reference.  The
 *       first cache_rows rows (0: 16384) are generated once into a device row cache, extended on
 *       demand as episodes get longer; an agent whose episode outlives the cache continues from the
 *       stream position it carries.
 *   per_agent = 1: [N][4], a stream per agent (extension), always generated from the carried state.
 *   NULL: noise off.  Replaces any table of f110_set_noise_table, and vice versa. */
int f110_set_noise_rng(f110_sim *h, const uint64_t *h_state_inc, int32_t per_agent, double std_dev,
                       int32_t cache_rows);
/* np.random.PCG64(seed): SeedSequence(seed).generate_state(4, uint64) + pcg64_set_seed, host only;
 * seed < 2^64.  out4 = {state.hi, state.lo, inc.hi, inc.lo}. */
int f110_pcg64_seed(uint64_t seed, uint64_t *out4);
/* generate the shared stream's rows [0, rows) into the row cache now (instead of on demand) */
int f110_noise_prepare(f110_sim *h, int32_t rows);

/* Simulator.reset base_classes.py:614-630 / RaceCar.reset :183-204.
 * h_poses [N][3]; h_env_mask [num_envs] or NULL (all). */
int f110_reset(f110_sim *h, const double *h_poses, const uint8_t *h_env_mask);
int f110_reset_device(f110_sim *h, const double *d_poses, const uint8_t *d_env_mask);
/* in-place re-seat on the device, no host round trip: every env whose agent `ego_idx` has
 * collisions != 0 (the `done` condition of f110_env.py:244) is reset to d_start_poses [N][3];
 * *d_count (device int32, may be NULL) is incremented once per env reset. */
int f110_reset_collided_device(f110_sim *h, const double *d_start_poses, int32_t ego_idx,
                               int32_t *d_count);
/* The same re-seat folded into the end of every following f110_step / f110_step_device (one kernel
 * boundary less per step), until called again with d_start_poses = NULL.  State, delay buffer and
 * step counters end up exactly as after step + f110_reset_collided_device; in_collision keeps the
 * step's value (the separate call clears it). */
int f110_set_auto_reseat(f110_sim *h, const double *d_start_poses, int32_t ego_idx, int32_t *d_count);

/* ---- F110Env episode logic on the device: _check_done f110_env.py:204-246 (start/finish-zone
 * toggles, lap counts / times, done = ego collided or all agents have 4 toggles) and the state part
 * of reset() :319-334, so GPU-resident RL loops never read poses back to decide `done`.
 * f110_episode_reset also performs f110_reset for the masked envs.  h_rot [num_envs][4] is
 * start_rot (:331) row-major, computed by the host like the reference does. */
typedef struct f110_episode_host {
    double *lap_times, *lap_counts, *toggles; /* [N] */
    double *current_time;                     /* [num_envs] */
    uint8_t *near_starts;                     /* [N] */
    uint8_t *done;                            /* [num_envs] */
    uint8_t *checkpoint_done;                 /* [N] toggle_list >= 4 */
} f110_episode_host;
typedef struct f110_episode_views {
    uint8_t *done, *checkpoint_done;
    double *lap_times, *lap_counts, *toggles, *current_time;
} f110_episode_views;
int f110_episode_init(f110_sim *h, int32_t ego_idx);
int f110_episode_reset(f110_sim *h, const double *h_poses, const double *h_rot,
                       const uint8_t *h_env_mask);
/* (These two, like f110_pure_pursuit_device, keep a device-resident loop in its env blocks: behind a step that went out as two
 * env blocks — f110_config.step_groups — they run per block on the block's stream; an env's bookkeeping reads that env only.) */
int f110_episode_step_device(f110_sim *h, const double *d_actions); /* f110_step_device + _check_done */
int f110_episode_reset_done_device(f110_sim *h, int32_t *d_count);  /* re-seat envs whose done flag is set */
int f110_episode_get(f110_sim *h, const f110_episode_host *out);
/* One host round trip per step for host-side RL loops (F110VecEnv): h_actions [N][2] up, the step,
 * _check_done, every per-agent / per-env scalar of the observation down in ONE copy, then (auto_reset)
 * the in-place re-seat of the envs whose done flag is set.  h_packed (f110_episode_packed_bytes(h)
 * bytes; pinned memory from f110_host_alloc for a full-rate copy) receives
 *   double [9][N]  poses_x, poses_y, poses_theta, linear_vels_x, ang_vels_z, collisions,
 *                  lap_times, lap_counts, toggles
 *   double [E]     current_time
 *   uint8  [N] near_starts, [N] checkpoint_done, [E] done
 * — the observation of the step just taken (before any re-seat).  Scans stay in HBM. */
int f110_episode_step_host(f110_sim *h, const double *h_actions, int32_t auto_reset, void *h_packed);
size_t f110_episode_packed_bytes(const f110_sim *h);
int f110_host_alloc(f110_sim *h, size_t bytes, void **h_out);   /* page-locked host memory */
/* h may be NULL once the handle that allocated it is destroyed.  Must NOT run concurrently with a step (or any other call) on a
 * handle that uses the block: the call drains every live handle's stream and drops their cached views of the block without
 * taking a per-handle lock — the caller serialises it against those handles like any other call on them. */
int f110_host_free(f110_sim *h, void *h_ptr);
int f110_episode_device_views(f110_sim *h, f110_episode_views *out);

/* env.step() of a host-driven loop as ONE call (replaces, per step, F110Env.step -> Simulator.step's agent
 * loops + observation dict base_classes.py:553-612 and, once f110_episode_init was called, _check_done
 * f110_env.py:204-246 and the re-seat of reset() :319-334): actions up, the step, the episode logic, and the
 * requested observation columns written by one kernel straight into the caller's PAGE-LOCKED memory
 * (f110_host_alloc — required: the kernel stores into it in place; anything else is refused with
 * F110_ERR_INVALID), scans by one DMA copy behind it.  Any pointer may be NULL = not wanted.  The episode
 * columns and F110_STEP_AUTO_RESET need f110_episode_init (else F110_ERR_STATE).  The block holds the
 * observation of the step just taken; with F110_STEP_AUTO_RESET finished envs (done != 0) are re-seated
 * at their start poses AFTER it was written, and the device-side done flag is cleared. */
typedef struct f110_host_block {
    double *state;            /* [7][N] columns x, y, steer, v, yaw, yaw_rate, slip (poses_x = row 0, ...) */
    double *collisions;       /* [N] */
    double *collision_idx;    /* [N] */
    double *agent_poses;      /* [3][N] Simulator.agent_poses (:574 snapshot) */
    double *lap_times;        /* [N] */
    double *lap_counts;       /* [N] */
    double *toggles;          /* [N] */
    double *current_time;     /* [E] */
    int32_t *in_collision;    /* [N] */
    uint8_t *near_starts;     /* [N] */
    uint8_t *checkpoint_done; /* [N] */
    uint8_t *done;            /* [E] */
    double *scans;            /* [N][B] (any host memory; page-locked for a full-rate copy) */
} f110_host_block;
#define F110_STEP_AUTO_RESET 1      /* re-seat finished envs inside the call */
#define F110_STEP_NO_SYNC 2         /* return once everything is enqueued: f110_sync(h) completes the block
                                       (gym.vector's step_async / step_wait split) */
#define F110_STEP_ACTIONS_MAPPED 4  /* h_actions is f110_host_alloc memory: read in place, no staging copy */
#define F110_STEP_SPIN_WAIT 8       /* wait by polling a page-locked completion word the last workgroup stores,
                                       instead of a runtime synchronise (ignored with scans / NO_SYNC) */
#define F110_STEP_POLL 32           /* wait by polling hipStreamQuery (a busy core, ~1 us wake-up) instead of
                                       hipStreamSynchronize (coarse wake-up quanta beyond ~30 us of waiting); the poll is
                                       bounded: after 250 us the call sleeps in hipStreamSynchronize */
#define F110_STEP_NO_FUSE 16        /* A/B: always run the episode logic + host block as a kernel of their own (with 2
                                       agents per env they are otherwise the finalize kernel's epilogue) */
#define F110_STEP_SCRIPTED 64       /* scripted cars (f110_controllers_set, below): h_actions is staged into device memory (as
                                       without F110_STEP_ACTIONS_MAPPED, which is ignored), the armed controllers overwrite their
                                       agents' rows there from the scans of the last step, and the step runs from that buffer.
                                       Armed line followers (f110_line_followers_set, below) then write theirs, and an armed
                                       planner (f110_mppi_set, below) its agents' rows behind them.
                                       The one-launch form of tiny batches does not apply.  F110_ERR_STATE with none of the
                                       three kinds armed.  Without the flag the call looks at none of them. */
int f110_step_host(f110_sim *h, const double *h_actions /* [N][2] */, const f110_host_block *out, int32_t flags);
/* measurement aid: {calls, host microseconds spent enqueuing, host microseconds spent waiting} of the
 * f110_step_host calls since the last read (cleared by the read) */
int f110_step_host_stats(f110_sim *h, double *out3);

/* Simulator.step base_classes.py:553-612.  actions [N][2] = (steer, speed).
 * Asynchronous on the handle's stream; outputs are read with f110_get_* (which sync). */
int f110_step(f110_sim *h, const double *h_actions);
int f110_step_device(f110_sim *h, const double *d_actions);

/* observation / state read-back (device -> host).  Any pointer may be NULL. */
typedef struct f110_obs_host {
    double *scans;          /* [N][B]  obs['scans'] */
    double *poses_x;        /* [N] */
    double *poses_y;        /* [N] */
    double *poses_theta;    /* [N] */
    double *linear_vels_x;  /* [N] */
    double *ang_vels_z;     /* [N] */
    double *collisions;     /* [N]  GJK flag OR wall flag (base_classes.py:588-589) */
    double *collision_idx;  /* [N]  collision_models.py:184-212 */
    double *state;          /* [N][7] RaceCar.state */
    double *agent_poses;    /* [N][3] Simulator.agent_poses (:574 snapshot) */
    int32_t *in_collision;  /* [N]  RaceCar.in_collision */
    int32_t *step_count;    /* [N]  steps since reset */
} f110_obs_host;
int f110_get_obs(f110_sim *h, const f110_obs_host *out);
/* A PARTIAL setter: RaceCar.state, the steering delay FIFO and its count, nothing else.  It leaves step_count (which picks the
 * noise row), in_collision / collisions / collision_idx / agent_poses, the agents' noise-stream positions, the episode arrays and
 * the host's bound on the steps since the last full reset as they are — a batch "restored" this way diverges at its first noisy
 * scan.  The exact snapshot / restore / clone of every column is f110_state_* / f110_clone_envs_device below. */
int f110_set_state(f110_sim *h, const double *h_state7 /* [N][7] */,
                   const double *h_steer_buf /* [N][2] newest first, or NULL */,
                   const int32_t *h_buf_count /* [N] or NULL */);

/* ---- exact snapshot, restore and clone of the simulator state (save / resume, roll-back, branching; the reference deep-copies
 * its Python objects, base_classes.py:98-112, f110_env.py:165-189).  A blob is a 256-byte header followed by one section per
 * column, [column][k * A] for per-agent columns and [column][k] for per-env ones (k = envs in the blob), each section 256-byte
 * aligned.  It carries, per agent: state[7], the steer FIFO [2] and its count, agent_poses[3], collisions, collision_idx,
 * in_collision, step_count, the noise-stream position (any device noise) and seed (per-agent streams); per env, once
 * f110_episode_init has run: start poses, start_rot[4], current_time, done and per agent near_start, toggle, lap_count, lap_time,
 * checkpoint; the [A][18] rows of f110_set_params_batch and the env's map slot while those are active; optionally
 * (F110_STATE_SCANS) the last scans [k * A][B].  NOT carried — configuration the target must already have: the maps and their
 * slots' tables, the beam / trig tables, the per-slot params, the noise table or seed, the auto re-seat poses.
 * Header (little-endian): char magic[8] "F110SNAP"; uint32 version (F110_STATE_VERSION); int32 k, A, B, flags; uint32 columns
 * (F110_STATE_COL_*); int32 noise_mode (0 off, 1 table, 2 shared PCG64 stream, 3 a stream per agent), noise_rows, n_maps,
 * ego_idx; int64 max_step (>= every step_count in the blob); uint64 noise_id[4] (shared stream: the PCG64 words of
 * f110_set_noise_rng; table: {FNV-1a 64 of its bytes, rows, B, 0}); double std_dev; uint64 total_bytes; zeros to 256.
 * A load refuses (F110_ERR_STATE, with a message) a blob of another version, A or B, another noise source, or a column set other
 * than the columns active on the target (episode, params, env map, noise); E may differ: entries are per env.  After a load
 * the host's bound on the steps since the last full reset covers every restored step_count, so the noise row cache grows as
 * far as the restored episodes need.  Every call joins a two-block step first; a save is stream-ordered behind the step before
 * it and a load in front of the step after it.  Out-of-range indices of the device forms are skipped (nothing is read or written
 * out of bounds) and counted into *d_status (device int32, may be NULL); a dst named twice is undefined there.
 * f110_clone_envs_device: env src[j] -> env dst[j] in one launch, no blob — src and dst must be disjoint. */
#define F110_STATE_VERSION 1
#define F110_STATE_SCANS 1            /* flags: the blob also holds the last scans */
enum {
    F110_STATE_COL_AGENT = 1,         /* state, steer FIFO, count, agent_poses, collision flags, step_count (always) */
    F110_STATE_COL_SCANS = 2,
    F110_STATE_COL_RNG = 4,           /* noise-stream position per agent (device noise) */
    F110_STATE_COL_RNG_SEED = 8,      /* per-agent streams: the seed words */
    F110_STATE_COL_EPISODE = 16,
    F110_STATE_COL_PARAMS = 32,       /* f110_set_params_batch rows */
    F110_STATE_COL_ENV_MAP = 64,      /* f110_set_env_maps slot */
    F110_STATE_COL_RESET_RNG = 128,   /* f110_reset_sampler_set: per env its stream {state, inc}, per agent its fallback pose */
    F110_STATE_COL_PARAM_RNG = 256    /* f110_param_sampler_set: per env its stream {state, inc} (the rows travel as F110_STATE_COL_PARAMS) */
};
#define F110_STATE_HEADER_BYTES 256
/* bytes of a blob of n_envs envs (the handle's current column set) */
size_t f110_state_bytes(const f110_sim *h, int32_t n_envs, int32_t flags);
/* envs d_env_idx[0..k) (NULL: every env, k must be num_envs) -> the device blob d_blob (16-byte aligned), asynchronous */
int f110_state_save_device(f110_sim *h, const int32_t *d_env_idx, int32_t k, void *d_blob, int32_t flags);
/* blob entry d_src[j] (NULL: j) -> env d_dst[j] (NULL: j), j < k; several dst may name one src.  Reads the header (a small
 * synchronous copy), then asynchronous. */
int f110_state_load_device(f110_sim *h, const void *d_blob, const int32_t *d_src, const int32_t *d_dst, int32_t k, int32_t *d_status);
int f110_clone_envs_device(f110_sim *h, const int32_t *d_src, const int32_t *d_dst, int32_t k, int32_t *d_status);
/* the whole handle to / from host memory (f110_state_bytes(h, num_envs, flags) bytes; f110_host_alloc memory for a full-rate
 * copy); both return once the copy is complete */
int f110_state_save(f110_sim *h, void *h_blob, int32_t flags);
int f110_state_load(f110_sim *h, const void *h_blob);

/* device-resident observation buffers (valid until f110_destroy; contents valid after the
 * step that produced them completes on the stream).  SoA columns of N doubles. */
typedef struct f110_device_views {
    double *scans;        /* [N][B] */
    double *state;        /* [7][N] columns x, y, steer, v, yaw, yaw_rate, slip */
    double *agent_poses;  /* [3][N] */
    double *collisions;   /* [N] */
    double *collision_idx;
    int32_t *in_collision;
    int32_t *step_count;
    void *stream;         /* hipStream_t */
} f110_device_views;
int f110_get_device_views(f110_sim *h, f110_device_views *out);
/* Hand f110_device_views.stream to EXTERNAL work (a torch / cupy stream wrapped around it, a user kernel) safely: everything the
 * handle has in flight — including the second env block of a two-block step, which runs on a stream of its own — is ordered in
 * front of what the caller enqueues on that stream next, and the following f110_*step* is submitted as ONE block on that stream,
 * i.e. behind the caller's work (its reads of the observation, its writes of the action buffer).  Call it once per iteration
 * between the handle's last call and the external work; it enqueues two event waits and never blocks the host.  Without it only
 * one-block steps (f110_config.step_groups = 1, or any handle that synchronises every step) are ordered against that stream. */
int f110_stream_fence(f110_sim *h);
/* free / total bytes of the handle's GPU (hipMemGetInfo) — lets a long run show that memory stays flat */
int f110_device_mem_info(f110_sim *h, size_t *free_bytes, size_t *total_bytes);
int f110_device_alloc(f110_sim *h, size_t bytes, void **d_out);
int f110_device_free(f110_sim *h, void *d_ptr);
int f110_memcpy_h2d(f110_sim *h, void *d_dst, const void *h_src, size_t bytes);
int f110_memcpy_d2h(f110_sim *h, void *h_dst, const void *d_src, size_t bytes);

/* ---- optional observation gather over RCCL / xGMI (BASELINE config 4; off the step path) ----
 * Environments never interact, so stepping needs no collective.  A consumer that wants every
 * rank's scans on every GPU creates one communicator (rank 0 makes the id, the launcher's control
 * plane broadcasts its 128 bytes) and calls f110_comm_all_gather_scans after a step: an
 * ncclAllGather of [N][B] float64 per rank, enqueued on the handle's stream.
 * d_recv: device buffer of n_ranks*N*B doubles. */
#define F110_COMM_ID_BYTES 128
int f110_comm_unique_id(void *out_id128);
int f110_comm_init(f110_sim *h, int32_t n_ranks, int32_t rank, const void *id128);
int f110_comm_all_gather_scans(f110_sim *h, void *d_recv);
/* The whole observation of Simulator.step (base_classes.py:594-610; SURVEY 8e: "scans [N_g,B] + 7
 * scalars/agent"): the scans as above AND the per-agent scalars, packed by a kernel behind the step as
 * double [F110_OBS_SCALARS][N] = poses_x, poses_y, poses_theta, linear_vels_x, linear_vels_y (always
 * 0., :603), ang_vels_z, collisions — two ncclAllGather calls inside ONE ncclGroupStart / End.
 * d_recv_scans: n_ranks*N*B doubles; d_recv_scalars: n_ranks*F110_OBS_SCALARS*N doubles (rank-major).
 * Honours f110_comm_set_overlap exactly like f110_comm_all_gather_scans (the scalar block is
 * double-buffered with the scans). */
#define F110_OBS_SCALARS 7
int f110_comm_all_gather_obs(f110_sim *h, void *d_recv_scans, void *d_recv_scalars);
/* The same gather with the two knobs SURVEY 8e prices: transport F110_GATHER_F32 sends the scans as float32 (a
 * conversion kernel in front of the collective; d_recv_scans then holds n_ranks*N*B FLOATS; the scalars stay
 * float64) — 142 MB instead of 283 MB per rank and step at 32 768 agents; root >= 0 gathers to that rank only
 * (grouped ncclSend / ncclRecv: every peer's block rides its one direct link to the root, the other ranks
 * receive nothing; their d_recv_scans may be NULL, and they pass a non-NULL d_recv_scalars — never written —
 * exactly when the root wants the scalar blocks), root = -1 is the all-gather above.  Honours
 * f110_comm_set_overlap. */
#define F110_GATHER_F64 0
#define F110_GATHER_F32 1
int f110_comm_gather_obs(f110_sim *h, void *d_recv_scans, void *d_recv_scalars, int32_t transport, int32_t root);
/* how the step is submitted (f110_config.step_groups): *groups = env blocks the handle can submit a step as (2 = two halves of
 * the envs on two streams that were OBSERVED to run next to each other when the handle was created; 1 = one block),
 * *probes = candidate streams that observation tried, *last = blocks the most recent f110_step_device was submitted as.
 * Any pointer may be NULL.  Bookkeeping for benchmarks and tests; no reference counterpart. */
int f110_step_groups(f110_sim *h, int32_t *groups, int32_t *probes, int32_t *last);
/* *launches = 1 when the most recent step ran as ONE kernel launch (round 6: a waiting f110_step_host of at most 4 agents with one or two
 * cars per env — the reference's own shape, F110Env(num_agents = 1 | 2) on one env — integrate, scan, finalize, the observation block and
 * the completion word in a single launch, k_step_tiny; results are the same bits), 0 = the per-kernel form.  Bookkeeping for
 * benchmarks and tests; no reference counterpart. */
int f110_step_launches(f110_sim *h, int32_t *launches);
/* size and rank of the communicator as RCCL itself reports them (ncclCommCount / ncclCommUserRank) */
int f110_comm_info(f110_sim *h, int32_t *n_ranks, int32_t *rank);
/* enable = 1: the gather OVERLAPS the following step.  The scans are double-buffered (a second
 * [N][B] buffer): f110_comm_all_gather_scans then runs on a stream of its own behind the step that
 * produced the current buffer, the next f110_step* fills the other buffer, and the step after that
 * waits for the gather before reusing the first.  While enabled, f110_device_views.scans alternates
 * between the two buffers (fetch it after each step); d_recv must not be reused by the caller before
 * the data has been consumed (alternate two receive buffers).  Any other call on the handle
 * (f110_sync, f110_get_obs, f110_memcpy_d2h, ...) first makes the main stream wait for outstanding
 * gathers. */
int f110_comm_set_overlap(f110_sim *h, int32_t enable);
int f110_comm_destroy(f110_sim *h);

/* HIP-event timing on the handle's stream (bench.py roofline leg).
 * f110_timer_begin/_end bracket a region; f110_profile_kernels(1) additionally brackets
 * every scan-kernel launch inside f110_step with its own event pair. */
int f110_timer_begin(f110_sim *h);
int f110_timer_end_ms(f110_sim *h, double *ms);
int f110_profile_kernels(f110_sim *h, int32_t enable);
int f110_profile_read(f110_sim *h, int32_t *n_launches, double *scan_ms_total,
                      double *dyn_ms_total, double *finalize_ms_total);

/* ---- unit entry points (one per reference kernel; used by the parity tests) ---- */
/* ScanSimulator2D.scan(pose, None)  laser_models.py:429-454 -> get_scan :148-186.
 * h_ranges [M][B]; h_hit_rc [M][B][2] (r,c) of the terminating sample or NULL;
 * h_lookups [M] table lookups per pose or NULL. */
int f110_scan_batch(f110_sim *h, const double *h_poses, int32_t m, double *h_ranges,
                    int32_t *h_hit_rc, int64_t *h_lookups);
/* examples/waypoint_follow.py:15-217 — PurePursuitPlanner.plan (nearest point on the waypoint
 * polyline, first look-ahead-circle cut with wrap-around, get_actuation), the reference's example
 * policy, so that a closed loop can stay on the GPU.  waypoints [M][3] = (x, y, speed) as the
 * planner reads them through conf.wpt_xind / wpt_yind / wpt_vind; actions [.][2] = (steer, speed),
 * the layout f110_step takes.  _batch: host poses [m][3]; _device: the live poses of all N agents
 * (observation poses_x / poses_y / poses_theta), device pointers, asynchronous on the handle's stream. */
int f110_pure_pursuit_batch(f110_sim *h, const double *h_waypoints, int32_t M, const double *h_poses,
                            int32_t m, double lookahead, double vgain, double wheelbase,
                            double max_reacquire, double *h_actions);
int f110_pure_pursuit_device(f110_sim *h, const double *d_waypoints, int32_t M, double lookahead,
                             double vgain, double wheelbase, double max_reacquire, double *d_actions);
/* _poses_device: the same policy for all N agents on poses the caller holds in device memory, d_poses [N][3] float64 = (x, y,
 * theta) — a particle filter's estimates (f110_pf_device), say — instead of the live poses.  A row whose pose is NaN gets
 * (0, 4.0), the policy's answer when it finds no waypoint.  Asynchronous, per env block behind a two-block step. */
int f110_pure_pursuit_poses_device(f110_sim *h, const double *d_waypoints, int32_t M, const double *d_poses, double lookahead,
                                   double vgain, double wheelbase, double max_reacquire, double *d_actions);
/* A reactive policy that CONSUMES the step's scans on the device (NOT a reference function: the stand-in for an RL policy in
 * a device-resident loop — examples/rl_loop_device.py, bench.py's "scans consumed on device" leg).  Per agent: the num_beams
 * ranges in 64 sectors, steer = clamp(steer_gain * centre angle of the sector with the largest mean range among those within
 * sector_limit rad of straight ahead, +-steer_max), speed = v_lo + (v_hi - v_lo) * min(1, shortest range of the eight middle
 * sectors / d_ref).  Reads the observation of the step just taken (f110_get_device_views().scans), writes d_actions [N][2] =
 * (steer, speed) — the layout f110_step_device takes; asynchronous on the handle's stream (per env block behind a two-block step). */
int f110_scan_policy_device(f110_sim *h, double steer_gain, double steer_max, double sector_limit, double v_lo,
                            double v_hi, double d_ref, double *d_actions);
/* Diagnostics of the scan kernels (step and unit form): with enable = 1 every marched ray is counted
 * as {fixed-point march on the padded table, re-marched exactly after a guard-band sample, exact
 * because the lidar is off the padded table / the layout has no fast path}.  out3 (or NULL) receives
 * and clears the counters; enable = -1 leaves the switch as it is.  Off by default (atomics). */
int f110_scan_path_stats(f110_sim *h, int32_t enable, int64_t *out3);
/* vehicle_dynamics_st / vehicle_dynamics_ks  dynamic_models.py:90-176; x [M][7], u [M][2] */
int f110_dynamics_batch(f110_sim *h, const double *h_x, const double *h_u,
                        const double *h_params18, int32_t m, double *h_f_st, double *h_f_ks);
/* pid  dynamic_models.py:178-221; in [M][4] = (speed, steer, current_speed, current_steer) */
int f110_pid_batch(f110_sim *h, const double *h_in, const double *h_params18, int32_t m,
                   double *h_accl_sv /* [M][2] */);
/* RaceCar.update_pose  base_classes.py:256-409 (without the scan) */
int f110_update_pose_batch(f110_sim *h, const double *h_state0, const double *h_buf0,
                           const int32_t *h_cnt0, const double *h_actions,
                           const double *h_params18, double time_step, int32_t integrator,
                           double lidar_dist, int32_t m, double *h_state1, double *h_buf1,
                           int32_t *h_cnt1, double *h_scan_pose);
/* get_vertices collision_models.py:237-260; poses [M][3] -> [M][4][2] */
int f110_get_vertices_batch(f110_sim *h, const double *h_poses, double length, double width,
                            int32_t m, double *h_vertices);
/* collision (GJK) collision_models.py:113-182 on M pairs of [4][2] */
int f110_gjk_batch(f110_sim *h, const double *h_va, const double *h_vb, int32_t m,
                   int32_t *h_flags);
/* collision_multiple :184-212 on G groups of n bodies [G][n][4][2] */
int f110_collision_multiple_batch(f110_sim *h, const double *h_vertices, int32_t groups,
                                  int32_t n, double *h_collisions, double *h_collision_idx);
/* check_ttc_jit laser_models.py:188-217 on M scans [M][B] with the handle's beam tables */
int f110_ttc_batch(f110_sim *h, const double *h_scans, const double *h_vels, int32_t m,
                   double ttc_thresh, int32_t *h_flags);
/* ray_cast laser_models.py:318-346 (+ get_blocked_view_indices :282-315) on M cases:
 * ego pose [M][3], opponent vertices [M][4][2], scans in/out [M][B], window [M][2] or NULL */
int f110_raycast_batch(f110_sim *h, const double *h_ego, const double *h_vertices, int32_t m,
                       double *h_scans_inout, int32_t *h_min_max_ind);
/* get_range laser_models.py:249-280; in [M][8] = (pose3, beam_theta, va2, vb2) */
int f110_get_range_batch(f110_sim *h, const double *h_in, int32_t m, double *h_out);
/* exact squared EDT of a binary image (nonzero = free), laser_models.py:40-53 */
int f110_edt_sq(f110_sim *h, const uint8_t *h_img, int32_t height, int32_t width,
                uint32_t *h_d2);
/* get_dt laser_models.py:40-53: dt = resolution * scipy.ndimage.distance_transform_edt(bitmap) — h_bitmap [height][width]
 * uint8, nonzero = free space (what edt treats as foreground), as the array is (no flip, no threshold); exact EDT on the
 * device, h_dt [height][width] float64. */
int f110_dt_from_bitmap(f110_sim *h, const uint8_t *h_bitmap, int32_t height, int32_t width, double resolution, double *h_dt);
/* The remaining small functions that `from f110_gym.envs import *` exposes in the reference (envs/__init__.py:2-5), M items per
 * call, one thread each, in the reference's expression order.  h_in [M][in_width(op, n)], h_out [M][out_width(op)]; n = vertices
 * per body for the ops that take bodies (the reference calls them with 4), ignored otherwise.
 *   op                          reference                        in (doubles per item)                                   out
 *   F110_OP_ACCL_CONSTRAINTS    dynamic_models.py:29-60          vel, accl, v_switch, a_max, v_min, v_max                  accl
 *   F110_OP_STEERING_CONSTRAINT dynamic_models.py:62-87          steering_angle, steering_velocity, s_min, s_max, sv_min, sv_max   steering_velocity
 *   F110_OP_CROSS               laser_models.py:219-230          v1[2], v2[2]                                              cross product
 *   F110_OP_ARE_COLLINEAR       laser_models.py:232-247          pt_a[2], pt_b[2], pt_c[2]                                 0. / 1.
 *   F110_OP_PERPENDICULAR       collision_models.py:34-48        pt[2]                                                     [2]
 *   F110_OP_TRIPLE_PRODUCT      collision_models.py:51-64        a[2], b[2], c[2]                                          [2]
 *   F110_OP_AVG_POINT           collision_models.py:67-78        vertices[n][2]                                            [2]
 *   F110_OP_FURTHEST_POINT      collision_models.py:81-92        vertices[n][2], d[2]                                      index (as a double)
 *   F110_OP_SUPPORT             collision_models.py:95-110       vertices1[n][2], vertices2[n][2], d[2]                    [2]
 *   F110_OP_GET_TRMTX           collision_models.py:218-235      pose[3]                                                   H[4][4] row-major
 *   F110_OP_XY_2_RC             laser_models.py:55-86            x, y, orig_x, orig_y, orig_c, orig_s, height, width, resolution   r, c (as doubles; -1, -1 out of bounds)
 *   F110_OP_DISTANCE_TRANSFORM  laser_models.py:88-104           x, y  (the handle's map: f110_set_map_*)                  dt[r, c] (dt[-1, -1] out of bounds)
 *   F110_OP_TRACE_RAY           laser_models.py:106-146          x, y, theta_index  (the handle's map, trig tables, eps, max_range)   range
 * (get_scan = f110_scan_batch, get_range = f110_get_range_batch, get_blocked_view_indices = the window of f110_raycast_batch,
 * get_dt = f110_dt_from_bitmap, the rest of the star-exports have had entry points since round 1.) */
enum {
    F110_OP_ACCL_CONSTRAINTS = 1, F110_OP_STEERING_CONSTRAINT, F110_OP_CROSS, F110_OP_ARE_COLLINEAR, F110_OP_PERPENDICULAR,
    F110_OP_TRIPLE_PRODUCT, F110_OP_AVG_POINT, F110_OP_FURTHEST_POINT, F110_OP_SUPPORT, F110_OP_GET_TRMTX, F110_OP_XY_2_RC,
    F110_OP_DISTANCE_TRANSFORM, F110_OP_TRACE_RAY
};
int f110_helper_batch(f110_sim *h, int32_t op, const double *h_in, int32_t m, int32_t n, double *h_out);
/* rng.normal(0., std_dev, num_beams) drawn `rows` times in a row from the PCG64 state h_state_inc4
 * (numpy/random/src/distributions/distributions.c random_standard_normal; laser_models.py:450-452):
 * h_out [rows][num_beams]; h_state_out2 (or NULL) = {state.hi, state.lo} after the last draw */
int f110_noise_rows_batch(f110_sim *h, const uint64_t *h_state_inc4, double std_dev, int32_t rows,
                          int32_t num_beams, double *h_out, uint64_t *h_state_out2);
/* Measurement aid (bench.py's L-bar): with enable = 1 the step's scan kernels sum the table lookups
 * of every ray they march (the reference's dependent gathers, laser_models.py:129-143).  out2 (or
 * NULL) receives and clears {the sum, 0 (round 1-4: how many of them the retired LDS-window layout served)};
 * enable = -1 leaves the switch as it is.  Off by default. */
int f110_scan_lookup_count(f110_sim *h, int32_t enable, int64_t *out2);
/* table index int(theta_index) of every beam for M headings (get_scan :167-184) */
int f110_beam_dir_index_batch(f110_sim *h, const double *h_thetas, int32_t m, int32_t *h_idx);

/* ---- track progress (no reference counterpart: what racing RL setups built on the reference compute on the host) ----
 * A track is a polyline of M points (x, y) in map coordinates, attached to a map slot (0 = f110_set_map_*, 1.. = f110_add_map_*).
 * closed != 0 adds the segment M-1 -> 0; a closed track whose last point equals its first bitwise drops that repeat first.
 * Refused (F110_ERR_INVALID): M < 2 (M < 3 closed), non-finite points, a zero-length segment (the closing one included).
 * Projection = examples/waypoint_follow.py:15-50 nearest_point_on_trajectory (first segment with the smallest distance, t clipped
 * to [0, 1]).  Per agent: s = cum[k] + t len[k] (metres along the track), lateral = signed distance to the projection (> 0 left of
 * the segment direction), heading_error = wrap(theta - atan2(dy, dx)) into [-pi, pi), segment = k, ds = s(after) - s(before) of the
 * step just taken (closed: wrapped into (-L/2, L/2]).  The columns belong to the observation of the step: computed from the same
 * post-step pose as poses_x / poses_y / poses_theta, before any in-step re-seat.  "before" is a per-agent cache of s and the pose it
 * was computed from, used only while that pose equals the current one bitwise (else the agent is re-projected at the head of the
 * step), so every pose writer (resets, re-seats, f110_set_state, state loads, clones) is covered without knowing about tracks. */
int f110_track_set(f110_sim *h, int32_t slot, const double *h_xy /* [M][2] */, int32_t M, int32_t closed);
/* on != 0: every step entry point also produces the track columns.  F110_ERR_STATE (at this call or at the next step) while an
 * env is assigned to a slot without a track.  Off by default: the step is then exactly what it is without tracks. */
int f110_track_enable(f110_sim *h, int32_t on);
struct f110_track_views {   /* (a struct tag, no typedef: the entry point below has the same name) */
    double *s;              /* [N] device pointers, stable for the life of the handle */
    double *ds;             /* [N] */
    double *lateral;        /* [N] */
    double *heading_error;  /* [N] */
    int32_t *segment;       /* [N] */
};
int f110_track_views(f110_sim *h, struct f110_track_views *out);
typedef struct f110_track_host {
    double *s;              /* [N] any pointer may be NULL */
    double *ds;
    double *lateral;
    double *heading_error;
    int32_t *segment;
} f110_track_host;
/* host copy of the last step's columns (synchronous) */
int f110_track_get(f110_sim *h, const f110_track_host *out);
/* page-locked destinations (f110_host_alloc) f110_step_host fills alongside its host block, with the block's completion
 * semantics; NULL (or every pointer NULL) unregisters */
int f110_track_host_block(f110_sim *h, const f110_track_host *pinned);
/* unit form: h_poses [m][3] on the track of `slot`; h_out [m][5] = s, lateral, heading_error, segment, t */
int f110_track_project_batch(f110_sim *h, int32_t slot, const double *h_poses, int32_t m, double *h_out);

/* ---- randomised start poses (no reference counterpart: training setups built on the reference pick a random waypoint, add
 * lateral / heading jitter, check the spot is free and call reset(poses) on the host).  A reset sampler draws an env's start
 * poses on the track of its map slot (f110_track_set; every env's slot must have one: F110_ERR_STATE at arming, or at the next
 * call that would draw).  Env e owns one PCG64 stream, np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(e,))) with e the
 * GLOBAL env index (f110_pcg64_seed_spawn), uniforms = Generator.random().  One draw, A agents, track length L, segments
 * (ax, ay, dx, dy, len, cum), float64 without contraction, every attempt consuming exactly 1 + 2A uniforms in this order:
 *   s0 = L * (s_lo + u * (s_hi - s_lo)); per agent j: s = s0 - j * gap (closed: s = fmod(s, L), + L when < 0), u_l, u_h,
 *   d = lateral * (2 u_l - 1), h = heading * (2 u_h - 1), k = the last segment with cum[k] <= s (0 when none),
 *   t = clip((s - cum[k]) / len[k], 0, 1), x = (ax + t dx) + d * (-dy / len), y = (ay + t dy) + d * (dx / len),
 *   theta = atan2(dy, dx) + h  (the device's atan2: within an ulp of NumPy's).
 *   Valid: every agent on the track (open: s >= 0), inside its slot's map (xy_2_rc) with dt[r][c] >= clearance, every pair
 *   (xi - xj)^2 + (yi - yj)^2 >= (2 clearance)^2.  The first valid attempt wins; none: a fallback (counted).
 * Explicit draw (f110_reset_sample*): f110_reset of the env to the drawn poses (and f110_episode_reset once f110_episode_init ran,
 * start_rot computed on the device: within an ulp of NumPy's cos / sin); on a fallback to the poses of the env's last reset of any
 * kind while the sampler was armed (zeros before the first one).
 * In-step draw: every call that re-seats envs (f110_set_auto_reseat, f110_reset_collided_device, the auto reset of
 * f110_step_host / f110_episode_step_host, f110_episode_reset_done_device) draws for the envs it re-seated, behind its last
 * kernel (per env block behind a two-block step), stream-ordered in front of the next call; the env ends as the re-seat would
 * have left it had its start poses been the drawn ones, with episode logic also start poses and start_rot; a fallback keeps the
 * re-seat's pose and the start columns.  Observations already written (the host block) stay the pre-re-seat ones.
 * Without a sampler nothing of this runs.  The stream position is state (F110_STATE_COL_RESET_RNG); the settings are configuration. */
typedef struct f110_reset_sampler {
    double s_lo, s_hi;     /* fractions of the track length, 0 <= s_lo < s_hi <= 1 */
    double gap;            /* metres between consecutive agents along the track, > 0 */
    double lateral;        /* largest lateral offset (m), >= 0 */
    double heading;        /* largest heading jitter (rad), >= 0 */
    double clearance;      /* metres, >= 0 */
    int32_t attempts;      /* 1 .. 1024 */
    int32_t pad;
} f110_reset_sampler;
/* {state.hi, state.lo, inc.hi, inc.lo} of PCG64(SeedSequence(entropy, spawn_key=(e,))) for e = e0 .. e0 + n - 1, host only:
 * h_entropy = the seed as NumPy's SeedSequence assembles it (little-endian uint32 words of an int, the words of every element
 * of a sequence one after the other), n_words >= 1 (a seed of 0 is the one word 0).  out [n][4]. */
int f110_pcg64_seed_spawn(const uint32_t *h_entropy, int32_t n_words, uint64_t e0, int32_t n, uint64_t *h_out);
/* arm (spec != NULL; h_streams [num_envs][4] from f110_pcg64_seed_spawn) or disarm (spec = NULL).  Out-of-range settings:
 * F110_ERR_INVALID.  Arming clears the counters and the fallback poses. */
int f110_reset_sampler_set(f110_sim *h, const f110_reset_sampler *spec, const uint64_t *h_streams);
/* explicit draws for the envs of the mask ([num_envs], NULL = all); _device is asynchronous on the handle's stream */
int f110_reset_sample(f110_sim *h, const uint8_t *h_env_mask);
int f110_reset_sample_device(f110_sim *h, const uint8_t *d_env_mask);
/* out2 (or NULL) = {draws, fallbacks} since the last clear; h_attempt [num_envs] (or NULL) = the winning attempt of each env's last
 * draw, -1 = a fallback or no draw yet; clear != 0 zeroes the counters */
int f110_reset_sampler_stats(f110_sim *h, uint64_t *out2, int32_t *h_attempt, int32_t clear);
/* h_poses [N][3] = each env's poses of its last reset of any kind (what an explicit fallback resets to) */
int f110_reset_sampler_poses(f110_sim *h, double *h_poses);
/* device pointers of the episode logic's start poses [N][3] and start_rot [num_envs][4] (f110_episode_init) */
int f110_episode_start_views(f110_sim *h, double **d_start_poses, double **d_start_rot);

/* ---- randomised vehicle parameters (no reference counterpart: the reference's update_params is a host call between episodes).
 * A parameter sampler draws an env's rows of the per-agent parameter block [N][18] on the device, wherever a reset sampler
 * would draw its start poses.  Each of the 18 slots (f110_config.params order: mu, C_Sf, C_Sr, lf, lr, h, m, I, s_min, s_max,
 * sv_min, sv_max, v_switch, a_max, v_min, v_max, width, length) has one f110_param_dist:
 *   kind   FIXED   the slot is not drawn: it consumes nothing and holds the nominal value
 *          UNIFORM v = a + u * (b - a), u the stream's next Generator.random(): bitwise Generator.uniform(a, b)
 *          NORMAL  v = a + b * z, z the stream's next Generator.standard_normal() (NumPy's ziggurat), then v < lo ? lo :
 *                  (v > hi ? hi : v): bitwise np.clip(Generator.normal(a, b), lo, hi)
 *   scope  AGENT   every agent of the env gets its own draw, in agent order
 *          ENV     one draw, shared by every agent of the env (surface friction belongs to the track, not to the car)
 *   relative != 0  the row gets nominal * v (one float64 multiply), nominal = that slot's value in the agent slot's parameter
 *                  set (f110_set_params) at arming; else v itself.
 * Order within an env: slots in index order; within a slot the env's single draw, or agents 0 .. A - 1.  float64 without
 * contraction.  Env e owns np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(e,))) with e the GLOBAL env index
 * (f110_pcg64_seed_spawn): the reset sampler's rule, so whoever arms both gives them different seeds.
 * Refused at arming (F110_ERR_INVALID; nothing written or allocated, a sampler already armed stays as it is): an unknown kind or
 * scope; a kind other than FIXED on width or length (the collision boxes and the iTTC side tables are the constructor's);
 * UNIFORM with a > b or a non-finite a or b; NORMAL with a non-finite a or b, b < 0, non-finite lo or hi, or lo > hi; an entry
 * whose reachable interval ([a, b] UNIFORM, [lo, hi] NORMAL, times the nominal of every agent slot when relative) leaves the
 * model's domain: mu, C_Sf, C_Sr, lf, lr, h, m, I, a_max, v_switch > 0; s_min < s_max, sv_min < sv_max, v_min < v_max over the
 * whole intervals (a slot that is not drawn counts with its nominal values).  So validity is settled once, on the host, by
 * intervals, and the draw has no rejection loop.
 * Refused for state (F110_ERR_STATE): arming while f110_set_params_batch rows are active, f110_set_params_batch and
 * f110_set_params while a sampler is armed: the rows have one owner.
 * Arming fills the block with the nominal rows and switches every consumer to it; no draw happens at arming.  In-step draws:
 * behind every call that re-seats envs, as for the reset sampler (per env block, +1 launch); either sampler may be armed without
 * the other, and with both the results do not depend on their order.  Disarming waits for the stream, returns to the per-slot
 * sets and frees what arming allocated.  The stream position is state (F110_STATE_COL_PARAM_RNG), the rows travel as
 * F110_STATE_COL_PARAMS; the entries are configuration. */
enum { F110_PARAM_FIXED = 0, F110_PARAM_UNIFORM = 1, F110_PARAM_NORMAL = 2 };
enum { F110_PARAM_SCOPE_AGENT = 0, F110_PARAM_SCOPE_ENV = 1 };
typedef struct f110_param_dist {
    int32_t kind, scope;
    double a, b;           /* UNIFORM: the interval; NORMAL: loc, scale */
    double lo, hi;         /* NORMAL: the clip */
    int32_t relative, pad;
} f110_param_dist;
/* arm (entries18 != NULL; h_streams [num_envs][4] from f110_pcg64_seed_spawn) or disarm (entries18 = NULL).  Arming clears the counter. */
int f110_param_sampler_set(f110_sim *h, const f110_param_dist *entries18, const uint64_t *h_streams);
/* explicit draws for the envs of the mask ([num_envs], NULL = all), with no reset; _device is asynchronous on the handle's stream */
int f110_param_sample(f110_sim *h, const uint8_t *h_env_mask);
int f110_param_sample_device(f110_sim *h, const uint8_t *d_env_mask);
/* *draws (or NULL) = envs drawn since the last clear; clear != 0 zeroes the counter */
int f110_param_sampler_stats(f110_sim *h, uint64_t *draws, int32_t clear);
/* the live per-agent rows [N][18], the sampler's or f110_set_params_batch's: a host copy (synchronous), the device pointer.
 * F110_ERR_STATE while neither is active. */
int f110_params_get(f110_sim *h, double *h_out);
int f110_params_view(f110_sim *h, const double **d_rows);
/* unit form: m envs of A agents with the nominal rows h_nominal [A][18] and the streams h_streams [m][4], drawn `rounds` times one
 * after the other; h_out [rounds][m * A][18] (a FIXED slot: the nominal), h_streams_out [m][4] (or NULL) the streams afterwards.
 * Refuses what arming refuses, and A outside 1..256, m < 1, rounds < 1. */
int f110_param_sample_batch(f110_sim *h, const f110_param_dist *entries18, const double *h_nominal, int32_t A, const uint64_t *h_streams,
                            int32_t m, int32_t rounds, double *h_out, uint64_t *h_streams_out);

/* ---- rendering (rendering.py draws with pyglet: map points, one quad per car, a label; this is its rgb_array form) ----
 * A render makes F frames of H x W pixels, one uint8 class per pixel (the highest that applies wins):
 *   0 OUTSIDE  the pixel centre is outside env e's map (xy_2_rc's bounds test)   1 FREE  inside, dt != 0
 *   2 WALL     inside, dt == 0 (the lidar's obstacles)                             3 TRACK a point of the slot's track (f110_track_set)
 *   4 SCAN     a lidar hit (range < max_range) of the camera agent                  5 CAR   inside another agent's box of env e
 *   6 SELF     inside the camera agent's box
 * Each frame has a camera agent n (global index) of env e = n / A.  Poses are Simulator.agent_poses (the observation's), scans the
 * last step's.  Pixel (i, j), row 0 at the top: u = ((j + 0.5) - W/2) m_per_px, v = (H/2 - (i + 0.5)) m_per_px,
 * x = cx + (u cos(phi) - v sin(phi)), y = cy + (u sin(phi) + v cos(phi)), all float64.  WORLD: (cx, cy, phi) = (center_x, center_y,
 * angle); FOLLOW: the camera agent's pose plus fwd_offset along its heading, phi = 0; EGO: the same centre, phi = theta - pi/2.
 * Boxes are get_vertices' (collision_models.py:218-260) with the agent's own length / width, or car_length / car_width when both
 * are > 0.  An agent with a non-finite pose is not drawn; a FOLLOW / EGO frame on one is all OUTSIDE.  A layer that is off adds
 * none of its classes (MAP off: FREE wherever nothing else is drawn).  A render changes no simulator state. */
enum { F110_VIEW_WORLD = 0, F110_VIEW_FOLLOW = 1, F110_VIEW_EGO = 2 };
enum { F110_LAYER_MAP = 1, F110_LAYER_TRACK = 2, F110_LAYER_SCAN = 4, F110_LAYER_CARS = 8, F110_LAYER_ALL = 15 };
enum { F110_CLASS_OUTSIDE = 0, F110_CLASS_FREE = 1, F110_CLASS_WALL = 2, F110_CLASS_TRACK = 3, F110_CLASS_SCAN = 4, F110_CLASS_CAR = 5,
       F110_CLASS_SELF = 6, F110_NCLASSES = 7 };
typedef struct f110_render_spec {
    int32_t width, height, view /* F110_VIEW_WORLD / _FOLLOW / _EGO */, layers /* F110_LAYER_* bits */;
    double m_per_px, center_x, center_y, angle /* WORLD only */, fwd_offset, car_length, car_width /* <= 0: params */;
} f110_render_spec;
/* F frames into d_classes [F][H][W] (required) and, if d_rgb != NULL, d_rgb [F][H][W][3] = palette[class]
 * (h_palette [7][3] or NULL = default).  h_agents [F] camera agents, or NULL with n_frames == N (frame f = agent f).
 * Asynchronous on the handle's stream, behind both env blocks of the last step; the next step waits for it.
 * Refused (F110_ERR_INVALID, nothing launched or written): W or H outside 1..4096, m_per_px not finite and > 0, an unknown view
 * or layer bit, an agent outside [0, N), n_frames < 1 (or != N without h_agents), F*H*W > 2^31. */
int f110_render_device(f110_sim *h, const f110_render_spec *spec, const int32_t *h_agents, int32_t n_frames,
                       uint8_t *d_classes, uint8_t *d_rgb, const uint8_t *h_palette);

/* ---- compact observations (no reference counterpart: what RL setups built on the reference compute on the host from
 * obs['scans'] before a policy sees it: a few pooled ranges, a few state columns, the last few frames stacked) ----
 * An encode turns the observation of the last step into out [N][F][D] float32.  It runs only when called, changes no simulator
 * state, and no step launches anything for it.  Every operation is one correctly rounded IEEE operation (compare, float64 add,
 * float64 divide, float64 -> float32 round-to-nearest-even); there is no trigonometry and no libm call, so results are defined
 * bit for bit.
 * Lidar part: beams [beam_lo, beam_hi) of the handle's B (0, 0 = all), W = beam_hi - beam_lo, cut into K = sectors sectors,
 *   0 <= K <= W (K = 0: no lidar part).  Sector k covers beams b0 = beam_lo + floor(k W / K) .. b1 = beam_lo + floor((k + 1) W / K)
 *   exclusive (integer arithmetic; never empty since K <= W).  v = pool of the sector:
 *     MIN     the smallest range; NaN if any beam is NaN (np.min)
 *     MEAN    ranges added in ascending beam order in float64, uncontracted, starting from the first beam, divided by b1 - b0
 *     CENTER  beam (b0 + b1 - 1) >> 1
 *   value = (float)(minimum(v, range_clip) / range_scale): minimum propagates NaN (np.minimum), the division is float64.
 * Feature part: the set bits of `features`, in ascending bit order behind the lidar values, each (float)(x / feat_scale[bit]):
 *     VX = state[3], STEER = state[2], YAW_RATE = state[5], SLIP = state[6], COLLISION = the collisions column,
 *     LATERAL, HEADING_ERROR, DS = the track columns of the step (f110_track_enable; F110_ERR_STATE while tracking is off).
 *   feat_scale entries of bits that are not set are ignored.  D = K + popcount(features).
 * Frames: F = frames, 1..16.  out[n][F-1] is the newest frame, out[n][0] the oldest.  A call moves agent n's frames 1..F-1 to
 *   0..F-2 and writes the new frame last.  The stack is the CALLER's buffer: the handle keeps no copy of it (and the state blobs
 *   do not contain it); pass the same buffer to every call.
 *   Episode starts: an agent whose step_count is 1 holds the first observation of an episode (after f110_reset + one step, and
 *   on the first step after an in-step re-seat): all F of its frames are set to the new frame.  An agent whose step_count is 0
 *   was re-seated inside the step just taken: its scans are still the finished episode's terminal ones, and it is encoded like
 *   any other agent (shift; lidar from those terminal scans, the feature columns as they stand after the re-seat).  Callers who
 *   bootstrap from terminal observations use the separate re-seat (f110_reset_collided_device) and encode in front of it.
 *   F110_OBS_FILL in flags treats every agent as an episode start: for the first call on a fresh buffer, and after a state load
 *   into a buffer of unknown content.
 * Refused (F110_ERR_INVALID, nothing launched or written): beam_lo < 0, beam_hi > B, beam_lo >= beam_hi (other than 0, 0),
 *   K < 0 or K > W, an unknown pool, feature bit or flag, F outside 1..16, range_clip or range_scale not finite and > 0 (checked
 *   when K > 0), a zero or non-finite feat_scale of a set bit, D = 0, F * D > F110_OBS_MAX_STACK, a null output or one that is not
 *   16-byte aligned. */
enum { F110_OBS_POOL_MIN = 0, F110_OBS_POOL_MEAN = 1, F110_OBS_POOL_CENTER = 2 };
enum { F110_OBS_VX = 1, F110_OBS_STEER = 2, F110_OBS_YAW_RATE = 4, F110_OBS_SLIP = 8, F110_OBS_COLLISION = 16, F110_OBS_LATERAL = 32,
       F110_OBS_HEADING_ERROR = 64, F110_OBS_DS = 128, F110_OBS_NFEATURES = 8,
       F110_OBS_TRACK_FEATURES = F110_OBS_LATERAL | F110_OBS_HEADING_ERROR | F110_OBS_DS, F110_OBS_ALL_FEATURES = 255 };
enum { F110_OBS_FILL = 1 };
enum { F110_OBS_MAX_FRAMES = 16, F110_OBS_MAX_STACK = 8192 /* floats per agent: a wave keeps its agent's stack in LDS */ };
typedef struct f110_obs_spec {
    int32_t beam_lo, beam_hi;   /* 0, 0 = all beams */
    int32_t sectors;            /* K */
    int32_t pool;               /* F110_OBS_POOL_* */
    int32_t features;           /* F110_OBS_* bits */
    int32_t frames;             /* F */
    int32_t flags;              /* F110_OBS_FILL */
    int32_t pad;
    double range_clip, range_scale;
    double feat_scale[F110_OBS_NFEATURES];   /* indexed by bit number */
} f110_obs_spec;
/* d_out [N][F][D] float32 in device memory.  Asynchronous on the handle's stream; right behind a two-block step it runs per env
 * block on the block's own stream (as f110_scan_policy_device does), so a device-resident loop keeps its blocks and the results
 * are those of one block.  h_pinned (or NULL): page-locked memory of f110_host_alloc (anything else: F110_ERR_INVALID) of the
 * same size that receives a copy of the whole stack, asynchronously behind the encode; f110_sync completes it. */
int f110_obs_encode_device(f110_sim *h, const f110_obs_spec *spec, float *d_out, float *h_pinned);
/* unit form on host arrays (with or without a map; spec->beam_* refer to the handle's B): h_scans [m][B], h_cols [m][8] = the
 * eight feature sources in bit order (all eight may be asked for), h_step_count [m], h_inout [m][F][D] updated in place. */
int f110_obs_encode_batch(f110_sim *h, const f110_obs_spec *spec, const double *h_scans, const double *h_cols, const int32_t *h_step_count,
                          int32_t m, float *h_inout);

/* ---- scripted cars: a follow-the-gap controller per agent (no reference counterpart: the standard reactive F1TENTH planner,
 * for the cars of an env that no policy drives) ----
 * A controller turns an agent's scan row of the last step into an action (steer, speed), the layout f110_step_device takes.  It
 * runs only when called (f110_follow_gap_device, or f110_step_host with F110_STEP_SCRIPTED), keeps no state between calls and
 * changes no simulator state; the state blobs do not contain it.  Every operation is one correctly rounded IEEE operation
 * (compare, float64 add, multiply, divide) or ceil; there is no libm call and nothing is contracted, so results are defined bit
 * for bit.
 * With r the agent's row, beams [lo, hi) = [beam_lo, beam_hi) (0, 0 = all B), W = hi - lo, S = smooth, inc = fov / (B - 1) and
 * angle(b) = -fov / 2. + inc * (double)b:
 *   1 clip     v[i] = r[lo + i] < range_clip ? r[lo + i] : range_clip; a NaN beam gives v[i] = 0
 *   2 smooth   p[i] = (v[a] + v[a + 1] + ... + v[b - 1]) / (double)(b - a), a = max(0, i - S / 2), b = min(W, i + S / 2 + 1); the
 *              adds run in ascending order starting from 0.0 + v[a], every window summed on its own (no running sum)
 *   3 closest  c = the first index of the minimum of p
 *   4 bubble   den = p[c] * inc; kb = den > 0 ? bubble_radius / den : +inf; half-width = W if !(kb < W), else (int)ceil(kb);
 *              q = p with q[i] = 0 for |i - c| <= half-width
 *   5 gap      beam i is free when q[i] > gap_threshold; [g0, g1) = the longest run of free beams, the lowest g0 on equal
 *              length; with no free beam the action is (0.0, v_blocked)
 *   6 target   CENTER: t = (g0 + g1 - 1) >> 1; FURTHEST: t = the first index of the maximum of q within the gap
 *   7 action   steer = clamp(steer_gain * angle(lo + t), +-steer_max); f = p[t] / d_ref;
 *              speed = v_lo + (v_hi - v_lo) * (f < 1 ? f : 1); if fabs(steer) > steer_slow, speed = min(speed, v_turn)
 * An agent whose step_count is 0 was re-seated inside the step just taken and its scans are still the finished episode's: it
 * gets (0, 0), the zero-action step of the reference's reset().
 * Refused (F110_ERR_INVALID, nothing launched or written): beam_lo < 0, beam_hi > B, beam_lo >= beam_hi (other than 0, 0),
 *   W > F110_GAP_MAX_WINDOW, B < 2, smooth even, outside 1..63 or above W, an unknown target, a non-finite setting, range_clip or
 *   d_ref not > 0, bubble_radius, gap_threshold or steer_slow < 0, steer_max < 0, v_lo > v_hi. */
enum { F110_GAP_TARGET_CENTER = 0, F110_GAP_TARGET_FURTHEST = 1 };
enum { F110_GAP_MAX_SPECS = 8, F110_GAP_MAX_SMOOTH = 63, F110_GAP_MAX_WINDOW = 4096 /* a wave keeps one free bit per beam */ };
typedef struct f110_gap_follower {
    int32_t beam_lo, beam_hi;   /* 0, 0 = all beams (the usual choice at 1080 beams: 180, 900) */
    int32_t smooth;             /* S, odd (5) */
    int32_t target;             /* F110_GAP_TARGET_* */
    double range_clip;          /* m (10.0) */
    double bubble_radius;       /* m (0.6) */
    double gap_threshold;       /* m (1.5) */
    double steer_gain, steer_max;      /* (1.0, 0.4189) */
    double v_lo, v_hi, d_ref;          /* (1.5, 4.0, 8.0) */
    double steer_slow, v_turn;         /* (0.2, 2.5) */
    double v_blocked;                  /* (0.5) */
} f110_gap_follower;
/* arms the controllers: specs [n_specs], 1 <= n_specs <= F110_GAP_MAX_SPECS, and h_assign [N] int32: -1 = external (the agent's
 * action comes from the caller), else the index of the agent's spec (anything else: F110_ERR_INVALID, nothing changed).
 * NULL, 0, NULL disarms them.  Arming launches nothing and no step looks at it without F110_STEP_SCRIPTED.  An agent that the
 * armed planner (f110_mppi_set) or a line follower (f110_line_followers_set) drives cannot have a controller too:
 * F110_ERR_INVALID, nothing changed. */
int f110_controllers_set(f110_sim *h, const f110_gap_follower *specs, int32_t n_specs, const int32_t *h_assign);
/* writes the armed agents' rows of d_actions [N][2] (device memory, 16-byte aligned) from the scans of the last step; rows of
 * external agents are never written (their waves leave before they load anything else).  Asynchronous on the handle's stream;
 * right behind a two-block step it runs per env block on the block's own stream (as f110_scan_policy_device does).
 * F110_ERR_STATE with nothing armed. */
int f110_follow_gap_device(f110_sim *h, double *d_actions);
/* unit form on host arrays (with or without a map; spec->beam_* refer to the handle's B and fov): h_scans [m][B], h_step_count
 * [m] or NULL (no row is fresh), h_actions [m][2], h_info [m][5] int32 or NULL: c, half-width, g0, g1, t; g0, g1, t are -1 for a
 * blocked row, all five for a row whose step_count is 0. */
int f110_follow_gap_batch(f110_sim *h, const f110_gap_follower *spec, const double *h_scans, const int32_t *h_step_count, int32_t m,
                          double *h_actions, int32_t *h_info);

/* ---- track preview: the raceline ahead of each agent, in its own frame (no reference counterpart: what trajectory-aided and
 * pure-pursuit-style policies interpolate from the waypoints on the host) ----
 * Per-point attributes.  A track may carry up to F110_TRACK_MAX_ATTRS float64 columns per point (curvature, a speed profile,
 * cos / sin of a heading ...): h_attr [M][C], M the slot's point count as f110_track_set stored it (a closed track's repeated
 * last point dropped).  Refused (F110_ERR_INVALID, nothing changed): another M, C outside 1..4, a non-finite value, a slot
 * without a track.  NULL, 0, 0 clears them, and so does f110_track_set on the slot.  They are configuration like the track and
 * not part of the state blobs.  Attributes are interpolated linearly, value by value: pass kappa, vx or cos / sin columns, not an
 * angle such as psi, whose wrap a linear blend does not know about. */
enum { F110_TRACK_MAX_ATTRS = 4 };
int f110_track_set_attrs(f110_sim *h, int32_t slot, const double *h_attr /* [M][C] */, int32_t M, int32_t C);
/* The preview.  It runs only when called, keeps no state in the handle and changes no simulator state.  Everything is float64
 * without contraction, every operation one correctly rounded IEEE operation except the one cos / sin of the EGO frame.
 * Agent n's track (the one on its env's map slot) has the segments (ax, ay, dx, dy, len, cum)[k] and the total length L; s_n is
 * its `s` column and (px, py, theta) the pose that column was computed from: the observation's pose of the step just taken, the
 * one no in-step re-seat overwrites (agent_poses; it keeps the heading a car arrived with where a wall hit zeroed the state's yaw
 * behind it, so poses_theta of such a car reads 0).  The preview belongs to that observation, as the other track columns do.  Station j of P:
 *   d_j = offset + (double)j * spacing;  s_j = s_n + d_j;  on a closed track: if (s_j >= L) s_j = s_j - L, once
 *   k   = the last segment with cum[k] <= s_j, 0 when there is none (so a NaN s_j gives 0): the reset sampler's rule
 *   t   = clip((s_j - cum[k]) / len[k], 0, 1), the clip passing NaN
 *   X = ax[k] + t * dx[k], Y = ay[k] + t * dy[k];  ux = dx[k] / len[k], uy = dy[k] / len[k]
 *   attr_c = a[c][k] + t * (a[c][k1] - a[c][k]), k1 = k + 1, on a closed track 0 behind the last segment (an open track has the
 *   point k + 1)
 * On an open track a station beyond the end clips to the last point (t = 1 on the last segment).
 * Frames.  WORLD: the channels are X, Y, ux, uy.  EGO: c = cos theta, sn = sin theta, rx = X - px, ry = Y - py and the channels
 * are c * rx + sn * ry, c * ry - sn * rx, c * ux + sn * uy, c * uy - sn * ux.  The attributes are the same in both.
 * Output.  out[n][j][.] holds the channels of the set bits in ascending bit order, each (float)(value / scale[bit]): a float64
 * divide, then the conversion, rounding to nearest even.
 * Refused with F110_ERR_INVALID, nothing launched or written: points outside 1..32, channels 0 or with an unknown bit, an unknown
 *   frame, flags != 0, offset not finite or < 0, spacing not finite or <= 0 (also when points == 1), a zero or non-finite scale of
 *   a set bit, a null or not 16-byte aligned d_out, an h_pinned that is not [N][P][D] floats of f110_host_alloc memory.
 * Refused with F110_ERR_STATE: tracking is off (device form), a slot in use has no track, a requested attribute channel is not
 *   present on a slot in use, a closed track in use has L <= offset + (P - 1) * spacing (one subtraction must be enough).
 * Not offered: a spacing that depends on the speed, stations behind the car, angle-aware interpolation of attributes. */
enum { F110_PREVIEW_X = 1, F110_PREVIEW_Y = 2, F110_PREVIEW_TAN_X = 4, F110_PREVIEW_TAN_Y = 8,
       F110_PREVIEW_ATTR0 = 16, F110_PREVIEW_ATTR1 = 32, F110_PREVIEW_ATTR2 = 64, F110_PREVIEW_ATTR3 = 128, F110_PREVIEW_NCHANNELS = 8 };
enum { F110_PREVIEW_FRAME_EGO = 0, F110_PREVIEW_FRAME_WORLD = 1 };
enum { F110_PREVIEW_MAX_POINTS = 32 };
typedef struct f110_track_preview {
    int32_t points;     /* P, 1..32 stations */
    int32_t channels;   /* F110_PREVIEW_* bits; D = popcount */
    int32_t frame;      /* F110_PREVIEW_FRAME_* */
    int32_t flags;      /* 0 */
    double offset;      /* metres ahead of the agent's projection to station 0, >= 0 */
    double spacing;     /* metres between stations, > 0 (ignored when P == 1, but still validated) */
    double scale[F110_PREVIEW_NCHANNELS];   /* by bit number; entries of clear bits are ignored */
} f110_track_preview;
/* device form: d_out [N][P][D] float32 in device memory.  Asynchronous on the handle's stream; right behind a two-block step it
 * runs per env block on the block's own stream (as f110_obs_encode_device does).  h_pinned (or NULL): f110_host_alloc memory of
 * the same shape that receives a copy behind the kernel, complete after f110_sync. */
int f110_track_preview_device(f110_sim *h, const f110_track_preview *spec, float *d_out /* [N][P][D] */, float *h_pinned);
/* unit form on host arrays, on the track of `slot` (tracking need not be on): h_in [m][4] = x, y, theta, s per row.  It does not
 * project: s comes from f110_track_project_batch.  h_out [m][P][D]; h_raw [m][P][8] or NULL: all eight channel values before
 * scaling, an absent attribute 0.0; h_seg [m][P] or NULL: k per station. */
int f110_track_preview_batch(f110_sim *h, const f110_track_preview *spec, int32_t slot, const double *h_in /* [m][4] x, y, theta, s */,
                             int32_t m, float *h_out /* [m][P][D] */, double *h_raw /* [m][P][8] or NULL */, int32_t *h_seg /* [m][P] or NULL */);

/* ---- neighbours: each agent's K nearest opponents of its own env, in its own frame (no reference counterpart: what overtaking,
 * blocking and self-play setups compute with an all-pairs search on the host) ----
 * It runs only when called, keeps no state in the handle and changes no simulator state.  Everything is float64 without
 * contraction, every operation one correctly rounded IEEE operation except one cos and one sin per agent.
 * Agent n = e * A + a looks at the other agents b != a of its env e.  Per agent: (x, y, theta) is the observation's pose of the step
 * just taken (agent_poses, the one `s` was computed from and no in-step re-seat overwrites), v is state[3] as it stands (the
 * encoder's VX rule: 0 for an env re-seated inside the step), s the track column (read only when GAP_S is asked for), and
 * c_a = cos theta_a, sn_a = sin theta_a, computed once per agent.  For the pair (a, b):
 *   rx = x_b - x_a;  ry = y_b - y_a;  d2 = rx * rx + ry * ry
 * Candidate b is eligible iff b != a and d2 <= R2, R2 = max_range * max_range computed once (max_range > 0, +inf allowed); a NaN
 * d2 is never eligible.  The eligible candidates are ordered by ascending d2, equal d2 by ascending b; the first K fill slots
 * 0 .. K - 1.  Channels, by bit number:
 *   0 DX      c_a * rx + sn_a * ry                 5 V_X    v_b * cd - v_a
 *   1 DY      c_a * ry - sn_a * rx                 6 V_Y    v_b * sd
 *   2 DIST    sqrt(d2)                             7 GAP_S  g = s_b - s_a; on a closed track of length L:
 *   3 COS_DTH cd = c_b * c_a + sn_b * sn_a                  if (g > 0.5 * L) g = g - L; else if (g <= -0.5 * L) g = g + L
 *   4 SIN_DTH sd = sn_b * c_a - c_b * sn_a         8 VALID  1.0        9 INDEX  (double)b
 * Output.  out[n][k][.] holds the channels of the set bits in ascending bit order, each (float)(value / scale[bit]): a float64
 * divide, then the conversion, rounding to nearest even.  A slot without a neighbour holds (float)pad in every requested channel,
 * unscaled, except VALID, which is 0.0f there.  num_agents == 1 is legal: every slot is then empty.
 * Refused with F110_ERR_INVALID, nothing launched or written: k outside 1..8, channels 0 or with an unknown bit, flags != 0,
 *   max_range NaN or <= 0, a pad that is not finite, a zero or non-finite scale of a set bit, a null or not 16-byte aligned d_out,
 *   an h_pinned that is not [N][K][D] floats of f110_host_alloc memory.
 * Refused with F110_ERR_STATE: GAP_S while tracking is off, GAP_S while a slot in use has no track, num_agents > 256.
 * Not offered: a field-of-view filter, ordering by track gap, race position, feeding the result into the encoder's stack, a
 * slip-aware velocity. */
enum { F110_NBR_DX = 1, F110_NBR_DY = 2, F110_NBR_DIST = 4, F110_NBR_COS_DTH = 8, F110_NBR_SIN_DTH = 16, F110_NBR_V_X = 32,
       F110_NBR_V_Y = 64, F110_NBR_GAP_S = 128, F110_NBR_VALID = 256, F110_NBR_INDEX = 512, F110_NBR_NCHANNELS = 10 };
enum { F110_NBR_MAX_K = 8, F110_NBR_MAX_AGENTS = 256 };
typedef struct f110_neighbors {
    int32_t k;          /* K, 1..8 slots per agent */
    int32_t channels;   /* F110_NBR_* bits; D = popcount */
    int32_t flags;      /* 0 */
    int32_t pad_;       /* alignment; ignored */
    double max_range;   /* metres, > 0, +inf allowed */
    double pad;         /* what an empty slot holds, finite */
    double scale[F110_NBR_NCHANNELS];   /* by bit number; entries of clear bits are ignored */
} f110_neighbors;
/* device form: d_out [N][K][D] float32 in device memory.  Asynchronous on the handle's stream; right behind a two-block step it
 * runs per env block on the block's own stream (as f110_track_preview_device does).  h_pinned (or NULL): f110_host_alloc memory
 * of the same shape that receives a copy behind the kernel, complete after f110_sync.  On a closed track GAP_S wraps with the
 * length of the track on the env's map slot; on an open one it does not wrap. */
int f110_neighbors_device(f110_sim *h, const f110_neighbors *spec, float *d_out /* [N][K][D] */, float *h_pinned);
/* unit form on host arrays: h_in [m][5] = x, y, theta, v, s per row, env-major; m a multiple of A, A in 1..256 whatever the
 * handle's num_agents is.  track_L > 0 wraps GAP_S as a closed track of that length, 0 does not wrap (anything else is refused).
 * h_out [m][K][D]; h_raw [m][K][10] or NULL: all ten channel values before scaling, in an empty slot pad and VALID 0.0; h_idx
 * [m][K] or NULL: b per slot, -1 for an empty one. */
int f110_neighbors_batch(f110_sim *h, const f110_neighbors *spec, int32_t A, double track_L, const double *h_in /* [m][5] x, y, theta, v, s */,
                         int32_t m, float *h_out /* [m][K][D] */, double *h_raw /* [m][K][10] or NULL */, int32_t *h_idx /* [m][K] or NULL */);

/* ---- scripted cars: a line follower per agent (no reference counterpart: pure pursuit on the track of the agent's map slot,
 * the speed from a track attribute, slower behind a car ahead; the opponent that drives the slot's raceline) ----
 * A third kind of scripted car beside the follow-the-gap controller and the planner.  It is stateless, runs only when called
 * (f110_follow_line_device, or f110_step_host with F110_STEP_SCRIPTED) and changes no simulator state; the state blobs do not
 * contain it.  Everything is float64 without contraction, every operation one correctly rounded IEEE operation except cos_sin and
 * atan in step 3, and only lx, ly and steer sit behind those: no branch and no part of the speed does.
 * Agent n = e * A + a with spec S; its track (the one on its env's map slot) has the segments (ax, ay, dx, dy, len, cum)[k], the
 * length L and the attributes a[c][.].  (px, py, th) is the observation's pose of the step just taken (agent_poses), s and lat
 * the track columns s and lateral of that step, v is state[3] as it stands (the neighbours' rule), cnt its step_count.
 *   0 fresh     cnt == 0 (re-seated inside the step just taken): the action is (0.0, 0.0)
 *   1 lookahead ld = look_base + look_gain * fabs(v);  if (!(ld >= look_min)) ld = look_min; else if (ld > look_max) ld = look_max
 *               (a NaN v gives look_min)
 *   2 station   s_t = s + ld; on a closed track: if (s_t >= L) s_t = s_t - L, once.  k, t, (X, Y) and (ux, uy) by the track
 *               preview's station rule at s_t (above; on an open track a station beyond the end clips to the last point).
 *               Tx = X - lane_offset * uy;  Ty = Y + lane_offset * ux
 *   3 steer     c = cos th, sn = sin th;  rx = Tx - px;  ry = Ty - py;  lx = c * rx + sn * ry;  ly = c * ry - sn * rx;
 *               d2 = lx * lx + ly * ly;  steer = d2 > 0 ? atan(((2.0 * wheelbase) * ly) / d2) : 0.0;
 *               if (steer > steer_max) steer = steer_max; else if (steer < -steer_max) steer = -steer_max
 *   4 speed     s_v = s + speed_look, with the same single wrap;  vref = attribute speed_attr at s_v by the preview's k, t and
 *               attribute rule, or v_const when speed_attr == -1;  speed = vgain * vref;
 *               if (fabs(lat - lane_offset) > lat_slow && v_recover < speed) speed = v_recover
 *   5 car ahead only when follow_range > 0 and A > 1; lim = -1; for b = 0 .. A - 1, b != a, ascending:
 *               g = s_b - s, wrapped by the neighbours' GAP_S rule on a closed track;
 *               b is eligible iff g > 0 && g <= follow_range && fabs(lat_b - lat) <= lane_width;
 *               cap = v_b + follow_gain * (g - follow_gap);  if (cap < speed) { speed = cap; lim = b; }   (a NaN cap never wins)
 *   6 clamp     if (speed < v_min) speed = v_min;  if (speed > v_max) speed = v_max.  The action is (steer, speed).
 * Refused with F110_ERR_INVALID, nothing launched or written, device allocations as they were: a non-finite setting;
 *   look_min <= 0, look_min > look_max, look_base < 0, look_gain < 0, speed_look < 0; wheelbase <= 0, steer_max < 0, v_min < 0,
 *   v_min > v_max; follow_range < 0, lane_width < 0, lat_slow < 0, speed_attr outside -1..3; an assignment outside
 *   -1..n_specs - 1, more than F110_LINE_MAX_SPECS specs; an agent that also has a follow-the-gap controller or the armed planner
 *   (f110_controllers_set and f110_mppi_set in turn refuse an agent that a line follower drives); a null or not 16-byte
 *   aligned action or info buffer.
 * Refused with F110_ERR_STATE: tracking off (device form); an armed agent's slot without a track or without attribute column
 *   speed_attr; a closed track in use with L <= max(look_max, speed_look) (one subtraction must be enough) or L <= 2 *
 *   follow_range; num_agents > 256 with follow_range > 0 (at arming); nothing armed.
 * Not offered: overtaking manoeuvres (the planner with the opponent term does those), a lane offset that varies along the line,
 * a wheelbase read from the agent's parameter row. */
enum { F110_LINE_MAX_SPECS = 8, F110_LINE_MAX_AGENTS = 256, F110_LINE_NRAW = 12, F110_LINE_NINFO = 4 };
typedef struct f110_line_follower {
    double look_base, look_gain, look_min, look_max;   /* m, s, m, m (0.8, 0.25, 0.6, 3.9) */
    double lane_offset;                                /* m to the left of the line (0.0) */
    double wheelbase, steer_max;                       /* (0.3302, 0.4189) */
    double v_const, vgain, speed_look;                 /* (2.0, 0.8, 0.6) */
    double lat_slow, v_recover;                        /* (0.5, 1.5) */
    double follow_range, follow_gap, follow_gain;      /* m, m, 1/s (6.0, 1.0, 1.0); follow_range 0: no car-ahead term */
    double lane_width;                                 /* m (0.6) */
    double v_min, v_max;                               /* (0.0, 20.0) */
    int32_t speed_attr;                                /* -1: v_const, else the track's attribute column (1: the raceline's vx) */
    int32_t pad_;                                      /* alignment; ignored */
} f110_line_follower;
/* arms the line followers: specs [n_specs], 1 <= n_specs <= F110_LINE_MAX_SPECS, and h_assign [N] int32: -1 = no line follower,
 * else the index of the agent's spec.  NULL, 0, NULL disarms them and frees their device memory.  Arming launches nothing and no
 * step looks at it without F110_STEP_SCRIPTED. */
int f110_line_followers_set(f110_sim *h, const f110_line_follower *specs, int32_t n_specs, const int32_t *h_assign /* [N] */);
/* writes the armed agents' rows of d_actions [N][2] (device memory, 16-byte aligned) and, when given, of d_info [N][4] float64 =
 * ld, vref, (double)k, (double)lim (-1.0 when no car limits; a fresh row: 0, 0, -1, -1).  Rows of agents without a line follower
 * are never written.  Asynchronous on the handle's stream; right behind a two-block step it runs per env block on the block's
 * own stream (as f110_follow_gap_device does). */
int f110_follow_line_device(f110_sim *h, double *d_actions /* [N][2] */, double *d_info /* [N][4] or NULL */);
/* unit form on host arrays, on the track of `slot` (tracking need not be on; it does not project): h_in [m][7] = x, y, theta, v,
 * s, lateral, step_count per row, env-major; m a multiple of A, A in 1..256 whatever the handle's num_agents is.  h_actions
 * [m][2]; h_raw [m][12] or NULL = ld, s_t, k, X, Y, Tx, Ty, lx, ly, vref, lim, the speed before step 6 (a fresh row: 0.0 but k and
 * lim, which are -1.0). */
int f110_follow_line_batch(f110_sim *h, const f110_line_follower *spec, int32_t slot, int32_t A, const double *h_in /* [m][7] */,
                           int32_t m, double *h_actions /* [m][2] */, double *h_raw /* [m][12] or NULL */);

/* ---- rollout: K candidate action sequences per agent rolled ahead from the agent's live state, against the map (no reference
 * counterpart: what MPPI, motion-primitive and lattice planners and safety shields ask K times per agent per step — "if I apply
 * this action sequence, where does the car end up, and does it leave the track?") ----
 * It runs only when called, keeps no state in the handle, changes no simulator state and no blob format; no step launches it.
 * Everything is float64 without contraction.
 * Candidates.  A candidate is H actions (steer, speed), float64 exactly as the action buffer, each held for `repeat` sim steps.
 * layout SHARED: d_actions is [K][H][2], one library for all agents; PER_AGENT: [N][K][H][2].
 * Start.  Candidate k of agent n starts from the agent's LIVE columns: state[7], both entries of the steering FIFO and its fill
 * count — what the next step would integrate from.
 * One sim step is
 *   1. one RaceCar.update_pose without the scan (the step's own integration: the two-step steering delay, the PID, the single-track
 *      model with its low-speed branch, RK4 or Euler) with the handle's time_step, integrator and lidar_dist and the agent's own
 *      parameter row (per agent slot, or f110_set_params_batch's);
 *   2. one clearance sample d = dt[xy_2_rc(x, y)] on the row-major distance table of the env's map slot at the reference point
 *      state[0..1] (NOT at the lidar); outside the table it is the table's last cell, as the scan sees it.
 * A candidate is alive while d > margin, written so that a NaN d dies; a NaN position dies too (it reads the out-of-table value).
 * The first step whose sample fails kills the candidate: its state stays as that step left it, and no further steps or samples
 * are taken.  This is FREE FLIGHT AGAINST THE MAP: other cars, the iTTC check and the zeroing of the velocity on a collision are
 * not modelled.  Until the simulator raises a collision flag the rollout is the simulator's own motion, bit for bit.
 * Frame.  MAP, or EGO: the agent's pose at the start, with c0 = cos theta0, s0 = sin theta0 taken once per agent.  A pose
 * (x, y, theta) with c = cos theta, s = sin theta reads in the MAP frame (x, y, c, s) and in the EGO frame, with rx = x - x0,
 * ry = y - y0,  (c0 * rx + s0 * ry,  c0 * ry - s0 * rx,  c * c0 + s * s0,  s * c0 - c * s0).
 * Channels, by bit number (raw float64 values per candidate):
 *   0 END_X, 1 END_Y, 2 END_COS, 3 END_SIN   the end pose in the frame
 *   4 END_V         state[3] at the end             5 END_YAW_RATE  state[5] at the end
 *   6 ALIVE         sim steps completed with d > margin, 0 .. H * repeat
 *   7 MIN_CLEAR     the minimum over the samples taken, the killing one included (m = +inf; per sample: if (!(d >= m)) m = d)
 *   8 PROGRESS      s(end) - s(start): both positions are projected by this call with the track projection's first-minimum search
 *                   (f110_track_*), the s column is not read; on a closed track of length L wrapped once:
 *                   if (g > 0.5 * L) g = g - L; else if (g <= -0.5 * L) g = g + L
 *   9 END_LAT       the signed lateral offset of the end position, the track projection's rule (left of the segment positive)
 * PROGRESS and END_LAT need a track (f110_track_set) on every map slot in use; tracking need not be enabled.
 * Output.  d_out[n][k][.] holds the channels of the set bits in ascending bit order, each (float)(value / scale[bit]): a float64
 * divide, then the conversion, rounding to nearest even.  With traj = 1, d_traj[n][k][h][0..3] is the pose (x, y, cos, sin) after
 * action h's last repeat, in the same frame, divided by the scales of END_X, END_Y, END_COS, END_SIN (read whether or not those
 * bits are set); a dead candidate repeats its frozen pose.
 * Refused with F110_ERR_INVALID, nothing launched or written: k outside 1..256, horizon outside 1..64, repeat outside 1..16 (so
 * also k * horizon * repeat == 0), an unknown layout or frame, channels 0 or with an unknown bit, traj other than 0 or 1, a scale
 * of a set bit (with traj: of bits 0..3 too) that is not finite and > 0, a NaN margin, a null d_actions or d_out, traj = 1 with a
 * null d_traj, an h_pinned that is not [N][K][D] floats of f110_host_alloc memory.
 * Refused with F110_ERR_STATE: no map, PROGRESS or END_LAT while a map slot in use has no track.
 * Not offered: float32 action input, footprint-corner clearance, feeding the result into the observation encoder, a
 * keyword on the env layers (a rollout is a function of the caller's candidates, not an observation).  A built-in cost and update
 * on top of it is the MPPI planner below (f110_mppi_*); the other cars' predicted motion is the opponent term below that
 * (f110_opponents, f110_rollout_opp_*). */
enum { F110_ROLL_END_X = 1, F110_ROLL_END_Y = 2, F110_ROLL_END_COS = 4, F110_ROLL_END_SIN = 8, F110_ROLL_END_V = 16,
       F110_ROLL_END_YAW_RATE = 32, F110_ROLL_ALIVE = 64, F110_ROLL_MIN_CLEAR = 128, F110_ROLL_PROGRESS = 256, F110_ROLL_END_LAT = 512,
       F110_ROLL_NCHANNELS = 10 };
enum { F110_ROLL_SHARED = 0, F110_ROLL_PER_AGENT = 1 };
enum { F110_ROLL_FRAME_EGO = 0, F110_ROLL_FRAME_MAP = 1 };
enum { F110_ROLL_MAX_K = 256, F110_ROLL_MAX_H = 64, F110_ROLL_MAX_REPEAT = 16 };
typedef struct f110_rollout {
    int32_t k;          /* K, 1..256 candidates per agent */
    int32_t horizon;    /* H, 1..64 actions per candidate */
    int32_t repeat;     /* 1..16 sim steps each action is held */
    int32_t layout;     /* F110_ROLL_SHARED / F110_ROLL_PER_AGENT */
    int32_t frame;      /* F110_ROLL_FRAME_* */
    int32_t channels;   /* F110_ROLL_* bits; D = popcount */
    int32_t traj;       /* 0, or 1: the trajectory output is written too */
    int32_t pad_;       /* alignment; ignored */
    double margin;      /* metres; not NaN (-inf: nothing dies of its clearance) */
    double scale[F110_ROLL_NCHANNELS];   /* by bit number; entries of clear bits are ignored (see traj) */
} f110_rollout;
/* device form: d_actions float64 in device memory in the spec's layout, d_out [N][K][D] and d_traj [N][K][H][4] (NULL when
 * traj = 0) float32 in device memory.  Asynchronous on the handle's stream; right behind a two-block step it runs per env block on
 * the block's own stream (as f110_neighbors_device does).  h_pinned (or NULL): f110_host_alloc memory of d_out's shape that
 * receives a copy behind the kernels, complete after f110_sync. */
int f110_rollout_device(f110_sim *h, const f110_rollout *spec, const double *d_actions, float *d_out /* [N][K][D] */,
                        float *d_traj /* [N][K][H][4] or NULL */, float *h_pinned);
/* unit form on host arrays, the same kernels on uploaded rows: h_start [m][10] = state[7], the FIFO's newest and older entry, its
 * fill count (0, 1 or 2) per row, all on map slot `slot`; h_params [m][18] a parameter row per row, or NULL: the handle's row of
 * agent slot 0; h_actions in the spec's layout with N = m.  h_out [m][K][D]; h_raw [m][K][10] or NULL: all ten channel values before
 * scaling (PROGRESS and END_LAT 0.0 when the slot has no track); h_traj [m][K][H][4] float32 (with traj = 1) or NULL; h_traj_raw
 * [m][K][H][4] float64, the same poses before scaling (with traj = 1), or NULL. */
int f110_rollout_batch(f110_sim *h, const f110_rollout *spec, int32_t slot, const double *h_start /* [m][10] */,
                       const double *h_params /* [m][18] or NULL */, const double *h_actions, int32_t m, float *h_out /* [m][K][D] */,
                       double *h_raw /* [m][K][10] or NULL */, float *h_traj /* [m][K][H][4] or NULL */, double *h_traj_raw /* or NULL */);

/* ---- MPPI planner: a sampling planner per agent on top of the rollout (no reference counterpart: model predictive path integral
 * control, the sampling planner run on F1TENTH cars, here for the cars of an env that plan instead of react) ----
 * It runs only when called (f110_mppi_device, or f110_step_host with F110_STEP_SCRIPTED), changes no simulator state and no blob
 * format.  A planner is armed on a handle with ONE spec, a strictly ascending list of M agent indices (the armed agents,
 * 1 <= M <= N) and one PCG64 stream per armed agent.  The handle owns per armed agent a nominal sequence U[H][2] of (steer, speed)
 * and the stream position (state.hi, state.lo, inc.hi, inc.lo, the words of f110_pcg64_seed_spawn).  Both are configuration of
 * the planner, not simulator state: the state blobs do not contain them (f110_mppi_get / f110_mppi_put checkpoint them next to a
 * blob).  Everything is float64 without contraction.
 * One call does, for every armed agent n (the rows of other agents are never read or written), with K = k, H = horizon:
 *   1 fresh row   if step_count[n] == 0 (at reset, or re-seated inside the step just taken): U[h] = (0.0, v_init) for every h first
 *   2 candidates  V[0] = U, without a draw.  Candidate k >= 1 has its own generator: the agent's, advanced by k * 2^20 LCG steps
 *                 (numpy.random.PCG64.advance's count).  For h = 0 .. H - 1 it draws e_s, then e_v, each one
 *                 Generator.standard_normal() (NumPy's ziggurat, as the scan noise), and
 *                   V[k][h] = (clamp(U[h][0] + sigma_steer * e_s, steer_min, steer_max),
 *                              clamp(U[h][1] + sigma_speed * e_v, speed_min, speed_max)),  clamp(x, lo, hi) = x < lo ? lo : (x > hi ? hi : x)
 *                 After the call the agent's generator stands 2^28 steps further on, whatever K is.
 *   3 rollout     every candidate is rolled as f110_rollout rolls it (above: the agent's live state, FIFO, fill count and
 *                 parameter row, the handle's time step, integrator and lidar offset, the env's map slot) with the spec's repeat
 *                 and margin; it yields ALIVE and MIN_CLEAR and, when w_progress or w_lat is non-zero, PROGRESS and END_LAT by
 *                 the rollout's projection rule (then every map slot an armed agent uses needs a track, else F110_ERR_STATE;
 *                 with both weights 0 no track is needed, nothing is projected and both values are 0.0)
 *   4 cost        c = w_dead * (double)(H * repeat - ALIVE)
 *                 c = c + w_clear * (MIN_CLEAR < clear_ref ? clear_ref - MIN_CLEAR : 0.0)
 *                 c = c - w_progress * PROGRESS
 *                 c = c + w_lat * fabs(END_LAT);   a NaN c becomes +inf
 *   5 weights     beta = the minimum of c_k, best = its first index.  If beta is not finite: w_0 = 1, every other w_k = 0.
 *                 Otherwise w_k = exp(-(c_k - beta) / lambda).  eta = sum w_k, q = sum w_k * w_k, both over ascending k from 0.0.
 *   6 update      U'[h][c] = (sum_k w_k * V[k][h][c]) / eta, the sum over ascending k from 0.0.  The agent's row of d_actions is
 *                 U'[0].  The stored nominal becomes U' (shift == 0), or U[h] = U'[h + 1] for h < H - 1 and U[H - 1] = U'[H - 1]
 *                 (shift == 1).
 *   7 info        d_info (or NULL) [N][4] float32: the armed rows hold (float)beta, (float)c_0, (float)(eta * eta / q), (float)best.
 * The sums are defined bit for bit given the weights; exp and the rollout's sin / cos are the device's.
 * Refused with F110_ERR_INVALID, nothing changed: k outside 1..256, horizon outside 1..64, repeat outside 1..16, shift other than
 *   0 or 1, a NaN margin, any other setting not finite, a sigma < 0, steer_min > steer_max, speed_min > speed_max, lambda <= 0, a
 *   weight < 0, v_init outside [speed_min, speed_max]; a list that is not strictly ascending or has an index outside 0 .. N - 1; an
 *   armed agent with a follow-the-gap assignment (and f110_controllers_set on an armed agent); M * K >= 2^31.
 * Not offered: several specs per handle, the iTTC check or the footprint in the prediction (the rollout's own limits),
 * a control-effort term, a covariance or a temporal correlation of the noise, float32 candidates, the planner inside the state
 * blobs.  The other cars enter the cost through the opponent term (f110_mppi_set_opponents, below). */
enum { F110_MPPI_MAX_K = 256, F110_MPPI_MAX_H = 64, F110_MPPI_MAX_REPEAT = 16 };
typedef struct f110_mppi {
    int32_t k;          /* K, 1..256 candidates per agent (candidate 0 is the nominal itself) */
    int32_t horizon;    /* H, 1..64 actions per candidate */
    int32_t repeat;     /* 1..16 sim steps each action is held */
    int32_t shift;      /* 0, or 1: the stored nominal moves one action ahead after every call */
    double margin;      /* metres; not NaN: a candidate is alive while the clearance is above it */
    double sigma_steer, sigma_speed;   /* >= 0 */
    double steer_min, steer_max;       /* steer_min <= steer_max */
    double speed_min, speed_max;       /* speed_min <= speed_max */
    double lambda;      /* > 0: the temperature */
    double w_dead, w_clear, w_progress, w_lat;   /* >= 0 */
    double clear_ref;   /* metres: clearance below it costs w_clear per metre */
    double v_init;      /* the speed of a fresh nominal, within [speed_min, speed_max] */
} f110_mppi;
/* arms the planner: h_agents [m] strictly ascending, h_streams [m][4] uint64.  NULL, NULL, 0, NULL disarms it and frees its
 * memory.  Arming sets every nominal to (0, v_init) and launches nothing; no step looks at it without F110_STEP_SCRIPTED. */
int f110_mppi_set(f110_sim *h, const f110_mppi *spec, const int32_t *h_agents, int32_t m, const uint64_t *h_streams /* [m][4] */);
/* one planning call: the armed agents' rows of d_actions [N][2] float64 (device memory, the step's layout) and of d_info [N][4]
 * float32 (or NULL).  Asynchronous on the handle's stream; right behind a two-block step it runs per env block on the block's own
 * stream, the ascending list split at the block's bounds.  F110_ERR_STATE with nothing armed or without a map. */
int f110_mppi_device(f110_sim *h, double *d_actions, float *d_info);
/* the planner's own memory, in the armed list's order: h_nominal [m][H][2], h_streams [m][4]; either may be NULL.  get waits for
 * the handle's work; put refuses (F110_ERR_INVALID, nothing changed) a nominal value that is not finite or outside the spec's
 * bounds.  F110_ERR_STATE with nothing armed. */
int f110_mppi_get(f110_sim *h, double *h_nominal, uint64_t *h_streams);
int f110_mppi_put(f110_sim *h, const double *h_nominal, const uint64_t *h_streams);
/* unit form on host arrays, the same kernels on uploaded rows laid out as f110_rollout_batch lays them: h_start [m][10] on map
 * slot `slot`, h_params [m][18] or NULL, h_fresh [m] int32 (the rows' step_count; NULL: none is fresh), h_nominal [m][H][2] and
 * h_streams [m][4] in and out.  Outputs, each may be NULL: h_actions [m][2], h_info [m][4], h_cand [m][K][H][2] (V), h_cost
 * [m][K], h_weight [m][K].  The planner armed on the handle, if any, is not touched. */
int f110_mppi_batch(f110_sim *h, const f110_mppi *spec, int32_t slot, const double *h_start /* [m][10] */,
                    const double *h_params /* [m][18] or NULL */, const int32_t *h_fresh /* [m] or NULL */, int32_t m,
                    double *h_nominal /* [m][H][2] */, uint64_t *h_streams /* [m][4] */, double *h_actions /* [m][2] */,
                    float *h_info /* [m][4] */, double *h_cand /* [m][K][H][2] */, double *h_cost /* [m][K] */, double *h_weight /* [m][K] */);

/* ---- opponents: the other cars of an agent's env predicted over the horizon, for the rollout and the MPPI planner (no reference
 * counterpart: what lets a sampling planner see the car in front) ----
 * The rollout and the planner above fly free against the map.  With these settings every candidate is also measured against where
 * the other cars of its env will be.  Everything is float64, nothing is contracted, operations run in the order written.
 * Opponents.  For agent n = e * A + a they are the other agents of env e, in ascending slot b != a: A - 1 of them (none with
 *   A = 1; A - 1 <= 31).  Opponent o is read from the LIVE columns at the call: x_o, y_o = state[0..1], v_o = state[3],
 *   theta_o = state[4].  With dx = x_o - x, dy = y_o - y from the agent's own start position, opponent o is ignored for the whole
 *   call if !(dx * dx + dy * dy <= max_range * max_range) (so a NaN ignores it); an ignored opponent's predictions are NaN.
 * Sample times.  tau_h = (double)((h + 1) * repeat) * time_step for h = 0 .. H - 1: the instant of the pose after action h's last
 *   repeat (the pose d_traj holds).
 * Prediction p_o(h), once per call:
 *   CV     (c, s) = cos, sin of theta_o, taken once.  d = v_o * tau_h;  p = (x_o + d * c, y_o + d * s).
 *   TRACK  the opponent keeps its lateral offset and runs along the raceline.  (x_o, y_o) is projected on its env's track by the
 *          rollout's rule (the first-minimum search of PROGRESS) -> (s_o, lat_o).  s = s_o + v_o * tau_h; on a closed track of
 *          length L wrapped once: if (s >= L) s = s - L; else if (s < 0.0) s = s + L.  An open track does not wrap (the segment
 *          parameter's clip holds s on the end segments).  k = the preview's segment of s (the last segment with cum[k] <= s, 0
 *          when none), (X, Y) and the unit tangent (ux, uy) the preview's station there in the MAP frame:
 *          t = clip((s - cum[k]) / len[k], 0, 1), X = ax + t * dx, Y = ay + t * dy, ux = dx / len, uy = dy / len.
 *          p = (X - lat_o * uy, Y + lat_o * ux).  This mode needs a track (f110_track_set) on every map slot in use (the planner: on
 *          the slots of the armed agents); tracking need not be enabled.
 * Per candidate.  The candidate's position is its MAP-frame state[0..1] after action h's last repeat, whatever the spec's frame; a
 *   candidate the map has killed repeats its frozen pose.  m = +inf, free = H, hit = false; for h ascending and o ascending:
 *     dx = x - p.x, dy = y - p.y, d = sqrt(dx * dx + dy * dy);
 *     if (d < m) m = d;   if (!hit && d < radius) { hit = true; free = h; }
 *   A NaN d does neither.  OPP_MIN = m, OPP_FREE = free.
 * Rollout.  f110_rollout_opp_device is f110_rollout_device plus d_opp [N][K][2] float32 = ((float)OPP_MIN, (float)OPP_FREE);
 *   d_out and d_traj are bit for bit what f110_rollout_device writes; the same stream and env-block behaviour (an env's cars are
 *   always in one block).
 * Planner.  f110_mppi_set_opponents attaches the term to the ARMED planner with two weights and a reference distance; it launches
 *   nothing.  With the term attached f110_mppi_device and a F110_STEP_SCRIPTED step cost every candidate as
 *     c = w_dead * ...;  c = c + w_clear * ...;
 *     c = c + w_hit * (double)(H - OPP_FREE);
 *     c = c + w_near * (OPP_MIN < near_ref ? near_ref - OPP_MIN : 0.0);
 *     c = c - w_progress * ...;  c = c + w_lat * ...;   a NaN c becomes +inf
 *   opp == NULL detaches it; f110_mppi_set, arming anew or disarming, drops it.  The term has no state of its own:
 *   f110_mppi_get / f110_mppi_put are unchanged.  Its prediction table is the planner's memory and goes with it.
 * Refused with F110_ERR_INVALID, nothing launched, written or changed: an unknown mode, a radius that is not finite and > 0, a
 *   max_range that is NaN or <= 0, a weight that is not finite or < 0, a near_ref that is not finite, a null d_opp, Ao outside
 *   0 .. 31 (the device forms: A - 1 > 31), and everything the rollout's and the planner's own calls refuse.
 * Refused with F110_ERR_STATE: no planner armed, no map (the rollout's forms: F110_ERR_NO_MAP, as f110_rollout_*), TRACK while a map
 *   slot in use has no track — checked when attaching and again at every call.
 * Not offered: the opponents' footprints (a disc of `radius` around the reference points), interaction (the opponents do not react
 *   to the candidate), a prediction from anything but the live state, per-opponent settings. */
enum { F110_OPP_CV = 0, F110_OPP_TRACK = 1 };
enum { F110_OPP_MAX = 31 };
typedef struct f110_opponents {
    int32_t mode;       /* F110_OPP_CV / F110_OPP_TRACK */
    int32_t pad_;       /* ignored */
    double radius;      /* metres, finite, > 0: a sample closer than this to a predicted opponent is a hit */
    double max_range;   /* metres, > 0, +inf allowed, not NaN: an opponent further than this from the agent at the start is ignored */
} f110_opponents;       /* 24 bytes */
/* f110_rollout_device with the opponent term: d_opp [N][K][2] float32 in device memory.  h_pinned receives d_out's copy. */
int f110_rollout_opp_device(f110_sim *h, const f110_rollout *spec, const f110_opponents *opp, const double *d_actions,
                            float *d_out /* [N][K][D] */, float *d_traj /* [N][K][H][4] or NULL */, float *d_opp /* [N][K][2] */,
                            float *h_pinned);
/* f110_rollout_batch with the opponent term on host rows: h_opp_rows [m][Ao][4] = (x, y, v, theta) of row r's opponents,
 * 0 <= Ao <= 31 (NULL with Ao = 0).  Outputs beside f110_rollout_batch's, each may be NULL: h_pred [m][Ao][H][2] float64 the
 * predictions, h_opp_raw [m][K][2] float64 (OPP_MIN, (double)OPP_FREE), h_opp [m][K][2] float32 what the device form writes. */
int f110_rollout_opp_batch(f110_sim *h, const f110_rollout *spec, const f110_opponents *opp, int32_t slot,
                           const double *h_start /* [m][10] */, const double *h_params /* [m][18] or NULL */, const double *h_actions,
                           const double *h_opp_rows /* [m][Ao][4] */, int32_t Ao, int32_t m, float *h_out /* [m][K][D] */,
                           double *h_raw /* [m][K][10] or NULL */, float *h_traj /* or NULL */, double *h_traj_raw /* or NULL */,
                           double *h_pred /* [m][Ao][H][2] or NULL */, double *h_opp_raw /* [m][K][2] or NULL */,
                           float *h_opp /* [m][K][2] or NULL */);
/* attaches the opponent term to the armed planner (opp == NULL: detaches it; the numbers are then ignored).  Launches nothing. */
int f110_mppi_set_opponents(f110_sim *h, const f110_opponents *opp, double w_hit, double w_near, double near_ref);
/* f110_mppi_batch with the opponent term on host rows: h_opp_rows [m][Ao][4] as above; h_opp_raw [m][K][2] float64 (or NULL) the
 * candidates' (OPP_MIN, (double)OPP_FREE).  The planner armed on the handle, and what is attached to it, is not touched. */
int f110_mppi_opp_batch(f110_sim *h, const f110_mppi *spec, const f110_opponents *opp, double w_hit, double w_near, double near_ref,
                        int32_t slot, const double *h_start /* [m][10] */, const double *h_params /* [m][18] or NULL */,
                        const int32_t *h_fresh /* [m] or NULL */, const double *h_opp_rows /* [m][Ao][4] */, int32_t Ao, int32_t m,
                        double *h_nominal /* [m][H][2] */, uint64_t *h_streams /* [m][4] */, double *h_actions /* [m][2] */,
                        float *h_info /* [m][4] */, double *h_cand /* [m][K][H][2] */, double *h_cost /* [m][K] */,
                        double *h_weight /* [m][K] */, double *h_opp_raw /* [m][K][2] or NULL */);

/* ---- particle filter: Monte-Carlo localisation per agent from its lidar scan (no reference counterpart: the particle filter of the
 * MIT racecar stack that F1TENTH cars localise with, here against the distance table the simulator already keeps) ----
 * It runs only when called (f110_pf_device), changes no simulator state and no blob format.  A filter is armed on a handle with ONE
 * spec, a strictly ascending list of M agent indices (the armed agents, 1 <= M <= N) and one PCG64 stream per armed agent (the
 * words of f110_pcg64_seed_spawn).  The handle owns per armed agent the cloud X[P][3] (x, y, theta of the car's reference point),
 * the normalised weights W[P], the last true pose last[3] and the stream position.  They are configuration of the filter, not
 * simulator state: the state blobs do not contain them (f110_pf_get / f110_pf_put checkpoint them next to a blob).  Arming stores
 * a cloud of zeros with W = 1 / P and last = 0: a row becomes a cloud around its car at its first call with step_count == 0 (right
 * after a reset), or through f110_pf_put.  Everything is float64 without contraction.
 * One call does, for every armed agent n (the rows of other agents are never read or written), with P = particles, B' = n_beams,
 * (x, y, th) = the agent's row of the observation's poses_x / poses_y / poses_theta and z[j] = beam b_j = beam_first +
 * j * beam_stride of its live scan:
 *   1 draws       sub-stream q of the agent's generator is the generator advanced by q * 2^16 steps (numpy.random.PCG64.advance).
 *                 Sub-stream 0 yields u = Generator.random() (one output); sub-stream p + 1 yields particle p's e_x, e_y, e_t, three
 *                 Generator.standard_normal() in this order.  After the call the generator stands 2^28 steps further on, whatever
 *                 P is.
 *   2 fresh row   if step_count[n] == 0: X[p] = (x + init_x * e_x, y + init_y * e_y, wrap(th + init_theta * e_t)), W[p] = 1 / P,
 *                 a_p = p; 3 and 4 are skipped.  wrap(t) = t > 2 pi ? t - 2 pi : (t < 0 ? t + 2 pi : t), the step's own yaw wrap.
 *   3 resample    ess = 1 / sum W[p]^2.  If ess < resample_frac * (double)P: C_j = sum_{i <= j} W[i]; for slot i
 *                 t_i = ((double)i + u) / (double)P * C_{P-1}, the ancestor a_i is the least j with C_j > t_i (P - 1 if none), the
 *                 new X[i] is the old X[a_i] and W[i] = 1 / P (systematic resampling).  Otherwise a_i = i.
 *   4 motion      dx = x - last.x, dy = y - last.y, a = cos(last.th) * dx + sin(last.th) * dy, b = -sin(last.th) * dx +
 *                 cos(last.th) * dy, dth = th - last.th, then dth - 2 pi if dth > pi, dth + 2 pi if dth <= -pi.  Per particle
 *                 fa = a + sigma_x * e_x, fb = b + sigma_y * e_y, and with c = cos(X.th), s = sin(X.th) of the old heading
 *                   X.x = X.x + (c * fa - s * fb),  X.y = X.y + (s * fa + c * fb),  X.th = wrap(X.th + dth + sigma_theta * e_t)
 *   5 sensor      the particle's lidar pose is formed from X[p] as the step forms scan_pose from the state (lidar_dist along the
 *                 heading).  r[p][j] is beam b_j of the noise-free scan at that pose on the env's map slot: the number
 *                 f110_scan_batch returns for that pose and beam (the handle's trig tables, eps and max_range).
 *                 e = (z[j] - r[p][j]) / sigma_hit, e2 = e * e, t_j = e2 if e2 < clip * clip, else clip * clip; a NaN e2 takes
 *                 the clip, or counts as 0.0 when clip * clip is +inf.  L[p] = -(0.5 / squash) * sum_j t_j.
 *   6 weights     Lmax = max L, w_p = W[p] * exp(L[p] - Lmax), eta = sum w_p, W'[p] = w_p / eta, or 1 / P for every p if
 *                 !(eta > 0).
 *   7 estimate    xh = sum W'[p] * X[p].x, yh = sum W'[p] * X[p].y, thh = atan2(sum W'[p] * sin(X[p].th), sum W'[p] * cos(X[p].th)).
 *                 The agent's row of d_pose [N][3] float64 is (xh, yh, thh); of d_info [N][4] float32 (or NULL):
 *                 (float)(1 / sum W'[p]^2), (float)sqrt(sum W'[p] * ((X.x - xh)^2 + (X.y - yh)^2)), (float)hypot(xh - x, yh - y),
 *                 1.0 if 3 resampled, else 0.0.  Then last = (x, y, th), and X and W' are stored.
 * Every sum runs over ascending indices from 0.0, on the device too (one lane walks it): given their terms the sums are defined bit
 * for bit, and so are the draws, the ancestors, the motion's additions and L given r.  exp, sin, cos, atan2, hypot and sqrt are the
 * device's; the rays are the scan's.
 * Refused with F110_ERR_INVALID, nothing changed: particles outside 1..1024, n_beams outside 1..128, beam_first < 0, beam_stride < 1,
 *   beam_first + (n_beams - 1) * beam_stride >= num_beams, a sigma or init sigma < 0, sigma_hit, clip or squash <= 0,
 *   resample_frac < 0, any setting not finite except clip = +inf; a list that is not strictly ascending or has an index outside
 *   0 .. N - 1; M * P * B' >= 2^31.  F110_ERR_STATE: nothing armed, or no map.
 * Not offered: global localisation (a cloud over all free space), several specs per handle, a four-component beam model or a
 * precomputed sensor table, KLD / adaptive P, noise proportional to the motion, opponents in the expected ranges (their returns are
 * what clip is for), float32 particles, the filter inside the state blobs. */
enum { F110_PF_MAX_P = 1024, F110_PF_MAX_BEAMS = 128 };
typedef struct f110_pf {
    int32_t particles;    /* P, 1..1024 */
    int32_t n_beams;      /* B', 1..128 beams of the agent's scan that are compared */
    int32_t beam_first;   /* >= 0 */
    int32_t beam_stride;  /* >= 1; beam_first + (n_beams - 1) * beam_stride < the handle's num_beams */
    double sigma_x, sigma_y, sigma_theta;   /* >= 0: odometry noise per call, car frame */
    double init_x, init_y, init_theta;      /* >= 0: the fresh cloud around the true pose */
    double sigma_hit;     /* > 0, metres */
    double clip;          /* > 0, in sigmas; +inf allowed: no truncation */
    double squash;        /* > 0: the log-likelihood is divided by it */
    double resample_frac; /* >= 0, finite: resample when ESS < resample_frac * P */
} f110_pf;               /* 4 * 4 + 10 * 8 = 96 bytes */
/* arms the filter: h_agents [m] strictly ascending, h_streams [m][4] uint64.  NULL, NULL, 0, NULL disarms it and frees its memory.
 * The new filter is built aside and swapped in on success; nothing is launched and no step looks at it. */
int f110_pf_set(f110_sim *h, const f110_pf *spec, const int32_t *h_agents, int32_t m, const uint64_t *h_streams /* [m][4] */);
/* one localisation call: the armed agents' rows of d_pose [N][3] float64 and of d_info [N][4] float32 (or NULL), device memory.
 * Asynchronous on the handle's stream; right behind a two-block step it runs per env block on the block's own stream, the ascending
 * list split at the block's bounds.  F110_ERR_STATE with nothing armed or without a map. */
int f110_pf_device(f110_sim *h, double *d_pose, float *d_info);
/* the filter's own memory, in the armed list's order: h_particles [m][P][3], h_weights [m][P], h_last [m][3], h_streams [m][4];
 * each may be NULL.  get waits for the handle's work; put refuses (F110_ERR_INVALID, nothing changed) a particle that is not finite
 * and a weight row with a negative or non-finite value or whose sum is not > 0.  F110_ERR_STATE with nothing armed. */
int f110_pf_get(f110_sim *h, double *h_particles, double *h_weights, double *h_last, uint64_t *h_streams);
int f110_pf_put(f110_sim *h, const double *h_particles, const double *h_weights, const double *h_last, const uint64_t *h_streams);
/* unit form on host arrays, the same kernels on uploaded rows: h_poses [m][3] the true poses on map slot `slot`, h_scans [m][B]
 * (B = num_beams), h_fresh [m] int32 (the rows' step_count; NULL: none is fresh); h_particles [m][P][3], h_weights [m][P], h_last
 * [m][3] and h_streams [m][4] in and out, checked as f110_pf_put checks them.  Outputs, each may be NULL: h_pose [m][3], h_info
 * [m][4], h_noise [m][P][3] (e_x, e_y, e_t), h_anc [m][P] int32 (a_p), h_expect [m][P][B'] (r), h_logw [m][P] (L).  The filter armed on
 * the handle, if any, is not touched. */
int f110_pf_batch(f110_sim *h, const f110_pf *spec, int32_t slot, const double *h_poses /* [m][3] */, const double *h_scans /* [m][B] */,
                  const int32_t *h_fresh /* [m] or NULL */, int32_t m, double *h_particles /* [m][P][3] */, double *h_weights /* [m][P] */,
                  double *h_last /* [m][3] */, uint64_t *h_streams /* [m][4] */, double *h_pose /* [m][3] */, float *h_info /* [m][4] */,
                  double *h_noise /* [m][P][3] */, int32_t *h_anc /* [m][P] */, double *h_expect /* [m][P][B'] */, double *h_logw /* [m][P] */);

#ifdef __cplusplus
}
#endif
#endif /* F110_H */
