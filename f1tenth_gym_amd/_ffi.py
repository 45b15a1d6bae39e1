"""ctypes binding of libf110_hip.so (include/f110.h).  No torch, no cffi.

The library is the product: if it cannot be loaded, or no MI355X is visible, every entry point
raises — there is deliberately no CPU fallback (the CPU oracle lives under oracle/ and is
test infrastructure only; nothing here imports it).
"""
import ctypes as C
import os

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
# F110_LIB_VARIANT=experimental (read HERE, by the Python host — the library reads no environment) selects
# libf110_hip_exp.so: the product plus every variant that was measured and not adopted, and f110_exp_set
VARIANT = "experimental" if os.environ.get("F110_LIB_VARIANT", "product").lower().startswith("exp") else "product"
LIB_PATH = os.path.join(_PKG, "libf110_hip_exp.so" if VARIANT == "experimental" else "libf110_hip.so")
ABI_VERSION = 1
NPARAMS = 18
PARAM_KEYS = ['mu', 'C_Sf', 'C_Sr', 'lf', 'lr', 'h', 'm', 'I', 's_min', 's_max', 'sv_min',
              'sv_max', 'v_switch', 'a_max', 'v_min', 'v_max', 'width', 'length']

OK, ERR_INVALID, ERR_NO_MAP, ERR_HIP, ERR_STATE, ERR_NOMEM = 0, -1, -2, -3, -4, -5
MAP_ROWMAJOR_F64, MAP_TILED_F64, MAP_CODE8, MAP_PADDED_F64, MAP_WINDOW_LDS = 0, 1, 2, 3, 4
MAP_DEFAULT = MAP_PADDED_F64   # fastest; falls back to row-major for maps too large for it
INTEGRATOR_RK4, INTEGRATOR_EULER = 1, 2

_dp = C.POINTER(C.c_double)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("num_envs", C.c_int32), ("num_agents", C.c_int32),
                ("num_beams", C.c_int32), ("theta_dis", C.c_int32), ("integrator", C.c_int32),
                ("device_id", C.c_int32), ("map_layout", C.c_int32), ("scan_block", C.c_int32),
                ("scan_tasks_per_wave", C.c_int32), ("step_groups", C.c_int32), ("step_graph", C.c_int32), ("fov", C.c_double), ("eps", C.c_double),
                ("max_range", C.c_double), ("time_step", C.c_double), ("lidar_dist", C.c_double),
                ("ttc_thresh", C.c_double), ("params", C.c_double * NPARAMS)]


class ObsHost(C.Structure):
    _fields_ = [("scans", _dp), ("poses_x", _dp), ("poses_y", _dp), ("poses_theta", _dp),
                ("linear_vels_x", _dp), ("ang_vels_z", _dp), ("collisions", _dp),
                ("collision_idx", _dp), ("state", _dp), ("agent_poses", _dp),
                ("in_collision", _i32p), ("step_count", _i32p)]


class EpisodeHost(C.Structure):
    _fields_ = [("lap_times", _dp), ("lap_counts", _dp), ("toggles", _dp), ("current_time", _dp),
                ("near_starts", _u8p), ("done", _u8p), ("checkpoint_done", _u8p)]


class ResetSamplerSpec(C.Structure):
    """struct f110_reset_sampler"""
    _fields_ = [("s_lo", C.c_double), ("s_hi", C.c_double), ("gap", C.c_double), ("lateral", C.c_double),
                ("heading", C.c_double), ("clearance", C.c_double), ("attempts", C.c_int32), ("pad", C.c_int32)]


class ParamDist(C.Structure):
    """struct f110_param_dist"""
    _fields_ = [("kind", C.c_int32), ("scope", C.c_int32), ("a", C.c_double), ("b", C.c_double), ("lo", C.c_double),
                ("hi", C.c_double), ("relative", C.c_int32), ("pad", C.c_int32)]


PARAM_FIXED, PARAM_UNIFORM, PARAM_NORMAL = 0, 1, 2
PARAM_SCOPE_AGENT, PARAM_SCOPE_ENV = 0, 1


class ObsSpec(C.Structure):
    """struct f110_obs_spec"""
    _fields_ = [("beam_lo", C.c_int32), ("beam_hi", C.c_int32), ("sectors", C.c_int32), ("pool", C.c_int32),
                ("features", C.c_int32), ("frames", C.c_int32), ("flags", C.c_int32), ("pad", C.c_int32),
                ("range_clip", C.c_double), ("range_scale", C.c_double), ("feat_scale", C.c_double * 8)]


OBS_POOL_MIN, OBS_POOL_MEAN, OBS_POOL_CENTER = 0, 1, 2
OBS_FILL, OBS_MAX_FRAMES, OBS_MAX_STACK = 1, 16, 8192


class GapFollowerSpec(C.Structure):
    """struct f110_gap_follower"""
    _fields_ = [("beam_lo", C.c_int32), ("beam_hi", C.c_int32), ("smooth", C.c_int32), ("target", C.c_int32),
                ("range_clip", C.c_double), ("bubble_radius", C.c_double), ("gap_threshold", C.c_double),
                ("steer_gain", C.c_double), ("steer_max", C.c_double), ("v_lo", C.c_double), ("v_hi", C.c_double), ("d_ref", C.c_double),
                ("steer_slow", C.c_double), ("v_turn", C.c_double), ("v_blocked", C.c_double)]


GAP_TARGET_CENTER, GAP_TARGET_FURTHEST = 0, 1
GAP_MAX_SPECS, GAP_MAX_SMOOTH, GAP_MAX_WINDOW = 8, 63, 4096
STEP_SCRIPTED = 64


class TrackPreviewSpec(C.Structure):
    """struct f110_track_preview"""
    _fields_ = [("points", C.c_int32), ("channels", C.c_int32), ("frame", C.c_int32), ("flags", C.c_int32),
                ("offset", C.c_double), ("spacing", C.c_double), ("scale", C.c_double * 8)]


PREVIEW_X, PREVIEW_Y, PREVIEW_TAN_X, PREVIEW_TAN_Y, PREVIEW_ATTR0, PREVIEW_ATTR1, PREVIEW_ATTR2, PREVIEW_ATTR3 = (1 << b for b in range(8))
PREVIEW_NCHANNELS, PREVIEW_FRAME_EGO, PREVIEW_FRAME_WORLD, PREVIEW_MAX_POINTS, TRACK_MAX_ATTRS = 8, 0, 1, 32, 4


class NeighborsSpec(C.Structure):
    """struct f110_neighbors"""
    _fields_ = [("k", C.c_int32), ("channels", C.c_int32), ("flags", C.c_int32), ("pad_", C.c_int32),
                ("max_range", C.c_double), ("pad", C.c_double), ("scale", C.c_double * 10)]


NBR_DX, NBR_DY, NBR_DIST, NBR_COS_DTH, NBR_SIN_DTH, NBR_V_X, NBR_V_Y, NBR_GAP_S, NBR_VALID, NBR_INDEX = (1 << b for b in range(10))
NBR_NCHANNELS, NBR_MAX_K, NBR_MAX_AGENTS = 10, 8, 256

LINE_FLOATS = ("look_base", "look_gain", "look_min", "look_max", "lane_offset", "wheelbase", "steer_max", "v_const", "vgain", "speed_look",
               "lat_slow", "v_recover", "follow_range", "follow_gap", "follow_gain", "lane_width", "v_min", "v_max")


class LineFollowerSpec(C.Structure):
    """struct f110_line_follower"""
    _fields_ = [(k, C.c_double) for k in LINE_FLOATS] + [("speed_attr", C.c_int32), ("pad_", C.c_int32)]


LINE_MAX_SPECS, LINE_MAX_AGENTS, LINE_NRAW, LINE_NINFO = 8, 256, 12, 4


class Obstacle(C.Structure):
    """struct f110_obstacle"""
    _fields_ = [("shape", C.c_int32), ("reserved", C.c_int32), ("x", C.c_double), ("y", C.c_double), ("c", C.c_double), ("s", C.c_double),
                ("half_length", C.c_double), ("half_width", C.c_double)]


OBST_BOX, OBST_DISC, MAX_OBSTACLES = 0, 1, 256


class RolloutSpec(C.Structure):
    """struct f110_rollout"""
    _fields_ = [("k", C.c_int32), ("horizon", C.c_int32), ("repeat", C.c_int32), ("layout", C.c_int32), ("frame", C.c_int32),
                ("channels", C.c_int32), ("traj", C.c_int32), ("pad_", C.c_int32), ("margin", C.c_double), ("scale", C.c_double * 10)]


(ROLL_END_X, ROLL_END_Y, ROLL_END_COS, ROLL_END_SIN, ROLL_END_V, ROLL_END_YAW_RATE, ROLL_ALIVE, ROLL_MIN_CLEAR, ROLL_PROGRESS,
 ROLL_END_LAT) = (1 << b for b in range(10))
ROLL_NCHANNELS, ROLL_SHARED, ROLL_PER_AGENT, ROLL_FRAME_EGO, ROLL_FRAME_MAP = 10, 0, 1, 0, 1
ROLL_MAX_K, ROLL_MAX_H, ROLL_MAX_REPEAT = 256, 64, 16


class MppiSpec(C.Structure):
    """struct f110_mppi"""
    _fields_ = [("k", C.c_int32), ("horizon", C.c_int32), ("repeat", C.c_int32), ("shift", C.c_int32), ("margin", C.c_double),
                ("sigma_steer", C.c_double), ("sigma_speed", C.c_double), ("steer_min", C.c_double), ("steer_max", C.c_double),
                ("speed_min", C.c_double), ("speed_max", C.c_double), ("lambda_", C.c_double), ("w_dead", C.c_double),
                ("w_clear", C.c_double), ("w_progress", C.c_double), ("w_lat", C.c_double), ("clear_ref", C.c_double), ("v_init", C.c_double)]


MPPI_MAX_K, MPPI_MAX_H, MPPI_MAX_REPEAT = 256, 64, 16


class OpponentsSpec(C.Structure):
    """struct f110_opponents"""
    _fields_ = [("mode", C.c_int32), ("pad_", C.c_int32), ("radius", C.c_double), ("max_range", C.c_double)]


OPP_CV, OPP_TRACK, OPP_MAX = 0, 1, 31


class PfSpec(C.Structure):
    """struct f110_pf"""
    _fields_ = [("particles", C.c_int32), ("n_beams", C.c_int32), ("beam_first", C.c_int32), ("beam_stride", C.c_int32),
                ("sigma_x", C.c_double), ("sigma_y", C.c_double), ("sigma_theta", C.c_double), ("init_x", C.c_double),
                ("init_y", C.c_double), ("init_theta", C.c_double), ("sigma_hit", C.c_double), ("clip", C.c_double),
                ("squash", C.c_double), ("resample_frac", C.c_double)]


PF_MAX_P, PF_MAX_BEAMS = 1024, 128


class EpisodeViews(C.Structure):
    _fields_ = [("done", C.c_void_p), ("checkpoint_done", C.c_void_p), ("lap_times", C.c_void_p),
                ("lap_counts", C.c_void_p), ("toggles", C.c_void_p), ("current_time", C.c_void_p)]


class HostBlock(C.Structure):
    """f110_host_block: where f110_step_host writes (page-locked memory of f110_host_alloc)"""
    _fields_ = [("state", _dp), ("collisions", _dp), ("collision_idx", _dp), ("agent_poses", _dp),
                ("lap_times", _dp), ("lap_counts", _dp), ("toggles", _dp), ("current_time", _dp),
                ("in_collision", _i32p), ("near_starts", _u8p), ("checkpoint_done", _u8p), ("done", _u8p),
                ("scans", _dp)]


GATHER_F64, GATHER_F32 = 0, 1
STATE_SCANS = 1          # f110_state_* flags: the blob also holds the last scans
STATE_HEADER_BYTES, STATE_VERSION = 256, 1
STEP_AUTO_RESET, STEP_NO_SYNC, STEP_ACTIONS_MAPPED, STEP_SPIN_WAIT, STEP_NO_FUSE, STEP_POLL = 1, 2, 4, 8, 16, 32


class DeviceViews(C.Structure):
    _fields_ = [("scans", C.c_void_p), ("state", C.c_void_p), ("agent_poses", C.c_void_p),
                ("collisions", C.c_void_p), ("collision_idx", C.c_void_p),
                ("in_collision", C.c_void_p), ("step_count", C.c_void_p), ("stream", C.c_void_p)]


class TrackViews(C.Structure):
    """struct f110_track_views: device pointers of the step's track columns"""
    _fields_ = [("s", C.c_void_p), ("ds", C.c_void_p), ("lateral", C.c_void_p), ("heading_error", C.c_void_p),
                ("segment", C.c_void_p)]


class TrackHost(C.Structure):
    """f110_track_host: host destinations of the track columns (any may be NULL)"""
    _fields_ = [("s", _dp), ("ds", _dp), ("lateral", _dp), ("heading_error", _dp), ("segment", _i32p)]


# name -> (restype, argtypes); every symbol include/f110.h declares
PROTOTYPES = {
    "f110_last_error": (C.c_char_p, [C.c_void_p]),
    "f110_abi_version": (C.c_int, []),
    "f110_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "f110_device_pci_bus_id": (C.c_int, [C.c_int32, C.c_char_p, C.c_int32]),
    "f110_build_info": (C.c_char_p, []),
    "f110_device_allocs": (C.c_int, [C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "f110_is_experimental": (C.c_int, []),
    "f110_exp_set": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32]),
    "f110_create": (C.c_int, [C.POINTER(Config), C.POINTER(C.c_void_p)]),
    "f110_destroy": (None, [C.c_void_p]),
    "f110_sync": (C.c_int, [C.c_void_p]),
    "f110_set_map_image": (C.c_int, [C.c_void_p, _u8p, C.c_int32, C.c_int32] + [C.c_double] * 4),
    "f110_set_map_dt": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_int32] + [C.c_double] * 5),
    "f110_get_map_dt": (C.c_int, [C.c_void_p, _dp]),
    "f110_map_shape": (C.c_int, [C.c_void_p, _i32p, _i32p]),
    "f110_set_trig_tables": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32]),
    "f110_set_beam_tables": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_int32]),
    "f110_set_params": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "f110_set_noise_table": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_int32]),
    "f110_set_noise_rng": (C.c_int, [C.c_void_p, _u64p, C.c_int32, C.c_double, C.c_int32]),
    "f110_pcg64_seed": (C.c_int, [C.c_uint64, _u64p]),
    "f110_noise_prepare": (C.c_int, [C.c_void_p, C.c_int32]),
    "f110_noise_rows_batch": (C.c_int, [C.c_void_p, _u64p, C.c_double, C.c_int32, C.c_int32, _dp, _u64p]),
    "f110_scan_lookup_count": (C.c_int, [C.c_void_p, C.c_int32, _i64p]),
    "f110_reset": (C.c_int, [C.c_void_p, _dp, _u8p]),
    "f110_reset_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "f110_add_map_image": (C.c_int, [C.c_void_p, _u8p, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, _i32p]),
    "f110_add_map_dt": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i32p]),
    "f110_set_env_maps": (C.c_int, [C.c_void_p, _i32p]),
    "f110_add_map_obstacles": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Obstacle), C.c_int32, _i32p]),
    "f110_set_map_obstacles": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(Obstacle), C.c_int32]),
    "f110_get_slot_dt": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "f110_slot_shape": (C.c_int, [C.c_void_p, C.c_int32, _i32p, _i32p]),
    "f110_slot_table": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), _i32p]),
    "f110_add_map_corridor": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, _i32p]),
    "f110_set_map_corridor": (C.c_int, [C.c_void_p, C.c_int32, _dp, _dp, C.c_int32, C.c_int32]),
    "f110_corridor_mask_batch": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, C.c_int32, C.c_int32, C.c_int32] + [C.c_double] * 5 + [_u8p, _i64p]),
    "f110_map_corridor_times": (C.c_int, [C.c_void_p, _dp]),
    "f110_raceline_batch": (C.c_int, [C.c_void_p, _dp, _dp, _i32p, C.c_int32, C.c_int32, C.c_int32] + [C.c_double] * 5 + [_dp, _i32p] + [_dp] * 6),
    "f110_map_centerline": (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_int32, _i32p, _dp, C.c_int32, _i32p, _i64p]),
    "f110_map_skeleton": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, _u8p, _i64p]),
    "f110_slot_frame": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "f110_map_centerline_times": (C.c_int, [C.c_void_p, _dp]),
    "f110_set_params_batch": (C.c_int, [C.c_void_p, _dp]),
    "f110_reset_collided_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "f110_set_auto_reseat": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "f110_episode_init": (C.c_int, [C.c_void_p, C.c_int32]),
    "f110_episode_reset": (C.c_int, [C.c_void_p, _dp, _dp, _u8p]),
    "f110_episode_step_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_episode_reset_done_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_episode_get": (C.c_int, [C.c_void_p, C.POINTER(EpisodeHost)]),
    "f110_episode_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "f110_episode_packed_bytes": (C.c_size_t, [C.c_void_p]),
    "f110_host_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "f110_host_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_episode_device_views": (C.c_int, [C.c_void_p, C.POINTER(EpisodeViews)]),
    "f110_step_host": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(HostBlock), C.c_int32]),
    "f110_step_host_stats": (C.c_int, [C.c_void_p, _dp]),
    "f110_step": (C.c_int, [C.c_void_p, _dp]),
    "f110_step_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_get_obs": (C.c_int, [C.c_void_p, C.POINTER(ObsHost)]),
    "f110_set_state": (C.c_int, [C.c_void_p, _dp, _dp, _i32p]),
    "f110_state_bytes": (C.c_size_t, [C.c_void_p, C.c_int32, C.c_int32]),
    "f110_state_save_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]),
    "f110_state_load_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "f110_clone_envs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "f110_state_save": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32]),
    "f110_state_load": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_get_device_views": (C.c_int, [C.c_void_p, C.POINTER(DeviceViews)]),
    "f110_stream_fence": (C.c_int, [C.c_void_p]),
    "f110_device_mem_info": (C.c_int, [C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    "f110_device_alloc": (C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]),
    "f110_device_free": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_memcpy_h2d": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "f110_memcpy_d2h": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "f110_comm_unique_id": (C.c_int, [C.c_void_p]),
    "f110_comm_init": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "f110_comm_all_gather_scans": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_comm_all_gather_obs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "f110_comm_gather_obs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "f110_comm_info": (C.c_int, [C.c_void_p, _i32p, _i32p]),
    "f110_step_groups": (C.c_int, [C.c_void_p, _i32p, _i32p, _i32p]),
    "f110_step_launches": (C.c_int, [C.c_void_p, _i32p]),
    "f110_comm_set_overlap": (C.c_int, [C.c_void_p, C.c_int32]),
    "f110_comm_destroy": (C.c_int, [C.c_void_p]),
    "f110_timer_begin": (C.c_int, [C.c_void_p]),
    "f110_timer_end_ms": (C.c_int, [C.c_void_p, _dp]),
    "f110_profile_kernels": (C.c_int, [C.c_void_p, C.c_int32]),
    "f110_profile_read": (C.c_int, [C.c_void_p, _i32p, _dp, _dp, _dp]),
    "f110_scan_batch": (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp, _i32p, _i64p]),
    "f110_scan_path_stats": (C.c_int, [C.c_void_p, C.c_int32, _i64p]),
    "f110_pure_pursuit_batch": (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, _dp]),
    "f110_pure_pursuit_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "f110_pure_pursuit_poses_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double,
                                                 C.c_void_p]),
    "f110_scan_policy_device": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "f110_dynamics_batch": (C.c_int, [C.c_void_p, _dp, _dp, _dp, C.c_int32, _dp, _dp]),
    "f110_pid_batch": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, _dp]),
    "f110_update_pose_batch": (C.c_int, [C.c_void_p, _dp, _dp, _i32p, _dp, _dp, C.c_double, C.c_int32,
                                         C.c_double, C.c_int32, _dp, _dp, _i32p, _dp]),
    "f110_get_vertices_batch": (C.c_int, [C.c_void_p, _dp, C.c_double, C.c_double, C.c_int32, _dp]),
    "f110_gjk_batch": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, _i32p]),
    "f110_collision_multiple_batch": (C.c_int, [C.c_void_p, _dp, C.c_int32, C.c_int32, _dp, _dp]),
    "f110_ttc_batch": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, C.c_double, _i32p]),
    "f110_raycast_batch": (C.c_int, [C.c_void_p, _dp, _dp, C.c_int32, _dp, _i32p]),
    "f110_get_range_batch": (C.c_int, [C.c_void_p, _dp, C.c_int32, _dp]),
    "f110_track_set": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, C.c_int32]),
    "f110_track_enable": (C.c_int, [C.c_void_p, C.c_int32]),
    "f110_track_views": (C.c_int, [C.c_void_p, C.POINTER(TrackViews)]),
    "f110_track_get": (C.c_int, [C.c_void_p, C.POINTER(TrackHost)]),
    "f110_track_host_block": (C.c_int, [C.c_void_p, C.POINTER(TrackHost)]),
    "f110_track_project_batch": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, _dp]),
    "f110_track_set_attrs": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, C.c_int32]),
    "f110_track_preview_device": (C.c_int, [C.c_void_p, C.POINTER(TrackPreviewSpec), C.c_void_p, C.c_void_p]),
    "f110_track_preview_batch": (C.c_int, [C.c_void_p, C.POINTER(TrackPreviewSpec), C.c_int32, _dp, C.c_int32, C.c_void_p, _dp, _i32p]),
    "f110_neighbors_device": (C.c_int, [C.c_void_p, C.POINTER(NeighborsSpec), C.c_void_p, C.c_void_p]),
    "f110_neighbors_batch": (C.c_int, [C.c_void_p, C.POINTER(NeighborsSpec), C.c_int32, C.c_double, _dp, C.c_int32, C.c_void_p, _dp, _i32p]),
    "f110_line_followers_set": (C.c_int, [C.c_void_p, C.POINTER(LineFollowerSpec), C.c_int32, _i32p]),
    "f110_follow_line_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "f110_follow_line_batch": (C.c_int, [C.c_void_p, C.POINTER(LineFollowerSpec), C.c_int32, C.c_int32, _dp, C.c_int32, _dp, _dp]),
    "f110_rollout_device": (C.c_int, [C.c_void_p, C.POINTER(RolloutSpec), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "f110_rollout_batch": (C.c_int, [C.c_void_p, C.POINTER(RolloutSpec), C.c_int32, _dp, _dp, _dp, C.c_int32, C.c_void_p, _dp, C.c_void_p, _dp]),
    "f110_mppi_set": (C.c_int, [C.c_void_p, C.POINTER(MppiSpec), _i32p, C.c_int32, _u64p]),
    "f110_mppi_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "f110_mppi_get": (C.c_int, [C.c_void_p, _dp, _u64p]),
    "f110_mppi_put": (C.c_int, [C.c_void_p, _dp, _u64p]),
    "f110_mppi_batch": (C.c_int, [C.c_void_p, C.POINTER(MppiSpec), C.c_int32, _dp, _dp, _i32p, C.c_int32, _dp, _u64p, _dp, C.c_void_p, _dp, _dp, _dp]),
    "f110_rollout_opp_device": (C.c_int, [C.c_void_p, C.POINTER(RolloutSpec), C.POINTER(OpponentsSpec), C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "f110_rollout_opp_batch": (C.c_int, [C.c_void_p, C.POINTER(RolloutSpec), C.POINTER(OpponentsSpec), C.c_int32, _dp, _dp, _dp, _dp, C.c_int32,
                                         C.c_int32, C.c_void_p, _dp, C.c_void_p, _dp, _dp, _dp, C.c_void_p]),
    "f110_mppi_set_opponents": (C.c_int, [C.c_void_p, C.POINTER(OpponentsSpec), C.c_double, C.c_double, C.c_double]),
    "f110_mppi_opp_batch": (C.c_int, [C.c_void_p, C.POINTER(MppiSpec), C.POINTER(OpponentsSpec), C.c_double, C.c_double, C.c_double, C.c_int32,
                                      _dp, _dp, _i32p, _dp, C.c_int32, C.c_int32, _dp, _u64p, _dp, C.c_void_p, _dp, _dp, _dp, _dp]),
    "f110_pf_set": (C.c_int, [C.c_void_p, C.POINTER(PfSpec), _i32p, C.c_int32, _u64p]),
    "f110_pf_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "f110_pf_get": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _u64p]),
    "f110_pf_put": (C.c_int, [C.c_void_p, _dp, _dp, _dp, _u64p]),
    "f110_pf_batch": (C.c_int, [C.c_void_p, C.POINTER(PfSpec), C.c_int32, _dp, _dp, _i32p, C.c_int32, _dp, _dp, _dp, _u64p, _dp, C.c_void_p, _dp,
                                _i32p, _dp, _dp]),
    "f110_render_device": (C.c_int, [C.c_void_p, C.c_void_p, _i32p, C.c_int32, C.c_void_p, C.c_void_p, _u8p]),
    "f110_obs_encode_device": (C.c_int, [C.c_void_p, C.POINTER(ObsSpec), C.c_void_p, C.c_void_p]),
    "f110_obs_encode_batch": (C.c_int, [C.c_void_p, C.POINTER(ObsSpec), _dp, _dp, _i32p, C.c_int32, C.c_void_p]),
    "f110_controllers_set": (C.c_int, [C.c_void_p, C.POINTER(GapFollowerSpec), C.c_int32, _i32p]),
    "f110_follow_gap_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_follow_gap_batch": (C.c_int, [C.c_void_p, C.POINTER(GapFollowerSpec), _dp, _i32p, C.c_int32, _dp, _i32p]),
    "f110_pcg64_seed_spawn": (C.c_int, [_u32p, C.c_int32, C.c_uint64, C.c_int32, _u64p]),
    "f110_reset_sampler_set": (C.c_int, [C.c_void_p, C.c_void_p, _u64p]),
    "f110_reset_sample": (C.c_int, [C.c_void_p, _u8p]),
    "f110_reset_sample_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_reset_sampler_stats": (C.c_int, [C.c_void_p, _u64p, _i32p, C.c_int32]),
    "f110_reset_sampler_poses": (C.c_int, [C.c_void_p, _dp]),
    "f110_param_sampler_set": (C.c_int, [C.c_void_p, C.c_void_p, _u64p]),
    "f110_param_sample": (C.c_int, [C.c_void_p, _u8p]),
    "f110_param_sample_device": (C.c_int, [C.c_void_p, C.c_void_p]),
    "f110_param_sampler_stats": (C.c_int, [C.c_void_p, _u64p, C.c_int32]),
    "f110_params_get": (C.c_int, [C.c_void_p, _dp]),
    "f110_params_view": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "f110_param_sample_batch": (C.c_int, [C.c_void_p, C.c_void_p, _dp, C.c_int32, _u64p, C.c_int32, C.c_int32, _dp, _u64p]),
    "f110_episode_start_views": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "f110_edt_sq": (C.c_int, [C.c_void_p, _u8p, C.c_int32, C.c_int32, _u32p]),
    "f110_beam_dir_index_batch": (C.c_int, [C.c_void_p, _dp, C.c_int32, _i32p]),
    "f110_dt_from_bitmap": (C.c_int, [C.c_void_p, _u8p, C.c_int32, C.c_int32, C.c_double, _dp]),
    "f110_helper_batch": (C.c_int, [C.c_void_p, C.c_int32, _dp, C.c_int32, C.c_int32, _dp]),
}

# f110_helper_batch ops (include/f110.h)
(OP_ACCL_CONSTRAINTS, OP_STEERING_CONSTRAINT, OP_CROSS, OP_ARE_COLLINEAR, OP_PERPENDICULAR, OP_TRIPLE_PRODUCT, OP_AVG_POINT,
 OP_FURTHEST_POINT, OP_SUPPORT, OP_GET_TRMTX, OP_XY_2_RC, OP_DISTANCE_TRANSFORM, OP_TRACE_RAY) = range(1, 14)

_lib = None


class F110LibraryError(RuntimeError):
    """libf110_hip.so is missing/unloadable, or the HIP runtime reported an error."""


class ExperimentalOnly(F110LibraryError):
    """the call needs libf110_hip_exp.so (F110_LIB_VARIANT=experimental): a layout, a step form or a
    switch that was measured and not adopted into the product library"""


def lib():
    """Load libf110_hip.so (built in-tree by f1tenth_gym_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise F110LibraryError(
                "%s not found — build it with `python -m f1tenth_gym_amd.build` "
                "(there is no CPU fallback for the MI355X hot path)" % LIB_PATH)
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as ex:
            raise F110LibraryError("cannot load %s: %s" % (LIB_PATH, ex))
        for name, (res, args) in PROTOTYPES.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                raise F110LibraryError("%s does not export %s (stale build?)" % (LIB_PATH, name))
            fn.restype = res
            fn.argtypes = args
        if L.f110_abi_version() != ABI_VERSION:
            raise F110LibraryError("ABI version mismatch: library %d, binding %d"
                                   % (L.f110_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def last_error(handle=None):
    msg = lib().f110_last_error(handle)
    return msg.decode("utf-8", "replace") if msg else ""


def check(rc, handle=None, invalid_exc=ValueError):
    """Map a return code to the exception type the reference raises for the same condition."""
    if rc == OK:
        return
    msg = last_error(handle)
    if rc == ERR_NO_MAP:
        raise ValueError(msg or 'Map is not set for scan simulator.')   # laser_models.py:445-446
    if rc == ERR_INVALID:
        if "out of bounds for list of agents" in msg:
            raise IndexError(msg)                                        # base_classes.py:534
        if "Invalid Integrator" in msg:
            raise SyntaxError(msg)                                       # base_classes.py:398
        raise invalid_exc(msg)
    if rc == ERR_NOMEM:
        raise MemoryError(msg)
    if rc == ERR_STATE and "experimental build only" in msg:
        raise ExperimentalOnly(msg)
    raise F110LibraryError(msg or ("libf110_hip error %d" % rc))


def device_count():
    n = C.c_int(0)
    rc = lib().f110_device_count(C.byref(n))
    return n.value if rc == OK else 0


def device_allocs():
    """(live, bytes): the device allocations this process's handles own right now, and their size."""
    live, nbytes = C.c_int64(0), C.c_int64(0)
    check(lib().f110_device_allocs(C.byref(live), C.byref(nbytes)), None)
    return live.value, nbytes.value


def as_f64(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and tuple(a.shape) != tuple(shape):
        raise ValueError("expected array of shape %s, got %s" % (tuple(shape), tuple(a.shape)))
    return a


def dptr(a):
    return a.ctypes.data_as(_dp)


def i32ptr(a):
    return a.ctypes.data_as(_i32p)


def u64ptr(a):
    return a.ctypes.data_as(_u64p)


def params_vector(params):
    try:
        return np.array([float(params[k]) for k in PARAM_KEYS], dtype=np.float64)
    except KeyError as ex:
        raise KeyError("vehicle params dict is missing %s" % ex)
