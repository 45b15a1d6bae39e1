"""f1tenth_gym_amd — MI355X-native batched F1TENTH env.step() hot path.

Python host + ctypes over a C ABI (include/f110.h) + hand-written HIP kernels for gfx950.
The names mirror the reference package f110_gym.envs so existing code ports by changing the
import:  F110Env, Simulator, Integrator, ScanSimulator2D and the free kernel functions.
"""
from .core import BatchSim, DeviceArray, StateBlob, DEFAULT_PARAMS  # noqa: F401
from .sim import Integrator, Simulator  # noqa: F401
from .laser import ScanSimulator2D  # noqa: F401
from .racecar import RaceCar  # noqa: F401
from .env import F110Env, F110VecEnv  # noqa: F401
from .sharded import ShardedVecEnv  # noqa: F401
from .planner import PurePursuitPlanner  # noqa: F401
from .track import Track  # noqa: F401
from .reset_sampler import ResetSampler  # noqa: F401
from .param_sampler import ParamSampler  # noqa: F401
from .obs_encoder import ObsEncoder  # noqa: F401
from .gap_follower import GapFollower  # noqa: F401
from .line_follower import LineFollower  # noqa: F401
from .track_preview import TrackPreview  # noqa: F401
from .neighbors import Neighbors  # noqa: F401
from .rollout import Rollout  # noqa: F401
from .mppi import Mppi  # noqa: F401
from .opponents import Opponents  # noqa: F401
from .particle_filter import ParticleFilter  # noqa: F401
from .obstacles import Obstacles  # noqa: F401
from .trackgen import TrackMap, random_track  # noqa: F401
from .raceline import Raceline  # noqa: F401
from . import render  # noqa: F401
from ._ffi import device_allocs  # noqa: F401
from .functional import (accl_constraints, steering_constraint, vehicle_dynamics_ks, vehicle_dynamics_st, pid, func_KS, func_ST,  # noqa: F401
                         perpendicular, tripleProduct, avgPoint, indexOfFurthestPoint, support, collision, collision_multiple,
                         get_trmtx, get_vertices, get_dt, xy_2_rc, distance_transform, trace_ray, get_scan, check_ttc_jit, cross,
                         are_collinear, get_range, get_blocked_view_indices, ray_cast)

__version__ = "0.1.0"


def register_gym():
    """Register 'f110-v0' like gym/f110_gym/__init__.py:1-5 (needs gym)."""
    from gym.envs.registration import register
    register(id='f110-v0', entry_point='f1tenth_gym_amd.env:F110Env')
