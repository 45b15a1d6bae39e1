"""`F110Env` — the reference's gym façade (f110_env.py:53-418) over the MI355X simulator, plus
`F110VecEnv`, the batched form RL loops should use (E envs per step, observations as arrays).

Kept from the reference: constructor kwargs and defaults (:104-159), `reset(poses)` that
advances one zero-action step and returns a 4-tuple (:306-349), `step(action)` returning
(obs, reward=timestep, done, info={'checkpoint_done': ...}) (:263-304), the lap/finish logic
(:204-246), `update_map`, `update_params`, `add_render_callback`.  `render('rgb_array')` draws the
scene on the device; the pyglet window ('human', 'human_fast') is out of scope and raises
NotImplementedError.
`gym` is optional: when importable F110Env subclasses gym.Env, otherwise `object`.
"""
import copy
import os

import numpy as np

from . import _ffi
from .core import DEFAULT_PARAMS
from .gap_follower import coerce_scripted
from .line_follower import MAX_AGENTS as LINE_MAX_AGENTS, coerce_scripted_mixed, has_line_follower
from .mppi import split_scripted
from .opponents import split_mppi_opponents
from .particle_filter import split_filter
from .obs_encoder import ObsEncoder
from .reset_sampler import ResetSampler
from .param_sampler import ParamSampler
from .sim import Integrator, Simulator
from .track_preview import TrackPreview
from .neighbors import Neighbors
from .track import Track
from .centerline import coerce_params
from .trackgen import TrackMap
from .raceline import Raceline

try:  # pragma: no cover - gym is absent from the build image
    import gym as _gym
    _EnvBase = _gym.Env
except Exception:  # noqa: BLE001
    _EnvBase = object

_PKG_MAPS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "maps")


def _resolve_map_path(kwargs):
    """f110_env.py:108-120: named maps ship with the package, anything else is a path stem."""
    if 'map' not in kwargs:
        return 'vegas', os.path.join(_PKG_MAPS, 'vegas.yaml')
    name = kwargs['map']
    if name in ('berlin', 'skirk', 'levine', 'vegas', 'stata_basement'):
        return name, os.path.join(_PKG_MAPS, name + '.yaml')
    return name, name + '.yaml'


class _LapLogic(object):
    """The start/finish bookkeeping of F110Env._check_done (f110_env.py:204-246), vectorised
    over a leading env axis: arrays are [E][A]."""

    def __init__(self, num_envs, num_agents, ego_idx):
        self.E, self.A, self.ego = num_envs, num_agents, ego_idx
        self.start_xs = np.zeros((num_envs, num_agents))
        self.start_ys = np.zeros((num_envs, num_agents))
        self.start_thetas = np.zeros((num_envs, num_agents))
        self.rot_c = np.ones((num_envs,))
        self.rot_s = np.zeros((num_envs,))
        self.near_starts = np.ones((num_envs, num_agents), dtype=bool)
        self.toggle_list = np.zeros((num_envs, num_agents))
        self.lap_times = np.zeros((num_envs, num_agents))
        self.lap_counts = np.zeros((num_envs, num_agents))
        self.current_time = np.zeros((num_envs,))
        self._c0, self._s0, self._sx0, self._sy0 = 1.0, 0.0, [0.0] * num_agents, [0.0] * num_agents

    def reset(self, poses, env_mask=None):
        m = np.ones((self.E,), dtype=bool) if env_mask is None else np.asarray(env_mask, dtype=bool)
        poses = np.asarray(poses, dtype=np.float64).reshape(self.E, self.A, 3)
        self.current_time[m] = 0.0
        self.near_starts[m] = True
        self.toggle_list[m] = 0
        self.start_xs[m] = poses[m, :, 0]
        self.start_ys[m] = poses[m, :, 1]
        self.start_thetas[m] = poses[m, :, 2]
        th = -self.start_thetas[:, self.ego]
        self.rot_c[m] = np.cos(th)[m]
        self.rot_s[m] = np.sin(th)[m]
        # update_single's constants as plain floats (env 0): the single-env step counts microseconds
        self._c0, self._s0 = float(self.rot_c[0]), float(self.rot_s[0])
        self._sx0, self._sy0 = [float(v) for v in self.start_xs[0]], [float(v) for v in self.start_ys[0]]

    def update_single(self, poses_x, poses_y, collisions, timestep):
        """update() for ONE env in plain Python floats: the same IEEE operations in the same order, without ~25 NumPy
        calls on arrays of A elements (the single-env F110Env.step is latency-bound, every microsecond of host time
        counts).  returns done (bool), checkpoint_done [A]"""
        ct = float(self.current_time[0]) + timestep
        self.current_time[0] = ct
        c, s = self._c0, self._s0
        sx, sy = self._sx0, self._sy0
        near, tog = self.near_starts[0], self.toggle_list[0]
        all4 = True
        for i in range(self.A):
            px = float(poses_x[i]) - sx[i]
            py = float(poses_y[i]) - sy[i]
            dx = c * px + (-s) * py
            ty = s * px + c * py
            if ty > 2:
                ty = ty - 2
            elif ty < -2:
                ty = -2 - ty
            else:
                ty = 0.0
            closes = dx ** 2 + ty ** 2 <= 0.1
            if closes != bool(near[i]):
                near[i] = closes
                tog[i] += 1
            t = float(tog[i])
            self.lap_counts[0, i] = t // 2
            if t < 4:
                self.lap_times[0, i] = ct
                all4 = False
        done = bool(collisions[self.ego] != 0) or all4
        return done, tog >= 4

    def update(self, poses_x, poses_y, collisions, timestep):
        """returns done[E], checkpoint_done[E][A]"""
        left_t, right_t = 2, 2
        self.current_time = self.current_time + timestep
        px = np.asarray(poses_x, dtype=np.float64).reshape(self.E, self.A) - self.start_xs
        py = np.asarray(poses_y, dtype=np.float64).reshape(self.E, self.A) - self.start_ys
        c, s = self.rot_c[:, None], self.rot_s[:, None]
        dx = c * px + (-s) * py          # start_rot @ [px; py], f110_env.py:223,331
        temp_y = s * px + c * py
        idx1 = temp_y > left_t
        idx2 = temp_y < -right_t
        temp_y = np.where(idx1, temp_y - left_t, np.where(idx2, -right_t - temp_y, 0.0))
        dist2 = dx ** 2 + temp_y ** 2
        closes = dist2 <= 0.1
        entered = closes & ~self.near_starts
        left = ~closes & self.near_starts
        self.near_starts = np.where(entered, True, np.where(left, False, self.near_starts))
        self.toggle_list = self.toggle_list + (entered | left)
        self.lap_counts[...] = self.toggle_list // 2
        running = self.toggle_list < 4
        self.lap_times[...] = np.where(running, self.current_time[:, None], self.lap_times)
        col = np.asarray(collisions).reshape(self.E, self.A)
        done = (col[:, self.ego] != 0) | np.all(self.toggle_list >= 4, axis=1)
        return done, self.toggle_list >= 4


def _reward_mode(reward):
    if reward not in ('timestep', 'progress'):
        raise ValueError("reward must be 'timestep' (the reference's) or 'progress' (the ego's progress along the track)")
    return reward


def _is_centerline(track):
    """track='centerline': the slot's own centreline instead of a given line"""
    return isinstance(track, str) and track == 'centerline'


def _is_raceline(track):
    """track='raceline': the racing line and speed profile solved on the device from the slot's own line"""
    return isinstance(track, str) and track == 'raceline'


def _is_extracted(track):
    return _is_centerline(track) or _is_raceline(track)


def _raceline_source(batch, slot, track_map, centerline):
    """what track='raceline' solves on map slot `slot`: a carved slot's generating line with the half widths it was CARVED with
    (TrackMap.carved_line: per point the smaller of its two segments', whatever column the line itself carries), elsewhere the
    slot's extracted centreline"""
    if track_map is None:
        return batch.centerline(int(slot), **coerce_params(centerline))
    if not track_map.track.closed:
        raise ValueError("track='raceline' needs a closed line (slot %d was carved from an open one)" % int(slot))
    return track_map.carved_line()


# the track columns' observation keys -> their names in BatchSim.track_views / track_host_block
_TRACK_OBS = {key: src for src, key in Simulator.TRACK_KEYS}


# F110Env.render('rgb_array'): the reference window at its first draw — 1000 x 800 pixels, zoom 1.2 on the 50 px/m scene
# (rendering.py), centred on the map origin
RENDER_DEFAULTS = {"width": 1000, "height": 800, "view": "world", "m_per_px": 0.024, "center": (0.0, 0.0), "angle": 0.0,
                   "fwd_offset": 0.0, "layers": None, "car_size": None, "palette": None}


def _render_spec(base, spec):
    """base updated by spec, validated (ValueError); layers None = every layer that has data"""
    from . import render as R
    unknown = set(spec) - set(RENDER_DEFAULTS)
    if unknown:
        raise ValueError("unknown render option(s): %s" % ", ".join(sorted(unknown)))
    out = dict(base)
    out.update(spec)
    R.make_spec(**{k: v for k, v in out.items() if k not in ("palette", "layers")})
    if out["layers"] is not None:
        R.layer_bits(out["layers"])
    R.check_palette(out["palette"])
    return out


def _render_call(sim, agents, spec, rgb, device):
    layers = spec["layers"]
    if layers is None:
        layers = ("map", "scan", "cars") + (("track",) if getattr(sim.batch, "tracks", None) else ())
    kw = {k: v for k, v in spec.items() if k != "layers"}
    b = sim.batch
    return (b.render_device if device else b.render)(agents, layers=layers, rgb=rgb, **kw)


class F110Env(_EnvBase):
    metadata = {'render.modes': ['human', 'human_fast', 'rgb_array']}
    render_callbacks = []

    def __init__(self, **kwargs):
        self.seed = kwargs.get('seed', 12345)
        self.map_name, self.map_path = _resolve_map_path(kwargs)
        self.map_ext = kwargs.get('map_ext', '.png')
        self.params = kwargs.get('params', dict(DEFAULT_PARAMS))
        self.num_agents = kwargs.get('num_agents', 2)
        self.timestep = kwargs.get('timestep', 0.01)
        self.ego_idx = kwargs.get('ego_idx', 0)
        self.integrator = kwargs.get('integrator', Integrator.RK4)
        self.lidar_dist = kwargs.get('lidar_dist', 0.0)
        self.start_thresh = 0.5
        self.poses_x, self.poses_y, self.poses_theta = [], [], []
        self.collisions = np.zeros((self.num_agents,))
        self._lap = _LapLogic(1, self.num_agents, self.ego_idx)
        # f110_env.py:192 does NOT hand ego_idx to its Simulator: obs['ego_idx'] is 0 whatever the env's
        # ego_idx is (pinned by tests/golden/env_episode_2agents.npz); ego_idx only steers _check_done
        self.sim = Simulator(self.params, self.num_agents, self.seed, time_step=self.timestep,
                             integrator=self.integrator, lidar_dist=self.lidar_dist,
                             device_id=kwargs.get('device_id', 0),
                             map_layout=kwargs.get('map_layout', _ffi.MAP_DEFAULT))
        self.sim.set_map(self.map_path, self.map_ext)
        # a carved track: track_map= (a TrackMap, a Track or a dict of random_track's arguments) registers its corridor
        # as slot 1 and runs the env there, with its line as the track unless track= names another; `map` stays slot 0
        self.track_map, self.map_slot = None, 0
        if kwargs.get('track_map') is not None:
            self.track_map = TrackMap.coerce(kwargs['track_map'])
            self.map_slot = self.sim.batch.add_track_map(self.track_map)
            self.sim.batch.set_env_maps([self.map_slot])
        # track progress (no reference counterpart): track= adds the obs keys of Simulator.TRACK_KEYS; reward='progress' pays the
        # ego's progress of the step (metres along the track) instead of the reference's constant timestep
        self.reward_mode = _reward_mode(kwargs.get('reward', 'timestep'))
        self.track = None
        if kwargs.get('track') is not None:
            track = kwargs['track']
            if _is_centerline(track):   # the map's centreline loop, extracted on the device
                track = self.sim.batch.centerline(self.map_slot, **coerce_params(kwargs.get('centerline')))
            elif _is_raceline(track):   # ... or the racing line solved from it (from the carved line, on a carved slot)
                track = self.sim.batch.raceline(_raceline_source(self.sim.batch, self.map_slot, self.track_map, kwargs.get('centerline')),
                                                Raceline.coerce(kwargs.get('raceline')))
            self.track = self.sim.set_track(Track.coerce(track), self.map_slot)
            self.sim.enable_track()
        elif self.track_map is not None:
            self.track = self.track_map.track
            self.sim.enable_track()
        elif self.reward_mode == 'progress':
            raise ValueError("reward='progress' needs a track (track=...)")
        # track preview: track_preview= adds obs['track_preview'], float32 [A][P][D], computed on the device after the step
        self.track_preview = None
        if kwargs.get('track_preview') is not None:
            self.track_preview = TrackPreview.coerce(kwargs['track_preview'])
            if self.track is None:
                raise ValueError("track_preview= needs a track (track=...)")
            self.track_preview.check_track(self.track)
        # neighbours: neighbors= adds obs['neighbors'], float32 [A][K][D], computed on the device after the step
        self.neighbors = None
        if kwargs.get('neighbors') is not None:
            self.neighbors = Neighbors.coerce(kwargs['neighbors'])
            if self.neighbors.needs_track and self.track is None:
                raise ValueError("neighbors= with 'gap_s' needs a track (track=...)")
        # static obstacles: obstacles= puts the env on a slot derived from slot 0 with the shapes stamped in
        self.obstacle_slot = None
        if kwargs.get('obstacles') is not None:
            self.obstacle_slot = self.sim.batch.add_obstacle_map(kwargs['obstacles'], self.map_slot)
            self.sim.batch.set_env_maps([self.obstacle_slot])
        # randomised start poses: random_start= (a ResetSampler or a dict of its settings) makes reset() without
        # poses draw them on the track
        self.random_start = None
        if kwargs.get('random_start') is not None:
            self.random_start = self.sim.batch.set_reset_sampler(ResetSampler.coerce(kwargs['random_start']))
        # randomised vehicle parameters: random_params= (a ParamSampler or a dict of its settings) makes every reset()
        # draw the cars' parameter rows on the device, in front of the reset
        self.random_params = _arm_random_params(self.sim.batch, kwargs.get('random_params'), 0)
        self.render_obs = None
        self.current_obs = None
        self._render_view = dict(RENDER_DEFAULTS)

    # attributes user code reads off the reference env
    lap_times = property(lambda self: self._lap.lap_times[0])
    lap_counts = property(lambda self: self._lap.lap_counts[0])
    current_time = property(lambda self: float(self._lap.current_time[0]))
    toggle_list = property(lambda self: self._lap.toggle_list[0])
    near_starts = property(lambda self: self._lap.near_starts[0])
    start_xs = property(lambda self: self._lap.start_xs[0])
    start_ys = property(lambda self: self._lap.start_ys[0])
    start_thetas = property(lambda self: self._lap.start_thetas[0])

    def step(self, action):
        obs = self.sim.step(action)
        if self.track_preview is not None:
            pv = self.sim.batch.track_preview_device(self.track_preview)
            obs['track_preview'] = pv.download()
            pv.free()
        if self.neighbors is not None:
            nb = self.sim.batch.neighbors_device(self.neighbors)
            obs['neighbors'] = nb.download()
            nb.free()
        obs['lap_times'] = self._lap.lap_times[0]
        obs['lap_counts'] = self._lap.lap_counts[0]
        self.current_obs = obs
        self.render_obs = {k: obs[k] for k in ('ego_idx', 'poses_x', 'poses_y', 'poses_theta', 'lap_times', 'lap_counts')}
        reward = self.timestep if self.reward_mode == 'timestep' else float(obs['progress_delta'][self.ego_idx])
        self.poses_x, self.poses_y, self.poses_theta = obs['poses_x'], obs['poses_y'], obs['poses_theta']
        self.collisions = obs['collisions']
        done, toggles = self._lap.update_single(obs['poses_x'], obs['poses_y'], obs['collisions'], self.timestep)
        info = {'checkpoint_done': toggles}
        self._last = (obs, reward, done, info)
        return obs, reward, done, info

    def snapshot(self):
        """an exact copy of the env: simulator state (device blob), lap bookkeeping and the last (obs, reward, done, info)"""
        return {"sim": self.sim.snapshot(), "host": copy.deepcopy((self._lap, self.poses_x, self.poses_y, self.poses_theta,
                                                                    self.collisions, self.current_obs, self.render_obs,
                                                                    getattr(self, "_last", None)))}

    def restore(self, snap):
        """back to a snapshot(); returns the (obs, reward, done, info) of the step before it"""
        self.sim.restore(snap["sim"])
        (self._lap, self.poses_x, self.poses_y, self.poses_theta, self.collisions, self.current_obs, self.render_obs,
         self._last) = copy.deepcopy(snap["host"])
        return copy.deepcopy(self._last)

    def reset(self, poses=None):
        """poses None (random_start only): the start poses are drawn on the track"""
        self.collisions = np.zeros((self.num_agents,))
        if self.random_params is not None:
            self.sim.batch.sample_params()
        if poses is None:
            if self.random_start is None:
                raise ValueError("reset() without poses needs random_start=")
            self.sim.batch.sample_reset()
            self.sim._steps_since_full_reset = 0
            poses = self.sim.batch.reset_sampler_poses()
        else:
            poses = np.asarray(poses, dtype=np.float64)
            self.sim.reset(poses)           # raises ValueError on a pose-count mismatch
        self._lap.reset(poses)
        action = np.zeros((self.num_agents, 2))
        return self.step(action)            # f110_env.py:337-338: reset advances one step

    def update_map(self, map_path, map_ext):
        """(an env made with obstacles= goes back to the plain map: call set_obstacles again to stamp them into the new one)"""
        self.sim.set_map(map_path, map_ext)
        self.obstacle_slot = None

    def set_obstacles(self, obstacles):
        """stamp another Obstacles into this env's map (in place when the env already runs on a derived slot)"""
        if self.obstacle_slot is None:
            self.obstacle_slot = self.sim.batch.add_obstacle_map(obstacles, self.map_slot)
            self.sim.batch.set_env_maps([self.obstacle_slot])
        else:
            self.sim.batch.set_obstacles(self.obstacle_slot, obstacles)

    def update_params(self, params, index=-1):
        _params_owner_check(self)
        self.sim.update_params(params, agent_idx=index)

    def get_params(self):
        """[A][18] float64: the cars' live parameter rows (random_params, or a per-agent set)"""
        return self.sim.batch.get_params()

    def params_view(self):
        """the live rows as a DeviceArray (BatchSim.params_view)"""
        return self.sim.batch.params_view()

    def add_render_callback(self, callback_func):
        F110Env.render_callbacks.append(callback_func)

    def set_render_view(self, **spec):
        """change what render('rgb_array') draws: width, height, view ('world' / 'follow' / 'ego'), m_per_px, center, angle,
        fwd_offset, layers (None: every layer that has data), car_size, palette"""
        self._render_view = _render_spec(self._render_view, spec)

    def render(self, mode='human'):
        """mode='rgb_array': uint8 [H][W][3] of the last observation, drawn on the device with the ego as SELF"""
        assert mode in self.metadata['render.modes']
        if mode != 'rgb_array':
            raise NotImplementedError("the pyglet window is outside this build's scope; use render('rgb_array') for frames")
        return _render_call(self.sim, [int(self.ego_idx)], self._render_view, True, False)[1][0]


def _arm_random_params(batch, spec, env_base):
    """random_params= of the env classes: None, or the ParamSampler armed on `batch` """
    if spec is None:
        return None
    return batch.set_param_sampler(ParamSampler.coerce(spec), env_base=env_base)


def _params_owner_check(env):
    if env.random_params is not None:
        raise RuntimeError("random_params= is armed and owns the parameter rows: update_params / update_params_batch are refused")


class F110VecEnv(object):
    """E independent F110 environments stepped by one device launch sequence.

    reset(poses[E][A][3], env_mask=None) / step(actions[E][A][2]) -> (obs, reward, done[E], info)
    with array observations (leading env axis).

    Resets.  reset(poses) of every env is the reference's reset(): re-seat + one zero-action step,
    whose observation is returned (f110_env.py:337-338).  A PARTIAL reset — reset(poses, env_mask)
    or `auto_reset=True`, which re-seats finished envs at their start poses inside step() (mask
    reset in place) — only re-seats: nobody is stepped, the envs that are in the middle
    of an episode are not disturbed, and a re-seated env's first observation arrives with the next
    step().  reset(poses, env_mask) therefore returns the previous step's tuple with `done`
    cleared for the re-seated envs.

    device_logic=True runs the lap / done bookkeeping (F110Env._check_done) and the auto-reset on
    the GPU: a step is ONE ABI call (f110_step_host) — the step's kernels read the actions in place
    from a page-locked buffer (`mapped_actions`; False: a staging copy first) and one kernel writes
    `done`, the lap arrays and the requested observation columns straight into page-locked host
    memory (scans: one DMA copy).  The arrays step() returns in that mode are VIEWS of that block,
    the same objects every step, overwritten by the next step(): copy what you keep, or pass
    copy_obs=True (the block stays valid as long as any array views it, also after close()).
    obs_fields selects the fields put into `obs` ('scans' is 8.6 KB per agent); episode_fields
    the episode columns brought back next to `done` (default: lap_times, lap_counts in obs and
    toggle_list, near_starts, checkpoint_done in info; () for the leanest loop); everything stays
    available in HBM through `device_views()`.  `env.action_buffer` ([E][A][2], page-locked) can be
    filled in place and step(None) called: no copy of the actions at all.  step_async() /
    step_wait() split the call the way gym.vector.VectorEnv does (between the two, `action_buffer` belongs to the
    GPU: the kernels read it in place — write the next actions only after step_wait()).

    Domain randomisation over tracks: `extra_maps=[(yaml_path, ext), ...]` registers further maps
    (slots 1, 2, ...; `map` is slot 0) and `env_map=[slot per env]` assigns them; `set_env_maps()`
    re-assigns later.

    Static obstacles (no reference counterpart): `obstacle_maps=[Obstacles | (base_slot, Obstacles), ...]` registers
    map slots derived from slot 0 (or base_slot) with the shapes stamped into their distance tables on the device; they are numbered
    after `extra_maps` and usable in `env_map`, and carry their base's track.  `set_obstacles(slot, obstacles)` re-draws one in
    place between episodes.  Obstacles belong to a slot, not to an env: one padded table of device memory per slot.

    Carved tracks (no reference counterpart): `track_maps=[TrackMap | Track | dict(random_track arguments), ...]` registers
    base map slots whose distance tables are corridors carved around a line on the device, numbered after `extra_maps` and before
    `obstacle_maps` (which may derive from them); each line is its slot's track unless `tracks=` names another.
    `set_track_map(slot, tm)` re-carves one in place between episodes, in the same frame.

    Track progress (no reference counterpart): `track=` (a Track, an [M][2] array or a csv path) puts a raceline on
    slot 0, `tracks={slot: track}` one per map slot.  The observation then also carries progress, progress_delta,
    lateral_offset, heading_error and track_segment ([E][A] each; obs_fields selects among them too — by default all of them), and
    reward='progress' makes the reward the ego's progress_delta, [E].  A track given as the string 'centerline' is the slot's own
    centreline loop, extracted from its distance table on the device (a derived obstacle slot: the line around its
    obstacles); `centerline=dict(seed=…, heading=…, spacing=…, smooth=…, max_passes=…)` sets BatchSim.centerline's parameters.
    The string 'raceline' is the racing line with a speed profile solved on the device from the carved line and its half
    widths on a slot of `track_maps`, from the extracted centreline elsewhere; `raceline=dict(spacing=…, levels=…, iters=…, margin=…,
    v_max=…, a_lat=…, a_accel=…, a_brake=…)` sets it.  The slot's track then carries the attribute columns kappa, vx and offset
    (the preview's attr0 .. attr2), and `set_track_map` on such a slot solves the new line's.

    Compact observations (no reference counterpart): `obs_encoder=` (an ObsEncoder or a dict of its settings) adds
    obs['encoded'], float32 [E][A][F][D]: pooled lidar sectors and scaled state / track columns, the last F frames stacked
    (newest last, refilled when an env starts an episode).  It is encoded on the device behind the step and lands in page-locked
    memory with the rest of the block, so it needs device_logic=True (ValueError otherwise; a host-logic loop calls
    env.sim.batch.encode_obs(enc) after its step instead).  The array is a persistent view like the others, overwritten by every
    step() / reset().  'encoded' is also an obs_fields entry (present by default with an encoder); an encoder's track features
    need a track.  The frame stack lives in device memory of this env (`encoded_stack`, a DeviceArray [E*A][F][D] for
    device-resident consumers) and is part of snapshot() / restore().

    Scripted cars (no reference counterpart): `scripted={slot: GapFollower | dict}` lets every env's car `slot`
    drive itself with a follow-the-gap controller that runs on the device on the last step's scans; `scripted=(assign,
    [controllers])` assigns per agent (assign int32 [E][A]: -1 = the caller's action, else an index into controllers).
    step(actions) keeps its [E][A][2] shape: the rows of scripted cars are ignored and replaced on the device.  A scripted
    car takes the zero action on the first step of an episode (reset()'s own step, and the step after an in-step re-seat).
    It needs device_logic=True (ValueError otherwise).  Controllers hold no state: snapshots do not change.
    An entry may also be a LineFollower: that car drives the line of its env's map slot — pure pursuit on the track,
    the speed from a track attribute (the raceline's vx with track='raceline'), slower behind a car ahead — from the track columns
    of the last step.  It needs track= / tracks= (ValueError otherwise).  The list of the (assign, [controllers]) form may mix
    the two controller classes, assign indexing the list; a dict in it is a GapFollower's settings.
    An entry may instead be an Mppi, at most one per env object: every env's car `slot` then plans on the device from its
    live state, behind the controllers, with the stream PCG64(SeedSequence(seed, spawn_key=(global agent index,))) of the env's
    `seed`.  `planner=(slot, Mppi)` says the same next to the (assign, [controllers]) form.  The planner's nominal sequences and
    stream positions are not part of snapshot() / restore(): keep env.sim.batch.get_mppi_state() next to a snapshot.
    `mppi_opponents=dict(opponents=Opponents | dict, w_hit=..., w_near=..., near_ref=...)` lets that planner see the
    other cars of its env: each is predicted over the horizon from its live state and every candidate pays for coming within the
    radius of a prediction (w_hit per action from there on) and for its smallest distance below near_ref (w_near per metre).  It
    holds no state.

    Track preview (no reference counterpart): `track_preview=` (a TrackPreview or a dict of its settings) adds
    obs['track_preview'], float32 [E][A][P][D]: P stations of the raceline ahead of each car, in its own frame or the map's,
    with the track's interpolated attributes (Track(attrs=...)).  It belongs to the observation it comes with (that step's
    poses and progress), is computed on the device behind the step and lands in page-locked memory with the rest of the
    block, so it needs device_logic=True and a track (ValueError otherwise; any other loop calls
    env.sim.batch.track_preview_device after its step).  A persistent view like the others; it holds no state.

    Neighbours (no reference counterpart): `neighbors=` (a Neighbors or a dict of its settings) adds
    obs['neighbors'], float32 [E][A][K][D]: each car's K nearest opponents of its own env in its own frame (position, distance,
    relative heading and velocity, gap along the track, validity, index).  It belongs to the observation it comes with, is
    computed on the device behind the step and lands in page-locked memory, so it needs device_logic=True, and a track only
    for 'gap_s' (ValueError otherwise; any other loop calls env.sim.batch.neighbors_device after its step).  It holds no state.

    Localisation (no reference counterpart): `particle_filter={slot: ParticleFilter | dict}` arms a particle filter on
    every env's car `slot` and runs it on the device behind each step: obs['pose_estimate'], float64 [E][A][3], is the estimate
    (x, y, theta) from the car's own scan and the pose's move since the last step, obs['pf_info'], float32 [E][A][4], is
    particle_filter.INFO; the rows of the other cars are NaN.  A car's cloud is drawn afresh around its start pose when its env is
    reset or re-seated.  Needs device_logic=True.  The clouds and stream positions are not part of snapshot() / restore(): keep
    env.sim.batch.get_pf_state() next to a snapshot.  The device copies (env.pose_estimate_buffer, env.pf_info_buffer) feed a
    device-side loop without a host wait (examples/particle_filter.py).
    """

    # every key of the reference's observation (base_classes.py:594-610, docs/api/obv.rst:6-14)
    _ALL = ("scans", "poses_x", "poses_y", "poses_theta", "linear_vels_x", "linear_vels_y", "ang_vels_z", "collisions")
    _TRACK = tuple(key for _, key in Simulator.TRACK_KEYS)

    # what the device episode logic can bring back next to `done` (info keys + the two lap arrays of obs)
    _EPISODE = ("lap_times", "lap_counts", "toggle_list", "near_starts", "checkpoint_done")

    def __init__(self, num_envs, auto_reset=False, device_logic=False, obs_fields=None, copy_obs=False,
                 episode_fields=None, mapped_actions=True, spin_wait=False, fuse_host_block=True, poll_wait=True, obs_encoder=None, scripted=None,
                 track_preview=None, neighbors=None, particle_filter=None, mppi_opponents=None, **kwargs):
        self.num_envs = int(num_envs)
        self.seed = kwargs.get('seed', 12345)
        self.map_name, self.map_path = _resolve_map_path(kwargs)
        self.map_ext = kwargs.get('map_ext', '.png')
        self.params = kwargs.get('params', dict(DEFAULT_PARAMS))
        self.num_agents = kwargs.get('num_agents', 2)
        self.timestep = kwargs.get('timestep', 0.01)
        self.ego_idx = kwargs.get('ego_idx', 0)
        self.auto_reset = auto_reset
        self.device_logic = bool(device_logic)
        tracks = dict(kwargs.get('tracks') or {})
        if kwargs.get('track') is not None:
            tracks[0] = kwargs['track']
        self.raceline = Raceline.coerce(kwargs.get('raceline'))
        # carved tracks: slots behind extra_maps, each with its generating line as the track (a tracks= entry wins)
        track_maps = [TrackMap.coerce(item) for item in kwargs.get('track_maps') or ()]
        for i, tm in enumerate(track_maps):
            tracks.setdefault(1 + len(kwargs.get('extra_maps', ())) + i, tm.track)
        self.reward_mode = _reward_mode(kwargs.get('reward', 'timestep'))
        if self.reward_mode == 'progress' and not tracks:
            raise ValueError("reward='progress' needs a track (track= or tracks=)")
        self.obs_encoder = None if obs_encoder is None else ObsEncoder.coerce(obs_encoder)
        self.obs_fields = tuple((self._ALL + (self._TRACK if tracks else ()) + (("encoded",) if self.obs_encoder is not None else ()))
                                if obs_fields is None else obs_fields)
        if "encoded" in self.obs_fields and self.obs_encoder is None:
            raise ValueError("the obs_fields entry 'encoded' needs obs_encoder=")
        if self.obs_encoder is not None:
            if not self.device_logic:
                raise ValueError("obs_encoder= needs device_logic=True (a host-logic loop calls env.sim.batch.encode_obs(enc) after its step)")
            if self.obs_encoder.needs_track and not tracks:
                raise ValueError("the encoder's track features need a track (track= or tracks=)")
            self.obs_encoder.check_beams(kwargs.get('num_beams', 1080))
        self._encode = self.obs_encoder is not None and "encoded" in self.obs_fields
        self.scripted = None
        self.planner = None   # (slot, Mppi): every env's car `slot` plans
        scripted, planner = split_scripted(scripted, kwargs.get('planner'))
        if scripted is not None or planner is not None:
            if not self.device_logic:
                raise ValueError("scripted= needs device_logic=True (any other loop arms env.sim.batch.set_controllers / set_mppi and calls "
                                 "BatchSim.follow_gap_device / mppi_device on its device action buffer)")
        self.line_followers = None   # (assign [E][A], [LineFollower]): the scripted cars that drive their slot's line
        if scripted is not None and has_line_follower(scripted):
            self.scripted, self.line_followers = coerce_scripted_mixed(scripted, self.num_envs, self.num_agents)
        elif scripted is not None:
            self.scripted = coerce_scripted(scripted, self.num_envs, self.num_agents)
        if self.scripted is not None:
            for c in self.scripted[1]:
                c.window(kwargs.get('num_beams', 1080))
        if self.line_followers is not None:
            if not tracks:
                raise ValueError("a LineFollower needs a track on its envs' map slots (track= or tracks=)")
            if self.num_agents > LINE_MAX_AGENTS and any(c.follow_range > 0.0 for c in self.line_followers[1]):
                raise ValueError("a LineFollower with follow_range > 0 serves at most %d cars per env" % LINE_MAX_AGENTS)
        if planner is not None:
            slot, mp = planner
            if not (0 <= slot < self.num_agents):
                raise ValueError("scripted: slot %r is not one of the %d cars of an env" % (slot, self.num_agents))
            if self.scripted is not None and np.any(self.scripted[0][:, slot] != -1):
                raise ValueError("scripted: car %d has both a follow-the-gap controller and the planner" % slot)
            if self.line_followers is not None and np.any(self.line_followers[0][:, slot] != -1):
                raise ValueError("scripted: car %d has both a line follower and the planner" % slot)
            if mp.needs_track and not tracks:
                raise ValueError("the planner's w_progress and w_lat need a track (track= or tracks=)")
            self.planner = (slot, mp)
        self.mppi_opponents = split_mppi_opponents(mppi_opponents)   # (Opponents, w_hit, w_near, near_ref): the planner sees the env's other cars
        if self.mppi_opponents is not None:
            if self.planner is None:
                raise ValueError("mppi_opponents= needs a planner (scripted={slot: Mppi(...)})")
            if self.mppi_opponents[0].needs_track and not tracks:
                raise ValueError("mppi_opponents in 'track' mode needs a track (track= or tracks=)")
        self.track_preview = None
        if track_preview is not None:
            self.track_preview = TrackPreview.coerce(track_preview)
            if not self.device_logic:
                raise ValueError("track_preview= needs device_logic=True (any other loop calls env.sim.batch.track_preview_device after its step)")
            if not tracks:
                raise ValueError("track_preview= needs a track (track= or tracks=)")
            tracks = {slot: t if _is_extracted(t) else Track.coerce(t) for slot, t in tracks.items()}
            for t in tracks.values():
                if not _is_extracted(t):   # (a centreline or a raceline is checked once it has been made, below)
                    self.track_preview.check_track(t)
        self.neighbors = None
        if neighbors is not None:
            self.neighbors = Neighbors.coerce(neighbors)
            if not self.device_logic:
                raise ValueError("neighbors= needs device_logic=True (any other loop calls env.sim.batch.neighbors_device after its step)")
            if self.neighbors.needs_track and not tracks:
                raise ValueError("neighbors= with 'gap_s' needs a track (track= or tracks=)")
        self.particle_filter = split_filter(particle_filter)   # (slot, ParticleFilter): every env's car `slot` localises
        if self.particle_filter is not None:
            if not self.device_logic:
                raise ValueError("particle_filter= needs device_logic=True (any other loop arms env.sim.batch.set_particle_filter and calls "
                                 "BatchSim.localize_device after its step)")
            if not (0 <= self.particle_filter[0] < self.num_agents):
                raise ValueError("particle_filter: slot %r is not one of the %d cars of an env" % (self.particle_filter[0], self.num_agents))
            self.particle_filter[1].check_beams(kwargs.get('num_beams', 1080))
        self.encoded_stack = None
        if not tracks and any(f in self._TRACK for f in self.obs_fields):
            raise ValueError("the track fields of obs_fields need a track (track= or tracks=)")
        self._lap = _LapLogic(self.num_envs, self.num_agents, self.ego_idx)
        self.sim = Simulator(self.params, self.num_agents, self.seed, time_step=self.timestep,
                             integrator=kwargs.get('integrator', Integrator.RK4),   # (no ego_idx: see obs['ego_idx'] below)
                             lidar_dist=kwargs.get('lidar_dist', 0.0), num_envs=self.num_envs,
                             num_beams=kwargs.get('num_beams', 1080), fov=kwargs.get('fov', 4.7),
                             scan_noise_std=kwargs.get('scan_noise_std', 0.01),
                             device_id=kwargs.get('device_id', 0),
                             map_layout=kwargs.get('map_layout', _ffi.MAP_DEFAULT), batched=True,
                             noise_mode=kwargs.get('noise_mode', 'device'), step_groups=kwargs.get('step_groups', 0))
        self.sim.set_map(self.map_path, self.map_ext)
        self._last = None
        self.map_slots = [(self.map_path, self.map_ext)]
        for path, ext in kwargs.get('extra_maps', ()):
            self.sim.batch.add_map(path, ext)
            self.map_slots.append((path, ext))
        # carved tracks: each registers a base slot whose table is the corridor of its line, carved on the device
        self.track_maps = {}
        for tm in track_maps:
            self.track_maps[self.sim.batch.add_track_map(tm)] = tm
            self.map_slots.append(tm)
        # track='centerline' (DESIGN §6n): the slot's centreline loop, extracted from its distance table on the device
        self.centerline = kwargs.get('centerline')
        # track='raceline' (DESIGN §6p): the racing line and speed profile solved from the slot's line, on the device
        self.raceline_slots = set()
        self._extract_centerlines(tracks)
        # static obstacles: each entry registers a slot derived from slot 0 (or from the entry's base slot)
        self.obstacle_slots = {}
        for item in kwargs.get('obstacle_maps', ()):
            base, ob = (int(item[0]), item[1]) if isinstance(item, tuple) and len(item) == 2 and isinstance(item[0], (int, np.integer)) else (0, item)
            slot = self.sim.batch.add_obstacle_map(ob, base)
            self.map_slots.append(self.map_slots[base])
            self.obstacle_slots[slot] = base
            if base in tracks and slot not in tracks:   # the same raceline (one Track object) on the derived slot
                tracks[base] = tracks[slot] = Track.coerce(tracks[base])
        self._extract_centerlines(tracks)   # (those of derived slots: the line around the obstacles)
        if kwargs.get('env_map') is not None:
            self.set_env_maps(kwargs['env_map'])
        self.tracks = {int(slot): self.sim.set_track(Track.coerce(t), int(slot)) for slot, t in sorted(tracks.items())}
        if self.tracks:
            self.sim.enable_track()
        # randomised start poses: reset() without poses and every auto re-seat draw them on the env's track;
        # env_base = this handle's first global env index (ShardedVecEnv)
        self.random_start = None
        if kwargs.get('random_start') is not None:
            self.random_start = self.sim.batch.set_reset_sampler(ResetSampler.coerce(kwargs['random_start']),
                                                                 env_base=int(kwargs.get('env_base', 0)))
        # randomised vehicle parameters: reset() draws the masked envs' rows in front of the reset, every auto
        # re-seat draws in the step; the same env_base rule
        self.random_params = _arm_random_params(self.sim.batch, kwargs.get('random_params'), int(kwargs.get('env_base', 0)))
        self._start_poses = None
        self._d_actions = None
        self.copy_obs = bool(copy_obs)
        self.episode_fields = tuple(self._EPISODE if episode_fields is None else episode_fields)
        self.mapped_actions = bool(mapped_actions)
        self.spin_wait = bool(spin_wait)
        self.fuse_host_block = bool(fuse_host_block)
        self.poll_wait = bool(poll_wait)
        if self.device_logic:
            b = self.sim.batch
            b.episode_init(self.ego_idx)
            self._d_actions = b.device_array((self.num_envs * self.num_agents, 2))
            self._build_host_block()
            if self.scripted is not None:
                b.set_controllers(*self.scripted)
            if self.line_followers is not None:
                b.set_line_followers(*self.line_followers)
            if self.planner is not None:   # agent_base: this handle's first global agent (ShardedVecEnv), so a sharded run draws the same numbers
                b.set_mppi(self.planner[1], np.arange(self.num_envs) * self.num_agents + self.planner[0], seed=self.seed,
                           agent_base=int(kwargs.get('env_base', 0)) * self.num_agents)
                if self.mppi_opponents is not None:
                    b.set_mppi_opponents(*self.mppi_opponents)
            if self.particle_filter is not None:   # likewise the filter's streams
                b.set_particle_filter(self.particle_filter[1], np.arange(self.num_envs) * self.num_agents + self.particle_filter[0], seed=self.seed,
                                      agent_base=int(kwargs.get('env_base', 0)) * self.num_agents)

    def _build_host_block(self):
        """the page-locked block f110_step_host fills, and the (obs, reward, done, info) tuple of views into it
        that step() hands out — built once: a step is one ABI call, no per-step allocation"""
        E, A, b = self.num_envs, self.num_agents, self.sim.batch
        want = ["done"]
        st_fields = {"poses_x": 0, "poses_y": 1, "poses_theta": 4, "linear_vels_x": 3, "ang_vels_z": 5}
        if any(f in st_fields for f in self.obs_fields):
            want.append("state")
        want += [f for f in ("collisions", "scans") if f in self.obs_fields]
        ep_names = {"lap_times": "lap_times", "lap_counts": "lap_counts", "toggle_list": "toggles",
                    "near_starts": "near_starts", "checkpoint_done": "checkpoint_done"}
        for f in self.episode_fields:
            want.append(ep_names[f])      # KeyError: not an episode field
        hb = self._hb = b.host_block(want)
        v = hb.views
        self.action_buffer = hb.actions.reshape(E, A, 2)   # write actions here and call step(None): no copy at all
        # obs['ego_idx'] is 0 whatever the env's ego_idx is: the reference env never hands ego_idx to its Simulator
        # (f110_env.py:192) — the same quirk F110Env reproduces; ego_idx steers the done rule only
        obs = {'ego_idx': 0}
        for f in self.obs_fields:
            if f in st_fields:
                obs[f] = v["state"][st_fields[f]].reshape(E, A)
            elif f == "linear_vels_y":
                obs[f] = np.zeros((E, A))      # base_classes.py:603: always 0. in the reference
            elif f == "scans":
                obs[f] = v["scans"].reshape(E, A, -1)
            elif f in _TRACK_OBS or f == "encoded":
                continue                       # (the track block and the encoder's block, below)
            else:
                obs[f] = v[f].reshape(E, A)
        info = {}
        for f in self.episode_fields:
            arr = v[ep_names[f]].reshape(E, A)
            if f in ("near_starts", "checkpoint_done"):
                arr = arr.view(np.bool_)
            (obs if f in ("lap_times", "lap_counts") else info)[f] = arr
        reward = self.timestep
        if self.tracks:   # the track columns: page-locked views step_host fills next to the block
            tv = b.track_host_block()
            for f in self.obs_fields:
                if f in _TRACK_OBS:
                    obs[f] = tv[_TRACK_OBS[f]].reshape(E, A)
            if self.reward_mode == 'progress':
                reward = tv["ds"].reshape(E, A)[:, self.ego_idx]
        if self._encode:   # the frame stack in device memory, and the page-locked copy every step's encode ends with
            shape = self.obs_encoder.shape(E * A)
            self.encoded_stack = b.device_array(shape, np.float32)
            self._enc_pinned = b.pinned_empty(shape, np.float32)
            self._enc_pinned[...] = 0.0
            self._enc_fill = True          # the first encode, and the one after a restore without a saved stack
            obs["encoded"] = self._enc_pinned.reshape((E, A) + shape[1:])
        if self.track_preview is not None:   # the preview in device memory, and the page-locked copy every step's call ends with
            shape = self.track_preview.shape(E * A)
            self.preview_buffer = b.device_array(shape, np.float32)
            self._prv_pinned = b.pinned_empty(shape, np.float32)
            self._prv_pinned[...] = 0.0
            obs["track_preview"] = self._prv_pinned.reshape((E, A) + shape[1:])
        if self.neighbors is not None:       # likewise the neighbours
            shape = self.neighbors.shape(E * A)
            self.neighbors_buffer = b.device_array(shape, np.float32)
            self._nbr_pinned = b.pinned_empty(shape, np.float32)
            self._nbr_pinned[...] = 0.0
            obs["neighbors"] = self._nbr_pinned.reshape((E, A) + shape[1:])
        if self.particle_filter is not None:   # the estimates in device memory (NaN in the rows of cars that are not armed, written once
            # here) and the host arrays every step's collect refills
            self.pose_estimate_buffer = b.device_array((E * A, 3), np.float64)
            self.pf_info_buffer = b.device_array((E * A, 4), np.float32)
            self.pose_estimate_buffer.upload(np.full((E * A, 3), np.nan))
            self.pf_info_buffer.upload(np.full((E * A, 4), np.nan, dtype=np.float32))
            obs["pose_estimate"] = np.full((E, A, 3), np.nan)
            obs["pf_info"] = np.full((E, A, 4), np.nan, dtype=np.float32)
        self._ret_views = (obs, reward, v["done"].view(np.bool_), info)

    def update_params_batch(self, params):
        """a vehicle parameter set per agent of every env ([E*A] dicts or [E*A][18] array; None: back
        to the per-slot sets of update_params)"""
        _params_owner_check(self)
        self.sim.batch.set_params_batch(params)

    def update_params(self, params, index=-1):
        _params_owner_check(self)
        self.sim.update_params(params, agent_idx=index)

    def get_params(self):
        """[E * A][18] float64: the live per-agent parameter rows (random_params, or update_params_batch)"""
        return self.sim.batch.get_params()

    def params_view(self):
        """the live rows as a DeviceArray (BatchSim.params_view): privileged input for a policy or critic, no copy"""
        return self.sim.batch.params_view()

    def _extract_centerlines(self, tracks):
        """replace the 'centerline' and 'raceline' entries of `tracks` whose slot is registered by the slot's extracted centreline or by
        the raceline solved from the slot's line"""
        b = self.sim.batch
        for slot, t in sorted(tracks.items()):
            if not (_is_extracted(t) and 0 <= int(slot) < len(self.map_slots)):
                continue
            if _is_centerline(t):
                tracks[slot] = b.centerline(int(slot), **coerce_params(self.centerline))
            else:
                tracks[slot] = b.raceline(_raceline_source(b, slot, self.track_maps.get(int(slot)), self.centerline), self.raceline)
                self.raceline_slots.add(int(slot))
            if self.track_preview is not None:
                self.track_preview.check_track(tracks[slot])

    def set_env_maps(self, env_map):
        """env_map [num_envs]: which registered track each env runs on (None: all on slot 0)"""
        self.sim.batch.set_env_maps(env_map)
        self.env_map = None if env_map is None else np.asarray(env_map, dtype=np.int32).copy()

    def set_obstacles(self, slot, obstacles):
        """re-stamp the derived slot `slot` (one of obstacle_maps=) with another Obstacles, in place: it applies from the next step
        on, behind whatever step is in flight"""
        self.sim.batch.set_obstacles(slot, obstacles)

    def set_track_map(self, slot, tm):
        """re-carve the slot `slot` (one of track_maps=) with another TrackMap of the same frame, in place, and make its line the
        slot's track: it applies from the next step on, behind whatever step is in flight.  Reset the slot's envs afterwards."""
        tm = TrackMap.coerce(tm)
        self.sim.batch.set_track_map(slot, tm)
        self.track_maps[int(slot)] = tm
        if int(slot) in self.raceline_slots:   # tracks={slot: 'raceline'}: the new line's raceline, not the line itself
            self.tracks[int(slot)] = self.sim.set_track(self.sim.batch.raceline(_raceline_source(self.sim.batch, slot, tm, self.centerline), self.raceline), int(slot))
        elif int(slot) in self.tracks:
            self.tracks[int(slot)] = tm.track

    def device_views(self):
        v = self.sim.batch.device_views()
        if self.device_logic:
            v.update(self.sim.batch.episode_device_views())
        return v

    def _ego_agents(self, env_idx):
        e = np.arange(self.num_envs) if env_idx is None else np.asarray(env_idx, dtype=np.int64).reshape(-1)
        if e.size < 1 or np.any(e < 0) or np.any(e >= self.num_envs):
            raise ValueError("env indices must be a non-empty list in [0, %d)" % self.num_envs)
        return e * self.num_agents + int(self.ego_idx)

    def render(self, env_idx=None, **spec):
        """host RGB frames uint8 [n][H][W][3] of envs env_idx (None: all), each env's ego the camera agent; spec as
        F110Env.set_render_view (defaults: F110Env.render's window)"""
        sp = _render_spec(RENDER_DEFAULTS, spec)
        return _render_call(self.sim, self._ego_agents(env_idx), sp, True, False)[1]

    def render_device(self, agents=None, **spec):
        """BatchSim.render_device on this env's simulator: class crops (and RGB with rgb=True) as DLPack-exportable
        DeviceArrays, one frame per agent of `agents` (global indices env * num_agents + agent; None: every agent)"""
        return self.sim.batch.render_device(agents, **spec)

    def reset(self, poses=None, env_mask=None, reseat_only=False):
        """env_mask None: every env, then one zero-action step (f110_env.py:319-334).  A partial mask re-seats the masked envs
        only and returns the last step's tuple with their done cleared.  reseat_only=True takes that path even when env_mask
        covers every env (ShardedVecEnv: a shard's slice of a partial global mask may).  poses None (random_start only): the
        masked envs draw their start poses on the device."""
        partial = env_mask is not None and (bool(reseat_only) or not np.all(env_mask))
        steps = self.sim._steps_since_full_reset
        if self.random_params is not None:
            self.sim.batch.sample_params(env_mask)
        if poses is None:
            if self.random_start is None:
                raise ValueError("reset() without poses needs random_start=")
            b = self.sim.batch
            b.sample_reset(env_mask)       # (with device_logic also the episode reset)
            poses = b.reset_sampler_poses().reshape(self.num_envs, self.num_agents, 3)
            if not self.device_logic:
                self._lap.reset(poses, env_mask)
        else:
            poses = np.asarray(poses, dtype=np.float64).reshape(self.num_envs, self.num_agents, 3)
            if self.device_logic:
                self.sim.batch.episode_reset(poses.reshape(-1, 3), env_mask)
            else:
                self.sim.reset(poses, env_mask)
                self._lap.reset(poses, env_mask)
        self._start_poses = poses.copy() if self._start_poses is None or env_mask is None else \
            np.where(np.asarray(env_mask, dtype=bool)[:, None, None], poses, self._start_poses)
        self.sim._steps_since_full_reset = steps if partial else 0
        if partial and self._last is not None:
            # partial reset: re-seat only (class docstring); envs in mid-episode are not stepped
            obs, reward, done, info = self._last
            done = np.where(np.asarray(env_mask, dtype=bool), False, done)
            self._last = (obs, reward, done, info)
            return self._last
        return self.step(np.zeros((self.num_envs, self.num_agents, 2)))

    def snapshot(self):
        """an exact copy of the vector env: simulator state (device blob, episode columns included with device_logic), the
        host lap bookkeeping, the start poses and the last (obs, reward, done, info)"""
        snap = {"sim": self.sim.snapshot(), "host": copy.deepcopy((self._lap, self._start_poses, self._last))}
        if self._encode:
            snap["encoded_stack"] = None if self._enc_fill else self.encoded_stack.download()
        return snap

    def restore(self, snap):
        """back to a snapshot(); returns the (obs, reward, done, info) of the step before it.  With device_logic the page-locked
        views step() hands out show that observation again."""
        self.sim.restore(snap["sim"])
        self._lap, self._start_poses, last = copy.deepcopy(snap["host"])
        if self._encode:   # the frame stack as it was; a snapshot without one: the next encode fills every frame
            stack = snap.get("encoded_stack")
            self._enc_fill = stack is None
            if stack is not None:
                self.encoded_stack.upload(stack)
        if self.device_logic and last is not None and not self.copy_obs:
            obs, r, done, info = self._ret_views   # write the saved observation into the block's views
            for mine, saved in ((obs, last[0]), (info, last[3])):
                for k, v in mine.items():
                    if isinstance(v, np.ndarray) and k in saved:   # (a snapshot taken without an encoder has no 'encoded')
                        np.copyto(v, saved[k])
            np.copyto(done, last[2])
            if isinstance(r, np.ndarray):
                np.copyto(r, last[1])
            last = self._ret_views
        self._last = last
        return last

    def _step_device(self, actions, sync=True):
        b, hb = self.sim.batch, self._hb
        if self.sim._noise is not None:
            self.sim._noise.ensure(b, self.sim._steps_since_full_reset + 1)
        if actions is not None and actions is not self.action_buffer:
            hb.actions[...] = np.asarray(actions, dtype=np.float64).reshape(hb.actions.shape)
        if self._encode or self.track_preview is not None or self.neighbors is not None or self.particle_filter is not None:
            # one wait per step: the step enqueued without a wait, the encode / the preview / the neighbours and their copies into page-locked memory behind it
            b.step_host(hb, None, auto_reset=self.auto_reset, sync=False, mapped_actions=self.mapped_actions, spin=self.spin_wait, fuse=self.fuse_host_block, poll=self.poll_wait,
                        scripted=self.scripted is not None or self.line_followers is not None or self.planner is not None)
            if self._encode:
                b.encode_obs_device(self.obs_encoder, self.encoded_stack, fill=self._enc_fill, pinned=self._enc_pinned)
                self._enc_fill = False
            if self.track_preview is not None:
                b.track_preview_device(self.track_preview, self.preview_buffer, pinned=self._prv_pinned)
            if self.neighbors is not None:
                b.neighbors_device(self.neighbors, self.neighbors_buffer, pinned=self._nbr_pinned)
            if self.particle_filter is not None:
                b.localize_device(self.pose_estimate_buffer, self.pf_info_buffer)
            if sync:
                b.sync()
        else:
            b.step_host(hb, None, auto_reset=self.auto_reset, sync=sync, mapped_actions=self.mapped_actions, spin=self.spin_wait, fuse=self.fuse_host_block, poll=self.poll_wait,
                        scripted=self.scripted is not None or self.line_followers is not None or self.planner is not None)
        self.sim._steps_since_full_reset += 1
        if not sync:
            return None
        return self._collect()

    def _collect(self):
        obs, r, done, info = self._ret_views
        if self.particle_filter is not None:   # (the step has been waited for)
            E, A = self.num_envs, self.num_agents
            np.copyto(obs["pose_estimate"], self.pose_estimate_buffer.download().reshape(E, A, 3))
            np.copyto(obs["pf_info"], self.pf_info_buffer.download().reshape(E, A, 4))
        if self.copy_obs:
            obs = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in obs.items()}
            done, info = done.copy(), {k: v.copy() for k, v in info.items()}
            r = r.copy() if isinstance(r, np.ndarray) else r
        self._last = (obs, r, done, info)
        return self._last

    # gym.vector.VectorEnv's split: step_async() enqueues the whole step and returns at once, step_wait()
    # blocks until the observation block is complete (the host may do other work in between)
    def step_async(self, actions):
        if not self.device_logic:
            raise ValueError("step_async needs device_logic=True")
        self._step_device(actions, sync=False)

    def step_wait(self):
        self.sim.batch.sync()
        return self._collect()

    def step(self, actions):
        if self.device_logic:
            return self._step_device(actions)
        if actions is None:
            raise ValueError("step(None) (actions taken from env.action_buffer) needs device_logic=True")
        obs = self.sim.step(actions)
        for f in self._TRACK:
            if f in obs and f not in self.obs_fields:
                del obs[f]
        reward = self.timestep if self.reward_mode == 'timestep' else self.sim.batch.get_track()["ds"].reshape(self.num_envs, self.num_agents)[:, self.ego_idx]
        done, toggles = self._lap.update(obs['poses_x'], obs['poses_y'], obs['collisions'], self.timestep)
        obs['lap_times'] = self._lap.lap_times
        obs['lap_counts'] = self._lap.lap_counts
        info = {'checkpoint_done': toggles, 'toggle_list': self._lap.toggle_list.copy(),
                'near_starts': self._lap.near_starts.copy()}
        if self.auto_reset and done.any():
            if self.random_params is not None:
                self.sim.batch.sample_params(done)
            if self.random_start is not None:   # the draw on the device, the drawn poses back for the host lap logic
                self.sim.batch.sample_reset(done)
                if np.all(done):
                    self.sim._steps_since_full_reset = 0
                drawn = self.sim.batch.reset_sampler_poses().reshape(self.num_envs, self.num_agents, 3)
                self._start_poses = np.where(done[:, None, None], drawn, self._start_poses)
            else:
                self.sim.reset(self._start_poses, done)
            self._lap.reset(self._start_poses, done)
        self._last = (obs, reward, done, info)
        return self._last
