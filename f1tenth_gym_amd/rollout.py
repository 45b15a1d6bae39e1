"""Rollout — candidate action sequences rolled ahead on the device, per agent.

Not a reference type: sampling planners built on the reference (MPPI, motion primitives, lattice planners, safety shields) either
restate the single-track model, the PID, the steering delay and the RK4 in their own code, or clone envs and step the whole
simulator.  Here one call (BatchSim.rollout_device) rolls K candidates of H actions, each held `repeat` steps, from every agent's
live state with the step's own integration, samples the map's clearance at every step and reports where each candidate ends, how
long it stayed clear of the walls and how far it got along the track — float32 [N][K][D] where the state already is.  This class
holds and validates the settings (include/f110.h, f110_rollout) and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

# channel name -> bit number; the output holds the requested channels in this order whatever order they are asked for in
CHANNELS = ("end_x", "end_y", "end_cos", "end_sin", "end_v", "end_yaw_rate", "alive", "min_clear", "progress", "end_lat")
FRAMES = {"ego": _ffi.ROLL_FRAME_EGO, "map": _ffi.ROLL_FRAME_MAP}
LAYOUTS = {"shared": _ffi.ROLL_SHARED, "per_agent": _ffi.ROLL_PER_AGENT}
MAX_K, MAX_H, MAX_REPEAT = _ffi.ROLL_MAX_K, _ffi.ROLL_MAX_H, _ffi.ROLL_MAX_REPEAT
TRAJ_CHANNELS = CHANNELS[:4]


class Rollout(object):
    """settings of a rollout.  k: K candidates per agent, 1 .. 256.  horizon: H actions (steer, speed) per candidate, 1 .. 64.
    repeat: sim steps each action is held, 1 .. 16.  channels: names from CHANNELS.  margin: metres; a candidate is alive while
    the map's clearance at its reference point is above it (not NaN).  frame: 'ego' (the agent's pose at the start: x ahead, y to
    the left) or 'map'.  scale: {channel: divisor} (default 1.0), finite and > 0.  layout: 'shared' (actions [K][H][2], one library
    for all agents) or 'per_agent' ([N][K][H][2]).  traj: also write the pose after every action, float32 [N][K][H][4] = x, y, cos,
    sin in the same frame with the scales of end_x, end_y, end_cos, end_sin.  The summary is float32 [N][K][D], D = len(channels).
    This is free flight against the map: other cars, the iTTC check and the stop on a collision are not modelled."""

    def __init__(self, k=8, horizon=8, repeat=1, channels=('alive', 'min_clear'), margin=0.0, frame='ego', scale=None, layout='shared',
                 traj=False):
        for name, v, hi in (("k", k, MAX_K), ("horizon", horizon, MAX_H), ("repeat", repeat, MAX_REPEAT)):
            if not is_int(v) or not (1 <= v <= hi):
                raise ValueError("%s must be an integer in 1 .. %d, got %r" % (name, hi, v))
        if isinstance(channels, str):
            channels = (channels,)
        channels = tuple(channels)
        for c in channels:
            if c not in CHANNELS:
                raise ValueError("unknown channel %r (known: %s)" % (c, ", ".join(CHANNELS)))
        if not channels:
            raise ValueError("a rollout needs at least one channel")
        if len(set(channels)) != len(channels):
            raise ValueError("a channel is listed twice: %r" % (channels,))
        if frame not in FRAMES:
            raise ValueError("frame must be one of %s, got %r" % (sorted(FRAMES), frame))
        if layout not in LAYOUTS:
            raise ValueError("layout must be one of %s, got %r" % (sorted(LAYOUTS), layout))
        if not isinstance(traj, (bool, np.bool_)) and traj not in (0, 1):
            raise ValueError("traj must be False or True, got %r" % (traj,))
        margin = float(margin)
        if np.isnan(margin):
            raise ValueError("margin must not be NaN")
        traj = bool(traj)
        scale = dict(scale or {})
        for key, v in scale.items():
            if key not in CHANNELS:
                raise ValueError("scale: unknown channel %r" % (key,))
            used = key in channels or (traj and key in TRAJ_CHANNELS)
            if used and not (np.isfinite(float(v)) and float(v) > 0.0):
                raise ValueError("scale[%r] must be finite and > 0, got %r" % (key, v))
        self.k, self.horizon, self.repeat, self.margin, self.frame, self.layout, self.traj = int(k), int(horizon), int(repeat), margin, frame, layout, traj
        self.channels = tuple(c for c in CHANNELS if c in channels)   # the fixed output order
        self.scale = {c: (float(scale[c]) if c in scale and (c in channels or (traj and c in TRAJ_CHANNELS)) else 1.0) for c in CHANNELS}
        self.dim = len(self.channels)

    @classmethod
    def coerce(cls, spec):
        """a Rollout, or a dict of its keyword arguments"""
        return coerce(cls, spec, "a rollout")

    @property
    def channel_mask(self):
        return sum(1 << CHANNELS.index(c) for c in self.channels)

    @property
    def needs_track(self):
        """'progress' and 'end_lat' project on the track of the env's map slot"""
        return "progress" in self.channels or "end_lat" in self.channels

    @property
    def steps(self):
        """sim steps per candidate"""
        return self.horizon * self.repeat

    def shape(self, num_agents_total):
        """the summary's shape [N][K][D]"""
        return (int(num_agents_total), self.k, self.dim)

    def traj_shape(self, num_agents_total):
        """the trajectory's shape [N][K][H][4]"""
        return (int(num_agents_total), self.k, self.horizon, 4)

    def actions_shape(self, num_agents_total):
        """the candidate actions' shape: [K][H][2], or [N][K][H][2] per agent"""
        tail = (self.k, self.horizon, 2)
        return tail if self.layout == "shared" else (int(num_agents_total),) + tail

    def spec(self):
        """the C struct"""
        return _ffi.RolloutSpec(self.k, self.horizon, self.repeat, LAYOUTS[self.layout], FRAMES[self.frame], self.channel_mask, int(self.traj), 0,
                                self.margin, (_ffi.C.c_double * 10)(*[self.scale[c] for c in CHANNELS]))

    def settings(self):
        """the keyword arguments that rebuild these settings"""
        keep = [c for c in CHANNELS if c in self.channels or (self.traj and c in TRAJ_CHANNELS)]
        return dict(k=self.k, horizon=self.horizon, repeat=self.repeat, channels=self.channels, margin=self.margin, frame=self.frame,
                    scale={c: self.scale[c] for c in keep}, layout=self.layout, traj=self.traj)

    def __repr__(self):
        return ("Rollout(k=%d, horizon=%d, repeat=%d, channels=%r, margin=%r, frame=%r, layout=%r, traj=%r)"
                % (self.k, self.horizon, self.repeat, self.channels, self.margin, self.frame, self.layout, self.traj))


__all__ = ["Rollout", "CHANNELS", "FRAMES", "LAYOUTS"]
