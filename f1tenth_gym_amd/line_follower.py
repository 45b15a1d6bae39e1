"""LineFollower — a scripted car that drives the line of its map slot, run on the device.

Not a reference type.  Pure pursuit on the track of the agent's map slot (track= / tracks=, 'raceline' for the solved line), the
speed from a track attribute (speed_attr=1 is the raceline's vx), slower behind a car ahead on the same lane.  Agents are assigned
a follower with BatchSim.set_line_followers or F110VecEnv(scripted=...); one kernel turns the track columns of the last step into
actions where they already are.  This class holds and validates the settings (include/f110.h, f110_line_follower, states the rule)
and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int
from .gap_follower import GapFollower

MAX_SPECS, MAX_AGENTS = _ffi.LINE_MAX_SPECS, _ffi.LINE_MAX_AGENTS
_FLOATS = _ffi.LINE_FLOATS
RAW = ("ld", "s_t", "k", "X", "Y", "Tx", "Ty", "lx", "ly", "vref", "lim", "speed")
INFO = ("ld", "vref", "k", "lim")


class LineFollower(object):
    """settings of one line follower.  Lookahead ld = clamp(look_base + look_gain * |v|, look_min, look_max) metres; the target is
    the line's point ld ahead, lane_offset metres to its left; steer = clamp(atan(2 * wheelbase * ly / d2), steer_max).  The
    speed is vgain times attribute column speed_attr of the track speed_look metres ahead (-1: v_const), v_recover at most when the
    car is more than lat_slow metres off its lane.  Behind a car within follow_range metres ahead and lane_width metres aside the
    speed is at most v_b + follow_gain * (gap - follow_gap); follow_range=0 turns that off.  The result is clamped to
    [v_min, v_max]."""

    def __init__(self, look_base=0.8, look_gain=0.25, look_min=0.6, look_max=3.9, lane_offset=0.0, wheelbase=0.3302, steer_max=0.4189,
                 speed_attr=1, v_const=2.0, vgain=0.8, speed_look=0.6, lat_slow=0.5, v_recover=1.5, follow_range=6.0, follow_gap=1.0,
                 follow_gain=1.0, lane_width=0.6, v_min=0.0, v_max=20.0):
        vals = dict(look_base=look_base, look_gain=look_gain, look_min=look_min, look_max=look_max, lane_offset=lane_offset,
                    wheelbase=wheelbase, steer_max=steer_max, v_const=v_const, vgain=vgain, speed_look=speed_look, lat_slow=lat_slow,
                    v_recover=v_recover, follow_range=follow_range, follow_gap=follow_gap, follow_gain=follow_gain, lane_width=lane_width,
                    v_min=v_min, v_max=v_max)
        for k in _FLOATS:
            vals[k] = float(vals[k])
            if not np.isfinite(vals[k]):
                raise ValueError("%s must be finite, got %r" % (k, vals[k]))
        for k in ("look_min", "wheelbase"):
            if not vals[k] > 0.0:
                raise ValueError("%s must be > 0, got %r" % (k, vals[k]))
        for k in ("look_base", "look_gain", "speed_look", "steer_max", "v_min", "follow_range", "lane_width", "lat_slow"):
            if vals[k] < 0.0:
                raise ValueError("%s must be >= 0, got %r" % (k, vals[k]))
        if vals["look_min"] > vals["look_max"]:
            raise ValueError("look_min = %r exceeds look_max = %r" % (vals["look_min"], vals["look_max"]))
        if vals["v_min"] > vals["v_max"]:
            raise ValueError("v_min = %r exceeds v_max = %r" % (vals["v_min"], vals["v_max"]))
        if not is_int(speed_attr) or not (-1 <= speed_attr < _ffi.TRACK_MAX_ATTRS):
            raise ValueError("speed_attr must be an integer in -1 .. %d, got %r" % (_ffi.TRACK_MAX_ATTRS - 1, speed_attr))
        self.speed_attr = int(speed_attr)
        self.__dict__.update(vals)

    @classmethod
    def coerce(cls, spec):
        """a LineFollower, or a dict of its keyword arguments"""
        return coerce(cls, spec, "a line follower")

    def settings(self):
        """the settings as a dict (the keyword arguments that rebuild this follower)"""
        d = dict((k, getattr(self, k)) for k in _FLOATS)
        d["speed_attr"] = self.speed_attr
        return d

    def spec(self):
        """the C struct"""
        return _ffi.LineFollowerSpec(*([getattr(self, k) for k in _FLOATS] + [self.speed_attr, 0]))

    def __repr__(self):
        return "LineFollower(%s)" % ", ".join("%s=%r" % kv for kv in self.settings().items())


def _coerce_any(c):
    """a controller of either class as it is; a dict is a GapFollower's settings, as it has always been"""
    return c if isinstance(c, LineFollower) else GapFollower.coerce(c)


def mixed_scripted(scripted, num_envs, num_agents):
    """F110VecEnv's `scripted` argument with both controller classes -> (assign int32 [E][A], the mixed list): {slot: controller}
    gives every env's car `slot` that controller; (assign, controllers) is taken as it is (-1 = external, else an index into
    the list)"""
    E, A = int(num_envs), int(num_agents)
    if isinstance(scripted, dict):
        assign = np.full((E, A), -1, dtype=np.int32)
        ctrls = []
        for slot, c in sorted(scripted.items()):
            if not is_int(slot) or not (0 <= slot < A):
                raise ValueError("scripted: slot %r is not one of the %d cars of an env" % (slot, A))
            assign[:, slot] = len(ctrls)
            ctrls.append(_coerce_any(c))
    else:
        try:
            assign, ctrls = scripted
        except (TypeError, ValueError):
            raise TypeError("scripted must be {slot: controller} or (assign [E][A], [controllers])")
        assign = np.array(assign, dtype=np.int32)
        if assign.shape != (E, A):
            raise ValueError("scripted: the assignment must be [%d][%d], got %r" % (E, A, assign.shape))
        ctrls = [_coerce_any(c) for c in ctrls]
    if len(ctrls) < 1:
        raise ValueError("scripted: at least one controller")
    if assign.min() < -1 or assign.max() >= len(ctrls):
        raise ValueError("scripted: an assignment is outside -1 .. %d" % (len(ctrls) - 1))
    return assign, ctrls


def coerce_scripted_mixed(scripted, num_envs, num_agents):
    """mixed_scripted, split by class -> ((gap_assign, [GapFollower]) or None, (line_assign, [LineFollower]) or None), what the
    two ABI calls take.  Each class keeps the order of the list and is re-indexed from 0; a class nobody is assigned to drops
    out."""
    E, A = int(num_envs), int(num_agents)
    assign, ctrls = mixed_scripted(scripted, E, A)
    out = []
    for cls, most in ((GapFollower, _ffi.GAP_MAX_SPECS), (LineFollower, MAX_SPECS)):
        idx = [i for i, c in enumerate(ctrls) if isinstance(c, cls)]
        if len(idx) > most:
            raise ValueError("scripted: 1 .. %d controllers of a kind, got %d %ss" % (most, len(idx), cls.__name__))
        own = np.full((E, A), -1, dtype=np.int32)
        for new, i in enumerate(idx):
            own[assign == i] = new
        out.append((own, [ctrls[i] for i in idx]) if idx and (own >= 0).any() else None)
    return tuple(out)


def has_line_follower(scripted):
    """does a `scripted` argument name a LineFollower?  (such inputs go through coerce_scripted_mixed; every other input keeps
    gap_follower.coerce_scripted's behaviour)"""
    if isinstance(scripted, dict):
        return any(isinstance(c, LineFollower) for c in scripted.values())
    try:
        _, ctrls = scripted
        return any(isinstance(c, LineFollower) for c in ctrls)
    except (TypeError, ValueError):
        return False


__all__ = ["LineFollower", "mixed_scripted", "coerce_scripted_mixed", "has_line_follower", "RAW", "INFO"]
