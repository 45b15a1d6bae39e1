"""GapFollower — a follow-the-gap controller for the cars no policy drives, run on the device.

Not a reference type: the reference leaves every car's action to the caller.  Here agents can be assigned a controller
(BatchSim.set_controllers, F110VecEnv(scripted=...)); one kernel turns their scan rows of the last step into actions where the
scans already are, and the other agents' actions stay the caller's.  This class holds and validates the settings
(include/f110.h, f110_gap_follower, states the rule) and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

TARGETS = {"center": _ffi.GAP_TARGET_CENTER, "furthest": _ffi.GAP_TARGET_FURTHEST}
MAX_SPECS, MAX_SMOOTH, MAX_WINDOW = _ffi.GAP_MAX_SPECS, _ffi.GAP_MAX_SMOOTH, _ffi.GAP_MAX_WINDOW
_FLOATS = ("range_clip", "bubble_radius", "gap_threshold", "steer_gain", "steer_max", "v_lo", "v_hi", "d_ref", "steer_slow", "v_turn",
           "v_blocked")


class GapFollower(object):
    """settings of one controller.  beams: (lo, hi), the window of beams it looks at; None: the middle two thirds of the
    handle's beams, B // 6 .. B - B // 6 (180 .. 900 at 1080 beams); (0, 0): all beams.  smooth: odd window of the running
    mean; range_clip, bubble_radius, gap_threshold in metres; target: 'center' or 'furthest'; steer = clamp(steer_gain *
    angle, steer_max); speed runs from v_lo to v_hi with the target's range over d_ref, is capped at v_turn beyond
    steer_slow, and is v_blocked when no beam is free.  num_beams (optional) checks the window at once; otherwise the handle
    that runs it checks it."""

    def __init__(self, beams=None, smooth=5, range_clip=10.0, bubble_radius=0.6, gap_threshold=1.5, target='center', steer_gain=1.0,
                 steer_max=0.4189, v_lo=1.5, v_hi=4.0, d_ref=8.0, steer_slow=0.2, v_turn=2.5, v_blocked=0.5, num_beams=None):
        if beams is not None:
            beams = tuple(beams)
            if len(beams) != 2 or not all(is_int(v) for v in beams) or not (beams == (0, 0) or 0 <= beams[0] < beams[1]):
                raise ValueError("beams must be (lo, hi) with 0 <= lo < hi, or (0, 0) for all, got %r" % (beams,))
            beams = (int(beams[0]), int(beams[1]))
            if beams[1] - beams[0] > MAX_WINDOW:
                raise ValueError("a window of %d beams exceeds %d" % (beams[1] - beams[0], MAX_WINDOW))
        if not is_int(smooth) or not (1 <= smooth <= MAX_SMOOTH) or smooth % 2 == 0:
            raise ValueError("smooth must be an odd integer in 1 .. %d, got %r" % (MAX_SMOOTH, smooth))
        if beams is not None and beams != (0, 0) and smooth > beams[1] - beams[0]:
            raise ValueError("smooth = %d exceeds the %d beams of the window" % (smooth, beams[1] - beams[0]))
        if target in (_ffi.GAP_TARGET_CENTER, _ffi.GAP_TARGET_FURTHEST) and is_int(target):
            target = "center" if target == _ffi.GAP_TARGET_CENTER else "furthest"
        if target not in TARGETS:
            raise ValueError("target must be one of %s, got %r" % (sorted(TARGETS), target))
        vals = dict(range_clip=range_clip, bubble_radius=bubble_radius, gap_threshold=gap_threshold, steer_gain=steer_gain, steer_max=steer_max,
                    v_lo=v_lo, v_hi=v_hi, d_ref=d_ref, steer_slow=steer_slow, v_turn=v_turn, v_blocked=v_blocked)
        for k in _FLOATS:
            vals[k] = float(vals[k])
            if not np.isfinite(vals[k]):
                raise ValueError("%s must be finite, got %r" % (k, vals[k]))
        for k in ("range_clip", "d_ref"):
            if not vals[k] > 0.0:
                raise ValueError("%s must be > 0, got %r" % (k, vals[k]))
        for k in ("bubble_radius", "gap_threshold", "steer_slow", "steer_max"):
            if vals[k] < 0.0:
                raise ValueError("%s must be >= 0, got %r" % (k, vals[k]))
        if vals["v_lo"] > vals["v_hi"]:
            raise ValueError("v_lo = %r exceeds v_hi = %r" % (vals["v_lo"], vals["v_hi"]))
        self.beams, self.smooth, self.target = beams, int(smooth), target
        self.__dict__.update(vals)
        if num_beams is not None:
            self.window(num_beams)

    @classmethod
    def coerce(cls, spec):
        """a GapFollower, or a dict of its keyword arguments"""
        return coerce(cls, spec, "a controller")

    def window(self, num_beams):
        """(lo, hi) at a scan of num_beams beams, checked against it"""
        B = int(num_beams)
        lo, hi = (B // 6, B - B // 6) if self.beams is None else ((0, B) if self.beams == (0, 0) else self.beams)
        if hi > B or lo >= hi:
            raise ValueError("beams [%d, %d) are not a range within the %d beams" % (lo, hi, B))
        if hi - lo > MAX_WINDOW:
            raise ValueError("a window of %d beams exceeds %d" % (hi - lo, MAX_WINDOW))
        if self.smooth > hi - lo:
            raise ValueError("smooth = %d exceeds the %d beams of the window" % (self.smooth, hi - lo))
        return lo, hi

    def settings(self):
        """the settings as a dict (the keyword arguments that rebuild this controller)"""
        d = dict(beams=self.beams, smooth=self.smooth, target=self.target)
        d.update((k, getattr(self, k)) for k in _FLOATS)
        return d

    def spec(self, num_beams):
        """the C struct for a handle of num_beams beams"""
        lo, hi = self.window(num_beams)
        return _ffi.GapFollowerSpec(lo, hi, self.smooth, TARGETS[self.target], *[getattr(self, k) for k in _FLOATS])

    def __repr__(self):
        return "GapFollower(%s)" % ", ".join("%s=%r" % kv for kv in self.settings().items())


def coerce_scripted(scripted, num_envs, num_agents):
    """F110VecEnv's `scripted` argument -> (assign int32 [E][A], [GapFollower]): {slot: controller} gives every env's car `slot`
    that controller; (assign, controllers) is taken as it is (assign [E][A], -1 = external, else an index into controllers)"""
    E, A = int(num_envs), int(num_agents)
    if isinstance(scripted, dict):
        assign = np.full((E, A), -1, dtype=np.int32)
        ctrls = []
        for slot, c in sorted(scripted.items()):
            if not is_int(slot) or not (0 <= slot < A):
                raise ValueError("scripted: slot %r is not one of the %d cars of an env" % (slot, A))
            assign[:, slot] = len(ctrls)
            ctrls.append(GapFollower.coerce(c))
    else:
        try:
            assign, ctrls = scripted
        except (TypeError, ValueError):
            raise TypeError("scripted must be {slot: controller} or (assign [E][A], [controllers])")
        assign = np.array(assign, dtype=np.int32)
        if assign.shape != (E, A):
            raise ValueError("scripted: the assignment must be [%d][%d], got %r" % (E, A, assign.shape))
        ctrls = [GapFollower.coerce(c) for c in ctrls]
    if not (1 <= len(ctrls) <= MAX_SPECS):
        raise ValueError("scripted: 1 .. %d controllers, got %d" % (MAX_SPECS, len(ctrls)))
    if assign.min() < -1 or assign.max() >= len(ctrls):
        raise ValueError("scripted: an assignment is outside -1 .. %d" % (len(ctrls) - 1))
    return assign, ctrls


__all__ = ["GapFollower", "TARGETS", "coerce_scripted"]
