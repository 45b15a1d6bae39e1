"""Opponents — the other cars of an agent's env predicted over a horizon, for the rollout and the MPPI planner.

Not a reference type.  The rollout and the planner fly free against the map; with these settings attached every candidate is also
measured against where the env's other cars will be: each is predicted from its live state, at constant velocity along its heading
('cv') or along the raceline with its lateral offset kept ('track'), once per call, and every candidate keeps its smallest distance
to a prediction (OPP_MIN) and the first action at which it comes within `radius` of one (OPP_FREE, the horizon when none does).
This class holds and validates the settings (include/f110.h, f110_opponents) and needs no GPU.
"""
import math

import numpy as np

from . import _ffi
from ._spec import coerce

MODES = {"cv": _ffi.OPP_CV, "track": _ffi.OPP_TRACK}
MAX_OPPONENTS = _ffi.OPP_MAX
CHANNELS = ("opp_min", "opp_free")   # the two values per candidate


def _number(name, v):
    if isinstance(v, (bool, np.bool_, str)) or v is None:
        raise ValueError("%s must be a number, got %r" % (name, v))
    return float(v)


def check_weights(w_hit, w_near, near_ref):
    """the planner's two weights (finite, >= 0) and its reference distance (finite), as floats"""
    w_hit, w_near, near_ref = _number("w_hit", w_hit), _number("w_near", w_near), _number("near_ref", near_ref)
    for name, v in (("w_hit", w_hit), ("w_near", w_near)):
        if not math.isfinite(v) or v < 0.0:
            raise ValueError("%s must be finite and >= 0, got %r" % (name, v))
    if not math.isfinite(near_ref):
        raise ValueError("near_ref must be finite, got %r" % (near_ref,))
    return w_hit, w_near, near_ref


class Opponents(object):
    """mode: 'cv' (constant velocity along the heading) or 'track' (along the raceline, the lateral offset kept; needs a track on
    the map slots in use).  radius: metres, finite and > 0; a sample closer than this to a predicted opponent is a hit.  max_range:
    metres, > 0, inf allowed; an opponent further than this from the agent at the start of the call is ignored."""

    def __init__(self, mode="cv", radius=0.4, max_range=float("inf")):
        if not isinstance(mode, str) or mode not in MODES:
            raise ValueError("mode must be 'cv' or 'track', got %r" % (mode,))
        radius, max_range = _number("radius", radius), _number("max_range", max_range)
        if not math.isfinite(radius) or not radius > 0.0:
            raise ValueError("radius must be finite and > 0, got %r" % (radius,))
        if math.isnan(max_range) or not max_range > 0.0:
            raise ValueError("max_range must be > 0 (inf allowed), got %r" % (max_range,))
        self.mode, self.radius, self.max_range = mode, radius, max_range

    @classmethod
    def coerce(cls, spec):
        """an Opponents, or a dict of its keyword arguments"""
        return coerce(cls, spec, "opponents", "an")

    @property
    def needs_track(self):
        return self.mode == "track"

    def spec(self):
        """the C struct"""
        return _ffi.OpponentsSpec(MODES[self.mode], 0, self.radius, self.max_range)

    def settings(self):
        """the keyword arguments that rebuild these settings"""
        return dict(mode=self.mode, radius=self.radius, max_range=self.max_range)

    def __repr__(self):
        return "Opponents(%s)" % ", ".join("%s=%r" % kv for kv in self.settings().items())


def split_mppi_opponents(arg):
    """the env layers' `mppi_opponents` argument, dict(opponents=..., w_hit=..., w_near=..., near_ref=...) -> (Opponents, w_hit,
    w_near, near_ref), or None for None"""
    if arg is None:
        return None
    if not isinstance(arg, dict) or "opponents" not in arg:
        raise TypeError("mppi_opponents must be a dict with 'opponents' and optionally w_hit, w_near, near_ref, got %r" % (arg,))
    extra = set(arg) - {"opponents", "w_hit", "w_near", "near_ref"}
    if extra:
        raise TypeError("mppi_opponents: unknown keys %s" % sorted(extra))
    return (Opponents.coerce(arg["opponents"]),) + check_weights(arg.get("w_hit", 0.0), arg.get("w_near", 0.0), arg.get("near_ref", 0.0))


__all__ = ["Opponents", "CHANNELS", "MODES", "MAX_OPPONENTS", "check_weights", "split_mppi_opponents"]
