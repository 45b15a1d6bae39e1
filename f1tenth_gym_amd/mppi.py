"""Mppi — a sampling planner per agent on the device, on top of the rollout.

Not a reference type: MPPI (model predictive path integral control) is the sampling planner run on F1TENTH cars.  Built on the
reference it means drawing K noisy action sequences around a nominal one, rolling each ahead with a restated vehicle model, weighting
them by exp(-cost / lambda) and averaging — per car and per step, in a second framework.  Here one call (BatchSim.mppi_device) does
all of that in device memory for every armed agent: the draws are NumPy's PCG64 and ziggurat, reproducible draw for draw, the motion
is the step's own integration (the rollout's), and the action lands in the step's action buffer.  This class holds and validates the
settings (include/f110.h, f110_mppi) and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

MAX_K, MAX_H, MAX_REPEAT = _ffi.MPPI_MAX_K, _ffi.MPPI_MAX_H, _ffi.MPPI_MAX_REPEAT
INFO = ("beta", "cost_nominal", "effective_samples", "best")   # the columns of the info output
_FLOATS = ("sigma_steer", "sigma_speed", "steer_min", "steer_max", "speed_min", "speed_max", "lam", "w_dead", "w_clear", "w_progress",
           "w_lat", "clear_ref", "v_init")


class Mppi(object):
    """settings of the planner.  k: K candidates per agent, 1 .. 256 (candidate 0 is the nominal sequence itself).  horizon: H
    actions (steer, speed) per candidate, 1 .. 64.  repeat: sim steps each action is held, 1 .. 16.  shift: after a call the stored
    nominal moves one action ahead (True) or stays (False).  margin: metres; a candidate is alive while the map's clearance at its
    reference point is above it (not NaN).  sigma_steer, sigma_speed >= 0: the standard deviations of the noise.  steer_min <=
    steer_max, speed_min <= speed_max: every sampled action is clamped to them.  lam > 0: the temperature (`lambda` in the C
    struct).  The cost of a candidate is w_dead * (sim steps not survived) + w_clear * max(clear_ref - min clearance, 0)
    - w_progress * (metres along the track) + w_lat * |lateral offset at the end|, every weight >= 0; w_progress and w_lat need a
    track on the map slots in use.  v_init: the speed of a fresh nominal (0 steer), within the speed bounds.  Every value but the
    margin must be finite.  This is free flight against the map: other cars are not predicted."""

    def __init__(self, k=64, horizon=8, repeat=3, shift=True, margin=0.3, sigma_steer=0.15, sigma_speed=1.0, steer_min=-0.4189,
                 steer_max=0.4189, speed_min=0.5, speed_max=7.0, lam=1.0, w_dead=10.0, w_clear=20.0, w_progress=10.0, w_lat=0.0,
                 clear_ref=0.6, v_init=2.0):
        for name, v, hi in (("k", k, MAX_K), ("horizon", horizon, MAX_H), ("repeat", repeat, MAX_REPEAT)):
            if not is_int(v) or not (1 <= v <= hi):
                raise ValueError("%s must be an integer in 1 .. %d, got %r" % (name, hi, v))
        if not isinstance(shift, (bool, np.bool_)) and not (is_int(shift) and shift in (0, 1)):
            raise ValueError("shift must be False or True, got %r" % (shift,))
        margin = float(margin)
        if np.isnan(margin):
            raise ValueError("margin must not be NaN")
        vals = dict(sigma_steer=sigma_steer, sigma_speed=sigma_speed, steer_min=steer_min, steer_max=steer_max, speed_min=speed_min,
                    speed_max=speed_max, lam=lam, w_dead=w_dead, w_clear=w_clear, w_progress=w_progress, w_lat=w_lat, clear_ref=clear_ref,
                    v_init=v_init)
        for name in _FLOATS:
            if isinstance(vals[name], (bool, np.bool_, str)):
                raise ValueError("%s must be a number, got %r" % (name, vals[name]))
            vals[name] = float(vals[name])
            if not np.isfinite(vals[name]):
                raise ValueError("%s must be finite, got %r" % (name, vals[name]))
        for name in ("sigma_steer", "sigma_speed", "w_dead", "w_clear", "w_progress", "w_lat"):
            if vals[name] < 0.0:
                raise ValueError("%s must be >= 0, got %r" % (name, vals[name]))
        if vals["steer_min"] > vals["steer_max"]:
            raise ValueError("steer_min exceeds steer_max")
        if vals["speed_min"] > vals["speed_max"]:
            raise ValueError("speed_min exceeds speed_max")
        if not vals["lam"] > 0.0:
            raise ValueError("lam must be > 0, got %r" % (vals["lam"],))
        if not (vals["speed_min"] <= vals["v_init"] <= vals["speed_max"]):
            raise ValueError("v_init must lie within [speed_min, speed_max]")
        self.k, self.horizon, self.repeat, self.shift, self.margin = int(k), int(horizon), int(repeat), bool(shift), margin
        for name in _FLOATS:
            setattr(self, name, vals[name])

    @classmethod
    def coerce(cls, spec):
        """an Mppi, or a dict of its keyword arguments"""
        return coerce(cls, spec, "a planner", "an")

    @property
    def needs_track(self):
        """w_progress and w_lat project on the track of the env's map slot"""
        return self.w_progress != 0.0 or self.w_lat != 0.0

    @property
    def steps(self):
        """sim steps per candidate"""
        return self.horizon * self.repeat

    def nominal_shape(self, m):
        """the stored nominal sequences of m armed agents: [m][H][2]"""
        return (int(m), self.horizon, 2)

    def fresh_nominal(self, m):
        """what arming stores: (0, v_init) for every action"""
        u = np.zeros(self.nominal_shape(m))
        u[..., 1] = self.v_init
        return u

    def spec(self):
        """the C struct"""
        return _ffi.MppiSpec(self.k, self.horizon, self.repeat, int(self.shift), self.margin, self.sigma_steer, self.sigma_speed, self.steer_min,
                             self.steer_max, self.speed_min, self.speed_max, self.lam, self.w_dead, self.w_clear, self.w_progress, self.w_lat,
                             self.clear_ref, self.v_init)

    def settings(self):
        """the keyword arguments that rebuild these settings"""
        d = dict(k=self.k, horizon=self.horizon, repeat=self.repeat, shift=self.shift, margin=self.margin)
        d.update({name: getattr(self, name) for name in _FLOATS})
        return d

    def __repr__(self):
        return "Mppi(%s)" % ", ".join("%s=%r" % kv for kv in self.settings().items())


def split_scripted(scripted, planner=None):
    """the env layers' `scripted` argument -> (the same without its planner entry, or None when nothing is left; (slot, Mppi) or
    None).  {slot: Mppi} entries are taken out of the dict form; `planner` = (slot, Mppi | dict) is the explicit form.  More than
    one planner is refused."""
    found = []
    if planner is not None:
        try:
            slot, mp = planner
        except (TypeError, ValueError):
            raise TypeError("planner must be (slot, Mppi)")
        found.append((slot, Mppi.coerce(mp)))
    if isinstance(scripted, dict):
        rest = {}
        for slot, c in scripted.items():
            if isinstance(c, Mppi):
                found.append((slot, c))
            else:
                rest[slot] = c
        scripted = rest or None
    if len(found) > 1:
        raise ValueError("at most one Mppi planner per env object, got %d" % len(found))
    if found and not is_int(found[0][0]):
        raise ValueError("the planner's slot must be an integer, got %r" % (found[0][0],))
    return scripted, ((int(found[0][0]), found[0][1]) if found else None)


__all__ = ["Mppi", "INFO", "split_scripted"]
