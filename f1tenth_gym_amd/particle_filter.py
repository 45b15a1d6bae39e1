"""ParticleFilter — Monte-Carlo localisation per agent on the device, from the car's own lidar scan.

Not a reference type: the reference hands every consumer the simulator's true pose.  A real F1TENTH car localises with a particle
filter against the map — the filter of the MIT racecar stack — and a stack that must survive localisation error has to be trained
and evaluated with one.  Built next to the reference that means casting P x B' rays per car and per step in a second framework and
keeping a cloud and a noise stream per car by hand.  Here one call (BatchSim.localize_device) does it in device memory for every
armed agent: the draws are NumPy's PCG64 and ziggurat, reproducible draw for draw, the expected ranges are the scan's own rays on
the env's map slot, and the estimate lands in device memory next to the observation.  This class holds and validates the settings
(include/f110.h, f110_pf) and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

MAX_P, MAX_BEAMS = _ffi.PF_MAX_P, _ffi.PF_MAX_BEAMS
INFO = ("effective_samples", "spread_xy", "err_xy", "resampled")   # the columns of the info output
_INTS = ("particles", "n_beams", "beam_first", "beam_stride")
_FLOATS = ("sigma_x", "sigma_y", "sigma_theta", "init_x", "init_y", "init_theta", "sigma_hit", "clip", "squash", "resample_frac")


class ParticleFilter(object):
    """settings of the filter.  particles: P per agent, 1 .. 1024.  n_beams: B' beams of the agent's scan that are compared, 1 .. 128:
    beam_first + j * beam_stride for j < B' (the last one must exist in the handle's scan: checked when the filter is armed).
    sigma_x, sigma_y, sigma_theta >= 0: the odometry noise added per call in the car's frame.  init_x, init_y, init_theta >= 0: the
    spread of a fresh cloud around the true pose (at a reset).  sigma_hit > 0: the range noise in metres.  clip > 0: a beam's error
    is truncated at that many sigmas (inf: no truncation) — what keeps an opponent's return from killing a particle.  squash > 0
    divides the log-likelihood.  resample_frac >= 0: the cloud is resampled when the effective sample size falls below
    resample_frac * P (0: never; above 1: at every call).  Every value but the clip must be finite.  This tracks a pose from a known
    start: it does not localise globally."""

    def __init__(self, particles=256, n_beams=54, beam_first=0, beam_stride=20, sigma_x=0.05, sigma_y=0.02, sigma_theta=0.02, init_x=0.1,
                 init_y=0.1, init_theta=0.05, sigma_hit=0.1, clip=3.0, squash=8.0, resample_frac=0.5):
        ints = dict(particles=particles, n_beams=n_beams, beam_first=beam_first, beam_stride=beam_stride)
        for name, lo, hi in (("particles", 1, MAX_P), ("n_beams", 1, MAX_BEAMS), ("beam_first", 0, 2 ** 31 - 1), ("beam_stride", 1, 2 ** 31 - 1)):
            if not is_int(ints[name]) or not (lo <= ints[name] <= hi):
                raise ValueError("%s must be an integer in %d .. %d, got %r" % (name, lo, hi, ints[name]))
        if beam_first + (n_beams - 1) * beam_stride > 2 ** 31 - 1:
            raise ValueError("the last beam does not fit 31 bits")
        vals = dict(sigma_x=sigma_x, sigma_y=sigma_y, sigma_theta=sigma_theta, init_x=init_x, init_y=init_y, init_theta=init_theta,
                    sigma_hit=sigma_hit, clip=clip, squash=squash, resample_frac=resample_frac)
        for name in _FLOATS:
            if isinstance(vals[name], (bool, np.bool_, str)):
                raise ValueError("%s must be a number, got %r" % (name, vals[name]))
            vals[name] = float(vals[name])
            if np.isnan(vals[name]) or (np.isinf(vals[name]) and not (name == "clip" and vals[name] > 0)):
                raise ValueError("%s must be finite%s, got %r" % (name, " or +inf" if name == "clip" else "", vals[name]))
        for name in ("sigma_x", "sigma_y", "sigma_theta", "init_x", "init_y", "init_theta", "resample_frac"):
            if vals[name] < 0.0:
                raise ValueError("%s must be >= 0, got %r" % (name, vals[name]))
        for name in ("sigma_hit", "clip", "squash"):
            if not vals[name] > 0.0:
                raise ValueError("%s must be > 0, got %r" % (name, vals[name]))
        for name in _INTS:
            setattr(self, name, int(ints[name]))
        for name in _FLOATS:
            setattr(self, name, vals[name])

    @classmethod
    def coerce(cls, spec):
        """a ParticleFilter, or a dict of its keyword arguments"""
        return coerce(cls, spec, "a filter")

    @property
    def beams(self):
        """the indices of the compared beams"""
        return self.beam_first + self.beam_stride * np.arange(self.n_beams)

    @property
    def last_beam(self):
        return self.beam_first + (self.n_beams - 1) * self.beam_stride

    def check_beams(self, num_beams):
        """the ABI's refusal of a beam past the scan"""
        if self.last_beam >= int(num_beams):
            raise ValueError("beam %d is past the scan's %d beams" % (self.last_beam, int(num_beams)))

    def cloud_shape(self, m):
        """the clouds of m armed agents: [m][P][3]"""
        return (int(m), self.particles, 3)

    def spec(self):
        """the C struct"""
        return _ffi.PfSpec(*([getattr(self, n) for n in _INTS] + [getattr(self, n) for n in _FLOATS]))

    def settings(self):
        """the keyword arguments that rebuild these settings"""
        return {name: getattr(self, name) for name in _INTS + _FLOATS}

    def __repr__(self):
        return "ParticleFilter(%s)" % ", ".join("%s=%r" % kv for kv in self.settings().items())


def split_filter(particle_filter):
    """the env layers' `particle_filter` argument, {slot: ParticleFilter | dict} with one entry -> (slot, ParticleFilter), or None"""
    if particle_filter is None:
        return None
    if not isinstance(particle_filter, dict) or len(particle_filter) != 1:
        raise ValueError("particle_filter must be {slot: ParticleFilter} with one entry (one spec per handle), got %r" % (particle_filter,))
    (slot, pf), = particle_filter.items()
    if not is_int(slot):
        raise ValueError("the filter's slot must be an integer, got %r" % (slot,))
    return int(slot), ParticleFilter.coerce(pf)


__all__ = ["ParticleFilter", "INFO", "split_filter"]
