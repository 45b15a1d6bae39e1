"""ObsEncoder — compact float32 observations with frame stacking, encoded on the device.

Not a reference type: RL setups built on the reference pool obs['scans'] into a few ranges, append a few state columns and
stack the last frames on the host.  Here one call (BatchSim.encode_obs_device) turns the last step's observation into
out [N][F][D] float32 where the scans already are; the stack is refilled for agents that start an episode, which only the
simulator knows (its step_count column).  This class holds and validates the settings (include/f110.h, f110_obs_spec) and
needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

POOLS = {"min": _ffi.OBS_POOL_MIN, "mean": _ffi.OBS_POOL_MEAN, "center": _ffi.OBS_POOL_CENTER}
# feature name -> bit number; the features follow the lidar values in this order whatever order they are asked for in
FEATURES = ("vx", "steer", "yaw_rate", "slip", "collision", "lateral", "heading_error", "ds")
TRACK_FEATURES = ("lateral", "heading_error", "ds")
MAX_FRAMES, MAX_STACK = _ffi.OBS_MAX_FRAMES, _ffi.OBS_MAX_STACK


class ObsEncoder(object):
    """settings of the observation encoder.  sectors: K pooled lidar values (0: none) of the beams `beams` = (lo, hi) (None:
    all); pool: 'min', 'mean' or 'center'; each value is min(v, range_clip) / range_scale.  features: names from FEATURES
    (the track ones need a track), each divided by scales[name] (default 1.0).  frames: F stacked frames, newest last.
    The output is float32 [N][F][D], D = sectors + len(features).  num_beams (optional) checks the beam range at once;
    otherwise the handle that encodes checks it."""

    def __init__(self, sectors=108, pool='min', beams=None, features=('vx', 'steer', 'yaw_rate', 'slip', 'collision'), frames=1,
                 range_clip=30.0, range_scale=30.0, scales=None, num_beams=None):
        if not is_int(sectors) or sectors < 0:
            raise ValueError("sectors must be an integer >= 0, got %r" % (sectors,))
        if pool not in POOLS:
            raise ValueError("pool must be one of %s, got %r" % (sorted(POOLS), pool))
        if beams is not None:
            beams = tuple(beams)
            if len(beams) != 2 or not all(is_int(v) for v in beams) or not (0 <= beams[0] < beams[1]):
                raise ValueError("beams must be (lo, hi) with 0 <= lo < hi, got %r" % (beams,))
            beams = (int(beams[0]), int(beams[1]))
        if isinstance(features, str):
            features = (features,)
        features = tuple(features)
        for f in features:
            if f not in FEATURES:
                raise ValueError("unknown feature %r (known: %s)" % (f, ", ".join(FEATURES)))
        if len(set(features)) != len(features):
            raise ValueError("a feature is listed twice: %r" % (features,))
        if not is_int(frames) or not (1 <= frames <= MAX_FRAMES):
            raise ValueError("frames must be an integer in 1 .. %d, got %r" % (MAX_FRAMES, frames))
        range_clip, range_scale = float(range_clip), float(range_scale)
        if not (np.isfinite(range_clip) and range_clip > 0.0 and np.isfinite(range_scale) and range_scale > 0.0):
            raise ValueError("range_clip and range_scale must be finite and > 0, got %r, %r" % (range_clip, range_scale))
        scales = dict(scales or {})
        for k, v in scales.items():
            if k not in FEATURES:
                raise ValueError("scales: unknown feature %r" % (k,))
            if not (np.isfinite(float(v)) and float(v) != 0.0):
                raise ValueError("scales[%r] must be finite and non-zero, got %r" % (k, v))
        self.sectors, self.pool, self.beams, self.frames = int(sectors), pool, beams, int(frames)
        self.features = tuple(f for f in FEATURES if f in features)   # the fixed output order
        self.range_clip, self.range_scale = range_clip, range_scale
        self.scales = {f: float(scales.get(f, 1.0)) for f in FEATURES}
        self.dim = self.sectors + len(self.features)
        if self.dim == 0:
            raise ValueError("an encoder needs sectors > 0 or at least one feature (D = 0)")
        if self.frames * self.dim > MAX_STACK:
            raise ValueError("frames * D = %d exceeds %d" % (self.frames * self.dim, MAX_STACK))
        if beams is not None and self.sectors > beams[1] - beams[0]:
            raise ValueError("sectors = %d exceeds the %d beams used" % (self.sectors, beams[1] - beams[0]))
        if num_beams is not None:
            self.check_beams(num_beams)

    @classmethod
    def coerce(cls, spec):
        """an ObsEncoder, or a dict of its keyword arguments"""
        return coerce(cls, spec, "obs_encoder", "an")

    def check_beams(self, num_beams):
        """the beam range and the sector count against a scan of num_beams beams; returns (lo, hi)"""
        lo, hi = self.beams if self.beams is not None else (0, int(num_beams))
        if hi > num_beams:
            raise ValueError("beams [%d, %d) are not a range within the %d beams" % (lo, hi, num_beams))
        if self.sectors > hi - lo:
            raise ValueError("sectors = %d exceeds the %d beams used" % (self.sectors, hi - lo))
        return lo, hi

    @property
    def needs_track(self):
        return any(f in TRACK_FEATURES for f in self.features)

    @property
    def feature_mask(self):
        return sum(1 << FEATURES.index(f) for f in self.features)

    def shape(self, num_agents_total):
        """the output shape [N][F][D]"""
        return (int(num_agents_total), self.frames, self.dim)

    def spec(self, fill=False):
        """the C struct"""
        lo, hi = self.beams if self.beams is not None else (0, 0)
        return _ffi.ObsSpec(lo, hi, self.sectors, POOLS[self.pool], self.feature_mask, self.frames, _ffi.OBS_FILL if fill else 0, 0,
                            self.range_clip, self.range_scale, (_ffi.C.c_double * 8)(*[self.scales[f] for f in FEATURES]))

    def __repr__(self):
        return ("ObsEncoder(sectors=%d, pool=%r, beams=%r, features=%r, frames=%d, range_clip=%r, range_scale=%r)"
                % (self.sectors, self.pool, self.beams, self.features, self.frames, self.range_clip, self.range_scale))


__all__ = ["ObsEncoder", "FEATURES", "POOLS"]
