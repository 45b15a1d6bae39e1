"""TrackPreview — the raceline ahead of each agent, in its own frame, computed on the device.

Not a reference type: trajectory-aided learners and pure-pursuit-style policies built on the reference interpolate the next few
waypoints in NumPy after copying the poses back.  Here one call (BatchSim.track_preview_device) turns each agent's arc length `s`
of the step just taken into P stations ahead of it — position, tangent and up to four interpolated per-point attributes of the
track (Track(attrs=...)), in the car's frame or the map's — as float32 [N][P][D] where the track tables already are.  This class
holds and validates the settings (include/f110.h, f110_track_preview) and needs no GPU.
"""
import numpy as np

from . import _ffi
from ._spec import coerce, is_int

# channel name -> bit number; the output holds the requested channels in this order whatever order they are asked for in
CHANNELS = ("x", "y", "tan_x", "tan_y", "attr0", "attr1", "attr2", "attr3")
FRAMES = {"ego": _ffi.PREVIEW_FRAME_EGO, "world": _ffi.PREVIEW_FRAME_WORLD}
MAX_POINTS = _ffi.PREVIEW_MAX_POINTS


class TrackPreview(object):
    """settings of the track preview.  points: P stations, 1 .. 32; station j lies offset + j * spacing metres ahead of the
    agent's projection on its track (offset >= 0, spacing > 0).  channels: names from CHANNELS ('attr0' .. 'attr3' are the
    track's attribute columns).  frame: 'ego' (x ahead, y to the left of the car; tangents rotated alike) or 'world'.  scale:
    {channel: divisor} (default 1.0), finite and non-zero.  The output is float32 [N][P][D], D = len(channels)."""

    def __init__(self, points=8, offset=0.5, spacing=0.5, channels=('x', 'y'), frame='ego', scale=None):
        if not is_int(points) or not (1 <= points <= MAX_POINTS):
            raise ValueError("points must be an integer in 1 .. %d, got %r" % (MAX_POINTS, points))
        if isinstance(channels, str):
            channels = (channels,)
        channels = tuple(channels)
        for c in channels:
            if c not in CHANNELS:
                raise ValueError("unknown channel %r (known: %s)" % (c, ", ".join(CHANNELS)))
        if not channels:
            raise ValueError("a preview needs at least one channel")
        if len(set(channels)) != len(channels):
            raise ValueError("a channel is listed twice: %r" % (channels,))
        if frame not in FRAMES:
            raise ValueError("frame must be one of %s, got %r" % (sorted(FRAMES), frame))
        offset, spacing = float(offset), float(spacing)
        if not (np.isfinite(offset) and offset >= 0.0):
            raise ValueError("offset must be finite and >= 0, got %r" % (offset,))
        if not (np.isfinite(spacing) and spacing > 0.0):
            raise ValueError("spacing must be finite and > 0, got %r" % (spacing,))
        scale = dict(scale or {})
        for k, v in scale.items():
            if k not in CHANNELS:
                raise ValueError("scale: unknown channel %r" % (k,))
            if k in channels and not (np.isfinite(float(v)) and float(v) != 0.0):
                raise ValueError("scale[%r] must be finite and non-zero, got %r" % (k, v))
        self.points, self.offset, self.spacing, self.frame = int(points), offset, spacing, frame
        self.channels = tuple(c for c in CHANNELS if c in channels)   # the fixed output order
        self.scale = {c: (float(scale[c]) if c in scale and c in channels else 1.0) for c in CHANNELS}
        self.dim = len(self.channels)

    @classmethod
    def coerce(cls, spec):
        """a TrackPreview, or a dict of its keyword arguments"""
        return coerce(cls, spec, "track_preview")

    @property
    def channel_mask(self):
        return sum(1 << CHANNELS.index(c) for c in self.channels)

    @property
    def num_attrs(self):
        """how many attribute columns a track must carry for this preview"""
        return max([CHANNELS.index(c) - 3 for c in self.channels if c.startswith("attr")] + [0])

    @property
    def reach(self):
        """metres from the agent's projection to the last station"""
        return self.offset + float(self.points - 1) * self.spacing

    def check_track(self, track):
        """what the library asks of a track in use: the requested attributes, and a closed track longer than the reach"""
        if self.num_attrs > track.num_attrs:
            raise ValueError("the preview asks for attribute %d, but the track carries %d" % (self.num_attrs - 1, track.num_attrs))
        if track.closed and not (track.length > self.reach):
            raise ValueError("the closed track is %.6g m long, not longer than the preview's reach of %.6g m" % (track.length, self.reach))

    def shape(self, num_agents_total):
        """the output shape [N][P][D]"""
        return (int(num_agents_total), self.points, self.dim)

    def spec(self):
        """the C struct"""
        return _ffi.TrackPreviewSpec(self.points, self.channel_mask, FRAMES[self.frame], 0, self.offset, self.spacing,
                                     (_ffi.C.c_double * 8)(*[self.scale[c] for c in CHANNELS]))

    def settings(self):
        """the keyword arguments that rebuild this preview"""
        return dict(points=self.points, offset=self.offset, spacing=self.spacing, channels=self.channels, frame=self.frame,
                    scale={c: self.scale[c] for c in self.channels})

    def __repr__(self):
        return ("TrackPreview(points=%d, offset=%r, spacing=%r, channels=%r, frame=%r)"
                % (self.points, self.offset, self.spacing, self.channels, self.frame))


__all__ = ["TrackPreview", "CHANNELS", "FRAMES"]
