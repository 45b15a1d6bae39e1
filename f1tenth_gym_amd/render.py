"""Rendering on the device (include/f110.h f110_render_device): the argument checks and constants shared by
BatchSim.render_device / render and the env layers.  Everything here runs without a GPU, so a bad spec raises ValueError
before the library is called."""
import ctypes as C
import math

import numpy as np

from . import _ffi

VIEWS = {"world": 0, "follow": 1, "ego": 2}
LAYERS = {"map": 1, "track": 2, "scan": 4, "cars": 8}
CLASSES = ("outside", "free", "wall", "track", "scan", "car", "self")
OUTSIDE, FREE, WALL, TRACK, SCAN, CAR, SELF = range(7)
# rendering.py's clear colour (outside, free), its map points and waypoint_follow.py's waypoints (wall, track), then scan,
# car (the other agents' quads) and self (the camera agent's)
DEFAULT_PALETTE = np.array([[9, 32, 87], [9, 32, 87], [183, 193, 222], [183, 193, 222], [255, 190, 0], [99, 52, 94], [172, 97, 185]],
                           dtype=np.uint8)
DEFAULT_PALETTE.setflags(write=False)
MAX_SIDE = 4096
MAX_PIXELS = 1 << 31


class RenderSpec(C.Structure):
    """f110_render_spec"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("view", C.c_int32), ("layers", C.c_int32),
                ("m_per_px", C.c_double), ("center_x", C.c_double), ("center_y", C.c_double), ("angle", C.c_double),
                ("fwd_offset", C.c_double), ("car_length", C.c_double), ("car_width", C.c_double)]


def _finite(v, what):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError("%s must be a number (got %r)" % (what, v))
    if not math.isfinite(v):
        raise ValueError("%s must be finite (got %r)" % (what, v))
    return v


def layer_bits(layers):
    """('map', 'cars', ...) or 'all' or an int mask -> the F110_LAYER_* bits"""
    if isinstance(layers, (int, np.integer)) and not isinstance(layers, bool):
        bits = int(layers)
        if bits & ~15 or bits < 0:
            raise ValueError("unknown layer bits 0x%x (map=1, track=2, scan=4, cars=8)" % bits)
        return bits
    if isinstance(layers, str):
        layers = tuple(LAYERS) if layers == "all" else (layers,)
    bits = 0
    for name in layers:
        if name not in LAYERS:
            raise ValueError("unknown layer %r (one of %s)" % (name, ", ".join(LAYERS)))
        bits |= LAYERS[name]
    return bits


def make_spec(width=64, height=64, view="ego", m_per_px=0.05, center=(0.0, 0.0), angle=0.0, fwd_offset=0.0,
              layers=("map", "cars"), car_size=None):
    """validated f110_render_spec (ValueError on anything the library would refuse)"""
    try:
        w, h = int(width), int(height)
    except (TypeError, ValueError):
        raise ValueError("width and height must be integers")
    if w != width or h != height or not (1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE):
        raise ValueError("width and height must be integers in 1..%d (got %r x %r)" % (MAX_SIDE, width, height))
    mpp = _finite(m_per_px, "m_per_px")
    if not mpp > 0:
        raise ValueError("m_per_px must be > 0 (got %r)" % m_per_px)
    if view not in VIEWS:
        raise ValueError("unknown view %r (one of %s)" % (view, ", ".join(VIEWS)))
    c = tuple(center)
    if len(c) != 2:
        raise ValueError("center must be (x, y)")
    cl = cw = 0.0
    if car_size is not None:
        cs = tuple(car_size)
        if len(cs) != 2:
            raise ValueError("car_size must be (length, width)")
        cl, cw = _finite(cs[0], "car length"), _finite(cs[1], "car width")
        if not (cl > 0 and cw > 0):
            raise ValueError("car_size must be positive (got %r)" % (car_size,))
    return RenderSpec(w, h, VIEWS[view], layer_bits(layers), mpp, _finite(c[0], "center x"), _finite(c[1], "center y"),
                      _finite(angle, "angle"), _finite(fwd_offset, "fwd_offset"), cl, cw)


def check_agents(agents, num_agents_total, spec):
    """camera agents -> int32 [F] (None: every agent, frame f = agent f); ValueError on an index outside [0, N) or too many pixels"""
    N = int(num_agents_total)
    if agents is None:
        a = np.arange(N, dtype=np.int32)
    else:
        a = np.asarray(agents)
        if a.ndim == 0:
            a = a.reshape(1)
        if a.ndim != 1 or a.size < 1:
            raise ValueError("agents must be a non-empty 1-D list of agent indices")
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError("agents must be integers")
        if np.any(a < 0) or np.any(a >= N):
            raise ValueError("agent index outside [0, %d): %s" % (N, a[(a < 0) | (a >= N)][:4].tolist()))
        a = np.ascontiguousarray(a, dtype=np.int32)
    if a.size * spec.width * spec.height > MAX_PIXELS:
        raise ValueError("%d frames of %d x %d pixels exceed 2^31" % (a.size, spec.height, spec.width))
    return a


def check_palette(palette):
    """[7][3] uint8 (None: DEFAULT_PALETTE)"""
    if palette is None:
        return np.ascontiguousarray(DEFAULT_PALETTE)
    p = np.asarray(palette)
    if p.shape != (7, 3):
        raise ValueError("palette must be [7][3] (one RGB colour per class), got shape %s" % (p.shape,))
    if np.issubdtype(p.dtype, np.floating) and not np.all(np.isfinite(p)):
        raise ValueError("palette must be finite")
    if np.any(p < 0) or np.any(p > 255) or np.any(p != np.round(p)):
        raise ValueError("palette entries must be integers in 0..255")
    return np.ascontiguousarray(p, dtype=np.uint8)


def colorize(classes, palette=None):
    """host-side palette[classes] (what the device's RGB output is)"""
    return check_palette(palette)[np.asarray(classes)]
