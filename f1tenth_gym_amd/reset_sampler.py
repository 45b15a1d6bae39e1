"""ResetSampler — randomised start poses along the track, drawn on the device at every reset.

Not a reference type: training setups built on the reference pick a random waypoint, add lateral and heading jitter,
check the spot is free and call reset(poses) on the host.  Here the draw runs on the device, inside the call that
re-seats an env, so auto-reset loops keep their one call per step.  This class holds and validates the settings and
computes each env's PCG64 stream words (np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(e,))) for the global
env index e) on the host; it needs no GPU.  BatchSim.set_reset_sampler arms it on a handle.
"""
import numpy as np

from . import _ffi

_U32 = (1 << 32) - 1


def _int_words(n):
    """NumPy's _int_to_uint32_array: little-endian uint32 words of a non-negative int (0 -> [0])"""
    n = int(n)
    if n < 0:
        raise ValueError("a seed must be non-negative, got %d" % n)
    words = [0] if n == 0 else []
    while n > 0:
        words.append(n & _U32)
        n >>= 32
    return words


def _words_of(x):
    """NumPy's _coerce_to_uint32_array for ints and (nested) sequences of ints"""
    if isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_)):
        return _int_words(x)
    if isinstance(x, np.ndarray) and x.dtype == np.uint32:
        return [int(v) for v in x.ravel()]
    out = []
    for v in x:
        out += _words_of(v)
    return out


def entropy_words(seed):
    """the run entropy of np.random.SeedSequence(seed), as uint32 words.  A plain int is split into its words here (NumPy's
    rule, the common case); anything else goes through NumPy's SeedSequence once (None: fresh OS entropy, drawn once), which
    validates it, and the words are held to that SeedSequence's entropy pool."""
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, (bool, np.bool_)):
        return np.array(_int_words(seed), dtype=np.uint32)
    ss = seed if isinstance(seed, np.random.SeedSequence) else np.random.SeedSequence(seed)
    if len(ss.spawn_key):
        raise ValueError("a SeedSequence with a spawn key cannot seed a reset sampler (pass its entropy)")
    try:   # NumPy's own coercion where it exists (a module-level helper of numpy.random.bit_generator)
        from numpy.random.bit_generator import _coerce_to_uint32_array
        words = [int(v) for v in _coerce_to_uint32_array(ss.entropy)]
    except ImportError:
        words = _words_of(ss.entropy)
    if not np.array_equal(np.random.SeedSequence(words).pool, ss.pool):   # the same run entropy mixes to the same pool
        raise ValueError("seed %r: its uint32 words could not be recovered" % (seed,))
    return np.array(words, dtype=np.uint32)


def stream_words(seed, n, e0=0):
    """{state.hi, state.lo, inc.hi, inc.lo} of PCG64(SeedSequence(seed, spawn_key=(e,))) for e = e0 .. e0 + n - 1: [n][4]"""
    ent = entropy_words(seed)
    if ent.size == 0:
        ent = np.zeros(1, dtype=np.uint32)   # (an empty sequence assembles to the zero-filled pool: the same words as [0])
    ent = np.ascontiguousarray(ent, dtype=np.uint32)
    out = np.empty((int(n), 4), dtype=np.uint64)
    rc = _ffi.lib().f110_pcg64_seed_spawn(ent.ctypes.data_as(_ffi._u32p), int(ent.size), int(e0), int(n), out.ctypes.data_as(_ffi._u64p))
    if rc != 0:
        raise ValueError("f110_pcg64_seed_spawn refused (%d)" % rc)
    return out


class ResetSampler(object):
    """settings of the start-pose draw (f110_reset_sampler).  s_range: fractions of the track length; gap: metres between
    consecutive agents along the track; lateral / heading: largest offset (m) / jitter (rad); clearance: metres (None: half
    the diagonal of the car, sqrt(length^2 + width^2) / 2, filled in by the handle that arms it); attempts: 1 .. 1024.
    seed: anything np.random.SeedSequence takes as entropy (None: OS entropy, drawn once here)."""

    def __init__(self, seed=None, s_range=(0.0, 1.0), gap=1.0, lateral=0.0, heading=0.0, clearance=None, attempts=16):
        s_lo, s_hi = (float(v) for v in s_range)
        if not (0.0 <= s_lo < s_hi <= 1.0):
            raise ValueError("s_range must satisfy 0 <= s_lo < s_hi <= 1, got (%r, %r)" % (s_lo, s_hi))
        gap, lateral, heading = float(gap), float(lateral), float(heading)
        if not (np.isfinite(gap) and gap > 0.0):
            raise ValueError("gap must be finite and > 0, got %r" % gap)
        if not (np.isfinite(lateral) and lateral >= 0.0):
            raise ValueError("lateral must be finite and >= 0, got %r" % lateral)
        if not (np.isfinite(heading) and heading >= 0.0):
            raise ValueError("heading must be finite and >= 0, got %r" % heading)
        if clearance is not None:
            clearance = float(clearance)
            if not (np.isfinite(clearance) and clearance >= 0.0):
                raise ValueError("clearance must be finite and >= 0, got %r" % clearance)
        if isinstance(attempts, (bool, np.bool_)) or int(attempts) != attempts or not (1 <= int(attempts) <= 1024):
            raise ValueError("attempts must be an integer in 1 .. 1024, got %r" % (attempts,))
        self.entropy = entropy_words(seed)   # (seed=None: the entropy is drawn once, so every shard and re-arm sees the same)
        self.seed = seed
        self.s_range = (s_lo, s_hi)
        self.gap, self.lateral, self.heading, self.clearance = gap, lateral, heading, clearance
        self.attempts = int(attempts)

    @classmethod
    def coerce(cls, spec):
        """a ResetSampler, or a dict of its keyword arguments"""
        if isinstance(spec, ResetSampler):
            return spec
        if isinstance(spec, dict):
            return cls(**spec)
        raise TypeError("random_start must be a ResetSampler or a dict of its settings, got %r" % (spec,))

    def with_clearance(self, length, width):
        """the clearance this sampler uses for a car of `length` x `width` (its own, when set)"""
        if self.clearance is not None:
            return self.clearance
        return float(np.sqrt(length * length + width * width) / 2.0)

    def streams(self, n, env_base=0):
        """the stream words of envs env_base .. env_base + n - 1: uint64 [n][4]"""
        return stream_words([int(w) for w in self.entropy], n, env_base)   # (each word w < 2^32 re-assembles to [w])

    def spec(self, length, width):
        """the C struct for a car of `length` x `width`"""
        return _ffi.ResetSamplerSpec(self.s_range[0], self.s_range[1], self.gap, self.lateral, self.heading,
                                     self.with_clearance(length, width), self.attempts, 0)

    def __repr__(self):
        return ("ResetSampler(s_range=%r, gap=%r, lateral=%r, heading=%r, clearance=%r, attempts=%d)"
                % (self.s_range, self.gap, self.lateral, self.heading, self.clearance, self.attempts))


__all__ = ["ResetSampler", "stream_words", "entropy_words"]
