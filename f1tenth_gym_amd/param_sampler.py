"""ParamSampler — randomised vehicle parameters, drawn on the device at every reset.

Not a reference type: the reference's update_params is a host call between episodes.  Here the draw runs on the device,
inside the call that re-seats an env, so auto-reset loops keep their one call per step while friction, stiffness, mass,
inertia, centre of gravity and the actuator limits change per episode.  This class holds the 18 entries (one per parameter
of _ffi.PARAM_KEYS; width and length cannot be drawn), validates them against the nominal parameter sets by intervals, and
computes each env's PCG64 stream words (np.random.PCG64(np.random.SeedSequence(seed, spawn_key=(e,))) for the global env
index e: the reset sampler's rule, so a user who arms both gives them different seeds).  It needs no GPU.
BatchSim.set_param_sampler arms it on a handle.

The draw of one env (include/f110.h): parameters in PARAM_KEYS order; within a parameter the env's single value (scope
'env') or agents 0 .. A - 1 (scope 'agent'); uniform(a, b) is Generator.uniform(a, b), normal(loc, scale, lo, hi) is
np.clip(Generator.normal(loc, scale), lo, hi); relative=True stores nominal * value.
"""
import numpy as np

from . import _ffi, _spec
from .reset_sampler import entropy_words, stream_words

KINDS = {"fixed": _ffi.PARAM_FIXED, "uniform": _ffi.PARAM_UNIFORM, "normal": _ffi.PARAM_NORMAL}
SCOPES = {"agent": _ffi.PARAM_SCOPE_AGENT, "env": _ffi.PARAM_SCOPE_ENV}
_POSITIVE = ("mu", "C_Sf", "C_Sr", "lf", "lr", "h", "m", "I", "v_switch", "a_max")
_BELOW = (("s_min", "s_max"), ("sv_min", "sv_max"), ("v_min", "v_max"))
_NOT_DRAWN = ("width", "length")


class Dist(object):
    """one entry (f110_param_dist): kind 'fixed' | 'uniform' | 'normal', scope 'agent' | 'env', a, b, lo, hi, relative"""

    def __init__(self, kind, a=0.0, b=0.0, lo=0.0, hi=0.0, scope="agent", relative=False):
        if kind not in KINDS:
            raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
        if scope not in SCOPES:
            raise ValueError("scope must be 'agent' or 'env', got %r" % (scope,))
        self.kind, self.scope, self.relative = kind, scope, bool(relative)
        self.a, self.b, self.lo, self.hi = float(a), float(b), float(lo), float(hi)

    @property
    def interval(self):
        """the interval a drawn value lies in"""
        return (self.a, self.b) if self.kind == "uniform" else (self.lo, self.hi)

    def entry(self):
        return _ffi.ParamDist(KINDS[self.kind], SCOPES[self.scope], self.a, self.b, self.lo, self.hi, 1 if self.relative else 0, 0)

    def __repr__(self):
        if self.kind == "fixed":
            return "fixed()"
        tail = ", scope=%r, relative=%r)" % (self.scope, self.relative)
        if self.kind == "uniform":
            return "uniform(%r, %r" % (self.a, self.b) + tail
        return "normal(%r, %r, %r, %r" % (self.a, self.b, self.lo, self.hi) + tail


def uniform(a, b, scope="agent", relative=False):
    """v = Generator.uniform(a, b)"""
    return Dist("uniform", a, b, scope=scope, relative=relative)


def normal(loc, scale, lo, hi, scope="agent", relative=False):
    """v = np.clip(Generator.normal(loc, scale), lo, hi)"""
    return Dist("normal", loc, scale, lo, hi, scope=scope, relative=relative)


def _as_dist(name, v):
    if isinstance(v, Dist):
        return v
    if isinstance(v, dict):
        return Dist(**v)
    if isinstance(v, (tuple, list)) and len(v) and isinstance(v[0], str):
        make = {"uniform": uniform, "normal": normal}.get(v[0])
        if make is None:
            raise ValueError("parameter %s: unknown distribution %r" % (name, v[0]))
        return make(*v[1:])
    raise TypeError("parameter %s: expected uniform(...), normal(...), a dict of Dist's arguments or a ('uniform' | 'normal', ...) "
                    "tuple, got %r" % (name, v))


def nominal_rows(params, num_agents=None):
    """[A][18] float64 of: an array of that shape, one parameter dict (every agent slot), or a list of A dicts"""
    if isinstance(params, dict):
        rows = np.stack([_ffi.params_vector(params)] * int(num_agents or 1))
    elif isinstance(params, (list, tuple)) and len(params) and isinstance(params[0], dict):
        rows = np.stack([_ffi.params_vector(p) for p in params])
    else:
        rows = np.array(params, dtype=np.float64)
        if rows.ndim == 1:
            rows = np.stack([rows] * int(num_agents or 1))
    if rows.ndim != 2 or rows.shape[1] != _ffi.NPARAMS or rows.shape[0] < 1:
        raise ValueError("nominal rows must be [A][%d], got %s" % (_ffi.NPARAMS, rows.shape))
    return np.ascontiguousarray(rows, dtype=np.float64)


class ParamSampler(object):
    """ParamSampler(seed, mu=uniform(0.5, 1.1, scope='env'), m=uniform(0.85, 1.15, relative=True), ...): the entries by
    parameter name; a parameter that is not named is not drawn.  seed: anything np.random.SeedSequence takes as entropy
    (None: OS entropy, drawn once here)."""

    def __init__(self, seed=None, **dists):
        unknown = [k for k in dists if k not in _ffi.PARAM_KEYS]
        if unknown:
            raise ValueError("unknown parameter(s) %s; the parameters are %s" % (sorted(unknown), _ffi.PARAM_KEYS))
        self.entropy = entropy_words(seed)   # (seed=None: drawn once, so every shard and re-arm sees the same)
        self.seed = seed
        self.dists = {k: _as_dist(k, dists[k]) for k in _ffi.PARAM_KEYS if k in dists}

    @classmethod
    def coerce(cls, spec):
        """a ParamSampler, or a dict of its keyword arguments"""
        return _spec.coerce(cls, spec, "random_params")

    def dist(self, name):
        return self.dists.get(name) or Dist("fixed")

    @property
    def drawn(self):
        """the names of the drawn parameters, in draw order"""
        return [k for k in _ffi.PARAM_KEYS if self.dist(k).kind != "fixed"]

    def streams(self, n, env_base=0):
        """the stream words of envs env_base .. env_base + n - 1: uint64 [n][4]"""
        return stream_words([int(w) for w in self.entropy], n, env_base)   # (each word w < 2^32 re-assembles to [w])

    def entries(self):
        """the 18 f110_param_dist entries, a ctypes array"""
        return (_ffi.ParamDist * _ffi.NPARAMS)(*[self.dist(k).entry() for k in _ffi.PARAM_KEYS])

    def validate(self, nominal, num_agents=None):
        """what arming refuses (include/f110.h), as a ValueError that names the parameter, before any ABI call.
        nominal: the agent slots' parameter sets, [A][18] / a dict / a list of dicts."""
        rows = nominal_rows(nominal, num_agents)
        for name in self.drawn:
            d = self.dist(name)
            if name in _NOT_DRAWN:
                raise ValueError("parameter %s cannot be drawn: the collision boxes and the iTTC side tables are the constructor's" % name)
            if not (np.isfinite(d.a) and np.isfinite(d.b)):
                raise ValueError("parameter %s: a = %r, b = %r must be finite" % (name, d.a, d.b))
            if d.kind == "uniform":
                if d.a > d.b:
                    raise ValueError("parameter %s: uniform needs a <= b, got %r, %r" % (name, d.a, d.b))
            else:
                if d.b < 0.0:
                    raise ValueError("parameter %s: normal needs scale >= 0, got %r" % (name, d.b))
                if not (np.isfinite(d.lo) and np.isfinite(d.hi)):
                    raise ValueError("parameter %s: normal needs finite clip bounds, got %r, %r" % (name, d.lo, d.hi))
                if d.lo > d.hi:
                    raise ValueError("parameter %s: normal needs lo <= hi, got %r, %r" % (name, d.lo, d.hi))
        for s in range(rows.shape[0]):
            reach = {}
            for p, name in enumerate(_ffi.PARAM_KEYS):
                d, nom = self.dist(name), float(rows[s, p])
                if d.kind == "fixed":
                    reach[name] = (nom, nom)
                    continue
                x, y = d.interval
                if d.relative:
                    x, y = nom * x, nom * y
                if not (np.isfinite(x) and np.isfinite(y)):
                    raise ValueError("parameter %s: its interval times the nominal value of agent slot %d is not finite" % (name, s))
                reach[name] = (min(x, y), max(x, y))
            for name in _POSITIVE:
                if self.dist(name).kind != "fixed" and not reach[name][0] > 0.0:
                    raise ValueError("parameter %s must stay above 0, its draws reach %r (agent slot %d)" % (name, reach[name][0], s))
            for lo_name, hi_name in _BELOW:
                if (self.dist(lo_name).kind != "fixed" or self.dist(hi_name).kind != "fixed") and not reach[lo_name][1] < reach[hi_name][0]:
                    raise ValueError("parameter %s must stay below %s, its draws reach %r against %r (agent slot %d)"
                                     % (lo_name, hi_name, reach[lo_name][1], reach[hi_name][0], s))
        return rows

    def __repr__(self):
        return "ParamSampler(%s)" % ", ".join("%s=%r" % (k, self.dists[k]) for k in _ffi.PARAM_KEYS if k in self.dists)


__all__ = ["ParamSampler", "Dist", "uniform", "normal", "nominal_rows"]
