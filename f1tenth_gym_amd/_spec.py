"""What the settings classes (Mppi, Rollout, ParticleFilter, Neighbors, TrackPreview, ObsEncoder, GapFollower, Opponents) share."""
import numpy as np


def is_int(v):
    """an integer that is not a bool"""
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def coerce(cls, spec, noun, article="a"):
    """`spec` as a `cls`: an instance as it is, a dict as its keyword arguments.  The refusal reads "<noun> must be <article>
    <class> or a dict of its settings": noun is what the callers name the argument ("a planner", "neighbors", ...)."""
    if isinstance(spec, cls):
        return spec
    if isinstance(spec, dict):
        return cls(**spec)
    raise TypeError("%s must be %s %s or a dict of its settings, got %r" % (noun, article, cls.__name__, spec))
