"""What the eight settings classes share (no GPU): `coerce` gives an instance back as itself, builds one from a dict of its keyword
arguments and refuses anything else with the class's own TypeError text; an integer setting is never a bool."""
import numpy as np
import pytest

import f1tenth_gym_amd as amd

# class, a dict of settings that differ from the defaults, the attribute that shows it, the TypeError text up to ", got ..."
CLASSES = [
    (amd.Mppi, dict(k=4, horizon=3), "k", "a planner must be an Mppi or a dict of its settings"),
    (amd.Rollout, dict(k=3, horizon=2), "k", "a rollout must be a Rollout or a dict of its settings"),
    (amd.ParticleFilter, dict(particles=17, n_beams=4), "particles", "a filter must be a ParticleFilter or a dict of its settings"),
    (amd.Neighbors, dict(k=2), "k", "neighbors must be a Neighbors or a dict of its settings"),
    (amd.TrackPreview, dict(points=3), "points", "track_preview must be a TrackPreview or a dict of its settings"),
    (amd.ObsEncoder, dict(sectors=4, frames=2), "frames", "obs_encoder must be an ObsEncoder or a dict of its settings"),
    (amd.GapFollower, dict(smooth=3), "smooth", "a controller must be a GapFollower or a dict of its settings"),
    (amd.Opponents, dict(radius=0.7), "radius", "opponents must be an Opponents or a dict of its settings"),
]
IDS = [c[0].__name__ for c in CLASSES]


@pytest.mark.parametrize("cls, settings, attr, text", CLASSES, ids=IDS)
def test_coerce_takes_an_instance_or_a_dict_and_nothing_else(cls, settings, attr, text):
    made = cls(**settings)
    assert cls.coerce(made) is made
    built = cls.coerce(dict(settings))
    assert type(built) is cls and built is not made and getattr(built, attr) == settings[attr] != getattr(cls(), attr)
    assert repr(vars(built)) == repr(vars(made))
    for other in (None, 3, "k=4", [("k", 4)], cls):
        with pytest.raises(TypeError) as e:
            cls.coerce(other)
        assert str(e.value) == "%s, got %r" % (text, other)
    with pytest.raises(TypeError):
        cls.coerce(dict(no_such_setting=1))            # the constructor's own refusal of an unknown keyword


@pytest.mark.parametrize("cls, settings, attr, text", CLASSES[:7], ids=IDS[:7])
def test_an_integer_setting_refuses_a_bool(cls, settings, attr, text):
    for flag in (True, np.True_):
        with pytest.raises(ValueError):
            cls(**dict(settings, **{attr: flag}))
    assert getattr(cls(**dict(settings, **{attr: np.int64(settings[attr])})), attr) == settings[attr]


def test_is_int():
    from f1tenth_gym_amd._spec import is_int
    for v in (0, -3, 1 << 40, np.int32(5), np.uint8(5), np.int64(-1)):
        assert is_int(v), v
    for v in (True, False, np.True_, np.bool_(False), 1.0, np.float64(2.0), "1", None, [1]):
        assert not is_int(v), v
