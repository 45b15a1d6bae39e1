"""ShardedVecEnv.reset decides "partial" once, from the global mask (no GPU: the shards are stand-ins recording their calls)."""
import numpy as np
import pytest

from f1tenth_gym_amd import sharded


class _Shard(object):
    calls = []

    def __init__(self, num_envs, **kw):
        self.num_envs, self.num_agents = num_envs, kw.get("num_agents", 2)
        self.device_logic = kw.get("device_logic", True)
        self.obs_fields = ()

    def reset(self, poses, env_mask=None, reseat_only=False):
        _Shard.calls.append((self.num_envs, None if env_mask is None else np.asarray(env_mask).tolist(), reseat_only))
        E = self.num_envs
        return {"x": np.zeros((E, self.num_agents))}, 0.01, np.zeros(E, bool), {"t": np.zeros((E, self.num_agents))}


@pytest.fixture
def env(monkeypatch):
    monkeypatch.setattr(sharded, "F110VecEnv", _Shard)
    _Shard.calls = []
    e = sharded.ShardedVecEnv(6, devices=(0, 0, 0), shard_sizes=[1, 2, 3], num_agents=1)
    e.close = lambda: None
    yield e
    for w in e._workers:
        w.stop()


def _calls():
    return sorted(_Shard.calls)


def test_a_partial_mask_covering_whole_shards_re_seats_only(env):
    env.reset(np.zeros((6, 1, 3)), [True, False, False, True, True, True])   # shard 0 (1 env) and shard 2 whole
    assert _calls() == [(1, [True], True), (2, [False, False], True), (3, [True, True, True], True)]


def test_full_and_unmasked_resets_are_full_on_every_shard(env):
    env.reset(np.zeros((6, 1, 3)), [True] * 6)
    assert _calls() == [(1, [True], False), (2, [True, True], False), (3, [True, True, True], False)]
    _Shard.calls = []
    env.reset(np.zeros((6, 1, 3)))
    assert _calls() == [(1, None, False), (2, None, False), (3, None, False)]
