"""GPU tests (-m gpu) of the agent-aligned scan's env order: k_scan_rays_agent walks an env's agents sector by sector
(scan_task_agent, f110_math.hpp) and a wave keeps its lanes' noise samples while consecutive tasks are on the same
(noise row, sector).  One task per wave can share nothing, so a handle built with scan_tasks_per_wave = 1 is the yardstick:
every other grouping must give the same bits.  The oracle (NumPy's rows, NORTH_STAR as in the other oracle tests) says the
bits are also the right ones."""
import numpy as np
import pytest

from _util import load_map_image, oracle_map_dt, bench_start_poses, rel_err

pytestmark = pytest.mark.gpu
NORTH_STAR = 1e-5
FIELDS = ("scans", "in_collision", "collisions", "state", "step_count")
SEED, STD = 12345, 0.01


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def orc():
    from oracle import orc as o
    return o


@pytest.fixture(scope="module")
def example_map():
    return load_map_image("example_map")


def _rows(T, B):
    return np.random.default_rng(SEED).normal(0., STD, size=(T, B))


def _actions(E, A, k):
    rng = np.random.default_rng(100 + k)
    return np.stack([rng.uniform(-0.3, 0.3, E * A), rng.uniform(1.0, 7.0, E * A)], axis=1)


# 8 steps as bursts of back-to-back f110_step_device calls; env 1 and env 3 are re-seated by mask after steps 2 and 5, so
# that neighbouring envs (which waves of 2 .. 4 tasks straddle: E is odd) sit on different noise rows from then on
BURSTS = (2, 3, 3)
RESEAT = np.array([0, 1, 0, 1, 0], dtype=np.uint8)


def _run(amd, example_map, E, A, B, tpw, groups, noise, bursts=BURSTS, reseat=RESEAT):
    """-> the observables after every burst"""
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, scan_tasks_per_wave=tpw, step_groups=groups)
    s.set_map_image(*example_map)
    noise(s)
    poses = bench_start_poses(E, A, gap_wp=4)
    s.reset(poses)
    d_act = s.device_array((E * A, 2))
    outs = []
    for k, burst in enumerate(bursts):
        d_act.upload(_actions(E, A, k))
        for _ in range(burst):
            s.step_device(d_act)
        outs.append(s.get(*FIELDS))
        if reseat is not None and k + 1 < len(bursts):
            s.reset(poses, reseat)
    s.close()
    return outs


def _same(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for kk in FIELDS:
            assert np.array_equal(g[kk], w[kk]), (what, "burst %d" % k, kk)


def _shared(s):
    s.set_noise_rng(SEED, STD)


_one_task = {}


def _yardstick(amd, example_map, E, A, B, groups, noise, key, **kw):
    """the same run with one task per wave, computed once per shape"""
    k = (E, A, B, groups, key)
    if k not in _one_task:
        _one_task[k] = _run(amd, example_map, E, A, B, 1, groups, noise, **kw)
    return _one_task[k]


# B = 64: one whole sector; 65: one lane in the last sector (the product marches so thin a scan with the flat kernel, which
# this change leaves alone: the case pins that); 125: the smallest beam count with two sectors, the last partly idle, that
# the agent-aligned kernel takes; 1080: the headline's 17 sectors, 56 lanes in the last
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("B", [64, 65, 125, 1080])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_task_grouping_is_invisible_with_the_shared_stream(amd, example_map, A, B, groups):
    E = 5
    want = _yardstick(amd, example_map, E, A, B, groups, _shared, "shared")
    assert (want[-1]["step_count"].reshape(E, A)[:, 0] == [8, 3, 8, 3, 8]).all()   # envs 1 and 3 are five rows behind their neighbours
    for tpw in (2, 3, 4):
        _same(_run(amd, example_map, E, A, B, tpw, groups, _shared), want, "A=%d B=%d tasks per wave %d groups %d" % (A, B, tpw, groups))


@pytest.fixture(scope="module")
def oracle_run(orc):
    """the oracle's run of the same scenario, NumPy's rows, once per (A, B)"""
    cache = {}

    def get(E, A, B):
        if (A, B) not in cache:
            dt, res, origin = oracle_map_dt("example_map")
            ref = orc.SimOracle(E, A, num_beams=B)
            ref.set_map_dt(dt, res, origin)
            ref.set_noise(_rows(8, B))
            poses = bench_start_poses(E, A, gap_wp=4)
            ref.reset(poses)
            outs = []
            for k, burst in enumerate(BURSTS):
                act = _actions(E, A, k)
                for _ in range(burst):
                    ref.step(act)
                outs.append({"scans": ref.scans.copy(), "state": ref.state.copy(), "collisions": ref.collisions.copy(),
                             "in_collision": ref.in_collision.copy(), "step_count": ref.step_count.copy()})
                if k + 1 < len(BURSTS):
                    ref.reset(poses, RESEAT)
            cache[(A, B)] = outs
        return cache[(A, B)]
    return get


def _near_oracle(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["collisions"], w["collisions"]) and np.array_equal(g["in_collision"], w["in_collision"]), (what, k)
        assert np.array_equal(g["step_count"], w["step_count"]), (what, k)
        es, er = rel_err(g["state"], w["state"]), rel_err(g["scans"], w["scans"])
        assert es < NORTH_STAR and er < NORTH_STAR, (what, k, es, er)


@pytest.mark.parametrize("B", [64, 65, 1080])
@pytest.mark.parametrize("A", [1, 2, 3])
def test_task_grouping_vs_oracle(amd, example_map, oracle_run, A, B):
    E = 5
    want = oracle_run(E, A, B)
    for tpw, groups in ((2, 1), (3, 2), (4, 2), (4, 1)):
        _near_oracle(_run(amd, example_map, E, A, B, tpw, groups, _shared), want, "A=%d B=%d tasks per wave %d groups %d" % (A, B, tpw, groups))


# ---- the rows that must not be shared
def _per_agent(E, A):
    def f(s):
        s.set_noise_rng(None, STD, per_agent_seeds=[1000 + 7 * i for i in range(E * A)])   # row -2: each agent's own row in scans[]
    return f


def _off(s):
    s.set_noise_off()                                  # row -1


def _cache4(s):
    s.set_noise_rng(SEED, STD, cache_rows=4)           # rows 0 .. 3 from the cache, then -2: the rows run out mid-run


def _table3(B):
    def f(s):
        s.set_noise_table(_rows(3, B))                 # an uploaded table of 3 rows: the row wraps
    return f


@pytest.mark.parametrize("kind", ["per_agent", "off", "cache4", "table3"])
@pytest.mark.parametrize("A", [2, 3])
def test_rows_that_are_not_shared(amd, example_map, kind, A):
    E, B = 5, 1080
    noise = {"per_agent": _per_agent(E, A), "off": _off, "cache4": _cache4, "table3": _table3(B)}[kind]
    if kind == "cache4":   # stepped to step 7 without a re-seat: every env runs past the cache's four rows
        kw = dict(bursts=(2, 3, 3), reseat=None)
    else:
        kw = {}
    for groups in (1, 2):
        want = _yardstick(amd, example_map, E, A, B, groups, noise, kind, **kw)
        if kind == "cache4":
            assert (want[-1]["step_count"] == 8).all()
        for tpw in (2, 3, 4):
            _same(_run(amd, example_map, E, A, B, tpw, groups, noise, **kw), want, "%s A=%d tasks per wave %d groups %d" % (kind, A, tpw, groups))


# ---- the longest-first form
def test_longest_first_form_with_grouped_tasks(amd, orc, example_map):
    """360 envs x 2 at 1080 beams = 12 240 tasks: the smallest batch that takes the longest-first kernel (SCHED).  30 steps, envs
    whose cars crashed re-seated in place by mask after every step, so that last step's long tasks sit on the list and the normal pass
    skips them between tasks that share a sample.  Bit for bit against one task per wave, and against the oracle."""
    E, A, B, T = 360, 2, 1080, 30
    dt, res, origin = oracle_map_dt("example_map")
    rows = _rows(T, B)
    ref = orc.SimOracle(E, A, num_beams=B)
    ref.set_map_dt(dt, res, origin)
    ref.set_noise(rows)
    poses = bench_start_poses(E, A, gap_wp=4)
    ref.reset(poses)
    sims = []
    for tpw in (1, 2, 3, 4):
        s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, scan_tasks_per_wave=tpw, step_groups=1)
        s.set_map_image(*example_map)
        s.set_noise_rng(SEED, STD)
        s.reset(poses)
        sims.append(s)
    rng = np.random.default_rng(9)
    reseated = 0
    for t in range(T):
        if t % 6 == 0:
            act = np.stack([rng.uniform(-0.3, 0.3, E * A), rng.uniform(3.0, 9.0, E * A)], axis=1)   # fast and blind: crashes
        ref.step(act, 8)
        outs = []
        for s in sims:
            s.step(act)
            outs.append(s.get(*FIELDS))
        for o, tpw in zip(outs[1:], (2, 3, 4)):
            for kk in FIELDS:
                assert np.array_equal(o[kk], outs[0][kk]), (kk, t, tpw)
        want = {"scans": ref.scans, "state": ref.state, "collisions": ref.collisions, "in_collision": ref.in_collision,
                "step_count": ref.step_count}
        _near_oracle([outs[2]], [want], "longest-first, step %d" % t)
        mask = (ref.collisions.reshape(E, A) != 0).any(axis=1).astype(np.uint8)
        if mask.any():
            reseated += int(mask.sum())
            ref.reset(poses, mask)
            for s in sims:
                s.reset(poses, mask)
    assert reseated > 0, "no env was re-seated: the scenario does not put neighbouring envs on different rows"
    for s in sims:
        s.close()
