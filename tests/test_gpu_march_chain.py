"""march_padded's rewritten loop (give-up decision as a per-lane range limit, boundary case behind one wave-uniform branch) on the
device, through every launch form that runs it: cars parked with their lidars on the inputs that take its rare paths — cell corners
and edges with axis-aligned headings, a beam along y = const, lidars on, just off and far off the map — scans array_equal to the
oracle, lookup totals equal where the library counts them; then a short noisy rollout with in-place resets.  The host twin is
tests/test_host_march_chain.py."""
import numpy as np
import pytest

from _util import bench_start_poses, map_stem, oracle_map_dt
from test_host_march_chain import FOV, rotated_sub_map, to_world

pytestmark = pytest.mark.gpu
E, A = 3, 2          # 6 agents: 102 tasks at 1080 beams (17 per agent, the last one 56 beams), waves of 3 tasks that straddle two agents
FAR, FAR_B = [1e9, -1e9, 1.0], [-1e9, 1e9, 1.0]      # two lidars off every map and out of each other's sight


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


def parked_poses(dt, res, origin, seed, cells=4, randoms=8):
    """the pose families of tests/test_host_march_chain.py with headings in [0, 2 pi] (a car at rest keeps such a pose through a
    zero-action step bit for bit).  lidar_dist is 0 in every sim below, so the LIDAR is what sits on the corner."""
    rng = np.random.default_rng(seed)
    H, W = dt.shape
    free = np.argwhere(dt > 0.3)
    yaw = origin[2] % (2 * np.pi)
    poses = []
    for r, c in free[rng.choice(len(free), cells, replace=False)]:
        poses.append(list(to_world(origin, c * res, r * res)) + [(yaw + rng.choice([0.0, np.pi / 2, np.pi, 3 * np.pi / 2])) % (2 * np.pi)])
        poses.append(list(to_world(origin, c * res, (r + 0.5) * res)) + [yaw])
        poses.append(list(to_world(origin, (c + 0.25) * res, r * res)) + [FOV / 2 + 1e-5])     # beam 0 along y = const (yaw 0)
        poses.append(list(to_world(origin, (c + rng.uniform()) * res, (r + rng.uniform()) * res)) + [rng.uniform(0, 2 * np.pi)])
    for r, c in free[rng.choice(len(free), randoms, replace=False)]:
        poses.append(list(to_world(origin, (c + rng.uniform()) * res, (r + rng.uniform()) * res)) + [rng.uniform(0, 2 * np.pi)])
    poses += [list(to_world(origin, 0.0, 0.0)) + [0.3], list(to_world(origin, -1.0, H * res / 2)) + [0.0],
              list(to_world(origin, W * res + 2.5, H * res + 2.5)) + [3.9], list(to_world(origin, -40.0, -40.0)) + [0.8],
              list(to_world(origin, W * res / 2, H * res + 29.0)) + [2 * np.pi - 1.6], [1e9, -1e9, 1.0], [1e300, 0.0, 0.0]]
    return np.asarray(poses)


class Parked(object):
    """poses of one map paired into envs of two cars that cannot see each other (the opponent ray-cast leaves the scan alone: the
    expectation is the map's own scan), with the oracle's scans and lookup total"""

    def __init__(self, orc, dt, res, origin, seed, beams=1080):
        self.dt, self.res, self.origin, self.beams = np.ascontiguousarray(dt), res, origin, beams
        so = orc.ScanOracle(beams, FOV)
        so.set_map_dt(self.dt, res, origin)
        poses = parked_poses(self.dt, res, origin, seed)
        half = (len(poses) + 1) // 2
        pair = orc.SimOracle(1, 2, num_beams=beams)
        pair.set_map_dt(self.dt, res, origin)
        envs = []
        for i in range(half):
            duo = np.asarray([poses[i], poses[i + half] if i + half < len(poses) else FAR])
            pair.reset(duo)
            pair.step(np.zeros((2, 2)))
            alone = np.asarray([so.scan(p) for p in duo])
            if np.array_equal(pair.scans, alone):
                envs.append(duo)
            else:        # they see each other: each gets a partner far away instead
                envs += [np.asarray([duo[0], FAR]), np.asarray([FAR, duo[1]])]
        while len(envs) % E:
            envs.append(np.asarray([FAR, FAR_B]))
        self.batches = [np.concatenate(envs[k:k + E]) for k in range(0, len(envs), E)]      # [E * A][3] each
        self.scans, self.row_lookups = [], []
        for batch in self.batches:
            rows, lk = [], []
            for p in batch:
                rows.append(so.scan(p))
                lk.append(so.last_lookups)
            self.scans.append(np.asarray(rows))
            self.row_lookups.append(np.asarray(lk, dtype=np.int64))
        self.lookups = int(np.sum(self.row_lookups))


def run_parked(sim, fam, count=True, groups=None):
    """every batch through sim.step with the cars at rest; scans array_equal; then once more with the lookup counter on (other
    instantiations of the same kernels)"""
    for counting in ((False, True) if count else (False,)):
        if counting:
            sim.scan_lookup_count(enable=True, read=True)
        for batch, want in zip(fam.batches, fam.scans):
            sim.reset(batch)
            sim.step(np.zeros((E * A, 2)))
            o = sim.get("scans", "state")
            assert np.array_equal(o["state"][:, [0, 1, 4]], batch) and not o["state"][:, 3].any()     # parked where they were put
            bad = np.argwhere(o["scans"] != want)
            assert bad.size == 0, (counting, len(bad), bad[:4], batch[bad[0][0]])
            if groups is not None:
                assert sim.step_groups()[2] == groups
        if counting:
            assert sim.scan_lookup_count(enable=False) == fam.lookups


@pytest.fixture(scope="module")
def families(orc):
    return {name: Parked(orc, *oracle_map_dt(name), seed=k) for k, name in enumerate(("berlin", "example_map", "skirk"))}


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("mapname", ["berlin", "example_map", "skirk"])
def test_agent_aligned_scan(amd, families, mapname, groups):
    """1080 beams, PADDED layout: k_scan_rays_agent, as one env block and as two"""
    fam = families[mapname]
    s = amd.BatchSim(num_envs=E, num_agents=A, map_layout=3, step_groups=groups)
    s.set_map_dt(fam.dt, fam.res, fam.origin)
    s.set_noise_off()
    run_parked(s, fam, groups=groups)
    s.close()


def test_rays_not_agent_aligned(amd, orc):
    """100 beams: k_scan_rays"""
    fam = Parked(orc, *oracle_map_dt("skirk"), seed=5, beams=100)
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=100, map_layout=3)
    s.set_map_dt(fam.dt, fam.res, fam.origin)
    s.set_noise_off()
    run_parked(s, fam)
    s.close()


def test_rowmajor_layout(amd, families):
    """layout 0: the plain march, untouched — the same expectations hold for it"""
    fam = families["berlin"]
    s = amd.BatchSim(num_envs=E, num_agents=A, map_layout=0)
    s.set_map_dt(fam.dt, fam.res, fam.origin)
    s.set_noise_off()
    run_parked(s, fam)
    s.close()


def test_more_beams_than_directions(amd, orc):
    """4096 beams: k_scan_dirs_agent marches each distinct table direction once (its lookup total is not the oracle's per-beam one)"""
    fam = Parked(orc, *oracle_map_dt("example_map"), seed=6, beams=4096)
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=4096, map_layout=3)
    s.set_map_dt(fam.dt, fam.res, fam.origin)
    s.set_noise_off()
    run_parked(s, fam, count=False)
    s.close()


def test_per_env_maps(amd, families):
    """two map slots, envs 0 and 2 on berlin and env 1 on skirk: the PER_ENV_MAP instantiations"""
    fa, fb = families["berlin"], families["skirk"]
    s = amd.BatchSim(num_envs=E, num_agents=A, map_layout=3)
    s.set_map_dt(fa.dt, fa.res, fa.origin)
    assert s.add_map_dt(fb.dt, fb.res, fb.origin) == 1
    s.set_env_maps([0, 1, 0])
    s.set_noise_off()
    n = min(len(fa.batches), len(fb.batches))
    for counting in (False, True):
        lookups = 0
        if counting:
            s.scan_lookup_count(enable=True, read=True)
        for k in range(n):
            batch = np.concatenate([fa.batches[k][:A], fb.batches[k][A:2 * A], fa.batches[k][2 * A:]])
            want = np.concatenate([fa.scans[k][:A], fb.scans[k][A:2 * A], fa.scans[k][2 * A:]])
            lookups += int(fa.row_lookups[k][:A].sum() + fb.row_lookups[k][A:2 * A].sum() + fa.row_lookups[k][2 * A:].sum())
            s.reset(batch)
            s.step(np.zeros((E * A, 2)))
            got = s.get("scans")["scans"]
            bad = np.argwhere(got != want)
            assert bad.size == 0, (counting, k, len(bad), bad[:4])
        if counting:
            assert s.scan_lookup_count(enable=False) == lookups
    s.close()


def test_rotated_origin(amd, orc):
    """an origin with a yaw: the IDENT = false instantiations"""
    dt, res, origin = rotated_sub_map()
    fam = Parked(orc, dt, res, origin, seed=7)
    s = amd.BatchSim(num_envs=E, num_agents=A, map_layout=3)
    s.set_map_dt(fam.dt, fam.res, fam.origin)
    s.set_noise_off()
    run_parked(s, fam)
    s.close()


def test_one_env_one_launch_step(amd, families):
    """one env of two cars through F110Env.step: k_step_tiny"""
    fam = families["berlin"]
    env = amd.F110Env(map=map_stem("berlin"), map_ext=".png", num_agents=2)
    env.sim.batch.set_noise_off()
    assert np.array_equal(env.sim.batch.get_map_dt(), fam.dt)
    for batch, want in zip(fam.batches, fam.scans):
        for e in range(E):
            obs, _, _, _ = env.reset(batch[e * A:(e + 1) * A])       # (reset advances one zero-action step)
            assert env.sim.batch.step_launches() == 1
            assert np.array_equal(np.asarray(obs["scans"]), want[e * A:(e + 1) * A]), (e, batch[e * A:(e + 1) * A])
    env.sim.batch.close()


def run_rollout(amd, orc, gap_wp):
    """40 steps of the bench's random actions on 8 envs of two cars (the second one gap_wp raceline waypoints behind the first),
    seed-12345 noise from the device generator, envs re-seated in place every fifth step (the ones whose ego crashed and three
    more in turn) — next to orc.SimOracle.  Per step: whether flags and state are the oracle's, the scans of both, the beams
    whose ray meets the other car's body (the only ones the opponent ray-cast can rewrite) and whether it rewrote any."""
    n_envs, T = 8, 40
    dt, res, origin = oracle_map_dt("example_map")
    s = amd.BatchSim(num_envs=n_envs, num_agents=A, map_layout=3)
    s.set_map_dt(dt, res, origin)
    s.set_noise_rng(12345, 0.01)
    ref = orc.SimOracle(n_envs, A)
    ref.set_map_dt(dt, res, origin)
    ref.set_noise(np.random.default_rng(12345).normal(0., 0.01, size=(T + 1, 1080)))
    poses = bench_start_poses(n_envs, A, gap_wp=gap_wp)
    s.reset(poses)
    ref.reset(poses)
    from f1tenth_gym_amd import workload
    sets = workload.action_sets(T // 20, n_envs * A, 0)      # bench.py's random policy: a new set every 20 steps
    steps, n_reset = [], 0
    for t in range(T):
        s.step(sets[t // 20])
        ref.step(sets[t // 20])
        o = s.get("scans", "state", "collisions", "in_collision")
        body = np.zeros((n_envs * A, 1080), dtype=bool)
        rewritten = False
        for i in range(n_envs * A):
            far = np.full(1080, 1e9)
            to_body = orc.ray_cast(ref.agent_poses[i], far, s.scan_angles, orc.get_vertices(ref.agent_poses[i ^ 1], s.params['length'], s.params['width']))
            body[i] = to_body != far
            rewritten |= bool(np.any(to_body[body[i]] <= ref.scans[i][body[i]]))      # (a rewritten beam holds the distance to the body)
        steps.append(dict(t=t, flags=(np.array_equal(o["collisions"], ref.collisions), np.array_equal(o["in_collision"], ref.in_collision)),
                          state=np.array_equal(o["state"], ref.state), got=o["scans"], want=ref.scans.copy(), body=body, rewritten=rewritten))
        if t % 5 == 4:
            mask = (ref.collisions.reshape(n_envs, A)[:, 0] != 0) | ((np.arange(n_envs) + t // 5) % 3 == 0)
            mask = mask.astype(np.uint8)
            n_reset += int(mask.sum())
            s.reset(poses, mask)
            ref.reset(poses, mask)
    s.close()
    assert n_reset >= 8 * 2
    return steps


def test_noisy_rollout_scans_array_equal(amd, orc):
    """flags exact, EVERY scan value array_equal to orc.SimOracle — with the two cars of an env half a lap apart (390 of the
    raceline's 783 waypoints), where walls stand between them and the opponent ray-cast rewrites no beam (checked on the oracle):
    every value is the march's and the noise generator's"""
    steps = run_rollout(amd, orc, 390)
    for st in steps:
        assert not st["rewritten"], st["t"]
        assert st["flags"] == (True, True) and st["state"], st["t"]
        assert np.array_equal(st["got"], st["want"]), (st["t"], np.argwhere(st["got"] != st["want"])[:4])


def test_noisy_rollout_cars_in_sight(amd, orc):
    """the same with the bench's own start poses, the second car six waypoints behind the first: flags and state exact, every
    beam that cannot meet the other car's body array_equal.  The beams that do meet it come out of the opponent ray-cast, which
    evaluates sin / cos on the device (an ulp from libm, tests/test_gpu_round2.py) and which this change does not reach: on an
    MI355X 2 - 15 of the 17 280 values of a step differ from the oracle's by one or two ulp (at most 3.3e-16), before this change
    and after it alike, all of them such beams (profiles/march_chain_rollout_ulp.txt) — held to that suite's 1e-12 relative"""
    steps = run_rollout(amd, orc, 6)
    for st in steps:
        assert st["flags"] == (True, True) and st["state"], st["t"]
        diff = st["got"] != st["want"]
        assert not (diff & ~st["body"]).any(), (st["t"], np.argwhere(diff & ~st["body"])[:4])
        assert np.all(np.abs(st["got"] - st["want"])[diff] <= 1e-12 * np.abs(st["want"])[diff] + 1e-12), st["t"]
    assert any(st["rewritten"] for st in steps) and sum(int(st["body"].sum()) for st in steps) > 1000      # the split above is not vacuous
