"""k_finalize_pair_wave (-m gpu): the two-car finalize as one-wave workgroups with the roles merged — the form a step takes when
it goes out as two env blocks.  step_groups=2 forces two blocks and therefore this form; a step_groups=1 twin runs
k_finalize_pair_roles and is the reference: every observable bit for bit.  Plus the oracle on the bench's inputs with in-step
re-seats, and the automatic choice of the block count just above 32 768 agents.
"""
import numpy as np
import pytest

from _util import load_map_image, oracle_map_dt, rel_err

pytestmark = pytest.mark.gpu

NORTH_STAR = 1e-5
FIELDS = ("scans", "state", "collisions", "collision_idx", "in_collision", "step_count")
AG = 12   # agents per one-wave workgroup (f110_kernels.hpp kFinalizeWaveAgents)


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


def blocks_pay(N, A):
    """f110_hip.hip env_blocks_pay, copied by hand: the sizes at which the automatic mode splits back-to-back steps.  (A copy
    cannot tell whether the rule is the right one — profiles/two_block_pair_sweep.txt is what says that — only that the
    library does what this copy says.)"""
    return not (A <= 4 and 2560 <= N <= 5120)


def room(side_px=400, wall_px=4, res=0.05):
    """an empty square room, 20 m across, centred on the origin: (image top row first, resolution, origin); the walls' inner
    faces are at +-(side_px / 2 - wall_px) * res = +-9.8 m"""
    img = np.full((side_px, side_px), 255, dtype=np.uint8)
    img[:wall_px] = 0
    img[-wall_px:] = 0
    img[:, :wall_px] = 0
    img[:, -wall_px:] = 0
    half = side_px * res / 2
    return img, res, [-half, -half, 0.0]


REACH = float(np.sqrt(0.58 ** 2 + 0.31 ** 2) + 1e-3)   # the pair test's centre-distance gate (default car)
FOV = 4.7
N_WALL = 24   # envs per wall scene: the last centimetres before the wall in steps of 4 mm, some of them inside the iTTC threshold


def placed_scenes():
    """[(name, (x0, y0, th0, v0), (x1, y1, th1, v1))]: one env of two cars per entry, placed in room()"""
    sc = []

    def rel(name, th0, dist, bearing, th1, x0=0.0, y0=0.0):
        sc.append((name, (x0, y0, th0, 0.0), (x0 + dist * np.cos(th0 + bearing), y0 + dist * np.sin(th0 + bearing), th1, 0.0)))

    rel("overlap", 0.3, 0.30, 0.4, 1.1)                       # the boxes overlap: the pair test hits
    rel("overlap_nose_tail", -2.0, 0.45, 0.0, -2.0)
    rel("reach_inside", 0.7, REACH * (1 - 1e-9), 2.0, 0.2)    # centres just inside / just outside reach (the boxes themselves apart)
    rel("reach_outside", 0.7, REACH * (1 + 1e-9), 2.0, 0.2)
    rel("reach_inside_ahead", -1.0, REACH * (1 - 1e-9), 0.0, -1.0 + np.pi / 2)
    rel("reach_outside_ahead", -1.0, REACH * (1 + 1e-9), 0.0, -1.0 + np.pi / 2)
    rel("behind", 1.3, 2.0, np.pi, 1.3)                       # directly behind: the window is empty
    rel("behind_close", 1.3, 0.9, np.pi, 0.1)
    for k, d in enumerate((0.9, 1.6, 3.0)):                   # straddling each end of the field of view
        rel("fov_left_%d" % k, 0.5 * k, d, FOV / 2, 0.5 * k + 0.8)
        rel("fov_right_%d" % k, -0.7 * k, d, -FOV / 2, 0.3)
    rel("ahead", 2.2, 1.5, 0.0, 2.2)                          # plain windows, near and far
    rel("ahead_far", 0.0, 6.0, 0.3, 1.0)
    for k in range(N_WALL):   # the ego drives into the wall (its heading is zeroed: the window is computed with theta = 0), the opponent watches
        x = 9.50 + 0.004 * k
        sc.append(("wall_%d" % k, (x, 1.0, 0.35, 8.0), (x - 1.4, 1.8, -0.3, 0.0)))
    for k in range(N_WALL):   # both cars of the env drive into the wall, side by side
        x = 9.50 + 0.004 * k
        sc.append(("both_%d" % k, (x, -3.0, 0.0, 8.0), (x - 0.002, -4.1, 0.0, 8.0)))
    return sc


def placed_batch(E):
    """E envs: the scenes, repeated with a shift so that each lands on other lanes of the one-wave workgroups and on both env blocks"""
    sc = placed_scenes()
    names, poses, vel = [], np.empty((E, 2, 3)), np.empty((E, 2))
    for e in range(E):
        name, c0, c1 = sc[(e + e // len(sc)) % len(sc)]
        names.append(name)
        poses[e, 0], poses[e, 1] = c0[:3], c1[:3]
        vel[e] = c0[3], c1[3]
    state = np.zeros((E * 2, 7))
    state[:, 0], state[:, 1], state[:, 4] = poses.reshape(-1, 3).T
    state[:, 3] = vel.reshape(-1)
    act = np.stack([np.zeros(E * 2), vel.reshape(-1)], axis=1)   # keep the speed: parked cars stay parked
    return names, poses.reshape(E * 2, 3), state, act


def _twins(amd, E, B, map_image, groups=(1, 2)):
    img, res, origin = map_image
    sims = []
    for g in groups:
        s = amd.BatchSim(num_envs=E, num_agents=2, num_beams=B, step_groups=g)
        s.set_map_image(img, res, origin)
        s.set_noise_rng(12345, 0.01)
        sims.append(s)
    return sims


def _same(sims, tag):
    outs = [s.get(*FIELDS) for s in sims]
    for kk in FIELDS:
        assert np.array_equal(outs[0][kk], outs[1][kk]), (kk, tag)
    return outs[1]


@pytest.mark.parametrize("B", [1080, 64])
@pytest.mark.parametrize("E", [1, 5, 13, 37])
def test_odd_env_counts_equal_one_block(amd, E, B):
    """a partly filled last workgroup, and a block boundary inside what one workgroup of 12 agents would hold: 120 steps of the
    bench's action sets from its start poses, noise on, every observable after every step"""
    from f1tenth_gym_amd import workload
    sims = _twins(amd, E, B, load_map_image("example_map"))
    assert sims[0].step_groups()[0] == 1 and sims[1].step_groups()[0] == (2 if E >= 2 else 1)
    poses = workload.start_poses(np.arange(E), 2)
    sets = workload.action_sets(6, E * 2, seed=1000)
    acts = []
    for s in sims:
        s.reset(poses)
        acts.append([s.device_array((E * 2, 2)) for _ in sets])
        for d, a in zip(acts[-1], sets):
            d.upload(a)
    for t in range(120):
        for s, da in zip(sims, acts):
            s.step_device(da[t // 20])
        o = _same(sims, t)
        assert sims[1].step_groups()[2] == (2 if E >= 2 else 1)
    assert (o["step_count"] == 120).all()
    for s in sims:
        s.close()


@pytest.mark.parametrize("B", [1080, 64])
def test_placed_poses_equal_one_block(amd, B):
    """the cases of the prologue, the pair test behind its wave-uniform skip and the window, one env each (placed_scenes), two
    steps: a hit, centres just inside and just outside reach, the opponent behind, across each end of the field of view, an ego
    crashed into the wall (window computed with theta = 0), both cars crashed"""
    E = 2 * len(placed_scenes()) + 5
    names, poses, state, act = placed_batch(E)
    sims = _twins(amd, E, B, room())
    for s in sims:
        s.reset(poses)
        s.set_state(state)
    acts = [s.device_array((E * 2, 2)) for s in sims]
    for step in range(2):
        for s, da in zip(sims, acts):
            da.upload(act)
            s.step_device(da)
        o = _same(sims, step)
        assert sims[1].step_groups()[2] == 2
        if step == 0:
            hit = (o["collision_idx"].reshape(E, 2) >= 0).all(axis=1)
            wall = o["in_collision"].reshape(E, 2) != 0
            by = lambda prefix: np.array([n.startswith(prefix) for n in names])
            assert hit[by("overlap")].all() and not hit[by("reach_outside")].any() and not hit[by("behind")].any() and not hit[by("fov")].any()
            assert not hit[by("reach_inside")].any()          # GJK ran (inside reach) and found the boxes apart
            assert wall[by("wall_"), 0].any() and not wall[by("wall_"), 1].any(), "no ego reached the wall: the scene does not exercise theta = 0"
            assert wall[by("both_")].all(axis=1).any(), "no env with both cars crashed"
            assert (o["state"].reshape(E, 2, 7)[wall][:, 4] == 0.0).all()
    for s in sims:
        s.close()


def test_two_blocks_with_reseats_vs_oracle(amd, orc):
    """bench.py's parity gate — its first 64 envs, 200 steps, its noise — stepped as two env blocks with finished envs re-seated
    inside the step's last kernel (the one-wave form's epilogue, its counter bumped from both streams): flags exact, floats within
    1e-5 of the oracle, the re-seat count equal to the one-block handle's and to the oracle's"""
    from f1tenth_gym_amd import workload
    E, A, T, B = 64, 2, 200, 1080
    img, res, origin = load_map_image("example_map")
    dt, _, _ = oracle_map_dt("example_map")
    noise = np.random.default_rng(12345).normal(0., 0.01, size=(T + 2, B))
    ref = orc.SimOracle(E, A, num_beams=B)
    ref.set_map_dt(dt, res, origin)
    ref.set_noise(noise)
    poses = workload.start_poses(workload.shard_envs(E, 0), A)
    sets = workload.action_sets((T + 19) // 20, E * A, seed=1000)
    sims = _twins(amd, E, B, (img, res, origin), groups=(2, 1))
    keep, acts, counts = [], [], []
    for s in sims:
        d = s.device_array((E * A, 3)); d.upload(poses); s.reset_device(d)
        c = s.device_array((1,), dtype=np.int32); c.upload(np.zeros(1, dtype=np.int32))
        s.set_auto_reseat(d, 0, c)
        keep.append(d); counts.append(c)
        acts.append([s.device_array((E * A, 2)) for _ in sets])
        for da, a in zip(acts[-1], sets):
            da.upload(a)
    ref.reset(poses)
    n_ref = 0
    for t in range(T):
        for s, da in zip(sims, acts):
            s.step_device(da[t // 20])
        ref.step(sets[t // 20], 8)
        col, wall = ref.collisions.copy(), ref.in_collision.copy()   # (the step's flags: the in-step re-seat keeps them, the oracle's reset clears the wall flag)
        mask = (col.reshape(E, A)[:, 0] != 0).astype(np.uint8)
        n_ref += int(mask.sum())
        ref.reset(poses, mask)
        if t % 8 == 7 or t == T - 1:
            o = sims[0].get("scans", "state", "collisions", "in_collision")
            assert np.array_equal(o["collisions"], col) and np.array_equal(o["in_collision"], wall), t
            es, er = rel_err(o["state"], ref.state), rel_err(o["scans"], ref.scans)
            assert es < NORTH_STAR and er < NORTH_STAR, (t, es, er)
            assert np.array_equal(o["scans"], sims[1].get("scans")["scans"]), t
            assert sims[0].step_groups()[2] == 2 and sims[1].step_groups()[2] == 1
    n = [int(c.download()[0]) for c in counts]
    assert n[0] == n[1] == n_ref and n_ref > 0, (n, n_ref)
    for s in sims:
        s.set_auto_reseat(None)
        s.close()


def test_automatic_rule_above_32768_agents(amd):
    """16 386 envs x 2 = 32 772 agents, the first size above the old one-block limit for two cars: three back-to-back
    f110_step_device calls on a handle in automatic mode end in the number of blocks env_blocks_pay gives for that size, and
    leave what a handle that never splits leaves"""
    E, B = 16386, 64
    sims = _twins(amd, E, B, room(), groups=(1, 0))
    groups, probes, _ = sims[1].step_groups()
    if groups < 2:
        pytest.skip("the stream probe found no second stream that runs beside the first (probes: %d)" % probes)
    rng = np.random.default_rng(31)
    p0 = np.stack([rng.uniform(-7.5, 7.5, E), rng.uniform(-7.5, 7.5, E), rng.uniform(-np.pi, np.pi, E)], axis=1)
    bearing, dist = rng.uniform(-np.pi, np.pi, E), rng.uniform(0.5, 2.0, E)   # some within reach, most in view
    p1 = np.stack([p0[:, 0] + dist * np.cos(bearing), p0[:, 1] + dist * np.sin(bearing), rng.uniform(-np.pi, np.pi, E)], axis=1)
    poses = np.stack([p0, p1], axis=1).reshape(E * 2, 3)
    act = np.stack([rng.uniform(-0.3, 0.3, E * 2), rng.uniform(0.0, 3.0, E * 2)], axis=1)
    acts = []
    for s in sims:
        s.reset(poses)
        acts.append(s.device_array((E * 2, 2)))
        acts[-1].upload(act)
    for s, da in zip(sims, acts):
        for _ in range(3):
            s.step_device(da)
    assert sims[0].step_groups()[2] == 1
    assert sims[1].step_groups()[2] == (2 if blocks_pay(E * 2, 2) else 1)
    o = _same(sims, "three steps")
    assert (o["collision_idx"] >= 0).any() and (o["step_count"] == 3).all()
    for s in sims:
        s.close()
