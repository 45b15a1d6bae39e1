"""The reference against the oracle on seeded random inputs that are in no other fixture.

The reference's side was recorded by RUNNING it (oracle/refshim/gen_fuzz_golden.py, build container only) into
tests/golden/reference_fuzz_{scan,sim,env,units}.npz: inputs it drew from its own maps (poses in free space, start
clusters), the actions it was given and every output it returned.  Here the oracle runs the same inputs and is held to
those outputs with the same tolerances as against the live reference.  oracle/refshim/fuzz_live.py runs these checks
on random configurations against the live reference instead.  The sweep walks the reference's public surface around
the other fixtures:

  * `ScanSimulator2D(num_beams, fov, eps, theta_dis, max_range)` (laser_models.py:360-381) with every
    argument away from its default, on every shipped track and on yaml files with a rotated origin
    and resolutions that are not powers of two (laser_models.py:55-86 xy_2_rc, :429-454 scan);
  * `Simulator` (base_classes.py:451-630) with random vehicle parameters, 1-6 cars, either integrator,
    time steps, lidar offsets, seeds and tracks.
"""
import hashlib
import os

import numpy as np
import pytest

from _util import GOLD, MAPS, rel_err
from oracle import orc

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_MAPS = os.path.join(os.path.dirname(HERE), "f1tenth_gym_amd", "maps")
# The reference's single-track model is unstable for some inputs (driving backwards with a light, grippy car is one): yaw
# and yaw rate run past 1e6 within a few steps.  From there sin / cos of the yaw amplify the 1-ulp differences between C's
# libm and NumPy's own kernels without bound — the state still agrees to 1e-12 RELATIVE while the scan directions no
# longer do.  So: everything is compared at every step as before, and a rollout whose |state| has passed DIVERGED is compared
# up to its first difference instead of failing on it (the GPU fuzzers in tools/debug stop at the divergence itself).  The
# hand-written cases below that get there (the reversing env episodes do) still agree to the end;
# oracle/refshim/fuzz_live.py's random ones nearly always do.
DIVERGED = 1e6


def map_files(name):
    """(yaml path, png path) of a track: tests/golden/maps or the package's copy of the reference's maps"""
    for d in (MAPS, PKG_MAPS):
        if os.path.isfile(os.path.join(d, name + ".yaml")) and os.path.isfile(os.path.join(d, name + ".png")):
            return os.path.join(d, name + ".yaml"), os.path.join(d, name + ".png")
    raise FileNotFoundError(name)


def dt_digest(dt):
    """pins a distance table bit for bit (the fixtures hold the reference's, not the 20 MB tables themselves)"""
    dt = np.ascontiguousarray(dt, dtype=np.float64)
    return np.frombuffer(hashlib.sha256(repr(dt.shape).encode() + dt.tobytes()).digest(), dtype=np.uint8)


def oracle_dt(name, resolution, ref_digest):
    """the oracle's EDT of a track's image at `resolution` (pinned against scipy in test_oracle_golden.py); it must be the
    very table the reference computed for the same image"""
    from PIL import Image
    img = np.array(Image.open(map_files(name)[1]))
    dt = orc.map_dt_from_image(img, resolution)
    assert np.array_equal(dt_digest(dt), ref_digest), "the oracle's distance table differs from the reference's"
    return dt


def row_digests(scans):
    """SHA-256 of every scan row (the last axis) of a float64 array: [..., 32] uint8"""
    scans = np.ascontiguousarray(scans, dtype=np.float64)
    flat = scans.reshape(-1, scans.shape[-1])
    return np.array([np.frombuffer(hashlib.sha256(r.tobytes()).digest(), dtype=np.uint8) for r in flat]).reshape(scans.shape[:-1] + (32,))


def reference_scans(rec, t, got):
    """the reference's scans [A, B] of step t.  A live record holds them as they are.  A fixture holds a digest of every row
    plus the values of the beams the oracle did not reproduce bit for bit when it was recorded (flat indices into [T, A, B]):
    the other beams are taken from `got` (the oracle's scans of the step), and the row digests decide whether they are the
    reference's own values — so the reference is pinned exactly on every beam and no row is stored whole."""
    if "scans" in rec:
        return rec["scans"][t]
    A, B = got.shape
    idx, val = rec["scan_beams"], rec["scan_values"]
    lo, hi = np.searchsorted(idx, [t * A * B, (t + 1) * A * B])
    ref = np.array(got, dtype=np.float64)
    ref.reshape(-1)[idx[lo:hi] - t * A * B] = val[lo:hi]
    assert np.array_equal(row_digests(ref), rec["scan_sha256"][t]), ("scans of step %d differ from the reference's beyond its stored beams" % t)
    return ref


def record(kind, idx):
    """the recorded reference run of case `idx` of a sweep: {field: array}"""
    z = np.load(os.path.join(GOLD, "reference_fuzz_%s.npz" % kind))
    pre = "%s%d_" % (kind, idx)
    rec = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
    assert rec, "no recorded reference run for %s case %d: regenerate with oracle/refshim/gen_fuzz_golden.py" % (kind, idx)
    return rec


def params_dict(vec):
    return dict(zip(orc.PARAM_KEYS, (float(v) for v in vec)))


SCAN_CASES = [
    # map, resolution override, origin override, num_beams, fov, eps, theta_dis, max_range
    ("example_map", None, None, 257, 4.7, 1e-4, 2000, 30.0),
    ("example_map", None, None, 180, 4.7, 0.03, 720, 8.0),
    ("example_map", None, None, 333, 6.1, 0.2, 3600, 30.0),
    ("berlin", None, None, 200, 4.7, 0.03, 2000, 8.0),
    ("berlin", None, None, 1080, 4.7, 0.2, 720, 30.0),
    ("skirk", None, None, 211, 3.3, 1e-4, 3600, 8.0),
    ("vegas", None, None, 240, 4.7, 0.03, 2000, 30.0),
    ("stata_basement", None, None, 150, 4.7, 0.2, 720, 8.0),
    ("berlin", 0.07, [-3.0, -4.0, 0.3], 190, 4.7, 1e-4, 2000, 30.0),
    ("skirk", 0.0437, [1.5, 2.5, -1.1], 222, 5.0, 0.03, 3600, 8.0),
    ("example_map", 0.11, [-40.0, -20.0, 2.4], 160, 4.7, 0.2, 720, 30.0),
    ("vegas", 0.05, [-11.6, -27.3, 0.0], 2100, 6.2, 1e-4, 2000, 30.0),   # more beams than table directions
]


def check_scan_case(case, idx, rec):
    """the oracle's ScanOracle against a recorded ScanSimulator2D run of SCAN_CASES-style `case` (index `idx`)"""
    name, _, _, beams, fov, eps, theta_dis, max_range = case
    res, origin = float(rec["resolution"]), rec["origin"]
    so = orc.ScanOracle(beams, fov, eps=eps, theta_dis=theta_dis, max_range=max_range)
    so.set_map_dt(oracle_dt(name, res, rec["dt_sha256"]), res, origin)
    assert so.cfg.theta_index_increment == rec["theta_index_increment"]
    assert len(rec["poses"]) >= 2
    for pose, want in zip(rec["poses"], rec["scans"]):
        got = so.scan(pose)
        assert np.array_equal(got, want), (idx, pose, float(np.max(np.abs(got - want))))
    # noise path: scan(pose, rng, std_dev) draws rng.normal(0, std_dev, num_beams) (laser_models.py:450-452)
    std = [0.01, 0.05, 0.2][idx % 3]
    got = so.scan(rec["poses"][0]) + np.random.default_rng(idx).normal(0., std, size=beams)
    assert np.array_equal(got, rec["noisy_scan"])


@pytest.mark.parametrize("case", range(len(SCAN_CASES)))
def test_scan_simulator_ctor_and_map_sweep(case):
    check_scan_case(SCAN_CASES[case], case, record("scan", case))


SIM_CASES = [
    # map, resolution override, origin override, agents, integrator, time_step, lidar_dist, steps
    ("example_map", None, None, 1, "RK4", 0.01, 0.0, 40),
    ("example_map", None, None, 3, "Euler", 0.005, 0.1, 30),
    ("berlin", None, None, 2, "RK4", 0.02, 0.275, 40),
    ("skirk", None, None, 4, "RK4", 0.01, 0.0, 25),
    ("vegas", None, None, 2, "RK4", 0.01, 0.0, 40),
    ("berlin", 0.07, [-3.0, -4.0, 0.3], 2, "RK4", 0.01, 0.0, 40),
    ("example_map", None, None, 6, "RK4", 0.015, 0.05, 20),
    ("stata_basement", None, None, 5, "Euler", 0.01, 0.2, 20),
]


def check_sim_case(case, idx, rec, oracle_scans=None):
    """the oracle's SimOracle against a recorded Simulator rollout of SIM_CASES-style `case` (index `idx`); the oracle's scans of
    every step compared are appended to `oracle_scans` if given"""
    name, _, _, A, integ, time_step, lidar_dist, _ = case
    acts = rec["actions"]
    T = len(acts)
    res, origin = float(rec["resolution"]), rec["origin"]
    o = orc.SimOracle(1, A, params=params_dict(rec["params"]), time_step=time_step, integrator={"RK4": 1, "Euler": 2}[integ], lidar_dist=lidar_dist)
    o.set_map_dt(oracle_dt(name, res, rec["dt_sha256"]), res, origin)
    if int(rec["own_params_agent"]) >= 0:     # Simulator.update_params(params, agent_idx) base_classes.py:503-519: one slot gets its own car
        o.set_params(params_dict(rec["own_params"]), int(rec["own_params_agent"]))
    o.set_noise(np.random.default_rng(int(rec["seed"])).normal(0., 0.01, size=(T, 1080)))
    o.reset(rec["start"])
    worst_state = worst_scan = 0.0
    diverged_at = stopped_at = None
    seen = {"wall": 0, "gjk": 0}
    for t in range(T):
        o.step(acts[t])
        if oracle_scans is not None:
            oracle_scans.append(o.scans.copy())
        if diverged_at is None and np.abs(o.state).max() > DIVERGED:
            diverged_at = t
        try:
            assert np.array_equal(o.collisions, rec["collisions"][t]), (idx, t)
            assert np.array_equal(o.collision_idx, rec["collision_idx"][t]), (idx, t)
            assert np.array_equal(o.in_collision, rec["in_collision"][t]), (idx, t)
            es, ec = rel_err(o.state, rec["state"][t]), rel_err(o.scans, reference_scans(rec, t, o.scans))
            assert es < 1e-9 and ec < 1e-9, (idx, t, es, ec)
        except AssertionError as ex:
            if diverged_at is None:
                raise
            print("case %d: the reference's dynamics diverged at step %d (|state| > 1e6); first difference at step %d %s: compared up to it" % (idx, diverged_at, t, str(ex)[:100]))
            stopped_at = t
            break
        worst_state, worst_scan = max(worst_state, es), max(worst_scan, ec)
        seen["wall"] += int(o.in_collision.any()); seen["gjk"] += int((o.collision_idx >= 0).any())
    assert worst_state < 1e-9 and worst_scan < 1e-9, (idx, worst_state, worst_scan)
    print("case %d: %s A=%d wall-hit steps %d, contact steps %d, state err %.1e scan err %.1e%s" % (
        idx, name, A, seen["wall"], seen["gjk"], worst_state, worst_scan,
        "" if diverged_at is None else " (dynamics diverged at step %d; compared %s)" % (diverged_at, "to the end" if stopped_at is None else "up to step %d" % stopped_at)))


@pytest.mark.parametrize("case", range(len(SIM_CASES)))
def test_simulator_sweep(case):
    check_sim_case(SIM_CASES[case], case, record("sim", case))


ENV_CASES = [
    # map name (None = the env's own default: vegas), agents, ego_idx, integrator, timestep, lidar_dist, steps
    (None, 2, 0, "RK4", 0.01, 0.0, 110),
    ("example_map", 1, 0, "Euler", 0.02, 0.1, 260),
    ("berlin", 3, 2, "RK4", 0.01, 0.275, 60),
    ("skirk", 2, 1, "RK4", 0.02, 0.0, 70),
    # an optional 8th field "circle": full lock forwards instead of back and forth through the start zone — laps complete without
    # the reversing that the reference's dynamics rarely survive, so the floats are compared through the lap count's changes too
    (None, 1, 0, "RK4", 0.02, 0.0, 190, "circle"),
]


def check_env_case(case, idx, rec, oracle_scans=None):
    """the oracle's Simulator under the package's host lap logic (`f1tenth_gym_amd.env._LapLogic`, what F110Env / F110VecEnv's
    host path run) against a recorded F110Env episode of ENV_CASES-style `case` (index `idx`); the oracle's scans of every step
    compared are appended to `oracle_scans` if given"""
    from f1tenth_gym_amd.env import _LapLogic
    name, A, ego, integ, ts, ld, _ = case[:7]
    acts = rec["actions"]       # [k] = what env.step got at step k; [0] = reset's zero-action step
    T = int(rec["steps"])
    res, origin = float(rec["resolution"]), rec["origin"]
    o = orc.SimOracle(1, A, params=params_dict(rec["params"]), time_step=ts, integrator={"RK4": 1, "Euler": 2}[integ], lidar_dist=ld)
    o.set_map_dt(oracle_dt(name or "vegas", res, rec["dt_sha256"]), res, origin)
    o.set_noise(np.random.default_rng(int(rec["seed"])).normal(0., 0.01, size=(T + 2, 1080)))
    start = rec["start"]
    lap = _LapLogic(1, A, ego)
    o.reset(start)
    lap.reset(start.reshape(1, A, 3))
    worst = 0.0
    diverged_at = stopped_at = None
    done = False
    for k in range(len(acts)):
        o.step(acts[k])
        if oracle_scans is not None:
            oracle_scans.append(o.scans.copy())
        st = o.state
        if diverged_at is None and np.abs(st).max() > DIVERGED:
            diverged_at = k
        d, ckpt = lap.update(st[:, 0], st[:, 1], o.collisions, ts)
        done = bool(rec["done"][k])
        assert rec["reward"][k] == ts and rec["ego_idx"][k] == 0
        try:
            err = max(rel_err(np.stack([st[:, 0], st[:, 1], st[:, 4], st[:, 3], st[:, 5]]),
                              np.stack([rec["poses_x"][k], rec["poses_y"][k], rec["poses_theta"][k], rec["linear_vels_x"][k], rec["ang_vels_z"][k]])),
                      rel_err(o.scans, reference_scans(rec, k, o.scans)))
            assert err < 1e-9, (idx, k, err)
            assert np.array_equal(o.collisions, rec["collisions"][k]), (idx, k)
            assert np.array_equal(lap.toggle_list[0], rec["toggle_list"][k]) and np.array_equal(lap.near_starts[0], rec["near_starts"][k]), (idx, k)
            assert np.array_equal(lap.lap_counts[0], rec["lap_counts"][k]) and np.array_equal(ckpt[0], rec["checkpoint_done"][k]), (idx, k)
            assert np.max(np.abs(lap.lap_times[0] - rec["lap_times"][k])) < 1e-12
            assert bool(d[0]) == done, (idx, k)
        except AssertionError as ex:
            if diverged_at is None:
                raise
            print("env case %d: the reference's dynamics diverged at step %d (|state| > 1e6); first difference at step %d %s: compared up to it" % (idx, diverged_at, k, str(ex)[:100]))
            stopped_at = k
            break
        worst = max(worst, err)
    assert done or len(acts) == T + 1, (idx, len(acts), T)
    assert worst < 1e-9, (idx, worst)
    print("env case %d: %s A=%d ego=%d: %d steps, toggles %s, collisions %s, done %s%s" % (
        idx, name or "vegas (default)", A, ego, len(acts) - 1, rec["toggle_list"][-1], rec["collisions"][-1], done,
        "" if diverged_at is None else " (dynamics diverged at step %d; compared %s)" % (diverged_at, "to the end" if stopped_at is None else "up to step %d" % stopped_at)))


@pytest.mark.parametrize("case", range(len(ENV_CASES)))
def test_f110env_sweep(case):
    """the reference F110Env (f110_env.py:104-349: constructor keywords, reset's zero-action step, _check_done's start-zone
    toggles in the EGO's start frame, lap counts / times, done on the ego's collision) against the oracle on random keywords,
    starts and actions"""
    check_env_case(ENV_CASES[case], case, record("env", case))


def random_params(rng):
    p = dict(zip(orc.PARAM_KEYS, orc.params_vec(None)))
    scale = {"mu": (0.6, 1.3), "C_Sf": (0.8, 1.2), "C_Sr": (0.8, 1.2), "lf": (0.9, 1.15), "lr": (0.9, 1.15), "h": (0.8, 1.3),
             "m": (0.8, 1.3), "I": (0.8, 1.4), "a_max": (0.6, 1.1), "sv_max": (0.6, 1.2), "v_switch": (0.6, 1.2),
             "width": (0.8, 1.3), "length": (0.85, 1.25)}
    for k, (lo, hi) in scale.items():
        p[k] = float(p[k] * rng.uniform(lo, hi))
    p["mu"] = float(rng.uniform(0.6, 1.3))
    p["sv_min"] = -p["sv_max"]
    p["v_max"] = float(rng.uniform(9.0, 20.0))
    return p


UNIT_N = 250


def unit_inputs(seed, n=UNIT_N):
    """the unit sweep's random inputs (a pure function of the seed: the generator and this test draw the same ones).
    Vertices are not drawn: they are what the reference's get_vertices made of the drawn poses (recorded)."""
    rng = np.random.default_rng(11000 + seed)
    d = {"params": [], "x": [], "u": [], "q": [], "LW": [], "pa": [], "pb": [], "multi_k": [], "multi_poses": []}
    # --- dynamics: random parameter sets and states on both sides of every switch
    for i in range(n):
        p = random_params(rng)
        x = np.array([rng.uniform(-50, 50), rng.uniform(-50, 50), rng.uniform(-0.45, 0.45), rng.choice([rng.uniform(-3, 20), rng.uniform(-0.6, 0.6)]),
                      rng.uniform(-7, 7), rng.uniform(-4, 4), rng.uniform(-0.6, 0.6)])
        if i % 7 == 0:
            x[2] = rng.choice([p["s_min"], p["s_max"]])     # on a steering limit
        u = np.array([rng.uniform(-4, 4), rng.uniform(-12, 12)])
        q = (rng.uniform(-6, 22), rng.uniform(-0.5, 0.5), rng.uniform(-6, 22), rng.uniform(-0.5, 0.5))
        if i % 5 == 0:
            q = (q[0], q[3] + rng.choice([0.0, 1e-5, -1e-5, 2e-4]), q[2], q[3])      # around the steering dead band
        d["params"].append(orc.params_vec(p)); d["x"].append(x); d["u"].append(u); d["q"].append(q)
    # --- collision: car-sized quadrilaterals near and through each other
    for i in range(n):
        L, W = rng.uniform(0.4, 0.7), rng.uniform(0.2, 0.4)
        pa = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-7, 7)])
        pb = pa + np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.8, 0.8), rng.uniform(-3.2, 3.2)])
        d["LW"].append((L, W)); d["pa"].append(pa); d["pb"].append(pb)
        if i % 10 == 0:
            k = int(rng.integers(2, 7))
            poses = np.zeros((6, 3))
            for j in range(k):
                poses[j] = pa + np.array([rng.uniform(-1.2, 1.2), rng.uniform(-1.2, 1.2), rng.uniform(-3, 3)])
            d["multi_k"].append(k); d["multi_poses"].append(poses)
    # --- ttc, get_range, blocked view, ray_cast on random scans, speeds and opponents
    m = max(10, n // 6)
    d.update(scan=[], vel=[], ego=[], opp=[], base=[], theta=[])
    for i in range(m):
        d["scan"].append(rng.uniform(0.05, 12.0, 1080))
        d["vel"].append(rng.choice([rng.uniform(-3, 20), 0.0, rng.uniform(20, 400)]))
        ego = np.array([rng.uniform(-3, 3), rng.uniform(-3, 3), rng.uniform(-3.1, 3.1)])
        d["ego"].append(ego)
        d["opp"].append(ego + np.array([rng.uniform(-4, 4), rng.uniform(-4, 4), rng.uniform(-3, 3)]))
        d["base"].append(rng.uniform(0.5, 30.0, 1080))
        d["theta"].append([rng.uniform(-7, 7) for _ in range(8)])
    d = {k: np.asarray(v) for k, v in d.items()}
    h = hashlib.sha256()
    for k in sorted(d):
        h.update(k.encode() + np.ascontiguousarray(d[k], dtype=np.float64).tobytes())
    d["sha256"] = np.frombuffer(h.digest(), dtype=np.uint8)
    return d


UNIT_BEAMS, UNIT_FOV, UNIT_TTC = 1080, 4.7, 0.005


def check_unit_functions(seed, rec):
    """the oracle's unit functions against the reference's recorded answers on unit_inputs(seed)"""
    d = unit_inputs(seed)
    assert np.array_equal(d["sha256"], rec["inputs_sha256"]), "the drawn inputs are not the recorded ones"
    n = len(d["x"])
    # --- dynamics
    for i in range(n):
        pv, x, u, q = d["params"][i], d["x"][i], d["u"][i], d["q"][i]
        p = params_dict(pv)
        assert rel_err(orc.vehicle_dynamics_st(x, u, pv), rec["st"][i]) < 1e-12, (seed, i)
        assert rel_err(orc.vehicle_dynamics_ks(x[:5], u, pv), rec["ks"][i]) < 1e-12, (seed, i)
        assert np.array_equal(orc.pid(q[0], q[1], q[2], q[3], p["sv_max"], p["a_max"], p["v_max"], p["v_min"]), rec["pid"][i]), (seed, i)
    # --- collision
    hits = 0
    for i in range(n):
        L, W = d["LW"][i]
        va, vb = rec["va"][i], rec["vb"][i]
        assert rel_err(orc.get_vertices(d["pa"][i], L, W), va) < 1e-12 and rel_err(orc.get_vertices(d["pb"][i], L, W), vb) < 1e-12
        want = bool(rec["collision"][i])
        assert bool(orc.collision(va, vb)) == want, (seed, i)
        hits += want
    for j, k in enumerate(d["multi_k"]):
        ocol, oidx = orc.collision_multiple(rec["multi_vertices"][j, :k])
        assert np.array_equal(ocol, rec["multi_col"][j, :k]) and np.array_equal(oidx, rec["multi_idx"][j, :k]), (seed, j)
    assert n // 8 < hits < n - n // 8
    # --- ttc, get_range, blocked view, ray_cast
    sa, co, sd = orc.build_beam_tables(UNIT_BEAMS, UNIT_FOV, 0.31, 0.15875, 0.17145)
    ttc = touched = 0
    for i in range(len(d["scan"])):
        want = bool(rec["ttc"][i])
        assert bool(orc.check_ttc(d["scan"][i], d["vel"][i], co, sd, UNIT_TTC)) == want, (seed, i)
        ttc += want
        ego, base, verts = d["ego"][i], d["base"][i], rec["opp_vertices"][i]
        assert orc.get_blocked_view_indices(ego, verts, sa) == tuple(int(v) for v in rec["blocked"][i]), (seed, i)
        changed = rec["ray_cast_changed"][i]      # the reference's ray_cast result where it differs from the input scan, NaN elsewhere
        want_scan = np.where(np.isnan(changed), base, changed)
        got = orc.ray_cast(ego, base.copy(), sa, verts)
        assert np.array_equal(got != base, want_scan != base) and rel_err(got, want_scan) < 1e-12, (seed, i)
        touched += int((want_scan != base).any())
        for j in range(8):
            a, b = verts[j % 4], verts[(j + 1) % 4]
            w, g = rec["get_range"][i, j], orc.get_range(ego, d["theta"][i, j], a, b)
            assert (np.isinf(w) and np.isinf(g)) or abs(g - w) <= 1e-12 * abs(w), (seed, i, j)
    assert ttc > 0 and touched > 0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_unit_functions_sweep(seed):
    """the functions under the step, called one by one on random inputs, recorded reference against the oracle: vehicle_dynamics_st /
    _ks and pid (dynamic_models.py:24-242) with random parameter sets and states on both sides of every switch, get_vertices /
    collision / collision_multiple (collision_models.py:113-260) on car-sized quadrilaterals near and through each other,
    check_ttc_jit, get_range, get_blocked_view_indices, ray_cast (laser_models.py:199-357) on random scans, speeds and opponents"""
    check_unit_functions(seed, record("units", seed))
