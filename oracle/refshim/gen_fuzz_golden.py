#!/usr/bin/env python3
"""Record the reference's side of tests/test_reference_fuzz.py into tests/golden/reference_fuzz_*.npz.

Build-container only (needs the reference tree, imported through ref_loader with the no-op numba shim).  For every case
of that module's tables the reference is RUN on seeded random inputs — poses in free space of its own distance table,
start clusters, random vehicle parameters and actions — and the inputs it was given and every output it returned are
stored; the test replays the inputs through the oracle.  No reference source is copied: the fixtures are data.
The scans of the Simulator and F110Env rollouts are stored as a SHA-256 per row plus the beams the oracle does not reproduce
bit for bit (compact_scans): every case is checked against the live reference before it is written.

    python oracle/refshim/gen_fuzz_golden.py                    # all four sweeps
    python oracle/refshim/gen_fuzz_golden.py --scale 4 sim env  # longer rollouts / more poses, some sweeps only

oracle/refshim/fuzz_live.py uses the record_* functions here on random configurations.
"""
import argparse
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO); sys.path.insert(0, os.path.join(REPO, "tests")); sys.path.insert(0, HERE)
import ref_loader  # noqa: E402
import test_reference_fuzz as T  # noqa: E402
from oracle import orc  # noqa: E402

GOLD = os.path.join(REPO, "tests", "golden")


def _variant_yaml(tmp, name, resolution, origin):
    """a yaml + png pair under tmp: the track's image with ANOTHER resolution / origin (incl. yaw)"""
    _, png = T.map_files(name)
    stem = os.path.join(str(tmp), "%s_r%g_y%g" % (name, resolution, origin[2]))
    shutil.copyfile(png, stem + ".png")
    with open(stem + ".yaml", "w") as f:
        f.write("image: %s.png\nresolution: %r\norigin: [%r, %r, %r]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n"
                % (os.path.basename(stem), resolution, origin[0], origin[1], origin[2]))
    return stem + ".yaml"


def _yaml_for(tmp, name, res2, org2):
    return T.map_files(name)[0] if res2 is None else _variant_yaml(tmp, name, res2, org2)


def _map_record(ref_scan):
    return {"resolution": np.float64(ref_scan.map_resolution), "origin": np.asarray(ref_scan.origin, dtype=np.float64),
            "dt_sha256": T.dt_digest(ref_scan.dt)}


def _free_poses(ref_sim, rng, n, clearance=0.3):
    """n poses inside free space of the loaded reference scan simulator (+ one outside the image)"""
    dt = ref_sim.dt
    rr, cc = np.nonzero(dt > clearance)
    pick = rng.integers(0, len(rr), n)
    res = ref_sim.map_resolution
    u = (cc[pick] + rng.uniform(0.0, 1.0, n)) * res
    v = (rr[pick] + rng.uniform(0.0, 1.0, n)) * res
    c, s = ref_sim.orig_c, ref_sim.orig_s
    poses = np.stack([ref_sim.orig_x + c * u - s * v, ref_sim.orig_y + s * u + c * v, rng.uniform(-7.0, 7.0, n)], axis=1)
    poses[-1, :2] = [ref_sim.orig_x - 3.0, ref_sim.orig_y - 2.0]    # out of bounds: reads dt[-1, -1] on the way in
    return poses


def _start_cluster(ref_scan, rng, A):
    """A cars around one free point, 0.5-1.2 m apart on a jittered line: close enough for opponent windows,
    an occasional GJK contact and (on narrow tracks) wall hits within a few dozen steps"""
    dt = ref_scan.dt
    rr, cc = np.nonzero(dt > 0.9)
    k = rng.integers(0, len(rr))
    res = ref_scan.map_resolution
    c, s = ref_scan.orig_c, ref_scan.orig_s
    u0, v0 = (cc[k] + 0.5) * res, (rr[k] + 0.5) * res
    th = rng.uniform(0, 2 * np.pi)
    out = np.empty((A, 3))
    for i in range(A):
        d = (i - (A - 1) / 2.0) * rng.uniform(0.8, 1.1)
        u, v = u0 + d * np.cos(th) + rng.uniform(-0.1, 0.1), v0 + d * np.sin(th) + rng.uniform(-0.1, 0.1)
        yaw_map = th + rng.uniform(-0.4, 0.4)
        out[i] = [ref_scan.orig_x + c * u - s * v, ref_scan.orig_y + s * u + c * v, yaw_map + np.arctan2(s, c)]
    return out


def record_scan(case, idx, tmp, scale=1.0):
    """ScanSimulator2D(*case) on poses in free space: noise-free scans, and one scan with noise"""
    name, res2, org2, beams, fov, eps, theta_dis, max_range = case
    ns = ref_loader.load_reference()
    ref = ns.laser_models.ScanSimulator2D(beams, fov, eps=eps, theta_dis=theta_dis, max_range=max_range)
    ref.set_map(_yaml_for(tmp, name, res2, org2), ".png")
    rng = np.random.default_rng(7000 + idx)
    poses = _free_poses(ref, rng, max(2, int(round(5 * T.SCAN_CASES[0][3] / beams * scale))))
    std = [0.01, 0.05, 0.2][idx % 3]
    return dict(_map_record(ref), theta_index_increment=np.float64(ref.theta_index_increment), poses=poses,
                scans=np.array([ref.scan(np.array(p), None) for p in poses]),
                noisy_scan=ref.scan(np.array(poses[0]), np.random.default_rng(idx), std_dev=std))


def record_sim(case, idx, tmp, scale=1.0):
    """a Simulator rollout of case: random parameters (one slot its own with >= 3 cars), a start cluster, random actions
    with car 0 turning hard into whatever is beside it for the last two thirds"""
    name, res2, org2, A, integ, time_step, lidar_dist, steps = case
    steps = max(6, int(round(steps * scale)))
    ns = ref_loader.load_reference()
    bc = ns.base_classes
    rng = np.random.default_rng(8000 + idx)
    seed = int(rng.integers(0, 2 ** 31))
    params = T.random_params(rng)
    ref_loader.fresh_racecar_class(ns)
    try:
        sim = bc.Simulator(dict(params), A, seed, time_step=time_step, integrator=getattr(bc.Integrator, integ), lidar_dist=lidar_dist)
        sim.set_map(_yaml_for(tmp, name, res2, org2), ".png")
        own, own_agent = orc.params_vec(None), -1
        if A >= 3:
            p2 = T.random_params(rng)
            sim.update_params(dict(p2), agent_idx=A - 1)
            own, own_agent = orc.params_vec(p2), A - 1
        scan_sim = bc.RaceCar.scan_simulator
        start = _start_cluster(scan_sim, rng, A)
        sim.reset(start.copy())
        out = {k: [] for k in ("actions", "collisions", "collision_idx", "in_collision", "state", "scans")}
        act = np.zeros((A, 2))
        for t in range(steps):
            if t % 8 == 0:
                act = np.stack([rng.uniform(-0.4, 0.4, A), rng.uniform(-1.0, 9.0, A)], axis=1)
            if t >= steps // 3:
                act[0] = [0.41, 7.0]    # car 0 turns as hard as it can at speed: into a wall or a neighbour on the narrow tracks
            out["actions"].append(act.copy())
            obs = sim.step(act.copy())
            out["collisions"].append(np.array(obs["collisions"], dtype=np.float64))
            out["collision_idx"].append(np.array(sim.collision_idx))
            out["in_collision"].append(np.array([int(a.in_collision) for a in sim.agents]))
            out["state"].append(np.array([a.state for a in sim.agents]))
            out["scans"].append(np.array(obs["scans"]))
        rec = {k: np.array(v) for k, v in out.items()}
        rec.update(_map_record(scan_sim), seed=np.int64(seed), params=orc.params_vec(params), own_params=own,
                   own_params_agent=np.int64(own_agent), start=start)
        return rec
    finally:
        ref_loader.fresh_racecar_class(ns)


def record_env(case, idx, scale=1.0):
    """an F110Env episode of case: forwards out of the start zone and backwards into it again (or circling at full lock),
    until the ego is done or the steps run out"""
    name, A, ego, integ, ts, ld, steps = case[:7]
    circle = len(case) > 7 and case[7] == "circle"
    steps = max(8, int(round(steps * scale)))
    ns = ref_loader.load_reference(with_env=True)
    rng = np.random.default_rng(9000 + idx)
    seed = int(rng.integers(0, 2 ** 31))
    params = T.random_params(rng)
    ref_loader.fresh_racecar_class(ns)
    try:
        kw = dict(num_agents=A, ego_idx=ego, seed=seed, timestep=ts, integrator=getattr(ns.base_classes.Integrator, integ), lidar_dist=ld, params=dict(params))
        if name is not None:
            kw.update(map=os.path.splitext(T.map_files(name)[0])[0], map_ext=".png")
        env = ns.f110_env.F110Env(**kw)
        scan_sim = ns.base_classes.RaceCar.scan_simulator
        start = _start_cluster(scan_sim, rng, A)
        keys = ("poses_x", "poses_y", "poses_theta", "linear_vels_x", "ang_vels_z", "scans", "collisions", "lap_counts", "lap_times")
        out = {k: [] for k in keys + ("actions", "checkpoint_done", "done", "reward", "ego_idx", "toggle_list", "near_starts")}
        obs, r, done, info = env.reset(start.copy())
        act = np.zeros((A, 2))
        sp = steer = np.zeros(A)
        for k in range(steps + 1):
            if k:
                if (k - 1) % 6 == 0:
                    sp = rng.uniform(2.0, 4.5, A)
                    steer = rng.uniform(-0.12, 0.12, A)
                # forwards until out of the 0.32 m start zone, backwards until in it again (toggles 1, 2, ...; f110_env.py:230-240)
                act = np.stack([steer, np.where(np.asarray(env.toggle_list) % 2 == 0, sp, -sp)], axis=1)
                if circle:
                    act = np.stack([np.full(A, 0.4), 0.75 * sp], axis=1)
                obs, r, done, info = env.step(act.copy())
            out["actions"].append(act.copy() if k else np.zeros((A, 2)))
            for key in keys:
                out[key].append(np.array(obs[key], dtype=np.float64))   # (copies: the env updates some of them in place)
            out["checkpoint_done"].append(np.array(info["checkpoint_done"]))
            out["done"].append(bool(done)); out["reward"].append(float(r)); out["ego_idx"].append(int(obs["ego_idx"]))
            out["toggle_list"].append(np.array(env.toggle_list)); out["near_starts"].append(np.array(env.near_starts))
            if done:
                break
        rec = {k: np.array(v) for k, v in out.items()}
        rec.update(_map_record(scan_sim), seed=np.int64(seed), params=orc.params_vec(params), start=start, steps=np.int64(steps))
        return rec
    finally:
        ref_loader.fresh_racecar_class(ns)


def record_units(seed):
    """the reference's unit functions on T.unit_inputs(seed)"""
    ns = ref_loader.load_reference()
    dm, cm, lm = ns.dynamic_models, ns.collision_models, ns.laser_models
    d = T.unit_inputs(seed)
    rec = {k: [] for k in ("st", "ks", "pid", "va", "vb", "collision", "multi_vertices", "multi_col", "multi_idx", "ttc",
                           "opp_vertices", "blocked", "ray_cast_changed", "get_range")}
    for pv, x, u, q in zip(d["params"], d["x"], d["u"], d["q"]):
        p = T.params_dict(pv)
        args = (p["mu"], p["C_Sf"], p["C_Sr"], p["lf"], p["lr"], p["h"], p["m"], p["I"], p["s_min"], p["s_max"], p["sv_min"], p["sv_max"],
                p["v_switch"], p["a_max"], p["v_min"], p["v_max"])
        rec["st"].append(dm.vehicle_dynamics_st(x.copy(), u.copy(), *args))
        rec["ks"].append(dm.vehicle_dynamics_ks(x[:5].copy(), u.copy(), *args))
        rec["pid"].append(np.array(dm.pid(q[0], q[1], q[2], q[3], p["sv_max"], p["a_max"], p["v_max"], p["v_min"]), dtype=np.float64))
    for (L, W), pa, pb in zip(d["LW"], d["pa"], d["pb"]):
        va, vb = cm.get_vertices(pa, L, W), cm.get_vertices(pb, L, W)
        rec["va"].append(va); rec["vb"].append(vb)
        rec["collision"].append(bool(cm.collision(va.copy(), vb.copy())))
    for j, k in enumerate(d["multi_k"]):
        L, W = d["LW"][10 * j]
        allv = np.zeros((6, 4, 2))
        allv[:k] = np.stack([cm.get_vertices(pose, L, W) for pose in d["multi_poses"][j, :k]])
        col, idx = cm.collision_multiple(allv[:k].copy())
        rec["multi_vertices"].append(allv)
        rec["multi_col"].append(np.concatenate([np.asarray(col, dtype=np.float64), np.zeros(6 - k)]))
        rec["multi_idx"].append(np.concatenate([np.asarray(idx, dtype=np.float64), np.zeros(6 - k)]))
    sa, co, sd = orc.build_beam_tables(T.UNIT_BEAMS, T.UNIT_FOV, 0.31, 0.15875, 0.17145)
    for i in range(len(d["scan"])):
        ego, base = d["ego"][i], d["base"][i]
        rec["ttc"].append(bool(lm.check_ttc_jit(d["scan"][i].copy(), d["vel"][i], sa, co, sd, T.UNIT_TTC)))
        verts = cm.get_vertices(d["opp"][i], 0.58, 0.31)
        rec["opp_vertices"].append(verts)
        rec["blocked"].append(lm.get_blocked_view_indices(ego, verts.copy(), sa))
        want = lm.ray_cast(ego, base.copy(), sa, verts.copy())
        rec["ray_cast_changed"].append(np.where(want != base, want, np.nan))
        rec["get_range"].append([lm.get_range(ego, th, verts[j % 4], verts[(j + 1) % 4]) for j, th in enumerate(d["theta"][i])])
    rec = {k: np.array(v) for k, v in rec.items()}
    rec["inputs_sha256"] = d["sha256"]
    return rec


def compact_scans(rec, oracle_scans):
    """the fixture form of a record's scans [T, A, B] (tests/test_reference_fuzz.py reference_scans): a SHA-256 of every row,
    and the values of the beams where the oracle's scans (one [A, B] block per step it compared) are not bit-equal to the
    reference's — every beam of the steps it did not reach"""
    scans = rec.pop("scans")
    differs = np.ones(scans.shape, dtype=bool)
    n = len(oracle_scans)
    if n:
        differs[:n] = np.array(oracle_scans) != scans[:n]
    beams = np.flatnonzero(differs)
    rec.update(scan_sha256=T.row_digests(scans), scan_beams=beams.astype(np.int64), scan_values=scans.reshape(-1)[beams])
    return rec


def _checked(check, case, idx, rec):
    """the oracle against the live record (as tests/test_reference_fuzz.py checks the fixture), then the record's fixture form"""
    oracle_scans = []
    check(case, idx, rec, oracle_scans)
    return compact_scans(rec, oracle_scans)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("sweeps", nargs="*", default=["scan", "sim", "env", "units"])
    ap.add_argument("--scale", type=float, default=1.0, help="poses per scan case and steps per rollout, relative to the committed sweep")
    args = ap.parse_args(argv)
    if not ref_loader.reference_available():
        print("the reference tree is not at %s" % ref_loader.REF_ROOT)
        return 1
    warnings.simplefilter("ignore")
    for kind in args.sweeps:
        arrays = {}
        with tempfile.TemporaryDirectory() as tmp:
            if kind == "scan":
                recs = [record_scan(c, i, tmp, args.scale) for i, c in enumerate(T.SCAN_CASES)]
            elif kind == "sim":
                recs = [_checked(T.check_sim_case, c, i, record_sim(c, i, tmp, args.scale)) for i, c in enumerate(T.SIM_CASES)]
            elif kind == "env":
                recs = [_checked(T.check_env_case, c, i, record_env(c, i, args.scale)) for i, c in enumerate(T.ENV_CASES)]
            elif kind == "units":
                recs = [record_units(s) for s in (0, 1, 2)]
            else:
                raise SystemExit("unknown sweep %r" % kind)
        for i, rec in enumerate(recs):
            arrays.update({"%s%d_%s" % (kind, i, k): v for k, v in rec.items()})
        path = os.path.join(GOLD, "reference_fuzz_%s.npz" % kind)
        np.savez_compressed(path, **arrays)
        print("wrote %s  %.1f KB" % (os.path.relpath(path, REPO), os.path.getsize(path) / 1024.))
    return 0


if __name__ == "__main__":
    sys.exit(main())
