"""Randomised vehicle parameters on the device (f110_param_sampler_*) against the NumPy model
tests/param_sampler_ref.py, which is NumPy's own Generator: the unit form at wave and workgroup edges, explicit draws, in-step
draws on every re-seat path (one launch, one block, two blocks), the drawn rows as the car's parameters, both samplers together,
snapshots and clones, the env classes and shards, the refusals, and nothing changed with the sampler off.  Every comparison is
bitwise."""
import gc
import os

import numpy as np
import pytest

import param_sampler_ref as ref
import rollout_ref as rr
from _util import MAPS, bench_start_poses, load_map_image, map_stem, oracle_map_dt, raceline
from reset_sampler_ref import SamplerModel, SlotModel, wrap_diff

pytestmark = pytest.mark.gpu

CSV = os.path.join(MAPS, "example_waypoints.csv")
KEYS = ref.PARAM_KEYS
CLEAR = float(np.sqrt(0.58 ** 2 + 0.31 ** 2) / 2)
SPECS = {
    "nothing": {},
    "uniform": {"mu": ("uniform", 0.5, 1.1, "agent", False)},
    "relative": {"m": ("uniform", 0.85, 1.15, "agent", True), "I": ("uniform", 0.9, 1.1, "agent", True)},
    "clipped": {"C_Sf": ("normal", 4.7, 0.5, 4.5, 5.0, "agent", False)},
    "scopes": {"mu": ("uniform", 0.5, 1.1, "env", False), "C_Sr": ("normal", 5.4, 0.3, 4.5, 6.5, "agent", False),
               "m": ("normal", 1.0, 0.1, 0.7, 1.3, "env", True), "a_max": ("uniform", 7.0, 11.0, "agent", False)},
    "all16": dict([(k, ("uniform", 0.9, 1.1, "agent" if i % 3 else "env", True)) for i, k in enumerate(KEYS[:16]) if i % 2 == 0] +
                  [(k, ("normal", 1.0, 0.05, 0.9, 1.1, "env" if i % 3 else "agent", True)) for i, k in enumerate(KEYS[:16]) if i % 2 == 1]),
}
DRIVE = {"mu": ("uniform", 0.5, 1.1, "env", False), "m": ("uniform", 0.85, 1.15, "agent", True), "C_Sf": ("normal", 4.7, 0.5, 4.5, 5.0, "agent", False)}


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _nominal(amd, A):
    """A agent slots with different masses, inertias and steering limits"""
    rows = np.tile(amd._ffi.params_vector(amd.core.DEFAULT_PARAMS), (A, 1))
    for a in range(A):
        rows[a, KEYS.index("m")] *= 1.0 + 0.25 * a
        rows[a, KEYS.index("I")] *= 1.0 + 0.1 * a
        rows[a, KEYS.index("s_max")] += 0.01 * a
    return rows


def _track(amd):
    return amd.Track.from_xy(raceline()[:, 1:3])


def _sim(amd, E, A=2, dists=None, seed=0, slots=False, **kw):
    """a handle on the example map; slots: the agent slots get _nominal's different parameter sets"""
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    s.set_track(_track(amd))
    if slots:
        for a, row in enumerate(_nominal(amd, A)):
            s.set_params(dict(zip(KEYS, row)), a)
    if dists is not None:
        s.set_param_sampler(ref.sampler_of(dists, seed))
    return s


def _model(amd, dists, seed, E, A, slots=False, env_base=0):
    nom = _nominal(amd, A) if slots else np.tile(amd._ffi.params_vector(amd.core.DEFAULT_PARAMS), (A, 1))
    return ref.ParamModel(dists, nom, E, seed=seed, env_base=env_base)


def _obs(s):
    o = s.get("state", "scans", "collisions", "in_collision", "step_count")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def _same(a, b, what=""):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), "%s %s differs" % (what, k)


def _bits_equal(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape and np.array_equal(got.view(np.uint64), want.view(np.uint64)), what


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs crash within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


# ---- 1. the unit form -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def unit_sim(amd):
    s = amd.BatchSim(num_envs=1, num_agents=1)
    yield s
    s.close()


def _clip_seed(amd, m, A, rounds):
    """the first seed for which the model alone shows a value at lo, one at hi and one inside"""
    d = SPECS["clipped"]
    for seed in range(500):
        M = ref.ParamModel(d, _nominal(amd, A), m, seed=seed, env_base=11)
        seen = []
        for _ in range(rounds):
            M.draw_mask(np.ones(m, dtype=bool))
            seen.append(M.rows[:, 1].copy())
        v = np.concatenate(seen)
        if np.any(v == 4.5) and np.any(v == 5.0) and np.any((v > 4.5) & (v < 5.0)):
            return seed
    raise AssertionError("no seed below 500 binds the clip on both sides and leaves a value inside")


@pytest.mark.parametrize("A", [1, 2, 4])
@pytest.mark.parametrize("m", [1, 63, 64, 65, 257])
def test_unit_form_matches_model(amd, unit_sim, m, A):
    rounds, nom = 3, _nominal(amd, A)
    for name in sorted(SPECS):
        dists = SPECS[name]
        seed = _clip_seed(amd, m, A, rounds) if name == "clipped" else 4242
        ps = ref.sampler_of(dists, seed)
        words = ps.streams(m, 11)
        M = ref.ParamModel(dists, nom, m, words=words)
        rows, after = unit_sim.param_sample_rows(ps, nom, words, rounds=rounds)
        assert rows.shape == (rounds, m * A, 18)
        for r in range(rounds):
            M.draw_mask(np.ones(m, dtype=bool))
            _bits_equal(rows[r], M.rows, "%s: round %d of m = %d, A = %d" % (name, r, m, A))
        assert np.array_equal(after, M.words()), "%s: the streams afterwards" % name
        if name == "nothing":
            assert np.array_equal(after, words) and np.array_equal(rows[-1], np.tile(nom, (m, 1)))
        if name == "clipped":
            v = rows[:, :, 1]
            assert np.any(v == 4.5) and np.any(v == 5.0) and np.any((v > 4.5) & (v < 5.0))


# ---- 2. explicit draws on a handle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_mask", [False, True])
def test_explicit_draw_touches_only_the_masked_envs(amd, device_mask):
    E, A, seed = 65, 2, 17
    s = _sim(amd, E, A, SPECS["scopes"], seed, slots=True)
    M = _model(amd, SPECS["scopes"], seed, E, A, slots=True)
    _bits_equal(s.get_params(), M.rows, "armed: the nominal rows, nothing drawn")
    assert s.param_sampler_stats()["draws"] == 0
    mask = np.arange(E) % 3 == 1
    if device_mask:
        d_mask = s.device_array((E,), np.uint8)
        d_mask.upload(mask.astype(np.uint8))
        s.sample_params_device(d_mask)
    else:
        s.sample_params(mask)
    M.draw_mask(mask)
    _bits_equal(s.get_params(), M.rows, "masked envs drawn, every other row unchanged")
    assert s.param_sampler_stats(clear=True)["draws"] == int(mask.sum())
    s.sample_params()      # every stream stands where the model's does: the masked ones one draw on, the others at their start
    M.draw_mask(np.ones(E, dtype=bool))
    _bits_equal(s.get_params(), M.rows, "the draw after")
    assert s.param_sampler_stats()["draws"] == E
    view = s.params_view()
    assert view.shape == (E * A, 18) and np.array_equal(view.download(), M.rows)
    s.close()


# ---- 3. in-step draws -------------------------------------------------------------------------------------------------------------------
FORMS = ["auto", "collided", "episode", "host_block", "episode_host"]


def _run_in_step(amd, form, E, A, T, seed, dists=DRIVE, step_groups=0, reset_sampler=None):
    """T crashing steps of one re-seat form with the sampler armed; after every step the rows must be the model's (re-seated
    envs one draw on, the others unchanged) and the counter the number of re-seats.  Returns (handle, rows per step, re-seats)"""
    s = _sim(amd, E, A, dists, seed, slots=True, step_groups=step_groups)
    if reset_sampler is not None:
        s.set_reset_sampler(**reset_sampler)
    M = _model(amd, dists, seed, E, A, slots=True)
    start = bench_start_poses(E, A)
    if form in ("episode", "host_block", "episode_host"):
        s.episode_init(0)
        s.episode_reset(start)
    else:
        s.reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    if form == "auto":
        s.set_auto_reseat(d_start, 0)
    d_act = s.device_array((E * A, 2))
    s._keep = (d_start, d_act)   # (the armed re-seat reads d_start: it lives with the handle)
    acts = _crash_actions(T, E * A)
    hb = s.host_block(["state", "done"]) if form == "host_block" else None
    if form == "episode_host":
        act_pin = s.pinned_empty((E * A, 2))
        packed = s.pinned_empty((s.packed_bytes(),), np.uint8)
    history, poses, reseats, launches = [], [], 0, set()
    for t in range(T):
        d_act.upload(acts[t])
        if form == "auto":
            s.step_device(d_act)
        elif form == "collided":
            s.step_device(d_act)
            s.reset_collided_device(d_start, 0)
        elif form == "episode":
            s.episode_step_device(d_act)
            s.episode_reset_done_device()
        elif form == "episode_host":
            act_pin[...] = acts[t]
            s.episode_step_host(act_pin, packed, auto_reset=True)
        else:
            hb.actions[...] = acts[t]
            s.step_host(hb, None, auto_reset=True)
            launches.add(s.step_launches())
        o = s.get("state", "step_count")
        seated = o["step_count"].reshape(E, A)[:, 0] == 0
        M.draw_mask(seated)
        reseats += int(seated.sum())
        rows = s.get_params()
        _bits_equal(rows, M.rows, "%s step %d: re-seated envs %s" % (form, t, np.flatnonzero(seated)[:8].tolist()))
        assert s.param_sampler_stats()["draws"] == reseats, "%s step %d" % (form, t)
        history.append(rows)
        poses.append((seated, o["state"][:, [0, 1, 4]].copy()))
    s._launches, s._poses = launches, poses
    return s, history, reseats


@pytest.mark.parametrize("form", FORMS)
def test_in_step_draws_on_a_tiny_handle(amd, form):
    """E = 2, A = 2: under f110_step_host the whole step is one launch, with the draw behind it as a second"""
    s, _, reseats = _run_in_step(amd, form, 2, 2, 300, seed=5)
    assert reseats >= 3, "the policy crashed too rarely (%d re-seats)" % reseats
    if form == "host_block":
        assert s._launches == {2}, s._launches   # k_step_tiny + the draw
    s.close()


@pytest.mark.parametrize("form", FORMS)
def test_in_step_draws_two_blocks_equal_one(amd, form):
    E, A, T = 512, 2, 100
    s1, h1, n1 = _run_in_step(amd, form, E, A, T, seed=6, step_groups=1)
    s2, h2, n2 = _run_in_step(amd, form, E, A, T, seed=6, step_groups=2)
    assert n1 == n2 and n1 >= 50
    if form in ("auto", "episode"):   # (the device forms split; the host forms run their one block on either handle)
        assert s1.step_groups()[2] == 1 and s2.step_groups()[2] == 2
    for a, b in zip(h1, h2):
        _bits_equal(a, b, "two blocks")
    _same(_obs(s1), _obs(s2), "two blocks")
    s1.close()
    s2.close()


# ---- 4. the drawn rows drive the car ------------------------------------------------------------------------------------------------------
def test_drawn_rows_drive_the_car(amd):
    E, A, seed = 33, 2, 23
    s = _sim(amd, E, A, DRIVE, seed, slots=True)
    s.sample_params()
    rows = s.get_params()
    M = _model(amd, DRIVE, seed, E, A, slots=True)
    M.draw_mask(np.ones(E, dtype=bool))
    _bits_equal(rows, M.rows, "the draw")
    assert len(np.unique(rows[:, 0])) == E and len(np.unique(rows[:, 6])) == E * A
    twin = _sim(amd, E, A, slots=True)
    twin.set_params_batch(rows)
    start = bench_start_poses(E, A)
    rng = np.random.default_rng(4)
    acts = np.stack([rng.uniform(-0.3, 0.3, (20, E * A)), rng.uniform(2.0, 7.0, (20, E * A))], axis=2)
    plain = _sim(amd, E, A, slots=True)
    for h in (s, twin, plain):
        h.reset(start)
    for t in range(20):
        for h in (s, twin, plain):
            h.step(acts[t])
        _same(_obs(s), _obs(twin), "step %d" % t)
    assert not np.array_equal(_obs(s)["state"], _obs(plain)["state"])   # (and the rows matter)
    # one agent's rollout from where it stands (an empty steering FIFO) with its drawn row: the model run with that row
    i = 5
    o = s.get("state")["state"]
    start10 = np.concatenate([o[i], [0.0, 0.0, 0.0]])[None, :]
    K, H, repeat = 3, 5, 3
    cand = np.stack([rng.uniform(-0.3, 0.3, (K, H)), rng.uniform(2.0, 6.0, (K, H))], axis=2)
    st = rr.settings(k=K, horizon=H, repeat=repeat, margin=0.2, traj=False)
    got = s.rollout_rows(amd.Rollout(**st), start10, cand, params=rows[i:i + 1], raw=True)
    flown = rr.fly(rr.scan_oracle("example_map"), start10, rows[i:i + 1], cand, False, repeat, 0.2, 1)
    want = rr.render(st, start10, flown)[1]
    keep = flown[4] >= 1e-9
    exact = list(rr.EXACT[:6])   # (no track on this call: PROGRESS and END_LAT are 0.0 on both sides)
    print("rollout with the drawn row: largest |got - want| %.3e" % np.max(np.abs(got[1][keep][:, exact] - want[keep][:, exact])))
    _bits_equal(got[1][keep][:, exact], want[keep][:, exact], "the rollout with the drawn row")
    other = rr.fly(rr.scan_oracle("example_map"), start10, _nominal(amd, A)[i % A][None, :], cand, False, repeat, 0.2, 1)
    assert not np.array_equal(other[0], flown[0])
    for h in (s, twin, plain):
        h.close()


# ---- 5. both samplers ---------------------------------------------------------------------------------------------------------------------
def _check_poses(got, want, what):
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    np.testing.assert_array_equal(got[:, :2], want[:, :2], err_msg=what + " x, y")
    assert np.all(np.abs(wrap_diff(got[:, 2], want[:, 2])) <= 1e-15), what + " theta"


def test_both_samplers_draw_independently(amd):
    E, A, T = 64, 2, 150
    s, _, reseats = _run_in_step(amd, "auto", E, A, T, seed=78, reset_sampler=dict(seed=77))
    assert reseats >= 10
    dt, res, origin = oracle_map_dt("example_map")
    R = SamplerModel(77, E, A, [SlotModel(_track(amd), dt, res, origin)], clearance=CLEAR)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    for seated, pose in s._poses:
        for e in np.flatnonzero(seated):
            p, _ = R.draw(e)
            _check_poses(pose[e * A:(e + 1) * A], start[e] if p is None else p, "env %d" % e)
    assert s.reset_sampler_stats()["draws"] == s.param_sampler_stats()["draws"] == reseats
    # arming and clearing either one leaves the other's next draw where it was
    M = _model(amd, DRIVE, 78, E, A, slots=True)
    for seated, _ in s._poses:
        M.draw_mask(seated)
    s.clear_reset_sampler()
    s.sample_params()
    M.draw_mask(np.ones(E, dtype=bool))
    _bits_equal(s.get_params(), M.rows, "after clearing the reset sampler")
    s.set_reset_sampler(seed=77)
    s.sample_params()
    M.draw_mask(np.ones(E, dtype=bool))
    _bits_equal(s.get_params(), M.rows, "after arming the reset sampler")
    R2 = SamplerModel(77, E, A, [SlotModel(_track(amd), dt, res, origin)], clearance=CLEAR)
    s.clear_param_sampler()
    s.sample_reset()
    want = np.stack([R2.draw(e)[0] for e in range(E)])
    _check_poses(s.reset_sampler_poses(), want, "after clearing the parameter sampler")
    s.set_param_sampler(ref.sampler_of(DRIVE, 78))
    s.sample_reset()
    want = np.stack([R2.draw(e)[0] for e in range(E)])
    _check_poses(s.reset_sampler_poses(), want, "after arming the parameter sampler")
    s.close()


# ---- 6. snapshots ---------------------------------------------------------------------------------------------------------------------------
def test_snapshot_restore_clone_and_subset(amd):
    E, A = 64, 2
    s, _, _ = _run_in_step(amd, "auto", E, A, 40, seed=9)
    blob = s.save_state()
    assert "param_rng" in blob.header["columns"] and "params" in blob.header["columns"]
    d_act = s.device_array((E * A, 2))
    acts = _crash_actions(80, E * A, seed=12)

    def run():
        seq = []
        for t in range(80):
            d_act.upload(acts[t])
            s.step_device(d_act)
            seq.append((_obs(s), s.get_params()))
        return seq
    s.param_sampler_stats(clear=True)
    first = run()
    assert s.param_sampler_stats()["draws"] >= 10
    rows_end = s.get_params()
    s.load_state(blob)
    again = run()
    for t, ((oa, ra), (ob, rb)) in enumerate(zip(first, again)):
        _same(oa, ob, "restored step %d" % t)
        _bits_equal(ra, rb, "restored rows, step %d" % t)
    # a blob from an armed handle is refused by an unarmed one, and the other way round
    twin = _sim(amd, E, A, slots=True)
    with pytest.raises(ValueError, match="parameter sampler|per-agent params"):
        twin.load_state(blob)
    twin.set_params_batch(rows_end)   # (the rows' column alone does not make it fit)
    with pytest.raises(ValueError, match="parameter sampler"):
        twin.load_state(blob)
    with pytest.raises(ValueError, match="parameter sampler"):
        s.load_state(twin.save_state())
    # clones hold their source's rows and draw what their source draws
    s.clone_envs(list(range(0, 32)), list(range(32, 64)))
    r = s.get_params().reshape(E, A, 18)
    _bits_equal(r[:32], r[32:], "cloned rows")
    s.sample_params()
    r = s.get_params().reshape(E, A, 18)
    _bits_equal(r[:32], r[32:], "the clones' next draw")
    # a subset blob carries rows and streams: envs 3, 5 into envs 10, 11
    sub = s.save_envs([3, 5])
    s.sample_params()
    s.load_envs(sub, [0, 1], [10, 11])
    r = s.get_params().reshape(E, A, 18)
    s.sample_params(np.isin(np.arange(E), [10, 11]))
    r2 = s.get_params().reshape(E, A, 18)
    s.load_envs(sub, [0, 1], [3, 5])
    _bits_equal(s.get_params().reshape(E, A, 18)[[3, 5]], r[[10, 11]], "subset rows")
    s.sample_params(np.isin(np.arange(E), [3, 5]))
    _bits_equal(s.get_params().reshape(E, A, 18)[[3, 5]], r2[[10, 11]], "subset streams")
    s.close()
    twin.close()


# ---- 7. the env classes -------------------------------------------------------------------------------------------------------------------
def test_vec_env_and_shards_agree(amd):
    E, A, T, seed = 48, 2, 30, 31
    rp = ref.sampler_of(DRIVE, seed)
    kw = dict(auto_reset=True, map=map_stem("example_map"), map_ext=".png", track=CSV, random_params=rp)
    envs = [amd.F110VecEnv(E, device_logic=True, **kw), amd.F110VecEnv(E, device_logic=False, **kw),
            amd.ShardedVecEnv(E, devices=[0, 0], shard_sizes=[19, 29], **kw)]
    start = bench_start_poses(E, A).reshape(E, A, 3)
    start[::4, 1] = start[::4, 0] + np.array([0.1, 0.0, 0.0])   # every fourth env: its cars overlap, so it is done at every step
    M = ref.ParamModel(DRIVE, np.tile(amd._ffi.params_vector(amd.core.DEFAULT_PARAMS), (A, 1)), E, seed=seed)
    firsts = [env.reset(start) for env in envs]
    M.draw_mask(np.ones(E, dtype=bool))             # the reset draws in front of itself ...
    for o, r, d, i in firsts[1:]:
        np.testing.assert_array_equal(d, firsts[0][2])
    assert firsts[0][2][::4].all()
    M.draw_mask(firsts[0][2])                       # ... and its own step re-seats the envs that end in it
    for env in envs:
        _bits_equal(env.get_params(), M.rows, "after the full reset")
    mask = np.arange(E) % 5 == 2
    for env in envs:
        env.reset(start, mask)
    M.draw_mask(mask)
    for env in envs:
        _bits_equal(env.get_params(), M.rows, "after the masked reset")
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    dones = 0
    for t in range(T):
        outs = [env.step(acts[t]) for env in envs]
        for o, r, d, i in outs[1:]:
            np.testing.assert_array_equal(o["poses_x"], outs[0][0]["poses_x"])
            np.testing.assert_array_equal(o["poses_y"], outs[0][0]["poses_y"])
            np.testing.assert_array_equal(d, outs[0][2])
        M.draw_mask(outs[0][2])
        dones += int(np.sum(outs[0][2]))
        for env in envs:
            _bits_equal(env.get_params(), M.rows, "step %d" % t)
    assert dones >= T * (E // 4)
    with pytest.raises(RuntimeError, match="random_params"):
        envs[0].update_params_batch(M.rows)
    with pytest.raises(RuntimeError, match="random_params"):
        envs[2].update_params(amd.core.DEFAULT_PARAMS)
    assert envs[0].params_view().shape == (E * A, 18) and len(envs[2].params_view()) == 2
    envs[2].close()
    for env in envs[:2]:
        env.sim.batch.close()


def test_f110env_random_params_over_three_episodes(amd):
    seed = 21
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, random_params=ref.sampler_of(DRIVE, seed))
    M = ref.ParamModel(DRIVE, np.tile(amd._ffi.params_vector(amd.core.DEFAULT_PARAMS), (2, 1)), 1, seed=seed)
    poses = bench_start_poses(1, 2)
    for ep in range(3):
        env.reset(poses)
        M.draw(0)
        _bits_equal(env.get_params(), M.rows, "episode %d" % ep)
        for t in range(5):
            env.step(np.array([[0.1, 3.0], [-0.1, 3.0]]))
        _bits_equal(env.get_params(), M.rows, "episode %d, after its steps" % ep)
    with pytest.raises(RuntimeError, match="random_params"):
        env.update_params(amd.core.DEFAULT_PARAMS)
    env.sim.batch.close()


# ---- 8. refusals and memory ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(amd):
    from f1tenth_gym_amd import _ffi
    from f1tenth_gym_amd.param_sampler import ParamSampler, normal, uniform
    NAN, INF = float("nan"), float("inf")
    E, A, seed = 8, 2, 3
    s = _sim(amd, E, A, SPECS["scopes"], seed, slots=True)
    M = _model(amd, SPECS["scopes"], seed, E, A, slots=True)
    s.sample_params()
    M.draw_mask(np.ones(E, dtype=bool))
    allocs = _ffi.device_allocs()
    refused = [("width", uniform(0.3, 0.4)), ("length", uniform(0.5, 0.6)), ("mu", uniform(1.1, 0.5)), ("mu", uniform(NAN, 0.5)),
               ("C_Sf", uniform(4.0, INF)), ("m", normal(3.7, -0.1, 3.0, 4.0)), ("m", normal(3.7, 0.1, -INF, 4.0)), ("m", normal(3.7, 0.1, 3.0, NAN)),
               ("m", normal(3.7, 0.1, 4.0, 3.0)), ("mu", uniform(0.0, 1.0)), ("C_Sr", normal(5.0, 1.0, 0.0, 6.0)), ("lf", uniform(0.0, 0.2)),
               ("lr", uniform(-0.1, 0.2)), ("h", uniform(0.0, 0.1)), ("I", uniform(-0.5, 1.5, relative=True)), ("a_max", normal(9.0, 1.0, -1.0, 12.0)),
               ("v_switch", uniform(0.0, 8.0)), ("s_min", uniform(-0.5, 0.5)), ("s_max", uniform(-1.0, 1.0, relative=True)),
               ("sv_min", uniform(-1.5, 1.0, relative=True)), ("sv_max", uniform(-4.0, 4.0)), ("v_min", uniform(-5.0, 25.0)), ("v_max", uniform(-6.0, 20.0))]
    words = np.ascontiguousarray(ParamSampler(99).streams(E), dtype=np.uint64)
    for name, dist in refused:
        ps = ParamSampler(99, **{name: dist})
        with pytest.raises(ValueError, match=r"\b%s\b" % name):   # the Python layer refuses first ...
            s.set_param_sampler(ps)
        rc = _ffi.lib().f110_param_sampler_set(s._h, ps.entries(), words.ctypes.data_as(_ffi._u64p))   # ... and so does the ABI
        assert rc == _ffi.ERR_INVALID and name in _ffi.last_error(s._h), (name, rc, _ffi.last_error(s._h))
        out = np.empty((1, A, 18))
        rc = _ffi.lib().f110_param_sample_batch(s._h, ps.entries(), _ffi.dptr(_nominal(amd, A)), A, words.ctypes.data_as(_ffi._u64p), 1, 1,
                                                _ffi.dptr(out), None)
        assert rc == _ffi.ERR_INVALID
    assert _ffi.lib().f110_param_sampler_set(s._h, ParamSampler(99).entries(), None) == _ffi.ERR_INVALID
    assert _ffi.device_allocs() == allocs
    _bits_equal(s.get_params(), M.rows, "the rows after the refusals")
    s.sample_params()                       # the armed sampler and its streams are as they were
    M.draw_mask(np.ones(E, dtype=bool))
    _bits_equal(s.get_params(), M.rows, "the armed sampler's next draw")
    # the rows have one owner
    with pytest.raises(_ffi.F110LibraryError, match="parameter sampler"):
        s.set_params_batch(M.rows)
    with pytest.raises(_ffi.F110LibraryError, match="parameter sampler"):
        s.set_params_batch(None)
    _bits_equal(s.get_params(), M.rows, "after the refused uploads")
    s.close()
    t = _sim(amd, E, A, slots=True)
    with pytest.raises(_ffi.F110LibraryError):
        t.get_params()
    with pytest.raises(_ffi.F110LibraryError):
        t.params_view()
    with pytest.raises(_ffi.F110LibraryError):
        t.sample_params()
    with pytest.raises(_ffi.F110LibraryError):
        t.param_sampler_stats()
    t.set_params_batch(M.rows)
    with pytest.raises(_ffi.F110LibraryError, match="f110_set_params_batch"):
        t.set_param_sampler(ref.sampler_of(SPECS["scopes"], seed))
    _bits_equal(t.get_params(), M.rows, "set_params_batch's rows through f110_params_get")
    t.close()


def test_memory_returns_and_nothing_changes_when_disarmed(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 16, 2
    gc.collect()
    base = _ffi.device_allocs()
    never = _sim(amd, E, A)
    s = _sim(amd, E, A)
    before = _ffi.device_allocs()
    s.set_param_sampler(ref.sampler_of(DRIVE, 1))
    assert _ffi.device_allocs()[0] > before[0]
    s.sample_params()
    s.set_param_sampler(ref.sampler_of(SPECS["scopes"], 2))   # re-arming replaces, it does not stack
    s.clear_param_sampler()
    assert _ffi.device_allocs() == before
    start = bench_start_poses(E, A)
    hbs = []
    for h in (never, s):
        h.episode_init(0)
        h.episode_reset(start)
        hbs.append(h.host_block(["state", "done"]))
    acts = _crash_actions(50, E * A, seed=2)
    for t in range(50):
        for h, hb in zip((never, s), hbs):
            hb.actions[...] = acts[t]
            h.step_host(hb, None, auto_reset=True)
        assert never.step_launches() == s.step_launches()
        _same(_obs(never), _obs(s), "disarmed step %d" % t)
    assert len(never.save_state().to_bytes()) == len(s.save_state().to_bytes())
    s.set_param_sampler(ref.sampler_of(DRIVE, 1))
    s.close()
    never.close()
    assert _ffi.device_allocs() == base
