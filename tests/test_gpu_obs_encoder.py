"""The observation encoder on the device (f110_obs_encode_*) against the NumPy model tests/obs_encoder_ref.py, bit for
bit on the uint32 view: the unit form over the grid of the host tests, the device form through noisy steps with in-step re-seats
(2 and 3 cars, track features, 4096 beams, per-env maps), env blocks, no effect on the simulation, the vector envs, shards,
a torch consumer, and the refusals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import obs_encoder_ref as ref
from _util import MAPS, bench_start_poses, load_any_map_image, load_map_image, map_stem, raceline

pytestmark = pytest.mark.gpu

CSV = os.path.join(MAPS, "example_waypoints.csv")
SEED, STD = 4242, 0.01
SCALES = {"vx": 8.0, "steer": 0.4189, "yaw_rate": 3.2, "slip": -0.7, "collision": 1.0, "lateral": 1.5, "heading_error": 3.0, "ds": 0.2}
FIVE = ("vx", "steer", "yaw_rate", "slip", "collision")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _same_bits(got, want, what):
    g, w = ref.bits(got), ref.bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d of %d floats differ, first at %s: got %r (0x%08x) want %r (0x%08x)" % (
            what, len(bad), g.size, bad[0].tolist(), got[tuple(bad[0])], g[tuple(bad[0])], want[tuple(bad[0])], w[tuple(bad[0])]))


def _crash_actions(T, N, seed=3):
    rng = np.random.default_rng(seed)   # hard steering at speed: envs hit the walls within a few dozen steps
    return np.stack([rng.uniform(-0.42, 0.42, (T, N)), rng.uniform(4.0, 12.0, (T, N))], axis=2)


def _columns(s, track):
    """what the model is fed: the downloaded scans, the eight feature sources [N][8] and step_count of the last step"""
    o = s.get("scans", "state", "collisions", "step_count")
    st = o["state"]
    cols = np.zeros((s.N, 8))
    cols[:, 0], cols[:, 1], cols[:, 2], cols[:, 3], cols[:, 4] = st[:, 3], st[:, 2], st[:, 5], st[:, 6], o["collisions"]
    if track:
        t = s.get_track()
        cols[:, 5], cols[:, 6], cols[:, 7] = t["lateral"], t["heading_error"], t["ds"]
    return np.array(o["scans"], copy=True), cols, np.array(o["step_count"], copy=True)


# ---- the unit form over the grid ---------------------------------------------------------------------------------------------
def test_unit_form_matches_model_over_the_grid(amd):
    rng = np.random.default_rng(11)
    sims = {B: amd.BatchSim(num_envs=1, num_agents=1, num_beams=B) for B in ref.GRID_B}   # (no map: a unit entry point)
    n = 0
    for B, beams, K, pool, F, fill in ref.unit_grid():
        feats = ref.FEATURES if n % 3 == 0 else (FIVE if n % 3 == 1 else ("steer", "ds"))
        enc = amd.ObsEncoder(sectors=K, pool=pool, beams=beams, features=feats, frames=F, range_clip=30.0, range_scale=30.0 if n % 2 else 7.0,
                             scales=SCALES, num_beams=B)
        scans, cols, sc, stack = ref.random_inputs(rng, 7, B, F, enc.dim)
        got = sims[B].obs_encode_batch(enc, scans, cols, sc, stack, fill)
        _same_bits(got, ref.encode(enc, scans, cols, sc, stack, fill), "B=%d beams=%r K=%d %s F=%d fill=%r" % (B, beams, K, pool, F, fill))
        n += 1
    assert n > 300
    # features only; more agents than a workgroup holds; results in float32's subnormal range (converted, not flushed)
    s = sims[61]
    enc = amd.ObsEncoder(sectors=0, features=ref.FEATURES, frames=3, scales=SCALES)
    scans, cols, sc, stack = ref.random_inputs(rng, 133, 61, 3, enc.dim)
    _same_bits(s.obs_encode_batch(enc, scans, cols, sc, stack), ref.encode(enc, scans, cols, sc, stack), "features only")
    enc = amd.ObsEncoder(sectors=61, pool="center", features=("vx",), frames=1)
    scans = np.full((2, 61), 1.0)
    scans[0, :] = 30.0 * 2.0 ** -130 * np.arange(1, 62)
    scans[1, :5] = [30.0 * 2.0 ** -149, 30.0 * 2.0 ** -150, 30.0 * 2.0 ** -151, 30.0 * 1.5 * 2.0 ** -149, 0.0]
    cols = np.zeros((2, 8))
    cols[:, 0] = [1e-41, -3e-45]
    z = np.zeros((2, 1, 62), np.float32)
    _same_bits(s.obs_encode_batch(enc, scans, cols, np.array([2, 2]), z), ref.encode(enc, scans, cols, np.array([2, 2]), z), "subnormal results")
    for b in sims.values():
        b.close()


def test_unit_form_matches_model_over_the_launch_forms(amd):
    """the rows of ref.launch_form_grid(): both sides of the staging rule (k_obs_encode<true> with exactly 64 KiB of LDS,
    k_obs_encode<false> walking the window in HBM from beam_lo), F up to 16, F * D up to the cap, every phase of the aligned store.
    profiles/obs_encoder_launch_forms.txt is to hold the kernel names a trace of this test sees."""
    rng = np.random.default_rng(13)
    rows = ref.launch_form_grid()
    sims = {B: amd.BatchSim(num_envs=1, num_agents=1, num_beams=B) for B in sorted({r[0] for r in rows})}
    forms = set()
    for row in rows:
        B, beams, K, pool, F, fill, feats, staged = row
        enc = ref.launch_form_encoder(amd.ObsEncoder, row, SCALES)
        W = B if beams is None else beams[1] - beams[0]
        assert ref.planned_staged(W, F, enc.dim) is staged, row
        scans, cols, sc, stack = ref.launch_form_inputs(rng, 7, row, enc.dim)
        got = sims[B].obs_encode_batch(enc, scans, cols, sc, stack, fill)
        _same_bits(got, ref.encode(enc, scans, cols, sc, stack, fill), "B=%d beams=%r K=%d %s F=%d fill=%r %s" % (
            B, beams, K, pool, F, fill, "staged" if staged else "unstaged"))
        forms.add(staged)
    assert forms == {True, False}
    for b in sims.values():
        b.close()


# ---- the device form through noisy steps with in-step re-seats ---------------------------------------------------------------
def _sim(amd, E, A=2, B=1080, track=False, maps=False, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, **kw)
    s.set_map_image(*load_map_image("example_map"))
    if maps:
        slot = s.add_map_image(*load_any_map_image("skirk"))
        s.set_env_maps(np.where(np.arange(E) % 3 == 1, slot, 0).astype(np.int32))
    s.set_noise_rng(SEED, STD)
    if track:
        s.set_track(amd.Track.from_xy(raceline()[:, 1:3]))
        s.enable_track()
    return s


def _armed(s, E, A):
    start = bench_start_poses(E, A)
    s.reset(start)
    d_start = s.device_array((E * A, 3))
    d_start.upload(start)
    s.set_auto_reseat(d_start, 0)
    d_act = s.device_array((E * A, 2))
    s._keep = (d_start, d_act)   # (the armed re-seat reads d_start: it lives with the handle)
    return d_act


@pytest.mark.parametrize("name,A,B,track,maps,enc_kw", [
    ("two_cars", 2, 1080, False, False, dict(sectors=108, pool="min", features=FIVE, frames=4)),
    ("three_cars", 3, 1080, False, False, dict(sectors=64, pool="mean", features=FIVE, frames=3, beams=(90, 990))),
    ("track", 2, 1080, True, False, dict(sectors=7, pool="center", features=ref.FEATURES, frames=4)),
    ("beams_4096", 2, 4096, False, False, dict(sectors=270, pool="mean", features=("vx", "collision"), frames=2)),
    ("per_env_maps", 2, 1080, False, True, dict(sectors=108, pool="min", features=FIVE, frames=4)),
    # F * D = 16 * 512 = 8192 next to a 4096-beam row: k_obs_encode<false>; the stack is 32 KiB per agent, 4 MiB in all
    ("unstaged_16_frames", 2, 4096, True, False, dict(sectors=504, pool="mean", features=ref.FEATURES, frames=16)),
])
def test_device_form_follows_model_through_reseats(amd, name, A, B, track, maps, enc_kw):
    E, T = 64, 120
    assert ref.planned_staged(B, enc_kw["frames"], enc_kw["sectors"] + len(enc_kw["features"])) is (name != "unstaged_16_frames")
    s = _sim(amd, E, A, B, track, maps)
    d_act = _armed(s, E, A)
    enc = amd.ObsEncoder(range_clip=10.0, range_scale=10.0, scales=SCALES, **enc_kw)
    acts = _crash_actions(T, E * A)
    stack = np.zeros(enc.shape(E * A), np.float32)
    out = None
    zeros = ones_after_zero = hits = 0
    prev_sc = None
    for t in range(T):
        d_act.upload(acts[t])
        s.step_device(d_act)
        out = s.encode_obs_device(enc, out)            # (the first call allocates the stack and fills every frame)
        scans, cols, sc = _columns(s, track)
        stack = ref.encode(enc, scans, cols, sc, stack, fill=(t == 0))
        _same_bits(out.download(), stack, "%s step %d" % (name, t))
        zeros += int(np.sum(sc == 0))
        hits += int(np.sum(cols[:, 4] != 0))
        if prev_sc is not None:
            ones_after_zero += int(np.sum((prev_sc == 0) & (sc == 1)))
        prev_sc = sc
    assert s.encode_obs_device(enc) is out and tuple(out.shape) == enc.shape(E * A) and out.dtype == np.float32   # (one buffer per encoder)
    stack = ref.encode(enc, *_columns(s, track), stack)     # ... and that call shifted the same step in once more
    assert zeros >= 20 and ones_after_zero >= 20, "too few re-seats to test the frame rule (%d, %d)" % (zeros, ones_after_zero)
    _same_bits(s.encode_obs(enc, out), ref.encode(enc, *_columns(s, track), stack), "the host form")
    s.close()


# ---- env blocks ------------------------------------------------------------------------------------------------------------------
def _everything(s):
    o = s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count", "agent_poses")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def test_two_blocks_equal_one_and_stay_two(amd):
    E, A, T = 512, 2, 50
    enc = amd.ObsEncoder(sectors=108, pool="min", features=FIVE, frames=4, scales=SCALES)
    stacks = []
    for groups in (1, 2):
        s = _sim(amd, E, A, step_groups=groups)
        d_act = _armed(s, E, A)
        acts = _crash_actions(T, E * A)
        out = None
        for t in range(T):
            d_act.upload(acts[t])
            s.step_device(d_act)
            s.step_device(d_act)                       # back to back: the second may go out as two blocks
            out = s.encode_obs_device(enc, out)
            s.step_device(d_act)                       # a step right behind the encode keeps its blocks
            assert s.step_groups()[2] == groups, "step %d went out as %d block(s)" % (t, s.step_groups()[2])
            out = s.encode_obs_device(enc, out)
        stacks.append((out.download(), _everything(s)))
        s.close()
    _same_bits(stacks[0][0], stacks[1][0], "two blocks against one")
    for k in stacks[0][1]:
        assert np.array_equal(stacks[0][1][k], stacks[1][1][k], equal_nan=True), k


@pytest.mark.parametrize("form", ["step_device", "step_host", "two_blocks"])
def test_encoding_changes_nothing_in_the_simulation(amd, form):
    E, A, T = 128, 2, 100
    enc = amd.ObsEncoder(sectors=108, pool="mean", features=FIVE, frames=4, scales=SCALES)
    acts = _crash_actions(T, E * A)
    res = []
    for with_enc in (False, True):
        s = _sim(amd, E, A, step_groups=2 if form == "two_blocks" else 0)
        if form == "step_host":
            s.episode_init(0)
            s.episode_reset(bench_start_poses(E, A))
            hb = s.host_block(["state", "scans", "done"])
            pinned = s.pinned_empty(enc.shape(E * A), np.float32)
        else:
            d_act = _armed(s, E, A)
        for t in range(T):
            if form == "step_host":
                hb.actions[...] = acts[t]
                s.step_host(hb, None, auto_reset=True, sync=not with_enc)
                if with_enc:
                    out = s.encode_obs_device(enc, pinned=pinned)
                    s.sync()
            else:
                d_act.upload(acts[t])
                s.step_device(d_act)
                if with_enc:
                    s.encode_obs_device(enc)
        o = _everything(s)
        if form == "step_host":
            o["hb_state"], o["hb_scans"], o["hb_done"] = (np.array(hb.views[k], copy=True) for k in ("state", "scans", "done"))
            if with_enc:
                _same_bits(pinned, out.download(), "the page-locked copy")
        res.append(o)
        s.close()
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k], equal_nan=True), "%s: %s differs with an encode after every step" % (form, k)


# ---- the vector envs -----------------------------------------------------------------------------------------------------------
def _vec(amd, E, enc, **kw):
    return amd.F110VecEnv(E, auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png", track=CSV, obs_encoder=enc, **kw)


def test_vec_env_encoded_obs_follow_model(amd):
    E, A, T = 48, 2, 80
    enc = amd.ObsEncoder(sectors=36, pool="min", features=ref.FEATURES, frames=4, scales=SCALES)
    env, env2 = _vec(amd, E, enc), _vec(amd, E, dict(sectors=36, pool="min", features=ref.FEATURES, frames=4, scales=SCALES))
    start = bench_start_poses(E, A).reshape(E, A, 3)
    obs = env.reset(start)[0]
    env2.reset(start)
    assert obs["encoded"].shape == (E, A, 4, enc.dim) and obs["encoded"].dtype == np.float32 and "encoded" in env.obs_fields
    assert tuple(env.encoded_stack.shape) == enc.shape(E * A)
    b = env.sim.batch
    stack = ref.encode(enc, *_columns(b, True), np.zeros(enc.shape(E * A), np.float32), fill=True)
    _same_bits(obs["encoded"].reshape(stack.shape), stack, "reset")
    acts = _crash_actions(T, E * A, seed=8).reshape(T, E, A, 2)
    dones = 0
    for t in range(T):
        view = env.step(acts[t])[0]["encoded"]
        assert view is obs["encoded"]                      # a persistent view of page-locked memory
        stack = ref.encode(enc, *_columns(b, True), stack)
        _same_bits(view.reshape(stack.shape), stack, "step %d" % t)
        _same_bits(env.encoded_stack.download(), stack, "device stack, step %d" % t)
        env2.step_async(acts[t])
        o2, _, d2, _ = env2.step_wait()
        _same_bits(o2["encoded"], view, "step_async / step_wait, step %d" % t)
        dones += int(np.sum(d2))
    assert dones > 5
    # obs_fields without 'encoded': nothing is encoded; with it alone: only that
    lean = _vec(amd, 4, enc, obs_fields=("poses_x",))
    assert "encoded" not in lean.reset(bench_start_poses(4, A).reshape(4, A, 3))[0] and lean.encoded_stack is None
    only = _vec(amd, 4, enc, obs_fields=("encoded",))
    assert sorted(k for k in only.reset(bench_start_poses(4, A).reshape(4, A, 3))[0]) == ["ego_idx", "encoded", "lap_counts", "lap_times"]


def test_vec_env_snapshot_restore_reproduces_encoded_obs(amd):
    E, A = 32, 2
    enc = amd.ObsEncoder(sectors=36, pool="mean", features=FIVE, frames=4, scales=SCALES)
    env = _vec(amd, E, enc)
    env.reset(bench_start_poses(E, A).reshape(E, A, 3))
    acts = _crash_actions(70, E * A, seed=9).reshape(70, E, A, 2)
    for t in range(10):
        env.step(acts[t])
    snap = env.snapshot()
    assert "encoded_stack" in snap and snap["encoded_stack"].shape == enc.shape(E * A)
    first = [np.array(env.step(acts[10 + t])[0]["encoded"], copy=True) for t in range(30)]
    last = env.restore(snap)
    _same_bits(last[0]["encoded"].reshape(-1), snap["encoded_stack"].reshape(-1), "the restored observation")
    for t in range(30):
        _same_bits(env.step(acts[10 + t])[0]["encoded"], first[t], "step %d after restore" % t)
    plain = amd.F110VecEnv(E, auto_reset=True, device_logic=True, map=map_stem("example_map"), map_ext=".png", track=CSV)
    plain.reset(bench_start_poses(E, A).reshape(E, A, 3))
    assert sorted(plain.snapshot()) == ["host", "sim"]     # snapshots taken without an encoder keep their keys


def test_sharded_equals_one_handle(amd):
    E, A, T = 30, 2, 40
    kw = dict(auto_reset=True, map=map_stem("example_map"), map_ext=".png", track=CSV,
              obs_encoder=dict(sectors=27, pool="min", features=ref.FEATURES, frames=3, scales=SCALES))
    one = amd.F110VecEnv(E, device_logic=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], shard_sizes=[7, 12, 11], **kw)
    start = bench_start_poses(E, A).reshape(E, A, 3)
    _same_bits(sh.reset(start)[0]["encoded"], one.reset(start)[0]["encoded"], "reset")
    acts = _crash_actions(T, E * A, seed=10).reshape(T, E, A, 2)
    for t in range(T):
        a, b = sh.step(acts[t]), one.step(acts[t])
        assert a[0]["encoded"].shape == (E, A, 3, 35)
        _same_bits(a[0]["encoded"], b[0]["encoded"], "step %d" % t)
        assert np.array_equal(a[2], b[2])
    sh.close()


def test_torch_consumer_in_a_fresh_process():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tests", "obs_encoder_torch_worker.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    if "SKIP" in out.stdout:
        pytest.skip(out.stdout.strip().splitlines()[-1])
    assert "OBS ENCODER TORCH OK" in out.stdout, out.stdout[-2000:]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_output_untouched(amd):
    from f1tenth_gym_amd import _ffi
    E, A = 8, 2
    N = E * A
    s = _sim(amd, E, A)
    s.reset(bench_start_poses(E, A))
    s.step(np.zeros((N, 2)))
    L = _ffi.lib()
    good = amd.ObsEncoder(sectors=108, features=FIVE, frames=4, scales=SCALES)
    out = s.device_array((N * 4 * good.dim + 64,), np.float32)
    sentinel = np.random.default_rng(1).normal(size=out.shape).astype(np.float32)
    out.upload(sentinel)
    other = np.zeros(good.shape(N), np.float32)            # ordinary host memory: not f110_host_alloc's

    def call(ptr=None, pinned=None, **fields):
        sp = good.spec()
        for k, v in fields.items():
            if k == "feat0":
                sp.feat_scale[0] = v
            else:
                setattr(sp, k, v)
        return L.f110_obs_encode_device(s._h, C.byref(sp), out.ptr if ptr is None else ptr, pinned)

    bad = [dict(beam_lo=-1, beam_hi=100), dict(beam_lo=0, beam_hi=1081), dict(beam_lo=500, beam_hi=500), dict(beam_lo=600, beam_hi=200),
           dict(beam_lo=0, beam_hi=100, sectors=101), dict(sectors=-1), dict(sectors=1081), dict(pool=3), dict(pool=-1), dict(features=256 | 1),
           dict(frames=0), dict(frames=17), dict(flags=2), dict(range_clip=0.0), dict(range_clip=float("nan")), dict(range_clip=float("inf")),
           dict(range_scale=-1.0), dict(range_scale=float("inf")), dict(feat0=0.0), dict(feat0=float("nan")), dict(feat0=float("inf")),
           dict(sectors=0, features=0), dict(sectors=1080, frames=8)]
    for f in bad:
        assert call(**f) == _ffi.ERR_INVALID, f
        assert _ffi.last_error(s._h), f
    assert call(ptr=0) == _ffi.ERR_INVALID and call(ptr=out.ptr + 4) == _ffi.ERR_INVALID        # null, misaligned
    assert L.f110_obs_encode_device(s._h, None, out.ptr, None) == _ffi.ERR_INVALID
    assert call(pinned=other.ctypes.data) == _ffi.ERR_INVALID                                     # not page-locked memory of the library
    small = s.pinned_empty((N * 4 * good.dim - 1,), np.float32)
    assert call(pinned=small.ctypes.data) == _ffi.ERR_INVALID                                     # ... or too small a block of it
    assert call(features=31 | 32) == _ffi.ERR_STATE and call(features=128) == _ffi.ERR_STATE      # track features, tracking off
    s.sync()
    assert np.array_equal(out.download().view(np.uint32), sentinel.view(np.uint32)), "a refused call wrote the output buffer"
    with pytest.raises(ValueError):
        s.encode_obs_device(good, out=s.device_array((N, 4, good.dim + 1), np.float32))
    with pytest.raises(ValueError):
        s.encode_obs_device(amd.ObsEncoder(sectors=8, beams=(0, 2000)))
    assert call() == _ffi.OK                                                                     # and the good spec goes through
    s.sync()
    got = out.download()
    assert not np.array_equal(got[:N * 4 * good.dim], sentinel[:N * 4 * good.dim]) and np.array_equal(got[N * 4 * good.dim:], sentinel[N * 4 * good.dim:])
    # the unit form refuses the same way and leaves the caller's array alone
    st = sentinel[:N * 4 * good.dim].reshape(good.shape(N)).copy()
    sp = good.spec()
    sp.frames = 17
    scans, cols, sc = _columns(s, False)
    assert L.f110_obs_encode_batch(s._h, C.byref(sp), _ffi.dptr(scans), _ffi.dptr(cols), _ffi.i32ptr(sc), N, st.ctypes.data) == _ffi.ERR_INVALID
    assert np.array_equal(st.view(np.uint32).reshape(-1), sentinel[:N * 4 * good.dim].view(np.uint32))
    s.close()
