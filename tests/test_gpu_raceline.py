"""The raceline and speed profile on the device (f110_raceline_batch, BatchSim.raceline) against the NumPy restatement
(tests/raceline_ref.py; tests/test_raceline_host.py holds the restatement's own conditions on the CPU): every output array_equal.

(1) the workgroup's edges at levels = 0 and both of the kernel's sizes, with both sizes of its beta table.
(2) levels and iteration counts.
(3) batching: lines of different lengths in one call, each equal to its own call.
(4) bounds: no room anywhere, on one half, a margin beyond every width, straights of exactly zero curvature.
(5) refusals leave the outputs and the device allocations as they were.
(6) ordering around two-block steps.
(7) BatchSim.raceline's Tracks, the env layers, the preview's vx channel, clearance on carved slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

import obstacles_ref as oref
import raceline_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAPS = os.path.join(ROOT, "tests", "golden", "maps")
OUT = ('alpha', 'xy', 'kappa', 'vx')


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


@pytest.fixture(scope="module")
def sim(amd):
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(oref.small_image(), oref.SMALL_RES, list(oref.SMALL_ORIGIN))
    yield s
    s.close()


def _want(q, w, sp):
    return ref.raceline(q, w, **{k: v for k, v in sp.items() if k != 'spacing'})


def _solve(s, lines, sp, line_iters=None):
    """BatchSim.raceline_batch -> one dict per line"""
    alpha, xy, kappa, vx, length, lap = s.raceline_batch(lines, sp, line_iters)
    out, o = [], 0
    for t, (q, w) in enumerate(lines):
        a = slice(o, o + q.shape[0])
        out.append(dict(alpha=alpha[a], xy=xy[a], kappa=kappa[a], vx=vx[a], length=float(length[t]), lap_time=float(lap[t])))
        o += q.shape[0]
    return out


def _same(got, want, what):
    for k in OUT:
        assert np.array_equal(got[k], want[k]), "%s: %s differs in %d of %d values" % (what, k, int((got[k] != want[k]).sum()), want[k].size)
    assert got['length'] == want['length'] and got['lap_time'] == want['lap_time'], what
    assert not any(np.isnan(got[k]).any() for k in OUT)


# ---- 1. the workgroup's edges --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [8, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096])
def test_workgroup_edges_at_one_level(sim, M):
    q, w = ref.ellipse(M, a=max(12.0, 0.08 * M), b=max(7.0, 0.05 * M))     # (stations ~0.4 m apart from M = 150 on)
    sp = ref.spec(levels=0, iters=12)
    _same(_solve(sim, [(q, w)], sp)[0], _want(q, w, sp), "M = %d" % M)


@pytest.mark.parametrize("M,levels,iters", [(64, 0, 512), (64, 0, 513), (1040, 2, 512), (1040, 2, 513), (72, 1, 4096)])
def test_beta_table_sizes(sim, M, levels, iters):
    """the kernel is built for 512 and for 4096 entries of beta, and for 256 and 1024 lanes: either side of both thresholds"""
    q, w = ref.ellipse(M)
    sp = ref.spec(levels=levels, iters=iters)
    _same(_solve(sim, [(q, w)], sp)[0], _want(q, w, sp), "M = %d, iters = %d" % (M, iters))


# ---- 2. levels and iteration counts --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("levels", [1, 2, 3, 4, 5, 6])
def test_levels_at_the_smallest_legal_line(sim, levels):
    q, w = ref.ellipse(8 << levels)
    sp = ref.spec(levels=levels, iters=25)
    got = _solve(sim, [(q, w)], sp)[0]
    _same(got, _want(q, w, sp), "levels = %d" % levels)
    assert np.abs(got['alpha']).max() > 0.0


def test_four_levels_at_the_longest_line(sim):
    q, w = ref.ellipse(4096, a=300.0, b=180.0)
    sp = ref.spec()
    _same(_solve(sim, [(q, w)], sp)[0], _want(q, w, sp), "M = 4096 at the defaults")


@pytest.mark.parametrize("iters", [0, 1, 2, 200])
def test_iteration_counts(sim, iters):
    q, w = ref.ellipse(336, a=25.0, b=15.0)
    sp = ref.spec(iters=iters)
    got = _solve(sim, [(q, w)], sp)[0]
    _same(got, _want(q, w, sp), "iters = %d" % iters)
    assert (iters == 0) == (not got['alpha'].any())


# ---- 3. batching ---------------------------------------------------------------------------------------------------------------
def test_lines_of_different_lengths_in_one_call(sim):
    sp = ref.spec(levels=3, iters=40)
    lines = [ref.ellipse(64), ref.ellipse(1048, a=60.0, b=45.0), ref.ellipse(336, a=25.0, b=15.0, phase=1.3), ref.ellipse(128, width=0.2), ref.ellipse(72, phase=2.0)]
    iters = [40, 40, 0, 40, 7]
    got = _solve(sim, lines, sp, iters)
    for t, (q, w) in enumerate(lines):
        # (a line's iteration count below the spec's reads the head of the spec's table: beta depends on k alone)
        _same(got[t], _want(q, w, dict(sp, iters=iters[t])), "line %d of 5" % t)
        _same(_solve(sim, [(q, w)], sp, [iters[t]])[0], got[t], "line %d alone" % t)
    # the small lines alone take the small kernel: the same bits
    small = [lines[0], lines[3], lines[4]]
    for g, t in zip(_solve(sim, small, sp, [40, 40, 7]), (0, 3, 4)):
        _same(g, got[t], "line %d among the short ones" % t)


# ---- 4. bounds -----------------------------------------------------------------------------------------------------------------
def test_bounds(sim):
    q, w = ref.ellipse(336, a=25.0, b=15.0)
    sp = ref.spec()
    centre = _solve(sim, [(q, w)], ref.spec(iters=0))[0]
    shut = _solve(sim, [(q, np.full(336, 0.25))], sp)[0]                 # b = 0 everywhere
    assert shut['xy'].tobytes() == q.tobytes() and not shut['alpha'].any()
    assert np.array_equal(shut['vx'], centre['vx']) and shut['lap_time'] == centre['lap_time']
    _same(shut, _want(q, np.full(336, 0.25), sp), "b = 0")
    half = w.copy()
    half[:168] = 0.3                                                     # b = 0 on one half (w - margin = 0 exactly)
    got = _solve(sim, [(q, half)], sp)[0]
    _same(got, _want(q, half, sp), "b = 0 on one half")
    assert not got['alpha'][:168].any() and np.abs(got['alpha'][168:]).max() > 0.1 and np.array_equal(got['xy'][:168], q[:168])
    wide = _solve(sim, [(q, w)], ref.spec(margin=5.0))[0]                # a margin beyond every half width
    assert wide['xy'].tobytes() == q.tobytes()
    _same(wide, _want(q, w, ref.spec(margin=5.0)), "margin 5")


def test_straights_of_zero_curvature(sim):
    q, w = ref.stadium(40, 24, width=0.3)        # no room: the straights stay straight, kappa is exactly 0 inside them
    sp = ref.spec(levels=3, iters=30)
    got = _solve(sim, [(q, w)], sp)[0]
    _same(got, _want(q, w, sp), "stadium")
    inside = np.r_[2:38, 66:102]
    assert not got['kappa'][inside].any() and got['vx'].max() == 8.0 and np.all(got['vx'] > 0.0)
    assert np.all(np.isfinite(got['vx'])) and np.isfinite(got['lap_time'])
    q, w = ref.stadium(40, 24, width=1.5)        # with room the line cuts the bends; still no NaN
    got = _solve(sim, [(q, w)], sp)[0]
    _same(got, _want(q, w, sp), "stadium with room")
    assert got['lap_time'] < _solve(sim, [(q, w)], sp, [0])[0]['lap_time']


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_everything_as_it_was(amd, sim):
    from f1tenth_gym_amd import _ffi
    from f1tenth_gym_amd.raceline import momentum
    L = _ffi.lib()
    dp, ip = (lambda a: a.ctypes.data_as(_ffi._dp)), (lambda a: a.ctypes.data_as(_ffi._i32p))
    q, w = ref.ellipse(64)
    beta = momentum(4096)
    outs = [np.full(n, 7.5) for n in (8192, 16384, 8192, 8192, 4, 4)]
    sim.sync()
    allocs = amd.device_allocs()

    def call(q=q, w=w, off=None, T=1, levels=3, iters=5, margin=0.3, v_max=8.0, a_lat=7.0, a_accel=7.0, a_brake=8.0, beta=beta, li=None, h=sim._h, o=outs):
        off = np.array([0, 64 if w is None else w.shape[0]], dtype=np.int32) if off is None else np.asarray(off, dtype=np.int32)
        return L.f110_raceline_batch(h, None if q is None else dp(q), None if w is None else dp(w), ip(off), T, levels, iters, margin, v_max, a_lat, a_accel, a_brake,
                                     None if beta is None else dp(beta), None if li is None else ip(np.asarray(li, dtype=np.int32)),
                                     *[None if a is None else dp(a) for a in o])
    nanq, infw, nanb = q.copy(), w.copy(), beta.copy()
    nanq[5, 1], infw[9], nanb[3] = np.nan, np.inf, np.nan
    twin = q.copy()
    twin[11] = twin[9]
    dup = np.ascontiguousarray(np.concatenate([q[:20], q[19:63]]))
    big = ref.ellipse(4097)
    cases = [("nan point", dict(q=nanq)), ("inf width", dict(w=infw)), ("nan beta", dict(beta=nanb)), ("M not a multiple", dict(q=q[:60], w=w[:60])),
             ("fewer than 8 coarse stations", dict(q=q[:56], w=w[:56])), ("M > 4096", dict(q=big[0], w=big[1], levels=0)), ("levels -1", dict(levels=-1)),
             ("levels 7", dict(levels=7)), ("iters -1", dict(iters=-1)), ("iters 4097", dict(iters=4097)), ("v_max 0", dict(v_max=0.0)), ("v_max inf", dict(v_max=np.inf)),
             ("a_lat nan", dict(a_lat=np.nan)), ("a_accel -1", dict(a_accel=-1.0)), ("a_brake 0", dict(a_brake=0.0)), ("margin -0.1", dict(margin=-0.1)),
             ("margin nan", dict(margin=np.nan)), ("no normal", dict(q=twin, levels=0)), ("T = 0", dict(T=0)), ("offsets[0]", dict(off=[1, 65])),
             ("a line's iters beyond the spec's", dict(li=[6])), ("a line's iters < 0", dict(li=[-1])), ("null points", dict(q=None)), ("null widths", dict(w=None)),
             ("null beta", dict(beta=None)), ("second line bad", dict(q=np.concatenate([q, q[:60]]), w=np.concatenate([w, w[:60]]), off=[0, 64, 124], T=2)),
             ("zero-length raceline segment", dict(q=dup, levels=0, iters=0)),       # (every normal exists: the device decides, after the solve)
             ("zero-length segment, second line", dict(q=np.concatenate([q, dup]), w=np.concatenate([w, w]), off=[0, 64, 128], T=2, levels=0, li=[5, 0]))]
    for name, kw in cases:
        assert call(**kw) == _ffi.ERR_INVALID, name
        assert _ffi.last_error(sim._h), name
        assert all(np.all(a == 7.5) for a in outs), name
        assert amd.device_allocs() == allocs, name
    assert "zero length" in _ffi.last_error(sim._h)
    for k in range(6):
        assert call(o=[None if j == k else a for j, a in enumerate(outs)]) == _ffi.ERR_INVALID
    assert call(h=None) == _ffi.ERR_INVALID and all(np.all(a == 7.5) for a in outs)
    # ... and the same arguments without the fault are taken (iters = 0 needs no beta)
    assert call() == _ffi.OK and call(iters=0, beta=None) == _ffi.OK and np.all(outs[0][64:] == 7.5) and not np.all(outs[3][:64] == 7.5)
    assert amd.device_allocs() == allocs
    with pytest.raises(ValueError):
        sim.raceline_batch([(q[:60], w[:60])], ref.spec(levels=3))
    with pytest.raises(ValueError):
        sim.raceline_batch([], None)
    with pytest.raises(ValueError, match="no track"):
        sim.raceline(0)


# ---- 6. ordering ---------------------------------------------------------------------------------------------------------------
def test_a_call_between_two_block_steps(amd):
    from f1tenth_gym_amd import random_track, TrackMap
    tr = random_track(2)
    tm = TrackMap(tr)
    E, A = 256, 2
    rng = np.random.default_rng(4)
    xy, tan = tr.point_at(rng.uniform(0.0, tr.length, E * A))
    poses = np.column_stack([xy, np.arctan2(tan[:, 1], tan[:, 0])])
    acts = np.stack([rng.uniform(-0.2, 0.2, E * A), rng.uniform(0.5, 3.0, E * A)], axis=1)
    sp = ref.spec(iters=30)
    line = ref.stations(tr)
    want = _want(*line, sp)
    out = []
    for synced in (False, True):
        s = amd.BatchSim(num_envs=E, num_agents=A, step_groups=2)
        s.set_map_image(oref.small_image(), oref.SMALL_RES, list(oref.SMALL_ORIGIN))
        d = s.add_track_map(tm)
        s.set_env_maps([d] * E)
        s.reset(poses)
        d_act = s.device_array((E * A, 2))
        d_act.upload(acts)
        s.step_device(d_act)
        s.step_device(d_act)
        if synced:
            s.sync()
        assert s.step_groups()[2] == 2
        _same(_solve(s, [line], sp)[0], want, "behind two-block steps (synced: %r)" % synced)
        s.step_device(d_act)          # ... and a step right behind the call
        assert s.step_groups()[2] == 2
        o = s.get("state", "scans", "collisions")
        out.append({k: np.array(v, copy=True) for k, v in o.items()})
        d_act.free()
        s.close()
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k


# ---- 7. the Python layers ------------------------------------------------------------------------------------------------------
def test_batchsim_raceline_returns_tracks(amd, sim):
    from f1tenth_gym_amd import random_track, Raceline, Track
    tracks = [random_track(1, 8.0, 1.0), random_track(2, 20.0, 1.2)]
    got = sim.raceline(tracks)
    assert isinstance(got, list) and len(got) == 2
    for tr, rl in zip(tracks, got):
        q, w = ref.stations(tr)
        want, centre = ref.raceline(q, w), ref.raceline(q, w, iters=0)
        assert rl.closed and rl.attr_names == ('kappa', 'vx', 'offset') and np.array_equal(rl.xy, want['xy'])
        assert np.array_equal(rl.attrs, np.stack([want['kappa'], want['vx'], want['alpha']], axis=1))
        assert rl.lap_time == want['lap_time'] and rl.center_lap_time == centre['lap_time'] and rl.length == want['length']
        assert rl.center.attr_names == ('half_width', 'kappa', 'vx') and np.array_equal(rl.center.xy, q)
        assert np.array_equal(rl.center.attrs, np.stack([w, centre['kappa'], centre['vx']], axis=1))
        assert rl.lap_time < rl.center_lap_time
    one = sim.raceline(tracks[0], dict(iters=50))
    assert isinstance(one, Track) and np.array_equal(one.xy, _want(*ref.stations(tracks[0]), ref.spec(iters=50))['xy'])
    assert np.array_equal(tracks[0].raceline(sim, Raceline(iters=50)).attrs, one.attrs)
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(oref.small_image(), oref.SMALL_RES, list(oref.SMALL_ORIGIN))
    slot = s.add_track_map(tracks[0])
    by_slot = s.raceline(slot)
    assert np.array_equal(by_slot.xy, got[0].xy) and np.array_equal(by_slot.attrs, got[0].attrs)
    mixed = s.raceline([slot, tracks[1]])
    assert np.array_equal(mixed[0].xy, got[0].xy) and np.array_equal(mixed[1].attrs, got[1].attrs)
    with pytest.raises(ValueError, match="half_width"):
        s.raceline(Track(tracks[0].xy))
    # a slot carved narrower than its line's column: the slot's raceline stays inside what was carved
    from f1tenth_gym_amd import TrackMap
    tm = TrackMap(tracks[0], half_width=0.5)
    narrow = s.raceline(s.add_track_map(tm))
    assert np.array_equal(narrow.xy, ref.raceline(*ref.stations(tm.carved_line()))['xy']) and np.abs(narrow.attrs[:, 2]).max() <= 0.2
    s.close()


def _kw(name="berlin", agents=1):
    return dict(map=os.path.join(MAPS, name), map_ext=".png", num_agents=agents)


def test_env_layers_on_a_map(amd):
    """track='raceline' on berlin: the three layers hold BatchSim.raceline(Track.from_map(...)); the preview's attr1 is vx"""
    E = 3
    cl, rs = dict(spacing=0.25, smooth=0.8), dict(iters=60, margin=0.35)
    pv = amd.TrackPreview(points=6, offset=0.5, spacing=1.5, channels=("x", "y", "attr0", "attr1"), frame="world")
    a = amd.F110VecEnv(E, device_logic=True, track='raceline', centerline=cl, raceline=rs, track_preview=pv, reward='progress', **_kw())
    line = amd.Track.from_map(a, 0, **cl)
    want = a.sim.batch.raceline(line, rs)
    q, w = ref.stations(line)
    r = _want(q, w, ref.spec(**rs))
    rl = a.tracks[0]
    assert a.raceline_slots == {0} and rl.attr_names == ('kappa', 'vx', 'offset')
    assert np.array_equal(rl.xy, want.xy) and np.array_equal(rl.attrs, want.attrs) and np.array_equal(rl.xy, r['xy']) and np.array_equal(rl.attrs[:, 1], r['vx'])
    assert rl.lap_time == r['lap_time'] < rl.center_lap_time
    xy, tan = rl.point_at(np.array([1.0, 20.0, 40.0]))
    poses = np.column_stack([xy, np.arctan2(tan[:, 1], tan[:, 0])]).reshape(E, 1, 3)
    o = a.reset(poses)[0]
    o = a.step(np.tile([0.0, 2.0], (E, 1, 1)))[0]
    p = np.column_stack([np.asarray(o[k]).reshape(-1) for k in ("poses_x", "poses_y", "poses_theta")])
    got = np.asarray(o["track_preview"]).reshape(E, 6, 4)
    model = rl.preview(p, np.asarray(o["progress"]).reshape(-1), pv)
    assert np.array_equal(got, model) and got[..., 3].min() > 0.0 and got[..., 3].max() <= 8.0
    first = {k: np.array(np.asarray(o[k]), copy=True) for k in ("progress", "lateral_offset", "track_preview")}
    a.sim.batch.close()
    sh = amd.ShardedVecEnv(E, devices=[0, 0, 0], track='raceline', centerline=cl, raceline=rs, track_preview=pv, reward='progress', **_kw())
    assert all(np.array_equal(k.tracks[0].xy, rl.xy) and np.array_equal(k.tracks[0].attrs, rl.attrs) for k in sh.shards)
    sh.reset(poses)
    o = sh.step(np.tile([0.0, 2.0], (E, 1, 1)))[0]
    for k, v in first.items():
        assert np.array_equal(np.asarray(o[k]).reshape(v.shape), v), k
    sh.close()
    one = amd.F110Env(track='raceline', centerline=cl, raceline=rs, reward='progress', **_kw())
    assert np.array_equal(one.track.xy, rl.xy) and np.array_equal(one.track.attrs, rl.attrs)
    one.sim.batch.close()
    with pytest.raises(ValueError):
        amd.F110VecEnv(E, device_logic=True, track='raceline', raceline=dict(iters=-1), **_kw())


def test_env_layers_on_carved_slots_and_clearance(amd):
    """tracks={slot: 'raceline'} on track_maps slots: the carved line with the half widths it was CARVED with is the source (not the
    line's own column, which half_width= may override and which a varying column is not carved at), set_track_map solves the new
    line's, and every station of the raceline keeps `margin` from the carved walls (less the raster's sqrt(2) cells)"""
    from f1tenth_gym_amd import random_track, TrackMap
    frame = dict(origin=(-15.0, -15.0, 0.0), shape=(480, 480))       # one frame for the three lines (radius 8: within 14 m of the origin)
    tms = [TrackMap(random_track(seed), **frame) for seed in (1, 2, 3)]
    margin = 0.3
    env = amd.F110VecEnv(3, device_logic=True, track_maps=tms[:2], tracks={1: 'raceline', 2: 'raceline'}, env_map=[1, 2, 1], **_kw("example_map"))
    assert env.raceline_slots == {1, 2}

    def check(slot, tm, env=env):
        b = env.sim.batch
        rl = env.tracks[slot]
        hw = np.asarray(tm.widths())
        q, w = ref.stations(amd.Track(tm.track.xy, attrs={'half_width': np.minimum(hw, np.roll(hw, 1))}))
        want = ref.raceline(q, w)
        assert np.array_equal(rl.xy, want['xy']) and np.array_equal(rl.attrs, np.stack([want['kappa'], want['vx'], want['alpha']], axis=1))
        assert b.tracks[slot] is rl and rl.lap_time < rl.center_lap_time
        table = b.get_map_dt(slot)
        res, ox, oy, oc, os_ = b.slot_frame(slot)
        assert oc == 1.0 and os_ == 0.0
        c, r = np.floor((rl.xy[:, 0] - ox) / res).astype(int), np.floor((rl.xy[:, 1] - oy) / res).astype(int)
        clear = table[r, c]
        print("slot %d: clearance %.4f m at the worst station, %.4f m asked" % (slot, clear.min(), margin - np.sqrt(2.0) * res))
        assert np.all(clear >= margin - np.sqrt(2.0) * res)
        return rl
    check(1, tms[0])
    check(2, tms[1])
    env.set_track_map(1, tms[2])
    check(1, tms[2])
    check(2, tms[1])
    o = env.reset(np.array([[list(env.tracks[m].xy[5]) + [0.0]] for m in (1, 2, 1)]))[0]
    assert np.all(np.abs(np.asarray(o["lateral_offset"])) < 0.05)
    env.sim.batch.close()
    # a half_width= narrower than the line's column (1.0), and a column that varies (carved at each segment's mean, so narrower
    # than the column at its local maxima): the offsets stay inside what was carved
    tr = random_track(1)
    col = 1.0 + 0.3 * np.sin(np.arange(tr.num_points) * 0.9)
    odd = [TrackMap(tr, half_width=0.5, **frame), TrackMap(amd.Track(tr.xy, attrs={'half_width': col}), **frame)]
    env = amd.F110VecEnv(2, device_logic=True, track_maps=odd[:2], tracks={1: 'raceline', 2: 'raceline'}, env_map=[1, 2], **_kw("example_map"))
    narrow = check(1, odd[0], env)
    assert np.abs(narrow.attrs[:, 2]).max() <= 0.5 - margin and np.all(narrow.center.attrs[:, 0] == 0.5)
    wavy = check(2, odd[1], env)
    at_stations = np.interp(np.arange(wavy.num_points) * tr.length / wavy.num_points, np.r_[tr.cum, tr.length], np.r_[col, col[0]])
    assert np.any(wavy.center.attrs[:, 0] < at_stations - 0.02)      # (narrower than the column where the column peaks)
    env.set_track_map(2, odd[0])
    assert np.array_equal(check(2, odd[0], env).xy, narrow.xy)
    env.sim.batch.close()
    # a line carved with widths of its own and no column: per point the smaller of its two segments' half widths
    hw = np.where(np.arange(tr.num_segments) % 7 < 3, 0.8, 1.0)
    bare = TrackMap(amd.Track(tr.xy), half_width=hw)
    one = amd.F110Env(track_map=bare, track='raceline', **_kw("example_map"))
    src = amd.Track(tr.xy, attrs={'half_width': np.minimum(hw, np.roll(hw, 1))})
    assert np.array_equal(one.track.xy, ref.raceline(*ref.stations(src))['xy'])
    one.sim.batch.close()


def test_example_runs():
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "raceline.py"), "--iters", "100"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                          text=True, timeout=120)
    assert proc.returncode == 0 and "lap completed" in proc.stdout, proc.stdout[-3000:]
