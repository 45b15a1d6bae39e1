"""Track progress on the device (include/f110.h f110_track_*, BatchSim.set_track / enable_track / track_views / get_track, the
track= / reward='progress' options of the env layers): the projection is the reference's nearest_point_on_trajectory
(examples/waypoint_follow.py:15-50, the oracle's orc_nearest_on_trajectory) bit for bit, on every step path, and the progress
of a step stays s(post) - s(pre) whatever wrote the pose in between."""
import os
import subprocess
import sys

import numpy as np
import pytest

from _util import MAPS, bench_start_poses, check_track_winner, load_map_image, map_stem, raceline, track_oracle as _oracle

pytestmark = pytest.mark.gpu

SEED, STD = 12345, 0.01
L_EXAMPLE = 156.35612
CSV = os.path.join(MAPS, "example_waypoints.csv")


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _track(amd, xy=None, closed=True):
    return amd.Track.from_xy(raceline()[:, 1:3] if xy is None else xy, closed=closed)


def _check_cols(got, want, what=""):
    """segment and t (unit form) exact; s and lateral exact (the same float64 operations); heading_error to 1e-12"""
    np.testing.assert_array_equal(got[:, 3], want[:, 3], err_msg=what + " segment")
    np.testing.assert_array_equal(got[:, 0], want[:, 0], err_msg=what + " s")
    np.testing.assert_array_equal(got[:, 1], want[:, 1], err_msg=what + " lateral")
    herr_g, herr_w = got[:, 2], want[:, 2]
    d = np.abs(np.mod(herr_g - herr_w + np.pi, 2 * np.pi) - np.pi)   # (+-pi are the same angle)
    assert np.all(d <= 1e-12 * np.maximum(1.0, np.abs(herr_w))), what + " heading_error"


def _cols(tr):
    return np.column_stack([tr["s"], tr["lateral"], tr["heading_error"], tr["segment"].astype(np.float64)])


def _sim(amd, E, A=2, track=None, enable=True, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    s.set_map_image(*load_map_image("example_map"))
    s.set_noise_rng(SEED, STD)
    if track is not None:
        s.set_track(track)
        if enable:
            s.enable_track()
    return s


def _actions(T, N, seed=7, vmax=8.0):
    rng = np.random.default_rng(seed)
    return np.stack([rng.uniform(-0.4, 0.4, (T, N)), rng.uniform(2.0, vmax, (T, N))], axis=2)


def _poses_of(s):
    return s.get("agent_poses")["agent_poses"]


# ------------------------------------------------------------------ unit parity (f110_track_project_batch)
def _wiggly_loop(n):
    a = np.linspace(0.0, 2 * np.pi, n, endpoint=False)
    r = 10.0 + 0.7 * np.sin(7 * a) + 0.3 * np.cos(13 * a)
    return np.column_stack([r * np.cos(a), r * np.sin(a)])


def _mixed_polyline(rng, n, closed=False):
    """n + 1 points whose segment lengths are log-uniform over 1 mm .. 50 m, turning by up to 2 rad at each vertex"""
    ln = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), n))
    ang = np.cumsum(rng.uniform(-2.0, 2.0, n))
    xy = np.vstack([[0.0, 0.0], np.cumsum(np.column_stack([ln * np.cos(ang), ln * np.sin(ang)]), axis=0)])
    return xy[:-1] if closed else xy


def _ngon(n, r=3.0, c=(0.0, 0.0)):
    a = 2 * np.pi * np.arange(n) / n
    return np.column_stack([c[0] + r * np.cos(a), c[1] + r * np.sin(a)])


UNIT_CASES = ["vertices", "equidistant", "far", "raceline", "big5000", "open", "closed_square", "lds1023", "lds1024", "lds1025",
              "open2", "closed3", "mixed", "shift1e5", "shift1e6", "ngon37_centre", "shared_vertices", "nan_pose"]


@pytest.mark.parametrize("case", UNIT_CASES)
def test_unit_parity_vs_oracle(amd, case):
    rng = np.random.default_rng(5)
    sq = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]])
    if case.startswith("lds"):   # both sides of the LDS staging limit (kTrackLdsSegs = 1024 segments)
        t = _track(amd, _wiggly_loop(int(case[3:])))
        poses = np.column_stack([rng.uniform(-12, 12, (2048, 2)), rng.uniform(-7, 7, 2048)])
        poses[:256, :2] = t.xy[rng.integers(0, t.num_points, 256)] + rng.normal(0, 1e-3, (256, 2))
    elif case == "open2":       # 2 segments, 14 idle lanes
        t = _track(amd, np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 2.0]]), closed=False)
        poses = np.column_stack([rng.uniform(-2, 3, (1024, 2)), rng.uniform(-7, 7, 1024)])
    elif case == "closed3":
        t = _track(amd, np.array([[0.0, 0.0], [3.0, 0.0], [1.0, 2.0]]))
        poses = np.column_stack([rng.uniform(-2, 4, (1024, 2)), rng.uniform(-7, 7, 1024)])
        poses[:3, :2] = [[4.0 / 3, 2.0 / 3], [1.5, -1.0], [1.0, 1.0]]   # the centroid, beyond a corner, near a vertex
    elif case == "mixed":       # segment lengths from 1 mm to 50 m in one track: pruning bounds of every size
        t = _track(amd, _mixed_polyline(rng, 600), closed=False)
        lo, hi = t.xy.min(axis=0) - 5, t.xy.max(axis=0) + 5
        poses = np.column_stack([rng.uniform(lo, hi, (2048, 2)), rng.uniform(-7, 7, 2048)])
        k = rng.integers(0, t.num_points - 1, 512)
        w = rng.uniform(0, 1, (512, 1))
        poses[:512, :2] = (1 - w) * t.xy[k] + w * t.xy[k + 1] + rng.normal(0, 1e-3, (512, 2))
    elif case.startswith("shift"):   # far from the origin: the 1 um margin against float64 rounding of 1e5..1e6 m coordinates
        off = float(case[5:])
        t = _track(amd, raceline()[:, 1:3] + off)
        lo, hi = t.xy.min(axis=0) - 2, t.xy.max(axis=0) + 2
        poses = np.column_stack([rng.uniform(lo, hi, (2048, 2)), rng.uniform(-7, 7, 2048)])
        poses[:256, :2] = t.xy[rng.integers(0, t.num_points, 256)]
    elif case == "ngon37_centre":   # all 37 distances equal up to rounding: the last bits and the first-index rule decide
        t = _track(amd, _ngon(37))
        poses = np.column_stack([rng.normal(0.0, 1e-15, (512, 2)), rng.uniform(-7, 7, 512)])
        poses[:8, :2] = 0.0
    elif case == "shared_vertices":   # exactly on a vertex: two segments at distance 0, the first one wins
        t = _track(amd, _mixed_polyline(rng, 300, closed=True))
        poses = np.column_stack([t.xy, rng.uniform(-7, 7, t.num_points)])
    elif case == "nan_pose":
        t = _track(amd)
        poses = np.column_stack([rng.uniform(-50, 20, (64, 2)), rng.uniform(-7, 7, 64)])
        poses[0::3, 0] = np.nan
        poses[1::3, 1] = np.nan
    elif case == "vertices":
        t = _track(amd)
        poses = np.column_stack([t.xy, rng.uniform(-7, 7, t.num_points)])
    elif case == "equidistant":
        t = _track(amd, sq)
        poses = np.array([[1.0, 1.0, 0.0], [1.0, 0.5, 1.0], [0.5, 1.0, 2.0], [1.5, 1.0, 3.0], [1.0, 1.5, -3.0], [3.0, 3.0, 0.5],
                          [-1.0, -1.0, 0.0], [3.0, -1.0, 0.0], [-1.0, 3.0, 0.0], [1.0, -2.0, 1.0]])
    elif case == "far":
        t = _track(amd)
        poses = np.column_stack([rng.uniform(-500, 500, (512, 2)), rng.uniform(-7, 7, 512)])
    elif case == "raceline":
        t = _track(amd)
        lo, hi = t.xy.min(axis=0) - 2, t.xy.max(axis=0) + 2
        poses = np.column_stack([rng.uniform(lo, hi, (4096, 2)), rng.uniform(-7, 7, 4096)])
    elif case == "big5000":   # more segments than the LDS holds: streamed from global / L2
        t = _track(amd, _wiggly_loop(5000))
        poses = np.column_stack([rng.uniform(-12, 12, (2048, 2)), rng.uniform(-7, 7, 2048)])
        poses[:64, :2] = t.xy[rng.integers(0, 5000, 64)]
    elif case == "open":
        t = _track(amd, raceline()[:300, 1:3], closed=False)
        poses = np.column_stack([rng.uniform(-30, 30, (2048, 2)), rng.uniform(-7, 7, 2048)])
    else:
        t = _track(amd, sq)
        poses = np.column_stack([rng.uniform(-3, 5, (2048, 2)), rng.uniform(-7, 7, 2048)])
    s = amd.BatchSim(num_envs=1, num_agents=1)
    s.set_map_image(*load_map_image("example_map"))
    s.set_track(t)
    got = s.track_project_batch(poses)
    want = _oracle(t, poses)
    _check_cols(got, want, case)
    np.testing.assert_array_equal(got[:, 4], want[:, 4], err_msg="t")
    if case == "equidistant":
        assert got[0, 3] == 0 and got[1, 3] == 0 and got[2, 3] == 3   # ties: the first segment wins
    if case == "nan_pose":   # the reference: np.argmin over all-NaN distances -> 0, t[0] NaN (its clip passes NaN through)
        nan = np.isnan(poses[:, 0]) | np.isnan(poses[:, 1])
        assert np.all(got[nan, 3] == 0) and np.all(np.isnan(got[nan, 4])) and np.all(np.isnan(got[nan, 0]))
        assert np.all(np.isnan(want[nan, 4])) and np.all(np.isnan(want[nan, 0]))
        assert np.array_equal(got[nan, :2], t.project(poses[nan])[:, :2], equal_nan=True)
        poses, got = poses[~nan], got[~nan]
    msg = check_track_winner(t, poses, got[:, 3])   # an independent extended-precision check of the winner
    assert msg is None, case + ": " + msg
    s.close()


def test_track_set_refusals(amd):
    from f1tenth_gym_amd._ffi import F110LibraryError as F110Error
    s = amd.BatchSim(num_envs=2, num_agents=1)
    s.set_map_image(*load_map_image("example_map"))
    L = amd._ffi.lib()
    bad = [(np.array([[0.0, 0.0]]), 0), (np.array([[0.0, 0.0], [1.0, 0.0]]), 1), (np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 0.0]]), 1),
           (np.array([[0.0, 0.0], [np.nan, 1.0], [1.0, 1.0]]), 0), (np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 0.0]]), 0),
           (np.array([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [1.0, 1.0]]), 1)]
    for xy, closed in bad:
        xy = np.ascontiguousarray(xy)
        assert L.f110_track_set(s._h, 0, amd._ffi.dptr(xy), xy.shape[0], closed) == amd._ffi.ERR_INVALID, (xy, closed)
    sq = np.ascontiguousarray([[0.0, 0.0], [1.0, 0.0], [1.0, 1.0], [0.0, 0.0]])   # closed + repeat: 3 points
    assert L.f110_track_set(s._h, 0, amd._ffi.dptr(sq), 4, 1) == amd._ffi.OK
    assert L.f110_track_set(s._h, 1, amd._ffi.dptr(sq), 4, 1) == amd._ffi.ERR_INVALID   # no slot 1
    with pytest.raises(ValueError):
        s.set_track([[0.0, 0.0], [1.0, 0.0]])
    # enabling while an env sits on a slot without a track
    s2 = amd.BatchSim(num_envs=2, num_agents=1)
    s2.set_map_image(*load_map_image("example_map"))
    with pytest.raises(F110Error):
        s2.enable_track()
    s2.set_track(_track(amd))
    s2.add_map_image(*load_map_image("example_map"))
    s2.enable_track()
    s2.set_env_maps([0, 1])     # slot 1 has no track: the next step refuses
    s2.reset(bench_start_poses(2, 1))
    with pytest.raises(F110Error):
        s2.step(np.zeros((2, 2)))
    s.close(); s2.close()


# ------------------------------------------------------------------ step parity
def _check_step(s, track, pre=None, what=""):
    """the track columns of the last step vs the oracle on the returned poses; with pre (poses the step started from): ds too"""
    tr = s.get_track()
    post = _poses_of(s)
    want = _oracle(track, post)
    _check_cols(_cols(tr), want, what)
    if pre is not None:
        ds = track.wrap_ds(want[:, 0] - _oracle(track, pre)[:, 0])
        np.testing.assert_array_equal(tr["ds"], ds, err_msg=what + " ds")
    return tr


@pytest.mark.parametrize("path", ["step", "step_device", "step_host", "step_host_no_fuse", "step_host_no_sync", "step_host_spin"])
def test_step_parity_every_entry_point(amd, path):
    E, A, T = 256, 2, 60
    t = _track(amd)
    s = _sim(amd, E, A, t)
    s.reset(bench_start_poses(E, A, gap_wp=4))
    acts = _actions(T, E * A)
    d_act = s.device_array((E * A, 2))
    hb = s.host_block(("state", "agent_poses"))
    thb = s.track_host_block()
    tr = None
    for k in range(T):
        if path == "step":
            s.step(acts[k])
        elif path == "step_device":
            d_act.upload(acts[k])
            s.step_device(d_act)
        else:
            s.step_host(hb, acts[k], sync=path != "step_host_no_sync", fuse=path != "step_host_no_fuse", spin=path == "step_host_spin")
            if path == "step_host_no_sync":
                s.sync()
            for key in ("s", "ds", "lateral", "heading_error", "segment"):
                assert np.array_equal(thb[key], s.get_track()[key]), (k, key)
        if k % 10 == 9:
            tr = _check_step(s, t, what="%s step %d" % (path, k))
    # ds over the last step against the poses before it
    pre = _poses_of(s)
    s.step(acts[0])
    _check_step(s, t, pre, path + " ds")
    assert tr is not None
    s.close()


def test_env_blocks_are_bit_identical_to_one_block(amd):
    E, A, T = 2048, 2, 40
    t = _track(amd)
    out = []
    for groups in (1, 2):
        s = _sim(amd, E, A, t, step_groups=groups)
        s.reset(bench_start_poses(E, A, gap_wp=4))
        d_act = s.device_array((E * A, 2))
        acts = _actions(T, E * A, seed=3)
        for k in range(T):
            d_act.upload(acts[k])
            s.step_device(d_act)
        assert s.step_groups()[2] == groups
        out.append((s.get_track(), _poses_of(s)))
        _check_step(s, t, what="groups=%d" % groups)
        s.close()
    for key in out[0][0]:
        assert np.array_equal(out[0][0][key], out[1][0][key]), key
    assert np.array_equal(out[0][1], out[1][1])


@pytest.mark.parametrize("A", [1, 2])
def test_tiny_path_equals_the_three_kernel_path(amd, A):
    """F110Env (one env: the one-launch k_step_tiny step through f110_step_host) vs BatchSim.step (the per-kernel form)"""
    T = 300
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=A, track=CSV)
    s = _sim(amd, 1, A, _track(amd))
    poses = bench_start_poses(1, A, gap_wp=4)
    obs, _, _, _ = env.reset(poses)
    s.reset(poses)
    s.step(np.zeros((A, 2)))
    rng = np.random.default_rng(2)
    for k in range(T):
        a = np.stack([rng.uniform(-0.3, 0.3, A), rng.uniform(2.0, 7.0, A)], axis=1)
        obs, r, done, _ = env.step(a)
        assert env.sim.batch.step_launches() == 3, k     # head pass + k_step_tiny + track pass
        s.step(a)
        tr = s.get_track()
        assert np.array_equal(obs["poses_x"], _poses_of(s)[:, 0]), k
        for src, key in amd.Simulator.TRACK_KEYS:
            assert np.array_equal(np.asarray(obs[key]), tr[src]), (k, key)
        if done:
            break
    _check_step(env.sim.batch, env.track, what="tiny A=%d" % A)
    env.sim.batch.close(); s.close()


def test_two_maps_with_different_tracks(amd):
    E, A, T = 64, 2, 40
    t0 = _track(amd)
    t1 = _track(amd, raceline()[::-1, 1:3])     # the same line, driven the other way
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.set_noise_rng(SEED, STD)
    s.add_map_image(*load_map_image("example_map"))
    s.set_track(t0, 0)
    s.set_track(t1, 1)
    env_map = np.arange(E) % 2
    s.set_env_maps(env_map)
    s.enable_track()
    s.reset(bench_start_poses(E, A, gap_wp=4))
    acts = _actions(T, E * A)
    for k in range(T):
        s.step(acts[k])
    tr = s.get_track()
    post = _poses_of(s)
    slot = np.repeat(env_map, A)
    for sl, t in ((0, t0), (1, t1)):
        m = slot == sl
        _check_cols(_cols(tr)[m], _oracle(t, post[m]), "slot %d" % sl)
    s.close()


# ------------------------------------------------------------------ the pruning seed (the last winner) and the LDS staging
def _start_on(t, rng, n):
    """n poses on random vertices of a track, heading along the segment that starts there"""
    k = rng.integers(0, t.num_segments, n)
    pts = t.points_closed()
    d = pts[k + 1] - pts[k]
    return np.column_stack([pts[k], np.arctan2(d[:, 1], d[:, 0])])


def _step_via(s, path, act, hb, d_act):
    if path == "step":
        s.step(act)
    elif path == "step_device":
        d_act.upload(act)
        s.step_device(d_act)
    else:
        s.step_host(hb, act, fuse=path != "step_host_no_fuse")


def _check_step_winner(s, track, pre, what, rows=None):
    """_check_step, plus the extended-precision check of every winner"""
    rows = slice(None) if rows is None else rows
    tr = s.get_track()
    post = _poses_of(s)[rows]
    want = _oracle(track, post)
    _check_cols(_cols(tr)[rows], want, what)
    ds = track.wrap_ds(want[:, 0] - _oracle(track, pre[rows])[:, 0])
    np.testing.assert_array_equal(tr["ds"][rows], ds, err_msg=what + " ds")
    msg = check_track_winner(track, post, tr["segment"][rows])
    assert msg is None, what + ": " + msg


STEP_PATHS = ["step", "step_device", "step_host", "step_host_no_fuse"]


@pytest.mark.parametrize("nseg", [782, 1025, 5000])
@pytest.mark.parametrize("path", STEP_PATHS)
def test_adversarial_hints_after_set_state(amd, nseg, path):
    """the step forms seed the search with the agent's last winning segment.  set_state moves agents (a) to the point of the track
    farthest along it from that segment and (b) to near-tie points between two distant segments: the seed is then far from the
    winner, and the result must still be the full first-minimum search's, bit for bit"""
    E, A = 40, 2
    N = E * A
    t = _track(amd) if nseg == 782 else _track(amd, _wiggly_loop(nseg))
    assert t.num_segments == nseg
    rng = np.random.default_rng(nseg)
    s = _sim(amd, E, A, t)
    s.reset(_start_on(t, rng, N))
    d_act = s.device_array((N, 2))
    hb = s.host_block(("state", "agent_poses"))
    pts = t.points_closed()
    mid = 0.5 * (pts[:-1] + pts[1:])
    acts = _actions(24, N, seed=nseg, vmax=5.0)
    for k in range(24):
        pre = s.get("state")["state"][:, [0, 1, 4]]
        _step_via(s, path, acts[k], hb, d_act)
        _check_step_winner(s, t, pre, "%s nseg %d step %d" % (path, nseg, k))
        if k % 4 != 3:
            continue
        seg = s.get_track()["segment"].astype(np.int64)
        st = s.get("state")["state"].copy()
        far = (seg + nseg // 2) % nseg                           # (a) the opposite side of the track from the last winner
        st[0::2, 0:2] = mid[far[0::2]]
        other = (seg[1::2] + rng.integers(nseg // 4, 3 * nseg // 4 + 1, seg[1::2].size)) % nseg
        tie = 0.5 * (mid[seg[1::2]] + mid[other])                  # (b) halfway between the winner's midpoint and a distant one
        st[1::2, 0:2] = tie + rng.normal(0.0, 1e-12, tie.shape) * (rng.random((tie.shape[0], 1)) < 0.5)
        s.set_state(st)
    s.close()


@pytest.mark.parametrize("layout", ["small_big", "big_small", "same_count"])
@pytest.mark.parametrize("A", [1, 2])
def test_mixed_slot_workgroups(amd, A, layout):
    """two slots, one track of <= kTrackLdsSegs segments (staged in LDS) and one of more (read from global memory); env_map
    alternates in runs of 5 envs, so slot changes fall inside the 16-agent workgroups — some workgroups' first agent sits on
    the staged slot, some on the other.  same_count: two different tracks of 1000 segments each (both fit the LDS; only the
    workgroup's first agent's slot is staged, and a table of the right size but the wrong slot must not be read)"""
    E = 80
    N = E * A
    small, big = _track(amd, _wiggly_loop(600)), _track(amd, 1.2 * _wiggly_loop(2048))
    tracks = {"small_big": (small, big), "big_small": (big, small),
              "same_count": (_track(amd, _wiggly_loop(1000)), _track(amd, 1.2 * _wiggly_loop(1000)))}[layout]
    s = amd.BatchSim(num_envs=E, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.set_noise_rng(SEED, STD)
    s.add_map_image(*load_map_image("example_map"))
    s.set_track(tracks[0], 0)
    s.set_track(tracks[1], 1)
    env_map = (np.arange(E) // 5) % 2
    s.set_env_maps(env_map)
    s.enable_track()
    slot = np.repeat(env_map, A)
    rng = np.random.default_rng(A)
    poses = np.empty((N, 3))
    for sl in (0, 1):
        poses[slot == sl] = _start_on(tracks[sl], rng, int((slot == sl).sum()))
    s.reset(poses)
    d_act = s.device_array((N, 2))
    hb = s.host_block(("state", "agent_poses"))
    acts = _actions(30, N, seed=20 + A, vmax=6.0)
    for k in range(30):
        path = STEP_PATHS[k % len(STEP_PATHS)]
        pre = s.get("state")["state"][:, [0, 1, 4]]
        _step_via(s, path, acts[k], hb, d_act)
        for sl in (0, 1):
            _check_step_winner(s, tracks[sl], pre, "A=%d %s %s step %d slot %d" % (A, layout, path, k, sl), slot == sl)
        if k == 14:   # swap the slots' tracks mid-run: every cached s and every seed goes stale at once
            tracks = tracks[::-1]
            s.set_track(tracks[0], 0)
            s.set_track(tracks[1], 1)
    s.close()


@pytest.mark.parametrize("how", ["clone_envs", "load_envs"])
def test_a_load_onto_another_slot_at_the_same_pose_re_projects(amd, how):
    """two envs at bitwise the same pose on two slots with different tracks; env 0 copied onto env 1 moves env 1 to slot 0 without
    changing its pose bits, so only the cache invalidation of the load tells the next step that env 1's cached s is stale"""
    A = 2
    t0, t1 = _track(amd), _track(amd, _wiggly_loop(1500))
    s = amd.BatchSim(num_envs=2, num_agents=A)
    s.set_map_image(*load_map_image("example_map"))
    s.add_map_image(*load_map_image("example_map"))
    s.set_track(t0, 0)
    s.set_track(t1, 1)
    s.set_env_maps([0, 1])
    s.enable_track()
    p = bench_start_poses(1, A, gap_wp=4)
    s.reset(np.vstack([p, p]))
    act = np.tile([[0.1, 3.0]], (2 * A, 1))
    s.step(act)
    post = _poses_of(s)
    assert np.array_equal(post[:A], post[A:])
    if how == "clone_envs":
        s.clone_envs([0], [1])
    else:
        s.load_envs(s.save_envs([0]), [0], [1])
    pre = s.get("state")["state"][:, [0, 1, 4]]
    s.step(act)
    _check_step_winner(s, t0, pre, how + " (both envs on slot 0 now)")
    s.close()


# ------------------------------------------------------------------ the invariant: ds = s(post) - s(pre) after every pose writer
def test_progress_after_every_pose_writer(amd):
    E, A = 32, 2
    N = E * A
    t = _track(amd)
    s = _sim(amd, E, A, t)
    s.episode_init(0)
    start = bench_start_poses(E, A, gap_wp=4)
    s.episode_reset(start)
    d_start = s.device_array((N, 3)); d_start.upload(start)
    d_cnt = s.device_array((1,), np.int32); d_cnt.upload(np.zeros(1, np.int32))
    acts = _actions(400, N, seed=11, vmax=12.0)
    it = iter(acts)
    hb = s.host_block(("state", "agent_poses", "done"))

    def step_checked(what, via_host=False):
        pre = s.get("state")["state"][:, [0, 1, 4]]
        if via_host:
            s.step_host(hb, next(it))
        else:
            s.step(next(it))
        _check_step(s, t, pre, what)

    for _ in range(5):
        step_checked("warm-up")
    rng = np.random.default_rng(4)
    # full and partial reset
    s.reset(start); step_checked("full reset")
    moved = start + np.concatenate([rng.uniform(-0.2, 0.2, (N, 2)), np.zeros((N, 1))], axis=1)
    mask = (np.arange(E) % 3 == 0).astype(np.uint8)
    s.reset(moved, mask); step_checked("partial reset")
    # auto re-seat inside f110_step_host (fast, blind driving until some env ends)
    seen = False
    for _ in range(300):
        pre = s.get("state")["state"][:, [0, 1, 4]]
        s.step_host(hb, _actions(1, N, seed=int(rng.integers(1 << 30)), vmax=14.0)[0], auto_reset=True)
        _check_step(s, t, pre, "auto-reset step")   # the columns are the step's, before the re-seat
        if hb.views["done"].any():
            seen = True
            step_checked("after auto re-seat")
            break
    assert seen, "no env finished: the auto re-seat was not exercised"
    # in-step re-seat (f110_set_auto_reseat) and f110_reset_collided_device
    s.set_auto_reseat(d_start, 0, d_cnt)
    for _ in range(60):
        step_checked("armed auto re-seat")
    s.set_auto_reseat(None, 0, None)
    s.reset_collided_device(d_start, 0, d_cnt); step_checked("reset_collided_device")
    s.episode_reset_done_device(d_cnt); step_checked("episode_reset_done_device")
    # set_state
    st = s.get("state")["state"].copy()
    st[:, 0] += 0.05
    s.set_state(st); step_checked("set_state")
    # state_load (whole handle) and clone_envs
    blob = s.save_state()
    for _ in range(3):
        step_checked("before load")
    s.load_state(blob); step_checked("state_load")
    s.clone_envs(np.arange(0, 8), np.arange(8, 16)); step_checked("clone_envs")
    # set_env_maps and set_track
    s.add_map_image(*load_map_image("example_map"))
    s.set_track(t, 1)
    s.set_env_maps(np.arange(E) % 2); step_checked("set_env_maps")
    s.set_track(t, 0); step_checked("set_track")
    s.close()


# ------------------------------------------------------------------ end to end: two laps of the example map
def test_two_laps_with_the_pure_pursuit_planner_sum_to_twice_the_track(amd):
    w = raceline()
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=1, track=CSV, reward='progress')
    assert round(env.track.length, 5) == L_EXAMPLE and env.track.num_segments == 782
    wp = np.ascontiguousarray(w[:, [1, 2, 5]])
    lookahead, vgain, wheelbase = 0.82461887897713965, 0.90338203837889, 0.17145 + 0.15875
    obs, total, done, _ = env.reset(np.array([[w[0, 1], w[0, 2], w[0, 3] + np.pi / 2]]))
    steps = 0
    while not done and steps < 20000:
        pose = np.array([[obs['poses_x'][0], obs['poses_y'][0], obs['poses_theta'][0]]])
        act = env.sim.batch.pure_pursuit_batch(wp, pose, lookahead, vgain, wheelbase)
        obs, r, done, _ = env.step(act)
        total += r
        steps += 1
    assert done and obs['lap_counts'][0] == 2 and obs['collisions'][0] == 0, (steps, obs['lap_counts'], obs['collisions'])
    assert abs(total - 2 * L_EXAMPLE) <= 0.01 * 2 * L_EXAMPLE, total
    env.sim.batch.close()


# ------------------------------------------------------------------ env layers
def test_vec_env_device_logic_views_equal_get_track(amd):
    E, A = 64, 2
    env = amd.F110VecEnv(E, device_logic=True, auto_reset=True, map=map_stem("example_map"), map_ext=".png", num_agents=A,
                         track=CSV, reward='progress')
    assert set(amd.F110VecEnv._TRACK) <= set(env.obs_fields)
    obs, r, done, _ = env.reset(bench_start_poses(E, A, gap_wp=4).reshape(E, A, 3))
    acts = _actions(100, E * A).reshape(100, E, A, 2)
    for k in range(100):
        if k % 2:
            env.step_async(acts[k]); obs, r, done, _ = env.step_wait()
        else:
            obs, r, done, _ = env.step(acts[k])
        tr = env.sim.batch.get_track()
        for src, key in amd.Simulator.TRACK_KEYS:
            assert np.array_equal(obs[key], tr[src].reshape(E, A)), (k, key)
        assert r.shape == (E,) and np.array_equal(r, tr["ds"].reshape(E, A)[:, 0])
    env.sim.batch.close()


def test_snapshot_restore_carries_the_track_keys(amd):
    env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2, track=CSV, reward='progress')
    env.reset(bench_start_poses(1, 2, gap_wp=4))
    acts = _actions(40, 2)
    for k in range(20):
        env.step(acts[k])
    snap = env.snapshot()
    last = env._last
    after = [env.step(acts[k]) for k in range(20, 40)]
    back = env.restore(snap)
    for key in ("progress", "progress_delta", "lateral_offset", "heading_error", "track_segment"):
        assert np.array_equal(np.asarray(back[0][key]), np.asarray(last[0][key])), key
    assert back[1] == last[1]
    again = [env.step(acts[k]) for k in range(20, 40)]
    for (o1, r1, _, _), (o2, r2, _, _) in zip(after, again):
        assert r1 == r2
        for key in ("progress", "progress_delta", "lateral_offset", "heading_error", "track_segment"):
            assert np.array_equal(np.asarray(o1[key]), np.asarray(o2[key])), key
    env.sim.batch.close()
    vec = amd.F110VecEnv(8, device_logic=True, map=map_stem("example_map"), map_ext=".png", num_agents=2, track=CSV, copy_obs=True)
    vec.reset(bench_start_poses(8, 2, gap_wp=4).reshape(8, 2, 3))
    vec.step(np.zeros((8, 2, 2)))
    snap = vec.snapshot()
    saved = {k: np.array(v) for k, v in vec._last[0].items() if isinstance(v, np.ndarray)}
    vec.step(np.ones((8, 2, 2)))
    back = vec.restore(snap)
    for key in amd.F110VecEnv._TRACK:
        assert np.array_equal(back[0][key], saved[key]), key
    vec.sim.batch.close()


@pytest.mark.parametrize("device_logic", [True, False])
def test_sharded_vec_env_equals_one_handle(amd, device_logic):
    E, A, T = 48, 2, 30
    kw = dict(map=map_stem("example_map"), map_ext=".png", num_agents=A, track=CSV, reward='progress', device_logic=device_logic,
              auto_reset=True)
    one = amd.F110VecEnv(E, copy_obs=True, **kw)
    sh = amd.ShardedVecEnv(E, devices=(0, 0), **kw)
    poses = bench_start_poses(E, A, gap_wp=4).reshape(E, A, 3)
    acts = _actions(T, E * A).reshape(T, E, A, 2)
    a, b = one.reset(poses), sh.reset(poses)
    for k in range(T):
        a, b = one.step(acts[k]), sh.step(acts[k])
        for key in amd.F110VecEnv._TRACK:
            assert np.array_equal(a[0][key], b[0][key]), (k, key)
        assert np.array_equal(a[1], b[1]), k
    sh.close(); one.sim.batch.close()


def test_track_views_through_dlpack_in_a_child_process(amd):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = r'''
import os, sys
try:
    import torch
except Exception as ex:
    print("SKIP torch is not importable: %s" % ex); sys.exit(0)
if not torch.cuda.is_available():
    print("SKIP this torch build sees no GPU"); sys.exit(0)
import numpy as np
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import f1tenth_gym_amd as amd
from _util import bench_start_poses, load_map_image, MAPS
s = amd.BatchSim(num_envs=16, num_agents=2)
s.set_map_image(*load_map_image("example_map"))
s.set_track(os.path.join(MAPS, "example_waypoints.csv"))
s.enable_track()
s.reset(bench_start_poses(16, 2))
for _ in range(5):
    s.step(np.tile([[0.0, 3.0]], (32, 1)))
v = s.track_views()
st = torch.from_dlpack(v["s"])
sg = torch.from_dlpack(v["segment"])
assert st.data_ptr() == v["s"].ptr and st.dtype == torch.float64 and sg.dtype == torch.int32 and tuple(st.shape) == (32,)
tr = s.get_track()
assert np.array_equal(st.cpu().numpy(), tr["s"]) and np.array_equal(sg.cpu().numpy(), tr["segment"])
del st, sg          # (as tests/dlpack_torch_worker.py: the tensors go, the stream drains, the handle closes before teardown)
torch.cuda.synchronize()
s.close()
print("DLPACK OK")
'''
    code = "ROOT = %r\n" % root + code
    out = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600, cwd=root)
    if "SKIP" in out.stdout:
        pytest.skip(out.stdout.strip().splitlines()[-1])
    assert out.returncode == 0 and "DLPACK OK" in out.stdout, (out.stdout[-800:], out.stderr[-1500:])


def test_gym_make_alias_takes_the_track(amd):
    import f110_gym
    env = f110_gym.make('f110-v0', map=map_stem("example_map"), map_ext=".png", num_agents=1, track=CSV, reward='progress')
    obs, r, _, _ = env.reset(bench_start_poses(1, 1))
    assert "progress" in obs and r == obs["progress_delta"][0]
    env.sim.batch.close()


# ------------------------------------------------------------------ no behaviour change without tracking
def test_no_track_and_track_not_enabled_are_todays_step(amd):
    T = 200
    runs = []
    for mode in ("none", "set", "set_then_disabled"):
        env = amd.F110Env(map=map_stem("example_map"), map_ext=".png", num_agents=2)
        if mode != "none":
            env.sim.set_track(CSV)
        if mode == "set_then_disabled":
            env.sim.enable_track(True)
            env.sim.enable_track(False)
        rng = np.random.default_rng(8)
        rec = [env.reset(bench_start_poses(1, 2, gap_wp=3))[0]]
        launches = []
        for _ in range(T):
            o = env.step(np.stack([rng.uniform(-0.4, 0.4, 2), rng.uniform(2.0, 9.0, 2)], axis=1))[0]
            assert "progress" not in o
            rec.append(o)
            launches.append(env.sim.batch.step_launches())
        runs.append((rec, launches))
        env.sim.batch.close()
    for rec, launches in runs[1:]:
        assert launches == runs[0][1]
        for a, b in zip(runs[0][0], rec):
            for key in a:
                assert np.array_equal(np.asarray(a[key]), np.asarray(b[key])), key
    assert set(runs[0][1]) == {1}
    # a batch on the per-kernel path
    E, A = 512, 2
    outs = []
    for mode in ("none", "set"):
        s = _sim(amd, E, A, _track(amd) if mode == "set" else None, enable=False)
        s.reset(bench_start_poses(E, A, gap_wp=4))
        for a in _actions(50, E * A):
            s.step(a)
        outs.append(s.get("scans", "state", "collisions", "collision_idx", "in_collision", "step_count"))
        s.close()
    for key in outs[0]:
        assert np.array_equal(outs[0][key], outs[1][key]), key
