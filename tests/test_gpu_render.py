"""Rendering on the device (include/f110.h f110_render_device, BatchSim.render_device / render, F110Env.render('rgb_array'),
F110VecEnv.render / render_device, ShardedVecEnv.render) against tests/render_ref.py: every pixel whose decision is further than
1e-9 m from flipping is equal, on every view, layer and map arrangement; a render changes no simulator state."""
import ctypes as C

import numpy as np
import pytest

import render_ref as R
from f1tenth_gym_amd import workload

pytestmark = pytest.mark.gpu

SEED, STD = 12345, 0.01
VIEWS = [dict(view="world", width=96, height=80, m_per_px=0.25, center=(-20.0, 2.0), angle=0.3),
         dict(view="follow", width=64, height=48, m_per_px=0.05, fwd_offset=1.5),
         dict(view="ego", width=64, height=64, m_per_px=0.05)]


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _img(name="example_map"):
    return workload.load_map_image(name)


def _dt_of(amd, img, res, origin):
    s = amd.BatchSim(num_envs=1, num_agents=1, num_beams=8)
    s.set_map_image(img, res, origin)
    dt = s.get_map_dt()
    s.close()
    return dt


def _sim(amd, E, A, img=None, res=None, origin=None, track=True, **kw):
    s = amd.BatchSim(num_envs=E, num_agents=A, **kw)
    i0, r0, o0 = _img()
    img, res, origin = (i0 if img is None else img), (r0 if res is None else res), (o0 if origin is None else origin)
    s.set_map_image(img, res, origin)
    s.set_noise_rng(SEED, STD)
    maps = [{"dt": s.get_map_dt(), "res": res, "origin": origin, "track": workload.raceline()[:, 1:3] if track else None}]
    if track:
        s.set_track(workload.raceline()[:, 1:3])
    return s, maps


def _run(sim, E, A, T=50, seed=3, vmax=8.0, gap=6):
    sim.reset(workload.bench_start_poses(E, A, gap_wp=gap))
    rng = np.random.default_rng(seed)
    for _ in range(T):
        sim.step(np.stack([rng.uniform(-0.4, 0.4, E * A), rng.uniform(2.0, vmax, E * A)], axis=1))


def _scene(sim, maps, env_slot=None, lengths=None, widths=None):
    o = sim.get("agent_poses", "scans")
    L = sim.params["length"] if lengths is None else lengths
    W = sim.params["width"] if widths is None else widths
    return R.Scene(o["agent_poses"], o["scans"], sim.A, maps, L, W, env_slot=env_slot, max_range=30.0)


def _check(sim, sc, agents, what, **spec):
    got = sim.render(agents, **spec)
    want, margin = R.render(sc, agents, **spec)
    R.compare(got, want, margin, what=what)
    return got


@pytest.mark.parametrize("A", [2, 3])
def test_parity_every_view_every_layer(amd, A):
    E = 4
    sim, maps = _sim(amd, E, A)
    _run(sim, E, A, gap=2)                     # 0.4 m apart: the cars start in contact
    assert sim.get("collisions")["collisions"].any(), "the run should contain collisions"
    sc = _scene(sim, maps)
    agents = np.arange(E * A)
    for spec in VIEWS:
        got = _check(sim, sc, agents, "A=%d %s" % (A, spec["view"]), layers="all", **spec)
        assert {1, 2, 6}.issubset(set(np.unique(got).tolist()))
    # the scan and the track show up where they should
    got = _check(sim, sc, agents, "wide world", layers="all", view="world", width=400, height=300, m_per_px=0.2, center=(-30.0, 0.0))
    assert (got == 3).any() and (got == 4).any()
    sim.close()


def test_yawed_origin_and_odd_resolution(amd):
    img, _, _ = _img()
    res, origin = 0.0537, [-55.3, -10.1, 0.37]
    sim, maps = _sim(amd, 2, 2, img, res, origin, track=False)
    sim.reset(np.array([[-20.03, 5.01, 0.4], [-18.02, 6.07, 1.0], [-30.05, 0.03, 2.0], [-29.01, 0.52, -1.0]]))
    for _ in range(5):
        sim.step(np.tile([0.05, 1.0], (4, 1)))
    sc = _scene(sim, maps)
    for spec in VIEWS:
        _check(sim, sc, np.arange(4), "yawed " + spec["view"], layers="all", **spec)
    sim.close()


def test_two_slots_with_their_own_tracks(amd):
    E, A = 4, 2
    sim, maps = _sim(amd, E, A)
    bimg, bres, borig = _img("berlin")
    slot = sim.add_map_image(bimg, bres, borig)
    btrack = np.array([[0.0, 0.0], [10.0, 0.0], [10.0, 5.0], [0.0, 5.0]])
    sim.set_track(btrack, slot)
    maps.append({"dt": _dt_of(amd, bimg, bres, borig), "res": bres, "origin": borig, "track": btrack})
    env_slot = np.array([0, 1, 0, 1], dtype=np.int32)
    sim.set_env_maps(env_slot)
    poses = workload.bench_start_poses(E, A, gap_wp=6).reshape(E, A, 3)
    poses[1] = [[1.03, 0.51, 0.1], [3.02, 0.23, 0.0]]
    poses[3] = [[9.01, 4.04, 1.5], [5.03, 5.06, 3.0]]
    sim.reset(poses.reshape(-1, 3))
    for _ in range(5):
        sim.step(np.tile([0.05, 1.0], (E * A, 1)))
    sc = _scene(sim, maps, env_slot=env_slot)
    for spec in VIEWS[1:]:
        got = _check(sim, sc, np.arange(E * A), "two slots " + spec["view"], layers="all", **spec)
        assert (got[2:4] == 3).any() or (got[6:8] == 3).any()
    sim.close()


def test_per_agent_params_and_car_size(amd):
    E, A = 3, 2
    sim, maps = _sim(amd, E, A)
    rng = np.random.default_rng(5)
    pv = np.tile(np.array([sim.params[k] for k in amd._ffi.PARAM_KEYS]), (E * A, 1))
    pv[:, 17] = rng.uniform(0.3, 1.2, E * A)   # length
    pv[:, 16] = rng.uniform(0.2, 0.6, E * A)   # width
    sim.set_params_batch(pv)
    sim.reset(workload.bench_start_poses(E, A, gap_wp=3))
    for _ in range(5):
        sim.step(np.tile([0.05, 1.0], (E * A, 1)))
    sc = _scene(sim, maps, lengths=pv[:, 17], widths=pv[:, 16])
    spec = dict(view="ego", width=80, height=80, m_per_px=0.02, layers=("map", "cars"))
    a = _check(sim, sc, np.arange(E * A), "per-agent params", **spec)
    b = _check(sim, sc, np.arange(E * A), "car_size", car_size=(1.47, 0.93), **spec)
    assert (b == 6).sum() > (a == 6).sum()
    sim.close()


def test_nan_poses(amd):
    E, A = 2, 2
    sim, maps = _sim(amd, E, A)
    _run(sim, E, A, T=3)
    ap = sim.device_views()["agent_poses"]
    host = ap.download()
    host[0, 1] = np.nan       # agent 1: x
    ap.upload(host)
    sc = _scene(sim, maps)
    assert np.isnan(sc.poses[1, 0])
    ego = sim.render([1], view="ego", layers="all")
    assert ego.shape == (1, 64, 64) and not ego.any()           # all OUTSIDE
    world = _check(sim, sc, [0, 1], "nan world", view="world", width=128, height=128, m_per_px=0.05,
                   center=tuple(host[:2, 0]), layers="all")
    assert not (world[1] == 6).any() and not (world[0] == 5).any()   # the NaN car is drawn nowhere
    sim.close()


def test_layers_and_palettes(amd):
    E, A = 2, 2
    sim, maps = _sim(amd, E, A)
    _run(sim, E, A, T=20)
    sc = _scene(sim, maps)
    agents = np.arange(E * A)
    spec = dict(view="follow", width=200, height=160, m_per_px=0.1, fwd_offset=2.0)
    full = sim.render(agents, layers="all", **spec)
    for name, classes in (("map", (0, 2)), ("track", (3,)), ("scan", (4,)), ("cars", (5, 6))):
        layers = tuple(k for k in R.LAYER if k != name)
        got = _check(sim, sc, agents, "without " + name, layers=layers, **spec)
        assert not np.isin(got, classes).any()
        assert np.isin(full, classes).any(), name
    custom = np.arange(21, dtype=np.uint8).reshape(7, 3) * 11
    for pal in (None, custom):
        cls, rgb = sim.render(agents, layers="all", rgb=True, palette=pal, **spec)
        assert rgb.shape == cls.shape + (3,) and rgb.dtype == np.uint8
        np.testing.assert_array_equal(rgb, amd.render.colorize(cls, pal))
        np.testing.assert_array_equal(cls, full)
    # widths that are not a multiple of 4 (the staged form) give the same pixels
    odd = sim.render(agents, layers="all", **dict(spec, width=199))
    np.testing.assert_array_equal(odd, sim.render(agents, layers="all", **dict(spec, width=199)))
    R.compare(odd, R.render(sc, agents, layers="all", **dict(spec, width=199))[0],
              R.render(sc, agents, layers="all", **dict(spec, width=199))[1], what="width 199")
    sim.close()


def _state(sim, track):
    o = sim.get("scans", "state", "agent_poses", "collisions", "collision_idx", "in_collision", "step_count")
    if track:
        o.update({"trk_" + k: v for k, v in sim.get_track().items()})
    return o


@pytest.mark.parametrize("path", ["device", "host", "two_blocks"])
def test_render_is_read_only(amd, path):
    E, A = (4096, 2) if path == "two_blocks" else (4, 2)
    kw = {"step_groups": 2} if path == "two_blocks" else {}
    T = 100 if path != "two_blocks" else 40
    runs = []
    for render in (False, True):
        sim, _ = _sim(amd, E, A, **kw)
        sim.enable_track()
        sim.reset(workload.bench_start_poses(E, A, gap_wp=6))
        rng = np.random.default_rng(11)
        hb = sim.host_block(("state", "scans")) if path == "host" else None
        d_act = sim.device_array((E * A, 2)) if path != "host" else None
        for _ in range(T):
            act = np.stack([rng.uniform(-0.4, 0.4, E * A), rng.uniform(2.0, 8.0, E * A)], axis=1)
            if path == "host":
                sim.step_host(hb, act)
            else:
                d_act.upload(act)
                sim.step_device(d_act)
            if render:
                sim.render_device([0, E * A - 1], view="ego", layers="all", rgb=True)
        runs.append(_state(sim, True))
        if path == "two_blocks":
            assert sim.step_groups()[2] == 2
        sim.close()
    for k in runs[0]:
        np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)


def test_render_behind_an_unsynchronised_two_block_step(amd):
    E, A = 4096, 2
    sim, _ = _sim(amd, E, A, step_groups=2)
    sim.reset(workload.bench_start_poses(E, A, gap_wp=6))
    d_act = sim.device_array((E * A, 2))
    d_act.upload(np.tile([0.1, 6.0], (E * A, 1)))
    agents = np.arange(0, E * A, 97)
    for _ in range(3):
        sim.step_device(d_act)
    early = sim.render_device(agents, view="ego", layers="all")   # enqueued right behind the step, no sync
    got = early.download()
    sim.sync()
    np.testing.assert_array_equal(got, sim.render(agents, view="ego", layers="all"))
    sc = _scene(sim, [{"dt": sim.get_map_dt(), "res": _img()[1], "origin": _img()[2], "track": workload.raceline()[:, 1:3]}])
    R.compare(got, *R.render(sc, agents, view="ego", layers="all"), what="two blocks")
    sim.close()


def test_map_changes_invalidate_the_grid(amd):
    sim, maps = _sim(amd, 1, 2, track=False)
    sim.reset(np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]))
    spec = dict(view="world", width=120, height=120, m_per_px=0.5, center=(0.0, 0.0), layers=("map",))
    first = sim.render([0], **spec)
    bimg, bres, borig = _img("berlin")
    sim.set_map_image(bimg, bres, borig)
    sc = _scene(sim, [{"dt": sim.get_map_dt(), "res": bres, "origin": borig}])
    second = _check(sim, sc, [0], "after set_map", **spec)
    assert not np.array_equal(first, second)
    dt = np.full((50, 60), 1.0)
    dt[10:20, 5:40] = 0.0
    sim.set_map_dt(dt, 0.3, [-5.0, -5.0, 0.2])
    sc = _scene(sim, [{"dt": dt, "res": 0.3, "origin": [-5.0, -5.0, 0.2]}])
    third = _check(sim, sc, [0], "after set_map_dt", **spec)
    assert (third == 2).sum() > 0 and not np.array_equal(second, third)
    sim.close()


def test_refusals_write_nothing(amd):
    from f1tenth_gym_amd import _ffi, render
    sim, _ = _sim(amd, 2, 2)
    sim.reset(workload.bench_start_poses(2, 2))
    buf = sim.device_array((4, 16, 16), np.uint8)
    sentinel = np.full((4, 16, 16), 0xAB, dtype=np.uint8)
    buf.upload(sentinel)
    L = _ffi.lib()
    ok = render.make_spec(width=16, height=16)

    def call(spec, agents, n):
        a = None if agents is None else np.ascontiguousarray(agents, dtype=np.int32)
        return L.f110_render_device(sim._h, C.byref(spec), None if a is None else a.ctypes.data_as(_ffi._i32p), n, buf.ptr, None, None)

    def spec_with(**kw):
        s = render.RenderSpec.from_buffer_copy(ok)
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    cases = [(spec_with(width=0), None, 4), (spec_with(height=4097), None, 4), (spec_with(m_per_px=0.0), None, 4),
             (spec_with(m_per_px=float("nan")), None, 4), (spec_with(m_per_px=float("inf")), None, 4), (spec_with(view=3), None, 4),
             (spec_with(layers=16), None, 4), (ok, [0, 4], 2), (ok, [-1], 1), (ok, [0], 0), (ok, None, 3),
             (spec_with(width=4096, height=4096), np.zeros(129), 129)]
    for spec, agents, n in cases:
        assert call(spec, agents, n) == _ffi.ERR_INVALID
        assert _ffi.last_error(sim._h)
    sim.sync()
    np.testing.assert_array_equal(buf.download(), sentinel)
    assert call(ok, None, 4) == _ffi.OK
    assert not np.array_equal(buf.download(), sentinel)
    for bad in (dict(width=0), dict(view="top"), dict(layers=("x",)), dict(m_per_px=-1.0)):
        with pytest.raises(ValueError):
            sim.render_device(**bad)
    with pytest.raises(ValueError):
        sim.render_device([4])
    sim.close()


def test_env_layers(amd):
    from f1tenth_gym_amd import _dlpack
    env = amd.F110Env(map=workload.map_stem("example_map"), map_ext=".png", num_agents=2, track=workload.raceline()[:, 1:3])
    env.reset(workload.bench_start_poses(1, 2, gap_wp=6))
    for _ in range(5):
        env.step(np.array([[0.0, 4.0], [0.05, 4.0]]))
    frame = env.render('rgb_array')
    assert frame.shape == (800, 1000, 3) and frame.dtype == np.uint8
    _, want = env.sim.batch.render([env.ego_idx], width=1000, height=800, view="world", m_per_px=0.024, center=(0.0, 0.0),
                                   layers="all", rgb=True)
    np.testing.assert_array_equal(frame, want[0])
    with pytest.raises(NotImplementedError):
        env.render('human')
    env.set_render_view(view="follow", width=128, height=96)
    assert env.render('rgb_array').shape == (96, 128, 3)
    env.sim.batch.close()

    kw = dict(map=workload.map_stem("example_map"), map_ext=".png", num_agents=2)
    vec = amd.F110VecEnv(4, **kw)
    poses = workload.bench_start_poses(4, 2, gap_wp=6).reshape(4, 2, 3)
    vec.reset(poses)
    vec.step(np.tile([0.0, 3.0], (4, 2, 1)))
    frames = vec.render([2, 0], width=64, height=48, view="ego", m_per_px=0.05)
    assert frames.shape == (2, 48, 64, 3) and frames.dtype == np.uint8
    np.testing.assert_array_equal(frames, vec.sim.batch.render([4, 0], width=64, height=48, view="ego",
                                                                layers=("map", "scan", "cars"), rgb=True)[1])
    crops = vec.render_device(None, width=32, height=32)
    info = _dlpack.read_capsule(crops.__dlpack__())
    assert info["shape"] == (8, 32, 32) and info["dtype"] == (_dlpack.kDLUInt, 8, 1)
    del info
    crops.free()
    sh = amd.ShardedVecEnv(4, devices=[0, 0], **kw)
    sh.reset(poses)
    sh.step(np.tile([0.0, 3.0], (4, 2, 1)))
    np.testing.assert_array_equal(sh.render([3, 0, 2], width=64, height=48, view="follow"),
                                  vec.render([3, 0, 2], width=64, height=48, view="follow"))
    sh.close()
    vec.sim.batch.close()


def test_full_batch_crops(amd):
    E, A = 32768, 2
    sim, maps = _sim(amd, E, A)
    sim.reset(workload.bench_start_poses(E, A))
    for acts in workload.action_sets(3, E * A, 0):
        sim.step(acts)
    cls = sim.render_device(None, view="ego", width=64, height=64, layers="all")
    sample = np.sort(np.random.default_rng(2).choice(E * A, 256, replace=False))
    got = np.stack([cls.download_part(int(n), 1)[0] for n in sample])
    cls.free()
    sc = _scene(sim, maps)
    R.compare(got, *R.render(sc, sample, view="ego", width=64, height=64, layers="all"), what="65536 crops")
    sim.close()
