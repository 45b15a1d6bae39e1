"""The obstacle stamp (f110_add_map_obstacles / f110_set_map_obstacles) at its kernels' edges and under the readers no
other test puts on a derived slot.  The fixtures are tests/obstacles_ref.py's; tests/test_obstacles_host.py holds their conditions
on the CPU (three chunks of k_obst_rows, Wa = 2048 and 2049, a multi-stride corner reduction, Wa = 0, 256 obstacles, the all-stamped
table, the border's residues).

(1) every table and list: the derived slot's table against the NumPy model and against a slot made from the blacked-out image, bit for
    bit; the WHOLE padded copy (border included, read from the device) against that slot's; every border cell equal to cell
    [H-1][W-1]; base and unrelated slots untouched; the same after re-stamps in place, alternating between shapes on one handle too.
(2) the rollout on a derived slot: the unit form against tests/rollout_ref.py on the model's table, the device form against an
    image-made twin and against the unit form, before and after a re-stamp that changes the out-of-bounds value.  The MPPI planner
    on the same slot against tests/mppi_ref.py, the twin and its own device form.
(3) a re-stamp enqueued behind a rollout (and behind the scripted cars' controllers) that rides the two env blocks.
(4) the render of two derived slots in one call, and clone_envs from an env on a derived slot."""
import numpy as np
import pytest

import obstacles_ref as ref
import rollout_ref as rref
from _util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


_model_cache = {}


def _model(fx, which):
    """(model table, stamp mask, base table) of list `which` of a fixture — computed once, shared, never written to"""
    name, img, res, origin, lists = fx
    key = (name, which)
    if key not in _model_cache:
        base = ref.table_from_bitmap(ref.free_from_image(img), res)
        t, m = ref.derived_table(base, lists[which][1], res, origin)
        for a in (t, m, base):
            a.setflags(write=False)
        _model_cache[key] = (t, m, base)
    return _model_cache[key]


def _twin_image(fx, which):
    return ref.image_with_stamps(fx[1], _model(fx, which)[1])


def _padded(s, slot, H, W, max_range=30.0):
    """the slot's whole padded copy [H + 2b][Wp] read from the device, and b"""
    from f1tenth_gym_amd import _ffi
    addr, row_bytes = s.map_table_address(slot)
    res = s._slot_res[slot]
    assert row_bytes % 8 == 0
    Wp = row_bytes // 8
    assert (Wp - W) % 2 == 0
    b = (Wp - W) // 2
    assert b == ref.pad_border(max_range, res), "slot %d: a border of %d cells, the formula gives %d" % (slot, b, ref.pad_border(max_range, res))
    out = np.empty((H + 2 * b, Wp))
    _ffi.check(_ffi.lib().f110_memcpy_d2h(s._h, out.ctypes.data, addr - (b * Wp + b) * 8, out.nbytes), s._h)
    return out, b


def _add_image(s, img, res, origin):
    slot = s.add_map_image(img, res, origin)
    s._slot_res[slot] = res
    return slot


def _add_derived(s, ob, base):
    slot = s.add_obstacle_map(ob, base=base)
    s._slot_res[slot] = s._slot_res[base]
    return slot


def _handle(amd, fx, max_range=30.0, **kw):
    """a handle whose slot 0 is the fixture's image"""
    kw.setdefault("num_envs", 1)
    kw.setdefault("num_agents", 1)
    s = amd.BatchSim(max_range=max_range, **kw)
    s.set_map_image(fx[1], fx[2], list(fx[3]))
    s._slot_res = {0: fx[2]}
    return s


def _check_slot(s, d, twin, want, what, max_range=30.0):
    """derived slot d against the model's table `want` and against image-made slot `twin`, whole padded copies included"""
    H, W = want.shape
    got = s.get_map_dt(d)
    assert got.shape == (H, W) and np.array_equal(got, want), "%s: the derived table differs from the model in %d cells" % (what, int((got != want).sum()))
    assert np.array_equal(got, s.get_map_dt(twin)), "%s: the derived table differs from the image-made slot's" % (what,)
    pd, b = _padded(s, d, H, W, max_range)
    pt, _ = _padded(s, twin, H, W, max_range)
    diff = np.argwhere(pd != pt)
    assert diff.size == 0, "%s: the padded copies differ in %d cells, first at padded (row, column) %s (border %d)" % (what, len(diff), diff[0].tolist(), b)
    assert np.array_equal(pd[b:b + H, b:b + W], got)
    border = np.ones(pd.shape, dtype=bool)
    border[b:b + H, b:b + W] = False
    assert np.all(pd[border] == got[H - 1, W - 1]), "%s: a border cell is not cell [H-1][W-1]" % (what,)


# ---- 1. tables and whole padded copies ----------------------------------------------------------------------------------------
def _table_fixtures():
    return {fx[0]: fx for fx in [ref.bar_fixture(4200), ref.bar_fixture(2048), ref.bar_fixture(2049), ref.mid_fixture(), ref.tall_fixture()] + ref.tiny_fixtures()}


@pytest.mark.parametrize("name", ["bar4200", "bar2048", "bar2049", "mid", "tall", "tiny1x1", "tiny1x300", "tiny300x1"])
def test_tables_and_padded_copies(amd, name):
    fx = _table_fixtures()[name]
    _, img, res, origin, lists = fx
    H, W = img.shape
    origin = list(origin)
    s = _handle(amd, fx)
    base0 = s.get_map_dt(0)
    if not ref.free_from_image(img).all():   # (a table without an occupied cell has no EDT to speak of)
        assert np.array_equal(base0, _model(fx, 0)[2])
    base = _add_image(s, img, res, origin)
    other = _add_image(s, np.ascontiguousarray(np.flipud(img)), res, origin)      # an unrelated slot
    base_pad, other_pad = _padded(s, base, H, W)[0], _padded(s, other, H, W)[0]
    for which, (label, ob, _) in enumerate(lists):
        want = _model(fx, which)[0]
        d = _add_derived(s, ob, base)
        d0 = _add_derived(s, ob, 0)
        twin = _add_image(s, _twin_image(fx, which), res, origin)
        _check_slot(s, d, twin, want, (name, label))
        _check_slot(s, d0, twin, want, (name, label, "from slot 0"))
    assert np.array_equal(s.get_map_dt(0), base0)
    assert np.array_equal(_padded(s, base, H, W)[0], base_pad) and np.array_equal(_padded(s, other, H, W)[0], other_pad)
    s.close()


@pytest.mark.parametrize("max_range", ref.EDGE_MAX_RANGES)
def test_border_at_every_workgroup_residue(amd, max_range):
    """24-row tables whose interior ends on a workgroup's last lane, on the next one's first and one lane short, and one that spans
    three workgroups, under a border of 186 (max_range 30), 256 (47.5) and 255 (47.25) cells"""
    widths = ref.edge_widths(max_range)
    b = ref.pad_border(max_range, ref.EDGE_RES)
    assert [(b + w) % 256 for w in widths] == [0, 1, 255, 0]
    s = _handle(amd, ref.edge_fixture(widths[0]), max_range)
    for w in widths:
        fx = ref.edge_fixture(w)
        _, img, res, origin, lists = fx
        origin = list(origin)
        want = _model(fx, 0)[0]
        base = _add_image(s, img, res, origin)
        base_pad = _padded(s, base, 24, w, max_range)[0]
        d = _add_derived(s, lists[0][1], base)
        twin = _add_image(s, _twin_image(fx, 0), res, origin)
        _check_slot(s, d, twin, want, ("edge", max_range, w), max_range)
        assert want[-1, -1] not in (0.0, _model(fx, 0)[2][-1, -1])     # the border's value is the stamp's doing
        s.set_obstacles(d, None)
        _check_slot(s, d, base, _model(fx, 0)[2], ("edge, emptied", max_range, w), max_range)
        s.set_obstacles(d, lists[0][1])
        _check_slot(s, d, twin, want, ("edge, stamped again", max_range, w), max_range)
        assert np.array_equal(_padded(s, base, 24, w, max_range)[0], base_pad)
    s.close()


def _small_fx():
    return ("small", ref.small_image(), ref.SMALL_RES, ref.SMALL_ORIGIN, ref.small_lists())


def test_lists_on_the_small_table(amd):
    """256 obstacles, 255, 1, 0, a box without extent, the disc of radius 1e200, shapes outside the table: each as a slot of its
    own, then all of them in turn on ONE slot (the same address throughout); after the 256 the empty list gives the base back"""
    fx = _small_fx()
    _, img, res, origin, lists = fx
    H, W = img.shape
    origin = list(origin)
    s = _handle(amd, fx)
    base0 = s.get_map_dt(0)
    assert np.array_equal(base0, _model(fx, 0)[2])
    other = _add_image(s, np.ascontiguousarray(np.flipud(img)), res, origin)
    other_pad = _padded(s, other, H, W)[0]
    twins = []
    for which, (label, ob, _) in enumerate(lists):
        d = _add_derived(s, ob, 0)
        twins.append(_add_image(s, _twin_image(fx, which), res, origin))
        _check_slot(s, d, twins[-1], _model(fx, which)[0], ("small", label))
    huge = [l[0] for l in lists].index("1e200 disc")
    assert _model(fx, huge)[0].max() == 0.0 and np.all(_padded(s, twins[huge], H, W)[0] == 0.0)
    for label in ("0", "zero box", "outside"):
        assert np.array_equal(_model(fx, [l[0] for l in lists].index(label))[0], base0)
    one = _add_derived(s, lists[0][1], 0)
    addr = s.map_table_address(one)
    order = list(range(len(lists))) + [0, 3, huge, 0]      # ... 256, none, everything, 256
    for which in order:
        s.set_obstacles(one, lists[which][1])
        assert s.map_table_address(one) == addr
        _check_slot(s, one, twins[which], _model(fx, which)[0], ("small, re-stamped", lists[which][0]))
    assert np.array_equal(s.get_map_dt(0), base0) and np.array_equal(_padded(s, other, H, W)[0], other_pad)
    s.close()


def test_restamps_on_the_wide_table(amd):
    """bar, discs only, bar on one slot: Wa goes 4200 -> 26 -> 4200 over the same scratch"""
    fx = ref.bar_fixture(4200)
    _, img, res, origin, lists = fx
    origin = list(origin)
    s = _handle(amd, fx)
    base = _add_image(s, img, res, origin)
    twins = [_add_image(s, _twin_image(fx, which), res, origin) for which in (0, 1)]
    d = _add_derived(s, lists[0][1], base)
    addr = s.map_table_address(d)
    for which in (0, 1, 0, 1, 0):
        s.set_obstacles(d, lists[which][1])
        assert s.map_table_address(d) == addr
        _check_slot(s, d, twins[which], _model(fx, which)[0], ("wide, re-stamped", lists[which][0]))
    s.close()


def test_restamps_alternate_between_two_shapes_on_one_handle(amd):
    """a derived slot of the 96 x 128 table and one of the 40 x 4200 table, each from its own image-made base, re-stamped in turn
    for three rounds: the grow-only scratch (mask, g, cols) sized for one shape serves the other; each re-stamp leaves the other
    slot as it was"""
    small = ("small, lists 0 and 1", ref.small_image(), ref.SMALL_RES, ref.SMALL_ORIGIN, [("list 0", ref.small_obstacles(0), None), ("list 1", ref.small_obstacles(1), None)])
    wide = ref.bar_fixture(4200)
    s = _handle(amd, small)
    fxs = (small, wide)
    bases = [_add_image(s, fx[1], fx[2], list(fx[3])) for fx in fxs]
    twins = [[_add_image(s, _twin_image(fx, which), fx[2], list(fx[3])) for which in (0, 1)] for fx in fxs]
    ds = [_add_derived(s, fx[4][0][1], b) for fx, b in zip(fxs, bases)]
    addrs = [s.map_table_address(d) for d in ds]
    holds = [0, 0]
    for rnd in range(3):
        for i in (0, 1):
            holds[i] = (rnd + 1) % 2
            s.set_obstacles(ds[i], fxs[i][4][holds[i]][1])
            for j in (0, 1):
                assert s.map_table_address(ds[j]) == addrs[j]
                _check_slot(s, ds[j], twins[j][holds[j]], _model(fxs[j], holds[j])[0], ("round %d, after re-stamping %s" % (rnd, fxs[i][0]), fxs[j][0]))
    for fx, b in zip(fxs, bases):
        assert np.array_equal(s.get_map_dt(b), _model(fx, 0)[2])
    s.close()


# ---- 2. the rollout on a derived slot -------------------------------------------------------------------------------------------
ROLL_CHANNELS = ("end_x", "end_y", "end_cos", "end_sin", "end_v", "end_yaw_rate", "alive", "min_clear")   # (no track on these slots: no progress)


def _roll_settings(frame="ego", channels=ROLL_CHANNELS, scale=None):
    return rref.settings(k=ref.ROLL_K, horizon=ref.ROLL_H, repeat=ref.ROLL_REPEAT, margin=ref.ROLL_MARGIN, frame=frame, channels=channels,
                         scale={"end_x": 2.0, "alive": float(ref.ROLL_H * ref.ROLL_REPEAT)} if scale is None else scale)


def _check_unit(s, flown, want, got, what):
    """tests/test_gpu_rollout.py's gate: raw values rel_err < 1e-5, every float32 output exactly (float)(raw / scale), ALIVE exact but
    for candidates within 1e-9 m of the margin (tests/test_obstacles_host.py: the model leaves out none of these) -> candidates left out"""
    out, traj, raw, traw = got
    w_raw, w_traw = want[1], want[3]
    keep = flown[4] >= 1e-9
    assert np.array_equal(raw[..., rref.ALIVE][keep], w_raw[..., rref.ALIVE][keep]), "%s: ALIVE differs" % (what,)
    err = max(rel_err(raw[keep], w_raw[keep]), rel_err(traw[keep], w_traw[keep]))
    assert err < 1e-5, "%s: rel_err %.3e" % (what, err)
    scale = np.array([float(s["scale"].get(c, 1.0)) for c in rref.CHANNELS])
    bits = [b for b, c in enumerate(rref.CHANNELS) if c in s["channels"]]
    with np.errstate(over="ignore", invalid="ignore"):
        own = (raw[..., bits] / scale[bits]).astype(np.float32)
        own_traj = (traw / scale[:4]).astype(np.float32)
    assert np.array_equal(rref.bits(out), rref.bits(own)), "%s: a float32 output is not (float)(raw / scale)" % (what,)
    assert np.array_equal(rref.bits(traj), rref.bits(own_traj)), "%s: a float32 trajectory value is not (float)(raw / scale)" % (what,)
    return int(np.count_nonzero(~keep)), keep.size


def test_rollout_unit_form_on_a_derived_slot(amd):
    start, actions = ref.rollout_case()
    fx = _small_fx()
    s = _handle(amd, fx)
    d = s.add_obstacle_map(ref.small_obstacles(0))
    left = total = 0
    for which in (0, 1):
        if which:
            s.set_obstacles(d, ref.small_obstacles(1))
        assert np.array_equal(s.get_map_dt(d), ref.rollout_table(which))
        flown = ref.rollout_flown(which)
        for frame in ("map", "ego"):
            st = _roll_settings(frame)
            got = s.rollout_rows(amd.Rollout(**st), start, actions, slot=d, raw=True)
            a, b = _check_unit(st, flown, rref.render(st, start, flown, None), got, ("list %d" % which, frame))
            left, total = left + a, total + b
        # slot 0 is the base, whatever the derived slot holds
        st = _roll_settings("map")
        got = s.rollout_rows(amd.Rollout(**st), start, actions, slot=0, raw=True)
        _check_unit(st, ref.rollout_flown("base"), rref.render(st, start, ref.rollout_flown("base"), None), got, ("base beside list %d" % which,))
    assert left * 100 <= total and left == 0, (left, total)
    s.close()


def _device_rollout(s, p, d_cand):
    out, traj = s.rollout_device(p, d_cand)
    res = out.download(), traj.download()
    out.free()
    traj.free()
    return res


@pytest.mark.parametrize("late", [False, True])
def test_rollout_device_form_on_a_derived_slot(amd, late):
    """32 envs x 2 cars, eight envs each on slot 0, the derived slot, the image-made twin of list 0 and that of list 1; the sixteen
    rows of the case on each.  late: the derived slot is added AFTER a first set_env_maps, which is then called again — the add finds
    no device-side slot table entry to refresh, the second set_env_maps must bring the out-of-bounds value along.  No set_env_maps
    follows the re-stamp: the value the rollout reads there is the one the re-stamp wrote on the device."""
    start, actions = ref.rollout_case()
    fx = _small_fx()
    _, img, res, origin, _ = fx
    origin = list(origin)
    E, A, R = 32, 2, 16
    masks = [ref.stamp_mask(ref.small_obstacles(w), ref.SMALL_H, ref.SMALL_W, res, origin) for w in (0, 1)]
    s = _handle(amd, fx, num_envs=E, num_agents=A)
    im = [s.add_map_image(ref.image_with_stamps(img, m), res, origin) for m in masks]
    if late:
        s.set_env_maps([0] * 16 + [im[0]] * 8 + [im[1]] * 8)
    d = s.add_obstacle_map(ref.small_obstacles(0))
    s.set_env_maps([0] * 8 + [d] * 8 + [im[0]] * 8 + [im[1]] * 8)
    rows = np.tile(start, (4, 1))
    s.reset(np.ascontiguousarray(rows[:, [0, 1, 4]]))
    s.set_state(rows[:, :7], rows[:, 7:9], rows[:, 9].astype(np.int32))
    st = _roll_settings("ego", ROLL_CHANNELS, scale={"end_x": 2.0})     # (ALIVE unscaled: whole numbers in float32)
    p = amd.Rollout(**st)
    d_cand = s.device_array(actions.shape)
    d_cand.upload(actions)
    alive_bit = ROLL_CHANNELS.index("alive")
    steps = float(ref.ROLL_H * ref.ROLL_REPEAT)
    runs = []
    for which in (0, 1):
        if which:
            s.set_obstacles(d, ref.small_obstacles(1))
        out, traj = _device_rollout(s, p, d_cand)
        g = lambda a, q: a[q * R:(q + 1) * R]   # noqa: E731
        assert np.array_equal(rref.bits(g(out, 1)), rref.bits(g(out, 2 + which))) and np.array_equal(rref.bits(g(traj, 1)), rref.bits(g(traj, 2 + which))), \
            "list %d: agents on the derived slot differ from their twins on the image-made slot" % which
        for q, slot in ((0, 0), (1, d), (2, im[0]), (3, im[1])):
            u_out, u_traj = s.rollout_rows(p, start, actions, slot=slot)
            assert np.array_equal(rref.bits(u_out), rref.bits(g(out, q))) and np.array_equal(rref.bits(u_traj), rref.bits(g(traj, q))), \
                "list %d: the device form differs from the unit form of slot %d" % (which, slot)
        assert np.array_equal(g(out, 1)[..., alive_bit], ref.rollout_flown(which)[1].astype(np.float32))
        runs.append(out[..., alive_bit])
    leavers = ref.rollout_left_table(1)
    on_d, on_0 = runs[0][R:2 * R], runs[0][:R]
    changed = (runs[1][R:2 * R] != on_d) & leavers
    assert np.count_nonzero(changed) >= 20 and np.all(runs[1][R:2 * R][leavers] == steps) and np.all(on_d[leavers] < steps)
    assert np.array_equal(runs[1][:R], on_0) and np.all(on_0[leavers] == steps)
    d_cand.free()
    s.close()


# ---- 2b. the MPPI planner on a derived slot ---------------------------------------------------------------------------------------
MPPI_K, MPPI_H, MPPI_REPEAT = 8, 5, 4


def _corridor_track(amd):
    """a closed track through the small fixture's corridor: 48 points round the ring"""
    return amd.Track(np.array([ref.small_corridor_pose(p)[:2] for p in np.linspace(0.0, 2.0 * np.pi, 48, endpoint=False)]))


def _table_oracle(which):
    from oracle import orc
    so = orc.ScanOracle(1080, 4.7)
    so.set_map_dt(ref.rollout_table(which), ref.SMALL_RES, list(ref.SMALL_ORIGIN))
    return so


def test_mppi_on_a_derived_slot(amd):
    """the planner's unit form on the derived slot against tests/mppi_ref.py on the model's table, before and after a re-stamp that
    lifts the out-of-bounds value over the margin, and bit for bit against the image-made twin; one device-form call per list with
    eight envs each on slot 0, the derived slot and the twin, each group against the unit form of its slot.  The rows that leave the
    table (ROLL_LEAVERS) die there under list 0 and live on under list 1: their action changes, and it is the model's."""
    import mppi_ref as mref
    from oracle import orc
    start, _ = ref.rollout_case()
    R = start.shape[0]
    fx = _small_fx()
    _, img, res, origin, _ = fx
    origin = list(origin)
    E, A = 24, 2
    N = E * A
    masks = [ref.stamp_mask(ref.small_obstacles(w), ref.SMALL_H, ref.SMALL_W, res, origin) for w in (0, 1)]
    s = _handle(amd, fx, num_envs=E, num_agents=A)
    im = [s.add_map_image(ref.image_with_stamps(img, m), res, origin) for m in masks]
    d = s.add_obstacle_map(ref.small_obstacles(0))
    track = _corridor_track(amd)
    for slot in [0, d] + im:
        s.set_track(track, slot)
    st = mref.settings(k=MPPI_K, horizon=MPPI_H, repeat=MPPI_REPEAT, margin=ref.ROLL_MARGIN, w_progress=3.0, w_lat=0.5, speed_max=7.0, v_init=4.0,
                       sigma_speed=1.5)
    mp = mref.mppi_of(amd, st)
    params = np.tile(orc.params_vec(), (R, 1))
    rng = np.random.default_rng(77)
    nom = np.stack([rng.uniform(-0.2, 0.2, (R, MPPI_H)), rng.uniform(3.0, 6.0, (R, MPPI_H))], axis=-1)
    words = mref.streams_for(91, range(R))
    rows = np.tile(start, (3, 1))
    s.reset(np.ascontiguousarray(rows[:, [0, 1, 4]]))
    s.set_state(rows[:, :7], rows[:, 7:9], rows[:, 9].astype(np.int32))
    s.set_mppi(mp, None, seed=92)
    stats = {"rows": 0, "left_out": 0, "rel_err": 0.0}
    acts = []
    for which in (0, 1):
        if which:
            s.set_obstacles(d, ref.small_obstacles(1))
        assert np.array_equal(s.get_map_dt(d), ref.rollout_table(which))
        want = mref.plan(st, _table_oracle(which), start, params, nom, words, 1, None, track)
        got = s.mppi_rows(mp, start, nom, words, slot=d, params=params)
        mref.check_rows(st, want, got, "list %d" % which, stats)
        twin = s.mppi_rows(mp, start, nom, words, slot=im[which], params=params)
        for key in got:
            assert mref.same_bits(got[key], twin[key]), "list %d: %s on the derived slot differs from the image-made twin's" % (which, key)
        acts.append((got["actions"], got["info"], want["actions"], want["raw"][:, :, 0]))
        # the device form: no set_env_maps follows the re-stamp
        s.set_env_maps([0] * 8 + [d] * 8 + [im[which]] * 8)
        nom0, words0 = s.get_mppi_state()
        count = s.get("step_count")["step_count"]
        act, info = s.mppi(np.zeros((N, 2)), info=True)
        nom1, words1 = s.get_mppi_state()
        for q, slot in enumerate((0, d, im[which])):
            idx = np.arange(q * R, (q + 1) * R)
            unit = s.mppi_rows(mp, start, nom0[idx], words0[idx], slot=slot, fresh=count[idx])
            for key, mine in (("actions", act), ("info", info), ("nominal", nom1), ("streams", words1)):
                assert mref.same_bits(unit[key], mine[idx]), "list %d: %s of the device form differs from the unit form of slot %d" % (which, key, slot)
    print("mppi on a derived slot: %d rows, %d left out, largest rel_err %.3e" % (stats["rows"], stats["left_out"], stats["rel_err"]))
    assert stats["left_out"] * 100 <= stats["rows"], stats
    # a row whose candidates leave the table: dead there under list 0, alive to the end under list 1
    steps = float(MPPI_H * MPPI_REPEAT)
    moved = [r for r in ref.ROLL_LEAVERS if np.any(acts[0][3][r] < steps) and np.all(acts[1][3][r] == steps) and not mref.same_bits(acts[0][0][r], acts[1][0][r])]
    assert moved, "no leaver's action changed with the re-stamp"
    for r in moved:
        assert not np.array_equal(acts[0][2][r], acts[1][2][r]) and rel_err(acts[1][0][r], acts[1][2][r]) < 1e-5 and rel_err(acts[0][0][r], acts[0][2][r]) < 1e-5
    s.close()


# ---- 3. a re-stamp behind calls that ride the env blocks --------------------------------------------------------------------------
BLOCK_E, BLOCK_A = 256, 2


def _block_poses():
    rng = np.random.default_rng(2)
    return np.array([[ref.small_corridor_pose(p), ref.small_corridor_pose(p + 0.6, 0.05)] for p in rng.uniform(0, 2 * np.pi, BLOCK_E)]).reshape(BLOCK_E * BLOCK_A, 3)


def _block_sim(amd, which):
    s = _handle(amd, _small_fx(), num_envs=BLOCK_E, num_agents=BLOCK_A, step_groups=2)
    d = s.add_obstacle_map(ref.small_obstacles(which))
    s.set_env_maps([d if e % 2 else 0 for e in range(BLOCK_E)])
    s.reset(_block_poses())
    return s, d


def _obs(s):
    o = s.get("state", "scans", "collisions", "in_collision", "step_count")
    return {k: np.array(v, copy=True) for k, v in o.items()}


def test_restamp_behind_a_rollout_on_two_blocks(amd):
    """two device steps, rollout_device, set_obstacles(list 1), rollout_device into a second buffer, a step, set_obstacles(list 0), a
    step — with no host synchronisation, and with sync() after every call: the same two summaries and the same final observations.
    The first rollout goes out behind the two-block step on both block streams without a join; the re-stamp must wait for it.  The
    first summary is that of a handle that only ever had list 0, the second that of one that only ever had list 1 (in the same state).
    512 agents x 256 candidates x 64 actions held 8 steps: the rollout is timed once with the handle's timer and must take between
    1 ms and 1 s, so that it is still running when the host reaches the re-stamp.  Measured on an MI355X: 4.5 ms."""
    N = BLOCK_E * BLOCK_A
    lists = [ref.small_obstacles(0), ref.small_obstacles(1)]
    p = amd.Rollout(k=256, horizon=64, repeat=8, channels=("end_x", "end_y", "alive", "min_clear"), margin=0.02, frame="ego")
    rng = np.random.default_rng(12)
    cand = np.stack([rng.uniform(-0.3, 0.3, (256, 64)), rng.uniform(0.05, 0.5, (256, 64))], axis=-1)
    acts = np.stack([rng.uniform(-0.2, 0.2, N), rng.uniform(0.5, 3.0, N)], axis=1)
    runs = []
    for synced in (False, True):
        s, d = _block_sim(amd, 0)
        sync = s.sync if synced else (lambda: None)
        d_act, d_cand = s.device_array((N, 2)), s.device_array(cand.shape)
        d_act.upload(acts)
        d_cand.upload(cand)
        bufs = [s.device_array(p.shape(N), np.float32) for _ in range(2)]
        s.step_device(d_act)          # (the first step after a reset forks from the main stream)
        sync()
        s.step_device(d_act)
        sync()
        assert s.step_groups()[2] == 2
        s.rollout_device(p, d_cand, bufs[0])
        sync()
        s.set_obstacles(d, lists[1])
        sync()
        s.rollout_device(p, d_cand, bufs[1])
        sync()
        s.step_device(d_act)
        sync()
        s.set_obstacles(d, lists[0])
        sync()
        s.step_device(d_act)
        runs.append((bufs[0].download(), bufs[1].download(), _obs(s)))
        assert np.array_equal(s.get_map_dt(d), ref.rollout_table(0))
        s.close()
    for i, what in enumerate(("first rollout", "second rollout")):
        assert np.array_equal(rref.bits(runs[0][i]), rref.bits(runs[1][i])), "%s: unsynchronised against synchronised" % what
    for k in runs[0][2]:
        assert np.array_equal(runs[0][2][k], runs[1][2][k], equal_nan=True), "final %s: unsynchronised against synchronised" % k
    # handles that only ever had one list, in the state the rollouts started from
    s0, _ = _block_sim(amd, 0)
    s0.step(acts)
    s0.step(acts)
    blob = s0.save_state()
    d_cand = s0.device_array(cand.shape)
    d_cand.upload(cand)
    s0.sync()
    s0.timer_begin()
    buf = s0.rollout_device(p, d_cand)
    ms = s0.timer_end_ms()
    print("rollout of %d agents x 256 candidates x 512 steps: %.3f ms" % (N, ms))
    assert 1.0 < ms < 1000.0, ms
    only0 = buf.download()
    s0.close()
    s1, _ = _block_sim(amd, 1)
    s1.load_state(blob)
    d_cand = s1.device_array(cand.shape)
    d_cand.upload(cand)
    only1 = s1.rollout_device(p, d_cand).download()
    s1.close()
    assert np.array_equal(rref.bits(runs[0][0]), rref.bits(only0)), "the first rollout read a table the re-stamp had begun to write"
    assert np.array_equal(rref.bits(runs[0][1]), rref.bits(only1)), "the second rollout did not read list 1's table"
    assert not np.array_equal(only0, only1)


def test_restamp_behind_the_controllers_on_two_blocks(amd):
    """the same with follow_gap_device on scripted cars in the rollout's place: the table's reader is the next step's scan"""
    N = BLOCK_E * BLOCK_A
    lists = [ref.small_obstacles(0), ref.small_obstacles(1)]
    acts = np.tile([0.0, 1.0], (N, 1))

    def run(synced, restamp=True, first=0):
        s, d = _block_sim(amd, first)
        sync = s.sync if synced else (lambda: None)
        s.set_controllers(np.zeros(N, dtype=np.int32), [amd.GapFollower()])
        d_acts = [s.device_array((N, 2)) for _ in range(3)]
        for a in d_acts:
            a.upload(acts)
        s.step_device(d_acts[0])
        sync()
        s.step_device(d_acts[0])
        sync()
        assert s.step_groups()[2] == 2
        s.follow_gap_device(d_acts[1])
        sync()
        if restamp:
            s.set_obstacles(d, lists[1])
            sync()
        s.follow_gap_device(d_acts[2])
        sync()
        s.step_device(d_acts[2])
        sync()
        mid = _obs(s) if synced else None
        if restamp:
            s.set_obstacles(d, lists[0])
            sync()
        s.step_device(d_acts[2])
        res = ([a.download() for a in d_acts[1:]], _obs(s), mid)
        s.close()
        return res
    free, tied, plain = run(False), run(True), run(True, restamp=False)
    for i in (0, 1):
        assert np.array_equal(free[0][i].view(np.uint64), tied[0][i].view(np.uint64)), "controller actions %d: unsynchronised against synchronised" % i
    for k in free[1]:
        assert np.array_equal(free[1][k], tied[1][k], equal_nan=True), "final %s: unsynchronised against synchronised" % k
    # the controllers read the scans of list 0 both times (no step in between), as on a handle that is never re-stamped
    assert np.array_equal(free[0][0].view(np.uint64), plain[0][0].view(np.uint64)) and np.array_equal(free[0][1].view(np.uint64), free[0][0].view(np.uint64))
    assert not np.array_equal(free[0][0], acts)
    # the step behind the re-stamp scanned list 1's table: odd envs see other ranges than without the re-stamp, even envs (slot 0) the same
    odd = np.repeat(np.arange(BLOCK_E) % 2 == 1, BLOCK_A)
    assert not np.array_equal(tied[2]["scans"][odd], plain[2]["scans"][odd]) and np.array_equal(tied[2]["scans"][~odd], plain[2]["scans"][~odd])


# ---- 4. render and clone ------------------------------------------------------------------------------------------------------------
def test_render_two_derived_slots_in_one_call(amd):
    fx = _small_fx()
    _, img, res, origin, _ = fx
    origin = list(origin)
    lists = [ref.small_obstacles(0), ref.small_obstacles(1)]
    masks = [ref.stamp_mask(ob, ref.SMALL_H, ref.SMALL_W, res, origin) for ob in lists]
    E = 8
    s = _handle(amd, fx, num_envs=E, num_agents=1)
    d1, d2 = s.add_obstacle_map(lists[1]), s.add_obstacle_map(lists[0])
    tw = [s.add_map_image(ref.image_with_stamps(img, m), res, origin) for m in masks]
    env_map = [d1, d2, tw[0], tw[1]] * 2
    s.set_env_maps(env_map)
    poses = np.array([ref.small_corridor_pose(0.9)] * 4 + [ref.small_corridor_pose(3.6, 0.2)] * 4)
    s.reset(poses)
    s.step(np.zeros((E, 2)))
    views = [dict(width=96, height=96, view="world", m_per_px=0.08, center=ref.small_cell_xy(48.0, 64.0), angle=0.0, layers=("map",)),
             dict(width=64, height=64, view="ego", m_per_px=0.05, fwd_offset=0.5, layers=("map",))]
    on = lambda slot: [e for e in range(E) if env_map[e] == slot]   # noqa: E731
    before = [s.render(**v) for v in views]
    for f in before:
        assert np.array_equal(f[on(d2)], f[on(tw[0])]) and np.array_equal(f[on(d1)], f[on(tw[1])]) and not np.array_equal(f[on(d1)], f[on(d2)])
    s.set_obstacles(d2, lists[1])
    after = [s.render(**v) for v in views]
    for f, g in zip(before, after):
        assert np.array_equal(g[on(d1)], f[on(d1)]), "re-stamping one derived slot changed the frames of the other's agents"
        assert np.array_equal(g[on(tw[0])], f[on(tw[0])]) and np.array_equal(g[on(tw[1])], f[on(tw[1])])
        assert np.array_equal(g[on(d2)], g[on(tw[1])]), "the re-stamped slot's frames are not its image-made twin's"
        assert not np.array_equal(g[on(d2)], f[on(d2)])
    s.close()


def test_clone_from_an_env_on_a_derived_slot(amd):
    """clone_envs under two env blocks, from envs on the derived slot (one per block) into envs on slot 0: the destinations' env-map
    entry becomes the derived slot and they step like the source, bit for bit, for 10 steps"""
    E, A = BLOCK_E, BLOCK_A
    s = _handle(amd, _small_fx(), num_envs=E, num_agents=A, step_groups=2)
    d = s.add_obstacle_map(ref.small_obstacles(0))
    src, dst = [1, 131], [4, 200]
    env_map = np.zeros(E, dtype=np.int32)
    env_map[src] = d
    s.set_env_maps(env_map)
    poses = _block_poses().reshape(E, A, 3)
    hx, hy = ref.small_cell_xy(38.0, 26.5)
    poses[1, 0] = (hx, hy, ref.SMALL_ORIGIN[2] + np.pi / 2)      # 12 cells in front of list 0's first box
    s.reset(poses.reshape(E * A, 3))
    rng = np.random.default_rng(3)
    acts = np.stack([rng.uniform(-0.2, 0.2, (E, A)), rng.uniform(0.5, 3.0, (E, A))], axis=2)
    acts[dst] = acts[src]
    acts[1, 0] = (0.0, 3.0)
    acts[4, 0] = (0.0, 3.0)
    acts = acts.reshape(E * A, 2)
    for _ in range(3):
        s.step(acts)
    s.clone_envs(src, dst)
    blob = s.save_envs(src + dst)
    assert blob.header["columns"] == ("agent", "env_map")
    assert np.frombuffer(blob.data[-256:].tobytes(), dtype=np.int32)[:4].tolist() == [d] * 4   # the env-map column: one int32 per env, the blob's last section
    rows = lambda e: [e * A + a for a in range(A)]   # noqa: E731
    for t in range(10):
        s.step(acts)
        o = _obs(s)
        for a, b in zip(src, dst):
            for k in o:
                assert np.array_equal(o[k][rows(a)], o[k][rows(b)], equal_nan=True), "step %d: env %d does not step like env %d (%s)" % (t, b, a, k)
    # and the table mattered: the same run with every env on slot 0 gives the sources (hence their clones) other ranges
    p = _handle(amd, _small_fx(), num_envs=E, num_agents=A, step_groups=2)
    p.reset(poses.reshape(E * A, 3))
    for _ in range(13):
        p.step(acts)
    plain = _obs(p)["scans"]
    for a in src:
        assert not np.array_equal(plain[rows(a)], o["scans"][rows(a)])
    assert np.array_equal(plain[rows(7)], o["scans"][rows(7)])       # (an env that stayed on slot 0)
    p.close()
    s.close()
