"""The host plumbing the two armed features share, the MPPI planner (f110_mppi_*) and the particle filter (f110_pf_*,
DESIGN §6l): the refusals of an armed list and of a call with nothing armed, held to their code AND their full text; the streams
both features give the same agents; and that arming, re-arming and disarming one feature leaves the other alone, bit for bit.

One shape throughout: 4 envs of 2 agents, 16 beams, example_map registered as two slots (envs alternate), step_groups = 2, so a
step goes out as two env blocks and a call right behind it rides the blocks' streams; the planner
with k = 4, horizon = 3, repeat = 2 and no track weight; the filter with 17 particles (lane grouping 32 with a ragged tail) and
beams 0, 4, 8, 12."""
import ctypes as C
import gc

import numpy as np
import pytest

from _util import bench_start_poses, load_map_image

pytestmark = pytest.mark.gpu

E, A, B = 4, 2, 16
N = E * A
MPPI = dict(k=4, horizon=3, repeat=2, w_progress=0.0, w_lat=0.0)
PF = dict(particles=17, n_beams=4, beam_first=0, beam_stride=4)
FEATURES = ("mppi", "pf")
# the library's texts, as its source spells them (N = 8)
FORM = {"mppi": "mppi: a spec, the agents and their streams, or NULL, NULL, 0, NULL", "pf": "pf: a spec, the agents and their streams, or NULL, NULL, 0, NULL"}
COUNT = {"mppi": "mppi: %d armed agents, but the handle has 1..8", "pf": "pf: %d armed agents, but the handle has 1..8"}
RANGE = {"mppi": "mppi: agents[%d] = %d is outside 0..7", "pf": "pf: agents[%d] = %d is outside 0..7"}
ORDER = {"mppi": "mppi: the agents are not strictly ascending at [%d]", "pf": "pf: the agents are not strictly ascending at [%d]"}
UNARMED = {"mppi": "mppi: no planner is armed (f110_mppi_set)", "pf": "pf: no filter is armed (f110_pf_set)"}
CLASH = "mppi: agent %d has a follow-the-gap controller (f110_controllers_set)"
AGENTS_TEXT = "agents must be a strictly ascending list of 1 .. 8 indices within 0 .. 7"


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _handle(amd):
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, step_groups=2)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    assert s.add_map_image(*load_map_image("example_map")) == 1
    s.set_env_maps(np.arange(E) % 2)
    return s


@pytest.fixture
def sim(amd):
    s = _handle(amd)
    yield s
    s.close()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _words(n):
    return np.arange(1, 4 * n + 1, dtype=np.uint64).reshape(n, 4)


class Raw(object):
    """the raw entry points of one feature on one handle: set with any argument left out, and _device, _get, _put"""

    def __init__(self, amd, s, who):
        from f1tenth_gym_amd import _ffi
        self.ffi, self.L, self.s, self.who = _ffi, _ffi.lib(), s, who
        self.sp = (amd.Mppi(**MPPI) if who == "mppi" else amd.ParticleFilter(**PF)).spec()
        self.out = s.device_array((N, 2 if who == "mppi" else 3))

    def set(self, agents, m=None, spec=True, streams=True):
        ag = None if agents is None else np.asarray(agents, dtype=np.int32)
        w = _words(max(len(agents or ()), 1)) if streams else None
        fn = self.L.f110_mppi_set if self.who == "mppi" else self.L.f110_pf_set
        return fn(self.s._h, C.byref(self.sp) if spec else None, None if ag is None else self.ffi.i32ptr(ag),
                  (0 if ag is None else len(ag)) if m is None else m, None if w is None else w.ctypes.data_as(self.ffi._u64p))

    def device(self):
        fn = self.L.f110_mppi_device if self.who == "mppi" else self.L.f110_pf_device
        return fn(self.s._h, self.out.ptr, None)

    def get_put(self, put):
        buf, w = np.zeros((N, 17, 3)), _words(N)
        if self.who == "mppi":
            return (self.L.f110_mppi_put if put else self.L.f110_mppi_get)(self.s._h, self.ffi.dptr(buf), w.ctypes.data_as(self.ffi._u64p))
        return (self.L.f110_pf_put if put else self.L.f110_pf_get)(self.s._h, self.ffi.dptr(buf), None, None, w.ctypes.data_as(self.ffi._u64p))

    def refused(self, rc, code, text):
        err = self.ffi.last_error(self.s._h)
        assert rc == code and err and err == text, (rc, err, text)


# ---- the refusals, character for character ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("who", FEATURES)
def test_armed_list_refusals_keep_their_code_and_text(amd, sim, who):
    r = Raw(amd, sim, who)
    INVALID, STATE = r.ffi.ERR_INVALID, r.ffi.ERR_STATE
    # nothing is armed yet
    r.refused(r.device(), STATE, UNARMED[who])
    r.refused(r.get_put(False), STATE, UNARMED[who])
    r.refused(r.get_put(True), STATE, UNARMED[who])
    # the partial-NULL forms
    r.refused(r.set([1, 2], spec=False), INVALID, FORM[who])
    r.refused(r.set(None, m=2), INVALID, FORM[who])
    r.refused(r.set([1, 2], streams=False), INVALID, FORM[who])
    r.refused(r.set(None, m=2, spec=False, streams=False), INVALID, FORM[who])
    r.refused(r.set(None, m=0, streams=False), INVALID, FORM[who])
    # the count
    r.refused(r.set([1, 2], m=0), INVALID, COUNT[who] % 0)
    r.refused(r.set(list(range(N + 1))), INVALID, COUNT[who] % (N + 1))
    # an index out of range, a repeated and a descending one; the first bad index decides
    r.refused(r.set([-1, 2]), INVALID, RANGE[who] % (0, -1))
    r.refused(r.set([1, 2, N]), INVALID, RANGE[who] % (2, N))
    r.refused(r.set([1, 1]), INVALID, ORDER[who] % 1)
    r.refused(r.set([3, 1, 2]), INVALID, ORDER[who] % 1)
    r.refused(r.set([0, 2, 1, N]), INVALID, ORDER[who] % 2)
    r.refused(r.set([0, N, 1]), INVALID, RANGE[who] % (1, N))
    # none of them armed anything, and the disarm form of nothing is fine
    r.refused(r.device(), STATE, UNARMED[who])
    assert r.set(None, m=0, spec=False, streams=False) == r.ffi.OK
    # a good list arms; a refused one after it leaves it armed
    assert r.set([1, 2, 5]) == r.ffi.OK, r.ffi.last_error(sim._h)
    r.refused(r.set([5, 2]), INVALID, ORDER[who] % 1)
    assert r.device() == r.ffi.OK, r.ffi.last_error(sim._h)
    assert r.get_put(False) == r.ffi.OK
    assert r.set(None, m=0, spec=False, streams=False) == r.ffi.OK
    r.refused(r.device(), STATE, UNARMED[who])
    r.out.free()


def test_planner_refuses_an_agent_with_a_controller_where_the_walk_meets_it(amd, sim):
    r, f = Raw(amd, sim, "mppi"), Raw(amd, sim, "pf")
    INVALID = r.ffi.ERR_INVALID
    assign = np.full(N, -1, dtype=np.int32)
    assign[3] = 0
    sim.set_controllers(assign, [amd.GapFollower()])
    r.refused(r.set([3]), INVALID, CLASH % 3)
    r.refused(r.set([1, 3, 5]), INVALID, CLASH % 3)
    r.refused(r.set([5, 3]), INVALID, ORDER["mppi"] % 1)          # descending AND clashing at [1]: the order is checked first
    r.refused(r.set([3, 1]), INVALID, CLASH % 3)                  # clashing at [0], descending at [1]: the first bad index decides
    r.refused(r.set([3, N]), INVALID, CLASH % 3)
    r.refused(r.set([N, 3]), INVALID, RANGE["mppi"] % (0, N))
    assert r.set([1, 2, 5]) == r.ffi.OK, r.ffi.last_error(sim._h)
    assert f.set([3]) == f.ffi.OK, f.ffi.last_error(sim._h)        # the filter drives nothing: a scripted car may be localised
    sim.clear_controllers()
    assert r.set([3]) == r.ffi.OK, r.ffi.last_error(sim._h)
    r.out.free()
    f.out.free()


def test_opponent_term_needs_an_armed_planner(amd, sim):
    from f1tenth_gym_amd import _ffi
    L, osp = _ffi.lib(), amd.Opponents().spec()
    args = (C.c_double(1.0), C.c_double(1.0), C.c_double(1.0))
    assert L.f110_mppi_set_opponents(sim._h, C.byref(osp), *args) == _ffi.ERR_STATE
    assert _ffi.last_error(sim._h) == UNARMED["mppi"]
    assert L.f110_mppi_set_opponents(sim._h, None, *args) == _ffi.OK          # detaching nothing is fine
    sim.set_mppi(MPPI, agents=[1, 2, 5])
    assert L.f110_mppi_set_opponents(sim._h, C.byref(osp), *args) == _ffi.OK, _ffi.last_error(sim._h)
    sim.clear_mppi()
    assert L.f110_mppi_set_opponents(sim._h, C.byref(osp), *args) == _ffi.ERR_STATE
    assert _ffi.last_error(sim._h) == UNARMED["mppi"]


def test_python_refusals_keep_their_type_and_text(amd, sim):
    from f1tenth_gym_amd import _ffi
    arm = {"mppi": lambda **kw: sim.set_mppi(MPPI, **kw), "pf": lambda **kw: sim.set_particle_filter(PF, **kw)}
    for who in FEATURES:
        for bad in ([], [-1, 2], [1, N], [2, 2], [3, 1]):
            with pytest.raises(ValueError) as e:
                arm[who](agents=bad)
            assert str(e.value) == AGENTS_TEXT, (who, bad)
        with pytest.raises(ValueError) as e:
            arm[who](agents=[1, 2], agent_base=-1)
        assert str(e.value) == "agent_base must be >= 0, got -1"
    for call, text in ((sim.get_mppi_state, "no planner is armed (set_mppi)"), (sim.set_mppi_state, "no planner is armed (set_mppi)"),
                       (sim.get_pf_state, "no filter is armed (set_particle_filter)"), (sim.set_pf_state, "no filter is armed (set_particle_filter)")):
        with pytest.raises(_ffi.F110LibraryError) as e:
            call()
        assert str(e.value) == text
    mp, pf = arm["mppi"](agents=[1, 2, 5]), arm["pf"](agents=[0, 5, 7])
    for call in (lambda: sim.set_mppi_state(streams=_words(2)), lambda: sim.set_pf_state(streams=_words(4))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "streams must be uint64 [3][4]"
    start = np.zeros((2, 10))
    start[:, [0, 1, 4]] = bench_start_poses(2, 1)
    nom, cloud = mp.fresh_nominal(2), (np.zeros(pf.cloud_shape(2)), np.full((2, 17), 1.0 / 17), np.zeros((2, 3)))
    poses, scans = start[:, [0, 1, 4]], np.ones((2, B))
    rows = {"mppi": lambda streams=_words(2), fresh=None, start=start: sim.mppi_rows(mp, start, nom, streams, fresh=fresh),
            "pf": lambda streams=_words(2), fresh=None: sim.localize_rows(pf, poses, scans, *cloud, streams=streams, fresh=fresh)}
    for who in FEATURES:
        with pytest.raises(ValueError) as e:
            rows[who](streams=_words(3))
        assert str(e.value) == "streams must be uint64 [2][4]"
        with pytest.raises(ValueError) as e:
            rows[who](fresh=[0, 1, 0])
        assert str(e.value) == "fresh must be [m]"
        w = _words(2)
        assert np.array_equal(rows[who](streams=w, fresh=[0, 1])["streams"].shape, (2, 4)) and np.array_equal(w, _words(2)), "the caller's streams were written"
    rol = amd.Rollout(k=3, horizon=2, channels=("alive",))
    for call in (lambda: rows["mppi"](start=np.zeros((2, 9))), lambda: sim.rollout_rows(rol, np.zeros((2, 9)), np.zeros((3, 2, 2)))):
        with pytest.raises(ValueError) as e:
            call()
        assert str(e.value) == "start must be [m][10] = state[7], FIFO newest, FIFO older, FIFO count"


# ---- the same streams for both features ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("agents, agent_base", [(None, 0), ([3, 4, 6], 0), (None, 5), ([3, 4, 6], 5)])
def test_both_features_give_an_agent_the_same_stream(amd, sim, agents, agent_base):
    from f1tenth_gym_amd.reset_sampler import stream_words
    seed = 20241
    sim.set_mppi(MPPI, agents=agents, seed=seed, agent_base=agent_base)
    sim.set_particle_filter(PF, agents=agents, seed=seed, agent_base=agent_base)
    planner, filt = sim.get_mppi_state()[1], sim.get_pf_state()[3]
    every = stream_words(seed, agent_base + N, 0)                        # agent n of a run that starts at agent 0
    expect = every[agent_base + np.arange(N)] if agents is None else np.stack([every[agent_base + n] for n in agents])
    assert planner.dtype == np.uint64 and planner.shape == expect.shape
    assert np.array_equal(planner, filt) and np.array_equal(planner, expect)
    assert np.array_equal(sim.mppi_agents, sim.pf_agents) and sim.mppi_agents.dtype == np.int32


# ---- both armed on one handle: one does not touch the other -----------------------------------------------------------------------------------
class Both(object):
    """a handle with the planner on [1, 2, 5] and the filter on [0, 5, 7], two device steps, a planner call and a filter call
    taken.  The steps read `d_fixed`, the planner writes `d_plan`: the cars move the same whatever is armed."""
    PLANNER, FILTER = [1, 2, 5], [0, 5, 7]

    def __init__(self, amd):
        s = self.s = _handle(amd)
        self.d_fixed, self.d_plan, self.d_pinfo = s.device_array((N, 2)), s.device_array((N, 2)), s.device_array((N, 4), np.float32)
        self.d_pose, self.d_finfo = s.device_array((N, 3)), s.device_array((N, 4), np.float32)
        self.d_fixed.upload(np.tile([0.05, 2.0], (N, 1)))
        self.arm_planner()
        self.arm_filter()
        for _ in range(2):
            self.step()
        self.plan()
        self.localize()

    def arm_planner(self, agents=PLANNER):
        self.s.set_mppi(MPPI, agents=agents, seed=3)

    def arm_filter(self, agents=FILTER):
        self.s.set_particle_filter(PF, agents=agents, seed=4)

    def step(self):
        self.s.step_device(self.d_fixed)
        assert self.s.step_groups()[2] == 2

    def plan(self):
        """the planner's next output: a step, then the call right behind it (on the blocks' streams)"""
        self.d_plan.upload(np.zeros((N, 2)))
        self.d_pinfo.upload(np.zeros((N, 4), dtype=np.float32))
        self.step()
        self.s.mppi_device(self.d_plan, self.d_pinfo)
        self.s.sync()
        return self.d_plan.download(), self.d_pinfo.download()

    def localize(self):
        self.d_pose.upload(np.zeros((N, 3)))
        self.d_finfo.upload(np.zeros((N, 4), dtype=np.float32))
        self.step()
        self.s.localize_device(self.d_pose, self.d_finfo)
        self.s.sync()
        return self.d_pose.download(), self.d_finfo.download()

    def close(self):
        for d in (self.d_fixed, self.d_plan, self.d_pinfo, self.d_pose, self.d_finfo):
            d.free()
        self.s.close()


def test_arming_one_feature_leaves_the_other_bit_for_bit(amd):
    gc.collect()
    a0 = amd.device_allocs()
    twin = Both(amd)
    a1 = amd.device_allocs()
    dist = Both(amd)
    a2 = amd.device_allocs()
    assert (a1[0] - a0[0], a1[1] - a0[1]) == (a2[0] - a1[0], a2[1] - a1[1])
    assert _same(twin.s.get_mppi_state(), dist.s.get_mppi_state()) and _same(twin.s.get_pf_state(), dist.s.get_pf_state())

    # the filter re-armed on another list, then disarmed: the planner's state and its next output are the twin's
    for disturb in (lambda: dist.arm_filter([2, 3]), dist.s.clear_particle_filter):
        disturb()
        assert _same(twin.s.get_mppi_state(), dist.s.get_mppi_state())
        got, want = dist.plan(), twin.plan()
        assert _same(got, want) and want[0][Both.PLANNER].any(axis=1).all() and not want[0][[0, 3, 4, 6, 7]].any()
        assert _same(twin.s.get_mppi_state(), dist.s.get_mppi_state())
    # the filter back as the twin's is (the twin's plan() calls stepped both handles alike, the twin's filter saw none of them)
    dist.arm_filter()
    dist.s.set_pf_state(*twin.s.get_pf_state())
    assert _same(twin.s.get_pf_state(), dist.s.get_pf_state())

    # the planner re-armed on another list, then disarmed: the filter's state and its next output are the twin's
    for disturb in (lambda: dist.arm_planner([0, 4, 6, 7]), dist.s.clear_mppi):
        disturb()
        assert _same(twin.s.get_pf_state(), dist.s.get_pf_state())
        got, want = dist.localize(), twin.localize()
        assert _same(got, want) and want[0][Both.FILTER].any(axis=1).all() and not want[0][[1, 2, 3, 4, 6]].any()
        assert _same(twin.s.get_pf_state(), dist.s.get_pf_state())
    dist.arm_planner()
    dist.s.set_mppi_state(*twin.s.get_mppi_state())
    assert _same(dist.plan(), twin.plan()) and _same(dist.localize(), twin.localize())

    assert amd.device_allocs() == a2, "re-arming to the same lists changed what the handle holds"
    dist.close()
    assert amd.device_allocs() == a1
    twin.close()
    assert amd.device_allocs() == a0
