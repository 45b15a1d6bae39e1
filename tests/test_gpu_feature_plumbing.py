"""The host plumbing the per-agent device features share: the check of a page-locked destination, its copy per env
block and on the main stream, what f110_host_free forgets, "every map slot in use has a track", and the unit forms' refusals of a
start row and of a map slot.  Every refusal is held to its code AND its full text; every copy to the bytes of the download.

One shape throughout: 4 envs of 2 agents, 16 beams, example_map registered as two slots (envs alternate), step_groups = 2, so a
step goes out as two env blocks and a call right behind it rides the blocks' streams."""
import ctypes as C

import numpy as np
import pytest

from _util import MAPS, bench_start_poses, load_map_image

pytestmark = pytest.mark.gpu

E, A, B = 4, 2, 16
N = E * A
CSV = MAPS + "/example_waypoints.csv"
FEATURES = ("obs", "preview", "neighbors", "rollout")
PINNED_TEXT = {"obs": "obs encode: h_pinned is not [N][F][D] floats of f110_host_alloc memory",
               "preview": "track preview: h_pinned is not [N][P][D] floats of f110_host_alloc memory",
               "neighbors": "neighbors: h_pinned is not [N][K][D] floats of f110_host_alloc memory",
               "rollout": "rollout: h_pinned is not [N][K][D] floats of f110_host_alloc memory"}


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _handle(amd, tracks=(0, 1)):
    """the shape of this file; `tracks`: the slots that get the raceline.  Reset, tracking on, envs alternating between the slots"""
    s = amd.BatchSim(num_envs=E, num_agents=A, num_beams=B, step_groups=2)
    s.set_map_image(*load_map_image("example_map"))
    s.reset(bench_start_poses(E, A))
    assert s.add_map_image(*load_map_image("example_map")) == 1
    for slot in tracks:
        s.set_track(CSV, slot)
    s.enable_track()
    s.set_env_maps(np.arange(E) % 2)
    return s


class Calls(object):
    """the four device forms on one handle, each with its spec, its output and the raw entry point (h_pinned as an address)"""

    def __init__(self, amd, s):
        from f1tenth_gym_amd import _ffi
        self.s, self.L, self.ffi = s, _ffi.lib(), _ffi
        self.enc = amd.ObsEncoder(sectors=4, pool="min", features=("vx", "steer"), frames=2)
        self.prv = amd.TrackPreview(points=3, channels=("x", "y"))
        self.nbr = amd.Neighbors(k=1, channels=("dx", "dy", "gap_s"))
        self.rol = amd.Rollout(k=3, horizon=2, repeat=2, channels=("end_x", "alive", "progress"))
        self.shape = {"obs": self.enc.shape(N), "preview": self.prv.shape(N), "neighbors": self.nbr.shape(N), "rollout": self.rol.shape(N)}
        self.out = {k: s.device_array(v, np.float32) for k, v in self.shape.items()}
        self.d_cand = s.device_array(self.rol.actions_shape(N))
        self.d_cand.upload(np.tile([0.05, 2.0], (3, 2, 1)))
        self.d_act = s.device_array((N, 2))
        self.d_act.upload(np.tile([0.05, 2.0], (N, 1)))

    def api(self, what, pinned=None):
        s = self.s
        if what == "obs":
            return s.encode_obs_device(self.enc, self.out[what], pinned=pinned)
        if what == "preview":
            return s.track_preview_device(self.prv, self.out[what], pinned=pinned)
        if what == "neighbors":
            return s.neighbors_device(self.nbr, self.out[what], pinned=pinned)
        return s.rollout_device(self.rol, self.d_cand, self.out[what], pinned=pinned)

    def raw(self, what, address):
        h, L, o = self.s._h, self.L, self.out[what].ptr
        if what == "obs":
            sp = self.enc.spec(False)
            return L.f110_obs_encode_device(h, C.byref(sp), o, address)
        if what == "preview":
            sp = self.prv.spec()
            return L.f110_track_preview_device(h, C.byref(sp), o, address)
        if what == "neighbors":
            sp = self.nbr.spec()
            return L.f110_neighbors_device(h, C.byref(sp), o, address)
        sp = self.rol.spec()
        return L.f110_rollout_device(h, C.byref(sp), self.d_cand.ptr, o, None, address)

    def floats(self, what):
        return int(np.prod(self.shape[what]))

    def host_alloc(self, nbytes):
        p = C.c_void_p()
        assert self.L.f110_host_alloc(self.s._h, nbytes, C.byref(p)) == self.ffi.OK
        return p.value

    def two_block_step(self):
        self.s.step_device(self.d_act)
        assert self.s.step_groups()[2] == 2, "the step went out as %d block(s)" % self.s.step_groups()[2]


@pytest.fixture(scope="module")
def full(amd):
    s = _handle(amd)
    c = Calls(amd, s)
    yield c
    s.close()


@pytest.mark.parametrize("what", FEATURES)
def test_pinned_destination_must_be_a_whole_block_of_the_library(full, what):
    c, ffi = full, full.ffi
    c.two_block_step()
    heap = np.zeros(c.shape[what], dtype=np.float32)
    assert c.raw(what, heap.ctypes.data) == ffi.ERR_INVALID and ffi.last_error(c.s._h) == PINNED_TEXT[what]
    with pytest.raises(ValueError) as e:
        c.api(what, pinned=heap)
    assert str(e.value) == PINNED_TEXT[what]
    short = c.host_alloc(4 * c.floats(what) - 4)                       # one float too short
    assert c.raw(what, short) == ffi.ERR_INVALID and ffi.last_error(c.s._h) == PINNED_TEXT[what]
    assert c.raw(what, short + 4) == ffi.ERR_INVALID                   # ... and a whole block's worth that starts inside it
    assert c.L.f110_host_free(c.s._h, short) == ffi.OK
    exact = c.host_alloc(4 * c.floats(what))
    assert c.raw(what, exact) == ffi.OK
    assert c.L.f110_host_free(c.s._h, exact) == ffi.OK


@pytest.mark.parametrize("what", FEATURES)
def test_pinned_copy_is_the_download_per_block_and_on_the_main_stream(full, what):
    c, s = full, full.s
    pin = s.pinned_empty(c.shape[what], np.float32)
    # right behind a two-block step: the call rides the blocks, one copy per block on the block's stream
    pin[...] = -7.0
    s.step_device(c.d_act)
    c.two_block_step()
    c.api(what, pinned=pin)
    s.sync()
    got = c.out[what].download()
    assert np.array_equal(_bits(np.array(pin)), _bits(got)) and not np.any(got == -7.0), "%s: the per-block copies" % what
    # after an intervening call (sync() went through the handle): the whole batch on the main stream
    pin[...] = -7.0
    c.two_block_step()
    s.sync()
    c.api(what, pinned=pin)
    s.sync()
    again = c.out[what].download()
    assert np.array_equal(_bits(np.array(pin)), _bits(again)) and not np.any(again == -7.0), "%s: the main-stream copy" % what
    assert not np.array_equal(_bits(again), _bits(got)), "%s: the second step changed nothing" % what


@pytest.mark.parametrize("what", FEATURES)
def test_freeing_the_pinned_block_behind_a_call_and_stepping_on(full, what):
    c, s, ffi = full, full.s, full.ffi
    for owner in (s._h, None):                                        # freed through the handle, and as a finalizer frees it
        block = c.host_alloc(4 * c.floats(what))
        c.two_block_step()
        assert c.raw(what, block) == ffi.OK
        assert c.L.f110_host_free(owner, block) == ffi.OK
        c.two_block_step()
        assert c.raw(what, None) == ffi.OK
        s.sync()
        assert np.all(np.isfinite(c.out[what].download())), what
    assert np.all(np.isfinite(s.get("state")["state"]))


def test_a_slot_in_use_without_a_track(amd):
    from f1tenth_gym_amd import _ffi
    s = _handle(amd, tracks=(0,))
    c = Calls(amd, s)
    h, L = s._h, c.L
    assert c.raw("neighbors", None) == _ffi.ERR_STATE
    assert _ffi.last_error(h) == "neighbors: GAP_S is requested, but map slot 1 has no track (f110_track_set)"
    assert c.raw("rollout", None) == _ffi.ERR_STATE
    assert _ffi.last_error(h) == "rollout: PROGRESS or END_LAT is requested, but map slot 1 has no track (f110_track_set)"
    planner = amd.Mppi(k=4, horizon=2, repeat=2, w_progress=4.0)
    d_act = s.device_array((N, 2))
    d_act.upload(np.zeros((N, 2)))
    s.set_mppi(planner, agents=[0, 3, 4], seed=1)                      # agent 3 is in env 1, which is on slot 1
    assert L.f110_mppi_device(h, d_act.ptr, None) == _ffi.ERR_STATE
    assert _ffi.last_error(h) == "mppi: w_progress or w_lat is set, but map slot 1 has no track (f110_track_set)"
    s.sync()
    assert not d_act.download().any(), "a refused call wrote the actions"
    s.set_mppi(planner, agents=[0, 1, 4], seed=1)                      # envs 0 and 2 only: both on slot 0
    assert L.f110_mppi_device(h, d_act.ptr, None) == _ffi.OK, _ffi.last_error(h)
    s.sync()
    act = d_act.download()
    assert act[[0, 1, 4]].any(axis=1).all() and not act[[2, 3, 5, 6, 7]].any()
    # without the track channels nothing asks for a track
    nbr, rol = amd.Neighbors(k=1, channels=("dx", "dy")), amd.Rollout(k=3, horizon=2, channels=("alive",))
    s.neighbors_device(nbr).free()
    s.rollout_device(rol, c.d_cand).free()
    s.close()


def test_unit_forms_refuse_a_fifo_count_and_a_slot_past_the_end(full, amd):
    c, s = full, full.s
    rows = np.zeros((3, 10))
    rows[:, [0, 1, 4]] = bench_start_poses(3, 1)
    rol = amd.Rollout(k=3, horizon=2, channels=("alive",))
    cand = np.tile([0.0, 2.0], (3, 2, 1))
    planner = amd.Mppi(k=4, horizon=2, repeat=2, w_progress=0.0)
    nom, words = planner.fresh_nominal(3), np.arange(1, 13, dtype=np.uint64).reshape(3, 4)
    bad = rows.copy()
    bad[1, 9] = 3.0
    with pytest.raises(ValueError) as e:
        s.rollout_rows(rol, bad, cand)
    assert str(e.value) == "rollout: row 1 has a FIFO fill count of 3, not 0, 1 or 2"
    with pytest.raises(ValueError) as e:
        s.mppi_rows(planner, bad, nom, words)
    assert str(e.value) == "mppi: row 1 has a FIFO fill count of 3, not 0, 1 or 2"
    with pytest.raises(ValueError) as e:
        s.rollout_rows(rol, rows, cand, slot=2)
    assert str(e.value) == "rollout: map slot 2, but 2 maps are registered"
    with pytest.raises(ValueError) as e:
        s.mppi_rows(planner, rows, nom, words, slot=2)
    assert str(e.value) == "mppi: map slot 2, but 2 maps are registered"
    # a refused unit call leaves the handle as it was: the good rows go through, on either slot, and the next step is two blocks
    for slot in (0, 1):
        assert s.rollout_rows(rol, rows, cand, slot=slot).shape == rol.shape(3)
        assert s.mppi_rows(planner, rows, nom, words, slot=slot)["actions"].shape == (3, 2)
    c.two_block_step()
