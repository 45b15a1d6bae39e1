"""The seeded fuzzers of the two newest features, in bounded seed chunks (as tests/test_gpu_round5.py runs the older ones):
tools/debug/fuzz_track.py (track progress against the oracle's nearest_on_trajectory on every step path, with the pruning seed made
stale between steps) and tools/debug/fuzz_snapshot.py (restores and clones replayed bit for bit; ShardedVecEnv against one
F110VecEnv under partial resets).  The nested experimental-build run (F110_NESTED_SUITE) takes a few seeds of every chunk."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu

NESTED = bool(os.environ.get("F110_NESTED_SUITE"))   # the lab build's re-run of the suite runs a few seeds of every chunk
TRACK_SEEDS, TRACK_CHUNK = 400, 100   # ~0.06 s per seed on one MI355X: ~25 s
SNAP_SEEDS, SNAP_CHUNK = 300, 100     # ~0.13 s per seed: ~40 s
ENV_SEEDS, ENV_CHUNK = 300, 100       # ~0.14 s per seed: ~40 s


@pytest.fixture(scope="module")
def amd():
    import f1tenth_gym_amd
    from f1tenth_gym_amd import _ffi
    assert _ffi.device_count() >= 1, "no MI355X visible: the HIP path cannot run (no CPU fallback)"
    return f1tenth_gym_amd


def _fuzzer(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "debug", name + ".py"))
    fz = importlib.util.module_from_spec(spec); spec.loader.exec_module(fz)
    return fz


@pytest.mark.parametrize("first", range(0, TRACK_SEEDS, TRACK_CHUNK))
def test_fuzz_track_bounded_seeds(amd, first):
    """tools/debug/fuzz_track.py, seeds 0 .. 399 in the driver-run suite (1 200 by hand without a mismatch): track progress on 1..3 slots
    with tracks of 3 .. 5000 segments on both sides of the LDS limit, random env_maps, every step entry point, stale pruning seeds
    after teleports, resets, re-seats, loads, clones and track swaps — bit-exact to the oracle, winners checked in extended
    precision; 1 200 seeds took 73 s (0.06 s per seed) on one MI355X"""
    fz = _fuzzer("fuzz_track")
    bad = [sd for sd in range(first, first + (2 if NESTED else TRACK_CHUNK)) if not fz.run(sd)]
    assert not bad, bad


@pytest.mark.parametrize("first", range(0, SNAP_SEEDS, SNAP_CHUNK))
def test_fuzz_snapshot_bounded_seeds(amd, first):
    """tools/debug/fuzz_snapshot.py run(), seeds 0 .. 299 in the driver-run suite (1 000 by hand without a mismatch): save / restore into the
    same handle, a fresh one with another row cache and other env indices of another env count, clones — all bit for bit over random
    noise modes, map slots, per-agent parameters, integrators, tracking and episode logic; the restored run against the oracle
    (shared-stream noise seeds: 651 of the 1 000); 1 000 seeds took 126 s (0.13 s per seed) on one MI355X"""
    fz = _fuzzer("fuzz_snapshot")
    bad = [sd for sd in range(first, first + (2 if NESTED else SNAP_CHUNK)) if not fz.run(sd)]
    assert not bad, bad


@pytest.mark.parametrize("first", range(0, ENV_SEEDS, ENV_CHUNK))
def test_fuzz_sharded_env_bounded_seeds(amd, first):
    """tools/debug/fuzz_snapshot.py run_env(), seeds 0 .. 299 in the driver-run suite (1 000 by hand without a mismatch): ShardedVecEnv of
    1..5 shards against one F110VecEnv, partial masks (one per seed covering exactly one shard), snapshot / restore, both
    device_logic values, tracking with reward='progress' — every returned array bit-equal; 1 000 seeds took 135 s (0.14 s per seed) on one MI355X"""
    fz = _fuzzer("fuzz_snapshot")
    bad = [sd for sd in range(first, first + (2 if NESTED else ENV_CHUNK)) if not fz.run_env(sd)]
    assert not bad, bad
