"""march_padded's loop after its control skeleton was rewritten (the give-up decision carried as a per-lane range limit, the
boundary case decided by one compare and entered wave by wave): the HOST instantiation of the same body, through
tests/host_harness, against the oracle on the inputs that take its rare paths, and as a stand-alone program under the host
sanitizers.  The -m gpu twin is tests/test_gpu_march_chain.py."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import orc
from _util import oracle_map_dt
from test_host_math import hh, _hh_scan, _padded_stats  # noqa: F401  (fixture: builds / loads the host harness)

HERE = os.path.dirname(os.path.abspath(__file__))
B, FOV = 1080, 4.7

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                reason="hipcc needed to build the host harness")


def rotated_sub_map():
    """a 400 x 400 window of example_map's table behind a rotated, shifted origin (and another resolution)"""
    dt, res, _ = oracle_map_dt("example_map")
    res2 = 0.0625
    return np.ascontiguousarray(dt[600:1000, 900:1300]) * (res2 / res), res2, [1.0, 2.0, -1.1]


def maps():
    for name in ("berlin", "example_map", "skirk"):
        yield (name,) + tuple(oracle_map_dt(name))
    yield ("rotated_sub",) + rotated_sub_map()


def to_world(origin, u, v):
    """map-frame metres (u along columns, v along rows) -> world"""
    c, s = np.cos(origin[2]), np.sin(origin[2])
    return origin[0] + c * u - s * v, origin[1] + s * u + c * v


def boundary_poses(dt, res, origin, rng, cells=6):
    """the families of test_padded_layout_guard_band_and_far_poses, for any origin yaw: lidar on a cell corner / edge with
    headings along the map's axes, a beam running along y = const, and lidars on, just off and far off the map"""
    H, W = dt.shape
    free = np.argwhere(dt > 0.3)
    yaw = origin[2]
    poses = []
    for r, c in free[rng.choice(len(free), cells, replace=False)]:
        poses.append(list(to_world(origin, c * res, r * res)) + [yaw + rng.choice([0.0, np.pi / 2, np.pi, -np.pi / 2])])
        poses.append(list(to_world(origin, c * res, (r + 0.5) * res)) + [yaw + 0.0])
        # beam 0 takes table direction 0 = (1, 0) exactly (yaw 0): it runs along the cell boundary y = const
        poses.append(list(to_world(origin, (c + 0.25) * res, r * res)) + [FOV / 2 + 1e-5])
        poses.append(list(to_world(origin, (c + rng.uniform()) * res, (r + rng.uniform()) * res)) + [rng.uniform(-7, 7)])
    poses += [list(to_world(origin, 0.0, 0.0)) + [0.3], list(to_world(origin, -1.0, H * res / 2)) + [0.0],
              list(to_world(origin, W * res + 2.5, H * res + 2.5)) + [3.9], list(to_world(origin, -40.0, -40.0)) + [0.8],
              list(to_world(origin, W * res / 2, H * res + 29.0)) + [-1.6], [1e9, -1e9, 1.0], [1e300, 0.0, 0.0]]
    return poses


def random_poses(dt, res, origin, rng, n):
    """half on free cells, half anywhere on the map's box and a little around it"""
    H, W = dt.shape
    free = np.argwhere(dt > 0.1)
    poses = []
    for r, c in free[rng.choice(len(free), n // 2, replace=False)]:
        poses.append(list(to_world(origin, (c + rng.uniform()) * res, (r + rng.uniform()) * res)) + [rng.uniform(-7, 7)])
    for _ in range(n - n // 2):
        poses.append(list(to_world(origin, rng.uniform(-1.0, W * res + 1.0), rng.uniform(-1.0, H * res + 1.0))) + [rng.uniform(-7, 7)])
    return poses


def test_march_equals_oracle_on_random_and_boundary_poses(hh):
    """ranges, hit cells, direction indices and lookup counts array_equal to the oracle on four maps: 200 random poses each and
    the boundary families — and the inputs do take the rare paths: at least 18 guard-band re-marches, at least 3*2*1080 rays
    of lidars the border does not cover (what the existing guard-band test reaches on these families)"""
    so = orc.ScanOracle(B, FOV)
    rng = np.random.default_rng(2026)
    _padded_stats(hh)
    total = dict(fast=0, guard=0, far=0)
    for name, dt, res, origin in maps():
        so.set_map_dt(dt, res, origin)
        poses = boundary_poses(dt, res, origin, rng) + random_poses(dt, res, origin, rng, 200)
        for pose in poses:
            ref, ref_hits = so.scan(pose, want_hits=True)
            ranges, hits, idx, lk = _hh_scan(hh, 3, so.dt, res, origin, so.sines, so.cosines, B, FOV, pose)
            assert np.array_equal(idx, so.beam_dir_indices(pose[2])), (name, pose)
            assert np.array_equal(hits, ref_hits), (name, pose)
            assert np.array_equal(ranges, ref), (name, pose)
            assert lk == so.last_lookups, (name, pose)
        st = _padded_stats(hh)
        assert st["fast"] + st["guard"] + st["far"] == len(poses) * B, (name, st)
        assert st["fast"] > 150 * B and st["far"] >= 2 * B, (name, st)      # every map: mostly the fast march, and the two absurd lidars at least
        for key in total:
            total[key] += st[key]
    assert 18 <= total["guard"] < 1e-3 * total["fast"] and total["far"] >= 3 * 2 * B, total


def test_march_standalone_under_host_sanitizers(tmp_path):
    """the same pose families marched by a stand-alone program (its own main) over an exactly-sized heap copy of the padded
    table, built for the HOST with the address and undefined-behaviour sanitizers; the program checks every offset the loop
    forms against the table's size itself (F110_MARCH_OFFSET_HOOK).  Run as a program; nothing is loaded into Python."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(HERE, "host_harness", "march_chain_main.hip")
    exe = str(tmp_path / "march_chain_san")
    built = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                            "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert built.returncode == 0, built.stdout[-3000:]
    rng = np.random.default_rng(7)
    guard = far = 0
    for name, dt, res, origin in maps():
        poses = np.asarray(boundary_poses(dt, res, origin, rng) + random_poses(dt, res, origin, rng, 40))
        tpath, ppath = str(tmp_path / (name + ".f64")), str(tmp_path / (name + "_poses.f64"))
        np.ascontiguousarray(dt, dtype=np.float64).tofile(tpath)
        poses.tofile(ppath)
        proc = subprocess.run([exe, tpath, str(dt.shape[0]), str(dt.shape[1]), repr(float(res)), repr(float(origin[0])), repr(float(origin[1])),
                               repr(float(origin[2])), ppath, str(len(poses)), str(B), repr(FOV)],
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        m = re.match(r"ok: (\d+) rays, fast (\d+) guard (\d+) far (\d+), lookups (\d+), offsets checked (\d+)", proc.stdout)
        assert proc.returncode == 0 and m, proc.stdout[-2000:]
        rays, fast, g, f, lookups, checked = (int(m.group(i)) for i in (1, 2, 3, 4, 5, 6))
        assert rays == len(poses) * B and fast > 40 * B, proc.stdout
        assert checked >= lookups - fast > 0, proc.stdout      # every load of every ray that was marched went through the check
        guard += g
        far += f
    assert guard >= 18 and far >= 3 * 2 * B, (guard, far)     # the program, too, is taken through the rare paths (the bar of the test above)
