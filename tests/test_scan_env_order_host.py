"""CPU check of the agent-aligned scan's task order (f110_math.hpp, scan_task_agent; tests/host_harness/scan_order_harness.hip is
its host instantiation): a bijection from task ids onto (agent, sector) that keeps the tasks of one (env, sector) together and
is the agent-major order at one agent per env.  The GPU tests (tests/test_gpu_scan_env_order.py) hold the kernel that walks
the tasks in this order to the one-task-per-wave run bit for bit."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
_up = C.POINTER(C.c_uint32)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    src = os.path.join(HERE, "host_harness", "scan_order_harness.hip")
    lib = str(tmp_path_factory.mktemp("scan_order_harness") / "libscan_order_harness.so")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", src, "-o", lib],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return C.CDLL(lib)


def task_map(hh, E, A, tpa):
    n = E * A * tpa
    agent, sector = np.full(n, 0xffffffff, dtype=np.uint32), np.full(n, 0xffffffff, dtype=np.uint32)
    hh.hh_scan_task_agent(C.c_uint32(n), C.c_uint32(tpa), C.c_uint32(A), agent.ctypes.data_as(_up), sector.ctypes.data_as(_up))
    return agent.astype(np.int64), sector.astype(np.int64)


@needs_hipcc
@pytest.mark.parametrize("E", [1, 5])
@pytest.mark.parametrize("tpa", [1, 2, 17])
@pytest.mark.parametrize("A", [1, 2, 3, 4])
def test_task_order(hh, A, tpa, E):
    n = E * A * tpa
    agent, sector = task_map(hh, E, A, tpa)
    # onto [0, E * A) x [0, tpa), every pair once
    assert agent.min() >= 0 and agent.max() < E * A and sector.min() >= 0 and sector.max() < tpa
    assert len(set(zip(agent.tolist(), sector.tolist()))) == n
    # the formula of the launch: env = task / (tpa * A), sector = (task % (tpa * A)) / A, agent in env = task % A
    task = np.arange(n)
    assert np.array_equal(agent, task // (tpa * A) * A + task % A) and np.array_equal(sector, task % (tpa * A) // A)
    # the tasks of one (env, sector) are consecutive, in agent order, and start at a multiple of A (an even grouping never splits a pair)
    env = agent // A
    for t0 in range(0, n, A):
        assert (env[t0:t0 + A] == env[t0]).all() and (sector[t0:t0 + A] == sector[t0]).all()
        assert np.array_equal(agent[t0:t0 + A] - env[t0] * A, np.arange(A))
    # env blocks are env-aligned: an env's tasks are one contiguous range of tpa * A ids
    assert np.array_equal(env, task // (tpa * A))
    if A == 1:   # the agent-major order the kernel walked before
        assert np.array_equal(agent, task // tpa) and np.array_equal(sector, task % tpa)


@needs_hipcc
def test_reciprocal_division_at_its_limit(hh):
    """rem / A through umulhi(rem, floor(2^32 / A) + 1) is exact while tpa * A * A <= 2^32: the largest launch shapes the host accepts
    (it walks agent-major beyond them), odd and even A, powers of two"""
    hh.hh_scan_task_inv_errors.restype = C.c_uint32
    for A in (2, 3, 4, 5, 7, 16, 255, 256, 1000, 4096, 65535, 65536):
        tpa = (1 << 32) // (A * A)
        assert tpa >= 1 and hh.hh_scan_task_inv_errors(C.c_uint32(tpa), C.c_uint32(A)) == 0, A
        assert hh.hh_scan_task_inv_errors(C.c_uint32(min(tpa, 17)), C.c_uint32(A)) == 0, A
    assert hh.hh_scan_task_inv_errors(C.c_uint32(2), C.c_uint32(65536)) == 0xffffffff   # refused: tpa * A * A > 2^32
