"""CPU checks of the device-memory owners ("Who owns device memory"): DevBuf and DevArena of csrc/f110_devmem.hpp over the
header's host seam, as a stand-alone program under the sanitizers; the counter's symbol in the header and the binding; and the
handle's source holding no free of its own.  The GPU test (tests/test_gpu_device_memory.py) holds every feature's memory to the counter."""
import os
import re
import shutil
import subprocess

import pytest

from f1tenth_gym_amd import _ffi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.isfile("/opt/rocm/bin/hipcc"),
                                 reason="hipcc needed to build the host harness")


def hipcc():
    return shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@needs_hipcc
def test_owner_program_is_clean_under_the_sanitizers(tmp_path):
    """the stand-alone program (its own main) under the address and undefined-behaviour sanitizers: host code only"""
    src = os.path.join(HERE, "host_harness", "devmem_harness.cpp")
    exe = str(tmp_path / "devmem_harness_san")
    subprocess.check_call([hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-DF110_DEVMEM_HOST",
                           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", src, "-o", exe],
                          stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    proc = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert proc.returncode == 0 and proc.stdout == "devmem harness: ok\n", proc.stdout


def test_the_counter_is_in_the_header_and_the_binding():
    with open(os.path.join(ROOT, "include", "f110.h")) as f:
        src = f.read()
    assert re.search(r"\bint f110_device_allocs\(int64_t \*live, int64_t \*bytes\);", src)
    assert "f110_device_allocs" in _ffi.PROTOTYPES
    assert re.search(r"#define F110_ABI_VERSION 1\b", src)


def test_the_handle_frees_through_its_owners_only():
    """f110_hip.hip calls hipFree / hipMalloc for the caller's own memory alone (f110_device_alloc / _free); f110_destroy lists no pointers"""
    with open(os.path.join(ROOT, "f1tenth_gym_amd", "csrc", "f110_hip.hip")) as f:
        src = f.read()
    code = re.sub(r"//[^\n]*", "", src)
    assert len(re.findall(r"\bhipFree\(", code)) == 1 and len(re.findall(r"\bhipMalloc\(", code)) == 1
    assert re.search(r"int f110_device_free\(.*?\n\{.*?hipFree\(.*?\n\}", code, flags=re.S)
    destroy = re.search(r"\nvoid f110_destroy\(f110_sim \*h\)\n\{(.*?)\n\}\n", code, flags=re.S).group(1)
    assert "delete h;" in destroy and "[]" not in destroy and "hipFree" not in destroy
