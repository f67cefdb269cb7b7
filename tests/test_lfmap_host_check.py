"""lf_sb's chunk map (csrc/vp9hip_lfmap.h) on the CPU, plain and under ASan + UBSan.

tests/c/lfmap_host_check.cpp is a stand-alone program (its own main, no device, no Python) that
includes the header the kernels include. For 4:2:0, 4:2:2, 4:4:0 and 4:4:4 at 8- and 16-bit pixels
it walks every (lane, u) of the workgroup and checks that the map enumerates every (plane, row,
chunk) of the loop filter's tile exactly once, stays inside the LDS tile without overlap, and
equals the former decode by division slot for slot. `make lfmap_host_check` builds both forms;
they are run directly.
"""
import fcntl
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "c", "build")


@pytest.fixture(scope="module")
def bins():
    os.makedirs(BUILD, exist_ok=True)
    with open(os.path.join(BUILD, ".make.lock"), "w") as lk:     # one make at a time (tests/test_sanitize.py)
        fcntl.flock(lk, fcntl.LOCK_EX)
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "lfmap_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_lfmap_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "lfmap_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "lfmap_host_check OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    assert r.stdout.count(" chunks\n") == 8, r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
