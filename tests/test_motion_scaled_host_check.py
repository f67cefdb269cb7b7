"""vp9hip_motion_scaled_host at the extreme grids, sizes and vectors, under the sanitizer builds (CPU suite).

tests/c/motion_scaled_host_check.c is a stand-alone program (its own main, no device, no Python)
over csrc/host/vp9h_motion_scaled.c: grids of 2 x 2 and 4096 x 4096 cells, 16384 x 1 and
1 x 16384 to 3 x 2 with every cell -32768 (the largest sums), both sources with the accumulated
sums at the int32 ends, an 8 x 8 field worked by hand with negative quarters and an intra cell,
in exact-size heap arrays with guard bytes around the inputs and the output.
`make motion_scaled_host_check` builds it plain and with ASan + UBSan, without -fwrapv: a signed
overflow in the 64-bit sums is a finding.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "motion_scaled_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_motion_scaled_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "motion_scaled_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "motion_scaled_host_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
