"""vp9hip_acc_propagate_host at its edges, under the sanitizer builds (CPU suite).

tests/c/acc_propagate_host_check.c is a stand-alone program (its own main, no device, no Python)
over csrc/host/vp9h_prop.c: vectors of +-32767, -32768 and INT32_MAX / INT32_MIN, 16384-sample
grids at C = 1, 1 x 1 grids, every element size, both layouts and modes, fill and keep, exact-size
arrays, guard bytes around the destination and the valid map. `make acc_propagate_host_check`
builds it plain and with ASan + UBSan, without -fwrapv, so a signed overflow in the definition is
a finding.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "acc_propagate_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_acc_propagate_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "acc_propagate_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "acc_propagate_host_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
