"""vp9hip_residual_host and the residual kernel's record guards on packets that break their own
counts, under the sanitizer build (CPU suite).

tests/c/residual_host_check.cpp is a stand-alone program (its own main, no device, no Python)
over csrc/vp9hip_residual_host.cpp and the guard helper of csrc/vp9hip_residual.h that k_residual
applies to every tx record: out-of-range blocks, eob counts and coefficient totals that disagree,
eob > N * N, into exact-size heap planes and into guarded ones. `make residual_host_check` builds
it plain and with ASan + UBSan; it is run directly. No GPU test feeds the kernel an invalid packet.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "residual_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_residual_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "residual_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "residual_host_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
