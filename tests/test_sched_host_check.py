"""The launch-list policy of csrc/vp9hip_sched.h under the sanitizer build (CPU suite).

tests/c/sched_host_check.cpp is a stand-alone program (its own main, no device, no Python) over
the fused-phase launch schedule and the k_lfr task table that the host planner, the static plan
and the device plan share: it sweeps small inputs (intra steps, LF diagonals, residual segments,
empty steps, k_lfr on and off; frames of 1..5 SB rows by 1..4 columns, j0 0..6) and checks
properties, parsing each table back the way the kernels read it. `make sched_host_check` builds
it plain and with ASan + UBSan; it is run directly.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "sched_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_sched_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "sched_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "sched_host_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
