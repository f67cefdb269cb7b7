"""vp9hip_bicubic_weights' 64-bit arithmetic at the extreme sizes, under the sanitizer builds (CPU
suite).

tests/c/bicubic_weights_check.c is a stand-alone program (its own main, no device, no Python)
over csrc/host/vp9h_convert.c: it sweeps the weights where c 2^Q nears 2^61 (T = 2^15) and
compares each with a 128-bit evaluation of the same formulas, into exact-size heap arrays.
`make sanitize` builds it plain and with ASan + UBSan beside the other host binaries (without
-fwrapv, so a signed overflow that the width argument of include/vp9hip.h missed is reported).
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "bicubic_weights_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_bicubic_weights_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "bicubic_weights_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "bicubic_weights_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
