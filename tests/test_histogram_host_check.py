"""vp9hip_frame_histograms_host at the extreme sizes and codes, under the sanitizer builds (CPU suite).

tests/c/hist_host_check.c is a stand-alone program (its own main, no device, no Python) over
csrc/host/vp9h_hist.c and csrc/host/vp9h_convert.c: 1x1, 16384x1, 1x16384 and 4096x4096 frames of
the constant codes 0, 2^bpp - 1 and 65535, in both modes, whose histograms have a closed form (one
bin a channel holds everything), in exact-size heap planes with a guarded output, and every
refusal. `make hist_host_check` builds it plain and with ASan + UBSan, without -fwrapv: a signed
overflow in the matrix is a finding.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "hist_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_hist_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "hist_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "hist_host_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
