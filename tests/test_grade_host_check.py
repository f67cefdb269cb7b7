"""vp9hip_grade_host, the C statement of the graded output, under the sanitizer builds (CPU suite).

tests/c/grade_host_check.c is a stand-alone program (its own main, no device, no Python) over
csrc/host/vp9h_grade.c: the table-free identity of include/vp9hip.h "Graded output" at 8, 10 and
12 bits over every code, both clips of the matrix stage, P = 65535 (which reads entry 4096), and
the refusal of an entry above out_max and of |m| > 2^16, with exact-size heap tables. `make
grade_host_check` builds it plain and with ASan + UBSan, without -fwrapv: a signed overflow in the
64-bit sum is a finding.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "grade_host_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_grade_host_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "grade_host_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "grade_host_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
