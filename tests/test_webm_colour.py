"""vp9h_webm_read_colour, the WebM Colour element of the VP9 track, under the sanitizer builds (CPU suite).

tests/c/webm_colour_check.c is a stand-alone program (its own main, no device, no Python) linked
against the parser, csrc/host/vp9h_webm.c. It writes its files element by element into exact-size
heap blocks: a Colour element with every field (4- and 8-byte floats), a track without one, an
empty one, a partial one, the file cut at every byte length (an error or the complete answer,
never a read past the cut), and sizes that run past their parent. `make webm_colour_check` builds
it plain and with ASan + UBSan.
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
        r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "ffmpeg-hybrid_amd", "csrc"), "webm_colour_check"],
                           capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return BUILD


@pytest.mark.parametrize("variant", ("plain", "asan"))
def test_webm_colour_check(bins, variant):
    r = subprocess.run([os.path.join(bins, "webm_colour_check_" + variant)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "webm_colour_check OK" in r.stdout, (r.stdout[-300:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
