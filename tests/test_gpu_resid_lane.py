"""GPU parity of the lane-per-block 4x4 residual path, sample-exact vs the oracle.

k_resid / k_resid_dev / k_resid_multi transform a 4x4 block (tx code 0: DCT/ADST, tx code 4:
lossless WHT) in one lane: 64 jobs per wave, the block's 16 coefficients by wide loads
whatever its eob is, intra residuals as two 16-byte stores, inter ones added in place one
4-pixel word per row. The cases:

  a  72x72 keyframes, default density and coef_stress at q_idx 255, at 8, 10 and 12 bits:
     many 4x4 blocks of every txtp, DC-only blocks, a job count that is no multiple of 64
  b  72x72 lossless at 8 and 10 bits, 4:2:0 and 4:4:4: the WHT path
  c  8x8 and 16x16 frames in batches of one: the coefficient arena is a few blocks, every
     wide load runs near or past its end (the pad behind the arena)
  d  136x72 key + 2 P with compound prediction at 8 and 10 bits: in-place 4x4 residuals
     through k_resid_multi, word-wide prediction loads and stores at the right and bottom
     partial SBs
  e  a keyframe case and the GOP again with the host planner (VP9HIP_HOST_PLAN=1): k_resid
     with a host job count instead of k_resid_dev's range
  f  the sparse setting (p_skip 0.7, p_zero_eob 0.9): skipped blocks, short job ranges
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

SPARSE = {"p_skip": 0.7, "p_zero_eob": 0.9}
LOSSLESS = {"lossless": 1, "q_idx": 0}
STRESS = {"coef_stress": 1, "q_idx": 255}


def _cmp(v9, got, ref, w, h, what, ssh=1, ssv=1):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


def _keyframes(v9, orc, dev, w, h, bpp, what, n=2, seed=0x8a00, ssh=1, ssv=1, **kw):
    """n keyframes as one batch (device planner unless dev was opened under the host one)."""
    frames = [v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + i, ss_h=ssh, ss_v=ssv, **kw)) for i in range(n)]
    dev.configure(w, h, bpp, nbufs=n, ss_h=ssh, ss_v=ssv)
    dev.stage_batch(frames, list(range(n)))
    dev.run_batch()
    dev.sync()
    for i, f in enumerate(frames):
        ref = v9.alloc_planes(w, h, bpp, ssh, ssv)
        orc.decode_frame(f.pkt, ref)
        _cmp(v9, dev.download(i), ref, w, h, "%s frame %d" % (what, i), ssh, ssv)


def _gop(v9, orc, dev, w, h, bpp, what, n=3, seed=0x8d00, **kw):
    """Key + (n - 1) P frames, each on the frame before it, as one batch."""
    refs = bench.gop_refs(n, n)
    frames = [v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + i, inter=int(refs[i] is not None), **kw))
              for i in range(n)]
    dev.configure(w, h, bpp, nbufs=n)
    dev.stage_batch(frames, list(range(n)), refs)
    dev.run_batch()
    dev.sync()
    dec = []
    for i, f in enumerate(frames):
        out = v9.alloc_planes(w, h, bpp)
        r = refs[i]
        orc.decode_frame(f.pkt, out, None if r is None else [dec[r[0]], dec[r[1]], dec[r[2]]])
        dec.append(out)
        _cmp(v9, dev.download(i), out, w, h, "%s frame %d" % (what, i))


@pytest.mark.parametrize("bpp", [8, 10, 12])
@pytest.mark.parametrize("kw", [{}, STRESS], ids=["default", "stress"])
def test_keyframes(v9, orc, gpu, bpp, kw):
    """Case a."""
    _keyframes(v9, orc, gpu, 72, 72, bpp, "72x72 %d-bit %s" % (bpp, "stress" if kw else "default"), seed=0x8a00 + bpp, **kw)


@pytest.mark.parametrize("bpp", [8, 10])
@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_lossless(v9, orc, gpu, bpp, ss):
    """Case b."""
    _keyframes(v9, orc, gpu, 72, 72, bpp, "72x72 %d-bit lossless ss=%d" % (bpp, ss), seed=0x8b00 + bpp, ssh=ss, ssv=ss,
               **LOSSLESS)


@pytest.mark.parametrize("bpp", [8, 10])
@pytest.mark.parametrize("size", [8, 16])
@pytest.mark.parametrize("kw", [{}, STRESS, LOSSLESS], ids=["default", "stress", "lossless"])
def test_tiny_arena(v9, orc, gpu, size, bpp, kw):
    """Case c."""
    for seed in range(3):
        _keyframes(v9, orc, gpu, size, size, bpp, "%dx%d %d-bit seed %d" % (size, size, bpp, seed), n=1,
                   seed=0x8c00 + 16 * seed + bpp, **kw)


@pytest.mark.parametrize("bpp", [8, 10])
def test_gop_in_place(v9, orc, gpu, bpp):
    """Case d."""
    _gop(v9, orc, gpu, 136, 72, bpp, "136x72 %d-bit compound GOP" % bpp, seed=0x8d00 + bpp, compound=1)


def test_host_planned(v9, orc):
    """Case e."""
    old = os.environ.get("VP9HIP_HOST_PLAN")
    os.environ["VP9HIP_HOST_PLAN"] = "1"            # read when the context is opened
    try:
        dev = v9.Device(0)
    finally:
        if old is None:
            del os.environ["VP9HIP_HOST_PLAN"]
        else:
            os.environ["VP9HIP_HOST_PLAN"] = old
    try:
        _keyframes(v9, orc, dev, 72, 72, 8, "host-planned 72x72 stress", seed=0x8e00, **STRESS)
        _keyframes(v9, orc, dev, 72, 72, 10, "host-planned 72x72 10-bit lossless", seed=0x8e10, **LOSSLESS)
        _gop(v9, orc, dev, 136, 72, 8, "host-planned 136x72 compound GOP", seed=0x8e20, compound=1)
    finally:
        dev.close()


def test_sparse(v9, orc, gpu):
    """Case f."""
    _keyframes(v9, orc, gpu, 72, 72, 8, "72x72 sparse", seed=0x8f00, **SPARSE)
    _gop(v9, orc, gpu, 136, 72, 8, "136x72 sparse GOP", seed=0x8f10, **SPARSE)
