"""GPU parity of the planner's tx records (k_psb -> k_pjplan), sample-exact vs the oracle.

k_psb enumerates every SB's tx blocks once and leaves one 8-byte record per tx block at
slot * JCAP (eob, residual key, rank within the key, position, intra mode); k_pjplan emits
the residual jobs and the intra job words from those records alone. The cases:

  a  200x136 lossless keyframes: every full SB has exactly JCAP = 384 tx blocks (six full
     chunks of 64, the clamp); the right column and bottom row are 8-px partial SBs
  b  72x72 4:4:4 lossless: JCAP = 768, ranks and counts beyond 9 bits
  c  72x72 4:2:2 and 4:4:0: the other chroma geometries
  d  520x72 10-bit, 2 tile columns, key + 2 P, sparse (p_skip 0.7, p_zero_eob 0.9): skipped
     blocks without eob entries inside the SB's eob window, inter tx records (destination from
     the frame pitch), intra blocks in inter frames (level schedule), a tile edge inside the
     frame (have_left at the tile's first SB column)
  e  a lossless batch (full record arenas), then a sparse batch of the same geometry in the
     same context and batch slot: nothing of the first batch's records may be read
  f  three batch slots (lossless, default density, sparse) run back to back without a host
     wait: each slot reads its own arena
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = 200, 136
SPARSE = {"p_skip": 0.7, "p_zero_eob": 0.9}
LOSSLESS = {"lossless": 1, "q_idx": 0}


def _cmp(v9, got, ref, w, h, what, ssh=1, ssv=1):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


@pytest.fixture(scope="module")
def sets(v9, orc):
    """The 200x136 8-bit 4:2:0 keyframe sets of cases a, e and f with their oracle frames
    (computed once, read-only): name -> [(frame, reference planes), ...]."""
    out = {}
    for name, kw, seed in (("lossless", LOSSLESS, 0x7a00), ("default", {}, 0x7a10), ("sparse", SPARSE, 0x7a20)):
        out[name] = []
        for i in range(2):
            f = v9.SynthFrame(v9.synth_params(W, H, 8, seed=seed + i, **kw))
            ref = v9.alloc_planes(W, H, 8)
            orc.decode_frame(f.pkt, ref)
            out[name].append((f, ref))
    return out


def _run_keyframes(v9, orc, gpu, w, h, bpp, frames, what, ssh=1, ssv=1):
    n = len(frames)
    gpu.configure(w, h, bpp, nbufs=n, ss_h=ssh, ss_v=ssv)
    gpu.stage_batch(frames, list(range(n)))
    gpu.run_batch()
    gpu.sync()
    for i, f in enumerate(frames):
        ref = v9.alloc_planes(w, h, bpp, ssh, ssv)
        orc.decode_frame(f.pkt, ref)
        _cmp(v9, gpu.download(i), ref, w, h, "%s frame %d" % (what, i), ssh, ssv)


def test_full_sbs_lossless(v9, gpu, sets):
    """Case a."""
    fr = sets["lossless"]
    gpu.configure(W, H, 8, nbufs=2)
    gpu.stage_batch([f for f, _ in fr], [0, 1])
    gpu.run_batch()
    gpu.sync()
    for i, (_, ref) in enumerate(fr):
        _cmp(v9, gpu.download(i), ref, W, H, "lossless keyframe %d" % i)


def test_444_lossless(v9, orc, gpu):
    """Case b."""
    f = v9.SynthFrame(v9.synth_params(72, 72, 8, seed=0x7b00, ss_h=0, ss_v=0, **LOSSLESS))
    _run_keyframes(v9, orc, gpu, 72, 72, 8, [f], "4:4:4 lossless", 0, 0)


@pytest.mark.parametrize("ssh,ssv", [(1, 0), (0, 1)])
def test_422_440(v9, orc, gpu, ssh, ssv):
    """Case c."""
    f = v9.SynthFrame(v9.synth_params(72, 72, 8, seed=0x7c00 + ssh, ss_h=ssh, ss_v=ssv))
    _run_keyframes(v9, orc, gpu, 72, 72, 8, [f], "ss=%d%d" % (ssh, ssv), ssh, ssv)


def test_sparse_gop_two_tiles(v9, orc, gpu):
    """Case d."""
    w, h, bpp, n = 520, 72, 10, 3
    refs = bench.gop_refs(n, n)
    frames = [v9.SynthFrame(v9.synth_params(w, h, bpp, seed=0x7d00 + i, log2_tile_cols=1,
                                            inter=int(refs[i] is not None), **SPARSE)) for i in range(n)]
    gpu.configure(w, h, bpp, nbufs=n)
    gpu.stage_batch(frames, list(range(n)), refs)
    gpu.run_batch()
    gpu.sync()
    dec = []
    for i, f in enumerate(frames):
        out = v9.alloc_planes(w, h, bpp)
        r = refs[i]
        orc.decode_frame(f.pkt, out, None if r is None else [dec[r[0]], dec[r[1]], dec[r[2]]])
        dec.append(out)
        _cmp(v9, gpu.download(i), out, w, h, "sparse GOP frame %d" % i)


def test_stale_records(v9, sets):
    """Case e."""
    dev = v9.Device(0)
    try:
        dev.configure(W, H, 8, nbufs=2)
        for name in ("lossless", "sparse"):        # same context, same batch slot
            dev.stage_batch([f for f, _ in sets[name]], [0, 1])
            dev.run_batch()
            dev.sync()
        for i, (_, ref) in enumerate(sets["sparse"]):
            _cmp(v9, dev.download(i), ref, W, H, "sparse batch after a lossless one, frame %d" % i)
    finally:
        dev.close()


def test_slot_isolation(v9, sets):
    """Case f."""
    names = ("lossless", "default", "sparse")
    dev = v9.Device(0)
    try:
        dev.configure(W, H, 8, nbufs=6)
        for k, name in enumerate(names):
            dev.set_slot(k)
            dev.stage_batch([f for f, _ in sets[name]], [2 * k, 2 * k + 1])
        bench.run_slots(dev, 3, 3)                 # no host wait between the slots' runs
        dev.sync()
        for k, name in enumerate(names):
            for i, (_, ref) in enumerate(sets[name]):
                _cmp(v9, dev.download(2 * k + i), ref, W, H, "slot %d (%s) frame %d" % (k, name, i))
    finally:
        dev.close()
