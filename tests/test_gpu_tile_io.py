"""Tile I/O of the pixel kernels: what moves between the frame buffers and the LDS tiles.

lf_sb (k_lf, the LF workgroups of k_plf) loads an SB's tile with its top and left halo in 16-byte
chunks and stores the filtered region back; the intra workgroup (pred_wg) loads the row above and
the column to the left, and stores the SB interior. Every case decodes into poisoned buffers
(0xA5 in every byte) and compares the visible Y / U / V with the oracle, sample-exact, with the
loop filter on. The shapes are the smallest at which this I/O can go wrong:

  64x64      one SB: no left and no top halo (the gx < 0, gy < 0 masks)
  136x72     3 x 2 SBs: both halos, an 8-pixel last column and an 8-row last row
  200x136    an interior SB with four neighbours
  520x72     two tile columns: the intra left column across a tile edge

at 8 and 10 bit, 4:2:0 for all and 4:2:2, 4:4:0, 4:4:4 for the first two; one case with
sharpness 3; a key + inter pair with intra blocks in the inter frame (the interior load path,
k_predd / k_lfro); and three keyframes in one batch (workgroups of one launch on different frames).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POISON = 0xA5
SHAPES = [(64, 64, {}), (136, 72, {}), (200, 136, {}), (520, 72, {"log2_tile_cols": 1})]
CASES = [(w, h, bpp, 1, 1, kw) for w, h, kw in SHAPES for bpp in (8, 10)]
CASES += [(w, h, bpp, ssh, ssv, kw) for w, h, kw in SHAPES[:2] for bpp in (8, 10) for ssh, ssv in ((1, 0), (0, 1), (0, 0))]
CASES += [(136, 72, 8, 1, 1, {"sharpness": 3})]


def _cmp(v9, got, ref, w, h, ssh, ssv, what):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


def _poisoned(gpu, w, h, bpp, nbufs, ssh=1, ssv=1):
    gpu.configure(w, h, bpp, nbufs=nbufs, ss_h=ssh, ss_v=ssv)
    gpu.fill(0, nbufs, POISON)
    gpu.sync()


@pytest.mark.parametrize("w,h,bpp,ssh,ssv,kw", CASES)
def test_keyframe_tile_io(v9, orc, gpu, w, h, bpp, ssh, ssv, kw):
    f = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=0x7110 + w + bpp, ss_h=ssh, ss_v=ssv, **kw))
    assert f.params.filter_level > 0
    _poisoned(gpu, w, h, bpp, 1, ssh, ssv)
    gpu.stage_batch([f], [0])
    gpu.run_batch()
    gpu.sync()
    ref = v9.alloc_planes(w, h, bpp, ssh, ssv)
    orc.decode_frame(f.pkt, ref)
    _cmp(v9, gpu.download(0), ref, w, h, ssh, ssv, "keyframe %dx%d@%d ss=%d%d %s" % (w, h, bpp, ssh, ssv, kw))


def test_inter_with_intra_blocks_tile_io(v9, orc, gpu):
    w, h = 136, 72
    key = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x7120))
    p = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x7121, inter=1, p_intra=0.4))
    assert key.params.filter_level > 0 and p.params.filter_level > 0
    _poisoned(gpu, w, h, 8, 2)
    gpu.stage_batch([key, p], [0, 1], [None, (0, 0, 0)])
    gpu.run_batch()
    gpu.sync()
    r0 = v9.alloc_planes(w, h, 8)
    orc.decode_frame(key.pkt, r0)
    r1 = v9.alloc_planes(w, h, 8)
    orc.decode_frame(p.pkt, r1, [r0, r0, r0])
    _cmp(v9, gpu.download(0), r0, w, h, 1, 1, "key of the pair")
    _cmp(v9, gpu.download(1), r1, w, h, 1, 1, "inter frame with intra blocks")


def test_three_frames_one_launch_tile_io(v9, orc, gpu):
    w, h = 136, 72
    frames = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x7130 + i)) for i in range(3)]
    _poisoned(gpu, w, h, 8, 3)
    gpu.stage_batch(frames, [0, 1, 2])
    gpu.run_batch()
    gpu.sync()
    for i, f in enumerate(frames):
        ref = v9.alloc_planes(w, h, 8)
        orc.decode_frame(f.pkt, ref)
        _cmp(v9, gpu.download(i), ref, w, h, 1, 1, "batch frame %d" % i)
