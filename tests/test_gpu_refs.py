"""GPU parity where the default generator never goes on the inter side, sample-exact vs the
oracle: every reference (ref_mix), references of three sizes in one frame, the legal scale
limits and one step beyond them, MVs far outside the frame (mv_range), odd frame sizes.

By default every single-reference block reads LAST and every compound block LAST + ALTREF, all
references have one size, MVs stay within +-64 px and decoded sizes are even. Here:

  refs     three different keyframes as LAST, GOLDEN and ALTREF; single-reference blocks on each
           of them, compound blocks on both codable pairs (asserted from the packet); again
           with segments and LF deltas (2, 0, -2, 5) per reference, so that a wrong lflvl row
           changes pixels. Before the GPU runs, the oracle must tell the frame from the one
           with GOLDEN and ALTREF exchanged, and from the one with their lflvl rows exchanged.
  mixed    LAST of the frame's size, GOLDEN larger, ALTREF smaller: compound blocks take the
           scaled template with one unscaled reference
  limits   a reference exactly twice the frame (step 32), one sixteenth of it (step 1), one
           axis only; one step beyond either limit the frame whose blocks use that reference
           is rejected alone with AVERROR_INVALIDDATA and the next clean batch is bit-exact
  far      MVs of +-500 px: blocks whose whole filter window lies outside the reference on
           each side and at a corner (asserted from the packet), unscaled and scaled
  odd      65x33, 67x41, 9x9 as key + inter, 4:2:0, 4:2:2 and 4:4:0: chroma one larger than
           half; and a scaled reference whose size alone is odd
"""
import numpy as np
import pytest

import synth_walk

pytestmark = pytest.mark.gpu

SEG_LF = {"enabled": 1, "update_map": 1, "update_data": 1, "lf_en": 0b0110, "lf": [0, 9, -7, 0, 0, 0, 0, 0], "nseg": 4,
          "lf_delta_update": 1, "lf_ref": [2, 0, -2, 5], "lf_mode": [1, -1]}


def _cmp(v9, got, ref, w, h, what, ssh=1, ssv=1):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


def _same(v9, a, b, w, h):
    return all(np.array_equal(x, y) for x, y in zip(v9.visible(a, w, h), v9.visible(b, w, h)))


def _oracle_key(v9, orc, w, h, bpp, seed, ssh=1, ssv=1):
    key = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, ss_h=ssh, ss_v=ssv))
    out = v9.alloc_planes(w, h, bpp, ssh, ssv)
    orc.decode_frame(key.pkt, out)
    return key, out


def check_ref_coverage(f):
    single, comp = set(), set()
    for b in f.blocks():
        if not b.intra:
            (comp if b.comp else single).add((b.ref[0], b.ref[1]) if b.comp else b.ref[0])
    assert single == {0, 1, 2}, "single-reference blocks on %s" % single
    assert comp == {(0, 2), (1, 2)}, "compound blocks on %s" % comp


# the first two seeds from 0xa000 on whose frame meets check_ref_coverage: (w, h, seg) -> seeds
# (bit depth does not change what the generator draws)
REF_SEEDS = {(200, 130, 0): (0xa000, 0xa001), (200, 130, 1): (0xa000, 0xa001), (66, 66, 0): (0xa000, 0xa001),
             (66, 66, 1): (0xa001, 0xa002)}


@pytest.mark.parametrize("seg", [0, 1], ids=["plain", "seg_lf"])
@pytest.mark.parametrize("w,h,bpp", [(200, 130, 8), (200, 130, 10), (66, 66, 8)])
def test_every_reference(v9, orc, gpu, w, h, bpp, seg):
    keys = [_oracle_key(v9, orc, w, h, bpp, 0xa100 + i)[1] for i in range(3)]
    gpu.configure(w, h, bpp, nbufs=4)
    for i in range(3):
        gpu.upload(i, keys[i])
    for seed in REF_SEEDS[(w, h, seg)]:
        f = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, inter=1, compound=1, ref_mix=1,
                                          **({"seg": SEG_LF} if seg else {})))
        check_ref_coverage(f)
        out = v9.alloc_planes(w, h, bpp)
        orc.decode_frame(f.pkt, out, keys)
        # the packet tells the references apart: GOLDEN and ALTREF exchanged is another picture
        swapped = v9.alloc_planes(w, h, bpp)
        orc.decode_frame(f.pkt, swapped, [keys[0], keys[2], keys[1]])
        assert not _same(v9, out, swapped, w, h)
        if seg:
            # ... and so is the frame with the LF levels of GOLDEN and ALTREF exchanged
            lv = bytes(f.pkt.lflvl)
            for s in range(8):
                for m in range(2):
                    f.pkt.lflvl[s * 8 + 4 + m], f.pkt.lflvl[s * 8 + 6 + m] = lv[s * 8 + 6 + m], lv[s * 8 + 4 + m]
            orc.decode_frame(f.pkt, swapped, keys)
            for k in range(64):
                f.pkt.lflvl[k] = lv[k]
            assert not _same(v9, out, swapped, w, h)
        gpu.submit(f, 3, (0, 1, 2))
        gpu.sync()
        _cmp(v9, gpu.download(3), out, w, h, "refs %dx%d@%d seg=%d seed %#x" % (w, h, bpp, seg, seed))


def _gpu_keys(v9, orc, dev, sizes, bpp, seed, ssh=1, ssv=1):
    """Keyframes of the given sizes decoded into buffers 0.. on the device and by the oracle."""
    refs = []
    for i, (rw, rh) in enumerate(sizes):
        key, out = _oracle_key(v9, orc, rw, rh, bpp, seed + i, ssh, ssv)
        dev.stage_batch([key], [i])
        dev.run_batch()
        dev.sync()
        _cmp(v9, dev.download(i), out, rw, rh, "reference keyframe %dx%d" % (rw, rh), ssh, ssv)
        refs.append(out)
    return refs


def _scaled_frame(v9, orc, dev, f, sizes, refs, bufs, out_buf, what, ssh=1, ssv=1):
    for r in range(3):
        f.pkt.ref_w[r], f.pkt.ref_h[r] = sizes[r]
    w, h, bpp = f.pkt.width, f.pkt.height, f.pkt.bpp
    dev.stage_batch([f], [out_buf], [bufs])
    dev.run_batch()
    dev.sync()
    out = v9.alloc_planes(w, h, bpp, ssh, ssv)
    orc.decode_frame(f.pkt, out, refs, list(sizes))
    _cmp(v9, dev.download(out_buf), out, w, h, what, ssh, ssv)
    return out


@pytest.mark.parametrize("bpp,kw", [(8, {}), (10, {}), (8, {"bilinear": 1})], ids=["8", "10", "bilinear"])
def test_mixed_scales(v9, orc, gpu, bpp, kw):
    """LAST the frame's size, GOLDEN larger, ALTREF smaller, from three keyframes."""
    w, h = 200, 130
    sizes = [(200, 130), (264, 200), (136, 72)]
    gpu.configure(264, 200, bpp, nbufs=4)
    refs = _gpu_keys(v9, orc, gpu, sizes, bpp, 0xa200)
    for seed in (0xa210, 0xa211):
        f = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, inter=1, compound=1, ref_mix=1, **kw))
        check_ref_coverage(f)
        out = _scaled_frame(v9, orc, gpu, f, sizes, refs, (0, 1, 2), 3, "mixed scales %d-bit %s seed %#x" % (bpp, kw, seed))
        other = v9.alloc_planes(w, h, bpp)
        orc.decode_frame(f.pkt, other, [refs[0], refs[2], refs[1]], [sizes[0], sizes[2], sizes[1]])
        assert not _same(v9, out, other, w, h)


LIMITS = [((128, 128), (64, 64)),       # a reference exactly twice the frame: step 32
          ((16, 16), (256, 256)),       # one sixteenth: step 1
          ((128, 72), (96, 72))]        # one axis only


@pytest.mark.parametrize("rs,fs", LIMITS, ids=["2x", "1_16", "x_only"])
def test_scale_limits(v9, orc, gpu, rs, fs):
    (rw, rh), (w, h) = rs, fs
    gpu.configure(max(rw, w), max(rh, h), 8, nbufs=2)
    refs = _gpu_keys(v9, orc, gpu, [rs], 8, 0xa300)
    for seed in (0xa310, 0xa311):
        f = v9.SynthFrame(v9.synth_params(w, h, 8, seed=seed, inter=1, compound=1, ref_mix=1))
        _scaled_frame(v9, orc, gpu, f, [rs] * 3, refs * 3, (0, 0, 0), 1, "reference %dx%d -> %dx%d seed %#x" % (rw, rh, w, h, seed))


@pytest.mark.parametrize("rs,fs", [((130, 128), (64, 64)), ((128, 130), (64, 64)), ((16, 16), (264, 256)),
                                   ((16, 16), (256, 264))], ids=["2x_w", "2x_h", "1_16_w", "1_16_h"])
def test_beyond_the_scale_limits_the_frame_is_rejected_alone(v9, orc, rs, fs):
    """GOLDEN one step beyond a limit (vp9.c:845-880: twice the frame, one sixteenth of it), LAST
    and ALTREF of the frame's size: the frame's blocks on GOLDEN cannot be predicted, so the
    frame is rejected (AVERROR_INVALIDDATA, the other frame of the batch not run); the same
    batch with a legal GOLDEN then decodes bit-exact."""
    (rw, rh), (w, h) = rs, fs
    dev = v9.Device(0)
    try:
        dev.configure(max(rw, w), max(rh, h), 8, nbufs=4)
        refs = _gpu_keys(v9, orc, dev, [fs, rs], 8, 0xa400)
        bad = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0xa410, inter=1, compound=1, ref_mix=1))   # meets the check
        good = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0xa411, inter=1, compound=1, ref_mix=1))
        check_ref_coverage(bad)
        bad.pkt.ref_w[1], bad.pkt.ref_h[1] = rs
        dev.stage_batch([bad, good], [2, 3], [(0, 1, 0), (0, 0, 0)])
        with pytest.raises(v9.Vp9HipError) as e:
            dev.run_batch()
            dev.sync()
        assert e.value.code == v9.EINVALIDDATA
        assert dev.frame_status(0) == [v9.EINVALIDDATA, v9.EAGAIN]
        bad.pkt.ref_w[1], bad.pkt.ref_h[1] = fs
        dev.stage_batch([bad, good], [2, 3], [(0, 0, 0), (0, 0, 0)])
        dev.run_batch()
        dev.sync()
        assert dev.frame_status(0) == [0, 0]
        for f, buf in ((bad, 2), (good, 3)):
            out = v9.alloc_planes(w, h, 8)
            orc.decode_frame(f.pkt, out, [refs[0]] * 3)
            _cmp(v9, dev.download(buf), out, w, h, "clean batch after the rejection, buffer %d" % buf)
    finally:
        dev.close()


def check_far_coverage(f, w, h):
    """Blocks of 8x8 and larger whose luma filter window (the block moved by its first MV, 3
    pixels before and 4 after it) lies wholly outside the reference: on each side, and at a
    corner (outside on both axes)."""
    seen = set()
    for b in f.blocks():
        if b.intra or b.bs > synth_walk.BS_8x8:
            continue
        bw, bh = (8 * x for x in synth_walk.BWH8[b.bs])
        x0, y0 = b.col * 8 + (b.mv[0] >> 3) - 3, b.row * 8 + (b.mv[1] >> 3) - 3
        sx = "left" if x0 + bw + 8 < 0 else "right" if x0 >= w else ""
        sy = "top" if y0 + bh + 8 < 0 else "bottom" if y0 >= h else ""
        seen.update(s for s in (sx, sy) if s)
        if sx and sy:
            seen.add("corner")
    assert seen == {"left", "right", "top", "bottom", "corner"}, seen


# the first two seeds from 0xa510 on whose frame meets check_far_coverage
FAR_SEEDS = {(72, "compound"): (0xa511, 0xa512), (72, "10"): (0xa511, 0xa512), (72, "bilinear"): (0xa510, 0xa511)}


@pytest.mark.parametrize("w,h", [(72, 72), (200, 130)])
@pytest.mark.parametrize("bpp,kw,name", [(8, {"compound": 1}, "compound"), (10, {}, "10"), (8, {"bilinear": 1}, "bilinear")],
                         ids=["compound", "10", "bilinear"])
def test_far_mvs(v9, orc, gpu, w, h, bpp, kw, name):
    keys = [_oracle_key(v9, orc, w, h, bpp, 0xa500 + i)[1] for i in range(3)]
    gpu.configure(w, h, bpp, nbufs=4)
    for i in range(3):
        gpu.upload(i, keys[i])
    for seed in FAR_SEEDS.get((w, name), (0xa510, 0xa511)):
        f = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, inter=1, ref_mix=1, mv_range=4000, **kw))
        check_far_coverage(f, w, h)
        gpu.submit(f, 3, (0, 1, 2))
        gpu.sync()
        out = v9.alloc_planes(w, h, bpp)
        orc.decode_frame(f.pkt, out, keys)
        _cmp(v9, gpu.download(3), out, w, h, "far MVs %dx%d@%d %s seed %#x" % (w, h, bpp, kw, seed))


def test_far_mvs_scaled_reference(v9, orc, gpu):
    """The scaled path clamps the MV before it scales it (pl_mc_luma_ref / pl_mc_chroma_ref)."""
    (rw, rh), (w, h) = (264, 200), (200, 130)
    gpu.configure(rw, rh, 8, nbufs=2)
    refs = _gpu_keys(v9, orc, gpu, [(rw, rh)], 8, 0xa600)
    for seed in (0xa610, 0xa611):
        f = v9.SynthFrame(v9.synth_params(w, h, 8, seed=seed, inter=1, compound=1, mv_range=4000))
        check_far_coverage(f, w, h)
        _scaled_frame(v9, orc, gpu, f, [(rw, rh)] * 3, refs * 3, (0, 0, 0), 1, "far MVs, scaled reference, seed %#x" % seed)


ODD = [(65, 33, 8, 1, 1), (65, 33, 10, 1, 1), (67, 41, 8, 1, 1), (67, 41, 10, 1, 1), (9, 9, 8, 1, 1), (9, 9, 10, 1, 1),
       (67, 41, 8, 1, 0), (67, 41, 8, 0, 1)]


@pytest.mark.parametrize("w,h,bpp,ssh,ssv", ODD)
def test_odd_sizes(v9, orc, gpu, w, h, bpp, ssh, ssv):
    """Key + inter as one batch; chroma is (w + 1) >> 1 by (h + 1) >> 1 where subsampled."""
    gpu.configure(w, h, bpp, nbufs=2, ss_h=ssh, ss_v=ssv)
    for seed in (0xa700, 0xa710, 0xa720):
        key = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, ss_h=ssh, ss_v=ssv))
        p = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 1, inter=1, compound=1, ss_h=ssh, ss_v=ssv))
        gpu.stage_batch([key, p], [0, 1], [None, (0, 0, 0)])
        gpu.run_batch()
        gpu.sync()
        k = v9.alloc_planes(w, h, bpp, ssh, ssv)
        orc.decode_frame(key.pkt, k)
        out = v9.alloc_planes(w, h, bpp, ssh, ssv)
        orc.decode_frame(p.pkt, out, [k, k, k])
        what = "%dx%d@%d ss %d%d seed %#x" % (w, h, bpp, ssh, ssv, seed)
        _cmp(v9, gpu.download(0), k, w, h, what + " key", ssh, ssv)
        _cmp(v9, gpu.download(1), out, w, h, what + " inter", ssh, ssv)


def test_odd_scaled_reference(v9, orc, gpu):
    """Only the reference's size is odd: 131x75 -> 200x130."""
    (rw, rh), (w, h) = (131, 75), (200, 130)
    gpu.configure(w, h, 8, nbufs=2)
    refs = _gpu_keys(v9, orc, gpu, [(rw, rh)], 8, 0xa800)
    for seed in (0xa810, 0xa811):
        f = v9.SynthFrame(v9.synth_params(w, h, 8, seed=seed, inter=1, compound=1))
        _scaled_frame(v9, orc, gpu, f, [(rw, rh)] * 3, refs * 3, (0, 0, 0), 1, "131x75 -> 200x130 seed %#x" % seed)
