"""Motion export, the definition (include/vp9hip.h "motion export"), without a GPU.

motion_field() restates the definition in numpy over frame.blocks(); it shares no code with the
library and is what tests/test_gpu_motion.py compares the device tensors with. Here: the
blocks of a packet partition the cell grid (every cell hit exactly once), the packets fill
mode[] / mv[] of every block the way the definition relies on (ff_vp9_fill_mv: four equal
copies at >= 8x8, row pairs at 8x4, column pairs at 4x8), for the synthetic generator's packets
and for the parser's, and vp9hip_motion_host, the C statement, equals the restatement.
"""
import ctypes

import numpy as np
import pytest

N_BS = 13
# width / height of VP9H_BS_* in 4-pixel units; below 8x8 a block covers its 8x8 unit
W4 = (16, 16, 8, 8, 8, 4, 4, 4, 2, 2, 2, 2, 2)
H4 = (16, 8, 16, 8, 4, 8, 4, 2, 4, 2, 2, 2, 2)
BS_8X8, BS_8X4, BS_4X8, BS_4X4 = 9, 10, 11, 12


def motion_field(blocks, width, height):
    """(mv, info, hits): int16 (GH, GW, 2, 2), uint8 (GH, GW, 4) and the number of blocks that
    cover each cell, from the definition."""
    cols8, rows8 = (width + 7) >> 3, (height + 7) >> 3
    gw, gh = 2 * cols8, 2 * rows8
    mv = np.zeros((gh, gw, 2, 2), np.int16)
    info = np.zeros((gh, gw, 4), np.uint8)
    hits = np.zeros((gh, gw), np.int32)
    for b in blocks:
        if b.bs >= N_BS or b.row >= rows8 or b.col >= cols8:
            continue
        r0, c0 = 2 * b.row, 2 * b.col
        r1, c1 = min(r0 + H4[b.bs], gh), min(c0 + W4[b.bs], gw)
        i0 = 255 if b.intra else b.ref[0]
        i1 = b.ref[1] if (not b.intra and b.comp) else 255
        bmv = np.array(b.mv[:], np.int16).reshape(4, 2, 2)       # [i][k][x, y]
        if i0 == 255:
            bmv[:, 0] = 0
        if i1 == 255:
            bmv[:, 1] = 0
        sub = np.array([[0, 1], [2, 3]])[np.arange(r0, r1)[:, None] & 1, np.arange(c0, c1)[None, :] & 1]
        info[r0:r1, c0:c1, 0] = i0
        info[r0:r1, c0:c1, 1] = i1
        info[r0:r1, c0:c1, 2] = np.array(b.mode[:], np.uint8)[sub]
        info[r0:r1, c0:c1, 3] = (b.bs | b.skip << 4 | b.seg_id << 5) & 255
        mv[r0:r1, c0:c1] = bmv[sub]
        hits[r0:r1, c0:c1] += 1
    return mv, info, hits


SIZES = [(8, 8), (66, 66), (66, 34), (200, 130)]
KINDS = {"key": {}, "inter": dict(inter=1), "compound": dict(inter=1, compound=1)}
CASES = [(w, h, k, {}) for w, h in SIZES for k in KINDS] + [(66, 66, "inter", dict(p_intra=0.4))]


def _synth(v9, w, h, kind, extra, seed=4100):
    return v9.SynthFrame(v9.synth_params(w, h, 8, seed=seed + 7 * w + h, **KINDS[kind], **extra))


def _id(c):
    return "%dx%d-%s%s" % (c[0], c[1], c[2], "-intra" if c[3] else "")


def _replicated(blocks):
    """The definition's premise, per block: mode[] and mv[] entries of sub-blocks the block's
    size does not split are equal."""
    for n, b in enumerate(blocks):
        m = list(b.mode)
        v = np.array(b.mv[:]).reshape(4, 4)
        if b.bs < BS_8X4:
            same = [(0, 1), (0, 2), (0, 3)]
        elif b.bs == BS_8X4:
            same = [(0, 1), (2, 3)]          # one row of the 8x8 per sub-block
        elif b.bs == BS_4X8:
            same = [(0, 2), (1, 3)]          # one column
        else:
            same = []
        for i, j in same:
            assert m[i] == m[j], "block %d (bs %d): mode[%d] != mode[%d]" % (n, b.bs, i, j)
            assert (v[i] == v[j]).all(), "block %d (bs %d): mv[%d] != mv[%d]" % (n, b.bs, i, j)


def _check_host(v9, frame):
    pk = frame.pkt
    mv, info, hits = motion_field(frame.blocks(), pk.width, pk.height)
    assert hits.min() == 1 and hits.max() == 1, "cells hit %d..%d times" % (hits.min(), hits.max())
    hmv, hinfo = v9.motion_host(frame)
    assert hmv.shape == mv.shape and hmv.dtype == np.int16 and hinfo.shape == info.shape and hinfo.dtype == np.uint8
    assert np.array_equal(hinfo, info) and np.array_equal(hmv, mv)
    return mv, info


@pytest.mark.parametrize("case", CASES, ids=_id)
def test_partition_replication_and_host(v9, case):
    w, h, kind, extra = case
    f = _synth(v9, w, h, kind, extra)
    _replicated(f.blocks())
    mv, info = _check_host(v9, f)
    assert mv.shape == (2 * ((h + 7) >> 3), 2 * ((w + 7) >> 3), 2, 2)
    if kind == "key":
        assert (info[..., 0] == 255).all() and (info[..., 1] == 255).all() and not mv.any()
    else:
        inter = info[..., 0] != 255
        assert (info[..., 0][inter] <= 2).all()
        assert inter.any() or (w, h) == (8, 8)                    # one block: it may be the intra one
        assert not mv[~inter].any()                               # intra cells: zero vectors
        single = inter & (info[..., 1] == 255)
        assert not mv[single][:, 1].any()
        if extra:
            assert (~inter).any() and inter.any()                 # intra blocks among inter blocks
        if kind == "compound" and (w, h) != (8, 8):
            assert (info[..., 1] != 255).any()


@pytest.mark.parametrize("w,h", SIZES)
def test_parsed_packets(v9, w, h):
    """The same frames through Stream.encode -> Stream.decode: the parser's packets keep the
    replication rule and give the same fields through the C statement and the restatement."""
    frames = [_synth(v9, w, h, k, {}) for k in ("key", "inter", "compound")]
    frames.append(_synth(v9, w, h, "inter", dict(p_intra=0.4), seed=4200))
    enc, dec = v9.Stream(), v9.Stream()
    for i, f in enumerate(frames):
        data, coded = enc.encode(f) if i == 0 else enc.encode(f, ref_slot=(0, 0, 0), refresh_mask=0)
        p, _ = dec.decode(data)
        assert p.pkt.nblocks == coded.pkt.nblocks
        _replicated(p.blocks())
        mv, info = _check_host(v9, p)
        cmv, cinfo = v9.motion_host(coded)
        assert np.array_equal(cmv, mv) and np.array_equal(cinfo, info)


def _copy_packet(v9, pkt):
    """A copy of a packet whose block array is the test's own (the original is not touched)."""
    blocks = (v9.Block * pkt.nblocks)()
    ctypes.memmove(blocks, pkt.blocks, ctypes.sizeof(blocks))
    cp = v9.FramePacket()
    ctypes.memmove(ctypes.byref(cp), ctypes.byref(pkt), ctypes.sizeof(cp))
    cp.blocks = ctypes.cast(blocks, ctypes.POINTER(v9.Block))
    return cp, blocks


def test_single_reference_second_vector_is_zero(v9):
    f = _synth(v9, 66, 66, "compound", {})
    want_mv, want_info, _ = motion_field(f.blocks(), 66, 66)
    cp, blocks = _copy_packet(v9, f.pkt)
    poisoned = 0
    for b in blocks:
        if not b.intra and not b.comp:
            for i in range(4):
                b.mv[i * 4 + 2], b.mv[i * 4 + 3] = 0x1234, -0x4321
            b.ref[1] = 2
            poisoned += 1
    assert poisoned
    mv, info = v9.motion_host(cp)
    assert np.array_equal(mv, want_mv) and np.array_equal(info, want_info)
    single = (info[..., 0] != 255) & (info[..., 1] == 255)
    assert single.any() and not mv[single][:, 1].any()
    # the restatement agrees on the poisoned copy, and the original packet is unchanged
    pmv, pinfo, _ = motion_field(list(blocks), 66, 66)
    assert np.array_equal(pmv, want_mv) and np.array_equal(pinfo, want_info)
    assert np.array_equal(v9.motion_host(f)[0], want_mv)


def test_64x64_at_the_corner_is_clipped(v9):
    """One 64x64 block at SB (1, 1) of a 66x66 frame covers the 2 x 2 cells the grid has left."""
    f = _synth(v9, 66, 66, "inter", {})
    cp, blocks = _copy_packet(v9, f.pkt)
    keep = [b for b in blocks if not (b.row >= 8 and b.col >= 8)]
    assert len(keep) < len(blocks)
    arr = (v9.Block * (len(keep) + 1))()
    for i, b in enumerate(keep):
        ctypes.memmove(ctypes.byref(arr[i]), ctypes.byref(b), ctypes.sizeof(v9.Block))
    big = arr[len(keep)]
    big.row, big.col, big.bs, big.skip, big.seg_id = 8, 8, 0, 1, 3
    big.ref[0] = 1
    for i in range(4):
        big.mode[i] = 13
        big.mv[i * 4], big.mv[i * 4 + 1] = -77, 1234
    cp.blocks, cp.nblocks = ctypes.cast(arr, ctypes.POINTER(v9.Block)), len(arr)
    mv, info, hits = motion_field(list(arr), 66, 66)
    assert hits.shape == (18, 18) and hits.min() == 1 and hits.max() == 1
    assert (info[16:, 16:] == (1, 255, 13, 0 | 1 << 4 | 3 << 5)).all()
    assert (mv[16:, 16:, 0] == (-77, 1234)).all() and not mv[16:, 16:, 1].any()
    hmv, hinfo = v9.motion_host(cp)
    assert np.array_equal(hmv, mv) and np.array_equal(hinfo, info)


def test_motion_host_bad_arguments(v9):
    f = _synth(v9, 8, 8, "key", {})
    L = v9.lib()
    mv, info = np.zeros((2, 2, 2, 2), np.int16), np.zeros((2, 2, 4), np.uint8)
    assert L.vp9hip_motion_host(ctypes.byref(f.pkt), mv.ctypes.data, info.ctypes.data) == 4
    assert L.vp9hip_motion_host(None, mv.ctypes.data, info.ctypes.data) == v9.EINVAL
    assert L.vp9hip_motion_host(ctypes.byref(f.pkt), None, info.ctypes.data) == v9.EINVAL
    assert L.vp9hip_motion_host(ctypes.byref(f.pkt), mv.ctypes.data, None) == v9.EINVAL
