"""The synthetic generator's coverage switches (eob_dense, ref_mix, mv_range, edge_large, p_intra) and the packet
walker the GPU tests build their coverage conditions on (tests/synth_walk.py).

With the switches at 0 the generator draws what it always drew: the digests below were taken
from the generator before the switches existed, over keyframes, inter frames, high bit depth,
coefficient stress, lossless, 4:4:4 with segmentation, and tile columns.
"""
import collections

import numpy as np
import pytest

import synth_walk

SEG = {"enabled": 1, "update_map": 1, "update_data": 1, "q_en": 6, "q": [0, 20, -20, 0, 0, 0, 0, 0], "lf_en": 2,
       "lf": [0, 10, 0, 0, 0, 0, 0, 0], "nseg": 4, "lf_delta_update": 1, "lf_ref": [2, 0, -2, 5], "lf_mode": [1, -1]}
PINNED = [
    (352, 288, 8, {"seed": 0x56503900},
     "bf77e023873c9dbd12e18af29fba5c450b824e8534bfbe2f6617e9484dcdc9f2"),
    (200, 130, 8, {"seed": 7, "inter": 1, "compound": 1},
     "04112afb5cf47882727238289e8d71c931c8783e6e0c0fd217b3a57f56721307"),
    (136, 72, 10, {"seed": 9, "coef_stress": 1, "q_idx": 255},
     "bdd43c419612b3ab93cc945a3b11806089590edd129f0645edf7306c476b57e4"),
    (66, 66, 12, {"seed": 11, "inter": 1, "bilinear": 1, "p_zero_eob": 0.3},
     "b9e93eaf063a6004ff27d91aec735f6b92dd004fdd7369c59a4f381aceb9ad79"),
    (200, 136, 8, {"seed": 13, "lossless": 1, "q_idx": 0},
     "dc011125406a584c6d00499e349ce452227677a0d7437dfbda0fa9ace188ffa5"),
    (176, 144, 10, {"seed": 15, "inter": 1, "compound": 1, "ss_h": 0, "ss_v": 0, "seg": SEG},
     "637a142a9eae95d4a864282cfde77223019c2ab54a91edc35f039d68e0e12ed2"),
    (1024, 128, 8, {"seed": 17, "log2_tile_cols": 2},
     "8033259b3410e7f8cb1f0ea6fe32d2af9ab46b6234565e291501c5ef19fe6675"),
]


@pytest.mark.parametrize("w,h,bpp,kw,digest", PINNED, ids=[str(i) for i in range(len(PINNED))])
def test_default_packets_are_pinned(v9, w, h, bpp, kw, digest):
    f = v9.SynthFrame(v9.synth_params(w, h, bpp, **kw))
    assert synth_walk.packet_digest(f.pkt) == digest
    # explicit zeros are the defaults
    z = v9.SynthFrame(v9.synth_params(w, h, bpp, eob_dense=0, ref_mix=0, mv_range=0, edge_large=0, p_intra=0, **kw))
    assert synth_walk.packet_digest(z.pkt) == digest
    # ±512 spelled out is the default range, draw for draw
    m = v9.SynthFrame(v9.synth_params(w, h, bpp, mv_range=512, **kw))
    assert synth_walk.packet_digest(m.pkt) == digest


def test_walker_replays_the_generator(v9):
    """The walk consumes exactly the packet's eobs and coefficients (asserted inside walk) for
    every subsampling, partial SBs, sub-8x8 blocks, skips and zero eobs; default eobs stay
    in 1..64."""
    for (w, h), (ssh, ssv), kw in (((136, 72), (1, 1), {}), ((67, 41), (1, 1), {"inter": 1, "p_zero_eob": 0.5}),
                                  ((72, 136), (0, 0), {}), ((130, 66), (1, 0), {"inter": 1}),
                                  ((66, 130), (0, 1), {"lossless": 1, "q_idx": 0})):
        f = v9.SynthFrame(v9.synth_params(w, h, 8, seed=21, ss_h=ssh, ss_v=ssv, **kw))
        txbs = list(synth_walk.walk(f.pkt))
        assert len(txbs) == f.pkt.neobs
        assert all(0 <= t.eob <= min(16 << (2 * t.tx), 64) for t in txbs)
        assert all((t.mode is None) == (not t.block.intra) for t in txbs)
        assert all(t.tx == (t.block.uvtx if t.plane else t.block.tx) for t in txbs)


@pytest.mark.parametrize("bpp,kw", [(8, {}), (10, {"coef_stress": 1, "q_idx": 255}), (12, {"p_zero_eob": 0.3}),
                                    (8, {"seg": SEG}), (8, {"inter": 1, "compound": 1})],
                         ids=["plain", "stress10", "zero_eob12", "seg", "inter"])
def test_eob_dense_reaches_the_edges(v9, bpp, kw):
    frames = [v9.SynthFrame(v9.synth_params(352, 288, bpp, seed=31 + i, eob_dense=1, **kw)) for i in range(16)]
    hist = synth_walk.eob_histogram([f.pkt for f in frames])
    for tx in (2, 3):
        N = 4 << tx
        n = N * N
        eobs = collections.Counter({e: c for (t, e), c in hist.items() if t == tx})
        tot = sum(c for e, c in eobs.items() if e)
        for e in (n, n - 1, 8 * N, 8 * N + 1, 65):
            # one draw in eight each, plus what the uniform draw adds: well above one in sixteen
            assert eobs[e] > tot / 16, (tx, e, eobs[e], tot)
        assert max(eobs) == n and min(e for e in eobs if e) >= 1
        other = sum(c for e, c in eobs.items() if e > 64 and e not in (n, n - 1, 8 * N, 8 * N + 1, 65))
        short = sum(c for e, c in eobs.items() if 1 <= e <= 64)
        assert other > tot / 8 and short > tot / 16            # the uniform draw and the default one
        assert (eobs[0] > 0) == bool(kw.get("p_zero_eob"))
    # smaller blocks are unchanged in kind
    assert all(e <= 16 << (2 * t) for (t, e) in hist if t < 2)


def test_eob_dense_leaves_small_transforms_and_lossless_alone(v9):
    a = v9.SynthFrame(v9.synth_params(200, 136, 8, seed=41, lossless=1, q_idx=0))
    b = v9.SynthFrame(v9.synth_params(200, 136, 8, seed=41, lossless=1, q_idx=0, eob_dense=1))
    assert synth_walk.packet_digest(a.pkt) == synth_walk.packet_digest(b.pkt)      # lossless: 4x4 only


def test_ref_mix_draws_every_reference(v9):
    f = v9.SynthFrame(v9.synth_params(352, 288, 8, seed=51, inter=1, compound=1, ref_mix=1))
    single, comp = collections.Counter(), collections.Counter()
    for b in f.blocks():
        if b.intra:
            continue
        if b.comp:
            comp[(b.ref[0], b.ref[1])] += 1
        else:
            single[b.ref[0]] += 1
    assert set(single) == {0, 1, 2} and min(single.values()) > sum(single.values()) / 6
    assert set(comp) == {(0, 2), (1, 2)} and min(comp.values()) > sum(comp.values()) / 4
    g = v9.SynthFrame(v9.synth_params(352, 288, 8, seed=51, inter=1, ref_mix=1))
    assert not any(b.comp for b in g.blocks())


def test_mv_range(v9):
    for r in (1, 100, 4000, 16383):
        f = v9.SynthFrame(v9.synth_params(200, 130, 8, seed=61, inter=1, compound=1, mv_range=r))
        mv = np.array([list(b.mv) for b in f.blocks() if not b.intra])
        assert mv.min() >= -r and mv.max() <= r
        assert mv.min() < -0.8 * r and mv.max() > 0.8 * r
    for r in (-1, 16384):
        with pytest.raises(v9.Vp9HipError):
            v9.SynthFrame(v9.synth_params(200, 130, 8, inter=1, mv_range=r))


def _cut_blocks(f):
    """(blocks the frame's right or bottom edge cuts, those of them with one of the two largest
    tx sizes the block size allows)"""
    cols, rows = (f.pkt.width + 7) >> 3, (f.pkt.height + 7) >> 3
    max_tx = [3, 3, 3, 3, 2, 2, 2, 1, 1, 1, 0, 0, 0]
    cut = [b for b in f.blocks() if b.col + synth_walk.BWH8[b.bs][0] > cols or b.row + synth_walk.BWH8[b.bs][1] > rows]
    return cut, [b for b in cut if b.tx >= max_tx[b.bs] - 1]


def test_edge_large_keeps_cut_blocks_whole_and_their_transforms_large(v9):
    """88x88: the second superblock column and row show 24 pixels. With edge_large the blocks
    the frame edge cuts are fewer and larger (fewer splits of cut squares) and seven in eight of them take
    one of their two largest tx sizes (three in four by the switch, half of the rest by the
    uniform draw; blocks of 8x8 and below have two sizes at most)."""
    big, n_cut = {}, {}
    for sw in (0, 1):
        fr = [v9.SynthFrame(v9.synth_params(88, 88, 8, seed=71 + i, edge_large=sw)) for i in range(64)]
        cut = [c for f in fr for c in _cut_blocks(f)[0]]
        large = [c for f in fr for c in _cut_blocks(f)[1]]
        n_cut[sw] = len(cut)
        big[sw] = sum(b.bs < 3 for b in cut)                     # the forced 64x32 / 32x64 of a cut superblock
        assert sw == 0 or len(large) > 0.8 * len(cut), (len(large), len(cut))
        # inside the frame nothing changes in kind: every tx size of the uncut 32x32 and larger blocks
        assert {b.tx for f in fr for b in f.blocks() if b.bs < 6} == {0, 1, 2, 3}
    # 128 cut superblocks stay whole with chance 0.7, not 0.3: 90 against 38, sigma 5 each
    assert n_cut[1] < n_cut[0] and big[1] > 1.5 * big[0], (n_cut, big)
    # lossless stays 4x4
    f = v9.SynthFrame(v9.synth_params(88, 88, 8, seed=71, lossless=1, q_idx=0, edge_large=1))
    assert {b.tx for b in f.blocks()} == {0}


def test_p_intra_sets_the_intra_share_of_inter_frames(v9):
    for share in (0.1, 0.5, 0.85, 1.0):
        f = v9.SynthFrame(v9.synth_params(352, 288, 8, seed=81, inter=1, p_intra=share))
        bl = f.blocks()
        got = sum(b.intra for b in bl) / len(bl)
        assert abs(got - share) < 0.05, (share, got, len(bl))         # > 1000 blocks: sigma < 0.016
    k = v9.SynthFrame(v9.synth_params(352, 288, 8, seed=81, p_intra=0.5))
    assert all(b.intra for b in k.blocks())                           # keyframes stay all intra
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(v9.Vp9HipError):
            v9.SynthFrame(v9.synth_params(352, 288, 8, inter=1, p_intra=bad))


def test_intra_txfm_type_is_the_reference_table(v9):
    # ff_vp9_intra_txfm_type: VERT ADST_DCT (2: second pass), HOR DCT_ADST, TM both ...
    assert [v9.intra_txfm_type(m) for m in range(10)] == [2, 1, 0, 0, 3, 2, 1, 2, 1, 3]
    with pytest.raises(v9.Vp9HipError):
        v9.intra_txfm_type(10)
