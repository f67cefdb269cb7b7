"""The crafted loop-filter frames of tests/lf_cases.py, checked with the oracle alone (CPU): the
frames are what they claim to be (no intra block, no coefficient, prediction a copy of the
picture), and every group meets the coverage conditions test_gpu_lf_arms.py relies on, counted
by the oracle's census: every reachable arm on lines that move, in both plane classes and
directions, the 7-tap arm under a 16-wide edge, every representable comparison on its
threshold and one above it. The natural-content set covers every level at every sharpness."""
import ctypes

import numpy as np
import pytest

import lf_cases
import lf_reference
import synth_walk


def _gid(g):
    return "L%d_S%d_%dbit_ss%d%d" % g


def test_seeds_are_the_first_from_the_base():
    assert lf_cases.SEEDS == tuple(lf_cases.SEED_BASE + i for i in range(len(lf_cases.SEEDS)))


@pytest.mark.parametrize("group", lf_cases.GROUPS, ids=_gid)
def test_unfiltered_frame_is_the_picture(v9, orc, group):
    level, sharp, bd, ssh, ssv = group
    for f, pic in lf_cases.group_frames(v9, group):
        w, h = f.pkt.width, f.pkt.height
        assert not any(b.intra for b in f.blocks())
        assert f.pkt.ncoefs > 0 and not any(ctypes.string_at(f.pkt.coefs, f.nbytes_coefs))
        assert all(b.mv[k] == 0 for b in f.blocks() for k in range(16))
        # inner transform edges: non-skip blocks above 8x8 whose transform is smaller than they
        assert any(not b.skip and b.bs < synth_walk.BS_8x8 and 1 << b.tx < 2 * min(synth_walk.BWH8[b.bs])
                   for b in f.blocks()) and any(b.skip for b in f.blocks())
        assert bytes(f.pkt.lflvl) == bytes([level]) * 64 and f.pkt.sharpness == sharp
        for k in range(64):
            f.pkt.lflvl[k] = 0
        f.pkt.filter_level = 0
        out = v9.alloc_planes(w, h, bd, ssh, ssv)
        orc.decode_frame(f.pkt, out, [pic, pic, pic])
        for a, b in zip(v9.visible(out, w, h, ssh, ssv), v9.visible(pic, w, h, ssh, ssv)):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("group", lf_cases.GROUPS, ids=_gid)
def test_group_meets_the_conditions(v9, orc, group):
    res = lf_cases.group_oracle(v9, orc, group)
    count, moved, tight = lf_cases.check_group(orc, group, [c for _, _, _, c in res])
    print("census %s\ncount %s\nmoved %s\ntight %s" % (group, count.tolist(), moved.tolist(), tight.tolist()))


def test_unreachable_cells_are_only_the_two_kinds():
    for group in lf_cases.GROUPS:
        E, I, H = lf_reference.limits(group[0], group[1], group[2])
        cells = lf_cases.unreachable(group)
        assert all(arm == "h4" for _, arm, _ in cells)        # these sizes hold a 16x16 chroma transform
        assert bool(cells) == (I <= H)
    assert [g[:2] for g in lf_cases.GROUPS if lf_cases.unreachable(g)] == [(63, 7)] * 3


@pytest.mark.parametrize("bd", [8, 10])
def test_natural_set_covers_every_level(v9, orc, bd):
    keys, res = lf_cases.natural_oracle(v9, orc, bd)
    frames = [(f, k) for f, k, _, _ in res]
    assert len(frames) == 24 and sum(k for _, k in frames) == 8
    for f, is_key in frames:
        lv = bytes(f.pkt.lflvl)
        assert len(set(lv)) == 8 if is_key else len({lv[s * 8 + 2 + k] for s in range(8) for k in range(6)}) == 48
    assert sorted({f.pkt.sharpness for f, _ in frames}) == list(range(8))
    lf_cases.check_natural_levels(frames)
    for i, (f, is_key, out, c) in enumerate(res):
        assert c.moved.sum() > 0, "frame %d has no line the filter moved" % i
