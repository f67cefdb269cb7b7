"""Accumulated propagation: a numpy restatement of the definition in include/vp9hip.h
("accumulated propagation"), sharing no code with the library, against vp9hip_acc_propagate_host
(CPU suite).

prop_ref / prop_stats / hand_cases below are what tests/test_gpu_acc_propagate.py compares the
kernels with. The coordinates are int64, the bilinear step is np.float32 operations in the stated
order and .astype(np.float16). Hand-made fields on a 40 x 24 picture (a 10 x 6 grid of cells) pin
every phase 0..15 on both axes, the clamps at the four edges, the rounding of negative vectors,
the clamp of the vectors, the rule that decides whether a cell applies (S = 0 included), fill and
keep at every element size, feature grids finer and coarser than the picture and 1 x 1, C of 1, 3
and 19, both layouts, the halves at the ends of their range and src_index. All comparisons are
exact: elements are compared as bits.

Phases: with FW = w the displacement is 2 vx and shows even phases only; with FW = w / 2 it is vx
and shows all 256 pairs, which the "phases" cases cover.
"""
import re

import numpy as np
import pytest

from test_acc_warp_definition import warp_ref
from test_motion_acc_definition import CELL, INTRA, NOFIELD, SCALED

I32MAX, I32MIN = 2 ** 31 - 1, -2 ** 31
W, H, GW, GH = 40, 24, 10, 6
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def bits(a):
    """An array's elements as unsigned integers of their size: what "equal" means here."""
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def prop_coords(acc, S, w, h, FW, FH):
    """Steps 1-3 for every sample of an FW x FH grid: (applies, Px, Py), int64 (FH, FW)."""
    fy, fx = np.mgrid[0:FH, 0:FW].astype(np.int64)
    X, Y = ((2 * fx + 1) * w) // (2 * FW), ((2 * fy + 1) * h) // (2 * FH)
    assert X.max() < w and Y.max() < h
    q = acc[Y >> 2, X >> 2]
    app = (q["hops"] > 0) & (q["root"] == np.uint32(S)) & (int(S) != 0)
    vx = np.clip(q["dx"].astype(np.int64), -32768, 32767)
    vy = np.clip(q["dy"].astype(np.int64), -32768, 32767)
    return app, (4 * vx * FW + w) // (2 * w), (4 * vy * FH + h) // (2 * h)      # numpy's // floors


def prop_ref(acc, S, item, w, h, interp="nearest", fill=0, pre=None):
    """The definition for one pair: item one source item (C, FH, FW), fill a number converted to
    its dtype, pre the destination's earlier content (then VP9HIP_PROP_KEEP). Returns (the
    destination item (C, FH, FW), valid uint8 (FH, FW))."""
    C, FH, FW = item.shape
    app, Px, Py = prop_coords(acc, S, w, h, FW, FH)
    fy, fx = np.mgrid[0:FH, 0:FW].astype(np.int64)
    cx, cy = (lambda v: np.clip(v, 0, FW - 1)), (lambda v: np.clip(v, 0, FH - 1))
    if not app.any():
        g = item                                         # nothing is gathered: every element is the other one
    elif interp == "nearest":
        g = item[:, cy(fy + ((Py + 8) >> 4)), cx(fx + ((Px + 8) >> 4))]
    else:
        assert item.dtype == np.float16
        x0, y0 = fx + (Px >> 4), fy + (Py >> 4)
        frx, fry = (Px & 15).astype(np.float32), (Py & 15).astype(np.float32)
        grx, gry = np.float32(16) - frx, np.float32(16) - fry
        s00, s01 = item[:, cy(y0), cx(x0)].astype(np.float32), item[:, cy(y0), cx(x0 + 1)].astype(np.float32)
        s10, s11 = item[:, cy(y0 + 1), cx(x0)].astype(np.float32), item[:, cy(y0 + 1), cx(x0 + 1)].astype(np.float32)
        top = grx * s00 + frx * s01
        bot = grx * s10 + frx * s11
        v = (gry * top + fry * bot) * np.float32(2.0 ** -8)
        assert top.dtype == np.float32 and v.dtype == np.float32
        g = v.astype(np.float16)
    other = np.broadcast_to(np.array([fill]).astype(item.dtype), item.shape) if pre is None else pre
    out = np.where(app[None], bits(g), bits(other)).view(item.dtype)
    return out, app.astype(np.uint8)


def prop_stats(acc, S, w, h, FW, FH):
    """What a pair exercises on a grid, from the reference alone: the share of samples that apply,
    of the applying samples the share whose nearest-mode source is clamped at an edge and the
    share with both bilinear fractions non-zero, the four sides (left, right, top, bottom) at
    which a source clamps, and the (frx, fry) phases of applying samples."""
    app, Px, Py = prop_coords(acc, S, w, h, FW, FH)
    fy, fx = np.mgrid[0:FH, 0:FW].astype(np.int64)
    tx, ty = fx + ((Px + 8) >> 4), fy + ((Py + 8) >> 4)
    hit = [app & (tx < 0), app & (tx > FW - 1), app & (ty < 0), app & (ty > FH - 1)]
    n = int(app.sum())
    both = app & ((Px & 15) != 0) & ((Py & 15) != 0)
    return dict(applying=n / app.size, edge=int((hit[0] | hit[1] | hit[2] | hit[3]).sum()) / n if n else 0.0,
                both=int(both.sum()) / n if n else 0.0, sides=np.array([m.any() for m in hit]),
                phases=set(zip((Px & 15)[app].tolist(), (Py & 15)[app].tolist())))


def _acc(gw, gh, dx, dy, root, hops=1, end=INTRA):
    a = np.zeros((gh, gw), CELL)
    a["dx"], a["dy"], a["root"], a["hops"], a["end"] = dx, dy, root, hops, end
    return a


def _grid_of(w, h):
    return 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)


def _items(rng, dtype, M, C, FH, FW):
    """M random items: any bit pattern, but finite halves for float16."""
    dtype = np.dtype(dtype)
    if dtype == np.float16:
        b = rng.integers(0, 0x7c00, (M, C, FH, FW)).astype(np.uint16) | (rng.integers(0, 2, (M, C, FH, FW)).astype(np.uint16) << 15)
        return b.view(np.float16)
    return rng.integers(0, 256, (M, C, FH, FW, dtype.itemsize), dtype=np.uint8).view(dtype)[..., 0]


def _spread(rng, gw, gh, w, h):
    """A field whose vectors reach past every edge, about 3/4 of it applying to root 4."""
    dx, dy = rng.integers(-8 * w - 9, 8 * w + 9, (gh, gw)), rng.integers(-8 * h - 9, 8 * h + 9, (gh, gw))
    a = _acc(gw, gh, dx, dy, np.where(rng.random((gh, gw)) < 0.75, 4, 3))
    a["hops"][rng.random((gh, gw)) < 0.1] = 0
    return a


FILLS = {np.dtype(np.uint8): 0xa5, np.dtype(np.int16): -12345, np.dtype(np.int32): 0x12345678,
         np.dtype(np.int64): 0x123456789abcdef0, np.dtype(np.float16): 1.5, np.dtype(np.float32): -2.75,
         np.dtype(np.float64): 3.0e100}


def hand_cases():
    """The hand-made calls: dicts of name, w, h, srcs (M, C, FH, FW), pairs [(acc, S, src item)],
    interp, fill, and pre (n, C, FH, FW) where the call keeps."""
    rng = np.random.default_rng(1901)
    cells = np.arange(GW * GH).reshape(GH, GW)

    def case(name, srcs, pairs, interp="nearest", w=W, h=H, keep=False):
        pre = _items(rng, srcs.dtype, len(pairs), *srcs.shape[1:]) if keep else None
        return dict(name=name, w=w, h=h, srcs=srcs, pairs=pairs, interp=interp, fill=FILLS[srcs.dtype], pre=pre)

    # every phase: on the half grid Px = vx, so cell i of field k has (frx, fry) = the nibbles of 60 k + i
    for k in range(5):
        idx = (60 * k + cells) % 256
        dx = 16 * ((cells + k) % 7 - 3) + (idx & 15)
        dy = 16 * ((cells * 3 + k) % 7 - 3) + (idx >> 4)
        for interp in ("nearest", "bilinear"):
            yield case("phases%d-%s" % (k, interp), _items(rng, np.float16, 1, 3, H // 2, W // 2),
                       [(_acc(GW, GH, dx, dy, 5, hops=1 + k), 5, 0)], interp)
    # the named vectors, on the picture's grid, the half grid and a finer odd one
    V = np.array([-1, -8, -9, 7, 8, 32767, -32767, -32768, I32MAX, I32MIN, 0, 3], np.int64)
    for k, (fw, fh) in enumerate(((W, H), (W // 2, H // 2), (2 * W + 3, 2 * H + 1), (7, 5))):
        a = _acc(GW, GH, V[(cells + k) % 12], V[(cells // 2 + 3 * k) % 12], 9, hops=65535, end=NOFIELD)
        yield case("vectors%d-u8" % k, _items(rng, np.uint8, 1, 1, fh, fw), [(a, 9, 0)])
        yield case("vectors%d-f16" % k, _items(rng, np.float16, 1, 1, fh, fw), [(a, 9, 0)], "bilinear")
    # which cells apply: hops 0 with the root, another root, root 0 with each end code; S = 0 never applies
    a = _acc(GW, GH, 9, -5, 7, hops=2)
    a["hops"][0, :] = 0
    a["root"][1, :5] = 8
    a["root"][1, 5:], a["end"][1, 5:] = 0, NOFIELD
    a["root"][2, :5], a["end"][2, :5] = 0, SCALED
    a["root"][2, 5:], a["end"][2, 5:] = 0, INTRA
    src = _items(rng, np.int32, 1, 1, H, W)
    yield case("applies", src, [(a.copy(), s, 0) for s in (7, 8, 6, 0)])
    # fill and keep, a non-zero pattern at every element size; the grids; C of 1, 3, 19
    grids = [(W, H), (W // 2, H // 2), (7, 5), (1, 1), (2 * W + 3, 2 * H + 1)]
    dts = [np.uint8, np.int16, np.int32, np.int64, np.float16, np.float32, np.float64]
    for k, (fw, fh) in enumerate(grids):
        for j, dt in enumerate(dts):
            C = (1, 3, 19)[(k + j) % 3]
            for keep in (False, True):
                yield case("grid%dx%d-%s-c%d%s" % (fw, fh, np.dtype(dt).name, C, "-keep" if keep else ""),
                           _items(rng, dt, 1, C, fh, fw), [(_spread(rng, GW, GH, W, H), 4, 0)], keep=keep)
        C = (19, 1, 3)[k % 3]
        yield case("grid%dx%d-bilinear-c%d" % (fw, fh, C), _items(rng, np.float16, 1, C, fh, fw),
                   [(_spread(rng, GW, GH, W, H), 4, 0)], "bilinear")
        yield case("grid%dx%d-bilinear-c%d-keep" % (fw, fh, C), _items(rng, np.float16, 1, C, fh, fw),
                   [(_spread(rng, GW, GH, W, H), 4, 0)], "bilinear", keep=True)
    # an odd picture that is no multiple of the cell
    for w, h, fw, fh in ((8, 8, 5, 3), (13, 9, 13, 9), (13, 9, 6, 11)):
        gw, gh = _grid_of(w, h)
        yield case("size%dx%d-%dx%d" % (w, h, fw, fh), _items(rng, np.int16, 1, 3, fh, fw),
                   [(_spread(rng, gw, gh, w, h), 4, 0)], w=w, h=h)
    # the halves at the ends of their range: subnormals, the smallest normals, +-0, 65504, pairs that cancel
    sp = np.array([0x0001, 0x8001, 0x0002, 0x03ff, 0x0400, 0x8400, 0x0401, 0x0000, 0x8000, 0x7bff, 0xfbff, 0x7bfe,
                   0x3c00, 0xbc00, 0x3c01, 0xbc01, 0x0003, 0x8003, 0x1400, 0x9400, 0x1001, 0x5bff], np.uint16)
    for k in range(4):
        b = sp[(np.arange(H // 2 * W // 2) * (k + 1) + k * np.arange(H // 2 * W // 2) // 7) % len(sp)].reshape(1, 1, H // 2, W // 2)
        idx = (67 * k + cells * 5) % 256
        yield case("halves%d" % k, b.view(np.float16), [(_acc(GW, GH, (idx & 15) - 16 * (k & 1), idx >> 4, 2), 2, 0)], "bilinear")
    # src_index: one item for every pair, and repeats out of order
    yield case("index-one", _items(rng, np.int16, 1, 3, 5, 7), [(_spread(rng, GW, GH, W, H), 4, 0) for _ in range(3)])
    yield case("index-repeats", _items(rng, np.float16, 3, 3, 5, 7),
               [(_spread(rng, GW, GH, W, H), 4, i) for i in (2, 0, 2, 1)], "bilinear")


@pytest.fixture(scope="module")
def cases():
    return list(hand_cases())


def case_refs(c):
    """The reference of every pair of a case: [(item (C, FH, FW), valid)]."""
    return [prop_ref(acc, S, c["srcs"][i], c["w"], c["h"], c["interp"], c["fill"], None if c["pre"] is None else c["pre"][k])
            for k, (acc, S, i) in enumerate(c["pairs"])]


def test_host_equals_the_restatement_in_both_layouts(v9, cases):
    for c in cases:
        keep = c["pre"] is not None
        for k, ((acc, S, i), (want, wvalid)) in enumerate(zip(c["pairs"], case_refs(c))):
            item = c["srcs"][i]
            for layout, to, back in (("nchw", (0, 1, 2), (0, 1, 2)), ("nhwc", (1, 2, 0), (2, 0, 1))):
                src = np.ascontiguousarray(item.transpose(to))
                out = np.ascontiguousarray(c["pre"][k].transpose(to)) if keep else None
                got, gvalid = v9.acc_propagate_host(acc, S, src, c["w"], c["h"], interp=c["interp"], layout=layout, fill=c["fill"],
                                                    keep=keep, valid=True, out=out)
                assert got.dtype == item.dtype and got.shape == src.shape
                bad = bits(got.transpose(back)) != bits(want)
                assert not bad.any(), "%s pair %d %s: %d elements differ, first %s" % (
                    c["name"], k, layout, int(bad.sum()), tuple(np.argwhere(bad)[0]))
                assert gvalid.dtype == np.uint8 and np.array_equal(gvalid, wvalid), c["name"]
            if item.shape[0] == 1:                       # (FH, FW) is C = 1 and comes back 2-D
                got = v9.acc_propagate_host(acc, S, item[0], c["w"], c["h"], interp=c["interp"], fill=c["fill"],
                                            keep=keep, out=c["pre"][k][0].copy() if keep else None)
                assert got.shape == item.shape[1:] and np.array_equal(bits(got), bits(want[0]))


def test_the_cases_cover_what_they_claim(cases):
    """From the restatement alone: phases, edges, vectors, the apply rule, keep, sizes and index."""
    by = {}
    for c in cases:
        _, C, FH, FW = c["srcs"].shape
        st = [prop_stats(acc, S, c["w"], c["h"], FW, FH) for acc, S, _ in c["pairs"]]
        by.setdefault(re.match("[a-z]+", c["name"]).group(), []).append(dict(c, st=st, C=C, FW=FW, FH=FH))
    every = {(x, y) for x in range(16) for y in range(16)}
    for interp in ("nearest", "bilinear"):
        assert set().union(*[c["st"][0]["phases"] for c in by["phases"] if c["interp"] == interp]) == every
    for kind in ("phases", "vectors", "grid"):
        assert np.logical_or.reduce([c["st"][0]["sides"] for c in by[kind]]).all(), kind
    seen = set(np.concatenate([c["pairs"][0][0]["dx"].ravel() for c in by["vectors"]]).tolist())
    assert {-1, -8, -9, 7, 8, 32767, -32767, -32768, I32MAX, I32MIN} <= seen
    assert all(c["st"][0]["applying"] == 1.0 for c in by["vectors"])
    assert [round(s["applying"] * 12) for s in by["applies"][0]["st"]] == [6, 1, 0, 0]     # twelfths of the field: S = 7, 8, 6, 0
    a = by["applies"][0]["pairs"][3][0]
    assert ((a["root"] == 0) & (a["hops"] > 0)).any()                                   # S = 0 would match these
    grids = {(c["FW"], c["FH"]) for c in by["grid"]}
    assert grids == {(W, H), (W // 2, H // 2), (7, 5), (1, 1), (2 * W + 3, 2 * H + 1)}
    for keep in (False, True):
        some = [c for c in by["grid"] if (c["pre"] is not None) == keep]
        assert {c["srcs"].dtype.itemsize for c in some} == {1, 2, 4, 8} and {c["C"] for c in some} == {1, 3, 19}
        assert {c["interp"] for c in some} == {"nearest", "bilinear"}
        assert all(0 < c["st"][0]["applying"] < 1 for c in some if c["FW"] > 1)
    for c in by["grid"]:                                 # the fill is no zero pattern at any size
        f = bits(np.array([c["fill"]]).astype(c["srcs"].dtype))[0]
        assert all((int(f) >> (8 * b)) & 0xff for b in range(c["srcs"].dtype.itemsize) if c["srcs"].dtype.kind != "f") and f != 0
    h = bits(np.concatenate([c["srcs"].ravel() for c in by["halves"]]))
    assert ((h & 0x7c00) == 0).any() and (h == 0).any() and (h == 0x8000).any() and (h == 0x7bff).any() and (h == 0xfbff).any()
    sub = 0
    for c in by["halves"]:                               # results that are subnormal halves, and exact zeros from cancelling pairs
        out = bits(case_refs(c)[0][0])
        sub += int((((out & 0x7c00) == 0) & ((out & 0x3ff) != 0)).sum())
    assert sub > 20
    assert [i for _, _, i in by["index"][0]["pairs"]] == [0, 0, 0] and by["index"][0]["srcs"].shape[0] == 1
    assert [i for _, _, i in by["index"][1]["pairs"]] == [2, 0, 2, 1]


def test_pairs_that_cancel_give_zero_and_subnormals_round_to_even(v9):
    """By hand: x and -x under equal weights cancel to +0; the smallest subnormal half under
    weights 8 / 8 against zero is 2^-25, a tie that rounds to the even 0; against the next
    subnormal it is 1.5 units, a tie that rounds to the even 2."""
    a = _acc(2, 2, 8, 0, 1)                              # w = 8, FW = 4: Px = 8, frx = 8, x0 = fx
    for left, right, want in ((0x3c00, 0xbc00, 0x0000), (0x7bff, 0xfbff, 0x0000), (0x0001, 0x0000, 0x0000),
                              (0x0001, 0x0002, 0x0002), (0x0002, 0x0003, 0x0002), (0x8001, 0x8002, 0x8002),
                              (0x03ff, 0x0400, 0x0400), (0x7bff, 0x7bff, 0x7bff)):
        src = np.array([[left, right, left, right]] * 4, np.uint16).view(np.float16)
        got = v9.acc_propagate_host(a, 1, src, 8, 8, interp="bilinear")
        assert bits(got)[0, 0] == want and bits(got)[0, 2] == want, (hex(left), hex(right), hex(int(bits(got)[0, 0])))
        assert bits(prop_ref(a, 1, src[None], 8, 8, "bilinear")[0])[0, 0, 0] == want


def test_nearest_rounds_half_up_and_negative_vectors_floor(v9):
    """-1, -8, -9, 7, 8 in 1/8 luma sample on ramps: the sample each lands on, by hand."""
    for vx, full, half_grid in ((-1, 0, 0), (-8, -1, 0), (-9, -1, -1), (7, 1, 0), (8, 1, 1), (4, 1, 0), (-4, 0, 0), (-12, -1, -1)):
        assert (2 * vx + 8) >> 4 == full and (vx + 8) >> 4 == half_grid
        a = _acc(GW, GH, vx, 0, 1)
        ramp = np.arange(W, dtype=np.uint8)[None, :].repeat(H, 0)
        assert v9.acc_propagate_host(a, 1, ramp, W, H)[3, 8] == 8 + full
        ramp = np.arange(W // 2, dtype=np.int64)[None, :].repeat(H // 2, 0) * 1000003
        assert v9.acc_propagate_host(a, 1, ramp, W, H)[3, 8] == (8 + half_grid) * 1000003
        # on a ramp the bilinear value is the ramp at the displaced position: exact in halves
        ramp = np.arange(W, dtype=np.float16)[None, :].repeat(H, 0)
        assert v9.acc_propagate_host(a, 1, ramp, W, H, interp="bilinear")[3, 8] == np.float16(8 + 2 * vx / 16)
        a = _acc(GW, GH, 0, vx, 1)                       # and down a column
        ramp = np.arange(H, dtype=np.float16)[:, None].repeat(W, 1)
        assert v9.acc_propagate_host(a, 1, ramp, W, H, interp="bilinear")[8, 3] == np.float16(8 + 2 * vx / 16)


def test_the_displacement_is_the_luma_and_the_chroma_rule():
    """Px = 2 vx on the picture's grid and vx on half of an even picture, over the clamped range."""
    vx = np.concatenate([np.arange(-32768, 32768, 97), [-32768, -1, 0, 1, 32767]]).astype(np.int64)
    for w in (8, 40, 66, 16384):
        assert np.array_equal((4 * vx * w + w) // (2 * w), 2 * vx)
        assert np.array_equal((4 * vx * (w // 2) + w) // (2 * w), vx)


def _warp_planes(rng, top):
    A = [rng.integers(0, top, s).astype(np.uint16) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
    B = [rng.integers(0, top, s).astype(np.uint16) for s in ((H, W), (H // 2, W // 2), (H // 2, W // 2))]
    return A, B


def test_against_acc_warp(v9):
    """The existing function as a cross-check: with the luma plane as a C = 1, E = 2 source on the
    picture's own grid the result is the luma of acc_warp's "picture" output on every applying
    cell, and with the half grid and a chroma plane its 4:2:0 chroma."""
    rng = np.random.default_rng(77)
    for k in range(6):
        acc = _spread(rng, GW, GH, W, H)
        A, B = _warp_planes(rng, 1024)
        for p, (fw, fh) in ((0, (W, H)), (1, (W // 2, H // 2)), (2, (W // 2, H // 2))):
            pic, _ = warp_ref(A, B, acc, 4, W, H, 1, 1, "nearest", "picture")
            want = pic[p].view(np.uint16)
            got, valid = v9.acc_propagate_host(acc, 4, B[p], W, H, fill=0xffff, valid=True)
            assert 0 < valid.mean() < 1
            assert np.array_equal(got[valid == 1], want[valid == 1]) and (got[valid == 0] == 0xffff).all()
            kept = v9.acc_propagate_host(acc, 4, B[p], W, H, keep=True, out=A[p].copy())     # keep: acc_warp's picture itself
            assert np.array_equal(kept, want)
        # bilinear, on integer-valued halves <= 2047: equal wherever the integer formula is exact
        A, B = _warp_planes(rng, 2048)
        pic, _ = warp_ref(A, B, acc, 4, W, H, 1, 1, "bilinear", "picture")
        exact_n = 0
        for p, (fw, fh) in ((0, (W, H)), (1, (W // 2, H // 2))):
            b = B[p].astype(np.int64)
            app, Px, Py = prop_coords(acc, 4, W, H, fw, fh)
            fy, fx = np.mgrid[0:fh, 0:fw].astype(np.int64)
            x0, y0, frx, fry = fx + (Px >> 4), fy + (Py >> 4), Px & 15, Py & 15
            cx, cy = (lambda v: np.clip(v, 0, fw - 1)), (lambda v: np.clip(v, 0, fh - 1))
            total = ((16 - fry) * ((16 - frx) * b[cy(y0), cx(x0)] + frx * b[cy(y0), cx(x0 + 1)]) +
                     fry * ((16 - frx) * b[cy(y0 + 1), cx(x0)] + frx * b[cy(y0 + 1), cx(x0 + 1)]))
            exact = app & (total % 256 == 0)
            got = v9.acc_propagate_host(acc, 4, B[p].astype(np.float16), W, H, interp="bilinear")
            assert np.array_equal(got[exact].astype(np.int64), pic[p].view(np.uint16)[exact].astype(np.int64))
            exact_n += int(exact.sum())
        assert exact_n > 20


def test_bad_arguments(v9):
    L = v9.lib()
    rng = np.random.default_rng(5)
    acc, src = _acc(GW, GH, 0, 0, 1), _items(rng, np.int16, 1, 3, 5, 7)[0]
    for kw in (dict(interp="cubic"), dict(layout="chwn")):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.acc_propagate_host(acc, 1, src, W, H, **kw)
        assert e.value.code == v9.EINVAL
    with pytest.raises(ValueError):
        v9.acc_propagate_host(acc, 1, src, W, H, interp="bilinear")          # int16 is not binary16
    with pytest.raises(ValueError):
        v9.acc_propagate_host(acc, 1, src, W, H, keep=True)
    with pytest.raises(ValueError):
        v9.acc_propagate_host(acc[:, :5], 1, src, W, H)
    import ctypes
    good = dict(width=W, height=H, fw=7, fh=5, channels=3, elem_size=2, layout=0, mode=0, flags=0, reserved=0, fill=0)
    assert v9.prop_layout(v9.PropDesc(**good)) == (7 * 5 * 3 * 2, 35)
    assert v9.prop_layout(v9.PropDesc(**dict(good, fw=16384, fh=16384, channels=4096, elem_size=8)))[0] == 2 ** 43
    out = np.full(7 * 5 * 3, 0x5a5a, np.int16)
    bad = [dict(width=0), dict(height=16385), dict(fw=0), dict(fh=16385), dict(channels=0), dict(channels=4097), dict(elem_size=3),
           dict(elem_size=16), dict(layout=2), dict(mode=2), dict(mode=1, elem_size=4), dict(flags=2), dict(reserved=1)]
    for kw in bad:
        d = v9.PropDesc(**dict(good, **kw))
        assert L.vp9hip_prop_layout(ctypes.byref(d), None) == v9.EINVAL, kw
        assert L.vp9hip_acc_propagate_host(acc.ctypes.data, 1, ctypes.byref(d), src.ctypes.data, out.ctypes.data, None) == v9.EINVAL
    d = v9.PropDesc(**good)
    assert L.vp9hip_prop_layout(None, None) == v9.EINVAL
    for args in ((None, 1, ctypes.byref(d), src.ctypes.data, out.ctypes.data), (acc.ctypes.data, 1, None, src.ctypes.data, out.ctypes.data),
                 (acc.ctypes.data, 1, ctypes.byref(d), None, out.ctypes.data), (acc.ctypes.data, 1, ctypes.byref(d), src.ctypes.data, None)):
        assert L.vp9hip_acc_propagate_host(*args, None) == v9.EINVAL
    assert (out == 0x5a5a).all()
    assert ctypes.sizeof(v9.PropDesc) == 48 and v9.PropDesc.fill.offset == 40
    assert v9.PROP_LAYOUTS == {"nchw": 0, "nhwc": 1} and v9.PROP_KEEP == 1 and v9.ABI_VERSION == 5
    for s in ("vp9hip_prop_layout", "vp9hip_acc_propagate", "vp9hip_acc_propagate_host", "vp9hip_prop_launch_dev",
              "vp9hip_decoder_acc_propagate"):
        assert s in v9.ABI_SYMBOLS and hasattr(L, s)
