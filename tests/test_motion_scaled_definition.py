"""Motion tensors at model size: the host statement (vp9hip_motion_scaled_host,
csrc/host/vp9h_motion_scaled.c) against a numpy restatement of the definition in
include/vp9hip.h ("motion tensors at model size"), and the properties the definition promises
checked on the restatement alone. CPU only; every comparison is exact, halves by bit pattern.

The restatement goes the long way round and shares no code with the cell-weight form the
library sums over: every cell's value and flag, expanded to its 4 x 4 pixels with np.repeat,
cropped to w x h, then the signed box of test_residual_scaled_definition (weight matrices over
pixels, Python's floor division). The half is float32(x) * float32(k) rounded to float16 by numpy.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_convert_scale import RATIOS
from test_residual_scaled_definition import bits, same, sbox

SIZES = RATIOS + [((8, 8), (1, 1)), ((66, 34), (33, 17)), ((130, 200), (224, 224))]
SOURCES = ["coded", "acc"]
FORMATS = ["i16", "f16"]
CELL = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("root", "<u4"), ("hops", "<u2"), ("end", "u1"), ("pad", "u1")])


# ------------------------------------------------------------------ the restatement
def grid(w, h):
    return 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)


def cell_values(source, mv=None, info=None, acc=None):
    """(vx, vy, 256 has) per cell, int64."""
    if source == "coded":
        has = np.asarray(info)[..., 0] != 255
        vx, vy = np.asarray(mv)[..., 0, 0].astype(np.int64), np.asarray(mv)[..., 0, 1].astype(np.int64)
    else:
        has = np.asarray(acc)["hops"] > 0
        vx = np.clip(np.asarray(acc)["dx"].astype(np.int64), -32768, 32767)
        vy = np.clip(np.asarray(acc)["dy"].astype(np.int64), -32768, 32767)
    return np.where(has, vx, 0), np.where(has, vy, 0), np.where(has, 256, 0).astype(np.int64)


def dense(cells, w, h):
    """F: every cell spread over its 4 x 4 pixels, cropped to the visible size."""
    return np.repeat(np.repeat(cells, 4, axis=0), 4, axis=1)[:h, :w]


def ref_tensor(w, h, fmt, ow, oh, source, mv=None, info=None, acc=None, mask=False, n=None):
    """The (2 or 3, OH, OW) tensor of one frame. n: (nw, nh) taken for the picture size instead of
    (w, h), the mistakes the GPU tests must be able to see."""
    planes = cell_values(source, mv, info, acc)[:3 if mask else 2]
    nw, nh = n or (w, h)
    out = np.stack([sbox(dense(p, nw, nh), ow, oh) for p in planes])
    if fmt == "f16":
        k = [np.float32(ow / (8.0 * w)), np.float32(oh / (8.0 * h)), np.float32(1.0 / 256)][:len(planes)]
        with np.errstate(over="ignore"):
            return np.stack([(p.astype(np.float32) * kk).astype(np.float16) for p, kk in zip(out, k)])
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)


def random_coded(rng, w, h, lo=-32768, hi=32767, intra=0.25):
    """mv, info of the grid of w x h: a quarter intra cells with stale vectors under them, a
    quarter compound cells, every second vector poison."""
    gw, gh = grid(w, h)
    mv = rng.integers(lo, hi + 1, (gh, gw, 2, 2)).astype(np.int16)
    mv[:, :, 1] = rng.choice(np.array([0x7fff, -0x8000], np.int16), (gh, gw, 2))
    info = rng.integers(0, 3, (gh, gw, 4)).astype(np.uint8)
    info[..., 0][rng.random((gh, gw)) < intra] = 255
    info[..., 1][rng.random((gh, gw)) < 0.75] = 255
    return mv, info


def random_acc(rng, w, h, lo=-40000, hi=40000, intra=0.25):
    """acc records of the grid of w x h: sums beyond int16 on both sides, a quarter of the cells
    with no hops and stale sums under them."""
    gw, gh = grid(w, h)
    a = np.zeros((gh, gw), CELL)
    a["dx"], a["dy"] = rng.integers(lo, hi + 1, (gh, gw)), rng.integers(lo, hi + 1, (gh, gw))
    a["root"], a["end"] = rng.integers(0, 1 << 32, (gh, gw)), rng.integers(0, 3, (gh, gw))
    a["hops"] = np.where(rng.random((gh, gw)) < intra, 0, rng.integers(1, 65536, (gh, gw)))
    return a


def random_source(rng, source, w, h):
    if source == "coded":
        mv, info = random_coded(rng, w, h)
        return dict(mv=mv, info=info)
    return dict(acc=random_acc(rng, w, h))


# ------------------------------------------------------------------ the restatement alone
def test_restatement_properties():
    rng = np.random.default_rng(171)
    for w, h in ((65, 33), (66, 34), (16, 16), (130, 200)):
        for source in SOURCES:
            src = random_source(rng, source, w, h)
            vx, vy, cov = cell_values(source, **src)
            # identity at resize == size: the dense field itself
            got = ref_tensor(w, h, "i16", w, h, source, mask=True, **src)
            for p, c in zip(got, (vx, vy, cov)):
                assert np.array_equal(p, dense(c, w, h))
    # w and h multiples of 4, one output per cell: the cell values
    w, h = 64, 40
    for source in SOURCES:
        src = random_source(rng, source, w, h)
        vx, vy, cov = cell_values(source, **src)
        got = ref_tensor(w, h, "i16", w // 4, h // 4, source, mask=True, **src)
        for p, c in zip(got, (vx, vy, cov)):
            assert np.array_equal(p, c[:h // 4, :w // 4])
    # a constant field stays constant; the coverage of all-intra and all-inter fields
    for (w, h), (ow, oh) in ((65, 33), (7, 5)), ((130, 200), (224, 224)), ((16, 16), (1, 1)):
        gw, gh = grid(w, h)
        for c in (-32768, -1234, -1, 0, 5, 32767):
            mv, info = np.zeros((gh, gw, 2, 2), np.int16), np.zeros((gh, gw, 4), np.uint8)
            mv[:, :, 0, 0], mv[:, :, 0, 1] = c, -1 - c
            got = ref_tensor(w, h, "i16", ow, oh, "coded", mv=mv, info=info, mask=True)
            assert (got[0] == c).all() and (got[1] == -1 - c).all() and (got[2] == 256).all()
            info[..., 0] = 255
            got = ref_tensor(w, h, "i16", ow, oh, "coded", mv=mv, info=info, mask=True)
            assert (got == 0).all()
            acc = np.zeros((gh, gw), CELL)
            acc["dx"], acc["dy"], acc["hops"] = c, -1 - c, 1
            got = ref_tensor(w, h, "i16", ow, oh, "acc", acc=acc, mask=True)
            assert (got[0] == c).all() and (got[1] == -1 - c).all() and (got[2] == 256).all()
            acc["hops"] = 0
            assert (ref_tensor(w, h, "i16", ow, oh, "acc", acc=acc, mask=True) == 0).all()


def test_aggregated_weight_is_the_sum_over_the_cells_pixels():
    """W(o, c) of the definition against the box weights summed over a cell's four columns, and
    the weights of one output summing to n."""
    from test_gpu_convert_scale import _weights
    for n, on in ((65, 33), (66, 33), (33, 7), (16, 40), (8, 1), (130, 224), (200, 224), (352, 3), (1, 1), (3, 9)):
        gc = 2 * ((n + 7) >> 3)
        px = np.zeros((on, 4 * gc), np.int64)
        px[:, :n] = _weights(n, on)
        o, c = np.arange(on, dtype=np.int64)[:, None], np.arange(gc, dtype=np.int64)[None, :]
        W = np.maximum(0, np.minimum((o + 1) * n, (4 * c + 4) * on) - np.maximum(o * n, 4 * c * on))
        assert np.array_equal(W, px.reshape(on, gc, 4).sum(axis=2)), (n, on)
        assert (W.sum(axis=1) == n).all()


# ------------------------------------------------------------------ the host statement against it
@pytest.mark.parametrize("source", SOURCES)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d-%dx%d" % (s[0] + s[1]))
def test_host_matches_the_restatement(v9, size, source):
    (w, h), (ow, oh) = size
    rng = np.random.default_rng(1700 + 7 * w + ow + (source == "acc"))
    src = random_source(rng, source, w, h)
    for fmt in FORMATS:
        for mask in (False, True):
            got = v9.motion_scaled_host(src.get("mv"), src.get("info"), w, h, fmt, (ow, oh), source=source,
                                        acc=src.get("acc"), mask=mask)
            same(got, ref_tensor(w, h, fmt, ow, oh, source, mask=mask, **src), "%s %s mask %d" % (source, fmt, mask))
    got = v9.motion_scaled_host(src.get("mv"), src.get("info"), w, h, "i16", None, source=source, acc=src.get("acc"), mask=True)
    same(got, ref_tensor(w, h, "i16", w, h, source, mask=True, **src), "%s own size" % source)


def test_host_strided_inputs(v9):
    """Fields inside larger planes, as the device holds them: what lies beyond the grid is poison."""
    w, h, ow, oh = 66, 34, 33, 17
    gw, gh = grid(w, h)
    rng = np.random.default_rng(172)
    mv, info = random_coded(rng, w, h)
    acc = random_acc(rng, w, h)
    big_mv, big_info = np.full((gh + 3, 50, 2, 2), 0x7fff, np.int16), np.full((gh + 3, 50, 4), 7, np.uint8)
    big_acc = np.zeros((gh + 3, 50), CELL)
    big_acc["dx"], big_acc["dy"], big_acc["hops"] = 0x7fffffff, -0x80000000, 9
    big_mv[:gh, :gw], big_info[:gh, :gw], big_acc[:gh, :gw] = mv, info, acc
    for fmt in FORMATS:
        got = v9.motion_scaled_host(big_mv[:gh, :gw], big_info[:gh, :gw], w, h, fmt, (ow, oh), mask=True)
        same(got, ref_tensor(w, h, fmt, ow, oh, "coded", mv=mv, info=info, mask=True), "coded strided " + fmt)
        got = v9.motion_scaled_host(None, None, w, h, fmt, (ow, oh), source="acc", acc=big_acc[:gh, :gw], mask=True)
        same(got, ref_tensor(w, h, fmt, ow, oh, "acc", acc=acc, mask=True), "acc strided " + fmt)


def test_host_chosen_cells(v9):
    """A compound cell with a poisoned second vector, stale vectors under intra cells, info[0]
    of 3..254 (has = 1), acc records at the int32 ends and at +-40000, hops 0 with nonzero dx."""
    w = h = 16
    mv, info = np.zeros((4, 4, 2, 2), np.int16), np.zeros((4, 4, 4), np.uint8)
    mv[:, :, 0, 0] = np.arange(16).reshape(4, 4) * 1000 - 8000
    mv[:, :, 0, 1] = 77 - np.arange(16).reshape(4, 4) * 900
    mv[:, :, 1] = 0x7fff                                    # every second vector poison
    info[..., 1] = 1                                        # compound everywhere
    info[0, :, 0] = (3, 100, 254, 255)                      # has = 1, 1, 1, 0
    info[1, 1, 0] = 255
    for (ow, oh) in ((16, 16), (4, 4), (1, 1), (3, 5)):
        for fmt in FORMATS:
            got = v9.motion_scaled_host(mv, info, w, h, fmt, (ow, oh), mask=True)
            same(got, ref_tensor(w, h, fmt, ow, oh, "coded", mv=mv, info=info, mask=True), "coded %dx%d %s" % (ow, oh, fmt))
    got = v9.motion_scaled_host(mv, info, w, h, "i16", (4, 4), mask=True)
    assert got[2, 0].tolist() == [256, 256, 256, 0] and got[0, 0, 3] == 0 and got[0, 1, 1] == 0
    assert got[0, 0, :3].tolist() == mv[0, :3, 0, 0].tolist()
    acc = np.zeros((4, 4), CELL)
    acc["hops"] = 1
    acc["dx"] = [[0x7fffffff, -0x80000000, 40000, -40000], [32767, -32768, 32768, -32769], [1, -1, 0, 5], [9, 9, 9, 9]]
    acc["dy"] = acc["dx"].T
    acc["hops"][3] = (0, 0, 65535, 2)                       # hops 0 over dx = 9: no vector, no coverage
    for (ow, oh) in ((16, 16), (4, 4), (1, 1), (3, 5)):
        for fmt in FORMATS:
            got = v9.motion_scaled_host(None, None, w, h, fmt, (ow, oh), source="acc", acc=acc, mask=True)
            same(got, ref_tensor(w, h, fmt, ow, oh, "acc", acc=acc, mask=True), "acc %dx%d %s" % (ow, oh, fmt))
    got = v9.motion_scaled_host(None, None, w, h, "i16", (4, 4), source="acc", acc=acc, mask=True)
    assert got[0, 0].tolist() == [32767, -32768, 32767, -32768] and got[0, 1].tolist() == [32767, -32768, 32767, -32768]
    assert got[0, 3].tolist() == [0, 0, 9, 9] and got[2, 3].tolist() == [0, 0, 256, 256]


def test_host_half_overflows_to_inf(v9):
    """16 x 16 -> 16384 x 1 with every vector 32767: kx = 128, the product 4194176 is beyond the
    half range and rounds to +inf; -32768 to -inf; y (ky = 1 / 128) stays finite."""
    w = h = 16
    for v, want in ((32767, 0x7c00), (-32768, 0xfc00)):
        mv, info = np.full((4, 4, 2, 2), v, np.int16), np.zeros((4, 4, 4), np.uint8)
        got = v9.motion_scaled_host(mv, info, w, h, "f16", (16384, 1), mask=True)
        assert got.shape == (3, 1, 16384)
        assert (got[0].view(np.uint16) == want).all()
        assert (got[1] == np.float16(np.float32(v) * np.float32(1 / 128.0))).all() and (got[2] == 1).all()
        same(got, ref_tensor(w, h, "f16", 16384, 1, "coded", mv=mv, info=info, mask=True), "inf")


def test_layout_and_every_einval(v9):
    L = v9.lib()
    w, h, ow, oh = 66, 34, 20, 12
    good = dict(format=0, source=0, planes=3, width=w, height=h, out_width=ow, out_height=oh, pitch=0, frame_stride=0)

    def layout(**kw):
        d = v9.MvtDesc(**dict(good, **kw))
        p = ctypes.c_int64(-1)
        return L.vp9hip_mvt_layout(ctypes.byref(d), ctypes.byref(p)), p.value
    assert layout() == (3 * 2 * ow * oh, 2 * ow)
    assert layout(planes=2) == (2 * 2 * ow * oh, 2 * ow)
    assert layout(pitch=48, frame_stride=3 * 48 * oh + 2) == (3 * 48 * oh, 48)
    assert layout(format=1, source=1, width=16384, height=16384, out_width=16384, out_height=16384)[0] == 3 * 2 * 16384 * 16384
    assert L.vp9hip_mvt_layout(None, None) == v9.EINVAL
    bad = [dict(format=-1), dict(format=2), dict(source=-1), dict(source=2), dict(planes=1), dict(planes=4), dict(width=0),
           dict(width=16385), dict(height=0), dict(height=16385), dict(out_width=0), dict(out_width=16385),
           dict(out_height=0), dict(out_height=16385), dict(pitch=2 * ow - 2), dict(pitch=2 * ow + 2), dict(pitch=-16),
           dict(frame_stride=3 * 2 * ow * oh - 2), dict(frame_stride=3 * 2 * ow * oh + 1), dict(frame_stride=-2)]
    for kw in bad:
        assert layout(**kw)[0] == v9.EINVAL, kw
    rng = np.random.default_rng(173)
    mv, info = random_coded(rng, w, h)
    acc = random_acc(rng, w, h)
    gw, gh = grid(w, h)
    out = np.full(3 * oh * ow + 1, 0x5a5a, np.int16)

    def host(mv=mv, info=info, acc=acc, cells=gw, dst=out.ctypes.data, desc=True, **kw):
        d = v9.MvtDesc(**dict(good, **kw))
        ptr = lambda a: None if a is None else a.ctypes.data
        return L.vp9hip_motion_scaled_host(ptr(mv), ptr(info), ptr(acc), cells, ctypes.byref(d) if desc else None, dst)
    for kw in bad:
        assert host(**kw) == v9.EINVAL, kw
    assert host(mv=None) == v9.EINVAL and host(info=None) == v9.EINVAL and host(acc=None, source=1) == v9.EINVAL
    assert host(dst=None) == v9.EINVAL and host(dst=out.ctypes.data + 1) == v9.EINVAL and host(desc=False) == v9.EINVAL
    assert host(cells=(w + 3) // 4 - 1) == v9.EINVAL and host(cells=0) == v9.EINVAL and host(cells=-gw) == v9.EINVAL
    assert (out == 0x5a5a).all()                            # a refused call writes nothing
    assert host(acc=None) == 0 and host(mv=None, info=None, source=1) == 0      # the other source's arrays may be NULL
    assert out[-1] == 0x5a5a and not (out[:-1] == 0x5a5a).all()
    # the wrapper: what the library refuses reaches it, what numpy cannot express is a ValueError
    for kw in (dict(resize=(0, 5)), dict(resize=(5, 16385)), dict(width=0), dict(height=16385)):
        a = dict(dict(mv=mv, info=info, width=w, height=h, fmt="i16", resize=(ow, oh)), **kw)
        with pytest.raises(v9.Vp9HipError) as e:
            v9.motion_scaled_host(**a)
        assert e.value.code == v9.EINVAL
    with pytest.raises(ValueError):
        v9.motion_scaled_host(mv[:, :5], info, w, h, "i16", (ow, oh))
    with pytest.raises(ValueError):
        v9.motion_scaled_host(mv, info, w, h, "i16", (ow, oh), source="acc")
    with pytest.raises(KeyError):
        v9.motion_scaled_host(mv, info, w, h, "i32", (ow, oh))
    assert v9.MVT_FORMATS == {"i16": 0, "f16": 1} and v9.MVT_SOURCES == {"coded": 0, "acc": 1}
    assert v9.ACC_CELL == CELL
    for s in ("vp9hip_mvt_layout", "vp9hip_motion_frames_scaled", "vp9hip_motion_scaled_host", "vp9hip_decoder_motion_scaled"):
        assert s in v9.ABI_SYMBOLS and hasattr(L, s)
    assert v9.ABI_VERSION == 5
