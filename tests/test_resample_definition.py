"""The definitions behind vp9hip_convert_frames_resampled (include/vp9hip.h, DESIGN.md
"Resampling: triangle filter, source regions, letterbox"): a numpy restatement that shares no
code with the library, its promised properties, torch's antialiased bilinear filter as an
outside witness, the library's own statement (vp9hip_resample_weights), the bound, and
letterbox_rect. CPU only; tests/test_gpu_convert_resample.py imports the restatement.

The restatement: weight matrices W[o, s] per axis,
  box:      max(0, min((o+1) n_src, (s+1) n_out) - max(o n_src, s n_out))
  triangle: max(0, 2 max(n_src, n_out) - |(2o+1) n_src - (2s+1) n_out|)
A = Wy @ P @ Wx.T in int64, D = (rows' sums of Wy) x (rows' sums of Wx),
result = (A + (D >> 1)) // D. A source rectangle is the sub-plane; a destination rectangle is
where the result is pasted into a plane of fill codes.
"""
import numpy as np
import pytest

PAIRS = [(65, 33), (33, 7), (16, 40), (288, 224), (352, 1), (7, 7), (17, 16), (1, 5), (5, 1)]
FILTERS = ("box", "triangle")


# ------------------------------------------------------------------ the restatement
def weights(filt, n_src, n_out):
    """W[o, s], int64."""
    o, s = np.arange(n_out, dtype=np.int64)[:, None], np.arange(n_src, dtype=np.int64)[None, :]
    if filt == "box":
        return np.maximum(0, np.minimum((o + 1) * n_src, (s + 1) * n_out) - np.maximum(o * n_src, s * n_out))
    assert filt == "triangle"
    return np.maximum(0, 2 * max(n_src, n_out) - np.abs((2 * o + 1) * n_src - (2 * s + 1) * n_out))


def sums(P, ow, oh, filt):
    """(A, D) of plane P resampled to ow x oh, int64."""
    h, w = P.shape
    Wy, Wx = weights(filt, h, oh), weights(filt, w, ow)
    return Wy @ P.astype(np.int64) @ Wx.T, Wy.sum(axis=1)[:, None] * Wx.sum(axis=1)[None, :]


def resample(P, ow, oh, filt):
    A, D = sums(P, ow, oh, filt)
    return (A + (D >> 1)) // D


def chroma_rect(r, ssh, ssv):
    x, y, w, h = r
    return x >> ssh, y >> ssv, (w + ssh) >> ssh, (h + ssv) >> ssv


def _sub(P, r):
    x, y, w, h = r
    return P[y:y + h, x:x + w]


def _paste(shape, fill, r, pic):
    out = np.full(shape, fill, np.int64)
    x, y, w, h = r
    assert pic.shape == (h, w)
    out[y:y + h, x:x + w] = pic
    return out


def resampled_planes(planes, OW, OH, filt, ssh, ssv, src=None, dst=None, fill=(0, 0, 0)):
    """(the semi-planar output's planes, the RGB formats' planes before the conversion) of one
    frame: src / dst in luma samples, None = the whole picture / the whole output."""
    h, w = planes[0].shape
    src = (0, 0, w, h) if src is None else src
    dst = (0, 0, OW, OH) if dst is None else dst
    csrc, cdst = chroma_rect(src, ssh, ssv), chroma_rect(dst, ssh, ssv)
    Y, U, V = _sub(planes[0], src), _sub(planes[1], csrc), _sub(planes[2], csrc)
    y = _paste((OH, OW), fill[0], dst, resample(Y, dst[2], dst[3], filt))
    ocw, och = (OW + ssh) >> ssh, (OH + ssv) >> ssv
    semi = [y] + [_paste((och, ocw), fill[1 + i], cdst, resample(C, cdst[2], cdst[3], filt)) for i, C in enumerate((U, V))]
    full = [y] + [_paste((OH, OW), fill[1 + i], dst, resample(C, dst[2], dst[3], filt)) for i, C in enumerate((U, V))]
    return semi, full


def default_fill(d, cs, full):
    return (0, 0, 0) if cs == 7 else (0 if full else 16 << (d - 8), 1 << (d - 1), 1 << (d - 1))


def letterbox(w, h, OW, OH, align=(1, 1)):
    if w * OH >= h * OW:
        dw, dh = OW, max(1, (h * OW + w // 2) // w)
    else:
        dw, dh = max(1, (w * OH + h // 2) // h), OH
    return (OW - dw) // 2 // align[0] * align[0], (OH - dh) // 2 // align[1] * align[1], dw, dh


def max_d(filt, n_src, n_out):
    return int(weights(filt, n_src, n_out).sum(axis=1).max())


def within_bound(filt, w, h, ow, oh, d):
    """The call's bound for one plane geometry, in Python's unbounded integers."""
    return max_d(filt, w, ow) * max_d(filt, h, oh) * ((1 << d) - 1) < 1 << 63


# ------------------------------------------------------------------ what the definition promises
@pytest.mark.parametrize("n_src,n_out", PAIRS)
def test_triangle_weights(n_src, n_out):
    W = weights("triangle", n_src, n_out)
    assert (W.sum(axis=1) > 0).all()
    assert (W.max(axis=1) >= max(n_src, n_out)).all()             # the nearest sample
    assert np.array_equal(W, W[::-1, ::-1])                       # flip symmetry
    if n_out >= n_src:                                            # upscale / identity: bilinear
        taps = (W > 0).sum(axis=1)
        assert taps.max() <= 2
        inner = (W[:, 0] == 0) & (W[:, -1] == 0) if n_src > 1 else np.zeros(n_out, bool)
        both = taps == 2
        assert (W.sum(axis=1)[both] == 2 * n_out).all()
        assert (W.sum(axis=1)[inner] == 2 * n_out).all()
    if n_src == n_out:
        assert np.array_equal(W, 2 * n_src * np.eye(n_src, dtype=np.int64))


@pytest.mark.parametrize("n_src,n_out", PAIRS)
def test_box_weights(n_src, n_out):
    W = weights("box", n_src, n_out)
    assert (W.sum(axis=1) == n_src).all() and (W.sum(axis=0) == n_out).all()


def test_identity_constant_and_rounding():
    rng = np.random.default_rng(1)
    P = rng.integers(0, 4096, (33, 65))
    for filt in FILTERS:
        assert np.array_equal(resample(P, 65, 33, filt), P)
        for ow, oh in ((7, 5), (130, 40), (1, 1), (64, 33)):
            assert (resample(np.full((33, 65), 1234), ow, oh, filt) == 1234).all()
    # 2:1 triangle: weights 1, 3, 3, 1 (x n_out) per axis away from the edge
    assert list(weights("triangle", 16, 8)[3, 5:9]) == [8, 24, 24, 8]
    # one output from 2 x 2: every weight equal, D = 4 w^2: 10 / 4 rounds up, 9 / 4 down
    assert resample(np.array([[1, 2], [3, 4]]), 1, 1, "triangle")[0, 0] == 3
    assert resample(np.array([[1, 2], [3, 3]]), 1, 1, "triangle")[0, 0] == 2


@pytest.mark.parametrize("size,out", [((65, 33), (33, 17)), ((352, 288), (224, 224)), ((16, 16), (40, 23)),
                                      ((352, 288), (3, 2))])
def test_triangle_is_torchs_antialiased_bilinear(size, out):
    import torch
    (w, h), (ow, oh) = size, out
    P = np.random.default_rng(w + ow).integers(0, 256, (h, w))
    t = torch.from_numpy(P.astype(np.float64))[None, None]
    ref = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bilinear", antialias=True, align_corners=False)[0, 0].numpy()
    err = np.abs(resample(P, ow, oh, "triangle") - ref).max()
    print("%dx%d -> %dx%d: max |tri - interpolate| = %.6f" % (w, h, ow, oh, err))
    assert err <= 0.5 + 1e-6


# ------------------------------------------------------------------ the library's statement of it
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("n_src,n_out", PAIRS)
def test_library_weights_match(v9, filt, n_src, n_out):
    W = weights(filt, n_src, n_out)
    for o in range(n_out):
        first, w, d = v9.resample_weights(filt, n_src, n_out, o)
        row = np.zeros(n_src, np.int64)
        row[first:first + len(w)] = w
        assert min(w) > 0 and np.array_equal(row, W[o]), (filt, n_src, n_out, o)
        assert d == W[o].sum()
        if filt == "box":
            assert d == n_src


def test_library_weights_arguments(v9):
    import ctypes
    L = v9.lib()
    for args in ((2, 8, 4, 0), (0, 0, 4, 0), (1, 8, 0, 0), (1, 8, 4, 4), (1, 8, 4, -1), (1, 16385, 4, 0), (0, 4, 16385, 0)):
        assert L.vp9hip_resample_weights(*args, None, None, 0, None) == v9.EINVAL, args
    assert L.vp9hip_resample_weights(1, 8, 4, 0, None, None, -1, None) == v9.EINVAL
    w, d = (ctypes.c_int32 * 2)(), ctypes.c_int64()       # cap below the tap count: the count and sum are whole
    assert L.vp9hip_resample_weights(1, 16, 8, 3, None, w, 2, ctypes.byref(d)) == 4 and list(w) == [8, 24] and d.value == 64
    assert v9.FILTERS == {"box": 0, "triangle": 1}
    assert ctypes.sizeof(v9.Rect) == 16 and ctypes.sizeof(v9.Resample) == 48


# ------------------------------------------------------------------ the bound
def test_the_bound():
    assert not within_bound("triangle", 7680, 4320, 1, 1, 12)
    assert within_bound("triangle", 7680, 4320, 2, 2, 12)
    assert within_bound("triangle", 7680, 4320, 1, 1, 8)
    assert max_d("triangle", 1088, 1) * 4095 > 1 << 32             # where column sums leave 32 bits
    n = 4320
    assert abs(max_d("triangle", n, 1) / (1.5 * n * n) - 1) < 1e-3
    # the O(1) ceiling the runtime tries first: at most 2M / n_out + 1 taps of at most 2M each
    for n_src, n_out in PAIRS + [(7680, 1), (4320, 2), (3840, 1920)]:
        m2 = 2 * max(n_src, n_out)
        assert max_d("triangle", n_src, n_out) <= m2 * (m2 // n_out + 1)


def test_library_sums_are_the_bounds_factors(v9):
    for n_src, n_out in ((7680, 1), (4320, 2), (1088, 3)):
        assert max(v9.resample_weights("triangle", n_src, n_out, o)[2] for o in range(n_out)) == max_d("triangle", n_src, n_out)


# ------------------------------------------------------------------ letterbox_rect
@pytest.mark.parametrize("args,want", [
    ((1920, 1080, 224, 224), (0, 49, 224, 126)),
    ((1080, 1920, 224, 224), (49, 0, 126, 224)),
    ((1920, 1080, 640, 360), (0, 0, 640, 360)),          # w OH == h OW
    ((352, 288, 40, 23), (6, 0, 28, 23)),
    ((4000, 3, 40, 23), (0, 11, 40, 1)),                 # a 1-pixel result (0.03 rounds to 0: at least 1)
    ((3, 4000, 40, 23), (19, 0, 1, 23)),
    ((16, 9, 7, 7), (0, 1, 7, 4)),                       # 63 / 16 = 3.94 rounds to 4
    ((1, 1, 5, 3), (1, 0, 3, 3)),
])
def test_letterbox_rect(v9, args, want):
    assert v9.letterbox_rect(*args) == want == letterbox(*args)
    w, h, OW, OH = args
    dx, dy, dw, dh = want
    assert 0 <= dx and dx + dw <= OW and 0 <= dy and dy + dh <= OH and (dw == OW or dh == OH)


def test_letterbox_rect_alignment(v9):
    assert v9.letterbox_rect(1920, 1080, 224, 224, align=(2, 2)) == (0, 48, 224, 126)
    assert v9.letterbox_rect(1080, 1920, 224, 224, align=(2, 1)) == (48, 0, 126, 224)
    assert v9.Device.letterbox_rect(1080, 1920, 224, 224, (4, 4)) == (48, 0, 126, 224)
    with pytest.raises(ValueError):
        v9.letterbox_rect(0, 5, 8, 8)


def test_restatement_rectangles():
    """A source rectangle is the sub-plane; a destination rectangle pastes into the fill."""
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, (30, 40)), rng.integers(0, 256, (15, 20)), rng.integers(0, 256, (15, 20))]
    semi, full = resampled_planes(planes, 12, 10, "triangle", 1, 1, src=(6, 2, 21, 17), dst=(2, 4, 7, 5), fill=(9, 8, 7))
    assert semi[0].shape == (10, 12) and semi[1].shape == (5, 6) and full[2].shape == (10, 12)
    assert np.array_equal(semi[0][4:9, 2:9], resample(planes[0][2:19, 6:27], 7, 5, "triangle"))
    assert np.array_equal(semi[1][2:5, 1:5], resample(planes[1][1:10, 3:14], 4, 3, "triangle"))
    assert np.array_equal(full[2][4:9, 2:9], resample(planes[2][1:10, 3:14], 7, 5, "triangle"))
    mask = np.ones((10, 12), bool)
    mask[4:9, 2:9] = False
    assert (semi[0][mask] == 9).all() and (full[1][mask] == 8).all() and (full[2][mask] == 7).all()
