"""The definition behind vp9hip_convert_frames_bicubic (include/vp9hip.h, DESIGN.md "Resampling:
bicubic"): a numpy restatement that shares no code with the library, its promised properties,
torch's antialiased bicubic filter as an outside witness, the library's own statement
(vp9hip_bicubic_weights) and the bound. CPU only; tests/test_gpu_convert_bicubic.py imports the
restatement.

The restatement, in Python's unbounded integers (object arrays): per axis, M = max(n_src, n_out),
T = 2M, Q = 14,
  u = |(2o+1) n_src - (2s+1) n_out|, present iff u < 2T
  c = 3u^3 - 5T u^2 + 2T^3 (u < T), -u^3 + 5T u^2 - 8T^2 u + 4T^3 (T <= u < 2T)
  q = (c 2^Q + T^3) // (2T^3)                      (Python's // floors)
A = Wy @ P @ Wx.T, D = (rows' sums of Wy) x (rows' sums of Wx),
result = clip((A + (D >> 1)) // D, 0, 2^bpp - 1). A source rectangle is the sub-plane; a
destination rectangle is where the result is pasted into a plane of fill codes.
"""
import ctypes

import numpy as np
import pytest

from test_resample_definition import _paste, _sub, chroma_rect

Q = 14
# what the issue lists: ((w, h), (ow, oh), bits)
TORCH_CASES = [((480, 270), (64, 64), 8), ((37, 23), (50, 41), 8), ((200, 130), (33, 17), 10), ((130, 66), (131, 67), 12),
               ((3, 2), (16, 16), 8), ((1, 1), (5, 3), 8), ((7, 5), (1, 1), 8)]


# ------------------------------------------------------------------ the restatement
def cubic_q(u, T):
    """q of one distance u (a Python integer), None if the tap is absent."""
    if u >= 2 * T:
        return None
    c = 3 * u ** 3 - 5 * T * u ** 2 + 2 * T ** 3 if u < T else -u ** 3 + 5 * T * u ** 2 - 8 * T * T * u + 4 * T ** 3
    return (c * 2 ** Q + T ** 3) // (2 * T ** 3)


_W = {}


def weights(n_src, n_out):
    """W[o, s] (0 where the tap is absent), int64 (|q| <= 2^14) computed in Python's integers;
    cached, read only."""
    if (n_src, n_out) not in _W:
        T = 2 * max(n_src, n_out)
        o, s = np.arange(n_out, dtype=np.int64)[:, None], np.arange(n_src, dtype=np.int64)[None, :]
        u = np.abs((2 * o + 1) * n_src - (2 * s + 1) * n_out).astype(object)
        near = 3 * u ** 3 - 5 * T * u ** 2 + 2 * T ** 3
        far = -u ** 3 + 5 * T * u ** 2 - 8 * T * T * u + 4 * T ** 3
        q = (np.where(u < T, near, far) * 2 ** Q + T ** 3) // (2 * T ** 3)       # objects: Python's //, which floors
        W = np.where(u < 2 * T, q, 0).astype(np.int64)
        W.setflags(write=False)
        _W[n_src, n_out] = W
    return _W[n_src, n_out]


def present(n_src, n_out):
    """Whether the tap (o, s) is present, bool array."""
    T = 2 * max(n_src, n_out)
    o, s = np.arange(n_out, dtype=np.int64)[:, None], np.arange(n_src, dtype=np.int64)[None, :]
    return np.abs((2 * o + 1) * n_src - (2 * s + 1) * n_out) < 2 * T


def sums(P, ow, oh):
    """(A, D) of plane P resampled to ow x oh: int64 where sum |qy| sum |qx| max P shows that
    no partial sum leaves it, Python's integers (object arrays) otherwise."""
    h, w = P.shape
    Wy, Wx = weights(h, oh), weights(w, ow)
    bound = int(np.abs(Wy).sum(axis=1).max()) * int(np.abs(Wx).sum(axis=1).max()) * max(1, int(np.abs(P).max()))
    if bound >= 1 << 62:
        Wy, Wx, P = Wy.astype(object), Wx.astype(object), P.astype(object)
    else:
        P = P.astype(np.int64)
    return Wy.dot(P).dot(Wx.T), Wy.sum(axis=1)[:, None] * Wx.sum(axis=1)[None, :]


def unclipped(P, ow, oh):
    A, D = sums(P, ow, oh)
    return ((A + (D >> 1)) // D).astype(np.int64)          # numpy's and Python's // both floor


def resample(P, ow, oh, bpp):
    return np.clip(unclipped(P, ow, oh), 0, (1 << bpp) - 1)


def resampled_planes(planes, OW, OH, bpp, ssh, ssv, src=None, dst=None, fill=(0, 0, 0)):
    """(the semi-planar output's planes, the RGB formats' planes before the conversion) of one
    frame: src / dst in luma samples, None = the whole picture / the whole output."""
    h, w = planes[0].shape
    src = (0, 0, w, h) if src is None else src
    dst = (0, 0, OW, OH) if dst is None else dst
    csrc, cdst = chroma_rect(src, ssh, ssv), chroma_rect(dst, ssh, ssv)
    Y, U, V = _sub(planes[0], src), _sub(planes[1], csrc), _sub(planes[2], csrc)
    y = _paste((OH, OW), fill[0], dst, resample(Y, dst[2], dst[3], bpp))
    ocw, och = (OW + ssh) >> ssh, (OH + ssv) >> ssv
    semi = [y] + [_paste((och, ocw), fill[1 + i], cdst, resample(C, cdst[2], cdst[3], bpp)) for i, C in enumerate((U, V))]
    full = [y] + [_paste((OH, OW), fill[1 + i], dst, resample(C, dst[2], dst[3], bpp)) for i, C in enumerate((U, V))]
    return semi, full


def step_edge(w, h, bpp):
    """A plane of 0 and the largest code with one vertical and one horizontal edge: the negative
    lobes undershoot on the dark side and overshoot on the bright side."""
    P = np.zeros((h, w), np.int64)
    P[h // 3:, w // 3:] = (1 << bpp) - 1
    return P


def axis_s(n_src, n_out):
    """S and max D of one axis from the closed formulas, without the matrix (sizes in the thousands)."""
    T = 2 * max(n_src, n_out)
    S = Dm = 0
    for o in range(n_out):
        k = (2 * o + 1) * n_src
        lo = max(0, (k - 2 * T) // (2 * n_out) - 1)
        qs = [cubic_q(abs(k - (2 * s + 1) * n_out), T) for s in range(lo, min(n_src, (k + 2 * T) // (2 * n_out) + 2))]
        qs = [q for q in qs if q is not None]
        S, Dm = max(S, sum(abs(q) for q in qs)), max(Dm, sum(qs))
    return S, Dm


def within_bound(w, h, ow, oh, bpp):
    return axis_s(w, ow)[0] * axis_s(h, oh)[0] * ((1 << bpp) - 1) < 1 << 62


# ------------------------------------------------------------------ what the definition promises
def test_d_is_positive():
    for n_src in range(1, 41):
        for n_out in range(1, 41):
            W = weights(n_src, n_out)
            assert min(W.sum(axis=1)) > 0, (n_src, n_out)
            assert W.max() <= 1 << Q and W.min() >= -1214              # Keys reaches -2 / 27 at x = 4 / 3
            assert np.array_equal(W, W[::-1, ::-1])                    # flip symmetry


def test_identity_constant_and_rounding():
    rng = np.random.default_rng(1)
    P = rng.integers(0, 4096, (33, 65))
    assert np.array_equal(weights(65, 65), (1 << Q) * np.eye(65, dtype=np.int64))     # c is 0 at every multiple of T
    assert np.array_equal(resample(P, 65, 33, 12), P)
    for ow, oh in ((7, 5), (130, 40), (1, 1), (64, 33)):
        for v in (0, 1234, 4095):
            assert (resample(np.full((33, 65), v), ow, oh, 12) == v).all()
    # 2 -> 1: u = 1 of T = 4 for both taps, equal weights; (1 + 2) / 2 rounds up, once per axis
    W = weights(2, 1)
    assert W[0, 0] == W[0, 1] > 0
    assert resample(np.array([[1, 2], [1, 2]]), 1, 1, 8)[0, 0] == 2
    assert resample(np.array([[1, 2], [3, 4]]), 1, 1, 8)[0, 0] == 3         # 10 / 4
    assert resample(np.array([[1, 2], [3, 3]]), 1, 1, 8)[0, 0] == 2         # 9 / 4
    # upscaling by 2, away from the edge: Catmull-Rom at x = 1.25, 0.25, 0.75, 1.75
    w = [int(x) for x in weights(8, 16)[7, 2:6]]
    keys = [-9 / 128, 111 / 128, 29 / 128, -3 / 128]
    assert all(abs(a - b * 2 ** Q) <= 0.5 for a, b in zip(w, keys)) and w[0] < 0 and w[3] < 0


@pytest.mark.parametrize("bpp", [8, 12])
def test_the_step_edge_clips(bpp):
    top = (1 << bpp) - 1
    for (w, h), (ow, oh) in (((24, 18), (50, 41)), ((66, 34), (40, 24))):
        raw = unclipped(step_edge(w, h, bpp), ow, oh)
        assert (raw < 0).any() and (raw > top).any()                   # the reference itself clips on this input
        out = resample(step_edge(w, h, bpp), ow, oh, bpp)
        assert out.min() == 0 and out.max() == top
        assert ((out == 0) == (raw <= 0)).all() and ((out == top) == (raw >= top)).all()


@pytest.mark.parametrize("size,out,bpp", TORCH_CASES)
@pytest.mark.parametrize("kind", ["noise", "smooth"])
def test_within_one_code_of_torchs_antialiased_bicubic(size, out, bpp, kind):
    import torch
    (w, h), (ow, oh) = size, out
    top = (1 << bpp) - 1
    if kind == "noise":
        P = np.random.default_rng(w + ow + bpp).integers(0, top + 1, (h, w))
    else:
        y, x = np.mgrid[0:h, 0:w]
        P = np.floor(top * (0.5 + 0.25 * np.sin(x / 9.0) + 0.25 * np.cos(y / 7.0))).astype(np.int64)
    t = torch.from_numpy(P.astype(np.float64))[None, None]
    ref = torch.nn.functional.interpolate(t, size=(oh, ow), mode="bicubic", antialias=True, align_corners=False)[0, 0].numpy()
    ref = np.floor(np.clip(ref, 0, top) + 0.5).astype(np.int64)
    diff = np.abs(resample(P, ow, oh, bpp) - ref)
    print("%dx%d -> %dx%d %d-bit %s: max |cub - interpolate| = %d, %.2f %% differ"
          % (w, h, ow, oh, bpp, kind, diff.max(), 100.0 * (diff > 0).mean()))
    assert diff.max() <= 1


# ------------------------------------------------------------------ the library's statement of it
EXTREME = [(16384, 1), (16384, 16384), (1, 16384), (7680, 224), (4320, 224)]


def _library_row_matches(v9, n_src, n_out, o):
    first, w, d, a = v9.bicubic_weights(n_src, n_out, o)
    T, k = 2 * max(n_src, n_out), (2 * o + 1) * n_src
    ref = [cubic_q(abs(k - (2 * s + 1) * n_out), T) for s in range(first, first + len(w))]
    assert ref == w, (n_src, n_out, o)
    assert d == sum(ref) and a == sum(abs(q) for q in ref)
    # nothing present on either side of them
    for s in (first - 1, first + len(w)):
        assert not (0 <= s < n_src) or cubic_q(abs(k - (2 * s + 1) * n_out), T) is None, (n_src, n_out, o, s)


def test_library_weights_match(v9):
    for n_src in range(1, 25):
        for n_out in range(1, 25):
            W, here = weights(n_src, n_out), present(n_src, n_out)
            for o in range(n_out):
                first, w, d, a = v9.bicubic_weights(n_src, n_out, o)
                row = np.zeros(n_src, np.int64)
                row[first:first + len(w)] = w
                assert np.array_equal(row, W[o]), (n_src, n_out, o)
                assert len(w) == here[o].sum() and here[o, first:first + len(w)].all()
                assert d == W[o].sum() > 0 and a == np.abs(W[o]).sum()


@pytest.mark.parametrize("n_src,n_out", EXTREME)
def test_library_weights_match_at_extreme_sizes(v9, n_src, n_out):
    outs = sorted(set([0, 1, n_out // 3, n_out // 2, n_out - 2, n_out - 1]) & set(range(n_out)))
    if n_out <= 224:
        outs = range(n_out)
    for o in outs:
        _library_row_matches(v9, n_src, n_out, o)


def test_library_weights_arguments(v9):
    L = v9.lib()
    for args in ((0, 4, 0), (8, 0, 0), (8, 4, 4), (8, 4, -1), (16385, 4, 0), (4, 16385, 0)):
        assert L.vp9hip_bicubic_weights(*args, None, None, 0, None, None) == v9.EINVAL, args
    assert L.vp9hip_bicubic_weights(8, 4, 0, None, None, -1, None, None) == v9.EINVAL
    w, d, a, f = (ctypes.c_int32 * 3)(7, 7, 7), ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    n = L.vp9hip_bicubic_weights(16, 8, 3, ctypes.byref(f), w, 2, ctypes.byref(d), ctypes.byref(a))   # cap below the count
    W = weights(16, 8)[3]
    assert n == 8 and f.value == 3 and list(w) == [W[3], W[4], 7] and d.value == W.sum() and a.value == np.abs(W).sum()
    assert L.vp9hip_bicubic_weights(16, 8, 3, None, None, 0, None, None) == 8            # every pointer may be NULL
    # the old surface is what it was
    assert L.vp9hip_resample_weights(2, 8, 4, 0, None, None, 0, None) == v9.EINVAL
    assert v9.FILTERS == {"box": 0, "triangle": 1} and v9.FILTER_BICUBIC == 2 and v9.ABI_VERSION == 5
    assert ctypes.sizeof(v9.Resample) == 48
    for name in ("vp9hip_convert_frames_bicubic", "vp9hip_decoder_convert_bicubic", "vp9hip_bicubic_weights"):
        assert name in v9.ABI_SYMBOLS and hasattr(L, name)


# ------------------------------------------------------------------ the bound
def test_the_bound(v9):
    assert not within_bound(7680, 4320, 1, 1, 12)
    assert not within_bound(7680, 4320, 2, 2, 12)
    assert within_bound(7680, 4320, 4, 4, 12)
    assert within_bound(7680, 4320, 1, 1, 8)
    sx, sy = axis_s(3840, 224)[0], axis_s(2160, 224)[0]
    assert 1 << 43 < sx * sy * 255 < 1 << 45                        # 4K -> 224 x 224 at 8 bits: near 2^44
    # the library's sums are the bound's factors
    for n_src, n_out in ((7680, 4), (4320, 2), (1088, 3)):
        assert max(v9.bicubic_weights(n_src, n_out, o)[3] for o in range(n_out)) == axis_s(n_src, n_out)[0]
    # the O(1) ceiling the runtime tries first: at most 4M / n_out + 1 taps of at most 2^Q each
    for n_src, n_out in [(65, 33), (33, 7), (16, 40), (352, 1), (7, 7), (1, 5), (7680, 4), (4320, 2), (3840, 1920)]:
        assert axis_s(n_src, n_out)[0] <= (1 << Q) * (4 * max(n_src, n_out) // n_out + 1)


def test_restatement_rectangles():
    """A source rectangle is the sub-plane; a destination rectangle pastes into the fill."""
    rng = np.random.default_rng(3)
    planes = [rng.integers(0, 256, (30, 40)), rng.integers(0, 256, (15, 20)), rng.integers(0, 256, (15, 20))]
    semi, full = resampled_planes(planes, 12, 10, 8, 1, 1, src=(6, 2, 21, 17), dst=(2, 4, 7, 5), fill=(9, 8, 7))
    assert semi[0].shape == (10, 12) and semi[1].shape == (5, 6) and full[2].shape == (10, 12)
    assert np.array_equal(semi[0][4:9, 2:9], resample(planes[0][2:19, 6:27], 7, 5, 8))
    assert np.array_equal(semi[1][2:5, 1:5], resample(planes[1][1:10, 3:14], 4, 3, 8))
    assert np.array_equal(full[2][4:9, 2:9], resample(planes[2][1:10, 3:14], 7, 5, 8))
    mask = np.ones((10, 12), bool)
    mask[4:9, 2:9] = False
    assert (semi[0][mask] == 9).all() and (full[1][mask] == 8).all() and (full[2][mask] == 7).all()
