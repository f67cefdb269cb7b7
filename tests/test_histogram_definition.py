"""The frame histograms' definition (include/vp9hip.h "frame histograms"), CPU suite.

ref_hist is the numpy statement of the definition and shares no code with the library's
csrc/host/vp9h_hist.c: PLANES is np.bincount of the clamped, shifted codes of each plane's
rectangle; RGBM restates the integer matrix from vp9hip_out_coefs' coefficients (nearest chroma
sample U[y >> ss_v][x >> ss_h], round half up, clip) and bincounts R, G, B and their maximum.
histograms_host (vp9hip_frame_histograms_host, the C statement) is compared with it exactly;
tests/test_gpu_histogram.py compares the kernel with the same reference.
"""
import ctypes

import numpy as np
import pytest

from test_metrics_definition import SUBSAMPLINGS, plane_sizes, random_planes

SIZES = [(1, 1), (16, 16), (65, 33), (70, 38)]
COLOURS = [(cs, fr) for cs in (1, 2, 5, 7) for fr in (False, True)]


def ref_hist(v9, planes, bpp, ss_h, ss_v, what, bins, rect, colorspace=2, full_range=False):
    """(C, bins) int32 of the luma rectangle rect = (x, y, w, h) of a frame and the chroma it covers."""
    k = bins.bit_length() - 1
    assert 1 << k == bins and 4 <= k <= bpp
    x, y, w, h = rect
    sh, maxv = bpp - k, (1 << bpp) - 1
    if what == "planes":
        out = []
        for p in range(3):
            sx, sy = (ss_h, ss_v) if p else (0, 0)
            px, py, pw, ph = x >> sx, y >> sy, (w + sx) >> sx, (h + sy) >> sy
            c = np.asarray(planes[p])[py:py + ph, px:px + pw].astype(np.int64)
            assert c.shape == (ph, pw)
            out.append(np.bincount((np.minimum(c, maxv) >> sh).ravel(), minlength=bins))
        return np.stack(out).astype(np.int32)
    yi, xi = np.arange(y, y + h)[:, None], np.arange(x, x + w)[None, :]
    Y = np.asarray(planes[0]).astype(np.int64)[yi, xi]
    U = np.asarray(planes[1]).astype(np.int64)[yi >> ss_v, xi >> ss_h]
    V = np.asarray(planes[2]).astype(np.int64)[yi >> ss_v, xi >> ss_h]
    if colorspace == 7:                                     # planes G, B, R
        R, G, B = (np.minimum(a, maxv) for a in (V, Y, U))
    else:
        (cy, crv, cgu, cgv, cbu), s = v9.out_coefs(colorspace, full_range, bpp, bpp)
        assert s == 14
        yy = cy * (Y - (0 if full_range else 16 << (bpp - 8))) + (1 << (s - 1))
        cu, cv = U - (1 << (bpp - 1)), V - (1 << (bpp - 1))
        R = np.clip((yy + crv * cv) >> s, 0, maxv)
        G = np.clip((yy - cgu * cu - cgv * cv) >> s, 0, maxv)
        B = np.clip((yy + cbu * cu) >> s, 0, maxv)
    M = np.maximum(R, np.maximum(G, B))
    return np.stack([np.bincount((a >> sh).ravel(), minlength=bins) for a in (R, G, B, M)]).astype(np.int32)


def check_sums(hist, what, rect, ss_h, ss_v):
    """Channel sums, and M's cumulative counts below every other channel's."""
    _, _, w, h = rect
    cw, ch = (w + ss_h) >> ss_h, (h + ss_v) >> ss_v
    sums = hist.astype(np.int64).sum(-1)
    if what == "planes":
        assert tuple(sums) == (w * h, cw * ch, cw * ch)
    else:
        assert tuple(sums) == (w * h,) * 4
        cum = np.cumsum(hist.astype(np.int64), axis=-1)
        assert (cum[3] <= cum[:3]).all()


def _check(v9, planes, w, h, bpp, ss_h, ss_v, what, bins, rect=None, cs=2, fr=False):
    r = rect or (0, 0, w, h)
    want = ref_hist(v9, planes, bpp, ss_h, ss_v, what, bins, r, cs, fr)
    got = v9.histograms_host(planes, w, h, bpp, ss_h, ss_v, what=what, bins=bins, colorspace=cs, full_range=fr, rect=rect)
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), (what, bins, r, cs, fr)
    check_sums(got, what, r, ss_h, ss_v)
    return got


def test_names(v9):
    assert v9.HIST_MODES == {"planes": 0, "rgbm": 1}
    assert v9.HIST_CHANNELS == {"planes": ("y", "u", "v"), "rgbm": ("r", "g", "b", "m")}
    for s in ("vp9hip_frame_histograms", "vp9hip_frame_histograms_host", "vp9hip_decoder_histograms"):
        assert s in v9.ABI_SYMBOLS and hasattr(v9.lib(), s)
    assert ctypes.sizeof(v9.HistDesc) == 24 + ctypes.sizeof(ctypes.c_void_p)


@pytest.mark.parametrize("ss", SUBSAMPLINGS)
@pytest.mark.parametrize("bpp", (8, 10, 12))
def test_host_matches_the_definition(v9, bpp, ss):
    ss_h, ss_v = ss
    rng = np.random.default_rng(2100 + 10 * bpp + 2 * ss_h + ss_v)
    for i, (w, h) in enumerate(SIZES):
        planes = random_planes(rng, w, h, bpp, ss_h, ss_v)
        for bins in (16, 256, 1 << bpp):
            _check(v9, planes, w, h, bpp, ss_h, ss_v, "planes", bins)
            cs, fr = COLOURS[(i + bins.bit_length()) % len(COLOURS)]
            _check(v9, planes, w, h, bpp, ss_h, ss_v, "rgbm", bins, cs=cs, fr=fr)


@pytest.mark.parametrize("bpp", (8, 10, 12))
def test_every_colour(v9, bpp):
    """The matrix's clips on both sides: noise in all three planes leaves the RGB cube often."""
    w, h = 70, 38
    rng = np.random.default_rng(77 + bpp)
    planes = random_planes(rng, w, h, bpp, 1, 1)
    for cs, fr in COLOURS:
        got = _check(v9, planes, w, h, bpp, 1, 1, "rgbm", 1 << bpp, cs=cs, fr=fr)
        if cs != 7:
            assert got[0, 0] > 0 and got[0, -1] > 0          # R clipped at both ends


@pytest.mark.parametrize("ss", SUBSAMPLINGS)
def test_rectangles(v9, ss):
    ss_h, ss_v = ss
    w, h, bpp = 70, 38, 10
    rng = np.random.default_rng(5 + 2 * ss_h + ss_v)
    planes = random_planes(rng, w, h, bpp, ss_h, ss_v)
    for rect in ((0, 0, 65, 33), (2, 4, 17, 15), (68, 36, 1, 1), (69 & ~ss_h, 37 & ~ss_v, 1, 1), (2, 0, 1, 38),
                 (0, 36, 70, 1), (0, 0, 70, 38)):
        _check(v9, planes, w, h, bpp, ss_h, ss_v, "planes", 1024, rect)
        _check(v9, planes, w, h, bpp, ss_h, ss_v, "rgbm", 256, rect, cs=5)


def test_codes_above_the_depth(v9):
    w, h, bpp = 17, 15, 10
    planes = [np.full((ph, pw), 65535, np.uint16) for pw, ph in plane_sizes(w, h, 1, 1)]
    planes[0][0, :3] = (1023, 1024, 512)
    for bins in (16, 256, 1024):
        got = _check(v9, planes, w, h, bpp, 1, 1, "planes", bins)
        assert got[0, -1] == w * h - 1 and got[0, bins // 2] == 1 and got[1, -1] == 9 * 8 and got[2, -1] == 9 * 8


def test_strided_planes(v9):
    w, h, bpp = 65, 33, 8
    rng = np.random.default_rng(9)
    wide = random_planes(rng, 2 * w, h, bpp, 1, 1)
    cw = (w + 1) >> 1
    padded = [wide[0][:, :w], wide[1][:, :cw], wide[2][:, :cw]]             # row stride above the width
    tight = [np.ascontiguousarray(p) for p in padded]
    for what in ("planes", "rgbm"):
        a = v9.histograms_host(padded, w, h, bpp, what=what)
        assert np.array_equal(a, v9.histograms_host(tight, w, h, bpp, what=what))
        assert np.array_equal(a, ref_hist(v9, tight, bpp, 1, 1, what, 256, (0, 0, w, h)))
    every_other = [p[:, ::2] for p in wide]                                  # element stride: copied by the wrapper
    assert np.array_equal(v9.histograms_host(every_other, w, h, bpp),
                          ref_hist(v9, [np.ascontiguousarray(p) for p in every_other], bpp, 1, 1, "planes", 256, (0, 0, w, h)))


def test_refusals_write_nothing(v9):
    L = v9.lib()
    px = np.arange(16, dtype=np.uint8).reshape(4, 4)
    ptrs = (ctypes.c_void_p * 3)(px.ctypes.data, px.ctypes.data, px.ctypes.data)
    hole = (ctypes.c_void_p * 3)(px.ctypes.data, None, px.ctypes.data)
    ls = (ctypes.c_ssize_t * 3)(4, 4, 4)
    out = np.full((4, 256), 0x5A5A5A5A, np.int32)

    def call(planes=ptrs, lines=ls, bpp=8, ss_h=1, ss_v=1, desc=True, rect=None, dst=True, **kw):
        f = dict(what=0, bins_log2=8, colorspace=2, full_range=0, width=4, height=4)
        f.update(kw)
        d = v9.HistDesc(f["what"], f["bins_log2"], f["colorspace"], f["full_range"], f["width"], f["height"], None)
        r = v9.Rect(*rect) if rect else None
        return L.vp9hip_frame_histograms_host(ctypes.byref(planes) if planes else None, ctypes.byref(lines) if lines else None,
                                              bpp, ss_h, ss_v, ctypes.byref(d) if desc else None,
                                              ctypes.byref(r) if r else None, out.ctypes.data if dst else None)
    bad = [dict(planes=None), dict(lines=None), dict(desc=False), dict(dst=False), dict(planes=hole),
           dict(bpp=9), dict(bpp=16), dict(ss_h=2), dict(ss_v=-1),
           dict(what=2), dict(what=-1), dict(bins_log2=3), dict(bins_log2=9), dict(bpp=10, bins_log2=11),
           dict(what=1, colorspace=0), dict(what=1, colorspace=6), dict(what=1, colorspace=8), dict(what=1, colorspace=-1),
           dict(width=0), dict(height=0), dict(width=16385), dict(height=16385),
           dict(rect=(1, 0, 1, 1)), dict(rect=(0, 1, 1, 1)), dict(rect=(0, 0, 5, 1)), dict(rect=(0, 0, 1, 5)),
           dict(rect=(2, 0, 3, 1)), dict(rect=(0, 2, 1, 3)), dict(rect=(0, 0, 0, 1)), dict(rect=(0, 0, 1, 0)),
           dict(rect=(-2, 0, 1, 1)), dict(rect=(0, -2, 1, 1)), dict(rect=(4, 0, 1, 1)), dict(rect=(0, 0, 0x7fffffff, 1)),
           dict(rect=(0, 0, 1, -1))]
    for kw in bad:
        assert call(**kw) == v9.EINVAL, kw
    assert (out == 0x5A5A5A5A).all()
    assert call(ss_h=0, ss_v=0, rect=(1, 1, 1, 1)) == 0                      # 4:4:4: any origin
    assert out[0, 5] == 1 and out[:3].sum() == 3 and (out[3] == 0x5A5A5A5A).all()
    assert call(what=1, colorspace=7, bins_log2=4, rect=(2, 2, 2, 2)) == 0   # writes C * B counts, no more
    flat = out.ravel()                                       # (4, 16) at the start of the array
    assert flat[:64].sum() == 16 and not flat[64:261].any() and flat[261] == 1 and (flat[768:] == 0x5A5A5A5A).all()
    with pytest.raises(ValueError):
        v9.histograms_host([px, px, px], 4, 4, 8, bins=100)
    with pytest.raises(ValueError):
        v9.histograms_host([px, px, px], 4, 4, 8, what="yuv")
    with pytest.raises(ValueError):
        v9.histograms_host([px, px, px.astype(np.uint16)], 4, 4, 8)
    with pytest.raises(ValueError):
        v9.histograms_host([px, px], 4, 4, 8)
    for bins in (8, 512):
        with pytest.raises(v9.Vp9HipError) as e:
            v9.histograms_host([px, px, px], 4, 4, 8, bins=bins)
        assert e.value.code == v9.EINVAL


# ------------------------------------------------------------------ hist_percentile
def test_percentile_table(v9):
    h = np.array([[0, 0, 4, 0, 4, 0, 2, 0],        # total 10
                  [5, 0, 0, 0, 0, 0, 0, 5],        # the ends
                  [0, 0, 0, 0, 0, 0, 0, 0],        # empty
                  [0, 0, 0, 7, 0, 0, 0, 0],        # one bin
                  [1, 1, 1, 1, 1, 1, 1, 1]], np.int32)
    table = {(0, 1): [2, 0, 0, 3, 0],              # zero: bin 0 if it is not empty, else the first that is not
             (1, 10): [2, 0, 0, 3, 0],
             (4, 10): [2, 0, 0, 3, 3],             # a tie: 10 * 4 >= 4 * 10 already at bin 2
             (41, 100): [4, 0, 0, 3, 3],
             (1, 2): [4, 0, 0, 3, 3],              # a tie at the median of row 1: bin 0 holds exactly half
             (51, 100): [4, 7, 0, 3, 4],
             (8, 10): [4, 7, 0, 3, 6],
             (81, 100): [6, 7, 0, 3, 6],
             (999, 1000): [6, 7, 0, 3, 7],
             (1, 1): [6, 7, 0, 3, 7]}
    for (num, den), want in table.items():
        got = v9.hist_percentile(h, num, den)
        assert got.dtype == np.int64 and got.shape == (5,) and list(got) == want, (num, den, got)
        assert int(v9.hist_percentile(h[0], num, den)) == want[0]
        assert np.array_equal(v9.hist_percentile(h.reshape(5, 1, 8), num, den), np.array(want).reshape(5, 1))
    big = np.array([[1 << 28, 0, 1 << 28, 1]], np.int32)                      # products past 32 bits
    assert list(v9.hist_percentile(big, 999999, 1000000)) == [2] and list(v9.hist_percentile(big, 1, 1)) == [3]
    for num, den in ((-1, 10), (11, 10), (0, 0)):
        with pytest.raises(ValueError):
            v9.hist_percentile(h, num, den)


def test_percentile_of_a_tensor(v9):
    torch = pytest.importorskip("torch")
    h = np.array([[0, 0, 4, 0, 4, 0, 2, 0], [0] * 8, [5, 0, 0, 0, 0, 0, 0, 5]], np.int32)
    for num, den in ((0, 1), (4, 10), (1, 2), (51, 100), (1, 1)):
        got = v9.hist_percentile(torch.from_numpy(h), num, den)
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), v9.hist_percentile(h, num, den))


# ------------------------------------------------------------------ light_levels
def _pq(e):
    """SMPTE ST 2084's EOTF from its constants, cd/m^2."""
    m1, m2, c1, c2, c3 = 0.1593017578125, 78.84375, 0.8359375, 18.8515625, 18.6875
    p = e ** (1 / m2)
    return 10000. * (max(p - c1, 0.) / (c2 - c3 * p)) ** (1 / m1)


def test_light_levels_pq(v9):
    h = np.zeros(1024, np.int32)
    h[769] = 1234
    lv = v9.light_levels(h, 10, "pq")
    want = _pq(769 / 1023)
    assert 990 < want < 1010                                 # code 769 is about 1000 cd/m^2
    for key in ("max_nits", "avg_nits", "p999/1000"):
        assert abs(lv[key] - want) <= 1e-9 * want, key
    h[520] = 3 * 1234                                        # a two-code mix: the weighted mean
    lv = v9.light_levels(h, 10, "pq", percentiles=((1, 2), (3, 4), (76, 100), (1, 1)))
    a, b = _pq(520 / 1023), want
    assert abs(lv["avg_nits"] - (3 * a + b) / 4) <= 1e-9 * b and abs(lv["max_nits"] - b) <= 1e-9 * b
    assert abs(lv["p1/2"] - a) <= 1e-9 * a and abs(lv["p3/4"] - a) <= 1e-9 * a
    assert abs(lv["p76/100"] - b) <= 1e-9 * b and abs(lv["p1/1"] - b) <= 1e-9 * b
    both = v9.light_levels(np.stack([h, np.zeros_like(h)]), 10, "pq")         # (N, B), one of them empty
    assert both["max_nits"].shape == (2,) and abs(both["max_nits"][0] - b) <= 1e-9 * b
    assert both["max_nits"][1] == 0 and both["avg_nits"][1] == 0 and both["p999/1000"][1] == 0


def test_light_levels_other_transfers_and_refusals(v9):
    h = np.zeros(256, np.int64)
    h[255] = h[128] = 10
    hlg = v9.light_levels(h, 8, "hlg", peak_nits=1000)
    assert abs(hlg["max_nits"] - 1000.) < 1e-3      # the constants have 8 digits
    assert True and 0 < hlg["avg_nits"] < 1000
    srgb = v9.light_levels(h, 8, "srgb", white_nits=100)
    assert abs(srgb["max_nits"] - 100.) < 1e-9 and abs(srgb["avg_nits"] - 50 * (1 + ((128 / 255 + .055) / 1.055) ** 2.4)) < 1e-9
    assert v9.light_levels(h, 8, "bt709")["max_nits"] == pytest.approx(203.)
    with pytest.raises(ValueError):
        v9.light_levels(h, 10, "pq")                         # a 256-bin table for a 10-bit depth
    with pytest.raises(ValueError):
        v9.light_levels(np.zeros((2, 2, 256)), 8, "pq")
    with pytest.raises(ValueError):
        v9.light_levels(h, 9, "pq")
    with pytest.raises(ValueError):
        v9.light_levels(h, 8, "gamma22")
