"""Residual tensors at model size: the host statement (vp9hip_residual_scaled_host,
csrc/host/vp9h_residual_scaled.c) against a numpy restatement of the definition in
include/vp9hip.h ("residual tensors at model size"), and the properties the definition promises
checked on the restatement alone. CPU only; every comparison is exact, halves by bit pattern.

The restatement shares no code with the library: the box weights as matrices
(test_gpu_convert_scale._weights), A = Wy @ P @ Wx.T in int64, sbox = (A + (w h >> 1)) // (w h)
with Python's floor division, all three planes resampled to OW x OH, the matrix from the
coefficients test_gpu_convert._coefs restates, no offsets, arithmetic shifts, clip to [-m, m],
the half as float32(x) * float32(1 / m) rounded to float16 by numpy.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_convert import KR_KB, _coefs, _rgb
from test_gpu_convert_scale import RATIOS, _weights

FORMATS = ["yuv_i16", "yuv_f16", "rgb_i16", "rgb_f16"]
SUBSAMPLINGS = [(1, 1), (1, 0), (0, 1), (0, 0)]
SIZES = RATIOS + [((1, 1), (1, 1)), ((70, 38), (70, 38))]
MATRICES = [(cs, full) for cs in sorted(KR_KB) for full in (0, 1)] + [(7, 1)]


# ------------------------------------------------------------------ the restatement
def sbox(P, ow, oh):
    h, w = P.shape
    A = _weights(h, oh) @ P.astype(np.int64) @ _weights(w, ow).T
    return (A + (w * h >> 1)) // (w * h)


def matrix(y, u, v, d, cs, full):
    """The RGB residual (R, G, B) of resampled int64 planes."""
    m = (1 << d) - 1
    if cs == 7:
        return [np.clip(x, -m, m) for x in (v, y, u)]
    (cy, crv, cgu, cgv, cbu), s = _coefs(cs, full, d, d)
    rnd = 1 << (s - 1)
    return [np.clip((cy * y + crv * v + rnd) >> s, -m, m),
            np.clip((cy * y - cgu * u - cgv * v + rnd) >> s, -m, m),
            np.clip((cy * y + cbu * u + rnd) >> s, -m, m)]


def resampled(planes, w, h, ssh, ssv, ow, oh):
    """y, u, v: the visible part of each plane through sbox, int64."""
    cw, ch = (w + ssh) >> ssh, (h + ssv) >> ssv
    return [sbox(np.asarray(planes[0])[:h, :w], ow, oh), sbox(np.asarray(planes[1])[:ch, :cw], ow, oh),
            sbox(np.asarray(planes[2])[:ch, :cw], ow, oh)]


def ref_tensor(planes, w, h, ssh, ssv, d, fmt, ow, oh, cs=2, full=0, pre=None):
    """The (3, OH, OW) tensor of one frame; pre: resampled(...) computed before."""
    yuv = pre if pre is not None else resampled(planes, w, h, ssh, ssv, ow, oh)
    out = np.stack(matrix(*yuv, d, cs, full) if fmt.startswith("rgb") else yuv)
    if fmt.endswith("f16"):
        return (out.astype(np.float32) * np.float32(1.0 / ((1 << d) - 1))).astype(np.float16)
    assert out.min() >= -32768 and out.max() <= 32767
    return out.astype(np.int16)


def bits(a):
    a = np.asarray(a)
    return a.view(np.int16) if a.dtype == np.float16 else a


def same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d differ, first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def random_field(rng, w, h, d, ssh, ssv, lo=None, hi=None):
    m = (1 << d) - 1
    lo, hi = (-m if lo is None else lo), (m if hi is None else hi)
    cw, ch = (w + ssh) >> ssh, (h + ssv) >> ssv
    return [rng.integers(lo, hi + 1, s).astype(np.int16) for s in ((h, w), (ch, cw), (ch, cw))]


# ------------------------------------------------------------------ the restatement alone
def test_sbox_properties():
    rng = np.random.default_rng(151)
    P = rng.integers(-4095, 4096, (33, 65))
    for ow, oh in ((33, 17), (7, 5), (100, 40), (1, 1), (65, 33)):
        base = sbox(P, ow, oh)
        for c in (-32768 + 4095, -1, 1, 777, 32767 - 4095):
            assert np.array_equal(sbox(P + c, ow, oh), base + c)
        # the unsigned form of the definition: flip the sign bit, take box, subtract
        flipped = (P.astype(np.int16).view(np.uint16) ^ 0x8000).astype(np.int64)
        assert np.array_equal(sbox(flipped, ow, oh) - 32768, base)
    assert np.array_equal(sbox(P, 65, 33), P)
    for c in (-32768, -1234, 0, 32767):
        assert (sbox(np.full((33, 65), c), 7, 5) == c).all()
    for blk, want in (([[-3, -3], [-2, -2]], -2), ([[-3, -2], [-2, -2]], -2), ([[-2, -1], [-1, -1]], -1),
                      ([[3, 3], [2, 2]], 3)):
        assert int(np.sum(blk)) in (-10, -9, -5, 10)
        assert sbox(np.array(blk), 1, 1)[0, 0] == want


def test_every_sum_fits_int32():
    worst = 0
    for d in (8, 10, 12):
        for cs, full in MATRICES[:-1]:
            (cy, crv, cgu, cgv, cbu), s = _coefs(cs, full, d, d)
            assert s == 14
            worst = max(worst, cy + crv, cy + cgu + cgv, cy + cbu)
    assert worst == 54367 and worst * 32768 + (1 << 13) < 1 << 31


@pytest.mark.parametrize("d", [8, 10, 12])
def test_rgb_residual_is_the_difference_of_two_pixels(d):
    """RGB(pred + r) - RGB(pred) is within one code of the matrix of r in every channel sample
    where neither pixel clips: same size, chroma at full resolution, every matrix and range. The
    input, uniform random pixels, leaves at least half of the channel samples unclipped by the
    reference conversion alone, so the property is not vacuous."""
    rng = np.random.default_rng(300 + d)
    m = (1 << d) - 1
    pred = [rng.integers(0, m + 1, (48, 64)) for _ in range(3)]
    pix = [rng.integers(0, m + 1, (48, 64)) for _ in range(3)]
    r = [a - b for a, b in zip(pix, pred)]
    for cs, full in MATRICES:
        a, b = _rgb(pix, d, 0, 0, cs, full, d), _rgb(pred, d, 0, 0, cs, full, d)
        res = matrix(*r, d, cs, full)
        alone = np.stack([(x > 0) & (x < m) for x in a])
        assert alone.mean() >= 0.5, (cs, full, alone.mean())
        worst = checked = 0
        for ch in range(3):
            free = alone[ch] & (b[ch] > 0) & (b[ch] < m)
            checked += int(free.sum())
            worst = max(worst, int(np.abs((a[ch] - b[ch]) - res[ch])[free].max()))
        assert worst <= 1 and checked > 0.2 * 3 * 48 * 64, (cs, full, worst, checked)


# ------------------------------------------------------------------ the host statement against it
@pytest.mark.parametrize("ss", SUBSAMPLINGS)
@pytest.mark.parametrize("d", [8, 10, 12])
def test_host_statement_equals_the_restatement(v9, d, ss):
    ssh, ssv = ss
    rng = np.random.default_rng(4000 + 100 * d + 10 * ssh + ssv)
    for (w, h), (ow, oh) in SIZES:
        planes = random_field(rng, w, h, d, ssh, ssv)
        pre = resampled(planes, w, h, ssh, ssv, ow, oh)
        what = "%dx%d -> %dx%d" % (w, h, ow, oh)
        for fmt in FORMATS:
            mats = MATRICES if fmt.startswith("rgb") and (w, h, ow, oh) == (65, 33, 33, 17) else [(2, 0)]
            for cs, full in mats:
                got = v9.residual_scaled_host(planes, w, h, ssh, ssv, d, fmt, (ow, oh), cs, full)
                same(got, ref_tensor(planes, w, h, ssh, ssv, d, fmt, ow, oh, cs, full, pre), "%s %s cs %d full %d" % (fmt, what, cs, full))
    # resize=None is the field's own size
    planes = random_field(rng, 70, 38, d, ssh, ssv)
    same(v9.residual_scaled_host(planes, 70, 38, ssh, ssv, d, "yuv_i16", None),
         ref_tensor(planes, 70, 38, ssh, ssv, d, "yuv_i16", 70, 38), "own size")


def clip_cases(w, h, ssh, ssv, d):
    """Fields that reach both clips of every RGB channel, and the int16 extremes."""
    m = (1 << d) - 1
    cw, ch = (w + ssh) >> ssh, (h + ssv) >> ssv

    def const(y, u, v):
        return [np.full((h, w), y, np.int16), np.full((ch, cw), u, np.int16), np.full((ch, cw), v, np.int16)]
    return {"max": const(32767, 32767, 32767), "min": const(-32768, -32768, -32768),
            "+m in Y and V": const(m, 0, m), "-m in Y and V": const(-m, 0, -m),
            "-m in Y and U": const(-m, -m, 0), "+m in Y and U": const(m, m, 0)}


@pytest.mark.parametrize("d", [8, 10, 12])
def test_extremes_and_clips(v9, d):
    m = (1 << d) - 1
    w, h, ow, oh = 65, 33, 7, 5
    reached = set()
    for name, planes in clip_cases(w, h, 1, 1, d).items():
        for fmt in FORMATS:
            got = v9.residual_scaled_host(planes, w, h, 1, 1, d, fmt, (ow, oh), 2, 0)
            same(got, ref_tensor(planes, w, h, 1, 1, d, fmt, ow, oh, 2, 0), "%s %s" % (name, fmt))
            if fmt == "yuv_i16" and name in ("max", "min"):
                assert (got == (32767 if name == "max" else -32768)).all()
            if fmt == "rgb_i16":
                if name in ("max", "min"):
                    assert (np.abs(got.astype(np.int32)) <= m).all()
                for chn in range(3):
                    for lim in (-m, m):
                        if (got[chn] == lim).all():
                            reached.add((chn, lim))
    assert reached == {(chn, lim) for chn in range(3) for lim in (-m, m)}


def test_strided_planes(v9):
    rng = np.random.default_rng(77)
    w, h, d = 65, 33, 10
    big = [rng.integers(-1023, 1024, s).astype(np.int16) for s in ((40, 128), (24, 96), (24, 96))]
    views = [big[0][:, 3:], big[1][1:, 5:], big[2][2::1, 7:]]
    for fmt in FORMATS:
        same(v9.residual_scaled_host(views, w, h, 1, 1, d, fmt, (33, 17)),
             ref_tensor(views, w, h, 1, 1, d, fmt, 33, 17), "strided " + fmt)
    # every second row: a pitch twice the row
    alt = [a[::2] for a in big]
    same(v9.residual_scaled_host(alt, 64, 20, 1, 1, d, "rgb_i16", (9, 9)),
         ref_tensor(alt, 64, 20, 1, 1, d, "rgb_i16", 9, 9), "every second row")


def test_layout(v9):
    L = v9.lib()
    pitch = ctypes.c_int64()

    def lay(fmt=0, ow=33, oh=17, p=0, fs=0):
        d = v9.ResidDesc(fmt, 2, 0, ow, oh, p, fs)
        return L.vp9hip_resid_layout(ctypes.byref(d), ctypes.byref(pitch)), pitch.value
    assert lay() == (3 * 66 * 17, 66)
    assert lay(p=80) == (3 * 80 * 17, 80)
    assert lay(p=66, fs=3 * 66 * 17 + 2)[0] == 3 * 66 * 17
    for kw in (dict(fmt=-1), dict(fmt=4), dict(ow=0), dict(ow=16385), dict(oh=0), dict(oh=16385), dict(p=64), dict(p=72),
               dict(p=-16), dict(fs=3 * 66 * 17 - 2), dict(fs=3 * 66 * 17 + 1), dict(fs=-2)):
        assert lay(**kw)[0] == v9.EINVAL, kw
    assert L.vp9hip_resid_layout(None, None) == v9.EINVAL


def test_host_statement_refuses(v9):
    L = v9.lib()
    planes = [np.zeros((8, 8), np.int16) for _ in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in planes])
    pitch = (ctypes.c_ssize_t * 3)(8, 8, 8)
    out = np.full(3 * 8 * 8 + 8, 0x5a5a, np.int16)

    def call(w=8, h=8, ssh=1, ssv=1, d=8, fmt=2, cs=2, ow=4, oh=4, p=0, fs=0, dst=None, pl=ptrs, pt=pitch, desc=True):
        de = v9.ResidDesc(fmt, cs, 0, ow, oh, p, fs)
        return L.vp9hip_residual_scaled_host(ctypes.byref(pl) if pl is not None else None,
                                             ctypes.byref(pt) if pt is not None else None, w, h, ssh, ssv, d,
                                             ctypes.byref(de) if desc else None, out.ctypes.data if dst is None else dst)
    assert call() == 0 and (out[:48] != 0x5a5a).all() and (out[48:] == 0x5a5a).all()
    out[:] = 0x5a5a
    null_plane = (ctypes.c_void_p * 3)(planes[0].ctypes.data, None, planes[2].ctypes.data)
    for kw in (dict(w=0), dict(w=16385), dict(h=0), dict(h=16385), dict(ssh=2), dict(ssv=-1), dict(d=9), dict(d=16),
               dict(fmt=-1), dict(fmt=4), dict(cs=0), dict(cs=6), dict(cs=8), dict(cs=-1), dict(fmt=3, cs=0),
               dict(ow=0), dict(ow=16385), dict(oh=0), dict(oh=16385), dict(p=6), dict(p=24), dict(p=-16), dict(fs=94),
               dict(fs=97), dict(fs=-2), dict(dst=out.ctypes.data + 1), dict(pl=None), dict(pt=None), dict(pl=null_plane),
               dict(desc=False)):
        assert call(**kw) == v9.EINVAL, kw
    assert (out == 0x5a5a).all()
    assert call(fmt=0, cs=0) == 0                  # the YUV formats do not look at the colour space
    with pytest.raises(v9.Vp9HipError) as e:
        v9.residual_scaled_host(planes, 8, 8, 1, 1, 8, "rgb_i16", (4, 4), colorspace=6)
    assert e.value.code == v9.EINVAL
    with pytest.raises(v9.Vp9HipError):
        v9.residual_scaled_host(planes, 8, 8, 1, 1, 8, "rgb_i16", (0, 4))
    with pytest.raises(ValueError):
        v9.residual_scaled_host(planes, 16, 8, 1, 1, 8, "rgb_i16", (4, 4))     # planes smaller than the size
