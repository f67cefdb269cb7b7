"""The frame metrics' definition (include/vp9hip.h "frame metrics"), CPU suite.

ref_metrics is the numpy statement of the definition and shares no code with the library: it
widens to int64 and uses abs, sum, argmax of the flattened mask and add.reduceat for the cells.
frame_metrics_host (vp9hip_frame_metrics_host, the C statement) is compared with it exactly;
tests/test_gpu_metrics.py compares the kernel with the same reference.
"""
import numpy as np
import pytest

FIELDS = ("sum_a", "sum_b", "sumsq_a", "sad", "sse", "ndiff", "maxdiff", "first")
SIZES = [(1, 1), (16, 16), (17, 15), (65, 33), (70, 38)]
SUBSAMPLINGS = [(1, 1), (1, 0), (0, 1), (0, 0)]


def plane_sizes(w, h, ss_h, ss_v):
    cw, ch = (w + ss_h) >> ss_h, (h + ss_v) >> ss_v
    return [(w, h), (cw, ch), (cw, ch)]


def ref_metrics(planes_a, planes_b, w, h, ss_h, ss_v):
    """(metrics (3, 8) int64, cells (MH, MW) int32 or None) of the top-left w x h luma samples
    and the chroma they cover."""
    out = np.zeros((3, 8), np.int64)
    cells = None
    for p, (pw, ph) in enumerate(plane_sizes(w, h, ss_h, ss_v)):
        a = np.asarray(planes_a[p])[:ph, :pw].astype(np.int64)
        assert a.shape == (ph, pw)
        out[p, 0] = a.sum()
        out[p, 2] = (a * a).sum()
        out[p, 7] = -1
        if planes_b is None:
            continue
        b = np.asarray(planes_b[p])[:ph, :pw].astype(np.int64)
        d = np.abs(a - b)
        ne = (d != 0).ravel()
        out[p, 1] = b.sum()
        out[p, 3] = d.sum()
        out[p, 4] = (d * d).sum()
        out[p, 5] = ne.sum()
        out[p, 6] = d.max()
        out[p, 7] = int(np.argmax(ne)) if ne.any() else -1
        if p == 0:
            rows = np.add.reduceat(d, np.arange(0, ph, 16), axis=0)
            cells = np.add.reduceat(rows, np.arange(0, pw, 16), axis=1).astype(np.int32)
    return out, cells


def random_planes(rng, w, h, bpp, ss_h, ss_v, hi=None):
    dt = np.uint8 if bpp == 8 else np.uint16
    hi = (1 << bpp) if hi is None else hi
    return [rng.integers(0, hi, (ph, pw)).astype(dt) for pw, ph in plane_sizes(w, h, ss_h, ss_v)]


def _check(v9, a, b, w, h, bpp, ss_h, ss_v):
    want, wcells = ref_metrics(a, b, w, h, ss_h, ss_v)
    if b is None:
        got = v9.frame_metrics_host(a, None, w, h, bpp, ss_h, ss_v)
        assert got.dtype == np.int64 and np.array_equal(got, want), (got, want)
        return got
    got, cells = v9.frame_metrics_host(a, b, w, h, bpp, ss_h, ss_v, cells=True)
    assert got.dtype == np.int64 and got.shape == (3, 8) and np.array_equal(got, want), (got, want)
    assert cells.dtype == np.int32 and cells.shape == ((h + 15) >> 4, (w + 15) >> 4)
    assert np.array_equal(cells, wcells)
    assert int(cells.astype(np.int64).sum()) == int(got[0, FIELDS.index("sad")])
    assert np.array_equal(v9.frame_metrics_host(a, b, w, h, bpp, ss_h, ss_v), want)     # without the map
    return got


def test_names(v9):
    assert v9.METRIC_FIELDS == FIELDS and v9.METRIC_CELL == 16


@pytest.mark.parametrize("ss", SUBSAMPLINGS)
@pytest.mark.parametrize("bpp", (8, 10, 12))
def test_host_matches_reference(v9, bpp, ss):
    ss_h, ss_v = ss
    rng = np.random.default_rng(1900 + bpp * 4 + ss_h * 2 + ss_v)
    for w, h in SIZES:
        a = random_planes(rng, w, h, bpp, ss_h, ss_v)
        b = random_planes(rng, w, h, bpp, ss_h, ss_v)
        _check(v9, a, b, w, h, bpp, ss_h, ss_v)
        # equal frames: all differences zero, first -1, psnr inf
        m = _check(v9, a, [p.copy() for p in a], w, h, bpp, ss_h, ss_v)
        assert not m[:, 3:7].any() and (m[:, 7] == -1).all() and np.array_equal(m[:, 0], m[:, 1])
        assert np.isinf(v9.psnr(m, bpp, w, h, ss_h, ss_v)).all()
        # one differing sample, at the last position of each plane
        c = [p.copy() for p in a]
        for p in c:
            p[-1, -1] ^= 1
        m = _check(v9, a, c, w, h, bpp, ss_h, ss_v)
        for p, (pw, ph) in enumerate(plane_sizes(w, h, ss_h, ss_v)):
            assert tuple(m[p, 3:]) == (1, 1, 1, 1, pw * ph - 1)
        # statistics only
        m = _check(v9, a, None, w, h, bpp, ss_h, ss_v)
        assert not m[:, [1, 3, 4, 5, 6]].any() and (m[:, 7] == -1).all()


def test_saturation_beyond_32_bits(v9):
    w, h, bpp = 352, 288, 12
    a = [np.full((ph, pw), 4095, np.uint16) for pw, ph in plane_sizes(w, h, 1, 1)]
    b = [np.zeros_like(p) for p in a]
    m = _check(v9, a, b, w, h, bpp, 1, 1)
    assert m[0, 4] == 4095 * 4095 * w * h > 1 << 40 and m[0, 2] == m[0, 4]
    ps = v9.psnr(m, bpp, w, h)
    assert ps.shape == (3,) and ps.dtype == np.float64 and np.allclose(ps, 0.0, atol=1e-9)


@pytest.mark.parametrize("bpp", (10, 12))
def test_codes_are_not_masked(v9, bpp):
    w, h = 70, 38
    rng = np.random.default_rng(77 + bpp)
    a = random_planes(rng, w, h, bpp, 1, 1, hi=65536)
    b = random_planes(rng, w, h, bpp, 1, 1, hi=65536)
    a[0][0, 0], b[0][0, 0] = 65535, 0
    a[1][:] = 65535
    m = _check(v9, a, b, w, h, bpp, 1, 1)
    assert m[0, 6] == 65535 and m[1, 0] == 65535 * 35 * 19


@pytest.mark.parametrize("bpp", (8, 10))
def test_linesize_larger_than_the_row(v9, bpp):
    w, h = 65, 33
    rng = np.random.default_rng(5 + bpp)
    # random frames of 96 x 48: the compared crop is their top-left corner, the rest is garbage
    big_a = random_planes(rng, 96, 48, bpp, 1, 1)
    big_b = random_planes(rng, 96, 48, bpp, 1, 1)
    va = [p[:ph, :pw] for p, (pw, ph) in zip(big_a, plane_sizes(w, h, 1, 1))]
    vb = [p[:ph, :pw] for p, (pw, ph) in zip(big_b, plane_sizes(w, h, 1, 1))]
    assert not va[0].flags["C_CONTIGUOUS"]
    want, wcells = ref_metrics(va, vb, w, h, 1, 1)
    for a, b in ((va, vb), (big_a, big_b)):           # strided views, and whole planes with a crop
        got, cells = v9.frame_metrics_host(a, b, w, h, bpp, cells=True)
        assert np.array_equal(got, want) and np.array_equal(cells, wcells)


def test_psnr(v9):
    m = np.zeros((2, 3, 8), np.int64)
    m[0, :, 4] = (255 * 255 * 64 * 32, 0, 16 * 32)
    m[1, :, 4] = (64 * 32, 32 * 16, 1)
    ps = v9.psnr(m, 8, 64, 32)
    assert ps.shape == (2, 3) and ps.dtype == np.float64
    assert abs(ps[0, 0]) < 1e-9 and np.isinf(ps[0, 1]) and np.isfinite(ps[0, 2])
    want = 10 * np.log10(255.0 ** 2 * np.array([64 * 32, 32 * 16, 32 * 16]) / np.array([64 * 32, 32 * 16, 1]))
    assert np.allclose(ps[1], want, rtol=1e-12)
    assert np.allclose(v9.psnr(m[1], 8, 64, 32, 0, 0)[2], 10 * np.log10(255.0 ** 2 * 64 * 32))


def test_einval(v9):
    a8 = [np.zeros((64, 64), np.uint8)] * 3
    a16 = [np.zeros((64, 64), np.uint16)] * 3
    bad = [dict(width=0), dict(height=0), dict(width=16385), dict(height=16385), dict(width=-3),
           dict(bpp=9), dict(bpp=16), dict(ss_h=2), dict(ss_v=-1), dict(ss_v=2)]
    for kw in bad:
        args = dict(width=16, height=16, bpp=8, ss_h=1, ss_v=1)
        args.update(kw)
        planes = a8 if args["bpp"] == 8 else a16
        with pytest.raises(v9.Vp9HipError) as e:
            v9.frame_metrics_host(planes, planes, **args)
        assert e.value.code == v9.EINVAL, kw
    with pytest.raises(v9.Vp9HipError) as e:
        v9.frame_metrics_host(a8, None, 16, 16, 8, cells=True)          # cells without b
    assert e.value.code == v9.EINVAL
    assert v9.frame_metrics_host(a8, None, 64, 64, 8)[0, 7] == -1
