"""The graded output's definition on the host (include/vp9hip.h "Graded output"):
vp9hip_grade_host against a numpy restatement that shares no code with the library, the WebM
Colour element written and read back, and the properties of make_grade's tables. No GPU.

make_grade's tables come from float64 formulas whose pow differs across libms, so they are held
to the formulas within +-1 table unit, not pinned bit for bit.
"""
import numpy as np
import pytest


def restate(bpp, in_lut, m, out_lut, codes):
    """The three stages, from the header's formulas: codes (..., 3) -> v (..., 3)."""
    L = np.asarray(in_lut, np.int64)[np.asarray(codes, np.int64)]
    P = np.clip((L @ np.asarray(m, np.int64).reshape(3, 3).T + 8192) >> 14, 0, 65535)      # numpy's >> floors
    i, f = P >> 4, P & 15
    o = np.asarray(out_lut, np.int64)
    return ((o[i] * (16 - f) + o[i + 1] * f + 8) >> 4).astype(np.uint16)


def random_grade(rng, bpp, out_max):
    """Seeded random tables (not curves: any index mistake shows) and a matrix with negative
    off-diagonal terms and row gains above 1."""
    in_lut = rng.integers(0, 65536, 1 << bpp)
    out_lut = rng.integers(0, out_max + 1, 4097)
    m = np.array([[30000, -9000, -2500], [-7000, 34000, -6000], [-1500, -12000, 36000]]) + rng.integers(-500, 500, (3, 3))
    return in_lut, m, out_lut


@pytest.mark.parametrize("bpp", [8, 10, 12])
@pytest.mark.parametrize("fmt", ["rgbp_u8", "rgbp_f16"])
def test_grade_host_is_the_definition(v9, bpp, fmt):
    rng = np.random.default_rng(100 * bpp + len(fmt))
    in_lut, m, out_lut = random_grade(rng, bpp, 65535 if fmt == "rgbp_f16" else 255)
    g = v9.Grade(bpp, fmt, in_lut, m, out_lut)
    codes = rng.integers(0, 1 << bpp, (37, 53, 3))
    codes[0, 0], codes[0, 1] = 0, (1 << bpp) - 1
    ref = restate(bpp, in_lut, m, out_lut, codes)
    got = v9.grade_host(g, codes)
    assert got.dtype == np.uint16 and got.shape == codes.shape
    assert np.array_equal(got, ref)
    P = (in_lut[codes] @ m.T + 8192) >> 14
    assert (P < 0).mean() > .01 and (P > 65535).mean() > .01       # both clips are exercised
    # the extremes of the matrix: the sum passes 32 bits
    big = np.array([[65536] * 3, [-65536] * 3, [65536, -65536, 65536]])
    g2 = v9.Grade(bpp, fmt, in_lut, big, out_lut)
    assert np.array_equal(v9.grade_host(g2, codes), restate(bpp, in_lut, big, out_lut, codes))


def test_grade_refuses_what_the_definition_excludes(v9):
    rng = np.random.default_rng(5)
    in_lut, m, out_lut = random_grade(rng, 10, 255)
    v9.Grade(10, "rgb24", in_lut, m, out_lut)
    bad_out = out_lut.copy()
    bad_out[4096] = 256
    bad_m = m.copy()
    bad_m[2, 0] = -65537
    for args in ((10, "rgb24", in_lut, m, bad_out), (10, "rgb24", in_lut, bad_m, out_lut), (10, "rgb24", in_lut[:-1], m, out_lut),
                 (10, "rgb24", in_lut, m, out_lut[:-1]), (9, "rgb24", in_lut, m, out_lut), (10, "semiplanar", in_lut, m, out_lut)):
        with pytest.raises(ValueError):
            v9.Grade(*args)
    # the C statement refuses them too (the desc built by hand, past the Python checks)
    g = v9.Grade(10, "rgb24", in_lut, m, out_lut)
    codes = np.zeros((1, 3), np.uint16)
    g.out_lut[7] = 300
    with pytest.raises(v9.Vp9HipError) as e:
        v9.grade_host(g, codes)
    assert e.value.code == v9.EINVAL
    g.out_lut[7] = 3
    g.m[1, 1] = 65537
    with pytest.raises(v9.Vp9HipError):
        v9.grade_host(g, codes)
    with pytest.raises(ValueError):
        v9.grade_host(v9.Grade(10, "rgb24", in_lut, m, out_lut), np.full((1, 3), 1024))


COLOUR = dict(matrix=9, bits_per_channel=10, range=1, transfer=16, primaries=9, max_cll=1000, max_fall=400,
              luminance_max=1000.0, luminance_min=0.005)


def test_webm_colour_round_trip(v9):
    frames = [b"\x01\x02\x03", b"\x04\x05"]
    before = v9.webm_write(frames, 64, 48)
    data = v9.webm_write(frames, 64, 48, colour=COLOUR)
    got = v9.webm_colour(data)
    assert got == dict(COLOUR, present=1)
    # the frames and the header are read as before
    info, fr = v9.webm_read(data)
    assert (info.width, info.height) == (64, 48) and [d for _, d, _ in fr] == frames
    # without it: today's bytes, and no element
    assert v9.webm_write(frames, 64, 48, colour=None) == before == v9.webm_write(frames, 64, 48)
    assert v9.webm_colour(before) == dict(present=0, matrix=2, bits_per_channel=0, range=0, transfer=2, primaries=2,
                                          max_cll=0, max_fall=0, luminance_max=0.0, luminance_min=0.0)
    part = v9.webm_colour(v9.webm_write(frames, 64, 48, colour=dict(transfer=18, primaries=9)))
    assert (part["present"], part["transfer"], part["primaries"], part["matrix"], part["range"]) == (1, 18, 9, 2, 0)
    with pytest.raises(v9.Vp9HipError):
        v9.webm_colour(data[:len(data) // 2])


def test_grade_for_maps_the_codes(v9):
    g = v9.grade_for(COLOUR, 10, "rgbp_f16")
    ref = v9.make_grade(10, "rgbp_f16", "pq", "bt2020", peak_nits=1000.0)
    assert all(np.array_equal(a, b) for a, b in ((g.in_lut, ref.in_lut), (g.m, ref.m), (g.out_lut, ref.out_lut)))
    g = v9.grade_for(dict(transfer=18, primaries=9), 10, "rgb24", tonemap="clip")
    ref = v9.make_grade(10, "rgb24", "hlg", "bt2020", tonemap="clip")
    assert np.array_equal(g.in_lut, ref.in_lut) and np.array_equal(g.out_lut, ref.out_lut)
    for t, p, names in ((1, 1, ("bt709", "bt709")), (13, 5, ("srgb", "bt601")), (1, 6, ("bt709", "bt601_525"))):
        g = v9.grade_for(dict(transfer=t, primaries=p), 8, "rgb24")
        ref = v9.make_grade(8, "rgb24", *names)
        assert np.array_equal(g.in_lut, ref.in_lut) and np.array_equal(g.m, ref.m)
    for c in (dict(transfer=2, primaries=1), dict(transfer=16, primaries=2), {}):
        with pytest.raises(ValueError):
            v9.grade_for(c, 10, "rgb24")


def _pq_nits(e):
    m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
    p = e ** (1 / m2)
    return 10000 * (max(p - c1, 0) / (c2 - c3 * p)) ** (1 / m1)


@pytest.mark.parametrize("fmt,top", [("rgbp_u8", 255), ("rgbp_f16", 65535)])
def test_make_grade_properties(v9, fmt, top):
    for tin, pin in (("pq", "bt2020"), ("hlg", "bt2020"), ("bt709", "bt601"), ("srgb", "bt709"), ("linear", "bt709")):
        for tone in ("clip", "reinhard"):
            for tout in ("srgb", "bt709", "linear"):
                g = v9.make_grade(10, fmt, tin, pin, transfer_out=tout, tonemap=tone)
                assert g.out_max == top and g.in_lut.shape == (1024,) and g.out_lut.shape == (4097,)
                assert (np.diff(g.in_lut.astype(int)) >= 0).all() and (np.diff(g.out_lut.astype(int)) >= 0).all()
                assert g.in_lut[0] == 0 and g.out_lut[0] == 0 and g.out_lut.max() <= top
    # PQ: code 0 is 0; the code of peak_nits and everything above it is 65535; below it, the formula +-1
    for peak in (1000, 4000):
        g = v9.make_grade(12, fmt, "pq", "bt2020", peak_nits=peak)
        nits = np.array([_pq_nits(c / 4095) for c in range(4096)])
        assert g.in_lut[0] == 0
        first = int(np.argmax(nits >= peak))
        assert nits[first] >= peak and (g.in_lut[first:] == 65535).all() and g.in_lut[first - 8] < 65535
        want = np.minimum(nits / peak, 1) * 65535
        assert np.abs(g.in_lut.astype(float) - want).max() <= 1
    # the matrix: identity for equal primaries, rows that sum to one (white stays white) otherwise, and
    # BT.2020 -> BT.709 as BT.2087 gives it
    assert np.array_equal(v9.make_grade(8, fmt, "srgb", "bt709").m, 16384 * np.eye(3, dtype=np.int32))
    m = v9.make_grade(10, fmt, "pq", "bt2020").m
    assert (np.abs(m.sum(axis=1) - 16384) <= 2).all()
    bt2087 = np.array([[1.6605, -0.5876, -0.0728], [-0.1246, 1.1329, -0.0083], [-0.0182, -0.1006, 1.1187]])
    assert np.abs(m / 16384 - bt2087).max() < 2e-4
    # the tone curves, from their formulas: reinhard maps the peak to the top and 0 to 0; clip reaches
    # the top at white_nits
    g = v9.make_grade(10, fmt, "pq", "bt2020", transfer_out="linear", peak_nits=1000, white_nits=250, tonemap="reinhard")
    x = np.arange(4097) / 4096 * 4
    assert np.abs(g.out_lut.astype(float) - x * (1 + x / 16) / (1 + x) * top).max() <= 1 and g.out_lut[4096] == top
    g = v9.make_grade(10, fmt, "pq", "bt2020", transfer_out="linear", peak_nits=1000, white_nits=250, tonemap="clip")
    assert np.abs(g.out_lut.astype(float) - np.minimum(x, 1) * top).max() <= 1 and (g.out_lut[1024:] == top).all()
    for kw in (dict(tonemap="bt2390"), dict(transfer_out="pq"), dict(primaries_out="p3"), dict(peak_nits=100)):
        with pytest.raises(ValueError):
            v9.make_grade(10, fmt, "pq", "bt2020", **kw)
    with pytest.raises(ValueError):
        v9.make_grade(10, fmt, "gamma22", "bt709")


def test_srgb_to_srgb_is_the_identity_within_one(v9):
    """Equal transfer and primaries at 8 bits: every code maps to itself +-1 (in_lut is 16 bits,
    the output curve is indexed at 12 and interpolated; sRGB's linear toe keeps the first segment exact
    enough)."""
    codes = np.repeat(np.arange(256)[:, None], 3, axis=1)
    g = v9.make_grade(8, "rgbp_u8", "srgb", "bt709", transfer_out="srgb", primaries_out="bt709")
    v = v9.grade_host(g, codes).astype(int)
    assert np.abs(v - codes).max() <= 1
    g = v9.make_grade(8, "rgbp_f16", "srgb", "bt709")
    v = v9.grade_host(g, codes).astype(float)
    assert np.abs(v / 257 - codes).max() <= 1
