"""The fused box-filter resize of the device output conversion (vp9hip_convert_frames_scaled /
vp9hip_decoder_convert_scaled, the kernel of csrc/vp9hip_convert_scale.hip) against a numpy
restatement of its integer definition (include/vp9hip.h, DESIGN.md "Box-filter resize").
Every comparison is exact, the half output included (its int16 bit patterns).

The restatement shares no code with the library. box(P, ow, oh) of a w x h plane:
weights wx(ox, sx) = max(0, min((ox+1) w, (sx+1) ow) - max(ox w, sx ow)) (wy alike with h, oh)
as matrices, A = Wy @ P @ Wx.T in int64, box = (A + (w h >> 1)) // (w h). Semi-planar resamples
chroma to ((OW + ss_h) >> ss_h, (OH + ss_v) >> ss_v); the RGB formats resample all three
planes to (OW, OH) and then run the conversion's arithmetic (test_gpu_convert.reference) as
for a 4:4:4 source.
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the conversion writes torch tensors and shares their HIP runtime
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_gpu_convert import FORMATS, _colors, _random_planes, _same, frame_bytes, reference
from test_stream import _frames

pytestmark = pytest.mark.gpu

# source size, output size
RATIOS = [((65, 33), (33, 17)),        # just under 2: three taps, odd chroma
          ((65, 33), (7, 5)),          # 11 x 8 taps
          ((16, 16), (40, 23)),        # upscale: two taps
          ((352, 288), (224, 224)),    # another ratio per axis, several output tiles
          ((352, 288), (300, 200)),    # wider than one tile, right and bottom edge tiles
          ((352, 288), (3, 2)),        # the footprint far exceeds any staging buffer
          ((352, 288), (1, 1)),
          ((352, 288), (176, 144))]    # exact 2:1


# ------------------------------------------------------------------ the reference
def _weights(n_src, n_out):
    o, s = np.arange(n_out, dtype=np.int64)[:, None], np.arange(n_src, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((o + 1) * n_src, (s + 1) * n_out) - np.maximum(o * n_src, s * n_out))


def _area_sum(P, ow, oh):
    h, w = P.shape
    return _weights(h, oh) @ P.astype(np.int64) @ _weights(w, ow).T


def box(P, ow, oh):
    h, w = P.shape
    return (_area_sum(P, ow, oh) + (w * h >> 1)) // (w * h)


def _resampled(planes, ow, oh, ssh, ssv):
    """(the semi-planar planes, the RGB formats' planes) of the resized frame."""
    ocw, och = (ow + ssh) >> ssh, (oh + ssv) >> ssv
    y = box(planes[0], ow, oh)
    return ([y, box(planes[1], ocw, och), box(planes[2], ocw, och)],
            [y, box(planes[1], ow, oh), box(planes[2], ow, oh)])


def scaled_reference(planes, fmt, d, ssh, ssv, cs, full, ow, oh, pre=None):
    semi, full_res = pre if pre is not None else _resampled(planes, ow, oh, ssh, ssv)
    if fmt == "semiplanar":
        return reference(semi, fmt, d, ssh, ssv, cs, full)
    return reference(full_res, fmt, d, 0, 0, cs, full)


def test_the_restatement_itself():
    """What the definition promises, checked on the restatement (no library call)."""
    for n_src, n_out in ((65, 33), (33, 7), (16, 40), (288, 224), (352, 1), (7, 7)):
        W = _weights(n_src, n_out)
        assert (W.sum(axis=1) == n_src).all() and (W.sum(axis=0) == n_out).all()
    rng = np.random.default_rng(1)
    P = rng.integers(0, 4096, (33, 65))
    assert np.array_equal(box(P, 65, 33), P)
    assert (box(np.full((33, 65), 1234), 7, 5) == 1234).all()
    assert box(np.array([[1, 2], [3, 4]]), 1, 1)[0, 0] == 3
    assert box(np.array([[1, 2], [3, 3]]), 1, 1)[0, 0] == 2
    assert box(np.array([[1, 2], [2, 2]]), 1, 1)[0, 0] == 2


# ------------------------------------------------------------------ every format, depth, subsampling, ratio
@pytest.mark.parametrize("ss", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("d", [8, 10, 12])
def test_formats_match_the_reference(v9, gpu, d, ss):
    ssh, ssv = ss
    rng = np.random.default_rng(2000 * d + 10 * ssh + ssv)
    for (w, h), (ow, oh) in RATIOS:
        gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
        planes = _random_planes(rng, w, h, d, ssh, ssv)
        gpu.upload(0, planes)
        pre = _resampled(planes, ow, oh, ssh, ssv)
        what = "%dx%d -> %dx%d" % (w, h, ow, oh)
        ocw, och = (ow + ssh) >> ssh, (oh + ssv) >> ssv
        y, uv = gpu.convert([0], "semiplanar", resize=(ow, oh))
        assert y.dtype == (torch.uint8 if d == 8 else torch.int16) and uv.dtype == y.dtype
        assert tuple(y.shape) == (1, oh, ow) and tuple(uv.shape) == (1, och, ocw, 2)
        ry, ruv = scaled_reference(planes, "semiplanar", d, ssh, ssv, 2, 0, ow, oh, pre)
        _same(y[0], ry, "semiplanar Y " + what)
        _same(uv[0], ruv, "semiplanar UV " + what)
        for cs, full in _colors(d, ssh, ssv):
            for fmt, shape, dt in (("rgb24", (1, oh, ow, 3), torch.uint8), ("rgbp_u8", (1, 3, oh, ow), torch.uint8),
                                   ("rgbp_f16", (1, 3, oh, ow), torch.float16)):
                got = gpu.convert([0], fmt, colorspace=cs, full_range=full, resize=(ow, oh))
                assert tuple(got.shape) == shape and got.dtype == dt
                _same(got[0], scaled_reference(planes, fmt, d, ssh, ssv, cs, full, ow, oh, pre),
                      "%s cs %d full %d %s" % (fmt, cs, full, what))


# ------------------------------------------------------------------ rounding: the half goes up, once
def test_half_rounds_up(v9, gpu):
    """2:1 of 2x2 blocks whose sums are 4k, 4k+1, 4k+2 and 4k+3: k, k, k+1, k+1."""
    w = h = 16
    gpu.configure(w, h, 8, nbufs=1, ss_h=0, ss_v=0)
    k = (np.arange(64).reshape(8, 8) * 3 + 1) % 250
    rem = (np.arange(64).reshape(8, 8) + np.arange(8)[:, None]) % 4
    planes, wants = [], []
    for p in range(3):
        r = (rem + p) % 4
        P = np.repeat(np.repeat(k, 2, axis=0), 2, axis=1)
        P[0::2, 1::2] += r >= 1          # the block's sum is 4k + r
        P[1::2, 0::2] += r >= 2
        P[1::2, 1::2] += r >= 3
        planes.append(P.astype(np.uint8))
        wants.append(k + (r >= 2))
        assert np.array_equal(box(P, 8, 8), wants[-1])
    gpu.upload(0, planes)
    y, uv = gpu.convert([0], "semiplanar", resize=(8, 8))
    _same(y[0], wants[0].astype(np.uint8), "Y")
    _same(uv[0], np.stack(wants[1:], axis=-1).astype(np.uint8), "UV")


def test_a_constant_plane_stays_constant(v9, gpu):
    d, val = 10, (1023, 517, 1)
    for (w, h), (ow, oh) in RATIOS:
        gpu.configure(w, h, d, nbufs=1)
        cw, ch = (w + 1) >> 1, (h + 1) >> 1
        planes = [np.full((h, w), val[0], np.uint16), np.full((ch, cw), val[1], np.uint16),
                  np.full((ch, cw), val[2], np.uint16)]
        gpu.upload(0, planes)
        y, uv = gpu.convert([0], "semiplanar", resize=(ow, oh))
        y, uv = y.cpu().numpy().view(np.uint16), uv.cpu().numpy().view(np.uint16)
        what = "%dx%d -> %dx%d" % (w, h, ow, oh)
        assert (y == val[0] << 6).all(), what
        assert (uv[..., 0] == val[1] << 6).all() and (uv[..., 1] == val[2] << 6).all(), what
        got = gpu.convert([0], "rgbp_f16", colorspace=2, resize=(ow, oh))
        flat = [np.full((oh, ow), v, np.int64) for v in val]
        _same(got[0], reference(flat, "rgbp_f16", d, 0, 0, 2, 0), "rgbp_f16 " + what)


# ------------------------------------------------------------------ sums beyond 32 bits
def test_sums_beyond_32_bits(v9, gpu):
    w, h, d = 1280, 832, 12
    rng = np.random.default_rng(64)
    gpu.configure(w, h, d, nbufs=1)
    planes = [rng.integers(4000, 4096, (h, w)).astype(np.uint16), rng.integers(4000, 4096, (h // 2, w // 2)).astype(np.uint16),
              rng.integers(4000, 4096, (h // 2, w // 2)).astype(np.uint16)]
    gpu.upload(0, planes)
    for ow, oh in ((1, 1), (2, 3)):
        assert int(_area_sum(planes[0], ow, oh).min()) > 1 << 32
        pre = _resampled(planes, ow, oh, 1, 1)
        y, uv = gpu.convert([0], "semiplanar", resize=(ow, oh))
        ry, ruv = scaled_reference(planes, "semiplanar", d, 1, 1, 2, 0, ow, oh, pre)
        _same(y[0], ry, "Y %dx%d" % (ow, oh))
        _same(uv[0], ruv, "UV %dx%d" % (ow, oh))
        got = gpu.convert([0], "rgbp_f16", colorspace=4, resize=(ow, oh))
        _same(got[0], scaled_reference(planes, "rgbp_f16", d, 1, 1, 4, 0, ow, oh, pre), "rgbp_f16 %dx%d" % (ow, oh))


# ------------------------------------------------------------------ only the crop contributes
def test_crop_of_a_larger_buffer(v9, gpu):
    rng = np.random.default_rng(5)
    gpu.configure(200, 130, 8, nbufs=1)
    planes = _random_planes(rng, 200, 130, 8, 1, 1)
    gpu.upload(0, planes)
    crop = [planes[0][:33, :65], planes[1][:17, :33], planes[2][:17, :33]]
    pre = _resampled(crop, 33, 17, 1, 1)
    for fmt in ("rgb24", "rgbp_u8", "rgbp_f16"):
        got = gpu.convert([0], fmt, colorspace=1, size=(65, 33), resize=(33, 17))
        _same(got[0], scaled_reference(crop, fmt, 8, 1, 1, 1, 0, 33, 17, pre), fmt)
    y, uv = gpu.convert([0], "semiplanar", size=(65, 33), resize=(33, 17))
    ry, ruv = scaled_reference(crop, "semiplanar", 8, 1, 1, 2, 0, 33, 17, pre)
    _same(y[0], ry, "Y")
    _same(uv[0], ruv, "UV")


# ------------------------------------------------------------------ equal size: the merged kernel's result
@pytest.mark.parametrize("d,ss,size,fmts", [
    (8, (1, 1), (65, 33), ["semiplanar"]),
    (10, (1, 1), (70, 38), FORMATS),
    (8, (1, 1), (16, 16), FORMATS),
    (12, (0, 0), (65, 33), FORMATS),
    (8, (0, 0), (70, 38), FORMATS),
])
def test_equal_size_is_the_unscaled_conversion(v9, gpu, d, ss, size, fmts):
    (w, h), (ssh, ssv) = size, ss
    rng = np.random.default_rng(31 + d + w)
    gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
    gpu.upload(0, _random_planes(rng, w, h, d, ssh, ssv))
    for fmt in fmts:
        for cs, full in [(2, 0)] if fmt == "semiplanar" else _colors(d, ssh, ssv):
            a = gpu.convert([0], fmt, colorspace=cs, full_range=full)
            b = gpu.convert([0], fmt, colorspace=cs, full_range=full, resize=(w, h))
            for x, y in zip(a if fmt == "semiplanar" else (a,), b if fmt == "semiplanar" else (b,)):
                _same(y, x.cpu().numpy(), "%s cs %d %dx%d" % (fmt, cs, w, h))


# ------------------------------------------------------------------ batches, pitches, gaps: nothing else is written
LAYOUTS = [  # fmt, depth, (ss_h, ss_v), pitch, gap after each frame
    ("rgb24", 8, (1, 1), 112, 48),
    ("rgb24", 8, (1, 1), 3 * 33, 13),          # tight: rows at every alignment, frames at odd addresses
    ("rgb24", 8, (1, 1), 3 * 33, 1),
    ("rgbp_u8", 8, (1, 1), 48, 16),
    ("rgbp_u8", 10, (1, 0), 0, 7),             # tight pitch 33
    ("rgbp_f16", 8, (1, 1), 80, 32),
    ("rgbp_f16", 10, (0, 0), 0, 6),            # tight pitch 66: rows 2-byte aligned only
    ("semiplanar", 8, (1, 1), 48, 16),
    ("semiplanar", 8, (1, 1), 0, 3),           # tight pitch 34, frames at odd addresses
    ("semiplanar", 10, (1, 1), 80, 64),
    ("semiplanar", 12, (0, 1), 0, 10),
]


@pytest.mark.parametrize("fmt,d,ss,pitch,gap", LAYOUTS)
def test_batch_layout_and_untouched_bytes(v9, gpu, fmt, d, ss, pitch, gap):
    w, h, ow, oh, (ssh, ssv) = 65, 33, 33, 17, ss
    rng = np.random.default_rng(177 + d + pitch + gap)
    gpu.configure(w, h, d, nbufs=3, ss_h=ssh, ss_v=ssv)
    frames = [_random_planes(rng, w, h, d, ssh, ssv) for _ in range(3)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [2, 0, 1]
    nbytes, pit, offs = v9.out_layout(fmt, ow, oh, d, ssh, ssv, pitch)
    stride = nbytes + gap
    total = 2 * stride + nbytes
    out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    cs, full = (5, 0) if d == 10 else (1, 0)
    res = gpu.convert(order, fmt, colorspace=cs, full_range=full, out=out, pitch=pitch, frame_stride=stride,
                      resize=(ow, oh))
    want = np.full(total + 32, 0xA5, np.uint8)
    for i, b in enumerate(order):
        ref = scaled_reference(frames[b], fmt, d, ssh, ssv, cs, full, ow, oh)
        want[i * stride: i * stride + nbytes] = frame_bytes(ref, fmt, pit, offs, nbytes)
        for g, r in zip(res if fmt == "semiplanar" else (res,), ref if fmt == "semiplanar" else (ref,)):
            _same(g[i], r, "%s frame %d" % (fmt, i))
    got = out.cpu().numpy()
    bad = got != want
    assert not bad.any(), "%d bytes differ, first at %d" % (int(bad.sum()), int(np.argmax(bad)))


def test_more_frames_than_one_launch_takes(v9, gpu):
    """33 frames (repeated buffers), 16x16 -> 8x8: the launches of 32 and 1 land at their own offsets."""
    w, h = 16, 16
    rng = np.random.default_rng(19)
    gpu.configure(w, h, 8, nbufs=2)
    frames = [_random_planes(rng, w, h, 8, 1, 1) for _ in range(2)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [(i * 7 + i // 3) % 2 for i in range(33)]
    got = gpu.convert(order, "rgb24", resize=(8, 8))
    refs = [scaled_reference(p, "rgb24", 8, 1, 1, 2, 0, 8, 8) for p in frames]
    _same(got, np.stack([refs[b] for b in order]), "33 frames")


# ------------------------------------------------------------------ the decoder's frames, with the stream's colour
def test_decoder_convert_resizes(v9):
    w, h = 352, 288
    enc = v9.Stream()
    enc.set_color(1, 1)
    fr = _frames(v9, w, h, 3)
    datas = [enc.encode(fr[0])[0]]
    for i in range(1, 3):
        datas.append(enc.encode(fr[i], ref_slot=(i - 1, 0, i - 1), refresh_mask=1 << i)[0])
    packets = [(data, pts) for pts, data in v9.ivf_read(v9.ivf_write(datas, w, h))[1]]
    dec = v9.Decoder(0, max_batch=4)
    try:
        infos = [info for _, info in dec.decode(packets, download=False)]
        assert len(infos) == 3
        planes = []
        for i in infos:
            pl = v9.alloc_planes(w, h, 8)
            ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pl])
            ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in pl])
            assert v9.lib().vp9hip_download_frame(dec.context(), i.buf, ptrs, ls) == 0
            planes.append(v9.visible(pl, w, h))
        out = torch.full((16,), 0xA5, dtype=torch.uint8, device="cuda")
        with pytest.raises((v9.Vp9HipError, ValueError)):
            dec.convert(infos, "rgbp_f16", out=out, resize=(88, 72))
        with pytest.raises(v9.Vp9HipError):
            dec.convert(infos, "rgbp_f16", resize=(88, 0))
        got = dec.convert(infos, "rgbp_f16", resize=(88, 72))
        assert tuple(got.shape) == (3, 3, 72, 88) and got.dtype == torch.float16
        for k in range(3):
            _same(got[k], scaled_reference(planes[k], "rgbp_f16", 8, 1, 1, 1, 1, 88, 72), "frame %d" % k)
        with pytest.raises(v9.Vp9HipError):        # convert released the buffers
            dec.release(infos[0].buf)
    finally:
        dec.close()


# ------------------------------------------------------------------ errors: refused before anything is written
def test_errors_write_nothing(v9, gpu):
    w, h = 65, 33
    gpu.configure(w, h, 8, nbufs=3)
    out = torch.full((3 * 4 * 80 * 40,), 0xA5, dtype=torch.uint8, device="cuda")
    for resize in ((0, 5), (5, 16385), (-1, 5), (5, 0)):
        with pytest.raises(v9.Vp9HipError) as e:
            gpu.convert([0], "rgb24", out=out, resize=resize)
        assert e.value.code == v9.EINVAL, resize
    small = torch.full((3 * 33 * 17 - 1,), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises((v9.Vp9HipError, ValueError)):
        gpu.convert([0], "rgb24", out=small, resize=(33, 17))
    cases = [dict(bufs=[0, 3]), dict(bufs=[-1]), dict(bufs=[0], size=(w + 1, h)), dict(bufs=[0], colorspace=0),
             dict(bufs=[0], pitch=64), dict(bufs=[0, 1], frame_stride=100)]
    for kw in cases:
        kw = dict(kw)
        with pytest.raises(v9.Vp9HipError) as e:
            gpu.convert(kw.pop("bufs"), "rgb24", out=out, resize=(33, 17), **kw)
        assert e.value.code == v9.EINVAL, kw
    L = v9.lib()
    d = v9.OutDesc(v9.OUT_FORMATS["rgb24"], 2, 0, w, h, 0, 0)
    one = (ctypes.c_int * 1)(0)
    for ow, oh in ((0, 5), (5, 16385), (16385, 5), (5, 0), (-3, 5)):
        assert L.vp9hip_convert_frames_scaled(gpu._c, one, 1, ctypes.byref(d), ow, oh, out.data_ptr(), None) == v9.EINVAL
    assert L.vp9hip_convert_frames_scaled(gpu._c, one, 0, ctypes.byref(d), 33, 17, out.data_ptr(), None) == v9.EINVAL
    assert L.vp9hip_convert_frames_scaled(gpu._c, one, 1, ctypes.byref(d), 33, 17, None, None) == v9.EINVAL
    d16 = v9.OutDesc(v9.OUT_FORMATS["rgbp_f16"], 2, 0, w, h, 0, 0)
    assert L.vp9hip_convert_frames_scaled(gpu._c, one, 1, ctypes.byref(d16), 33, 17, out.data_ptr() + 1, None) == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((small == 0xA5).all())
