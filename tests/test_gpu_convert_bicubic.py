"""The fused bicubic resampling of the device output conversion (vp9hip_convert_frames_bicubic /
vp9hip_decoder_convert_bicubic, the kernel of csrc/vp9hip_convert_cubic.hip): the whole picture,
a source and a destination rectangle per frame, the fill, the clip. Every comparison is exact,
the half output included (its int16 bit patterns), against the numpy restatement of
tests/test_bicubic_definition.py (which shares no code with the library) followed by the
conversion's reference of tests/test_gpu_convert.py.
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the conversion writes torch tensors and shares their HIP runtime
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_bicubic_definition import resample, resampled_planes, step_edge, sums, unclipped
from test_gpu_convert import FORMATS, _colors, _random_planes, _same, frame_bytes, reference
from test_gpu_convert_resample import _check_frames, convert_reference
from test_resample_definition import default_fill
from test_stream import _frames

pytestmark = pytest.mark.gpu

SIZE = (66, 34)
OUTS = [(40, 24), (33, 17), (131, 67), (1, 1)]          # down (twice), up across two tiles, everything to one sample


# ------------------------------------------------------------------ 1. every format, depth, subsampling
@pytest.mark.parametrize("ss", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("d", [8, 10, 12])
def test_formats_match_the_reference(v9, gpu, d, ss):
    (w, h), (ssh, ssv) = SIZE, ss
    rng = np.random.default_rng(5000 * d + 10 * ssh + ssv)
    gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
    planes = _random_planes(rng, w, h, d, ssh, ssv)
    gpu.upload(0, planes)
    for ow, oh in OUTS:
        pre = resampled_planes(planes, ow, oh, d, ssh, ssv)
        what = "%dx%d -> %dx%d" % (w, h, ow, oh)
        ocw, och = (ow + ssh) >> ssh, (oh + ssv) >> ssv
        y, uv = gpu.convert([0], "semiplanar", resize=(ow, oh), filter="bicubic")
        assert y.dtype == (torch.uint8 if d == 8 else torch.int16) and uv.dtype == y.dtype
        assert tuple(y.shape) == (1, oh, ow) and tuple(uv.shape) == (1, och, ocw, 2)
        _check_frames((y, uv), [convert_reference(pre, "semiplanar", d, ssh, ssv, 2, 0)], "semiplanar", what)
        for cs, full in _colors(d, ssh, ssv):           # colour space 7 (pass-through) for 4:4:4
            for fmt, shape, dt in (("rgb24", (1, oh, ow, 3), torch.uint8), ("rgbp_u8", (1, 3, oh, ow), torch.uint8),
                                   ("rgbp_f16", (1, 3, oh, ow), torch.float16)):
                got = gpu.convert([0], fmt, colorspace=cs, full_range=full, resize=(ow, oh), filter="bicubic")
                assert tuple(got.shape) == shape and got.dtype == dt
                _same(got[0], convert_reference(pre, fmt, d, ssh, ssv, cs, full), "%s cs %d full %d %s" % (fmt, cs, full, what))


# ------------------------------------------------------------------ 2. equal size: the unscaled conversion
@pytest.mark.parametrize("d,ss,size,fmts", [
    (8, (1, 1), (65, 33), ["semiplanar"]),
    (10, (1, 0), (70, 38), ["semiplanar"]),
    (12, (0, 0), (65, 33), FORMATS),
    (8, (0, 0), (130, 38), FORMATS),
])
def test_equal_size_is_the_unscaled_conversion(v9, gpu, d, ss, size, fmts):
    """Every plane that keeps its size is copied: all of them for semi-planar, and for the RGB
    formats of a 4:4:4 source."""
    (w, h), (ssh, ssv) = size, ss
    rng = np.random.default_rng(43 + d + w)
    gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
    gpu.upload(0, _random_planes(rng, w, h, d, ssh, ssv))
    for fmt in fmts:
        for cs, full in [(2, 0)] if fmt == "semiplanar" else _colors(d, ssh, ssv):
            a = gpu.convert([0], fmt, colorspace=cs, full_range=full)
            b = gpu.convert([0], fmt, colorspace=cs, full_range=full, resize=(w, h), filter="bicubic")
            for x, y in zip(a if fmt == "semiplanar" else (a,), b if fmt == "semiplanar" else (b,)):
                _same(y, x.cpu().numpy(), "%s cs %d %dx%d" % (fmt, cs, w, h))


# ------------------------------------------------------------------ 3. a constant plane stays constant
@pytest.mark.parametrize("val", [(0, 0, 0), (1023, 1023, 1023), (1023, 517, 1)])
def test_a_constant_plane_stays_constant(v9, gpu, val):
    d, (w, h) = 10, SIZE
    gpu.configure(w, h, d, nbufs=1)
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    gpu.upload(0, [np.full((h, w), val[0], np.uint16), np.full((ch, cw), val[1], np.uint16), np.full((ch, cw), val[2], np.uint16)])
    for ow, oh in OUTS + [(66, 40)]:
        y, uv = gpu.convert([0], "semiplanar", resize=(ow, oh), filter="bicubic")
        y, uv = y.cpu().numpy().view(np.uint16), uv.cpu().numpy().view(np.uint16)
        what = "%dx%d -> %dx%d" % (w, h, ow, oh)
        assert (y == val[0] << 6).all(), what
        assert (uv[..., 0] == val[1] << 6).all() and (uv[..., 1] == val[2] << 6).all(), what
        got = gpu.convert([0], "rgbp_f16", colorspace=2, resize=(ow, oh), filter="bicubic")
        flat = [np.full((oh, ow), v, np.int64) for v in val]
        _same(got[0], reference(flat, "rgbp_f16", d, 0, 0, 2, 0), "rgbp_f16 " + what)


# ------------------------------------------------------------------ 4. the step edge: the clip, both ways
@pytest.mark.parametrize("d", [8, 12])
def test_the_step_edge_clips(v9, gpu, d):
    (w, h), top = SIZE, (1 << d) - 1
    dt = np.uint8 if d == 8 else np.uint16
    gpu.configure(w, h, d, nbufs=1, ss_h=0, ss_v=0)
    edge = step_edge(w, h, d).astype(dt)
    planes = [edge, edge[::-1].copy(), edge[:, ::-1].copy()]
    gpu.upload(0, planes)
    for ow, oh in ((131, 67), (40, 24)):
        raw = unclipped(planes[0], ow, oh)
        assert (raw < 0).sum() > 0 and (raw > top).sum() > 0         # the reference's unclipped value leaves the range
        y, uv = gpu.convert([0], "semiplanar", resize=(ow, oh), filter="bicubic")
        sh = 0 if d == 8 else 16 - d
        got = y[0].cpu().numpy().view(dt).astype(np.int64) >> sh
        assert (got[raw < 0] == 0).all() and (got[raw > top] == top).all()
        assert np.array_equal(got, resample(planes[0], ow, oh, d))
        pre = resampled_planes(planes, ow, oh, d, 0, 0)
        _check_frames((y, uv), [convert_reference(pre, "semiplanar", d, 0, 0, 2, 0)], "semiplanar", "%dx%d" % (ow, oh))
        got = gpu.convert([0], "rgbp_f16", colorspace=7, full_range=1, resize=(ow, oh), filter="bicubic")
        _same(got[0], convert_reference(pre, "rgbp_f16", d, 0, 0, 7, 1), "rgbp_f16 %dx%d" % (ow, oh))


# ------------------------------------------------------------------ 5. sums beyond 32 bits
def test_sums_beyond_32_bits(v9, gpu):
    w, h, d = 2048, 1088, 12
    gpu.configure(w, h, d, nbufs=1)
    planes = [np.full((h, w), 4095, np.uint16), np.full((h // 2, w // 2), 4095, np.uint16), np.full((h // 2, w // 2), 4095, np.uint16)]
    gpu.upload(0, planes)
    ow, oh = 3, 2
    assert int(sums(planes[0], ow, oh)[0].min()) > 1 << 32
    pre = resampled_planes(planes, ow, oh, d, 1, 1)
    assert (pre[0][0] == 4095).all()
    got = gpu.convert([0], "semiplanar", resize=(ow, oh), filter="bicubic")
    _check_frames(got, [convert_reference(pre, "semiplanar", d, 1, 1, 2, 0)], "semiplanar", "3x2")
    got = gpu.convert([0], "rgbp_f16", colorspace=4, resize=(ow, oh), filter="bicubic")
    _same(got[0], convert_reference(pre, "rgbp_f16", d, 1, 1, 4, 0), "rgbp_f16 3x2")
    # random samples through the same sums
    rng = np.random.default_rng(64)
    planes = [rng.integers(3000, 4096, (h, w)).astype(np.uint16), rng.integers(0, 4096, (h // 2, w // 2)).astype(np.uint16),
              rng.integers(0, 4096, (h // 2, w // 2)).astype(np.uint16)]
    gpu.upload(0, planes)
    pre = resampled_planes(planes, ow, oh, d, 1, 1)
    got = gpu.convert([0], "semiplanar", resize=(ow, oh), filter="bicubic")
    _check_frames(got, [convert_reference(pre, "semiplanar", d, 1, 1, 2, 0)], "semiplanar", "3x2 random")


def test_more_rows_than_the_weight_table_holds(v9, gpu):
    """A row with more than 512 taps rebuilds its vertical weights per block of source rows."""
    w, h, d = 24, 1300, 8
    rng = np.random.default_rng(65)
    gpu.configure(w, h, d, nbufs=1)
    planes = _random_planes(rng, w, h, d, 1, 1)
    gpu.upload(0, planes)
    for ow, oh in ((5, 2), (24, 1)):
        pre = resampled_planes(planes, ow, oh, d, 1, 1)
        got = gpu.convert([0], "semiplanar", resize=(ow, oh), filter="bicubic")
        _check_frames(got, [convert_reference(pre, "semiplanar", d, 1, 1, 2, 0)], "semiplanar", "%dx%d" % (ow, oh))
        got = gpu.convert([0], "rgb24", colorspace=1, resize=(ow, oh), filter="bicubic")
        _same(got[0], convert_reference(pre, "rgb24", d, 1, 1, 1, 0), "rgb24 %dx%d" % (ow, oh))


# ------------------------------------------------------------------ 6. source rectangles
SRC_RECTS = [(0, 0, 200, 130), (2, 4, 65, 33), (198, 128, 2, 2), (0, 0, 1, 1), (64, 0, 64, 64), (6, 2, 131, 97), (190, 120, 9, 9)]


@pytest.mark.parametrize("d,ss", [(8, (1, 1)), (10, (0, 0)), (8, (1, 0))])
def test_source_rectangles(v9, gpu, d, ss):
    w, h, (ssh, ssv) = 200, 130, ss
    rng = np.random.default_rng(710 + d + ssh)
    gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
    planes = _random_planes(rng, w, h, d, ssh, ssv)
    gpu.upload(0, planes)
    cs, full = (5, 0) if d == 10 else (1, 1)
    for ow, oh in ((33, 17), (40, 23)):
        pres = [resampled_planes(planes, ow, oh, d, ssh, ssv, src=r) for r in SRC_RECTS]
        for fmt in FORMATS:
            got = gpu.convert([0] * len(SRC_RECTS), fmt, colorspace=cs, full_range=full, resize=(ow, oh), filter="bicubic",
                              src_rects=SRC_RECTS)
            _check_frames(got, [convert_reference(p, fmt, d, ssh, ssv, cs, full) for p in pres], fmt, "%s -> %dx%d" % (fmt, ow, oh))
    # one rectangle is every frame's
    got = gpu.convert([0, 0], "rgb24", resize=(33, 17), filter="bicubic", src_rects=SRC_RECTS[5])
    ref = convert_reference(resampled_planes(planes, 33, 17, d, ssh, ssv, src=SRC_RECTS[5]), "rgb24", d, ssh, ssv, 2, 0)
    _check_frames(got, [ref, ref], "rgb24", "broadcast")


# ------------------------------------------------------------------ 7. nothing outside the rectangle contributes
@pytest.mark.parametrize("d", [8, 12])
def test_nothing_outside_the_rectangle_contributes(v9, gpu, d):
    """The same bytes whatever lies outside the rectangle: the rest of the picture and the
    buffer's padding (filled before the upload) at the largest code, then at zero."""
    w, h = 200, 130
    gpu.configure(w, h, d, nbufs=1)
    dt, top = (np.uint8 if d == 8 else np.uint16), (1 << d) - 1
    rng = np.random.default_rng(720 + d)
    inner = _random_planes(rng, w, h, d, 1, 1)
    for rect in ((6, 2, 131, 97), (64, 64, 8, 8), (198, 128, 2, 2)):
        x, y, rw, rh = rect
        cx, cy, cw, ch = x >> 1, y >> 1, (rw + 1) >> 1, (rh + 1) >> 1
        results = []
        for poison, byte in ((top, 0xFF), (0, 0)):
            planes = [np.full((h, w), poison, dt), np.full((h // 2, w // 2), poison, dt), np.full((h // 2, w // 2), poison, dt)]
            planes[0][y:y + rh, x:x + rw] = inner[0][y:y + rh, x:x + rw]
            for p in (1, 2):
                planes[p][cy:cy + ch, cx:cx + cw] = inner[p][cy:cy + ch, cx:cx + cw]
            gpu.fill(0, 1, byte)
            gpu.upload(0, planes)
            results.append([gpu.convert([0], fmt, colorspace=1, resize=size, filter="bicubic", src_rects=rect)
                            for size in ((33, 17), (40, 23), (150, 100)) for fmt in ("semiplanar", "rgbp_f16")])
        i = 0
        for size in ((33, 17), (40, 23), (150, 100)):
            pre = resampled_planes(inner, size[0], size[1], d, 1, 1, src=rect)
            for fmt in ("semiplanar", "rgbp_f16"):
                for got in (results[0][i], results[1][i]):
                    _check_frames(got, [convert_reference(pre, fmt, d, 1, 1, 1, 0)], fmt, "%s %s -> %dx%d" % (rect, fmt, size[0], size[1]))
                i += 1


# ------------------------------------------------------------------ 8. a rectangle per frame, across the launch boundary
def test_rectangles_per_frame_across_launches(v9, gpu):
    """33 outputs from 2 buffers, 16x16 -> 8x8: the launches of 32 and 1 take their own rectangles."""
    w, h = 16, 16
    rng = np.random.default_rng(31)
    gpu.configure(w, h, 8, nbufs=2)
    frames = [_random_planes(rng, w, h, 8, 1, 1) for _ in range(2)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [(i * 7 + i // 3) % 2 for i in range(33)]
    rects = [(2 * (i % 4), 2 * (i % 3), 4 + i % 7, 3 + i % 9) for i in range(33)]
    assert len(set(rects)) == 33
    for fmt in ("rgb24", "semiplanar"):
        got = gpu.convert(order, fmt, resize=(8, 8), filter="bicubic", src_rects=rects)
        refs = [convert_reference(resampled_planes(frames[b], 8, 8, 8, 1, 1, src=r), fmt, 8, 1, 1, 2, 0) for b, r in zip(order, rects)]
        _check_frames(got, refs, fmt, fmt)


# ------------------------------------------------------------------ 9. letterbox: picture, fill, and nothing else
DST_RECTS = [(4, 2, 30, 17), (0, 0, 40, 23), (38, 22, 2, 1), (0, 0, 1, 1)]


def test_letterbox_rect_places_the_picture(v9, gpu):
    w, h, ow, oh = 66, 34, 48, 48
    rng = np.random.default_rng(77)
    gpu.configure(w, h, 8, nbufs=1)
    planes = _random_planes(rng, w, h, 8, 1, 1)
    gpu.upload(0, planes)
    for fmt, align in (("rgbp_u8", (1, 1)), ("semiplanar", (2, 2))):
        rect = v9.letterbox_rect(w, h, ow, oh, align)
        assert rect[2] == ow and rect[3] < oh
        got = gpu.convert([0], fmt, colorspace=1, resize=(ow, oh), filter="bicubic", dst_rects=rect)
        pre = resampled_planes(planes, ow, oh, 8, 1, 1, dst=rect, fill=default_fill(8, 1, 0))
        _check_frames(got, [convert_reference(pre, fmt, 8, 1, 1, 1, 0)], fmt, fmt)


@pytest.mark.parametrize("src", [None, (2, 4, 33, 17)])
@pytest.mark.parametrize("fill", [None, "arbitrary"])
@pytest.mark.parametrize("d,ss", [(8, (1, 1)), (10, (0, 0))])
@pytest.mark.parametrize("fmt", FORMATS)
def test_letterbox_writes_picture_and_fill_only(v9, gpu, fmt, d, ss, fill, src):
    w, h, ow, oh, (ssh, ssv) = 65, 33, 40, 23, ss
    rng = np.random.default_rng(910 + d + len(fmt))
    gpu.configure(w, h, d, nbufs=2, ss_h=ssh, ss_v=ssv)
    frames = [_random_planes(rng, w, h, d, ssh, ssv) for _ in range(2)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [1, 0, 0, 1]
    cs, full = (7, 1) if (d == 10 and fmt == "rgbp_u8") else (5, 0) if d == 10 else (1, 1)
    codes = default_fill(d, cs, full) if fill is None else (3 << (d - 8), 200 << (d - 8), (1 << d) - 1)
    tight = v9.out_layout(fmt, ow, oh, d, ssh, ssv)[1]
    pitch = (tight + 15) // 16 * 16 + 16
    nbytes, pit, offs = v9.out_layout(fmt, ow, oh, d, ssh, ssv, pitch)
    stride = nbytes + 38
    total = 3 * stride + nbytes
    out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    res = gpu.convert(order, fmt, colorspace=cs, full_range=full, out=out, pitch=pitch, frame_stride=stride,
                      resize=(ow, oh), filter="bicubic", src_rects=src, dst_rects=DST_RECTS,
                      fill=None if fill is None else codes)
    want = np.full(total + 32, 0xA5, np.uint8)
    refs = []
    for i, b in enumerate(order):
        pre = resampled_planes(frames[b], ow, oh, d, ssh, ssv, src=src, dst=DST_RECTS[i], fill=codes)
        refs.append(convert_reference(pre, fmt, d, ssh, ssv, cs, full))
        want[i * stride: i * stride + nbytes] = frame_bytes(refs[-1], fmt, pit, offs, nbytes)
    _check_frames(res, refs, fmt, fmt)
    got = out.cpu().numpy()
    bad = got != want
    assert not bad.any(), "%d bytes differ, first at %d" % (int(bad.sum()), int(np.argmax(bad)))


# ------------------------------------------------------------------ 10. the decoder's frames
def test_decoder_convert_bicubic(v9):
    w, h = 352, 288
    enc = v9.Stream()
    enc.set_color(1, 1)
    fr = _frames(v9, w, h, 2)
    datas = [enc.encode(fr[0])[0], enc.encode(fr[1], ref_slot=(0, 0, 0), refresh_mask=2)[0]]
    packets = [(data, pts) for pts, data in v9.ivf_read(v9.ivf_write(datas, w, h))[1]]
    dec = v9.Decoder(0, max_batch=4)
    try:
        infos = [info for _, info in dec.decode(packets, download=False)]
        assert len(infos) == 2
        planes = []
        for i in infos:
            pl = v9.alloc_planes(w, h, 8)
            ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pl])
            ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in pl])
            assert v9.lib().vp9hip_download_frame(dec.context(), i.buf, ptrs, ls) == 0
            planes.append(v9.visible(pl, w, h))
        with pytest.raises(ValueError):
            dec.convert(infos, "rgbp_f16", filter="bicubic")
        with pytest.raises(v9.Vp9HipError):
            dec.convert(infos, "rgbp_f16", resize=(88, 72), filter="bicubic", src_rects=(32, 16, 256, 280))
        rect = (32, 16, 256, 240)
        got = dec.convert(infos, "rgbp_f16", resize=(88, 72), filter="bicubic", src_rects=rect)
        assert tuple(got.shape) == (2, 3, 72, 88) and got.dtype == torch.float16
        for k in range(2):
            pre = resampled_planes(planes[k], 88, 72, 8, 1, 1, src=rect)
            _same(got[k], convert_reference(pre, "rgbp_f16", 8, 1, 1, 1, 1), "frame %d" % k)
        with pytest.raises(v9.Vp9HipError):        # convert released the buffers
            dec.release(infos[0].buf)
    finally:
        dec.close()


# ------------------------------------------------------------------ 11. errors: refused before anything is written
def test_errors_write_nothing(v9, gpu):
    w, h, ow, oh = 66, 34, 40, 24
    L = v9.lib()
    gpu.configure(w, h, 8, nbufs=2)
    out = torch.full((34 * 4 * 48 * 24,), 0xA5, dtype=torch.uint8, device="cuda")      # 33 frames of any format, and slack
    one, two = (ctypes.c_int * 1)(0), (ctypes.c_int * 2)(0, 1)
    many = (ctypes.c_int * 33)(*[i % 2 for i in range(33)])
    torch.cuda.synchronize()                        # the direct calls below run on the context's own stream

    def call(fmt="rgb24", filt=2, size=(ow, oh), src=None, dst=None, fill=(0, 0, 0), bufs=one, rs=True, entry="vp9hip_convert_frames_bicubic"):
        desc = v9.OutDesc(v9.OUT_FORMATS[fmt], 2, 0, w, h, 0, 0)
        r = v9.Resample(filt, size[0], size[1])
        if src is not None:
            r._s = (v9.Rect * len(src))(*[v9.Rect(*x) for x in src])
            r.src_rects = ctypes.cast(r._s, ctypes.POINTER(v9.Rect))
        if dst is not None:
            r._d = (v9.Rect * len(dst))(*[v9.Rect(*x) for x in dst])
            r.dst_rects = ctypes.cast(r._d, ctypes.POINTER(v9.Rect))
        r.fill[:] = fill
        return getattr(L, entry)(gpu._c, bufs, len(bufs), ctypes.byref(desc), ctypes.byref(r) if rs else None, out.data_ptr(), None)

    bad = [dict(filt=0), dict(filt=1), dict(filt=3), dict(filt=-1), dict(rs=False),
           dict(src=[(0, 0, w + 1, h)]), dict(src=[(2, 0, w - 1, h)]), dict(src=[(0, 2, w, h - 1)]),   # past the visible size
           dict(src=[(0, 0, 0, 8)]), dict(src=[(0, 0, 8, 0)]), dict(src=[(-2, 0, 8, 8)]),
           dict(src=[(1, 0, 8, 8)]), dict(src=[(0, 1, 8, 8)]),                                         # odd x / y at 4:2:0
           dict(bufs=two, src=[(0, 0, 8, 8), (0, 0, w, h + 1)]),                                       # the second frame's
           dict(bufs=many, src=[(0, 0, 8, 8)] * 32 + [(0, 0, w, h + 1)]),      # the second launch's: nothing of the first is written
           dict(bufs=many, dst=[(0, 0, 8, 8)] * 32 + [(0, 0, ow + 1, 8)]),
           dict(bufs=many, fmt="semiplanar", dst=[(0, 0, 8, 8)] * 32 + [(1, 0, 8, 8)]),
           dict(dst=[(0, 0, ow, oh)], fill=(256, 0, 0)), dict(dst=[(0, 0, ow, oh)], fill=(0, 0, 256)),
           dict(dst=[(0, 0, ow, oh)], fill=(0, -1, 0)),
           dict(dst=[(0, 0, ow + 1, oh)]), dict(dst=[(1, 0, ow, oh)]), dict(dst=[(0, 4, ow, oh - 3)]),  # past the output
           dict(dst=[(0, 0, 0, 4)]), dict(dst=[(0, 0, 4, 0)]), dict(dst=[(0, -2, 4, 4)]),
           dict(fmt="semiplanar", dst=[(1, 0, 8, 8)]), dict(fmt="semiplanar", dst=[(0, 3, 8, 8)]),      # odd dx / dy, semi-planar 4:2:0
           dict(size=(0, oh)), dict(size=(16385, oh)), dict(size=(ow, 0)), dict(size=(ow, 16385)),
           dict(entry="vp9hip_convert_frames_resampled")]                                                # the old entry still refuses 2
    for kw in bad:
        assert call(**kw) == v9.EINVAL, kw
    # what convert_args refuses is refused here too
    desc = v9.OutDesc(v9.OUT_FORMATS["rgb24"], 0, 0, w, h, 0, 0)
    rs = v9.Resample(2, ow, oh)
    assert L.vp9hip_convert_frames_bicubic(gpu._c, one, 1, ctypes.byref(desc), ctypes.byref(rs), out.data_ptr(), None) == v9.EINVAL
    desc.colorspace = 2
    assert L.vp9hip_convert_frames_bicubic(gpu._c, one, 0, ctypes.byref(desc), ctypes.byref(rs), out.data_ptr(), None) == v9.EINVAL
    assert L.vp9hip_convert_frames_bicubic(gpu._c, one, 1, ctypes.byref(desc), ctypes.byref(rs), None, None) == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())                # every refusal above came before the first launch
    # an odd dx is fine for the RGB formats: the control that the calls above were refused for their reason
    assert call(dst=[(1, 3, 8, 8)], fill=(16, 128, 128)) == 0
    torch.cuda.synchronize()
    assert not bool((out[:3 * ow * oh] == 0xA5).all())
    out.fill_(0xA5)
    # the Python layer: the arguments need resize, and unknown names are refused there
    for kw in (dict(filter="bicubic"), dict(resize=(ow, oh), filter="lanczos"), dict(resize=(ow, oh), filter="cubic"),
               dict(resize=(ow, oh), filter="bicubic", src_rects=[(0, 0, 8, 8)] * 2)):
        with pytest.raises(ValueError):
            gpu.convert([0], "rgb24", out=out, **kw)
    with pytest.raises(v9.Vp9HipError) as e:
        gpu.convert([0], "rgb24", out=out, resize=(ow, oh), filter="bicubic", src_rects=(0, 0, w, h + 2))
    assert e.value.code == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # the bound: 7680x4320 at 12 bits -> 2x2 is over it (no upload, no launch), -> 4x4 under it
    gpu.configure(7680, 4320, 12, nbufs=1)
    gpu.fill(0, 1, 0)
    desc = v9.OutDesc(v9.OUT_FORMATS["rgbp_f16"], 2, 0, 7680, 4320, 0, 0)
    for size in ((1, 1), (2, 2)):
        rs = v9.Resample(2, size[0], size[1])
        assert L.vp9hip_convert_frames_bicubic(gpu._c, one, 1, ctypes.byref(desc), ctypes.byref(rs), out.data_ptr(), None) == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    rs = v9.Resample(2, 4, 4)
    gpu.sync()
    assert L.vp9hip_convert_frames_bicubic(gpu._c, one, 1, ctypes.byref(desc), ctypes.byref(rs), out.data_ptr(), None) == 0
    gpu.sync()
    torch.cuda.synchronize()
    assert not bool((out[:3 * 4 * 4 * 2] == 0xA5).all()) and bool((out[3 * 4 * 4 * 2:] == 0xA5).all())
    gpu.configure(16, 16, 8, nbufs=1)               # give the memory back
