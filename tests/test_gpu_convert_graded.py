"""The graded output of the device conversion (vp9hip_convert_frames_graded /
vp9hip_decoder_convert_graded, the graded instantiations of k_convert_resample and
k_convert_cubic). The reference is the ungraded R, G, B codes at the source's depth from the
restatements the ungraded tests hold (tests/test_gpu_convert.py's matrix over the resampled planes
of tests/test_resample_definition.py / tests/test_bicubic_definition.py), then grade_host, which
tests/test_grade_definition.py holds to numpy. Every comparison is exact, the half output
included (its int16 bit patterns).

The tables are seeded random u16, not curves, so an index or packing mistake shows anywhere; the
matrix has negative off-diagonal terms and row gains above 1, and every reference of a random
picture asserts that its matrix stage clips at 0 and at 65535 for at least 1 % of samples each (a
frame that is one fill triple, and the decoder's synthetic frames, cannot promise that).
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the conversion writes torch tensors and shares their HIP runtime
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_gpu_convert import _random_planes, _rgb, _same, frame_bytes
from test_gpu_convert_bicubic import resampled_planes as cubic_planes
from test_gpu_convert_resample import resampled_planes
from test_stream import _frames

pytestmark = pytest.mark.gpu

RGB_FORMATS = ("rgb24", "rgbp_u8", "rgbp_f16")
FILTERS = ("box", "triangle", "bicubic")
M = np.array([[30000, -9000, -2500], [-7000, 34000, -6000], [-1500, -12000, 36000]], np.int64)
_tables = {}


def tables(d, fmt):
    """The test grade of depth d and fmt's out_max: (in_lut, m, out_lut), made once."""
    top = 65535 if fmt == "rgbp_f16" else 255
    if (d, top) not in _tables:
        rng = np.random.default_rng(4200 + d + top)
        _tables[d, top] = (rng.integers(0, 65536, 1 << d), M, rng.integers(0, top + 1, 4097))
    return _tables[d, top]


def device_grade(v9, dev, d, fmt):
    return dev.grade(v9.Grade(d, fmt, *tables(d, fmt)))


def pre_planes(planes, ow, oh, filt, d, ssh, ssv, **kw):
    """The three planes at the output size, before the matrix (the RGB formats' side)."""
    if filt == "bicubic":
        return cubic_planes(planes, ow, oh, d, ssh, ssv, **kw)[1]
    return resampled_planes(planes, ow, oh, filt, ssh, ssv, **kw)[1]


def graded_reference(v9, full_res, fmt, d, cs, full, clips=True):
    """One frame as Device.convert(grade=...) returns it, from the three output-size planes."""
    in_lut, m, out_lut = tables(d, fmt)
    codes = np.stack(_rgb(full_res, d, 0, 0, cs, full, d), axis=-1)          # the ungraded codes at out_bits = d
    if clips:
        P = (np.asarray(in_lut)[codes] @ np.asarray(m).T + 8192) >> 14
        assert (P < 0).mean() >= .01 and (P > 65535).mean() >= .01, ((P < 0).mean(), (P > 65535).mean())
    v = v9.grade_host(v9.Grade(d, fmt, in_lut, m, out_lut), codes)
    if fmt == "rgb24":
        return v.astype(np.uint8)
    v = np.ascontiguousarray(v.transpose(2, 0, 1))
    if fmt == "rgbp_u8":
        return v.astype(np.uint8)
    return (v.astype(np.float32) * np.float32(1.0 / 65535)).astype(np.float16)


# ------------------------------------------------------------------ 1. formats, depths, filters
@pytest.mark.parametrize("fmt", RGB_FORMATS)
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("d,ss,cs,full", [(8, (1, 1), 1, 0), (10, (1, 1), 5, 0), (12, (1, 1), 2, 1), (10, (0, 0), 5, 0),
                                         (10, (0, 0), 7, 1)])
def test_formats_depths_filters(v9, gpu, d, ss, cs, full, filt, fmt):
    (w, h), (ow, oh), (ssh, ssv) = (70, 38), (24, 16), ss
    rng = np.random.default_rng(10 * d + ssh + cs)
    gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
    planes = _random_planes(rng, w, h, d, ssh, ssv)
    gpu.upload(0, planes)
    g = device_grade(v9, gpu, d, fmt)
    got = gpu.convert([0], fmt, colorspace=cs, full_range=full, resize=(ow, oh), filter=filt, grade=g)
    assert tuple(got.shape) == ((1, oh, ow, 3) if fmt == "rgb24" else (1, 3, oh, ow))
    assert got.dtype == (torch.float16 if fmt == "rgbp_f16" else torch.uint8)
    ref = graded_reference(v9, pre_planes(planes, ow, oh, filt, d, ssh, ssv), fmt, d, cs, full)
    _same(got[0], ref, "%s %s %d bits cs %d" % (fmt, filt, d, cs))


# ------------------------------------------------------------------ 2. the visible size
@pytest.mark.parametrize("fmt", RGB_FORMATS)
def test_visible_size(v9, gpu, fmt):
    """resize=None: the box filter at equal size, the identity; 4:2:0 chroma doubles exactly, so the
    codes are the unscaled conversion's (nearest chroma sample)."""
    w, h, d = 70, 38, 10
    rng = np.random.default_rng(21)
    gpu.configure(w, h, d, nbufs=1)
    planes = _random_planes(rng, w, h, d, 1, 1)
    gpu.upload(0, planes)
    up = [planes[0]] + [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in planes[1:]]
    got = gpu.convert([0], fmt, colorspace=5, grade=device_grade(v9, gpu, d, fmt))
    _same(got[0], graded_reference(v9, up, fmt, d, 5, 0), fmt)


# ------------------------------------------------------------------ 3. letterbox: picture, graded fill, nothing else
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("fmt", RGB_FORMATS)
def test_letterbox_fill_pitch_and_gaps(v9, gpu, fmt, filt):
    w, h, d, ow, oh = 70, 38, 10, 32, 32
    rng = np.random.default_rng(33)
    gpu.configure(w, h, d, nbufs=2)
    frames = [_random_planes(rng, w, h, d, 1, 1) for _ in range(2)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order, rects = [1, 0, 1], [(3, 7, 26, 14), (0, 0, 32, 32), (30, 31, 2, 1)]
    codes = (300, 811, 97)                                  # not black
    tight = v9.out_layout(fmt, ow, oh, d, 1, 1)[1]
    pitch = (tight + 15) // 16 * 16 + 16
    nbytes, pit, offs = v9.out_layout(fmt, ow, oh, d, 1, 1, pitch)
    stride = nbytes + 38
    total = 2 * stride + nbytes
    out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    res = gpu.convert(order, fmt, colorspace=5, out=out, pitch=pitch, frame_stride=stride, resize=(ow, oh), filter=filt,
                      dst_rects=rects, fill=codes, grade=device_grade(v9, gpu, d, fmt))
    want = np.full(total + 32, 0xA5, np.uint8)
    for i, b in enumerate(order):
        ref = graded_reference(v9, pre_planes(frames[b], ow, oh, filt, d, 1, 1, dst=rects[i], fill=codes), fmt, d, 5, 0,
                               clips=i != 2)              # frame 2 is two pixels of picture in one triple of fill
        _same(res[i], ref, "%s %s frame %d" % (fmt, filt, i))
        want[i * stride: i * stride + nbytes] = frame_bytes(ref, fmt, pit, offs, nbytes)
    border = graded_reference(v9, [np.full((1, 1), c, np.int64) for c in codes], fmt, d, 5, 0, clips=False)
    px = res[0][0, 0] if fmt == "rgb24" else res[0][:, 0, 0]
    _same(px, border.reshape(3), "the border is the graded fill triple")
    got = out.cpu().numpy()
    bad = got != want
    assert not bad.any(), "%d bytes differ, first at %d" % (int(bad.sum()), int(np.argmax(bad)))


# ------------------------------------------------------------------ 4. tile edges, 5. the launch split
@pytest.mark.parametrize("filt", FILTERS)
def test_tile_edges(v9, gpu, filt):
    """129 x 5 crosses the 128 x 4 tile in both axes."""
    w, h, d, ow, oh = 200, 38, 10, 129, 5
    rng = np.random.default_rng(44)
    gpu.configure(w, h, d, nbufs=1)
    planes = _random_planes(rng, w, h, d, 1, 1)
    gpu.upload(0, planes)
    for fmt in RGB_FORMATS:
        got = gpu.convert([0], fmt, colorspace=5, resize=(ow, oh), filter=filt, grade=device_grade(v9, gpu, d, fmt))
        _same(got[0], graded_reference(v9, pre_planes(planes, ow, oh, filt, d, 1, 1), fmt, d, 5, 0), "%s %s" % (fmt, filt))


@pytest.mark.parametrize("filt", ("box", "bicubic"))
def test_33_frames_cross_the_launch_split(v9, gpu, filt):
    w, h, d = 16, 16, 8
    rng = np.random.default_rng(55)
    gpu.configure(w, h, d, nbufs=2)
    frames = [_random_planes(rng, w, h, d, 1, 1) for _ in range(2)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [(i * 7 + i // 3) % 2 for i in range(33)]
    got = gpu.convert(order, "rgb24", resize=(12, 10), filter=filt, grade=device_grade(v9, gpu, d, "rgb24"))
    refs = [graded_reference(v9, pre_planes(p, 12, 10, filt, d, 1, 1), "rgb24", d, 2, 0) for p in frames]
    _same(got, np.stack([refs[b] for b in order]), "33 frames")


# ------------------------------------------------------------------ 6. the table-free identity
def test_table_free_identity(v9, gpu):
    """in_lut[c] = c << 6, m = 16384 I, out_lut[i] = min(16 i, 65535), rgbp_f16: v = c << 6."""
    w, h, d = 70, 38, 10
    rng = np.random.default_rng(66)
    gpu.configure(w, h, d, nbufs=1, ss_h=0, ss_v=0)
    planes = _random_planes(rng, w, h, d, 0, 0)
    planes[0][0, :64] = np.arange(960, 1024)                # the top codes among them
    gpu.upload(0, planes)
    g = gpu.grade("rgbp_f16", np.arange(1024) << 6, 16384 * np.eye(3, dtype=np.int64), np.minimum(16 * np.arange(4097), 65535))
    got = gpu.convert([0], "rgbp_f16", colorspace=7, full_range=True, grade=g)
    v = np.stack([planes[2], planes[0], planes[1]]).astype(np.int64) << 6      # planes are G, B, R
    _same(got[0], (v.astype(np.float32) * np.float32(1.0 / 65535)).astype(np.float16), "identity")


# ------------------------------------------------------------------ 7. errors: refused before anything is written
def test_errors_write_nothing(v9, gpu):
    w, h, d = 70, 38, 10
    L = v9.lib()
    gpu.configure(w, h, d, nbufs=1)
    out = torch.full((8 * w * h,), 0xA5, dtype=torch.uint8, device="cuda")
    g16, g8 = device_grade(v9, gpu, d, "rgbp_f16"), device_grade(v9, gpu, d, "rgb24")
    other = device_grade(v9, gpu, 8, "rgb24")
    torch.cuda.synchronize()                        # the direct calls below run on the context's own stream
    one = (ctypes.c_int * 1)(0)

    def call(fmt, grade, filt=0, size=(w, h)):
        desc = v9.OutDesc(v9.OUT_FORMATS[fmt], 2, 0, w, h, 0, 0)
        rs = v9.Resample(filt, *size)
        return L.vp9hip_convert_frames_graded(gpu._c, one, 1, ctypes.byref(desc), ctypes.byref(rs), grade, out.data_ptr(), None)

    assert call("semiplanar", g8._g) == v9.EINVAL
    assert call("rgb24", other._g) == v9.EINVAL             # a grade of another depth
    assert call("rgb24", g16._g) == v9.EINVAL               # out_max is not the format's
    assert call("rgbp_u8", g16._g) == v9.EINVAL
    assert call("rgbp_f16", g8._g) == v9.EINVAL
    assert call("rgb24", None) == v9.EINVAL                 # a NULL grade
    assert call("rgb24", g8._g, filt=3) == v9.EINVAL and call("rgb24", g8._g, size=(0, h)) == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    # the Python layer
    with pytest.raises(ValueError):
        gpu.convert([0], "semiplanar", out=out, grade=g8)
    with pytest.raises(ValueError):
        gpu.convert([0], "rgb24", out=out, grade=v9.Grade(d, "rgb24", *tables(d, "rgb24")))     # host data only
    for bad in (other, g16):
        with pytest.raises(v9.Vp9HipError) as e:
            gpu.convert([0], "rgb24", out=out, grade=bad)
        assert e.value.code == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())
    assert call("rgb24", g8._g) == 0                        # the control: the same call with its own grade
    torch.cuda.synchronize()
    assert not bool((out[:3 * w * h] == 0xA5).all())


# ------------------------------------------------------------------ 8. the decoder's frames
def test_decoder_convert_graded(v9, gpu):
    w, h, d = 176, 144, 10
    frames = _frames(v9, w, h, 3, bpp=d)
    enc = v9.Stream()
    enc.set_color(5, 0)
    datas = [enc.encode(frames[0])[0]]
    for i in range(1, 3):
        datas.append(enc.encode(frames[i], ref_slot=(i - 1, 0, i - 1), refresh_mask=1 << i)[0])
    packets = [(data, pts) for pts, data in v9.ivf_read(v9.ivf_write(datas, w, h))[1]]
    dec = v9.Decoder(0, max_batch=4)
    try:
        infos = [info for _, info in dec.decode(packets, download=False)]
        assert len(infos) == 3 and all((i.bpp, i.colorspace, i.full_range) == (d, 5, 0) for i in infos)
        planes = []
        for i in infos:
            pl = v9.alloc_planes(w, h, d)
            ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pl])
            ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in pl])
            assert v9.lib().vp9hip_download_frame(dec.context(), i.buf, ptrs, ls) == 0
            planes.append(v9.visible(pl, w, h))
        g = dec.grade(v9.Grade(d, "rgbp_f16", *tables(d, "rgbp_f16")))
        with pytest.raises(ValueError):
            dec.convert(infos, "semiplanar", grade=g)
        got = dec.convert(infos, "rgbp_f16", resize=(44, 36), filter="triangle", grade=g)
        assert tuple(got.shape) == (3, 3, 36, 44) and got.dtype == torch.float16
        gpu.configure(w, h, d, nbufs=3)
        for b, p in enumerate(planes):
            gpu.upload(b, p)
        same = gpu.convert([0, 1, 2], "rgbp_f16", colorspace=5, full_range=False, resize=(44, 36), filter="triangle",
                           grade=device_grade(v9, gpu, d, "rgbp_f16"))
        assert torch.equal(got.view(torch.int16), same.view(torch.int16))
        for k in range(3):
            ref = graded_reference(v9, pre_planes(planes[k], 44, 36, "triangle", d, 1, 1), "rgbp_f16", d, 5, 0, clips=False)
            _same(got[k], ref, "frame %d" % k)
        with pytest.raises(v9.Vp9HipError):        # convert released the buffers
            dec.release(infos[0].buf)
    finally:
        dec.close()


# ------------------------------------------------------------------ 9. ordered like torch's current stream
def test_ordered_on_a_side_stream(v9, gpu):
    """The shape of test_gpu_convert's where="side" case: the stream is kept busy before `out` is
    filled on it; a graded conversion that ran ahead of that fill would be overwritten by it."""
    w, h, d = 352, 288, 10
    rng = np.random.default_rng(99)
    gpu.configure(w, h, d, nbufs=1)
    planes = _random_planes(rng, w, h, d, 1, 1)
    gpu.upload(0, planes)
    g = device_grade(v9, gpu, d, "rgb24")
    busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    out = torch.empty(3 * w * h, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for _ in range(40):
            busy.add_(1.0)
        out.fill_(0xA5)
        got = gpu.convert([0], "rgb24", colorspace=5, out=out, grade=g)
        host = got.cpu()
    up = [planes[0]] + [np.repeat(np.repeat(p, 2, axis=0), 2, axis=1) for p in planes[1:]]
    _same(host[0], graded_reference(v9, up, "rgb24", d, 5, 0), "side")
