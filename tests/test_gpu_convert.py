"""Device output conversion (vp9hip_convert_frames / vp9hip_decoder_convert, the kernel of
csrc/vp9hip_convert.hip) against a numpy restatement of its integer definition
(include/vp9hip.h, DESIGN.md "Output conversion"). Every comparison is exact, the half
output included (its int16 bit patterns).

The reference below shares no code with the library: nearest chroma sample
U[y >> ss_v][x >> ss_h]; y' = Y - (full ? 0 : 16 << (d - 8)), cu / cv = U / V - 2^(d-1);
coefficients floor(x * 2^S + 0.5) with S = 14 + d - o; R, G, B = clip((sum + 2^(S-1)) >> S,
0, 2^o - 1); RGB streams (code 7) hold G, B, R; half = float32(x) * float32(1 / m), rounded
to nearest even.
"""
import ctypes
import math

import numpy as np
import pytest

try:     # torch first: the conversion writes torch tensors and shares their HIP runtime (see _torch_first)
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_stream import _frames

pytestmark = pytest.mark.gpu

KR_KB = {1: (.299, .114), 2: (.2126, .0722), 3: (.299, .114), 4: (.212, .087), 5: (.2627, .0593)}
SIZES = [(16, 16), (65, 33), (70, 38), (352, 288)]
FORMATS = ["semiplanar", "rgb24", "rgbp_u8", "rgbp_f16"]


# ------------------------------------------------------------------ the reference
def _coefs(cs, full, d, o):
    kr, kb = KR_KB[cs]
    s = 14 + d - o
    m = float((1 << o) - 1)
    up = float(1 << (d - 8))
    sy = m / float((1 << d) - 1) if full else m / (219. * up)
    sc = m / float((1 << d) - 1) if full else m / (224. * up)
    kg = 1. - kr - kb
    x = (sy, 2. * (1. - kr) * sc, 2. * kb * (1. - kb) / kg * sc, 2. * kr * (1. - kr) / kg * sc, 2. * (1. - kb) * sc)
    return [int(math.floor(v * float(1 << s) + .5)) for v in x], s


def _rgb(planes, d, ssh, ssv, cs, full, o):
    """(R, G, B) int64 arrays at output depth o."""
    Y = planes[0].astype(np.int64)
    h, w = Y.shape
    yi, xi = (np.arange(h) >> ssv)[:, None], (np.arange(w) >> ssh)[None, :]
    U, V = planes[1].astype(np.int64)[yi, xi], planes[2].astype(np.int64)[yi, xi]
    m = (1 << o) - 1
    if cs == 7:
        out = [V, Y, U]
        if o < d:
            out = [np.minimum((x + (1 << (d - 9))) >> (d - 8), 255) for x in out]
        return out
    (cy, crv, cgu, cgv, cbu), s = _coefs(cs, full, d, o)
    y = Y - (0 if full else 16 << (d - 8))
    cu, cv = U - (1 << (d - 1)), V - (1 << (d - 1))
    rnd = 1 << (s - 1)
    return [np.clip((cy * y + crv * cv + rnd) >> s, 0, m),
            np.clip((cy * y - cgu * cu - cgv * cv + rnd) >> s, 0, m),
            np.clip((cy * y + cbu * cu + rnd) >> s, 0, m)]


def reference(planes, fmt, d, ssh, ssv, cs, full):
    """One frame in the shape Device.convert returns it (without the batch axis)."""
    if fmt == "semiplanar":
        dt, sh = (np.uint8, 0) if d == 8 else (np.uint16, 16 - d)
        y = (planes[0].astype(np.uint32) << sh).astype(dt)
        uv = (np.stack([planes[1], planes[2]], axis=-1).astype(np.uint32) << sh).astype(dt)
        return y, uv
    if fmt == "rgbp_f16":
        m = (1 << d) - 1
        rgb = np.stack(_rgb(planes, d, ssh, ssv, cs, full, d))
        return (rgb.astype(np.float32) * np.float32(1.0 / m)).astype(np.float16)
    rgb = np.stack(_rgb(planes, d, ssh, ssv, cs, full, 8)).astype(np.uint8)
    return rgb if fmt == "rgbp_u8" else np.ascontiguousarray(rgb.transpose(1, 2, 0))


def frame_bytes(ref, fmt, pitch, offs, nbytes):
    """A converted frame as the bytes of its layout, 0xA5 wherever nothing is written."""
    buf = np.full(nbytes, 0xA5, np.uint8)

    def put(off, rows):
        rows = np.ascontiguousarray(rows)
        raw = rows.view(np.uint8).reshape(rows.shape[0], -1)
        for y in range(raw.shape[0]):
            buf[off + y * pitch: off + y * pitch + raw.shape[1]] = raw[y]
    if fmt == "semiplanar":
        put(0, ref[0])
        put(offs[1], ref[1].reshape(ref[1].shape[0], -1))
    elif fmt == "rgb24":
        put(0, ref.reshape(ref.shape[0], -1))
    else:
        for p in range(3):
            put(offs[p], ref[p])
    return buf


def _bits(a):
    """Exact comparison form: integers, or a half array's bit patterns."""
    a = np.asarray(a)
    return a.view(np.int16) if a.dtype == np.float16 else a


def _same(got, ref, what):
    got = got.cpu().numpy()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert got.dtype.itemsize == ref.dtype.itemsize, what
    g, r = _bits(got), _bits(ref)
    bad = g.view(r.dtype) != r if g.dtype != r.dtype else g != r
    assert not bad.any(), "%s: %d of %d differ" % (what, int(bad.sum()), bad.size)


def _random_planes(rng, w, h, d, ssh, ssv):
    """Samples over the whole code range (below black, above white: the clips are exercised)."""
    dt = np.uint8 if d == 8 else np.uint16
    cw, ch = (w + ssh) >> ssh, (h + ssv) >> ssv
    return [rng.integers(0, 1 << d, (h, w)).astype(dt), rng.integers(0, 1 << d, (ch, cw)).astype(dt),
            rng.integers(0, 1 << d, (ch, cw)).astype(dt)]


def _colors(d, ssh, ssv):
    c = [(1, 0), (2, 1)]
    if d == 8:
        c.append((3, 1))
    if d == 10:
        c.append((5, 0))
    if d == 12:
        c.append((4, 0))
    if not ssh and not ssv:
        c.append((7, 1))
    return c


# ------------------------------------------------------------------ every format, depth, subsampling, size
@pytest.mark.parametrize("ss", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("d", [8, 10, 12])
def test_formats_match_the_reference(v9, gpu, d, ss):
    ssh, ssv = ss
    rng = np.random.default_rng(1000 * d + 10 * ssh + ssv)
    for w, h in SIZES:
        gpu.configure(w, h, d, nbufs=1, ss_h=ssh, ss_v=ssv)
        planes = _random_planes(rng, w, h, d, ssh, ssv)
        gpu.upload(0, planes)
        cw, ch = (w + ssh) >> ssh, (h + ssv) >> ssv
        y, uv = gpu.convert([0], "semiplanar")
        assert y.dtype == (torch.uint8 if d == 8 else torch.int16) and uv.dtype == y.dtype
        assert tuple(y.shape) == (1, h, w) and tuple(uv.shape) == (1, ch, cw, 2)
        ry, ruv = reference(planes, "semiplanar", d, ssh, ssv, 2, 0)
        _same(y[0], ry, "semiplanar Y %dx%d" % (w, h))
        _same(uv[0], ruv, "semiplanar UV %dx%d" % (w, h))
        for cs, full in _colors(d, ssh, ssv):
            for fmt, shape, dt in (("rgb24", (1, h, w, 3), torch.uint8), ("rgbp_u8", (1, 3, h, w), torch.uint8),
                                   ("rgbp_f16", (1, 3, h, w), torch.float16)):
                got = gpu.convert([0], fmt, colorspace=cs, full_range=full)
                assert tuple(got.shape) == shape and got.dtype == dt
                _same(got[0], reference(planes, fmt, d, ssh, ssv, cs, full), "%s cs %d full %d %dx%d" % (fmt, cs, full, w, h))


def test_crop_of_a_larger_buffer(v9, gpu):
    """size below the configured one converts the top-left crop (odd chroma sizes)."""
    rng = np.random.default_rng(5)
    gpu.configure(200, 130, 8, nbufs=1)
    planes = _random_planes(rng, 200, 130, 8, 1, 1)
    gpu.upload(0, planes)
    crop = [planes[0][:33, :65], planes[1][:17, :33], planes[2][:17, :33]]
    for fmt in ("rgb24", "rgbp_f16"):
        got = gpu.convert([0], fmt, colorspace=1, size=(65, 33))
        _same(got[0], reference(crop, fmt, 8, 1, 1, 1, 0), fmt)
    y, uv = gpu.convert([0], "semiplanar", size=(65, 33))
    _same(y[0], crop[0], "Y")
    _same(uv[0], np.stack(crop[1:], axis=-1), "UV")


# ------------------------------------------------------------------ batches, pitches, gaps: nothing else is written
LAYOUTS = [  # fmt, depth, (ss_h, ss_v), pitch, gap after each frame
    ("rgb24", 8, (1, 1), 208, 48),
    ("rgb24", 8, (1, 1), 3 * 65, 13),          # tight: rows at every alignment, frames at odd addresses
    ("rgb24", 8, (1, 1), 3 * 65, 1),           # tight: 4-byte aligned rows among them
    ("rgbp_u8", 8, (1, 1), 80, 16),
    ("rgbp_u8", 10, (1, 0), 0, 7),             # tight pitch 65
    ("rgbp_f16", 8, (1, 1), 144, 32),
    ("rgbp_f16", 10, (0, 0), 0, 6),            # tight pitch 130: rows 2-byte aligned only
    ("semiplanar", 8, (1, 1), 80, 16),
    ("semiplanar", 8, (1, 1), 0, 3),           # tight pitch 66
    ("semiplanar", 10, (1, 1), 144, 64),
    ("semiplanar", 12, (0, 1), 0, 10),
]


@pytest.mark.parametrize("fmt,d,ss,pitch,gap", LAYOUTS)
def test_batch_layout_and_untouched_bytes(v9, gpu, fmt, d, ss, pitch, gap):
    w, h, (ssh, ssv) = 65, 33, ss
    rng = np.random.default_rng(77 + d + pitch + gap)
    gpu.configure(w, h, d, nbufs=3, ss_h=ssh, ss_v=ssv)
    frames = [_random_planes(rng, w, h, d, ssh, ssv) for _ in range(3)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [2, 0, 1]
    nbytes, pit, offs = v9.out_layout(fmt, w, h, d, ssh, ssv, pitch)
    stride = nbytes + gap
    total = 2 * stride + nbytes
    out = torch.full((total + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    cs, full = (5, 0) if d == 10 else (1, 0)
    res = gpu.convert(order, fmt, colorspace=cs, full_range=full, out=out, pitch=pitch, frame_stride=stride)
    want = np.full(total + 32, 0xA5, np.uint8)
    for i, b in enumerate(order):
        ref = reference(frames[b], fmt, d, ssh, ssv, cs, full)
        want[i * stride: i * stride + nbytes] = frame_bytes(ref, fmt, pit, offs, nbytes)
        for g, r in zip(res if fmt == "semiplanar" else (res,), ref if fmt == "semiplanar" else (ref,)):
            _same(g[i], r, "%s frame %d" % (fmt, i))
    got = out.cpu().numpy()
    bad = got != want
    assert not bad.any(), "%d bytes differ, first at %d" % (int(bad.sum()), int(np.argmax(bad)))


def test_more_frames_than_one_launch_takes(v9, gpu):
    """40 frames (repeated buffers): the launches of 32 and 8 land at their own offsets."""
    w, h = 16, 16
    rng = np.random.default_rng(9)
    gpu.configure(w, h, 8, nbufs=2)
    frames = [_random_planes(rng, w, h, 8, 1, 1) for _ in range(2)]
    for b, p in enumerate(frames):
        gpu.upload(b, p)
    order = [(i * 7 + i // 3) % 2 for i in range(40)]
    got = gpu.convert(order, "rgb24")
    refs = [reference(p, "rgb24", 8, 1, 1, 2, 0) for p in frames]
    _same(got, np.stack([refs[b] for b in order]), "40 frames")


@pytest.mark.parametrize("where", ["default", "side", "handle"])
def test_ordered_like_torchs_current_stream(v9, gpu, where):
    """The conversion takes its place in torch's current stream: the default (null) stream,
    which the C ABI cannot name, a stream of torch's own, or an explicit handle. The stream
    is kept busy for a few ms before `out` is filled on it; a conversion that ran ahead of that
    fill would be overwritten by it."""
    w, h = 352, 288
    rng = np.random.default_rng(11)
    gpu.configure(w, h, 8, nbufs=1)
    planes = _random_planes(rng, w, h, 8, 1, 1)
    gpu.upload(0, planes)
    busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    out = torch.empty(3 * w * h, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side if where != "default" else torch.cuda.current_stream()):
        for _ in range(40):
            busy.add_(1.0)
        out.fill_(0xA5)
        got = gpu.convert([0], "rgb24", out=out, stream=side.cuda_stream if where == "handle" else None)
        host = got.cpu()
    _same(host[0], reference(planes, "rgb24", 8, 1, 1, 2, 0), where)


# ------------------------------------------------------------------ errors: refused before anything is written
def test_errors_write_nothing(v9, gpu):
    w, h = 65, 33
    gpu.configure(w, h, 8, nbufs=3)
    out = torch.full((3 * 4 * 80 * 40,), 0xA5, dtype=torch.uint8, device="cuda")
    cases = [dict(bufs=[0, 3]), dict(bufs=[-1]), dict(bufs=[0], size=(w + 1, h)), dict(bufs=[0], size=(w, h + 1)),
             dict(bufs=[0], colorspace=0), dict(bufs=[0], colorspace=6), dict(bufs=[0], pitch=200),
             dict(bufs=[0, 1], frame_stride=100)]
    for kw in cases:
        kw = dict(kw)
        with pytest.raises(v9.Vp9HipError) as e:
            gpu.convert(kw.pop("bufs"), "rgb24", out=out, **kw)
        assert e.value.code == v9.EINVAL, kw
    L = v9.lib()
    d = v9.OutDesc(v9.OUT_FORMATS["rgb24"], 2, 0, w, h, 0, 0)
    one = (ctypes.c_int * 1)(0)
    assert L.vp9hip_convert_frames(gpu._c, one, 0, ctypes.byref(d), out.data_ptr(), None) == v9.EINVAL
    assert L.vp9hip_convert_frames(gpu._c, one, 1, ctypes.byref(d), None, None) == v9.EINVAL
    d16 = v9.OutDesc(v9.OUT_FORMATS["rgbp_f16"], 2, 0, w, h, 0, 0)
    assert L.vp9hip_convert_frames(gpu._c, one, 1, ctypes.byref(d16), out.data_ptr() + 1, None) == v9.EINVAL
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


# ------------------------------------------------------------------ the decoder's frames, with the stream's colour
def test_decoder_convert_uses_the_streams_color(v9):
    w, h = 352, 288
    enc = v9.Stream()
    enc.set_color(1, 1)
    fr = _frames(v9, w, h, 4)
    datas = [enc.encode(fr[0])[0]]
    for i in range(1, 4):
        datas.append(enc.encode(fr[i], ref_slot=(i - 1, 0, i - 1), refresh_mask=1 << i)[0])
    packets = [(data, pts) for pts, data in v9.ivf_read(v9.ivf_write(datas, w, h))[1]]
    dec = v9.Decoder(0, max_batch=4)
    try:
        infos = [info for _, info in dec.decode(packets, download=False)]
        assert len(infos) == 4
        assert all((i.colorspace, i.full_range, i.width, i.height) == (1, 1, w, h) for i in infos)
        planes = []
        for i in infos:
            pl = v9.alloc_planes(w, h, 8)
            ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pl])
            ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in pl])
            assert v9.lib().vp9hip_download_frame(dec.context(), i.buf, ptrs, ls) == 0
            planes.append(v9.visible(pl, w, h))
        # frames of two sizes, or of two colour descriptions, in one call: refused, nothing written
        out = torch.full((4 * 3 * w * h,), 0xA5, dtype=torch.uint8, device="cuda")
        for field, value in (("width", w - 16), ("height", h - 2), ("colorspace", 2), ("full_range", 0)):
            mixed = [type(i).from_buffer_copy(i) for i in infos]
            setattr(mixed[2], field, value)
            with pytest.raises(v9.Vp9HipError) as e:
                dec.convert(mixed, "rgb24", out=out)
            assert e.value.code == v9.EINVAL, field
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all())
        got = dec.convert(infos[:2], "rgb24")
        half = dec.convert(infos[2:], "rgbp_f16")
        for k in range(2):
            _same(got[k], reference(planes[k], "rgb24", 8, 1, 1, 1, 1), "rgb24 frame %d" % k)
            _same(half[k], reference(planes[2 + k], "rgbp_f16", 8, 1, 1, 1, 1), "half frame %d" % (2 + k))
        with pytest.raises(v9.Vp9HipError):        # convert released the buffers
            dec.release(infos[0].buf)
    finally:
        dec.close()
