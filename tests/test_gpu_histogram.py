"""Device frame histograms (vp9hip_frame_histograms / vp9hip_decoder_histograms, k_hist of
csrc/vp9hip_hist.hip) against the numpy statement of the definition in
tests/test_histogram_definition.py. Every comparison is exact (int32).

Frames are written with Device.upload, which fills the visible samples of a buffer; the
rectangle tests count less than that, over noise, so a sample counted from outside shows.
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the histograms are torch tensors and share their HIP runtime (see _torch_first)
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_histogram_definition import check_sums, ref_hist
from test_metrics_definition import SUBSAMPLINGS, plane_sizes, random_planes
from test_stream import _frames

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (65, 33), (70, 38), (352, 288)]
COLOURS = [(1, False), (2, True), (5, False), (7, True), (2, False), (5, True), (1, True), (7, False)]


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])


def _both(v9, gpu, planes, bpp, ss_h, ss_v, bins_list, rect=None, size=None, cs=2, fr=False, buf=0):
    """Both modes of buffer `buf` (which holds planes) against the reference, for every bins."""
    w, h = size or (planes[0].shape[1], planes[0].shape[0])
    r = rect or (0, 0, w, h)
    for bins in bins_list:
        for what in ("planes", "rgbm"):
            got = gpu.histograms([buf], what=what, bins=bins, colorspace=cs, full_range=fr, size=size,
                                 rects=rect)
            assert got.dtype == torch.int32 and tuple(got.shape) == (1, 3 if what == "planes" else 4, bins)
            want = ref_hist(v9, planes, bpp, ss_h, ss_v, what, bins, r, cs, fr)
            _same(got[0], want, "%s %d bins, rect %r, %d bits ss %d%d cs %d/%d" % (what, bins, r, bpp, ss_h, ss_v, cs, fr))
            check_sums(want, what, r, ss_h, ss_v)


# ------------------------------------------------------------------ every depth, subsampling, size, mode
@pytest.mark.parametrize("ss", SUBSAMPLINGS)
@pytest.mark.parametrize("bpp", [8, 10, 12])
def test_formats_match_the_reference(v9, gpu, bpp, ss):
    ss_h, ss_v = ss
    rng = np.random.default_rng(210 * bpp + 10 * ss_h + ss_v)
    for i, (w, h) in enumerate(SIZES):
        gpu.configure(w, h, bpp, nbufs=1, ss_h=ss_h, ss_v=ss_v)
        planes = random_planes(rng, w, h, bpp, ss_h, ss_v)
        gpu.upload(0, planes)
        cs, fr = COLOURS[(i + bpp + 2 * ss_h + ss_v) % len(COLOURS)]
        _both(v9, gpu, planes, bpp, ss_h, ss_v, sorted({256, 1 << bpp}), cs=cs, fr=fr)
    _both(v9, gpu, planes, bpp, ss_h, ss_v, [16])              # the fewest bins, on the last size


# ------------------------------------------------------------------ rectangles and crops
RECTS = [(0, 0, 65, 33), (198, 128, 2, 2), (64, 32, 17, 15), (2, 0, 1, 130), (0, 0, 200, 130)]


@pytest.mark.parametrize("bpp", [8, 10])
def test_rectangles_of_a_larger_buffer(v9, gpu, bpp):
    rng = np.random.default_rng(21 + bpp)
    w, h = 200, 130
    gpu.configure(w, h, bpp, nbufs=2)
    planes = [random_planes(rng, w, h, bpp, 1, 1) for _ in range(2)]
    for i, p in enumerate(planes):
        gpu.upload(i, p)
    for rect in RECTS:
        _both(v9, gpu, planes[0], bpp, 1, 1, [256], rect=rect, cs=5)
    for size in ((65, 33), (1, 1), (17, 15)):                   # the top-left crop, without rectangles
        _both(v9, gpu, planes[1], bpp, 1, 1, [1 << bpp], size=size, buf=1)
    _both(v9, gpu, planes[0], bpp, 1, 1, [256], rect=(2, 2, 15, 13), size=(17, 15))    # a rectangle inside a crop
    # per-frame rectangles that differ within one call
    bufs, rects = [0, 0, 1], [RECTS[2], RECTS[1], RECTS[3]]
    for what in ("planes", "rgbm"):
        got = gpu.histograms(bufs, what=what, bins=256, rects=rects)
        want = np.stack([ref_hist(v9, planes[b], bpp, 1, 1, what, 256, r) for b, r in zip(bufs, rects)])
        _same(got, want, "three rectangles, " + what)


@pytest.mark.parametrize("ss", [(0, 0), (1, 0), (0, 1)])
def test_rectangles_at_other_subsamplings(v9, gpu, ss):
    ss_h, ss_v = ss
    rng = np.random.default_rng(40 + 2 * ss_h + ss_v)
    w, h, bpp = 200, 130, 10
    gpu.configure(w, h, bpp, nbufs=1, ss_h=ss_h, ss_v=ss_v)
    planes = random_planes(rng, w, h, bpp, ss_h, ss_v)
    gpu.upload(0, planes)
    for rect in ((199 & ~ss_h, 129 & ~ss_v, 1, 1), (66 | (1 - ss_h), 32 | (1 - ss_v), 17, 15), (16, 0, 48, 130), (0, 0, 200, 130)):
        _both(v9, gpu, planes, bpp, ss_h, ss_v, [1024], rect=rect)


# ------------------------------------------------------------------ concentration: where run combining goes wrong
def _constant(w, h, bpp, code):
    dt = np.uint8 if bpp == 8 else np.uint16
    return [np.full((ph, pw), code, dt) for pw, ph in plane_sizes(w, h, 1, 1)]


@pytest.mark.parametrize("case", [(1920, 1080, 8), (352, 288, 12)])
def test_constant_frames(v9, gpu, case):
    w, h, bpp = case
    gpu.configure(w, h, bpp, nbufs=1)
    for code in (0, (1 << bpp) - 1, 16 << (bpp - 8)):
        planes = _constant(w, h, bpp, code)
        planes[1][:] = planes[2][:] = 1 << (bpp - 1)
        gpu.upload(0, planes)
        # the reference of one grey pixel, times w h: every pixel is the same
        one = ref_hist(v9, [p[:1, :1] for p in planes], bpp, 0, 0, "rgbm", 1 << bpp, (0, 0, 1, 1)).astype(np.int64) * (w * h)
        for bins in (256, 1 << bpp):
            got = gpu.histograms([0], bins=bins).cpu().numpy()[0]
            assert got[0, code >> (bpp - bins.bit_length() + 1)] == w * h and got[1, bins // 2] == (w // 2) * (h // 2)
            assert got[2, bins // 2] == (w // 2) * (h // 2) and np.count_nonzero(got) == 3
            rgbm = gpu.histograms([0], what="rgbm", bins=bins)
            _same(rgbm[0], one.reshape(4, bins, -1).sum(-1).astype(np.int32), "constant %d, %d bins" % (code, bins))
            assert np.count_nonzero(one) == 4                            # grey: one bin a channel


@pytest.mark.parametrize("bpp", [8, 10])
def test_concentrated_pictures(v9, gpu, bpp):
    w, h = 352, 288
    dt = np.uint8 if bpp == 8 else np.uint16
    rng = np.random.default_rng(88 + bpp)
    gpu.configure(w, h, bpp, nbufs=1)
    top = (1 << bpp) - 1
    pictures = {}
    # a two-valued checkerboard, in every plane
    pictures["checkerboard"] = [np.where((np.mgrid[:ph, :pw].sum(0)) & 1, top - 3, 7).astype(dt) for pw, ph in plane_sizes(w, h, 1, 1)]
    # left half constant, right half noise
    half = random_planes(rng, w, h, bpp, 1, 1)
    for p in half:
        p[:, :p.shape[1] // 2] = 100
    pictures["half constant"] = half
    # a horizontal ramp with runs of 1, 2, ... 17 equal codes: runs cross the lanes' 16-sample segments
    lengths = np.tile(np.arange(1, 18), 8)
    row = np.repeat(np.arange(lengths.size) * 3 % (top + 1), lengths)[:w]
    assert row.size == w
    ramp = [np.broadcast_to(row[:pw], (ph, pw)).astype(dt) for pw, ph in plane_sizes(w, h, 1, 1)]
    ramp[0] = np.ascontiguousarray(ramp[0])
    ramp[0][1::2] = ramp[0][1::2, ::-1]                          # and the odd rows run the other way
    pictures["ramp"] = ramp
    # the same code in long vertical stripes: a lane meets its run again in the next block
    pictures["stripes"] = [((np.mgrid[:ph, :pw][1] // 16) * 5 % (top + 1)).astype(dt) for pw, ph in plane_sizes(w, h, 1, 1)]
    for name, planes in pictures.items():
        planes = [np.ascontiguousarray(p) for p in planes]
        gpu.upload(0, planes)
        for what, bins in (("planes", 256), ("planes", 1 << bpp), ("rgbm", 1 << bpp), ("rgbm", 16)):
            got = gpu.histograms([0], what=what, bins=bins)
            _same(got[0], ref_hist(v9, planes, bpp, 1, 1, what, bins, (0, 0, w, h)), "%s %s %d" % (name, what, bins))


def test_codes_above_the_depth(v9, gpu):
    w, h, bpp = 70, 38, 10
    gpu.configure(w, h, bpp, nbufs=1)
    rng = np.random.default_rng(10)
    planes = [rng.choice(np.array([1023, 1024, 65535, 5, 512], np.uint16), (ph, pw)) for pw, ph in plane_sizes(w, h, 1, 1)]
    planes[0][3, :40] = 65535                                    # whole segments above the depth
    planes[0][4, :40] = 1024
    gpu.upload(0, planes)
    for bins in (16, 256, 1024):
        got = gpu.histograms([0], bins=bins)
        want = ref_hist(v9, planes, bpp, 1, 1, "planes", bins, (0, 0, w, h))
        _same(got[0], want, "codes above the depth, %d bins" % bins)
        assert want[0, -1] == np.count_nonzero(planes[0] >= 1023)


# ------------------------------------------------------------------ batches: the split at 32 frames
def test_batches(v9, gpu):
    w, h = 16, 16
    rng = np.random.default_rng(34)
    gpu.configure(w, h, 8, nbufs=3)
    planes = [random_planes(rng, w, h, 8, 1, 1) for _ in range(3)]
    for i, p in enumerate(planes):
        gpu.upload(i, p)
    n = 33
    bufs = [int(x) for x in rng.integers(0, 3, n)]
    bufs[:3] = [0, 1, 1]
    bufs[31], bufs[32] = 0, 2                                    # the frame past the split differs from the one before
    for what, C in (("planes", 3), ("rgbm", 4)):
        ref = [ref_hist(v9, p, 8, 1, 1, what, 256, (0, 0, w, h)) for p in planes]
        want = np.stack([ref[b] for b in bufs])
        out = torch.full((n * C * 256 + 8,), -1, dtype=torch.int32, device="cuda")
        got = gpu.histograms(bufs, what=what, out=out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (n, C, 256)
        _same(got, want, "33 frames, " + what)
        assert bool((out[n * C * 256:] == -1).all())
        _same(gpu.histograms(bufs, what=what, out=out), want, "second call into the same out")
        assert bool((out[n * C * 256:] == -1).all())
    with pytest.raises(ValueError):
        gpu.histograms(bufs, out=out[:100])
    with pytest.raises(ValueError):
        gpu.histograms(bufs, out=out.to(torch.int64))


@pytest.mark.parametrize("case", [(2040, 2047, 8), (2040, 300, 10)])
def test_large_batches(v9, gpu, case):
    """32 frames: every frame gets its share of HIST_FILL = 1024 workgroups, 32 each, so a wave
    walks many blocks (csrc/vp9hip_hist.h); a single frame of the same size gets a workgroup for
    every 32 blocks."""
    w, h, bpp = case
    rng = np.random.default_rng(w + h)
    gpu.configure(w, h, bpp, nbufs=2)
    planes = [random_planes(rng, w, h, bpp, 1, 1) for _ in range(2)]
    for p in planes:
        p[0][h // 3:h // 2] = 77                                 # flat bands in the noise
    for i, p in enumerate(planes):
        gpu.upload(i, p)
    bufs = [int(x) for x in rng.integers(0, 2, 32)]
    bufs[:2] = [0, 1]
    for what, bins in (("planes", 1 << bpp), ("rgbm", 256)):
        ref = [ref_hist(v9, p, bpp, 1, 1, what, bins, (0, 0, w, h)) for p in planes]
        _same(gpu.histograms(bufs, what=what, bins=bins), np.stack([ref[b] for b in bufs]), "32 frames of %dx%d" % (w, h))
        _same(gpu.histograms([1], what=what, bins=bins)[0], ref[1], "one frame of %dx%d" % (w, h))
    same = gpu.histograms([1] * 32).cpu().numpy()                # the same buffer 32 times: 32 identical tables
    assert (same == same[0]).all() and same[0].sum() == w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)


# ------------------------------------------------------------------ streams
@pytest.mark.parametrize("where", ["default", "side", "handle"])
def test_ordered_like_torchs_current_stream(v9, gpu, where):
    """The call takes its place in torch's current stream: the default (null) stream, which the C
    ABI cannot name, a stream of torch's own, or an explicit handle. The stream is kept busy for
    a few ms before `out` is filled on it; a histogram that ran ahead of that fill would be
    overwritten by it."""
    w, h = 352, 288
    rng = np.random.default_rng(12)
    gpu.configure(w, h, 8, nbufs=1)
    planes = random_planes(rng, w, h, 8, 1, 1)
    gpu.upload(0, planes)
    busy = torch.zeros(64 << 20, dtype=torch.float32, device="cuda")
    out = torch.empty(4 * 256, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side if where != "default" else torch.cuda.current_stream()):
        for _ in range(40):
            busy.add_(1.0)
        out.fill_(-7)
        got = gpu.histograms([0], what="rgbm", out=out, stream=side.cuda_stream if where == "handle" else None)
        host = got.cpu()
    _same(host[0], ref_hist(v9, planes, 8, 1, 1, "rgbm", 256, (0, 0, w, h)), where)


# ------------------------------------------------------------------ refusals: nothing is written
def test_refusals_write_nothing(v9, gpu):
    w, h = 66, 34
    gpu.configure(w, h, 10, nbufs=3)
    out = torch.full((4 * 4 * 1024,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    cases = [dict(bufs=[0, 3]), dict(bufs=[-1]), dict(bufs=[]), dict(bufs=[0], bins=8), dict(bufs=[0], bins=2048),
             dict(bufs=[0], what="rgbm", colorspace=0), dict(bufs=[0], what="rgbm", colorspace=6),
             dict(bufs=[0], what="rgbm", colorspace=8),
             dict(bufs=[0], size=(w + 1, h)), dict(bufs=[0], size=(w, h + 1)), dict(bufs=[0], size=(0, h)), dict(bufs=[0], size=(w, 0)),
             dict(bufs=[0], rects=(1, 0, 2, 2)), dict(bufs=[0], rects=(0, 1, 2, 2)), dict(bufs=[0], rects=(0, 0, w + 1, 1)),
             dict(bufs=[0], rects=(0, 0, 1, h + 1)), dict(bufs=[0], rects=(64, 0, 3, 1)), dict(bufs=[0], rects=(0, 32, 1, 3)),
             dict(bufs=[0], rects=(0, 0, 0, 1)), dict(bufs=[0], rects=(0, 0, 1, 0)), dict(bufs=[0], rects=(-2, 0, 4, 4)),
             dict(bufs=[0], rects=(0, -2, 4, 4)), dict(bufs=[0], rects=(0, 0, 0x7fffffff, 1)),
             dict(bufs=[0], rects=(0, 0, 18, 16), size=(17, 15)),
             dict(bufs=[0, 1, 2], rects=[(0, 0, 4, 4), (0, 0, 4, 4), (66, 0, 1, 1)])]       # the last of three
    for kw in cases:
        kw = dict(kw)
        with pytest.raises(v9.Vp9HipError) as e:
            gpu.histograms(kw.pop("bufs"), out=out, **kw)
        assert e.value.code == v9.EINVAL, kw
    L = v9.lib()
    one = (ctypes.c_int * 1)(0)
    d = v9.HistDesc(0, 8, 2, 0, w, h, None)
    fn = L.vp9hip_frame_histograms
    assert fn(gpu._c, None, 1, ctypes.byref(d), out.data_ptr(), None) == v9.EINVAL
    assert fn(gpu._c, one, 1, None, out.data_ptr(), None) == v9.EINVAL
    assert fn(gpu._c, one, 1, ctypes.byref(d), None, None) == v9.EINVAL
    assert fn(gpu._c, one, 0, ctypes.byref(d), out.data_ptr(), None) == v9.EINVAL
    assert fn(gpu._c, one, 1, ctypes.byref(d), out.data_ptr() + 2, None) == v9.EINVAL
    assert fn(None, one, 1, ctypes.byref(d), out.data_ptr(), None) == v9.EINVAL
    for what in (-1, 2):
        assert fn(gpu._c, one, 1, ctypes.byref(v9.HistDesc(what, 8, 2, 0, w, h, None)), out.data_ptr(), None) == v9.EINVAL
    fresh = v9.Device(0)                            # not configured
    try:
        with pytest.raises(v9.Vp9HipError) as e:
            fresh.histograms([0], size=(w, h), out=out)
        assert e.value.code == v9.EINVAL
    finally:
        fresh.close()
    for kw in (dict(bins=100), dict(what="yuv"), dict(rects=[(0, 0, 1, 1)] * 2)):
        with pytest.raises(ValueError):
            gpu.histograms([0], out=out, **kw)
    torch.cuda.synchronize()
    assert bool((out == -0x5A5A5A5B).all())


# ------------------------------------------------------------------ the decoder's frames
def test_decoder_histograms(v9):
    w, h = 352, 288
    enc = v9.Stream()
    fr = _frames(v9, w, h, 4)
    datas = [enc.encode(fr[0])[0]]
    for i in range(1, 4):
        datas.append(enc.encode(fr[i], ref_slot=(i - 1, 0, i - 1), refresh_mask=1 << i)[0])
    packets = [(data, pts) for pts, data in v9.ivf_read(v9.ivf_write(datas, w, h))[1]]
    dec = v9.Decoder(0, max_batch=4)
    try:
        infos = [info for _, info in dec.decode(packets, download=False)]
        assert len(infos) == 4
        planes = []
        for i in infos:
            pl = v9.alloc_planes(w, h, 8)
            ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pl])
            ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in pl])
            assert v9.lib().vp9hip_download_frame(dec.context(), i.buf, ptrs, ls) == 0
            planes.append(v9.visible(pl, w, h))
        f0 = infos[0]
        cs = 2 if f0.colorspace in (0, 6) else f0.colorspace           # the frames' own colour; unknown: BT.709
        for what in ("planes", "rgbm"):
            want = np.stack([v9.histograms_host(p, w, h, 8, what=what, colorspace=cs, full_range=bool(f0.full_range))
                             for p in planes])
            for _ in range(2):                                          # nothing was released: a second call works
                _same(dec.histograms(infos, what=what), want, "decoded frames, " + what)
        assert (want[1:] != want[:-1]).any()                            # the frames do differ
        rect = (32, 16, 99, 77)
        want = np.stack([v9.histograms_host(p, w, h, 8, bins=16, rect=rect) for p in planes])
        _same(dec.histograms(infos, bins=16, rects=rect), want, "a rectangle of decoded frames")
        for field, value in (("width", w - 16), ("height", h - 2), ("bpp", 10), ("ss_h", 0), ("ss_v", 0), ("colorspace", 5),
                             ("full_range", 1 - f0.full_range)):
            mixed = [type(i).from_buffer_copy(i) for i in infos]
            setattr(mixed[2], field, value)
            with pytest.raises(v9.Vp9HipError) as e:
                dec.histograms(mixed, what="rgbm")
            assert e.value.code == v9.EINVAL, field
        for i in infos:
            dec.release(i.buf)
        with pytest.raises(v9.Vp9HipError) as e:                        # released frames are not the caller's
            dec.histograms(infos)
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()


# ------------------------------------------------------------------ the decode does not notice
def test_decode_unchanged(v9, gpu):
    w, h = 352, 288
    key = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x21000))
    inter = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x21001, inter=1))

    def decode(between=None):
        gpu.submit(key, 0)
        if between:
            between()
        gpu.submit(inter, 1, (0, 0, 0))
        gpu.sync()
        return [gpu.download(0), gpu.download(1)]
    gpu.configure(w, h, 8, nbufs=2)
    before = decode()
    got = gpu.histograms([1, 0], what="rgbm")
    torch.cuda.synchronize()
    vis = [v9.visible(f, w, h) for f in before]
    _same(got, np.stack([ref_hist(v9, vis[1], 8, 1, 1, "rgbm", 256, (0, 0, w, h)),
                         ref_hist(v9, vis[0], 8, 1, 1, "rgbm", 256, (0, 0, w, h))]), "decoded frames")
    after = [gpu.download(0), gpu.download(1)]
    again = decode(lambda: gpu.histograms([1], bins=16))                # a call in the decode's midst
    torch.cuda.synchronize()
    for x, y, z in zip(before, after, again):
        for p in range(3):
            assert np.array_equal(x[p], y[p]) and np.array_equal(x[p], z[p])
