"""Device frame metrics (vp9hip_frame_metrics / vp9hip_decoder_metrics, k_metrics of
csrc/vp9hip_metrics.hip) against the numpy statement of the definition in
tests/test_metrics_definition.py. Every comparison is exact (int64 / int32).

Frames are written with Device.upload, which fills the visible samples of a buffer; the crop
tests compare less than that, so what lies beyond the compared size differs between a and b.
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the metrics are torch tensors and share their HIP runtime (see _torch_first)
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_metrics_definition import FIELDS, SUBSAMPLINGS, plane_sizes, random_planes, ref_metrics
from test_stream import _frames

pytestmark = pytest.mark.gpu

SIZES = [(16, 16), (65, 33), (70, 38), (352, 288)]
F = {n: i for i, n in enumerate(FIELDS)}


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, got, want)


def _pair(gpu, a, b, w, h, ss_h=1, ss_v=1, size=None):
    """Upload a, b into buffers 0, 1 and compare metrics + map of (0, 1) over `size` with the reference."""
    gpu.upload(0, a)
    gpu.upload(1, b)
    cw, ch = size or (w, h)
    m, cells = gpu.metrics([0], [1], size=size, cells=True)
    assert m.dtype == torch.int64 and tuple(m.shape) == (1, 3, 8)
    assert cells.dtype == torch.int32 and tuple(cells.shape) == (1, (ch + 15) >> 4, (cw + 15) >> 4)
    want, wcells = ref_metrics(a, b, cw, ch, ss_h, ss_v)
    what = "%dx%d of %dx%d ss %d%d" % (cw, ch, w, h, ss_h, ss_v)
    _same(m[0], want, what)
    _same(cells[0], wcells, what + " cells")
    _same(gpu.metrics([0], [1], size=size)[0], want, what + " without the map")
    return m[0].cpu().numpy(), cells[0].cpu().numpy()


# ------------------------------------------------------------------ every depth, subsampling, size
@pytest.mark.parametrize("ss", SUBSAMPLINGS)
@pytest.mark.parametrize("bpp", [8, 10, 12])
def test_formats_match_the_reference(v9, gpu, bpp, ss):
    ss_h, ss_v = ss
    rng = np.random.default_rng(190 * bpp + 10 * ss_h + ss_v)
    for w, h in SIZES:
        gpu.configure(w, h, bpp, nbufs=2, ss_h=ss_h, ss_v=ss_v)
        a = random_planes(rng, w, h, bpp, ss_h, ss_v)
        b = random_planes(rng, w, h, bpp, ss_h, ss_v)
        _pair(gpu, a, b, w, h, ss_h, ss_v)


# ------------------------------------------------------------------ the tail masks
@pytest.mark.parametrize("bpp", [8, 10])
def test_crops_of_a_larger_buffer(v9, gpu, bpp):
    rng = np.random.default_rng(19 + bpp)
    gpu.configure(200, 130, bpp, nbufs=2)
    a = random_planes(rng, 200, 130, bpp, 1, 1)
    b = random_planes(rng, 200, 130, bpp, 1, 1)
    for size in ((65, 33), (1, 1), (17, 15), (200, 130)):
        _pair(gpu, a, b, 200, 130, size=size)


# ------------------------------------------------------------------ 32-bit accumulators overflow here
@pytest.mark.parametrize("case", [(352, 288, 12), (1920, 1080, 8)])
def test_saturation(v9, gpu, case):
    w, h, bpp = case
    dt = np.uint8 if bpp == 8 else np.uint16
    gpu.configure(w, h, bpp, nbufs=2)
    a = [np.full((ph, pw), (1 << bpp) - 1, dt) for pw, ph in plane_sizes(w, h, 1, 1)]
    b = [np.zeros_like(p) for p in a]
    m, _ = _pair(gpu, a, b, w, h)
    peak = (1 << bpp) - 1
    assert m[0, F["sse"]] == peak * peak * w * h and m[0, F["sumsq_a"]] == m[0, F["sse"]]
    assert m[0, F["sad"]] == peak * w * h and m[0, F["ndiff"]] == w * h and m[0, F["first"]] == 0


@pytest.mark.parametrize("bpp", [8, 12])
def test_single_differing_sample(v9, gpu, bpp):
    w, h = 70, 38                                   # partial cells on both edges: 5 x 3 cells
    rng = np.random.default_rng(3 + bpp)
    gpu.configure(w, h, bpp, nbufs=2)
    a = random_planes(rng, w, h, bpp, 1, 1)
    for x, y in ((0, 0), (w - 1, h - 1), (66, 3), (5, 35)):
        b = [p.copy() for p in a]
        b[0][y, x] ^= 3
        d = abs(int(a[0][y, x]) - int(b[0][y, x]))
        m, cells = _pair(gpu, a, b, w, h)
        assert tuple(m[0, 3:]) == (d, d * d, 1, d, y * w + x)
        assert not m[1:, 3:7].any() and (m[1:, 7] == -1).all()
        assert np.count_nonzero(cells) == 1 and cells[y >> 4, x >> 4] == d
    b = [p.copy() for p in a]                       # the last visible chroma sample
    b[2][-1, -1] ^= 1
    m, cells = _pair(gpu, a, b, w, h)
    assert tuple(m[2, 3:]) == (1, 1, 1, 1, 35 * 19 - 1) and not cells.any() and (m[:2, 7] == -1).all()


# ------------------------------------------------------------------ batches: the split at 32 pairs
def test_batches(v9, gpu):
    w, h = 16, 16
    rng = np.random.default_rng(33)
    gpu.configure(w, h, 8, nbufs=3)
    planes = [random_planes(rng, w, h, 8, 1, 1) for _ in range(3)]
    for i, p in enumerate(planes):
        gpu.upload(i, p)
    n = 33
    ba = [int(x) for x in rng.integers(0, 3, n)]
    bb = [int(x) for x in rng.integers(0, 3, n)]
    ba[:3], bb[:3] = [0, 1, 2], [0, 1, 1]           # a == b entries, and a repeat
    ba[32], bb[32] = 2, 0                           # the pair past the split differs
    want = np.stack([ref_metrics(planes[x], planes[y], w, h, 1, 1)[0] for x, y in zip(ba, bb)])
    wcells = np.stack([ref_metrics(planes[x], planes[y], w, h, 1, 1)[1] for x, y in zip(ba, bb)])
    out = torch.full((n * 24 + 8,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")   # bytes of 0xA5
    assert bool((out.view(torch.uint8) == 0xA5).all())
    m, cells = gpu.metrics(ba, bb, cells=True, out=out)
    assert m.data_ptr() == out.data_ptr() and tuple(m.shape) == (n, 3, 8) and tuple(cells.shape) == (n, 1, 1)
    _same(m, want, "33 pairs")
    _same(cells, wcells, "33 pairs' cells")
    assert bool((out.view(torch.uint8)[n * 192:] == 0xA5).all())
    m2 = gpu.metrics(ba, bb, out=out)               # what the records held before does not matter
    _same(m2, want, "second call into the same out")
    assert bool((out.view(torch.uint8)[n * 192:] == 0xA5).all())
    stats = gpu.metrics(ba)                         # statistics only
    wstats = np.stack([ref_metrics(planes[x], None, w, h, 1, 1)[0] for x in ba])
    _same(stats, wstats, "statistics only")
    assert not wstats[:, :, [1, 3, 4, 5, 6]].any() and (wstats[:, :, 7] == -1).all()


@pytest.mark.parametrize("case", [(2040, 2047, 8), (2040, 300, 10)])
def test_large_batches_take_tall_strips(v9, gpu, case):
    """The launcher cuts small launches into 32-row strips, one per workgroup. 32 pairs of these
    sizes take the other paths: 128-row strips, four per workgroup, and 64-row strips, two per
    workgroup (MET_FILL = 1024 workgroups a launch, csrc/vp9hip_metrics.h)."""
    w, h, bpp = case
    rng = np.random.default_rng(w + h)
    gpu.configure(w, h, bpp, nbufs=2)
    planes = [random_planes(rng, w, h, bpp, 1, 1) for _ in range(2)]
    for i, p in enumerate(planes):
        gpu.upload(i, p)
    ref = {(x, y): ref_metrics(planes[x], planes[y], w, h, 1, 1) for x in (0, 1) for y in (0, 1)}
    ba = [int(x) for x in rng.integers(0, 2, 32)]
    bb = [int(x) for x in rng.integers(0, 2, 32)]
    ba[:2], bb[:2] = [0, 1], [1, 1]
    m, cells = gpu.metrics(ba, bb, cells=True)
    _same(m, np.stack([ref[k][0] for k in zip(ba, bb)]), "32 pairs of %dx%d" % (w, h))
    _same(cells, np.stack([ref[k][1] for k in zip(ba, bb)]), "32 pairs' cells")


def test_side_stream(v9, gpu):
    w, h = 65, 33
    rng = np.random.default_rng(8)
    gpu.configure(w, h, 8, nbufs=2)
    a, b = random_planes(rng, w, h, 8, 1, 1), random_planes(rng, w, h, 8, 1, 1)
    gpu.upload(0, a)
    gpu.upload(1, b)
    want = ref_metrics(a, b, w, h, 1, 1)[0]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = gpu.metrics([0], [1]).cpu()
    _same(got[0], want, "torch side stream")
    got = gpu.metrics([0], [1], stream=side.cuda_stream)
    side.synchronize()
    _same(got[0], want, "stream handle")


# ------------------------------------------------------------------ errors: refused before anything is written
def test_errors_write_nothing(v9, gpu):
    w, h = 65, 33
    gpu.configure(w, h, 8, nbufs=3)
    out = torch.full((4 * 24,), -0x5A5A5A5A5A5A5A5B, dtype=torch.int64, device="cuda")
    cases = [dict(a=[0, 3], b=[0, 1]), dict(a=[0], b=[3]), dict(a=[-1], b=[0]), dict(a=[0], b=[-1]), dict(a=[], b=[]),
             dict(a=[0], b=[1], size=(w + 1, h)), dict(a=[0], b=[1], size=(w, h + 1)), dict(a=[0], b=[1], size=(0, h)),
             dict(a=[0], b=[1], size=(w, 0)), dict(a=[0], b=None, cells=True), dict(a=[3], b=None)]
    for kw in cases:
        kw = dict(kw)
        with pytest.raises(v9.Vp9HipError) as e:
            gpu.metrics(kw.pop("a"), kw.pop("b"), out=out, **kw)
        assert e.value.code == v9.EINVAL, kw
    L = v9.lib()
    one = (ctypes.c_int * 1)(0)
    cells = torch.full((16,), 0x25A5A5A5, dtype=torch.int32, device="cuda")
    assert L.vp9hip_frame_metrics(gpu._c, None, one, 1, w, h, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_frame_metrics(gpu._c, one, one, 1, w, h, None, None, None) == v9.EINVAL
    assert L.vp9hip_frame_metrics(gpu._c, one, one, 0, w, h, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_frame_metrics(gpu._c, one, one, 1, w, h, out.data_ptr() + 4, None, None) == v9.EINVAL
    assert L.vp9hip_frame_metrics(gpu._c, one, one, 1, w, h, out.data_ptr(), cells.data_ptr() + 2, None) == v9.EINVAL
    assert L.vp9hip_frame_metrics(gpu._c, one, None, 1, w, h, out.data_ptr(), cells.data_ptr(), None) == v9.EINVAL
    fresh = v9.Device(0)                            # not configured
    try:
        with pytest.raises(v9.Vp9HipError) as e:
            fresh.metrics([0], [0], size=(w, h), out=out)
        assert e.value.code == v9.EINVAL
    finally:
        fresh.close()
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == 0xA5).all()) and bool((cells == 0x25A5A5A5).all())


# ------------------------------------------------------------------ the decoder's frames
def test_decoder_metrics(v9):
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
        want = [ref_metrics(planes[k + 1], planes[k], w, h, 1, 1) for k in range(3)]
        assert all(m[0, F["ndiff"]] > 0 for m, _ in want)           # the frames do differ
        for _ in range(2):                                           # nothing was released: a second call works
            m, cells = dec.metrics(infos[1:], infos[:-1], cells=True)
            _same(m, np.stack([x[0] for x in want]), "consecutive frames")
            _same(cells, np.stack([x[1] for x in want]), "consecutive frames' cells")
        _same(dec.metrics(infos), np.stack([ref_metrics(p, None, w, h, 1, 1)[0] for p in planes]), "statistics")
        for field, value in (("width", w - 16), ("height", h - 2), ("bpp", 10), ("ss_h", 0), ("ss_v", 0)):
            mixed = [type(i).from_buffer_copy(i) for i in infos]
            setattr(mixed[2], field, value)
            for args in ((mixed[1:], infos[:-1]), (infos[1:], mixed[:-1]), (mixed, None)):
                with pytest.raises(v9.Vp9HipError) as e:
                    dec.metrics(*args)
                assert e.value.code == v9.EINVAL, field
        for i in infos:
            dec.release(i.buf)
        with pytest.raises(v9.Vp9HipError) as e:                    # released frames are not the caller's
            dec.metrics(infos[1:], infos[:-1])
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()


# ------------------------------------------------------------------ the decode does not notice
def test_decode_unchanged(v9, gpu):
    w, h = 352, 288
    key = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x19000))
    inter = v9.SynthFrame(v9.synth_params(w, h, 8, seed=0x19001, inter=1))

    def decode():
        gpu.submit(key, 0)
        gpu.submit(inter, 1, (0, 0, 0))
        gpu.sync()
        return [gpu.download(0), gpu.download(1)]
    gpu.configure(w, h, 8, nbufs=2)
    before = decode()
    m, cells = gpu.metrics([1, 0], [0, 0], cells=True)
    torch.cuda.synchronize()
    vis = [v9.visible(f, w, h) for f in before]
    _same(m, np.stack([ref_metrics(vis[1], vis[0], w, h, 1, 1)[0], ref_metrics(vis[0], vis[0], w, h, 1, 1)[0]]), "decoded pair")
    after = [gpu.download(0), gpu.download(1)]
    again = decode()
    for x, y, z in zip(before, after, again):
        for p in range(3):
            assert np.array_equal(x[p], y[p]) and np.array_equal(x[p], z[p])
