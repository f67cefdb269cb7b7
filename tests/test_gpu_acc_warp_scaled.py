"""Accumulated residual at model size on the GPU: k_acc_warp_scale against the composition of the
two numpy restatements (tests/test_acc_warp_scaled_definition.py: warp_ref, then ref_tensor, the
coverage sbox of the widened mask), which share no code with the library. Exact equality, halves
by bit pattern.

Shapes are the smallest at which the kernel can still go wrong: a source wider than one
256-column chunk (528), an output wider than one 128-column tile (130, 2 w + 1), an output height
that is no multiple of the 4 waves (5, 9), odd chroma (66 -> 33), a context larger than the
visible size. The chains are those of tests/test_gpu_acc_warp.py: decoded once a shape, pixels and
fields downloaded, the 18 pairs in one call per (mode, format, size). Then the device against
k_acc_warp at 4:4:4, crafted fields through vp9hip_warp_scale_launch_dev (the hand-made cases,
every other one on oddly pitched planes, guard bytes around the destination), 33 pairs across the
launch split, the lifecycle rules, and the bitstream decoder.
"""
try:     # torch first: acc_warp_tensors returns torch tensors that share the HIP runtime (see _torch_first)
    import torch
except Exception:  # pragma: no cover
    torch = None

import ctypes

import numpy as np
import pytest

from test_acc_warp_definition import warp_ref, warp_stats
from test_acc_warp_scaled_definition import FORMATS, INTERPS, all_cases, coverage_ref, ref_scaled
from test_gpu_acc_warp import N, PAIRS, REFS, _device, _download, _gop, _pack
from test_gpu_motion_acc import stream_acc  # noqa: F401  (a fixture: the hidden-frame stream and its reference fields)
from test_residual_scaled_definition import bits, resampled

pytestmark = pytest.mark.gpu

CHAINS = {
    "8x8": dict(w=8, h=8),
    "66x66": dict(w=66, h=66),
    "200x130": dict(w=200, h=130),
    "528x72-2tiles": dict(w=528, h=72, synth=dict(log2_tile_cols=1), sizes=[None, (1, 1), (17, 9), (130, 5)]),
    "66x34-in-200x130-mv512": dict(w=66, h=34, cfg=(200, 130), synth=dict(mv_range=512)),
    "66x66-10bit": dict(w=66, h=66, bpp=10),
    "66x66-444": dict(w=66, h=66, ss=(0, 0)),
    "66x66-440": dict(w=66, h=66, ss=(0, 1)),
}


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    g, w = bits(got), bits(want)
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        raise AssertionError("%s: %d elements differ, first %s: got %s, want %s" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


class _Refs:
    """The reference of a set of pairs: warp_ref once a pair and mode, the resampled planes once
    a pair, mode and size; tensor() formats them."""

    def __init__(self, pairs, pix, accs, serials, w, h, ss_h, ss_v, bpp):
        self.geo = (w, h, ss_h, ss_v, bpp)
        self.warp = {(i, m): warp_ref(pix[a], pix[b], accs[a], serials[b], w, h, ss_h, ss_v, m, "residual")
                     for i, (a, b) in enumerate(pairs) for m in INTERPS}
        self.n, self.pre = len(pairs), {}

    def tensor(self, interp, fmt, size, cov, cs=2, full=0):
        w, h, ss_h, ss_v, bpp = self.geo
        ow, oh = size or (w, h)
        out = []
        for i in range(self.n):
            R, mask = self.warp[i, interp]
            key = (i, interp, ow, oh)
            if key not in self.pre:
                self.pre[key] = resampled(R, w, h, ss_h, ss_v, ow, oh)
            out.append(ref_scaled(R, mask, w, h, ss_h, ss_v, bpp, fmt, ow, oh, cs, full, cov, self.pre[key]))
        return np.stack(out)


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains(v9, name):
    c = CHAINS[name]
    w, h, bpp, (ss_h, ss_v) = c["w"], c["h"], c.get("bpp", 8), c.get("ss", (1, 1))
    sizes = c.get("sizes", [None, (1, 1), (17, 9), (2 * w + 1, h)])
    frames = _gop(v9, w, h, bpp, ss_h, ss_v, **c.get("synth", {}))
    dev = _device(v9, c.get("cfg", (w, h)), N, bpp, ss_h, ss_v)
    try:
        dev.stage_batch(frames, list(range(N)), REFS)
        dev.run_batch()
        dev.sync()
        pix = [v9.visible(dev.download(i), w, h, ss_h, ss_v) for i in range(N)]
        fields = [dev.download_motion_acc(i) for i in range(N)]
        accs, serials = [f[0] for f in fields], [f[1] for f in fields]
        refs = _Refs(PAIRS, pix, accs, serials, w, h, ss_h, ss_v, bpp)
        far = PAIRS.index((6, 0))
        # what the inputs exercise, from the reference alone
        if name == "200x130":
            cov = coverage_ref(refs.warp[far, "nearest"][1], w, h, 17, 9, "yuv_i16")
            part, whole = int(((cov > 0) & (cov < 256)).sum()), int((cov == 256).sum())
            print("200x130 (6, 0) at 17 x 9: coverage partial in %d outputs, 256 in %d of %d" % (part, whole, cov.size))
            assert part > 0 and whole > 0
        if name == "8x8":
            assert warp_stats(accs[6], serials[0], w, h, ss_h, ss_v)["applying"] == 0
        ba, bb = [a for a, _ in PAIRS], [b for _, b in PAIRS]
        k = 0
        for interp in INTERPS:
            for fmt in FORMATS:
                for size in sizes:
                    cov, k = bool(k & 1), k + 1
                    got = dev.acc_warp_tensors(ba, bb, fmt, resize=size, interp=interp, coverage=cov, size=(w, h))
                    torch.cuda.synchronize()
                    _same(got, refs.tensor(interp, fmt, size, cov), "%s %s %s -> %s coverage %d" % (name, interp, fmt, size, cov))
                    if name == "8x8":
                        assert not bits(got[far].cpu().numpy()).any(), "8x8 (6, 0): nothing applies"
        if (ss_h, ss_v) == (0, 0):
            # device against device: at 4:4:4 and the visible size the tensor is k_acc_warp's three planes
            for interp in INTERPS:
                t = dev.acc_warp_tensors(ba, bb, "yuv_i16", resize=None, interp=interp, size=(w, h))
                y, u, v = dev.acc_warp(ba, bb, output="residual", interp=interp, size=(w, h))
                torch.cuda.synchronize()
                for p, plane in enumerate((y, u, v)):
                    assert torch.equal(t[:, p], plane), "444 identity %s plane %d" % (interp, p)
    finally:
        dev.close()


# ------------------------------------------------------------------ crafted fields through vp9hip_warp_scale_launch_dev
def _upload_pairs(pairs, w, h, bpp, ss_h, ss_v, pad):
    """pairs of (A, B, acc, sb) of one geometry as device buffers: (keep-alive list, a, b and
    field pointers, plane offsets, pitches in bytes, field pitch in cells)."""
    bypp = 1 if bpp == 8 else 2
    cw = (w + ss_h) >> ss_h
    gw, gh = 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
    pitch = ((w + pad) * bypp, (cw + pad) * bypp)
    keep, ap, bp, cp, off = [], [], [], [], None
    for A, B, acc, sb in pairs:
        ta, off = _pack(A, pitch, bypp, 0x5a)
        tb, _ = _pack(B, pitch, bypp, 0xa5)
        cells = np.full((gh, gw + pad, 4), 0x5a5a5a5a, np.int32)
        cells[:, :gw] = np.ascontiguousarray(acc).view(np.int32).reshape(gh, gw, 4)
        tc = torch.from_numpy(cells).cuda()
        keep += [ta, tb, tc]
        ap.append(ta.data_ptr()); bp.append(tb.data_ptr()); cp.append(tc.data_ptr())
    return keep, ap, bp, cp, off, pitch, gw + pad


def _launch_dev(v9, up, serials, w, h, bpp, ss_h, ss_v, fmt, size, interp, cov, guard=64):
    """One raw launch over uploaded pairs: ((n, P, OH, OW) numpy array, True if the guard bytes
    around dst are unchanged)."""
    keep, ap, bp, cp, off, pitch, acc_pitch = up
    n, P = len(ap), 4 if cov else 3
    ow, oh = size or (w, h)
    stride, _ = v9.warpt_layout(fmt, (ow, oh), coverage=cov)
    dst = torch.full((guard + n * stride + guard,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    v9.warp_scale_launch_dev(ap, bp, cp, serials, off, pitch, acc_pitch, w, h, bpp, ss_h, ss_v, fmt, size,
                             dst.data_ptr() + guard, interp=interp, coverage=cov)
    torch.cuda.synchronize()
    d = dst.cpu().numpy()
    clean = bool((d[:guard] == 0x5a).all() and (d[guard + n * stride:] == 0x5a).all())
    body = np.ascontiguousarray(d[guard:guard + n * stride]).view(np.float16 if fmt.endswith("f16") else np.int16)
    return body.reshape(n, P, oh, ow), clean


def test_hand_made_cases_on_the_device(v9):
    """The definition test's cases, each through both modes and both sizes with the four formats
    dealt over them; every other case with planes and a field pitched 3 elements past their width
    (rows that no vector access fits) and poison there."""
    for k, (name, A, B, acc, sb, w, h, bpp, ss_h, ss_v) in enumerate(all_cases()):
        up = _upload_pairs([(A, B, acc, sb)], w, h, bpp, ss_h, ss_v, pad=3 * (k & 1))
        j = k
        for interp in INTERPS:
            R, mask = warp_ref(A, B, acc, sb, w, h, ss_h, ss_v, interp, "residual")
            for size in ((5, 3), None):
                fmt, cov, j = FORMATS[j & 3], bool((j >> 2) & 1), j + 1
                got, clean = _launch_dev(v9, up, [sb], w, h, bpp, ss_h, ss_v, fmt, size, interp, cov)
                assert clean, "%s: bytes outside the layout changed" % name
                ow, oh = size or (w, h)
                _same(got[0], ref_scaled(R, mask, w, h, ss_h, ss_v, bpp, fmt, ow, oh, coverage=cov),
                      "%s %s %s -> %s coverage %d" % (name, interp, fmt, size, cov))


def test_33_pairs_cross_the_launch_split(v9):
    rng = np.random.default_rng(33)
    w = h = 8
    pairs = []
    for i in range(33):
        A = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((8, 8), (4, 4), (4, 4))]
        B = [rng.integers(0, 256, s, dtype=np.uint8) for s in ((8, 8), (4, 4), (4, 4))]
        acc = np.zeros((2, 2), v9.ACC_CELL)
        acc["dx"], acc["dy"] = rng.integers(-80, 80, (2, 2)), rng.integers(-80, 80, (2, 2))
        acc["root"], acc["hops"] = rng.integers(100 + i, 102 + i, (2, 2)), rng.integers(0, 3, (2, 2))
        if i == 32:                                      # the pair past the split applies everywhere
            acc["root"], acc["hops"] = 100 + i, 1
        pairs.append((A, B, acc, 100 + i))
    up = _upload_pairs(pairs, w, h, 8, 1, 1, pad=0)
    for interp, fmt in (("nearest", "yuv_i16"), ("bilinear", "rgb_f16")):
        got, clean = _launch_dev(v9, up, [sb for _, _, _, sb in pairs], w, h, 8, 1, 1, fmt, (3, 3), interp, True)
        assert clean
        covered = 0
        for i, (A, B, acc, sb) in enumerate(pairs):
            R, mask = warp_ref(A, B, acc, sb, w, h, 1, 1, interp, "residual")
            _same(got[i], ref_scaled(R, mask, w, h, 1, 1, 8, fmt, 3, 3, coverage=True), "pair %d %s %s" % (i, interp, fmt))
            covered += int(mask.sum())
        assert 4 < covered < 33 * 4
        assert float(got[32, 3].astype(np.float32).min()) == (256.0 if fmt == "yuv_i16" else 1.0)


def test_launch_dev_refuses_bad_arguments(v9):
    L = v9.lib()
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    one = (ctypes.c_void_p * 1)(t.data_ptr())
    ser = (ctypes.c_uint32 * 1)(1)
    off, pitch = (ctypes.c_int64 * 3)(0, 64, 80), (ctypes.c_int32 * 2)(8, 4)

    def call(a=one, b=one, acc=one, s=ser, n=1, off=off, pitch=pitch, ap=2, w=8, h=8, bpp=8, sh=1, sv=1, mode=0, fmt=2, cs=2,
             planes=4, ow=3, oh=3, p=0, fs=0, desc=True, dst=t.data_ptr() + 1024):
        d = v9.WarptDesc(fmt, cs, 0, mode, planes, w, h, ow, oh, p, fs)
        return L.vp9hip_warp_scale_launch_dev(a, b, acc, s, n, ctypes.byref(off) if off else None,
                                              ctypes.byref(pitch) if pitch else None, ap, bpp, sh, sv,
                                              ctypes.byref(d) if desc else None, dst, None)
    bad = [dict(a=None), dict(b=None), dict(acc=None), dict(s=None), dict(n=0), dict(off=None), dict(pitch=None), dict(ap=1),
           dict(w=0), dict(h=16385), dict(bpp=9), dict(sh=2), dict(sv=-1), dict(mode=2), dict(mode=-1), dict(dst=None),
           dict(dst=t.data_ptr() + 1025), dict(pitch=(ctypes.c_int32 * 2)(7, 4)), dict(pitch=(ctypes.c_int32 * 2)(8, 3)),
           dict(acc=(ctypes.c_void_p * 1)(t.data_ptr() + 8)), dict(a=(ctypes.c_void_p * 1)(None)),
           dict(bpp=10, pitch=(ctypes.c_int32 * 2)(17, 8)), dict(fmt=4), dict(fmt=-1), dict(cs=0), dict(cs=6), dict(cs=8),
           dict(planes=2), dict(planes=5), dict(ow=0), dict(oh=16385), dict(p=4), dict(p=24), dict(fs=70), dict(fs=73),
           dict(desc=False)]
    for kw in bad:
        assert call(**kw) == v9.EINVAL, kw
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ------------------------------------------------------------------ lifecycle
W, H = 200, 130


@pytest.fixture
def chain3(v9):
    """Key + 2 inter at 200x130 in buffers 0..2 of a 5-buffer context."""
    frames = _gop(v9, W, H, seed=7600, n=3)
    dev = _device(v9, (W, H), 5)
    dev.stage_batch(frames, [0, 1, 2], REFS[:3])
    dev.run_batch()
    dev.sync()
    yield dev, frames
    dev.close()


def test_errors_write_nothing(v9, chain3):
    dev, frames = chain3
    out = torch.full((2 * 4 * 9 * 17 + 16,), 0x5a5a, dtype=torch.int16, device="cuda")
    half = out.view(torch.float16)
    base = dict(fmt="rgb_i16", resize=(17, 9), coverage=True, out=out)
    cases = [(dict(bufs=[1, 5], root_bufs=[0, 0]), v9.EINVAL), (dict(bufs=[1], root_bufs=[-1]), v9.EINVAL),
             (dict(bufs=[-1], root_bufs=[0]), v9.EINVAL), (dict(bufs=[1], root_bufs=[5]), v9.EINVAL),
             (dict(bufs=[], root_bufs=[]), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], size=(W + 1, H)), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], size=(W, H + 1)), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], size=(0, H)), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], size=(W, 0)), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], size=(W - 8, H)), v9.EINVAL),      # another grid than the field's
             (dict(bufs=[1], root_bufs=[0], size=(W, H - 10)), v9.EINVAL),
             (dict(bufs=[1, 3], root_bufs=[0, 0]), v9.EAGAIN),                  # never written: no field
             (dict(bufs=[1, 1], root_bufs=[0, 4]), v9.EAGAIN),
             (dict(bufs=[1], root_bufs=[0], fmt="rgb_u8"), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], interp="cubic"), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], colorspace=0), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], colorspace=6), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], resize=(0, 9)), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], resize=(17, 16385)), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], pitch=24), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], pitch=40), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], frame_stride=4 * 34 * 9 - 2), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], frame_stride=4 * 34 * 9 + 1), v9.EINVAL)]
    for kw, code in cases:
        with pytest.raises(v9.Vp9HipError) as e:
            dev.acc_warp_tensors(**dict(base, **kw))
        assert e.value.code == code, kw
    with pytest.raises(v9.Vp9HipError) as e:
        dev.acc_warp_tensors([1], [0], "rgb_f16", resize=(17, 9), out=half, pitch=24)
    assert e.value.code == v9.EINVAL
    L = v9.lib()
    one, zero = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0)

    def raw(c=dev._c, a=one, b=zero, n=1, dst=out.data_ptr(), desc=True, **kw):
        f = dict(dict(format=2, colorspace=2, full_range=0, mode=0, planes=4, width=W, height=H, out_width=17, out_height=9,
                      pitch=0, frame_stride=0), **kw)
        d = v9.WarptDesc(*[f[k] for k, _ in v9.WarptDesc._fields_])
        return L.vp9hip_acc_warp_scaled(c, a, b, n, ctypes.byref(d) if desc else None, dst, None)
    for kw in (dict(a=None), dict(b=None), dict(dst=None), dict(c=None), dict(n=-1), dict(desc=False), dict(mode=2), dict(mode=-1),
               dict(format=4), dict(format=-1), dict(planes=2), dict(planes=5), dict(dst=out.data_ptr() + 1), dict(pitch=8),
               dict(colorspace=8)):
        assert raw(**kw) == v9.EINVAL, kw
    dev.upload(4, v9.alloc_planes(W, H, 8))              # an uploaded b holds pixels and no field
    with pytest.raises(v9.Vp9HipError) as e:
        dev.acc_warp_tensors([1], [4], **{k: v for k, v in base.items()})
    assert e.value.code == v9.EAGAIN
    for other in (_device(v9, (W, H), 2, acc=False), v9.Device(0)):   # motion export alone; not configured
        try:
            if other.w:
                other.stage_batch(frames[:2], [0, 1], REFS[:2])
                other.run_batch()
                other.sync()
            with pytest.raises(v9.Vp9HipError) as e:
                other.acc_warp_tensors([1], [0], size=(W, H), **base)
            assert e.value.code == v9.EINVAL
        finally:
            other.close()
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a).all())
    assert raw() == 0                                    # and the same arguments without a fault are served
    torch.cuda.synchronize()
    assert bool((out[:4 * 9 * 17] != 0x5a5a).any()) and bool((out[4 * 9 * 17:] == 0x5a5a).all())


def test_views_out_stream_and_an_overwritten_root(v9, chain3):
    dev, frames = chain3
    pix = [v9.visible(dev.download(i), W, H) for i in range(3)]
    fields = [dev.download_motion_acc(i) for i in range(3)]
    accs, serials = [f[0] for f in fields], [f[1] for f in fields]
    pairs = [(1, 0), (2, 0), (2, 1), (2, 2)]
    ba, bb = [a for a, _ in pairs], [b for _, b in pairs]
    refs = _Refs(pairs, pix, accs, serials, W, H, 1, 1, 8)
    # the result: dtype by the format, (N, P, OH, OW), tight
    t = dev.acc_warp_tensors(ba, bb, "rgb_f16", resize=(17, 9), coverage=True)
    torch.cuda.synchronize()
    assert t.dtype == torch.float16 and tuple(t.shape) == (4, 4, 9, 17) and t.stride() == (4 * 9 * 17, 9 * 17, 17, 1)
    _same(t, refs.tensor("nearest", "rgb_f16", (17, 9), True), "views")
    t = dev.acc_warp_tensors(ba, bb, "yuv_i16", interp="bilinear")
    torch.cuda.synchronize()
    assert t.dtype == torch.int16 and tuple(t.shape) == (4, 3, H, W) and t.is_contiguous()
    _same(t, refs.tensor("bilinear", "yuv_i16", None, False), "resize=None is the configured size")
    # out=, pitch and frame_stride: written in place, strided, nothing between the rows or past the layout
    stride = 3 * 48 * 9 + 32
    out = torch.full((4 * stride // 2 + 64,), 0x5a5a, dtype=torch.int16, device="cuda")
    t = dev.acc_warp_tensors(ba, bb, "rgb_i16", resize=(17, 9), interp="bilinear", colorspace=5, full_range=True, out=out,
                             pitch=48, frame_stride=stride)
    torch.cuda.synchronize()
    assert t.data_ptr() == out.data_ptr() and t.stride() == (stride // 2, 24 * 9, 24, 1) and tuple(t.shape) == (4, 3, 9, 17)
    _same(t, refs.tensor("bilinear", "rgb_i16", (17, 9), False, 5, 1), "out=, pitched")
    host = out.cpu().numpy()
    frames_ = host[:4 * stride // 2].reshape(4, stride // 2)
    assert (frames_[:, :3 * 24 * 9].reshape(4, 27, 24)[:, :, 17:] == 0x5a5a).all() and (frames_[:, 3 * 24 * 9:] == 0x5a5a).all()
    assert (host[4 * stride // 2:] == 0x5a5a).all()
    with pytest.raises(ValueError):
        dev.acc_warp_tensors(ba, bb, "rgb_i16", resize=(17, 9), out=out[:100])
    with pytest.raises(ValueError):
        dev.acc_warp_tensors(ba, bb, "rgb_i16", resize=(17, 9), out=out.view(torch.float16))
    with pytest.raises(ValueError):
        dev.acc_warp_tensors(ba, bb[:2], "rgb_i16", resize=(17, 9))
    # a torch side stream as the current stream, and its handle
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        t = dev.acc_warp_tensors(ba, bb, "yuv_f16", resize=(130, 5), interp="bilinear", coverage=True)
        side.synchronize()
    _same(t, refs.tensor("bilinear", "yuv_f16", (130, 5), True), "torch side stream")
    t = dev.acc_warp_tensors(ba, bb, "rgb_i16", resize=(17, 9), stream=side.cuda_stream)
    side.synchronize()
    _same(t, refs.tensor("nearest", "rgb_i16", (17, 9), False), "stream handle")
    # the calls changed nothing they read
    for i in range(3):
        for p, (a, b) in enumerate(zip(pix[i], v9.visible(dev.download(i), W, H))):
            assert np.array_equal(a, b), "frame %d plane %d changed" % (i, p)
        cells, serial = dev.download_motion_acc(i)
        assert serial == serials[i] and cells.tobytes() == accs[i].tobytes()
    mv_before = [dev.download_motion(i) for i in range(3)]
    dev.acc_warp_tensors(ba, bb, "rgb_f16", resize=(17, 9))
    torch.cuda.synchronize()
    for i in range(3):
        for a, b in zip(mv_before[i], dev.download_motion(i)):
            assert a.tobytes() == b.tobytes()
    # another frame decoded into the root's buffer: its serial is new, so nothing applies
    t = dev.acc_warp_tensors([1, 2], [0, 0], "yuv_i16", resize=(17, 9), coverage=True)
    torch.cuda.synchronize()
    assert int(t[:, 3].sum()) > 0
    later = v9.SynthFrame(v9.synth_params(W, H, 8, seed=7700))
    dev.stage_batch([later], [0])
    dev.run_batch()
    dev.sync()
    for fmt in ("yuv_i16", "rgb_f16"):
        t = dev.acc_warp_tensors([1, 2], [0, 0], fmt, resize=(17, 9), coverage=True)
        torch.cuda.synchronize()
        assert not bits(t.cpu().numpy()).any(), fmt
    # and a later decode is what it would have been without the calls
    fresh = _device(v9, (W, H), 5)
    try:
        for d in (dev, fresh):
            d.stage_batch(frames, [2, 3, 4], [None, (2, 2, 2), (3, 2, 2)])
            d.run_batch()
            d.sync()
        for i in (2, 3, 4):
            for a, b in zip(v9.visible(dev.download(i), W, H), v9.visible(fresh.download(i), W, H)):
                assert np.array_equal(a, b)
            assert dev.download_motion_acc(i)[0]["dx"].tobytes() == fresh.download_motion_acc(i)[0]["dx"].tobytes()
    finally:
        fresh.close()


# ------------------------------------------------------------------ the decoder's frames
@pytest.fixture(scope="module")
def decoded_tensors():
    return {}


COMBOS = [("nearest", "rgb_f16", (17, 9), True), ("bilinear", "yuv_i16", None, False), ("bilinear", "rgb_i16", (130, 5), True),
          ("nearest", "yuv_f16", (1, 1), False)]


@pytest.mark.parametrize("max_batch", [1, 7])
def test_decoder(v9, stream_acc, decoded_tensors, max_batch):  # noqa: F811
    """Every output of the stream with a hidden frame and a show_existing_frame, held, against
    the key frame; the fields of the reference come from a separate Stream parse."""
    pkts, want_acc, xi, hidden = stream_acc
    dec = v9.Decoder(0, export_motion_acc=True, max_batch=max_batch)
    try:
        infos = [info for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False)]
        assert len(infos) == len(want_acc) == 8
        pix = [_download(v9, dec, i) for i in infos]
        accs, serials = [a for a, _ in want_acc], [s for _, s in want_acc]
        w, h = infos[0].width, infos[0].height
        cs = 2 if infos[0].colorspace in (0, 6) else infos[0].colorspace
        full = infos[0].full_range
        refs = _Refs([(t, 0) for t in range(8)], pix, accs, serials, w, h, 1, 1, 8)
        res = {}
        for interp, fmt, size, cov in COMBOS:
            got = dec.acc_warp_tensors(infos, [infos[0]] * 8, fmt, resize=size, interp=interp, coverage=cov)
            _same(got, refs.tensor(interp, fmt, size, cov, cs, full), "decoder batch %d %s %s -> %s" % (max_batch, interp, fmt, size))
            res[interp, fmt] = got.cpu().numpy().copy()
        assert bits(res["nearest", "rgb_f16"][1:, 3]).any()             # something applies in the inter frames
        # the shown-existing output is the hidden frame: its own field and serial, as a and as b
        pairs = [(xi + 1, xi), (xi, xi)]
        got = dec.acc_warp_tensors([infos[a] for a, _ in pairs], [infos[b] for _, b in pairs], "yuv_i16", resize=(17, 9), coverage=True)
        _same(got, _Refs(pairs, pix, accs, serials, w, h, 1, 1, 8).tensor("nearest", "yuv_i16", (17, 9), True), "shown existing")
        out = torch.full((2 * 4 * 9 * 17,), 0x5a5a, dtype=torch.int16, device="cuda")
        mixed = type(infos[1]).from_buffer_copy(infos[1])
        mixed.width -= 16
        colour = type(infos[1]).from_buffer_copy(infos[1])
        colour.colorspace = 5 if infos[1].colorspace != 5 else 1
        ranged = type(infos[1]).from_buffer_copy(infos[1])
        ranged.full_range ^= 1
        for args in (([mixed], [infos[0]]), ([infos[1]], [mixed]), ([infos[1], colour], [infos[0]] * 2),
                     ([infos[1], ranged], [infos[0]] * 2)):
            with pytest.raises(v9.Vp9HipError) as e:             # two sizes; two colour descriptions in one call
                dec.acc_warp_tensors(*args, "rgb_i16", resize=(17, 9), coverage=True, out=out)
            assert e.value.code == v9.EINVAL
        dec.release(infos[0].buf)
        with pytest.raises(v9.Vp9HipError) as e:                 # a released root is not the caller's
            dec.acc_warp_tensors([infos[1]], [infos[0]], "rgb_i16", resize=(17, 9), coverage=True, out=out)
        assert e.value.code == v9.EINVAL
        torch.cuda.synchronize()
        assert bool((out == 0x5a5a).all())
        for i in infos[1:]:
            dec.release(i.buf)
    finally:
        dec.close()
    decoded_tensors[max_batch] = res
    if len(decoded_tensors) == 2:                                # both batch sizes equal each other
        for key in res:
            assert np.array_equal(bits(decoded_tensors[1][key]), bits(decoded_tensors[7][key])), key


def test_decoder_without_the_flag(v9, stream_acc):  # noqa: F811
    dec = v9.Decoder(0, export_motion=True, max_batch=4)
    try:
        infos = [info for _, info in dec.decode([(d, i) for i, d in enumerate(stream_acc[0][:2])], download=False)]
        with pytest.raises(v9.Vp9HipError) as e:
            dec.acc_warp_tensors([infos[1]], [infos[0]], "rgb_f16", resize=(17, 9))
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()
