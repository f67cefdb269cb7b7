"""Accumulated residual on the GPU: k_acc_warp against the numpy restatement of the definition
(tests/test_acc_warp_definition.py, which shares no code with the library). Exact equality.

Chains: the key + 6 inter GOPs of tests/test_motion_acc_definition.py are decoded once a shape;
the pixels and the accumulated fields are downloaded, and one call warps the 18 pairs (t, 0),
(t, t - 1), (t, t), t = 1 .. 6, in both modes and both outputs with the mask. What the inputs
exercise is asserted first, from the reference alone (warp_stats; measured on the CPU):

  input         pair    applying cells          clamped at a plane edge, nearest (of applying cells
                                                with a visible luma sample)
  66x66         (6, 0)  >= 1/2     0.83         >= 1/10    0.38
  200x130       (6, 0)  >= 1/2     0.57         >= 1/10    0.17
  mv_range=512  (6, 0)  >= 3/4     0.79         >= 9/10    1.00
  200x130       (6, 5)  0 < . < 1/4   0.18      (the root match separates cells inside one call)
  8x8           (6, 0)  none: the residual is zero and the picture is frame 6

Then crafted fields through vp9hip_warp_launch_dev (the hand-made cases of the definition test,
33 pairs across the split at 32, guard bytes around the destination), the lifecycle rules, and
the bitstream decoder.
"""
try:     # torch first: acc_warp returns torch views that share the HIP runtime (see _torch_first)
    import torch
except Exception:  # pragma: no cover
    torch = None

import ctypes

import numpy as np
import pytest

from test_acc_warp_definition import MODES, hand_cases, warp_ref, warp_stats
from test_gpu_motion_acc import stream_acc  # noqa: F401  (a fixture: the hidden-frame stream and its reference fields)
from test_motion_acc_definition import gop_parents

pytestmark = pytest.mark.gpu

N = 7
REFS = [None] + [gop_parents(t) for t in range(1, N)]       # buffer t holds frame t, serial t + 1
PAIRS = [(t, b) for t in range(1, N) for b in (0, t - 1, t)]


def _gop(v9, w, h, bpp=8, ss_h=1, ss_v=1, seed=7100, n=N, **kw):
    """gop_frames of tests/test_motion_acc_definition.py, at any depth and subsampling."""
    kw = dict(dict(mv_range=64, ref_mix=0, ss_h=ss_h, ss_v=ss_v), **kw)
    return [v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + t, inter=int(t > 0), compound=int(t > 1), **kw))
            for t in range(n)]


def _device(v9, cfg, nbufs, bpp=8, ss_h=1, ss_v=1, acc=True):
    dev = v9.Device(0)
    dev.set_export(motion=True, motion_acc=acc)
    dev.configure(cfg[0], cfg[1], bpp, nbufs=nbufs, ss_h=ss_h, ss_v=ss_v)
    dev.set_timing(False)
    return dev


def _same(got, want, what):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s: %d elements differ, first %s: got %s, want %s" % (
            what, len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def _check_call(got, pairs, pix, accs, serials, w, h, ss_h, ss_v, interp, output, what):
    """A call's (y, u, v, mask) against the restatement, pair by pair."""
    for i, (a, b) in enumerate(pairs):
        want, wmask = warp_ref(pix[a], pix[b], accs[a], serials[b], w, h, ss_h, ss_v, interp, output)
        for p in range(3):
            _same(got[p][i], want[p], "%s %s %s pair %s plane %d" % (what, interp, output, (a, b), p))
        _same(got[3][i], wmask, "%s pair %s mask" % (what, (a, b)))


CHAINS = {
    "8x8": dict(w=8, h=8),
    "66x66": dict(w=66, h=66, applying=0.5, edge=0.1),
    "200x130": dict(w=200, h=130, applying=0.5, edge=0.1, partial=True),
    "528x72-2tiles": dict(w=528, h=72, synth=dict(log2_tile_cols=1)),
    "66x34-in-200x130-mv512": dict(w=66, h=34, cfg=(200, 130), synth=dict(mv_range=512), applying=0.75, edge=0.9),
    "200x130-refmix": dict(w=200, h=130, synth=dict(ref_mix=1)),
    "66x66-10bit": dict(w=66, h=66, bpp=10),
    "66x66-444": dict(w=66, h=66, ss=(0, 0)),
    "66x66-440": dict(w=66, h=66, ss=(0, 1)),
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains(v9, name):
    c = CHAINS[name]
    w, h, bpp, (ss_h, ss_v) = c["w"], c["h"], c.get("bpp", 8), c.get("ss", (1, 1))
    frames = _gop(v9, w, h, bpp, ss_h, ss_v, **c.get("synth", {}))
    dev = _device(v9, c.get("cfg", (w, h)), N, bpp, ss_h, ss_v)
    try:
        dev.stage_batch(frames, list(range(N)), REFS)
        dev.run_batch()
        dev.sync()
        pix = [v9.visible(dev.download(i), w, h, ss_h, ss_v) for i in range(N)]
        fields = [dev.download_motion_acc(i) for i in range(N)]
        accs, serials = [f[0] for f in fields], [f[1] for f in fields]
        assert serials == list(range(1, N + 1))
        # what the inputs exercise, from the reference alone
        far = warp_stats(accs[6], serials[0], w, h, ss_h, ss_v)
        print("%s (6, 0): applying %.2f, clamped at an edge %.2f" % (name, far["applying"], far["edge"]))
        if "applying" in c:
            assert far["applying"] >= c["applying"] and far["edge"] >= c["edge"], far
        if c.get("partial"):
            near = warp_stats(accs[6], serials[5], w, h, ss_h, ss_v)
            print("%s (6, 5): applying %.2f" % (name, near["applying"]))
            assert 0 < near["applying"] < 0.25, near
        if name == "8x8":
            assert far["applying"] == 0
        assert all(warp_stats(accs[t], serials[t], w, h, ss_h, ss_v)["applying"] == 0 for t in range(1, N))   # (t, t): intra cells have no hops
        ba, bb = [a for a, _ in PAIRS], [b for _, b in PAIRS]
        for interp, output in MODES:
            got = dev.acc_warp(ba, bb, output=output, interp=interp, mask=True, size=(w, h))
            torch.cuda.synchronize()
            _check_call(got, PAIRS, pix, accs, serials, w, h, ss_h, ss_v, interp, output, name)
            if name == "8x8":
                i = PAIRS.index((6, 0))
                for p in range(3):
                    want = pix[6][p].astype(np.int16) if output == "picture" else np.zeros_like(pix[6][p], np.int16)
                    _same(got[p][i], want, "8x8 (6, 0): nothing applies")
    finally:
        dev.close()


# ------------------------------------------------------------------ crafted fields through vp9hip_warp_launch_dev
def _pack(planes, pitch, bypp, poison):
    """A frame buffer holding three planes at the given (luma, chroma) pitches in bytes, `poison`
    wherever no visible sample lies: (cuda uint8 tensor, plane offsets)."""
    rows = [p.shape[0] for p in planes]
    off = [0, pitch[0] * rows[0], pitch[0] * rows[0] + pitch[1] * rows[1]]
    buf = np.full(off[2] + pitch[1] * rows[2], poison, np.uint8)
    for p, a in enumerate(planes):
        pt = pitch[1 if p else 0]
        view = buf[off[p]:off[p] + pt * rows[p]].reshape(rows[p], pt)
        view[:, :a.shape[1] * bypp] = np.ascontiguousarray(a).view(np.uint8).reshape(rows[p], -1)
    return torch.from_numpy(buf).cuda(), off


def _launch_dev(v9, pairs, w, h, bpp, ss_h, ss_v, interp, output, pad, guard=64):
    """pairs of (A, B, acc, sb) of one geometry through the raw entry: ((y, u, v, mask) numpy
    arrays with the pair first, True if the guard bytes around dst and mask are unchanged)."""
    bypp = 1 if bpp == 8 else 2
    cw, ch = (w + ss_h) >> ss_h, (h + ss_v) >> ss_v
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
    n = len(pairs)
    stride, doff = v9.warp_layout(w, h, ss_h, ss_v)
    dst = torch.full((guard + n * stride + guard,), 0x5a, dtype=torch.uint8, device="cuda")
    mask = torch.full((guard + n * gh * gw + guard,), 0x5a, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    v9.warp_launch_dev(ap, bp, cp, [sb for _, _, _, sb in pairs], off, pitch, gw + pad, w, h, bpp, ss_h, ss_v, interp, output,
                       dst.data_ptr() + guard, mask.data_ptr() + guard, None)
    torch.cuda.synchronize()
    d, m = dst.cpu().numpy(), mask.cpu().numpy()
    clean = bool((d[:guard] == 0x5a).all() and (d[guard + n * stride:] == 0x5a).all() and
                 (m[:guard] == 0x5a).all() and (m[guard + n * gh * gw:] == 0x5a).all())
    body = d[guard:guard + n * stride].reshape(n, stride)
    planes = [np.ascontiguousarray(body[:, o:o + 2 * pw * ph]).view(np.int16).reshape(n, ph, pw)
              for o, (pw, ph) in zip(doff, ((w, h), (cw, ch), (cw, ch)))]
    return planes + [m[guard:guard + n * gh * gw].reshape(n, gh, gw)], clean


def test_hand_made_cases_on_the_device(v9):
    """The definition test's cases, one launch each and mode; every other case with planes and a
    field pitched 3 elements past their width (rows that no vector access fits) and poison there."""
    for k, (name, A, B, acc, sb, w, h, bpp, ss_h, ss_v) in enumerate(hand_cases()):
        for interp, output in MODES:
            got, clean = _launch_dev(v9, [(A, B, acc, sb)], w, h, bpp, ss_h, ss_v, interp, output, pad=3 * (k & 1))
            assert clean, "%s: bytes outside the layout changed" % name
            want, wmask = warp_ref(A, B, acc, sb, w, h, ss_h, ss_v, interp, output)
            for p in range(3):
                _same(got[p][0], want[p], "%s %s %s plane %d" % (name, interp, output, p))
            _same(got[3][0], wmask, name + " mask")


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
    for interp, output in MODES:
        got, clean = _launch_dev(v9, pairs, w, h, 8, 1, 1, interp, output, pad=0)
        assert clean
        masks = 0
        for i, (A, B, acc, sb) in enumerate(pairs):
            want, wmask = warp_ref(A, B, acc, sb, w, h, 1, 1, interp, output)
            for p in range(3):
                _same(got[p][i], want[p], "pair %d %s %s plane %d" % (i, interp, output, p))
            _same(got[3][i], wmask, "pair %d mask" % i)
            masks += int(wmask.sum())
        assert 4 < masks < 33 * 4


def test_launch_dev_refuses_bad_arguments(v9):
    L = v9.lib()
    t = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    one = (ctypes.c_void_p * 1)(t.data_ptr())
    ser = (ctypes.c_uint32 * 1)(1)
    off, pitch = (ctypes.c_int64 * 3)(0, 64, 80), (ctypes.c_int32 * 2)(8, 4)

    def call(a=one, b=one, acc=one, s=ser, n=1, off=off, pitch=pitch, ap=2, w=8, h=8, bpp=8, sh=1, sv=1, mode=0, out=0,
             dst=t.data_ptr() + 1024):
        return L.vp9hip_warp_launch_dev(a, b, acc, s, n, ctypes.byref(off) if off else None, ctypes.byref(pitch) if pitch else None,
                                        ap, w, h, bpp, sh, sv, mode, out, dst, None, None)
    bad = [dict(a=None), dict(b=None), dict(acc=None), dict(s=None), dict(n=0), dict(off=None), dict(pitch=None), dict(ap=1),
           dict(w=0), dict(h=16385), dict(bpp=9), dict(sh=2), dict(sv=-1), dict(mode=2), dict(out=-1), dict(dst=None),
           dict(dst=t.data_ptr() + 1026), dict(pitch=(ctypes.c_int32 * 2)(7, 4)), dict(pitch=(ctypes.c_int32 * 2)(8, 3)),
           dict(acc=(ctypes.c_void_p * 1)(t.data_ptr() + 8)), dict(a=(ctypes.c_void_p * 1)(None)),
           dict(bpp=10, pitch=(ctypes.c_int32 * 2)(17, 8))]
    for kw in bad:
        assert call(**kw) == v9.EINVAL, kw
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ------------------------------------------------------------------ lifecycle
W, H = 200, 130


@pytest.fixture
def chain3(v9):
    """Key + 2 inter at 200x130 in buffers 0..2 of a 5-buffer context: (dev, pixels, fields)."""
    frames = _gop(v9, W, H, seed=7600, n=3)
    dev = _device(v9, (W, H), 5)
    dev.stage_batch(frames, [0, 1, 2], REFS[:3])
    dev.run_batch()
    dev.sync()
    yield dev, frames
    dev.close()


def test_errors_write_nothing(v9, chain3):
    dev, frames = chain3
    stride, _ = v9.warp_layout(W, H)
    out = torch.full((2 * stride // 2,), 0x5a5a, dtype=torch.int16, device="cuda")
    cases = [(dict(bufs=[1, 5], root_bufs=[0, 0]), v9.EINVAL), (dict(bufs=[1], root_bufs=[-1]), v9.EINVAL),
             (dict(bufs=[-1], root_bufs=[0]), v9.EINVAL), (dict(bufs=[1], root_bufs=[5]), v9.EINVAL),
             (dict(bufs=[], root_bufs=[]), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], size=(W + 1, H)), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], size=(W, H + 1)), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], size=(0, H)), v9.EINVAL), (dict(bufs=[1], root_bufs=[0], size=(W, 0)), v9.EINVAL),
             (dict(bufs=[1], root_bufs=[0], size=(W - 8, H)), v9.EINVAL),      # another grid than the field's
             (dict(bufs=[1], root_bufs=[0], size=(W, H - 10)), v9.EINVAL),
             (dict(bufs=[1, 3], root_bufs=[0, 0]), v9.EAGAIN),                  # never written: no field
             (dict(bufs=[1, 1], root_bufs=[0, 4]), v9.EAGAIN)]
    for kw, code in cases:
        with pytest.raises(v9.Vp9HipError) as e:
            dev.acc_warp(out=out, mask=True, **kw)
        assert e.value.code == code, kw
    for kw in (dict(output="sum"), dict(interp="cubic")):
        with pytest.raises(v9.Vp9HipError) as e:
            dev.acc_warp([1], [0], out=out, **kw)
        assert e.value.code == v9.EINVAL
    L = v9.lib()
    one, zero = (ctypes.c_int * 1)(1), (ctypes.c_int * 1)(0)
    assert L.vp9hip_acc_warp(dev._c, None, zero, 1, W, H, 0, 0, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, None, 1, W, H, 0, 0, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, 1, W, H, 0, 0, None, None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(None, one, zero, 1, W, H, 0, 0, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, -1, W, H, 0, 0, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, 1, W, H, 2, 0, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, 1, W, H, 0, 2, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, 1, W, H, -1, 0, out.data_ptr(), None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, 1, W, H, 0, 0, out.data_ptr() + 2, None, None) == v9.EINVAL
    assert L.vp9hip_acc_warp(dev._c, one, zero, 1, W, H, 0, 0, out.data_ptr() + 4, None, None) == v9.EINVAL
    dev.upload(4, v9.alloc_planes(W, H, 8))              # an uploaded b holds pixels and no field
    with pytest.raises(v9.Vp9HipError) as e:
        dev.acc_warp([1], [4], out=out)
    assert e.value.code == v9.EAGAIN
    for other in (_device(v9, (W, H), 2, acc=False), v9.Device(0)):   # motion export alone; not configured
        try:
            if other.w:
                other.stage_batch(frames[:2], [0, 1], REFS[:2])
                other.run_batch()
                other.sync()
            with pytest.raises(v9.Vp9HipError) as e:
                other.acc_warp([1], [0], size=(W, H), out=out)
            assert e.value.code == v9.EINVAL
        finally:
            other.close()
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a).all())


def test_a_refused_run_leaves_no_field(v9):
    frames = _gop(v9, W, H, seed=7400, n=3)
    v9.test_hooks(reject_batch=1, reject_frame=1)
    try:
        dev = v9.Device(0)
    finally:
        v9.test_hooks()
    try:
        dev.set_export(motion=True, motion_acc=True)
        dev.configure(W, H, 8, nbufs=3)
        dev.set_timing(False)
        dev.stage_batch(frames, [0, 1, 2], REFS[:3])
        with pytest.raises(v9.Vp9HipError) as e:
            dev.run_batch()
        assert e.value.code == v9.EINVALIDDATA
        out = torch.full((v9.warp_layout(W, H)[0] // 2,), 0x5a5a, dtype=torch.int16, device="cuda")
        for a, b in ((1, 0), (2, 2), (0, 0)):
            with pytest.raises(v9.Vp9HipError) as e:
                dev.acc_warp([a], [b], out=out)
            assert e.value.code == v9.EAGAIN
        torch.cuda.synchronize()
        assert bool((out == 0x5a5a).all())
        dev.stage_batch(frames, [0, 1, 2], REFS[:3])     # the hook names the first batch only
        dev.run_batch()
        dev.sync()
        m = dev.acc_warp([1], [0], mask=True)[3]
        torch.cuda.synchronize()
        assert int(m.sum()) > 0
    finally:
        dev.close()


def test_views_out_stream_and_an_overwritten_root(v9, chain3):
    dev, frames = chain3
    pix = [v9.visible(dev.download(i), W, H) for i in range(3)]
    fields = [dev.download_motion_acc(i) for i in range(3)]
    accs, serials = [f[0] for f in fields], [f[1] for f in fields]
    pairs = [(1, 0), (2, 0), (2, 1), (2, 2)]
    ba, bb = [a for a, _ in pairs], [b for _, b in pairs]
    stride, off = v9.warp_layout(W, H)
    cw, ch, gw, gh = (W + 1) >> 1, (H + 1) >> 1, 2 * ((W + 7) >> 3), 2 * ((H + 7) >> 3)
    # the views: int16, one allocation, the layout's offsets and strides
    y, u, v, m = dev.acc_warp(ba, bb, mask=True)
    torch.cuda.synchronize()
    assert (y.dtype, u.dtype, v.dtype, m.dtype) == (torch.int16, torch.int16, torch.int16, torch.uint8)
    assert tuple(y.shape) == (4, H, W) and tuple(u.shape) == (4, ch, cw) and tuple(v.shape) == (4, ch, cw) and tuple(m.shape) == (4, gh, gw)
    assert y.stride() == (stride // 2, W, 1) and u.stride() == (stride // 2, cw, 1) and v.stride() == (stride // 2, cw, 1)
    assert u.data_ptr() == y.data_ptr() + off[1] and v.data_ptr() == y.data_ptr() + off[2] and m.is_contiguous()
    _check_call((y, u, v, m), pairs, pix, accs, serials, W, H, 1, 1, "nearest", "residual", "views")
    # out=: written in place, nothing past the layout; size= defaults to the configured size
    out = torch.full((4 * stride // 2 + 64,), 0x5a5a, dtype=torch.int16, device="cuda")
    got = dev.acc_warp(ba, bb, output="picture", interp="bilinear", mask=True, out=out)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out.data_ptr() and bool((out[4 * stride // 2:] == 0x5a5a).all())
    _check_call(got, pairs, pix, accs, serials, W, H, 1, 1, "bilinear", "picture", "out=")
    with pytest.raises(ValueError):
        dev.acc_warp(ba, bb, out=out[:100])
    with pytest.raises(ValueError):
        dev.acc_warp(ba, bb[:2])
    # stream=: a torch side stream as the current stream, and its handle
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = dev.acc_warp(ba, bb, interp="bilinear", mask=True)
        side.synchronize()
    _check_call(got, pairs, pix, accs, serials, W, H, 1, 1, "bilinear", "residual", "torch side stream")
    got = dev.acc_warp(ba, bb, output="picture", mask=True, stream=side.cuda_stream)
    side.synchronize()
    _check_call(got, pairs, pix, accs, serials, W, H, 1, 1, "nearest", "picture", "stream handle")
    # the call changed nothing it read
    for i in range(3):
        for p, (a, b) in enumerate(zip(pix[i], v9.visible(dev.download(i), W, H))):
            assert np.array_equal(a, b), "frame %d plane %d changed" % (i, p)
        cells, serial = dev.download_motion_acc(i)
        assert serial == serials[i] and cells.tobytes() == accs[i].tobytes()
    mv_before = [dev.download_motion(i) for i in range(3)]
    dev.acc_warp(ba, bb)
    torch.cuda.synchronize()
    for i in range(3):
        for a, b in zip(mv_before[i], dev.download_motion(i)):
            assert a.tobytes() == b.tobytes()
    # another frame decoded into the root's buffer: its serial is new, so nothing applies
    assert int(m[0].sum()) > 0
    later = v9.SynthFrame(v9.synth_params(W, H, 8, seed=7700))
    dev.stage_batch([later], [0])
    dev.run_batch()
    dev.sync()
    y2, u2, v2, m2 = dev.acc_warp([1, 2], [0, 0], mask=True)
    torch.cuda.synchronize()
    assert int(m2.sum()) == 0 and int(y2.abs().sum()) == 0 and int(u2.abs().sum()) == 0 and int(v2.abs().sum()) == 0
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
def decoded_warp():
    return {}


def _download(v9, dec, info):
    pl = v9.alloc_planes(info.width, info.height, 8)
    ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in pl])
    ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in pl])
    assert v9.lib().vp9hip_download_frame(dec.context(), info.buf, ptrs, ls) == 0
    return v9.visible(pl, info.width, info.height)


@pytest.mark.parametrize("max_batch", [1, 7])
def test_decoder(v9, stream_acc, decoded_warp, max_batch):  # noqa: F811
    """Every output of the stream with a hidden frame and a show_existing_frame, held, against
    the key frame; the fields of the reference come from a separate Stream parse."""
    pkts, want_acc, xi, hidden = stream_acc
    dec = v9.Decoder(0, export_motion_acc=True, max_batch=max_batch)
    try:
        infos = [info for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False)]
        assert len(infos) == len(want_acc) == 8
        pix = [_download(v9, dec, i) for i in infos]
        accs, serials = [a for a, _ in want_acc], [s for _, s in want_acc]
        assert serials[0] == 1 and serials[xi] == hidden[1]
        w, h = infos[0].width, infos[0].height
        pairs = [(t, 0) for t in range(8)]
        stats = [warp_stats(accs[t], 1, w, h) for t in range(1, 8)]
        assert all(s["applying"] > 0.25 for s in stats), [s["applying"] for s in stats]
        res = {}
        for interp, output in MODES:
            got = dec.acc_warp(infos, [infos[0]] * 8, output=output, interp=interp, mask=True)
            _check_call(got, pairs, pix, accs, serials, w, h, 1, 1, interp, output, "decoder batch %d" % max_batch)
            res[interp, output] = [t.cpu().numpy().copy() for t in got]
        # the shown-existing output is the hidden frame: its own field and serial, as a and as b
        got = dec.acc_warp([infos[xi + 1], infos[xi]], [infos[xi], infos[xi]], mask=True)
        _check_call(got, [(xi + 1, xi), (xi, xi)], pix, accs, serials, w, h, 1, 1, "nearest", "residual", "shown existing")
        mixed = type(infos[1]).from_buffer_copy(infos[1])
        mixed.width -= 16
        for args in (([mixed], [infos[0]]), ([infos[1]], [mixed])):
            with pytest.raises(v9.Vp9HipError) as e:
                dec.acc_warp(*args)
            assert e.value.code == v9.EINVAL
        dec.release(infos[0].buf)
        with pytest.raises(v9.Vp9HipError) as e:         # a released root is not the caller's
            dec.acc_warp([infos[1]], [infos[0]])
        assert e.value.code == v9.EINVAL
        for i in infos[1:]:
            dec.release(i.buf)
    finally:
        dec.close()
    decoded_warp[max_batch] = res
    if len(decoded_warp) == 2:                           # both batch sizes equal each other
        for key in res:
            for a, b in zip(decoded_warp[1][key], decoded_warp[7][key]):
                assert np.array_equal(a, b)


def test_decoder_without_the_flag(v9, stream_acc):  # noqa: F811
    dec = v9.Decoder(0, export_motion=True, max_batch=4)
    try:
        infos = [info for _, info in dec.decode([(d, i) for i, d in enumerate(stream_acc[0][:2])], download=False)]
        with pytest.raises(v9.Vp9HipError) as e:
            dec.acc_warp([infos[1]], [infos[0]])
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()
