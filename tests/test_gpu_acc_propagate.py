"""Accumulated propagation on the GPU: k_prop_nchw / k_prop_nhwc against the numpy restatement of
the definition (tests/test_acc_propagate_definition.py, which shares no code with the library).
Exact equality of bits.

Crafted fields through vp9hip_prop_launch_dev (the hand-made cases of the definition test in both
layouts, every other one with the field pitched 3 cells past GW and the tensors at addresses that
are only element-aligned, poison in the padding and guard bytes around the destination and the
valid map; 33 pairs across the split at 32). Chains: the key + 6 inter GOPs of
tests/test_gpu_acc_warp.py, decoded once a shape; one call carries the tensors of all seven frames
over the 18 pairs (t, serial of frame 0), (t, serial of t - 1), (t, own serial), t = 1 .. 6, on
four grids and in five configurations (eight with their modes). What the inputs exercise is asserted first, from the
reference alone, for the pair (6, root 0) on every grid (measured on the CPU, 66x66 / 200x130):

  applying samples               >= 1/4     0.83 .. 0.85 / 0.58 .. 0.63
  samples that do not apply      >= 1/10    0.15 .. 0.17 / 0.37 .. 0.42
  nearest source clamped         >= 1/20    0.30 .. 0.34 / 0.15 .. 0.18   (of the applying samples)
  both bilinear fractions != 0   >= 1/4     0.82 .. 0.98 / 0.76 .. 0.89   (of the applying samples)

Then the lifecycle rules and the bitstream decoder.
"""
try:     # torch first: acc_propagate takes and returns torch tensors that share the HIP runtime (see _torch_first)
    import torch
except Exception:  # pragma: no cover
    torch = None

import ctypes

import numpy as np
import pytest

from test_acc_propagate_definition import bits, hand_cases, prop_ref, prop_stats
from test_gpu_acc_warp import N, REFS, _device, _gop
from test_gpu_motion_acc import stream_acc  # noqa: F401  (a fixture: the hidden-frame stream and its reference fields)

pytestmark = pytest.mark.gpu

PAIRS = [(t, b) for t in range(1, N) for b in (0, t - 1, t)]
TO = {"nchw": (0, 1, 2), "nhwc": (1, 2, 0)}            # an item (C, FH, FW) into the layout, and back
BACK = {"nchw": (0, 1, 2), "nhwc": (2, 0, 1)}


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = bits(got) != bits(want)
    if bad.any():
        at = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: %d elements differ, first %s: got %#x, want %#x" % (
            what, int(bad.sum()), at, int(bits(got)[at]), int(bits(want)[at])))


def _np(t):
    """A cuda tensor as a numpy array; bits survive (no numpy type is needed for the view)."""
    return t.cpu().numpy()


# ------------------------------------------------------------------ crafted fields through vp9hip_prop_launch_dev
def _launch_dev(v9, srcs, pairs, w, h, interp, layout, fill, pre, pad, odd, guard=64):
    """pairs [(acc, S, src item)] over the items srcs (M, C, FH, FW) through the raw entry, in
    `layout`: (items (n, C, FH, FW), valid (n, FH, FW), True if the guard bytes around both are
    unchanged). pad: cells of poison past a field's row; odd: the tensors start one element past
    a 256-byte boundary."""
    M, C, FH, FW = srcs.shape
    E, n = srcs.dtype.itemsize, len(pairs)
    gw, gh = 2 * ((w + 7) >> 3), 2 * ((h + 7) >> 3)
    keep, ptrs = [], []
    for acc, _, _ in pairs:
        cells = np.full((gh, gw + pad, 4), 0x5a5a5a5a, np.int32)
        cells[:, :gw] = np.ascontiguousarray(acc).view(np.int32).reshape(gh, gw, 4)
        keep.append(torch.from_numpy(cells).cuda())
        ptrs.append(keep[-1].data_ptr())
    item = C * FH * FW * E
    off = 256 + (E if odd else 0)
    lay = lambda a: np.ascontiguousarray(a.transpose((0,) + tuple(1 + i for i in TO[layout])))   # noqa: E731
    sbuf = np.full(off + M * item + guard, 0xa5, np.uint8)
    sbuf[off:off + M * item] = lay(srcs).view(np.uint8).ravel()
    dbuf = np.full(off + n * item + guard, 0x5a, np.uint8)
    if pre is not None:
        dbuf[off:off + n * item] = lay(pre).view(np.uint8).ravel()
    ts, td = torch.from_numpy(sbuf).cuda(), torch.from_numpy(dbuf).cuda()
    tv = torch.full((guard + n * FH * FW + guard,), 0x5a, dtype=torch.uint8, device="cuda")
    bitsv = int.from_bytes(np.array([fill]).astype(srcs.dtype).tobytes(), "little")
    d = v9.PropDesc(w, h, FW, FH, C, E, v9.PROP_LAYOUTS[layout], v9.WARP_MODES[interp], v9.PROP_KEEP if pre is not None else 0, 0, bitsv)
    torch.cuda.synchronize()
    v9.prop_launch_dev(ptrs, gw + pad, [S for _, S, _ in pairs], [i for _, _, i in pairs], M, d, ts.data_ptr() + off,
                       td.data_ptr() + off, tv.data_ptr() + guard, None)
    torch.cuda.synchronize()
    dn, vn = td.cpu().numpy(), tv.cpu().numpy()
    clean = bool((dn[:off] == 0x5a).all() and (dn[off + n * item:] == 0x5a).all() and (vn[:guard] == 0x5a).all() and
                 (vn[guard + n * FH * FW:] == 0x5a).all() and (ts.cpu().numpy() == sbuf).all())
    shape = (n,) + tuple(np.array((C, FH, FW))[list(TO[layout])])
    out = dn[off:off + n * item].copy().view(srcs.dtype).reshape(shape).transpose((0,) + tuple(1 + i for i in BACK[layout]))
    return out, vn[guard:guard + n * FH * FW].reshape(n, FH, FW), clean


def _check_case(v9, c, layout, pad, odd):
    got, valid, clean = _launch_dev(v9, c["srcs"], c["pairs"], c["w"], c["h"], c["interp"], layout, c["fill"], c["pre"], pad, odd)
    assert clean, "%s %s: bytes outside the tensors changed" % (c["name"], layout)
    for k, (acc, S, i) in enumerate(c["pairs"]):
        want, wvalid = prop_ref(acc, S, c["srcs"][i], c["w"], c["h"], c["interp"], c["fill"], None if c["pre"] is None else c["pre"][k])
        _same(np.ascontiguousarray(got[k]), want, "%s pair %d %s" % (c["name"], k, layout))
        assert np.array_equal(valid[k], wvalid), "%s pair %d %s valid" % (c["name"], k, layout)


def test_hand_made_cases_on_the_device(v9):
    """The definition test's cases, one launch each and layout; every other case with the field
    pitched 3 cells past its width and the tensors only element-aligned, and poison there."""
    for k, c in enumerate(hand_cases()):
        for layout in ("nchw", "nhwc"):
            _check_case(v9, c, layout, pad=3 * (k & 1), odd=bool(k & 1))


def test_33_pairs_cross_the_launch_split(v9):
    rng = np.random.default_rng(33)
    w = h = 8
    for dtype, interp in ((np.int16, "nearest"), (np.float16, "bilinear"), (np.int64, "nearest")):
        srcs = rng.integers(0, 2000, (4, 3, 3, 5)).astype(dtype)
        pairs = []
        for i in range(33):
            acc = np.zeros((2, 2), v9.ACC_CELL)
            acc["dx"], acc["dy"] = rng.integers(-80, 80, (2, 2)), rng.integers(-80, 80, (2, 2))
            acc["root"], acc["hops"] = rng.integers(100 + i, 102 + i, (2, 2)), rng.integers(0, 3, (2, 2))
            if i == 32:                                  # the pair past the split applies everywhere
                acc["root"], acc["hops"] = 100 + i, 1
            pairs.append((acc, 100 + i, i % 4))
        c = dict(name="33 pairs %s" % np.dtype(dtype).name, w=w, h=h, srcs=srcs, pairs=pairs, interp=interp, fill=7, pre=None)
        masks = sum(int(prop_ref(acc, S, srcs[i], w, h)[1].sum()) for acc, S, i in pairs)
        assert int(prop_ref(*pairs[32][:2], srcs[0], w, h)[1].sum()) == 15 and 15 < masks < 33 * 15
        for layout in ("nchw", "nhwc"):
            _check_case(v9, c, layout, pad=0, odd=False)
            _check_case(v9, dict(c, pre=rng.integers(3000, 4000, (33, 3, 3, 5)).astype(dtype)), layout, pad=0, odd=True)


def test_launch_dev_refuses_bad_arguments(v9):
    L = v9.lib()
    t = torch.zeros(8192, dtype=torch.uint8, device="cuda")
    base = t.data_ptr()
    one, ser, idx = (ctypes.c_void_p * 1)(base), (ctypes.c_uint32 * 1)(1), (ctypes.c_int * 1)(0)
    good = dict(width=8, height=8, fw=5, fh=3, channels=3, elem_size=2, layout=0, mode=0, flags=0, reserved=0, fill=0)

    def call(acc=one, ap=2, s=ser, i=idx, n=1, m=1, d=good, src=base + 1024, dst=base + 4096):
        dd = v9.PropDesc(**d) if d else None
        return L.vp9hip_prop_launch_dev(acc, ap, s, i, n, m, ctypes.byref(dd) if dd else None, src, dst, None, None)
    assert call(i=None) == 0                             # a NULL src_index is pair i -> item i
    bad = [dict(acc=None), dict(ap=1), dict(s=None), dict(n=0), dict(m=0), dict(d=None), dict(src=None), dict(dst=None),
           dict(i=(ctypes.c_int * 1)(1)), dict(i=(ctypes.c_int * 1)(-1)), dict(i=None, n=2, m=1, acc=(ctypes.c_void_p * 2)(base, base)),
           dict(acc=(ctypes.c_void_p * 1)(base + 8)), dict(acc=(ctypes.c_void_p * 1)(None)),
           dict(src=base + 1025), dict(dst=base + 4097), dict(dst=base + 1024), dict(dst=base + 1024 + 88), dict(dst=base + 1024 - 88),
           dict(d=dict(good, width=0)), dict(d=dict(good, fw=16385)), dict(d=dict(good, channels=4097)), dict(d=dict(good, elem_size=3)),
           dict(d=dict(good, layout=2)), dict(d=dict(good, mode=2)), dict(d=dict(good, mode=1, elem_size=4)), dict(d=dict(good, flags=2)),
           dict(d=dict(good, reserved=1))]
    torch.cuda.synchronize()
    t.zero_()
    for kw in bad:
        assert call(**kw) == v9.EINVAL, kw
    assert call(dst=base + 1024 + 90) == 0 and call(dst=base + 1024 - 90) == 0        # the ranges touch and do not overlap
    torch.cuda.synchronize()


# ------------------------------------------------------------------ chains
CONFIGS = {
    "u8-c1": dict(dtype=np.uint8, C=1, layout="nchw", interps=("nearest",)),
    "i64-c1": dict(dtype=np.int64, C=1, layout="nchw", interps=("nearest",)),
    "f16-c19-nchw": dict(dtype=np.float16, C=19, layout="nchw", interps=("nearest", "bilinear")),
    "f16-c19-nhwc": dict(dtype=np.float16, C=19, layout="nhwc", interps=("nearest", "bilinear")),
    "f16-c64-nhwc": dict(dtype=np.float16, C=64, layout="nhwc", interps=("nearest", "bilinear")),
}
SHAPES = {"66x66": (66, 66, (66, 66)), "200x130": (200, 130, (200, 130))}


@pytest.fixture(scope="module")
def gops(v9):
    """Per shape, decoded once: (dev, accumulated fields, serials); the devices stay open for the module."""
    out = {}
    for name, (w, h, cfg) in SHAPES.items():
        dev = _device(v9, cfg, N)
        dev.stage_batch(_gop(v9, w, h), list(range(N)), REFS)
        dev.run_batch()
        dev.sync()
        fields = [dev.download_motion_acc(i) for i in range(N)]
        out[name] = (dev, [f[0] for f in fields], [f[1] for f in fields])
    yield out
    for dev, _, _ in out.values():
        dev.close()


def _grids(w, h):
    return [(w, h), ((w + 1) >> 1, (h + 1) >> 1), (14, 9), (2 * w + 3, h)]


@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_chains_exercise_what_they_claim(gops, shape):
    """From the reference alone, for the pair (6, root 0) on every grid; conditions, not measurements."""
    w, h, _ = SHAPES[shape]
    _, accs, serials = gops[shape]
    assert serials == list(range(1, N + 1))
    for fw, fh in _grids(w, h):
        s = prop_stats(accs[6], serials[0], w, h, fw, fh)
        print("%s grid %dx%d (6, root 0): applying %.2f, not applying %.2f, clamped at an edge %.3f, both fractions %.2f" % (
            shape, fw, fh, s["applying"], 1 - s["applying"], s["edge"], s["both"]))
        assert s["applying"] >= 1 / 4 and 1 - s["applying"] >= 1 / 10 and s["edge"] >= 1 / 20 and s["both"] >= 1 / 4, s
        for t in range(1, N):                            # (t, own serial): intra cells have no hops
            assert prop_stats(accs[t], serials[t], w, h, fw, fh)["applying"] == 0


@pytest.mark.parametrize("config", list(CONFIGS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_chains(v9, gops, shape, config):
    w, h, _ = SHAPES[shape]
    dev, accs, serials = gops[shape]
    c = CONFIGS[config]
    rng = np.random.default_rng(len(config) + w)
    ba, roots, idx = [a for a, _ in PAIRS], [serials[b] for _, b in PAIRS], [b for _, b in PAIRS]
    for fw, fh in _grids(w, h):
        if c["dtype"] == np.float16:                     # finite halves of every size, a tenth of them subnormal
            b = rng.integers(0, 0x7c00, (N, c["C"], fh, fw)).astype(np.uint16)
            b[rng.random(b.shape) < 0.1] &= 0x03ff
            items = (b | (rng.integers(0, 2, b.shape).astype(np.uint16) << 15)).view(np.float16)
        else:
            items = rng.integers(0, 256, (N, c["C"], fh, fw, np.dtype(c["dtype"]).itemsize), dtype=np.uint8).view(c["dtype"])[..., 0]
        lay = np.ascontiguousarray(items.transpose((0,) + tuple(1 + i for i in TO[c["layout"]])))
        src = torch.from_numpy(lay[:, 0] if c["C"] == 1 else lay).cuda()
        for interp in c["interps"]:
            got, valid = dev.acc_propagate(ba, roots, src, interp=interp, layout=c["layout"], fill=3, valid=True, src_index=idx,
                                           size=(w, h))
            torch.cuda.synchronize()
            assert got.dtype == src.dtype and tuple(got.shape) == (len(PAIRS),) + tuple(src.shape[1:]) and got.is_contiguous()
            assert valid.dtype == torch.uint8 and tuple(valid.shape) == (len(PAIRS), fh, fw)
            g, vm = _np(got), _np(valid)
            if c["C"] == 1:
                g = g[:, None]
            g = g.transpose((0,) + tuple(1 + i for i in BACK[c["layout"]]))
            for k, (a, b) in enumerate(PAIRS):
                want, wvalid = prop_ref(accs[a], serials[b], items[b], w, h, interp, 3)
                _same(np.ascontiguousarray(g[k]), want, "%s %s grid %dx%d %s pair %s" % (shape, config, fw, fh, interp, (a, b)))
                assert np.array_equal(vm[k], wvalid)
                if a == b:
                    assert not wvalid.any()


# ------------------------------------------------------------------ lifecycle
W, H = 200, 130
FW, FH = 50, 33


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


def _labels(rng, m, c=None, lo=0, hi=100):
    shape = (m, FH, FW) if c is None else (m, c, FH, FW)
    return rng.integers(lo, hi, shape).astype(np.int16)


def test_errors_write_nothing(v9, chain3):
    dev, frames = chain3
    rng = np.random.default_rng(1)
    src = torch.from_numpy(_labels(rng, 2, 3)).cuda()
    out = torch.full((2, 3, FH, FW), 0x5a5a, dtype=torch.int16, device="cuda")
    ok = dict(bufs=[1, 2], root_serials=[1, 1])
    cases = [(dict(bufs=[1, 5], root_serials=[1, 1]), v9.EINVAL), (dict(bufs=[-1, 1], root_serials=[1, 1]), v9.EINVAL),
             (dict(ok, src_index=[0, 2]), v9.EINVAL), (dict(ok, src_index=[-1, 0]), v9.EINVAL),
             (dict(ok, size=(W + 1, H)), v9.EINVAL), (dict(ok, size=(W, H + 1)), v9.EINVAL), (dict(ok, size=(0, H)), v9.EINVAL),
             (dict(ok, size=(W - 8, H)), v9.EINVAL), (dict(ok, size=(W, H - 10)), v9.EINVAL),      # another grid than the field's
             (dict(ok, interp="cubic"), v9.EINVAL), (dict(ok, layout="chwn"), v9.EINVAL),
             (dict(bufs=[1, 3], root_serials=[1, 1]), v9.EAGAIN),                                  # never written: no field
             (dict(bufs=[4, 1], root_serials=[1, 1]), v9.EAGAIN)]
    for kw, code in cases:
        with pytest.raises(v9.Vp9HipError) as e:
            dev.acc_propagate(src=src, out=out, valid=True, **kw)
        assert e.value.code == code, kw
    with pytest.raises(v9.Vp9HipError) as e:             # n = 0
        dev.acc_propagate([], [], src[:1], out=out[:0])
    assert e.value.code == v9.EINVAL
    for kw in (dict(keep=True, out=None), dict(interp="bilinear"), dict(out=out[:1]), dict(out=out.to(torch.int32)),
               dict(root_serials=[1]), dict(src_index=[0]), dict(src=src.cpu()), dict(src=src[:, :, :, ::2])):
        with pytest.raises(ValueError):
            dev.acc_propagate(**dict(dict(ok, src=src, out=out), **kw))
    with pytest.raises(ValueError):                      # three items for two pairs, and no index
        dev.acc_propagate(src=torch.from_numpy(_labels(rng, 3, 3)).cuda(), out=out, **ok)
    # the C entry itself: the descriptor, the pointers, the two ranges
    L = v9.lib()
    aa, ser = (ctypes.c_int * 2)(1, 2), (ctypes.c_uint32 * 2)(1, 1)
    good = dict(width=W, height=H, fw=FW, fh=FH, channels=3, elem_size=2, layout=0, mode=0, flags=0, reserved=0, fill=0)
    item = 3 * FH * FW * 2

    def call(c=dev._c, a=aa, s=ser, i=None, n=2, m=2, d=good, sp=src.data_ptr(), dp=out.data_ptr()):
        dd = v9.PropDesc(**d) if d else None
        return L.vp9hip_acc_propagate(c, a, s, i, n, m, ctypes.byref(dd) if dd else None, sp, dp, None, None)
    bad = [dict(c=None), dict(a=None), dict(s=None), dict(n=0), dict(n=-1), dict(m=0), dict(m=1), dict(d=None), dict(sp=None), dict(dp=None),
           dict(d=dict(good, channels=0)), dict(d=dict(good, elem_size=3)), dict(d=dict(good, layout=-1)), dict(d=dict(good, mode=2)),
           dict(d=dict(good, mode=1, elem_size=4, channels=1)), dict(d=dict(good, mode=1, elem_size=1, channels=6)),
           dict(d=dict(good, flags=2)), dict(d=dict(good, flags=-1)), dict(d=dict(good, reserved=7)),
           dict(sp=src.data_ptr() + 1), dict(dp=out.data_ptr() + 1),
           dict(sp=out.data_ptr()), dict(sp=out.data_ptr() + item), dict(sp=out.data_ptr() + 2 * item - 2, m=1, i=(ctypes.c_int * 2)(0, 0))]
    for kw in bad:
        assert call(**kw) == v9.EINVAL, kw
    dev.upload(4, v9.alloc_planes(W, H, 8))              # an uploaded frame holds pixels and no field
    with pytest.raises(v9.Vp9HipError) as e:
        dev.acc_propagate([4], [1], src, out=out[:1], src_index=[0])
    assert e.value.code == v9.EAGAIN
    for other in (_device(v9, (W, H), 2, acc=False), v9.Device(0)):   # motion export alone; not configured
        try:
            if other.w:
                other.stage_batch(frames[:2], [0, 1], REFS[:2])
                other.run_batch()
                other.sync()
            with pytest.raises(v9.Vp9HipError) as e:
                other.acc_propagate([1, 1], [1, 1], src, size=(W, H), out=out)
            assert e.value.code == v9.EINVAL
        finally:
            other.close()
    torch.cuda.synchronize()
    assert bool((out == 0x5a5a).all())


def test_keep_out_streams_and_roots_that_are_gone(v9, chain3):
    dev, frames = chain3
    rng = np.random.default_rng(2)
    fields = [dev.download_motion_acc(i) for i in range(3)]
    accs, serials = [f[0] for f in fields], [f[1] for f in fields]
    pix = [v9.visible(dev.download(i), W, H) for i in range(3)]
    pairs = [(1, 0), (2, 0), (2, 1), (2, 2)]
    ba, roots, idx = [a for a, _ in pairs], [serials[b] for _, b in pairs], [b for _, b in pairs]
    items = _labels(rng, 3, 3)                           # values below 100
    src = torch.from_numpy(items).cuda()

    def check(got, valid, what, interp="nearest", fill=0, pre=None, its=items):
        g, vm = _np(got), _np(valid)
        for k, (a, b) in enumerate(pairs):
            want, wvalid = prop_ref(accs[a], serials[b], its[b], W, H, interp, fill, None if pre is None else pre[k])
            _same(g[k], want, "%s pair %s" % (what, (a, b)))
            assert np.array_equal(vm[k], wvalid), what
    # keep: the pre-filled elements stay exactly where nothing applies and change elsewhere
    pre = _labels(rng, 4, 3, 200, 300)                   # no value of the source
    out = torch.from_numpy(pre).cuda()
    got, valid = dev.acc_propagate(ba, roots, src, keep=True, valid=True, src_index=idx, out=out)
    torch.cuda.synchronize()
    assert got.data_ptr() == out.data_ptr()
    check(got, valid, "keep", pre=pre)
    g, vm = _np(got), _np(valid).astype(bool)
    assert 0 < vm[:3].mean() < 1 and not vm[3].any()
    assert (g == pre)[~np.broadcast_to(vm[:, None], g.shape)].all() and (g < 100)[np.broadcast_to(vm[:, None], g.shape)].all()
    # out= with fill: written in place, the fill converted to the dtype
    out2 = torch.full((4, 3, FH, FW), 0x5a5a, dtype=torch.int16, device="cuda")
    got, valid = dev.acc_propagate(ba, roots, src, fill=-7, valid=True, src_index=idx, out=out2)
    torch.cuda.synchronize()
    assert got.data_ptr() == out2.data_ptr()
    check(got, valid, "out=", fill=-7)
    assert not isinstance(dev.acc_propagate(ba, roots, src, src_index=idx), tuple)
    # one source item for every pair; 3-D tensors are C = 1 and come back 3-D
    one = torch.from_numpy(items[:1, 0].copy()).cuda()
    got = dev.acc_propagate([1, 2], [serials[0]] * 2, one)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (2, FH, FW)
    for k, a in enumerate((1, 2)):
        _same(_np(got)[k], prop_ref(accs[a], serials[0], items[0, :1], W, H)[0][0], "one item, 3-D")
    # a torch side stream as the current stream, and its handle; float16 bilinear, NHWC
    halves = rng.integers(-2000, 2000, (3, 19, FH, FW)).astype(np.float16)
    hsrc = torch.from_numpy(np.ascontiguousarray(halves.transpose(0, 2, 3, 1))).cuda()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got, valid = dev.acc_propagate(ba, roots, hsrc, interp="bilinear", layout="nhwc", valid=True, src_index=idx)
        side.synchronize()
    check(got.permute(0, 3, 1, 2).contiguous(), valid, "torch side stream", interp="bilinear", its=halves)
    got, valid = dev.acc_propagate(ba, roots, hsrc, layout="nhwc", fill=1.5, valid=True, src_index=idx, stream=side.cuda_stream)
    side.synchronize()
    check(got.permute(0, 3, 1, 2).contiguous(), valid, "stream handle", fill=1.5, its=halves)
    # the calls changed nothing they read
    assert np.array_equal(_np(src), items)
    for i in range(3):
        for p, (a, b) in enumerate(zip(pix[i], v9.visible(dev.download(i), W, H))):
            assert np.array_equal(a, b), "frame %d plane %d changed" % (i, p)
        cells, serial = dev.download_motion_acc(i)
        assert serial == serials[i] and cells.tobytes() == accs[i].tobytes()
    # a root whose buffer has been overwritten still applies: the point of passing serials
    before, vbefore = dev.acc_propagate([1, 2], [serials[0]] * 2, src, fill=-1, valid=True, src_index=[0, 0])
    torch.cuda.synchronize()
    assert int(vbefore.sum()) > 0
    later = v9.SynthFrame(v9.synth_params(W, H, 8, seed=7700))
    dev.stage_batch([later], [0])
    dev.run_batch()
    dev.sync()
    assert dev.download_motion_acc(0)[1] != serials[0]
    after, vafter = dev.acc_propagate([1, 2], [serials[0]] * 2, src, fill=-1, valid=True, src_index=[0, 0])
    torch.cuda.synchronize()
    assert torch.equal(after, before) and torch.equal(vafter, vbefore)
    # another frame decoded into a's buffer: the old serial applies nowhere
    dev.stage_batch([v9.SynthFrame(v9.synth_params(W, H, 8, seed=7701))], [2])
    dev.run_batch()
    dev.sync()
    got, valid = dev.acc_propagate([1, 2], [serials[0]] * 2, src, fill=-1, valid=True, src_index=[0, 0])
    torch.cuda.synchronize()
    assert torch.equal(got[0], before[0]) and int(valid[1].sum()) == 0 and bool((got[1] == -1).all())


# ------------------------------------------------------------------ the decoder's frames
@pytest.fixture(scope="module")
def decoded_prop():
    return {}


@pytest.mark.parametrize("max_batch", [1, 7])
def test_decoder(v9, stream_acc, decoded_prop, max_batch):  # noqa: F811
    """The key frame's labels carried to all 8 outputs of the stream with a hidden frame and a
    show_existing_frame, with the key frame released first; the fields of the reference come from
    a separate Stream parse."""
    pkts, want_acc, xi, hidden = stream_acc
    dec = v9.Decoder(0, export_motion_acc=True, max_batch=max_batch)
    try:
        infos = [info for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False)]
        assert len(infos) == len(want_acc) == 8
        accs, serials = [a for a, _ in want_acc], [s for _, s in want_acc]
        w, h = infos[0].width, infos[0].height
        key = dec.motion_acc(infos[0])[1]
        assert key == serials[0] == 1 and serials[xi] == hidden[1]
        assert xi > 0 and accs[xi].tobytes() != accs[xi - 1].tobytes()      # the shown-existing output has the hidden frame's field
        rng = np.random.default_rng(8)
        fw, fh = (w + 1) >> 1, (h + 1) >> 1
        labels = rng.integers(0, 2 ** 62, (1, fh, fw))                  # int64 class ids no float carries
        feats = rng.integers(-2000, 2000, (1, 5, fh, fw)).astype(np.float16)
        tl, tf = torch.from_numpy(labels).cuda(), torch.from_numpy(feats).cuda()
        dec.release(infos[0].buf)                        # the key frame's pixels are gone
        rest = infos[1:]
        got, valid = dec.acc_propagate(rest, [key] * 7, tl, fill=-1, valid=True)
        gf = dec.acc_propagate(rest, [key] * 7, tf, interp="bilinear")
        g, vm, gfn = _np(got), _np(valid), _np(gf)
        shares = []
        for k in range(7):
            want, wvalid = prop_ref(accs[k + 1], key, labels, w, h, "nearest", -1)
            _same(g[k], want[0], "decoder batch %d output %d labels" % (max_batch, k + 1))
            assert np.array_equal(vm[k], wvalid)
            _same(gfn[k], prop_ref(accs[k + 1], key, feats[0], w, h, "bilinear", 0)[0], "decoder batch %d output %d features" % (max_batch, k + 1))
            shares.append(float(wvalid.mean()))
        assert all(s > 0.25 for s in shares), shares
        # the key frame itself has no chain: nothing applies, and it is not held any more
        with pytest.raises(v9.Vp9HipError) as e:
            dec.acc_propagate([infos[0]], [key], tl)
        assert e.value.code == v9.EINVAL
        mixed = type(infos[1]).from_buffer_copy(infos[1])
        mixed.width -= 16
        with pytest.raises(v9.Vp9HipError) as e:
            dec.acc_propagate([infos[1], mixed], [key] * 2, tl)
        assert e.value.code == v9.EINVAL
        for i in rest:
            dec.release(i.buf)
    finally:
        dec.close()
    decoded_prop[max_batch] = (g, vm, gfn)
    if len(decoded_prop) == 2:                           # both batch sizes equal each other
        for a, b in zip(decoded_prop[1], decoded_prop[7]):
            assert np.array_equal(bits(a), bits(b))


def test_decoder_without_the_flag(v9, stream_acc):  # noqa: F811
    dec = v9.Decoder(0, export_motion=True, max_batch=4)
    try:
        infos = [info for _, info in dec.decode([(d, i) for i, d in enumerate(stream_acc[0][:2])], download=False)]
        src = torch.zeros((1, 4, 4), dtype=torch.uint8, device="cuda")
        with pytest.raises(v9.Vp9HipError) as e:
            dec.acc_propagate([infos[1]], [1], src)
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()
