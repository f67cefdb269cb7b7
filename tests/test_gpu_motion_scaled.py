"""Motion tensors at model size on the GPU (vp9hip_motion_frames_scaled /
vp9hip_decoder_motion_scaled, the kernel of csrc/vp9hip_motion_scale.hip) against the numpy
restatement of tests/test_motion_scaled_definition.py, which spreads the cells over pixels and
shares nothing with the kernel's sum over cells. Every comparison is exact, the halves by their
bit patterns.

A test gets its fields by decoding a small synthetic chain (gop_frames of
test_motion_acc_definition) with the export flags on. Where it needs chosen values it overwrites
the fields through the views of Device.motion / Device.motion_acc, after filling the whole
pitched planes with poison through raw views built from frame_motion's pointers: 0x7fff in every
int16 of the mv plane and every int32 of the acc plane (a far vector with hops > 0), 0x7f in
every byte of the info plane (an inter cell: 0x7fff there would read as intra and hide the
poisoned vector beside it).
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the tensors are torch's and share its HIP runtime (see _torch_first)
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_gpu_motion import _stream
from test_motion_acc_definition import gop_frames, gop_parents
from test_motion_scaled_definition import (CELL, FORMATS, SIZES, SOURCES, bits, cell_values, dense, grid, random_acc,
                                           random_coded, ref_tensor)
from test_residual_scaled_definition import sbox

pytestmark = pytest.mark.gpu

DTYPES = {"i16": "int16", "f16": "float16"}


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d differ, first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def _device(v9, w, h, nbufs=1, cfg=None, motion=True, acc=True, seed=7600):
    """A context of size cfg (default w x h) whose nbufs <= 3 buffers hold the fields of the first
    frames of a decoded w x h chain."""
    dev = v9.Device(0)
    if motion:
        dev.set_export(motion=True, motion_acc=acc)
    cw, ch = cfg or (w, h)
    dev.configure(cw, ch, 8, nbufs=nbufs)
    dev.set_timing(False)
    dev.frames = gop_frames(v9, w, h, nbufs, seed=seed)
    dev.stage_batch(dev.frames, list(range(nbufs)), [None] + [gop_parents(t) for t in range(1, nbufs)])
    dev.run_batch()
    dev.sync()
    dev.cfg, dev.size, dev.has_acc = (cw, ch), (w, h), motion and acc
    return dev


def _raw_planes(dev, buf):
    """Views of the whole pitched planes of buffer buf: mv int16, info uint8, acc int32 (or None)."""
    mv, info, _, pitch, _ = dev.frame_motion(buf)
    rows = 2 * ((dev.cfg[1] + 7) >> 3)
    assert pitch == 2 * ((dev.cfg[0] + 7) >> 3)

    def view(ptr, shape, typestr):
        class _View:
            __cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "version": 2}
        return torch.as_tensor(_View(), device="cuda")
    acc = view(dev.frame_motion_acc(buf)[0], (rows, pitch, 4), "<i4") if dev.has_acc else None
    return view(mv, (rows, pitch, 2, 2), "<i2"), view(info, (rows, pitch, 4), "|u1"), acc


def _set_field(dev, buf, mv=None, info=None, acc=None):
    """Poison the whole planes, then write the field through the library's own views."""
    rmv, rinfo, racc = _raw_planes(dev, buf)
    gw, gh = grid(*dev.size)
    if mv is not None:
        rmv.fill_(0x7fff)
        rinfo.fill_(0x7f)
        vmv, vinfo = dev.motion(buf)
        assert tuple(vmv.shape) == (gh, gw, 2, 2) == mv.shape and tuple(vinfo.shape) == (gh, gw, 4) == info.shape
        vmv.copy_(torch.from_numpy(mv))
        vinfo.copy_(torch.from_numpy(info))
    if acc is not None:
        racc.fill_(0x7fff)
        vacc = dev.motion_acc(buf)
        assert tuple(vacc.shape) == (gh, gw, 4) and acc.shape == (gh, gw)
        vacc.copy_(torch.from_numpy(acc.view("<i4").reshape(gh, gw, 4)))
    torch.cuda.synchronize()


def _tensor(dev, bufs, fmt, resize, source, mask, **kw):
    got = dev.motion_tensors(bufs, fmt, resize=resize, source=source, mask=mask, size=dev.size, **kw)
    ow, oh = resize if resize is not None else dev.size
    assert tuple(got.shape) == (len(bufs), 3 if mask else 2, oh, ow) and got.dtype == getattr(torch, DTYPES[fmt])
    return got


# ------------------------------------------------------------------ 1. random fields, every size, source, format and P
WRONG_GRID = {((65, 33), (33, 17)), ((66, 34), (33, 17)), ((130, 200), (224, 224))}


def test_sizes_sources_formats_planes(v9):
    """All of SIZES. Three of them have a visible size that is no multiple of 8, where taking the
    grid for the picture (n = 4 GW, 4 GH instead of w, h) gives another result: asserted on the
    reference alone before the kernel is compared."""
    rng = np.random.default_rng(7700)
    devs = {}
    try:
        for (w, h), (ow, oh) in SIZES:
            if (w, h) not in devs:
                devs[w, h] = _device(v9, w, h)
                mv, info = random_coded(rng, w, h)
                acc = random_acc(rng, w, h)
                _set_field(devs[w, h], 0, mv, info, acc)
                devs[w, h].src = dict(coded=dict(mv=mv, info=info), acc=dict(acc=acc))
            dev = devs[w, h]
            what = "%dx%d -> %dx%d" % (w, h, ow, oh)
            for source in SOURCES:
                src = dev.src[source]
                want = {fmt: ref_tensor(w, h, fmt, ow, oh, source, mask=True, **src) for fmt in FORMATS}
                if ((w, h), (ow, oh)) in WRONG_GRID:
                    gw, gh = grid(w, h)
                    wrong = ref_tensor(w, h, "i16", ow, oh, source, mask=True, n=(4 * gw, 4 * gh), **src)
                    cols = int((wrong != want["i16"]).any(axis=(0, 1)).sum())
                    print("%s %s: the grid taken for the picture differs in %d of %d columns" % (what, source, cols, ow))
                    assert cols > ow // 2
                for fmt in FORMATS:
                    for mask in (False, True):
                        got = _tensor(dev, [0], fmt, (ow, oh), source, mask)
                        _same(got[0], want[fmt][:3 if mask else 2], "%s %s %s mask %d" % (what, source, fmt, mask))
        for (w, h), dev in devs.items():               # resize=None: the dense field itself, through the same kernel
            for source in SOURCES:
                got = _tensor(dev, [0], "i16", None, source, True)
                want = np.stack([dense(c, w, h) for c in cell_values(source, **dev.src[source])]).astype(np.int16)
                _same(got[0], want, "%dx%d own size %s" % (w, h, source))
    finally:
        for dev in devs.values():
            dev.close()


# ------------------------------------------------------------------ 2. the division floors
def test_negative_sums_floor(v9):
    """8 x 8 -> 1 x 1: four cells of equal weight whose vectors sum to 4k + r. The mean rounds
    half up, floor((4k + r + 2) / 4) = k, k, k + 1, k + 1 for r = 0..3; a division that
    truncates toward zero gives k + 1 at r = 1 for a negative k."""
    dev = _device(v9, 8, 8)
    try:
        for k in (-8191, -5, -1, 0, 3):
            for r in range(4):
                ry = (r + 3) % 4
                mv, info = np.zeros((2, 2, 2, 2), np.int16), np.zeros((2, 2, 4), np.uint8)
                mv[:, :, 0, 0] = k
                mv[:, :, 0, 1] = -k
                mv.reshape(4, 2, 2)[:r, 0, 0] += 1
                mv.reshape(4, 2, 2)[:ry, 0, 1] += 1
                mv[:, :, 1] = 0x7fff
                acc = np.zeros((2, 2), CELL)
                acc["dx"], acc["dy"], acc["hops"] = mv[:, :, 0, 0], mv[:, :, 0, 1], 3
                assert int(acc["dx"].sum()) == 4 * k + r and int(acc["dy"].sum()) == -4 * k + ry
                _set_field(dev, 0, mv, info, acc)
                want = np.array([k + (r >= 2), -k + (ry >= 2), 256], np.int16).reshape(3, 1, 1)
                for source, src in (("coded", dict(mv=mv, info=info)), ("acc", dict(acc=acc))):
                    assert np.array_equal(ref_tensor(8, 8, "i16", 1, 1, source, mask=True, **src), want)
                    _same(_tensor(dev, [0], "i16", (1, 1), source, True)[0], want, "k %d r %d %s" % (k, r, source))
    finally:
        dev.close()


# ------------------------------------------------------------------ 3. what never enters a sum
def test_second_vector_and_stale_intra_bytes(v9):
    """Compound cells with a poisoned second vector, intra cells (info[0] == 255) with poisoned
    vectors under them, info[0] of 3..254 counting as inter, hops 0 over nonzero sums."""
    w, h = 16, 16
    dev = _device(v9, w, h)
    try:
        mv, info = np.zeros((4, 4, 2, 2), np.int16), np.zeros((4, 4, 4), np.uint8)
        mv[:, :, 0, 0] = np.arange(16).reshape(4, 4) * 100 - 700
        mv[:, :, 0, 1] = 300 - np.arange(16).reshape(4, 4) * 41
        mv[:, :, 1] = -0x8000
        info[..., 1] = 2
        info[0, :, 0] = (3, 100, 254, 255)
        info[2, 1:3, 0] = 255
        mv[2, 1:3, 0] = 0x7fff                          # stale bytes under the intra cells
        mv[0, 3, 0] = -0x8000
        acc = np.zeros((4, 4), CELL)
        acc["dx"], acc["dy"], acc["hops"] = mv[:, :, 0, 0], mv[:, :, 0, 1], 1
        acc["hops"][2, 1:3] = 0
        acc["hops"][0, 3] = 0
        acc["dx"][0, 3] = 0x7fffffff
        _set_field(dev, 0, mv, info, acc)
        for source, src in (("coded", dict(mv=mv, info=info)), ("acc", dict(acc=acc))):
            own = ref_tensor(w, h, "i16", 4, 4, source, mask=True, **src)
            assert own[2, 0].tolist() == [256, 256, 256, 0] and own[2, 2].tolist() == [256, 0, 0, 256]
            assert own[0, 0, 3] == 0 and (own[:2, 2, 1:3] == 0).all() and own[0, 0, 0] == -700
            for ow, oh in ((4, 4), (16, 16), (1, 1), (3, 5), (2, 2)):
                for fmt in FORMATS:
                    _same(_tensor(dev, [0], fmt, (ow, oh), source, True)[0],
                          ref_tensor(w, h, fmt, ow, oh, source, mask=True, **src), "%s %dx%d %s" % (source, ow, oh, fmt))
    finally:
        dev.close()


# ------------------------------------------------------------------ 4. the acc clamp comes before the sum
def test_acc_clamp_before_the_sum(v9):
    """One cell of INT32_MAX beside three of -30000, 8 x 8 -> 1 x 1: clamped first, the mean is
    (32767 - 90000) / 4; summed first and clamped afterwards it would be 32767."""
    dev = _device(v9, 8, 8)
    try:
        acc = np.zeros((2, 2), CELL)
        acc["hops"] = 2
        acc["dx"] = [[0x7fffffff, -30000], [-30000, -30000]]
        acc["dy"] = [[30000, 30000], [-0x80000000, 30000]]
        want = ref_tensor(8, 8, "i16", 1, 1, "acc", acc=acc, mask=True)
        late = [int(np.clip(sbox(dense(acc[f].astype(np.int64), 8, 8), 1, 1)[0, 0], -32768, 32767)) for f in ("dx", "dy")]
        assert late == [32767, -32768] and want[:2, 0, 0].tolist() == [-14308, 14308]
        _set_field(dev, 0, acc=acc)
        _same(_tensor(dev, [0], "i16", (1, 1), "acc", True)[0], want, "clamp")
        _same(_tensor(dev, [0], "f16", (1, 1), "acc", True)[0], ref_tensor(8, 8, "f16", 1, 1, "acc", acc=acc, mask=True), "clamp f16")
    finally:
        dev.close()


# ------------------------------------------------------------------ 5. a larger context: nothing beyond GW is read; streams
def test_larger_context_and_streams(v9):
    """66 x 34 fields (18 x 10 cells) in a 200 x 130 context (pitch 50): the cells beyond the
    grid are poison, in the rows of the grid and below them."""
    w, h, ow, oh = 66, 34, 33, 17
    rng = np.random.default_rng(5)
    dev = _device(v9, w, h, nbufs=2, cfg=(200, 130))
    try:
        fields = []
        for b in range(2):
            assert dev.frame_motion(b)[2:4] == ((18, 10), 50) and dev.frame_motion_acc(b)[1:3] == ((18, 10), 50)
            mv, info = random_coded(rng, w, h, lo=-2000, hi=2000)      # small beside the poison
            acc = random_acc(rng, w, h, lo=-2000, hi=2000)
            _set_field(dev, b, mv, info, acc)
            fields.append(dict(coded=dict(mv=mv, info=info), acc=dict(acc=acc)))
        rmv, rinfo, racc = _raw_planes(dev, 0)
        assert bool((rmv[:, 18:] == 0x7fff).all()) and bool((rinfo[10:] == 0x7f).all()) and bool((racc[:, 18:] == 0x7fff).all())
        for source in SOURCES:
            want = np.stack([ref_tensor(w, h, "f16", ow, oh, source, mask=True, **fields[b][source]) for b in (1, 0)])
            _same(_tensor(dev, [1, 0], "f16", (ow, oh), source, True), want, source + " null stream")
            for rs in ((7, 5), (224, 224), (1, 1), None):
                for b in (0, 1):
                    o = rs or (w, h)
                    _same(_tensor(dev, [b], "i16", rs, source, True)[0],
                          ref_tensor(w, h, "i16", o[0], o[1], source, mask=True, **fields[b][source]), "%s %s buf %d" % (source, rs, b))
            side = torch.cuda.Stream()
            with torch.cuda.stream(side):
                got = _tensor(dev, [1, 0], "f16", (ow, oh), source, True).cpu()
            _same(got, want, source + " torch side stream")
            got = _tensor(dev, [1, 0], "f16", (ow, oh), source, True, stream=side.cuda_stream)
            side.synchronize()
            _same(got, want, source + " stream handle")
    finally:
        dev.close()


# ------------------------------------------------------------------ 6. more frames than one launch takes, layout
def test_33_buffers_pitch_and_stride(v9):
    w, h, ow, oh = 65, 33, 33, 17
    rng = np.random.default_rng(33)
    dev = _device(v9, w, h, nbufs=3)
    try:
        fields = []
        for b in range(3):
            mv, info = random_coded(rng, w, h)
            acc = random_acc(rng, w, h)
            _set_field(dev, b, mv, info, acc)
            fields.append(dict(coded=dict(mv=mv, info=info), acc=dict(acc=acc)))
        order = [(7 * i + 1) % 3 for i in range(33)]
        pitch = 80
        for fmt, source, mask in (("i16", "coded", True), ("f16", "acc", False), ("f16", "coded", True)):
            P = 3 if mask else 2
            stride = P * pitch * oh + 48
            dt = getattr(torch, DTYPES[fmt])
            out = torch.full((33 * stride // 2,), 0x2bcd, dtype=torch.int16, device="cuda").view(dt)
            got = _tensor(dev, order, fmt, (ow, oh), source, mask, out=out, pitch=pitch, frame_stride=stride)
            assert got.stride() == (stride // 2, pitch * oh // 2, pitch // 2, 1) and got.data_ptr() == out.data_ptr()
            refs = [ref_tensor(w, h, fmt, ow, oh, source, mask=mask, **f[source]) for f in fields]
            want = np.full((33, stride // 2), 0x2bcd, np.int16)
            for i, b in enumerate(order):
                rows = want[i, :P * oh * pitch // 2].reshape(P * oh, pitch // 2)
                rows[:, :ow] = bits(refs[b]).reshape(P * oh, ow)
            torch.cuda.synchronize()
            raw = out.view(torch.int16).cpu().numpy().reshape(33, stride // 2)
            assert np.array_equal(raw, want), "%s %s: %d elements differ" % (fmt, source, int((raw != want).sum()))
    finally:
        dev.close()


# ------------------------------------------------------------------ 7. end to end
def test_decoded_fields(v9):
    """A decoded chain: the downloaded fields feed the host statement, motion_scaled_host."""
    w, h, n = 200, 130, 3
    dev = _device(v9, w, h, nbufs=n, seed=7800)
    try:
        fields = [dev.download_motion(b) + (dev.download_motion_acc(b)[0],) for b in range(n)]
        assert all((f[1][..., 0] != 255).any() and f[0].any() for f in fields[1:]) and (fields[2][2]["hops"] > 1).any()
        for rs in ((64, 48), (224, 224)):
            for source in SOURCES:
                for fmt in FORMATS:
                    got = _tensor(dev, list(range(n)), fmt, rs, source, True)
                    want = np.stack([v9.motion_scaled_host(mv, info, w, h, fmt, rs, source=source, acc=acc, mask=True)
                                     for mv, info, acc in fields])
                    _same(got, want, "%s %s %s" % (rs, source, fmt))
        mv, info, acc = fields[2]
        _same(_tensor(dev, [2], "i16", (64, 48), "coded", True)[0],
              ref_tensor(w, h, "i16", 64, 48, "coded", mv=mv, info=info, mask=True), "against the restatement")
    finally:
        dev.close()


def test_decoder_motion_tensors(v9):
    """A stream with a hidden frame and a show_existing_frame of it: the frames' own size, the
    shown buffer's fields, nothing released by the call, a released frame refused."""
    pkts = _stream(v9)
    ow, oh = 64, 48
    dec = v9.Decoder(0, export_motion_acc=True, max_batch=4)
    try:
        prev, n, seen = None, 0, []
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            mv, inf = dec.motion(info, download=True)
            field = (mv, inf, dec.motion_acc(info, download=True)[0])
            held = ([prev[0]] if prev else []) + [info]
            fields = ([prev[1]] if prev else []) + [field]
            for source in SOURCES:
                for fmt in (FORMATS if n in (0, 4, 5) else ["f16"]):
                    got = dec.motion_tensors(held, fmt, resize=(ow, oh), source=source, mask=True)
                    want = np.stack([v9.motion_scaled_host(m, i, info.width, info.height, fmt, (ow, oh), source=source, acc=a,
                                                           mask=True) for m, i, a in fields])
                    _same(got, want, "output %d %s %s" % (n, source, fmt))
            if n == 1:                                   # resize=None: the frames' visible size, two planes
                got = dec.motion_tensors([info], "i16")
                assert tuple(got.shape) == (1, 2, info.height, info.width)
                _same(got[0], ref_tensor(info.width, info.height, "i16", info.width, info.height, "coded", mv=mv, info=inf), "own size")
            if prev:
                dec.release(prev[0].buf)                 # the call released nothing: this still works
            prev = (info, field)
            seen.append(field)
            n += 1
        assert n == 8 and dec.eof
        # output 4 shows the hidden frame: a field no other output has, with inter cells
        assert (seen[4][1][..., 0] != 255).any() and all(seen[4][0].tobytes() != s[0].tobytes() for s in seen[:4] + seen[5:])
        other = type(info).from_buffer_copy(info)
        other.width -= 8
        with pytest.raises(v9.Vp9HipError) as e:
            dec.motion_tensors([info, other], "i16", resize=(ow, oh))
        assert e.value.code == v9.EINVAL
        dec.release(info.buf)
        with pytest.raises(v9.Vp9HipError) as e:         # a released frame is not the caller's
            dec.motion_tensors([info], "i16", resize=(ow, oh))
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()
    for kw, refused in ((dict(), ("coded", "acc")), (dict(export_motion=True), ("acc",)), (dict(export_residual=True), ("coded", "acc"))):
        dec = v9.Decoder(0, max_batch=4, **kw)           # without the flag the source needs
        try:
            for _, info in dec.decode([(pkts[0], 0)], download=False):
                for source in refused:
                    with pytest.raises(v9.Vp9HipError) as e:
                        dec.motion_tensors([info], "i16", resize=(ow, oh), source=source)
                    assert e.value.code == v9.EINVAL
                if "coded" not in refused:
                    assert tuple(dec.motion_tensors([info], "i16", resize=(ow, oh)).shape) == (1, 2, oh, ow)
                dec.release(info.buf)
        finally:
            dec.close()


# ------------------------------------------------------------------ 8. errors: refused before anything is written
def test_errors_write_nothing(v9):
    w, h, ow, oh = 66, 34, 20, 12
    dev = _device(v9, w, h, nbufs=3, cfg=(200, 130))
    noacc = _device(v9, w, h, acc=False)
    plain = _device(v9, w, h, motion=False)
    fresh = v9.Device(0)                                # not configured
    try:
        other = v9.SynthFrame(v9.synth_params(80, 48, 8, seed=0x17b00))
        dev.submit(other, 2)                            # a field of another grid
        dev.sync()
        assert dev.frame_motion(2)[2] == (20, 12) and dev.frame_motion(0)[2] == (18, 10)
        out = torch.full((4 * 3 * 64 * 48,), 0x2bcd, dtype=torch.int16, device="cuda")
        ok = dict(bufs=[0, 1], fmt="i16", resize=(ow, oh), source="acc", mask=True, size=(w, h))
        assert tuple(dev.motion_tensors(out=torch.empty_like(out), **ok).shape) == (2, 3, oh, ow)
        # 72 x 40 has the grid of 66 x 34: the size is the caller's statement, taken as it is
        assert tuple(dev.motion_tensors(out=torch.empty_like(out), **dict(ok, size=(72, 40))).shape) == (2, 3, oh, ow)
        cases = [dict(bufs=[0, 3]), dict(bufs=[-1]), dict(bufs=[]), dict(bufs=[0, 2]), dict(bufs=[2, 0]), dict(bufs=[2]),
                 dict(size=(0, h)), dict(size=(w, 0)), dict(size=(16385, h)), dict(size=(w, 16385)), dict(size=(74, h)),
                 dict(size=(w, 42)), dict(size=(58, h)), dict(size=(200, 130)), dict(size=None),
                 dict(resize=(0, oh)), dict(resize=(ow, 0)), dict(resize=(16385, oh)), dict(resize=(ow, 16385)),
                 dict(pitch=2 * ow - 2), dict(pitch=2 * ow + 2), dict(pitch=-16), dict(frame_stride=3 * 2 * ow * oh - 2),
                 dict(frame_stride=3 * 2 * ow * oh + 1), dict(frame_stride=-2)]
        for kw in cases:
            for source in SOURCES:
                with pytest.raises(v9.Vp9HipError) as e:
                    dev.motion_tensors(out=out, **dict(ok, source=source, **kw))
                assert e.value.code == v9.EINVAL, (kw, source)
        for rs in ((ow, oh), None):
            for d2 in (plain, fresh):                   # no motion flag, with and without buffers
                for source in SOURCES:
                    with pytest.raises(v9.Vp9HipError) as e:
                        d2.motion_tensors([0], "i16", resize=rs, source=source, size=(w, h), out=out)
                    assert e.value.code == v9.EINVAL
            with pytest.raises(v9.Vp9HipError) as e:    # the accumulated source without its flag
                noacc.motion_tensors([0], "i16", resize=rs, source="acc", out=out)
            assert e.value.code == v9.EINVAL
        L = v9.lib()
        two = (ctypes.c_int * 2)(0, 1)

        def raw(bufs=two, n=2, fmt=0, source=1, planes=3, dst=out.data_ptr(), desc=True, ctx=dev._c):
            de = v9.MvtDesc(fmt, source, planes, w, h, ow, oh, 0, 0)
            return L.vp9hip_motion_frames_scaled(ctx, bufs, n, ctypes.byref(de) if desc else None, dst, None)
        assert raw(n=0) == v9.EINVAL and raw(n=-1) == v9.EINVAL
        assert raw(fmt=2) == v9.EINVAL and raw(fmt=-1) == v9.EINVAL and raw(source=2) == v9.EINVAL and raw(source=-1) == v9.EINVAL
        assert raw(planes=1) == v9.EINVAL and raw(planes=4) == v9.EINVAL
        assert raw(dst=None) == v9.EINVAL and raw(dst=out.data_ptr() + 1) == v9.EINVAL
        assert raw(bufs=None) == v9.EINVAL and raw(desc=False) == v9.EINVAL and raw(ctx=None) == v9.EINVAL
        dev.upload(1, v9.alloc_planes(200, 130, 8))     # written by another path: the field is gone
        for bufs in ([0, 1], [1, 0], [1]):
            for source in SOURCES:
                with pytest.raises(v9.Vp9HipError) as e:
                    dev.motion_tensors(bufs, "i16", resize=(ow, oh), source=source, size=(w, h), out=out)
                assert e.value.code == v9.EAGAIN
        torch.cuda.synchronize()
        assert bool((out == 0x2bcd).all())
        assert raw(n=1) == 0                            # and the same call with a good argument is taken
        torch.cuda.synchronize()
        assert not bool((out[:3 * ow * oh] == 0x2bcd).all()) and bool((out[3 * ow * oh:] == 0x2bcd).all())
    finally:
        for d2 in (dev, noacc, plain, fresh):
            d2.close()


# ------------------------------------------------------------------ 9. nothing else changes
def test_pixels_fields_and_decode_unchanged(v9):
    frames = gop_frames(v9, 200, 130, 3, seed=7900)
    refs = [None] + [gop_parents(t) for t in (1, 2)]

    def state(dev, b):
        mv, info = dev.download_motion(b)
        acc, serial = dev.download_motion_acc(b)
        return [a.tobytes() for a in dev.download(b)] + [mv.tobytes(), info.tobytes(), acc.tobytes(), serial]

    def decode(call):
        dev = v9.Device(0)
        try:
            dev.set_export(motion=True, motion_acc=True)
            dev.configure(200, 130, 8, nbufs=3)
            dev.set_timing(False)
            dev.stage_batch(frames[:2], [0, 1], refs[:2])
            dev.run_batch()
            dev.sync()
            before = [state(dev, b) for b in (0, 1)]
            if call:
                for source in SOURCES:
                    for fmt in FORMATS:
                        dev.motion_tensors([1, 0, 1], fmt, resize=(64, 48), source=source, mask=True)
                torch.cuda.synchronize()
                assert [state(dev, b) for b in (0, 1)] == before, "pixels or fields changed by the call"
            dev.stage_batch(frames[2:], [2], refs[2:])
            dev.run_batch()
            dev.sync()
            return before + [state(dev, 2)]
        finally:
            dev.close()
    assert decode(True) == decode(False)
