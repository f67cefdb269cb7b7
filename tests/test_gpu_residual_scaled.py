"""Residual tensors at model size on the GPU (vp9hip_residual_frames_scaled /
vp9hip_decoder_residual_scaled, the kernel of csrc/vp9hip_residual_scale.hip) against the numpy
restatement of tests/test_residual_scaled_definition.py. Every comparison is exact, the halves by
their bit patterns.

A test gets a field by decoding one synthetic keyframe of the wanted size with the residual flag
on and overwriting the field through Device.residual's views; the samples outside the visible
size are reached through a raw view of the padded plane built from frame_residual's pointers and
pitches.
"""
import ctypes

import numpy as np
import pytest

try:     # torch first: the tensors are torch's and share its HIP runtime (see _torch_first)
    import torch
except Exception:   # pragma: no cover
    torch = None

from test_gpu_convert_scale import RATIOS
from test_gpu_motion import _stream
from test_residual_definition import reference as decoded_reference
from test_residual_scaled_definition import (FORMATS, MATRICES, SUBSAMPLINGS, bits, clip_cases, random_field, ref_tensor,
                                             resampled)

pytestmark = pytest.mark.gpu

POISON = 0x7fff
DTYPES = {"yuv_i16": "int16", "yuv_f16": "float16", "rgb_i16": "int16", "rgb_f16": "float16"}


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = bits(got) != bits(want)
    assert not bad.any(), "%s: %d of %d differ, first at %s" % (what, int(bad.sum()), bad.size, tuple(np.argwhere(bad)[0]))


def _device(v9, w, h, d=8, ssh=1, ssv=1, nbufs=1, cfg=None, residual=True):
    """A context of size cfg (default w x h) whose nbufs buffers each hold the field of one
    decoded w x h keyframe."""
    dev = v9.Device(0)
    if residual:
        dev.set_export(motion=False, residual=True)
    cw, ch = cfg or (w, h)
    dev.configure(cw, ch, d, nbufs=nbufs, ss_h=ssh, ss_v=ssv)
    dev.set_timing(False)
    key = v9.SynthFrame(v9.synth_params(w, h, d, seed=0x15a00 + w, ss_h=ssh, ss_v=ssv))
    for b in range(nbufs):
        dev.submit(key, b)
    dev.sync()
    dev.cfg = (cw, ch)
    return dev


def _raw_planes(dev, buf):
    """int16 views of the whole padded planes of buffer buf's field."""
    ptrs, pitch, _, _ = dev.frame_residual(buf)
    rows = (dev.cfg[1] + 63) // 64 * 64
    out = []
    for p in range(3):
        class _View:
            __cuda_array_interface__ = {"shape": (rows >> (dev.ss_v if p else 0), pitch[p]), "typestr": "<i2",
                                        "data": (ptrs[p], False), "version": 2}
        out.append(torch.as_tensor(_View(), device="cuda"))
    return out


def _set_field(dev, buf, planes, poison=True):
    """Fill the padded planes with POISON, then write the visible part through Device.residual."""
    if poison:
        for raw in _raw_planes(dev, buf):
            raw.fill_(POISON)
    for view, a in zip(dev.residual(buf), planes):
        assert tuple(view.shape) == a.shape
        view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ 1. random fields
@pytest.mark.parametrize("ss", SUBSAMPLINGS)
@pytest.mark.parametrize("d", [8, 10, 12])
def test_formats_match_the_reference(v9, d, ss):
    ssh, ssv = ss
    rng = np.random.default_rng(7000 + 100 * d + 10 * ssh + ssv)
    devs = {}
    try:
        for (w, h), (ow, oh) in RATIOS:
            if (w, h) not in devs:
                devs[w, h] = _device(v9, w, h, d, ssh, ssv)
            dev = devs[w, h]
            planes = random_field(rng, w, h, d, ssh, ssv)
            _set_field(dev, 0, planes)
            pre = resampled(planes, w, h, ssh, ssv, ow, oh)
            what = "%dx%d -> %dx%d" % (w, h, ow, oh)
            for fmt in FORMATS:
                mats = MATRICES if fmt.startswith("rgb") and (w, h, ow, oh) == (65, 33, 33, 17) else [(2, 0)]
                for cs, full in mats:
                    got = dev.residual_tensors([0], fmt, resize=(ow, oh), colorspace=cs, full_range=full)
                    assert tuple(got.shape) == (1, 3, oh, ow) and got.dtype == getattr(torch, DTYPES[fmt])
                    _same(got[0], ref_tensor(planes, w, h, ssh, ssv, d, fmt, ow, oh, cs, full, pre),
                          "%s cs %d full %d %s" % (fmt, cs, full, what))
            if (ow, oh) == (33, 17):               # resize=None: the field's own size, the identity
                got = dev.residual_tensors([0], "yuv_i16")
                assert tuple(got.shape) == (1, 3, h, w)
                _same(got[0], ref_tensor(planes, w, h, ssh, ssv, d, "yuv_i16", w, h), "own size " + what)
    finally:
        for dev in devs.values():
            dev.close()


# ------------------------------------------------------------------ 2. rounding at negative halves
def test_negative_halves_round_up(v9):
    """2:1 of 2x2 blocks whose sums are 4k, 4k+1, 4k+2 and 4k+3, k negative and positive: k, k,
    k+1, k+1. A division that truncates toward zero gives k+1 for the first two of a negative k."""
    w = h = 16
    dev = _device(v9, w, h, 8, 0, 0)
    try:
        k = (np.arange(64).reshape(8, 8) * 7) % 97 - 50
        rem = (np.arange(64).reshape(8, 8) + np.arange(8)[:, None]) % 4
        assert (k < -1).any() and (k > 0).any()
        planes, wants = [], []
        for p in range(3):
            r = (rem + p) % 4
            P = np.repeat(np.repeat(k, 2, axis=0), 2, axis=1)
            P[0::2, 1::2] += r >= 1                # the block's sum is 4k + r
            P[1::2, 0::2] += r >= 2
            P[1::2, 1::2] += r >= 3
            planes.append(P.astype(np.int16))
            wants.append(k + (r >= 2))
        _set_field(dev, 0, planes)
        want = np.stack(wants).astype(np.int16)
        assert np.array_equal(ref_tensor(planes, w, h, 0, 0, 8, "yuv_i16", 8, 8), want)
        _same(dev.residual_tensors([0], "yuv_i16", resize=(8, 8))[0], want, "negative halves")
    finally:
        dev.close()


# ------------------------------------------------------------------ 3. extremes
def test_extremes_and_clips(v9):
    w, h, d, ow, oh = 65, 33, 12, 7, 5
    m = (1 << d) - 1
    dev = _device(v9, w, h, d)
    try:
        for name, planes in clip_cases(w, h, 1, 1, d).items():
            _set_field(dev, 0, planes)
            for fmt in FORMATS:
                got = dev.residual_tensors([0], fmt, resize=(ow, oh))
                _same(got[0], ref_tensor(planes, w, h, 1, 1, d, fmt, ow, oh), "%s %s" % (name, fmt))
                if fmt == "yuv_i16" and name in ("max", "min"):
                    assert bool((got == (32767 if name == "max" else -32768)).all())
                if fmt == "rgb_i16" and name in ("max", "min"):
                    assert bool((got == (m if name == "max" else -m)).all())
    finally:
        dev.close()


# ------------------------------------------------------------------ 4. more frames than one launch takes, layout
def test_33_buffers_pitch_and_stride(v9):
    w, h, ow, oh, d = 65, 33, 33, 17, 10
    rng = np.random.default_rng(33)
    dev = _device(v9, w, h, d, nbufs=3)
    try:
        fields = [random_field(rng, w, h, d, 1, 1) for _ in range(3)]
        for b in range(3):
            _set_field(dev, b, fields[b])
        order = [(7 * i + 1) % 3 for i in range(33)]
        pitch, stride = 80, 3 * 80 * oh + 48
        for fmt in ("rgb_i16", "yuv_f16"):
            dt = getattr(torch, DTYPES[fmt])
            out = torch.full((33 * stride // 2,), 0x2bcd, dtype=torch.int16, device="cuda").view(dt)
            got = dev.residual_tensors(order, fmt, resize=(ow, oh), out=out, pitch=pitch, frame_stride=stride)
            assert tuple(got.shape) == (33, 3, oh, ow) and got.stride() == (stride // 2, pitch * oh // 2, pitch // 2, 1)
            refs = [ref_tensor(f, w, h, 1, 1, d, fmt, ow, oh) for f in fields]
            want = np.full((33, stride // 2), 0x2bcd, np.int16)
            for i, b in enumerate(order):
                rows = want[i, :3 * oh * pitch // 2].reshape(3 * oh, pitch // 2)
                rows[:, :ow] = bits(refs[b]).reshape(3 * oh, ow)
            torch.cuda.synchronize()
            raw = out.view(torch.int16).cpu().numpy().reshape(33, stride // 2)
            assert np.array_equal(raw, want), "%s: %d elements differ" % (fmt, int((raw != want).sum()))
    finally:
        dev.close()


# ------------------------------------------------------------------ 5. a larger context, streams
def test_larger_context_and_streams(v9):
    w, h, d, ow, oh = 66, 34, 8, 20, 12
    rng = np.random.default_rng(5)
    dev = _device(v9, w, h, d, nbufs=2, cfg=(200, 130))
    try:
        fields = [random_field(rng, w, h, d, 1, 1) for _ in range(2)]
        for b in range(2):
            assert dev.frame_residual(b)[2] == (w, h)
            _set_field(dev, b, fields[b])
        want = np.stack([ref_tensor(fields[b], w, h, 1, 1, d, "rgb_f16", ow, oh) for b in (1, 0)])
        _same(dev.residual_tensors([1, 0], "rgb_f16", resize=(ow, oh)), want, "null stream")
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = dev.residual_tensors([1, 0], "rgb_f16", resize=(ow, oh)).cpu()
        _same(got, want, "torch side stream")
        got = dev.residual_tensors([1, 0], "rgb_f16", resize=(ow, oh), stream=side.cuda_stream)
        side.synchronize()
        _same(got, want, "stream handle")
    finally:
        dev.close()


# ------------------------------------------------------------------ 6. end to end
def test_decoded_fields(v9, orc):
    """The three frames of the residual definition's 200x130 case: download_residual feeds the
    restatement."""
    frames, _, _ = decoded_reference(orc, v9, "200x130")
    w, h, ow, oh = 200, 130, 64, 48
    dev = v9.Device(0)
    try:
        dev.set_export(motion=False, residual=True)
        dev.configure(w, h, 8, nbufs=3)
        dev.set_timing(False)
        dev.stage_batch(frames, [0, 1, 2], [None, (0, 0, 0), (1, 0, 1)])
        dev.run_batch()
        dev.sync()
        fields = [dev.download_residual(b) for b in range(3)]
        assert all(any(a.any() for a in f) for f in fields)
        for fmt in FORMATS:
            got = dev.residual_tensors([0, 1, 2], fmt, resize=(ow, oh))
            _same(got, np.stack([ref_tensor(f, w, h, 1, 1, 8, fmt, ow, oh) for f in fields]), fmt)
    finally:
        dev.close()


def test_decoder_residual_tensors(v9):
    """A stream with a hidden frame and a show_existing_frame of it: the frames' own colour
    space, nothing released by the call, a released frame refused."""
    pkts = _stream(v9)
    ow, oh = 64, 48
    dec = v9.Decoder(0, export_residual=True, max_batch=4)
    try:
        prev, n = None, 0
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            cs = 2 if info.colorspace in (0, 6) else info.colorspace
            held = ([prev[0]] if prev else []) + [info]
            fields = ([prev[1]] if prev else []) + [dec.residual(info, download=True)]
            fmts = FORMATS if n in (0, 5) else ["rgb_f16"]
            for fmt in fmts:
                got = dec.residual_tensors(held, fmt, resize=(ow, oh))
                want = np.stack([ref_tensor(f, info.width, info.height, info.ss_h, info.ss_v, info.bpp, fmt, ow, oh, cs,
                                            info.full_range) for f in fields])
                _same(got, want, "output %d %s" % (n, fmt))
            if prev:
                dec.release(prev[0].buf)           # the call released nothing: this still works
            prev = (info, fields[-1])
            n += 1
        assert n == 8 and dec.eof
        other = type(info).from_buffer_copy(info)
        other.width -= 8
        with pytest.raises(v9.Vp9HipError) as e:
            dec.residual_tensors([info, other], "yuv_i16", resize=(ow, oh))
        assert e.value.code == v9.EINVAL
        dec.release(info.buf)
        with pytest.raises(v9.Vp9HipError) as e:    # a released frame is not the caller's
            dec.residual_tensors([info], "yuv_i16", resize=(ow, oh))
        assert e.value.code == v9.EINVAL
    finally:
        dec.close()
    dec = v9.Decoder(0, max_batch=4)               # without the flag
    try:
        for _, info in dec.decode([(pkts[0], 0)], download=False):
            with pytest.raises(v9.Vp9HipError) as e:
                dec.residual_tensors([info], "yuv_i16", resize=(ow, oh))
            assert e.value.code == v9.EINVAL
            dec.release(info.buf)
    finally:
        dec.close()


# ------------------------------------------------------------------ 7. errors: refused before anything is written
def test_errors_write_nothing(v9):
    w, h, ow, oh = 66, 34, 20, 12
    dev = _device(v9, w, h, 8, nbufs=3, cfg=(200, 130))
    plain = _device(v9, w, h, 8, nbufs=1, residual=False)
    fresh = v9.Device(0)                            # not configured
    try:
        other = v9.SynthFrame(v9.synth_params(72, 40, 8, seed=0x15b00))
        dev.submit(other, 2)                        # a field of another visible size
        dev.sync()
        assert dev.frame_residual(2)[2] == (72, 40)
        out = torch.full((4 * 3 * 64 * 48,), 0x2bcd, dtype=torch.int16, device="cuda")
        ok = dict(bufs=[0, 1], fmt="rgb_i16", resize=(ow, oh))
        assert tuple(dev.residual_tensors(out=torch.empty_like(out), **ok).shape) == (2, 3, oh, ow)
        cases = [dict(bufs=[0, 3]), dict(bufs=[-1]), dict(bufs=[]), dict(bufs=[0, 2]), dict(bufs=[2, 0]), dict(colorspace=0),
                 dict(colorspace=6), dict(colorspace=8), dict(colorspace=-1), dict(fmt="rgb_f16", colorspace=0),
                 dict(resize=(0, oh)), dict(resize=(ow, 0)), dict(resize=(16385, oh)), dict(resize=(ow, 16385)),
                 dict(pitch=2 * ow - 2), dict(pitch=2 * ow + 2), dict(pitch=-16), dict(frame_stride=3 * 2 * ow * oh - 2),
                 dict(frame_stride=3 * 2 * ow * oh + 1), dict(frame_stride=-2)]
        for kw in cases:
            with pytest.raises(v9.Vp9HipError) as e:
                dev.residual_tensors(out=out.view(torch.float16) if kw.get("fmt", "").endswith("f16") else out, **dict(ok, **kw))
            assert e.value.code == v9.EINVAL, kw
        for d2 in (plain, fresh):                   # no residual flag, with and without buffers
            for rs in ((ow, oh), None):
                with pytest.raises(v9.Vp9HipError) as e:
                    d2.residual_tensors([0], "yuv_i16", resize=rs, out=out)
                assert e.value.code == v9.EINVAL
        L = v9.lib()
        two = (ctypes.c_int * 2)(0, 1)

        def raw(bufs=two, n=2, fmt=2, dst=out.data_ptr(), desc=True, ctx=dev._c):
            de = v9.ResidDesc(fmt, 2, 0, ow, oh, 0, 0)
            return L.vp9hip_residual_frames_scaled(ctx, bufs, n, ctypes.byref(de) if desc else None, dst, None)
        assert raw(n=0) == v9.EINVAL and raw(n=-1) == v9.EINVAL
        assert raw(fmt=4) == v9.EINVAL and raw(fmt=-1) == v9.EINVAL
        assert raw(dst=None) == v9.EINVAL and raw(dst=out.data_ptr() + 1) == v9.EINVAL
        assert raw(bufs=None) == v9.EINVAL and raw(desc=False) == v9.EINVAL and raw(ctx=None) == v9.EINVAL
        dev.upload(1, v9.alloc_planes(200, 130, 8))                 # written by another path: the field is gone
        for bufs in ([0, 1], [1, 0], [1]):
            with pytest.raises(v9.Vp9HipError) as e:
                dev.residual_tensors(bufs, "rgb_i16", resize=(ow, oh), out=out)
            assert e.value.code == v9.EAGAIN
        torch.cuda.synchronize()
        assert bool((out == 0x2bcd).all())
        assert raw(n=1) == 0                        # and the same call with a good argument is taken
        torch.cuda.synchronize()
        assert not bool((out[:3 * ow * oh] == 0x2bcd).all())
    finally:
        for d2 in (dev, plain, fresh):
            d2.close()


# ------------------------------------------------------------------ 8. nothing else changes
def test_pixels_fields_and_decode_unchanged(v9, orc):
    frames, _, _ = decoded_reference(orc, v9, "200x130")

    def decode(call):
        dev = v9.Device(0)
        try:
            dev.set_export(motion=False, residual=True)
            dev.configure(200, 130, 8, nbufs=3)
            dev.set_timing(False)
            dev.stage_batch(frames[:2], [0, 1], [None, (0, 0, 0)])
            dev.run_batch()
            dev.sync()
            before = [[a.tobytes() for a in dev.download(b) + dev.download_residual(b)] for b in (0, 1)]
            if call:
                for fmt in FORMATS:
                    dev.residual_tensors([1, 0, 1], fmt, resize=(64, 48))
                torch.cuda.synchronize()
                after = [[a.tobytes() for a in dev.download(b) + dev.download_residual(b)] for b in (0, 1)]
                assert after == before, "pixels or fields changed by the call"
            dev.stage_batch(frames[2:], [2], [(1, 0, 1)])
            dev.run_batch()
            dev.sync()
            return before + [[a.tobytes() for a in dev.download(2) + dev.download_residual(2)]]
        finally:
            dev.close()
    assert decode(True) == decode(False)
