"""Motion export on the GPU: k_motion's tensors against the numpy restatement of the definition
(tests/test_motion_definition.py, which shares no code with the library). Exact equality.

Batch path over sizes / formats / tile columns / a larger context, torch views, pixels
untouched, the error codes, slot rotation, and the bitstream decoder with a hidden frame and a
show_existing_frame. No test feeds the kernel an invalid packet: its clipping is the host
statement's, checked by tests/c/motion_host_check.c under the sanitizer builds.
"""
try:     # torch first: Device.motion returns torch views that share the HIP runtime (see _torch_first)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

import numpy as np
import pytest

from test_motion_definition import motion_field
from test_stream import _frames

pytestmark = pytest.mark.gpu


def _batch(v9, w, h, bpp=8, seed=5100, **kw):
    """key + P + compound P; refs of the P frames: the frame before (LAST, ALTREF), the key (GOLDEN)."""
    key = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, **kw))
    p = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 1, inter=1, p_intra=0.3, **kw))
    c = v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 2, inter=1, compound=1, **kw))
    return [key, p, c], [None, (0, 0, 0), (1, 0, 1)]


def _want(frames):
    out = []
    for f in frames:
        mv, info, hits = motion_field(f.blocks(), f.pkt.width, f.pkt.height)
        assert hits.min() == 1 and hits.max() == 1
        out.append((mv, info))
    return out


def _run(v9, frames, refs, cfg, export=True, bufs=None, **fmt):
    dev = v9.Device(0)
    if export:
        dev.set_export(motion=True)
    dev.configure(cfg[0], cfg[1], frames[0].pkt.bpp, nbufs=len(frames), **fmt)
    dev.set_timing(False)
    dev.stage_batch(frames, bufs or list(range(len(frames))), refs)
    dev.run_batch()
    dev.sync()
    return dev


def _same(got, want, what):
    (gmv, ginfo), (wmv, winfo) = got, want
    assert gmv.shape == wmv.shape and gmv.dtype == np.int16, what
    assert ginfo.shape == winfo.shape and ginfo.dtype == np.uint8, what
    assert np.array_equal(ginfo, winfo), "%s: info differs in %d cells" % (what, int((ginfo != winfo).any(-1).sum()))
    assert np.array_equal(gmv, wmv), "%s: mv differs in %d cells" % (what, int((gmv != wmv).any((-1, -2)).sum()))


CASES = {
    "8x8": dict(w=8, h=8),
    "66x66": dict(w=66, h=66),
    "200x130": dict(w=200, h=130),
    "66x66-10bit": dict(w=66, h=66, bpp=10),
    "66x34-444": dict(w=66, h=34, synth=dict(ss_h=0, ss_v=0)),
    "528x72-2tiles": dict(w=528, h=72, synth=dict(log2_tile_cols=1)),
    "66x66-in-200x130": dict(w=66, h=66, cfg=(200, 130)),
}


@pytest.mark.parametrize("name", list(CASES))
def test_batch_fields(v9, name):
    c = CASES[name]
    w, h, synth = c["w"], c["h"], c.get("synth", {})
    frames, refs = _batch(v9, w, h, c.get("bpp", 8), **synth)
    fmt = {k: synth[k] for k in ("ss_h", "ss_v") if k in synth}
    dev = _run(v9, frames, refs, c.get("cfg", (w, h)), **fmt)
    try:
        for i, want in enumerate(_want(frames)):
            _same(dev.download_motion(i), want, "%s frame %d" % (name, i))
    finally:
        dev.close()


def test_torch_views(v9):
    """Device.motion: zero-copy views strided over the fixed pitch of a larger context."""
    frames, refs = _batch(v9, 66, 34, seed=5200)
    dev = _run(v9, frames, refs, (200, 130))
    try:
        for i, want in enumerate(_want(frames)):
            mv, info = dev.motion(i, device="cuda:0")
            assert tuple(mv.shape) == (10, 18, 2, 2) and mv.dtype == torch.int16 and mv.stride() == (2 * 25 * 4, 4, 2, 1)
            assert tuple(info.shape) == (10, 18, 4) and info.dtype == torch.uint8 and info.stride() == (2 * 25 * 4, 4, 1)
            _same((mv.cpu().numpy(), info.cpu().numpy()), want, "views frame %d" % i)
    finally:
        dev.close()


def test_pixels_untouched_and_error_codes(v9):
    frames, refs = _batch(v9, 200, 130, seed=5300)
    off = _run(v9, frames, refs, (200, 130), export=False)
    on = _run(v9, frames, refs, (200, 130))
    try:
        for i in range(3):
            for p, (a, b) in enumerate(zip(off.download(i), on.download(i))):
                assert a.tobytes() == b.tobytes(), "frame %d plane %d changed with export on" % (i, p)
        for call in (off.motion, off.download_motion):
            with pytest.raises(v9.Vp9HipError) as e:
                call(0)
            assert e.value.code == v9.EINVAL
        with pytest.raises(v9.Vp9HipError) as e:
            on.set_export(motion=False)            # configured: the flags are fixed
        assert e.value.code == v9.EINVAL
        on.set_export(motion=True)                 # no change: accepted
        with pytest.raises(v9.Vp9HipError) as e:
            on.download_motion(3)                  # no such buffer
        assert e.value.code == v9.EINVAL
    finally:
        off.close()
        on.close()
    dev = v9.Device(0)
    try:
        dev.set_export(motion=True)
        dev.configure(200, 130, 8, nbufs=2)
        for call in (dev.motion, dev.download_motion):
            with pytest.raises(v9.Vp9HipError) as e:
                call(1)                            # never written
            assert e.value.code == v9.EAGAIN
        key = v9.SynthFrame(v9.synth_params(200, 130, 8, seed=5310))
        dev.submit(key, 1)
        dev.sync()
        _same(dev.download_motion(1), _want([key])[0], "submit")
        dev.fill(1, 1, 0)                          # written by another path: the field is gone
        dev.sync()
        with pytest.raises(v9.Vp9HipError) as e:
            dev.download_motion(1)
        assert e.value.code == v9.EAGAIN
    finally:
        dev.close()


def test_slots_keep_earlier_fields(v9):
    """Five batches of two frames over the three pipeline slots into ten buffers: a later batch in
    a slot (its arena reused) leaves the earlier batches' fields alone."""
    w, h = 136, 72
    dev = v9.Device(0)
    dev.set_export(motion=True)
    dev.configure(w, h, 8, nbufs=10)
    dev.set_timing(False)
    frames = []
    try:
        for k in range(5):
            pair = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=5400 + 2 * k)),
                    v9.SynthFrame(v9.synth_params(w, h, 8, seed=5401 + 2 * k, inter=1, compound=k & 1))]
            frames += pair
            dev.set_slot(k % 3)
            dev.stage_batch(pair, [2 * k, 2 * k + 1], [None, (2 * k,) * 3])
            dev.run_batch()
        dev.sync()
        for i, want in enumerate(_want(frames)):
            _same(dev.download_motion(i), want, "buffer %d" % i)
    finally:
        dev.close()


def test_buffer_written_twice_keeps_the_last_field(v9):
    """Two frames of one batch write buffer 0 (the pixel path chains them): the one launch must
    not let both export into the buffer's planes; the field is the later frame's, whole."""
    w, h = 200, 130
    a = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5600))
    p = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5601, inter=1, compound=1))
    b = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5602))
    q = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5603, inter=1))
    frames, bufs, refs = [a, p, b, q], [0, 1, 0, 2], [None, (0, 0, 0), None, (0, 0, 0)]
    dev = _run(v9, frames, refs, (w, h), bufs=bufs)
    try:
        want = _want(frames)
        for buf, i in ((0, 2), (1, 1), (2, 3)):
            _same(dev.download_motion(buf), want[i], "buffer %d = frame %d" % (buf, i))
        dev.run_batch()                            # a replay of the same staging
        dev.sync()
        _same(dev.download_motion(0), want[2], "buffer 0 after a second run")
    finally:
        dev.close()


def test_refused_run_leaves_no_field(v9):
    """A batch with inter frames that the device planner refuses stops before its launches
    (tests/test_gpu_rejected_batch.py): none of its buffers holds a field afterwards, and a
    later good batch gives them theirs."""
    w, h = 200, 130
    frames, refs = _batch(v9, w, h, seed=5700)
    v9.test_hooks(reject_batch=1, reject_frame=1)
    try:
        dev = v9.Device(0)
    finally:
        v9.test_hooks()
    try:
        dev.set_export(motion=True)
        dev.configure(w, h, 8, nbufs=3)
        dev.set_timing(False)
        dev.stage_batch(frames, [0, 1, 2], refs)
        with pytest.raises(v9.Vp9HipError) as e:
            dev.run_batch()
        assert e.value.code == v9.EINVALIDDATA
        for buf in range(3):
            with pytest.raises(v9.Vp9HipError) as e:
                dev.download_motion(buf)
            assert e.value.code == v9.EAGAIN
        dev.stage_batch(frames, [0, 1, 2], refs)   # the hook names the first batch only
        dev.run_batch()
        dev.sync()
        for i, want in enumerate(_want(frames)):
            _same(dev.download_motion(i), want, "restaged frame %d" % i)
    finally:
        dev.close()


def _stream(v9, w=352, h=288):
    """key + 7 inter: key, P, [hidden ALTREF + P] superframe, P, show_existing of the hidden
    frame, three compound P on (LAST, GOLDEN, ALTREF = hidden); the shape of
    tests/test_ivf_decoder.py's stream."""
    fr = _frames(v9, w, h, 8, compound=1, seed=5500)
    enc = v9.Stream()
    d0, _ = enc.encode(fr[0])
    d1, _ = enc.encode(fr[1], ref_slot=(0, 0, 0), refresh_mask=1 << 1)
    dh, _ = enc.encode(fr[2], show_frame=0, ref_slot=(1, 0, 0), refresh_mask=1 << 2)      # hidden
    d3, _ = enc.encode(fr[3], ref_slot=(1, 0, 2), refresh_mask=1 << 3, refresh_ctx=1, parallel=0)
    d4, _ = enc.encode(fr[4], ref_slot=(3, 0, 2), refresh_mask=1 << 4)
    dx, _ = enc.encode(None, show_existing_frame=1, show_slot=2)
    tail = [enc.encode(fr[i], ref_slot=(i - 1, 0, 2), refresh_mask=1 << i)[0] for i in (5, 6, 7)]
    return [d0, d1, v9.superframe_join([dh, d3]), d4, dx] + tail


@pytest.fixture(scope="module")
def stream_fields(v9):
    """The stream and, per output, the restatement of its packet as a separate Stream parses it:
    (packets, fields in output order, index of the shown-existing output, the hidden frame's field)."""
    pkts = _stream(v9)
    st = v9.Stream()
    slots, outs, hidden, shown_existing = [None] * 8, [], None, None
    for data in pkts:
        for fr in v9.superframe_split(data):
            p, info = st.decode(fr)
            if info.show_existing_frame:
                shown_existing = len(outs)
                outs.append(slots[info.show_slot])
                continue
            field = motion_field(p.blocks(), p.pkt.width, p.pkt.height)[:2]
            for s in range(8):
                if info.refresh_mask & (1 << s):
                    slots[s] = field
            if info.show_frame:
                outs.append(field)
            else:
                hidden = field
    assert len(outs) == 8 and hidden is not None and outs[shown_existing] is hidden
    return pkts, outs, shown_existing, hidden


@pytest.mark.parametrize("max_batch", [1, 7])
def test_decoder_fields(v9, stream_fields, max_batch):
    pkts, want, xi, hidden = stream_fields
    dec = v9.Decoder(0, export_motion=True, max_batch=max_batch)
    try:
        got = []
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            got.append(dec.motion(info, download=True))
            if len(got) == 2:
                mv, inf = dec.motion(info)         # the torch views of the same field
                _same((mv.cpu().numpy(), inf.cpu().numpy()), got[-1], "views")
            dec.release(info.buf)
        assert dec.eof and len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            _same(g, w, "batch %d output %d" % (max_batch, i))
        _same(got[xi], hidden, "show_existing_frame")
    finally:
        dec.close()


def test_decoder_without_export(v9, stream_fields):
    pkts = stream_fields[0]
    dec = v9.Decoder(0, max_batch=4)
    try:
        n = 0
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            if n == 0:
                with pytest.raises(v9.Vp9HipError) as e:
                    dec.motion(info, download=True)
                assert e.value.code == v9.EINVAL
            dec.release(info.buf)
            n += 1
        assert n == 8
    finally:
        dec.close()
    dec = v9.Decoder(0, export_motion=True)
    try:
        dec.send_packet(pkts[0])
        with pytest.raises(v9.Vp9HipError) as e:
            v9._check("vp9hip_decoder_set_export", v9.lib().vp9hip_decoder_set_export(dec._d, 0))
        assert e.value.code == v9.EINVAL           # after the first send_packet
    finally:
        dec.close()
