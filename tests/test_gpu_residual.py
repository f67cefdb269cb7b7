"""Residual export on the GPU: k_residual's planes against the numpy restatement of the definition
(tests/test_residual_definition.py: the oracle's itxfm_add on flat blocks, no transform code
shared with the library). Exact equality over the coded area.

Batch path over the smallest shapes where the kernel can go wrong (one block, frame edges cutting
blocks, 10 / 12 bits, 4:4:4 / 4:2:2, the WHT, tile columns, a larger context, dense 32x32 eobs
with coefficients that wrap and clip), the whole-frame check against the oracle's frame loop,
torch views, pixels untouched, motion and residual together, the error codes, re-runs and
staleness, slot rotation, and the bitstream decoder with a hidden frame and a
show_existing_frame. No test feeds the kernel an invalid packet: its guards are the shared
helper's, checked by tests/c/residual_host_check.cpp under the sanitizer build.
"""
try:     # torch first: Device.residual returns torch views that share the HIP runtime (see _torch_first)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

import numpy as np
import pytest

from test_gpu_motion import _stream
from test_motion_definition import motion_field
from test_residual_definition import (CASES, FLAT_SEEDS, SEED, check_against_flat_reconstruction, flat_inter_frame,
                                      flat_reconstruction, reference, residual_planes, same)

pytestmark = pytest.mark.gpu

REFS = [None, (0, 0, 0), (1, 0, 1)]      # of key + P + compound P: the frame before (LAST, ALTREF), the key (GOLDEN)


def _run(v9, frames, refs, cfg, motion=False, residual=True, bufs=None):
    pk = frames[0].pkt
    dev = v9.Device(0)
    if motion or residual:
        dev.set_export(motion=motion, residual=residual)
    dev.configure(cfg[0], cfg[1], pk.bpp, nbufs=1 + max(bufs or range(len(frames))), ss_h=pk.ss_h, ss_v=pk.ss_v)
    dev.set_timing(False)
    dev.stage_batch(frames, bufs or list(range(len(frames))), refs)
    dev.run_batch()
    dev.sync()
    return dev


@pytest.mark.parametrize("name", list(CASES))
def test_batch_fields(v9, orc, name):
    c = CASES[name]
    frames, want, _ = reference(orc, v9, name)
    dev = _run(v9, frames, REFS, c.get("cfg", (c["w"], c["h"])))
    try:
        for i in range(len(frames)):
            same(dev.download_residual(i), want[i], "%s frame %d" % (name, i))
    finally:
        dev.close()


@pytest.mark.parametrize("bpp", [8, 10])
def test_whole_frame_against_the_oracles_frame_loop(v9, orc, bpp):
    """The device field against recon - mid of the oracle's own frame loop over flat references
    (no walk on the test's side), and the device's pixels against the same reconstruction."""
    f = flat_inter_frame(v9, bpp, FLAT_SEEDS[bpp])
    diff, ref = flat_reconstruction(orc, v9, f)
    dev = v9.Device(0)
    try:
        dev.set_export(motion=False, residual=True)
        dev.configure(f.pkt.width, f.pkt.height, bpp, nbufs=2)
        dev.upload(0, ref)
        dev.submit(f, 1, (0, 0, 0))
        dev.sync()
        check_against_flat_reconstruction(dev.download_residual(1), diff, f.pkt)
        mid = 1 << (bpp - 1)
        for a, d in zip(v9.visible(dev.download(1), f.pkt.width, f.pkt.height), diff):
            assert np.array_equal(a.astype(np.int32) - mid, d)
    finally:
        dev.close()


def test_torch_views(v9, orc):
    """Device.residual: zero-copy int16 views of the visible size, strided over the pitch of a
    larger context."""
    frames = [v9.SynthFrame(v9.synth_params(66, 34, 8, seed=SEED + 500 + i, inter=int(i > 0), compound=int(i > 1)))
              for i in range(3)]
    want = [residual_planes(orc, v9, f) for f in frames]
    dev = _run(v9, frames, REFS, (200, 130))
    try:
        for i in range(3):
            down = dev.download_residual(i)
            same(down, want[i], "download frame %d" % i)
            y, u, v = dev.residual(i, device="cuda:0")
            assert tuple(y.shape) == (34, 66) and tuple(u.shape) == (17, 33) and tuple(v.shape) == (17, 33)
            assert y.dtype == u.dtype == v.dtype == torch.int16
            assert y.stride() == (256, 1) and u.stride() == (128, 1) and v.stride() == (128, 1)
            for t, d in zip((y, u, v), down):
                assert np.array_equal(t.cpu().numpy(), d[:t.shape[0], :t.shape[1]])
    finally:
        dev.close()


def test_pixels_untouched_and_both_exports(v9, orc):
    """Export off / residual / motion / both: byte-identical pixels, and each field equal to what
    it is alone."""
    frames, want, _ = reference(orc, v9, "200x130")
    off = _run(v9, frames, REFS, (200, 130), residual=False)
    res = _run(v9, frames, REFS, (200, 130))
    mot = _run(v9, frames, REFS, (200, 130), motion=True, residual=False)
    both = _run(v9, frames, REFS, (200, 130), motion=True)
    try:
        for i in range(3):
            pix = [a.tobytes() for a in off.download(i)]
            for name, dev in (("residual", res), ("motion", mot), ("both", both)):
                assert [a.tobytes() for a in dev.download(i)] == pix, "frame %d changed with %s export" % (i, name)
            same(res.download_residual(i), want[i], "alone, frame %d" % i)
            same(both.download_residual(i), want[i], "with motion, frame %d" % i)
            mv, info, _ = motion_field(frames[i].blocks(), 200, 130)
            for dev in (mot, both):
                gmv, ginfo = dev.download_motion(i)
                assert np.array_equal(gmv, mv) and np.array_equal(ginfo, info)
        for dev in (off, mot):                     # without the residual flag
            for call in (dev.residual, dev.download_residual, dev.frame_residual):
                with pytest.raises(v9.Vp9HipError) as e:
                    call(0)
                assert e.value.code == v9.EINVAL
        with pytest.raises(v9.Vp9HipError) as e:
            res.download_motion(0)                 # without the motion flag
        assert e.value.code == v9.EINVAL
    finally:
        for dev in (off, res, mot, both):
            dev.close()


def test_error_codes(v9, orc):
    frames, want, _ = reference(orc, v9, "66x66")
    dev = v9.Device(0)
    try:
        dev.set_export(motion=False, residual=True)
        dev.configure(66, 66, 8, nbufs=2)
        for flags in ((True, True), (True, False), (False, False)):
            with pytest.raises(v9.Vp9HipError) as e:
                dev.set_export(*flags)             # configured: the flags are fixed
            assert e.value.code == v9.EINVAL
        dev.set_export(motion=False, residual=True)        # no change: accepted
        for buf in (-1, 2):
            with pytest.raises(v9.Vp9HipError) as e:
                dev.download_residual(buf)         # no such buffer
            assert e.value.code == v9.EINVAL
        for call in (dev.residual, dev.download_residual, dev.frame_residual):
            with pytest.raises(v9.Vp9HipError) as e:
                call(1)                            # never written
            assert e.value.code == v9.EAGAIN
        dev.submit(frames[0], 1)
        dev.sync()
        same(dev.download_residual(1), want[0], "submit")
        assert dev.frame_residual(1)[2] == (66, 66)
        dev.fill(1, 1, 0)                          # written by another path: the field is gone
        dev.sync()
        with pytest.raises(v9.Vp9HipError) as e:
            dev.download_residual(1)
        assert e.value.code == v9.EAGAIN
        dev.submit(frames[0], 1)
        dev.sync()
        same(dev.download_residual(1), want[0], "submit again")
        dev.upload(1, v9.alloc_planes(66, 66, 8))
        with pytest.raises(v9.Vp9HipError) as e:
            dev.download_residual(1)
        assert e.value.code == v9.EAGAIN
    finally:
        dev.close()


def test_reruns_and_staleness(v9, orc):
    """run_batch twice on one staging (the second a graph replay) gives the same bytes; an
    all-skip frame staged into a buffer that held a dense field leaves all zeros."""
    frames, want, _ = reference(orc, v9, "130x130-dense-stress")
    dev = _run(v9, frames, REFS, (130, 130))
    try:
        first = [dev.download_residual(i) for i in range(3)]
        dev.run_batch()
        dev.run_batch()
        dev.sync()
        for i in range(3):
            same(first[i], want[i], "first run, frame %d" % i)
            same(dev.download_residual(i), want[i], "third run, frame %d" % i)
        assert any(a.any() for a in first[1])
        skip = v9.SynthFrame(v9.synth_params(130, 130, 8, seed=SEED + 600, inter=1, p_skip=1.0))
        assert all(b.skip for b in skip.blocks())
        dev.stage_batch([skip], [1], [(0, 0, 0)])
        dev.run_batch()
        dev.sync()
        got = dev.download_residual(1)
        assert [a.shape for a in got] == [a.shape for a in first[1]] and not any(a.any() for a in got)
        same(dev.download_residual(2), want[2], "the neighbour buffer")
    finally:
        dev.close()


def test_slots_keep_earlier_fields(v9, orc):
    """Five batches of two frames over the three pipeline slots into ten buffers: a later batch in
    a slot (its arena reused) leaves the earlier batches' fields alone."""
    w, h = 136, 72
    dev = v9.Device(0)
    dev.set_export(motion=False, residual=True)
    dev.configure(w, h, 8, nbufs=10)
    dev.set_timing(False)
    frames = []
    try:
        assert v9.PIPELINE_SLOTS == 3
        for k in range(5):
            pair = [v9.SynthFrame(v9.synth_params(w, h, 8, seed=SEED + 700 + 2 * k)),
                    v9.SynthFrame(v9.synth_params(w, h, 8, seed=SEED + 701 + 2 * k, inter=1, compound=k & 1))]
            frames += pair
            dev.set_slot(k % v9.PIPELINE_SLOTS)
            dev.stage_batch(pair, [2 * k, 2 * k + 1], [None, (2 * k,) * 3])
            dev.run_batch()
        dev.sync()
        for i, f in enumerate(frames):
            same(dev.download_residual(i), residual_planes(orc, v9, f), "buffer %d" % i)
    finally:
        dev.close()


@pytest.fixture(scope="module")
def stream_fields(v9, orc):
    """The motion test's stream (a hidden frame and a show_existing_frame of it) and, per output,
    the restatement over its packet as a separate Stream parses it."""
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
            field = residual_planes(orc, v9, p)
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
    dec = v9.Decoder(0, export_residual=True, max_batch=max_batch)
    try:
        got = []
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            got.append(dec.residual(info, download=True))
            if len(got) == 2:
                views = dec.residual(info)         # the torch views of the same field
                assert tuple(views[0].shape) == (info.height, info.width)
                for t, d in zip(views, got[-1]):
                    assert np.array_equal(t.cpu().numpy(), d[:t.shape[0], :t.shape[1]])
                with pytest.raises(v9.Vp9HipError) as e:
                    dec.motion(info, download=True)        # the motion flag is off
                assert e.value.code == v9.EINVAL
            dec.release(info.buf)
        assert dec.eof and len(got) == len(want)
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, "batch %d output %d" % (max_batch, i))
        same(got[xi], hidden, "show_existing_frame")
    finally:
        dec.close()


def test_decoder_without_export(v9, stream_fields):
    pkts = stream_fields[0]
    dec = v9.Decoder(0, max_batch=4, export_motion=True)
    try:
        n = 0
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            if n == 0:
                with pytest.raises(v9.Vp9HipError) as e:
                    dec.residual(info, download=True)
                assert e.value.code == v9.EINVAL
            dec.release(info.buf)
            n += 1
        assert n == 8
    finally:
        dec.close()
