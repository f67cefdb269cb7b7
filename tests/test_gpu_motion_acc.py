"""Accumulated motion on the GPU: k_mvacc's records against the numpy restatement of the
definition (tests/test_motion_acc_definition.py, which shares no code with the library). Exact
equality.

The kernel walks a chain through the frames of a batch and closes it with one read of a finished
record at a parent outside the batch; the definition is a frame-by-frame recurrence. Every chain
here runs as one batch (all walk), as batches of one frame rotating over the pipeline slots (all
recurrence) and split 3 + 4, and the three must agree with each other and with the reference.
Then the serials, the torch view, the end codes, the lifecycle rules and the bitstream decoder.
"""
try:     # torch first: Device.motion_acc returns torch views that share the HIP runtime (see _torch_first)
    import torch  # noqa: F401
except Exception:  # pragma: no cover
    torch = None

import numpy as np
import pytest

from test_gpu_motion import _stream
from test_motion_acc_definition import CELL, INTRA, NOFIELD, SCALED, acc_chain, acc_frame, gop_fields, gop_frames, gop_parents
from test_motion_definition import motion_field

pytestmark = pytest.mark.gpu

N = 7
REFS = [None] + [gop_parents(t) for t in range(1, N)]       # buffer t holds frame t


def _device(v9, cfg, nbufs, acc=True, motion=True):
    dev = v9.Device(0)
    if motion or acc:
        dev.set_export(motion=motion, motion_acc=acc)
    dev.configure(cfg[0], cfg[1], 8, nbufs=nbufs)
    dev.set_timing(False)
    return dev


def _run_split(v9, frames, cfg, split):
    """The chain in batches of the sizes in `split`, batch k in slot k % 3: (cells, serial) per frame."""
    dev = _device(v9, cfg, N)
    try:
        t = 0
        for k, n in enumerate(split):
            dev.set_slot(k % 3)
            dev.stage_batch(frames[t:t + n], list(range(t, t + n)), REFS[t:t + n])
            dev.run_batch()
            t += n
        dev.sync()
        return [dev.download_motion_acc(i) for i in range(N)]
    finally:
        dev.close()


def _same(got, want, what):
    assert got.dtype == CELL and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        r, c = bad[0]
        raise AssertionError("%s: %d cells differ, first (%d, %d): got %s, want %s" % (what, len(bad), r, c, got[r, c], want[r, c]))


CHAINS = {
    "8x8": dict(w=8, h=8),
    "66x66": dict(w=66, h=66),
    "200x130": dict(w=200, h=130),
    "528x72-2tiles": dict(w=528, h=72, synth=dict(log2_tile_cols=1)),
    "66x34-in-200x130-mv512": dict(w=66, h=34, cfg=(200, 130), synth=dict(mv_range=512)),
    "200x130-refmix": dict(w=200, h=130, synth=dict(ref_mix=1)),
}


@pytest.mark.parametrize("name", list(CHAINS))
def test_chains_walk_equals_recurrence(v9, name):
    c = CHAINS[name]
    w, h = c["w"], c["h"]
    frames = gop_frames(v9, w, h, N, **c.get("synth", {}))
    want, clamped = acc_chain(gop_fields(frames), gop_parents)
    if "mv512" in name:                                   # the reference alone: mostly clamps
        inter = sum(int((a["hops"] > 0).sum()) for a in want[1:])
        assert sum(int(m.sum()) for m in clamped) * 2 > inter
    cfg = c.get("cfg", (w, h))
    runs = {"one batch": _run_split(v9, frames, cfg, [N]),
            "batches of one": _run_split(v9, frames, cfg, [1] * N),
            "3 + 4": _run_split(v9, frames, cfg, [3, 4])}
    for how, got in runs.items():
        for t, (cells, serial) in enumerate(got):
            assert serial == t + 1, "%s %s: frame %d has serial %d" % (name, how, t, serial)
            _same(cells, want[t], "%s %s frame %d" % (name, how, t))
    # every root is the serial the API returned for that frame (or 0: unknown)
    serials = {s for _, s in runs["one batch"]}
    for cells, _ in runs["one batch"]:
        assert set(np.unique(cells["root"]).tolist()) <= serials | {0}
    for how in ("batches of one", "3 + 4"):
        for t in range(N):
            assert runs[how][t][0].tobytes() == runs["one batch"][t][0].tobytes(), "%s: %s differs from one batch at frame %d" % (name, how, t)


def test_torch_view(v9):
    """Device.motion_acc: a zero-copy int32 view strided over the fixed pitch of a larger context."""
    frames = gop_frames(v9, 66, 34, 3, seed=7200)
    want, _ = acc_chain(gop_fields(frames), gop_parents)
    dev = _device(v9, (200, 130), 3)
    try:
        dev.stage_batch(frames, [0, 1, 2], REFS[:3])
        dev.run_batch()
        dev.sync()
        for i in range(3):
            ptr, (gw, gh), pitch, serial, stream = dev.frame_motion_acc(i)
            assert (gw, gh, pitch, serial) == (18, 10, 50, i + 1) and ptr and stream
            t = dev.motion_acc(i, device="cuda:0")
            assert tuple(t.shape) == (10, 18, 4) and t.dtype == torch.int32 and t.stride() == (50 * 4, 4, 1)
            assert t.data_ptr() == ptr
            dx, dy, root, hops, end = [x.cpu().numpy() for x in v9.acc_fields(t)]
            assert np.array_equal(dx, want[i]["dx"]) and np.array_equal(dy, want[i]["dy"])
            assert np.array_equal(root.astype(np.uint32), want[i]["root"])
            assert np.array_equal(hops, want[i]["hops"]) and np.array_equal(end, want[i]["end"])
    finally:
        dev.close()


def _field(f):
    return motion_field(f.blocks(), f.pkt.width, f.pkt.height)[:2]


def test_uploaded_reference_has_no_field(v9):
    w, h = 200, 130
    p = v9.SynthFrame(v9.synth_params(w, h, 8, seed=7301, inter=1, p_intra=0.3))
    dev = _device(v9, (w, h), 2)
    try:
        dev.upload(0, v9.alloc_planes(w, h, 8))
        dev.stage_batch([p], [1], [(0, 0, 0)])
        dev.run_batch()
        dev.sync()
        cells, serial = dev.download_motion_acc(1)
        assert serial == 1
        _same(cells, acc_frame(*_field(p), 1, [None] * 3)[0], "P on an uploaded frame")
        inter = cells["hops"] > 0
        assert inter.any() and (~inter).any()
        assert (cells["end"][inter] == NOFIELD).all() and (cells["root"][inter] == 0).all() and (cells["hops"][inter] == 1).all()
        assert (cells["end"][~inter] == INTRA).all() and (cells["root"][~inter] == 1).all()
    finally:
        dev.close()


def test_not_the_last_writer_is_no_parent(v9):
    """[a, p, b, q] into buffers [0, 1, 0, 2]: p reads buffer 0 as a wrote it, but b writes it
    later and only b's field survives the batch, so p has no parent; q chains into b."""
    w, h = 200, 130
    a = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5600))
    p = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5601, inter=1, compound=1))
    b = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5602))
    q = v9.SynthFrame(v9.synth_params(w, h, 8, seed=5603, inter=1))
    dev = _device(v9, (w, h), 3)
    try:
        dev.stage_batch([a, p, b, q], [0, 1, 0, 2], [None, (0, 0, 0), None, (0, 0, 0)])
        dev.run_batch()
        dev.sync()
        wb = acc_frame(*_field(b), 3, [None] * 3)[0]
        for _ in range(2):
            _same(dev.download_motion_acc(0)[0], wb, "buffer 0 = b")
            assert dev.download_motion_acc(0)[1] == 3
            got_p, sp = dev.download_motion_acc(1)
            _same(got_p, acc_frame(*_field(p), 2, [None] * 3)[0], "p")
            assert sp == 2 and (got_p["end"][got_p["hops"] > 0] == NOFIELD).all()
            got_q, sq = dev.download_motion_acc(2)
            _same(got_q, acc_frame(*_field(q), 4, [wb] * 3)[0], "q")
            assert sq == 4 and (got_q["root"][got_q["hops"] > 0] == 3).all()    # q's own intra cells end in q
            dev.run_batch()                              # a re-run keeps the serials
            dev.sync()
    finally:
        dev.close()


@pytest.mark.parametrize("one_batch", [False, True])
def test_scaled_parent(v9, one_batch):
    """A 320x208 frame predicted from a 200x130 key: the parent's grid differs."""
    (rw, rh), (w, h) = (200, 130), (320, 208)
    key = v9.SynthFrame(v9.synth_params(rw, rh, 8, seed=900))
    f = v9.SynthFrame(v9.synth_params(w, h, 8, seed=901, inter=1))
    for r in range(3):
        f.pkt.ref_w[r], f.pkt.ref_h[r] = rw, rh
    dev = _device(v9, (w, h), 2)
    try:
        if one_batch:
            dev.stage_batch([key, f], [0, 1], [None, (0, 0, 0)])
            dev.run_batch()
        else:
            dev.stage_batch([key], [0])
            dev.run_batch()
            dev.stage_batch([f], [1], [(0, 0, 0)])
            dev.run_batch()
        dev.sync()
        cells, serial = dev.download_motion_acc(1)
        assert serial == 2 and cells.shape == (52, 80)
        _same(cells, acc_frame(*_field(f), 2, [None] * 3, (SCALED,) * 3)[0], "scaled")
        inter = cells["hops"] > 0
        assert inter.any() and (cells["end"][inter] == SCALED).all()
        _same(dev.download_motion_acc(0)[0], acc_frame(*_field(key), 1, [None] * 3)[0], "key")
    finally:
        dev.close()


def test_refused_run_then_restage(v9):
    w, h = 200, 130
    frames = gop_frames(v9, w, h, 3, seed=7400)
    v9.test_hooks(reject_batch=1, reject_frame=1)
    try:
        dev = v9.Device(0)
    finally:
        v9.test_hooks()
    try:
        dev.set_export(motion=True, motion_acc=True)
        dev.configure(w, h, 8, nbufs=3)
        dev.set_timing(False)
        dev.stage_batch(frames, [0, 1, 2], REFS[:3])
        with pytest.raises(v9.Vp9HipError) as e:
            dev.run_batch()
        assert e.value.code == v9.EINVALIDDATA
        for buf in range(3):
            for call in (dev.download_motion_acc, dev.motion_acc, dev.frame_motion_acc):
                with pytest.raises(v9.Vp9HipError) as e:
                    call(buf)
                assert e.value.code == v9.EAGAIN
        dev.stage_batch(frames, [0, 1, 2], REFS[:3])     # the hook names the first batch only
        dev.run_batch()
        dev.sync()
        want, _ = acc_chain(gop_fields(frames), gop_parents, serial0=4)   # restagings count
        for i in range(3):
            cells, serial = dev.download_motion_acc(i)
            assert serial == 4 + i
            _same(cells, want[i], "restaged frame %d" % i)
    finally:
        dev.close()


def test_error_codes_and_nothing_else_changes(v9):
    w, h = 200, 130
    frames = gop_frames(v9, w, h, 3, seed=7500)
    devs = []
    try:
        for acc in (False, True):
            dev = _device(v9, (w, h), 4, acc=acc)
            devs.append(dev)
            dev.stage_batch(frames, [0, 1, 2], REFS[:3])
            dev.run_batch()
            dev.sync()
        off, on = devs
        for i in range(3):
            for p, (a, b) in enumerate(zip(off.download(i), on.download(i))):
                assert a.tobytes() == b.tobytes(), "frame %d plane %d changed with the flag on" % (i, p)
            for a, b in zip(off.download_motion(i), on.download_motion(i)):
                assert a.tobytes() == b.tobytes(), "frame %d: the motion field changed with the flag on" % i
        for call in (off.download_motion_acc, off.motion_acc, off.frame_motion_acc):
            with pytest.raises(v9.Vp9HipError) as e:
                call(0)                                  # motion export alone: no such plane
            assert e.value.code == v9.EINVAL
        for buf, code in ((3, v9.EAGAIN), (4, v9.EINVAL), (-1, v9.EINVAL)):
            with pytest.raises(v9.Vp9HipError) as e:
                on.download_motion_acc(buf)              # never written / no such buffer
            assert e.value.code == code
        with pytest.raises(v9.Vp9HipError) as e:
            on.set_export(motion=True)                   # configured: the flags are fixed
        assert e.value.code == v9.EINVAL
        on.set_export(motion=True, motion_acc=True)      # no change: accepted
        on.fill(1, 1, 0)                                 # written by another path: the field is gone
        on.sync()
        with pytest.raises(v9.Vp9HipError) as e:
            on.download_motion_acc(1)
        assert e.value.code == v9.EAGAIN
    finally:
        for dev in devs:
            dev.close()
    dev = v9.Device(0)
    try:
        with pytest.raises(v9.Vp9HipError) as e:
            dev.set_export(motion=False, motion_acc=True)    # only together with the motion export
        assert e.value.code == v9.EINVAL
        with pytest.raises(v9.Vp9HipError) as e:
            dev.set_export(motion=False, residual=True, motion_acc=True)
        assert e.value.code == v9.EINVAL
    finally:
        dev.close()


@pytest.fixture(scope="module")
def stream_acc(v9):
    """test_gpu_motion.py's stream (hidden ALTREF, show_existing_frame) and, per output, the
    reference from a separate Stream parse with slot tracking: (packets, [(cells, serial)] in
    output order, index of the shown-existing output, the hidden frame's (cells, serial))."""
    pkts = _stream(v9)
    st = v9.Stream()
    slots, outs, hidden, shown_existing, serial = [None] * 8, [], None, None, 0
    for data in pkts:
        for fr in v9.superframe_split(data):
            p, info = st.decode(fr)
            if info.show_existing_frame:
                shown_existing = len(outs)
                outs.append(slots[info.show_slot])
                continue
            serial += 1
            intra = p.pkt.keyframe or p.pkt.intraonly
            par = [None] * 3 if intra else [slots[info.ref_slot[k]][0] for k in range(3)]
            mv, inf = motion_field(p.blocks(), p.pkt.width, p.pkt.height)[:2]
            rec = (acc_frame(mv, inf, serial, par)[0], serial)
            for s in range(8):
                if info.refresh_mask & (1 << s):
                    slots[s] = rec
            if info.show_frame:
                outs.append(rec)
            else:
                hidden = rec
    assert len(outs) == 8 and hidden is not None and outs[shown_existing] is hidden
    assert max(int(c["hops"].max()) for c, _ in outs) >= 4
    return pkts, outs, shown_existing, hidden


@pytest.fixture(scope="module")
def decoded_acc():
    return {}


@pytest.mark.parametrize("max_batch", [1, 7])
def test_decoder(v9, stream_acc, decoded_acc, max_batch):
    pkts, want, xi, hidden = stream_acc
    dec = v9.Decoder(0, export_motion_acc=True, max_batch=max_batch)
    try:
        got = []
        for _, info in dec.decode([(d, i) for i, d in enumerate(pkts)], download=False):
            got.append(dec.motion_acc(info, download=True))
            if len(got) == 3:
                t, serial = dec.motion_acc(info)         # the torch view of the same field
                assert serial == got[-1][1] and t.dtype == torch.int32
                assert np.array_equal(t.cpu().numpy().reshape(-1), got[-1][0].view("<i4").reshape(-1))
                dec.motion(info, download=True)          # the flag turned the motion export on
            dec.release(info.buf)
        assert dec.eof and len(got) == len(want)
        for i, ((g, gs), (w, ws)) in enumerate(zip(got, want)):
            assert gs == ws, "batch %d output %d: serial %d, want %d" % (max_batch, i, gs, ws)
            _same(g, w, "batch %d output %d" % (max_batch, i))
        assert got[xi][1] == hidden[1]
        _same(got[xi][0], hidden[0], "show_existing_frame")
    finally:
        dec.close()
    decoded_acc[max_batch] = got
    if len(decoded_acc) == 2:                            # both batch sizes equal each other
        for (a, sa), (b, sb) in zip(decoded_acc[1], decoded_acc[7]):
            assert sa == sb and a.tobytes() == b.tobytes()


def test_decoder_without_the_flag(v9, stream_acc):
    dec = v9.Decoder(0, export_motion=True, max_batch=4)
    try:
        n = 0
        for _, info in dec.decode([(d, i) for i, d in enumerate(stream_acc[0])], download=False):
            if n == 0:
                with pytest.raises(v9.Vp9HipError) as e:
                    dec.motion_acc(info, download=True)
                assert e.value.code == v9.EINVAL
            dec.release(info.buf)
            n += 1
        assert n == 8
    finally:
        dec.close()
