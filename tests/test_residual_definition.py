"""Residual export, the definition (include/vp9hip.h "residual export"), without a GPU.

residual_planes() restates the definition in numpy: the packet's tx blocks from synth_walk.walk,
the scatter by the oracle's scan tables, and the oracle's itxfm_add on a flat block of 0 and on a
flat block of m = 2^bpp - 1, combined by the header's identity clip(r, -m, m) = add(0) + (add(m) -
m). It shares no transform code with the library and is what tests/test_gpu_residual.py compares
the device planes with. Here: vp9hip_residual_host, the C++ statement, equals it on every case of
the GPU list; an all-skip frame is all zeros; a whole inter frame reconstructed by the oracle's
own frame loop from flat references equals mid + residual (positions, plane geometry and chroma
subsampling, with no walk on the test's side); and the cases cover what they are there for.
"""
import ctypes

import numpy as np
import pytest

from synth_walk import walk

# name -> frame size, bit depth, generator switches, context size. The batches are the motion
# tests' shape: key + P + compound P (test_gpu_residual.py wires the references).
CASES = {
    "8x8": dict(w=8, h=8),
    "66x66": dict(w=66, h=66),
    "200x130": dict(w=200, h=130, seed=6100),            # this seed draws a DC-only 32x32 block
    "66x66-10bit": dict(w=66, h=66, bpp=10),
    "66x34-12bit-444": dict(w=66, h=34, bpp=12, synth=dict(ss_h=0, ss_v=0)),
    "72x40-422": dict(w=72, h=40, synth=dict(ss_h=1, ss_v=0)),
    "66x66-lossless": dict(w=66, h=66, synth=dict(lossless=1)),
    "528x72-2tiles": dict(w=528, h=72, synth=dict(log2_tile_cols=1)),
    "66x66-in-200x130": dict(w=66, h=66, cfg=(200, 130)),
    "130x130-dense-stress": dict(w=130, h=130, synth=dict(eob_dense=1, coef_stress=1)),
    "130x130-dense-stress-10bit": dict(w=130, h=130, bpp=10, synth=dict(eob_dense=1, coef_stress=1)),
}
SEED = 6100


def shapes(pkt):
    cw, ch = 8 * ((pkt.width + 7) >> 3), 8 * ((pkt.height + 7) >> 3)
    return [(ch, cw), (ch >> pkt.ss_v, cw >> pkt.ss_h), (ch >> pkt.ss_v, cw >> pkt.ss_h)]


def tx_type(v9, pkt, t):
    """(tx code of the oracle's itxfm_add: 0..3, 4 = WHT; txtp) of a walked tx block."""
    if pkt.lossless:
        return 4, 0
    if t.block.intra and t.plane == 0 and t.tx < 3:
        return t.tx, v9.intra_txfm_type(t.mode)
    return t.tx, 0


def residual_planes(orc, v9, frame, seen=None):
    """The three int16 planes of the definition for one packet. `seen`, a set, collects (tx code,
    txtp, eob) of every coded block."""
    pkt = frame.pkt if hasattr(frame, "pkt") else frame
    m = (1 << pkt.bpp) - 1
    cdt, pdt = (np.int16, np.uint8) if pkt.bpp == 8 else (np.int32, np.uint16)
    coefs = np.frombuffer(ctypes.string_at(pkt.coefs, pkt.ncoefs * cdt().itemsize), cdt) if pkt.ncoefs else np.zeros(0, cdt)
    out = [np.zeros(s, np.int16) for s in shapes(pkt)]
    scans = {}
    for t in walk(pkt):
        if not t.eob:
            continue
        tx, txtp = tx_type(v9, pkt, t)
        if seen is not None:
            seen.add((tx, txtp, t.eob))
        n = 4 << (tx & 3)
        if (tx, txtp) not in scans:
            scans[tx, txtp] = orc.scan(tx, txtp)
        blk = np.zeros(n * n, cdt)
        blk[scans[tx, txtp][:t.eob]] = coefs[t.coef:t.coef + t.eob]
        lo, hi = np.zeros((n, n), pdt), np.full((n, n), m, pdt)
        orc.itxfm_add(pkt.bpp, lo, blk.copy(), t.eob, tx, txtp)
        orc.itxfm_add(pkt.bpp, hi, blk, t.eob, tx, txtp)
        r = lo.astype(np.int32) + (hi.astype(np.int32) - m)          # clip(r, 0, m) + clip(r, -m, 0)
        sh, sv = (pkt.ss_h, pkt.ss_v) if t.plane else (0, 0)
        x0, y0 = (t.block.col * 8 >> sh) + 4 * t.x, (t.block.row * 8 >> sv) + 4 * t.y
        dst = out[t.plane][y0:y0 + n, x0:x0 + n]                      # what lies outside the coded area is dropped
        dst[...] = r[:dst.shape[0], :dst.shape[1]]
    return out


def batch(v9, name):
    """The case's frames: key + P + compound P."""
    c = CASES[name]
    w, h, bpp, kw = c["w"], c["h"], c.get("bpp", 8), c.get("synth", {})
    seed = c.get("seed", SEED + 16 * (1 + list(CASES).index(name)))
    return [v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed, **kw)),
            v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 1, inter=1, p_intra=0.3, **kw)),
            v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 2, inter=1, compound=1, **kw))]


_cache = {}


def reference(orc, v9, name):
    """(frames, their residual planes, the (tx, txtp, eob) seen) of a case: computed once, shared
    by the CPU and the GPU tests, never modified."""
    if name not in _cache:
        frames, seen = batch(v9, name), set()
        want = [residual_planes(orc, v9, f, seen) for f in frames]
        for pl in want:
            for a in pl:
                a.setflags(write=False)
        _cache[name] = (frames, want, seen)
    return _cache[name]


def same(got, want, what):
    assert len(got) == 3
    for p, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and g.dtype == np.int16, "%s plane %d: %s %s" % (what, p, g.shape, g.dtype)
        bad = g != w
        assert not bad.any(), "%s plane %d: %d samples differ, first at (y, x) = %s" % (
            what, p, int(bad.sum()), tuple(np.argwhere(bad)[0]))


@pytest.mark.parametrize("name", list(CASES))
def test_host_statement_equals_the_restatement(v9, orc, name):
    frames, want, _ = reference(orc, v9, name)
    for i, f in enumerate(frames):
        same(v9.residual_host(f), want[i], "%s frame %d" % (name, i))


def test_all_skip_is_all_zero(v9, orc):
    f = v9.SynthFrame(v9.synth_params(200, 130, 8, seed=SEED + 900, inter=1, p_skip=1.0))
    assert all(b.skip for b in f.blocks()) and f.pkt.neobs == 0
    for got, want in zip(v9.residual_host(f), residual_planes(orc, v9, f)):
        assert got.shape == want.shape and not got.any() and not want.any()


def flat_inter_frame(v9, bpp, seed):
    """An inter frame without intra blocks and without the loop filter, for the whole-frame check."""
    f = v9.SynthFrame(v9.synth_params(200, 130, bpp, seed=seed, inter=1, compound=1, filter_level=0, p_intra=1e-9))
    assert not any(b.intra for b in f.blocks()), "seed %d draws an intra block" % seed
    assert any(not b.skip for b in f.blocks())
    return f


FLAT_SEEDS = {8: SEED + 950, 10: SEED + 951}


def flat_reconstruction(orc, v9, f):
    """recon - mid of the oracle's decode_frame from three references flat at mid = 2^(bpp - 1):
    motion compensation of a flat plane is flat, so this is the clipped residual."""
    pkt = f.pkt
    mid = 1 << (pkt.bpp - 1)
    ref = v9.alloc_planes(pkt.width, pkt.height, pkt.bpp, pkt.ss_h, pkt.ss_v)
    for a in ref:
        a[...] = mid
    out = v9.alloc_planes(pkt.width, pkt.height, pkt.bpp, pkt.ss_h, pkt.ss_v)
    orc.decode_frame(pkt, out, [ref, ref, ref])
    return [a.astype(np.int32) - mid for a in v9.visible(out, pkt.width, pkt.height, pkt.ss_h, pkt.ss_v)], ref


def check_against_flat_reconstruction(got, diff, pkt):
    m, mid = (1 << pkt.bpp) - 1, 1 << (pkt.bpp - 1)
    for p, (g, d) in enumerate(zip(got, diff)):
        vis = np.clip(g[:d.shape[0], :d.shape[1]].astype(np.int32), -mid, m - mid)
        assert np.array_equal(vis, d), "plane %d: %d samples differ" % (p, int((vis != d).sum()))
    assert any(d.any() for d in diff)


@pytest.mark.parametrize("bpp", [8, 10])
def test_whole_frame_against_the_oracles_frame_loop(v9, orc, bpp):
    f = flat_inter_frame(v9, bpp, FLAT_SEEDS[bpp])
    diff, _ = flat_reconstruction(orc, v9, f)
    check_against_flat_reconstruction(v9.residual_host(f), diff, f.pkt)


def test_cases_cover_what_they_are_for(v9, orc):
    seen = set()
    for name in CASES:
        seen |= reference(orc, v9, name)[2]
    pairs = {(tx, tp) for tx, tp, _ in seen}
    want = {(tx, tp) for tx in range(3) for tp in range(4)} | {(3, 0), (4, 0)}
    assert want <= pairs, "missing (tx, txtp): %s" % sorted(want - pairs)
    for tx in range(4):
        assert any(e == 1 for t, tp, e in seen if t == tx and tp == 0), "no DC-only block of tx %d" % tx
    assert any(e > 64 for t, _, e in seen if t == 3), "no 32x32 block with eob > 64"
    assert any(e == 1024 for t, _, e in seen if t == 3), "no full 32x32 block"
    for name, bpp in (("130x130-dense-stress", 8), ("130x130-dense-stress-10bit", 10)):
        m = (1 << bpp) - 1
        planes = [a for fr in reference(orc, v9, name)[1] for a in fr]
        assert any((a == m).any() for a in planes) and any((a == -m).any() for a in planes), "%s never reaches +-m" % name
        assert all(abs(int(a.min())) <= m and int(a.max()) <= m for a in planes)


def test_residual_host_refuses_small_planes_and_bad_packets(v9):
    f = v9.SynthFrame(v9.synth_params(66, 34, 8, seed=SEED + 970))
    L = v9.lib()
    planes = [np.zeros(s, np.int16) for s in shapes(f.pkt)]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in planes])
    pitch = (ctypes.c_ssize_t * 3)(*[a.shape[1] for a in planes])
    rows = (ctypes.c_int * 3)(*[a.shape[0] for a in planes])
    call = lambda pk, r: L.vp9hip_residual_host(ctypes.byref(pk), ctypes.byref(ptrs), ctypes.byref(pitch), ctypes.byref(r))
    assert call(f.pkt, rows) == 0
    short = (ctypes.c_int * 3)(rows[0] - 1, rows[1], rows[2])
    assert call(f.pkt, short) == v9.EINVAL
    cp = v9.FramePacket()
    ctypes.memmove(ctypes.byref(cp), ctypes.byref(f.pkt), ctypes.sizeof(cp))
    cp.ncoefs -= 1                                              # the totals disagree
    before = [a.copy() for a in planes]
    assert call(cp, rows) == v9.EINVALIDDATA
    assert all(np.array_equal(a, b) for a, b in zip(planes, before))
