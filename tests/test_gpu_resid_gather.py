"""GPU parity of resid_wave's one-round-trip coefficient gather and mask-free passes (8x8, 16x16,
32x32), sample-exact vs the oracle.

Per round of 8N scan-order coefficients, lane li of a block takes the eight at k0 + 8 * li: the
coefficients by wide loads from the dword at or below an only element-aligned address, their
LDS offsets in one 16-byte table load. Lanes whose eight start at or past eob skip the round;
what a live lane loads from eob on belongs to the next block (or, at the arena's end, is the pad)
and is scattered as zeros. The wave's whole LDS block is zeroed first and both passes read every
row. The cases:

  a  mixed eobs: 136x72 keyframes (two SB columns, partial right and bottom SBs), 2 per batch,
     at 8, 10 and 12 bits, with the default density, coef_stress at q_idx 255, and eob_dense=1
  b  arena end: 8x8, 16x16, 32x32 and 64x64 frames in batches of one, three seeds, at 8 and 10
     bits: the wide loads of the last blocks run to the arena's end and into its pad
  c  in place: 136x72 key + 2 P with compound prediction at 8 and 10 bits (k_resid_multi, at
     the partial SBs)
  d  a keyframe case and the GOP under the host planner (VP9HIP_HOST_PLAN=1): k_resid with a
     host job count
  e  the sparse setting (p_skip 0.7, p_zero_eob 0.9)

Coverage is asserted from the packets (synth_walk) before anything is launched. For each of
8x8, 16x16, 32x32 the frames of case a must hold a block with eob <= 8 (one live lane), an eob
that is no multiple of 8 (a tail to zero), blocks whose coefficients start at an odd and at an
even element offset of the batch's arena (the funnel shift), every txtp at 8x8 and 16x16 (by
the planners' own mode table), and an eob > 8N at 16x16 and 32x32 (a second round; an 8x8
block has 64 = 8N coefficients at most). What one setting can hold:

  - the default density stops eobs at 64, so only eob_dense=1 has second rounds: asserted there;
  - a 32x32 block with eob <= 8 did not turn up in 64 seeds of coef_stress or eob_dense frame
    pairs: the default-density case holds it, and the three settings together hold everything.

So each setting asserts what it is for, and the default one everything but the second round.
Case b asserts that in at least one seed per size the arena's last coded tx block is 8x8 or
larger. At 4:2:0 an 8x8 frame's last coded block is a 4x4 chroma one whatever the seed (none
of 8,192 seeds ends otherwise), so the 8x8 frames run at 4:2:0 and at 4:4:4, and carry the
assertion at 4:4:4. The seeds below were chosen on the CPU so that all of it holds; bit depth
does not change what the generator draws for the 136x72 cases.
"""
import os

import numpy as np
import pytest

import synth_walk

pytestmark = pytest.mark.gpu

W, H = 136, 72
SETTINGS = {"default": ({}, 0xa001), "stress": ({"coef_stress": 1, "q_idx": 255}, 0xa001), "dense": ({"eob_dense": 1}, 0xa01c)}
SPARSE = {"p_skip": 0.7, "p_zero_eob": 0.9}
# (bpp, frame size) -> first of the three seeds' base (seed = base + 16 * k + bpp)
ARENA_SEEDS = {(8, 8): 0xb000, (8, 16): 0xb000, (8, 32): 0xb040, (8, 64): 0xb000,
               (10, 8): 0xb040, (10, 16): 0xb000, (10, 32): 0xb000, (10, 64): 0xb000}
TXTPS = {"t0", "t1", "t2", "t3"}


def coverage(v9, frames):
    """tx size code -> what its coded blocks in the batch hold."""
    c = {1: set(), 2: set(), 3: set()}
    base = 0                                   # the batch's arena holds the frames' coefficients back to back
    for f in frames:
        for t in synth_walk.walk(f.pkt):
            if t.tx in c and t.eob:
                N = 4 << t.tx
                if t.eob <= 8:
                    c[t.tx].add("le8")
                if t.eob % 8:
                    c[t.tx].add("tail")
                if t.eob > 8 * N:
                    c[t.tx].add("round2")
                c[t.tx].add("odd" if (base + t.coef) & 1 else "even")
                if t.tx < 3 and t.plane == 0 and t.block.intra:
                    c[t.tx].add("t%d" % v9.intra_txfm_type(t.mode))
        base += f.pkt.ncoefs
    return c


def check_setting(name, c):
    for tx in (1, 2, 3):
        want = {"tail", "odd", "even"} | (TXTPS if tx < 3 else set())
        if name == "default" or tx < 3:
            want |= {"le8"}
        if name == "dense" and tx > 1:
            want |= {"round2"}
        assert want <= c[tx], "%s, tx code %d: missing %s" % (name, tx, sorted(want - c[tx]))


def _cmp(v9, got, ref, w, h, what, ssh=1, ssv=1):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


def _run_keyframes(v9, orc, dev, frames, w, h, bpp, what, ss=1):
    n = len(frames)
    dev.configure(w, h, bpp, nbufs=n, ss_h=ss, ss_v=ss)
    dev.stage_batch(frames, list(range(n)))
    dev.run_batch()
    dev.sync()
    for i, f in enumerate(frames):
        ref = v9.alloc_planes(w, h, bpp, ss, ss)
        orc.decode_frame(f.pkt, ref)
        _cmp(v9, dev.download(i), ref, w, h, "%s frame %d" % (what, i), ss, ss)


def _pair(v9, bpp, name):
    kw, seed = SETTINGS[name]
    return [v9.SynthFrame(v9.synth_params(W, H, bpp, seed=seed + i, **kw)) for i in range(2)]


def _gop(v9, orc, dev, bpp, seed, what, **kw):
    refs = [None, (0, 0, 0), (1, 1, 0)]
    frames = [v9.SynthFrame(v9.synth_params(W, H, bpp, seed=seed + i, inter=int(i > 0), **kw)) for i in range(3)]
    c = coverage(v9, frames[1:])
    assert all(c[tx] for tx in (1, 2, 3)) or "p_skip" in kw, "inter frames without 8x8, 16x16 or 32x32 blocks: %s" % c
    dev.configure(W, H, bpp, nbufs=3)
    dev.stage_batch(frames, [0, 1, 2], refs)
    dev.run_batch()
    dev.sync()
    dec = []
    for i, f in enumerate(frames):
        out = v9.alloc_planes(W, H, bpp)
        r = refs[i]
        orc.decode_frame(f.pkt, out, None if r is None else [dec[r[0]], dec[r[1]], dec[r[2]]])
        dec.append(out)
        _cmp(v9, dev.download(i), out, W, H, "%s frame %d" % (what, i))


@pytest.mark.parametrize("bpp", [8, 10, 12])
@pytest.mark.parametrize("name", ["default", "stress", "dense"])
def test_mixed_eobs(v9, orc, gpu, name, bpp):
    """Case a."""
    frames = _pair(v9, bpp, name)
    check_setting(name, coverage(v9, frames))
    _run_keyframes(v9, orc, gpu, frames, W, H, bpp, "136x72 %d-bit %s" % (bpp, name))


@pytest.mark.parametrize("bpp", [8, 10, 12])
def test_settings_together_hold_everything(v9, bpp):
    """Case a's coverage over its three settings (needs no launch)."""
    c = {1: set(), 2: set(), 3: set()}
    for name in SETTINGS:
        for tx, s in coverage(v9, _pair(v9, bpp, name)).items():
            c[tx] |= s
    for tx in (1, 2, 3):
        want = {"le8", "tail", "odd", "even"} | (TXTPS if tx < 3 else set()) | ({"round2"} if tx > 1 else set())
        assert want <= c[tx], "tx code %d: missing %s" % (tx, sorted(want - c[tx]))


@pytest.mark.parametrize("bpp", [8, 10])
@pytest.mark.parametrize("size,ss", [(8, 1), (8, 0), (16, 1), (32, 1), (64, 1)], ids=["8", "8-444", "16", "32", "64"])
def test_arena_end(v9, orc, gpu, size, ss, bpp):
    """Case b."""
    lasts = []
    for k in range(3):
        seed = ARENA_SEEDS[(bpp, size)] + 16 * k + bpp
        f = v9.SynthFrame(v9.synth_params(size, size, bpp, seed=seed, ss_h=ss, ss_v=ss))
        coded = [t for t in synth_walk.walk(f.pkt) if t.eob]
        lasts.append(coded[-1].tx if coded else None)
        _run_keyframes(v9, orc, gpu, [f], size, size, bpp, "%dx%d %d-bit ss=%d seed %#x" % (size, size, bpp, ss, seed), ss)
    if (size, ss) != (8, 1):
        assert any(tx is not None and tx >= 1 for tx in lasts), "no arena ends in an 8x8 or larger block: %s" % lasts


@pytest.mark.parametrize("bpp", [8, 10])
def test_gop_in_place(v9, orc, gpu, bpp):
    """Case c."""
    _gop(v9, orc, gpu, bpp, 0xa100 + bpp, "136x72 %d-bit compound GOP" % bpp, compound=1)


def test_host_planned(v9, orc):
    """Case d."""
    old = os.environ.get("VP9HIP_HOST_PLAN")
    os.environ["VP9HIP_HOST_PLAN"] = "1"            # read when the context is opened
    try:
        dev = v9.Device(0)
    finally:
        if old is None:
            del os.environ["VP9HIP_HOST_PLAN"]
        else:
            os.environ["VP9HIP_HOST_PLAN"] = old
    try:
        frames = _pair(v9, 8, "dense")
        check_setting("dense", coverage(v9, frames))
        _run_keyframes(v9, orc, dev, frames, W, H, 8, "host-planned 136x72 dense")
        _gop(v9, orc, dev, 8, 0xa108, "host-planned 136x72 compound GOP", compound=1)
    finally:
        dev.close()


def test_sparse(v9, orc, gpu):
    """Case e."""
    frames = [v9.SynthFrame(v9.synth_params(W, H, 8, seed=0xa200 + i, **SPARSE)) for i in range(2)]
    _run_keyframes(v9, orc, gpu, frames, W, H, 8, "136x72 sparse")
    _gop(v9, orc, gpu, 8, 0xa210, "136x72 sparse GOP", **SPARSE)
