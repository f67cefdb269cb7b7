"""The frames of tests/test_gpu_intra_edges.py and the census over them (not a test module).

What check_intra_mode (vp9recon.c:37-221) resolves for a tx block is a cell: (luma or chroma,
tx size, final mode after mode_conv, the edge that mode reads, cut short by the frame or not).
The top edge is cut by the frame's right edge, the left edge by its bottom. The frames are tiny,
one full superblock plus a cut one or less, and drawn with edge_large=1, so that blocks the
frame edge cuts stay whole and take large transforms. census() counts the cells from the packets
with synth_walk.intra_jobs, on the CPU; check_census() is the condition a case must meet before
anything is launched. The CPU checks of the walker and of the planners
(tests/test_intra_edges_host.py) run over the same packets.

Which blocks cross the frame edge follows from decode_sb (vp9.c:1115-1193): a square whose
midpoint along an axis lies inside the frame is partitioned freely, so a block of length L along
that axis may show more than L / 2 of it; a square whose midpoint lies outside splits or takes
the forced partition, whose coded block is L / 2 long along the axis and may show any part of
that. With at most 24 pixels of a cut superblock visible (SIZES), blocks 64 long along an axis
never cross the edge, 32-long ones show 8, 16 or 24 pixels and 16-long ones 8.

Not every short cell shows in the picture. V, D135, D117, D153 and TM read the top row at or left
of a pixel's own column, H, D135, D117, D153 and TM the left column at or above its own row: a
wrong clamp there changes only pixels outside the frame, which no later block reads (a scratch
build with ct = n - 1 for luma 32x32 V alone decodes every frame here exactly). The clamp shows
through DC, TOP_DC, D45 and D63 on the top edge and DC, LEFT_DC and D207 on the left one. The
census asks for every cell all the same: the planners' words are checked for all of them on the
CPU, and the kernel's reads stay inside its tile for all of them.
"""
import collections
import functools

import synth_walk

# luma sizes. 72 and 88 leave 8 and 24 pixels of the second superblock. 80 leaves 16: a 32x32
# transform sees 16 pixels only in the forced 32x64 / 64x32 block of a superblock that shows 9
# to 16 pixels (a free 32x32 block has its midpoint inside the frame, which leaves 24), so the
# clamp length 16 needs this size. 24x72 and 8x72: the left column's block is itself cut
# (TOP_DC short); 72x24, 72x8: LEFT_DC.
SIZES = [(72, 72), (88, 88), (80, 80), (24, 72), (8, 72), (72, 24), (72, 8)]
COUNTS = {(72, 72): 32, (88, 88): 32, (80, 80): 32, (24, 72): 40, (8, 72): 40, (72, 24): 40, (72, 8): 40}   # 256
TILE_SIZE = (520, 72)            # the narrowest frame that may have two tile columns
N_TILE = 96
FORMATS = {"420": (1, 1), "444": (0, 0), "422": (1, 0), "440": (0, 1)}

# first seed of each case: the first base, counting up in steps of 0x400 from 0xe0000 (4:2:0),
# 0xe40000 (4:4:4), 0xe80000 (4:2:2), 0xec0000 (4:4:0), 0xf00000 (gop) and 0xf40000 (tile), for
# which the case's condition holds, found on the CPU (the rarest cells are the 32x32 chroma
# transforms of 4:2:0, which need a 64x64 block); the bit depth does not change what is drawn
SEEDS = {("key", "420"): 0xfbc00, ("key", "444"): 0xe40400, ("key", "422"): 0xe80400, ("key", "440"): 0xec0000,
         ("gop", "420"): 0xf10000, ("tile", "420"): 0xf40000}
CASES = sorted(SEEDS)
GOP_P = 5                        # P frames per keyframe of a "gop" chain
P_INTRA = 0.85

# Cells that cannot be short, by (plane class 0 luma / 1 chroma, tx size code, is the plane
# subsampled along the edge's axis): the reason. Every other (plane class, tx, axis) can.
NEVER_SHORT = {
    (0, 0, 0): "the frame is coded in 8-pixel columns and rows: luma n_px_have is a multiple of 8",
    (0, 1, 0): "the frame is coded in 8-pixel columns and rows: luma n_px_have is a multiple of 8",
    (1, 0, 0): "n_px_have is a multiple of 4 in every plane",
    (1, 0, 1): "n_px_have is a multiple of 4 in every plane",
    (1, 1, 0): "along an axis that is not subsampled chroma is laid out as luma: a multiple of 8",
    (1, 3, 1): "uvtx is 32x32 along a subsampled axis only in a block 64 long along it (a 32-long one "
               "has 16 chroma pixels), and a 64-long block crosses the edge only with more than 32 "
               "pixels visible: none of SIZES",
}
# At 4:2:2 / 4:4:0 the forced 64x32 (32x64) block of a cut superblock has a 32x32 chroma transform
# that the edge cuts along the axis that is not subsampled, but it is the block's only one along
# the other axis and starts at the frame's edge there: the edge that is cut is not available
# (CHROMA32_AVAIL below), no mode reads it. At 4:4:4 chroma is laid out as luma.


def axis_ss(pc, axis, ss_h, ss_v):
    return (ss_h, ss_v)[axis] if pc else 0


def short_feasible(pc, tx, axis, ss_h, ss_v):
    """Can a tx block of plane class pc have a short edge along axis 0 (top) / 1 (left)?"""
    return (pc, tx, axis_ss(pc, axis, ss_h, ss_v)) not in NEVER_SHORT


def clamp_lengths(pc, tx, axis, ss_h, ss_v):
    """The short n_px_have values a feasible cell must show with SIZES: the 8, 16 and 24 visible
    luma pixels of the cut superblock, in the plane's units, below the tx size."""
    if not short_feasible(pc, tx, axis, ss_h, ss_v):
        return set()
    ss = axis_ss(pc, axis, ss_h, ss_v)
    return {v >> ss for v in (8, 16, 24) if (v >> ss) < (4 << tx)}


@functools.lru_cache(maxsize=None)
def frames(v9, kind, fmt, bpp=8):
    """The case's frames per size in batch order: {(w, h): [(SynthFrame, refs or None), ...]}.
    kind "key": COUNTS keyframes of each size; "gop": chains of one keyframe and GOP_P P frames
    (each reads the frame before it as LAST and its keyframe as GOLDEN and ALTREF) with the
    intra share raised; "tile": N_TILE keyframes of TILE_SIZE with two tile columns."""
    ss_h, ss_v = FORMATS[fmt]
    seed = SEEDS[(kind, fmt)]
    out = collections.OrderedDict()
    common = dict(ss_h=ss_h, ss_v=ss_v, edge_large=1)
    if kind == "tile":
        w, h = TILE_SIZE
        out[(w, h)] = [(v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + i, log2_tile_cols=1, **common)), None)
                       for i in range(N_TILE)]
        return out
    for si, (w, h) in enumerate(SIZES):
        fl = []
        for i in range(COUNTS[(w, h)]):
            s = seed + si * 64 + i
            if kind == "key" or i % (GOP_P + 1) == 0:
                fl.append((v9.SynthFrame(v9.synth_params(w, h, bpp, seed=s, **common)), None))
            else:
                k = i - i % (GOP_P + 1)
                fl.append((v9.SynthFrame(v9.synth_params(w, h, bpp, seed=s, inter=1, compound=1, p_intra=P_INTRA,
                                                         **common)), (i - 1, k, k)))
        out[(w, h)] = fl
    return out


def packets(v9, kind, fmt, inter_only=False):
    return [f.pkt for fl in frames(v9, kind, fmt).values() for f, r in fl if r is not None or not inter_only]


@functools.lru_cache(maxsize=None)
def references(v9, orc, kind, fmt, bpp):
    """The oracle's pictures of the case's frames, {(w, h): [planes, ...]}: decoded once and
    shared by every executor's test (nothing writes to them)."""
    ss_h, ss_v = FORMATS[fmt]
    out = {}
    for (w, h), fl in frames(v9, kind, fmt, bpp).items():
        dec = []
        for f, r in fl:
            pl = v9.alloc_planes(w, h, bpp, ss_h, ss_v)
            orc.decode_frame(f.pkt, pl, None if r is None else [dec[r[0]], dec[r[1]], dec[r[2]]])
            dec.append(pl)
        out[(w, h)] = dec
    return out


Census = collections.namedtuple("Census", "short lengths modes tr tile_first")


def census(pkts):
    """Counters over the intra tx blocks of the packets:
    short[(plane class, tx, final mode, axis)]   blocks whose final mode reads the edge of that
                                                 axis (0 top, 1 left), there but shorter than the tx
    lengths[(plane class, tx, axis, n_px_have)]  the short lengths of those blocks
    modes[(plane class, tx, final mode)]         every block
    tr[(final mode, state, why)]                 the 4x4 top-right of D45 / D63: "real", or "repl"
                                                 because have_right is false ("inner") or because
                                                 the frame ends ("frame")
    tile_first[(plane class, tx, coded mode)]    blocks with have_top in the first column of a
                                                 tile column but the first"""
    short, lengths, modes, tr, tile_first = (collections.Counter() for _ in range(5))
    for pkt in pkts:
        for t in synth_walk.intra_jobs(pkt):
            pc, n = int(t.plane > 0), 4 << t.tx
            modes[(pc, t.tx, t.final)] += 1
            left, top = synth_walk.EDGES[t.final][:2]
            for axis, reads, avail, have in ((0, top, t.have_top, t.top_have), (1, left, t.have_left, t.left_have)):
                if reads and avail and have < n:
                    short[(pc, t.tx, t.final, axis)] += 1
                    lengths[(pc, t.tx, axis, have)] += 1
            if t.tr != "none":
                tr[(t.final, t.tr, "" if t.tr == "real" else "frame" if t.have_right else "inner")] += 1
            if t.have_top and not t.have_left and t.block.col > 0:
                tile_first[(pc, t.tx, t.mode)] += 1
    return Census(short, lengths, modes, tr, tile_first)


def _name(pc, tx):
    return "%s %dx%d" % ("chroma" if pc else "luma", 4 << tx, 4 << tx)


# The (have_left, have_top) a 32x32 chroma transform can have in SIZES frames, by (ss_h, ss_v).
# Along a subsampled axis it lies in a block 64 long, and SIZES frames hold one whole superblock,
# at the frame's origin: along that axis the transform is the block's only one and starts at the
# frame's edge. Along an axis that is not subsampled the block holds two (or is the second 32-long
# block of the superblock). Every other tx size, luma's 32x32 included, has all four.
CHROMA32_AVAIL = {(1, 1): [(0, 0)], (1, 0): [(0, 0), (0, 1)], (0, 1): [(0, 0), (1, 0)],
                  (0, 0): [(0, 0), (0, 1), (1, 0), (1, 1)]}


def final_modes(pc, tx, ss_h, ss_v):
    """The final modes a tx block of this class and size can have in SIZES frames."""
    avail = CHROMA32_AVAIL[(ss_h, ss_v)] if pc and tx == 3 else CHROMA32_AVAIL[(0, 0)]
    return {synth_walk.MODE_CONV[m][l][t] for m in range(10) for l, t in avail}


def edge_modes(pc, tx, axis, ss_h, ss_v):
    """The final modes that read the edge of axis 0 (top) / 1 (left) with that edge there."""
    avail = CHROMA32_AVAIL[(ss_h, ss_v)] if pc and tx == 3 else CHROMA32_AVAIL[(0, 0)]
    fm = {synth_walk.MODE_CONV[m][l][t] for m in range(10) for l, t in avail if (t, l)[axis]}
    return {m for m in fm if synth_walk.EDGES[m][1 - axis]}


def check_census(c, ss_h, ss_v):
    """The condition on a case of SIZES frames: every final mode at every tx size of luma and of
    chroma (final_modes); every feasible short cell; every clamp length on each edge; nothing
    from NEVER_SHORT; the 4x4 top-right in its three states."""
    miss = []
    for pc in (0, 1):
        for tx in range(4):
            for m in range(15):
                if m not in final_modes(pc, tx, ss_h, ss_v):
                    assert not c.modes[(pc, tx, m)], "%s with final mode %s against CHROMA32_AVAIL" % (
                        _name(pc, tx), synth_walk.MODE_NAMES[m])
                    continue
                if not c.modes[(pc, tx, m)]:
                    miss.append("no %s block with final mode %s" % (_name(pc, tx), synth_walk.MODE_NAMES[m]))
            for axis in (0, 1):
                edge = "left" if axis else "top"
                got = {h for (p, t, a, h) in c.lengths if (p, t, a) == (pc, tx, axis)}
                if not short_feasible(pc, tx, axis, ss_h, ss_v):
                    assert not got, "%s %s edge short (%s) against NEVER_SHORT: %s" % (
                        _name(pc, tx), edge, sorted(got), NEVER_SHORT[(pc, tx, axis_ss(pc, axis, ss_h, ss_v))])
                    continue
                readers = edge_modes(pc, tx, axis, ss_h, ss_v)
                assert not got or readers, "%s %s edge read against CHROMA32_AVAIL" % (_name(pc, tx), edge)
                for m in sorted(readers):
                    if not c.short[(pc, tx, m, axis)]:
                        miss.append("no short %s edge: %s mode %s" % (edge, _name(pc, tx), synth_walk.MODE_NAMES[m]))
                want = clamp_lengths(pc, tx, axis, ss_h, ss_v) if readers else set()
                if not want <= got:
                    miss.append("%s %s edge: short lengths %s, want %s" % (_name(pc, tx), edge, sorted(got), sorted(want)))
    for m in (3, 7):
        for key in ((m, "real", ""), (m, "repl", "inner"), (m, "repl", "frame")):
            if not c.tr[key]:
                miss.append("4x4 top-right of %s never %s %s" % (synth_walk.MODE_NAMES[m], key[1], key[2]))
    assert not miss, "%d cells not covered: %s" % (len(miss), "; ".join(miss))


# tile case: the tx sizes a block in the first column of the second tile column can have with
# have_top. TILE_SIZE is one full superblock row and a cut one that shows 8 pixels: a 32x32
# chroma transform needs a 64x64 block, which in the full row starts at row 0 (no top) and
# which the cut row cannot hold (it splits or takes the forced 64x32 partition).
TILE_FIRST_TXS = {0: (0, 1, 2, 3), 1: (0, 1, 2)}


def check_tile_census(c):
    for pc, txs in TILE_FIRST_TXS.items():
        for tx in txs:
            for mode in range(10):
                assert c.tile_first[(pc, tx, mode)], "second tile's first column: no %s block of mode %s" % (
                    _name(pc, tx), synth_walk.MODE_NAMES[mode])
        assert not [k for k in c.tile_first if k[0] == pc and k[1] not in txs]
