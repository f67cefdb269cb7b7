"""Helpers over pass-1 packets (not a test module): a digest of a packet's contents and a
walker that replays the order in which vp9hip_synth_frame (csrc/host/vp9h_synth.c), the
bitstream and the planners enumerate tx blocks: the packet's blocks in order; per coded block
the planes 0..2; per plane the tx blocks that start inside the frame, rows then columns
(vp9block.c:1005-1127). The GPU tests build their coverage conditions on it."""
import collections
import ctypes
import hashlib

BWH8 = [(8, 8), (8, 4), (4, 8), (4, 4), (4, 2), (2, 4), (2, 2), (2, 1), (1, 2), (1, 1), (1, 1), (1, 1), (1, 1)]
BS_8x8 = 9

TxBlock = collections.namedtuple("TxBlock", "bi block plane tx x y eob coef mode")


def packet_digest(pkt):
    """sha256 over everything a pass-1 packet carries."""
    h = hashlib.sha256()
    csz = 2 if pkt.bpp == 8 else 4
    h.update(repr((pkt.width, pkt.height, pkt.bpp, pkt.ss_h, pkt.ss_v, pkt.keyframe, pkt.intraonly, pkt.lossless,
                   pkt.filter_level, pkt.sharpness, pkt.log2_tile_cols, pkt.log2_tile_rows, bytes(pkt.lflvl),
                   list(pkt.ref_w), list(pkt.ref_h), pkt.nblocks, pkt.neobs, pkt.ncoefs)).encode())
    if pkt.nblocks:
        h.update(ctypes.string_at(pkt.blocks, pkt.nblocks * ctypes.sizeof(pkt.blocks._type_)))
    if pkt.neobs:
        h.update(ctypes.string_at(pkt.eobs, pkt.neobs * 2))
    if pkt.ncoefs:
        h.update(ctypes.string_at(pkt.coefs, pkt.ncoefs * csz))
    return h.hexdigest()


def walk(pkt):
    """Every coded tx block of the packet in packet order: TxBlock(block index, block, plane,
    tx size code, x, y (4x4 units inside the block), eob, index of its first coefficient, the
    intra mode that predicts it or None). Checks that the walk consumes exactly the packet's
    eobs and coefficients."""
    cols, rows = (pkt.width + 7) >> 3, (pkt.height + 7) >> 3
    ne = nc = 0
    for bi in range(pkt.nblocks):
        b = pkt.blocks[bi]
        if b.skip:
            continue
        w4, h4 = BWH8[b.bs]
        for pl in range(3):
            tx = b.uvtx if pl else b.tx
            step = 1 << tx
            ex, ey = min(2 * (cols - b.col), w4 * 2), min(2 * (rows - b.row), h4 * 2)
            if pl:
                ex >>= pkt.ss_h
                ey >>= pkt.ss_v
            for y in range(0, ey, step):
                for x in range(0, ex, step):
                    e = pkt.eobs[ne]
                    mode = None
                    if b.intra:
                        mode = b.uvmode if pl else b.mode[y * 2 + x if b.bs > BS_8x8 and b.tx == 0 else 0]
                    yield TxBlock(bi, b, pl, tx, x, y, e, nc, mode)
                    ne += 1
                    nc += e
    assert (ne, nc) == (pkt.neobs, pkt.ncoefs), ((ne, nc), (pkt.neobs, pkt.ncoefs))


# check_intra_mode's tables (vp9recon.c:49-97). Modes: 0 V, 1 H, 2 DC, 3 D45, 4 D135, 5 D117,
# 6 D153, 7 D63, 8 D207, 9 TM, 10 LEFT_DC, 11 TOP_DC, 12 DC_128, 13 DC_127, 14 DC_129.
MODE_NAMES = ["V", "H", "DC", "D45", "D135", "D117", "D153", "D63", "D207", "TM", "LEFT_DC", "TOP_DC", "DC_128",
              "DC_127", "DC_129"]
# mode_conv[mode][have_left][have_top]
MODE_CONV = [[[13, 0], [13, 0]], [[14, 14], [1, 1]], [[12, 11], [10, 2]], [[13, 3], [13, 3]], [[4, 4], [4, 4]],
             [[5, 5], [5, 5]], [[6, 6], [6, 6]], [[13, 7], [13, 7]], [[14, 14], [8, 8]], [[14, 0], [1, 9]]]
# edges[final mode] = (needs_left, needs_top, needs_topleft, needs_topright)
EDGES = [(0, 1, 0, 0), (1, 0, 0, 0), (1, 1, 0, 0), (0, 1, 0, 1), (1, 1, 1, 0), (1, 1, 1, 0), (1, 1, 1, 0),
         (0, 1, 0, 1), (1, 0, 0, 0), (1, 1, 1, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 0, 0), (0, 0, 0, 0),
         (0, 0, 0, 0)]

IntraTx = collections.namedtuple("IntraTx", "bi block plane tx x y mode final have_top have_left have_right "
                                            "top_have left_have tr")


def tile_col_start(pkt, col):
    """First 8x8 column of the tile column that holds 8x8 column `col` (set_tile_offset,
    vp9.c:1244-1250)."""
    sb_cols = (pkt.width + 63) >> 6
    for t in range(1 << pkt.log2_tile_cols):
        s0 = min((t * sb_cols) >> pkt.log2_tile_cols, sb_cols)
        s1 = min(((t + 1) * sb_cols) >> pkt.log2_tile_cols, sb_cols)
        if s0 <= col >> 3 < s1:
            return s0 << 3
    raise ValueError(col)


def intra_jobs(pkt):
    """Every intra tx block of the packet in the order intra_recon predicts them (per block
    luma, U, V; rows then columns; vp9recon.c:235-364), the blocks of skip blocks included,
    with what check_intra_mode (vp9recon.c:37-221) resolves for it, restated from the packet
    alone: IntraTx(block index, block, plane, tx size code, x, y (4x4 units of the plane inside
    the block), coded mode, final mode after mode_conv (0..14), have_top, have_left (false at
    the block's tile-column start), have_right, n_px_have of the top and of the left edge (the
    reference's formulas, whether or not the edge is there), the 4x4 top-right: "none" (not
    read), "real" or "repl" (the last top pixel repeated)."""
    cols, rows = (pkt.width + 7) >> 3, (pkt.height + 7) >> 3
    for bi in range(pkt.nblocks):
        b = pkt.blocks[bi]
        if not b.intra:
            continue
        w8, h8 = BWH8[b.bs]
        tile0 = tile_col_start(pkt, b.col)
        for pl in range(3):
            ss_h, ss_v = (pkt.ss_h, pkt.ss_v) if pl else (0, 0)
            tx = b.uvtx if pl else b.tx
            step = 1 << tx
            w4 = (w8 * 2) >> ss_h
            ex, ey = min(2 * (cols - b.col), w8 * 2) >> ss_h, min(2 * (rows - b.row), h8 * 2) >> ss_v
            for y in range(0, ey, step):
                for x in range(0, ex, step):
                    mode = b.uvmode if pl else b.mode[y * 2 + x if b.bs > BS_8x8 and b.tx == 0 else 0]
                    have_top = b.row > 0 or y > 0
                    have_left = b.col > tile0 or x > 0
                    have_right = x < w4 - 1
                    final = MODE_CONV[mode][have_left][have_top]
                    top_have = (((cols - b.col) << (not ss_h)) - x) * 4
                    left_have = (((rows - b.row) << (not ss_v)) - y) * 4
                    tr = "none"
                    if tx == 0 and EDGES[final][3]:
                        tr = "real" if have_top and have_right and 8 <= top_have else "repl"
                    yield IntraTx(bi, b, pl, tx, x, y, mode, final, have_top, have_left, have_right, top_have,
                                  left_have, tr)


def eob_histogram(pkts):
    """Counter of (tx size code, eob) over the coded tx blocks of the packets."""
    return collections.Counter((t.tx, t.eob) for p in pkts for t in walk(p))
