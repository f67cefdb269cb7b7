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


def eob_histogram(pkts):
    """Counter of (tx size code, eob) over the coded tx blocks of the packets."""
    return collections.Counter((t.tx, t.eob) for p in pkts for t in walk(p))
