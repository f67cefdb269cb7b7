"""CPU checks behind tests/test_gpu_intra_edges.py, over the same packets (intra_edge_cases).

The GPU test's coverage condition is counted with synth_walk.intra_jobs, a restatement of
check_intra_mode (vp9recon.c:37-221) from the packet alone. Two checks keep it and the planners
honest without a GPU:

  oracle trace   the oracle's check_intra_mode records what it resolved (vp9o_set_intra_trace);
                 the walker's sequence equals it call for call;
  planner export pl_intra_job through the host planner's argument rules (pl_intra_job_blk,
                 vp9hip_intra_job_host) and through the device planner's (pl_intra_job_sb,
                 vp9hip_intra_job_dev: x = 0, pw4 from TXR_RIGHT, positions from the SB and the
                 block's unit in it, the chroma plane size shifted by the subsampling), the very
                 functions the planners call, agrees with the walker on every intra tx block: the slot is
                 the final mode's, ct = min(n, n_px_have) - 1 on the top edge, cl on the left,
                 trreal is the "real" top-right.
"""
import pytest

import intra_edge_cases as cases
import synth_walk

TR_CODE = {"none": 0, "real": 1, "repl": 2}
# mslot of a final mode (vp9hip_work.h: 0 V, 1 H, 2 DL, 3 DR, 4 VR, 5 HD, 6 VL, 7 HU, 8 TM, 9 DC,
# 10 LEFT_DC, 11 TOP_DC, 12 DC_128, 13 DC_127, 14 DC_129), by mode (V H DC D45 D135 D117 D153 D63 ...)
SLOT_OF_MODE = [0, 1, 9, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14]
IDS = ["%s-%s" % c for c in cases.CASES]


@pytest.mark.parametrize("kind,fmt", cases.CASES, ids=IDS)
def test_walker_equals_the_oracle_trace(v9, orc, kind, fmt):
    ss_h, ss_v = cases.FORMATS[fmt]
    n = 0
    for (w, h), fl in cases.frames(v9, kind, fmt).items():
        dec = []
        for i, (f, r) in enumerate(fl):
            pl = v9.alloc_planes(w, h, 8, ss_h, ss_v)
            got = orc.intra_trace(f.pkt, pl, None if r is None else [dec[r[0]], dec[r[1]], dec[r[2]]])
            dec.append(pl)
            want = [(t.plane, t.tx, t.final, t.top_have if t.have_top else 0, t.left_have if t.have_left else 0,
                     TR_CODE[t.tr]) for t in synth_walk.intra_jobs(f.pkt)]
            assert len(got) == len(want), (w, h, i, len(got), len(want))
            for k, (g, x) in enumerate(zip(got.tolist(), want)):
                assert tuple(g) == x, "%dx%d frame %d call %d: oracle %s walker %s" % (w, h, i, k, g, x)
            n += len(want)
    assert n > 1000


def _planner_jobs(v9, pkt, t):
    """What the host planner and the device planner resolve for tx block t, each from what it
    holds of the block (pl_intra_job_blk, pl_intra_job_sb)."""
    cols, rows = (pkt.width + 7) >> 3, (pkt.height + 7) >> 3
    sh, sv = (pkt.ss_h, pkt.ss_v) if t.plane else (0, 0)
    b = t.block
    tile0 = synth_walk.tile_col_start(pkt, b.col)
    bx, by = b.col * 8 >> sh, b.row * 8 >> sv
    sbx, sby = b.col >> 3, b.row >> 3
    ux0, uy0 = ((bx - sbx * (64 >> sh)) >> 2) + t.x, ((by - sby * (64 >> sv)) >> 2) + t.y
    pw4 = (synth_walk.BWH8[b.bs][0] * 2) >> sh
    return (v9.intra_job_host(t.plane, t.tx, t.mode, bx, by, t.x, t.y, pw4, tile0, cols, rows, pkt.ss_h, pkt.ss_v, ux0, uy0),
            v9.intra_job_dev(t.plane, t.tx, t.mode, sbx, sby, ux0, uy0, t.x < pw4 - 1, tile0 >> 3, cols, rows, pkt.ss_h,
                             pkt.ss_v))


@pytest.mark.parametrize("kind,fmt", cases.CASES, ids=IDS)
def test_planners_agree_with_the_walker(v9, kind, fmt):
    n = 0
    for pkt in cases.packets(v9, kind, fmt):
        for t in synth_walk.intra_jobs(pkt):
            size = 4 << t.tx
            want = (SLOT_OF_MODE[t.final], int(t.have_top), int(t.have_left), min(size, t.top_have) - 1,
                    min(size, t.left_have) - 1)
            for who, j in zip(("host", "device"), _planner_jobs(v9, pkt, t)):
                what = "%s planner %dx%d block %d plane %d tx %d (%d, %d): %s, walker %s %s" % (
                    who, pkt.width, pkt.height, t.bi, t.plane, t.tx, t.x, t.y, j, want, t.tr)
                assert tuple(j[:5]) == want, what
                # the planners resolve trreal for every 4x4 block, whether or not its mode reads
                # the top-right (the kernel's formulas read it for D45 and D63 only)
                if t.tr != "none":
                    assert j.trreal == int(t.tr == "real"), what
                else:
                    assert j.trreal == int(t.tx == 0 and t.have_top and t.have_right and t.top_have >= 8), what
                # the edges the planner orders the job after are the ones its final mode reads
                left, top, tl, tr = synth_walk.EDGES[t.final]
                assert j.nd == left | top << 1 | tl << 2 | tr << 3
                assert j.trx == int(t.tx == 0 and tr and t.have_right)
            n += 1
    assert n > 1000


def test_intra_job_exports_reject_what_no_packet_has(v9):
    assert v9.intra_job_host(0, 0, 0, 56, 56, 1, 1, 2, 0, 8, 8, 1, 1, 15, 15).slot == 0
    with pytest.raises(v9.Vp9HipError):
        v9.intra_job_host(0, 0, 10, 0, 0, 0, 0, 2, 0, 8, 8, 1, 1, 0, 0)        # no coded mode
    with pytest.raises(v9.Vp9HipError):
        v9.intra_job_host(0, 0, 0, 64, 0, 0, 0, 2, 0, 8, 8, 1, 1, 0, 0)         # right of the frame
    with pytest.raises(v9.Vp9HipError):
        v9.intra_job_dev(1, 0, 0, 1, 0, 0, 0, 0, 0, 8, 8, 1, 1)                 # SB right of the frame
    with pytest.raises(v9.Vp9HipError):
        v9.intra_job_dev(0, 0, 0, 0, 0, 0, 0, 0, 1, 8, 8, 1, 1)                 # tile starts after its SB
