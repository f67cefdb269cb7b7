"""GPU check of k_pjplan's intra pass schedule against its host restatement, record for record.

k_pjplan (csrc/vp9hip_plan.hip) list-schedules each SB's intra jobs into passes; readiness is a
test of two unit masks per job against the done bits of a row and a column of the SB plane. Every
case of tests/plan_sched_cases.py (64x64, 80x80, 88x88 and 128x64 frames; 4:2:0, 4:2:2, 4:4:0 and
4:4:4; keyframes, and key + P chains with p_intra 0.5; edge_large off and on; one 10-bit case;
lossless 4:2:0 and 4:4:4 frames for SBs of 384 and 768 jobs) is decoded as one batch, and per SB

  - the device's records (vp9hip_test_plan_records) equal vp9hip_plan_sched_host's: job and pass
    counts, every pass word, the job at every position (plane, size, mode slot, unit);
  - they are a valid schedule by the Python-derived producers: every job exactly once, every
    producer in a strictly earlier pass, at most 64 lanes per pass;
  - the pixels equal the oracle's.

The census (an SB with more than 256 jobs, a job with more than four producers, an SB the frame
edge cuts, an inter SB with uncovered units, a 4x4 with trx, a 4:4:4 SB of more than six chunks)
is asserted from the packets before the first launch.
"""
import numpy as np
import pytest

import plan_sched_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = 0x000fff0f           # plane, tx size, mode slot, x4, y4 of a PJob word


def _cmp(v9, got, ref, w, h, what, ssh, ssv):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


@pytest.mark.parametrize("name", list(cases.CASES))
def test_records_equal_restatement(v9, orc, gpu, name):
    cases.check_census(v9)
    fmt, (w, h), bpp, kind, extra = cases.CASES[name]
    ssh, ssv = cases.FORMATS[fmt]
    fl = cases.frames(v9, name)
    n = len(fl)
    gpu.configure(w, h, bpp, nbufs=n, ss_h=ssh, ss_v=ssv)
    gpu.stage_batch([f for f, r in fl], list(range(n)), [r for f, r in fl] if kind == "gop" else None)
    gpu.run_batch()
    gpu.sync()
    sbs, wgs, passes, jobs_a = gpu.plan_records()
    slot_of = {}
    for s in range(len(sbs)):
        if wgs[s][3] == s:
            slot_of[(int(sbs[s][0]), int(sbs[s][1]) & 0xffff, int(sbs[s][1]) >> 16)] = s
    seen = 0
    for i, (sbx, sby), jobs, prods in cases.case_sbs(v9, name):
        what = "%s frame %d SB (%d, %d)" % (name, i, sbx, sby)
        s = slot_of[(i, sbx, sby)]
        order, ref_passes, _ = v9.plan_sched_host(ssh, ssv, [q.word for q in jobs])
        nj, npass = int(wgs[s][2]) & 0xffff, int(wgs[s][2]) >> 16
        assert (nj, npass) == (len(jobs), len(ref_passes)), "%s: %d jobs in %d passes, restatement %d in %d" % (
            what, nj, npass, len(jobs), len(ref_passes))
        assert np.array_equal(passes[s][:npass], ref_passes), "%s: pass words differ" % what
        ref_words = np.array([jobs[int(j)].word for j in order], np.uint32) & FIELDS
        bad = np.nonzero((jobs_a[s][:nj] & FIELDS) != ref_words)[0]
        assert not len(bad), "%s: position %d holds job word %#x, restatement %#x" % (
            what, bad[0], jobs_a[s][bad[0]], ref_words[bad[0]])
        # the device's own records as a schedule: positions -> decode indices by the job's unit
        by_unit = {(q.p, q.ux0, q.uy0): j for j, q in enumerate(jobs)}
        dev_order = [by_unit[(int(a) & 3, int(a) >> 12 & 15, int(a) >> 16 & 15)] for a in jobs_a[s][:nj]]
        cases.check_schedule(jobs, prods, dev_order, passes[s][:npass])
        seen += 1
    assert seen, "%s: no SB with intra jobs" % name
    dec = []
    for i, (f, r) in enumerate(fl):
        out = v9.alloc_planes(w, h, bpp, ssh, ssv)
        orc.decode_frame(f.pkt, out, None if r is None else [dec[r[0]], dec[r[1]], dec[r[2]]])
        dec.append(out)
        _cmp(v9, gpu.download(i), out, w, h, "%s frame %d" % (name, i), ssh, ssv)
