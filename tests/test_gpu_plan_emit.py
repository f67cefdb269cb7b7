"""GPU check of k_pjplan's pass loop and of the emit after it: the device's records against the
host restatement, record for record.

k_pjplan (csrc/vp9hip_plan.hip) builds an SB's passes with a loop that only decides (a packed
prefix sum per chunk of 64 priority positions; a taken lane notes its pass and its rank inside its
size class and marks its units in the packed done words) and writes the pass words and the jobs
once, after the loop, from those records. 64x64 and 128x64 keyframes (one and two SBs) at 4:2:0
and 4:4:4 with

  - lossless content, every SB tiled by 4x4 jobs in all planes: the full 384 / 768 jobs, every
    pass of 16 jobs from several chunks;
  - edge_large content, 16x16 and 32x32 jobs beside small ones;
  - the keyframes of the same size and format of tests/plan_sched_cases.py, a mix of all sizes.

That the frames hold these shapes is asserted from the packets before the launch. Per SB the
device's WGRec, pass words and PJobs (vp9hip_test_plan_records) must equal vp9hip_plan_sched_host's
word for word, be a valid schedule by the Python-derived producers, and the pixels must equal the
oracle's.
"""
import numpy as np
import pytest

import plan_sched_cases as cases
from test_gpu_plan_heights import FIELDS, _cmp, frames as height_frames

pytestmark = pytest.mark.gpu


def frames(v9, fmt, w, h, kind):
    if kind == "mixed":
        return [f for f, r in cases.frames(v9, "key-%s-%dx%d" % (fmt, w, h))]
    return height_frames(v9, fmt, w, h, kind)


def check_shapes(fmt, w, kind, sbs):
    ss_h, ss_v = cases.FORMATS[fmt]
    jcap = 256 + 2 * (16 >> ss_h) * (16 >> ss_v)
    sizes = {q.ts for _, _, jobs, _ in sbs for q in jobs}
    if kind == "lossless":
        assert len(sbs) == w // 64 and all(len(jobs) == jcap for _, _, jobs, _ in sbs) and sizes == {0}
    elif kind == "edge_large":
        assert sizes >= {2, 3} and len(sizes) >= 3, "sizes %r" % sizes
    else:
        assert len(sizes) >= 3 and sizes >= {0, 2}, "sizes %r" % sizes
        assert any(len(jobs) > 64 for _, _, jobs, _ in sbs), "no SB of more than one chunk"


@pytest.mark.parametrize("kind", ["lossless", "edge_large", "mixed"])
@pytest.mark.parametrize("w,h", [(64, 64), (128, 64)])
@pytest.mark.parametrize("fmt", ["420", "444"])
def test_records_and_pixels(v9, orc, gpu, fmt, w, h, kind):
    ssh, ssv = cases.FORMATS[fmt]
    fl = frames(v9, fmt, w, h, kind)
    sbs = []
    for i, f in enumerate(fl):
        for sb, jobs in cases.sb_jobs(f.pkt).items():
            sbs.append((i, sb, jobs, cases.producers(jobs, ssh, ssv)))
    check_shapes(fmt, w, kind, sbs)
    n = len(fl)
    gpu.configure(w, h, 8, nbufs=n, ss_h=ssh, ss_v=ssv)
    gpu.stage_batch(fl, list(range(n)))
    gpu.run_batch()
    gpu.sync()
    dsbs, wgs, passes, jobs_a = gpu.plan_records()
    slot_of = {}
    for s in range(len(dsbs)):
        if wgs[s][3] == s:
            slot_of[(int(dsbs[s][0]), int(dsbs[s][1]) & 0xffff, int(dsbs[s][1]) >> 16)] = s
    for i, (sbx, sby), jobs, prods in sbs:
        what = "%s %dx%d %s frame %d SB (%d, %d)" % (fmt, w, h, kind, i, sbx, sby)
        s = slot_of[(i, sbx, sby)]
        order, ref_passes, _ = v9.plan_sched_host(ssh, ssv, [q.word for q in jobs])
        nj, npass = int(wgs[s][2]) & 0xffff, int(wgs[s][2]) >> 16
        assert (nj, npass) == (len(jobs), len(ref_passes)), "%s: %d jobs in %d passes, restatement %d in %d" % (
            what, nj, npass, len(jobs), len(ref_passes))
        bad = np.nonzero(passes[s][:npass] != ref_passes)[0]
        assert not len(bad), "%s: pass %d is %#x, restatement %#x" % (what, bad[0], passes[s][bad[0]], ref_passes[bad[0]])
        ref_words = np.array([jobs[int(j)].word for j in order], np.uint32) & FIELDS
        bad = np.nonzero((jobs_a[s][:nj] & FIELDS) != ref_words)[0]
        assert not len(bad), "%s: position %d holds job word %#x, restatement %#x" % (
            what, bad[0], jobs_a[s][bad[0]], ref_words[bad[0]])
        by_unit = {(q.p, q.ux0, q.uy0): j for j, q in enumerate(jobs)}
        dev_order = [by_unit[(int(a) & 3, int(a) >> 12 & 15, int(a) >> 16 & 15)] for a in jobs_a[s][:nj]]
        cases.check_schedule(jobs, prods, dev_order, passes[s][:npass])
    for i, f in enumerate(fl):
        out = v9.alloc_planes(w, h, 8, ssh, ssv)
        orc.decode_frame(f.pkt, out, None)
        _cmp(v9, gpu.download(i), out, w, h, "%s %dx%d %s frame %d" % (fmt, w, h, kind, i), ssh, ssv)
