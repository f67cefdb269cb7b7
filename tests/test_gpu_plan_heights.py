"""GPU check of k_pjplan's heights relaxation through what it decides: the priority order of the
list-scheduled passes, so the device's records against the host restatement, record for record.

k_pjplan (csrc/vp9hip_plan.hip) relaxes the heights of an SB's intra jobs chunk by chunk of 64
jobs (pl_heights_chunk of csrc/vp9hip_planlogic.h): a lane keeps its job's first four producers in
registers, and producers past the fourth take a loop in the chunks that hold such a job. 64x64 and
128x64 keyframes at 4:2:0 and 4:4:4 give both shapes:

  - lossless frames, every SB tiled by 4x4 jobs in all planes: the full 384 / 768 jobs, 6 / 12
    chunks, at least three of them with producers in earlier chunks;
  - edge_large frames, whose 16x16 and 32x32 jobs beside small ones have more than four producers.

That the seeds hold these shapes is asserted from the packets before the launch. Per SB the
device's WGRec, pass words and PJobs (vp9hip_test_plan_records) must equal vp9hip_plan_sched_host's
(one-sweep heights), be a valid schedule by the Python-derived producers, and the pixels must
equal the oracle's.
"""
import functools

import numpy as np
import pytest

import plan_sched_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = 0x000fff0f           # plane, tx size, mode slot, x4, y4 of a PJob word
SEED = 0x5c4f1100
# edge_large keyframes per case: seed offsets whose frames hold long lists (check_shapes)
LARGE = {("420", 64): (5, 16, 22), ("420", 128): (1, 12, 13), ("444", 64): (3, 14, 21), ("444", 128): (3, 10, 17)}


@functools.lru_cache(maxsize=None)
def frames(v9, fmt, w, h, kind):
    ss_h, ss_v = cases.FORMATS[fmt]
    if kind == "lossless":
        return [v9.SynthFrame(v9.synth_params(w, h, 8, seed=SEED + w, ss_h=ss_h, ss_v=ss_v, **cases.LOSSLESS))]
    return [v9.SynthFrame(v9.synth_params(w, h, 8, seed=SEED + w + 16 * i, ss_h=ss_h, ss_v=ss_v, edge_large=1))
            for i in LARGE[(fmt, w)]]


def check_shapes(v9, fmt, w, h, kind, sbs):
    """sbs: [(frame, (sbx, sby), jobs, producers)]. The shapes the case is there for."""
    ss_h, ss_v = cases.FORMATS[fmt]
    jcap = 256 + 2 * (16 >> ss_h) * (16 >> ss_v)
    if kind == "lossless":
        assert len(sbs) == w // 64 and all(len(jobs) == jcap and all(q.ts == 0 for q in jobs) for _, _, jobs, _ in sbs)
        for _, _, jobs, prods in sbs:             # chunks with a producer in an earlier chunk
            assert sum(any(d < c for j in range(c, c + 64) for d in prods[j]) for c in range(64, jcap, 64)) >= 3
    else:
        long = [(len(s), jobs[j].ts) for _, _, jobs, prods in sbs for j, s in enumerate(prods) if len(s) > 4]
        assert len(long) >= 6 and max(n for n, _ in long) >= 12 and any(ts >= 2 for _, ts in long), \
            "too few jobs with more than four producers: %r" % long


def _cmp(v9, got, ref, w, h, what, ssh, ssv):
    for p, (a, b) in enumerate(zip(v9.visible(got, w, h, ssh, ssv), v9.visible(ref, w, h, ssh, ssv))):
        if not np.array_equal(a, b):
            ys, xs = np.nonzero(a != b)
            raise AssertionError("%s plane %d: %d px differ, first at (x=%d, y=%d): gpu %d oracle %d"
                                 % (what, p, len(ys), xs[0], ys[0], a[ys[0], xs[0]], b[ys[0], xs[0]]))


@pytest.mark.parametrize("kind", ["lossless", "edge_large"])
@pytest.mark.parametrize("w,h", [(64, 64), (128, 64)])
@pytest.mark.parametrize("fmt", ["420", "444"])
def test_records_and_pixels(v9, orc, gpu, fmt, w, h, kind):
    ssh, ssv = cases.FORMATS[fmt]
    fl = frames(v9, fmt, w, h, kind)
    sbs = []
    for i, f in enumerate(fl):
        for sb, jobs in cases.sb_jobs(f.pkt).items():
            sbs.append((i, sb, jobs, cases.producers(jobs, ssh, ssv)))
    check_shapes(v9, fmt, w, h, kind, sbs)
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
        assert np.array_equal(passes[s][:npass], ref_passes), "%s: pass words differ" % what
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
