"""CPU check of the device planner's heights relaxation (pl_heights_chunk of
csrc/vp9hip_planlogic.h, the routine k_pjplan runs, here through vp9hip_plan_heights_host with a
loop over 64 lanes in place of the wave).

A job's height is its longest path to a sink of the SB's producer graph. Producers precede their
consumers in decode order, so one sweep h[d] = max(h[d], h[j] + 1) from the last job to the first
is exact; it runs here over producers derived in Python from geometry
(plan_sched_cases.producers). The routine must give the same heights

  - on every SB of every case of tests/plan_sched_cases.py, and
  - on job lists built here: 0, 1, 64, 65 and 128 jobs, SBs tiled by 4x4 jobs in all planes (384
    jobs at 4:2:0, 768 = 12 chunks at 4:4:4, chains across every chunk boundary), a 32x32, a 16x16
    and an 8x8 job beside 4x4 jobs (17, 5 and 4 producers) and a job without producers.

The reference's heights lie in 1..63 on all of them, so the planner's clamp at 63 is not what
makes the two agree.
"""
import numpy as np
import pytest

import plan_sched_cases as cases

# edges read by the mode of a PJob slot (pl_slot_needs): 1 left, 2 top, 4 top-left, 8 top-right
NEEDS = [2, 1, 2 | 8, 7, 7, 7, 2 | 8, 1, 7, 3, 1, 2, 0, 0, 0]
V, H, TM, DC, DC128 = 0, 1, 8, 9, 12


def job(p, ts, ux0, uy0, slot, trx=0):
    nd = NEEDS[slot]
    return cases.Job(p, ts, ux0, uy0, (nd & 1, nd >> 1 & 1, nd >> 2 & 1, nd >> 3 & 1), trx,
                     p | ts << 2 | slot << 8 | ux0 << 12 | uy0 << 16 | trx << 30)


def tiled(ss_h, ss_v, n=None):
    """4x4 TM jobs (left, top and top-left read) in raster order, plane after plane: chains run
    along every row and down every column, so they cross each boundary between chunks of 64."""
    out = []
    for p in range(3):
        w, h = (16 >> ss_h, 16 >> ss_v) if p else (16, 16)
        out += [job(p, 0, u, v, TM) for v in range(h) for u in range(w)]
    return out if n is None else out[:n]


def mixed():
    """Luma jobs, producers first: a 16x16 DC job under an 8x8 and two 4x4 and beside two 8x8
    (5 producers), a 32x32 TM job under eight 4x4, beside eight 4x4, with the 16x16 at its top-left
    (17), an 8x8 DC job under two 4x4 and beside two 4x4 (4)."""
    jobs = [job(0, 1, 4, 2, DC128), job(0, 0, 6, 3, DC128), job(0, 0, 7, 3, H), job(0, 1, 2, 4, DC128), job(0, 1, 2, 6, V)]
    big16 = len(jobs)
    jobs.append(job(0, 2, 4, 4, DC))
    jobs += [job(0, 0, u, 7, H) for u in range(8, 16)] + [job(0, 0, 7, v, V) for v in range(8, 16)]
    big32 = len(jobs)
    jobs.append(job(0, 3, 8, 8, TM))
    jobs += [job(0, 0, 2, 9, DC128), job(0, 0, 3, 9, H), job(0, 0, 1, 10, DC128), job(0, 0, 1, 11, V)]
    four = len(jobs)
    jobs.append(job(0, 1, 2, 10, DC))
    return jobs, big16, big32, four


def reference(prods):
    h = [1] * len(prods)
    for j in range(len(prods) - 1, -1, -1):
        for d in prods[j]:
            h[d] = max(h[d], h[j] + 1)
    return h


def check(v9, jobs, prods, ss_h, ss_v, what):
    ref = reference(prods)
    assert all(1 <= x <= 63 for x in ref), "%s: reference heights outside 1..63 (max %d)" % (what, max(ref))
    got = v9.plan_heights_host(ss_h, ss_v, [q.word for q in jobs])
    bad = np.nonzero(got != np.array(ref, np.uint32))[0]
    assert not len(bad), "%s: job %d height %d, longest path %d (%d of %d differ)" % (
        what, bad[0], got[bad[0]], ref[bad[0]], len(bad), len(jobs))
    return ref


@pytest.mark.parametrize("name", list(cases.CASES))
def test_heights_of_cases(v9, name):
    ss_h, ss_v = cases.FORMATS[cases.CASES[name][0]]
    seen = 0
    for i, sb, jobs, prods in cases.case_sbs(v9, name):
        check(v9, jobs, prods, ss_h, ss_v, "%s frame %d SB %r" % (name, i, sb))
        seen += 1
    assert seen


@pytest.mark.parametrize("nj", [0, 1, 64, 65, 128])
def test_heights_small_counts(v9, nj):
    jobs = tiled(1, 1, nj)
    ref = check(v9, jobs, cases.producers(jobs, 1, 1), 1, 1, "%d tiled jobs" % nj)
    if nj:
        assert ref[0] == max(ref) == min(nj, 16) + (nj // 16 - 1 if nj > 16 else 0)      # the chain from job 0 to the last full row's end


@pytest.mark.parametrize("fmt,jcap", [("420", 384), ("444", 768)])
def test_heights_full_jcap(v9, fmt, jcap):
    ss_h, ss_v = cases.FORMATS[fmt]
    jobs = tiled(ss_h, ss_v)
    assert len(jobs) == jcap
    prods = cases.producers(jobs, ss_h, ss_v)
    # a chain across every chunk boundary inside a plane: the first job of a chunk reads the job above it
    for c in range(64, jcap, 64):
        if jobs[c].uy0:
            assert any(d < c for d in prods[c]), "no producer of job %d in an earlier chunk" % c
    ref = check(v9, jobs, prods, ss_h, ss_v, "%s tiled by 4x4" % fmt)
    assert ref[0] == 31


def test_heights_long_lists(v9):
    jobs, big16, big32, four = mixed()
    prods = cases.producers(jobs, 1, 1)
    assert (jobs[big16].ts, len(prods[big16])) == (2, 5)
    assert (jobs[big32].ts, len(prods[big32])) == (3, 17)
    assert (jobs[four].ts, len(prods[four])) == (1, 4)
    assert len(prods[0]) == 0
    ref = check(v9, jobs, prods, 1, 1, "mixed sizes")
    # every producer of the long lists stands above its consumer, the fifth and later ones too
    for j in (big16, big32, four):
        assert all(ref[d] > ref[j] for d in prods[j])


def test_heights_long_list_across_chunks(v9):
    """The jobs of test_heights_long_lists after 50 tiled ones of the chroma planes: the 32x32
    job then lies in the second chunk, with producers in both."""
    pre = [job(1 + (i >= 32), 0, i % 8, (i % 32) // 8, TM) for i in range(50)]
    jobs = pre + mixed()[0]
    prods = cases.producers(jobs, 1, 1)
    assert max(len(s) for s in prods) == 17 and len(jobs) > 64
    j32 = next(j for j, q in enumerate(jobs) if q.ts == 3)
    assert j32 >= 64 and any(d < 64 for d in prods[j32]) and any(d >= 64 for d in prods[j32])
    check(v9, jobs, prods, 1, 1, "mixed sizes behind 50 chroma jobs")


def test_heights_rejects_bad_arguments(v9):
    with pytest.raises(v9.Vp9HipError):
        v9.plan_heights_host(1, 1, [1 << 12 | 1 << 2])        # an 8x8 at an odd unit
    with pytest.raises(v9.Vp9HipError):
        v9.plan_heights_host(1, 1, [0] * 385)                 # more jobs than an SB holds
