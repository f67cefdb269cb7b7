"""CPU check of the device planner's pass loop and emit (plan_sb of csrc/vp9hip_plan.hip) through
vp9hip_plan_emit_host, which runs the kernel's own routines (csrc/vp9hip_planlogic.h: the packed
take scan and its fields, the rank inside the size class, the packed done words, the pass-word
scan and the positions' index arithmetic) with a loop over 64 slots in place of the wave's lanes.

The reference is vp9hip_plan_sched_host, the scalar restatement of the schedule, which shares
none of these routines: the order of the jobs, every pass word and the pass count must be equal

  - on every SB of every case of tests/plan_sched_cases.py, and
  - on job lists built here: 0, 1, 63, 64, 65 and 128 jobs, SBs tiled by 4x4 jobs in all planes
    (384 jobs at 4:2:0, 768 at 4:4:4), a chain in which each job waits for the one before it
    (passes of one job), and mixes of 32x32, 16x16, 8x8 and 4x4 jobs.

What the cases must contain is asserted from the restatement's own output (test_conditions): a
pass with jobs of one size class from two different chunks of the priority order, a pass with all
four classes, a pass that fills exactly 64 lanes, and a pass in which a ready job did not fit
and a smaller job of a later chunk was taken.

Not met, and why: an SB with more than 64 passes, and so a chain with npass > 64. A job reads
units to its left, above it and above it to the right only, so along a chain of 4x4 jobs in one
plane the row never decreases and the column decreases only with a step down: at most 15 steps
down and 15 + 15 to the right, 46 jobs (chain() builds exactly that chain: 46 passes of one job),
and the chains of different planes run side by side, since no job waits for another plane. Passes
that the 64 lanes limit hold 16 4x4 jobs, so the 768 jobs of a 4:4:4 SB tiled by 4x4 jobs need 48
passes and take 53 with the ramps of the TM wavefront; larger jobs waste lanes of a pass but cover
their area with fewer lanes. The restatement gives no SB of the cases or of the lists here more
than 53 passes (MOST_PASSES, asserted), so the carry of the pass-word scan across groups of 64
passes is covered by its routine (pl_pass_first) only, not by a schedule.
"""
import numpy as np
import pytest

import plan_sched_cases as cases
from test_plan_heights_host import DC128, H, job, mixed, tiled

D45 = 2                       # PJob slot of D45: reads the top row and the top-right unit


def chain():
    """46 luma 4x4 jobs, each reading the one before it: row 0 left to right (H), then down the
    right edge by turns: a step down and to the left (D45 with its top-right unit inside the
    block, so it reads the job above it to the right), then one to the right again (H)."""
    jobs = [job(0, 0, u, 0, H if u else DC128) for u in range(16)]
    u, v = 15, 0
    while v < 15:
        v += 1
        u -= 1
        jobs.append(job(0, 0, u, v, D45, trx=1))              # reads (u, v - 1): no job, and (u + 1, v - 1)
        u += 1
        jobs.append(job(0, 0, u, v, H))                       # reads (u - 1, v)
    return jobs


def mixed_sizes(ss_h, ss_v):
    """All four sizes without producers (DC_128), luma then chroma: two 32x32, four 16x16, eight
    8x8 and 4x4 jobs over the rest of the SB, largest first in decode order and in every plane, so
    the first passes hold several classes and the lanes run out in the middle of a chunk."""
    out = []
    for p in range(3):
        w, h = (16 >> ss_h, 16 >> ss_v) if p else (16, 16)
        taken = set()

        def put(ts, u, v):
            n = 1 << ts
            if u + n <= w and v + n <= h and not any((x, y) in taken for x in range(u, u + n) for y in range(v, v + n)):
                taken.update((x, y) for x in range(u, u + n) for y in range(v, v + n))
                out.append(job(p, ts, u, v, DC128))
        put(3, 0, 0)
        for u, v in ((8, 0), (12, 0), (8, 4), (0, 8)):
            put(2, u, v)
        for u, v in ((12, 4), (14, 4), (12, 6), (14, 6), (4, 8), (6, 8)):
            put(1, u, v)
        for v in range(h):
            for u in range(w):
                put(0, u, v)
    return out


def interleaved():
    """Luma jobs without producers in the decode order 16x16, 4x4, 4x4, 4x4, ...: every height is
    1, so the priority order is the decode order, and a pass's 16x16 jobs come from more than one
    chunk once the first chunks' small jobs are gone."""
    big = [(u, v) for v in range(0, 8, 4) for u in range(0, 16, 4)]
    small = [(u, v) for v in range(8, 16) for u in range(16)]
    out = []
    for i, (u, v) in enumerate(big):
        out.append(job(0, 2, u, v, DC128))
        out += [job(0, 0, x, y, DC128) for x, y in small[i * 16:(i + 1) * 16]]
    return out + [job(p, 0, u, v, DC128) for p in (1, 2) for v in range(8) for u in range(8)]


def one_of_each():
    """Luma jobs without producers: 32x32, 16x16, 8x8, 4x4 and one more 4x4 (64 lanes), then more
    of each size."""
    first = [job(0, 3, 0, 0, DC128), job(0, 2, 8, 0, DC128), job(0, 1, 12, 0, DC128), job(0, 0, 14, 0, DC128),
             job(0, 0, 15, 0, DC128)]
    rest = [job(0, 2, 8, 4, DC128), job(0, 1, 12, 2, DC128), job(0, 1, 12, 4, DC128), job(0, 0, 14, 1, DC128),
            job(0, 0, 15, 1, DC128), job(0, 3, 0, 8, DC128)]
    return first + rest


BUILT = {
    "tiled-0": lambda: (tiled(1, 1, 0), 1, 1), "tiled-1": lambda: (tiled(1, 1, 1), 1, 1),
    "tiled-63": lambda: (tiled(1, 1, 63), 1, 1), "tiled-64": lambda: (tiled(1, 1, 64), 1, 1),
    "tiled-65": lambda: (tiled(1, 1, 65), 1, 1), "tiled-128": lambda: (tiled(1, 1, 128), 1, 1),
    "tiled-420": lambda: (tiled(1, 1), 1, 1), "tiled-444": lambda: (tiled(0, 0), 0, 0),
    "chain": lambda: (chain(), 1, 1),
    "long-lists": lambda: (mixed()[0], 1, 1),
    "mixed-420": lambda: (mixed_sizes(1, 1), 1, 1), "mixed-444": lambda: (mixed_sizes(0, 0), 0, 0),
    "interleaved": lambda: (interleaved(), 1, 1), "one-of-each": lambda: (one_of_each(), 1, 1),
}
MOST_PASSES = 53


def check(v9, jobs, ss_h, ss_v, what):
    """The emit's order, pass words and counts against the restatement's. Returns the
    restatement's (order, passes)."""
    words = [q.word for q in jobs]
    order, passes, _ = v9.plan_sched_host(ss_h, ss_v, words)
    got_order, got_passes, njobs = v9.plan_emit_host(ss_h, ss_v, words)
    assert (njobs, len(got_passes)) == (len(jobs), len(passes)), "%s: %d jobs in %d passes, restatement %d in %d" % (
        what, njobs, len(got_passes), len(jobs), len(passes))
    bad = np.nonzero(got_passes != passes)[0]
    assert not len(bad), "%s: pass %d is %#x, restatement %#x" % (what, bad[0], got_passes[bad[0]], passes[bad[0]])
    bad = np.nonzero(got_order != order)[0]
    assert not len(bad), "%s: position %d holds job %d, restatement %d (%d of %d differ)" % (
        what, bad[0], got_order[bad[0]], order[bad[0]], len(bad), len(jobs))
    return order, passes


@pytest.mark.parametrize("name", list(cases.CASES))
def test_emit_of_cases(v9, name):
    ss_h, ss_v = cases.FORMATS[cases.CASES[name][0]]
    seen = 0
    for i, sb, jobs, prods in cases.case_sbs(v9, name):
        check(v9, jobs, ss_h, ss_v, "%s frame %d SB %r" % (name, i, sb))
        seen += 1
    assert seen


@pytest.mark.parametrize("name", list(BUILT))
def test_emit_of_built_lists(v9, name):
    jobs, ss_h, ss_v = BUILT[name]()
    prods = cases.producers(jobs, ss_h, ss_v)
    order, passes = check(v9, jobs, ss_h, ss_v, name)
    cases.check_schedule(jobs, prods, order, passes)
    if name == "chain":
        assert len(jobs) == 46 and all(j - 1 in prods[j] for j in range(1, len(jobs)))
        assert len(passes) == len(jobs) and all(int(w) & 0x3fff == 1 << 9 for w in passes)      # one 4x4 job each


def shapes(v9, jobs, ss_h, ss_v):
    """What the restatement's schedule of one SB holds of the conditions ({name: 1}), and its
    pass count ("passes")."""
    n = len(jobs)
    if not n:
        return {"passes": 0}
    prods = cases.producers(jobs, ss_h, ss_v)
    order, passes, _ = v9.plan_sched_host(ss_h, ss_v, [q.word for q in jobs])
    pass_of = cases.check_schedule(jobs, prods, order, passes)
    hgt = np.minimum(v9.plan_heights_host(ss_h, ss_v, [q.word for q in jobs]).astype(np.int64), 63)
    prio = sorted(range(n), key=lambda j: (-hgt[j], j))
    chunk = {j: pos // 64 for pos, j in enumerate(prio)}
    found = {"passes": len(passes)}
    by_pass = [[] for _ in passes]
    for j in range(n):
        by_pass[pass_of[j]].append(j)
    for k, (w, taken) in enumerate(zip((int(x) for x in passes), by_pass)):
        cnt = [w >> 9 & 31, w >> 5 & 15, w >> 2 & 7, w & 3]
        if all(cnt):
            found["all four classes"] = 1
        if sum(c * (4 << ts) for ts, c in enumerate(cnt)) == 64:
            found["exactly 64 lanes"] = 1
        if any(len({chunk[j] for j in taken if jobs[j].ts == ts}) > 1 for ts in range(4)):
            found["one class from two chunks"] = 1
        # a job ready for this pass that a later pass took, and a smaller job of a later chunk in this pass
        for j in range(n):
            if pass_of[j] > k and all(pass_of[d] < k for d in prods[j]) and \
                    any(chunk[t] > chunk[j] and jobs[t].ts < jobs[j].ts for t in taken):
                found["a ready job did not fit, a later chunk's smaller job was taken"] = 1
                break
    return found


CONDITIONS = ["one class from two chunks", "all four classes", "exactly 64 lanes",
              "a ready job did not fit, a later chunk's smaller job was taken"]


def test_conditions(v9):
    """The cases above contain every shape the emit can get wrong (conditions, not measurements)."""
    found, most = set(), 0
    lists = [BUILT[name]() for name in BUILT]
    for name in cases.CASES:
        ss_h, ss_v = cases.FORMATS[cases.CASES[name][0]]
        lists += [(jobs, ss_h, ss_v) for i, sb, jobs, prods in cases.case_sbs(v9, name)]
    for jobs, ss_h, ss_v in lists:
        got = shapes(v9, jobs, ss_h, ss_v)
        most = max(most, got.pop("passes"))
        found |= set(got)
    assert most == MOST_PASSES, "the longest schedule has %d passes (see the docstring)" % most
    missing = [c for c in CONDITIONS if c not in found]
    assert not missing, "no case with: %s" % "; ".join(missing)


def test_emit_rejects_bad_arguments(v9):
    with pytest.raises(v9.Vp9HipError):
        v9.plan_emit_host(1, 1, [1 << 12 | 1 << 2])           # an 8x8 at an odd unit
    with pytest.raises(v9.Vp9HipError):
        v9.plan_emit_host(1, 1, [0] * 385)                    # more jobs than an SB holds
