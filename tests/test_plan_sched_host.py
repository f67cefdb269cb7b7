"""CPU check of the intra pass schedule's readiness masks and of its host restatement.

For every intra job of the cases' packets (tests/plan_sched_cases.py) two producer sets must
agree: the jobs covering the units of the job's masks (pl_deps of csrc/vp9hip_planlogic.h, the
function k_pjplan runs, here through vp9hip_plan_sched_host) and the set derived in Python from
the job's geometry and the edges its final mode reads. The restatement's passes must be a valid
schedule (every job once, producers strictly earlier, at most 64 lanes, sizes 32 to 4 inside a
pass), no shorter than the host planner's dependency levels (plan_stats "levels"), and the cases
must draw every item of the census the GPU test relies on.
"""
import pytest

import plan_sched_cases as cases


def test_census(v9):
    cases.check_census(v9)


@pytest.mark.parametrize("name", list(cases.CASES))
def test_masks_and_restatement(v9, name):
    ss_h, ss_v = cases.FORMATS[cases.CASES[name][0]]
    npass, njobs = {}, {}
    for i, sb, jobs, prods in cases.case_sbs(v9, name):
        order, passes, masks = v9.plan_sched_host(ss_h, ss_v, [q.word for q in jobs])
        got = cases.mask_producers(jobs, masks, ss_h, ss_v)
        for j, (a, b) in enumerate(zip(got, prods)):
            assert a == b, "%s frame %d SB %r job %d %r: masks name %r, geometry %r" % (name, i, sb, j, jobs[j][:6],
                                                                                      sorted(a), sorted(b))
        cases.check_schedule(jobs, prods, order, passes)
        npass[i] = npass.get(i, 0) + len(passes)
        njobs[i] = njobs.get(i, 0) + len(jobs)
    for i, (f, r) in enumerate(cases.frames(v9, name)):
        st = v9.plan_stats(f)
        assert int(st["pjobs"]) == njobs.get(i, 0), "%s frame %d: the walker and the host planner count jobs differently" % (name, i)
        assert npass.get(i, 0) >= int(st["levels"]), "%s frame %d: fewer passes than dependency levels" % (name, i)


def test_restatement_rejects_bad_arguments(v9):
    with pytest.raises(v9.Vp9HipError):
        v9.plan_sched_host(1, 1, [1 << 12 | 1 << 2])          # an 8x8 at an odd unit
    with pytest.raises(v9.Vp9HipError):
        v9.plan_sched_host(1, 1, [3])                         # plane 3
