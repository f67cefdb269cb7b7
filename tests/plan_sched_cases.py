"""Cases of the intra pass schedule tests (not a test module): tiny frames whose superblocks'
intra jobs, in decode order, come from the packets alone (synth_walk.intra_jobs), the producers of
every job derived from geometry in Python, and the census the cases must meet.

The device planner (k_pjplan, csrc/vp9hip_plan.hip) list-schedules the intra jobs of one SB into
passes of at most 64 lanes. A job is ready when every 4x4 unit it reads in its own SB plane
belongs to a job of an earlier pass; it tests that with two 16-bit masks per job (the units of
its top run and of its left run that an earlier job covers, pl_deps of csrc/vp9hip_planlogic.h)
against the done bits of that row and column. vp9hip_plan_sched_host restates the whole schedule
in scalar code; tests/test_plan_sched_host.py checks its masks against producers() below and
its passes for validity on the CPU, tests/test_gpu_plan_sched.py the device's records against it.
"""
import collections
import functools

import synth_walk

SIZES = [(64, 64), (80, 80), (88, 88), (128, 64)]
FORMATS = {"420": (1, 1), "422": (1, 0), "440": (0, 1), "444": (0, 0)}
SLOT_OF = [0, 1, 9, 2, 3, 4, 5, 6, 7, 8, 10, 11, 12, 13, 14]        # PJob mode slot of a final mode
P_INTRA = 0.5
GOP_P = 3
LOSSLESS = {"lossless": 1, "q_idx": 0}

Job = collections.namedtuple("Job", "p ts ux0 uy0 needs trx word")


def sb_jobs(pkt):
    """{(sbx, sby): [Job, ...]} of one packet: the intra tx blocks of each SB in decode order.
    needs = (left, top, top-left, top-right) of the final mode; trx: the 4x4 top-right lies
    inside the block; word: the job word vp9hip_plan_sched_host takes."""
    out = collections.OrderedDict()
    for t in synth_walk.intra_jobs(pkt):
        b = t.block
        sh, sv = (pkt.ss_h, pkt.ss_v) if t.plane else (0, 0)
        ux0 = (((b.col & 7) * 2) >> sh) + t.x
        uy0 = (((b.row & 7) * 2) >> sv) + t.y
        needs = synth_walk.EDGES[t.final]
        trx = int(t.tx == 0 and t.have_right and needs[3])
        word = t.plane | t.tx << 2 | SLOT_OF[t.final] << 8 | ux0 << 12 | uy0 << 16 | trx << 30
        out.setdefault((b.col >> 3, b.row >> 3), []).append(Job(t.plane, t.tx, ux0, uy0, needs, trx, word))
    return out


def cover(jobs, ss_h, ss_v):
    """{(plane, ux, uy): job index} of the SB's 4x4 units, clipped to the plane's units."""
    m = {}
    for j, q in enumerate(jobs):
        units, unitsv = (16 >> ss_h, 16 >> ss_v) if q.p else (16, 16)
        n = 1 << q.ts
        for v in range(q.uy0, min(q.uy0 + n, unitsv)):
            for u in range(q.ux0, min(q.ux0 + n, units)):
                assert (q.p, u, v) not in m, "two intra jobs cover one unit"
                m[(q.p, u, v)] = j
    return m


def reads(q, ss_h, ss_v):
    """The units of its own SB plane job q's final mode reads: the top row from the top-left unit
    (if read) to the top-right unit (if read and inside the block, else the row stops at the
    job's width), and the left column (vp9recon.c:71-221: edges outside the SB are other SBs')."""
    units, unitsv = (16 >> ss_h, 16 >> ss_v) if q.p else (16, 16)
    left, top, topleft, _ = q.needs
    n = 1 << q.ts
    out = []
    if q.uy0 > 0:
        u0 = q.ux0 - 1 if topleft else q.ux0
        u1 = q.ux0 + n + q.trx if top else q.ux0
        out += [(u, q.uy0 - 1) for u in range(max(u0, 0), min(u1, units))]
    if q.ux0 > 0 and left:
        out += [(q.ux0 - 1, v) for v in range(q.uy0, min(q.uy0 + n, unitsv))]
    return out


def producers(jobs, ss_h, ss_v):
    """Per job the set of earlier jobs of the SB whose pixels it reads."""
    m = cover(jobs, ss_h, ss_v)
    out = []
    for j, q in enumerate(jobs):
        s = set()
        for u, v in reads(q, ss_h, ss_v):
            d = m.get((q.p, u, v))
            if d is not None and d < j:
                s.add(d)
        out.append(s)
    return out


def mask_producers(jobs, masks, ss_h, ss_v):
    """Per job the set of jobs covering the units of its masks (bit u: unit u of row uy0 - 1,
    bit 16 + v: unit v of column ux0 - 1). Every masked unit must be covered."""
    m = cover(jobs, ss_h, ss_v)
    out = []
    for q, mk in zip(jobs, masks):
        mk = int(mk)
        s = set()
        for b in range(32):
            if mk >> b & 1:
                s.add(m[(q.p, b, q.uy0 - 1) if b < 16 else (q.p, q.ux0 - 1, b - 16)])
        out.append(s)
    return out


def check_schedule(jobs, prods, order, passes):
    """The pass records of one SB are a valid schedule: every job exactly once, a pass's jobs by
    size 32, 16, 8, 4 with the counts of its word, at most 64 lanes, every producer in a strictly
    earlier pass. Returns the pass of each job."""
    n = len(jobs)
    assert sorted(int(x) for x in order[:n]) == list(range(n)), "not every job exactly once"
    pass_of = [None] * n
    at = 0
    for k, w in enumerate(int(x) for x in passes):
        assert w >> 14 == at, "pass %d starts at %d, its word says %d" % (k, at, w >> 14)
        cnt = [w >> 9 & 31, w >> 5 & 15, w >> 2 & 7, w & 3]
        assert sum(cnt) > 0 and sum(c * (4 << ts) for ts, c in enumerate(cnt)) <= 64, "pass %d: %r" % (k, cnt)
        for ts in (3, 2, 1, 0):
            for _ in range(cnt[ts]):
                j = int(order[at])
                assert jobs[j].ts == ts, "pass %d position %d: size %d, expected %d" % (k, at, jobs[j].ts, ts)
                pass_of[j] = k
                at += 1
    assert at == n
    for j in range(n):
        for d in prods[j]:
            assert pass_of[d] < pass_of[j], "job %d (pass %d) reads job %d (pass %d)" % (j, pass_of[j], d, pass_of[d])
    return pass_of


# ---- the cases: name -> (format, size, bits, kind, extra synth parameters)
def _cases():
    c = collections.OrderedDict()
    for fmt in FORMATS:
        for w, h in SIZES:
            for kind in ("key", "gop"):
                c["%s-%s-%dx%d" % (kind, fmt, w, h)] = (fmt, (w, h), 8, kind, {})
    c["key-420-88x88-10bit"] = ("420", (88, 88), 10, "key", {})
    c["key-420-64x64-lossless"] = ("420", (64, 64), 8, "key", LOSSLESS)
    c["key-444-64x64-lossless"] = ("444", (64, 64), 8, "key", LOSSLESS)
    return c


CASES = _cases()
KEYS_PER_CASE = 6


@functools.lru_cache(maxsize=None)
def frames(v9, name):
    """The case's frames in batch order, [(SynthFrame, refs or None), ...]: keyframes, or chains
    of a keyframe and GOP_P P frames with p_intra 0.5 (each reads the frame before it as LAST and
    its keyframe as GOLDEN and ALTREF); edge_large alternates frame by frame (chain by chain)."""
    fmt, (w, h), bpp, kind, extra = CASES[name]
    ss_h, ss_v = FORMATS[fmt]
    seed = 0x5c4ed000 + 0x100 * list(CASES).index(name)
    fl = []
    if kind == "key":
        for i in range(KEYS_PER_CASE):
            fl.append((v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + i, ss_h=ss_h, ss_v=ss_v, edge_large=i & 1,
                                                     **extra)), None))
    else:
        for ch in range(2):
            k = len(fl)
            common = dict(ss_h=ss_h, ss_v=ss_v, edge_large=ch & 1, **extra)
            fl.append((v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 16 * ch, **common)), None))
            for i in range(k + 1, k + 1 + GOP_P):
                fl.append((v9.SynthFrame(v9.synth_params(w, h, bpp, seed=seed + 16 * ch + i - k, inter=1, p_intra=P_INTRA,
                                                         **common)), (i - 1, k, k)))
    return fl


@functools.lru_cache(maxsize=None)
def case_sbs(v9, name):
    """[(frame index, (sbx, sby), jobs, producers)] over the SBs of the case that hold intra jobs."""
    ss_h, ss_v = FORMATS[CASES[name][0]]
    out = []
    for i, (f, r) in enumerate(frames(v9, name)):
        for sb, jobs in sb_jobs(f.pkt).items():
            out.append((i, sb, jobs, producers(jobs, ss_h, ss_v)))
    return out


CENSUS = ["an SB with more than 256 intra jobs", "a job with more than four distinct producers",
          "an SB the frame edge cuts", "an SB with uncovered units between intra jobs", "a 4x4 with trx",
          "a 4:4:4 SB using more than six chunks of 64 jobs"]


@functools.lru_cache(maxsize=None)
def census(v9):
    """Counter over CENSUS of the SBs (jobs, for the second and fifth item) of all cases."""
    c = collections.Counter()
    for name, (fmt, (w, h), bpp, kind, extra) in CASES.items():
        ss_h, ss_v = FORMATS[fmt]
        for i, (sbx, sby), jobs, prods in case_sbs(v9, name):
            c[CENSUS[0]] += len(jobs) > 256
            c[CENSUS[1]] += sum(len(s) > 4 for s in prods)
            cut = sbx * 64 + 64 > w or sby * 64 + 64 > h
            c[CENSUS[2]] += cut
            m = cover(jobs, ss_h, ss_v)
            # a whole SB of an inter frame in which an intra job reads a unit no intra job covers
            inter = frames(v9, name)[i][1] is not None
            c[CENSUS[3]] += inter and not cut and any((q.p, u, v) not in m for q in jobs for u, v in reads(q, ss_h, ss_v))
            c[CENSUS[4]] += sum(q.trx for q in jobs)
            c[CENSUS[5]] += fmt == "444" and len(jobs) > 384
    return c


def check_census(v9):
    c = census(v9)
    missing = [k for k in CENSUS if not c[k]]
    assert not missing, "the cases do not draw: %s" % "; ".join(missing)
