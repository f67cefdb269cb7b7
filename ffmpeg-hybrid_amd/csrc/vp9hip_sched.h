/*
 * Launch-list policy of a batch, stated once for the three planners of vp9hip_runtime.cpp: the
 * host planner (stage_host, VP9HIP_HOST_PLAN=1), the static plan of a keyframe batch
 * (build_static_plan) and the device plan (plan_dev, every run of a batch with inter frames):
 * a batch's phases, the fused-phase launch schedule, the k_lfr task table. Host-only plain
 * C++, no HIP types and no context: the callers own the Launch records, the byte accounting
 * and the counter blocks. tests/c/sched_host_check.cpp sweeps it. Internal to libvp9hip.
 */
#ifndef VP9HIP_SCHED_H
#define VP9HIP_SCHED_H
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

// Residuals run inside the fused launches (one intra diagonal ahead) for phases of fewer
// frames than this; wide phases (keyframe batches) keep their separate k_resid launches:
// measured C2 +6.5 % fused, C3 -2 %, C4 -8 %
#define RES_FUSE_MAX_FRAMES 8
// The loop filter of phases of fewer frames than this runs as one row-pipelined k_lfr launch
// (its tail after the fused diagonals); wide phases keep diagonal launches: measured C2
// +8-10 %, C3 -6 % with k_lfr everywhere (its long-lived workgroups crowd the other groups'
// intra wavefronts)
#define LFR_MAX_FRAMES 8
#define PLF_LAG 3   // a fused launch's LF diagonal runs this far behind its intra diagonal (sched_fused_phase)

typedef std::pair<uint32_t, uint32_t> SchedRange;    // (offset, count) of a list part or job range

// Frame dependencies inside a batch: an inter frame follows the frames whose output it
// references, and a frame overwriting a buffer follows every earlier frame that reads or
// writes that buffer. Dependent frames form chains; chains are spread over G stream groups,
// and within a group frames of equal chain position ("phase") are interleaved in every
// launch (a keyframe batch is one phase per group).
struct SchedPhases {
    std::vector<int> pos, grp;          // per frame: chain position, stream group
    int G = 1, maxpos = 0, NP = 0;      // phase id = grp * (maxpos + 1) + pos
    std::vector<char> res_fused;        // per phase: residuals inside the fused launches
    std::vector<char> lvl_ph;           // per phase: intra SBs by dependency level (inter frames)
    int phase(int i) const { return grp[i] * (maxpos + 1) + pos[i]; }
};
// intra[i]: frame i is a keyframe or intra-only; ref_bufs (n x 3) may be null for a batch
// without inter frames (false when an inter frame has none). max_groups: stream groups
// allowed; fuse: fused intra + LF launches; lfr_any: k_lfr at all; level_sched: level phases;
// lf_rows > 1: k_lfr (and levels) for phases of any width.
struct SchedPolicy { int max_groups; bool fuse, lfr_any, level_sched; int lf_rows; };
inline bool sched_batch_phases(int n, const char *intra, const int *out_bufs, const int *ref_bufs,
                               const SchedPolicy &p, SchedPhases &o)
{
    std::vector<int> comp(n);
    o.pos.assign(n, 0);
    for (int i = 0; i < n; i++) comp[i] = i;
    auto find = [&](int x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
    for (int i = 0; i < n; i++) {
        if (!intra[i] && !ref_bufs) return false;
        for (int j = 0; j < i; j++) {
            bool dep = out_bufs[j] == out_bufs[i];
            for (int r = 0; r < 3 && !dep; r++)
                dep = (!intra[i] && ref_bufs[i * 3 + r] == out_bufs[j]) || (!intra[j] && ref_bufs[j * 3 + r] == out_bufs[i]);
            if (dep) { o.pos[i] = std::max(o.pos[i], o.pos[j] + 1); comp[find(i)] = find(j); }
        }
    }
    std::vector<int> roots;
    for (int i = 0; i < n; i++) if (find(i) == i) roots.push_back(i);
    // G groups: as many as allowed, but chains split evenly (unless there are many: 4 GOP
    // chains over 3 streams run 2/1/1 and the pair sets the time)
    const int nroots = (int) roots.size();
    int G = std::max(1, std::min(p.max_groups, nroots));
    while (G > 1 && nroots % G && nroots < 16 * G) G--;
    o.G = G;
    o.maxpos = 0;
    o.grp.resize(n);
    for (int i = 0; i < n; i++) {
        o.grp[i] = (int) (std::lower_bound(roots.begin(), roots.end(), find(i)) - roots.begin()) % G;
        o.maxpos = std::max(o.maxpos, o.pos[i]);
    }
    o.NP = G * (o.maxpos + 1);
    std::vector<int> phase_n(o.NP, 0);
    for (int i = 0; i < n; i++) phase_n[o.phase(i)]++;
    o.res_fused.resize(o.NP);
    for (int ph = 0; ph < o.NP; ph++) o.res_fused[ph] = p.fuse && phase_n[ph] < RES_FUSE_MAX_FRAMES;
    // level-scheduled phases (inter frames of k_lfr phases): MC, all residuals, the intra
    // SBs by dependency level (k_pred), then the whole loop filter as one k_lfr launch
    o.lvl_ph.assign(o.NP, 0);
    if (p.lfr_any && p.level_sched) {
        for (int ph = 0; ph < o.NP; ph++) o.lvl_ph[ph] = p.lf_rows > 1 || phase_n[ph] < LFR_MAX_FRAMES;
        for (int i = 0; i < n; i++)
            if (intra[i]) o.lvl_ph[o.phase(i)] = 0;
        for (int ph = 0; ph < o.NP; ph++) if (o.lvl_ph[ph]) o.res_fused[ph] = false;
    }
    return true;
}

// LF diagonals (of nlfd) that run inside a phase's fused launches. With k_lfr (lfr), LF
// diagonals fuse into the launches the intra wavefront (np diagonals, nres residual
// segments) needs anyway and k_lfr filters the rest; without it, all of them.
inline int sched_fused_nlf(int np, int nres, int nlfd, bool lfr)
{
    const int jlfr = std::max(0, std::max(np, nres - 1) - PLF_LAG);
    return lfr ? std::min(jlfr, nlfd) : nlfd;
}

// Fused schedule of a phase: launch t runs intra diagonal t and LF diagonal t - PLF_LAG.
// LF of SB (x, y) (diagonal x + 2y = j) rewrites pre-LF pixels of SBs
// (x - 1 .. x, y - 1 .. y) that the intra blocks of SBs (x - 1 .. x + 1, y .. y + 1)
// read; those are on intra diagonals <= x_in_tile + y + 2 <= j + 2, i.e. in earlier
// launches. Conversely the intra diagonal t reads SBs on diagonals t - 1, t - 2,
// whose pixels no LF SB of diagonal t - 3 touches (that needs x - x_in_tile + y < 0).
// This is the ordering the reference gets from its pre-LF intra_pred_data row
// (vp9.c:1404-1416), without a second copy.
// The residuals of intra diagonal t + 1 (inverse transforms, incl. inter residuals added
// onto the MC prediction) run in launch t too, so no separate residual pass precedes the
// wavefront: launch -1 holds diagonal 0's alone. nres = 0: no fused residuals (the static
// plan; launch -1 is then empty and not emitted).
// An LF diagonal with no intra or residual partner is a launch of its own.
// intra(t), 0 <= t < np; lf(j), 0 <= j < nlf; res(d, tc), 0 <= d < nres: the (offset, count)
// of intra diagonal t's workgroup list, of LF diagonal j's SB list, of diagonal d's residual
// jobs of tx code tc; outside those bounds a range is (0, 0). Per launch they are called in
// this order, each once, so a planner that builds its lists on demand (the host planner)
// gets the intra list first, then the LF list.
// emit(fused, step, a, b, rr): fused: step = t, a the intra list, b the LF list, rr[5] the
// residual ranges (all zero when there are no jobs); else an LF launch: step = j, a its list.
template <class Intra, class Lf, class Res, class Emit>
inline void sched_fused_phase(int np, int nlf, int nres, Intra &&intra, Lf &&lf, Res &&res, Emit &&emit)
{
    const SchedRange none(0u, 0u);
    const int nt = std::max(std::max(np, nlf ? nlf + PLF_LAG : 0), nres - 1);
    for (int t = -1; t < nt; t++) {
        const SchedRange pv = t >= 0 && t < np ? intra(t) : none;
        const int j = t - PLF_LAG;
        const SchedRange lv = j >= 0 && j < nlf ? lf(j) : none;
        SchedRange rr[5] = { none, none, none, none, none };
        bool any = false;
        for (int tc = 0; t + 1 < nres && tc < 5; tc++) { rr[tc] = res(t + 1, tc); any |= rr[tc].second > 0; }
        if (!any) std::fill(rr, rr + 5, none);
        if (pv.second || any) emit(true, t, pv, lv, rr);
        else if (lv.second) emit(false, j, lv, none, rr);
    }
}

// k_lfr task table of a phase (parsed by k_lfro / k_lfrd): one task per (frame, SB row) of
// the filtered frames, rows-major (row 0 of every frame, then row 1, ...: a task's
// dependency has a lower number, which the kernels' ticket order relies on). j0: the LF
// diagonals x + 2y < j0 ran in earlier (fused) launches, so row r starts at column
// start(r) = max(0, j0 - 2r); a row with no column left has no task. Layout, appended to
// `out`: nt offsets (relative to the table's start), then per task
//   { dep, nc, c0, dep0, id(frame, r, c0) .. id(frame, r, nc - 1) }
// dep: the task of the row above in the same frame, or ~0u; nc: the frame's SB columns; c0:
// the first column filtered here; dep0: the columns of dep's row final before the launch
// (max(0, start(r - 1) - 1), 0 without a dep); id: the LF record of an SB. Returns nt
// (nothing is appended when it is 0). frames: (sb_rows, sb_cols).
template <class Id>
inline uint32_t sched_lfr_tasks(const std::vector<std::pair<int, int>> &frames, int j0, Id &&id, std::vector<uint32_t> &out)
{
    auto start = [&](int r) { return std::max(0, j0 - 2 * r); };
    int maxr = 0;
    for (const auto &f : frames) maxr = std::max(maxr, f.first);
    std::vector<uint32_t> prev(frames.size(), ~0u), offs, recs;    // prev: task of (frame, r - 1)
    for (int r = 0; r < maxr; r++)
        for (size_t f = 0; f < frames.size(); f++) {
            if (r >= frames[f].first) continue;
            const int nc = frames[f].second, c0 = start(r);
            const uint32_t dep = prev[f];
            if (c0 >= nc) { prev[f] = ~0u; continue; }
            prev[f] = (uint32_t) offs.size();
            offs.push_back((uint32_t) recs.size());
            recs.insert(recs.end(), { dep, (uint32_t) nc, (uint32_t) c0, dep != ~0u ? (uint32_t) std::max(0, start(r - 1) - 1) : 0u });
            for (int x = c0; x < nc; x++) recs.push_back(id((int) f, r, x));
        }
    const uint32_t nt = (uint32_t) offs.size();
    for (uint32_t o : offs) out.push_back(o + nt);
    out.insert(out.end(), recs.begin(), recs.end());
    return nt;
}

#endif
