// Property sweep of csrc/vp9hip_sched.h (no device, no Python): the fused-phase launch
// schedule and the k_lfr task table that the host planner, the static plan and the device
// plan share. Small inputs, properties only (no pinned outputs). `make sched_host_check`
// builds it plain and with ASan + UBSan; tests/test_sched_host_check.py runs both.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <vector>

#include "../../ffmpeg-hybrid_amd/csrc/vp9hip_sched.h"

static long g_checks = 0;
#define CHECK(cond, ...) do { g_checks++; if (!(cond)) { fprintf(stderr, "sched_host_check FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
    fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); exit(1); } } while (0)

static uint32_t g_rng = 0x9e3779b9u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

struct Emitted { bool fused; int step; SchedRange a, b, rr[5]; };

// One schedule: np intra steps, nlfd LF diagonals, nres residual segments; empty[] thins them out.
static void check_schedule(int np, int nlfd, int nres, bool lfr, bool thin)
{
    // list sizes (0 = empty step) and distinct offsets, so a part is recognised by its offset
    std::vector<uint32_t> pn(np), ln(nlfd);
    std::vector<std::vector<uint32_t>> rn(nres, std::vector<uint32_t>(5));
    for (auto &v : pn) v = thin && rnd() % 3 == 0 ? 0 : 1 + rnd() % 4;
    for (auto &v : ln) v = thin && rnd() % 3 == 0 ? 0 : 1 + rnd() % 4;
    for (auto &d : rn)
        for (auto &v : d) v = thin && rnd() % 2 == 0 ? 0 : 1 + rnd() % 4;
    const int nlf = sched_fused_nlf(np, nres, nlfd, lfr);
    CHECK(nlf >= 0 && nlf <= nlfd, "nlf %d of %d", nlf, nlfd);
    if (!lfr) CHECK(nlf == nlfd, "without k_lfr every LF diagonal fuses");
    // with k_lfr the fused LF diagonals need no launch beyond the intra / residual ones
    if (lfr && nlf) CHECK(nlf + PLF_LAG <= std::max(np, nres - 1), "nlf %d np %d nres %d", nlf, np, nres);
    std::vector<Emitted> out;
    int calls_i = 0, calls_l = 0;
    sched_fused_phase(np, nlf, nres,
        [&](int t) { CHECK(t >= 0 && t < np, "intra(%d)", t); calls_i++; return SchedRange(1000u + t, pn[t]); },
        [&](int j) { CHECK(j >= 0 && j < nlf, "lf(%d)", j); calls_l++; return SchedRange(2000u + j, ln[j]); },
        [&](int d, int tc) { CHECK(d >= 0 && d < nres && tc >= 0 && tc < 5, "res(%d, %d)", d, tc); return SchedRange(3000u + d * 5 + tc, rn[d][tc]); },
        [&](int fused, int step, SchedRange a, SchedRange b, const SchedRange *rr) {
            Emitted e = { fused != 0, step, a, b, {} };
            for (int k = 0; k < 5; k++) e.rr[k] = rr[k];
            out.push_back(e);
        });
    CHECK(calls_i == np && calls_l == nlf, "each list asked for once: %d/%d %d/%d", calls_i, np, calls_l, nlf);
    std::vector<int> at_i(np, -1), at_l(nlfd, -1), at_r(nres, -1);    // launch index of each part
    for (size_t k = 0; k < out.size(); k++) {
        const Emitted &e = out[k];
        bool res = false;
        for (int tc = 0; tc < 5; tc++) res |= e.rr[tc].second > 0;
        if (!e.fused) {                                    // an LF diagonal on its own
            CHECK(e.a.second > 0 && !e.b.second && !res, "LF launch %zu", k);
            const int j = e.step;
            CHECK(j >= 0 && j < nlf && e.a == SchedRange(2000u + j, ln[j]) && at_l[j] < 0, "LF launch %zu diagonal %d", k, j);
            at_l[j] = (int) k;
            // it had no partner: intra step j + PLF_LAG and the residuals of the next one are empty
            const int t = j + PLF_LAG;
            CHECK(t >= np || !pn[t], "LF diagonal %d alone beside intra step %d", j, t);
            continue;
        }
        CHECK(e.a.second || res, "launch %zu is empty", k);     // no launch is empty
        const int t = e.step;
        if (e.a.second) {
            CHECK(t >= 0 && t < np && e.a == SchedRange(1000u + t, pn[t]) && at_i[t] < 0, "intra step of launch %zu", k);
            at_i[t] = (int) k;
        }
        if (e.b.second) {
            const int j = t - PLF_LAG;
            CHECK(j >= 0 && j < nlf && e.b == SchedRange(2000u + j, ln[j]) && at_l[j] < 0, "LF part of launch %zu", k);
            at_l[j] = (int) k;
        }
        if (res) {
            const int d = t + 1;
            CHECK(d >= 0 && d < nres && at_r[d] < 0, "residuals of launch %zu", k);
            for (int tc = 0; tc < 5; tc++) CHECK(e.rr[tc] == SchedRange(3000u + d * 5 + tc, rn[d][tc]), "residual range %d of launch %zu", tc, k);
            at_r[d] = (int) k;
        } else {
            for (int tc = 0; tc < 5; tc++) CHECK(e.rr[tc] == SchedRange(0u, 0u), "no residuals: zero ranges");
        }
        if (k) CHECK(out[k - 1].step + (out[k - 1].fused ? 0 : PLF_LAG) < t, "launches in step order");
    }
    // every non-empty intra step in exactly one launch (at step t: checked above)
    for (int t = 0; t < np; t++) CHECK((at_i[t] >= 0) == (pn[t] > 0), "intra step %d", t);
    // every non-empty LF diagonal j < nlf exactly once, after the intra steps <= j + 2; none beyond nlf
    for (int j = 0; j < nlfd; j++) {
        CHECK((at_l[j] >= 0) == (j < nlf && ln[j] > 0), "LF diagonal %d (nlf %d)", j, nlf);
        for (int t = 0; at_l[j] >= 0 && t < np && t <= j + 2; t++)
            CHECK(at_i[t] < at_l[j], "LF diagonal %d in launch %d, intra step %d in launch %d", j, at_l[j], t, at_i[t]);
    }
    // the residuals of diagonal d exactly once, in a launch before the one holding intra step d
    for (int d = 0; d < nres; d++) {
        bool any = false;
        for (int tc = 0; tc < 5; tc++) any |= rn[d][tc] > 0;
        CHECK((at_r[d] >= 0) == any, "residuals of diagonal %d", d);
        if (any && d < np && at_i[d] >= 0) CHECK(at_r[d] < at_i[d], "residuals of diagonal %d after its intra step", d);
    }
}

// One table over `frames`, parsed back the way k_lfro / k_lfrd read it.
static void check_table(const std::vector<std::pair<int, int>> &frames, int j0)
{
    std::vector<uint32_t> out(3, 0xabcdu);                 // the table is appended
    auto id = [](int f, int r, int c) { return (uint32_t) (f << 16 | r << 8 | c); };
    std::map<uint32_t, int> asked;
    const uint32_t nt = sched_lfr_tasks(frames, j0, [&](int f, int r, int c) { asked[id(f, r, c)]++; return id(f, r, c); }, out);
    CHECK(out[0] == 0xabcdu && out[2] == 0xabcdu, "the words before the table are kept");
    if (!nt) CHECK(out.size() == 3, "an empty table appends nothing");
    const uint32_t *T = out.data() + 3;
    const size_t words = out.size() - 3;
    auto start = [&](int r) { return std::max(0, j0 - 2 * r); };
    std::map<uint32_t, int> seen;
    std::vector<std::vector<uint32_t>> task_of(frames.size());          // per frame, row: its task or ~0u
    for (size_t f = 0; f < frames.size(); f++) task_of[f].assign(frames[f].first, ~0u);
    size_t expect = nt;                                    // records are back to back after the offsets
    int last_row = -1, last_frame = -1;
    for (uint32_t k = 0; k < nt; k++) {
        CHECK(T[k] == expect && T[k] + 4 <= words, "task %u: offset %u, expected %zu (rebased by %u tasks)", k, T[k], expect, nt);
        const uint32_t *R = T + T[k];
        const uint32_t dep = R[0], nc = R[1], c0 = R[2];
        CHECK(c0 < nc && T[k] + 4 + (nc - c0) <= words, "task %u: columns %u..%u", k, c0, nc);
        const int f = (int) (R[4] >> 16), r = (int) (R[4] >> 8 & 0xff);
        CHECK(f < (int) frames.size() && r < frames[f].first && (int) nc == frames[f].second, "task %u: frame %d row %d", k, f, r);
        CHECK((int) c0 == start(r), "task %u: row %d starts at %u, not %d", k, r, c0, start(r));
        for (uint32_t x = c0; x < nc; x++) { CHECK(R[4 + x - c0] == id(f, r, (int) x), "task %u column %u", k, x); seen[R[4 + x - c0]]++; }
        // rows-major across frames
        CHECK(r > last_row || (r == last_row && f > last_frame), "task %u: (row %d, frame %d) after (%d, %d)", k, r, f, last_row, last_frame);
        last_row = r; last_frame = f;
        CHECK(task_of[f][r] == ~0u, "task %u: a second task of frame %d row %d", k, f, r);
        task_of[f][r] = k;
        // dep: the task of the row above in the same frame, or ~0u; it has a lower number
        const uint32_t above = r ? task_of[f][r - 1] : ~0u;
        CHECK(dep == above && (dep == ~0u || dep < k), "task %u: dep %u, row above %u", k, dep, above);
        CHECK(R[3] == (dep != ~0u ? (uint32_t) std::max(0, start(r - 1) - 1) : 0u), "task %u: word 3 = %u", k, R[3]);
        expect += 4 + (nc - c0);
    }
    CHECK(expect == words, "table of %zu words, %zu parsed", words, expect);
    // every cell with col >= max(0, j0 - 2 row) exactly once, and no other cell
    size_t cells = 0;
    for (size_t f = 0; f < frames.size(); f++)
        for (int r = 0; r < frames[f].first; r++) {
            CHECK((task_of[f][r] != ~0u) == (start(r) < frames[f].second), "frame %zu row %d: task %u", f, r, task_of[f][r]);
            for (int c = 0; c < frames[f].second; c++) {
                const bool in = c >= start(r);
                CHECK(seen[id((int) f, r, c)] == (in ? 1 : 0) && asked[id((int) f, r, c)] == (in ? 1 : 0), "cell (%zu, %d, %d)", f, r, c);
                cells += in;
            }
        }
    size_t total = 0;
    for (auto &kv : seen) total += kv.second;
    CHECK(total == cells, "%zu records for %zu cells", total, cells);
}

int main()
{
    // schedule: np 0..6, LF diagonals 0..9, nres 0..7, k_lfr on and off, full and randomly thinned steps
    for (int np = 0; np <= 6; np++)
        for (int nlfd = 0; nlfd <= 9; nlfd++)
            for (int nres = 0; nres <= 7; nres++)
                for (int lfr = 0; lfr < 2; lfr++) {
                    check_schedule(np, nlfd, nres, lfr != 0, false);
                    for (int rep = 0; rep < 8; rep++) check_schedule(np, nlfd, nres, lfr != 0, true);
                }
    // table: one frame, and every pair of frames, of 1..5 rows by 1..4 columns, j0 0..6
    for (int j0 = 0; j0 <= 6; j0++)
        for (int r1 = 1; r1 <= 5; r1++)
            for (int c1 = 1; c1 <= 4; c1++) {
                check_table({ { r1, c1 } }, j0);
                for (int r2 = 1; r2 <= 5; r2++)
                    for (int c2 = 1; c2 <= 4; c2++) check_table({ { r1, c1 }, { r2, c2 } }, j0);
            }
    check_table({}, 3);
    {   // 1 column by 5 rows, j0 = 2: row 0 has no task, row 1 is task 0 and has no dep
        std::vector<uint32_t> t;
        const uint32_t nt = sched_lfr_tasks({ { 5, 1 } }, 2, [](int, int r, int) { return (uint32_t) r; }, t);
        CHECK(nt == 4 && t[t[0]] == ~0u && t[t[0] + 2] == 0 && t[t[0] + 4] == 1, "5x1, j0 2: %u tasks, dep %u", nt, t[t[0]]);
        CHECK(t[t[1]] == 0 && t[t[1] + 3] == 0, "5x1, j0 2: row 2 follows task 0, none of its columns final");
    }
    printf("sched_host_check OK (%ld checks)\n", g_checks);
    return 0;
}
