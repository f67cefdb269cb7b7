/* vp9hip_motion_acc_host at its edges: the accumulated-motion recurrence of include/vp9hip.h on
 * the host, where the sanitizer builds can watch it (make -C ffmpeg-hybrid_amd/csrc
 * motion_acc_host_check; built without -fwrapv, so a signed overflow is a finding). Extreme
 * vectors, the 2 x 2 and 4096 x 4096 grids, NULL parents with each end code, the wrap and
 * saturation cases; `out` is an exact-size heap block (ASan) with guard bytes around a second
 * copy (every build). No device, no Python. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

#define GUARD 64

static int fails;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "motion_acc_host_check: %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }
/* floor(v / 32), spelled without a shift of a negative value */
static int fl32(int v) { int q = v / 32; return (v % 32 != 0 && v < 0) ? q - 1 : q; }

/* Run one frame twice: into an exact-size block and into a guarded one; returns the first. */
static vp9hip_acc_cell *run(const int16_t *mv, const uint8_t *info, int gw, int gh, uint32_t serial,
                            const vp9hip_acc_cell *const par[3], const int pend[3], int twice)
{
    const size_t bytes = (size_t) gw * gh * sizeof(vp9hip_acc_cell);
    vp9hip_acc_cell *out = malloc(bytes);
    memset(out, 0x5a, bytes);
    CHECK(vp9hip_motion_acc_host(mv, info, gw, gh, serial, par, pend, out) == 0);
    if (twice) {
        uint8_t *g = malloc(bytes + 2 * GUARD);
        memset(g, 0xa5, bytes + 2 * GUARD);
        CHECK(vp9hip_motion_acc_host(mv, info, gw, gh, serial, par, pend, (vp9hip_acc_cell *) (g + GUARD)) == 0);
        for (int i = 0; i < GUARD; i++) CHECK(g[i] == 0xa5 && g[GUARD + bytes + i] == 0xa5);
        CHECK(!memcmp(g + GUARD, out, bytes));
        free(g);
    }
    return out;
}

static void set_cell(int16_t *mv, uint8_t *info, size_t cell, int i0, int i1, int mx, int my)
{
    info[cell * 4] = (uint8_t) i0; info[cell * 4 + 1] = (uint8_t) i1; info[cell * 4 + 2] = 0; info[cell * 4 + 3] = 0;
    mv[cell * 4] = (int16_t) mx; mv[cell * 4 + 1] = (int16_t) my;
    mv[cell * 4 + 2] = 0x7abc; mv[cell * 4 + 3] = -0x7abc;     /* the second vector: never read */
}

static int same(const vp9hip_acc_cell *a, int32_t dx, int32_t dy, uint32_t root, int hops, int end)
{
    return a->dx == dx && a->dy == dy && a->root == root && a->hops == hops && a->end == end && a->pad == 0;
}

int main(void)
{
    CHECK(sizeof(vp9hip_acc_cell) == 16);
    static const int ext[] = { 32767, -32767, -32768, 0, 1, -1, 15, 16, -16, -17 };
    const int next = (int) (sizeof(ext) / sizeof(ext[0]));
    const int none[3] = { VP9HIP_ACC_END_NOFIELD, VP9HIP_ACC_END_SCALED, VP9HIP_ACC_END_NOFIELD };

    /* the 2 x 2 grid: every pair of extreme vectors from every cell, each reference name, a
     * parent whose records differ per cell */
    {
        const int gw = 2, gh = 2;
        int16_t mv[16]; uint8_t info[16];
        vp9hip_acc_cell p[4];
        for (int i = 0; i < 4; i++) {
            p[i].dx = 1000 * i; p[i].dy = -1000 * i; p[i].root = 77 + (uint32_t) i; p[i].hops = (uint16_t) (3 + i);
            p[i].end = (uint8_t) (i % 3); p[i].pad = 0;
        }
        for (int a = 0; a < next; a++)
            for (int b = 0; b < next; b++)
                for (int name = 0; name < 3; name++) {
                    for (size_t cell = 0; cell < 4; cell++) set_cell(mv, info, cell, name, 255, ext[a], ext[b]);
                    const vp9hip_acc_cell *par[3] = { p, p, p };
                    vp9hip_acc_cell *o = run(mv, info, gw, gh, 9, par, none, 1);
                    for (int r = 0; r < gh; r++)
                        for (int c = 0; c < gw; c++) {
                            const int pc = clampi(fl32(32 * c + 16 + ext[a]), 0, gw - 1);
                            const int pr = clampi(fl32(32 * r + 16 + ext[b]), 0, gh - 1);
                            const vp9hip_acc_cell *q = &p[pr * gw + pc];
                            CHECK(same(&o[r * gw + c], ext[a] + q->dx, ext[b] + q->dy, q->root, q->hops + 1, q->end));
                        }
                    free(o);
                    /* no parent for that name, with each end code */
                    for (int e = VP9HIP_ACC_END_NOFIELD; e <= VP9HIP_ACC_END_SCALED; e++) {
                        const vp9hip_acc_cell *par2[3] = { p, p, p };
                        int pend[3] = { VP9HIP_ACC_END_NOFIELD, VP9HIP_ACC_END_NOFIELD, VP9HIP_ACC_END_NOFIELD };
                        par2[name] = NULL; pend[name] = e;
                        o = run(mv, info, gw, gh, 9, par2, pend, 1);
                        for (int i = 0; i < 4; i++) CHECK(same(&o[i], ext[a], ext[b], 0, 1, e));
                        free(o);
                    }
                }
        /* intra cells, an unknown name, a compound cell */
        set_cell(mv, info, 0, 255, 255, 0, 0);
        set_cell(mv, info, 1, 7, 255, 5, -6);
        set_cell(mv, info, 2, 3, 1, -5, 6);
        set_cell(mv, info, 3, 1, 2, 40, 40);
        const vp9hip_acc_cell *par[3] = { p, p, p };
        vp9hip_acc_cell *o = run(mv, info, gw, gh, 0xfffffffeu, par, none, 1);
        CHECK(same(&o[0], 0, 0, 0xfffffffeu, 0, VP9HIP_ACC_END_INTRA));
        CHECK(same(&o[1], 5, -6, 0, 1, VP9HIP_ACC_END_NOFIELD));
        CHECK(same(&o[2], -5, 6, 0, 1, VP9HIP_ACC_END_NOFIELD));
        CHECK(same(&o[3], 40 + p[3].dx, 40 + p[3].dy, p[3].root, p[3].hops + 1, p[3].end));
        free(o);
        /* the wrap and saturation cases */
        p[0].dx = INT32_MAX; p[0].dy = INT32_MIN; p[0].hops = 65535;
        p[1].dx = INT32_MIN; p[1].dy = INT32_MAX; p[1].hops = 65534;
        set_cell(mv, info, 0, 0, 255, 1, -1);
        set_cell(mv, info, 1, 0, 255, -1, 1);
        set_cell(mv, info, 2, 0, 255, 32767, -32768 + 32);      /* from (1, 0) to (0, 1): p[1] */
        set_cell(mv, info, 3, 0, 255, -32768, -32768);          /* to (0, 0) */
        o = run(mv, info, gw, gh, 1, par, none, 1);
        CHECK(same(&o[0], INT32_MIN, INT32_MAX, p[0].root, 65535, p[0].end));
        CHECK(same(&o[1], INT32_MAX, INT32_MIN, p[1].root, 65535, p[1].end));
        CHECK(same(&o[2], INT32_MIN + 32767, INT32_MAX - 32736, p[1].root, 65535, p[1].end));
        CHECK(same(&o[3], INT32_MAX - 32768, (int32_t) 0x7fff8000, p[0].root, 65535, p[0].end));
        free(o);
    }

    /* the 4096 x 4096 grid: extreme vectors in every corner region, first without parents, then
     * chained onto that result */
    {
        const int gw = 4096, gh = 4096;
        const size_t cells = (size_t) gw * gh;
        int16_t *mv = malloc(cells * 8);
        uint8_t *info = malloc(cells * 4);
        for (int r = 0; r < gh; r++)
            for (int c = 0; c < gw; c++) {
                const size_t cell = (size_t) r * gw + c;
                const int i0 = (r * 7 + c) % 11 == 0 ? 255 : (r + c) % 3;
                set_cell(mv, info, cell, i0, (c & 1) ? 255 : 1, ext[(r + 3 * c) % next], ext[(5 * r + c) % next]);
            }
        const vp9hip_acc_cell *nopar[3] = { NULL, NULL, NULL };
        vp9hip_acc_cell *a = run(mv, info, gw, gh, 5, nopar, none, 0);
        const vp9hip_acc_cell *par[3] = { a, NULL, a };
        vp9hip_acc_cell *b = run(mv, info, gw, gh, 6, par, none, 0);
        uint64_t bad = 0;
        for (int r = 0; r < gh; r++)
            for (int c = 0; c < gw; c++) {
                const size_t cell = (size_t) r * gw + c;
                const int i0 = info[cell * 4], mx = mv[cell * 4], my = mv[cell * 4 + 1];
                if (i0 == 255) { bad += !same(&a[cell], 0, 0, 5, 0, 0) + !same(&b[cell], 0, 0, 6, 0, 0); continue; }
                bad += !same(&a[cell], mx, my, 0, 1, none[i0]);
                if (i0 == 1) { bad += !same(&b[cell], mx, my, 0, 1, VP9HIP_ACC_END_SCALED); continue; }
                const int pc = clampi(fl32(32 * c + 16 + mx), 0, gw - 1), pr = clampi(fl32(32 * r + 16 + my), 0, gh - 1);
                const vp9hip_acc_cell *q = &a[(size_t) pr * gw + pc];
                bad += !same(&b[cell], mx + q->dx, my + q->dy, q->root, q->hops + 1, q->end);
            }
        CHECK(bad == 0);
        free(a); free(b); free(mv); free(info);
    }

    /* bad arguments */
    {
        int16_t mv[4] = { 0 }; uint8_t info[4] = { 255, 255, 0, 0 };
        vp9hip_acc_cell o;
        const vp9hip_acc_cell *nopar[3] = { NULL, NULL, NULL };
        const int intra_end[3] = { VP9HIP_ACC_END_INTRA, VP9HIP_ACC_END_NOFIELD, VP9HIP_ACC_END_NOFIELD };
        CHECK(vp9hip_motion_acc_host(NULL, info, 1, 1, 1, nopar, none, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, NULL, 1, 1, 1, nopar, none, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 1, 1, 1, NULL, none, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 1, 1, 1, nopar, NULL, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 1, 1, 1, nopar, none, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 0, 1, 1, nopar, none, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 1, 4097, 1, nopar, none, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 1, 1, 1, nopar, intra_end, &o) == VP9HIP_EINVAL);
        CHECK(vp9hip_motion_acc_host(mv, info, 1, 1, 1, nopar, none, &o) == 0 && same(&o, 0, 0, 1, 0, 0));
    }
    if (fails) { fprintf(stderr, "motion_acc_host_check: %d checks failed\n", fails); return 1; }
    printf("motion_acc_host_check OK\n");
    return 0;
}
