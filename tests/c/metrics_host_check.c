// vp9hip_frame_metrics_host (csrc/host/vp9h_metrics.c) at the extreme sizes and codes: a
// stand-alone program, no device, no Python, built plain and with ASan + UBSan (without
// -fwrapv, so a signed overflow is a finding). The planes are exact-size heap blocks, so a read
// past the visible size is a finding too; the outputs sit between guard bytes. Every case has a
// closed form, which the result is compared with.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

#define GUARD 64
static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

typedef struct { uint8_t *base; size_t bytes; } guarded;
static void *g_alloc(guarded *g, size_t bytes)
{
    g->bytes = bytes;
    g->base = malloc(bytes + 2 * GUARD);
    if (!g->base) { printf("out of memory\n"); exit(2); }
    memset(g->base, 0xC3, bytes + 2 * GUARD);
    return g->base + GUARD;
}
static void g_free(guarded *g)
{
    for (size_t i = 0; i < GUARD; i++) CHECK(g->base[i] == 0xC3 && g->base[GUARD + g->bytes + i] == 0xC3);
    free(g->base);
}

// One pair of w x h frames (exact-size planes, tight rows) of the constant codes va / vb, with b
// optional, checked against the closed form.
static void constant_case(int w, int h, int bpp, int ss_h, int ss_v, unsigned va, unsigned vb, int with_b, int with_cells)
{
    const int by = bpp > 8 ? 2 : 1;
    const int cw = (w + ss_h) >> ss_h, ch = (h + ss_v) >> ss_v;
    const int mw = (w + 15) >> 4, mh = (h + 15) >> 4;
    void *pa[3], *pb[3];
    ptrdiff_t ls[3];
    for (int p = 0; p < 3; p++) {
        const size_t pw = p ? cw : w, ph = p ? ch : h, n = pw * ph;
        pa[p] = malloc(n * by);
        pb[p] = malloc(n * by);
        if (!pa[p] || !pb[p]) { printf("out of memory\n"); exit(2); }
        ls[p] = (ptrdiff_t) pw * by;
        for (size_t i = 0; i < n; i++) {
            if (by == 1) { ((uint8_t *) pa[p])[i] = (uint8_t) va; ((uint8_t *) pb[p])[i] = (uint8_t) vb; }
            else { ((uint16_t *) pa[p])[i] = (uint16_t) va; ((uint16_t *) pb[p])[i] = (uint16_t) vb; }
        }
    }
    guarded go, gc;
    int64_t *out = g_alloc(&go, 24 * sizeof(int64_t));
    int32_t *cells = g_alloc(&gc, (size_t) mw * mh * sizeof(int32_t));
    const int r = vp9hip_frame_metrics_host((const void *const *) pa, ls, with_b ? (const void *const *) pb : NULL,
                                            with_b ? ls : NULL, w, h, bpp, ss_h, ss_v, out, with_cells ? cells : NULL);
    CHECK(r == 0);
    const int64_t d = va > vb ? (int64_t) va - vb : (int64_t) vb - va;
    for (int p = 0; p < 3 && r == 0; p++) {
        const int64_t n = (int64_t) (p ? cw : w) * (p ? ch : h);
        const int64_t *m = out + 8 * p;
        CHECK(m[VP9HIP_METRIC_SUM_A] == n * va);
        CHECK(m[VP9HIP_METRIC_SUMSQ_A] == n * va * va);
        CHECK(m[VP9HIP_METRIC_SUM_B] == (with_b ? n * vb : 0));
        CHECK(m[VP9HIP_METRIC_SAD] == (with_b ? n * d : 0));
        CHECK(m[VP9HIP_METRIC_SSE] == (with_b ? n * d * d : 0));
        CHECK(m[VP9HIP_METRIC_NDIFF] == (with_b && d ? n : 0));
        CHECK(m[VP9HIP_METRIC_MAXDIFF] == (with_b ? d : 0));
        CHECK(m[VP9HIP_METRIC_FIRST] == (with_b && d ? 0 : -1));
    }
    if (with_cells && r == 0) {
        int64_t sum = 0;
        for (int cy = 0; cy < mh; cy++)
            for (int cx = 0; cx < mw; cx++) {
                const int64_t vis = (int64_t) (w - 16 * cx < 16 ? w - 16 * cx : 16) * (h - 16 * cy < 16 ? h - 16 * cy : 16);
                CHECK(cells[cy * mw + cx] == vis * d);
                sum += cells[cy * mw + cx];
            }
        CHECK(sum == out[VP9HIP_METRIC_SAD]);
    }
    g_free(&go);
    g_free(&gc);
    for (int p = 0; p < 3; p++) { free(pa[p]); free(pb[p]); }
}

// A refused call leaves the outputs as they were.
static void refused(void)
{
    uint8_t px[4] = { 1, 2, 3, 4 };
    const void *pl[3] = { px, px, px };
    const ptrdiff_t ls[3] = { 1, 1, 1 };
    guarded go, gc;
    int64_t *out = g_alloc(&go, 24 * sizeof(int64_t));
    int32_t *cells = g_alloc(&gc, sizeof(int32_t));
    memset(out, 0x5A, 24 * sizeof(int64_t));
    memset(cells, 0x5A, sizeof(int32_t));
    CHECK(vp9hip_frame_metrics_host(pl, ls, pl, ls, 0, 1, 8, 1, 1, out, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(pl, ls, pl, ls, 1, 16385, 8, 1, 1, out, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(pl, ls, pl, ls, 1, 1, 9, 1, 1, out, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(pl, ls, pl, ls, 1, 1, 8, 2, 1, out, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(pl, ls, pl, ls, 1, 1, 8, 1, -1, out, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(pl, ls, NULL, NULL, 1, 1, 8, 1, 1, out, cells) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(NULL, ls, pl, ls, 1, 1, 8, 1, 1, out, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_metrics_host(pl, ls, pl, ls, 1, 1, 8, 1, 1, NULL, NULL) == VP9HIP_EINVAL);
    for (size_t i = 0; i < 24 * sizeof(int64_t); i++) CHECK(((uint8_t *) out)[i] == 0x5A);
    for (size_t i = 0; i < sizeof(int32_t); i++) CHECK(((uint8_t *) cells)[i] == 0x5A);
    g_free(&go);
    g_free(&gc);
}

int main(void)
{
    refused();
    for (int ss = 0; ss < 4; ss++) {
        constant_case(1, 1, 8, ss & 1, ss >> 1, 255, 0, 1, 1);
        constant_case(1, 1, 12, ss & 1, ss >> 1, 65535, 0, 1, 1);
        constant_case(16384, 1, 10, ss & 1, ss >> 1, 65535, 0, 1, 1);
        constant_case(1, 16384, 10, ss & 1, ss >> 1, 0, 65535, 1, 1);
    }
    constant_case(16384, 1, 8, 1, 1, 255, 7, 1, 1);
    constant_case(1, 16384, 8, 1, 1, 9, 9, 1, 1);                 // equal frames: FIRST -1
    constant_case(16384, 1, 12, 1, 1, 4095, 0, 0, 0);             // statistics only
    constant_case(4096, 4096, 12, 0, 0, 65535, 0, 1, 1);          // sum a^2 = 65535^2 * 2^24 per plane
    constant_case(4096, 4096, 12, 1, 1, 65535, 0, 1, 0);
    if (fails) { printf("metrics_host_check: %d failures\n", fails); return 1; }
    printf("metrics_host_check OK\n");
    return 0;
}
