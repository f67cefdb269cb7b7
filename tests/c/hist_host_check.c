// vp9hip_frame_histograms_host (csrc/host/vp9h_hist.c) at the extreme sizes and codes: a
// stand-alone program, no device, no Python, built plain and with ASan + UBSan (without
// -fwrapv, so a signed overflow is a finding). The planes are exact-size heap blocks, so a read
// past the rectangle's planes is a finding too; the output sits between guard bytes. Every case
// is a constant frame, whose histogram has a closed form: one bin a channel holds everything.
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

// One w x h frame (exact-size planes, tight rows) of the constant code v in all three planes.
// PLANES, and RGBM with colour space 7 (the planes pass through): the bin is known. RGBM with a
// matrix: some one bin of every channel holds w h, and M's bin is the largest of the three.
static void constant_case(int w, int h, int bpp, int ss_h, int ss_v, unsigned v, int what, int k, int colorspace, int full_range)
{
    const int by = bpp > 8 ? 2 : 1;
    const int cw = (w + ss_h) >> ss_h, ch = (h + ss_v) >> ss_v;
    void *pl[3];
    ptrdiff_t ls[3];
    for (int p = 0; p < 3; p++) {
        const size_t pw = p ? cw : w, ph = p ? ch : h, n = pw * ph;
        pl[p] = malloc(n * by);
        if (!pl[p]) { printf("out of memory\n"); exit(2); }
        ls[p] = (ptrdiff_t) pw * by;
        for (size_t i = 0; i < n; i++) {
            if (by == 1) ((uint8_t *) pl[p])[i] = (uint8_t) v;
            else ((uint16_t *) pl[p])[i] = (uint16_t) v;
        }
    }
    const int C = what == VP9HIP_HIST_RGBM ? 4 : 3, B = 1 << k;
    guarded go;
    int32_t *out = g_alloc(&go, (size_t) C * B * sizeof(int32_t));
    memset(out, 0x5A, (size_t) C * B * sizeof(int32_t));          // what it held before does not matter
    const vp9hip_hist_desc d = { what, k, colorspace, full_range, w, h, NULL };
    const int r = vp9hip_frame_histograms_host((const void *const *) pl, ls, bpp, ss_h, ss_v, &d, NULL, out);
    CHECK(r == 0);
    const unsigned maxv = (1u << bpp) - 1, stored = by == 1 ? (v & 255) : v;
    const int known = (int) ((stored > maxv ? maxv : stored) >> (bpp - k));
    int at[4] = { -1, -1, -1, -1 };
    for (int c = 0; c < C && r == 0; c++) {
        const int64_t n = what == VP9HIP_HIST_PLANES && c ? (int64_t) cw * ch : (int64_t) w * h;
        int nonzero = 0;
        for (int b = 0; b < B; b++)
            if (out[c * B + b]) { nonzero++; at[c] = b; CHECK(out[c * B + b] == n); }
        CHECK(nonzero == 1);
        if (what == VP9HIP_HIST_PLANES || colorspace == 7) CHECK(at[c] == known);
    }
    if (what == VP9HIP_HIST_RGBM && r == 0) {
        const int m = at[0] > at[1] ? (at[0] > at[2] ? at[0] : at[2]) : (at[1] > at[2] ? at[1] : at[2]);
        CHECK(at[3] == m);
    }
    g_free(&go);
    for (int p = 0; p < 3; p++) free(pl[p]);
}

// A refused call leaves the output as it was.
static void refused(void)
{
    uint8_t px[4] = { 1, 2, 3, 4 };
    const void *pl[3] = { px, px, px }, *hole[3] = { px, NULL, px };
    const ptrdiff_t ls[3] = { 2, 1, 1 };
    guarded go;
    const size_t bytes = 4 * 256 * sizeof(int32_t);
    int32_t *out = g_alloc(&go, bytes);
    memset(out, 0x5A, bytes);
    const vp9hip_hist_desc ok = { VP9HIP_HIST_PLANES, 8, 2, 0, 2, 2, NULL };
    vp9hip_hist_desc d;
    const vp9hip_rect odd_x = { 1, 0, 1, 1 }, odd_y = { 0, 1, 1, 1 }, wide = { 0, 0, 3, 1 }, tall = { 0, 0, 1, 3 },
                      empty = { 0, 0, 0, 1 }, neg = { -2, 0, 1, 1 }, right = { 2, 0, 1, 1 }, huge = { 0, 0, 0x7fffffff, 1 };
    CHECK(vp9hip_frame_histograms_host(NULL, ls, 8, 1, 1, &ok, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, NULL, 8, 1, 1, &ok, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, NULL, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, NULL, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(hole, ls, 8, 1, 1, &ok, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 9, 1, 1, &ok, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 2, 1, &ok, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, -1, &ok, NULL, out) == VP9HIP_EINVAL);
    d = ok; d.what = 2;
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    d = ok; d.what = -1;
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    d = ok; d.bins_log2 = 3;
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    d = ok; d.bins_log2 = 9;
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    d = ok; d.width = 0;
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    d = ok; d.height = 16385;
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    for (int cs = 0; cs <= 8; cs += (cs == 0 ? 6 : 2)) {           // 0, 6, 8
        d = ok; d.what = VP9HIP_HIST_RGBM; d.colorspace = cs;
        CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &d, NULL, out) == VP9HIP_EINVAL);
    }
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &odd_x, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &odd_y, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &wide, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &tall, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &empty, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &neg, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &right, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 1, 1, &ok, &huge, out) == VP9HIP_EINVAL);
    for (size_t i = 0; i < bytes; i++) CHECK(((uint8_t *) out)[i] == 0x5A);
    CHECK(vp9hip_frame_histograms_host(pl, ls, 8, 0, 0, &ok, &odd_x, out) == 0);   // 4:4:4: any x
    CHECK(out[2] == 1 && out[256 + 2] == 1 && out[512 + 2] == 1);
    g_free(&go);
}

int main(void)
{
    refused();
    static const int sizes[4][2] = { { 1, 1 }, { 16384, 1 }, { 1, 16384 }, { 4096, 4096 } };
    static const int depths[3] = { 8, 10, 12 };
    for (int s = 0; s < 4; s++)
        for (int di = 0; di < 3; di++) {
            const int w = sizes[s][0], h = sizes[s][1], bpp = depths[di];
            const int ss = (s + di) & 3;                          // the four subsamplings in turn
            const unsigned codes[3] = { 0, (1u << bpp) - 1, 65535 };
            for (int ci = 0; ci < 3; ci++) {
                const int k = ci == 0 ? 4 : ci == 1 ? bpp : 8;
                constant_case(w, h, bpp, ss & 1, ss >> 1, codes[ci], VP9HIP_HIST_PLANES, k, 2, 0);
                constant_case(w, h, bpp, ss & 1, ss >> 1, codes[ci], VP9HIP_HIST_RGBM, k, ci == 2 ? 7 : (s & 1 ? 5 : 1), di & 1);
                if (s < 3) constant_case(w, h, bpp, ss & 1, ss >> 1, codes[ci], VP9HIP_HIST_RGBM, bpp, ci == 2 ? 2 : 7, 1);
            }
        }
    if (fails) { printf("hist_host_check: %d failures\n", fails); return 1; }
    printf("hist_host_check OK\n");
    return 0;
}
