/* vp9hip_acc_warp_host at its edges: the accumulated residual of include/vp9hip.h on the host,
 * where the sanitizer builds can watch it (make -C ffmpeg-hybrid_amd/csrc acc_warp_host_check;
 * built without -fwrapv, so a signed overflow or a shift of a negative value is a finding).
 * Extreme vectors (+-32767, -32768, INT32_MAX / INT32_MIN) from every cell, stored codes of
 * 65535, planes 1 sample wide, odd planes and the 16384-sample extremes, every subsampling, both
 * modes and outputs. The planes and the field are exact-size heap blocks (ASan sees a read past
 * the visible size), the output and the mask sit between guard bytes (every build), and every
 * sample is compared with a second statement written here. No device, no Python. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

#define GUARD 64

static int fails;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "acc_warp_host_check: %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
/* floor(v / 16), spelled without a shift of a negative value */
static int64_t fl16(int64_t v) { int64_t q = v / 16; return (v % 16 != 0 && v < 0) ? q - 1 : q; }

static uint64_t rnd_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) (rnd_state >> 33);
}

static int64_t get(const void *plane, int hbd, int64_t pw, int64_t x, int64_t y)
{
    return hbd ? ((const uint16_t *) plane)[y * pw + x] : ((const uint8_t *) plane)[y * pw + x];
}

static const int32_t ext[] = { 0, -1, -8, -9, 7, 8, 32767, -32767, -32768, INT32_MAX, INT32_MIN, 123, -4567 };
#define NEXT ((int) (sizeof(ext) / sizeof(ext[0])))

/* One pair of w x h at the given depth and subsampling, top: the largest stored code. */
static void pair(int w, int h, int bpp, int ss_h, int ss_v, uint32_t top)
{
    const int hbd = bpp > 8;
    const int64_t gw = 2 * ((w + 7) >> 3), gh = 2 * ((h + 7) >> 3);
    void *a[3], *b[3];
    ptrdiff_t ls[3];
    int64_t pw[3], ph[3], off[3];
    const int64_t bytes = vp9hip_warp_layout(w, h, ss_h, ss_v, off);
    CHECK(bytes > 0);
    for (int p = 0; p < 3; p++) {
        pw[p] = p ? (w + ss_h) >> ss_h : w; ph[p] = p ? (h + ss_v) >> ss_v : h;
        ls[p] = (ptrdiff_t) (pw[p] * (hbd ? 2 : 1));
        a[p] = malloc((size_t) (ls[p] * ph[p])); b[p] = malloc((size_t) (ls[p] * ph[p]));
        for (int64_t i = 0; i < pw[p] * ph[p]; i++) {
            const uint32_t va = rnd() % 8 == 0 ? top : rnd() % (top + 1), vb = rnd() % 8 == 0 ? top : rnd() % (top + 1);
            if (hbd) { ((uint16_t *) a[p])[i] = (uint16_t) va; ((uint16_t *) b[p])[i] = (uint16_t) vb; }
            else { ((uint8_t *) a[p])[i] = (uint8_t) va; ((uint8_t *) b[p])[i] = (uint8_t) vb; }
        }
    }
    CHECK(off[0] == 0 && off[1] == 2 * pw[0] * ph[0] && off[2] == off[1] + 2 * pw[1] * ph[1] && bytes == off[2] + 2 * pw[2] * ph[2]);
    vp9hip_acc_cell *acc = malloc((size_t) (gw * gh) * sizeof(*acc));
    const uint32_t sb = 0xfffffff0u;
    for (int64_t i = 0; i < gw * gh; i++) {
        acc[i].dx = ext[(i + i / gw) % NEXT]; acc[i].dy = ext[(3 * i + i / gw) % NEXT];
        acc[i].root = i % 5 == 0 ? sb - 1 : i % 7 == 0 ? 0 : sb;
        acc[i].hops = (uint16_t) (i % 11 == 0 ? 0 : i % 3 == 0 ? 65535 : 1 + i % 9);
        acc[i].end = (uint8_t) (i % 3); acc[i].pad = 0;
    }
    uint8_t *dg = malloc((size_t) bytes + 2 * GUARD), *mg = malloc((size_t) (gw * gh) + 2 * GUARD);
    for (int mode = VP9HIP_WARP_NEAREST; mode <= VP9HIP_WARP_BILINEAR; mode++)
        for (int output = VP9HIP_WARP_RESIDUAL; output <= VP9HIP_WARP_PICTURE; output++) {
            memset(dg, 0xa5, (size_t) bytes + 2 * GUARD);
            memset(mg, 0xa5, (size_t) (gw * gh) + 2 * GUARD);
            CHECK(vp9hip_acc_warp_host((const void *const *) a, ls, (const void *const *) b, ls, acc, sb, w, h, bpp, ss_h, ss_v,
                                       mode, output, dg + GUARD, mg + GUARD) == 0);
            for (int i = 0; i < GUARD; i++)
                CHECK(dg[i] == 0xa5 && dg[GUARD + bytes + i] == 0xa5 && mg[i] == 0xa5 && mg[GUARD + gw * gh + i] == 0xa5);
            uint64_t bad = 0;
            for (int64_t i = 0; i < gw * gh; i++) bad += mg[GUARD + i] != (acc[i].hops > 0 && acc[i].root == sb);
            for (int p = 0; p < 3; p++) {
                const int sh = p ? ss_h : 0, sv = p ? ss_v : 0;
                for (int64_t y = 0; y < ph[p]; y++)
                    for (int64_t x = 0; x < pw[p]; x++) {
                        const vp9hip_acc_cell *q = &acc[((sv ? 2 * y : y) / 4) * gw + (sh ? 2 * x : x) / 4];
                        const int app = q->hops > 0 && q->root == sb;
                        const int64_t px = clampl(q->dx, -32768, 32767) * (sh ? 1 : 2), py = clampl(q->dy, -32768, 32767) * (sv ? 1 : 2);
                        const int64_t av = get(a[p], hbd, pw[p], x, y);
                        int64_t pred;
                        if (mode == VP9HIP_WARP_NEAREST) {
                            pred = get(b[p], hbd, pw[p], clampl(x + fl16(px + 8), 0, pw[p] - 1), clampl(y + fl16(py + 8), 0, ph[p] - 1));
                        } else {
                            const int64_t x0 = x + fl16(px), y0 = y + fl16(py), fx = px - 16 * fl16(px), fy = py - 16 * fl16(py);
                            const int64_t xa = clampl(x0, 0, pw[p] - 1), xb = clampl(x0 + 1, 0, pw[p] - 1);
                            const int64_t ya = clampl(y0, 0, ph[p] - 1), yb = clampl(y0 + 1, 0, ph[p] - 1);
                            const int64_t top_row = (16 - fx) * get(b[p], hbd, pw[p], xa, ya) + fx * get(b[p], hbd, pw[p], xb, ya);
                            const int64_t bot_row = (16 - fx) * get(b[p], hbd, pw[p], xa, yb) + fx * get(b[p], hbd, pw[p], xb, yb);
                            pred = ((16 - fy) * top_row + fy * bot_row + 128) / 256;
                        }
                        uint16_t got;
                        memcpy(&got, dg + GUARD + off[p] + 2 * (y * pw[p] + x), 2);
                        const uint16_t want = output == VP9HIP_WARP_RESIDUAL
                                                  ? (uint16_t) (int16_t) (app ? clampl(av - pred, -32768, 32767) : 0)
                                                  : (uint16_t) (app ? pred : av);
                        bad += got != want;
                    }
            }
            CHECK(bad == 0);
            /* without a mask */
            uint8_t *d2 = malloc((size_t) bytes);
            CHECK(vp9hip_acc_warp_host((const void *const *) a, ls, (const void *const *) b, ls, acc, sb, w, h, bpp, ss_h, ss_v,
                                       mode, output, d2, NULL) == 0);
            CHECK(!memcmp(d2, dg + GUARD, (size_t) bytes));
            free(d2);
        }
    free(dg); free(mg); free(acc);
    for (int p = 0; p < 3; p++) { free(a[p]); free(b[p]); }
}

int main(void)
{
    static const int sizes[][2] = { { 1, 1 }, { 1, 9 }, { 5, 3 }, { 24, 16 }, { 66, 34 }, { 16384, 9 }, { 7, 16384 } };
    for (unsigned s = 0; s < sizeof(sizes) / sizeof(sizes[0]); s++)
        for (int ss = 0; ss < 4; ss++) {
            pair(sizes[s][0], sizes[s][1], 8, ss & 1, ss >> 1, 255);
            pair(sizes[s][0], sizes[s][1], 10, ss & 1, ss >> 1, 1023);
            pair(sizes[s][0], sizes[s][1], 12, ss & 1, ss >> 1, 65535);     /* stored codes beyond the depth */
        }

    /* the int16 clamp of the residual, both ways */
    {
        uint16_t hi[16], lo[16];
        for (int i = 0; i < 16; i++) { hi[i] = 65535; lo[i] = 0; }
        const void *const ph[3] = { hi, hi, hi }, *const pl[3] = { lo, lo, lo };
        const ptrdiff_t ls[3] = { 8, 8, 8 };
        vp9hip_acc_cell acc[4];
        memset(acc, 0, sizeof(acc));
        for (int i = 0; i < 4; i++) { acc[i].root = 3; acc[i].hops = 1; }
        int16_t out[48];
        CHECK(vp9hip_acc_warp_host(ph, ls, pl, ls, acc, 3, 4, 4, 12, 0, 0, VP9HIP_WARP_BILINEAR, VP9HIP_WARP_RESIDUAL, out, NULL) == 0);
        for (int i = 0; i < 48; i++) CHECK(out[i] == 32767);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, VP9HIP_WARP_NEAREST, VP9HIP_WARP_RESIDUAL, out, NULL) == 0);
        for (int i = 0; i < 48; i++) CHECK(out[i] == -32768);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, VP9HIP_WARP_BILINEAR, VP9HIP_WARP_PICTURE, out, NULL) == 0);
        for (int i = 0; i < 48; i++) CHECK((uint16_t) out[i] == 65535);

        /* bad arguments: refused, and nothing written */
        memset(out, 0x5a, sizeof(out));
        int16_t ref[48];
        memset(ref, 0x5a, sizeof(ref));
        CHECK(vp9hip_acc_warp_host(NULL, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, NULL, ph, ls, acc, 3, 4, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, NULL, ls, acc, 3, 4, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, NULL, acc, 3, 4, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, NULL, 3, 4, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, 0, 0, NULL, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 0, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 16385, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 9, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 2, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 0, -1, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, 2, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_warp_host(pl, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, 0, -1, out, NULL) == VP9HIP_EINVAL);
        const void *const hole[3] = { lo, NULL, lo };
        CHECK(vp9hip_acc_warp_host(hole, ls, ph, ls, acc, 3, 4, 4, 12, 0, 0, 0, 0, out, NULL) == VP9HIP_EINVAL);
        CHECK(!memcmp(out, ref, sizeof(out)));
        CHECK(vp9hip_warp_layout(0, 4, 0, 0, NULL) == VP9HIP_EINVAL && vp9hip_warp_layout(4, 4, 0, 2, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_warp_layout(16384, 16384, 0, 0, NULL) == 6ll * 16384 * 16384);
    }
    if (fails) { fprintf(stderr, "acc_warp_host_check: %d checks failed\n", fails); return 1; }
    printf("acc_warp_host_check OK\n");
    return 0;
}
