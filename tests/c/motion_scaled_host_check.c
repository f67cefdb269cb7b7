// vp9hip_motion_scaled_host (csrc/host/vp9h_motion_scaled.c) at the extreme grids, sizes and
// vectors: a stand-alone program, no device, no Python, built plain and with ASan + UBSan
// (without -fwrapv, so a signed overflow is a finding). The source arrays are exact-size heap
// blocks, the (h + 3) >> 2 rows of (w + 3) >> 2 cells the visible size touches, between guard
// bytes, so a read of a cell beyond the visible size is a finding too; the output sits between
// guard bytes as well. Every case is a constant field (sbox of a constant is the constant), or
// small enough to state by hand.
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

// One w x h field of the constant vector (vx, vy) in every cell, second vectors poison, to
// ow x oh from both sources as int16 with the coverage: the constants, 256.
static void constant_case(int w, int h, int vx, int vy, int ow, int oh)
{
    const size_t cw = (size_t) (w + 3) >> 2, ch = (size_t) (h + 3) >> 2, n = cw * ch;
    guarded gm, gi, ga, go;
    int16_t *mv = g_alloc(&gm, n * 8);
    uint8_t *info = g_alloc(&gi, n * 4);
    vp9hip_acc_cell *acc = g_alloc(&ga, n * sizeof(vp9hip_acc_cell));
    for (size_t i = 0; i < n; i++) {
        mv[4 * i] = (int16_t) vx; mv[4 * i + 1] = (int16_t) vy; mv[4 * i + 2] = 0x7fff; mv[4 * i + 3] = 0x7fff;
        info[4 * i] = (uint8_t) (i % 3); info[4 * i + 1] = 1; info[4 * i + 2] = 0; info[4 * i + 3] = 0;
        // the acc sums lie beyond int16 on the vector's side: the clamp brings them to (vx, vy) at the int16 ends
        acc[i] = (vp9hip_acc_cell) { vx == -32768 ? INT32_MIN : vx == 32767 ? INT32_MAX : vx,
                                     vy == -32768 ? -40000 : vy == 32767 ? 40000 : vy, 5, 65535, 0, 0 };
    }
    for (int src = VP9HIP_MVT_CODED; src <= VP9HIP_MVT_ACC; src++) {
        const vp9hip_mvt_desc d = { VP9HIP_MVT_I16, src, 3, w, h, ow, oh, 0, 0 };
        int16_t *out = g_alloc(&go, (size_t) 3 * ow * oh * 2);
        // the other source's arrays are not looked at: NULL
        const int r = vp9hip_motion_scaled_host(src ? NULL : mv, src ? NULL : info, src ? acc : NULL, (ptrdiff_t) cw, &d, out);
        CHECK(r == 0);
        for (int i = 0; i < ow * oh && r == 0; i++)
            CHECK(out[i] == vx && out[ow * oh + i] == vy && out[2 * ow * oh + i] == 256);
        g_free(&go);
    }
    g_free(&gm); g_free(&gi); g_free(&ga);
}

// 8 x 8 (a 2 x 2 grid) -> 1 x 1 and 2 x 2 by hand: negative quarters, an intra cell with a
// stale vector, and the half formats' bits
static void by_hand(void)
{
    guarded gm, gi, go;
    int16_t *mv = g_alloc(&gm, 4 * 8);
    uint8_t *info = g_alloc(&gi, 4 * 4);
    const int16_t vec[4][2] = { { -3, 8 }, { -2, -16 }, { -2, 24 }, { 999, -999 } };
    for (int i = 0; i < 4; i++) {
        mv[4 * i] = vec[i][0]; mv[4 * i + 1] = vec[i][1]; mv[4 * i + 2] = -32768; mv[4 * i + 3] = -32768;
        memset(info + 4 * i, 0, 4);
    }
    info[12] = 255;                                        // cell (1, 1) is intra: 999 / -999 never enter
    vp9hip_mvt_desc d = { VP9HIP_MVT_I16, VP9HIP_MVT_CODED, 3, 8, 8, 1, 1, 0, 0 };
    int16_t *out = g_alloc(&go, 6);
    // every cell weighs 16 of 64: x: A = 16 (-3 - 2 - 2 + 0) = -112 -> floor((-112 + 32) / 64) = -2 (-1.75 rounds to -2);
    // y: A = 16 (8 - 16 + 24) = 256 -> floor(288 / 64) = 4; coverage: A = 16 * 3 * 256 -> 192
    CHECK(vp9hip_motion_scaled_host(mv, info, NULL, 2, &d, out) == 0);
    CHECK(out[0] == -2 && out[1] == 4 && out[2] == 192);
    mv[0] = -2;                                            // x: A = -96 -> floor(-64 / 64) = -1 (-1.5 rounds up to -1)
    CHECK(vp9hip_motion_scaled_host(mv, info, NULL, 2, &d, out) == 0);
    CHECK(out[0] == -1 && out[1] == 4 && out[2] == 192);
    mv[0] = -3;
    g_free(&go);
    d.out_width = d.out_height = 2; d.format = VP9HIP_MVT_F16;
    uint16_t *ob = g_alloc(&go, 24);
    CHECK(vp9hip_motion_scaled_host(mv, info, NULL, 2, &d, ob) == 0);
    // kx = ky = 2 / 64 = 1 / 32: -3 / 32 = -0.09375 -> 0xAE00, -2 / 32 = -0.0625 -> 0xAC00, 0 -> 0;
    // 8 / 32 = 0.25 -> 0x3400, -16 / 32 = -0.5 -> 0xB800, 24 / 32 = 0.75 -> 0x3A00; coverage 1 -> 0x3C00, 0
    CHECK(ob[0] == 0xAE00 && ob[1] == 0xAC00 && ob[2] == 0xAC00 && ob[3] == 0);
    CHECK(ob[4] == 0x3400 && ob[5] == 0xB800 && ob[6] == 0x3A00 && ob[7] == 0);
    CHECK(ob[8] == 0x3C00 && ob[9] == 0x3C00 && ob[10] == 0x3C00 && ob[11] == 0);
    g_free(&go);
    // a pitch of its own: rows 16 bytes apart, the gap untouched; two planes
    d.format = VP9HIP_MVT_I16; d.planes = 2; d.pitch = 16;
    out = g_alloc(&go, 64);
    CHECK(vp9hip_motion_scaled_host(mv, info, NULL, 2, &d, out) == 0);
    CHECK(out[0] == -3 && out[1] == -2 && out[8] == -2 && out[9] == 0 && out[16] == 8 && out[17] == -16 && out[24] == 24 && out[25] == 0);
    for (int i = 0; i < 32; i++)
        if ((i & 7) > 1) CHECK((uint16_t) out[i] == 0xC3C3);
    g_free(&go);
    g_free(&gm); g_free(&gi);
}

// A refused call leaves the output as it was.
static void refused(void)
{
    const int16_t mv[16] = { 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16 };
    const uint8_t info[16] = { 0 };
    vp9hip_acc_cell acc[4];
    memset(acc, 0, sizeof(acc));
    guarded go;
    int16_t *out = g_alloc(&go, 64);
    const vp9hip_mvt_desc ok = { VP9HIP_MVT_I16, VP9HIP_MVT_CODED, 3, 8, 8, 1, 1, 0, 0 };
    vp9hip_mvt_desc d;
#define REFUSED(mod) do { d = ok; mod; CHECK(vp9hip_motion_scaled_host(mv, info, acc, 2, &d, out) == VP9HIP_EINVAL); } while (0)
    REFUSED(d.format = 2);
    REFUSED(d.format = -1);
    REFUSED(d.source = 2);
    REFUSED(d.source = -1);
    REFUSED(d.planes = 1);
    REFUSED(d.planes = 4);
    REFUSED(d.width = 0);
    REFUSED(d.width = 16385);
    REFUSED(d.height = 0);
    REFUSED(d.height = 16385);
    REFUSED(d.out_width = 0);
    REFUSED(d.out_height = 16385);
    REFUSED(d.pitch = 1);
    REFUSED(d.pitch = 24);
    REFUSED(d.frame_stride = 4);
    REFUSED(d.frame_stride = 7);
    CHECK(vp9hip_motion_scaled_host(NULL, info, acc, 2, &ok, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_motion_scaled_host(mv, NULL, acc, 2, &ok, out) == VP9HIP_EINVAL);
    d = ok; d.source = VP9HIP_MVT_ACC;
    CHECK(vp9hip_motion_scaled_host(mv, info, NULL, 2, &d, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_motion_scaled_host(mv, info, acc, 1, &ok, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_motion_scaled_host(mv, info, acc, 2, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_motion_scaled_host(mv, info, acc, 2, &ok, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_motion_scaled_host(mv, info, acc, 2, &ok, (uint8_t *) out + 1) == VP9HIP_EINVAL);
    for (int i = 0; i < 32; i++) CHECK((uint16_t) out[i] == 0xC3C3);
    g_free(&go);
}

int main(void)
{
    refused();
    by_hand();
    constant_case(8, 8, -32768, 32767, 1, 1);              // a 2 x 2 grid
    constant_case(5, 3, 32767, -32768, 7, 9);              // a 2 x 2 grid partly visible, upscaled
    constant_case(1, 1, -1, 1, 16384, 1);                  // the widest upscale
    constant_case(16384, 1, -32768, -32768, 3, 2);
    constant_case(1, 16384, -32768, -32768, 3, 2);
    constant_case(16384, 16384, -32768, -32768, 3, 2);     // a 4096 x 4096 grid: |A| = 2^15 2^28, the largest sums
    constant_case(16384, 16384, 32767, 32767, 1, 1);
    if (fails) { printf("motion_scaled_host_check: %d failures\n", fails); return 1; }
    printf("motion_scaled_host_check OK\n");
    return 0;
}
