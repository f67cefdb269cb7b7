// vp9hip_residual_scaled_host (csrc/host/vp9h_residual_scaled.c) at the extreme sizes and codes:
// a stand-alone program, no device, no Python, built plain and with ASan + UBSan (without
// -fwrapv, so a signed overflow is a finding). The planes are exact-size heap blocks between
// guard bytes, so a read past the visible size is a finding too; the output sits between guard
// bytes as well. Every case is a constant plane (sbox of a constant is the constant), or small
// enough to state by hand.
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

static int64_t clip_pm(int64_t v, int64_t m) { return v < -m ? -m : v > m ? m : v; }
static int64_t floor_shift(int64_t v, int s) { return v >= 0 ? v >> s : -((-v + ((int64_t) 1 << s) - 1) >> s); }

// One w x h field (exact-size planes, tight rows) of the constants y, u, v to ow x oh in the two
// int16 formats, against the closed form: the planes themselves, and their matrix.
static void constant_case(int w, int h, int bpp, int ss_h, int ss_v, int y, int u, int v, int ow, int oh, int cs, int full)
{
    const int cw = (w + ss_h) >> ss_h, ch = (h + ss_v) >> ss_v;
    const int val[3] = { y, u, v };
    guarded gp[3], go;
    const int16_t *pl[3];
    ptrdiff_t pitch[3];
    for (int p = 0; p < 3; p++) {
        const size_t n = (size_t) (p ? cw : w) * (p ? ch : h);
        int16_t *q = g_alloc(&gp[p], n * 2);
        for (size_t i = 0; i < n; i++) q[i] = (int16_t) val[p];
        pl[p] = q;
        pitch[p] = p ? cw : w;
    }
    const int64_t m = (1 << bpp) - 1;
    int32_t c[5], S;
    CHECK(vp9hip_out_coefs(cs, full, bpp, bpp, c, &S) == 0);
    int64_t rgb[3];
    if (cs == 7) {
        rgb[0] = clip_pm(v, m); rgb[1] = clip_pm(y, m); rgb[2] = clip_pm(u, m);
    } else {
        const int64_t rnd = (int64_t) 1 << (S - 1);
        rgb[0] = clip_pm(floor_shift((int64_t) c[0] * y + (int64_t) c[1] * v + rnd, S), m);
        rgb[1] = clip_pm(floor_shift((int64_t) c[0] * y - (int64_t) c[2] * u - (int64_t) c[3] * v + rnd, S), m);
        rgb[2] = clip_pm(floor_shift((int64_t) c[0] * y + (int64_t) c[4] * u + rnd, S), m);
    }
    for (int fmt = VP9HIP_RESID_YUV_I16; fmt <= VP9HIP_RESID_RGB_I16; fmt += 2) {
        vp9hip_resid_desc d = { fmt, cs, full, ow, oh, 0, 0 };
        int16_t *out = g_alloc(&go, (size_t) 3 * ow * oh * 2);
        const int r = vp9hip_residual_scaled_host(pl, pitch, w, h, ss_h, ss_v, bpp, &d, out);
        CHECK(r == 0);
        for (int p = 0; p < 3 && r == 0; p++)
            for (int i = 0; i < ow * oh; i++)
                CHECK(out[p * ow * oh + i] == (fmt == VP9HIP_RESID_YUV_I16 ? val[p] : rgb[p]));
        g_free(&go);
    }
    for (int p = 0; p < 3; p++) g_free(&gp[p]);
}

// 3 x 2 -> 2 x 1 by hand, negative halves included, and the half formats' bits
static void by_hand(void)
{
    guarded gp[3], go;
    const int16_t src[3][6] = { { -3, -2, 5, -2, -3, 4 }, { -1, -1, -1, -1, -1, -2 }, { 32767, 32767, 32767, 32767, 32767, 32767 } };
    const int16_t *pl[3];
    const ptrdiff_t pitch[3] = { 3, 3, 3 };
    for (int p = 0; p < 3; p++) {
        int16_t *q = g_alloc(&gp[p], 12);
        memcpy(q, src[p], 12);
        pl[p] = q;
    }
    // weights per axis: x: output 0 takes columns 0 (2), 1 (1); output 1 takes 1 (1), 2 (2); y: both rows (1 each); w h = 6
    // Y: out0 A = 2(-3) + (-2) + 2(-2) + (-3) = -15 -> floor((-15 + 3) / 6) = -2;  out1 A = -2 + 10 - 3 + 8 = 13 -> floor(16 / 6) = 2
    // U: out0 A = -6 -> floor(-3 / 6) = -1;  out1 A = -1 - 2 - 1 - 4 = -8 -> floor(-5 / 6) = -1
    vp9hip_resid_desc d = { VP9HIP_RESID_YUV_I16, 2, 0, 2, 1, 0, 0 };
    int16_t *out = g_alloc(&go, 12);
    CHECK(vp9hip_residual_scaled_host(pl, pitch, 3, 2, 0, 0, 8, &d, out) == 0);
    CHECK(out[0] == -2 && out[1] == 2 && out[2] == -1 && out[3] == -1 && out[4] == 32767 && out[5] == 32767);
    d.format = VP9HIP_RESID_YUV_F16;
    CHECK(vp9hip_residual_scaled_host(pl, pitch, 3, 2, 0, 0, 8, &d, out) == 0);
    // -2 / 255 = -0.0078431 = -0x1.010102p-7 -> half 0xA004; 2 / 255 -> 0x2004; -1 / 255 -> 0x9C04; 32767 / 255 = 128.498 -> 0x5804
    const uint16_t *ob = (const uint16_t *) out;
    CHECK(ob[0] == 0xA004 && ob[1] == 0x2004 && ob[2] == 0x9C04 && ob[3] == 0x9C04 && ob[4] == 0x5804 && ob[5] == 0x5804);
    g_free(&go);
    // a pitch of its own: rows 16 bytes apart, the gap untouched
    d.format = VP9HIP_RESID_YUV_I16; d.pitch = 16;
    out = g_alloc(&go, 48);
    CHECK(vp9hip_residual_scaled_host(pl, pitch, 3, 2, 0, 0, 8, &d, out) == 0);
    CHECK(out[0] == -2 && out[1] == 2 && out[8] == -1 && out[9] == -1 && out[16] == 32767 && out[17] == 32767);
    for (int i = 0; i < 24; i++)
        if ((i & 7) > 1) CHECK((uint16_t) out[i] == 0xC3C3);
    g_free(&go);
    for (int p = 0; p < 3; p++) g_free(&gp[p]);
}

// A refused call leaves the output as it was.
static void refused(void)
{
    const int16_t px[4] = { 1, 2, 3, 4 };
    const int16_t *pl[3] = { px, px, px };
    const ptrdiff_t pitch[3] = { 2, 2, 2 };
    guarded go;
    int16_t *out = g_alloc(&go, 64);
    const vp9hip_resid_desc ok = { VP9HIP_RESID_RGB_I16, 2, 0, 1, 1, 0, 0 };
    vp9hip_resid_desc d;
#define REFUSED(w, h, sh, sv, bpp, mod) do { d = ok; mod; CHECK(vp9hip_residual_scaled_host(pl, pitch, w, h, sh, sv, bpp, &d, out) == VP9HIP_EINVAL); } while (0)
    REFUSED(0, 2, 0, 0, 8, (void) 0);
    REFUSED(2, 16385, 0, 0, 8, (void) 0);
    REFUSED(2, 2, 2, 0, 8, (void) 0);
    REFUSED(2, 2, 0, -1, 8, (void) 0);
    REFUSED(2, 2, 0, 0, 9, (void) 0);
    REFUSED(2, 2, 0, 0, 8, d.format = 4);
    REFUSED(2, 2, 0, 0, 8, d.format = -1);
    REFUSED(2, 2, 0, 0, 8, d.colorspace = 0);
    REFUSED(2, 2, 0, 0, 8, d.colorspace = 6);
    REFUSED(2, 2, 0, 0, 8, d.out_width = 0);
    REFUSED(2, 2, 0, 0, 8, d.out_height = 16385);
    REFUSED(2, 2, 0, 0, 8, d.pitch = 1);
    REFUSED(2, 2, 0, 0, 8, d.pitch = 24);
    REFUSED(2, 2, 0, 0, 8, d.frame_stride = 4);
    REFUSED(2, 2, 0, 0, 8, d.frame_stride = 7);
    CHECK(vp9hip_residual_scaled_host(NULL, pitch, 2, 2, 0, 0, 8, &ok, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_residual_scaled_host(pl, NULL, 2, 2, 0, 0, 8, &ok, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_residual_scaled_host(pl, pitch, 2, 2, 0, 0, 8, NULL, out) == VP9HIP_EINVAL);
    CHECK(vp9hip_residual_scaled_host(pl, pitch, 2, 2, 0, 0, 8, &ok, NULL) == VP9HIP_EINVAL);
    CHECK(vp9hip_residual_scaled_host(pl, pitch, 2, 2, 0, 0, 8, &ok, (uint8_t *) out + 1) == VP9HIP_EINVAL);
    for (int i = 0; i < 32; i++) CHECK((uint16_t) out[i] == 0xC3C3);
    g_free(&go);
}

int main(void)
{
    refused();
    by_hand();
    for (int ss = 0; ss < 4; ss++) {
        constant_case(1, 1, 8, ss & 1, ss >> 1, -255, 7, -7, 1, 1, 2, 0);
        constant_case(1, 1, 12, ss & 1, ss >> 1, 32767, -32768, 32767, 1, 1, 5, 0);
        constant_case(16384, 1, 10, ss & 1, ss >> 1, -32768, 32767, -32768, 1, 1, 2, 1);
        constant_case(1, 16384, 10, ss & 1, ss >> 1, 32767, 32767, 32767, 1, 1, 1, 0);
    }
    constant_case(1, 1, 12, 1, 1, -4095, -4095, 0, 16384, 1, 5, 0);           // the widest upscale
    constant_case(1, 1, 8, 0, 0, 255, 0, 255, 1, 16384, 7, 1);
    constant_case(4096, 4096, 12, 0, 0, -32768, -32768, -32768, 3, 2, 5, 0);  // |A| = 2^15 * 2^24 an output... the largest sums
    constant_case(4096, 4096, 12, 1, 1, -32768, 32767, -32768, 3, 2, 2, 0);
    if (fails) { printf("residual_scaled_host_check: %d failures\n", fails); return 1; }
    printf("residual_scaled_host_check OK\n");
    return 0;
}
