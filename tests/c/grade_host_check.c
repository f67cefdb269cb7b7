// vp9hip_grade_host (csrc/host/vp9h_grade.c): a stand-alone program, no device, no Python, built
// plain and with ASan + UBSan (without -fwrapv, so a signed overflow is a finding). The tables
// are exact-size heap blocks, so a read past entry 2^bpp - 1 or 4096 is a finding too. Checked:
// the table-free identity of include/vp9hip.h "Graded output" at 8, 10 and 12 bits over every
// code, both clips of the matrix stage, P = 65535 (which reads entry 4096), and the refusals.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

static int fails;
#define CHECK(c) do { if (!(c)) { printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static void *xmalloc(size_t n)
{
    void *p = malloc(n);
    if (!p) { printf("out of memory\n"); exit(2); }
    return p;
}

// in_lut[c] = c << (16 - bpp), m = 16384 I, out_lut[i] = min(16 i, 65535): v = c << (16 - bpp)
static void identity(int bpp)
{
    const int n = 1 << bpp;
    uint16_t *in = xmalloc(n * sizeof(*in)), *out = xmalloc(VP9HIP_GRADE_OUT_LUT * sizeof(*out));
    uint16_t *codes = xmalloc(3 * (size_t) n * sizeof(*codes)), *v = xmalloc(3 * (size_t) n * sizeof(*v));
    int32_t m[9] = { 16384, 0, 0, 0, 16384, 0, 0, 0, 16384 };
    for (int c = 0; c < n; c++) in[c] = (uint16_t) (c << (16 - bpp));
    for (int i = 0; i < VP9HIP_GRADE_OUT_LUT; i++) out[i] = (uint16_t) (16 * i < 65535 ? 16 * i : 65535);
    for (int c = 0; c < n; c++) {                          // every code in every channel, the others elsewhere
        codes[3 * c] = (uint16_t) c; codes[3 * c + 1] = (uint16_t) (n - 1 - c); codes[3 * c + 2] = (uint16_t) (c * 7 % n);
    }
    const vp9hip_grade_desc g = { bpp, 65535, in, m, out };
    CHECK(vp9hip_grade_host(&g, codes, n, v) == 0);
    int bad = 0;
    for (int i = 0; i < 3 * n; i++) bad += v[i] != codes[i] << (16 - bpp);
    CHECK(bad == 0);
    free(in); free(out); free(codes); free(v);
}

int main(void)
{
    identity(8); identity(10); identity(12);

    // the matrix stage's clips and rounding, read back through out_lut[i] = i (v = (P + 8) >> 4
    // between entries: out_lut is linear, so v = (16 i + f + 8) >> 4)
    uint16_t *in = xmalloc(256 * sizeof(*in)), *out = xmalloc(VP9HIP_GRADE_OUT_LUT * sizeof(*out));
    for (int c = 0; c < 256; c++) in[c] = (uint16_t) (c * 257);
    for (int i = 0; i < VP9HIP_GRADE_OUT_LUT; i++) out[i] = (uint16_t) i;
    {
        // row 0: -4 L_R (below 0: 0); row 1: 4 L_R + 4 L_G + 4 L_B (above 65535: 65535, entry 4096);
        // row 2: L_R / 2 + 1/16384 of L_G (the + 8192 and the floor)
        const int32_t m[9] = { -65536, 0, 0, 65536, 65536, 65536, 8192, 1, 0 };
        const vp9hip_grade_desc g = { 8, 65535, in, m, out };
        const uint16_t codes[9] = { 255, 255, 255, 1, 0, 0, 3, 255, 9 };
        uint16_t v[9];
        CHECK(vp9hip_grade_host(&g, codes, 3, v) == 0);
        CHECK(v[0] == 0);                                  // -4 * 65535
        CHECK(v[1] == 4096);                               // P = 65535: i = 4095, f = 15, (4095 + 15 * 4096 + 8) >> 4
        CHECK(v[2] == ((65535 / 2 + 4 + 8) >> 4));         // (65535 * 8192 + 65535 + 8192) >> 14 = 32771; (32771 + 8) >> 4
        CHECK(v[3] == 0);                                  // -4 * 257
        CHECK(v[4] == ((4 * 257 + 8) >> 4));
        CHECK(v[5] == ((129 + 8) >> 4));                   // (257 * 8192 + 8192) >> 14 = 129
        CHECK(v[6] == 0 && v[7] == 4096);
        CHECK(v[8] == (((3 * 257 * 8192 + 65535 + 8192) >> 14) + 8) >> 4);
        // the largest magnitudes: the sum passes 32 bits and no signed overflow is reported
        const int32_t mm[9] = { 65536, 65536, 65536, -65536, -65536, -65536, 65536, -65536, 65536 };
        const vp9hip_grade_desc gm = { 8, 65535, in, mm, out };
        CHECK(vp9hip_grade_host(&gm, codes, 1, v) == 0 && v[0] == 4096 && v[1] == 0 && v[2] == 4096);
        // the u8 output: entries above 255 are refused, at 255 accepted
        for (int i = 0; i < VP9HIP_GRADE_OUT_LUT; i++) out[i] = (uint16_t) (i >> 4 > 255 ? 255 : i >> 4);
        vp9hip_grade_desc g8 = { 8, 255, in, m, out };
        CHECK(vp9hip_grade_host(&g8, codes, 3, v) == 0 && v[1] == 255);
        out[4096] = 256;
        memset(v, 0xA5, sizeof(v));
        CHECK(vp9hip_grade_host(&g8, codes, 3, v) == VP9HIP_EINVAL);
        out[4096] = 255; out[0] = 256;
        CHECK(vp9hip_grade_host(&g8, codes, 3, v) == VP9HIP_EINVAL);
        out[0] = 0;
        // |m| > 2^16, either sign, any position
        for (int k = 0; k < 9; k++)
            for (int sgn = -1; sgn <= 1; sgn += 2) {
                int32_t mb[9];
                memcpy(mb, m, sizeof(mb));
                mb[k] = sgn * 65537;
                const vp9hip_grade_desc gb = { 8, 255, in, mb, out };
                CHECK(vp9hip_grade_host(&gb, codes, 3, v) == VP9HIP_EINVAL);
            }
        // the description itself, and a code beyond the depth
        g8.bpp = 9;      CHECK(vp9hip_grade_host(&g8, codes, 3, v) == VP9HIP_EINVAL); g8.bpp = 8;
        g8.out_max = 1023; CHECK(vp9hip_grade_host(&g8, codes, 3, v) == VP9HIP_EINVAL); g8.out_max = 255;
        g8.in_lut = NULL; CHECK(vp9hip_grade_host(&g8, codes, 3, v) == VP9HIP_EINVAL); g8.in_lut = in;
        CHECK(vp9hip_grade_host(NULL, codes, 3, v) == VP9HIP_EINVAL);
        CHECK(vp9hip_grade_host(&g8, NULL, 3, v) == VP9HIP_EINVAL);
        CHECK(vp9hip_grade_host(&g8, codes, -1, v) == VP9HIP_EINVAL);
        const uint16_t over[3] = { 0, 256, 0 };
        CHECK(vp9hip_grade_host(&g8, over, 1, v) == VP9HIP_EINVAL);
        for (int i = 0; i < 9; i++) CHECK(v[i] == 0xA5A5);  // a refused call writes nothing
        CHECK(vp9hip_grade_host(&g8, codes, 0, v) == 0);
    }
    free(in); free(out);
    if (fails) { printf("grade_host_check: %d failures\n", fails); return 1; }
    printf("grade_host_check OK\n");
    return 0;
}
