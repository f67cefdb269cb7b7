/* vp9hip_acc_warp_scaled_host at its edges: the accumulated residual at model size of
 * include/vp9hip.h on the host, where the sanitizer builds can watch it
 * (make -C ffmpeg-hybrid_amd/csrc acc_warp_scaled_host_check; built without -fwrapv, so a signed
 * overflow or a shift of a negative value is a finding). The extreme vectors and codes of
 * acc_warp_host_check.c (+-32767, -32768, INT32_MAX / INT32_MIN from every cell, stored codes of
 * 65535), sizes 1 x 1 up to 16384 x 9 and 7 x 16384, output sizes 1 x 1 and 16384 x 1 among
 * others, every subsampling, three depths, both modes, the four formats, with and without the
 * coverage. The planes and the field are exact-size heap blocks (ASan sees a read past the
 * visible size), the output sits between guard bytes (every build), and every output sample is
 * compared with a second statement written here, arranged another way: the full-size residual
 * planes first, then the unsigned form of the box (sign bit flipped, column sums, one floor of a
 * non-negative quotient), the matrix with a division, the half through frexp / nearbyint. No
 * device, no Python. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

#define GUARD 64

static int fails;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "acc_warp_scaled_host_check: %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
/* floor(v / d), d > 0, spelled without a shift of a negative value */
static int64_t fl(int64_t v, int64_t d) { int64_t q = v / d; return (v % d != 0 && v < 0) ? q - 1 : q; }

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

/* box(P, ow, oh) of an unsigned w x h plane: column sums of each output row, then the row */
static void ubox(const uint16_t *P, int64_t w, int64_t h, int64_t ow, int64_t oh, int64_t *out)
{
    uint64_t *col = malloc((size_t) w * sizeof(*col));
    for (int64_t oy = 0; oy < oh; oy++) {
        memset(col, 0, (size_t) w * sizeof(*col));
        for (int64_t sy = oy * h / oh; sy * oh < (oy + 1) * h; sy++) {
            const int64_t lo = sy * oh > oy * h ? sy * oh : oy * h, hi = (sy + 1) * oh < (oy + 1) * h ? (sy + 1) * oh : (oy + 1) * h;
            for (int64_t x = 0; x < w; x++) col[x] += (uint64_t) (hi - lo) * P[sy * w + x];
        }
        for (int64_t ox = 0; ox < ow; ox++) {
            uint64_t A = 0;
            for (int64_t sx = ox * w / ow; sx * ow < (ox + 1) * w; sx++) {
                const int64_t lo = sx * ow > ox * w ? sx * ow : ox * w, hi = (sx + 1) * ow < (ox + 1) * w ? (sx + 1) * ow : (ox + 1) * w;
                A += (uint64_t) (hi - lo) * col[sx];
            }
            out[oy * ow + ox] = (int64_t) ((A + (uint64_t) (w * h / 2)) / (uint64_t) (w * h));
        }
    }
    free(col);
}

/* the half nearest to f, ties to even, by value */
static uint16_t half_of(float f)
{
    const uint16_t sign = signbit(f) ? 0x8000 : 0;
    const double v = fabs((double) f);
    if (v == 0) return sign;
    int e;
    frexp(v, &e);                                                     /* v = m 2^e, 0.5 <= m < 1 */
    const double quantum = ldexp(1.0, e - 1 >= -14 ? e - 11 : -24);
    const double r = nearbyint(v / quantum) * quantum;                /* the default rounding mode: to nearest even */
    if (r >= 65536.0) return (uint16_t) (sign | 0x7c00);
    if (r < ldexp(1.0, -14)) return (uint16_t) (sign | (uint16_t) (r / ldexp(1.0, -24)));
    frexp(r, &e);
    return (uint16_t) (sign | ((e - 1 + 15) << 10) | ((int) (r / ldexp(1.0, e - 11)) - 1024));
}

/* One pair of w x h at the given depth and subsampling, top: the largest stored code, to ow x oh. */
static void pair(int w, int h, int bpp, int ss_h, int ss_v, uint32_t top, int ow, int oh, int variant)
{
    const int hbd = bpp > 8;
    const int64_t gw = 2 * ((w + 7) >> 3), gh = 2 * ((h + 7) >> 3);
    void *a[3], *b[3];
    ptrdiff_t ls[3];
    int64_t pw[3], ph[3];
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
    vp9hip_acc_cell *acc = malloc((size_t) (gw * gh) * sizeof(*acc));
    const uint32_t sb = 0xfffffff0u;
    for (int64_t i = 0; i < gw * gh; i++) {
        acc[i].dx = ext[(i + i / gw) % NEXT]; acc[i].dy = ext[(3 * i + i / gw) % NEXT];
        acc[i].root = i % 5 == 0 ? sb - 1 : i % 7 == 0 ? 0 : sb;
        acc[i].hops = (uint16_t) (i % 11 == 0 ? 0 : i % 3 == 0 ? 65535 : 1 + i % 9);
        acc[i].end = (uint8_t) (i % 3); acc[i].pad = 0;
    }
    const int64_t m = ((int64_t) 1 << bpp) - 1, no = (int64_t) ow * oh;
    uint16_t *flip = malloc((size_t) w * h * 2);
    int64_t *res[4];
    for (int p = 0; p < 4; p++) res[p] = malloc((size_t) no * sizeof(int64_t));
    for (int mode = VP9HIP_WARP_NEAREST; mode <= VP9HIP_WARP_BILINEAR; mode++) {
        /* the second statement: R_p + 32768 at full size, then its box */
        for (int p = 0; p < 4; p++) {
            const int q3 = p == 3, sh = p && !q3 ? ss_h : 0, sv = p && !q3 ? ss_v : 0;
            const int64_t W = q3 ? w : pw[p], H = q3 ? h : ph[p];
            for (int64_t y = 0; y < H; y++)
                for (int64_t x = 0; x < W; x++) {
                    const vp9hip_acc_cell *q = &acc[((sv ? 2 * y : y) / 4) * gw + (sh ? 2 * x : x) / 4];
                    const int app = q->hops > 0 && q->root == sb;
                    if (q3) { flip[y * W + x] = (uint16_t) (app ? 256 : 0); continue; }
                    int64_t r = 0;
                    if (app) {
                        const int64_t px = clampl(q->dx, -32768, 32767) * (sh ? 1 : 2), py = clampl(q->dy, -32768, 32767) * (sv ? 1 : 2);
                        int64_t pred;
                        if (mode == VP9HIP_WARP_NEAREST) {
                            pred = get(b[p], hbd, W, clampl(x + fl(px + 8, 16), 0, W - 1), clampl(y + fl(py + 8, 16), 0, H - 1));
                        } else {
                            const int64_t x0 = x + fl(px, 16), y0 = y + fl(py, 16), fx = px - 16 * fl(px, 16), fy = py - 16 * fl(py, 16);
                            const int64_t xa = clampl(x0, 0, W - 1), xb = clampl(x0 + 1, 0, W - 1);
                            const int64_t ya = clampl(y0, 0, H - 1), yb = clampl(y0 + 1, 0, H - 1);
                            const int64_t top_row = (16 - fx) * get(b[p], hbd, W, xa, ya) + fx * get(b[p], hbd, W, xb, ya);
                            const int64_t bot_row = (16 - fx) * get(b[p], hbd, W, xa, yb) + fx * get(b[p], hbd, W, xb, yb);
                            pred = ((16 - fy) * top_row + fy * bot_row + 128) / 256;
                        }
                        r = clampl(get(a[p], hbd, W, x, y) - pred, -32768, 32767);
                    }
                    flip[y * W + x] = (uint16_t) (r + 32768);
                }
            ubox(flip, W, H, ow, oh, res[p]);
            if (!q3)
                for (int64_t i = 0; i < no; i++) res[p][i] -= 32768;
        }
        for (int k = 0; k < 2; k++) {
            /* two of the eight (format, planes) combinations a call, all eight over the variants */
            const int format = (variant + 2 * k + mode) & 3, planes = 3 + ((variant + k + (mode ^ (variant >> 2))) & 1);
            const int cs = (variant % 3 == 2) ? 7 : 1 + (variant + k) % 5, full = (variant >> 1) & 1;
            const int64_t row = 2 * (int64_t) ow, pitch = (variant & 1) && ow < 4096 ? (row + 31) & ~(int64_t) 15 : row;
            vp9hip_warpt_desc d = { format, cs, full, mode, planes, w, h, ow, oh, pitch == row ? 0 : pitch, 0 };
            int64_t gotp = 0;
            const int64_t bytes = vp9hip_warpt_layout(&d, &gotp);
            CHECK(bytes == planes * pitch * oh && gotp == pitch);
            uint8_t *dg = malloc((size_t) bytes + 2 * GUARD);
            memset(dg, 0xa5, (size_t) bytes + 2 * GUARD);
            CHECK(vp9hip_acc_warp_scaled_host((const void *const *) a, ls, (const void *const *) b, ls, acc, sb, bpp, ss_h, ss_v,
                                              &d, dg + GUARD) == 0);
            for (int i = 0; i < GUARD; i++) CHECK(dg[i] == 0xa5 && dg[GUARD + bytes + i] == 0xa5);
            int32_t c[5] = { 0 }, S = 0;
            if (format & 2) CHECK(vp9hip_out_coefs(cs, full, bpp, bpp, c, &S) == 0);
            uint64_t bad = 0;
            for (int64_t oy = 0; oy < oh; oy++) {
                for (int64_t ox = 0; ox < ow; ox++) {
                    const int64_t i = oy * ow + ox, y = res[0][i], u = res[1][i], v = res[2][i];
                    int64_t o[4] = { y, u, v, res[3][i] };
                    if ((format & 2) && cs == 7) {
                        o[0] = clampl(v, -m, m); o[1] = clampl(y, -m, m); o[2] = clampl(u, -m, m);
                    } else if (format & 2) {
                        const int64_t den = (int64_t) 1 << S;
                        o[0] = clampl(fl(c[0] * y + c[1] * v + den / 2, den), -m, m);
                        o[1] = clampl(fl(c[0] * y - c[2] * u - c[3] * v + den / 2, den), -m, m);
                        o[2] = clampl(fl(c[0] * y + c[4] * u + den / 2, den), -m, m);
                    }
                    for (int p = 0; p < planes; p++) {
                        uint16_t got, want;
                        memcpy(&got, dg + GUARD + (p * oh + oy) * pitch + 2 * ox, 2);
                        if (format & 1) {
                            volatile float f = (float) o[p] * (p == 3 ? 1.0f / 256 : (float) (1.0 / (double) m));
                            want = half_of(f);
                        } else {
                            want = (uint16_t) (int16_t) o[p];
                        }
                        bad += got != want;
                    }
                }
                /* the pitch's padding is not written */
                for (int p = 0; p < planes; p++)
                    for (int64_t x = row; x < pitch; x++) bad += dg[GUARD + (p * oh + oy) * pitch + x] != 0xa5;
            }
            CHECK(bad == 0);
            free(dg);
        }
    }
    for (int p = 0; p < 4; p++) free(res[p]);
    free(flip); free(acc);
    for (int p = 0; p < 3; p++) { free(a[p]); free(b[p]); }
}

int main(void)
{
    /* source size, output size */
    static const int cases[][4] = { { 1, 1, 1, 1 }, { 1, 1, 16384, 1 }, { 1, 9, 1, 1 }, { 1, 9, 3, 20 }, { 5, 3, 1, 1 }, { 5, 3, 5, 3 },
                                    { 5, 3, 16384, 1 }, { 24, 16, 7, 5 }, { 24, 16, 49, 20 }, { 66, 34, 1, 1 }, { 66, 34, 17, 9 },
                                    { 66, 34, 16384, 1 }, { 16384, 9, 1, 1 }, { 16384, 9, 16384, 1 }, { 16384, 9, 224, 3 },
                                    { 7, 16384, 1, 1 }, { 7, 16384, 2, 224 } };
    int variant = 0;
    for (unsigned s = 0; s < sizeof(cases) / sizeof(cases[0]); s++)
        for (int ss = 0; ss < 4; ss++) {
            /* the 16384-sample extremes take one depth a subsampling, each depth in turn, to stay quick */
            const int big = cases[s][0] * cases[s][1] > 100000, only = (int) (s + ss) % 3;
            if (!big || only == 0) pair(cases[s][0], cases[s][1], 8, ss & 1, ss >> 1, 255, cases[s][2], cases[s][3], variant++);
            if (!big || only == 1) pair(cases[s][0], cases[s][1], 10, ss & 1, ss >> 1, 1023, cases[s][2], cases[s][3], variant++);
            if (!big || only == 2)                                      /* stored codes beyond the depth */
                pair(cases[s][0], cases[s][1], 12, ss & 1, ss >> 1, 65535, cases[s][2], cases[s][3], variant++);
        }

    /* the int16 clamp of the residual, both ways, through the mean and the RGB clip; the coverage's ends */
    {
        uint16_t hi[16], lo[16];
        for (int i = 0; i < 16; i++) { hi[i] = 65535; lo[i] = 0; }
        const void *const ph[3] = { hi, hi, hi }, *const pl[3] = { lo, lo, lo };
        const ptrdiff_t ls[3] = { 8, 8, 8 };
        vp9hip_acc_cell acc[4];
        memset(acc, 0, sizeof(acc));
        for (int i = 0; i < 4; i++) { acc[i].root = 3; acc[i].hops = 1; }
        int16_t out[4 * 6];
        vp9hip_warpt_desc d = { VP9HIP_RESID_YUV_I16, 2, 0, VP9HIP_WARP_BILINEAR, 4, 4, 4, 3, 2, 0, 0 };
        CHECK(vp9hip_acc_warp_scaled_host(ph, ls, pl, ls, acc, 3, 12, 0, 0, &d, out) == 0);
        for (int i = 0; i < 24; i++) CHECK(out[i] == (i < 18 ? 32767 : 256));
        d.mode = VP9HIP_WARP_NEAREST;
        CHECK(vp9hip_acc_warp_scaled_host(pl, ls, ph, ls, acc, 3, 12, 0, 0, &d, out) == 0);
        for (int i = 0; i < 24; i++) CHECK(out[i] == (i < 18 ? -32768 : 256));
        d.format = VP9HIP_RESID_RGB_I16;
        CHECK(vp9hip_acc_warp_scaled_host(pl, ls, ph, ls, acc, 3, 12, 0, 0, &d, out) == 0);
        for (int i = 0; i < 18; i++) CHECK(out[i] == -4095 || (i >= 6 && i < 12));    /* G: Y - U - V, whatever it is */
        CHECK(vp9hip_acc_warp_scaled_host(pl, ls, ph, ls, acc, 4, 12, 0, 0, &d, out) == 0);   /* another serial: nothing applies */
        for (int i = 0; i < 24; i++) CHECK(out[i] == 0);

        /* bad arguments: refused, and nothing written */
        memset(out, 0x5a, sizeof(out));
        int16_t ref[24];
        memset(ref, 0x5a, sizeof(ref));
        const vp9hip_warpt_desc good = { VP9HIP_RESID_RGB_F16, 2, 0, VP9HIP_WARP_NEAREST, 4, 4, 4, 3, 2, 0, 0 };
#define REFUSED(A, LA, B, LB, ACC, BPP, SH, SV, D, DST) \
        CHECK(vp9hip_acc_warp_scaled_host(A, LA, B, LB, ACC, 3, BPP, SH, SV, D, DST) == VP9HIP_EINVAL)
        REFUSED(NULL, ls, ph, ls, acc, 12, 0, 0, &good, out);
        REFUSED(pl, NULL, ph, ls, acc, 12, 0, 0, &good, out);
        REFUSED(pl, ls, NULL, ls, acc, 12, 0, 0, &good, out);
        REFUSED(pl, ls, ph, NULL, acc, 12, 0, 0, &good, out);
        REFUSED(pl, ls, ph, ls, NULL, 12, 0, 0, &good, out);
        REFUSED(pl, ls, ph, ls, acc, 12, 0, 0, NULL, out);
        REFUSED(pl, ls, ph, ls, acc, 12, 0, 0, &good, NULL);
        REFUSED(pl, ls, ph, ls, acc, 12, 0, 0, &good, (uint8_t *) out + 1);
        REFUSED(pl, ls, ph, ls, acc, 9, 0, 0, &good, out);
        REFUSED(pl, ls, ph, ls, acc, 12, 2, 0, &good, out);
        REFUSED(pl, ls, ph, ls, acc, 12, 0, -1, &good, out);
        const void *const hole[3] = { lo, NULL, lo };
        REFUSED(hole, ls, ph, ls, acc, 12, 0, 0, &good, out);
        REFUSED(pl, ls, hole, ls, acc, 12, 0, 0, &good, out);
        CHECK(vp9hip_acc_warp_scaled_host(pl, ls, ph, ls, acc, 3, 12, 0, 0, &good, out) == 0);
        memset(out, 0x5a, sizeof(out));
        vp9hip_warpt_desc e;
#define BAD_DESC(field, value) do { e = good; e.field = (value); REFUSED(pl, ls, ph, ls, acc, 12, 0, 0, &e, out); } while (0)
        BAD_DESC(format, -1); BAD_DESC(format, 4); BAD_DESC(colorspace, 0); BAD_DESC(colorspace, 6); BAD_DESC(colorspace, 8);
        BAD_DESC(mode, -1); BAD_DESC(mode, 2); BAD_DESC(planes, 2); BAD_DESC(planes, 5); BAD_DESC(planes, 0);
        BAD_DESC(width, 0); BAD_DESC(width, 16385); BAD_DESC(height, 0); BAD_DESC(height, 16385);
        BAD_DESC(out_width, 0); BAD_DESC(out_width, 16385); BAD_DESC(out_height, 0); BAD_DESC(out_height, 16385);
        BAD_DESC(pitch, 4); BAD_DESC(pitch, 24); BAD_DESC(pitch, -16); BAD_DESC(frame_stride, 46); BAD_DESC(frame_stride, 49);
        BAD_DESC(frame_stride, -2);
        CHECK(!memcmp(out, ref, sizeof(out)));
        e = good; e.format = VP9HIP_RESID_YUV_F16; e.colorspace = 0;          /* the YUV formats do not look at the colour space */
        CHECK(vp9hip_acc_warp_scaled_host(pl, ls, ph, ls, acc, 3, 12, 0, 0, &e, out) == 0);
        e = good; e.pitch = 16; e.frame_stride = 4 * 16 * 2 + 2;
        CHECK(vp9hip_warpt_layout(&e, NULL) == 4 * 16 * 2);
        e.planes = 3;
        CHECK(vp9hip_warpt_layout(&e, NULL) == 3 * 16 * 2 && vp9hip_warpt_layout(NULL, NULL) == VP9HIP_EINVAL);
        e.out_width = e.out_height = 16384; e.pitch = e.frame_stride = 0; e.planes = 4;
        CHECK(vp9hip_warpt_layout(&e, NULL) == 8ll * 16384 * 16384);
    }
    if (fails) { fprintf(stderr, "acc_warp_scaled_host_check: %d checks failed\n", fails); return 1; }
    printf("acc_warp_scaled_host_check OK\n");
    return 0;
}
