/* vp9hip_acc_propagate_host at its edges: the accumulated propagation of include/vp9hip.h on the
 * host, where the sanitizer builds can watch it (make -C ffmpeg-hybrid_amd/csrc
 * acc_propagate_host_check; built without -fwrapv, so a signed overflow or a shift of a negative
 * value is a finding). Extreme vectors (+-32767, -32768, INT32_MAX / INT32_MIN) from every cell,
 * 16384-sample grids at C = 1, 1 x 1 grids, pictures 1 sample wide and 16384 wide, every element
 * size, both layouts and modes, fill and keep. The field, the source and the pre-filled
 * destination are exact-size heap blocks (ASan sees a read past them), the destination and the
 * valid map sit between guard bytes (every build), and every element is compared with a second
 * statement written here (its binary16 conversions go through ldexp and nearbyint, not through
 * the integers of the library's). No device, no Python. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/vp9hip.h"

#define GUARD 64

static int fails;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "acc_propagate_host_check: %s:%d: %s\n", __FILE__, __LINE__, #c); fails++; } } while (0)

static int64_t clampl(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }
/* floor(v / d), d > 0, spelled without a shift of a negative value */
static int64_t fld(int64_t v, int64_t d) { int64_t q = v / d; return (v % d != 0 && v < 0) ? q - 1 : q; }

static uint64_t rnd_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void)
{
    rnd_state = rnd_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t) (rnd_state >> 33);
}

static float h2f(uint16_t hv)
{
    const int e = (hv >> 10) & 31, m = hv & 0x3ff;
    const float a = e ? ldexpf((float) (m + 1024), e - 25) : ldexpf((float) m, -24);
    return (hv & 0x8000) ? -a : a;
}

static uint16_t f2h(float f)
{
    const uint16_t sign = signbit(f) ? 0x8000 : 0;
    const double a = fabs((double) f);
    if (a == 0) return sign;
    int e;
    frexp(a, &e);                                        /* a = m 2^e, m in [0.5, 1) */
    int q = e - 1 < -14 ? -24 : e - 11;                  /* the exponent of the half's last place */
    double r = nearbyint(ldexp(a, -q));                  /* round to nearest even (the default mode) */
    if (q == -24) return (uint16_t) (sign | (uint16_t) r);
    if (r == 2048) { r = 1024; q++; }
    if (q + 25 >= 31) return (uint16_t) (sign | 0x7c00);
    return (uint16_t) (sign | (q + 25) << 10 | ((int) r - 1024));
}

static const int32_t ext[] = { 0, -1, -8, -9, 7, 8, 32767, -32767, -32768, INT32_MAX, INT32_MIN, 123, -4567 };
#define NEXT ((int) (sizeof(ext) / sizeof(ext[0])))

/* One pair: a w x h picture, an fw x fh grid of C channels of E bytes. */
static void pair(int w, int h, int fw, int fh, int C, int E, int layout, int mode, int keep)
{
    const int64_t gw = 2 * ((w + 7) >> 3), gh = 2 * ((h + 7) >> 3), plane = (int64_t) fw * fh;
    vp9hip_prop_desc d;
    memset(&d, 0, sizeof(d));
    d.width = w; d.height = h; d.fw = fw; d.fh = fh; d.channels = C; d.elem_size = E; d.layout = layout; d.mode = mode;
    d.flags = keep ? VP9HIP_PROP_KEEP : 0;
    d.fill = 0xf1e2d3c4b5a69788ull;
    int64_t vb = 0;
    const int64_t bytes = vp9hip_prop_layout(&d, &vb);
    CHECK(bytes == plane * C * E && vb == plane);
    vp9hip_acc_cell *acc = malloc((size_t) (gw * gh) * sizeof(*acc));
    const uint32_t S = 0xfffffff0u;
    for (int64_t i = 0; i < gw * gh; i++) {
        acc[i].dx = ext[(i + i / gw) % NEXT]; acc[i].dy = ext[(3 * i + i / gw) % NEXT];
        acc[i].root = i % 5 == 0 ? S - 1 : i % 7 == 0 ? 0 : S;
        acc[i].hops = (uint16_t) (i % 11 == 0 ? 0 : i % 3 == 0 ? 65535 : 1 + i % 9);
        acc[i].end = (uint8_t) (i % 3); acc[i].pad = 0;
    }
    uint8_t *src = malloc((size_t) bytes), *pre = malloc((size_t) bytes);
    for (int64_t i = 0; i < bytes; i++) { src[i] = (uint8_t) rnd(); pre[i] = (uint8_t) rnd(); }
    if (mode == VP9HIP_WARP_BILINEAR)                    /* finite halves, many of them subnormal */
        for (int64_t i = 0; i < bytes / 2; i++) {
            uint16_t v = (uint16_t) (rnd() % 0x7c00);
            if (rnd() % 4 == 0) v &= 0x03ff;
            if (rnd() & 1) v |= 0x8000;
            memcpy(src + 2 * i, &v, 2);
        }
    uint8_t *dg = malloc((size_t) bytes + 2 * GUARD), *vg = malloc((size_t) plane + 2 * GUARD);
    memset(dg, 0xa5, (size_t) bytes + 2 * GUARD);
    memset(vg, 0xa5, (size_t) plane + 2 * GUARD);
    memcpy(dg + GUARD, pre, (size_t) bytes);
    CHECK(vp9hip_acc_propagate_host(acc, S, &d, src, dg + GUARD, vg + GUARD) == 0);
    for (int i = 0; i < GUARD; i++)
        CHECK(dg[i] == 0xa5 && dg[GUARD + bytes + i] == 0xa5 && vg[i] == 0xa5 && vg[GUARD + plane + i] == 0xa5);
    uint64_t bad = 0;
    for (int64_t fy = 0; fy < fh; fy++)
        for (int64_t fx = 0; fx < fw; fx++) {
            const int64_t X = (2 * fx + 1) * w / (2 * fw), Y = (2 * fy + 1) * h / (2 * fh);
            const vp9hip_acc_cell *q = &acc[(Y / 4) * gw + X / 4];
            const int app = q->hops > 0 && q->root == S;
            bad += vg[GUARD + fy * fw + fx] != app;
            const int64_t px = fld(4 * clampl(q->dx, -32768, 32767) * fw + w, 2 * (int64_t) w);
            const int64_t py = fld(4 * clampl(q->dy, -32768, 32767) * fh + h, 2 * (int64_t) h);
            for (int64_t ch = 0; ch < C; ch++) {
#define AT(yy, xx) ((layout == VP9HIP_PROP_NHWC ? ((yy) * fw + (xx)) * C + ch : (ch * fh + (yy)) * fw + (xx)) * E)
                uint8_t want[8];
                if (!app) {
                    if (keep) memcpy(want, pre + AT(fy, fx), (size_t) E);
                    else for (int b = 0; b < E; b++) want[b] = (uint8_t) (d.fill >> (8 * b));
                } else if (mode == VP9HIP_WARP_NEAREST) {
                    memcpy(want, src + AT(clampl(fy + fld(py + 8, 16), 0, fh - 1), clampl(fx + fld(px + 8, 16), 0, fw - 1)), (size_t) E);
                } else {
                    const int64_t x0 = fx + fld(px, 16), y0 = fy + fld(py, 16);
                    const float frx = (float) (px - 16 * fld(px, 16)), fry = (float) (py - 16 * fld(py, 16));
                    const int64_t xa = clampl(x0, 0, fw - 1), xb = clampl(x0 + 1, 0, fw - 1);
                    const int64_t ya = clampl(y0, 0, fh - 1), yb = clampl(y0 + 1, 0, fh - 1);
                    uint16_t s[4];
                    memcpy(&s[0], src + AT(ya, xa), 2); memcpy(&s[1], src + AT(ya, xb), 2);
                    memcpy(&s[2], src + AT(yb, xa), 2); memcpy(&s[3], src + AT(yb, xb), 2);
                    const float top = (16 - frx) * h2f(s[0]) + frx * h2f(s[1]);
                    const float bot = (16 - frx) * h2f(s[2]) + frx * h2f(s[3]);
                    volatile float u0 = (16 - fry) * top, u1 = fry * bot;          /* each a binary32 of its own */
                    volatile float sum = u0 + u1;
                    const uint16_t r = f2h(sum * 0.00390625f);
                    memcpy(want, &r, 2);
                }
                bad += memcmp(want, dg + GUARD + AT(fy, fx), (size_t) E) != 0;
#undef AT
            }
        }
    CHECK(bad == 0);
    /* without a valid map */
    uint8_t *d2 = malloc((size_t) bytes);
    memcpy(d2, pre, (size_t) bytes);
    CHECK(vp9hip_acc_propagate_host(acc, S, &d, src, d2, NULL) == 0);
    CHECK(!memcmp(d2, dg + GUARD, (size_t) bytes));
    /* serial 0 never applies, also where a chain ended with root 0 */
    memcpy(d2, pre, (size_t) bytes);
    CHECK(vp9hip_acc_propagate_host(acc, 0, &d, src, d2, vg + GUARD) == 0);
    uint64_t any = 0;
    for (int64_t i = 0; i < plane; i++) any += vg[GUARD + i];
    CHECK(any == 0);
    if (keep) CHECK(!memcmp(d2, pre, (size_t) bytes));
    free(d2); free(dg); free(vg); free(src); free(pre); free(acc);
}

int main(void)
{
    static const int es[] = { 1, 2, 4, 8 };
    static const int shapes[][5] = { { 40, 24, 40, 24, 3 }, { 40, 24, 20, 12, 19 }, { 40, 24, 7, 5, 3 }, { 40, 24, 1, 1, 19 },
                                     { 40, 24, 83, 49, 1 }, { 1, 1, 1, 1, 1 }, { 1, 9, 5, 3, 3 }, { 13, 9, 6, 11, 3 },
                                     { 16384, 9, 16384, 2, 1 }, { 7, 16384, 3, 16384, 1 }, { 16384, 8, 1, 1, 1 },
                                     { 8, 8, 16384, 1, 1 }, { 1, 1, 16384, 3, 1 } };
    for (unsigned s = 0; s < sizeof(shapes) / sizeof(shapes[0]); s++)
        for (int e = 0; e < 4; e++)
            for (int v = 0; v < 4; v++) {
                pair(shapes[s][0], shapes[s][1], shapes[s][2], shapes[s][3], shapes[s][4], es[e], v & 1, VP9HIP_WARP_NEAREST, v >> 1);
                if (es[e] == 2)
                    pair(shapes[s][0], shapes[s][1], shapes[s][2], shapes[s][3], shapes[s][4], 2, v & 1, VP9HIP_WARP_BILINEAR, v >> 1);
            }

    /* bad arguments: refused, and nothing written */
    {
        vp9hip_acc_cell acc[4];
        memset(acc, 0, sizeof(acc));
        uint16_t src[12], out[12], ref[12];
        memset(src, 0, sizeof(src));
        memset(out, 0x5a, sizeof(out));
        memset(ref, 0x5a, sizeof(ref));
        const vp9hip_prop_desc good = { 8, 8, 2, 2, 3, 2, VP9HIP_PROP_NCHW, VP9HIP_WARP_NEAREST, 0, 0, 0 };
        CHECK(vp9hip_prop_layout(&good, NULL) == 24);
        vp9hip_prop_desc d;
#define BAD(field, value) do { d = good; d.field = value; CHECK(vp9hip_prop_layout(&d, NULL) == VP9HIP_EINVAL); \
                               CHECK(vp9hip_acc_propagate_host(acc, 1, &d, src, out, NULL) == VP9HIP_EINVAL); } while (0)
        BAD(width, 0); BAD(width, 16385); BAD(height, 0); BAD(height, 16385); BAD(fw, 0); BAD(fw, 16385); BAD(fh, 0); BAD(fh, 16385);
        BAD(channels, 0); BAD(channels, 4097); BAD(elem_size, 0); BAD(elem_size, 3); BAD(elem_size, 16); BAD(layout, 2); BAD(layout, -1);
        BAD(mode, 2); BAD(mode, -1); BAD(flags, 2); BAD(flags, -1); BAD(reserved, 1);
        d = good; d.mode = VP9HIP_WARP_BILINEAR; d.elem_size = 4;
        CHECK(vp9hip_prop_layout(&d, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_prop_layout(NULL, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_propagate_host(NULL, 1, &good, src, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_propagate_host(acc, 1, NULL, src, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_propagate_host(acc, 1, &good, NULL, out, NULL) == VP9HIP_EINVAL);
        CHECK(vp9hip_acc_propagate_host(acc, 1, &good, src, NULL, NULL) == VP9HIP_EINVAL);
        CHECK(!memcmp(out, ref, sizeof(out)));
        d = good; d.fw = d.fh = 16384; d.channels = 4096; d.elem_size = 8;
        CHECK(vp9hip_prop_layout(&d, NULL) == (int64_t) 1 << 43);
    }
    if (fails) { fprintf(stderr, "acc_propagate_host_check: %d checks failed\n", fails); return 1; }
    printf("acc_propagate_host_check OK\n");
    return 0;
}
