/*
 * Accumulated residual at model size, host side: the layout of the output and the C statement of
 * the definition (include/vp9hip.h "accumulated residual at model size"). No
 * device code. The statement takes one output sample at a time, in 64-bit integers, straight
 * from the text of the definition and of the two sections it composes: every source sample of
 * an output's footprint is the clamped difference of a's sample and b's displaced one, weighted
 * by the box filter and floored. It calls neither vp9hip_acc_warp_host nor
 * vp9hip_residual_scaled_host (the tests hold it against their composition) and shares nothing
 * with the kernel (vp9hip_warp_scale.hip) but vp9hip_out_coefs. Built without -fwrapv by the
 * stand-alone check (tests/c/acc_warp_scaled_host_check.c): nothing here may overflow a signed
 * integer or shift a negative value.
 */
#include <string.h>

#include "../../../include/vp9hip.h"

int64_t vp9hip_warpt_layout(const vp9hip_warpt_desc *d, int64_t *pitch)
{
    if (!d || d->format < VP9HIP_RESID_YUV_I16 || d->format > VP9HIP_RESID_RGB_F16) return VP9HIP_EINVAL;
    if (d->planes != 3 && d->planes != 4) return VP9HIP_EINVAL;
    if (d->out_width < 1 || d->out_width > 16384 || d->out_height < 1 || d->out_height > 16384) return VP9HIP_EINVAL;
    if (d->pitch < 0 || d->frame_stride < 0) return VP9HIP_EINVAL;
    const int64_t row = 2 * (int64_t) d->out_width;
    const int64_t p = d->pitch ? d->pitch : row;
    if (p < row || (p != row && (p & 15))) return VP9HIP_EINVAL;
    const int64_t bytes = d->planes * p * d->out_height;
    if (d->frame_stride && (d->frame_stride < bytes || (d->frame_stride & 1))) return VP9HIP_EINVAL;
    if (pitch) *pitch = p;
    return bytes;
}

static int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t i64max(int64_t a, int64_t b) { return a > b ? a : b; }
static int64_t clampi(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : v > hi ? hi : v; }

/* floor(a / b), b > 0 (C's division truncates toward zero) */
static int64_t floor_div(int64_t a, int64_t b)
{
    int64_t q = a / b;
    if (a % b < 0) q--;
    return q;
}

typedef struct pair {
    const void *const *a, *const *b;
    const ptrdiff_t *la, *lb;
    const vp9hip_acc_cell *acc;
    uint32_t serial_b;
    int64_t w, h, gw;
    int hbd, ss_h, ss_v, mode;
} pair;

static int64_t px_at(const void *plane, ptrdiff_t linesize, int hbd, int64_t x, int64_t y)
{
    const uint8_t *row = (const uint8_t *) plane + y * linesize;
    return hbd ? ((const uint16_t *) row)[x] : row[x];
}

/* step 2 of "accumulated residual" for the cell of luma sample (x, y) */
static int applies(const pair *s, int64_t x, int64_t y)
{
    const vp9hip_acc_cell q = s->acc[(y / 4) * s->gw + x / 4];
    return q.hops > 0 && q.root == s->serial_b;
}

/* R_p[y][x]: steps 1-6 of "accumulated residual" for one sample of plane p */
static int64_t resid_at(const pair *s, int p, int64_t x, int64_t y)
{
    const int sh = p ? s->ss_h : 0, sv = p ? s->ss_v : 0;
    const int64_t pw = (s->w + sh) >> sh, ph = (s->h + sv) >> sv;
    const vp9hip_acc_cell q = s->acc[(y * (1 << sv) / 4) * s->gw + x * (1 << sh) / 4];
    if (!(q.hops > 0 && q.root == s->serial_b)) return 0;
    const int64_t Px = clampi(q.dx, -32768, 32767) * (2 >> sh), Py = clampi(q.dy, -32768, 32767) * (2 >> sv);
    int64_t pred;
    if (s->mode == VP9HIP_WARP_NEAREST) {
        pred = px_at(s->b[p], s->lb[p], s->hbd, clampi(x + floor_div(Px + 8, 16), 0, pw - 1),
                     clampi(y + floor_div(Py + 8, 16), 0, ph - 1));
    } else {
        const int64_t x0 = x + floor_div(Px, 16), y0 = y + floor_div(Py, 16);
        const int64_t fx = Px - 16 * floor_div(Px, 16), fy = Py - 16 * floor_div(Py, 16);
        const int64_t xa = clampi(x0, 0, pw - 1), xb = clampi(x0 + 1, 0, pw - 1);
        const int64_t ya = clampi(y0, 0, ph - 1), yb = clampi(y0 + 1, 0, ph - 1);
        pred = ((16 - fx) * (16 - fy) * px_at(s->b[p], s->lb[p], s->hbd, xa, ya) +
                fx * (16 - fy) * px_at(s->b[p], s->lb[p], s->hbd, xb, ya) +
                (16 - fx) * fy * px_at(s->b[p], s->lb[p], s->hbd, xa, yb) +
                fx * fy * px_at(s->b[p], s->lb[p], s->hbd, xb, yb) + 128) / 256;
    }
    return clampi(px_at(s->a[p], s->la[p], s->hbd, x, y) - pred, -32768, 32767);
}

/* sbox(., ow, oh) at (ox, oy) of plane p's residual (p < 3) or of 256 applies (p == 3, over luma) */
static int64_t sbox_at(const pair *s, int p, int64_t ow, int64_t oh, int64_t ox, int64_t oy)
{
    const int sh = p == 1 || p == 2 ? s->ss_h : 0, sv = p == 1 || p == 2 ? s->ss_v : 0;
    const int64_t w = (s->w + sh) >> sh, h = (s->h + sv) >> sv;
    const int64_t sx0 = ox * w / ow, sx1 = ((ox + 1) * w + ow - 1) / ow;
    const int64_t sy0 = oy * h / oh, sy1 = ((oy + 1) * h + oh - 1) / oh;
    int64_t A = 0;
    for (int64_t sy = sy0; sy < sy1; sy++) {
        const int64_t wy = i64min((oy + 1) * h, (sy + 1) * oh) - i64max(oy * h, sy * oh);
        int64_t row = 0;
        for (int64_t sx = sx0; sx < sx1; sx++) {
            const int64_t wx = i64min((ox + 1) * w, (sx + 1) * ow) - i64max(ox * w, sx * ow);
            row += wx * (p == 3 ? 256 * applies(s, sx, sy) : resid_at(s, p, sx, sy));
        }
        A += wy * row;
    }
    return floor_div(A + w * h / 2, w * h);
}

/* float -> half bits, round to nearest even (any finite float) */
static uint16_t half_bits(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint16_t sign = (uint16_t) (u >> 16 & 0x8000);
    u &= 0x7fffffff;
    if (u >= 0x47800000) return (uint16_t) (sign | 0x7c00);          /* 65536 and above: infinity */
    if (u < 0x38800000) {                                            /* below 2^-14: a subnormal half */
        float a, half = 0.5f;
        uint32_t hb, ab;
        memcpy(&a, &u, 4);
        a += half;                                                   /* the FPU rounds at the half's last bit */
        memcpy(&ab, &a, 4);
        memcpy(&hb, &half, 4);
        return (uint16_t) (sign | (ab - hb));
    }
    u += 0xfff + (u >> 13 & 1);
    return (uint16_t) (sign | ((u - ((uint32_t) 112 << 23)) >> 13));
}

int vp9hip_acc_warp_scaled_host(const void *const a[3], const ptrdiff_t linesize_a[3],
                                const void *const b[3], const ptrdiff_t linesize_b[3],
                                const vp9hip_acc_cell *acc, uint32_t serial_b, int bpp, int ss_h, int ss_v,
                                const vp9hip_warpt_desc *d, void *dst)
{
    if (!a || !b || !linesize_a || !linesize_b || !acc || !d || !dst || ((uintptr_t) dst & 1)) return VP9HIP_EINVAL;
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384) return VP9HIP_EINVAL;
    if (ss_h < 0 || ss_h > 1 || ss_v < 0 || ss_v > 1 || (bpp != 8 && bpp != 10 && bpp != 12)) return VP9HIP_EINVAL;
    if (d->mode != VP9HIP_WARP_NEAREST && d->mode != VP9HIP_WARP_BILINEAR) return VP9HIP_EINVAL;
    for (int p = 0; p < 3; p++)
        if (!a[p] || !b[p]) return VP9HIP_EINVAL;
    int64_t op = 0;
    if (vp9hip_warpt_layout(d, &op) < 0) return VP9HIP_EINVAL;
    const int rgb = d->format == VP9HIP_RESID_RGB_I16 || d->format == VP9HIP_RESID_RGB_F16;
    const int half = d->format == VP9HIP_RESID_YUV_F16 || d->format == VP9HIP_RESID_RGB_F16;
    int32_t c[5] = { 0 }, S = 0;
    if (rgb && vp9hip_out_coefs(d->colorspace, d->full_range, bpp, bpp, c, &S) < 0) return VP9HIP_EINVAL;
    const pair s = { a, b, linesize_a, linesize_b, acc, serial_b, d->width, d->height, 2 * ((d->width + 7) >> 3),
                     bpp > 8, ss_h, ss_v, d->mode };
    const int64_t OW = d->out_width, OH = d->out_height, m = ((int64_t) 1 << bpp) - 1;
    const float fscale = (float) (1.0 / (double) m), cscale = 1.0f / 256;
    for (int64_t oy = 0; oy < OH; oy++)
        for (int64_t ox = 0; ox < OW; ox++) {
            const int64_t y = sbox_at(&s, 0, OW, OH, ox, oy), u = sbox_at(&s, 1, OW, OH, ox, oy),
                          v = sbox_at(&s, 2, OW, OH, ox, oy);
            int64_t o[4] = { y, u, v, 0 };
            if (rgb && d->colorspace == 7) {
                o[0] = clampi(v, -m, m); o[1] = clampi(y, -m, m); o[2] = clampi(u, -m, m);
            } else if (rgb) {
                const int64_t rnd = (int64_t) 1 << (S - 1), den = (int64_t) 1 << S;
                o[0] = clampi(floor_div(c[0] * y + c[1] * v + rnd, den), -m, m);
                o[1] = clampi(floor_div(c[0] * y - c[2] * u - c[3] * v + rnd, den), -m, m);
                o[2] = clampi(floor_div(c[0] * y + c[4] * u + rnd, den), -m, m);
            }
            if (d->planes == 4) o[3] = sbox_at(&s, 3, OW, OH, ox, oy);
            for (int p = 0; p < d->planes; p++) {
                uint8_t *q = (uint8_t *) dst + (p * OH + oy) * op + 2 * ox;
                uint16_t bits;
                if (half) {
                    volatile float f = (float) o[p] * (p == 3 ? cscale : fscale);   /* the float32 product, rounded once */
                    bits = half_bits(f);
                } else {
                    bits = (uint16_t) (int16_t) o[p];
                }
                memcpy(q, &bits, 2);
            }
        }
    return 0;
}
