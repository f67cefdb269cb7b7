/*
 * Residual tensors at model size, host side: the layout of the output and the C statement of
 * the definition (include/vp9hip.h "residual tensors at model size"). No device
 * code. The statement takes one output sample at a time, in 64-bit integers, straight from the
 * formulas: it is what a result can be reproduced from, and shares nothing with the kernel
 * (vp9hip_residual_scale.hip) but vp9hip_out_coefs.
 */
#include <string.h>

#include "../../../include/vp9hip.h"

int64_t vp9hip_resid_layout(const vp9hip_resid_desc *d, int64_t *pitch)
{
    if (!d || d->format < VP9HIP_RESID_YUV_I16 || d->format > VP9HIP_RESID_RGB_F16) return VP9HIP_EINVAL;
    if (d->out_width < 1 || d->out_width > 16384 || d->out_height < 1 || d->out_height > 16384) return VP9HIP_EINVAL;
    if (d->pitch < 0 || d->frame_stride < 0) return VP9HIP_EINVAL;
    const int64_t row = 2 * (int64_t) d->out_width;
    const int64_t p = d->pitch ? d->pitch : row;
    if (p < row || (p != row && (p & 15))) return VP9HIP_EINVAL;
    const int64_t bytes = 3 * p * d->out_height;
    if (d->frame_stride && (d->frame_stride < bytes || (d->frame_stride & 1))) return VP9HIP_EINVAL;
    if (pitch) *pitch = p;
    return bytes;
}

/* floor(a / b), b > 0 (C's division truncates toward zero) */
static int64_t floor_div(int64_t a, int64_t b)
{
    int64_t q = a / b;
    if (a % b < 0) q--;
    return q;
}

static int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t i64max(int64_t a, int64_t b) { return a > b ? a : b; }

/* sbox(P, ow, oh) at (ox, oy) of a w x h plane */
static int64_t sbox_at(const int16_t *P, ptrdiff_t pitch, int64_t w, int64_t h, int64_t ow, int64_t oh, int64_t ox, int64_t oy)
{
    const int64_t sx0 = ox * w / ow, sx1 = ((ox + 1) * w + ow - 1) / ow;
    const int64_t sy0 = oy * h / oh, sy1 = ((oy + 1) * h + oh - 1) / oh;
    int64_t A = 0;
    for (int64_t sy = sy0; sy < sy1; sy++) {
        const int64_t wy = i64min((oy + 1) * h, (sy + 1) * oh) - i64max(oy * h, sy * oh);
        int64_t row = 0;
        for (int64_t sx = sx0; sx < sx1; sx++) {
            const int64_t wx = i64min((ox + 1) * w, (sx + 1) * ow) - i64max(ox * w, sx * ow);
            row += wx * P[sy * pitch + sx];
        }
        A += wy * row;
    }
    return floor_div(A + (w * h >> 1), w * h);
}

static int64_t clip_pm(int64_t v, int64_t m) { return v < -m ? -m : v > m ? m : v; }

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

int vp9hip_residual_scaled_host(const int16_t *const planes[3], const ptrdiff_t pitch[3], int width, int height,
                                int ss_h, int ss_v, int bpp, const vp9hip_resid_desc *d, void *dst)
{
    if (!planes || !pitch || !planes[0] || !planes[1] || !planes[2] || !d || !dst || ((uintptr_t) dst & 1)) return VP9HIP_EINVAL;
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return VP9HIP_EINVAL;
    if (ss_h < 0 || ss_h > 1 || ss_v < 0 || ss_v > 1 || (bpp != 8 && bpp != 10 && bpp != 12)) return VP9HIP_EINVAL;
    int64_t op = 0;
    if (vp9hip_resid_layout(d, &op) < 0) return VP9HIP_EINVAL;
    const int rgb = d->format == VP9HIP_RESID_RGB_I16 || d->format == VP9HIP_RESID_RGB_F16;
    const int half = d->format == VP9HIP_RESID_YUV_F16 || d->format == VP9HIP_RESID_RGB_F16;
    int32_t c[5] = { 0 }, S = 0;
    if (rgb && vp9hip_out_coefs(d->colorspace, d->full_range, bpp, bpp, c, &S) < 0) return VP9HIP_EINVAL;
    const int64_t cw = (width + ss_h) >> ss_h, ch = (height + ss_v) >> ss_v;
    const int64_t OW = d->out_width, OH = d->out_height, m = ((int64_t) 1 << bpp) - 1;
    const float fscale = (float) (1.0 / (double) m);
    for (int64_t oy = 0; oy < OH; oy++)
        for (int64_t ox = 0; ox < OW; ox++) {
            const int64_t y = sbox_at(planes[0], pitch[0], width, height, OW, OH, ox, oy);
            const int64_t u = sbox_at(planes[1], pitch[1], cw, ch, OW, OH, ox, oy);
            const int64_t v = sbox_at(planes[2], pitch[2], cw, ch, OW, OH, ox, oy);
            int64_t o[3] = { y, u, v };
            if (rgb && d->colorspace == 7) {
                o[0] = clip_pm(v, m); o[1] = clip_pm(y, m); o[2] = clip_pm(u, m);
            } else if (rgb) {
                const int64_t rnd = (int64_t) 1 << (S - 1);
                /* >> of a negative int64_t is arithmetic with every compiler this builds with; floor_div says it outright */
                o[0] = clip_pm(floor_div(c[0] * y + c[1] * v + rnd, (int64_t) 1 << S), m);
                o[1] = clip_pm(floor_div(c[0] * y - c[2] * u - c[3] * v + rnd, (int64_t) 1 << S), m);
                o[2] = clip_pm(floor_div(c[0] * y + c[4] * u + rnd, (int64_t) 1 << S), m);
            }
            for (int p = 0; p < 3; p++) {
                uint8_t *q = (uint8_t *) dst + (p * OH + oy) * op + 2 * ox;
                uint16_t bits;
                if (half) {
                    volatile float f = (float) o[p] * fscale;        /* the float32 product, rounded once, a value of its own */
                    bits = half_bits(f);
                } else {
                    bits = (uint16_t) (int16_t) o[p];
                }
                memcpy(q, &bits, 2);
            }
        }
    return 0;
}
