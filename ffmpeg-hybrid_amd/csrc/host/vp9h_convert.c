/*
 * Output conversion, host side: the layout of a converted frame and the integer colour
 * matrix (include/vp9hip.h, DESIGN.md "Output conversion"). No device code: the kernel
 * (vp9hip_convert.hip) takes what these two compute as arguments.
 */
#include <math.h>
#include <string.h>

#include "../../../include/vp9hip.h"

int64_t vp9hip_out_layout(const vp9hip_out_desc *d, int bpp, int ss_h, int ss_v, int64_t *pitch,
                          int64_t plane_offset[3])
{
    if (!d || d->width <= 0 || d->height <= 0 || d->pitch < 0 || d->frame_stride < 0) return VP9HIP_EINVAL;
    if ((bpp != 8 && bpp != 10 && bpp != 12) || ss_h < 0 || ss_h > 1 || ss_v < 0 || ss_v > 1) return VP9HIP_EINVAL;
    const int64_t w = d->width, h = d->height;
    const int64_t cw = (w + ss_h) >> ss_h, ch = (h + ss_v) >> ss_v;
    const int64_t bs = bpp > 8 ? 2 : 1;
    int64_t row, rows;
    switch (d->format) {
    case VP9HIP_OUT_SEMIPLANAR: row = (w > 2 * cw ? w : 2 * cw) * bs; rows = h + ch; break;
    case VP9HIP_OUT_RGB24:      row = 3 * w; rows = h; break;
    case VP9HIP_OUT_RGBP_U8:    row = w; rows = 3 * h; break;
    case VP9HIP_OUT_RGBP_F16:   row = 2 * w; rows = 3 * h; break;
    default: return VP9HIP_EINVAL;
    }
    int64_t p = d->pitch ? d->pitch : row;
    if (p < row || (p != row && (p & 15))) return VP9HIP_EINVAL;
    const int64_t bytes = p * rows;
    if (d->frame_stride && d->frame_stride < bytes) return VP9HIP_EINVAL;
    if (pitch) *pitch = p;
    if (plane_offset) {
        if (d->format == VP9HIP_OUT_SEMIPLANAR) {
            plane_offset[0] = 0; plane_offset[1] = p * h; plane_offset[2] = p * h + bs;
        } else if (d->format == VP9HIP_OUT_RGB24) {
            plane_offset[0] = 0; plane_offset[1] = 1; plane_offset[2] = 2;
        } else {
            plane_offset[0] = 0; plane_offset[1] = p * h; plane_offset[2] = 2 * p * h;
        }
    }
    return bytes;
}

/* The filters' definition (include/vp9hip.h), one output index of one axis. Plain 64-bit
 * arithmetic from the formulas, no shortcut: this is what a result can be reproduced from. */
int vp9hip_resample_weights(int filter, int n_src, int n_out, int o, int *first, int32_t *weights, int cap,
                            int64_t *sum)
{
    if (filter != VP9HIP_FILTER_BOX && filter != VP9HIP_FILTER_TRIANGLE) return VP9HIP_EINVAL;
    if (n_src < 1 || n_src > 16384 || n_out < 1 || n_out > 16384 || o < 0 || o >= n_out || cap < 0) return VP9HIP_EINVAL;
    const int64_t w = n_src, ow = n_out;
    int64_t s0, s1;
    if (filter == VP9HIP_FILTER_BOX) {
        s0 = o * w / ow;                               /* [o w, (o+1) w) meets [s ow, (s+1) ow) */
        s1 = ((o + 1) * w + ow - 1) / ow;
    } else {
        const int64_t m2 = 2 * (w > ow ? w : ow), c = (2 * (int64_t) o + 1) * w;
        const int64_t lo = c - m2 + ow;                /* (2 s + 1) ow > c - 2M */
        s0 = lo < 0 ? 0 : lo / (2 * ow);
        s1 = (c + m2 + ow - 1) / (2 * ow);             /* (2 s + 1) ow < c + 2M */
        if (s1 > w) s1 = w;
    }
    int64_t d = 0;
    for (int64_t s = s0; s < s1; s++) {
        int64_t t;
        if (filter == VP9HIP_FILTER_BOX) {
            const int64_t a = o * w > s * ow ? o * w : s * ow, b = (o + 1) * w < (s + 1) * ow ? (o + 1) * w : (s + 1) * ow;
            t = b - a;
        } else {
            const int64_t m2 = 2 * (w > ow ? w : ow), e = (2 * (int64_t) o + 1) * w - (2 * s + 1) * ow;
            t = m2 - (e < 0 ? -e : e);
        }
        if (weights && s - s0 < cap) weights[s - s0] = (int32_t) t;
        d += t;
    }
    if (first) *first = (int) s0;
    if (sum) *sum = d;
    return (int) (s1 - s0);
}

/* The bicubic definition (include/vp9hip.h), one output index of one axis, in plain 64-bit
 * arithmetic from the formulas. With sizes up to 16384, T <= 2^15: u < 2^16, every partial sum
 * of c is below 2^52, |c 2^Q| below 2^61 (tests/c/bicubic_weights_check.c sweeps the extreme
 * sizes under UBSan). */
#define BICUBIC_Q 14
static int64_t bicubic_q(int64_t u, int64_t t)
{
    const int64_t t3 = t * t * t;
    const int64_t c = u < t ? u * u * (3 * u - 5 * t) + 2 * t3 : ((5 * t - u) * u - 8 * t * t) * u + 4 * t3;
    const int64_t num = c * ((int64_t) 1 << BICUBIC_Q) + t3, den = 2 * t3;
    int64_t q = num / den;                             /* truncates: floor it */
    if (num % den < 0) q--;
    return q;
}

int vp9hip_bicubic_weights(int n_src, int n_out, int o, int *first, int32_t *weights, int cap, int64_t *sum,
                           int64_t *abs_sum)
{
    if (n_src < 1 || n_src > 16384 || n_out < 1 || n_out > 16384 || o < 0 || o >= n_out || cap < 0) return VP9HIP_EINVAL;
    const int64_t w = n_src, ow = n_out, t = 2 * (w > ow ? w : ow), k = (2 * (int64_t) o + 1) * w;
    const int64_t lo = k - 2 * t + ow;                 /* (2 s + 1) ow > k - 2T */
    int64_t s0 = lo < 0 ? 0 : lo / (2 * ow);
    int64_t s1 = (k + 2 * t + ow - 1) / (2 * ow);      /* (2 s + 1) ow < k + 2T */
    if (s1 > w) s1 = w;
    int64_t d = 0, a = 0;
    for (int64_t s = s0; s < s1; s++) {
        const int64_t e = k - (2 * s + 1) * ow, q = bicubic_q(e < 0 ? -e : e, t);
        if (weights && s - s0 < cap) weights[s - s0] = (int32_t) q;
        d += q;
        a += q < 0 ? -q : q;
    }
    if (first) *first = (int) s0;
    if (sum) *sum = d;
    if (abs_sum) *abs_sum = a;
    return (int) (s1 - s0);
}

int vp9hip_out_coefs(int colorspace, int full_range, int bpp, int out_bits, int32_t c[5], int32_t *shift)
{
    if (!c || !shift || (bpp != 8 && bpp != 10 && bpp != 12) || (out_bits != 8 && out_bits != bpp)) return VP9HIP_EINVAL;
    double kr, kb;
    switch (colorspace) {
    case 1: case 3: kr = .299;  kb = .114;  break;   /* BT.470BG / SMPTE-170M (BT.601) */
    case 2:         kr = .2126; kb = .0722; break;   /* BT.709     */
    case 4:         kr = .212;  kb = .087;  break;   /* SMPTE-240M */
    case 5:         kr = .2627; kb = .0593; break;   /* BT.2020 NCL */
    case 7:                                          /* RGB planes: no matrix */
        memset(c, 0, 5 * sizeof(c[0]));
        *shift = bpp - out_bits;
        return 0;
    default: return VP9HIP_EINVAL;
    }
    const int s = 14 + bpp - out_bits;
    const double m = (double) ((1 << out_bits) - 1), up = (double) (1 << (bpp - 8));
    const double sy = full_range ? m / (double) ((1 << bpp) - 1) : m / (219. * up);
    const double sc = full_range ? m / (double) ((1 << bpp) - 1) : m / (224. * up);
    const double kg = 1. - kr - kb, one = (double) (1 << s);
    const double x[5] = { sy, 2. * (1. - kr) * sc, 2. * kb * (1. - kb) / kg * sc, 2. * kr * (1. - kr) / kg * sc,
                          2. * (1. - kb) * sc };
    for (int i = 0; i < 5; i++) c[i] = (int32_t) floor(x[i] * one + .5);
    *shift = s;
    return 0;
}
