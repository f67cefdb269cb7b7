/*
 * Motion tensors at model size, host side: the layout of the output and the C statement of the
 * definition (include/vp9hip.h "motion tensors at model size"). No device code.
 * The statement takes one output sample at a time, in 64-bit integers, over the cells of its
 * footprint with the aggregated weight W: it is what a result can be reproduced from, and
 * shares nothing with the kernel (vp9hip_motion_scale.hip).
 */
#include <string.h>

#include "../../../include/vp9hip.h"

int64_t vp9hip_mvt_layout(const vp9hip_mvt_desc *d, int64_t *pitch)
{
    if (!d || d->format < VP9HIP_MVT_I16 || d->format > VP9HIP_MVT_F16) return VP9HIP_EINVAL;
    if (d->source < VP9HIP_MVT_CODED || d->source > VP9HIP_MVT_ACC || d->planes < 2 || d->planes > 3) return VP9HIP_EINVAL;
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384) return VP9HIP_EINVAL;
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

/* floor(a / b), b > 0 (C's division truncates toward zero) */
static int64_t floor_div(int64_t a, int64_t b)
{
    int64_t q = a / b;
    if (a % b < 0) q--;
    return q;
}

static int64_t i64min(int64_t a, int64_t b) { return a < b ? a : b; }
static int64_t i64max(int64_t a, int64_t b) { return a > b ? a : b; }
static int64_t clamp16(int64_t v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

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
    u += 0xfff + (u >> 13 & 1);                                      /* 65520 and above carries into 0x7c00 */
    return (uint16_t) (sign | ((u - ((uint32_t) 112 << 23)) >> 13));
}

/* (vx, vy, 256 has) of cell (r, c) */
static void cell_value(const int16_t *mv, const uint8_t *info, const vp9hip_acc_cell *acc, ptrdiff_t pc, int source,
                       int64_t r, int64_t c, int64_t v[3])
{
    const ptrdiff_t i = (ptrdiff_t) r * pc + (ptrdiff_t) c;
    int has;
    if (source == VP9HIP_MVT_CODED) {
        has = info[4 * i] != 255;
        v[0] = has ? mv[4 * i] : 0;
        v[1] = has ? mv[4 * i + 1] : 0;
    } else {
        has = acc[i].hops > 0;
        v[0] = has ? clamp16(acc[i].dx) : 0;
        v[1] = has ? clamp16(acc[i].dy) : 0;
    }
    v[2] = has ? 256 : 0;
}

int vp9hip_motion_scaled_host(const int16_t *mv, const uint8_t *info, const vp9hip_acc_cell *acc,
                              ptrdiff_t pitch_cells, const vp9hip_mvt_desc *d, void *dst)
{
    if (!d || !dst || ((uintptr_t) dst & 1)) return VP9HIP_EINVAL;
    int64_t op = 0;
    if (vp9hip_mvt_layout(d, &op) < 0) return VP9HIP_EINVAL;
    if (d->source == VP9HIP_MVT_CODED ? !mv || !info : !acc) return VP9HIP_EINVAL;
    const int64_t w = d->width, h = d->height, OW = d->out_width, OH = d->out_height;
    if (pitch_cells < (w + 3) >> 2) return VP9HIP_EINVAL;
    const float kx = (float) ((double) OW / (8.0 * (double) w)), ky = (float) ((double) OH / (8.0 * (double) h));
    const float scale[3] = { kx, ky, 1.0f / 256 };
    for (int64_t oy = 0; oy < OH; oy++)
        for (int64_t ox = 0; ox < OW; ox++) {
            const int64_t c0 = ox * w / (4 * OW), c1 = ((ox + 1) * w + 4 * OW - 1) / (4 * OW);
            const int64_t r0 = oy * h / (4 * OH), r1 = ((oy + 1) * h + 4 * OH - 1) / (4 * OH);
            int64_t A[3] = { 0, 0, 0 };
            for (int64_t r = r0; r < r1; r++) {
                const int64_t wy = i64max(0, i64min((oy + 1) * h, (4 * r + 4) * OH) - i64max(oy * h, 4 * r * OH));
                int64_t row[3] = { 0, 0, 0 };
                for (int64_t c = c0; c < c1; c++) {
                    const int64_t wx = i64max(0, i64min((ox + 1) * w, (4 * c + 4) * OW) - i64max(ox * w, 4 * c * OW));
                    int64_t v[3];
                    cell_value(mv, info, acc, pitch_cells, d->source, r, c, v);
                    for (int p = 0; p < 3; p++) row[p] += wx * v[p];
                }
                for (int p = 0; p < 3; p++) A[p] += wy * row[p];
            }
            for (int p = 0; p < d->planes; p++) {
                const int64_t o = floor_div(A[p] + (w * h >> 1), w * h);
                uint8_t *q = (uint8_t *) dst + (p * OH + oy) * op + 2 * ox;
                uint16_t bits;
                if (d->format == VP9HIP_MVT_F16) {
                    volatile float f = (float) o * scale[p];         /* the float32 product, rounded once, a value of its own */
                    bits = half_bits(f);
                } else {
                    bits = (uint16_t) (int16_t) o;
                }
                memcpy(q, &bits, 2);
            }
        }
    return 0;
}
