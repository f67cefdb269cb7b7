/*
 * Graded output, host side: the check of a grade's description and the C statement of its three
 * stages (include/vp9hip.h "Graded output"). Plain 64-bit arithmetic from the
 * formulas, no device code: this is what a graded pixel can be reproduced from.
 */
#include <stddef.h>

#include "../../../include/vp9hip.h"

/* What vp9hip_grade_create and vp9hip_grade_host accept. */
int vp9hip_grade_check(const vp9hip_grade_desc *g)
{
    if (!g || !g->in_lut || !g->m || !g->out_lut) return VP9HIP_EINVAL;
    if (g->bpp != 8 && g->bpp != 10 && g->bpp != 12) return VP9HIP_EINVAL;
    if (g->out_max != 255 && g->out_max != 65535) return VP9HIP_EINVAL;
    for (int i = 0; i < 9; i++)
        if (g->m[i] > 65536 || g->m[i] < -65536) return VP9HIP_EINVAL;
    for (int i = 0; i < VP9HIP_GRADE_OUT_LUT; i++)
        if (g->out_lut[i] > g->out_max) return VP9HIP_EINVAL;
    return 0;
}

int vp9hip_grade_host(const vp9hip_grade_desc *g, const uint16_t *rgb_codes, int64_t n_pixels, uint16_t *v)
{
    const int r = vp9hip_grade_check(g);
    if (r < 0) return r;
    if (!rgb_codes || !v || n_pixels < 0) return VP9HIP_EINVAL;
    const int top = (1 << g->bpp) - 1;
    for (int64_t i = 0; i < 3 * n_pixels; i++)
        if (rgb_codes[i] > top) return VP9HIP_EINVAL;
    for (int64_t p = 0; p < n_pixels; p++) {
        int64_t L[3];
        for (int c = 0; c < 3; c++) L[c] = g->in_lut[rgb_codes[3 * p + c]];
        for (int row = 0; row < 3; row++) {
            const int32_t *m = g->m + 3 * row;
            const int64_t s = m[0] * L[0] + m[1] * L[1] + m[2] * L[2] + 8192;
            int64_t P = s >= 0 ? s >> 14 : -((-s + 16383) >> 14);        /* floor, whatever >> does to a negative */
            P = P < 0 ? 0 : P > 65535 ? 65535 : P;
            const int64_t k = P >> 4, f = P & 15;
            v[3 * p + row] = (uint16_t) ((g->out_lut[k] * (16 - f) + g->out_lut[k + 1] * f + 8) >> 4);
        }
    }
    return 0;
}
