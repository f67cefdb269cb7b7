// Frame histograms on the host: the C statement of the definition in include/vp9hip.h ("frame
// histograms"), one sample at a time. Plain C11, no HIP: the stand-alone check
// (tests/c/hist_host_check.c) compiles this file as it is, beside host/vp9h_convert.c for
// vp9hip_out_coefs.
#include <stddef.h>
#include <stdint.h>

#include "../../../include/vp9hip.h"

static inline int32_t hist_sample(const void *plane, ptrdiff_t linesize, int hb, int x, int y)
{
    const uint8_t *row = (const uint8_t *) plane + (ptrdiff_t) y * linesize;
    return hb ? (int32_t) ((const uint16_t *) row)[x] : (int32_t) row[x];
}

static inline int32_t hist_clip(int64_t v, int32_t hi) { return v < 0 ? 0 : v > hi ? hi : (int32_t) v; }

int vp9hip_frame_histograms_host(const void *const planes[3], const ptrdiff_t linesize[3], int bpp, int ss_h, int ss_v,
                                 const vp9hip_hist_desc *d, const vp9hip_rect *rect, int32_t *out)
{
    if (!planes || !linesize || !d || !out) return VP9HIP_EINVAL;
    if (bpp != 8 && bpp != 10 && bpp != 12) return VP9HIP_EINVAL;
    if (ss_h < 0 || ss_h > 1 || ss_v < 0 || ss_v > 1) return VP9HIP_EINVAL;
    if (d->what != VP9HIP_HIST_PLANES && d->what != VP9HIP_HIST_RGBM) return VP9HIP_EINVAL;
    if (d->bins_log2 < 4 || d->bins_log2 > bpp) return VP9HIP_EINVAL;
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384) return VP9HIP_EINVAL;
    for (int p = 0; p < 3; p++)
        if (!planes[p]) return VP9HIP_EINVAL;
    vp9hip_rect r = { 0, 0, d->width, d->height };
    if (rect) r = *rect;
    if (r.w < 1 || r.h < 1 || r.x < 0 || r.y < 0 || r.x > d->width - r.w || r.y > d->height - r.h) return VP9HIP_EINVAL;
    if ((r.x & ((1 << ss_h) - 1)) || (r.y & ((1 << ss_v) - 1))) return VP9HIP_EINVAL;
    const int hb = bpp > 8, k = d->bins_log2, sh = bpp - k;
    const int32_t maxv = (1 << bpp) - 1;
    const ptrdiff_t B = (ptrdiff_t) 1 << k;
    int32_t c[5], shift;
    if (d->what == VP9HIP_HIST_RGBM && vp9hip_out_coefs(d->colorspace, d->full_range, bpp, bpp, c, &shift) < 0)
        return VP9HIP_EINVAL;
    const int C = d->what == VP9HIP_HIST_RGBM ? 4 : 3;
    for (ptrdiff_t i = 0; i < C * B; i++) out[i] = 0;

    if (d->what == VP9HIP_HIST_PLANES) {
        for (int p = 0; p < 3; p++) {
            const int sx = p ? ss_h : 0, sy = p ? ss_v : 0;
            const int px = r.x >> sx, py = r.y >> sy, pw = (r.w + sx) >> sx, ph = (r.h + sy) >> sy;
            for (int y = py; y < py + ph; y++)
                for (int x = px; x < px + pw; x++) {
                    const int32_t v = hist_sample(planes[p], linesize[p], hb, x, y);
                    out[p * B + ((v > maxv ? maxv : v) >> sh)]++;
                }
        }
        return 0;
    }
    const int32_t yoff = d->full_range ? 0 : 16 << (bpp - 8), coff = 1 << (bpp - 1);
    const int64_t rnd = shift > 0 ? (int64_t) 1 << (shift - 1) : 0;
    for (int y = r.y; y < r.y + r.h; y++)
        for (int x = r.x; x < r.x + r.w; x++) {
            const int64_t Y = hist_sample(planes[0], linesize[0], hb, x, y);
            const int64_t U = hist_sample(planes[1], linesize[1], hb, x >> ss_h, y >> ss_v);
            const int64_t V = hist_sample(planes[2], linesize[2], hb, x >> ss_h, y >> ss_v);
            int32_t R, G, Bl;
            if (d->colorspace == 7) {                       /* planes G, B, R: no matrix */
                R = hist_clip((V + rnd) >> shift, maxv);
                G = hist_clip((Y + rnd) >> shift, maxv);
                Bl = hist_clip((U + rnd) >> shift, maxv);
            } else {
                /* |yy| < 2^16 * 2^15 + 2^13 and each product below 2^31: 64 bits hold the sums; >> of a
                 * negative sum is the arithmetic shift (floor) on every compiler this builds with */
                const int64_t yy = (Y - yoff) * c[0] + rnd, cu = U - coff, cv = V - coff;
                R = hist_clip((yy + c[1] * cv) >> shift, maxv);
                G = hist_clip((yy - c[2] * cu - c[3] * cv) >> shift, maxv);
                Bl = hist_clip((yy + c[4] * cu) >> shift, maxv);
            }
            const int32_t M = R > G ? (R > Bl ? R : Bl) : (G > Bl ? G : Bl);
            out[R >> sh]++;
            out[B + (G >> sh)]++;
            out[2 * B + (Bl >> sh)]++;
            out[3 * B + (M >> sh)]++;
        }
    return 0;
}
