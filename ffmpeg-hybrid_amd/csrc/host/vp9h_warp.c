// vp9hip_acc_warp_host: one pair of the accumulated residual on the host, the C statement of the
// definition in include/vp9hip.h ("accumulated residual"), one sample at a time in 64-bit
// integers. k_acc_warp (vp9hip_warp.hip) computes the same integers a run of samples a lane;
// this is what the tests compare it with and what the sanitizer builds run
// (tests/c/acc_warp_host_check.c, built without -fwrapv: nothing here may overflow a signed
// integer or shift a negative value). vp9hip_warp_layout, the output's layout, lives here too.
#include <string.h>

#include "../../../include/vp9hip.h"

int64_t vp9hip_warp_layout(int width, int height, int ss_h, int ss_v, int64_t off[3])
{
    if (width < 1 || width > 16384 || height < 1 || height > 16384 || (ss_h | ss_v) & ~1) return VP9HIP_EINVAL;
    const int64_t y = 2 * (int64_t) width * height;
    const int64_t c = 2 * (int64_t) ((width + ss_h) >> ss_h) * ((height + ss_v) >> ss_v);
    if (off) { off[0] = 0; off[1] = y; off[2] = y + c; }
    return y + 2 * c;
}

static int64_t cl(int64_t v, int64_t n)
{
    return v < 0 ? 0 : v > n - 1 ? n - 1 : v;
}

// floor(v / 16) and v mod 16 in 0..15 without shifting a negative value
static int64_t floor16(int64_t v)
{
    return v >= 0 ? v / 16 : -((15 - v) / 16);
}

static int64_t sample(const void *plane, ptrdiff_t linesize, int hbd, int64_t x, int64_t y)
{
    const uint8_t *row = (const uint8_t *) plane + y * linesize;
    return hbd ? ((const uint16_t *) row)[x] : row[x];
}

int vp9hip_acc_warp_host(const void *const a[3], const ptrdiff_t linesize_a[3],
                         const void *const b[3], const ptrdiff_t linesize_b[3],
                         const vp9hip_acc_cell *acc, uint32_t serial_b, int width, int height, int bpp,
                         int ss_h, int ss_v, int mode, int output, void *dst, uint8_t *mask)
{
    int64_t off[3];
    if (!a || !b || !linesize_a || !linesize_b || !acc || !dst) return VP9HIP_EINVAL;
    if (vp9hip_warp_layout(width, height, ss_h, ss_v, off) < 0) return VP9HIP_EINVAL;
    if (bpp != 8 && bpp != 10 && bpp != 12) return VP9HIP_EINVAL;
    if (mode != VP9HIP_WARP_NEAREST && mode != VP9HIP_WARP_BILINEAR) return VP9HIP_EINVAL;
    if (output != VP9HIP_WARP_RESIDUAL && output != VP9HIP_WARP_PICTURE) return VP9HIP_EINVAL;
    for (int p = 0; p < 3; p++)
        if (!a[p] || !b[p]) return VP9HIP_EINVAL;
    const int hbd = bpp > 8;
    const int64_t gw = 2 * ((width + 7) >> 3), gh = 2 * ((height + 7) >> 3);
    if (mask)
        for (int64_t i = 0; i < gw * gh; i++)
            mask[i] = acc[i].hops > 0 && acc[i].root == serial_b;
    for (int p = 0; p < 3; p++) {
        const int sh = p ? ss_h : 0, sv = p ? ss_v : 0;
        const int64_t pw = (width + sh) >> sh, ph = (height + sv) >> sv;
        uint8_t *const out = (uint8_t *) dst + off[p];
        for (int64_t y = 0; y < ph; y++)
            for (int64_t x = 0; x < pw; x++) {
                const vp9hip_acc_cell q = acc[(y * (1 << sv) / 4) * gw + x * (1 << sh) / 4];
                const int applies = q.hops > 0 && q.root == serial_b;
                const int64_t av = sample(a[p], linesize_a[p], hbd, x, y);
                int64_t pred = 0;
                if (applies) {
                    const int64_t vx = q.dx < -32768 ? -32768 : q.dx > 32767 ? 32767 : q.dx;
                    const int64_t vy = q.dy < -32768 ? -32768 : q.dy > 32767 ? 32767 : q.dy;
                    const int64_t px = vx * (2 >> sh), py = vy * (2 >> sv);
                    if (mode == VP9HIP_WARP_NEAREST) {
                        pred = sample(b[p], linesize_b[p], hbd, cl(x + floor16(px + 8), pw), cl(y + floor16(py + 8), ph));
                    } else {
                        const int64_t x0 = x + floor16(px), y0 = y + floor16(py);
                        const int64_t fx = px - 16 * floor16(px), fy = py - 16 * floor16(py);
                        const int64_t s00 = sample(b[p], linesize_b[p], hbd, cl(x0, pw), cl(y0, ph));
                        const int64_t s01 = sample(b[p], linesize_b[p], hbd, cl(x0 + 1, pw), cl(y0, ph));
                        const int64_t s10 = sample(b[p], linesize_b[p], hbd, cl(x0, pw), cl(y0 + 1, ph));
                        const int64_t s11 = sample(b[p], linesize_b[p], hbd, cl(x0 + 1, pw), cl(y0 + 1, ph));
                        pred = ((16 - fx) * (16 - fy) * s00 + fx * (16 - fy) * s01 + (16 - fx) * fy * s10 +
                                fx * fy * s11 + 128) / 256;
                    }
                }
                uint8_t *const o = out + 2 * (y * pw + x);
                if (output == VP9HIP_WARP_RESIDUAL) {
                    int64_t d = applies ? av - pred : 0;
                    d = d < -32768 ? -32768 : d > 32767 ? 32767 : d;
                    const int16_t v = (int16_t) d;
                    memcpy(o, &v, 2);
                } else {
                    const uint16_t v = (uint16_t) (applies ? pred : av);
                    memcpy(o, &v, 2);
                }
            }
    }
    return 0;
}
