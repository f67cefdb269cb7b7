// vp9hip_acc_propagate_host: one pair of the accumulated propagation on the host, the C statement
// of the definition in include/vp9hip.h ("accumulated propagation"), one sample at a time. The
// kernels (vp9hip_prop.hip) compute the same bits; this is what the tests compare them with and
// what the sanitizer builds run (tests/c/acc_propagate_host_check.c, built without -fwrapv:
// nothing here may overflow a signed integer or shift a negative value). The binary32 operations
// of the bilinear step are one statement each and the file is compiled with -ffp-contract=off;
// binary16 is converted in integers, so nothing depends on the compiler's half support.
// vp9hip_prop_layout, the descriptor's check and the item size, lives here too.
#include <string.h>

#include "../../../include/vp9hip.h"

int64_t vp9hip_prop_layout(const vp9hip_prop_desc *d, int64_t *valid_bytes)
{
    if (!d) return VP9HIP_EINVAL;
    if (d->width < 1 || d->width > 16384 || d->height < 1 || d->height > 16384) return VP9HIP_EINVAL;
    if (d->fw < 1 || d->fw > 16384 || d->fh < 1 || d->fh > 16384 || d->channels < 1 || d->channels > 4096) return VP9HIP_EINVAL;
    if (d->elem_size != 1 && d->elem_size != 2 && d->elem_size != 4 && d->elem_size != 8) return VP9HIP_EINVAL;
    if (d->layout != VP9HIP_PROP_NCHW && d->layout != VP9HIP_PROP_NHWC) return VP9HIP_EINVAL;
    if (d->mode != VP9HIP_WARP_NEAREST && d->mode != VP9HIP_WARP_BILINEAR) return VP9HIP_EINVAL;
    if (d->mode == VP9HIP_WARP_BILINEAR && d->elem_size != 2) return VP9HIP_EINVAL;
    if ((d->flags & ~VP9HIP_PROP_KEEP) || d->reserved) return VP9HIP_EINVAL;
    const int64_t plane = (int64_t) d->fw * d->fh;
    if (valid_bytes) *valid_bytes = plane;
    return plane * d->channels * d->elem_size;
}

static int64_t cl(int64_t v, int64_t n)
{
    return v < 0 ? 0 : v > n - 1 ? n - 1 : v;
}

// floor(a / b), b > 0, without dividing or shifting a negative value
static int64_t floordiv(int64_t a, int64_t b)
{
    return a >= 0 ? a / b : -((b - 1 - a) / b);
}

// binary16 -> binary32, exact, in integers
static float half_to_float(uint16_t hv)
{
    const uint32_t sign = (uint32_t) (hv & 0x8000u) << 16, e = (hv >> 10) & 31u, m = hv & 0x3ffu;
    uint32_t u;
    if (e == 31) {
        u = sign | 0x7f800000u | m << 13;
    } else if (e) {
        u = sign | (e + 112) << 23 | m << 13;
    } else if (m) {                              // a subnormal half is m 2^-24: normalise it
        uint32_t mm = m, ee = 113;
        while (!(mm & 0x400u)) { mm <<= 1; ee--; }
        u = sign | ee << 23 | (mm & 0x3ffu) << 13;
    } else {
        u = sign;
    }
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// binary32 -> the nearest-even binary16, subnormal halves included, in integers
static uint16_t float_to_half(float f)
{
    uint32_t u;
    memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t) (sign | 0x7c00u | (a > 0x7f800000u ? 0x200u : 0));
    if (a >= 0x477ff000u) return (uint16_t) (sign | 0x7c00u);            // >= 65520 rounds to infinity
    if (a >= 0x38800000u) {                                              // a normal half
        const uint32_t r = a - 0x38000000u, h = r >> 13, rem = r & 0x1fffu;
        return (uint16_t) (sign | (h + (rem > 0x1000u || (rem == 0x1000u && (h & 1)))));
    }
    if (a < 0x33000000u) return (uint16_t) sign;                         // below 2^-25: zero (2^-25 itself ties to even, 0)
    const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u, s = 126 - e;   // the value is m 2^(e - 150): units of 2^-24
    const uint32_t h = m >> s, rem = m & ((1u << s) - 1), half = 1u << (s - 1);
    return (uint16_t) (sign | (h + (rem > half || (rem == half && (h & 1)))));
}

int vp9hip_acc_propagate_host(const vp9hip_acc_cell *acc, uint32_t root_serial, const vp9hip_prop_desc *d,
                              const void *src, void *dst, uint8_t *valid)
{
    if (!acc || !d || !src || !dst || vp9hip_prop_layout(d, NULL) < 0) return VP9HIP_EINVAL;
    const int64_t w = d->width, h = d->height, FW = d->fw, FH = d->fh, C = d->channels, E = d->elem_size;
    const int64_t gw = 2 * ((w + 7) >> 3);
    const int nhwc = d->layout == VP9HIP_PROP_NHWC, keep = d->flags & VP9HIP_PROP_KEEP;
    const uint8_t *const s8 = (const uint8_t *) src;
    uint8_t *const d8 = (uint8_t *) dst;
    uint8_t fill[8];
    for (int i = 0; i < 8; i++) fill[i] = (uint8_t) (d->fill >> (8 * i));
    for (int64_t fy = 0; fy < FH; fy++)
        for (int64_t fx = 0; fx < FW; fx++) {
            const int64_t X = ((2 * fx + 1) * w) / (2 * FW), Y = ((2 * fy + 1) * h) / (2 * FH);
            const vp9hip_acc_cell q = acc[(Y / 4) * gw + X / 4];
            const int applies = q.hops > 0 && root_serial != 0 && q.root == root_serial;
            if (valid) valid[fy * FW + fx] = (uint8_t) applies;
            const int64_t vx = q.dx < -32768 ? -32768 : q.dx > 32767 ? 32767 : q.dx;
            const int64_t vy = q.dy < -32768 ? -32768 : q.dy > 32767 ? 32767 : q.dy;
            const int64_t px = floordiv(4 * vx * FW + w, 2 * w), py = floordiv(4 * vy * FH + h, 2 * h);
            const int64_t xs = cl(fx + floordiv(px + 8, 16), FW), ys = cl(fy + floordiv(py + 8, 16), FH);
            const int64_t x0 = fx + floordiv(px, 16), y0 = fy + floordiv(py, 16);
            const float frx = (float) (px - 16 * floordiv(px, 16)), fry = (float) (py - 16 * floordiv(py, 16));
            const float grx = 16.0f - frx, gry = 16.0f - fry;
            for (int64_t ch = 0; ch < C; ch++) {
#define AT(yy, xx) ((nhwc ? ((yy) * FW + (xx)) * C + ch : (ch * FH + (yy)) * FW + (xx)) * E)
                uint8_t *const o = d8 + AT(fy, fx);
                if (!applies) {
                    if (!keep) memcpy(o, fill, (size_t) E);
                } else if (d->mode == VP9HIP_WARP_NEAREST) {
                    memcpy(o, s8 + AT(ys, xs), (size_t) E);
                } else {
                    uint16_t hv[4];
                    memcpy(&hv[0], s8 + AT(cl(y0, FH), cl(x0, FW)), 2);
                    memcpy(&hv[1], s8 + AT(cl(y0, FH), cl(x0 + 1, FW)), 2);
                    memcpy(&hv[2], s8 + AT(cl(y0 + 1, FH), cl(x0, FW)), 2);
                    memcpy(&hv[3], s8 + AT(cl(y0 + 1, FH), cl(x0 + 1, FW)), 2);
                    const float s00 = half_to_float(hv[0]), s01 = half_to_float(hv[1]);
                    const float s10 = half_to_float(hv[2]), s11 = half_to_float(hv[3]);
                    const float t0 = grx * s00;
                    const float t1 = frx * s01;
                    const float top = t0 + t1;
                    const float b0 = grx * s10;
                    const float b1 = frx * s11;
                    const float bot = b0 + b1;
                    const float u0 = gry * top;
                    const float u1 = fry * bot;
                    const float sum = u0 + u1;
                    const float v = sum * 0.00390625f;
                    const uint16_t r = float_to_half(v);
                    memcpy(o, &r, 2);
                }
#undef AT
            }
        }
    return 0;
}
