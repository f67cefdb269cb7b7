// Device code k_residual_scale (vp9hip_residual_scale.hip) and k_acc_warp_scale
// (vp9hip_warp_scale.hip) share: one output pixel of include/vp9hip.h "residual tensors at model
// size" from its three resampled values: the matrix without offsets, the clip to [-m, m], the
// half's two roundings and the planar stores. __device__ __forceinline__ only.
#ifndef VP9HIP_RESID_DEV_H
#define VP9HIP_RESID_DEV_H

#include "vp9hip_convert_dev.h"

namespace residdev {

__device__ __forceinline__ int clip_pm(int v, int m) { return min(max(v, -m), m); }

// Pixel (ox, oy) of the frame at dst from y, u, v = o0, o1, o2. FMT: VP9HIP_RESID_*: bit 1 the
// RGB matrix, bit 0 the half output. A: the launch's arguments, of which c, rnd, shift, maxv, rgb,
// fscale, pitch and plane are read. The caller has checked ox < ow, oy < oh. The arguments come
// by value on purpose, as cvt_store_px's do: by reference k_residual_scale's register
// allocation changed (93 -> 71 / 95 / 95 / 95 VGPRs by format), by value it is what it was.
template <int FMT, class A>
__device__ __forceinline__ void resid_store_px(const A a, uint8_t *dst, int ox, int oy, int o0, int o1, int o2)
{
    if constexpr ((FMT & 2) != 0) {
        const int y = o0, u = o1, v = o2;
        if (a.rgb) {                                   // planes G, B, R
            o0 = clip_pm(v, a.maxv); o1 = clip_pm(y, a.maxv); o2 = clip_pm(u, a.maxv);
        } else {                                       // no offsets: the pixel's and its prediction's cancel
            const int yy = a.c[0] * y + a.rnd;
            o0 = clip_pm((yy + a.c[1] * v) >> a.shift, a.maxv);
            o1 = clip_pm((yy - a.c[2] * u - a.c[3] * v) >> a.shift, a.maxv);
            o2 = clip_pm((yy + a.c[4] * u) >> a.shift, a.maxv);
        }
    }
    uint8_t *row = dst + (int64_t) oy * a.pitch;
    const int64_t pl = a.plane / 2;
    if constexpr ((FMT & 1) != 0) {                    // half: one float multiply, round to nearest even
        _Float16 *p = reinterpret_cast<_Float16 *>(row) + ox;
        p[0] = cvtdev::to_half(o0, a.fscale); p[pl] = cvtdev::to_half(o1, a.fscale); p[2 * pl] = cvtdev::to_half(o2, a.fscale);
    } else {
        int16_t *p = reinterpret_cast<int16_t *>(row) + ox;
        p[0] = (int16_t) o0; p[pl] = (int16_t) o1; p[2 * pl] = (int16_t) o2;
    }
}

}  // namespace residdev

#endif
