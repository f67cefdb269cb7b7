// Device code k_acc_warp (vp9hip_warp.hip), k_acc_warp_scale (vp9hip_warp_scale.hip) and the
// propagation kernels (vp9hip_prop.hip) share: cl, the vector clamp and the split of a
// displacement in 1/16 sample (vclamp, near16, whole16, phase16), which all three use, and one run of consecutive samples of a plane, as include/vp9hip.h "accumulated residual" defines
// them: a's samples of the run, and the run's prediction from b through the cell's vector
// (steps 4 and 5: nearest, bilinear). Everything is __device__ __forceinline__: no kernels, no
// __shared__.
//
// Bounds, for every caller: a row of `a` is read only at x0 <= x < x0 + nv, and every b
// coordinate is clamped to 0 .. PW - 1 / 0 .. PH - 1 before its load. Where no column clamp acts
// and the whole span lies inside the visible row, the run's source samples are consecutive
// bytes and come in one load a row instead of one a sample; the address is whatever the vector
// makes it, and gfx950 serves unaligned global loads. The vector load of `a` is taken only where
// the run is whole and its address aligned to its size.
#ifndef VP9HIP_WARP_DEV_H
#define VP9HIP_WARP_DEV_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

namespace warpdev {

__device__ __forceinline__ int cl(const int v, const int n)
{
    return v < 0 ? 0 : v > n - 1 ? n - 1 : v;
}

// step 3: a cell's accumulated component clamped to the int16 range
__device__ __forceinline__ int vclamp(const int d)
{
    return d < -32768 ? -32768 : d > 32767 ? 32767 : d;
}

// a displacement p in 1/16 sample: the whole samples to the nearest position (step 4), and the
// whole samples below it and the phase 0..15 (step 5); arithmetic shifts
__device__ __forceinline__ int near16(const int p) { return (p + 8) >> 4; }
__device__ __forceinline__ int whole16(const int p) { return p >> 4; }
__device__ __forceinline__ uint32_t phase16(const int p) { return (uint32_t) p & 15; }

template <typename T> __device__ __forceinline__ uint32_t ld(const uint8_t *row, const int x)
{
    return ((const T *) row)[x];
}

// NS consecutive samples from byte address p, which need not be aligned: one load of the next
// power of two of bytes (the caller has checked that all of them lie inside the visible row)
template <typename T, int NS> __device__ __forceinline__ void ld_span(const uint8_t *p, uint32_t (&v)[NS])
{
    constexpr int NB = NS * (int) sizeof(T), W = NB <= 2 ? 2 : NB <= 4 ? 4 : NB <= 8 ? 8 : 16;
    uint32_t w[4] = { 0, 0, 0, 0 };
    __builtin_memcpy(w, p, W);
#pragma unroll
    for (int i = 0; i < NS; i++) {
        constexpr int SPD = 4 / (int) sizeof(T);
        v[i] = (w[i / SPD] >> (8 * sizeof(T) * (i % SPD))) & (sizeof(T) == 1 ? 0xffu : 0xffffu);
    }
}
// the bytes ld_span<T, NS> reads
template <typename T, int NS> __device__ __forceinline__ constexpr int span_bytes()
{
    return NS * (int) sizeof(T) <= 2 ? 2 : NS * (int) sizeof(T) <= 4 ? 4 : NS * (int) sizeof(T) <= 8 ? 8 : 16;
}

// a's samples x0 .. x0 + nv - 1 of row ra into av (the caller zeroed it): 1 <= nv <= RUN
template <typename T, int RUN>
__device__ __forceinline__ void ld_run(const uint8_t *const ra, const int x0, const int nv, uint32_t (&av)[RUN])
{
    const uint8_t *const at = ra + (size_t) x0 * sizeof(T);
    if (nv == RUN && !((uintptr_t) at & (RUN * sizeof(T) - 1))) {
        uint32_t wv[2] = { 0, 0 };
        if (RUN * sizeof(T) == 8) { const uint2 v = *(const uint2 *) at; wv[0] = v.x; wv[1] = v.y; }
        else if (RUN * sizeof(T) == 4) wv[0] = *(const uint32_t *) at;
        else wv[0] = *(const uint16_t *) at;
#pragma unroll
        for (int i = 0; i < RUN; i++) {
            constexpr int SPD = 4 / (int) sizeof(T);
            av[i] = (wv[i / SPD] >> (8 * sizeof(T) * (i % SPD))) & (sizeof(T) == 1 ? 0xffu : 0xffffu);
        }
    } else {
#pragma unroll
        for (int i = 0; i < RUN; i++)
            if (i < nv) av[i] = ld<T>(ra, x0 + i);
    }
}

// The prediction of the run of RUN samples from (x0, y) of a plane: pb the plane in b, PW x PH
// its visible size, (px, py) the cell's vector in 1/16 sample of the plane.
template <typename T, int RUN, int MODE>
__device__ __forceinline__ void warp_pred(const uint8_t *const pb, const size_t pitch, const int PW, const int PH,
                                          const int x0, const int y, const int px, const int py, uint32_t (&pv)[RUN])
{
    if (MODE == VP9HIP_WARP_NEAREST) {
        const uint8_t *const rb = pb + (size_t) cl(y + near16(py), PH) * pitch;
        const int xs = x0 + near16(px);
        if (xs >= 0 && xs * (int) sizeof(T) + span_bytes<T, RUN>() <= PW * (int) sizeof(T)) {
            ld_span<T, RUN>(rb + (size_t) xs * sizeof(T), pv);           // no column clamps: the run is contiguous
        } else {
#pragma unroll
            for (int i = 0; i < RUN; i++) pv[i] = ld<T>(rb, cl(xs + i, PW));
        }
    } else {
        const int ys = y + whole16(py), xs = x0 + whole16(px);
        const uint32_t fx = phase16(px), fy = phase16(py);
        const uint8_t *const r0 = pb + (size_t) cl(ys, PH) * pitch, *const r1 = pb + (size_t) cl(ys + 1, PH) * pitch;
        // the run's RUN + 1 columns of both rows, blended down the column first
        uint32_t t[RUN + 1], u[RUN + 1];
        if (xs >= 0 && xs * (int) sizeof(T) + span_bytes<T, RUN + 1>() <= PW * (int) sizeof(T)) {
            ld_span<T, RUN + 1>(r0 + (size_t) xs * sizeof(T), t);        // no column clamps: one span a row
            ld_span<T, RUN + 1>(r1 + (size_t) xs * sizeof(T), u);
        } else {
#pragma unroll
            for (int i = 0; i <= RUN; i++) {
                const int xx = cl(xs + i, PW);
                t[i] = ld<T>(r0, xx);
                u[i] = ld<T>(r1, xx);
            }
        }
        // (16 - fx)(16 - fy) s00 + fx (16 - fy) s01 + (16 - fx) fy s10 + fx fy s11, regrouped by
        // column: exact in integers, at most 256 * 65535 + 128 < 2^32
#pragma unroll
        for (int i = 0; i <= RUN; i++) t[i] = (16 - fy) * t[i] + fy * u[i];
#pragma unroll
        for (int i = 0; i < RUN; i++) pv[i] = ((16 - fx) * t[i] + fx * t[i + 1] + 128) >> 8;
    }
}

}  // namespace warpdev

#endif
