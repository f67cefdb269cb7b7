// Device code the four output conversion kernels share (vp9hip_convert.hip, _scale, _resample,
// _cubic): the stored pixel that include/vp9hip.h defines bit for bit (matrix, clip, the half's
// two roundings, the per-format stores) and the arithmetic the resize kernels have in common.
// Included by those four files, and by vp9hip_residual_scale.hip and vp9hip_warp_scale.hip
// (through vp9hip_resid_dev.h too) for floordiv, rounded_quot and to_half. Everything is
// __device__ __forceinline__: no kernels, no __shared__.
#ifndef VP9HIP_CONVERT_DEV_H
#define VP9HIP_CONVERT_DEV_H

#include "vp9hip_convert.h"

namespace cvtdev {

// The resize kernels' output tile, TH waves, each one row of TW columns (the launch grid is
// cvt_tile_grid's), and the source columns per pass: 64 lanes x 4 samples.
constexpr int TW = CVT_TILE_W, TH = CVT_TILE_H;
constexpr int CHUNK = 256;

__device__ __forceinline__ int clip(int v, int hi) { return min(max(v, 0), hi); }

// The half output: the float product rounded to float, then to the nearest-even half, as the
// definition says. Left to the compiler, the two become one v_fma_mixlo_f16 here, which rounds
// once and differs where the float product rounds onto a half's midpoint (12-bit samples
// show it); the empty asm keeps the float product a value of its own.
__device__ __forceinline__ _Float16 to_half(int v, float fscale)
{
    float f = (float) v * fscale;
    asm volatile("" : "+v"(f));
    return (_Float16) f;
}

// floor(t / d) for 0 <= t < 2^30, 0 < d, with rcp = 1.0 / d in double: the estimate is within
// one of the quotient (its error is below 2^-22), the remainder corrects it. A few instructions
// where the compiler's expansion of an integer division by a kernel argument takes about 25,
// and a wave needs 16 of them before its first load. Sizes are at most 2^14, so the box
// filter's t = o n_src + n_src + n_out - 1 stays below 2^29, the keys and terms of the
// triangle and the cubic below 2^30.
__device__ __forceinline__ int floordiv(int t, int d, double rcp)
{
    int q = (int) ((double) t * rcp);
    const int r = t - q * d;
    if (r < 0) q--;
    else if (r >= d) q++;
    return q;
}

// floor((A + (den >> 1)) / den), the quotient below 2^16 (16-bit samples at most), with
// rcp = 1.0 / den in double: the estimate is within 2^-30 of the quotient, the exact 64-bit
// remainder (|r| < 2 den < 2^63) corrects it. The unsigned filters (box, triangle).
__device__ __forceinline__ int rounded_quot(uint64_t acc, uint64_t den, double rcp)
{
    const uint64_t A = acc + (den >> 1);
    uint32_t q = (uint32_t) ((double) A * rcp);
    const int64_t r = (int64_t) (A - q * den);
    if (r < 0) q--;
    else if (r >= (int64_t) den) q++;
    return (int) q;
}

// v[i] += wy * sample i of the 4 at p (aligned to their 4 or 8 bytes), as one W x W -> A
// product each: u32 u32 -> u32 (box), u32 u32 -> u64 (triangle), i32 i32 -> i64 (cubic).
template <int HBD, class W, class A>
__device__ __forceinline__ void add_row(const uint8_t *p, W wy, A (&v)[4])
{
    if constexpr (HBD) {
        const uint2 s = *reinterpret_cast<const uint2 *>(p);
        v[0] += (A) wy * (W) (s.x & 0xffff); v[1] += (A) wy * (W) (s.x >> 16);
        v[2] += (A) wy * (W) (s.y & 0xffff); v[3] += (A) wy * (W) (s.y >> 16);
    } else {
        const uint32_t s = *reinterpret_cast<const uint32_t *>(p);
        v[0] += (A) wy * (W) (s & 0xff); v[1] += (A) wy * (W) (s >> 8 & 0xff);
        v[2] += (A) wy * (W) (s >> 16 & 0xff); v[3] += (A) wy * (W) (s >> 24);
    }
}

// One plane geometry of one frame: the source rectangle (x, y, w, h) of planes with `pitch`,
// resampled to dw x dh and placed at (dx, dy) of the output plane.
struct Geo { int x, y, w, h, dx, dy, dw, dh; };

// Frame z's geometries: luma, and the chroma planes: the source rectangle at their
// subsampling; the destination rectangle at the output's (semi-planar: the source's; RGB: none)
__device__ __forceinline__ void frame_geo(const CvtResampleArgs &s, int z, Geo &gy, Geo &gc)
{
    const vp9hip_rect sr = s.src_rect[z], dr = s.dst_rect[z];
    gy = { sr.x, sr.y, sr.w, sr.h, dr.x, dr.y, dr.w, dr.h };
    gc = { sr.x >> s.ss_h, sr.y >> s.ss_v, (sr.w + s.ss_h) >> s.ss_h, (sr.h + s.ss_v) >> s.ss_v,
           dr.x >> s.ds_h, dr.y >> s.ds_v, (dr.w + s.ds_h) >> s.ds_h, (dr.h + s.ds_v) >> s.ds_v };
}

// Three samples of one pixel -> R, G, B codes: the integer definition of include/vp9hip.h /
// DESIGN.md "Output conversion" (coefficients with `shift` fractional bits, round half up, clip).
__device__ __forceinline__ void cvt_rgb(const CvtArgs &a, int Y, int U, int V, int &R, int &G, int &B)
{
    if (a.rgb) {                                       // planes G, B, R
        R = min((V + a.rnd) >> a.shift, a.maxv);
        G = min((Y + a.rnd) >> a.shift, a.maxv);
        B = min((U + a.rnd) >> a.shift, a.maxv);
    } else {
        const int yy = (Y - a.yoff) * a.c[0] + a.rnd, cu = U - a.coff, cv = V - a.coff;
        R = clip((yy + a.c[1] * cv) >> a.shift, a.maxv);
        G = clip((yy - a.c[2] * cu - a.c[3] * cv) >> a.shift, a.maxv);
        B = clip((yy + a.c[4] * cu) >> a.shift, a.maxv);
    }
}

// One row of a grade's matrix over the three linear codes, then out_lut: the definition of
// include/vp9hip.h "Graded output". Each product is one 32 x 32 -> 64 multiply-add (|m| <= 2^16,
// L < 2^16: the sum passes 32 bits); P >> 4 <= 4095, so the second entry read is at most 4096.
__device__ __forceinline__ int grade_row(const int32_t *m, const uint16_t *out_lut, int LR, int LG, int LB)
{
    int64_t s = (int64_t) m[0] * LR + 8192;
    s += (int64_t) m[1] * LG;
    s += (int64_t) m[2] * LB;
    const int P = (int) min(max(s >> 14, (int64_t) 0), (int64_t) 65535);
    const int i = P >> 4, f = P & 15;
    return ((int) out_lut[i] * (16 - f) + (int) out_lut[i + 1] * f + 8) >> 4;
}

// R, G, B codes at the source's depth (each <= 2^bpp - 1: cvt_rgb clipped them) -> graded codes.
__device__ __forceinline__ void cvt_grade(const CvtGrade &g, int &R, int &G, int &B)
{
    const int LR = g.in_lut[R], LG = g.in_lut[G], LB = g.in_lut[B];
    R = grade_row(g.m, g.out_lut, LR, LG, LB);
    G = grade_row(g.m + 3, g.out_lut, LR, LG, LB);
    B = grade_row(g.m + 6, g.out_lut, LR, LG, LB);
}

// Output pixel (x, oy) of frame `dst` from the resize kernels: Y, U, V are the samples of an
// ow x oh RGB output's pixel, or, semi-planar, the luma sample (x, oy) of ow x oh and the chroma
// pair (x, oy) of cow x coh (ctile: this workgroup's tile has chroma). Stores are per element,
// lanes on consecutive pixels, only inside the output. The arguments come by value on purpose:
// the copy is free (everything here is inlined into a kernel whose arguments they are), and it
// leaves k_convert_scale's code before this call the same instruction for instruction, where a
// reference changed its register allocation from the first load on (90 -> 91 VGPRs).
// GR: the graded instantiations (RGB formats only) pass the codes through the grade g, a second
// by-value argument for the same reason; without GR it is never read and costs nothing.
template <int FMT, int HBD, int GR = 0>
__device__ __forceinline__ void cvt_store_px(const CvtArgs a, uint8_t *dst, int x, int oy, int ow, int oh, int cow, int coh,
                                             bool ctile, int Y, int U, int V, const CvtGrade g = CvtGrade())
{
    static_assert(!GR || FMT != VP9HIP_OUT_SEMIPLANAR, "a grade is defined for the RGB formats");
    constexpr int BS = HBD ? 2 : 1;
    if constexpr (FMT == VP9HIP_OUT_SEMIPLANAR) {
        if (x < ow && oy < oh) {
            uint8_t *p = dst + (int64_t) oy * a.pitch + (int64_t) x * BS;
            if constexpr (HBD) *reinterpret_cast<uint16_t *>(p) = (uint16_t) (Y << a.msb);
            else *p = (uint8_t) Y;
        }
        if (ctile && x < cow && oy < coh) {
            uint8_t *p = dst + a.plane + (int64_t) oy * a.pitch + (int64_t) x * 2 * BS;
            if constexpr (HBD) {
                reinterpret_cast<uint16_t *>(p)[0] = (uint16_t) (U << a.msb);
                reinterpret_cast<uint16_t *>(p)[1] = (uint16_t) (V << a.msb);
            } else {
                p[0] = (uint8_t) U; p[1] = (uint8_t) V;
            }
        }
    } else {
        if (x >= ow || oy >= oh) return;
        int R, G, B;
        cvt_rgb(a, Y, U, V, R, G, B);
        if constexpr (GR) cvt_grade(g, R, G, B);
        uint8_t *row = dst + (int64_t) oy * a.pitch;
        if constexpr (FMT == VP9HIP_OUT_RGB24) {
            uint8_t *p = row + (int64_t) x * 3;
            p[0] = (uint8_t) R; p[1] = (uint8_t) G; p[2] = (uint8_t) B;
        } else if constexpr (FMT == VP9HIP_OUT_RGBP_U8) {
            row[x] = (uint8_t) R; row[a.plane + x] = (uint8_t) G; row[2 * a.plane + x] = (uint8_t) B;
        } else {                                       // half: one float multiply, round to nearest even
            _Float16 *p = reinterpret_cast<_Float16 *>(row) + x;
            const int64_t pl = a.plane / 2;
            p[0] = to_half(R, a.fscale);
            p[pl] = to_half(G, a.fscale);
            p[2 * pl] = to_half(B, a.fscale);
        }
    }
}

}  // namespace cvtdev

#endif
