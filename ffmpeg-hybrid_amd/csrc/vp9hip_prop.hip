// Accumulated propagation for gfx950: a caller's tensor of the root frame gathered through a
// frame's accumulated field, the bits of include/vp9hip.h ("accumulated propagation"), for n
// pairs in one launch. Two addressing shapes, because one cannot coalesce both layouts.
//
// k_prop_nchw: lanes run along fx. blockIdx.z is the pair, blockIdx.y a group of PROP_TH feature
// rows, blockIdx.x a tile of PROP_TW * NS columns times a chunk of PROP_CCHUNK channels (the
// chunks are a grid dimension, so a C = 1 label map and a C = 256 feature map both fill the
// machine). A lane owns NS = 4 / 2 / 1 consecutive samples at E = 1 / 2 / >= 4: their cells and
// source coordinates are computed once and reused over the chunk's channels. A wave's store is
// 256 contiguous bytes a channel at E <= 4 (512 at E = 8), one 4-byte (E-byte) store a lane; the
// gather is contiguous wherever neighbouring samples share a vector. A lane's samples go out as
// one store only where all NS lie inside the row, the address is 4-byte aligned and (keep) all
// of them apply; else element by element, so odd FW and E-aligned-only pointers take the same
// kernel.
//
// k_prop_nhwc: a sample's C * E bytes are contiguous, and lanes run along them in units of V
// bytes, V the widest power of two <= 16 that divides C * E and both pointers (so V >= E). A
// sample takes L lanes, L the power of two >= its units (at most the workgroup); a workgroup
// carries PROP_WG / L samples, several a wave when C * E is small; blockIdx.y * gridDim.x +
// blockIdx.x numbers a pair's workgroups. Every lane of a sample computes the sample's cell and
// source coordinate itself (the field read is one broadcast line). C = 1 is the same addresses
// in both layouts and takes k_prop_nchw.
//
// The pair's record (field, serial, source item) sits in the kernel arguments and is indexed by
// blockIdx.z, sizes and strides are plain arguments: all wave-uniform, read with scalar loads.
// No LDS, no atomics: every element has one writer (the valid map: the lane of channel chunk 0 /
// of unit 0).
//
// Bounds: a lane outside the grid returns before any access; the cell index is clamped to the
// field's grid all the same; every source coordinate is clamped to 0 .. FW - 1 / 0 .. FH - 1
// before its load; vector accesses are taken only where address and length allow.
//
// Bilinear (binary16 elements): four loads an element and the binary32 operations of step 5, one
// rounding each. The products of top and bot are exact, so how the compiler groups them cannot
// change a bit; (16 - fry) top and fry bot are not, and hipcc would fuse one of them into the
// add (and the add into a mixed-precision conversion, as vp9hip_convert_dev.h to_half records):
// contraction is off for this file's arithmetic and each of the three values is pinned with an
// empty asm. The final conversion is the hardware's v_cvt_f16_f32: round to nearest even with
// subnormal halves, HIP's default mode for f16 (the GPU tests hold it to the host statement on
// subnormal results).
#include "vp9hip_prop.h"
#include "vp9hip_warp_dev.h"

namespace {

using namespace warpdev;                // cl, vclamp, near16, whole16, phase16: shared with k_acc_warp

// floor(t / d) for d > 0 from rcp = 1 / d in double: exact after one correction, |t| < 2^40
__device__ __forceinline__ int64_t floordiv(const int64_t t, const int d, const double rcp)
{
    int64_t q = (int64_t) ((double) t * rcp);
    const int64_t r = t - q * d;
    if (r < 0) q--;
    else if (r >= d) q++;
    return q;
}

// What steps 1 - 3 give for a sample (fx, fy): whether its cell applies, and (px, py), the
// displacement in 1/16 feature sample.
struct Disp {
    bool app;
    int px, py;
};

__device__ __forceinline__ Disp prop_disp(const PropArgs &g, const uint32_t z, const int fx, const int fy)
{
    const int X = (int) floordiv((int64_t) (2 * fx + 1) * g.w, 2 * g.fw, g.rfw);
    const int Y = (int) floordiv((int64_t) (2 * fy + 1) * g.h, 2 * g.fh, g.rfh);
    const uint4 q = g.acc[z][(size_t) cl(Y >> 2, g.gh) * (size_t) g.acc_pitch + (size_t) cl(X >> 2, g.gw)];
    const uint32_t S = g.serial[z];
    Disp d;
    d.app = (q.w & 0xffffu) != 0 && S != 0 && q.z == S;
    d.px = (int) floordiv((int64_t) 4 * vclamp((int) q.x) * g.fw + g.w, 2 * g.w, g.rw);
    d.py = (int) floordiv((int64_t) 4 * vclamp((int) q.y) * g.fh + g.h, 2 * g.h, g.rh);
    return d;
}

// step 5 on four halves: every operation one binary32 operation
#pragma clang fp contract(off)
__device__ __forceinline__ uint16_t bilin(const uint16_t h00, const uint16_t h01, const uint16_t h10, const uint16_t h11,
                                          const float frx, const float fry)
{
#pragma clang fp contract(off)
    const float s00 = (float) __builtin_bit_cast(_Float16, h00), s01 = (float) __builtin_bit_cast(_Float16, h01);
    const float s10 = (float) __builtin_bit_cast(_Float16, h10), s11 = (float) __builtin_bit_cast(_Float16, h11);
    const float grx = 16.0f - frx, gry = 16.0f - fry;
    float top = grx * s00 + frx * s01;              // exact products: one rounding however it is grouped
    float bot = grx * s10 + frx * s11;
    asm volatile("" : "+v"(top), "+v"(bot));
    float u0 = gry * top, u1 = fry * bot;
    asm volatile("" : "+v"(u0), "+v"(u1));
    float v = u0 + u1;
    asm volatile("" : "+v"(v));
    v *= 0.00390625f;
    asm volatile("" : "+v"(v));
    return __builtin_bit_cast(uint16_t, (_Float16) v);
}

template <int E> struct Elem;
template <> struct Elem<1> { typedef uint8_t T; };
template <> struct Elem<2> { typedef uint16_t T; };
template <> struct Elem<4> { typedef uint32_t T; };
template <> struct Elem<8> { typedef uint64_t T; };

template <int E, int MODE>
__global__ __launch_bounds__(PROP_TW * PROP_TH) void k_prop_nchw(const PropArgs g, const int xtiles)
{
    typedef typename Elem<E>::T T;
    constexpr int NS = E == 1 ? 4 : E == 2 ? 2 : 1;
    const uint32_t z = blockIdx.z;
    const int xt = (int) (blockIdx.x % (uint32_t) xtiles), chunk = (int) (blockIdx.x / (uint32_t) xtiles);
    const int fx0 = (xt * PROP_TW + (int) threadIdx.x) * NS, fy = (int) (blockIdx.y * PROP_TH + threadIdx.y);
    if (fx0 >= g.fw || fy >= g.fh) return;
    const int nv = g.fw - fx0 < NS ? g.fw - fx0 : NS;                 // samples of this lane inside the row, >= 1
    const int c0 = chunk * PROP_CCHUNK, c1 = c0 + PROP_CCHUNK < g.c ? c0 + PROP_CCHUNK : g.c;

    bool app[NS];
    int i00[NS], i01[NS], i10[NS], i11[NS];                          // element indices inside a channel plane, < 2^28
    float frx[NS], fry[NS];
    bool all = true;
#pragma unroll
    for (int i = 0; i < NS; i++) {
        const Disp d = prop_disp(g, z, cl(fx0 + i, g.fw), fy);       // a sample past the row repeats the last: never stored
        app[i] = d.app;
        all = all && d.app;
        if (MODE == VP9HIP_WARP_NEAREST) {
            i00[i] = cl(fy + near16(d.py), g.fh) * g.fw + cl(fx0 + i + near16(d.px), g.fw);
        } else {
            const int x0 = fx0 + i + whole16(d.px), y0 = fy + whole16(d.py);
            const int xa = cl(x0, g.fw), xb = cl(x0 + 1, g.fw), ya = cl(y0, g.fh) * g.fw, yb = cl(y0 + 1, g.fh) * g.fw;
            i00[i] = ya + xa; i01[i] = ya + xb; i10[i] = yb + xa; i11[i] = yb + xb;
            frx[i] = (float) phase16(d.px); fry[i] = (float) phase16(d.py);
        }
    }
    const size_t plane = (size_t) g.fw * (size_t) g.fh, at = (size_t) fy * (size_t) g.fw + (size_t) fx0;
    if (g.valid && chunk == 0) {
        uint8_t *const vp = g.valid + (size_t) z * plane + at;
#pragma unroll
        for (int i = 0; i < NS; i++)
            if (i < nv) vp[i] = app[i] ? 1 : 0;
    }
    const T *const sp = (const T *) g.src[z];
    T *const dp = (T *) (g.dst + (size_t) z * (size_t) g.item) + at;
    const T fill = (T) g.fill;
    const bool whole = nv == NS && (!g.keep || all);                  // one store a channel, where its address allows
    for (int ch = c0; ch < c1; ch++) {
        const T *const s = sp + (size_t) ch * plane;
        T *const o = dp + (size_t) ch * plane;
        T v[NS];
#pragma unroll
        for (int i = 0; i < NS; i++) {
            if constexpr (MODE == VP9HIP_WARP_NEAREST) v[i] = app[i] ? s[i00[i]] : fill;
            else v[i] = app[i] ? (T) bilin(s[i00[i]], s[i01[i]], s[i10[i]], s[i11[i]], frx[i], fry[i]) : fill;
        }
        bool done = false;
        if constexpr (NS > 1) {
            if (whole && !((uintptr_t) o & 3)) {
                uint32_t pk = 0;
#pragma unroll
                for (int i = 0; i < NS; i++) pk |= (uint32_t) v[i] << (8 * E * i);
                *(uint32_t *) o = pk;
                done = true;
            }
        }
        if (!done) {
#pragma unroll
            for (int i = 0; i < NS; i++)
                if (i < nv && (app[i] || !g.keep)) o[i] = v[i];
        }
    }
}

template <int V> struct Unit;
template <> struct Unit<1> { typedef uint8_t T; };
template <> struct Unit<2> { typedef uint16_t T; };
template <> struct Unit<4> { typedef uint32_t T; };
template <> struct Unit<8> { typedef uint2 T; };
template <> struct Unit<16> { typedef uint4 T; };

// the bilinear value of a unit of V bytes: V / 2 halves
template <int V>
__device__ __forceinline__ typename Unit<V>::T bilin_unit(const typename Unit<V>::T a, const typename Unit<V>::T b,
                                                          const typename Unit<V>::T c, const typename Unit<V>::T d,
                                                          const float frx, const float fry)
{
    constexpr int NH = V / 2;
    uint16_t ha[NH], hb[NH], hc[NH], hd[NH], r[NH];
    __builtin_memcpy(ha, &a, V); __builtin_memcpy(hb, &b, V); __builtin_memcpy(hc, &c, V); __builtin_memcpy(hd, &d, V);
#pragma unroll
    for (int i = 0; i < NH; i++) r[i] = bilin(ha[i], hb[i], hc[i], hd[i], frx, fry);
    typename Unit<V>::T o;
    __builtin_memcpy(&o, r, V);
    return o;
}

template <int V, int MODE>
__global__ __launch_bounds__(PROP_WG) void k_prop_nhwc(const PropArgs g, const int units, const int lshift)
{
    typedef typename Unit<V>::T T;
    const uint32_t z = blockIdx.z;
    const int lane = (int) threadIdx.x & ((1 << lshift) - 1);
    const int64_t smp = ((int64_t) blockIdx.y * gridDim.x + blockIdx.x) * (PROP_WG >> lshift) + ((int) threadIdx.x >> lshift);
    const int64_t plane = (int64_t) g.fw * g.fh;
    if (smp >= plane) return;
    const int fy = (int) (smp / g.fw), fx = (int) (smp - (int64_t) fy * g.fw);
    const Disp d = prop_disp(g, z, fx, fy);
    if (g.valid && lane == 0) g.valid[(size_t) z * (size_t) plane + (size_t) smp] = d.app ? 1 : 0;
    if (!d.app && g.keep) return;
    T *const o = (T *) (g.dst + (size_t) z * (size_t) g.item) + (size_t) smp * (size_t) units;
    const T *const sp = (const T *) g.src[z];
    if (!d.app) {
        uint64_t f2[2] = { g.fill, g.fill };
        T fv;
        __builtin_memcpy(&fv, f2, V);
        for (int u = lane; u < units; u += 1 << lshift) o[u] = fv;
    } else if (MODE == VP9HIP_WARP_NEAREST) {
        const T *const s = sp + ((size_t) cl(fy + near16(d.py), g.fh) * (size_t) g.fw + (size_t) cl(fx + near16(d.px), g.fw)) * (size_t) units;
        for (int u = lane; u < units; u += 1 << lshift) o[u] = s[u];
    } else if constexpr (V >= 2) {
        const int x0 = fx + whole16(d.px), y0 = fy + whole16(d.py);
        const size_t xa = (size_t) cl(x0, g.fw), xb = (size_t) cl(x0 + 1, g.fw);
        const size_t ya = (size_t) cl(y0, g.fh) * (size_t) g.fw, yb = (size_t) cl(y0 + 1, g.fh) * (size_t) g.fw;
        const T *const s00 = sp + (ya + xa) * (size_t) units, *const s01 = sp + (ya + xb) * (size_t) units;
        const T *const s10 = sp + (yb + xa) * (size_t) units, *const s11 = sp + (yb + xb) * (size_t) units;
        const float frx = (float) phase16(d.px), fry = (float) phase16(d.py);
        for (int u = lane; u < units; u += 1 << lshift) o[u] = bilin_unit<V>(s00[u], s01[u], s10[u], s11[u], frx, fry);
    }
}

template <int E> void nchw_launch(const PropArgs &a, const int mode, const int n, hipStream_t st)
{
    constexpr int NS = E == 1 ? 4 : E == 2 ? 2 : 1;
    const int xtiles = (a.fw + PROP_TW * NS - 1) / (PROP_TW * NS), chunks = (a.c + PROP_CCHUNK - 1) / PROP_CCHUNK;
    const dim3 grid((unsigned) (xtiles * chunks), (unsigned) ((a.fh + PROP_TH - 1) / PROP_TH), (unsigned) n), wg(PROP_TW, PROP_TH);
    if constexpr (E == 2) {
        if (mode == VP9HIP_WARP_BILINEAR) {
            hipLaunchKernelGGL((k_prop_nchw<2, VP9HIP_WARP_BILINEAR>), grid, wg, 0, st, a, xtiles);
            return;
        }
    }
    hipLaunchKernelGGL((k_prop_nchw<E, VP9HIP_WARP_NEAREST>), grid, wg, 0, st, a, xtiles);
}

template <int V> void nhwc_launch(const PropArgs &a, const int mode, const int n, const int64_t bytes, hipStream_t st)
{
    const int units = (int) (bytes / V);
    int lshift = 0;
    while ((1 << lshift) < units && (1 << lshift) < PROP_WG) lshift++;
    const int64_t per = PROP_WG >> lshift, plane = (int64_t) a.fw * a.fh;
    // the workgroups of a pair, folded into x and y: a dimension's threads must stay below 2^32
    const int64_t blocks = (plane + per - 1) / per, gx = blocks < (1 << 20) ? blocks : (1 << 20);
    const dim3 grid((unsigned) gx, (unsigned) ((blocks + gx - 1) / gx), (unsigned) n), wg(PROP_WG);
    if constexpr (V >= 2) {
        if (mode == VP9HIP_WARP_BILINEAR) {
            hipLaunchKernelGGL((k_prop_nhwc<V, VP9HIP_WARP_BILINEAR>), grid, wg, 0, st, a, units, lshift);
            return;
        }
    }
    hipLaunchKernelGGL((k_prop_nhwc<V, VP9HIP_WARP_NEAREST>), grid, wg, 0, st, a, units, lshift);
}

} // namespace

hipError_t vp9hip_prop_launch(const PropArgs &a, int esize, int layout, int mode, int n, hipStream_t st)
{
    if (n < 1 || n > PROP_MAX_PAIRS || a.w < 1 || a.h < 1 || a.fw < 1 || a.fw > 16384 || a.fh < 1 || a.fh > 16384 ||
        a.c < 1 || a.c > 4096 || a.gw < 1 || a.gh < 1 || !a.dst ||
        (esize != 1 && esize != 2 && esize != 4 && esize != 8) ||
        (layout != VP9HIP_PROP_NCHW && layout != VP9HIP_PROP_NHWC) ||
        (mode != VP9HIP_WARP_NEAREST && !(mode == VP9HIP_WARP_BILINEAR && esize == 2)))
        return hipErrorInvalidValue;
    if (layout == VP9HIP_PROP_NCHW || a.c == 1) {
        if (esize == 1) nchw_launch<1>(a, mode, n, st);
        else if (esize == 2) nchw_launch<2>(a, mode, n, st);
        else if (esize == 4) nchw_launch<4>(a, mode, n, st);
        else nchw_launch<8>(a, mode, n, st);
    } else {
        // the widest unit that divides a sample's bytes and every pointer (items are whole samples)
        const int64_t bytes = (int64_t) a.c * esize;
        uintptr_t low = (uintptr_t) bytes | (uintptr_t) a.dst | 16;
        for (int i = 0; i < n; i++) low |= (uintptr_t) a.src[i];
        const int v = (int) (low & (~low + 1));
        if (v < esize) return hipErrorInvalidValue;              // a pointer not aligned to the element
        if (v == 16) nhwc_launch<16>(a, mode, n, bytes, st);
        else if (v == 8) nhwc_launch<8>(a, mode, n, bytes, st);
        else if (v == 4) nhwc_launch<4>(a, mode, n, bytes, st);
        else if (v == 2) nhwc_launch<2>(a, mode, n, bytes, st);
        else nhwc_launch<1>(a, mode, n, bytes, st);
    }
    return hipGetLastError();
}
