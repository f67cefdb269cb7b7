// Accumulated residual at model size for gfx950: k_acc_warp_scale displaces frame b by frame a's
// accumulated vectors, takes a - warp(b) and box-resamples it to out_w x out_h in the same
// launch: planar (3 or 4) x out_h x out_w, YUV or the RGB residual, int16 or half, n pairs per
// launch (blockIdx.z). The full-size residual planes k_acc_warp would store, and a second kernel
// read back, never exist. The definition is include/vp9hip.h "accumulated residual at model
// size" / DESIGN.md 18a: the composition of "accumulated residual" and "residual tensors at
// model size".
//
// The shape is k_residual_scale's (vp9hip_residual_scale.hip), with the sample computed instead
// of loaded:
//   - a workgroup owns 128 x 4 outputs, one output row per wave, two columns per lane;
//   - the wave walks its row's source rows in chunks of 256 source columns; a lane owns 4
//     consecutive source samples aligned to 4: in luma and in 4:4:4 chroma one 4 x 4 cell's run
//     (k_acc_warp's unit), in 4:2:0 chroma two cells' 2-sample runs;
//   - a lane's field record (16 B, 1 KiB contiguous a wave) is loaded once per cell row, and the
//     next cell row's is issued before this one's picture loads, so the dependent `b` gather
//     does not wait behind it row by row;
//   - a's samples of a cell row's source rows (4 luma rows, 2 or 4 chroma rows) are loaded
//     together, before the first b gather, which has to wait for the record: one round trip a
//     cell row for them instead of one a row behind the gather's;
//   - per source row r = applies ? clamp(a - pred, int16) : 0 for the run (the prediction is
//     vp9hip_warp_dev.h's, as k_acc_warp computes it; where the cell does not apply nothing is
//     loaded), and
//     wy * (r + 32768) goes into four u32 column sums: the unsigned form of sbox, with the
//     bounds of k_residual_scale (column sums < h * 65535 < 2^30, quotient < 2^16);
//   - the column sums go to LDS once per chunk, each lane adds wx * sum over the part of its two
//     columns' footprints inside the chunk in 64 bits, and one division per output sample goes
//     through the host's double 1 / (w h) and the exact remainder;
//   - the coverage is one more column sum of the luma pass, 256 wy per applying cell: all four
//     samples of a lane share a cell, so it is one value a lane.
// U and V share geometry, vector and verdict and go in one pass. All planes resample to one
// grid, so a lane holds y, u, v (and the coverage) of its pixels and runs the matrix and the
// stores (vp9hip_resid_dev.h, as k_residual_scale does).
//
// The pair's record (buffers, field, S_b) sits in the kernel arguments and is indexed by
// blockIdx.z; sizes and pitches are plain arguments: all wave-uniform. No atomics, no inline
// assembly; LDS only for the column sums.
//
// Bounds: source columns are walked only below the footprint's end, which is at most the visible
// width, and source rows below the visible height, so `a` is read only at x < PW, y < PH (a
// partial run sample by sample: the planes may be exact-size and oddly pitched). Every `b`
// coordinate is clamped before its load. The cell index is clamped to the grid. Samples of a
// run beyond the visible width are not read; their column sums are never used. Vector loads are
// taken only at addresses aligned to their size, except the `b` span load, as in k_acc_warp.
// Stores are per element, only at ox < out_w, oy < out_h.
#include "vp9hip_convert_dev.h"
#include "vp9hip_resid_dev.h"
#include "vp9hip_warp_dev.h"
#include "vp9hip_warp_scale.h"

namespace {

using namespace cvtdev;
using warpdev::cl;
using warpdev::vclamp;

__device__ __forceinline__ uint32_t overlap(int lo, int n_src, int so, int n_out)
{
    return (uint32_t) (min(lo + n_src, so + n_out) - max(lo, so));
}

// A cell's verdict and its vector in 1/16 sample of a plane (mx = 2 >> ss_h, my = 2 >> ss_v)
struct Cell { int px, py; bool app; };

__device__ __forceinline__ Cell cell_of(const uint4 q, const uint32_t serial, const int mx, const int my)
{
    const int dx = (int) q.x, dy = (int) q.y;
    Cell c;
    c.app = (q.w & 0xffffu) != 0 && q.z == serial;
    c.px = vclamp(dx) * mx;
    c.py = vclamp(dy) * my;
    return c;
}

// a's 4 samples from x0 of row ra, packed as they lie in memory (8 bit: x; 16 bit: x, y), nv of
// them visible (1..4), the others 0: one vector load where the run is whole and aligned to its
// size, else a load a sample
template <typename T> __device__ __forceinline__ uint2 ld_a4(const uint8_t *const ra, const int x0, const int nv)
{
    const uint8_t *const at = ra + (size_t) x0 * sizeof(T);
    uint32_t lo = 0, hi = 0;
    if (nv == 4 && !((uintptr_t) at & (4 * sizeof(T) - 1))) {
        if (sizeof(T) == 2) { const uint2 r = *(const uint2 *) at; lo = r.x; hi = r.y; }
        else lo = *(const uint32_t *) at;
    } else {
        const uint32_t s0 = warpdev::ld<T>(ra, x0), s1 = nv > 1 ? warpdev::ld<T>(ra, x0 + 1) : 0;
        const uint32_t s2 = nv > 2 ? warpdev::ld<T>(ra, x0 + 2) : 0, s3 = nv > 3 ? warpdev::ld<T>(ra, x0 + 3) : 0;
        if (sizeof(T) == 2) { lo = s0 | s1 << 16; hi = s2 | s3 << 16; }
        else lo = s0 | s1 << 8 | s2 << 16 | s3 << 24;
    }
    return make_uint2(lo, hi);
}

// sample i of ld_a4's 4
template <typename T, int I> __device__ __forceinline__ uint32_t a4_sample(const uint2 r)
{
    if (sizeof(T) == 2) return ((I < 2 ? r.x : r.y) >> (16 * (I & 1))) & 0xffffu;
    return (r.x >> (8 * I)) & 0xffu;
}

// row j of a cell row's 4 (j is wave-uniform: selects, no indexed registers)
__device__ __forceinline__ uint32_t row_of(const uint32_t (&a)[4], const int j)
{
    return j == 0 ? a[0] : j == 1 ? a[1] : j == 2 ? a[2] : a[3];
}

// v[i] += wy * (r_i + 32768), r the accumulated residual of the RUN samples from (x0, y) of a
// plane, x0 < PW, y < PH: ar a's samples from ld_a4, the run's first at index I0; pb the plane in
// b, PW x PH its visible size
template <typename T, int RUN, int MODE, int I0>
__device__ __forceinline__ void add_run(const uint2 ar, const uint8_t *const pb, const size_t pitch, const int PW,
                                        const int PH, const int x0, const int y, const Cell &c, const uint32_t wy,
                                        uint32_t *const v)
{
    uint32_t code[RUN];
#pragma unroll
    for (int i = 0; i < RUN; i++) code[i] = 32768;
    if (c.app) {
        uint32_t pv[RUN];
#pragma unroll
        for (int i = 0; i < RUN; i++) pv[i] = 0;
        warpdev::warp_pred<T, RUN, MODE>(pb, pitch, PW, PH, x0, y, c.px, c.py, pv);
        const uint32_t av[4] = { a4_sample<T, 0>(ar), a4_sample<T, 1>(ar), a4_sample<T, 2>(ar), a4_sample<T, 3>(ar) };
#pragma unroll
        for (int i = 0; i < RUN; i++) {
            int d = (int) av[I0 + i] - (int) pv[i];
            d = d < -32768 ? -32768 : d > 32767 ? 32767 : d;
            code[i] = (uint32_t) (d + 32768);
        }
    }
#pragma unroll
    for (int i = 0; i < RUN; i++) v[i] += wy * code[i];
}

// out[p][k] = sbox(R_p, ow, oh) at (tx0 + lane + 64 k, oy), k = 0, 1, of pair z: CH false: the
// luma plane, and cov[k] the coverage; CH true: U and V. All waves of the workgroup call this
// together with the same tx0 (the barriers); a wave whose row is outside (row_ok false) and lanes
// whose column is outside take part with empty ranges (their result is not stored). cs: this
// wave's 2 x CHUNK column sums.
template <typename T, int MODE, bool CH>
__device__ __forceinline__ void warp_sbox_row(const WarpScaleArgs &a, const int z, const int tx0, const int oy,
                                              const bool row_ok, uint32_t *const cs, const int lane,
                                              int (&out)[CH ? 2 : 1][2], int (&cov)[2])
{
    constexpr int NP = CH ? 2 : 1;
    const int sh = CH ? a.ss_h : 0, sv = CH ? a.ss_v : 0;
    const int w = CH ? a.cw : a.w, h = CH ? a.ch : a.h, ow = a.ow, oh = a.oh;
    const size_t pitch = (size_t) a.src_pitch[CH ? 1 : 0];
    const double rcp = a.rcp[CH ? 1 : 0];
    const uint8_t *pa[NP], *pb[NP];
#pragma unroll
    for (int p = 0; p < NP; p++) {
        pa[p] = a.a[z] + a.off[CH ? 1 + p : 0];
        pb[p] = a.b[z] + a.off[CH ? 1 + p : 0];
    }
    const uint4 *const field = a.acc[z];
    const uint32_t serial = a.serial[z];
    const int mx = 2 >> sh, my = 2 >> sv;
    const bool two = CH && sh;                                  // the lane's 4 samples lie in two cells

    const int fx0 = floordiv(tx0 * w, ow, a.rx), fx1 = floordiv(min(tx0 + TW, ow) * w + ow - 1, ow, a.rx);
    const int ylo = oy * h;
    const int sy0 = row_ok ? floordiv(ylo, oh, a.ry) : 0, sy1 = row_ok ? floordiv(ylo + h + oh - 1, oh, a.ry) : 0;
    int xlo[2], xa[2], xb[2];
    uint64_t acc[NP][2] = {}, cacc[2] = {};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 + lane + 64 * k;
        const bool ok = row_ok && ox < ow;
        xlo[k] = ox * w;
        xa[k] = ok ? floordiv(xlo[k], ow, a.rx) : 0;
        xb[k] = ok ? floordiv(xlo[k] + w + ow - 1, ow, a.rx) : 0;
    }
    for (int c0 = fx0 & ~3; c0 < fx1; c0 += CHUNK) {
        const int sx = c0 + lane * 4;
        uint32_t v[NP][4] = {};
        uint32_t vc = 0;
        if (sx < fx1 && sy0 < sy1) {
            const int cc0 = cl((sx << sh) >> 2, a.gw), cc1 = cl(cc0 + 1, a.gw);
            int r = (sy0 << sv) >> 2;
            const uint4 *frow = field + (size_t) cl(r, a.gh) * (size_t) a.acc_pitch;
            uint4 q0 = frow[cc0], q1 = q0;
            if (two) q1 = frow[cc1];
            int sy = sy0, so = sy0 * oh;
            while (sy < sy1) {
                const int rend = min(sy1, ((r + 1) << 2) >> sv);     // the end of cell row r's source rows
                const Cell k0 = cell_of(q0, serial, mx, my), k1 = cell_of(q1, serial, mx, my);
                if (rend < sy1) {                                   // the next cell row's records, in flight over this one's rows
                    frow = field + (size_t) cl(r + 1, a.gh) * (size_t) a.acc_pitch;
                    q0 = frow[cc0]; q1 = q0;
                    if (two) q1 = frow[cc1];
                }
                // a's samples of this cell row's source rows, all in flight before the first b gather,
                // which depends on the record; where the cell does not apply nothing is loaded
                const int nrow = rend - sy, nva = w - sx < 4 ? w - sx : 4;
                uint32_t alo[NP][4], ahi[NP][4];
#pragma unroll
                for (int p = 0; p < NP; p++)
#pragma unroll
                    for (int j = 0; j < 4; j++) alo[p][j] = ahi[p][j] = 0;
                if (k0.app || (two && k1.app)) {
#pragma unroll
                    for (int j = 0; j < 4; j++)
                        if (j < nrow) {
#pragma unroll
                            for (int p = 0; p < NP; p++) {
                                const uint2 r = ld_a4<T>(pa[p] + (size_t) (sy + j) * pitch, sx, nva);
                                alo[p][j] = r.x; ahi[p][j] = r.y;
                            }
                        }
                }
                for (int j = 0; j < nrow; j++, sy++, so += oh) {
                    const uint32_t wy = overlap(ylo, h, so, oh);
#pragma unroll
                    for (int p = 0; p < NP; p++) {
                        const uint2 a4 = make_uint2(row_of(alo[p], j), row_of(ahi[p], j));
                        if (two) {
                            add_run<T, 2, MODE, 0>(a4, pb[p], pitch, w, h, sx, sy, k0, wy, &v[p][0]);
                            if (sx + 2 < fx1) add_run<T, 2, MODE, 2>(a4, pb[p], pitch, w, h, sx + 2, sy, k1, wy, &v[p][2]);
                        } else {
                            add_run<T, 4, MODE, 0>(a4, pb[p], pitch, w, h, sx, sy, k0, wy, &v[p][0]);
                        }
                    }
                    if (!CH) vc += k0.app ? wy * 256 : 0;
                }
                r++;
            }
        }
#pragma unroll
        for (int p = 0; p < NP; p++)
            reinterpret_cast<uint4 *>(cs + p * CHUNK)[lane] = make_uint4(v[p][0], v[p][1], v[p][2], v[p][3]);
        if (!CH) cs[CHUNK + lane] = vc;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int s0 = max(xa[k], c0), s1 = min(xb[k], c0 + CHUNK);
            int so = s0 * ow;
            for (int s = s0; s < s1; s++, so += ow) {
                const uint32_t wx = overlap(xlo[k], w, so, ow);
#pragma unroll
                for (int p = 0; p < NP; p++) acc[p][k] += (uint64_t) wx * cs[p * CHUNK + s - c0];
                if (!CH) cacc[k] += (uint64_t) wx * cs[CHUNK + ((s - c0) >> 2)];
            }
        }
        __syncthreads();
    }
    const uint64_t den = (uint64_t) w * (uint64_t) h;
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
        for (int p = 0; p < NP; p++) out[p][k] = rounded_quot(acc[p][k], den, rcp) - 32768;
        if (!CH) cov[k] = rounded_quot(cacc[k], den, rcp);
    }
}

// T: the sample type; MODE: VP9HIP_WARP_*; FMT: VP9HIP_RESID_*: bit 1 the RGB matrix, bit 0 the half output
template <typename T, int MODE, int FMT>
__global__ __launch_bounds__(256) void k_acc_warp_scale(const WarpScaleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t colsum[TH][2 * CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx0 = blockIdx.x * TW, oy = blockIdx.y * TH + wave, z = blockIdx.z;
    uint8_t *dst = a.dst + (int64_t) z * a.frame_stride;
    uint32_t *cs = colsum[wave];
    const bool row_ok = oy < a.oh;

    int Yk[1][2], UV[2][2], C[2] = { 0, 0 }, unused[2];
    warp_sbox_row<T, MODE, false>(a, z, tx0, oy, row_ok, cs, lane, Yk, C);
    warp_sbox_row<T, MODE, true>(a, z, tx0, oy, row_ok, cs, lane, UV, unused);
    if (!row_ok) return;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 + lane + 64 * k;
        if (ox >= a.ow) continue;
        residdev::resid_store_px<FMT>(a, dst, ox, oy, Yk[0][k], UV[0][k], UV[1][k]);
        if (a.cov) {
            uint8_t *row = dst + 3 * a.plane + (int64_t) oy * a.pitch;
            if constexpr ((FMT & 1) != 0) reinterpret_cast<_Float16 *>(row)[ox] = to_half(C[k], 1.0f / 256);
            else reinterpret_cast<int16_t *>(row)[ox] = (int16_t) C[k];
        }
    }
}

template <typename T, int MODE>
void launch_format(const WarpScaleArgs &a, const int format, const dim3 grid, hipStream_t st)
{
    const dim3 wg(64 * TH, 1, 1);
    switch (format) {
    case VP9HIP_RESID_YUV_I16: hipLaunchKernelGGL((k_acc_warp_scale<T, MODE, VP9HIP_RESID_YUV_I16>), grid, wg, 0, st, a); break;
    case VP9HIP_RESID_YUV_F16: hipLaunchKernelGGL((k_acc_warp_scale<T, MODE, VP9HIP_RESID_YUV_F16>), grid, wg, 0, st, a); break;
    case VP9HIP_RESID_RGB_I16: hipLaunchKernelGGL((k_acc_warp_scale<T, MODE, VP9HIP_RESID_RGB_I16>), grid, wg, 0, st, a); break;
    default: hipLaunchKernelGGL((k_acc_warp_scale<T, MODE, VP9HIP_RESID_RGB_F16>), grid, wg, 0, st, a); break;
    }
}

template <typename T>
void launch_mode(const WarpScaleArgs &a, const int mode, const int format, const dim3 grid, hipStream_t st)
{
    if (mode == VP9HIP_WARP_NEAREST) launch_format<T, VP9HIP_WARP_NEAREST>(a, format, grid, st);
    else launch_format<T, VP9HIP_WARP_BILINEAR>(a, format, grid, st);
}

}  // namespace

hipError_t vp9hip_warp_scale_launch(const WarpScaleArgs &a, int hbd, int mode, int format, int n, hipStream_t st)
{
    if (format < VP9HIP_RESID_YUV_I16 || format > VP9HIP_RESID_RGB_F16 || n < 1 || n > WSC_MAX_PAIRS || !a.dst ||
        (mode != VP9HIP_WARP_NEAREST && mode != VP9HIP_WARP_BILINEAR) || a.w < 1 || a.h < 1 || a.cw < 1 || a.ch < 1 ||
        a.gw < 1 || a.gh < 1 || a.ow < 1 || a.oh < 1)
        return hipErrorInvalidValue;
    const dim3 grid = cvt_tile_grid(a.ow, a.oh, n);
    if (hbd) launch_mode<uint16_t>(a, mode, format, grid, st);
    else launch_mode<uint8_t>(a, mode, format, grid, st);
    return hipGetLastError();
}
