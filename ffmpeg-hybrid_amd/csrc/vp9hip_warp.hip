// Accumulated residual for gfx950: k_acc_warp displaces frame b by frame a's accumulated vectors
// and leaves a - warp(b) (or the warped picture itself), the integers of include/vp9hip.h
// ("accumulated residual"), for n pairs in one launch.
//
// Work distribution: blockIdx.z is the pair, blockIdx.y a cell row, and a workgroup is 64 cells
// x the 4 luma rows of that cell row. A lane owns one cell's part of one row: 4 luma samples,
// and one or two of the cell's chroma runs (4 >> ss_h samples each; the cell's 2 (4 >> ss_v)
// chroma rows of U and V are dealt to the four lanes of the cell column). So a wave covers 64
// consecutive cells of one row: its acc read is 1 KiB contiguous (the four waves of a workgroup
// read the same KiB, three of them from the cache), its `a` read 256 / 512 contiguous bytes and
// its store 512 contiguous bytes, one 8-byte store a lane (4 bytes for a 2-sample chroma run).
// Only the `b` gather is irregular: a cell's vector moves its whole run, so the lanes of a wave
// read runs that are contiguous wherever neighbouring cells share a vector.
//
// The pair's record (buffers, field, S_b) sits in the kernel arguments and is indexed by
// blockIdx.z, the sizes and pitches are plain arguments: all wave-uniform, read with scalar
// loads. No LDS, no atomics: every output element has one writer.
//
// Bounds: a lane outside the grid returns before any access; the cell index is clamped to the
// grid all the same. A lane whose run starts outside the visible plane touches no pixel. `a` is
// read and the output written only at x < PW, y < PH (a partial run sample by sample). Every
// `b` coordinate is clamped to 0 .. PW - 1 / 0 .. PH - 1 before its load, also those of a
// partial run's unused samples. Where no column clamp acts and the whole span lies inside the
// visible row (every lane but those whose source is within a few samples of the left or right
// edge), the run's source samples are consecutive bytes and come in one load a row instead of
// one a sample; the address is whatever the vector makes it, and gfx950 serves unaligned global
// loads. The vector loads of `a` and the stores are taken only where the address is aligned to
// their size, else the run goes sample by sample, so odd widths, tight odd-sized outputs and
// unaligned test planes are served by the same kernel.
#include "vp9hip_warp.h"
#include "vp9hip_warp_dev.h"

namespace {

using namespace warpdev;                // cl, vclamp, ld_run, warp_pred: shared with k_acc_warp_scale

// One run of RUN samples of a plane from (x0, y): pa / pb the plane in a and b, PW x PH its
// visible size, (px, py) the cell's vector in 1/16 sample of the plane, drow the output row.
template <typename T, int RUN, int MODE, int OUT>
__device__ __forceinline__ void warp_run(const uint8_t *const pa, const uint8_t *const pb, const size_t pitch,
                                         const int PW, const int PH, const int x0, const int y, const int px,
                                         const int py, const bool app, uint16_t *const drow)
{
    if (x0 >= PW || y >= PH) return;
    const int nv = PW - x0 < RUN ? PW - x0 : RUN;               // visible samples of the run, >= 1
    uint32_t av[RUN], pv[RUN];
#pragma unroll
    for (int i = 0; i < RUN; i++) av[i] = pv[i] = 0;
    if (OUT == VP9HIP_WARP_PICTURE || app) {
        ld_run<T, RUN>(pa + (size_t) y * pitch, x0, nv, av);
    }
    if (app) warp_pred<T, RUN, MODE>(pb, pitch, PW, PH, x0, y, px, py, pv);
    uint32_t o[RUN];
#pragma unroll
    for (int i = 0; i < RUN; i++) {
        if (OUT == VP9HIP_WARP_RESIDUAL) {
            int d = app ? (int) av[i] - (int) pv[i] : 0;
            d = d < -32768 ? -32768 : d > 32767 ? 32767 : d;
            o[i] = (uint32_t) d & 0xffffu;
        } else {
            o[i] = app ? pv[i] : av[i];
        }
    }
    uint16_t *const dp = drow + x0;
    if (nv == RUN && !((uintptr_t) dp & (RUN * 2 - 1))) {
        if (RUN == 4) *(uint2 *) dp = make_uint2(o[0] | o[1] << 16, o[2] | o[3] << 16);
        else if (RUN == 2) *(uint32_t *) dp = o[0] | o[1] << 16;
        else dp[0] = (uint16_t) o[0];
    } else {
#pragma unroll
        for (int i = 0; i < RUN; i++)
            if (i < nv) dp[i] = (uint16_t) o[i];
    }
}

template <typename T, int MODE, int OUT>
__global__ __launch_bounds__(WARP_TW * WARP_TH) void k_acc_warp(const WarpArgs g)
{
    const uint32_t z = blockIdx.z;
    const int c = (int) (blockIdx.x * WARP_TW + threadIdx.x), r = (int) blockIdx.y, j = (int) threadIdx.y;
    if (c >= g.gw || r >= g.gh) return;
    const uint8_t *const fa = g.a[z], *const fb = g.b[z];
    const uint4 q = g.acc[z][(size_t) cl(r, g.gh) * (size_t) g.acc_pitch + (size_t) cl(c, g.gw)];
    const bool app = (q.w & 0xffffu) != 0 && q.z == g.serial[z];
    if (g.mask && j == 0) g.mask[((size_t) z * g.gh + r) * g.gw + c] = app ? 1 : 0;
    const int dx = (int) q.x, dy = (int) q.y;
    const int vx = vclamp(dx), vy = vclamp(dy);
    uint8_t *const out = g.dst + (size_t) z * g.dstride;

    // luma: row 4 r + j, samples 4 c .. 4 c + 3; 1/8 -> 1/16 sample
    {
        const int y = 4 * r + j;
        uint16_t *const drow = (uint16_t *) (out + g.doff[0]) + (size_t) y * g.w;
        warp_run<T, 4, MODE, OUT>(fa + g.off[0], fb + g.off[0], (size_t) g.pitch[0], g.w, g.h, 4 * c, y, vx * 2, vy * 2,
                                  app, drow);
    }
    // chroma: the cell's nr = 4 >> ss_v rows of U, then of V, dealt to j = 0 .. 3
    const int sh = g.ss_h, sv = g.ss_v, lnr = 2 - sv, nr = 1 << lnr;
    const int px = vx * (2 >> sh), py = vy * (2 >> sv);
    for (int t = j; t < 2 * nr; t += WARP_TH) {
        const int p = 1 + (t >> lnr), y = (r << lnr) + (t & (nr - 1));
        uint16_t *const drow = (uint16_t *) (out + g.doff[p]) + (size_t) y * g.cw;
        const uint8_t *const pa = fa + g.off[p], *const pb = fb + g.off[p];
        if (sh) warp_run<T, 2, MODE, OUT>(pa, pb, (size_t) g.pitch[1], g.cw, g.ch, 2 * c, y, px, py, app, drow);
        else warp_run<T, 4, MODE, OUT>(pa, pb, (size_t) g.pitch[1], g.cw, g.ch, 4 * c, y, px, py, app, drow);
    }
}

template <typename T>
void warp_launch(const WarpArgs &a, const int mode, const int output, const dim3 grid, hipStream_t st)
{
    const dim3 wg(WARP_TW, WARP_TH);
    if (mode == VP9HIP_WARP_NEAREST) {
        if (output == VP9HIP_WARP_RESIDUAL) hipLaunchKernelGGL((k_acc_warp<T, VP9HIP_WARP_NEAREST, VP9HIP_WARP_RESIDUAL>), grid, wg, 0, st, a);
        else hipLaunchKernelGGL((k_acc_warp<T, VP9HIP_WARP_NEAREST, VP9HIP_WARP_PICTURE>), grid, wg, 0, st, a);
    } else {
        if (output == VP9HIP_WARP_RESIDUAL) hipLaunchKernelGGL((k_acc_warp<T, VP9HIP_WARP_BILINEAR, VP9HIP_WARP_RESIDUAL>), grid, wg, 0, st, a);
        else hipLaunchKernelGGL((k_acc_warp<T, VP9HIP_WARP_BILINEAR, VP9HIP_WARP_PICTURE>), grid, wg, 0, st, a);
    }
}

} // namespace

hipError_t vp9hip_warp_launch(const WarpArgs &a, int hbd, int mode, int output, int n, hipStream_t st)
{
    if (n < 1 || n > WARP_MAX_PAIRS || a.w < 1 || a.h < 1 || a.gw < 1 || a.gh < 1 || a.gh > 65535 || !a.dst ||
        (mode != VP9HIP_WARP_NEAREST && mode != VP9HIP_WARP_BILINEAR) ||
        (output != VP9HIP_WARP_RESIDUAL && output != VP9HIP_WARP_PICTURE))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned) ((a.gw + WARP_TW - 1) / WARP_TW), (unsigned) a.gh, (unsigned) n);
    if (hbd) warp_launch<uint16_t>(a, mode, output, grid, st);
    else warp_launch<uint8_t>(a, mode, output, grid, st);
    return hipGetLastError();
}
