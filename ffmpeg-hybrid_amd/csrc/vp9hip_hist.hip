// Frame histograms for gfx950: k_hist reads n device frames once and leaves, per frame, the
// counts of include/vp9hip.h ("frame histograms"): C x B int32, C = 3 planes (Y, U, V) or the
// four channels R, G, B, max(R, G, B) of the conversion's codes at the source's depth.
//
// Work distribution: a frame's rectangle, widened on the left to a multiple of 16 columns, is
// cut into blocks of 64 columns x 16 rows (RGBM: 16 row groups of 1 << ss_v luma rows, the rows
// one chroma row covers). The waves of the frame's workgroups (blockIdx.z is the frame) take the
// blocks round robin; inside a block lane l holds the 16 samples at column 16 (l & 3) of row
// (group) l >> 2, as k_metrics does: one 16-byte load at 8 bits, two above. In RGBM mode the lane
// reads its 16 >> ss_h chroma samples of U and of V once and uses them for every luma position
// they cover, in both rows of the group; the matrix is cvtdev::cvt_rgb, the conversion's own.
//
// Bounds: a lane loads only where x < the rectangle's right edge and y < its bottom edge. x is a
// multiple of 16 and the planes' pitches are multiples of 32 samples (64 for luma) that cover the
// configured width, so the 16 samples from x lie inside the row, and the 16 >> ss_h chroma samples
// from x >> ss_h likewise. Samples left of the rectangle (first segment only) and right of it
// are loaded and not counted. A bin index is below B for any stored code: PLANES clamps the code
// to 2^bpp - 1 first, cvt_rgb clips its results to [0, 2^bpp - 1].
//
// Contention. Decoded video is flat: whole waves hit one LDS address and the adds serialise. The
// countermeasure is run combining, carried through a lane's whole walk: a lane keeps, for every
// channel, an open run (bin, count) in registers, a sample of the same bin only increments the
// count, and the run goes to LDS (one ds_add_u32 of the count) when the bin changes, and once at
// the end. In PLANES mode a segment of 16 equal samples joins the run in one step. A constant
// frame so costs one LDS atomic per lane and channel, whatever its size; noise costs one per
// sample as without it. One LDS copy per workgroup (no replication, so the largest tables fit).
//
// Counters: every counter here is 32 bits wide: the LDS bins, the lanes' run counts and the
// output. A frame has at most 2^28 samples, so none can wrap; there is no narrower counter.
//
// LDS per workgroup (dynamic): PLANES B x 4 bytes, the planes one after the other in the same
// table (64 B .. 16 KiB); RGBM 4 x B x 4 bytes (256 B .. 64 KiB at 12 bits, one bin per code).
// Each workgroup adds its non-zero bins to the output with 32-bit global atomics; the launcher
// zeroes the output with a memset on the same stream first. Integer sums commute: the result
// does not depend on the schedule.
#include <algorithm>

#include "vp9hip_convert_dev.h"
#include "vp9hip_hist.h"

namespace {

// A lane's open run of one channel
struct Run { uint32_t bin = 0, cnt = 0; };

__device__ __forceinline__ void run_add(Run &r, uint32_t *const h, const uint32_t bin, const uint32_t cnt)
{
    if (bin != r.bin) {
        if (r.cnt) atomicAdd(h + r.bin, r.cnt);
        r.bin = bin; r.cnt = 0;
    }
    r.cnt += cnt;
}
__device__ __forceinline__ void run_close(Run &r, uint32_t *const h)
{
    if (r.cnt) atomicAdd(h + r.bin, r.cnt);
    r.cnt = 0;
}

// ND dwords from p, aligned to min(4 ND, 16) bytes
template <int ND> __device__ __forceinline__ void load_dwords(const uint8_t *const p, uint32_t (&u)[ND])
{
    if constexpr (ND == 2) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        u[0] = v.x; u[1] = v.y;
    } else {
#pragma unroll
        for (int q = 0; q < ND / 4; q++) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[q];
            u[4 * q] = v.x; u[4 * q + 1] = v.y; u[4 * q + 2] = v.z; u[4 * q + 3] = v.w;
        }
    }
}

// Sample j of the dwords u (j is a constant after unrolling)
template <typename T> __device__ __forceinline__ uint32_t sample(const uint32_t *const u, const int j)
{
    if constexpr (sizeof(T) == 1) return (u[j >> 2] >> (8 * (j & 3))) & 0xffu;
    else return (u[j >> 1] >> (16 * (j & 1))) & 0xffffu;
}

// The part of plane (px, py, pw, ph) that falls to wave gw of nw: into the LDS table h
template <typename T>
__device__ __forceinline__ void hist_plane(uint32_t *const h, const uint8_t *const pl, const size_t pitch, const uint32_t px,
                                           const uint32_t py, const uint32_t pw, const uint32_t ph, const uint32_t maxv,
                                           const uint32_t sh, const uint32_t gw, const uint32_t nw, const uint32_t lane)
{
    constexpr int NDW = 4 * (int) sizeof(T);               // dwords of a lane's 16 samples
    const uint32_t ax0 = px & ~15u, xe = px + pw, ye = py + ph;
    const uint32_t nbx = (xe - ax0 + 63) / 64, nb = nbx * ((ph + 15) / 16);
    Run r;
    for (uint32_t k = gw; k < nb; k += nw) {
        const uint32_t x = ax0 + 64 * (k % nbx) + 16 * (lane & 3), y = py + 16 * (k / nbx) + (lane >> 2);
        if (x >= xe || y >= ye) continue;
        uint32_t u[NDW];
        load_dwords<NDW>(pl + (size_t) y * pitch + (size_t) x * sizeof(T), u);
        const bool whole = x >= px && x + 16 <= xe;
        bool flat = whole && u[0] == __builtin_rotateleft32(u[0], 8 * (int) sizeof(T));
#pragma unroll
        for (int d = 1; d < NDW; d++) flat = flat && u[d] == u[0];
        if (flat) {
            run_add(r, h, min(sample<T>(u, 0), maxv) >> sh, 16u);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (whole || (x + j >= px && x + j < xe)) run_add(r, h, min(sample<T>(u, j), maxv) >> sh, 1u);
        }
    }
    run_close(r, h);
}

// The conversion's arguments that cvt_rgb reads, from the histogram's
__device__ __forceinline__ void hist_cvt(const HistArgs &g, CvtArgs &m)
{
#pragma unroll
    for (int i = 0; i < 5; i++) m.c[i] = g.c[i];
    m.shift = g.shift; m.rnd = g.rnd; m.yoff = g.yoff; m.coff = g.coff; m.rgb = g.rgb;
    m.maxv = (1 << g.bpp) - 1;
}

// The part of the luma rectangle (rx, ry, rw, rh) that falls to wave gw of nw: R, G, B, M into
// the four tables of B bins at h
template <typename T, int SSH>
__device__ __forceinline__ void hist_rgbm(uint32_t *const h, const HistArgs &g, const uint8_t *const src, const uint32_t rx,
                                          const uint32_t ry, const uint32_t rw, const uint32_t rh, const uint32_t B,
                                          const uint32_t sh, const uint32_t gw, const uint32_t nw, const uint32_t lane)
{
    constexpr int NDW = 4 * (int) sizeof(T);               // dwords of a lane's 16 luma samples
    constexpr int NDC = NDW >> SSH;                        // of its 16 >> SSH chroma samples
    CvtArgs m;
    hist_cvt(g, m);
    const uint32_t ssv = (uint32_t) g.ss_v;
    const uint32_t ax0 = rx & ~15u, xe = rx + rw, ye = ry + rh;
    const uint32_t nbx = (xe - ax0 + 63) / 64, ngr = (rh + ssv) >> ssv, nb = nbx * ((ngr + 15) / 16);
    const size_t pitch = (size_t) g.pitch[0], cpitch = (size_t) g.pitch[1];
    const uint8_t *const py = src + g.off[0], *const pu = src + g.off[1], *const pv = src + g.off[2];
    Run rr, rg, rb, rm;
    for (uint32_t k = gw; k < nb; k += nw) {
        const uint32_t x = ax0 + 64 * (k % nbx) + 16 * (lane & 3);
        const uint32_t y0 = ry + ((16 * (k / nbx) + (lane >> 2)) << ssv);    // ry is a multiple of 1 << ss_v
        if (x >= xe || y0 >= ye) continue;
        uint32_t cu[NDC], cv[NDC];
        const size_t cat = (size_t) (y0 >> ssv) * cpitch + (size_t) (x >> SSH) * sizeof(T);
        load_dwords<NDC>(pu + cat, cu);
        load_dwords<NDC>(pv + cat, cv);
        const bool whole = x >= rx && x + 16 <= xe;
#pragma unroll
        for (uint32_t row = 0; row < 2; row++) {
            const uint32_t y = y0 + row;
            if (row > ssv || y >= ye) break;
            uint32_t u[NDW];
            load_dwords<NDW>(py + (size_t) y * pitch + (size_t) x * sizeof(T), u);
#pragma unroll
            for (int j = 0; j < 16; j++) {
                if (!(whole || (x + j >= rx && x + j < xe))) continue;
                int R, G, Bc;
                cvtdev::cvt_rgb(m, (int) sample<T>(u, j), (int) sample<T>(cu, j >> SSH), (int) sample<T>(cv, j >> SSH), R, G, Bc);
                const int M = max(R, max(G, Bc));
                run_add(rr, h, (uint32_t) R >> sh, 1u);
                run_add(rg, h + B, (uint32_t) G >> sh, 1u);
                run_add(rb, h + 2 * B, (uint32_t) Bc >> sh, 1u);
                run_add(rm, h + 3 * B, (uint32_t) M >> sh, 1u);
            }
        }
    }
    run_close(rr, h); run_close(rg, h + B); run_close(rb, h + 2 * B); run_close(rm, h + 3 * B);
}

// The workgroup's non-zero bins [0, count) into the output, the table left zero
__device__ __forceinline__ void hist_flush(uint32_t *const h, int32_t *const out, const uint32_t count, const uint32_t tid)
{
    for (uint32_t i = tid; i < count; i += HIST_WG) {
        const uint32_t v = h[i];
        if (v) {
            atomicAdd(out + i, (int32_t) v);
            h[i] = 0;
        }
    }
}

template <typename T, int RGBM, int SSH>
__global__ __launch_bounds__(HIST_WG) void k_hist(const HistArgs g)
{
    extern __shared__ uint32_t hist[];
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t z = blockIdx.z;
    const uint32_t B = 1u << g.bins_log2, sh = (uint32_t) (g.bpp - g.bins_log2), maxv = (1u << g.bpp) - 1u;
    const uint32_t gw = blockIdx.x * (HIST_WG / 64) + wave, nw = gridDim.x * (HIST_WG / 64);
    const vp9hip_rect rc = g.rect[z];
    const uint8_t *const src = g.src[z];
    constexpr uint32_t C = RGBM ? 4 : 3;
    int32_t *const out = g.out + (size_t) z * C * B;

    for (uint32_t i = tid; i < (RGBM ? 4 * B : B); i += HIST_WG) hist[i] = 0;
    __syncthreads();
    if constexpr (RGBM) {
        hist_rgbm<T, SSH>(hist, g, src, (uint32_t) rc.x, (uint32_t) rc.y, (uint32_t) rc.w, (uint32_t) rc.h, B, sh, gw, nw, lane);
        __syncthreads();
        hist_flush(hist, out, 4 * B, tid);
    } else {
#pragma unroll 1
        for (int p = 0; p < 3; p++) {
            const uint32_t s_h = p ? g.ss_h : 0, s_v = p ? g.ss_v : 0;
            hist_plane<T>(hist, src + g.off[p], (size_t) g.pitch[p ? 1 : 0], (uint32_t) rc.x >> s_h, (uint32_t) rc.y >> s_v,
                          ((uint32_t) rc.w + s_h) >> s_h, ((uint32_t) rc.h + s_v) >> s_v, maxv, sh, gw, nw, lane);
            __syncthreads();
            hist_flush(hist, out + p * B, B, tid);          // leaves the table zero for the next plane
            __syncthreads();
        }
    }
}

} // namespace

hipError_t vp9hip_hist_launch(const HistArgs &a, int hbd, int n, hipStream_t st)
{
    if (n < 1 || n > HIST_MAX_FRAMES || !a.out || a.bins_log2 < 4 || a.bins_log2 > a.bpp) return hipErrorInvalidValue;
    const bool rgbm = a.what == VP9HIP_HIST_RGBM;
    const size_t B = (size_t) 1 << a.bins_log2, C = rgbm ? 4 : 3;
    // The grid: the frame with the most blocks gets a workgroup for every 4 HIST_MIN_BLOCKS of its
    // blocks, but no more than its share of HIST_FILL: every workgroup ends with up to C B global
    // atomics, so a frame is given few workgroups with long walks rather than many short ones.
    int64_t nb = 1;
    for (int i = 0; i < n; i++) {
        const vp9hip_rect &r = a.rect[i];
        const int64_t cols = (r.x + r.w - (r.x & ~15) + 63) / 64;
        const int64_t rows = rgbm ? (((r.h + a.ss_v) >> a.ss_v) + 15) / 16 : (r.h + 15) / 16;
        nb = std::max(nb, cols * rows);
    }
    const int64_t cap = std::max(HIST_FILL / n, 1);
    const int64_t wgs = std::min((nb + 4 * HIST_MIN_BLOCKS - 1) / (4 * HIST_MIN_BLOCKS), cap);
    hipError_t e = hipMemsetAsync(a.out, 0, (size_t) n * C * B * sizeof(int32_t), st);
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned) wgs, 1, (unsigned) n), wg(HIST_WG);
    const size_t lds = (rgbm ? 4 : 1) * B * sizeof(uint32_t);
    if (!rgbm) {
        if (hbd) hipLaunchKernelGGL((k_hist<uint16_t, 0, 0>), grid, wg, lds, st, a);
        else hipLaunchKernelGGL((k_hist<uint8_t, 0, 0>), grid, wg, lds, st, a);
    } else if (a.ss_h) {
        if (hbd) hipLaunchKernelGGL((k_hist<uint16_t, 1, 1>), grid, wg, lds, st, a);
        else hipLaunchKernelGGL((k_hist<uint8_t, 1, 1>), grid, wg, lds, st, a);
    } else {
        if (hbd) hipLaunchKernelGGL((k_hist<uint16_t, 1, 0>), grid, wg, lds, st, a);
        else hipLaunchKernelGGL((k_hist<uint8_t, 1, 0>), grid, wg, lds, st, a);
    }
    return hipGetLastError();
}
