// Residual tensors at model size for gfx950: the visible w x h of the residual fields' three
// int16 planes -> planar 3 x out_h x out_w, YUV or the RGB residual, int16 or half, n frames per
// launch (blockIdx.z), reading each visible sample about once and writing only the small output.
// The definition is include/vp9hip.h "residual tensors at model size" / DESIGN.md 15a.
//
// sbox(P, ow, oh) = floor((A + (w h >> 1)) / (w h)), A the exact signed area sum with the box
// filter's weights. The weights of one output sum to w h, so sbox(P) = box(P ^ 0x8000) - 32768
// with the stored code read as u16: flipping the sign bit adds 32768 to every sample. That form
// is taken here: everything is unsigned, the bounds are k_convert_scale's (column sums
// < h * 65535 < 2^30, quotient < 2^16), the division is rounded_quot as it stands, and its floor
// of a non-negative number is the floor the definition asks of the signed one.
//
// The shape is k_convert_scale's (vp9hip_convert_scale.hip):
//   - a workgroup owns 128 x 4 outputs, one output row per wave, two columns per lane;
//   - the wave walks its row's source rows in chunks of 256 source columns, each lane loading
//     4 consecutive int16 per row (8 B, coalesced) and adding wy * (sample ^ 0x8000) into four
//     u32 column sums;
//   - the column sums go to LDS once per chunk, and each lane adds wx * sum over the part of its
//     two columns' footprints inside the chunk, in 64 bits;
//   - one division per output sample through the host's double 1 / (w h) and the exact
//     remainder.
// U and V have one geometry and go in one pass. All three planes resample to one grid, so a lane
// holds y, u, v of its pixels and runs the matrix and the stores. Loads are aligned groups of 4
// samples below the footprint's end, which is at most the visible width, so they stay inside the
// field's 64-padded plane, and what lies beyond the visible size has weight zero. Stores are per
// element, lanes on consecutive pixels, only at ox < out_w, oy < out_h. The row routine is this
// file's own (the sample's flip is the one thing add_row does not do).
#include "vp9hip_convert_dev.h"
#include "vp9hip_resid_dev.h"
#include "vp9hip_residual_scale.h"

#include <array>
#include <utility>

namespace {

using namespace cvtdev;

__device__ __forceinline__ uint32_t overlap(int lo, int n_src, int so, int n_out)
{
    return (uint32_t) (min(lo + n_src, so + n_out) - max(lo, so));
}

// v[i] += wy * (sample i ^ 0x8000) of the 4 int16 at p (aligned to their 8 bytes)
__device__ __forceinline__ void add_row_flipped(const uint8_t *p, uint32_t wy, uint32_t (&v)[4])
{
    uint2 s = *reinterpret_cast<const uint2 *>(p);
    s.x ^= 0x80008000u; s.y ^= 0x80008000u;
    v[0] += wy * (s.x & 0xffff); v[1] += wy * (s.x >> 16);
    v[2] += wy * (s.y & 0xffff); v[3] += wy * (s.y >> 16);
}

// out[p][k] = sbox(P[p], ow, oh) at (tx0 + lane + 64 k, oy), k = 0, 1, for NP planes of one
// w x h geometry. All waves of the workgroup call this together with the same tx0 (the
// barriers); a wave whose row is outside (row_ok false) and lanes whose column is outside take
// part with empty ranges (their result is not stored). cs: this wave's NP x CHUNK column sums.
template <int NP>
__device__ __forceinline__ void sbox_row(const uint8_t *const (&P)[NP], int pitch, int w, int h, int ow, int oh, int tx0,
                                         int oy, bool row_ok, double rcp, double rx, double ry, uint32_t *cs, int lane,
                                         int (&out)[NP][2])
{
    const int fx0 = floordiv(tx0 * w, ow, rx), fx1 = floordiv(min(tx0 + TW, ow) * w + ow - 1, ow, rx);
    const int ylo = oy * h;
    const int sy0 = row_ok ? floordiv(ylo, oh, ry) : 0, sy1 = row_ok ? floordiv(ylo + h + oh - 1, oh, ry) : 0;
    int xlo[2], xa[2], xb[2];
    uint64_t acc[NP][2] = {};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 + lane + 64 * k;
        const bool ok = row_ok && ox < ow;
        xlo[k] = ox * w;
        xa[k] = ok ? floordiv(xlo[k], ow, rx) : 0;
        xb[k] = ok ? floordiv(xlo[k] + w + ow - 1, ow, rx) : 0;
    }
    for (int c0 = fx0 & ~3; c0 < fx1; c0 += CHUNK) {
        const int sx = c0 + lane * 4;
        uint32_t v[NP][4] = {};
        if (sx < fx1) {
            const int64_t o = (int64_t) sy0 * pitch + (int64_t) sx * 2;
            int so = sy0 * oh;
#pragma unroll 4
            for (int sy = sy0; sy < sy1; sy++, so += oh) {
                const uint32_t wy = overlap(ylo, h, so, oh);
#pragma unroll
                for (int p = 0; p < NP; p++) add_row_flipped(P[p] + o + (int64_t) (sy - sy0) * pitch, wy, v[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < NP; p++)
            reinterpret_cast<uint4 *>(cs + p * CHUNK)[lane] = make_uint4(v[p][0], v[p][1], v[p][2], v[p][3]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int s0 = max(xa[k], c0), s1 = min(xb[k], c0 + CHUNK);
            int so = s0 * ow;
            for (int s = s0; s < s1; s++, so += ow) {
                const uint32_t wx = overlap(xlo[k], w, so, ow);
#pragma unroll
                for (int p = 0; p < NP; p++) acc[p][k] += (uint64_t) wx * cs[p * CHUNK + s - c0];
            }
        }
        __syncthreads();
    }
    const uint64_t den = (uint64_t) w * (uint64_t) h;
#pragma unroll
    for (int p = 0; p < NP; p++)
#pragma unroll
        for (int k = 0; k < 2; k++) out[p][k] = rounded_quot(acc[p][k], den, rcp) - 32768;
}

// FMT: VP9HIP_RESID_*: bit 1 the RGB matrix, bit 0 the half output
template <int FMT>
__global__ __launch_bounds__(256) void k_residual_scale(const ResidScaleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t colsum[TH][2 * CHUNK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx0 = blockIdx.x * TW, oy = blockIdx.y * TH + wave;
    const uint8_t *src = a.src[blockIdx.z];
    uint8_t *dst = a.dst + (int64_t) blockIdx.z * a.frame_stride;
    uint32_t *cs = colsum[wave];
    const bool row_ok = oy < a.oh;

    int Yk[1][2], UV[2][2];
    const uint8_t *const py[1] = { src + a.src_off[0] }, *const puv[2] = { src + a.src_off[1], src + a.src_off[2] };
    sbox_row<1>(py, a.src_pitch[0], a.w, a.h, a.ow, a.oh, tx0, oy, row_ok, a.rcp[0], a.rx, a.ry, cs, lane, Yk);
    sbox_row<2>(puv, a.src_pitch[1], a.cw, a.ch, a.ow, a.oh, tx0, oy, row_ok, a.rcp[1], a.rx, a.ry, cs, lane, UV);
    if (!row_ok) return;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 + lane + 64 * k;
        if (ox >= a.ow) continue;
        residdev::resid_store_px<FMT>(a, dst, ox, oy, Yk[0][k], UV[0][k], UV[1][k]);   // shared with k_acc_warp_scale
    }
}

typedef void (*KFn)(const ResidScaleArgs);
template <size_t... I>
constexpr std::array<KFn, sizeof...(I)> kernel_table(std::index_sequence<I...>)
{
    return { { k_residual_scale<(int) I>... } };
}
const std::array<KFn, 4> g_kernels = kernel_table(std::make_index_sequence<4>());

}  // namespace

hipError_t vp9hip_residual_scale_launch(const ResidScaleArgs &a, int format, int n, hipStream_t st)
{
    if (format < 0 || format > 3 || n < 1 || n > RSC_MAX_FRAMES) return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_kernels[format], cvt_tile_grid(a.ow, a.oh, n), dim3(64 * TH, 1, 1), 0, st, a);
    return hipGetLastError();
}
