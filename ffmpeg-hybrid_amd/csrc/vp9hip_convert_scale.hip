// Fused crop + box-filter resize + output conversion for gfx950: the visible w x h of the
// decoder's planes -> out_w x out_h semi-planar, RGB24, planar RGB u8 or planar RGB half,
// n frames per launch (blockIdx.z), reading each visible sample about once and writing only
// the small output.
//
// box(P, ow, oh) is the exact area mean of include/vp9hip.h / DESIGN.md "Box-filter resize":
//   A(ox, oy) = sum_sy wy(oy, sy) sum_sx wx(ox, sx) P[sy][sx],   box = (A + (w h >> 1)) / (w h)
// with the overlap weights computed from the formula where they are used (no tables). The sum
// is exact in any order; this kernel takes the columns first, because that order needs no
// cross-lane step per source row:
//   - a workgroup owns 128 x 4 output pixels, one output row per wave, two columns per lane;
//   - the wave walks its row's source rows in chunks of 256 source columns, each lane loading
//     4 consecutive samples per row (4 B / 8 B, coalesced) and adding wy * sample into four
//     int32 column sums (< h * 65535 < 2^30);
//   - the column sums go to LDS once per chunk, and each lane adds wx * sum over the part of
//     its two columns' footprints inside the chunk, in 64 bits;
//   - one division per output sample: the host's double 1 / (w h) gives the quotient to
//     within one (it is below 2^16, the estimate's error below 2^-30), and the exact 64-bit
//     remainder corrects it.
// The chunk loop covers any footprint (-> 1 x 1 walks the whole plane with one wave: correct,
// not fast). U and V have one geometry and are taken in one pass. The three planes of an RGB
// output are resampled to the same grid, so a lane holds Y, U and V of its pixels and runs the
// matrix of the full-size conversion (cvt_store_px, vp9hip_convert_dev.h). Semi-planar chroma
// has its own grid (OCW x OCH): the workgroups whose tile lies inside it take it too. The footprints' bounds are divisions by
// an argument; they use the host's reciprocal and a correction as the quotient does. Loads
// are aligned groups of 4 samples below the footprint's end, which is at most the visible
// width, so they stay inside the 64-padded plane and padding has weight zero. Stores are per
// element, lanes on consecutive pixels, only at ox < out_w, oy < out_h.
#include "vp9hip_convert_dev.h"

#include <array>
#include <utility>

namespace {

using namespace cvtdev;

// lo = o n_src: the overlap of [lo, lo + n_src) and [so, so + n_out), so = s n_out: the weight
// of source s for output o
__device__ __forceinline__ uint32_t overlap(int lo, int n_src, int so, int n_out)
{
    return (uint32_t) (min(lo + n_src, so + n_out) - max(lo, so));
}

// out[p][k] = box(P[p], ow, oh) at (tx0 + lane + 64 k, oy), k = 0, 1, for NP planes of one
// w x h geometry (U and V). All waves of the workgroup call this together with the same tx0
// (the barriers); a wave whose row is outside (row_ok false) and lanes whose column is outside
// take part with empty ranges and get 0. cs: this wave's NP x CHUNK column sums.
template <int HBD, int NP>
__device__ __forceinline__ void box_row(const uint8_t *const (&P)[NP], int pitch, int w, int h, int ow, int oh, int tx0,
                                        int oy, bool row_ok, double rcp, double rx, double ry, uint32_t *cs, int lane,
                                        int (&out)[NP][2])
{
    // the tile's source columns, this row's source rows
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
            const int64_t o = (int64_t) sy0 * pitch + (int64_t) sx * (HBD ? 2 : 1);
            int so = sy0 * oh;
#pragma unroll 4
            for (int sy = sy0; sy < sy1; sy++, so += oh) {
                const uint32_t wy = overlap(ylo, h, so, oh);
#pragma unroll
                for (int p = 0; p < NP; p++) add_row<HBD>(P[p] + o + (int64_t) (sy - sy0) * pitch, wy, v[p]);
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
        for (int k = 0; k < 2; k++) out[p][k] = rounded_quot(acc[p][k], den, rcp);
}

// FMT: VP9HIP_OUT_*; HBD: 16-bit source samples.
template <int FMT, int HBD>
__global__ __launch_bounds__(256) void k_convert_scale(const CvtScaleArgs s)
{
    __shared__ __attribute__((aligned(16))) uint32_t colsum[TH][2 * CHUNK];
    const CvtArgs &a = s.c;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tx0 = blockIdx.x * TW, oy = blockIdx.y * TH + wave;
    const uint8_t *src = a.src[blockIdx.z];
    uint8_t *dst = a.dst + (int64_t) blockIdx.z * a.frame_stride;
    uint32_t *cs = colsum[wave];

    int Yk[1][2], UV[2][2] = {};
    const uint8_t *const py[1] = { src + a.src_off[0] }, *const puv[2] = { src + a.src_off[1], src + a.src_off[2] };
    box_row<HBD, 1>(py, a.src_pitch[0], a.w, a.h, s.ow, s.oh, tx0, oy, oy < s.oh, s.rcp[0], s.rx[0], s.ry[0], cs, lane, Yk);
    const bool ctile = tx0 < s.cow;                    // uniform: semi-planar chroma has fewer tiles
    if (ctile)
        box_row<HBD, 2>(puv, a.src_pitch[1], a.cw, a.ch, s.cow, s.coh, tx0, oy, oy < s.coh, s.rcp[1], s.rx[1], s.ry[1], cs, lane, UV);
#pragma unroll
    for (int k = 0; k < 2; k++)
        cvt_store_px<FMT, HBD>(a, dst, tx0 + lane + 64 * k, oy, s.ow, s.oh, s.cow, s.coh, ctile, Yk[0][k], UV[0][k], UV[1][k]);
}

typedef void (*KFn)(const CvtScaleArgs);
// index: format << 1 | hbd
template <size_t... I>
constexpr std::array<KFn, sizeof...(I)> kernel_table(std::index_sequence<I...>)
{
    return { { k_convert_scale<(int) (I >> 1), (int) (I & 1)>... } };
}
const std::array<KFn, 8> g_kernels = kernel_table(std::make_index_sequence<8>());

}  // namespace

hipError_t vp9hip_convert_scale_launch(const CvtScaleArgs &a, int format, int hbd, int n, hipStream_t st)
{
    if (!cvt_launch_ok(format, n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_kernels[format << 1 | !!hbd], cvt_tile_grid(a.ow, a.oh, n), dim3(64 * TH, 1, 1), 0, st, a);
    return hipGetLastError();
}
