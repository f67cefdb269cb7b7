// Motion tensors at model size for gfx950: the motion field (mv + info) or the accumulated field
// (vp9hip_acc_cell records) of a frame of visible size w x h -> planar P x out_h x out_w, the
// vectors' x and y and optionally the inter coverage, int16 or half, n frames per launch
// (blockIdx.z), reading each cell of the footprint about once and writing only the small output.
// The definition is include/vp9hip.h "motion tensors at model size" / DESIGN.md 17a.
//
// The dense field is constant over a 4 x 4 cell, so the area sum runs over cells with the
// aggregated weight W(o, c) = min((o + 1) n, (4 c + 4) on) - max(o n, 4 c on) inside the
// footprint: the box filter's weights of the cell's four pixel columns (rows) added up, the last
// cell clipped at n on with no special case. As in k_residual_scale the signed mean is taken as
// box(v ^ 0x8000) - 32768: everything is unsigned, a column sum is below h * 65535 < 2^30, the
// quotient below 2^16, and rounded_quot serves as it stands. The coverage (256 has) is unsigned
// to begin with.
//
// The shape is k_convert_scale's / k_residual_scale's over cells instead of samples:
//   - a workgroup owns 128 x 4 outputs, one output row per wave, two columns per lane;
//   - the wave walks the cell rows of its row's footprint in chunks of 128 cell columns, each
//     lane loading two whole cells a row (coded: 16 B of mv and 8 B of info; acc: two 16 B
//     records; coalesced) and adding Wy * value into u32 column sums for x, y and the coverage;
//     Wy is the wave's (the wave index is read as a scalar);
//   - the column sums go to LDS once per chunk, and each lane adds W(ox, c) * sum over the part
//     of its two columns' footprints inside the chunk, in 64 bits;
//   - one rounded_quot per output, then the format's store, only at ox < out_w, oy < out_h.
// A lane's pair of cells starts at an even column below the tile's footprint end, which is at
// most ceil(w / 4) <= GW; GW is even, so no cell at or beyond GW is loaded: in a larger context
// the pitch exceeds GW and what lies there is another frame's or nothing. Rows likewise stay
// below ceil(h / 4) <= GH. Both ends are clamped to the grid once more before any access.
#include "vp9hip_convert_dev.h"
#include "vp9hip_motion_scale.h"

#include <array>
#include <utility>

namespace {

using namespace cvtdev;

constexpr int MCHUNK = 128;            // cell columns per pass: 64 lanes x 2 cells

__device__ __forceinline__ uint32_t overlap(int lo, int n_src, int so, int n_out)
{
    return (uint32_t) (min(lo + n_src, so + n_out) - max(lo, so));
}

// v[p][j] += wy * (plane p of cell j, sign-flipped for x and y), j = 0, 1: the two cells at p0
// (coded: their mv entries, p1 their info dwords; acc: their records)
template <int SRC, int NP>
__device__ __forceinline__ void add_cells(const uint8_t *p0, const uint8_t *p1, uint32_t wy, uint32_t (&v)[NP][2])
{
    uint32_t ux[2], uy[2];
    bool has[2];
    if constexpr (SRC == 0) {
        const uint4 m = *reinterpret_cast<const uint4 *>(p0);      // x0 | y0 << 16, second vector, x1 | y1 << 16, second vector
        const uint2 i = *reinterpret_cast<const uint2 *>(p1);
        const uint32_t w0[2] = { m.x ^ 0x80008000u, m.z ^ 0x80008000u };
        has[0] = (i.x & 0xff) != 255; has[1] = (i.y & 0xff) != 255;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            ux[j] = has[j] ? w0[j] & 0xffff : 0x8000u;
            uy[j] = has[j] ? w0[j] >> 16 : 0x8000u;
        }
    } else {
        const uint4 q[2] = { reinterpret_cast<const uint4 *>(p0)[0], reinterpret_cast<const uint4 *>(p0)[1] };
#pragma unroll
        for (int j = 0; j < 2; j++) {                              // dx, dy, root, hops | end << 16
            has[j] = (q[j].w & 0xffff) != 0;
            ux[j] = has[j] ? (uint32_t) (min(max((int) q[j].x, -32768), 32767) + 32768) : 0x8000u;
            uy[j] = has[j] ? (uint32_t) (min(max((int) q[j].y, -32768), 32767) + 32768) : 0x8000u;
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++) {
        v[0][j] += wy * ux[j];
        v[1][j] += wy * uy[j];
        if constexpr (NP == 3) v[2][j] += has[j] ? wy << 8 : 0u;
    }
}

// SRC: VP9HIP_MVT_CODED / _ACC; FMT: VP9HIP_MVT_I16 / _F16; NP: 2 or 3 planes
template <int SRC, int FMT, int NP>
__global__ __launch_bounds__(256) void k_motion_scale(const MotionScaleArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t colsum[TH][NP * MCHUNK];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tx0 = blockIdx.x * TW, oy = blockIdx.y * TH + wave;
    const uint8_t *src = a.src[blockIdx.z];
    uint8_t *dst = a.dst + (int64_t) blockIdx.z * a.frame_stride;
    uint32_t *cs = colsum[wave];
    const bool row_ok = oy < a.oh;
    const int w = a.w, h = a.h, ow = a.ow, oh = a.oh, ow4 = 4 * ow, oh4 = 4 * oh;
    constexpr int CELL = SRC == 0 ? 8 : 16;                        // bytes of a cell in the plane at src

    // the tile's cell columns and the wave's cell rows (all waves share the columns: the barriers)
    const int fx0 = floordiv(tx0 * w, ow4, a.rx);
    const int fx1 = min(floordiv(min(tx0 + TW, ow) * w + ow4 - 1, ow4, a.rx), a.gw);
    const int ylo = oy * h;
    const int r0 = row_ok ? floordiv(ylo, oh4, a.ry) : 0;
    const int r1 = row_ok ? min(floordiv(ylo + h + oh4 - 1, oh4, a.ry), a.gh) : 0;
    int xlo[2], xa[2], xb[2];
    uint64_t acc[NP][2] = {};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 + lane + 64 * k;
        const bool ok = row_ok && ox < ow;
        xlo[k] = ox * w;
        xa[k] = ok ? floordiv(xlo[k], ow4, a.rx) : 0;
        xb[k] = ok ? min(floordiv(xlo[k] + w + ow4 - 1, ow4, a.rx), a.gw) : 0;
    }
    for (int c0 = fx0 & ~1; c0 < fx1; c0 += MCHUNK) {
        const int cx = c0 + lane * 2;
        uint32_t v[NP][2] = {};
        if (cx < fx1) {
            const uint8_t *p0 = src + ((int64_t) r0 * a.src_pitch + cx) * CELL;
            const uint8_t *p1 = src + a.info_off + ((int64_t) r0 * a.src_pitch + cx) * 4;
            const int64_t s0 = (int64_t) a.src_pitch * CELL, s1 = (int64_t) a.src_pitch * 4;
            int so = r0 * oh4;
#pragma unroll 4
            for (int r = r0; r < r1; r++, so += oh4, p0 += s0, p1 += s1)
                add_cells<SRC, NP>(p0, p1, overlap(ylo, h, so, oh4), v);
        }
#pragma unroll
        for (int p = 0; p < NP; p++) reinterpret_cast<uint2 *>(cs + p * MCHUNK)[lane] = make_uint2(v[p][0], v[p][1]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int s0 = max(xa[k], c0), s1 = min(xb[k], c0 + MCHUNK);
            int so = s0 * ow4;
            for (int s = s0; s < s1; s++, so += ow4) {
                const uint32_t wx = overlap(xlo[k], w, so, ow4);
#pragma unroll
                for (int p = 0; p < NP; p++) acc[p][k] += (uint64_t) wx * cs[p * MCHUNK + s - c0];
            }
        }
        __syncthreads();
    }
    if (!row_ok) return;
    const uint64_t den = (uint64_t) w * (uint64_t) h;
    uint8_t *row = dst + (int64_t) oy * a.pitch;
    const int64_t pl = a.plane / 2;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 + lane + 64 * k;
        if (ox >= ow) continue;
        int o[NP];
        o[0] = rounded_quot(acc[0][k], den, a.rcp) - 32768;
        o[1] = rounded_quot(acc[1][k], den, a.rcp) - 32768;
        if constexpr (NP == 3) o[2] = rounded_quot(acc[2][k], den, a.rcp);
        if constexpr (FMT == 1) {                                  // half: one float multiply, round to nearest even
            _Float16 *p = reinterpret_cast<_Float16 *>(row) + ox;
            p[0] = to_half(o[0], a.kx); p[pl] = to_half(o[1], a.ky);
            if constexpr (NP == 3) p[2 * pl] = to_half(o[2], 1.0f / 256);
        } else {
            int16_t *p = reinterpret_cast<int16_t *>(row) + ox;
            p[0] = (int16_t) o[0]; p[pl] = (int16_t) o[1];
            if constexpr (NP == 3) p[2 * pl] = (int16_t) o[2];
        }
    }
}

typedef void (*KFn)(const MotionScaleArgs);
// index: source * 4 + format * 2 + (planes - 2)
template <size_t... I>
constexpr std::array<KFn, sizeof...(I)> kernel_table(std::index_sequence<I...>)
{
    return { { k_motion_scale<(int) (I >> 2), (int) (I >> 1 & 1), 2 + (int) (I & 1)>... } };
}
const std::array<KFn, 8> g_kernels = kernel_table(std::make_index_sequence<8>());

}  // namespace

hipError_t vp9hip_motion_scale_launch(const MotionScaleArgs &a, int source, int format, int planes, int n, hipStream_t st)
{
    if (source < 0 || source > 1 || format < 0 || format > 1 || planes < 2 || planes > 3 || n < 1 || n > MSC_MAX_FRAMES)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_kernels[source * 4 + format * 2 + planes - 2], cvt_tile_grid(a.ow, a.oh, n), dim3(64 * TH, 1, 1), 0, st, a);
    return hipGetLastError();
}
