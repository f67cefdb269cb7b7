// Fused source rectangle + resize (box or triangle filter) + letterbox + output conversion for
// gfx950: one source rectangle of each frame's planes -> one destination rectangle of an
// out_w x out_h semi-planar, RGB24, planar RGB u8 or planar RGB half frame, the rest of the
// output filled, n frames per launch (blockIdx.z), each with rectangles of its own.
//
// The definitions are those of include/vp9hip.h / DESIGN.md "Resampling: triangle filter,
// source regions, letterbox". For one axis of n_src source samples and n_out output samples:
//   box:       weight(o, s) = the overlap of [o n_src, (o+1) n_src) and [s n_out, (s+1) n_out)
//   triangle:  weight(o, s) = max(0, 2M - |(2o+1) n_src - (2s+1) n_out|),  M = max(n_src, n_out)
//   A(ox, oy) = sum_sy wy sum_sx wx P[sy][sx],  D = Dx(ox) Dy(oy) (the weights' sums),
//   result = (A + (D >> 1)) / D
// all in exact integers, whatever the order. The structure is k_convert_scale's
// (vp9hip_convert_scale.hip): a workgroup owns 128 x 4 output pixels, one output row per wave;
// the wave walks its row's source rows in chunks of 256 source columns, each lane adding
// wy * sample into four column sums over coalesced 4-sample loads; the sums go to LDS once per
// chunk, and each lane adds wx * sum over its two columns' footprints. What differs:
//   - a filter enters in two places only, the footprint [first, last) of an output index and
//     the weight of a (source, output) pair: struct Axis holds both, for both filters;
//   - the geometry is per frame (kernel arguments indexed by blockIdx.z, wave-uniform), so the
//     reciprocals that turn the footprints' divisions into a multiply and a correction are
//     computed here, once per pass, and the divisor Dx Dy is per output sample: each lane sums
//     the weights it applies, takes 1.0 / (Dx Dy) in double for the quotient's estimate (it is
//     below 2^16, the estimate's error below 2^-30) and corrects it by the exact remainder;
//   - the column sums are 64-bit (Dy * sample passes 2^32 from about 1088 rows -> 1 at 12
//     bits) and A approaches 2^63: the host accepts a call only below that bound;
//   - aligned groups of 4 samples may begin left of a source rectangle and end right of it:
//     a lane's horizontal pass runs over its own footprint only, so those samples have no
//     weight, and a group begins below the rectangle's right edge, which is inside the visible
//     width, so it ends inside the 64-padded plane; rows are the rectangle's rows only;
//   - a tile without a pixel of the destination rectangle loads nothing and stores the fill.
// Pixels outside the destination rectangle take the fill codes in place of the resampled
// samples and go through the same conversion, so the fill is the conversion of the codes.
#include "vp9hip_convert_dev.h"

#include <array>
#include <utility>

namespace {

using namespace cvtdev;

// One axis of one plane's geometry: n_src source samples -> n_out output samples. An output
// index o has a key, a source index s a term (both below 2^30); weight(key, term) is the
// integer weight of the pair inside the footprint [first(key), last(key)), where it is > 0.
template <int FILT>
struct Axis {
    int n_src, n_out, two_m, d;
    double rcp;
    __device__ __forceinline__ Axis(int ns, int no)
        : n_src(ns), n_out(no), two_m(2 * max(ns, no)), d(FILT ? 2 * no : no), rcp(1.0 / (double) (FILT ? 2 * no : no)) {}
    __device__ __forceinline__ int key(int o) const { return FILT ? (2 * o + 1) * n_src : o * n_src; }
    __device__ __forceinline__ int term(int s) const { return FILT ? (2 * s + 1) * n_out : s * n_out; }
    __device__ __forceinline__ int step() const { return d; }       // term(s + 1) - term(s)
    __device__ __forceinline__ int first(int k) const
    {
        if constexpr (FILT) {                                       // (2s+1) n_out > key - 2M
            const int t = k - two_m + n_out;
            return t < 0 ? 0 : floordiv(t, d, rcp);
        } else
            return floordiv(k, d, rcp);
    }
    __device__ __forceinline__ int last(int k) const
    {
        if constexpr (FILT) return min(n_src, floordiv(k + two_m + n_out - 1, d, rcp));   // (2s+1) n_out < key + 2M
        else return floordiv(k + n_src + n_out - 1, d, rcp);
    }
    __device__ __forceinline__ uint32_t weight(int k, int t) const
    {
        if constexpr (FILT) return (uint32_t) (two_m - (k < t ? t - k : k - t));
        else return (uint32_t) (min(k + n_src, t + n_out) - max(k, t));
    }
};

// out[p][k] = the output plane's sample at column tx0 + lane + 64 k of row oy, k = 0, 1, for NP
// planes of one geometry (U and V): the resampled rectangle inside the destination rectangle,
// fill[p] outside. All waves of the workgroup call this together with the same tx0 and
// ty0 = the tile's first row (the barriers; the early return is the same for all of them); a
// wave whose row is outside and lanes whose column is outside take part with empty ranges.
// cs: this wave's NP x CHUNK column sums.
template <int FILT, int HBD, int NP>
__device__ __forceinline__ void resample_row(const uint8_t *const (&P)[NP], int pitch, const Geo &g, int tx0, int ty0, int oy,
                                             uint64_t *cs, int lane, const int (&fill)[NP], int (&out)[NP][2])
{
#pragma unroll
    for (int p = 0; p < NP; p++) out[p][0] = out[p][1] = fill[p];
    // the tile's output columns inside the rectangle; none, or no row: the fill alone
    const int oa = max(tx0 - g.dx, 0), ob = min(tx0 + TW - g.dx, g.dw);
    if (oa >= ob || ty0 + TH <= g.dy || ty0 >= g.dy + g.dh) return;
    const Axis<FILT> X(g.w, g.dw), Y(g.h, g.dh);
    // the tile's source columns (absolute), this row's source rows (inside the rectangle)
    const int fx0 = g.x + X.first(X.key(oa)), fx1 = g.x + X.last(X.key(ob - 1));
    const int ry = oy - g.dy;
    const bool row_ok = ry >= 0 && ry < g.dh;
    const int ky = Y.key(row_ok ? ry : 0);
    const int sy0 = row_ok ? Y.first(ky) : 0, sy1 = row_ok ? Y.last(ky) : 0;
    uint32_t dsum_y = 0;
    for (int sy = sy0, t = Y.term(sy0); sy < sy1; sy++, t += Y.step()) dsum_y += Y.weight(ky, t);
    int kx[2], xa[2], xb[2];
    bool ok[2];
    uint32_t dsum_x[2] = {};
    uint64_t acc[NP][2] = {};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int ox = tx0 - g.dx + lane + 64 * k;
        ok[k] = row_ok && ox >= 0 && ox < g.dw;
        kx[k] = X.key(ok[k] ? ox : 0);
        xa[k] = ok[k] ? g.x + X.first(kx[k]) : 0;
        xb[k] = ok[k] ? g.x + X.last(kx[k]) : 0;
    }
    for (int c0 = fx0 & ~3; c0 < fx1; c0 += CHUNK) {
        const int sx = c0 + lane * 4;
        uint64_t v[NP][4] = {};
        if (sx < fx1) {
            const int64_t o = (int64_t) (g.y + sy0) * pitch + (int64_t) sx * (HBD ? 2 : 1);
            int t = Y.term(sy0);
#pragma unroll 4
            for (int sy = sy0; sy < sy1; sy++, t += Y.step()) {
                const uint32_t wy = Y.weight(ky, t);
#pragma unroll
                for (int p = 0; p < NP; p++) add_row<HBD>(P[p] + o + (int64_t) (sy - sy0) * pitch, wy, v[p]);
            }
        }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            ulonglong2 *q = reinterpret_cast<ulonglong2 *>(cs + p * CHUNK + lane * 4);
            q[0] = make_ulonglong2(v[p][0], v[p][1]);
            q[1] = make_ulonglong2(v[p][2], v[p][3]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int s0 = max(xa[k], c0), s1 = min(xb[k], c0 + CHUNK);
            int t = X.term(s0 - g.x);
            for (int s = s0; s < s1; s++, t += X.step()) {
                const uint32_t wx = X.weight(kx[k], t);
                dsum_x[k] += wx;
#pragma unroll
                for (int p = 0; p < NP; p++) acc[p][k] += (uint64_t) wx * cs[p * CHUNK + s - c0];
            }
        }
        __syncthreads();
    }
    // one division per output sample, by the sum of the weights it took
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!ok[k]) continue;
        const uint64_t den = (uint64_t) dsum_x[k] * dsum_y;
        const double rcp = 1.0 / (double) den;
#pragma unroll
        for (int p = 0; p < NP; p++) out[p][k] = rounded_quot(acc[p][k], den, rcp);
    }
}

// FMT: VP9HIP_OUT_*; HBD: 16-bit source samples; FILT: VP9HIP_FILTER_*.
template <int FMT, int HBD, int FILT>
__global__ __launch_bounds__(256) void k_convert_resample(const CvtResampleArgs s)
{
    __shared__ __attribute__((aligned(16))) uint64_t colsum[TH][2 * CHUNK];
    const CvtArgs &a = s.c;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, oy = ty0 + wave;
    const int z = blockIdx.z;
    const uint8_t *src = a.src[z];
    uint8_t *dst = a.dst + (int64_t) z * a.frame_stride;
    uint64_t *cs = colsum[wave];

    Geo gy, gc;
    frame_geo(s, z, gy, gc);
    int Yk[1][2], UV[2][2] = {};
    const uint8_t *const py[1] = { src + a.src_off[0] }, *const puv[2] = { src + a.src_off[1], src + a.src_off[2] };
    const int fy[1] = { s.fill[0] }, fuv[2] = { s.fill[1], s.fill[2] };
    resample_row<FILT, HBD, 1>(py, a.src_pitch[0], gy, tx0, ty0, oy, cs, lane, fy, Yk);
    const bool ctile = tx0 < s.cow;                    // uniform: semi-planar chroma has fewer tiles
    if (ctile) resample_row<FILT, HBD, 2>(puv, a.src_pitch[1], gc, tx0, ty0, oy, cs, lane, fuv, UV);
#pragma unroll
    for (int k = 0; k < 2; k++)
        cvt_store_px<FMT, HBD>(a, dst, tx0 + lane + 64 * k, oy, s.ow, s.oh, s.cow, s.coh, ctile, Yk[0][k], UV[0][k], UV[1][k]);
}

// The graded instantiations (include/vp9hip.h "Graded output"; FMT is an RGB format): the same
// tile with the grade on the stored pixel. A kernel of its own with a second argument, its body
// repeated here: routing both kernels through one inlined function changed k_convert_resample's
// register allocation, and the ungraded instantiations stay instruction for instruction.
template <int FMT, int HBD, int FILT>
__global__ __launch_bounds__(256) void k_convert_resample_graded(const CvtResampleArgs s, const CvtGrade g)
{
    __shared__ __attribute__((aligned(16))) uint64_t colsum[TH][2 * CHUNK];
    const CvtArgs &a = s.c;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, oy = ty0 + wave;
    const int z = blockIdx.z;
    const uint8_t *src = a.src[z];
    uint8_t *dst = a.dst + (int64_t) z * a.frame_stride;
    uint64_t *cs = colsum[wave];

    Geo gy, gc;
    frame_geo(s, z, gy, gc);
    int Yk[1][2], UV[2][2] = {};
    const uint8_t *const py[1] = { src + a.src_off[0] }, *const puv[2] = { src + a.src_off[1], src + a.src_off[2] };
    const int fy[1] = { s.fill[0] }, fuv[2] = { s.fill[1], s.fill[2] };
    resample_row<FILT, HBD, 1>(py, a.src_pitch[0], gy, tx0, ty0, oy, cs, lane, fy, Yk);
    const bool ctile = tx0 < s.cow;                    // uniform: semi-planar chroma has fewer tiles
    if (ctile) resample_row<FILT, HBD, 2>(puv, a.src_pitch[1], gc, tx0, ty0, oy, cs, lane, fuv, UV);
#pragma unroll
    for (int k = 0; k < 2; k++)
        cvt_store_px<FMT, HBD, 1>(a, dst, tx0 + lane + 64 * k, oy, s.ow, s.oh, s.cow, s.coh, ctile, Yk[0][k], UV[0][k], UV[1][k], g);
}

typedef void (*KFn)(const CvtResampleArgs);
// index: format << 2 | hbd << 1 | filter
template <size_t... I>
constexpr std::array<KFn, sizeof...(I)> kernel_table(std::index_sequence<I...>)
{
    return { { k_convert_resample<(int) (I >> 2), (int) (I >> 1 & 1), (int) (I & 1)>... } };
}
const std::array<KFn, 16> g_kernels = kernel_table(std::make_index_sequence<16>());

typedef void (*KGFn)(const CvtResampleArgs, const CvtGrade);
// index: (format - 1) << 2 | hbd << 1 | filter
template <size_t... I>
constexpr std::array<KGFn, sizeof...(I)> graded_table(std::index_sequence<I...>)
{
    return { { k_convert_resample_graded<(int) (I >> 2) + 1, (int) (I >> 1 & 1), (int) (I & 1)>... } };
}
const std::array<KGFn, 12> g_graded = graded_table(std::make_index_sequence<12>());

}  // namespace

hipError_t vp9hip_convert_resample_launch(const CvtResampleArgs &a, int format, int hbd, int filter, int n, hipStream_t st)
{
    if (!cvt_launch_ok(format, n) || filter < 0 || filter > 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_kernels[format << 2 | !!hbd << 1 | filter], cvt_tile_grid(a.ow, a.oh, n), dim3(64 * TH, 1, 1), 0, st, a);
    return hipGetLastError();
}

hipError_t vp9hip_convert_resample_graded_launch(const CvtResampleArgs &a, const CvtGrade &g, int format, int hbd, int filter,
                                                 int n, hipStream_t st)
{
    if (!cvt_launch_ok(format, n) || format == VP9HIP_OUT_SEMIPLANAR || filter < 0 || filter > 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_graded[(format - 1) << 2 | !!hbd << 1 | filter], cvt_tile_grid(a.ow, a.oh, n), dim3(64 * TH, 1, 1), 0, st,
                       a, g);
    return hipGetLastError();
}
