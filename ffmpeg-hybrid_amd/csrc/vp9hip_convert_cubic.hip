// Fused source rectangle + bicubic resize + letterbox + output conversion for gfx950: the frame
// of k_convert_resample (vp9hip_convert_resample.hip) with the Keys cubic (a = -1/2), widened
// when downscaling, as the filter. One source rectangle of each frame's planes -> one
// destination rectangle of an out_w x out_h semi-planar, RGB24, planar RGB u8 or planar RGB
// half frame, the rest of the output filled, n frames per launch (blockIdx.z), each with
// rectangles of its own.
//
// The definition is that of include/vp9hip.h / DESIGN.md "Resampling: bicubic". For one axis of
// n_src source samples and n_out output samples, M = max(n_src, n_out), T = 2M, Q = 14:
//   u = |(2o+1) n_src - (2s+1) n_out|, present iff u < 2T
//   c(u) = 3u^3 - 5T u^2 + 2T^3 (u < T),  -u^3 + 5T u^2 - 8T^2 u + 4T^3 (T <= u < 2T)
//   q(o, s) = floor((c(u) 2^Q + T^3) / (2T^3)),  D(o) = sum_s q(o, s)
//   A(ox, oy) = sum_sy qy sum_sx qx P[sy][sx],  result = clip(floor((A + (D >> 1)) / D), 0, 2^bpp - 1)
// with D = Dx(ox) Dy(oy), all in exact signed integers, whatever the order. A workgroup owns
// 128 x 4 output pixels, one output row per wave; the wave walks its row's source rows in
// chunks of 256 source columns, each lane adding qy * sample into four signed 64-bit column
// sums over coalesced 4-sample loads; the sums go to LDS once per chunk, and each lane adds
// qx * sum over its two columns' footprints. What differs from the triangle:
//   - a weight is a 64-bit cubic and a division, so it is never evaluated where it is applied.
//     The row's qy (wave-uniform) are built once by the wave's 64 lanes into an LDS table of
//     QCAP entries and read back by every lane, for every chunk and plane of the geometry; a
//     row with more taps than QCAP (ratios past QCAP / 4) rebuilds the table per block of QCAP
//     source rows inside each chunk: smaller blocks, never a refusal.
//   - the tile's qx are built per chunk by the whole workgroup into a table of 4 * CHUNK
//     entries that serves all four waves and both planes of the geometry. It always fits: when
//     n_src >= n_out a source sample is a tap of at most 4 consecutive outputs (o in an open
//     interval of length 4), so the entry of (s, o) is [s - c0][o & 3], built one source column
//     per thread; when n_src < n_out an output has at most 4 consecutive taps, so the entry
//     is [column][s & 3], built one output column per thread. Either way a thread evaluates
//     at most 4 of 5 candidates around the nearest index;
//   - the sums are signed, A + (D >> 1) may be negative (the result is then 0), the quotient may
//     pass the largest code (it is then that): one exact floor division and one clip per output
//     sample, the quotient estimated in double and corrected by the exact 64-bit remainder;
//   - footprints are twice the triangle's: 2 max(1, n_src / n_out) samples on each side.
// |A| stays below 2^62: the host accepts a call only below that bound. Loads stay inside the
// 64-padded plane as in k_convert_resample: a group of 4 samples begins below the rectangle's
// right edge, rows are the rectangle's rows only. A tile without a pixel of the destination
// rectangle loads nothing and stores the fill. Pixels outside the destination rectangle take
// the fill codes in place of the resampled samples and go through the same conversion.
#include "vp9hip_convert_dev.h"

#include <array>
#include <utility>

namespace {

using namespace cvtdev;

constexpr int QCAP = 512;              // a wave's qy table: source rows per block
constexpr int QBITS = 14;              // Q

// LDS writes of a wave's lanes before, reads by its other lanes after: a wave's LDS operations
// complete in order, so only the compiler has to keep them in place.
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Keeps a wave-uniform value in vector registers: the reciprocals and T^3 only ever feed vector
// instructions (doubles, 64-bit products), and the scalar file is what this kernel runs out of.
template <class V>
__device__ __forceinline__ V in_vgpr(V x)
{
    asm volatile("" : "+v"(x));
    return x;
}

// One axis of one plane's geometry: n_src source samples -> n_out output samples. An output
// index o has a key, a source index s a term (both below 2^30); the pair's tap is present
// inside the footprint [first(key), last(key)), where u = |key - term| < 2T, and weighs q(u).
struct Axis {
    int n_src, n_out, t;
    int64_t t3;
    double rcp, rcp_den;                               // 1 / (2 n_out), 1 / (2 T^3)
    __device__ __forceinline__ Axis(int ns, int no)
        : n_src(ns), n_out(no), t(2 * max(ns, no)), t3(in_vgpr((int64_t) t * t * t)), rcp(in_vgpr(1.0 / (double) (2 * no))),
          rcp_den(in_vgpr(1.0 / (double) (2 * t3))) {}
    __device__ __forceinline__ int key(int o) const { return (2 * o + 1) * n_src; }
    __device__ __forceinline__ int term(int s) const { return (2 * s + 1) * n_out; }
    __device__ __forceinline__ int first(int k) const              // (2s+1) n_out > key - 2T
    {
        const int x = k - 2 * t + n_out;
        return x < 0 ? 0 : floordiv(x, 2 * n_out, rcp);
    }
    __device__ __forceinline__ int last(int k) const               // (2s+1) n_out < key + 2T
    {
        return min(n_src, floordiv(k + 2 * t + n_out - 1, 2 * n_out, rcp));
    }
    // the output index nearest a source sample's centre, and the reverse
    __device__ __forceinline__ int near_out(int term_s) const { return floordiv(term_s, 2 * n_src, 1.0 / (double) (2 * n_src)); }
    __device__ __forceinline__ int near_src(int key_o) const { return floordiv(key_o, 2 * n_out, rcp); }
    // q for 0 <= u < 2T: |c| < 2^52, |c 2^Q + T^3| < 2^61, the quotient's magnitude below 2^15,
    // so the double estimate is within one of it and the exact remainder corrects it
    __device__ __forceinline__ int q(int u) const
    {
        const int64_t U = u, T = t;
        const int64_t c = u < t ? U * U * (3 * U - 5 * T) + 2 * t3 : ((5 * T - U) * U - 8 * T * T) * U + 4 * t3;
        const int64_t num = c * (1 << QBITS) + t3, den = 2 * t3;
        int64_t e = (int64_t) __builtin_floor((double) num * rcp_den);
        const int64_t r = num - e * den;
        if (r < 0) e--;
        else if (r >= den) e++;
        return (int) e;
    }
    __device__ __forceinline__ int weight(int k, int x) const { return q(k < x ? x - k : k - x); }
};

// The workgroup's LDS: every wave's column sums (two planes), the tile's qx for one chunk, every
// wave's qy for one block of source rows.
struct __attribute__((aligned(16))) Lds {
    int64_t colsum[TH][2 * CHUNK];
    int32_t qx[4 * CHUNK];
    int32_t qy[TH][QCAP];
};

// out[p][k] = the output plane's sample at column tx0 + lane + 64 k of row oy, k = 0, 1, for NP
// planes of one geometry (U and V): the resampled rectangle inside the destination rectangle,
// fill[p] outside. All waves of the workgroup call this together with the same tx0 and
// ty0 = the tile's first row (the barriers; the early return is the same for all of them); a
// wave whose row is outside and lanes whose column is outside take part with empty ranges.
template <int HBD, int NP>
__device__ __forceinline__ void resample_row(const uint8_t *const (&P)[NP], int pitch, const Geo &g, int tx0, int ty0, int oy,
                                             Lds &L, int wave, int lane, const int (&fill)[NP], int smax, int (&out)[NP][2])
{
#pragma unroll
    for (int p = 0; p < NP; p++) out[p][0] = out[p][1] = fill[p];
    // the tile's output columns inside the rectangle; none, or no row: the fill alone
    const int oa = max(tx0 - g.dx, 0), ob = min(tx0 + TW - g.dx, g.dw);
    if (oa >= ob || ty0 + TH <= g.dy || ty0 >= g.dy + g.dh) return;
    const Axis X(g.w, g.dw), Y(g.h, g.dh);
    const int tid = wave * 64 + lane;
    int64_t *cs = L.colsum[wave];
    int32_t *qyt = L.qy[wave];
    // the tile's source columns (absolute), this row's source rows (inside the rectangle)
    const int fx0 = g.x + X.first(X.key(oa)), fx1 = g.x + X.last(X.key(ob - 1));
    const int ry = oy - g.dy;
    const bool row_ok = ry >= 0 && ry < g.dh;
    const int ky = Y.key(row_ok ? ry : 0);
    const int sy0 = row_ok ? Y.first(ky) : 0, sy1 = row_ok ? Y.last(ky) : 0;
    // the row's qy, 64 at a time, and their sum; the table holds them all if they fit
    const int ny = sy1 - sy0;
    const bool once = ny <= QCAP;
    int dsum_y = 0;
    for (int i = lane; i < ny; i += 64) {
        const int q = Y.weight(ky, Y.term(sy0 + i));
        dsum_y += q;
        if (once) qyt[i] = q;
    }
#pragma unroll
    for (int m = 32; m; m >>= 1) dsum_y += __shfl_xor(dsum_y, m);
    wave_sync();
    const bool down = g.w >= g.dw;                     // uniform: how the qx table is indexed
    int ox[2], kx[2], xa[2], xb[2];
    bool ok[2];
    int dsum_x[2] = {};
    int64_t acc[NP][2] = {};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        ox[k] = tx0 - g.dx + lane + 64 * k;
        ok[k] = row_ok && ox[k] >= 0 && ox[k] < g.dw;
        kx[k] = X.key(ok[k] ? ox[k] : 0);
        xa[k] = ok[k] ? g.x + X.first(kx[k]) : 0;
        xb[k] = ok[k] ? g.x + X.last(kx[k]) : 0;
    }
    for (int c0 = fx0 & ~3; c0 < fx1; c0 += CHUNK) {
        // the tile's qx over this chunk: at most 4 of the 5 candidates are present
        if (down) {
            const int s = c0 + tid - g.x;
            if (s >= 0 && s < g.w && c0 + tid < fx1) {
                const int x = X.term(s), oc = X.near_out(x);
#pragma unroll
                for (int j = -2; j <= 2; j++) {
                    const int o = oc + j;
                    if (o < 0 || o >= g.dw) continue;
                    const int k = X.key(o), u = k < x ? x - k : k - x;
                    if (u < 2 * X.t) L.qx[tid * 4 + (o & 3)] = X.q(u);
                }
            }
        } else if (tid < TW) {
            const int o = tx0 - g.dx + tid;
            if (o >= 0 && o < g.dw) {
                const int k = X.key(o), sc = X.near_src(k);
#pragma unroll
                for (int j = -2; j <= 2; j++) {
                    const int s = sc + j;
                    if (s < 0 || s >= g.w) continue;
                    const int x = X.term(s), u = k < x ? x - k : k - x;
                    if (u < 2 * X.t) L.qx[tid * 4 + (s & 3)] = X.q(u);
                }
            }
        }
        const int sx = c0 + lane * 4;
        int64_t v[NP][4] = {};
        for (int r0 = 0; r0 < ny; r0 += QCAP) {
            const int nb = min(QCAP, ny - r0);
            if (!once) {                               // this block's qy in place of the last one's
                wave_sync();
                for (int i = lane; i < nb; i += 64) qyt[i] = Y.weight(ky, Y.term(sy0 + r0 + i));
                wave_sync();
            }
            if (sx < fx1) {
                const int64_t o = (int64_t) (g.y + sy0 + r0) * pitch + (int64_t) sx * (HBD ? 2 : 1);
#pragma unroll 4
                for (int i = 0; i < nb; i++) {
                    const int32_t wy = qyt[i];
#pragma unroll
                    for (int p = 0; p < NP; p++) add_row<HBD>(P[p] + o + (int64_t) i * pitch, wy, v[p]);
                }
            }
        }
#pragma unroll
        for (int p = 0; p < NP; p++) {
            longlong2 *q = reinterpret_cast<longlong2 *>(cs + p * CHUNK + lane * 4);
            q[0] = make_longlong2(v[p][0], v[p][1]);
            q[1] = make_longlong2(v[p][2], v[p][3]);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int s0 = max(xa[k], c0), s1 = min(xb[k], c0 + CHUNK);
            for (int s = s0; s < s1; s++) {
                const int wx = L.qx[down ? (s - c0) * 4 + (ox[k] & 3) : (lane + 64 * k) * 4 + ((s - g.x) & 3)];
                dsum_x[k] += wx;
#pragma unroll
                for (int p = 0; p < NP; p++) acc[p][k] += (int64_t) wx * cs[p * CHUNK + s - c0];
            }
        }
        __syncthreads();
    }
    // one floor division and one clip per output sample. Below 0: 0. Otherwise the double
    // estimate of the quotient is within one of it while it is below 2^16 (past that the result
    // is the largest code anyway), and the exact remainder (|r| < 2 den < 2^63) corrects it.
#pragma unroll
    for (int k = 0; k < 2; k++) {
        if (!ok[k]) continue;
        const int64_t den = (int64_t) dsum_x[k] * dsum_y;
        const double rcp = 1.0 / (double) den;
#pragma unroll
        for (int p = 0; p < NP; p++) {
            const int64_t A = acc[p][k] + (den >> 1);
            const double e = (double) A * rcp;
            int r;
            if (A < 0) r = 0;
            else if (e >= 65536.0) r = smax;
            else {
                int64_t q = (int64_t) e;
                const int64_t rem = A - q * den;
                if (rem < 0) q--;
                else if (rem >= den) q++;
                r = min((int) q, smax);
            }
            out[p][k] = r;
        }
    }
}

// FMT: VP9HIP_OUT_*; HBD: 16-bit source samples.
template <int FMT, int HBD>
__global__ __launch_bounds__(256) void k_convert_cubic(const CvtCubicArgs ca)
{
    __shared__ Lds L;
    const CvtResampleArgs &s = ca.r;
    const CvtArgs &a = s.c;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, oy = ty0 + wave;
    const int z = blockIdx.z;
    const uint8_t *src = a.src[z];
    uint8_t *dst = a.dst + (int64_t) z * a.frame_stride;

    Geo gy, gc;
    frame_geo(s, z, gy, gc);
    int Yk[1][2], UV[2][2] = {};
    const uint8_t *const py[1] = { src + a.src_off[0] }, *const puv[2] = { src + a.src_off[1], src + a.src_off[2] };
    const int fy[1] = { s.fill[0] }, fuv[2] = { s.fill[1], s.fill[2] };
    resample_row<HBD, 1>(py, a.src_pitch[0], gy, tx0, ty0, oy, L, wave, lane, fy, ca.smax, Yk);
    const bool ctile = tx0 < s.cow;                    // uniform: semi-planar chroma has fewer tiles
    if (ctile) resample_row<HBD, 2>(puv, a.src_pitch[1], gc, tx0, ty0, oy, L, wave, lane, fuv, ca.smax, UV);
#pragma unroll
    for (int k = 0; k < 2; k++)
        cvt_store_px<FMT, HBD>(a, dst, tx0 + lane + 64 * k, oy, s.ow, s.oh, s.cow, s.coh, ctile, Yk[0][k], UV[0][k], UV[1][k]);
}

// The graded instantiations (include/vp9hip.h "Graded output"; FMT is an RGB format): the same
// tile with the grade on the stored pixel. A kernel of its own with a second argument, its body
// repeated here: routing both kernels through one inlined function changed k_convert_cubic's
// register allocation, and the ungraded instantiations stay instruction for instruction.
template <int FMT, int HBD>
__global__ __launch_bounds__(256) void k_convert_cubic_graded(const CvtCubicArgs ca, const CvtGrade g)
{
    __shared__ Lds L;
    const CvtResampleArgs &s = ca.r;
    const CvtArgs &a = s.c;
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tx0 = blockIdx.x * TW, ty0 = blockIdx.y * TH, oy = ty0 + wave;
    const int z = blockIdx.z;
    const uint8_t *src = a.src[z];
    uint8_t *dst = a.dst + (int64_t) z * a.frame_stride;

    Geo gy, gc;
    frame_geo(s, z, gy, gc);
    int Yk[1][2], UV[2][2] = {};
    const uint8_t *const py[1] = { src + a.src_off[0] }, *const puv[2] = { src + a.src_off[1], src + a.src_off[2] };
    const int fy[1] = { s.fill[0] }, fuv[2] = { s.fill[1], s.fill[2] };
    resample_row<HBD, 1>(py, a.src_pitch[0], gy, tx0, ty0, oy, L, wave, lane, fy, ca.smax, Yk);
    const bool ctile = tx0 < s.cow;                    // uniform: semi-planar chroma has fewer tiles
    if (ctile) resample_row<HBD, 2>(puv, a.src_pitch[1], gc, tx0, ty0, oy, L, wave, lane, fuv, ca.smax, UV);
#pragma unroll
    for (int k = 0; k < 2; k++)
        cvt_store_px<FMT, HBD, 1>(a, dst, tx0 + lane + 64 * k, oy, s.ow, s.oh, s.cow, s.coh, ctile, Yk[0][k], UV[0][k], UV[1][k], g);
}

typedef void (*KFn)(const CvtCubicArgs);
// index: format << 1 | hbd
template <size_t... I>
constexpr std::array<KFn, sizeof...(I)> kernel_table(std::index_sequence<I...>)
{
    return { { k_convert_cubic<(int) (I >> 1), (int) (I & 1)>... } };
}
const std::array<KFn, 8> g_kernels = kernel_table(std::make_index_sequence<8>());

typedef void (*KGFn)(const CvtCubicArgs, const CvtGrade);
// index: (format - 1) << 1 | hbd
template <size_t... I>
constexpr std::array<KGFn, sizeof...(I)> graded_table(std::index_sequence<I...>)
{
    return { { k_convert_cubic_graded<(int) (I >> 1) + 1, (int) (I & 1)>... } };
}
const std::array<KGFn, 6> g_graded = graded_table(std::make_index_sequence<6>());

}  // namespace

hipError_t vp9hip_convert_cubic_launch(const CvtCubicArgs &a, int format, int hbd, int n, hipStream_t st)
{
    if (!cvt_launch_ok(format, n)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_kernels[format << 1 | !!hbd], cvt_tile_grid(a.r.ow, a.r.oh, n), dim3(64 * TH, 1, 1), 0, st, a);
    return hipGetLastError();
}

hipError_t vp9hip_convert_cubic_graded_launch(const CvtCubicArgs &a, const CvtGrade &g, int format, int hbd, int n, hipStream_t st)
{
    if (!cvt_launch_ok(format, n) || format == VP9HIP_OUT_SEMIPLANAR) return hipErrorInvalidValue;
    hipLaunchKernelGGL(g_graded[(format - 1) << 1 | !!hbd], cvt_tile_grid(a.r.ow, a.r.oh, n), dim3(64 * TH, 1, 1), 0, st, a, g);
    return hipGetLastError();
}
