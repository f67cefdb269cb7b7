// Frame metrics for gfx950: k_metrics reads n pairs of device frames once and leaves, per plane
// of each pair, the eight exact sums of include/vp9hip.h ("frame metrics") and, for luma, the
// SAD of every 16x16 cell. A pure streaming read of 2 x the visible bytes.
//
// Work distribution: a frame is cut into strips of MET_TW x th luma samples (th = 32, 64 or 128,
// chosen by the launcher) and the co-located chroma; the 256-thread workgroups of a pair
// (blockIdx.z) share its strips round robin, strip s, s + gridDim.x, ... A plane's part of a
// strip is cut into blocks of 64 columns x 16 rows; a wave takes blocks w, w + 4, ..., and inside
// a block lane l reads the 16 samples at column 16 (l & 3) of row l >> 2: one 16-byte load at 8
// bits, two above. So a wave owns four whole 16x16 cells of a luma block and sums a cell with
// four shuffles: the map is written with plain stores, each cell by exactly one wave, and needs
// no initialisation.
//
// Bounds: a lane loads only where x < visible width and y < visible height of the plane. x is a
// multiple of 16 and the planes' pitches are multiples of 32 samples (64 for luma) that cover
// the configured width, so the 16 samples from x lie inside the row; the tail samples past the
// visible width are masked to zero in a and b alike, which takes them out of every sum.
//
// Accumulators. A plane's part of a strip is at most (MET_TW / 64) (128 / 16) = 32 blocks, 8 for
// each wave, so a lane sees at most 8 x 16 = 128 samples of a plane and strip, and a workgroup
// takes at most MET_MAX_STRIPS = 256 strips (the launcher sizes the grid for it): 2^15 samples.
//   sum a, sum b, sad:  2^15 * 65535 < 2^31                     u32
//   ndiff:              two u16 halves, 2^14 each               packed u32
//   maxdiff:            two u16 halves                          packed u32
//   first:              y * plane width + x < 2^28              u32, all ones = none
//   sum a^2, sse:       8 bits: 2^15 * 255^2 < 2^31             u32
//                       16 bits: 65535^2 alone is 2^32 - 2^17 + 1, two overflow: u64 from the first sample
// The sums are widened to u64 before the wave adds them up. Each workgroup adds its totals to the
// pair's record with 64-bit atomics, all of a pair's to the same two cache lines: they
// serialise, so the launcher gives a pair no more workgroups than
// its share of MET_FILL and each workgroup several strips instead. FIRST is an
// unsigned minimum, so the all-ones it starts from is already the -1 of "none". Integer sums
// commute: the result does not depend on the schedule.
#include <algorithm>
#include <type_traits>

#include "vp9hip_metrics.h"

namespace {

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(uint32_t v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ uint32_t as_u32(us2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ us2 pk_absdiff(us2 a, us2 b)
{
    return __builtin_elementwise_max(a, b) - __builtin_elementwise_min(a, b);
}

#define MET_NONE 0xffffffffu

template <typename T> struct MetAcc {
    // the sums of squares: u32 is enough for 8-bit codes, see above
    typedef typename std::conditional<sizeof(T) == 1, uint32_t, uint64_t>::type Wide;
    uint32_t sa = 0, sb = 0, sad = 0, seg = 0, first = MET_NONE;
    us2 nd = { 0, 0 }, mx = { 0, 0 };
    Wide sq = 0, sse = 0;
};

// One dword of a and of b: four 8-bit samples
template <bool HASB>
__device__ __forceinline__ void met_dword(MetAcc<uint8_t> &A, const uint32_t ua, const uint32_t ub)
{
    A.sa = __builtin_amdgcn_sad_u8(ua, 0u, A.sa);
    A.sq = __builtin_amdgcn_udot4(ua, ua, A.sq, false);
    if (HASB) {
        A.sb = __builtin_amdgcn_sad_u8(ub, 0u, A.sb);
        A.seg = __builtin_amdgcn_sad_u8(ua, ub, A.seg);
        // |a - b| of the even and the odd bytes, in 16-bit halves
        const us2 de = pk_absdiff(as_us2(ua & 0x00ff00ffu), as_us2(ub & 0x00ff00ffu));
        const us2 dd = pk_absdiff(as_us2((ua >> 8) & 0x00ff00ffu), as_us2((ub >> 8) & 0x00ff00ffu));
        const us2 one = { 1, 1 };
        A.mx = __builtin_elementwise_max(A.mx, __builtin_elementwise_max(de, dd));
        A.nd += __builtin_elementwise_min(de, one) + __builtin_elementwise_min(dd, one);
        A.sse = __builtin_amdgcn_udot2(de, de, A.sse, false);
        A.sse = __builtin_amdgcn_udot2(dd, dd, A.sse, false);
    }
}

// One dword of a and of b: two 16-bit samples
template <bool HASB>
__device__ __forceinline__ void met_dword(MetAcc<uint16_t> &A, const uint32_t ua, const uint32_t ub)
{
    const us2 one = { 1, 1 };
    A.sa = __builtin_amdgcn_udot2(as_us2(ua), one, A.sa, false);
    A.sq += (uint64_t) (ua & 0xffffu) * (ua & 0xffffu);
    A.sq += (uint64_t) (ua >> 16) * (ua >> 16);
    if (HASB) {
        A.sb = __builtin_amdgcn_udot2(as_us2(ub), one, A.sb, false);
        const us2 d = pk_absdiff(as_us2(ua), as_us2(ub));
        const uint32_t ud = as_u32(d);
        A.seg = __builtin_amdgcn_udot2(d, one, A.seg, false);
        A.mx = __builtin_elementwise_max(A.mx, d);
        A.nd += __builtin_elementwise_min(d, one);
        A.sse += (uint64_t) (ud & 0xffffu) * (ud & 0xffffu);
        A.sse += (uint64_t) (ud >> 16) * (ud >> 16);
    }
}

// The partial sums of the four waves: [plane][wave][field]
struct MetLds {
    unsigned long long part[3][MET_WG / 64][VP9HIP_METRIC_FIELDS];
};

// A wave's reduction with DPP moves (VALU, no LDS traffic): an inclusive scan of each row of 16
// lanes (row_shr 1, 2, 4, 8), then row 0's total into row 1 and row 2's into row 3
// (row_bcast:15, rows 1 and 3), then lane 31's into rows 2 and 3 (row_bcast:31). A lane without
// a source, or outside the row mask, receives the identity. Lane 63 ends with the wave's total;
// the other lanes hold partial scans. Called with the whole wave active.
struct MetAdd { static constexpr uint32_t idn = 0u; template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a + b; } };
struct MetMax { static constexpr uint32_t idn = 0u; template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a > b ? a : b; } };
struct MetMin { static constexpr uint32_t idn = ~0u; template <typename T> static __device__ __forceinline__ T f(T a, T b) { return a < b ? a : b; } };

template <int CTRL, int ROWS> __device__ __forceinline__ uint32_t met_dpp(const uint32_t idn, const uint32_t v)
{
    return (uint32_t) __builtin_amdgcn_update_dpp((int) idn, (int) v, CTRL, ROWS, 0xf, false);
}
template <int CTRL, int ROWS> __device__ __forceinline__ uint64_t met_dpp(const uint32_t idn, const uint64_t v)
{
    return (uint64_t) met_dpp<CTRL, ROWS>(idn, (uint32_t) (v >> 32)) << 32 | met_dpp<CTRL, ROWS>(idn, (uint32_t) v);
}
template <class Op, typename T> __device__ __forceinline__ T wave_red(T v)
{
    v = Op::f(v, met_dpp<0x111, 0xf>(Op::idn, v));          // row_shr:1
    v = Op::f(v, met_dpp<0x112, 0xf>(Op::idn, v));          // row_shr:2
    v = Op::f(v, met_dpp<0x114, 0xf>(Op::idn, v));          // row_shr:4
    v = Op::f(v, met_dpp<0x118, 0xf>(Op::idn, v));          // row_shr:8
    v = Op::f(v, met_dpp<0x142, 0xa>(Op::idn, v));          // row_bcast:15 into rows 1, 3
    v = Op::f(v, met_dpp<0x143, 0xc>(Op::idn, v));          // row_bcast:31 into rows 2, 3
    return v;
}

// One block of a plane: 64 columns x 16 rows from (bx, by), lane l the 16 samples at column
// 16 (l & 3) of row l >> 2, into the lane's accumulators; a luma block's four cells into the map.
template <typename T, bool HASB, bool CELLS>
__device__ __forceinline__ void met_block(MetAcc<T> &A, const MetArgs &g, const uint32_t z, const bool luma,
                                          const uint8_t *const pa, const uint8_t *const pb, const size_t pitch,
                                          const uint32_t vw, const uint32_t vh, const uint32_t bx, const uint32_t by,
                                          const uint32_t lane)
{
    constexpr int NDW = 4 * (int) sizeof(T);               // dwords of a lane's 16 samples
    constexpr int SPD = 4 / (int) sizeof(T);               // samples per dword
    const uint32_t lx = 16 * (lane & 3), ly = lane >> 2;
    const uint32_t x = bx + lx, y = by + ly;
    A.seg = 0;
    if (x < vw && y < vh) {
        const size_t at = (size_t) y * pitch + (size_t) x * sizeof(T);
        uint32_t ua[NDW], ub[NDW];
#pragma unroll
        for (int q = 0; q < NDW / 4; q++) {
            const uint4 v = ((const uint4 *) (pa + at))[q];
            ua[4 * q] = v.x; ua[4 * q + 1] = v.y; ua[4 * q + 2] = v.z; ua[4 * q + 3] = v.w;
        }
#pragma unroll
        for (int q = 0; q < NDW / 4; q++) {
            uint4 v = make_uint4(0, 0, 0, 0);
            if (HASB) v = ((const uint4 *) (pb + at))[q];
            ub[4 * q] = v.x; ub[4 * q + 1] = v.y; ub[4 * q + 2] = v.z; ub[4 * q + 3] = v.w;
        }
        const uint32_t keep = vw - x;                   // visible samples from x on, >= 1
        if (keep < 16) {
#pragma unroll
            for (int d = 0; d < NDW; d++) {
                const uint32_t kd = keep > (uint32_t) (SPD * d) ? keep - SPD * d : 0u;   // of this dword
                const uint32_t m = kd >= (uint32_t) SPD ? ~0u : (1u << (kd * (32 / SPD))) - 1u;
                ua[d] &= m; ub[d] &= m;
            }
        }
#pragma unroll
        for (int d = 0; d < NDW; d++) met_dword<HASB>(A, ua[d], ub[d]);
        if (HASB && A.seg && y * vw + x < A.first) {
            // the segment's first differing sample, if the segment starts below the lane's first so far
            uint32_t j = MET_NONE;
#pragma unroll
            for (int d = 0; d < NDW; d++) {
                const uint32_t bit = (uint32_t) (__ffs((int) (ua[d] ^ ub[d])) - 1);   // all ones: equal
                const uint32_t smp = (bit >> (sizeof(T) == 1 ? 3 : 4)) + SPD * d;
                j = smp < j ? smp : j;
            }
            j += y * vw + x;
            A.first = j < A.first ? j : A.first;
        }
        A.sad += A.seg;
    }
    if (CELLS && luma) {
        // the block's four cells: the 16 rows of a cell column are lanes 4 apart
        uint32_t c = A.seg;
        c += __shfl_xor(c, 4, 64);
        c += __shfl_xor(c, 8, 64);
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        const uint32_t cx = (bx >> 4) + lane, cy = by >> 4;
        if (lane < 4 && cx < (uint32_t) g.mw && cy < (uint32_t) g.mh)
            g.cells[((size_t) z * g.mh + cy) * g.mw + cx] = (int32_t) c;
    }
}

template <typename T, bool HASB, bool CELLS>
__global__ __launch_bounds__(MET_WG) void k_metrics(const MetArgs g)
{
    __shared__ MetLds S;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t z = blockIdx.z;
    const uint8_t *const fa = g.a[z], *const fb = HASB ? g.b[z] : nullptr;

#pragma unroll 1
    for (int p = 0; p < 3; p++) {
        const uint32_t sh = p ? g.ss_h : 0, sv = p ? g.ss_v : 0;
        const uint32_t vw = p ? g.cw : g.w, vh = p ? g.ch : g.h;
        const uint32_t bw = (MET_TW / 64) >> sh, nblk = bw * (((uint32_t) g.th / 16) >> sv);
        const size_t pitch = (size_t) g.pitch[p ? 1 : 0];
        const uint8_t *const pa = fa + g.off[p], *const pb = HASB ? fb + g.off[p] : nullptr;
        MetAcc<T> A;
        for (uint32_t s = blockIdx.x; s < (uint32_t) g.nstrips; s += gridDim.x) {
            const uint32_t x0 = (s % (uint32_t) g.nsx) * (MET_TW >> sh), y0 = (s / (uint32_t) g.nsx) * ((uint32_t) g.th >> sv);
            for (uint32_t k = wave; k < nblk; k += MET_WG / 64)
                met_block<T, HASB, CELLS>(A, g, z, p == 0, pa, pb, pitch, vw, vh, x0 + 64 * (k % bw), y0 + 16 * (k / bw), lane);
        }
        // per wave, then per workgroup below
        const uint64_t sa = wave_red<MetAdd>((uint64_t) A.sa);
        const uint64_t sq = wave_red<MetAdd>((uint64_t) A.sq);
        uint64_t sb = 0, sad = 0, sse = 0;
        uint32_t nd = 0, mx = 0, first = MET_NONE;
        if (HASB) {
            sb = wave_red<MetAdd>((uint64_t) A.sb);
            sad = wave_red<MetAdd>((uint64_t) A.sad);
            sse = wave_red<MetAdd>((uint64_t) A.sse);
            nd = wave_red<MetAdd>((uint32_t) A.nd.x + A.nd.y);
            mx = wave_red<MetMax>((uint32_t) (A.mx.x > A.mx.y ? A.mx.x : A.mx.y));
            first = wave_red<MetMin>(A.first);
        }
        if (lane == 63) {                                       // the lane that holds the wave's totals
            unsigned long long *r = S.part[p][wave];
            r[VP9HIP_METRIC_SUM_A] = sa; r[VP9HIP_METRIC_SUM_B] = sb; r[VP9HIP_METRIC_SUMSQ_A] = sq;
            r[VP9HIP_METRIC_SAD] = sad; r[VP9HIP_METRIC_SSE] = sse; r[VP9HIP_METRIC_NDIFF] = nd;
            r[VP9HIP_METRIC_MAXDIFF] = mx;
            r[VP9HIP_METRIC_FIRST] = first == MET_NONE ? ~0ull : (unsigned long long) first;
        }
    }
    __syncthreads();
    if (tid < 3 * VP9HIP_METRIC_FIELDS) {
        const uint32_t p = tid / VP9HIP_METRIC_FIELDS, f = tid % VP9HIP_METRIC_FIELDS;
        unsigned long long v = S.part[p][0][f];
#pragma unroll
        for (int w = 1; w < MET_WG / 64; w++) {
            const unsigned long long o = S.part[p][w][f];
            v = f == VP9HIP_METRIC_MAXDIFF ? (o > v ? o : v) : f == VP9HIP_METRIC_FIRST ? (o < v ? o : v) : v + o;
        }
        unsigned long long *dst = g.out + ((size_t) z * 3 + p) * VP9HIP_METRIC_FIELDS + f;
        // a total that changes nothing is not sent. (Reading the record first, to skip an extreme
        // it has passed already, was tried and lost: the reads queue behind the atomics.)
        if (f == VP9HIP_METRIC_FIRST) { if (v != ~0ull) atomicMin(dst, v); }
        else if (f == VP9HIP_METRIC_MAXDIFF) { if (v) atomicMax(dst, v); }
        else if (v) atomicAdd(dst, v);
    }
}

// The records before the sums: zeros, FIRST all ones
__global__ __launch_bounds__(MET_WG) void k_metrics_init(unsigned long long *out, const uint32_t count)
{
    const uint32_t i = blockIdx.x * MET_WG + threadIdx.x;
    if (i < count) out[i] = i % VP9HIP_METRIC_FIELDS == VP9HIP_METRIC_FIRST ? ~0ull : 0ull;
}

template <typename T>
void met_launch(const MetArgs &a, const dim3 grid, hipStream_t st)
{
    if (!a.has_b) hipLaunchKernelGGL((k_metrics<T, false, false>), grid, dim3(MET_WG), 0, st, a);
    else if (!a.cells) hipLaunchKernelGGL((k_metrics<T, true, false>), grid, dim3(MET_WG), 0, st, a);
    else hipLaunchKernelGGL((k_metrics<T, true, true>), grid, dim3(MET_WG), 0, st, a);
}

} // namespace

hipError_t vp9hip_metrics_launch(const MetArgs &args, int hbd, int n, hipStream_t st)
{
    MetArgs a = args;
    if (n < 1 || n > MET_MAX_PAIRS || a.w < 1 || a.h < 1 || !a.out || (a.cells && !a.has_b)) return hipErrorInvalidValue;
    // The strips: the tallest that still give the launch MET_FILL workgroups, so small frames
    // spread over the machine; then no more workgroups a pair than its share of MET_FILL, each
    // with the same number of strips (up to rounding) and at most MET_MAX_STRIPS.
    a.nsx = (a.w + MET_TW - 1) / MET_TW;
    a.th = 128;
    while (a.th > 32 && (int64_t) n * a.nsx * ((a.h + a.th - 1) / a.th) < MET_FILL) a.th >>= 1;
    a.nstrips = a.nsx * ((a.h + a.th - 1) / a.th);
    const int cap = std::max((MET_FILL + n - 1) / n, (a.nstrips + MET_MAX_STRIPS - 1) / MET_MAX_STRIPS);
    const int per = (a.nstrips + cap - 1) / cap;                // strips a workgroup
    const int wgs = (a.nstrips + per - 1) / per;
    const uint32_t count = (uint32_t) n * 3 * VP9HIP_METRIC_FIELDS;
    hipLaunchKernelGGL(k_metrics_init, dim3((count + MET_WG - 1) / MET_WG), dim3(MET_WG), 0, st, a.out, count);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned) wgs, 1, (unsigned) n);
    if (hbd) met_launch<uint16_t>(a, grid, st);
    else met_launch<uint8_t>(a, grid, st);
    return hipGetLastError();
}
