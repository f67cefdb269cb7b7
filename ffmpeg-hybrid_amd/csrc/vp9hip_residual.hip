// Residual export for gfx950: k_residual puts what itxfm_add adds before its clip, clipped to
// +-(2^bpp - 1), into three int16 planes per exporting frame (include/vp9hip.h, "residual
// export"), from what the device planner leaves resident: one TxRec per tx block of every SB
// slot (k_psb), the slots' record counts and coefficient bases, and the coefficient arena.
//
// One 256-thread workgroup per SB slot of an exporting frame, and it writes every sample of the
// SB's three squares exactly once: no pre-clear, no atomics, no ordering between stores.
//   1. The records (at most RES_JCAP) are loaded 256 at a time. A workgroup scan of their eobs
//      gives each block's coefficient offset (the sum k_pjplan forms), and in the same scan each
//      coded block gets its rank among the SB's blocks of its size. Every record passes the
//      guards of resid_rec_n (vp9hip_residual.h) or is dropped: the records come from untrusted
//      packets, and the kernel does not wait for the planner's verdict.
//   2. A record that survives marks its 4x4 units in an LDS byte map and enters the list of its
//      size, so the lanes of a wave run one transform size.
//   3. The units no block marked are stored as zeros (8 bytes per row and lane).
//   4. 4x4 blocks (the WHT included): one lane a block, resid4_tx in registers, four 8-byte row
//      stores. 8x8 / 16x16 / 32x32: N lanes a block, 64 / N blocks a wave; the scan-order
//      coefficients are scattered into a padded LDS image, lane li transforms column li, the image
//      is rewritten transposed, lane li transforms its column again and stores one int16 of each of
//      the block's N rows, so N adjacent lanes write one contiguous segment. A wave works in its
//      own part of LDS, so the passes are ordered by wave barriers alone. Blocks with eob 1 and a
//      DCT_DCT type take the reference's DC-only shortcut.
// The transforms are the __host__ __device__ ones of vp9hip_resid4.h / vp9hip_residn.h under the
// M32 (8-bit, wrapping, int16 intermediates) and M64 (int64, int32 intermediates) policies.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define VP9T_STORAGE static __constant__ constexpr
#include "vp9_tables.h"
#include <type_traits>

#include "vp9hip_residual.h"

namespace {

#define DEV __device__ __forceinline__

DEV void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// what the workgroup scan carries: the eobs, and the counts of the coded blocks per size, two to a word
struct Scan3 { uint32_t e, c01, c23; };
DEV Scan3 operator+(const Scan3 &a, const Scan3 &b) { return { a.e + b.e, a.c01 + b.c01, a.c23 + b.c23 }; }

template <typename COEF> struct ResLds {
    uint32_t w[RES_JCAP];              // TxRec.w
    uint32_t coff[RES_JCAP];           // first coefficient (element offset in the arena)
    uint32_t em[RES_JCAP];             // eob | key << 11 | rank in its size << 16; 0xffffffff: dropped or not coded
    uint16_t idx[RES_JCAP];            // the coded records by size: 4x4, 8x8, 16x16, 32x32
    uint8_t cover[3 * 256];            // 4x4 units a coded block covers
    Scan3 ws[RES_WG / 64];
    COEF img[RES_WG / 64][64 * 34];    // per wave: 64 / N blocks of N rows of RStride coefficients
};

template <int N> DEV const int16_t *scan_n(uint32_t txtp)
{
    if (N == 8) return txtp == 1 ? vp9t_scan_col_8x8 : txtp == 2 ? vp9t_scan_row_8x8 : vp9t_scan_default_8x8;
    if (N == 16) return txtp == 1 ? vp9t_scan_col_16x16 : txtp == 2 ? vp9t_scan_row_16x16 : vp9t_scan_default_16x16;
    return vp9t_scan_default_32x32;
}

struct Geo {
    int16_t *plane[3];
    uint32_t pitch[2];
    uint32_t px0[2], py0[2];           // the SB's top-left in the luma / chroma planes
    int32_t maxv;
};
DEV uint32_t rec_pitch(const Geo &G, uint32_t w) { return (w & 3) ? G.pitch[1] : G.pitch[0]; }
DEV int16_t *rec_dst(const Geo &G, uint32_t w)
{
    // selects, not indexed member arrays (scratch)
    const uint32_t p = w & 3, ux0 = (w >> 12) & 15, uy0 = (w >> 16) & 15;
    int16_t *const base = p == 0 ? G.plane[0] : p == 1 ? G.plane[1] : G.plane[2];
    const uint32_t py0 = p ? G.py0[1] : G.py0[0], px0 = p ? G.px0[1] : G.px0[0];
    return base + (size_t) (py0 + 4 * uy0) * rec_pitch(G, w) + px0 + 4 * ux0;
}

// the 4x4 blocks of the list idx[0 .. n): a lane each
template <class M, typename COEF>
DEV void blocks4(const ResLds<COEF> &S, const Geo &G, const COEF *__restrict__ coefs, uint32_t n, uint32_t tid)
{
    for (uint32_t i = tid; i < n; i += RES_WG) {
        const uint32_t t = S.idx[i];
        if (t == 0xffff) continue;                              // dropped for its coefficient offset
        const uint32_t w = S.w[t], em = S.em[t], eob = em & 2047, key = (em >> 11) & 31;
        const COEF *src = coefs + S.coff[t];
        COEF c[16];
#pragma unroll
        for (int k = 0; k < 16; k++) c[k] = (uint32_t) k < eob ? src[k] : (COEF) 0;
        int32_t res[16];
        resid4_block<M, COEF>((int) (key >> 2), (int) (key & 3), c, (int) eob, res);
        int16_t *dst = rec_dst(G, w);
        const uint32_t pitch = rec_pitch(G, w);
#pragma unroll
        for (int y = 0; y < 4; y++) {
            const uint32_t r0 = (uint32_t) resid_clip(res[y], G.maxv) & 0xffff, r1 = (uint32_t) resid_clip(res[4 + y], G.maxv) & 0xffff;
            const uint32_t r2 = (uint32_t) resid_clip(res[8 + y], G.maxv) & 0xffff, r3 = (uint32_t) resid_clip(res[12 + y], G.maxv) & 0xffff;
            *(uint2 *) (dst + (size_t) y * pitch) = make_uint2(r0 | r1 << 16, r2 | r3 << 16);
        }
    }
}

// the N x N blocks of the list idx[first .. first + n): N lanes a block, 64 / N blocks a wave
template <int N, class M, typename COEF>
DEV void blocksn(ResLds<COEF> &S, const Geo &G, const COEF *__restrict__ coefs, uint32_t first, uint32_t n, uint32_t tid)
{
    typedef typename M::T T;
    constexpr int SS = RStride<N, COEF>::S, BITS = resid_bits(N), PER = RES_WG / N;
    static_assert(64 / N * N * SS <= 64 * 34, "a wave's blocks fit its part of the image");
    const uint32_t lane = tid & 63, li = lane % N;
    COEF *img = S.img[tid >> 6] + (lane / N) * (N * SS);
    for (uint32_t r0 = 0; r0 < n; r0 += PER) {                  // uniform over the workgroup
        const uint32_t i = r0 + tid / N;
        const uint32_t t = i < n ? S.idx[first + i] : 0xffffu;
        const bool act = t != 0xffff;                           // 0xffff: dropped for its coefficient offset
        uint32_t w = 0, eob = 0, txtp = 0, coff = 0;
        if (act) {
            const uint32_t em = S.em[t];
            w = S.w[t]; eob = em & 2047; txtp = (em >> 11) & 3; coff = S.coff[t];
        }
        const bool full = act && !(eob == 1 && txtp == 0);
        wsync();                                                // the previous round's reads are done
        if (full)
#pragma unroll
            for (int k = 0; k < N; k++) img[li * SS + k] = 0;
        wsync();
        if (full) {
            const int16_t *scan = scan_n<N>(txtp);
            for (uint32_t k = li; k < eob; k += N) {
                const uint32_t pos = (uint32_t) scan[k] & (N * N - 1);
                img[(pos / N) * SS + pos % N] = coefs[coff + k];
            }
        }
        wsync();
        T v[N];
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = 0;
        if (full) {                                             // first pass (type_a): column li
#pragma unroll
            for (int k = 0; k < N; k++) v[k] = M::in(img[k * SS + li]);
            tx1n<N, M>(v, (int) (txtp & 1));
        }
        wsync();
        if (full)                                               // into row li: the block transposed
#pragma unroll
            for (int k = 0; k < N; k++) img[li * SS + k] = (COEF) (int64_t) v[k];
        wsync();
        int32_t out[N];
        if (full) {                                             // second pass (type_b): column li again
#pragma unroll
            for (int k = 0; k < N; k++) v[k] = M::in(img[k * SS + li]);
            tx1n<N, M>(v, (int) (txtp >> 1));
#pragma unroll
            for (int k = 0; k < N; k++) {
                const int32_t ov = (COEF) (int64_t) v[k];
                out[k] = (int32_t) ((uint32_t) ov + (1u << (BITS - 1))) >> BITS;
            }
        } else {
            const int32_t add = act ? resid_dc_only<M>((int32_t) coefs[coff], BITS) : 0;
#pragma unroll
            for (int k = 0; k < N; k++) out[k] = add;
        }
        if (act) {
            int16_t *dst = rec_dst(G, w) + li;
            const uint32_t pitch = rec_pitch(G, w);
#pragma unroll
            for (int k = 0; k < N; k++) dst[(size_t) k * pitch] = (int16_t) resid_clip(out[k], G.maxv);
        }
    }
}

template <bool HB>
__global__ __launch_bounds__(RES_WG) void k_residual(ResidArgs A)
{
    typedef typename std::conditional<HB, int32_t, int16_t>::type COEF;
    typedef typename std::conditional<HB, M64, M32>::type M;
    __shared__ ResLds<COEF> S;
    const ResidFrame F = A.frames[blockIdx.y];
    const uint32_t s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t slot = F.slot0 + s;
    if (s >= F.nsb || slot >= A.nslots || !F.sb_cols) return;          // uniform: before any barrier
    const uint32_t sbx = s % F.sb_cols, sby = s / F.sb_cols;
    const uint32_t dord = F.slot0 + (uint32_t) pl_sb_dorder((int) sbx, (int) sby, (int) F.sb_cols);
    const COEF *coefs = (const COEF *) A.coefs;
    uint32_t T = A.sb_tn[slot] & 0xffff;
    T = T < A.jcap ? T : A.jcap;
    T = T < RES_JCAP ? T : RES_JCAP;
    const uint32_t coef_sb = dord < A.nslots ? A.sb_coef0[dord] : 0u;
    const TxRec *rec = A.txrec + (size_t) slot * A.jcap;
    Geo G;
    G.plane[0] = (int16_t *) F.plane[0]; G.plane[1] = (int16_t *) F.plane[1]; G.plane[2] = (int16_t *) F.plane[2];
    G.pitch[0] = F.pitch[0]; G.pitch[1] = F.pitch[1];
    G.px0[0] = sbx * 64; G.py0[0] = sby * 64;
    G.px0[1] = sbx * (64u >> F.ss_h); G.py0[1] = sby * (64u >> F.ss_v);
    G.maxv = (int32_t) F.maxv;

    for (uint32_t i = tid; i < 3 * 256 / 4; i += RES_WG) ((uint32_t *) S.cover)[i] = 0;
    // 1. offsets, guards, ranks
    Scan3 carry = { 0, 0, 0 };
    for (uint32_t c0 = 0; c0 < T; c0 += RES_WG) {                        // uniform
        const uint32_t t = c0 + tid;
        TxRec r = { 0, 0 };
        if (t < T) r = rec[t];
        const uint32_t e0 = TXR_EOB(r.m), key = TXR_KEY(r.m);
        Scan3 v = { e0, 0, 0 };
        // the offset below needs the scan; the guards' other inputs do not
        const int n0 = t < T && e0 ? resid_rec_n(key, e0, r.w & 3, (r.w >> 12) & 15, (r.w >> 16) & 15, sbx, sby, F.sb_cols,
                                                 F.sb_rows, F.ss_h, F.ss_v, 0, A.total_coefs) : 0;
        const uint32_t cls = n0 == 8 ? 1u : n0 == 16 ? 2u : n0 == 32 ? 3u : 0u;
        if (n0) { if (cls < 2) v.c01 = 1u << (16 * cls); else v.c23 = 1u << (16 * (cls - 2)); }
        Scan3 inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            Scan3 u;
            u.e = __shfl_up(inc.e, d, 64); u.c01 = __shfl_up(inc.c01, d, 64); u.c23 = __shfl_up(inc.c23, d, 64);
            if (lane >= (uint32_t) d) inc = inc + u;
        }
        __syncthreads();                                                 // the previous chunk's sums were read
        if (lane == 63) S.ws[wave] = inc;
        __syncthreads();
        Scan3 base = carry, tot = carry;
#pragma unroll
        for (uint32_t k = 0; k < RES_WG / 64; k++) {
            const Scan3 x = S.ws[k];
            if (k < wave) base = base + x;
            tot = tot + x;
        }
        carry = tot;
        if (t < T) {
            const uint64_t off = (uint64_t) coef_sb + base.e + inc.e - e0;
            // a dropped record's coefficients still count: the offsets of the blocks behind it stay right
            const bool ok = n0 && off + e0 <= A.total_coefs;
            const uint32_t packed = cls < 2 ? base.c01 + inc.c01 - v.c01 : base.c23 + inc.c23 - v.c23;
            const uint32_t rank = (packed >> (16 * (cls & 1))) & 0xffff;
            S.w[t] = r.w;
            S.coff[t] = (uint32_t) off;
            S.em[t] = ok ? e0 | key << 11 | rank << 16 : 0xffffffffu;
            if (ok) {                                                    // 2. its units in the map
                const uint32_t p = r.w & 3, ux0 = (r.w >> 12) & 15, uy0 = (r.w >> 16) & 15, step = (uint32_t) n0 >> 2;
                for (uint32_t y = 0; y < step; y++)
                    for (uint32_t x = 0; x < step; x++) S.cover[p * 256 + (uy0 + y) * 16 + ux0 + x] = 1;
            }
        }
    }
    // the lists' bases: a record dropped for its offset leaves its list entry unused (marked below)
    const uint32_t n4 = carry.c01 & 0xffff, n8 = carry.c01 >> 16, n16 = carry.c23 & 0xffff, n32 = carry.c23 >> 16;
    const uint32_t b8 = n4, b16 = b8 + n8, b32 = b16 + n16;               // n4 + n8 + n16 + n32 <= T <= RES_JCAP
    for (uint32_t i = tid; i < RES_JCAP; i += RES_WG) S.idx[i] = 0xffff;
    __syncthreads();
    for (uint32_t t = tid; t < T; t += RES_WG) {
        const uint32_t em = S.em[t];
        if (em == 0xffffffffu) continue;
        const uint32_t tc = (em >> 13) & 7, cls = tc == 4 ? 0u : tc;
        const uint32_t b = cls == 0 ? 0u : cls == 1 ? b8 : cls == 2 ? b16 : b32;
        S.idx[b + (em >> 16)] = (uint16_t) t;
    }
    __syncthreads();
    // 3. zeros where no block is
#pragma unroll
    for (uint32_t p = 0; p < 3; p++) {
        const uint32_t c = p ? 1u : 0u, ux = tid & 15, uy = tid >> 4;
        const uint32_t uw = 16u >> (p ? F.ss_h : 0u), uh = 16u >> (p ? F.ss_v : 0u);
        if (ux < uw && uy < uh && !S.cover[p * 256 + tid]) {
            int16_t *dst = G.plane[p] + (size_t) (G.py0[c] + 4 * uy) * G.pitch[c] + G.px0[c] + 4 * ux;
#pragma unroll
            for (int y = 0; y < 4; y++) *(uint2 *) (dst + (size_t) y * G.pitch[c]) = make_uint2(0u, 0u);
        }
    }
    // 4. the blocks, size by size
    blocks4<M, COEF>(S, G, coefs, n4, tid);
    blocksn<8, M, COEF>(S, G, coefs, b8, n8, tid);
    blocksn<16, M, COEF>(S, G, coefs, b16, n16, tid);
    blocksn<32, M, COEF>(S, G, coefs, b32, n32, tid);
}

} // namespace

hipError_t vp9hip_residual_launch(const ResidArgs &A, int nframes, int max_sb, int hb, hipStream_t st)
{
    if (nframes <= 0 || max_sb <= 0) return hipSuccess;
    const dim3 grid((unsigned) max_sb, (unsigned) nframes);
    if (hb) hipLaunchKernelGGL(k_residual<true>, grid, dim3(RES_WG), 0, st, A);
    else hipLaunchKernelGGL(k_residual<false>, grid, dim3(RES_WG), 0, st, A);
    return hipGetLastError();
}
