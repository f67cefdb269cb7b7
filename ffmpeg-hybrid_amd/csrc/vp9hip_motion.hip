// Motion export for gfx950: k_motion turns the resident block array of a batch into the dense
// per-4x4-cell tensors of include/vp9hip.h ("motion export"): info (refs, mode, size / skip /
// segment) and mv (two coded vectors) for every cell of every exporting frame, each cell once.
//
// The blocks are untrusted (the kernel does not wait for the planner's verdict): row, col and
// bs are clipped here, a block outside the grid or of an unknown size covers nothing, and no
// store leaves the GW x GH cells of the frame's own planes.
//
// Work distribution, k_mcq's flat-task idiom: a 256-thread workgroup takes 256 consecutive
// blocks of one frame; each thread loads its block (13 dwords), packs what the cells need into
// LDS (structure of arrays, so lanes reading neighbouring owners hit neighbouring banks, never a
// 13-dword stride) and counts its clipped cells; the workgroup scans the counts; the threads
// then walk the flat cell indices in strides of 256, each finding its owner by a binary search
// of the 257 prefix sums (8 LDS reads), and store one 8-byte mv and one 4-byte info per cell.
// Consecutive flat indices inside a block row are consecutive addresses. No atomics, no
// pre-clear. A 64x64 block is 256 cells and a 4x4-coded 8x8 is 4: one thread per block looping
// over its cells (k_motion_loop, kept for the measurement) is imbalanced and uncoalesced.
#include "vp9hip_motion.h"

namespace {

// log2 of a block size's width / height in 4-pixel units, a nibble per VP9H_BS_* (sizes below
// 8x8 cover their 8x8 unit: 2 x 2 cells)
#define MOT_LW 0x1111122233344ull
#define MOT_LH 0x1111212323434ull

// What the cells of one block need, from its 13 dwords (vp9h_block: row, col | bs, tx, uvtx, skip |
// intra, comp, seg_id, filter | mode[4] | uvmode, ref[2], pad | mv[4][2] as x | y << 16).
struct MotBlk {
    uint32_t pos;       // first cell: row | col << 16
    uint32_t geo;       // clipped width in cells | ceil(65536 / width) << 8
    uint32_t info;      // info bytes 0, 1, 3 (byte 2, the cell's mode, is zero)
    uint32_t cnt;       // clipped cells
    uint32_t mvk[2];    // all ones for a reference whose vectors are exported, else zero
};

__device__ __forceinline__ MotBlk mot_block(const uint32_t d0, const uint32_t d1, const uint32_t d2, const uint32_t d4,
                                            const uint32_t gw, const uint32_t gh)
{
    MotBlk m;
    const uint32_t row = d0 & 0xffff, col = d0 >> 16, bs = d1 & 0xff, skip = d1 >> 24;
    const uint32_t intra = d2 & 0xff, comp = (d2 >> 8) & 0xff, seg = (d2 >> 16) & 0xff;
    const uint32_t r0 = 2 * row, c0 = 2 * col;
    uint32_t cw = 0, ch = 0;
    if (bs < VP9H_N_BS && r0 < gh && c0 < gw) {
        cw = 1u << ((uint32_t) (MOT_LW >> (4 * bs)) & 15);
        ch = 1u << ((uint32_t) (MOT_LH >> (4 * bs)) & 15);
        cw = cw < gw - c0 ? cw : gw - c0;
        ch = ch < gh - r0 ? ch : gh - r0;
    }
    const uint32_t i0 = intra ? 255u : (d4 >> 8) & 0xff;
    const uint32_t i1 = (!intra && comp) ? (d4 >> 16) & 0xff : 255u;
    m.pos = r0 | c0 << 16;
    // y = t / cw for t < 256, cw <= 16 as (t * ceil(65536 / cw)) >> 16: the error t / 65536 is
    // below the 1 / cw a quotient's fraction stays under 1 by
    m.geo = cw | (cw ? (65536u + cw - 1) / cw : 0u) << 8;
    m.info = i0 | i1 << 8 | ((bs | skip << 4 | seg << 5) & 0xff) << 24;
    m.cnt = cw * ch;
    m.mvk[0] = i0 != 255 ? ~0u : 0u;
    m.mvk[1] = i1 != 255 ? ~0u : 0u;
    return m;
}

struct MotLds {
    uint32_t off[MOT_WG + 1];          // exclusive prefix sums of the cell counts
    uint32_t wsum[MOT_WG / 64];
    uint32_t pos[MOT_WG], geo[MOT_WG], info[MOT_WG], mode[MOT_WG];
    // [sub-block i * 2 + reference][block], masked. Rows padded by 4 dwords: the lanes of one
    // block read 4 different i of the same column, which an unpadded row stride (a multiple of
    // 32 banks) would put on one bank; with it they fall 8 banks apart
    uint32_t mv[8][MOT_WG + 4];
};

__global__ __launch_bounds__(MOT_WG) void k_motion(const MotionFrame *__restrict__ frames,
                                                   const uint32_t *__restrict__ blocks)
{
    __shared__ MotLds S;
    const MotionFrame F = frames[blockIdx.y];
    const uint32_t tid = threadIdx.x, b0 = blockIdx.x * MOT_WG;
    if (b0 >= F.nblk) return;                                   // uniform: before any barrier
    const uint32_t gw = 2 * F.cols8, gh = 2 * F.rows8;
    uint32_t cnt = 0;
    if (b0 + tid < F.nblk) {
        const uint32_t *p = blocks + (size_t) (F.blk0 + b0 + tid) * 13;
        const MotBlk m = mot_block(p[0], p[1], p[2], p[4], gw, gh);
        cnt = m.cnt;
        S.pos[tid] = m.pos; S.geo[tid] = m.geo; S.info[tid] = m.info; S.mode[tid] = p[3];
#pragma unroll
        for (int j = 0; j < 8; j++) S.mv[j][tid] = p[5 + j] & m.mvk[j & 1];
    }
    // exclusive scan of the 256 counts: inside each wave by shuffles, then the waves' totals
    uint32_t inc = cnt;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = __shfl_up(inc, d, 64);
        if ((tid & 63) >= (uint32_t) d) inc += v;
    }
    if ((tid & 63) == 63) S.wsum[tid >> 6] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (uint32_t w = 0; w < MOT_WG / 64; w++) base += w < (tid >> 6) ? S.wsum[w] : 0u;
    S.off[tid] = base + inc - cnt;
    if (tid == MOT_WG - 1) S.off[MOT_WG] = base + inc;
    __syncthreads();
    const uint32_t T = S.off[MOT_WG];
    uint8_t *const mvp = (uint8_t *) F.mv, *const infop = (uint8_t *) F.info;
    for (uint32_t g = tid; g < T; g += MOT_WG) {
        // the owner: the last k with off[k] <= g (blocks without cells share their successor's offset)
        uint32_t lo = 0, hi = MOT_WG;
#pragma unroll
        for (int s = 0; s < 8; s++) {
            const uint32_t mid = (lo + hi) >> 1;
            if (S.off[mid] <= g) lo = mid; else hi = mid;
        }
        const uint32_t t = g - S.off[lo], geo = S.geo[lo], pos = S.pos[lo];
        const uint32_t cw = geo & 0xff, y = (t * (geo >> 8)) >> 16, x = t - y * cw;
        const uint32_t r = (pos & 0xffff) + y, c = (pos >> 16) + x;
        if (r >= gh || c >= gw) continue;                       // cannot happen: cw, ch were clipped
        const uint32_t i = (r & 1) * 2 + (c & 1);
        const size_t cell = (size_t) r * F.pitch + c;
        const uint32_t mode = (S.mode[lo] >> (8 * i)) & 0xff;
        *(uint2 *) (mvp + cell * 8) = make_uint2(S.mv[2 * i][lo], S.mv[2 * i + 1][lo]);
        *(uint32_t *) (infop + cell * 4) = S.info[lo] | mode << 16;
    }
}

// The measured alternative: one thread per block, looping over its cells.
__global__ __launch_bounds__(MOT_WG) void k_motion_loop(const MotionFrame *__restrict__ frames,
                                                        const uint32_t *__restrict__ blocks)
{
    const MotionFrame F = frames[blockIdx.y];
    const uint32_t bi = blockIdx.x * MOT_WG + threadIdx.x;
    if (bi >= F.nblk) return;
    const uint32_t gw = 2 * F.cols8, gh = 2 * F.rows8;
    const uint32_t *p = blocks + (size_t) (F.blk0 + bi) * 13;
    const MotBlk m = mot_block(p[0], p[1], p[2], p[4], gw, gh);
    const uint32_t cw = m.geo & 0xff, ch = cw ? m.cnt / cw : 0, modes = p[3];
    uint32_t mv[8];
#pragma unroll
    for (int j = 0; j < 8; j++) mv[j] = p[5 + j] & m.mvk[j & 1];
    uint8_t *const mvp = (uint8_t *) F.mv, *const infop = (uint8_t *) F.info;
    for (uint32_t y = 0; y < ch; y++)
        for (uint32_t x = 0; x < cw; x++) {
            const uint32_t r = (m.pos & 0xffff) + y, c = (m.pos >> 16) + x;
            if (r >= gh || c >= gw) continue;
            const uint32_t i = (r & 1) * 2 + (c & 1);
            const size_t cell = (size_t) r * F.pitch + c;
            // four selects, not an indexed register array (scratch)
            const uint32_t m0 = i == 0 ? mv[0] : i == 1 ? mv[2] : i == 2 ? mv[4] : mv[6];
            const uint32_t m1 = i == 0 ? mv[1] : i == 1 ? mv[3] : i == 2 ? mv[5] : mv[7];
            *(uint2 *) (mvp + cell * 8) = make_uint2(m0, m1);
            *(uint32_t *) (infop + cell * 4) = m.info | ((modes >> (8 * i)) & 0xff) << 16;
        }
}

} // namespace

hipError_t vp9hip_motion_launch(const MotionFrame *frames, int nframes, int max_blk, const vp9h_block *blocks,
                                int shape, hipStream_t st)
{
    if (nframes <= 0 || max_blk <= 0) return hipSuccess;
    const dim3 grid((unsigned) ((max_blk + MOT_WG - 1) / MOT_WG), (unsigned) nframes);
    if (shape == 1) hipLaunchKernelGGL(k_motion_loop, grid, dim3(MOT_WG), 0, st, frames, (const uint32_t *) blocks);
    else hipLaunchKernelGGL(k_motion, grid, dim3(MOT_WG), 0, st, frames, (const uint32_t *) blocks);
    return hipGetLastError();
}
