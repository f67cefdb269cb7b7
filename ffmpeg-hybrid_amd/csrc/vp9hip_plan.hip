// Device planner (gfx950): the per-frame work planning of the pixel path, from the pass-1
// packets resident in HBM to the records the pixel kernels consume (vp9hip_work.h). It
// replaces, on the GPU, the host planner of vp9hip_runtime.cpp and applies the same rules
// (vp9hip_planlogic.h), so a batch needs nothing from the host between its packets and its
// frames except the launch list, which depends on the record counts only.
//
//   k_pblk   one thread per block: the SB slot of each block, the slots' block ranges,
//            decode-order validation, eob entries per block
//   (scan)   eob entries -> each block's first eob
//   k_psb    one wave per SB, the one enumeration of its tx blocks in decode order: eobs ->
//            coefficient total, residual-job counts per (tcode, txtp), MC-unit count, the intra
//            4x4-unit map, and one record per tx block (TxRec: eob, key, rank within the key,
//            position, intra mode)
//   (scan)   coefficients (decode order) -> each SB's first coefficient; counts -> record offsets
//   k_pjplan one wave per SB: from the records, the residual jobs and the intra job words with
//            check_intra_mode resolved (vp9recon.c:37-221); then the intra jobs' producers,
//            heights, list-scheduled passes (the host's merge_mixed, restated wave-parallel),
//            the SB's intra step
//   k_pllf   one wave per SB: the LF program (vp9block.c:1142-1262, vp9lpf.c:31-230)
//   k_plmc   one wave per SB of inter frames: MC units (vp9_mc_template.c:30-464)
//   k_plevel one workgroup per level-scheduled inter frame: SB dependency levels along
//            anti-diagonals
//   k_pkeys  step-list offsets; the launch summary the host reads back
//   k_plists the intra step lists
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "vp9hip_plan.h"

#define DEV __device__ __forceinline__

namespace {

// Wave-wide scans and reductions on DPP (row shifts within 16-lane rows, then the gfx9
// row broadcasts of lanes 15 / 31): VALU-latency steps instead of ds_bpermute round trips.
// Every value of a uniform lane index is read with readlane.
enum { OP_ADD, OP_OR, OP_MAX };
template <int OP> DEV uint32_t dpp_op(uint32_t a, uint32_t b) { return OP == OP_OR ? (a | b) : OP == OP_MAX ? (a > b ? a : b) : (a + b); }
template <int OP> DEV uint32_t wscan_dpp(uint32_t v)
{
    v = dpp_op<OP>(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x111, 0xf, 0xf, true));   // row_shr:1
    v = dpp_op<OP>(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x112, 0xf, 0xf, true));   // row_shr:2
    v = dpp_op<OP>(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x114, 0xf, 0xf, true));   // row_shr:4
    v = dpp_op<OP>(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x118, 0xf, 0xf, true));   // row_shr:8
    v = dpp_op<OP>(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x142, 0xa, 0xf, false));  // row_bcast:15
    v = dpp_op<OP>(v, (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x143, 0xc, 0xf, false));  // row_bcast:31
    return v;
}
DEV uint32_t wscan_incl(uint32_t v, int) { return wscan_dpp<OP_ADD>(v); }
DEV uint32_t rdl(uint32_t v, int l) { return (uint32_t) __builtin_amdgcn_readlane((int) v, l); }
DEV int rdl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
DEV uint32_t wsum(uint32_t v) { return rdl(wscan_dpp<OP_ADD>(v), 63); }
DEV uint32_t mbcnt(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0));
}
// Bounds guard of every planner write: false (and a status bit) when i >= cap.
DEV bool inb(const PlanDev &D, uint32_t i, uint32_t cap, uint32_t bit)
{
    if (i < cap) return true;
    atomicOr(&D.status[1], bit);
    atomicOr(&D.status[0], PLS_BOUNDS);
    return false;
}
// A frame's packet is inconsistent: its status bits, for the batch and for the frame.
DEV void plan_fail(const PlanDev &D, const PlanFrame &F, uint32_t st)
{
    atomicOr(D.status, st);
    if ((uint32_t) F.frame < D.nframes) atomicOr(&D.fbad[F.frame], st);
}
// The planner's workgroups are one wave: the LDS unit executes a wave's DS instructions in
// order, so a wave-scope fence (compiler ordering) replaces the workgroup barrier.
DEV void wsync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// A block as the planner uses it: fields out of range are clamped (the batch fails with
// PLS_BLOCK / PLS_MODE from k_pblk / k_psb, and every later index stays in bounds).
DEV vp9h_block load_block(const vp9h_block *g)
{
    vp9h_block b = *g;
    if (b.bs >= VP9H_N_BS) b.bs = VP9H_BS_4x4;
    if (b.tx > 3) b.tx = 0;
    if (b.uvtx > 3) b.uvtx = 0;
    return b;
}
// The block fields the tx enumeration reads (16 bytes in LDS instead of 52).
struct PBlk {
    uint16_t row, col;
    uint8_t bs, tx, uvtx, skip, intra, uvmode;
    uint8_t mode[4];
    uint8_t pad[2];
};
DEV PBlk pblk(const vp9h_block &b)
{
    PBlk r;
    r.row = b.row; r.col = b.col; r.bs = b.bs; r.tx = b.tx; r.uvtx = b.uvtx; r.skip = b.skip; r.intra = b.intra;
    r.uvmode = b.uvmode;
    for (int i = 0; i < 4; i++) r.mode[i] = b.mode[i];
    r.pad[0] = r.pad[1] = 0;
    return r;
}
DEV bool block_ok(const vp9h_block &b)
{
    return b.bs < VP9H_N_BS && b.tx <= 3 && b.uvtx <= 3;
}

// Per (block, plane) tx-block counts, packed all | eob << 10 | intra jobs << 20, and their
// exclusive scan over the SB's blocks in decode order (pre[3 * nb] = totals); ent: the tx grid
// of each (block, plane) entry, so the per-tx code reads one word instead of redoing pl_txgrid:
// txs | tx blocks per row << 2 | the entry's first 4x4 unit in its SB plane, x << 7, y << 11 |
// the block's width in the plane (4x4 units) << 15
#define ENT_TXS(e) ((int) ((e) & 3))
#define ENT_NX(e)  ((int) (((e) >> 2) & 31))
#define ENT_UX(e)  ((int) (((e) >> 7) & 15))
#define ENT_UY(e)  ((int) (((e) >> 11) & 15))
#define ENT_PW4(e) ((int) (((e) >> 15) & 31))
template <int SSH, int SSV, class B>
DEV uint32_t sb_prefix(const B *blk, int nb, int cols, int rows, bool mine, uint32_t *pre, uint32_t *ent, int lane)
{
    uint32_t v[3] = { 0, 0, 0 };
    if (lane < nb) {
        const B &b = blk[lane];
        for (int p = 0; p < 3; p++) {
            const PlTxGrid g = pl_txgrid(b, p, cols, rows, SSH, SSV);
            const uint32_t n = (uint32_t) (g.nx * g.ny);
            v[p] = n | (b.skip ? 0u : n) << 10 | (b.intra && mine ? n : 0u) << 20;
            const int sh = p ? SSH : 0, sv = p ? SSV : 0;
            ent[3 * lane + p] = (uint32_t) g.txs | (uint32_t) (g.nx & 31) << 2 | (uint32_t) ((g.bx >> 2) & ((16 >> sh) - 1)) << 7 |
                                (uint32_t) ((g.by >> 2) & ((16 >> sv) - 1)) << 11 | (uint32_t) (g.pw4 & 31) << 15;
        }
    }
    const uint32_t sum = v[0] + v[1] + v[2];
    const uint32_t incl = wscan_incl(sum, lane), excl = incl - sum;
    if (lane < nb) {
        pre[3 * lane] = excl;
        pre[3 * lane + 1] = excl + v[0];
        pre[3 * lane + 2] = excl + v[0] + v[1];
    }
    const uint32_t tot = rdl(incl, 63);
    if (lane == 0) pre[3 * nb] = tot;
    wsync();
    return tot;
}

// q = l / n for l < 4096, 1 <= n <= 16: the multiply by ceil(2^16 / n) is exact there
DEV int udiv16(int l, int n)
{
    return (int) (((uint32_t) l * ((65536u + (uint32_t) n - 1) / (uint32_t) n)) >> 16);
}
DEV bool mc_refs_ok(const vp9h_block &b, const PlMcGeo &g)
{
    if (b.ref[0] > 2 || (b.comp && b.ref[1] > 2)) return false;
    const int r1 = b.comp ? b.ref[1] : b.ref[0];
    return g.scale[b.ref[0]][0] != 0xFFFF && g.scale[r1][0] != 0xFFFF;
}

DEV uint32_t cnt_idx(const PlanDev &D, const PlanFrame &F, uint32_t seg, uint32_t slot, int tc, int tp)
{
    return D.seg_pre4[seg] + (uint32_t) tc * F.s4 + (uint32_t) tp * D.seg_sz[seg] + D.slot_pos[slot];
}

struct SbGeo {
    int sbx, sby, tile_sb0, mine;
    uint32_t slot, seg, dord;
};
DEV SbGeo sb_geo(const PlanFrame &F, int s)
{
    SbGeo G;
    G.sbx = s % F.sb_cols;
    G.sby = s / F.sb_cols;
    const int tile = pl_tile_of(G.sbx, F.sb_cols, F.log2_tc, &G.tile_sb0);
    G.mine = tile >= F.tile_lo && tile < F.tile_hi;
    G.slot = F.slot0 + (uint32_t) s;
    G.seg = F.seg0 + (F.by_diag ? (uint32_t) ((G.sbx - G.tile_sb0) + G.sby) : 0u);
    G.dord = F.slot0 + (uint32_t) pl_sb_dorder(G.sbx, G.sby, F.sb_cols);
    return G;
}

// The SB's block range; 0 blocks if it has none (the batch is already marked invalid).
DEV int sb_blocks(const PlanDev &D, uint32_t slot, uint32_t &b0, uint32_t &st)
{
    b0 = D.sb_first[slot];
    const uint32_t b1 = D.sb_end[slot];
    if (b0 == 0xffffffffu || b1 == 0xffffffffu || b1 <= b0 || b1 > D.total_blocks) { st |= PLS_ORDER; b0 = 0; return 0; }
    if (b1 - b0 > 64) { st |= PLS_ORDER; return 64; }
    return (int) (b1 - b0);
}

// ------------------------------------------------------------------ k_pblk
__global__ __launch_bounds__(256) void k_pblk(PlanDev D)
{
    const PlanFrame &F = D.frames[blockIdx.y];
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= F.nblk) return;
    const uint32_t gi = F.blk0 + i;
    const int cols = F.mc.cols, rows = F.mc.rows;
    auto sb_of = [&](const vp9h_block &b, int &dord) {
        const int sbx = pl_min(b.col, cols - 1) >> 3, sby = pl_min(b.row, rows - 1) >> 3;
        dord = pl_sb_dorder(sbx, sby, F.sb_cols);
        return F.slot0 + (uint32_t) (sby * F.sb_cols + sbx);
    };
    const vp9h_block raw = D.blocks[gi];
    uint32_t st = 0;
    if (!block_ok(raw) || raw.row >= rows || raw.col >= cols) st |= PLS_BLOCK;
    const vp9h_block b = load_block(&D.blocks[gi]);
    int d, dp = -1, dn = -1;
    const uint32_t slot = sb_of(b, d);
    uint32_t sp = 0xffffffffu, sn = 0xffffffffu;
    if (i > 0) sp = sb_of(load_block(&D.blocks[gi - 1]), dp);
    if (i + 1 < F.nblk) sn = sb_of(load_block(&D.blocks[gi + 1]), dn);
    if (!inb(D, slot, D.nslots, 1u)) return;
    if (sp != slot) {
        D.sb_first[slot] = gi;
        if (i > 0 && dp >= d) st |= PLS_ORDER;       // SBs in decode order, each one contiguous
    }
    if (sn != slot) D.sb_end[slot] = gi + 1;
    uint32_t n = 0;
    if (!b.skip)
        for (int p = 0; p < 3; p++) {
            const PlTxGrid g = pl_txgrid(b, p, cols, rows, F.mc.ss_h, F.mc.ss_v);
            n += (uint32_t) (g.nx * g.ny);
        }
    D.blk_neob[gi] = n;
    if (st) plan_fail(D, F, st);
}

// VP9HIP_PLAN_PROF: shader-clock cycles of each k_psb / k_pjplan phase, summed over the SBs
#define PPT(k) do { if (D.prof) { const unsigned long long t_ = clock64(); \
        if (lane == 0) atomicAdd(&D.prof[k], t_ - pt0); pt0 = t_; } } while (0)
#define JA_TRX (1u << 30)     // PlanLds.ja: the 4x4 top-right lies inside the block (trx)

// ------------------------------------------------------------------ the SB's tx enumeration
// The front half of the enumeration of an SB's tx blocks in decode order: its blocks, the
// per-(block, plane) prefix counts, the first tx of every (block, plane) entry (ost, for the
// max-scan of sb_own) and the SB's window of eob entries.
template <int JCAP> struct SbEnumLds {
    PBlk blk[64];
    uint32_t pre[3 * 64 + 1];
    uint32_t ent[3 * 64];         // tx grid of each (block, plane) entry (ENT_*)
    uint32_t eb[64];              // first eob entry of each block
    alignas(4) uint16_t ost[JCAP];   // (block, plane) entry starting at tx t, else 0
};
struct SbEnum {
    int nb, T;                    // blocks, tx blocks (clamped to JCAP)
    uint32_t b0, tot;             // first block, sb_prefix's totals
    uint32_t E0, E;               // the SB's eob entries: D.eobs[E0 .. E0 + E)
};
template <int SSH, int SSV, int JCAP>
DEV SbEnum sb_enum(const PlanDev &D, const PlanFrame &F, const SbGeo &G, SbEnumLds<JCAP> &S, vp9h_block &own, uint32_t &st,
                   int lane)
{
    SbEnum R;
    R.nb = sb_blocks(D, G.slot, R.b0, st);
    uint32_t be = 0;
    if (lane < R.nb) {
        own = load_block(&D.blocks[R.b0 + lane]);
        S.blk[lane] = pblk(own);
        be = D.blk_eob0[R.b0 + (uint32_t) lane];
        S.eb[lane] = be;
    }
    // the SB's eob entries are contiguous in the packet (its coded blocks' tx in decode order)
    R.E0 = rdl(be, 0);
    const uint32_t E1 = R.nb ? D.blk_eob0[R.b0 + (uint32_t) R.nb] : R.E0;
    R.E = E1 - R.E0;
    if (E1 < R.E0 || R.E > (uint32_t) JCAP || E1 > D.total_eobs) { st |= PLS_EOB; R.E = 0; }
    for (int i = lane; i < JCAP / 2; i += 64) ((uint32_t *) S.ost)[i] = 0;
    wsync();
    R.tot = sb_prefix<SSH, SSV>(S.blk, R.nb, F.mc.cols, F.mc.rows, G.mine, S.pre, S.ent, lane);
    R.T = pl_min((int) (R.tot & 1023), JCAP);
    // each non-empty (block, plane) entry marks its first tx (the ranges are disjoint)
    if (lane < R.nb)
        for (int p = 0; p < 3; p++) {
            const int k = 3 * lane + p;
            const uint32_t a0 = S.pre[k] & 1023, a1 = S.pre[k + 1] & 1023;
            if (a1 > a0 && a0 < (uint32_t) R.T) S.ost[a0] = (uint16_t) k;
        }
    wsync();
    return R;
}
// The (block, plane) entry of tx c + lane of a chunk of 64: a max-scan over the entries'
// first tx (the largest k with pre[k] <= t); carry runs from chunk to chunk.
DEV int sb_own(const uint16_t *ost, int c, int T, uint32_t &carry, int lane)
{
    const uint32_t v = c + lane < T ? ost[c + lane] : 0u;
    const uint32_t incl = dpp_op<OP_MAX>(wscan_dpp<OP_MAX>(v), carry);
    carry = rdl(incl, 63);
    return (int) incl;
}
// The eob of tx t of the SB, in block b (0 for skipped blocks, which have no entries): one
// load from the SB's eob window, range-checked against the window and the tx size. (A frame whose eob
// count disagrees with its packet shifts the later frames' eobs: k_pkeys' totals check
// rejects the batch then, PLS_TOTAL.)
template <int JCAP>
DEV int sb_tx_eob(const PlanDev &D, const SbEnumLds<JCAP> &S, const SbEnum &R, int b, int txs, uint32_t t, uint32_t &st)
{
    if (S.blk[b].skip) return 0;
    const uint32_t i = S.eb[b] - R.E0 + t - (S.pre[3 * b] & 1023);
    if (i >= R.E) { st |= PLS_EOB; return 0; }
    const int e = D.eobs[R.E0 + i];
    if (e > (16 << (2 * txs))) { st |= PLS_EOB; return 0; }
    return e;
}

// ------------------------------------------------------------------ k_psb
// The one enumeration of the SB's tx blocks: the counts the scans need (residual jobs per
// key, coefficients, MC units), the intra unit map, and one TxRec per tx block for k_pjplan,
// which emits from the records alone (what is counted is what is emitted).
// Residual-job counts: lane k holds key k's count, one ballot per distinct key of a chunk;
// a job's rank within its key is the count before the chunk plus its position in the ballot.
// Intra unit map: ORed into IBC copies of the 24 map words (copy = lane & 3), so at most a
// quarter of a chunk's lanes share an address. Round 4's per-lane map columns (6.2 KB of
// LDS) removed the conflicts but cut occupancy from 32 to 15 waves per CU and made the
// kernel 1.58x slower; the blocks are held as 16-byte PBlk for the same reason (LDS 3.9 KB
// per workgroup at 4:2:0, 4.6 KB at 4:4:4: the 32-waves/CU cap binds, not LDS).
// The kernel is bound by the instructions it issues (8 waves per SIMD hide its loads), so
// per-tx work that k_pjplan can do from the record is left to it (pl_intra_job).
#define IBC 4
template <int SSH, int SSV>
__global__ __launch_bounds__(64) void k_psb(PlanDev D)
{
    constexpr int CW = 16 >> SSH, CH = 16 >> SSV, JCAP = 256 + 2 * CW * CH;
    __shared__ SbEnumLds<JCAP> S;
    __shared__ uint32_t ibw[24 * IBC];
    const PlanFrame F = D.frames[blockIdx.y];     // by value, before any store: one batch of scalar loads
    const PlMcGeo &mcg = D.frames[blockIdx.y].mc; // the reference scales are indexed: left in memory
    const int s = blockIdx.x, lane = threadIdx.x;
    if (s >= F.sb_cols * F.sb_rows) return;
    unsigned long long pt0 = D.prof ? clock64() : 0;
    const SbGeo G = sb_geo(F, s);
    const int cols = F.mc.cols, rows = F.mc.rows;
    uint32_t st = 0;
    if (lane < 24 * IBC / 2) { ibw[2 * lane] = 0; ibw[2 * lane + 1] = 0; }
    vp9h_block own;
    const SbEnum R = sb_enum<SSH, SSV>(D, F, G, S, own, st, lane);
    const int nb = R.nb, T = R.T;
    const bool rec_ok = inb(D, G.slot, D.nslots, 4u);
    TxRec *rec = D.txrec + (size_t) G.slot * JCAP;
    PPT(0);
    uint32_t ncoef = 0, kcnt = 0, ocarry = 0;
    for (int c = 0; c < T; c += 64) {
        const int t = c + lane;
        const int k = sb_own(S.ost, c, T, ocarry, lane);
        int key = -1;
        uint32_t w = 0, m = 0;
        if (t < T) {
            const int bi = (k * 171) >> 9, p = k - 3 * bi;      // k / 3 for k < 192
            const uint32_t en = S.ent[k];
            const PBlk &b = S.blk[bi];
            const int sh = p ? SSH : 0, sv = p ? SSV : 0, txs = ENT_TXS(en), step = 1 << txs;
            const int l = t - (int) (S.pre[k] & 1023), nx = pl_max(ENT_NX(en), 1), q = udiv16(l, nx);
            const int x = (l - q * nx) << txs, y = q << txs;        // 4x4 units in the block
            const int e = sb_tx_eob(D, S, R, bi, txs, (uint32_t) t, st);
            ncoef += (uint32_t) e;
            int mode = 0, txtp = 0;
            if (b.intra) {
                mode = p ? b.uvmode : b.mode[b.bs > VP9H_BS_8x8 && b.tx == 0 ? y * 2 + x : 0];
                if (mode > 9) { st |= PLS_MODE; mode = 0; }
                txtp = p || txs == 3 ? 0 : pl_intra_txfm_type(mode);
            }
            const int ux0 = ENT_UX(en) + x, uy0 = ENT_UY(en) + y;
            m = (uint32_t) e | (uint32_t) ((F.lossless ? 4 : txs) * 4 + txtp) << 11;
            if (e && G.mine) { key = (int) TXR_KEY(m); m |= 1u << 16; }
            w = (uint32_t) p | (uint32_t) txs << 2 | (uint32_t) (ux0 & 15) << 12 | (uint32_t) (uy0 & 15) << 16;
            if (b.intra && G.mine) {
                // the job's 4x4 units in the SB plane's unit map
                const int units = 16 >> sh, unitsv = 16 >> sv;
                uint32_t um = 0;
                for (int u = ux0; u < ux0 + step && u < units; u++) um |= 1u << u;
                for (int v = uy0; v < uy0 + step && v < unitsv; v++)
                    atomicOr(&ibw[(p * 8 + (v >> 1)) * IBC + (lane & (IBC - 1))], um << ((v & 1) * 16));
                // pl_intra_job's other inputs: k_pjplan resolves check_intra_mode
                w |= (uint32_t) mode << 8 | (x < ENT_PW4(en) - 1 ? TXR_RIGHT : 0u) | TXR_JOB;
            }
        }
        // counts and ranks within each key, in decode order: one ballot per distinct key
        uint64_t pend = __ballot(key >= 0);
        while (pend) {
            const int kk = rdl(key, __builtin_ctzll(pend));
            const uint64_t mk = __ballot(key == kk);
            const uint32_t base = rdl(kcnt, kk);
            if (key == kk) m |= (base + mbcnt(mk)) << 17;
            if (lane == kk) kcnt += (uint32_t) __popcll(mk);
            pend &= ~mk;
        }
        if (t < T && rec_ok) { TxRec r; r.w = w; r.m = m; rec[t] = r; }
    }
    PPT(1);
    // MC units of the SB's inter blocks
    uint32_t nmc = 0;
    if (lane < nb && G.mine && !own.intra) {
        if (mc_refs_ok(own, mcg)) nmc = (uint32_t) pl_mc_block(own, mcg, 0, [](const McUnit &) {});
        else st |= PLS_REF;
    }
    nmc = wsum(nmc);
    ncoef = wsum(ncoef);
    wsync();
    uint32_t ib = 0;
    if (lane < 24)
#pragma unroll
        for (int j = 0; j < IBC; j++) ib |= ibw[lane * IBC + j];
    if (lane < 20) {
        const uint32_t ci = cnt_idx(D, F, G.seg, G.slot, lane >> 2, lane & 3);
        if (inb(D, ci, D.cap_cnt, 2u)) D.cnt[ci] = kcnt;
    }
    if (lane == 20) {
        const uint32_t ci = D.seg_pre1[G.seg] + D.slot_pos[G.slot];
        if (inb(D, ci, D.cap_cntm, 2u)) D.cntm[ci] = nmc;
    }
    if (lane < 24 && rec_ok) D.ibits[(size_t) G.slot * 24 + lane] = ib;
    if (lane == 0 && rec_ok) D.sb_tn[G.slot] = (uint32_t) T | (uint32_t) pl_min((int) (R.tot >> 20), JCAP) << 16;
    if (lane == 0 && inb(D, G.dord, D.nslots, 8u)) D.sb_ncoef[G.dord] = ncoef;
    if (st) plan_fail(D, F, st);
    PPT(2);
}

// ------------------------------------------------------------------ k_pjplan
// plan_sb's LDS: the unit map, then the heights, then the priority order share one region,
// each dead before the next is written; the producer lists die with the heights, and the
// readiness masks and done bits of the pass loop take their place (7.2 KB at 4:2:0)
template <int JCAP> struct alignas(16) PlanLds {   // 16: jmap rows are stored 16 bytes at a time
    uint32_t ja[JCAP];            // PJob word per intra job (decode order), bit 30: the 4x4
                                  // top-right lies inside the block (trx)
    union {
        uint16_t jmap[3][256];    // producing job of each 4x4 unit (PL_JM_ENT)
        struct {
            union {
                uint32_t hgt[JCAP];           // longest path to a sink (list-scheduling priority)
                uint16_t ord[JCAP];           // jobs by (height desc, index asc)
            } h;
            uint16_t doff[JCAP + 1];      // producers of job j: dep[2 (doff & 2047) ..] (count doff >> 11)
            union {
                uint16_t dep[4 * JCAP];
                struct {
                    // pl_deps' masks of job j: the units it waits for (after the pass loop: the
                    // pass words, counted from the positions' records)
                    uint32_t mk[JCAP];
                    // units whose job an earlier pass took: bit u of the 16-bit row p * 16 + v and
                    // bit v of the 16-bit column p * 16 + u for unit (u, v) of plane p, two rows
                    // to a word (pl_done_bits; a fourth plane's worth, and indices masked, so that
                    // no job word can address past them)
                    uint32_t drow[32], dcol[32];
                } rd;
            } d;
            uint32_t hs[64];              // height histogram -> list starts (before: the heights' spare words)
        } b;
    } u;
};
static_assert(sizeof(uint16_t[3][256]) <= sizeof(uint32_t[256 + 2 * 64]), "the unit map fits the heights' region");
#define JM_ENT PL_JM_ENT

// edges the job's (substituted) mode reads: 1 left, 2 top, 4 top-left, 8 top-right (pl_intra_job)
DEV uint32_t needs_of(uint32_t a)
{
    return (uint32_t) pl_slot_needs((int) ((a >> 8) & 15));
}
DEV uint32_t wor(uint32_t v) { return rdl(wscan_dpp<OP_OR>(v), 63); }
DEV bool wany(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }
// f(integral_constant<int, c>) for c = 0 .. N - 1: an unrolled loop over the chunks of a lane's register arrays
template <int N, class F> DEV void each_chunk(F &&f)
{
    if constexpr (N > 0) {
        each_chunk<N - 1>(f);
        f(std::integral_constant<int, N - 1>());
    }
}

// One wave per SB: the residual jobs (every coded tx block, bucketed by transform) and the
// intra job words of the SB, from k_psb's records alone: no block, no eob entry is read again.
// A job's position is its key's scanned base (lanes 0..19 hold the 20 bases, fetched by key
// across lanes) plus its rank in the record, so every counted position is written, with an
// eob-0 job where the coefficient check fails.
// The wave's loads are issued in three batches, not one chain per chunk: the SB's header
// words with the first chunk of records (its address needs only the slot; lanes past the
// record count are masked afterwards), then the key bases with the other chunks, then the
// nonzero boxes of every chunk; the stores follow (six chunks at a time: one group at 4:2:0,
// two at 4:4:4, whose records would not fit the registers). Bounds failures are reported at the end
// (an atomic in between would turn the later uniform loads into dependent vector loads).
// ja: k_pjplan's LDS job words; returns the SB's intra job count
template <int SSH, int SSV>
DEV int pjob_sb(const PlanDev &D, const PlanFrame &F, const SbGeo &G, uint32_t *ja)
{
    constexpr int CW = 16 >> SSH, CH = 16 >> SSV, JCAP = 256 + 2 * CW * CH, NCH = 6;
    const int lane = threadIdx.x;
    unsigned long long pt0 = D.prof ? clock64() : 0;
    const uint32_t slot = G.slot;
    uint32_t st = 0, bf = 0;                  // PLS_* bits, status[1] bits of failed bounds
    if (slot >= D.nslots) bf |= 4u;
    if (G.dord >= D.nslots) bf |= 32u;
    const TxRec *rec = D.txrec + (size_t) slot * JCAP;
    TxRec x[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) x[c].w = x[c].m = 0;
    if (!bf) x[0] = rec[lane];
    const uint32_t tn = bf ? 0u : D.sb_tn[slot];
    const uint32_t coef_sb = bf ? 0u : D.sb_coef0[G.dord];
    // record bases of the SB's residual keys (tcode * 4 + txtp) in lanes 0..19
    uint32_t rb = 0;
    if (lane < 20) {
        const uint32_t ci = cnt_idx(D, F, G.seg, slot, lane >> 2, lane & 3);
        if (ci < D.cap_cnt) rb = D.cnt0[ci];
        else bf |= 16u;
    }
    const int T = pl_min((int) (tn & 0xffff), JCAP), NJ = pl_min((int) (tn >> 16), JCAP);
    if (lane >= T) x[0].w = x[0].m = 0;
    const uint32_t rbase = slot * D.rcap;
    const uint16_t *nz16 = (const uint16_t *) D.nz;        // nzc | nzr << 8 per (key, eob)
    const int cols = F.mc.cols, rows = F.mc.rows, tx0l = G.tile_sb0 * 64;
    uint32_t carry = 0;                       // SB-relative first coefficient of the chunk
    unsigned long long ibytes = 0;
    int nj = 0;
    for (int g0 = 0; g0 < T; g0 += 64 * NCH) {            // groups of NCH chunks
#pragma unroll
    for (int c = 0; c < NCH; c++)
        if (g0 || c) {
            x[c].w = x[c].m = 0;
            if (g0 + c * 64 + lane < T) x[c] = rec[g0 + c * 64 + lane];
        }
    PPT(3);
    // pass 1: coefficient offsets, nonzero boxes, the intra job words
    uint32_t coef[NCH], nzv[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        if (g0 + c * 64 >= T) break;
        const uint32_t w = x[c].w, m = x[c].m;
        const uint32_t e0 = TXR_EOB(m), key = TXR_KEY(m);
        const uint32_t incl = wscan_incl(e0, lane);
        uint32_t cf = coef_sb + carry + incl - e0, e = e0;
        carry += rdl(incl, 63);
        if (TXR_EMIT(m) && cf + e > D.total_coefs) { st |= PLS_COEF; e = 0; cf = 0; x[c].m = m & ~2047u; }
        coef[c] = cf;
        nzv[c] = TXR_EMIT(m) ? nz16[key * 1025 + e] : 0u;
        const uint64_t mj = __ballot((w & TXR_JOB) != 0);
        if (w & TXR_JOB) {
            // check_intra_mode resolved (vp9recon.c:37-221) from the record's inputs
            const int p = w & 3, txs = (w >> 2) & 3, ux0 = (w >> 12) & 15, uy0 = (w >> 16) & 15;
            const PlIntra pi = pl_intra_job_sb(p, txs, (int) ((w >> 8) & 15), (int) e0, G.sbx, G.sby, ux0, uy0,
                                               (w & TXR_RIGHT) != 0, tx0l, cols, rows, SSH, SSV);
            ja[nj + (int) mbcnt(mj)] = pi.a | (pi.trx ? JA_TRX : 0u);      // at most T <= JCAP
        }
        nj += __popcll(mj);
    }
    PPT(4);
    // pass 2: the residual jobs
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        if (g0 + c * 64 >= T) break;
        const uint32_t w = x[c].w, m = x[c].m, key = TXR_KEY(m);
        const uint32_t base = (uint32_t) __shfl((int) rb, (int) key);
        if (TXR_EMIT(m)) {
            const int p = w & 3, txs = (w >> 2) & 3, ux0 = (w >> 12) & 15, uy0 = (w >> 16) & 15;
            const int sh = p ? SSH : 0, sv = p ? SSV : 0;
            const bool intra = (w & TXR_JOB) != 0;
            uint32_t dst;
            if (intra) dst = rbase + pl_resid_unit(p, ux0, uy0, SSH, SSV);
            else {
                dst = (uint32_t) ((size_t) (G.sby * (64 >> sv) + uy0 * 4) * F.pitch[p ? 1 : 0] + G.sbx * (64 >> sh) + ux0 * 4);
                ibytes += (unsigned long long) (2 * (16 << (2 * txs)) * F.bypp);
            }
            // RJob: coef, dst, eob | frame << 16, ptx | nzc << 8 | nzr << 16 (pad 0)
            const uint32_t ptx = (uint32_t) p | (key >> 2) << 2 | (intra ? 0u : 1u) << 5 | (key & 3) << 6;
            const uint32_t pos = base + TXR_RANK(m);
            if (pos < D.cap_rjobs)
                *(uint4 *) &D.rjobs[pos] = make_uint4(coef[c], dst, TXR_EOB(m) | (uint32_t) (F.frame & 0xffff) << 16,
                                                      ptx | nzv[c] << 8);
            else bf |= 64u;
        }
    }
    PPT(5);
    }
    for (int d = 32; d; d >>= 1) ibytes += __shfl_xor(ibytes, d);
    if (lane == 0 && ibytes) {
        if ((uint32_t) F.frame < D.nframes) atomicAdd(&D.fbytes[2 * F.frame], ibytes);
        else bf |= 2048u;
    }
    bf = wor(bf);
    if (lane == 0 && bf) { atomicOr(&D.status[1], bf); atomicOr(&D.status[0], PLS_BOUNDS); }
    st = wor(st);
    if (lane == 0 && st) plan_fail(D, F, st);
    return pl_min(nj, NJ);
}
static_assert(sizeof(RJob) == 16 && offsetof(RJob, eob) == 8 && offsetof(RJob, frame) == 10 && offsetof(RJob, ptx) == 12 &&
              offsetof(RJob, nzc) == 13 && offsetof(RJob, nzr) == 14, "pjob_sb stores an RJob as one uint4");

// One wave per SB: producers of every intra job, heights, priority order, list-scheduled
// passes (the host's merge_mixed), the PJob / pass records, the SB's records, its level
// dependencies and intra step. The job words are in S.ja already (pjob_sb), nj of them.
// (Two SBs per wave with the second's job words loaded under the first's scheduling cut the
// first load's share of a wave's cycles from 31 to 20 %, but not the kernel: 2,880 -> 2,926 us
// per C3 batch. By its counters the kernel is bound by scalar issue: about 4,300 SALU per wave at
// 22 waves per CU)
template <int SSH, int SSV>
DEV void plan_sb(const PlanDev &D, const PlanFrame &F, const SbGeo &G, PlanLds<256 + 2 * (16 >> SSH) * (16 >> SSV)> &S, int nj)
{
    constexpr int CW = 16 >> SSH, CH = 16 >> SSV, JCAP = 256 + 2 * CW * CH, NCH = JCAP / 64;
    const int lane = threadIdx.x;
    unsigned long long pt0 = D.prof ? clock64() : 0;
    const uint32_t slot = G.slot;
    const uint32_t rbase = slot * D.rcap;
    uint32_t st = 0;
    const int NJ = pl_min(nj, JCAP);
    for (int i = lane; i < 3 * 256 / 8; i += 64) ((uint4 *) &S.u.jmap[0][0])[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
    wsync();
    PPT(6);
    // the unit map: each job's 4x4 units hold JM_ENT(job, units to the job's right edge, units
    // to its bottom edge), so the producer walk below steps past a producer's extent from the
    // entry alone (one LDS read per producer instead of the entry and the job's word)
    for (int j = lane; j < NJ; j += 64) {
        const uint32_t a = S.ja[j];
        const int p = a & 3, step = 1 << ((a >> 2) & 3), ux0 = (a >> 12) & 15, uy0 = (a >> 16) & 15;
        const int units = p ? CW : 16, unitsv = p ? CH : 16;
        if (ux0 + step <= units) {
            // a job is an aligned square inside its plane's 16-unit rows, so each of its unit
            // rows is one aligned 2 / 4 / 8 / 16-byte store: a 32x32 job paints 8 rows, not 64
            // units (the loop's trip count is the largest job's of the chunk)
            uint16_t *row = &S.u.jmap[p][uy0 * 16 + ux0];
            for (int v = 0; v < step && uy0 + v < unitsv; v++, row += 16) {
                const uint32_t b = JM_ENT(j, 0, step - 1 - v);
                // two units: right distances r and r - 1 (the lower address first)
                auto e2 = [&](uint32_t r) { return (b | r << 10) | (b | (r - 1) << 10) << 16; };
                if (step == 1) *row = (uint16_t) b;
                else if (step == 2) *(uint32_t *) row = e2(1);
                else if (step == 4) *(uint2 *) row = make_uint2(e2(3), e2(1));
                else *(uint4 *) row = make_uint4(e2(7), e2(5), e2(3), e2(1));
            }
        } else {
            for (int v = uy0; v < uy0 + step && v < unitsv; v++)
                for (int u = ux0; u < ux0 + step && u < units; u++)
                    S.u.jmap[p][v * 16 + u] = (uint16_t) JM_ENT(j, ux0 + step - 1 - u, uy0 + step - 1 - v);
        }
    }
    wsync();
    PPT(7);

    // ---- producers of every intra job (the pixels its substituted mode reads): pl_deps walks
    // the two runs of units job j reads in the unit map
    auto deps_of = [&](int j, auto fn) {
        const uint32_t a = S.ja[j];
        const int p = a & 3, ts = (a >> 2) & 3, ux0 = (a >> 12) & 15, uy0 = (a >> 16) & 15;
        return pl_deps(S.u.jmap[p], j, ux0, uy0, 1 << ts, (int) needs_of(a), (a & JA_TRX) ? 1 : 0, p ? CW : 16, p ? CH : 16, fn);
    };
    uint32_t mreg[NCH];                       // pl_deps' masks of jobs c * 64 + lane
#pragma unroll
    for (int c = 0; c < NCH; c++) mreg[c] = 0;
    {
        // one enumeration: job j's list starts at the prefix sum of the per-size bounds (an
        // n-unit job reads at most 2n + 2 units: its left column, and the top row with the
        // top-left and top-right units; 4 * JCAP for a tiling of 4x4 jobs): every bound is
        // even, so doff[j] holds the start / 2 in bits 0-10 and the length in bits 11-15
        uint32_t carry = 0;
        for (int c = 0; c < NJ; c += 64) {
            const int j = c + lane;
            const uint32_t cap = j < NJ ? 2u * (1u << ((S.ja[j] >> 2) & 3)) + 2u : 0u;
            const uint32_t incl = wscan_incl(cap, lane);
            const uint32_t off = carry + incl - cap;
            uint32_t mk = 0;
            if (j < NJ) {
                uint32_t k = off;
                if (off + cap <= 4u * JCAP) mk = deps_of(j, [&](int d) { if (k < off + cap) S.u.b.d.dep[k++] = (uint16_t) d; });
                else st |= PLS_SCHED;
                // (an empty list starts at 0: the heights read a list's first four entries unasked)
                S.u.b.doff[j] = (uint16_t) (k > off ? off >> 1 | (k - off) << 11 : 0u);
            }
            // the masks wait in registers until the lists are dead (selects on the uniform
            // chunk index: the array stays in registers)
#pragma unroll
            for (int cc = 0; cc < NCH; cc++)
                if (c == cc * 64) mreg[cc] = mk;
            carry += rdl(incl, 63);
        }
        wsync();                              // jmap is dead: hgt overlays it
        for (int j = lane; j < NJ; j += 64) S.u.b.h.hgt[j] = 1;
    }
    wsync();
    PPT(8);
    // ---- heights (longest path to a sink). Producers precede their consumers (d < j), so
    // the chunks of 64 jobs are finished last to first: a chunk's consumers in later chunks
    // are final, and the chunk relaxes until none of its own jobs rises (at most one round
    // per job of a chain inside it); its last round pushes final heights to every producer.
    // pl_heights_chunk's round reads the lane's height and issues four returning maxima from
    // registers, one wait; a producer that does not exist is a word of hs, which is not live yet
    // (VP9HIP_PLAN_DBG bit 4, timing only: no relaxation, every height stays 1)
    {
        uint32_t *hgt = S.u.b.h.hgt;
        const uint32_t spare = (uint32_t) (S.u.b.hs - hgt);
        auto each = [&](auto fn) { const bool r = fn(lane, 0); wsync(); return __any(r) != 0; };
        auto amax = [&](uint32_t i, uint32_t v) { return atomicMax(&hgt[i], v); };
        for (int c = (D.dbg & 16) ? -1 : ((NJ - 1) & ~63); c >= 0; c -= 64)
            pl_heights_chunk<1>(hgt, S.u.b.d.dep, S.u.b.doff, c, NJ, spare, each, amax);
    }
    PPT(9);
    // ---- priority order: height descending, then decode order. The heights go to registers
    // first: the order overlays them (NCH = JCAP / 64 chunks). The producer lists are dead:
    // the masks and the (empty) done bits take their place
    int hreg[NCH];
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int j = c * 64 + lane;
        hreg[c] = j < NJ ? pl_min((int) S.u.b.h.hgt[j], 63) : -1;
        if (j < NJ) S.u.b.d.rd.mk[j] = mreg[c];
    }
    if (lane < 32) S.u.b.d.rd.drow[lane] = S.u.b.d.rd.dcol[lane] = 0;
    S.u.b.hs[lane] = 0;
    wsync();
#pragma unroll
    for (int c = 0; c < NCH; c++)
        if (hreg[c] >= 0) atomicAdd(&S.u.b.hs[hreg[c]], 1u);
    wsync();
    {
        const uint32_t v = S.u.b.hs[63 - lane];                // heights from the top
        const uint32_t incl = wscan_incl(v, lane);
        wsync();
        S.u.b.hs[63 - lane] = incl - v;
        wsync();
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            if (c * 64 >= NJ) break;
            const int j = c * 64 + lane;
            const int h = hreg[c];
            // the chunk's lanes of this lane's height, from one ballot per bit of the height (no
            // loop over the chunk's distinct heights); the first of them takes the height's
            // next positions for all, each lane its rank among them
            uint64_t m = __ballot(h >= 0);
#pragma unroll
            for (int b = 0; b < 6; b++) {
                const uint64_t bal = __ballot((h >> b) & 1);
                m &= ((h >> b) & 1) ? bal : ~bal;
            }
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
            uint32_t base = 0;
            if (h >= 0 && rank == 0) base = atomicAdd(&S.u.b.hs[h], (uint32_t) __popcll(m));
            base = (uint32_t) __shfl((int) base, __ffsll((unsigned long long) m) - 1);
            if (h >= 0) S.u.b.h.ord[base + rank] = (uint16_t) j;
        }
    }
    wsync();
    PPT(10);
    // ---- list scheduling (merge_mixed): each pass takes, in priority order, every ready job
    // (all producers in earlier passes) that still fits in 64 lanes; lane groups by size.
    // The pass loop only decides: a taken lane notes its pass and its rank among the pass's jobs
    // of its size, and marks its units done. The jobs and the pass words are written once, after
    // the loop, chunk-wide (the epilogue below).
    uint32_t *gpass = D.passes + (size_t) slot * JCAP;
    PJob *gjob = D.pjobs + (size_t) slot * JCAP;
    int done = 0, npass = 0;
    // Each lane holds, per chunk c of the priority order, position c * 64 + lane: its job with
    // its size code and the done rows of its two runs (pl_jw), its masks, what it ORs into the
    // done bits once taken (pl_done_bits for its rows and its columns, pl_done_reg: computed here,
    // once, not at every take), its record once taken (pl_take_rec; registers, not LDS: the
    // resource report allows it), and bit c of `pend` while it is unscheduled. A job is ready
    // when the done rows hold every unit of its masks: two independent 16-bit LDS reads.
    uint32_t jwreg[NCH], mkreg[NCH], rcreg[NCH], drreg[NCH], dcreg[NCH], dxreg[NCH];
    uint32_t pend = 0;
#pragma unroll
    for (int c = 0; c < NCH; c++) {
        const int pos = c * 64 + lane;
        jwreg[c] = mkreg[c] = drreg[c] = dcreg[c] = dxreg[c] = 0;
        rcreg[c] = PL_REC_NONE;
        if (pos < NJ) {
            const uint32_t j = S.u.b.h.ord[pos], a = S.ja[j];
            const int p = a & 3, ts = (a >> 2) & 3, ux0 = (a >> 12) & 15, uy0 = (a >> 16) & 15;
            jwreg[c] = pl_jw(j, a);
            drreg[c] = pl_done_bits(ts, ux0, uy0);
            dcreg[c] = pl_done_bits(ts, uy0, ux0);
            dxreg[c] = pl_done_reg(p, ts, ux0, uy0);
            mkreg[c] = S.u.b.d.rd.mk[j];
            pend |= 1u << c;
        }
    }
    const uint16_t *drow16 = (const uint16_t *) S.u.b.d.rd.drow, *dcol16 = (const uint16_t *) S.u.b.d.rd.dcol;      // the 16-bit rows
    if (D.dbg & 2) done = NJ;                 // ablation (timing only): no pass building
    while (done < NJ) {
        // No job of a pass may see another job of the same pass as done, and the takes below
        // mark their units at once. So the readiness of every chunk is read here, at the top of
        // the pass, before the first update (the batched form: one bit per chunk in one register,
        // 2 NCH reads back to back with no branch around them, at 4:4:4 too: the reads' results
        // die into `rdy` one by one and cost no registers). The wave's LDS operations execute
        // in program order; wsync() at the pass's end holds the compiler to it.
        uint32_t rdy = 0;
#pragma unroll
        for (int c = 0; c < NCH; c++) {
            const uint32_t jw = jwreg[c], mk = mkreg[c];
            // every lane reads (scheduled and empty positions too: their indices are valid)
            const uint32_t have = drow16[PL_JW_ROW(jw)] | (uint32_t) dcol16[PL_JW_COL(jw)] << 16;
            rdy |= (have & mk) == mk ? 1u << c : 0u;
        }
        rdy &= pend;
        int budget = 64;
        uint32_t pc = 0;                      // class counts of the pass so far, a byte each
        // (each_chunk, not a loop under #pragma unroll: at 4:4:4 the compiler leaves the twelve
        // visits rolled, and the lanes' register arrays then go through indexed moves)
        each_chunk<NCH>([&](auto C) {
            constexpr int c = decltype(C)::value;
            if (budget < 4) return;
            const bool cand = (rdy >> c) & 1u;
            if (!wany(cand)) return;              // nothing ready in this chunk
            // takes in priority order by one packed prefix sum: the longest prefix of the chunk's
            // ready jobs that fits. (A second round over the jobs skipped can take nothing: the
            // first one skipped is larger than the lanes left, and so is every prefix sum after
            // it. Any packing that respects the producers is exact; only the pass count
            // depends on it.)
            // (the position's word through an empty asm: what the take derives from it is the
            // same in every pass, and hoisted out of the loop it costs some 50 registers at 4:2:0)
            uint32_t jw = jwreg[c];
            asm volatile("" : "+v"(jw));
            const uint32_t ts8 = PL_JW_TS8(jw);
            const uint32_t pre = wscan_incl(cand ? pl_take_val(ts8) : 0u, lane), incl = pl_take_lanes(pre);
            const bool take = cand && incl <= (uint32_t) budget;
            const uint64_t m = __builtin_amdgcn_ballot_w64(take);
            if (!m) return;
            // the job's units are done for the passes that follow: one 32-bit OR for its rows and
            // one for its columns, and the next word (16x16) or three (32x32) in the visits that
            // take such a job
            uint32_t dx = dxreg[c];
            asm volatile("" : "+v"(dx));           // (as jw above: its fields are not hoisted)
            const uint32_t dr = drreg[c], dc = dcreg[c], ri = PL_DONE_ROW(dx), ci = PL_DONE_COL(dx);
            if (take) {
                pend &= ~(1u << c);
                rcreg[c] = pl_take_rec(npass, pre, pc, ts8);
                atomicOr(&S.u.b.d.rd.drow[ri], dr);
                atomicOr(&S.u.b.d.rd.dcol[ci], dc);
            }
            const bool big = take && PL_DONE_TS(dx) >= 2;
            if (wany(big)) {
                if (big) {
                    atomicOr(&S.u.b.d.rd.drow[(ri + 1) & 31], dr);
                    atomicOr(&S.u.b.d.rd.dcol[(ci + 1) & 31], dc);
                }
                if (big && PL_DONE_TS(dx) == 3)
                    for (uint32_t i = 2; i < 4; i++) {
                        atomicOr(&S.u.b.d.rd.drow[(ri + i) & 31], dr);
                        atomicOr(&S.u.b.d.rd.dcol[(ci + i) & 31], dc);
                    }
            }
            const int last = 63 - __builtin_clzll(m);
            pc += rdl(pre, last);
            budget -= (int) rdl(incl, last);
        });
        if (pc == 0) { st |= PLS_SCHED; break; }
        done += (int) pl_take_count(pc);
        npass++;
        wsync();
    }
    // ---- epilogue: the pass words and the jobs, once. The passes' class counts are counted
    // from the records (one LDS add per chunk of positions; the masks' words are dead), lanes own
    // passes for the scan that gives each pass its first job, and each position's index is its
    // pass's first job, the jobs of larger sizes in the pass, and its rank (pl_emit_index).
    // (VP9HIP_PLAN_DBG bit 5, timing only: no epilogue; the records are then missing)
    if (!(D.dbg & 32)) {
        uint32_t *pw = S.u.b.d.rd.mk;
        for (int P = lane; P < npass; P += 64) pw[P] = 0;
        wsync();
        each_chunk<NCH>([&](auto C) {
            constexpr int c = decltype(C)::value;
            if (c * 64 < NJ && rcreg[c] != PL_REC_NONE) atomicAdd(&pw[rcreg[c] & 1023u], pl_take_val(PL_JW_TS8(jwreg[c])));
        });
        wsync();
        uint32_t carry = 0;
        for (int g = 0; g < npass; g += 64) {
            const int P = g + lane;
            const uint32_t cls = P < npass ? pw[P] : 0u, tot = pl_take_count(cls);
            const uint32_t incl = wscan_incl(tot, lane);
            const uint32_t w = pl_pass_word(pl_pass_first(carry, incl, tot), cls);
            carry += rdl(incl, 63);
            if (P < npass) {
                pw[P] = w;
                if (inb(D, (uint32_t) P, JCAP, 256u)) gpass[P] = w;
            }
        }
        wsync();
        each_chunk<NCH>([&](auto C) {
            constexpr int c = decltype(C)::value;
            const uint32_t rc = rcreg[c], jw = jwreg[c];
            if (c * 64 < NJ && rc != PL_REC_NONE) {
                const uint32_t a = S.ja[PL_JW_J(jw)], at = pl_emit_index(pw[rc & 1023u], rc, PL_JW_TS(jw));
                PJob pj;
                pj.a = a & ~JA_TRX;
                pj.roff = ((a >> 4) & 1) ? rbase + pl_resid_unit(a & 3, (a >> 12) & 15, (a >> 16) & 15, SSH, SSV) : 0u;
                if (inb(D, at, JCAP, 128u)) gjob[at] = pj;
            }
        });
    }
    if (lane == 0) {
        SBRec sr;
        sr.frame = (uint32_t) F.frame; sr.sbx = (uint16_t) G.sbx; sr.sby = (uint16_t) G.sby;
        sr.tile_x0 = (uint16_t) (G.tile_sb0 << 3);
        sr.flags = F.intra ? 0 : 1;
        D.sbs[slot] = sr;
        WGRec w;
        w.job0 = slot * JCAP; w.pass0 = slot * JCAP;
        w.njobs = (uint16_t) done; w.npass = (uint16_t) npass;
        w.sb[0] = slot;
        D.wgs[slot] = w;
    }
    PPT(11);

    // ---- cross-SB reads of level-scheduled inter frames: left / top / top-left SBs whose
    // intra units this SB's jobs read (the host's umap levels)
    uint32_t dmask = 0;
    if (F.levels && !F.intra)
        for (int j = lane; j < NJ; j += 64) {
            const uint32_t a = S.ja[j];
            const int p = a & 3, ts = (a >> 2) & 3, ux0 = (a >> 12) & 15, uy0 = (a >> 16) & 15;
            const int units = p ? CW : 16, unitsv = p ? CH : 16;
            const int fx = G.sbx * units + ux0, fy = G.sby * unitsv + uy0;
            pl_cross_reads(ux0, uy0, fx, fy, 1 << ts, (int) needs_of(a), (a & JA_TRX) ? 1 : 0, [&](int ux, int uy) {
                if (ux < 0 || uy < 0 || ux >= F.sb_cols * units) return;
                const int nx = ux / units, ny = uy / unitsv, u = ux - nx * units, v = uy - ny * unitsv;
                const uint32_t ns = F.slot0 + (uint32_t) (ny * F.sb_cols + nx);
                if (!((D.ibits[(size_t) ns * 24 + p * 8 + (v >> 1)] >> ((v & 1) * 16 + u)) & 1)) return;
                dmask |= nx < G.sbx ? (ny < G.sby ? 8u : 2u) : 4u;      // TL, L, T
            });
        }
    dmask = wor(dmask);
    PPT(12);


    // ---- the SB's intra step (diagonal phases; level phases in k_plevel) and batch totals
    if (lane == 0) {
        const uint32_t has = done > 0;
        D.sb_info[slot] = has | dmask;
        if (D.static_lists) {
            if (!has && G.mine) st |= PLS_SCHED;          // the staged step list holds every SB
            D.sb_kpos[slot] = (uint32_t) npass;           // k_psort's key (no step keys here)
        } else if (has && !(F.levels && !F.intra)) {
            const uint32_t key = F.key0 + (uint32_t) ((G.sbx - G.tile_sb0) + G.sby);
            D.sb_key[slot] = key;
            D.sb_kpos[slot] = inb(D, key, D.nkeys, 1024u) ? atomicAdd(&D.key_cnt[key], 1u) : 0u;
        }
    }
    st = wor(st);
    if (lane == 0 && st) plan_fail(D, F, st);
    PPT(13);
}
// pjob_sb and plan_sb of one SB in one wave: the intra job words stay in LDS (no round trip
// through HBM, one wave start instead of two); plan_sb's 7.2 KB (4:2:0) is all the LDS.
template <int SSH, int SSV>
__global__ __launch_bounds__(64) void k_pjplan(PlanDev D)
{
    __shared__ PlanLds<256 + 2 * (16 >> SSH) * (16 >> SSV)> S;
    const PlanFrame F = D.frames[blockIdx.y];     // by value, before any store: one batch of scalar loads
    if ((int) blockIdx.x >= F.sb_cols * F.sb_rows) return;
    const SbGeo G = sb_geo(F, blockIdx.x);        // once for both halves (tile column loop, divisions)
    const int nj = pjob_sb<SSH, SSV>(D, F, G, S.ja);
    wsync();
    plan_sb<SSH, SSV>(D, F, G, S, nj);
}

// ------------------------------------------------------------------ k_plmc
// MC units of the SB's inter blocks in decode order (vp9_mc_template.c:30-464), one wave per
// SB of the batch's inter frames. A kernel of its own: the unit emission is large code that
// keyframe batches never run, and it needs none of k_pjplan's LDS.
template <int SSH, int SSV>
__global__ __launch_bounds__(64) void k_plmc(PlanDev D)
{
    const PlanFrame &F = D.frames[blockIdx.y];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (F.intra || s >= F.sb_cols * F.sb_rows) return;
    const SbGeo G = sb_geo(F, s);
    uint32_t st = 0, b0;
    const int nb = sb_blocks(D, G.slot, b0, st);
    const uint32_t ci = D.seg_pre1[G.seg] + D.slot_pos[G.slot];
    const uint32_t base = inb(D, ci, D.cap_cntm, 16u) ? D.cntm0[ci] : 0u;
    vp9h_block b;
    bool mc = false;
    if (lane < nb) {
        b = load_block(&D.blocks[b0 + lane]);
        mc = G.mine && !b.intra && mc_refs_ok(b, F.mc);
    }
    const uint32_t n = mc ? (uint32_t) pl_mc_block(b, F.mc, 0, [](const McUnit &) {}) : 0u;
    const uint32_t incl = wscan_incl(n, lane);
    uint32_t o = base + incl - n;
    unsigned long long mbytes = 0;
    if (mc)
        pl_mc_block(b, F.mc, (uint32_t) F.frame, [&](const McUnit &m) {
            if (inb(D, o, D.cap_mcs, 512u)) D.mcs[o] = m;
            o++;
            mbytes += (unsigned long long) m.w * m.h * F.bypp * (1 + m.nref);
        });
    for (int d = 32; d; d >>= 1) mbytes += __shfl_xor(mbytes, d);
    if (lane == 0 && mbytes && inb(D, (uint32_t) F.frame, D.nframes, 2048u)) atomicAdd(&D.fbytes[2 * F.frame + 1], mbytes);
}

// ------------------------------------------------------------------ k_pllf
// The SB's loop-filter levels, masks and program (vp9block.c:1438-1452 via mask_edges,
// vp9lpf.c:31-230 via pl_lf_item): one wave per SB, 0.7 KB of LDS.
template <int SSH, int SSV>
__global__ __launch_bounds__(64) void k_pllf(PlanDev D)
{
    __shared__ uint32_t lfm[2][2][8];        // LF masks [cls][dir][row]: kinds 0..3 in bytes
    __shared__ uint8_t lfl[64];              // LF level of each 8x8
    __shared__ uint32_t prog[LF_PROG_BYTES / 4];
    const PlanFrame &F = D.frames[blockIdx.y];
    const int s = blockIdx.x, lane = threadIdx.x;
    if (!F.filter_level || s >= F.sb_cols * F.sb_rows) return;
    const SbGeo G = sb_geo(F, s);
    const int cols = F.mc.cols, rows = F.mc.rows;
    uint32_t st = 0, b0;
    const int nb = sb_blocks(D, G.slot, b0, st);
    if (lane < 32) (&lfm[0][0][0])[lane] = 0;
    lfl[lane] = 0;
    for (int i = lane; i < LF_PROG_BYTES / 4; i += 64) prog[i] = 0;
    wsync();
    if (lane < nb) {
        const vp9h_block b = load_block(&D.blocks[b0 + lane]);
        if (const int lvl = pl_lf_level(b, F.lflvl, F.filter_level)) {
            const int bw8 = pl_bwh(1, b.bs, 0), bh8 = pl_bwh(1, b.bs, 1), col7 = b.col & 7, row7 = b.row & 7;
            for (int yy = 0; yy < bh8; yy++)
                for (int xx = 0; xx < bw8; xx++)
                    if (row7 + yy < 8 && col7 + xx < 8) lfl[(row7 + yy) * 8 + col7 + xx] = (uint8_t) lvl;
            pl_lf_block_masks(b, cols, rows, SSH, SSV, [&](int cls, int d, int y, int k, unsigned v) {
                if (y < 8) atomicOr(&lfm[cls][d][y], (v & 255u) << (8 * k));
            });
        }
    }
    wsync();
    uint8_t *pg = (uint8_t *) prog;
    for (int i = lane; i < pl_lf_items(SSH, SSV); i += 64)
        pl_lf_item(i, SSH, SSV, G.sbx == 0, G.sby == 0, [&](int pos) { return (int) lfl[pos]; },
                   [&](int cls, int d, int y, int k) { return (lfm[cls][d][y] >> (8 * k)) & 255u; },
                   [&](int off, uint8_t v) { pg[off] = v; });
    wsync();
    uint32_t *g = (uint32_t *) &D.lfs[G.slot];
    for (int i = lane; i < (int) (sizeof(LFRec) / 4); i += 64)
        g[i] = i == 0 ? (uint32_t) F.frame : i == 1 ? ((uint32_t) G.sbx | (uint32_t) G.sby << 16) : prog[i - 2];
}

// ------------------------------------------------------------------ k_plevel
// Level schedule of one inter frame: an SB with intra jobs gets 1 + the highest level of
// the left / top / top-left SBs whose intra pixels it reads (0 if none), computed along
// anti-diagonals; its key is the phase's key0 + level.
__global__ __launch_bounds__(256) void k_plevel(PlanDev D)
{
    const PlanFrame &F = D.frames[blockIdx.x];
    if (!F.levels || F.intra) return;
    const int W = F.sb_cols, H = F.sb_rows;
    for (int d = 0; d < W + H - 1; d++) {
        const int x0 = pl_max(0, d - (H - 1)), x1 = pl_min(d, W - 1);
        for (int x = x0 + (int) threadIdx.x; x <= x1; x += 256) {
            const int y = d - x;
            const uint32_t slot = F.slot0 + (uint32_t) (y * W + x);
            const uint32_t info = D.sb_info[slot];
            if (!(info & 1)) continue;
            // neighbours of earlier diagonals: agent-scope loads (not the CU's L1)
            auto lv = [&](uint32_t n) {
                return (int) (__hip_atomic_load(&D.sb_key[n], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - F.key0) + 1;
            };
            int lvl = 0;
            if ((info & 2) && x > 0) lvl = pl_max(lvl, lv(slot - 1));
            if ((info & 4) && y > 0) lvl = pl_max(lvl, lv(slot - W));
            if ((info & 8) && x > 0 && y > 0) lvl = pl_max(lvl, lv(slot - W - 1));
            const uint32_t key = F.key0 + (uint32_t) lvl;
            if (!inb(D, key, D.nkeys, 4096u)) continue;
            __hip_atomic_store(&D.sb_key[slot], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            D.sb_kpos[slot] = atomicAdd(&D.key_cnt[key], 1u);
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------ k_pkeys
// One workgroup: exclusive scan of the step-key counts, and the launch summary:
// out[0] status, out[1 .. 1 + ng) count-matrix offsets at the host's gather indices,
// then nk + 1 key offsets, then 2 x nframes 64-bit byte totals.
__global__ __launch_bounds__(1024) void k_pkeys(PlanDev D, int nk, const uint32_t *gidx, int ng, int nframes,
                                                uint32_t *out)
{
    __shared__ uint32_t part[1024];
    const int t = threadIdx.x;
    const int per = (nk + 1023) / 1024, k0 = t * per, k1 = pl_min(nk, k0 + per);
    uint32_t s = 0;
    for (int k = k0; k < k1; k++) s += D.key_cnt[k];
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const uint32_t v = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    uint32_t run = part[t] - s;
    uint32_t *ko = out + 1 + ng;
    for (int k = k0; k < k1; k++) {
        D.key_off[k] = run;
        ko[k] = run;
        run += D.key_cnt[k];
    }
    if (t == 1023) { D.key_off[nk] = part[1023]; ko[nk] = part[1023]; }
    for (int i = t; i < ng; i += 1024)      // bit 31: an MC-count offset
        out[1 + i] = (gidx[i] >> 31) ? D.cntm0[gidx[i] & 0x7fffffffu] : D.cnt0[gidx[i]];
    uint32_t *fb = ko + nk + 1;
    for (int i = t; i < 2 * nframes; i += 1024) {
        fb[2 * i] = (uint32_t) D.fbytes[i];
        fb[2 * i + 1] = (uint32_t) (D.fbytes[i] >> 32);
    }
    // every frame's eob and coefficient totals as the scans saw them against its packet's
    // counts: a frame that disagrees shifts the eobs / coefficients of every later frame in
    // the batch-wide scans, so the batch fails as a whole (PLS_TOTAL names no frame)
    for (int i = t; i < nframes; i += 1024) {
        const PlanFrame &F = D.frames[i];
        const uint32_t ne = D.blk_eob0[F.blk0 + F.nblk] - D.blk_eob0[F.blk0];
        const uint32_t d0 = F.slot0, d1 = F.slot0 + (uint32_t) (F.sb_cols * F.sb_rows);
        const uint32_t nc = d1 <= D.nslots ? D.sb_coef0[d1] - D.sb_coef0[d0] : ~0u;
        if (ne != F.neob || nc != F.ncoef || D.blk_eob0[F.blk0] != F.eob0 || D.sb_coef0[d0] != F.coef0)
            atomicOr(D.status, PLS_TOTAL);
    }
    __syncthreads();
    for (int i = t; i < nframes; i += 1024) fb[4 * nframes + i] = D.fbad[i];     // per-frame status
    if (t == 0) { out[0] = D.status[0]; out[1 + ng + nk + 1 + 5 * nframes] = D.status[1]; }
}

// ------------------------------------------------------------------ k_plists
__global__ __launch_bounds__(256) void k_plists(PlanDev D)
{
    const PlanFrame &F = D.frames[blockIdx.y];
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= F.sb_cols * F.sb_rows) return;
    const uint32_t slot = F.slot0 + (uint32_t) s;
    if (!(D.sb_info[slot] & 1)) return;
    const uint32_t key = D.sb_key[slot];
    if (!inb(D, key, D.nkeys, 8192u)) return;
    const uint32_t i = D.key_off[key] + D.sb_kpos[slot];
    if (inb(D, i, D.cap_dlists, 16384u)) D.dlists[i] = slot;
}

// ------------------------------------------------------------------ k_psort
// Static step lists (keyframe batches): one workgroup per intra step, its SBs reordered by
// the length of their pass chains, longest first (sb_kpos: the SB's passes, from k_pjplan; a
// per-pass row count was measured 2 % slower in its scheduling loop for the same order).
// A k_plf launch lasts until its slowest chain ends; chains dispatched in descending length
// start the long ones first, and the short ones fill the CUs behind them (longest-processing-
// time order). Counting sort over 256 bins (passes, longest first; more than 255 share the
// last), each thread's entries held in registers between the histogram and the scatter
// (one workgroup owns the segment: every read precedes every write); segments of more than
// PSORT_PER * 1024 entries keep the staged order.
#define PSORT_PER 8
__global__ __launch_bounds__(1024) void k_psort(PlanDev D, const uint32_t *ko)
{
    __shared__ uint32_t hist[256];
    const uint32_t k = blockIdx.x, t = threadIdx.x;
    const uint32_t a = ko[k], e = ko[k + 1];
    if (e <= a + 1 || e > D.nslots || e - a > PSORT_PER * 1024u) return;
    if (t < 256) hist[t] = 0;
    __syncthreads();
    uint32_t sl[PSORT_PER], bn[PSORT_PER];
#pragma unroll
    for (int j = 0; j < PSORT_PER; j++) {
        const uint32_t i = a + t + (uint32_t) j * 1024u;
        sl[j] = i < e ? D.dlists[i] : 0u;
    }
#pragma unroll
    for (int j = 0; j < PSORT_PER; j++) {
        const uint32_t i = a + t + (uint32_t) j * 1024u;
        const uint32_t c = i < e ? D.sb_kpos[sl[j]] : 0u;
        bn[j] = 255u - (c < 255u ? c : 255u);
        if (i < e) atomicAdd(&hist[bn[j]], 1u);
    }
    __syncthreads();
    const uint32_t v = t < 256 ? hist[t] : 0u;
    for (uint32_t d = 1; d < 256; d <<= 1) {           // inclusive scan of the bins
        const uint32_t x = t < 256 && t >= d ? hist[t - d] : 0u;
        __syncthreads();
        if (t < 256) hist[t] += x;
        __syncthreads();
    }
    if (t < 256) hist[t] -= v;                         // exclusive: each bin's first position
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PSORT_PER; j++) {
        const uint32_t i = a + t + (uint32_t) j * 1024u;
        if (i < e) D.dlists[a + atomicAdd(&hist[bn[j]], 1u)] = sl[j];
    }
}

// ------------------------------------------------------------------ k_pguard
// Batches whose launch list is fixed at staging (keyframe batches, runtime "static plan"):
// their pixel kernels run after the planner without a host check of its status, so the
// frames the planner rejected (fbad != 0: the frame's packet is inconsistent) are
// neutralised here: no intra passes (WGRec), and their residual jobs write nothing but
// zeros into the spare scratch slot (slot nslots) from no coefficients. The other frames'
// records address only their own data (k_pjplan), so they reconstruct as if alone; a status
// that names no frame (PLS_BOUNDS, PLS_TOTAL) neutralises the whole batch (every WGRec, the summary's
// residual ranges). The status is re-copied into the summary (k_plists' bound checks come
// after k_pkeys), which the host reads when it next waits for the batch (vp9hip_sync /
// sync_slot: AVERROR_INVALIDDATA; vp9hip_batch_frame_status: which frames).
__global__ __launch_bounds__(256) void k_pguard(PlanDev D, uint32_t *summary, int ng)
{
    const uint32_t st = __builtin_amdgcn_readfirstlane(D.status[0]);
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) summary[0] = st;
    if (!st) return;
    const bool all = (st & (PLS_BOUNDS | PLS_TOTAL)) != 0;
    const PlanFrame &F = D.frames[blockIdx.y];
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (all && blockIdx.y == 0)
        for (int i = s; i < ng; i += (int) gridDim.x * 256) summary[1 + i] = 0;
    if (!all) {
        const uint32_t spare = D.nslots * D.rcap;        // resid scratch has nslots + 1 slots
        const uint32_t nt = gridDim.x * gridDim.y * 256u;
        for (uint32_t i = (blockIdx.y * gridDim.x + blockIdx.x) * 256u + threadIdx.x; i + 1 < D.cap_rjobs; i += nt) {
            RJob r = D.rjobs[i];
            if (r.frame >= D.nframes || !D.fbad[r.frame]) continue;
            r.coef = 0; r.dst = spare; r.eob = 0; r.nzc = 1; r.nzr = 1;
            r.ptx &= (uint8_t) ~(1u << 5);                   // scratch, not in place
            D.rjobs[i] = r;
        }
    }
    const bool bad = all || ((uint32_t) F.frame < D.nframes && D.fbad[F.frame]);
    if (!bad || s >= F.sb_cols * F.sb_rows) return;
    const uint32_t slot = F.slot0 + (uint32_t) s;
    if (slot < D.nslots) { D.wgs[slot].njobs = 0; D.wgs[slot].npass = 0; }
}

// stage 0: k_psb; 1: k_pjplan, then k_pllf (filtered frames) and k_plmc (inter frames)
template <int SSH, int SSV>
void launch_sb_kernels(hipStream_t st, const PlanDev &D, int max_sb, int nframes, int stage, int flags)
{
    const dim3 g(max_sb, nframes);
    if (stage == 0) { hipLaunchKernelGGL((k_psb<SSH, SSV>), g, dim3(64), 0, st, D); return; }
    hipLaunchKernelGGL((k_pjplan<SSH, SSV>), g, dim3(64), 0, st, D);
    if (flags & 1) hipLaunchKernelGGL((k_pllf<SSH, SSV>), g, dim3(64), 0, st, D);
    if (flags & 2) hipLaunchKernelGGL((k_plmc<SSH, SSV>), g, dim3(64), 0, st, D);
}

// ss: ss_h | ss_v << 1 (as the pixel kernels' launchers)
void launch_sb(int ss, hipStream_t st, const PlanDev &D, int max_sb, int nframes, int stage, int flags)
{
    switch (ss) {
    case 3: launch_sb_kernels<1, 1>(st, D, max_sb, nframes, stage, flags); break;
    case 1: launch_sb_kernels<1, 0>(st, D, max_sb, nframes, stage, flags); break;
    case 2: launch_sb_kernels<0, 1>(st, D, max_sb, nframes, stage, flags); break;
    default: launch_sb_kernels<0, 0>(st, D, max_sb, nframes, stage, flags); break;
    }
}

} // namespace

extern "C" {
// Temporary storage of the exclusive scans over up to n elements.
size_t vp9hip_plan_scan_bytes(size_t n)
{
    size_t b = 0;
    if (hipcub::DeviceScan::ExclusiveSum(nullptr, b, (const uint32_t *) nullptr, (uint32_t *) nullptr, (int) n) != hipSuccess) return 0;
    return b;
}

// Enqueue the device planner of a staged batch on `st`. The caller has zeroed
// status / key_cnt / fbytes and set sb_first / sb_end to 0xffffffff.
// nb / nslots / ncnt: blocks, SB slots, count-matrix entries (each array + 1 zero entry).
int vp9hip_plan_enqueue(hipStream_t st, const PlanDev *Dp, int ss, int nframes, int max_blk, int max_sb, uint32_t nb,
                        uint32_t nslots, uint32_t ncnt, int nk, const uint32_t *gidx, int ng, uint32_t *summary,
                        void *scan_tmp, size_t scan_bytes, int any_levels, int flags, int guard)
{
    const PlanDev &D = *Dp;
    if (nframes <= 0) return 0;
    hipLaunchKernelGGL(k_pblk, dim3((max_blk + 255) / 256, nframes), dim3(256), 0, st, D);
    size_t tb = scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(scan_tmp, tb, D.blk_neob, D.blk_eob0, (int) nb + 1, st) != hipSuccess) return -1;
    launch_sb(ss, st, D, max_sb, nframes, 0, 0);
    tb = scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(scan_tmp, tb, D.sb_ncoef, D.sb_coef0, (int) nslots + 1, st) != hipSuccess) return -1;
    tb = scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(scan_tmp, tb, D.cnt, D.cnt0, (int) ncnt + 1, st) != hipSuccess) return -1;
    tb = scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(scan_tmp, tb, D.cntm, D.cntm0, (int) nslots + 1, st) != hipSuccess) return -1;
    launch_sb(ss, st, D, max_sb, nframes, 1, flags);
    if (any_levels) hipLaunchKernelGGL(k_plevel, dim3(nframes), dim3(256), 0, st, D);
    if (D.static_lists && D.stat_ko && !(D.dbg & 4))             // VP9HIP_PLAN_DBG bit 2: staged order
        hipLaunchKernelGGL(k_psort, dim3(nk), dim3(1024), 0, st, D, D.stat_ko);
    hipLaunchKernelGGL(k_pkeys, dim3(1), dim3(1024), 0, st, D, nk, gidx, ng, nframes, summary);
    if (!D.static_lists) hipLaunchKernelGGL(k_plists, dim3((max_sb + 255) / 256, nframes), dim3(256), 0, st, D);
    if (guard) hipLaunchKernelGGL(k_pguard, dim3((max_sb + 255) / 256, nframes), dim3(256), 0, st, D, summary, ng);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
}
