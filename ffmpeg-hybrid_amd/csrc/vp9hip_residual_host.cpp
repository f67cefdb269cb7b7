// vp9hip_residual_host: the residual field of one packet on the host, the C++ statement of the
// definition in include/vp9hip.h ("residual export") over the packet alone. k_residual
// (vp9hip_residual.hip) computes the same planes from the planner's tx records with the same 1-D
// transforms (vp9hip_resid4.h, vp9hip_residn.h) and the same record guards (vp9hip_residual.h);
// this is what the tests compare it with and what the sanitizer build runs
// (tests/c/residual_host_check.cpp). No device code, no HIP.
#include <stddef.h>
#include <string.h>

#include "../../include/vp9hip.h"
#include "vp9_tables.h"
#include "vp9hip_residual.h"

namespace {

// width / height of a block size in 4-pixel units (ff_vp9_bwh_tab[0], vp9data.c:25-38)
const uint8_t bs_w4[VP9H_N_BS] = { 16, 16, 8, 8, 8, 4, 4, 4, 2, 2, 2, 1, 1 };
const uint8_t bs_h4[VP9H_N_BS] = { 16, 8, 16, 8, 4, 8, 4, 2, 4, 2, 1, 2, 1 };
// ff_vp9_intra_txfm_type (vp9data.c:437-452), intra modes 0..9
const uint8_t intra_txtp[10] = { 2, 1, 0, 0, 3, 2, 1, 2, 1, 3 };

const int16_t *scan_of(int n, int txtp)
{
    if (n == 8) return txtp == 1 ? vp9t_scan_col_8x8 : txtp == 2 ? vp9t_scan_row_8x8 : vp9t_scan_default_8x8;
    if (n == 16) return txtp == 1 ? vp9t_scan_col_16x16 : txtp == 2 ? vp9t_scan_row_16x16 : vp9t_scan_default_16x16;
    return vp9t_scan_default_32x32;
}

// One N x N block (N >= 8): res[y * N + x], before the clip
template <int N, class M, typename COEF> void block_n(int txtp, int eob, const COEF *src, int32_t *res)
{
    typedef typename M::T T;
    constexpr int BITS = resid_bits(N);
    if (eob == 1 && txtp == 0) {
        const int32_t add = resid_dc_only<M>((int32_t) src[0], BITS);
        for (int k = 0; k < N * N; k++) res[k] = add;
        return;
    }
    static thread_local COEF cb[N * N], tmp[N * N];
    const int16_t *scan = scan_of(N, txtp);
    for (int k = 0; k < N * N; k++) cb[k] = 0;
    for (int k = 0; k < eob; k++) cb[scan[k]] = src[k];
    T v[N];
    for (int x = 0; x < N; x++) {                  // first pass (type_a): column x into row x
        for (int k = 0; k < N; k++) v[k] = M::in(cb[k * N + x]);
        tx1n<N, M>(v, txtp & 1);
        for (int k = 0; k < N; k++) tmp[x * N + k] = (COEF) (int64_t) v[k];
    }
    for (int x = 0; x < N; x++) {                  // second pass (type_b): column x of the transposed block
        for (int k = 0; k < N; k++) v[k] = M::in(tmp[k * N + x]);
        tx1n<N, M>(v, txtp >> 1);
        for (int k = 0; k < N; k++) {
            const int32_t ov = (COEF) (int64_t) v[k];
            res[k * N + x] = (int32_t) ((uint32_t) ov + (1u << (BITS - 1))) >> BITS;
        }
    }
}

template <class M, typename COEF> void block_any(int n, int tcode, int txtp, int eob, const COEF *src, int32_t *res)
{
    if (n == 4) {
        COEF c[16];
        int32_t r4[16];
        for (int k = 0; k < 16; k++) c[k] = k < eob ? src[k] : (COEF) 0;
        resid4_block<M, COEF>(tcode, txtp, c, eob, r4);
        for (int x = 0; x < 4; x++)
            for (int y = 0; y < 4; y++) res[y * 4 + x] = r4[x * 4 + y];
    } else if (n == 8) block_n<8, M, COEF>(txtp, eob, src, res);
    else if (n == 16) block_n<16, M, COEF>(txtp, eob, src, res);
    else block_n<32, M, COEF>(txtp, eob, src, res);
}

// The walk of the packet's tx blocks (the enumeration of vp9h_frame.eobs); with `write` the
// blocks are transformed and stored, without it only checked.
int walk(const vp9h_frame *f, int16_t *const planes[3], const ptrdiff_t pitch[3], const int cw[3], const int ch[3], bool write)
{
    const int cols = (f->width + 7) >> 3, rows = (f->height + 7) >> 3;
    const uint32_t sb_cols = (uint32_t) (cols + 7) >> 3, sb_rows = (uint32_t) (rows + 7) >> 3;
    const int32_t m = (1 << f->bpp) - 1;
    uint64_t ne = 0, nc = 0;
    static thread_local int32_t res[32 * 32];
    for (uint32_t bi = 0; bi < f->nblocks; bi++) {
        const vp9h_block &b = f->blocks[bi];
        if (b.bs >= VP9H_N_BS || b.row >= rows || b.col >= cols || b.tx > 3 || b.uvtx > 3) return VP9HIP_EINVALIDDATA;
        if (f->lossless && (b.tx || b.uvtx)) return VP9HIP_EINVALIDDATA;
        if (b.skip) continue;
        const int w4 = bs_w4[b.bs] < 2 ? 2 : bs_w4[b.bs], h4 = bs_h4[b.bs] < 2 ? 2 : bs_h4[b.bs];   // below 8x8: the 8x8 unit
        const int end_x = 2 * (cols - b.col) < w4 ? 2 * (cols - b.col) : w4;
        const int end_y = 2 * (rows - b.row) < h4 ? 2 * (rows - b.row) : h4;
        for (int p = 0; p < 3; p++) {
            const int sh = p ? f->ss_h : 0, sv = p ? f->ss_v : 0;
            const int txs = p ? b.uvtx : b.tx, step = 1 << txs, n = 4 << txs;
            const int ex = end_x >> sh, ey = end_y >> sv;
            const int bx = b.col * 8 >> sh, by = b.row * 8 >> sv;
            for (int y = 0; y < ey; y += step)
                for (int x = 0; x < ex; x += step) {
                    if (ne >= f->neobs) return VP9HIP_EINVALIDDATA;
                    const uint32_t eob = f->eobs[ne++];
                    int txtp = 0;
                    if (b.intra && !p && txs < 3) {
                        const int mode = b.mode[b.bs > VP9H_BS_8x8 && b.tx == 0 ? (y * 2 + x) & 3 : 0];
                        if (mode > 9) return VP9HIP_EINVALIDDATA;
                        txtp = intra_txtp[mode];
                    }
                    const int tcode = f->lossless ? 4 : txs;
                    const int x0 = bx + 4 * x, y0 = by + 4 * y;
                    const int sw = 64 >> sh, shh = 64 >> sv;
                    // the guards the kernel applies to the planner's record of this tx block
                    const int gn = resid_rec_n((uint32_t) (tcode * 4 + txtp), eob, (uint32_t) p, (uint32_t) (x0 % sw) >> 2,
                                               (uint32_t) (y0 % shh) >> 2, (uint32_t) (x0 / sw), (uint32_t) (y0 / shh), sb_cols,
                                               sb_rows, f->ss_h, f->ss_v, nc, f->ncoefs);
                    if (gn != n) return VP9HIP_EINVALIDDATA;
                    const uint64_t c0 = nc;
                    nc += eob;
                    if (!write || !eob) continue;
                    if (f->bpp == 8) block_any<M32, int16_t>(n, tcode, txtp, (int) eob, (const int16_t *) f->coefs + c0, res);
                    else block_any<M64, int32_t>(n, tcode, txtp, (int) eob, (const int32_t *) f->coefs + c0, res);
                    for (int yy = 0; yy < n && y0 + yy < ch[p]; yy++)       // samples outside the coded area are dropped
                        for (int xx = 0; xx < n && x0 + xx < cw[p]; xx++)
                            planes[p][(ptrdiff_t) (y0 + yy) * pitch[p] + x0 + xx] = (int16_t) resid_clip(res[yy * n + xx], m);
                }
        }
    }
    return ne == f->neobs && nc == f->ncoefs ? 0 : VP9HIP_EINVALIDDATA;
}

} // namespace

extern "C" int vp9hip_residual_host(const vp9h_frame *pkt, int16_t *const planes[3], const ptrdiff_t pitch[3], const int rows[3])
{
    if (!pkt || !planes || !pitch || !rows || pkt->width <= 0 || pkt->height <= 0 || pkt->width > 16384 || pkt->height > 16384)
        return VP9HIP_EINVAL;
    if ((pkt->bpp != 8 && pkt->bpp != 10 && pkt->bpp != 12) || pkt->ss_h > 1 || pkt->ss_v > 1) return VP9HIP_EINVAL;
    if ((pkt->nblocks && !pkt->blocks) || (pkt->neobs && !pkt->eobs) || (pkt->ncoefs && !pkt->coefs)) return VP9HIP_EINVAL;
    int cw[3], ch[3];
    for (int p = 0; p < 3; p++) {
        cw[p] = 8 * ((pkt->width + 7) >> 3) >> (p ? pkt->ss_h : 0);
        ch[p] = 8 * ((pkt->height + 7) >> 3) >> (p ? pkt->ss_v : 0);
        if (!planes[p] || pitch[p] < cw[p] || rows[p] < ch[p]) return VP9HIP_EINVAL;
    }
    // every block, eob and coefficient index is checked before the first store
    if (const int r = walk(pkt, planes, pitch, cw, ch, false)) return r;
    for (int p = 0; p < 3; p++)
        for (int y = 0; y < ch[p]; y++) memset(planes[p] + (ptrdiff_t) y * pitch[p], 0, (size_t) cw[p] * 2);
    return walk(pkt, planes, pitch, cw, ch, true);
}
