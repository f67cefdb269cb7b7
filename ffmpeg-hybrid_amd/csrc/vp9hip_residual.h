// Residual export (vp9hip_residual.hip, vp9hip_residual_host.cpp): what the runtime hands the
// launcher, and what the kernel and the host statement of the definition share: the guards of
// one tx record and the block transform around the 1-D transforms of vp9hip_resid4.h /
// vp9hip_residn.h. Everything shared is __host__ __device__ (plain inline functions for a host
// compiler). Internal to libvp9hip.
#ifndef VP9HIP_RESIDUAL_H
#define VP9HIP_RESIDUAL_H

#include <stdint.h>

#include "vp9hip_residn.h"

// One exporting frame of a batch (device memory, uploaded with the batch): its SB slots in the
// planner's arrays and the three int16 planes of its output buffer's residual block.
struct ResidFrame {
    uint64_t plane[3];                 // device planes (int16), picture geometry, 64-padded
    uint32_t pitch[2];                 // elements per row: luma, chroma
    uint32_t slot0, nsb;               // SB slots [slot0, slot0 + nsb) in raster order; 0: exports nothing
    uint32_t sb_cols, sb_rows;
    uint32_t ss_h, ss_v;
    uint32_t maxv;                     // m = 2^bpp - 1
    uint32_t pad;
};

#define RES_WG 256                     // threads per workgroup, one workgroup per SB slot
#define RES_JCAP 768                   // tx records per SB slot at most (4:4:4)

// The guards of one tx record (TxRec fields, vp9hip_plan.h): the side N of its transform (4, 8,
// 16, 32), or 0 for a record that is skipped. key = tcode * 4 + txtp with tcode 0..3 the size
// and 4 the WHT; (ux0, uy0) the position in its SB's plane in 4x4 units; coef_off the element
// offset of its first scan-order coefficient in an arena of total_coefs elements. A record that
// passes lies inside the SB's 64 >> ss square of its plane, in an SB of the frame, and reads
// eob <= N * N coefficients inside the arena.
R4_HD int resid_rec_n(uint32_t key, uint32_t eob, uint32_t p, uint32_t ux0, uint32_t uy0, uint32_t sbx, uint32_t sby,
                      uint32_t sb_cols, uint32_t sb_rows, uint32_t ss_h, uint32_t ss_v, uint64_t coef_off,
                      uint64_t total_coefs)
{
    const uint32_t tcode = key >> 2;
    if (tcode > 4 || p > 2 || (tcode == 3 && (key & 3))) return 0;      // 32x32 is DCT_DCT; the WHT has no type
    const uint32_t n = tcode == 4 ? 4u : 4u << tcode;
    const uint32_t sw = 64u >> (p ? ss_h : 0u), sh = 64u >> (p ? ss_v : 0u);
    if (ss_h > 1 || ss_v > 1 || 4 * ux0 + n > sw || 4 * uy0 + n > sh) return 0;
    if (sbx >= sb_cols || sby >= sb_rows) return 0;
    if (eob > n * n || coef_off + eob > total_coefs) return 0;
    return (int) n;
}

R4_HD int resid_clip(int32_t v, int32_t m) { return v < -m ? -m : v > m ? m : v; }

// What itxfm_add adds before its clip, for a DC-only block (vp9dsp_template.c:1165-1178)
template <class M> R4_HD int32_t resid_dc_only(int32_t c0, int bits)
{
    typedef typename M::T T;
    const T t1 = M::r14(M::in(c0) * (T) 11585);
    const int32_t tdc = (int32_t) M::r14(t1 * (T) 11585);
    return (int32_t) ((uint32_t) tdc + (1u << (bits - 1))) >> bits;
}
R4_HD constexpr int resid_bits(int n) { return n == 4 ? 4 : n == 8 ? 5 : 6; }

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>

#include "vp9hip_plan.h"

// What one k_residual launch reads (device pointers into the batch arena, by value).
struct ResidArgs {
    const ResidFrame *frames;
    const TxRec *txrec;                // jcap records per SB slot (k_psb)
    const uint32_t *sb_tn;             // per slot: records written (low 16 bits)
    const uint32_t *sb_coef0;          // per slot in packet order: first coefficient
    const void *coefs;                 // int16 (8-bit) or int32 scan-order coefficients
    uint32_t total_coefs, jcap, nslots;
};

// One launch over nframes frames: grid (max_sb, nframes), max_sb the largest nsb of the frames.
hipError_t vp9hip_residual_launch(const ResidArgs &args, int nframes, int max_sb, int hb, hipStream_t st);
#endif

#endif
