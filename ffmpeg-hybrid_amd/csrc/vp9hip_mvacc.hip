// Accumulated motion for gfx950: k_mvacc follows every cell's first-reference vector one frame
// back and adds the parent cell's finished record, the 16-byte record of include/vp9hip.h
// ("accumulated motion"); the frames of a batch run in one launch per chain position (level), so a
// parent inside the batch is finished when its children read it, like a parent outside it.
//
// One lane per cell, a workgroup is 64 x 4 cells: a wave's own info / mv loads and its record
// store run along a row (256 / 512 / 1024 contiguous bytes; the store is one dwordx4 per lane),
// and the one dependent gather is a 16-byte read of the parent's record at the snapped cell.
//
// The measured alternative (k_mvacc<true>, tools/mvacc_bench.py) is one launch for the whole
// batch in which a lane walks: while the parent is a frame of the batch it snaps to the parent
// cell, reads that cell's info / mv and goes on from its centre; at a parent outside the batch
// one 16-byte read closes the chain. Every hop snaps to a cell centre, so the walk gives the
// recurrence's integers, and a parent's index is below the frame's own (checked here too), so it
// ends after at most nframes steps. It re-reads every ancestor's cells per descendant: equal at
// chain depth 1, 1.7x (depth 4) and 3.9x (depth 16) slower at 3840x2160.
//
// The parent differs per lane (LAST / GOLDEN / ALTREF), so the frame records are read per lane,
// 80 bytes each and at most a few KiB a batch: they stay in the vector L1 / L2, and a lane
// touches a few dwords of one per hop. No LDS, no atomics.
//
// The planes are untrusted (k_motion's input was): a reference name above 2 ends the chain, and
// every cell index is clamped to the grid before a load. No store leaves the GW x GH cells.
#include "vp9hip_mvacc.h"

namespace {

// AccFrame as dwords
enum { AF_MV = 0, AF_INFO = 2, AF_ACC = 4, AF_GW = 6, AF_GH = 7, AF_PITCH = 8, AF_SERIAL = 9, AF_PAR = 10, AF_EXT = 14,
       AF_DWORDS = 20 };
static_assert(sizeof(AccFrame) == AF_DWORDS * 4, "AccFrame layout");

__device__ __forceinline__ uint64_t af_ptr(const uint32_t *rec, int at)
{
    return (uint64_t) rec[at] | (uint64_t) rec[at + 1] << 32;
}

__device__ __forceinline__ int acc_snap(const int cell, const int v, const int n)
{
    const int p = (32 * cell + 16 + v) >> 5;     // arithmetic: floors
    return p < 0 ? 0 : p > n - 1 ? n - 1 : p;
}

// WALK: one launch, chains followed through the batch's mv / info planes; else a parent inside
// the batch is read as finished records (one launch per chain position, frames from `order`)
template <bool WALK>
__global__ __launch_bounds__(ACC_TW * ACC_TH) void k_mvacc(const AccFrame *__restrict__ frames, const uint32_t nframes,
                                                           const uint32_t *__restrict__ order, const uint32_t first)
{
    const uint32_t f = WALK ? blockIdx.z : order[first + blockIdx.z];
    if (f >= nframes) return;
    const AccFrame F = frames[f];
    const int gw = (int) F.gw, gh = (int) F.gh;
    const int c = (int) (blockIdx.x * ACC_TW + threadIdx.x), r = (int) (blockIdx.y * ACC_TH + threadIdx.y);
    if (c >= gw || r >= gh) return;
    const size_t pitch = F.pitch, own = (size_t) r * pitch + c;
    uint32_t inf = ((const uint32_t *) F.info)[own];
    uint32_t m = ((const uint32_t *) F.mv)[2 * own];             // the first reference's vector: x | y << 16
    const uint32_t *words = (const uint32_t *) frames;
    uint32_t fi = f, sx = 0, sy = 0, hops = 0, root = 0, end = VP9HIP_ACC_END_NOFIELD;
    int cc = c, cr = r;
    for (;;) {
        const uint32_t *rec = words + (size_t) fi * AF_DWORDS;
        const uint32_t i0 = inf & 0xff;
        if (i0 == 255) { root = rec[AF_SERIAL]; end = VP9HIP_ACC_END_INTRA; break; }
        const int mx = (int16_t) (m & 0xffff), my = (int16_t) (m >> 16);
        sx += (uint32_t) mx; sy += (uint32_t) my; hops++;
        if (i0 > 2) break;                                       // an unknown name: NOFIELD
        const int32_t p = (int32_t) rec[AF_PAR + i0];
        if (p < ACC_PAR_EXT) { end = (uint32_t) (-2 - p) & 0xff; break; }
        cc = acc_snap(cc, mx, gw); cr = acc_snap(cr, my, gh);
        const size_t at = (size_t) cr * pitch + cc;
        if (p == ACC_PAR_EXT || !WALK) {
            if (p != ACC_PAR_EXT && (uint32_t) p >= fi) break;
            const uint64_t plane = p == ACC_PAR_EXT ? af_ptr(rec, AF_EXT + 2 * (int) i0)
                                                    : af_ptr(words + (size_t) p * AF_DWORDS, AF_ACC);
            const uint4 q = ((const uint4 *) plane)[at];
            sx += q.x; sy += q.y; root = q.z;
            hops += q.w & 0xffff;
            end = (q.w >> 16) & 0xff;
            break;
        }
        if ((uint32_t) p >= fi) break;                           // cannot happen: parents come earlier
        fi = (uint32_t) p;
        const uint32_t *prec = words + (size_t) fi * AF_DWORDS;
        inf = ((const uint32_t *) af_ptr(prec, AF_INFO))[at];
        m = ((const uint32_t *) af_ptr(prec, AF_MV))[2 * at];
    }
    hops = hops < 65535 ? hops : 65535;
    ((uint4 *) F.acc)[own] = make_uint4(sx, sy, root, hops | end << 16);
}

} // namespace

hipError_t vp9hip_mvacc_launch(const AccFrame *frames, int nframes, int max_gw, int max_gh, int shape,
                               const uint32_t *order, const int *level_n, int nlevels, hipStream_t st)
{
    if (nframes <= 0 || max_gw <= 0 || max_gh <= 0) return hipSuccess;
    const dim3 wg(ACC_TW, ACC_TH);
    const unsigned gx = (unsigned) ((max_gw + ACC_TW - 1) / ACC_TW), gy = (unsigned) ((max_gh + ACC_TH - 1) / ACC_TH);
    if (shape == 1) {
        hipLaunchKernelGGL(k_mvacc<true>, dim3(gx, gy, (unsigned) nframes), wg, 0, st, frames, (uint32_t) nframes,
                           (const uint32_t *) nullptr, 0u);
        return hipGetLastError();
    }
    uint32_t first = 0;
    for (int l = 0; l < nlevels; first += (uint32_t) level_n[l], l++)
        if (level_n[l] > 0)
            hipLaunchKernelGGL(k_mvacc<false>, dim3(gx, gy, (unsigned) level_n[l]), wg, 0, st, frames, (uint32_t) nframes,
                               order, first);
    return hipGetLastError();
}
