/*
 * The loop filter's LDS tile geometry and the chunk map of lf_sb (k_lf and the LF workgroups of
 * k_plf), shared by the device kernels (vp9hip_kernels.hip) and the CPU check
 * tests/c/lfmap_host_check.cpp. One statement, two executors: every function is
 * __host__ __device__.
 *
 * A tile row starts XL pixels left of the SB (16 at 8-bit, 8 at 16-bit, so chunks stay 16-byte
 * aligned) and holds XL + 64 (luma) / XL + CW (chroma) pixels; rows y = -8 .. 63 (luma) /
 * CH - 1 (chroma). The tile moves between HBM and LDS in 16-byte chunks, numbered
 *   luma 72 rows x YK, then U, then V, CR rows x CK each (NCHUNK in all),
 * and thread `lane` of NT moves chunks lane + u NT, u = 0 .. NU - 1.
 *
 * lane / YK and lane / CK are taken once per thread (LfMap::of); the chunk of every u then
 * follows from the constants u NT / YK and u NT % YK by one compare (a carry), because u is a
 * compile-time constant of the unrolled loops: no division per chunk.
 * Internal to libvp9hip.
 */
#ifndef VP9HIP_LFMAP_H
#define VP9HIP_LFMAP_H
#include <stdint.h>

#if defined(__HIPCC__)
#define LFM_HD __host__ __device__ __forceinline__
#else
#define LFM_HD inline
#endif

/* PS: bytes per pixel; SH / SV: chroma subsampling; NT: threads of the workgroup */
template <int PS, int SH, int SV, int NT> struct LfMap {
    static constexpr int CW = 64 >> SH, CH = 64 >> SV;
    static constexpr int CPX = 16 / PS;               /* pixels per chunk                      */
    static constexpr int XL = CPX;                    /* left halo loaded (8 used)             */
    static constexpr int YP = PS == 1 ? 84 : 74;      /* luma tile pitch, pixels               */
    static constexpr int UVP = CW + XL + (PS == 1 ? 4 : 2);
    static constexpr int YK = (64 + XL) / CPX;        /* chunks per luma tile row              */
    static constexpr int CK = (CW + XL) / CPX;        /* chunks per chroma tile row            */
    static constexpr int CR = CH + 8;                 /* chroma tile rows                      */
    static constexpr int NY = 72 * YK;
    static constexpr int NCHUNK = NY + 2 * CR * CK;
    static constexpr int NU = (NCHUNK + NT - 1) / NT; /* chunks per thread                     */

    /* what a thread keeps of its lane number */
    struct Lane { int lane, qy, my, qc, mc; };
    static LFM_HD Lane of(int lane)
    {
        Lane l;
        l.lane = lane;
        l.qy = (int) ((unsigned) lane / (unsigned) YK); l.my = lane - l.qy * YK;
        l.qc = (int) ((unsigned) lane / (unsigned) CK); l.mc = lane - l.qc * CK;
        return l;
    }

    /* chunk lane + u NT -> plane p, tile row r, chunk column k; false: past the last chunk
     * (p, r, k are then unspecified). */
    static LFM_HD bool chunk(const Lane &l, int u, int &p, int &r, int &k)
    {
        const int c0 = u * NT, ci = l.lane + c0;
        /* luma: (lane + c0) / YK = lane / YK + c0 / YK + carry */
        const int sy = l.my + c0 % YK, cy = sy >= YK;
        const int ry = l.qy + c0 / YK + cy, ky = sy - (cy ? YK : 0);
        /* chroma: lane + c0 - NY = lane + dq CK + dm, 0 <= dm < CK (c0 - NY may be negative) */
        const int d = c0 - NY;
        const int dq = d >= 0 ? d / CK : -((-d + CK - 1) / CK), dm = d - dq * CK;
        const int sc = l.mc + dm, cc = sc >= CK;
        const int rr = l.qc + dq + cc, kc = sc - (cc ? CK : 0);
        const int v = rr >= CR;
        /* c0 + NT <= NY / c0 >= NY fold the test for all but the one u that holds the boundary */
        const bool luma = c0 + NT <= NY || (c0 < NY && ci < NY);
        p = luma ? 0 : 1 + v;
        r = luma ? ry : rr - (v ? CR : 0);
        k = luma ? ky : kc;
        return c0 + NT <= NCHUNK || ci < NCHUNK;
    }

    /* element offset of chunk (r, k) in its plane's tile (luma pitch YP, chroma UVP) */
    static LFM_HD int tile_off(int p, int r, int k) { return r * (p ? UVP : YP) + CPX * k; }
};

#endif
