/*
 * Inverse transform of one 4x4 block held in one lane's registers (k_resid's tx codes 0 and
 * 4), shared by the device kernels (vp9hip_kernels.hip: resid_wave4) and the host entry
 * vp9hip_resid4_host (the CPU check against the oracle, tests/test_resid_lane_host.py). One
 * restatement of the reference, two executors: every function is __host__ __device__.
 *
 *   M32 / M64          the transform arithmetic policies (8-bit wrap-around / int64)
 *   idct4, iadst4      vp9dsp_template.c:1202-1232
 *   iwht4              iwht4_1d (vp9dsp_template.c:1719-1748)
 *   resid4_scan        the three 4x4 scans as compile-time constants
 *   resid4_tx          scan-order coefficients -> 16 column-major residuals
 * Internal to libvp9hip.
 */
#ifndef VP9HIP_RESID4_H
#define VP9HIP_RESID4_H
#include <stdint.h>

#if defined(__HIPCC__)
#define R4_HD __host__ __device__ __forceinline__
#else
#define R4_HD inline      /* a host C++ compiler: the policies' members add their own `static` */
#endif

/* Transform arithmetic policy. 8-bit: uint32 bit patterns (defined wrap-around, identical to
 * the reference's `x * 11585U` products cast back to int) with an arithmetic rounding shift.
 * High bit depth: int64. */
struct M32 {
    typedef uint32_t T;
    static R4_HD T in(int32_t v) { return (uint32_t) v; }
    static R4_HD T r14(T v) { return (uint32_t) ((int32_t) (v + 8192u) >> 14); }
};
struct M64 {
    typedef int64_t T;
    static R4_HD T in(int32_t v) { return (int64_t) v; }
    static R4_HD T r14(T v) { return (v + 8192) >> 14; }
};

#define R4_R(x) M::r14(x)
#define R4_C(k) ((T) (k))

/* vp9dsp_template.c:1202-1216 */
template <class M> R4_HD void idct4(typename M::T *io)
{
    typedef typename M::T T;
    T t0 = R4_R((io[0] + io[2]) * R4_C(11585)), t1 = R4_R((io[0] - io[2]) * R4_C(11585));
    T t2 = R4_R(io[1] * R4_C(6270) - io[3] * R4_C(15137)), t3 = R4_R(io[1] * R4_C(15137) + io[3] * R4_C(6270));
    io[0] = t0 + t3; io[1] = t1 + t2; io[2] = t1 - t2; io[3] = t0 - t3;
}
/* vp9dsp_template.c:1218-1232 */
template <class M> R4_HD void iadst4(typename M::T *io)
{
    typedef typename M::T T;
    T t0 = R4_C(5283) * io[0] + R4_C(15212) * io[2] + R4_C(9929) * io[3];
    T t1 = R4_C(9929) * io[0] - R4_C(5283) * io[2] - R4_C(15212) * io[3];
    T t2 = R4_C(13377) * (io[0] - io[2] + io[3]);
    T t3 = R4_C(13377) * io[1];
    io[0] = R4_R(t0 + t3); io[1] = R4_R(t1 + t3); io[2] = R4_R(t2); io[3] = R4_R(t0 + t1 - t3);
}
#undef R4_R
#undef R4_C

/* iwht4_1d (vp9dsp_template.c:1719-1748), int temporaries */
R4_HD void iwht4(int32_t *io, int pass)
{
    uint32_t t0, t1, t2, t3, t4;
    if (pass == 0) { t0 = io[0] >> 2; t1 = io[3] >> 2; t2 = io[1] >> 2; t3 = io[2] >> 2; }
    else { t0 = io[0]; t1 = io[3]; t2 = io[1]; t3 = io[2]; }
    t0 += t2; t3 -= t1; t4 = (uint32_t) ((int32_t) (t0 - t3) >> 1); t1 = t4 - t1; t2 = t4 - t2; t0 -= t1; t3 += t2;
    io[0] = (int32_t) t0; io[1] = (int32_t) t1; io[2] = (int32_t) t2; io[3] = (int32_t) t3;
}

/* Position row * 4 + col of scan-order coefficient k: vp9t_scan_{default,col,row}_4x4 of
 * vp9_tables.h (txtp 1 scans by columns, 2 by rows, the lossless WHT uses the default scan)
 * as a constant expression, so an unrolled loop over k indexes registers, not memory. */
R4_HD constexpr int resid4_scan(int tcode, int txtp, int k)
{
    constexpr uint8_t def[16] = { 0x0, 0x1, 0x4, 0x5, 0x2, 0x8, 0x3, 0x6, 0xc, 0x9, 0x7, 0xa, 0xd, 0xb, 0xe, 0xf };
    constexpr uint8_t col[16] = { 0x0, 0x1, 0x2, 0x4, 0x3, 0x5, 0x6, 0x8, 0x7, 0x9, 0xa, 0xc, 0xd, 0xb, 0xe, 0xf };
    constexpr uint8_t row[16] = { 0x0, 0x4, 0x1, 0x8, 0x5, 0xc, 0x9, 0x2, 0x6, 0xd, 0x3, 0xa, 0x7, 0xe, 0xb, 0xf };
    return tcode == 4 ? def[k] : txtp == 1 ? col[k] : txtp == 2 ? row[k] : def[k];
}

/* One 4x4 block: c[k] = scan-order coefficient k (live for k < eob, anything after it),
 * TCODE 0 (DCT / ADST by TXTP: bit 0 the first pass, bit 1 the second) or 4 (WHT, TXTP 0).
 * res[x * 4 + y] = the residual of pixel (x, y), column-major like the residual scratch, not
 * yet saturated to int16: (out + 8) >> 4 for the DCT / ADST, the WHT's output as it is (the
 * lossless transform has no rounding shift). */
template <int TCODE, int TXTP, class M, typename COEF>
R4_HD void resid4_tx(const COEF (&c)[16], int eob, int32_t (&res)[16])
{
    typedef typename M::T T;
    constexpr int BITS = 4;
    if (TCODE != 4 && TXTP == 0 && eob == 1) {
        /* DC-only shortcut (vp9dsp_template.c:1165-1178) */
        const T t1 = M::r14(M::in((int32_t) c[0]) * (T) 11585);
        const int32_t tdc = (int32_t) M::r14(t1 * (T) 11585);
        const int32_t add = (int32_t) ((uint32_t) tdc + (1u << (BITS - 1))) >> BITS;
#pragma unroll
        for (int k = 0; k < 16; k++) res[k] = add;
        return;
    }
    COEF m[16], tmp[16];
#pragma unroll
    for (int k = 0; k < 16; k++) m[resid4_scan(TCODE, TXTP, k)] = k < eob ? c[k] : (COEF) 0;
    if (TCODE == 4) {
        /* lossless WHT (vp9dsp_template.c:1719-1750) */
#pragma unroll
        for (int x = 0; x < 4; x++) {
            int32_t v[4] = { m[x], m[4 + x], m[8 + x], m[12 + x] };
            iwht4(v, 0);
#pragma unroll
            for (int k = 0; k < 4; k++) tmp[x * 4 + k] = (COEF) v[k];
        }
#pragma unroll
        for (int x = 0; x < 4; x++) {
            int32_t v[4] = { tmp[x], tmp[4 + x], tmp[8 + x], tmp[12 + x] };
            iwht4(v, 1);
#pragma unroll
            for (int k = 0; k < 4; k++) res[x * 4 + k] = (int32_t) (COEF) v[k];
        }
        return;
    }
    /* first pass (type_a): column x of the block into row x */
#pragma unroll
    for (int x = 0; x < 4; x++) {
        T v[4] = { M::in(m[x]), M::in(m[4 + x]), M::in(m[8 + x]), M::in(m[12 + x]) };
        if (TXTP & 1) iadst4<M>(v); else idct4<M>(v);
#pragma unroll
        for (int k = 0; k < 4; k++) tmp[x * 4 + k] = (COEF) (int64_t) v[k];
    }
    /* second pass (type_b): column x of the transposed block */
#pragma unroll
    for (int x = 0; x < 4; x++) {
        T v[4] = { M::in(tmp[x]), M::in(tmp[4 + x]), M::in(tmp[8 + x]), M::in(tmp[12 + x]) };
        if (TXTP >> 1) iadst4<M>(v); else idct4<M>(v);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int32_t ov = (COEF) (int64_t) v[k];
            res[x * 4 + k] = (int32_t) ((uint32_t) ov + (1u << (BITS - 1))) >> BITS;
        }
    }
}

/* resid4_tx of a run-time tx code (0 or 4) and txtp */
template <class M, typename COEF>
R4_HD void resid4_block(int tcode, int txtp, const COEF (&c)[16], int eob, int32_t (&res)[16])
{
    if (tcode == 4) resid4_tx<4, 0, M, COEF>(c, eob, res);
    else if (txtp == 0) resid4_tx<0, 0, M, COEF>(c, eob, res);
    else if (txtp == 1) resid4_tx<0, 1, M, COEF>(c, eob, res);
    else if (txtp == 2) resid4_tx<0, 2, M, COEF>(c, eob, res);
    else resid4_tx<0, 3, M, COEF>(c, eob, res);
}

/* Bytes from a block's first coefficient to the end of what the kernels' wide loads may
 * read, whatever eob is: 8-bit (int16) blocks read the nine dwords from the dword at or
 * below the first coefficient, high bit depth (int32) ones sixteen dwords from it. */
#define R4_READ_SPAN16 36
#define R4_READ_SPAN32 64
#endif
