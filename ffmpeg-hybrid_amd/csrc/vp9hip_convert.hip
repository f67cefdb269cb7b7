// Output conversion kernel for gfx950: the decoder's pitched planar YUV planes -> semi-planar
// (NV12 / P010 style), packed RGB24, planar RGB u8 or planar RGB half, n frames per launch.
//
// A pure streaming kernel (no reuse, no LDS): each lane converts a run of 16 pixels of two
// luma rows (one row without vertical subsampling), so the chroma of a 4:2:0 pair is loaded
// once. Loads are 16 B (8 B for 8 chroma bytes); the source planes are padded to 64 samples,
// so a load may pass the visible width but not the plane. Stores are 16 B where the
// destination row is 16-byte aligned (a run starts at a multiple of 16 bytes in its row for
// every format, so this is uniform per row), 4 B where it is 4-byte aligned, else per
// element; a run that crosses the right edge stores per element up to the width. Nothing is
// written outside the visible rows and columns.
//
// The arithmetic is the integer definition of include/vp9hip.h / DESIGN.md "Output
// conversion": nearest chroma sample, coefficients with `shift` fractional bits as kernel
// arguments, round half up, clip.
#include "vp9hip_convert_dev.h"

#include <array>
#include <utility>

namespace {

// n samples (8 or 16) of 1 or 2 bytes at p (aligned to their total size, at most 16 B per load)
template <int HBD, int N>
__device__ __forceinline__ void load_run(const uint8_t *p, int (&s)[N])
{
    constexpr int NB = N * (HBD ? 2 : 1);
    uint32_t w[NB / 4];
    if constexpr (NB == 8) {
        const uint2 v = *reinterpret_cast<const uint2 *>(p);
        w[0] = v.x; w[1] = v.y;
    } else {
#pragma unroll
        for (int i = 0; i < NB / 16; i++) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    }
#pragma unroll
    for (int i = 0; i < N; i++)
        s[i] = HBD ? (int) (w[i / 2] >> (16 * (i & 1)) & 0xffff) : (int) (w[i / 4] >> (8 * (i & 3)) & 0xff);
}

// The first nbytes of the NW words w to p. A whole run: 16-byte stores if p is 16-byte
// aligned, 4-byte stores if it is 4-byte aligned. Otherwise, and for a run cut at the right
// edge, element by element (ELEM bytes each; p is ELEM-aligned).
template <int NW, int ELEM>
__device__ __forceinline__ void store_run(uint8_t *p, const uint32_t (&w)[NW], int nbytes)
{
    static_assert(NW % 4 == 0, "whole 16-byte stores");
    const uintptr_t a = (uintptr_t) p;
    if (nbytes == NW * 4 && !(a & 3)) {
        if (!(a & 15)) {
#pragma unroll
            for (int i = 0; i < NW / 4; i++)
                reinterpret_cast<uint4 *>(p)[i] = make_uint4(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < NW; i++) reinterpret_cast<uint32_t *>(p)[i] = w[i];
        }
        return;
    }
    if constexpr (ELEM == 2) {
#pragma unroll
        for (int i = 0; i < NW * 2; i++)
            if (2 * i < nbytes) reinterpret_cast<uint16_t *>(p)[i] = (uint16_t) (w[i / 2] >> (16 * (i & 1)));
    } else {
#pragma unroll
        for (int i = 0; i < NW * 4; i++)
            if (i < nbytes) p[i] = (uint8_t) (w[i / 4] >> (8 * (i & 3)));
    }
}

// FMT: VP9HIP_OUT_*; HBD: 16-bit source samples; SSH / SSV: chroma subsampling.
template <int FMT, int HBD, int SSH, int SSV>
__global__ __launch_bounds__(256) void k_convert(const CvtArgs a)
{
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 16;
    const int y0 = (blockIdx.y * 4 + threadIdx.y) << SSV;
    if (x0 >= a.w || y0 >= a.h) return;
    constexpr int BS = HBD ? 2 : 1;        // source bytes per sample
    constexpr int NC = 16 >> SSH;          // chroma samples under the run
    const uint8_t *src = a.src[blockIdx.z];
    uint8_t *dst = a.dst + (int64_t) blockIdx.z * a.frame_stride;
    const int npx = min(16, a.w - x0);
    const int cx0 = x0 >> SSH, cy = y0 >> SSV;

    int U[NC], V[NC];
    {
        const int64_t co = (int64_t) cy * a.src_pitch[1] + (int64_t) cx0 * BS;
        load_run<HBD, NC>(src + a.src_off[1] + co, U);
        load_run<HBD, NC>(src + a.src_off[2] + co, V);
    }
    if constexpr (FMT == VP9HIP_OUT_SEMIPLANAR) {      // the UV row of this chroma row
        constexpr int NW = NC * 2 * BS / 4;
        uint32_t w[NW];
#pragma unroll
        for (int i = 0; i < NW; i++) {
            if constexpr (HBD) w[i] = (uint32_t) (U[i] << a.msb) | (uint32_t) (V[i] << a.msb) << 16;
            else w[i] = (uint32_t) U[2 * i] | (uint32_t) V[2 * i] << 8 | (uint32_t) U[2 * i + 1] << 16 | (uint32_t) V[2 * i + 1] << 24;
        }
        store_run<NW, BS>(dst + a.plane + (int64_t) cy * a.pitch + (int64_t) cx0 * 2 * BS, w, min(NC, a.cw - cx0) * 2 * BS);
    }
#pragma unroll
    for (int r = 0; r <= SSV; r++) {
        const int y = y0 + r;
        if (y >= a.h) break;
        int Y[16];
        load_run<HBD, 16>(src + a.src_off[0] + (int64_t) y * a.src_pitch[0] + (int64_t) x0 * BS, Y);
        uint8_t *row = dst + (int64_t) y * a.pitch;
        if constexpr (FMT == VP9HIP_OUT_SEMIPLANAR) {
            constexpr int NW = 16 * BS / 4;
            uint32_t w[NW];
#pragma unroll
            for (int i = 0; i < NW; i++) {
                if constexpr (HBD) w[i] = (uint32_t) (Y[2 * i] << a.msb) | (uint32_t) (Y[2 * i + 1] << a.msb) << 16;
                else w[i] = (uint32_t) Y[4 * i] | (uint32_t) Y[4 * i + 1] << 8 | (uint32_t) Y[4 * i + 2] << 16 | (uint32_t) Y[4 * i + 3] << 24;
            }
            store_run<NW, BS>(row + (int64_t) x0 * BS, w, npx * BS);
        } else {
            int R[16], G[16], B[16];
#pragma unroll
            for (int i = 0; i < 16; i++) cvtdev::cvt_rgb(a, Y[i], U[i >> SSH], V[i >> SSH], R[i], G[i], B[i]);
            if constexpr (FMT == VP9HIP_OUT_RGB24) {
                uint32_t w[12] = {};
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    w[(3 * i) / 4] |= (uint32_t) R[i] << (8 * ((3 * i) & 3));
                    w[(3 * i + 1) / 4] |= (uint32_t) G[i] << (8 * ((3 * i + 1) & 3));
                    w[(3 * i + 2) / 4] |= (uint32_t) B[i] << (8 * ((3 * i + 2) & 3));
                }
                store_run<12, 1>(row + (int64_t) x0 * 3, w, npx * 3);
            } else if constexpr (FMT == VP9HIP_OUT_RGBP_U8) {
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    const int (&C)[16] = p == 0 ? R : p == 1 ? G : B;
                    uint32_t w[4];
#pragma unroll
                    for (int i = 0; i < 4; i++)
                        w[i] = (uint32_t) C[4 * i] | (uint32_t) C[4 * i + 1] << 8 | (uint32_t) C[4 * i + 2] << 16 | (uint32_t) C[4 * i + 3] << 24;
                    store_run<4, 1>(row + p * a.plane + x0, w, npx);
                }
            } else {                                   // half: one float multiply, round to nearest even
                // (pairs compile to v_cvt_pk_f16_f32 of two float products: the two roundings
                // of the definition without cvtdev::to_half's asm)
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    const int (&C)[16] = p == 0 ? R : p == 1 ? G : B;
                    uint32_t w[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const _Float16 lo = (_Float16) ((float) C[2 * i] * a.fscale), hi = (_Float16) ((float) C[2 * i + 1] * a.fscale);
                        w[i] = (uint32_t) __builtin_bit_cast(uint16_t, lo) | (uint32_t) __builtin_bit_cast(uint16_t, hi) << 16;
                    }
                    store_run<8, 2>(row + p * a.plane + (int64_t) x0 * 2, w, npx * 2);
                }
            }
        }
    }
}

typedef void (*KFn)(const CvtArgs);
// index: format << 3 | hbd << 2 | ss_h << 1 | ss_v
template <size_t... I>
constexpr std::array<KFn, sizeof...(I)> kernel_table(std::index_sequence<I...>)
{
    return { { k_convert<(int) (I >> 3), (int) (I >> 2 & 1), (int) (I >> 1 & 1), (int) (I & 1)>... } };
}
const std::array<KFn, 32> g_kernels = kernel_table(std::make_index_sequence<32>());

}  // namespace

hipError_t vp9hip_convert_launch(const CvtArgs &a, int format, int hbd, int ss_h, int ss_v, int n, hipStream_t st)
{
    if (!cvt_launch_ok(format, n)) return hipErrorInvalidValue;
    const int runs = (a.w + 15) / 16, rows = (a.h + ss_v) >> ss_v;
    const dim3 grid((runs + 63) / 64, (rows + 3) / 4, n), block(64, 4, 1);
    hipLaunchKernelGGL(g_kernels[format << 3 | !!hbd << 2 | !!ss_h << 1 | !!ss_v], grid, block, 0, st, a);
    return hipGetLastError();
}
