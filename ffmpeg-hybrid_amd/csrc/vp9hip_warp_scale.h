// Accumulated residual at model size (vp9hip_warp_scale.hip): what the runtime hands the launcher.
#ifndef VP9HIP_WARP_SCALE_H
#define VP9HIP_WARP_SCALE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vp9hip_convert.h"

#define WSC_MAX_PAIRS 32               // pairs per launch (blockIdx.z): their records are kernel arguments

struct WarpScaleArgs {
    const uint8_t *a[WSC_MAX_PAIRS];   // the pairs' frame buffers
    const uint8_t *b[WSC_MAX_PAIRS];
    const uint4 *acc[WSC_MAX_PAIRS];   // a's accumulated field, acc_pitch cells a row
    uint32_t serial[WSC_MAX_PAIRS];    // S_b: the serial stored with b's field
    uint8_t *dst;                      // pair 0 of this launch
    int64_t frame_stride, pitch;       // destination, bytes
    int64_t plane;                     // destination bytes from one plane to the next (pitch OH)
    int64_t off[3];                    // source planes inside a buffer, bytes
    int32_t src_pitch[2];              // luma / chroma pitch of a and b, bytes
    int32_t w, h, cw, ch;              // visible luma / chroma size
    int32_t ss_h, ss_v;
    int32_t gw, gh, acc_pitch;         // the field's grid and its pitch in cells
    int32_t ow, oh;                    // output size, of every plane
    int32_t cov;                       // a fourth plane: the coverage
    int32_t c[5];                      // CY, CRV, CGU, CGV, CBU (vp9hip_out_coefs at out_bits = bpp)
    int32_t shift, rnd;                // >> shift after + rnd = 2^(shift-1)
    int32_t maxv;                      // m = 2^bpp - 1: the RGB formats clip to [-m, m]
    int32_t rgb;                       // source planes are G, B, R: no matrix
    float   fscale;                    // half output: float(1.0 / m)
    double  rcp[2];                    // 1.0 / (w h), 1.0 / (cw ch): the quotient's estimate, corrected in the kernel
    double  rx, ry;                    // 1.0 / ow, 1.0 / oh: the footprints' bounds, likewise
};

// One launch of k_acc_warp_scale over n <= WSC_MAX_PAIRS pairs on st; hbd: 16-bit samples; mode
// VP9HIP_WARP_NEAREST / _BILINEAR, format VP9HIP_RESID_*. Returns the launch's hipError_t.
hipError_t vp9hip_warp_scale_launch(const WarpScaleArgs &a, int hbd, int mode, int format, int n, hipStream_t st);

#endif
