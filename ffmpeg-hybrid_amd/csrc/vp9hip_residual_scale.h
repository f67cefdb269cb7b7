// Residual tensors at model size (vp9hip_residual_scale.hip): what the runtime hands the launcher.
#ifndef VP9HIP_RESIDUAL_SCALE_H
#define VP9HIP_RESIDUAL_SCALE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vp9hip_convert.h"

#define RSC_MAX_FRAMES CVT_MAX_FRAMES  // frames per launch (blockIdx.z): their fields are kernel arguments

struct ResidScaleArgs {
    const uint8_t *src[RSC_MAX_FRAMES]; // the frames' residual fields (three int16 planes each)
    uint8_t *dst;                      // frame 0 of this launch
    int64_t frame_stride, pitch;       // destination, bytes
    int64_t plane;                     // destination bytes from one plane to the next (pitch OH)
    int64_t src_off[3];                // source planes inside a field, bytes
    int32_t src_pitch[2];              // luma / chroma source pitch, bytes
    int32_t w, h, cw, ch;              // visible luma / chroma size
    int32_t ow, oh;                    // output size, of all three planes
    int32_t c[5];                      // CY, CRV, CGU, CGV, CBU (vp9hip_out_coefs at out_bits = bpp)
    int32_t shift, rnd;                // >> shift after + rnd = 2^(shift-1)
    int32_t maxv;                      // m = 2^bpp - 1: the RGB formats clip to [-m, m]
    int32_t rgb;                       // source planes are G, B, R: no matrix
    float   fscale;                    // half output: float(1.0 / m)
    double  rcp[2];                    // 1.0 / (w h), 1.0 / (cw ch): the quotient's estimate, corrected in the kernel
    double  rx, ry;                    // 1.0 / ow, 1.0 / oh: the footprints' bounds, likewise
};

// One launch of k_residual_scale over n <= RSC_MAX_FRAMES frames; format: VP9HIP_RESID_*.
hipError_t vp9hip_residual_scale_launch(const ResidScaleArgs &a, int format, int n, hipStream_t st);

#endif
