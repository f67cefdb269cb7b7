// Motion tensors at model size (vp9hip_motion_scale.hip): what the runtime hands the launcher.
#ifndef VP9HIP_MOTION_SCALE_H
#define VP9HIP_MOTION_SCALE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vp9hip_convert.h"

#define MSC_MAX_FRAMES CVT_MAX_FRAMES  // frames per launch (blockIdx.z): their fields are kernel arguments

struct MotionScaleArgs {
    const uint8_t *src[MSC_MAX_FRAMES]; // the frames' mv planes (coded) or acc planes (acc)
    uint8_t *dst;                      // frame 0 of this launch
    int64_t frame_stride, pitch;       // destination, bytes
    int64_t plane;                     // destination bytes from one plane to the next (pitch OH)
    int64_t info_off;                  // coded: bytes from a field's mv plane to its info plane
    int32_t src_pitch;                 // cells a source row, even
    int32_t gw, gh;                    // the fields' grid, gw even: no cell at or beyond it is loaded
    int32_t w, h;                      // visible size
    int32_t ow, oh;                    // output size
    float   kx, ky;                    // half output: float(OW / (8.0 w)), float(OH / (8.0 h))
    double  rcp;                       // 1.0 / (w h): the quotient's estimate, corrected in the kernel
    double  rx, ry;                    // 1.0 / (4 ow), 1.0 / (4 oh): the cell footprints' bounds, likewise
};

// One launch of k_motion_scale over n <= MSC_MAX_FRAMES frames; source / format: VP9HIP_MVT_*,
// planes 2 or 3.
hipError_t vp9hip_motion_scale_launch(const MotionScaleArgs &a, int source, int format, int planes, int n, hipStream_t st);

#endif
