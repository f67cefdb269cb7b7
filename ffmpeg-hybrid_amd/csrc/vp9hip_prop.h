// Accumulated propagation (vp9hip_prop.hip): what the runtime hands the launcher.
#ifndef VP9HIP_PROP_H
#define VP9HIP_PROP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define PROP_MAX_PAIRS 32              // pairs per launch (blockIdx.z): their records are kernel arguments
#define PROP_TW 64                     // NCHW: lanes of a workgroup row, one wave along fx
#define PROP_TH 4                      // NCHW: feature rows per workgroup, 256 threads
#define PROP_CCHUNK 8                  // NCHW: channels a lane carries its sample through (a grid dimension)
#define PROP_WG 256                    // NHWC: threads per workgroup

struct PropArgs {
    const uint4 *acc[PROP_MAX_PAIRS];  // the pairs' accumulated fields, acc_pitch cells a row
    const uint8_t *src[PROP_MAX_PAIRS];// the pairs' source items
    uint32_t serial[PROP_MAX_PAIRS];   // S: the root's serial
    uint8_t *dst;                      // pair 0 of this launch, `item` bytes a pair
    uint8_t *valid;                    // pair 0 of this launch: fh x fw bytes a pair, or NULL
    uint64_t fill;                     // the fill element repeated over 8 bytes
    int64_t item;                      // bytes of an item
    double rw, rh, rfw, rfh;           // 1 / (2 w), 1 / (2 h), 1 / (2 FW), 1 / (2 FH)
    int32_t w, h, fw, fh, c;
    int32_t gw, gh, acc_pitch;         // the field's grid and its pitch in cells
    int32_t keep;
};

// One launch over n <= PROP_MAX_PAIRS pairs on st: esize the element's bytes, layout
// VP9HIP_PROP_NCHW / _NHWC, mode VP9HIP_WARP_NEAREST / _BILINEAR (esize 2 only). Returns the
// launch's hipError_t.
hipError_t vp9hip_prop_launch(const PropArgs &a, int esize, int layout, int mode, int n, hipStream_t st);

#endif
