// Accumulated residual (vp9hip_warp.hip): what the runtime hands the launcher.
#ifndef VP9HIP_WARP_H
#define VP9HIP_WARP_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define WARP_MAX_PAIRS 32              // pairs per launch (blockIdx.z): their records are kernel arguments
#define WARP_TW 64                     // cells per workgroup row: one wave, consecutive lanes along a row
#define WARP_TH 4                      // luma rows per workgroup: one cell row, 256 threads

struct WarpArgs {
    const uint8_t *a[WARP_MAX_PAIRS];  // the pairs' frame buffers
    const uint8_t *b[WARP_MAX_PAIRS];
    const uint4 *acc[WARP_MAX_PAIRS];  // a's accumulated field, acc_pitch cells a row
    uint32_t serial[WARP_MAX_PAIRS];   // S_b: the serial stored with b's field
    uint8_t *dst;                      // pair 0 of this launch
    uint8_t *mask;                     // pair 0 of this launch: gh x gw bytes a pair, or NULL
    int64_t off[3];                    // planes inside a buffer, bytes
    int64_t doff[3];                   // planes inside a pair's output, bytes
    int64_t dstride;                   // bytes between pairs in dst
    int32_t pitch[2];                  // luma / chroma pitch of a and b, bytes
    int32_t w, h, cw, ch;              // visible luma / chroma size
    int32_t ss_h, ss_v;
    int32_t gw, gh, acc_pitch;         // the field's grid and its pitch in cells
};

// One k_acc_warp launch over n <= WARP_MAX_PAIRS pairs on st; hbd: 16-bit samples; mode
// VP9HIP_WARP_NEAREST / _BILINEAR, output VP9HIP_WARP_RESIDUAL / _PICTURE. Returns the launch's
// hipError_t.
hipError_t vp9hip_warp_launch(const WarpArgs &a, int hbd, int mode, int output, int n, hipStream_t st);

#endif
