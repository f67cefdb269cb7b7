// Motion export (vp9hip_motion.hip): what the runtime hands the launcher.
#ifndef VP9HIP_MOTION_H
#define VP9HIP_MOTION_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define MOT_WG 256                     // threads per workgroup = blocks per workgroup

// One exporting frame of a batch (device memory, uploaded with the batch): its blocks inside the
// batch's block array, its 8x8 grid, and the two side planes of its output buffer.
struct MotionFrame {
    uint32_t blk0, nblk;               // blocks [blk0, blk0 + nblk) of the batch's array
    uint32_t cols8, rows8;             // (width + 7) >> 3, (height + 7) >> 3: GW = 2 cols8, GH = 2 rows8
    uint64_t mv, info;                 // device planes: 8 / 4 bytes per cell
    uint32_t pitch;                    // cells per plane row, >= GW (the planes hold >= GH rows)
    uint32_t pad;
};

// One k_motion launch over nframes frames: grid (ceil(max_blk / MOT_WG), nframes); frames /
// blocks are device pointers (blocks 4-byte aligned). shape 0: the flat-task kernel; 1: one
// thread per block looping over its cells (the measured alternative, tools/motion_bench.py).
hipError_t vp9hip_motion_launch(const MotionFrame *frames, int nframes, int max_blk, const vp9h_block *blocks,
                                int shape, hipStream_t st);

#endif
