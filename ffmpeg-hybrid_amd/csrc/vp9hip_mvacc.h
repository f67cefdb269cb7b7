// Accumulated motion (vp9hip_mvacc.hip): what the runtime hands the launcher.
#ifndef VP9HIP_MVACC_H
#define VP9HIP_MVACC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define ACC_TW 64                      // cells per workgroup row: one wave, consecutive lanes along a row
#define ACC_TH 4                       // rows per workgroup: 256 threads

// AccFrame.par[k]: a frame index of the batch (below the frame's own), ACC_PAR_EXT (the finished
// records of AccFrame.ext[k]), or ACC_PAR_NONE(end) for no parent with its end code
#define ACC_PAR_EXT (-1)
#define ACC_PAR_NONE(end) (-2 - (int32_t) (end))

// One frame of a batch (device memory, uploaded with the batch, 80 bytes): its own three planes,
// grid, pitch and serial, and its parent per reference name. Every plane a record names, the
// external ones included, has `pitch` cells a row and at least gh rows; an in-batch parent has
// the frame's own grid.
struct AccFrame {
    uint64_t mv, info, acc;            // device planes: 8 / 4 / 16 bytes per cell
    uint32_t gw, gh;                   // the grid; gw == 0: the frame exports nothing
    uint32_t pitch, serial;
    int32_t par[3];
    uint32_t level;                    // chain position inside the batch: 1 + the in-batch parents' largest
    uint64_t ext[3];                   // par[k] == ACC_PAR_EXT: the parent's acc plane
};

// k_mvacc over nframes frames, grid (ceil(max_gw / ACC_TW), ceil(max_gh / ACC_TH), frames).
// shape 0: one launch per chain position, each reading only finished records; order (device)
// lists the frames to run by level, level_n[l] (host) is the number of them at level l < nlevels.
// shape 1 (the measured alternative, tools/mvacc_bench.py): one launch over all nframes frames,
// every lane walks its chain through the batch's mv / info planes; order / level_n are unused.
hipError_t vp9hip_mvacc_launch(const AccFrame *frames, int nframes, int max_gw, int max_gh, int shape,
                               const uint32_t *order, const int *level_n, int nlevels, hipStream_t st);

#endif
