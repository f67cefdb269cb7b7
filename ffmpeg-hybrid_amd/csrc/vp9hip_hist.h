// Frame histograms (vp9hip_hist.hip): what the runtime hands the launcher.
#ifndef VP9HIP_HIST_H
#define VP9HIP_HIST_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define HIST_MAX_FRAMES 32             // frames per launch (blockIdx.z): their buffers and rectangles are kernel arguments
#define HIST_WG 256                    // threads per workgroup
#define HIST_FILL 1024                 // workgroups a launch aims for: 4 on each of 256 CUs, as k_metrics
#define HIST_MIN_BLOCKS 8              // blocks of 64 x 16 a wave should at least have before a frame gets another workgroup

struct HistArgs {
    const uint8_t *src[HIST_MAX_FRAMES];   // the frames' device buffers
    vp9hip_rect rect[HIST_MAX_FRAMES];     // their luma rectangles, validated by the runtime
    int32_t *out;                      // frame 0 of this launch: C x B counts, zeroed by the launcher
    int64_t off[3];                    // planes inside a buffer, bytes
    int32_t pitch[2];                  // luma / chroma pitch, bytes
    int32_t ss_h, ss_v;
    int32_t what;                      // VP9HIP_HIST_*
    int32_t bins_log2, bpp;
    // VP9HIP_HIST_RGBM: the conversion's matrix at the source's depth, the fields of CvtArgs that cvt_rgb reads
    int32_t c[5];
    int32_t shift, rnd, yoff, coff, rgb;
};

// The n x C x B counts at out set to zero (a memset node on st), then one launch over
// n <= HIST_MAX_FRAMES frames, both on st; hbd: 16-bit samples. Returns the hipError_t.
hipError_t vp9hip_hist_launch(const HistArgs &a, int hbd, int n, hipStream_t st);

#endif
