// Frame metrics (vp9hip_metrics.hip): what the runtime hands the launcher.
#ifndef VP9HIP_METRICS_H
#define VP9HIP_METRICS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define MET_MAX_PAIRS 32               // pairs per launch (blockIdx.z): their buffers are kernel arguments
#define MET_WG 256                     // threads per workgroup
#define MET_TW 256                     // luma columns of a workgroup's strip: one wave per 64
#define MET_MAX_STRIPS 256             // strips of 128 rows a workgroup may take: what its u32 accumulators hold
#define MET_FILL 1024                  // workgroups a launch aims for: 4 on each of 256 CUs

struct MetArgs {
    const uint8_t *a[MET_MAX_PAIRS];   // the pairs' device buffers; b is not read without has_b
    const uint8_t *b[MET_MAX_PAIRS];
    unsigned long long *out;           // pair 0 of this launch: 3 x VP9HIP_METRIC_FIELDS records, initialised
    int32_t *cells;                    // pair 0 of this launch: mh x mw, or NULL
    int64_t off[3];                    // planes inside a buffer, bytes
    int32_t pitch[2];                  // luma / chroma pitch, bytes
    int32_t w, h, cw, ch;              // visible luma / chroma size compared
    int32_t ss_h, ss_v;
    int32_t mw, mh;                    // the cell map's size
    int32_t has_b;
    int32_t th, nsx, nstrips;          // the launcher's: strip height, strips a row, strips a frame
};

// The records of n pairs at out set to "nothing seen" (zeros, FIRST all ones), then one k_metrics
// launch over n <= MET_MAX_PAIRS pairs, both on st; hbd: 16-bit samples. Returns the launches'
// hipError_t.
hipError_t vp9hip_metrics_launch(const MetArgs &a, int hbd, int n, hipStream_t st);

#endif
