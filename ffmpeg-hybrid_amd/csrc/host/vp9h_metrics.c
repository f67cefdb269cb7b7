// Frame metrics on the host: the C statement of the definition in include/vp9hip.h ("frame
// metrics"), one sample at a time in 64-bit integers. Plain C11, no HIP: the stand-alone check
// (tests/c/metrics_host_check.c) compiles this file as it is.
#include <stddef.h>
#include <stdint.h>

#include "../../../include/vp9hip.h"

static inline int64_t met_sample(const void *plane, ptrdiff_t linesize, int hb, int x, int y)
{
    const uint8_t *row = (const uint8_t *) plane + (ptrdiff_t) y * linesize;
    return hb ? (int64_t) ((const uint16_t *) row)[x] : (int64_t) row[x];
}

int vp9hip_frame_metrics_host(const void *const a[3], const ptrdiff_t linesize_a[3],
                              const void *const b[3], const ptrdiff_t linesize_b[3],
                              int width, int height, int bpp, int ss_h, int ss_v,
                              int64_t out[24], int32_t *cells)
{
    if (!a || !linesize_a || !out || (b && !linesize_b) || (cells && !b)) return VP9HIP_EINVAL;
    if (width < 1 || width > 16384 || height < 1 || height > 16384) return VP9HIP_EINVAL;
    if (bpp != 8 && bpp != 10 && bpp != 12) return VP9HIP_EINVAL;
    if (ss_h < 0 || ss_h > 1 || ss_v < 0 || ss_v > 1) return VP9HIP_EINVAL;
    for (int p = 0; p < 3; p++)
        if (!a[p] || (b && !b[p])) return VP9HIP_EINVAL;
    const int hb = bpp > 8;
    const int mw = (width + VP9HIP_METRIC_CELL - 1) / VP9HIP_METRIC_CELL;
    const int mh = (height + VP9HIP_METRIC_CELL - 1) / VP9HIP_METRIC_CELL;
    if (cells)
        for (ptrdiff_t i = 0; i < (ptrdiff_t) mw * mh; i++) cells[i] = 0;
    for (int p = 0; p < 3; p++) {
        const int pw = p ? (width + ss_h) >> ss_h : width, ph = p ? (height + ss_v) >> ss_v : height;
        int64_t *m = out + p * VP9HIP_METRIC_FIELDS;
        for (int f = 0; f < VP9HIP_METRIC_FIELDS; f++) m[f] = 0;
        m[VP9HIP_METRIC_FIRST] = -1;
        for (int y = 0; y < ph; y++)
            for (int x = 0; x < pw; x++) {
                const int64_t va = met_sample(a[p], linesize_a[p], hb, x, y);
                m[VP9HIP_METRIC_SUM_A] += va;
                m[VP9HIP_METRIC_SUMSQ_A] += va * va;
                if (!b) continue;
                const int64_t vb = met_sample(b[p], linesize_b[p], hb, x, y);
                const int64_t d = va > vb ? va - vb : vb - va;
                m[VP9HIP_METRIC_SUM_B] += vb;
                m[VP9HIP_METRIC_SAD] += d;
                m[VP9HIP_METRIC_SSE] += d * d;
                if (d) {
                    m[VP9HIP_METRIC_NDIFF]++;
                    if (d > m[VP9HIP_METRIC_MAXDIFF]) m[VP9HIP_METRIC_MAXDIFF] = d;
                    if (m[VP9HIP_METRIC_FIRST] < 0) m[VP9HIP_METRIC_FIRST] = (int64_t) y * pw + x;
                }
                if (cells && p == 0)
                    cells[(ptrdiff_t) (y / VP9HIP_METRIC_CELL) * mw + x / VP9HIP_METRIC_CELL] += (int32_t) d;
            }
    }
    return 0;
}
