// Output conversion (vp9hip_convert.hip): what the runtime hands the launcher.
#ifndef VP9HIP_CONVERT_H
#define VP9HIP_CONVERT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/vp9hip.h"

#define CVT_MAX_FRAMES 32              // frames per launch (blockIdx.z): their buffers are kernel arguments

struct CvtArgs {
    const uint8_t *src[CVT_MAX_FRAMES];  // the frames' device buffers
    uint8_t *dst;                      // frame 0 of this launch
    int64_t frame_stride, pitch;       // destination, bytes
    int64_t plane;                     // destination bytes from one plane to the next (planar RGB: G, B; semi-planar: UV)
    int64_t src_off[3];                // source planes inside a buffer, bytes
    int32_t src_pitch[2];              // luma / chroma source pitch, bytes
    int32_t w, h, cw, ch;              // visible luma / chroma size
    int32_t c[5];                      // CY, CRV, CGU, CGV, CBU (vp9hip_out_coefs)
    int32_t shift, rnd;                // >> shift after + rnd (matrix: 2^(shift-1); RGB source: its depth reduction)
    int32_t yoff, coff;                // luma black level, chroma mid level
    int32_t maxv;                      // largest output code
    int32_t rgb;                       // source planes are G, B, R: no matrix
    int32_t msb;                       // semi-planar: samples << msb (16 - bpp above 8 bits)
    float   fscale;                    // half output: float(1.0 / maxv)
};

// What every launcher checks before it indexes its kernel table and sizes its grid.
inline bool cvt_launch_ok(int format, int n) { return format >= 0 && format <= 3 && n >= 1 && n <= CVT_MAX_FRAMES; }

// The resize kernels' workgroup: CVT_TILE_H waves, each one row of CVT_TILE_W output columns,
// and the grid that covers n frames of ow x oh with it.
constexpr int CVT_TILE_W = 128, CVT_TILE_H = 4;
inline dim3 cvt_tile_grid(int ow, int oh, int n)
{
    return dim3((ow + CVT_TILE_W - 1) / CVT_TILE_W, (oh + CVT_TILE_H - 1) / CVT_TILE_H, n);
}

// One launch over n <= CVT_MAX_FRAMES frames of `format` (VP9HIP_OUT_*); hbd: 16-bit source
// samples. Returns the launch's hipError_t.
hipError_t vp9hip_convert_launch(const CvtArgs &a, int format, int hbd, int ss_h, int ss_v, int n, hipStream_t st);

// The fused box-filter resize (vp9hip_convert_scale.hip). c.w / c.h / c.cw / c.ch stay the
// visible source size; c.pitch / c.plane / c.frame_stride describe the out_w x out_h output.
struct CvtScaleArgs {
    CvtArgs c;
    int32_t ow, oh;                    // output luma (and RGB) size
    int32_t cow, coh;                  // size the chroma planes are resampled to (RGB: ow, oh; semi-planar: OCW, OCH)
    double  rcp[2];                    // 1.0 / (w h), 1.0 / (cw ch): the quotient's estimate, corrected in the kernel
    double  rx[2], ry[2];              // 1.0 / ow, 1.0 / cow and 1.0 / oh, 1.0 / coh: the footprints' bounds, likewise
};

// One launch of k_convert_scale over n <= CVT_MAX_FRAMES frames.
hipError_t vp9hip_convert_scale_launch(const CvtScaleArgs &a, int format, int hbd, int n, hipStream_t st);

// The fused resampling with source rectangles and letterbox (vp9hip_convert_resample.hip).
// c.pitch / c.plane / c.frame_stride describe the ow x oh output; c.w / c.h / c.cw / c.ch are
// not read: each frame of the launch has rectangles of its own, in luma samples, validated by
// the runtime (inside the visible picture / the output, aligned to the subsampling).
struct CvtResampleArgs {
    CvtArgs c;
    int32_t ow, oh;                    // output luma (and RGB) size
    int32_t cow, coh;                  // the chroma planes' output grid (RGB: ow, oh; semi-planar: OCW, OCH)
    int32_t ss_h, ss_v;                // the source's chroma subsampling: a source rectangle's chroma rectangle
    int32_t ds_h, ds_v;                // the output's: a destination rectangle's (semi-planar: ss_h, ss_v; RGB: 0, 0)
    int32_t fill[3];                   // sample codes outside the destination rectangle, at the source's depth
    vp9hip_rect src_rect[CVT_MAX_FRAMES];
    vp9hip_rect dst_rect[CVT_MAX_FRAMES];
};

// One launch of k_convert_resample over n <= CVT_MAX_FRAMES frames; filter: VP9HIP_FILTER_*.
hipError_t vp9hip_convert_resample_launch(const CvtResampleArgs &a, int format, int hbd, int filter, int n, hipStream_t st);

// The fused bicubic resampling (vp9hip_convert_cubic.hip): the arguments of the resampling
// kernel and the largest sample code of the source's depth, which the result is clipped to.
struct CvtCubicArgs {
    CvtResampleArgs r;
    int32_t smax;                      // 2^bpp - 1
};

// One launch of k_convert_cubic over n <= CVT_MAX_FRAMES frames.
hipError_t vp9hip_convert_cubic_launch(const CvtCubicArgs &a, int format, int hbd, int n, hipStream_t st);

// Graded output (include/vp9hip.h "Graded output"): the tables in device memory and the matrix,
// a kernel argument of its own beside the conversion's, which stay as they are. The graded
// kernels take c.c / c.shift / c.maxv at the source's depth (out_bits = bpp) for every RGB
// format and c.fscale = float(1.0 / 65535).
struct CvtGrade {
    const uint16_t *in_lut;            // 1 << bpp entries
    const uint16_t *out_lut;           // VP9HIP_GRADE_OUT_LUT entries
    int32_t m[9];                      // row-major, 14 fractional bits
};

// The same launches through the graded instantiations; format: one of the three RGB formats.
hipError_t vp9hip_convert_resample_graded_launch(const CvtResampleArgs &a, const CvtGrade &g, int format, int hbd, int filter,
                                                 int n, hipStream_t st);
hipError_t vp9hip_convert_cubic_graded_launch(const CvtCubicArgs &a, const CvtGrade &g, int format, int hbd, int n, hipStream_t st);

// host/vp9h_grade.c: 0, or VP9HIP_EINVAL for a description vp9hip_grade_create refuses.
extern "C" int vp9hip_grade_check(const vp9hip_grade_desc *g);

#endif
