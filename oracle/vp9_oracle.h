/*
 * ORACLE — test infrastructure only. A scalar CPU restatement of the reference
 * libavcodec VP9 pixel path (vp9recon.c, vp9_mc_template.c, vp9lpf.c, the
 * reconstruction half of vp9block.c and vp9dsp_template.c) that consumes the same
 * pass-1 frame packet (include/vp9hip.h) as the HIP path. Only tests/,
 * __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it.
 *
 * Parity status: the reference decoder could not be built or run in this pipeline
 * (SURVEY.md §8c), and the FATE bitstreams are absent, so this restatement is
 * "parity unpinned" against reference outputs; it is pinned by property tests built
 * from the reference's own checkasm generators (tests/checkasm/vp9dsp.c).
 */
#ifndef VP9_ORACLE_H
#define VP9_ORACLE_H
#include <stddef.h>
#include <stdint.h>
#include "../include/vp9hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* A frame: planes of uint8_t (bpp 8) or uint16_t (bpp > 8); stride in PIXELS.
 * Buffers must cover the frame size rounded up to 64 luma pixels. */
typedef struct vp9o_planes {
    void     *data[3];
    ptrdiff_t stride[3];
    int       w, h;        /* visible size */
} vp9o_planes;

/* Reconstruct + loop-filter one frame. refs[i] = LAST/GOLDEN/ALTREF (may be NULL
 * for intra frames). Returns 0 or a negative error. */
int vp9o_decode_frame(const vp9h_frame *f, vp9o_planes *cur, const vp9o_planes *refs);
/* The same frame with the tile columns of each SB row on up to nthreads threads and the
 * loop filter of the previous row overlapped (decode_tiles_mt + loopfilter_proc,
 * vp9.c:1442-1551): the slice-threaded CPU baseline. Output identical. */
int vp9o_decode_frame_tiles(const vp9h_frame *f, vp9o_planes *cur, const vp9o_planes *refs, int nthreads);

/* Optional trace of check_intra_mode (vp9recon.c:37-221) for tests that restate it from the
 * packet: while buf is set, every call of vp9o_decode_frame's intra reconstruction appends six
 * int32 (plane, tx size code, final mode after mode_conv 0..14, n_px_have of the top edge or 0
 * without have_top, n_px_have of the left edge or 0 without have_left, the 4x4 top-right:
 * 0 not read, 1 real, 2 replicated) while fewer than cap records are held. The count goes on
 * past cap. NULL ends the trace. Not for vp9o_decode_frame_tiles (one buffer, no lock). */
void vp9o_set_intra_trace(int32_t *buf, size_t cap);
size_t vp9o_intra_trace_count(void);

/* Optional census of the loop filter's line routine (loop_filter, vp9dsp_template.c:1780-1889).
 * While buf is set, every line it processes, from vp9o_decode_frame or vp9o_loop_filter, adds
 * to buf, VP9O_LF_CENSUS_N int64 the caller zeroed:
 *   count[plane class: luma, chroma][direction: column edge, row edge][coded width: 4, 8, 16]
 *        [arm: off (fm false), n4 (4-wide without hev), h4 (4-wide with hev), f8 (7-tap),
 *         f16 (15-tap)]                                                        60 cells
 *   moved, same shape: the lines of the cell whose output differs from their input  60 cells
 *   tight[plane class][10]: per comparison the lines where the deciding quantity equals its
 *        threshold, then those where it is one above: the largest neighbour difference against
 *        I (E's test passing), 2|p0-q0| + (|p1-q1|>>1) against E (I's test passing), the inner
 *        flat maximum against F (filtered lines of width 8 and 16), the outer flat maximum
 *        against F (width 16, inner flat), max(|p1-p0|, |q1-q0|) against H (lines that take the
 *        4-wide arms)                                                          20 cells
 * Plane class and direction are those of the frame path's filter_plane_cols / rows;
 * vp9o_loop_filter counts as luma with its dir. The arm is decided a second time, from the
 * pixels before the filter; pixels do not change. NULL ends it; off, a line costs one pointer
 * test. Not for vp9o_decode_frame_tiles (one buffer, no lock). */
#define VP9O_LF_CENSUS_N 140
void vp9o_set_lf_census(int64_t *buf);
/* E (mblim), I (lim), H (hev threshold) of a level as the frame path derives them (vp9.c:673-686,
 * vp9lpf.c:49), before the shift to the bit depth. Level 0 is never filtered. */
void vp9o_lf_limits(int level, int sharpness, int out[3]);

/* DSP entry points for unit tests (stride in pixels). */
void vp9o_itxfm_add(int bpp, void *dst, ptrdiff_t stride, void *coef, int eob, int tx, int txtp);
void vp9o_intra_pred(int bpp, void *dst, ptrdiff_t stride, const void *left, const void *top,
                     int tx, int mode);
void vp9o_loop_filter(int bpp, void *dst, ptrdiff_t stride, int kind, int wd1, int wd2, int dir,
                      int E, int I, int H);
/* scaled MC (do_scaled_8tap / do_scaled_bilin, vp9dsp_template.c:2363-2482) */
void vp9o_mc_scaled(int bpp, void *dst, ptrdiff_t ds, const void *src, ptrdiff_t ss, int w, int h,
                    int mx, int my, int dx, int dy, int filter, int avg);
void vp9o_mc(int bpp, void *dst, ptrdiff_t ds, const void *src, ptrdiff_t ss, int w, int h,
             int mx, int my, int filter, int avg);
/* scan table access: returns pointer to the scan for tx (0..3, 4 = lossless) / txtp */
const int16_t *vp9o_scan(int tx, int txtp);

#ifdef __cplusplus
}
#endif
#endif
