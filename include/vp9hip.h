/*
 * vp9hip.h — C-ABI boundary of the MI355X VP9 hybrid decoder.
 *
 * The host (entropy decode, header parse) produces one "pass-1 frame packet" per
 * frame; the device (gfx950 HIP kernels) runs the whole per-superblock pixel path:
 * inverse transforms, intra prediction, motion compensation and the loop filter.
 *
 * The packet mirrors the reference decoder's 2-pass buffers
 * (/root/reference/libavcodec/vp9.c:335-353, vp9block.c:1352-1362): one VP9Block
 * per coded block (vp9dec.h:89-97), the per-tx-block eobs and the dequantized
 * coefficients in scan order (vp9block.c:805-923), plus the frame-header values the
 * pixel path reads (vp9.c:669-791: LF level / sharpness / lossless / tiling).
 *
 * Entry points replace, one for one, the hooks the reference's hybrid path calls:
 *   vp9hip_open/close      <- ff_vp9_webgpu_init/uninit      (vp9_webgpu.h:370-375; vp9.c:1905-1917, 1281-1292)
 *   vp9hip_submit_frame    <- ff_vp9_webgpu_begin/end_frame  (vp9_webgpu.h:470-480; vp9.c:1319-1324, 1840-1845)
 *                             and FFHWAccel.start_frame/decode_slice/end_frame (hwaccel_internal.h:34-166; vp9.c:1694-1713)
 *   vp9hip_download_frame  <- the end_frame readback         (vp9_webgpu.c:2995-3056)
 *   vp9hip_flush           <- FFHWAccel.flush                (hwaccel_internal.h:165; vp9.c:1865-1883)
 * Errors are FFmpeg-style negative AVERROR codes (VP9HIP_E*).
 * A context is not thread-safe; use one host thread per context.
 */
#ifndef VP9HIP_H
#define VP9HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: vp9h_synth_params / vp9h_enc_params end in a vp9h_seg_params; vp9hip_test_hooks,
 * vp9hip_batch_frame_status and VP9HIP_PIPELINE_SLOTS added. Callers check
 * vp9hip_abi_version() == VP9HIP_ABI_VERSION before passing structs. */
/* 3: vp9h_frame_info and vp9hip_decoded_frame end in colorspace / full_range;
 * vp9h_stream_set_color and the output conversion (vp9hip_out_desc, vp9hip_convert_frames,
 * vp9hip_decoder_convert) added. vp9hip_convert_frames_scaled / vp9hip_decoder_convert_scaled
 * came later as new symbols only: no struct changed, so the version stayed. */
/* 4: vp9h_synth_params ends in eob_dense / ref_mix / mv_range. */
/* 5: vp9h_synth_params ends in edge_large / p_intra. vp9hip_convert_frames_resampled /
 * vp9hip_decoder_convert_resampled / vp9hip_resample_weights (with vp9hip_rect and
 * vp9hip_resample) came later, again as new symbols and new structs only: no existing struct
 * changed, so the version stayed. The motion export (vp9hip_set_export, vp9hip_frame_motion,
 * vp9hip_download_motion, vp9hip_motion_host, vp9hip_decoder_set_export,
 * vp9hip_decoder_frame_motion) likewise: new symbols only. The bicubic filter
 * (VP9HIP_FILTER_BICUBIC, vp9hip_convert_frames_bicubic, vp9hip_decoder_convert_bicubic,
 * vp9hip_bicubic_weights) likewise: a new macro and new symbols, the filter enum and
 * vp9hip_resample unchanged. The residual export (VP9HIP_EXPORT_RESIDUAL, vp9hip_frame_residual,
 * vp9hip_download_residual, vp9hip_residual_host, vp9hip_decoder_frame_residual) likewise: new
 * symbols only. Accumulated motion (VP9HIP_EXPORT_MOTION_ACC, vp9hip_acc_cell,
 * vp9hip_frame_motion_acc, vp9hip_download_motion_acc, vp9hip_motion_acc_host,
 * vp9hip_decoder_frame_motion_acc) likewise: a new macro, a new struct and new symbols. The
 * residual tensors at model size (VP9HIP_RESID_*, vp9hip_resid_desc,
 * vp9hip_residual_frames_scaled, vp9hip_residual_scaled_host, vp9hip_decoder_residual_scaled)
 * likewise: a new enum, a new struct and new symbols. The motion tensors at model size
 * (VP9HIP_MVT_*, vp9hip_mvt_desc, vp9hip_mvt_layout, vp9hip_motion_frames_scaled,
 * vp9hip_motion_scaled_host, vp9hip_decoder_motion_scaled) likewise. The accumulated residual
 * (VP9HIP_WARP_*, vp9hip_warp_layout, vp9hip_acc_warp, vp9hip_acc_warp_host,
 * vp9hip_warp_launch_dev, vp9hip_decoder_acc_warp) likewise: new enums and new symbols. The
 * accumulated residual at model size (vp9hip_warpt_desc, vp9hip_warpt_layout,
 * vp9hip_acc_warp_scaled, vp9hip_acc_warp_scaled_host, vp9hip_warp_scale_launch_dev,
 * vp9hip_decoder_acc_warp_scaled) likewise: a new struct and new symbols. The accumulated
 * propagation (VP9HIP_PROP_*, vp9hip_prop_desc, vp9hip_prop_layout, vp9hip_acc_propagate,
 * vp9hip_acc_propagate_host, vp9hip_prop_launch_dev, vp9hip_decoder_acc_propagate) likewise: new
 * enums, a new struct and new symbols. The graded output (vp9hip_grade, vp9hip_grade_desc,
 * vp9hip_grade_create, vp9hip_grade_destroy, vp9hip_convert_frames_graded,
 * vp9hip_decoder_convert_graded, vp9hip_grade_host) and the WebM colour description
 * (vp9h_webm_colour, vp9h_webm_read_colour) likewise: new structs and new symbols. The frame
 * histograms (VP9HIP_HIST_*, vp9hip_hist_desc, vp9hip_frame_histograms,
 * vp9hip_frame_histograms_host, vp9hip_decoder_histograms) likewise: a new enum, a new struct and
 * new symbols. */
#define VP9HIP_ABI_VERSION 5

/* FFmpeg AVERROR values used by the boundary (libavutil/error.h). */
#define VP9HIP_EINVAL       (-22)          /* AVERROR(EINVAL)   */
#define VP9HIP_ENOMEM       (-12)          /* AVERROR(ENOMEM)   */
#define VP9HIP_ENOSYS       (-38)          /* AVERROR(ENOSYS)   */
#define VP9HIP_EINVALIDDATA (-1094995529)  /* AVERROR_INVALIDDATA */
#define VP9HIP_EEXTERNAL    (-542398533)   /* AVERROR_EXTERNAL (HIP runtime failure) */
#define VP9HIP_EBUG         (-558323010)   /* AVERROR_BUG (internal invariant broken) */
#define VP9HIP_EAGAIN       (-11)          /* AVERROR(EAGAIN)   */
#define VP9HIP_EOF          (-541478725)   /* AVERROR_EOF       */

/* enum BlockSize (vp9shared.h:86-101) */
enum { VP9H_BS_64x64, VP9H_BS_64x32, VP9H_BS_32x64, VP9H_BS_32x32, VP9H_BS_32x16,
       VP9H_BS_16x32, VP9H_BS_16x16, VP9H_BS_16x8, VP9H_BS_8x16, VP9H_BS_8x8,
       VP9H_BS_8x4, VP9H_BS_4x8, VP9H_BS_4x4, VP9H_N_BS };
/* enum TxfmMode (vp9.h:27-35) */
enum { VP9H_TX_4X4, VP9H_TX_8X8, VP9H_TX_16X16, VP9H_TX_32X32 };
/* enum FilterMode (vp9.h:64-71) */
enum { VP9H_FILTER_SMOOTH, VP9H_FILTER_REGULAR, VP9H_FILTER_SHARP, VP9H_FILTER_BILINEAR };
/* intra modes 0..9 (vp9.h:45-62), inter modes (vp9shared.h:43-48) */
enum { VP9H_NEARESTMV = 10, VP9H_NEARMV = 11, VP9H_ZEROMV = 12, VP9H_NEWMV = 13 };

/* One coded block in decode order (VP9Block, vp9dec.h:89-97). 52 bytes. */
typedef struct vp9h_block {
    uint16_t row, col;      /* position in 8x8 units (vp9block.c:1276-1279)            */
    uint8_t  bs;            /* VP9H_BS_*                                               */
    uint8_t  tx, uvtx;      /* luma / chroma transform size (vp9block.c:1291)         */
    uint8_t  skip;          /* final skip flag, after vp9block.c:1310-1314             */
    uint8_t  intra, comp;   /* intra block; compound prediction                       */
    uint8_t  seg_id;        /* segment (selects LF level)                              */
    uint8_t  filter;        /* VP9H_FILTER_* for inter blocks                          */
    uint8_t  mode[4];       /* luma mode per 4x4 sub-block (intra 0..9, inter 10..13)  */
    uint8_t  uvmode;        /* chroma intra mode                                       */
    uint8_t  ref[2];        /* 0=LAST 1=GOLDEN 2=ALTREF                                */
    uint8_t  pad0;
    int16_t  mv[4][2][2];   /* [b_idx][ref][x,y] in 1/8 luma pel                       */
} vp9h_block;

/*
 * One frame of pass-1 output.
 * eobs: for every block with skip == 0, one uint16 per transform block that lies
 *   inside the frame (end_x/end_y clipping of vp9recon.c:243-244), in the reference's
 *   loop order: luma tx blocks row-major, then U, then V (vp9recon.c:269-357).
 *   Blocks with skip == 1 store nothing.
 * coefs: for every tx block with eob > 0, `eob` dequantized coefficients in scan
 *   order (the values decode_coeffs_b_generic stores at coef[scan[i]],
 *   vp9block.c:905-917): int16 for bpp == 8, int32 for bpp > 8.
 */
typedef struct vp9h_frame {
    int32_t  width, height;        /* visible size                                    */
    uint8_t  bpp;                  /* 8, 10, 12                                       */
    uint8_t  ss_h, ss_v;           /* chroma subsampling                              */
    uint8_t  keyframe, intraonly;
    uint8_t  lossless;             /* WHT 4x4 everywhere (vp9.c:704-705)              */
    uint8_t  filter_level;         /* s->s.h.filter.level                             */
    uint8_t  sharpness;            /* s->s.h.filter.sharpness                         */
    uint8_t  log2_tile_cols;
    uint8_t  log2_tile_rows;
    uint8_t  pad0[2];
    uint8_t  lflvl[8][4][2];       /* segmentation.feat[s].lflvl (vp9.c:767-791)       */
    int32_t  ref_w[3], ref_h[3];   /* visible size of LAST/GOLDEN/ALTREF (MC clamp)   */
    uint32_t nblocks;
    uint32_t neobs;
    uint64_t ncoefs;
    const vp9h_block *blocks;
    const uint16_t   *eobs;
    const void       *coefs;
} vp9h_frame;

/* ---- device context ---------------------------------------------------- */
typedef struct vp9hip_ctx vp9hip_ctx;

/* Open a context on HIP device `device`. Returns 0 or a negative error. The context reads
 * its VP9HIP_* environment switches (kernel A/B selections and diagnostics)
 * here, once; nothing later reads the environment. */
int  vp9hip_open(int device, vp9hip_ctx **out);
void vp9hip_close(vp9hip_ctx *ctx);
/* Test hooks, copied by every context opened afterwards (0, 0 = off, the default):
 * reject_batch = k | f << 16 makes frame f of the k-th batch the context stages (k >= 1,
 * restagings count) start with an intra block whose mode the device planner rejects;
 * lfr_spin = n bounds the row loop filter's hand-off waits to n polls (forcing its timeout
 * path). No reference counterpart; never called in production. */
void vp9hip_test_hooks(int reject_batch, uint32_t lfr_spin);
/* Test only: the device planner's intra schedule of the current slot's batch, copied to the
 * host after the device went idle. Per SB slot s (cap_slots of them at least): sbs + 3 s =
 * frame, sbx | sby << 16, tile_x0 | flags << 16; wgs + 4 s = first job, first pass word,
 * njobs | npass << 16, SB slot; the SB's pass words (first job << 14 | 4x4 jobs << 9 | 8x8 << 5 |
 * 16x16 << 2 | 32x32) at passes + job capacity * s and its job words (PJob.a) in pass order at
 * jobs_a + job capacity * s. Any pointer may be NULL. Returns the number of SB slots (*jcap:
 * the job capacity per SB) or a negative error; VP9HIP_EINVAL for a batch the host planned. */
int  vp9hip_test_plan_records(vp9hip_ctx *ctx, int cap_slots, int *jcap, uint32_t *sbs, uint32_t *wgs,
                              uint32_t *passes, uint32_t *jobs_a);
/* Test only, no device: the device planner's schedule of one SB restated in scalar code. ja[nj]:
 * the SB's intra jobs in decode order, each plane | tx size << 2 | mode slot << 8 | x4 << 12 |
 * y4 << 16 | trx << 30 (the PJob word's fields; trx: the 4x4 top-right lies inside the block).
 * Producers of a job: the earlier jobs covering the units of its top and left runs (masks[j]:
 * those units, bit u of the top row, bit 16 + v of the left column); heights: longest path to a
 * sink, at most 63; order: height descending, then index; per pass, chunk by chunk of 64 in that
 * order, the longest prefix of the ready jobs that fits the lanes left of 64; a pass's jobs
 * by size 32, 16, 8, 4, take order within a size. order[nj]: the decode index of the job at each
 * position of the SB's job array; passes: the pass words. Returns the number of passes, -1 for
 * bad arguments, -2 if a mask names a unit no earlier job covers or a pass can take no job. */
int  vp9hip_plan_sched_host(int ss_h, int ss_v, int nj, const uint32_t *ja, uint16_t *order, uint32_t *passes,
                            uint32_t *masks);
/* Test only, no device: the heights of the same jobs from the device planner's own relaxation
 * (the routine k_pjplan runs, a loop over 64 slots in place of the wave's lanes): heights[nj],
 * longest path to a sink, not clamped. Returns 0, -1 for bad arguments, -2 for overlapping jobs. */
int  vp9hip_plan_heights_host(int ss_h, int ss_v, int nj, const uint32_t *ja, uint32_t *heights);

/* Test only, no device: the same schedule from the device planner's own pass loop and emit (the
 * routines k_pjplan runs: the packed take scan, the ranks, the packed done words, the pass-word
 * scan and the positions; a loop over 64 slots in place of the wave's lanes). order and passes as
 * vp9hip_plan_sched_host's, *njobs (may be NULL) the jobs placed. Returns the number of passes,
 * -1 for bad arguments, -2 if a pass can take no job. */
int  vp9hip_plan_emit_host(int ss_h, int ss_v, int nj, const uint32_t *ja, uint16_t *order, uint32_t *passes,
                           int *njobs);

/* Allocate `nbufs` device frame buffers of w x h (padded to 64 internally). */
int  vp9hip_configure(vp9hip_ctx *ctx, int width, int height, int bpp, int ss_h, int ss_v,
                      int nbufs);

/*
 * Queue one frame: `out_buf` receives the reconstruction, ref_buf[0..2] are the
 * device buffers holding LAST/GOLDEN/ALTREF (ignored for intra frames).
 * The packet is copied (staged) before return; execution is asynchronous.
 */
int  vp9hip_submit_frame(vp9hip_ctx *ctx, const vp9h_frame *pkt, int out_buf,
                         const int ref_buf[3]);

/*
 * Batched form for independent (intra-only) frames: stage all packets into device
 * memory once (vp9hip_stage_batch), then run the pixel path over all of them with
 * frames interleaved in each wavefront launch (vp9hip_run_batch). run may be
 * repeated; the inputs stay resident in HBM.
 */
int  vp9hip_stage_batch(vp9hip_ctx *ctx, const vp9h_frame *pkts, int n, const int *out_bufs);
int  vp9hip_run_batch(vp9hip_ctx *ctx);
/*
 * Batch with inter frames: ref_bufs[3*i .. 3*i+2] are the LAST/GOLDEN/ALTREF buffers of
 * frame i (ignored for keyframes). Frames that reference (or overwrite) the output of an
 * earlier frame of the batch run after it; independent chains run concurrently.
 */
int  vp9hip_stage_batch_refs(vp9hip_ctx *ctx, const vp9h_frame *pkts, int n, const int *out_bufs,
                             const int *ref_bufs);

/*
 * Tile-column sharding of ONE stream over several devices (one context per device).
 * Every context stages the same packets. Its reconstruction covers only tile columns
 * [tile_lo, tile_hi), which is MC, residuals and intra; tile columns decode
 * independently (vp9.c:1244-1250, vp9recon.c:46). Its loop filter covers the whole
 * frame. Per phase (vp9hip_batch_phases, the frames of one chain position,
 * vp9hip_phase_frames):
 *   1. vp9hip_run_phase(ctx, ph, VP9HIP_PART_RECON);
 *   2. exchange the pre-LF stripes of that phase's frames (vp9hip_stripe pack, an
 *      all-gather, vp9hip_stripe unpack of the other shards' columns);
 *   3. vp9hip_run_phase(ctx, ph, VP9HIP_PART_LF).
 * Every device then holds the full post-LF frames that later phases reference.
 * The device form of the reference's slice-threaded tile decode: tile-column jobs
 * (decode_tiles_mt, vp9.c:1442-1520), then the loop filter over the whole frame
 * (loopfilter_proc, vp9.c:1522-1551; dispatched at vp9.c:1806).
 */
#define VP9HIP_PART_RECON 0
#define VP9HIP_PART_LF    1
int  vp9hip_stage_batch_tiles(vp9hip_ctx *ctx, const vp9h_frame *pkts, int n, const int *out_bufs,
                              const int *ref_bufs, int tile_lo, int tile_hi);
int  vp9hip_batch_phases(vp9hip_ctx *ctx);
/* Frame groups of the staged batch: independent chains run on that many HIP streams. */
int  vp9hip_batch_groups(vp9hip_ctx *ctx);
/* Batch indices of the frames in `phase` (up to cap written); returns their count. */
int  vp9hip_phase_frames(vp9hip_ctx *ctx, int phase, int *frames, int cap);
int  vp9hip_run_phase(vp9hip_ctx *ctx, int phase, int part);
/*
 * Pack (to_frame = 0) or unpack (1) the pixel columns of tile columns [tile_lo, tile_hi)
 * of batch frame `frame`, all 8-aligned rows, Y then U then V, between its device
 * buffer and contiguous device memory `dev`. The copy is asynchronous on the context's
 * stream. Returns the byte count, which is all it does when dev is NULL.
 */
int64_t vp9hip_stripe(vp9hip_ctx *ctx, int frame, int tile_lo, int tile_hi, void *dev, int to_frame);

/* Batch slots per context. */
#define VP9HIP_MAX_SLOTS 4
/* Batch slots the decoder (vp9hip_decoder_*) and the FFHWAccel adapter rotate: batch k + 3
 * is staged only after batch k's slot is checked, so three batches are in flight, each on
 * one frame-group stream (the context default: the slots' streams fit the 4 hardware
 * queues; bench.py times C3 / C4 / C5 at this depth, C2 at 4). */
#define VP9HIP_PIPELINE_SLOTS 3
/* Select batch slot 0 .. VP9HIP_MAX_SLOTS - 1 (default 0): stage_batch*, run_batch,
 * batch_phases, run_phase and stripe act on the current slot. Each slot holds its own
 * staged batch (arena, plan, launch graph) and runs on HIP streams of its own (slots 2..
 * create theirs at first selection); the frame buffers are the context's. Staged batches
 * that share no frame buffer run concurrently (one batch's device planning and intra
 * wavefront under another's loop filter); a batch that reads or writes a buffer of
 * another slot's batch follows that slot's last run. */
int  vp9hip_set_batch_slot(vp9hip_ctx *ctx, int slot);
/* Wait for the last run of batch slot `slot` only (other slots' work may continue)
 * and check it as vp9hip_sync does (VP9HIP_EBUG: a loop-filter hand-off timed out). */
int  vp9hip_sync_slot(vp9hip_ctx *ctx, int slot);
/* Per-frame outcome of the last stage / run of batch slot `slot` after stage_batch*,
 * run_batch, vp9hip_sync_slot or vp9hip_sync reported AVERROR_INVALIDDATA for it (the device
 * planner or the staging checks rejected frames): status[i] (staging order, up to cap) is 0
 * for a frame that was reconstructed, AVERROR_INVALIDDATA for a rejected frame, and
 * AVERROR(EAGAIN) for a valid frame that was not run (a batch planned on the host's
 * schedule stops before its pixel launches: stage those frames again). Keyframe batches
 * (launch lists fixed at staging) reconstruct the frames the planner did not reject; a
 * rejection that names no frame rejects all. Returns the batch's frame count. No reference
 * counterpart beyond vp9.c failing only the corrupt frame's decode (:1827-1832). */
int  vp9hip_batch_frame_status(vp9hip_ctx *ctx, int slot, int *status, int cap);
/* Make HIP stream `stream` (a hipStream_t; NULL: the null stream) wait for the last run of
 * batch slot `slot`, without a host wait: work enqueued on it afterwards sees that run's
 * frames. The loop-filter hand-off check needs a host wait (vp9hip_sync_slot). */
int  vp9hip_slot_stream_wait(vp9hip_ctx *ctx, int slot, void *stream);
/* 1 while the last run of batch slot `slot` is still executing, 0 once it is done. */
int  vp9hip_slot_busy(vp9hip_ctx *ctx, int slot);
/* Wait for all queued work of every batch slot. VP9HIP_EBUG if a row-pipelined
 * loop-filter launch (k_lfrd / k_lfro) of any slot gave up a bounded wait on another workgroup's
 * progress (frames not trusted). */
int  vp9hip_sync(vp9hip_ctx *ctx);

/* Copy device buffer `buf` into host planes (linesize in bytes). Synchronous. */
int  vp9hip_download_frame(vp9hip_ctx *ctx, int buf, uint8_t *const planes[3],
                           const ptrdiff_t linesize[3]);
/*
 * Zero-copy export of device buffer `buf` (replaces the D2H of vp9hip_download_frame for
 * consumers on the GPU; the hwcontext frame export of SURVEY 8f rank 2,
 * hwaccel_internal.h:146, libavutil/hwcontext.h:26-44): device pointers and byte
 * pitches of the three planes, the visible size, and the current batch slot's main
 * hipStream_t. Each batch slot runs on streams of its own, so a consumer orders its reads
 * after the slot that wrote the frame (vp9hip_slot_stream_wait), or reads after
 * vp9hip_sync / vp9hip_sync_slot. Pointers stay valid until vp9hip_configure /
 * vp9hip_close.
 */
int  vp9hip_frame_device(vp9hip_ctx *ctx, int buf, void *planes[3], ptrdiff_t linesize[3],
                         int *width, int *height, void **stream);

/* ---- output conversion: decoded planes -> what GPU consumers read -------------------
 * The reference leaves this to libswscale / the hwcontext's transfer; here the frames stay
 * on the device, so the crop, chroma upsample, colour matrix and range expansion run there.
 * The arithmetic is integer and exact (DESIGN.md "Output conversion"): chroma is the nearest
 * sample U[y >> ss_v][x >> ss_h]; 14 fractional coefficient bits, round half up, clip. */
enum { VP9HIP_OUT_SEMIPLANAR,  /* Y plane, then interleaved UV plane, at the source's subsampling:
                                  NV12/NV16/NV24 for 8-bit; 16-bit MSB-aligned (P010/P012 style,
                                  sample << (16 - bpp)) above 8 bits */
       VP9HIP_OUT_RGB24,       /* packed R,G,B u8, H x W x 3 */
       VP9HIP_OUT_RGBP_U8,     /* planar u8, 3 x H x W */
       VP9HIP_OUT_RGBP_F16 };  /* planar IEEE half in [0,1], 3 x H x W */
typedef struct vp9hip_out_desc {
    int32_t format;            /* VP9HIP_OUT_*                                          */
    int32_t colorspace;        /* VP9 code 1..5 or 7 (ignored for SEMIPLANAR); 0/6: EINVAL */
    int32_t full_range;
    int32_t width, height;     /* visible size to convert (<= the configured size)      */
    int64_t pitch;             /* bytes per output row, 0 = tight; must be a multiple of 16 if not tight */
    int64_t frame_stride;      /* bytes between frames, 0 = tight                        */
} vp9hip_out_desc;
/* Host only. The layout of one converted frame of a bpp / ss_h / ss_v source: returns its
 * bytes (pitch x rows of all planes) or VP9HIP_EINVAL; *pitch is the row pitch in effect and
 * plane_offset the byte offsets of its planes (R, G, B; or Y, the UV plane, and V's first
 * sample inside it; RGB24: 0, 1, 2). The tight pitch is the widest row: 3 w (RGB24), w (u8
 * planes), 2 w (half planes); SEMIPLANAR uses one pitch for both planes, the larger of the Y
 * row and the UV row (2 chroma samples per chroma column), and has (h + chroma rows) rows. */
int64_t vp9hip_out_layout(const vp9hip_out_desc *d, int bpp, int ss_h, int ss_v,
                          int64_t *pitch, int64_t plane_offset[3]);
/* Host only. The integer matrix of colour space 1..5 (VP9 codes: 1 / 3 BT.601, 2 BT.709,
 * 4 SMPTE-240M, 5 BT.2020 NCL) for bpp-bit samples and out_bits-bit output (8, or bpp for
 * the half format): c = CY, CRV, CGU, CGV, CBU, each floor(x * 2^shift + 0.5) with
 * shift = 14 + bpp - out_bits. Code 7 (RGB planes G, B, R) has no matrix: c is zero and
 * shift = bpp - out_bits. Codes 0 and 6: VP9HIP_EINVAL. */
int     vp9hip_out_coefs(int colorspace, int full_range, int bpp, int out_bits, int32_t c[5], int32_t *shift);
/* Convert the visible d->width x d->height pixels of device buffers bufs[0 .. n-1] (any
 * order, repeats allowed) into n frames at dst_dev (device memory, laid out as
 * vp9hip_out_layout says, frame i at i * frame_stride), in one launch per 32 frames. Enqueues
 * on `stream` (a hipStream_t; NULL: the current slot's main stream) and returns without
 * waiting. It orders nothing itself: the caller orders it after the frames' producer with
 * vp9hip_slot_stream_wait or a sync, exactly as for vp9hip_frame_device. Bytes outside the
 * visible rows and columns (pitch padding, frame_stride gaps) are not written.
 * VP9HIP_EINVAL: a buffer index out of range, a size above the configured one, n <= 0, a
 * NULL dst_dev, a layout vp9hip_out_layout refuses, or a dst_dev / frame_stride that is odd
 * for a 16-bit output. */
int  vp9hip_convert_frames(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_out_desc *d,
                           void *dst_dev, void *stream);
/*
 * Box-filter resize, fused into the conversion (one launch per 32 frames crops, resamples
 * and converts; the full-size frame is never written). The definition is integer and exact,
 * like the rest of the conversion (DESIGN.md "Box-filter resize").
 *
 * box(P, ow, oh) resamples a visible plane P of w x h integer samples to ow x oh: the exact
 * area mean, rounded once.
 *   wx(ox, sx) = max(0, min((ox+1) w, (sx+1) ow) - max(ox w, sx ow))
 *       the overlap of [ox w, (ox+1) w) and [sx ow, (sx+1) ow); one ox's weights sum to w.
 *       wy(oy, sy) is the same with h and oh.
 *   A(ox, oy)  = sum_sy wy(oy, sy) sum_sx wx(ox, sx) P[sy][sx]       exact integers, < 2^63
 *   box        = (A + (w h >> 1)) / (w h)                            floor: round half up
 * There is no intermediate rounding and no normalised weight, so every evaluation order
 * gives the same integers. The same formula serves every ratio: with ow == w and oh == h it
 * is the identity, and upscaling is nearest-neighbour with blended seams (an output sample
 * inside one source sample copies it, one across a boundary blends the two by area); the
 * interpolating (bilinear) filter is VP9HIP_FILTER_TRIANGLE of
 * vp9hip_convert_frames_resampled below, bicubic is vp9hip_convert_frames_bicubic.
 *
 * For a visible source of w x h luma and cw x ch chroma (cw = (w + ss_h) >> ss_h) and an
 * output of OW x OH:
 *   SEMIPLANAR: Y' = box(Y, OW, OH), U' = box(U, OCW, OCH), V' = box(V, OCW, OCH) with
 *       OCW = (OW + ss_h) >> ss_h, OCH = (OH + ss_v) >> ss_v; then interleaved and
 *       << (16 - bpp) above 8 bits as without a resize.
 *   RGB24, RGBP_U8, RGBP_F16: all three planes are resampled to the output size, box(Y, OW,
 *       OH), box(U, OW, OH), box(V, OW, OH) (the chroma plane is taken to cover the same
 *       picture area as luma: siting is not coded); the three planes, at the source's depth,
 *       then go through the conversion's arithmetic unchanged, as a 4:4:4 source would:
 *       matrix, clip, code-7 pass-through, the half multiply.
 * Only the visible d->width x d->height (the top-left crop) contributes: samples of the
 * 64-padding, or of a configured size larger than the visible one, never enter a sum. Other
 * regions of the picture are the source rectangles of vp9hip_convert_frames_resampled.
 *
 * d->width / d->height stay the visible source size; the output is laid out as
 * vp9hip_out_layout says for a desc of out_width x out_height with d's pitch / frame_stride.
 * Checked as vp9hip_convert_frames before the first launch (a refused call writes nothing);
 * out_width / out_height outside 1..16384: VP9HIP_EINVAL.
 */
int  vp9hip_convert_frames_scaled(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_out_desc *d,
                                  int out_width, int out_height, void *dst_dev, void *stream);
/*
 * Resampling with a choice of filter, a source rectangle and a destination rectangle per
 * output frame (letterbox), fused into the conversion like the box resize: one launch per 32
 * frames. Integer and exact, one right answer (DESIGN.md "Resampling: triangle filter, source
 * regions, letterbox").
 *
 * tri(P, ow, oh), the triangle filter of a w x h plane P of integer samples:
 *   M = max(w, ow);  tx(ox, sx) = max(0, 2M - |(2 ox + 1) w - (2 sx + 1) ow|),  0 <= sx < w
 *       the triangle 1 - |d| / s of support s = max(1, w / ow) source samples over the
 *       distance d between the output sample's centre and the source sample's, scaled by
 *       2 ow s to an integer. ty(oy, sy) is the same with h and oh.
 *   Dx(ox) = sum_sx tx(ox, sx) > 0 (the nearest source sample weighs >= M); Dy(oy) alike
 *   A(ox, oy) = sum_sy ty sum_sx tx P[sy][sx]                        exact integers
 *   tri = (A + (Dx Dy >> 1)) / (Dx Dy)                               floor: round half up
 * One rounding, no normalised weight tables, any evaluation order gives the same integers.
 * Taps outside the plane are absent from A and D alike: the edge clamps. ow == w is the
 * identity; a constant plane stays constant; upscaling has two taps per axis that sum to
 * 2 ow, ordinary bilinear interpolation with half-pixel centres (align_corners = False);
 * downscaling widens the triangle, so it is antialiased: the correctly rounded value of
 * torch's interpolate(mode="bilinear", antialias=True).
 * Bound: a call is accepted only if max_ox Dx * max_oy Dy * (2^bpp - 1) < 2^63 for every
 * (source geometry -> destination geometry) pair it uses, luma and chroma (7680 x 4320 at 12
 * bits -> 1 x 1 is just over it, -> 2 x 2 and the 8-bit -> 1 x 1 are under it).
 *
 * Source rectangle (x, y, w, h) in luma samples: inside d->width x d->height, w, h >= 1, x a
 * multiple of 1 << ss_h and y of 1 << ss_v (for every format). Its chroma rectangle is
 * (x >> ss_h, y >> ss_v, (w + ss_h) >> ss_h, (h + ss_v) >> ss_v). The filter is applied to the
 * sub-plane as if it were the whole plane: nothing outside it enters a sum, edges clamp at
 * it. NULL src_rects: the visible picture.
 *
 * Destination rectangle (dx, dy, dw, dh) inside the out_width x out_height output, dw, dh >=
 * 1, and fill codes fill[0..2] at the source's depth (Y, U, V; G, B, R for colour space 7),
 * 0 <= fill[p] < 2^bpp:
 *   RGB formats: the three planes are resampled to dw x dh and placed at (dx, dy); every
 *       other pixel is the conversion's arithmetic applied to (fill[0], fill[1], fill[2]).
 *   SEMIPLANAR: dx a multiple of 1 << ss_h, dy of 1 << ss_v; luma resampled to dw x dh, chroma
 *       to ((dw + ss_h) >> ss_h) x ((dh + ss_v) >> ss_v) at (dx >> ss_h, dy >> ss_v); everything
 *       else is the fill codes (<< (16 - bpp) above 8 bits).
 * NULL dst_rects: the whole output, fill unused. Every visible output byte is written,
 * picture or fill; pitch padding and frame gaps are not.
 *
 * VP9HIP_FILTER_BOX applies box of vp9hip_convert_frames_scaled to the same geometry; with
 * no rectangles the two calls give the same bytes.
 *
 * Checked as vp9hip_convert_frames, plus the above, before the first launch (a refused call
 * writes nothing): any violation, a NULL vp9hip_resample or an unknown filter is
 * VP9HIP_EINVAL (VP9HIP_FILTER_BICUBIC included: it has an entry of its own,
 * vp9hip_convert_frames_bicubic below). Not offered: Lanczos, siting-aware chroma, mean / std
 * normalisation, rotation.
 */
enum { VP9HIP_FILTER_BOX, VP9HIP_FILTER_TRIANGLE };
typedef struct vp9hip_rect { int32_t x, y, w, h; } vp9hip_rect;
typedef struct vp9hip_resample {
    int32_t filter;                 /* VP9HIP_FILTER_* */
    int32_t out_width, out_height;  /* 1..16384 */
    const vp9hip_rect *src_rects;   /* n entries, or NULL: the visible picture */
    const vp9hip_rect *dst_rects;   /* n entries, or NULL: the whole output */
    int32_t fill[3];
} vp9hip_resample;
int  vp9hip_convert_frames_resampled(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_out_desc *d,
                                     const vp9hip_resample *rs, void *dst_dev, void *stream);
/* Host only: the C statement of the filters' definition. The taps of output index o of an
 * axis of n_src source samples resampled to n_out (both 1..16384): returns their count,
 * *first = the first source index, weights[0 .. min(count, cap) - 1] and *sum = D(o) (box:
 * n_src); first / weights / sum may be NULL. VP9HIP_EINVAL: an unknown filter, a size or o
 * out of range, cap < 0. */
int  vp9hip_resample_weights(int filter, int n_src, int n_out, int o,
                             int *first, int32_t *weights, int cap, int64_t *sum);
/*
 * Bicubic resampling, with the struct, the rectangles, the fill, the formats and the layout of
 * vp9hip_convert_frames_resampled, and one launch per 32 frames like it. Integer and exact,
 * one right answer (DESIGN.md "Resampling: bicubic"). The filter is the Keys cubic with
 * a = -1/2 (Catmull-Rom), widened when downscaling (antialiased): the kernel of torch's
 * interpolate(mode="bicubic", antialias=True) and of PIL's BICUBIC.
 *
 * One axis of n_src source samples and n_out output samples: M = max(n_src, n_out), T = 2M,
 * Q = 14. For output index o and source index s, 0 <= s < n_src:
 *   u      = |(2o+1) n_src - (2s+1) n_out|     the distance in units of 1/T of the filter's
 *                                              unit; the tap is present iff u < 2T
 *   c(u)   = 3u^3 - 5T u^2 + 2T^3              for u < T
 *          = -u^3 + 5T u^2 - 8T^2 u + 4T^3     for T <= u < 2T   (c / 2T^3 is Keys at x = u/T)
 *   q(o,s) = floor((c(u) 2^Q + T^3) / (2T^3))  floor toward -inf: round half up;
 *                                              -1,214 <= q <= 2^14 (Keys is >= -2/27)
 *   D(o)   = sum_s q(o,s) over the present taps, > 0
 * cub(P, ow, oh) of a w x h plane P of integer samples at bpp bits, with qx, Dx from (w, ow)
 * and qy, Dy from (h, oh):
 *   A(ox, oy) = sum_sy qy sum_sx qx P[sy][sx]                        exact signed integers
 *   cub = clip(floor((A + (Dx Dy >> 1)) / (Dx Dy)), 0, 2^bpp - 1)
 * One rounding, then one clip (the negative lobes overshoot); no normalised weight tables, so
 * any evaluation order gives the same integers. Taps outside the plane, or outside the source
 * rectangle, are absent from A and D alike. ow == w is the identity (every other tap has u a
 * multiple of T, where c is 0 exactly); a constant plane stays constant. The weights are Keys
 * rounded to Q = 14 bits, so the result is within one code of the rounded and clipped value of
 * torch's float64 interpolate(mode="bicubic", antialias=True, align_corners=False), not that
 * value itself (at 12 bits about 5 % of samples differ by that one); Q = 16 would pass 64 bits
 * in c 2^Q at T = 2^15, so Q is not tunable.
 * Bound: with S = max_o sum_s |q(o,s)| of an axis, a call is accepted only if
 * Sx Sy (2^bpp - 1) < 2^62 for every (source geometry -> destination geometry) pair it uses,
 * luma and chroma (7680 x 4320 at 12 bits -> 1 x 1 and -> 2 x 2 are over it, -> 4 x 4 and the
 * 8-bit -> 1 x 1 are under it).
 *
 * rs->filter must be VP9HIP_FILTER_BICUBIC; everything else of rs, the source and destination
 * rectangles' rules, the chroma rectangles and the fill codes are those of
 * vp9hip_convert_frames_resampled. Checked before the first launch (a refused call writes
 * nothing): any violation, a NULL rs or another filter is VP9HIP_EINVAL. Not offered: Lanczos,
 * siting-aware chroma, mean / std normalisation, rotation.
 */
#define VP9HIP_FILTER_BICUBIC 2
int  vp9hip_convert_frames_bicubic(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_out_desc *d,
                                   const vp9hip_resample *rs, void *dst_dev, void *stream);
/* Host only: the C statement of the bicubic definition. The present taps of output index o of
 * an axis of n_src source samples resampled to n_out (both 1..16384): returns their count,
 * *first = the first source index, weights[0 .. min(count, cap) - 1] = q, *sum = D(o) and
 * *abs_sum = sum |q|; first / weights / sum / abs_sum may be NULL. VP9HIP_EINVAL: a size or o
 * out of range, cap < 0. */
int  vp9hip_bicubic_weights(int n_src, int n_out, int o, int *first, int32_t *weights, int cap,
                            int64_t *sum, int64_t *abs_sum);

/*
 * Graded output: a colour pipeline (transfer curve -> 3x3 matrix -> transfer curve / tone map)
 * on the stored pixel of the RGB formats, in the same launch as the crop, the resize and the
 * matrix (DESIGN.md "Graded output"). Integer and exact: the device does LUT -> integer 3x3 ->
 * LUT on integer codes with one stated rounding per stage; whatever float mathematics made the
 * tables (PQ, HLG, sRGB, tone curves, primaries) ran once on the host.
 *
 * A grade is in_lut (2^bpp entries of u16), m[3][3] (int32, 14 fractional bits, |m| <= 2^16)
 * and out_lut (4097 entries of u16, each <= out_max); out_max is 255 for RGB24 / RGBP_U8 and
 * 65535 for RGBP_F16. Defined for the three RGB formats only.
 *
 * For every output pixel take the R, G, B codes the same call's arithmetic gives at the
 * source's depth, vp9hip_out_coefs(..., out_bits = bpp): shift 14, clip to 2^bpp - 1, for the u8
 * formats too (the reduction to 8 bits moves into out_lut); colour space 7 passes its planes
 * through as without a grade. Then, for c = R, G, B and each output row r of m:
 *   L_c = in_lut[code_c]
 *   P_r = clip((m[r][0] L_R + m[r][1] L_G + m[r][2] L_B + 8192) >> 14, 0, 65535)
 *                                      64-bit sum, arithmetic shift (floor)
 *   i = P_r >> 4, f = P_r & 15
 *   v_r = (out_lut[i] (16 - f) + out_lut[i + 1] f + 8) >> 4           i + 1 <= 4096
 * v_r is stored as the u8, or as the half of v_r * float(1.0 / 65535) with the half format's two
 * roundings. Fill pixels (dst_rects) are fill[0..2] through the same arithmetic, matrix and
 * grade included. Nothing before the codes changes: the filters, rectangles, bounds and layouts
 * are those of vp9hip_convert_frames_resampled / _bicubic.
 *
 * The property that needs no tables to check: with in_lut[c] = c << (16 - bpp), m = 16384 I,
 * out_lut[i] = min(16 i, 65535) and RGBP_F16, v = c << (16 - bpp) exactly.
 * The limit: linear light is indexed at 12 bits and interpolated, so a curve with an infinite
 * slope at 0 (a pure power law) is off by up to about 1.6 u8 codes in its first segment; sRGB
 * and BT.709 have a linear toe and are not affected. Per-channel curves only: operators that
 * need the three channels at once (BT.2390 in ICtCp, max-RGB hue-preserving maps) are not
 * expressible.
 *
 * vp9hip_grade_create validates the desc (bpp 8 / 10 / 12, out_max 255 or 65535, every out_lut
 * entry <= out_max, every |m| <= 2^16, no NULL pointer: otherwise VP9HIP_EINVAL) and uploads the
 * tables to device memory once; it may synchronise. vp9hip_grade_destroy frees them (NULL: no-op)
 * and must not run while a conversion that uses the grade is in flight.
 *
 * vp9hip_convert_frames_graded: rs is the vp9hip_resample of the ungraded entries, any of the
 * three filters (box and triangle take the resampling kernel, bicubic the cubic one); the
 * visible size without a resize is the box filter with out_width == d->width, out_height ==
 * d->height, which is the identity. One launch per 32 frames, returns without waiting. All
 * checks of the ungraded entries apply, plus VP9HIP_EINVAL for SEMIPLANAR, a NULL grade, a
 * grade whose bpp is not the configured one, or whose out_max is not the format's. All checks
 * run before the first launch: a refused call writes nothing.
 */
typedef struct vp9hip_grade vp9hip_grade;
typedef struct vp9hip_grade_desc {
    int32_t bpp;                    /* 8, 10 or 12: in_lut has 1 << bpp entries */
    int32_t out_max;                /* 255 (RGB24, RGBP_U8) or 65535 (RGBP_F16) */
    const uint16_t *in_lut;
    const int32_t *m;               /* 9 coefficients, row-major: m[3 r + c] */
    const uint16_t *out_lut;        /* 4097 entries */
} vp9hip_grade_desc;
#define VP9HIP_GRADE_OUT_LUT 4097
int  vp9hip_grade_create(vp9hip_ctx *ctx, const vp9hip_grade_desc *desc, vp9hip_grade **out);
void vp9hip_grade_destroy(vp9hip_grade *g);
int  vp9hip_convert_frames_graded(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_out_desc *d,
                                  const vp9hip_resample *rs, const vp9hip_grade *grade, void *dst_dev, void *stream);
/* Host only: the C statement of the three stages. rgb_codes: n_pixels interleaved R, G, B codes
 * (each < 2^bpp); v: n_pixels interleaved results. VP9HIP_EINVAL: what vp9hip_grade_create
 * refuses, a NULL array, n_pixels < 0, or a code >= 2^bpp (nothing is written then). */
int  vp9hip_grade_host(const vp9hip_grade_desc *desc, const uint16_t *rgb_codes, int64_t n_pixels, uint16_t *v);

/* ---- motion export: the stream's own motion field and block modes as device tensors ----
 * The second product of the decode besides the pixels (FFmpeg's AV_FRAME_DATA_MOTION_VECTORS /
 * +export_mvs, which its VP9 decoder never filled): per 4x4 luma block the references, the
 * prediction mode, the block size / skip / segment and the coded motion vectors, written from
 * the batch's resident block array by one kernel (k_motion) per batch. Off by default; with it
 * off nothing is allocated and nothing is launched.
 *
 * Definition, in integers. For a frame of visible size width x height let cols8 = (width + 7)
 * >> 3 and rows8 = (height + 7) >> 3. The motion field is a grid of GW x GH = 2 cols8 x
 * 2 rows8 cells, each one 4x4 luma block. The frame's blocks in decode order partition the 8x8
 * grid (the planner rejects packets where they do not). A block at (row, col) in 8x8 units of
 * size bs covers the cells [2 row, 2 row + h4) x [2 col, 2 col + w4) clipped to the grid, w4 /
 * h4 its width / height in 4-pixel units; a block below 8x8 covers its whole 8x8 unit, 2 x 2
 * cells. A block with row >= rows8, col >= cols8 or bs >= VP9H_N_BS covers nothing. For cell
 * (r, c) inside block b, with i = (r & 1) * 2 + (c & 1):
 *   info[r][c][0] = b.intra ? 255 : b.ref[0]
 *   info[r][c][1] = (!b.intra && b.comp) ? b.ref[1] : 255
 *   info[r][c][2] = b.mode[i]
 *   info[r][c][3] = (uint8_t) (b.bs | b.skip << 4 | b.seg_id << 5)
 *   mv[r][c][k][0..1] = b.mv[i][k][0..1], (x, y) in 1/8 luma pel, for each reference k whose
 *       info byte is not 255, else 0: an intra block has all four values 0, a single-reference
 *       block has mv[r][c][1] = 0 whatever the packet holds there.
 * This relies on the packet filling all four mode[] / mv[] entries of every block as the
 * reference does (ff_vp9_fill_mv: four equal copies at >= 8x8, row pairs at 8x4, column pairs
 * at 4x8), as the planner's chroma vectors already do. A keyframe or intra-only frame gives
 * bytes 0 and 1 equal to 255 and zero vectors everywhere. Reference names are LAST / GOLDEN /
 * ALTREF as in the packet: mapping names to buffers stays the caller's business, through the
 * refs it staged with. Vectors are the coded ones, in the current frame's coordinates, also
 * under reference scaling. Not exported: transform sizes, the interpolation filter, chroma
 * vectors. */
#define VP9HIP_EXPORT_MOTION 1
/* Export flags (0, VP9HIP_EXPORT_MOTION, and / or VP9HIP_EXPORT_RESIDUAL, "residual export"
 * below, and / or VP9HIP_EXPORT_MOTION_ACC, "accumulated motion" below, which is VP9HIP_EINVAL
 * without VP9HIP_EXPORT_MOTION) of the next vp9hip_configure, which then allocates
 * two side planes per frame buffer, freed with the buffers: mv (8 bytes per cell) and info (4
 * bytes per cell), of the fixed cell pitch 2 ((cfg_width + 7) >> 3) and 2 ((cfg_height + 7) >> 3)
 * rows; a smaller frame in a larger context uses the top-left of its planes. VP9HIP_EINVAL:
 * unknown flags, or a change of the flags of a configured context. VP9HIP_ENOSYS: export with
 * VP9HIP_HOST_PLAN=1 (the host-planned path does not upload the blocks).
 * With export on, vp9hip_stage_batch / _refs (and vp9hip_submit_frame, which goes through them)
 * mark the batch's output buffers, and every vp9hip_run_batch writes their fields with one
 * k_motion launch ahead of the pixel work, so vp9hip_sync_slot / vp9hip_slot_stream_wait /
 * vp9hip_sync cover it. Every cell of the GW x GH grid is written, nothing else. A buffer that
 * several frames of one batch write keeps the field of the last of them (cells outside that
 * frame's grid are unspecified). The field of a frame the planner rejects is unspecified; a
 * vp9hip_run_batch that fails before its launches (AVERROR_INVALIDDATA from a batch planned on
 * the host's schedule) leaves none of the batch's buffers with a field until a later run. vp9hip_stage_batch_tiles does not export; it,
 * vp9hip_upload_frame and vp9hip_fill_buffers leave the buffers they write without a field. */
int  vp9hip_set_export(vp9hip_ctx *ctx, int flags);
/* The field of device buffer `buf`, in place, in the style of vp9hip_frame_device: device
 * pointers of the mv plane (int16, [gh][pitch_cells][2][2]) and the info plane (uint8,
 * [gh][pitch_cells][4]), the grid of the frame last exported into the buffer, the pitch in
 * cells, and the current slot's main hipStream_t; any output pointer may be NULL. Ordering is
 * the caller's, as for the pixels. VP9HIP_EINVAL without export or for a bad buf;
 * VP9HIP_EAGAIN if the buffer holds no exported field. */
int  vp9hip_frame_motion(vp9hip_ctx *ctx, int buf, void **mv_dev, void **info_dev, int *gw, int *gh,
                         int64_t *pitch_cells, void **stream);
/* Copy the field of `buf` into tight host arrays mv[gh][gw][2][2] and info[gh][gw][4] (either may
 * be NULL). Waits for the batches writing the buffer, like vp9hip_download_frame. Errors as
 * vp9hip_frame_motion. */
int  vp9hip_download_motion(vp9hip_ctx *ctx, int buf, int16_t *mv, uint8_t *info);
/* Host only, no device: the C statement of the definition above over pkt's blocks in decode
 * order, into tight mv[GH][GW][2][2] / info[GH][GW][4], with the clipping rules of the kernel
 * (blocks outside the grid or of an unknown size cover nothing; nothing outside the arrays is
 * written; cells no block covers keep their bytes). Returns the number of cells written
 * (a cell two blocks cover counts twice), or VP9HIP_EINVAL for a NULL argument or a packet
 * without a size. */
int  vp9hip_motion_host(const vp9h_frame *pkt, int16_t *mv, uint8_t *info);

/* ---- accumulated motion: every cell's displacement to the frame its content came from ----
 * The motion field above is relative to each frame's own references. Temporal propagation of
 * labels or features and CoViAR-style models want the vectors followed back through the GOP
 * until an intra cell or a keyframe. With VP9HIP_EXPORT_MOTION_ACC (only together with
 * VP9HIP_EXPORT_MOTION) one more kernel (k_mvacc) per batch does that on the device, where the
 * fields are resident and the runtime knows every frame's three reference buffers. Off by
 * default; with it off nothing is allocated and nothing is launched.
 *
 * With the flag vp9hip_configure allocates one more side plane per frame buffer, freed with the
 * buffers: 16 bytes (one vp9hip_acc_cell) per cell, at the motion planes' cell pitch and rows.
 *
 * Serials. Every frame staged by vp9hip_stage_batch / _refs on a context with the flag gets a
 * serial from a per-context uint32_t counter that starts at 1 and advances one per frame in
 * staging order; restagings count, a re-run of a staged batch keeps its serials. The serial lives
 * with the buffer's field, as the grid does.
 *
 * Parent of frame i of a batch for reference name k (0 LAST, 1 GOLDEN, 2 ALTREF). Let B =
 * ref_bufs[3 i + k]. If an earlier frame of the batch writes B, the parent is the latest such
 * frame j < i, provided j is the last writer of B in the batch; otherwise there is none
 * (NOFIELD). If no frame of the batch writes B and B holds an accumulated field (host-side
 * state, set and cleared exactly as the motion field's), the parent is that field, with its grid
 * and serial. In every other case there is none (NOFIELD): a buffer without a field, an external
 * buffer that a later frame of the batch overwrites. A parent whose grid (GW, GH) differs from
 * the frame's is none with SCALED.
 *
 * Record of cell (r, c) of frame t, with info, mv, GW and GH as the motion export defines them
 * and i0 = info[r][c][0]:
 *   i0 == 255 (an intra cell, hence every cell of a keyframe): { 0, 0, serial_t, 0, INTRA, 0 }.
 *   Otherwise let (mx, my) = mv[r][c][0]: only the first reference is followed, a compound
 *   block's second vector is ignored.
 *   i0 > 2, or no parent for name i0: { mx, my, 0, 1, NOFIELD or SCALED, 0 }.
 *   Else the parent cell is
 *     c' = clamp((32 c + 16 + mx) >> 5, 0, GW - 1)
 *     r' = clamp((32 r + 16 + my) >> 5, 0, GH - 1)
 *   (an arithmetic shift, so the division floors: the cell centre is displaced by the vector and
 *   snapped to the cell it lands in), q is the parent's record at (r', c'), and the record is
 *     { mx + q.dx, my + q.dy, q.root, min(q.hops + 1, 65535), q.end, 0 }.
 *   The two sums wrap modulo 2^32 (unsigned adds); they cannot wrap before hops saturates, since
 *   |mv| <= 2^15.
 * Every cell of the GW x GH grid is written, and nothing else. The field of a frame the planner
 * rejects, and of anything chained through it, is unspecified. A buffer written by several frames
 * of a batch keeps the last writer's field. A refused run, vp9hip_upload_frame,
 * vp9hip_fill_buffers and sharded batches leave the buffers they touch without a field. */
#define VP9HIP_EXPORT_MOTION_ACC 4
typedef struct vp9hip_acc_cell {   /* 16 bytes */
    int32_t  dx, dy;   /* sum of the coded vectors along the chain, 1/8 luma pel */
    uint32_t root;     /* serial of the frame where the chain ended, 0: unknown  */
    uint16_t hops;     /* frames stepped through, saturating at 65535            */
    uint8_t  end;      /* VP9HIP_ACC_END_*                                       */
    uint8_t  pad;      /* 0                                                      */
} vp9hip_acc_cell;
enum { VP9HIP_ACC_END_INTRA, VP9HIP_ACC_END_NOFIELD, VP9HIP_ACC_END_SCALED };
/* The accumulated field of device buffer `buf`, in place, in the style of vp9hip_frame_motion:
 * the device pointer of the plane (vp9hip_acc_cell [gh][pitch_cells]), the grid and serial of the
 * frame last exported into the buffer, the pitch in cells, and the current slot's main
 * hipStream_t; any output pointer may be NULL. VP9HIP_EINVAL without the flag or for a bad buf;
 * VP9HIP_EAGAIN if the buffer holds no field. */
int  vp9hip_frame_motion_acc(vp9hip_ctx *ctx, int buf, void **acc_dev, int *gw, int *gh,
                             int64_t *pitch_cells, uint32_t *serial, void **stream);
/* Copy the field of `buf` into a tight host array acc[gh][gw] (may be NULL). Waits for the
 * batches writing the buffer, like vp9hip_download_motion. Errors as vp9hip_frame_motion_acc. */
int  vp9hip_download_motion_acc(vp9hip_ctx *ctx, int buf, vp9hip_acc_cell *acc, uint32_t *serial);
/* Host only, no device: one frame of the recurrence above over tight arrays of one grid:
 * mv[gh][gw][2][2], info[gh][gw][4], out[gh][gw], and per reference name the parent's records
 * parent[k][gh][gw], or NULL for no parent, when parent_end[k] (VP9HIP_ACC_END_NOFIELD or
 * _SCALED) says why. VP9HIP_EINVAL for a NULL argument, a grid outside 1..4096 or a NULL parent
 * with another end code. */
int  vp9hip_motion_acc_host(const int16_t *mv, const uint8_t *info, int gw, int gh, uint32_t serial,
                            const vp9hip_acc_cell *const parent[3], const int parent_end[3],
                            vp9hip_acc_cell *out);

/* ---- residual export: what the transforms add to the prediction, as device tensors ----
 * The third input of compressed-domain models besides I-frame pixels and motion vectors. The
 * decode computes the residual of every coded transform block anyway (keyframes hold it in a
 * scratch for a moment, inter frames add it into the prediction in place); with
 * VP9HIP_EXPORT_RESIDUAL one more kernel (k_residual) per batch puts it where a consumer can
 * read it: three int16 planes per frame in picture geometry. Off by default; with it off nothing
 * is allocated and nothing is launched.
 *
 * Definition, in integers. For a frame of visible size w x h at bpp bits let m = 2^bpp - 1,
 * cols8 = (w + 7) >> 3 and rows8 = (h + 7) >> 3. The residual field is three int16 planes: Y of
 * 8 cols8 x 8 rows8 samples, U and V of (8 cols8 >> ss_h) x (8 rows8 >> ss_v): the coded area.
 * Take a tx block of the packet (the enumeration of vp9h_frame.eobs) with eob > 0, of plane p,
 * top-left (x0, y0) in that plane, size N and type (tx, txtp): the WHT in lossless frames; for
 * luma of an intra block below 32x32 the type of vp9hip_intra_txfm_type(mode); DCT_DCT for
 * everything else. Let r[y][x] be what itxfm_add adds before its clip
 * (vp9dsp_template.c:1139-1180: (out + (1 << (bits - 1))) >> bits, the DC-only shortcut
 * included). Then
 *   res[p][y0 + y][x0 + x] = clip(r[y][x], -m, m)
 * and every sample of the coded area that no such block covers is 0: skip blocks, eob 0, and
 * what a frame-edge partition leaves uncoded. Samples of a tx block outside the coded area are
 * unspecified (stored or dropped); nothing is written outside the buffer's 64-padded planes.
 * Why the clip: a prediction lies in [0, m], so clip(pred + r, 0, m) == clip(pred + clip(r, -m,
 * m), 0, m) for every pred: the clipped residual is all of the residual any picture can see, and
 * it fits int16 at 12 bits. It is also checkable against the reference's itxfm_add alone, on a
 * flat block of 0 and a flat block of m:
 *   clip(r, -m, m) = add(0) + (add(m) - m)
 * where add(v) is the pixel itxfm_add leaves on a block that was v everywhere (add(0) = clip(r,
 * 0, m), add(m) - m = clip(r, -m, 0)). Not exported: the prediction, the reconstruction before
 * the loop filter, coefficients in the frequency domain.
 *
 * vp9hip_set_export accepts VP9HIP_EXPORT_MOTION | VP9HIP_EXPORT_RESIDUAL in any combination,
 * under the rules stated there. With the residual flag vp9hip_configure allocates, per frame
 * buffer, one block of three int16 planes, freed with the buffers, in the pixel planes' padded
 * geometry: the pixel planes' pitches counted in elements and their 64-aligned heights, so a
 * consumer indexes residual and pixels alike and a whole tx block always fits. A field lives as a
 * motion field does: staging an exporting batch marks its output buffers, every vp9hip_run_batch
 * writes the whole coded area of their fields (zeros included) on the slot's main stream ahead of
 * the pixel work, so vp9hip_sync_slot / vp9hip_slot_stream_wait / vp9hip_sync cover it; a re-run
 * writes the same bytes; a buffer several frames of one batch write keeps the last writer's
 * field; the field of a frame the planner rejects is unspecified; vp9hip_stage_batch_tiles does
 * not export, and it, vp9hip_upload_frame, vp9hip_fill_buffers and a run the planner refuses
 * leave the buffers without a field. */
#define VP9HIP_EXPORT_RESIDUAL 2
/* The field of device buffer `buf`, in place: device pointers of the three int16 planes, their
 * pitches in elements, the visible size of the frame last exported into the buffer (the planes
 * hold its coded area, see above) and the current slot's main hipStream_t; any output pointer
 * may be NULL. Ordering is the caller's, as for the pixels. VP9HIP_EINVAL without the flag or
 * for a bad buf; VP9HIP_EAGAIN if the buffer holds no field. */
int  vp9hip_frame_residual(vp9hip_ctx *ctx, int buf, void *planes[3], int64_t pitch[3], int *width, int *height,
                           void **stream);
/* Copy the coded area of the field of `buf` into host planes (a NULL plane is skipped) of
 * linesize[] bytes a row (at least two bytes per sample of the coded width). Waits for the batches
 * writing the buffer, like vp9hip_download_frame. Errors as vp9hip_frame_residual. */
int  vp9hip_download_residual(vp9hip_ctx *ctx, int buf, int16_t *const planes[3], const ptrdiff_t linesize[3]);
/* Host only, no device: the C++ statement of the definition above over the packet alone, with
 * the kernel's 1-D transforms and record guards. planes[p] has pitch[p] int16 elements a row and
 * rows[p] rows, each at least the coded area, which is written: zeros, then the blocks (samples
 * outside the coded area are dropped). Every block, eob and coefficient index is checked
 * against the packet's counts and the plane sizes before anything is read or written: a packet
 * that breaks them returns VP9HIP_EINVALIDDATA with the planes untouched. VP9HIP_EINVAL for
 * NULL arguments, a packet without a size or format, or planes smaller than the coded area. */
int  vp9hip_residual_host(const vp9h_frame *pkt, int16_t *const planes[3], const ptrdiff_t pitch[3], const int rows[3]);

/* ---- residual tensors at model size: signed box resize and the RGB matrix, fused ----
 * What a CoViAR-style consumer reads is an (N, 3, OH, OW) residual tensor, usually RGB, at the
 * model's size. One launch per 32 frames (k_residual_scale) makes it from the fields above:
 * crop to the visible size, exact box resize, optionally the colour matrix, int16 or half.
 *
 * Definition, in integers.
 * Source: the field of a buffer as vp9hip_frame_residual reports it: the visible w x h luma
 * samples of the frame last exported into it and the cw x ch chroma samples,
 * cw = (w + ss_h) >> ss_h, ch = (h + ss_v) >> ss_v. Samples are the stored int16 codes,
 * whatever they are: the definition holds for every int16 value, so a consumer that wrote into
 * the views gets a defined result. Samples of the coded area beyond the visible size, and of the
 * padding, never enter a sum.
 * Signed box: sbox(P, ow, oh) of a w x h plane uses the weights wx, wy of box ("Box-filter
 * resize" above) unchanged:
 *   A(ox, oy) = sum_sy wy(oy, sy) sum_sx wx(ox, sx) P[sy][sx]     exact, |A| <= 2^15 2^28
 *   sbox      = floor((A + (w h >> 1)) / (w h))
 * The division floors toward minus infinity, so negative means round half up as well:
 * -2.5 -> -2, -2.25 -> -2. The weights of one output sample sum to w h, so
 * sbox(P + c) = sbox(P) + c for every constant c, and sbox(P) = box(P + 32768) - 32768: with the
 * sign bit of every stored sample flipped the source is a u16 plane for which the bounds of box
 * hold as they stand (column sums below 2^30, quotient below 2^16). An implementation may use
 * either form; both give the floor.
 * Resampling: all three planes are resampled to OW x OH, as the RGB formats of the scaled
 * conversion do: chroma covers the same picture area as luma. Call the results y, u, v.
 * Formats:
 *   VP9HIP_RESID_YUV_I16  the planes y, u, v.
 *   VP9HIP_RESID_RGB_I16  with (CY, CRV, CGU, CGV, CBU), S of vp9hip_out_coefs(colorspace,
 *     full_range, bpp, bpp) and m = 2^bpp - 1:
 *       R = clip((CY y + CRV v + 2^(S-1)) >> S, -m, m)
 *       G = clip((CY y - CGU u - CGV v + 2^(S-1)) >> S, -m, m)
 *       B = clip((CY y + CBU u + 2^(S-1)) >> S, -m, m)
 *     with arithmetic shifts and no offsets (the pixel's and its prediction's cancel).
 *     colorspace 7 (RGB planes) is R = v, G = y, B = u, clipped alike; 0 and 6 are VP9HIP_EINVAL.
 *     Every sum fits int32 for every int16 input: the largest CY + CBU (and CY + CGU + CGV) over
 *     all matrices and depths is 54,367, and 54,367 x 32,768 + 2^13 < 2^31.
 *   VP9HIP_RESID_YUV_F16, VP9HIP_RESID_RGB_F16  half(float(x) * float(1.0 / m)) of the integer
 *     value: one float32 multiply and one round-to-nearest-even conversion, as VP9HIP_OUT_RGBP_F16.
 *     RGB lies in [-1, 1]; YUV does for fields the decoder wrote. Other scalings are the caller's.
 * What the RGB residual is: for a pixel and a prediction that both convert without clipping,
 * RGB(pred + r) - RGB(pred) differs from the matrix of r by at most one code per channel (two
 * floors of sums that differ by the linear part), at the same size with chroma at full
 * resolution, for every matrix, range and depth.
 * Not offered: the triangle and bicubic filters, source / destination rectangles, energy maps. */
enum { VP9HIP_RESID_YUV_I16, VP9HIP_RESID_YUV_F16, VP9HIP_RESID_RGB_I16, VP9HIP_RESID_RGB_F16 };
/* The output of n frames: planar (n, 3, OH, OW) 16-bit elements; plane p of frame i starts at
 * dst + i frame_stride + p pitch OH. */
typedef struct vp9hip_resid_desc {
    int32_t format;            /* VP9HIP_RESID_* */
    int32_t colorspace;        /* VP9 code; ignored by the YUV formats */
    int32_t full_range;
    int32_t out_width, out_height;   /* 1..16384 */
    int64_t pitch;             /* bytes per output row, 0 = tight (2 OW); else a multiple of 16, >= 2 OW */
    int64_t frame_stride;      /* bytes between frames, 0 = tight (3 pitch OH); else even, >= 3 pitch OH */
} vp9hip_resid_desc;
/* Bytes of one frame of d (3 pitch OH) and the pitch in effect, or VP9HIP_EINVAL for a format
 * outside the enum, an output size outside 1..16384 or a pitch / frame stride the comments above
 * exclude. Host only; the colour fields are not looked at. */
int64_t vp9hip_resid_layout(const vp9hip_resid_desc *d, int64_t *pitch);
/* The fields of bufs[0 .. n-1] (any order, repeats allowed) into dst_dev. Every buffer must hold
 * a field and all fields must be of one visible size. Enqueues on `stream` (NULL: the current
 * slot's main stream) and returns; it orders nothing itself, exactly as vp9hip_convert_frames.
 * The buffers' pointers travel as kernel arguments, 32 frames per launch: no device table, no
 * allocation, no host wait, so the call can sit in a captured stream. Only the OW x OH elements
 * of each plane are written. Everything is checked before the first launch: a refused call
 * writes nothing. VP9HIP_EINVAL: no residual flag, a buffer index out of range, n <= 0, NULL
 * bufs or desc, fields of different sizes, a format outside the enum, colorspace 0, 6 or outside
 * 1..7 with an RGB format, an output size outside 1..16384, a NULL or odd dst_dev, a pitch or
 * frame stride the struct's comments exclude. VP9HIP_EAGAIN: a buffer without a field. */
int  vp9hip_residual_frames_scaled(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_resid_desc *d,
                                   void *dst_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one frame, one output
 * sample at a time in 64-bit integers. planes[p] are int16 planes of pitch[p] elements a row
 * holding at least the visible width x height (chroma: cw x ch) samples, which are all it reads;
 * dst is the frame's output in host memory, laid out by d (frame_stride is checked, not used).
 * VP9HIP_EINVAL: NULL arguments, width / height outside 1..16384, ss not 0 / 1, bpp not 8 / 10 /
 * 12, and what vp9hip_residual_frames_scaled refuses of d and dst; a refused call writes nothing. */
int  vp9hip_residual_scaled_host(const int16_t *const planes[3], const ptrdiff_t pitch[3], int width, int height,
                                 int ss_h, int ss_v, int bpp, const vp9hip_resid_desc *d, void *dst);

/* ---- motion tensors at model size: signed box resize of the motion fields, fused ----
 * The third input of a compressed-domain model at its own size, beside the pixels (the scaled
 * conversion) and the residual (above): an (N, 2 or 3, OH, OW) tensor of the motion vectors, and
 * optionally of how much of each output sample is inter-coded. One launch per 32 frames
 * (k_motion_scale) makes it from the fields of the motion export or of the accumulated motion.
 *
 * Definition, in integers.
 * Source: the motion field of a buffer as vp9hip_frame_motion reports it (VP9HIP_MVT_CODED), or
 * its accumulated field as vp9hip_frame_motion_acc reports it (VP9HIP_MVT_ACC), of a frame of
 * visible size w x h: GW = 2 ((w + 7) >> 3) and GH = 2 ((h + 7) >> 3) must equal the field's
 * grid. Every cell (r, c) has a value (vx, vy) and a flag has:
 *   VP9HIP_MVT_CODED  has = info[r][c][0] != 255; (vx, vy) = mv[r][c][0] when has, else (0, 0).
 *     The first reference's vector, as k_mvacc follows it; mv[r][c][1] is never looked at. The
 *     stored bytes are taken as they are (info[r][c][0] of 3..254 is has = 1), so a consumer that
 *     wrote into the views gets a defined result.
 *   VP9HIP_MVT_ACC    has = hops > 0; (vx, vy) = (clamp(dx, -32768, 32767),
 *     clamp(dy, -32768, 32767)) when has, else (0, 0). The clamp comes before any sum, so the
 *     bounds below hold for every int32 record.
 * Dense field: F[y][x] = the value of cell (y >> 2, x >> 2) for x < w, y < h. The output planes
 * are sbox(Fx, OW, OH), sbox(Fy, OW, OH) and, with three planes, sbox(256 has, OW, OH), sbox the
 * signed box of "residual tensors at model size": the weights wx, wy of "Box-filter resize", then
 * floor((A + (w h >> 1)) / (w h)). Intra cells count as zero vectors in the mean; dividing by
 * the coverage plane is the caller's choice.
 * F is constant over a cell, so the sum may run over cells with the aggregated weight
 *   W(o, c) = max(0, min((o + 1) n, (4 c + 4) on) - max(o n, 4 c on))      n = w or h, on = OW or OH
 * which is the sum of wx(o, sx) over the cell's four pixel columns (rows). The output intervals
 * end at n on, so a partly visible last cell is clipped without a special case and a cell beyond
 * the visible size has weight 0; the weights of one output sum to n.
 * Bounds: a column sum over cell rows is at most 2^14 2^15 = 2^29 in magnitude, |A| <= 2^43.
 * With the sign bit flipped the values are u16 and the bounds and the division of box hold as
 * they stand, as for the residual.
 * Formats:
 *   VP9HIP_MVT_I16  the integers: 1/8 luma pel of the source picture; the coverage plane 0..256.
 *   VP9HIP_MVT_F16  the displacement in output pixels: x is half(float(v) * kx) with
 *     kx = (float) ((double) OW / (8.0 w)), y the same with ky from OH and h, the coverage
 *     half(float(c) * (1.0f / 256)): one float32 multiply and one round-to-nearest-even
 *     conversion, as VP9HIP_OUT_RGBP_F16. A product beyond the half range becomes +-inf by that
 *     rounding.
 * Not offered: other filters, rectangles, the second reference's vectors, a per-reference split. */
enum { VP9HIP_MVT_I16, VP9HIP_MVT_F16 };
enum { VP9HIP_MVT_CODED, VP9HIP_MVT_ACC };
/* The output of n frames: planar (n, P, OH, OW) 16-bit elements, P = planes; plane p of frame i
 * starts at dst + i frame_stride + p pitch OH. Planes: x, y and, with P = 3, the coverage. */
typedef struct vp9hip_mvt_desc {
    int32_t format;            /* VP9HIP_MVT_I16 / _F16 */
    int32_t source;            /* VP9HIP_MVT_CODED / _ACC */
    int32_t planes;            /* 2 or 3 */
    int32_t width, height;     /* the frames' visible size, 1..16384; set by vp9hip_decoder_motion_scaled */
    int32_t out_width, out_height;   /* 1..16384 */
    int64_t pitch;             /* bytes per output row, 0 = tight (2 OW); else a multiple of 16, >= 2 OW */
    int64_t frame_stride;      /* bytes between frames, 0 = tight (P pitch OH); else even, >= P pitch OH */
} vp9hip_mvt_desc;
/* Bytes of one frame of d (P pitch OH) and the pitch in effect, or VP9HIP_EINVAL for a format,
 * source or planes out of range, a width, height or output size outside 1..16384 or a pitch /
 * frame stride the comments above exclude. Host only. */
int64_t vp9hip_mvt_layout(const vp9hip_mvt_desc *d, int64_t *pitch);
/* The fields of bufs[0 .. n-1] (any order, repeats allowed) into dst_dev, under the contract of
 * vp9hip_residual_frames_scaled: it enqueues on `stream` (NULL: the current slot's main stream)
 * and returns, orders nothing itself, passes the buffers' pointers as kernel arguments, 32 frames
 * per launch (no device table, no allocation, no host wait: it can sit in a captured stream),
 * writes only the OW x OH elements of each plane, and checks everything before the first launch:
 * a refused call writes nothing. VP9HIP_EINVAL: no motion export, VP9HIP_MVT_ACC without
 * VP9HIP_EXPORT_MOTION_ACC, a buffer index out of range, n <= 0, NULL bufs or desc, a format,
 * source or planes out of range, a width or height outside 1..16384 or not giving a field's grid
 * (hence fields of different grids), an output size outside 1..16384, a NULL or odd dst_dev, a
 * pitch or frame stride the struct's comments exclude. VP9HIP_EAGAIN: a buffer without a field. */
int  vp9hip_motion_frames_scaled(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_mvt_desc *d,
                                 void *dst_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one frame, one output
 * sample at a time in 64-bit integers. VP9HIP_MVT_CODED reads mv ([GH][pitch_cells][2][2]) and
 * info ([GH][pitch_cells][4]), VP9HIP_MVT_ACC reads acc ([GH][pitch_cells]); the other pointers
 * may be NULL. Only cells (r, c) with 4 c < width and 4 r < height are read. dst is the frame's
 * output in host memory, laid out by d (frame_stride is checked, not used). VP9HIP_EINVAL: a
 * NULL d or dst or source array, pitch_cells below (width + 3) >> 2, and what
 * vp9hip_motion_frames_scaled refuses of d and dst; a refused call writes nothing. */
int  vp9hip_motion_scaled_host(const int16_t *mv, const uint8_t *info, const vp9hip_acc_cell *acc,
                               ptrdiff_t pitch_cells, const vp9hip_mvt_desc *d, void *dst);

/* ---- frame metrics: exact sums over two device frames ---------------------------------
 * What a consumer needs to decide which frames are worth converting: near-duplicate and scene
 * cut detection (FFmpeg's scene score is the mean luma SAD of consecutive frames), PSNR against
 * a reference in another buffer, a coarse "what changed" map. One launch reads n pairs of
 * device frames once; everything is an integer sum with one right answer.
 *
 * A frame pair is (a, b): two buffers of one configured context, so of one depth and
 * subsampling. width x height is the visible luma size compared, the top-left crop as in
 * vp9hip_out_desc; the chroma planes are ((width + ss_h) >> ss_h) x ((height + ss_v) >> ss_v).
 * A sample is the stored code, uint8_t at 8 bits, else uint16_t; it is not masked to the depth.
 *
 * For each plane p (Y, U, V) of each pair, over the plane's visible samples, VP9HIP_METRIC_FIELDS
 * int64_t values in the order of the enum below. All fit: the largest is
 * sum a^2 <= 65535^2 * 2^28 < 2^61; FIRST <= 2^28. With bufs_b == NULL (statistics only)
 * SUM_B, SAD, SSE, NDIFF and MAXDIFF are 0 and FIRST is -1. The result of n pairs is a tight
 * (n, 3, VP9HIP_METRIC_FIELDS) int64 array, 192 bytes a pair, plane-major.
 *
 * The cell map (optional, luma only, needs b): MW = (width + 15) >> 4, MH = (height + 15) >> 4,
 * cells[i][cy][cx] = sum |a - b| over the visible luma samples of the 16 x 16 cell (a partial
 * cell sums what is visible), int32_t (at most 256 * 65535 < 2^24), tight (n, MH, MW). The
 * cells of a pair sum to its plane 0 SAD. Not offered: other cell sizes (pool the map), chroma
 * maps, rectangles other than the top-left crop, SSIM / VMAF. */
enum { VP9HIP_METRIC_SUM_A,    /* sum a                                                   */
       VP9HIP_METRIC_SUM_B,    /* sum b                                                   */
       VP9HIP_METRIC_SUMSQ_A,  /* sum a^2                                                 */
       VP9HIP_METRIC_SAD,      /* sum |a - b|                                             */
       VP9HIP_METRIC_SSE,      /* sum (a - b)^2                                           */
       VP9HIP_METRIC_NDIFF,    /* samples with a != b                                     */
       VP9HIP_METRIC_MAXDIFF,  /* max |a - b| (0 if none differ)                          */
       VP9HIP_METRIC_FIRST,    /* min (y * plane_width + x) over samples with a != b, -1 if none */
       VP9HIP_METRIC_FIELDS };
#define VP9HIP_METRIC_CELL 16
/* The metrics of the pairs (bufs_a[i], bufs_b[i]), i < n, into out_dev (device memory, n * 192
 * bytes) and, if cells_dev is not NULL, their cell maps into cells_dev (device memory,
 * n * MH * MW * 4 bytes). Any buffers in any order, repeats allowed, a == b allowed; bufs_b may
 * be NULL (statistics only). n above 32 is split into launches of at most 32 pairs. Enqueues on
 * `stream` (NULL: the current slot's main stream) and returns without waiting; it orders
 * nothing itself, exactly as vp9hip_convert_frames. No host wait, no allocation and no host
 * read of device memory, so it can sit in a captured stream. The results do not depend on what
 * out_dev / cells_dev held before; only those bytes are written. Everything is checked before
 * the first launch: a refused call writes nothing. VP9HIP_EINVAL: an unconfigured context, a
 * buffer index out of range, n <= 0, NULL bufs_a or out_dev, width / height outside
 * 1 .. the configured size, out_dev not 8-byte aligned, cells_dev not 4-byte aligned, cells_dev
 * without bufs_b. */
int  vp9hip_frame_metrics(vp9hip_ctx *ctx, const int *bufs_a, const int *bufs_b, int n,
                          int width, int height, int64_t *out_dev, int32_t *cells_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one pair of host frames
 * (linesize in bytes; b may be NULL, cells may be NULL): out[3][8], cells[MH][MW].
 * VP9HIP_EINVAL: NULL a, linesize_a or out, sizes outside 1..16384, bpp not 8 / 10 / 12, ss not
 * 0 / 1, b without linesize_b, cells without b. */
int  vp9hip_frame_metrics_host(const void *const a[3], const ptrdiff_t linesize_a[3],
                               const void *const b[3], const ptrdiff_t linesize_b[3],
                               int width, int height, int bpp, int ss_h, int ss_v,
                               int64_t out[24], int32_t *cells);

/* ---- frame histograms: per-plane and max-RGB code counts of device frames ----------------
 * What the consumers after the metrics and the graded output read: the distribution of
 * max(R, G, B) for a frame's light level (MaxCLL / MaxFALL, percentiles for a tone map's peak),
 * the histogram distance of consecutive frames for shot boundaries, percentile levels of
 * 10 / 12-bit sources. One launch reads n device frames once; every value is an integer count
 * with one right answer.
 *
 * A frame is a buffer of a configured context, of depth bpp (8 / 10 / 12) and subsampling ss_h,
 * ss_v. Each frame has a luma rectangle (x, y, w, h) under the rules of
 * vp9hip_resample.src_rects: inside the width x height given to the call, w, h >= 1, x a
 * multiple of 1 << ss_h and y of 1 << ss_v; its chroma rectangle is
 * (x >> ss_h, y >> ss_v, (w + ss_h) >> ss_h, (h + ss_v) >> ss_v). NULL rects: the top-left
 * width x height crop, as for the metrics.
 *
 * Bins: bins_log2 = k, 4 <= k <= bpp, B = 2^k. The bin of a code c is
 * min(c, 2^bpp - 1) >> (bpp - k): k = bpp is one bin per code, and stored codes above the depth
 * (only a consumer can have written them) land in the last bin.
 *
 * VP9HIP_HIST_PLANES (C = 3): channels Y, U, V, each the count per bin of the plane's samples
 * inside its rectangle. Channel 0 sums to w h, channels 1 and 2 to cw ch.
 *
 * VP9HIP_HIST_RGBM (C = 4): for every luma position (x, y) of the rectangle take the R, G, B
 * codes at the source's depth exactly as the graded output's definition above takes them: the
 * conversion's arithmetic with vp9hip_out_coefs(colorspace, full_range, bpp, out_bits = bpp),
 * chroma the nearest sample U[y >> ss_v][x >> ss_h], round half up, clip to 2^bpp - 1; colour
 * space 7 passes its planes through (G, B, R); colour spaces 0 and 6 are VP9HIP_EINVAL.
 * Channels R, G, B and M = max(R, G, B), each summing to w h. Defined for the source codes the
 * conversion's own arithmetic is defined for: codes within the depth.
 *
 * The result of n frames is a tight (n, C, B) int32 array; every count is at most 2^28. It does
 * not depend on what the destination held before, and only those bytes are written. Not
 * offered: joint or 2-D histograms, histograms of a graded or resized output, weights. */
enum { VP9HIP_HIST_PLANES,     /* Y, U, V                                                 */
       VP9HIP_HIST_RGBM };     /* R, G, B, max(R, G, B) at the source's depth             */
typedef struct vp9hip_hist_desc {
    int32_t what;               /* VP9HIP_HIST_* */
    int32_t bins_log2;          /* k: 4 .. bpp */
    int32_t colorspace;         /* RGBM: as vp9hip_out_desc; PLANES: not read */
    int32_t full_range;
    int32_t width, height;      /* the visible luma size the rectangles lie in */
    const vp9hip_rect *rects;   /* n entries, or NULL: the top-left width x height crop */
} vp9hip_hist_desc;
/* The histograms of the frames bufs[i], i < n, into out_dev (device memory, n * C * B * 4
 * bytes), under the contract of vp9hip_frame_metrics: any buffers in any order, repeats
 * allowed. n above 32 is split into launches of at most 32 frames. Enqueues on `stream` (NULL:
 * the current slot's main stream) and returns without waiting; it orders nothing itself. The
 * buffers' pointers and the rectangles travel as kernel arguments: no device table, no host
 * wait, no allocation and no host read of device memory, so it can sit in a captured stream.
 * The call zeroes out_dev itself (a memset on the same stream). Everything is checked before
 * the first launch: a refused call writes nothing. VP9HIP_EINVAL: an unconfigured context, a
 * buffer index out of range, n <= 0, NULL bufs, d or out_dev, `what` out of range, bins_log2
 * outside 4 .. bpp, RGBM with colour space 0 or 6 (or any other vp9hip_out_coefs refuses),
 * width / height outside 1 .. the configured size, a rectangle that breaks the rules above,
 * out_dev not 4-byte aligned. */
int  vp9hip_frame_histograms(vp9hip_ctx *ctx, const int *bufs, int n, const vp9hip_hist_desc *d,
                             int32_t *out_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one host frame (linesize in
 * bytes), one sample at a time: out[C][B]. d->rects is not read: `rect` is this frame's
 * rectangle, or NULL for the d->width x d->height crop. VP9HIP_EINVAL: NULL planes, linesize, d
 * or out, bpp not 8 / 10 / 12, ss not 0 / 1, sizes outside 1..16384, and what
 * vp9hip_frame_histograms refuses of d and the rectangle; a refused call writes nothing. */
int  vp9hip_frame_histograms_host(const void *const planes[3], const ptrdiff_t linesize[3],
                                  int bpp, int ss_h, int ss_v, const vp9hip_hist_desc *d,
                                  const vp9hip_rect *rect, int32_t *out);

/* ---- accumulated residual: frame t minus the root frame displaced by the accumulated motion ----
 * The input CoViAR-style models read beside the accumulated motion, and the motion-compensated
 * prediction of a frame from its root (label and feature propagation): one launch per 32 pairs
 * (k_acc_warp) gathers the root's samples through the accumulated field, where the fields and
 * both pictures are resident. On demand, like the frame metrics: nothing in the decode path
 * changes, and without the call nothing is launched or allocated.
 *
 * Definition, in integers. A pair is (a, b): two buffers of one configured context. a must hold
 * an accumulated field (vp9hip_frame_motion_acc would succeed) whose grid GW x GH is the grid of
 * the width x height given, GW = 2 ((width + 7) >> 3), GH = 2 ((height + 7) >> 3); width x height
 * is the visible luma size, the top-left crop as in vp9hip_frame_metrics, and the chroma planes
 * are ((width + ss_h) >> ss_h) x ((height + ss_v) >> ss_v). b must hold an accumulated field too;
 * S_b is the serial stored with it (host-side state, no device read). A sample is the stored
 * code, uint8_t at 8 bits, else uint16_t, not masked to the depth.
 * For plane p with subsampling (sh, sv) ((0, 0) for luma), visible size PW x PH, and sample (x, y):
 *   1. The cell is c = (x << sh) >> 2, r = (y << sv) >> 2, and q = acc_a[r][c].
 *   2. The cell applies iff q.hops > 0 && q.root == S_b. So intra cells never apply, chains that
 *      ended NOFIELD / SCALED (root 0; a serial is never 0) never apply, and a b that another
 *      frame has since been decoded into never applies.
 *   3. vx = clamp(q.dx, -32768, 32767), vy likewise, as VP9HIP_MVT_ACC. Px = vx << (1 - sh) and
 *      Py = vy << (1 - sv) are in 1/16 sample of the plane (<< on a negative value multiplies).
 *   4. VP9HIP_WARP_NEAREST: pred = B_p[cl(y + ((Py + 8) >> 4), PH)][cl(x + ((Px + 8) >> 4), PW)]
 *      with cl(v, n) = clamp(v, 0, n - 1) and arithmetic shifts.
 *   5. VP9HIP_WARP_BILINEAR: x0 = x + (Px >> 4), fx = Px & 15, y0 and fy likewise; the four
 *      samples s00, s01 (row cl(y0, PH), columns cl(x0, PW), cl(x0 + 1, PW)) and s10, s11 (row
 *      cl(y0 + 1, PH));
 *      pred = ((16 - fx)(16 - fy) s00 + fx (16 - fy) s01 + (16 - fx) fy s10 + fx fy s11 + 128) >> 8,
 *      at most 256 * 65535 + 128 < 2^32.
 *   6. VP9HIP_WARP_RESIDUAL (int16_t): clamp(A_p[y][x] - pred, -32768, 32767) where the cell
 *      applies, 0 elsewhere.
 *   7. VP9HIP_WARP_PICTURE (uint16_t): pred where the cell applies, A_p[y][x] elsewhere.
 *   8. The optional mask is uint8_t, tight (n, GH, GW): 1 where the cell applies, else 0.
 * The destination is tight per pair, 2-byte elements: Y (PH x PW of luma), then U, then V;
 * vp9hip_warp_layout gives the three offsets and the pair stride.
 * Not offered: sub-pel filters other than bilinear, the second reference, a per-hop warp. */
enum { VP9HIP_WARP_NEAREST, VP9HIP_WARP_BILINEAR };
enum { VP9HIP_WARP_RESIDUAL, VP9HIP_WARP_PICTURE };
/* Bytes of one pair's output (the stride between pairs) and, if off is not NULL, the byte
 * offsets of its Y, U and V planes; VP9HIP_EINVAL for a width or height outside 1..16384 or a
 * subsampling other than 0 / 1. Host only. */
int64_t vp9hip_warp_layout(int width, int height, int ss_h, int ss_v, int64_t off[3]);
/* The pairs (bufs_a[i], bufs_b[i]), i < n, into dst_dev (device memory, n strides of
 * vp9hip_warp_layout) and, if mask_dev is not NULL, their masks into mask_dev (n * GH * GW
 * bytes), under the contract of vp9hip_frame_metrics: any buffers in any order, repeats and
 * a == b allowed; n above 32 is split into launches of at most 32 pairs; it enqueues on `stream`
 * (NULL: the current slot's main stream) and returns without waiting, orders nothing itself, does
 * not allocate and reads no device memory on the host, so it can sit in a captured stream; only
 * the bytes of the layout (and of the mask) are written; everything is checked before the first
 * launch: a refused call writes nothing. VP9HIP_EINVAL: a context without
 * VP9HIP_EXPORT_MOTION_ACC or not configured, a buffer index out of range, n <= 0, NULL bufs_a,
 * bufs_b or dst_dev, a width / height outside 1 .. the configured size or whose grid is not that
 * of a's field, dst_dev not 8-byte aligned, an unknown mode or output. VP9HIP_EAGAIN: an a or a
 * b without a field (checked after the indices, before the grid). */
int  vp9hip_acc_warp(vp9hip_ctx *ctx, const int *bufs_a, const int *bufs_b, int n, int width, int height,
                     int mode, int output, void *dst_dev, uint8_t *mask_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one pair of host frames
 * (linesize in bytes) and a's field as a tight array acc[GH][GW], one sample at a time in 64-bit
 * integers; dst is the pair's output laid out by vp9hip_warp_layout, mask ([GH][GW]) may be NULL.
 * VP9HIP_EINVAL: a NULL a, b, linesize, acc or dst, sizes outside 1..16384, bpp not 8 / 10 / 12,
 * ss not 0 / 1, an unknown mode or output; a refused call writes nothing. */
int  vp9hip_acc_warp_host(const void *const a[3], const ptrdiff_t linesize_a[3],
                          const void *const b[3], const ptrdiff_t linesize_b[3],
                          const vp9hip_acc_cell *acc, uint32_t serial_b, int width, int height, int bpp,
                          int ss_h, int ss_v, int mode, int output, void *dst, uint8_t *mask);
/* Diagnostics (tools/acc_warp_bench.py, the crafted-field tests): k_acc_warp over caller-made
 * pictures and fields in device memory, on `stream`, split into launches of 32 pairs like
 * vp9hip_acc_warp. Pair i reads the frames a_dev[i] and b_dev[i] (planes at plane_off[p] bytes
 * inside each, rows pitch[0] / pitch[1] bytes apart for luma / chroma, covering the visible
 * size), the field acc_dev[i] (vp9hip_acc_cell [GH][acc_pitch_cells], 16-byte aligned) and the
 * serial serial_b[i]; the arrays themselves are host memory. VP9HIP_EINVAL: NULL arguments,
 * n <= 0, sizes outside 1..16384, bpp not 8 / 10 / 12, ss not 0 / 1, a pitch that does not
 * cover the plane's visible width or is odd above 8 bits, acc_pitch_cells below GW, dst_dev not
 * 8-byte aligned, an unknown mode or output. */
int  vp9hip_warp_launch_dev(const void *const *a_dev, const void *const *b_dev, const void *const *acc_dev,
                            const uint32_t *serial_b, int n, const int64_t plane_off[3], const int32_t pitch[2],
                            int64_t acc_pitch_cells, int width, int height, int bpp, int ss_h, int ss_v,
                            int mode, int output, void *dst_dev, uint8_t *mask_dev, void *stream);

/* ---- accumulated residual at model size: warp, signed box resize and the RGB matrix, fused ----
 * The accumulated residual as an (N, 3 or 4, OH, OW) tensor at the model's size, in one launch
 * per 32 pairs (k_acc_warp_scale): the composition of the two sections it names, without the
 * full-size planes between them. On demand, under the contract of vp9hip_acc_warp: nothing in the
 * decode path changes, and without the call nothing is launched or allocated.
 *
 * Definition, in integers. For a pair (a, b) of visible size w x h and mode VP9HIP_WARP_NEAREST /
 * VP9HIP_WARP_BILINEAR:
 *   1. R_Y, R_U, R_V are the VP9HIP_WARP_RESIDUAL planes of "accumulated residual", steps 1-6:
 *      int16 after the clamp, 0 where the cell does not apply.
 *   2. The output is "residual tensors at model size" applied to (R_Y, R_U, R_V) as a field of
 *      visible size w x h: all three planes through sbox(., OW, OH) with the same weights, the
 *      same floor and the same bounds (R is any int16, so the bounds hold as stated there), then
 *      one of the four formats VP9HIP_RESID_YUV_I16 / YUV_F16 / RGB_I16 / RGB_F16 with the same
 *      matrix without offsets, the same clip to [-m, m], m = 2^bpp - 1, the same colorspace 7
 *      rule and the same half rounding.
 *   3. The optional fourth plane is the coverage: C = sbox(256 applies(x >> 2, y >> 2), OW, OH)
 *      over the w x h luma samples (x, y), applies being step 2 of "accumulated residual"
 *      (hops > 0 && root == S_b): the integer 0..256 in the I16 formats,
 *      half(float(C) * (1.0f / 256)) in the F16 formats, as VP9HIP_MVT_F16's coverage. It is not
 *      the coverage of vp9hip_motion_frames_scaled over VP9HIP_MVT_ACC, which knows nothing of
 *      the root match.
 *   4. Layout: planar (n, P, OH, OW) 16-bit elements, P = 3 or 4; plane p of pair i starts at
 *      dst + i frame_stride + p pitch OH. Pitch and frame stride follow the rules of
 *      vp9hip_resid_desc with P in place of 3.
 * Not offered: the picture output at model size (an unsigned picture with offsets is the scaled
 * conversion's ground), other filters, rectangles. */
typedef struct vp9hip_warpt_desc {
    int32_t format;                 /* VP9HIP_RESID_* */
    int32_t colorspace, full_range; /* as vp9hip_resid_desc */
    int32_t mode;                   /* VP9HIP_WARP_NEAREST / VP9HIP_WARP_BILINEAR */
    int32_t planes;                 /* 3, or 4 with the coverage */
    int32_t width, height;          /* the visible size; vp9hip_decoder_acc_warp_scaled sets it from the frames */
    int32_t out_width, out_height;  /* 1..16384 */
    int64_t pitch;                  /* bytes per output row, 0 = tight (2 OW); else a multiple of 16, >= 2 OW */
    int64_t frame_stride;           /* bytes between pairs, 0 = tight (P pitch OH); else even, >= P pitch OH */
} vp9hip_warpt_desc;
/* Bytes of one pair of d (P pitch OH) and the pitch in effect, or VP9HIP_EINVAL for a format
 * outside the enum, planes not 3 / 4, an output size outside 1..16384 or a pitch / frame stride
 * the comments above exclude. Host only; mode, size and the colour fields are not looked at. */
int64_t vp9hip_warpt_layout(const vp9hip_warpt_desc *d, int64_t *pitch);
/* The pairs (bufs_a[i], bufs_b[i]), i < n, into dst_dev under the contract of vp9hip_acc_warp:
 * any buffers in any order, repeats and a == b allowed; n above 32 is split into launches of at
 * most 32 pairs; it enqueues on `stream` (NULL: the current slot's main stream) and returns
 * without waiting, orders nothing itself, does not allocate and reads no device memory on the
 * host, so it can sit in a captured stream; only the OW x OH elements of each plane are written;
 * everything is checked before the first launch: a refused call writes nothing. VP9HIP_EINVAL:
 * what vp9hip_acc_warp refuses (with d->width, d->height as the size), what
 * vp9hip_residual_frames_scaled refuses of format, colour, output size, dst_dev (NULL or odd),
 * pitch and frame stride, a NULL d, planes not 3 / 4, an unknown mode. VP9HIP_EAGAIN: an a or a b
 * without a field (checked after the indices, before the grid). */
int  vp9hip_acc_warp_scaled(vp9hip_ctx *ctx, const int *bufs_a, const int *bufs_b, int n,
                            const vp9hip_warpt_desc *d, void *dst_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one pair of host frames
 * (linesize in bytes) and a's field as a tight array acc[GH][GW], one output sample at a time in
 * 64-bit integers; the size is d->width x d->height; dst is the pair's output in host memory,
 * laid out by d (frame_stride is checked, not used). It reads only visible samples.
 * VP9HIP_EINVAL: what vp9hip_acc_warp_host and vp9hip_residual_scaled_host refuse, planes not
 * 3 / 4; a refused call writes nothing. */
int  vp9hip_acc_warp_scaled_host(const void *const a[3], const ptrdiff_t linesize_a[3],
                                 const void *const b[3], const ptrdiff_t linesize_b[3],
                                 const vp9hip_acc_cell *acc, uint32_t serial_b, int bpp, int ss_h, int ss_v,
                                 const vp9hip_warpt_desc *d, void *dst);
/* Diagnostics (tools/acc_warp_scale_bench.py, the crafted-field tests): k_acc_warp_scale over
 * caller-made pictures and fields in device memory, as vp9hip_warp_launch_dev describes them,
 * with the size from d. VP9HIP_EINVAL: what vp9hip_warp_launch_dev refuses of its arguments and
 * what vp9hip_acc_warp_scaled refuses of d and dst_dev. */
int  vp9hip_warp_scale_launch_dev(const void *const *a_dev, const void *const *b_dev, const void *const *acc_dev,
                                  const uint32_t *serial_b, int n, const int64_t plane_off[3], const int32_t pitch[2],
                                  int64_t acc_pitch_cells, int bpp, int ss_h, int ss_v,
                                  const vp9hip_warpt_desc *d, void *dst_dev, void *stream);

/* ---- accumulated propagation: a caller's tensor of the root frame displaced by the accumulated motion ----
 * Temporal propagation of labels or features: a model runs on the key frame, and its label map
 * or feature map is carried to the frames that follow through their accumulated fields. It is
 * the gather of "accumulated residual" with the caller's tensor as source and destination
 * instead of the frame buffers: the tensor lives on its own grid, has C channels and its own
 * element type. One launch per 32 pairs (k_prop_nchw / k_prop_nhwc). On demand, like
 * vp9hip_acc_warp: nothing in the decode path changes, and without the call nothing is launched
 * or allocated.
 *
 * Definition. A pair i is (a, S, src item): a is a buffer of a configured context that holds an
 * accumulated field, of grid GW x GH for the visible size w x h exactly as in "accumulated
 * residual"; S is the root's serial, a uint32_t the caller gives (vp9hip_frame_motion_acc and
 * vp9hip_download_motion_acc report a frame's serial). No root buffer is needed: the key frame's
 * pixels may have been released long ago, and its buffer overwritten. Serial 0 never applies.
 * The source item is src[src_index[i]]; a NULL src_index means i.
 * The tensor: M source items and n destination items, each of C channels on a feature grid
 * FW x FH that covers the visible w x h picture uniformly; elements of E = 1, 2, 4 or 8 bytes;
 * tight NCHW (VP9HIP_PROP_NCHW: element (ch, fy, fx) of an item at ((ch FH + fy) FW + fx) E
 * bytes) or tight NHWC (VP9HIP_PROP_NHWC: at ((fy FW + fx) C + ch) E bytes). The layout changes
 * addresses only. FW, FH in 1..16384, C in 1..4096, w and h as vp9hip_acc_warp.
 * For an output sample (fx, fy), all channels alike:
 *   1. The luma sample under its centre is X = ((2 fx + 1) w) / (2 FW), Y = ((2 fy + 1) h) / (2 FH):
 *      non-negative operands, the division floors, X < w and Y < h. The cell is c = X >> 2,
 *      r = Y >> 2, and q = acc_a[r][c].
 *   2. The cell applies iff q.hops > 0 && q.root == S: step 2 of "accumulated residual" with S in
 *      place of S_b.
 *   3. vx = clamp(q.dx, -32768, 32767), vy likewise. The displacement in 1/16 feature sample is
 *      Px = floor((4 vx FW + w) / (2 w)), Py = floor((4 vy FH + h) / (2 h)): a floor division of
 *      possibly negative 64-bit values, 2 vx FW / w rounded half up. With FW = w it is 2 vx, the
 *      luma rule of vp9hip_acc_warp; with w even and FW = w / 2 it is vx, its 4:2:0 chroma rule.
 *   4. VP9HIP_WARP_NEAREST: xs = cl(fx + ((Px + 8) >> 4), FW), ys = cl(fy + ((Py + 8) >> 4), FH)
 *      with cl and the shifts of "accumulated residual"; the element (ch, ys, xs) of the source
 *      item is copied bit for bit, at any E.
 *   5. VP9HIP_WARP_BILINEAR: E = 2 only, the elements are IEEE binary16. x0 = fx + (Px >> 4),
 *      frx = Px & 15, y0 and fry likewise; the four samples s00, s01 (row cl(y0, FH), columns
 *      cl(x0, FW), cl(x0 + 1, FW)) and s10, s11 (row cl(y0 + 1, FH)) are widened to binary32
 *      (exact). Each of the following operations is one binary32 operation, rounded to nearest
 *      even and never contracted:
 *        top = (16 - frx) s00 + frx s01
 *        bot = (16 - frx) s10 + frx s11
 *        v   = ((16 - fry) top + fry bot) 2^-8
 *      and the element is v rounded to the nearest-even binary16, subnormal halves included. The
 *      products of top and bot are exact, and no binary32 subnormal can arise. Non-finite inputs
 *      are outside the definition.
 *   6. Where the cell does not apply the element is the low E bytes of `fill`; with
 *      VP9HIP_PROP_KEEP the destination element is not written at all (the caller pre-fills it,
 *      e.g. with a cheap fresh inference).
 *   7. The optional valid output is uint8_t, tight (n, FH, FW): 1 where the sample's cell applies,
 *      else 0; written in both cases of step 6.
 * Not offered: source or destination rectangles, letterboxed grids, other filters, bilinear on
 * other element types, the second reference, strided tensors. */
enum { VP9HIP_PROP_NCHW, VP9HIP_PROP_NHWC };
#define VP9HIP_PROP_KEEP 1          /* flags: leave the destination where the cell does not apply */
typedef struct vp9hip_prop_desc {
    int32_t width, height;          /* the visible size w x h; vp9hip_decoder_acc_propagate sets it from the frames */
    int32_t fw, fh;                 /* the feature grid FW x FH, 1..16384 */
    int32_t channels;               /* C, 1..4096 */
    int32_t elem_size;              /* E: 1, 2, 4 or 8 bytes */
    int32_t layout;                 /* VP9HIP_PROP_NCHW / VP9HIP_PROP_NHWC */
    int32_t mode;                   /* VP9HIP_WARP_NEAREST / VP9HIP_WARP_BILINEAR (E = 2: binary16) */
    int32_t flags;                  /* 0 or VP9HIP_PROP_KEEP */
    int32_t reserved;               /* 0 */
    uint64_t fill;                  /* its low E bytes are the element where the cell does not apply */
} vp9hip_prop_desc;
/* Bytes of one item of d (C FH FW E) and, if valid_bytes is not NULL, of one item's valid map
 * (FH FW); VP9HIP_EINVAL for a NULL d, a width, height, fw or fh outside 1..16384, channels
 * outside 1..4096, an elem_size other than 1 / 2 / 4 / 8, an unknown layout or mode, bilinear
 * with elem_size != 2, unknown flag bits or a reserved field that is not 0. Host only. */
int64_t vp9hip_prop_layout(const vp9hip_prop_desc *d, int64_t *valid_bytes);
/* The pairs (bufs_a[i], root_serials[i], src item src_index[i]), i < n, of the m source items at
 * src_dev into the n items at dst_dev (device memory, strides of vp9hip_prop_layout) and, if
 * valid_dev is not NULL, their valid maps into valid_dev (n FH FW bytes), under the contract of
 * vp9hip_acc_warp: any buffers in any order, repeats allowed; n above 32 is split into launches
 * of at most 32 pairs; it enqueues on `stream` (NULL: the current slot's main stream) and returns
 * without waiting, orders nothing itself, does not allocate and reads no device memory on the
 * host, so it can sit in a captured stream; only the elements of the definition (and the valid
 * maps) are written; everything is checked before the first launch: a refused call writes
 * nothing. VP9HIP_EINVAL: a context without VP9HIP_EXPORT_MOTION_ACC or not configured, a buffer
 * index out of range, n <= 0 or m <= 0, NULL bufs_a, root_serials, d, src_dev or dst_dev, a
 * src_index[i] outside 0..m-1 (a NULL src_index with n > m), a width / height outside 1 .. the
 * configured size or whose grid is not that of a's field, what vp9hip_prop_layout refuses,
 * src_dev or dst_dev not aligned to E, the byte ranges of the m source items and the n
 * destination items overlapping. VP9HIP_EAGAIN: an a without a field (checked after the indices,
 * before the grid). */
int  vp9hip_acc_propagate(vp9hip_ctx *ctx, const int *bufs_a, const uint32_t *root_serials, const int *src_index,
                          int n, int m, const vp9hip_prop_desc *d, const void *src_dev, void *dst_dev,
                          uint8_t *valid_dev, void *stream);
/* Host only, no device: the C statement of the definition above for one pair, one sample at a
 * time: a's field as a tight array acc[GH][GW], one source item src and one destination item dst
 * in host memory, valid ([FH][FW]) may be NULL. The binary32 operations of step 5 are spelled
 * one a statement and the file is compiled with contraction off; the conversions to and from
 * binary16 are done in integers. VP9HIP_EINVAL: a NULL acc, d, src or dst, what
 * vp9hip_prop_layout refuses; a refused call writes nothing. */
int  vp9hip_acc_propagate_host(const vp9hip_acc_cell *acc, uint32_t root_serial, const vp9hip_prop_desc *d,
                               const void *src, void *dst, uint8_t *valid);
/* Diagnostics (tools/acc_propagate_bench.py, the crafted-field tests): the propagation kernels
 * over caller-made fields in device memory, on `stream`, split into launches of 32 pairs like
 * vp9hip_acc_propagate. Pair i reads the field acc_dev[i] (vp9hip_acc_cell
 * [GH][acc_pitch_cells], 16-byte aligned) with the serial serials[i]; the arrays themselves are
 * host memory. VP9HIP_EINVAL: NULL arguments, n <= 0 or m <= 0, acc_pitch_cells below GW, and
 * what vp9hip_acc_propagate refuses of src_index, d, src_dev and dst_dev. */
int  vp9hip_prop_launch_dev(const void *const *acc_dev, int64_t acc_pitch_cells, const uint32_t *serials,
                            const int *src_index, int n, int m, const vp9hip_prop_desc *d, const void *src_dev,
                            void *dst_dev, uint8_t *valid_dev, void *stream);

/* Upload host planes into device buffer `buf` (test hook for reference frames). */
int  vp9hip_upload_frame(vp9hip_ctx *ctx, int buf, const uint8_t *const planes[3],
                         const ptrdiff_t linesize[3]);

/* Drop queued work and the staged batches of every slot (FFHWAccel.flush). */
int  vp9hip_flush(vp9hip_ctx *ctx);
/* Fill device buffers [buf0, buf0 + count) with the byte `value`, asynchronously on the
 * context's stream (the bench poisons its frame buffers before the timed steps, so the
 * frames it verifies afterwards were written by those steps). No reference counterpart. */
int  vp9hip_fill_buffers(vp9hip_ctx *ctx, int buf0, int count, int value);

/*
 * Per-kernel timing of the last run (HIP events on the execution stream):
 * names[i] / ms[i] / launches[i] for up to `cap` kernel classes. Returns count.
 */
int  vp9hip_last_timing(vp9hip_ctx *ctx, const char **names, double *ms, int *launches, int cap);

/* Per-launch HIP-event timing on/off (default on). */
int  vp9hip_set_timing(vp9hip_ctx *ctx, int on);
/* Graph replay of a staged batch (default on): run_batch captures the batch's launch
 * sequence into a HIP graph once and replays it. Off: every run_batch enqueues the
 * launches directly (cheaper for a batch that runs once, e.g. the decoder's). */
int  vp9hip_set_graph(vp9hip_ctx *ctx, int on);

/* Algorithmic bytes (B = C + P(1+R) + 2P[LF]) of the staged batch,
 * per kernel class in vp9hip_last_timing order. Returns count. */
int  vp9hip_alg_bytes(vp9hip_ctx *ctx, double *bytes, int cap);

/* Host-only planning statistics of one packet (no device needed), 16 values:
 * SBs with intra work, passes, intra jobs, residual jobs, intra jobs per tx size (4),
 * lane use, max passes per SB, LF records, MC units, intra / LF wavefront steps,
 * intra dependency levels (summed over SBs: the lower bound of the passes), pixel rows
 * the passes loop over (each pass: its largest job size). A 17th value (cap >= 17): intra
 * steps under the dependency-level schedule of inter frames (= the diagonals otherwise);
 * 18-20: pass-packing estimates; 21-23 (cap >= 23): MC predicted-pixel bytes, those x (1 +
 * references), and the 128-byte lines the MC window rows touch, each unit counted alone. */
int  vp9hip_plan_stats(const vp9h_frame *pkt, double *out, int cap);
/* Diagnostics: per SB of one packet (raster order) the pixel rows its intra passes loop
 * over, as staged for the device (the wavefront-tail estimate of tools/wave_tail.py).
 * Returns the SB count, or a negative AVERROR. */
int  vp9hip_plan_sb_costs(const vp9h_frame *pkt, double *out, int cap);

int  vp9hip_abi_version(void);
/* PCI bus id ("0000:75:00.0") and name of HIP device `device` (so a multi-GPU run can show
 * each rank on its own card). VP9HIP_ENOSYS if there is no such device. */
int  vp9hip_device_info(int device, char *pci_bus_id, int len, char *name, int name_len);

/* ---- synthetic pass-1 generator (test / bench input) -------------------- */
/*
 * Generates a pseudo-random but structurally legal frame packet. Defaults follow the
 * stream settings of SURVEY.md §8(d): random partitions (P(split) 0.5 at 64/32, 0.3
 * at 16, 10 % sub-8x8), uniform intra modes, skip 0.2, TX_MODE_SELECT, per tx block
 * eob uniform in [1, min(n,64)] (eob_dense: 16x16 and 32x32 blocks up to all n
 * coefficients) with geometric(0.6) magnitudes and random sign,
 * base_q_idx 60 (no deltas), filter level 36, sharpness 0, LF deltas at the libvpx
 * defaults. inter != 0: an inter frame whose single-reference blocks read LAST and whose
 * compound blocks read LAST + ALTREF (ref_mix: every reference, see below), 50 % NEWMV,
 * MVs uniform in +-64 px (mv_range: another range), 10 % intra blocks (p_intra: another
 * share). A square the frame edge cuts splits with chance 0.7 (edge_large: 0.3). The packet
 * owns heap arrays; release with vp9hip_synth_free.
 */
/* Segmentation and loop-filter deltas of a frame (vp9.c:692-765, vp9block.c:101-141): what
 * vp9h_stream_encode writes into the frame header, and what vp9hip_synth_frame assumes for
 * the packet's segment ids, per-segment dequantization and LF levels. Values are the ones in
 * effect for the frame (the encoder codes the LF deltas that differ from the stream's, and
 * the segment features when update_data). All zero: no segmentation, libvpx's default LF
 * deltas (ref 1, 0, -1, -1; mode 0, 0) unchanged. */
typedef struct vp9h_seg_params {
    int32_t enabled;               /* segmentation_enabled                                  */
    int32_t update_map;            /* code the blocks' segment ids (else the map is kept)   */
    int32_t temporal;              /* inter frames: ids predicted from the previous map     */
    int32_t update_data;           /* code the per-segment features                         */
    int32_t abs_delta;             /* feature values absolute (else deltas to the frame's)  */
    int32_t q_en, lf_en;           /* bit s: segment s has the alternate q / LF feature     */
    int32_t q[8], lf[8];
    int32_t nseg;                  /* synth: segment ids drawn from 0 .. nseg - 1           */
    int32_t lf_delta_update;       /* lf_ref / lf_mode below are in effect (else defaults)  */
    int32_t lf_ref[4], lf_mode[2];
} vp9h_seg_params;

typedef struct vp9h_synth_params {
    int32_t  width, height;
    int32_t  bpp;              /* 8 / 10 / 12                                   */
    int32_t  ss_h, ss_v;       /* 1,1 = 4:2:0                                   */
    int32_t  log2_tile_cols;
    int32_t  inter;            /* 0 = keyframe; 1 = inter frame (see ref_mix)   */
    int32_t  compound;         /* inter: allow compound LAST+ALTREF blocks      */
    int32_t  q_idx;            /* base_q_idx (0 + lossless -> WHT)              */
    int32_t  lossless;
    int32_t  filter_level;
    int32_t  sharpness;
    int32_t  bilinear;         /* frame-level bilinear MC filter                */
    int32_t  coef_stress;      /* 1: coefficients uniform over the full range   */
    float    p_zero_eob;       /* chance that a tx block codes eob 0            */
    float    p_skip;           /* default 0.2                                   */
    uint64_t seed;
    vp9h_seg_params seg;       /* segmentation / LF deltas (default: none)      */
    /* ABI version 4; all zero = the draws above, packet for packet                 */
    int32_t  eob_dense;        /* 1: a tx block of n = N * N > 64 coefficients draws its
                                * eob from n, n - 1, 8N, 8N + 1, 65, uniform in [1, n]
                                * (twice as likely) and the default draw            */
    int32_t  ref_mix;          /* 1: single-reference blocks read LAST, GOLDEN or ALTREF,
                                * compound ones LAST or GOLDEN with ALTREF (codable
                                * under sign bias 0, 0, 1)                           */
    int32_t  mv_range;         /* nonzero MVs uniform in +-mv_range 1/8 pel, at most
                                * 16383 (0: 512)                                    */
    /* ABI version 5; all zero = the draws above, packet for packet                 */
    int32_t  edge_large;       /* 1: a square the frame's right or bottom edge cuts splits
                                * with chance 0.3, not 0.7 (else the forced H / V
                                * partition), and a block that edge cuts takes one of its
                                * two largest legal tx sizes three times in four    */
    float    p_intra;          /* inter frames: share of intra blocks (0: 0.1)      */
} vp9h_synth_params;

/* Fill p with the §8(d) defaults for a w x h bpp stream. */
void vp9hip_synth_defaults(vp9h_synth_params *p, int width, int height, int bpp);
int  vp9hip_synth_frame(vp9h_frame *out, const vp9h_synth_params *p);
void vp9hip_synth_free(vp9h_frame *f);

/* ---- host bitstream side: VP9 frame <-> pass-1 packet ----------
 * vp9h_decode_frame parses one frame's compressed data (uncompressed + compressed
 * header, tiles) into a pass-1 packet: the host entropy decode whose output the device
 * path consumes. It follows decode_frame_header / decode_tiles / decode_sb /
 * ff_vp9_decode_block of the reference (vp9.c:519-1395, vp9block.c:80-1130). The packet
 * owns heap arrays; release them with vp9h_frame_free.
 * vp9h_encode_frame writes a pass-1 packet as a VP9 bitstream (the synthetic stream
 * generator): default probabilities, frame_parallel, tx_mode = TX_MODE_SELECT, libvpx's
 * default LF deltas. Release the buffer with vp9h_buffer_free.
 * These one-frame forms take keyframes and intra-only frames (no reference state);
 * streams with inter frames go through a vp9h_stream below. Profiles 0-3. */
int  vp9h_decode_frame(const uint8_t *data, size_t size, vp9h_frame *out);
int  vp9h_encode_frame(const vp9h_frame *pkt, int base_q_idx, uint8_t **out, size_t *size);
void vp9h_frame_free(vp9h_frame *f);
void vp9h_buffer_free(uint8_t *p);

/*
 * A stream's host parse state (VP9Context's frame-to-frame state: the 4 saved probability
 * contexts prob_ctx, the 8 reference slots' sizes, the last frame's MV pairs and the
 * segmentation-map reference, vp9.c:1616-1686; the persistent header s->s.h). One
 * vp9h_stream either decodes or encodes one stream, frame by frame, in order.
 */
typedef struct vp9h_stream vp9h_stream;
int  vp9h_stream_open(vp9h_stream **out);
void vp9h_stream_close(vp9h_stream *s);

/* Tile-column threads of vp9h_stream_decode (default 1): the tile columns of a frame are
 * entropy-decoded concurrently, as decode_tiles_mt does with slice threads
 * (vp9.c:1441-1520, launched at 1777-1806). The packet is the serial walk's, byte for byte. */
int  vp9h_stream_set_threads(vp9h_stream *s, int n);
/* Encoding streams: the colour space (VP9 code: 0 unknown, 1 BT.470BG/601, 2 BT.709,
 * 3 SMPTE-170M/601, 4 SMPTE-240M, 5 BT.2020 NCL, 7 RGB) and range bit that the colour config
 * of the following keyframes / intra-only frames codes (read_colorspace_details,
 * vp9.c:457-517). Default 2, 0. Code 6 (reserved): VP9HIP_EINVAL. Code 7 has no range bit
 * (full range) and vp9h_stream_encode accepts it only for 4:4:4 packets (profile 1 / 3),
 * else it returns VP9HIP_EINVAL. */
int  vp9h_stream_set_color(vp9h_stream *s, int colorspace, int full_range);

/* What the frame header decided beyond the packet (reference slot bookkeeping for the
 * device buffers, vp9.c:1686-1691, 1845-1849). */
typedef struct vp9h_frame_info {
    int32_t show_existing_frame;   /* 1: no packet; output reference slot show_slot        */
    int32_t show_slot;
    int32_t show_frame;            /* 0: decoded into the slots but not output             */
    int32_t refresh_mask;          /* slots that receive this frame                        */
    int32_t ref_slot[3];           /* LAST / GOLDEN / ALTREF slots (inter frames)           */
    int32_t sign_bias[3];
    int32_t error_res, refresh_ctx, parallel, ctx_id;
    int32_t allow_hp, interp, comp_mode, tx_mode;
    uint32_t header_size, compressed_header_size;
    int32_t colorspace, full_range; /* the stream's colour space code and range in effect for  */
                                   /* this frame (avctx->colorspace / color_range: kept over  */
                                   /* inter frames and show_existing_frame; RGB is full range; */
                                   /* a profile-0 intra-only frame sets BT.601 limited)        */
} vp9h_frame_info;

/* Parse one frame (one superframe part) of the stream: the packet, or for
 * show_existing_frame only `info` (out is left empty). */
int  vp9h_stream_decode(vp9h_stream *s, const uint8_t *data, size_t size, vp9h_frame *out,
                        vp9h_frame_info *info);

/*
 * The same parse in two steps, so consecutive frames of one stream overlap as the
 * reference's frame threads do (ff_thread_finish_setup once the headers are parsed,
 * vp9.c:1752-1754; the next frame then waits per SB row for this frame's MV pairs and
 * segmentation map, vp9mvs.c:177-178, vp9block.c:116-117):
 *   vp9h_stream_decode_begin parses the headers and advances the stream: the next frame's
 *   begin may follow at once unless *serial is set (refresh_frame_context without
 *   frame_parallel_decoding_mode: the next headers read the probabilities this frame's tiles
 *   adapt, so its finish must complete first). *pending is NULL for show_existing_frame
 *   (info says which slot). data must stay valid until finish.
 *   vp9h_stream_decode_finish walks the tiles on `threads` tile-column threads, waiting for
 *   the rows of the earlier frames' side buffers it reads, and frees the pending frame. The
 *   finishes of one stream may run concurrently on different threads if each frame's finish
 *   starts after the previous frame's finish has started.
 * The packets equal vp9h_stream_decode's byte for byte (tests/c/host_san.cpp). A frame
 * whose tiles fail makes the later frames that read its side buffers fail too. */
typedef struct vp9h_pending vp9h_pending;
int  vp9h_stream_decode_begin(vp9h_stream *s, const uint8_t *data, size_t size, vp9h_pending **pending,
                              vp9h_frame_info *info, int *serial);
int  vp9h_stream_decode_finish(vp9h_pending *pending, int threads, vp9h_frame *out);
void vp9h_pending_free(vp9h_pending *pending);     /* a begun frame that will not be finished */

/* Encoder choices for one frame (vp9h_enc_defaults: the SURVEY 8(d) stream settings). */
typedef struct vp9h_enc_params {
    int32_t base_q_idx;
    int32_t show_existing_frame, show_slot;   /* 1: write a show_existing_frame header only */
    int32_t show_frame;
    int32_t error_res;
    int32_t refresh_mask;          /* -1: keyframes / intra-only all slots, inter slot 0   */
    int32_t ref_slot[3];
    int32_t sign_bias[3];          /* default 0, 0, 1: compound prediction allowed          */
    int32_t refresh_ctx, parallel, ctx_id, reset_ctx;
    int32_t allow_hp;
    int32_t interp;                /* -1: fixed if every inter block shares one filter      */
    int32_t comp_mode;             /* -1: switchable when the packet has compound blocks    */
    int32_t tx_mode;               /* -1: TX_MODE_SELECT                                    */
    int32_t prob_updates;          /* 0: none; else the seed of random forward updates      */
    int32_t keep_modes;            /* 1: code the packet's inter modes, taking the MVs they  */
                                   /*    predict (NEAREST / NEAR / ZERO); 0: keep the MVs    */
    vp9h_seg_params seg;           /* segmentation / LF deltas to code (default: none)      */
} vp9h_enc_params;
void vp9h_enc_defaults(vp9h_enc_params *p);

/*
 * Write one frame. `coded` (optional) receives the packet exactly as written, which is
 * what vp9h_stream_decode returns for the bitstream. It differs from `pkt` only where
 * the syntax cannot say what the packet says:
 *   - an inter mode whose predicted MV is not the packet's MV becomes NEWMV (keep_modes:
 *     the mode stays and the MV becomes the predicted one);
 *   - a low-precision MV difference loses its odd 1/8-pel step (vp9mvs.c:302-318);
 *   - a skipped inter block takes the largest transform size (vp9block.c:213-215);
 *   - an inter block <= 8x8 without coefficients becomes skip (vp9block.c:1310-1314);
 *   - fields the syntax does not carry are zero (intra blocks' MVs / refs / filter,
 *     single-reference blocks' second MV and reference).
 */
int  vp9h_stream_encode(vp9h_stream *s, const vp9h_frame *pkt, const vp9h_enc_params *p,
                        uint8_t **out, size_t *size, vp9h_frame *coded);

/* The frame type from the first header bits: 0 keyframe (its parse needs no earlier
 * frame), 1 other frame, 2 show_existing_frame, or AVERROR_INVALIDDATA. */
int  vp9h_frame_type(const uint8_t *data, size_t size);

/* The slot bookkeeping of a frame from the start of its uncompressed header, without
 * stream state (vp9.c:519-611, what vp9.c knows before ff_thread_finish_setup):
 * show_existing_frame + show_slot, show_frame, error_res, refresh_mask, and ref_slot /
 * sign_bias of inter frames; the other fields are zero. Returns 0 keyframe, 1 inter frame,
 * 2 show_existing_frame, 3 intra-only frame, or AVERROR_INVALIDDATA. Being stateless, it
 * fills colorspace / full_range only for frames whose header codes them (keyframes, and
 * intra-only frames in profiles 1-3) and leaves 0 otherwise: the values in effect for any
 * other frame are the stream's (vp9h_stream_decode / vp9h_stream_decode_begin). */
int  vp9h_frame_peek(const uint8_t *data, size_t size, vp9h_frame_info *info);

/* Split a superframe into its frames (vp9_superframe_split_bsf,
 * bsf/vp9_superframe_split.c:40-95): up to cap (offset, size) pairs; returns the frame
 * count (1 for a plain frame) or a negative error. */
int  vp9h_superframe_split(const uint8_t *data, size_t size, size_t *offsets, size_t *sizes, int cap);

/* ---- IVF container (libavformat/ivfdec.c, ivfenc.c) ------------- */
typedef struct vp9h_ivf_header {
    char     fourcc[5];            /* "VP90" for VP9, NUL-terminated                        */
    int32_t  width, height;
    uint32_t time_base_den, time_base_num;
    uint32_t nb_frames;
    uint32_t header_size;
} vp9h_ivf_header;
/* ivfdec.c probe (:27-34): 98 (AVPROBE_SCORE_MAX - 2) for an IVF header, else 0. */
int  vp9h_ivf_probe(const uint8_t *buf, size_t size);
/* ivfdec.c read_header (:36-77): AVERROR_INVALIDDATA for a zero time base. */
int  vp9h_ivf_read_header(const uint8_t *buf, size_t size, vp9h_ivf_header *h);
/* ivfdec.c read_packet (:79-90): the frame at *pos (32 = the first), advancing *pos.
 * Returns 0, or VP9HIP_EOF at the end; a short last frame sets *truncated. */
int  vp9h_ivf_read_frame(const uint8_t *buf, size_t size, size_t *pos, const uint8_t **data, uint32_t *frame_size,
                         int64_t *pts, int *truncated);
/* ivfenc.c write_header (:54-73) with fourcc VP90, and write_packet's frame header (:75-88). */
int  vp9h_ivf_write_header(uint8_t out[32], int width, int height, uint32_t time_base_den, uint32_t time_base_num,
                           uint32_t nb_frames);
void vp9h_ivf_write_frame_header(uint8_t out[12], uint32_t frame_size, int64_t pts);

/* ---- WebM / Matroska demux of a VP9 track (libavformat/matroskadec.c) -- */
typedef struct vp9h_webm_info {
    char     doctype[16];          /* "webm" / "matroska" (EBML DocType)                     */
    char     codec_id[32];         /* "V_VP9"                                                */
    uint64_t track;                /* TrackNumber of the first VP9 video track               */
    int32_t  width, height;        /* PixelWidth / PixelHeight                               */
    uint64_t timecode_scale;       /* ns per timecode unit (Info TimecodeScale, 1000000)     */
} vp9h_webm_info;
/* Reading position (opaque to callers beyond zero-initialisation by read_header). */
typedef struct vp9h_webm_cursor {
    uint64_t pos, seg_end, cluster_end, track;
    int64_t  cluster_tc, block_pts, block_duration;
    int32_t  cluster_unknown, keyframe;
    int32_t  nlaces, lace_idx;
    uint64_t lace_pos;
    uint32_t lace_size[256];
} vp9h_webm_cursor;
/* matroska_probe (matroskadec.c:1614-1660): 100 for an EBML header with a matroska / webm
 * DocType, 50 for another EBML document, else 0. */
int  vp9h_webm_probe(const uint8_t *buf, size_t size);
/* matroska_read_header (matroskadec.c:3303-3490): EBML header checks, Info, the first
 * VP9 video track; *cur then points at the first Cluster. AVERROR_INVALIDDATA if there
 * is no V_VP9 track or the header is malformed. */
int  vp9h_webm_read_header(const uint8_t *buf, size_t size, vp9h_webm_info *info, vp9h_webm_cursor *cur);
/* matroska_read_packet: the next frame (one lace of a SimpleBlock / Block of the track),
 * pts in timecode units (INT64_MIN: none), keyframe flag (SimpleBlock; -1 unknown).
 * Returns 0, VP9HIP_EOF at the end, or AVERROR_INVALIDDATA. */
int  vp9h_webm_read_frame(const uint8_t *buf, size_t size, vp9h_webm_cursor *cur, const uint8_t **data,
                          uint32_t *frame_size, int64_t *pts, int *keyframe);
/* The Colour element (0x55B0) of the first VP9 video track: what the VP9 header does not carry
 * (transfer function, primaries, mastering levels) and what it does (matrix, range). The codes
 * are those of ISO/IEC 23091-2 as Matroska stores them (transfer 16 = PQ, 18 = HLG, 1 = BT.709,
 * 13 = sRGB; primaries 9 = BT.2020, 1 = BT.709, 5 = BT.601 625, 6 = BT.601 525; range 1 =
 * limited, 2 = full). An absent field is 2 ("unspecified") for matrix, transfer and primaries
 * and 0 for the others; an absent element is not an error and leaves present = 0. */
typedef struct vp9h_webm_colour {
    int32_t present;               /* the track has a Colour element                         */
    int32_t matrix;                /* MatrixCoefficients 0x55B1                              */
    int32_t bits_per_channel;      /* BitsPerChannel 0x55B2                                  */
    int32_t range;                 /* Range 0x55B9                                           */
    int32_t transfer;              /* TransferCharacteristics 0x55BA                         */
    int32_t primaries;             /* Primaries 0x55BB                                       */
    int32_t max_cll, max_fall;     /* MaxCLL 0x55BC, MaxFALL 0x55BD, cd/m^2                  */
    double  luminance_max;         /* MasteringMetadata (0x55D0) LuminanceMax 0x55D9, cd/m^2 */
    double  luminance_min;         /* LuminanceMin 0x55DA                                    */
} vp9h_webm_colour;
/* Reads it from the file's header (up to the first Cluster). Returns 0, VP9HIP_EINVAL for a
 * NULL argument, or AVERROR_INVALIDDATA as vp9h_webm_read_header does (no V_VP9 track, a
 * truncated or oversize element); never reads past size. */
int  vp9h_webm_read_colour(const uint8_t *buf, size_t size, vp9h_webm_colour *out);

/* ---- bitstream decoder: avcodec_send_packet / avcodec_receive_frame for VP9 -------------
 * The decode loop of vp9_decode_frame (vp9.c:1558-1865) over the host parse (vp9h_stream)
 * and the device path (vp9hip_ctx): superframes split, show_existing_frame, hidden frames,
 * reference slots by refresh mask. Frames are reconstructed in batches of up to
 * max_batch frames (decoder delay, like frame threading); send_packet(NULL) drains.
 * The host parse runs on parse_threads threads ahead of the caller.
 * Errors: VP9HIP_EAGAIN from send_packet = read frames first (no free buffer);
 * from receive_frame = send more input; VP9HIP_EOF after a drain. */
typedef struct vp9hip_decoder vp9hip_decoder;
typedef struct vp9hip_decoder_params {
    int32_t device;
    int32_t max_batch;             /* frames per GPU batch (decoder delay), default 16; the  */
                                   /* decoder holds 8 + (VP9HIP_PIPELINE_SLOTS + 1) max_batch */
                                   /* + extra_bufs buffers                                    */
    int32_t extra_bufs;            /* output frames the caller may hold at once, default 4     */
    int32_t max_width, max_height; /* buffer size; 0: the first keyframe's (larger inter      */
                                   /* frames, e.g. reference scaling up, need it set)         */
    int32_t parse_threads;         /* host parse threads (0: parse in the caller's thread);    */
                                   /* a keyframe starts a new parse chain, so keyframe-only   */
                                   /* streams parse frame-parallel, GOPs GOP-parallel         */
} vp9hip_decoder_params;
typedef struct vp9hip_decoded_frame {
    int32_t buf;                   /* device buffer of vp9hip_decoder_context()              */
    int32_t width, height, bpp, ss_h, ss_v;
    int64_t pts;
    int32_t colorspace, full_range; /* vp9h_frame_info's, of the frame in this buffer         */
} vp9hip_decoded_frame;
void vp9hip_decoder_defaults(vp9hip_decoder_params *p);
int  vp9hip_decoder_open(const vp9hip_decoder_params *p, vp9hip_decoder **out);
void vp9hip_decoder_close(vp9hip_decoder *d);
/* The device context holding the frames: vp9hip_download_frame / vp9hip_frame_device. */
vp9hip_ctx *vp9hip_decoder_context(vp9hip_decoder *d);
int  vp9hip_decoder_send_packet(vp9hip_decoder *d, const uint8_t *data, size_t size, int64_t pts);
/* The next output frame; its buffer stays valid until vp9hip_decoder_release. */
int  vp9hip_decoder_receive_frame(vp9hip_decoder *d, vp9hip_decoded_frame *out);
int  vp9hip_decoder_release(vp9hip_decoder *d, int buf);
/* Convert n received frames (all of one size, colour space and range, else VP9HIP_EINVAL)
 * to `format` (VP9HIP_OUT_*) at dst_dev with vp9hip_convert_frames; pitch / frame_stride as
 * in vp9hip_out_desc. Colour space and range are the frames'; an unknown colour space (code
 * 0 or 6) converts as BT.709. Received frames are complete (receive_frame checked their
 * batch), so this only enqueues on `stream` (NULL: the context's main stream) and returns:
 * the buffers must stay un-released (vp9hip_decoder_release) until the work on `stream` has
 * finished. */
int  vp9hip_decoder_convert(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n, int format,
                            void *dst_dev, int64_t pitch, int64_t frame_stride, void *stream);
/* The same through vp9hip_convert_frames_scaled: the frames resampled to out_width x
 * out_height; pitch / frame_stride describe that output. */
int  vp9hip_decoder_convert_scaled(vp9hip_decoder *dec, const vp9hip_decoded_frame *frames, int n, int format,
                                   int out_width, int out_height, void *dst_dev,
                                   int64_t pitch, int64_t frame_stride, void *stream);
/* The same through vp9hip_convert_frames_resampled; the rectangles are per entry of frames. */
int  vp9hip_decoder_convert_resampled(vp9hip_decoder *dec, const vp9hip_decoded_frame *frames, int n, int format,
                                      const vp9hip_resample *rs, void *dst_dev, int64_t pitch,
                                      int64_t frame_stride, void *stream);
/* The same through vp9hip_convert_frames_bicubic (rs->filter == VP9HIP_FILTER_BICUBIC). */
int  vp9hip_decoder_convert_bicubic(vp9hip_decoder *dec, const vp9hip_decoded_frame *frames, int n, int format,
                                    const vp9hip_resample *rs, void *dst_dev, int64_t pitch,
                                    int64_t frame_stride, void *stream);
/* The same through vp9hip_convert_frames_graded (any filter of rs; a grade made with
 * vp9hip_grade_create on vp9hip_decoder_context), with the stream's matrix and range. */
int  vp9hip_decoder_convert_graded(vp9hip_decoder *dec, const vp9hip_decoded_frame *frames, int n, int format,
                                   const vp9hip_resample *rs, const vp9hip_grade *grade, void *dst_dev,
                                   int64_t pitch, int64_t frame_stride, void *stream);
/* Motion export (see vp9hip_set_export): flags = VP9HIP_EXPORT_MOTION makes every decoded frame,
 * hidden ones included, leave its motion field beside its pixels. Call before the first
 * vp9hip_decoder_send_packet; VP9HIP_EINVAL afterwards. The flags reach the context before it is
 * configured, and again when a new format reconfigures it. */
int  vp9hip_decoder_set_export(vp9hip_decoder *d, int flags);
/* The field of a received frame, in place (device pointers, grid, pitch in cells, as
 * vp9hip_frame_motion): valid while the frame is un-released. Received frames are complete, so
 * this only looks up. A show_existing_frame output returns the field of the frame it shows; a
 * hidden frame's field exists but is handed out only that way. VP9HIP_EINVAL without export or
 * for a frame the caller does not hold. */
int  vp9hip_decoder_frame_motion(vp9hip_decoder *d, const vp9hip_decoded_frame *frame, void **mv, void **info,
                                 int *gw, int *gh, int64_t *pitch_cells);
/* The accumulated motion field of a received frame, in place (as vp9hip_frame_motion_acc), under
 * the rules of vp9hip_decoder_frame_motion: valid while the frame is un-released (the decoder
 * keeps a reference buffer, and with it the parent's plane, while a pending frame reads it), a
 * show_existing_frame output carries the shown buffer's field and serial. Needs
 * VP9HIP_EXPORT_MOTION | VP9HIP_EXPORT_MOTION_ACC in vp9hip_decoder_set_export's flags;
 * VP9HIP_EINVAL without them or for a frame the caller does not hold. */
int  vp9hip_decoder_frame_motion_acc(vp9hip_decoder *d, const vp9hip_decoded_frame *frame, void **acc_dev,
                                     int *gw, int *gh, int64_t *pitch_cells, uint32_t *serial);
/* The residual field of a received frame, in place (as vp9hip_frame_residual), under the rules
 * of vp9hip_decoder_frame_motion: valid while the frame is un-released, a show_existing_frame
 * output returns the field of the frame it shows, hidden frames export too. Needs
 * VP9HIP_EXPORT_RESIDUAL in vp9hip_decoder_set_export's flags; VP9HIP_EINVAL without it or for
 * a frame the caller does not hold. */
int  vp9hip_decoder_frame_residual(vp9hip_decoder *d, const vp9hip_decoded_frame *frame, void *planes[3],
                                   int64_t pitch[3]);
/* The residual tensors of received frames through vp9hip_residual_frames_scaled, under the
 * rules of vp9hip_decoder_metrics: every frame must be of one size, depth and subsampling and
 * held by the caller, else VP9HIP_EINVAL; it only enqueues and releases nothing. With
 * desc->colorspace < 0 the colour space and range are the frames' own: all frames must then
 * share them, and an unknown colour space (0, 6) is treated as BT.709. A show_existing_frame
 * output uses the field of the frame it shows. Needs VP9HIP_EXPORT_RESIDUAL in
 * vp9hip_decoder_set_export's flags. */
int  vp9hip_decoder_residual_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n,
                                    const vp9hip_resid_desc *desc, void *dst_dev, void *stream);
/* The motion tensors of received frames through vp9hip_motion_frames_scaled, under the rules
 * of vp9hip_decoder_residual_scaled: every frame must be of one size and held by the caller, else
 * VP9HIP_EINVAL; desc's width and height are not read but taken from the frames; it only
 * enqueues and releases nothing. A show_existing_frame output uses the shown buffer's field, as
 * vp9hip_decoder_frame_motion_acc does. Needs VP9HIP_EXPORT_MOTION in
 * vp9hip_decoder_set_export's flags, and VP9HIP_EXPORT_MOTION_ACC for VP9HIP_MVT_ACC. */
int  vp9hip_decoder_motion_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n,
                                  const vp9hip_mvt_desc *desc, void *dst_dev, void *stream);
/* The metrics of the pairs (frames_a[i], frames_b[i]) of received frames through
 * vp9hip_frame_metrics, under the rules of vp9hip_decoder_convert: every frame of both arrays
 * must be of one size, depth and subsampling and held by the caller, else VP9HIP_EINVAL; the size
 * compared is the frames' own; frames_b may be NULL; it only enqueues. It releases nothing:
 * consecutive-frame use needs the same frame as b of one pair and a of the next. */
int  vp9hip_decoder_metrics(vp9hip_decoder *d, const vp9hip_decoded_frame *frames_a,
                            const vp9hip_decoded_frame *frames_b, int n,
                            int64_t *out_dev, int32_t *cells_dev, void *stream);
/* The histograms of received frames through vp9hip_frame_histograms, under the rules of
 * vp9hip_decoder_metrics: every frame must be of one size, depth and subsampling and held by
 * the caller (a released frame is VP9HIP_EINVAL); the size is the frames' own (desc->width /
 * height are not read; desc->rects lie inside it); it only enqueues and releases nothing. With
 * desc->colorspace < 0 the colour space and range are the frames' own, as in
 * vp9hip_decoder_residual_scaled: all frames must then share them, and an unknown colour space
 * (0, 6) is treated as BT.709. */
int  vp9hip_decoder_histograms(vp9hip_decoder *d, const vp9hip_decoded_frame *frames, int n,
                               const vp9hip_hist_desc *desc, int32_t *out_dev, void *stream);
/* The accumulated residual of the pairs (frames_a[i], frames_b[i]) of received frames through
 * vp9hip_acc_warp, under the rules of vp9hip_decoder_metrics: every frame of both arrays must be
 * of one size, depth and subsampling and held by the caller (a released frame is
 * VP9HIP_EINVAL); the size is the frames' own; it only enqueues and releases nothing. A
 * show_existing_frame output uses the shown buffer's field and serial. Needs
 * VP9HIP_EXPORT_MOTION_ACC in vp9hip_decoder_set_export's flags. */
int  vp9hip_decoder_acc_warp(vp9hip_decoder *d, const vp9hip_decoded_frame *frames_a,
                             const vp9hip_decoded_frame *frames_b, int n, int mode, int output,
                             void *dst_dev, uint8_t *mask_dev, void *stream);
/* The accumulated residual at model size of the pairs (frames_a[i], frames_b[i]) of received
 * frames through vp9hip_acc_warp_scaled, under the rules of vp9hip_decoder_acc_warp: every frame
 * of both arrays must be of one size, depth and subsampling and held by the caller; desc's width
 * and height are not read but taken from the frames; a show_existing_frame output uses the shown
 * buffer's field and serial. The colour space and range are those of the frames_a, which must
 * share them, as vp9hip_decoder_residual_scaled with colorspace < 0 (unknown: BT.709); desc's
 * own are not read. It only enqueues and releases nothing. Needs VP9HIP_EXPORT_MOTION_ACC. */
int  vp9hip_decoder_acc_warp_scaled(vp9hip_decoder *d, const vp9hip_decoded_frame *frames_a,
                                    const vp9hip_decoded_frame *frames_b, int n,
                                    const vp9hip_warpt_desc *desc, void *dst_dev, void *stream);
/* The accumulated propagation of the pairs (frames[i], root_serials[i], src item src_index[i]) of
 * received frames through vp9hip_acc_propagate, under the rules of vp9hip_decoder_acc_warp: every
 * frame must be of one size and held by the caller; desc's width and height are not read but
 * taken from the frames; a show_existing_frame output uses the shown buffer's field. The root
 * needs no frame: its serial is enough, also after the caller released it. It only enqueues and
 * releases nothing. Needs VP9HIP_EXPORT_MOTION_ACC. */
int  vp9hip_decoder_acc_propagate(vp9hip_decoder *d, const vp9hip_decoded_frame *frames,
                                  const uint32_t *root_serials, const int *src_index, int n, int m,
                                  const vp9hip_prop_desc *desc, const void *src_dev, void *dst_dev,
                                  uint8_t *valid_dev, void *stream);
/* avcodec_flush_buffers: drop queued frames and reference state (seek). */
int  vp9hip_decoder_flush(vp9hip_decoder *d);

#ifdef __cplusplus
}
#endif
#endif /* VP9HIP_H */
