"""MI355X VP9 hybrid decoder — Python host bindings.

The product is the C-ABI shared library ``libvp9hip.so`` (include/vp9hip.h): host
runtime + gfx950 HIP kernels for the VP9 pixel path (inverse transforms, intra
prediction, motion compensation, loop filter). This module only binds it with
ctypes and mirrors the reference's decode API for this path
(``avcodec_send_packet`` / ``avcodec_receive_frame``, libavcodec/avcodec.c:707-717;
the VP9 decoder's frame loop vp9.c:1606-1863) at the pass-1 packet level.

There is no CPU fallback: if the HIP library cannot be loaded, every entry point
raises :class:`Vp9HipUnavailable`.
"""
import collections
import ctypes
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvp9hip.so")

# AVERROR codes (include/vp9hip.h)
EINVAL = -22
ENOMEM = -12
ENOSYS = -38
EAGAIN = -11
EOF = -541478725
EINVALIDDATA = -1094995529
EEXTERNAL = -542398533
EBUG = -558323010

BS_64x64, BS_64x32, BS_32x64, BS_32x32, BS_32x16, BS_16x32, BS_16x16, BS_16x8, BS_8x16, \
    BS_8x8, BS_8x4, BS_4x8, BS_4x4 = range(13)


class Vp9HipUnavailable(RuntimeError):
    pass


class Vp9HipError(RuntimeError):
    def __init__(self, fn, code):
        super().__init__("%s failed with AVERROR %d" % (fn, code))
        self.code = code


class Block(ctypes.Structure):
    """vp9h_block (include/vp9hip.h) == VP9Block (vp9dec.h:89-97)."""
    _fields_ = [("row", ctypes.c_uint16), ("col", ctypes.c_uint16), ("bs", ctypes.c_uint8),
                ("tx", ctypes.c_uint8), ("uvtx", ctypes.c_uint8), ("skip", ctypes.c_uint8),
                ("intra", ctypes.c_uint8), ("comp", ctypes.c_uint8), ("seg_id", ctypes.c_uint8),
                ("filter", ctypes.c_uint8), ("mode", ctypes.c_uint8 * 4), ("uvmode", ctypes.c_uint8),
                ("ref", ctypes.c_uint8 * 2), ("pad0", ctypes.c_uint8),
                ("mv", ctypes.c_int16 * 16)]


class FramePacket(ctypes.Structure):
    """vp9h_frame: one pass-1 frame packet."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bpp", ctypes.c_uint8),
                ("ss_h", ctypes.c_uint8), ("ss_v", ctypes.c_uint8), ("keyframe", ctypes.c_uint8),
                ("intraonly", ctypes.c_uint8), ("lossless", ctypes.c_uint8),
                ("filter_level", ctypes.c_uint8), ("sharpness", ctypes.c_uint8),
                ("log2_tile_cols", ctypes.c_uint8), ("log2_tile_rows", ctypes.c_uint8),
                ("pad0", ctypes.c_uint8 * 2), ("lflvl", ctypes.c_uint8 * 64),
                ("ref_w", ctypes.c_int32 * 3), ("ref_h", ctypes.c_int32 * 3),
                ("nblocks", ctypes.c_uint32), ("neobs", ctypes.c_uint32), ("ncoefs", ctypes.c_uint64),
                ("blocks", ctypes.POINTER(Block)), ("eobs", ctypes.POINTER(ctypes.c_uint16)),
                ("coefs", ctypes.c_void_p)]


class SegParams(ctypes.Structure):
    """vp9h_seg_params: segmentation and LF deltas in effect for a frame."""
    _fields_ = [("enabled", ctypes.c_int32), ("update_map", ctypes.c_int32), ("temporal", ctypes.c_int32),
                ("update_data", ctypes.c_int32), ("abs_delta", ctypes.c_int32), ("q_en", ctypes.c_int32),
                ("lf_en", ctypes.c_int32), ("q", ctypes.c_int32 * 8), ("lf", ctypes.c_int32 * 8),
                ("nseg", ctypes.c_int32), ("lf_delta_update", ctypes.c_int32), ("lf_ref", ctypes.c_int32 * 4),
                ("lf_mode", ctypes.c_int32 * 2)]


def seg_params(**kw):
    """A SegParams from keyword fields (lists for q / lf / lf_ref / lf_mode)."""
    p = SegParams()
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k in ("q", "lf", "lf_ref", "lf_mode"):
            v = (ctypes.c_int32 * {"q": 8, "lf": 8, "lf_ref": 4, "lf_mode": 2}[k])(*v)
        setattr(p, k, v)
    return p


class SynthParams(ctypes.Structure):
    """vp9h_synth_params."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bpp", ctypes.c_int32),
                ("ss_h", ctypes.c_int32), ("ss_v", ctypes.c_int32), ("log2_tile_cols", ctypes.c_int32),
                ("inter", ctypes.c_int32), ("compound", ctypes.c_int32), ("q_idx", ctypes.c_int32),
                ("lossless", ctypes.c_int32), ("filter_level", ctypes.c_int32),
                ("sharpness", ctypes.c_int32), ("bilinear", ctypes.c_int32),
                ("coef_stress", ctypes.c_int32), ("p_zero_eob", ctypes.c_float),
                ("p_skip", ctypes.c_float), ("seed", ctypes.c_uint64), ("seg", SegParams),
                ("eob_dense", ctypes.c_int32), ("ref_mix", ctypes.c_int32), ("mv_range", ctypes.c_int32),
                ("edge_large", ctypes.c_int32), ("p_intra", ctypes.c_float)]


class FrameInfo(ctypes.Structure):
    """vp9h_frame_info: the frame header's reference bookkeeping."""
    _fields_ = [("show_existing_frame", ctypes.c_int32), ("show_slot", ctypes.c_int32),
                ("show_frame", ctypes.c_int32), ("refresh_mask", ctypes.c_int32),
                ("ref_slot", ctypes.c_int32 * 3), ("sign_bias", ctypes.c_int32 * 3),
                ("error_res", ctypes.c_int32), ("refresh_ctx", ctypes.c_int32), ("parallel", ctypes.c_int32),
                ("ctx_id", ctypes.c_int32), ("allow_hp", ctypes.c_int32), ("interp", ctypes.c_int32),
                ("comp_mode", ctypes.c_int32), ("tx_mode", ctypes.c_int32),
                ("header_size", ctypes.c_uint32), ("compressed_header_size", ctypes.c_uint32),
                ("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32)]


class EncParams(ctypes.Structure):
    """vp9h_enc_params: the encoder's per-frame choices."""
    _fields_ = [("base_q_idx", ctypes.c_int32), ("show_existing_frame", ctypes.c_int32),
                ("show_slot", ctypes.c_int32), ("show_frame", ctypes.c_int32), ("error_res", ctypes.c_int32),
                ("refresh_mask", ctypes.c_int32), ("ref_slot", ctypes.c_int32 * 3),
                ("sign_bias", ctypes.c_int32 * 3), ("refresh_ctx", ctypes.c_int32), ("parallel", ctypes.c_int32),
                ("ctx_id", ctypes.c_int32), ("reset_ctx", ctypes.c_int32), ("allow_hp", ctypes.c_int32),
                ("interp", ctypes.c_int32), ("comp_mode", ctypes.c_int32), ("tx_mode", ctypes.c_int32),
                ("prob_updates", ctypes.c_int32), ("keep_modes", ctypes.c_int32), ("seg", SegParams)]


_lib_handle = None
# torch's ROCm wheel ships its own libamdhip64 under the same soname as /opt/rocm's, which
# libvp9hip.so links: whichever process loads first serves both. torch's device init fails
# ("No HIP GPUs are available") on the newer /opt/rocm runtime, so torch interop
# (frame_tensors) needs torch imported before this library is loaded.
_torch_first = False

ABI_VERSION = 5               # VP9HIP_ABI_VERSION of include/vp9hip.h these bindings mirror
PIPELINE_SLOTS = 3             # VP9HIP_PIPELINE_SLOTS: batch slots the decoder / adapter rotate
# Exported symbols of include/vp9hip.h (checked by the CPU test suite).
ABI_SYMBOLS = ["vp9hip_open", "vp9hip_close", "vp9hip_configure", "vp9hip_submit_frame",
               "vp9hip_stage_batch", "vp9hip_stage_batch_refs", "vp9hip_run_batch", "vp9hip_sync",
               "vp9hip_download_frame",
               "vp9hip_upload_frame", "vp9hip_flush", "vp9hip_last_timing", "vp9hip_set_timing",
               "vp9hip_alg_bytes", "vp9hip_plan_stats", "vp9hip_plan_sb_costs", "vp9hip_abi_version", "vp9hip_set_graph",
               "vp9hip_stage_batch_tiles", "vp9hip_batch_phases", "vp9hip_phase_frames", "vp9hip_run_phase",
               "vp9hip_stripe", "vp9hip_frame_device", "vp9hip_batch_groups", "vp9hip_set_batch_slot", "vp9hip_sync_slot", "vp9hip_slot_busy",
               "vp9hip_fill_buffers", "vp9hip_device_info", "vp9hip_test_hooks", "vp9hip_batch_frame_status",
               "vp9h_decode_frame", "vp9h_encode_frame", "vp9h_frame_free", "vp9h_buffer_free",
               "vp9h_stream_open", "vp9h_stream_close", "vp9h_stream_set_threads", "vp9h_stream_decode", "vp9h_stream_encode",
               "vp9h_enc_defaults", "vp9h_superframe_split", "vp9h_frame_type", "vp9h_frame_peek",
               "vp9hip_slot_stream_wait",
               "vp9hip_synth_defaults", "vp9hip_synth_frame", "vp9hip_synth_free",
               "vp9h_ivf_probe", "vp9h_ivf_read_header", "vp9h_ivf_read_frame", "vp9h_ivf_write_header",
               "vp9h_ivf_write_frame_header", "vp9h_webm_probe", "vp9h_webm_read_header", "vp9h_webm_read_frame",
               "vp9hip_decoder_defaults", "vp9hip_decoder_open", "vp9hip_decoder_close", "vp9hip_decoder_context",
               "vp9hip_decoder_send_packet", "vp9hip_decoder_receive_frame", "vp9hip_decoder_release",
               "vp9hip_decoder_flush",
               "vp9h_stream_set_color", "vp9hip_out_layout", "vp9hip_out_coefs", "vp9hip_convert_frames",
               "vp9hip_decoder_convert", "vp9hip_convert_frames_scaled", "vp9hip_decoder_convert_scaled",
               "vp9hip_convert_frames_resampled", "vp9hip_decoder_convert_resampled", "vp9hip_resample_weights",
               "vp9hip_convert_frames_bicubic", "vp9hip_decoder_convert_bicubic", "vp9hip_bicubic_weights",
               "vp9hip_frame_metrics", "vp9hip_frame_metrics_host", "vp9hip_decoder_metrics",
               "vp9hip_resid_layout", "vp9hip_residual_frames_scaled", "vp9hip_residual_scaled_host",
               "vp9hip_decoder_residual_scaled",
               "vp9hip_mvt_layout", "vp9hip_motion_frames_scaled", "vp9hip_motion_scaled_host",
               "vp9hip_decoder_motion_scaled",
               "vp9hip_warp_layout", "vp9hip_acc_warp", "vp9hip_acc_warp_host", "vp9hip_warp_launch_dev",
               "vp9hip_decoder_acc_warp",
               "vp9hip_warpt_layout", "vp9hip_acc_warp_scaled", "vp9hip_acc_warp_scaled_host",
               "vp9hip_warp_scale_launch_dev", "vp9hip_decoder_acc_warp_scaled",
               "vp9hip_prop_layout", "vp9hip_acc_propagate", "vp9hip_acc_propagate_host", "vp9hip_prop_launch_dev",
               "vp9hip_decoder_acc_propagate",
               "vp9hip_grade_create", "vp9hip_grade_destroy", "vp9hip_convert_frames_graded",
               "vp9hip_decoder_convert_graded", "vp9hip_grade_host", "vp9h_webm_read_colour",
               "vp9hip_frame_histograms", "vp9hip_frame_histograms_host", "vp9hip_decoder_histograms"]


def lib():
    """Load libvp9hip.so (fails loudly: there is no CPU fallback)."""
    global _lib_handle
    if _lib_handle is not None:
        return _lib_handle
    if not os.path.exists(LIB_PATH):
        raise Vp9HipUnavailable("libvp9hip.so not built: run __graft_entry__.build() (%s)" % LIB_PATH)
    global _torch_first
    _torch_first = "torch" in sys.modules
    L = ctypes.CDLL(LIB_PATH)
    # the struct mirrors below are the header's of this ABI version (vp9h_synth_params and
    # vp9h_enc_params grew in version 2, vp9h_frame_info and vp9hip_decoded_frame in 3,
    # vp9h_synth_params again in 4 and 5): a
    # library built from another header is refused
    if L.vp9hip_abi_version() != ABI_VERSION:
        raise Vp9HipUnavailable("libvp9hip.so ABI version %d, these bindings need %d: rebuild it (%s)"
                                % (L.vp9hip_abi_version(), ABI_VERSION, LIB_PATH))
    vp = ctypes.c_void_p
    L.vp9hip_open.argtypes = [ctypes.c_int, ctypes.POINTER(vp)]
    L.vp9hip_close.argtypes = [vp]
    L.vp9hip_close.restype = None
    L.vp9hip_configure.argtypes = [vp] + [ctypes.c_int] * 6
    L.vp9hip_submit_frame.argtypes = [vp, ctypes.POINTER(FramePacket), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.vp9hip_stage_batch.argtypes = [vp, ctypes.POINTER(FramePacket), ctypes.c_int, ctypes.POINTER(ctypes.c_int)]
    L.vp9hip_stage_batch_refs.argtypes = [vp, ctypes.POINTER(FramePacket), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                          ctypes.POINTER(ctypes.c_int)]
    L.vp9hip_stage_batch_tiles.argtypes = [vp, ctypes.POINTER(FramePacket), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                           ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.c_int]
    L.vp9hip_batch_phases.argtypes = [vp]
    L.vp9hip_batch_groups.argtypes = [vp]
    L.vp9hip_set_batch_slot.argtypes = [vp, ctypes.c_int]
    L.vp9hip_sync_slot.argtypes = [vp, ctypes.c_int]
    L.vp9hip_batch_frame_status.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.vp9hip_slot_busy.argtypes = [vp, ctypes.c_int]
    L.vp9hip_phase_frames.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.vp9hip_run_phase.argtypes = [vp, ctypes.c_int, ctypes.c_int]
    L.vp9hip_stripe.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    L.vp9hip_stripe.restype = ctypes.c_int64
    L.vp9hip_frame_device.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_ssize_t),
                                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_void_p)]
    L.vp9hip_device_info.argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.c_char_p, ctypes.c_int]
    L.vp9hip_fill_buffers.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.vp9hip_test_hooks.argtypes = [ctypes.c_int, ctypes.c_uint32]
    L.vp9hip_test_hooks.restype = None
    L.vp9hip_run_batch.argtypes = [vp]
    L.vp9hip_sync.argtypes = [vp]
    L.vp9hip_download_frame.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                        ctypes.POINTER(ctypes.c_ssize_t)]
    L.vp9hip_upload_frame.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_ssize_t)]
    L.vp9hip_flush.argtypes = [vp]
    L.vp9hip_last_timing.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_double),
                                     ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    L.vp9hip_alg_bytes.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
    L.vp9hip_set_timing.argtypes = [vp, ctypes.c_int]
    L.vp9hip_synth_defaults.argtypes = [ctypes.POINTER(SynthParams), ctypes.c_int, ctypes.c_int, ctypes.c_int]
    L.vp9hip_synth_defaults.restype = None
    L.vp9hip_synth_frame.argtypes = [ctypes.POINTER(FramePacket), ctypes.POINTER(SynthParams)]
    L.vp9hip_synth_free.argtypes = [ctypes.POINTER(FramePacket)]
    L.vp9hip_synth_free.restype = None
    L.vp9h_decode_frame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(FramePacket)]
    L.vp9h_encode_frame.argtypes = [ctypes.POINTER(FramePacket), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p),
                                    ctypes.POINTER(ctypes.c_size_t)]
    L.vp9h_frame_free.argtypes = [ctypes.POINTER(FramePacket)]
    L.vp9h_frame_free.restype = None
    L.vp9h_buffer_free.argtypes = [ctypes.c_void_p]
    L.vp9h_buffer_free.restype = None
    L.vp9h_stream_open.argtypes = [ctypes.POINTER(ctypes.c_void_p)]
    L.vp9h_stream_set_threads.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.vp9h_stream_close.argtypes = [ctypes.c_void_p]
    L.vp9h_stream_close.restype = None
    L.vp9h_stream_decode.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(FramePacket),
                                     ctypes.POINTER(FrameInfo)]
    L.vp9h_stream_encode.argtypes = [ctypes.c_void_p, ctypes.POINTER(FramePacket), ctypes.POINTER(EncParams),
                                     ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.POINTER(FramePacket)]
    L.vp9h_enc_defaults.argtypes = [ctypes.POINTER(EncParams)]
    L.vp9h_enc_defaults.restype = None
    L.vp9h_superframe_split.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                        ctypes.POINTER(ctypes.c_size_t), ctypes.c_int]
    L.vp9h_frame_type.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    L.vp9h_frame_peek.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(FrameInfo)]
    L.vp9hip_slot_stream_wait.argtypes = [vp, ctypes.c_int, ctypes.c_void_p]
    L.vp9h_ivf_probe.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    L.vp9h_ivf_read_header.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(IvfHeader)]
    L.vp9h_ivf_read_frame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                      ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32),
                                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    L.vp9h_ivf_write_header.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32,
                                        ctypes.c_uint32]
    L.vp9h_ivf_write_frame_header.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int64]
    L.vp9h_ivf_write_frame_header.restype = None
    L.vp9h_webm_probe.argtypes = [ctypes.c_void_p, ctypes.c_size_t]
    L.vp9h_webm_read_header.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(WebmInfo),
                                        ctypes.POINTER(WebmCursor)]
    L.vp9h_webm_read_frame.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(WebmCursor),
                                       ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint32),
                                       ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int)]
    L.vp9hip_decoder_defaults.argtypes = [ctypes.POINTER(DecoderParams)]
    L.vp9hip_decoder_defaults.restype = None
    L.vp9hip_decoder_open.argtypes = [ctypes.POINTER(DecoderParams), ctypes.POINTER(vp)]
    L.vp9hip_decoder_close.argtypes = [vp]
    L.vp9hip_decoder_close.restype = None
    L.vp9hip_decoder_context.argtypes = [vp]
    L.vp9hip_decoder_context.restype = vp
    L.vp9hip_decoder_send_packet.argtypes = [vp, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int64]
    L.vp9hip_decoder_receive_frame.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo)]
    L.vp9hip_decoder_release.argtypes = [vp, ctypes.c_int]
    L.vp9hip_decoder_flush.argtypes = [vp]
    L.vp9h_stream_set_color.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    L.vp9hip_out_layout.argtypes = [ctypes.POINTER(OutDesc), ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                    ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_out_layout.restype = ctypes.c_int64
    L.vp9hip_out_coefs.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int32)]
    L.vp9hip_convert_frames.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(OutDesc),
                                        ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_convert.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int, ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_void_p]
    L.vp9hip_convert_frames_scaled.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(OutDesc),
                                               ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_convert_scaled.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int, ctypes.c_int,
                                                ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                                                ctypes.c_int64, ctypes.c_void_p]
    L.vp9hip_convert_frames_resampled.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(OutDesc),
                                                  ctypes.POINTER(Resample), ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_convert_resampled.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int, ctypes.c_int,
                                                   ctypes.POINTER(Resample), ctypes.c_void_p, ctypes.c_int64,
                                                   ctypes.c_int64, ctypes.c_void_p]
    L.vp9hip_resample_weights.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32),
                                                                ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_convert_frames_bicubic.argtypes = L.vp9hip_convert_frames_resampled.argtypes
    L.vp9hip_decoder_convert_bicubic.argtypes = L.vp9hip_decoder_convert_resampled.argtypes
    L.vp9hip_grade_create.argtypes = [vp, ctypes.POINTER(GradeDesc), ctypes.POINTER(vp)]
    L.vp9hip_grade_destroy.argtypes = [vp]
    L.vp9hip_grade_destroy.restype = None
    L.vp9hip_convert_frames_graded.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(OutDesc),
                                               ctypes.POINTER(Resample), vp, ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_convert_graded.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int, ctypes.c_int,
                                                ctypes.POINTER(Resample), vp, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64,
                                                ctypes.c_void_p]
    L.vp9hip_grade_host.argtypes = [ctypes.POINTER(GradeDesc), ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    L.vp9h_webm_read_colour.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(WebmColour)]
    L.vp9hip_bicubic_weights.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int32),
                                                               ctypes.c_int, ctypes.POINTER(ctypes.c_int64),
                                                               ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_resid4_host.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    L.vp9hip_residn_host.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3
    L.vp9hip_intra_job_host.argtypes = [ctypes.c_int] * 15 + [ctypes.POINTER(ctypes.c_int32)]
    L.vp9hip_intra_job_dev.argtypes = [ctypes.c_int] * 13 + [ctypes.POINTER(ctypes.c_int32)]
    L.vp9hip_plan_sched_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    L.vp9hip_plan_heights_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 2
    L.vp9hip_plan_emit_host.argtypes = [ctypes.c_int] * 3 + [ctypes.c_void_p] * 4
    L.vp9hip_test_plan_records.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int)] + [ctypes.c_void_p] * 4
    # motion export
    L.vp9hip_set_export.argtypes = [vp, ctypes.c_int]
    L.vp9hip_frame_motion.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                      ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_void_p)]
    L.vp9hip_download_motion.argtypes = [vp, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_motion_host.argtypes = [ctypes.POINTER(FramePacket), ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_motion_launch_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                           ctypes.c_void_p]
    L.vp9hip_decoder_set_export.argtypes = [vp, ctypes.c_int]
    L.vp9hip_decoder_frame_motion.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.POINTER(ctypes.c_void_p),
                                              ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_int),
                                              ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int64)]
    # accumulated motion
    u32p, ip = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_int)
    L.vp9hip_frame_motion_acc.argtypes = [vp, ctypes.c_int, ctypes.POINTER(ctypes.c_void_p), ip, ip,
                                          ctypes.POINTER(ctypes.c_int64), u32p, ctypes.POINTER(ctypes.c_void_p)]
    L.vp9hip_download_motion_acc.argtypes = [vp, ctypes.c_int, ctypes.c_void_p, u32p]
    L.vp9hip_motion_acc_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint32,
                                         ctypes.POINTER(ctypes.c_void_p * 3), ctypes.POINTER(ctypes.c_int * 3),
                                         ctypes.c_void_p]
    L.vp9hip_mvacc_launch_dev.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                          ctypes.c_void_p, ip, ctypes.c_int, ctypes.c_void_p]
    L.vp9hip_decoder_frame_motion_acc.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.POINTER(ctypes.c_void_p),
                                                  ip, ip, ctypes.POINTER(ctypes.c_int64), u32p]
    # residual export
    i64p3, vp3 = ctypes.POINTER(ctypes.c_int64 * 3), ctypes.POINTER(ctypes.c_void_p * 3)
    L.vp9hip_frame_residual.argtypes = [vp, ctypes.c_int, vp3, i64p3, ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_void_p)]
    L.vp9hip_download_residual.argtypes = [vp, ctypes.c_int, vp3, ctypes.POINTER(ctypes.c_ssize_t * 3)]
    L.vp9hip_residual_host.argtypes = [ctypes.POINTER(FramePacket), vp3, ctypes.POINTER(ctypes.c_ssize_t * 3),
                                       ctypes.POINTER(ctypes.c_int * 3)]
    L.vp9hip_residual_relaunch.argtypes = [vp, ctypes.c_void_p]
    L.vp9hip_decoder_frame_residual.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), vp3, i64p3]
    # residual tensors at model size
    L.vp9hip_resid_layout.restype = ctypes.c_int64
    L.vp9hip_resid_layout.argtypes = [ctypes.POINTER(ResidDesc), ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_residual_frames_scaled.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ResidDesc),
                                                ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_residual_scaled_host.argtypes = [vp3, ctypes.POINTER(ctypes.c_ssize_t * 3)] + [ctypes.c_int] * 5 + \
                                             [ctypes.POINTER(ResidDesc), ctypes.c_void_p]
    L.vp9hip_decoder_residual_scaled.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int,
                                                 ctypes.POINTER(ResidDesc), ctypes.c_void_p, ctypes.c_void_p]
    # motion tensors at model size
    L.vp9hip_mvt_layout.restype = ctypes.c_int64
    L.vp9hip_mvt_layout.argtypes = [ctypes.POINTER(MvtDesc), ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_motion_frames_scaled.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(MvtDesc),
                                              ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_motion_scaled_host.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ssize_t,
                                            ctypes.POINTER(MvtDesc), ctypes.c_void_p]
    L.vp9hip_decoder_motion_scaled.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int,
                                               ctypes.POINTER(MvtDesc), ctypes.c_void_p, ctypes.c_void_p]
    # frame metrics
    L.vp9hip_frame_metrics.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                       ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_frame_metrics_host.argtypes = [vp3, ctypes.POINTER(ctypes.c_ssize_t * 3), vp3, ctypes.POINTER(ctypes.c_ssize_t * 3)] + \
                                           [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_metrics.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.POINTER(DecodedFrameInfo), ctypes.c_int,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # frame histograms
    L.vp9hip_frame_histograms.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(HistDesc),
                                          ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_frame_histograms_host.argtypes = [vp3, ctypes.POINTER(ctypes.c_ssize_t * 3)] + [ctypes.c_int] * 3 + \
                                              [ctypes.POINTER(HistDesc), ctypes.POINTER(Rect), ctypes.c_void_p]
    L.vp9hip_decoder_histograms.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.c_int, ctypes.POINTER(HistDesc),
                                            ctypes.c_void_p, ctypes.c_void_p]
    # accumulated residual
    L.vp9hip_warp_layout.restype = ctypes.c_int64
    L.vp9hip_warp_layout.argtypes = [ctypes.c_int] * 4 + [ctypes.POINTER(ctypes.c_int64 * 3)]
    L.vp9hip_acc_warp.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)] + [ctypes.c_int] * 5 + \
                                 [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_acc_warp_host.argtypes = [vp3, ctypes.POINTER(ctypes.c_ssize_t * 3), vp3, ctypes.POINTER(ctypes.c_ssize_t * 3),
                                       ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_int] * 7 + \
                                      [ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_warp_launch_dev.argtypes = [ctypes.POINTER(ctypes.c_void_p)] * 3 + [u32p, ctypes.c_int,
                                         ctypes.POINTER(ctypes.c_int64 * 3), ctypes.POINTER(ctypes.c_int32 * 2),
                                         ctypes.c_int64] + [ctypes.c_int] * 7 + \
                                        [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_acc_warp.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.POINTER(DecodedFrameInfo)] + \
                                         [ctypes.c_int] * 3 + [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    # accumulated residual at model size
    L.vp9hip_warpt_layout.restype = ctypes.c_int64
    L.vp9hip_warpt_layout.argtypes = [ctypes.POINTER(WarptDesc), ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_acc_warp_scaled.argtypes = [vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                         ctypes.POINTER(WarptDesc), ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_acc_warp_scaled_host.argtypes = [vp3, ctypes.POINTER(ctypes.c_ssize_t * 3), vp3, ctypes.POINTER(ctypes.c_ssize_t * 3),
                                              ctypes.c_void_p, ctypes.c_uint32] + [ctypes.c_int] * 3 + \
                                             [ctypes.POINTER(WarptDesc), ctypes.c_void_p]
    L.vp9hip_warp_scale_launch_dev.argtypes = [ctypes.POINTER(ctypes.c_void_p)] * 3 + [u32p, ctypes.c_int,
                                               ctypes.POINTER(ctypes.c_int64 * 3), ctypes.POINTER(ctypes.c_int32 * 2),
                                               ctypes.c_int64] + [ctypes.c_int] * 3 + \
                                              [ctypes.POINTER(WarptDesc), ctypes.c_void_p, ctypes.c_void_p]
    L.vp9hip_decoder_acc_warp_scaled.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), ctypes.POINTER(DecodedFrameInfo),
                                                 ctypes.c_int, ctypes.POINTER(WarptDesc), ctypes.c_void_p, ctypes.c_void_p]
    # accumulated propagation
    L.vp9hip_prop_layout.restype = ctypes.c_int64
    L.vp9hip_prop_layout.argtypes = [ctypes.POINTER(PropDesc), ctypes.POINTER(ctypes.c_int64)]
    L.vp9hip_acc_propagate.argtypes = [vp, ctypes.POINTER(ctypes.c_int), u32p, ctypes.POINTER(ctypes.c_int), ctypes.c_int,
                                       ctypes.c_int, ctypes.POINTER(PropDesc)] + [ctypes.c_void_p] * 4
    L.vp9hip_acc_propagate_host.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.POINTER(PropDesc)] + [ctypes.c_void_p] * 3
    L.vp9hip_prop_launch_dev.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.c_int64, u32p, ctypes.POINTER(ctypes.c_int),
                                         ctypes.c_int, ctypes.c_int, ctypes.POINTER(PropDesc)] + [ctypes.c_void_p] * 4
    L.vp9hip_decoder_acc_propagate.argtypes = [vp, ctypes.POINTER(DecodedFrameInfo), u32p, ctypes.POINTER(ctypes.c_int),
                                               ctypes.c_int, ctypes.c_int, ctypes.POINTER(PropDesc)] + [ctypes.c_void_p] * 4
    _lib_handle = L
    return L


class IvfHeader(ctypes.Structure):
    _fields_ = [("fourcc", ctypes.c_char * 5), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("time_base_den", ctypes.c_uint32), ("time_base_num", ctypes.c_uint32),
                ("nb_frames", ctypes.c_uint32), ("header_size", ctypes.c_uint32)]


class WebmInfo(ctypes.Structure):
    _fields_ = [("doctype", ctypes.c_char * 16), ("codec_id", ctypes.c_char * 32), ("track", ctypes.c_uint64),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("timecode_scale", ctypes.c_uint64)]


class WebmCursor(ctypes.Structure):
    _fields_ = [("pos", ctypes.c_uint64), ("seg_end", ctypes.c_uint64), ("cluster_end", ctypes.c_uint64),
                ("track", ctypes.c_uint64), ("cluster_tc", ctypes.c_int64), ("block_pts", ctypes.c_int64),
                ("block_duration", ctypes.c_int64), ("cluster_unknown", ctypes.c_int32), ("keyframe", ctypes.c_int32),
                ("nlaces", ctypes.c_int32), ("lace_idx", ctypes.c_int32), ("lace_pos", ctypes.c_uint64),
                ("lace_size", ctypes.c_uint32 * 256)]


class WebmColour(ctypes.Structure):
    """vp9h_webm_colour: the Colour element of the first VP9 video track."""
    _fields_ = [("present", ctypes.c_int32), ("matrix", ctypes.c_int32), ("bits_per_channel", ctypes.c_int32),
                ("range", ctypes.c_int32), ("transfer", ctypes.c_int32), ("primaries", ctypes.c_int32),
                ("max_cll", ctypes.c_int32), ("max_fall", ctypes.c_int32), ("luminance_max", ctypes.c_double),
                ("luminance_min", ctypes.c_double)]


class DecoderParams(ctypes.Structure):
    _fields_ = [("device", ctypes.c_int32), ("max_batch", ctypes.c_int32), ("extra_bufs", ctypes.c_int32),
                ("max_width", ctypes.c_int32), ("max_height", ctypes.c_int32), ("parse_threads", ctypes.c_int32)]


class DecodedFrameInfo(ctypes.Structure):
    _fields_ = [("buf", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("bpp", ctypes.c_int32), ("ss_h", ctypes.c_int32), ("ss_v", ctypes.c_int32),
                ("pts", ctypes.c_int64), ("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32)]


class OutDesc(ctypes.Structure):
    """vp9hip_out_desc: the format and layout of converted frames."""
    _fields_ = [("format", ctypes.c_int32), ("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("pitch", ctypes.c_int64),
                ("frame_stride", ctypes.c_int64)]


class ResidDesc(ctypes.Structure):
    """vp9hip_resid_desc: the format and layout of residual tensors at model size."""
    _fields_ = [("format", ctypes.c_int32), ("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32), ("pitch", ctypes.c_int64),
                ("frame_stride", ctypes.c_int64)]


class WarptDesc(ctypes.Structure):
    """vp9hip_warpt_desc: the format, mode and layout of the accumulated residual at model size."""
    _fields_ = [("format", ctypes.c_int32), ("colorspace", ctypes.c_int32), ("full_range", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("planes", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32), ("pitch", ctypes.c_int64),
                ("frame_stride", ctypes.c_int64)]


class PropDesc(ctypes.Structure):
    """vp9hip_prop_desc: the sizes, element, layout, mode and fill of an accumulated propagation."""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("fw", ctypes.c_int32), ("fh", ctypes.c_int32),
                ("channels", ctypes.c_int32), ("elem_size", ctypes.c_int32), ("layout", ctypes.c_int32),
                ("mode", ctypes.c_int32), ("flags", ctypes.c_int32), ("reserved", ctypes.c_int32), ("fill", ctypes.c_uint64)]


class MvtDesc(ctypes.Structure):
    """vp9hip_mvt_desc: the format, source and layout of motion tensors at model size."""
    _fields_ = [("format", ctypes.c_int32), ("source", ctypes.c_int32), ("planes", ctypes.c_int32),
                ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32), ("pitch", ctypes.c_int64),
                ("frame_stride", ctypes.c_int64)]


class Rect(ctypes.Structure):
    """vp9hip_rect: (x, y, w, h) in luma samples."""
    _fields_ = [("x", ctypes.c_int32), ("y", ctypes.c_int32), ("w", ctypes.c_int32), ("h", ctypes.c_int32)]


class Resample(ctypes.Structure):
    """vp9hip_resample: filter, output size, per-frame rectangles (or NULL) and the fill codes."""
    _fields_ = [("filter", ctypes.c_int32), ("out_width", ctypes.c_int32), ("out_height", ctypes.c_int32),
                ("src_rects", ctypes.POINTER(Rect)), ("dst_rects", ctypes.POINTER(Rect)), ("fill", ctypes.c_int32 * 3)]


class HistDesc(ctypes.Structure):
    """vp9hip_hist_desc: what is counted, the bins, the colour of RGBM, the size and the rectangles (or NULL)."""
    _fields_ = [("what", ctypes.c_int32), ("bins_log2", ctypes.c_int32), ("colorspace", ctypes.c_int32),
                ("full_range", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32),
                ("rects", ctypes.POINTER(Rect))]


class GradeDesc(ctypes.Structure):
    """vp9hip_grade_desc: the depth, the output's largest code and the three host tables."""
    _fields_ = [("bpp", ctypes.c_int32), ("out_max", ctypes.c_int32), ("in_lut", ctypes.c_void_p), ("m", ctypes.c_void_p),
                ("out_lut", ctypes.c_void_p)]


# VP9HIP_OUT_*: the names Device.convert / Decoder.convert take
OUT_FORMATS = {"semiplanar": 0, "rgb24": 1, "rgbp_u8": 2, "rgbp_f16": 3}
# VP9HIP_RESID_*: the names Device.residual_tensors / Decoder.residual_tensors take
RESID_FORMATS = {"yuv_i16": 0, "yuv_f16": 1, "rgb_i16": 2, "rgb_f16": 3}
# VP9HIP_MVT_*: the names Device.motion_tensors / Decoder.motion_tensors take for fmt and source
MVT_FORMATS = {"i16": 0, "f16": 1}
MVT_SOURCES = {"coded": 0, "acc": 1}
# VP9HIP_FILTER_*: the names of their filter argument
FILTERS = {"box": 0, "triangle": 1}
# VP9HIP_HIST_*: the names histograms() takes for what, and their channels
HIST_MODES = {"planes": 0, "rgbm": 1}
HIST_CHANNELS = {"planes": ("y", "u", "v"), "rgbm": ("r", "g", "b", "m")}
# VP9HIP_FILTER_BICUBIC, filter="bicubic": entries of its own (vp9hip_convert_frames_bicubic)
FILTER_BICUBIC = 2


def _check(fn, r):
    if r < 0:
        raise Vp9HipError(fn, r)
    return r


def resid4_host(bpp, tcode, txtp, eobs, coefs):
    """The 4x4 residual kernels' lane routine run on the host (vp9hip_resid4_host): coefs is
    (n, 16) scan-order coefficients (int16 at 8 bits, int32 above), eobs (n,) in 1..16; returns
    the (n, 16) int32 residuals, column-major (x * 4 + y), before the int16 saturation."""
    hb = int(bpp > 8)
    coefs = np.ascontiguousarray(coefs, np.int32 if hb else np.int16)
    eobs = np.ascontiguousarray(eobs, np.uint8)
    n = len(eobs)
    assert coefs.shape == (n, 16)
    res = np.empty((n, 16), np.int32)
    _check("vp9hip_resid4_host", lib().vp9hip_resid4_host(hb, tcode, txtp, n, eobs.ctypes.data, coefs.ctypes.data,
                                                          res.ctypes.data))
    return res


def residn_host(bpp, tcode, txtp, eobs, coefs):
    """The lane-per-column residual kernels' block routine run on the host (vp9hip_residn_host):
    tcode 1..3 = 8x8, 16x16, 32x32 (N = 4 << tcode); coefs is (n, N * N) scan-order
    coefficients (int16 at 8 bits, int32 above), eobs (n,) in 1..N * N; returns the (n, N * N)
    int32 residuals, column-major (x * N + y), before the int16 saturation."""
    hb = int(bpp > 8)
    coefs = np.ascontiguousarray(coefs, np.int32 if hb else np.int16)
    eobs = np.ascontiguousarray(eobs, np.uint16)
    n = len(eobs)
    nn = (4 << tcode) ** 2 if 1 <= tcode <= 3 else coefs.shape[1]
    assert coefs.shape == (n, nn)
    res = np.empty((n, nn), np.int32)
    _check("vp9hip_residn_host", lib().vp9hip_residn_host(hb, tcode, txtp, n, eobs.ctypes.data, coefs.ctypes.data,
                                                          res.ctypes.data))
    return res


def plan_sched_host(ss_h, ss_v, ja):
    """The device planner's intra schedule of one SB in scalar host code
    (vp9hip_plan_sched_host): ja = the SB's job words in decode order (plane | tx size << 2 |
    mode slot << 8 | x4 << 12 | y4 << 16 | trx << 30). Returns (order, passes, masks): the decode
    index of the job at each position of the SB's job array, the pass words, and per job the units
    it waits for (bit u of its top row, bit 16 + v of its left column)."""
    ja = np.ascontiguousarray(ja, np.uint32)
    n = len(ja)
    order, passes, masks = np.empty(n, np.uint16), np.empty(max(n, 1), np.uint32), np.empty(n, np.uint32)
    npass = _check("vp9hip_plan_sched_host", lib().vp9hip_plan_sched_host(ss_h, ss_v, n, ja.ctypes.data, order.ctypes.data,
                                                                         passes.ctypes.data, masks.ctypes.data))
    return order, passes[:npass].copy(), masks


def plan_heights_host(ss_h, ss_v, ja):
    """The heights (longest path to a sink, unclamped) the device planner's relaxation gives the
    jobs of one SB, from the kernel's routine run on the host (vp9hip_plan_heights_host); ja as
    for plan_sched_host."""
    ja = np.ascontiguousarray(ja, np.uint32)
    heights = np.empty(len(ja), np.uint32)
    _check("vp9hip_plan_heights_host", lib().vp9hip_plan_heights_host(ss_h, ss_v, len(ja), ja.ctypes.data, heights.ctypes.data))
    return heights


def plan_emit_host(ss_h, ss_v, ja):
    """The same schedule from the device planner's own pass loop and emit run on the host
    (vp9hip_plan_emit_host: the kernel's routines, a loop over 64 slots in place of the lanes); ja
    as for plan_sched_host. Returns (order, passes, njobs) in plan_sched_host's layout."""
    ja = np.ascontiguousarray(ja, np.uint32)
    n = len(ja)
    order, passes, njobs = np.full(n, 0xffff, np.uint16), np.empty(max(n, 1), np.uint32), ctypes.c_int(0)
    npass = _check("vp9hip_plan_emit_host", lib().vp9hip_plan_emit_host(ss_h, ss_v, n, ja.ctypes.data, order.ctypes.data,
                                                                       passes.ctypes.data, ctypes.addressof(njobs)))
    return order, passes[:npass].copy(), njobs.value


def intra_txfm_type(mode):
    """txtp (bit 0: ADST in the first pass, bit 1: in the second) the planners give a luma
    intra block of `mode` below 32x32 (vp9hip_intra_txfm_type)."""
    return _check("vp9hip_intra_txfm_type", lib().vp9hip_intra_txfm_type(int(mode)))


IntraJob = collections.namedtuple("IntraJob", "slot have_top have_left ct cl trreal nd trx")


def intra_job_host(p, txs, mode, bx, by, x, y, pw4, tile_x0, cols, rows, ss_h, ss_v, ux0, uy0):
    """The host planner's check_intra_mode of one tx block (vp9hip_intra_job_host =
    pl_intra_job_blk) from what it holds: plane, tx size code, coded mode, the block's plane
    pixel position, the tx block's (x, y) and the block's width in 4x4 units, the tile's first
    8x8 column, the frame's 8x8 columns and rows, the subsampling and the tx block's 4x4 unit
    in its SB. Returns IntraJob(slot of the final mode, have_top, have_left, ct, cl, trreal, nd,
    trx)."""
    out = (ctypes.c_int32 * 8)()
    _check("vp9hip_intra_job_host", lib().vp9hip_intra_job_host(p, txs, mode, bx, by, x, y, pw4, tile_x0, cols, rows,
                                                                ss_h, ss_v, ux0, uy0, out))
    return IntraJob(*out)


def intra_job_dev(p, txs, mode, sbx, sby, ux0, uy0, right, tile_sb0, cols, rows, ss_h, ss_v):
    """The same from what the device planner's k_pjplan holds (vp9hip_intra_job_dev =
    pl_intra_job_sb): the SB, the tx block's 4x4 unit in it, whether a tx block lies to its
    right in the block, the tile's first SB column."""
    out = (ctypes.c_int32 * 8)()
    _check("vp9hip_intra_job_dev", lib().vp9hip_intra_job_dev(p, txs, mode, sbx, sby, ux0, uy0, int(right), tile_sb0, cols,
                                                              rows, ss_h, ss_v, out))
    return IntraJob(*out)


def synth_params(width, height, bpp=8, **kw):
    """§8(d) default stream settings, overridable by keyword."""
    p = SynthParams()
    lib().vp9hip_synth_defaults(ctypes.byref(p), width, height, bpp)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k == "seg" and isinstance(v, dict):
            v = seg_params(**v)
        setattr(p, k, v)
    return p


class SynthFrame:
    """A pass-1 frame packet generated by vp9hip_synth_frame (owns its C arrays)."""

    def __init__(self, params):
        self.params = params
        self.pkt = FramePacket()
        _check("vp9hip_synth_frame", lib().vp9hip_synth_frame(ctypes.byref(self.pkt), ctypes.byref(params)))

    def __del__(self):
        if getattr(self, "pkt", None) is not None and _lib_handle is not None:
            _lib_handle.vp9hip_synth_free(ctypes.byref(self.pkt))
            self.pkt = None

    @property
    def nbytes_coefs(self):
        return self.pkt.ncoefs * (2 if self.pkt.bpp == 8 else 4)

    def blocks(self):
        return [self.pkt.blocks[i] for i in range(self.pkt.nblocks)]


def encode_frame(frame, base_q_idx):
    """Write a pass-1 packet (SynthFrame or FramePacket) as a VP9 frame bitstream
    (vp9h_encode_frame): returns bytes."""
    pkt = frame.pkt if hasattr(frame, "pkt") else frame
    buf, n = ctypes.c_void_p(), ctypes.c_size_t()
    _check("vp9h_encode_frame", lib().vp9h_encode_frame(ctypes.byref(pkt), base_q_idx, ctypes.byref(buf), ctypes.byref(n)))
    try:
        return ctypes.string_at(buf.value, n.value)
    finally:
        lib().vp9h_buffer_free(buf)


class DecodedFrame:
    """The pass-1 packet of one VP9 frame bitstream, parsed on the host by
    vp9h_decode_frame (owns its C arrays); usable wherever a SynthFrame is."""

    def __init__(self, data):
        self._data = bytes(data)
        self.pkt = FramePacket()
        _check("vp9h_decode_frame", lib().vp9h_decode_frame(self._data, len(self._data), ctypes.byref(self.pkt)))

    def __del__(self):
        if getattr(self, "pkt", None) is not None and _lib_handle is not None:
            _lib_handle.vp9h_frame_free(ctypes.byref(self.pkt))
            self.pkt = None


class _OwnedPacket:
    """A pass-1 packet whose arrays the library allocated (vp9h_frame_free)."""

    def __init__(self):
        self.pkt = FramePacket()

    def __del__(self):
        if getattr(self, "pkt", None) is not None and _lib_handle is not None:
            _lib_handle.vp9h_frame_free(ctypes.byref(self.pkt))
            self.pkt = None

    def blocks(self):
        return [self.pkt.blocks[i] for i in range(self.pkt.nblocks)]


def enc_params(**kw):
    """vp9h_enc_defaults, overridable by keyword (ref_slot / sign_bias take 3-sequences)."""
    p = EncParams()
    lib().vp9h_enc_defaults(ctypes.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if k in ("ref_slot", "sign_bias"):
            v = (ctypes.c_int32 * 3)(*v)
        if k == "seg" and isinstance(v, dict):
            v = seg_params(**v)
        setattr(p, k, v)
    return p


class Stream:
    """A stream's host parse state (vp9h_stream): decode or encode frames in order."""

    def __init__(self, threads=1):
        self._s = ctypes.c_void_p()
        _check("vp9h_stream_open", lib().vp9h_stream_open(ctypes.byref(self._s)))
        if threads != 1:
            self.set_threads(threads)

    def set_color(self, colorspace, full_range):
        """Encoding: the colour space code (0..5, 7 = RGB) and range bit the following intra
        frames code (vp9h_stream_set_color; the default is 2 = BT.709, limited)."""
        _check("vp9h_stream_set_color", lib().vp9h_stream_set_color(self._s, int(colorspace), int(bool(full_range))))

    def set_threads(self, n):
        """Tile-column threads of decode (vp9h_stream_set_threads)."""
        _check("vp9h_stream_set_threads", lib().vp9h_stream_set_threads(self._s, int(n)))

    def close(self):
        if self._s:
            lib().vp9h_stream_close(self._s)
            self._s = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode(self, data):
        """One frame of compressed data -> (packet or None for show_existing_frame, FrameInfo)."""
        data = bytes(data)
        out, info = _OwnedPacket(), FrameInfo()
        _check("vp9h_stream_decode", lib().vp9h_stream_decode(self._s, data, len(data), ctypes.byref(out.pkt),
                                                               ctypes.byref(info)))
        return (None if info.show_existing_frame else out), info

    def encode(self, frame, params=None, **kw):
        """Write one frame (a packet, or None with show_existing_frame=1): returns
        (bytes, coded packet or None)."""
        p = params if params is not None else enc_params(**kw)
        pkt = None if frame is None else (frame.pkt if hasattr(frame, "pkt") else frame)
        buf, n = ctypes.c_void_p(), ctypes.c_size_t()
        coded = _OwnedPacket()
        _check("vp9h_stream_encode", lib().vp9h_stream_encode(self._s, ctypes.byref(pkt) if pkt is not None else None,
                                                               ctypes.byref(p), ctypes.byref(buf), ctypes.byref(n),
                                                               ctypes.byref(coded.pkt)))
        try:
            data = ctypes.string_at(buf.value, n.value)
        finally:
            lib().vp9h_buffer_free(buf)
        return data, (coded if pkt is not None else None)


def superframe_split(data):
    """The frames of a superframe (vp9h_superframe_split), as bytes objects."""
    data = bytes(data)
    offs, sizes = (ctypes.c_size_t * 8)(), (ctypes.c_size_t * 8)()
    n = _check("vp9h_superframe_split", lib().vp9h_superframe_split(data, len(data), offs, sizes, 8))
    return [data[offs[i]:offs[i] + sizes[i]] for i in range(n)]


def superframe_join(frames):
    """Pack frames into one superframe with the index vp9_superframe_split reads."""
    if len(frames) == 1:
        return bytes(frames[0])
    mx = max(len(f) for f in frames)
    ln = 1 if mx < 1 << 8 else 2 if mx < 1 << 16 else 3 if mx < 1 << 24 else 4
    marker = 0xc0 | (ln - 1) << 3 | (len(frames) - 1)
    idx = bytes([marker]) + b"".join(len(f).to_bytes(ln, "little") for f in frames) + bytes([marker])
    return b"".join(bytes(f) for f in frames) + idx


def out_coefs(colorspace, full_range, bpp, out_bits):
    """((CY, CRV, CGU, CGV, CBU), shift) of the integer colour matrix (vp9hip_out_coefs)."""
    c, sh = (ctypes.c_int32 * 5)(), ctypes.c_int32()
    _check("vp9hip_out_coefs", lib().vp9hip_out_coefs(int(colorspace), int(bool(full_range)), int(bpp), int(out_bits),
                                                       c, ctypes.byref(sh)))
    return tuple(c), sh.value


def out_layout(fmt, width, height, bpp=8, ss_h=1, ss_v=1, pitch=0, frame_stride=0):
    """(bytes per frame, pitch, plane offsets) of one converted frame (vp9hip_out_layout);
    fmt is a key of OUT_FORMATS."""
    d = OutDesc(OUT_FORMATS[fmt], 2, 0, int(width), int(height), int(pitch), int(frame_stride))
    p, off = ctypes.c_int64(), (ctypes.c_int64 * 3)()
    n = _check("vp9hip_out_layout", lib().vp9hip_out_layout(ctypes.byref(d), int(bpp), int(ss_h), int(ss_v),
                                                             ctypes.byref(p), off))
    return n, p.value, tuple(off)


def resample_weights(filter, n_src, n_out, o):
    """(first source index, weights, their sum D) of output index o of an axis of n_src samples
    resampled to n_out with `filter` ("box" / "triangle" or a VP9HIP_FILTER_* code): the
    library's statement of the filters' definition (vp9hip_resample_weights, host only)."""
    f = FILTERS.get(filter, filter)
    n = _check("vp9hip_resample_weights", lib().vp9hip_resample_weights(int(f), int(n_src), int(n_out), int(o), None, None, 0, None))
    first, d, w = ctypes.c_int(), ctypes.c_int64(), (ctypes.c_int32 * n)()
    _check("vp9hip_resample_weights", lib().vp9hip_resample_weights(int(f), int(n_src), int(n_out), int(o), ctypes.byref(first),
                                                                    w, n, ctypes.byref(d)))
    return first.value, list(w), d.value


def bicubic_weights(n_src, n_out, o):
    """(first source index, weights q, their sum D, the sum S of their magnitudes) of output
    index o of an axis of n_src samples resampled to n_out with the bicubic filter: the library's
    statement of its definition (vp9hip_bicubic_weights, host only)."""
    fn = lib().vp9hip_bicubic_weights
    n = _check("vp9hip_bicubic_weights", fn(int(n_src), int(n_out), int(o), None, None, 0, None, None))
    first, d, a, w = ctypes.c_int(), ctypes.c_int64(), ctypes.c_int64(), (ctypes.c_int32 * n)()
    _check("vp9hip_bicubic_weights", fn(int(n_src), int(n_out), int(o), ctypes.byref(first), w, n, ctypes.byref(d), ctypes.byref(a)))
    return first.value, list(w), d.value, a.value


GRADE_OUT_LUT = 4097           # VP9HIP_GRADE_OUT_LUT


def _grade_table(name, values, n, top):
    a = np.asarray(values)
    if a.shape != (n,) or not np.issubdtype(a.dtype, np.integer) or (a.size and (a.min() < 0 or a.max() > top)):
        raise ValueError("Grade: %s takes %d integers in 0..%d" % (name, n, top))
    return np.ascontiguousarray(a, np.uint16)


class Grade:
    """A graded output's three tables (include/vp9hip.h "Graded output"): in_lut, 2^bpp u16; m,
    3 x 3 int32 with 14 fractional bits, |m| <= 2^16; out_lut, 4097 u16 of at most out_max (255 for
    "rgb24" / "rgbp_u8", 65535 for "rgbp_f16": `fmt` is the format name or out_max itself). On
    its own it is host data (grade_host takes it); Device.grade / Decoder.grade return the one
    that convert(grade=...) takes, with the tables in device memory (vp9hip_grade_create) until
    close() or collection."""

    def __init__(self, bpp, fmt, in_lut, m, out_lut):
        self.bpp = int(bpp)
        self.out_max = int(fmt) if not isinstance(fmt, str) else 65535 if fmt == "rgbp_f16" else 255
        if self.bpp not in (8, 10, 12) or self.out_max not in (255, 65535) or fmt == "semiplanar":
            raise ValueError("Grade: bpp is 8, 10 or 12 and fmt one of the RGB formats")
        self.in_lut = _grade_table("in_lut", in_lut, 1 << self.bpp, 65535)
        self.out_lut = _grade_table("out_lut", out_lut, GRADE_OUT_LUT, self.out_max)
        m = np.asarray(m)
        if m.size != 9 or not np.issubdtype(m.dtype, np.integer) or np.abs(m).max() > 1 << 16:
            raise ValueError("Grade: m takes 3 x 3 integers of magnitude at most 2^16")
        self.m = np.ascontiguousarray(m.reshape(3, 3), np.int32)
        self._g = None
        self._ctx = None

    def desc(self):
        """The vp9hip_grade_desc of the tables (they stay this object's)."""
        return GradeDesc(self.bpp, self.out_max, self.in_lut.ctypes.data, self.m.ctypes.data, self.out_lut.ctypes.data)

    def _on(self, ctx):
        g = Grade(self.bpp, self.out_max, self.in_lut, self.m, self.out_lut)
        h = ctypes.c_void_p()
        d = g.desc()
        _check("vp9hip_grade_create", lib().vp9hip_grade_create(ctx, ctypes.byref(d), ctypes.byref(h)))
        g._g, g._ctx = h, ctx
        return g

    def close(self):
        if self._g is not None:
            lib().vp9hip_grade_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _grade_handle(grade, fmt):
    """convert(grade=...)'s checks of its own: an RGB format, a grade with device tables."""
    if fmt == "semiplanar":
        raise ValueError("convert: a grade is defined for the RGB formats, not semiplanar")
    if not isinstance(grade, Grade) or grade._g is None:
        raise ValueError("convert: grade takes what Device.grade / Decoder.grade return")
    return grade._g


def grade_host(g, codes):
    """The three stages of Grade g on the host (vp9hip_grade_host, the C statement of the
    definition): codes is an integer array (..., 3) of R, G, B codes below 2^bpp; returns the
    uint16 array of the same shape."""
    codes = np.asarray(codes)
    if codes.ndim < 1 or codes.shape[-1] != 3 or (codes.size and (codes.min() < 0 or codes.max() >= 1 << g.bpp)):
        raise ValueError("grade_host: codes is (..., 3) with values below 2^bpp")
    c = np.ascontiguousarray(codes, np.uint16)
    v = np.empty(c.shape, np.uint16)
    d = g.desc()
    _check("vp9hip_grade_host", lib().vp9hip_grade_host(ctypes.byref(d), c.ctypes.data, c.size // 3, v.ctypes.data))
    return v


# CIE xy of R, G, B; the white point of all of them is D65
_PRIMARIES = {"bt709": ((.64, .33), (.30, .60), (.15, .06)),
              "bt601": ((.64, .33), (.29, .60), (.15, .06)),              # 625 lines (BT.470BG)
              "bt601_525": ((.63, .34), (.31, .595), (.155, .07)),        # 525 lines (SMPTE 170M)
              "bt2020": ((.708, .292), (.170, .797), (.131, .046))}
_SDR_TRANSFERS = ("bt709", "srgb", "linear")


def _rgb_to_xyz(name):
    xy = np.array(_PRIMARIES[name], np.float64)
    P = np.stack([xy[:, 0] / xy[:, 1], np.ones(3), (1 - xy[:, 0] - xy[:, 1]) / xy[:, 1]])
    white = np.array([.3127 / .3290, 1., (1 - .3127 - .3290) / .3290])
    return P * np.linalg.solve(P, white)


def _eotf_nits(transfer, e, peak_nits, white_nits):
    """Display light in cd/m^2 of the signal e in [0, 1]."""
    e = np.asarray(e, np.float64)
    if transfer == "pq":                                   # SMPTE ST 2084
        m1, m2, c1, c2, c3 = 2610 / 16384, 2523 / 4096 * 128, 3424 / 4096, 2413 / 4096 * 32, 2392 / 4096 * 32
        p = e ** (1 / m2)
        return 10000. * (np.maximum(p - c1, 0) / (c2 - c3 * p)) ** (1 / m1)
    if transfer == "hlg":                                  # BT.2100: inverse OETF, then gamma 1.2 per channel
        a = .17883277
        b, c = 1 - 4 * a, .5 - a * np.log(4 * a)
        s = np.where(e <= .5, e * e / 3, (np.exp((np.minimum(e, 1.) - c) / a) + b) / 12)
        return peak_nits * s ** 1.2
    if transfer == "bt709":
        return white_nits * np.where(e < .081, e / 4.5, ((e + .099) / 1.099) ** (1 / .45))
    if transfer == "srgb":
        return white_nits * np.where(e <= .04045, e / 12.92, ((e + .055) / 1.055) ** 2.4)
    if transfer == "linear":
        return white_nits * e
    raise ValueError("make_grade: transfer_in is 'pq', 'hlg', 'bt709', 'srgb' or 'linear'")


def _oetf(transfer, x):
    x = np.clip(np.asarray(x, np.float64), 0, 1)
    if transfer == "srgb":
        return np.where(x <= .0031308, 12.92 * x, 1.055 * x ** (1 / 2.4) - .055)
    if transfer == "bt709":
        return np.where(x < .018, 4.5 * x, 1.099 * x ** .45 - .099)
    if transfer == "linear":
        return x
    raise ValueError("make_grade: transfer_out is 'srgb', 'bt709' or 'linear' (display-referred SDR)")


def make_grade(bpp, fmt, transfer_in, primaries_in, transfer_out="srgb", primaries_out="bt709", peak_nits=1000,
               white_nits=203, tonemap="reinhard"):
    """The integer tables of a colour pipeline, computed once in float64 on the host: a Grade
    (host data; Device.grade(g) uploads it).
      in_lut[c]  = the input EOTF of c / (2^bpp - 1) in cd/m^2, / peak_nits, clipped to 1, as the
                   nearest u16. transfer_in: "pq" (ST 2084), "hlg", "bt709", "srgb", "linear".
                   "hlg" is the inverse OETF and then the system gamma 1.2 on each channel: an
                   approximation of BT.2100's OOTF, which applies the gamma to the luminance.
                   The SDR transfers take peak_nits = white_nits.
      m          = primaries_in -> primaries_out through XYZ with D65 ("bt709", "bt601" (625
                   lines), "bt601_525", "bt2020"), round(x 2^14).
      out_lut[i] = x = (i / 4096) peak_nits / white_nits, tone-mapped ("clip": min(x, 1);
                   "reinhard": x (1 + x / w^2) / (1 + x), w = peak_nits / white_nits, which maps
                   w to 1), through the output OETF (transfer_out: "srgb", "bt709", "linear"),
                   times out_max, as the nearest integer.
    Both curves are per channel. Operators that need the three channels at once (BT.2390 in
    ICtCp, max-RGB hue-preserving maps) cannot be a grade and are out of scope."""
    bpp = int(bpp)
    if bpp not in (8, 10, 12):
        raise ValueError("make_grade: bpp is 8, 10 or 12")
    if tonemap not in ("clip", "reinhard"):
        raise ValueError("make_grade: tonemap is 'clip' or 'reinhard'")
    if primaries_in not in _PRIMARIES or primaries_out not in _PRIMARIES:
        raise ValueError("make_grade: primaries are " + ", ".join(repr(k) for k in _PRIMARIES))
    peak, white = float(peak_nits), float(white_nits)
    if transfer_in in _SDR_TRANSFERS:
        peak = white
    if not (white > 0 and peak >= white):
        raise ValueError("make_grade: 0 < white_nits <= peak_nits")
    out_max = 65535 if fmt == "rgbp_f16" else 255
    code = np.arange(1 << bpp, dtype=np.float64) / ((1 << bpp) - 1)
    in_lut = np.rint(np.clip(_eotf_nits(transfer_in, code, peak, white) / peak, 0, 1) * 65535).astype(np.int64)
    if primaries_in == primaries_out:
        m = np.eye(3)
    else:
        m = np.linalg.solve(_rgb_to_xyz(primaries_out), _rgb_to_xyz(primaries_in))
    m = np.rint(m * (1 << 14)).astype(np.int64)
    x = np.arange(GRADE_OUT_LUT, dtype=np.float64) / 4096 * (peak / white)
    w = peak / white
    x = np.minimum(x, 1) if tonemap == "clip" else x * (1 + x / (w * w)) / (1 + x)
    out_lut = np.rint(_oetf(transfer_out, x) * out_max).astype(np.int64)
    return Grade(bpp, fmt, in_lut, m, out_lut)


# Matroska's TransferCharacteristics / Primaries codes -> make_grade's names
_WEBM_TRANSFERS = {16: "pq", 18: "hlg", 1: "bt709", 13: "srgb"}
_WEBM_PRIMARIES = {9: "bt2020", 1: "bt709", 5: "bt601", 6: "bt601_525"}


def grade_for(colour, bpp, fmt, **kw):
    """make_grade for a stream's colour description (webm_colour's dict): transfer codes 16 (PQ),
    18 (HLG), 1 (BT.709), 13 (sRGB) and primaries 9 (BT.2020), 1 (BT.709), 5 / 6 (BT.601 625 /
    525); any other code, "unspecified" included, is a ValueError (pass the names to make_grade
    yourself). A mastering LuminanceMax becomes peak_nits unless given; kw goes to make_grade."""
    t, p = colour.get("transfer", 2), colour.get("primaries", 2)
    if t not in _WEBM_TRANSFERS or p not in _WEBM_PRIMARIES:
        raise ValueError("grade_for: no grade for transfer %r, primaries %r" % (t, p))
    if "peak_nits" not in kw and colour.get("luminance_max", 0) > 0:
        kw["peak_nits"] = colour["luminance_max"]
    return make_grade(bpp, fmt, _WEBM_TRANSFERS[t], _WEBM_PRIMARIES[p], **kw)


def letterbox_rect(w, h, OW, OH, align=(1, 1)):
    """The destination rectangle (dx, dy, dw, dh) that places a w x h picture inside OW x OH
    at its aspect ratio, centred. In integers: if w OH >= h OW the picture takes the full
    width, dw = OW and dh = max(1, (h OW + w // 2) // w) (the height rounded to nearest);
    otherwise the full height, dh = OH and dw = max(1, (w OH + h // 2) // h). Then
    dx = (OW - dw) // 2 and dy = (OH - dh) // 2, each rounded down to a multiple of align[0] /
    align[1] (the subsampling, (2, 2) for a 4:2:0 semi-planar output)."""
    w, h, OW, OH = int(w), int(h), int(OW), int(OH)
    if min(w, h, OW, OH) < 1 or min(align) < 1:
        raise ValueError("letterbox_rect: sizes and alignment must be positive")
    if w * OH >= h * OW:
        dw, dh = OW, max(1, (h * OW + w // 2) // w)       # <= OH: h OW <= w OH
    else:
        dw, dh = max(1, (w * OH + h // 2) // h), OH       # <= OW likewise
    dx, dy = (OW - dw) // 2, (OH - dh) // 2
    return dx // align[0] * align[0], dy // align[1] * align[1], dw, dh


def _rect_array(name, rects, n):
    """n vp9hip_rects of a rectangle argument: one 4-tuple for every frame, or n of them."""
    rects = list(rects)
    if len(rects) == 4 and not hasattr(rects[0], "__len__"):
        rects = [rects] * n
    if len(rects) != n or any(len(r) != 4 for r in rects):
        raise ValueError("convert: %s takes one (x, y, w, h) or one per frame (%d)" % (name, n))
    return (Rect * n)(*[Rect(*(int(v) for v in r)) for r in rects])


def _resample_arg(n, resize, filter, src_rects, dst_rects, fill, bpp, colorspace, full_range):
    """The vp9hip_resample of convert()'s filter / src_rects / dst_rects / fill arguments, or
    None when none of them is given; they need resize. The arrays it points to are kept alive
    as attributes of the struct."""
    if filter == "box" and src_rects is None and dst_rects is None and fill is None:
        return None
    if resize is None:
        raise ValueError("convert: filter, src_rects, dst_rects and fill need resize=(OW, OH)")
    if filter not in FILTERS and filter != "bicubic":
        raise ValueError("convert: filter is 'box', 'triangle' or 'bicubic'")
    ow, oh = (int(x) for x in resize)
    rs = Resample(FILTER_BICUBIC if filter == "bicubic" else FILTERS[filter], ow, oh)
    if src_rects is not None:
        rs._src = _rect_array("src_rects", src_rects, n)
        rs.src_rects = ctypes.cast(rs._src, ctypes.POINTER(Rect))
    if dst_rects is not None:
        rs._dst = _rect_array("dst_rects", dst_rects, n)
        rs.dst_rects = ctypes.cast(rs._dst, ctypes.POINTER(Rect))
    if fill is None:      # black, by the range in effect
        fill = (0, 0, 0) if colorspace == 7 else (0 if full_range else 16 << (bpp - 8), 1 << (bpp - 1), 1 << (bpp - 1))
    rs.fill[:] = [int(v) for v in fill]
    return rs


EXPORT_MOTION = 1              # VP9HIP_EXPORT_MOTION


def motion_host(frame):
    """The motion field of one packet (SynthFrame, a parsed packet or a FramePacket) on the host,
    vp9hip_motion_host, the C statement of the definition in include/vp9hip.h: (mv, info), int16
    (GH, GW, 2, 2) and uint8 (GH, GW, 4) with GW x GH = 2 ((width + 7) >> 3) x 2 ((height + 7) >> 3)
    cells of 4x4 luma pixels. Cells no block covers are zero."""
    pkt = frame.pkt if hasattr(frame, "pkt") else frame
    gw, gh = 2 * ((pkt.width + 7) >> 3), 2 * ((pkt.height + 7) >> 3)
    if gw <= 0 or gh <= 0:
        raise Vp9HipError("vp9hip_motion_host", EINVAL)
    mv, info = np.zeros((gh, gw, 2, 2), np.int16), np.zeros((gh, gw, 4), np.uint8)
    _check("vp9hip_motion_host", lib().vp9hip_motion_host(ctypes.byref(pkt), mv.ctypes.data, info.ctypes.data))
    return mv, info


def _motion_views(mv, info, gw, gh, pitch, device):
    """Zero-copy torch views of a field's two device planes, strided over the fixed pitch."""
    if not _torch_first:
        raise Vp9HipUnavailable("motion: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
    import torch

    class _Mv:
        __cuda_array_interface__ = {"shape": (gh, gw, 2, 2), "typestr": "<i2", "data": (mv, False),
                                    "strides": (pitch * 8, 8, 4, 2), "version": 2}

    class _Info:
        __cuda_array_interface__ = {"shape": (gh, gw, 4), "typestr": "|u1", "data": (info, False),
                                    "strides": (pitch * 4, 4, 1), "version": 2}
    return torch.as_tensor(_Mv(), device=device or "cuda"), torch.as_tensor(_Info(), device=device or "cuda")


EXPORT_MOTION_ACC = 4          # VP9HIP_EXPORT_MOTION_ACC
ACC_END_INTRA, ACC_END_NOFIELD, ACC_END_SCALED = 0, 1, 2   # VP9HIP_ACC_END_*
# vp9hip_acc_cell
ACC_CELL = np.dtype([("dx", "<i4"), ("dy", "<i4"), ("root", "<u4"), ("hops", "<u2"), ("end", "u1"), ("pad", "u1")])


def motion_acc_host(mv, info, serial, parents=(None, None, None), parent_end=(ACC_END_NOFIELD,) * 3):
    """One frame of the accumulated-motion recurrence on the host (vp9hip_motion_acc_host, the C
    statement of the definition in include/vp9hip.h): mv int16 (GH, GW, 2, 2) and info uint8
    (GH, GW, 4) as motion_host gives them, the frame's serial, per reference name the parent's
    ACC_CELL array (GH, GW) or None with parent_end[k] (ACC_END_NOFIELD / ACC_END_SCALED) saying
    why. Returns the frame's ACC_CELL array (GH, GW)."""
    mv, info = np.ascontiguousarray(mv, np.int16), np.ascontiguousarray(info, np.uint8)
    gh, gw = info.shape[:2]
    if mv.shape != (gh, gw, 2, 2) or info.shape != (gh, gw, 4):
        raise Vp9HipError("vp9hip_motion_acc_host", EINVAL)
    par = [None if q is None else np.ascontiguousarray(q, ACC_CELL) for q in parents]
    if any(q is not None and q.shape != (gh, gw) for q in par):
        raise Vp9HipError("vp9hip_motion_acc_host", EINVAL)
    ptrs = (ctypes.c_void_p * 3)(*[None if q is None else q.ctypes.data for q in par])
    ends = (ctypes.c_int * 3)(*[int(e) for e in parent_end])
    out = np.empty((gh, gw), ACC_CELL)
    _check("vp9hip_motion_acc_host", lib().vp9hip_motion_acc_host(mv.ctypes.data, info.ctypes.data, gw, gh, serial,
                                                                  ctypes.byref(ptrs), ctypes.byref(ends), out.ctypes.data))
    return out


def acc_fields(t):
    """The five fields (dx, dy, root, hops, end) of an accumulated-motion view (Device.motion_acc:
    int32 (GH, GW, 4) with columns dx, dy, root, hops | end << 16), torch or numpy. root is the
    serial's 32 bits in an int32."""
    w = t[..., 3]
    return t[..., 0], t[..., 1], t[..., 2], w & 0xffff, (w >> 16) & 0xff


def _acc_view(acc, gw, gh, pitch, device):
    """Zero-copy torch int32 view (GH, GW, 4) of a field's device plane, strided over the pitch."""
    if not _torch_first:
        raise Vp9HipUnavailable("motion_acc: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
    import torch

    class _Acc:
        __cuda_array_interface__ = {"shape": (gh, gw, 4), "typestr": "<i4", "data": (acc, False),
                                    "strides": (pitch * 16, 16, 4), "version": 2}
    return torch.as_tensor(_Acc(), device=device or "cuda")


EXPORT_RESIDUAL = 2            # VP9HIP_EXPORT_RESIDUAL


def residual_shapes(width, height, ss_h=1, ss_v=1):
    """(rows, columns) of the three planes of a residual field's coded area (include/vp9hip.h):
    Y of 8 rows8 x 8 cols8, U and V of that shifted by the subsampling."""
    cw, ch = 8 * ((width + 7) >> 3), 8 * ((height + 7) >> 3)
    return [(ch, cw), (ch >> ss_v, cw >> ss_h), (ch >> ss_v, cw >> ss_h)]


def _plane_ptrs(planes):
    return ((ctypes.c_void_p * 3)(*[a.ctypes.data for a in planes]),
            (ctypes.c_ssize_t * 3)(*[a.strides[0] for a in planes]))


def residual_host(frame):
    """The residual field of one packet (SynthFrame, a parsed packet or a FramePacket) on the host,
    vp9hip_residual_host, the C++ statement of the definition in include/vp9hip.h: three int16
    arrays of the coded area (residual_shapes), clip(r, -m, m) where a coded tx block lies, 0
    elsewhere."""
    pkt = frame.pkt if hasattr(frame, "pkt") else frame
    if pkt.width <= 0 or pkt.height <= 0:
        raise Vp9HipError("vp9hip_residual_host", EINVAL)
    planes = [np.full(s, 0x5a5a, np.int16) for s in residual_shapes(pkt.width, pkt.height, pkt.ss_h, pkt.ss_v)]
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in planes])
    pitch = (ctypes.c_ssize_t * 3)(*[a.shape[1] for a in planes])
    rows = (ctypes.c_int * 3)(*[a.shape[0] for a in planes])
    _check("vp9hip_residual_host", lib().vp9hip_residual_host(ctypes.byref(pkt), ctypes.byref(ptrs), ctypes.byref(pitch),
                                                              ctypes.byref(rows)))
    return planes


def _residual_views(ptrs, pitch, width, height, ss_h, ss_v, device):
    """Zero-copy torch int16 views of a field's three device planes, of the visible size, strided
    over the planes' pitch."""
    if not _torch_first:
        raise Vp9HipUnavailable("residual: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
    import torch
    out = []
    for p in range(3):
        pw = width if p == 0 else (width + ss_h) >> ss_h
        ph = height if p == 0 else (height + ss_v) >> ss_v

        class _View:
            __cuda_array_interface__ = {"shape": (ph, pw), "typestr": "<i2", "data": (ptrs[p], False),
                                        "strides": (pitch[p] * 2, 2), "version": 2}
        out.append(torch.as_tensor(_View(), device=device or "cuda"))
    return out


def _resid_desc(fn, fmt, resize, size, colorspace, full_range, pitch, frame_stride):
    """The ResidDesc of a residual_tensors call: resize=None is the field's own size."""
    ow, oh = (int(x) for x in (resize if resize is not None else size))
    return ResidDesc(RESID_FORMATS[fmt], int(colorspace), int(bool(full_range)), ow, oh, int(pitch), int(frame_stride))


def residual_scaled_host(planes, width, height, ss_h, ss_v, bpp, fmt, resize, colorspace=2, full_range=False):
    """The residual tensor of one frame on the host, vp9hip_residual_scaled_host, the C statement
    of the definition in include/vp9hip.h ("residual tensors at model size"): planes are three
    2-D int16 arrays (rows may be strided) holding at least the visible width x height luma and
    the chroma samples they cover; the result is a (3, OH, OW) int16 or float16 array, fmt a key
    of RESID_FORMATS, resize = (OW, OH) or None for the field's own size."""
    pl = []
    for a in planes:
        a = np.asarray(a)
        if a.ndim != 2 or a.dtype != np.int16:
            raise ValueError("residual_scaled_host: planes must be 2-D int16 arrays")
        if a.strides[1] != 2 or a.strides[0] < 0 or a.strides[0] % 2:
            a = np.ascontiguousarray(a)
        pl.append(a)
    if len(pl) != 3:
        raise ValueError("residual_scaled_host: three planes a frame")
    d = _resid_desc("vp9hip_residual_scaled_host", fmt, resize, (width, height), colorspace, full_range, 0, 0)
    sane = 1 <= width <= 16384 and 1 <= height <= 16384 and ss_h in (0, 1) and ss_v in (0, 1)
    if sane:                                          # what the library refuses it does not read
        for p, a in enumerate(pl):
            pw, ph = (width, height) if p == 0 else ((width + ss_h) >> ss_h, (height + ss_v) >> ss_v)
            if a.shape[0] < ph or a.shape[1] < pw:
                raise ValueError("residual_scaled_host: plane %d is smaller than %d x %d" % (p, pw, ph))
    ok = 1 <= d.out_width <= 16384 and 1 <= d.out_height <= 16384
    out = np.full((3, d.out_height, d.out_width) if ok else (3, 1, 1), 0x5a5a, np.int16)
    ptrs = (ctypes.c_void_p * 3)(*[a.ctypes.data for a in pl])
    pitch = (ctypes.c_ssize_t * 3)(*[a.strides[0] // 2 for a in pl])
    _check("vp9hip_residual_scaled_host",
           lib().vp9hip_residual_scaled_host(ctypes.byref(ptrs), ctypes.byref(pitch), int(width), int(height), int(ss_h),
                                             int(ss_v), int(bpp), ctypes.byref(d), out.ctypes.data))
    return out.view(np.float16) if fmt.endswith("f16") else out


def _resid_out(n, d, out):
    """The destination of a residual_tensors call: (flat storage tensor, (N, 3, OH, OW) view of
    it). The storage is allocated, or `out` itself: a contiguous int16 or float16 cuda tensor (by
    the format) of at least the layout's elements. A descriptor the library refuses gets one
    element to hand it, so the refusal is the library's."""
    import torch
    dt = torch.float16 if d.format & 1 else torch.int16
    pitch = ctypes.c_int64()
    nbytes = lib().vp9hip_resid_layout(ctypes.byref(d), ctypes.byref(pitch))
    if nbytes < 0:
        flat = out.view(-1) if out is not None else torch.empty(1, dtype=dt, device="cuda")
        return flat, None
    stride = d.frame_stride or nbytes
    total = ((max(n, 1) - 1) * stride + nbytes) // 2
    if out is None:
        out = torch.empty(total, dtype=dt, device="cuda")
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dt and out.is_contiguous()
              and out.numel() >= total):
        raise ValueError("residual_tensors: out must be a contiguous %s cuda tensor of at least %d elements" % (dt, total))
    flat = out.view(-1)
    return flat, flat.as_strided((max(n, 0), 3, d.out_height, d.out_width),
                                 (stride // 2, pitch.value * d.out_height // 2, pitch.value // 2, 1))


def _mvt_desc(fmt, source, mask, resize, size, pitch, frame_stride):
    """The MvtDesc of a motion_tensors call: resize=None is the visible size, the dense field."""
    w, h = (int(x) for x in size)
    ow, oh = (int(x) for x in (resize if resize is not None else size))
    return MvtDesc(MVT_FORMATS[fmt], MVT_SOURCES[source], 3 if mask else 2, w, h, ow, oh, int(pitch), int(frame_stride))


def motion_scaled_host(mv, info, width, height, fmt, resize, source="coded", acc=None, mask=False):
    """The motion tensor of one frame on the host, vp9hip_motion_scaled_host, the C statement of
    the definition in include/vp9hip.h ("motion tensors at model size"): source "coded" reads mv
    int16 (GH, GW, 2, 2) and info uint8 (GH, GW, 4) as Device.motion / motion_host give them,
    source "acc" reads acc, an ACC_CELL array (GH, GW) (mv and info may then be None); rows may
    be strided, and the arrays must cover the (height + 3) >> 2 x (width + 3) >> 2 cells of the
    visible width x height. The result is a (2 or 3, OH, OW) int16 or float16 array: x, y and
    with mask the coverage; fmt a key of MVT_FORMATS, resize = (OW, OH) or None for the visible
    size."""
    fn = "vp9hip_motion_scaled_host"
    d = _mvt_desc(fmt, source, mask, resize, (width, height), 0, 0)
    sane = 1 <= width <= 16384 and 1 <= height <= 16384

    def rows(a, name, dtype, tail, cell):
        """a with rows of whole cells, its pitch in cells"""
        a = np.asarray(a)
        if a.dtype != dtype or a.shape[2:] != tail or a.ndim != 2 + len(tail):
            raise ValueError("%s: %s must be a %s array (GH, GW%s)" % (fn, name, np.dtype(dtype).name, "".join(", %d" % t for t in tail)))
        if not a[:1, :1].flags.c_contiguous or (a.shape[1] > 1 and a.strides[1] != cell) or a.strides[0] < 0 or a.strides[0] % cell:
            a = np.ascontiguousarray(a)
        if sane and (a.shape[0] < (height + 3) >> 2 or a.shape[1] < (width + 3) >> 2):
            raise ValueError("%s: %s is smaller than the visible %d x %d" % (fn, name, width, height))
        return a, (a.strides[0] // cell if a.shape[0] > 1 else a.shape[1])

    ptrs, pitches = [None, None, None], []
    if d.source == 0:
        m, pm = rows(mv, "mv", np.int16, (2, 2), 8)
        i, pi = rows(info, "info", np.uint8, (4,), 4)
        if pm != pi:                                      # one pitch for both planes, as on the device
            m, i = np.ascontiguousarray(m), np.ascontiguousarray(i)
            pm = pi = m.shape[1]
            if m.shape[:2] != i.shape[:2]:
                raise ValueError("%s: mv and info of different grids" % fn)
        ptrs[0], ptrs[1], pitches, keep = m.ctypes.data, i.ctypes.data, pm, (m, i)
    else:
        if acc is None:
            raise ValueError("%s: source 'acc' needs acc" % fn)
        a, pa = rows(acc, "acc", ACC_CELL, (), 16)
        ptrs[2], pitches, keep = a.ctypes.data, pa, (a,)
    ok = 1 <= d.out_width <= 16384 and 1 <= d.out_height <= 16384
    out = np.full((d.planes, d.out_height, d.out_width) if ok else (d.planes, 1, 1), 0x5a5a, np.int16)
    _check(fn, lib().vp9hip_motion_scaled_host(ptrs[0], ptrs[1], ptrs[2], pitches, ctypes.byref(d), out.ctypes.data))
    del keep
    return out.view(np.float16) if fmt == "f16" else out


def _mvt_out(n, d, out):
    """The destination of a motion_tensors call: (flat storage tensor, (N, P, OH, OW) view of
    it), as _resid_out. A descriptor the library refuses gets one element to hand it, so the
    refusal is the library's."""
    import torch
    dt = torch.float16 if d.format & 1 else torch.int16
    pitch = ctypes.c_int64()
    nbytes = lib().vp9hip_mvt_layout(ctypes.byref(d), ctypes.byref(pitch))
    if nbytes < 0:
        flat = out.view(-1) if out is not None else torch.empty(1, dtype=dt, device="cuda")
        return flat, None
    stride = d.frame_stride or nbytes
    total = ((max(n, 1) - 1) * stride + nbytes) // 2
    if out is None:
        out = torch.empty(total, dtype=dt, device="cuda")
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dt and out.is_contiguous()
              and out.numel() >= total):
        raise ValueError("motion_tensors: out must be a contiguous %s cuda tensor of at least %d elements" % (dt, total))
    flat = out.view(-1)
    return flat, flat.as_strided((max(n, 0), d.planes, d.out_height, d.out_width),
                                 (stride // 2, pitch.value * d.out_height // 2, pitch.value // 2, 1))


METRIC_FIELDS = ("sum_a", "sum_b", "sumsq_a", "sad", "sse", "ndiff", "maxdiff", "first")   # VP9HIP_METRIC_*
METRIC_CELL = 16               # VP9HIP_METRIC_CELL


def _metric_map_shape(width, height):
    return (int(height) + METRIC_CELL - 1) // METRIC_CELL, (int(width) + METRIC_CELL - 1) // METRIC_CELL


def frame_metrics_host(planes_a, planes_b, width, height, bpp, ss_h=1, ss_v=1, cells=False):
    """The metrics of one pair of host frames, vp9hip_frame_metrics_host, the C statement of the
    definition in include/vp9hip.h: an int64 (3, 8) array, plane by METRIC_FIELDS, over the
    top-left width x height luma samples and the chroma they cover; with cells=True
    (metrics, map), map the int32 (MH, MW) luma SAD of every 16x16 cell. planes_* are three 2-D
    arrays each, uint8 at 8 bits, else uint16 (rows may be strided; the codes are not masked to
    the depth); planes_b=None gives the statistics of a alone."""
    dt = np.uint8 if bpp == 8 else np.uint16
    sane = 1 <= width <= 16384 and 1 <= height <= 16384 and ss_h in (0, 1) and ss_v in (0, 1)

    def prep(planes):
        out = []
        for p, a in enumerate(planes):
            a = np.asarray(a)
            if a.ndim != 2 or a.dtype != dt:
                raise ValueError("frame_metrics_host: planes must be 2-D %s arrays" % np.dtype(dt).name)
            if a.strides[1] != a.itemsize or a.strides[0] < 0:
                a = np.ascontiguousarray(a)
            if sane:                                  # what the library refuses it does not read
                pw, ph = (width, height) if p == 0 else ((width + ss_h) >> ss_h, (height + ss_v) >> ss_v)
                if a.shape[0] < ph or a.shape[1] < pw:
                    raise ValueError("frame_metrics_host: plane %d is smaller than %d x %d" % (p, pw, ph))
            out.append(a)
        if len(out) != 3:
            raise ValueError("frame_metrics_host: three planes a frame")
        return out
    pa = prep(planes_a)
    pb = prep(planes_b) if planes_b is not None else None
    out = np.full((3, len(METRIC_FIELDS)), -0x5a5a, np.int64)
    cmap = np.full(_metric_map_shape(width, height) if sane else (1, 1), -0x5a5a, np.int32) if cells else None
    ap, als = _plane_ptrs(pa)
    bp, bls = _plane_ptrs(pb) if pb is not None else (None, None)
    _check("vp9hip_frame_metrics_host",
           lib().vp9hip_frame_metrics_host(ctypes.byref(ap), ctypes.byref(als), ctypes.byref(bp) if pb is not None else None,
                                           ctypes.byref(bls) if pb is not None else None, int(width), int(height), int(bpp),
                                           int(ss_h), int(ss_v), out.ctypes.data, cmap.ctypes.data if cells else None))
    return (out, cmap) if cells else out


def _hist_desc(fn, what, bins, colorspace, full_range, width, height, rects, n):
    """(HistDesc, channels, bins) of histograms()' arguments; the rectangle array is kept alive
    by the desc's _keep."""
    if what not in HIST_MODES:
        raise ValueError("%s: what is %s" % (fn, " or ".join(repr(k) for k in HIST_MODES)))
    bins = int(bins)
    if bins < 1 or bins & (bins - 1):
        raise ValueError("%s: bins is a power of two" % fn)
    d = HistDesc(HIST_MODES[what], bins.bit_length() - 1, int(colorspace), int(bool(full_range)), int(width), int(height), None)
    if rects is not None:
        d._keep = _rect_array("rects", rects, n)
        d.rects = ctypes.cast(d._keep, ctypes.POINTER(Rect))
    return d, len(HIST_CHANNELS[what]), bins


def histograms_host(planes, width, height, bpp, ss_h=1, ss_v=1, what="planes", bins=256, colorspace=2, full_range=False,
                    rect=None):
    """The histograms of one host frame, vp9hip_frame_histograms_host, the C statement of the
    definition in include/vp9hip.h "frame histograms": an int32 (C, B) array, channels Y, U, V
    (what="planes") or R, G, B, max(R, G, B) at the source's depth (what="rgbm") by `bins` bins,
    a power of two in 16 .. 2^bpp; a code's bin is min(c, 2^bpp - 1) >> (bpp - log2 bins). Over
    the luma rectangle rect = (x, y, w, h) inside width x height (default: all of it) and the
    chroma it covers. planes are three 2-D arrays, uint8 at 8 bits, else uint16 (rows may be
    strided)."""
    fn = "histograms_host"
    dt = np.uint8 if bpp == 8 else np.uint16
    d, C, B = _hist_desc(fn, what, bins, colorspace, full_range, width, height, None, 1)
    sane = 1 <= width <= 16384 and 1 <= height <= 16384 and ss_h in (0, 1) and ss_v in (0, 1)
    pl = []
    for p, a in enumerate(planes):
        a = np.asarray(a)
        if a.ndim != 2 or a.dtype != dt:
            raise ValueError("%s: planes must be 2-D %s arrays" % (fn, np.dtype(dt).name))
        if a.strides[1] != a.itemsize or a.strides[0] < 0:
            a = np.ascontiguousarray(a)
        if sane:                                      # what the library refuses it does not read
            pw, ph = (width, height) if p == 0 else ((width + ss_h) >> ss_h, (height + ss_v) >> ss_v)
            if a.shape[0] < ph or a.shape[1] < pw:
                raise ValueError("%s: plane %d is smaller than %d x %d" % (fn, p, pw, ph))
        pl.append(a)
    if len(pl) != 3:
        raise ValueError("%s: three planes a frame" % fn)
    out = np.full((C, min(B, 4096)), -0x5a5a, np.int32)
    ptrs, ls = _plane_ptrs(pl)
    r = Rect(*(int(v) for v in rect)) if rect is not None else None
    _check("vp9hip_frame_histograms_host",
           lib().vp9hip_frame_histograms_host(ctypes.byref(ptrs), ctypes.byref(ls), int(bpp), int(ss_h), int(ss_v),
                                              ctypes.byref(d), ctypes.byref(r) if r is not None else None, out.ctypes.data))
    return out


def hist_percentile(h, num, den):
    """The smallest bin k with den * sum(h[..., :k + 1]) >= num * sum(h[...]), for every leading
    index of h (a tensor or array whose last axis is bins): int64, in integer arithmetic. num = 0
    gives bin 0 if h[..., 0] > 0, else the first non-zero bin (0 for an all-zero row); num = den
    gives the last non-zero bin."""
    num, den = int(num), int(den)
    if den < 1 or not 0 <= num <= den:
        raise ValueError("hist_percentile: 0 <= num <= den, den >= 1")
    if hasattr(h, "cumsum") and not isinstance(h, np.ndarray):       # a torch tensor: stays on its device
        import torch
        c = h.to(torch.int64).cumsum(-1)
        ok = (den * c >= num * c[..., -1:]) & (c > 0)
        first = ok.to(torch.int64).argmax(-1)
        return torch.where(ok.any(-1), first, torch.zeros_like(first))
    c = np.cumsum(np.asarray(h).astype(np.int64), axis=-1)
    ok = (den * c >= num * c[..., -1:]) & (c > 0)
    return np.where(ok.any(-1), ok.argmax(-1), 0).astype(np.int64)


def light_levels(h_m, bpp, transfer, peak_nits=10000, white_nits=203, percentiles=((999, 1000),)):
    """One frame's contribution to MaxCLL / MaxFALL from its max(R, G, B) histogram: h_m is the M
    channel of histograms(what="rgbm", bins=1 << bpp) as host data, (B,) or (N, B), one bin per
    code (fewer bins are a ValueError). A dict of float64 values, scalars or (N,):
      "max_nits"  the display light (_eotf_nits of code / (2^bpp - 1): transfer "pq", "hlg",
                  "bt709", "srgb", "linear"; peak_nits scales HLG, white_nits the SDR transfers)
                  of the highest non-zero code,
      "avg_nits"  sum h[c] nits(c) / sum h,
      "p<num>/<den>" for each (num, den) of percentiles: nits of hist_percentile(h_m, num, den).
    An empty histogram gives 0 for all three. The intended use, a tone map keyed to the content
    and not to the mastering display:
        levels = light_levels(dev.histograms(bufs, "rgbm", bins=1 << bpp)[0, 3].cpu().numpy(), bpp, "pq")
        g = grade_for(colour, bpp, fmt, peak_nits=max(levels["p999/1000"], white_nits))"""
    h = np.asarray(h_m)
    bpp = int(bpp)
    if bpp not in (8, 10, 12):
        raise ValueError("light_levels: bpp is 8, 10 or 12")
    if h.ndim not in (1, 2) or h.shape[-1] != 1 << bpp:
        raise ValueError("light_levels: h_m is (B,) or (N, B) with one bin per code, B = %d" % (1 << bpp))
    h = h.astype(np.int64)
    nits = _eotf_nits(transfer, np.arange(1 << bpp, dtype=np.float64) / ((1 << bpp) - 1), float(peak_nits), float(white_nits))
    nits = np.asarray(nits, np.float64)
    total = h.sum(-1)
    some = total > 0
    top = hist_percentile(h, 1, 1)
    out = {"max_nits": np.where(some, nits[top], 0.),
           "avg_nits": (h * nits).sum(-1) / np.where(some, total, 1)}
    for num, den in percentiles:
        out["p%d/%d" % (num, den)] = np.where(some, nits[hist_percentile(h, num, den)], 0.)
    return {k: (float(v) if h.ndim == 1 else v) for k, v in out.items()}


# VP9HIP_WARP_*: the names acc_warp takes for interp and output
WARP_MODES = {"nearest": 0, "bilinear": 1}
WARP_OUTPUTS = {"residual": 0, "picture": 1}


def warp_layout(width, height, ss_h=1, ss_v=1):
    """(bytes of one pair, (Y, U, V byte offsets)) of an accumulated-residual output
    (vp9hip_warp_layout): tight 2-byte planes, Y then U then V."""
    off = (ctypes.c_int64 * 3)()
    stride = lib().vp9hip_warp_layout(int(width), int(height), int(ss_h), int(ss_v), ctypes.byref(off))
    _check("vp9hip_warp_layout", stride)
    return stride, tuple(off)


def _warp_names(fn, output, interp):
    if output not in WARP_OUTPUTS or interp not in WARP_MODES:
        raise Vp9HipError(fn, EINVAL)
    return WARP_MODES[interp], WARP_OUTPUTS[output]


def acc_warp_host(planes_a, planes_b, acc, serial_b, width, height, bpp, ss_h=1, ss_v=1, output="residual",
                  interp="nearest", mask=False):
    """One pair of the accumulated residual on the host, vp9hip_acc_warp_host, the C statement of
    the definition in include/vp9hip.h ("accumulated residual"): planes_a / planes_b are three 2-D
    arrays each (uint8 at 8 bits, else uint16; rows may be strided), acc a's ACC_CELL array
    (GH, GW), serial_b the serial of b's field. Returns (y, u, v), or (y, u, v, mask) with
    mask=True: int16 arrays (H, W), (CH, CW), (CH, CW), for output "picture" the uint16 codes'
    bit pattern; the mask uint8 (GH, GW)."""
    fn = "vp9hip_acc_warp_host"
    mode, outp = _warp_names(fn, output, interp)
    dt = np.uint8 if bpp == 8 else np.uint16
    width, height = int(width), int(height)
    stride, off = warp_layout(width, height, ss_h, ss_v)
    cw, ch = (width + ss_h) >> ss_h, (height + ss_v) >> ss_v
    gw, gh = 2 * ((width + 7) >> 3), 2 * ((height + 7) >> 3)

    def prep(planes):
        out = []
        for p, a in enumerate(planes):
            a = np.asarray(a)
            if a.ndim != 2 or a.dtype != dt:
                raise ValueError("acc_warp_host: planes must be 2-D %s arrays" % np.dtype(dt).name)
            if a.strides[1] != a.itemsize or a.strides[0] < 0:
                a = np.ascontiguousarray(a)
            pw, ph = (width, height) if p == 0 else (cw, ch)
            if a.shape[0] < ph or a.shape[1] < pw:
                raise ValueError("acc_warp_host: plane %d is smaller than %d x %d" % (p, pw, ph))
            out.append(a)
        if len(out) != 3:
            raise ValueError("acc_warp_host: three planes a frame")
        return out
    pa, pb = prep(planes_a), prep(planes_b)
    acc = np.ascontiguousarray(acc, ACC_CELL)
    if acc.shape != (gh, gw):
        raise ValueError("acc_warp_host: acc must be (%d, %d) cells" % (gh, gw))
    dst = np.full(stride // 2, 0x5a5a, np.int16)
    m = np.full((gh, gw), 0x5a, np.uint8) if mask else None
    ap, als = _plane_ptrs(pa)
    bp, bls = _plane_ptrs(pb)
    _check(fn, lib().vp9hip_acc_warp_host(ctypes.byref(ap), ctypes.byref(als), ctypes.byref(bp), ctypes.byref(bls),
                                          acc.ctypes.data, int(serial_b) & 0xffffffff, width, height, int(bpp), int(ss_h),
                                          int(ss_v), mode, outp, dst.ctypes.data, m.ctypes.data if mask else None))
    y = dst[:width * height].reshape(height, width)
    u = dst[off[1] // 2:off[1] // 2 + cw * ch].reshape(ch, cw)
    v = dst[off[2] // 2:off[2] // 2 + cw * ch].reshape(ch, cw)
    return (y, u, v, m) if mask else (y, u, v)


# VP9HIP_PROP_*: the names acc_propagate takes for layout, and its flag
PROP_LAYOUTS = {"nchw": 0, "nhwc": 1}
PROP_KEEP = 1


def _prop_names(fn, interp, layout):
    if interp not in WARP_MODES or layout not in PROP_LAYOUTS:
        raise Vp9HipError(fn, EINVAL)
    return WARP_MODES[interp], PROP_LAYOUTS[layout]


def _prop_dims(what, shape, layout):
    """(C, FH, FW, squeezed) of one item's shape: (C, FH, FW), (FH, FW, C) with layout "nhwc", or
    (FH, FW), which is C = 1."""
    if len(shape) == 2:
        return 1, int(shape[0]), int(shape[1]), True
    if len(shape) != 3:
        raise ValueError("%s: an item is (C, FH, FW), (FH, FW, C) with layout=\"nhwc\", or (FH, FW)" % what)
    if layout == "nhwc":
        return int(shape[2]), int(shape[0]), int(shape[1]), False
    return int(shape[0]), int(shape[1]), int(shape[2]), False


def _prop_desc(fn, size, c, fh, fw, esize, interp, layout, fill_bits, keep):
    """The PropDesc of a call; interp and layout are names."""
    mode, lay = _prop_names(fn, interp, layout)
    w, h = (int(x) for x in size)
    return PropDesc(w, h, fw, fh, c, esize, lay, mode, PROP_KEEP if keep else 0, 0, int(fill_bits) & 0xffffffffffffffff)


def prop_layout(desc):
    """(bytes of one item, bytes of one item's valid map) of a PropDesc (vp9hip_prop_layout)."""
    vb = ctypes.c_int64()
    item = lib().vp9hip_prop_layout(ctypes.byref(desc), ctypes.byref(vb))
    _check("vp9hip_prop_layout", item)
    return item, vb.value


def acc_propagate_host(acc, root_serial, src, width, height, interp="nearest", layout="nchw", fill=0, keep=False,
                       valid=False, out=None):
    """One pair of the accumulated propagation on the host, vp9hip_acc_propagate_host, the C
    statement of the definition in include/vp9hip.h ("accumulated propagation"): acc the frame's
    ACC_CELL array (GH, GW), root_serial the root's serial, src one source item, a numpy array
    (C, FH, FW), (FH, FW, C) with layout "nhwc", or (FH, FW), of 1, 2, 4 or 8-byte elements
    (float16 for interp "bilinear"). fill is a number converted to src's dtype; keep=True leaves
    `out` (an array like src, required then) where the cell does not apply. Returns the item, of
    src's dtype and shape, or (item, valid) with valid=True: uint8 (FH, FW)."""
    fn = "vp9hip_acc_propagate_host"
    src = np.ascontiguousarray(src)
    c, fh, fw, _ = _prop_dims("acc_propagate_host", src.shape, layout)
    if src.dtype.itemsize not in (1, 2, 4, 8):
        raise ValueError("acc_propagate_host: elements of 1, 2, 4 or 8 bytes")
    if interp == "bilinear" and src.dtype != np.float16:
        raise ValueError("acc_propagate_host: interp=\"bilinear\" needs float16")
    bits = int.from_bytes(np.array([fill]).astype(src.dtype).tobytes(), "little")
    d = _prop_desc(fn, (width, height), c, fh, fw, src.dtype.itemsize, interp, layout, bits, keep)
    gw, gh = 2 * ((int(width) + 7) >> 3), 2 * ((int(height) + 7) >> 3)
    acc = np.ascontiguousarray(acc, ACC_CELL)
    if acc.shape != (gh, gw):
        raise ValueError("acc_propagate_host: acc must be (%d, %d) cells" % (gh, gw))
    if keep and out is None:
        raise ValueError("acc_propagate_host: keep=True needs out=")
    if out is None:
        out = np.full(src.nbytes, 0x5a, np.uint8).view(src.dtype).reshape(src.shape)
    elif not (isinstance(out, np.ndarray) and out.dtype == src.dtype and out.shape == src.shape and out.flags.c_contiguous):
        raise ValueError("acc_propagate_host: out must be a contiguous array of src's dtype and shape")
    m = np.full((fh, fw), 0x5a, np.uint8) if valid else None
    _check(fn, lib().vp9hip_acc_propagate_host(acc.ctypes.data, int(root_serial) & 0xffffffff, ctypes.byref(d),
                                               src.ctypes.data, out.ctypes.data, m.ctypes.data if valid else None))
    return (out, m) if valid else out


def prop_launch_dev(acc_ptrs, acc_pitch, serials, src_index, m, desc, src_ptr, dst_ptr, valid_ptr=None, stream=None):
    """The propagation kernels over caller-made device fields (vp9hip_prop_launch_dev; the bench
    tool and the crafted-field tests): per pair the device pointer of the frame's field and the
    root's serial; acc_pitch the fields' pitch in cells, src_index the pairs' source items (None:
    pair i reads item i) of the m items at src_ptr, desc a PropDesc."""
    n = len(acc_ptrs)
    idx = (ctypes.c_int * max(n, 1))(*[int(x) for x in src_index]) if src_index is not None else None
    _check("vp9hip_prop_launch_dev",
           lib().vp9hip_prop_launch_dev((ctypes.c_void_p * max(n, 1))(*acc_ptrs), int(acc_pitch),
                                        (ctypes.c_uint32 * max(n, 1))(*[int(x) & 0xffffffff for x in serials]), idx, n, int(m),
                                        ctypes.byref(desc), src_ptr, dst_ptr, valid_ptr, stream))


def _prop_torch(what, n, src, size, interp, layout, fill, keep, valid, src_index, out, fn):
    """The checked arguments of an acc_propagate call over torch tensors: (PropDesc, M, src_index
    array or None, destination, uint8 (N, FH, FW) valid map or None)."""
    import torch
    esize = {torch.uint8: 1, torch.int8: 1, torch.int16: 2, torch.float16: 2, torch.bfloat16: 2, torch.int32: 4,
             torch.float32: 4, torch.int64: 8, torch.float64: 8}
    if not (isinstance(src, torch.Tensor) and src.is_cuda and src.is_contiguous() and src.dtype in esize and src.dim() in (3, 4)):
        raise ValueError("%s: src must be a contiguous cuda tensor (M, C, FH, FW), (M, FH, FW, C) or (M, FH, FW) of an "
                         "integer or floating type of 1, 2, 4 or 8 bytes" % what)
    if interp == "bilinear" and src.dtype != torch.float16:
        raise ValueError("%s: interp=\"bilinear\" needs float16" % what)
    if keep and out is None:
        raise ValueError("%s: keep=True needs out=" % what)
    m = int(src.shape[0])
    c, fh, fw, _ = _prop_dims(what, tuple(src.shape[1:]), layout)
    if src_index is None:
        if m != n and m != 1:
            raise ValueError("%s: src_index=None needs as many source items as pairs, or one" % what)
        idx = None if m == n else (ctypes.c_int * max(n, 1))()
    else:
        src_index = [int(x) for x in src_index]
        if len(src_index) != n:
            raise ValueError("%s: src_index and the pairs differ in length" % what)
        idx = (ctypes.c_int * max(n, 1))(*src_index)
    bits = int.from_bytes(bytes(torch.tensor([fill]).to(src.dtype).view(torch.uint8).tolist()), "little")
    d = _prop_desc(fn, size, c, fh, fw, esize[src.dtype], interp, layout, bits, keep)
    shape = (n,) + tuple(src.shape[1:])
    if out is None:
        out = torch.empty((max(n, 1),) + shape[1:], dtype=src.dtype, device=src.device)[:n]
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == src.dtype and tuple(out.shape) == shape
              and out.is_contiguous()):
        raise ValueError("%s: out must be a contiguous cuda tensor of src's dtype and shape %s" % (what, shape))
    v = torch.empty((max(n, 1), fh, fw), dtype=torch.uint8, device=src.device)[:n] if valid else None
    return d, m, idx, out, v


def _warp_out(n, width, height, ss_h, ss_v, mask, out):
    """The destinations of an acc_warp call: (flat int16 cuda tensor, (y, u, v) views of it,
    uint8 (N, GH, GW) mask or None). `out` is a contiguous int16 cuda tensor of at least
    N * stride / 2 elements, or None."""
    import torch
    sane = 1 <= width <= 16384 and 1 <= height <= 16384 and ss_h in (0, 1) and ss_v in (0, 1)
    stride, off = warp_layout(width, height, ss_h, ss_v) if sane else (2, (0, 0, 0))
    n = max(n, 0)
    need = n * stride // 2
    if out is None:
        out = torch.empty(max(need, 4), dtype=torch.int16, device="cuda")
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int16 and out.is_contiguous()
              and out.numel() >= need):
        raise ValueError("acc_warp: out must be a contiguous int16 cuda tensor of at least %d elements" % need)
    flat = out.view(-1)
    views, m = None, None
    if sane:
        cw, ch = (width + ss_h) >> ss_h, (height + ss_v) >> ss_v
        views = tuple(flat.as_strided((n, ph, pw), (stride // 2, pw, 1), flat.storage_offset() + o // 2)
                      for o, (pw, ph) in zip(off, ((width, height), (cw, ch), (cw, ch))))
        if mask:
            m = torch.empty((max(n, 1), 2 * ((height + 7) >> 3), 2 * ((width + 7) >> 3)), dtype=torch.uint8, device="cuda")[:n]
    elif mask:
        m = torch.empty((max(n, 1), 1, 1), dtype=torch.uint8, device="cuda")[:n]
    return flat, views, m


def warp_launch_dev(a_ptrs, b_ptrs, acc_ptrs, serials, plane_off, pitch, acc_pitch, width, height, bpp, ss_h, ss_v,
                    interp, output, dst_ptr, mask_ptr=None, stream=None):
    """k_acc_warp over caller-made device pictures and fields (vp9hip_warp_launch_dev; the bench
    tool and the crafted-field tests): per pair the device pointers of frame a, frame b and a's
    field and b's serial; plane_off the planes' byte offsets inside a frame, pitch the (luma,
    chroma) row pitch in bytes, acc_pitch the field's pitch in cells."""
    fn = "vp9hip_warp_launch_dev"
    mode, outp = _warp_names(fn, output, interp)
    n = len(a_ptrs)
    arr = lambda v: (ctypes.c_void_p * max(n, 1))(*v)   # noqa: E731
    _check(fn, lib().vp9hip_warp_launch_dev(arr(a_ptrs), arr(b_ptrs), arr(acc_ptrs),
                                            (ctypes.c_uint32 * max(n, 1))(*[int(x) & 0xffffffff for x in serials]), n,
                                            ctypes.byref((ctypes.c_int64 * 3)(*plane_off)),
                                            ctypes.byref((ctypes.c_int32 * 2)(*pitch)), int(acc_pitch), int(width), int(height),
                                            int(bpp), int(ss_h), int(ss_v), mode, outp, dst_ptr, mask_ptr, stream))


def _warpt_desc(fn, fmt, interp, coverage, resize, size, colorspace, full_range, pitch, frame_stride):
    """The WarptDesc of an acc_warp_tensors call: resize=None is the visible size itself."""
    if fmt not in RESID_FORMATS or interp not in WARP_MODES:
        raise Vp9HipError(fn, EINVAL)
    w, h = (int(x) for x in size)
    ow, oh = (int(x) for x in (resize if resize is not None else size))
    return WarptDesc(RESID_FORMATS[fmt], int(colorspace), int(bool(full_range)), WARP_MODES[interp], 4 if coverage else 3,
                     w, h, ow, oh, int(pitch), int(frame_stride))


def warpt_layout(fmt, resize, coverage=False, pitch=0, frame_stride=0):
    """(bytes of one pair, pitch in effect) of an accumulated residual at model size
    (vp9hip_warpt_layout): planar (3 or 4, OH, OW) 16-bit elements, resize = (OW, OH)."""
    d = _warpt_desc("vp9hip_warpt_layout", fmt, "nearest", coverage, resize, (1, 1), 2, 0, pitch, frame_stride)
    p = ctypes.c_int64()
    nbytes = lib().vp9hip_warpt_layout(ctypes.byref(d), ctypes.byref(p))
    _check("vp9hip_warpt_layout", nbytes)
    return nbytes, p.value


def acc_warp_scaled_host(planes_a, planes_b, acc, serial_b, width, height, bpp, ss_h, ss_v, fmt, resize, interp="nearest",
                         coverage=False, colorspace=2, full_range=False):
    """One pair of the accumulated residual at model size on the host,
    vp9hip_acc_warp_scaled_host, the C statement of the definition in include/vp9hip.h
    ("accumulated residual at model size"): the arguments of acc_warp_host, fmt a key of
    RESID_FORMATS, resize = (OW, OH) or None for the visible size. Returns a (3, OH, OW) int16 or
    float16 array, (4, OH, OW) with coverage=True: the last plane the coverage."""
    fn = "vp9hip_acc_warp_scaled_host"
    dt = np.uint8 if bpp == 8 else np.uint16
    width, height = int(width), int(height)
    d = _warpt_desc(fn, fmt, interp, coverage, resize, (width, height), colorspace, full_range, 0, 0)
    sane = 1 <= width <= 16384 and 1 <= height <= 16384 and ss_h in (0, 1) and ss_v in (0, 1)

    def prep(planes):
        out = []
        for p, a in enumerate(planes):
            a = np.asarray(a)
            if a.ndim != 2 or a.dtype != dt:
                raise ValueError("acc_warp_scaled_host: planes must be 2-D %s arrays" % np.dtype(dt).name)
            if a.strides[1] != a.itemsize or a.strides[0] < 0:
                a = np.ascontiguousarray(a)
            if sane:                                  # what the library refuses it does not read
                pw, ph = (width, height) if p == 0 else ((width + ss_h) >> ss_h, (height + ss_v) >> ss_v)
                if a.shape[0] < ph or a.shape[1] < pw:
                    raise ValueError("acc_warp_scaled_host: plane %d is smaller than %d x %d" % (p, pw, ph))
            out.append(a)
        if len(out) != 3:
            raise ValueError("acc_warp_scaled_host: three planes a frame")
        return out
    pa, pb = prep(planes_a), prep(planes_b)
    acc = np.ascontiguousarray(acc, ACC_CELL)
    if sane and acc.shape != (2 * ((height + 7) >> 3), 2 * ((width + 7) >> 3)):
        raise ValueError("acc_warp_scaled_host: acc must be (%d, %d) cells" % (2 * ((height + 7) >> 3), 2 * ((width + 7) >> 3)))
    ok = 1 <= d.out_width <= 16384 and 1 <= d.out_height <= 16384
    out = np.full((d.planes, d.out_height, d.out_width) if ok else (d.planes, 1, 1), 0x5a5a, np.int16)
    ap, als = _plane_ptrs(pa)
    bp, bls = _plane_ptrs(pb)
    _check(fn, lib().vp9hip_acc_warp_scaled_host(ctypes.byref(ap), ctypes.byref(als), ctypes.byref(bp), ctypes.byref(bls),
                                                 acc.ctypes.data, int(serial_b) & 0xffffffff, int(bpp), int(ss_h), int(ss_v),
                                                 ctypes.byref(d), out.ctypes.data))
    return out.view(np.float16) if fmt.endswith("f16") else out


def _warpt_out(n, d, out):
    """The destination of an acc_warp_tensors call, as _resid_out's: (flat storage tensor,
    (N, P, OH, OW) view of it, or None for a descriptor the library refuses)."""
    import torch
    dt = torch.float16 if d.format & 1 else torch.int16
    pitch = ctypes.c_int64()
    nbytes = lib().vp9hip_warpt_layout(ctypes.byref(d), ctypes.byref(pitch))
    if nbytes < 0:
        flat = out.view(-1) if out is not None else torch.empty(1, dtype=dt, device="cuda")
        return flat, None
    stride = d.frame_stride or nbytes
    total = ((max(n, 1) - 1) * stride + nbytes) // 2
    if out is None:
        out = torch.empty(total, dtype=dt, device="cuda")
    elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == dt and out.is_contiguous()
              and out.numel() >= total):
        raise ValueError("acc_warp_tensors: out must be a contiguous %s cuda tensor of at least %d elements" % (dt, total))
    flat = out.view(-1)
    return flat, flat.as_strided((max(n, 0), d.planes, d.out_height, d.out_width),
                                 (stride // 2, pitch.value * d.out_height // 2, pitch.value // 2, 1))


def warp_scale_launch_dev(a_ptrs, b_ptrs, acc_ptrs, serials, plane_off, pitch, acc_pitch, width, height, bpp, ss_h, ss_v,
                          fmt, resize, dst_ptr, interp="nearest", coverage=False, colorspace=2, full_range=False,
                          out_pitch=0, frame_stride=0, stream=None):
    """k_acc_warp_scale over caller-made device pictures and fields (vp9hip_warp_scale_launch_dev;
    the bench tool and the crafted-field tests): the pictures and fields as warp_launch_dev takes
    them, the output as acc_warp_scaled_host describes it, written at dst_ptr."""
    fn = "vp9hip_warp_scale_launch_dev"
    d = _warpt_desc(fn, fmt, interp, coverage, resize, (width, height), colorspace, full_range, out_pitch, frame_stride)
    n = len(a_ptrs)
    arr = lambda v: (ctypes.c_void_p * max(n, 1))(*v)   # noqa: E731
    _check(fn, lib().vp9hip_warp_scale_launch_dev(arr(a_ptrs), arr(b_ptrs), arr(acc_ptrs),
                                                  (ctypes.c_uint32 * max(n, 1))(*[int(x) & 0xffffffff for x in serials]), n,
                                                  ctypes.byref((ctypes.c_int64 * 3)(*plane_off)),
                                                  ctypes.byref((ctypes.c_int32 * 2)(*pitch)), int(acc_pitch), int(bpp),
                                                  int(ss_h), int(ss_v), ctypes.byref(d), dst_ptr, stream))


def psnr(metrics, bpp, width, height, ss_h=1, ss_v=1):
    """PSNR in dB of each plane from metrics records (a host array (..., 3, 8), e.g.
    Device.metrics(...).cpu()): float64 (..., 3), 10 log10((2^bpp - 1)^2 count / sse) with count
    the plane's visible samples; inf where sse is 0."""
    m = np.asarray(metrics)
    if m.shape[-2:] != (3, len(METRIC_FIELDS)):
        raise ValueError("psnr: metrics must be (..., 3, %d)" % len(METRIC_FIELDS))
    cw, ch = (width + ss_h) >> ss_h, (height + ss_v) >> ss_v
    count = np.array([width * height, cw * ch, cw * ch], np.float64)
    sse = m[..., METRIC_FIELDS.index("sse")].astype(np.float64)
    peak = float((1 << bpp) - 1) ** 2
    with np.errstate(divide="ignore"):
        return np.where(sse == 0, np.inf, 10.0 * np.log10(peak * count / np.where(sse == 0, 1.0, sse)))


def alloc_planes(width, height, bpp, ss_h=1, ss_v=1, pad=64):
    """Host planes padded to 64 luma pixels (the layout the oracle expects)."""
    dt = np.uint8 if bpp == 8 else np.uint16
    W = (width + pad - 1) // pad * pad
    H = (height + pad - 1) // pad * pad
    return [np.zeros((H, W), dt), np.zeros((H >> ss_v, W >> ss_h), dt), np.zeros((H >> ss_v, W >> ss_h), dt)]


def visible(planes, width, height, ss_h=1, ss_v=1):
    cw, ch = (width + ss_h) >> ss_h, (height + ss_v) >> ss_v
    return [planes[0][:height, :width], planes[1][:ch, :cw], planes[2][:ch, :cw]]


def decode_frame(data):
    """Host entropy decode of one VP9 frame -> DecodedFrame (pass-1 packet)."""
    return DecodedFrame(data)


def test_hooks(reject_batch=0, lfr_spin=0, reject_frame=0):
    """Test hooks copied by every context opened afterwards (vp9hip_test_hooks): frame
    reject_frame of the reject_batch-th batch a context stages starts with an intra block
    whose mode the planner rejects; lfr_spin bounds the row loop filter's hand-off waits
    (0, 0: off)."""
    lib().vp9hip_test_hooks(int(reject_batch) | int(reject_frame) << 16 if reject_batch else 0, int(lfr_spin))


def device_info(device):
    """(PCI bus id, name) of HIP device `device` (vp9hip_device_info)."""
    bus, name = ctypes.create_string_buffer(64), ctypes.create_string_buffer(256)
    _check("vp9hip_device_info", lib().vp9hip_device_info(device, bus, 64, name, 256))
    return bus.value.decode(), name.value.decode()


def _enqueue_for_torch(ctx_stream, stream, launch):
    """Run launch(hipStream_t handle or None) so that it is ordered like work on torch's current
    stream. An explicit `stream` handle, or a current stream of torch's own, is used as it is.
    torch's default stream is the null stream, which the C ABI cannot name (NULL selects the
    context's main stream, a non-blocking one): then the launch goes to the context's main
    stream `ctx_stream`, which first waits for torch's stream and is waited for by it afterwards."""
    import torch
    if stream is not None:
        return launch(stream)
    cur = torch.cuda.current_stream()
    if cur.cuda_stream:
        return launch(cur.cuda_stream)
    ext = torch.cuda.ExternalStream(ctx_stream)
    ext.wait_stream(cur)
    r = launch(None)
    cur.wait_stream(ext)
    return r


class Device:
    """A vp9hip context on one GPU (vp9hip_open / vp9hip_configure)."""

    def __init__(self, device=0):
        self._c = ctypes.c_void_p()
        _check("vp9hip_open", lib().vp9hip_open(device, ctypes.byref(self._c)))
        self.w = self.h = 0
        self.bpp = 8

    def close(self):
        if self._c:
            lib().vp9hip_close(self._c)
            self._c = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def configure(self, width, height, bpp=8, nbufs=4, ss_h=1, ss_v=1):
        _check("vp9hip_configure", lib().vp9hip_configure(self._c, width, height, bpp, ss_h, ss_v, nbufs))
        self.w, self.h, self.bpp, self.ss_h, self.ss_v = width, height, bpp, ss_h, ss_v

    def set_export(self, motion=True, residual=False, motion_acc=False):
        """Motion and / or residual export on / off for the next configure (vp9hip_set_export):
        every batch then leaves each frame's motion field (motion / download_motion) and / or
        residual field (residual / download_residual) beside its pixels; motion_acc (only with
        motion) adds the accumulated motion field (motion_acc / download_motion_acc)."""
        _check("vp9hip_set_export", lib().vp9hip_set_export(self._c, (EXPORT_MOTION if motion else 0) |
                                                            (EXPORT_RESIDUAL if residual else 0) |
                                                            (EXPORT_MOTION_ACC if motion_acc else 0)))

    def frame_motion_acc(self, buf):
        """The accumulated field of buffer `buf` in place (vp9hip_frame_motion_acc): (pointer,
        (GW, GH), pitch in cells, serial, hipStream_t handle)."""
        acc, st = ctypes.c_void_p(), ctypes.c_void_p()
        gw, gh, pitch, ser = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64(), ctypes.c_uint32()
        _check("vp9hip_frame_motion_acc", lib().vp9hip_frame_motion_acc(self._c, buf, ctypes.byref(acc), ctypes.byref(gw),
                                                                        ctypes.byref(gh), ctypes.byref(pitch),
                                                                        ctypes.byref(ser), ctypes.byref(st)))
        return acc.value, (gw.value, gh.value), pitch.value, ser.value, st.value

    def motion_acc(self, buf, device=None):
        """Zero-copy torch int32 view (GH, GW, 4) of buffer `buf`'s accumulated motion field,
        strided over the plane's pitch: columns dx, dy, root, hops | end << 16 (acc_fields splits
        them). Call sync() first (or order consumers after the slot that wrote the frame)."""
        acc, (gw, gh), pitch, _, _ = self.frame_motion_acc(buf)
        return _acc_view(acc, gw, gh, pitch, device)

    def download_motion_acc(self, buf):
        """Buffer `buf`'s accumulated motion field as a numpy ACC_CELL array (GH, GW), and its
        serial (vp9hip_download_motion_acc; waits for the batches writing the buffer)."""
        _, (gw, gh), _, _, _ = self.frame_motion_acc(buf)
        cells, ser = np.empty((gh, gw), ACC_CELL), ctypes.c_uint32()
        _check("vp9hip_download_motion_acc", lib().vp9hip_download_motion_acc(self._c, buf, cells.ctypes.data, ctypes.byref(ser)))
        return cells, ser.value

    def frame_residual(self, buf):
        """The residual field of buffer `buf` in place (vp9hip_frame_residual): ([ptr] * 3,
        [pitch in int16 elements] * 3, (width, height) of the frame, hipStream_t handle)."""
        ptrs, pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)()
        w, h, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p()
        _check("vp9hip_frame_residual", lib().vp9hip_frame_residual(self._c, buf, ctypes.byref(ptrs), ctypes.byref(pitch),
                                                                    ctypes.byref(w), ctypes.byref(h), ctypes.byref(st)))
        return list(ptrs), list(pitch), (w.value, h.value), st.value

    def residual(self, buf, device=None):
        """Zero-copy torch int16 views (Y, U, V) of buffer `buf`'s residual field, of the frame's
        visible size, strided over the planes' pitch. Call sync() first (or order consumers
        after the slot that wrote the frame), as for frame_tensors."""
        ptrs, pitch, (w, h), _ = self.frame_residual(buf)
        return _residual_views(ptrs, pitch, w, h, self.ss_h, self.ss_v, device)

    def download_residual(self, buf):
        """Buffer `buf`'s residual field as three numpy int16 arrays of the coded area
        (residual_shapes; vp9hip_download_residual, which waits for the batches writing the
        buffer)."""
        _, _, (w, h), _ = self.frame_residual(buf)
        planes = [np.empty(s, np.int16) for s in residual_shapes(w, h, self.ss_h, self.ss_v)]
        ptrs, ls = _plane_ptrs(planes)
        _check("vp9hip_download_residual", lib().vp9hip_download_residual(self._c, buf, ctypes.byref(ptrs), ctypes.byref(ls)))
        return planes

    def residual_tensors(self, bufs, fmt, resize=None, colorspace=2, full_range=False, out=None, stream=None,
                         pitch=0, frame_stride=0):
        """The residual fields of device buffers `bufs` (any order, repeats allowed, all of one
        visible size) as one (N, 3, OH, OW) cuda tensor at the model's size, made on the GPU in
        one launch per 32 frames (vp9hip_residual_frames_scaled, the definition in
        include/vp9hip.h "residual tensors at model size"): cropped to the visible size, all
        three planes box-resampled to resize = (OW, OH) with the exact signed box filter (None:
        the field's own size, the identity, through the same kernel), and by fmt "yuv_i16" the
        planes y, u, v as int16, "rgb_i16" the RGB residual of the colour matrix `colorspace`
        (the VP9 code, 1..5, 7 = RGB planes) / full_range clipped to [-m, m], m = 2^bpp - 1, or
        "yuv_f16" / "rgb_f16" the same values times 1 / m as float16. `out` is a contiguous
        int16 / float16 cuda tensor to write into (else one is allocated); pitch / frame_stride
        in bytes as in vp9hip_resid_desc (0 = tight), the result then strided over them. Runs in
        the order of torch's current stream (or on `stream`, a hipStream_t handle; see
        _enqueue_for_torch) and does not wait: order it after the fields' producer (sync(), or
        vp9hip_slot_stream_wait), as for convert. Needs torch imported before the library was
        loaded (see _torch_first)."""
        fn = "vp9hip_residual_frames_scaled"
        if not _torch_first:
            raise Vp9HipUnavailable("residual_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        bufs = [int(b) for b in bufs]
        if not bufs:
            raise Vp9HipError(fn, EINVAL)
        size = (1, 1)
        if resize is None:
            size = self.frame_residual(bufs[0])[2]
        d = _resid_desc(fn, fmt, resize, size, colorspace, full_range, pitch, frame_stride)
        flat, res = _resid_out(len(bufs), d, out)
        arr = (ctypes.c_int * len(bufs))(*bufs)
        call = lambda st: lib().vp9hip_residual_frames_scaled(self._c, arr, len(bufs), ctypes.byref(d), flat.data_ptr(), st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check(fn, call(stream))
        else:
            _check(fn, _enqueue_for_torch(main.value, stream, call))
        return res

    def motion_tensors(self, bufs, fmt, resize=None, source="coded", mask=False, size=None, out=None, stream=None,
                       pitch=0, frame_stride=0):
        """The motion fields (source "coded") or accumulated motion fields (source "acc") of
        device buffers `bufs` (any order, repeats allowed, all of the visible size `size` =
        (width, height), default the configured size) as one (N, 2 or 3, OH, OW) cuda tensor at
        the model's size, made on the GPU in one launch per 32 frames
        (vp9hip_motion_frames_scaled, the definition in include/vp9hip.h "motion tensors at
        model size"): every cell's first vector (intra cells, and acc cells of no hops, as zero;
        acc sums clamped to int16) spread over its 4 x 4 pixels, cropped to the visible size and
        box-resampled to resize = (OW, OH) with the exact signed box filter (None: the visible
        size, the dense field itself, through the same kernel). Planes x, y and with mask=True
        the inter coverage. fmt "i16": int16 in 1/8 luma pel of the source, the coverage
        0..256; "f16": float16 displacement in output pixels, the coverage 0..1. `out` is a
        contiguous int16 / float16 cuda tensor to write into (else one is allocated); pitch /
        frame_stride in bytes as in vp9hip_mvt_desc (0 = tight), the result then strided over
        them. Runs in the order of torch's current stream (or on `stream`, a hipStream_t handle;
        see _enqueue_for_torch) and does not wait: order it after the fields' producer (sync(),
        or vp9hip_slot_stream_wait), as for convert. Needs torch imported before the library was
        loaded (see _torch_first)."""
        fn = "vp9hip_motion_frames_scaled"
        if not _torch_first:
            raise Vp9HipUnavailable("motion_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        bufs = [int(b) for b in bufs]
        if not bufs:
            raise Vp9HipError(fn, EINVAL)
        d = _mvt_desc(fmt, source, mask, resize, size if size is not None else (self.w, self.h), pitch, frame_stride)
        flat, res = _mvt_out(len(bufs), d, out)
        arr = (ctypes.c_int * len(bufs))(*bufs)
        call = lambda st: lib().vp9hip_motion_frames_scaled(self._c, arr, len(bufs), ctypes.byref(d), flat.data_ptr(), st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check(fn, call(stream))
        else:
            _check(fn, _enqueue_for_torch(main.value, stream, call))
        return res

    def frame_motion(self, buf):
        """The field of buffer `buf` in place (vp9hip_frame_motion): (mv pointer, info pointer,
        (GW, GH), pitch in cells, hipStream_t handle)."""
        mv, info, st = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        gw, gh, pitch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _check("vp9hip_frame_motion", lib().vp9hip_frame_motion(self._c, buf, ctypes.byref(mv), ctypes.byref(info),
                                                                ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(pitch),
                                                                ctypes.byref(st)))
        return mv.value, info.value, (gw.value, gh.value), pitch.value, st.value

    def motion(self, buf, device=None):
        """Zero-copy torch views (mv, info) of buffer `buf`'s motion field: int16 (GH, GW, 2, 2)
        and uint8 (GH, GW, 4), strided over the planes' fixed pitch. Call sync() first (or order
        consumers after the slot that wrote the frame), as for frame_tensors."""
        mv, info, (gw, gh), pitch, _ = self.frame_motion(buf)
        return _motion_views(mv, info, gw, gh, pitch, device)

    def download_motion(self, buf):
        """Buffer `buf`'s motion field as numpy arrays (mv, info) of motion()'s shapes
        (vp9hip_download_motion; waits for the batches writing the buffer)."""
        _, _, (gw, gh), _, _ = self.frame_motion(buf)
        mv, info = np.empty((gh, gw, 2, 2), np.int16), np.empty((gh, gw, 4), np.uint8)
        _check("vp9hip_download_motion", lib().vp9hip_download_motion(self._c, buf, mv.ctypes.data, info.ctypes.data))
        return mv, info

    def submit(self, frame, out_buf, refs=(0, 0, 0)):
        r = (ctypes.c_int * 3)(*refs)
        pkt = frame.pkt if hasattr(frame, "pkt") else frame
        _check("vp9hip_submit_frame", lib().vp9hip_submit_frame(self._c, ctypes.byref(pkt), out_buf, r))

    def stage_batch(self, frames, out_bufs, ref_bufs=None, tiles=None):
        """Stage a batch; ref_bufs: per frame (LAST, GOLDEN, ALTREF) buffer ids or None
        (keyframes). Dependent frames are chained, independent chains run concurrently.
        tiles=(lo, hi): reconstruct only tile columns [lo, hi) (a shard of a tile-sharded
        stream, run with run_phase; see tileshard.py)."""
        arr = (FramePacket * len(frames))(*[f.pkt if hasattr(f, "pkt") else f for f in frames])
        ob = (ctypes.c_int * len(out_bufs))(*out_bufs)
        self._staged = (arr, frames)   # keep host packets alive
        if ref_bufs is None and tiles is None:
            _check("vp9hip_stage_batch", lib().vp9hip_stage_batch(self._c, arr, len(frames), ob))
            return
        flat = []
        for r in (ref_bufs if ref_bufs is not None else [None] * len(frames)):
            flat += list(r) if r is not None else [0, 0, 0]
        rb = (ctypes.c_int * len(flat))(*flat)
        if tiles is not None:
            _check("vp9hip_stage_batch_tiles",
                   lib().vp9hip_stage_batch_tiles(self._c, arr, len(frames), ob, rb, int(tiles[0]), int(tiles[1])))
            return
        _check("vp9hip_stage_batch_refs", lib().vp9hip_stage_batch_refs(self._c, arr, len(frames), ob, rb))

    PART_RECON, PART_LF = 0, 1
    MAX_SLOTS = 4                  # VP9HIP_MAX_SLOTS (include/vp9hip.h)

    def set_slot(self, slot):
        """Select batch slot 0 .. MAX_SLOTS - 1 (vp9hip_set_batch_slot): staged batches run in
        turn overlap one batch's device planning and pixel chains with the others'."""
        _check("vp9hip_set_batch_slot", lib().vp9hip_set_batch_slot(self._c, int(slot)))

    def phases(self):
        """Number of phases (chain positions) of the staged batch."""
        return _check("vp9hip_batch_phases", lib().vp9hip_batch_phases(self._c))

    def groups(self):
        """Frame groups (concurrent HIP streams) of the staged batch."""
        return _check("vp9hip_batch_groups", lib().vp9hip_batch_groups(self._c))

    def phase_frames(self, phase):
        """Batch indices of the frames in `phase`."""
        n = _check("vp9hip_phase_frames", lib().vp9hip_phase_frames(self._c, phase, None, 0))
        a = (ctypes.c_int * max(n, 1))()
        _check("vp9hip_phase_frames", lib().vp9hip_phase_frames(self._c, phase, a, n))
        return list(a[:n])

    def run_phase(self, phase, part):
        _check("vp9hip_run_phase", lib().vp9hip_run_phase(self._c, phase, part))

    def stripe(self, frame, tile_lo, tile_hi, dev_ptr=None, to_frame=False):
        """Pack / unpack the pre-LF columns of tile columns [lo, hi) of batch frame `frame`
        to / from device memory at dev_ptr (an int address); returns the byte count."""
        return _check("vp9hip_stripe", lib().vp9hip_stripe(self._c, frame, tile_lo, tile_hi,
                                                           ctypes.c_void_p(dev_ptr) if dev_ptr else None,
                                                           int(bool(to_frame))))

    def run_batch(self):
        _check("vp9hip_run_batch", lib().vp9hip_run_batch(self._c))

    def plan_records(self):
        """Test only (vp9hip_test_plan_records): the device planner's intra schedule of the current
        slot's batch, read back once the device is idle. Returns (sbs, wgs, passes, jobs_a):
        uint32 arrays of shape (slots, 3), (slots, 4), (slots, jcap) and (slots, jcap)."""
        jcap = ctypes.c_int()
        ns = _check("vp9hip_test_plan_records", lib().vp9hip_test_plan_records(self._c, 0, ctypes.byref(jcap), None, None,
                                                                               None, None))
        sbs, wgs = np.empty((ns, 3), np.uint32), np.empty((ns, 4), np.uint32)
        passes, jobs = np.empty((ns, jcap.value), np.uint32), np.empty((ns, jcap.value), np.uint32)
        _check("vp9hip_test_plan_records", lib().vp9hip_test_plan_records(self._c, ns, ctypes.byref(jcap), sbs.ctypes.data,
                                                                          wgs.ctypes.data, passes.ctypes.data, jobs.ctypes.data))
        return sbs, wgs, passes, jobs

    def sync(self):
        _check("vp9hip_sync", lib().vp9hip_sync(self._c))

    def sync_slot(self, slot):
        """Wait for batch slot `slot`'s last run and check its loop-filter hand-offs."""
        _check("vp9hip_sync_slot", lib().vp9hip_sync_slot(self._c, int(slot)))

    def frame_status(self, slot):
        """Per-frame outcome of the slot's last stage / run after it reported
        AVERROR_INVALIDDATA (vp9hip_batch_frame_status): 0 reconstructed, EINVALIDDATA
        rejected, EAGAIN valid but not run."""
        n = _check("vp9hip_batch_frame_status", lib().vp9hip_batch_frame_status(self._c, int(slot), None, 0))
        a = (ctypes.c_int * max(n, 1))()
        _check("vp9hip_batch_frame_status", lib().vp9hip_batch_frame_status(self._c, int(slot), a, n))
        return list(a[:n])

    def fill(self, buf0, count, value):
        """Fill device buffers [buf0, buf0 + count) with byte `value` (async, context stream)."""
        _check("vp9hip_fill_buffers", lib().vp9hip_fill_buffers(self._c, int(buf0), int(count), int(value)))

    def set_timing(self, on):
        _check("vp9hip_set_timing", lib().vp9hip_set_timing(self._c, int(bool(on))))

    def timing(self):
        names = (ctypes.c_char_p * 8)()
        ms = (ctypes.c_double * 8)()
        cnt = (ctypes.c_int * 8)()
        n = _check("vp9hip_last_timing", lib().vp9hip_last_timing(self._c, names, ms, cnt, 8))
        return {names[i].decode(): (ms[i], cnt[i]) for i in range(n)}

    def alg_bytes(self):
        """Algorithmic bytes of the staged batch per kernel class, keyed like timing()."""
        b = (ctypes.c_double * 8)()
        n = _check("vp9hip_alg_bytes", lib().vp9hip_alg_bytes(self._c, b, 8))
        names = list(self.timing().keys())
        return {names[i]: b[i] for i in range(n)}

    def _plane_args(self, planes):
        ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])
        ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in planes])
        return ptrs, ls

    def download(self, buf):
        planes = alloc_planes(self.w, self.h, self.bpp, self.ss_h, self.ss_v)
        ptrs, ls = self._plane_args(planes)
        _check("vp9hip_download_frame", lib().vp9hip_download_frame(self._c, buf, ptrs, ls))
        return planes

    def frame_device(self, buf):
        """Device planes of buffer `buf` without a copy: ([ptr] * 3, [pitch bytes] * 3,
        (width, height), hipStream_t handle) -- vp9hip_frame_device."""
        ptrs = (ctypes.c_void_p * 3)()
        ls = (ctypes.c_ssize_t * 3)()
        w, h, st = ctypes.c_int(), ctypes.c_int(), ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self._c, buf, ptrs, ls, ctypes.byref(w), ctypes.byref(h),
                                                                ctypes.byref(st)))
        return list(ptrs), list(ls), (w.value, h.value), st.value

    def frame_tensors(self, buf, device=None):
        """Zero-copy torch views (uint8 / int16 storage of the u16 samples) of buffer
        `buf`'s visible planes, via __cuda_array_interface__. Call sync() first (or order
        consumers after the context's stream). Needs torch imported before the library was
        loaded (see _torch_first)."""
        if not _torch_first:
            raise Vp9HipUnavailable("frame_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        ptrs, ls, (w, h), _ = self.frame_device(buf)
        bpp = 1 if self.bpp == 8 else 2
        out = []
        for p in range(3):
            pw = w if p == 0 else (w + self.ss_h) >> self.ss_h
            ph = h if p == 0 else (h + self.ss_v) >> self.ss_v

            class _View:
                __cuda_array_interface__ = {"shape": (ph, pw), "typestr": "|u1" if bpp == 1 else "<i2",
                                            "data": (ptrs[p], False), "strides": (ls[p], bpp), "version": 2}
            out.append(torch.as_tensor(_View(), device=device or "cuda"))
        return out

    @staticmethod
    def _convert_out(n, fmt, w, h, bpp, ss_h, ss_v, out, pitch, frame_stride):
        """The destination of a conversion: (storage tensor, result, pitch, frame stride). The
        storage is a flat uint8 tensor (allocated, or `out` itself: a contiguous uint8 cuda
        tensor of at least the layout's bytes); the result is the strided view(s) of it that
        convert() returns."""
        import torch
        nbytes, pitch, off = out_layout(fmt, w, h, bpp, ss_h, ss_v, pitch, frame_stride)
        stride = frame_stride or nbytes
        total = (n - 1) * stride + nbytes
        if out is None:
            out = torch.empty(total, dtype=torch.uint8, device="cuda")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                  and out.numel() >= total):
            raise ValueError("convert: out must be a contiguous uint8 cuda tensor of at least %d bytes" % total)
        flat = out.view(-1)
        if fmt == "rgb24":
            return flat, flat.as_strided((n, h, w, 3), (stride, pitch, 3, 1)), pitch, stride
        if fmt == "rgbp_u8":
            return flat, flat.as_strided((n, 3, h, w), (stride, off[1], pitch, 1)), pitch, stride
        if fmt == "rgbp_f16":
            if flat.data_ptr() & 1 or stride & 1:
                raise ValueError("convert: half output needs an even address and frame stride")
            half = flat[:total // 2 * 2].view(torch.float16)
            return flat, half.as_strided((n, 3, h, w), (stride // 2, off[1] // 2, pitch // 2, 1)), pitch, stride
        cw, ch = (w + ss_h) >> ss_h, (h + ss_v) >> ss_v
        if bpp == 8:
            return flat, (flat.as_strided((n, h, w), (stride, pitch, 1)),
                          flat[off[1]:].as_strided((n, ch, cw, 2), (stride, pitch, 2, 1))), pitch, stride
        if flat.data_ptr() & 1 or stride & 1:
            raise ValueError("convert: 16-bit output needs an even address and frame stride")
        wide = flat[:total // 2 * 2].view(torch.int16)
        return flat, (wide.as_strided((n, h, w), (stride // 2, pitch // 2, 1)),
                      wide[off[1] // 2:].as_strided((n, ch, cw, 2), (stride // 2, pitch // 2, 2, 1))), pitch, stride

    @staticmethod
    def _resize_arg(fn, resize):
        """(OW, OH) of a resize argument; outside 1..16384 is refused as the library refuses it."""
        ow, oh = (int(x) for x in resize)
        if not (1 <= ow <= 16384 and 1 <= oh <= 16384):
            raise Vp9HipError(fn, EINVAL)
        return ow, oh

    def grade(self, fmt, in_lut=None, m=None, out_lut=None):
        """A Grade for convert(grade=...) with its tables in this device's memory
        (vp9hip_grade_create): grade(g) of a host Grade (make_grade's, grade_for's), or
        grade(fmt, in_lut, m, out_lut) at the configured depth."""
        g = fmt if isinstance(fmt, Grade) else Grade(self.bpp, fmt, in_lut, m, out_lut)
        return g._on(self._c)

    def convert(self, bufs, fmt, colorspace=2, full_range=False, size=None, out=None, stream=None,
                pitch=0, frame_stride=0, resize=None, filter="box", src_rects=None, dst_rects=None, fill=None, grade=None):
        """Convert device buffers `bufs` (any order) to `fmt` on the GPU (vp9hip_convert_frames):
        "rgb24" -> (N,H,W,3) uint8, "rgbp_u8" -> (N,3,H,W) uint8, "rgbp_f16" -> (N,3,H,W)
        float16 in [0,1], "semiplanar" -> (y, uv) views of one allocation, (N,H,W) and
        (N,CH,CW,2), uint8 (NV12 style) or, above 8 bits, int16 storage of the MSB-aligned
        samples (P010 style) as frame_tensors does. colorspace is the VP9 code (1..5, 7 = RGB
        planes), size the visible (width, height) (default: the configured size). `out` is a
        contiguous uint8 cuda tensor to write into (else one is allocated); pitch / frame_stride
        as in vp9hip_out_desc (0 = tight). resize=(OW, OH) resamples the visible picture to OW x OH
        with the exact box filter in the same launch (vp9hip_convert_frames_scaled; the shapes,
        `out`, pitch and frame_stride are then the output's, the UV view (N,OCH,OCW,2)); a given
        resize always takes that kernel, None is the unscaled one. With resize, filter="triangle"
        (antialiased bilinear; "box" is the default), src_rects (one (x, y, w, h) in luma samples,
        or one per frame: the region resampled instead of the whole visible picture), dst_rects
        (likewise: where in the OW x OH output the picture goes, see letterbox_rect) and fill (the
        three sample codes written elsewhere; default black by the range in effect) take
        vp9hip_convert_frames_resampled, the exact definitions of include/vp9hip.h;
        filter="bicubic" (Keys a = -1/2, antialiased when downscaling, clipped: within one code of
        torch's interpolate(mode="bicubic", antialias=True)) takes the same arguments through
        vp9hip_convert_frames_bicubic; any of them without resize is a ValueError. grade (what
        Device.grade returns; RGB formats only, "semiplanar" is a ValueError) passes every stored
        pixel through the grade's in_lut, matrix and out_lut in the same launch
        (vp9hip_convert_frames_graded, any filter; without resize the visible size, which is the
        box filter at equal size). Runs in the order of torch's current stream (or on
        `stream`, a hipStream_t handle; see _enqueue_for_torch) and does not wait: order it after the frames' producer (sync(), or
        vp9hip_slot_stream_wait), as for frame_tensors. Needs torch imported before the library
        was loaded (see _torch_first)."""
        if not _torch_first:
            raise Vp9HipUnavailable("convert: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        bufs = [int(b) for b in bufs]
        w, h = size if size is not None else (self.w, self.h)
        d = OutDesc(OUT_FORMATS[fmt], int(colorspace), int(bool(full_range)), int(w), int(h), int(pitch), int(frame_stride))
        rs = _resample_arg(len(bufs), resize, filter, src_rects, dst_rects, fill, self.bpp, int(colorspace), full_range)
        if grade is not None:
            gh = _grade_handle(grade, fmt)
            if rs is None:
                rs = Resample(FILTERS["box"], *(int(x) for x in (resize if resize is not None else (w, h))))
        fn = ("vp9hip_convert_frames_graded" if grade is not None else
              "vp9hip_convert_frames" if resize is None else
              "vp9hip_convert_frames_scaled" if rs is None else
              "vp9hip_convert_frames_bicubic" if rs.filter == FILTER_BICUBIC else "vp9hip_convert_frames_resampled")
        if not bufs:
            raise Vp9HipError(fn, EINVAL)
        ow, oh = (w, h) if resize is None else self._resize_arg(fn, resize)
        flat, res, _, _ = self._convert_out(len(bufs), fmt, ow, oh, self.bpp, self.ss_h, self.ss_v, out, pitch, frame_stride)
        arr = (ctypes.c_int * len(bufs))(*bufs)
        if grade is not None:
            call = lambda st: lib().vp9hip_convert_frames_graded(self._c, arr, len(bufs), ctypes.byref(d), ctypes.byref(rs), gh,
                                                                 flat.data_ptr(), st)
        elif rs is not None:
            call = lambda st: getattr(lib(), fn)(self._c, arr, len(bufs), ctypes.byref(d), ctypes.byref(rs), flat.data_ptr(), st)
        elif resize is None:
            call = lambda st: lib().vp9hip_convert_frames(self._c, arr, len(bufs), ctypes.byref(d), flat.data_ptr(), st)
        else:
            call = lambda st: lib().vp9hip_convert_frames_scaled(self._c, arr, len(bufs), ctypes.byref(d), ow, oh,
                                                                 flat.data_ptr(), st)
        _check(fn, _enqueue_for_torch(self.frame_device(0)[3], stream, call))
        return res

    letterbox_rect = staticmethod(letterbox_rect)

    @staticmethod
    def _metrics_out(n, w, h, cells, out):
        """The destinations of a metrics call: ((N, 3, 8) int64 view, (N, MH, MW) int32 map or
        None). `out` is a contiguous int64 cuda tensor of at least N * 24 elements, or None."""
        import torch
        need = max(n, 0) * 3 * len(METRIC_FIELDS)
        if out is None:
            out = torch.empty(max(need, 1), dtype=torch.int64, device="cuda")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous()
                  and out.numel() >= need):
            raise ValueError("metrics: out must be a contiguous int64 cuda tensor of at least %d elements" % need)
        res = out.view(-1)[:need].view(max(n, 0), 3, len(METRIC_FIELDS))
        cmap = None
        if cells:
            mh, mw = _metric_map_shape(w, h) if 1 <= w <= 16384 and 1 <= h <= 16384 else (1, 1)
            cmap = torch.empty((max(n, 1), mh, mw), dtype=torch.int32, device="cuda")[:max(n, 0)]
        return res, cmap

    def metrics(self, bufs_a, bufs_b=None, size=None, cells=False, out=None, stream=None):
        """The exact frame metrics of the pairs (bufs_a[i], bufs_b[i]) of device buffers on the GPU
        (vp9hip_frame_metrics, the definition in include/vp9hip.h): an (N, 3, 8) int64 cuda
        tensor, pair by plane by METRIC_FIELDS, over the top-left `size` = (width, height) luma
        samples (default: the configured size) and the chroma they cover; with cells=True
        (metrics, map), map the (N, MH, MW) int32 luma SAD of every 16x16 cell (its cells sum to
        the pair's luma "sad"). Any buffers in any order, repeats and a == b allowed;
        bufs_b=None gives the statistics of a alone ("sum_a", "sumsq_a"; "first" is -1). `out` is
        a contiguous int64 cuda tensor to write the N * 24 values into (else one is allocated).
        Runs in the order of torch's current stream (or on `stream`, a hipStream_t handle; see
        _enqueue_for_torch) and does not wait: order it after the frames' producer (sync(), or
        vp9hip_slot_stream_wait), as for convert. Needs torch imported before the library was
        loaded (see _torch_first)."""
        if not _torch_first:
            raise Vp9HipUnavailable("metrics: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        bufs_a = [int(b) for b in bufs_a]
        n = len(bufs_a)
        if bufs_b is not None:
            bufs_b = [int(b) for b in bufs_b]
            if len(bufs_b) != n:
                raise ValueError("metrics: bufs_a and bufs_b differ in length")
        w, h = (int(x) for x in size) if size is not None else (self.w, self.h)
        res, cmap = self._metrics_out(n, w, h, cells, out)
        aa = (ctypes.c_int * max(n, 1))(*bufs_a)
        ab = (ctypes.c_int * max(n, 1))(*bufs_b) if bufs_b is not None else None
        call = lambda st: lib().vp9hip_frame_metrics(self._c, aa, ab, n, w, h, res.data_ptr(),
                                                     cmap.data_ptr() if cells else None, st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check("vp9hip_frame_metrics", call(stream))
        else:
            _check("vp9hip_frame_metrics", _enqueue_for_torch(main.value, stream, call))
        return (res, cmap) if cells else res

    @staticmethod
    def _hist_out(n, C, B, out):
        """The (N, C, B) int32 destination of a histograms call; `out` is a contiguous int32 cuda
        tensor of at least N * C * B elements, or None."""
        import torch
        need = max(n, 0) * C * min(B, 4096)
        if out is None:
            out = torch.empty(max(need, 1), dtype=torch.int32, device="cuda")
        elif not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == torch.int32 and out.is_contiguous()
                  and out.numel() >= need):
            raise ValueError("histograms: out must be a contiguous int32 cuda tensor of at least %d elements" % need)
        return out.view(-1)[:need].view(max(n, 0), C, min(B, 4096))

    def histograms(self, bufs, what="planes", bins=256, colorspace=2, full_range=False, size=None, rects=None, out=None,
                   stream=None):
        """The histograms of the device buffers bufs on the GPU, one launch per 32 frames
        (vp9hip_frame_histograms, the definition in include/vp9hip.h "frame histograms"): an
        (N, C, B) int32 cuda tensor, channels Y, U, V (what="planes") or R, G, B, max(R, G, B) of
        the conversion's codes at the source's depth (what="rgbm", with colorspace / full_range
        as for convert) by B = `bins` bins, a power of two in 16 .. 2^bpp (one bin per code at
        2^bpp). Over the top-left `size` = (width, height) luma samples (default: the configured
        size), or over `rects`: one luma rectangle (x, y, w, h) inside it for every frame, or one
        per frame, x / y multiples of the chroma subsampling. Any buffers in any order, repeats
        allowed. `out` is a contiguous int32 cuda tensor to write the N * C * B counts into (else
        one is allocated). The scene-cut distance of consecutive frames is
        (h[1:] - h[:-1]).abs().sum((1, 2)); hist_percentile and light_levels read the tables.
        Runs in the order of torch's current stream (or on `stream`, a hipStream_t handle; see
        _enqueue_for_torch) and does not wait: order it after the frames' producer (sync(), or
        vp9hip_slot_stream_wait), as for convert. Needs torch imported before the library was
        loaded (see _torch_first)."""
        if not _torch_first:
            raise Vp9HipUnavailable("histograms: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        bufs = [int(b) for b in bufs]
        n = len(bufs)
        w, h = (int(x) for x in size) if size is not None else (self.w, self.h)
        d, C, B = _hist_desc("histograms", what, bins, colorspace, full_range, w, h, rects, n)
        res = self._hist_out(n, C, B, out)
        arr = (ctypes.c_int * max(n, 1))(*bufs)
        call = lambda st: lib().vp9hip_frame_histograms(self._c, arr, n, ctypes.byref(d), res.data_ptr(), st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check("vp9hip_frame_histograms", call(stream))
        else:
            _check("vp9hip_frame_histograms", _enqueue_for_torch(main.value, stream, call))
        return res

    def acc_warp(self, bufs, root_bufs, output="residual", interp="nearest", mask=False, size=None, out=None, stream=None):
        """The accumulated residual of the pairs (bufs[i], root_bufs[i]) of device buffers on the GPU
        (vp9hip_acc_warp, the definition in include/vp9hip.h "accumulated residual"): frame
        bufs[i] minus frame root_bufs[i] displaced by bufs[i]'s accumulated motion, wherever a
        cell's chain ended in the frame root_bufs[i] holds (elsewhere 0); output "picture" gives
        the displaced picture itself (elsewhere bufs[i]'s own samples). interp "nearest" or
        "bilinear". Returns (y, u, v), or (y, u, v, mask) with mask=True: int16 cuda views
        (N, H, W), (N, CH, CW), (N, CH, CW) of one allocation laid out by warp_layout, for
        "picture" the uint16 codes' bit pattern (codes of up to 12 bits are the values
        themselves); the mask uint8 (N, GH, GW), 1 where the cell applies. `size` = (width,
        height) is the visible size (default: the configured size); `out` a contiguous int16 cuda
        tensor to write into (else one is allocated). Needs set_export(motion_acc=True). Runs in
        the order of torch's current stream (or on `stream`, a hipStream_t handle; see
        _enqueue_for_torch) and does not wait: order it after the frames' producer (sync(), or
        vp9hip_slot_stream_wait), as for metrics. Needs torch imported before the library was
        loaded (see _torch_first)."""
        fn = "vp9hip_acc_warp"
        if not _torch_first:
            raise Vp9HipUnavailable("acc_warp: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        mode, outp = _warp_names(fn, output, interp)
        bufs, root_bufs = [int(b) for b in bufs], [int(b) for b in root_bufs]
        n = len(bufs)
        if len(root_bufs) != n:
            raise ValueError("acc_warp: bufs and root_bufs differ in length")
        w, h = (int(x) for x in size) if size is not None else (self.w, self.h)
        flat, views, m = _warp_out(n, w, h, getattr(self, "ss_h", 1), getattr(self, "ss_v", 1), mask, out)
        aa, ab = (ctypes.c_int * max(n, 1))(*bufs), (ctypes.c_int * max(n, 1))(*root_bufs)
        call = lambda st: lib().vp9hip_acc_warp(self._c, aa, ab, n, w, h, mode, outp, flat.data_ptr(),
                                                m.data_ptr() if mask else None, st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check(fn, call(stream))
        else:
            _check(fn, _enqueue_for_torch(main.value, stream, call))
        return views + (m,) if mask else views

    def acc_propagate(self, bufs, root_serials, src, interp="nearest", layout="nchw", fill=0, keep=False, valid=False,
                      src_index=None, size=None, out=None, stream=None):
        """A tensor of the root frame carried to the frames in bufs through their accumulated
        motion, on the GPU (vp9hip_acc_propagate, the definition in include/vp9hip.h "accumulated
        propagation"): item i of the result is source item src_index[i] displaced by bufs[i]'s
        accumulated field wherever a cell's chain ended in the frame of serial root_serials[i]
        (frame_motion_acc / download_motion_acc report a frame's serial; the root's pixels need
        not exist any more). src is a contiguous cuda tensor (M, C, FH, FW), (M, FH, FW, C) with
        layout "nhwc", or (M, FH, FW) (C = 1), on any feature grid FW x FH that covers the
        picture; uint8 / int8, int16 / float16 / bfloat16, int32 / float32 or int64 / float64.
        interp "nearest" copies elements bit for bit (label maps); "bilinear" needs float16.
        Elsewhere an element is `fill` (converted to src's dtype), or with keep=True what `out`
        held (keep needs out=). src_index=None reads item i when M == N and item 0 when M == 1.
        Returns the tensor, of src's dtype and layout with N items, or (tensor, valid) with
        valid=True: uint8 (N, FH, FW), 1 where the sample's cell applies. `size` = (width,
        height) is the visible size (default: the configured size). Needs
        set_export(motion_acc=True). Runs in the order of torch's current stream (or on `stream`,
        a hipStream_t handle; see _enqueue_for_torch) and does not wait, like acc_warp. Needs
        torch imported before the library was loaded (see _torch_first)."""
        fn = "vp9hip_acc_propagate"
        if not _torch_first:
            raise Vp9HipUnavailable("acc_propagate: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        bufs, root_serials = [int(b) for b in bufs], [int(x) & 0xffffffff for x in root_serials]
        n = len(bufs)
        if len(root_serials) != n:
            raise ValueError("acc_propagate: bufs and root_serials differ in length")
        d, m, idx, res, v = _prop_torch("acc_propagate", n, src, size if size is not None else (self.w, self.h), interp, layout,
                                        fill, keep, valid, src_index, out, fn)
        aa, ser = (ctypes.c_int * max(n, 1))(*bufs), (ctypes.c_uint32 * max(n, 1))(*root_serials)
        call = lambda st: lib().vp9hip_acc_propagate(self._c, aa, ser, idx, n, m, ctypes.byref(d), src.data_ptr(),
                                                     res.data_ptr(), v.data_ptr() if valid else None, st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check(fn, call(stream))
        else:
            _check(fn, _enqueue_for_torch(main.value, stream, call))
        return (res, v) if valid else res

    def acc_warp_tensors(self, bufs, root_bufs, fmt, resize=None, interp="nearest", coverage=False, colorspace=2,
                         full_range=False, size=None, out=None, stream=None, pitch=0, frame_stride=0):
        """The accumulated residual of the pairs (bufs[i], root_bufs[i]) as one (N, 3, OH, OW) cuda
        tensor at the model's size, made on the GPU in one launch per 32 pairs
        (vp9hip_acc_warp_scaled, the definition in include/vp9hip.h "accumulated residual at model
        size"): what acc_warp(output="residual") leaves, box-resampled to resize = (OW, OH) and
        formatted as residual_tensors does (fmt, colorspace, full_range, pitch, frame_stride as
        there), without the full-size planes in between; resize=None is the visible size through
        the same kernel. coverage=True adds a fourth plane: how much of each output sample's
        area lies in applying cells, 0..256 (int16) or 0..1 (float16). `size` = (width, height)
        is the visible size (default: the configured size). Needs set_export(motion_acc=True).
        Runs in the order of torch's current stream (or on `stream`) and does not wait, like
        residual_tensors. Needs torch imported before the library was loaded (see _torch_first)."""
        fn = "vp9hip_acc_warp_scaled"
        if not _torch_first:
            raise Vp9HipUnavailable("acc_warp_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        bufs, root_bufs = [int(b) for b in bufs], [int(b) for b in root_bufs]
        n = len(bufs)
        if len(root_bufs) != n:
            raise ValueError("acc_warp_tensors: bufs and root_bufs differ in length")
        d = _warpt_desc(fn, fmt, interp, coverage, resize, size if size is not None else (self.w, self.h), colorspace,
                        full_range, pitch, frame_stride)
        if resize is None and not (1 <= d.out_width <= 16384 and 1 <= d.out_height <= 16384):
            d.out_width = d.out_height = 1           # no size to default to: the library refuses the size itself
        flat, res = _warpt_out(n, d, out)
        aa, ab = (ctypes.c_int * max(n, 1))(*bufs), (ctypes.c_int * max(n, 1))(*root_bufs)
        call = lambda st: lib().vp9hip_acc_warp_scaled(self._c, aa, ab, n, ctypes.byref(d), flat.data_ptr(), st)
        main = ctypes.c_void_p()
        # an unconfigured context has no buffer to ask for its stream: the library refuses the call itself
        if lib().vp9hip_frame_device(self._c, 0, (ctypes.c_void_p * 3)(), (ctypes.c_ssize_t * 3)(), None, None,
                                     ctypes.byref(main)):
            _check(fn, call(stream))
        else:
            _check(fn, _enqueue_for_torch(main.value, stream, call))
        return res

    def upload(self, buf, planes):
        planes = [np.ascontiguousarray(p) for p in planes]
        ptrs, ls = self._plane_args(planes)
        _check("vp9hip_upload_frame", lib().vp9hip_upload_frame(self._c, buf, ptrs, ls))

    def flush(self):
        _check("vp9hip_flush", lib().vp9hip_flush(self._c))


class PacketDecoder:
    """send_packet / receive_frame over pass-1 frame packets (no bitstream parse).

    Reference slots are simplified: every decoded frame becomes LAST, GOLDEN and
    ALTREF of the next inter frame. Bitstreams go through Decoder.
    """

    def __init__(self, device=0, nbufs=4):
        self.dev = Device(device)
        self.nbufs = nbufs
        self._configured = None
        self._queue = []
        self._last = None
        self._next = 0

    def send_packet(self, frame):
        pkt = frame.pkt if hasattr(frame, "pkt") else frame
        cfg = (pkt.width, pkt.height, pkt.bpp)
        if self._configured != cfg:
            self.dev.configure(pkt.width, pkt.height, pkt.bpp, self.nbufs, pkt.ss_h, pkt.ss_v)
            self._configured = cfg
            self._last = None
        out = self._next
        self._next = (self._next + 1) % self.nbufs
        ref = self._last if self._last is not None else out
        self.dev.submit(pkt, out, (ref, ref, ref))
        self._last = out
        self._queue.append(out)

    def receive_frame(self):
        """Returns the next decoded frame as visible numpy planes, or None (EAGAIN)."""
        if not self._queue:
            return None
        buf = self._queue.pop(0)
        w, h, bpp = self._configured
        return visible(self.dev.download(buf), w, h)


class Decoder:
    """avcodec_send_packet / avcodec_receive_frame for AV_CODEC_ID_VP9 (vp9hip_decoder):
    compressed VP9 packets in, decoded frames out. The host parses each frame
    (vp9h_stream), the MI355X reconstructs them in batches of up to max_batch frames.

    send_packet(data, pts) -> None; raises Vp9HipError with code EAGAIN when frames must
    be received first. send_packet(None) drains. receive_frame() -> (planes, info) with
    visible numpy planes (download=True) or a device-buffer handle, None when more input
    is needed (EAGAIN) or after the drain (EOF, which also sets .eof).
    """

    def __init__(self, device=0, max_batch=16, extra_bufs=4, max_width=0, max_height=0, parse_threads=None,
                 export_motion=False, export_residual=False, export_motion_acc=False):
        self.params = DecoderParams()
        lib().vp9hip_decoder_defaults(ctypes.byref(self.params))
        self.params.device, self.params.max_batch, self.params.extra_bufs = device, max_batch, extra_bufs
        self.params.max_width, self.params.max_height = max_width, max_height
        if parse_threads is not None:
            self.params.parse_threads = parse_threads
        self._d = ctypes.c_void_p()
        _check("vp9hip_decoder_open", lib().vp9hip_decoder_open(ctypes.byref(self.params), ctypes.byref(self._d)))
        self.eof = False
        if export_motion or export_residual or export_motion_acc:   # accumulated motion turns motion on
            _check("vp9hip_decoder_set_export",
                   lib().vp9hip_decoder_set_export(self._d, (EXPORT_MOTION if export_motion or export_motion_acc else 0) |
                                                   (EXPORT_RESIDUAL if export_residual else 0) |
                                                   (EXPORT_MOTION_ACC if export_motion_acc else 0)))

    def close(self):
        if self._d:
            lib().vp9hip_decoder_close(self._d)
            self._d = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def send_packet(self, data, pts=0):
        if data is None:
            _check("vp9hip_decoder_send_packet", lib().vp9hip_decoder_send_packet(self._d, None, 0, 0))
            return
        data = bytes(data)
        _check("vp9hip_decoder_send_packet", lib().vp9hip_decoder_send_packet(self._d, data, len(data), pts))

    def receive_frame(self, download=True):
        """Next output frame: (visible planes, DecodedFrameInfo) with download=True, else
        (None, info) with info.buf valid until release(info.buf). None: EAGAIN / EOF."""
        info = DecodedFrameInfo()
        r = lib().vp9hip_decoder_receive_frame(self._d, ctypes.byref(info))
        if r == EAGAIN:
            return None
        if r == EOF:
            self.eof = True
            return None
        _check("vp9hip_decoder_receive_frame", r)
        if not download:
            return None, info
        planes = alloc_planes(info.width, info.height, info.bpp, info.ss_h, info.ss_v)
        ptrs = (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])
        ls = (ctypes.c_ssize_t * 3)(*[p.strides[0] for p in planes])
        try:
            _check("vp9hip_download_frame", lib().vp9hip_download_frame(self.context(), info.buf, ptrs, ls))
        finally:
            self.release(info.buf)
        return visible(planes, info.width, info.height, info.ss_h, info.ss_v), info

    def release(self, buf):
        _check("vp9hip_decoder_release", lib().vp9hip_decoder_release(self._d, buf))

    def context(self):
        return ctypes.c_void_p(lib().vp9hip_decoder_context(self._d))

    def motion(self, info, download=False, device=None):
        """The motion field of a frame of receive_frame(download=False), valid until
        release(info.buf) (vp9hip_decoder_frame_motion; needs export_motion=True): zero-copy
        torch views (mv, info) as Device.motion returns them, or numpy copies with
        download=True. A show_existing_frame output has the field of the frame it shows."""
        mv, inf = ctypes.c_void_p(), ctypes.c_void_p()
        gw, gh, pitch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _check("vp9hip_decoder_frame_motion",
               lib().vp9hip_decoder_frame_motion(self._d, ctypes.byref(info), ctypes.byref(mv), ctypes.byref(inf),
                                                 ctypes.byref(gw), ctypes.byref(gh), ctypes.byref(pitch)))
        if not download:
            return _motion_views(mv.value, inf.value, gw.value, gh.value, pitch.value, device)
        m, i = np.empty((gh.value, gw.value, 2, 2), np.int16), np.empty((gh.value, gw.value, 4), np.uint8)
        _check("vp9hip_download_motion", lib().vp9hip_download_motion(self.context(), info.buf, m.ctypes.data, i.ctypes.data))
        return m, i

    def motion_acc(self, info, download=False, device=None):
        """The accumulated motion field of a frame of receive_frame(download=False), valid until
        release(info.buf) (vp9hip_decoder_frame_motion_acc; needs export_motion_acc=True):
        (cells, serial) with cells the zero-copy torch int32 view Device.motion_acc returns, or
        a numpy ACC_CELL array with download=True. A show_existing_frame output has the field and
        serial of the frame it shows."""
        acc, ser = ctypes.c_void_p(), ctypes.c_uint32()
        gw, gh, pitch = ctypes.c_int(), ctypes.c_int(), ctypes.c_int64()
        _check("vp9hip_decoder_frame_motion_acc",
               lib().vp9hip_decoder_frame_motion_acc(self._d, ctypes.byref(info), ctypes.byref(acc), ctypes.byref(gw),
                                                     ctypes.byref(gh), ctypes.byref(pitch), ctypes.byref(ser)))
        if not download:
            return _acc_view(acc.value, gw.value, gh.value, pitch.value, device), ser.value
        cells = np.empty((gh.value, gw.value), ACC_CELL)
        _check("vp9hip_download_motion_acc",
               lib().vp9hip_download_motion_acc(self.context(), info.buf, cells.ctypes.data, None))
        return cells, ser.value

    def residual(self, info, download=False, device=None):
        """The residual field of a frame of receive_frame(download=False), valid until
        release(info.buf) (vp9hip_decoder_frame_residual; needs export_residual=True): zero-copy
        torch int16 views (Y, U, V) of the visible size as Device.residual returns them, or numpy
        copies of the coded area with download=True. A show_existing_frame output has the field
        of the frame it shows."""
        ptrs, pitch = (ctypes.c_void_p * 3)(), (ctypes.c_int64 * 3)()
        _check("vp9hip_decoder_frame_residual",
               lib().vp9hip_decoder_frame_residual(self._d, ctypes.byref(info), ctypes.byref(ptrs), ctypes.byref(pitch)))
        if not download:
            return _residual_views(list(ptrs), list(pitch), info.width, info.height, info.ss_h, info.ss_v, device)
        planes = [np.empty(s, np.int16) for s in residual_shapes(info.width, info.height, info.ss_h, info.ss_v)]
        hp, ls = _plane_ptrs(planes)
        _check("vp9hip_download_residual",
               lib().vp9hip_download_residual(self.context(), info.buf, ctypes.byref(hp), ctypes.byref(ls)))
        return planes

    def residual_tensors(self, infos, fmt, resize=None, out=None):
        """The residual fields of frames of receive_frame(download=False) (their
        DecodedFrameInfos, all of one size, depth, subsampling, colour space and range, all still
        held) as Device.residual_tensors returns them, with the frames' own colour description
        (vp9hip_decoder_residual_scaled; needs export_residual=True), on torch's current stream;
        waits for it. Unlike Decoder.convert it releases nothing: the pixels and the motion of
        the same frames are usually wanted too."""
        fn = "vp9hip_decoder_residual_scaled"
        if not _torch_first:
            raise Vp9HipUnavailable("residual_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos = list(infos)
        if not infos:
            raise Vp9HipError(fn, EINVAL)
        f = infos[0]
        d = _resid_desc(fn, fmt, resize, (f.width, f.height), -1, 0, 0, 0)
        flat, res = _resid_out(len(infos), d, out)
        arr = (DecodedFrameInfo * len(infos))(*infos)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_residual_scaled(self._d, arr, len(infos), ctypes.byref(d), flat.data_ptr(), st)
        _check(fn, _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return res

    def motion_tensors(self, infos, fmt, resize=None, source="coded", mask=False, out=None):
        """The motion fields (source "coded"; needs export_motion=True) or accumulated motion
        fields (source "acc"; needs export_motion_acc=True) of frames of
        receive_frame(download=False) (their DecodedFrameInfos, all of one size, all still held)
        as Device.motion_tensors returns them, at the frames' own visible size
        (vp9hip_decoder_motion_scaled), on torch's current stream; waits for it. A
        show_existing_frame output has the tensor of the frame it shows. Like
        Decoder.residual_tensors it releases nothing."""
        fn = "vp9hip_decoder_motion_scaled"
        if not _torch_first:
            raise Vp9HipUnavailable("motion_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos = list(infos)
        if not infos:
            raise Vp9HipError(fn, EINVAL)
        f = infos[0]
        d = _mvt_desc(fmt, source, mask, resize, (f.width, f.height), 0, 0)
        flat, res = _mvt_out(len(infos), d, out)
        arr = (DecodedFrameInfo * len(infos))(*infos)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_motion_scaled(self._d, arr, len(infos), ctypes.byref(d), flat.data_ptr(), st)
        _check(fn, _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return res

    def grade(self, fmt, in_lut=None, m=None, out_lut=None, bpp=None):
        """A Grade for convert(grade=...) with its tables in the decoder's device memory, as
        Device.grade: grade(g) of a host Grade, or grade(fmt, in_lut, m, out_lut, bpp=...)."""
        g = fmt if isinstance(fmt, Grade) else Grade(bpp, fmt, in_lut, m, out_lut)
        return g._on(self.context())

    def convert(self, infos, fmt, out=None, resize=None, filter="box", src_rects=None, dst_rects=None, fill=None, grade=None):
        """Convert the frames of receive_frame(download=False) (their DecodedFrameInfos, all of
        one size, colour space and range) to `fmt` as Device.convert does, with the frames' own
        colour description (vp9hip_decoder_convert; with resize=(OW, OH)
        vp9hip_decoder_convert_scaled; with filter / src_rects / dst_rects / fill as well, which
        mean what they mean there, vp9hip_decoder_convert_resampled, or vp9hip_decoder_convert_bicubic for
        filter="bicubic"; with grade, what Decoder.grade returns, vp9hip_decoder_convert_graded for
        any of them), on torch's current stream; waits for it and releases
        the buffers. Returns the tensor(s)."""
        if not _torch_first:
            raise Vp9HipUnavailable("convert: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos = list(infos)
        f = infos[0] if infos else DecodedFrameInfo()
        cs = 2 if f.colorspace in (0, 6) else f.colorspace
        rs = _resample_arg(len(infos), resize, filter, src_rects, dst_rects, fill, f.bpp or 8, cs, f.full_range)
        if grade is not None:
            gh = _grade_handle(grade, fmt)
            if rs is None:
                rs = Resample(FILTERS["box"], *(int(x) for x in (resize if resize is not None else (f.width, f.height))))
        fn = ("vp9hip_decoder_convert_graded" if grade is not None else
              "vp9hip_decoder_convert" if resize is None else
              "vp9hip_decoder_convert_scaled" if rs is None else
              "vp9hip_decoder_convert_bicubic" if rs.filter == FILTER_BICUBIC else "vp9hip_decoder_convert_resampled")
        if not infos:
            raise Vp9HipError(fn, EINVAL)
        arr = (DecodedFrameInfo * len(infos))(*infos)
        ow, oh = (f.width, f.height) if resize is None else Device._resize_arg(fn, resize)
        flat, res, pitch, stride = Device._convert_out(len(infos), fmt, ow, oh, f.bpp, f.ss_h, f.ss_v, out, 0, 0)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        if grade is not None:
            call = lambda st: lib().vp9hip_decoder_convert_graded(self._d, arr, len(infos), OUT_FORMATS[fmt], ctypes.byref(rs), gh,
                                                                  flat.data_ptr(), 0, 0, st)
        elif rs is not None:
            call = lambda st: getattr(lib(), fn)(self._d, arr, len(infos), OUT_FORMATS[fmt], ctypes.byref(rs),
                                                 flat.data_ptr(), 0, 0, st)
        elif resize is None:
            call = lambda st: lib().vp9hip_decoder_convert(self._d, arr, len(infos), OUT_FORMATS[fmt], flat.data_ptr(), 0, 0, st)
        else:
            call = lambda st: lib().vp9hip_decoder_convert_scaled(self._d, arr, len(infos), OUT_FORMATS[fmt], ow, oh,
                                                                  flat.data_ptr(), 0, 0, st)
        _check(fn, _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        for i in infos:
            self.release(i.buf)
        return res

    def metrics(self, infos_a, infos_b=None, cells=False):
        """The exact frame metrics of the pairs (infos_a[i], infos_b[i]) of frames of
        receive_frame(download=False) (their DecodedFrameInfos, all of one size, depth and
        subsampling, all still held), as Device.metrics returns them: an (N, 3, 8) int64 cuda
        tensor, or (metrics, map) with cells=True (vp9hip_decoder_metrics). infos_b=None gives
        the statistics of the frames alone. Runs on torch's current stream and waits for it.
        Unlike Decoder.convert it releases nothing: the scene-cut use, metrics(infos[1:],
        infos[:-1]), needs every frame twice, so the caller releases the buffers when it is done
        with them."""
        if not _torch_first:
            raise Vp9HipUnavailable("metrics: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos_a = list(infos_a)
        n = len(infos_a)
        if infos_b is not None:
            infos_b = list(infos_b)
            if len(infos_b) != n:
                raise ValueError("metrics: infos_a and infos_b differ in length")
        if not n:
            raise Vp9HipError("vp9hip_decoder_metrics", EINVAL)
        f = infos_a[0]
        res, cmap = Device._metrics_out(n, f.width, f.height, cells, None)
        aa = (DecodedFrameInfo * n)(*infos_a)
        ab = (DecodedFrameInfo * n)(*infos_b) if infos_b is not None else None
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_metrics(self._d, aa, ab, n, res.data_ptr(),
                                                       cmap.data_ptr() if cells else None, st)
        _check("vp9hip_decoder_metrics", _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return (res, cmap) if cells else res

    def histograms(self, infos, what="planes", bins=256, rects=None, out=None):
        """The histograms of frames of receive_frame(download=False) (their DecodedFrameInfos, all
        of one size, depth, subsampling and, for what="rgbm", colour space and range, all still
        held), as Device.histograms returns them (vp9hip_decoder_histograms): over the frames' own
        size, or `rects` inside it, with the frames' own colour space and range (unknown: BT.709).
        Runs on torch's current stream and waits for it; like metrics it releases nothing."""
        if not _torch_first:
            raise Vp9HipUnavailable("histograms: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos = list(infos)
        n = len(infos)
        if not n:
            raise Vp9HipError("vp9hip_decoder_histograms", EINVAL)
        f = infos[0]
        d, C, B = _hist_desc("histograms", what, bins, -1, False, f.width, f.height, rects, n)
        res = Device._hist_out(n, C, B, out)
        arr = (DecodedFrameInfo * n)(*infos)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_histograms(self._d, arr, n, ctypes.byref(d), res.data_ptr(), st)
        _check("vp9hip_decoder_histograms", _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return res

    def acc_warp(self, infos, root_infos, output="residual", interp="nearest", mask=False):
        """The accumulated residual of the pairs (infos[i], root_infos[i]) of frames of
        receive_frame(download=False) (all of one size, depth and subsampling, all still held;
        needs export_motion_acc=True), as Device.acc_warp returns it (vp9hip_decoder_acc_warp):
        keep the key frame un-released and pass it as every root. Runs on torch's current stream
        and waits for it; like metrics it releases nothing."""
        fn = "vp9hip_decoder_acc_warp"
        if not _torch_first:
            raise Vp9HipUnavailable("acc_warp: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        mode, outp = _warp_names(fn, output, interp)
        infos, root_infos = list(infos), list(root_infos)
        n = len(infos)
        if len(root_infos) != n:
            raise ValueError("acc_warp: infos and root_infos differ in length")
        if not n:
            raise Vp9HipError(fn, EINVAL)
        f = infos[0]
        flat, views, m = _warp_out(n, f.width, f.height, f.ss_h, f.ss_v, mask, None)
        aa, ab = (DecodedFrameInfo * n)(*infos), (DecodedFrameInfo * n)(*root_infos)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_acc_warp(self._d, aa, ab, n, mode, outp, flat.data_ptr(),
                                                        m.data_ptr() if mask else None, st)
        _check(fn, _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return views + (m,) if mask else views

    def acc_propagate(self, infos, root_serials, src, interp="nearest", layout="nchw", fill=0, keep=False, valid=False,
                      src_index=None, out=None):
        """A tensor of the root frame carried to the frames infos of receive_frame(download=False)
        (all of one size, all still held; needs export_motion_acc=True), as Device.acc_propagate
        returns it (vp9hip_decoder_acc_propagate): take the key frame's serial from
        motion_acc(info)[1], run the model on it, release it, and pass the serial as every root.
        Runs on torch's current stream and waits for it; like acc_warp it releases nothing."""
        fn = "vp9hip_decoder_acc_propagate"
        if not _torch_first:
            raise Vp9HipUnavailable("acc_propagate: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos, root_serials = list(infos), [int(x) & 0xffffffff for x in root_serials]
        n = len(infos)
        if len(root_serials) != n:
            raise ValueError("acc_propagate: infos and root_serials differ in length")
        if not n:
            raise Vp9HipError(fn, EINVAL)
        f = infos[0]
        d, m, idx, res, v = _prop_torch("acc_propagate", n, src, (f.width, f.height), interp, layout, fill, keep, valid,
                                        src_index, out, fn)
        aa, ser = (DecodedFrameInfo * n)(*infos), (ctypes.c_uint32 * n)(*root_serials)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_acc_propagate(self._d, aa, ser, idx, n, m, ctypes.byref(d), src.data_ptr(),
                                                             res.data_ptr(), v.data_ptr() if valid else None, st)
        _check(fn, _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return (res, v) if valid else res

    def acc_warp_tensors(self, infos, root_infos, fmt, resize=None, interp="nearest", coverage=False, out=None):
        """The accumulated residual at model size of the pairs (infos[i], root_infos[i]) of frames
        of receive_frame(download=False) (all of one size, depth and subsampling, all still held;
        the infos of one colour space and range, which are the ones used; needs
        export_motion_acc=True), as Device.acc_warp_tensors returns it
        (vp9hip_decoder_acc_warp_scaled). Runs on torch's current stream and waits for it; like
        acc_warp it releases nothing."""
        fn = "vp9hip_decoder_acc_warp_scaled"
        if not _torch_first:
            raise Vp9HipUnavailable("acc_warp_tensors: import torch before ffmpeg-hybrid_amd loads libvp9hip.so "
                                    "(both use libamdhip64; torch's device init needs its own runtime loaded first)")
        import torch
        infos, root_infos = list(infos), list(root_infos)
        n = len(infos)
        if len(root_infos) != n:
            raise ValueError("acc_warp_tensors: infos and root_infos differ in length")
        if not n:
            raise Vp9HipError(fn, EINVAL)
        f = infos[0]
        d = _warpt_desc(fn, fmt, interp, coverage, resize, (f.width, f.height), 2, 0, 0, 0)
        flat, res = _warpt_out(n, d, out)
        aa, ab = (DecodedFrameInfo * n)(*infos), (DecodedFrameInfo * n)(*root_infos)
        main = ctypes.c_void_p()
        _check("vp9hip_frame_device", lib().vp9hip_frame_device(self.context(), 0, (ctypes.c_void_p * 3)(),
                                                                (ctypes.c_ssize_t * 3)(), None, None, ctypes.byref(main)))
        call = lambda st: lib().vp9hip_decoder_acc_warp_scaled(self._d, aa, ab, n, ctypes.byref(d), flat.data_ptr(), st)
        _check(fn, _enqueue_for_torch(main.value, None, call))
        torch.cuda.current_stream().synchronize()
        return res

    def flush(self):
        _check("vp9hip_decoder_flush", lib().vp9hip_decoder_flush(self._d))
        self.eof = False

    def decode(self, packets, download=True):
        """Decode an iterable of (data, pts) or data: yields receive_frame results in
        output order, draining at the end (the ffmpeg -i ... -f null - loop)."""
        for item in packets:
            data, pts = item if isinstance(item, tuple) else (item, 0)
            while True:
                try:
                    self.send_packet(data, pts)
                    break
                except Vp9HipError as e:
                    if e.code != EAGAIN:
                        raise
                    got = self.receive_frame(download)
                    if got is None:
                        raise
                    yield got
            while True:
                got = self.receive_frame(download)
                if got is None:
                    break
                yield got
        self.send_packet(None)
        while True:
            got = self.receive_frame(download)
            if got is None:
                break
            yield got


def frame_peek(data):
    """(type, FrameInfo) from the start of the uncompressed header (vp9h_frame_peek): type 0
    keyframe, 1 inter, 2 show_existing_frame, 3 intra-only; slot bookkeeping without state."""
    data = bytes(data)
    info = FrameInfo()
    t = _check("vp9h_frame_peek", lib().vp9h_frame_peek(data, len(data), ctypes.byref(info)))
    return t, info


def vp9h_type(data):
    """Frame type from the header's first bits (vp9h_frame_type): 0 key, 1 other, 2
    show_existing_frame, or a negative AVERROR."""
    data = bytes(data)
    return lib().vp9h_frame_type(data, len(data))


# ---- IVF (libavformat/ivfdec.c, ivfenc.c) -------------------------------------------
def ivf_probe(data):
    data = bytes(data[:32])
    return lib().vp9h_ivf_probe(data, len(data))


def ivf_read(data):
    """IVF bytes -> (IvfHeader, [(pts, frame bytes)]). A short last frame is returned
    as far as it goes (av_get_packet)."""
    data = bytes(data)
    h = IvfHeader()
    _check("vp9h_ivf_read_header", lib().vp9h_ivf_read_header(data, len(data), ctypes.byref(h)))
    frames = []
    pos = ctypes.c_size_t(32)
    ptr, n, pts, tr = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_int64(), ctypes.c_int()
    base = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value
    while True:
        r = lib().vp9h_ivf_read_frame(data, len(data), ctypes.byref(pos), ctypes.byref(ptr), ctypes.byref(n),
                                      ctypes.byref(pts), ctypes.byref(tr))
        if r == EOF:
            break
        _check("vp9h_ivf_read_frame", r)
        off = ptr.value - base
        frames.append((pts.value, data[off:off + n.value]))
    return h, frames


def ivf_write(frames, width, height, time_base=(1, 30)):
    """[(pts, bytes)] or [bytes] -> IVF bytes (fourcc VP90, frame count filled in)."""
    hdr = ctypes.create_string_buffer(32)
    _check("vp9h_ivf_write_header", lib().vp9h_ivf_write_header(hdr, width, height, time_base[1], time_base[0],
                                                                 len(frames)))
    out = [hdr.raw]
    fh = ctypes.create_string_buffer(12)
    for i, f in enumerate(frames):
        pts, data = f if isinstance(f, tuple) else (i, f)
        lib().vp9h_ivf_write_frame_header(fh, len(data), pts)
        out += [fh.raw, bytes(data)]
    return b"".join(out)


NOPTS = -(1 << 63)


def webm_probe(data):
    data = bytes(data)
    return lib().vp9h_webm_probe(data, len(data))


def webm_read(data):
    """WebM / Matroska bytes -> (WebmInfo, [(pts, frame bytes, keyframe)]) of the first VP9
    video track (vp9h_webm_read_header / _read_frame; pts in TimecodeScale units, NOPTS
    for later laces of a block without a duration)."""
    data = bytes(data)
    info, cur = WebmInfo(), WebmCursor()
    _check("vp9h_webm_read_header", lib().vp9h_webm_read_header(data, len(data), ctypes.byref(info), ctypes.byref(cur)))
    frames = []
    ptr, n, pts, key = ctypes.c_void_p(), ctypes.c_uint32(), ctypes.c_int64(), ctypes.c_int()
    base = ctypes.cast(ctypes.c_char_p(data), ctypes.c_void_p).value
    while True:
        r = lib().vp9h_webm_read_frame(data, len(data), ctypes.byref(cur), ctypes.byref(ptr), ctypes.byref(n),
                                       ctypes.byref(pts), ctypes.byref(key))
        if r == EOF:
            break
        _check("vp9h_webm_read_frame", r)
        off = ptr.value - base
        frames.append((pts.value, data[off:off + n.value], key.value))
    return info, frames


# ---- a small WebM muxer (matroskaenc.c's element layout) for tests and tools: not the product
def _ebml_id(i):
    return i.to_bytes((i.bit_length() + 7) // 8, "big")


def _ebml_size(n, width=None, unknown=False):
    if unknown:
        w = width or 8
        return bytes([0xFF >> (w - 1) | (0x80 >> (w - 1))] + [0xFF] * (w - 1)) if w > 1 else b"\xff"
    w = width or next(k for k in range(1, 9) if n < (1 << (7 * k)) - 1)
    return (n | (1 << (7 * w))).to_bytes(w, "big")


def _el(i, payload, unknown=False, width=None):
    return _ebml_id(i) + _ebml_size(len(payload), width, unknown) + payload


def _uint(i, v):
    return _el(i, v.to_bytes(max(1, (v.bit_length() + 7) // 8), "big"))


WEBM_COLOUR_IDS = {"matrix": 0x55B1, "bits_per_channel": 0x55B2, "range": 0x55B9, "transfer": 0x55BA, "primaries": 0x55BB,
                   "max_cll": 0x55BC, "max_fall": 0x55BD}


def webm_colour(data):
    """The Colour element of the first VP9 video track as a dict (vp9h_webm_read_colour):
    present, matrix, bits_per_channel, range, transfer, primaries, max_cll, max_fall,
    luminance_max, luminance_min; absent fields are 2 ("unspecified") or 0."""
    data = bytes(data)
    c = WebmColour()
    _check("vp9h_webm_read_colour", lib().vp9h_webm_read_colour(data, len(data), ctypes.byref(c)))
    return {k: getattr(c, k) for k, _ in WebmColour._fields_}


def _webm_colour_element(colour):
    """The Colour element (0x55B0) of webm_colour's keys; luminance_* as 8-byte floats."""
    import struct
    body = b"".join(_uint(i, int(colour[k])) for k, i in WEBM_COLOUR_IDS.items() if k in colour)
    mm = b"".join(_el(i, struct.pack(">d", float(colour[k]))) for k, i in (("luminance_max", 0x55D9), ("luminance_min", 0x55DA))
                  if k in colour)
    return _el(0x55B0, body + (_el(0x55D0, mm) if mm else b""))


def webm_write(frames, width, height, timecode_scale=1000000, cluster_frames=8, lacing=None,
               unknown_sizes=False, block_groups=False, other_track=False, voids=False, colour=None):
    """[(pts, bytes)] or [bytes] -> WebM bytes with one V_VP9 track (number 1). Options for
    tests: lacing = "xiph" / "fixed" / "ebml" (frames laced in pairs), unknown-size Segment
    and Clusters, BlockGroup + Block instead of SimpleBlock, an interleaved second track's
    blocks, Void elements. colour: a dict of webm_colour's keys, written as the video track's
    Colour element (None: no element)."""
    fr = [f if isinstance(f, tuple) else (i, f) for i, f in enumerate(frames)]
    hdr = _el(0x1A45DFA3, _uint(0x4286, 1) + _uint(0x42F7, 1) + _uint(0x42F2, 4) + _uint(0x42F3, 8) +
              _el(0x4282, b"webm") + _uint(0x4287, 4) + _uint(0x4285, 2))
    info = _el(0x1549A966, _uint(0x2AD7B1, timecode_scale) + _el(0x4D80, b"vp9hip"))
    video = _el(0xE0, _uint(0xB0, width) + _uint(0xBA, height) + (_webm_colour_element(colour) if colour is not None else b""))
    tracks = [_el(0xAE, _uint(0xD7, 1) + _uint(0x73C5, 1) + _uint(0x83, 1) + _el(0x86, b"V_VP9") + video)]
    if other_track:
        tracks.append(_el(0xAE, _uint(0xD7, 2) + _uint(0x73C5, 2) + _uint(0x83, 2) + _el(0x86, b"A_OPUS")))
    body = [info, _el(0x1654AE6B, b"".join(tracks))]
    if voids:
        body.insert(1, _el(0xEC, b"\0" * 5))

    def block(track, rel, flags, payloads, kind):
        head = bytes([0x80 | track]) + (rel & 0xFFFF).to_bytes(2, "big")
        if kind is None:
            return head + bytes([flags]) + payloads[0]
        n = len(payloads)
        if kind == "xiph":
            lace = bytes([n - 1]) + b"".join(b"\xff" * (len(p) // 255) + bytes([len(p) % 255]) for p in payloads[:-1])
            return head + bytes([flags | 0x02]) + lace + b"".join(payloads)
        if kind == "fixed":
            return head + bytes([flags | 0x04]) + bytes([n - 1]) + b"".join(payloads)
        sizes = _ebml_size(len(payloads[0]))                        # EBML lacing: size, then signed deltas
        for a, b in zip(payloads, payloads[1:-1]):
            d = len(b) - len(a)
            w = next(k for k in range(1, 9) if abs(d) < (1 << (7 * k - 1)) - 1)
            sizes += (d + (1 << (7 * w - 1)) - 1 | (1 << (7 * w))).to_bytes(w, "big")
        return head + bytes([flags | 0x06]) + bytes([n - 1]) + sizes + b"".join(payloads)

    for c0 in range(0, len(fr), cluster_frames):
        grp = fr[c0:c0 + cluster_frames]
        tc = grp[0][0]
        parts = [_uint(0xE7, tc)]
        k = 0
        while k < len(grp):
            n = 2 if lacing and k + 1 < len(grp) and (lacing != "fixed" or len(grp[k][1]) == len(grp[k + 1][1])) else 1
            pays = [d for _, d in grp[k:k + n]]
            rel = grp[k][0] - tc
            if block_groups:
                parts.append(_el(0xA0, _el(0xA1, block(1, rel, 0, pays, lacing if n > 1 else None)) +
                                 (_uint(0x9B, n * (grp[1][0] - grp[0][0] if len(grp) > 1 else 1)) if n > 1 else b"")))
            else:
                parts.append(_el(0xA3, block(1, rel, 0x80 if k == 0 and c0 == 0 else 0, pays, lacing if n > 1 else None)))
            if other_track:
                parts.append(_el(0xA3, block(2, rel, 0x80, [b"\x01\x02\x03"], None)))
            if voids and k == 0:
                parts.append(_el(0xEC, b"\0\0"))
            k += n
        payload = b"".join(parts)
        body.append(_el(0x1F43B675, payload, unknown=unknown_sizes))
    body.append(_el(0x1C53BB6B, _el(0xBB, _uint(0xB3, 0))))        # a Cues element after the clusters
    return hdr + _el(0x18538067, b"".join(body), unknown=unknown_sizes)


PLAN_STAT_NAMES = ("sbs", "passes", "pjobs", "rjobs", "jobs_4x4", "jobs_8x8", "jobs_16x16",
                   "jobs_32x32", "lane_use", "max_passes_sb", "lf_records", "mc_units", "pred_steps",
                   "lf_steps", "levels", "pass_rows", "level_steps", "asap_passes", "firstfit_passes", "firstfit_height_passes",
                   "mc_out_bytes", "mc_alg_bytes", "mc_line_bytes")


def plan_sb_costs(frame):
    """Per SB of one packet (raster order) the pixel rows its intra passes loop over, as staged
    for the device (vp9hip_plan_sb_costs; host only, tools/wave_tail.py)."""
    n = ((frame.pkt.width + 63) >> 6) * ((frame.pkt.height + 63) >> 6)
    out = (ctypes.c_double * n)()
    got = _check("vp9hip_plan_sb_costs", lib().vp9hip_plan_sb_costs(ctypes.byref(frame.pkt), out, n))
    return np.array(out[:got])


def plan_stats(frame):
    """Host-only work-planning statistics of one pass-1 packet (vp9hip_plan_stats)."""
    out = (ctypes.c_double * len(PLAN_STAT_NAMES))()
    _check("vp9hip_plan_stats", lib().vp9hip_plan_stats(ctypes.byref(frame.pkt), out, len(PLAN_STAT_NAMES)))
    return dict(zip(PLAN_STAT_NAMES, list(out)))
