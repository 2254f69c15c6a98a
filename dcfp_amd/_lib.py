"""ctypes binding of libdcfp_hip.so (the C-ABI declared in include/dcfp_hip.h).

The library is the only compute path of this package: there is no CPU or eager-PyTorch
fallback.  `lib()` raises if the shared object is missing; every wrapper raises
RuntimeError on a non-zero status (<0 descriptor error, >0 hipError_t).
"""
import ctypes as C
import os
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("DCFP_LIB") or os.path.join(_HERE, "libdcfp_hip.so")   # DCFP_LIB: A/B builds
CSRC = os.path.join(_HERE, "csrc")

_lib = None
_lock = threading.Lock()


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("N", "Cin", "H", "W", "Cout", "KH", "KW", "stride", "pad", "dil", "Hout", "Wout",
                 "x_pitch", "dy_pitch")]


class ConvF16Desc(C.Structure):
    """DcfpConvF16Desc: one conv of the fp16 deployment engine (NHWC fp16, packed weights)."""
    _fields_ = [(n, C.c_int32) for n in
                ("N", "H", "W", "Cin8", "x_pitch", "Cout", "K", "stride", "pad", "dil", "Hout", "Wout",
                 "y_pitch", "y_off", "res_pitch", "res_off", "relu")]


class ConvF8Desc(C.Structure):
    """DcfpConvF8Desc: one conv of the fp8 deployment engine (NHWC e4m3, packed weights)."""
    _fields_ = [(n, C.c_int32) for n in
                ("N", "H", "W", "Cin16", "x_pitch", "Cout", "K", "stride", "pad", "dil", "Hout", "Wout",
                 "y_pitch", "y_off", "res_pitch", "res_off", "relu")] + [("res_mul", C.c_float)]


class EicEntry(C.Structure):
    _fields_ = [("gamma", C.c_void_p), ("grad", C.c_void_p), ("eic", C.c_void_p),
                ("n", C.c_int32), ("pad_", C.c_int32)]


class SgdEntry(C.Structure):
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("momentum_buf", C.c_void_p),
                ("n", C.c_int64), ("first_chunk", C.c_int64),
                ("weight_decay", C.c_float), ("pad_", C.c_int32)]


class GateEntry(C.Structure):
    """DcfpGateEntry: one scored BatchNorm layer of the gate kernels (Taylor score, slimming L1 term)."""
    _fields_ = [("gamma", C.c_void_p), ("beta", C.c_void_p), ("ggrad", C.c_void_p), ("bgrad", C.c_void_p),
                ("score", C.c_void_p), ("n", C.c_int32), ("pad_", C.c_int32)]


class FilterEntry(C.Structure):
    """DcfpFilterEntry: one matrix of `rows` rows of K contiguous floats of a filter_reduce launch."""
    _fields_ = [("w", C.c_void_p), ("g", C.c_void_p), ("out", C.c_void_p), ("rows", C.c_int32), ("K", C.c_int32),
                ("first_unit", C.c_int64)]


class FpgmEntry(C.Structure):
    """DcfpFpgmEntry: one matrix [C, K] of an fpgm call."""
    _fields_ = [("w", C.c_void_p), ("out", C.c_void_p), ("C", C.c_int32), ("K", C.c_int32),
                ("first_tile", C.c_int64), ("ws_off", C.c_int64)]


class AdamEntry(C.Structure):
    """DcfpAdamEntry: one tensor of a multi-tensor AdamW launch."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_int64), ("first_chunk", C.c_int64)]


class NormEntry(C.Structure):
    """DcfpNormEntry: one gradient tensor of a dcfp_grad_norm_f32 call."""
    _fields_ = [("data", C.c_void_p), ("n", C.c_int64), ("first_chunk", C.c_int64)]


class GradNorm(C.Structure):
    """DcfpGradNorm: what dcfp_grad_norm_f32 leaves on the device."""
    _fields_ = [("sqnorm", C.c_double), ("norm", C.c_float), ("coef", C.c_float)]


class SgdExEntry(C.Structure):
    """DcfpSgdExEntry: DcfpSgdEntry plus the (nullable) EMA pointer."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("momentum_buf", C.c_void_p), ("ema", C.c_void_p),
                ("n", C.c_int64), ("first_chunk", C.c_int64), ("weight_decay", C.c_float), ("pad_", C.c_int32)]


class AdamExEntry(C.Structure):
    """DcfpAdamExEntry: DcfpAdamEntry plus the (nullable) EMA pointer."""
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("ema", C.c_void_p), ("n", C.c_int64), ("first_chunk", C.c_int64)]


class BnRunning(C.Structure):
    """DcfpBnRunning: nn.BatchNorm2d's training-mode bookkeeping folded into the statistics kernels."""
    _fields_ = [("running_mean", C.c_void_p), ("running_var", C.c_void_p), ("num_batches_tracked", C.c_void_p),
                ("momentum", C.c_float), ("pad_", C.c_int32)]


class WpEntry(C.Structure):
    """DcfpWpEntry: one weight tensor -> permuted copy of the multi-tensor refresh."""
    _fields_ = [("w", C.c_void_p), ("wp", C.c_void_p), ("first_block", C.c_int64), ("n_blocks", C.c_int64)] + \
               [(n, C.c_int32) for n in ("T", "Ck", "CkP", "M", "Mpad", "sAm", "sAc", "perm8")]


class AugTap(C.Structure):
    """DcfpAugTap: one column or row of the augmentation's geometry tables."""
    _fields_ = [(n, C.c_int32) for n in ("src", "c0", "c1", "lsrc")]


class AugSample(C.Structure):
    """DcfpAugSample: one sample of an augmentation launch (host record, device pointers)."""
    _fields_ = [("image", C.c_void_p), ("label", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("src_h", "src_w", "col_off", "row_off", "lut_a_off", "lut_b_off",
                                         "hsv_flags", "hue_delta")] + \
               [("sat_alpha", C.c_float), ("pad_", C.c_int32)]


class CcSample(C.Structure):
    """DcfpCcSample: one sample of a connected-components launch (host record, device pointer)."""
    _fields_ = [("label", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("src_h", "src_w", "dst_h", "dst_w", "Hp", "Wp", "row_off", "col_off", "cls",
                                         "pad_")] + \
               [("work_off", C.c_int64)]


class VoteMap(C.Structure):
    """DcfpVoteMap: the low-resolution logits of one (scale, flip) pass of a vote launch (host record, device pointer)."""
    _fields_ = [("logits", C.c_void_p)] + [(n, C.c_int32) for n in ("h", "w", "hs", "ws", "flip")] + \
               [("weight", C.c_float)]


class SlidePass(C.Structure):
    """DcfpSlidePass: the low-resolution logits of the tiles of one (scale, flip) pass of a sliding-window vote."""
    _fields_ = [("logits", C.c_void_p)] + \
               [(n, C.c_int32) for n in ("lh", "lw", "hs", "ws", "th", "tw", "rows", "cols", "flip")] + \
               [("weight", C.c_float)]


class EngineInfo(C.Structure):
    """dcfp_engine_info_t: what a flat engine file says about itself."""
    _fields_ = [(n, C.c_int32) for n in ("format", "num_classes", "in_channels", "align_corner", "model", "n_records",
                                         "n_buffers", "n_slots", "has_input_table")]


SLIDE_MAX_PASSES, SLIDE_MAX_TILES_PER_AXIS = 16, 32    # DCFP_SLIDE_MAX_* of include/dcfp_hip.h
AUG_SATURATION, AUG_HUE = 1, 2
SGD_CHUNK = 16384
FILTER_ABS_SUM, FILTER_L2, FILTER_DOT_SQ_ACC = 0, 1, 2    # DCFP_FILTER_* of include/dcfp_hip.h
FPGM_TILE = 64                                            # DCFP_FPGM_TILE
DIGEST_CHUNK, DIGEST_MAX_BLOCKS = 4096, 2048              # DCFP_DIGEST_*
CONV_FWD, CONV_DGRAD, CONV_WGRAD = 0, 1, 2
E_BADDESC, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -3   # DCFP_E_* of include/dcfp_hip.h

_P, _I, _L, _F, _Z = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t
_D = C.POINTER(ConvDesc)
_R = C.POINTER(BnRunning)
_H = C.POINTER(ConvF16Desc)
_H8 = C.POINTER(ConvF8Desc)

# name -> (restype, argtypes); mirrors include/dcfp_hip.h one to one
SIGNATURES = {
    "dcfp_abi_version": (_I, []),
    "dcfp_conv2d_workspace_bytes": (_Z, [_D, _I]),
    "dcfp_conv2d_wp_layout": (_I, [_D, _I, C.POINTER(WpEntry)]),
    "dcfp_conv2d_permute_weights_multi_f32": (_I, [_P, _I, _L, _P]),
    "dcfp_conv2d_pitch_supported": (_I, [_D]),
    "dcfp_conv2d_kernel_name": (_I, [_D, _I, C.c_char_p, _I]),
    "dcfp_conv2d_executed_fraction": (C.c_double, [_D, _I]),
    "dcfp_wino_tile_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_int64)]),
    "dcfp_conv2d_workspace_is_scratch": (_I, [_D, _I]),
    "dcfp_conv2d_dgrad_fanin_supported": (_I, [_D]),
    "dcfp_conv2d_dgrad_fanin_f32_nchw": (_I, [_D, _P, _L, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "dcfp_conv2d_dgrad_fanin_red_slots": (_L, [_D]),
    "dcfp_conv2d_dgrad_fanin_red_f32_nchw": (_I, [_D, _P, _L, _P, _P, _P, _P, _P, _P, _P, _P, _P, _Z, _I, _P]),
    "dcfp_bn_bwd_sums_from_partials_f32": (_I, [_P, _L, _I, _P, _F, _P, _P, _P, _P, _P]),
    "dcfp_conv2d_xform_bytes": (_Z, [_D]),
    "dcfp_conv2d_fwd_keep_f32_nchw": (_I, [_D, _P, _P, _P, _L, _P, _Z, _P, _P, _Z, _P]),
    "dcfp_conv2d_wgrad_kept_f32_nchw": (_I, [_D, _P, _L, _P, _Z, _P, _P, _Z, _P]),
    "dcfp_conv2d_fwd_f32_nchw": (_I, [_D, _P, _P, _P, _P, _L, _P, _Z, _I, _P]),
    "dcfp_conv2d_fwd_fused_f32_nchw": (_I, [_D, _P, _P, _P, _P, _P, _I, _P, _P, _Z, _I, _P]),
    "dcfp_conv2d_dgrad_f32_nchw": (_I, [_D, _P, _L, _P, _P, _I, _P, _Z, _I, _P]),
    "dcfp_conv2d_wgrad_f32_nchw": (_I, [_D, _P, _L, _P, _P, _P, _P, _Z, _P]),
    "dcfp_bn_workspace_bytes": (_Z, [_I, _I, _I]),
    "dcfp_bn_stats_f32": (_I, [_P, _L, _I, _I, _I, _P, _P, _R, _P, _Z, _P]),
    "dcfp_bn_apply_f32": (_I, [_P, _P, _P, _P, _P, _F, _P, _I, _P, _L, _I, _I, _I, _I, _I, _P]),
    "dcfp_bn_bwd_reduce_f32": (_I, [_P, _L, _P, _P, _L, _P, _P, _P, _P, _F, _I, _I, _I, _I, _P, _P, _P, _P,
                                    _P, _Z, _P]),
    "dcfp_bn_update_running_f32": (_I, [_P, _P, _I, _F, _F, _P, _P, _P, _P]),
    "dcfp_syncbn_combine_f32": (_I, [_P, _I, _I, _P, _P, _P, _R, _P]),
    "dcfp_syncbn_p2p_mailbox_bytes": (_Z, [_I, _I]),
    "dcfp_p2p_alloc": (_I, [_Z, _I, C.POINTER(C.c_void_p)]),
    "dcfp_p2p_free": (_I, [_P]),
    "dcfp_p2p_export": (_I, [_P, _P]),
    "dcfp_p2p_import": (_I, [_P, C.POINTER(C.c_void_p)]),
    "dcfp_p2p_unmap": (_I, [_P]),
    "dcfp_syncbn_p2p_exchange_f32": (_I, [C.POINTER(C.c_void_p), _I, _I, C.c_uint32, _I, _P, _I, _I, _P, _R,
                                          C.c_uint32, _P, _P]),
    "dcfp_bn_apply_relu_mask_f32": (_I, [_P, _P, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _P]),
    "dcfp_conv2d_fwd_stat_slots": (_L, [_D, _P, _L]),
    "dcfp_conv2d_fwd_stats_f32_nchw": (_I, [_D, _P, _P, _P, _L, _P, _P, _Z, _I, _P]),
    "dcfp_bn_stats_from_partials_f32": (_I, [_P, _L, _I, _I, _P, _P, _R, _P]),
    "dcfp_bn_bwd_apply_f32": (_I, [_P, _L, _P, _P, _L, _P, _P, _P, _P, _F, _P, _P, _F, _P, _I, _P, _P,
                                   _I, _I, _I, _I, _I, _P]),
    "dcfp_bn_bwd_fused_sync_bytes": (_Z, [_I, _I, _I]),
    "dcfp_bn_bwd_fused_f32": (_I, [_P, _L, _P, _P, _L, _P, _P, _P, _P, _F, _F, _I, _P, _P, _I, _I, _I, _I, _I,
                                   _P, _P, _P, _P, _P, _Z, C.c_uint32, C.c_uint32, _P, _P]),
    "dcfp_maxpool3x3s2_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dcfp_maxpool3x3s2_bwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "dcfp_rowsum_f32": (_I, [_P, _L, _P, _F, _I, _I, _I, _P]),
    "dcfp_broadcast_hw_f32": (_I, [_P, _F, _P, _L, _I, _I, _I, _I, _P]),
    "dcfp_add_f32": (_I, [_P, _P, _P, _L, _P]),
    "dcfp_channel_scale_f32": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "dcfp_upsample_bilinear_fwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dcfp_upsample_bilinear_bwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dcfp_resize_bilinear_into_f32": (_I, [_P, _L, _I, _I, _I, _I, _P, _L, _I, _I, _I, _I, _P]),
    "dcfp_resize_bilinear_adjoint_f32": (_I, [_P, _L, _I, _I, _I, _I, _I, _P, _L, _I, _I, _I, _I, _P]),
    "dcfp_ppm_pool_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _I, _P, _L, _I, _P]),
    "dcfp_ppm_pool_adjoint_f32": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _L, _I, _P, _P]),
    "dcfp_ppm_resize_adjoint_f32": (_I, [_P, _L, _I, _I, _I, _I, _I, _P, _P, _I, _P]),
    "dcfp_upsample_ce_workspace_bytes": (_Z, [_I, _I, _I]),
    "dcfp_upsample_ce_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P,
                                      _Z, _P]),
    "dcfp_upsample_ce_bwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dcfp_upsample_ce_bwd_plan": (_I, [_I, _I, _I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                       C.POINTER(C.c_int)]),
    "dcfp_ohem_zoom_gt_prob_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "dcfp_ohem_threshold_f32": (_I, [_P, _P, _L, _I, _F, _L, _P, _P]),
    "dcfp_ohem_keep_mask_u8": (_I, [_P, _P, _L, _P, _P]),
    "dcfp_upsample_margin_f32": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dcfp_maxfilter2d_s1_f32": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "dcfp_upsample_wce_workspace_bytes": (_Z, [_I, _I, _I]),
    "dcfp_upsample_wce_fwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _Z, _P]),
    "dcfp_upsample_wce_bwd_f32": (_I, [_P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P]),
    "dcfp_upsample_argmax_f32": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dcfp_confusion_matrix_i64": (_I, [_P, _P, _I, _L, _I, _P, _P]),
    "dcfp_vote_multiscale_f32": (_I, [C.POINTER(VoteMap), _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "dcfp_gather_tiles_f32": (_I, [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P]),
    "dcfp_vote_sliding_f32": (_I, [C.POINTER(SlidePass), _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "dcfp_label_boundary_workspace_bytes": (_Z, [_I, _I, _I]),
    "dcfp_label_boundary_i32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dcfp_label_boundary_i64": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _Z, _P]),
    "dcfp_png_deflate_bound": (_Z, [_I, _I]),
    "dcfp_png_deflate_workspace_bytes": (_Z, [_I, _I, _I, _I]),
    "dcfp_png_deflate_labels_i32": (_I, [_P, _I, _I, _I, _P, _I, _P, _Z, _P, _P, _P, _Z, _P]),
    "dcfp_augment_u8_to_f32_nchw": (_I, [C.POINTER(AugSample), _I, _I, _I, _P, _L, _P, _L, _P, _L, _P, _I, _P, _P, _P, _P]),
    "dcfp_balance_weight_f32": (_I, [_P, _P, _P, _I, _L, _I, _I, _I, C.c_double, _P, _P]),
    "dcfp_components_workspace_bytes": (_Z, [_I, _I]),
    "dcfp_label_components_u8": (_I, [C.POINTER(CcSample), _I, _P, _L, _P, _P, _Z, _P, _P]),
    "dcfp_component_pixel_i32": (_I, [C.POINTER(CcSample), _I, _P, _Z, _P, _P, _P, _P, _P]),
    "dcfp_eic_update_f32": (_I, [_P, _I, _F, _F, _P]),
    "dcfp_sgd_momentum_f32": (_I, [_P, _I, _L, _F, _F, _I, _P]),
    "dcfp_adamw_f32": (_I, [_P, _I, _L, _F, _F, _F, _F, _F, _F, _F, _P]),
    "dcfp_conv2d_fwd_f16_nhwc": (_I, [_H, _P, _P, _P, _P, _P, _P]),
    "dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw": (_I, [_H, _P, _P, _P, _P, _P]),
    "dcfp_maxpool3x3s2_nhwc_f16": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dcfp_avgpool_nhwc_f16_workspace_bytes": (_Z, [_I, _I, _L]),
    "dcfp_avgpool_nhwc_f16": (_I, [_P, _P, _I, _L, _I, _I, _I, _P, _Z, _P]),
    "dcfp_broadcast_nhwc_f16": (_I, [_P, _I, _P, _I, _L, _I, _I, _I, _P]),
    "dcfp_nchw_f32_to_nhwc_f16": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "dcfp_conv2d_fwd_f8_nhwc": (_I, [_H8, _P, _P, _P, _P, _P, _P, _P]),
    "dcfp_conv2d_fwd_f8_nhwc_to_f32_nchw": (_I, [_H8, _P, _P, _P, _P, _P, _P]),
    "dcfp_cast_nhwc_f16_to_f8": (_I, [_P, _I, _P, _I, _I, _L, _I, _F, _P]),
    "dcfp_maxpool3x3s2_nhwc_f8": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P]),
    "dcfp_avgpool_nhwc_f8_to_f16": (_I, [_P, _P, _I, _L, _I, _I, _I, _F, _P, _Z, _P]),
    "dcfp_broadcast_nhwc_f16_to_f8": (_I, [_P, _I, _P, _I, _L, _I, _I, _I, _F, _P]),
    "dcfp_resize_bilinear_nhwc_f16": (_I, [_P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _P]),
    "dcfp_pyramid_pool_nhwc_f16_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _P]),
    "dcfp_pyramid_pool_nhwc_f16": (_I, [_P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _Z, _P]),
    "dcfp_kd_workspace_bytes": (_Z, [_I, _I, _I, _I, _I]),
    "dcfp_kd_fwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _P, _Z, _P, _P, _P]),
    "dcfp_pairwise_workspace_bytes": (_Z, [_I, _I, _I, _I, _I, _I, _I]),
    "dcfp_pairwise_fwd_f32": (_I, [_P, _P, _I, _L, _I, _I, _I, _I, _I, _I, _P, _Z, _P, _I, _P]),
    "dcfp_pairwise_bwd_f32": (_I, [_I, _I, _I, _I, _I, _I, _P, _Z, _P, _P, _P]),
    "dcfp_lovasz_workspace_bytes": (_Z, [_I, _I]),
    "dcfp_lovasz_hist_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _Z, _P]),
    "dcfp_lovasz_scan_f32": (_I, [_I, _I, _P, _Z, _P, _P, _P]),
    "dcfp_lovasz_bwd_f32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _P, _P]),
    "dcfp_lovasz_errors_u32": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P]),
    "dcfp_gate_taylor_f32": (_I, [_P, _I, _P]),
    "dcfp_gate_l1reg_f32": (_I, [_P, _I, _F, _P]),
    "dcfp_filter_reduce_units": (_L, [_I, _I]),
    "dcfp_filter_reduce_f32": (_I, [_P, _I, _L, _I, _P]),
    "dcfp_fpgm_workspace_bytes": (_Z, [_I]),
    "dcfp_fpgm_f32": (_I, [_P, _I, _L, _P, _Z, _P]),
    "dcfp_state_digest_workspace_bytes": (_Z, [_Z]),
    "dcfp_state_digest_u64": (_I, [_P, _Z, C.c_uint64, _P, _Z, _P, _P]),
    "dcfp_grad_norm_workspace_bytes": (_Z, [_L]),
    "dcfp_grad_norm_f32": (_I, [_P, _I, _L, _F, _P, _Z, _P, _P, _P]),
    "dcfp_sgd_momentum_ex_f32": (_I, [_P, _I, _L, _F, _F, _I, _P, _F, _P]),
    "dcfp_adamw_ex_f32": (_I, [_P, _I, _L, _F, _F, _F, _F, _F, _F, _F, _P, _F, _P]),
    "dcfp_engine_open": (_I, [C.c_char_p, C.POINTER(_P), C.c_char_p, _Z]),
    "dcfp_engine_open_memory": (_I, [_P, _Z, C.POINTER(_P), C.c_char_p, _Z]),
    "dcfp_engine_close": (None, [_P]),
    "dcfp_engine_info": (_I, [_P, C.POINTER(EngineInfo)]),
    "dcfp_engine_weight_bytes": (_Z, [_P]),
    "dcfp_engine_upload": (_I, [_P, _P, _P]),
    "dcfp_engine_output_shape": (_I, [_P, _I, _I, _I, C.POINTER(_I), C.POINTER(_I), C.POINTER(_I)]),
    "dcfp_engine_buffer_shapes": (_I, [_P, _I, _I, C.POINTER(_I), _I]),
    "dcfp_engine_workspace_bytes": (_Z, [_P, _I, _I, _I]),
    "dcfp_engine_run_f32": (_I, [_P, _P, _P, _I, _I, _I, _P, _Z, _P, _P]),
    "dcfp_engine_run_u8": (_I, [_P, _P, _P, _Z, _I, _I, _I, _P, _Z, _P, _P]),
    "dcfp_image_u8_hwc_to_nhwc_f16": (_I, [_P, _Z, _I, _I, _I, _P, C.POINTER(_I), _P, _I, _P]),
}


def build(verbose=False):
    """Compile csrc/*.hip for gfx950 into libdcfp_hip.so (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or r.returncode != 0:
        print(r.stdout[-4000:])
        print(r.stderr[-4000:])
    if r.returncode != 0:
        raise RuntimeError("building libdcfp_hip.so failed")
    return LIB_PATH


def lib():
    """Load the shared object (after torch, so that it binds to the HIP runtime already in
    the process) and attach signatures.  No fallback: a missing library is an error."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C dcfp_amd/csrc`). dcfp_amd has no non-HIP fallback.")
        try:
            import torch  # noqa: F401  (loads libamdhip64.so.7 first; ours resolves to it)
        except Exception:  # pragma: no cover
            pass
        handle = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(status, what):
    if status != 0:
        kind = "descriptor/shape" if status < 0 else "hipError_t"
        raise RuntimeError(f"{what} failed: status {status} ({kind})")
