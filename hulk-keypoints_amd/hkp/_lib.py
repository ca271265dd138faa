"""ctypes binding of libhulkkp.so (the C ABI declared in include/hulkkp.h).

This is the only place the product touches native code.  There is no CPU or
PyTorch fallback: if the library is missing or a call fails, it raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# the product loads its own in-tree library; A/B tooling may point this process at
# another build of the same ABI with use_library() before the first call
LIB_PATH = os.path.join(_HERE, "libhulkkp.so")

HKP_LAYOUT_NHWC = 0
HKP_LAYOUT_NCHW = 1
HKP_LOSS_BCE = 0
HKP_LOSS_MSE = 1
HKP_LOSS_QFL = 2                   # hkp_heat_loss_multi_ex and hkp_heat_loss_planes only
HKP_ABSENT_ZERO = 0
HKP_ABSENT_IGNORE = 1
HKP_NORM_ELEMENTS = 0
HKP_NORM_INSTANCES = 1
QFL_BETA_RANGE = (1.0, 8.0)        # hkp_heat_loss_multi_ex's beta, both ends included
MAX_INSTANCES = 16                 # slots per plane of the multi-instance labels (hkp_heat_peaks' max_peaks limit)


class HkpError(RuntimeError):
    pass


class ConvDesc(ctypes.Structure):
    """hkp_conv_desc; `tile` (HKP_TILE_*, default 0 = the planner) is per call."""
    _fields_ = [(n, ctypes.c_int32) for n in
                ("n", "h", "w", "c", "k", "r", "s", "stride", "pad", "dilation", "in_layout", "tile")]


# hkp_conv_desc.tile policies (include/hulkkp.h)
(HKP_TILE_AUTO, HKP_TILE_NO_SK, HKP_TILE_SK, HKP_TILE_256, HKP_TILE_128_MF16, HKP_TILE_128_MF32, HKP_TILE_64_PAIR,
 HKP_TILE_RESERVED_7, HKP_TILE_RESERVED_8, HKP_TILE_256_TAIL, HKP_TILE_HALO, HKP_TILE_256_A3, HKP_TILE_AUTO_A3,
 HKP_TILE_DUO, HKP_TILE_RESERVED_14, HKP_TILE_192_A3, HKP_TILE_160_A3, HKP_TILE_MIX_A3) = range(18)
# hkp_conv_kernel_name ops
HKP_KOP_FWD_X3, HKP_KOP_DGRAD_X3, HKP_KOP_FWD_F16, HKP_KOP_STEM_X3, HKP_KOP_WGRAD_X3, HKP_KOP_FWD_X3_W16, \
    HKP_KOP_FWD_X3_X16, HKP_KOP_STEM_X3_IMAGE, HKP_KOP_STEM_X3_IMAGE_U8, HKP_KOP_FWD_F16_BN = range(10)
HKP_X3_W16, HKP_X3_ALL, HKP_X3_X16 = 2, 3, 4          # hkp_conv2d_fwd_x3_products product sets
HKP_MIX_PLAN_LEN = 14                                 # hkp_conv_x3_mix_plan's out[]
HKP_X3_LAUNCH_PLAN_LEN = 34                           # hkp_conv_x3_launch_plan's out[]
# its kernel ids (out[0])
HKP_X3K_TILE_256, HKP_X3K_TILE_128_MF16, HKP_X3K_TILE_128_MF32, HKP_X3K_PAIR_64, HKP_X3K_SK_128, HKP_X3K_SK_64, \
    HKP_X3K_A3, HKP_X3K_A3_192, HKP_X3K_A3_160, HKP_X3K_A3_160X128, HKP_X3K_A3_MIX, HKP_X3K_TAIL, HKP_X3K_HALO, \
    HKP_X3K_HALO_BNIN, HKP_X3K_DUO, HKP_X3K_STEM_PAIR, HKP_X3K_STEM_PATCH, HKP_X3K_STEM_PATCH_IMAGE, \
    HKP_X3K_STEM_PATCH_U8, HKP_X3K_COUNT = range(20)
# the per-launch values of out[], in order
X3_LAUNCH_FIELDS = ("kernel", "blocks", "threads", "n_tiles", "nks", "sk_units", "sk_one", "mt0", "main_blocks",
                    "tail_groups", "tail_mt0", "tail_units", "mix_b1", "mix_b2", "mix_m1", "mix_m2", "mix_p1", "mix_p2",
                    "stagger_blocks", "stagger_ns", "uses_ws", "ws_bytes")


class PackJob(ctypes.Structure):
    """hkp_pack_job (hkp_weight_pack_x3_batch)."""
    _fields_ = [("w", ctypes.c_void_p), ("out", ctypes.c_void_p), ("inv_scale", ctypes.c_void_p),
                ("kind", ctypes.c_int32), ("k", ctypes.c_int32), ("rs", ctypes.c_int32), ("c", ctypes.c_int32),
                ("r", ctypes.c_int32), ("s", ctypes.c_int32), ("pad", ctypes.c_int32), ("phase", ctypes.c_int32)]


class AdamTensor(ctypes.Structure):
    """hkp_adam_tensor (hkp_adam_step)."""
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("n", ctypes.c_int64)]


# hkp_aug_stage.kind and the fixed sizes of the augmentation ABI (include/hulkkp.h)
HKP_AUG_LUT, HKP_AUG_HSV, HKP_AUG_BLUR, HKP_AUG_NOISE = 1, 2, 3, 4
HKP_AUG_MAX_STAGES = 8
HKP_AUG_GAUSS_TABLE = 4096
HKP_AUG_TILE_H, HKP_AUG_TILE_W = 16, 64


class AugStage(ctypes.Structure):
    """hkp_aug_stage (hkp_augment_u8)."""
    _fields_ = [("kind", ctypes.c_int32), ("reserved0", ctypes.c_int32), ("f", ctypes.c_float * 3),
                ("key", ctypes.c_uint32 * 2), ("reserved1", ctypes.c_int32)]


class AugProgram(ctypes.Structure):
    """hkp_aug_program (hkp_augment_u8)."""
    _fields_ = [("nstages", ctypes.c_int32), ("reserved", ctypes.c_int32 * 7),
                ("stages", AugStage * HKP_AUG_MAX_STAGES)]


assert ctypes.sizeof(AugStage) == 32 and ctypes.sizeof(AugProgram) == 288

# the affine warp's ABI (include/hulkkp.h)
HKP_WARP_BILINEAR, HKP_WARP_NEAREST = 0, 1
HKP_WARP_BORDER_CONSTANT, HKP_WARP_BORDER_REPLICATE, HKP_WARP_BORDER_REFLECT101 = 0, 1, 2
HKP_WARP_MAX_DIM = 16384
# the ignore masks' ABI (include/hulkkp.h)
HKP_MASK_BOX, HKP_MASK_DISC = 1, 2
HKP_MASK_MAX_REGIONS = 64
HKP_MASK_MAX_DIM = 4096
MASK_MAX_K = 8                     # class bits of a mask byte (hkp_heat_loss_masked)
HKP_LINE_MAX_S = 128               # segment slots per plane of the line labels (hkp_line_target)


class WarpXform(ctypes.Structure):
    """hkp_warp_xform (hkp_warp_affine_u8): the inverse map dest -> source in Q16
    and the fill colour (B, G, R, unused)."""
    _fields_ = [("m", ctypes.c_int32 * 6), ("fill", ctypes.c_uint8 * 4), ("reserved", ctypes.c_int32)]


assert ctypes.sizeof(WarpXform) == 32


class ResampleImage(ctypes.Structure):
    """hkp_resample_image (hkp_resample_u8): where one image of the batch lies in the
    flat input, its size, the word offsets of its axis tables, its destination
    rectangle and the fill colour (B, G, R, unused)."""
    _fields_ = [("offset", ctypes.c_int64), ("hs", ctypes.c_int32), ("ws", ctypes.c_int32),
                ("xtab", ctypes.c_int64), ("ytab", ctypes.c_int64), ("x0", ctypes.c_int32), ("y0", ctypes.c_int32),
                ("wd", ctypes.c_int32), ("hd", ctypes.c_int32), ("fill", ctypes.c_uint8 * 4),
                ("reserved", ctypes.c_int32 * 3)]


assert ctypes.sizeof(ResampleImage) == 64

# the cable-scene renderer's ABI (include/hulkkp.h)
HKP_SYNTH_MAX_DIM = 4096
HKP_SYNTH_MAX_SEGS = 512


class SynthSeg(ctypes.Structure):
    """hkp_synth_seg (hkp_synth_cables_u8): one capsule in the kernel's fixed point."""
    _fields_ = [("x0", ctypes.c_int32), ("y0", ctypes.c_int32), ("ux", ctypes.c_int32), ("uy", ctypes.c_int32),
                ("len", ctypes.c_int32), ("r", ctypes.c_int32), ("r_in2", ctypes.c_int32), ("r_out2", ctypes.c_int32),
                ("r2", ctypes.c_int32), ("inv", ctypes.c_uint32), ("inv_r2", ctypes.c_uint32),
                ("bgr", ctypes.c_uint8 * 4), ("shade", ctypes.c_int32), ("arc", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 2)]


class SynthScene(ctypes.Structure):
    """hkp_synth_scene (hkp_synth_cables_u8): one image's pieces and background."""
    _fields_ = [("seg_off", ctypes.c_int32), ("seg_cnt", ctypes.c_int32), ("key", ctypes.c_uint32 * 2),
                ("bg0", ctypes.c_uint8 * 4), ("bg1", ctypes.c_uint8 * 4), ("cell_log2", ctypes.c_int32),
                ("reserved", ctypes.c_int32 * 9)]


assert ctypes.sizeof(SynthSeg) == 64 and ctypes.sizeof(SynthScene) == 64

# the test-time augmentation merge's ABI (include/hulkkp.h)
HKP_MERGE_LOGIT, HKP_MERGE_PROB = 0, 1
HKP_MERGE_MAX_VIEWS = 8


class MergeView(ctypes.Structure):
    """hkp_merge_view (hkp_logits_merge): where one view's logits lie in the packed
    buffer, its lattice, the per-axis map base node -> view node and its weight."""
    _fields_ = [("off", ctypes.c_int64), ("h", ctypes.c_int32), ("w", ctypes.c_int32), ("ay", ctypes.c_double),
                ("by", ctypes.c_double), ("ax", ctypes.c_double), ("bx", ctypes.c_double),
                ("weight", ctypes.c_double), ("reserved", ctypes.c_int64)]


assert ctypes.sizeof(MergeView) == 64

_P = ctypes.c_void_p
_I32 = ctypes.c_int32
_I64 = ctypes.c_int64
_F = ctypes.c_float
_CD = ctypes.POINTER(ConvDesc)

# name -> (restype, argtypes); must cover every function include/hulkkp.h declares
SIGNATURES = {
    "hkp_last_error": (ctypes.c_char_p, []),
    "hkp_version": (ctypes.c_char_p, []),
    "hkp_conv_out_hw": (ctypes.c_int, [_CD, ctypes.POINTER(_I32), ctypes.POINTER(_I32)]),
    "hkp_conv_stat_tiles": (_I64, [_CD]),
    "hkp_conv_x3_stat_tile_rows": (_I32, [_CD, _I32]),
    "hkp_conv_x3_stat_layout": (_I32, [_CD, _I32, ctypes.POINTER(_I32)]),
    "hkp_conv_x3_mix_plan": (_I32, [_I64, _I32, _I32, ctypes.POINTER(_I32)]),
    "hkp_conv_x3_launch_plan": (_I32, [_CD, _I32, _I32, _I32, _I32, ctypes.c_char_p, _I32, ctypes.POINTER(_I64)]),
    "hkp_conv2d_fwd": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P]),
    "hkp_bn_finalize": (ctypes.c_int, [_I32, _I64, _I64, _I32, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "hkp_bn_finalize_workspace_bytes": (_I64, [_I32, _I64]),
    "hkp_bn_finalize_ws": (ctypes.c_int, [_I32, _I64, _I64, _I32, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P, _I64,
                                          _P]),
    "hkp_bn_stats": (ctypes.c_int, [_I32, _I64, _I64, _I32, _P, _P, _P, _I64, _P]),
    "hkp_bn_finalize_seg": (ctypes.c_int, [_I32, _I64, _I32, ctypes.POINTER(_I32), _P, _P, _P, _F, _F, _P, _P, _P, _P,
                                           _P, _P, _I64, _P]),
    "hkp_bn_stats_seg": (ctypes.c_int, [_I32, _I64, _I32, ctypes.POINTER(_I32), _P, _P, _P, _I64, _P]),
    "hkp_bn_finalize_ranks": (ctypes.c_int, [_I32, _I32, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P]),
    "hkp_bn_eval_params": (ctypes.c_int, [_I32, _P, _P, _P, _P, _F, _P, _P, _P]),
    "hkp_bn_apply": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _I32, _P, _P, _I32, _P]),
    "hkp_bn_apply_f16": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _P, _I32, _P, _P, _P]),
    "hkp_bn_relu_maxpool": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _I32, _P, _P]),
    "hkp_head_fc": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "hkp_bn_apply_head": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _I32, _P, _P, _P, _P]),
    "hkp_upsample_sigmoid": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    "hkp_gauss_target": (ctypes.c_int, [_I32, _I32, _I32, _I32, _F, _P, _P, _P]),
    "hkp_weight_pack_x3": (ctypes.c_int, [_I32, _I32, _I32, _P, _P, _P, _P]),
    "hkp_conv2d_fwd_x3": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "hkp_conv2d_fwd_x3_products": (ctypes.c_int, [_CD, _P, _P, _P, _I32, _P, _P, _P, _I64, _P]),
    "hkp_conv2d_fwd_x3_bnin": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "hkp_conv2d_fwd_f16_bnin": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "hkp_conv_x3_sk_workspace_bytes": (_I64, []),
    "hkp_absmax": (ctypes.c_int, [_I64, _P, _P, _P]),
    "hkp_weight_pack_f16": (ctypes.c_int, [_I32, _I32, _P, _P, _P, _P]),
    "hkp_conv2d_fwd_f16": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "hkp_conv2d_fwd_f16_bn": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P, _I32, _P, _P, _I64, _P]),
    "hkp_gram_f16_workspace_bytes": (_I64, [_I64, _I32]),
    "hkp_gram_f16": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _P, _I64, _P]),
    "hkp_bn_from_gram_workspace_bytes": (_I64, [_I32, _I32]),
    "hkp_bn_from_gram": (ctypes.c_int, [_I32, _I32, _I64, _P, _P, _P, _P, _P, _P, _F, _F, _P, _P, _P, _P, _P, _P,
                                        _I64, _P]),
    "hkp_conv_kernel_name": (_I32, [_CD, _I32, _I32, ctypes.c_char_p, _I32]),
    "hkp_upsample_argmax_ws_bytes": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_stem_pack_x3_elems": (_I64, [_CD]),
    "hkp_stem_pack_x3": (ctypes.c_int, [_CD, _P, _P, _P]),
    "hkp_stem_pack_x3_u8": (ctypes.c_int, [_CD, _P, _P, _P]),
    "hkp_images_u8_to_nchw": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P]),
    "hkp_soft_argmax": (ctypes.c_int, [_I32, _I32, _I32, _I32, _F, _P, _P, _P]),
    "hkp_heat_peaks": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _P]),
    "hkp_heat_overlay": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P]),
    "hkp_stem_weight_pack_x3": (ctypes.c_int, [_I32, _I32, _P, _P, _P, _P]),
    "hkp_conv2d_fwd_stem_x3": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P]),
    "hkp_stem_x3_image_ok": (_I32, [_CD]),
    "hkp_conv2d_fwd_stem_x3_image": (ctypes.c_int, [_CD, _P, _I32, _P, _P, _P, _P, _P]),
    "hkp_split_pack_x3": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _P]),
    "hkp_weight_flip_pack_x3": (ctypes.c_int, [_CD, _P, _P, _P, _P]),
    "hkp_conv2d_bwd_data_x3": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    "hkp_phase_taps": (_I32, [_I32, _I32, _I32, _I32]),
    "hkp_conv2d_bwd_data_x3_strided": (ctypes.c_int, [_CD, _P, ctypes.POINTER(_P), ctypes.POINTER(_P), _P, _P, _P,
                                                       _P, _I64, _P]),
    "hkp_weight_pack_x3_batch_ws_bytes": (_I64, [_I32, ctypes.POINTER(PackJob)]),
    "hkp_weight_pack_x3_batch": (ctypes.c_int, [_I32, ctypes.POINTER(PackJob), _P, _I64, _P]),
    "hkp_conv_bwd_filter_x3_workspace": (_I64, [_CD]),
    "hkp_conv2d_bwd_filter_x3": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P, _I64, _P]),
    "hkp_adam_step": (ctypes.c_int, [_I32, ctypes.POINTER(AdamTensor), _F, _F, _F, _F, _F, _F, _F, _P]),
    # gradient clipping / weight EMA (ema: host array of device pointers; coef, partials, out: device)
    "hkp_grad_norm_partials": (_I64, [_I32, ctypes.POINTER(AdamTensor)]),
    "hkp_grad_norm": (ctypes.c_int, [_I32, ctypes.POINTER(AdamTensor), _F, _P, _I64, _P, _P]),
    "hkp_adam_step_ex": (ctypes.c_int, [_I32, ctypes.POINTER(AdamTensor), ctypes.POINTER(_P), _F, _P, _F, _F, _F, _F,
                                        _F, _F, _F, _P]),
    # backward
    "hkp_conv_weight_flip":(ctypes.c_int, [_CD, _P, _P, _P]),
    "hkp_conv2d_bwd_data": (ctypes.c_int, [_CD, _P, _P, _P, _P, _P]),
    "hkp_conv_bwd_filter_workspace": (_I64, [_CD]),
    "hkp_conv2d_bwd_filter": (ctypes.c_int, [_CD, _P, _P, _P, _I32, _P, _I64, _P]),
    "hkp_bn_bwd_tiles": (_I64, [_I64]),
    "hkp_bn_bwd_reduce": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hkp_bn_bwd_finalize": (ctypes.c_int, [_I32, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hkp_bn_bwd_stats": (ctypes.c_int, [_I32, _I64, _P, _P, _P, _P, _P]),
    "hkp_bn_bwd_finalize_ranks": (ctypes.c_int, [_I32, _I32, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "hkp_bn_bwd_apply": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "hkp_maxpool_bwd": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P, _P]),
    "hkp_heat_loss_workspace": (_I64, []),
    "hkp_heat_loss": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _P, _P, _P, _F, _P, _P, _P, _P]),
    # multi-instance labels pts [n,k,m,3] (u, v, flag)
    "hkp_gauss_target_multi": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _F, _P, _P, _P]),
    "hkp_heat_loss_multi_workspace": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_heat_loss_multi": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _F, _P, _P, _P, _P]),
    # ... with the quality focal kind and the divisor's choice (norm_mode, beta after absent_mode)
    "hkp_heat_loss_multi_ex": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _P, _P, _F, _P, _P,
                                              _P, _P]),
    # ... with plane weights [n,k], the per-plane outputs and top-k (topk after beta; weights after pts;
    # plane_loss, plane_used after dheat)
    "hkp_heat_loss_planes_workspace": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_heat_loss_planes": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P, _P, _P, _F,
                                            _P, _P, _P, _P, _P, _P]),
    # ... with a per-pixel ignore mask uint8 [n,H,W] of class bits (mask after weights; plane_pixels after
    # plane_used)
    "hkp_heat_loss_masked_workspace": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_heat_loss_masked": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P, _P, _P, _P,
                                            _F, _P, _P, _P, _P, _P, _P, _P]),
    # evaluation: peaks/counts of hkp_heat_peaks against pts (thresholds: float array on the host)
    "hkp_peaks_match": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(_F), _P, _P, _P, _P, _P, _P,
                                       _P, _P, _P]),
    "hkp_head_bwd_workspace": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_head_bwd": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _I64, _P]),
    "hkp_head_fc_bwd_workspace": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_head_fc_bwd": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P, _I64, _P]),
    # hybrid JPEG decode, device half (the geometry struct: hkp.jpeg.Geom)
    "hkp_jpeg_planes_bytes": (_I64, [_P]),
    "hkp_jpeg_reconstruct": (ctypes.c_int, [_I32, _P, _P, _P, _P, _I64, _P, _P]),
    # domain randomisation (programs_host: AugProgram array on the host, programs: its device copy)
    "hkp_augment_u8": (ctypes.c_int, [_I32, _I32, _I32, _P, _P, ctypes.POINTER(AugProgram), _P, _P, _P, _P]),
    # affine warp (xforms_host: WarpXform array on the host, xforms: its device copy)
    "hkp_warp_affine_u8": (ctypes.c_int, [_I32, _I32, _I32, _P, _I32, _I32, _P, ctypes.POINTER(WarpXform), _P, _I32,
                                          _I32, _P]),
    # ignore masks: the one-channel nearest warp (border, fill byte, lut [n,256] or null) and the rasteriser
    # of region records (regions fp32 [n,r,6] on the device)
    "hkp_warp_mask_u8": (ctypes.c_int, [_I32, _I32, _I32, _P, _I32, _I32, _P, ctypes.POINTER(WarpXform), _P, _I32, _I32,
                                        _P, _P]),
    "hkp_mask_regions_u8": (ctypes.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P]),
    # antialiased resize (records_host / tables_host: host copies, validated; records / tables: device copies)
    "hkp_resample_u8": (ctypes.c_int, [_I32, _P, _I64, ctypes.POINTER(ResampleImage), _P, _P, _P, _I64, _I32, _I32,
                                       _P, _P]),
    # procedural cable scenes (scenes_host / segs_host: host copies, validated; scenes / segs: device copies)
    "hkp_synth_cables_u8": (ctypes.c_int, [_I32, _I32, _I32, _P, ctypes.POINTER(SynthScene), _P,
                                           ctypes.POINTER(SynthSeg), _P, _I32, _P]),
    # test-time augmentation: views' logits merged on the base lattice (table: MergeView records, perm: device)
    "hkp_logits_merge": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P]),
    # associative-embedding tags (tags: channel k of image 0 of low_all, batch stride in elements;
    # order: int32 array on the host)
    "hkp_tag_loss_workspace": (_I64, [_I32]),
    "hkp_tag_loss": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _F, _F, _F, _P, _P, _P,
                                    _P]),
    "hkp_peaks_group": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, ctypes.POINTER(_I32), _F, _P, _P,
                                       _P, _I64, _P, _P, _P, _P]),
    # line labels lines [n,k,s,5] (x0, y0, x1, y1, flag): target f64 and / or d2 f32, each nullable
    "hkp_line_target": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _F, _P, _P, _P, _P]),
    # the plane loss against line labels (lines in place of pts; weights and mask nullable)
    "hkp_heat_loss_lines_workspace": (_I64, [_I32, _I32, _I32, _I32]),
    "hkp_heat_loss_lines": (ctypes.c_int, [_I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _F, _I32, _P, _P, _P, _P,
                                           _F, _P, _P, _P, _P, _P, _P, _P]),
}

# the A/B instruments of the tools-only build (include/hulkkp_ab.h, `make ab`);
# bound only when the loaded library exports them — the product library does not
AB_SIGNATURES = {
    "hkp_debug_x3_stamps": (None, [_P]),
    "hkp_debug_x3_stagger": (None, [_I32]),
    "hkp_debug_x3_split_tail": (None, [_I32]),
    "hkp_debug_stem_pair": (None, [_I32]),
    "hkp_debug_fin_regs": (None, [_I32]),
    "hkp_debug_x3_pair128": (None, [_I32]),
    "hkp_debug_x3_store": (None, [_I32]),
    "hkp_debug_duo_stagger": (None, [_I32]),
    "hkp_debug_x3_prio": (None, [_I32]),
    "hkp_debug_x3_a_wrap": (None, [_I32]),
}
AB_LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "tools", "ab_lib", "libhulkkp_ab.so")

_lib = None


def use_library(path):
    """Tools only (in-process A/B of two builds): load `path` instead of the in-tree
    library.  Must run before the first kernel call of the process."""
    global LIB_PATH
    if _lib is not None:
        raise HkpError("use_library: %s is already loaded" % LIB_PATH)
    LIB_PATH = path


def use_ab_library():
    """Tools only: load the A/B build (tools/ab_lib/libhulkkp_ab.so, `make -C
    hulk-keypoints_amd/csrc ab`), whose hkp_debug_* knobs the product library lacks."""
    if not os.path.exists(AB_LIB_PATH):
        raise HkpError("the A/B build is missing (%s): run `make -C hulk-keypoints_amd/csrc ab`" % AB_LIB_PATH)
    use_library(AB_LIB_PATH)


def lib():
    """Load libhulkkp.so once; raise HkpError (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HkpError("libhulkkp.so is not built (%s); run `python -c 'import __graft_entry__ as g; g.build()'`"
                           % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        other = os.path.abspath(LIB_PATH) != os.path.join(_HERE, "libhulkkp.so")
        for name, (res, args) in SIGNATURES.items():
            if other and not hasattr(L, name):
                continue                # tools: an older build of the ABI (its missing calls raise if used)
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        for name, (res, args) in AB_SIGNATURES.items():
            if hasattr(L, name):
                fn = getattr(L, name)
                fn.restype = res
                fn.argtypes = args
        _lib = L
    return _lib


def call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        msg = lib().hkp_last_error().decode(errors="replace")
        raise HkpError("%s failed (rc=%d): %s" % (name, rc, msg))
    return rc


def version():
    return lib().hkp_version().decode()
