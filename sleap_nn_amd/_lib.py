"""ctypes binding of libposehip.so (the C ABI declared in include/posehip.h).

The HIP library is the product: if it cannot be loaded this module raises -- there is no
CPU or PyTorch fallback anywhere in ``sleap_nn_amd``.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libposehip.so")

PH_OK = 0
PH_E_INVALID, PH_E_HIP, PH_E_CAPACITY, PH_E_INFEASIBLE, PH_E_WORKSPACE = -1, -2, -3, -4, -5

OP_INPUT_CONV, OP_CONV, OP_POOL, OP_UPSAMPLE, OP_CONVT, OP_HEAD, OP_STEM = 1, 2, 3, 4, 5, 6, 7
OP_PATCH_STEM, OP_DWCONV, OP_LAYERNORM, OP_LINEAR, OP_PATCH_CONV, OP_GELU, OP_SCALE_ADD, OP_GLOBAL_MAXPOOL = 8, 9, 10, 11, 12, 13, 14, 15
OP_PATCH_MERGE, OP_WINDOW_ATTN = 16, 17  # Swin Transformer encoder (swin_kernels.hip)
OP_GRN = 18  # ConvNeXtV2's Global Response Normalization (convnextv2_kernels.hip)
OP_WINDOW_ATTN_V2 = 22  # Swinv2's cosine window attention (swin_kernels.hip's cosine variant, swinv2_kernels.hip above window 8); its table, padded-token q | 0 | v and head scales are derived on the host
OP_RESNET_STEM, OP_CONV_S2, OP_ADD_RELU = 19, 20, 21  # ResNet encoder: normalised 7x7 stride-2 stem + 3x3 stride-2 max pool, strided 1x1 / 3x3 conv, relu(a + b) (resnet_kernels.hip)
FLAG_RELU, FLAG_SIGMOID, FLAG_GELU, FLAG_SCALE_RESIDUAL, FLAG_SOFTMAX, FLAG_SILU, FLAG_NO_TRAIN = 1, 2, 4, 8, 16, 32, 64
FLAG_LN_EPS_1EM5, FLAG_RESIDUAL = 128, 256
FLAG_NO_NORM = 1024  # PH_OP_PATCH_MERGE: the four-phase gather alone (Swinv2 norms behind the reduction); FLAG_RESIDUAL on PH_OP_LAYERNORM: dst = src1 + LayerNorm(src0)
FLAG_PAD0_NORM = 512  # PH_OP_PATCH_STEM: padding 0 and (x / 255 - mean) / std with the handle's input statistics (ph_model_set_input_norm)
LOSS_MSE, LOSS_BCE_DICE, LOSS_MASKED_SMOOTH_L1 = 1, 2, 3  # PH_LOSS_*: ph_model_set_head_loss
# PH_KV_*: kernel family an op of the last forward ran (ph_model_last_kernels) and the share of its direct-convolution
# FLOPs that family puts through the matrix cores
KV_NONE, KV_DIRECT, KV_WINO1D, KV_WINO2D, KV_W16, KV_C16, KV_ROWGEMM, KV_WINO4, KV_F16, KV_STEM, KV_WINO2D_KS, KV_FUSED, KV_SMALLMAP, KV_F16_ROWS, KV_F16_BLOCK, KV_MLP = range(16)
SWIN_KV_WINDOW_ATTN = 21  # PH_KV_WINDOW_ATTN (swin_kernels.hip); not named KV_* either, for the reason below
SWIN_KV_WINDOW_ATTN_BWD = 24  # PH_KV_WINDOW_ATTN_BWD (swin_train_kernels.hip): reported by ph_model_last_backward_kernels
SWIN_KV_WINDOW_ATTN_F16, SWIN_KV_F16_MERGE_LN = 22, 23  # PH_KV_WINDOW_ATTN_F16 / PH_KV_SWIN_F16_MERGE_LN: the Swin ops on fp16 activations (swin_f16_kernels.hip, handle option swint_f16)
CNX2_KV_GRN, CNX2_KV_GRN_FUSED, CNX2_KV_PATCH_STEM_NORM = 25, 26, 27  # PH_KV_GRN / PH_KV_GRN_FUSED / PH_KV_PATCH_STEM_NORM (convnextv2_kernels.hip)
RESNET_KV_STEM, RESNET_KV_CONV_S2, RESNET_KV_ADD_RELU = 29, 30, 31  # PH_KV_RESNET_STEM / PH_KV_CONV_S2 / PH_KV_ADD_RELU (resnet_kernels.hip, the strided row-GEMM modes)
SWINV2_KV_WINDOW_ATTN, SWINV2_KV_LAYERNORM_ADD, SWINV2_KV_MERGE_GATHER = 32, 33, 34  # PH_KV_WINDOW_ATTN_V2 / PH_KV_LAYERNORM_ADD / PH_KV_PATCH_MERGE_GATHER (swin_kernels.hip's cosine variant, swinv2_kernels.hip, swin_train_kernels.hip's gather)
SWINV2_KV_WINDOW_ATTN_WIDE = 35  # PH_KV_WINDOW_ATTN_V2_WIDE (swinv2_kernels.hip): the key-tiled kernel of windows 9..24
CNX2_KV_GRN_BWD = 28  # PH_KV_GRN_BWD (convnextv2_train_kernels.hip): reported by ph_model_last_backward_kernels
CNX_KV_F16_STEM, CNX_KV_F16_DW, CNX_KV_F16_LN, CNX_KV_F16_GEMM, CNX_KV_F16_ELTWISE = 16, 17, 18, 19, 20  # PH_KV_CNX_F16_*: the ConvNeXt encoder ops on fp16 activations (convnext_f16_kernels.hip); not named KV_*: that prefix lists the families a 3x3 conv can come back with (benchlegs.common.conv_kernel_short_names)
KV_NAMES = {KV_NONE: "none", KV_DIRECT: "conv3x3_mfma_dma_persist_kernel (direct)", KV_WINO1D: "conv3x3_wino_persist_kernel (Winograd F(2,3) along x)",
            KV_WINO2D: "conv3x3_wino2d_kernel<64> (Winograd F(2x2,3x3))", KV_W16: "conv3x3_w16_kernel (wave-private Winograd F(2x2,3x3), 16x16x4 MFMA)",
            KV_C16: "conv3x3_c16_kernel (direct)", KV_ROWGEMM: "gemm_mfma_dma_kernel (row GEMM, direct)", KV_WINO4: "conv3x3_wino4_kernel (Winograd F(4x4,3x3))",
            KV_F16: "conv3x3_f16_persist_kernel (direct, fp16 matrix pipe)", KV_STEM: "stem_fused_kernel",
            KV_WINO2D_KS: "conv3x3_wino2d_kernel<64, split K> + splitk_reduce_kernel", KV_FUSED: "fused into its producer's epilogue",
            KV_SMALLMAP: "conv3x3_sm_kernel (Winograd F(2x2,3x3), small maps)",
            KV_F16_ROWS: "conv3x3_f16_rows_kernel (direct, plain fp16 on v_mfma_f32_16x16x32_f16: row tiles, loader waves, folded bilinear x2)",
            KV_F16_BLOCK: "block2_c32_f16_kernel (two convs of a 32-channel encoder block in one launch, plain fp16)",
            KV_MLP: "cnblock_mlp_kernel (CNBlock MLP: Linear + GELU + Linear + layer scale + residual in one launch, chained MFMA products)",
            CNX_KV_F16_STEM: "patch_stem_f16_kernel (ConvNeXt patch stem, fp16 output)",
            CNX_KV_F16_DW: "dwconv7_f16_kernel / dwconv7_ln_f16_kernel (depthwise 7x7 on fp16 activations, LayerNorm fused in inference plans)",
            CNX_KV_F16_LN: "layernorm_f16_kernel (LayerNorm over channels, fp16 storage, fp32 moments)",
            CNX_KV_F16_GEMM: "gemm_f16_kernel (row GEMM on v_mfma_f32_32x32x16_f16: Linear / 2x2-stride-2 conv)",
            CNX_KV_F16_ELTWISE: "gelu_fmt_kernel / scale_add_fmt_kernel (fp16 activations)",
            SWIN_KV_WINDOW_ATTN: "window_attn_kernel (shifted-window attention, one wave per window and head, v_mfma_f32_32x32x2_f32)",
            SWIN_KV_WINDOW_ATTN_BWD: "window_attn_bwd_kernel (backward of the shifted-window attention core, v_mfma_f32_32x32x2_f32, fixed-order slices)",
            SWIN_KV_WINDOW_ATTN_F16: "window_attn_f16_kernel (shifted-window attention on v_mfma_f32_32x32x16_f16: fp16 q / k / v / p, fp32 logits)",
            SWIN_KV_F16_MERGE_LN: "patch_merge_ln_f16_kernel (four-phase gather + LayerNorm(4C), fp16 storage, fp32 moments)",
            CNX2_KV_GRN: "grn_reduce_kernel + grn_apply_kernel (Global Response Normalization: fixed-slice sums of squares, then the apply pass)",
            CNX2_KV_GRN_FUSED: "grn_finalize_kernel (fused GRN plan: sums of squares from the Linear in front, per-sample scaled weights for the Linear behind)",
            CNX2_KV_PATCH_STEM_NORM: "patch_stem_norm_kernel (padding-0 patch stem with input statistics)",
            CNX2_KV_GRN_BWD: "grn_bwd_reduce_kernel + grn_bwd_sample_kernel + grn_bwd_param_kernel + grn_bwd_apply_kernel (backward of Global Response Normalization, fixed-order sums)"}
# PH_BR_*: the route word of one op's step of the last backward (ph_model_last_backward_routes, include/posehip.h).  Per concat part p (0 / 1), at bit 11 p:
# weight-gradient route (4 bits), data-gradient route (6 bits), "accumulated into an existing gradient" (1 bit); then the op's own output gradient (who applied the
# ReLU mask, who summed the bias gradient) and the flags of a step that closes another op's gradient or fuses / skips a launch
BR_PART_BITS = 11
BR_WG_NONE, BR_WG_DIRECT, BR_WG_WINO, BR_WG_WINO16, BR_WG_ROWS9, BR_WG_ROWSKK, BR_WG_INPUT, BR_WG_PATCH_STEM, BR_WG_CONVT_TAPS, BR_WG_ROW_GEMM = range(10)
BR_WG_NAMES = {BR_WG_NONE: "none", BR_WG_DIRECT: "launch_wgrad (32x32 tiles)", BR_WG_WINO: "launch_wgrad_wino", BR_WG_WINO16: "launch_wgrad16_wino",
               BR_WG_ROWS9: "nine row GEMMs (conv_wgrad_rows on a 3x3 conv)", BR_WG_ROWSKK: "k^2 row GEMMs (k x k conv)", BR_WG_INPUT: "launch_input_wgrad",
               BR_WG_PATCH_STEM: "launch_patch_stem_wgrad", BR_WG_CONVT_TAPS: "transposed-conv taps (nine gathered row GEMMs)", BR_WG_ROW_GEMM: "Linear / 2x2-stride-2 conv row GEMM"}
# data-gradient route: 0 = none, a KV_* code below 32 = the LDS-DMA family's kernel (ConvRoute::kv), else one of
BR_DG_NONE, BR_DG_REGSTAGED, BR_DG_GEMM5, BR_DG_GEMM4, BR_DG_GEMM0 = 0, 32, 33, 34, 35
BR_DG_NAMES = {BR_DG_NONE: "none", BR_DG_REGSTAGED: "launch_conv3x3 (register-staged)", BR_DG_GEMM5: "row GEMM mode 5 (k x k taps)", BR_DG_GEMM4: "row GEMM mode 4 (3x3 stride 2)",
               BR_DG_GEMM0: "row GEMM mode 0 (Linear / 2x2-stride-2 conv)"}
BR_DG_DMA_CODES = (KV_DIRECT, KV_WINO1D, KV_WINO2D, KV_W16, KV_C16, KV_WINO4, KV_WINO2D_KS)  # the kv of a ConvRoute in the LDS-DMA family
BR_MASK_NONE, BR_MASK_OWN, BR_MASK_EARLIER = range(3)
BR_MASK_NAMES = {BR_MASK_NONE: "none", BR_MASK_OWN: "this step (launch_relu_mask / launch_relu_mask_bias_grad)", BR_MASK_EARLIER: "an earlier step's stores (mask_fold)"}
BR_BIAS_NONE, BR_BIAS_OWN, BR_BIAS_WITH_MASK, BR_BIAS_CLOSER, BR_BIAS_INPUT_WGRAD, BR_BIAS_ROW_WGRAD = range(6)
BR_BIAS_NAMES = {BR_BIAS_NONE: "none", BR_BIAS_OWN: "own launch_bias_grad", BR_BIAS_WITH_MASK: "launch_relu_mask_bias_grad", BR_BIAS_CLOSER: "the closing pool / head step",
                 BR_BIAS_INPUT_WGRAD: "spare column of launch_input_wgrad", BR_BIAS_ROW_WGRAD: "the Linear's weight-gradient row GEMM"}
BR_FLAGS = ("folded_mask", "summed_bias", "gelu_fused", "no_launch")  # bits 27..30
_BR_MASK_SHIFT, _BR_BIAS_SHIFT, _BR_FLAG_SHIFT = 22, 24, 27


def br_dgrad_name(code: int) -> str:
    return BR_DG_NAMES[code] if code in BR_DG_NAMES else KV_NAMES[code]


def br_encode(wgrad=(0, 0), dgrad=(0, 0), accumulate=(0, 0), mask=0, bias=0, **flags) -> int:
    """The route word of the given fields (the inverse of ``br_decode``)."""
    word = 0
    for p in (0, 1):
        assert 0 <= wgrad[p] < 16 and 0 <= dgrad[p] < 64
        word |= (int(wgrad[p]) | int(dgrad[p]) << 4 | (1 if accumulate[p] else 0) << 10) << (BR_PART_BITS * p)
    assert 0 <= mask < 4 and 0 <= bias < 8 and set(flags) <= set(BR_FLAGS)
    word |= int(mask) << _BR_MASK_SHIFT | int(bias) << _BR_BIAS_SHIFT
    for i, name in enumerate(BR_FLAGS):
        word |= (1 if flags.get(name) else 0) << (_BR_FLAG_SHIFT + i)
    return word


def br_decode(word: int) -> dict:
    """Fields of one route word: ``wgrad`` / ``dgrad`` / ``accumulate`` per concat part, ``mask``, ``bias`` and the four flags of ``BR_FLAGS``."""
    word = int(word)
    parts = [(word >> (BR_PART_BITS * p)) & ((1 << BR_PART_BITS) - 1) for p in (0, 1)]
    out = {"wgrad": tuple(q & 15 for q in parts), "dgrad": tuple((q >> 4) & 63 for q in parts), "accumulate": tuple((q >> 10) & 1 for q in parts),
           "mask": (word >> _BR_MASK_SHIFT) & 3, "bias": (word >> _BR_BIAS_SHIFT) & 7}
    for i, name in enumerate(BR_FLAGS):
        out[name] = (word >> (_BR_FLAG_SHIFT + i)) & 1
    return out


KV_MFMA_SHARE = {KV_NONE: 0.0, KV_DIRECT: 1.0, KV_WINO1D: 2.0 / 3.0, KV_WINO2D: 4.0 / 9.0, KV_W16: 4.0 / 9.0, KV_C16: 1.0, KV_ROWGEMM: 1.0, KV_WINO4: 0.25, KV_F16: 1.0, KV_STEM: 4.0 / 9.0, KV_WINO2D_KS: 4.0 / 9.0, KV_FUSED: 0.0, KV_SMALLMAP: 4.0 / 9.0, KV_F16_ROWS: 1.0, KV_F16_BLOCK: 1.0, KV_MLP: 1.0, CNX_KV_F16_STEM: 0.0, CNX_KV_F16_DW: 0.0, CNX_KV_F16_LN: 0.0, CNX_KV_F16_GEMM: 1.0, CNX_KV_F16_ELTWISE: 0.0, SWIN_KV_WINDOW_ATTN: 1.0, SWIN_KV_WINDOW_ATTN_BWD: 1.0, SWIN_KV_WINDOW_ATTN_F16: 1.0, SWIN_KV_F16_MERGE_LN: 0.0, CNX2_KV_GRN: 0.0, CNX2_KV_GRN_FUSED: 0.0, CNX2_KV_PATCH_STEM_NORM: 0.0, CNX2_KV_GRN_BWD: 0.0, SWINV2_KV_WINDOW_ATTN: 1.0, SWINV2_KV_LAYERNORM_ADD: 0.0, SWINV2_KV_MERGE_GATHER: 0.0}


class OpDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "src0", "src1", "dst", "cin0", "cin1", "cout", "ksize", "flags", "weight", "bias", "out_index", "dst2", "weight2", "bias2", "cmid")]


class AugSample(C.Structure):
    """``struct ph_aug_sample`` (include/posehip.h): one sample's augmentation parameters."""

    _fields_ = [("minv", C.c_float * 6), ("m", C.c_float * 6), ("edge", C.c_float * 12), ("flags", C.c_int32), ("uni_lo", C.c_int32), ("uni_hi", C.c_int32),
                ("gauss_mean", C.c_float), ("gauss_std", C.c_float), ("contrast", C.c_float), ("brightness", C.c_float), ("erase_y", C.c_int32),
                ("erase_x", C.c_int32), ("erase_h", C.c_int32), ("erase_w", C.c_int32), ("fill", C.c_int32 * 3), ("seed", C.c_uint32), ("pad_", C.c_int32)]


class GemmCase(C.Structure):
    """``struct ph_gemm_case`` (include/posehip.h): one row-GEMM launch of ph_debug_gemm_run (test support)."""

    _fields_ = ([(n, C.c_int32) for n in ("variant", "mode", "M", "H", "W", "ksize", "tap_stride", "out_patch", "out_tap", "out_H", "out_W", "all_phases", "act", "affine_first",
                                          "late_split", "persist2", "sq_hw", "sq_nseg", "cin0", "cin1", "cout", "bn", "variant_used", "bn_used")]
                + [(n, C.c_void_p) for n in ("src0", "src1", "residual", "aux", "dst", "dst_pre", "sumsq", "weight", "bias", "scale", "shift")])


class ConvRouteCase(C.Structure):
    """``struct ph_conv_route_case`` (include/posehip.h): one exact-fp32 3x3 conv launch as ph_debug_conv3x3_route takes it (test support; launches nothing)."""

    _fields_ = ([(n, C.c_int32) for n in ("c0p", "c1p", "coutp", "bn", "B", "H", "W", "forms", "flags", "head_cout", "head_wcp", "use_dma", "dma32", "use_wino", "persist", "use_c16",
                                          "use_w16", "use_wino2d", "use_wino4", "wino4_min_cin", "use_sm", "splitk", "ptr_salt")] + [("split_scratch_bytes", C.c_int64)])


class ConvRunCase(C.Structure):
    """``struct ph_conv_run_case`` (include/posehip.h): one routed exact-fp32 3x3 conv launch of ph_debug_conv3x3_run (test support)."""

    _fields_ = ([(n, C.c_int32) for n in ("cin0", "cin1", "cout", "bn", "B", "H", "W", "forms", "flags", "head_cout", "use_dma", "dma32", "use_wino", "persist", "use_c16", "use_w16",
                                          "use_wino2d", "use_wino4", "wino4_min_cin", "use_sm", "splitk", "relu", "splitk_finish", "head_sigmoid", "kernel", "kv", "ksplit", "props",
                                          "n_cu", "counters_zero")]
                + [("split_scratch_bytes", C.c_int64)]
                + [(n, C.c_void_p) for n in ("src0", "src1", "dst", "dst_pool", "relu_mask_src", "head_dst", "split_scratch", "weight", "bias", "head_w", "head_b")])


class ConvRouteOut(C.Structure):
    """``struct ph_conv_route_out``: the ConvKernel, its KV_* code, the K slices and the PH_CRP_* property bits."""

    _fields_ = [(n, C.c_int32) for n in ("kernel", "kv", "ksplit", "props")]


AUG_FLIP, AUG_WARP, AUG_UNIFORM, AUG_GAUSS, AUG_CONTRAST, AUG_BRIGHTNESS, AUG_ERASE = 1, 2, 4, 8, 16, 32, 64


class PosehipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"libposehip error {code}: {msg}")
        self.code = code


_lib = None

_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); mirrors include/posehip.h one to one
SIGNATURES = {
    "ph_last_error": (C.c_char_p, []),
    "ph_version": (C.c_int, []),
    "ph_local_peaks_scratch_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ph_op_desc_size": (_i32, []),
    "ph_model_set_option": (C.c_int, [_vp, C.c_char_p, C.c_double]),
    "ph_model_get_option": (C.c_int, [_vp, C.c_char_p, C.POINTER(C.c_double)]),
    "ph_model_create": (_vp, [C.POINTER(OpDesc), _i32, C.POINTER(_vp), C.POINTER(_i64), _i32, _i32, _i32]),
    "ph_model_destroy": (None, [_vp]),
    "ph_model_workspace_bytes": (_i64, [_vp, _i32, _i32, _i32]),
    "ph_model_output_shape": (C.c_int, [_vp, _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i32), C.POINTER(_i32)]),
    "ph_model_forward": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, C.POINTER(_vp), _vp]),
    "ph_model_num_params": (_i64, [_vp]),
    "ph_model_set_params": (C.c_int, [_vp, _vp, _vp]),
    "ph_model_grad_bucket_split": (_i64, [_vp]),
    "ph_model_set_bucket_event": (C.c_int, [_vp, _vp]),
    "ph_comm_available": (C.c_int, []),
    "ph_comm_unique_id": (C.c_int, [_vp]),
    "ph_comm_create": (_vp, [_vp, _i32, _i32]),
    "ph_comm_destroy": (None, [_vp]),
    "ph_comm_world": (_i32, [_vp]),
    "ph_allreduce": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "ph_model_set_comm": (C.c_int, [_vp, _vp, _vp]),
    "ph_model_backward_workspace_bytes": (_i64, [_vp, _i32, _i32, _i32]),
    "ph_model_backward": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_f32), _vp, _i32, _f32,
                                    _i32, _i32, _f32, _vp, _vp, _vp]),
    "ph_model_set_head_loss": (C.c_int, [_vp, _i32, _i32, C.POINTER(_f32), _i32]),
    "ph_model_set_branch_scales": (C.c_int, [_vp, _vp, _i32, _i32]),
    "ph_model_set_input_norm": (C.c_int, [_vp, C.POINTER(_f32), C.POINTER(_f32), _i32]),
    "ph_model_backward_pad_vector": (_i64, [_vp, _i32, _i32, _i32, C.POINTER(_i32)]),
    "ph_model_backward_profile_read": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_double), _i32, C.POINTER(C.c_double)]),
    "ph_model_last_backward_kernels": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "ph_model_last_backward_routes": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "ph_loss_scratch_bytes": (_i64, [_i32, _i32]),
    "ph_loss_bce_dice": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _f32, _vp, _vp, _vp, _i64, _vp]),
    "ph_loss_masked_smooth_l1": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _i64, _vp]),
    "ph_render_seg_targets": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _i64, _vp]),
    "ph_debug_split_plan": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_int64)]),
    "ph_model_debug_allocs": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(_i64), _i32, C.POINTER(_i32)]),
    "ph_debug_gemm_bench": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_float)]),
    "ph_debug_row_wgrad_bench": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "ph_conv_route_case_size": (_i32, []),
    "ph_debug_conv3x3_route": (C.c_int, [C.POINTER(ConvRouteCase), _i32, C.POINTER(ConvRouteOut)]),
    "ph_conv_run_case_size": (_i32, []),
    "ph_debug_conv3x3_run": (C.c_int, [C.POINTER(ConvRunCase)]),
    "ph_gemm_case_size": (_i32, []),
    "ph_debug_gemm_run": (C.c_int, [C.POINTER(GemmCase)]),
    "ph_debug_window_attn_v2_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "ph_debug_window_attn_v2_wide_run": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32]),
    "ph_debug_window_tokens": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i64]),
    "ph_render_confmaps": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "ph_render_pafs": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "ph_render_class_maps": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp]),
    "ph_instance_centroids": (C.c_int, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "ph_adam_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _i32, _f32, _vp]),
    "ph_adamw_step": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i64, _f32, _f32, _f32, _f32, _f32, _i32, _f32, _vp]),
    "ph_model_set_profiling": (C.c_int, [_vp, _i32]),
    "ph_model_profile_read": (C.c_int, [_vp, C.POINTER(C.c_double), _i32, C.POINTER(_i32)]),
    "ph_model_last_kernels": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "ph_model_last_rows_plans": (C.c_int, [_vp, C.POINTER(_i32), _i32]),
    "ph_model_last_ranges": (C.c_int, [_vp, C.POINTER(_i64), _i32, C.POINTER(_i32)]),
    "ph_model_set_clock_probe": (C.c_int, [_vp, _vp]),
    "ph_model_read_slot": (C.c_int, [_vp, _i32, _vp, _i64, _vp]),
    "ph_local_peaks": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _vp, _i64, _vp]),
    "ph_global_peaks": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _vp, _vp]),
    "ph_paf_score": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "ph_crop_bboxes": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ph_resize_bilinear_aa": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "ph_sample_class_maps": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ph_group_class_peaks": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "ph_lsap": (C.c_int, [_vp, _i32, _i32, _vp, _vp]),
    "ph_toposort_edges": (C.c_int, [_vp, _i32, _vp]),
    "ph_centroid_select": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ph_topdown_scatter": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "ph_group_packed": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _f32, C.c_double, _i32, _i32, _i32, _f32, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ph_aug_sample_size": (_i32, []),
    "ph_augment": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ph_tile_extract": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp]),
    "ph_tile_merge": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ph_tile_merge_heads": (C.c_int, [_vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp]),
    "ph_seg_scratch_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ph_seg_center_peaks": (C.c_int, [_vp, _i32, _i32, _i32, _f32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "ph_seg_assign": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp]),
    "ph_seg_gate": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _f32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp]),
    "ph_seg_cleanup_scratch_bytes": (_i64, [_i32, _i32, _i32, _i32, _i32]),
    "ph_seg_cleanup": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i64, _vp]),
    "ph_seg_merge_scratch_bytes": (_i64, [_i32, _i32, _i32, _i32]),
    "ph_seg_merge_tables": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i64, _vp]),
    "ph_seg_semantic_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "ph_seg_semantic": (C.c_int, [_vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _i64, _vp]),
    "ph_seg_place_crops": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "ph_mask_pair_stats": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ph_mask_boundary_scratch_bytes": (_i64, [_i32, _i32, _i32]),
    "ph_mask_boundary": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _i64, _vp]),
    "ph_track_pose_scores": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _i32, C.c_double, _vp]),
    "ph_track_mask_pairs": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
    "ph_track_pose_scores_shifted": (C.c_int, [_vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _i32, C.c_double, _vp]),
    "ph_flow_job_size": (C.c_int, []),
    "ph_flow_levels": (C.c_int, [_i32, _i32, _i32, _i32, _vp]),
    "ph_flow_pyramid": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _i64, _vp]),
    "ph_flow_track": (C.c_int, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.c_double, _vp, _vp, _vp]),
    "ph_group_batch": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, C.c_double, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
}


def lib():
    """Load (once) and return the bound library; raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -m sleap_nn_amd.build` "
            "(hipcc --offload-arch=gfx950). sleap_nn_amd has no CPU fallback."
        )
    # libposehip must share ONE HIP runtime with torch (torch bundles its own libamdhip64 with the
    # same SONAME as /opt/rocm's): load torch's copy first, globally, so the loader binds
    # libposehip's libamdhip64.so.7 dependency to it whatever the import order was.
    import torch

    bundled = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(bundled):
        C.CDLL(bundled, mode=C.RTLD_GLOBAL)
    l = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype = res
        fn.argtypes = args
    if l.ph_op_desc_size() != C.sizeof(OpDesc):
        raise ImportError(f"{LIB_PATH}: struct ph_op_desc is {l.ph_op_desc_size()} bytes, this binding's OpDesc {C.sizeof(OpDesc)}: rebuild the library")
    if l.ph_aug_sample_size() != C.sizeof(AugSample):
        raise ImportError(f"{LIB_PATH}: struct ph_aug_sample is {l.ph_aug_sample_size()} bytes, this binding's AugSample {C.sizeof(AugSample)}: rebuild the library")
    _lib = l
    return l


def check(rc: int) -> int:
    if rc is not None and rc < 0:
        raise PosehipError(int(rc), lib().ph_last_error().decode("utf-8", "replace"))
    return rc


def current_stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_cuda(t, name="tensor"):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live on the GPU (got {t.device}); sleap_nn_amd runs on MI355X only")
    return t
