/*
 * posehip.h -- C ABI of libposehip.so, the MI355X (gfx950) hot path that replaces the
 * ATen/SciPy arithmetic behind sleap-nn's ModelBackend / inference ops seam.
 *
 * Every entry point is `extern "C"`, takes plain pointers + sizes + a hipStream_t passed
 * as void*, returns 0 on success or a negative PH_E_* code (never throws); the text of
 * the last error of the calling thread is available from ph_last_error().
 * Device pointers ("dev") must be HIP device memory of the current device; "host"
 * pointers are ordinary host memory.  The caller owns all inputs and outputs.
 *
 * Which reference interface each group replaces (paths relative to talmolab/sleap-nn):
 *   ph_model_*          sleap_nn/inference/layers/backends/torch_backend.py:113-153
 *                       (TorchBackend.__call__) -> training/lightning_modules.py:1840-1848
 *                       (squeeze + normalize_on_gpu) -> architectures/model.py:237-261
 *                       (Model.forward) -> architectures/unet.py:260-299 and
 *                       encoder_decoder.py:130-141,318-336,522-558,705-730.
 *   ph_local_peaks      inference/ops/peaks.py:184-259 (find_local_peaks[_rough]) with
 *                       ops/crops.py:31-124 + data/instance_cropping.py:129-171.
 *   ph_global_peaks     inference/ops/peaks.py:89-181 (find_global_peaks[_rough]).
 *   ph_paf_score        inference/ops/paf.py:84-497 (get_connection_candidates,
 *                       make_line_subs, get_paf_lines, score_paf_lines[_batch]) and
 *                       inference/utils.py:29-130 (interp1d).
 *   ph_lsap             scipy.optimize.linear_sum_assignment as called at
 *                       inference/ops/paf.py:589.
 *   ph_group_batch      inference/ops/paf.py:500-1149 (match_candidates_*,
 *                       assign_connections_to_instances, make_predicted_instances,
 *                       group_instances_*) + inference/streaming.py:147-255 padding.
 *   ph_toposort_edges   inference/ops/paf.py:890-912.
 *   ph_group_packed     inference/layers/bottomup.py:126-195 (hand-off) + inference/streaming.py:147-255.
 *   ph_centroid_select  inference/layers/centroid.py:195-261 + layers/topdown.py:183-235.
 *   ph_topdown_scatter  inference/layers/topdown.py:236-260.
 *   ph_augment          data/skia_augmentation.py (apply_intensity_augmentation_skia,
 *                       apply_flip_augmentation_skia, apply_geometric_augmentation_skia) as
 *                       called at data/custom_datasets.py:1101-1117.
 *   ph_tile_extract     inference/layers/tiled.py:62-84 (_extract_square_tile, per tile).
 *   ph_tile_merge       inference/tile_merger.py:107-179 (TileMerger.integrate per tile + merge) and the
 *                       crop of inference/layers/tiled.py:262-263.
 *   ph_tile_merge_heads the same stitch for the heads of inference/layers/tiled.py:353-668 in one launch.
 *   ph_loss_* / ph_model_set_head_loss   training/losses.py:64-133 as called at training/lightning_modules.py:3052-3109, 3463-3475.
 *   ph_render_seg_targets   data/segmentation_maps.py as called at data/custom_datasets.py:3593-3626.
 *   ph_seg_place_crops  inference/segmentation_convert.py:74-133 (decode_mask_to_image_res) over the entries that
 *                       inference/layers/topdown_segmentation.py:163-284 emits.
 *   ph_seg_*            inference/segmentation.py:12-237 (find_center_peaks, group_instances_from_offsets) as called
 *                       at inference/layers/segmentation.py:159-266, and the thresholding of :438-503 (semantic).
 *   ph_track_pose_scores   tracking/tracker.py:513-586 (get_scores' loop over instance / candidate pairs) with evaluation.py:644-760
 *                       (compute_oks) and tracking/utils.py:184-252 (compute_iou, compute_euclidean_distance, compute_cosine_sim).
 *   ph_track_mask_pairs    tracking/utils.py:127-244 (get_mask, compute_mask_iou: masks decoded to the image grid by
 *                       inference/segmentation_convert.py:74-133 and ANDed pair by pair), on the device label maps.
 */
#ifndef POSEHIP_H
#define POSEHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PH_VERSION 134

/* error codes */
#define PH_OK 0
#define PH_E_INVALID -1     /* bad argument / unsupported configuration            */
#define PH_E_HIP -2         /* a HIP runtime call failed                           */
#define PH_E_CAPACITY -3    /* caller-provided output capacity too small           */
#define PH_E_INFEASIBLE -4  /* assignment problem has no finite-cost solution      */
#define PH_E_WORKSPACE -5   /* workspace too small                                 */

const char* ph_last_error(void);
int ph_version(void);

/* ------------------------------------------------------------------------------------
 * Network (encoder-decoder forward).  The host describes the network as a flat program of
 * ops over numbered activation slots; weights are handed over in the reference's own
 * state_dict layout (Conv2d: OIHW, ConvTranspose2d: IOHW, fp32, host memory) and are
 * re-packed for the MFMA kernels at creation.
 * ---------------------------------------------------------------------------------- */

enum ph_op_kind {
  PH_OP_INPUT_CONV = 1, /* uint8|float NCHW image -> /255 -> conv kxk "same" + bias + ReLU -> NHWC slot */
  PH_OP_CONV = 2,       /* conv kxk "same" over concat(src0, src1) + bias (+ReLU) -> NHWC slot          */
  PH_OP_POOL = 3,       /* 2x2/2 max pool, zero pad bottom/right when odd (architectures/common.py)     */
  PH_OP_UPSAMPLE = 4,   /* bilinear x2, align_corners=False (encoder_decoder.py:431-435)                */
  PH_OP_CONVT = 5,      /* ConvTranspose2d(k3,s2,p1,op1) + bias [-> folded BatchNorm: * weight2[c] + bias2[c]] (+ReLU | SiLU)
                           (encoder_decoder.py:439-461; the reference's decoder builds it with batch_norm=False, ReLU) */
  PH_OP_HEAD = 6,       /* 1x1 conv + bias (+sigmoid) -> NCHW fp32 output #out_index (heads.py:58-67)   */
  PH_OP_STEM = 7,       /* fused first encoder block: image -> /255 -> conv3x3+ReLU (weight/bias) ->
                           conv3x3+ReLU (weight2/bias2, cout <= 16) -> [full-res NHWC slot dst, if >= 0]
                           -> 2x2 max pool -> NHWC slot dst2.  One launch, the two full-resolution
                           activations never touch HBM unless dst >= 0.                               */
  /* ConvNeXt encoder (architectures/convnext.py:19-130; CNBlock / LayerNorm2d are torchvision's) */
  PH_OP_PATCH_STEM = 8, /* image -> /255 -> Conv2d(k = ksize, stride = cmid, padding 1) + bias -> NHWC slot
                           (convnext.py:73-84; the LayerNorm2d that follows is a PH_OP_LAYERNORM)       */
  PH_OP_DWCONV = 9,     /* depthwise 7x7 "same" conv + bias, weight (C,1,7,7)  (CNBlock.block[0])       */
  PH_OP_LAYERNORM = 10, /* LayerNorm over channels, eps 1e-6 (1e-5 with PH_FLAG_LN_EPS_1EM5), weight/bias = affine (LayerNorm2d, block[2]; the Swin norms) */
  PH_OP_LINEAR = 11,    /* per-pixel Linear(cin0 -> cout), weight (cout, cin0) + bias; PH_FLAG_GELU: erf-GELU
                           epilogue (block[3..4]); PH_FLAG_SCALE_RESIDUAL: dst = weight2[c] * (acc + bias) +
                           src1 (block[5], layer_scale, residual add); PH_FLAG_RESIDUAL: dst = acc + bias + src1;
                           PH_FLAG_RESIDUAL | PH_FLAG_RELU: dst = relu(acc + bias + src1) (the tail of a ResNet bottleneck);
                           bias = -1: Linear(bias=False)                                                 */
  PH_OP_PATCH_CONV = 12, /* Conv2d(k2, s2) + bias, weight (cout, cin0, 2, 2)  (convnext.py:101-110)     */
  /* the two epilogues of PH_OP_LINEAR as ops of their own: the training program keeps the
     pre-activation tensors that autograd needs (GELU input, un-scaled block output)              */
  PH_OP_GELU = 13,      /* dst = GELU_erf(src0)                                                          */
  PH_OP_SCALE_ADD = 14, /* dst = weight[c] * src0 + src1   (layer_scale * block(x) + x)                  */
  PH_OP_GLOBAL_MAXPOOL = 15, /* dst (1x1) = max over H x W of src0 (nn.AdaptiveMaxPool2d(1), heads.py:519-520) */
  /* Swin Transformer encoder (architectures/swint.py; the blocks are torchvision's SwinTransformerBlock / PatchMerging).  Exact fp32 or, under
     "swint_f16", fp16 storage at inference; ph_model_backward runs their backward on the exact-fp32 program (swin_train_kernels.hip). */
  PH_OP_PATCH_MERGE = 16, /* (B, H, W, C) -> (B, ceil(H/2), ceil(W/2), 4C): concat of x[0::2,0::2], x[1::2,0::2], x[0::2,1::2], x[1::2,1::2] (zeros past an odd
                             edge) + LayerNorm over the 4C channels (weight / bias = its affine), one launch; the bias-less PH_OP_LINEAR `reduction` follows.
                             Backward: the gather is rebuilt in scratch, LayerNorm backward over it, scatter to the four phases (the padding receives nothing) */
  PH_OP_WINDOW_ATTN = 17, /* shifted-window multi-head attention core: src0 = qkv slot (B, H, W, 3C) of the un-padded, un-rolled map (q | k | v, head a owns
                             channels 32 a .. 32 a + 31 of each), weight = relative_position_bias_table ((2 ksize - 1)^2, heads), bias = qkv.bias (3C; the q, k, v
                             of a padded token), ksize = window side (2..8), cin1 = heads (cout = 32 heads), cmid = nominal shift (an axis whose padded size the
                             window covers is not shifted).  dst (B, H, W, C) = softmax(q k^T / sqrt(32) + bias [- 100 across the shift's bands]) v at each
                             token's own pixel: pad, roll, window partition, reverse and crop are index arithmetic of the one launch.
                             Backward (window_attn_bwd_kernel): S and P are recomputed from the qkv slot; gradients of the slot, of the table and -- through the
                             padded tokens, whose q, k, v are qkv.bias -- of qkv.bias */
  /* ConvNeXtV2 encoder (HuggingFace ConvNextV2Backbone behind the reference's PretrainedBackbone, architectures/pretrained.py).  Exact fp32.  Its two ops of its own
     (PH_OP_GRN, the PH_FLAG_PAD0_NORM stem) carry PH_FLAG_NO_TRAIN: ph_model_backward runs their steps on a handle whose option pretrained_train is 1
     (convnextv2_train_kernels.hip; the stem's weight gradient is the patch stem's im2col + row-wgrad GEMM over normalised patches) and refuses the program otherwise. */
  PH_OP_GRN = 18,         /* Global Response Normalization over a (B, H, W, C) slot (cin0 = cout = C): G[b,c] = sqrt(sum_hw x^2), N[b,c] = G[b,c] / (mean_c G[b,:] + 1e-6),
                             dst = weight[c] * (x * N[b,c]) + bias[c] + x; weight / bias (1,1,1,C).  Two launches (convnextv2_kernels.hip): grn_reduce_kernel writes
                             per-(sample, pixel slice, channel) sums of squares into the scratch region -- fixed slices, no atomics, so two forwards are bit-identical --
                             and grn_apply_kernel adds the slices in order, takes the channel mean over the C true channels and applies; pad channels come out zero.
                             Backward (T = sum_hw g x, D = mean_c G + 1e-6, dG = w T / D - (sum_c w T G) / (C D^2), K = dG / G where G > 0 else 0):
                             dx = g (1 + w N) + x K, dweight[c] = sum_b T N, dbias[c] = sum_{b,hw} g; the same fixed slices, sums added in slice and sample order */
  /* ResNet encoder (HuggingFace ResNetBackbone behind the reference's PretrainedBackbone).  Exact fp32, inference only: the three ops carry PH_FLAG_NO_TRAIN and
     ph_model_backward refuses them whatever the handle's options.  BatchNorm (eval) never reaches the library: the host folds it into each conv's weight and bias. */
  PH_OP_RESNET_STEM = 19, /* image -> (x / 255 - mean[ci]) / std[ci] (ph_model_set_input_norm) -> Conv2d(k7, s2, p3) + bias + ReLU -> NHWC slot dst (H/2 x W/2)
                             -> MaxPool2d(k3, s2, p1) -> NHWC slot dst2 (H/4 x W/4).  The conv's zero padding applies to the NORMALISED image.  Two launches
                             (resnet_kernels.hip): the im2col product (K = 49 cin) on v_mfma_f32_32x32x2_f32, then the pool.  weight (cout, cin0, 7, 7), cin0 <= 4 */
  PH_OP_CONV_S2 = 20,     /* Conv2d(k = ksize in {1, 3}, stride 2, padding ksize / 2) + bias (+ReLU) over an even-sized map, as a row GEMM whose rows gather their
                             taps at stride 2 (gemm_mfma_dma_tile_kernel mode 4 / mode 6).  weight (cout, cin0, k, k) */
  PH_OP_ADD_RELU = 21,    /* dst = relu(src0 + src1), element-wise over two slots of one shape (cin0 = cout channels): the tail of a ResNet basic block */
  /* Swin Transformer V2 encoder (HuggingFace Swinv2Backbone behind the reference's PretrainedBackbone).  Exact fp32, inference only: its ops of its own -- this one,
     PH_OP_LAYERNORM with PH_FLAG_RESIDUAL, PH_OP_PATCH_MERGE with PH_FLAG_NO_NORM -- carry PH_FLAG_NO_TRAIN and ph_model_backward refuses the program whatever the
     handle's options.  The host hands the library DERIVED tensors for this op and the qkv Linear in front of it (computed in float64 from the checkpoint's parameters). */
  PH_OP_WINDOW_ATTN_V2 = 22 /* cosine window attention core (swin_kernels.hip's cosine variant; swinv2_kernels.hip above window 8): src0 = qkv slot (B, H, W, 3C) as PH_OP_WINDOW_ATTN, weight = 16 sigmoid(continuous
                             position bias) HEAD-MAJOR (heads, (2 ksize - 1)^2), bias = (3C) query.bias | zeros | value.bias (the q, k, v of a padded token: hidden state
                             0, key has no bias), weight2 = (heads) exp(min(logit_scale, log 100)), ksize = window side (2..24; 9..24 run the key-tiled kernel), cin1 = heads (cout = 32 heads), cmid = the
                             layer's shift, applied on both axes whatever the map (HuggingFace rolls and masks a shifted layer even where one window covers the axis).
                             dst = softmax(scale (q / max(|q|, 1e-12)) . (k / max(|k|, 1e-12)) + bias [- 200 across the shift's bands: the installed
                             Swinv2SelfAttention adds its -100 mask twice]) v at each token's own pixel */
};

#define PH_FLAG_RELU 1
#define PH_FLAG_SIGMOID 2
#define PH_FLAG_GELU 4
#define PH_FLAG_SCALE_RESIDUAL 8
#define PH_FLAG_SOFTMAX 16 /* PH_OP_HEAD: softmax over the output channels (ClassVectorsHead, heads.py:536-537) */
#define PH_FLAG_SILU 32    /* PH_OP_CONVT: SiLU instead of ReLU (the activation is an epilogue parameter of the phase GEMMs) */
#define PH_FLAG_NO_TRAIN 64 /* PH_OP_HEAD: a head of the segmentation model types, which neither MSE nor cross entropy trains; the forward ignores it,
                               ph_model_backward refuses the program unless ph_model_set_head_loss chose the head's loss on this handle.
                               PH_OP_GRN / PH_OP_PATCH_STEM with PH_FLAG_PAD0_NORM: refused unless the handle option pretrained_train is 1.
                               PH_OP_RESNET_STEM / PH_OP_CONV_S2 / PH_OP_ADD_RELU (a ResNet program): always refused, they have no backward step.
                               PH_OP_WINDOW_ATTN_V2, PH_OP_LAYERNORM with PH_FLAG_RESIDUAL, PH_OP_PATCH_MERGE with PH_FLAG_NO_NORM (a Swinv2 program): always refused */
#define PH_FLAG_LN_EPS_1EM5 128 /* PH_OP_LAYERNORM / PH_OP_PATCH_MERGE: eps 1e-5 (nn.LayerNorm's default: the Swin norms) instead of 1e-6 */
#define PH_FLAG_RESIDUAL 256    /* PH_OP_LINEAR: dst = acc + bias + src1 (a residual add without a layer scale: Swin's attn.proj and mlp.3; ConvNeXtV2's pwconv2).
                                   PH_OP_LAYERNORM: dst = src1 + LayerNorm(src0) (Swinv2 norms after each branch; src1 and dst are distinct slots; exact fp32 only) */
#define PH_FLAG_PAD0_NORM 512   /* PH_OP_PATCH_STEM: padding 0 instead of 1 and the input is (x / 255 - mean[ci]) / std[ci] with the handle's input statistics
                                   (ph_model_set_input_norm; 0 and 1 until set): HuggingFace's ConvNextV2Embeddings behind PretrainedBackbone._normalize */
#define PH_FLAG_NO_NORM 1024    /* PH_OP_PATCH_MERGE: the four-phase gather alone, no LayerNorm and no weight / bias (Swinv2 norms behind the reduction); exact fp32 only */

typedef struct ph_op_desc {
  int32_t kind;      /* enum ph_op_kind                                              */
  int32_t src0;      /* input slot (-1 = the network input image)                    */
  int32_t src1;      /* second concat source slot or -1                              */
  int32_t dst;       /* output slot (PH_OP_HEAD: ignored)                            */
  int32_t cin0;      /* logical channels of src0                                     */
  int32_t cin1;      /* logical channels of src1 (0 if none)                         */
  int32_t cout;      /* logical output channels                                      */
  int32_t ksize;     /* kernel size (PH_OP_CONV / INPUT_CONV: odd, <= 7)             */
  int32_t flags;     /* PH_FLAG_*                                                    */
  int32_t weight;    /* index into the weights[] array of ph_model_create, or -1     */
  int32_t bias;      /* index into the weights[] array, or -1 (PH_OP_LINEAR: -1 = Linear(bias=False)) */
  int32_t out_index; /* PH_OP_HEAD: which output pointer receives the result         */
  int32_t dst2;      /* PH_OP_STEM: pooled output slot; PH_OP_CONV (ReLU): optional fused 2x2 max-pool slot, -1 = none */
  int32_t weight2;   /* PH_OP_STEM: second conv weight index; PH_OP_LINEAR: layer_scale index; PH_OP_CONVT: folded-BN scale or -1 */
  int32_t bias2;     /* PH_OP_STEM: second conv bias index; PH_OP_CONVT: folded-BN shift or -1 */
  int32_t cmid;      /* PH_OP_STEM: channels between the two convs (<= 16); PH_OP_PATCH_STEM: stride; PH_OP_WINDOW_ATTN: nominal shift */
} ph_op_desc;

/* sizeof(ph_op_desc) as the library was compiled: a binding checks its own struct against it
 * before handing arrays to ph_model_create (16 int32 fields = 64 bytes in PH_VERSION 101). */
int32_t ph_op_desc_size(void);

typedef struct ph_model ph_model;

/* Create a model on the current HIP device.  `weights[i]` are host fp32 arrays (layouts
 * above); they are copied, the caller may free them afterwards.  Returns NULL on error. */
ph_model* ph_model_create(const ph_op_desc* ops, int32_t n_ops, const float* const* weights,
                          const int64_t* weight_numel, int32_t n_weights, int32_t n_slots,
                          int32_t n_outputs);
void ph_model_destroy(ph_model* m);

/* Bytes of device workspace ph_model_forward needs for a (B, C, H, W) input. */
int64_t ph_model_workspace_bytes(const ph_model* m, int32_t batch, int32_t height, int32_t width);

/* Shape of output #i for an (H, W) input: writes channels/height/width. */
int ph_model_output_shape(const ph_model* m, int32_t out_index, int32_t height, int32_t width,
                          int32_t* c, int32_t* h, int32_t* w);

/* Forward.  input_dev: (B, C, H, W) NCHW, dtype 0 = uint8 (divided by 255),
 * 1 = float32 already in [0,1], 2 = float32 in [0,255] (divided by 255)
 * (data/normalization.py:7-35; the data-dependent max()>1 test is resolved by the caller).
 * out_dev[i]: (B, c_i, h_i, w_i) NCHW fp32.  Everything is enqueued on `stream`. */
int ph_model_forward(ph_model* m, const void* input_dev, int32_t in_dtype, int32_t batch,
                     int32_t in_channels, int32_t height, int32_t width, void* workspace_dev,
                     int64_t workspace_bytes, float* const* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Training step pieces (forward = ph_model_forward on the UNFUSED program with bilinear
 * up-sampling; reference: training/lightning_modules.py:1850-1922, training/losses.py:8-63,
 * torch.optim.Adam as configured at lightning_modules.py:752-763).
 * The "canonical parameter arena" is weights[] of ph_model_create concatenated in order
 * (each in the reference's state_dict layout), fp32, on the device.
 * ---------------------------------------------------------------------------------- */
int64_t ph_model_num_params(const ph_model* m);

/* Rebuild every packed weight buffer of the model from the canonical arena (device gather). */
int ph_model_set_params(ph_model* m, const float* params_flat_dev, void* stream);

int64_t ph_model_backward_workspace_bytes(const ph_model* m, int32_t batch, int32_t height, int32_t width);

/* Loss + backward of the last ph_model_forward (same input, shapes and activation workspace).
 *   head_out_dev[i] / target_dev[i]: (B, c_i, h_i, w_i) NCHW fp32 predictions and targets.
 *   loss = sum_i loss_weights[i] * (MSE_i [+ OHKM_i]);  loss_dev: float[1 + n_outputs] = {total, per head}.
 *   sample_weights_dev: NULL (plain nn.MSELoss) or float[B] on the device: MSE_i becomes mean_b(w_b * mean_chw(diff^2)),
 *   the negative-sample weighting of training/lightning_modules.py:526-545 (w_b = negative_loss_weight for negative
 *   frames, 1 otherwise; train stage only -- the caller passes NULL for validation).  OHKM is not weighted (as there).
 *   grads_flat_dev: d loss / d params in the canonical arena layout (every entry is written).
 * Deterministic (fixed-order reductions, no float atomics). */
int ph_model_backward(ph_model* m, const void* input_dev, int32_t in_dtype, int32_t batch, int32_t in_channels,
                      int32_t height, int32_t width, const void* act_workspace_dev, void* grad_workspace_dev,
                      int64_t grad_workspace_bytes, const float* const* head_out_dev, const float* const* target_dev,
                      const float* loss_weights_host, const float* sample_weights_dev, int32_t ohkm_enabled, float hard_to_easy_ratio,
                      int32_t min_hard_keypoints, int32_t max_hard_keypoints, float ohkm_loss_scale,
                      float* loss_dev, float* grads_flat_dev, void* stream);

/* Loss of output `out_index` in ph_model_backward, chosen per handle before a step (reference: training/lightning_modules.py:3052-3109, 3463-3475).
 *   PH_LOSS_MSE               nn.MSELoss; on a PH_FLAG_NO_TRAIN head (the instance-centre map) without OHKM and sample weights.  n_params = 0.
 *   PH_LOSS_BCE_DICE          compute_bce_dice_loss (training/losses.py:64-105) on a one-channel head; params = {bce_weight, dice_weight, smooth,
 *                             pos_weight (negative: none)}, n_params = 4.  In the plans a backward can follow (exact fp32, every activation kept) the head
 *                             then emits LOGITS -- its PH_FLAG_SIGMOID epilogue is skipped -- and head_out_dev[out_index] of ph_model_backward is those
 *                             logits; inference plans still return probabilities.  Set it before the forward of the step.
 *   PH_LOSS_MASKED_SMOOTH_L1  compute_masked_smooth_l1 (losses.py:108-133); target_dev[out_index] is (B, c + 1, h, w): the c target channels, then the
 *                             binary weight mask.  n_params = 0.
 * A head whose loss was set is no longer refused for PH_FLAG_NO_TRAIN; a handle on which nothing was set behaves as before. */
#define PH_LOSS_MSE 1
#define PH_LOSS_BCE_DICE 2
#define PH_LOSS_MASKED_SMOOTH_L1 3
int ph_model_set_head_loss(ph_model* m, int32_t out_index, int32_t kind, const float* params, int32_t n_params);

/* Per-sample scales of the residual branches (stochastic depth as torchvision's StochasticDepth(p, "row") applies it in train mode: bernoulli(1 - p) / (1 - p)
 * per sample).  scales_dev: device float[n_branches][batch], borrowed until the ph_model_backward of the step has been enqueued; NULL clears it.
 * n_branches must equal the number of PH_OP_LINEAR ops with PH_FLAG_RESIDUAL, which the rows follow in program order.  While set, the i-th such op computes
 * dst = s[i][b] * (acc + bias) + src1 in ph_model_forward (the row GEMM without its residual, then one element-wise pass), and ph_model_backward feeds
 * s[i][b] * G(dst) to its weight, bias and data gradients and the plain G(dst) to src1.  A forward or backward whose batch differs from `batch`, or a forward
 * in a non-fp32 format, is refused while scales are set.  With none set the launch sequence is what it is without this call. */
int ph_model_set_branch_scales(ph_model* m, const float* scales_dev, int32_t n_branches, int32_t batch);
/* Per-channel input statistics of a PH_OP_PATCH_STEM with PH_FLAG_PAD0_NORM (host arrays of n <= 4 floats, copied; std must be non-zero).  They are the
 * checkpoint's image_mean / image_std buffers, not parameters: nothing in the parameter arena maps onto them. */
int ph_model_set_input_norm(ph_model* m, const float* mean, const float* std, int32_t n);
/* Byte offset, in the gradient workspace of a (batch, height, width) step, of the (3C) vector that holds the padded tokens' share of a qkv.bias gradient
 * (sum of dq | dk | dv over the padded tokens of the windows) between the attention op's step and the qkv Linear's; after ph_model_backward it holds that
 * of the program's FIRST attention op, *n_floats = its 3C.  For tests and tools. */
int64_t ph_model_backward_pad_vector(const ph_model* m, int32_t batch, int32_t height, int32_t width, int32_t* n_floats);

/* The two losses on their own (deterministic: fixed-order partial sums, no float atomics; three launches on `stream`, no host synchronisation).
 *   ph_loss_bce_dice: logits / target (B, 1, h, w) fp32, target values in {0, 1}.  BCE = binary_cross_entropy_with_logits (mean, optional pos_weight:
 *     negative = none) in its stable form; Dice per sample (2 sum(p t) + smooth) / (sum p + sum t + smooth), loss = bce_weight * BCE +
 *     dice_weight * (1 - mean_b dice_b).  loss_dev[0] = the loss, grad_dev (B, 1, h, w) = loss_weight * d loss / d logit.
 *   ph_loss_masked_smooth_l1: pred / target (B, C, h, w), mask (B, 1, h, w) binary, broadcast over C.  loss = sum smooth_l1(mask * pred, mask * target;
 *     beta 1) / (C * sum mask), exactly 0 with an all-zero gradient when the mask is empty.  grad_dev (B, C, h, w) = loss_weight * d loss / d pred.
 *   scratch_dev: ph_loss_scratch_bytes(B, C) bytes (covers both), 8-byte aligned. */
int64_t ph_loss_scratch_bytes(int32_t B, int32_t C);
int ph_loss_bce_dice(const float* logits_dev, const float* target_dev, int32_t B, int32_t h, int32_t w, float bce_weight, float dice_weight, float smooth,
                     float pos_weight, float loss_weight, float* loss_dev, float* grad_dev, void* scratch_dev, int64_t scratch_bytes, void* stream);
int ph_loss_masked_smooth_l1(const float* pred_dev, const float* target_dev, const float* mask_dev, int32_t B, int32_t C, int32_t h, int32_t w,
                             float loss_weight, float* loss_dev, float* grad_dev, void* scratch_dev, int64_t scratch_bytes, void* stream);

/* Two gradient buckets for overlapping the data-parallel all-reduce with the backward sweep (DDP's bucketing,
 * training/model_trainer.py:1751-1813 runs the reference under Lightning's DDP strategy).  The sweep runs heads -> decoder ->
 * middle -> encoder and the arena is in program order, so its tail becomes final first: ph_model_grad_bucket_split returns the
 * offset B (closest to the middle at which the arena splits cleanly between two ops; n_params if it never does), and an event
 * handed to ph_model_set_bucket_event (a hipEvent_t; NULL = off) is recorded on the backward's stream as soon as every gradient
 * in [B, n_params) is final -- a collective on another stream can wait on it while the rest of the backward still runs. */
int64_t ph_model_grad_bucket_split(const ph_model* m);
int ph_model_set_bucket_event(ph_model* m, void* hip_event);

/* ------------------------------------------------------------------------------------
 * Data-parallel gradient exchange over RCCL (what Lightning's DDP strategy does for the reference: training/model_trainer.py:1751-1813,
 * docs/guides/multi-gpu.md:67-81).  One process per GPU.  librccl is opened at run time (dlopen): ph_comm_available() says whether it could be.
 *   ph_comm_unique_id   rank 0 draws 128 opaque bytes (ncclGetUniqueId) and hands them to every rank over the host language's own channel
 *   ph_comm_create      collective over the ranks, on the CURRENT HIP device (ncclCommInitRank); NULL + ph_last_error() on failure
 *   ph_allreduce        in-place SUM of `count` floats over the ranks, enqueued on `stream`
 *   ph_model_set_comm   ph_model_backward then exchanges the gradient arena itself: the tail bucket [ph_model_grad_bucket_split, n_params) on
 *                       `comm_stream` as soon as the sweep has finished it, the head bucket behind the sweep; the stream ph_model_backward runs on
 *                       waits for both, so the ph_adam_step enqueued next (grad_scale = 1 / world: DDP's mean) reads the sum.  comm = NULL: off.
 * ---------------------------------------------------------------------------------- */
typedef struct ph_comm ph_comm;
int ph_comm_available(void);
int ph_comm_unique_id(void* out_id128);
ph_comm* ph_comm_create(const void* id128, int32_t world, int32_t rank);
void ph_comm_destroy(ph_comm* comm);
int32_t ph_comm_world(const ph_comm* comm);
int ph_allreduce(ph_comm* comm, float* buf_dev, int64_t count, void* stream);
int ph_model_set_comm(ph_model* m, ph_comm* comm, void* comm_stream);

/* torch.optim.Adam step (weight_decay = 0) on flat device arrays; max_exp_avg_sq_dev != NULL enables
 * amsgrad.  grad_scale multiplies the gradient first (1/world_size after a sum all-reduce). */
int ph_adam_step(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                 float* max_exp_avg_sq_dev, int64_t n, float lr, float beta1, float beta2, float eps,
                 int32_t step, float grad_scale, void* stream);
/* torch.optim.AdamW step (the reference's other optimizer choice, lightning_modules.py:752-755): decoupled weight decay
 * param *= 1 - lr * weight_decay, then the Adam update above (torch's default weight_decay is 0.01). */
int ph_adamw_step(float* params_dev, const float* grads_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                  float* max_exp_avg_sq_dev, int64_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int32_t step, float grad_scale, void* stream);

/* On-device rendering of the training targets (reference: data/confidence_maps.py:96-166
 * generate_multiconfmaps; data/edge_maps.py:15-78,120-220,250-323 generate_pafs).
 * points_dev: (B, I, N, 2) fp32 (x, y) image coordinates, NaN = missing.  Grids are
 * arange(0, size, stride).  Confmaps: (B, N, h, w), Gaussian sigma*stride, max over instances.
 * PAFs: (B, 2E, h, w) channel 2e = x, 2e+1 = y, summed over instances; edges_dev int32 (E, 2). */
int ph_render_confmaps(const float* points_dev, int32_t B, int32_t I, int32_t N, int32_t img_h, int32_t img_w,
                       int32_t stride, float sigma, float* out_dev, void* stream);
int ph_render_pafs(const float* points_dev, const int32_t* edges_dev, int32_t B, int32_t I, int32_t N, int32_t E,
                   int32_t img_h, int32_t img_w, int32_t stride, float sigma, float* out_dev, void* stream);

/* Identity class maps of a batch in one launch (reference: data/identity.py:34-137 generate_class_maps).
 * points_dev: (B, I, N, 2) fp32, NaN = missing; weights_dev: (B, C, I) fp32 class weights (0 / 1: the one-hot class vectors
 * in the layout the caller's reshape gives them).  Per grid point: M_i = max over nodes of exp(-d^2 / (2 (sigma*stride)^2))
 * (NaN -> 0), S = sum_i M_i, mask_i = M_i / S where M_i > threshold else 0, out[c] = max_i weights[c][i] * mask_i (0 for I = 0).
 * out_dev: (B, C, h, w) fp32, h = ceil(img_h / stride).  threshold >= 0; a frame's points and weights must fit 64 KiB. */
int ph_render_class_maps(const float* points_dev, const float* weights_dev, int32_t B, int32_t I, int32_t N, int32_t C,
                         int32_t img_h, int32_t img_w, int32_t stride, float sigma, float threshold, float* out_dev,
                         void* stream);
/* Instance centroids (reference: data/instance_centroids.py:7-98 generate_centroids).  points_dev: (n, N, 2) fp32; out_dev: (n, 2).
 * The anchor node when anchor_ind >= 0 and both its coordinates are present; else the NaN-ignoring mean, counted per axis;
 * NaN when no node has a coordinate.  anchor_ind < 0: always the mean. */
int ph_instance_centroids(const float* points_dev, int64_t n, int32_t N, int32_t anchor_ind, float* out_dev, void* stream);

/* Targets of the segmentation model types from instance masks (reference: data/segmentation_maps.py).  masks_dev: (B, I, H, W) uint8, non-zero =
 * foreground, of the image's size; n_instances_dev int32[B]: slots at or beyond n_instances[b] are padding and are never read as masks (a real, empty mask
 * is different: its centroid is the image centre and it does get a Gaussian).  Output grids are (H / s, W / s) (integer division), cell i of an axis
 * covering the rows [floor(i H / out), ceil((i + 1) H / out)) -- the windows of adaptive_avg_pool2d, which is what F.interpolate(mode="area") runs.
 *   centroids_dev float (B, I, 2) = (x, y), areas_dev int64 (B, I): with compute_stats != 0 they are computed first (exact 64-bit sums of x, y and the
 *     pixel count, one fp64 division each, rounded to fp32; (W / 2, H / 2) for an empty mask; NaN / 0 in padding slots); with compute_stats == 0 they are
 *     inputs, e.g. what a call for another head's stride has written.  Both are required.
 *   fg_dev (B, 1, h, w) or NULL: 1 where more than half of the window's pixels lie in the union of the masks (2 count > window; exactly half is
 *     background), with maxpool != 0 where any does.
 *   center_dev (B, 1, h, w) or NULL: max over the instances of exp(-((x - cx)^2 + (y - cy)^2) / (2 (sigma s)^2)) on the grid i s + s / 2.
 *   offsets_dev (B, 2, h, w) / weight_dev (B, 1, h, w), both or neither: among the instances that cover more than half of the cell's window, the one with
 *     the smallest area wins (equal areas: the higher index); offsets = (cx - x, cy - y), weight 1; zeros elsewhere.  Their batch strides are given in
 *     floats, so both may be channel ranges of one (B, 3, h, w) tensor (what PH_LOSS_MASKED_SMOOTH_L1 takes as its target). */
int ph_render_seg_targets(const uint8_t* masks_dev, const int32_t* n_instances_dev, int32_t B, int32_t I, int32_t H, int32_t W, int32_t output_stride,
                          float sigma, int32_t maxpool, int32_t compute_stats, float* centroids_dev, int64_t* areas_dev, float* fg_dev, float* center_dev,
                          float* offsets_dev, int64_t offsets_batch_stride, float* weight_dev, int64_t weight_batch_stride, void* stream);

/* Diagnostic / test hook (pure host arithmetic, no GPU needed): the split-K plan the 3x3 kernels would take for a layer of this shape on a chip of n_cu CUs
 * under handle option conv_splitk = splitk (padded channel counts; section 4.1d of DESIGN.md).  out[0] = K slices on the F(2x2,3x3) kernel, out[1] = on the
 * F(4x4,3x3) kernel (1 = no split), out[2], out[3] = KiB of partial-sum scratch each would need (0 when it does not split). */
int ph_debug_split_plan(int32_t B, int32_t H, int32_t W, int32_t cin_padded, int32_t cout_padded, int32_t splitk, int32_t n_cu, int64_t* out4);

/* Diagnostic / test hook (pure host arithmetic, no GPU needed): the route of one exact-fp32 3x3 conv launch on a chip of n_cu CUs (csrc/conv3x3_route.h, DESIGN.md
 * "Routing of the exact-fp32 3x3 conv").  The case is turned into launch arguments with dummy non-null pointers where a bit says the pointer exists; nothing is launched.
 *   c0p, c1p, coutp, bn, B, H, W   padded channel counts, N tile (32 / 64), map
 *   forms        PH_CRF_*: the weight forms that exist        flags   PH_CRA_*: the arguments of the launch (head_cout / head_wcp with PH_CRA_HEAD)
 *   use_dma ... splitk   the option fields of the launch arguments, as the runtime fills them from the handle's options and the kind of plan
 *   ptr_salt     varies the dummy pointers (the route may not depend on their values)
 *   split_scratch_bytes   0 = the plan reserved no split-K scratch
 * out: kernel = the ConvKernel (0 register-staged, 1 9-tap LDS-DMA, 2 F(2,3), 3 conv3x3_c16, 4 wave-private F(2x2,3x3), 5 wave-split F(2x2,3x3), 6 F(4x4,3x3), 7 small-map),
 * kv = its PH_KV_* code, ksplit = K slices, props = PH_CRP_* bits. */
#define PH_CRF_DMA 1
#define PH_CRF_WINO 2
#define PH_CRF_WINO2 4
#define PH_CRF_W16 8
#define PH_CRF_C16 16
#define PH_CRF_WINO4 32
#define PH_CRF_SM 64
#define PH_CRA_SRC1 1
#define PH_CRA_SRC1_LOWRES 2
#define PH_CRA_POOL 4
#define PH_CRA_SKIP_DST 8
#define PH_CRA_ACCUMULATE 16
#define PH_CRA_RELU_MASK 32
#define PH_CRA_HEAD 64
#define PH_CRP_MASK 1      /* stores plainly: applies a ReLU mask                      */
#define PH_CRP_POOLS 2     /* writes the fused 2x2 max pool from its Winograd tiles    */
#define PH_CRP_HEAD_W2D 4  /* may carry a 1x1 head: wave-split form                    */
#define PH_CRP_HEAD_W16 8  /* ... wave-private form                                    */
#define PH_CRP_LOWRES 16   /* folds a half-resolution second source                    */
#define PH_CRP_HEAD_SM 32  /* may carry a 1x1 head: small-map form                     */
typedef struct ph_conv_route_case {
  int32_t c0p, c1p, coutp, bn, B, H, W;
  int32_t forms, flags, head_cout, head_wcp;
  int32_t use_dma, dma32, use_wino, persist, use_c16, use_w16, use_wino2d, use_wino4, wino4_min_cin, use_sm, splitk;
  int32_t ptr_salt;
  int64_t split_scratch_bytes;
} ph_conv_route_case;
typedef struct ph_conv_route_out {
  int32_t kernel, kv, ksplit, props;
} ph_conv_route_out;
int32_t ph_conv_route_case_size(void);
int ph_debug_conv3x3_route(const ph_conv_route_case* c, int32_t n_cu, ph_conv_route_out* out);

/* Diagnostic / test hook: every device allocation the handle owns, in the order it was made (ph_model_create's packed weights, gather maps and derived forms,
 * then whatever later calls added: the lazy fp16 packs of the first fp16 forward, the tables of the first ph_model_set_params).  *n_rows = the number of
 * allocations; the first min(max_rows, *n_rows) rows of ptrs[] / bytes[] are filled with the device pointer and the size of the allocation as the runtime
 * reports it (max_rows = 0 only counts).  The pointers stay the handle's: read them, never free or write them. */
int ph_model_debug_allocs(const ph_model* m, void** ptrs, int64_t* bytes, int32_t max_rows, int32_t* n_rows);

/* Diagnostic (tools/gemm_bench.py): average milliseconds of one row-GEMM kernel variant on synthetic operands. */
int ph_debug_gemm_bench(int32_t variant, int32_t M, int32_t K, int32_t N, int32_t mode, int32_t H, int32_t W,
                        int32_t act, int32_t iters, float* ms_out);

/* Test support (tests/test_gpu_row_gemm.py), not a product path: ONE launch of the row GEMM (gemm_mfma_dma_kernel / gemm_mfma_dma_tile_kernel) on
 * operands the caller owns, synchronised before it returns.  The host arrays go through the product's own packers; launch checks come back as error codes.
 *   variant      0..4 = that tile variant (256x128, 256x96, 256x64, 256x32, 128x128; the pack's N tile must be the variant's), -1 = the library's own choice
 *   mode ...     as the forward / backward routines set them: mode 0 Linear, 1 Conv2d k2 s2, 2 Conv2d 3x3 "same", 3 ConvTranspose2d(k3, s2, p1, op1) phase(s),
 *                4 Conv2d 3x3 s2 p1, 5 Conv2d k x k "same", 6 Conv2d 1x1 at tap_stride with the residual before the activation.  M = output rows (modes 1, 4, 6:
 *                pixels of the strided grid; mode 3: input pixels), H x W = the INPUT map.  act: 0 none, 1 ReLU, 2 GELU, 3 times GELU'(aux), 4 SiLU.
 *   cin0, cin1, cout   true channel counts; every device tensor is NHWC with its channels padded to a multiple of 16 (pad channels of the sources: zeros)
 *   bn           N tile of the weight pack (128, 96, 64, 32) or 0 = the one the library chooses for pad16(cout)
 *   variant_used, bn_used   written by the call
 *   src0, src1, residual, aux, dst, dst_pre, sumsq   device pointers; all but src0 and dst may be NULL where the mode allows
 *   weight       host, canonical: (cout, cin0 + cin1, taps) -- taps = 1, 4 (ky, kx), 9 or k^2 (ky, kx) -- and for mode 3 the ConvTranspose2d weight (cin0, cout, 3, 3)
 *                (all_phases: the four phases in one launch; else phase out_tap = 2 (oy & 1) + (ox & 1))
 *   bias, scale, shift   host, cout floats; scale and shift may be NULL */
typedef struct ph_gemm_case {
  int32_t variant, mode, M, H, W, ksize, tap_stride, out_patch, out_tap, out_H, out_W, all_phases, act, affine_first, late_split, persist2, sq_hw, sq_nseg;
  int32_t cin0, cin1, cout, bn;
  int32_t variant_used, bn_used;
  const float *src0, *src1, *residual, *aux;
  float *dst, *dst_pre, *sumsq;
  const float *weight, *bias, *scale, *shift;
} ph_gemm_case;
int32_t ph_gemm_case_size(void);
int ph_debug_gemm_run(ph_gemm_case* c);

/* Test support (tests/test_gpu_conv3x3.py), not a product path: ONE routed launch of the exact-fp32 3x3 conv on tensors the caller owns, synchronised before it returns.
 * The canonical weight and bias go through the product's own packers and device derivations (the forms named in `forms`, PH_CRF_*, built as ph_model_create builds
 * them); the kernel is chosen by conv3x3_route on the device's CU count and launched by launch_conv3x3_routed: a case steers the route through the option fields only.
 * Launch checks come back as error codes; whatever the call allocates is freed on every way out.
 *   cin0, cin1, cout   true channel counts; every device tensor is NHWC fp32 with its channels padded to a multiple of 16 (pad channels of the sources: zeros)
 *   bn           N tile of the packing: 64 from 64 padded output channels on, 32 below -- or 64 with 32 padded output channels and K >= 64 (the half-empty-tile packing)
 *   flags        PH_CRA_*; each pointer bit must agree with its pointer (src1, dst_pool, relu_mask_src, head_w).  PH_CRA_SRC1_LOWRES: src1 is (B, H/2, W/2, c1p)
 *   use_dma ... splitk, split_scratch_bytes   as ph_conv_route_case; split_scratch_bytes > 0 needs split_scratch
 *   relu, splitk_finish, head_cout, head_sigmoid   ConvArgs' fields of those names (the head's weight rows are padded to pad16(cout) channels)
 *   src0, src1, dst, dst_pool, relu_mask_src, head_dst, split_scratch   device pointers; head_dst is NCHW (B, head_cout, H, W)
 *   weight (cout, cin0 + cin1, 3, 3), bias (cout), head_w (head_cout, cout), head_b (head_cout)   host, canonical
 * written by the call: kernel, kv, ksplit, props as ph_conv_route_out; n_cu = the CU count the route was asked with; counters_zero = 1 when the split-K counters the
 * call owns (zeroed, of the size a model handle holds; handed to the launch only where splitk_finish != 0) are all zero again after the launch. */
typedef struct ph_conv_run_case {
  int32_t cin0, cin1, cout, bn, B, H, W;
  int32_t forms, flags, head_cout;
  int32_t use_dma, dma32, use_wino, persist, use_c16, use_w16, use_wino2d, use_wino4, wino4_min_cin, use_sm, splitk;
  int32_t relu, splitk_finish, head_sigmoid;
  int32_t kernel, kv, ksplit, props, n_cu, counters_zero;
  int64_t split_scratch_bytes;
  const float *src0, *src1;
  float *dst, *dst_pool;
  const float* relu_mask_src;
  float *head_dst, *split_scratch;
  const float *weight, *bias, *head_w, *head_b;
} ph_conv_run_case;
int32_t ph_conv_run_case_size(void);
int ph_debug_conv3x3_run(ph_conv_run_case* c);

/* Test support (tests/test_gpu_window_attn_v2.py), not a product path: ONE launch of the cosine window attention (window_attn_kernel, cosine variant) on tensors the caller owns,
 * synchronised before it returns.  All pointers are device pointers: qkv (B, H, W, 96 heads) = query | key | value of the map, qkv_bias (96 heads) = what a padded token's
 * q, k, v are (its key section is zeros in the product), scale (heads), table (heads, (2 w - 1)^2), dst (B, H, W, 32 heads).  shift applies on both axes. */
int ph_debug_window_attn_v2_run(const float* qkv, const float* qkv_bias, const float* scale, const float* table, float* dst, int32_t B, int32_t H, int32_t W, int32_t heads,
                                int32_t w, int32_t shift);
/* Test support (tests/test_gpu_window_attn_v2_wide.py): the same on the key-tiled kernel (window_attn_v2_wide_kernel), for windows of 2..24.  The product path sends that
 * kernel windows of 9..24 only; here 2..8 run on it too. */
int ph_debug_window_attn_v2_wide_run(const float* qkv, const float* qkv_bias, const float* scale, const float* table, float* dst, int32_t B, int32_t H, int32_t W,
                                     int32_t heads, int32_t w, int32_t shift);

/* Test support (tests/test_window_geometry_cpu.py), host code only (no GPU needed): the token map of a window-attention launch on a (B, H, W) map with windows of side w
 * (2..24) and shifts sh, sw < w, computed by the functions the kernels call (csrc/window_attn.h).  pix_out / code_out: host arrays of `capacity` int32 each, filled as
 * [window][w * w] with the windows in the kernels' order (b, wy, wx): pix = (b H + y) W + x of the token's pixel or -1 for a padded token,
 * code = ty | tx << code_bits | band << 2 code_bits (code_bits 4: w <= 16, the one-wave kernels' form; 5: the key-tiled kernel's); two tokens of a window are masked
 * against each other where their bands differ. */
int ph_debug_window_tokens(int32_t B, int32_t H, int32_t W, int32_t w, int32_t sh, int32_t sw, int32_t code_bits, int32_t* pix_out, int32_t* code_out, int64_t capacity);

/* Diagnostic (tools/row_wgrad_bench.py): average milliseconds of the row weight-gradient GEMM dW[n][k] = sum_m dY[m][n] X[m][k]
 * (Linear layers of the training step, train_kernels.h launch_row_wgrad) on synthetic operands, and the largest error of 64
 * sampled entries against a float64 sum on the host, relative to the largest of them. */
int ph_debug_row_wgrad_bench(int32_t M, int32_t n, int32_t k, int32_t iters, float* ms_out, float* max_rel_err_out);

/* Per-handle options (the library reads no environment variables and keeps no process-global
 * tunables).  Every key selects between kernel variants that compute the same result; defaults
 * are the measured-best ones.  Keys: "conv_wino" (1 Winograd F(2,3) 3x3 kernels | 2 only the
 * N-tile-64 layers | 0 direct 9-tap kernels), "stem_wino", "dgrad_wino" (0: direct kernels for the backward's data-gradient convs), "conv_dma", "conv_dma32",
 * "conv_persist", "conv_c16", "conv_dma_stagger", "fuse_gelu_fwd", "fuse_gelu_bwd", "wgrad_rows", "convt_phase", "workspace_reuse" (1: activation slots of an inference forward share memory by lifetime),
 * "conv_precision" (0 exact fp32 MFMA | 1 split-fp16 MFMA, 22-bit products | 2 plain fp16, the reference's autocast mode),
 * "convnext_f16" (1: under "conv_precision" 2 a program with ConvNeXt encoder ops runs whole on fp16 activations -- patch stem, depthwise 7x7 + LayerNorm,
 * Linear / 2x2-stride-2 convs as fp16 MFMA row GEMMs, then the fp16 decoder; 0, the default: such a program runs exact fp32 under every precision),
 * "swint_f16" (1: under "conv_precision" 2 a program with the Swin ops runs whole on fp16 activations -- patch stem, LayerNorms, qkv / proj / MLP / reduction Linears as
 * fp16 MFMA row GEMMs, window attention on the fp16 matrix pipe with fp32 logits, patch-merge norm, then the fp16 decoder; 0, the default: exact fp32 under every precision;
 * independent of "convnext_f16"),
 * "gemm_late_split", "gemm_persist2", "conv_gemm_fill", "conv_gemm_fill_wino", "conv_gemm_fill_wino2d",
 * "conv_wino2d" / "conv_w16" (the Winograd F(2x2,3x3) kernels), "conv_wino4" (K-heavy 3x3 convs on the Winograd F(4x4,3x3) kernel: 1 inference
 * plans | 2 every plan | 0 never), "conv_wino4_min_cin", "upsample_fold" (a bilinear x2 read only by the next conv's second source rides in that kernel's input transform), "head_fuse" (a 1x1 head computed in its producer conv's epilogue),
 * "conv_splitk" / "conv_splitk_finish" / "conv_n32_wino2d" / "conv_smallmap" (the small-batch routings: K split over workgroups, Cout-32 layers on the N-tile-64 kernels,
 * conv3x3_sm_kernel on (8 x 8 pixels, 16 channels) units for small maps: 1 inference plans where estimated faster | 2 wherever the shape fits | 0 never),
 * "pool_peephole" (unfused programs: a conv writes the next op's 2x2 max pool), "dw_ln_fuse" (ConvNeXt: LayerNorm inside the
 * depthwise / stem kernels), "wgrad_wino" (3x3 weight gradients in the Winograd domain), "mask_fold" (ReLU masks applied by the kernel
 * that completes a gradient), "conv_f16_rows" (plain fp16: conv3x3_f16_rows_kernel 1 where its plan is estimated faster | 2 wherever the shape fits | 0 never), "conv_f16_rows_pin" (that kernel's tile pinned: see ph_model_last_rows_plans), "upsample_f16math"
 * (plain fp16: the bilinear x2 blended in packed fp16 arithmetic, folded or standalone: same bits), "stem_f16mfma" (plain fp16: stem_f16_kernel), "block_fuse" (plain fp16, inference plans:
 * the two convs of a 32-channel encoder block in one launch), "mlp_fuse" (inference plans: CNBlock's Linear + GELU + Linear + layer scale + residual in one launch at 96 / 192 channels),
 * "grn_fuse" (inference plans: ConvNeXtV2 blocks on the fused GRN plan; only a program whose first Linear carries the GELU can take it, so the unfused training program runs the
 * two-launch GRN forward whatever this says).  Two keys are switches of ph_model_backward, not kernel variants: "pretrained_train" (1: the backward accepts a
 * ConvNeXtV2 program, whose GRN and padding-0 stem ops carry PH_FLAG_NO_TRAIN; 0, the default: it refuses them) and "bwd_frozen_ops" (n: the first n ops of the program get no
 * backward step and none of their parameters' gradients is written -- a frozen encoder; the bucket event and the two-bucket exchange still fire; 0, the default: every op).
 * Unknown key -> PH_E_INVALID. */
int ph_model_set_option(ph_model* m, const char* key, double value);
int ph_model_get_option(const ph_model* m, const char* key, double* value);

/* Per-op timing with HIP events recorded on the forward's own stream (used by bench.py for
 * the roofline object).  While enabled every forward records one event before each op and
 * one after the last; ph_model_profile_read waits for the last recorded forward, returns
 * the milliseconds accumulated per op since profiling was enabled and the number of
 * forwards they cover.  enabled: 1 = start (clears the accumulated times), 0 = stop recording
 * (what was accumulated stays readable), 2 = resume without clearing -- so a caller can sample
 * every n-th forward of a timed region instead of paying ~25 event records in each. */
int ph_model_set_profiling(ph_model* m, int32_t enabled);
int ph_model_profile_read(ph_model* m, double* op_ms, int32_t n_ops, int32_t* n_forwards);

/* Which kernel family each op of the LAST ph_model_forward ran (codes[i] for op i, PH_KV_*; 0 for ops that are not matrix
 * work or were folded into their producer).  bench.py prices a launch's executed MFMA FLOPs from this instead of restating
 * the dispatch rules: direct kernels execute the direct-convolution count 2*Cin*Cout*k*k*H*W, Winograd F(2,3) 2/3 of it,
 * F(2x2,3x3) 4/9, F(4x4,3x3) 1/4. */
#define PH_KV_NONE 0
#define PH_KV_DIRECT 1    /* 9-tap halo kernels on v_mfma_f32_32x32x2_f32 (conv3x3_mfma_*), conv3x3_c16 excluded */
#define PH_KV_WINO1D 2    /* conv3x3_wino_persist_kernel: Winograd F(2,3) along x                                */
#define PH_KV_WINO2D 3    /* conv3x3_wino2d_kernel: wave-split Winograd F(2x2,3x3)                               */
#define PH_KV_W16 4       /* conv3x3_w16_kernel: wave-private Winograd F(2x2,3x3) on v_mfma_f32_16x16x4_f32      */
#define PH_KV_C16 5       /* conv3x3_c16_kernel (16 -> 16 channels, direct)                                      */
#define PH_KV_ROWGEMM 6   /* gemm_mfma_dma_*_kernel (row GEMM: Linear, 2x2/s2, k x k taps, transposed-conv phases) */
#define PH_KV_WINO4 7     /* conv3x3_wino4_kernel: Winograd F(4x4,3x3)                                           */
#define PH_KV_F16 8       /* conv3x3_f16_persist_kernel (fp16 matrix pipe; split precision = 3 MFMAs per product) */
#define PH_KV_STEM 9      /* stem_fused_kernel (second conv on v_mfma_f32_16x16x4_f32; "stem_wino" picks its form) */
#define PH_KV_WINO2D_KS 10 /* conv3x3_wino2d_kernel, K split over workgroups + splitk_reduce_kernel (small batches)       */
#define PH_KV_SMALLMAP 12 /* conv3x3_sm_kernel: Winograd F(2x2,3x3) on 8 x 8-pixel x 16-channel units (small maps, small batches)      */
#define PH_KV_F16_ROWS 13 /* conv3x3_f16_rows_kernel: plain fp16 on v_mfma_f32_16x16x32_f16, row tiles, loader waves, folded bilinear x2 */
#define PH_KV_F16_BLOCK 14 /* block2_c32_f16_kernel: conv(<= 16 -> 32) + conv(32 -> 32) (+ pool) of an encoder block in one launch (plain fp16); the second conv reports PH_KV_FUSED */
#define PH_KV_MLP 15      /* cnblock_mlp_kernel: Linear(C, 4C) + GELU + Linear(4C, C) + layer scale + residual of a CNBlock in one launch (both Linear ops report it; the second has no launch of its own) */
#define PH_KV_CNX_F16_STEM 16 /* patch_stem_f16_kernel: ConvNeXt patch stem, fp16 output (plain fp16 precision)                                    */
#define PH_KV_CNX_F16_DW 17   /* dwconv7_f16_kernel / dwconv7_ln_f16_kernel: depthwise 7x7 on fp16 activations (with the LayerNorm behind it in inference plans: that op reports PH_KV_FUSED) */
#define PH_KV_CNX_F16_LN 18   /* layernorm_f16_kernel: LayerNorm over the channels of an fp16 tensor, fp32 moments                                  */
#define PH_KV_CNX_F16_GEMM 19 /* gemm_f16_kernel: Linear / 2x2-stride-2 conv as a row GEMM on v_mfma_f32_32x32x16_f16 (bias, GELU, layer scale + residual epilogues) */
#define PH_KV_CNX_F16_ELTWISE 20 /* gelu_fmt_kernel / scale_add_fmt_kernel on fp16 activations (unfused programs)                                    */
#define PH_KV_WINDOW_ATTN 21 /* window_attn_kernel (plain variant): one wave per (window, head), q k^T and p v on v_mfma_f32_32x32x2_f32, softmax in registers */
#define PH_KV_WINDOW_ATTN_F16 22 /* window_attn_f16_kernel: the same plan on v_mfma_f32_32x32x16_f16, fp16 q / k / v / p, fp32 logits and softmax statistics ("swint_f16") */
#define PH_KV_SWIN_F16_MERGE_LN 23 /* patch_merge_ln_f16_kernel: four-phase gather + LayerNorm(4C) on fp16 activations, fp32 moments ("swint_f16") */
#define PH_KV_WINDOW_ATTN_BWD 24 /* window_attn_bwd_kernel (ph_model_last_backward_kernels): backward of the attention core, one wave per (window, head), fixed-order slices */
#define PH_KV_GRN 25 /* grn_reduce_kernel + grn_apply_kernel: Global Response Normalization, fixed-slice sums of squares then the apply pass */
#define PH_KV_GRN_FUSED 26 /* grn_finalize_kernel: the fused GRN plan ("grn_fuse"); the sums of squares come from the Linear in front (gemm_mfma_dma_kernel<.., EPI = 2>), the Linear behind runs per sample on weights scaled by grn_scale_weights_kernel */
#define PH_KV_PATCH_STEM_NORM 27 /* patch_stem_norm_kernel: the padding-0 patch stem with input statistics (PH_FLAG_PAD0_NORM) */
#define PH_KV_GRN_BWD 28 /* grn_bwd_reduce_kernel + grn_bwd_sample_kernel + grn_bwd_param_kernel + grn_bwd_apply_kernel (ph_model_last_backward_kernels): backward of a PH_OP_GRN step, fixed-slice sums, no atomics */
#define PH_KV_RESNET_STEM 29 /* resnet_stem_conv_kernel + maxpool3s2_kernel: normalised 7x7 stride-2 stem as an im2col product on v_mfma_f32_32x32x2_f32, then the 3x3 stride-2 max pool */
#define PH_KV_CONV_S2 30 /* gemm_mfma_dma_tile_kernel mode 4 (3x3 stride 2 pad 1) / mode 6 (1x1 stride 2) as the forward of a PH_OP_CONV_S2 */
#define PH_KV_ADD_RELU 31 /* add_relu_kernel: dst = relu(src0 + src1), float4 per thread */
#define PH_KV_WINDOW_ATTN_V2 32 /* window_attn_kernel (cosine variant, swin_kernels.hip): cosine window attention, one wave per (window, head) on v_mfma_f32_32x32x2_f32 */
#define PH_KV_LAYERNORM_ADD 33 /* layernorm_add_kernel: dst = src1 + LayerNorm(src0) */
#define PH_KV_PATCH_MERGE_GATHER 34 /* patch_merge_gather_kernel as the forward of a PH_OP_PATCH_MERGE with PH_FLAG_NO_NORM */
#define PH_KV_WINDOW_ATTN_V2_WIDE 35 /* window_attn_v2_wide_kernel: cosine window attention of windows 9..24, one workgroup per (window, head), keys tiled, online softmax */
#define PH_KV_FUSED 11   /* no launch of its own: a 1x1 head computed in the epilogue of the conv that produces its input */
int ph_model_last_kernels(const ph_model* m, int32_t* codes, int32_t n_ops);
/* ... and the tile plan of every op of the LAST ph_model_forward that ran conv3x3_f16_rows_kernel (PH_KV_F16_ROWS): quad[4 i .. 4 i + 3] = {R rows, Wt columns of a tile, MT M tiles
 * per wave, MG pixel groups} of op i, as f16_rows_plan chose them; zeros for an op on any other kernel.  The kernel instantiation is (Wt % 16 == 0, MT, MG).  Written where the
 * forward decides; host integers only.  The handle option "conv_f16_rows_pin" (R | Wt << 8 | MG << 16; 0, the default: the planner's search) makes the planner consider that
 * one tile -- under every constraint of the search; a layer it does not fit gets the search -- so that a test can run each instantiation on purpose. */
int ph_model_last_rows_plans(const ph_model* m, int32_t* quad, int32_t n_ops);
/* Per-op times of the LAST ph_model_backward, recorded while profiling is on (ph_model_set_profiling).  op_ms[i]: op i's step of the reverse sweep; op_ms_first[i]: its part up to the
 * first data-gradient GEMM (Linear / 2x2-stride-2 ops: the scaling pass and the weight-gradient GEMM; 0 elsewhere); *loss_ms: losses and head-output gradients. */
int ph_model_backward_profile_read(ph_model* m, double* op_ms, double* op_ms_first, int32_t n_ops, double* loss_ms);
/* ... and of the LAST ph_model_backward: PH_KV_WINDOW_ATTN_BWD for a PH_OP_WINDOW_ATTN step, PH_KV_GRN_BWD for a PH_OP_GRN step, PH_KV_ROWGEMM for a Linear / 2x2-stride-2 step,
 * 0 elsewhere -- and for every op of a frozen prefix (handle option bwd_frozen_ops), which runs no step. */
int ph_model_last_backward_kernels(const ph_model* m, int32_t* codes, int32_t n_ops);
/* ... and which route each op's step of the LAST ph_model_backward took, one bit field per op, written where the sweep takes the decision (tests pin every route to a
 * float64 reference without restating a predicate).  0 for an op that ran no step: a frozen prefix (bwd_frozen_ops), an op whose output nobody reads.
 *   bits  0..10  concat part 0: weight-gradient route PH_BR_WG_* (4 bits), data-gradient route (6 bits), 1 bit "accumulated into a gradient that was there"
 *   bits 11..21  concat part 1, the same layout
 *   bits 22..23  who applied the ReLU mask to the op's own output gradient: PH_BR_MASK_*
 *   bits 24..26  who summed the op's bias gradient: PH_BR_BIAS_*
 *   bits 27..30  PH_BR_FOLDED_MASK, PH_BR_SUMMED_BIAS, PH_BR_GELU_FUSED, PH_BR_NO_LAUNCH
 * The data-gradient route of a 3x3 conv on the LDS-DMA family is the PH_KV_* code of its kernel (all below 32); the other routes are PH_BR_DG_*. */
#define PH_BR_PART_BITS 11
#define PH_BR_WG_NONE 0
#define PH_BR_WG_DIRECT 1      /* launch_wgrad: the 32x32-tile nine-tap kernel                                  */
#define PH_BR_WG_WINO 2        /* launch_wgrad_wino: Winograd F(2x2,3x3) domain                                */
#define PH_BR_WG_WINO16 3      /* launch_wgrad16_wino: 16 -> 16 padded channels                                */
#define PH_BR_WG_ROWS9 4       /* nine row-wgrad GEMMs on a 3x3 conv ("wgrad_rows")                            */
#define PH_BR_WG_ROWSKK 5      /* k^2 row-wgrad GEMMs of a k x k conv                                          */
#define PH_BR_WG_INPUT 6       /* launch_input_wgrad: the first 3x3 conv, from the image                       */
#define PH_BR_WG_PATCH_STEM 7  /* launch_patch_stem_wgrad(_norm): im2col + one row-wgrad GEMM                  */
#define PH_BR_WG_CONVT_TAPS 8  /* transposed conv: nine stride-2-gathered row-wgrad GEMMs                      */
#define PH_BR_WG_ROW_GEMM 9    /* Linear / 2x2-stride-2 conv: one row-wgrad GEMM per tap                       */
#define PH_BR_DG_NONE 0
#define PH_BR_DG_REGSTAGED 32  /* launch_conv3x3: the register-staged 3x3 kernel                               */
#define PH_BR_DG_GEMM5 33      /* row GEMM mode 5: k x k taps on the flipped, swapped weights                  */
#define PH_BR_DG_GEMM4 34      /* row GEMM mode 4: 3x3 stride-2 conv (transposed conv's data gradient)         */
#define PH_BR_DG_GEMM0 35      /* row GEMM mode 0: Linear / 2x2-stride-2 conv                                  */
#define PH_BR_ACCUMULATE (1 << 10) /* (within a part) the source slot already held a gradient                  */
#define PH_BR_MASK_SHIFT 22
#define PH_BR_MASK_NONE 0
#define PH_BR_MASK_OWN 1       /* this step's launch_relu_mask / launch_relu_mask_bias_grad                    */
#define PH_BR_MASK_EARLIER 2   /* the step that completed the gradient applied it as it stored ("mask_fold")   */
#define PH_BR_BIAS_SHIFT 24
#define PH_BR_BIAS_NONE 0
#define PH_BR_BIAS_OWN 1         /* this step's launch_bias_grad                                               */
#define PH_BR_BIAS_WITH_MASK 2   /* launch_relu_mask_bias_grad: one pass with the mask                         */
#define PH_BR_BIAS_CLOSER 3      /* the pool / head step that completed the gradient summed it                 */
#define PH_BR_BIAS_INPUT_WGRAD 4 /* the spare column of launch_input_wgrad                                     */
#define PH_BR_BIAS_ROW_WGRAD 5   /* a Linear's weight-gradient row GEMM (column sums of dY)                    */
#define PH_BR_FOLDED_MASK (1 << 27) /* this step applied the ReLU mask of the op that produced its source      */
#define PH_BR_SUMMED_BIAS (1 << 28) /* ... and summed that op's bias gradient                                  */
#define PH_BR_GELU_FUSED (1 << 29)  /* Linear: the GELU derivative rode in the data-gradient GEMM's epilogue   */
#define PH_BR_NO_LAUNCH (1 << 30)   /* GELU: its step launched nothing (fused away by its consumer)            */
int ph_model_last_backward_routes(const ph_model* m, int32_t* routes, int32_t n_ops);

/* Which workspace byte ranges every launch of the LAST ph_model_forward was handed, as the run-time routing decided them (tests of the
 * planner / router agreement: no launch may write a range it, or a later launch, still reads).  One row of six int64 per range:
 * {op index, launch ordinal within the op, 0 = source | 1 = destination, activation slot (-1: the scratch region), byte offset into
 * the workspace, bytes}.  A range is recorded
 * where its pointer goes into the launcher's arguments; an op without a launch of its own (PH_KV_FUSED, the second PH_KV_MLP op, a
 * folded bilinear, a LayerNorm applied by the depthwise kernel, a pool written by a conv epilogue) has no rows: its ranges appear under
 * the op that did the work.  The scratch region behind the slots is a destination of the launches that are handed it.  Host-side
 * bookkeeping of the forward: no launch, no device access.  Writes min(*n_rows, max_rows) rows; rows may be NULL when max_rows is 0. */
int ph_model_last_ranges(const ph_model* m, int64_t* rows, int32_t max_rows, int32_t* n_rows);

/* Diagnostic: when buf_dev != NULL the conv3x3 kernels that carry a probe write into the record block of
 * their op -- 32768 x uint64 per op of the program, op i at buf_dev + 32768 i words (the buffer must hold
 * 32768 x n_ops words) -- e.g. {delta s_memtime, delta s_memrealtime} per workgroup (fp16 pipe; the F(4x4,3x3)
 * kernel in -DW4_CLOCK builds): the shader clock under load is d_memtime / d_memrealtime * 100 MHz
 * (tools/clockprobe_f16.py, tools/clockprobe_layers.py).  NULL turns it off (default). */
int ph_model_set_clock_probe(ph_model* m, void* buf_dev);

/* Debug/parity helper: copy activation slot `slot` of the last forward (NHWC, padded
 * channels) into an NCHW fp32 device buffer of the logical channel count.  Needs a plan that does not recycle ranges: the handle option
 * "workspace_reuse" 0 (every activation kept, nothing fused across ops) or 2 (the inference plan of 1 -- its routing, fusions and skipped stores --
 * with one range per slot: what a fused launch read and what it wrote can be read back; a tensor the fusion keeps out of HBM holds nothing). */
int ph_model_read_slot(ph_model* m, int32_t slot, float* out_dev, int64_t out_numel, void* stream);

/* ------------------------------------------------------------------------------------
 * Peak finding
 * ---------------------------------------------------------------------------------- */

/* Local maxima (strict > over the 8 neighbours, -inf outside) above `threshold`, emitted in
 * the reference's (sample, y, x, channel) order, optionally refined by the integral
 * (first-moment) offset over a patch x patch zero-padded window (refine != 0).
 * cms_dev: (B, C, H, W) fp32.  Outputs (device, capacity `cap` rows):
 *   out_xy (cap,2) f32 [x,y]; out_val (cap) f32; out_sample (cap) i32; out_channel (cap) i32
 *   out_count: device int32[2 + 2B]: [0] = total peaks found (may exceed cap: then only the
 *   first cap rows are valid and the caller should retry), [1+b] = peaks of sample b,
 *   [1+B+b] = exclusive offset of sample b (b = 0..B, last entry = total).
 * xy_scale: out_xy = refined (x, y) * xy_scale in one fp32 multiply -- 1 for find_local_peaks itself, the confidence
 *   maps' output stride for callers that go on in image coordinates (`peaks * cms_output_stride`, layers/bottomup.py:111).
 * scratch_dev: >= 4*(2*B*H + 2) bytes runs the three-pass kernels (count rows, scan, emit: the maps are read twice); with
 *   ph_local_peaks_scratch_bytes(B, C, H, W) bytes the maps are read ONCE (one block per sample and eight rows finds, refines and stages its peaks in order;
 *   a placement pass over the staged peaks puts them at their final offsets) -- same outputs bit for bit, two launches, no atomics. */
int ph_local_peaks(const float* cms_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                   float threshold, int32_t refine, int32_t patch, float* out_xy, float* out_val,
                   int32_t* out_sample, int32_t* out_channel, int32_t* out_count, int32_t cap,
                   float xy_scale, void* scratch_dev, int64_t scratch_bytes, void* stream);

int64_t ph_local_peaks_scratch_bytes(int32_t B, int32_t C, int32_t H, int32_t W);

/* Global peak per (sample, channel): value = max; x = first column containing the max,
 * y = first row containing the max (independent, as the reference); below `threshold`
 * -> NaN coords and value 0.  out_xy (B,C,2), out_val (B,C). */
int ph_global_peaks(const float* cms_dev, int32_t B, int32_t C, int32_t H, int32_t W,
                    float threshold, int32_t refine, int32_t patch, float* out_xy, float* out_val,
                    void* stream);

/* Crop gather (top-down stage 2 pick-up; inference/ops/crops.py:31-124): n crops of
 * crop_h x crop_w from (B, C, H, W) images (dtype 0 = uint8, 1 = float32), zero outside the image.
 * topleft_xy_dev: (n, 2) float32 bbox top-left corners (x, y) as produced by make_centered_bboxes;
 * the integer origin is trunc(tl + half) - half with half = (crop_w/2, crop_h/2) (crops.py:85-90).
 * out_dev: (n, C, crop_h, crop_w), same dtype as the images. */
int ph_crop_bboxes(const void* images_dev, int32_t dtype, int32_t B, int32_t C, int32_t H, int32_t W,
                   const float* topleft_xy_dev, const int32_t* sample_inds_dev, int32_t n,
                   int32_t crop_h, int32_t crop_w, void* out_dev, void* stream);

/* Top-down glue, device side.  ph_centroid_select = CentroidLayer.postprocess after the peak finding (inference/layers/centroid.py:195-261:
 * per frame keep the peaks in order, or the max_instances largest values in descending order (torch.topk) when there are more; NaN-pad to
 * (B, max_instances, 2) / (B, max_instances); undo input scale and eff_scale (inference/ops/coord.py:40-70)) plus what TopDownLayer.predict
 * (inference/layers/topdown.py:127-150, 183-267) derives from the valid centroids IN SIZED SPACE (centroid * eff_scale: the crops are cut from the
 * sizematched frame): make_centered_bboxes (data/instance_cropping.py:129-171) around the sized centroid -- out_bboxes (B, max_instances, 4, 2; NaN where
 * empty) holds those boxes / eff_scale (image space, as the reference stores them) --, and the stage-2 lists in torch.nonzero order of the valid mask
 * (frame, then slot): list_sample int32[n_valid], list_topleft float[n_valid, 2] (sized space: the ph_crop_bboxes inputs), list_slot int32[n_valid] = frame * max_instances + slot,
 * pos_of_slot int32[B * max_instances] = list position or -1, out_n_valid int32[1].  peaks / counts are ph_local_peaks' outputs (coordinates
 * already multiplied by the output stride through its xy_scale).  eff_scale_dev float[B] or NULL; every list pointer may be NULL (centroid-only use). */
int ph_centroid_select(const float* peaks_xy_dev, const float* peak_vals_dev, const int32_t* counts_dev, int32_t B, int32_t max_instances,
                       int32_t cap, float input_scale, const float* eff_scale_dev, float crop_h, float crop_w, float* out_centroids_dev,
                       float* out_vals_dev, float* out_bboxes_dev, int32_t* list_sample_dev, float* list_topleft_dev, int32_t* list_slot_dev,
                       int32_t* pos_of_slot_dev, int32_t* out_n_valid_dev, void* stream);

/* ... and the way back (topdown.py:236-267): crop-local keypoints (n_valid, n_nodes, 2) / values (n_valid, n_nodes) of stage 2 into
 * out_keypoints = (crop keypoints + the crop's top-left (add_crop_offset, ops/coord.py:73-90)) / eff_scale of the slot's frame (sized space ->
 * image space; eff_scale_dev float[slots / max_instances] or NULL = 1), out_crop_keypoints, out_vals, all (slots = B * max_instances,
 * n_nodes[, 2]) and NaN where pos_of_slot is -1. */
int ph_topdown_scatter(const float* crop_xy_dev, const float* crop_vals_dev, const float* list_topleft_dev, const int32_t* pos_of_slot_dev,
                       int32_t slots, int32_t n_nodes, const float* eff_scale_dev, int32_t max_instances, float* out_keypoints_dev,
                       float* out_crop_keypoints_dev, float* out_vals_dev, void* stream);

/* Antialiased bilinear resize of planes x H x W -> planes x OH x OW (uint8: dtype 0, float32: dtype 1), NCHW planes.
 * Replaces torchvision.transforms.v2.functional.resize as called by resize_image (data/resizing.py:70-84, the input-scale step)
 * and apply_sizematcher (data/resizing.py:136-175): for tensors that is torch's interpolate(mode="bilinear",
 * align_corners=False, antialias=True).  uint8 results are bit-exact with the CPU operator (int16 fixed-point weights,
 * horizontal pass first into a uint8 intermediate); float32 matches to fp32 rounding.  tmp_dev: planes * H * OW elements of the
 * same dtype (only read/written when both axes change; may be NULL otherwise). */
int ph_resize_bilinear_aa(const void* src_dev, int32_t dtype, int32_t planes, int32_t H, int32_t W,
                          void* dst_dev, int32_t OH, int32_t OW, void* tmp_dev, void* stream);

/* Class-map sampling for multi-class bottom-up (inference/ops/identity.py:86-101): for each peak
 * gather the K class probabilities at (round-half-even(y), round-half-even(x)) clamped to the map.
 * class_maps_dev (B, K, H, W) fp32; peaks_xy_dev (n, 2) in class-map pixels; out_probs_dev (n, K). */
int ph_sample_class_maps(const float* class_maps_dev, int32_t B, int32_t K, int32_t H, int32_t W,
                         const float* peaks_xy_dev, const int32_t* sample_inds_dev, int32_t n,
                         float* out_probs_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * PAF line-integral scoring (device)
 * ---------------------------------------------------------------------------------- */

/* pafs_dev: (B, 2E, H, W) NCHW fp32 (the head output; the reference's permute to
 * (B,H,W,2E) is folded into the indexing).  peaks are the ph_local_peaks outputs ALREADY
 * multiplied by the confmap stride (image-space x,y), grouped by sample:
 * peak_offsets_dev int32[B+1].  edges_dev int32[E*2] (src node, dst node).
 * t_dev: float[n_points] = torch.linspace(0,1,n_points) values.
 * Outputs (device): cand_edge (cap) i32, cand_src/cand_dst (cap) i32 = peak indices LOCAL
 * to the sample, cand_score (cap) f32, cand_offsets int32[B+1] (+ total in [B]).
 * Candidates of one sample are ordered by edge, then src peak, then dst peak (ascending).
 * scratch_dev: >= 4*(n_peaks_total + B*(n_nodes+1) + B*(E+1) + 16) bytes. */
int ph_paf_score(const float* pafs_dev, int32_t B, int32_t E2, int32_t H, int32_t W,
                 const float* peaks_xy_dev, const int32_t* peak_channel_dev,
                 const int32_t* peak_offsets_dev, int32_t n_peaks_total, int32_t n_nodes,
                 const int32_t* edges_dev, int32_t n_edges, const float* t_dev, int32_t n_points,
                 int32_t pafs_stride, float max_edge_length, float dist_penalty_weight,
                 int32_t* cand_edge, int32_t* cand_src, int32_t* cand_dst, float* cand_score,
                 int32_t* cand_offsets, int32_t cap, void* scratch_dev, int64_t scratch_bytes,
                 void* stream);

/* ------------------------------------------------------------------------------------
 * Host (CPU) stage: assignment + instance assembly.  Pure host code, no HIP calls.
 * ---------------------------------------------------------------------------------- */

/* Rectangular linear sum assignment (minimise), row-major cost (nr x nc) doubles; +inf =
 * forbidden.  Writes min(nr,nc) pairs sorted by row.  Tie behaviour follows SciPy's
 * rectangular_lsap (shortest augmenting path).  PH_E_INFEASIBLE if no finite solution. */
int ph_lsap(const double* cost, int32_t nr, int32_t nc, int32_t* rows, int32_t* cols);

/* BFS edge order from the topological root; out_order has room for n_edges entries;
 * returns the number of entries written (>=0) or a negative error. */
int ph_toposort_edges(const int32_t* edges, int32_t n_edges, int32_t* out_order);

/* Match + assemble a batch (all host arrays).  Inputs mirror ScoredBatch
 * (inference/streaming.py:43-112) in flattened form.  Outputs are NaN-padded:
 *   out_kpts (B, max_inst, n_nodes, 2), out_vals (B, max_inst, n_nodes), out_scores (B, max_inst),
 *   out_n_inst int32[B] = instances found per sample before truncation.
 * If an instance count exceeds max_inst: truncate_by_score != 0 keeps the top max_inst by
 * instance score (numpy argsort()[::-1] order), else keeps the first max_inst. */
int ph_group_batch(int32_t B, int32_t n_nodes, const int32_t* edges, int32_t n_edges,
                   const float* peaks_xy, const float* peak_vals, const int32_t* peak_channel,
                   const int32_t* peak_offsets, const int32_t* cand_edge, const int32_t* cand_src,
                   const int32_t* cand_dst, const float* cand_score, const int32_t* cand_offsets,
                   float min_line_score, double min_instance_peaks, int32_t min_instance_peaks_is_fraction,
                   int32_t max_inst, int32_t truncate_by_score, float* out_kpts, float* out_vals,
                   float* out_scores, int32_t* out_n_inst);

/* The whole CPU stage of a bottom-up batch from the packed D2H arena of the GPU stage, in one call: unpack + capacity check + the
 * max_peaks_per_node guard (inference/layers/bottomup.py:126-161), ph_group_batch, then the input-scale / eff_scale undo and the output sizing of
 * group_scored_batch (inference/streaming.py:147-255).  arena (host, pinned or not) = float32 / int32 words
 *   [counts 2+2B (ph_local_peaks' out_count) | cand offsets B+1 | xy 2*peak_cap | vals peak_cap | cand score cand_cap | channel peak_cap |
 *    cand edge cand_cap | cand src cand_cap | cand dst cand_cap].
 * max_instances < 0 = None (keep every instance); max_peaks_per_node < 0 = no guard; eff_scale float[B] or NULL.
 * Outputs (B, out_cap, n_nodes, 2) / (B, out_cap, n_nodes) / (B, out_cap) NaN-padded (row stride out_cap, or max(1, max_instances) when that is given
 * and <= out_cap), out_n_inst int32[B].  status int32[4]: [0] peaks, [1] candidates, [2] flags -- 1: arena capacity exceeded (nothing grouped: re-run
 * the GPU stage with at least status[0] / status[1] entries), 2: out_cap too small (nothing grouped: come back with status[3]), 4: guard fired (all NaN)
 * --, [3] instances per frame the caller should keep (max over frames, >= 1; max_instances when given). */
int ph_group_packed(const float* arena, int32_t B, int32_t n_nodes, int32_t peak_cap, int32_t cand_cap, const int32_t* edges, int32_t n_edges,
                    float min_line_score, double min_instance_peaks, int32_t min_instance_peaks_is_fraction, int32_t max_instances,
                    int32_t max_peaks_per_node, float input_scale, const float* eff_scale, int32_t out_cap, float* out_kpts, float* out_vals,
                    float* out_scores, int32_t* out_n_inst, int32_t* status);

/* Host: Hungarian matching of peaks to classes per (sample, channel)
 * (inference/ops/identity.py:13-76).  probs (n, K) fp32, sample/channel (n) int32.
 * Writes matched (peak index, class index) pairs that also are the peak's arg-max class
 * (is_best filter, identity.py:61-66) in (sample, channel) order; returns the pair count. */
int ph_group_class_peaks(const float* probs, const int32_t* sample_inds, const int32_t* channel_inds,
                         int32_t n, int32_t n_samples, int32_t n_channels, int32_t K,
                         int32_t* out_peak_inds, int32_t* out_class_inds);

/* ------------------------------------------------------------------------------------
 * Training augmentation (data/skia_augmentation.py)
 * ---------------------------------------------------------------------------------- */

#define PH_AUG_FLIP 1        /* mirror left/right before the affine (keypoints: x' = (W-1) - x, then the pair swap) */
#define PH_AUG_WARP 2        /* resample through minv with coverage of the mapped frame; keypoints mapped by m   */
#define PH_AUG_UNIFORM 4     /* uniform integer noise in [uni_lo, uni_hi] added in int16, clipped              */
#define PH_AUG_GAUSS 8       /* trunc(N(gauss_mean, gauss_std)) added in int16, clipped (uint8 units)           */
#define PH_AUG_CONTRAST 16   /* uint8(clip((v - 127.5) * contrast + 127.5, 0, 255)), fp32, no contraction        */
#define PH_AUG_BRIGHTNESS 32 /* uint8(clip(v * brightness, 0, 255))                                              */
#define PH_AUG_ERASE 64      /* [erase_y, erase_y + erase_h) x [erase_x, erase_x + erase_w) = fill[c] after the warp */

/* One sample's parameters (host-drawn; sleap_nn_amd/data/augmentation.py).  Coordinates are pixel coordinates
 * (pixel (x, y) covers [x, x+1) x [y, y+1)).  minv maps an output pixel centre to a source point, the flip folded in
 * (x -> W - x): sx = minv[0] x + minv[1] y + minv[2], sy = minv[3] x + minv[4] y + minv[5]; the bilinear sample is taken
 * at (sx - 0.5, sy - 0.5) in index coordinates, clamp to edge.  m is the skia matrix itself (keypoints).  edge[4][3]:
 * the mapped frame rectangle M [0,W]x[0,H] as four half-planes nx x + ny y + d >= 0 with |(nx, ny)| = 1.
 * seed keys the counter-based noise: (seed, sample, channel, source y, source x). */
typedef struct ph_aug_sample {
  float minv[6];
  float m[6];
  float edge[12];
  int32_t flags;
  int32_t uni_lo, uni_hi;
  float gauss_mean, gauss_std;
  float contrast, brightness;
  int32_t erase_y, erase_x, erase_h, erase_w;
  int32_t fill[3];
  uint32_t seed;
  int32_t pad_;
} ph_aug_sample;

int32_t ph_aug_sample_size(void);

/* Intensity + flip + affine + erase of a batch in one image launch (and one keypoint launch).
 * src_dev / dst_dev: (B, C, H, W), dtype 0 = uint8, 1 = float32 in [0, 1] (quantised (uint8)(x * 255) on the way in,
 * u / 255 on the way out); C is 1 or 3; src and dst must not overlap.  kp_in_dev / kp_out_dev: (B, I, N, 2) fp32,
 * NaN = missing (both NULL when there are no keypoints; must not overlap).  params_dev: B ph_aug_sample in device memory.
 * sym_pairs_dev: int32 (n_pairs, 2) node pairs swapped, in order, after a flip.  counters_dev: NULL or int32[4]
 * incremented per (sample, tile): [0] copy tiles, [1] zero tiles (outside the mapped frame, nothing loaded), [2] tiles
 * sampled from an LDS-staged source box, [3] tiles gathered directly (source box over the LDS budget). */
int ph_augment(const void* src_dev, void* dst_dev, int32_t dtype, int32_t B, int32_t C, int32_t H, int32_t W,
               const float* kp_in_dev, float* kp_out_dev, int32_t I, int32_t N, const ph_aug_sample* params_dev,
               const int32_t* sym_pairs_dev, int32_t n_pairs, int32_t* counters_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Tiled inference (inference/layers/tiled.py)
 * ---------------------------------------------------------------------------------- */

/* All tiles of all frames of a batch in one launch.  frames_dev: (F, C, H, W), dtype 0 = uint8, 1 = float32, NCHW contiguous.
 * y_origins_dev int32[ny] / x_origins_dev int32[nx]: tile origins per axis in frame pixels (device memory; the grid is their
 * Cartesian product).  tiles_dev: (F * ny * nx, C, tile_size, tile_size) of the same dtype; tile iy * nx + ix of frame f is row
 * f * ny * nx + iy * nx + ix.  Pixels outside the frame are written as zeros.  No alignment of rows or origins is assumed. */
int ph_tile_extract(const void* frames_dev, int32_t dtype, int32_t F, int32_t C, int32_t H, int32_t W, const int32_t* y_origins_dev, int32_t ny,
                    const int32_t* x_origins_dev, int32_t nx, int32_t tile_size, void* tiles_dev, void* stream);

/* Stitch per-tile maps into per-frame maps with an importance window, as a gather.  tile_maps_dev: (F * ny * nx, N, th, tw) fp32 in
 * the row order of ph_tile_extract; window_dev: (th, tw) fp32; origins in OUTPUT pixels (device memory); out_dev: (F, N, h, w) fp32.
 * Per output pixel, over the covering tiles in ascending tile index (iy outer, ix inner), starting from acc = cnt = +0:
 * acc = acc + tile * w, cnt = cnt + w as separate round-to-nearest fp32 operations, result acc / cnt -- the sequence
 * TileMerger.integrate / merge(eps=None) performs, so the output is bit-identical to that canvas cropped to (h, w); pixels no tile
 * covers are NaN.  Tiles may reach past (h, w): only the cropped region is written. */
int ph_tile_merge(const float* tile_maps_dev, const float* window_dev, int32_t F, int32_t N, int32_t th, int32_t tw, const int32_t* y_origins_dev,
                  int32_t ny, const int32_t* x_origins_dev, int32_t nx, int32_t h, int32_t w, float* out_dev, void* stream);

/* ph_tile_merge for K heads (1 <= K <= 4) in ONE launch (the tiled segmentation wrappers: foreground 1, centre 1, offset 2 channels;
 * DESIGN.md section 10a).  arenas_dev / outs_dev / channels are HOST arrays of K entries: arenas_dev[k] is a device pointer to
 * (F * ny * nx, channels[k], th, tw) fp32 in the row order of ph_tile_extract, outs_dev[k] one to a contiguous (F, channels[k], h, w)
 * fp32 map; channels[k] >= 1 and at most 8 channels in total.  Window, origins, (h, w) and the arithmetic are ph_tile_merge's and shared
 * by the heads; per pixel the covering tiles are walked once, the window loaded once per tile, cnt and every channel's accumulator
 * kept in registers.  Channels are independent, so each output is bit-identical to ph_tile_merge on its arena and to the matching
 * channels of a TileMerger canvas of sum(channels).  Pointers and channel counts go to the kernel by value (no device pointer
 * table, no host synchronisation).  No output may overlap an arena or another output. */
int ph_tile_merge_heads(const float* const* arenas_dev, const int32_t* channels, int32_t K, const float* window_dev, int32_t F, int32_t th, int32_t tw,
                        const int32_t* y_origins_dev, int32_t ny, const int32_t* x_origins_dev, int32_t nx, int32_t h, int32_t w, float* const* outs_dev,
                        void* stream);

/* ------------------------------------------------------------------------------------
 * Bottom-up instance segmentation grouping (inference/segmentation.py)
 * ---------------------------------------------------------------------------------- */

/* Scratch of ph_seg_center_peaks for B maps of (h, w) and a candidate list of `cap` entries per frame. */
int64_t ph_seg_scratch_bytes(int32_t B, int32_t h, int32_t w, int32_t cap);

/* Plateau-aware centre peaks of B centre maps (B, h, w) fp32 (find_center_peaks, segmentation.py:12-60).  A pixel is a candidate
 * when hm > threshold and hm >= every in-image value of its nms_kernel x nms_kernel window (3, 5 or 7); candidates that touch by
 * 4-connectivity form one component, represented by its maximum (raster-first on ties) and numbered by its raster-first pixel.
 * max_instances > 0 and more components: the max_instances largest values, descending (torch.topk); otherwise component order.
 * centers_dev int32 (B, max_centers, 2) = (x, y) in map pixels, scores_dev fp32 (B, max_centers).  counts_dev int32[2 B]:
 * [b] = centres of frame b, [B + b] = its candidates.  Both are TRUE counts: a frame with more candidates than `cap` reports 0
 * centres, one with more centres than max_centers has only the first max_centers written -- the caller compares and comes back
 * with room (the convention of ph_local_peaks).  pix_counts_dev int32 (n_count_bufs, B, max_centers) is zeroed here for
 * ph_seg_assign / ph_seg_gate.  Two launches, no host synchronisation; scratch must be 8-byte aligned. */
int ph_seg_center_peaks(const float* center_dev, int32_t B, int32_t h, int32_t w, float threshold, int32_t nms_kernel, int32_t max_instances, int32_t cap,
                        int32_t max_centers, int32_t* centers_dev, float* scores_dev, int32_t* counts_dev, int32_t* pix_counts_dev, int32_t n_count_bufs,
                        void* scratch_dev, int64_t scratch_bytes, void* stream);

/* Label map of the foreground pixels (segmentation.py:159-190): for fg > fg_threshold, px = x s + s/2 + dx, py = y s + s/2 + dy,
 * cx = xc s + s/2, cy = yc s + s/2, d = (px - cx)^2 + (py - cy)^2 in fp32 with every operation rounded on its own (no FMA), label =
 * first argmin over the frame's centres.  fg_dev (B, 1, h, w), offsets_dev (B, 2, h, w) = (dx, dy); centers_dev / counts_dev from
 * ph_seg_center_peaks.  labels_dev (B, h, w) of label_bytes-wide signed integers (1: max_centers <= 127, 2: <= 32767, 4), -1 =
 * background; dist_dev NULL or fp32 (B, h, w) = the chosen d; pix_counts_dev[b][k] += pixels labelled k (buffer 0 of the array
 * ph_seg_center_peaks zeroed). */
int ph_seg_assign(const float* fg_dev, const float* offsets_dev, int32_t B, int32_t h, int32_t w, float fg_threshold, int32_t output_stride,
                  const int32_t* centers_dev, const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes, void* labels_dev, float* dist_dev,
                  int32_t* pix_counts_dev, void* stream);

/* Adaptive distance gate (segmentation.py:197-211), `iters` passes: r2 = (alpha * sqrt(count / pi) * s)^2 in fp32 from the
 * kept-pixel counts of the previous pass, keep = d <= r2[label] recomputed over ALL assigned pixels of labels_in_dev each pass, as the reference does.
 * pix_counts_dev int32 (iters + 1, B, max_centers): buffer 0 = ph_seg_assign's counts, buffer k + 1 = the counts after pass k
 * (zeroed by ph_seg_center_peaks).  labels_out_dev (its own buffer) = the labels kept by the last pass, -1 elsewhere. */
int ph_seg_gate(const void* labels_in_dev, const float* dist_dev, int32_t B, int32_t h, int32_t w, float alpha, int32_t output_stride, int32_t iters,
                const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes, int32_t* pix_counts_dev, void* labels_out_dev, void* stream);

/* Mask cleanup of the label map ph_seg_assign / ph_seg_gate wrote (_clean_instance_mask at radius 0, segmentation.py:240-273; DESIGN.md
 * section 4.2d): per (frame, label) keep the largest 4-connected component -- raster-first on equal areas -- and fill its interior
 * holes (binary_fill_holes: complement cells that cannot reach the outside of the image by 4-connected steps through the complement;
 * pixels of other instances count as complement, so masks may overlap afterwards).  labels_out_dev (its own buffer, the input's
 * type): pixels of dropped components become -1.  record_dev int32 [areas (B, max_centers) | hole counts (B, max_centers) | holes
 * per frame B | pool words needed per frame B]: area = kept component + its holes, 0 for a label without pixels.  holes_dev int32
 * (B, hole_cap, 2) = (pixel index y * w + x, label), instance-major, raster order inside an instance, offsets from an exclusive scan
 * of the hole counts; the per-frame totals are TRUE counts: entries beyond hole_cap are not written and the caller comes back with
 * room.  Boxes (bounding box + a one-pixel ring) whose two bitmaps exceed the LDS ones are flooded in a pool of pool_words 64-bit
 * words per frame inside the scratch; a frame that needs more reports its need the same way (instances without room keep their
 * holes unfilled until then).  h, w <= 32767.  Integer arithmetic only: exact, and identical from run to run.  Eight launches on
 * `stream`, no host synchronisation; scratch 8-byte aligned, ph_seg_cleanup_scratch_bytes(B, h, w, max_centers, pool_words) bytes. */
int64_t ph_seg_cleanup_scratch_bytes(int32_t B, int32_t h, int32_t w, int32_t max_centers, int32_t pool_words);
int ph_seg_cleanup(const void* labels_in_dev, int32_t B, int32_t h, int32_t w, const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes,
                   void* labels_out_dev, int32_t* record_dev, int32_t* holes_dev, int32_t hole_cap, int32_t pool_words, void* scratch_dev,
                   int64_t scratch_bytes, void* stream);

/* Pair tables for the fragment merge (merge_instances' region-adjacency graph, inference/segmentation.py:424-579) from
 * the label map ph_seg_assign / ph_seg_gate (or ph_seg_cleanup) wrote; center_dev (B, 1, h, w), offsets_dev (B, 2, h, w), centers_dev /
 * counts_dev from ph_seg_center_peaks.  With n = min(counts[b], max_centers) and d = dilate in [1, 4]:
 *   contact T[a][b] (a != b) = pixels labelled b with at least one pixel labelled a within L1 distance <= d inside the image (SciPy's cross
 *     iterated d times, border value 0); a pixel counts once per a.  Exact integers; _contact_fraction's overlap(i, j) = T[i][j] + T[j][i].
 *   moments_dev double (B, max_centers, 4) = sums over the label's pixels of (rx, ry, rx^2, ry^2), rx = (x - xc) s + dx, ry = (y - yc) s + dy:
 *     the offset-predicted centre relative to the instance's own; float64 sums of the fp32 offsets in a fixed order (bit-identical from run
 *     to run and on any stream; no floating-point atomics); zeros for a label without pixels or at and beyond n.
 *   edges_dev int32 (B, edge_cap, 5) = (i, j, T[i][j], T[j][i], fp32 bits of the ridge minimum) for the pairs i < j with T[i][j] + T[j][i] > 0,
 *     in (i, j) order; edge_counts_dev[b] is the TRUE count: entries beyond edge_cap are not written and the caller comes back with room.
 *     Ridge minimum: min of the centre map over the cells round(c_i + (c_j - c_i) k / 47), k = 7..39, clipped to the map
 *     (_center_valley_ridge's 33 interior samples of 48; computed in integers, no sample is a rounding tie); NaN if a sample is NaN.
 * max_centers <= 4096 and B * max_centers^2 <= 2^29 (a dense table in the scratch); h, w <= 32767.  Four launches on `stream`, no host
 * synchronisation; scratch 8-byte aligned, ph_seg_merge_scratch_bytes(B, h, w, max_centers) bytes (0 for arguments out of range). */
int64_t ph_seg_merge_scratch_bytes(int32_t B, int32_t h, int32_t w, int32_t max_centers);
int ph_seg_merge_tables(const void* labels_dev, const float* center_dev, const float* offsets_dev, int32_t B, int32_t h, int32_t w, int32_t output_stride,
                        int32_t dilate, const int32_t* centers_dev, const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes, double* moments_dev,
                        int32_t* edge_counts_dev, int32_t* edges_dev, int32_t edge_cap, void* scratch_dev, int64_t scratch_bytes, void* stream);

/* Semantic variant (layers/segmentation.py:438-503): mask_dev uint8 (B, h, w) = fg > fg_threshold, count_dev int32[B] its
 * pixels, sum_dev double[B] the sum of fg over them (fixed summation order: deterministic; the reference's score is sum / count). */
int64_t ph_seg_semantic_scratch_bytes(int32_t B, int32_t h, int32_t w);
int ph_seg_semantic(const float* fg_dev, int32_t B, int32_t h, int32_t w, float fg_threshold, uint8_t* mask_dev, int32_t* count_dev, double* sum_dev,
                    void* scratch_dev, int64_t scratch_bytes, void* stream);

/* Top-down crop masks into frame space (decode_mask_to_image_res, inference/segmentation_convert.py:74-133, for a batch).
 * masks_dev uint8 (N, h, w) as ph_seg_semantic writes them; pos_of_slot_dev int32[B * P] as ph_centroid_select writes it (-1 = empty slot, a
 * value at or beyond N counts as empty); geom_dev int32 (N, 4) = (ox, oy, He, We): the rounded image-space origin and the decoded extent of
 * each crop.  out_dev uint8 (B, P, H, W), 16-byte aligned -- pred_form 0 of ph_mask_pair_stats at pred_stride 1.  Pixel (y, x) of slot s
 * with crop k = pos_of_slot[s]: v = y - oy, u = x - ox; inside 0 <= v < He, 0 <= u < We it is masks[k][(v * h) / He][(u * w) / We] (integer
 * division: the nearest resample to (He, We), then the top-left pad / clip), else 0.  A crop whose He or We is outside [1, 65535] is empty.
 * Every byte of out_dev is written (no memset needed), nothing is accumulated: identical from run to run.  1 <= P <= 64, h, w <= 32767,
 * B P H W < 2^32 (PH_E_INVALID beyond).  One launch, no host synchronisation. */
int ph_seg_place_crops(const uint8_t* masks_dev, int32_t N, int32_t h, int32_t w, const int32_t* pos_of_slot_dev, const int32_t* geom_dev, int32_t B, int32_t P,
                       int32_t H, int32_t W, uint8_t* out_dev, void* stream);

/* ------------------------------------------------------------------------------------
 * Segmentation evaluation (evaluation.py:339-409 _align_pair / _mask_pair_stats / _mask_to_boundary / _boundary_iou)
 * ---------------------------------------------------------------------------------- */

/* Contingency table of a predicted and a ground-truth mask set per frame, in one pass over the pixels (_mask_pair_stats,
 * evaluation.py:352-372, without its P * G image passes).  gt_dev uint8 (B, G, H, W), nonzero = foreground, masks may overlap.
 * pred_form 0: pred_dev uint8 (B, P, ph, pw), masks may overlap; pred_form 1 / 2 / 4: pred_dev is a label map (B, ph, pw) of signed
 * integers that many bytes wide, -1 = background, labels in [0, P) (what ph_seg_assign / ph_seg_gate write).  Canvas pixel (y, x)
 * reads prediction cell (y / pred_stride, x / pred_stride): nearest up-sampling by an exact integer factor.  The canvas is _align_pair's
 * (evaluation.py:339-349), top-left aligned, max(H, ph * pred_stride) x max(W, pw * pred_stride); a set has no foreground outside its
 * own extent, and its foreground outside the other set's extent still counts in its area.  n_pred_dev / n_gt_dev int32[B]: slots at or
 * beyond the count are never read and their outputs are 0 (a label at or beyond n_pred is background).  inter_dev int32 (B, P, G),
 * pred_area_dev int32 (B, P), gt_area_dev int32 (B, G) are zeroed here on `stream`; integer accumulation only, so the result is exact
 * and identical from run to run.  1 <= P, G <= 64 (PH_E_INVALID beyond).  One launch, no host synchronisation. */
int ph_mask_pair_stats(const void* pred_dev, int32_t pred_form, int32_t P, int32_t ph, int32_t pw, int32_t pred_stride, const uint8_t* gt_dev, int32_t G,
                       int32_t H, int32_t W, int32_t B, const int32_t* n_pred_dev, const int32_t* n_gt_dev, int32_t* inter_dev, int32_t* pred_area_dev,
                       int32_t* gt_area_dev, void* stream);

/* Boundary region of N masks (_mask_to_boundary, evaluation.py:375-393): masks_dev uint8 (N, H, W), nonzero = foreground; out_dev uint8
 * (N, H, W) = 1 where mask AND NOT eroded, else 0.  A pixel is eroded exactly when min(y, x, H - 1 - y, W - 1 - x) >= d and every pixel
 * of its (2d + 1) x (2d + 1) window is foreground: d iterations of a 3x3 erosion behind a one-pixel zero border.  The caller computes
 * d = max(1, round(0.02 * sqrt(H^2 + W^2))).  Separable (a row pass into scratch_dev, then a column pass); scratch_dev of
 * ph_mask_boundary_scratch_bytes(N, H, W) bytes, 2-byte aligned; out_dev must not be masks_dev.  Two launches. */
int64_t ph_mask_boundary_scratch_bytes(int32_t N, int32_t H, int32_t W);
int ph_mask_boundary(const uint8_t* masks_dev, int32_t N, int32_t H, int32_t W, int32_t d, uint8_t* out_dev, void* scratch_dev, int64_t scratch_bytes,
                     void* stream);

/* ------------------------------------------------------------------------------------
 * Cross-frame tracking (tracking/tracker.py:513-586 get_scores, tracking/utils.py:127-252)
 * ---------------------------------------------------------------------------------- */

enum ph_track_method { PH_TRACK_OKS = 0, PH_TRACK_IOU = 1, PH_TRACK_EUCLID = 2, PH_TRACK_COSINE = 3 };

/* Every pose pair score of a batch in one call (host code, float64, the reference's operation order).  cur (B, I, N, 2): the features of the
 * batch's frames, instance-major, N pairs of doubles per instance (keypoints (x, y) with NaN for a missing node for PH_TRACK_OKS; any
 * feature of 2 N numbers for PH_TRACK_EUCLID / PH_TRACK_COSINE; N = 2, [xmin, ymin, xmax, ymax], for PH_TRACK_IOU).  hist (L, I, N, 2):
 * the features of earlier frames, newest LAST, the last n_hist slots valid.  counts int32 (B + L): the instances of each cur frame, then
 * of each hist slot; rows at or beyond a count are never read.  out double (B, L, I, I): [b][k - 1][i][j] = the score of instance i of
 * frame b against instance j of the frame k calls earlier, which is cur[b - k] if b >= k and hist[L - (k - b)] otherwise; NaN where i or
 * j is beyond its frame's count or the lag reaches beyond n_hist.  PH_TRACK_OKS: compute_oks with the current instance as points_gt, its
 * bounding-box area as the scale, np.spacing(1) and oks_stddev; PH_TRACK_IOU: compute_iou with its + 1s; PH_TRACK_EUCLID: minus the
 * Euclidean norm; PH_TRACK_COSINE: the cosine.  A NaN stays NaN where NumPy gives NaN.  1 <= L <= 32. */
int ph_track_pose_scores(const double* cur, int32_t B, const double* hist, int32_t L, int32_t n_hist, int32_t I, int32_t N, const int32_t* counts,
                         int32_t method, double oks_stddev, double* out);

/* Weighted contingency tables of a batch of label maps against earlier label maps.  labels_dev (B, h, w) and hist_dev (L, h, w): signed
 * integers label_bytes (1, 2 or 4) wide, -1 = background, as ph_seg_assign / ph_seg_gate write them; a label at or beyond P is treated as
 * BACKGROUND.  hist_dev holds earlier frames, newest LAST, the last n_hist slots valid.  row_weight_dev int32[h], col_weight_dev int32[w]:
 * the image rows / columns a cell row / column stands for (0 in the padding); image_pixels = sum(row_weight) * sum(col_weight), stated
 * by the caller, must be below 2^31 (the counters are int32).  inter_dev int32 (B, L, P, P): [b][k - 1][a][c] = the sum over cells (v, u)
 * of row_weight[v] * col_weight[u] where frame b has label a and the frame k calls earlier has label c -- that frame is labels[b - k] if
 * b >= k and hist[L - (k - b)] otherwise; a lag that reaches beyond n_hist is written as zeros.  area_dev int32 (B, P): [b][a] = the same
 * weighted count of label a alone.  Both are zeroed here on `stream`; integer accumulation only, so the result is exact and identical
 * from run to run and on any stream.  1 <= P <= 64, 1 <= L <= 32 (PH_E_INVALID beyond).  One launch, no host synchronisation. */
int ph_track_mask_pairs(const void* labels_dev, int32_t label_bytes, int32_t B, int32_t h, int32_t w, const void* hist_dev, int32_t L, int32_t n_hist,
                        const int32_t* row_weight_dev, const int32_t* col_weight_dev, int64_t image_pixels, int32_t P, int32_t* inter_dev, int32_t* area_dev,
                        void* stream);

/* ph_track_pose_scores for candidates whose features differ per current frame (the flow-shift tracker: a past instance's keypoints are moved onto each
 * current frame before the feature function).  cur (B, I, N, 2) as above; hist (B, L, I, N, 2): [b][g][j] = the feature of candidate j
 * of group g (a lag, or a reference frame) as seen from frame b; counts_cur int32 (B); counts_hist int32 (B, L): 0 for a group that does not exist.  out double
 * (B, L, I, I): [b][g][i][j] = the score of instance i of frame b against candidate j of group g, by the same pair functions; NaN beyond a count.  1 <= L <= 32. */
int ph_track_pose_scores_shifted(const double* cur, int32_t B, const double* hist, int32_t L, int32_t I, int32_t N, const int32_t* counts_cur,
                                 const int32_t* counts_hist, int32_t method, double oks_stddev, double* out);

/* ------------------------------------------------------------------------------------
 * Pyramidal Lucas-Kanade optical flow (the flow-shift tracker; sleap_nn_amd/tracking/flow.py pyr_lk is the definition)
 * ---------------------------------------------------------------------------------- */

#define PH_FLOW_MAX_LEVELS 8 /* max_level 0..7: levels 0..7 */

/* One job of ph_flow_track: the pyramids of a reference frame and of a current frame (device pointers per level, level 0 = the frame itself, all uint8,
 * dense rows, the sizes ph_flow_pyramid gives for the launch's H, W, win and max_level) and the points [pt_begin, pt_end) of the launch's point array,
 * which lie on the reference frame.  136 bytes. */
typedef struct ph_flow_job {
  const uint8_t* ref[PH_FLOW_MAX_LEVELS];
  const uint8_t* cur[PH_FLOW_MAX_LEVELS];
  int32_t pt_begin, pt_end;
} ph_flow_job;
int ph_flow_job_size(void);

/* Levels of the pyramid of an H x W frame: level l + 1 is ((w + 1) / 2, (h + 1) / 2) and exists while both sides exceed win, up to max_level.  Returns the
 * number of levels (1 .. max_level + 1) and writes their (height, width) pairs to sizes (int32[2 * PH_FLOW_MAX_LEVELS], may be null); PH_E_INVALID for win
 * outside 3..41, max_level outside 0..7 or a side below 2. */
int ph_flow_levels(int32_t H, int32_t W, int32_t win, int32_t max_level, int32_t* sizes);

/* Every level above 0 of B uint8 frames (B, H, W): separable [1 4 6 4 1] at (2x, 2y), reflect-101 borders, (sum + 128) >> 8 -- bit-identical to pyr_lk's
 * levels.  out_dev: B records of S = sum over levels l >= 1 of h_l * w_l bytes, the levels of a frame one after another (level 1 first); out_bytes >= B * S.
 * One launch per level on `stream`, no host synchronisation.  Returns the number of levels. */
int ph_flow_pyramid(const uint8_t* frames_dev, int32_t B, int32_t H, int32_t W, int32_t win, int32_t max_level, uint8_t* out_dev, int64_t out_bytes, void* stream);

/* pyr_lk for a list of jobs in ONE launch: one wave works one point through all of its levels.  jobs_dev: n_jobs ph_flow_job records ON THE DEVICE;
 * points_dev float32 (n_points, 2) (x, y), NaN = no point; every point must belong to exactly one job's range.  shifted_dev float32 (n_points, 2): the
 * point on the current frame, NaN where status is 0; status_dev uint8 (n_points).  The grid is (max_job_points, n_jobs): a job's points beyond
 * max_job_points, and points no job names, come back lost (NaN, status 0).  max_iter 1..100, eps > 0 (the reference: 30, 0.01).  No atomics, no host
 * synchronisation.  win 3..41 and max_level 0..7, PH_E_INVALID beyond. */
int ph_flow_track(const ph_flow_job* jobs_dev, int32_t n_jobs, int32_t max_job_points, const float* points_dev, int32_t n_points, int32_t H, int32_t W,
                  int32_t win, int32_t max_level, int32_t max_iter, double eps, float* shifted_dev, uint8_t* status_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* POSEHIP_H */
