// Internal structures of the network runtime shared by model.hip (handle, options, accessors), weights.hip (weight forms, ph_model_create), plan.hip (workspace plan), forward.hip (forward), backward.hip (backward) and
// train.hip (parameter arena, bucket split, branch scales, head losses).
#pragma once
#include <string>
#include <vector>

#include "act_format.h"
#include "common.h"
#include "convnext_f16_kernels.h"
#include "f16_kernels.h"
#include "net_kernels.h"
#include "conv3x3_route.h"

namespace ph {

struct PackedOp {
  ph_op_desc d;
  float* w_dev = nullptr;
  float* b_dev = nullptr;
  float* w2_dev = nullptr;
  float* b2_dev = nullptr;
  float* w_dma_dev = nullptr;  // conv weights in the LDS-DMA (quad-major piece) layout
  float* b_grn_dev = nullptr;  // residual Linear behind a PH_OP_GRN: W2 grn.bias + b2, the bias of the fused GRN plan ("grn_fuse"); folded at creation, and again by ph_model_set_params in a program that can take that plan
  float* w_mlp_dev = nullptr;  // Linear of a CNBlock MLP pair (inference programs): its weight as cnblock_mlp_kernel's LDS images
  int bn = 0;
  float* wd_gemm_dev[4] = {nullptr, nullptr, nullptr, nullptr};  // Linear / 2x2 conv: transposed weights (per tap) for the data gradient
  int bn_dg = 0;
  float* dw_flip_dev = nullptr;  // depthwise conv: spatially flipped taps (data gradient)
  float* w_gemm_dev = nullptr;  // 3x3 conv weights in the row-GEMM layout (small feature maps)
  float* b_gemm_dev = nullptr;
  int bn_g = 0;
  // data-gradient weights of a 3x3 conv (flipped taps, in/out swapped), one set per concat source
  float* wd_dev[2] = {nullptr, nullptr};
  float* wd_dma_dev[2] = {nullptr, nullptr};
  float* zero_bias_dev = nullptr;
  float* wdk_gemm_dev[2] = {nullptr, nullptr};  // k x k conv (k != 3): data-gradient weights (flipped taps, in/out swapped) in the row-GEMM layout, per concat source
  int bn_dk[2] = {0, 0};
  int bn_d[2] = {0, 0};
  float* w_wino_dev = nullptr;             // 3x3 conv, N tile 32 or 64 (fused stem: its second conv): Winograd F(2,3) weights derived on the device from w_dev
  float* wd_wino_dev[2] = {nullptr, nullptr};  // ... and from wd_dev (data gradient)
  float* w_stem2_dev = nullptr;            // fused stem: F(2x2,3x3) weights of the second conv
  float* w_w16_dev = nullptr;              // 3x3 conv, Cout 16 / 32, Cin 16 / 32: wave-private F(2x2,3x3) weights derived from w_dev
  float* wd_w16_dev[2] = {nullptr, nullptr};  // ... and from wd_dev (data gradient)
  float* w_wino2_dev = nullptr;            // 3x3 conv, N tile 64: Winograd F(2x2,3x3) weights derived from w_dev
  float* wd_wino2_dev[2] = {nullptr, nullptr};  // ... and from wd_dev (data gradient)
  float* w_n64_dev = nullptr;              // 3x3 conv with 32 output channels and >= 64 input channels: the weights packed once more for an N tile of 64 (upper half zeros) ...
  float* b_n64_dev = nullptr;              // ... with a 64-entry bias, so that the layer can run on the F(2x2,3x3) kernel's half-empty-N-tile form (w_wino2_dev is derived from w_n64_dev)
  float* w_sm_dev = nullptr;               // 3x3 conv: small-map F(2x2,3x3) weights derived from w_dev (conv3x3_sm_kernel)
  float* w_wino4_dev = nullptr;            // 3x3 conv, N tile 64, >= 64 padded input channels: Winograd F(4x4,3x3) weights derived from w_dev (w_n64_dev where that exists)
  float* wd_wino4_dev[2] = {nullptr, nullptr};  // ... and from wd_dev (data gradient: Cout input channels)
  // ConvTranspose2d(k3, s2, p1, op1) as four output-phase row GEMMs (mode 3) + its data gradient (mode 4)
  float* wt_phase_dev[4] = {nullptr, nullptr, nullptr, nullptr};
  float* bt_dev = nullptr;       // bias padded to the GEMM's N tiles
  float* wt_dgrad_dev = nullptr; // 3x3 stride-2 conv weights (out = cin0, in = cout) in the row-GEMM layout
  float* wt_scale_dev = nullptr; // optional folded-BatchNorm scale / shift (weight2 / bias2), padded like bt_dev
  float* wt_shift_dev = nullptr;
  int bn_t = 0, bn_td = 0;
  float* w_f16_dev[2] = {nullptr, nullptr};  // 3x3 conv / transposed conv on the fp16 matrix pipe: [0] split-fp16, [1] plain fp16 weights (derived lazily from w_dma_dev)
  void* w_cnx_f16_dev = nullptr;  // Linear / 2x2-stride-2 conv on the fp16 matrix pipe: gemm_f16_kernel's weight image (derived from w_dma_dev at ph_model_create)
  float* w16_dev = nullptr;   // 16 -> 16 channel 3x3 conv: [tap][ci][co] for conv3x3_c16_kernel
  float* wd16_dev = nullptr;  // ... and of its data gradient
};

// One packed device buffer and the gather map that rebuilds it from the canonical parameter arena
// (map[i] = index into the arena, -1 = structural zero).
struct PackedBuffer {
  float* dst = nullptr;
  int* map = nullptr;
  size_t n = 0;
};

// The forms derived on the device from a packed buffer (not pure gathers of parameters: Winograd transforms, fp16 images).  What each kind is -- its size, the launch
// that computes it, the meaning of DerivedBuffer::p[] -- stands once, in the table of weights.hip.
enum DerivedKind {
  DERIVED_WINO = 0,            // Winograd F(2,3) transform of a 3x3 conv's packing
  DERIVED_F16_PACK = 1,        // fp16 weight pack of the LDS-DMA panels
  DERIVED_WINO2D = 2,          // F(2x2,3x3) transform
  DERIVED_W16 = 3,             // wave-private F(2x2,3x3) transform
  DERIVED_STEM_WINO2D = 4,     // the fused stem's second conv: F(2x2,3x3) transform
  DERIVED_WINO4 = 5,           // F(4x4,3x3) transform
  DERIVED_SMALLMAP = 6,        // small-map F(2x2,3x3) transform
  DERIVED_GEMM_F16_IMAGE = 7,  // fp16 row-GEMM weight image of a Linear / 2x2-stride-2 conv
  DERIVED_STEM_WINO = 8,       // the fused stem's second conv: F(2,3) transform
  DERIVED_KINDS
};

// Who reads a derived form, i.e. when ph_model_set_params recomputes it (reads_forms in weights.hip is the rule)
enum RefreshClass {
  REFRESH_ALWAYS = 0,  // every ph_model_set_params, a launch of its own
  REFRESH_BATCHED,     // every ph_model_set_params, as a segment of the kind's one multi-buffer launch
  REFRESH_INFERENCE,   // only while the handle's options let a plan read it (F(4x4,3x3), small-map: inference plans); else left stale
  REFRESH_F16_GEMM,    // only on a Linear program's plain-fp16 pipe (convnext_f16 / swint_f16); else left stale
  REFRESH_CLASSES
};

struct DerivedBuffer {
  const float* src = nullptr;
  float* dst = nullptr;
  DerivedKind kind = DERIVED_WINO;
  int p[5] = {0, 0, 0, 0, 0};  // the kind's parameters, in the order its table entry names them
};

struct SlotShape {
  int c = 0, cp = 0, h = 0, w = 0;  // cp: channels padded for the plan's format
  int64_t offset = -1;
  int def_op = -1;                  // index of the op that writes the slot
};

// One workspace byte range a launch of the last forward was handed (ph_model_last_ranges).
struct RangeRec {
  int op = 0, launch = 0, is_dst = 0;  // op index in the program, launch ordinal within that op, 0 = source | 1 = destination
  int slot = -1;                       // activation slot the range belongs to (-1: the scratch region behind the slots)
  int64_t offset = 0, bytes = 0;
};

struct Plan {
  std::vector<SlotShape> slots;
  int64_t tmp_offset = 0, tmp_bytes = 0, total = 0;
  bool reuse = false;  // slots share memory by lifetime (handle option workspace_reuse)
  bool recycle = false;  // ... and their ranges really are handed on (workspace_reuse 1).  reuse without recycle (workspace_reuse 2): the inference plan's routing and fusions with every slot in a range of its own, so that ph_model_read_slot can read what the fused launches read and wrote
  std::vector<char> unread;  // reuse plans: slot has no reader in the program (a fused conv+pool's full-resolution output the decoder never taps)
  int fmt = FMT_F32;  // activation format of every slot (act_format.h)
  int bpc = 4;        // bytes per channel in that format
};

}  // namespace ph

struct ph_model {
  std::vector<ph::PackedOp> ops;
  int n_slots = 0, n_outputs = 0;
  std::vector<void*> allocs;
  void* gather_table_dev = nullptr;           // GatherSegment table of `packed` (ph_model_set_params: one gather launch for all of them)
  int gather_segments = 0;
  unsigned gather_blocks = 0;
  bool pack_tables_built = false;             // PackSegment tables of the F(2,3) [0] / F(2x2,3x3) [1] buffers in `derived`
  void* pack_table_dev[2] = {nullptr, nullptr};
  int pack_segments[2] = {0, 0};
  unsigned pack_blocks[2] = {0, 0};
  // last forward (for ph_model_read_slot)
  ph::Plan last_plan;
  char* last_ws = nullptr;
  int last_batch = 0;
  std::vector<int> last_variant;  // PH_KV_* code of the kernel each op of the last forward ran (ph_model_last_kernels)
  std::vector<int32_t> last_rows_plan;    // (R, Wt, MT, MG) of each op of the last forward that ran conv3x3_f16_rows_kernel, zeros elsewhere; written where fwd_conv_f16 decides (ph_model_last_rows_plans)
  std::vector<ph::RangeRec> last_ranges;  // workspace ranges each launch of the last forward read / wrote (ph_model_last_ranges)
  std::vector<hipEvent_t> bwd_ev;         // profiling on: [0] before the losses, [1 + 2 (n - 1 - i)] before op i's step of the reverse sweep, [2 + 2 (n - 1 - i)] between its weight- and data-gradient
                                          // launches (Linear ops; elsewhere recorded at once), [2 n + 1] after the sweep (ph_model_backward_profile_read)
  bool bwd_ev_recorded = false;
  std::vector<int> last_bwd_variant;      // PH_KV_* code of the kernel each op's step of the last ph_model_backward ran (ph_model_last_backward_kernels)
  std::vector<int32_t> last_bwd_route;    // PH_BR_* route word of each op's step of the last ph_model_backward, written where the step decides (ph_model_last_backward_routes)
  // ph_model_set_branch_scales: (branch_n, branch_batch) per-sample scales of the residual Linears' branches (stochastic depth), borrowed; nullptr = none
  const float* branch_scales = nullptr;
  // ph_model_set_input_norm: per-channel statistics of a PH_FLAG_PAD0_NORM patch stem (the checkpoint's image_mean / image_std buffers)
  float in_mean[4] = {0.f, 0.f, 0.f, 0.f};
  float in_std[4] = {1.f, 1.f, 1.f, 1.f};
  int branch_n = 0, branch_batch = 0;
  // optional per-op HIP-event timing (ph_model_set_profiling)
  bool profiling = false;
  bool events_pending = false;
  std::vector<hipEvent_t> ev;      // n_ops + 1 events: ev[i] before op i, ev[n_ops] after the last
  std::vector<double> op_ms;       // accumulated per op
  int profiled_forwards = 0;
  unsigned long long* clock_probe = nullptr;  // diagnostic buffer (ph_model_set_clock_probe)
  ph_comm* comm = nullptr;                    // ph_model_set_comm: ph_model_backward exchanges the gradient arena over it (two buckets on comm_stream)
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev[3] = {nullptr, nullptr, nullptr};  // tail final / sweep done (caller's stream) / exchange done (side stream)
  std::vector<hipEvent_t> comm_events_owned;
  hipEvent_t bucket_event = nullptr;          // recorded mid-backward when the arena tail is final (ph_model_set_bucket_event)
  float* zeros_dev = nullptr;                 // zero page for LDS-DMA halo padding
  unsigned* split_counters_dev = nullptr;     // PH_SPLIT_COUNTERS zeroed counters of the split-K launches' in-kernel second stage (a handle's forwards are serialised, as its plan / profiling state already requires)
  int conv_splitk_finish = 0;                 // "conv_splitk_finish": 0 (default) = splitk_reduce_kernel as a launch of its own; 1 = the last-arriving workgroup of a split-K unit runs the second stage in the same launch; 2 (round 5) = the unit's workgroups wait (bounded) for all slices and SHARE the second stage (claimed by atomic bits; the last arriver sweeps unclaimed shares: no deadlock).  All three bit-identical.  Measured (cfg1 forward): 299 us (0) / 391 (1: one workgroup adds up to 24 planes of its 64-KiB tile at one CU's memory rate) / 370 (2: the wait for the slowest slice + device-scope fences + remote reads of the other XCDs' planes cost more than the ~6-us launch that spreads the same bytes over the chip)
  std::vector<int64_t> weight_offset;          // canonical arena offset of weights[i] (ph_model_create order)
  std::vector<int64_t> weight_numel;
  int64_t n_params = 0;
  bool forms_stale[ph::REFRESH_CLASSES] = {};  // ph_model_set_params skipped the derived forms of this class (nothing the handle's options allow reads them): refresh_stale_weights derives them before their next use
  std::vector<ph::DerivedBuffer> derived;      // refreshed after the gathers of ph_model_set_params
  std::vector<ph::PackedBuffer> packed;        // every packed weight buffer, for ph_model_set_params
  // ---- per-handle options (ph_model_set_option); the library reads no environment variables
  int use_dma = 1;                            // "conv_dma": 0 selects the register-staged 3x3 kernel
  int dma32 = 1;                              // "conv_dma32": Cout <= 48 layers on the LDS-DMA kernel (BN = 32) instead of the register-staged one
  int conv_wino = 1;                          // "conv_wino": Winograd F(2,3) 3x3 kernels (2: N-tile-64 layers only, 0: direct 9-tap kernels)
  int conv_w16 = 1;                           // "conv_w16": Cout-32 / Cin-16-or-32 3x3 convs on the wave-private F(2x2,3x3) kernel
  int conv_wino2d = 1;                        // "conv_wino2d": N-tile-64 3x3 convs on the F(2x2,3x3) kernel (0: the F(2,3)-along-x kernel)
  int conv_wino4 = 1;                         // "conv_wino4": K-heavy N-tile-64 3x3 convs on the F(4x4,3x3) kernel: 1 in inference plans (workspace_reuse), 2 in every plan -- both where the route estimates it faster than F(2x2,3x3) (conv3x3_route.hip) --, 3 every plan and wherever the shape fits, 0 never
  int conv_wino4_min_cin = 64;                // "conv_wino4_min_cin": padded input channels (both sources) from which a layer takes that kernel
  int conv_n32_wino2d = 1;                    // "conv_n32_wino2d" (1: inference plans, 2: every plan, 0: never): Cout-32 layers with >= 64 input channels (the last decoder level of an output-stride-2 UNet: 96 -> 32) on the F(2x2,3x3) kernel with a half-empty N tile of 64 instead of the N-tile-32 F(2,3) kernel
  int block_fuse = 1;                         // "block_fuse"
  int grn_fuse = 0;                           // "grn_fuse": ConvNeXtV2 blocks on the fused GRN plan (sums of squares from the first Linear's epilogue, per-sample scaled weights for the second); 0 (default): grn_reduce_kernel + grn_apply_kernel -- measured faster, DESIGN 4.4e
  int pretrained_train = 0;                   // "pretrained_train": 1 = ph_model_backward accepts the ConvNeXtV2 ops that carry PH_FLAG_NO_TRAIN (PH_OP_GRN: convnextv2_train_kernels.hip; the PH_FLAG_PAD0_NORM stem); 0 (default): refused, as before those backward steps existed
  int bwd_frozen_ops = 0;                     // "bwd_frozen_ops": the first n ops of the program are frozen -- the reverse sweep of ph_model_backward runs no step for them and writes none of their gradients (the reference's freeze_encoder()); 0 (default): every op
  int mlp_fuse = 1;                           // "mlp_fuse": CNBlock's Linear -> GELU -> Linear -> scale + residual in one launch (cnblock_mlp_kernel) where the width fits
  int stem_f16mfma = 1;                       // "stem_f16mfma"
  int upsample_f16math = 1;                   // "upsample_f16math"
  int conv_f16_rows = 1;                      // "conv_f16_rows" (plain fp16: the row-tile kernel of f16_rows_kernels.hip; 1 where estimated faster, 2 wherever it fits, 0 never)
  int conv_f16_rows_pin = 0;                  // "conv_f16_rows_pin": R | Wt << 8 | MG << 16 -- f16_rows_plan considers only that tile (still under every constraint of the search; a layer it does not fit gets the normal search); 0 (default): the search
  int conv_smallmap = 1;                      // "conv_smallmap" (1: inference plans with conv_splitk = 1 (the automatic small-batch routing), where estimated faster; 2: every fp32 3x3 conv whose shape fits, any plan; 0: never): conv3x3_sm_kernel
  int conv_splitk = 1;                        // "conv_splitk" (1: where estimated faster, inference plans only; n >= 2: force n slices in every plan; 0: never): F(2x2,3x3) layers with fewer (pixel tile, N tile) units than half the CUs split K over workgroups + a fixed-order second stage (small batches); n >= 2 forces n slices, 0 never
  int upsample_fold = 1;                      // "upsample_fold": a bilinear x2 whose only reader is the next conv's second source is folded into that conv's F(4x4,3x3) input transform (inference plans)
  int dgrad_wino = 1;                         // "dgrad_wino": 0 = direct 9-tap kernels for the backward's data-gradient convs (A/B: ~7 % slower cfg3 step, same gradients to the digit)
  int stem_wino = 2;                          // "stem_wino"
  int conv_persist = 1;                       // "conv_persist"
  int conv_c16 = 1;                           // "conv_c16"
  int dma_stagger = 1;                        // "conv_dma_stagger"
  int gemm_late_split = 0;                    // "gemm_late_split"
  int gemm_persist2 = 0;                      // "gemm_persist2"
  int fuse_gelu_fwd = 1;                      // Linear -> GELU op pair: one GEMM whose epilogue writes both tensors (0: two kernels)
  int fuse_gelu_bwd = 1;                      // Linear data gradient multiplies by GELU' in its epilogue (0: separate kernel)
  int wgrad_wino = 1;                         // "wgrad_wino": 3x3 weight gradients in the Winograd F(2x2,3x3) domain (layers with >= 32 padded channels on both sides)
  int dw_ln_fuse = 1;                         // "dw_ln_fuse"
  int head_fuse = 1;                          // "head_fuse"
  int pool_peephole = 1;                      // "pool_peephole"
  int mask_fold = 1;                          // "mask_fold": max-pool backward applies the ReLU mask of the conv it closes (no separate mask pass there)
  int wgrad_rows = 0;                         // 3x3 weight gradients of wide layers as nine row-wgrad GEMMs (off by default: measured slower than the 32x32-tile kernel; 1 auto, 2 always)
  double gemm_fill_threshold_wino2d = 0.4;    // ... and when it is the F(2x2,3x3) kernel (fill counted on its 16x16-pixel tiles)
  double gemm_fill_threshold_wino = 0.5;      // ... and the (lower) break-even when the halo kernel is the Winograd one
  double gemm_fill_threshold = 0.8;           // 3x3 convs whose maps fill the 16x32 tiles less than this run as row GEMMs
  int workspace_reuse = 0;                    // "workspace_reuse": 1 = slots of an inference program share memory by lifetime (no read-back, no backward); 2 = the same plan (routing, fusions, stores skipped) with a range per slot: the slots a launch really wrote can be read back, a tensor a fusion keeps out of HBM holds nothing
  int convt_one_launch = 1;                   // "convt_one_launch": the four output-phase GEMMs of a transposed conv as ONE launch (grid.y = phase) instead of four (four launch floors at small batches)
  int convt_phase = 1;                        // "convt_phase": transposed convs as four phase GEMMs (0: zero-stuffing + 3x3 conv, 4x the FLOPs; A/B)
  int swint_f16 = 0;                          // "swint_f16": 1 = a Swin program under conv_precision 2 runs whole on fp16 activations (swin_f16_kernels.hip + the fp16 row GEMM / LayerNorm); 0 (default) = exact fp32
  int convnext_f16 = 0;                       // "convnext_f16": 1 = a ConvNeXt program under conv_precision 2 runs whole on fp16 activations (convnext_f16_kernels.hip); 0 (default) = it runs exact fp32, as before the fp16 ConvNeXt kernels existed
  int conv_precision = 0;                     // "conv_precision": 0 exact fp32 MFMA; 1 split-fp16 MFMA (22-bit products, fp32 accumulate); 2 plain fp16 (autocast-equivalent)
  // ph_model_set_head_loss: loss of output i in ph_model_backward (0 = never set: MSE / cross entropy as the flags say, PH_FLAG_NO_TRAIN heads refused)
  int head_loss_kind[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float head_loss_params[8][4] = {};          // PH_LOSS_BCE_DICE: bce_weight, dice_weight, smooth, pos_weight (< 0: none)
};


namespace ph {
int build_plan(const ph_model* m, int B, int H, int W, Plan& plan, int fmt = FMT_F32);
int forward_format(const ph_model* m);  // format the forward of this program runs in under the handle's conv_precision
int drain_events(ph_model* m);  // profiling: fold the events of the last forward into op_ms
bool has_other_reader(const ph_model* m, int slot, size_t except_op);  // an op other than `except_op` reads `slot`
int bucket_split_op(const ph_model* m, int64_t* offset_out);  // train.hip: the op whose backward step makes the arena tail [*offset_out, n_params) final; -1 = no clean split
// Run-time fusions in which the launch of op i also computes op i + 1 (or leaves op i to the launch of op i + 1), so that a dst is written while an earlier op's sources are
// still being read.  Conditions on the program, the handle options and the plan only -- what is known before any weight form is derived; defined in plan.hip.  fuses_block2 and
// fuses_grn are called by BOTH the router (forward.hip, which fuses) and build_plan (which holds the releases due at op i + 1 / extends the GELU output's lifetime): the two
// cannot drift apart.  The others are the router's alone -- fuses_mlp: cnblock_mlp_kernel is safe with y exactly on x, build_plan does not hold that pair, and fwd_linear_mlp
// refuses the fusion for any other overlap of the plan's ranges; the rest: build_plan covers them by the kinds of the two ops (its `forwarded` rule), not by these predicates.
bool fuses_block2(const ph_model* m, size_t i, int fmt, bool reuse);  // block2_c32_f16_kernel: conv(<= 16 -> 32) + conv(32 -> 32) (+ pool)
bool fuses_mlp(const ph_model* m, size_t i, int fmt, bool reuse);     // cnblock_mlp_kernel: Linear + GELU + Linear + layer scale + residual
bool fuses_grn(const ph_model* m, size_t i, int fmt);                 // fused GRN plan: Linear + GELU, GRN, residual Linear
bool fuses_pool(const ph_model* m, size_t i);                         // pool peephole: conv + ReLU writes the pool op behind it
bool fuses_layernorm(const ph_model* m, size_t i, bool reuse);        // the LayerNorm behind a patch stem / depthwise conv rides in that kernel
bool defers_upsample_f32(const ph_model* m, size_t i, const Plan& plan);  // a bilinear x2 left to the fp32 conv behind it
bool defers_upsample_f16(const ph_model* m, size_t i, const Plan& plan);  // ... to the fp16 row-tile conv behind it
// weights.hip
int ensure_f16_weights(ph_model* m, int plain, hipStream_t s);                      // the lazy fp16 packs of the 3x3 convs ([plain] = 0 split, 1 plain fp16), derived at the first forward that needs them
int refresh_stale_weights(ph_model* m, const Plan& plan, hipStream_t s);            // the forms ph_model_set_params left stale, before the first forward that reads them
int refresh_derived(ph_model* m, const float* params_flat_dev, hipStream_t s);      // the derived-form half of ph_model_set_params (+ the GRN bias fold)
void apply_conv_options(const ph_model* m, ConvArgs& a);
enum ConvPlanKind { CONV_PLAN_INFERENCE, CONV_PLAN_TRAIN_FWD, CONV_PLAN_DGRAD };  // whose launch: an inference plan's forward (workspace_reuse), a training plan's forward, a data gradient
void apply_conv_plan_options(const ph_model* m, ConvPlanKind kind, ConvArgs& a);  // after apply_conv_options: conv_wino4 / conv_smallmap / conv_splitk / dgrad_wino as that kind of launch reads them
// Whether head op `d` applies its sigmoid epilogue in `plan`.  A head whose loss is PH_LOSS_BCE_DICE emits LOGITS in the plans a backward can follow
// (exact fp32, every activation kept): the loss kernel supervises the logit, as the reference's training_step does (lightning_modules.py:3052-3075).
inline int head_sigmoid(const ph_model* m, const Plan& plan, const ph_op_desc& d) {
  if (!(d.flags & PH_FLAG_SIGMOID)) return 0;
  const bool trainable_plan = plan.fmt == FMT_F32 && !plan.reuse;
  return (trainable_plan && d.out_index >= 0 && d.out_index < 8 && m->head_loss_kind[d.out_index] == PH_LOSS_BCE_DICE) ? 0 : 1;
}
}  // namespace ph
