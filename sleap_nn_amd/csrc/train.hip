// Backward pass + parameter management of the network runtime (C ABI: ph_model_backward,
// ph_model_set_params, ph_model_num_params).  Together with ph_model_forward and ph_adam_step this
// is one training step of the reference's LightningModule.training_step
// (sleap_nn/training/lightning_modules.py:1850-1922: forward, per-head MSE (+OHKM), weighted sum,
// autograd backward) for UNet models with bilinear up-sampling; gradients come out in the
// reference's state_dict layout (OIHW arena) so that a flat RCCL all-reduce + Adam apply directly.
#include <algorithm>

#include "model_internal.h"
#include "train_kernels.h"

using namespace ph;

static_assert(PH_MAX_OUTPUTS == sizeof(ph_model::head_loss_kind) / sizeof(int), "ph_model keeps one head loss per possible output");

namespace {

struct BwdPlan {
  Plan act;                         // activation slots (same layout as the forward workspace)
  std::vector<int64_t> head_dy_off; // per output: NCHW dY buffer offset in the grad workspace
  int64_t scratch_off = 0, scratch_bytes = 0, total = 0;
  // Swin programs: the padded tokens' (3C) share of a qkv.bias gradient lives from the attention op's step until the qkv Linear's step (whose weight-gradient
  // GEMM owns the scratch) has written that bias gradient; the residual Linears' scaled output gradient (branch scales set) is an operand of that GEMM
  int64_t pad_off = -1, scaled_off = -1;
};

inline float ln_eps(const ph_op_desc& d) { return (d.flags & PH_FLAG_LN_EPS_1EM5) ? 1e-5f : 1e-6f; }

int build_bwd_plan(const ph_model* m, int B, int H, int W, BwdPlan& bp) {
  int rc = build_plan(m, B, H, W, bp.act);
  if (rc != PH_OK) return rc;
  int64_t off = bp.act.total;  // gradient slots mirror the activation slots one to one
  bp.head_dy_off.assign(m->n_outputs, -1);
  int64_t scratch = 0, pad_floats = 0, scaled_floats = 0;
  for (const PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    if (d.kind == PH_OP_STEM || (d.kind == PH_OP_CONV && d.dst2 >= 0)) {
      set_error("backward needs the unfused program (no stem / conv+pool fusion)");
      return PH_E_INVALID;
    }
    if (d.kind == PH_OP_CONV && d.ksize != 3 && !op.wdk_gemm_dev[0]) {
      set_error("backward of a %d x %d conv needs its data-gradient GEMM weights (model built by an older ph_model_create?)", d.ksize, d.ksize);
      return PH_E_INVALID;
    }
    if (d.kind == PH_OP_CONVT) {
      if (!op.wt_dgrad_dev || op.wt_scale_dev || (d.flags & PH_FLAG_SILU)) {
        set_error("backward of a transposed conv supports bias + ReLU (the reference's decoder); folded BatchNorm / SiLU are inference-only");
        return PH_E_INVALID;
      }
      const SlotShape& si = bp.act.slots[d.src0];
      scratch = std::max<int64_t>(scratch, row_wgrad_slab_floats(B * si.h * si.w, d.cin0, d.cout));
      scratch = std::max<int64_t>(scratch, bias_scratch_floats(pad16(d.cout)));
      continue;
    }
    if (d.kind == PH_OP_LINEAR && (d.flags & (PH_FLAG_GELU | PH_FLAG_SCALE_RESIDUAL))) {
      set_error("backward needs the unfused ConvNeXt program (GELU / layer-scale as ops of their own)");
      return PH_E_INVALID;
    }
    if (d.kind >= PH_OP_PATCH_STEM) {
      const SlotShape& so = bp.act.slots[d.dst];
      const int64_t npix = (int64_t)B * so.h * so.w;
      int64_t need = bias_scratch_floats(so.cp);
      switch (d.kind) {
        case PH_OP_PATCH_STEM: need = std::max(need, patch_stem_wgrad_scratch_floats(d.cin0, d.cout, d.ksize, npix)); break;
        case PH_OP_DWCONV: need = std::max(need, dwconv7_wgrad_scratch_floats(B, so.h, so.cp)); break;
        case PH_OP_LAYERNORM: need = std::max(need, 2 * npix + chan_reduce_scratch_floats(so.cp)); break;
        case PH_OP_LINEAR:
        case PH_OP_PATCH_CONV: need = std::max(need, row_wgrad_slab_floats((int)npix, d.cout, d.cin0)); break;
        case PH_OP_SCALE_ADD: need = std::max(need, chan_reduce_scratch_floats(so.cp)); break;
        case PH_OP_GRN: need = std::max(need, grn_bwd_scratch_floats(B, so.h * so.w, so.cp)); break;  // slice sums of x^2, g x, g; per-sample coefficients and parameter shares
        case PH_OP_PATCH_MERGE: need = std::max(need, 2 * npix + chan_reduce_scratch_floats(so.cp) + 2 * npix * so.cp); break;  // statistics, reduction partials, gather, its gradient
        case PH_OP_WINDOW_ATTN: {
          const SlotShape& si = bp.act.slots[d.src0];
          need = std::max(need, window_attn_bwd_scratch_floats(B, si.h, si.w, d.cout, d.cin1, d.ksize));
          pad_floats = std::max<int64_t>(pad_floats, d.cin0);
          break;
        }
        default: break;
      }
      if (d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_RESIDUAL)) scaled_floats = std::max<int64_t>(scaled_floats, npix * so.cp);
      scratch = std::max(scratch, need);
      continue;
    }
    if (d.kind == PH_OP_HEAD) {
      const SlotShape& s0 = bp.act.slots[d.src0];
      bp.head_dy_off[d.out_index] = off;
      off += align_up((int64_t)B * d.cout * s0.h * s0.w * 4, 256);
      scratch = std::max<int64_t>(scratch, head_bwd_scratch_floats(s0.cp, d.cout, (int64_t)B * s0.h * s0.w));
      scratch = std::max<int64_t>(scratch, loss_scratch_floats(d.cout) + 64);
      scratch = std::max<int64_t>(scratch, seg_loss_scratch_floats(B, d.cout));
    } else if (d.kind == PH_OP_CONV) {
      const SlotShape& s0 = bp.act.slots[d.src0];
      scratch = std::max<int64_t>(scratch, wgrad_slab_floats(d.cin0, d.cout, B, s0.h, s0.w));
      if (d.cin1 > 0) scratch = std::max<int64_t>(scratch, wgrad_slab_floats(d.cin1, d.cout, B, s0.h, s0.w));
      scratch = std::max<int64_t>(scratch, row_wgrad_slab_floats(B * s0.h * s0.w, d.cout, std::max(d.cin0, d.cin1)));
      scratch = std::max<int64_t>(scratch, bias_scratch_floats(pad16(d.cout)));
    } else if (d.kind == PH_OP_INPUT_CONV) {
      if (d.ksize != 3) scratch = std::max<int64_t>(scratch, patch_stem_wgrad_scratch_floats(d.cin0, d.cout, d.ksize, (int64_t)B * H * W));  // im2col + one row-wgrad GEMM
      scratch = std::max<int64_t>(scratch, input_wgrad_scratch_floats(d.cin0, d.cout));
      scratch = std::max<int64_t>(scratch, bias_scratch_floats(pad16(d.cout)));
    }
  }
  if (pad_floats > 0) {
    bp.pad_off = off;
    off += align_up(pad_floats * 4, 256);
  }
  if (scaled_floats > 0) {
    bp.scaled_off = off;
    off += align_up(scaled_floats * 4, 256);
  }
  bp.scratch_off = off;
  bp.scratch_bytes = align_up(scratch * 4, 256);
  bp.total = off + bp.scratch_bytes;
  return PH_OK;
}

}  // namespace

extern "C" {

int64_t ph_model_num_params(const ph_model* m) {
  if (!m) {
    set_error("ph_model_num_params: null model");
    return PH_E_INVALID;
  }
  return m->n_params;
}

int ph_model_set_params(ph_model* m, const float* params_flat_dev, void* stream) {
  PH_REQUIRE(m && params_flat_dev, "ph_model_set_params: null argument");
  if (!m->gather_table_dev && !m->packed.empty()) {  // built once: every packed buffer of the model is a segment of one launch
    std::vector<GatherSegment> seg;
    unsigned blocks = 0;
    for (const PackedBuffer& pb : m->packed) {
      if (pb.n == 0) continue;
      seg.push_back(GatherSegment{pb.map, pb.dst, pb.n, blocks});
      blocks += (unsigned)((pb.n + 1023) / 1024);
    }
    void* t = nullptr;
    PH_HIP_CHECK(hipMalloc(&t, seg.size() * sizeof(GatherSegment)));
    m->allocs.push_back(t);
    PH_HIP_CHECK(hipMemcpy(t, seg.data(), seg.size() * sizeof(GatherSegment), hipMemcpyHostToDevice));
    m->gather_table_dev = t;
    m->gather_segments = (int)seg.size();
    m->gather_blocks = blocks;
  }
  {
    int rc = launch_gather_multi(params_flat_dev, static_cast<const GatherSegment*>(m->gather_table_dev), m->gather_segments, m->gather_blocks, static_cast<hipStream_t>(stream));
    if (rc != PH_OK) return rc;
  }
  // derived buffers: the F(2,3) and F(2x2,3x3) transforms (most of them) each go in ONE table-driven launch, the rest one by one
  if (!m->pack_tables_built) {
    for (int kind = 0; kind < 2; ++kind) {
      std::vector<PackSegment> seg;
      unsigned blocks = 0;
      for (const DerivedBuffer& db : m->derived) {
        const bool mine = kind == 0 ? (db.kind == DERIVED_WINO && db.bn != 0) : db.kind == DERIVED_WINO2D;
        if (!mine) continue;
        const unsigned long long total = (unsigned long long)(kind == 0 ? wino_pack_floats(db.panels, db.bn) : wino2d_pack_floats(db.panels, db.bn));
        if (total == 0) continue;
        seg.push_back(PackSegment{db.src, db.dst, total, db.bn, blocks});
        blocks += (unsigned)((total + 1023) / 1024);
      }
      void* t = nullptr;
      if (!seg.empty()) {
        PH_HIP_CHECK(hipMalloc(&t, seg.size() * sizeof(PackSegment)));
        m->allocs.push_back(t);
        PH_HIP_CHECK(hipMemcpy(t, seg.data(), seg.size() * sizeof(PackSegment), hipMemcpyHostToDevice));
      }
      m->pack_table_dev[kind] = t;
      m->pack_segments[kind] = (int)seg.size();
      m->pack_blocks[kind] = blocks;
    }
    m->pack_tables_built = true;
  }
  {
    int rc = launch_wino_pack_multi(static_cast<const PackSegment*>(m->pack_table_dev[0]), m->pack_segments[0], m->pack_blocks[0], static_cast<hipStream_t>(stream));
    if (rc == PH_OK) rc = launch_wino2d_pack_multi(static_cast<const PackSegment*>(m->pack_table_dev[1]), m->pack_segments[1], m->pack_blocks[1], static_cast<hipStream_t>(stream));
    if (rc != PH_OK) return rc;
  }
  for (const DerivedBuffer& db : m->derived) {
    if ((db.kind == DERIVED_WINO && db.bn != 0) || db.kind == DERIVED_WINO2D) continue;  // in the two launches above
    if (db.kind == DERIVED_WINO4 || db.kind == DERIVED_SMALLMAP) {  // F(4x4,3x3) / small-map weights: only inference plans read them (conv_wino4 = conv_smallmap = 1) -- a training step does not pay for the re-derivation,
      if ((db.kind == DERIVED_WINO4 ? m->conv_wino4 : m->conv_smallmap) < 2 && !m->workspace_reuse) {  // the next forward that wants them refreshes them (ph_model_forward)
        m->wino4_stale = true;
        continue;
      }
      const int rc5 = db.kind == DERIVED_WINO4 ? launch_wino4_pack(db.src, db.dst, db.panels, db.bn, static_cast<hipStream_t>(stream)) : launch_sm_pack(db.src, db.dst, db.panels, db.bn, db.n_tiles, static_cast<hipStream_t>(stream));
      if (rc5 != PH_OK) return rc5;
      continue;
    }
    if (db.kind == DERIVED_GEMM_F16_IMAGE) {  // fp16 row-GEMM images: only a plain-fp16 forward reads them -- a training step does not pay for them, the next such forward refreshes them (ph_model_forward)
      if (m->conv_precision != 2 || !(m->convnext_f16 || m->swint_f16)) {
        m->cnx_f16_stale = true;
        continue;
      }
      const int rc7 = launch_gemm_f16_weight_image(db.src, db.dst, db.panels, db.n_tiles, fmt_cpad(FMT_F16, db.panels), fmt_cpad(FMT_F16, db.n_tiles), db.chunks0, db.bn, static_cast<hipStream_t>(stream));
      if (rc7 != PH_OK) return rc7;
      continue;
    }
    int rc = db.kind == DERIVED_F16_PACK ? launch_f16_weight_pack(db.src, db.dst, db.n_tiles, db.chunks0, db.chunks1, db.bn, db.plain, static_cast<hipStream_t>(stream))
             : db.kind == DERIVED_W16 ? launch_w16_pack(db.src, db.dst, db.panels, db.bn, static_cast<hipStream_t>(stream))
             : db.kind == DERIVED_STEM_WINO2D ? launch_stem_wino2d_pack(db.src, db.dst, static_cast<hipStream_t>(stream))
                            : launch_stem_wino_pack(db.src, db.dst, static_cast<hipStream_t>(stream));
    if (rc != PH_OK) return rc;
  }
  // fused GRN plan ("grn_fuse"): the constant term W2 grn.bias + b2 of a residual Linear behind a GRN op follows the parameters.  Only a program whose first Linear
  // carries the GELU can take that plan (fuses_grn), so an unfused (training) program never pays for this
  for (size_t i = 2; i < m->ops.size(); ++i) {
    const PackedOp& op = m->ops[i];
    const ph_op_desc& g = m->ops[i - 1].d;
    const ph_op_desc& l1 = m->ops[i - 2].d;
    if (!op.b_grn_dev || g.kind != PH_OP_GRN || !(l1.kind == PH_OP_LINEAR && l1.flags == PH_FLAG_GELU)) continue;
    int rc = launch_grn_fold_bias(params_flat_dev + m->weight_offset[op.d.weight], params_flat_dev + m->weight_offset[op.d.bias], params_flat_dev + m->weight_offset[g.bias], op.b_grn_dev,
                                  op.d.cout, op.d.cin0, static_cast<hipStream_t>(stream));
    if (rc != PH_OK) return rc;
  }
  return PH_OK;
}

// Smallest / largest arena offset an op's parameters start at (-1: the op has none).
static int64_t op_param_offset(const ph_model* m, const ph_op_desc& d, bool highest = false) {
  int64_t v = -1;
  for (int idx : {d.weight, d.bias, d.weight2, d.bias2})
    if (idx >= 0 && idx < (int)m->weight_offset.size()) v = v < 0 ? m->weight_offset[idx] : (highest ? std::max(v, m->weight_offset[idx]) : std::min(v, m->weight_offset[idx]));
  return v;
}

// The op (forward order) whose completion in the reverse sweep makes the arena tail [offset, n_params) final: the program's
// parameters lie in op order, so the candidates are the ops at which the arena splits cleanly; the one closest to the middle wins.
static int bucket_split_op(const ph_model* m, int64_t* offset_out) {
  const int n = (int)m->ops.size();
  std::vector<int64_t> off(n), hi(n);
  for (int i = 0; i < n; ++i) {
    off[i] = op_param_offset(m, m->ops[i].d);
    hi[i] = op_param_offset(m, m->ops[i].d, true);
  }
  int best = -1;
  int64_t best_off = m->n_params;
  for (int k = 1; k < n; ++k) {
    if (off[k] <= 0) continue;
    bool clean = true;
    for (int i = 0; i < n && clean; ++i)
      if (off[i] >= 0) clean = i < k ? hi[i] < off[k] : off[i] >= off[k];  // EVERY parameter of an earlier op (weight2 / bias2 too) lies below the split
    if (!clean) continue;
    if (best < 0 || std::llabs(2 * off[k] - m->n_params) < std::llabs(2 * best_off - m->n_params)) {
      best = k;
      best_off = off[k];
    }
  }
  if (offset_out) *offset_out = best_off;
  return best;
}

int64_t ph_model_grad_bucket_split(const ph_model* m) {
  if (!m) {
    set_error("ph_model_grad_bucket_split: null model");
    return PH_E_INVALID;
  }
  int64_t off = m->n_params;
  bucket_split_op(m, &off);
  return off;
}

int ph_model_set_bucket_event(ph_model* m, void* hip_event) {
  PH_REQUIRE(m, "ph_model_set_bucket_event: null model");
  m->bucket_event = static_cast<hipEvent_t>(hip_event);
  return PH_OK;
}

// Data-parallel training behind the C ABI: with a communicator attached, ph_model_backward exchanges the gradient arena itself -- the tail bucket [split, n_params) on
// `comm_stream` as soon as the sweep has finished it (the encoder's gradients are still being computed on the caller's stream), the head bucket behind the sweep -- and the
// caller's stream waits for both before ph_model_backward's work on it counts as done: the next thing enqueued there (ph_adam_step with grad_scale = 1 / world) sees the
// SUM over the ranks.  What DDP's bucketed all-reduce does in the reference (training/model_trainer.py:1751-1813 hands the model to Lightning's DDP strategy).
int ph_model_set_comm(ph_model* m, ph_comm* comm, void* comm_stream) {
  PH_REQUIRE(m, "ph_model_set_comm: null model");
  PH_REQUIRE(!comm || comm_stream, "ph_model_set_comm: a communicator needs a side stream of its own (not the stream ph_model_backward runs on)");
  m->comm = comm;
  m->comm_stream = static_cast<hipStream_t>(comm_stream);
  if (comm && !m->comm_ev[0]) {
    for (auto& e : m->comm_ev) PH_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    for (auto& e : m->comm_ev) m->comm_events_owned.push_back(e);
  }
  return PH_OK;
}

int64_t ph_model_backward_workspace_bytes(const ph_model* m, int32_t batch, int32_t height, int32_t width) {
  if (!m || batch <= 0 || height <= 0 || width <= 0) {
    set_error("ph_model_backward_workspace_bytes: bad arguments");
    return PH_E_INVALID;
  }
  BwdPlan bp;
  int rc = build_bwd_plan(m, batch, height, width, bp);
  if (rc != PH_OK) return rc;
  return bp.total;
}

int ph_model_backward(ph_model* m, const void* input_dev, int32_t in_dtype, int32_t batch, int32_t in_channels, int32_t height, int32_t width,
                      const void* act_workspace_dev, void* grad_workspace_dev, int64_t grad_workspace_bytes, const float* const* head_out_dev,
                      const float* const* target_dev, const float* loss_weights_host, const float* sample_weights_dev, int32_t ohkm_enabled, float hard_to_easy_ratio,
                      int32_t min_hard_keypoints, int32_t max_hard_keypoints, float ohkm_loss_scale, float* loss_dev, float* grads_flat_dev, void* stream) {
  PH_REQUIRE(m && input_dev && act_workspace_dev && grad_workspace_dev && head_out_dev && target_dev && loss_weights_host && loss_dev && grads_flat_dev,
             "ph_model_backward: null argument");
  PH_REQUIRE(((uintptr_t)grad_workspace_dev & 255) == 0, "gradient workspace must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  // per-sample branch scales (ph_model_set_branch_scales): residual Linear i of the program (in program order) is scaled by row i
  std::vector<int> branch_of(m->ops.size(), -1);
  {
    int n_res = 0;
    for (size_t i = 0; i < m->ops.size(); ++i)
      if (m->ops[i].d.kind == PH_OP_LINEAR && (m->ops[i].d.flags & PH_FLAG_RESIDUAL)) branch_of[i] = n_res++;
    PH_REQUIRE(!m->branch_scales || (m->branch_n == n_res && m->branch_batch == batch),
               "ph_model_backward: branch scales are set for %d branches x batch %d, the step has %d x %d", m->branch_n, m->branch_batch, n_res, batch);
  }
  m->last_bwd_variant.assign(m->ops.size(), PH_KV_NONE);
  const size_t n_ops = m->ops.size();
  const bool prof = m->profiling;  // per-op events of this sweep (ph_model_backward_profile_read)
  if (prof && m->bwd_ev.size() != 2 * n_ops + 2) {
    for (auto& e : m->bwd_ev) (void)hipEventDestroy(e);
    m->bwd_ev.assign(2 * n_ops + 2, nullptr);
    for (auto& e : m->bwd_ev) PH_HIP_CHECK(hipEventCreate(&e));
  }
  m->bwd_ev_recorded = false;
  for (const auto& op : m->ops) {  // the MSE / cross-entropy gradients below are not these heads' losses: they train only with a loss chosen by ph_model_set_head_loss
    if (op.d.kind != PH_OP_HEAD) continue;
    PH_REQUIRE(op.d.out_index >= 0 && op.d.out_index < PH_MAX_OUTPUTS, "ph_model_backward: head output index %d out of range", op.d.out_index);
    PH_REQUIRE(!((op.d.flags & PH_FLAG_NO_TRAIN) && m->head_loss_kind[op.d.out_index] == 0),
               "ph_model_backward: head %d belongs to a segmentation model type, whose losses (BCE + Dice, masked smooth-L1) are not built: inference only", op.d.out_index);
  }
  for (const auto& op : m->ops)  // the ConvNeXtV2 ops (GRN, the padding-0 stem with input statistics) carry PH_FLAG_NO_TRAIN: their backward steps run on request only
    PH_REQUIRE(m->pretrained_train || !(op.d.kind != PH_OP_HEAD && (op.d.flags & PH_FLAG_NO_TRAIN)),
               "ph_model_backward: op kind %d is inference only on this handle (a 'pretrained' ConvNeXtV2 backbone trains with the handle option pretrained_train = 1)", op.d.kind);
  // frozen prefix ("bwd_frozen_ops"): ops [0, frozen) get no step.  The program is in topological order, so nothing a frozen op reads is written by a trainable one:
  // the trainable ops still leave their data gradients in the frozen ops' output slots (the skips), and nobody reads them
  const int frozen = std::max(0, std::min(m->bwd_frozen_ops, (int)m->ops.size()));
  PH_REQUIRE(m->last_plan.fmt == FMT_F32, "backward needs the activations of an exact-fp32 forward (handle option conv_precision = 0)");
  PH_REQUIRE(!m->last_plan.reuse, "backward needs every activation of the forward (handle option workspace_reuse = 0)");
  BwdPlan bp;
  int rc = build_bwd_plan(m, batch, height, width, bp);
  if (rc != PH_OK) return rc;
  if (bp.total > grad_workspace_bytes) {
    set_error("gradient workspace too small: need %lld bytes, got %lld", (long long)bp.total, (long long)grad_workspace_bytes);
    return PH_E_WORKSPACE;
  }
  const char* aws = static_cast<const char*>(act_workspace_dev);
  char* gws = static_cast<char*>(grad_workspace_dev);
  auto A = [&](int slot) { return reinterpret_cast<const float*>(aws + bp.act.slots[slot].offset); };
  auto G = [&](int slot) { return reinterpret_cast<float*>(gws + bp.act.slots[slot].offset); };
  float* scratch = reinterpret_cast<float*>(gws + bp.scratch_off);
  float* pad_vec = bp.pad_off >= 0 ? reinterpret_cast<float*>(gws + bp.pad_off) : nullptr;
  float* scaled_gy = bp.scaled_off >= 0 ? reinterpret_cast<float*>(gws + bp.scaled_off) : nullptr;
  int pad_bias = -1, pad_n = 0;  // weights[] index of the qkv.bias whose gradient still lacks the padded tokens' share (pad_vec), and its length
  std::vector<char> init(m->n_slots, 0);
  std::vector<char> fused_away(m->ops.size(), 0);
  // ReLU-mask folding: the gradient of a conv + ReLU output is complete when its FIRST consumer (program order = last in this sweep)
  // has added its share; when that consumer is a max pool, pool_bwd applies the mask itself (it reads the activation anyway) and the
  // conv's own step only reduces the bias gradient (handle option "mask_fold")
  std::vector<int> first_consumer(m->n_slots, -1), producer(m->n_slots, -1);
  std::vector<char> masked(m->n_slots, 0), bias_done(m->n_slots, 0);
  for (int oi = (int)m->ops.size() - 1; oi >= 0; --oi) {
    const ph_op_desc& d = m->ops[oi].d;
    if (d.src0 >= 0) first_consumer[d.src0] = oi;
    if (d.src1 >= 0) first_consumer[d.src1] = oi;
    if (d.dst >= 0) producer[d.dst] = oi;
  }
  OhkmParams ok;
  ok.enabled = ohkm_enabled;
  ok.hard_to_easy_ratio = hard_to_easy_ratio;
  ok.min_hard = min_hard_keypoints;
  ok.max_hard = max_hard_keypoints;
  ok.loss_scale = ohkm_loss_scale;

  if (prof) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[0], s));
  // ---- losses and head-output gradients (loss_dev: [0] = total, [1 + i] = head i)
  std::vector<float> lw(loss_weights_host, loss_weights_host + m->n_outputs);
  for (const PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    if (d.kind != PH_OP_HEAD) continue;
    const SlotShape& s0 = bp.act.slots[d.src0];
    PH_REQUIRE(head_out_dev[d.out_index] && target_dev[d.out_index], "head %d: null output/target", d.out_index);
    float* dy = reinterpret_cast<float*>(gws + bp.head_dy_off[d.out_index]);
    const int kind = m->head_loss_kind[d.out_index];
    const float* hp = m->head_loss_params[d.out_index];
    const int64_t plane = (int64_t)s0.h * s0.w;
    if (kind == PH_LOSS_BCE_DICE) {  // head_out_dev holds logits (head_sigmoid, model_internal.h); dy is the gradient wrt the logit
      PH_REQUIRE(d.cout == 1 && !(d.flags & PH_FLAG_SOFTMAX), "head %d: BCE + Dice needs a one-channel map head", d.out_index);
      rc = launch_bce_dice(head_out_dev[d.out_index], target_dev[d.out_index], batch, s0.h, s0.w, hp[0], hp[1], hp[2], hp[3], lw[d.out_index], scratch, dy,
                           loss_dev + 1 + d.out_index, s);
    } else if (kind == PH_LOSS_MASKED_SMOOTH_L1) {  // target_dev: (B, cout + 1, h, w), the last channel is the weight mask
      PH_REQUIRE(!(d.flags & (PH_FLAG_SOFTMAX | PH_FLAG_SIGMOID)), "head %d: masked smooth-L1 needs a linear map head", d.out_index);
      rc = launch_masked_smooth_l1(head_out_dev[d.out_index], target_dev[d.out_index], (d.cout + 1) * plane, target_dev[d.out_index] + d.cout * plane, (d.cout + 1) * plane,
                                   batch, d.cout, s0.h, s0.w, lw[d.out_index], scratch, dy, loss_dev + 1 + d.out_index, s);
    } else if (kind == PH_LOSS_MSE && (d.flags & PH_FLAG_NO_TRAIN)) {  // the centre head: plain nn.MSELoss (F.mse_loss, lightning_modules.py:3074)
      PH_REQUIRE(!(d.flags & (PH_FLAG_SOFTMAX | PH_FLAG_SIGMOID)), "head %d: MSE on a segmentation head needs a linear map head", d.out_index);
      rc = launch_loss(head_out_dev[d.out_index], target_dev[d.out_index], nullptr, batch, d.cout, s0.h, s0.w, lw[d.out_index], OhkmParams{}, scratch, dy,
                       loss_dev + 1 + d.out_index, s);
    } else if (d.flags & PH_FLAG_SOFTMAX)  // class-vector head: cross entropy on the softmax output, gradient wrt the logits
      rc = launch_class_ce(head_out_dev[d.out_index], target_dev[d.out_index], batch, d.cout, lw[d.out_index], dy, loss_dev + 1 + d.out_index, s);
    else
      rc = launch_loss(head_out_dev[d.out_index], target_dev[d.out_index], sample_weights_dev, batch, d.cout, s0.h, s0.w, lw[d.out_index], ok, scratch, dy,
                       loss_dev + 1 + d.out_index, s);
    if (rc != PH_OK) return rc;
  }
  // total = sum_h w_h * loss_h (the weights are a by-value kernel argument)
  rc = launch_total_loss(loss_dev + 1, lw.data(), m->n_outputs, loss_dev, s);
  if (rc != PH_OK) return rc;

  // ---- reverse sweep
  int64_t split_off = m->n_params;
  const bool exchange = m->comm != nullptr;  // (a communicator of ONE rank runs the same schedule: two in-place sums that change nothing -- what the single-GPU test exercises)
  const int split_op = (m->bucket_event || exchange) ? bucket_split_op(m, &split_off) : -1;
  if (split_op < 0) split_off = m->n_params;
  auto tail_final = [&]() -> int {  // gradients [bucket split, n_params) are final from here on
    if (m->bucket_event) PH_HIP_CHECK(hipEventRecord(m->bucket_event, s));
    if (exchange && split_off < m->n_params) {  // tail bucket: on the side stream, under the rest of the sweep
      PH_HIP_CHECK(hipEventRecord(m->comm_ev[0], s));
      PH_HIP_CHECK(hipStreamWaitEvent(m->comm_stream, m->comm_ev[0], 0));
      return ph_allreduce(m->comm, grads_flat_dev + split_off, m->n_params - split_off, m->comm_stream);
    }
    return PH_OK;
  };
  for (int oi = (int)m->ops.size() - 1; oi >= 0; --oi) {
    const PackedOp& op = m->ops[oi];
    const ph_op_desc& d = op.d;
    const size_t ev_i = 1 + 2 * (n_ops - 1 - (size_t)oi);
    if (prof) {
      PH_HIP_CHECK(hipEventRecord(m->bwd_ev[ev_i], s));
      if (d.kind != PH_OP_LINEAR && d.kind != PH_OP_PATCH_CONV) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[ev_i + 1], s));
    }
    // an op whose output no op reads (a ConvNeXtV2 stage norm whose map the decoder does not take: output stride 8) has no gradient to pass on: like a frozen op
    const bool dead = d.kind != PH_OP_HEAD && d.dst >= 0 && first_consumer[d.dst] < 0 && (d.dst2 < 0 || first_consumer[d.dst2] < 0);
    if (oi < frozen || dead) {  // no step: the gradients of its parameters stay as the caller left them
      if (prof && (d.kind == PH_OP_LINEAR || d.kind == PH_OP_PATCH_CONV)) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[ev_i + 1], s));
      if (oi == split_op) rc = tail_final();  // the split op lies in the frozen part: the tail was final when the last trainable op finished
      if (rc != PH_OK) return rc;
      continue;
    }
    switch (d.kind) {
      case PH_OP_HEAD: {
        const SlotShape& s0 = bp.act.slots[d.src0];
        const float* dy = reinterpret_cast<const float*>(gws + bp.head_dy_off[d.out_index]);
        // this head completes the gradient of a conv + ReLU output (its first consumer): that ReLU's mask, and the conv's bias gradient, ride in the stores
        const int pr = producer[d.src0];
        const bool fold = m->mask_fold && first_consumer[d.src0] == oi && pr >= 0 && m->ops[pr].d.kind == PH_OP_CONV && (m->ops[pr].d.flags & PH_FLAG_RELU) &&
                          head_bwd_can_fold(s0.cp, s0.h * s0.w);
        const bool sum_bias = fold && m->ops[pr].d.bias >= 0;
        rc = launch_head_bwd(dy, head_out_dev[d.out_index], head_sigmoid(m, m->last_plan, d), A(d.src0), op.w_dev, batch, s0.h * s0.w, d.cin0, s0.cp, d.cout,
                             init[d.src0], G(d.src0), grads_flat_dev + m->weight_offset[d.weight], d.bias >= 0 ? grads_flat_dev + m->weight_offset[d.bias] : nullptr,
                             scratch, s, fold ? A(d.src0) : nullptr, sum_bias ? grads_flat_dev + m->weight_offset[m->ops[pr].d.bias] : nullptr,
                             sum_bias ? m->ops[pr].d.cout : 0);
        init[d.src0] = 1;
        if (fold) masked[d.src0] = 1;
        bias_done[d.src0] = sum_bias ? 1 : 0;
        break;
      }
      case PH_OP_CONV: {
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "conv output slot %d received no gradient", d.dst);
        const size_t npix = (size_t)batch * so.h * so.w;
        if (masked[d.dst]) {  // the last contributor applied the ReLU mask already (and, if it was a max pool's backward, summed the bias gradient)
          if (d.bias >= 0 && !bias_done[d.dst]) {
            rc = launch_bias_grad(G(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
            if (rc != PH_OK) return rc;
          }
        } else if ((d.flags & PH_FLAG_RELU) && d.bias >= 0) {  // mask + bias gradient in one pass
          rc = launch_relu_mask_bias_grad(G(d.dst), A(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
          if (rc != PH_OK) return rc;
        } else {
          if (d.flags & PH_FLAG_RELU) {
            rc = launch_relu_mask(G(d.dst), A(d.dst), npix * so.cp, s);
            if (rc != PH_OK) return rc;
          }
          if (d.bias >= 0) {
            rc = launch_bias_grad(G(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
            if (rc != PH_OK) return rc;
          }
        }
        const int srcs[2] = {d.src0, d.src1}, parts[2] = {d.cin0, d.cin1}, offs[2] = {0, d.cin0};
        if (d.ksize != 3) {
          // k x k "same" conv (kernel_size 5 / 7 / 9, the 7 x 7 convs of a stem block; encoder_decoder.py:38-141,144-225): the weight gradient is
          // k^2 row-wgrad GEMMs (one per tap: rows = pixels, the x operand gathered at the tap's offset), the data gradient the same k^2-tap row
          // GEMM as the forward (mode 5) on the flipped, in/out-swapped weights, accumulating where the source already has a gradient
          for (int part = 0; part < 2; ++part) {
            if (parts[part] <= 0 || srcs[part] < 0) continue;
            const SlotShape& si = bp.act.slots[srcs[part]];
            for (int tap = 0; tap < d.ksize * d.ksize; ++tap) {
              RowWgradArgs w{};
              w.dy = G(d.dst);
              w.x = A(srcs[part]);
              w.slab = scratch;
              w.np = so.cp;
              w.kp = si.cp;
              w.M = (int)npix;
              w.patch = 2;
              w.ksize = d.ksize;
              w.tap = tap;
              w.H = so.h;
              w.W = so.w;
              rc = launch_row_wgrad_part(w, d.cout, parts[part], d.cin0 + d.cin1, offs[part], d.ksize * d.ksize, grads_flat_dev + m->weight_offset[d.weight], s);
              if (rc != PH_OK) return rc;
            }
            GemmArgs g{};
            g.src0 = G(d.dst);
            g.c0p = so.cp;
            g.wpack = op.wdk_gemm_dev[part];
            g.bias = op.zero_bias_dev;
            g.dst = G(srcs[part]);
            g.residual = init[srcs[part]] ? G(srcs[part]) : nullptr;
            g.zeros = m->zeros_dev;
            g.coutp = si.cp;
            g.bn = op.bn_dk[part];
            g.M = (int)npix;
            g.mode = 5;
            g.ksize = d.ksize;
            g.H = so.h;
            g.W = so.w;
            g.late_split = m->gemm_late_split;
            rc = launch_gemm(g, s);
            if (rc != PH_OK) return rc;
            init[srcs[part]] = 1;
          }
          break;
        }
        for (int part = 0; part < 2; ++part) {
          if (parts[part] <= 0 || srcs[part] < 0) continue;
          const SlotShape& si = bp.act.slots[srcs[part]];
          const double tile_fill = ((double)si.cp / ((si.cp + 127) / 128 * 128)) * ((double)so.cp / ((so.cp + 127) / 128 * 128));
          if (m->wgrad_rows == 2 || (m->wgrad_rows == 1 && si.cp >= 128 && so.cp >= 128 && tile_fill >= 0.8)) {
            // nine row-wgrad GEMMs (one per tap): 128x128 tiles on the MFMA instead of 32x32, for wide layers
            for (int tap = 0; tap < 9; ++tap) {
              RowWgradArgs w{};
              w.dy = G(d.dst);
              w.x = A(srcs[part]);
              w.slab = scratch;
              w.np = so.cp;
              w.kp = si.cp;
              w.M = (int)npix;
              w.patch = 2;
              w.tap = tap;
              w.H = so.h;
              w.W = so.w;
              rc = launch_row_wgrad_part(w, d.cout, parts[part], d.cin0 + d.cin1, offs[part], 9, grads_flat_dev + m->weight_offset[d.weight], s);
              if (rc != PH_OK) return rc;
            }
          } else {
            WgradArgs w{};
            w.x = A(srcs[part]);
            w.dy = G(d.dst);
            w.slab = scratch;
            w.cxp = si.cp;
            w.coutp = so.cp;
            w.B = batch;
            w.H = so.h;
            w.W = so.w;
            if (m->wgrad_wino && w.cxp == 16 && w.coutp == 16)
              rc = launch_wgrad16_wino(w, parts[part], d.cout, d.cin0 + d.cin1, offs[part], grads_flat_dev + m->weight_offset[d.weight], s);
            else if (m->wgrad_wino && w.coutp >= 32)
              rc = launch_wgrad_wino(w, parts[part], d.cout, d.cin0 + d.cin1, offs[part], grads_flat_dev + m->weight_offset[d.weight], s);
            else
              rc = launch_wgrad(w, parts[part], d.cout, d.cin0 + d.cin1, offs[part], grads_flat_dev + m->weight_offset[d.weight], s);
            if (rc != PH_OK) return rc;
          }
          // data gradient: conv3x3 of the masked output gradient with the flipped, swapped weights
          ConvArgs a{};
          a.src0 = G(d.dst);
          a.c0p = so.cp;
          a.src1 = nullptr;
          a.c1p = 0;
          a.wpack = op.wd_dev[part];
          a.wpack_dma = op.wd_dma_dev[part];
          a.wpack_wino = op.wd_wino_dev[part];
          a.wpack_wino2 = op.wd_wino2_dev[part];
          a.wpack_w16 = op.wd_w16_dev[part];
          a.wpack_wino4 = op.wd_wino4_dev[part];
          a.use_wino4 = m->conv_wino4 == 3 ? 2 : (m->conv_wino4 == 2 ? 1 : 0);  // (training plans keep every slot: the F(4x4,3x3) kernel runs in them only on request)
          a.w16 = op.wd16_dev;
          a.bias = op.zero_bias_dev;
          a.dst = G(srcs[part]);
          a.coutp = si.cp;
          a.B = batch;
          a.H = so.h;
          a.W = so.w;
          a.relu = 0;
          a.bn = op.bn_d[part];
          a.clock_probe = nullptr;
          a.zeros = m->zeros_dev;
          a.dst_pool = nullptr;
          apply_conv_options(m, a);
          if (!m->dgrad_wino) a.use_wino = 0;
          a.accumulate = init[srcs[part]];
          const bool dma = m->use_dma && (a.bn == 64 || m->dma32);
          {  // this launch completes the gradient of a conv + ReLU output and its kernel has a lane-local epilogue: that ReLU's mask rides there
            const int pr = producer[srcs[part]];
            const int pk = pr >= 0 ? m->ops[pr].d.kind : -1;
            if (m->mask_fold && dma && first_consumer[srcs[part]] == oi && (pk == PH_OP_CONV || pk == PH_OP_INPUT_CONV) && (m->ops[pr].d.flags & PH_FLAG_RELU) &&
                d.src0 != d.src1 && conv3x3_dma_honours_mask(a)) {
              a.relu_mask_src = A(srcs[part]);
              masked[srcs[part]] = 1;
            }
          }
          rc = dma ? launch_conv3x3_dma(a, s) : launch_conv3x3(a, s);
          if (rc != PH_OK) return rc;
          init[srcs[part]] = 1;
        }
        break;
      }
      case PH_OP_CONVT: {  // y = ReLU(ConvTranspose2d(x; Wt) + b), encoder_decoder.py:439-461
        const SlotShape& so = bp.act.slots[d.dst];
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "transposed conv output slot %d received no gradient", d.dst);
        const size_t npix = (size_t)batch * so.h * so.w;
        if (d.flags & PH_FLAG_RELU)
          rc = launch_relu_mask_bias_grad(G(d.dst), A(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
        else
          rc = launch_bias_grad(G(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
        // dWt[ci][co][ky][kx] = sum over input pixels (y, x) of x[y, x, ci] * dY[2y - 1 + ky, 2x - 1 + kx, co]: one row-wgrad GEMM per tap,
        // rows = input pixels, the dY operand gathered with stride 2 (patch 3); the result lands in the IOHW layout directly
        for (int tap = 0; tap < 9 && rc == PH_OK; ++tap) {
          RowWgradArgs w{};
          w.dy = A(d.src0);  // the "n" operand: input channels
          w.np = si.cp;
          w.x = G(d.dst);    // the gathered "k" operand: output channels
          w.kp = so.cp;
          w.slab = scratch;
          w.M = batch * si.h * si.w;
          w.patch = 3;
          w.tap = tap;
          w.H = so.h;
          w.W = so.w;
          rc = launch_row_wgrad(w, d.cin0, d.cout, 9, grads_flat_dev + m->weight_offset[d.weight], s);
        }
        if (rc != PH_OK) return rc;
        // dX = Conv2d(dY, Wt viewed as (out = cin0, in = cout, 3, 3), stride 2, pad 1): row GEMM mode 4
        GemmArgs g{};
        g.src0 = G(d.dst);
        g.c0p = so.cp;
        g.wpack = op.wt_dgrad_dev;
        g.bias = op.zero_bias_dev;
        g.dst = G(d.src0);
        g.residual = init[d.src0] ? G(d.src0) : nullptr;  // accumulate into a gradient that is already there
        g.zeros = m->zeros_dev;
        g.coutp = si.cp;
        g.bn = op.bn_td;
        g.M = batch * si.h * si.w;
        g.mode = 4;
        g.H = so.h;
        g.W = so.w;
        g.late_split = m->gemm_late_split;
        rc = launch_gemm(g, s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_INPUT_CONV: {
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "first conv output received no gradient");
        PH_REQUIRE(d.cin0 == in_channels, "input has %d channels, network expects %d", in_channels, d.cin0);
        const size_t npix = (size_t)batch * so.h * so.w;
        // (a masked gradient and a 3 x 3 kernel: the weight-gradient launch below reads every element anyway and sums the bias gradient in a spare column)
        const bool bias_in_wgrad = masked[d.dst] && d.bias >= 0 && d.ksize == 3 && !bias_done[d.dst];
        if (masked[d.dst]) {  // the last contributor applied the ReLU mask already
          if (d.bias >= 0 && !bias_done[d.dst] && !bias_in_wgrad) {
            rc = launch_bias_grad(G(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
            if (rc != PH_OK) return rc;
          }
        } else if ((d.flags & PH_FLAG_RELU) && d.bias >= 0) {  // mask + bias gradient in one pass
          rc = launch_relu_mask_bias_grad(G(d.dst), A(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
          if (rc != PH_OK) return rc;
        } else {
          if (d.flags & PH_FLAG_RELU) {
            rc = launch_relu_mask(G(d.dst), A(d.dst), npix * so.cp, s);
            if (rc != PH_OK) return rc;
          }
          if (d.bias >= 0) {
            rc = launch_bias_grad(G(d.dst), npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
            if (rc != PH_OK) return rc;
          }
        }
        if (d.ksize != 3)  // first k x k "same" conv: im2col of the image + one row-wgrad GEMM (as the ConvNeXt patch stem, padding k / 2, stride 1)
          rc = launch_patch_stem_wgrad(input_dev, in_dtype, G(d.dst), batch, d.cin0, height, width, so.h, so.w, d.ksize, 1, d.ksize / 2, so.cp, d.cout,
                                       grads_flat_dev + m->weight_offset[d.weight], scratch, s);
        else
          rc = launch_input_wgrad(input_dev, in_dtype, G(d.dst), batch, d.cin0, height, width, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.weight], scratch, s,
                                  bias_in_wgrad ? grads_flat_dev + m->weight_offset[d.bias] : nullptr);
        break;
      }
      case PH_OP_POOL: {
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "pool output slot %d received no gradient", d.dst);
        const int pr = producer[d.src0];
        const bool fold = m->mask_fold && first_consumer[d.src0] == oi && pr >= 0 && m->ops[pr].d.kind == PH_OP_CONV && (m->ops[pr].d.flags & PH_FLAG_RELU);
        // ... and, the gradient being complete and masked as it is stored, it is summed per channel on the way: the producer conv's bias gradient,
        // which its own step would otherwise read the whole tensor again for
        const bool sum_bias = fold && m->ops[pr].d.bias >= 0 && pool_bwd_can_sum_bias(si.cp);
        rc = launch_pool_bwd(G(d.dst), A(d.src0), batch, si.h, si.w, si.cp, init[d.src0], fold ? 1 : 0, G(d.src0),
                             sum_bias ? grads_flat_dev + m->weight_offset[m->ops[pr].d.bias] : nullptr, sum_bias ? m->ops[pr].d.cout : 0, scratch, s);
        init[d.src0] = 1;
        masked[d.src0] = fold ? 1 : 0;
        bias_done[d.src0] = sum_bias ? 1 : 0;
        break;
      }
      case PH_OP_UPSAMPLE: {
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "upsample output slot %d received no gradient", d.dst);
        rc = launch_upsample_bwd(G(d.dst), batch, si.h, si.w, si.cp, init[d.src0], G(d.src0), s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_SCALE_ADD: {  // y = s * u + x
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "scale-add output slot %d received no gradient", d.dst);
        const size_t npix = (size_t)batch * so.h * so.w;
        rc = launch_chan_reduce(G(d.dst), A(d.src0), nullptr, npix, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.weight], scratch, s);
        if (rc != PH_OK) return rc;
        PH_REQUIRE(!init[d.src0], "scale-add input slot %d already has a gradient", d.src0);
        rc = launch_scale_add_bwd(G(d.dst), op.w_dev, G(d.src0), G(d.src1), init[d.src1], so.cp, npix * so.cp, s);
        init[d.src0] = 1;
        init[d.src1] = 1;
        break;
      }
      case PH_OP_GELU: {
        if (fused_away[oi]) break;  // its consumer's data-gradient GEMM already wrote G(src0) through the GELU derivative
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "GELU output slot %d received no gradient", d.dst);
        rc = launch_gelu_bwd(G(d.dst), A(d.src0), G(d.src0), init[d.src0], (size_t)batch * so.h * so.w * so.cp, s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_LINEAR:
      case PH_OP_PATCH_CONV: {
        const SlotShape& so = bp.act.slots[d.dst];
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "GEMM output slot %d received no gradient", d.dst);
        PH_REQUIRE(!init[d.src0], "GEMM input slot %d already has a gradient (accumulation is not supported here)", d.src0);
        const bool patch = d.kind == PH_OP_PATCH_CONV;
        PH_REQUIRE(!patch || (si.h % 2 == 0 && si.w % 2 == 0), "2x2/stride-2 conv backward needs even input sizes");
        const int M = batch * so.h * so.w;
        const int taps = patch ? 4 : 1;
        // Linear fed by a GELU whose output nobody else reads (CNBlock: Linear -> GELU -> Linear): the data-gradient
        // GEMM multiplies by GELU'(pre-activation) in its epilogue and writes the GELU input's gradient directly,
        // so the GELU output's gradient never exists in HBM
        int gelu_op = -1;
        if (!patch && m->fuse_gelu_bwd) {
          int readers = 0;
          for (size_t j = 0; j < m->ops.size(); ++j) {
            const ph_op_desc& e = m->ops[j].d;
            if (e.src0 == d.src0 || e.src1 == d.src0) readers += 1;
            if ((int)j < oi && e.dst == d.src0 && e.kind == PH_OP_GELU) gelu_op = (int)j;
          }
          if (gelu_op >= 0 && (readers != 1 || init[m->ops[gelu_op].d.src0])) gelu_op = -1;
        }
        // a Linear layer's bias gradient (column sums of dY) comes out of its weight-gradient GEMM, which stages every dY row anyway
        const bool bias_in_wgrad = !patch && !(d.flags & PH_FLAG_RELU) && d.bias >= 0;
        // a residual Linear under branch scales: its weight, bias and data gradients see s[branch][b] * G(dst) (one scaling pass), its residual source the plain G(dst)
        const float* gy = G(d.dst);
        if (branch_of[oi] >= 0 && m->branch_scales) {
          PH_REQUIRE(scaled_gy, "backward plan has no region for the scaled gradient");
          rc = launch_scale_samples(G(d.dst), m->branch_scales + (size_t)branch_of[oi] * batch, scaled_gy, (size_t)so.h * so.w * so.cp, batch, s);
          if (rc != PH_OK) return rc;
          gy = scaled_gy;
        }
        if (d.flags & PH_FLAG_RELU)
          rc = launch_relu_mask_bias_grad(G(d.dst), A(d.dst), (size_t)M, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
        else if (!bias_in_wgrad && d.bias >= 0)  // (Linear(bias=False): Swin's patch-merging reduction has none)
          rc = launch_bias_grad(G(d.dst), (size_t)M, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
        for (int tap = 0; tap < taps && rc == PH_OK; ++tap) {
          RowWgradArgs w{};
          w.dy = gy;
          w.x = A(d.src0);
          w.slab = scratch;
          w.np = so.cp;
          w.kp = si.cp;
          w.M = M;
          if (bias_in_wgrad) {
            w.gb = grads_flat_dev + m->weight_offset[d.bias];
            w.gb_n = d.cout;
          }
          w.patch = patch ? 1 : 0;
          w.tap = tap;
          w.H = si.h;
          w.W = si.w;
          rc = launch_row_wgrad(w, d.cout, d.cin0, taps, grads_flat_dev + m->weight_offset[d.weight], s);
          if (rc != PH_OK) break;
          if (prof && tap == 0) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[ev_i + 1], s));  // (a 2x2-stride-2 conv interleaves its four taps: all but the first weight-gradient GEMM count as data gradient)
          GemmArgs g{};
          g.src0 = gy;
          g.c0p = so.cp;
          g.wpack = op.wd_gemm_dev[tap];
          g.bias = op.zero_bias_dev;
          g.dst = G(d.src0);
          g.zeros = m->zeros_dev;
          g.coutp = si.cp;
          g.bn = op.bn_dg;
          g.M = M;
          g.mode = 0;
          g.out_patch = patch ? 1 : 0;
          g.out_tap = tap;
          g.out_H = si.h;
          g.out_W = si.w;
          if (gelu_op >= 0) {
            g.dst = G(m->ops[gelu_op].d.src0);
            g.act = 3;
            g.aux = A(m->ops[gelu_op].d.src0);
          }
          rc = launch_gemm(g, s);
        }
        init[d.src0] = 1;
        if (gelu_op >= 0) {
          init[m->ops[gelu_op].d.src0] = 1;
          fused_away[gelu_op] = 1;
        }
        m->last_bwd_variant[oi] = PH_KV_ROWGEMM;
        if (rc == PH_OK && d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_RESIDUAL)) {  // dst = acc + bias + src1: the residual source takes G(dst) as it is
          rc = launch_grad_fanout(G(d.dst), G(d.src1), init[d.src1], (size_t)M * so.cp, s);
          init[d.src1] = 1;
        }
        if (rc == PH_OK && pad_bias >= 0 && d.kind == PH_OP_LINEAR && d.bias == pad_bias) {  // the qkv Linear has written qkv.bias's gradient: add the padded tokens' share
          rc = launch_vec_add(grads_flat_dev + m->weight_offset[d.bias], pad_vec, pad_n, s);
          pad_bias = -1;
        }
        break;
      }
      case PH_OP_WINDOW_ATTN: {
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "window attention output slot %d received no gradient", d.dst);
        PH_REQUIRE(!init[d.src0] && pad_bias < 0 && pad_vec, "window attention: the qkv slot %d must have the attention core as its only reader", d.src0);
        WindowAttnBwdArgs w{};
        w.qkv = A(d.src0);
        w.table = op.w_dev;
        w.qkv_bias = op.b_dev;
        w.gout = G(d.dst);
        w.gqkv = G(d.src0);
        w.gtable = grads_flat_dev + m->weight_offset[d.weight];
        w.gpad = pad_vec;
        w.scratch = scratch;
        w.B = batch;
        w.H = si.h;
        w.W = si.w;
        w.C = d.cout;
        w.heads = d.cin1;
        w.w = d.ksize;
        w.sh = d.ksize >= (si.h + d.ksize - 1) / d.ksize * d.ksize ? 0 : d.cmid;  // per axis, as the forward
        w.sw = d.ksize >= (si.w + d.ksize - 1) / d.ksize * d.ksize ? 0 : d.cmid;
        rc = launch_window_attn_bwd(w, s);
        m->last_bwd_variant[oi] = PH_KV_WINDOW_ATTN_BWD;
        init[d.src0] = 1;
        pad_bias = d.bias;
        pad_n = d.cin0;
        break;
      }
      case PH_OP_PATCH_MERGE: {  // dst = LayerNorm(gather(src0)) over 4C channels; the gathered tensor is rebuilt in scratch
        const SlotShape& so = bp.act.slots[d.dst];
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "patch merge output slot %d received no gradient", d.dst);
        const size_t npix = (size_t)batch * so.h * so.w;
        float* xg = scratch;
        float* gxg = xg + npix * so.cp;
        float* stats = gxg + npix * so.cp;
        float* red = stats + 2 * npix;
        rc = launch_patch_merge_gather(A(d.src0), xg, batch, si.h, si.w, d.cin0, s);
        if (rc != PH_OK) return rc;
        rc = launch_layernorm_bwd(xg, G(d.dst), op.w_dev, gxg, stats, 0, so.c, so.cp, npix, s, ln_eps(d));
        if (rc != PH_OK) return rc;
        rc = launch_chan_reduce(G(d.dst), xg, stats, npix, so.cp, so.c, grads_flat_dev + m->weight_offset[d.weight], red, s);
        if (rc != PH_OK) return rc;
        rc = launch_chan_reduce(G(d.dst), nullptr, nullptr, npix, so.cp, so.c, grads_flat_dev + m->weight_offset[d.bias], red, s);
        if (rc != PH_OK) return rc;
        rc = launch_patch_merge_scatter(gxg, G(d.src0), init[d.src0], batch, si.h, si.w, d.cin0, s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_LAYERNORM: {
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "LayerNorm output slot %d received no gradient", d.dst);
        const size_t npix = (size_t)batch * so.h * so.w;
        float* stats = scratch;
        float* red = scratch + 2 * npix;
        rc = launch_layernorm_bwd(A(d.src0), G(d.dst), op.w_dev, G(d.src0), stats, init[d.src0], so.c, so.cp, npix, s, ln_eps(d));
        if (rc != PH_OK) return rc;
        rc = launch_chan_reduce(G(d.dst), A(d.src0), stats, npix, so.cp, so.c, grads_flat_dev + m->weight_offset[d.weight], red, s);
        if (rc != PH_OK) return rc;
        rc = launch_chan_reduce(G(d.dst), nullptr, nullptr, npix, so.cp, so.c, grads_flat_dev + m->weight_offset[d.bias], red, s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_DWCONV: {
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "depthwise conv output slot %d received no gradient", d.dst);
        rc = launch_bias_grad(G(d.dst), (size_t)batch * so.h * so.w, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
        if (rc != PH_OK) return rc;
        rc = launch_dwconv7_wgrad(A(d.src0), G(d.dst), batch, so.h, so.w, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.weight], scratch, s);
        if (rc != PH_OK) return rc;
        DwConvArgs a{};
        a.src = G(d.dst);
        a.w = op.dw_flip_dev;
        a.bias = nullptr;
        a.dst = G(d.src0);
        a.cp = so.cp;
        a.B = batch;
        a.H = so.h;
        a.W = so.w;
        a.accumulate = init[d.src0];
        rc = launch_dwconv7(a, s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_GLOBAL_MAXPOOL: {
        const SlotShape& si = bp.act.slots[d.src0];
        PH_REQUIRE(init[d.dst], "global pool output slot %d received no gradient", d.dst);
        rc = launch_global_maxpool_bwd(A(d.src0), G(d.dst), batch, si.h * si.w, si.cp, init[d.src0], G(d.src0), s);
        init[d.src0] = 1;
        break;
      }
      case PH_OP_PATCH_STEM: {
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "stem output received no gradient");
        PH_REQUIRE(d.cin0 == in_channels, "input has %d channels, network expects %d", in_channels, d.cin0);
        rc = launch_bias_grad(G(d.dst), (size_t)batch * so.h * so.w, so.cp, d.cout, grads_flat_dev + m->weight_offset[d.bias], scratch, s);
        if (rc != PH_OK) return rc;
        if (d.flags & PH_FLAG_PAD0_NORM)  // ConvNeXtV2 embeddings: padding 0, patches of (x / 255 - mean) / std; the bias gradient above is the same
          rc = launch_patch_stem_wgrad_norm(input_dev, in_dtype, G(d.dst), batch, d.cin0, height, width, so.h, so.w, d.ksize, d.cmid, so.cp, d.cout, m->in_mean, m->in_std,
                                            grads_flat_dev + m->weight_offset[d.weight], scratch, s);
        else
          rc = launch_patch_stem_wgrad(input_dev, in_dtype, G(d.dst), batch, d.cin0, height, width, so.h, so.w, d.ksize, d.cmid, 1, so.cp, d.cout,
                                       grads_flat_dev + m->weight_offset[d.weight], scratch, s);
        break;
      }
      case PH_OP_GRN: {  // y = w (x N) + beta + x: convnextv2_train_kernels.hip
        const SlotShape& so = bp.act.slots[d.dst];
        PH_REQUIRE(init[d.dst], "GRN output slot %d received no gradient", d.dst);
        PH_REQUIRE(bp.act.slots[d.src0].cp == so.cp && so.c == d.cout, "GRN channel mismatch");
        GrnBwdArgs a{};
        a.x = A(d.src0);
        a.gy = G(d.dst);
        a.weight = op.w_dev;
        a.gx = G(d.src0);
        a.gw = grads_flat_dev + m->weight_offset[d.weight];
        a.gb = grads_flat_dev + m->weight_offset[d.bias];
        a.scratch = scratch;
        a.B = batch;
        a.HW = so.h * so.w;
        a.c = d.cout;
        a.cp = so.cp;
        a.accumulate = init[d.src0];
        rc = launch_grn_bwd(a, s);
        m->last_bwd_variant[oi] = PH_KV_GRN_BWD;
        init[d.src0] = 1;
        break;
      }
      default:
        set_error("backward: unsupported op kind %d", d.kind);
        rc = PH_E_INVALID;
    }
    if (rc != PH_OK) return rc;
    if (oi == split_op) {
      rc = tail_final();
      if (rc != PH_OK) return rc;
    }
  }
  PH_REQUIRE(pad_bias < 0, "window attention: no qkv Linear took the padded tokens' share of its bias gradient");
  if (prof) {
    PH_HIP_CHECK(hipEventRecord(m->bwd_ev[2 * n_ops + 1], s));
    m->bwd_ev_recorded = true;
  }
  if (m->bucket_event && split_op < 0) PH_HIP_CHECK(hipEventRecord(m->bucket_event, s));
  if (exchange) {  // head bucket (the whole arena when it does not split), then the caller's stream joins the side stream
    PH_HIP_CHECK(hipEventRecord(m->comm_ev[1], s));
    PH_HIP_CHECK(hipStreamWaitEvent(m->comm_stream, m->comm_ev[1], 0));
    rc = ph_allreduce(m->comm, grads_flat_dev, split_off, m->comm_stream);
    if (rc != PH_OK) return rc;
    PH_HIP_CHECK(hipEventRecord(m->comm_ev[2], m->comm_stream));
    PH_HIP_CHECK(hipStreamWaitEvent(s, m->comm_ev[2], 0));
  }
  return PH_OK;
}

int ph_model_set_branch_scales(ph_model* m, const float* scales_dev, int32_t n_branches, int32_t batch) {
  PH_REQUIRE(m, "ph_model_set_branch_scales: null model");
  if (!scales_dev) {
    m->branch_scales = nullptr;
    m->branch_n = m->branch_batch = 0;
    return PH_OK;
  }
  int n_res = 0;
  for (const auto& op : m->ops)
    if (op.d.kind == PH_OP_LINEAR && (op.d.flags & PH_FLAG_RESIDUAL)) n_res += 1;
  PH_REQUIRE(n_res > 0, "ph_model_set_branch_scales: the program has no residual Linear (PH_FLAG_RESIDUAL)");
  PH_REQUIRE(n_branches == n_res, "ph_model_set_branch_scales: %d branches given, the program has %d residual Linear ops", n_branches, n_res);
  PH_REQUIRE(batch > 0, "ph_model_set_branch_scales: batch %d", batch);
  m->branch_scales = scales_dev;
  m->branch_n = n_branches;
  m->branch_batch = batch;
  return PH_OK;
}

int64_t ph_model_backward_pad_vector(const ph_model* m, int32_t batch, int32_t height, int32_t width, int32_t* n_floats) {
  if (!m || batch <= 0 || height <= 0 || width <= 0) {
    set_error("ph_model_backward_pad_vector: bad arguments");
    return PH_E_INVALID;
  }
  BwdPlan bp;
  int rc = build_bwd_plan(m, batch, height, width, bp);
  if (rc != PH_OK) return rc;
  int n = 0;
  for (const auto& op : m->ops)
    if (op.d.kind == PH_OP_WINDOW_ATTN) {  // the sweep runs in reverse: the first attention op of the program is the last to write the region
      n = op.d.cin0;
      break;
    }
  if (bp.pad_off < 0 || n == 0) {
    set_error("ph_model_backward_pad_vector: the program has no window attention op");
    return PH_E_INVALID;
  }
  if (n_floats) *n_floats = n;
  return bp.pad_off;
}

int ph_model_backward_profile_read(ph_model* m, double* op_ms, double* op_ms_first, int32_t n_ops, double* loss_ms) {
  PH_REQUIRE(m && op_ms && op_ms_first && loss_ms, "ph_model_backward_profile_read: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_backward_profile_read: model has %d ops", (int)m->ops.size());
  PH_REQUIRE(m->bwd_ev_recorded && m->bwd_ev.size() == 2 * (size_t)n_ops + 2, "ph_model_backward_profile_read: no profiled ph_model_backward (ph_model_set_profiling first)");
  PH_HIP_CHECK(hipEventSynchronize(m->bwd_ev[2 * n_ops + 1]));
  float ms = 0.f;
  PH_HIP_CHECK(hipEventElapsedTime(&ms, m->bwd_ev[0], m->bwd_ev[1]));
  *loss_ms = ms;
  for (int i = 0; i < n_ops; ++i) {
    const size_t e = 1 + 2 * (size_t)(n_ops - 1 - i);
    PH_HIP_CHECK(hipEventElapsedTime(&ms, m->bwd_ev[e], m->bwd_ev[e + 1]));
    op_ms_first[i] = ms;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, m->bwd_ev[e], m->bwd_ev[e + 2]));
    op_ms[i] = ms;
  }
  return PH_OK;
}

int ph_model_last_backward_kernels(const ph_model* m, int32_t* codes, int32_t n_ops) {
  PH_REQUIRE(m && codes && n_ops >= 0, "ph_model_last_backward_kernels: bad arguments");
  for (int i = 0; i < n_ops; ++i) codes[i] = i < (int)m->last_bwd_variant.size() ? m->last_bwd_variant[i] : PH_KV_NONE;
  return PH_OK;
}

int ph_model_set_head_loss(ph_model* m, int32_t out_index, int32_t kind, const float* params, int32_t n_params) {
  PH_REQUIRE(m, "ph_model_set_head_loss: null model");
  PH_REQUIRE(out_index >= 0 && out_index < m->n_outputs && out_index < PH_MAX_OUTPUTS, "ph_model_set_head_loss: output %d of %d", out_index, m->n_outputs);
  PH_REQUIRE(kind == PH_LOSS_MSE || kind == PH_LOSS_BCE_DICE || kind == PH_LOSS_MASKED_SMOOTH_L1, "ph_model_set_head_loss: unknown loss kind %d", kind);
  PH_REQUIRE(n_params == (kind == PH_LOSS_BCE_DICE ? 4 : 0) && (n_params == 0 || params), "ph_model_set_head_loss: loss kind %d takes %d parameters, got %d", kind,
             kind == PH_LOSS_BCE_DICE ? 4 : 0, n_params);
  for (const auto& op : m->ops) {
    if (op.d.kind != PH_OP_HEAD || op.d.out_index != out_index) continue;
    PH_REQUIRE(kind != PH_LOSS_BCE_DICE || (op.d.cout == 1 && !(op.d.flags & PH_FLAG_SOFTMAX)), "ph_model_set_head_loss: BCE + Dice needs a one-channel map head");
    PH_REQUIRE(kind != PH_LOSS_MASKED_SMOOTH_L1 || !(op.d.flags & (PH_FLAG_SOFTMAX | PH_FLAG_SIGMOID)), "ph_model_set_head_loss: masked smooth-L1 needs a linear map head");
  }
  m->head_loss_kind[out_index] = kind;
  for (int i = 0; i < 4; ++i) m->head_loss_params[out_index][i] = i < n_params ? params[i] : 0.f;
  return PH_OK;
}

}  // extern "C"
