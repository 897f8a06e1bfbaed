// The backward launch sequence of the network path (C ABI: ph_model_backward, ph_model_backward_workspace_bytes, ph_model_backward_pad_vector): the losses, then one step
// routine per op kind (bwd_*) over one BackwardCtx, which carries the call's constants, the per-slot state of the reverse sweep and the notes one op's step leaves for a
// later op's.  Together with ph_model_forward and ph_adam_step this is one training step of the reference's LightningModule.training_step
// (sleap_nn/training/lightning_modules.py:1850-1922: forward, per-head MSE (+OHKM), weighted sum, autograd backward); gradients come out in the reference's state_dict
// layout (OIHW arena) so that a flat RCCL all-reduce + Adam apply directly.  Each step's scratch formula (bwd_*_scratch_floats) sits directly above the routine that
// consumes the scratch; build_bwd_plan takes the maximum over them.
#include <algorithm>

#include "model_internal.h"
#include "train_kernels.h"

using namespace ph;

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
inline bool is_residual_linear(const ph_op_desc& d) { return d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_RESIDUAL); }
inline bool is_row_gemm(const ph_op_desc& d) { return d.kind == PH_OP_LINEAR || d.kind == PH_OP_PATCH_CONV; }  // the two kinds bwd_linear serves

// The losses' inputs of one ph_model_backward call (bwd_losses)
struct LossArgs {
  const float* const* target_dev;
  const float* loss_weights_host;
  const float* sample_weights_dev;
  OhkmParams ohkm;
  float* loss_dev;  // [0] = total, [1 + i] = head i
};

struct BackwardCtx {
  // ---- constants of the call
  ph_model* const m;
  const BwdPlan& bp;
  const int batch, height, width, in_channels, in_dtype;
  const void* const input_dev;
  const char* const aws;  // activation workspace of the forward this backward follows
  char* const gws;        // gradient workspace: one gradient slot per activation slot, the heads' dY buffers, the pad vector, the scaled gradient, the scratch
  const float* const* const head_out_dev;
  float* const grads_flat_dev;
  const hipStream_t s;
  const bool prof;        // per-op events of this sweep (ph_model_backward_profile_read)
  // frozen prefix ("bwd_frozen_ops"): ops [0, frozen) get no step.  The program is in topological order, so nothing a frozen op reads is written by a trainable one:
  // the trainable ops still leave their data gradients in the frozen ops' output slots (the skips), and nobody reads them
  const int frozen;
  const int n_cu;         // CUs of the device, read once per call (the data-gradient convs' routes)
  std::vector<int> branch_of;  // per op: row of the per-sample branch scales (ph_model_set_branch_scales) -- residual Linear i of the program, in program order --, else -1
  // per slot: the first op (program order = last in this sweep) that reads it, and the op that writes it; -1 = none
  std::vector<int> first_consumer, producer;
  int split_op = -1;      // the op whose step makes the arena tail [split_off, n_params) final (bucket_split_op); -1: no mid-sweep event or exchange, or no clean split
  int64_t split_off = 0;  // = n_params where split_op < 0

  // ---- the sweep state.  "At rest" is what ph_model_backward leaves behind the last op; only pad_bias has a rest state to check
  int oi = -1;  // the op whose step runs (set by the sweep loop of ph_model_backward)
  // per slot: the gradient slot holds a gradient (the next contributor accumulates).  Set by every step for the slots it writes, read by every step: its dst must be
  // set, a source that is set makes the launch accumulate.  No rest state: a slot nobody consumed (a dead op's) stays 0
  std::vector<char> init;
  // per slot, ReLU-mask folding: the gradient of a conv + ReLU output is complete when its FIRST consumer has added its share; that consumer's launch can apply the mask
  // as it stores (handle option "mask_fold").  masked: set by bwd_head, bwd_pool and conv3x3_dgrad for their source slot; read by finish_output_grad (bwd_conv,
  // bwd_input_conv) for its own dst.  bias_done (the producer conv's bias gradient was summed on the way too): set by bwd_head and bwd_pool, read by
  // finish_output_grad and bwd_input_conv.  Neither is cleared: each slot's producer runs its step once
  std::vector<char> masked, bias_done;
  // per op: a GELU whose consumer's data-gradient GEMM already wrote the GELU input's gradient through the GELU derivative.  Set by bwd_linear, read by bwd_gelu
  // (which then launches nothing); not cleared, the GELU's step comes once
  std::vector<char> fused_away;
  // weights[] index of the qkv.bias whose gradient still lacks the padded tokens' share (pad_vec()), and its length.  Set by bwd_window_attn, cleared by bwd_linear
  // (the qkv Linear, once its weight-gradient GEMM has written that bias gradient).  At rest: pad_bias < 0 (ph_model_backward checks)
  int pad_bias = -1, pad_n = 0;

  // ---- profiling events of the current step: m->bwd_ev[ev_i] before it, [ev_i + 1] between its weight- and data-gradient launches, [ev_i + 2] before the next step
  size_t ev_i = 0;
  // bwd_linear calls this behind its first weight-gradient GEMM; for every other kind, and for a Linear that gets no step, the sweep loop records the mid event at once
  int mark_first_part() {
    if (prof) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[ev_i + 1], s));
    return PH_OK;
  }

  // ---- the route record of the current step (ph_model_last_backward_routes, PH_BR_* of posehip.h): each step notes a route in the branch that launches it
  void note(int32_t bits) { m->last_bwd_route[oi] |= bits; }
  void note_wgrad(int part, int route) { note(route << (PH_BR_PART_BITS * part)); }
  void note_dgrad(int part, int route, bool accumulate) { note((route << 4 | (accumulate ? PH_BR_ACCUMULATE : 0)) << (PH_BR_PART_BITS * part)); }
  void note_mask(int who) { note(who << PH_BR_MASK_SHIFT); }
  void note_bias(int who) { note(who << PH_BR_BIAS_SHIFT); }

  // ---- accessors
  const SlotShape& slot(int i) const { return bp.act.slots[i]; }
  const float* A(int i) const { return reinterpret_cast<const float*>(aws + bp.act.slots[i].offset); }  // activation of slot i
  float* G(int i) const { return reinterpret_cast<float*>(gws + bp.act.slots[i].offset); }              // gradient of slot i
  float* scratch() const { return reinterpret_cast<float*>(gws + bp.scratch_off); }
  float* pad_vec() const { return bp.pad_off >= 0 ? reinterpret_cast<float*>(gws + bp.pad_off) : nullptr; }
  float* scaled_gy() const { return bp.scaled_off >= 0 ? reinterpret_cast<float*>(gws + bp.scaled_off) : nullptr; }
  float* head_dy(int out_index) const { return reinterpret_cast<float*>(gws + bp.head_dy_off[out_index]); }
  float* grad_of(int weight) const { return grads_flat_dev + m->weight_offset[weight]; }  // arena gradient of weights[weight]
  size_t npix(const SlotShape& q) const { return (size_t)batch * q.h * q.w; }
  bool exchange() const { return m->comm != nullptr; }  // (a communicator of ONE rank runs the same schedule: two in-place sums that change nothing -- what the single-GPU test exercises)
  // The current step completes the gradient of slot `src` (it is the slot's first consumer) and the slot is the output of a `kind0` (or `kind1`) op with a ReLU: that
  // op, whose mask may then ride in this step's stores ("mask_fold"); else nullptr
  const ph_op_desc* relu_producer_closed_by(int src, int kind0, int kind1 = -1) const {
    const int pr = producer[src];
    if (!m->mask_fold || first_consumer[src] != oi || pr < 0) return nullptr;
    const ph_op_desc& p = m->ops[pr].d;
    return ((p.kind == kind0 || p.kind == kind1) && (p.flags & PH_FLAG_RELU)) ? &p : nullptr;
  }
};

// The program's read / write index, the branch rows and the bucket split of a fresh context
void index_program(BackwardCtx& c) {
  const ph_model* m = c.m;
  const size_t n_ops = m->ops.size();
  c.branch_of.assign(n_ops, -1);
  int n_res = 0;
  for (size_t i = 0; i < n_ops; ++i)
    if (is_residual_linear(m->ops[i].d)) c.branch_of[i] = n_res++;
  c.first_consumer.assign(m->n_slots, -1);
  c.producer.assign(m->n_slots, -1);
  for (int oi = (int)n_ops - 1; oi >= 0; --oi) {
    const ph_op_desc& d = m->ops[oi].d;
    if (d.src0 >= 0) c.first_consumer[d.src0] = oi;
    if (d.src1 >= 0) c.first_consumer[d.src1] = oi;
    if (d.dst >= 0) c.producer[d.dst] = oi;
  }
  c.init.assign(m->n_slots, 0);
  c.masked.assign(m->n_slots, 0);
  c.bias_done.assign(m->n_slots, 0);
  c.fused_away.assign(n_ops, 0);
  c.split_off = m->n_params;
  c.split_op = (m->bucket_event || c.exchange()) ? bucket_split_op(m, &c.split_off) : -1;
  if (c.split_op < 0) c.split_off = m->n_params;
}

// ---- shared launch helpers

// The "finish the output gradient" prologue of a conv's step (bwd_conv, bwd_input_conv): G(dst) holds every consumer's share; apply the ReLU mask unless the last
// contributor did, and reduce the bias gradient unless that contributor did or (`bias_elsewhere`) a later launch of the step will
int finish_output_grad(BackwardCtx& c, const ph_op_desc& d, bool bias_elsewhere) {
  const SlotShape& so = c.slot(d.dst);
  const size_t npix = c.npix(so);
  if (c.masked[d.dst]) {  // the last contributor applied the ReLU mask already (and, if it was a max pool's or a head's backward, may have summed the bias gradient)
    c.note_mask(PH_BR_MASK_EARLIER);
    if (d.bias >= 0 && c.bias_done[d.dst]) c.note_bias(PH_BR_BIAS_CLOSER);
    if (d.bias >= 0 && !c.bias_done[d.dst] && !bias_elsewhere) {
      c.note_bias(PH_BR_BIAS_OWN);
      return launch_bias_grad(c.G(d.dst), npix, so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
    }
    return PH_OK;
  }
  if ((d.flags & PH_FLAG_RELU) && d.bias >= 0) {  // mask + bias gradient in one pass
    c.note_mask(PH_BR_MASK_OWN);
    c.note_bias(PH_BR_BIAS_WITH_MASK);
    return launch_relu_mask_bias_grad(c.G(d.dst), c.A(d.dst), npix, so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  }
  if (d.flags & PH_FLAG_RELU) {
    c.note_mask(PH_BR_MASK_OWN);
    int rc = launch_relu_mask(c.G(d.dst), c.A(d.dst), npix * so.cp, c.s);
    if (rc != PH_OK) return rc;
  }
  if (d.bias >= 0) {
    c.note_bias(PH_BR_BIAS_OWN);
    return launch_bias_grad(c.G(d.dst), npix, so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  }
  return PH_OK;
}

// How a row-wgrad GEMM gathers the rows of its "k" operand (RowWgradArgs::patch, ksize, H, W), and where its result goes: the (n, k) block at input-channel offset
// k_off of a weight gradient whose input-channel axis is k_total wide and which has `taps` taps
struct TapGather {
  int patch, ksize, H, W;
};
struct WgradDst {
  float* grad;
  int n, k, k_total, k_off, taps;
};

// One tap of a weight gradient as a row-wgrad GEMM over M rows: fills the RowWgradArgs and launches.  dy (np padded channels) is the "n" operand, x (kp) the gathered "k"
// operand; gb: a Linear's bias gradient (gb_n channels) out of the same launch
int launch_wgrad_tap(BackwardCtx& c, const float* dy, int np, const float* x, int kp, int M, const TapGather& t, const WgradDst& to, int tap, float* gb = nullptr, int gb_n = 0) {
  RowWgradArgs w{};
  w.dy = dy;
  w.x = x;
  w.slab = c.scratch();
  w.np = np;
  w.kp = kp;
  w.M = M;
  w.gb = gb;
  w.gb_n = gb_n;
  w.patch = t.patch;
  w.ksize = t.ksize;
  w.tap = tap;
  w.H = t.H;
  w.W = t.W;
  return launch_row_wgrad_part(w, to.n, to.k, to.k_total, to.k_off, to.taps, to.grad, c.s);
}

// ---- the two-bucket exchange of the gradient arena

// Gradients [bucket split, n_params) are final from here on: the sweep loop calls this behind the split op's step
int bwd_tail_final(BackwardCtx& c) {
  ph_model* m = c.m;
  if (m->bucket_event) PH_HIP_CHECK(hipEventRecord(m->bucket_event, c.s));
  if (c.exchange() && c.split_off < m->n_params) {  // tail bucket: on the side stream, under the rest of the sweep
    PH_HIP_CHECK(hipEventRecord(m->comm_ev[0], c.s));
    PH_HIP_CHECK(hipStreamWaitEvent(m->comm_stream, m->comm_ev[0], 0));
    return ph_allreduce(m->comm, c.grads_flat_dev + c.split_off, m->n_params - c.split_off, m->comm_stream);
  }
  return PH_OK;
}

// Behind the sweep: the bucket event of an arena that does not split, the head bucket (the whole arena then), and the caller's stream joins the side stream
int bwd_head_bucket(BackwardCtx& c) {
  ph_model* m = c.m;
  if (m->bucket_event && c.split_op < 0) PH_HIP_CHECK(hipEventRecord(m->bucket_event, c.s));
  if (!c.exchange()) return PH_OK;
  PH_HIP_CHECK(hipEventRecord(m->comm_ev[1], c.s));
  PH_HIP_CHECK(hipStreamWaitEvent(m->comm_stream, m->comm_ev[1], 0));
  int rc = ph_allreduce(m->comm, c.grads_flat_dev, c.split_off, m->comm_stream);
  if (rc != PH_OK) return rc;
  PH_HIP_CHECK(hipEventRecord(m->comm_ev[2], m->comm_stream));
  PH_HIP_CHECK(hipStreamWaitEvent(c.s, m->comm_ev[2], 0));
  return PH_OK;
}

// ---- heads: losses, then the head's own step

int64_t bwd_head_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {  // (bwd_losses and bwd_head)
  const SlotShape& s0 = act.slots[d.src0];
  return std::max({head_bwd_scratch_floats(s0.cp, d.cout, (int64_t)B * s0.h * s0.w), loss_scratch_floats(d.cout) + 64, seg_loss_scratch_floats(B, d.cout)});
}

// Losses and head-output gradients (loss_dev: [0] = total, [1 + i] = head i)
int bwd_losses(BackwardCtx& c, const LossArgs& a) {
  const ph_model* m = c.m;
  std::vector<float> lw(a.loss_weights_host, a.loss_weights_host + m->n_outputs);
  for (const PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    if (d.kind != PH_OP_HEAD) continue;
    const SlotShape& s0 = c.slot(d.src0);
    const float* out = c.head_out_dev[d.out_index];
    const float* tgt = a.target_dev[d.out_index];
    PH_REQUIRE(out && tgt, "head %d: null output/target", d.out_index);
    float* dy = c.head_dy(d.out_index);
    float* loss = a.loss_dev + 1 + d.out_index;
    const int kind = m->head_loss_kind[d.out_index];
    const float* hp = m->head_loss_params[d.out_index];
    const int64_t plane = (int64_t)s0.h * s0.w;
    int rc;
    if (kind == PH_LOSS_BCE_DICE) {  // head_out_dev holds logits (head_sigmoid, model_internal.h); dy is the gradient wrt the logit
      PH_REQUIRE(d.cout == 1 && !(d.flags & PH_FLAG_SOFTMAX), "head %d: BCE + Dice needs a one-channel map head", d.out_index);
      rc = launch_bce_dice(out, tgt, c.batch, s0.h, s0.w, hp[0], hp[1], hp[2], hp[3], lw[d.out_index], c.scratch(), dy, loss, c.s);
    } else if (kind == PH_LOSS_MASKED_SMOOTH_L1) {  // target_dev: (B, cout + 1, h, w), the last channel is the weight mask
      PH_REQUIRE(!(d.flags & (PH_FLAG_SOFTMAX | PH_FLAG_SIGMOID)), "head %d: masked smooth-L1 needs a linear map head", d.out_index);
      rc = launch_masked_smooth_l1(out, tgt, (d.cout + 1) * plane, tgt + d.cout * plane, (d.cout + 1) * plane, c.batch, d.cout, s0.h, s0.w, lw[d.out_index], c.scratch(), dy, loss, c.s);
    } else if (kind == PH_LOSS_MSE && (d.flags & PH_FLAG_NO_TRAIN)) {  // the centre head: plain nn.MSELoss (F.mse_loss, lightning_modules.py:3074)
      PH_REQUIRE(!(d.flags & (PH_FLAG_SOFTMAX | PH_FLAG_SIGMOID)), "head %d: MSE on a segmentation head needs a linear map head", d.out_index);
      rc = launch_loss(out, tgt, nullptr, c.batch, d.cout, s0.h, s0.w, lw[d.out_index], OhkmParams{}, c.scratch(), dy, loss, c.s);
    } else if (d.flags & PH_FLAG_SOFTMAX)  // class-vector head: cross entropy on the softmax output, gradient wrt the logits
      rc = launch_class_ce(out, tgt, c.batch, d.cout, lw[d.out_index], dy, loss, c.s);
    else
      rc = launch_loss(out, tgt, a.sample_weights_dev, c.batch, d.cout, s0.h, s0.w, lw[d.out_index], a.ohkm, c.scratch(), dy, loss, c.s);
    if (rc != PH_OK) return rc;
  }
  // total = sum_h w_h * loss_h (the weights are a by-value kernel argument)
  return launch_total_loss(a.loss_dev + 1, lw.data(), m->n_outputs, a.loss_dev, c.s);
}

int bwd_head(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  // this head completes the gradient of a conv + ReLU output (its first consumer): that ReLU's mask, and the conv's bias gradient, ride in the stores
  const ph_op_desc* pr = c.relu_producer_closed_by(d.src0, PH_OP_CONV);
  const bool fold = pr && head_bwd_can_fold(s0.cp, s0.h * s0.w);
  const bool sum_bias = fold && pr->bias >= 0;
  int rc = launch_head_bwd(c.head_dy(d.out_index), c.head_out_dev[d.out_index], head_sigmoid(c.m, c.m->last_plan, d), c.A(d.src0), op.w_dev, c.batch, s0.h * s0.w, d.cin0, s0.cp,
                           d.cout, c.init[d.src0], c.G(d.src0), c.grad_of(d.weight), d.bias >= 0 ? c.grad_of(d.bias) : nullptr, c.scratch(), c.s, fold ? c.A(d.src0) : nullptr,
                           sum_bias ? c.grad_of(pr->bias) : nullptr, sum_bias ? pr->cout : 0);
  c.note((fold ? PH_BR_FOLDED_MASK : 0) | (sum_bias ? PH_BR_SUMMED_BIAS : 0));
  c.init[d.src0] = 1;
  if (fold) c.masked[d.src0] = 1;
  c.bias_done[d.src0] = sum_bias ? 1 : 0;
  return rc;
}

// ---- conv (3 x 3 and k x k "same", one or two concat sources)

int64_t bwd_conv_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {
  const SlotShape& s0 = act.slots[d.src0];
  int64_t need = wgrad_slab_floats(d.cin0, d.cout, B, s0.h, s0.w);
  if (d.cin1 > 0) need = std::max(need, wgrad_slab_floats(d.cin1, d.cout, B, s0.h, s0.w));
  need = std::max(need, row_wgrad_slab_floats(B * s0.h * s0.w, d.cout, std::max(d.cin0, d.cin1)));  // (the k x k path and "wgrad_rows")
  return std::max(need, bias_scratch_floats(pad16(d.cout)));
}

// Concat source `part` of a conv: its slot, its channels and where they start on the weight's input-channel axis
struct ConvPart {
  int src, cin, off;
  bool present() const { return cin > 0 && src >= 0; }
};
inline ConvPart conv_part(const ph_op_desc& d, int part) { return part == 0 ? ConvPart{d.src0, d.cin0, 0} : ConvPart{d.src1, d.cin1, d.cin0}; }

// The weight gradient of source `p` as k^2 row-wgrad GEMMs (one per tap: rows = pixels, the x operand gathered at the tap's offset)
int conv_wgrad_rows(BackwardCtx& c, const ph_op_desc& d, const ConvPart& p) {
  const SlotShape& so = c.slot(d.dst);
  const int taps = d.ksize * d.ksize;
  const WgradDst to{c.grad_of(d.weight), d.cout, p.cin, d.cin0 + d.cin1, p.off, taps};
  for (int tap = 0; tap < taps; ++tap) {
    int rc = launch_wgrad_tap(c, c.G(d.dst), so.cp, c.A(p.src), c.slot(p.src).cp, (int)c.npix(so), TapGather{2, d.ksize, so.h, so.w}, to, tap);
    if (rc != PH_OK) return rc;
  }
  return PH_OK;
}

// k x k "same" conv (kernel_size 5 / 7 / 9, the 7 x 7 convs of a stem block; encoder_decoder.py:38-141,144-225): the weight gradient is k^2 row-wgrad GEMMs, the data
// gradient the same k^2-tap row GEMM as the forward (mode 5) on the flipped, in/out-swapped weights, accumulating where the source already has a gradient
int bwd_conv_kxk(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  for (int part = 0; part < 2; ++part) {
    const ConvPart p = conv_part(d, part);
    if (!p.present()) continue;
    c.note_wgrad(part, PH_BR_WG_ROWSKK);
    int rc = conv_wgrad_rows(c, d, p);
    if (rc != PH_OK) return rc;
    c.note_dgrad(part, PH_BR_DG_GEMM5, c.init[p.src]);
    GemmArgs g{};
    g.src0 = c.G(d.dst);
    g.c0p = so.cp;
    g.wpack = op.wdk_gemm_dev[part];
    g.bias = op.zero_bias_dev;
    g.dst = c.G(p.src);
    g.residual = c.init[p.src] ? c.G(p.src) : nullptr;
    g.zeros = c.m->zeros_dev;
    g.coutp = c.slot(p.src).cp;
    g.bn = op.bn_dk[part];
    g.M = (int)c.npix(so);
    g.mode = 5;
    g.ksize = d.ksize;
    g.H = so.h;
    g.W = so.w;
    g.late_split = c.m->gemm_late_split;
    rc = launch_gemm(g, c.s);
    if (rc != PH_OK) return rc;
    c.init[p.src] = 1;
  }
  return PH_OK;
}

// 3 x 3 weight gradient of source `p`: nine row-wgrad GEMMs on 128x128 MFMA tiles for wide layers ("wgrad_rows"), else the 32x32-tile kernel, in the Winograd
// F(2x2,3x3) domain where "wgrad_wino" and the channel counts allow
int conv3x3_wgrad(BackwardCtx& c, const ph_op_desc& d, int part, const ConvPart& p) {
  const ph_model* m = c.m;
  const SlotShape& so = c.slot(d.dst);
  const SlotShape& si = c.slot(p.src);
  const double tile_fill = ((double)si.cp / ((si.cp + 127) / 128 * 128)) * ((double)so.cp / ((so.cp + 127) / 128 * 128));
  if (m->wgrad_rows == 2 || (m->wgrad_rows == 1 && si.cp >= 128 && so.cp >= 128 && tile_fill >= 0.8)) {
    c.note_wgrad(part, PH_BR_WG_ROWS9);
    return conv_wgrad_rows(c, d, p);
  }
  WgradArgs w{};
  w.x = c.A(p.src);
  w.dy = c.G(d.dst);
  w.slab = c.scratch();
  w.cxp = si.cp;
  w.coutp = so.cp;
  w.B = c.batch;
  w.H = so.h;
  w.W = so.w;
  if (m->wgrad_wino && w.cxp == 16 && w.coutp == 16) {
    c.note_wgrad(part, PH_BR_WG_WINO16);
    return launch_wgrad16_wino(w, p.cin, d.cout, d.cin0 + d.cin1, p.off, c.grad_of(d.weight), c.s);
  }
  if (m->wgrad_wino && w.coutp >= 32) {
    c.note_wgrad(part, PH_BR_WG_WINO);
    return launch_wgrad_wino(w, p.cin, d.cout, d.cin0 + d.cin1, p.off, c.grad_of(d.weight), c.s);
  }
  c.note_wgrad(part, PH_BR_WG_DIRECT);
  return launch_wgrad(w, p.cin, d.cout, d.cin0 + d.cin1, p.off, c.grad_of(d.weight), c.s);
}

// 3 x 3 data gradient of source `p` (concat part `part`): conv3x3 of the masked output gradient with the flipped, swapped weights
int conv3x3_dgrad(BackwardCtx& c, const PackedOp& op, int part, const ConvPart& p) {
  const ph_model* m = c.m;
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  ConvArgs a{};
  a.src0 = c.G(d.dst);
  a.c0p = so.cp;
  a.src1 = nullptr;
  a.c1p = 0;
  a.wpack = op.wd_dev[part];
  a.wpack_dma = op.wd_dma_dev[part];
  a.wpack_wino = op.wd_wino_dev[part];
  a.wpack_wino2 = op.wd_wino2_dev[part];
  a.wpack_w16 = op.wd_w16_dev[part];
  a.wpack_wino4 = op.wd_wino4_dev[part];
  a.w16 = op.wd16_dev;
  a.bias = op.zero_bias_dev;
  a.dst = c.G(p.src);
  a.coutp = c.slot(p.src).cp;
  a.B = c.batch;
  a.H = so.h;
  a.W = so.w;
  a.relu = 0;
  a.bn = op.bn_d[part];
  a.clock_probe = nullptr;
  a.zeros = m->zeros_dev;
  a.dst_pool = nullptr;
  apply_conv_options(m, a);
  apply_conv_plan_options(m, CONV_PLAN_DGRAD, a);  // (training plans keep every slot: the F(4x4,3x3) kernel runs in them only on request)
  a.accumulate = c.init[p.src];
  // this launch completes the gradient of a conv + ReLU output and its kernel has a lane-local epilogue: that ReLU's mask rides there
  if (c.relu_producer_closed_by(p.src, PH_OP_CONV, PH_OP_INPUT_CONV) && d.src0 != d.src1 && conv3x3_route(a, c.n_cu).takes_mask) {
    a.relu_mask_src = c.A(p.src);
    c.masked[p.src] = 1;
    c.note(PH_BR_FOLDED_MASK);
  }
  const ConvRoute r = conv3x3_route(a, c.n_cu);
  c.note_dgrad(part, r.kernel == CONV_REGSTAGED ? PH_BR_DG_REGSTAGED : r.kv, a.accumulate != 0);
  int rc = launch_conv3x3_routed(a, r, c.s);
  if (rc != PH_OK) return rc;
  c.init[p.src] = 1;
  return PH_OK;
}

int bwd_conv(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  PH_REQUIRE(c.init[d.dst], "conv output slot %d received no gradient", d.dst);
  int rc = finish_output_grad(c, d, false);
  if (rc != PH_OK) return rc;
  if (d.ksize != 3) return bwd_conv_kxk(c, op);
  for (int part = 0; part < 2; ++part) {
    const ConvPart p = conv_part(d, part);
    if (!p.present()) continue;
    rc = conv3x3_wgrad(c, d, part, p);
    if (rc != PH_OK) return rc;
    rc = conv3x3_dgrad(c, op, part, p);
    if (rc != PH_OK) return rc;
  }
  return PH_OK;
}

// ---- transposed conv: y = ReLU(ConvTranspose2d(x; Wt) + b), encoder_decoder.py:439-461

int64_t bwd_convt_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {
  return std::max(row_wgrad_slab_floats(B * act.slots[d.src0].h * act.slots[d.src0].w, d.cin0, d.cout), bias_scratch_floats(pad16(d.cout)));
}

int bwd_convt(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "transposed conv output slot %d received no gradient", d.dst);
  int rc;
  if (d.flags & PH_FLAG_RELU) {
    c.note_mask(PH_BR_MASK_OWN);
    c.note_bias(PH_BR_BIAS_WITH_MASK);
    rc = launch_relu_mask_bias_grad(c.G(d.dst), c.A(d.dst), c.npix(so), so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  } else {
    c.note_bias(PH_BR_BIAS_OWN);
    rc = launch_bias_grad(c.G(d.dst), c.npix(so), so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  }
  // dWt[ci][co][ky][kx] = sum over input pixels (y, x) of x[y, x, ci] * dY[2y - 1 + ky, 2x - 1 + kx, co]: one row-wgrad GEMM per tap, rows = input pixels, the dY
  // operand gathered with stride 2 (patch 3); the result lands in the IOHW layout directly.  The operands are exchanged: the "n" operand is the INPUT (input
  // channels), the gathered "k" operand the output gradient (output channels)
  const WgradDst to{c.grad_of(d.weight), d.cin0, d.cout, d.cout, 0, 9};
  c.note_wgrad(0, PH_BR_WG_CONVT_TAPS);
  for (int tap = 0; tap < 9 && rc == PH_OK; ++tap)
    rc = launch_wgrad_tap(c, /*n operand*/ c.A(d.src0), si.cp, /*gathered k operand*/ c.G(d.dst), so.cp, c.batch * si.h * si.w, TapGather{3, 3, so.h, so.w}, to, tap);
  if (rc != PH_OK) return rc;
  // dX = Conv2d(dY, Wt viewed as (out = cin0, in = cout, 3, 3), stride 2, pad 1): row GEMM mode 4
  GemmArgs g{};
  g.src0 = c.G(d.dst);
  g.c0p = so.cp;
  g.wpack = op.wt_dgrad_dev;
  g.bias = op.zero_bias_dev;
  g.dst = c.G(d.src0);
  g.residual = c.init[d.src0] ? c.G(d.src0) : nullptr;  // accumulate into a gradient that is already there
  g.zeros = c.m->zeros_dev;
  g.coutp = si.cp;
  g.bn = op.bn_td;
  g.M = c.batch * si.h * si.w;
  g.mode = 4;
  g.H = so.h;
  g.W = so.w;
  g.late_split = c.m->gemm_late_split;
  c.note_dgrad(0, PH_BR_DG_GEMM4, g.residual != nullptr);
  rc = launch_gemm(g, c.s);
  c.init[d.src0] = 1;
  return rc;
}

// ---- the first conv of a UNet (reads the image)

int64_t bwd_input_conv_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {
  const SlotShape& so = act.slots[d.dst];  // (stride 1, "same": the image's size)
  int64_t need = std::max(input_wgrad_scratch_floats(d.cin0, d.cout), bias_scratch_floats(pad16(d.cout)));
  if (d.ksize != 3) need = std::max(need, patch_stem_wgrad_scratch_floats(d.cin0, d.cout, d.ksize, (int64_t)B * so.h * so.w));  // im2col + one row-wgrad GEMM
  return need;
}

int bwd_input_conv(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "first conv output received no gradient");
  PH_REQUIRE(d.cin0 == c.in_channels, "input has %d channels, network expects %d", c.in_channels, d.cin0);
  // (a masked gradient and a 3 x 3 kernel: the weight-gradient launch below reads every element anyway and sums the bias gradient in a spare column)
  const bool bias_in_wgrad = c.masked[d.dst] && d.bias >= 0 && d.ksize == 3 && !c.bias_done[d.dst];
  int rc = finish_output_grad(c, d, bias_in_wgrad);
  if (rc != PH_OK) return rc;
  if (d.ksize != 3) {  // first k x k "same" conv: im2col of the image + one row-wgrad GEMM (as the ConvNeXt patch stem, padding k / 2, stride 1)
    c.note_wgrad(0, PH_BR_WG_PATCH_STEM);
    return launch_patch_stem_wgrad(c.input_dev, c.in_dtype, c.G(d.dst), c.batch, d.cin0, c.height, c.width, so.h, so.w, d.ksize, 1, d.ksize / 2, so.cp, d.cout, c.grad_of(d.weight),
                                   c.scratch(), c.s);
  }
  c.note_wgrad(0, PH_BR_WG_INPUT);
  if (bias_in_wgrad) c.note_bias(PH_BR_BIAS_INPUT_WGRAD);
  return launch_input_wgrad(c.input_dev, c.in_dtype, c.G(d.dst), c.batch, d.cin0, c.height, c.width, so.cp, d.cout, c.grad_of(d.weight), c.scratch(), c.s,
                            bias_in_wgrad ? c.grad_of(d.bias) : nullptr);
}

// ---- pool, bilinear x2, global max pool, GELU: no parameters

int bwd_pool(BackwardCtx& c, const PackedOp& op) {  // (scratch: the bias partials, which fit what the producer conv's own step reserves)
  const ph_op_desc& d = op.d;
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "pool output slot %d received no gradient", d.dst);
  // this pool completes the gradient of a conv + ReLU output: pool_bwd applies the mask itself (it reads the activation anyway) ...
  const ph_op_desc* pr = c.relu_producer_closed_by(d.src0, PH_OP_CONV);
  const bool fold = pr != nullptr;
  // ... and, the gradient being complete and masked as it is stored, it is summed per channel on the way: the producer conv's bias gradient,
  // which its own step would otherwise read the whole tensor again for
  const bool sum_bias = fold && pr->bias >= 0 && pool_bwd_can_sum_bias(si.cp);
  int rc = launch_pool_bwd(c.G(d.dst), c.A(d.src0), c.batch, si.h, si.w, si.cp, c.init[d.src0], fold ? 1 : 0, c.G(d.src0), sum_bias ? c.grad_of(pr->bias) : nullptr,
                           sum_bias ? pr->cout : 0, c.scratch(), c.s);
  c.note((fold ? PH_BR_FOLDED_MASK : 0) | (sum_bias ? PH_BR_SUMMED_BIAS : 0));
  c.init[d.src0] = 1;
  c.masked[d.src0] = fold ? 1 : 0;
  c.bias_done[d.src0] = sum_bias ? 1 : 0;
  return rc;
}

int bwd_upsample(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "upsample output slot %d received no gradient", d.dst);
  int rc = launch_upsample_bwd(c.G(d.dst), c.batch, si.h, si.w, si.cp, c.init[d.src0], c.G(d.src0), c.s);
  c.init[d.src0] = 1;
  return rc;
}

int bwd_global_maxpool(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "global pool output slot %d received no gradient", d.dst);
  int rc = launch_global_maxpool_bwd(c.A(d.src0), c.G(d.dst), c.batch, si.h * si.w, si.cp, c.init[d.src0], c.G(d.src0), c.s);
  c.init[d.src0] = 1;
  return rc;
}

int bwd_gelu(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (c.fused_away[c.oi]) {  // its consumer's data-gradient GEMM already wrote G(src0) through the GELU derivative
    c.note(PH_BR_NO_LAUNCH);
    return PH_OK;
  }
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "GELU output slot %d received no gradient", d.dst);
  int rc = launch_gelu_bwd(c.G(d.dst), c.A(d.src0), c.G(d.src0), c.init[d.src0], c.npix(so) * so.cp, c.s);
  c.init[d.src0] = 1;
  return rc;
}

// ---- layer scale + residual: y = s * u + x

int64_t bwd_scale_add_scratch_floats(const Plan& act, int, const ph_op_desc& d) { return chan_reduce_scratch_floats(act.slots[d.dst].cp); }

int bwd_scale_add(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "scale-add output slot %d received no gradient", d.dst);
  int rc = launch_chan_reduce(c.G(d.dst), c.A(d.src0), nullptr, c.npix(so), so.cp, d.cout, c.grad_of(d.weight), c.scratch(), c.s);
  if (rc != PH_OK) return rc;
  PH_REQUIRE(!c.init[d.src0], "scale-add input slot %d already has a gradient", d.src0);
  rc = launch_scale_add_bwd(c.G(d.dst), op.w_dev, c.G(d.src0), c.G(d.src1), c.init[d.src1], so.cp, c.npix(so) * so.cp, c.s);
  c.init[d.src0] = 1;
  c.init[d.src1] = 1;
  return rc;
}

// ---- Linear and 2x2/stride-2 conv: row GEMMs

int64_t bwd_linear_scratch_floats(const Plan& act, int B, const ph_op_desc& d) { return row_wgrad_slab_floats((int)((int64_t)B * act.slots[d.dst].h * act.slots[d.dst].w), d.cout, d.cin0); }

// Linear fed by a GELU whose output nobody else reads (CNBlock: Linear -> GELU -> Linear): the data-gradient GEMM multiplies by GELU'(pre-activation) in its epilogue
// and writes the GELU input's gradient directly, so the GELU output's gradient never exists in HBM.  Returns that GELU's op index, or -1
int fusable_gelu(const BackwardCtx& c, const ph_op_desc& d) {
  if (d.kind != PH_OP_LINEAR || !c.m->fuse_gelu_bwd || has_other_reader(c.m, d.src0, (size_t)c.oi)) return -1;
  const int pr = c.producer[d.src0];
  if (pr < 0 || pr >= c.oi || c.m->ops[pr].d.kind != PH_OP_GELU || c.init[c.m->ops[pr].d.src0]) return -1;
  return pr;
}

// The data-gradient GEMM of tap `tap`: G(src0) = gy x W^T, or -- gelu_op >= 0 -- the gradient of that GELU's input through the GELU derivative
int linear_dgrad(BackwardCtx& c, const PackedOp& op, const float* gy, int tap, int gelu_op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  const SlotShape& si = c.slot(d.src0);
  GemmArgs g{};
  g.src0 = gy;
  g.c0p = so.cp;
  g.wpack = op.wd_gemm_dev[tap];
  g.bias = op.zero_bias_dev;
  g.dst = c.G(d.src0);
  g.zeros = c.m->zeros_dev;
  g.coutp = si.cp;
  g.bn = op.bn_dg;
  g.M = c.batch * so.h * so.w;
  g.mode = 0;
  g.out_patch = d.kind == PH_OP_PATCH_CONV ? 1 : 0;
  g.out_tap = tap;
  g.out_H = si.h;
  g.out_W = si.w;
  if (gelu_op >= 0) {
    g.dst = c.G(c.m->ops[gelu_op].d.src0);
    g.act = 3;
    g.aux = c.A(c.m->ops[gelu_op].d.src0);
  }
  return launch_gemm(g, c.s);
}

int bwd_linear(BackwardCtx& c, const PackedOp& op) {  // PH_OP_LINEAR and PH_OP_PATCH_CONV
  ph_model* m = c.m;
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "GEMM output slot %d received no gradient", d.dst);
  PH_REQUIRE(!c.init[d.src0], "GEMM input slot %d already has a gradient (accumulation is not supported here)", d.src0);
  const bool patch = d.kind == PH_OP_PATCH_CONV;
  PH_REQUIRE(!patch || (si.h % 2 == 0 && si.w % 2 == 0), "2x2/stride-2 conv backward needs even input sizes");
  const int M = c.batch * so.h * so.w;
  const int taps = patch ? 4 : 1;
  const int gelu_op = fusable_gelu(c, d);
  // a Linear layer's bias gradient (column sums of dY) comes out of its weight-gradient GEMM, which stages every dY row anyway
  const bool bias_in_wgrad = !patch && !(d.flags & PH_FLAG_RELU) && d.bias >= 0;
  // a residual Linear under branch scales: its weight, bias and data gradients see s[branch][b] * G(dst) (one scaling pass), its residual source the plain G(dst)
  const float* gy = c.G(d.dst);
  int rc = PH_OK;
  if (c.branch_of[c.oi] >= 0 && m->branch_scales) {
    PH_REQUIRE(c.scaled_gy(), "backward plan has no region for the scaled gradient");
    rc = launch_scale_samples(c.G(d.dst), m->branch_scales + (size_t)c.branch_of[c.oi] * c.batch, c.scaled_gy(), (size_t)so.h * so.w * so.cp, c.batch, c.s);
    if (rc != PH_OK) return rc;
    gy = c.scaled_gy();
  }
  if (d.flags & PH_FLAG_RELU) {
    c.note_mask(PH_BR_MASK_OWN);
    c.note_bias(PH_BR_BIAS_WITH_MASK);
    rc = launch_relu_mask_bias_grad(c.G(d.dst), c.A(d.dst), (size_t)M, so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  } else if (!bias_in_wgrad && d.bias >= 0) {  // (Linear(bias=False): Swin's patch-merging reduction has none)
    c.note_bias(PH_BR_BIAS_OWN);
    rc = launch_bias_grad(c.G(d.dst), (size_t)M, so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  } else if (bias_in_wgrad) {
    c.note_bias(PH_BR_BIAS_ROW_WGRAD);
  }
  c.note_wgrad(0, PH_BR_WG_ROW_GEMM);
  c.note_dgrad(0, PH_BR_DG_GEMM0, false);  // (the source has no gradient yet: required above)
  if (gelu_op >= 0) c.note(PH_BR_GELU_FUSED);
  const WgradDst to{c.grad_of(d.weight), d.cout, d.cin0, d.cin0, 0, taps};
  for (int tap = 0; tap < taps && rc == PH_OK; ++tap) {
    rc = launch_wgrad_tap(c, gy, so.cp, c.A(d.src0), si.cp, M, TapGather{patch ? 1 : 0, 3, si.h, si.w}, to, tap, bias_in_wgrad ? c.grad_of(d.bias) : nullptr, bias_in_wgrad ? d.cout : 0);
    if (rc != PH_OK) break;
    if (tap == 0) {  // (a 2x2-stride-2 conv interleaves its four taps: all but the first weight-gradient GEMM count as data gradient)
      rc = c.mark_first_part();
      if (rc != PH_OK) return rc;
    }
    rc = linear_dgrad(c, op, gy, tap, gelu_op);
  }
  c.init[d.src0] = 1;
  if (gelu_op >= 0) {
    c.init[m->ops[gelu_op].d.src0] = 1;
    c.fused_away[gelu_op] = 1;
  }
  m->last_bwd_variant[c.oi] = PH_KV_ROWGEMM;
  if (rc == PH_OK && is_residual_linear(d)) {  // dst = acc + bias + src1: the residual source takes G(dst) as it is
    rc = launch_grad_fanout(c.G(d.dst), c.G(d.src1), c.init[d.src1], (size_t)M * so.cp, c.s);
    c.init[d.src1] = 1;
  }
  if (rc == PH_OK && c.pad_bias >= 0 && d.kind == PH_OP_LINEAR && d.bias == c.pad_bias) {  // the qkv Linear has written qkv.bias's gradient: add the padded tokens' share
    rc = launch_vec_add(c.grad_of(d.bias), c.pad_vec(), c.pad_n, c.s);
    c.pad_bias = -1;
  }
  return rc;
}

// ---- Swin: shifted-window attention core, patch merging

int64_t bwd_window_attn_scratch_floats(const Plan& act, int B, const ph_op_desc& d) { return window_attn_bwd_scratch_floats(B, act.slots[d.src0].h, act.slots[d.src0].w, d.cout, d.cin1, d.ksize); }

int bwd_window_attn(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "window attention output slot %d received no gradient", d.dst);
  PH_REQUIRE(!c.init[d.src0] && c.pad_bias < 0 && c.pad_vec(), "window attention: the qkv slot %d must have the attention core as its only reader", d.src0);
  WindowAttnBwdArgs w{};
  w.qkv = c.A(d.src0);
  w.table = op.w_dev;
  w.qkv_bias = op.b_dev;
  w.gout = c.G(d.dst);
  w.gqkv = c.G(d.src0);
  w.gtable = c.grad_of(d.weight);
  w.gpad = c.pad_vec();
  w.scratch = c.scratch();
  w.B = c.batch;
  w.H = si.h;
  w.W = si.w;
  w.C = d.cout;
  w.heads = d.cin1;
  w.w = d.ksize;
  w.sh = window_axis_shift(si.h, d.ksize, d.cmid);  // per axis, as the forward
  w.sw = window_axis_shift(si.w, d.ksize, d.cmid);
  int rc = launch_window_attn_bwd(w, c.s);
  c.m->last_bwd_variant[c.oi] = PH_KV_WINDOW_ATTN_BWD;
  c.init[d.src0] = 1;
  c.pad_bias = d.bias;
  c.pad_n = d.cin0;
  return rc;
}

int64_t bwd_patch_merge_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {  // statistics, reduction partials, gather, its gradient
  const SlotShape& so = act.slots[d.dst];
  const int64_t npix = (int64_t)B * so.h * so.w;
  return 2 * npix + chan_reduce_scratch_floats(so.cp) + 2 * npix * so.cp;
}

int bwd_patch_merge(BackwardCtx& c, const PackedOp& op) {  // dst = LayerNorm(gather(src0)) over 4C channels; the gathered tensor is rebuilt in scratch
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  const SlotShape& si = c.slot(d.src0);
  PH_REQUIRE(c.init[d.dst], "patch merge output slot %d received no gradient", d.dst);
  const size_t npix = c.npix(so);
  float* xg = c.scratch();
  float* gxg = xg + npix * so.cp;
  float* stats = gxg + npix * so.cp;
  float* red = stats + 2 * npix;
  int rc = launch_patch_merge_gather(c.A(d.src0), xg, c.batch, si.h, si.w, d.cin0, c.s);
  if (rc != PH_OK) return rc;
  rc = launch_layernorm_bwd(xg, c.G(d.dst), op.w_dev, gxg, stats, 0, so.c, so.cp, npix, c.s, ln_eps(d));
  if (rc != PH_OK) return rc;
  rc = launch_chan_reduce(c.G(d.dst), xg, stats, npix, so.cp, so.c, c.grad_of(d.weight), red, c.s);
  if (rc != PH_OK) return rc;
  rc = launch_chan_reduce(c.G(d.dst), nullptr, nullptr, npix, so.cp, so.c, c.grad_of(d.bias), red, c.s);
  if (rc != PH_OK) return rc;
  rc = launch_patch_merge_scatter(gxg, c.G(d.src0), c.init[d.src0], c.batch, si.h, si.w, d.cin0, c.s);
  c.init[d.src0] = 1;
  return rc;
}

// ---- ConvNeXt: LayerNorm, depthwise 7 x 7, patch stem; ConvNeXtV2: GRN

int64_t bwd_layernorm_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {  // statistics, then the reduction partials
  const SlotShape& so = act.slots[d.dst];
  return 2 * ((int64_t)B * so.h * so.w) + chan_reduce_scratch_floats(so.cp);
}

int bwd_layernorm(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "LayerNorm output slot %d received no gradient", d.dst);
  const size_t npix = c.npix(so);
  float* stats = c.scratch();
  float* red = c.scratch() + 2 * npix;
  int rc = launch_layernorm_bwd(c.A(d.src0), c.G(d.dst), op.w_dev, c.G(d.src0), stats, c.init[d.src0], so.c, so.cp, npix, c.s, ln_eps(d));
  if (rc != PH_OK) return rc;
  rc = launch_chan_reduce(c.G(d.dst), c.A(d.src0), stats, npix, so.cp, so.c, c.grad_of(d.weight), red, c.s);
  if (rc != PH_OK) return rc;
  rc = launch_chan_reduce(c.G(d.dst), nullptr, nullptr, npix, so.cp, so.c, c.grad_of(d.bias), red, c.s);
  c.init[d.src0] = 1;
  return rc;
}

int64_t bwd_dwconv_scratch_floats(const Plan& act, int B, const ph_op_desc& d) { return dwconv7_wgrad_scratch_floats(B, act.slots[d.dst].h, act.slots[d.dst].cp); }

int bwd_dwconv(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "depthwise conv output slot %d received no gradient", d.dst);
  int rc = launch_bias_grad(c.G(d.dst), c.npix(so), so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  if (rc != PH_OK) return rc;
  rc = launch_dwconv7_wgrad(c.A(d.src0), c.G(d.dst), c.batch, so.h, so.w, so.cp, d.cout, c.grad_of(d.weight), c.scratch(), c.s);
  if (rc != PH_OK) return rc;
  DwConvArgs a{};
  a.src = c.G(d.dst);
  a.w = op.dw_flip_dev;
  a.bias = nullptr;
  a.dst = c.G(d.src0);
  a.cp = so.cp;
  a.B = c.batch;
  a.H = so.h;
  a.W = so.w;
  a.accumulate = c.init[d.src0];
  rc = launch_dwconv7(a, c.s);
  c.init[d.src0] = 1;
  return rc;
}

int64_t bwd_patch_stem_scratch_floats(const Plan& act, int B, const ph_op_desc& d) { return patch_stem_wgrad_scratch_floats(d.cin0, d.cout, d.ksize, (int64_t)B * act.slots[d.dst].h * act.slots[d.dst].w); }

int bwd_patch_stem(BackwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "stem output received no gradient");
  PH_REQUIRE(d.cin0 == c.in_channels, "input has %d channels, network expects %d", c.in_channels, d.cin0);
  c.note_bias(PH_BR_BIAS_OWN);
  c.note_wgrad(0, PH_BR_WG_PATCH_STEM);
  int rc = launch_bias_grad(c.G(d.dst), c.npix(so), so.cp, d.cout, c.grad_of(d.bias), c.scratch(), c.s);
  if (rc != PH_OK) return rc;
  if (d.flags & PH_FLAG_PAD0_NORM)  // ConvNeXtV2 embeddings: padding 0, patches of (x / 255 - mean) / std; the bias gradient above is the same
    return launch_patch_stem_wgrad_norm(c.input_dev, c.in_dtype, c.G(d.dst), c.batch, d.cin0, c.height, c.width, so.h, so.w, d.ksize, d.cmid, so.cp, d.cout, c.m->in_mean, c.m->in_std,
                                        c.grad_of(d.weight), c.scratch(), c.s);
  return launch_patch_stem_wgrad(c.input_dev, c.in_dtype, c.G(d.dst), c.batch, d.cin0, c.height, c.width, so.h, so.w, d.ksize, d.cmid, 1, so.cp, d.cout, c.grad_of(d.weight), c.scratch(),
                                 c.s);
}

// (slice sums of x^2, g x, g; per-sample coefficients and parameter shares)
int64_t bwd_grn_scratch_floats(const Plan& act, int B, const ph_op_desc& d) { return grn_bwd_scratch_floats(B, act.slots[d.dst].h * act.slots[d.dst].w, act.slots[d.dst].cp); }

int bwd_grn(BackwardCtx& c, const PackedOp& op) {  // y = w (x N) + beta + x: convnextv2_train_kernels.hip
  const ph_op_desc& d = op.d;
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.init[d.dst], "GRN output slot %d received no gradient", d.dst);
  PH_REQUIRE(c.slot(d.src0).cp == so.cp && so.c == d.cout, "GRN channel mismatch");
  GrnBwdArgs a{};
  a.x = c.A(d.src0);
  a.gy = c.G(d.dst);
  a.weight = op.w_dev;
  a.gx = c.G(d.src0);
  a.gw = c.grad_of(d.weight);
  a.gb = c.grad_of(d.bias);
  a.scratch = c.scratch();
  a.B = c.batch;
  a.HW = so.h * so.w;
  a.c = d.cout;
  a.cp = so.cp;
  a.accumulate = c.init[d.src0];
  int rc = launch_grn_bwd(a, c.s);
  c.m->last_bwd_variant[c.oi] = PH_KV_GRN_BWD;
  c.init[d.src0] = 1;
  return rc;
}

// ---- dispatch, and the plan

int bwd_op(BackwardCtx& c, const PackedOp& op) {
  switch (op.d.kind) {
    case PH_OP_HEAD: return bwd_head(c, op);
    case PH_OP_CONV: return bwd_conv(c, op);
    case PH_OP_CONVT: return bwd_convt(c, op);
    case PH_OP_INPUT_CONV: return bwd_input_conv(c, op);
    case PH_OP_POOL: return bwd_pool(c, op);
    case PH_OP_UPSAMPLE: return bwd_upsample(c, op);
    case PH_OP_SCALE_ADD: return bwd_scale_add(c, op);
    case PH_OP_GELU: return bwd_gelu(c, op);
    case PH_OP_LINEAR:
    case PH_OP_PATCH_CONV: return bwd_linear(c, op);
    case PH_OP_WINDOW_ATTN: return bwd_window_attn(c, op);
    case PH_OP_PATCH_MERGE: return bwd_patch_merge(c, op);
    case PH_OP_LAYERNORM: return bwd_layernorm(c, op);
    case PH_OP_DWCONV: return bwd_dwconv(c, op);
    case PH_OP_GLOBAL_MAXPOOL: return bwd_global_maxpool(c, op);
    case PH_OP_PATCH_STEM: return bwd_patch_stem(c, op);
    case PH_OP_GRN: return bwd_grn(c, op);
    default:
      set_error("backward: unsupported op kind %d", op.d.kind);
      return PH_E_INVALID;
  }
}

// Scratch floats the step of op `d` (and, a head, its loss) needs.  Every kind from the patch stem up has at least a bias reduction over its output, whether its step
// reduces one or not (GELU, global max pool): the workspace size is part of the ABI's behaviour
int64_t bwd_op_scratch_floats(const Plan& act, int B, const ph_op_desc& d) {
  const int64_t floor = d.kind >= PH_OP_PATCH_STEM ? bias_scratch_floats(act.slots[d.dst].cp) : 0;
  switch (d.kind) {
    case PH_OP_HEAD: return bwd_head_scratch_floats(act, B, d);
    case PH_OP_CONV: return bwd_conv_scratch_floats(act, B, d);
    case PH_OP_CONVT: return bwd_convt_scratch_floats(act, B, d);
    case PH_OP_INPUT_CONV: return bwd_input_conv_scratch_floats(act, B, d);
    case PH_OP_SCALE_ADD: return std::max(floor, bwd_scale_add_scratch_floats(act, B, d));
    case PH_OP_LINEAR:
    case PH_OP_PATCH_CONV: return std::max(floor, bwd_linear_scratch_floats(act, B, d));
    case PH_OP_WINDOW_ATTN: return std::max(floor, bwd_window_attn_scratch_floats(act, B, d));
    case PH_OP_PATCH_MERGE: return std::max(floor, bwd_patch_merge_scratch_floats(act, B, d));
    case PH_OP_LAYERNORM: return std::max(floor, bwd_layernorm_scratch_floats(act, B, d));
    case PH_OP_DWCONV: return std::max(floor, bwd_dwconv_scratch_floats(act, B, d));
    case PH_OP_PATCH_STEM: return std::max(floor, bwd_patch_stem_scratch_floats(act, B, d));
    case PH_OP_GRN: return std::max(floor, bwd_grn_scratch_floats(act, B, d));
    default: return floor;  // pool, bilinear x2 (0); GELU, global max pool (the floor)
  }
}

// Whether the program can be trained at all: the unfused program, with the data-gradient weight forms ph_model_create derives for it
int check_trainable_program(const ph_model* m) {
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
    if (d.kind == PH_OP_CONVT && (!op.wt_dgrad_dev || op.wt_scale_dev || (d.flags & PH_FLAG_SILU))) {
      set_error("backward of a transposed conv supports bias + ReLU (the reference's decoder); folded BatchNorm / SiLU are inference-only");
      return PH_E_INVALID;
    }
    if (d.kind == PH_OP_LINEAR && (d.flags & (PH_FLAG_GELU | PH_FLAG_SCALE_RESIDUAL))) {
      set_error("backward needs the unfused ConvNeXt program (GELU / layer-scale as ops of their own)");
      return PH_E_INVALID;
    }
  }
  return PH_OK;
}

// The gradient workspace: gradient slots (mirroring the activation slots one to one), one NCHW dY buffer per head, the pad vector (Swin), the scaled gradient (residual
// Linears), then the scratch every step shares -- the maximum over the steps' formulas
int build_bwd_plan(const ph_model* m, int B, int H, int W, BwdPlan& bp) {
  int rc = build_plan(m, B, H, W, bp.act);
  if (rc != PH_OK) return rc;
  rc = check_trainable_program(m);
  if (rc != PH_OK) return rc;
  int64_t off = bp.act.total;
  bp.head_dy_off.assign(m->n_outputs, -1);
  int64_t scratch = 0, pad_floats = 0, scaled_floats = 0;
  for (const PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    scratch = std::max(scratch, bwd_op_scratch_floats(bp.act, B, d));
    if (d.kind == PH_OP_HEAD) {
      const SlotShape& s0 = bp.act.slots[d.src0];
      bp.head_dy_off[d.out_index] = off;
      off += align_up((int64_t)B * d.cout * s0.h * s0.w * 4, 256);
    }
    if (d.kind == PH_OP_WINDOW_ATTN) pad_floats = std::max<int64_t>(pad_floats, d.cin0);
    if (is_residual_linear(d)) scaled_floats = std::max<int64_t>(scaled_floats, (int64_t)B * bp.act.slots[d.dst].h * bp.act.slots[d.dst].w * bp.act.slots[d.dst].cp);
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

// The handle checks of ph_model_backward that need no plan, in the order the ABI has always made them
int check_backward_handle(ph_model* m, int batch) {
  int n_res = 0;  // per-sample branch scales (ph_model_set_branch_scales): one row per residual Linear of the program
  for (const PackedOp& op : m->ops)
    if (is_residual_linear(op.d)) n_res += 1;
  PH_REQUIRE(!m->branch_scales || (m->branch_n == n_res && m->branch_batch == batch),
             "ph_model_backward: branch scales are set for %d branches x batch %d, the step has %d x %d", m->branch_n, m->branch_batch, n_res, batch);
  const size_t n_ops = m->ops.size();
  m->last_bwd_variant.assign(n_ops, PH_KV_NONE);
  m->last_bwd_route.assign(n_ops, 0);
  if (m->profiling && m->bwd_ev.size() != 2 * n_ops + 2) {
    for (auto& e : m->bwd_ev) (void)hipEventDestroy(e);
    m->bwd_ev.assign(2 * n_ops + 2, nullptr);
    for (auto& e : m->bwd_ev) PH_HIP_CHECK(hipEventCreate(&e));
  }
  m->bwd_ev_recorded = false;
  for (const auto& op : m->ops) {  // the MSE / cross-entropy gradients of bwd_losses are not these heads' losses: they train only with a loss chosen by ph_model_set_head_loss
    if (op.d.kind != PH_OP_HEAD) continue;
    PH_REQUIRE(op.d.out_index >= 0 && op.d.out_index < PH_MAX_OUTPUTS, "ph_model_backward: head output index %d out of range", op.d.out_index);
    PH_REQUIRE(!((op.d.flags & PH_FLAG_NO_TRAIN) && m->head_loss_kind[op.d.out_index] == 0),
               "ph_model_backward: head %d belongs to a segmentation model type, whose losses (BCE + Dice, masked smooth-L1) are not built: inference only", op.d.out_index);
  }
  for (const auto& op : m->ops)  // a ResNet program (HuggingFace ResNetBackbone behind the 'pretrained' backbone) has no backward step at all: BatchNorm with batch statistics is another op
    PH_REQUIRE(op.d.kind != PH_OP_RESNET_STEM && op.d.kind != PH_OP_CONV_S2 && op.d.kind != PH_OP_ADD_RELU,
               "ph_model_backward: op kind %d belongs to a 'pretrained' ResNet backbone, which is inference only", op.d.kind);
  for (const auto& op : m->ops)  // nor has a Swinv2 program (HuggingFace Swinv2Backbone): the cosine attention, the residual-after-norm LayerNorm and the norm-less patch merge are forward only
    PH_REQUIRE(op.d.kind != PH_OP_WINDOW_ATTN_V2 && !(op.d.kind == PH_OP_LAYERNORM && (op.d.flags & PH_FLAG_RESIDUAL)) && !(op.d.kind == PH_OP_PATCH_MERGE && (op.d.flags & PH_FLAG_NO_NORM)),
               "ph_model_backward: op kind %d belongs to a 'pretrained' Swinv2 backbone, which is inference only", op.d.kind);
  for (const auto& op : m->ops)  // the ConvNeXtV2 ops (GRN, the padding-0 stem with input statistics) carry PH_FLAG_NO_TRAIN: their backward steps run on request only
    PH_REQUIRE(m->pretrained_train || !(op.d.kind != PH_OP_HEAD && (op.d.flags & PH_FLAG_NO_TRAIN)),
               "ph_model_backward: op kind %d is inference only on this handle (a 'pretrained' ConvNeXtV2 backbone trains with the handle option pretrained_train = 1)", op.d.kind);
  PH_REQUIRE(m->last_plan.fmt == FMT_F32, "backward needs the activations of an exact-fp32 forward (handle option conv_precision = 0)");
  PH_REQUIRE(!m->last_plan.reuse, "backward needs every activation of the forward (handle option workspace_reuse = 0)");
  return PH_OK;
}

}  // namespace

extern "C" {

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
  int rc = check_backward_handle(m, batch);
  if (rc != PH_OK) return rc;
  BwdPlan bp;
  rc = build_bwd_plan(m, batch, height, width, bp);
  if (rc != PH_OK) return rc;
  if (bp.total > grad_workspace_bytes) {
    set_error("gradient workspace too small: need %lld bytes, got %lld", (long long)bp.total, (long long)grad_workspace_bytes);
    return PH_E_WORKSPACE;
  }
  const int n_ops = (int)m->ops.size();
  int n_cu = 0;
  rc = device_cu_count(&n_cu);
  if (rc != PH_OK) return rc;
  BackwardCtx c{m, bp, batch, height, width, in_channels, in_dtype, input_dev, static_cast<const char*>(act_workspace_dev), static_cast<char*>(grad_workspace_dev), head_out_dev,
                grads_flat_dev, s, m->profiling, std::max(0, std::min(m->bwd_frozen_ops, n_ops)), n_cu};
  index_program(c);
  if (c.prof) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[0], s));
  rc = bwd_losses(c, LossArgs{target_dev, loss_weights_host, sample_weights_dev, OhkmParams{ohkm_enabled, hard_to_easy_ratio, min_hard_keypoints, max_hard_keypoints, ohkm_loss_scale}, loss_dev});
  if (rc != PH_OK) return rc;
  // ---- reverse sweep
  for (c.oi = n_ops - 1; c.oi >= 0; --c.oi) {
    const PackedOp& op = m->ops[c.oi];
    const ph_op_desc& d = op.d;
    // an op whose output no op reads (a ConvNeXtV2 stage norm whose map the decoder does not take: output stride 8) has no gradient to pass on: like a frozen op
    const bool dead = d.kind != PH_OP_HEAD && d.dst >= 0 && c.first_consumer[d.dst] < 0 && (d.dst2 < 0 || c.first_consumer[d.dst2] < 0);
    const bool no_step = c.oi < c.frozen || dead;  // the gradients of its parameters stay as the caller left them
    c.ev_i = 1 + 2 * (size_t)(n_ops - 1 - c.oi);
    if (c.prof) {  // the mid event: a Linear / 2x2-stride-2 conv records it behind its first weight-gradient GEMM (mark_first_part); every other kind, and a Linear without a step, at once
      PH_HIP_CHECK(hipEventRecord(m->bwd_ev[c.ev_i], s));
      if (!is_row_gemm(d) || no_step) PH_HIP_CHECK(hipEventRecord(m->bwd_ev[c.ev_i + 1], s));
    }
    if (!no_step) {
      rc = bwd_op(c, op);
      if (rc != PH_OK) return rc;
    }
    if (c.oi == c.split_op) {  // (a split op in the frozen part: the tail was final when the last trainable op finished)
      rc = bwd_tail_final(c);
      if (rc != PH_OK) return rc;
    }
  }
  PH_REQUIRE(c.pad_bias < 0, "window attention: no qkv Linear took the padded tokens' share of its bias gradient");
  if (c.prof) {
    PH_HIP_CHECK(hipEventRecord(m->bwd_ev[2 * (size_t)n_ops + 1], s));
    m->bwd_ev_recorded = true;
  }
  return bwd_head_bucket(c);
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

}  // extern "C"
