// Training-side state of the network runtime handle (C ABI): the parameter arena (ph_model_num_params, ph_model_set_params), the gradient arena's bucket split with its
// event and communicator setters, the branch scales, the head losses, and the accessors of what the last ph_model_backward left (profile, kernels).  The backward's
// launch sequence itself is backward.hip.
#include <algorithm>

#include "model_internal.h"
#include "train_kernels.h"

using namespace ph;

static_assert(PH_MAX_OUTPUTS == sizeof(ph_model::head_loss_kind) / sizeof(int), "ph_model keeps one head loss per possible output");

// Smallest / largest arena offset an op's parameters start at (-1: the op has none).
static int64_t op_param_offset(const ph_model* m, const ph_op_desc& d, bool highest = false) {
  int64_t v = -1;
  for (int idx : {d.weight, d.bias, d.weight2, d.bias2})
    if (idx >= 0 && idx < (int)m->weight_offset.size()) v = v < 0 ? m->weight_offset[idx] : (highest ? std::max(v, m->weight_offset[idx]) : std::min(v, m->weight_offset[idx]));
  return v;
}

// The op (forward order) whose completion in the reverse sweep makes the arena tail [offset, n_params) final: the program's
// parameters lie in op order, so the candidates are the ops at which the arena splits cleanly; the one closest to the middle wins.
int ph::bucket_split_op(const ph_model* m, int64_t* offset_out) {
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
  return refresh_derived(m, params_flat_dev, static_cast<hipStream_t>(stream));  // (weights.hip: the derived forms follow the packed buffers they are computed from)
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

int ph_model_last_backward_routes(const ph_model* m, int32_t* routes, int32_t n_ops) {
  PH_REQUIRE(m && routes && n_ops >= 0, "ph_model_last_backward_routes: bad arguments");
  for (int i = 0; i < n_ops; ++i) routes[i] = i < (int)m->last_bwd_route.size() ? m->last_bwd_route[i] : 0;
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
