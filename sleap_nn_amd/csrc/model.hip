// Host runtime of the network path: the error string, ph_model_destroy, the options table and the small accessors of the C ABI (ph_model_*); the handle's
// weight forms and ph_model_create are weights.hip, the workspace plan is plan.hip, the forward launch sequence forward.hip.  Together they replace TorchBackend.__call__ ->
// LightningModule.forward -> Model.forward -> UNet.forward of the reference
// (sleap_nn/inference/layers/backends/torch_backend.py:113-153,
//  training/lightning_modules.py:1840-1848, architectures/model.py:237-261,
//  architectures/unet.py:260-299).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "model_internal.h"
#include "train_kernels.h"

namespace ph {

static thread_local std::string g_err;

void set_error(const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
}

}  // namespace ph

namespace ph {

int device_cu_count(int* out) {
  static std::atomic<int> cache[64];  // zero-initialised; a count is a device property, racing writers store the same value
  int dev = 0;
  PH_HIP_CHECK(hipGetDevice(&dev));
  int n = (dev >= 0 && dev < 64) ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (!n) {
    PH_HIP_CHECK(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
    if (dev >= 0 && dev < 64) cache[dev].store(n, std::memory_order_relaxed);
  }
  *out = n;
  return PH_OK;
}

void apply_conv_options(const ph_model* m, ConvArgs& a) {
  a.use_wino = m->conv_wino;
  a.use_wino2d = m->conv_wino2d;
  a.wino4_min_cin = m->conv_wino4_min_cin;
  a.use_w16 = m->conv_w16;
  a.persist = m->conv_persist;
  a.use_c16 = m->conv_c16;
  a.dma_stagger = m->dma_stagger;
  a.splitk = m->conv_splitk;  // (ph_model_forward clears it for a training plan unless a slice count is forced)
  a.split_counters = m->split_counters_dev;
  a.split_counters_n = m->split_counters_dev ? 4096 : 0;  // (units; the buffer holds three words per unit)
  a.splitk_finish = m->conv_splitk_finish;
  a.use_sm = 0;  // (apply_conv_plan_options: the kind of plan decides)
  a.use_dma = m->use_dma;
  a.dma32 = m->dma32;
}

// The options whose meaning depends on the plan a launch belongs to.  The F(4x4,3x3) kernel, the small-map kernel and the automatic K split are routings of inference
// plans (they were measured there; a training program's forward keeps the kernels its gradient tests were pinned with) unless the option asks for every plan.
void apply_conv_plan_options(const ph_model* m, ConvPlanKind kind, ConvArgs& a) {
  const bool inference = kind == CONV_PLAN_INFERENCE;
  a.use_wino4 = m->conv_wino4 == 3 ? 2 : ((m->conv_wino4 == 2 || (m->conv_wino4 == 1 && inference)) ? 1 : 0);
  if (kind == CONV_PLAN_DGRAD) {  // (no small-map kernel: it has no accumulate / mask form; splitk stays as set: a data-gradient conv gets no split scratch)
    if (!m->dgrad_wino) a.use_wino = 0;
    return;
  }
  a.use_sm = m->conv_smallmap >= 2 ? 2 : ((m->conv_smallmap == 1 && m->conv_splitk == 1 && inference && m->use_dma) ? 1 : 0);
  if (a.splitk == 1 && !inference) a.splitk = 0;
}

int drain_events(ph_model* m) {
  if (!m->events_pending) return PH_OK;
  const size_t n = m->ops.size();
  PH_HIP_CHECK(hipEventSynchronize(m->ev[n]));
  for (size_t i = 0; i < n; ++i) {
    float ms = 0.f;
    PH_HIP_CHECK(hipEventElapsedTime(&ms, m->ev[i], m->ev[i + 1]));
    m->op_ms[i] += ms;
  }
  m->profiled_forwards += 1;
  m->events_pending = false;
  return PH_OK;
}

}  // namespace ph

using namespace ph;

extern "C" {

const char* ph_last_error(void) { return ph::g_err.c_str(); }
int ph_version(void) { return PH_VERSION; }

void ph_model_destroy(ph_model* m) {
  if (!m) return;
  for (void* p : m->allocs) (void)hipFree(p);
  for (hipEvent_t e : m->ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->bwd_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : m->comm_events_owned) (void)hipEventDestroy(e);
  delete m;
}

int64_t ph_model_workspace_bytes(const ph_model* m, int32_t batch, int32_t height, int32_t width) {
  if (!m || batch <= 0 || height <= 0 || width <= 0) {
    set_error("ph_model_workspace_bytes: bad arguments");
    return PH_E_INVALID;
  }
  Plan plan;
  int rc = build_plan(m, batch, height, width, plan, forward_format(m));
  if (rc != PH_OK) return rc;
  return plan.total;
}

int ph_model_output_shape(const ph_model* m, int32_t out_index, int32_t height, int32_t width, int32_t* c, int32_t* h, int32_t* w) {
  PH_REQUIRE(m && c && h && w, "ph_model_output_shape: null argument");
  Plan plan;
  int rc = build_plan(m, 1, height, width, plan);
  if (rc != PH_OK) return rc;
  for (const PackedOp& op : m->ops)
    if (op.d.kind == PH_OP_HEAD && op.d.out_index == out_index) {
      *c = op.d.cout;
      *h = plan.slots[op.d.src0].h;
      *w = plan.slots[op.d.src0].w;
      return PH_OK;
    }
  set_error("no head writes output %d", out_index);
  return PH_E_INVALID;
}

int32_t ph_op_desc_size(void) { return (int32_t)sizeof(ph_op_desc); }

int ph_debug_split_plan(int32_t B, int32_t H, int32_t W, int32_t cin_padded, int32_t cout_padded, int32_t splitk, int32_t n_cu, int64_t* out4) {
  PH_REQUIRE(out4 && B > 0 && H > 0 && W > 0 && cin_padded > 0 && cout_padded > 0 && n_cu > 0 && (cin_padded % 16) == 0 && (cout_padded % 16) == 0, "ph_debug_split_plan: bad arguments");
  out4[0] = wino2d_ksplit_shape(B, H, W, cin_padded, cout_padded, splitk, n_cu);
  out4[1] = ((H & 3) || (W & 3)) ? 1 : wino4_ksplit_shape(B, H, W, cin_padded, cout_padded, splitk, n_cu);
  out4[2] = wino2d_split_scratch_bytes(B, H, W, cin_padded, cout_padded, splitk, n_cu) / 1024;
  out4[3] = wino4_split_scratch_bytes(B, H, W, cin_padded, cout_padded, splitk, n_cu) / 1024;
  return PH_OK;
}

int32_t ph_conv_route_case_size(void) { return (int32_t)sizeof(ph_conv_route_case); }

int ph_debug_conv3x3_route(const ph_conv_route_case* c, int32_t n_cu, ph_conv_route_out* out) {
  PH_REQUIRE(c && out && n_cu > 0 && c->B > 0 && c->H > 0 && c->W > 0 && c->c0p > 0 && c->c1p >= 0 && c->coutp > 0 && (c->bn == 32 || c->bn == 64), "ph_debug_conv3x3_route: bad arguments");
  float* const p = reinterpret_cast<float*>((uintptr_t)4096 * (uintptr_t)(1 + (c->ptr_salt & 0xFFFF)));  // never read: the route looks at which pointers are null
  auto have = [&](int32_t word, int32_t bit) { return (word & bit) ? p : nullptr; };
  ConvArgs a{};
  a.src0 = a.wpack = a.bias = a.zeros = p;
  a.dst = p;
  a.c0p = c->c0p, a.c1p = c->c1p, a.coutp = c->coutp, a.bn = c->bn, a.B = c->B, a.H = c->H, a.W = c->W;
  a.relu = 1;
  a.wpack_dma = have(c->forms, PH_CRF_DMA), a.wpack_wino = have(c->forms, PH_CRF_WINO), a.wpack_wino2 = have(c->forms, PH_CRF_WINO2), a.wpack_w16 = have(c->forms, PH_CRF_W16);
  a.w16 = have(c->forms, PH_CRF_C16), a.wpack_wino4 = have(c->forms, PH_CRF_WINO4), a.wpack_sm = have(c->forms, PH_CRF_SM);
  a.src1 = have(c->flags, PH_CRA_SRC1);
  a.src1_lowres = (c->flags & PH_CRA_SRC1_LOWRES) ? 1 : 0;
  a.dst_pool = have(c->flags, PH_CRA_POOL);
  a.skip_dst = (c->flags & PH_CRA_SKIP_DST) ? 1 : 0;
  a.accumulate = (c->flags & PH_CRA_ACCUMULATE) ? 1 : 0;
  a.relu_mask_src = have(c->flags, PH_CRA_RELU_MASK);
  a.head_w = a.head_b = have(c->flags, PH_CRA_HEAD);
  a.head_dst = have(c->flags, PH_CRA_HEAD);
  a.head_cout = c->head_cout, a.head_wcp = c->head_wcp;
  if (c->split_scratch_bytes > 0) a.split_scratch = p, a.split_scratch_bytes = c->split_scratch_bytes;
  a.use_dma = c->use_dma, a.dma32 = c->dma32, a.use_wino = c->use_wino, a.persist = c->persist, a.use_c16 = c->use_c16, a.use_w16 = c->use_w16, a.use_wino2d = c->use_wino2d;
  a.use_wino4 = c->use_wino4, a.wino4_min_cin = c->wino4_min_cin, a.use_sm = c->use_sm, a.splitk = c->splitk;
  const ConvRoute r = conv3x3_route(a, n_cu);
  out->kernel = (int32_t)r.kernel;
  out->kv = r.kv;
  out->ksplit = r.ksplit;
  out->props = (r.takes_mask ? PH_CRP_MASK : 0) | (r.pools ? PH_CRP_POOLS : 0) | (r.head_w2d ? PH_CRP_HEAD_W2D : 0) | (r.head_w16 ? PH_CRP_HEAD_W16 : 0) |
               (r.folds_lowres ? PH_CRP_LOWRES : 0) | (r.head_sm ? PH_CRP_HEAD_SM : 0);
  return PH_OK;
}

int ph_model_debug_allocs(const ph_model* m, void** ptrs, int64_t* bytes, int32_t max_rows, int32_t* n_rows) {
  PH_REQUIRE(m && n_rows && max_rows >= 0 && (max_rows == 0 || (ptrs && bytes)), "ph_model_debug_allocs: bad arguments");
  *n_rows = (int32_t)m->allocs.size();
  for (int32_t i = 0; i < max_rows && i < *n_rows; ++i) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    PH_HIP_CHECK(hipMemGetAddressRange(&base, &size, m->allocs[i]));
    ptrs[i] = m->allocs[i];
    bytes[i] = (int64_t)size;
  }
  return PH_OK;
}

namespace {
struct OptionRef {
  const char* key;
  int* i;
  double* d;
};
// every tunable of a handle; defaults are the measured-best variants (DESIGN.md, appendix "handle options")
std::vector<OptionRef> option_table(ph_model* m) {
  return {
      {"conv_wino", &m->conv_wino, nullptr},            // 1 Winograd F(2,3) 3x3 kernels, 2 only N-tile-64 layers, 0 direct 9-tap kernels
      {"conv_w16", &m->conv_w16, nullptr},              // 1: Cout-32 / Cin-16-or-32 3x3 convs on the wave-private F(2x2,3x3) kernel; 0: F(2,3) along x
      {"conv_wino2d", &m->conv_wino2d, nullptr},        // 1: N-tile-64 3x3 convs on the F(2x2,3x3) kernel; 0: F(2,3) along x only
      {"conv_wino4", &m->conv_wino4, nullptr},          // K-heavy 3x3 convs on the F(4x4,3x3) kernel: 1 inference plans, 2 every plan (both: where estimated faster), 3 every plan wherever it fits, 0 never
      {"conv_wino4_min_cin", &m->conv_wino4_min_cin, nullptr},  // padded input channels from which a layer takes it
      {"conv_n32_wino2d", &m->conv_n32_wino2d, nullptr},  // Cout-32 / K >= 64 layers on the F(2x2,3x3) kernel with a half-empty N tile (0: the N-tile-32 F(2,3) kernel)
      {"conv_splitk_finish", &m->conv_splitk_finish, nullptr},  // 0: the split-K second stage as a launch of its own (A/B, tests)
      {"grn_fuse", &m->grn_fuse, nullptr},                // ConvNeXtV2 blocks on the fused GRN plan: 1 sums of squares from the first Linear's epilogue + per-sample scaled weights for the second; 0 (default, measured faster) two GRN launches
      {"pretrained_train", &m->pretrained_train, nullptr},  // 1: ph_model_backward accepts a ConvNeXtV2 program (GRN backward, weight gradient of the padding-0 stem); 0 (default) refuses its PH_FLAG_NO_TRAIN ops
      {"bwd_frozen_ops", &m->bwd_frozen_ops, nullptr},      // the first n ops get no backward step (frozen encoder); 0 (default) none
      {"mlp_fuse", &m->mlp_fuse, nullptr},              // inference plans: CNBlock's two Linears (+ GELU, layer scale, residual) in one launch (cnblock_mlp_kernel)
      {"block_fuse", &m->block_fuse, nullptr},          // plain fp16, inference plans: the two convs of a 32-channel encoder block in one launch (block2_c32_f16_kernel)
      {"stem_f16mfma", &m->stem_f16mfma, nullptr},      // plain fp16: the fused first block with BOTH convs on the fp16 matrix pipe (stem_f16_kernel) instead of stem_fused_kernel<CIN, 3>
      {"upsample_f16math", &m->upsample_f16math, nullptr},  // a bilinear x2 folded into conv3x3_f16_rows_kernel blends in packed fp16 arithmetic (1) or in fp32 as upsample2x_fmt_kernel does (0)
      {"conv_f16_rows", &m->conv_f16_rows, nullptr},    // plain-fp16 precision: conv3x3_f16_rows_kernel 0 never, 1 where its plan is estimated faster than conv3x3_f16_persist_kernel, 2 wherever the shape fits
      {"conv_f16_rows_pin", &m->conv_f16_rows_pin, nullptr},  // tests: the one (R, Wt, MG) tile f16_rows_plan considers, packed R | Wt << 8 | MG << 16 (0: the search)
      {"conv_smallmap", &m->conv_smallmap, nullptr},    // conv3x3_sm_kernel for small maps at small batches: 0 never, 1 where estimated faster (inference plans, conv_splitk = 1), 2 wherever the shape fits
      {"conv_splitk", &m->conv_splitk, nullptr},        // split K on the F(2x2,3x3) kernel for layers with fewer work units than CUs: 0 never, 1 where estimated faster, n >= 2 force n slices
      {"upsample_fold", &m->upsample_fold, nullptr},    // bilinear x2 folded into the F(4x4,3x3) input transform of the conv that consumes it
      {"stem_wino", &m->stem_wino, nullptr},            // second conv of the fused stem in Winograd form
      {"dgrad_wino", &m->dgrad_wino, nullptr},          // 0: direct 9-tap kernels for the backward's data-gradient convs
      {"conv_dma", &m->use_dma, nullptr},               // 0: register-staged 3x3 kernel instead of the LDS-DMA family
      {"conv_dma32", &m->dma32, nullptr},               // 0: Cout <= 48 layers on the register-staged kernel
      {"conv_persist", &m->conv_persist, nullptr},      // 0: one pixel tile per workgroup
      {"conv_c16", &m->conv_c16, nullptr},              // 0: 16 -> 16 channel layers on the generic kernel
      {"conv_dma_stagger", &m->dma_stagger, nullptr},   // 0: SIMD-partner waves issue DMA pieces at the same step
      {"fuse_gelu_fwd", &m->fuse_gelu_fwd, nullptr},
      {"fuse_gelu_bwd", &m->fuse_gelu_bwd, nullptr},
      {"dw_ln_fuse", &m->dw_ln_fuse, nullptr},          // ConvNeXt inference: LayerNorm fused into the depthwise 7x7 kernel
      {"head_fuse", &m->head_fuse, nullptr},            // a 1x1 head on a 64-channel conv output is computed in that conv's F(2x2,3x3) epilogue
      {"pool_peephole", &m->pool_peephole, nullptr},    // unfused programs: a conv whose next op pools its output writes the pooled tensor from its epilogue
      {"mask_fold", &m->mask_fold, nullptr},            // ReLU mask applied by the pool backward that completes a conv output's gradient
      {"wgrad_wino", &m->wgrad_wino, nullptr},          // 3x3 weight gradients: 1 Winograd F(2x2,3x3) domain, 0 direct nine-tap kernel
      {"wgrad_rows", &m->wgrad_rows, nullptr},          // 0 32x32-tile wgrad kernel, 1 auto, 2 nine row-wgrad GEMMs
      {"workspace_reuse", &m->workspace_reuse, nullptr},  // 1: activation slots share memory once their last reader has run (inference programs only); 2: that plan's routing and fusions, every slot in its own range (tests: ph_model_read_slot across a fused launch)
      {"convt_one_launch", &m->convt_one_launch, nullptr},  // 1: the four output-phase GEMMs of a transposed conv in one launch (grid.y = phase); 0: four launches
      {"convt_phase", &m->convt_phase, nullptr},        // 0: transposed convs by zero-stuffing + 3x3 conv (4x the FLOPs; A/B reference)
      {"convnext_f16", &m->convnext_f16, nullptr},      // 1: under conv_precision 2 a ConvNeXt program runs whole in plain fp16 (0: exact fp32 whatever the precision)
      {"swint_f16", &m->swint_f16, nullptr},            // 1: under conv_precision 2 a Swin program runs whole in plain fp16 (0: exact fp32 whatever the precision); independent of convnext_f16
      {"conv_precision", &m->conv_precision, nullptr},  // 0 exact fp32 MFMA, 1 split-fp16 MFMA (22-bit products), 2 plain fp16 (autocast-equivalent)
      {"gemm_late_split", &m->gemm_late_split, nullptr},
      {"gemm_persist2", &m->gemm_persist2, nullptr},
      {"conv_gemm_fill", nullptr, &m->gemm_fill_threshold},            // tile fill below which a 3x3 conv runs as a row GEMM (0 disables)
      {"conv_gemm_fill_wino", nullptr, &m->gemm_fill_threshold_wino},  // ... when the halo kernel is the Winograd one
      {"conv_gemm_fill_wino2d", nullptr, &m->gemm_fill_threshold_wino2d},  // ... when it is the F(2x2,3x3) kernel (16x16-pixel tiles)
  };
}
}  // namespace

int ph_model_set_input_norm(ph_model* m, const float* mean, const float* std, int32_t n) {
  PH_REQUIRE(m && mean && std && n >= 1 && n <= 4, "ph_model_set_input_norm: needs 1..4 channels");
  for (int c = 0; c < n; ++c) PH_REQUIRE(std[c] != 0.f && std::isfinite(std[c]) && std::isfinite(mean[c]), "ph_model_set_input_norm: channel %d has a zero or non-finite statistic", c);
  for (int c = 0; c < n; ++c) {
    m->in_mean[c] = mean[c];
    m->in_std[c] = std[c];
  }
  return PH_OK;
}

int ph_model_set_option(ph_model* m, const char* key, double value) {
  PH_REQUIRE(m && key, "ph_model_set_option: null argument");
  for (const OptionRef& o : option_table(m))
    if (!strcmp(o.key, key)) {
      if (o.i) *o.i = (int)value;
      if (o.d) *o.d = (!strcmp(key, "conv_gemm_fill_wino") || !strcmp(key, "conv_gemm_fill_wino2d")) ? std::max(value, 1e-3) : value;
      return PH_OK;
    }
  set_error("ph_model_set_option: unknown option '%s'", key);
  return PH_E_INVALID;
}

int ph_model_get_option(const ph_model* m, const char* key, double* value) {
  PH_REQUIRE(m && key && value, "ph_model_get_option: null argument");
  for (const OptionRef& o : option_table(const_cast<ph_model*>(m)))
    if (!strcmp(o.key, key)) {
      *value = o.i ? (double)*o.i : *o.d;
      return PH_OK;
    }
  set_error("ph_model_get_option: unknown option '%s'", key);
  return PH_E_INVALID;
}

int ph_model_set_profiling(ph_model* m, int32_t enabled) {
  PH_REQUIRE(m, "ph_model_set_profiling: null model");
  if (enabled && m->ev.empty()) {
    m->ev.resize(m->ops.size() + 1);
    for (auto& e : m->ev) PH_HIP_CHECK(hipEventCreate(&e));
  }
  if (enabled == 1 || m->op_ms.size() != m->ops.size()) {
    m->op_ms.assign(m->ops.size(), 0.0);
    m->profiled_forwards = 0;
    m->events_pending = false;
  }
  m->profiling = enabled != 0;
  return PH_OK;
}

int ph_model_profile_read(ph_model* m, double* op_ms, int32_t n_ops, int32_t* n_forwards) {
  PH_REQUIRE(m && op_ms && n_forwards, "ph_model_profile_read: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_profile_read: model has %d ops", (int)m->ops.size());
  int rc = drain_events(m);
  if (rc != PH_OK) return rc;
  for (int i = 0; i < n_ops; ++i) op_ms[i] = i < (int)m->op_ms.size() ? m->op_ms[i] : 0.0;
  *n_forwards = m->profiled_forwards;
  return PH_OK;
}

int ph_model_last_kernels(const ph_model* m, int32_t* codes, int32_t n_ops) {
  PH_REQUIRE(m && codes, "ph_model_last_kernels: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_last_kernels: model has %d ops", (int)m->ops.size());
  for (int i = 0; i < n_ops; ++i) codes[i] = i < (int)m->last_variant.size() ? m->last_variant[i] : PH_KV_NONE;
  return PH_OK;
}

int ph_model_last_rows_plans(const ph_model* m, int32_t* quad, int32_t n_ops) {
  PH_REQUIRE(m && quad, "ph_model_last_rows_plans: null argument");
  PH_REQUIRE(n_ops == (int32_t)m->ops.size(), "ph_model_last_rows_plans: model has %d ops", (int)m->ops.size());
  for (int i = 0; i < 4 * n_ops; ++i) quad[i] = i < (int)m->last_rows_plan.size() ? m->last_rows_plan[i] : 0;
  return PH_OK;
}

int ph_model_last_ranges(const ph_model* m, int64_t* rows, int32_t max_rows, int32_t* n_rows) {
  PH_REQUIRE(m && n_rows && max_rows >= 0 && (rows || max_rows == 0), "ph_model_last_ranges: bad arguments");
  *n_rows = (int32_t)m->last_ranges.size();
  for (int i = 0; i < max_rows && i < *n_rows; ++i) {
    const RangeRec& r = m->last_ranges[i];
    rows[6 * i] = r.op;
    rows[6 * i + 1] = r.launch;
    rows[6 * i + 2] = r.is_dst;
    rows[6 * i + 3] = r.slot;
    rows[6 * i + 4] = r.offset;
    rows[6 * i + 5] = r.bytes;
  }
  return PH_OK;
}

int ph_model_set_clock_probe(ph_model* m, void* buf_dev) {
  PH_REQUIRE(m, "ph_model_set_clock_probe: null model");
  m->clock_probe = static_cast<unsigned long long*>(buf_dev);
  return PH_OK;
}

int ph_model_read_slot(ph_model* m, int32_t slot, float* out_dev, int64_t out_numel, void* stream) {
  PH_REQUIRE(m && out_dev && m->last_ws, "ph_model_read_slot: no forward has run");
  PH_REQUIRE(slot >= 0 && slot < m->n_slots && m->last_plan.slots[slot].offset >= 0, "bad slot %d", slot);
  PH_REQUIRE(!m->last_plan.recycle, "activations are recycled in this plan: set the handle option workspace_reuse to 0 (or 2) before the forward to read a slot back");
  const SlotShape& s = m->last_plan.slots[slot];
  PH_REQUIRE(out_numel == (int64_t)m->last_batch * s.c * s.h * s.w, "slot %d has %d x %d x %d x %d elements", slot, m->last_batch, s.c, s.h, s.w);
  if (m->last_plan.fmt != FMT_F32)
    return launch_slot_to_nchw_fmt(m->last_plan.fmt, m->last_ws + s.offset, out_dev, m->last_batch, s.h * s.w, s.cp, s.c, static_cast<hipStream_t>(stream));
  return launch_nhwc_to_nchw(reinterpret_cast<float*>(m->last_ws + s.offset), out_dev, m->last_batch, s.h * s.w, s.cp, s.c,
                             static_cast<hipStream_t>(stream));
}

}  // extern "C"
