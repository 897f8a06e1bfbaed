// State of one ph_model_forward call (forward.hip): what the per-op launch routines (fwd_*) share.  Host bookkeeping only.
#pragma once
#include <vector>

#include "model_internal.h"

namespace ph {

// diagnostic clock probe (ph_model_set_clock_probe): 64-bit words reserved per op of the program -- the largest writer (the F(2x2,3x3) kernel's stamps) takes 256 x 8 x 8
static constexpr size_t PH_PROBE_WORDS_PER_OP = 32768;

struct ForwardCtx {
  // ---- constants of the call
  ph_model* const m;
  const Plan& plan;
  const int fmt;      // activation format of every slot (= plan.fmt)
  const int rs_div;   // pixel stride in 4-byte units = cp / rs_div
  const int batch, height, width, in_channels, in_dtype;
  const void* const input_dev;
  char* const ws;
  float* const* const out_dev;
  const hipStream_t s;
  int* const kv;      // PH_KV_* code per op (m->last_variant)
  const int n_cu;     // CUs of the device, read once per call: what every routing estimate of the call is made with

  // ---- the range recorder.  Every slot pointer that goes into a launcher's arguments is taken through rd() (a source) or wr() (a destination), which note the slot's
  // byte range under the current op and launch (ph_model_last_ranges): the record follows the routing, whatever it decides.
  std::vector<RangeRec>& rr;  // m->last_ranges
  size_t op_index = 0;        // ops dispatched so far, the current one included: the current op is op_index - 1, the next one op_index
  int launch_no = 0;          // launch ordinal within the current op

  // ---- the cross-op notes: what one op's routine leaves for a later op's.  All back at rest after the last op (ph_model_forward checks)
  bool skip_next_gelu = false;       // set by fwd_linear_f32 (its epilogue wrote the GELU op behind it), cleared by fwd_gelu
  bool skip_next_scale_add = false;  // set by fwd_linear_f32 (its epilogue wrote the scale-add op behind it), cleared by fwd_scale_add
  bool skip_next_linear = false;     // set by fwd_linear_mlp (cnblock_mlp_kernel computed the second Linear with the first), cleared by fwd_linear
  int pooled_by_conv = -1;           // slot whose 2x2 max pool the producing conv's epilogue already wrote (pool peephole): set by fwd_conv3x3_f32, cleared by fwd_pool
  int deferred_up = -1;              // index of a bilinear op left to the conv that follows it: set by fwd_upsample, cleared by fwd_conv (which hands it to fwd_conv_f16 / fwd_conv3x3_f32)
  int fused_grn = -1;                // fused GRN plan: 1-based index of the op of a ConvNeXtV2 block that ran last on that plan: set by fwd_linear_f32 (Linear + GELU), moved on by fwd_grn, cleared by fwd_linear_grn (the residual Linear)
  int fused_ln = -1;                 // index of a LayerNorm op its producer already applied: set by ride_layernorm (fwd_patch_stem, fwd_dwconv), cleared by fwd_layernorm
  std::vector<char> head_done;       // head ops the producing conv's epilogue already computed: set by attach_head (fwd_conv_f16 may take it back), read by fwd_head
  std::vector<char> conv_done;       // conv ops the conv in front of them already computed (two-conv block kernel): set by fwd_conv_f16, read by fwd_conv
  int branch = 0;                    // residual Linear ops seen so far (row of the branch scales); fwd_linear_f32

  int op_i() const { return (int)op_index - 1; }
  const PackedOp* next_op() const { return op_index < m->ops.size() ? &m->ops[op_index] : nullptr; }
  const SlotShape& slot(int sidx) const { return plan.slots[sidx]; }
  static int relu(const ph_op_desc& d) { return (d.flags & PH_FLAG_RELU) ? 1 : 0; }
  void ran(int variant) { kv[op_index - 1] = variant; }  // the kernel the current op ran (ph_model_last_kernels)
  unsigned long long* probe_block() const { return m->clock_probe ? m->clock_probe + PH_PROBE_WORDS_PER_OP * (op_index - 1) : nullptr; }  // one record block per op (diagnostic builds / kernels that stamp)
  // a conv with a fused pool whose full-resolution output nothing reads (inference plans; e.g. cfg3's second encoder block: 1 GiB per 32 frames): only the pool is stored
  bool pool_dst_unread(const ph_op_desc& d) const { return d.dst2 >= 0 && plan.reuse && !plan.unread.empty() && plan.unread[d.dst]; }
  float* scratch() const { return reinterpret_cast<float*>(ws + plan.tmp_offset); }  // the scratch region behind the slots (note_tmp records its use)

  int64_t slot_bytes(int sidx) const {
    const SlotShape& q = plan.slots[sidx];
    return (int64_t)batch * q.h * q.w * q.cp * plan.bpc;
  }
  void note(int is_dst, int sidx, int64_t offset, int64_t bytes) { rr.push_back(RangeRec{(int)op_index - 1, launch_no, is_dst, sidx, offset, bytes}); }
  float* rd(int sidx) {
    note(0, sidx, plan.slots[sidx].offset, slot_bytes(sidx));
    return reinterpret_cast<float*>(ws + plan.slots[sidx].offset);
  }
  float* wr(int sidx) {
    note(1, sidx, plan.slots[sidx].offset, slot_bytes(sidx));
    return reinterpret_cast<float*>(ws + plan.slots[sidx].offset);
  }
  void note_tmp(int is_dst) { note(is_dst, -1, plan.tmp_offset, plan.tmp_bytes); }
  void unnote(int is_dst, int sidx) {  // a pointer of the current launch that was replaced before the launch
    for (size_t k = rr.size(); k-- > 0 && rr[k].op == (int)op_index - 1;)
      if (rr[k].launch == launch_no && rr[k].is_dst == is_dst && rr[k].slot == sidx) {
        rr.erase(rr.begin() + k);
        return;
      }
  }
  void launch_before() {  // the ranges noted so far belong to a launch that runs AFTER the one about to be made (a deferred bilinear produced after all)
    for (size_t k = rr.size(); k-- > 0 && rr[k].op == (int)op_index - 1;)
      if (rr[k].launch == launch_no) rr[k].launch += 1;
  }
  size_t mark() const { return rr.size(); }         // mark() ... rollback(mark): the ranges a trial set of arguments noted, dropped when the trial is not taken
  void rollback(size_t mark) { rr.resize(mark); }
  void next_launch() { ++launch_no; }
};

}  // namespace ph
