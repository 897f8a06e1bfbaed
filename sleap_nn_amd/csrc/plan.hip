// Workspace planning of the network path: the activation format a program runs in (forward_format), the slot plan of one forward (build_plan) and the
// predicates of the run-time fusions (fuses_*, defers_upsample_*), which the router (forward.hip) calls and, where a fusion changes lifetimes, build_plan too.
#include <algorithm>
#include <vector>

#include "model_internal.h"

namespace ph {

// Programs made only of the UNet-style ops can run on the fp16 matrix pipe (handle option "conv_precision"); so can, in the
// plain fp16 precision and with the handle option "convnext_f16" set, programs with the ConvNeXt encoder ops (convnext_f16_kernels.hip).  Anything else (class-vector heads
// and the global max pool in front of them, non-3x3 kernels, ConvNeXt programs in the split precision) and every training program
// (conv_precision 0) stays in exact fp32.  A program with the Swin ops (window attention, patch merging) answers to the handle option
// "swint_f16" instead of "convnext_f16" (swin_f16_kernels.hip): the two options are independent, neither changes the other's programs.
int forward_format(const ph_model* m) {
  if (m->conv_precision != 1 && m->conv_precision != 2) return FMT_F32;
  bool swin = false;
  for (const PackedOp& op : m->ops) swin = swin || op.d.kind == PH_OP_WINDOW_ATTN || op.d.kind == PH_OP_PATCH_MERGE;
  for (const PackedOp& op : m->ops)  // a Swinv2 program has no fp16 form: exact whatever the precision and whatever "swint_f16" says
    if (op.d.kind == PH_OP_WINDOW_ATTN_V2) return FMT_F32;
  const bool enc_f16 = m->conv_precision == 2 && (swin ? m->swint_f16 : m->convnext_f16) != 0;  // the encoder ops have an fp16 form and may use it
  for (const PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    switch (d.kind) {
      case PH_OP_STEM:
      case PH_OP_INPUT_CONV:
      case PH_OP_POOL:
      case PH_OP_UPSAMPLE:
        break;
      case PH_OP_PATCH_STEM:
      case PH_OP_DWCONV:
      case PH_OP_LAYERNORM:
      case PH_OP_PATCH_CONV:
      case PH_OP_GELU:
      case PH_OP_SCALE_ADD:
        if (!enc_f16) return FMT_F32;
        break;
      case PH_OP_WINDOW_ATTN:
      case PH_OP_PATCH_MERGE:
        if (!enc_f16) return FMT_F32;
        break;
      case PH_OP_GRN:  // a ConvNeXtV2 program has no fp16 form: exact whatever the precision and whatever "convnext_f16" says
        return FMT_F32;      case PH_OP_LINEAR:  // (a Linear with a ReLU is a class-vector head's: exact; PH_FLAG_RESIDUAL is a Swin block's, with or without a bias)
        if (!enc_f16 || (d.flags & ~(PH_FLAG_GELU | PH_FLAG_SCALE_RESIDUAL | (swin ? PH_FLAG_RESIDUAL : 0))) || !op.w_cnx_f16_dev) return FMT_F32;
        break;
      case PH_OP_CONV:
      case PH_OP_CONVT:
        if (d.ksize != 3) return FMT_F32;
        break;
      case PH_OP_HEAD:
        if (d.flags & PH_FLAG_SOFTMAX) return FMT_F32;
        break;
      default:
        return FMT_F32;
    }
  }
  return m->conv_precision == 1 ? FMT_SPLIT : FMT_F16;
}

bool has_other_reader(const ph_model* m, int slot, size_t except_op) {
  for (size_t k = 0; k < m->ops.size(); ++k)
    if (k != except_op && (m->ops[k].d.src0 == slot || m->ops[k].d.src1 == slot)) return true;
  return false;
}

static bool only_reader_is_next(const ph_model* m, size_t i) { return !has_other_reader(m, m->ops[i].d.dst, i + 1); }  // nothing but op i + 1 reads op i's dst

// inference plans, plain fp16: conv(<= 16 -> 32) + ReLU whose only reader is the next op, a conv(32 -> 32) (+ ReLU, + pool): both in ONE launch, the intermediate
// tensor stays in LDS (block2_c32_f16_kernel).  The conditions are on PADDED channel counts, and the pool is optional: with three convs per block the router takes
// enc0's second and third conv ((16 -> 16), (16 -> 16) + pool: weights and biases zero-padded to 32) and enc1's first and second ((16 -> 32), (32 -> 32) with NO pool
// behind it: dst_pool = nullptr, only the full-resolution tensor is stored) -- both under test in tests/test_gpu_block_structure.py
bool fuses_block2(const ph_model* m, size_t i, int fmt, bool reuse) {
  if (fmt != FMT_F16 || !m->block_fuse || !reuse || i + 1 >= m->ops.size()) return false;
  const PackedOp& op = m->ops[i];
  const PackedOp& nxo = m->ops[i + 1];
  const ph_op_desc& d = op.d;
  const ph_op_desc& nx = nxo.d;
  if (!(d.kind == PH_OP_CONV && d.src0 >= 0 && d.src1 < 0 && d.ksize == 3 && d.dst2 < 0 && op.bn == 32 && fmt_cpad(fmt, d.cout) == 32 && fmt_cpad(fmt, d.cin0) == 32 && d.cin0 <= 16)) return false;
  if (!(nx.kind == PH_OP_CONV && nx.ksize == 3 && nx.src0 == d.dst && nx.src1 < 0 && nxo.bn == 32 && fmt_cpad(fmt, nx.cout) == 32 && nx.cin0 == d.cout)) return false;
  return only_reader_is_next(m, i);
}

// CNBlock's MLP in one launch (inference plans that recycle slots: the 4C-wide hidden tensor is nobody else's business): Linear + GELU whose only reader is a
// Linear with layer scale + residual, both at a width cnblock_mlp_kernel takes
bool fuses_mlp(const ph_model* m, size_t i, int fmt, bool reuse) {
  if (!m->mlp_fuse || !reuse || fmt != FMT_F32 || i + 1 >= m->ops.size()) return false;  // (fp32 only: the fp16 pipe runs the pair as two row GEMMs)
  const PackedOp& op = m->ops[i];
  const PackedOp& nxo = m->ops[i + 1];
  const ph_op_desc& d = op.d;
  const ph_op_desc& nx = nxo.d;
  if (!(d.kind == PH_OP_LINEAR && (d.flags & PH_FLAG_GELU) && op.w_mlp_dev && d.src0 >= 0 && fmt_cpad(fmt, d.cin0) == d.cin0)) return false;
  if (!(nx.kind == PH_OP_LINEAR && (nx.flags & PH_FLAG_SCALE_RESIDUAL) && nxo.w_mlp_dev && nx.src0 == d.dst && nx.src1 >= 0 && nx.src1 != d.dst && nx.cin0 == d.cout && nx.cout == d.cin0 &&
        fmt_cpad(fmt, nx.cout) == nx.cout))
    return false;
  return only_reader_is_next(m, i);
}

// ConvNeXtV2 block on the fused GRN plan (handle option "grn_fuse"): op i = Linear + GELU, i + 1 = GRN, i + 2 = the residual Linear; nobody else reads the two tensors between
bool fuses_grn(const ph_model* m, size_t i, int fmt) {
  if (!m->grn_fuse || fmt != FMT_F32 || m->branch_scales || i + 2 >= m->ops.size()) return false;
  const ph_op_desc& d = m->ops[i].d;
  const ph_op_desc& g = m->ops[i + 1].d;
  const ph_op_desc& l2 = m->ops[i + 2].d;
  if (!(d.kind == PH_OP_LINEAR && d.flags == PH_FLAG_GELU && d.src0 >= 0)) return false;
  if (!(g.kind == PH_OP_GRN && g.src0 == d.dst && g.cin0 == d.cout)) return false;
  if (!(l2.kind == PH_OP_LINEAR && (l2.flags & PH_FLAG_RESIDUAL) && l2.src0 == g.dst && l2.cin0 == g.cout && m->ops[i + 2].b_grn_dev)) return false;
  return only_reader_is_next(m, i) && only_reader_is_next(m, i + 1);
}

// Exact-fp32 inference plans: op i is a bilinear x2 whose only reader is the NEXT op, a 3x3 conv that takes it as its second source -- the op is not launched, the conv
// decides (fwd_conv3x3_f32: the F(4x4,3x3) and small-map kernels up-sample in their input transform; any other kernel gets the tensor produced late)
bool defers_upsample_f32(const ph_model* m, size_t i, const Plan& plan) {
  if (!(plan.fmt == FMT_F32 && plan.reuse && m->upsample_fold && (m->conv_wino4 || m->conv_smallmap) && m->use_dma && i + 1 < m->ops.size())) return false;
  const ph_op_desc& d = m->ops[i].d;
  const PackedOp& nxo = m->ops[i + 1];
  const ph_op_desc& nx = nxo.d;
  if (!(nx.kind == PH_OP_CONV && nx.ksize == 3 && nx.src1 == d.dst && nx.src0 != d.dst && nx.dst2 < 0)) return false;
  if (!((m->conv_wino4 && nxo.w_wino4_dev != nullptr) || (m->conv_smallmap && nxo.w_sm_dev != nullptr))) return false;  // (a form that is switched off does not defer the launch)
  return only_reader_is_next(m, i);
}

// The same on the fp16 pipe: conv3x3_f16_rows_kernel's loader waves blend the half-resolution tensor into the halo (fwd_conv_f16).  NOT the fp32 predicate with another
// format: the conv may carry a fused pool here (no nx.dst2 guard), must have the N tile of 64 that kernel takes, and the map sizes are checked against the plan.
bool defers_upsample_f16(const ph_model* m, size_t i, const Plan& plan) {
  if (!(plan.fmt == FMT_F16 && plan.reuse && m->upsample_fold && m->conv_f16_rows && i + 1 < m->ops.size())) return false;
  const ph_op_desc& d = m->ops[i].d;
  const PackedOp& nxo = m->ops[i + 1];
  const ph_op_desc& nx = nxo.d;
  const SlotShape& s0 = plan.slots[d.src0];
  if (!(nx.kind == PH_OP_CONV && nx.ksize == 3 && nx.src1 == d.dst && nx.src0 != d.dst && nxo.bn == 64 && plan.slots[nx.src0].h == 2 * s0.h && plan.slots[nx.src0].w == 2 * s0.w)) return false;
  return only_reader_is_next(m, i);
}

// Unfused programs (the training forward): op i is a 3x3 conv + ReLU without a pool of its own and op i + 1 is the 2x2 max pool of its output -- the conv's epilogue may write
// both tensors.  Conditions on the program and the options only; whether the kernel that takes the layer can do it is the router's to ask (fwd_conv3x3_f32)
bool fuses_pool(const ph_model* m, size_t i) {
  if (!m->pool_peephole || !m->use_dma || i + 1 >= m->ops.size()) return false;
  const ph_op_desc& d = m->ops[i].d;
  const ph_op_desc& nx = m->ops[i + 1].d;
  return (d.flags & PH_FLAG_RELU) && d.dst2 < 0 && nx.kind == PH_OP_POOL && nx.src0 == d.dst;
}

// Inference plans: op i + 1 is the LayerNorm of op i's dst and nothing else reads that dst -- the producer (patch stem, depthwise conv) may apply it and write the
// LayerNorm's dst.  The producing kernel's own limits (widths, the built-in eps) stay with its routine.
bool fuses_layernorm(const ph_model* m, size_t i, bool reuse) {
  if (!m->dw_ln_fuse || !reuse || i + 1 >= m->ops.size()) return false;
  const ph_op_desc& d = m->ops[i].d;
  const ph_op_desc& nx = m->ops[i + 1].d;
  return nx.kind == PH_OP_LAYERNORM && !(nx.flags & PH_FLAG_RESIDUAL) && nx.src0 == d.dst && nx.cin0 == d.cout && only_reader_is_next(m, i);
}

int build_plan(const ph_model* m, int B, int H, int W, Plan& plan, int fmt) {
  plan.slots.assign(m->n_slots, SlotShape());
  plan.fmt = fmt;
  plan.bpc = fmt_bytes_per_channel(fmt);
  const int bpc = plan.bpc;
  int64_t off = 0, tmp = 0;
  int n_cu = 0;  // CUs of the device, read once where a layer's split-K scratch depends on it
  // Slot allocation.  Default: every slot gets its own range (training keeps every activation; ph_model_read_slot can read any of
  // them back).  With the handle option "workspace_reuse" (inference programs) a slot's range returns to a free list after its
  // last reader and later slots take the best-fitting free block: 9.0 -> 3.6 GB at cfg3 x 32 frames, and a layer's output is
  // written where an older tensor has just left the caches.
  const bool reuse = m->workspace_reuse != 0;
  plan.reuse = reuse;
  plan.recycle = reuse && m->workspace_reuse != 2;
  const int n_ops = (int)m->ops.size();
  std::vector<int> last_use(m->n_slots, -1);
  std::vector<int64_t> slot_bytes(m->n_slots, 0);
  std::vector<char> released(m->n_slots, 0);
  if (reuse)
    for (int j = 0; j < n_ops; ++j) {
      const ph_op_desc& e = m->ops[j].d;
      if (e.src0 >= 0 && e.src0 < m->n_slots) last_use[e.src0] = j;
      if (e.src1 >= 0 && e.src1 < m->n_slots) last_use[e.src1] = j;
    }
  if (reuse)  // a bilinear op the next conv may fold into its input transform (fwd_upsample, defers_upsample_*): that conv then reads the op's SOURCE
    for (int j = 0; j + 1 < n_ops; ++j) {
      const ph_op_desc& e = m->ops[j].d;
      const ph_op_desc& nx = m->ops[j + 1].d;
      if (e.kind == PH_OP_UPSAMPLE && nx.kind == PH_OP_CONV && nx.src1 == e.dst && e.src0 >= 0 && e.src0 < m->n_slots) last_use[e.src0] = std::max(last_use[e.src0], j + 1);
    }
  if (reuse)  // fused GRN plan: the residual Linear reads the GELU output itself, one op after the GRN op that is its last reader in the program
    for (int j = 0; j + 2 < n_ops; ++j)
      if (fuses_grn(m, (size_t)j, fmt)) last_use[m->ops[j].d.dst] = std::max(last_use[m->ops[j].d.dst], j + 2);
  plan.unread.assign(m->n_slots, 0);
  if (reuse)
    for (int sl = 0; sl < m->n_slots; ++sl) plan.unread[sl] = last_use[sl] < 0;
  std::vector<std::pair<int64_t, int64_t>> free_list;  // (offset, bytes), kept sorted and coalesced
  auto release = [&](int slot) {
    free_list.emplace_back(plan.slots[slot].offset, slot_bytes[slot]);
    std::sort(free_list.begin(), free_list.end());
    for (size_t k = 0; k + 1 < free_list.size();)
      if (free_list[k].first + free_list[k].second == free_list[k + 1].first) {
        free_list[k].second += free_list[k + 1].second;
        free_list.erase(free_list.begin() + k + 1);
      } else
        ++k;
    released[slot] = 1;
  };
  auto alloc = [&](int slot, int64_t bytes) {
    bytes = align_up(bytes, 256);
    slot_bytes[slot] = bytes;
    int best = -1;
    for (size_t k = 0; k < free_list.size(); ++k)
      if (free_list[k].second >= bytes && (best < 0 || free_list[k].second < free_list[best].second)) best = (int)k;
    if (best >= 0) {
      const int64_t o = free_list[best].first;
      free_list[best].first += bytes;
      free_list[best].second -= bytes;
      if (free_list[best].second == 0) free_list.erase(free_list.begin() + best);
      return o;
    }
    if (!free_list.empty() && free_list.back().first + free_list.back().second == off) {  // grow the trailing free block
      const int64_t o = free_list.back().first;
      free_list.pop_back();
      off = o + bytes;
      return o;
    }
    const int64_t o = off;
    off += bytes;
    return o;
  };
  int op_i = -1;
  for (const PackedOp& op : m->ops) {
    const ph_op_desc& d = op.d;
    ++op_i;
    // Run-time fusions let op i write op i + 1's dst one op early (pool_peephole: a conv's epilogue writes the pool that follows it;
    // fuse_gelu_fwd: a Linear writes its GELU or its layer-scale + residual; dw_ln_fuse: a depthwise / stem conv writes its LayerNorm).  Such a dst must not land on
    // a range op i is still reading, so the releases due before a pool / GELU / LayerNorm of the previous op's output wait one op.  The same for the second conv of a pair
    // block2_c32_f16_kernel takes (fuses_block2, the router's own predicate): its dst and pooled dst are stored by the launch that DMA-loads the first conv's src0, halo
    // pixels of other workgroups' tiles included, tile rounds apart -- that src0 (released here: its last reader is the first conv) must stay out of the free list.
    // (cnblock_mlp_kernel's pair is NOT held: a row tile reads all of its x and residual rows before it stores them and no other tile reads them, so y exactly on x
    // is safe; ph_model_forward refuses the fusion for any other overlap.)
    const bool forwarded = op_i > 0 && (((d.kind == PH_OP_POOL || d.kind == PH_OP_GELU || d.kind == PH_OP_LAYERNORM || d.kind == PH_OP_SCALE_ADD) && d.src0 >= 0 && d.src0 == m->ops[op_i - 1].d.dst) ||
                                        fuses_block2(m, (size_t)op_i - 1, fmt, reuse));
    if (plan.recycle && !forwarded)  // slots whose last reader ran before this op (a slot nobody reads is released right after the op that wrote it)
      for (int sl = 0; sl < m->n_slots; ++sl)
        if (!released[sl] && plan.slots[sl].offset >= 0 && slot_bytes[sl] > 0 && std::max(last_use[sl], plan.slots[sl].def_op) < op_i) release(sl);
    int h, w;
    if (d.src0 < 0) {
      h = H;
      w = W;
    } else {
      PH_REQUIRE(d.src0 < m->n_slots && plan.slots[d.src0].offset >= 0, "op reads slot %d before it is written", d.src0);
      h = plan.slots[d.src0].h;
      w = plan.slots[d.src0].w;
    }
    if (d.kind == PH_OP_HEAD) continue;
    if (d.kind == PH_OP_STEM) {
      PH_REQUIRE(d.src0 < 0, "stem op must read the network input");
      PH_REQUIRE(d.dst2 >= 0 && d.dst2 < m->n_slots && d.dst < m->n_slots, "bad stem slots");
      if (d.dst >= 0) {
        SlotShape& f = plan.slots[d.dst];
        f.c = d.cout; f.cp = fmt_cpad(fmt, 16); f.h = h; f.w = w; f.def_op = op_i;
        f.offset = alloc(d.dst, (int64_t)B * h * w * f.cp * bpc);
      }
      SlotShape& p = plan.slots[d.dst2];
      p.c = d.cout; p.cp = fmt_cpad(fmt, 16); p.h = (h + 1) / 2; p.w = (w + 1) / 2; p.def_op = op_i;
      p.offset = alloc(d.dst2, (int64_t)B * p.h * p.w * p.cp * bpc);
      continue;
    }
    if (d.kind == PH_OP_RESNET_STEM) {  // dst: the stride-2 conv map (read by the op's own pool launch only), dst2: the pooled map
      PH_REQUIRE(d.src0 < 0, "resnet stem must read the network input");
      PH_REQUIRE(d.dst >= 0 && d.dst < m->n_slots && d.dst2 >= 0 && d.dst2 < m->n_slots && d.dst != d.dst2, "bad resnet stem slots");
      SlotShape& f = plan.slots[d.dst];
      f.c = d.cout; f.cp = fmt_cpad(fmt, d.cout); f.h = (h - 1) / 2 + 1; f.w = (w - 1) / 2 + 1; f.def_op = op_i;
      f.offset = alloc(d.dst, (int64_t)B * f.h * f.w * f.cp * bpc);
      SlotShape& p = plan.slots[d.dst2];
      p.c = d.cout; p.cp = f.cp; p.h = (f.h - 1) / 2 + 1; p.w = (f.w - 1) / 2 + 1; p.def_op = op_i;
      p.offset = alloc(d.dst2, (int64_t)B * p.h * p.w * p.cp * bpc);
      continue;
    }
    int oh = h, ow = w;
    if (d.kind == PH_OP_CONV_S2) {
      PH_REQUIRE(d.src0 >= 0 && h % 2 == 0 && w % 2 == 0, "a stride-2 conv needs an even map, got %dx%d: input H,W must be multiples of the model max stride", h, w);
      oh = h / 2;
      ow = w / 2;
    } else if (d.kind == PH_OP_ADD_RELU) {
      PH_REQUIRE(d.src0 >= 0 && d.src1 >= 0 && d.src1 < m->n_slots && plan.slots[d.src1].offset >= 0, "add: slot %d is not written yet", d.src1);
      const SlotShape& s1 = plan.slots[d.src1];
      PH_REQUIRE(s1.h == h && s1.w == w && s1.c == d.cout && plan.slots[d.src0].c == d.cout, "add: the two sources differ in shape");
    }
    if (d.kind == PH_OP_PATCH_STEM) {
      PH_REQUIRE(d.src0 < 0, "patch stem must read the network input");
      const int pad2 = (d.flags & PH_FLAG_PAD0_NORM) ? 0 : 2;
      oh = (h + pad2 - d.ksize) / d.cmid + 1;
      ow = (w + pad2 - d.ksize) / d.cmid + 1;
      PH_REQUIRE(oh > 0 && ow > 0, "input %dx%d is too small for the %dx%d patch stem", h, w, d.ksize, d.ksize);
    } else if (d.kind == PH_OP_PATCH_CONV) {
      oh = h / 2;
      ow = w / 2;
      PH_REQUIRE(oh > 0 && ow > 0, "input of a 2x2/stride-2 convolution is smaller than 2x2");
    } else if (d.kind == PH_OP_PATCH_MERGE) {  // pad to even, four phases on the channels
      oh = (h + 1) / 2;
      ow = (w + 1) / 2;
      PH_REQUIRE(plan.slots[d.src0].c == d.cin0 && d.cout == 4 * d.cin0, "patch merge channel mismatch");
    } else if (d.kind == PH_OP_WINDOW_ATTN || d.kind == PH_OP_WINDOW_ATTN_V2) {
      PH_REQUIRE(d.src0 >= 0 && plan.slots[d.src0].c == d.cin0 && d.cin0 == 3 * d.cout, "window attention reads a (3C)-channel qkv slot");
    } else if ((d.kind == PH_OP_LINEAR && (d.flags & (PH_FLAG_SCALE_RESIDUAL | PH_FLAG_RESIDUAL))) || d.kind == PH_OP_SCALE_ADD ||
               (d.kind == PH_OP_LAYERNORM && (d.flags & PH_FLAG_RESIDUAL))) {
      PH_REQUIRE(d.src1 >= 0 && d.src1 < m->n_slots && plan.slots[d.src1].offset >= 0, "residual slot %d is not written yet", d.src1);
      const SlotShape& s1 = plan.slots[d.src1];
      PH_REQUIRE(s1.h == h && s1.w == w && s1.c == d.cout, "residual shape mismatch");
    }
    if (d.kind == PH_OP_GLOBAL_MAXPOOL) {
      oh = 1;
      ow = 1;
    }
    if (d.kind == PH_OP_POOL) {
      oh = (h + 1) / 2;
      ow = (w + 1) / 2;
    } else if (d.kind == PH_OP_UPSAMPLE || d.kind == PH_OP_CONVT) {
      oh = 2 * h;
      ow = 2 * w;
    }
    if (d.kind == PH_OP_CONV && d.src1 >= 0) {
      const SlotShape& s1 = plan.slots[d.src1];
      PH_REQUIRE(s1.offset >= 0, "op reads slot %d before it is written", d.src1);
      PH_REQUIRE(s1.h == h && s1.w == w,
                 "concat sources differ in size (%dx%d vs %dx%d): input H,W must be multiples of the model max stride",
                 h, w, s1.h, s1.w);
    }
    if (d.kind == PH_OP_CONVT) tmp = std::max<int64_t>(tmp, (int64_t)B * oh * ow * fmt_cpad(fmt, d.cin0) * bpc);
    if (d.kind == PH_OP_GRN) {  // the slice sums of grn_reduce_kernel
      PH_REQUIRE(fmt == FMT_F32 && d.src0 >= 0 && plan.slots[d.src0].c == d.cin0 && d.cin0 == d.cout, "GRN channel mismatch");
      tmp = std::max<int64_t>(tmp, grn_scratch_floats(B, h * w, pad16(d.cout)) * (int64_t)sizeof(float));
      if (op_i >= 1 && fuses_grn(m, (size_t)op_i - 1, fmt)) {  // block sums of the first Linear's epilogue, then one scaled weight image per sample for the second
        const PackedOp& l2 = m->ops[op_i + 1];
        tmp = std::max<int64_t>(tmp, grn_fused_partial_floats(B * h * w, h * w, pad16(d.cout)) * (int64_t)sizeof(float));
        tmp = std::max<int64_t>(tmp, (int64_t)B * gemm_pack_floats(pad16(l2.d.cout), pad16(d.cout), l2.bn) * (int64_t)sizeof(float));
      }
    }
    if (d.kind == PH_OP_CONV && d.ksize == 3 && fmt == FMT_F32 && (m->conv_splitk >= 2 || (m->conv_splitk == 1 && reuse))) {  // (auto: inference plans only, as the kernel choice below)  // partial-sum planes of a split-K launch (conv3x3_wino2d_kernel<.., KS>)
      if (!n_cu) {
        const int rc = device_cu_count(&n_cu);
        if (rc != PH_OK) return rc;
      }
      tmp = std::max<int64_t>(tmp, wino2d_split_scratch_bytes(B, h, w, pad16(d.cin0) + (d.src1 >= 0 ? pad16(d.cin1) : 0), pad16(d.cout), m->conv_splitk, n_cu));
      if (m->conv_wino4) tmp = std::max<int64_t>(tmp, wino4_split_scratch_bytes(B, h, w, pad16(d.cin0) + (d.src1 >= 0 ? pad16(d.cin1) : 0), pad16(d.cout), m->conv_splitk, n_cu));
    }
    PH_REQUIRE(d.dst >= 0 && d.dst < m->n_slots, "bad dst slot %d", d.dst);
    SlotShape& s = plan.slots[d.dst];
    s.c = (d.kind == PH_OP_POOL || d.kind == PH_OP_UPSAMPLE || d.kind == PH_OP_GLOBAL_MAXPOOL) ? d.cin0 : d.cout;
    s.cp = fmt_cpad(fmt, s.c);
    s.h = oh;
    s.w = ow;
    s.def_op = op_i;
    s.offset = alloc(d.dst, (int64_t)B * oh * ow * s.cp * bpc);
    if (d.kind == PH_OP_CONV && d.dst2 >= 0) {  // fused 2x2 max pool of the conv output
      PH_REQUIRE(d.dst2 < m->n_slots && (d.flags & PH_FLAG_RELU), "fused pool needs a valid slot and a ReLU conv");
      SlotShape& p = plan.slots[d.dst2];
      p.c = d.cout;
      p.cp = fmt_cpad(fmt, d.cout);
      p.h = (oh + 1) / 2;
      p.w = (ow + 1) / 2;
      p.def_op = op_i;
      p.offset = alloc(d.dst2, (int64_t)B * p.h * p.w * p.cp * bpc);
    }
  }
  plan.tmp_offset = off;
  plan.tmp_bytes = align_up(tmp, 256);
  plan.total = off + plan.tmp_bytes;
  return PH_OK;
}

}  // namespace ph
