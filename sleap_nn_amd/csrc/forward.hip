// The forward launch sequence of the network path (C ABI: ph_model_forward): one launch routine per op kind (fwd_*) over one ForwardCtx, which carries the call's
// constants, the launch record of ph_model_last_ranges and the notes one op leaves for a later one (the run-time fusions).  Host code only: every kernel is behind a
// launch_* function.  Replaces Model.forward -> UNet.forward of the reference (architectures/model.py:237-261, architectures/unet.py:260-299).
#include <algorithm>
#include <vector>

#include "forward_internal.h"
#include "train_kernels.h"

using namespace ph;

namespace {

// ---- pieces several routines share

// The first head op behind the current op that reads `slot` (a conv's dst), -1 if none: the candidate for that conv's epilogue.  Only the FIRST such head is looked at.
int find_head_reader(const ForwardCtx& c, int slot) {
  for (size_t j = c.op_index; j < c.m->ops.size(); ++j)
    if (c.m->ops[j].d.kind == PH_OP_HEAD && c.m->ops[j].d.src0 == slot) return (int)j;
  return -1;
}

// What every fused-head form asks of the head op itself; the shape conditions differ per kernel and stay with the callers
bool head_can_ride(const ForwardCtx& c, const ph_op_desc& hx) { return !(hx.flags & PH_FLAG_SOFTMAX) && c.out_dev[hx.out_index]; }

// Head op j rides in the epilogue of the conv whose arguments are `a` (ConvArgs / ConvF16Args: the same head_* fields).  When nothing else reads the conv's dst the tensor
// never reaches HBM (inference plans; training keeps every activation).
template <typename Args>
void attach_head(ForwardCtx& c, Args& a, int j, int wcp, int conv_dst) {
  const PackedOp& h = c.m->ops[j];
  a.head_w = h.w_dev;
  a.head_b = h.b_dev;
  a.head_dst = c.out_dev[h.d.out_index];
  a.head_cout = h.d.cout;
  a.head_wcp = wcp;
  a.head_sigmoid = head_sigmoid(c.m, c.plan, h.d);
  c.head_done[j] = 1;
  if (c.plan.reuse && !has_other_reader(c.m, conv_dst, (size_t)j)) a.skip_dst = 1;
}

// The LayerNorm op behind the current op (fuses_layernorm holds) rides in the kernel whose arguments are `a` (PatchStemArgs / DwConvArgs / DwConvF16Args): the kernel takes
// the affine and writes the LayerNorm's dst in place of its own
template <typename Args>
void ride_layernorm(ForwardCtx& c, const ph_op_desc& d, Args& a) {
  const PackedOp& ln = *c.next_op();
  a.ln_gamma = ln.w_dev;
  a.ln_beta = ln.b_dev;
  a.ln_c = d.cout;
  c.unnote(1, d.dst);
  a.dst = c.wr(ln.d.dst);
  c.fused_ln = (int)c.op_index;
}

// what the two users of the fp16 3x3 conv kernels (fwd_conv_f16, fwd_convt_stuffed) fill alike; sources, dst and pool are the caller's
void conv_f16_common(const ForwardCtx& c, const PackedOp& op, int c0p, int H, int W, ConvF16Args& f) {
  const SlotShape& so = c.slot(op.d.dst);
  f.rs0 = c0p / c.rs_div;
  f.chunks0 = c0p / (c.fmt == FMT_F16 ? 32 : 16);
  f.wpack = op.w_f16_dev[c.fmt == FMT_F16 ? 1 : 0];
  f.bias = op.b_dev;
  f.rs_dst = so.cp / c.rs_div;
  f.coutp = so.cp;
  f.B = c.batch;
  f.H = H;
  f.W = W;
  f.relu = c.relu(op.d);
  f.bn = op.bn;
  f.prec = c.fmt == FMT_F16 ? 1 : 3;
  f.zeros = c.m->zeros_dev;
  f.clock_probe = c.probe_block();
}

// records and launches the kernel the route names
int launch_routed(ForwardCtx& c, const ConvArgs& a, const ConvRoute& r) {
  c.ran(r.kv);
  return launch_conv3x3_routed(a, r, c.s);
}

// ---- network input

int fwd_input_conv(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  PH_REQUIRE(d.cin0 == c.in_channels, "input has %d channels, network expects %d", c.in_channels, d.cin0);
  InputConvArgs a{};
  a.src = c.input_dev;
  a.w = op.w_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.dtype = c.in_dtype;
  a.cin = d.cin0;
  a.coutp = pad16(d.cout);
  a.B = c.batch;
  a.H = c.height;
  a.W = c.width;
  a.relu = c.relu(d);
  a.ksize = d.ksize;
  a.out_fmt = c.fmt;
  a.dst_cp = c.slot(d.dst).cp;
  return launch_input_conv(a, c.s);
}

int fwd_stem(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  PH_REQUIRE(d.cin0 == c.in_channels, "input has %d channels, network expects %d", c.in_channels, d.cin0);
  StemArgs a{};
  a.src = c.input_dev;
  a.w0 = op.w_dev;
  a.b0 = op.b_dev;
  a.w1 = op.w2_dev;
  a.w1w = op.w_wino_dev;
  a.w1w2 = op.w_stem2_dev;
  a.b1 = op.b2_dev;
  a.dst_full = d.dst >= 0 ? c.wr(d.dst) : nullptr;
  a.dst_pool = c.wr(d.dst2);
  a.dtype = c.in_dtype;
  a.cin = d.cin0;
  a.B = c.batch;
  a.H = c.height;
  a.W = c.width;
  a.wino = c.m->stem_wino;
  a.f16_mfma = c.m->stem_f16mfma;
  a.out_fmt = c.fmt;
  c.ran(PH_KV_STEM);
  return launch_stem(a, c.s);
}

int fwd_patch_stem(ForwardCtx& c, const PackedOp& op) {
  const ph_model* m = c.m;
  const ph_op_desc& d = op.d;
  PH_REQUIRE(d.cin0 == c.in_channels, "input has %d channels, network expects %d", c.in_channels, d.cin0);
  const SlotShape& so = c.slot(d.dst);
  if (c.fmt == FMT_F16 && !(d.flags & PH_FLAG_PAD0_NORM)) {
    PatchStemF16Args f{};
    f.src = c.input_dev;
    f.w = op.w_dev;
    f.bias = op.b_dev;
    f.dst = c.wr(d.dst);
    f.dtype = c.in_dtype;
    f.cin = d.cin0;
    f.wcp = pad16(d.cout);
    f.cp = so.cp;
    f.B = c.batch;
    f.H = c.height;
    f.W = c.width;
    f.OH = so.h;
    f.OW = so.w;
    f.k = d.ksize;
    f.stride = d.cmid;
    c.ran(PH_KV_CNX_F16_STEM);
    return launch_patch_stem_f16(f, c.s);
  }
  PH_REQUIRE(!(d.flags & PH_FLAG_PAD0_NORM) || c.fmt == FMT_F32, "the padding-0 patch stem runs in exact fp32 only");
  PatchStemArgs a{};
  a.src = c.input_dev;
  a.w = op.w_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.dtype = c.in_dtype;
  a.cin = d.cin0;
  a.coutp = so.cp;
  a.B = c.batch;
  a.H = c.height;
  a.W = c.width;
  a.OH = so.h;
  a.OW = so.w;
  a.k = d.ksize;
  a.stride = d.cmid;
  if (d.flags & PH_FLAG_PAD0_NORM) {  // ConvNeXtV2 embeddings: padding 0, (x / 255 - mean) / std on the way in
    a.pad0_norm = 1;
    for (int ch = 0; ch < 4; ++ch) {
      a.mean[ch] = m->in_mean[ch];
      a.std[ch] = m->in_std[ch];
    }
    c.ran(PH_KV_PATCH_STEM_NORM);
    return launch_patch_stem_norm(a, c.s);
  }
  // the stem's LayerNorm2d rides in the patch kernel (inference plans: nothing else reads the un-normalised tensor); the fused form has eps 1e-6 built in
  if (c.fmt == FMT_F32 && a.cin == 1 && a.coutp <= 128 && a.k >= 2 && a.k <= 4 && a.stride >= 1 && a.stride <= 4 && fuses_layernorm(m, c.op_i(), c.plan.reuse) &&
      !(c.next_op()->d.flags & PH_FLAG_LN_EPS_1EM5))
    ride_layernorm(c, d, a);
  return launch_patch_stem(a, c.s);
}

// ---- 3x3 / k x k convolutions

// plain fp16: this conv and the one behind it in ONE launch, the tensor between them stays in LDS (block2_c32_f16_kernel; fuses_block2 holds and the weight forms exist)
int fwd_conv_block2(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const PackedOp& nxo = *c.next_op();
  const ph_op_desc& nx = nxo.d;
  const SlotShape& s0 = c.slot(d.src0);
  Block2Args b2{};
  b2.src = c.rd(d.src0);
  b2.wa = op.w_f16_dev[1];
  b2.wb = nxo.w_f16_dev[1];
  b2.ba = op.b_dev;
  b2.bb = nxo.b_dev;
  b2.dst_full = c.pool_dst_unread(nx) ? nullptr : c.wr(nx.dst);
  b2.dst_pool = nx.dst2 >= 0 ? c.wr(nx.dst2) : nullptr;
  b2.B = c.batch;
  b2.H = s0.h;
  b2.W = s0.w;
  b2.relu_a = c.relu(d);
  b2.relu_b = c.relu(nx);
  b2.zeros = c.m->zeros_dev;
  c.conv_done[c.op_index] = 1;
  c.ran(PH_KV_F16_BLOCK);
  return launch_block2_c32_f16(b2, c.s);
}

// 3x3 conv on the fp16 matrix pipe (split or plain fp16).  `up`: index of a bilinear op in front that was left to this conv, or -1
int fwd_conv_f16(ForwardCtx& c, const PackedOp& op, int up) {
  const ph_model* m = c.m;
  const Plan& plan = c.plan;
  const ph_op_desc& d = op.d;
  const int fmt = c.fmt, rs_div = c.rs_div;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0 && (d.src1 < 0 || c.slot(d.src1).c == d.cin1), "conv channel mismatch");
  const SlotShape& so = c.slot(d.dst);
  if (fuses_block2(m, c.op_i(), fmt, plan.reuse)) {  // (the predicate build_plan holds this pair's releases on)
    const PackedOp& nxo = *c.next_op();
    if (nxo.w_f16_dev[1] && op.w_f16_dev[1] && so.cp == 32 && s0.cp == 32 && c.slot(nxo.d.dst).cp == 32) return fwd_conv_block2(c, op);
  }
  ConvF16Args f{};
  f.src0 = c.rd(d.src0);
  if (d.src1 >= 0) {
    f.src1 = c.rd(d.src1);
    f.rs1 = c.slot(d.src1).cp / rs_div;
    f.chunks1 = c.slot(d.src1).cp / (fmt == FMT_F16 ? 32 : 16);
  }
  f.dst = c.wr(d.dst);
  f.dst_pool = d.dst2 >= 0 ? c.wr(d.dst2) : nullptr;
  f.skip_dst = c.pool_dst_unread(d) ? 1 : 0;
  conv_f16_common(c, op, s0.cp, s0.h, s0.w, f);
  int head = -1;
  if (m->head_fuse && fmt == FMT_F16 && !f.dst_pool && op.bn == 64 && (so.cp == 64 || (so.cp == 128 && m->conv_f16_rows))) {
    // plain fp16: a 1x1 head that reads this conv's 64-channel output rides in its epilogue (four MFMAs on the staged fp16 row)
    // (128 channels: only conv3x3_f16_rows_kernel holds both N tiles of a pixel in one workgroup -- undone below if that kernel does not take the layer)
    // (eligibility: the head's input channels padded for the FORMAT equal this conv's; the transposed-conv form in fwd_convt_stuffed asks for pad16(..) == 64 instead)
    head = find_head_reader(c, d.dst);
    if (head >= 0 && head_can_ride(c, m->ops[head].d) && m->ops[head].d.cout <= 32 && fmt_cpad(FMT_F16, m->ops[head].d.cin0) == so.cp) attach_head(c, f, head, so.cp, d.dst);
  }
  if (up >= 0 || (fmt == FMT_F16 && m->conv_f16_rows)) {
    // conv3x3_f16_rows_kernel (row tiles, loader waves, weights L2 -> registers; f16_rows_kernels.hip) where its plan is estimated faster ("conv_f16_rows" 2: wherever
    // the shape fits).  A bilinear x2 in front of this conv that only feeds its second source was not launched (fwd_upsample): the kernel reads the
    // half-resolution tensor itself; if it does not take the layer, the tensor is produced now.
    const int n_cu = c.n_cu;
    bool on_rows = false;
    if (fmt == FMT_F16 && m->conv_f16_rows) {
      ConvF16Args r = f;
      const size_t mark = c.mark();
      if (up >= 0) {
        const ph_op_desc& u = m->ops[up].d;
        r.src1 = c.rd(u.src0);
        r.rs1 = c.slot(u.src0).cp / rs_div;
        r.src1_lowres = 1;
        r.rows_blend16 = m->upsample_f16math ? 1 : 0;
      }
      const double c_rows = f16_rows_plan(r, n_cu, m->conv_f16_rows_pin);
      double c_old = f16_conv_cost(f, n_cu);
      if (up >= 0) c_old += f16_upsample_cost(c.batch, s0.h / 2, s0.w / 2, c.slot(d.src1).cp, n_cu);
      if (f.head_w && !(f.bn == 64 && f.coutp == 64))  // a head only the row-tile kernel fuses: the other way costs head1x1_mfma_kernel's launch (its bytes at ~5 TB/s + the boundary)
        c_old += (double)c.batch * s0.h * s0.w * (f.coutp * 2.0 + f.head_cout * 4.0) / 2500.0 + 3000.0;
      if (c_rows >= 0 && (m->conv_f16_rows >= 2 || c_rows < 0.95 * c_old)) {  // (the estimates are good to a few per cent: a tie stays with the round-2 kernel, measured 6 - 8 % faster on the 2-chunk 192 x 192 layers of cfg5)
        f = r;
        on_rows = true;
        if (up >= 0) c.unnote(0, d.src1);  // (the half-resolution tensor took the up-sampled one's place)
      } else {
        c.rollback(mark);
      }
    }
    if (up >= 0 && !on_rows) {
      const ph_op_desc& u = m->ops[up].d;
      const SlotShape& sl = c.slot(u.src0);
      c.launch_before();
      int rc = launch_upsample_fmt(fmt, c.rd(u.src0), c.wr(u.dst), c.batch, sl.h, sl.w, sl.cp, c.s, (fmt == FMT_F16 && m->upsample_f16math) ? 1 : 0);
      if (rc != PH_OK) return rc;
      c.next_launch();
    }
    if (on_rows) {
      c.ran(PH_KV_F16_ROWS);
      const int32_t quad[4] = {f.rows_r, f.rows_wt, f.rows_mt, f.rows_mg};
      std::copy(quad, quad + 4, c.m->last_rows_plan.begin() + 4 * c.op_i());
      return launch_conv3x3_f16_rows(f, c.s);
    }
    if (f.head_w && (f.bn != 64 || f.coutp != 64)) {  // (a head only the row-tile kernel fuses: leave it to its own launch)
      c.head_done[head] = 0;
      f.head_w = nullptr;
      f.skip_dst = c.pool_dst_unread(d) ? 1 : 0;
    }
  }
  c.ran(PH_KV_F16);
  return launch_conv3x3_f16(f, c.s);
}

// A conv as a row GEMM over its taps (gemm_mfma_dma_kernel): mode 2 = the nine taps of a 3x3 conv, mode 5 = the k^2 taps of a k x k "same" conv
int launch_conv_rowgemm(ForwardCtx& c, const PackedOp& op, const float* src0, int c0p, const float* src1, int c1p, float* dst, int coutp, int mode) {
  const SlotShape& s0 = c.slot(op.d.src0);
  GemmArgs g{};
  g.src0 = src0;
  g.src1 = src1;
  g.c0p = c0p;
  g.c1p = c1p;
  g.wpack = op.w_gemm_dev;
  g.bias = op.b_gemm_dev;
  g.dst = dst;
  g.zeros = c.m->zeros_dev;
  g.coutp = coutp;
  g.bn = op.bn_g;
  g.M = c.batch * s0.h * s0.w;
  g.mode = mode;
  g.H = s0.h;
  g.W = s0.w;
  g.act = c.relu(op.d);
  g.late_split = c.m->gemm_late_split;
  if (mode == 5) g.ksize = op.d.ksize;
  else g.persist2 = c.m->gemm_persist2;
  c.ran(PH_KV_ROWGEMM);
  return launch_gemm(g, c.s);
}

// k x k "same" conv, k != 3: k^2-tap row GEMM (exact fp32; inference only)
int fwd_conv_kxk(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0 && (d.src1 < 0 || c.slot(d.src1).c == d.cin1), "conv channel mismatch");
  const float* const src0 = c.rd(d.src0);
  const float* const src1 = d.src1 >= 0 ? c.rd(d.src1) : nullptr;
  int rc = launch_conv_rowgemm(c, op, src0, s0.cp, src1, d.src1 >= 0 ? c.slot(d.src1).cp : 0, c.wr(d.dst), pad16(d.cout), 5);
  if (rc == PH_OK && d.dst2 >= 0) {  // the fused-pool flag of the plan, unfused here
    c.next_launch();
    rc = launch_pool(c.rd(d.dst), c.wr(d.dst2), c.batch, s0.h, s0.w, pad16(d.cout), c.s);
  }
  return rc;
}

// The op before this conv is a bilinear x2 (op `up`) that only feeds its second source and was not launched: the F(4x4,3x3) and small-map kernels read the
// half-resolution tensor themselves (the up-sampling rides in their input transform); any other kernel gets the tensor now.
int resolve_deferred_up_f32(ForwardCtx& c, const ph_op_desc& d, int up, ConvArgs& a) {
  const ph_op_desc& u = c.m->ops[up].d;
  const SlotShape& sl = c.slot(u.src0);
  ConvArgs f = a;
  const size_t mark = c.mark();
  f.src1 = c.rd(u.src0);
  f.src1_lowres = 1;
  if (conv3x3_route(f, c.n_cu).folds_lowres) {
    a = f;
    c.unnote(0, d.src1);  // (the half-resolution tensor took the up-sampled one's place)
    return PH_OK;
  }
  c.rollback(mark);
  c.launch_before();
  int rc = launch_upsample(c.rd(u.src0), c.wr(u.dst), c.batch, sl.h, sl.w, sl.cp, c.s);
  if (rc != PH_OK) return rc;
  c.next_launch();
  return PH_OK;
}

// small feature map (the 16x32-pixel tiles of the halo kernel would be mostly padding) or a Cout that fits the halo kernel's N tile badly -> 9-tap row GEMM
bool conv3x3_prefers_rowgemm(const ForwardCtx& c, const PackedOp& op, const ConvArgs& a) {
  const ph_model* m = c.m;
  const SlotShape& s0 = c.slot(op.d.src0);
  if (!(m->use_dma && op.d.dst2 < 0 && op.w_gemm_dev && !a.src1_lowres)) return false;
  const double fill = (double)s0.h * s0.w / ((double)((s0.h + 15) / 16 * 16) * ((s0.w + 31) / 32 * 32));
  // the halo kernel pads Cout to a multiple of its N tile (64): e.g. Cout = 96 does 33 % extra MFMA work there,
  // none in the row GEMM (N tiles of 96 / 128)
  const double n_fill = (double)a.coutp / ((a.coutp + op.bn - 1) / op.bn * op.bn);
  const int bn_g = op.bn_g > 0 ? op.bn_g : 128;
  const double n_fill_g = (double)a.coutp / ((a.coutp + bn_g - 1) / bn_g * bn_g);
  // the halo kernel runs Winograd F(2,3) (2/3 of the MFMA work) where its weights exist: it wins down to ~0.5 tile fill (measured on the ConvNeXt decoder: 48x48 and 24x24 maps)
  double halo_gain = (op.w_wino_dev && m->use_dma) ? m->gemm_fill_threshold / m->gemm_fill_threshold_wino : 1.0;
  double halo_fill = fill;
  if (conv3x3_wino2d_sets_rowgemm_fill(a)) {
    // the F(2x2,3x3) kernel: 16x16-pixel tiles and 4/9 of the MFMA work -- it beats the 9-tap row GEMM down to ~0.4 tile fill
    halo_fill = (double)s0.h * s0.w / ((double)((s0.h + 15) / 16 * 16) * ((s0.w + 15) / 16 * 16));
    halo_gain = m->gemm_fill_threshold / m->gemm_fill_threshold_wino2d;
  }
  return halo_fill * halo_gain < m->gemm_fill_threshold || n_fill * halo_fill * halo_gain < 0.8 * n_fill_g;
}

// A 1x1 head that reads this conv's output rides in the epilogue of the F(2x2,3x3) kernel (the accumulator layout is the MFMA's B operand: conv3x3_wino2d_kernel), of the
// wave-private kernel or of the small-map kernel.  (Eligibility is per kernel and on pad16 of the head's input channels: exact fp32 pads to 16, unlike the fp16 form.)
void try_head_f32(ForwardCtx& c, const ph_op_desc& d, ConvArgs& a, const ConvRoute& rt) {
  const bool on_sm = rt.kernel == CONV_SMALLMAP;
  if (!(c.m->head_fuse && !a.dst_pool && ((a.coutp == 64 && a.bn == 64) || ((a.coutp == 16 || a.coutp == 32) && a.bn == 32)) && c.m->use_dma)) return;
  const int j = find_head_reader(c, d.dst);
  if (j < 0) return;
  const ph_op_desc& hx = c.m->ops[j].d;
  ConvArgs no4 = a;  // (a fused head beats F(4x4,3x3) + a head launch on the 64-channel layers both could take: ask what runs without that kernel; head_w then keeps it off)
  no4.use_wino4 = 0;
  const bool on_w2d = a.coutp == 64 && hx.cout <= 32 && pad16(hx.cin0) == 64 && conv3x3_family_route(no4, c.n_cu).head_w2d;
  const bool on_w16 = a.coutp <= 32 && hx.cout <= 16 && pad16(hx.cin0) == a.coutp && conv3x3_family_route(a, c.n_cu).head_w16;  // (conv3x3_w16_kernel<.., HEAD>)
  const bool sm_head = rt.head_sm && pad16(hx.cin0) == a.coutp;  // (conv3x3_sm_kernel: the workgroup holds every channel of its pixels)
  if (head_can_ride(c, hx) && (sm_head || (!on_sm && (on_w2d || on_w16)))) attach_head(c, a, j, a.coutp, d.dst);
}

// 3x3 conv in exact fp32: the LDS-DMA kernel family, the small-map kernel or the 9-tap row GEMM.  `up`: index of a bilinear op in front that was left to this conv, or -1
int fwd_conv3x3_f32(ForwardCtx& c, const PackedOp& op, int up) {
  const ph_model* m = c.m;
  const Plan& plan = c.plan;
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  ConvArgs a{};
  a.src0 = c.rd(d.src0);
  a.c0p = s0.cp;
  a.src1 = d.src1 >= 0 ? c.rd(d.src1) : nullptr;
  a.c1p = d.src1 >= 0 ? c.slot(d.src1).cp : 0;
  PH_REQUIRE(s0.c == d.cin0 && (d.src1 < 0 || c.slot(d.src1).c == d.cin1), "conv channel mismatch");
  a.wpack = op.w_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.coutp = pad16(d.cout);
  a.B = c.batch;
  a.H = s0.h;
  a.W = s0.w;
  a.relu = c.relu(d);
  a.bn = op.bn;
  a.clock_probe = c.probe_block();
  a.dst_pool = d.dst2 >= 0 ? c.wr(d.dst2) : nullptr;
  a.skip_dst = c.pool_dst_unread(d) ? 1 : 0;
  a.wpack_dma = op.w_dma_dev;
  a.wpack_wino = op.w_wino_dev;
  a.wpack_wino2 = op.w_wino2_dev;
  a.wpack_w16 = op.w_w16_dev;
  a.w16 = op.w16_dev;
  a.zeros = m->zeros_dev;
  apply_conv_options(m, a);
  apply_conv_plan_options(m, plan.reuse ? CONV_PLAN_INFERENCE : CONV_PLAN_TRAIN_FWD, a);
  a.wpack_sm = op.w_sm_dev;
  a.wpack_wino4 = op.w_wino4_dev;
  // (the two round-4 routings below -- Cout-32 layers on the N-tile-64 kernels, split K -- apply to inference plans only: a training program's forward keeps the kernels its
  // gradient tests were pinned with.  The wave-private kernel's two-source (16 + 32 -> 16) and fused-head forms are NOT gated that way: they are shapes of conv_w16 itself and
  // run in every plan; tests/test_gpu_training.py's default network (filters 8, output stride 2: concat 16 + 32 -> 16) trains through the two-source form, its gradients are
  // compared with autograd's)
  if (op.w_n64_dev && op.w_wino2_dev && op.w_wino_dev && (m->conv_n32_wino2d >= 2 || (m->conv_n32_wino2d == 1 && plan.reuse)) && conv3x3_n64_swap_ok(a)) {
    // Cout 32, K >= 64 (and not a shape of the wave-private kernel): N tile 64 with its upper half empty -- the F(2x2,3x3) kernel skips the missing half's MFMAs
    a.bn = 64;
    a.wpack = op.w_n64_dev;
    a.bias = op.b_n64_dev;
    a.wpack_dma = nullptr;
  }
  if (plan.tmp_bytes > 0) {
    a.split_scratch = c.scratch();
    a.split_scratch_bytes = plan.tmp_bytes;
  }
  if (up >= 0) {
    int rc = resolve_deferred_up_f32(c, d, up, a);
    if (rc != PH_OK) return rc;
  }
  // Each answer below changes the arguments the next question is asked with.  The small-map kernel is decided here, once: the head and pool fusions do not move a layer on or off it
  const ConvRoute rt = conv3x3_route(a, c.n_cu);
  const bool on_sm = rt.kernel == CONV_SMALLMAP;
  if (!on_sm && conv3x3_prefers_rowgemm(c, op, a)) return launch_conv_rowgemm(c, op, a.src0, a.c0p, a.src1, a.c1p, a.dst, a.coutp, 2);
  try_head_f32(c, d, a, rt);
  if (!a.head_w && (a.bn == 64 || m->dma32) && fuses_pool(m, c.op_i())) {
    // An UNFUSED program (the training forward: the backward walks one op per activation) still gets the conv kernels' fused
    // 2x2 max pool: when the next op is the pool of this conv's output, the epilogue writes both tensors and the pool op is skipped.
    const ph_op_desc& nx = c.next_op()->d;
    a.dst_pool = c.wr(nx.dst);
    if (conv3x3_family_route(a, c.n_cu).pools) {  // the F(2x2,3x3) kernels (a Winograd tile is a pool window); other kernels keep the separate pool
      c.pooled_by_conv = d.dst;
    } else {
      a.dst_pool = nullptr;
      c.unnote(1, nx.dst);
    }
  }
  if (a.split_scratch) c.note_tmp(1);  // (partial-sum planes of a split-K launch)
  if (on_sm) return launch_routed(c, a, rt);
  ConvArgs q = a;  // (the small-map kernel declined the layer above)
  q.use_sm = 0;
  return launch_routed(c, a, conv3x3_route(q, c.n_cu));
}

int fwd_conv(ForwardCtx& c, const PackedOp& op) {
  if (c.conv_done[c.op_i()]) {  // computed by the conv in front of it (fwd_conv_block2)
    c.ran(PH_KV_FUSED);
    return PH_OK;
  }
  const int up = c.deferred_up;  // (fwd_upsample defers only to a 3x3 conv)
  c.deferred_up = -1;
  PH_REQUIRE(up < 0 || op.d.ksize == 3, "a deferred bilinear op in front of a %dx%d conv", op.d.ksize, op.d.ksize);
  if (c.fmt != FMT_F32) return fwd_conv_f16(c, op, up);
  if (op.d.ksize != 3) return fwd_conv_kxk(c, op);
  return fwd_conv3x3_f32(c, op, up);
}

// ---- pool, up-sampling, transposed conv

int fwd_pool(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (c.pooled_by_conv == d.src0) {  // written by the producing conv's epilogue
    c.pooled_by_conv = -1;
    return PH_OK;
  }
  const SlotShape& s0 = c.slot(d.src0);
  float* const src = c.rd(d.src0);
  float* const dst = c.wr(d.dst);
  return c.fmt == FMT_F32 ? launch_pool(src, dst, c.batch, s0.h, s0.w, s0.cp, c.s) : launch_pool_fmt(c.fmt, src, dst, c.batch, s0.h, s0.w, s0.cp, c.s);
}

int fwd_upsample(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  if (defers_upsample_f32(c.m, c.op_i(), c.plan) || defers_upsample_f16(c.m, c.op_i(), c.plan)) {  // inference plans: the conv behind it decides (fwd_conv3x3_f32 / fwd_conv_f16)
    c.deferred_up = c.op_i();
    return PH_OK;
  }
  float* const src = c.rd(d.src0);
  float* const dst = c.wr(d.dst);
  return c.fmt == FMT_F32 ? launch_upsample(src, dst, c.batch, s0.h, s0.w, s0.cp, c.s)
                          : launch_upsample_fmt(c.fmt, src, dst, c.batch, s0.h, s0.w, s0.cp, c.s, (c.fmt == FMT_F16 && c.m->upsample_f16math) ? 1 : 0);
}

// ConvTranspose2d as four output-phase GEMMs: 9 taps per INPUT pixel, no zero-stuffed tensor (exact fp32)
int fwd_convt_phase(ForwardCtx& c, const PackedOp& op) {
  const ph_model* m = c.m;
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  int rc = PH_OK;
  for (int ph = 0; ph < (m->convt_one_launch ? 1 : 4) && rc == PH_OK; ++ph) {  // one launch for the four phases (grid.y), or four launches
    GemmArgs g{};
    if (ph) c.next_launch();
    g.src0 = c.rd(d.src0);
    g.c0p = s0.cp;
    g.wpack = op.wt_phase_dev[ph];
    g.bias = op.bt_dev;
    g.dst = c.wr(d.dst);
    g.zeros = m->zeros_dev;
    g.coutp = so.cp;
    g.bn = op.bn_t;
    g.M = c.batch * s0.h * s0.w;
    g.mode = 3;
    g.ntaps = (1 + (ph >> 1)) * (1 + (ph & 1));
    g.H = s0.h;
    g.W = s0.w;
    g.out_patch = 1;
    g.out_tap = ph;
    if (m->convt_one_launch) {
      g.all_phases = 1;
      for (int q = 0; q < 4; ++q) g.wpack_ph[q] = op.wt_phase_dev[q];
    }
    g.out_H = 2 * s0.h;
    g.out_W = 2 * s0.w;
    g.act = (d.flags & PH_FLAG_SILU) ? 4 : c.relu(d);
    g.scale = op.wt_scale_dev;
    g.shift = op.wt_shift_dev;
    g.affine_first = op.wt_scale_dev ? 1 : 0;
    g.late_split = m->gemm_late_split;
    rc = launch_gemm(g, c.s);
  }
  c.ran(PH_KV_ROWGEMM);
  return rc;
}

// ConvTranspose2d as zero-stuffing + a 3x3 conv (4x the FLOPs): the fp16 formats, and the A/B form of exact fp32 (convt_phase 0)
int fwd_convt_stuffed(ForwardCtx& c, const PackedOp& op) {
  const ph_model* m = c.m;
  const ph_op_desc& d = op.d;
  const int fmt = c.fmt, rs_div = c.rs_div;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(!op.wt_scale_dev && !(d.flags & PH_FLAG_SILU), "folded BatchNorm / SiLU on a transposed conv need the phase GEMMs (exact precision, convt_phase = 1)");
  float* tmp = c.scratch();
  c.note_tmp(1);
  int rc = launch_zero_stuff(c.rd(d.src0), tmp, c.batch, s0.h, s0.w, s0.cp / rs_div, c.s);  // 16-B quads: format-agnostic
  if (rc != PH_OK) return rc;
  c.next_launch();
  c.note_tmp(0);  // (the conv below reads the zero-stuffed tensor)
  if (fmt != FMT_F32) {
    const SlotShape& so = c.slot(d.dst);
    ConvF16Args f{};
    f.src0 = tmp;
    f.dst = c.wr(d.dst);
    conv_f16_common(c, op, s0.cp, 2 * s0.h, 2 * s0.w, f);
    if (m->head_fuse && fmt == FMT_F16 && op.bn == 64 && so.cp == 64) {
      // plain fp16: a 1x1 head that reads this conv's 64-channel output rides in its epilogue, as in fwd_conv_f16 (conv3x3_f16_persist_kernel only: 64 channels; the head's
      // input channels are checked as pad16(..) == 64 here, which is NOT fmt_cpad(FMT_F16, ..) == so.cp for 33 .. 48 channels -- both kept as they were)
      const int j = find_head_reader(c, d.dst);
      if (j >= 0 && head_can_ride(c, m->ops[j].d) && m->ops[j].d.cout <= 32 && pad16(m->ops[j].d.cin0) == 64) attach_head(c, f, j, 64, d.dst);
    }
    c.ran(PH_KV_F16);
    return launch_conv3x3_f16(f, c.s);
  }
  ConvArgs a{};
  a.src0 = tmp;
  a.c0p = s0.cp;
  a.src1 = nullptr;
  a.c1p = 0;
  a.wpack = op.w_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.coutp = pad16(d.cout);
  a.B = c.batch;
  a.H = 2 * s0.h;
  a.W = 2 * s0.w;
  a.relu = c.relu(d);
  a.bn = op.bn;
  a.clock_probe = nullptr;
  a.dst_pool = nullptr;
  a.wpack_dma = op.w_dma_dev;
  a.zeros = m->zeros_dev;
  apply_conv_options(m, a);
  return launch_routed(c, a, conv3x3_route(a, c.n_cu));
}

int fwd_convt(ForwardCtx& c, const PackedOp& op) {
  PH_REQUIRE(c.slot(op.d.src0).c == op.d.cin0, "convT channel mismatch");
  if (c.fmt == FMT_F32 && c.m->convt_phase && op.wt_phase_dev[0]) return fwd_convt_phase(c, op);
  return fwd_convt_stuffed(c, op);
}

// ---- ConvNeXt / Swin encoder ops

int fwd_dwconv(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0, "depthwise conv channel mismatch");
  if (c.fmt == FMT_F16) {
    DwConvF16Args f{};
    f.src = c.rd(d.src0);
    f.w = op.w_dev;
    f.bias = op.b_dev;
    f.dst = c.wr(d.dst);
    f.wcp = pad16(d.cout);
    f.cp = s0.cp;
    f.B = c.batch;
    f.H = s0.h;
    f.W = s0.w;
    if (f.cp <= 1024 && fuses_layernorm(c.m, c.op_i(), c.plan.reuse)) ride_layernorm(c, d, f);  // as below: the LayerNorm rides in the depthwise kernel
    c.ran(PH_KV_CNX_F16_DW);
    return launch_dwconv7_f16(f, c.s);
  }
  DwConvArgs a{};
  a.src = c.rd(d.src0);
  a.w = op.w_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.cp = s0.cp;
  a.B = c.batch;
  a.H = s0.h;
  a.W = s0.w;
  // CNBlock: the LayerNorm that follows rides in the depthwise kernel (inference plans: nothing else reads the depthwise output)
  if (c.fmt == FMT_F32 && fuses_layernorm(c.m, c.op_i(), c.plan.reuse)) ride_layernorm(c, d, a);
  return launch_dwconv7(a, c.s);
}

int fwd_layernorm(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (c.fused_ln == c.op_i()) {  // applied by the patch stem / depthwise conv before it
    c.fused_ln = -1;
    if (c.fmt == FMT_F16) c.ran(PH_KV_FUSED);
    return PH_OK;
  }
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0, "LayerNorm channel mismatch");
  const float eps = (d.flags & PH_FLAG_LN_EPS_1EM5) ? 1e-5f : 1e-6f;
  if (d.flags & PH_FLAG_RESIDUAL) {  // dst = src1 + LayerNorm(src0): Swinv2's layernorm_before / layernorm_after
    const SlotShape& s1 = c.slot(d.src1);
    PH_REQUIRE(c.fmt == FMT_F32 && s1.cp == s0.cp && c.slot(d.dst).cp == s0.cp && d.src1 != d.dst && d.src0 != d.dst, "the residual LayerNorm runs in exact fp32 on distinct slots of one shape");
    const float* x = c.rd(d.src0);
    const float* res = c.rd(d.src1);
    c.ran(PH_KV_LAYERNORM_ADD);
    return launch_layernorm_add(x, res, op.w_dev, op.b_dev, c.wr(d.dst), s0.c, s0.cp, (size_t)c.batch * s0.h * s0.w, c.s, eps);
  }
  if (c.fmt == FMT_F16) {
    c.ran(PH_KV_CNX_F16_LN);
    return launch_layernorm_f16(c.rd(d.src0), op.w_dev, op.b_dev, c.wr(d.dst), s0.c, pad16(s0.c), s0.cp, (size_t)c.batch * s0.h * s0.w, c.s, eps);
  }
  return launch_layernorm(c.rd(d.src0), op.w_dev, op.b_dev, c.wr(d.dst), s0.c, s0.cp, (size_t)c.batch * s0.h * s0.w, c.s, eps);
}

int fwd_patch_merge(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE((c.fmt == FMT_F32 || c.fmt == FMT_F16) && s0.c == d.cin0 && s0.cp == d.cin0 && so.cp == d.cout, "patch merge channel mismatch");
  if (d.flags & PH_FLAG_NO_NORM) {  // Swinv2: the gather alone (its norm sits behind the reduction)
    PH_REQUIRE(c.fmt == FMT_F32, "the patch-merge gather without a norm runs in exact fp32 only");
    const float* x = c.rd(d.src0);
    c.ran(PH_KV_PATCH_MERGE_GATHER);
    return launch_patch_merge_gather(x, c.wr(d.dst), c.batch, s0.h, s0.w, d.cin0, c.s);
  }
  const float eps = (d.flags & PH_FLAG_LN_EPS_1EM5) ? 1e-5f : 1e-6f;
  if (c.fmt == FMT_F16) {
    c.ran(PH_KV_SWIN_F16_MERGE_LN);
    return launch_patch_merge_ln_f16(c.rd(d.src0), op.w_dev, op.b_dev, c.wr(d.dst), c.batch, s0.h, s0.w, d.cin0, eps, c.s);
  }
  return launch_patch_merge_ln(c.rd(d.src0), op.w_dev, op.b_dev, c.wr(d.dst), c.batch, s0.h, s0.w, d.cin0, eps, c.s);
}

// what the plain and the cosine op fill alike; the shift is the caller's
WindowAttnArgs window_attn_args(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  WindowAttnArgs a{};
  a.qkv = c.rd(d.src0);
  a.table = op.w_dev;
  a.qkv_bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.B = c.batch;
  a.H = s0.h;
  a.W = s0.w;
  a.C = d.cout;
  a.heads = d.cin1;
  a.w = d.ksize;
  return a;
}

int fwd_window_attn(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE((c.fmt == FMT_F32 || c.fmt == FMT_F16) && s0.c == d.cin0 && s0.cp == d.cin0 && c.slot(d.dst).cp == d.cout, "window attention channel mismatch");
  WindowAttnArgs a = window_attn_args(c, op);
  a.sh = window_axis_shift(s0.h, d.ksize, d.cmid);
  a.sw = window_axis_shift(s0.w, d.ksize, d.cmid);
  if (c.fmt == FMT_F16) {
    c.ran(PH_KV_WINDOW_ATTN_F16);
    return launch_window_attn_f16(a, c.s);
  }
  c.ran(PH_KV_WINDOW_ATTN);
  return launch_window_attn(a, c.s);
}

// cosine window attention of a Swinv2 block (swin_kernels.hip, swinv2_kernels.hip): the table, the padded token's q | 0 | v and the head scales are the host's derived tensors
int fwd_window_attn_v2(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(c.fmt == FMT_F32 && s0.c == d.cin0 && s0.cp == d.cin0 && c.slot(d.dst).cp == d.cout, "cosine window attention channel mismatch");
  WindowAttnArgs a = window_attn_args(c, op);
  a.scale = op.w2_dev;
  a.sh = a.sw = d.cmid;  // the layer's shift on both axes, whatever the map
  if (d.ksize > 8) {  // more than 64 tokens per window: the key-tiled kernel
    c.ran(PH_KV_WINDOW_ATTN_V2_WIDE);
    return launch_window_attn_v2_wide(a, c.s);
  }
  c.ran(PH_KV_WINDOW_ATTN_V2);
  return launch_window_attn_v2(a, c.s);
}

// ---- Linear / 2x2-stride-2 conv (row GEMMs)

int fwd_linear_f16(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(op.w_cnx_f16_dev && !(d.flags & ~(PH_FLAG_GELU | PH_FLAG_SCALE_RESIDUAL | PH_FLAG_RESIDUAL)), "op has no fp16 row-GEMM form");
  GemmF16Args f{};
  f.src = c.rd(d.src0);
  f.wimg = op.w_cnx_f16_dev;
  f.bias = (d.kind == PH_OP_LINEAR && d.bias == -1) ? nullptr : op.b_dev;  // Linear(bias=False): the patch-merging reduction
  f.dst = c.wr(d.dst);
  f.cinp = s0.cp;
  f.coutp = so.cp;
  f.M = c.batch * so.h * so.w;
  f.taps = d.kind == PH_OP_PATCH_CONV ? 4 : 1;
  f.H = s0.h;
  f.W = s0.w;
  f.gelu = (d.flags & PH_FLAG_GELU) ? 1 : 0;
  if (d.flags & PH_FLAG_SCALE_RESIDUAL) f.scale = op.w2_dev;
  if (d.flags & (PH_FLAG_SCALE_RESIDUAL | PH_FLAG_RESIDUAL)) f.residual = c.rd(d.src1);  // (no layer scale: dst = acc + bias + src1)
  c.ran(PH_KV_CNX_F16_GEMM);
  return launch_gemm_f16(f, c.s);
}

// fuses_mlp holds for this Linear and the next: do the plan's widths and ranges let cnblock_mlp_kernel take the pair?
// build_plan releases x (d.src0) before it places y (nx.dst): y may come to lie on x's range, or across it where free blocks have coalesced.  cnblock_mlp_kernel is
// safe for y EXACTLY on x (or on the residual) -- a row tile reads all of its x rows at its start and its residual elements in the epilogue, each before the store of
// the same elements, and no other tile reads those rows -- and for nothing else: y shifted against x would overwrite rows another tile has yet to read.  Then: two GEMMs.
bool mlp_pair_fits(const ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const ph_op_desc& nx = c.next_op()->d;
  bool pair = c.slot(d.src0).cp == d.cin0 && c.slot(nx.dst).cp == nx.cout && c.slot(nx.src1).cp == nx.cout;
  for (int src : {d.src0, nx.src1}) {
    const int64_t ys = c.slot(nx.dst).offset, ye = ys + c.slot_bytes(nx.dst), xs = c.slot(src).offset, xe = xs + c.slot_bytes(src);
    if (ys < xe && xs < ye && !(ys == xs && ye == xe)) pair = false;
  }
  return pair;
}

// CNBlock's MLP in one launch: this Linear + GELU and the Linear + layer scale + residual behind it (cnblock_mlp_kernel)
int fwd_linear_mlp(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const PackedOp& nxo = *c.next_op();
  const ph_op_desc& nx = nxo.d;
  const SlotShape& so = c.slot(d.dst);
  MlpArgs f{};
  f.x = c.rd(d.src0);
  f.w1img = op.w_mlp_dev;
  f.w2img = nxo.w_mlp_dev;
  f.b1 = op.b_dev;
  f.b2 = nxo.b_dev;
  f.scale = nxo.w2_dev;
  f.residual = c.rd(nx.src1);
  f.dst = c.wr(nx.dst);
  f.M = c.batch * so.h * so.w;
  f.C = d.cin0;
  c.ran(PH_KV_MLP);
  c.skip_next_linear = true;
  return launch_cnblock_mlp(f, c.s);
}

// fused GRN plan, the residual Linear: (W2 diag(s_b)) x + (W2 grn.bias + b2) + residual, one GEMM per sample on its own scaled weight image
int fwd_linear_grn(ForwardCtx& c, const PackedOp& op) {
  const ph_model* m = c.m;
  const Plan& plan = c.plan;
  const ph_op_desc& d = op.d;
  const int batch = c.batch;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  c.fused_grn = -1;
  const ph_op_desc& g = m->ops[c.op_index - 2].d;
  const SlotShape& sx = c.slot(g.src0);  // the GELU output: what the GEMM reads instead of the GRN slot
  const int hw = sx.h * sx.w;
  const int64_t wfl = gemm_pack_floats(so.cp, sx.cp, op.bn);
  PH_REQUIRE(op.b_grn_dev && sx.cp == s0.cp && plan.tmp_bytes >= (int64_t)batch * wfl * (int64_t)sizeof(float), "fused GRN: scaled-weight scratch is missing from the plan");
  float* wsc = c.scratch();
  const float* scale = c.rd(d.src0);  // launch 0: the scales grn_finalize_kernel left in the GRN slot -> the per-sample weight images in the scratch region
  c.note_tmp(1);
  int rc = launch_grn_scale_weights(op.w_dma_dev, scale, wsc, batch, so.cp, sx.cp, op.bn, c.s);
  c.next_launch();
  const float* x = c.rd(g.src0);      // launch 1 (one GEMM per sample, recorded once): GELU output, weight images, residual -> dst
  c.note_tmp(0);
  const float* res = c.rd(d.src1);
  float* y = c.wr(d.dst);
  c.ran(PH_KV_ROWGEMM);
  for (int b = 0; b < batch && rc == PH_OK; ++b) {
    GemmArgs f{};
    f.src0 = x + (size_t)b * hw * sx.cp;
    f.wpack = wsc + (size_t)b * wfl;
    f.bias = op.b_grn_dev;
    f.residual = res + (size_t)b * hw * so.cp;
    f.dst = y + (size_t)b * hw * so.cp;
    f.zeros = m->zeros_dev;
    f.c0p = sx.cp;
    f.coutp = so.cp;
    f.bn = op.bn;
    f.M = hw;
    f.mode = 0;
    f.H = s0.h;
    f.W = s0.w;
    f.late_split = m->gemm_late_split;
    rc = launch_gemm(f, c.s);
  }
  return rc;
}

// the fp32 row GEMM, with its epilogue fusions: the GELU or the scale-add op behind it (unfused programs), the fused GRN plan's sums of squares
int fwd_linear_f32(ForwardCtx& c, const PackedOp& op) {
  const ph_model* m = c.m;
  const Plan& plan = c.plan;
  const ph_op_desc& d = op.d;
  const int batch = c.batch;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  GemmArgs a{};
  a.src0 = c.rd(d.src0);
  a.wpack = op.w_dma_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.zeros = m->zeros_dev;
  a.c0p = s0.cp;
  a.coutp = so.cp;
  a.bn = op.bn;
  a.M = batch * so.h * so.w;
  a.mode = d.kind == PH_OP_PATCH_CONV ? 1 : 0;
  a.H = s0.h;
  a.W = s0.w;
  a.act = (d.flags & PH_FLAG_GELU) ? 2 : c.relu(d);
  if (d.flags & PH_FLAG_SCALE_RESIDUAL) {
    a.scale = op.w2_dev;
    a.residual = c.rd(d.src1);
  } else if (d.flags & PH_FLAG_RESIDUAL) {  // dst = acc + bias + src1
    if (m->branch_scales) {  // dst = s[branch][b] * (acc + bias) + src1: the GEMM without its residual, then one element-wise pass
      c.ran(PH_KV_ROWGEMM);
      a.late_split = m->gemm_late_split;
      int rc = launch_gemm(a, c.s);
      c.next_launch();
      if (rc == PH_OK)
        rc = launch_scale_samples_add(static_cast<float*>(c.wr(d.dst)), static_cast<const float*>(c.rd(d.src1)), m->branch_scales + (size_t)c.branch * batch, (size_t)so.h * so.w * so.cp, batch, c.s);
      ++c.branch;
      return rc;
    }
    a.residual = c.rd(d.src1);
  }
  if (fuses_grn(m, c.op_i(), c.fmt)) {  // fused GRN plan: the epilogue also leaves the per-(32-row block, sample) sums of squares of its output in the scratch region
    const int hw = so.h * so.w;
    PH_REQUIRE(plan.tmp_bytes >= grn_fused_partial_floats(a.M, hw, so.cp) * (int64_t)sizeof(float), "fused GRN scratch is missing from the plan");
    a.sumsq = c.scratch();
    a.sq_hw = hw;
    a.sq_nseg = grn_fused_nseg(hw);
    c.note_tmp(1);
    c.fused_grn = (int)c.op_index;
  }
  a.late_split = m->gemm_late_split;
  const PackedOp* nxo = c.next_op();
  // training program (Linear and GELU as separate ops, the pre-activation is kept for the backward pass): the
  // GEMM epilogue writes both the pre-activation and GELU(pre-activation), the GELU op after it becomes a no-op
  if (m->fuse_gelu_fwd && a.mode == 0 && a.act == 0 && !a.residual && nxo) {
    const ph_op_desc& nx = nxo->d;
    if (nx.kind == PH_OP_GELU && nx.src0 == d.dst && nx.dst != d.dst) {
      a.act = 2;
      a.dst_pre = a.dst;
      a.dst = c.wr(nx.dst);
      c.skip_next_gelu = true;
    }
  }
  // ... and (CNBlock's second Linear -> layer scale + residual, separate ops in a training program because the backward needs the un-scaled
  // output): the epilogue writes the un-scaled output AND scale * output + residual, the scale-add op after it becomes a no-op
  if (m->fuse_gelu_fwd && a.mode == 0 && a.act == 0 && !a.residual && !a.dst_pre && nxo && so.cp % a.bn == 0) {
    const ph_op_desc& nx = nxo->d;
    if (nx.kind == PH_OP_SCALE_ADD && nx.src0 == d.dst && nx.dst != d.dst && nx.src1 != d.dst && nx.src1 >= 0 && nx.cin0 == d.cout) {
      a.scale = nxo->w_dev;
      a.residual = c.rd(nx.src1);
      a.dst_pre = a.dst;
      a.dst = c.wr(nx.dst);
      c.skip_next_scale_add = true;
    }
  }
  c.ran(PH_KV_ROWGEMM);
  return launch_gemm(a, c.s);
}

int launch_tap1_gemm(ForwardCtx& c, const PackedOp& op, int stride, const float* residual);  // (with the ResNet ops below)

int fwd_linear(ForwardCtx& c, const PackedOp& op) {  // PH_OP_LINEAR and PH_OP_PATCH_CONV
  if (c.skip_next_linear) {  // the second Linear of a CNBlock MLP that cnblock_mlp_kernel computed with the first
    c.skip_next_linear = false;
    c.ran(PH_KV_MLP);
    return PH_OK;
  }
  PH_REQUIRE(c.slot(op.d.src0).c == op.d.cin0, "GEMM channel mismatch");
  if (op.d.kind == PH_OP_LINEAR && (op.d.flags & PH_FLAG_RESIDUAL) && (op.d.flags & PH_FLAG_RELU)) {  // dst = relu(acc + bias + src1): a ResNet bottleneck's tail
    PH_REQUIRE(c.fmt == FMT_F32 && !c.m->branch_scales && c.slot(op.d.src1).cp == c.slot(op.d.dst).cp, "the residual + ReLU epilogue runs in exact fp32 without branch scales");
    c.ran(PH_KV_ROWGEMM);
    return launch_tap1_gemm(c, op, 1, c.rd(op.d.src1));
  }
  if (c.fmt == FMT_F16) return fwd_linear_f16(c, op);
  if (fuses_mlp(c.m, c.op_i(), c.fmt, c.plan.reuse) && mlp_pair_fits(c, op)) return fwd_linear_mlp(c, op);
  if (c.fused_grn == c.op_i() && op.d.kind == PH_OP_LINEAR) return fwd_linear_grn(c, op);
  return fwd_linear_f32(c, op);
}

// ---- ResNet encoder ops (resnet_kernels.hip, the strided row-GEMM modes)

int fwd_resnet_stem(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  PH_REQUIRE(d.cin0 == c.in_channels, "input has %d channels, network expects %d", c.in_channels, d.cin0);
  PH_REQUIRE(c.fmt == FMT_F32, "the resnet stem runs in exact fp32 only");
  const SlotShape& sf = c.slot(d.dst);
  const SlotShape& sp = c.slot(d.dst2);
  ResnetStemArgs a{};
  a.src = c.input_dev;
  a.wimg = op.w_dev;
  a.bias = op.b_dev;
  a.conv_dst = c.wr(d.dst);  // launch 0: image -> the stride-2 map
  a.dtype = c.in_dtype;
  a.cin = d.cin0;
  a.coutp = sf.cp;
  a.B = c.batch;
  a.H = c.height;
  a.W = c.width;
  a.OH = sf.h;
  a.OW = sf.w;
  a.PH = sp.h;
  a.PW = sp.w;
  for (int ch = 0; ch < 4; ++ch) {
    a.mean[ch] = c.m->in_mean[ch];
    a.std[ch] = c.m->in_std[ch];
  }
  c.ran(PH_KV_RESNET_STEM);
  int rc = launch_resnet_stem(a, c.s);
  if (rc != PH_OK) return rc;
  c.next_launch();
  const float* full = c.rd(d.dst);  // launch 1: the stride-2 map -> the pooled map
  return launch_maxpool3s2(full, c.wr(d.dst2), c.batch, sf.h, sf.w, sf.cp, c.s);
}

// one-tap row GEMM (mode 6): a 1x1 conv at stride 1 or 2, bias (+ residual) (+ ReLU) with the residual in front of the activation
int launch_tap1_gemm(ForwardCtx& c, const PackedOp& op, int stride, const float* residual) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  GemmArgs g{};
  g.src0 = c.rd(d.src0);
  g.c0p = s0.cp;
  g.wpack = op.w_dma_dev;
  g.bias = op.b_dev;
  g.residual = residual;
  g.dst = c.wr(d.dst);
  g.zeros = c.m->zeros_dev;
  g.coutp = so.cp;
  g.bn = op.bn;
  g.M = c.batch * so.h * so.w;
  g.mode = 6;
  g.tap_stride = stride;
  g.H = s0.h;
  g.W = s0.w;
  g.act = c.relu(d);
  g.late_split = c.m->gemm_late_split;
  return launch_gemm(g, c.s);
}

int fwd_conv_s2(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  const SlotShape& so = c.slot(d.dst);
  PH_REQUIRE(c.fmt == FMT_F32 && s0.c == d.cin0, "stride-2 conv channel mismatch");
  c.ran(PH_KV_CONV_S2);
  if (d.ksize == 1) return launch_tap1_gemm(c, op, 2, nullptr);
  GemmArgs g{};  // 3x3 stride 2 pad 1: nine taps gathered from the 2H x 2W map (the mode the transposed conv's data gradient runs on)
  g.src0 = c.rd(d.src0);
  g.c0p = s0.cp;
  g.wpack = op.w_dma_dev;
  g.bias = op.b_dev;
  g.dst = c.wr(d.dst);
  g.zeros = c.m->zeros_dev;
  g.coutp = so.cp;
  g.bn = op.bn;
  g.M = c.batch * so.h * so.w;
  g.mode = 4;
  g.H = s0.h;
  g.W = s0.w;
  g.act = c.relu(d);
  g.late_split = c.m->gemm_late_split;
  return launch_gemm(g, c.s);
}

int fwd_add_relu(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(c.fmt == FMT_F32 && s0.c == d.cin0 && c.slot(d.src1).cp == s0.cp && c.slot(d.dst).cp == s0.cp, "add channel mismatch");
  const float* x = c.rd(d.src0);
  const float* y = c.rd(d.src1);
  c.ran(PH_KV_ADD_RELU);
  return launch_add_relu(x, y, c.wr(d.dst), (size_t)c.batch * s0.h * s0.w * s0.cp, c.s);
}

// ---- GRN, element-wise ops, heads

int fwd_grn(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(c.fmt == FMT_F32 && s0.c == d.cin0 && s0.cp == pad16(d.cout) && c.slot(d.dst).cp == s0.cp, "GRN channel mismatch");
  PH_REQUIRE(c.plan.tmp_bytes >= grn_scratch_floats(c.batch, s0.h * s0.w, s0.cp) * (int64_t)sizeof(float), "GRN scratch is missing from the plan");
  if (c.fused_grn == c.op_i()) {  // fused GRN plan: the block sums the Linear in front left in the scratch region -> scale[b][c] = 1 + weight[c] N[b,c], kept in this op's own slot
    c.fused_grn = (int)c.op_index;
    c.note_tmp(0);
    c.ran(PH_KV_GRN_FUSED);
    return launch_grn_finalize(c.scratch(), op.w_dev, c.wr(d.dst), c.batch, s0.h * s0.w, d.cout, s0.cp, c.s);
  }
  GrnArgs a{};
  a.src = c.rd(d.src0);  // launch 0, the reduction: the slot -> the slice sums in the scratch region
  c.note_tmp(1);
  c.next_launch();
  c.rd(d.src0);          // launch 1, the apply pass: the slot and the slice sums -> dst
  c.note_tmp(0);
  a.weight = op.w_dev;
  a.bias = op.b_dev;
  a.dst = c.wr(d.dst);
  a.partial = c.scratch();
  a.B = c.batch;
  a.HW = s0.h * s0.w;
  a.c = d.cout;
  a.cp = s0.cp;
  c.ran(PH_KV_GRN);
  return launch_grn(a, c.s);
}

int fwd_global_maxpool(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0, "global pool channel mismatch");
  return launch_global_maxpool(c.rd(d.src0), c.wr(d.dst), c.batch, s0.h * s0.w, s0.cp, c.s);
}

int fwd_gelu(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (c.skip_next_gelu) {  // already produced by the preceding Linear's epilogue
    c.skip_next_gelu = false;
    return PH_OK;
  }
  const SlotShape& s0 = c.slot(d.src0);
  if (c.fmt == FMT_F16) {
    c.ran(PH_KV_CNX_F16_ELTWISE);
    return launch_gelu_fmt(c.fmt, c.rd(d.src0), c.wr(d.dst), (size_t)c.batch * s0.h * s0.w, s0.cp, c.s);
  }
  return launch_gelu_fwd(c.rd(d.src0), c.wr(d.dst), (size_t)c.batch * s0.h * s0.w * s0.cp, c.s);
}

int fwd_scale_add(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (c.skip_next_scale_add) {  // already produced by the preceding Linear's epilogue
    c.skip_next_scale_add = false;
    return PH_OK;
  }
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0, "scale-add channel mismatch");
  if (c.fmt == FMT_F16) {
    c.ran(PH_KV_CNX_F16_ELTWISE);
    return launch_scale_add_fmt(c.fmt, c.rd(d.src0), c.rd(d.src1), op.w_dev, c.wr(d.dst), (size_t)c.batch * s0.h * s0.w, pad16(d.cout), s0.cp, c.s);
  }
  return launch_scale_add_fwd(c.rd(d.src0), c.rd(d.src1), op.w_dev, c.wr(d.dst), s0.cp, (size_t)c.batch * s0.h * s0.w * s0.cp, c.s);
}

int fwd_head(ForwardCtx& c, const PackedOp& op) {
  const ph_op_desc& d = op.d;
  if (c.head_done[c.op_i()]) {  // computed by its producer's epilogue
    c.ran(PH_KV_FUSED);
    return PH_OK;
  }
  const SlotShape& s0 = c.slot(d.src0);
  PH_REQUIRE(s0.c == d.cin0, "head channel mismatch");
  PH_REQUIRE(c.out_dev[d.out_index] != nullptr, "output %d is null", d.out_index);
  int rc = launch_head_fmt(c.fmt, c.rd(d.src0), op.w_dev, op.b_dev, c.out_dev[d.out_index], c.batch, s0.h * s0.w, s0.cp, pad16(d.cin0), d.cout, head_sigmoid(c.m, c.plan, d), c.s);
  if (rc == PH_OK && (d.flags & PH_FLAG_SOFTMAX)) {
    PH_REQUIRE(s0.h == 1 && s0.w == 1, "softmax head expects a pooled (1x1) feature");
    rc = launch_softmax_rows(c.out_dev[d.out_index], c.batch, d.cout, c.s);
  }
  return rc;
}

int fwd_op(ForwardCtx& c, const PackedOp& op) {
  switch (op.d.kind) {
    case PH_OP_INPUT_CONV: return fwd_input_conv(c, op);
    case PH_OP_STEM: return fwd_stem(c, op);
    case PH_OP_PATCH_STEM: return fwd_patch_stem(c, op);
    case PH_OP_CONV: return fwd_conv(c, op);
    case PH_OP_POOL: return fwd_pool(c, op);
    case PH_OP_UPSAMPLE: return fwd_upsample(c, op);
    case PH_OP_CONVT: return fwd_convt(c, op);
    case PH_OP_DWCONV: return fwd_dwconv(c, op);
    case PH_OP_LAYERNORM: return fwd_layernorm(c, op);
    case PH_OP_PATCH_MERGE: return fwd_patch_merge(c, op);
    case PH_OP_WINDOW_ATTN: return fwd_window_attn(c, op);
    case PH_OP_WINDOW_ATTN_V2: return fwd_window_attn_v2(c, op);
    case PH_OP_LINEAR:
    case PH_OP_PATCH_CONV: return fwd_linear(c, op);
    case PH_OP_GRN: return fwd_grn(c, op);
    case PH_OP_RESNET_STEM: return fwd_resnet_stem(c, op);
    case PH_OP_CONV_S2: return fwd_conv_s2(c, op);
    case PH_OP_ADD_RELU: return fwd_add_relu(c, op);
    case PH_OP_GLOBAL_MAXPOOL: return fwd_global_maxpool(c, op);
    case PH_OP_GELU: return fwd_gelu(c, op);
    case PH_OP_SCALE_ADD: return fwd_scale_add(c, op);
    case PH_OP_HEAD: return fwd_head(c, op);
    default:
      set_error("unknown op kind %d", op.d.kind);
      return PH_E_INVALID;
  }
}

}  // namespace

extern "C" int ph_model_forward(ph_model* m, const void* input_dev, int32_t in_dtype, int32_t batch, int32_t in_channels, int32_t height, int32_t width, void* workspace_dev,
                                int64_t workspace_bytes, float* const* out_dev, void* stream) {
  PH_REQUIRE(m && input_dev && workspace_dev && out_dev, "ph_model_forward: null argument");
  PH_REQUIRE(in_dtype >= 0 && in_dtype <= 2, "ph_model_forward: bad in_dtype %d", in_dtype);
  PH_REQUIRE(((uintptr_t)workspace_dev & 255) == 0, "workspace must be 256-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  Plan plan;
  const int fmt = forward_format(m);
  PH_REQUIRE(!m->branch_scales || (fmt == FMT_F32 && batch == m->branch_batch),
             "ph_model_forward: branch scales are set for batch %d in exact fp32; this forward has batch %d%s", m->branch_batch, batch, fmt == FMT_F32 ? "" : " and a non-fp32 format");
  int rc = build_plan(m, batch, height, width, plan, fmt);
  if (rc != PH_OK) return rc;
  if (fmt != FMT_F32) {
    rc = ensure_f16_weights(m, fmt == FMT_F16 ? 1 : 0, s);
    if (rc != PH_OK) return rc;
  }
  if (plan.total > workspace_bytes) {
    set_error("workspace too small: need %lld bytes, got %lld", (long long)plan.total, (long long)workspace_bytes);
    return PH_E_WORKSPACE;
  }
  char* ws = static_cast<char*>(workspace_dev);
  m->last_ranges.clear();
  if (m->profiling) {
    rc = drain_events(m);
    if (rc != PH_OK) return rc;
  }
  rc = refresh_stale_weights(m, plan, s);
  if (rc != PH_OK) return rc;
  m->last_variant.assign(m->ops.size(), PH_KV_NONE);
  m->last_rows_plan.assign(4 * m->ops.size(), 0);
  int n_cu = 0;
  rc = device_cu_count(&n_cu);
  if (rc != PH_OK) return rc;
  ForwardCtx c{m, plan, fmt, 4 / plan.bpc, batch, height, width, in_channels, in_dtype, input_dev, ws, out_dev, s, m->last_variant.data(), n_cu, m->last_ranges};
  c.head_done.assign(m->ops.size(), 0);
  c.conv_done.assign(m->ops.size(), 0);
  for (const PackedOp& op : m->ops) {
    if (m->profiling) PH_HIP_CHECK(hipEventRecord(m->ev[c.op_index], s));
    ++c.op_index;
    c.launch_no = 0;
    rc = fwd_op(c, op);
    if (rc != PH_OK) return rc;
  }
  // every note one op left for a later one has been taken (no program the project emits gets here with one pending: a new fusion that forgets its hand-over does)
  const char* pending = c.deferred_up >= 0 ? "deferred_up" : c.fused_ln >= 0 ? "fused_ln" : c.fused_grn >= 0 ? "fused_grn" : c.pooled_by_conv >= 0 ? "pooled_by_conv"
                        : c.skip_next_gelu ? "skip_next_gelu" : c.skip_next_scale_add ? "skip_next_scale_add" : c.skip_next_linear ? "skip_next_linear" : nullptr;
  PH_REQUIRE(!pending, "ph_model_forward: the note '%s' of a run-time fusion was still pending after the last op", pending);
  if (m->profiling) {
    PH_HIP_CHECK(hipEventRecord(m->ev[m->ops.size()], s));
    m->events_pending = true;
  }
  m->last_plan = plan;
  m->last_ws = ws;
  m->last_batch = batch;
  return PH_OK;
}
