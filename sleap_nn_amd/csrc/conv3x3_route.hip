// The route of an exact-fp32 3x3 conv (conv3x3_route.h).  Host code only; every function here is pure.
#include "conv3x3_route.h"

#include "common.h"
#include "posehip.h"

namespace ph {

namespace {

// Winograd weights are in play: use_wino 2 keeps them to the N-tile-64 layers
bool wino_on(const ConvArgs& a) { return a.use_wino && a.wpack_wino && (a.bn == 64 || a.use_wino != 2); }

// The K split the cost models price a kernel at: the shape's split wherever the plan reserved scratch at all (NOT the launch's ksplit, which also looks at the
// scratch size and at accumulate / mask / head)
int modelled_ksplit(const ConvArgs& a, int n_cu, ConvKernel k) {
  if (!a.split_scratch) return 1;
  return k == CONV_WINO4 ? wino4_ksplit_shape(a.B, a.H, a.W, a.c0p + a.c1p, a.coutp, a.splitk, n_cu) : wino2d_ksplit_shape(a.B, a.H, a.W, a.c0p + a.c1p, a.coutp, a.splitk, n_cu);
}

// K slices of the launch: the shape's split where the launch may split at all and its partial-sum planes fit the scratch
int launch_ksplit(const ConvArgs& a, int n_cu, ConvKernel k) {
  if (!a.split_scratch || a.relu_mask_src || (k == CONV_WINO2D && (a.accumulate || a.head_w))) return 1;
  const int ks = modelled_ksplit(a, n_cu, k);
  return (ks > 1 && (int64_t)ks * a.B * a.H * a.W * a.coutp * 4 <= a.split_scratch_bytes) ? ks : 1;
}

// Priority order inside the LDS-DMA family: F(4x4,3x3) where legal and (unless forced) estimated faster than the wave-split F(2x2,3x3) kernel, the wave-private
// kernel, conv3x3_c16, wave-split F(2x2,3x3), then F(2,3) along x or the 9-tap kernel
ConvKernel family_kernel(const ConvArgs& a, int n_cu) {
  const bool wino = wino_on(a);
  if (wino && a.persist && a.use_wino4 && a.c0p + a.c1p >= a.wino4_min_cin && wino4_shape_ok(a) &&
      (a.use_wino4 >= 2 || wino4_cost_us(a, n_cu, modelled_ksplit(a, n_cu, CONV_WINO4)) <= wino2d_cost_us(a, n_cu, modelled_ksplit(a, n_cu, CONV_WINO2D))))
    return CONV_WINO4;
  if (wino && a.persist && a.use_w16 && w16_fits(a)) return CONV_W16;
  if (a.use_c16 && a.w16 && a.c0p == 16 && a.coutp == 16 && !a.src1 && !a.dst_pool) return CONV_C16;
  if (wino && a.persist && a.use_wino2d && a.wpack_wino2 && a.bn == 64 && a.c0p + a.c1p >= 32 && wino2d_fits(a)) return CONV_WINO2D;
  return (a.persist && wino) ? CONV_WINO1D : CONV_DMA9;
}

// The small-map kernel against the family's kernel, both priced in microseconds of launch body; + ~6 us for a bilinear x2 the other kernel cannot fold.
// use_sm = 2 forces it wherever the shape fits (tests, A/B).
bool smallmap_takes(const ConvArgs& a, int n_cu) {
  if (!a.use_sm || !sm_fits(a)) return false;
  if (a.use_sm >= 2) return true;
  ConvArgs hi = a;  // what runs otherwise takes the up-sampled tensor, unless it is the F(4x4,3x3) kernel
  hi.src1_lowres = 0;
  const ConvKernel r = a.src1_lowres && family_kernel(a, n_cu) == CONV_WINO4 ? CONV_WINO4 : family_kernel(hi, n_cu);
  const double extra = (a.src1_lowres && r != CONV_WINO4) ? 6.0 : 0.0;
  double other;
  if (r == CONV_WINO4 || r == CONV_WINO2D) {
    other = r == CONV_WINO4 ? wino4_cost_us(a, n_cu, modelled_ksplit(a, n_cu, r)) : wino2d_cost_us(a, n_cu, modelled_ksplit(a, n_cu, r));
    if ((a.coutp & 63) != 0 && (a.coutp & 63) <= 32) other *= 0.6;  // the half-empty N tile: the waves of the missing half skip their MFMAs (published workload, 96 -> 32 at 160 x 280 x 4: 55 us measured, 94 modelled)
  } else if (r == CONV_W16) {
    other = w16_cost_us(a, n_cu);
  } else {
    return false;  // the 16 -> 16 / F(2,3) / direct kernels keep their layers
  }
  return sm_cost_us(a, n_cu) < other + extra;
}

}  // namespace

// Measured unit times (cfg3 layers, K from 128 to 768 channels): a 32 x 16-pixel tile of the pipelined F(4x4,3x3) kernel costs ~11 us outside its K loop + 1.5 us per quarter
// (4 channels: 3 200 cycles per quarter, 23 000 per tile outside the loop), a 16 x 16-pixel tile of the wave-split F(2x2,3x3) kernel ~8 us + 1.0 us per quarter.  Both kernels
// run one persistent workgroup per CU, so a launch costs rounds of the chip x unit time.
double wino4_cost_us(const ConvArgs& a, int n_cu, int ksplit) {
  const long tiles = (long)((a.H + 15) / 16) * ((a.W + 31) / 32) * a.B * ((a.coutp + 63) / 64);
  const double Qn = (a.c0p + a.c1p) / 4.0;
  return (double)((tiles * ksplit + n_cu - 1) / n_cu) * (11.0 + 1.5 * Qn / ksplit) + (ksplit > 1 ? 8.0 : 0.0);
}
double wino2d_cost_us(const ConvArgs& a, int n_cu, int ksplit) {
  const long tiles = (long)((a.H + 15) / 16) * ((a.W + 15) / 16) * a.B * ((a.coutp + 63) / 64);
  const double Qn = (a.c0p + a.c1p) / 4.0;
  return (double)((tiles * ksplit + n_cu - 1) / n_cu) * (8.0 + 1.0 * Qn / ksplit) + (ksplit > 1 ? 8.0 : 0.0);
}
// the wave-private kernel: 16 x 32-pixel tiles, ~6 us + 3 us per 16 input channels (cfg1's 128 x 128 levels: 32 workgroups, 9 - 15 us)
double w16_cost_us(const ConvArgs& a, int n_cu) {
  const long tiles = (long)((a.H + 31) / 32) * ((a.W + 15) / 16) * a.B;
  return (double)((tiles + n_cu - 1) / n_cu) * (6.0 + 3.0 * (a.c0p + a.c1p) / 16.0);
}

ConvRoute conv3x3_family_route(const ConvArgs& a, int n_cu) {
  ConvRoute r;
  r.kernel = family_kernel(a, n_cu);
  const bool f2x2_or_4 = r.kernel == CONV_W16 || r.kernel == CONV_WINO2D || r.kernel == CONV_WINO4;
  if (r.kernel == CONV_WINO2D || r.kernel == CONV_WINO4) r.ksplit = launch_ksplit(a, n_cu, r.kernel);
  switch (r.kernel) {
    case CONV_C16: r.kv = PH_KV_C16; break;
    case CONV_W16: r.kv = PH_KV_W16; break;
    case CONV_WINO2D: r.kv = r.ksplit > 1 ? PH_KV_WINO2D_KS : PH_KV_WINO2D; break;
    case CONV_WINO4: r.kv = PH_KV_WINO4; break;
    case CONV_WINO1D: r.kv = PH_KV_WINO1D; break;
    default: r.kv = PH_KV_DIRECT; break;
  }
  r.takes_mask = f2x2_or_4 && !a.dst_pool && !a.head_w && !a.skip_dst;  // these kernels store lane-locally; the fused pool / head epilogues are forward-only
  r.pools = r.kernel == CONV_W16 || r.kernel == CONV_WINO2D;
  r.folds_lowres = r.kernel == CONV_WINO4;
  r.head_w2d = r.kernel == CONV_WINO2D && r.ksplit <= 1;
  r.head_w16 = r.kernel == CONV_W16 && w16_takes_head(a);
  return r;
}

ConvRoute conv3x3_route(const ConvArgs& a, int n_cu) {
  ConvRoute r;
  if (smallmap_takes(a, n_cu)) {  // small maps at small batches: (8 x 8 pixels, 16 channels) units, one launch, no split K
    r.kernel = CONV_SMALLMAP;
    r.kv = PH_KV_SMALLMAP;
    r.folds_lowres = true;
    r.head_sm = a.coutp <= 32;  // (the workgroup holds every channel of its pixels)
    return r;
  }
  if (!(a.use_dma && (a.bn == 64 || a.dma32))) {  // the options or the N tile keep the layer off the LDS-DMA family
    r.kernel = CONV_REGSTAGED;
    r.kv = PH_KV_DIRECT;
    return r;
  }
  return conv3x3_family_route(a, n_cu);
}

bool conv3x3_wino2d_sets_rowgemm_fill(const ConvArgs& a) {
  return a.use_dma && a.use_wino && a.use_wino2d && a.persist && a.wpack_wino2 && a.bn == 64 && a.c0p + a.c1p >= 32 && wino2d_fits(a);
}
bool conv3x3_n64_swap_ok(const ConvArgs& a) { return a.use_dma && a.use_wino && a.use_wino2d && a.persist && !w16_fits(a) && wino2d_fits(a); }

}  // namespace ph
