// Which kernel runs an exact-fp32 3x3 "same" conv ("Routing of the exact-fp32 3x3 conv"): the one decision the launcher, the forward and backward
// routines and the plan read.  Pure host arithmetic on the arguments and a CU count: no HIP call, no global state (ph_debug_conv3x3_route runs it without a GPU).
#pragma once
#include "net_kernels.h"

namespace ph {

enum ConvKernel {
  CONV_REGSTAGED,  // launch_conv3x3: the register-staged kernel (options conv_dma = 0, or conv_dma32 = 0 on an N tile of 32)
  CONV_DMA9,       // conv3x3_mfma_dma_*_kernel: 9 taps, LDS-DMA
  CONV_WINO1D,     // conv3x3_wino_persist_kernel: F(2,3) along x
  CONV_C16,        // conv3x3_c16_kernel: 16 -> 16 channels
  CONV_W16,        // conv3x3_w16_kernel: wave-private F(2x2,3x3)
  CONV_WINO2D,     // conv3x3_wino2d_kernel: wave-split F(2x2,3x3), one stage or split K (ksplit > 1)
  CONV_WINO4,      // conv3x3_wino4_kernel: F(4x4,3x3), one stage or split K
  CONV_SMALLMAP,   // conv3x3_sm_kernel
};

struct ConvRoute {
  ConvKernel kernel = CONV_DMA9;
  int kv = 0;      // PH_KV_* code of the launch (ph_model_last_kernels); the register-staged kernel records PH_KV_DIRECT in a forward
  int ksplit = 1;  // K slices of the launch (the two split-K forms; 1 = one stage)
  bool takes_mask = false;    // stores plainly: applies ConvArgs::relu_mask_src (the F(2x2,3x3) / F(4x4,3x3) kernels without fused pool / head / unread dst)
  bool pools = false;         // writes ConvArgs::dst_pool in its epilogue as a Winograd tile's pool window (the two F(2x2,3x3) kernels)
  bool folds_lowres = false;  // reads a half-resolution src1 itself (F(4x4,3x3), small-map)
  bool head_w2d = false;      // may carry a 1x1 head: the wave-split form (64 output channels, <= 32 head channels, one stage)
  bool head_w16 = false;      // ... the wave-private form (16 -> 16 / 32 -> 32 channels, <= 16 head channels)
  bool head_sm = false;       // ... the small-map form (<= 32 output channels)
};

// The kernel that runs `a` on a chip of n_cu CUs (n_cu > 0).
ConvRoute conv3x3_route(const ConvArgs& a, int n_cu);
// The LDS-DMA family's own choice for `a`, whatever the small-map kernel or the register-staged gate would say: what the small-map estimate is compared with,
// and what the head and pool fusions of fwd_conv3x3_f32 ask once the small-map kernel has declined the layer.
ConvRoute conv3x3_family_route(const ConvArgs& a, int n_cu);

// Estimated launch bodies in microseconds (the dispatch floor excluded) on ksplit K slices: rounds of the chip x unit time, + ~8 us for a split-K second stage
double wino4_cost_us(const ConvArgs& a, int n_cu, int ksplit);
double wino2d_cost_us(const ConvArgs& a, int n_cu, int ksplit);
double w16_cost_us(const ConvArgs& a, int n_cu);

// fwd_conv3x3_f32's two questions about the wave-split F(2x2,3x3) kernel that are NOT "does it run": they are asked before the weight pack is chosen and ignore the
// kernels in front of it (moved here word for word from the forward; a.wpack_wino2 etc. are the op's forms)
bool conv3x3_wino2d_sets_rowgemm_fill(const ConvArgs& a);  // conv3x3_prefers_rowgemm compares the row GEMM with 16 x 16-pixel tiles instead of 16 x 32
bool conv3x3_n64_swap_ok(const ConvArgs& a);               // a Cout-32 layer may move to the N-tile-64 pack (the caller checks that the n64 / wino2 / wino forms exist)

int launch_conv3x3_routed(const ConvArgs& a, const ConvRoute& r, hipStream_t s);  // launches what `r` names (net_kernels.hip)

}  // namespace ph
