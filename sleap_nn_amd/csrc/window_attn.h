// Window attention: the token geometry, the argument struct and the host-side check that the five kernels share (swin_kernels.hip: window_attn_kernel, plain and
// cosine; swin_f16_kernels.hip: window_attn_f16_kernel; swin_train_kernels.hip: window_attn_bwd_kernel; swinv2_kernels.hip: window_attn_v2_wide_kernel).
//
// The map (B, H, W) is padded to multiples of the window side w, rolled by (-sh, -sw) and cut into w x w windows; all of it is index arithmetic:
//   * windows are numbered (b, wy, wx), a launch's items (window, head) with the head fastest;
//   * token t = ty w + tx of window (wy, wx) sits at (ry, rx) = (wy w + ty, wx w + tx) of the rolled, padded grid and comes from pixel ((ry + sh) mod pH,
//     (rx + sw) mod pW); past the map it is a padded token (pix = -1): its q, k, v are qkv_bias, it is a key like any other and it is never stored;
//   * band mask of a shifted axis: only the last window row / column holds two bands, split at w - shift.  Two tokens of a window are masked against each other where
//     their bands differ;
//   * the accumulator registers of a 32x32 MFMA tile hold the keys in the order window_key(); the relative-position bias of a pair is window_bias_index().
// Everything here is __host__ __device__: ph_debug_window_tokens (swin_kernels.hip) fills the token map on the host, with no HIP call, from the same functions the
// kernels call (tests/test_window_geometry_cpu.py).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace ph {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// Geometry of one launch, as every window-attention argument struct carries it
struct WindowGeom {
  int B = 0, H = 0, W = 0, C = 0, heads = 0;
  int w = 0;           // window side: 2..8, or 2..24 for the key-tiled kernel
  int sh = 0, sw = 0;  // per-axis shift.  Swin (torchvision): window_axis_shift() per axis; Swinv2 (HuggingFace): the layer's shift on both axes, whatever the map
};

struct WindowAttnArgs : WindowGeom {
  const void* qkv = nullptr;        // (B, H, W, 3C): q | k | v of the un-padded, un-rolled map; head a owns channels 32 a .. 32 a + 31 of each.  fp32; FMT_F16 for the fp16 kernel
  const float* table = nullptr;     // bias table, head-major: [heads][(2w - 1)^2] (Swin: relative_position_bias_table; Swinv2: 16 sigmoid(continuous position bias))
  const float* qkv_bias = nullptr;  // (3C) fp32: what a padded token's q, k, v are (Swinv2: query.bias | zeros | value.bias)
  const float* scale = nullptr;     // cosine kernels only: (heads) exp(min(logit_scale, log 100))
  void* dst = nullptr;              // (B, H, W, C), in the format of qkv
};

// torchvision's shifted_window_attention: an axis the window covers whole (window >= padded size) is not shifted.  Decided per axis, from the launch's own map.
__host__ __device__ inline int window_axis_shift(int size, int w, int shift) { return w >= (size + w - 1) / w * w ? 0 : shift; }

struct WindowGrid {
  int H, W, w;
  int pH, pW;      // padded map
  int nwh, nww;    // windows per column / row
  int N, rel;      // tokens per window, entries of one head's bias table
  long long nwin;  // B nwh nww
};
__host__ __device__ inline WindowGrid window_grid(int B, int H, int W, int w) {
  WindowGrid g;
  g.H = H, g.W = W, g.w = w;
  g.pH = (H + w - 1) / w * w, g.pW = (W + w - 1) / w * w;
  g.nwh = g.pH / w, g.nww = g.pW / w;
  g.N = w * w, g.rel = (2 * w - 1) * (2 * w - 1);
  g.nwin = (long long)B * g.nwh * g.nww;
  return g;
}

// item = (first_window + window) heads + head -> its window and head.  I: the width the caller's item index has (long long, or unsigned where it is a block index)
struct WindowItem {
  int b, wy, wx, head;
};
template <typename I>
__host__ __device__ inline WindowItem window_decode(const WindowGrid& g, I item, int heads, I first_window = 0) {
  WindowItem it;
  it.head = (int)(item % (I)heads);
  I win = first_window + item / (I)heads;
  it.wx = (int)(win % (I)g.nww);
  win /= (I)g.nww;
  it.wy = (int)(win % (I)g.nwh);
  it.b = (int)(win / (I)g.nwh);
  return it;
}

struct TokenInfo {
  int pix;   // pixel index (b H + y) W + x, -1 = padded token
  int code;  // ty | tx << BITS | band << 2 BITS
};
// BITS: width of a coordinate field, 4 for windows up to 16 a side (the one-wave kernels: up to 8), 5 up to 24 (the key-tiled kernel)
template <int BITS>
__host__ __device__ inline TokenInfo window_token(const WindowGrid& g, const WindowItem& it, int t, int sh, int sw) {
  const int w = g.w;
  const int ty = t / w, tx = t - ty * w;
  int y = it.wy * w + ty + sh, x = it.wx * w + tx + sw;
  if (y >= g.pH) y -= g.pH;
  if (x >= g.pW) x -= g.pW;
  const int band = ((sh > 0 && it.wy == g.nwh - 1 && ty >= w - sh) ? 2 : 0) | ((sw > 0 && it.wx == g.nww - 1 && tx >= w - sw) ? 1 : 0);
  TokenInfo k;
  k.pix = (y < g.H && x < g.W) ? (it.b * g.H + y) * g.W + x : -1;
  k.code = ty | (tx << BITS) | (band << (2 * BITS));
  return k;
}
template <int BITS>
__host__ __device__ inline int token_ty(int code) { return code & ((1 << BITS) - 1); }
template <int BITS>
__host__ __device__ inline int token_tx(int code) { return (code >> BITS) & ((1 << BITS) - 1); }
template <int BITS>
__host__ __device__ inline int token_band(int code) { return code >> (2 * BITS); }

// The key that accumulator register r of lane half `half` holds in 32-key tile tj of a v_mfma_f32_32x32 product
__host__ __device__ constexpr int window_key(int tj, int r, int half) { return tj * 32 + 8 * (r >> 2) + 4 * half + (r & 3); }

// Bias table entry of query i against key j: (ty_i - ty_j + w - 1)(2w - 1) + (tx_i - tx_j + w - 1).  The key-tiled kernel sums the query's part once per query tile:
// window_bias_index(ci, cj, w) == window_bias_row(ci, w) - window_bias_col(cj, w).
template <int BITS>
__host__ __device__ inline int window_bias_index(int ci, int cj, int w) {
  return (token_ty<BITS>(ci) - token_ty<BITS>(cj) + w - 1) * (2 * w - 1) + (token_tx<BITS>(ci) - token_tx<BITS>(cj) + w - 1);
}
template <int BITS>
__host__ __device__ inline int window_bias_row(int ci, int w) { return (token_ty<BITS>(ci) + w - 1) * (2 * w - 1) + (token_tx<BITS>(ci) + w - 1); }
template <int BITS>
__host__ __device__ inline int window_bias_col(int cj, int w) { return token_ty<BITS>(cj) * (2 * w - 1) + token_tx<BITS>(cj); }

// The one argument check of every launcher (swin_kernels.hip).  label names the kernel in the messages, max_w is its largest window, pointers whether every pointer it
// needs is set.  On success *g is the launch's grid and, where blocks is given, *blocks the workgroups of a launch that puts `per_block` (window, head) items in each.
int window_attn_check(const char* label, int max_w, bool pointers, const WindowGeom& a, WindowGrid* g, int per_block = 0, unsigned* blocks = nullptr);

}  // namespace ph
