// Launcher declarations of convnext_f16_kernels.hip: the ConvNeXt encoder ops on plain-fp16 activations (FMT_F16, act_format.h).
// Every kernel reads and writes NHWC fp16 with the channels padded to 32, does its sums in fp32 and writes exact zeros into
// the pad channels.  The per-channel vectors (bias, LayerNorm affine, layer scale) and the vector-pipe weights (patch stem,
// depthwise 7x7) stay the fp32 buffers of the exact path, padded to `wcp` = a multiple of 16 <= cp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace ph {

struct PatchStemF16Args {
  const void* src;    // NCHW uint8 / float image
  const float* w;     // [tap][cin][wcp] fp32
  const float* bias;  // [wcp]
  void* dst;          // FMT_F16, cp channels, OH x OW
  int dtype, cin, wcp, cp, B, H, W, OH, OW, k, stride;
};
int launch_patch_stem_f16(const PatchStemF16Args& a, hipStream_t s);

struct DwConvF16Args {
  const void* src;    // FMT_F16, cp channels
  const float* w;     // [49][wcp] fp32
  const float* bias;  // [wcp]
  void* dst;          // FMT_F16, cp channels
  int wcp, cp, B, H, W;
  // fused LayerNorm over the TRUE channels of the result (dst = LN(dwconv(src))); nullptr = off
  const float* ln_gamma = nullptr;  // [wcp], zero-padded
  const float* ln_beta = nullptr;
  int ln_c = 0;
};
int launch_dwconv7_f16(const DwConvF16Args& a, hipStream_t s);

// eps: 1e-6 for LayerNorm2d / CNBlock's norm (convnext.py:67), 1e-5 for the Swin norms (PH_FLAG_LN_EPS_1EM5)
int launch_layernorm_f16(const void* src, const float* gamma, const float* beta, void* dst, int c, int wcp, int cp, size_t npix, hipStream_t s, float eps = 1e-6f);

// Row GEMM on v_mfma_f32_32x32x16_f16: dst[m][n] = epilogue(sum_k A[m][k] W[n][k] + bias[n]), fp32 accumulators.
struct GemmF16Args {
  const void* src = nullptr;        // FMT_F16 activations, cinp channels per pixel
  const void* wimg = nullptr;       // launch_gemm_f16_weight_image output
  const float* bias = nullptr;      // fp32, >= coutp entries, zero-padded; nullptr: no bias
  const float* scale = nullptr;     // layer scale (fp32, >= coutp, zero-padded) or nullptr; needs a residual
  const void* residual = nullptr;   // FMT_F16 (M, coutp) or nullptr: dst = scale * (acc + bias) + residual, without a scale dst = acc + bias + residual
  void* dst = nullptr;              // FMT_F16 (M, coutp)
  int cinp = 0, coutp = 0;          // padded channels (multiples of 32)
  int M = 0;                        // output rows (pixels)
  int taps = 1;                     // 1: Linear, row m = pixel m; 4: Conv2d k2 s2, row m = output pixel (b, oy, ox), K = 4 cinp (tap = 2 dy + dx outermost)
  int H = 0, W = 0;                 // taps 4: INPUT spatial size
  int gelu = 0;                     // erf-GELU in fp32 on acc + bias
};
int launch_gemm_f16(const GemmF16Args& a, hipStream_t s);
// fp16 weight image of a Linear (taps 1) / Conv2d k2 s2 (taps 4) from the fp32 row-GEMM pack (weights.hip: pack_gemm with N tile bn):
// [32-row block of cout][K step of 16][lane][8 halves] = the A fragment of one MFMA, K = taps x cinp
int64_t gemm_f16_weight_image_halves(int coutp, int cinp, int taps);
int launch_gemm_f16_weight_image(const float* wpack, void* dst, int cout, int cin, int coutp, int cinp, int taps, int bn, hipStream_t s);

// format-generic elementwise ops (load8 / store8): dst = GELU_erf(src); dst = scale[c] * src + residual
int launch_gelu_fmt(int fmt, const void* src, void* dst, size_t npix, int cp, hipStream_t s);
int launch_scale_add_fmt(int fmt, const void* src, const void* residual, const float* scale, void* dst, size_t npix, int wcp, int cp, hipStream_t s);

}  // namespace ph
