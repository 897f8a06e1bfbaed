// ResNet encoder kernels for gfx950 (MI355X, CDNA4): what HuggingFace's ResNetBackbone needs beyond the ops the other encoders already have (the reference wraps it in
// PretrainedBackbone, sleap_nn/architectures/pretrained.py).  BatchNorm (eval) is folded into each conv's weight and bias on the host, so every conv here is conv + bias (+ ReLU).
//
//   stem ........ (x / 255 - mean) / std -> Conv2d(k7, s2, p3) + bias + ReLU -> MaxPool2d(k3, s2, p1), two launches: resnet_stem_conv_kernel, maxpool3s2_kernel
//   add + ReLU .. the tail of a basic block: dst = relu(src0 + src1)
//
// The strided 3x3 and 1x1 convs and the bottleneck's 1x1 convs are row GEMMs (convnext_kernels.hip: gemm_mfma_dma_tile_kernel modes 4 and 6), the stride-1 3x3 convs are
// PH_OP_CONV.  Layout as everywhere: NHWC fp32 with the channels padded to 16; pad channels have zero weights and a zero bias and come out as zeros.
#include <algorithm>

#include "common.h"
#include "net_kernels.h"

namespace ph {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

// ---------------------------------------------------------------------------------------
// Stem conv as an im2col product on the fp32 matrix pipe.  A workgroup (4 waves) owns a tile of 4 rows x 32 columns of the stride-2 map: it stages the 13 x 69 input
// pixels the tile's taps reach, NORMALISED, in LDS -- a pixel outside the frame is 0 there, i.e. the zero padding applies to the normalised image (which is why the
// statistics cannot be folded into the weights).  Wave w owns row w: 32 pixels = the N side of v_mfma_f32_32x32x2_f32, 32 output channels = its M side, K = 49 cin in
// KH = ceil(K / 2) steps.  Step s multiplies k = s in the lower lane half and k = s + KH in the upper one; the weights come from HBM / L2 in exactly that order
// ([N block][step][lane]: one coalesced 256-B load per step), the pixels from LDS through a table of the taps' offsets.  Accumulation order is a function of the layer
// alone: two forwards are bit-identical and a frame's result does not depend on the batch around it.
// ---------------------------------------------------------------------------------------
constexpr int RS_ROWS = 4, RS_COLS = 32;
constexpr int RS_IN_ROWS = 2 * RS_ROWS + 5, RS_IN_COLS = 2 * RS_COLS + 5;  // 13 x 69
constexpr int RS_PLANE = RS_IN_ROWS * RS_IN_COLS;
constexpr int RS_MAX_CIN = 4, RS_MAX_KH = (49 * RS_MAX_CIN + 1) / 2;

__global__ __launch_bounds__(256) void resnet_stem_conv_kernel(ResnetStemArgs a) {
  __shared__ float tile[RS_MAX_CIN * RS_PLANE];
  __shared__ int koff[2 * RS_MAX_KH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ox0 = blockIdx.x * RS_COLS, oy0 = blockIdx.y * RS_ROWS, b = blockIdx.z;
  const int K = 49 * a.cin, KH = (K + 1) >> 1;
  for (int idx = tid; idx < a.cin * RS_PLANE; idx += 256) {
    const int ci = idx / RS_PLANE, r = idx - ci * RS_PLANE;
    const int iy = r / RS_IN_COLS, ix = r - iy * RS_IN_COLS;
    const int gy = 2 * oy0 - 3 + iy, gx = 2 * ox0 - 3 + ix;
    float v = 0.f;  // outside the frame: the conv's zero padding, applied AFTER the normalisation
    if (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
      const size_t at = (((size_t)b * a.cin + ci) * a.H + gy) * a.W + gx;
      if (a.dtype == 0)
        v = (float)reinterpret_cast<const uint8_t*>(a.src)[at] / 255.0f;
      else {
        v = reinterpret_cast<const float*>(a.src)[at];
        if (a.dtype == 2) v = v / 255.0f;
      }
      v = (v - a.mean[ci]) / a.std[ci];
    }
    tile[idx] = v;
  }
  for (int k = tid; k < 2 * KH; k += 256) {
    int off = 0;  // (k = K of an odd K: its weight is zero, any staged pixel will do)
    if (k < K) {
      const int ci = k / 49, t = k - ci * 49;
      off = ci * RS_PLANE + (t / 7) * RS_IN_COLS + (t % 7);
    }
    koff[k] = off;
  }
  __syncthreads();
  const int px = lane & 31, lh = lane >> 5;
  const int pbase = 2 * wave * RS_IN_COLS + 2 * px;
  const int oy = oy0 + wave, ox = ox0 + px;
  const int nblk = (a.coutp + 31) >> 5;
  for (int nb = 0; nb < nblk; ++nb) {
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float* wl = a.wimg + (size_t)nb * KH * 64 + lane;
    for (int s = 0; s < KH; ++s) {
      const float wv = wl[(size_t)s * 64];
      const float xv = tile[koff[s + KH * lh] + pbase];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wv, xv, acc, 0, 0, 0);  // D[channel][pixel]: a lane owns pixel (lane & 31), its registers run over channels
    }
    if (oy < a.OH && ox < a.OW) {
      float* o = a.conv_dst + (((size_t)b * a.OH + oy) * a.OW + ox) * a.coutp;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int col = nb * 32 + 8 * q + 4 * lh;  // registers 4 q .. 4 q + 3: four consecutive channels
        if (col < a.coutp) {                       // (coutp is a multiple of 16: a quad is inside or outside as a whole)
          const f32x4 bq = *reinterpret_cast<const f32x4*>(a.bias + col);
          f32x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = fmaxf(acc[4 * q + e] + bq[e], 0.f);
          *reinterpret_cast<f32x4*>(o + col) = v;
        }
      }
    }
  }
}

// MaxPool2d(k3, s2, p1) over an NHWC map, one thread per (output pixel, channel quad).  torch pads with -inf: a tap outside the map never wins.  That equals zero
// padding here only because the pool follows a ReLU (every value is >= 0 and the window's centre tap is always inside); the kernel keeps the -inf form so that it
// stays right for any input.
__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W, int PH, int PW, int cp) {
  const int groups = cp >> 2;
  const size_t total = (size_t)B * PH * PW * groups;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int gq = (int)(idx % groups);
    size_t p = idx / groups;
    const int x = (int)(p % PW);
    p /= PW;
    const int y = (int)(p % PH);
    const int b = (int)(p / PH);
    const float ninf = -__builtin_inff();
    f32x4 m = {ninf, ninf, ninf, ninf};
    for (int dy = -1; dy <= 1; ++dy) {
      const int yy = 2 * y + dy;
      if (yy < 0 || yy >= H) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xx = 2 * x + dx;
        if (xx < 0 || xx >= W) continue;
        const f32x4 v = *reinterpret_cast<const f32x4*>(src + (((size_t)b * H + yy) * W + xx) * cp + gq * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    }
    *reinterpret_cast<f32x4*>(dst + (((size_t)b * PH + y) * PW + x) * cp + gq * 4) = m;
  }
}

int64_t resnet_stem_weight_floats(int cin, int coutp) { return (int64_t)((coutp + 31) / 32) * ((49 * cin + 1) / 2) * 64; }

int launch_resnet_stem(const ResnetStemArgs& a, hipStream_t s) {
  PH_REQUIRE(a.cin >= 1 && a.cin <= RS_MAX_CIN && a.coutp > 0 && a.coutp % 16 == 0 && a.B > 0 && a.B <= 65535, "resnet stem takes 1..4 input channels and a batch of at most 65535");
  PH_REQUIRE(a.OH == (a.H - 1) / 2 + 1 && a.OW == (a.W - 1) / 2 + 1 && a.PH == (a.OH - 1) / 2 + 1 && a.PW == (a.OW - 1) / 2 + 1, "resnet stem output sizes do not match k7 s2 p3 / k3 s2 p1");
  const dim3 grid((unsigned)((a.OW + RS_COLS - 1) / RS_COLS), (unsigned)((a.OH + RS_ROWS - 1) / RS_ROWS), (unsigned)a.B);
  PH_REQUIRE(grid.y <= 65535, "resnet stem: frame too tall");
  hipLaunchKernelGGL(resnet_stem_conv_kernel, grid, dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

int launch_maxpool3s2(const float* src, float* dst, int B, int H, int W, int cp, hipStream_t s) {
  const int PH = (H - 1) / 2 + 1, PW = (W - 1) / 2 + 1;
  const size_t total = (size_t)B * PH * PW * (cp / 4);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3(blocks), dim3(256), 0, s, src, dst, B, H, W, PH, PW, cp);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// dst = relu(a + b) over n floats (n a multiple of 4: whole pixels of a channel-padded map).  Pad channels are zero in both sources and stay zero.
__global__ __launch_bounds__(256) void add_relu_kernel(const float* __restrict__ x, const float* __restrict__ y, float* __restrict__ dst, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const f32x4 u = reinterpret_cast<const f32x4*>(x)[i], v = reinterpret_cast<const f32x4*>(y)[i];
    f32x4 r;
#pragma unroll
    for (int e = 0; e < 4; ++e) r[e] = fmaxf(u[e] + v[e], 0.f);
    reinterpret_cast<f32x4*>(dst)[i] = r;
  }
}

int launch_add_relu(const float* x, const float* y, float* dst, size_t n, hipStream_t s) {
  PH_REQUIRE(n > 0 && n % 4 == 0, "add_relu: element count must be a positive multiple of 4");
  const size_t n4 = n / 4;
  const int blocks = (int)std::min<size_t>((n4 + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(add_relu_kernel, dim3(blocks), dim3(256), 0, s, x, y, dst, n4);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph
