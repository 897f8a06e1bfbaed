// ConvNeXtV2 encoder kernels for gfx950 (MI355X, CDNA4): what HuggingFace's ConvNextV2Backbone needs beyond the ConvNeXt ops of
// convnext_kernels.hip (the reference wraps it in PretrainedBackbone, sleap_nn/architectures/pretrained.py).
//
//   embeddings ...... (x / 255 - mean) / std -> Conv2d(k = patch, stride = patch, padding 0, bias); the LayerNorm behind it is a PH_OP_LAYERNORM
//   GRN ............. on the (B, H, W, 4C) hidden tensor of a block, between the GELU and the second Linear:
//                     G[b,c] = sqrt(sum_hw x^2), N[b,c] = G[b,c] / (mean_c G[b,:] + 1e-6), y = weight[c] * (x * N[b,c]) + bias[c] + x
//
// GRN needs all of H x W of a (sample, channel) before any output element: two launches.  grn_reduce_kernel cuts a sample's pixels into
// grn_slices(HW) fixed slices and writes one sum of squares per (sample, slice, channel) -- plain stores, no atomics, every addition in an
// order fixed by the shape, so two forwards of one input are bit-identical and a frame's sums do not depend on the batch around it.
// grn_apply_kernel adds the slices in slice order, takes the channel mean over the true channels and applies.  Layout as everywhere: NHWC
// fp32 with the channels padded to 16; the pad channels of the source are zeros, are left out of the mean and come out as zeros.
#include <algorithm>

#include "common.h"
#include "net_kernels.h"

namespace ph {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// One thread = one output pixel x 4 output channels, straight from the NCHW image.  K = k * k * Cin <= 256 products: VALU work, bound by the NHWC store.
// Weights [tap][ci][Cp] (the patch stem's pack).  Padding 0: every tap of an output pixel lies inside the image (OH = (H - k) / stride + 1).
__global__ __launch_bounds__(256) void patch_stem_norm_kernel(PatchStemArgs a) {
  const int groups = a.coutp >> 2;
  const size_t total = (size_t)a.B * a.OH * a.OW * groups;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int gq = (int)(idx % groups);
    size_t p = idx / groups;
    const int ox = (int)(p % a.OW);
    p /= a.OW;
    const int oy = (int)(p % a.OH);
    const int b = (int)(p / a.OH);
    f32x4 acc = *reinterpret_cast<const f32x4*>(a.bias + gq * 4);
    for (int ci = 0; ci < a.cin; ++ci) {
      const size_t plane = ((size_t)b * a.cin + ci) * a.H * a.W;
      const float mean = a.mean[ci], sd = a.std[ci];
      for (int ky = 0; ky < a.k; ++ky) {
        const int yy = oy * a.stride + ky;
        for (int kx = 0; kx < a.k; ++kx) {
          const int xx = ox * a.stride + kx;
          float v;
          if (a.dtype == 0)
            v = (float)reinterpret_cast<const uint8_t*>(a.src)[plane + (size_t)yy * a.W + xx] / 255.0f;
          else {
            v = reinterpret_cast<const float*>(a.src)[plane + (size_t)yy * a.W + xx];
            if (a.dtype == 2) v = v / 255.0f;
          }
          v = (v - mean) / sd;
          const f32x4 w = *reinterpret_cast<const f32x4*>(a.w + ((size_t)(ky * a.k + kx) * a.cin + ci) * a.coutp + gq * 4);
          acc += v * w;
        }
      }
    }
    *reinterpret_cast<f32x4*>(a.dst + (((size_t)b * a.OH + oy) * a.OW + ox) * a.coutp + gq * 4) = acc;
  }
}

int launch_patch_stem_norm(const PatchStemArgs& a, hipStream_t s) {
  PH_REQUIRE(a.pad0_norm && a.cin >= 1 && a.cin <= 4 && !a.ln_gamma && (a.coutp & 3) == 0, "patch_stem_norm_kernel takes 1..4 input channels and no fused LayerNorm");
  PH_REQUIRE(a.OH == (a.H - a.k) / a.stride + 1 && a.OW == (a.W - a.k) / a.stride + 1 && a.OH > 0 && a.OW > 0, "patch stem output size does not match padding 0");
  const size_t total = (size_t)a.B * a.OH * a.OW * (a.coutp / 4);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(patch_stem_norm_kernel, dim3(blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// GRN.  A workgroup of the reduction owns (slice, sample, chunk of <= 256 channel quads).  Its 256 threads are rows x quads: thread (r, q) adds the
// squares of quad q over the slice's pixels r, r + rows, ..., then row 0 adds the rows' sums in row order and stores.  Every load is a float4 of a
// contiguous run of channels.
// ---------------------------------------------------------------------------------------
constexpr int GRN_MIN_SLICE = 256;  // pixels
constexpr int GRN_MAX_SLICES = 32;

int grn_slice_pixels(int HW) { return std::max(GRN_MIN_SLICE, (HW + GRN_MAX_SLICES - 1) / GRN_MAX_SLICES); }
int grn_slices(int HW) { return (HW + grn_slice_pixels(HW) - 1) / grn_slice_pixels(HW); }
int64_t grn_scratch_floats(int B, int HW, int cp) { return (int64_t)B * grn_slices(HW) * cp; }

__global__ __launch_bounds__(256) void grn_reduce_kernel(const float* __restrict__ src, float* __restrict__ partial, int HW, int cp, int slice_px, int nslices) {
  __shared__ f32x4 sh[256];
  const int G = cp >> 2;
  const int slice = blockIdx.x, b = blockIdx.y, q0 = blockIdx.z * 256;
  const int gc = min(256, G - q0);  // quads of this chunk
  const int rows = 256 / gc;
  const int tid = threadIdx.x, r = tid / gc, q = tid - r * gc;
  const int p0 = slice * slice_px, p1 = min(HW, p0 + slice_px);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (r < rows) {
    const float* base = src + (size_t)b * HW * cp + (size_t)(q0 + q) * 4;
    // four loads in flight per thread, four partial sums: the order of the additions is still a function of the shape alone
    f32x4 a1 = {0.f, 0.f, 0.f, 0.f}, a2 = a1, a3 = a1;
    int p = p0 + r;
    for (; p + 3 * rows < p1; p += 4 * rows) {
      const f32x4 v0 = *reinterpret_cast<const f32x4*>(base + (size_t)p * cp);
      const f32x4 v1 = *reinterpret_cast<const f32x4*>(base + (size_t)(p + rows) * cp);
      const f32x4 v2 = *reinterpret_cast<const f32x4*>(base + (size_t)(p + 2 * rows) * cp);
      const f32x4 v3 = *reinterpret_cast<const f32x4*>(base + (size_t)(p + 3 * rows) * cp);
      acc += v0 * v0;
      a1 += v1 * v1;
      a2 += v2 * v2;
      a3 += v3 * v3;
    }
    for (; p < p1; p += rows) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(base + (size_t)p * cp);
      acc += v * v;
    }
    acc = (acc + a1) + (a2 + a3);
  }
  sh[tid] = acc;
  __syncthreads();
  if (r == 0) {
    for (int k = 1; k < rows; ++k) acc += sh[k * gc + q];
    *reinterpret_cast<f32x4*>(partial + ((size_t)b * nslices + slice) * cp + (size_t)(q0 + q) * 4) = acc;
  }
}

// A workgroup of the apply pass owns (slice, sample): it rebuilds the sample's N[c] in LDS from the slice sums (nslices x cp floats out of L2, against the
// slice_px x cp floats it then streams), then y = weight * (x * N) + bias + x over its pixels, float4 per thread, channels fastest.
__global__ __launch_bounds__(256) void grn_apply_kernel(GrnArgs a, int slice_px, int nslices) {
  extern __shared__ float sN[];  // [cp]
  __shared__ float sRed[256];
  const int G = a.cp >> 2;
  const int slice = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  float local = 0.f;
  for (int q = tid; q < G; q += 256) {
    const float* pp = a.partial + (size_t)b * nslices * a.cp + (size_t)q * 4;
    f32x4 ss = *reinterpret_cast<const f32x4*>(pp);
    for (int k = 1; k < nslices; ++k) ss += *reinterpret_cast<const f32x4*>(pp + (size_t)k * a.cp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g = (q * 4 + e < a.c) ? sqrtf(ss[e]) : 0.f;
      sN[q * 4 + e] = g;
      local += g;
    }
  }
  sRed[tid] = local;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) sRed[tid] += sRed[tid + d];
    __syncthreads();
  }
  const float denom = sRed[0] / (float)a.c + 1e-6f;
  for (int q = tid; q < a.cp; q += 256) sN[q] = sN[q] / denom;  // (other threads' G values: the barriers of the sum above made them visible)
  __syncthreads();
  const int p0 = slice * slice_px, p1 = min(a.HW, p0 + slice_px);
  const size_t base = ((size_t)b * a.HW + p0) * a.cp;
  const int total = (p1 - p0) * G;
  int q = tid % G;          // channel quad of element e = tid + 256 k: advanced by 256 mod G per step instead of a division per element
  const int dq = 256 % G;
#pragma unroll 4
  for (int e = tid; e < total; e += 256) {
    const f32x4 x = *reinterpret_cast<const f32x4*>(a.src + base + (size_t)e * 4);
    const f32x4 n = *reinterpret_cast<const f32x4*>(sN + q * 4);
    const f32x4 w = *reinterpret_cast<const f32x4*>(a.weight + q * 4);
    const f32x4 bb = *reinterpret_cast<const f32x4*>(a.bias + q * 4);
    *reinterpret_cast<f32x4*>(a.dst + base + (size_t)e * 4) = w * (x * n) + bb + x;
    q += dq;
    q -= q >= G ? G : 0;
  }
}

int launch_grn(const GrnArgs& a, hipStream_t s) {
  PH_REQUIRE(a.src && a.dst && a.partial && a.weight && a.bias, "launch_grn: null argument");
  PH_REQUIRE(a.B > 0 && a.B <= 65535 && a.HW > 0 && a.c > 0 && a.c <= a.cp && (a.cp & 15) == 0 && a.cp <= 15360, "launch_grn: bad shape (B %d, HW %d, C %d / %d)", a.B, a.HW, a.c, a.cp);
  PH_REQUIRE((int64_t)a.HW * (a.cp >> 2) < ((int64_t)1 << 31), "launch_grn: a sample has 2^31 channel quads or more");
  const int slice_px = grn_slice_pixels(a.HW), nslices = grn_slices(a.HW);
  const int chunks = ((a.cp >> 2) + 255) / 256;
  hipLaunchKernelGGL(grn_reduce_kernel, dim3(nslices, a.B, chunks), dim3(256), 0, s, a.src, a.partial, a.HW, a.cp, slice_px, nslices);
  PH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(grn_apply_kernel, dim3(nslices, a.B), dim3(256), (size_t)a.cp * sizeof(float), s, a, slice_px, nslices);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Fused GRN plan (handle option "grn_fuse").  The Linear + GELU GEMM's epilogue has left, for every 32-row block of the (B HW, Cp) hidden tensor and every
// sample the block touches, the sum of squares of that sample's rows in the block (a block that straddles a sample boundary has split its sum there; with
// fewer than 32 pixels per sample a block holds several whole samples).  Sample b's rows [b HW, (b + 1) HW) lie in blocks b HW / 32 .. ((b + 1) HW - 1) / 32, and
// in block k it is segment b - (32 k) / HW.  One workgroup per sample adds them in block order -- no atomics -- and writes scale[b][c] = 1 + weight[c] N[b,c].
// ---------------------------------------------------------------------------------------
int grn_fused_nseg(int HW) { return 31 / HW + 2; }
int64_t grn_fused_partial_floats(int M, int HW, int cp) { return (int64_t)((M + 31) / 32) * grn_fused_nseg(HW) * cp; }

__global__ __launch_bounds__(256) void grn_finalize_kernel(const float* __restrict__ partial, const float* __restrict__ weight, float* __restrict__ scale, int HW, int c, int cp, int nseg) {
  extern __shared__ float sG[];  // [cp]
  __shared__ float sRed[256];
  const int b = blockIdx.x, tid = threadIdx.x, G = cp >> 2;
  const int k0 = (int)(((long long)b * HW) >> 5), k1 = (int)((((long long)b + 1) * HW - 1) >> 5);
  float local = 0.f;
  for (int q = tid; q < G; q += 256) {
    f32x4 ss = {0.f, 0.f, 0.f, 0.f};
    for (int k = k0; k <= k1; ++k) {
      const int seg = b - (int)(((long long)k << 5) / HW);
      ss += *reinterpret_cast<const f32x4*>(partial + ((size_t)k * nseg + seg) * cp + (size_t)q * 4);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const float g = (q * 4 + e < c) ? sqrtf(ss[e]) : 0.f;
      sG[q * 4 + e] = g;
      local += g;
    }
  }
  sRed[tid] = local;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) sRed[tid] += sRed[tid + d];
    __syncthreads();
  }
  const float denom = sRed[0] / (float)c + 1e-6f;
  for (int i = tid; i < cp; i += 256) scale[(size_t)b * cp + i] = 1.0f + weight[i] * (sG[i] / denom);  // (pad channels: weight 0 -> 1)
}

int launch_grn_finalize(const float* partial, const float* weight, float* scale, int B, int HW, int c, int cp, hipStream_t s) {
  PH_REQUIRE(partial && weight && scale && B > 0 && HW > 0 && c > 0 && c <= cp && (cp & 15) == 0 && cp <= 15360, "launch_grn_finalize: bad arguments");
  hipLaunchKernelGGL(grn_finalize_kernel, dim3(B), dim3(256), (size_t)cp * sizeof(float), s, partial, weight, scale, HW, c, cp, grn_fused_nseg(HW));
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// The fused plan's constant term W2 grn.bias + b2, recomputed from a device parameter arena (ph_model_set_params: ph_model_create folds it on the host, and the parameters
// move once the backbone trains).  One thread per output channel, a double-precision sum in input-channel order: the products of two floats are exact in double, so
// this is the host fold bit for bit.  cout x cin multiply-adds, once per parameter upload of an inference handle.
__global__ __launch_bounds__(256) void grn_fold_bias_kernel(const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ grn_bias, float* __restrict__ dst, int cout, int cin) {
  const int co = blockIdx.x * 256 + threadIdx.x;
  if (co >= cout) return;
  double acc = b2[co];
  for (int ci = 0; ci < cin; ++ci) acc += (double)w2[(size_t)co * cin + ci] * (double)grn_bias[ci];
  dst[co] = (float)acc;
}

int launch_grn_fold_bias(const float* w2, const float* b2, const float* grn_bias, float* dst, int cout, int cin, hipStream_t s) {
  PH_REQUIRE(w2 && b2 && grn_bias && dst && cout > 0 && cin > 0, "launch_grn_fold_bias: bad arguments");
  hipLaunchKernelGGL(grn_fold_bias_kernel, dim3((cout + 255) / 256), dim3(256), 0, s, w2, b2, grn_bias, dst, cout, cin);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// pack_gemm image of a Linear (one tap, one source): [n tile][stage of 32 input channels][piece = n / 8][slot][row n % 8][4], input channel = 32 stage + 4 (slot ^ (piece & 1)) + e
int64_t gemm_pack_floats(int coutp, int c0p, int bn) { return (int64_t)((coutp + bn - 1) / bn) * ((c0p + 31) / 32) * (bn / 8) * 256; }

__global__ __launch_bounds__(256) void grn_scale_weights_kernel(const float* __restrict__ wpack, const float* __restrict__ scale, float* __restrict__ dst, long long quads, int stages, int bp, int c0p) {
  const int b = blockIdx.y;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < quads; i += (long long)gridDim.x * 256) {
    const int slot = (int)((i >> 3) & 7);  // a quad is 4 floats: 64 quads per 256-float piece, 8 per slot
    const long long piece = i >> 6;
    const int pb = (int)(piece % bp), st = (int)((piece / bp) % stages);
    const int ch = st * 32 + ((slot ^ (pb & 1)) << 2);
    f32x4 w = *reinterpret_cast<const f32x4*>(wpack + i * 4);
    if (ch < c0p) w *= *reinterpret_cast<const f32x4*>(scale + (size_t)b * c0p + ch);  // (channels past c0p hold zero weights)
    *reinterpret_cast<f32x4*>(dst + (size_t)b * quads * 4 + i * 4) = w;
  }
}

int launch_grn_scale_weights(const float* wpack, const float* scale, float* dst, int B, int coutp, int c0p, int bn, hipStream_t s) {
  PH_REQUIRE(wpack && scale && dst && B > 0 && B <= 65535 && (c0p & 15) == 0 && (bn & 7) == 0, "launch_grn_scale_weights: bad arguments");
  const long long quads = gemm_pack_floats(coutp, c0p, bn) / 4;
  const unsigned gx = (unsigned)std::min<long long>((quads + 255) / 256, 4096);
  hipLaunchKernelGGL(grn_scale_weights_kernel, dim3(gx, B), dim3(256), 0, s, wpack, scale, dst, quads, (c0p + 31) / 32, bn / 8, c0p);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph
