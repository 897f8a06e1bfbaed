// ConvNeXt encoder ops on plain-fp16 activations for gfx950 (the reference's autocast mode, torch_backend.py:113-143; its
// tolerance is 5e-3).  The fp32 forms and the reference semantics of every op: convnext_kernels.hip.
//
// Storage is FMT_F16 (act_format.h): NHWC fp16, channels padded to 32.  Every tensor of the program, the CNBlock residual
// stream included, is stored in fp16 (tools/convnext_f16_emulation.py measures what that costs: ~1e-3 of the heads' scale,
// the same as with an fp32 residual stream); all arithmetic inside a kernel is fp32: the vector-pipe ops (patch stem,
// depthwise 7x7) multiply fp32 weights, LayerNorm takes its moments in fp32 over the TRUE channel count, the row GEMM
// accumulates fp16 products in fp32 on v_mfma_f32_32x32x16_f16 and evaluates bias / erf-GELU / layer scale + residual on the
// fp32 accumulators.  Pad channels are written as exact zeros: zero weight rows and zero-padded bias / affine / scale vectors
// (fp32, padded to `wcp` = a multiple of 16; channels in [wcp, cp) are forced to zero).
#include <algorithm>

#include "act_format.h"
#include "common.h"
#include "convnext_f16_kernels.h"
#include "device_math.h"

namespace ph {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {
constexpr float LN_EPS_F16 = 1e-6f;  // eps of LayerNorm2d / CNBlock's nn.LayerNorm (convnext.py:67)
constexpr int DW_STRIP = 8, DW_ROWS = 2;

__device__ __forceinline__ float image_value(const void* src, int dtype, size_t o) {
  if (dtype == 0) return (float)reinterpret_cast<const uint8_t*>(src)[o] / 255.0f;
  const float v = reinterpret_cast<const float*>(src)[o];
  return dtype == 2 ? v / 255.0f : v;
}
}  // namespace

// ---------------------------------------------------------------------------------------
// Patch stem: image / 255 -> k x k conv, stride s, padding 1, + bias -> fp16.  One thread = one output pixel x 8 output
// channels (one 16-byte store); any number of input channels (gray and RGB), uint8 and float images.  Weights [tap][ci][wcp].
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_stem_f16_kernel(PatchStemF16Args a) {
  const int groups = a.cp >> 3;
  const size_t total = (size_t)a.B * a.OH * a.OW * groups;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int g = (int)(idx % groups);
    size_t p = idx / groups;
    const size_t pix = p;
    const int ox = (int)(p % a.OW);
    p /= a.OW;
    const int oy = (int)(p % a.OH);
    const int b = (int)(p / a.OH);
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (8 * g < a.wcp) {
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.bias + 8 * g), b1 = *reinterpret_cast<const f32x4*>(a.bias + 8 * g + 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc[e] = b0[e];
        acc[4 + e] = b1[e];
      }
      for (int ci = 0; ci < a.cin; ++ci) {
        const size_t plane = ((size_t)b * a.cin + ci) * a.H * a.W;
        for (int ky = 0; ky < a.k; ++ky) {
          const int yy = oy * a.stride + ky - 1;
          if (yy < 0 || yy >= a.H) continue;
          for (int kx = 0; kx < a.k; ++kx) {
            const int xx = ox * a.stride + kx - 1;
            if (xx < 0 || xx >= a.W) continue;
            const float v = image_value(a.src, a.dtype, plane + (size_t)yy * a.W + xx);
            const float* wp = a.w + ((size_t)(ky * a.k + kx) * a.cin + ci) * a.wcp + 8 * g;
            const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              acc[e] += v * w0[e];
              acc[4 + e] += v * w1[e];
            }
          }
        }
      }
    }
    store8<FMT_F16>(a.dst, pix, a.cp, g, acc);
  }
}

int launch_patch_stem_f16(const PatchStemF16Args& a, hipStream_t s) {
  PH_REQUIRE(a.src && a.w && a.bias && a.dst && a.cp % 32 == 0 && a.wcp % 16 == 0 && a.wcp <= a.cp && a.cin >= 1 && a.OH > 0 && a.OW > 0, "patch_stem_f16: bad arguments");
  const size_t total = (size_t)a.B * a.OH * a.OW * (a.cp / 8);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 256 * 32);
  hipLaunchKernelGGL(patch_stem_f16_kernel, dim3(blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Depthwise 7x7 "same" convolution + bias on fp16 activations: dwconv7_kernel's plan (one thread = 4 channels x a block of
// DW_ROWS x DW_STRIP output pixels, the 14 input values of a row kept in registers for every output they feed) with 8-byte
// loads of four halves in place of 16-byte loads of four floats: half the bytes of the bandwidth-bound fp32 form.
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ void dw7_f16_accumulate(const DwConvF16Args& a, int b, int y0, int x0, int gq, f32x4 (&acc)[DW_ROWS][DW_STRIP]) {
  const bool wok = gq * 4 < a.wcp;  // channels in [wcp, cp) have no weights: exact zeros
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  const f32x4 bias = wok ? *reinterpret_cast<const f32x4*>(a.bias + gq * 4) : zero;
#pragma unroll
  for (int r = 0; r < DW_ROWS; ++r)
#pragma unroll
    for (int o = 0; o < DW_STRIP; ++o) acc[r][o] = bias;
  if (!wok) return;
  const float* wq = a.w + gq * 4;
  const _Float16* src = reinterpret_cast<const _Float16*>(a.src);
#pragma unroll
  for (int ir = 0; ir < DW_ROWS + 6; ++ir) {
    const int iy = y0 + ir - 3;
    if (iy < 0 || iy >= a.H) continue;
    const _Float16* row = src + ((size_t)(b * a.H + iy) * a.W) * a.cp + gq * 4;
    f32x4 in[DW_STRIP + 6];
#pragma unroll
    for (int i = 0; i < DW_STRIP + 6; ++i) {
      const int ix = x0 + i - 3;
      const int cx = min(max(ix, 0), a.W - 1);
      const f16x4 v = *reinterpret_cast<const f16x4*>(row + (size_t)cx * a.cp);
      const bool ok = ix >= 0 && ix < a.W;
#pragma unroll
      for (int e = 0; e < 4; ++e) in[i][e] = ok ? (float)v[e] : 0.f;
    }
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r) {
      const int ky = ir - r;  // this input row is kernel row ky of output row r
      if (ky < 0 || ky > 6) continue;
#pragma unroll
      for (int kx = 0; kx < 7; ++kx) {
        const f32x4 w = *reinterpret_cast<const f32x4*>(wq + (size_t)(ky * 7 + kx) * a.wcp);
#pragma unroll
        for (int o = 0; o < DW_STRIP; ++o) acc[r][o] += in[o + kx] * w;
      }
    }
  }
}

__global__ __launch_bounds__(256) void dwconv7_f16_kernel(DwConvF16Args a) {
  const int groups = a.cp >> 2;
  const int strips = (a.W + DW_STRIP - 1) / DW_STRIP;
  const int rblocks = (a.H + DW_ROWS - 1) / DW_ROWS;
  const size_t total = (size_t)a.B * rblocks * strips * groups;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int gq = (int)(idx % groups);
    size_t p = idx / groups;
    const int st = (int)(p % strips);
    p /= strips;
    const int rb = (int)(p % rblocks);
    const int b = (int)(p / rblocks);
    const int x0 = st * DW_STRIP, y0 = rb * DW_ROWS;
    f32x4 acc[DW_ROWS][DW_STRIP];
    dw7_f16_accumulate(a, b, y0, x0, gq, acc);
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r) {
      if (y0 + r >= a.H) continue;
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o)
        if (x0 + o < a.W) {
          const float v[4] = {acc[r][o][0], acc[r][o][1], acc[r][o][2], acc[r][o][3]};
          store4<FMT_F16>(a.dst, (size_t)(b * a.H + y0 + r) * a.W + x0 + o, a.cp, gq * 4, v);
        }
    }
  }
}

// Depthwise 7x7 + LayerNorm in one pass (CNBlock's first two ops in an inference plan: the depthwise output never reaches HBM), as
// dwconv7_ln_kernel: a workgroup owns whole pixels -- spb strips of DW_ROWS x DW_STRIP pixels x all channel quads --, the per-pixel
// moments of the fp32 accumulators are reduced through LDS, 16 lanes per pixel, two passes (mean, then the biased variance about it
// over the TRUE channels).  cp <= 1024.
__global__ __launch_bounds__(256) void dwconv7_ln_f16_kernel(DwConvF16Args a) {
  constexpr int NPIX = DW_ROWS * DW_STRIP;
  __shared__ float red[16 * 256];  // [local strip][pixel][channel quad]: spb * groups <= 256
  __shared__ float stat[2 * 256];  // mean | rstd per (local strip, pixel): spb <= 16
  const int groups = a.cp >> 2;
  const int spb = min(256 / groups, 16);
  const int strips = (a.W + DW_STRIP - 1) / DW_STRIP;
  const int sgroups = (strips + spb - 1) / spb;
  const int rblocks = (a.H + DW_ROWS - 1) / DW_ROWS;
  const int tid = threadIdx.x;
  const int ls = tid / groups, gq = tid - ls * groups;
  int t = blockIdx.x;
  const int sg = t % sgroups;
  t /= sgroups;
  const int rb = t % rblocks;
  const int b = t / rblocks;
  const int st = sg * spb + ls;
  const bool owner = ls < spb;                 // this thread has a (strip, quad) cell of the LDS images
  const bool active = owner && st < strips;
  const int x0 = st * DW_STRIP, y0 = rb * DW_ROWS;
  f32x4 acc[DW_ROWS][DW_STRIP];
  if (active) {
    dw7_f16_accumulate(a, b, y0, x0, gq, acc);
  } else {
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r)
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o) acc[r][o] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  const float inv_c = 1.0f / (float)a.ln_c;
  const int n_items = spb * NPIX;
  auto reduce_items = [&](float* out, bool second) __attribute__((always_inline)) {
    for (int item = tid >> 4; item < n_items; item += 16) {
      const int sub = tid & 15;
      float s = 0.f;
      for (int g = sub; g < groups; g += 16) s += red[item * groups + g];
      s += __shfl_xor(s, 8, 16);
      s += __shfl_xor(s, 4, 16);
      s += __shfl_xor(s, 2, 16);
      s += __shfl_xor(s, 1, 16);
      if (sub == 0) out[item] = second ? 1.0f / sqrtf(s * inv_c + LN_EPS_F16) : s * inv_c;
    }
  };
  if (owner) {
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r)
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o) red[(ls * NPIX + r * DW_STRIP + o) * groups + gq] = (acc[r][o][0] + acc[r][o][1]) + (acc[r][o][2] + acc[r][o][3]);  // pad channels are exact zeros
  }
  __syncthreads();
  reduce_items(stat, false);
  __syncthreads();
  if (owner) {
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r)
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o) {
        const float mean = stat[ls * NPIX + r * DW_STRIP + o];
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float d = acc[r][o][e] - mean;
          ss += (gq * 4 + e < a.ln_c) ? d * d : 0.f;
        }
        red[(ls * NPIX + r * DW_STRIP + o) * groups + gq] = ss;
      }
  }
  __syncthreads();
  reduce_items(stat + 256, true);
  __syncthreads();
  if (active) {
    const bool wok = gq * 4 < a.wcp;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 g = wok ? *reinterpret_cast<const f32x4*>(a.ln_gamma + gq * 4) : zero, bt = wok ? *reinterpret_cast<const f32x4*>(a.ln_beta + gq * 4) : zero;
#pragma unroll
    for (int r = 0; r < DW_ROWS; ++r) {
      if (y0 + r >= a.H) continue;
#pragma unroll
      for (int o = 0; o < DW_STRIP; ++o)
        if (x0 + o < a.W) {
          const float mean = stat[ls * NPIX + r * DW_STRIP + o], rstd = stat[256 + ls * NPIX + r * DW_STRIP + o];
          float y[4];
#pragma unroll
          for (int e = 0; e < 4; ++e) y[e] = (acc[r][o][e] - mean) * rstd * g[e] + bt[e];
          store4<FMT_F16>(a.dst, (size_t)(b * a.H + y0 + r) * a.W + x0 + o, a.cp, gq * 4, y);
        }
    }
  }
}

int launch_dwconv7_f16(const DwConvF16Args& a, hipStream_t s) {
  PH_REQUIRE(a.src && a.w && a.bias && a.dst && a.cp % 32 == 0 && a.wcp % 16 == 0 && a.wcp <= a.cp && a.B > 0 && a.H > 0 && a.W > 0, "dwconv7_f16: bad arguments");
  if (a.ln_gamma) {
    PH_REQUIRE(a.ln_beta && a.ln_c > 0 && a.ln_c <= a.wcp && a.cp <= 1024, "fused fp16 dwconv + LayerNorm: bad arguments");
    const int groups = a.cp >> 2, spb = std::min(256 / groups, 16), strips = (a.W + DW_STRIP - 1) / DW_STRIP;
    const size_t blocks = (size_t)a.B * ((a.H + DW_ROWS - 1) / DW_ROWS) * ((strips + spb - 1) / spb);
    PH_REQUIRE(blocks < ((size_t)1 << 31), "fused fp16 dwconv + LayerNorm: too many workgroups");
    hipLaunchKernelGGL(dwconv7_ln_f16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    PH_HIP_CHECK(hipGetLastError());
    return PH_OK;
  }
  const size_t total = (size_t)a.B * ((a.H + DW_ROWS - 1) / DW_ROWS) * ((a.W + DW_STRIP - 1) / DW_STRIP) * (a.cp / 4);
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 256 * 64);
  hipLaunchKernelGGL(dwconv7_f16_kernel, dim3(blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Standalone LayerNorm over the channel axis (after the stem, in front of a 2x2/stride-2 conv): layernorm_kernel on fp16
// storage.  16 lanes per pixel, 8 channels per load; mean and biased variance in fp32 over the TRUE channel count.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layernorm_f16_kernel(const void* __restrict__ src, const float* __restrict__ gamma, const float* __restrict__ beta, void* __restrict__ dst,
                                                            int c, int wcp, int cp, size_t npix, float eps) {
  const int sub = threadIdx.x & 15;
  const int groups = cp >> 3;
  const float inv_c = 1.0f / (float)c;
  const size_t stride = (size_t)gridDim.x * 16;
  const size_t rounds = (npix + stride - 1) / stride;
  size_t pix = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  for (size_t it = 0; it < rounds; ++it, pix += stride) {
    const bool live = pix < npix;
    const size_t p = live ? pix : npix - 1;
    float v[8];
    float s = 0.f;
    for (int g = sub; g < groups; g += 16) {
      load8<FMT_F16>(src, p, cp, g, v);
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));  // pad channels hold zeros
    }
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    const float mean = s * inv_c;
    float ss = 0.f;
    for (int g = sub; g < groups; g += 16) {
      load8<FMT_F16>(src, p, cp, g, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[e] - mean;
        ss += (8 * g + e < c) ? d * d : 0.f;
      }
    }
    ss += __shfl_xor(ss, 8, 16);
    ss += __shfl_xor(ss, 4, 16);
    ss += __shfl_xor(ss, 2, 16);
    ss += __shfl_xor(ss, 1, 16);
    const float rstd = 1.0f / sqrtf(ss * inv_c + eps);
    if (live) {
      for (int g = sub; g < groups; g += 16) {
        load8<FMT_F16>(src, p, cp, g, v);
        float r[8];
        if (8 * g < wcp) {
          const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + 8 * g), g1 = *reinterpret_cast<const f32x4*>(gamma + 8 * g + 4);
          const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + 8 * g), b1 = *reinterpret_cast<const f32x4*>(beta + 8 * g + 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            r[e] = (v[e] - mean) * rstd * g0[e] + b0[e];
            r[4 + e] = (v[4 + e] - mean) * rstd * g1[e] + b1[e];
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) r[e] = 0.f;
        }
        store8<FMT_F16>(dst, p, cp, g, r);
      }
    }
  }
}

int launch_layernorm_f16(const void* src, const float* gamma, const float* beta, void* dst, int c, int wcp, int cp, size_t npix, hipStream_t s, float eps) {
  PH_REQUIRE(src && gamma && beta && dst && c > 0 && c <= wcp && wcp % 16 == 0 && wcp <= cp && cp % 32 == 0 && npix > 0, "layernorm_f16: bad arguments");
  const int blocks = (int)std::min<size_t>((npix + 15) / 16, 256 * 32);
  hipLaunchKernelGGL(layernorm_f16_kernel, dim3(blocks), dim3(256), 0, s, src, gamma, beta, dst, c, wcp, cp, npix, eps);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Row GEMM on v_mfma_f32_32x32x16_f16.  The weights are the A operand (rows = output channels), the activations the B operand
// (columns = pixels), as in conv3x3_f16_persist_kernel: a lane owns one pixel (lane & 31) and accumulator registers 4q .. 4q + 3
// are the four consecutive output channels 8 q + 4 (lane >> 5) .. + 3 of the 32-channel block -- one 8-byte store each.
//   Both operands come straight from memory in fragment form: the activation fragment of K step s is the 16 bytes
//   [pixel][16 s + 8 (lane >> 5) .. + 7] of the NHWC fp16 tensor, the weight fragment one 16-byte piece of the MFMA-ready image
//   [32-row block][K step][lane][8] (1 KiB per wave instruction, L2-resident).  No LDS: two register stages of fragments, the
//   loads of K step s + 2 are issued behind the MFMAs of step s and land under those of step s + 1 (K steps come in pairs: the
//   padded K is a multiple of 32).
//   Workgroup = 4 waves = 256 pixels x 32 NB output channels; a wave owns 64 pixels x 32 NB channels (2 x NB accumulator tiles).
//   NB = 3 where the 32-channel blocks of N come in threes (96 / 192 / 384 / 768 channels and their 4x hidden widths: one N tile
//   covers a 96-channel layer, so the 4C-wide hidden tensor is read once), else 2 with the last tile's missing block skipped.
//   The N tiles of one pixel tile are neighbours in the grid, so the activation rows are shared through the L2.
//   TAPS 4: Conv2d k2 s2 as the same product over the 2 x 2 gather, K = 4 cinp, tap = 2 dy + dx outermost.
//   M need not be a multiple of the tile (rows past M read row M - 1 and are not stored); K and N are the padded counts.
// ---------------------------------------------------------------------------------------
template <int TAPS, int NB>
__global__ __launch_bounds__(256, 2) void gemm_f16_kernel(GemmF16Args a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lx = lane & 31, lh = lane >> 5;
  const int nblks = a.coutp >> 5;
  const int ntn = (nblks + NB - 1) / NB;
  const int ntile = blockIdx.x % ntn;
  const size_t mtile = blockIdx.x / ntn;
  const int kpt = a.cinp >> 4;  // K steps per tap (even: cinp is a multiple of 32)
  const int ksteps = TAPS * kpt;
  const int nb0 = ntile * NB;
  const _Float16* src = reinterpret_cast<const _Float16*>(a.src);
  size_t row[2], rowoff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    row[i] = mtile * 256 + wave * 64 + i * 32 + lx;
    const size_t m = row[i] < (size_t)a.M ? row[i] : (size_t)a.M - 1;
    if (TAPS == 1) {
      rowoff[i] = m * a.cinp + 8 * lh;
    } else {
      const int OW = a.W >> 1, OH = a.H >> 1;
      const size_t ox = m % OW, t = m / OW;
      const size_t oy = t % OH, b = t / OH;
      rowoff[i] = ((b * a.H + 2 * oy) * a.W + 2 * ox) * a.cinp + 8 * lh;
    }
  }
  bool valid[NB];  // (workgroup-uniform) the tile's n-th 32-channel block exists; a missing one re-reads block nb0 and is neither multiplied nor stored
  const f16x8* wA[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    valid[n] = nb0 + n < nblks;
    wA[n] = reinterpret_cast<const f16x8*>(a.wimg) + (size_t)(valid[n] ? nb0 + n : nb0) * ksteps * 64 + lane;
  }
  f32x16 acc[NB][2];
#pragma unroll
  for (int n = 0; n < NB; ++n)
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][p][r] = 0.f;
  struct Frag {
    f16x8 A[NB], B[2];
  };
  auto load = [&](Frag& f, int step) __attribute__((always_inline)) {
    const int st = step < ksteps ? step : ksteps - 1;  // (past the end: the last step again, in bounds, unused)
    size_t koff;
    if (TAPS == 1) {
      koff = (size_t)st * 16;
    } else {
      const int tap = st / kpt, kc = st - tap * kpt;
      koff = ((size_t)(tap >> 1) * a.W + (tap & 1)) * a.cinp + (size_t)kc * 16;
    }
#pragma unroll
    for (int n = 0; n < NB; ++n) f.A[n] = wA[n][(size_t)st * 64];
#pragma unroll
    for (int p = 0; p < 2; ++p) f.B[p] = *reinterpret_cast<const f16x8*>(src + rowoff[p] + koff);
  };
  auto multiply = [&](const Frag& f) __attribute__((always_inline)) {
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      if (!valid[n]) continue;
#pragma unroll
      for (int p = 0; p < 2; ++p) acc[n][p] = __builtin_amdgcn_mfma_f32_32x32x16_f16(f.A[n], f.B[p], acc[n][p], 0, 0, 0);
    }
  };
  Frag f0, f1;
  load(f0, 0);
  load(f1, 1);
  for (int ks = 0; ks < ksteps; ks += 2) {
    multiply(f0);
    load(f0, ks + 2);
    multiply(f1);
    load(f1, ks + 3);
  }
  // epilogue on the fp32 accumulators: + bias (if any), erf-GELU, (layer scale +) residual; four consecutive channels per 8-byte store
  const _Float16* res = reinterpret_cast<const _Float16*>(a.residual);
#pragma unroll
  for (int n = 0; n < NB; ++n) {
    if (!valid[n]) continue;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c0 = (nb0 + n) * 32 + 8 * q + 4 * lh;
      f32x4 bias = {0.f, 0.f, 0.f, 0.f};  // (no bias: Swin's patch-merging reduction)
      if (a.bias) bias = *reinterpret_cast<const f32x4*>(a.bias + c0);
      f32x4 sc = {1.f, 1.f, 1.f, 1.f};  // (a residual without a layer scale: Swin's attn.proj and mlp.3 -- 1 * v + r is v + r exactly)
      if (a.scale) sc = *reinterpret_cast<const f32x4*>(a.scale + c0);
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        if (row[p] >= (size_t)a.M) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          v[e] = acc[n][p][4 * q + e] + bias[e];
          if (a.gelu) v[e] = gelu_f(v[e]);
        }
        if (res) {
          const f16x4 r = *reinterpret_cast<const f16x4*>(res + row[p] * a.coutp + c0);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = sc[e] * v[e] + (float)r[e];
        }
        store4<FMT_F16>(a.dst, row[p], a.coutp, c0, v);
      }
    }
  }
}

int launch_gemm_f16(const GemmF16Args& a, hipStream_t s) {
  PH_REQUIRE(a.src && a.wimg && a.dst && a.M > 0 && a.cinp > 0 && a.cinp % 32 == 0 && a.coutp > 0 && a.coutp % 32 == 0, "gemm_f16: bad arguments");
  PH_REQUIRE(a.taps == 1 || (a.taps == 4 && a.H >= 2 && a.W >= 2 && a.M % ((a.H / 2) * (a.W / 2)) == 0), "gemm_f16: 1 tap (Linear) or 4 taps (2x2/stride-2 conv over an H x W input)");
  PH_REQUIRE(!a.scale || a.residual, "gemm_f16: a layer scale needs a residual");
  const int nblks = a.coutp / 32, nb = nblks % 3 == 0 ? 3 : 2;
  const size_t blocks = (size_t)((a.M + 255) / 256) * ((nblks + nb - 1) / nb);
  PH_REQUIRE(blocks < ((size_t)1 << 31), "gemm_f16: too many workgroups");
  const dim3 grid((unsigned)blocks);
  if (a.taps == 1 && nb == 3)
    hipLaunchKernelGGL((gemm_f16_kernel<1, 3>), grid, dim3(256), 0, s, a);
  else if (a.taps == 1)
    hipLaunchKernelGGL((gemm_f16_kernel<1, 2>), grid, dim3(256), 0, s, a);
  else if (nb == 3)
    hipLaunchKernelGGL((gemm_f16_kernel<4, 3>), grid, dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((gemm_f16_kernel<4, 2>), grid, dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// fp32 row-GEMM pack (weights.hip: pack_gemm; [n tile of bn][stage = 32-channel slice x taps, taps innermost][piece = n / 8][slot = channel quad ^
// (piece & 1)][row n % 8][4], zero-padded) -> the fp16 image of gemm_f16_kernel.  One thread = one lane's 8 halves of one K step.
__global__ __launch_bounds__(256) void gemm_f16_weight_image_kernel(const float* __restrict__ wpack, f16x8* __restrict__ dst, int cout, int cin, int coutp, int cinp, int taps, int bn) {
  const int kpt = cinp >> 4, ksteps = taps * kpt;
  const size_t total = (size_t)(coutp >> 5) * ksteps * 64;
  const int bp = bn >> 3, slices = cinp >> 5;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int lane = (int)(i & 63);
    size_t t = i >> 6;
    const int ks = (int)(t % ksteps), nblk = (int)(t / ksteps);
    const int n = nblk * 32 + (lane & 31);
    const int tap = ks / kpt, c0 = (ks - tap * kpt) * 16 + 8 * (lane >> 5);
    f16x8 o;
    const int nt = n / bn, nn = n - nt * bn, pb = nn >> 3, r = nn & 7;
    const bool ok = n < cout;  // (rows past cout are the image's zero padding; the pack holds every row below it)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      float v = 0.f;
      if (ok && c < cin) {
        const int slot = ((c & 31) >> 2) ^ (pb & 1);
        v = wpack[((((size_t)nt * slices + (c >> 5)) * taps + tap) * bp + pb) * 256 + slot * 32 + r * 4 + (c & 3)];
      }
      o[j] = (_Float16)v;
    }
    dst[i] = o;
  }
}

int64_t gemm_f16_weight_image_halves(int coutp, int cinp, int taps) { return (int64_t)coutp * cinp * taps; }

int launch_gemm_f16_weight_image(const float* wpack, void* dst, int cout, int cin, int coutp, int cinp, int taps, int bn, hipStream_t s) {
  PH_REQUIRE(wpack && dst && cout > 0 && cin > 0 && coutp % 32 == 0 && cinp % 32 == 0 && cout <= coutp && cin <= cinp && (taps == 1 || taps == 4) && bn >= 8 && bn % 8 == 0,
             "gemm_f16_weight_image: bad arguments");
  const size_t items = (size_t)(coutp / 32) * taps * (cinp / 16) * 64;
  hipLaunchKernelGGL(gemm_f16_weight_image_kernel, dim3((unsigned)std::min<size_t>((items + 255) / 256, 4096)), dim3(256), 0, s, wpack, reinterpret_cast<f16x8*>(dst), cout, cin, coutp,
                     cinp, taps, bn);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Format-generic elementwise ops of the unfused program (8 channels per thread through load8 / store8).
// ---------------------------------------------------------------------------------------
template <int FMT>
__global__ __launch_bounds__(256) void gelu_fmt_kernel(const void* __restrict__ src, void* __restrict__ dst, size_t npix, int cp) {
  const int groups = cp >> 3;
  const size_t total = npix * groups;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int g = (int)(i % groups);
    const size_t pix = i / groups;
    float v[8];
    load8<FMT>(src, pix, cp, g, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = gelu_f(v[e]);
    store8<FMT>(dst, pix, cp, g, v);
  }
}

template <int FMT>
__global__ __launch_bounds__(256) void scale_add_fmt_kernel(const void* __restrict__ src, const void* __restrict__ residual, const float* __restrict__ scale, void* __restrict__ dst,
                                                            size_t npix, int wcp, int cp) {
  const int groups = cp >> 3;
  const size_t total = npix * groups;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int g = (int)(i % groups);
    const size_t pix = i / groups;
    float v[8], r[8];
    load8<FMT>(src, pix, cp, g, v);
    load8<FMT>(residual, pix, cp, g, r);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (8 * g < wcp ? scale[8 * g + e] : 0.f) * v[e] + r[e];
    store8<FMT>(dst, pix, cp, g, v);
  }
}

int launch_gelu_fmt(int fmt, const void* src, void* dst, size_t npix, int cp, hipStream_t s) {
  PH_REQUIRE(src && dst && npix > 0 && cp > 0 && cp % 16 == 0, "gelu_fmt: bad arguments");
  const dim3 grid((unsigned)std::min<size_t>((npix * (cp / 8) + 255) / 256, 256 * 32));
  if (fmt == FMT_F16)
    hipLaunchKernelGGL(gelu_fmt_kernel<FMT_F16>, grid, dim3(256), 0, s, src, dst, npix, cp);
  else if (fmt == FMT_SPLIT)
    hipLaunchKernelGGL(gelu_fmt_kernel<FMT_SPLIT>, grid, dim3(256), 0, s, src, dst, npix, cp);
  else
    hipLaunchKernelGGL(gelu_fmt_kernel<FMT_F32>, grid, dim3(256), 0, s, src, dst, npix, cp);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

int launch_scale_add_fmt(int fmt, const void* src, const void* residual, const float* scale, void* dst, size_t npix, int wcp, int cp, hipStream_t s) {
  PH_REQUIRE(src && residual && scale && dst && npix > 0 && cp > 0 && cp % 16 == 0 && wcp % 8 == 0 && wcp <= cp, "scale_add_fmt: bad arguments");
  const dim3 grid((unsigned)std::min<size_t>((npix * (cp / 8) + 255) / 256, 256 * 32));
  if (fmt == FMT_F16)
    hipLaunchKernelGGL(scale_add_fmt_kernel<FMT_F16>, grid, dim3(256), 0, s, src, residual, scale, dst, npix, wcp, cp);
  else if (fmt == FMT_SPLIT)
    hipLaunchKernelGGL(scale_add_fmt_kernel<FMT_SPLIT>, grid, dim3(256), 0, s, src, residual, scale, dst, npix, wcp, cp);
  else
    hipLaunchKernelGGL(scale_add_fmt_kernel<FMT_F32>, grid, dim3(256), 0, s, src, residual, scale, dst, npix, wcp, cp);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph
