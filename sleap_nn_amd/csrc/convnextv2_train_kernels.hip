// Backward of ConvNeXtV2's Global Response Normalization for gfx950 (MI355X, CDNA4); the forward is convnextv2_kernels.hip.
//
//   forward, per sample b and channel c of the (B, HW, 4C) hidden tensor:
//     s = sum_p x^2,  G = sqrt(s),  D = mean_c G + 1e-6,  N = G / D,  y = w x N + beta + x
//   backward, g = dL/dy:
//     T[b,c]  = sum_p g x                  dbeta[c] = sum_{b,p} g              dw[c] = sum_b T[b,c] N[b,c]
//     dN[b,c] = w[c] T[b,c]                dG[b,c]  = dN[b,c] / D[b] - (sum_c' dN[b,c'] G[b,c']) / (C D[b]^2)
//     K[b,c]  = dG[b,c] / G[b,c] where G > 0, else 0       (d sqrt(s) / dx = x / G; autograd's gradient of a channel that is all zeros is finite: x K = 0 there)
//     dx      = g (1 + w N) + x K
//
// Four launches, shaped as the forward's two.  grn_bwd_reduce_kernel walks the forward's fixed slices (grn_slices) and writes, per (sample, slice, channel), the
// three sums x^2, g x and g -- recomputed from the kept input slot: the forward's slice sums lived in scratch.  grn_bwd_sample_kernel (one workgroup per sample) adds
// the slices in slice order and forms A = 1 + w N, K and the sample's shares of dw and dbeta; grn_bwd_param_kernel adds those shares in sample order;
// grn_bwd_apply_kernel streams x and g once and stores (or, where the source slot already holds a gradient, adds) dx = g A + x K.  Plain stores, no atomics, every
// addition in an order fixed by the shape: two backward passes over one input are bit-identical and a sample's dx does not depend on the batch around it.  Every
// load and store of the two streaming kernels is a float4 of a contiguous run of channels.  Pad channels (c >= C): A = K = 0, so dx is zero there whatever g holds.
//
// Scratch (floats): sums [B][slices][3][cp] | A [B][cp] | K [B][cp] | dw shares [B][cp] | dbeta shares [B][cp]   (grn_bwd_scratch_floats)
#include <algorithm>

#include "common.h"
#include "net_kernels.h"
#include "train_kernels.h"

namespace ph {

typedef float f32x4 __attribute__((ext_vector_type(4)));

int64_t grn_bwd_scratch_floats(int B, int HW, int cp) { return (int64_t)B * grn_slices(HW) * 3 * cp + (int64_t)4 * B * cp; }

// A workgroup owns (slice, sample, chunk of <= 256 channel quads); thread (r, q) adds quad q over the slice's pixels r, r + rows, ...; row 0 adds the rows in row order.
__global__ __launch_bounds__(256) void grn_bwd_reduce_kernel(const float* __restrict__ x, const float* __restrict__ g, float* __restrict__ sums, int HW, int cp, int slice_px, int nslices) {
  __shared__ f32x4 sh[3][256];
  const int G = cp >> 2;
  const int slice = blockIdx.x, b = blockIdx.y, q0 = blockIdx.z * 256;
  const int gc = min(256, G - q0);
  const int rows = 256 / gc;
  const int tid = threadIdx.x, r = tid / gc, q = tid - r * gc;
  const int p0 = slice * slice_px, p1 = min(HW, p0 + slice_px);
  f32x4 sxx = {0.f, 0.f, 0.f, 0.f}, sgx = sxx, sg = sxx;
  if (r < rows) {
    const size_t off = (size_t)b * HW * cp + (size_t)(q0 + q) * 4;
    const float* xb = x + off;
    const float* gb = g + off;
    // two pixels (four loads) in flight per thread, two partial sums of each kind: the order of the additions is a function of the shape alone
    f32x4 bxx = sxx, bgx = sxx, bg = sxx;
    int p = p0 + r;
    for (; p + rows < p1; p += 2 * rows) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(xb + (size_t)p * cp);
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gb + (size_t)p * cp);
      const f32x4 x1 = *reinterpret_cast<const f32x4*>(xb + (size_t)(p + rows) * cp);
      const f32x4 g1 = *reinterpret_cast<const f32x4*>(gb + (size_t)(p + rows) * cp);
      sxx += x0 * x0;
      sgx += g0 * x0;
      sg += g0;
      bxx += x1 * x1;
      bgx += g1 * x1;
      bg += g1;
    }
    for (; p < p1; p += rows) {
      const f32x4 x0 = *reinterpret_cast<const f32x4*>(xb + (size_t)p * cp);
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gb + (size_t)p * cp);
      sxx += x0 * x0;
      sgx += g0 * x0;
      sg += g0;
    }
    sxx += bxx;
    sgx += bgx;
    sg += bg;
  }
  sh[0][tid] = sxx;
  sh[1][tid] = sgx;
  sh[2][tid] = sg;
  __syncthreads();
  if (r == 0) {
    for (int k = 1; k < rows; ++k) {
      sxx += sh[0][k * gc + q];
      sgx += sh[1][k * gc + q];
      sg += sh[2][k * gc + q];
    }
    float* dst = sums + ((size_t)b * nslices + slice) * 3 * cp + (size_t)(q0 + q) * 4;
    *reinterpret_cast<f32x4*>(dst) = sxx;
    *reinterpret_cast<f32x4*>(dst + cp) = sgx;
    *reinterpret_cast<f32x4*>(dst + 2 * cp) = sg;
  }
}

// One workgroup per sample.  Both block sums (sum_c G and sum_c dN G) run over a thread's channels c = tid, tid + 256, ... and then a fixed tree.
__global__ __launch_bounds__(256) void grn_bwd_sample_kernel(const float* __restrict__ sums, const float* __restrict__ weight, float* __restrict__ coefA, float* __restrict__ coefK,
                                                             float* __restrict__ dw_share, float* __restrict__ db_share, int c, int cp, int nslices) {
  __shared__ float red[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* sb = sums + (size_t)b * nslices * 3 * cp;
  float sumG = 0.f, sumDG = 0.f;
  for (int ch = tid; ch < c; ch += 256) {
    float sxx = sb[ch], sgx = sb[cp + ch];
    for (int k = 1; k < nslices; ++k) {
      sxx += sb[(size_t)k * 3 * cp + ch];
      sgx += sb[(size_t)k * 3 * cp + cp + ch];
    }
    const float Gc = sqrtf(sxx);
    sumG += Gc;
    sumDG += weight[ch] * sgx * Gc;
  }
  red[tid] = sumG;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const float D = red[0] / (float)c + 1e-6f;
  __syncthreads();
  red[tid] = sumDG;
  __syncthreads();
  for (int d = 128; d >= 1; d >>= 1) {
    if (tid < d) red[tid] += red[tid + d];
    __syncthreads();
  }
  const float cross = red[0] / ((float)c * D * D);
  for (int ch = tid; ch < cp; ch += 256) {
    float A = 0.f, K = 0.f, dws = 0.f, dbs = 0.f;
    if (ch < c) {
      float sxx = sb[ch], sgx = sb[cp + ch], sgg = sb[2 * cp + ch];  // the same order as above: the same G
      for (int k = 1; k < nslices; ++k) {
        sxx += sb[(size_t)k * 3 * cp + ch];
        sgx += sb[(size_t)k * 3 * cp + cp + ch];
        sgg += sb[(size_t)k * 3 * cp + 2 * cp + ch];
      }
      const float Gc = sqrtf(sxx), w = weight[ch];
      const float N = Gc / D;
      const float dG = w * sgx / D - cross;
      A = 1.0f + w * N;
      K = Gc > 0.f ? dG / Gc : 0.f;
      dws = sgx * N;
      dbs = sgg;
    }
    coefA[(size_t)b * cp + ch] = A;
    coefK[(size_t)b * cp + ch] = K;
    dw_share[(size_t)b * cp + ch] = dws;
    db_share[(size_t)b * cp + ch] = dbs;
  }
}

// dw[c] = sum_b dw_share[b][c], dbeta[c] likewise, in sample order; one thread per true channel.
__global__ __launch_bounds__(256) void grn_bwd_param_kernel(const float* __restrict__ dw_share, const float* __restrict__ db_share, float* __restrict__ gw, float* __restrict__ gb, int B, int c, int cp) {
  const int ch = blockIdx.x * 256 + threadIdx.x;
  if (ch >= c) return;
  float w = dw_share[ch], bb = db_share[ch];
  for (int b = 1; b < B; ++b) {
    w += dw_share[(size_t)b * cp + ch];
    bb += db_share[(size_t)b * cp + ch];
  }
  gw[ch] = w;
  gb[ch] = bb;
}

// A workgroup owns (slice, sample): dx = g A[b] + x K[b] over its pixels, float4 per thread, channels fastest.  A and K are cp floats each per sample and every
// thread re-reads them with the period of the channel count: they stay in the CU's cache beside the two streams.
__global__ __launch_bounds__(256) void grn_bwd_apply_kernel(const float* __restrict__ x, const float* __restrict__ g, const float* __restrict__ coefA, const float* __restrict__ coefK,
                                                            float* __restrict__ gx, int HW, int cp, int slice_px, int accumulate) {
  const int G = cp >> 2;
  const int slice = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int p0 = slice * slice_px, p1 = min(HW, p0 + slice_px);
  const size_t base = ((size_t)b * HW + p0) * cp;
  const float* A = coefA + (size_t)b * cp;
  const float* K = coefK + (size_t)b * cp;
  const int total = (p1 - p0) * G;
  int q = tid % G;  // channel quad of element e = tid + 256 k: advanced by 256 mod G per step, as the forward's apply pass does
  const int dq = 256 % G;
#pragma unroll 4
  for (int e = tid; e < total; e += 256) {
    const f32x4 xv = *reinterpret_cast<const f32x4*>(x + base + (size_t)e * 4);
    const f32x4 gv = *reinterpret_cast<const f32x4*>(g + base + (size_t)e * 4);
    const f32x4 a = *reinterpret_cast<const f32x4*>(A + q * 4);
    const f32x4 k = *reinterpret_cast<const f32x4*>(K + q * 4);
    f32x4 out = gv * a + xv * k;
    float* dst = gx + base + (size_t)e * 4;
    if (accumulate) out += *reinterpret_cast<const f32x4*>(dst);
    *reinterpret_cast<f32x4*>(dst) = out;
    q += dq;
    q -= q >= G ? G : 0;
  }
}

int launch_grn_bwd(const GrnBwdArgs& a, hipStream_t s) {
  PH_REQUIRE(a.x && a.gy && a.gx && a.weight && a.gw && a.gb && a.scratch, "launch_grn_bwd: null argument");
  PH_REQUIRE(a.B > 0 && a.B <= 65535 && a.HW > 0 && a.c > 0 && a.c <= a.cp && (a.cp & 15) == 0 && a.cp <= 15360, "launch_grn_bwd: bad shape (B %d, HW %d, C %d / %d)", a.B, a.HW, a.c, a.cp);
  PH_REQUIRE((int64_t)a.HW * (a.cp >> 2) < ((int64_t)1 << 31), "launch_grn_bwd: a sample has 2^31 channel quads or more");
  const int slice_px = grn_slice_pixels(a.HW), nslices = grn_slices(a.HW);
  const int chunks = ((a.cp >> 2) + 255) / 256;
  float* sums = a.scratch;
  float* coefA = sums + (size_t)a.B * nslices * 3 * a.cp;
  float* coefK = coefA + (size_t)a.B * a.cp;
  float* dws = coefK + (size_t)a.B * a.cp;
  float* dbs = dws + (size_t)a.B * a.cp;
  hipLaunchKernelGGL(grn_bwd_reduce_kernel, dim3(nslices, a.B, chunks), dim3(256), 0, s, a.x, a.gy, sums, a.HW, a.cp, slice_px, nslices);
  PH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(grn_bwd_sample_kernel, dim3(a.B), dim3(256), 0, s, sums, a.weight, coefA, coefK, dws, dbs, a.c, a.cp, nslices);
  PH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(grn_bwd_param_kernel, dim3((a.c + 255) / 256), dim3(256), 0, s, dws, dbs, a.gw, a.gb, a.B, a.c, a.cp);
  PH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(grn_bwd_apply_kernel, dim3(nslices, a.B), dim3(256), 0, s, a.x, a.gy, coefA, coefK, a.gx, a.HW, a.cp, slice_px, a.accumulate);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph
