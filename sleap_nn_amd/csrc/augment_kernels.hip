// Training augmentation on the device: intensity (uniform / Gaussian noise, contrast, brightness), left/right flip,
// affine warp with anti-aliased frame coverage, and random erase, for a whole batch in one image launch.
//
// Replaces the per-sample CPU skia stage of the reference (sleap_nn/data/skia_augmentation.py:
// apply_intensity_augmentation_skia, apply_flip_augmentation_skia, apply_geometric_augmentation_skia, called at
// data/custom_datasets.py:1101-1117).  The per-sample scalars are drawn on the host in the reference's order
// (sleap_nn_amd/data/augmentation.py); this file only applies them.  Per output pixel (x, y) of sample b, channel c:
//   * warp samples: q = minv (x + 0.5, y + 0.5) (flip folded into minv as x -> W - x), bilinear clamp-to-edge sample of
//     the intensity-augmented source at q - 0.5 (index coordinates), times the area of the pixel square inside the
//     mapped frame rectangle M [0,W]x[0,H] (skia's anti-aliased drawImage over a black clear), rounded to nearest;
//   * other samples are copied (reversed along x under a flip), so they stay bit-exact;
//   * the erase rectangle is filled last.
// The intensity of a source pixel is a function of (sample, channel, source y, source x) only -- the noise comes from a
// counter-based hash keyed by (seed, sample, channel, y, x) -- so the fused launch equals an intensity launch followed by
// a geometric one.
//
// Layout: one 256-thread workgroup per (64 x 32 output tile, sample); each thread owns 4 adjacent pixels of two rows
// (one 4-byte / 16-byte store per row and channel).  Warp tiles first map their corners through minv: a tile whose
// source footprint misses the frame is written as zeros without a load; otherwise the clamped source box is staged
// into LDS (intensity applied while staging, so every source pixel's noise / LUT is computed once) when it fits the
// budget, and sampled straight from global memory when it does not (extreme zoom-out).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

namespace ph {

namespace {

constexpr int AUG_TX = 64, AUG_TY = 32, AUG_THREADS = 256;
constexpr int AUG_LDS = 20480;  // bytes of one staged source channel (5 workgroups per CU fit the 160 KiB LDS)

__device__ __forceinline__ uint32_t mix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x7feb352dU;
  x ^= x >> 15;
  x *= 0x846ca68bU;
  x ^= x >> 16;
  return x;
}

__device__ __forceinline__ uint32_t noise_key(uint32_t seed, int b, int c, int y, int x, uint32_t salt) {
  uint32_t h = mix32(seed ^ salt);
  h = mix32(h ^ (uint32_t)b);
  h = mix32(h ^ (uint32_t)c);
  h = mix32(h ^ (uint32_t)y);
  return mix32(h ^ (uint32_t)x);
}

// (0, 1] from 24 random bits
__device__ __forceinline__ float unit_open0(uint32_t h) { return ((float)(h >> 8) + 1.0f) * (1.0f / 16777216.0f); }

// the intensity chain of one source value, in the reference's order: uniform noise, Gaussian noise, contrast, brightness
__device__ __forceinline__ int intensity(int v, const ph_aug_sample& s, int b, int c, int y, int x) {
#pragma clang fp contract(off)
  const int f = s.flags;
  if (f & PH_AUG_UNIFORM) {
    const uint32_t span = (uint32_t)(s.uni_hi - s.uni_lo + 1);
    const int n = s.uni_lo + (int)(noise_key(s.seed, b, c, y, x, 0x2545F491U) % span);
    v = min(max(v + n, 0), 255);
  }
  if (f & PH_AUG_GAUSS) {
    const uint32_t h1 = noise_key(s.seed, b, c, y, x, 0x9E3779B9U);
    const uint32_t h2 = mix32(h1 ^ 0x68E31DA4U);
    const float r = sqrtf(-2.0f * logf(unit_open0(h1)));
    const float z = r * cospif(2.0f * ((float)(h2 >> 8) * (1.0f / 16777216.0f)));
    float g = s.gauss_mean + s.gauss_std * z;
    g = fminf(fmaxf(g, -32768.0f), 32767.0f);
    v = min(max(v + (int)g, 0), 255);  // (int) truncates toward zero, like astype(int16)
  }
  if (f & PH_AUG_CONTRAST) {
    float t = ((float)v - 127.5f) * s.contrast;
    t = t + 127.5f;
    v = (int)fminf(fmaxf(t, 0.0f), 255.0f);
  }
  if (f & PH_AUG_BRIGHTNESS) {
    const float t = (float)v * s.brightness;
    v = (int)fminf(fmaxf(t, 0.0f), 255.0f);
  }
  return v;
}

template <typename T>
__device__ __forceinline__ int load_q(const T* p) {
  if constexpr (sizeof(T) == 1) {
    return (int)*p;
  } else {
    const float q = fminf(fmaxf(*p * 255.0f, 0.0f), 255.0f);  // (x * 255).astype(uint8)
    return (int)q;
  }
}

// area of the unit pixel square [px, px+1] x [py, py+1] inside the half-planes (edge k: n.p + d >= 0) marked in `partial`
// (Sutherland-Hodgman: a square clipped by four lines has at most 8 vertices; one out-of-line copy, edge pixels only)
__device__ __noinline__ float clipped_area(float px, float py, float e0, float e1, float e2, float e3, float e4, float e5, float e6, float e7, float e8,
                                           float e9, float e10, float e11, int partial) {
  const float e[12] = {e0, e1, e2, e3, e4, e5, e6, e7, e8, e9, e10, e11};
  constexpr int NV = 9;
  float vx[NV], vy[NV];
  vx[0] = px; vy[0] = py;
  vx[1] = px + 1.0f; vy[1] = py;
  vx[2] = px + 1.0f; vy[2] = py + 1.0f;
  vx[3] = px; vy[3] = py + 1.0f;
  int n = 4;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!(partial & (1 << k))) continue;
    const float nx = e[3 * k], ny = e[3 * k + 1], d = e[3 * k + 2];
    float ox[NV], oy[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) ox[j] = oy[j] = 0.0f;
    int m = 0;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      if (i < n) {
        const int i2 = (i + 1 == n) ? 0 : i + 1;
        float ax = vx[i], ay = vy[i], bx = 0.0f, by = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j)
          if (j == i2) { bx = vx[j]; by = vy[j]; }
        const float da = nx * ax + ny * ay + d, db = nx * bx + ny * by + d;
        const bool ina = da >= 0.0f, inb = db >= 0.0f;
        // static-index writes (selects) keep the polygon in registers
        if (ina) {
#pragma unroll
          for (int j = 0; j < NV; ++j)
            if (j == m) { ox[j] = ax; oy[j] = ay; }
          m = min(m + 1, NV - 1);
        }
        if (ina != inb) {
          const float t = da / (da - db);
          const float cx = ax + t * (bx - ax), cy = ay + t * (by - ay);
#pragma unroll
          for (int j = 0; j < NV; ++j)
            if (j == m) { ox[j] = cx; oy[j] = cy; }
          m = min(m + 1, NV - 1);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < NV; ++j) { vx[j] = ox[j]; vy[j] = oy[j]; }
    n = m;
  }
  if (n < 3) return 0.0f;
  float a = 0.0f;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    if (i < n) {
      const int i2 = (i + 1 == n) ? 0 : i + 1;
      float bx = 0.0f, by = 0.0f;
#pragma unroll
      for (int j = 0; j < NV; ++j)
        if (j == i2) { bx = vx[j]; by = vy[j]; }
      a += vx[i] * by - bx * vy[i];
    }
  }
  return fminf(fmaxf(0.5f * fabsf(a), 0.0f), 1.0f);
}

// coverage of output pixel (x, y) by the mapped frame rectangle
__device__ __forceinline__ float coverage(int x, int y, const ph_aug_sample& s) {
  const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
  int partial = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float nx = s.edge[3 * k], ny = s.edge[3 * k + 1];
    const float dist = nx * cx + ny * cy + s.edge[3 * k + 2];
    const float half = 0.5f * (fabsf(nx) + fabsf(ny));
    if (dist <= -half) return 0.0f;
    if (dist < half) partial |= 1 << k;
  }
  if (!partial) return 1.0f;
  // clip in pixel-local coordinates (the square [0,1]^2): the shoelace sum of frame-sized coordinates would cancel
  float dl[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) dl[k] = s.edge[3 * k] * (float)x + s.edge[3 * k + 1] * (float)y + s.edge[3 * k + 2];
  return clipped_area(0.0f, 0.0f, s.edge[0], s.edge[1], dl[0], s.edge[3], s.edge[4], dl[1], s.edge[6], s.edge[7], dl[2], s.edge[9], s.edge[10], dl[3], partial);
}

// four uint8 results packed little-endian (pixel x0 + j in byte j) -> one 4-byte (uint8) or 16-byte (float) store
template <typename T>
__device__ __forceinline__ void store4(T* row, int x, int W, uint32_t v, bool vec) {
  if constexpr (sizeof(T) == 1) {
    if (vec) {
      *reinterpret_cast<uint32_t*>(row + x) = v;
      return;
    }
    for (int j = 0; j < 4; ++j)
      if (x + j < W) row[x + j] = (T)((v >> (8 * j)) & 255);
  } else {
    const float f0 = (float)(v & 255) / 255.0f, f1 = (float)((v >> 8) & 255) / 255.0f, f2 = (float)((v >> 16) & 255) / 255.0f, f3 = (float)(v >> 24) / 255.0f;
    if (vec) {
      *reinterpret_cast<float4*>(row + x) = make_float4(f0, f1, f2, f3);
      return;
    }
    const float f[4] = {f0, f1, f2, f3};
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (x + j < W) row[x + j] = f[j];
  }
}

template <typename T>
__global__ __launch_bounds__(AUG_THREADS) void augment_image_kernel(const T* __restrict__ src, T* __restrict__ dst, int C, int H, int W, int tiles_x,
                                                                    const ph_aug_sample* __restrict__ params, int vec_ok, int* __restrict__ counters) {
  __shared__ uint8_t stage[AUG_LDS];
  const int b = blockIdx.y;
  const ph_aug_sample s = params[b];
  const int x0 = (blockIdx.x % tiles_x) * AUG_TX, y0 = (blockIdx.x / tiles_x) * AUG_TY;
  const int tid = threadIdx.x;
  const int lx = (tid & 15) * 4, ly = (tid >> 4) * 2;  // 4 pixels x 2 rows per thread
  const bool vec = vec_ok && (x0 + lx + 4 <= W);
  const size_t plane = (size_t)H * W;
  const bool flip = s.flags & PH_AUG_FLIP;
  const bool erase = s.flags & PH_AUG_ERASE;

  if (!(s.flags & PH_AUG_WARP)) {  // copy path (reversed along x under a flip)
    if (tid == 0 && counters) atomicAdd(&counters[0], 1);
    for (int c = 0; c < C; ++c) {
      const T* sp = src + ((size_t)b * C + c) * plane;
      T* dp = dst + ((size_t)b * C + c) * plane;
      const int fill = c == 0 ? s.fill[0] : (c == 1 ? s.fill[1] : s.fill[2]);
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const int y = y0 + ly + r;
        if (y >= H) continue;
        uint32_t packed = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int x = x0 + lx + j;
          const int sx = flip ? W - 1 - x : x;
          int v = 0;
          if (x < W) v = intensity(load_q(sp + (size_t)y * W + sx), s, b, c, y, sx);
          if (erase && y >= s.erase_y && y < s.erase_y + s.erase_h && x >= s.erase_x && x < s.erase_x + s.erase_w) v = fill;
          packed |= (uint32_t)v << (8 * j);
        }
        store4(dp + (size_t)y * W, x0 + lx, W, packed, vec);
      }
    }
    return;
  }

  // source footprint of the tile: the corners of its pixel squares through minv (pixel coordinates)
  float qx_lo = INFINITY, qx_hi = -INFINITY, qy_lo = INFINITY, qy_hi = -INFINITY;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float px = (float)(x0 + ((k & 1) ? AUG_TX : 0)), py = (float)(y0 + ((k & 2) ? AUG_TY : 0));
    const float qx = s.minv[0] * px + s.minv[1] * py + s.minv[2], qy = s.minv[3] * px + s.minv[4] * py + s.minv[5];
    qx_lo = fminf(qx_lo, qx); qx_hi = fmaxf(qx_hi, qx);
    qy_lo = fminf(qy_lo, qy); qy_hi = fmaxf(qy_hi, qy);
  }
  const bool outside = qx_hi < -1.0f || qy_hi < -1.0f || qx_lo > (float)W + 1.0f || qy_lo > (float)H + 1.0f;
  // clamped index box of every bilinear tap of the tile (one texel of slack against rounding)
  const int bx0 = min(max((int)floorf(qx_lo - 0.5f) - 1, 0), W - 1), bx1 = min(max((int)floorf(qx_hi - 0.5f) + 2, 0), W - 1);
  const int by0 = min(max((int)floorf(qy_lo - 0.5f) - 1, 0), H - 1), by1 = min(max((int)floorf(qy_hi - 0.5f) + 2, 0), H - 1);
  const int bw = bx1 - bx0 + 1, bh = by1 - by0 + 1;
  const bool staged = !outside && (long)bw * bh <= AUG_LDS;
  if (tid == 0 && counters) atomicAdd(&counters[outside ? 1 : (staged ? 2 : 3)], 1);

  for (int c = 0; c < C; ++c) {
    const T* sp = src + ((size_t)b * C + c) * plane;
    T* dp = dst + ((size_t)b * C + c) * plane;
    const int fill = c == 0 ? s.fill[0] : (c == 1 ? s.fill[1] : s.fill[2]);
    if (staged) {
      __syncthreads();  // the previous channel's reads are done
      // each wave takes every fourth row; 8 rows x 2 column chunks per step keep 16 loads in flight per lane
      const int wave = tid >> 6, lane = tid & 63;
      for (int c0 = 0; c0 < bw; c0 += 128) {
        for (int r0 = wave; r0 < bh; r0 += 32) {
          int val[8][2];
#pragma unroll
          for (int ru = 0; ru < 8; ++ru)
#pragma unroll
            for (int cu = 0; cu < 2; ++cu) {
              const int r = r0 + 4 * ru, i = c0 + lane + 64 * cu;
              val[ru][cu] = (r < bh && i < bw) ? load_q(sp + (size_t)(by0 + r) * W + bx0 + i) : 0;
            }
#pragma unroll
          for (int ru = 0; ru < 8; ++ru)
#pragma unroll
            for (int cu = 0; cu < 2; ++cu) {
              const int r = r0 + 4 * ru, i = c0 + lane + 64 * cu;
              if (r < bh && i < bw) stage[r * bw + i] = (uint8_t)intensity(val[ru][cu], s, b, c, by0 + r, bx0 + i);
            }
        }
      }
      __syncthreads();
    }
    // not unrolled: the gather path inlines the intensity chain four times per pixel
#pragma unroll 1
    for (int r = 0; r < 2; ++r) {
      const int y = y0 + ly + r;
      if (y >= H) continue;
      uint32_t packed = 0;
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        const int x = x0 + lx + j;
        int out = 0;
        const float cov = (outside || x >= W) ? 0.0f : coverage(x, y, s);
        if (cov > 0.0f) {
          const float cx = (float)x + 0.5f, cy = (float)y + 0.5f;
          const float u = s.minv[0] * cx + s.minv[1] * cy + s.minv[2] - 0.5f;
          const float w = s.minv[3] * cx + s.minv[4] * cy + s.minv[5] - 0.5f;
          const float fu = floorf(u), fw = floorf(w);
          const float fx = u - fu, fy = w - fw;
          const int xa = min(max((int)fu, 0), W - 1), xb = min(max((int)fu + 1, 0), W - 1);
          const int ya = min(max((int)fw, 0), H - 1), yb = min(max((int)fw + 1, 0), H - 1);
          int v00, v01, v10, v11;
          if (staged) {
            const int ca = min(max(xa - bx0, 0), bw - 1), cb = min(max(xb - bx0, 0), bw - 1);
            const int ra = min(max(ya - by0, 0), bh - 1), rb = min(max(yb - by0, 0), bh - 1);
            v00 = stage[ra * bw + ca]; v01 = stage[ra * bw + cb];
            v10 = stage[rb * bw + ca]; v11 = stage[rb * bw + cb];
          } else {
            v00 = intensity(load_q(sp + (size_t)ya * W + xa), s, b, c, ya, xa);
            v01 = intensity(load_q(sp + (size_t)ya * W + xb), s, b, c, ya, xb);
            v10 = intensity(load_q(sp + (size_t)yb * W + xa), s, b, c, yb, xa);
            v11 = intensity(load_q(sp + (size_t)yb * W + xb), s, b, c, yb, xb);
          }
          const float top = (float)v00 + fx * (float)(v01 - v00);
          const float bot = (float)v10 + fx * (float)(v11 - v10);
          const float val = (top + fy * (bot - top)) * cov;
          out = min(max((int)floorf(val + 0.5f), 0), 255);
        }
        if (erase && y >= s.erase_y && y < s.erase_y + s.erase_h && x >= s.erase_x && x < s.erase_x + s.erase_w) out = fill;
        packed |= (uint32_t)out << (8 * j);
      }
      store4(dp + (size_t)y * W, x0 + lx, W, packed, vec);
    }
  }
}

// one thread per (sample, instance, node): pair swap and mirror under a flip, then the skia matrix
__global__ __launch_bounds__(256) void augment_points_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int I, int N, int W,
                                                             const ph_aug_sample* __restrict__ params, const int32_t* __restrict__ pairs, int n_pairs) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= B * I * N) return;
  const int n = idx % N, bi = idx / N, b = bi / I;
  const ph_aug_sample& s = params[b];
  int src_n = n;
  if (s.flags & PH_AUG_FLIP)  // the swaps run in order, so the source slot is found by undoing them from the last one
    for (int k = n_pairs - 1; k >= 0; --k) {
      const int pa = pairs[2 * k], pb = pairs[2 * k + 1];
      if (pa < 0 || pb < 0 || pa >= N || pb >= N) continue;  // out-of-range pairs are ignored, never followed
      if (src_n == pa) src_n = pb;
      else if (src_n == pb) src_n = pa;
    }
  float x = in[((size_t)bi * N + src_n) * 2], y = in[((size_t)bi * N + src_n) * 2 + 1];
  if (s.flags & PH_AUG_FLIP) x = (float)(W - 1) - x;
  if (s.flags & PH_AUG_WARP) {
    const float nx = s.m[0] * x + s.m[1] * y + s.m[2];
    const float ny = s.m[3] * x + s.m[4] * y + s.m[5];
    x = nx;
    y = ny;
  }
  out[(size_t)idx * 2] = x;
  out[(size_t)idx * 2 + 1] = y;
}

bool overlaps(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return pa < pb + nb && pb < pa + na;
}

}  // namespace

}  // namespace ph

extern "C" int32_t ph_aug_sample_size(void) { return (int32_t)sizeof(ph_aug_sample); }

extern "C" int ph_augment(const void* src_dev, void* dst_dev, int32_t dtype, int32_t B, int32_t C, int32_t H, int32_t W, const float* kp_in_dev, float* kp_out_dev,
                          int32_t I, int32_t N, const ph_aug_sample* params_dev, const int32_t* sym_pairs_dev, int32_t n_pairs, int32_t* counters_dev, void* stream) {
  using namespace ph;
  PH_REQUIRE(src_dev && dst_dev && params_dev, "ph_augment: null image or parameter pointer");
  PH_REQUIRE(dtype == 0 || dtype == 1, "ph_augment: dtype must be 0 (uint8) or 1 (float32), got %d", dtype);
  PH_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, "ph_augment: bad shape B=%d H=%d W=%d", B, H, W);
  PH_REQUIRE(C == 1 || C == 3, "ph_augment: images must have 1 or 3 channels, got %d", C);
  const size_t esz = dtype == 0 ? 1 : 4;
  const size_t img_bytes = (size_t)B * C * H * W * esz;
  PH_REQUIRE(!overlaps(src_dev, img_bytes, dst_dev, img_bytes), "ph_augment: source and destination images overlap");
  PH_REQUIRE((kp_in_dev == nullptr) == (kp_out_dev == nullptr), "ph_augment: keypoints need both an input and an output");
  if (kp_in_dev) {
    PH_REQUIRE(I >= 0 && N >= 0, "ph_augment: bad keypoint shape I=%d N=%d", I, N);
    const size_t kp_bytes = (size_t)B * I * N * 2 * sizeof(float);
    PH_REQUIRE(kp_bytes == 0 || !overlaps(kp_in_dev, kp_bytes, kp_out_dev, kp_bytes), "ph_augment: keypoint input and output overlap");
    PH_REQUIRE(n_pairs >= 0 && (n_pairs == 0 || sym_pairs_dev), "ph_augment: %d symmetric pairs without a pair array", n_pairs);
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int tiles_x = (W + AUG_TX - 1) / AUG_TX, tiles_y = (H + AUG_TY - 1) / AUG_TY;
  PH_REQUIRE((long)tiles_x * tiles_y <= 0x7fffffffL, "ph_augment: frame too large");
  const dim3 grid((unsigned)(tiles_x * tiles_y), (unsigned)B);
  const int vec_ok = (W % 4 == 0) && (((uintptr_t)dst_dev & (dtype == 0 ? 3 : 15)) == 0);
  if (dtype == 0)
    hipLaunchKernelGGL(augment_image_kernel<uint8_t>, grid, dim3(AUG_THREADS), 0, s, static_cast<const uint8_t*>(src_dev), static_cast<uint8_t*>(dst_dev), C, H, W, tiles_x,
                       params_dev, vec_ok, counters_dev);
  else
    hipLaunchKernelGGL(augment_image_kernel<float>, grid, dim3(AUG_THREADS), 0, s, static_cast<const float*>(src_dev), static_cast<float*>(dst_dev), C, H, W, tiles_x,
                       params_dev, vec_ok, counters_dev);
  PH_HIP_CHECK(hipGetLastError());
  const long npts = kp_in_dev ? (long)B * I * N : 0;
  if (npts > 0) {
    hipLaunchKernelGGL(augment_points_kernel, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0, s, kp_in_dev, kp_out_dev, B, I, N, W, params_dev, sym_pairs_dev, n_pairs);
    PH_HIP_CHECK(hipGetLastError());
  }
  return PH_OK;
}
