// Training targets of the segmentation model types, rendered on the device from instance masks (C ABI: ph_render_seg_targets).
//
// Replaces the per-frame CPU code of the reference's dataset (sleap_nn/data/segmentation_maps.py: generate_foreground_mask,
// generate_center_heatmap, generate_center_offsets, _compute_mask_centroids, as called at data/custom_datasets.py:3593-3626):
//   * seg_mask_stats_kernel: a workgroup per (frame, instance slot) sums x, y and the pixel count of its mask in 64-bit integers
//     (exact, so the order of the reduction does not matter), divides once in fp64 and rounds to fp32 -- the value the reference
//     gets from numpy's float64 mean when torch takes it into fp32 arithmetic.  An empty mask gets the image centre.
//   * seg_render_kernel: a thread per output cell of one frame (blockIdx.y), grid-stride over the cells.  The cell's window is
//     that of adaptive_avg_pool2d (what F.interpolate(mode="area") runs): [floor(i H / out), ceil((i + 1) H / out)), not uniform
//     when the stride does not divide the size.  "area average > 0.5" is decided on integers, 2 count > window: the fp32 quotient
//     count / n differs from 1/2 by at least 1 / (2 n) whenever 2 count != n, far above its rounding error, so both decide alike.
//     Foreground: pixels of the window in the union of the frame's masks.  Offsets: one pass over the instances keeps the winner
//     among those covering more than half of the window -- smallest full-resolution area, the higher index among equal areas,
//     which is what the reference's stable descending sort followed by in-order overwriting leaves -- so no sort and no
//     per-instance map exists.  Centre map: max over the instances of the Gaussian, every operation rounded on its own.
// Slots at or beyond n_instances[b] are never read.  Bounds: window rows / columns are < H / W by the ceil formula (i < out), a
// mask index is < B I H W, an output index < B h w (times the caller's batch stride), both in 64 bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace ph {

namespace {

__device__ __forceinline__ unsigned long long block_sum_256_u64(unsigned long long v, unsigned long long* red /* >= 4 */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  const unsigned long long t = red[0] + red[1] + red[2] + red[3];
  __syncthreads();
  return t;
}

// grid (I, B)
__global__ __launch_bounds__(256) void seg_mask_stats_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ n_inst, int I, int H, int W,
                                                             float* __restrict__ centroids /* B,I,2 */, long long* __restrict__ areas /* B,I */) {
  __shared__ unsigned long long red[4];
  const int i = blockIdx.x, b = blockIdx.y;
  const size_t slot = (size_t)b * I + i;
  if (i >= n_inst[b]) {  // padding (workgroup-uniform): the mask is not read
    if (threadIdx.x == 0) {
      centroids[2 * slot] = NAN;
      centroids[2 * slot + 1] = NAN;
      areas[slot] = 0;
    }
    return;
  }
  const uint8_t* m = masks + slot * (size_t)H * W;
  const size_t n = (size_t)H * W;
  unsigned long long sx = 0, sy = 0, cnt = 0;
  for (size_t p = threadIdx.x; p < n; p += 256) {
    if (m[p]) {
      sx += (unsigned long long)(p % W);
      sy += (unsigned long long)(p / W);
      cnt += 1;
    }
  }
  sx = block_sum_256_u64(sx, red);
  sy = block_sum_256_u64(sy, red);
  cnt = block_sum_256_u64(cnt, red);
  if (threadIdx.x == 0) {
    centroids[2 * slot] = cnt ? (float)((double)sx / (double)cnt) : (float)((double)W / 2.0);
    centroids[2 * slot + 1] = cnt ? (float)((double)sy / (double)cnt) : (float)((double)H / 2.0);
    areas[slot] = (long long)cnt;
  }
}

// grid (blocks, B); a thread owns cells p, p + gridDim.x * 256, ... of frame blockIdx.y
__global__ __launch_bounds__(256) void seg_render_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ n_inst, int I, int H, int W, int h, int w, int stride,
                                                         float denom /* 2 (sigma stride)^2 */, int maxpool, const float* __restrict__ centroids, const long long* __restrict__ areas,
                                                         float* __restrict__ fg, float* __restrict__ center, float* __restrict__ offsets, long long off_bs,
                                                         float* __restrict__ weight, long long wt_bs) {
  const int b = blockIdx.y;
  const int n = min(max(n_inst[b], 0), I);
  const int plane = h * w;
  const uint8_t* mb = masks + (size_t)b * I * H * W;
  const float* cb = centroids + (size_t)b * I * 2;
  const long long* ab = areas + (size_t)b * I;
  const float half = (float)stride / 2.0f;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < plane; p += gridDim.x * 256) {
    const int oy = p / w, ox = p - oy * w;
    const int y0 = (int)(((long long)oy * H) / h), y1 = (int)((((long long)oy + 1) * H + h - 1) / h);
    const int x0 = (int)(((long long)ox * W) / w), x1 = (int)((((long long)ox + 1) * W + w - 1) / w);
    const int win = (y1 - y0) * (x1 - x0);
    const float gx = (float)(ox * stride) + half, gy = (float)(oy * stride) + half;
    if (fg) {
      int cnt = 0;
      for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
          const size_t q = (size_t)y * W + x;
          int any = 0;
          for (int i = 0; i < n && !any; ++i) any = mb[(size_t)i * H * W + q] != 0;
          cnt += any;
        }
      fg[(size_t)b * plane + p] = (maxpool ? cnt > 0 : 2 * cnt > win) ? 1.0f : 0.0f;
    }
    if (center) {
      float best = 0.0f;
      for (int i = 0; i < n; ++i) {
        const float dx = __fsub_rn(gx, cb[2 * i]), dy = __fsub_rn(gy, cb[2 * i + 1]);
        const float d2 = __fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy));
        best = fmaxf(best, expf(__fdiv_rn(-d2, denom)));
      }
      center[(size_t)b * plane + p] = best;
    }
    if (offsets) {
      int win_i = -1;
      long long win_area = 0;
      for (int i = 0; i < n; ++i) {
        const uint8_t* mi = mb + (size_t)i * H * W;
        int cnt = 0;
        for (int y = y0; y < y1; ++y)
          for (int x = x0; x < x1; ++x) cnt += mi[(size_t)y * W + x] != 0;
        if (2 * cnt > win && (win_i < 0 || ab[i] <= win_area)) {  // <=: among equal areas the later instance overwrites
          win_i = i;
          win_area = ab[i];
        }
      }
      float* ob = offsets + (size_t)b * off_bs;
      ob[p] = win_i >= 0 ? __fsub_rn(cb[2 * win_i], gx) : 0.0f;
      ob[(size_t)plane + p] = win_i >= 0 ? __fsub_rn(cb[2 * win_i + 1], gy) : 0.0f;
      weight[(size_t)b * wt_bs + p] = win_i >= 0 ? 1.0f : 0.0f;
    }
  }
}

}  // namespace
}  // namespace ph

using namespace ph;

extern "C" int ph_render_seg_targets(const uint8_t* masks_dev, const int32_t* n_instances_dev, int32_t B, int32_t I, int32_t H, int32_t W, int32_t output_stride,
                                     float sigma, int32_t maxpool, int32_t compute_stats, float* centroids_dev, int64_t* areas_dev, float* fg_dev, float* center_dev,
                                     float* offsets_dev, int64_t offsets_batch_stride, float* weight_dev, int64_t weight_batch_stride, void* stream) {
  PH_REQUIRE(n_instances_dev && centroids_dev && areas_dev, "ph_render_seg_targets: null argument");
  PH_REQUIRE(B > 0 && B <= 65535 && I >= 0 && I <= 65535 && H > 0 && W > 0 && (int64_t)H * W < (int64_t)1 << 31, "ph_render_seg_targets: bad shape (%d, %d, %d, %d)", B, I, H, W);
  PH_REQUIRE(I == 0 || masks_dev, "ph_render_seg_targets: null masks");
  PH_REQUIRE(output_stride >= 1 && H / output_stride >= 1 && W / output_stride >= 1, "ph_render_seg_targets: output stride %d does not fit (%d, %d)", output_stride, H, W);
  PH_REQUIRE((offsets_dev == nullptr) == (weight_dev == nullptr), "ph_render_seg_targets: offsets and weight come together");
  const int h = H / output_stride, w = W / output_stride;
  PH_REQUIRE(!offsets_dev || (offsets_batch_stride >= (int64_t)2 * h * w && weight_batch_stride >= (int64_t)h * w), "ph_render_seg_targets: batch strides smaller than a sample");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const double ss = (double)sigma * (double)output_stride;
  const float denom = (float)(2.0 * ss * ss);  // the reference's Python float 2 * scaled_sigma ** 2, taken into fp32 arithmetic
  PH_REQUIRE(!center_dev || denom > 0.f, "ph_render_seg_targets: sigma must be positive");
  if (compute_stats && I > 0)
    hipLaunchKernelGGL(seg_mask_stats_kernel, dim3(I, B), dim3(256), 0, s, masks_dev, n_instances_dev, I, H, W, centroids_dev, reinterpret_cast<long long*>(areas_dev));
  if (fg_dev || center_dev || offsets_dev) {
    const unsigned blocks = (unsigned)std::min(((int64_t)h * w + 255) / 256, (int64_t)32);
    hipLaunchKernelGGL(seg_render_kernel, dim3(blocks, B), dim3(256), 0, s, masks_dev, n_instances_dev, I, H, W, h, w, output_stride, denom, maxpool ? 1 : 0, centroids_dev,
                       reinterpret_cast<const long long*>(areas_dev), fg_dev, center_dev, offsets_dev, (long long)offsets_batch_stride, weight_dev,
                       (long long)weight_batch_stride);
  }
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
