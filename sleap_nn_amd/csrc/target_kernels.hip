// Training targets of the identity and top-down model types, rendered on the device.
//
// Replaces the per-sample CPU code of the reference's datasets (sleap_nn/data/identity.py:34-137 generate_class_maps,
// sleap_nn/data/instance_centroids.py:7-98 generate_centroids) by one launch per batch each:
//   * render_class_maps_kernel: a workgroup belongs to ONE frame (blockIdx.y) and stages that frame's points (I, N, 2) and
//     class-weight matrix (C, I) in LDS once; a thread then owns output pixels of the frame and makes two sweeps over the
//     instances.  Sweep 1 sums the per-instance maps M_i into S; sweep 2 walks the weight matrix row by row and, for every
//     non-zero weight, recomputes M_i and folds weight * (M_i > threshold ? M_i / S : 0) into the row's maximum.  Nothing of
//     size (I, h, w) exists anywhere, and no per-thread array is indexed at run time (which hipcc would put in scratch): the
//     second sweep costs VALU work only, because every LDS read is the same address in all lanes (a broadcast, no bank
//     conflict), and with one-hot weights it evaluates at most I instances whatever C is.
//     M_i is the maximum over the nodes of exp(-d^2 / (2 (sigma * stride)^2)) with NaN counted as 0.  It is computed as exp of
//     the MINIMUM non-NaN d^2: one transcendental per instance and sweep instead of N, the same value wherever expf is monotone
//     and within one ulp of it otherwise.
//   * instance_centroids_kernel: a thread per instance; the anchor node when it is fully visible (copied bit for bit), else the
//     per-axis NaN-ignoring mean, summed in the order of the host's torch sum, else NaN.
// Writes are coalesced (consecutive threads own consecutive pixels of a plane).  Bounds: a pixel index is < h * w, a point index
// < I * N * 2 and a weight index < C * I by construction of the loops; the LDS size is checked against 64 KiB at the entry point.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "common.h"

namespace ph {

// the per-instance map of instance i at grid point (gx, gy): s_pts = this frame's (I, N, 2) points in LDS
__device__ __forceinline__ float instance_map(const float* __restrict__ s_pts, int i, int N, float gx, float gy, float inv) {
  float dmin = INFINITY;
  const float* p = s_pts + (size_t)i * N * 2;
  for (int n = 0; n < N; ++n) {
    const float dx = gx - p[2 * n], dy = gy - p[2 * n + 1];
    const float d = dx * dx + dy * dy;
    if (d == d) dmin = fminf(dmin, d);  // a NaN coordinate: the node contributes 0 (nan_to_num), i.e. never the maximum
  }
  return dmin < INFINITY ? expf(-dmin * inv) : 0.f;
}

__global__ __launch_bounds__(256) void render_class_maps_kernel(const float* __restrict__ pts /* B,I,N,2 */, const float* __restrict__ weights /* B,C,I */, int I, int N,
                                                                int C, int h, int w, int stride, float sigma, float threshold, float* __restrict__ out /* B,C,h,w */) {
  extern __shared__ float s_mem[];
  float* s_pts = s_mem;                      // I * N * 2
  float* s_w = s_mem + (size_t)I * N * 2;    // C * I
  const int b = blockIdx.y;
  const int n_pts = I * N * 2, n_w = C * I;
  for (int t = threadIdx.x; t < n_pts; t += 256) s_pts[t] = pts[(size_t)b * n_pts + t];
  for (int t = threadIdx.x; t < n_w; t += 256) s_w[t] = weights[(size_t)b * n_w + t];
  __syncthreads();
  const float inv = 1.0f / (2.0f * sigma * sigma);
  const int plane = h * w;
  float* o = out + (size_t)b * C * plane;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < plane; p += gridDim.x * 256) {
    const float gx = (float)((p % w) * stride), gy = (float)((p / w) * stride);
    float S = 0.f;
    for (int i = 0; i < I; ++i) S += instance_map(s_pts, i, N, gx, gy, inv);
    for (int c = 0; c < C; ++c) {
      float best = 0.f;
      for (int i = 0; i < I; ++i) {
        const float wt = s_w[c * I + i];
        if (wt == 0.f) continue;
        const float m = instance_map(s_pts, i, N, gx, gy, inv);
        // m > threshold >= 0 implies S >= m > 0: the division is never 0 / 0
        if (m > threshold) best = fmaxf(best, wt * (m / S));
      }
      o[(size_t)c * plane + p] = best;
    }
  }
}

// One of the partial sums of a torch CPU sum over a strided row (ATen's cascade: 16 terms are summed in order, the chunk is folded into
// the next level, and so on every 256 and 4096 terms), so that the mean below rounds as the host's does.
struct CascadeSum {
  float l0 = 0.f, l1 = 0.f, l2 = 0.f, l3 = 0.f;
  int i = 0;
  __device__ __forceinline__ void add(float v) {
    l0 += v;
    if ((++i & 15) == 0) {
      l1 += l0, l0 = 0.f;
      if ((i & 0xf0) == 0) {
        l2 += l1, l1 = 0.f;
        if ((i & 0xf00) == 0) l3 += l2, l2 = 0.f;
      }
    }
  }
  __device__ __forceinline__ float total() const { return ((l0 + l1) + l2) + l3; }
};

__global__ __launch_bounds__(256) void instance_centroids_kernel(const float* __restrict__ pts /* n,N,2 */, int64_t n, int N, int anchor, float* __restrict__ out /* n,2 */) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* p = pts + (size_t)i * N * 2;
  if (anchor >= 0) {
    const float ax = p[2 * anchor], ay = p[2 * anchor + 1];
    if (ax == ax && ay == ay) {
      out[2 * i] = ax;
      out[2 * i + 1] = ay;
      return;
    }
  }
  // The sum of the present coordinates in the order of torch's CPU sum over the node axis: four interleaved partial sums (node index
  // mod 4), the N % 4 last nodes added to the first, then the four added up.  A missing coordinate is a zero term, as in the reference.
  CascadeSum sx[4], sy[4];
  int cx = 0, cy = 0;
  const int q = N / 4;
  for (int g = 0; g < q; ++g) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float x = p[2 * (4 * g + k)], y = p[2 * (4 * g + k) + 1];
      sx[k].add(x == x ? x : 0.f);
      sy[k].add(y == y ? y : 0.f);
      cx += x == x;
      cy += y == y;
    }
  }
  float tx = sx[0].total(), ty = sy[0].total();
  for (int k = 4 * q; k < N; ++k) {
    const float x = p[2 * k], y = p[2 * k + 1];
    tx += x == x ? x : 0.f;
    ty += y == y ? y : 0.f;
    cx += x == x;
    cy += y == y;
  }
#pragma unroll
  for (int k = 1; k < 4; ++k) tx += sx[k].total(), ty += sy[k].total();
  const bool none = cx == 0 && cy == 0;  // no node with any coordinate
  out[2 * i] = none ? NAN : tx / (float)max(cx, 1);
  out[2 * i + 1] = none ? NAN : ty / (float)max(cy, 1);
}

}  // namespace ph

using namespace ph;

extern "C" int ph_render_class_maps(const float* points_dev, const float* weights_dev, int32_t B, int32_t I, int32_t N, int32_t C, int32_t img_h, int32_t img_w,
                                    int32_t stride, float sigma, float threshold, float* out_dev, void* stream) {
  PH_REQUIRE(out_dev && B > 0 && I >= 0 && N > 0 && C > 0 && img_h > 0 && img_w > 0 && stride > 0, "ph_render_class_maps: bad arguments B=%d I=%d N=%d C=%d %dx%d stride %d",
             B, I, N, C, img_h, img_w, stride);
  PH_REQUIRE(I == 0 || (points_dev && weights_dev), "ph_render_class_maps: null pointer");
  PH_REQUIRE(threshold >= 0.f, "ph_render_class_maps: threshold must be >= 0 (got %g): below it an empty pixel would be 0 / 0", (double)threshold);
  PH_REQUIRE(B <= 65535, "ph_render_class_maps: at most 65535 frames per launch (got %d)", B);
  const int h = (img_h + stride - 1) / stride, w = (img_w + stride - 1) / stride;  // len(arange(0, size, stride))
  PH_REQUIRE((int64_t)h * w <= 0x7fffffffLL - 256 * 65536LL, "ph_render_class_maps: grid of %d x %d points is too large", h, w);
  const int64_t lds_floats = (int64_t)I * N * 2 + (int64_t)C * I;
  PH_REQUIRE(lds_floats * 4 <= 64 * 1024, "ph_render_class_maps: a frame's points and weights (I=%d N=%d C=%d: %lld bytes) exceed the 64 KiB of LDS staged per workgroup", I, N, C,
             (long long)(lds_floats * 4));
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const int plane = h * w;
  const int per_frame = std::max(1, (cus * 8 + B - 1) / B);  // about 8 workgroups of 4 waves per CU over the batch, grid-stride beyond
  const unsigned gx = (unsigned)std::min((plane + 255) / 256, std::min(per_frame, 65536));
  hipLaunchKernelGGL(render_class_maps_kernel, dim3(gx, (unsigned)B), dim3(256), (size_t)lds_floats * 4, static_cast<hipStream_t>(stream), points_dev, weights_dev, I, N, C, h,
                     w, stride, sigma * (float)stride, threshold, out_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

extern "C" int ph_instance_centroids(const float* points_dev, int64_t n, int32_t N, int32_t anchor_ind, float* out_dev, void* stream) {
  PH_REQUIRE(n >= 0 && N > 0 && anchor_ind < N, "ph_instance_centroids: bad arguments n=%lld N=%d anchor_ind=%d", (long long)n, N, anchor_ind);
  if (n == 0) return PH_OK;
  PH_REQUIRE(points_dev && out_dev, "ph_instance_centroids: null pointer");
  PH_REQUIRE(n <= 0x7fffffffLL * 256, "ph_instance_centroids: too many instances (%lld)", (long long)n);
  hipLaunchKernelGGL(instance_centroids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), points_dev, n, N, anchor_ind, out_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
