// Pyramidal Lucas-Kanade optical flow for the flow-shift tracker (sleap_nn/tracking/tracker.py:631-841, which calls OpenCV's calcOpticalFlowPyrLK once per
// past frame of the window for every new frame and rebuilds both pyramids on the host each time).  The definition of every number here is
// sleap_nn_amd/tracking/flow.py pyr_lk (its docstring); DESIGN.md section 4.2g.
//   * flow_pyr_down_kernel: one level from the one below, a thread per output pixel: [1 4 6 4 1] x [1 4 6 4 1] at (2x, 2y), reflect-101, (sum + 128) >> 8.
//     Integer sums: bit-identical to the CPU levels.  One launch per level for all frames of a batch.
//   * flow_track_kernel: grid (points of a job, jobs), ONE WAVE per point, through all of its levels.  Per level the (win + 3)^2 uint8 patch of the reference
//     level lands in LDS (reflect-101), the Scharr derivatives of its (win + 1)^2 inner positions are computed from it into LDS (zero outside the image: no
//     derivative planes in memory), then the fixed-point I / Ix / Iy windows (int16, LDS) and the normal matrix (integer lane sums, a 64-bit butterfly).  Every
//     iteration stages the (win + 1)^2 patch of the current level into LDS, samples J, and reduces the two mismatch sums the same way.  All lanes hold the same
//     reduced integers, so every branch is uniform; float32 arithmetic in the CPU function's order with contraction off; lane 0 stores the result.
//     LDS 19.1 KB per workgroup (one wave), no atomics, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)  // the float32 recurrence is stated operation by operation (flow.py): no fused multiply-add

namespace ph {

constexpr int kFlowMinWin = 3;
constexpr int kFlowMaxWin = 41;
constexpr int kFlowLevels = PH_FLOW_MAX_LEVELS;

struct FlowLevels {
  int n;
  int h[kFlowLevels], w[kFlowLevels];
};

__host__ __device__ inline int reflect101(int i, int n) {  // (n >= 2; |i| stays within a few n: the bounds tests see to it)
  while ((unsigned)i >= (unsigned)n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}

static int flow_levels(int H, int W, int win, int max_level, FlowLevels* out) {
  PH_REQUIRE(win >= kFlowMinWin && win <= kFlowMaxWin, "ph_flow: win=%d must lie in [%d, %d]", win, kFlowMinWin, kFlowMaxWin);
  PH_REQUIRE(max_level >= 0 && max_level < kFlowLevels, "ph_flow: max_level=%d must lie in [0, %d]", max_level, kFlowLevels - 1);
  PH_REQUIRE(H >= 2 && W >= 2 && (int64_t)H * W <= 0x7fffffffLL, "ph_flow: bad frame size %d x %d (sides of at least 2, below 2^31 pixels)", H, W);
  out->n = 1;
  out->h[0] = H, out->w[0] = W;
  while (out->n - 1 < max_level) {
    const int h = (out->h[out->n - 1] + 1) / 2, w = (out->w[out->n - 1] + 1) / 2;
    if (w <= win || h <= win) break;
    out->h[out->n] = h, out->w[out->n] = w;
    ++out->n;
  }
  return PH_OK;
}

__global__ __launch_bounds__(256) void flow_pyr_down_kernel(const uint8_t* __restrict__ src, int64_t src_stride, int sh, int sw, uint8_t* __restrict__ dst,
                                                            int64_t dst_stride, int dh, int dw) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  const int y = blockIdx.y * 4 + threadIdx.y;
  if (x >= dw || y >= dh) return;
  const uint8_t* s = src + (size_t)blockIdx.z * src_stride;
  int cx[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) cx[d] = reflect101(2 * x + d - 2, sw);
  const int k[5] = {1, 4, 6, 4, 1};
  int sum = 0;
#pragma unroll
  for (int dy = 0; dy < 5; ++dy) {
    const uint8_t* row = s + (size_t)reflect101(2 * y + dy - 2, sh) * sw;
    int r = 0;
#pragma unroll
    for (int dx = 0; dx < 5; ++dx) r += k[dx] * (int)row[cx[dx]];
    sum += k[dy] * r;
  }
  dst[(size_t)blockIdx.z * dst_stride + (size_t)y * dw + x] = (uint8_t)((sum + 128) >> 8);
}

__device__ inline long long wave_sum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ inline int floor_to_int(float v) { return (int)fminf(fmaxf(floorf(v), -1.0e9f), 1.0e9f); }
__device__ inline int round_to_int(float v) { return (int)fminf(fmaxf(rintf(v), -1.0e9f), 1.0e9f); }
__device__ inline bool flow_outside(int ix, int iy, int w, int h, int win) { return ix < -win || ix >= w || iy < -win || iy >= h; }

struct FlowWeights {
  int w00, w01, w10, w11;
};
__device__ inline FlowWeights flow_weights(float a, float b) {
  FlowWeights q;
  q.w00 = (int)rintf((1.f - a) * (1.f - b) * 16384.f);
  q.w01 = (int)rintf(a * (1.f - b) * 16384.f);
  q.w10 = (int)rintf((1.f - a) * b * 16384.f);
  q.w11 = 16384 - q.w00 - q.w01 - q.w10;
  return q;
}

constexpr int kWinArea = kFlowMaxWin * kFlowMaxWin;
constexpr int kDerArea = (kFlowMaxWin + 1) * (kFlowMaxWin + 1);
constexpr int kRawArea = (kFlowMaxWin + 3) * (kFlowMaxWin + 3);

__global__ __launch_bounds__(64) void flow_track_kernel(const ph_flow_job* __restrict__ jobs, const float* __restrict__ points, int n_points, FlowLevels lv, int win,
                                                        int max_iter, double eps2, float* __restrict__ shifted, uint8_t* __restrict__ status) {
  __shared__ int16_t sI[kWinArea], sIx[kWinArea], sIy[kWinArea];
  __shared__ int16_t sDx[kDerArea], sDy[kDerArea];
  __shared__ uint8_t sRaw[kRawArea];
  const int lane = threadIdx.x;
  const ph_flow_job* job = jobs + blockIdx.y;
  const int pt_begin = job->pt_begin, pt_end = job->pt_end;
  if (pt_begin < 0 || pt_end > n_points || pt_end <= pt_begin || blockIdx.x >= (unsigned)(pt_end - pt_begin)) return;  // (uniform over the wave; the outputs were preset to lost)
  const int pt = pt_begin + (int)blockIdx.x;
  const float px = points[(size_t)2 * pt], py = points[(size_t)2 * pt + 1];
  if (isnan(px) || isnan(py)) return;

  const float half = (float)(win - 1) * 0.5f;
  const int n_win = win * win;
  const int step_y = 64 / win, step_x = 64 % win;  // a lane's next pixel, 64 further along the window
  const int x_first = lane % win, y_first = lane / win;
  float nx = 0.f, ny = 0.f;
  bool found = true;

  for (int l = lv.n - 1; l >= 0; --l) {
    const int h = lv.h[l], w = lv.w[l];
    const float sc = 1.f / (float)(1 << l);
    const float pvx = px * sc, pvy = py * sc;
    if (l == lv.n - 1) {
      nx = pvx, ny = pvy;
    } else {
      nx = nx * 2.f, ny = ny * 2.f;
    }
    const float wx = pvx - half, wy = pvy - half;
    const int ix = floor_to_int(wx), iy = floor_to_int(wy);
    if (flow_outside(ix, iy, w, h, win)) {
      if (l == 0) found = false;
      continue;
    }
    const FlowWeights q = flow_weights(wx - (float)ix, wy - (float)iy);

    // the reference level's patch, one pixel of margin for the Scharr taps and one more for the bilinear corner
    const uint8_t* ref = job->ref[l];
    const int rs = win + 3, ds = win + 1;
    __syncthreads();
    for (int i = lane; i < rs * rs; i += 64) {
      const int ry = i / rs, rx = i - ry * rs;
      sRaw[i] = ref[(size_t)reflect101(iy - 1 + ry, h) * w + reflect101(ix - 1 + rx, w)];
    }
    __syncthreads();
    for (int i = lane; i < ds * ds; i += 64) {
      const int y = i / ds, x = i - y * ds;
      int gx = 0, gy = 0;
      if (ix + x >= 0 && ix + x < w && iy + y >= 0 && iy + y < h) {  // outside the image the derivatives are 0
        const uint8_t* r0 = sRaw + y * rs + x;  // raw (x + 1, y + 1) is the centre
        const uint8_t* r1 = r0 + rs;
        const uint8_t* r2 = r1 + rs;
        gx = 3 * ((int)r0[2] + (int)r2[2]) + 10 * (int)r1[2] - 3 * ((int)r0[0] + (int)r2[0]) - 10 * (int)r1[0];
        gy = 3 * ((int)r2[0] + (int)r2[2]) + 10 * (int)r2[1] - 3 * ((int)r0[0] + (int)r0[2]) - 10 * (int)r0[1];
      }
      sDx[i] = (int16_t)gx;
      sDy[i] = (int16_t)gy;
    }
    __syncthreads();
    int a11 = 0, a12 = 0, a22 = 0;  // a lane's share: at most 27 products below 2^24.1
    for (int p = lane, x = x_first, y = y_first; p < n_win; p += 64) {
      const uint8_t* r = sRaw + (y + 1) * rs + x + 1;
      const int iv = ((int)r[0] * q.w00 + (int)r[1] * q.w01 + (int)r[rs] * q.w10 + (int)r[rs + 1] * q.w11 + 256) >> 9;
      const int d = y * ds + x;
      const int gx = ((int)sDx[d] * q.w00 + (int)sDx[d + 1] * q.w01 + (int)sDx[d + ds] * q.w10 + (int)sDx[d + ds + 1] * q.w11 + 8192) >> 14;
      const int gy = ((int)sDy[d] * q.w00 + (int)sDy[d + 1] * q.w01 + (int)sDy[d + ds] * q.w10 + (int)sDy[d + ds + 1] * q.w11 + 8192) >> 14;
      sI[p] = (int16_t)iv, sIx[p] = (int16_t)gx, sIy[p] = (int16_t)gy;
      a11 += gx * gx, a12 += gx * gy, a22 += gy * gy;
      x += step_x, y += step_y;
      if (x >= win) x -= win, ++y;
    }
    const float scale = 1.f / (float)(1 << 20);
    const float A11 = (float)wave_sum((long long)a11) * scale;
    const float A12 = (float)wave_sum((long long)a12) * scale;
    const float A22 = (float)wave_sum((long long)a22) * scale;
    const float D = A11 * A22 - A12 * A12;
    const float dif = A11 - A22;
    const float min_eig = (A22 + A11 - sqrtf(dif * dif + 4.f * A12 * A12)) / (float)(2 * win * win);
    if ((double)min_eig < 1e-4 || D < 1.1920928955078125e-7f) {
      if (l == 0) found = false;
      continue;
    }
    const float Dinv = 1.f / D;

    const uint8_t* cur = job->cur[l];
    float wnx = nx - half, wny = ny - half;
    float pdx = 0.f, pdy = 0.f;
    for (int j = 0; j < max_iter; ++j) {
      const int jx = floor_to_int(wnx), jy = floor_to_int(wny);
      if (flow_outside(jx, jy, w, h, win)) {
        if (l == 0) found = false;
        break;
      }
      const FlowWeights u = flow_weights(wnx - (float)jx, wny - (float)jy);
      __syncthreads();
      for (int i = lane; i < ds * ds; i += 64) {
        const int ry = i / ds, rx = i - ry * ds;
        sRaw[i] = cur[(size_t)reflect101(jy + ry, h) * w + reflect101(jx + rx, w)];
      }
      __syncthreads();
      int b1 = 0, b2 = 0;  // at most 27 products below 2^25
      for (int p = lane, x = x_first, y = y_first; p < n_win; p += 64) {
        const uint8_t* r = sRaw + y * ds + x;
        const int jv = ((int)r[0] * u.w00 + (int)r[1] * u.w01 + (int)r[ds] * u.w10 + (int)r[ds + 1] * u.w11 + 256) >> 9;
        const int diff = jv - (int)sI[p];
        b1 += diff * (int)sIx[p], b2 += diff * (int)sIy[p];
        x += step_x, y += step_y;
        if (x >= win) x -= win, ++y;
      }
      const float fb1 = (float)wave_sum((long long)b1) * scale;
      const float fb2 = (float)wave_sum((long long)b2) * scale;
      const float dx = (A12 * fb2 - A22 * fb1) * Dinv;
      const float dy = (A12 * fb1 - A11 * fb2) * Dinv;
      wnx = wnx + dx, wny = wny + dy;
      nx = wnx + half, ny = wny + half;
      if ((double)dx * (double)dx + (double)dy * (double)dy <= eps2) break;
      if (j > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) {
        nx = nx - dx * 0.5f, ny = ny - dy * 0.5f;
        break;
      }
      pdx = dx, pdy = dy;
    }
  }
  if (found && flow_outside(round_to_int(nx - half), round_to_int(ny - half), lv.w[0], lv.h[0], win)) found = false;
  if (found && lane == 0) {
    shifted[(size_t)2 * pt] = nx;
    shifted[(size_t)2 * pt + 1] = ny;
    status[pt] = 1;
  }
}

}  // namespace ph

extern "C" int ph_flow_job_size(void) { return (int)sizeof(ph_flow_job); }

extern "C" int ph_flow_levels(int32_t H, int32_t W, int32_t win, int32_t max_level, int32_t* sizes) {
  ph::FlowLevels lv;
  if (int rc = ph::flow_levels(H, W, win, max_level, &lv); rc != PH_OK) return rc;
  if (sizes)
    for (int l = 0; l < lv.n; ++l) sizes[2 * l] = lv.h[l], sizes[2 * l + 1] = lv.w[l];
  return lv.n;
}

extern "C" int ph_flow_pyramid(const uint8_t* frames_dev, int32_t B, int32_t H, int32_t W, int32_t win, int32_t max_level, uint8_t* out_dev, int64_t out_bytes,
                               void* stream) {
  using namespace ph;
  FlowLevels lv;
  if (int rc = flow_levels(H, W, win, max_level, &lv); rc != PH_OK) return rc;
  PH_REQUIRE(frames_dev && B >= 1 && B <= 65535, "ph_flow_pyramid: null frames or B=%d outside [1, 65535]", B);
  int64_t S = 0;
  for (int l = 1; l < lv.n; ++l) S += (int64_t)lv.h[l] * lv.w[l];
  PH_REQUIRE(out_bytes >= (int64_t)B * S && (S == 0 || out_dev), "ph_flow_pyramid: out_dev holds %lld bytes, %d frames of %lld needed", (long long)out_bytes, B,
             (long long)S);
  hipStream_t s = static_cast<hipStream_t>(stream);
  int64_t off = 0;  // of level l inside a frame's record
  for (int l = 1; l < lv.n; ++l) {
    const uint8_t* src = l == 1 ? frames_dev : out_dev + (off - (int64_t)lv.h[l - 1] * lv.w[l - 1]);
    const int64_t src_stride = l == 1 ? (int64_t)H * W : S;
    const dim3 grid((unsigned)((lv.w[l] + 63) / 64), (unsigned)((lv.h[l] + 3) / 4), (unsigned)B);
    hipLaunchKernelGGL(flow_pyr_down_kernel, grid, dim3(64, 4), 0, s, src, src_stride, lv.h[l - 1], lv.w[l - 1], out_dev + off, S, lv.h[l], lv.w[l]);
    off += (int64_t)lv.h[l] * lv.w[l];
  }
  PH_HIP_CHECK(hipGetLastError());
  return lv.n;
}

extern "C" int ph_flow_track(const ph_flow_job* jobs_dev, int32_t n_jobs, int32_t max_job_points, const float* points_dev, int32_t n_points, int32_t H, int32_t W,
                             int32_t win, int32_t max_level, int32_t max_iter, double eps, float* shifted_dev, uint8_t* status_dev, void* stream) {
  using namespace ph;
  FlowLevels lv;
  if (int rc = flow_levels(H, W, win, max_level, &lv); rc != PH_OK) return rc;
  PH_REQUIRE(jobs_dev && points_dev && shifted_dev && status_dev, "ph_flow_track: null pointer");
  PH_REQUIRE(n_jobs >= 1 && n_jobs <= 65535 && max_job_points >= 1 && n_points >= 1 && n_points <= 0x3fffffff,
             "ph_flow_track: n_jobs=%d (1..65535), max_job_points=%d (>= 1), n_points=%d (1..2^30 - 1)", n_jobs, max_job_points, n_points);
  PH_REQUIRE(max_iter >= 1 && max_iter <= 100 && eps > 0 && eps <= 10, "ph_flow_track: max_iter=%d must lie in [1, 100] and eps=%g in (0, 10]", max_iter, eps);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PH_HIP_CHECK(hipMemsetAsync(shifted_dev, 0xff, sizeof(float) * 2 * (size_t)n_points, s));  // all bits set: NaN
  PH_HIP_CHECK(hipMemsetAsync(status_dev, 0, (size_t)n_points, s));
  hipLaunchKernelGGL(flow_track_kernel, dim3((unsigned)max_job_points, (unsigned)n_jobs), dim3(64), 0, s, jobs_dev, points_dev, n_points, lv, win, max_iter, eps * eps,
                     shifted_dev, status_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
