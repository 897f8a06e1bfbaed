// Cross-frame mask tracking: the weighted contingency tables of a batch of label maps against earlier label maps.
//
// Replaces the host work of mask tracking in the reference (sleap_nn/tracking/utils.py:127-244: every mask decoded to the image grid by
// decode_mask_to_image_res, then one crop AND per (current mask, candidate mask) pair, over a window of 25 frames by default).  The label map of a bottom-up
// segmentation frame is already on the device (ph_seg_assign / ph_seg_gate), so the intersections of ALL (label of frame b, label of the frame k calls
// earlier) pairs are one pass per (b, k): a cell (v, u) whose labels are (a, c) adds row_weight[v] * col_weight[u] to bin [a][c].  The weights are the image
// rows / columns a cell row / column stands for under the nearest resample to the image grid (separable, the integer rule of ph_seg_place_crops; 0 in the
// padding), so the sums are exactly the image-grid pixel counts.
//   * track_mask_pairs_kernel: grid (chunks, L, B).  A thread owns kCells consecutive cells of a map row and folds equal (a, c) neighbours into a run; a run
//     bumps the workgroup's private LDS table (P * P bins, 16 KB at P = 64, and P area bins) with integer LDS atomics; background cells cost nothing.  The
//     table is flushed once per workgroup with global integer atomics, zero bins skipped.  The areas of frame b are summed by the lag-1 workgroups only.
//     Integer sums only: exact, and the same in every run and on any stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace ph {

constexpr int kTrackMaxLabels = 64;
constexpr int kTrackMaxLags = 32;
constexpr int kCells = 8;  // cells per thread and step, along a row

template <typename LabelT>
__global__ __launch_bounds__(256) void track_mask_pairs_kernel(const LabelT* __restrict__ labels, const LabelT* __restrict__ hist, int B, int h, int w, int L, int n_hist,
                                                               const int32_t* __restrict__ row_weight, const int32_t* __restrict__ col_weight, int P,
                                                               int32_t* __restrict__ inter, int32_t* __restrict__ area) {
  __shared__ int32_t tbl[kTrackMaxLabels * kTrackMaxLabels + kTrackMaxLabels];  // [P * P intersections | P areas]
  const int b = blockIdx.z;
  const int k = blockIdx.y + 1;  // the lag, in calls
  const LabelT* past = nullptr;
  if (b >= k)
    past = labels + (size_t)(b - k) * h * w;
  else if (k - b <= n_hist)
    past = hist + (size_t)(L - (k - b)) * h * w;  // newest last
  const bool with_area = k == 1;
  if (!past && !with_area) return;  // (uniform over the workgroup; the output was zeroed)
  const int n_tbl = P * P + P;
  int32_t* ar = tbl + P * P;
  for (int i = threadIdx.x; i < n_tbl; i += 256) tbl[i] = 0;
  __syncthreads();

  const LabelT* cur = labels + (size_t)b * h * w;
  const int gpr = (w + kCells - 1) / kCells;  // groups per row
  const int groups = h * gpr;
  for (int g = blockIdx.x * 256 + threadIdx.x; g < groups; g += gridDim.x * 256) {
    const int v = g / gpr;
    const int u0 = (g % gpr) * kCells;
    const int rw = row_weight[v];
    if (rw == 0) continue;  // a padding row
    const size_t base = (size_t)v * w + u0;
    int ra = -1, rc = -1, wsum = 0;  // the open run: labels and summed column weights
#pragma unroll
    for (int j = 0; j <= kCells; ++j) {
      int a = -1, c = -1, cw = 0;
      if (j < kCells && u0 + j < w) {
        cw = col_weight[u0 + j];
        if (cw != 0) {
          a = (int)cur[base + j];
          if (a < 0 || a >= P) a = -1;
          if (a >= 0 && past) {
            c = (int)past[base + j];
            if (c < 0 || c >= P) c = -1;
          }
        }
      }
      if (j < kCells && a == ra && c == rc) {
        wsum += cw;
        continue;
      }
      if (ra >= 0 && wsum != 0) {
        const int add = rw * wsum;
        if (with_area) atomicAdd(&ar[ra], add);
        if (rc >= 0) atomicAdd(&tbl[ra * P + rc], add);
      }
      ra = a, rc = c, wsum = cw;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_tbl; i += 256) {
    const int32_t val = tbl[i];
    if (val == 0) continue;
    if (i < P * P)
      atomicAdd(&inter[((size_t)b * L + (k - 1)) * P * P + i], val);
    else
      atomicAdd(&area[(size_t)b * P + (i - P * P)], val);
  }
}

}  // namespace ph

extern "C" int ph_track_mask_pairs(const void* labels_dev, int32_t label_bytes, int32_t B, int32_t h, int32_t w, const void* hist_dev, int32_t L, int32_t n_hist,
                                   const int32_t* row_weight_dev, const int32_t* col_weight_dev, int64_t image_pixels, int32_t P, int32_t* inter_dev, int32_t* area_dev,
                                   void* stream) {
  using namespace ph;
  PH_REQUIRE(labels_dev && hist_dev && row_weight_dev && col_weight_dev && inter_dev && area_dev, "ph_track_mask_pairs: null pointer");
  PH_REQUIRE(label_bytes == 1 || label_bytes == 2 || label_bytes == 4, "ph_track_mask_pairs: label_bytes must be 1, 2 or 4, got %d", label_bytes);
  PH_REQUIRE(B >= 1 && B <= 65535 && h >= 1 && w >= 1, "ph_track_mask_pairs: bad shape B=%d (1..65535) h=%d w=%d", B, h, w);
  PH_REQUIRE(P >= 1 && P <= kTrackMaxLabels, "ph_track_mask_pairs: P=%d must lie in [1, %d]", P, kTrackMaxLabels);
  PH_REQUIRE(L >= 1 && L <= kTrackMaxLags, "ph_track_mask_pairs: L=%d must lie in [1, %d]", L, kTrackMaxLags);
  PH_REQUIRE(n_hist >= 0 && n_hist <= L, "ph_track_mask_pairs: n_hist=%d must lie in [0, L=%d]", n_hist, L);
  PH_REQUIRE((int64_t)h * w <= 0x7fffffffLL, "ph_track_mask_pairs: maps of %d x %d cells exceed the int32 indices", h, w);
  PH_REQUIRE(image_pixels >= 0 && image_pixels < 0x80000000LL, "ph_track_mask_pairs: %lld image pixels per frame exceed the int32 counters (below 2^31)",
             (long long)image_pixels);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PH_HIP_CHECK(hipMemsetAsync(inter_dev, 0, sizeof(int32_t) * (size_t)B * L * P * P, s));
  PH_HIP_CHECK(hipMemsetAsync(area_dev, 0, sizeof(int32_t) * (size_t)B * P, s));
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const int64_t groups = (int64_t)h * ((w + kCells - 1) / kCells);
  // a workgroup walks at least 8 x 256 groups before it flushes its table; no more than 8 workgroups per CU over all (b, k)
  const int64_t chunks = std::max<int64_t>(1, std::min<int64_t>((groups + 2047) / 2048, std::max<int64_t>(1, (int64_t)cus * 8 / ((int64_t)B * L))));
  const dim3 grid((unsigned)chunks, (unsigned)L, (unsigned)B);
#define PH_LAUNCH_TRACK(T)                                                                                                                                        \
  hipLaunchKernelGGL((track_mask_pairs_kernel<T>), grid, dim3(256), 0, s, static_cast<const T*>(labels_dev), static_cast<const T*>(hist_dev), B, h, w, L, n_hist, \
                     row_weight_dev, col_weight_dev, P, inter_dev, area_dev)
  if (label_bytes == 1)
    PH_LAUNCH_TRACK(int8_t);
  else if (label_bytes == 2)
    PH_LAUNCH_TRACK(int16_t);
  else
    PH_LAUNCH_TRACK(int32_t);
#undef PH_LAUNCH_TRACK
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
