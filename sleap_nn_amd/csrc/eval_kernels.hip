// Segmentation evaluation: the pair statistics of two mask sets per frame, and the boundary region of a mask.
//
// Replaces the host loops of sleap_nn/evaluation.py: _mask_pair_stats (:352-372, P * G full-image logical_and / logical_or passes per
// frame behind _align_pair :339-349) and _mask_to_boundary (:375-393, copyMakeBorder + d iterations of a 3x3 erode).
//   * mask_pair_stats_kernel: ONE pass over the canvas pixels.  A thread owns 16 consecutive pixels of a canvas row and gives each a
//     membership word per set (bit g = ground-truth mask g covers it; bit p = predicted mask p, or the one bit of its label); equal
//     neighbours are folded into a run, and a run bumps the workgroup's LDS table (areas per set bit, intersections per bit pair) with
//     integer LDS atomics -- background pixels cost nothing, and almost every other pixel has one bit per side.  The table is flushed
//     once per workgroup with global integer atomics, zero entries skipped.  All sums are integers: exact, and the same in every run.
//     union = pred_area + gt_area - inter is left to the caller.
//   * mask_boundary: separable.  Row pass: rowok(y, x) = the 2d + 1 pixels (y, x - d .. x + d) are inside the image and foreground,
//     from the distance to the nearest background pixel on each side (found by a scan of at most d + 1 pixels per 16-pixel group, then
//     carried through the group), packed 16 pixels to a uint16.  Column pass: eroded = AND of rowok over rows y - d .. y + d, 16 pixels
//     per load, left at the first zero; out = mask AND NOT eroded.  (2d + 1) / 16 two-byte loads per pixel, never (2d + 1)^2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace ph {

constexpr int kEvalMaxMasks = 64;  // one bit of a uint64 membership word per mask
constexpr int kPx = 16;            // pixels per thread: one 16-byte load along W

// Nonzero flags of pixels x0 .. x0 + 15 of a row of `width` bytes read at cell x / s; bit j = pixel x0 + j.  Pixels at or beyond
// width * s are 0.  s == 1 and the 16 bytes inside the row: one 16-byte load when the address allows it, four 4-byte loads when it is
// 4-byte aligned; everything else byte by byte.
__device__ __forceinline__ uint32_t nonzero16(const uint8_t* __restrict__ row, int x0, int width, int s) {
  uint32_t bits = 0;
  if (s == 1 && x0 + kPx <= width) {
    const uint8_t* p = row + x0;
    uint32_t w[4];
    if (((uintptr_t)p & 15) == 0) {
      const uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x, w[1] = v.y, w[2] = v.z, w[3] = v.w;
    } else if (((uintptr_t)p & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = reinterpret_cast<const uint32_t*>(p)[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
    }
    if ((w[0] | w[1] | w[2] | w[3]) == 0) return 0;
#pragma unroll
    for (int j = 0; j < kPx; ++j) bits |= (uint32_t)(((w[j >> 2] >> (8 * (j & 3))) & 0xffu) != 0) << j;
    return bits;
  }
#pragma unroll
  for (int j = 0; j < kPx; ++j) {
    const int c = (x0 + j) / s;
    if (c < width) bits |= (uint32_t)(row[c] != 0) << j;
  }
  return bits;
}

// PRED_FORM 0: uint8 stack (B, P, ph, pw); 1 / 2 / 4: label map (B, ph, pw) of that many bytes, -1 = background.
template <typename LabelT, bool STACK>
__global__ __launch_bounds__(256) void mask_pair_stats_kernel(const void* __restrict__ pred_v, int P, int ph, int pw, int s, const uint8_t* __restrict__ gt, int G,
                                                              int H, int W, int Hc, int Wc, const int32_t* __restrict__ n_pred, const int32_t* __restrict__ n_gt,
                                                              int32_t* __restrict__ inter, int32_t* __restrict__ pred_area, int32_t* __restrict__ gt_area) {
  __shared__ int32_t tbl[kEvalMaxMasks * kEvalMaxMasks + 2 * kEvalMaxMasks];  // [P * G intersections | P areas | G areas]
  const int b = blockIdx.y;
  const int np = min(max(n_pred[b], 0), P), ng = min(max(n_gt[b], 0), G);
  const int n_tbl = P * G + P + G;
  int32_t* pa = tbl + P * G;
  int32_t* ga = pa + P;
  for (int i = threadIdx.x; i < n_tbl; i += 256) tbl[i] = 0;
  __syncthreads();

  const int gpr = (Wc + kPx - 1) / kPx;  // groups per canvas row
  const int groups = Hc * gpr;
  const int pe_w = pw * s;  // the prediction's extent on the canvas (ph * s rows)
  for (int k = blockIdx.x * 256 + threadIdx.x; k < groups; k += gridDim.x * 256) {
    const int y = k / gpr;
    const int x0 = (k % gpr) * kPx;
    uint64_t gm[kPx], pm[kPx];
#pragma unroll
    for (int j = 0; j < kPx; ++j) gm[j] = 0, pm[j] = 0;
    uint32_t any_g = 0, any_p = 0;
    if (y < H && x0 < W) {
      for (int g = 0; g < ng; ++g) {
        const uint32_t bits = nonzero16(gt + (((size_t)b * G + g) * H + y) * (size_t)W, x0, W, 1);
        if (bits == 0) continue;
        any_g |= bits;
#pragma unroll
        for (int j = 0; j < kPx; ++j) gm[j] |= (uint64_t)((bits >> j) & 1u) << g;
      }
    }
    const int cy = y / s;
    if (cy < ph && x0 < pe_w) {
      if constexpr (STACK) {
        const uint8_t* pred = static_cast<const uint8_t*>(pred_v);
        for (int p = 0; p < np; ++p) {
          const uint32_t bits = nonzero16(pred + (((size_t)b * P + p) * ph + cy) * (size_t)pw, x0, pw, s);
          if (bits == 0) continue;
          any_p |= bits;
#pragma unroll
          for (int j = 0; j < kPx; ++j) pm[j] |= (uint64_t)((bits >> j) & 1u) << p;
        }
      } else {
        const LabelT* row = static_cast<const LabelT*>(pred_v) + ((size_t)b * ph + cy) * (size_t)pw;
#pragma unroll
        for (int j = 0; j < kPx; ++j) {
          const int c = (x0 + j) / s;
          if (c < pw) {
            const int l = (int)row[c];
            if (l >= 0 && l < np) pm[j] = 1ull << l, any_p |= 1u << j;
          }
        }
      }
    }
    if ((any_g | any_p) == 0) continue;
    // fold equal neighbours into runs, one table update per run
    uint64_t rg = gm[0], rp = pm[0];
    int cnt = 1;
#pragma unroll
    for (int j = 1; j <= kPx; ++j) {
      const bool same = j < kPx && gm[j] == rg && pm[j] == rp;
      if (same) {
        ++cnt;
        continue;
      }
      if ((rg | rp) != 0) {
        for (uint64_t m = rg; m; m &= m - 1) atomicAdd(&ga[__builtin_ctzll(m)], cnt);
        for (uint64_t m = rp; m; m &= m - 1) {
          const int p = __builtin_ctzll(m);
          atomicAdd(&pa[p], cnt);
          for (uint64_t q = rg; q; q &= q - 1) atomicAdd(&tbl[p * G + __builtin_ctzll(q)], cnt);
        }
      }
      if (j < kPx) rg = gm[j], rp = pm[j], cnt = 1;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < n_tbl; i += 256) {
    const int32_t v = tbl[i];
    if (v == 0) continue;
    if (i < P * G)
      atomicAdd(&inter[(size_t)b * P * G + i], v);
    else if (i < P * G + P)
      atomicAdd(&pred_area[(size_t)b * P + (i - P * G)], v);
    else
      atomicAdd(&gt_area[(size_t)b * G + (i - P * G - P)], v);
  }
}

// ---- boundary -----------------------------------------------------------------------------------------------------------------------

// rowok bits of the 16-pixel group xg of row (n, y): bit j = pixels x - d .. x + d (x = 16 xg + j) are all inside [0, W) and foreground
__global__ __launch_bounds__(256) void boundary_row_kernel(const uint8_t* __restrict__ masks, int N, int H, int W, int d, uint16_t* __restrict__ rowok) {
  const int gpr = (W + kPx - 1) / kPx;
  const size_t groups = (size_t)N * H * gpr;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < groups; k += (size_t)gridDim.x * 256) {
    const int x0 = (int)(k % gpr) * kPx;
    const uint8_t* row = masks + (k / gpr) * (size_t)W;  // rows are numbered n * H + y
    const uint32_t m = nonzero16(row, x0, W, 1);
    uint32_t ok = 0;
    if (m != 0) {
      // nearest background pixel left of the group, -1 = the border; a scan that finds none within d + 1 pixels stands for "far enough"
      int last = x0 - 1;
      while (last >= 0 && x0 - 1 - last <= d && row[last] != 0) --last;
      int next = x0 + kPx;
      while (next < W && next - (x0 + kPx) <= d && row[next] != 0) ++next;
      uint32_t okl = 0, okr = 0;
#pragma unroll
      for (int j = 0; j < kPx; ++j) {
        if (!((m >> j) & 1u)) last = x0 + j;
        okl |= (uint32_t)(x0 + j - last > d) << j;
      }
#pragma unroll
      for (int j = kPx - 1; j >= 0; --j) {
        if (!((m >> j) & 1u)) next = x0 + j;
        okr |= (uint32_t)(next - (x0 + j) > d) << j;
      }
      ok = okl & okr;
    }
    rowok[k] = (uint16_t)ok;
  }
}

__global__ __launch_bounds__(256) void boundary_col_kernel(const uint8_t* __restrict__ masks, const uint16_t* __restrict__ rowok, int N, int H, int W, int d,
                                                           uint8_t* __restrict__ out) {
  const int gpr = (W + kPx - 1) / kPx;
  const size_t groups = (size_t)N * H * gpr;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < groups; k += (size_t)gridDim.x * 256) {
    const int xg = (int)(k % gpr);
    const int x0 = xg * kPx;
    const size_t r = k / gpr;  // n * H + y
    const int y = (int)(r % H);
    const uint32_t m = nonzero16(masks + r * (size_t)W, x0, W, 1);
    uint32_t er = 0;
    if (m != 0 && y >= d && y + d <= H - 1) {
      er = 0xffffu;
      for (int yy = -d; yy <= d && er != 0; ++yy) er &= rowok[(size_t)((int64_t)r + yy) * gpr + xg];
    }
    const uint32_t bd = m & ~er;
    uint8_t* o = out + r * (size_t)W + x0;
    if (x0 + kPx <= W && ((uintptr_t)o & 15) == 0) {
      uint32_t w[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        w[q] = ((bd >> (4 * q)) & 1u) | (((bd >> (4 * q + 1)) & 1u) << 8) | (((bd >> (4 * q + 2)) & 1u) << 16) | (((bd >> (4 * q + 3)) & 1u) << 24);
      *reinterpret_cast<uint4*>(o) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
      for (int j = 0; j < kPx; ++j)
        if (x0 + j < W) o[j] = (uint8_t)((bd >> j) & 1u);
    }
  }
}

}  // namespace ph

extern "C" int ph_mask_pair_stats(const void* pred_dev, int32_t pred_form, int32_t P, int32_t ph, int32_t pw, int32_t pred_stride, const uint8_t* gt_dev, int32_t G,
                                  int32_t H, int32_t W, int32_t B, const int32_t* n_pred_dev, const int32_t* n_gt_dev, int32_t* inter_dev, int32_t* pred_area_dev,
                                  int32_t* gt_area_dev, void* stream) {
  using namespace ph;
  PH_REQUIRE(pred_dev && gt_dev && n_pred_dev && n_gt_dev && inter_dev && pred_area_dev && gt_area_dev, "ph_mask_pair_stats: null pointer");
  PH_REQUIRE(pred_form == 0 || pred_form == 1 || pred_form == 2 || pred_form == 4,
             "ph_mask_pair_stats: pred_form must be 0 (uint8 stack) or the label width 1, 2 or 4, got %d", pred_form);
  PH_REQUIRE(B > 0 && H > 0 && W > 0 && ph > 0 && pw > 0, "ph_mask_pair_stats: bad shape B=%d H=%d W=%d ph=%d pw=%d", B, H, W, ph, pw);
  PH_REQUIRE(P >= 1 && P <= kEvalMaxMasks && G >= 1 && G <= kEvalMaxMasks, "ph_mask_pair_stats: P=%d and G=%d must lie in [1, %d]", P, G, kEvalMaxMasks);
  PH_REQUIRE(pred_stride >= 1, "ph_mask_pair_stats: pred_stride must be >= 1, got %d", pred_stride);
  PH_REQUIRE(B <= 65535, "ph_mask_pair_stats: at most 65535 frames per call, got %d", B);
  const int64_t Hc = std::max<int64_t>(H, (int64_t)ph * pred_stride), Wc = std::max<int64_t>(W, (int64_t)pw * pred_stride);
  PH_REQUIRE(Hc * (Wc + kPx) <= 0x7fffffffLL, "ph_mask_pair_stats: canvas %lld x %lld exceeds the int32 counters", (long long)Hc, (long long)Wc);
  hipStream_t s = static_cast<hipStream_t>(stream);
  PH_HIP_CHECK(hipMemsetAsync(inter_dev, 0, sizeof(int32_t) * (size_t)B * P * G, s));
  PH_HIP_CHECK(hipMemsetAsync(pred_area_dev, 0, sizeof(int32_t) * (size_t)B * P, s));
  PH_HIP_CHECK(hipMemsetAsync(gt_area_dev, 0, sizeof(int32_t) * (size_t)B * G, s));
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const int64_t groups = Hc * ((Wc + kPx - 1) / kPx);
  // a workgroup walks at least 8 x 256 groups before it flushes its table; no more than 8 workgroups per CU over the batch
  const int64_t per_frame = std::max<int64_t>(1, std::min<int64_t>((groups + 2047) / 2048, std::max<int64_t>(1, (int64_t)cus * 8 / B)));
  const dim3 grid((unsigned)per_frame, (unsigned)B);
#define PH_LAUNCH_PAIR(T, STACK)                                                                                                                              \
  hipLaunchKernelGGL((mask_pair_stats_kernel<T, STACK>), grid, dim3(256), 0, s, pred_dev, P, ph, pw, pred_stride, gt_dev, G, H, W, (int)Hc, (int)Wc, n_pred_dev, \
                     n_gt_dev, inter_dev, pred_area_dev, gt_area_dev)
  if (pred_form == 0)
    PH_LAUNCH_PAIR(int8_t, true);
  else if (pred_form == 1)
    PH_LAUNCH_PAIR(int8_t, false);
  else if (pred_form == 2)
    PH_LAUNCH_PAIR(int16_t, false);
  else
    PH_LAUNCH_PAIR(int32_t, false);
#undef PH_LAUNCH_PAIR
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

extern "C" int64_t ph_mask_boundary_scratch_bytes(int32_t N, int32_t H, int32_t W) {
  if (N <= 0 || H <= 0 || W <= 0) return 0;
  return (int64_t)N * H * ((W + ph::kPx - 1) / ph::kPx) * (int64_t)sizeof(uint16_t);
}

extern "C" int ph_mask_boundary(const uint8_t* masks_dev, int32_t N, int32_t H, int32_t W, int32_t d, uint8_t* out_dev, void* scratch_dev, int64_t scratch_bytes,
                                void* stream) {
  using namespace ph;
  PH_REQUIRE(masks_dev && out_dev && scratch_dev, "ph_mask_boundary: null pointer");
  PH_REQUIRE(N > 0 && H > 0 && W > 0, "ph_mask_boundary: bad shape N=%d H=%d W=%d", N, H, W);
  PH_REQUIRE(d >= 1, "ph_mask_boundary: d must be >= 1, got %d", d);
  PH_REQUIRE(masks_dev != out_dev, "ph_mask_boundary: masks and out are the same buffer");
  PH_REQUIRE(((uintptr_t)scratch_dev & 1) == 0, "ph_mask_boundary: scratch must be 2-byte aligned");
  const int64_t need = ph_mask_boundary_scratch_bytes(N, H, W);
  if (scratch_bytes < need) {
    set_error("ph_mask_boundary: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
    return PH_E_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const size_t groups = (size_t)N * H * ((W + kPx - 1) / kPx);
  const unsigned grid = (unsigned)std::min<size_t>((groups + 255) / 256, (size_t)cus * 8);  // 8 workgroups of 4 waves per CU, grid-stride beyond
  uint16_t* rowok = static_cast<uint16_t*>(scratch_dev);
  hipLaunchKernelGGL(boundary_row_kernel, dim3(grid), dim3(256), 0, s, masks_dev, N, H, W, d, rowok);
  PH_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(boundary_col_kernel, dim3(grid), dim3(256), 0, s, masks_dev, rowok, N, H, W, d, out_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
