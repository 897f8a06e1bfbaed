// Bottom-up instance segmentation: the per-pixel part of the fragment merge (sleap_nn/inference/segmentation.py:424-579, the region-adjacency
// graph of merge_instances) on the device.  Runs on the label map ph_seg_assign / ph_seg_gate leave on the device, on the caller's stream, no
// host synchronisation.  The graph itself (tens of nodes: affinities and agglomeration) is host work on what comes out of here.
//
//   * mt_init_kernel: the dense contact table T (frame, a, b) = 0 and the per (frame, label) bounding boxes = empty.
//   * mt_contact_kernel<label type, d>: one block per (frame, 16 x 64 tile), the tile and a halo of d cells in LDS as int32 (-1 outside the
//     image, for background and for a label at or beyond the frame's centre count).  A pixel labelled b looks at the 2 d (d + 1) cells of its
//     L1 diamond (SciPy's cross iterated d times); interior pixels (every neighbour is b or nothing) stop there.  Otherwise the neighbour
//     labels are de-duplicated in registers -- a cell counts when no earlier cell of the diamond carries its label -- and T[a][b] += 1 once per
//     distinct a.  With at most MT_LDS_N centres in the frame the block adds into an LDS copy of the table and of the boxes and flushes the
//     non-zero entries once; with more it adds to the global table directly (many labels: little contention).  Integer atomics only.
//   * mt_moment_kernel: one block per (frame, label) over the label's bounding box: sums of rx, ry, rx^2, ry^2 in float64 with
//     rx = (x - xc) s + dx (the offset-predicted centre relative to the instance's own centre).  A thread adds its pixels in raster order of a
//     fixed pixel -> thread map (pixel index in the box mod 256), the 256 partial sums are folded by a fixed tree: the order of every addition
//     depends on the label map alone, so the sums are bit-identical from run to run and on any stream.  No floating-point atomics.
//   * mt_edge_kernel: one block per frame walks the pairs (i, j) in row-major order, keeps i < j with T[i][j] + T[j][i] > 0 by an ordered
//     compaction (block scan) and writes (i, j, T[i][j], T[j][i], ridge minimum); the true count is reported, entries beyond edge_cap are
//     not written.  Ridge minimum: the fp32 minimum (NaN if any sample is NaN, as np.min) of the centre map over the cells
//     round(ca + (cb - ca) k / 47), k = 7..39, in integer arithmetic: floor((2 (47 ca + (cb - ca) k) + 47) / 94); no sample is a rounding tie.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace ph {

constexpr int MT_TH = 16, MT_TW = 64;  // tile of the contact pass: 1024 pixels, 4 per thread
constexpr int MT_LDS_N = 64;           // centres per frame up to which a block accumulates the table in LDS (16 KiB)
constexpr int MT_MAX_CENTERS = 4096;   // the dense table holds max_centers^2 counters per frame

__device__ __forceinline__ int mt_scan256(int v, int* total, int* lds /* >= 4 ints */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int n = __shfl_up(inc, d, 64);
    if (lane >= d) inc += n;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int s = lds[w];
    if (w < wave) base += s;
    tot += s;
  }
  __syncthreads();
  *total = tot;
  return base + inc - v;
}

__global__ __launch_bounds__(256) void mt_init_kernel(int64_t n_table, int64_t n_box, int* __restrict__ table, int* __restrict__ box) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_table) table[i] = 0;
  if (i < n_box) {
    box[4 * i] = 0x7fffffff;
    box[4 * i + 1] = 0x7fffffff;
    box[4 * i + 2] = -1;
    box[4 * i + 3] = -1;
  }
}

template <typename LT, int D>
__global__ __launch_bounds__(256) void mt_contact_kernel(const LT* __restrict__ labels, int H, int W, int tiles_x, const int* __restrict__ counts, int max_centers,
                                                         int* __restrict__ table, int* __restrict__ box) {
  constexpr int SW = MT_TW + 2 * D, SH = MT_TH + 2 * D;
  constexpr int M = 2 * D * (D + 1);
  __shared__ int s_lab[SH * SW];
  __shared__ int s_tab[MT_LDS_N * MT_LDS_N];
  __shared__ int s_box[4 * MT_LDS_N];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(counts[b], max_centers);
  if (n <= 0) return;  // (block-uniform)
  const int ty0 = (blockIdx.x / tiles_x) * MT_TH, tx0 = (blockIdx.x % tiles_x) * MT_TW;
  const LT* lab = labels + (size_t)b * H * W;
  int* tab = table + (size_t)b * max_centers * max_centers;
  int* bx = box + (size_t)b * max_centers * 4;
  const bool in_lds = n <= MT_LDS_N;
  for (int i = tid; i < SH * SW; i += 256) {
    const int y = ty0 - D + i / SW, x = tx0 - D + i % SW;
    int v = -1;
    if (y >= 0 && y < H && x >= 0 && x < W) v = (int)lab[(size_t)y * W + x];
    s_lab[i] = (v >= 0 && v < n) ? v : -1;  // nothing at or beyond n ever indexes a table
  }
  if (in_lds) {
    for (int i = tid; i < n * n; i += 256) s_tab[i] = 0;
    for (int i = tid; i < n; i += 256) {
      s_box[4 * i] = 0x7fffffff;
      s_box[4 * i + 1] = 0x7fffffff;
      s_box[4 * i + 2] = -1;
      s_box[4 * i + 3] = -1;
    }
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = tid + e * 256;
    const int r = i >> 6, c = i & 63;
    const int* ctr = s_lab + (r + D) * SW + c + D;
    const int bl = *ctr;
    if (bl < 0) continue;
    int* pb = in_lds ? s_box + 4 * bl : bx + 4 * bl;
    atomicMin(&pb[0], tx0 + c);
    atomicMin(&pb[1], ty0 + r);
    atomicMax(&pb[2], tx0 + c);
    atomicMax(&pb[3], ty0 + r);
    int nb[M];
    int k = 0;
    bool any = false;
#pragma unroll
    for (int dy = -D; dy <= D; ++dy) {
      const int span = D - (dy < 0 ? -dy : dy);
#pragma unroll
      for (int dx = -D; dx <= D; ++dx) {
        if (dx < -span || dx > span || (dx == 0 && dy == 0)) continue;
        int a = ctr[dy * SW + dx];
        a = a == bl ? -1 : a;
        nb[k++] = a;
        any |= a >= 0;
      }
    }
    if (!any) continue;
#pragma unroll
    for (int q = 0; q < M; ++q) {
      const int a = nb[q];
      bool fresh = a >= 0;
#pragma unroll
      for (int j = 0; j < q; ++j) fresh &= nb[j] != a;
      if (fresh) {
        if (in_lds) atomicAdd(&s_tab[a * n + bl], 1);
        else atomicAdd(&tab[(size_t)a * max_centers + bl], 1);
      }
    }
  }
  if (!in_lds) return;
  __syncthreads();
  for (int i = tid; i < n * n; i += 256) {
    const int v = s_tab[i];
    if (v) atomicAdd(&tab[(size_t)(i / n) * max_centers + i % n], v);
  }
  for (int i = tid; i < n; i += 256) {
    if (s_box[4 * i + 2] < 0) continue;
    atomicMin(&bx[4 * i], s_box[4 * i]);
    atomicMin(&bx[4 * i + 1], s_box[4 * i + 1]);
    atomicMax(&bx[4 * i + 2], s_box[4 * i + 2]);
    atomicMax(&bx[4 * i + 3], s_box[4 * i + 3]);
  }
}

template <typename LT>
__global__ __launch_bounds__(256) void mt_moment_kernel(const LT* __restrict__ labels, const float* __restrict__ offsets, int H, int W, int stride,
                                                        const int* __restrict__ centers, const int* __restrict__ counts, int max_centers, const int* __restrict__ box,
                                                        double* __restrict__ moments) {
  __shared__ double s_red[4][256];
  const int b = blockIdx.y, l = blockIdx.x, tid = threadIdx.x;
  const size_t rec = (size_t)b * max_centers + l;
  const int n = min(counts[b], max_centers);
  const int x0 = box[4 * rec], y0 = box[4 * rec + 1], x1 = box[4 * rec + 2], y1 = box[4 * rec + 3];
  if (l >= n || x1 < x0 || y1 < y0) {  // (block-uniform) no such instance, or one without pixels
    if (tid < 4) moments[4 * rec + tid] = 0.0;
    return;
  }
  const LT* lab = labels + (size_t)b * H * W;
  const float* ox = offsets + (size_t)b * 2 * H * W;
  const float* oy = ox + (size_t)H * W;
  const int xc = centers[2 * rec], yc = centers[2 * rec + 1];
  const int bw = x1 - x0 + 1, total = bw * (y1 - y0 + 1);
  double sx = 0.0, sy = 0.0, sxx = 0.0, syy = 0.0;
  for (int i = tid; i < total; i += 256) {
    const int y = y0 + i / bw, x = x0 + i % bw;
    const size_t p = (size_t)y * W + x;
    if ((int)lab[p] != l) continue;
    const double rx = (double)((x - xc) * stride) + (double)ox[p];
    const double ry = (double)((y - yc) * stride) + (double)oy[p];
    sx += rx;
    sy += ry;
    sxx += rx * rx;
    syy += ry * ry;
  }
  s_red[0][tid] = sx;
  s_red[1][tid] = sy;
  s_red[2][tid] = sxx;
  s_red[3][tid] = syy;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (tid < half) {
#pragma unroll
      for (int q = 0; q < 4; ++q) s_red[q][tid] += s_red[q][tid + half];
    }
    __syncthreads();
  }
  if (tid < 4) moments[4 * rec + tid] = s_red[tid][0];
}

__global__ __launch_bounds__(256) void mt_edge_kernel(const float* __restrict__ hm, int H, int W, const int* __restrict__ centers, const int* __restrict__ counts,
                                                      int max_centers, const int* __restrict__ table, int* __restrict__ edge_counts, int* __restrict__ edges,
                                                      int edge_cap) {
  __shared__ int red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(counts[b], max_centers);
  const int* tab = table + (size_t)b * max_centers * max_centers;
  const int* cen = centers + (size_t)b * max_centers * 2;
  const float* map = hm + (size_t)b * H * W;
  int run = 0;
  for (int p0 = 0; p0 < n * n; p0 += 256) {  // (n <= 4096: n * n fits an int)
    const int p = p0 + tid;
    int i = 0, j = 0, tij = 0, tji = 0;
    if (p < n * n) {
      i = p / n;
      j = p - i * n;
      if (i < j) {
        tij = tab[(size_t)i * max_centers + j];
        tji = tab[(size_t)j * max_centers + i];
      }
    }
    const int flag = (tij + tji) > 0;
    int tot;
    const int pos = run + mt_scan256(flag, &tot, red);
    run += tot;
    if (flag && pos < edge_cap) {
      const int ax = cen[2 * i], ay = cen[2 * i + 1], ex = cen[2 * j] - ax, ey = cen[2 * j + 1] - ay;
      float m = 0.f;
      for (int k = 7; k <= 39; ++k) {
        const int xi = min(max((2 * (47 * ax + ex * k) + 47) / 94, 0), W - 1);  // (the point lies between two centres of the map: never negative)
        const int yi = min(max((2 * (47 * ay + ey * k) + 47) / 94, 0), H - 1);
        const float v = map[(size_t)yi * W + xi];
        m = (k == 7 || v < m || v != v) ? v : m;
      }
      int* dst = edges + ((size_t)b * edge_cap + pos) * 5;
      dst[0] = i;
      dst[1] = j;
      dst[2] = tij;
      dst[3] = tji;
      dst[4] = __float_as_int(m);
    }
  }
  if (tid == 0) edge_counts[b] = run;
}

struct MtLayout {
  int64_t table, box, total;  // byte offsets
};

static inline MtLayout mt_layout(int64_t B, int64_t mc) {
  MtLayout L;
  L.table = 0;
  L.box = align_up(B * mc * mc * 4, 8);
  L.total = align_up(L.box + B * mc * 16, 8);
  return L;
}

}  // namespace ph

using namespace ph;

extern "C" int64_t ph_seg_merge_scratch_bytes(int32_t B, int32_t h, int32_t w, int32_t max_centers) {
  if (B <= 0 || h <= 0 || w <= 0 || max_centers <= 0 || max_centers > MT_MAX_CENTERS) return 0;
  return mt_layout(B, max_centers).total;
}

extern "C" int ph_seg_merge_tables(const void* labels_dev, const float* center_dev, const float* offsets_dev, int32_t B, int32_t h, int32_t w, int32_t output_stride,
                                   int32_t dilate, const int32_t* centers_dev, const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes,
                                   double* moments_dev, int32_t* edge_counts_dev, int32_t* edges_dev, int32_t edge_cap, void* scratch_dev, int64_t scratch_bytes,
                                   void* stream) {
  PH_REQUIRE(labels_dev && center_dev && offsets_dev && centers_dev && counts_dev && moments_dev && edge_counts_dev && edges_dev && scratch_dev,
             "ph_seg_merge_tables: null pointer");
  PH_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && h <= 32767 && w <= 32767 && (int64_t)h * w <= 0x7fffffffLL,
             "ph_seg_merge_tables: bad map shape B=%d h=%d w=%d (each side at most 32767)", B, h, w);
  PH_REQUIRE(output_stride >= 1 && output_stride <= 1024, "ph_seg_merge_tables: output_stride=%d out of range [1, 1024]", output_stride);
  PH_REQUIRE(dilate >= 1 && dilate <= 4, "ph_seg_merge_tables: dilate=%d out of range [1, 4]", dilate);
  PH_REQUIRE(max_centers > 0 && max_centers <= MT_MAX_CENTERS && (int64_t)B * max_centers * max_centers <= (1LL << 29),
             "ph_seg_merge_tables: max_centers=%d (B=%d) beyond the dense contact table (at most %d, B * max_centers^2 <= 2^29)", max_centers, B, MT_MAX_CENTERS);
  PH_REQUIRE(edge_cap > 0 && (int64_t)B * edge_cap * 5 <= 0x7fffffffLL, "ph_seg_merge_tables: edge_cap=%d must be positive (B * edge_cap * 5 < 2^31)", edge_cap);
  PH_REQUIRE((label_bytes == 1 && max_centers <= 127) || (label_bytes == 2 && max_centers <= 32767) || label_bytes == 4,
             "ph_seg_merge_tables: %d-byte labels cannot hold %d centres", label_bytes, max_centers);
  PH_REQUIRE(((uintptr_t)scratch_dev & 7) == 0, "ph_seg_merge_tables: scratch must be 8-byte aligned");
  const MtLayout L = mt_layout(B, max_centers);
  PH_REQUIRE(scratch_bytes >= L.total, "ph_seg_merge_tables: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)L.total);
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* sc = static_cast<char*>(scratch_dev);
  int* table = reinterpret_cast<int*>(sc + L.table);
  int* box = reinterpret_cast<int*>(sc + L.box);
  const int64_t n_table = (int64_t)B * max_centers * max_centers, n_box = (int64_t)B * max_centers;
  const int tiles_x = (w + MT_TW - 1) / MT_TW, tiles_y = (h + MT_TH - 1) / MT_TH;
  hipLaunchKernelGGL(mt_init_kernel, dim3((unsigned)((n_table + 255) / 256)), dim3(256), 0, s, n_table, n_box, table, box);
#define PH_MT_CONTACT(LT, D) \
  hipLaunchKernelGGL((mt_contact_kernel<LT, D>), dim3(tiles_x * tiles_y, B), dim3(256), 0, s, in, h, w, tiles_x, counts_dev, max_centers, table, box)
#define PH_MT_RUN(LT)                                                                                                                                      \
  do {                                                                                                                                                     \
    const LT* in = static_cast<const LT*>(labels_dev);                                                                                                     \
    if (dilate == 1) PH_MT_CONTACT(LT, 1);                                                                                                                 \
    else if (dilate == 2) PH_MT_CONTACT(LT, 2);                                                                                                            \
    else if (dilate == 3) PH_MT_CONTACT(LT, 3);                                                                                                            \
    else PH_MT_CONTACT(LT, 4);                                                                                                                             \
    hipLaunchKernelGGL((mt_moment_kernel<LT>), dim3(max_centers, B), dim3(256), 0, s, in, offsets_dev, h, w, output_stride, centers_dev, counts_dev,       \
                       max_centers, box, moments_dev);                                                                                                     \
  } while (0)
  if (label_bytes == 1) PH_MT_RUN(int8_t);
  else if (label_bytes == 2) PH_MT_RUN(int16_t);
  else PH_MT_RUN(int32_t);
#undef PH_MT_RUN
#undef PH_MT_CONTACT
  hipLaunchKernelGGL(mt_edge_kernel, dim3(B), dim3(256), 0, s, center_dev, h, w, centers_dev, counts_dev, max_centers, table, edge_counts_dev, edges_dev, edge_cap);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
