// Bottom-up instance segmentation: grouping foreground pixels into instances on the device, and the semantic (one mask per frame) variant.
//
// Replaces the host post-process of sleap_nn/inference/layers/segmentation.py:159-266 -- four full-resolution fp32 channels copied
// to the host per frame, then find_center_peaks (max-pool + SciPy connected components, inference/segmentation.py:12-60) and an
// (M foreground pixels) x (N centres) distance matrix with argmin (segmentation.py:159-190) and the adaptive distance gate
// (segmentation.py:197-211) -- by a fixed sequence of launches on the caller's stream, no host synchronisation in between:
//   * seg_cand_kernel: one block per (frame, 8 rows).  A pixel is a candidate when hm > threshold and hm >= every in-image value of
//     its k x k window (the max-pool pads with -inf).  Candidates are staged in raster order (block scan per 256 columns; a block's
//     staging area holds all its pixels, so nothing can overflow) and counted.
//   * seg_collapse_kernel: one block per frame.  Compacts the staged candidates into one raster-ordered list, finds each one's four
//     4-connected neighbours in it (left / right are the list neighbours, up / down a binary search), and runs min-label
//     propagation with pointer jumping until a sweep changes nothing: every plateau ends up labelled by its raster-first pixel.
//     The representative of a component is its maximum value, raster-first on ties (one 64-bit atomic max of
//     (ordered value, ~list index) per candidate); components are numbered by their raster-first pixel (a scan over the roots).
//     With max_instances set and more components, the max_instances largest values are kept in descending order.  The list lives
//     in LDS up to SG_LDS_CAND candidates and in the caller's scratch beyond.
//   * seg_assign_kernel: a thread owns 4 pixels; the centres of the frame are staged in LDS SG_CHUNK at a time and every foreground
//     pixel keeps the first minimum of d = (px - cx)^2 + (py - cy)^2 -- fp32, every product and sum rounded on its own (see the
//     pragma below), the operation order of the torch expression, so the argmin is the reference's bit for bit.  Writes the label
//     map (-1 = background) in the narrowest integer type the caller asked for, d per pixel when the gate needs it, and per-centre
//     pixel counts (integer atomics: LDS histogram per block, then one global add per non-empty bin).
//   * seg_gate_kernel: one launch per gate pass.  r2 = (alpha * sqrt(count / pi) * stride)^2 from the counts of the previous pass,
//     keep = d <= r2[label] recomputed over ALL assigned pixels, as the reference does, new counts; the last pass writes the gated label map.
//   * seg_sem_kernel + seg_sem_final_kernel: pixel count and sum of fg over fg > threshold per frame (fixed-order partial sums,
//     double accumulation: deterministic) and the 0 / 1 map.
//   * seg_place_kernel: top-down crop masks into frame space (decode_mask_to_image_res, inference/segmentation_convert.py:74-133, for a whole
//     batch): the output (B, P, H, W) is walked as one flat array of 16-byte chunks, one chunk per lane per step, stored as one
//     16-byte vector.  A chunk usually lies in one row; where W is no multiple of 16 it runs on into the next row (or slot) and
//     the lane re-reads that row's crop record.  Nearest source index (u * w) / We by one division where a lane enters the crop,
//     then by remainder stepping.  Every byte is written, nothing is accumulated.
// All of it is HBM-shaped integer / index work: each of the four channels is read once (the centre map a second time only around
// pixels above the threshold), and what goes back to the host is one small integer per pixel instead of 16 bytes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

// d must round its two products and its sum separately, as the torch expression does; hipcc contracts a * b + c by default and
// the __fmul_rn / __fadd_rn wrappers do not prevent it once inlined (see tile_kernels.hip).  Plain operators under this pragma.
#pragma clang fp contract(off)

namespace ph {

constexpr int SG_ROWS = 8;          // rows per candidate block
constexpr int SG_LDS_CAND = 2048;   // candidates whose list is kept in LDS (16 bytes each)
constexpr int SG_CHUNK = 1024;      // centres staged in LDS at a time; also the size of the per-block count histogram
constexpr int SG_PIX = 4;           // pixels per thread in the assignment / gate / semantic kernels

__device__ __forceinline__ int sg_scan256(int v, int* total, int* lds /* >= 4 ints */) {
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

// ---- centre peaks -------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void seg_cand_kernel(const float* __restrict__ hm, int H, int W, float thr, int half, int groups,
                                                       int* __restrict__ blk_count, int* __restrict__ stage) {
  __shared__ int red[4];
  const int blk = blockIdx.x;
  const int b = blk / groups, y0 = (blk - b * groups) * SG_ROWS;
  const float* plane = hm + (size_t)b * H * W;
  int* stg = stage + (size_t)blk * SG_ROWS * W;
  const int rows = min(SG_ROWS, H - y0);
  int base = 0;
  for (int r = 0; r < rows; ++r) {
    const int y = y0 + r;
    for (int xb = 0; xb < W; xb += 256) {
      const int x = xb + (int)threadIdx.x;
      int c = 0;
      if (x < W) {
        const float v = plane[(size_t)y * W + x];
        if (v > thr) {  // (most pixels of a centre map stop here; NaN compares false)
          bool ok = true;
          for (int dy = -half; dy <= half; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= H) continue;
            for (int dx = -half; dx <= half; ++dx) {
              const int xx = x + dx;
              if (xx < 0 || xx >= W) continue;
              ok = ok && (v >= plane[(size_t)yy * W + xx]);  // (a NaN in the window: false, as hm >= NaN-pooled is)
            }
          }
          c = ok ? 1 : 0;
        }
      }
      int tot;
      const int ex = sg_scan256(c, &tot, red);
      if (c) stg[base + ex] = y * W + x;
      base += tot;
    }
  }
  if (threadIdx.x == 0) blk_count[blk] = base;
}

__device__ __forceinline__ unsigned sg_ordered(float v) {
  const unsigned u = __float_as_uint(v + 0.0f);  // (-0 -> +0: equal values, equal keys)
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ int sg_find(const int* pos, int n, int key) {
  int lo = 0, hi = n - 1;
  while (lo <= hi) {
    const int mid = (lo + hi) >> 1;
    const int p = pos[mid];
    if (p == key) return mid;
    if (p < key) lo = mid + 1; else hi = mid - 1;
  }
  return -1;
}

__global__ __launch_bounds__(256) void seg_collapse_kernel(const float* __restrict__ hm, int B, int H, int W, int groups, const int* __restrict__ blk_count,
                                                           const int* __restrict__ stage, int cap, int max_centers, int max_instances, int* __restrict__ gscratch,
                                                           int* __restrict__ centers, float* __restrict__ scores, int* __restrict__ counts,
                                                           int* __restrict__ pix_counts, int n_count_bufs) {
  __shared__ int s_pos[SG_LDS_CAND];
  __shared__ int s_lab[SG_LDS_CAND];
  __shared__ unsigned long long s_nbr[SG_LDS_CAND];
  __shared__ int red[4];
  __shared__ int s_changed;
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* plane = hm + (size_t)b * H * W;
  for (int k = 0; k < n_count_bufs; ++k)
    for (int i = tid; i < max_centers; i += 256) pix_counts[((size_t)k * B + b) * max_centers + i] = 0;
  int* pos;
  int* lab;
  unsigned long long* nbr;  // (up, down) list indices during the propagation; the component's best key afterwards
  if (cap <= SG_LDS_CAND) {
    pos = s_pos;
    lab = s_lab;
    nbr = s_nbr;
  } else {
    int* g = gscratch + (size_t)b * 4 * cap;
    nbr = reinterpret_cast<unsigned long long*>(g);
    pos = g + 2 * (size_t)cap;
    lab = g + 3 * (size_t)cap;
  }
  // one raster-ordered list of the frame's candidates
  int n = 0;
  for (int g = 0; g < groups; ++g) {
    const int c = blk_count[b * groups + g];
    const int* stg = stage + (size_t)(b * groups + g) * SG_ROWS * W;
    for (int i = tid; i < c; i += 256)
      if (n + i < cap) pos[n + i] = stg[i];
    n += c;
  }
  if (tid == 0) counts[B + b] = n;
  if (n > cap || n == 0) {  // (block-uniform) more candidates than the list holds: the caller sees the count and comes back with room
    if (tid == 0) counts[b] = 0;
    return;
  }
  __syncthreads();
  int2* ud = reinterpret_cast<int2*>(nbr);
  for (int i = tid; i < n; i += 256) {
    const int p = pos[i];
    const int y = p / W;
    ud[i] = make_int2(y > 0 ? sg_find(pos, n, p - W) : -1, y < H - 1 ? sg_find(pos, n, p + W) : -1);
    lab[i] = i;
  }
  // min-label propagation over the 4-connected candidates.  A thread writes lab[i] of its own candidates only and labels only ever
  // decrease to indices of the same component, so reading a neighbour's label while it changes is harmless; a sweep that changes
  // nothing has read final values everywhere.
  volatile int* vlab = lab;
  int again;
  do {
    __syncthreads();
    if (tid == 0) s_changed = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
      const int p = pos[i];
      const int x = p - (p / W) * W;
      const int cur = vlab[i];
      int m = cur;
      if (i > 0 && x > 0 && pos[i - 1] == p - 1) m = min(m, vlab[i - 1]);
      if (i + 1 < n && x < W - 1 && pos[i + 1] == p + 1) m = min(m, vlab[i + 1]);
      const int2 n2 = ud[i];
      if (n2.x >= 0) m = min(m, vlab[n2.x]);
      if (n2.y >= 0) m = min(m, vlab[n2.y]);
      m = min(m, vlab[m]);  // pointer jump
      if (m < cur) {
        vlab[i] = m;
        s_changed = 1;
      }
    }
    __syncthreads();
    again = s_changed;
  } while (again);
  // representative = maximum value, raster-first on ties
  for (int i = tid; i < n; i += 256) nbr[i] = 0ull;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const unsigned long long key = ((unsigned long long)sg_ordered(plane[pos[i]]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)i);
    atomicMax(&nbr[lab[i]], key);
  }
  __syncthreads();
  // components in the order of their raster-first pixel: lab[r] <- pixel of component r's representative (r <= the root's index, and
  // entries below a chunk are never read again, so the list is compacted in place)
  int n_comp = 0;
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + tid;
    const bool root = i < n && lab[i] == i;
    int rep_pos = 0;
    if (root) rep_pos = pos[(int)(0xFFFFFFFFu - (unsigned)(nbr[i] & 0xFFFFFFFFull))];
    int tot;
    const int ex = sg_scan256(root ? 1 : 0, &tot, red);
    if (root) lab[n_comp + ex] = rep_pos;
    n_comp += tot;
  }
  __syncthreads();
  int* cxy = centers + (size_t)b * max_centers * 2;
  float* sc = scores + (size_t)b * max_centers;
  if (max_instances > 0 && n_comp > max_instances) {  // torch.topk: the largest values, descending (equal values: the earlier component first)
    float* val = reinterpret_cast<float*>(nbr);
    for (int r = tid; r < n_comp; r += 256) val[r] = plane[lab[r]];
    __syncthreads();
    for (int r = tid; r < n_comp; r += 256) {
      const float v = val[r];
      int rank = 0;
      for (int q = 0; q < n_comp; ++q) {
        const float u = val[q];
        rank += (u > v || (u == v && q < r)) ? 1 : 0;
      }
      if (rank < max_instances && rank < max_centers) {
        const int p = lab[r];
        cxy[2 * rank] = p - (p / W) * W;
        cxy[2 * rank + 1] = p / W;
        sc[rank] = v;
      }
    }
    if (tid == 0) counts[b] = max_instances;
  } else {
    for (int r = tid; r < n_comp && r < max_centers; r += 256) {
      const int p = lab[r];
      cxy[2 * r] = p - (p / W) * W;
      cxy[2 * r + 1] = p / W;
      sc[r] = plane[p];
    }
    if (tid == 0) counts[b] = n_comp;
  }
}

// ---- pixel assignment ---------------------------------------------------------------------------------------------

// per-centre pixel counts of a block: LDS histogram when the frame's centres fit it, global atomics otherwise
struct SegHist {
  int* lds;
  int* glob;
  int n;
  bool local;
  __device__ __forceinline__ void init(int* lds_, int* glob_, int n_) {
    lds = lds_;
    glob = glob_;
    n = n_;
    local = n_ <= SG_CHUNK;
    if (local)
      for (int i = threadIdx.x; i < n; i += 256) lds[i] = 0;
    __syncthreads();
  }
  __device__ __forceinline__ void add(int k) { atomicAdd(local ? &lds[k] : &glob[k], 1); }
  __device__ __forceinline__ void flush() {
    __syncthreads();
    if (local)
      for (int i = threadIdx.x; i < n; i += 256) {
        const int c = lds[i];
        if (c) atomicAdd(&glob[i], c);
      }
  }
};

template <typename LT>
__global__ __launch_bounds__(256) void seg_assign_kernel(const float* __restrict__ fg, const float* __restrict__ off, int H, int W, float fg_thr, float stride, float half,
                                                         const int* __restrict__ centers, const int* __restrict__ counts, int max_centers, LT* __restrict__ labels,
                                                         float* __restrict__ dist, int* __restrict__ pix_counts) {
  __shared__ float s_cx[SG_CHUNK], s_cy[SG_CHUNK];
  __shared__ int s_hist[SG_CHUNK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int hw = H * W;
  const int n = min(counts[b], max_centers);
  const float* fgp = fg + (size_t)b * hw;
  const float* dxp = off + (size_t)b * 2 * hw;
  const float* dyp = dxp + hw;
  const int* cxy = centers + (size_t)b * max_centers * 2;
  const int p0 = blockIdx.x * (256 * SG_PIX) + tid;
  bool isfg[SG_PIX];
  float px[SG_PIX], py[SG_PIX], best[SG_PIX];
  int besti[SG_PIX];
#pragma unroll
  for (int e = 0; e < SG_PIX; ++e) {
    const int p = p0 + e * 256;
    isfg[e] = false;
    px[e] = py[e] = 0.f;
    best[e] = __builtin_inff();
    besti[e] = 0;
    if (p < hw && fgp[p] > fg_thr) {
      isfg[e] = true;
      const int y = p / W, x = p - y * W;
      // pixel_x = x * stride + stride / 2, then + dx: three roundings (segmentation.py:171-176)
      const float bx = (float)x * stride + half, by = (float)y * stride + half;
      px[e] = bx + dxp[p];
      py[e] = by + dyp[p];
    }
  }
  for (int c0 = 0; c0 < n; c0 += SG_CHUNK) {
    const int m = min(SG_CHUNK, n - c0);
    __syncthreads();
    for (int i = tid; i < m; i += 256) {
      s_cx[i] = (float)cxy[2 * (c0 + i)] * stride + half;
      s_cy[i] = (float)cxy[2 * (c0 + i) + 1] * stride + half;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < SG_PIX; ++e) {
      if (!isfg[e]) continue;
      float bd = best[e];
      int bi = besti[e];
      for (int i = 0; i < m; ++i) {
        const float ddx = px[e] - s_cx[i], ddy = py[e] - s_cy[i];
        const float a = ddx * ddx, c = ddy * ddy;
        const float d = a + c;
        if (d < bd || (d != d && bd == bd)) {  // first minimum; a NaN wins over numbers, the first one over later ones (torch.argmin)
          bd = d;
          bi = c0 + i;
        }
      }
      best[e] = bd;
      besti[e] = bi;
    }
  }
  SegHist hist;
  hist.init(s_hist, pix_counts + (size_t)b * max_centers, n);
#pragma unroll
  for (int e = 0; e < SG_PIX; ++e) {
    const int p = p0 + e * 256;
    if (p >= hw) continue;
    const bool on = isfg[e] && n > 0;
    labels[(size_t)b * hw + p] = on ? (LT)besti[e] : (LT)-1;
    if (dist) dist[(size_t)b * hw + p] = on ? best[e] : 0.f;
    if (on) hist.add(besti[e]);
  }
  hist.flush();
}

template <typename LT>
__global__ __launch_bounds__(256) void seg_gate_kernel(const LT* __restrict__ labels_in, const float* __restrict__ dist, int hw, float alpha, float stride,
                                                       const int* __restrict__ counts, int max_centers, const int* __restrict__ cnt_in, int* __restrict__ cnt_out,
                                                       LT* __restrict__ labels_out) {
  __shared__ int s_hist[SG_CHUNK];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int n = min(counts[b], max_centers);
  SegHist hist;
  hist.init(s_hist, cnt_out + (size_t)b * max_centers, n);
  const int p0 = blockIdx.x * (256 * SG_PIX) + tid;
#pragma unroll
  for (int e = 0; e < SG_PIX; ++e) {
    const int p = p0 + e * 256;
    if (p >= hw) continue;
    const int l = (int)labels_in[(size_t)b * hw + p];
    bool keep = false;
    if (l >= 0) {
      // r2 = (alpha * sqrt(count / pi) * stride)^2, fp32, in this order (segmentation.py:209-211)
      const float q = (float)cnt_in[(size_t)b * max_centers + l] / 3.14159274101257324f;
      const float rg = alpha * __fsqrt_rn(q);
      const float rp = rg * stride;
      keep = dist[(size_t)b * hw + p] <= rp * rp;
    }
    if (keep) hist.add(l);
    if (labels_out) labels_out[(size_t)b * hw + p] = keep ? (LT)l : (LT)-1;
  }
  hist.flush();
}

// ---- semantic -----------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void seg_sem_kernel(const float* __restrict__ fg, int hw, float thr, uint8_t* __restrict__ mask, int* __restrict__ part_cnt,
                                                      double* __restrict__ part_sum) {
  __shared__ int s_c[4];
  __shared__ double s_s[4];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int p0 = blockIdx.x * (256 * SG_PIX) + tid;
  int c = 0;
  double s = 0.0;
#pragma unroll
  for (int e = 0; e < SG_PIX; ++e) {
    const int p = p0 + e * 256;
    if (p >= hw) continue;
    const float v = fg[(size_t)b * hw + p];
    const bool on = v > thr;
    mask[(size_t)b * hw + p] = on ? 1 : 0;
    if (on) {
      ++c;
      s += (double)v;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    s += __shfl_xor(s, d, 64);
  }
  if ((tid & 63) == 0) {
    s_c[tid >> 6] = c;
    s_s[tid >> 6] = s;
  }
  __syncthreads();
  if (tid == 0) {
    part_cnt[(size_t)b * gridDim.x + blockIdx.x] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    part_sum[(size_t)b * gridDim.x + blockIdx.x] = ((s_s[0] + s_s[1]) + s_s[2]) + s_s[3];
  }
}

__global__ __launch_bounds__(64) void seg_sem_final_kernel(const int* __restrict__ part_cnt, const double* __restrict__ part_sum, int n_part, int* __restrict__ count,
                                                           double* __restrict__ sum) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int c = 0;
  double s = 0.0;
  for (int i = lane; i < n_part; i += 64) {  // (fixed order: lane-strided partials, then the butterfly)
    c += part_cnt[(size_t)b * n_part + i];
    s += part_sum[(size_t)b * n_part + i];
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    c += __shfl_xor(c, d, 64);
    s += __shfl_xor(s, d, 64);
  }
  if (lane == 0) {
    count[b] = c;
    sum[b] = s;
  }
}

// Output pixel (y, x) of slot s with crop k = pos_of_slot[s] >= 0 and record (ox, oy, He, We) = geom[k]:
//   v = y - oy, u = x - ox;  0 <= v < He and 0 <= u < We  ->  masks[k][(v * h) / He][(u * w) / We], else 0.
// h, w <= 32767 (checked on the host) and extents outside [1, 65535] make the crop empty, so both products fit 32 bits; coordinate
// differences are taken in unsigned arithmetic after the sign test, so no origin can overflow them.  `total` = B P H W < 2^32.
__global__ __launch_bounds__(256) void seg_place_kernel(const uint8_t* __restrict__ masks, const int* __restrict__ pos_of_slot, const int* __restrict__ geom, int N, int h,
                                                        int w, int slots, int H, int W, uint32_t total, uint8_t* __restrict__ out) {
  const uint32_t n_chunks = total / 16u + (total % 16u != 0u);
  const uint32_t step = gridDim.x * 256u;
  for (uint32_t c = blockIdx.x * 256u + threadIdx.x; c < n_chunks; c += step) {
    const uint32_t i0 = c * 16u;
    const uint32_t row0 = i0 / (uint32_t)W;
    int x = (int)(i0 - row0 * (uint32_t)W);
    int slot = (int)(row0 / (uint32_t)H);
    int y = (int)(row0 - (uint32_t)slot * (uint32_t)H);
    const uint8_t* src = nullptr;  // the crop row that output row (slot, y) reads, or null: the row is zero
    int ox = 0;
    uint32_t We = 0u;
    auto load_row = [&]() {
      src = nullptr;
      if (slot >= slots) return;  // (stepping off the end of the last row)
      const int k = pos_of_slot[slot];
      if (k < 0 || k >= N) return;
      const int gx = geom[4 * k], gy = geom[4 * k + 1], He = geom[4 * k + 2], we = geom[4 * k + 3];
      if (He < 1 || He > 65535 || we < 1 || we > 65535 || gy > y) return;
      const uint32_t v = (uint32_t)y - (uint32_t)gy;
      if (v >= (uint32_t)He) return;
      src = masks + ((size_t)k * h + (v * (uint32_t)h) / (uint32_t)He) * w;
      ox = gx;
      We = (uint32_t)we;
    };
    load_row();
    const int n = (int)min(16u, total - i0);
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    uint32_t q = 0u, r = 0u;  // source column of the current pixel and the remainder (u * w) % We
    bool stepping = false;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (i < n) {
        uint32_t px = 0u;
        if (src && x >= ox) {
          const uint32_t u = (uint32_t)x - (uint32_t)ox;
          if (u < We) {
            if (!stepping) {
              const uint32_t t = u * (uint32_t)w;
              q = u ? t / We : 0u;
              r = t - q * We;
              stepping = true;
            }
            px = src[q];
            r += (uint32_t)w;
            while (r >= We) {
              r -= We;
              ++q;
            }
          }
        }
        word[i >> 2] |= px << (8 * (i & 3));
        if (++x == W) {
          x = 0;
          if (++y == H) {
            y = 0;
            ++slot;
          }
          load_row();
          stepping = false;
        }
      }
    }
    if (n == 16) {
      reinterpret_cast<uint4*>(out)[c] = make_uint4(word[0], word[1], word[2], word[3]);
    } else {  // the last, short chunk of the array
#pragma unroll
      for (int i = 0; i < 16; ++i)
        if (i < n) out[(size_t)i0 + i] = (uint8_t)(word[i >> 2] >> (8 * (i & 3)));
    }
  }
}

static inline int seg_pix_blocks(int hw) { return (hw + 256 * SG_PIX - 1) / (256 * SG_PIX); }

}  // namespace ph

using namespace ph;

#define PH_SEG_SHAPE(fn)                                                                                       \
  PH_REQUIRE(B > 0 && h > 0 && w > 0, fn ": bad map shape B=%d h=%d w=%d", B, h, w);                           \
  PH_REQUIRE((int64_t)h * w <= 0x7fffffffLL && B <= 65535, fn ": map too large (B=%d h=%d w=%d)", B, h, w)

extern "C" int64_t ph_seg_scratch_bytes(int32_t B, int32_t h, int32_t w, int32_t cap) {
  if (B <= 0 || h <= 0 || w <= 0 || cap <= 0) return 0;
  const int64_t groups = (h + SG_ROWS - 1) / SG_ROWS;
  int64_t ints = B * groups + B * groups * SG_ROWS * w;
  ints = align_up(ints, 2);
  if (cap > SG_LDS_CAND) ints += (int64_t)B * 4 * cap;
  return ints * 4;
}

extern "C" int ph_seg_center_peaks(const float* center_dev, int32_t B, int32_t h, int32_t w, float threshold, int32_t nms_kernel, int32_t max_instances, int32_t cap,
                                   int32_t max_centers, int32_t* centers_dev, float* scores_dev, int32_t* counts_dev, int32_t* pix_counts_dev, int32_t n_count_bufs,
                                   void* scratch_dev, int64_t scratch_bytes, void* stream) {
  PH_REQUIRE(center_dev && centers_dev && scores_dev && counts_dev && pix_counts_dev && scratch_dev, "ph_seg_center_peaks: null pointer");
  PH_SEG_SHAPE("ph_seg_center_peaks");
  PH_REQUIRE(nms_kernel == 3 || nms_kernel == 5 || nms_kernel == 7, "ph_seg_center_peaks: center_nms_kernel must be 3, 5 or 7, got %d", nms_kernel);
  PH_REQUIRE(cap > 0 && max_centers > 0 && n_count_bufs > 0, "ph_seg_center_peaks: cap=%d max_centers=%d n_count_bufs=%d must be positive", cap, max_centers, n_count_bufs);
  PH_REQUIRE(((uintptr_t)scratch_dev & 7) == 0, "ph_seg_center_peaks: scratch must be 8-byte aligned");
  const int64_t need = ph_seg_scratch_bytes(B, h, w, cap);
  if (scratch_bytes < need) {
    set_error("ph_seg_center_peaks: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
    return PH_E_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int groups = (h + SG_ROWS - 1) / SG_ROWS;
  int* blk_count = static_cast<int*>(scratch_dev);
  int* stage = blk_count + (size_t)B * groups;
  int* glist = static_cast<int*>(scratch_dev) + align_up((int64_t)B * groups + (int64_t)B * groups * SG_ROWS * w, 2);
  hipLaunchKernelGGL(seg_cand_kernel, dim3(B * groups), dim3(256), 0, s, center_dev, h, w, threshold, nms_kernel / 2, groups, blk_count, stage);
  hipLaunchKernelGGL(seg_collapse_kernel, dim3(B), dim3(256), 0, s, center_dev, B, h, w, groups, blk_count, stage, cap, max_centers, max_instances, glist, centers_dev,
                     scores_dev, counts_dev, pix_counts_dev, n_count_bufs);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

extern "C" int ph_seg_assign(const float* fg_dev, const float* offsets_dev, int32_t B, int32_t h, int32_t w, float fg_threshold, int32_t output_stride,
                             const int32_t* centers_dev, const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes, void* labels_dev, float* dist_dev,
                             int32_t* pix_counts_dev, void* stream) {
  PH_REQUIRE(fg_dev && offsets_dev && centers_dev && counts_dev && labels_dev && pix_counts_dev, "ph_seg_assign: null pointer");
  PH_SEG_SHAPE("ph_seg_assign");
  PH_REQUIRE(output_stride > 0 && max_centers > 0, "ph_seg_assign: output_stride=%d max_centers=%d must be positive", output_stride, max_centers);
  PH_REQUIRE((label_bytes == 1 && max_centers <= 127) || (label_bytes == 2 && max_centers <= 32767) || label_bytes == 4,
             "ph_seg_assign: %d-byte labels cannot hold %d centres", label_bytes, max_centers);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(seg_pix_blocks(h * w), B);
  const float st = (float)output_stride, half = (float)(output_stride / 2.0);
#define PH_SEG_ASSIGN(LT) \
  hipLaunchKernelGGL((seg_assign_kernel<LT>), grid, dim3(256), 0, s, fg_dev, offsets_dev, h, w, fg_threshold, st, half, centers_dev, counts_dev, max_centers, static_cast<LT*>(labels_dev), dist_dev, pix_counts_dev)
  if (label_bytes == 1) PH_SEG_ASSIGN(int8_t);
  else if (label_bytes == 2) PH_SEG_ASSIGN(int16_t);
  else PH_SEG_ASSIGN(int32_t);
#undef PH_SEG_ASSIGN
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

extern "C" int ph_seg_gate(const void* labels_in_dev, const float* dist_dev, int32_t B, int32_t h, int32_t w, float alpha, int32_t output_stride, int32_t iters,
                           const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes, int32_t* pix_counts_dev, void* labels_out_dev, void* stream) {
  PH_REQUIRE(labels_in_dev && dist_dev && counts_dev && pix_counts_dev && labels_out_dev, "ph_seg_gate: null pointer");
  PH_REQUIRE(labels_in_dev != labels_out_dev, "ph_seg_gate: the gated label map needs a buffer of its own (every pass re-reads the assignment)");
  PH_SEG_SHAPE("ph_seg_gate");
  PH_REQUIRE(iters >= 1 && output_stride > 0 && max_centers > 0, "ph_seg_gate: iters=%d output_stride=%d max_centers=%d must be positive", iters, output_stride, max_centers);
  PH_REQUIRE(label_bytes == 1 || label_bytes == 2 || label_bytes == 4, "ph_seg_gate: label_bytes must be 1, 2 or 4, got %d", label_bytes);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(seg_pix_blocks(h * w), B);
  const size_t buf = (size_t)B * max_centers;
  for (int k = 0; k < iters; ++k) {
    const int* cin = pix_counts_dev + (size_t)k * buf;
    int* cout = pix_counts_dev + (size_t)(k + 1) * buf;
    const bool last = k + 1 == iters;
#define PH_SEG_GATE(LT) \
  hipLaunchKernelGGL((seg_gate_kernel<LT>), grid, dim3(256), 0, s, static_cast<const LT*>(labels_in_dev), dist_dev, h * w, alpha, (float)output_stride, counts_dev, max_centers, cin, cout, last ? static_cast<LT*>(labels_out_dev) : (LT*)nullptr)
    if (label_bytes == 1) PH_SEG_GATE(int8_t);
    else if (label_bytes == 2) PH_SEG_GATE(int16_t);
    else PH_SEG_GATE(int32_t);
#undef PH_SEG_GATE
  }
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

extern "C" int64_t ph_seg_semantic_scratch_bytes(int32_t B, int32_t h, int32_t w) {
  if (B <= 0 || h <= 0 || w <= 0) return 0;
  return (int64_t)B * seg_pix_blocks(h * w) * 16;
}

extern "C" int ph_seg_semantic(const float* fg_dev, int32_t B, int32_t h, int32_t w, float fg_threshold, uint8_t* mask_dev, int32_t* count_dev, double* sum_dev,
                               void* scratch_dev, int64_t scratch_bytes, void* stream) {
  PH_REQUIRE(fg_dev && mask_dev && count_dev && sum_dev && scratch_dev, "ph_seg_semantic: null pointer");
  PH_SEG_SHAPE("ph_seg_semantic");
  PH_REQUIRE(((uintptr_t)scratch_dev & 7) == 0 && ((uintptr_t)sum_dev & 7) == 0, "ph_seg_semantic: scratch and sums must be 8-byte aligned");
  const int64_t need = ph_seg_semantic_scratch_bytes(B, h, w);
  if (scratch_bytes < need) {
    set_error("ph_seg_semantic: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)need);
    return PH_E_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = seg_pix_blocks(h * w);
  double* part_sum = static_cast<double*>(scratch_dev);
  int* part_cnt = reinterpret_cast<int*>(part_sum + (size_t)B * nb);
  hipLaunchKernelGGL(seg_sem_kernel, dim3(nb, B), dim3(256), 0, s, fg_dev, h * w, fg_threshold, mask_dev, part_cnt, part_sum);
  hipLaunchKernelGGL(seg_sem_final_kernel, dim3(B), dim3(64), 0, s, part_cnt, part_sum, nb, count_dev, sum_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

extern "C" int ph_seg_place_crops(const uint8_t* masks_dev, int32_t N, int32_t h, int32_t w, const int32_t* pos_of_slot_dev, const int32_t* geom_dev, int32_t B, int32_t P,
                                  int32_t H, int32_t W, uint8_t* out_dev, void* stream) {
  PH_REQUIRE(pos_of_slot_dev && out_dev && (N == 0 || (masks_dev && geom_dev)), "ph_seg_place_crops: null pointer");
  PH_REQUIRE(P >= 1 && P <= 64, "ph_seg_place_crops: P=%d must lie in [1, 64] (the mask evaluator's limit)", P);
  PH_REQUIRE(B > 0 && H > 0 && W > 0 && N >= 0, "ph_seg_place_crops: bad shape B=%d H=%d W=%d N=%d", B, H, W, N);
  PH_REQUIRE(N == 0 || (h >= 1 && h <= 32767 && w >= 1 && w <= 32767), "ph_seg_place_crops: crop masks of %d x %d; each side must lie in [1, 32767]", h, w);
  const int64_t total = (int64_t)B * P * H * W;
  PH_REQUIRE(total <= 0xffffffffLL, "ph_seg_place_crops: output of %lld bytes; at most 2^32 - 1 per call", (long long)total);
  PH_REQUIRE(((uintptr_t)out_dev & 15) == 0, "ph_seg_place_crops: the output must be 16-byte aligned");
  const int64_t chunks = (total + 15) / 16;
  const int blocks = (int)std::min<int64_t>((chunks + 255) / 256, 1 << 20);
  hipLaunchKernelGGL(seg_place_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), masks_dev, pos_of_slot_dev, geom_dev, N, h, w, B * P, H, W,
                     (uint32_t)total, out_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
