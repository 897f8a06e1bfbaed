// Bottom-up instance segmentation: mask cleanup on the device (sleap_nn/inference/segmentation.py:224-273, _clean_instance_mask at
// radius 0): per instance keep the largest 4-connected component (raster-first on ties) and fill its interior holes.  Runs on the
// label map ph_seg_assign / ph_seg_gate leave on the device, on the caller's stream, no host synchronisation.  Integer-only: every
// result is exact and identical from run to run, whatever the scheduling.
//
// Component pass, the whole label map at once (two neighbouring pixels are joined when they carry the same non-negative label):
//   * cl_init_kernel: per (frame, label) records (best key, bounding box, counters).
//   * cl_tile_kernel: one block per (frame, 16 x 64 tile).  Min-label propagation with pointer jumping in LDS until a sweep changes
//     nothing: every tile-local component is labelled by its raster-first pixel.  Writes the parent plane (frame pixel index of the
//     local root) and, at local roots, the component's pixel count and bounding box inside the tile (LDS integer atomics).
//   * cl_merge_kernel: pixels on a tile's left / top border with an equal neighbour across it unite the two trees in the global
//     int32 parent plane: find both roots, hang the larger on the smaller with atomicMin, repeat with what was there if another
//     thread came first.  Parents only ever point to smaller pixel indices, so each component ends rooted at its raster-first pixel.
//   * cl_flatten_kernel: parent <- root for every labelled pixel; local roots add their tile's count to area[root] (integer atomics).
//   * cl_select_kernel: each root: one 64-bit atomicMax of (area << 32) | ~root per (frame, label): largest area, raster-first on ties.
//   * cl_write_kernel: the cleaned label map (pixels of dropped components -> -1) in the input's type; local roots of the kept
//     component merge their tile boxes into the (frame, label) bounding box.
// Hole pass, one workgroup per (frame, instance), over the kept component's bounding box grown by a one-pixel ring (everything
// outside that box is connected to the image border, and so is the ring; a ring cell outside the image stands for the outside):
//   * the box bit-packed, one 64-bit word per 64 columns: `free` = not the component, `reach` = free cells known to connect to the
//     ring.  A thread owns rows: it ORs in the rows above and below, ANDs with free, and floods along the row by carry propagation
//     ((free + seed) ^ free) & free, left to right and (bit-reversed) right to left with the carry handed from word to word; sweeps
//     repeat until a workgroup-wide vote sees no change.  Bits only ever get set, so reading a neighbour row while it changes is harmless.
//   * holes = free & ~reach.  The bitmaps live in LDS up to CL_LDS_WORDS words each (60 KiB of the CU's 160 KiB together: two
//     workgroups stay resident) and in a pool of the caller's scratch beyond; a frame whose large boxes need more pool than it has
//     reports the need and the caller comes back with room, as for the candidate list of ph_seg_center_peaks.
//   * first launch: hole counts and cleaned areas per instance; second launch: each instance's offset is the sum of the counts
//     before it (exclusive scan, instance-major) and its holes are written in raster order as int32 pairs (pixel index, label).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

namespace ph {

constexpr int CL_TH = 16, CL_TW = 64;        // tile of the component pass
constexpr int CL_TILE = CL_TH * CL_TW;       // 1024 pixels, 4 per thread
constexpr int CL_LDS_WORDS = 3840;           // 64-bit words per bitmap kept in LDS (two bitmaps: 60 KiB)

typedef unsigned long long u64;

__device__ __forceinline__ int cl_scan256(int v, int* total, int* lds /* >= 4 ints */) {
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

// per (frame, label): best = 0 (no component), box = empty; per frame: counters = 0
__global__ __launch_bounds__(256) void cl_init_kernel(int B, int max_centers, u64* __restrict__ best, int* __restrict__ box, int* __restrict__ rec_area,
                                                      int* __restrict__ rec_holes, int* __restrict__ rec_total, int* __restrict__ rec_pool) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < B * max_centers) {
    best[i] = 0ull;
    box[4 * i] = 0x7fffffff;
    box[4 * i + 1] = 0x7fffffff;
    box[4 * i + 2] = -1;
    box[4 * i + 3] = -1;
    rec_area[i] = 0;
    rec_holes[i] = 0;
  }
  if (i < B) {
    rec_total[i] = 0;
    rec_pool[i] = 0;
  }
}

template <typename LT>
__global__ __launch_bounds__(256) void cl_tile_kernel(const LT* __restrict__ labels, int H, int W, int tiles_x, int* __restrict__ parent, int* __restrict__ cnt,
                                                      int* __restrict__ area, int* __restrict__ bb_lo, int* __restrict__ bb_hi) {
  __shared__ int s_lab[CL_TILE];  // tile-local index of the smallest known member of the pixel's component
  __shared__ int s_val[CL_TILE];  // the pixel's label, -1 outside the image
  __shared__ int s_cnt[CL_TILE];
  __shared__ int s_x0[CL_TILE], s_y0[CL_TILE], s_x1[CL_TILE], s_y1[CL_TILE];
  const int b = blockIdx.y, tid = threadIdx.x;
  const int ty0 = (blockIdx.x / tiles_x) * CL_TH, tx0 = (blockIdx.x % tiles_x) * CL_TW;
  const size_t plane = (size_t)b * H * W;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = tid + e * 256;
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    s_val[i] = (y < H && x < W) ? (int)labels[plane + (size_t)y * W + x] : -1;
    s_lab[i] = i;
    s_cnt[i] = 0;
    s_x0[i] = 0x7fffffff;
    s_y0[i] = 0x7fffffff;
    s_x1[i] = -1;
    s_y1[i] = -1;
  }
  __syncthreads();
  // A thread writes s_lab of its own pixels only and labels only ever decrease to members of the same component, so a neighbour's
  // label read while it changes is harmless; a sweep that changes nothing has read final values everywhere.
  volatile int* vlab = s_lab;
  int again;
  do {
    int ch = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int i = tid + e * 256;
      const int v = s_val[i];
      if (v < 0) continue;
      const int r = i >> 6, c = i & 63;
      const int cur = vlab[i];
      int m = cur;
      if (c > 0 && s_val[i - 1] == v) m = min(m, vlab[i - 1]);
      if (c < CL_TW - 1 && s_val[i + 1] == v) m = min(m, vlab[i + 1]);
      if (r > 0 && s_val[i - CL_TW] == v) m = min(m, vlab[i - CL_TW]);
      if (r < CL_TH - 1 && s_val[i + CL_TW] == v) m = min(m, vlab[i + CL_TW]);
      m = min(m, vlab[m]);  // pointer jump
      if (m < cur) {
        vlab[i] = m;
        ch = 1;
      }
    }
    again = __syncthreads_or(ch);
  } while (again);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = tid + e * 256;
    if (s_val[i] < 0) continue;
    const int root = s_lab[i];
    atomicAdd(&s_cnt[root], 1);
    atomicMin(&s_x0[root], tx0 + (i & 63));
    atomicMax(&s_x1[root], tx0 + (i & 63));
    atomicMin(&s_y0[root], ty0 + (i >> 6));
    atomicMax(&s_y1[root], ty0 + (i >> 6));
  }
  __syncthreads();
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int i = tid + e * 256;
    const int y = ty0 + (i >> 6), x = tx0 + (i & 63);
    if (y >= H || x >= W) continue;
    const int p = y * W + x;
    const int root = s_lab[i];
    parent[plane + p] = (ty0 + (root >> 6)) * W + tx0 + (root & 63);  // (a background pixel: itself)
    const int c = s_cnt[i];
    cnt[plane + p] = c;
    area[plane + p] = 0;
    if (c > 0) {  // a local root; h, w <= 32767, so two coordinates fit one word
      bb_lo[plane + p] = (s_y0[i] << 16) | s_x0[i];
      bb_hi[plane + p] = (s_y1[i] << 16) | s_x1[i];
    }
  }
}

__device__ __forceinline__ int cl_find(int* parent, int a) {
  for (;;) {
    const int p = __hip_atomic_load(&parent[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == a) return a;
    a = p;
  }
}

__device__ __forceinline__ void cl_union(int* parent, int a, int c) {
  for (;;) {
    a = cl_find(parent, a);
    c = cl_find(parent, c);
    if (a == c) return;
    if (a < c) {
      const int t = a;
      a = c;
      c = t;
    }
    const int old = atomicMin(&parent[a], c);  // a > c: hang the later root on the earlier one
    if (old == a) return;
    a = old;  // another thread hung a first: unite what it pointed to with c
  }
}

template <typename LT>
__global__ __launch_bounds__(256) void cl_merge_kernel(const LT* __restrict__ labels, int H, int W, int* __restrict__ parent) {
  const int b = blockIdx.y;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int y = p / W, x = p - y * W;
  const bool left = x > 0 && (x % CL_TW) == 0, up = y > 0 && (y % CL_TH) == 0;
  if (!left && !up) return;
  const LT* lab = labels + (size_t)b * H * W;
  int* par = parent + (size_t)b * H * W;
  const int v = (int)lab[p];
  if (v < 0) return;
  if (left && (int)lab[p - 1] == v) cl_union(par, p, p - 1);
  if (up && (int)lab[p - W] == v) cl_union(par, p, p - W);
}

template <typename LT>
__global__ __launch_bounds__(256) void cl_flatten_kernel(const LT* __restrict__ labels, int hw, int* __restrict__ parent, const int* __restrict__ cnt,
                                                         int* __restrict__ area) {
  const size_t plane = (size_t)blockIdx.y * hw;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw || (int)labels[plane + p] < 0) return;
  int* par = parent + plane;
  const int r = cl_find(par, p);
  __hip_atomic_store(&par[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // (a thread walking through p sees its old parent or the root)
  const int c = cnt[plane + p];
  if (c > 0) atomicAdd(&area[plane + r], c);
}

template <typename LT>
__global__ __launch_bounds__(256) void cl_select_kernel(const LT* __restrict__ labels, int hw, const int* __restrict__ parent, const int* __restrict__ area,
                                                        const int* __restrict__ counts, int max_centers, u64* __restrict__ best) {
  const int b = blockIdx.y;
  const size_t plane = (size_t)b * hw;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int l = (int)labels[plane + p];
  if (l < 0 || l >= min(counts[b], max_centers) || parent[plane + p] != p) return;
  atomicMax(&best[(size_t)b * max_centers + l], ((u64)(unsigned)area[plane + p] << 32) | (u64)(0xFFFFFFFFu - (unsigned)p));
}

template <typename LT>
__global__ __launch_bounds__(256) void cl_write_kernel(const LT* __restrict__ labels, int hw, const int* __restrict__ parent, const int* __restrict__ cnt,
                                                       const int* __restrict__ bb_lo, const int* __restrict__ bb_hi, const int* __restrict__ counts, int max_centers,
                                                       const u64* __restrict__ best, LT* __restrict__ out, int* __restrict__ box) {
  const int b = blockIdx.y;
  const size_t plane = (size_t)b * hw;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= hw) return;
  const int l = (int)labels[plane + p];
  bool keep = false;
  if (l >= 0 && l < min(counts[b], max_centers)) {
    const u64 key = best[(size_t)b * max_centers + l];
    keep = key != 0ull && parent[plane + p] == (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull));
  }
  out[plane + p] = keep ? (LT)l : (LT)-1;
  if (keep && cnt[plane + p] > 0) {
    int* bx = box + ((size_t)b * max_centers + l) * 4;
    const int lo = bb_lo[plane + p], hi = bb_hi[plane + p];
    atomicMin(&bx[0], lo & 0xffff);
    atomicMin(&bx[1], lo >> 16);
    atomicMax(&bx[2], hi & 0xffff);
    atomicMax(&bx[3], hi >> 16);
  }
}

// seeds (a subset of free) spread along the runs of free towards higher bits: adding a seed to its run carries to the run's end
__device__ __forceinline__ u64 cl_fill_up(u64 free, u64 seed) { return (((free + seed) ^ free) & free) | seed; }

template <typename LT, bool WRITE>
__global__ __launch_bounds__(256) void cl_hole_kernel(const LT* __restrict__ cleaned, int H, int W, const int* __restrict__ counts, int max_centers,
                                                      const u64* __restrict__ best, const int* __restrict__ box, u64* __restrict__ pool, int pool_words,
                                                      int* __restrict__ pool_off, int* __restrict__ rec_area, int* __restrict__ rec_holes, int* __restrict__ rec_total,
                                                      int* __restrict__ rec_pool, int* __restrict__ holes, int hole_cap) {
  __shared__ u64 s_bits[2 * CL_LDS_WORDS];
  __shared__ int red[4];
  __shared__ int s_off;
  const int b = blockIdx.y, l = blockIdx.x, tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int n = min(counts[b], max_centers);
  if (l >= n) return;  // (block-uniform, like every return below)
  const size_t rec = (size_t)b * max_centers + l;
  int base = 0;
  if (WRITE) {  // offset = the holes of the instances before this one; the last instance also records the frame's total
    int part = 0;
    for (int k = tid; k < l; k += 256) part += rec_holes[(size_t)b * max_centers + k];
    int tot;
    const int ex = cl_scan256(part, &tot, red);
    (void)ex;
    base = tot;
    const int mine = rec_holes[rec];
    if (l == n - 1 && tid == 0) rec_total[b] = base + mine;
    if (mine == 0) return;
  }
  const u64 key = best[rec];
  if (key == 0ull) return;  // no pixels: area 0, no holes (cl_init_kernel wrote both)
  const int area = (int)(key >> 32);
  const int x0 = box[4 * rec], y0 = box[4 * rec + 1], x1 = box[4 * rec + 2], y1 = box[4 * rec + 3];
  if (y1 - y0 < 2 || x1 - x0 < 2) {  // a hole has component pixels on all four sides: the box is at least 3 x 3
    if (tid == 0) rec_area[rec] = area;
    return;
  }
  const int R = y1 - y0 + 3, C = x1 - x0 + 3;  // the box and its ring
  const int wpr = (C + 63) >> 6;
  const int nw = R * wpr;
  u64* fr;
  u64* rc0;
  if (nw <= CL_LDS_WORDS) {
    fr = s_bits;
    rc0 = s_bits + nw;
  } else {
    if (!WRITE) {
      if (tid == 0) {
        s_off = atomicAdd(&rec_pool[b], 2 * nw);
        pool_off[rec] = s_off;
      }
      __syncthreads();
    } else if (tid == 0) {
      s_off = pool_off[rec];
    }
    if (WRITE) __syncthreads();
    const int off = s_off;
    if (off < 0 || (int64_t)off + 2 * (int64_t)nw > (int64_t)pool_words) {  // no room: the frame's need is in rec_pool, the caller comes back
      if (tid == 0) rec_area[rec] = area;
      return;
    }
    fr = pool + (size_t)b * pool_words + off;
    rc0 = fr + nw;
  }
  volatile u64* rc = rc0;
  const LT* lab = cleaned + (size_t)b * H * W;
  const int last_wd = (C - 1) >> 6;
  const u64 last_bit = 1ull << ((C - 1) & 63);
  for (int wi = wave; wi < nw; wi += 4) {
    const int r = wi / wpr, wd = wi - r * wpr;
    const int c = wd * 64 + lane;
    const int y = y0 - 1 + r, x = x0 - 1 + c;
    const bool in = c < C;
    const bool comp = in && y >= 0 && y < H && x >= 0 && x < W && (int)lab[(size_t)y * W + x] == l;
    const u64 cm = __ballot(comp), colmask = __ballot(in);
    if (lane == 0) {
      const u64 f = ~cm & colmask;
      const u64 ring = (r == 0 || r == R - 1) ? colmask : ((wd == 0 ? 1ull : 0ull) | (wd == last_wd ? last_bit : 0ull));
      fr[wi] = f;
      rc[wi] = f & ring;
    }
  }
  __syncthreads();
  int again;
  do {
    int ch = 0;
    for (int r = tid; r < R; r += 256) {
      u64 carry = 0ull;
      for (int wd = 0; wd < wpr; ++wd) {
        const int i = r * wpr + wd;
        const u64 f = fr[i], old = rc[i];
        u64 s = old | carry;
        if (r > 0) s |= rc[i - wpr];
        if (r < R - 1) s |= rc[i + wpr];
        const u64 up = cl_fill_up(f, s & f);
        carry = up >> 63;
        if (up != old) {
          rc[i] = up;
          ch = 1;
        }
      }
      carry = 0ull;
      for (int wd = wpr - 1; wd >= 0; --wd) {
        const int i = r * wpr + wd;
        const u64 f = fr[i], old = rc[i];
        const u64 s = (old | (carry << 63)) & f;
        const u64 dn = __brevll(cl_fill_up(__brevll(f), __brevll(s)));
        carry = dn & 1ull;
        if (dn != old) {
          rc[i] = dn;
          ch = 1;
        }
      }
    }
    again = __syncthreads_or(ch);
  } while (again);
  // holes: free cells the flood never reached, in raster order
  int run = 0;
  for (int i0 = 0; i0 < nw; i0 += 256) {
    const int i = i0 + tid;
    u64 hb = i < nw ? (fr[i] & ~rc[i]) : 0ull;
    int tot;
    const int ex = cl_scan256(__popcll(hb), &tot, red);
    if (WRITE) {
      const int r = i / wpr, wd = i - r * wpr;
      int pos = base + run + ex;
      while (hb) {
        const int bit = __ffsll((long long)hb) - 1;
        hb &= hb - 1ull;
        if (pos < hole_cap) {
          int* dst = holes + ((size_t)b * hole_cap + pos) * 2;
          dst[0] = (y0 - 1 + r) * W + (x0 - 1 + wd * 64 + bit);
          dst[1] = l;
        }
        ++pos;
      }
    }
    run += tot;
  }
  if (!WRITE && tid == 0) {
    rec_holes[rec] = run;
    rec_area[rec] = area + run;
  }
}

struct ClLayout {
  int64_t parent, cnt, area, bb_lo, bb_hi, best, box, pool_off, pool, total;  // byte offsets
};

static inline ClLayout cl_layout(int64_t B, int64_t h, int64_t w, int64_t mc, int64_t pool_words) {
  ClLayout L;
  const int64_t plane = align_up(B * h * w * 4, 8);
  L.parent = 0;
  L.cnt = plane;
  L.area = 2 * plane;
  L.bb_lo = 3 * plane;
  L.bb_hi = 4 * plane;
  L.best = 5 * plane;
  L.box = L.best + B * mc * 8;
  L.pool_off = L.box + B * mc * 16;
  L.pool = align_up(L.pool_off + B * mc * 4, 8);
  L.total = L.pool + B * pool_words * 8;
  return L;
}

}  // namespace ph

using namespace ph;

extern "C" int64_t ph_seg_cleanup_scratch_bytes(int32_t B, int32_t h, int32_t w, int32_t max_centers, int32_t pool_words) {
  if (B <= 0 || h <= 0 || w <= 0 || max_centers <= 0 || pool_words < 0) return 0;
  return cl_layout(B, h, w, max_centers, pool_words).total;
}

extern "C" int ph_seg_cleanup(const void* labels_in_dev, int32_t B, int32_t h, int32_t w, const int32_t* counts_dev, int32_t max_centers, int32_t label_bytes,
                              void* labels_out_dev, int32_t* record_dev, int32_t* holes_dev, int32_t hole_cap, int32_t pool_words, void* scratch_dev,
                              int64_t scratch_bytes, void* stream) {
  PH_REQUIRE(labels_in_dev && counts_dev && labels_out_dev && record_dev && holes_dev && scratch_dev, "ph_seg_cleanup: null pointer");
  PH_REQUIRE(labels_in_dev != labels_out_dev, "ph_seg_cleanup: the cleaned label map needs a buffer of its own");
  PH_REQUIRE(B > 0 && B <= 65535 && h > 0 && w > 0 && h <= 32767 && w <= 32767 && (int64_t)h * w <= 0x7fffffffLL,
             "ph_seg_cleanup: bad map shape B=%d h=%d w=%d (each side at most 32767)", B, h, w);
  PH_REQUIRE(max_centers > 0 && hole_cap > 0 && pool_words >= 0, "ph_seg_cleanup: max_centers=%d, hole_cap=%d must be positive, pool_words=%d not negative", max_centers,
             hole_cap, pool_words);
  PH_REQUIRE((label_bytes == 1 && max_centers <= 127) || (label_bytes == 2 && max_centers <= 32767) || label_bytes == 4,
             "ph_seg_cleanup: %d-byte labels cannot hold %d centres", label_bytes, max_centers);
  PH_REQUIRE(((uintptr_t)scratch_dev & 7) == 0, "ph_seg_cleanup: scratch must be 8-byte aligned");
  {  // a frame's pool need is summed in int32: a box beyond the LDS bitmaps spans ~1000 rows + columns, so its component has about as many pixels
    const int64_t full = 2 * ((int64_t)h + 2) * (((int64_t)w + 2 + 63) / 64);
    PH_REQUIRE(full * ((int64_t)h * w / 900 + 1) <= 0x7fffffffLL, "ph_seg_cleanup: map of %d x %d too large for the hole pass's pool accounting", h, w);
  }
  const ClLayout L = cl_layout(B, h, w, max_centers, pool_words);
  if (scratch_bytes < L.total) {
    set_error("ph_seg_cleanup: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, (long long)L.total);
    return PH_E_WORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  char* sc = static_cast<char*>(scratch_dev);
  int* parent = reinterpret_cast<int*>(sc + L.parent);
  int* cnt = reinterpret_cast<int*>(sc + L.cnt);
  int* area = reinterpret_cast<int*>(sc + L.area);
  int* bb_lo = reinterpret_cast<int*>(sc + L.bb_lo);
  int* bb_hi = reinterpret_cast<int*>(sc + L.bb_hi);
  u64* best = reinterpret_cast<u64*>(sc + L.best);
  int* box = reinterpret_cast<int*>(sc + L.box);
  int* pool_off = reinterpret_cast<int*>(sc + L.pool_off);
  u64* pool = reinterpret_cast<u64*>(sc + L.pool);
  const size_t bm = (size_t)B * max_centers;
  int* rec_area = record_dev;
  int* rec_holes = record_dev + bm;
  int* rec_total = record_dev + 2 * bm;
  int* rec_pool = rec_total + B;
  const int hw = h * w;
  const int tiles_x = (w + CL_TW - 1) / CL_TW, tiles_y = (h + CL_TH - 1) / CL_TH;
  const dim3 pix((hw + 255) / 256, B), inst(max_centers, B);
  hipLaunchKernelGGL(cl_init_kernel, dim3((int)((std::max<size_t>(bm, B) + 255) / 256)), dim3(256), 0, s, B, max_centers, best, box, rec_area, rec_holes, rec_total, rec_pool);
#define PH_CL_RUN(LT)                                                                                                                                              \
  do {                                                                                                                                                             \
    const LT* in = static_cast<const LT*>(labels_in_dev);                                                                                                          \
    LT* out = static_cast<LT*>(labels_out_dev);                                                                                                                    \
    hipLaunchKernelGGL((cl_tile_kernel<LT>), dim3(tiles_x * tiles_y, B), dim3(256), 0, s, in, h, w, tiles_x, parent, cnt, area, bb_lo, bb_hi);                     \
    hipLaunchKernelGGL((cl_merge_kernel<LT>), pix, dim3(256), 0, s, in, h, w, parent);                                                                             \
    hipLaunchKernelGGL((cl_flatten_kernel<LT>), pix, dim3(256), 0, s, in, hw, parent, cnt, area);                                                                  \
    hipLaunchKernelGGL((cl_select_kernel<LT>), pix, dim3(256), 0, s, in, hw, parent, area, counts_dev, max_centers, best);                                         \
    hipLaunchKernelGGL((cl_write_kernel<LT>), pix, dim3(256), 0, s, in, hw, parent, cnt, bb_lo, bb_hi, counts_dev, max_centers, best, out, box);                   \
    hipLaunchKernelGGL((cl_hole_kernel<LT, false>), inst, dim3(256), 0, s, out, h, w, counts_dev, max_centers, best, box, pool, pool_words, pool_off, rec_area,    \
                       rec_holes, rec_total, rec_pool, holes_dev, hole_cap);                                                                                       \
    hipLaunchKernelGGL((cl_hole_kernel<LT, true>), inst, dim3(256), 0, s, out, h, w, counts_dev, max_centers, best, box, pool, pool_words, pool_off, rec_area,     \
                       rec_holes, rec_total, rec_pool, holes_dev, hole_cap);                                                                                       \
  } while (0)
  if (label_bytes == 1) PH_CL_RUN(int8_t);
  else if (label_bytes == 2) PH_CL_RUN(int16_t);
  else PH_CL_RUN(int32_t);
#undef PH_CL_RUN
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
