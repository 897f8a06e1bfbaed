// Tiled inference: cut the frames of a batch into overlapping square tiles, and stitch the per-tile confidence maps back.
//
// Replaces the Python slicing of sleap_nn/inference/layers/tiled.py (_extract_square_tile per tile, TileMerger.integrate per
// tile + TileMerger.merge per frame, sleap_nn/inference/tile_merger.py:107-179) by two launches per batch:
//   * tile_extract_kernel: a pure copy.  The output is walked in 16-byte chunks (always aligned: chunks never straddle a tile
//     row); a chunk whose source lies inside the frame at a 16-byte-aligned (or, failing that, 4-byte-aligned) address is
//     loaded as vectors, anything else element by element with zeros past the frame's bottom / right edge.
//   * tile_merge_kernel: the stitch as a GATHER.  A thread owns 4 consecutive output pixels of one row and walks the tiles that
//     cover them in ascending tile index (iy outer, ix inner) -- the order in which TileMerger.integrate is called -- with
//     acc = acc + tile * w and cnt = cnt + w as separate float32 operations (no contraction), then acc / cnt.  That is the
//     reference's per-pixel sequence of roundings, so the result is bit-identical to its CPU canvas; there is no ACC / CNT
//     canvas, no atomics, and every tile element is read once.  cnt depends on the pixel only and is shared by the channels.
// Both are HBM-bound; a wave covers 256 consecutive pixels of a row, so tile-row and window-row segments are coalesced and
// the window (th x tw floats) stays in L2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"

// The stitch must round the product and the sum separately, as the torch canvas does.  hipcc contracts a * b + c into an FMA by
// default, and the __fmul_rn / __fadd_rn wrappers do not prevent it (they are plain operators compiled under the default, and fuse
// once inlined): the arithmetic below is written with plain operators under this pragma, and the build's ISA holds no FMA outside
// the division sequences.  Division is IEEE-correct (hipcc's default for fp32), denormals are kept (gfx9 default).
#pragma clang fp contract(off)

namespace ph {

// ---- extract ------------------------------------------------------------------------------------------------------

template <typename T>
struct alignas(16) Chunk16 {
  T v[16 / sizeof(T)];
};

// V = elements per output chunk: 16 / sizeof(T) (tile_size % V == 0, 16-byte-aligned output) or 1
template <typename T, int V>
__global__ __launch_bounds__(256) void tile_extract_kernel(const T* __restrict__ frames, T* __restrict__ out, const int32_t* __restrict__ yo,
                                                           const int32_t* __restrict__ xo, int F, int C, int H, int W, int ny, int nx, int ts) {
  const int tsv = ts / V;
  const int T_ = ny * nx;
  const size_t chunks = (size_t)F * T_ * C * ts * tsv;
  for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < chunks; k += (size_t)gridDim.x * 256) {
    const int xc = (int)(k % tsv);
    size_t r = k / tsv;
    const int ty = (int)(r % ts);
    r /= ts;
    const int c = (int)(r % C);
    r /= C;
    const int t = (int)(r % T_);
    const int f = (int)(r / T_);
    const int y = yo[t / nx] + ty;
    const int x = xo[t % nx] + xc * V;
    const bool row_in = y >= 0 && y < H;
    const T* src = frames + (((size_t)f * C + c) * H + (row_in ? y : 0)) * (size_t)W;  // (never dereferenced when the row is outside)
    if constexpr (V == 1) {
      out[k] = (row_in && x >= 0 && x < W) ? src[x] : (T)0;
    } else {
      Chunk16<T> v;
      if (row_in && x >= 0 && x + V <= W) {
        const uintptr_t a = (uintptr_t)(src + x);
        if ((a & 15) == 0) {
          v = *reinterpret_cast<const Chunk16<T>*>(src + x);
        } else if ((a & 3) == 0) {
          const uint32_t* s4 = reinterpret_cast<const uint32_t*>(src + x);
          uint32_t* d4 = reinterpret_cast<uint32_t*>(v.v);
#pragma unroll
          for (int j = 0; j < 4; ++j) d4[j] = s4[j];
        } else {
#pragma unroll
          for (int j = 0; j < V; ++j) v.v[j] = src[x + j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) v.v[j] = (row_in && x + j >= 0 && x + j < W) ? src[x + j] : (T)0;
      }
      *reinterpret_cast<Chunk16<T>*>(out + k * V) = v;
    }
  }
}

template <typename T>
static int run_extract(const T* frames, T* out, const int32_t* yo, const int32_t* xo, int F, int C, int H, int W, int ny, int nx, int ts, hipStream_t s) {
  constexpr int VEC = 16 / (int)sizeof(T);
  const bool vec = ts % VEC == 0 && ((uintptr_t)out & 15) == 0;
  const size_t chunks = (size_t)F * ny * nx * C * ts * (vec ? ts / VEC : ts);
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const unsigned grid = (unsigned)std::min<size_t>((chunks + 255) / 256, (size_t)cus * 8);  // 8 workgroups of 4 waves per CU, grid-stride beyond
  if (vec)
    hipLaunchKernelGGL((tile_extract_kernel<T, VEC>), dim3(grid), dim3(256), 0, s, frames, out, yo, xo, F, C, H, W, ny, nx, ts);
  else
    hipLaunchKernelGGL((tile_extract_kernel<T, 1>), dim3(grid), dim3(256), 0, s, frames, out, yo, xo, F, C, H, W, ny, nx, ts);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---- merge --------------------------------------------------------------------------------------------------------

template <int V>
__device__ __forceinline__ void load_row(const float* __restrict__ p, float (&v)[V]) {
  if constexpr (V == 4) {
    if (((uintptr_t)p & 15) == 0) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < V; ++j) v[j] = p[j];
}

// V consecutive pixels (y, x .. x + V - 1) of frame f that the SAME tiles cover: tile rows [iy0, iy1], tile columns [ix0, ix1]
// (each index re-tested: the origin lists need not be sorted).
template <int V>
__device__ __forceinline__ void merge_pixels(const float* __restrict__ tiles, const float* __restrict__ win, const int32_t* __restrict__ yo,
                                             const int32_t* __restrict__ xo, int f, int N, int th, int tw, int ny, int nx, int h, int w, int y, int x,
                                             int iy0, int iy1, int ix0, int ix1, float* __restrict__ out) {
  const size_t plane = (size_t)th * tw;
  float cnt[V];
#pragma unroll
  for (int j = 0; j < V; ++j) cnt[j] = 0.0f;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const int dy = y - yo[iy];
    if (dy < 0 || dy >= th) continue;
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int dx = x - xo[ix];
      if (dx < 0 || dx + V > tw) continue;
      float wv[V];
      load_row<V>(win + (size_t)dy * tw + dx, wv);
#pragma unroll
      for (int j = 0; j < V; ++j) cnt[j] = cnt[j] + wv[j];
    }
  }
  const size_t T_ = (size_t)ny * nx;
  for (int n = 0; n < N; ++n) {
    float acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0f;
    for (int iy = iy0; iy <= iy1; ++iy) {
      const int dy = y - yo[iy];
      if (dy < 0 || dy >= th) continue;
      for (int ix = ix0; ix <= ix1; ++ix) {
        const int dx = x - xo[ix];
        if (dx < 0 || dx + V > tw) continue;
        const size_t off = (size_t)dy * tw + dx;
        float wv[V], tv[V];
        load_row<V>(win + off, wv);
        load_row<V>(tiles + (((size_t)f * T_ + (size_t)iy * nx + ix) * N + n) * plane + off, tv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float p = tv[j] * wv[j];  // (its own rounding: see the pragma above)
          acc[j] = acc[j] + p;
        }
      }
    }
    float* o = out + (((size_t)f * N + n) * h + y) * (size_t)w + x;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(acc[0] / cnt[0], acc[1] / cnt[1], acc[2] / cnt[2], acc[3] / cnt[3]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = acc[j] / cnt[j];
    }
  }
}

// V = 4: w % 4 == 0, tw >= 4, 16-byte-aligned output (so no tile can cover only the inner pixels of a group); V = 1 otherwise.
template <int V>
__global__ __launch_bounds__(256) void tile_merge_kernel(const float* __restrict__ tiles, const float* __restrict__ win, const int32_t* __restrict__ yo,
                                                         const int32_t* __restrict__ xo, int F, int N, int th, int tw, int ny, int nx, int h, int w,
                                                         float* __restrict__ out) {
  const int wv = w / V;
  const size_t groups = (size_t)F * h * wv;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    const int x = (int)(g % wv) * V;
    const size_t r = g / wv;
    const int y = (int)(r % h);
    const int f = (int)(r / h);
    int iy0 = ny, iy1 = -1;
    for (int i = 0; i < ny; ++i) {
      const int d = y - yo[i];
      if (d >= 0 && d < th) {
        iy0 = min(iy0, i);
        iy1 = i;
      }
    }
    int ix0 = nx, ix1 = -1;
    bool same = true;  // every tile covers all V pixels of the group or none of them
    for (int i = 0; i < nx; ++i) {
      const int d = x - xo[i];
      const bool first = d >= 0 && d < tw, last = d + V - 1 >= 0 && d + V - 1 < tw;
      if (first || last) {
        ix0 = min(ix0, i);
        ix1 = i;
      }
      same = same && (first == last);
    }
    if (V == 1 || same) {
      merge_pixels<V>(tiles, win, yo, xo, f, N, th, tw, ny, nx, h, w, y, x, iy0, iy1, ix0, ix1, out);
    } else {
      for (int j = 0; j < V; ++j) merge_pixels<1>(tiles, win, yo, xo, f, N, th, tw, ny, nx, h, w, y, x + j, iy0, iy1, ix0, ix1, out);
    }
  }
}

}  // namespace ph

extern "C" int ph_tile_extract(const void* frames_dev, int32_t dtype, int32_t F, int32_t C, int32_t H, int32_t W, const int32_t* y_origins_dev, int32_t ny,
                               const int32_t* x_origins_dev, int32_t nx, int32_t tile_size, void* tiles_dev, void* stream) {
  using namespace ph;
  PH_REQUIRE(frames_dev && tiles_dev && y_origins_dev && x_origins_dev, "ph_tile_extract: null pointer");
  PH_REQUIRE(dtype == 0 || dtype == 1, "ph_tile_extract: dtype must be 0 (uint8) or 1 (float32), got %d", dtype);
  PH_REQUIRE(F > 0 && C > 0 && H > 0 && W > 0, "ph_tile_extract: bad frame shape F=%d C=%d H=%d W=%d", F, C, H, W);
  PH_REQUIRE(ny > 0 && nx > 0 && tile_size > 0, "ph_tile_extract: bad grid ny=%d nx=%d tile_size=%d", ny, nx, tile_size);
  PH_REQUIRE((int64_t)ny * nx <= 0x7fffffffLL / F, "ph_tile_extract: too many tiles (%d x %d x %d)", F, ny, nx);
  PH_REQUIRE(frames_dev != tiles_dev, "ph_tile_extract: frames and tiles are the same buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (dtype == 0)
    return run_extract(static_cast<const uint8_t*>(frames_dev), static_cast<uint8_t*>(tiles_dev), y_origins_dev, x_origins_dev, F, C, H, W, ny, nx, tile_size, s);
  return run_extract(static_cast<const float*>(frames_dev), static_cast<float*>(tiles_dev), y_origins_dev, x_origins_dev, F, C, H, W, ny, nx, tile_size, s);
}

extern "C" int ph_tile_merge(const float* tile_maps_dev, const float* window_dev, int32_t F, int32_t N, int32_t th, int32_t tw, const int32_t* y_origins_dev,
                             int32_t ny, const int32_t* x_origins_dev, int32_t nx, int32_t h, int32_t w, float* out_dev, void* stream) {
  using namespace ph;
  PH_REQUIRE(tile_maps_dev && window_dev && y_origins_dev && x_origins_dev && out_dev, "ph_tile_merge: null pointer");
  PH_REQUIRE(F > 0 && N > 0 && th > 0 && tw > 0, "ph_tile_merge: bad tile-map shape F=%d N=%d th=%d tw=%d", F, N, th, tw);
  PH_REQUIRE(ny > 0 && nx > 0 && h > 0 && w > 0, "ph_tile_merge: bad grid / output ny=%d nx=%d h=%d w=%d", ny, nx, h, w);
  PH_REQUIRE((int64_t)ny * nx <= 0x7fffffffLL / F, "ph_tile_merge: too many tiles (%d x %d x %d)", F, ny, nx);
  PH_REQUIRE(tile_maps_dev != out_dev, "ph_tile_merge: tile maps and output are the same buffer");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = w % 4 == 0 && tw >= 4 && ((uintptr_t)out_dev & 15) == 0;
  const size_t groups = (size_t)F * h * (vec ? w / 4 : w);
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const unsigned grid = (unsigned)std::min<size_t>((groups + 255) / 256, (size_t)cus * 8);  // 8 workgroups of 4 waves per CU, grid-stride beyond
  if (vec)
    hipLaunchKernelGGL((tile_merge_kernel<4>), dim3(grid), dim3(256), 0, s, tile_maps_dev, window_dev, y_origins_dev, x_origins_dev, F, N, th, tw, ny, nx, h, w, out_dev);
  else
    hipLaunchKernelGGL((tile_merge_kernel<1>), dim3(grid), dim3(256), 0, s, tile_maps_dev, window_dev, y_origins_dev, x_origins_dev, F, N, th, tw, ny, nx, h, w, out_dev);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---- merge, several heads in one launch ---------------------------------------------------------------------------

namespace ph {

constexpr int kMergeMaxHeads = 4;
constexpr int kMergeMaxChannels = 8;

// Kernel argument, by value: one entry per CHANNEL of the concatenated heads (the host flattens head k, channel n to slot j).
// src[j] = arena_k + n * th * tw with tile stride cs[j] * th * tw; dst[j] = out_k + n * h * w with frame stride cs[j] * h * w; cs[j] = c_k.
struct MergeHeadsArgs {
  const float* src[kMergeMaxChannels];
  float* dst[kMergeMaxChannels];
  int32_t cs[kMergeMaxChannels];
};

// As merge_pixels, but the window row segment of a covering tile is loaded once and feeds cnt and all CT accumulators (registers:
// CT * V + V floats).  Per channel the sequence of roundings is merge_pixels' own: acc = acc + tile * w, cnt = cnt + w, acc / cnt.
template <int CT, int V>
__device__ __forceinline__ void merge_heads_pixels(const MergeHeadsArgs& a, const float* __restrict__ win, const int32_t* __restrict__ yo,
                                                   const int32_t* __restrict__ xo, int f, int th, int tw, int ny, int nx, int h, int w, int y, int x,
                                                   int iy0, int iy1, int ix0, int ix1) {
  const size_t plane = (size_t)th * tw;
  const size_t T_ = (size_t)ny * nx;
  float cnt[V], acc[CT][V];
#pragma unroll
  for (int j = 0; j < V; ++j) cnt[j] = 0.0f;
#pragma unroll
  for (int c = 0; c < CT; ++c)
#pragma unroll
    for (int j = 0; j < V; ++j) acc[c][j] = 0.0f;
  for (int iy = iy0; iy <= iy1; ++iy) {
    const int dy = y - yo[iy];
    if (dy < 0 || dy >= th) continue;
    for (int ix = ix0; ix <= ix1; ++ix) {
      const int dx = x - xo[ix];
      if (dx < 0 || dx + V > tw) continue;
      const size_t off = (size_t)dy * tw + dx;
      const size_t t = (size_t)f * T_ + (size_t)iy * nx + ix;
      float wv[V];
      load_row<V>(win + off, wv);
#pragma unroll
      for (int j = 0; j < V; ++j) cnt[j] = cnt[j] + wv[j];
#pragma unroll
      for (int c = 0; c < CT; ++c) {
        float tv[V];
        load_row<V>(a.src[c] + t * (size_t)a.cs[c] * plane + off, tv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const float p = tv[j] * wv[j];  // (its own rounding: see the pragma above)
          acc[c][j] = acc[c][j] + p;
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    float* o = a.dst[c] + ((size_t)f * a.cs[c] * h + y) * (size_t)w + x;
    if constexpr (V == 4) {
      *reinterpret_cast<float4*>(o) = make_float4(acc[c][0] / cnt[0], acc[c][1] / cnt[1], acc[c][2] / cnt[2], acc[c][3] / cnt[3]);
    } else {
#pragma unroll
      for (int j = 0; j < V; ++j) o[j] = acc[c][j] / cnt[j];
    }
  }
}

// Thread mapping and coverage search of tile_merge_kernel.  V = 4: w % 4 == 0, tw >= 4 and every output 16-byte aligned.
template <int CT, int V>
__global__ __launch_bounds__(256) void tile_merge_heads_kernel(const MergeHeadsArgs a, const float* __restrict__ win, const int32_t* __restrict__ yo,
                                                               const int32_t* __restrict__ xo, int F, int th, int tw, int ny, int nx, int h, int w) {
  const int wv = w / V;
  const size_t groups = (size_t)F * h * wv;
  for (size_t g = (size_t)blockIdx.x * 256 + threadIdx.x; g < groups; g += (size_t)gridDim.x * 256) {
    const int x = (int)(g % wv) * V;
    const size_t r = g / wv;
    const int y = (int)(r % h);
    const int f = (int)(r / h);
    int iy0 = ny, iy1 = -1;
    for (int i = 0; i < ny; ++i) {
      const int d = y - yo[i];
      if (d >= 0 && d < th) {
        iy0 = min(iy0, i);
        iy1 = i;
      }
    }
    int ix0 = nx, ix1 = -1;
    bool same = true;  // every tile covers all V pixels of the group or none of them
    for (int i = 0; i < nx; ++i) {
      const int d = x - xo[i];
      const bool first = d >= 0 && d < tw, last = d + V - 1 >= 0 && d + V - 1 < tw;
      if (first || last) {
        ix0 = min(ix0, i);
        ix1 = i;
      }
      same = same && (first == last);
    }
    if (V == 1 || same) {
      merge_heads_pixels<CT, V>(a, win, yo, xo, f, th, tw, ny, nx, h, w, y, x, iy0, iy1, ix0, ix1);
    } else {
      for (int j = 0; j < V; ++j) merge_heads_pixels<CT, 1>(a, win, yo, xo, f, th, tw, ny, nx, h, w, y, x + j, iy0, iy1, ix0, ix1);
    }
  }
}

template <int CT>
static void launch_merge_heads(bool vec, unsigned grid, hipStream_t s, const MergeHeadsArgs& a, const float* win, const int32_t* yo, const int32_t* xo, int F,
                               int th, int tw, int ny, int nx, int h, int w) {
  if (vec)
    hipLaunchKernelGGL((tile_merge_heads_kernel<CT, 4>), dim3(grid), dim3(256), 0, s, a, win, yo, xo, F, th, tw, ny, nx, h, w);
  else
    hipLaunchKernelGGL((tile_merge_heads_kernel<CT, 1>), dim3(grid), dim3(256), 0, s, a, win, yo, xo, F, th, tw, ny, nx, h, w);
}

}  // namespace ph

extern "C" int ph_tile_merge_heads(const float* const* arenas_dev, const int32_t* channels, int32_t K, const float* window_dev, int32_t F, int32_t th, int32_t tw,
                                   const int32_t* y_origins_dev, int32_t ny, const int32_t* x_origins_dev, int32_t nx, int32_t h, int32_t w, float* const* outs_dev,
                                   void* stream) {
  using namespace ph;
  PH_REQUIRE(arenas_dev && channels && window_dev && y_origins_dev && x_origins_dev && outs_dev, "ph_tile_merge_heads: null pointer");
  PH_REQUIRE(K >= 1 && K <= kMergeMaxHeads, "ph_tile_merge_heads: K must be 1..%d, got %d", kMergeMaxHeads, K);
  int total = 0;
  for (int k = 0; k < K; ++k) {
    PH_REQUIRE(arenas_dev[k] && outs_dev[k], "ph_tile_merge_heads: null pointer (head %d)", k);
    PH_REQUIRE(channels[k] >= 1 && channels[k] <= kMergeMaxChannels, "ph_tile_merge_heads: head %d has %d channels (1..%d)", k, channels[k], kMergeMaxChannels);
    total += channels[k];
  }
  PH_REQUIRE(total <= kMergeMaxChannels, "ph_tile_merge_heads: %d channels in total (at most %d)", total, kMergeMaxChannels);
  PH_REQUIRE(F > 0 && th > 0 && tw > 0, "ph_tile_merge_heads: bad tile-map shape F=%d th=%d tw=%d", F, th, tw);
  PH_REQUIRE(ny > 0 && nx > 0 && h > 0 && w > 0, "ph_tile_merge_heads: bad grid / output ny=%d nx=%d h=%d w=%d", ny, nx, h, w);
  PH_REQUIRE((int64_t)ny * nx <= 0x7fffffffLL / F, "ph_tile_merge_heads: too many tiles (%d x %d x %d)", F, ny, nx);
  // byte ranges: no output may overlap an arena or another output
  const uint64_t tiles = (uint64_t)F * ny * nx, plane = (uint64_t)th * tw * sizeof(float), frame = (uint64_t)h * w * sizeof(float);
  auto overlap = [](uintptr_t a, uint64_t na, uintptr_t b, uint64_t nb) { return a < b + nb && b < a + na; };
  for (int k = 0; k < K; ++k) {
    const uintptr_t o = (uintptr_t)outs_dev[k];
    const uint64_t no = (uint64_t)F * channels[k] * frame;
    for (int j = 0; j < K; ++j) {
      PH_REQUIRE(!overlap(o, no, (uintptr_t)arenas_dev[j], tiles * channels[j] * plane), "ph_tile_merge_heads: output %d aliases arena %d", k, j);
      PH_REQUIRE(j == k || !overlap(o, no, (uintptr_t)outs_dev[j], (uint64_t)F * channels[j] * frame), "ph_tile_merge_heads: output %d aliases output %d", k, j);
    }
  }
  MergeHeadsArgs a{};
  bool vec = w % 4 == 0 && tw >= 4;
  int c = 0;
  for (int k = 0; k < K; ++k) {
    vec = vec && ((uintptr_t)outs_dev[k] & 15) == 0;
    for (int n = 0; n < channels[k]; ++n, ++c) {
      a.src[c] = arenas_dev[k] + (size_t)n * th * tw;
      a.dst[c] = outs_dev[k] + (size_t)n * h * w;
      a.cs[c] = channels[k];
    }
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t groups = (size_t)F * h * (vec ? w / 4 : w);
  int cus = 0;
  if (int rc = device_cu_count(&cus); rc != PH_OK) return rc;
  const unsigned grid = (unsigned)std::min<size_t>((groups + 255) / 256, (size_t)cus * 8);  // 8 workgroups of 4 waves per CU, grid-stride beyond
  switch (total) {
    case 1: launch_merge_heads<1>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    case 2: launch_merge_heads<2>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    case 3: launch_merge_heads<3>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    case 4: launch_merge_heads<4>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    case 5: launch_merge_heads<5>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    case 6: launch_merge_heads<6>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    case 7: launch_merge_heads<7>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
    default: launch_merge_heads<8>(vec, grid, s, a, window_dev, y_origins_dev, x_origins_dev, F, th, tw, ny, nx, h, w); break;
  }
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
