// Swin Transformer V2 encoder kernels for gfx950 (MI355X, CDNA4): what HuggingFace's Swinv2Backbone needs beyond the ops the other encoders already have (the reference
// wraps it in PretrainedBackbone, sleap_nn/architectures/pretrained.py).  Exact fp32, inference only.
//
//   window_attn_v2_wide_kernel .. cosine window attention for windows of 9..24 tokens a side (up to 576 tokens): one workgroup per (window, head), the keys tiled, online
//                            softmax.  Windows up to 8 run the cosine variant of window_attn_kernel (swin_kernels.hip: launch_window_attn_v2), where the operation --
//                            q and k normalised per token and head, the head's logit scale, a bias table the host computed (16 sigmoid(MLP(coords))), the band-mask
//                            constant as HuggingFace applies it -- is described.
//   layernorm_add_kernel ... dst = res + LayerNorm(src): Swinv2 norms AFTER each branch (layernorm_before / layernorm_after) and adds the shortcut to the normed branch.
//
// The patch-merge gather without a norm is patch_merge_gather_kernel (swin_train_kernels.hip); the Linear layers are the ordinary row GEMMs.
#include <algorithm>

#include "common.h"
#include "device_math.h"
#include "net_kernels.h"

namespace ph {

// ---------------------------------------------------------------------------------------
// Windows of 9..24 tokens a side (81..576 tokens): the same operation with the keys tiled.  One workgroup = one (window, head); its four waves take the 32-query tiles
// wave, wave + 4, ..  A query tile keeps the lane layout of window_attn_kernel (query in the lane, the 32 keys of the current tile in the accumulator registers of S^T = K Q^T, those
// registers unchanged as the B operand of O^T += V^T P^T) and walks the key tiles with an online softmax: a running maximum m and a running sum per query, both per lane
// (m agrees between the two lane halves after one exchange; the sum's halves are added once, at the end).  Each tile multiplies the 16 O^T accumulators and the sum by
// exp(m_old - m_new): the factor is uniform per lane (the query is the lane's column) and exactly 1 where the maximum did not move, so there is no branch on the data.
//   * m starts from the first tile's real scores (tile 0 never rescales); every tile holds at least one live key, so no expression forms (-inf) - (-inf).
//   * dead key columns exist only in the last tile (N mod 32 != 0): they take no part in the maximum and their p is 0.
//   * shift: the layer's own (a.sh = a.sw), whatever the map: HuggingFace rolls and masks a shifted layer even where one window covers the padded axis.
//   * LDS, filled once per workgroup: the head's bias table ((2w - 1)^2 floats), the tokens' pixel and code (window_attn.h, 5 bits per coordinate) and each key's
//     1 / max(||k||, 1e-12), so that a key tile is not normalised again by every query tile.  Entries N .. 32 T - 1 mirror token 0: every address stays in range.
//   * K and V tiles come from L2 once per query tile; the next tile's loads are issued before the current tile's arithmetic.
// No atomics; one barrier, which every wave reaches (a wave without a query tile only skips the loop behind it).
// ---------------------------------------------------------------------------------------
constexpr int WIDE_MAX_W = 24, WIDE_MAX_N = WIDE_MAX_W * WIDE_MAX_W, WIDE_MAX_REL = (2 * WIDE_MAX_W - 1) * (2 * WIDE_MAX_W - 1);

typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void window_attn_v2_wide_kernel(WindowAttnArgs a) {
  __shared__ float tbl[WIDE_MAX_REL];
  __shared__ __attribute__((aligned(16))) int tok_pix[WIDE_MAX_N];
  __shared__ __attribute__((aligned(16))) int tok_code[WIDE_MAX_N];
  __shared__ float k_inv[WIDE_MAX_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const WindowGrid grid = window_grid(a.B, a.H, a.W, a.w);
  const int w = grid.w, N = grid.N, rel = grid.rel, T = (N + 31) >> 5;
  const WindowItem it = window_decode<unsigned>(grid, blockIdx.x, a.heads);
  const int head = it.head;
  const int C3 = 3 * a.C;
  const float* qkv = static_cast<const float*>(a.qkv);
  for (int i = threadIdx.x; i < rel; i += 256) tbl[i] = a.table[(size_t)head * rel + i];
  for (int i = threadIdx.x; i < T * 32; i += 256) {
    const TokenInfo tk = window_token<5>(grid, it, i < N ? i : 0, a.sh, a.sw);
    const int pix = tk.pix;
    tok_pix[i] = pix;
    tok_code[i] = tk.code;
    const float* kb = (pix >= 0 ? qkv + (size_t)pix * C3 : a.qkv_bias) + a.C + head * 32;
    float ss = 0.f;
#pragma unroll
    for (int v4 = 0; v4 < 8; ++v4) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kb + v4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) ss = fmaf(kv[e], kv[e], ss);
    }
    k_inv[i] = 1.0f / fmaxf(sqrtf(ss), 1e-12f);
  }
  __syncthreads();
  const float hscale = a.scale[head];
  const int hoff = head * 32;
  // key tile tj as it leaves memory: K of token 32 tj + (l & 31), channels 16 half .. + 15; V of key j(tj, r, half), channel l & 31
  auto load_tile = [&](int tj, float (&kr)[16], float (&vr)[16]) {
    const int pk = tok_pix[tj * 32 + l31];
    const float* kb = (pk >= 0 ? qkv + (size_t)pk * C3 : a.qkv_bias) + a.C + hoff + half * 16;
#pragma unroll
    for (int v4 = 0; v4 < 4; ++v4) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kb + v4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) kr[v4 * 4 + e] = kv[e];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const i32x4 p4 = *reinterpret_cast<const i32x4*>(&tok_pix[window_key(tj, 4 * g, half)]);
#pragma unroll
      for (int e = 0; e < 4; ++e) vr[g * 4 + e] = (p4[e] >= 0 ? qkv + (size_t)p4[e] * C3 : a.qkv_bias)[2 * a.C + hoff + l31];
    }
  };
  for (int ti = wave; ti < T; ti += 4) {
    const int tq = ti * 32 + l31;
    const int pixq = tok_pix[tq];
    const int ci = tok_code[tq];
    const int bi = token_band<5>(ci);
    const int qrow = window_bias_row<5>(ci, w);
    float q[16];
    {
      const float* qb = (pixq >= 0 ? qkv + (size_t)pixq * C3 : a.qkv_bias) + hoff + half * 16;
      float qss = 0.f;
#pragma unroll
      for (int v4 = 0; v4 < 4; ++v4) {
        const f32x4 qv = *reinterpret_cast<const f32x4*>(qb + v4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          q[v4 * 4 + e] = qv[e];
          qss = fmaf(qv[e], qv[e], qss);
        }
      }
      qss += __shfl_xor(qss, 32, 64);
      const float qn = hscale / fmaxf(sqrtf(qss), 1e-12f);
#pragma unroll
      for (int e = 0; e < 16; ++e) q[e] *= qn;
    }
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    float m = 0.f, sum = 0.f;
    float kn[16], vn[16];
    load_tile(0, kn, vn);
    for (int tj = 0; tj < T; ++tj) {
      const int tk = tj * 32 + l31;
      const float kscale = tk < N ? k_inv[tk] : 0.f;
      float k[16], v[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        k[e] = kn[e] * kscale;
        v[e] = window_key(tj, e, half) < N ? vn[e] : 0.f;
      }
      if (tj + 1 < T) load_tile(tj + 1, kn, vn);
      f32x16 s;
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) s = __builtin_amdgcn_mfma_f32_32x32x2f32(k[kk], q[kk], s, 0, 0, 0);
      float tmx = -INFINITY;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const i32x4 c4 = *reinterpret_cast<const i32x4*>(&tok_code[window_key(tj, 4 * g, half)]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = g * 4 + e;
          const int cj = c4[e];
          float val = s[r] + tbl[qrow - window_bias_col<5>(cj, w)];
          if (bi != token_band<5>(cj)) val += -200.0f;
          s[r] = val;
          if (window_key(tj, r, half) < N) tmx = fmaxf(tmx, val);  // dead key columns take no part in the softmax
        }
      }
      tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));  // finite: every tile has a live key
      const float m_new = tj == 0 ? tmx : fmaxf(m, tmx);
      const float f = tj == 0 ? 1.0f : exp_comp(m - m_new);
      m = m_new;
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = window_key(tj, r, half) < N ? exp_comp(s[r] - m_new) : 0.f;
        s[r] = p;
        ps += p;
      }
      sum = fmaf(sum, f, ps);
#pragma unroll
      for (int e = 0; e < 16; ++e) o[e] *= f;
      // O^T[c][i] += sum_j V[j][c] P[i][j]
#pragma unroll
      for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(v[r], s[r], o, 0, 0, 0);
    }
    sum += __shfl_xor(sum, 32, 64);
    // query tq: channels 8 g + 4 half + (0..3) of the head, at the token's own pixel
    if (tq < N && pixq >= 0) {
      const float inv_sum = 1.0f / sum;
      float* out = static_cast<float*>(a.dst) + (size_t)pixq * a.C + hoff + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 r4;
#pragma unroll
        for (int e = 0; e < 4; ++e) r4[e] = o[g * 4 + e] * inv_sum;
        *reinterpret_cast<f32x4*>(out + 8 * g) = r4;
      }
    }
  }
}

int launch_window_attn_v2_wide(const WindowAttnArgs& a, hipStream_t s) {
  WindowGrid g;
  unsigned blocks;
  const int rc = window_attn_check("key-tiled cosine window attention", WIDE_MAX_W, a.qkv && a.table && a.qkv_bias && a.scale && a.dst, a, &g, 1, &blocks);
  if (rc != PH_OK) return rc;
  hipLaunchKernelGGL(window_attn_v2_wide_kernel, dim3(blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// dst = res + LayerNorm(src) over the channel axis of NHWC tensors: layernorm_kernel (convnext_kernels.hip: 16 lanes per pixel, two-pass mean / biased variance, pad
// channels excluded and written as zeros) with the shortcut added to the normed value.  res and dst are distinct tensors.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void layernorm_add_kernel(const float* __restrict__ src, const float* __restrict__ res, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, float* __restrict__ dst, int c, int cp, size_t npix, float eps) {
  const int sub = threadIdx.x & 15;
  const int quads = cp >> 2;
  const float inv_c = 1.0f / (float)c;
  const size_t stride = (size_t)gridDim.x * 16;
  const size_t rounds = (npix + stride - 1) / stride;
  size_t pix = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  for (size_t it = 0; it < rounds; ++it, pix += stride) {
    const bool live = pix < npix;
    const float* p = src + (live ? pix : npix - 1) * cp;
    float s = 0.f;
    for (int q = sub; q < quads; q += 16) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + q * 4);
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    s += __shfl_xor(s, 8, 16);
    s += __shfl_xor(s, 4, 16);
    s += __shfl_xor(s, 2, 16);
    s += __shfl_xor(s, 1, 16);
    const float mean = s * inv_c;
    float ss = 0.f;
    for (int q = sub; q < quads; q += 16) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(p + q * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[e] - mean;
        ss += (q * 4 + e < c) ? d * d : 0.f;
      }
    }
    ss += __shfl_xor(ss, 8, 16);
    ss += __shfl_xor(ss, 4, 16);
    ss += __shfl_xor(ss, 2, 16);
    ss += __shfl_xor(ss, 1, 16);
    const float rstd = 1.0f / sqrtf(ss * inv_c + eps);
    if (live) {
      float* o = dst + pix * cp;
      const float* rp = res + pix * cp;
      for (int q = sub; q < quads; q += 16) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(p + q * 4);
        const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + q * 4);
        const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + q * 4);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(rp + q * 4);
        f32x4 r;
#pragma unroll
        for (int e = 0; e < 4; ++e) r[e] = sc[e] + ((v[e] - mean) * rstd * g[e] + bt[e]);
        *reinterpret_cast<f32x4*>(o + q * 4) = r;
      }
    }
  }
}

int launch_layernorm_add(const float* src, const float* res, const float* gamma, const float* beta, float* dst, int c, int cp, size_t npix, hipStream_t s, float eps) {
  PH_REQUIRE(src && res && gamma && beta && dst && res != dst && src != dst && c > 0 && cp >= c && (cp & 3) == 0 && npix > 0, "residual LayerNorm: bad arguments");
  const int blocks = (int)std::min<size_t>((npix + 15) / 16, 256 * 32);
  hipLaunchKernelGGL(layernorm_add_kernel, dim3(blocks), dim3(256), 0, s, src, res, gamma, beta, dst, c, cp, npix, eps);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph

using namespace ph;

// Test support (tests/test_gpu_window_attn_v2.py), not a product path: one launch of the cosine window attention on tensors the caller owns, through launch_window_attn_v2
// and its checks, synchronised before it returns.
extern "C" int ph_debug_window_attn_v2_run(const float* qkv, const float* qkv_bias, const float* scale, const float* table, float* dst, int32_t B, int32_t H, int32_t W,
                                           int32_t heads, int32_t w, int32_t shift) {
  PH_REQUIRE(qkv && qkv_bias && scale && table && dst && heads > 0, "ph_debug_window_attn_v2_run: bad arguments");
  WindowAttnArgs a{};
  a.qkv = qkv;
  a.qkv_bias = qkv_bias;
  a.scale = scale;
  a.table = table;
  a.dst = dst;
  a.B = B;
  a.H = H;
  a.W = W;
  a.C = heads * 32;
  a.heads = heads;
  a.w = w;
  a.sh = a.sw = shift;
  const int rc = launch_window_attn_v2(a, nullptr);
  PH_HIP_CHECK(hipDeviceSynchronize());
  return rc;
}

// Test support (tests/test_gpu_window_attn_v2_wide.py), not a product path: one launch of the key-tiled kernel on tensors the caller owns, through
// launch_window_attn_v2_wide and its checks (windows 2..24: the product path sends it 9..24 only), synchronised before it returns.
extern "C" int ph_debug_window_attn_v2_wide_run(const float* qkv, const float* qkv_bias, const float* scale, const float* table, float* dst, int32_t B, int32_t H, int32_t W,
                                                int32_t heads, int32_t w, int32_t shift) {
  PH_REQUIRE(heads > 0, "ph_debug_window_attn_v2_wide_run: heads must be positive");  // (the pointers are the launcher's check: "null pointer")
  WindowAttnArgs a{};
  a.qkv = qkv;
  a.qkv_bias = qkv_bias;
  a.scale = scale;
  a.table = table;
  a.dst = dst;
  a.B = B;
  a.H = H;
  a.W = W;
  a.C = heads * 32;
  a.heads = heads;
  a.w = w;
  a.sh = a.sw = shift;
  const int rc = launch_window_attn_v2_wide(a, nullptr);
  PH_HIP_CHECK(hipDeviceSynchronize());
  return rc;
}
