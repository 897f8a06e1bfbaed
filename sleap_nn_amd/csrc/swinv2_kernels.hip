// Swin Transformer V2 encoder kernels for gfx950 (MI355X, CDNA4): what HuggingFace's Swinv2Backbone needs beyond the ops the other encoders already have (the reference
// wraps it in PretrainedBackbone, sleap_nn/architectures/pretrained.py).  Exact fp32, inference only.
//
//   window_attn_v2_kernel .. cosine window attention: the plan of window_attn_kernel (swin_kernels.hip; pad, roll, partition, mask, reverse and crop as index arithmetic of
//                            one launch) with q and k normalised per token and head, the head's logit scale, a bias table the host computed (16 sigmoid(MLP(coords)))
//                            and the band-mask constant of the shifted block as HuggingFace applies it.
//   window_attn_v2_wide_kernel .. the same operation for windows of 9..24 tokens a side (up to 576 tokens): one workgroup per (window, head), the keys tiled, online softmax.
//   layernorm_add_kernel ... dst = res + LayerNorm(src): Swinv2 norms AFTER each branch (layernorm_before / layernorm_after) and adds the shortcut to the normed branch.
//
// The patch-merge gather without a norm is patch_merge_gather_kernel (swin_train_kernels.hip); the Linear layers are the ordinary row GEMMs.
#include <algorithm>

#include "common.h"
#include "device_math.h"
#include "net_kernels.h"

namespace ph {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// exp(x) for x <= 0 through the hardware exp2, with the rounding of x log2(e) compensated: scores here reach +-100 before the bias, so x goes far enough from 0 for the
// plain product's rounding (|x| 2^-24 relative in the result) to show
__device__ __forceinline__ float exp_comp(float x) {
  const float l2e = 1.4426950408889634f, l2e_lo = 1.92596299e-8f;  // log2(e) = l2e + l2e_lo
  const float t = x * l2e;
  const float lo = fmaf(x, l2e, -t) + x * l2e_lo;
  return __builtin_amdgcn_exp2f(t) * fmaf(lo, 0.6931471805599453f, 1.0f);
}

// ---------------------------------------------------------------------------------------
// One wave = one (window, head); four waves (consecutive heads, then the next window) per workgroup.  N = w^2 <= 64 tokens, head dimension 32, T = ceil(N / 32)
// 32-token tiles; registers, lanes and accumulator order exactly as window_attn_kernel:
//   S^T = K Q^T on v_mfma_f32_32x32x2_f32 (A = K, B = Q; the two lane halves hold channels 0..15 / 16..31 of their token), query i in the lane (column l & 31), keys
//   j = 8 (r >> 2) + 4 (l >> 5) + (r & 3) in its accumulator registers; O^T = V^T P^T takes those registers as its B operand unchanged.
// What Swinv2 changes:
//   * q and k are divided by max(||.||_2, 1e-12) over the head's 32 channels (F.normalize): a lane holds 16 of them, the sum of squares takes one exchange with lane
//     l ^ 32.  The head's scale exp(min(logit_scale, log 100)) (a.scale, computed by the host) is folded into q behind the normalisation.
//   * a padded token has hidden state 0: q = query.bias, k = 0 exactly (key has no bias: the key section of a.qkv_bias is zero, its normalised k is 0 / 1e-12 = 0), v = value.bias.
//     It is a key like any other and is never stored.
//   * the band mask adds -200 where the bands differ: Swinv2SelfAttention.forward adds the (-100) mask TWICE.  With |q.k| scale <= 100 and a bias in (0, 16) a masked score
//     can stay above an unmasked one: the constant is part of the arithmetic, not a stand-in for minus infinity.
//   * shift: the layer's own (a.shift, both axes), whatever the map: HuggingFace rolls and masks a shifted layer even where one window covers the padded axis.
// ---------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void window_attn_v2_kernel(WindowAttnV2Args a) {
  __shared__ float tbl[4][232];
  __shared__ int tok_pix[4][64];
  __shared__ int tok_code[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int w = a.w, N = w * w;
  const int pH = (a.H + w - 1) / w * w, pW = (a.W + w - 1) / w * w;
  const int nwh = pH / w, nww = pW / w;
  const long long total = (long long)a.B * nwh * nww * a.heads;
  long long item = (long long)blockIdx.x * 4 + wave;
  const bool live = item < total;
  if (!live) item = total - 1;
  const int head = (int)(item % a.heads);
  long long win = item / a.heads;
  const int wx = (int)(win % nww);
  win /= nww;
  const int wy = (int)(win % nwh);
  const int b = (int)(win / nwh);
  const int rel = (2 * w - 1) * (2 * w - 1);
  for (int i = lane; i < rel; i += 64) tbl[wave][i] = a.table[(size_t)head * rel + i];
  {
    const int t = lane < N ? lane : 0;  // (dead lanes mirror token 0: their table index stays in range)
    const int ty = t / w, tx = t - ty * w;
    int y = wy * w + ty + a.shift, x = wx * w + tx + a.shift;
    if (y >= pH) y -= pH;
    if (x >= pW) x -= pW;
    const int band = ((a.shift > 0 && wy == nwh - 1 && ty >= w - a.shift) ? 2 : 0) | ((a.shift > 0 && wx == nww - 1 && tx >= w - a.shift) ? 1 : 0);
    tok_pix[wave][lane] = (y < a.H && x < a.W) ? (b * a.H + y) * a.W + x : -1;
    tok_code[wave][lane] = ty | (tx << 4) | (band << 8);
  }
  __syncthreads();
  const int C3 = 3 * a.C;
  const float hscale = a.scale[head];
  // Q and K: token ti * 32 + (l & 31), channels 16 half .. 16 half + 15 of the head, each divided by its token's norm over all 32
  float q[T][16], k[T][16];
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int t = ti * 32 + l31;
    const int pix = tok_pix[wave][t];
    const float* base = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias) + head * 32 + half * 16;
    const bool on = t < N;
    float qss = 0.f, kss = 0.f;
#pragma unroll
    for (int v4 = 0; v4 < 4; ++v4) {
      f32x4 qv = {0.f, 0.f, 0.f, 0.f}, kv = {0.f, 0.f, 0.f, 0.f};
      if (on) {
        qv = *reinterpret_cast<const f32x4*>(base + v4 * 4);
        kv = *reinterpret_cast<const f32x4*>(base + a.C + v4 * 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[ti][v4 * 4 + e] = qv[e];
        k[ti][v4 * 4 + e] = kv[e];
        qss = fmaf(qv[e], qv[e], qss);
        kss = fmaf(kv[e], kv[e], kss);
      }
    }
    qss += __shfl_xor(qss, 32, 64);
    kss += __shfl_xor(kss, 32, 64);
    const float qn = hscale / fmaxf(sqrtf(qss), 1e-12f), kn = 1.0f / fmaxf(sqrtf(kss), 1e-12f);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      q[ti][e] *= qn;
      k[ti][e] *= kn;
    }
  }
  // V: key j(tj, r, half), channel l & 31 of the head
  float v[T][16];
#pragma unroll
  for (int tj = 0; tj < T; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = tj * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
      float val = 0.f;
      if (j < N) {
        const int pix = tok_pix[wave][j];
        val = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias)[2 * a.C + head * 32 + l31];
      }
      v[tj][r] = val;
    }
  // S^T tiles [tj][ti]
  f32x16 s[T][T];
#pragma unroll
  for (int tj = 0; tj < T; ++tj)
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(k[tj][kk], q[ti][kk], acc, 0, 0, 0);
      s[tj][ti] = acc;
    }
  // bias, band mask, softmax over the keys of each query (= this lane's column)
  f32x16 o[T];
  float inv_sum[T];
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int ci = tok_code[wave][ti * 32 + l31];
    const int tyi = ci & 15, txi = (ci >> 4) & 15, bi = ci >> 8;
    float mx = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = tj * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        if (j < N) {  // dead key columns take no part in the softmax
          const int cj = tok_code[wave][j];
          const int tyj = cj & 15, txj = (cj >> 4) & 15, bj = cj >> 8;
          float val = s[tj][ti][r] + tbl[wave][(tyi - tyj + w - 1) * (2 * w - 1) + (txi - txj + w - 1)];
          if (bi != bj) val += -200.0f;
          s[tj][ti][r] = val;
          mx = fmaxf(mx, val);
        }
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = tj * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
        const float p = j < N ? exp_comp(s[tj][ti][r] - mx) : 0.f;
        s[tj][ti][r] = p;
        sum += p;
      }
    sum += __shfl_xor(sum, 32, 64);
    inv_sum[ti] = 1.0f / sum;
    // O^T[c][i] = sum_j V[j][c] P[i][j]
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(v[tj][r], s[tj][ti][r], acc, 0, 0, 0);
    o[ti] = acc;
  }
  // query ti * 32 + (l & 31): channels 8 g + 4 half + (0..3) of the head, at the token's own pixel
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int t = ti * 32 + l31;
    const int pix = tok_pix[wave][t];
    if (live && t < N && pix >= 0) {
      float* out = a.dst + (size_t)pix * a.C + head * 32 + 4 * half;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        f32x4 r4;
#pragma unroll
        for (int e = 0; e < 4; ++e) r4[e] = o[ti][g * 4 + e] * inv_sum[ti];
        *reinterpret_cast<f32x4*>(out + 8 * g) = r4;
      }
    }
  }
}

int launch_window_attn_v2(const WindowAttnV2Args& a, hipStream_t s) {
  PH_REQUIRE(a.qkv && a.table && a.qkv_bias && a.scale && a.dst, "cosine window attention: null pointer");
  PH_REQUIRE(a.w >= 2 && a.w <= 8, "cosine window attention: window_size %d is outside 2..8", a.w);
  PH_REQUIRE(a.heads > 0 && a.C == a.heads * 32, "cosine window attention: head dimension must be 32 (C %d, heads %d)", a.C, a.heads);
  PH_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && (long long)a.B * a.H * a.W < (1ll << 31) / 4, "cosine window attention: bad map size");
  PH_REQUIRE(a.shift >= 0 && a.shift < a.w, "cosine window attention: shift must be smaller than the window");
  const long long nwin = (long long)a.B * ((a.H + a.w - 1) / a.w) * ((a.W + a.w - 1) / a.w);
  const long long blocks = (nwin * a.heads + 3) / 4;
  PH_REQUIRE(blocks < (1ll << 31), "cosine window attention: too many windows");
  if (a.w * a.w <= 32)
    hipLaunchKernelGGL(window_attn_v2_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(window_attn_v2_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Windows of 9..24 tokens a side (81..576 tokens): the same operation with the keys tiled.  One workgroup = one (window, head); its four waves take the 32-query tiles
// wave, wave + 4, ..  A query tile keeps the lane layout above (query in the lane, the 32 keys of the current tile in the accumulator registers of S^T = K Q^T, those
// registers unchanged as the B operand of O^T += V^T P^T) and walks the key tiles with an online softmax: a running maximum m and a running sum per query, both per lane
// (m agrees between the two lane halves after one exchange; the sum's halves are added once, at the end).  Each tile multiplies the 16 O^T accumulators and the sum by
// exp(m_old - m_new): the factor is uniform per lane (the query is the lane's column) and exactly 1 where the maximum did not move, so there is no branch on the data.
//   * m starts from the first tile's real scores (tile 0 never rescales); every tile holds at least one live key, so no expression forms (-inf) - (-inf).
//   * dead key columns exist only in the last tile (N mod 32 != 0): they take no part in the maximum and their p is 0.
//   * LDS, filled once per workgroup: the head's bias table ((2w - 1)^2 floats), the tokens' pixel and code (5 bits per coordinate, the band above them) and each key's
//     1 / max(||k||, 1e-12), so that a key tile is not normalised again by every query tile.  Entries N .. 32 T - 1 mirror token 0: every address stays in range.
//   * K and V tiles come from L2 once per query tile; the next tile's loads are issued before the current tile's arithmetic.
// No atomics; one barrier, which every wave reaches (a wave without a query tile only skips the loop behind it).
// ---------------------------------------------------------------------------------------
constexpr int WIDE_MAX_W = 24, WIDE_MAX_N = WIDE_MAX_W * WIDE_MAX_W, WIDE_MAX_REL = (2 * WIDE_MAX_W - 1) * (2 * WIDE_MAX_W - 1);

typedef int i32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void window_attn_v2_wide_kernel(WindowAttnV2Args a) {
  __shared__ float tbl[WIDE_MAX_REL];
  __shared__ __attribute__((aligned(16))) int tok_pix[WIDE_MAX_N];
  __shared__ __attribute__((aligned(16))) int tok_code[WIDE_MAX_N];
  __shared__ float k_inv[WIDE_MAX_N];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const int w = a.w, N = w * w, T = (N + 31) >> 5;
  const int pH = (a.H + w - 1) / w * w, pW = (a.W + w - 1) / w * w;
  const int nwh = pH / w, nww = pW / w;
  const int head = (int)(blockIdx.x % (unsigned)a.heads);
  unsigned win = blockIdx.x / (unsigned)a.heads;
  const int wx = (int)(win % (unsigned)nww);
  win /= (unsigned)nww;
  const int wy = (int)(win % (unsigned)nwh);
  const int b = (int)(win / (unsigned)nwh);
  const int rel = (2 * w - 1) * (2 * w - 1);
  const int C3 = 3 * a.C;
  for (int i = threadIdx.x; i < rel; i += 256) tbl[i] = a.table[(size_t)head * rel + i];
  for (int i = threadIdx.x; i < T * 32; i += 256) {
    const int t = i < N ? i : 0;
    const int ty = t / w, tx = t - ty * w;
    int y = wy * w + ty + a.shift, x = wx * w + tx + a.shift;
    if (y >= pH) y -= pH;
    if (x >= pW) x -= pW;
    const int band = ((a.shift > 0 && wy == nwh - 1 && ty >= w - a.shift) ? 2 : 0) | ((a.shift > 0 && wx == nww - 1 && tx >= w - a.shift) ? 1 : 0);
    const int pix = (y < a.H && x < a.W) ? (b * a.H + y) * a.W + x : -1;
    tok_pix[i] = pix;
    tok_code[i] = ty | (tx << 5) | (band << 10);
    const float* kb = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias) + a.C + head * 32;
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
    const float* kb = (pk >= 0 ? a.qkv + (size_t)pk * C3 : a.qkv_bias) + a.C + hoff + half * 16;
#pragma unroll
    for (int v4 = 0; v4 < 4; ++v4) {
      const f32x4 kv = *reinterpret_cast<const f32x4*>(kb + v4 * 4);
#pragma unroll
      for (int e = 0; e < 4; ++e) kr[v4 * 4 + e] = kv[e];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const i32x4 p4 = *reinterpret_cast<const i32x4*>(&tok_pix[tj * 32 + 8 * g + 4 * half]);
#pragma unroll
      for (int e = 0; e < 4; ++e) vr[g * 4 + e] = (p4[e] >= 0 ? a.qkv + (size_t)p4[e] * C3 : a.qkv_bias)[2 * a.C + hoff + l31];
    }
  };
  for (int ti = wave; ti < T; ti += 4) {
    const int tq = ti * 32 + l31;
    const int pixq = tok_pix[tq];
    const int ci = tok_code[tq];
    const int tyi = ci & 31, txi = (ci >> 5) & 31, bi = ci >> 10;
    const int qrow = (tyi + w - 1) * (2 * w - 1) + (txi + w - 1);
    float q[16];
    {
      const float* qb = (pixq >= 0 ? a.qkv + (size_t)pixq * C3 : a.qkv_bias) + hoff + half * 16;
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
        v[e] = (tj * 32 + 8 * (e >> 2) + 4 * half + (e & 3)) < N ? vn[e] : 0.f;
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
        const i32x4 c4 = *reinterpret_cast<const i32x4*>(&tok_code[tj * 32 + 8 * g + 4 * half]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = g * 4 + e;
          const int cj = c4[e];
          const int tyj = cj & 31, txj = (cj >> 5) & 31, bj = cj >> 10;
          float val = s[r] + tbl[qrow - tyj * (2 * w - 1) - txj];
          if (bi != bj) val += -200.0f;
          s[r] = val;
          if (tj * 32 + 8 * g + 4 * half + e < N) tmx = fmaxf(tmx, val);  // dead key columns take no part in the softmax
        }
      }
      tmx = fmaxf(tmx, __shfl_xor(tmx, 32, 64));  // finite: every tile has a live key
      const float m_new = tj == 0 ? tmx : fmaxf(m, tmx);
      const float f = tj == 0 ? 1.0f : exp_comp(m - m_new);
      m = m_new;
      float ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = (tj * 32 + 8 * (r >> 2) + 4 * half + (r & 3)) < N ? exp_comp(s[r] - m_new) : 0.f;
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
      float* out = a.dst + (size_t)pixq * a.C + hoff + 4 * half;
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

int launch_window_attn_v2_wide(const WindowAttnV2Args& a, hipStream_t s) {
  PH_REQUIRE(a.qkv && a.table && a.qkv_bias && a.scale && a.dst, "key-tiled cosine window attention: null pointer");
  PH_REQUIRE(a.w >= 2 && a.w <= WIDE_MAX_W, "key-tiled cosine window attention: window_size %d is outside 2..%d", a.w, WIDE_MAX_W);
  PH_REQUIRE(a.heads > 0 && a.C == a.heads * 32, "key-tiled cosine window attention: head dimension must be 32 (C %d, heads %d)", a.C, a.heads);
  PH_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && (long long)a.B * a.H * a.W < (1ll << 31) / 4, "key-tiled cosine window attention: bad map size");
  PH_REQUIRE(a.shift >= 0 && a.shift < a.w, "key-tiled cosine window attention: shift must be smaller than the window");
  const long long blocks = (long long)a.B * ((a.H + a.w - 1) / a.w) * ((a.W + a.w - 1) / a.w) * a.heads;
  PH_REQUIRE(blocks < (1ll << 31), "key-tiled cosine window attention: too many windows");
  hipLaunchKernelGGL(window_attn_v2_wide_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
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
  WindowAttnV2Args a{};
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
  a.shift = shift;
  const int rc = launch_window_attn_v2(a, nullptr);
  PH_HIP_CHECK(hipDeviceSynchronize());
  return rc;
}

// Test support (tests/test_gpu_window_attn_v2_wide.py), not a product path: one launch of the key-tiled kernel on tensors the caller owns, through
// launch_window_attn_v2_wide and its checks (windows 2..24: the product path sends it 9..24 only), synchronised before it returns.
extern "C" int ph_debug_window_attn_v2_wide_run(const float* qkv, const float* qkv_bias, const float* scale, const float* table, float* dst, int32_t B, int32_t H, int32_t W,
                                                int32_t heads, int32_t w, int32_t shift) {
  PH_REQUIRE(heads > 0, "ph_debug_window_attn_v2_wide_run: heads must be positive");  // (the pointers are the launcher's check: "null pointer")
  WindowAttnV2Args a{};
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
  a.shift = shift;
  const int rc = launch_window_attn_v2_wide(a, nullptr);
  PH_HIP_CHECK(hipDeviceSynchronize());
  return rc;
}
