// Swin Transformer encoder kernels for gfx950 (MI355X, CDNA4).
//
// Reference semantics (torchvision's public SwinTransformer definition, instantiated by the reference at
// architectures/swint.py): shifted_window_attention and PatchMerging.  Activations are the NHWC fp32 slots of the
// ConvNeXt path; the Linear layers around these kernels are the ordinary row GEMMs.
//
//   window_attn_kernel ..... pad to window multiples, roll by (-sh, -sw), cut into w x w windows, per head
//                            softmax(q k^T / sqrt(32) + bias [+ band mask]) v, un-window, roll back, crop --
//                            all of it index arithmetic on the loads and stores of one launch.  Its cosine variant is
//                            the Swinv2 attention of windows up to 8 (launch_window_attn_v2).
//   patch_merge_ln_kernel .. gather of the four 2x2 phases to 4C channels + LayerNorm over them.
#include <algorithm>

#include "common.h"
#include "device_math.h"
#include "net_kernels.h"

namespace ph {

// The one argument check of the five launchers (window_attn.h)
int window_attn_check(const char* label, int max_w, bool pointers, const WindowGeom& a, WindowGrid* g, int per_block, unsigned* blocks) {
  PH_REQUIRE(pointers, "%s: null pointer", label);
  PH_REQUIRE(a.w >= 2 && a.w <= max_w, "%s: window_size %d is outside 2..%d", label, a.w, max_w);
  PH_REQUIRE(a.heads > 0 && a.C == a.heads * 32, "%s: head dimension must be 32 (C %d, heads %d)", label, a.C, a.heads);
  PH_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && (long long)a.B * a.H * a.W < (1ll << 31) / 4, "%s: bad map size", label);
  PH_REQUIRE(a.sh >= 0 && a.sh < a.w && a.sw >= 0 && a.sw < a.w, "%s: shift must be smaller than the window", label);
  *g = window_grid(a.B, a.H, a.W, a.w);
  if (blocks) {
    const long long n = (g->nwin * a.heads + per_block - 1) / per_block;
    PH_REQUIRE(n < (1ll << 31), "%s: too many windows", label);
    *blocks = (unsigned)n;
  }
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// One wave = one (window, head); four waves (consecutive heads, then the next window) per workgroup.  N = w^2 <= 64
// tokens, head dimension 32, T = ceil(N / 32) 32-token tiles.  Everything lives in registers:
//   S^T = K Q^T on v_mfma_f32_32x32x2_f32 (A = K, B = Q; the two lane halves hold channels 0..15 / 16..31 of their
//   token, the same permutation of the K index on both operands, so the loads are four dwordx4 per token).  The
//   transposed product puts query i in the lane (column l & 31) and the keys window_key(tj, r, l >> 5) in its
//   accumulator registers: bias, mask, row maximum and row sum are lane-local plus one exchange with lane l ^ 32.
//   O^T = V^T P^T takes those registers as its B operand unchanged (K index = key j in the accumulator order), with V
//   loaded in the same key order as its A operand; O^T again has the query in the lane, four consecutive channels in
//   each register quad: the stores are dwordx4 at the token's ORIGINAL pixel.
// Token geometry, padded tokens and the band mask: window_attn.h.
// COSINE (Swinv2; exact fp32 as the plain variant, same registers, lanes and accumulator order) changes four things:
//   * q and k are divided by max(||.||_2, 1e-12) over the head's 32 channels (F.normalize): a lane holds 16 of them, the
//     sum of squares takes one exchange with lane l ^ 32.  The head's scale exp(min(logit_scale, log 100)) (a.scale,
//     computed by the host) is folded into q behind the normalisation.  A padded token has hidden state 0: q =
//     query.bias, k = 0 exactly (the key section of a.qkv_bias is zero, its normalised k is 0 / 1e-12 = 0), v = value.bias.
//   * the band mask adds -200, not -100: Swinv2SelfAttention.forward adds the (-100) mask TWICE.  With |q.k| scale <= 100
//     and a bias in (0, 16) a masked score can stay above an unmasked one: the constant is part of the arithmetic, not
//     a stand-in for minus infinity.
//   * exp_comp instead of exp_hw: the scores go far enough from the maximum for the argument's rounding to show.
//   * a dead key column (j >= N) is skipped by a guard; the plain variant gives it a score of -inf and lets exp_hw
//     return 0.  Both give p = 0; each variant keeps the form it was compiled with (code objects).
// ---------------------------------------------------------------------------------------
template <int T, bool COSINE>
__global__ __launch_bounds__(256) void window_attn_kernel(WindowAttnArgs a) {
  __shared__ float tbl[4][232];
  __shared__ int tok_pix[4][64];
  __shared__ int tok_code[4][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const WindowGrid grid = window_grid(a.B, a.H, a.W, a.w);
  const int w = grid.w, N = grid.N, rel = grid.rel;
  const long long total = grid.nwin * a.heads;
  long long item = (long long)blockIdx.x * 4 + wave;
  const bool live = item < total;
  if (!live) item = total - 1;
  const WindowItem it = window_decode(grid, item, a.heads);
  const int head = it.head;
  for (int i = lane; i < rel; i += 64) tbl[wave][i] = a.table[(size_t)head * rel + i];
  {
    const TokenInfo tk = window_token<4>(grid, it, lane < N ? lane : 0, a.sh, a.sw);  // (dead lanes mirror token 0: their table index stays in range)
    tok_pix[wave][lane] = tk.pix;
    tok_code[wave][lane] = tk.code;
  }
  __syncthreads();
  const int C3 = 3 * a.C;
  const float* qkv = static_cast<const float*>(a.qkv);
  const float qscale = COSINE ? a.scale[head] : 0.17677669529663688f;  // the head's scale, applied behind the normalisation : 32^-0.5
  // Q and K: token ti * 32 + (l & 31), channels 16 half .. 16 half + 15 of the head (cosine: each divided by its token's norm over all 32)
  float q[T][16], k[T][16];
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int t = ti * 32 + l31;
    const int pix = tok_pix[wave][t];
    const float* base = (pix >= 0 ? qkv + (size_t)pix * C3 : a.qkv_bias) + head * 32 + half * 16;
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
        if constexpr (COSINE) {
          q[ti][v4 * 4 + e] = qv[e];
          qss = fmaf(qv[e], qv[e], qss);
          kss = fmaf(kv[e], kv[e], kss);
        } else {
          q[ti][v4 * 4 + e] = qv[e] * qscale;
        }
        k[ti][v4 * 4 + e] = kv[e];
      }
    }
    if constexpr (COSINE) {
      qss += __shfl_xor(qss, 32, 64);
      kss += __shfl_xor(kss, 32, 64);
      const float qn = qscale / fmaxf(sqrtf(qss), 1e-12f), kn = 1.0f / fmaxf(sqrtf(kss), 1e-12f);
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        q[ti][e] *= qn;
        k[ti][e] *= kn;
      }
    }
  }
  // V: key j(tj, r, half), channel l & 31 of the head
  float v[T][16];
#pragma unroll
  for (int tj = 0; tj < T; ++tj)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = window_key(tj, r, half);
      float val = 0.f;
      if (j < N) {
        const int pix = tok_pix[wave][j];
        val = (pix >= 0 ? qkv + (size_t)pix * C3 : a.qkv_bias)[2 * a.C + head * 32 + l31];
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
    float mx = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = window_key(tj, r, half);
        auto score = [&] {
          const int cj = tok_code[wave][j];
          float val = s[tj][ti][r] + tbl[wave][window_bias_index<4>(ci, cj, w)];
          if (token_band<4>(ci) != token_band<4>(cj)) val += COSINE ? -200.0f : -100.0f;
          return val;
        };
        // dead key columns take no part in the softmax
        if constexpr (COSINE) {
          if (j < N) {
            const float val = score();
            s[tj][ti][r] = val;
            mx = fmaxf(mx, val);
          }
        } else {
          float val = score();
          if (j >= N) val = -INFINITY;
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
        float p;
        if constexpr (COSINE)
          p = window_key(tj, r, half) < N ? exp_comp(s[tj][ti][r] - mx) : 0.f;
        else
          p = exp_hw(s[tj][ti][r] - mx);
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
      float* out = static_cast<float*>(a.dst) + (size_t)pix * a.C + head * 32 + 4 * half;
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

template <bool COSINE>
static int launch_window_attn_variant(const char* label, const WindowAttnArgs& a, hipStream_t s) {
  WindowGrid g;
  unsigned blocks;
  const int rc = window_attn_check(label, 8, a.qkv && a.table && a.qkv_bias && a.dst && (a.scale || !COSINE), a, &g, 4, &blocks);
  if (rc != PH_OK) return rc;
  if (g.N <= 32)
    hipLaunchKernelGGL((window_attn_kernel<1, COSINE>), dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((window_attn_kernel<2, COSINE>), dim3(blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
int launch_window_attn(const WindowAttnArgs& a, hipStream_t s) { return launch_window_attn_variant<false>("window attention", a, s); }
int launch_window_attn_v2(const WindowAttnArgs& a, hipStream_t s) { return launch_window_attn_variant<true>("cosine window attention", a, s); }

// ---------------------------------------------------------------------------------------
// Patch merging up to its Linear: out pixel (oy, ox) = LayerNorm(concat(x[2oy][2ox], x[2oy+1][2ox], x[2oy][2ox+1],
// x[2oy+1][2ox+1])) over 4C channels, zeros where an odd map ends.  One wave per output pixel; two-pass mean / biased
// variance as layernorm_kernel (the second and third pass re-read the four source pixels from L1 / L2).
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_merge_ln_kernel(const float* __restrict__ src, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                             float* __restrict__ dst, int B, int H, int W, int c, float eps) {
  const int lane = threadIdx.x & 63;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const size_t npix = (size_t)B * OH * OW;
  const int cq = c >> 2, quads = cq * 4;
  const float inv_c = 1.0f / (float)(4 * c);
  for (size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); pix < npix; pix += (size_t)gridDim.x * 4) {
    const int ox = (int)(pix % OW);
    const int oy = (int)((pix / OW) % OH);
    const int b = (int)(pix / ((size_t)OW * OH));
    auto load = [&](int qd) {
      const int ph = qd / cq, cc = qd - ph * cq;
      const int y = 2 * oy + (ph & 1), x = 2 * ox + (ph >> 1);
      if (y >= H || x >= W) return f32x4{0.f, 0.f, 0.f, 0.f};
      return *reinterpret_cast<const f32x4*>(src + ((size_t)(b * H + y) * W + x) * c + cc * 4);
    };
    float s = 0.f;
    for (int qd = lane; qd < quads; qd += 64) {
      const f32x4 v = load(qd);
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    const float mean = s * inv_c;
    float ss = 0.f;
    for (int qd = lane; qd < quads; qd += 64) {
      const f32x4 v = load(qd);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float d = v[e] - mean;
        ss += d * d;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    const float rstd = 1.0f / sqrtf(ss * inv_c + eps);
    float* o = dst + pix * (size_t)(4 * c);
    for (int qd = lane; qd < quads; qd += 64) {
      const f32x4 v = load(qd);
      const f32x4 g = *reinterpret_cast<const f32x4*>(gamma + qd * 4);
      const f32x4 bt = *reinterpret_cast<const f32x4*>(beta + qd * 4);
      f32x4 r;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = (v[e] - mean) * rstd * g[e] + bt[e];
      *reinterpret_cast<f32x4*>(o + qd * 4) = r;
    }
  }
}

int launch_patch_merge_ln(const float* src, const float* gamma, const float* beta, float* dst, int B, int H, int W, int c, float eps, hipStream_t s) {
  PH_REQUIRE(src && gamma && beta && dst && B > 0 && H > 0 && W > 0, "patch merge: bad arguments");
  PH_REQUIRE(c > 0 && (c & 3) == 0, "patch merge: channel count %d must be a multiple of 4", c);
  const size_t npix = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2);
  const int blocks = (int)std::min<size_t>((npix + 3) / 4, 256 * 32);
  hipLaunchKernelGGL(patch_merge_ln_kernel, dim3(blocks), dim3(256), 0, s, src, gamma, beta, dst, B, H, W, c, eps);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

template <int BITS>
static void fill_window_tokens(const WindowGrid& g, int sh, int sw, int32_t* pix, int32_t* code) {
  for (long long win = 0; win < g.nwin; ++win) {
    const WindowItem it = window_decode(g, win, 1);
    for (int t = 0; t < g.N; ++t) {
      const TokenInfo tk = window_token<BITS>(g, it, t, sh, sw);
      pix[win * g.N + t] = tk.pix;
      code[win * g.N + t] = tk.code;
    }
  }
}

}  // namespace ph

// Test support (tests/test_window_geometry_cpu.py), not a product path: the token map of a launch, [window][N] in the kernels' window order (b, wy, wx), from the
// functions the kernels call (window_attn.h).  Host code only: no HIP call.
extern "C" int ph_debug_window_tokens(int32_t B, int32_t H, int32_t W, int32_t w, int32_t sh, int32_t sw, int32_t code_bits, int32_t* pix_out, int32_t* code_out,
                                      int64_t capacity) {
  using namespace ph;
  PH_REQUIRE(pix_out && code_out, "ph_debug_window_tokens: null pointer");
  PH_REQUIRE(w >= 2 && w <= 24, "ph_debug_window_tokens: window_size %d is outside 2..24", w);
  PH_REQUIRE(code_bits == 5 || (code_bits == 4 && w <= 16), "ph_debug_window_tokens: code_bits %d cannot hold the coordinates of window %d (4: up to 16, 5: up to 24)", code_bits, w);
  PH_REQUIRE(B > 0 && H > 0 && W > 0 && (long long)B * H * W < (1ll << 31) / 4, "ph_debug_window_tokens: bad map size");
  PH_REQUIRE(sh >= 0 && sh < w && sw >= 0 && sw < w, "ph_debug_window_tokens: shift must be smaller than the window");
  const WindowGrid g = window_grid(B, H, W, w);
  PH_REQUIRE(capacity >= g.nwin * g.N, "ph_debug_window_tokens: capacity %lld is below the %lld tokens of the launch", (long long)capacity, g.nwin * g.N);
  if (code_bits == 4)
    fill_window_tokens<4>(g, sh, sw, pix_out, code_out);
  else
    fill_window_tokens<5>(g, sh, sw, pix_out, code_out);
  return PH_OK;
}
