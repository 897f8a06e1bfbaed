// Swin Transformer encoder kernels on plain-fp16 activations (FMT_F16, act_format.h) for gfx950: the fp16 forms of
// swin_kernels.hip (reference semantics there).  The Linear layers around them are gemm_f16_kernel, the norms
// layernorm_f16_kernel (convnext_f16_kernels.hip).  All Swin widths are multiples of 32 (head dimension 32): no pad channels.
//
//   window_attn_f16_kernel ..... window_attn_kernel's plan on v_mfma_f32_32x32x16_f16: fp16 q, k, v, fp32 logits and softmax
//                                statistics, p rounded to fp16 as the second product's operand, fp16 output.
//   patch_merge_ln_f16_kernel .. gather of the four 2x2 phases to 4C channels + LayerNorm over them, fp32 moments, fp16 in and out.
// What is rounded where: tools/swint_f16_emulation.py.
#include <algorithm>

#include "act_format.h"
#include "common.h"
#include "device_math.h"
#include "net_kernels.h"

namespace ph {

// ---------------------------------------------------------------------------------------
// One wave = one (window, head); four waves (consecutive heads, then the next window) per workgroup, as window_attn_kernel.
// N = w^2 <= 64 tokens, head dimension 32, T = ceil(N / 32) 32-token tiles, everything in registers:
//   S^T = K Q^T: two v_mfma_f32_32x32x16_f16 per tile pair (A = K, B = Q).  Lane half h holds channels 16 h .. 16 h + 15 of its
//   token (two 16-byte loads); K step s takes elements 8 s .. 8 s + 7 of them on BOTH operands -- the same permutation of the
//   K index, so the product is q . k.  The 32^-0.5 scale goes on the fp32 accumulator.  Query i is the lane (column l & 31), the
//   keys window_key(tj, r, h) its accumulator registers: bias, mask, row maximum and row sum are lane-local plus one
//   exchange with lane l ^ 32.  p = fp16(exp(s - max)); the row sum is taken over the ROUNDED p.
//   O^T = V^T P^T: registers 8 s .. 8 s + 7 of a P^T tile, converted, are the B operand of K step s as they stand (K index
//   8 h + e <-> key 16 s + 8 (e >> 2) + 4 h + (e & 3)); V is loaded in that key order as the A operand (row = channel l & 31:
//   2-byte loads, 64 contiguous bytes per wave half-row).  O^T has the query in the lane and four consecutive channels in each
//   register quad: 8-byte stores at the token's ORIGINAL pixel.
// Token geometry, padded tokens (q, k, v = fp16(qkv.bias), read from the fp32 vector) and the band mask: window_attn.h.
// ---------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void window_attn_f16_kernel(WindowAttnArgs a) {
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
  const float qscale = 0.17677669529663688f;  // 32^-0.5
  const _Float16* qkv = reinterpret_cast<const _Float16*>(a.qkv);
  // Q and K: token ti * 32 + (l & 31), channels 16 half .. 16 half + 15 of the head; [ti][K step]
  f16x8 q[T][2], k[T][2];
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int t = ti * 32 + l31;
    const int pix = tok_pix[wave][t];
    const int ch = head * 32 + half * 16;
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        q[ti][s][e] = (_Float16)0.f;
        k[ti][s][e] = (_Float16)0.f;
      }
    if (t < N) {
      if (pix >= 0) {
        const _Float16* base = qkv + (size_t)pix * C3 + ch;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          q[ti][s] = *reinterpret_cast<const f16x8*>(base + 8 * s);
          k[ti][s] = *reinterpret_cast<const f16x8*>(base + a.C + 8 * s);
        }
      } else {
        const float* base = a.qkv_bias + ch;
#pragma unroll
        for (int v4 = 0; v4 < 4; ++v4) {
          const f32x4 qv = *reinterpret_cast<const f32x4*>(base + v4 * 4);
          const f32x4 kv = *reinterpret_cast<const f32x4*>(base + a.C + v4 * 4);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            q[ti][v4 >> 1][(v4 & 1) * 4 + e] = (_Float16)qv[e];
            k[ti][v4 >> 1][(v4 & 1) * 4 + e] = (_Float16)kv[e];
          }
        }
      }
    }
  }
  // V: [tj][K step s][e] = key window_key(tj, 8 s + e, half), channel l & 31 of the head
  f16x8 v[T][2];
#pragma unroll
  for (int tj = 0; tj < T; ++tj)
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int j = window_key(tj, 8 * s + e, half);
        _Float16 val = (_Float16)0.f;
        if (j < N) {
          const int pix = tok_pix[wave][j];
          const int ch = 2 * a.C + head * 32 + l31;
          val = pix >= 0 ? qkv[(size_t)pix * C3 + ch] : (_Float16)a.qkv_bias[ch];
        }
        v[tj][s][e] = val;
      }
  // S^T tiles [tj][ti]
  f32x16 st[T][T];
#pragma unroll
  for (int tj = 0; tj < T; ++tj)
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
      f32x16 acc;
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
      for (int s = 0; s < 2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(k[tj][s], q[ti][s], acc, 0, 0, 0);
      st[tj][ti] = acc;
    }
  // scale, bias, band mask, softmax over the keys of each query (= this lane's column), then O^T
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int ci = tok_code[wave][ti * 32 + l31];
    float mx = -INFINITY;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = window_key(tj, r, half);
        const int cj = tok_code[wave][j];
        float val = st[tj][ti][r] * qscale + tbl[wave][window_bias_index<4>(ci, cj, w)];
        if (token_band<4>(ci) != token_band<4>(cj)) val += -100.0f;
        if (j >= N) val = -INFINITY;  // dead key columns take no part in the softmax
        st[tj][ti][r] = val;
        mx = fmaxf(mx, val);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
    f16x8 p[T][2];
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const _Float16 ph = (_Float16)exp_hw(st[tj][ti][r] - mx);
        p[tj][r >> 3][r & 7] = ph;
        sum += (float)ph;  // over the rounded operand: what the second product multiplies
      }
    sum += __shfl_xor(sum, 32, 64);
    const float inv_sum = 1.0f / sum;
    // O^T[c][i] = sum_j V[j][c] P[i][j]
    f32x16 o;
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int s = 0; s < 2; ++s) o = __builtin_amdgcn_mfma_f32_32x32x16_f16(v[tj][s], p[tj][s], o, 0, 0, 0);
    // query ti * 32 + (l & 31): channels 8 g + 4 half + (0..3) of the head, at the token's own pixel
    const int t = ti * 32 + l31;
    const int pix = tok_pix[wave][t];
    if (live && t < N && pix >= 0) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float r4[4] = {o[g * 4] * inv_sum, o[g * 4 + 1] * inv_sum, o[g * 4 + 2] * inv_sum, o[g * 4 + 3] * inv_sum};
        store4<FMT_F16>(a.dst, (size_t)pix, a.C, head * 32 + 8 * g + 4 * half, r4);
      }
    }
  }
}

int launch_window_attn_f16(const WindowAttnArgs& a, hipStream_t s) {
  WindowGrid g;
  unsigned blocks;
  const int rc = window_attn_check("window attention (fp16)", 8, a.qkv && a.table && a.qkv_bias && a.dst, a, &g, 4, &blocks);
  if (rc != PH_OK) return rc;
  if (g.N <= 32)
    hipLaunchKernelGGL(window_attn_f16_kernel<1>, dim3(blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(window_attn_f16_kernel<2>, dim3(blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Patch merging up to its Linear on fp16 storage: patch_merge_ln_kernel with 16-byte loads of eight halves.  One wave per
// output pixel; two-pass mean / biased variance in fp32 over the 4C gathered channels (zeros where an odd map ends take part
// in the moments, as the reference's padding does); the second and third pass re-read the four source pixels from L1 / L2.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_merge_ln_f16_kernel(const void* __restrict__ src_, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                 void* __restrict__ dst, int B, int H, int W, int c, float eps) {
  const int lane = threadIdx.x & 63;
  const int OH = (H + 1) / 2, OW = (W + 1) / 2;
  const size_t npix = (size_t)B * OH * OW;
  const int co = c >> 3, octs = co * 4;
  const float inv_c = 1.0f / (float)(4 * c);
  const _Float16* src = reinterpret_cast<const _Float16*>(src_);
  for (size_t pix = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); pix < npix; pix += (size_t)gridDim.x * 4) {
    const int ox = (int)(pix % OW);
    const int oy = (int)((pix / OW) % OH);
    const int b = (int)(pix / ((size_t)OW * OH));
    auto load = [&](int og, float (&v)[8]) {
      const int ph = og / co, cc = og - ph * co;
      const int y = 2 * oy + (ph & 1), x = 2 * ox + (ph >> 1);
      if (y >= H || x >= W) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        return;
      }
      load8<FMT_F16>(src, (size_t)(b * H + y) * W + x, c, cc, v);
    };
    float v[8];
    float s = 0.f;
    for (int og = lane; og < octs; og += 64) {
      load(og, v);
      s += ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
    const float mean = s * inv_c;
    float ss = 0.f;
    for (int og = lane; og < octs; og += 64) {
      load(og, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[e] - mean;
        ss += d * d;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) ss += __shfl_xor(ss, m, 64);
    const float rstd = 1.0f / sqrtf(ss * inv_c + eps);
    for (int og = lane; og < octs; og += 64) {
      load(og, v);
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gamma + og * 8), g1 = *reinterpret_cast<const f32x4*>(gamma + og * 8 + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(beta + og * 8), b1 = *reinterpret_cast<const f32x4*>(beta + og * 8 + 4);
      float r[8];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        r[e] = (v[e] - mean) * rstd * g0[e] + b0[e];
        r[4 + e] = (v[4 + e] - mean) * rstd * g1[e] + b1[e];
      }
      store8<FMT_F16>(dst, pix, 4 * c, og, r);
    }
  }
}

int launch_patch_merge_ln_f16(const void* src, const float* gamma, const float* beta, void* dst, int B, int H, int W, int c, float eps, hipStream_t s) {
  PH_REQUIRE(src && gamma && beta && dst && B > 0 && H > 0 && W > 0, "patch merge (fp16): bad arguments");
  PH_REQUIRE(c > 0 && (c & 31) == 0, "patch merge (fp16): channel count %d must be a multiple of 32", c);
  const size_t npix = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2);
  const int blocks = (int)std::min<size_t>((npix + 3) / 4, 256 * 32);
  hipLaunchKernelGGL(patch_merge_ln_f16_kernel, dim3(blocks), dim3(256), 0, s, src, gamma, beta, dst, B, H, W, c, eps);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph
