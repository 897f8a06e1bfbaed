// Swin Transformer encoder kernels for gfx950 (MI355X, CDNA4).
//
// Reference semantics (torchvision's public SwinTransformer definition, instantiated by the reference at
// architectures/swint.py): shifted_window_attention and PatchMerging.  Activations are the NHWC fp32 slots of the
// ConvNeXt path; the Linear layers around these kernels are the ordinary row GEMMs.
//
//   window_attn_kernel ..... pad to window multiples, roll by (-sh, -sw), cut into w x w windows, per head
//                            softmax(q k^T / sqrt(32) + bias [+ band mask]) v, un-window, roll back, crop --
//                            all of it index arithmetic on the loads and stores of one launch.
//   patch_merge_ln_kernel .. gather of the four 2x2 phases to 4C channels + LayerNorm over them.
#include <algorithm>

#include "common.h"
#include "device_math.h"
#include "net_kernels.h"

namespace ph {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------
// One wave = one (window, head); four waves (consecutive heads, then the next window) per workgroup.  N = w^2 <= 64
// tokens, head dimension 32, T = ceil(N / 32) 32-token tiles.  Everything lives in registers:
//   S^T = K Q^T on v_mfma_f32_32x32x2_f32 (A = K, B = Q; the two lane halves hold channels 0..15 / 16..31 of their
//   token, the same permutation of the K index on both operands, so the loads are four dwordx4 per token).  The
//   transposed product puts query i in the lane (column l & 31) and the keys j = 8 (r >> 2) + 4 (l >> 5) + (r & 3) in its
//   accumulator registers: bias, mask, row maximum and row sum are lane-local plus one exchange with lane l ^ 32.
//   O^T = V^T P^T takes those registers as its B operand unchanged (K index = key j in the accumulator order), with V
//   loaded in the same key order as its A operand; O^T again has the query in the lane, four consecutive channels in
//   each register quad: the stores are dwordx4 at the token's ORIGINAL pixel.
// A token's rolled, padded grid position (ry, rx) = (wy w + ty, wx w + tx) comes from pixel ((ry + sh) mod pH,
// (rx + sw) mod pW); past the map it is a padded token: q, k, v = qkv.bias, a key like any other, never stored.
// Band mask of the shifted block: only the last window row / column holds two bands, split at w - shift.
// ---------------------------------------------------------------------------------------
struct TokenInfo {
  int pix;   // pixel index (b H + y) W + x, -1 = padded token
  int code;  // ty | tx << 4 | band << 8
};

template <int T>
__global__ __launch_bounds__(256) void window_attn_kernel(WindowAttnArgs a) {
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
    int y = wy * w + ty + a.sh, x = wx * w + tx + a.sw;
    if (y >= pH) y -= pH;
    if (x >= pW) x -= pW;
    const int band = ((a.sh > 0 && wy == nwh - 1 && ty >= w - a.sh) ? 2 : 0) | ((a.sw > 0 && wx == nww - 1 && tx >= w - a.sw) ? 1 : 0);
    tok_pix[wave][lane] = (y < a.H && x < a.W) ? (b * a.H + y) * a.W + x : -1;
    tok_code[wave][lane] = ty | (tx << 4) | (band << 8);
  }
  __syncthreads();
  const int C3 = 3 * a.C;
  const float qscale = 0.17677669529663688f;  // 32^-0.5
  // Q and K: token ti * 32 + (l & 31), channels 16 half .. 16 half + 15 of the head
  float q[T][16], k[T][16];
#pragma unroll
  for (int ti = 0; ti < T; ++ti) {
    const int t = ti * 32 + l31;
    const int pix = tok_pix[wave][t];
    const float* base = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias) + head * 32 + half * 16;
    const bool on = t < N;
#pragma unroll
    for (int v4 = 0; v4 < 4; ++v4) {
      f32x4 qv = {0.f, 0.f, 0.f, 0.f}, kv = {0.f, 0.f, 0.f, 0.f};
      if (on) {
        qv = *reinterpret_cast<const f32x4*>(base + v4 * 4);
        kv = *reinterpret_cast<const f32x4*>(base + a.C + v4 * 4);
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        q[ti][v4 * 4 + e] = qv[e] * qscale;
        k[ti][v4 * 4 + e] = kv[e];
      }
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
        const int cj = tok_code[wave][j];
        const int tyj = cj & 15, txj = (cj >> 4) & 15, bj = cj >> 8;
        float val = s[tj][ti][r] + tbl[wave][(tyi - tyj + w - 1) * (2 * w - 1) + (txi - txj + w - 1)];
        if (bi != bj) val += -100.0f;
        if (j >= N) val = -INFINITY;  // dead key columns take no part in the softmax
        s[tj][ti][r] = val;
        mx = fmaxf(mx, val);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int tj = 0; tj < T; ++tj)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = exp_hw(s[tj][ti][r] - mx);
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

int launch_window_attn(const WindowAttnArgs& a, hipStream_t s) {
  PH_REQUIRE(a.qkv && a.table && a.qkv_bias && a.dst, "window attention: null pointer");
  PH_REQUIRE(a.w >= 2 && a.w <= 8, "window attention: window_size %d is outside 2..8", a.w);
  PH_REQUIRE(a.heads > 0 && a.C == a.heads * 32, "window attention: head dimension must be 32 (C %d, heads %d)", a.C, a.heads);
  PH_REQUIRE(a.B > 0 && a.H > 0 && a.W > 0 && (long long)a.B * a.H * a.W < (1ll << 31) / 4, "window attention: bad map size");
  PH_REQUIRE(a.sh >= 0 && a.sh < a.w && a.sw >= 0 && a.sw < a.w, "window attention: shift must be smaller than the window");
  const long long nwin = (long long)a.B * ((a.H + a.w - 1) / a.w) * ((a.W + a.w - 1) / a.w);
  const long long blocks = (nwin * a.heads + 3) / 4;
  PH_REQUIRE(blocks < (1ll << 31), "window attention: too many windows");
  if (a.w * a.w <= 32)
    hipLaunchKernelGGL(window_attn_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL(window_attn_kernel<2>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

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

}  // namespace ph
