// Swin Transformer training kernels for gfx950 (MI355X, CDNA4): the backward of swin_kernels.hip.
//
//   window_attn_bwd_kernel ... gradient of the shifted-window attention core with respect to the qkv slot, the
//                              relative-position bias table and (through the padded tokens) qkv.bias.
//   patch_merge_gather / scatter ... the four-phase gather of PatchMerging and its transpose; the LayerNorm between
//                              them is layernorm_bwd_kernel (convnext_train_kernels.hip).
//   grad_fanout / scale_samples / ... the residual fan-out and the per-sample branch scales (stochastic depth).
#include <algorithm>

#include "common.h"
#include "device_math.h"
#include "net_kernels.h"

namespace ph {

constexpr int WAB_SLICES = 256;  // workgroups of the attention backward = slices of its two fixed-order reductions

// ---------------------------------------------------------------------------------------
// One wave = one (window, head) at a time, four waves per workgroup, as window_attn_kernel; but a workgroup is one of
// at most WAB_SLICES slices and walks a fixed contiguous range of windows (items = (window, head) pairs of the range in
// order, item k on wave k & 3), so that the sums over windows have a fixed order.  With the notation of the forward
// (S = Qs K^T + bias + mask, Qs = q / sqrt(32), P = softmax(S), O = P V) and D_i = sum_j P_ij dP_ij:
//   dP = dO V^T,  dS = P * (dP - D),  dV = P^T dO,  dK = dS^T Qs,  dq = dS K / sqrt(32),  dtable[rel(i, j)] += dS_ij.
// Pass 1 (query in the lane): S^T = K Qs^T and dP^T = V dO^T on v_mfma_f32_32x32x2_f32 put query i in the lane and the
//   keys window_key(tj, r, l >> 5) in the accumulator registers, exactly the forward's layout: row maximum,
//   row sum and D_i are lane-local plus one exchange with lane l ^ 32; they go to a 64-float LDS row each.  dS^T is the
//   B operand of dq^T = K^T dS^T as it stands (K loaded key-major, as the forward loads V).  The dS tile also goes to
//   LDS (32 x 65 floats) for the table gradient: lane e owns table entry e + 64 n, walks the tile's queries i and reads
//   dS[i][i - offset(e)] where that key exists -- a gather, so no atomics.
// Pass 2 (key in the lane): S = Qs K^T and dP = dO V^T with the operands swapped put key j in the lane and the queries in
//   the registers; P = exp(S - m_i) / l_i with the statistics read back from LDS.  P and dS are then the B operands of
//   dV^T = dO^T P and dK^T = Qs^T dS (dO and Qs loaded query-major), with key j in the lane: dwordx4 stores at the token's pixel.
// Masked pairs carry -100, not -inf: they are in every sum, as in the forward.  Dead columns (j >= N) have P = 0; dead
// and padded queries have dO = 0, hence dS = 0.  A padded token's q, k, v are qkv.bias: its dq is zero (its output row is
// cropped), its dk and dv are summed over the window's padded tokens by a fixed butterfly and added to the wave's partial.
// Partials: [slice][wave][heads * rel | 2C] floats, zeroed by the launcher; a wave adds to its own row only (same lane,
// program order).  window_attn_bwd_final_kernel sums the rows in order.
// ---------------------------------------------------------------------------------------
template <int T>
__global__ __launch_bounds__(256) void window_attn_bwd_kernel(WindowAttnBwdArgs a, int per, int part_stride) {
  __shared__ float tbl[4][232];
  __shared__ int tok_pix[4][64];
  __shared__ int tok_code[4][64];
  __shared__ float st_m[4][64], st_il[4][64], st_d[4][64];
  __shared__ float dsl[4][32 * 65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int half = lane >> 5, l31 = lane & 31;
  const WindowGrid grid = window_grid(a.B, a.H, a.W, a.w);
  const int w = grid.w, N = grid.N, rel = grid.rel, w2 = 2 * w - 1;
  const long long nwin = grid.nwin;
  const long long lo = (long long)blockIdx.x * per;
  const long long hi = lo + per < nwin ? lo + per : nwin;
  const long long n_items = hi > lo ? (hi - lo) * a.heads : 0;
  const long long iters = (n_items + 3) / 4;
  const int C3 = 3 * a.C;
  const float qscale = 0.17677669529663688f;  // 32^-0.5
  float* pt = a.scratch + ((size_t)blockIdx.x * 4 + wave) * (size_t)part_stride;  // this wave's partial row: table part ...
  float* pp = pt + a.heads * rel;                                                  // ... and padded-token part (dk | dv)
  for (long long it = 0; it < iters; ++it) {
    long long item = it * 4 + wave;
    const bool live = item < n_items;
    if (!live) item = n_items - 1;
    const WindowItem wi = window_decode(grid, item, a.heads, lo);
    const int head = wi.head;
    __syncthreads();  // the previous item's readers of the LDS rows are done
    for (int i = lane; i < rel; i += 64) tbl[wave][i] = a.table[(size_t)head * rel + i];
    {
      const TokenInfo tk = window_token<4>(grid, wi, lane < N ? lane : 0, a.sh, a.sw);  // (dead lanes mirror token 0: their table index stays in range)
      tok_pix[wave][lane] = tk.pix;
      tok_code[wave][lane] = tk.code;
    }
    __syncthreads();
    const bool any_pad = __any(lane < N && tok_pix[wave][lane] < 0) != 0;
    // token-major operands: token ti * 32 + (l & 31), channels 16 half .. 16 half + 15 of the head
    float q[T][16], kr[T][16], vr[T][16], go[T][16];
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
      const int t = ti * 32 + l31;
      const int pix = tok_pix[wave][t];
      const bool on = t < N;
      const float* base = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias) + head * 32 + half * 16;
      const float* gbase = a.gout + (size_t)(pix >= 0 ? pix : 0) * a.C + head * 32 + half * 16;
#pragma unroll
      for (int v4 = 0; v4 < 4; ++v4) {
        f32x4 qv = {0.f, 0.f, 0.f, 0.f}, kv = qv, vv = qv, gv = qv;
        if (on) {
          qv = *reinterpret_cast<const f32x4*>(base + v4 * 4);
          kv = *reinterpret_cast<const f32x4*>(base + a.C + v4 * 4);
          vv = *reinterpret_cast<const f32x4*>(base + 2 * a.C + v4 * 4);
          if (pix >= 0) gv = *reinterpret_cast<const f32x4*>(gbase + v4 * 4);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          q[ti][v4 * 4 + e] = qv[e] * qscale;
          kr[ti][v4 * 4 + e] = kv[e];
          vr[ti][v4 * 4 + e] = vv[e];
          go[ti][v4 * 4 + e] = gv[e];
        }
      }
    }
    // ---- pass 1: query in the lane
    float tacc[4] = {0.f, 0.f, 0.f, 0.f};  // table entries lane + 64 n of this (window, head)
#pragma unroll
    for (int ti = 0; ti < T; ++ti) {
      f32x16 s[T], dp[T];
#pragma unroll
      for (int tj = 0; tj < T; ++tj) {
        f32x16 acc, acc2;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f, acc2[e] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          acc = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[tj][kk], q[ti][kk], acc, 0, 0, 0);
          acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[tj][kk], go[ti][kk], acc2, 0, 0, 0);
        }
        s[tj] = acc;
        dp[tj] = acc2;
      }
      const int ci = tok_code[wave][ti * 32 + l31];
      float mx = -INFINITY;
#pragma unroll
      for (int tj = 0; tj < T; ++tj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = window_key(tj, r, half);
          const int cj = tok_code[wave][j];
          float val = s[tj][r] + tbl[wave][window_bias_index<4>(ci, cj, w)];
          if (token_band<4>(ci) != token_band<4>(cj)) val += -100.0f;
          if (j >= N) val = -INFINITY;
          s[tj][r] = val;
          mx = fmaxf(mx, val);
        }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
      float sum = 0.f;
#pragma unroll
      for (int tj = 0; tj < T; ++tj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = exp_hw(s[tj][r] - mx);
          s[tj][r] = p;
          sum += p;
        }
      sum += __shfl_xor(sum, 32, 64);
      const float inv_sum = 1.0f / sum;
      float dsum = 0.f;
#pragma unroll
      for (int tj = 0; tj < T; ++tj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float p = s[tj][r] * inv_sum;
          s[tj][r] = p;
          dsum += p * dp[tj][r];
        }
      dsum += __shfl_xor(dsum, 32, 64);
      if (half == 0) {
        st_m[wave][ti * 32 + l31] = mx;
        st_il[wave][ti * 32 + l31] = inv_sum;
        st_d[wave][ti * 32 + l31] = dsum;
      }
      // dS^T in place of P^T; the tile to LDS for the table gradient
#pragma unroll
      for (int tj = 0; tj < T; ++tj)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = window_key(tj, r, half);
          const float d = s[tj][r] * (dp[tj][r] - dsum);
          s[tj][r] = d;
          dsl[wave][l31 * 65 + j] = d;
        }
      // dq^T[c][i] = sum_j K[j][c] dS[i][j]
      f32x16 accq;
#pragma unroll
      for (int e = 0; e < 16; ++e) accq[e] = 0.f;
#pragma unroll
      for (int tj = 0; tj < T; ++tj) {
        float kv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int j = window_key(tj, r, half);
          float val = 0.f;
          if (j < N) {
            const int pix = tok_pix[wave][j];
            val = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias)[a.C + head * 32 + l31];
          }
          kv[r] = val;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) accq = __builtin_amdgcn_mfma_f32_32x32x2f32(kv[r], s[tj][r], accq, 0, 0, 0);
      }
      {
        const int t = ti * 32 + l31;
        const int pix = tok_pix[wave][t];
        if (live && t < N && pix >= 0) {
          float* out = a.gqkv + (size_t)pix * C3 + head * 32 + 4 * half;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4 r4;
#pragma unroll
            for (int e = 0; e < 4; ++e) r4[e] = accq[g * 4 + e] * qscale;
            *reinterpret_cast<f32x4*>(out + 8 * g) = r4;
          }
        }
      }
      __syncthreads();
      {  // table gradient of this query tile: entry e = (dy + w - 1) (2w - 1) + (dx + w - 1), (dy, dx) = (ty_i - ty_j, tx_i - tx_j)
        const int ni = N - ti * 32 < 32 ? N - ti * 32 : 32;
#pragma unroll
        for (int n = 0; n < 4; ++n) {
          const int e = lane + 64 * n;
          if (e < rel) {
            const int dy = e / w2 - (w - 1), dx = e % w2 - (w - 1);
            float acc = 0.f;
            for (int ii = 0; ii < ni; ++ii) {
              const int c = tok_code[wave][ti * 32 + ii];
              const int tyj = token_ty<4>(c) - dy, txj = token_tx<4>(c) - dx;
              if (tyj >= 0 && tyj < w && txj >= 0 && txj < w) acc += dsl[wave][ii * 65 + tyj * w + txj];
            }
            tacc[n] += acc;
          }
        }
      }
      __syncthreads();
    }
    if (live) {
#pragma unroll
      for (int n = 0; n < 4; ++n) {
        const int e = lane + 64 * n;
        if (e < rel) pt[head * rel + e] += tacc[n];
      }
    }
    // ---- pass 2: key in the lane
#pragma unroll
    for (int tj = 0; tj < T; ++tj) {
      const int tk = tj * 32 + l31;
      const int cj = tok_code[wave][tk];
      f32x16 acck, accv;
#pragma unroll
      for (int e = 0; e < 16; ++e) acck[e] = 0.f, accv[e] = 0.f;
#pragma unroll
      for (int ti = 0; ti < T; ++ti) {
        f32x16 s2, dp2;
#pragma unroll
        for (int e = 0; e < 16; ++e) s2[e] = 0.f, dp2[e] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
          s2 = __builtin_amdgcn_mfma_f32_32x32x2f32(q[ti][kk], kr[tj][kk], s2, 0, 0, 0);
          dp2 = __builtin_amdgcn_mfma_f32_32x32x2f32(go[ti][kk], vr[tj][kk], dp2, 0, 0, 0);
        }
        float gov[16], qv[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int i = window_key(ti, r, half);
          const int ci = tok_code[wave][i];
          float val = s2[r] + tbl[wave][window_bias_index<4>(ci, cj, w)];
          if (token_band<4>(ci) != token_band<4>(cj)) val += -100.0f;
          float p = exp_hw(val - st_m[wave][i]) * st_il[wave][i];
          if (tk >= N) p = 0.f;
          s2[r] = p;
          dp2[r] = p * (dp2[r] - st_d[wave][i]);
          float gval = 0.f, qval = 0.f;
          if (i < N) {
            const int pix = tok_pix[wave][i];
            qval = (pix >= 0 ? a.qkv + (size_t)pix * C3 : a.qkv_bias)[head * 32 + l31] * qscale;
            if (pix >= 0) gval = a.gout[(size_t)pix * a.C + head * 32 + l31];
          }
          gov[r] = gval;
          qv[r] = qval;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          accv = __builtin_amdgcn_mfma_f32_32x32x2f32(gov[r], s2[r], accv, 0, 0, 0);   // dV^T[c][j] += dO[i][c] P[i][j]
          acck = __builtin_amdgcn_mfma_f32_32x32x2f32(qv[r], dp2[r], acck, 0, 0, 0);   // dK^T[c][j] += Qs[i][c] dS[i][j]
        }
      }
      const int pix = tok_pix[wave][tk];
      if (live && tk < N && pix >= 0) {
        float* out = a.gqkv + (size_t)pix * C3 + a.C + head * 32 + 4 * half;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          f32x4 k4, v4;
#pragma unroll
          for (int e = 0; e < 4; ++e) k4[e] = acck[g * 4 + e], v4[e] = accv[g * 4 + e];
          *reinterpret_cast<f32x4*>(out + 8 * g) = k4;
          *reinterpret_cast<f32x4*>(out + a.C + 8 * g) = v4;
        }
      }
      if (any_pad && live) {  // (wave-uniform) the padded keys' dk, dv: fixed butterfly over the 32 lanes of each half
        const bool padded = tk < N && pix < 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          float sk = padded ? acck[r] : 0.f, sv = padded ? accv[r] : 0.f;
#pragma unroll
          for (int m = 16; m >= 1; m >>= 1) {
            sk += __shfl_xor(sk, m, 64);
            sv += __shfl_xor(sv, m, 64);
          }
          if (l31 == 0) {
            const int c = head * 32 + 8 * (r >> 2) + 4 * half + (r & 3);
            pp[c] += sk;
            pp[a.C + c] += sv;
          }
        }
      }
    }
  }
}

// gtable[r][h] and gpad[c]: the partial rows summed in row order (one thread per output element)
__global__ __launch_bounds__(256) void window_attn_bwd_final_kernel(const float* __restrict__ part, int n_rows, int part_stride, int heads, int rel, int C,
                                                                    float* __restrict__ gtable, float* __restrict__ gpad) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  const int nt = heads * rel;
  if (idx < nt) {
    float s = 0.f;
    for (int p = 0; p < n_rows; ++p) s += part[(size_t)p * part_stride + idx];
    gtable[(size_t)(idx % rel) * heads + idx / rel] = s;
  } else if (idx < nt + 3 * C) {
    const int c = idx - nt;
    float s = 0.f;
    if (c >= C)  // (a padded token's dq is zero: its output row is cropped)
      for (int p = 0; p < n_rows; ++p) s += part[(size_t)p * part_stride + nt + (c - C)];
    gpad[c] = s;
  }
}

static int wab_slices(long long nwin) { return (int)std::min<long long>(WAB_SLICES, nwin); }

int64_t window_attn_bwd_scratch_floats(int B, int H, int W, int C, int heads, int w) {
  const WindowGrid g = window_grid(B, H, W, w);
  return (int64_t)wab_slices(g.nwin) * 4 * ((int64_t)heads * g.rel + 2 * C);
}

int launch_window_attn_bwd(const WindowAttnBwdArgs& a, hipStream_t s) {
  WindowGrid g;
  const int rc = window_attn_check("window attention backward", 8, a.qkv && a.table && a.qkv_bias && a.gout && a.gqkv && a.gtable && a.gpad && a.scratch, a, &g);
  if (rc != PH_OK) return rc;
  const int slices = wab_slices(g.nwin);
  const int per = (int)((g.nwin + slices - 1) / slices);
  const int rel = g.rel;
  const int stride = a.heads * rel + 2 * a.C;
  PH_HIP_CHECK(hipMemsetAsync(a.scratch, 0, (size_t)slices * 4 * stride * sizeof(float), s));
  if (g.N <= 32)
    hipLaunchKernelGGL(window_attn_bwd_kernel<1>, dim3(slices), dim3(256), 0, s, a, per, stride);
  else
    hipLaunchKernelGGL(window_attn_bwd_kernel<2>, dim3(slices), dim3(256), 0, s, a, per, stride);
  hipLaunchKernelGGL(window_attn_bwd_final_kernel, dim3((a.heads * rel + 3 * a.C + 255) / 256), dim3(256), 0, s, a.scratch, slices * 4, stride, a.heads, rel, a.C, a.gtable,
                     a.gpad);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Patch merging: gathered channel ph * c + cc of output pixel (oy, ox) is channel cc of input pixel (2 oy + (ph & 1), 2 ox + (ph >> 1)),
// zero past an odd edge (patch_merge_ln_kernel).  One thread per float4 of the gathered tensor.
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void patch_merge_gather_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W, int c, size_t n4) {
  const int OH = (H + 1) / 2, OW = (W + 1) / 2, cq = c >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const int qd = (int)(i % (size_t)(4 * cq));
    const size_t pix = i / (size_t)(4 * cq);
    const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), b = (int)(pix / ((size_t)OW * OH));
    const int ph = qd / cq, cc = qd - ph * cq;
    const int y = 2 * oy + (ph & 1), x = 2 * ox + (ph >> 1);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (y < H && x < W) v = *reinterpret_cast<const f32x4*>(src + ((size_t)(b * H + y) * W + x) * c + cc * 4);
    *reinterpret_cast<f32x4*>(dst + i * 4) = v;
  }
}
__global__ __launch_bounds__(256) void patch_merge_scatter_kernel(const float* __restrict__ gsrc, float* __restrict__ gdst, int accumulate, int B, int H, int W, int c,
                                                                  size_t n4) {
  const int OH = (H + 1) / 2, OW = (W + 1) / 2, cq = c >> 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const int qd = (int)(i % (size_t)(4 * cq));
    const size_t pix = i / (size_t)(4 * cq);
    const int ox = (int)(pix % OW), oy = (int)((pix / OW) % OH), b = (int)(pix / ((size_t)OW * OH));
    const int ph = qd / cq, cc = qd - ph * cq;
    const int y = 2 * oy + (ph & 1), x = 2 * ox + (ph >> 1);
    if (y >= H || x >= W) continue;  // the zero padding receives nothing
    f32x4 v = *reinterpret_cast<const f32x4*>(gsrc + i * 4);
    f32x4* o = reinterpret_cast<f32x4*>(gdst + ((size_t)(b * H + y) * W + x) * c + cc * 4);
    if (accumulate) v += *o;
    *o = v;
  }
}
static inline unsigned ew_blocks(size_t n4) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n4 + 255) / 256, 256 * 64)); }

int launch_patch_merge_gather(const float* src, float* dst, int B, int H, int W, int c, hipStream_t s) {
  PH_REQUIRE(src && dst && B > 0 && H > 0 && W > 0 && c > 0 && (c & 3) == 0, "patch merge gather: bad arguments");
  const size_t n4 = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * c;  // 4C / 4 quads per output pixel
  hipLaunchKernelGGL(patch_merge_gather_kernel, dim3(ew_blocks(n4)), dim3(256), 0, s, src, dst, B, H, W, c, n4);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
int launch_patch_merge_scatter(const float* gsrc, float* gdst, int accumulate, int B, int H, int W, int c, hipStream_t s) {
  PH_REQUIRE(gsrc && gdst && B > 0 && H > 0 && W > 0 && c > 0 && (c & 3) == 0, "patch merge scatter: bad arguments");
  const size_t n4 = (size_t)B * ((H + 1) / 2) * ((W + 1) / 2) * c;
  hipLaunchKernelGGL(patch_merge_scatter_kernel, dim3(ew_blocks(n4)), dim3(256), 0, s, gsrc, gdst, accumulate, B, H, W, c, n4);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

// ---------------------------------------------------------------------------------------
// Element-wise passes (all sizes are multiples of 4 floats: padded channel counts are multiples of 16)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void grad_fanout_kernel(const float* __restrict__ gy, float* __restrict__ gx, int accumulate, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    f32x4 v = reinterpret_cast<const f32x4*>(gy)[i];
    if (accumulate) v += reinterpret_cast<const f32x4*>(gx)[i];
    reinterpret_cast<f32x4*>(gx)[i] = v;
  }
}
// dst = scale[b] * src (+ res): src may be dst
__global__ __launch_bounds__(256) void scale_samples_kernel(const float* src, const float* __restrict__ res, const float* __restrict__ scale, float* dst, size_t per4,
                                                            size_t n4) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
    const float sc = scale[i / per4];
    f32x4 v = reinterpret_cast<const f32x4*>(src)[i] * sc;
    if (res) v += reinterpret_cast<const f32x4*>(res)[i];
    reinterpret_cast<f32x4*>(dst)[i] = v;
  }
}
__global__ __launch_bounds__(256) void vec_add_kernel(float* __restrict__ dst, const float* __restrict__ src, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) dst[i] += src[i];
}

int launch_grad_fanout(const float* gy, float* gx, int accumulate, size_t n, hipStream_t s) {
  PH_REQUIRE(gy && gx && (n & 3) == 0, "gradient fan-out: bad arguments");
  hipLaunchKernelGGL(grad_fanout_kernel, dim3(ew_blocks(n / 4)), dim3(256), 0, s, gy, gx, accumulate, n / 4);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
int launch_scale_samples(const float* src, const float* scale, float* dst, size_t per_sample, int B, hipStream_t s) {
  PH_REQUIRE(src && scale && dst && B > 0 && per_sample > 0 && (per_sample & 3) == 0, "sample scaling: bad arguments");
  hipLaunchKernelGGL(scale_samples_kernel, dim3(ew_blocks(per_sample / 4 * B)), dim3(256), 0, s, src, (const float*)nullptr, scale, dst, per_sample / 4, per_sample / 4 * B);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
int launch_scale_samples_add(float* dst, const float* res, const float* scale, size_t per_sample, int B, hipStream_t s) {
  PH_REQUIRE(dst && res && scale && B > 0 && per_sample > 0 && (per_sample & 3) == 0, "sample scaling: bad arguments");
  hipLaunchKernelGGL(scale_samples_kernel, dim3(ew_blocks(per_sample / 4 * B)), dim3(256), 0, s, (const float*)dst, res, scale, dst, per_sample / 4, per_sample / 4 * B);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}
int launch_vec_add(float* dst, const float* src, int n, hipStream_t s) {
  PH_REQUIRE(dst && src && n > 0, "vector add: bad arguments");
  hipLaunchKernelGGL(vec_add_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dst, src, n);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph
