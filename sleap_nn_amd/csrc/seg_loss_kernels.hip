// Losses of the segmentation model types for gfx950: BCE + Dice on foreground logits and masked smooth-L1 on the centre offsets,
// each with its gradient (C ABI: ph_loss_bce_dice, ph_loss_masked_smooth_l1, ph_loss_scratch_bytes; ph_model_backward calls the
// launchers for heads whose loss was chosen with ph_model_set_head_loss).
//
// Reference semantics (paths relative to talmolab/sleap-nn):
//   compute_bce_dice_loss ........ training/losses.py:64-105 (binary_cross_entropy_with_logits, mean; Dice per sample, 1 - mean)
//   compute_masked_smooth_l1 ..... training/losses.py:108-133 (smooth_l1 of mask * pred against mask * target, sum / sum(mask))
//
// Shape of launch_loss (train_kernels.hip): a partial-sum launch over fixed slices, a one-thread finalise that writes the loss
// and the few gradient coefficients, an elementwise gradient launch.  No host synchronisation, no float atomics: the partials
// are summed in slice order, so a second run is bitwise identical.  A thread sums its few elements in fp32; from the wave
// reduction on the sums are fp64 (the Dice loss 1 - mean(dice) cancels when the prediction is good, and the few hundred fp64
// additions per workgroup cost nothing beside the loads).
// Bounds: every element index is < B * C * HW by the loop limits; a slice's range is clipped to its sample / tensor.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "train_kernels.h"

namespace ph {

namespace {

constexpr int SEG_SLICES = 64;

__device__ __forceinline__ double block_sum_256_f64(double v, double* red /* >= 4 doubles */) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  if (lane == 0) red[wave] = v;
  __syncthreads();
  const double t = (red[0] + red[1]) + (red[2] + red[3]);
  __syncthreads();
  return t;
}

// sigmoid(z), 1 - sigmoid(z) and softplus(-z) = -log(sigmoid(z)) from e = exp(-|z|): no overflow, no cancellation at large |z|
struct Sig {
  float p, q, sp;  // p = sigmoid(z), q = 1 - p, sp = max(-z, 0) + log1p(exp(-|z|))
};
__device__ __forceinline__ Sig sig(float z) {
  const float e = expf(-fabsf(z));
  const float r = 1.0f / (1.0f + e);
  Sig s;
  s.p = z >= 0.f ? r : e * r;
  s.q = z >= 0.f ? e * r : r;
  s.sp = fmaxf(-z, 0.f) + log1pf(e);
  return s;
}

// grid (SEG_SLICES, B): slice sl of sample b -> partial[(b * SEG_SLICES + sl) * 4 + {bce, sum p t, sum p, sum t}]
__global__ __launch_bounds__(256) void bce_dice_partial_kernel(const float* __restrict__ z, const float* __restrict__ t, int HW, float pos_weight /* < 0: none */,
                                                               double* __restrict__ partial) {
  __shared__ double red[4];
  const int sl = blockIdx.x, b = blockIdx.y;
  const size_t per = ((size_t)HW + SEG_SLICES - 1) / SEG_SLICES;
  const size_t lo = std::min((size_t)HW, (size_t)sl * per), hi = std::min((size_t)HW, lo + per);
  const float* zb = z + (size_t)b * HW;
  const float* tb = t + (size_t)b * HW;
  const float pwm1 = pos_weight < 0.f ? 0.f : pos_weight - 1.f;
  float a_bce = 0.f, a_pt = 0.f, a_p = 0.f, a_t = 0.f;
  for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
    const float zv = zb[i], tv = tb[i];
    const Sig s = sig(zv);
    a_bce += (1.f - tv) * zv + (1.f + pwm1 * tv) * s.sp;
    a_pt += s.p * tv;
    a_p += s.p;
    a_t += tv;
  }
  double* out = partial + ((size_t)b * SEG_SLICES + sl) * 4;
  const double s0 = block_sum_256_f64((double)a_bce, red);
  const double s1 = block_sum_256_f64((double)a_pt, red);
  const double s2 = block_sum_256_f64((double)a_p, red);
  const double s3 = block_sum_256_f64((double)a_t, red);
  if (threadIdx.x == 0) {
    out[0] = s0;
    out[1] = s1;
    out[2] = s2;
    out[3] = s3;
  }
}

// One thread.  coeff[0] = loss_weight * bce_weight / N; per sample b, with U = sum p + sum t + smooth and D = 2 sum p t + smooth:
// coeff[1 + 2b] = loss_weight * dice_weight / B * 2 / U, coeff[2 + 2b] = loss_weight * dice_weight / B * D / U^2, so that
// d loss / d p_i = -(coeff[1 + 2b] t_i - coeff[2 + 2b]).
__global__ void bce_dice_final_kernel(const double* __restrict__ partial, int B, int HW, float bce_weight, float dice_weight, float smooth, float loss_weight,
                                      float* __restrict__ coeff, float* __restrict__ loss_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double bce = 0.0, dice = 0.0;
  for (int b = 0; b < B; ++b) {
    double pt = 0.0, p = 0.0, t = 0.0;
    for (int k = 0; k < SEG_SLICES; ++k) {
      const double* q = partial + ((size_t)b * SEG_SLICES + k) * 4;
      bce += q[0];
      pt += q[1];
      p += q[2];
      t += q[3];
    }
    const double U = p + t + (double)smooth, D = 2.0 * pt + (double)smooth;
    dice += D / U;
    const double k = (double)loss_weight * (double)dice_weight / (double)B;
    coeff[1 + 2 * b] = (float)(k * 2.0 / U);
    coeff[2 + 2 * b] = (float)(k * D / (U * U));
  }
  const double n = (double)B * (double)HW;
  coeff[0] = (float)((double)loss_weight * (double)bce_weight / n);
  loss_out[0] = (float)((double)bce_weight * (bce / n) + (double)dice_weight * (1.0 - dice / (double)B));
}

__global__ __launch_bounds__(256) void bce_dice_grad_kernel(const float* __restrict__ z, const float* __restrict__ t, const float* __restrict__ coeff, int HW, size_t n,
                                                            float pos_weight, float* __restrict__ dz) {
  const float kb = coeff[0];
  const float pwm1 = pos_weight < 0.f ? 0.f : pos_weight - 1.f;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const size_t b = i / HW;
    const float tv = t[i];
    const Sig s = sig(z[i]);
    const float g_bce = (1.f - tv) - (1.f + pwm1 * tv) * s.q;
    const float g_dice = -(coeff[1 + 2 * b] * tv - coeff[2 + 2 * b]) * (s.p * s.q);
    dz[i] = kb * g_bce + g_dice;
  }
}

// Element e of the (B, C, HW) prediction; the target and the mask may be planes of a wider tensor (batch strides in floats).
__device__ __forceinline__ void sl1_operands(const float* __restrict__ pred, const float* __restrict__ tgt, int64_t tgt_bs, const float* __restrict__ mask, int64_t mask_bs,
                                             int C, int HW, size_t e, float& d, float& m) {
  const size_t b = e / ((size_t)C * HW), r = e - b * (size_t)C * HW;
  const size_t hw = r % HW;
  m = mask[b * mask_bs + hw];
  d = m * pred[e] - m * tgt[b * tgt_bs + r];
}

// grid (SEG_SLICES): partial[2 sl + {sum of smooth-L1 terms, sum of the broadcast mask}]
__global__ __launch_bounds__(256) void sl1_partial_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int64_t tgt_bs, const float* __restrict__ mask,
                                                          int64_t mask_bs, int C, int HW, size_t n, double* __restrict__ partial) {
  __shared__ double red[4];
  const int sl = blockIdx.x;
  const size_t per = (n + SEG_SLICES - 1) / SEG_SLICES;
  const size_t lo = std::min(n, (size_t)sl * per), hi = std::min(n, lo + per);
  float a_l = 0.f, a_m = 0.f;
  for (size_t e = lo + threadIdx.x; e < hi; e += 256) {
    float d, m;
    sl1_operands(pred, tgt, tgt_bs, mask, mask_bs, C, HW, e, d, m);
    const float ad = fabsf(d);
    a_l += ad < 1.f ? 0.5f * d * d : ad - 0.5f;
    a_m += m;
  }
  const double s0 = block_sum_256_f64((double)a_l, red);
  const double s1 = block_sum_256_f64((double)a_m, red);
  if (threadIdx.x == 0) {
    partial[2 * sl] = s0;
    partial[2 * sl + 1] = s1;
  }
}

// One thread: n_valid = sum of the broadcast mask; none -> loss exactly 0 and coefficient 0 (no division).
__global__ void sl1_final_kernel(const double* __restrict__ partial, float loss_weight, float* __restrict__ coeff, float* __restrict__ loss_out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double l = 0.0, nv = 0.0;
  for (int k = 0; k < SEG_SLICES; ++k) {
    l += partial[2 * k];
    nv += partial[2 * k + 1];
  }
  if (nv == 0.0) {
    coeff[0] = 0.f;
    loss_out[0] = 0.f;
  } else {
    coeff[0] = (float)((double)loss_weight / nv);
    loss_out[0] = (float)(l / nv);
  }
}

__global__ __launch_bounds__(256) void sl1_grad_kernel(const float* __restrict__ pred, const float* __restrict__ tgt, int64_t tgt_bs, const float* __restrict__ mask,
                                                       int64_t mask_bs, const float* __restrict__ coeff, int C, int HW, size_t n, float* __restrict__ dy) {
  const float k = coeff[0];
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (size_t)gridDim.x * 256) {
    float g = 0.f;
    if (k != 0.f) {  // kernel-uniform; no valid pixel: zeros whatever the operands hold
      float d, m;
      sl1_operands(pred, tgt, tgt_bs, mask, mask_bs, C, HW, e, d, m);
      g = k * m * fminf(fmaxf(d, -1.f), 1.f);  // d/dd of smooth-L1 (beta 1): d inside (-1, 1), sign(d) outside, +-1 at the joint
    }
    dy[e] = g;
  }
}

unsigned grad_blocks(size_t n) { return (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 16384)); }

}  // namespace

int64_t seg_loss_scratch_floats(int B, int C) {
  (void)C;
  const int64_t bce = (int64_t)B * SEG_SLICES * 4 * 2 + 2 + 2 * (int64_t)B;  // fp64 partials (two floats each), then the coefficients
  const int64_t sl1 = (int64_t)SEG_SLICES * 2 * 2 + 2;
  return std::max(bce, sl1);
}

int launch_bce_dice(const float* logits, const float* tgt, int B, int H, int W, float bce_weight, float dice_weight, float smooth, float pos_weight, float loss_weight,
                    float* scratch, float* dz, float* loss_out, hipStream_t s) {
  PH_REQUIRE(B > 0 && H > 0 && W > 0 && (int64_t)H * W < (int64_t)1 << 31, "bce_dice: bad shape (%d, 1, %d, %d)", B, H, W);
  PH_REQUIRE(B <= 65535, "bce_dice: more than 65535 samples");
  PH_REQUIRE(((uintptr_t)scratch & 7) == 0, "bce_dice: scratch must be 8-byte aligned");
  double* partial = reinterpret_cast<double*>(scratch);
  float* coeff = scratch + (size_t)B * SEG_SLICES * 4 * 2;
  const int HW = H * W;
  const size_t n = (size_t)B * HW;
  hipLaunchKernelGGL(bce_dice_partial_kernel, dim3(SEG_SLICES, B), dim3(256), 0, s, logits, tgt, HW, pos_weight, partial);
  hipLaunchKernelGGL(bce_dice_final_kernel, dim3(1), dim3(1), 0, s, partial, B, HW, bce_weight, dice_weight, smooth, loss_weight, coeff, loss_out);
  hipLaunchKernelGGL(bce_dice_grad_kernel, dim3(grad_blocks(n)), dim3(256), 0, s, logits, tgt, coeff, HW, n, pos_weight, dz);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

int launch_masked_smooth_l1(const float* pred, const float* tgt, int64_t tgt_batch_stride, const float* mask, int64_t mask_batch_stride, int B, int C, int H, int W,
                            float loss_weight, float* scratch, float* dy, float* loss_out, hipStream_t s) {
  PH_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (int64_t)H * W < (int64_t)1 << 31, "masked_smooth_l1: bad shape (%d, %d, %d, %d)", B, C, H, W);
  PH_REQUIRE(tgt_batch_stride >= (int64_t)C * H * W && mask_batch_stride >= (int64_t)H * W, "masked_smooth_l1: batch strides smaller than a sample");
  PH_REQUIRE(((uintptr_t)scratch & 7) == 0, "masked_smooth_l1: scratch must be 8-byte aligned");
  double* partial = reinterpret_cast<double*>(scratch);
  float* coeff = scratch + (size_t)SEG_SLICES * 2 * 2;
  const int HW = H * W;
  const size_t n = (size_t)B * C * HW;
  hipLaunchKernelGGL(sl1_partial_kernel, dim3(SEG_SLICES), dim3(256), 0, s, pred, tgt, tgt_batch_stride, mask, mask_batch_stride, C, HW, n, partial);
  hipLaunchKernelGGL(sl1_final_kernel, dim3(1), dim3(1), 0, s, partial, loss_weight, coeff, loss_out);
  hipLaunchKernelGGL(sl1_grad_kernel, dim3(grad_blocks(n)), dim3(256), 0, s, pred, tgt, tgt_batch_stride, mask, mask_batch_stride, coeff, C, HW, n, dy);
  PH_HIP_CHECK(hipGetLastError());
  return PH_OK;
}

}  // namespace ph

using namespace ph;

extern "C" {

int64_t ph_loss_scratch_bytes(int32_t B, int32_t C) {
  if (B <= 0 || C <= 0) {
    set_error("ph_loss_scratch_bytes: bad arguments");
    return PH_E_INVALID;
  }
  return align_up(seg_loss_scratch_floats(B, C) * 4, 256);
}

int ph_loss_bce_dice(const float* logits_dev, const float* target_dev, int32_t B, int32_t h, int32_t w, float bce_weight, float dice_weight, float smooth, float pos_weight,
                     float loss_weight, float* loss_dev, float* grad_dev, void* scratch_dev, int64_t scratch_bytes, void* stream) {
  PH_REQUIRE(logits_dev && target_dev && loss_dev && grad_dev && scratch_dev, "ph_loss_bce_dice: null argument");
  PH_REQUIRE(B > 0 && scratch_bytes >= seg_loss_scratch_floats(B, 1) * 4, "ph_loss_bce_dice: scratch too small (ph_loss_scratch_bytes)");
  return launch_bce_dice(logits_dev, target_dev, B, h, w, bce_weight, dice_weight, smooth, pos_weight, loss_weight, static_cast<float*>(scratch_dev), grad_dev, loss_dev,
                         static_cast<hipStream_t>(stream));
}

int ph_loss_masked_smooth_l1(const float* pred_dev, const float* target_dev, const float* mask_dev, int32_t B, int32_t C, int32_t h, int32_t w, float loss_weight,
                             float* loss_dev, float* grad_dev, void* scratch_dev, int64_t scratch_bytes, void* stream) {
  PH_REQUIRE(pred_dev && target_dev && mask_dev && loss_dev && grad_dev && scratch_dev, "ph_loss_masked_smooth_l1: null argument");
  PH_REQUIRE(B > 0 && C > 0 && scratch_bytes >= seg_loss_scratch_floats(B, C) * 4, "ph_loss_masked_smooth_l1: scratch too small (ph_loss_scratch_bytes)");
  return launch_masked_smooth_l1(pred_dev, target_dev, (int64_t)C * h * w, mask_dev, (int64_t)h * w, B, C, h, w, loss_weight, static_cast<float*>(scratch_dev), grad_dev,
                                 loss_dev, static_cast<hipStream_t>(stream));
}

}  // extern "C"
