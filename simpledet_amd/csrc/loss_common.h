// Scalar arithmetic the loss kernels share: each function is ONE expression in the reference's order of
// operations, so two operators that call it give equal bits for equal operands.  Device only.
#pragma once
#include "common.h"
#include <math.h>

namespace sd {

// mshadow_op::sigmoid in fp32 -- mx.sym.sigmoid of both FCOS graphs (the losses, the fused decode with
// input_logits = 1 and sd_fcos_sigmoid), the RepPoints decode, FocalLoss's forward (focal_loss-inl.h:113) and
// Activation(act_type='sigmoid'), the Mask Scoring R-CNN mask_pred_prob
__device__ __forceinline__ float sigmoid_f32(float x) { return 1.0f / (1.0f + expf(-x)); }

// pow(r, gamma) of the focal losses (focal_loss-inl.h:192-230, models/FCOS/loss.py:86-106).  GAMMA: 0 / 1 / 2
// multiply-only, -1 powf
template <int GAMMA>
__device__ __forceinline__ float pow_gamma(float r, float gamma) {
  if (GAMMA == 2) return r * r;
  if (GAMMA == 1) return r;
  if (GAMMA == 0) return 1.0f;
  return powf(r, gamma);
}

// mshadow_op::smooth_l1_loss / smooth_l1_gradient; bsq = sigma^2, ibsq = 1 / sigma^2
__device__ __forceinline__ float smooth_l1(float v, float bsq, float ibsq) {
  if (v > ibsq) return v - 0.5f * ibsq;
  if (v < -ibsq) return -v - 0.5f * ibsq;
  return 0.5f * v * v * bsq;
}
__device__ __forceinline__ float smooth_l1_grad(float v, float bsq, float ibsq) {
  if (v > ibsq) return 1.0f;
  if (v < -ibsq) return -1.0f;
  return bsq * v;
}

// SoftmaxOutput's row of two classes (the RPN heads): m = max, e_c = expf(x_c - m), s = e_0 + e_1, p_c = e_c / s
__device__ __forceinline__ void softmax2(float x0, float x1, float& p0, float& p1) {
  const float m = fmaxr(x0, x1);
  const float e0 = expf(x0 - m), e1 = expf(x1 - m);
  const float s = e0 + e1;
  p0 = e0 / s;
  p1 = e1 / s;
}

// SoftmaxOutput's gradient of one class: (p - [the label names this class]) * (grad_scale / norm)
__device__ __forceinline__ float softmax_ce_grad(float p, bool hit, float scale) {
  return (p - (hit ? 1.0f : 0.0f)) * scale;
}

}  // namespace sd
