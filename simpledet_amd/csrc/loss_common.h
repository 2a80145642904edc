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

}  // namespace sd
