// Shared by the FCOS kernels (fcos_head.hip: the training losses; fcos_decode.hip: the test-time decode).
#pragma once
#include "common.h"

namespace sd {

// mx.sym.sigmoid as both FCOS graphs use it: ONE expression, so that the losses, the fused decode
// (input_logits = 1) and sd_fcos_sigmoid give the same bits for the same logit.
__device__ __forceinline__ float fcos_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

}  // namespace sd
