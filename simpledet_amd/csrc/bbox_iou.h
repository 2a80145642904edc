// bbox_overlaps_cython's IoU of one box against one query box (the RPN anchor targets and the CrowdHuman RoI
// targets share it; tests/test_rpn_target.py pins it to the reference's compiled bbox.pyx).
#pragma once
#include "common.h"

namespace sd {

// operator_py/cython/bbox.pyx:56-72 -- C float arithmetic, the integer literal 1 added as a double
__device__ __forceinline__ float rpn_iou(const float4 b, const float4 q) {
  const float box_area = (float)(((double)(q.z - q.x) + 1.0) * ((double)(q.w - q.y) + 1.0));
  float ov = 0.f;
  const float iw = (float)((double)((q.z < b.z ? q.z : b.z) - (q.x > b.x ? q.x : b.x)) + 1.0);
  if (iw > 0) {
    const float ih = (float)((double)((q.w < b.w ? q.w : b.w) - (q.y > b.y ? q.y : b.y)) + 1.0);
    if (ih > 0) {
      const float ua = (float)(((((double)(b.z - b.x) + 1.0) * ((double)(b.w - b.y) + 1.0)) +
                                (double)box_area) - (double)(iw * ih));
      ov = iw * ih / ua;
    }
  }
  return ov;
}

}  // namespace sd
