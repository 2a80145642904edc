// Box arithmetic more than one operator file uses, each function ONE expression order so that its users give equal
// bits for equal operands.  Device only.
#pragma once
#include "common.h"

namespace sd {

// contrib.box_iou(format="corner") of one pair: no +1, extents clamped at 0, 0 where the union is <= 0 (the RepPoints
// IoU assigner and both IoU matrices of the FreeAnchor head)
__device__ __forceinline__ float box_iou_corner(const float* a, const float* g) {
  const float l = fmaxr(a[0], g[0]), t = fmaxr(a[1], g[1]), r = fminr(a[2], g[2]), b = fminr(a[3], g[3]);
  float w = r - l, h = b - t;
  w = w < 0.f ? 0.f : w;
  h = h < 0.f ? 0.f : h;
  const float i = w * h;
  const float u = ((a[2] - a[0]) * (a[3] - a[1]) + (g[2] - g[0]) * (g[3] - g[1])) - i;
  return u <= 0.f ? 0.f : i / u;
}

// operator_cxx/contrib/decodebbox.cc:60-110 for one box b and its four deltas d: means / stds, +1 widths, xywh (the
// exponential in double, as the reference's std::exp on a float promoted by its double literal) or xyxy deltas, then
// std::max(std::min(x, m), 0) against wm = im_w - 1, hm = im_h - 1
__device__ __forceinline__ float4 decode_box(const float4 b, const float4 d, const float* means, const float* stds,
                                             bool xyxy, float wm, float hm) {
  const float width = b.z - b.x + 1.0f, height = b.w - b.y + 1.0f;
  float px1, py1, px2, py2;
  if (!xyxy) {
    const float ctr_x = b.x + 0.5f * (width - 1.0f), ctr_y = b.y + 0.5f * (height - 1.0f);
    const float dx = d.x * stds[0] + means[0], dy = d.y * stds[1] + means[1];
    const float dw = d.z * stds[2] + means[2], dh = d.w * stds[3] + means[3];
    const float pred_ctr_x = dx * width + ctr_x, pred_ctr_y = dy * height + ctr_y;
    const float pred_w = (float)(exp((double)dw) * (double)width);
    const float pred_h = (float)(exp((double)dh) * (double)height);
    px1 = pred_ctr_x - 0.5f * (pred_w - 1.0f);
    py1 = pred_ctr_y - 0.5f * (pred_h - 1.0f);
    px2 = pred_ctr_x + 0.5f * (pred_w - 1.0f);
    py2 = pred_ctr_y + 0.5f * (pred_h - 1.0f);
  } else {
    px1 = b.x + (d.x * stds[0] + means[0]) * width;
    py1 = b.y + (d.y * stds[1] + means[1]) * height;
    px2 = b.z + (d.z * stds[2] + means[2]) * width;
    py2 = b.w + (d.w * stds[3] + means[3]) * height;
  }
  float4 o;
  o.x = fmaxr(fminr(px1, wm), 0.0f);
  o.y = fmaxr(fminr(py1, hm), 0.0f);
  o.z = fmaxr(fminr(px2, wm), 0.0f);
  o.w = fmaxr(fminr(py2, hm), 0.0f);
  return o;
}

}  // namespace sd
