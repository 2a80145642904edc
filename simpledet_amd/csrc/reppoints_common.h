// Shared by the RepPoints kernels (reppoints_head.hip: the training head; reppoints_decode.hip: the test-time
// decode): _points2bbox (models/RepPoints/point_ops.py:219-274) as ONE set of expressions, so that both give the
// same bits for the same points.  The point count and the distance between two points of a set are arguments: the
// training head passes compile-time constants and register arrays (step 1, fully unrolled after inlining), the
// decode reads the 2 * num_points channels of one location where they lie (step 2 * H * W) for any num_points.
#pragma once
#include "common.h"
#include <math.h>

namespace sd {

enum { kRpMinmax = 0, kRpPartial = 1, kRpMoment = 2 };

struct RpMoment { float mean, std, half; };
// mean of K, sqrt(mean((v - mean)^2)), half extent std * exp(moment_transfer) (point_ops.py:253-265); the sums
// run sequentially in point order; point k is v[k * step]
__device__ __forceinline__ RpMoment rp_moment_n(const float* v, long step, int K, float e) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) s = s + v[k * step];
  RpMoment r;
  r.mean = s / (float)K;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float d = v[k * step] - r.mean;
    q = q + d * d;
  }
  r.std = sqrtf(q / (float)K);
  r.half = r.std * e;
  return r;
}

// _points2bbox: box = [left, top, right, bottom]; e0, e1 = exp(moment_transfer) (read for the moment transform only)
__device__ __forceinline__ void rp_points2bbox_n(const float* x, const float* y, long step, int K, int transform,
                                                 float e0, float e1, float* box) {
  if (transform == kRpMoment) {
    const RpMoment mx = rp_moment_n(x, step, K, e0), my = rp_moment_n(y, step, K, e1);
    box[0] = mx.mean - mx.half; box[1] = my.mean - my.half;
    box[2] = mx.mean + mx.half; box[3] = my.mean + my.half;
  } else {
    const int Q = transform == kRpPartial ? (K < 4 ? K : 4) : K;
    float l = x[0], r = x[0], t = y[0], b = y[0];
#pragma unroll
    for (int k = 1; k < Q; ++k) {
      const float xv = x[k * step], yv = y[k * step];
      l = fminr(l, xv); r = fmaxr(r, xv);
      t = fminr(t, yv); b = fmaxr(b, yv);
    }
    box[0] = l; box[1] = t; box[2] = r; box[3] = b;
  }
}

template <int K>
__device__ __forceinline__ RpMoment rp_moment(const float* v, float e) { return rp_moment_n(v, 1, K, e); }

template <int K, int TR>
__device__ __forceinline__ void rp_points2bbox(const float* x, const float* y, float e0, float e1, float* box) {
  rp_points2bbox_n(x, y, 1, K, TR, e0, e1, box);
}

}  // namespace sd
