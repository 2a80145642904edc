// The Mask Scoring R-CNN training head for gfx950, fp32: the mask loss that also hands out the gathered sigmoid,
// and the MaskIoU loss with its target.
//
// The reference (models/msrcnn/builder.py) trains this model with
//   MaskFasterRcnnHead.get_loss (:383-424)  split / stack / gather_nd / concat -> Activation(sigmoid) = mask_pred_prob,
//                                           and -> reshape -> SigmoidCrossEntropy.  The gathered plane has two
//                                           consumers, so its backward adds two gradients before gather_nd's
//                                           backward zero-fills and scatters the (R, K, P) gradient.
//   MaskIoUConvHead.get_loss (:143-168)     the same gather chain on the (R, K) IoU predictions, the Python CustomOp
//                                           maskiou_compute (models/msrcnn/maskiou_compute.py:14-38: four asnumpy()
//                                           copies, numpy, two copies back -- a host synchronisation in the middle of
//                                           the step) and ~10 nodes for 0.5 * sum((t - p)^2 * w) / max(sum w, 1).
//
// Mask loss.  The forward runs the units of sigmoid_ce.hip's fused mask loss through the same functions
// (sigmoid_ce_common.h: ce_fwd_unit, ce_rows_kernel), so out and count_sum carry sd_mask_loss_fwd's bits, and in the
// same pass stores prob = 1.0f / (1.0f + expf(-x)) for every element of a row whose cls names a plane -- elements
// whose target is -1 included: the MaskIoU head reads them -- and +0.0 for the rows it does not.  The backward is
// sigmoid_ce.hip's dense one-pass kernel with one more term in the selected plane:
//     d = g_ce + d_prob * (p * (1.0f - p)),    p recomputed by the forward's expression (equal bits to reading prob)
// With d_prob == NULL the same kernel instance as sd_mask_loss_bwd runs.
//
// MaskIoU loss, per RoI r (maskiou_compute.py:20-35 with numpy's types; a wave per RoI):
//     pred = prob > 0.5f;  Ps = count(pred) (ballot + popcount);  I = sum(target where pred);  T = sum(target)
//     union = max(double(T) / double(ratio) + double(Ps) - double(I), 1.0)       numpy.maximum: a NaN propagates;
//     iou_target = float(double(max(I, 0)) / union)                               ratio 0 follows IEEE (-inf -> 1)
//     weight = cls > 0 ? 1 : 0
// I and T: lane l adds elements 4l .. 4l+3 of every 256-element chunk in index order, then the fixed butterfly --
// exact for the integer-valued targets (-1, 0, 1) of the contract whatever the order, a fixed-order float sum else.
//     c = (int)cls[r] if it names a column;  p = iou_pred[r, c];  s_r = ((iou_target - p)^2) * weight,  w_r = weight
// go to the workspace for the rows with a valid cls (0 and 0 for the others: they reach neither S nor W, and their
// iou_pred is not read); a second kernel, one wave, adds them in a fixed order:
//     S = sum s_r,  W = sum w_r,  loss = 0.5f * S / max(W, 1),  weight_sum = W
// Backward: d_iou_pred[r, c] = ((-(iou_target - p)) * weight) / max(W, 1) * grad_scale, +0.0 everywhere else; nothing
// flows to prob, target or ratio (the reference BlockGrads the CustomOp's outputs).
//
// No float atomics, every workspace slot is written before it is read, no memset node, no host synchronisation:
// repeated calls give equal bits and every call captures into a graph.
#include "sigmoid_ce_common.h"

namespace sd {

// the logit of element e of the gathered row, for the sigmoid alone (the row's cls names a plane)
__device__ __forceinline__ float msr_prob_at(const CeMask& s, unsigned e, float t, float x) {
  if (t != -1.0f) return sigmoid_f32(x);                       // counted: the loss already loaded it
  const unsigned r = e / s.P;
  const int c = mask_class(s.cls[r], s.K);                 // the row's class, looked up once
  if (c < 0) return 0.0f;                                  // a rejected row: +0.0, logits not read
  return sigmoid_f32(s.logits[((size_t)r * s.K + (unsigned)c) * s.P + (e - r * s.P)]);   // ignored by the loss, still predicted
}

// mask-loss forward: the units of the fused mask loss, and prob next to them
template <bool VEC>
__global__ __launch_bounds__(kCeT) void msr_mask_fwd_kernel(CeMask s, CeUnits g, float* __restrict__ prob,
                                                            float* __restrict__ lpart, int* __restrict__ cpart) {
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned u = blockIdx.x * kCeWaves + threadIdx.x / kWave; u < g.units; u += step) {
    unsigned e0, cnt;
    float4 t, x;
    ce_fwd_unit<CeMask, VEC>(s, g, u, nullptr, nullptr, lpart, cpart, e0, cnt, t, x);
    if (!cnt) continue;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {   // one RoI; x holds its plane whenever cls names one, whatever the targets are
      if (mask_class(s.cls[e0 / s.P], s.K) >= 0) p = make_float4(sigmoid_f32(x.x), sigmoid_f32(x.y), sigmoid_f32(x.z), sigmoid_f32(x.w));
    } else {
      p.x = msr_prob_at(s, e0, t.x, x.x);
      if (cnt > 1) p.y = msr_prob_at(s, e0 + 1, t.y, x.y);
      if (cnt > 2) p.z = msr_prob_at(s, e0 + 2, t.z, x.z);
      if (cnt > 3) p.w = msr_prob_at(s, e0 + 3, t.w, x.w);
    }
    ce_store4<VEC>(prob + e0, cnt, p);
  }
}

// numpy.maximum: a NaN in either operand is the result
__device__ __forceinline__ double np_max(double a, double b) { return a != a ? a : (b != b ? b : (a > b ? a : b)); }

// MaskIoU forward, a wave per RoI: iou_target, weight and the row's terms of S and W
template <bool VEC>
__global__ __launch_bounds__(kCeT) void maskiou_rows_kernel(const float* __restrict__ iou_pred,
                                                            const float* __restrict__ prob,
                                                            const float* __restrict__ target,
                                                            const float* __restrict__ ratio,
                                                            const float* __restrict__ cls,
                                                            float* __restrict__ iou_target, float* __restrict__ weight,
                                                            float* __restrict__ s_row, float* __restrict__ w_row,
                                                            unsigned R, unsigned K, unsigned P) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned r = blockIdx.x * kCeWaves + threadIdx.x / kWave; r < R; r += step) {
    const float* pp = prob + (size_t)r * P;
    const float* tp = target + (size_t)r * P;
    int ps = 0;
    float isum = 0.f, tsum = 0.f;
    for (unsigned c0 = 0; c0 < P; c0 += kCeUnit) {      // wave-uniform trip count: every lane reaches the ballots
      const unsigned e0 = c0 + 4u * lane;
      const unsigned cnt = e0 >= P ? 0u : (P - e0 < 4u ? P - e0 : 4u);
      float4 p = make_float4(0.f, 0.f, 0.f, 0.f), t = p;
      if (cnt) {
        p = ce_load4<VEC>(pp + e0, cnt);      // absent elements: prob 0 (not predicted), target 0
        t = ce_load4<VEC>(tp + e0, cnt);
      }
      const bool bx = p.x > 0.5f, by = p.y > 0.5f, bz = p.z > 0.5f, bw = p.w > 0.5f;
      ps += __popcll(__ballot(bx)) + __popcll(__ballot(by)) + __popcll(__ballot(bz)) + __popcll(__ballot(bw));
      isum += (((bx ? t.x : 0.f) + (by ? t.y : 0.f)) + (bz ? t.z : 0.f)) + (bw ? t.w : 0.f);
      tsum += ((t.x + t.y) + t.z) + t.w;
    }
    isum = wave_sum_f32(isum);
    tsum = wave_sum_f32(tsum);
    if (lane == 0) {
      const double uni = np_max((double)tsum / (double)ratio[r] + (double)ps - (double)isum, 1.0);
      const float imax = isum != isum ? isum : (isum > 0.f ? isum : 0.f);
      const float it = (float)((double)imax / uni);
      const float cv = cls[r];
      const float w = cv > 0.0f ? 1.0f : 0.0f;
      iou_target[r] = it;
      weight[r] = w;
      const int c = mask_class(cv, K);
      float s = 0.f, wv = 0.f;
      if (c >= 0) {
        const float d = it - iou_pred[(size_t)r * K + (unsigned)c];
        s = (d * d) * w;
        wv = w;
      }
      s_row[r] = s;
      w_row[r] = wv;
    }
  }
}

// one wave: the row terms in a fixed order (lane l takes rows l, l + 64, ...; then the butterfly)
__global__ __launch_bounds__(kWave) void maskiou_finish_kernel(const float* __restrict__ s_row,
                                                               const float* __restrict__ w_row, unsigned R,
                                                               float* __restrict__ loss, float* __restrict__ weight_sum) {
  float s = 0.f, w = 0.f;
  for (unsigned i = threadIdx.x; i < R; i += kWave) {
    s += s_row[i];
    w += w_row[i];
  }
  s = wave_sum_f32(s);
  w = wave_sum_f32(w);
  if (threadIdx.x == 0) {
    *loss = (0.5f * s) / fmaxr(w, 1.0f);
    *weight_sum = w;
  }
}

// MaskIoU backward: every element of d_iou_pred once
__global__ __launch_bounds__(kCeT) void maskiou_bwd_kernel(const float* __restrict__ iou_pred,
                                                           const float* __restrict__ cls,
                                                           const float* __restrict__ iou_target,
                                                           const float* __restrict__ weight,
                                                           const float* __restrict__ weight_sum,
                                                           float* __restrict__ d_iou_pred, unsigned R, unsigned K,
                                                           float scale) {
  const unsigned n = R * K;
  const float den = fmaxr(*weight_sum, 1.0f);
  for (unsigned i = blockIdx.x * kCeT + threadIdx.x; i < n; i += gridDim.x * kCeT) {
    const unsigned r = i / K;
    float d = 0.f;
    if (mask_class(cls[r], K) == (int)(i - r * K)) d = (((-(iou_target[r] - iou_pred[i])) * weight[r]) / den) * scale;
    d_iou_pred[i] = d;
  }
}

static int maskiou_check_dims(int R, int K, long P) {
  SD_REQUIRE(R >= 0 && K >= 0 && P >= 0, "negative dimension (R=%d K=%d P=%ld)", R, K, P);
  if ((K > 0 && R > kCeMaxElems / K) || (P > 0 && R > kCeMaxElems / P))
    return fail(SD_ERR_UNSUPPORTED, "R*K = %d x %d or R*P = %d x %ld elements exceed the limit %ld", R, K, R, P,
                kCeMaxElems);
  return SD_OK;
}

// workspace: [256-byte alignment slack][R floats: s_r][R floats: w_r]
static size_t maskiou_workspace_bytes(int R) {
  if (R <= 0) return 512;
  return 256 + (((size_t)R * 8 + 255) & ~(size_t)255);
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_msrcnn_mask_loss_workspace_bytes(int R, int K, long P) { return mask_workspace_bytes(R, K, P); }

extern "C" int sd_msrcnn_mask_loss_fwd(const float* logits, const float* cls, const float* target, float* out,
                                       float* count_sum, float* prob, int R, int K, long P, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  if (int e = mask_check_dims(R, K, P)) return e;
  if (R == 0 || K == 0 || P == 0) return SD_OK;
  SD_REQUIRE(logits && cls && target && out && count_sum && prob, "null pointer");
  const long k = (long)R * P;
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, 1, k, "msrcnn_mask_loss_fwd", &w)) return e;
  hipStream_t st = (hipStream_t)stream;
  const CeUnits g = ce_units(1, k);
  const CeMask s{logits, cls, target, (unsigned)K, (unsigned)P};
  const int grid = ce_grid(g.units, kCeWaves);
  if (P % 4 == 0 && ce_aligned16(logits, target, prob))
    hipLaunchKernelGGL(msr_mask_fwd_kernel<true>, dim3(grid), dim3(kCeT), 0, st, s, g, prob, w.lpart, w.cpart);
  else
    hipLaunchKernelGGL(msr_mask_fwd_kernel<false>, dim3(grid), dim3(kCeT), 0, st, s, g, prob, w.lpart, w.cpart);
  launch_rows(w.lpart, w, g, 1, out, nullptr, count_sum, st);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_msrcnn_mask_loss_bwd(const float* logits, const float* cls, const float* target,
                                       const float* d_prob, float* d_logits, int R, int K, long P, float grad_scale,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  if (int e = mask_check_dims(R, K, P)) return e;
  if (R == 0 || K == 0 || P == 0) return SD_OK;
  SD_REQUIRE(logits && cls && target && d_logits, "null pointer");
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, 1, (long)R * P, "msrcnn_mask_loss_bwd", &w)) return e;
  launch_mask_bwd(logits, cls, target, d_prob, d_logits, R, K, P, grad_scale, w, (hipStream_t)stream);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" size_t sd_maskiou_loss_workspace_bytes(int R, int K, long P) {
  (void)K;
  (void)P;
  return maskiou_workspace_bytes(R);
}

extern "C" int sd_maskiou_loss_fwd(const float* iou_pred, const float* prob, const float* target, const float* ratio,
                                   const float* cls, float* iou_target, float* weight, float* loss,
                                   float* weight_sum, int R, int K, long P, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  if (int e = maskiou_check_dims(R, K, P)) return e;
  if (R == 0 || K == 0 || P == 0) return SD_OK;
  SD_REQUIRE(iou_pred && prob && target && ratio && cls && iou_target && weight && loss && weight_sum, "null pointer");
  const size_t need = maskiou_workspace_bytes(R);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "maskiou_loss_fwd workspace too small: %zu < %zu bytes", workspace_bytes, need);
  float* s_row = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  float* w_row = s_row + R;
  hipStream_t st = (hipStream_t)stream;
  const int grid = ce_grid(R, kCeWaves);
  if (P % 4 == 0 && ce_aligned16(prob, target))
    hipLaunchKernelGGL(maskiou_rows_kernel<true>, dim3(grid), dim3(kCeT), 0, st, iou_pred, prob, target, ratio, cls,
                       iou_target, weight, s_row, w_row, (unsigned)R, (unsigned)K, (unsigned)P);
  else
    hipLaunchKernelGGL(maskiou_rows_kernel<false>, dim3(grid), dim3(kCeT), 0, st, iou_pred, prob, target, ratio, cls,
                       iou_target, weight, s_row, w_row, (unsigned)R, (unsigned)K, (unsigned)P);
  hipLaunchKernelGGL(maskiou_finish_kernel, dim3(1), dim3(kWave), 0, st, (const float*)s_row, (const float*)w_row,
                     (unsigned)R, loss, weight_sum);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_maskiou_loss_bwd(const float* iou_pred, const float* cls, const float* iou_target,
                                   const float* weight, const float* weight_sum, float* d_iou_pred, int R, int K,
                                   float grad_scale, void* stream) {
  if (int e = maskiou_check_dims(R, K, 0)) return e;
  if (R == 0 || K == 0) return SD_OK;
  SD_REQUIRE(iou_pred && cls && iou_target && weight && weight_sum && d_iou_pred, "null pointer");
  hipLaunchKernelGGL(maskiou_bwd_kernel, dim3(ce_grid((long)R * K, kCeT)), dim3(kCeT), 0, (hipStream_t)stream,
                     iou_pred, cls, iou_target, weight, weight_sum, d_iou_pred, (unsigned)R, (unsigned)K, grad_scale);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
