// _contrib_SigmoidCrossEntropy (the Mask R-CNN mask loss) and a fused class-gather mask loss for gfx950, fp32.
//
// The reference (operator_cxx/contrib/sigmoid_cross_entropy.cu:44-122, -inl.h:68-119) runs an element kernel that
// materialises loss and count at full size, two mshadow row reductions and two more full-size passes for the
// division and the scale.  Its graph (models/maskrcnn/builder.py:278-313) feeds it through split / stack /
// gather_nd / concat, whose backward zero-fills and scatters a (R, K, P) gradient that is 1/K non-zero.  Here:
//
//   drop-in operator   data / label (n, k) -> out, loss_sum, count_sum (n) and, only if asked for, loss / count (n, k)
//   fused mask loss    logits (R, K, P), cls (R), target (R, P): plane (int)cls[r] of every row, flattened to ONE
//                      row of R*P elements, through the same element and reduction code; the backward writes all
//                      of d_logits once (+0.0 in the planes that are not selected)
//
// Element rules (t = target, x = logit), with the reference's promotions: its literals `-1.`, `1.` and `1. /` are
// doubles, so the expressions are evaluated partly in double and rounded to float ONCE:
//   t == -1:  loss = 0, count = 0, gradient = +0.0 -- the branch is on the target alone; the logit is not looked
//             at, NaN and inf included, and the element does not reach the row sum
//   else      loss = float( (-1.0 * x) * double(t - [x >= 0]) + double(logf(1 + expf(x - 2 * x * [x >= 0]))) )
//             g    = float( 1.0 / (1.0 + double(expf(-x))) - double(t) ),  count = 1
//   row:      count_sum = float(sum count) + 1e-5f;  out = loss_sum / count_sum
//             d = (g / count_sum) * grad_scale          -- two float roundings, as the reference's two passes
// Quirks kept: `normalization` is parsed and never used by the reference (the division always happens; it has no
// entry here); `out` is NOT multiplied by grad_scale, only the gradient is; the backward recomputes the count.
// An ignored element's gradient is written as +0.0 (the reference's 0 / count_sum * scale is -0.0 for a
// negative grad_scale: the one bit that differs).
//
// Fused op: a row whose cls is NaN, negative or >= K is treated as fully ignored -- its logits are not read, it
// is not counted and its gradient is zero.  The reference's gather_nd has undefined behaviour there (no bounds
// check on the device).
//
// Work decomposition (both ops, both directions): a row is cut into UNITS of 256 consecutive elements; a wave
// owns a unit, lane l its elements 4l .. 4l+3.  A lane adds its four losses in index order, the wave adds its
// lanes with the fixed butterfly of wave_sum_f32, and the unit's partial goes to the workspace; a second kernel
// adds a row's partials in a fixed order (lane l takes partials l, l + 64, ...; then the same butterfly).  One
// long row (the reference's only call sites: n = 1, k ~ 2e5) is thereby spread over k / 256 waves, and many
// short rows get a wave each.  No float atomics, every partial slot is written before it is read (nothing to
// clear, no memset node), no host synchronisation: two calls give equal bits and the calls capture into a graph.
// Counts are integers (exact for any k; the conversion (float)count + 1e-5f equals the reference's float sum
// of ones for every k <= 2^24).
// The 16-byte path (k % 4 == 0, or P % 4 == 0, and 16-byte aligned pointers) and the scalar path assign the
// same elements to the same lanes in the same order: equal bits.  The fused op on (R, K, P) and the drop-in
// operator on the gathered (1, R*P) row run the same units through the same functions: equal bits as well.
// The element, unit and reduction code lives in sigmoid_ce_common.h: msrcnn_head.hip runs the same functions.
#include "sigmoid_ce_common.h"

namespace sd {

// drop-in backward, second pass: the gradient of every unit
template <bool VEC>
__global__ __launch_bounds__(kCeT) void ce_bwd_units_kernel(CeRows s, CeUnits g, const float* __restrict__ count_sum,
                                                            float scale, float* __restrict__ d_data) {
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned u = blockIdx.x * kCeWaves + threadIdx.x / kWave; u < g.units; u += step) {
    unsigned row, e0, cnt;
    ce_lane_span(g, u, row, e0, cnt);
    if (!cnt) continue;
    const float cs = count_sum[row];
    const float4 t = s.template targets<VEC>(row, e0, cnt);
    const float4 x = s.template logits_at<VEC>(row, e0, cnt, t);
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (t.x != -1.0f) d.x = ce_grad(x.x, t.x, cs, scale);
    if (t.y != -1.0f) d.y = ce_grad(x.y, t.y, cs, scale);
    if (t.z != -1.0f) d.z = ce_grad(x.z, t.z, cs, scale);
    if (t.w != -1.0f) d.w = ce_grad(x.w, t.w, cs, scale);
    ce_store4<VEC>(d_data + (size_t)row * g.k + e0, cnt, d);
  }
}

}  // namespace sd

using namespace sd;

// ------------------------------------------------------------------------------------ drop-in operator --
static int ce_check_dims(long n, long k) {
  SD_REQUIRE(n >= 0 && k >= 0, "negative dimension (n=%ld k=%ld)", n, k);
  if (k > 0 && n > kCeMaxElems / k)
    return fail(SD_ERR_UNSUPPORTED, "n*k = %ld x %ld elements exceed the limit %ld", n, k, kCeMaxElems);
  return SD_OK;
}

extern "C" size_t sd_sigmoid_ce_workspace_bytes(long n, long k) { return ce_workspace_bytes(n, k); }

extern "C" int sd_sigmoid_ce_fwd(const float* data, const float* label, float* out, float* loss, float* loss_sum,
                                 float* count, float* count_sum, long n, long k, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (int e = ce_check_dims(n, k)) return e;
  if (n == 0 || k == 0) return SD_OK;
  SD_REQUIRE(data && label && out && loss_sum && count_sum, "null pointer");
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, n, k, "sigmoid_ce_fwd", &w)) return e;
  hipStream_t st = (hipStream_t)stream;
  const CeUnits g = ce_units(n, k);
  const CeRows s{data, label, (unsigned)k};
  const bool vec = k % 4 == 0 && ce_aligned16(data, label, loss, count);
  launch_fwd_units(s, g, vec, loss, count, w, st);
  launch_rows(w.lpart, w, g, n, out, loss_sum, count_sum, st);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_sigmoid_ce_bwd(const float* data, const float* label, float* d_data, float* count,
                                 float* count_sum, long n, long k, float grad_scale, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  if (int e = ce_check_dims(n, k)) return e;
  if (n == 0 || k == 0) return SD_OK;
  SD_REQUIRE(data && label && d_data && count_sum, "null pointer");
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, n, k, "sigmoid_ce_bwd", &w)) return e;
  hipStream_t st = (hipStream_t)stream;
  const CeUnits g = ce_units(n, k);
  const CeRows s{data, label, (unsigned)k};
  const bool vec = k % 4 == 0 && ce_aligned16(data, label, d_data, count);
  launch_count_units(s, g, vec, count, w, st);
  launch_rows(nullptr, w, g, n, nullptr, nullptr, count_sum, st);
  const int grid = ce_grid(g.units, kCeWaves);
  if (vec)
    hipLaunchKernelGGL(ce_bwd_units_kernel<true>, dim3(grid), dim3(kCeT), 0, st, s, g, count_sum, grad_scale, d_data);
  else
    hipLaunchKernelGGL(ce_bwd_units_kernel<false>, dim3(grid), dim3(kCeT), 0, st, s, g, count_sum, grad_scale, d_data);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// ------------------------------------------------------------------------------------ fused mask loss --
extern "C" size_t sd_mask_loss_workspace_bytes(int R, int K, long P) { return mask_workspace_bytes(R, K, P); }

extern "C" int sd_mask_loss_fwd(const float* logits, const float* cls, const float* target, float* out,
                                float* count_sum, int R, int K, long P, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (int e = mask_check_dims(R, K, P)) return e;
  if (R == 0 || K == 0 || P == 0) return SD_OK;
  SD_REQUIRE(logits && cls && target && out && count_sum, "null pointer");
  const long k = (long)R * P;
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, 1, k, "mask_loss_fwd", &w)) return e;
  hipStream_t st = (hipStream_t)stream;
  const CeUnits g = ce_units(1, k);
  const CeMask s{logits, cls, target, (unsigned)K, (unsigned)P};
  launch_fwd_units(s, g, P % 4 == 0 && ce_aligned16(logits, target), nullptr, nullptr, w, st);
  launch_rows(w.lpart, w, g, 1, out, nullptr, count_sum, st);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_mask_loss_bwd(const float* logits, const float* cls, const float* target, float* d_logits, int R,
                                int K, long P, float grad_scale, void* workspace, size_t workspace_bytes,
                                void* stream) {
  if (int e = mask_check_dims(R, K, P)) return e;
  if (R == 0 || K == 0 || P == 0) return SD_OK;
  SD_REQUIRE(logits && cls && target && d_logits, "null pointer");
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, 1, (long)R * P, "mask_loss_bwd", &w)) return e;
  launch_mask_bwd(logits, cls, target, nullptr, d_logits, R, K, P, grad_scale, w, (hipStream_t)stream);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
