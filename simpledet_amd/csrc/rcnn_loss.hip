// The Faster / Mask R-CNN loss heads: RpnHead / FPNRpnHead.get_loss (symbol/builder.py:163-206,
// models/FPN/builder.py:156-237) and BboxHead.get_loss (symbol/builder.py:405-446) -- SoftmaxOutput, the
// smooth_l1 chain behind MakeLoss, and the four numbers the AccWithIgnore and L1 metrics compute.  fp32 only.
//   forward   one launch over the rows (per-level tensors read in place, no concat) + one workgroup that adds the
//             workgroups' partials in a fixed order into the state block {valid, correct, fg, reg_sum}
//   backward  one launch that writes every gradient; the normaliser comes from the state block
#include "../../include/simpledet_ops.h"
#include "loss_common.h"
#include "wg_common.h"

namespace sd {

constexpr int kRlT = 256;
constexpr int kRlWaves = kRlT / kWave;
constexpr int kRlMaxL = SD_MAX_FPN_LEVELS;
constexpr int kRlMaxBlocks = 1024;          // partials the finishing workgroup adds: four per thread at the most
constexpr int kRlMaxEpl = 16;               // classes per lane of the R-CNN row kernel: K <= 1024

struct RlState {           // the state block, 16 bytes
  int valid, correct, fg;
  float reg_sum;
};

// ---- partial sums ------------------------------------------------------------------------------------------
// a workgroup's four sums -> part[4 * block ..]; all threads call
__device__ __forceinline__ void rl_put_partial(int valid, int correct, int fg, float reg, int* part) {
  __shared__ int shi[kRlWaves];
  __shared__ float shf[kRlWaves];
  const int v = block_sum_i32<kRlT>(valid, shi);
  const int c = block_sum_i32<kRlT>(correct, shi);
  const int f = block_sum_i32<kRlT>(fg, shi);
  const float r = block_sum_f32<kRlT, false>(reg, shf);
  if (threadIdx.x == 0) {
    int* o = part + 4 * (long)blockIdx.x;
    o[0] = v; o[1] = c; o[2] = f; o[3] = __float_as_int(r);
  }
}

// ONE workgroup: thread t adds partials t, t + 256, ... in order, then the fixed-order workgroup sums
__global__ __launch_bounds__(kRlT) void rl_finish_kernel(const int* part, int nparts, RlState* state) {
  __shared__ int shi[kRlWaves];
  __shared__ float shf[kRlWaves];
  int v = 0, c = 0, f = 0;
  float r = 0.f;
  for (int b = threadIdx.x; b < nparts; b += kRlT) {
    const int* o = part + 4 * (long)b;
    v += o[0]; c += o[1]; f += o[2];
    r += __int_as_float(o[3]);
  }
  v = block_sum_i32<kRlT>(v, shi);
  c = block_sum_i32<kRlT>(c, shi);
  f = block_sum_i32<kRlT>(f, shi);
  r = block_sum_f32<kRlT, false>(r, shf);
  if (threadIdx.x == 0) {
    state->valid = v; state->correct = c; state->fg = f; state->reg_sum = r;
  }
}

// ---- RPN ---------------------------------------------------------------------------------------------------
struct RpnLossArgs {
  const float* cls[kRlMaxL];    // (N, 2A, HW_l); NULL table: the class half is not computed
  const float* delta[kRlMaxL];  // (N, 4A, HW_l)
  float* dcls[kRlMaxL];
  float* ddelta[kRlMaxL];
  long off[kRlMaxL + 1];        // off[l] = positions in front of level l, off[L] = HW
  int L, N, A;
  int do_cls, do_box;
  const float *label, *target, *weight;   // (N, A * HW), (N, 4A, HW) twice
  int ignore;
  float bsq, ibsq;
  float cls_gs, reg_gs;
  float* prob;                  // (N, 2, A, HW) or NULL
  float* reg_loss;              // (N, 4A, HW) or NULL
  int* part;
  const RlState* state;
};

// the level of position q of the concat: its index, first position and size
struct RlLevel { int l; long first, hw; };
__device__ __forceinline__ RlLevel rl_level(const RpnLossArgs& a, long q) {
  RlLevel r{0, 0, a.off[1]};
#pragma unroll
  for (int l = 1; l < kRlMaxL; ++l)
    if (l < a.L && q >= a.off[l]) { r.l = l; r.first = a.off[l]; r.hw = a.off[l + 1] - a.off[l]; }
  return r;
}
template <typename T>
__device__ __forceinline__ T* rl_pick(T* const (&tab)[kRlMaxL], int lv) {
  T* p = tab[0];
#pragma unroll
  for (int l = 1; l < kRlMaxL; ++l)
    if (lv == l) p = tab[l];
  return p;
}

// One thread per label: image n, anchor a, position q -- its two logits (channels a and A + a of the level) and
// the four deltas of anchor a (channels 4a .. 4a + 3).  Consecutive threads take consecutive positions.
template <bool BWD>
__global__ __launch_bounds__(kRlT) void rpn_loss_kernel(RpnLossArgs a) {
  const long HW = a.off[a.L], AHW = (long)a.A * HW, total = (long)a.N * AHW;
  int valid = 0, correct = 0, fg = 0;
  float reg = 0.f;
  float scale = 0.f;
  if (BWD && a.do_cls) scale = a.cls_gs / (float)imaxr(a.state->valid, 1);
  for (long i = (long)blockIdx.x * kRlT + threadIdx.x; i < total; i += (long)gridDim.x * kRlT) {
    const long n = i / AHW, r = i - n * AHW;
    const long an = r / HW, q = r - an * HW;
    const RlLevel lv = rl_level(a, q);
    const long p = q - lv.first;
    if (a.do_cls) {
      const float* x = rl_pick(a.cls, lv.l);
      const long i0 = (n * 2 * a.A + an) * lv.hw + p, i1 = i0 + (long)a.A * lv.hw;
      float p0, p1;
      softmax2(x[i0], x[i1], p0, p1);
      const int k = (int)a.label[i];
      const bool on = k != a.ignore;
      if (!BWD) {
        if (a.prob) {
          const long o = (n * 2 * a.A + an) * HW + q;
          a.prob[o] = p0;
          a.prob[o + AHW] = p1;
        }
        valid += on ? 1 : 0;
        correct += on && (p1 > p0 ? 1 : 0) == k ? 1 : 0;   // argmax_channel: a tie goes to class 0
        fg += on && k != 0 ? 1 : 0;
      } else {
        float* g = rl_pick(a.dcls, lv.l);
        g[i0] = on ? softmax_ce_grad(p0, k == 0, scale) : 0.f;
        g[i1] = on ? softmax_ce_grad(p1, k == 1, scale) : 0.f;
      }
    }
    if (a.do_box) {
      const float* d = rl_pick(a.delta, lv.l);
      float* g = BWD ? rl_pick(a.ddelta, lv.l) : nullptr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long ch = n * 4 * a.A + an * 4 + j;
        const long il = ch * lv.hw + p, ic = ch * HW + q;
        const float v = d[il] - a.target[ic];
        const float w = a.weight[ic];
        if (!BWD) {
          const float loss = w * smooth_l1(v, a.bsq, a.ibsq);
          if (a.reg_loss) a.reg_loss[ic] = loss;
          reg += loss;
        } else {
          g[il] = smooth_l1_grad(v, a.bsq, a.ibsq) * (w * a.reg_gs);
        }
      }
    }
  }
  if (!BWD) rl_put_partial(valid, correct, fg, reg, a.part);
}

// ---- R-CNN -------------------------------------------------------------------------------------------------
struct RcnnLossArgs {
  const float *x, *label;            // (R, K), (R,); x NULL: the class half is not computed
  const float *delta, *target, *weight;   // (R, D)
  int R, K, D;
  int do_cls, do_box;
  float bsq, ibsq;
  float cls_gs, reg_gs;
  float *prob, *reg_loss;
  float *dx, *ddelta;
  int* part;
  const RlState* state;
};

// One wave per row: lane j holds classes j, j + 64, ... (EPL of them; two for the 81 classes of COCO).  The row's
// maximum and sum are wave reductions in a fixed order; the arg-max is over p, the lowest class among equals.
template <int EPL, bool BWD>
__global__ __launch_bounds__(kRlT) void rcnn_loss_kernel(RcnnLossArgs a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  int correct = 0, fg = 0;
  float reg = 0.f;
  float scale = 0.f;
  if (BWD && a.do_cls) scale = a.cls_gs / (float)imaxr(a.state->valid, 1);
  for (int row = blockIdx.x * kRlWaves + wave; row < a.R; row += gridDim.x * kRlWaves) {
    if (a.do_cls) {
      const float* x = a.x + (long)row * a.K;
      float e[EPL];
      float m = -INFINITY;
#pragma unroll
      for (int t = 0; t < EPL; ++t) {
        const int k = lane + t * kWave;
        e[t] = k < a.K ? x[k] : -INFINITY;
        m = fmaxr(m, e[t]);
      }
      m = wave_max_f32(m);
      float s = 0.f;
#pragma unroll
      for (int t = 0; t < EPL; ++t) {
        e[t] = lane + t * kWave < a.K ? expf(e[t] - m) : 0.f;
        s += e[t];
      }
      s = wave_sum_f32(s);
      const int lab = (int)a.label[row];
      float best = -1.f;
      int best_k = 0x7fffffff;
#pragma unroll
      for (int t = 0; t < EPL; ++t) {
        const int k = lane + t * kWave;
        if (k < a.K) {
          const float p = e[t] / s;
          if (!BWD) {
            if (a.prob) a.prob[(long)row * a.K + k] = p;
            if (p > best) { best = p; best_k = k; }
          } else {
            a.dx[(long)row * a.K + k] = softmax_ce_grad(p, k == lab, scale);
          }
        }
      }
      if (!BWD) {
        const float top = wave_max_f32(best);
        // the lowest class whose p equals the row's maximum: the largest ~k
        const unsigned cand = best == top ? ~(unsigned)best_k : 0u;
        const unsigned won = wave_max_u32(cand);
        const int arg = won ? (int)~won : 0x7fffffff;   // a row of NaN has no arg-max here
        if (lane == 0) {
          correct += arg == lab ? 1 : 0;
          fg += lab != 0 ? 1 : 0;
        }
      }
    }
    if (a.do_box) {
      const long o = (long)row * a.D;
      for (int d = lane; d < a.D; d += kWave) {
        const float v = a.delta[o + d] - a.target[o + d];
        const float w = a.weight[o + d];
        if (!BWD) {
          const float loss = w * smooth_l1(v, a.bsq, a.ibsq);
          if (a.reg_loss) a.reg_loss[o + d] = loss;
          reg += loss;
        } else {
          a.ddelta[o + d] = smooth_l1_grad(v, a.bsq, a.ibsq) * (w * a.reg_gs);
        }
      }
    }
  }
  // 'batch' normalisation: every row counts, so valid = R (thread 0 of workgroup 0 carries it)
  if (!BWD) rl_put_partial(a.do_cls && blockIdx.x == 0 && threadIdx.x == 0 ? a.R : 0, correct, fg, reg, a.part);
}

static int rl_blocks(long units) { return (int)(units < kRlMaxBlocks ? (units < 1 ? 1 : units) : kRlMaxBlocks); }
static size_t rl_ws_bytes(int blocks) { return round256((size_t)blocks * 4 * sizeof(int)) + 256; }

// the 256-byte aligned partials inside the caller's workspace
static int rl_take_ws(void* workspace, size_t workspace_bytes, int blocks, int** part) {
  WsCarver c(workspace);
  *part = c.take<int>((size_t)blocks * 4 * sizeof(int));
  if (!workspace || workspace_bytes < c.need())
    return fail(SD_ERR_WORKSPACE, "loss workspace too small: %zu < %zu bytes", workspace_bytes, c.need());
  return SD_OK;
}

static int rpn_loss_table(RpnLossArgs& a, const float* const* cls_ptrs_host, const float* const* delta_ptrs_host,
                          const long* hw_host, int L, int N, int A, const float* cls_label, const float* reg_target,
                          const float* reg_weight, float ignore_label, float sigma, bool* empty) {
  SD_REQUIRE(L >= 1 && L <= kRlMaxL, "L = %d outside [1,%d]", L, kRlMaxL);
  SD_REQUIRE(N >= 0 && A >= 1, "bad N / A");
  SD_REQUIRE(hw_host, "null level sizes");
  SD_REQUIRE(sigma > 0.f, "sigma must be positive");
  SD_REQUIRE(ignore_label == (float)(int)ignore_label, "ignore_label must be an integer");
  a.do_cls = cls_ptrs_host != nullptr;
  a.do_box = delta_ptrs_host != nullptr;
  SD_REQUIRE(a.do_cls || a.do_box, "neither the class half nor the box half is given");
  long hw = 0;
  int i = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(hw_host[l] >= 0, "negative size of level %d", l);
    if (hw_host[l] == 0) continue;
    if (a.do_cls) SD_REQUIRE(cls_ptrs_host[l], "null logit pointer in level %d", l);
    if (a.do_box) SD_REQUIRE(delta_ptrs_host[l], "null delta pointer in level %d", l);
    a.cls[i] = a.do_cls ? cls_ptrs_host[l] : nullptr;
    a.delta[i] = a.do_box ? delta_ptrs_host[l] : nullptr;
    a.off[i] = hw;
    hw += hw_host[l];
    if ((double)N * 4.0 * A * (double)hw > 2147483647.0)
      return fail(SD_ERR_UNSUPPORTED, "rpn_loss: more than 2^31 - 1 elements");
    ++i;
  }
  for (int l = i; l <= kRlMaxL; ++l) a.off[l] = hw;
  a.L = i;
  a.N = N; a.A = A;
  *empty = N == 0 || hw == 0;
  if (*empty) return SD_OK;
  SD_REQUIRE(!a.do_cls || cls_label, "null pointer (cls_label)");
  SD_REQUIRE(!a.do_box || (reg_target && reg_weight), "null pointer (reg_target / reg_weight)");
  a.label = cls_label; a.target = reg_target; a.weight = reg_weight;
  a.ignore = (int)ignore_label;
  a.bsq = sigma * sigma; a.ibsq = 1.0f / a.bsq;
  return SD_OK;
}

static int rcnn_loss_args(RcnnLossArgs& a, const float* cls_logit, const float* cls_label, const float* bbox_delta,
                          const float* bbox_target, const float* bbox_weight, int R, int K, int D, float sigma) {
  SD_REQUIRE(R >= 0 && K >= 1 && D >= 0, "bad R / K / D");
  SD_REQUIRE(sigma > 0.f, "smooth_l1_scalar must be positive");
  if (K > kRlMaxEpl * kWave) return fail(SD_ERR_UNSUPPORTED, "rcnn_loss: K = %d > %d", K, kRlMaxEpl * kWave);
  if ((long)R * (K > D ? K : D) > 2147483647L) return fail(SD_ERR_UNSUPPORTED, "rcnn_loss: more than 2^31 - 1 elements");
  a.do_cls = cls_logit != nullptr;
  a.do_box = bbox_delta != nullptr && D > 0;
  SD_REQUIRE(cls_logit || bbox_delta, "neither the class half nor the box half is given");
  SD_REQUIRE(!a.do_cls || cls_label, "null pointer (cls_label)");
  SD_REQUIRE(!a.do_box || (bbox_target && bbox_weight), "null pointer (bbox_target / bbox_weight)");
  a.x = cls_logit; a.label = cls_label; a.delta = bbox_delta; a.target = bbox_target; a.weight = bbox_weight;
  a.R = R; a.K = K; a.D = D;
  a.bsq = sigma * sigma; a.ibsq = 1.0f / a.bsq;
  return SD_OK;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_rpn_loss_workspace_bytes(int N, int A, long HW) {
  if (N <= 0 || A <= 0 || HW <= 0) return 256;
  return rl_ws_bytes(rl_blocks(cdiv((long)N * A * HW, kRlT)));
}

extern "C" size_t sd_rcnn_loss_workspace_bytes(int R) {
  if (R <= 0) return 256;
  return rl_ws_bytes(rl_blocks(cdiv(R, kRlWaves)));
}

extern "C" int sd_rpn_loss_fwd(const float* const* cls_ptrs_host, const float* const* delta_ptrs_host,
                               const long* hw_host, int L, const float* cls_label, const float* reg_target,
                               const float* reg_weight, int N, int A, float ignore_label, float sigma, float* prob,
                               float* reg_loss, int32_t* state, void* workspace, size_t workspace_bytes,
                               void* stream) {
  RpnLossArgs a{};
  bool empty = false;
  if (int e = rpn_loss_table(a, cls_ptrs_host, delta_ptrs_host, hw_host, L, N, A, cls_label, reg_target, reg_weight,
                             ignore_label, sigma, &empty))
    return e;
  if (empty) return SD_OK;
  SD_REQUIRE(state, "null pointer (state)");
  a.prob = a.do_cls ? prob : nullptr;
  a.reg_loss = a.do_box ? reg_loss : nullptr;
  const int blocks = rl_blocks(cdiv((long)N * A * a.off[a.L], kRlT));
  if (int e = rl_take_ws(workspace, workspace_bytes, blocks, &a.part)) return e;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rpn_loss_kernel<false>, dim3(blocks), dim3(kRlT), 0, st, a);
  hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(kRlT), 0, st, a.part, blocks, (RlState*)state);
  SD_LAUNCH_CHECK();
  note_dispatch("rpn_loss_kernel<fwd> grid=%d L=%d + rl_finish_kernel", blocks, a.L);
  return SD_OK;
}

extern "C" int sd_rpn_loss_bwd(const float* const* cls_ptrs_host, const float* const* delta_ptrs_host,
                               const long* hw_host, int L, const float* cls_label, const float* reg_target,
                               const float* reg_weight, int N, int A, float ignore_label, float sigma,
                               float cls_grad_scale, float reg_grad_scale, const int32_t* state,
                               float* const* dcls_ptrs_host, float* const* ddelta_ptrs_host, void* stream) {
  RpnLossArgs a{};
  bool empty = false;
  // a half is computed when its gradient table is given
  if (int e = rpn_loss_table(a, dcls_ptrs_host ? cls_ptrs_host : nullptr, ddelta_ptrs_host ? delta_ptrs_host : nullptr,
                             hw_host, L, N, A, cls_label, reg_target, reg_weight, ignore_label, sigma, &empty))
    return e;
  if (empty) return SD_OK;
  SD_REQUIRE(!a.do_cls || state, "null pointer (state)");
  int i = 0;
  for (int l = 0; l < L; ++l) {
    if (hw_host[l] == 0) continue;
    if (a.do_cls) SD_REQUIRE(dcls_ptrs_host[l], "null gradient pointer in level %d", l);
    if (a.do_box) SD_REQUIRE(ddelta_ptrs_host[l], "null gradient pointer in level %d", l);
    a.dcls[i] = a.do_cls ? dcls_ptrs_host[l] : nullptr;
    a.ddelta[i] = a.do_box ? ddelta_ptrs_host[l] : nullptr;
    ++i;
  }
  a.cls_gs = cls_grad_scale; a.reg_gs = reg_grad_scale;
  a.state = (const RlState*)state;
  const int blocks = rl_blocks(cdiv((long)N * A * a.off[a.L], kRlT));
  hipLaunchKernelGGL(rpn_loss_kernel<true>, dim3(blocks), dim3(kRlT), 0, (hipStream_t)stream, a);
  SD_LAUNCH_CHECK();
  note_dispatch("rpn_loss_kernel<bwd> grid=%d L=%d", blocks, a.L);
  return SD_OK;
}

extern "C" int sd_rcnn_loss_fwd(const float* cls_logit, const float* cls_label, const float* bbox_delta,
                                const float* bbox_target, const float* bbox_weight, int R, int K, int D, float sigma,
                                float* prob, float* reg_loss, int32_t* state, void* workspace,
                                size_t workspace_bytes, void* stream) {
  RcnnLossArgs a{};
  if (int e = rcnn_loss_args(a, cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight, R, K, D, sigma)) return e;
  if (R == 0) return SD_OK;
  SD_REQUIRE(state, "null pointer (state)");
  a.prob = a.do_cls ? prob : nullptr;
  a.reg_loss = a.do_box ? reg_loss : nullptr;
  const int blocks = rl_blocks(cdiv(R, kRlWaves));
  if (int e = rl_take_ws(workspace, workspace_bytes, blocks, &a.part)) return e;
  hipStream_t st = (hipStream_t)stream;
  if (K <= 2 * kWave)
    hipLaunchKernelGGL((rcnn_loss_kernel<2, false>), dim3(blocks), dim3(kRlT), 0, st, a);
  else
    hipLaunchKernelGGL((rcnn_loss_kernel<kRlMaxEpl, false>), dim3(blocks), dim3(kRlT), 0, st, a);
  hipLaunchKernelGGL(rl_finish_kernel, dim3(1), dim3(kRlT), 0, st, a.part, blocks, (RlState*)state);
  SD_LAUNCH_CHECK();
  note_dispatch("rcnn_loss_kernel<%d,fwd> grid=%d + rl_finish_kernel", K <= 2 * kWave ? 2 : kRlMaxEpl, blocks);
  return SD_OK;
}

extern "C" int sd_rcnn_loss_bwd(const float* cls_logit, const float* cls_label, const float* bbox_delta,
                                const float* bbox_target, const float* bbox_weight, int R, int K, int D, float sigma,
                                float cls_grad_scale, float reg_grad_scale, const int32_t* state, float* d_cls_logit,
                                float* d_bbox_delta, void* stream) {
  RcnnLossArgs a{};
  // a half is computed when its gradient is asked for
  if (int e = rcnn_loss_args(a, d_cls_logit ? cls_logit : nullptr, cls_label, d_bbox_delta ? bbox_delta : nullptr,
                             bbox_target, bbox_weight, R, K, D, sigma))
    return e;
  if (R == 0) return SD_OK;
  SD_REQUIRE(!a.do_cls || state, "null pointer (state)");
  a.dx = d_cls_logit; a.ddelta = d_bbox_delta;
  a.cls_gs = cls_grad_scale; a.reg_gs = reg_grad_scale;
  a.state = (const RlState*)state;
  const int blocks = rl_blocks(cdiv(R, kRlWaves));
  hipStream_t st = (hipStream_t)stream;
  if (K <= 2 * kWave)
    hipLaunchKernelGGL((rcnn_loss_kernel<2, true>), dim3(blocks), dim3(kRlT), 0, st, a);
  else
    hipLaunchKernelGGL((rcnn_loss_kernel<kRlMaxEpl, true>), dim3(blocks), dim3(kRlT), 0, st, a);
  SD_LAUNCH_CHECK();
  note_dispatch("rcnn_loss_kernel<%d,bwd> grid=%d", K <= 2 * kWave ? 2 : kRlMaxEpl, blocks);
  return SD_OK;
}
