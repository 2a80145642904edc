// FCOS training head for gfx950, fp32: target assignment and the three losses.
//
// The reference builds its targets (models/FCOS/input.py:180-263, make_fcos_gt) from ~60 symbol nodes that
// materialise (N, 4, M, HW) and (N, 1, M, HW) tensors about twenty times, and its losses
// (models/FCOS/loss.py:86-196) from ~25 element-wise nodes run twice behind five reshapes and a concat per
// tensor (models/FCOS/builder.py:207-214).  Everything is a function of one location and the M boxes of its
// image, or of one logit and the target of its location, so here it is
//
//   fcos_target_kernel   one location per thread, the image's gt rows staged in LDS in chunks of 128 and
//                        broadcast-read, a running first-minimum over the boxes; writes centerness (N, HW),
//                        offset (N, 4, HW), cls_id (N, HW) int32 (-1 ignored, 0 background, 1..K class) and,
//                        on request, the reference's dense one-hot (N, K*HW); every store is coalesced along
//                        the plane.  Per-workgroup partials of the three normalisers go to the workspace.
//   fcos_state_kernel    one workgroup sums the partials in a fixed order into the state block:
//                        int[0] = #(foreground, not ignored) = the reference's sum(labels * mask),
//                        int[1] = #(centerness != ignore_label and > 0), float[2] = sum(centerness * iou mask).
//                        All three depend on the targets alone, so the losses never reduce them again.
//   fcos_loss_fwd_kernel + fcos_loss_final_kernel
//                        partial sums over a CANONICAL index space (the concatenated (N, K*HW) order), whatever
//                        the number of levels: L = 5 and L = 1 reduce in the same order and give equal bits.
//   fcos_loss_bwd_kernel ONE launch for the three gradients of all levels, written in the logits' own
//                        per-level layout.  The class gradient is streamed in 16-byte items that start at the
//                        gradient row's first 16-byte boundary; rows whose logits sit on another phase are
//                        loaded by 4-byte accesses, and the ragged ends of a row take the scalar path through
//                        the same element function: any 4-byte aligned pointer gives the same bits.
//
// No float atomics, no memset node, no host read: every call is graph-capturable and repeatable bit for bit.
// The arithmetic is the reference's float32 order (the library is built with -ffp-contract=off and correctly
// rounded divide / sqrt).  Where the reference multiplies by a 0/1 mask and adds, the per-box loop selects
// (equal bits for finite boxes); the two places where a NaN target can meet a zero mask -- the final centerness
// and the forward sums -- keep the multiplication, so a degenerate box's NaN goes where the reference's goes.
#include "loss_common.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {

constexpr int kFcT = 256;
constexpr int kFcWaves = kFcT / kWave;
constexpr int kFcMaxL = SD_MAX_FPN_LEVELS;
constexpr int kFcChunk = 128;                  // gt rows per LDS chunk
constexpr int kFcMaxBlocks = kNumCU * 8;
constexpr int kFcMaxImages = 65535;            // gridDim.y of the target kernel
constexpr long kFcMaxElems = 2147483647L;      // element indices are 32-bit inside the kernels

struct FcosGrid {   // PreMakeFCOSgt (input.py:14-79)
  int L, HW;
  int stride[kFcMaxL], gw[kFcMaxL], gh[kFcMaxL], begin[kFcMaxL + 1];
  float lower[kFcMaxL], upper[kFcMaxL];
};

struct FcosTargetArgs {
  const float* gt;
  const float* im_info;
  float* centerness;
  float* offset;
  int* cls_id;
  float* cls_dense;   // null: not wanted
  int* part_i;        // [blocks][2]
  float* part_f;      // [blocks]
  int N, M, K;
  float ignore_offset, ignore_label;
  FcosGrid g;
};

// mxnet_op one_hot: j = static_cast<int>(cls - 1); a class only for 0 <= j < K
__device__ __forceinline__ int fcos_class(float cls, int K) {
  const float l = cls - 1.0f;
  const int j = l >= -2147483648.0f && l < 2147483648.0f ? (int)l : -1;
  return j >= 0 && j < K ? j + 1 : 0;
}

__global__ __launch_bounds__(kFcT) void fcos_target_kernel(FcosTargetArgs a) {
  __shared__ float sgt[kFcChunk * 5];
  __shared__ float shf[kFcWaves];
  __shared__ int shi[kFcWaves];
  const int n = blockIdx.y;
  const int j = blockIdx.x * kFcT + threadIdx.x;
  const bool live = j < a.g.HW;
  const float ori_h = a.im_info[0], ori_w = a.im_info[1];   // image 0 decides for the batch (input.py:61-73)
  const float io = a.ignore_offset, il = a.ignore_label;
  float x = 0.f, y = 0.f, lo = 0.f, up = 0.f;
  if (live) {
    int l = 0;
    while (l + 1 < a.g.L && j >= a.g.begin[l + 1]) ++l;
    const int p = j - a.g.begin[l], s = a.g.stride[l];
    const float half = (float)s * 0.5f;
    if (ori_h < ori_w) {   // loc_x / loc_y: the meshgrid row-major
      x = (float)((p % a.g.gw[l]) * s) + half;
      y = (float)((p / a.g.gw[l]) * s) + half;
    } else {               // loc_x_T / loc_y_T: y.T and x.T flattened
      x = (float)((p % a.g.gh[l]) * s) + half;
      y = (float)((p / a.g.gh[l]) * s) + half;
    }
    lo = a.g.lower[l];
    up = a.g.upper[l];
  }
  float bsz = 0.f, b0 = io, b1 = io, b2 = io, b3 = io, bcls = 0.f;
  bool have = false;
  for (int m0 = 0; m0 < a.M; m0 += kFcChunk) {
    const int mc = iminr(kFcChunk, a.M - m0);
    __syncthreads();
    const float* src = a.gt + ((long)n * a.M + m0) * 5;
    for (int i = threadIdx.x; i < mc * 5; i += kFcT) sgt[i] = src[i];
    __syncthreads();
    if (live) {
      for (int m = 0; m < mc; ++m) {
        const float x1 = sgt[m * 5], y1 = sgt[m * 5 + 1], x2 = sgt[m * 5 + 2], y2 = sgt[m * 5 + 3];
        float o0 = x - x1, o1 = y - y1, o2 = x2 - x, o3 = y2 - y;
        const bool inb = fminr(fminr(o0, o1), fminr(o2, o3)) >= 0.f;
        if (!inb) o0 = o1 = o2 = o3 = io;
        const float great = fmaxr(fmaxr(o0, o1), fmaxr(o2, o3));   // after the in-box masking (input.py:197)
        const bool st = great >= lo && great < up;
        if (!st) o0 = o1 = o2 = o3 = io;
        const float sz = st ? (o0 + o2) * (o1 + o3) : 1e10f;
        if (!have || sz < bsz) {   // argmin: the first minimum
          have = true;
          bsz = sz; b0 = o0; b1 = o1; b2 = o2; b3 = o3; bcls = sgt[m * 5 + 4];
        }
      }
    }
  }
  int fg = 0, cc = 0;
  float cm = 0.f;
  if (live) {
    const float flag = b0 != io ? 1.0f : 0.0f;
    const float lrmin = b2 < b0 ? b2 : b0, lrmax = b2 < b0 ? b0 : b2;
    const float tbmin = b3 < b1 ? b3 : b1, tbmax = b3 < b1 ? b1 : b3;
    float c = sqrtf((lrmin * tbmin) / (lrmax * tbmax)) * flag;
    const float nif = (x < ori_w && y < ori_h) ? 1.0f : 0.0f;
    c = c * nif + (1.0f - nif) * il;
    int cid = flag != 0.f ? fcos_class(bcls, a.K) : 0;
    if (nif == 0.f) cid = -1;
    const long row = (long)n * a.g.HW;
    a.centerness[row + j] = c;
    a.cls_id[row + j] = cid;
    float* o = a.offset + row * 4 + j;
    o[0] = b0;
    o[(long)a.g.HW] = b1;
    o[2L * a.g.HW] = b2;
    o[3L * a.g.HW] = b3;
    if (a.cls_dense) {
      float* d = a.cls_dense + row * a.K + j;
      for (int k = 0; k < a.K; ++k) d[(long)k * a.g.HW] = cid < 0 ? il : cid == k + 1 ? 1.0f : 0.0f;
    }
    fg = cid >= 1;
    cc = c != il && c > 0.f;
    cm = c * ((b0 != io && c > 0.f) ? 1.0f : 0.0f);   // loss.py:169-175
  }
  fg = block_sum_i32<kFcT>(fg, shi);
  cc = block_sum_i32<kFcT>(cc, shi);
  cm = block_sum_f32<kFcT>(cm, shf);
  if (threadIdx.x == 0) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    a.part_i[2 * b] = fg;
    a.part_i[2 * b + 1] = cc;
    a.part_f[b] = cm;
  }
}

__global__ __launch_bounds__(kFcT) void fcos_state_kernel(const int* __restrict__ part_i,
                                                          const float* __restrict__ part_f, int blocks,
                                                          int* __restrict__ state) {
  __shared__ float shf[kFcWaves];
  __shared__ int shi[kFcWaves];
  int fg = 0, cc = 0;
  float cm = 0.f;
  for (int b = threadIdx.x; b < blocks; b += kFcT) {
    fg += part_i[2 * b];
    cc += part_i[2 * b + 1];
    cm += part_f[b];
  }
  fg = block_sum_i32<kFcT>(fg, shi);
  cc = block_sum_i32<kFcT>(cc, shi);
  cm = block_sum_f32<kFcT>(cm, shf);
  if (threadIdx.x == 0) {
    state[0] = fg;
    state[1] = cc;
    state[2] = __float_as_int(cm);
    state[3] = 0;
  }
}

// ------------------------------------------------------------------------------------------ losses --
struct FcosLossArgs {
  const float* cls[kFcMaxL];
  const float* ctr[kFcMaxL];
  const float* off[kFcMaxL];
  float* dcls[kFcMaxL];
  float* dctr[kFcMaxL];
  float* doff[kFcMaxL];
  int hw[kFcMaxL], begin[kFcMaxL + 1];
  unsigned item_begin[kFcMaxL + 1];   // backward: the class gradient's 16-byte items, per level
  int L, N, K, HW;
  const float* centerness;
  const float* offset;
  const int* cls_id;
  const int* state;
  float* part;     // forward: [blocks][3]
  float* losses;   // forward: centerness, classification, offset
  float alpha, one_minus_alpha, gamma, ignore_offset, ignore_label;
};

__device__ __forceinline__ int fcos_level(const FcosLossArgs& a, int j) {
  int l = 0;
  while (l + 1 < a.L && j >= a.begin[l + 1]) ++l;
  return l;
}

// make_sigmoid_focal_loss (loss.py:86-106) for one unmasked element; pos = (label == 1).
// The label enters as a 0/1 factor there: the branch not taken is a product with 0 added to the other.
struct FocalTerms { float a, logp, minus_log, p; };
template <int GAMMA>
__device__ __forceinline__ FocalTerms fcos_focal_terms(const FcosLossArgs& a, float x, bool pos) {
  FocalTerms t;
  t.p = sigmoid_f32(x);
  const float ge = x >= 0.f ? 1.0f : 0.0f;
  const float minus_logits_mask = (-1.0f * x) * ge;
  const float negative_abs = x - (2.0f * x) * ge;
  t.minus_log = minus_logits_mask - logf(1.0f + expf(negative_abs));
  const float pc = t.p > 1.0f ? 1.0f : t.p < 1e-5f ? 1e-5f : t.p;
  t.logp = logf(pc);
  t.a = pos ? a.alpha * pow_gamma<GAMMA>(1.0f - t.p, a.gamma) : a.one_minus_alpha * pow_gamma<GAMMA>(t.p, a.gamma);
  return t;
}
template <int GAMMA>
__device__ __forceinline__ float fcos_focal_loss(const FcosLossArgs& a, float x, bool pos) {
  const FocalTerms t = fcos_focal_terms<GAMMA>(a, x, pos);
  return -1.0f * (pos ? t.a * t.logp : t.a * t.minus_log);
}
template <int GAMMA>
__device__ __forceinline__ float fcos_focal_grad(const FcosLossArgs& a, float x, bool pos, float norm) {
  const FocalTerms t = fcos_focal_terms<GAMMA>(a, x, pos);
  const float omp = 1.0f - t.p;
  const float inner = pos ? omp - (t.p * a.gamma) * t.logp : (t.minus_log * omp) * a.gamma - t.p;
  return (-1.0f * (t.a * inner)) / norm;
}

__device__ __forceinline__ float fcos_clip(float v, float lo, float hi) { return v > hi ? hi : v < lo ? lo : v; }

// one location of the centerness BCE (loss.py:147-151) and the IoU loss (:159-196)
struct FcosLoc {
  float x_ctr, c, t[4], x[4];
  float maskc, maski;
};
__device__ __forceinline__ FcosLoc fcos_load_loc(const FcosLossArgs& a, int n, int j) {
  FcosLoc q;
  const int l = fcos_level(a, j), p = j - a.begin[l], hw = a.hw[l];
  const long t0 = (long)n * 4 * a.HW + j;
  q.c = a.centerness[(long)n * a.HW + j];
  q.x_ctr = a.ctr[l][(long)n * hw + p];
  for (int e = 0; e < 4; ++e) {
    q.t[e] = a.offset[t0 + (long)e * a.HW];
    q.x[e] = a.off[l][((long)n * 4 + e) * hw + p];
  }
  q.maskc = (q.c != a.ignore_label && q.c > 0.f) ? 1.0f : 0.0f;
  q.maski = (q.t[0] != a.ignore_offset && q.c > 0.f) ? 1.0f : 0.0f;
  return q;
}
struct IouTerms { float wi, hi, I1, U1, pw, ph, p[4]; };
__device__ __forceinline__ IouTerms fcos_iou_terms(const FcosLoc& q) {
  IouTerms r;
  for (int e = 0; e < 4; ++e) r.p[e] = fcos_clip(q.x[e], 0.f, 1e4f) * q.maski;
  const float ta = (q.t[0] + q.t[2]) * (q.t[1] + q.t[3]);
  r.pw = r.p[0] + r.p[2];
  r.ph = r.p[1] + r.p[3];
  const float pa = r.pw * r.ph;
  r.wi = fminr(r.p[0], q.t[0]) + fminr(r.p[2], q.t[2]);
  r.hi = fminr(r.p[3], q.t[3]) + fminr(r.p[1], q.t[1]);
  const float ai = r.wi * r.hi;
  const float au = (ta + pa) - ai;
  r.I1 = ai + 1.0f;
  r.U1 = au + 1.0f;
  return r;
}

template <int GAMMA>
__global__ __launch_bounds__(kFcT) void fcos_loss_fwd_kernel(FcosLossArgs a) {
  __shared__ float sh[kFcWaves];
  const unsigned step = gridDim.x * kFcT;
  const unsigned ncls = (unsigned)a.N * a.K * a.HW, nloc = (unsigned)a.N * a.HW;
  float s_cls = 0.f, s_ctr = 0.f, s_off = 0.f;
  // the class logits in the concatenated order v = (n * K + k) * HW + j
  for (unsigned v = blockIdx.x * kFcT + threadIdx.x; v < ncls; v += step) {
    const unsigned row = v / a.HW;
    const int j = (int)(v - row * a.HW);
    const int n = (int)(row / a.K), k = (int)(row - (unsigned)n * a.K);
    const int id = a.cls_id[(long)n * a.HW + j];
    if (id >= 0) {
      const int l = fcos_level(a, j);
      const float x = a.cls[l][(long)row * a.hw[l] + (j - a.begin[l])];
      s_cls += fcos_focal_loss<GAMMA>(a, x, id == k + 1);
    }
  }
  for (unsigned i = blockIdx.x * kFcT + threadIdx.x; i < nloc; i += step) {
    const int n = (int)(i / a.HW), j = (int)(i - (unsigned)n * a.HW);
    const FcosLoc q = fcos_load_loc(a, n, j);
    const float p = sigmoid_f32(q.x_ctr);
    const float bce = (-q.c) * logf(fcos_clip(p, 1e-5f, 1.0f)) - (1.0f - q.c) * logf(fcos_clip(1.0f - p, 1e-5f, 1.0f));
    s_ctr += bce * q.maskc;
    const IouTerms r = fcos_iou_terms(q);
    s_off += (-logf(r.I1 / r.U1)) * (q.c * q.maski);
  }
  s_ctr = block_sum_f32<kFcT>(s_ctr, sh);
  s_cls = block_sum_f32<kFcT>(s_cls, sh);
  s_off = block_sum_f32<kFcT>(s_off, sh);
  if (threadIdx.x == 0) {
    a.part[3 * blockIdx.x] = s_ctr;
    a.part[3 * blockIdx.x + 1] = s_cls;
    a.part[3 * blockIdx.x + 2] = s_off;
  }
}

__global__ __launch_bounds__(kFcT) void fcos_loss_final_kernel(const float* __restrict__ part, int blocks,
                                                               const int* __restrict__ state,
                                                               float* __restrict__ losses) {
  __shared__ float sh[kFcWaves];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int b = threadIdx.x; b < blocks; b += kFcT) {
    s0 += part[3 * b];
    s1 += part[3 * b + 1];
    s2 += part[3 * b + 2];
  }
  s0 = block_sum_f32<kFcT>(s0, sh);
  s1 = block_sum_f32<kFcT>(s1, sh);
  s2 = block_sum_f32<kFcT>(s2, sh);
  if (threadIdx.x == 0) {
    losses[0] = s0 / ((float)state[1] + 1e-30f);
    losses[1] = s1 / ((float)state[0] + 1.0f);
    losses[2] = s2 / (__int_as_float(state[2]) + 1e-30f);
  }
}

template <int GAMMA>
__global__ __launch_bounds__(kFcT) void fcos_loss_bwd_kernel(FcosLossArgs a) {
  const unsigned step = gridDim.x * kFcT;
  const float norm_cls = (float)a.state[0] + 1.0f;
  const float norm_ctr = (float)a.state[1] + 1e-30f;
  const float norm_off = __int_as_float(a.state[2]) + 1e-30f;
  const unsigned nitems = a.item_begin[a.L];
  for (unsigned it = blockIdx.x * kFcT + threadIdx.x; it < nitems; it += step) {
    int l = 0;
    while (l + 1 < a.L && it >= a.item_begin[l + 1]) ++l;
    const int hw = a.hw[l];
    const unsigned Q = (unsigned)((hw + 3) / 4 + 1);
    const unsigned local = it - a.item_begin[l];
    const unsigned row = local / Q;
    const int q = (int)(local - row * Q);
    float* drow = a.dcls[l] + (long)row * hw;
    const float* xrow = a.cls[l] + (long)row * hw;
    const int n = (int)(row / a.K), k1 = (int)(row - (unsigned)n * a.K) + 1;
    const int* ids = a.cls_id + (long)n * a.HW + a.begin[l];
    const int p0 = 4 * q - (int)(((uintptr_t)drow >> 2) & 3);   // drow + p0 sits on a 16-byte boundary
    if (p0 >= 0 && p0 + 4 <= hw) {
      float4 x;
      if ((((uintptr_t)(xrow + p0)) & 15) == 0) {
        x = *reinterpret_cast<const float4*>(xrow + p0);
      } else {
        x = make_float4(xrow[p0], xrow[p0 + 1], xrow[p0 + 2], xrow[p0 + 3]);
      }
      const int i0 = ids[p0], i1 = ids[p0 + 1], i2 = ids[p0 + 2], i3 = ids[p0 + 3];
      float4 g;
      g.x = i0 >= 0 ? fcos_focal_grad<GAMMA>(a, x.x, i0 == k1, norm_cls) : 0.f;
      g.y = i1 >= 0 ? fcos_focal_grad<GAMMA>(a, x.y, i1 == k1, norm_cls) : 0.f;
      g.z = i2 >= 0 ? fcos_focal_grad<GAMMA>(a, x.z, i2 == k1, norm_cls) : 0.f;
      g.w = i3 >= 0 ? fcos_focal_grad<GAMMA>(a, x.w, i3 == k1, norm_cls) : 0.f;
      *reinterpret_cast<float4*>(drow + p0) = g;
    } else {
      for (int e = 0; e < 4; ++e) {
        const int p = p0 + e;
        if (p >= 0 && p < hw) {
          const int id = ids[p];
          drow[p] = id >= 0 ? fcos_focal_grad<GAMMA>(a, xrow[p], id == k1, norm_cls) : 0.f;
        }
      }
    }
  }
  const unsigned nloc = (unsigned)a.N * a.HW;
  for (unsigned i = blockIdx.x * kFcT + threadIdx.x; i < nloc; i += step) {
    const int n = (int)(i / a.HW), j = (int)(i - (unsigned)n * a.HW);
    const int l = fcos_level(a, j), p = j - a.begin[l], hw = a.hw[l];
    const FcosLoc q = fcos_load_loc(a, n, j);
    const float pc = sigmoid_f32(q.x_ctr);
    a.dctr[l][(long)n * hw + p] = ((pc - q.c) * q.maskc) / norm_ctr;
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    if (q.maski != 0.f) {
      const IouTerms r = fcos_iou_terms(q);
      const float cm = q.c * q.maski;
      for (int e = 0; e < 4; ++e) {
        // d(-log((I + 1) / (U + 1))) with U = target + pred - I; at pred == target the min is the prediction's
        const float side = (e & 1) ? r.wi : r.hi, other = (e & 1) ? r.pw : r.ph;
        const float d = r.p[e] <= q.t[e] ? side : 0.f;
        const float v = (other - d) / r.U1 - d / r.I1;
        const bool inside = q.x[e] >= 0.f && q.x[e] <= 1e4f;   // clip's gradient
        g[e] = inside ? (v * cm) / norm_off : 0.f;
      }
    }
    for (int e = 0; e < 4; ++e) a.doff[l][((long)n * 4 + e) * hw + p] = g[e];
  }
}

static char* align256(void* p) { return reinterpret_cast<char*>(((uintptr_t)p + 255) & ~(uintptr_t)255); }

static int fcos_grid_blocks(long items) {
  const long b = (items + kFcT - 1) / kFcT;
  return (int)(b < 1 ? 1 : b > kFcMaxBlocks ? kFcMaxBlocks : b);
}

// the level table of the losses; *HW = sum of the level sizes
static int fcos_loss_table(FcosLossArgs& a, const float* const* cls, const float* const* ctr,
                           const float* const* off, const long* hw, int L, int N, int K, bool* empty) {
  SD_REQUIRE(N >= 0 && K >= 0 && L >= 0, "negative dimension (N=%d K=%d L=%d)", N, K, L);
  if (L > kFcMaxL) return fail(SD_ERR_UNSUPPORTED, "L=%d levels exceed the limit %d", L, kFcMaxL);
  SD_REQUIRE(L == 0 || hw, "null level table");
  long total = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(hw[l] >= 0, "level %d has a negative size %ld", l, hw[l]);
    total += hw[l];
    if (total > kFcMaxElems) return fail(SD_ERR_UNSUPPORTED, "more than %ld locations", kFcMaxElems);
  }
  const long n = (long)N * (K > 4 ? K : 4) * total;
  if ((double)N * (K > 4 ? K : 4) * (double)total > (double)kFcMaxElems)
    return fail(SD_ERR_UNSUPPORTED, "N*max(K,4)*HW = %ld elements exceed the limit %ld", n, kFcMaxElems);
  *empty = N == 0 || K == 0 || total == 0;
  if (*empty) return SD_OK;
  SD_REQUIRE(cls && ctr && off, "null level table");
  a.L = 0;
  a.begin[0] = 0;
  for (int l = 0; l < L; ++l) {
    if (hw[l] == 0) continue;   // an empty level holds nothing
    SD_REQUIRE(cls[l] && ctr[l] && off[l], "null pointer in level %d", l);
    a.cls[a.L] = cls[l]; a.ctr[a.L] = ctr[l]; a.off[a.L] = off[l];
    a.hw[a.L] = (int)hw[l];
    a.begin[a.L + 1] = a.begin[a.L] + (int)hw[l];
    ++a.L;
  }
  a.N = N; a.K = K; a.HW = (int)total;
  return SD_OK;
}

template <int GAMMA>
static void launch_fwd(const FcosLossArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL(fcos_loss_fwd_kernel<GAMMA>, dim3(grid), dim3(kFcT), 0, st, a);
}
template <int GAMMA>
static void launch_bwd(const FcosLossArgs& a, int grid, hipStream_t st) {
  hipLaunchKernelGGL(fcos_loss_bwd_kernel<GAMMA>, dim3(grid), dim3(kFcT), 0, st, a);
}

}  // namespace sd

using namespace sd;

extern "C" int sd_fcos_num_locations(int data_h, int data_w, const int* strides_host, int L, long* hw_levels_host,
                                     long* hw_total_host) {
  SD_REQUIRE(data_h >= 0 && data_w >= 0 && L >= 0, "negative dimension (data_h=%d data_w=%d L=%d)", data_h, data_w, L);
  if (L > kFcMaxL) return fail(SD_ERR_UNSUPPORTED, "L=%d levels exceed the limit %d", L, kFcMaxL);
  SD_REQUIRE(hw_total_host && (L == 0 || strides_host), "null pointer");
  long total = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(strides_host[l] >= 1, "stride %d of level %d is not positive", strides_host[l], l);
    // len(range(0, w, stride)) * len(range(0, h, stride))  (input.py:99-107)
    const long hw = (long)cdiv(data_h, strides_host[l]) * cdiv(data_w, strides_host[l]);
    if (hw_levels_host) hw_levels_host[l] = hw;
    total += hw;
  }
  *hw_total_host = total;
  return SD_OK;
}

extern "C" size_t sd_fcos_target_workspace_bytes(int N, long HW) {
  if (N < 0 || HW < 0) return 0;
  const size_t blocks = (size_t)N * (size_t)((HW + kFcT - 1) / kFcT);
  return 256 + blocks * 3 * sizeof(float);
}

extern "C" int sd_fcos_target(const float* gt_bbox, const float* im_info, float* centerness, float* offset,
                              int* cls_id, float* cls_dense_or_null, int* state, int N, int M, int K, int data_h,
                              int data_w, const int* strides_host, const float* lower_host_or_null,
                              const float* upper_host_or_null, int L, float ignore_offset, float ignore_label,
                              void* workspace, size_t workspace_bytes, void* stream) {
  SD_REQUIRE(N >= 0 && M >= 0 && K >= 0 && data_h >= 0 && data_w >= 0 && L >= 0,
             "negative dimension (N=%d M=%d K=%d data_h=%d data_w=%d L=%d)", N, M, K, data_h, data_w, L);
  if (L > kFcMaxL) return fail(SD_ERR_UNSUPPORTED, "L=%d levels exceed the limit %d", L, kFcMaxL);
  SD_REQUIRE(ignore_offset == ignore_offset && ignore_label == ignore_label, "ignore_offset or ignore_label is NaN");
  // an in-box offset is >= 0 and a label is 0 or 1: the ignore values must be distinguishable from both
  SD_REQUIRE(ignore_offset < 0.f, "ignore_offset=%g must be negative", (double)ignore_offset);
  SD_REQUIRE(ignore_label < 0.f, "ignore_label=%g must be negative", (double)ignore_label);
  SD_REQUIRE((lower_host_or_null == nullptr) == (upper_host_or_null == nullptr), "one stage bound table without the other");
  SD_REQUIRE(lower_host_or_null || L <= 5, "the default stage bounds cover 5 levels, L=%d", L);
  SD_REQUIRE(L == 0 || strides_host, "null pointer");
  static const float kLower[5] = {-1e-5f, 64.f, 128.f, 256.f, 512.f}, kUpper[5] = {64.f, 128.f, 256.f, 512.f, 1e5f};
  FcosTargetArgs a{};
  long total = 0;
  a.g.L = 0;
  a.g.begin[0] = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(strides_host[l] >= 1, "stride %d of level %d is not positive", strides_host[l], l);
    const float lo = lower_host_or_null ? lower_host_or_null[l] : kLower[l];
    const float up = upper_host_or_null ? upper_host_or_null[l] : kUpper[l];
    SD_REQUIRE(lo == lo && up == up, "stage bound of level %d is NaN", l);
    const int gh = cdiv(data_h, strides_host[l]), gw = cdiv(data_w, strides_host[l]);
    const long hw = (long)gh * gw;
    total += hw;
    if (total > kFcMaxElems) return fail(SD_ERR_UNSUPPORTED, "more than %ld locations", kFcMaxElems);
    if (hw == 0) continue;
    const int i = a.g.L++;
    a.g.stride[i] = strides_host[l]; a.g.gh[i] = gh; a.g.gw[i] = gw;
    a.g.lower[i] = lo; a.g.upper[i] = up;
    a.g.begin[i + 1] = (int)total;
  }
  const double cells = (double)N * (double)total;
  if (cells * (K > 4 ? K : 4) > (double)kFcMaxElems || (double)N * M * 5 > (double)kFcMaxElems)
    return fail(SD_ERR_UNSUPPORTED, "N*max(K,4)*HW or N*M*5 elements exceed the limit %ld", kFcMaxElems);
  // N is the launch's gridDim.y, and the state kernel adds N * ceil(HW / 256) partials in one workgroup
  if (N > kFcMaxImages) return fail(SD_ERR_UNSUPPORTED, "N=%d images exceed the limit %d", N, kFcMaxImages);
  if (N == 0 || total == 0) return SD_OK;
  SD_REQUIRE(M >= 1, "M=0: the smallest-area choice needs at least one gt row per image");
  SD_REQUIRE(gt_bbox && im_info && centerness && offset && cls_id && state, "null pointer");
  const size_t need = sd_fcos_target_workspace_bytes(N, total);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "fcos_target workspace too small: %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const int bx = cdiv(total, kFcT), blocks = bx * N;
  a.gt = gt_bbox; a.im_info = im_info; a.centerness = centerness; a.offset = offset; a.cls_id = cls_id;
  a.cls_dense = cls_dense_or_null;
  a.part_i = reinterpret_cast<int*>(align256(workspace));
  a.part_f = reinterpret_cast<float*>(a.part_i + 2 * (size_t)blocks);
  a.N = N; a.M = M; a.K = K; a.ignore_offset = ignore_offset; a.ignore_label = ignore_label;
  a.g.HW = (int)total;
  hipLaunchKernelGGL(fcos_target_kernel, dim3(bx, N), dim3(kFcT), 0, st, a);
  hipLaunchKernelGGL(fcos_state_kernel, dim3(1), dim3(kFcT), 0, st, a.part_i, a.part_f, blocks, state);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" size_t sd_fcos_loss_workspace_bytes(int N, int K, long HW) {
  if (N < 0 || K < 0 || HW < 0) return 0;
  return 256 + (size_t)fcos_grid_blocks((long)N * K * HW) * 3 * sizeof(float);
}

extern "C" int sd_fcos_loss_fwd(const float* const* cls_ptrs_host, const float* const* ctr_ptrs_host,
                                const float* const* off_ptrs_host, const long* hw_host, int L,
                                const float* centerness, const float* offset, const int* cls_id, const int* state,
                                float* losses, int N, int K, double alpha, double gamma, float ignore_offset,
                                float ignore_label, void* workspace, size_t workspace_bytes, void* stream) {
  SD_REQUIRE(alpha == alpha && gamma == gamma && ignore_offset == ignore_offset && ignore_label == ignore_label,
             "alpha, gamma, ignore_offset or ignore_label is NaN");
  FcosLossArgs a{};
  bool empty = false;
  if (int e = fcos_loss_table(a, cls_ptrs_host, ctr_ptrs_host, off_ptrs_host, hw_host, L, N, K, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(centerness && offset && cls_id && state && losses, "null pointer");
  const size_t need = sd_fcos_loss_workspace_bytes(N, K, a.HW);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "fcos_loss_fwd workspace too small: %zu < %zu bytes", workspace_bytes, need);
  a.centerness = centerness; a.offset = offset; a.cls_id = cls_id; a.state = state; a.losses = losses;
  a.part = reinterpret_cast<float*>(align256(workspace));
  a.alpha = (float)alpha; a.one_minus_alpha = (float)(1.0 - alpha); a.gamma = (float)gamma;   // (1 - alpha): a Python float, rounded once
  a.ignore_offset = ignore_offset; a.ignore_label = ignore_label;
  hipStream_t st = (hipStream_t)stream;
  const int grid = fcos_grid_blocks((long)N * K * a.HW);
  if (a.gamma == 2.0f) launch_fwd<2>(a, grid, st);
  else if (a.gamma == 1.0f) launch_fwd<1>(a, grid, st);
  else if (a.gamma == 0.0f) launch_fwd<0>(a, grid, st);
  else launch_fwd<-1>(a, grid, st);
  hipLaunchKernelGGL(fcos_loss_final_kernel, dim3(1), dim3(kFcT), 0, st, a.part, grid, state, losses);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_fcos_loss_bwd(const float* const* cls_ptrs_host, const float* const* ctr_ptrs_host,
                                const float* const* off_ptrs_host, float* const* dcls_ptrs_host,
                                float* const* dctr_ptrs_host, float* const* doff_ptrs_host, const long* hw_host,
                                int L, const float* centerness, const float* offset, const int* cls_id,
                                const int* state, int N, int K, double alpha, double gamma, float ignore_offset,
                                float ignore_label, void* stream) {
  SD_REQUIRE(alpha == alpha && gamma == gamma && ignore_offset == ignore_offset && ignore_label == ignore_label,
             "alpha, gamma, ignore_offset or ignore_label is NaN");
  FcosLossArgs a{};
  bool empty = false;
  if (int e = fcos_loss_table(a, cls_ptrs_host, ctr_ptrs_host, off_ptrs_host, hw_host, L, N, K, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(centerness && offset && cls_id && state, "null pointer");
  SD_REQUIRE(dcls_ptrs_host && dctr_ptrs_host && doff_ptrs_host, "null level table");
  unsigned long items = 0;
  int i = 0;
  a.item_begin[0] = 0;
  for (int l = 0; l < L; ++l) {
    if (hw_host[l] == 0) continue;
    SD_REQUIRE(dcls_ptrs_host[l] && dctr_ptrs_host[l] && doff_ptrs_host[l], "null gradient pointer in level %d", l);
    a.dcls[i] = dcls_ptrs_host[l]; a.dctr[i] = dctr_ptrs_host[l]; a.doff[i] = doff_ptrs_host[l];
    items += (unsigned long)N * K * ((hw_host[l] + 3) / 4 + 1);
    if (items > (unsigned long)kFcMaxElems)
      return fail(SD_ERR_UNSUPPORTED, "the class gradient has more than %ld 16-byte items", kFcMaxElems);
    a.item_begin[++i] = (unsigned)items;
  }
  a.centerness = centerness; a.offset = offset; a.cls_id = cls_id; a.state = state;
  a.alpha = (float)alpha; a.one_minus_alpha = (float)(1.0 - alpha); a.gamma = (float)gamma;   // (1 - alpha): a Python float, rounded once
  a.ignore_offset = ignore_offset; a.ignore_label = ignore_label;
  hipStream_t st = (hipStream_t)stream;
  const int grid = fcos_grid_blocks((long)items);
  if (a.gamma == 2.0f) launch_bwd<2>(a, grid, st);
  else if (a.gamma == 1.0f) launch_bwd<1>(a, grid, st);
  else if (a.gamma == 0.0f) launch_bwd<0>(a, grid, st);
  else launch_bwd<-1>(a, grid, st);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
