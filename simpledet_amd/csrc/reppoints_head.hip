// RepPoints training head for gfx950, fp32: both assigners and the two box losses.
//
// The reference builds its targets (models/RepPoints/point_ops.py:67-216) from (M, P) float matrices -- about ten
// per image for the point assigner with three top-k sorts, a (P, M) box_iou with five `where` for the IoU
// assigner -- and its box losses (models/RepPoints/builder.py:415-481) from a transpose, reshape, flip, tile and
// concat per level and stage.  Everything is a function of one point and the M gt rows of its image, so here it is
//
//   rp_init_kernel     clears the per-point selection keys (all ones) and the per-gt column maxima (0).
//   rp_point_kernel    one workgroup per (gt, image): scans only the points of the gt's own level, num_pos rounds
//                      of a 64-bit arg-min over the key (distance bits, flat point index); each selected point gets
//                      a 64-bit atomicMin of (distance bits, gt index).  Integer atomics: independent of order.
//   rp_box_kernel      one point per thread, gt rows in LDS: the init box from the 2 * num_points channels
//                      (coalesced along w, channel by channel), kept in the workspace; the M IoUs, their column
//                      maxima reduced per wave and workgroup, then one atomicMax per gt and workgroup on the IoU's
//                      bit pattern (an IoU is >= 0: unsigned order is float order).
//   rp_assign_kernel   one point per thread: the key becomes label_init / gt_init; the same IoUs again (same
//                      expression, same bits), compared with the column maxima, become label_refine / gt_refine;
//                      per-workgroup counts of label >= 1 go to the workspace.
//   rp_state_kernel    one workgroup adds the counts: state = [#init, #refine, bits(#init + 1), bits(#refine + 1)],
//                      the two BBoxNorm denominators (bbox_norm-inl.h:116-122).
//   rp_loss_fwd_kernel one point per thread, both stages: absolute points, box, residual, smooth-L1, weight.
//   rp_loss_bwd_kernel + rp_dmt_kernel
//                      the same, then the chain rule of the expressions as written into the per-level layout of the
//                      inputs; the moment_transfer gradient as per-workgroup partials summed in a fixed order.
//
// No float atomics, no memset node, no host read: every call is graph-capturable and repeatable bit for bit.  The
// arithmetic is the reference's float32 expressions one operation at a time (-ffp-contract=off, correctly rounded
// divide / sqrt); the sums over the points of a set run sequentially in point order.
#include "reppoints_common.h"
#include "loss_common.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {

constexpr int kRpT = 256;
constexpr int kRpWaves = kRpT / kWave;
constexpr int kRpMaxL = SD_MAX_FPN_LEVELS;
constexpr int kRpMaxM = 128;
constexpr int kRpMaxPos = 16;
constexpr int kRpMaxImages = 65535;            // gridDim.y
constexpr long kRpMaxElems = 2147483647L;      // element indices are 32-bit inside the kernels
constexpr unsigned kRpInfBits = 0x7f800000u;
constexpr unsigned long long kRpNoKey = ~0ull;

struct RpLevels {   // _gen_points (point_ops.py:18-30): level l holds (h, w) row-major, x = w * stride, y = h * stride
  int L, P;
  int stride[kRpMaxL], gw[kRpMaxL], hw[kRpMaxL], begin[kRpMaxL + 1];
  float lvl[kRpMaxL];   // floor(log2(stride))
};

__device__ __forceinline__ int rp_level(const RpLevels& g, int j) {
  int l = 0;
  while (l + 1 < g.L && j >= g.begin[l + 1]) ++l;
  return l;
}

// ------------------------------------------------------------------------------- points -> box --
// the 2 * K channels of one location: (y0, x0, y1, x1, ...), hw elements apart
template <int K>
__device__ __forceinline__ void rp_load(const float* base, int hw, float* y, float* x) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    y[k] = base[(long)(2 * k) * hw];
    x[k] = base[(long)(2 * k + 1) * hw];
  }
}

// rp_moment and rp_points2bbox (_points2bbox, point_ops.py:219-274): reppoints_common.h, shared with the decode

// upstream box_iou, corner format (no +1): extents clamped at 0, 0 where the union is <= 0
__device__ __forceinline__ float rp_iou(const float* a, const float* g) {
  const float l = fmaxr(a[0], g[0]), t = fmaxr(a[1], g[1]), r = fminr(a[2], g[2]), b = fminr(a[3], g[3]);
  float w = r - l, h = b - t;
  w = w < 0.f ? 0.f : w;
  h = h < 0.f ? 0.f : h;
  const float i = w * h;
  const float u = ((a[2] - a[0]) * (a[3] - a[1]) + (g[2] - g[0]) * (g[3] - g[1])) - i;
  return u <= 0.f ? 0.f : i / u;
}

// ---------------------------------------------------------------------------------------- targets --
struct RpTargetArgs {
  const float* pts[kRpMaxL];
  const float* gt;
  const float* mt;
  float* label_init;
  float* gt_init;
  float* label_refine;
  float* gt_refine;
  float* boxes;                 // workspace [N * P * 4]
  unsigned long long* keys;     // workspace [N * P]
  unsigned* colmax;             // workspace [N * M]
  int* part;                    // workspace [blocks * 2]
  int N, M, num_pos;
  float scale, pos_thr, neg_thr, min_pos, lvl_min, lvl_max;
  RpLevels g;
};

__global__ __launch_bounds__(kRpT) void rp_init_kernel(unsigned long long* keys, long nkeys, unsigned* colmax, long ncol) {
  const long step = (long)gridDim.x * kRpT;
  for (long i = (long)blockIdx.x * kRpT + threadIdx.x; i < nkeys; i += step) keys[i] = kRpNoKey;
  for (long i = (long)blockIdx.x * kRpT + threadIdx.x; i < ncol; i += step) colmax[i] = 0u;
}

__global__ __launch_bounds__(kRpT) void rp_point_kernel(RpTargetArgs a) {
  __shared__ unsigned long long sk[kRpT];
  const int m = blockIdx.x, n = blockIdx.y;
  const float* g = a.gt + ((long)n * a.M + m) * 5;
  const float l = g[0], t = g[1], r = g[2], b = g[3];
  if (!(g[4] > 0.f)) return;   // not a valid gt (padding rows are -1): the whole workgroup leaves
  const float gx = (l + r) / 2.0f, gy = (t + b) / 2.0f;
  const float gw = fmaxr(r - l, 1e-6f), gh = fmaxr(b - t, 1e-6f);
  float lvl = floorf((log2f(gw / a.scale) + log2f(gh / a.scale)) / 2.0f);
  lvl = fmaxr(fminr(lvl, a.lvl_max), a.lvl_min);
  unsigned long long last = 0ull;
  for (int round = 0; round < a.num_pos; ++round) {
    unsigned long long best = kRpNoKey;
    for (int li = 0; li < a.g.L; ++li) {
      if (a.g.lvl[li] != lvl) continue;
      const int w = a.g.gw[li], s = a.g.stride[li], b0 = a.g.begin[li];
      for (int p = threadIdx.x; p < a.g.hw[li]; p += kRpT) {
        const int ph = p / w;
        const float px = (float)((p - ph * w) * s), py = (float)(ph * s);
        const float dx = (px - gx) / gw, dy = (py - gy) / gh;
        const float d = sqrtf(dx * dx + dy * dy);
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)(b0 + p);
        if ((round == 0 || key > last) && key < best) best = key;
      }
    }
    sk[threadIdx.x] = best;
    __syncthreads();
    for (int s = kRpT / 2; s > 0; s >>= 1) {
      if (threadIdx.x < s && sk[threadIdx.x + s] < sk[threadIdx.x]) sk[threadIdx.x] = sk[threadIdx.x + s];
      __syncthreads();
    }
    const unsigned long long kmin = sk[0];
    __syncthreads();
    if (kmin == kRpNoKey) break;   // fewer points in the level than num_pos
    if (threadIdx.x == 0) {
      const unsigned j = (unsigned)(kmin & 0xffffffffull);
      atomicMin(a.keys + (long)n * a.g.P + j, (kmin & 0xffffffff00000000ull) | (unsigned)m);
    }
    last = kmin;
  }
}

template <int K, int TR>
__global__ __launch_bounds__(kRpT) void rp_box_kernel(RpTargetArgs a) {
  __shared__ float sgt[kRpMaxM * 5];
  __shared__ unsigned smax[kRpMaxM];
  const int n = blockIdx.y, j = blockIdx.x * kRpT + threadIdx.x;
  const bool live = j < a.g.P;
  for (int i = threadIdx.x; i < a.M * 5; i += kRpT) sgt[i] = a.gt[(long)n * a.M * 5 + i];
  for (int i = threadIdx.x; i < a.M; i += kRpT) smax[i] = 0u;
  __syncthreads();
  float box[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const int l = rp_level(a.g, j), p = j - a.g.begin[l], hw = a.g.hw[l], w = a.g.gw[l];
    const float s = (float)a.g.stride[l];
    const int ph = p / w;
    const float cx = (float)((p - ph * w) * a.g.stride[l]), cy = (float)(ph * a.g.stride[l]);
    float x[K], y[K], bb[4];
    rp_load<K>(a.pts[l] + (long)n * 2 * K * hw + p, hw, y, x);
    float e0 = 1.f, e1 = 1.f;
    if (TR == kRpMoment) { e0 = expf(a.mt[0]); e1 = expf(a.mt[1]); }
    // _offset_to_boxes (point_ops.py:51-64): the box of the raw offsets, THEN * stride, then + centre
    rp_points2bbox<K, TR>(x, y, e0, e1, bb);
    box[0] = cx + bb[0] * s; box[1] = cy + bb[1] * s; box[2] = cx + bb[2] * s; box[3] = cy + bb[3] * s;
    float* o = a.boxes + ((long)n * a.g.P + j) * 4;
    o[0] = box[0]; o[1] = box[1]; o[2] = box[2]; o[3] = box[3];
  }
  for (int m = 0; m < a.M; ++m) {
    const float v = rp_iou(box, sgt + m * 5);
    const unsigned wm = wave_max_u32(live ? __float_as_uint(v) : 0u);
    if ((threadIdx.x & (kWave - 1)) == 0 && wm) atomicMax(smax + m, wm);
  }
  __syncthreads();
  for (int m = threadIdx.x; m < a.M; m += kRpT)
    if (smax[m]) atomicMax(a.colmax + (long)n * a.M + m, smax[m]);
}

__global__ __launch_bounds__(kRpT) void rp_assign_kernel(RpTargetArgs a) {
  __shared__ float sgt[kRpMaxM * 5];
  __shared__ float scol[kRpMaxM];
  __shared__ int shi[kRpWaves];
  const int n = blockIdx.y, j = blockIdx.x * kRpT + threadIdx.x;
  const bool live = j < a.g.P;
  for (int i = threadIdx.x; i < a.M * 5; i += kRpT) sgt[i] = a.gt[(long)n * a.M * 5 + i];
  for (int i = threadIdx.x; i < a.M; i += kRpT) scol[i] = __uint_as_float(a.colmax[(long)n * a.M + i]);
  __syncthreads();
  int ci = 0, cr = 0;
  if (live) {
    const long i = (long)n * a.g.P + j;
    // point assigner: the gt of least surviving distance, else label -1 and a zero box (point_ops.py:130-136)
    const unsigned long long key = a.keys[i];
    float li = -1.0f, b[4] = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)(key >> 32) < kRpInfBits) {
      const float* g = sgt + (unsigned)(key & 0xffffffffull) * 5;
      li = g[4]; b[0] = g[0]; b[1] = g[1]; b[2] = g[2]; b[3] = g[3];
    }
    a.label_init[i] = li;
    float* o = a.gt_init + i * 4;
    o[0] = b[0]; o[1] = b[1]; o[2] = b[2]; o[3] = b[3];
    ci = 1.0f <= li;
    // IoU assigner (point_ops.py:140-175)
    const float* bx = a.boxes + i * 4;
    const float box[4] = {bx[0], bx[1], bx[2], bx[3]};
    float best = 0.f;
    int arg = 0;
    bool maxfg = false;
    for (int m = 0; m < a.M; ++m) {
      const float v = rp_iou(box, sgt + m * 5);
      if (m == 0 || v > best) { best = v; arg = m; }   // the first arg-max, padding rows included
      if (v == scol[m] && scol[m] > a.min_pos) maxfg = true;
    }
    float as = -1.0f;
    if (best < a.neg_thr) as = 0.0f;
    if (maxfg) as = 1.0f;
    if (best >= a.pos_thr) as = 1.0f;
    const float* g = sgt + arg * 5;     // a "max fg" box takes the class of its OWN arg-max gt
    const float lr = as > 0.f ? g[4] : as;
    a.label_refine[i] = lr;
    o = a.gt_refine + i * 4;
    o[0] = as > 0.f ? g[0] : 0.f; o[1] = as > 0.f ? g[1] : 0.f;
    o[2] = as > 0.f ? g[2] : 0.f; o[3] = as > 0.f ? g[3] : 0.f;
    cr = 1.0f <= lr;
  }
  ci = block_sum_i32<kRpT>(ci, shi);
  cr = block_sum_i32<kRpT>(cr, shi);
  if (threadIdx.x == 0) {
    const int b = blockIdx.y * gridDim.x + blockIdx.x;
    a.part[2 * b] = ci;
    a.part[2 * b + 1] = cr;
  }
}

__global__ __launch_bounds__(kRpT) void rp_state_kernel(const int* __restrict__ part, int blocks, int* __restrict__ state) {
  __shared__ int shi[kRpWaves];
  int ci = 0, cr = 0;
  for (int b = threadIdx.x; b < blocks; b += kRpT) {
    ci += part[2 * b];
    cr += part[2 * b + 1];
  }
  ci = block_sum_i32<kRpT>(ci, shi);
  cr = block_sum_i32<kRpT>(cr, shi);
  if (threadIdx.x == 0) {
    state[0] = ci;
    state[1] = cr;
    state[2] = __float_as_int((float)ci + 1.0f);   // sum(1 <= label) + 1 (bbox_norm-inl.h:119-122)
    state[3] = __float_as_int((float)cr + 1.0f);
  }
}

// ------------------------------------------------------------------------------------------ losses --
struct RpLossArgs {
  const float* pts[2][kRpMaxL];
  float* dpts[2][kRpMaxL];
  const float* label[2];
  const float* gtb[2];
  float* loss[2];
  const float* mt;
  const int* state;
  float* part;      // backward: [blocks][4] = (init x, init y, refine x, refine y)
  int N, add;
  float scale, grad_scale[2];
  RpLevels g;
};

// smooth_l1 / smooth_l1_grad (loss_common.h) with sigma = 3 (X.smooth_l1(scalar=3.0))
constexpr float kRpBsq = 9.0f, kRpIbsq = 1.0f / 9.0f;

struct RpLoc { int n, j, l, p, hw; float s, cx, cy; };
__device__ __forceinline__ RpLoc rp_loc(const RpLevels& g, unsigned i) {
  RpLoc q;
  q.n = (int)(i / (unsigned)g.P);
  q.j = (int)(i - (unsigned)q.n * (unsigned)g.P);
  q.l = rp_level(g, q.j);
  q.p = q.j - g.begin[q.l];
  q.hw = g.hw[q.l];
  const int w = g.gw[q.l], ph = q.p / w;
  q.s = (float)g.stride[q.l];
  q.cx = (float)((q.p - ph * w) * g.stride[q.l]);
  q.cy = (float)(ph * g.stride[q.l]);
  return q;
}

// _offset_to_pts (point_ops.py:33-48): (y, x) -> (x, y), * stride, + centre
template <int K>
__device__ __forceinline__ void rp_abs_points(const RpLossArgs& a, int stage, const RpLoc& q, float* x, float* y) {
  rp_load<K>(a.pts[stage][q.l] + (long)q.n * 2 * K * q.hw + q.p, q.hw, y, x);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    x[k] = x[k] * q.s + q.cx;
    y[k] = y[k] * q.s + q.cy;
  }
}

template <int K, int TR>
__global__ __launch_bounds__(kRpT) void rp_loss_fwd_kernel(RpLossArgs a) {
  const unsigned i = blockIdx.x * kRpT + threadIdx.x;
  if (i >= (unsigned)a.N * (unsigned)a.g.P) return;
  const RpLoc q = rp_loc(a.g, i);
  float e0 = 1.f, e1 = 1.f;
  if (TR == kRpMoment) { e0 = expf(a.mt[0]); e1 = expf(a.mt[1]); }
  const float nt = q.s * a.scale;   // normalize_term (builder.py:430-432)
#pragma unroll
  for (int st = 0; st < 2; ++st) {
    float x[K], y[K], box[4];
    rp_abs_points<K>(a, st, q, x, y);
    rp_points2bbox<K, TR>(x, y, e0, e1, box);
    const float w = a.label[st][i] > 0.f ? 1.0f : 0.0f;
    const float* g = a.gtb[st] + (long)i * 4;
    float* o = a.loss[st] + (long)i * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = smooth_l1((box[e] - g[e]) / nt, kRpBsq, kRpIbsq) * w;
  }
}

// gradient of min / max over the first Q values: every tied value takes it (MXNet's reduce backward)
template <int K, int Q>
__device__ __forceinline__ void rp_minmax_bwd(const float* v, float lo, float hi, float glo, float ghi, float* d) {
#pragma unroll
  for (int k = 0; k < K; ++k) d[k] = k < Q ? (v[k] == lo ? glo : 0.f) + (v[k] == hi ? ghi : 0.f) : 0.f;
}

// the chain rule of rp_moment as written; returns d(exp(moment_transfer)) of this set = d(half) * std
template <int K>
__device__ __forceinline__ float rp_moment_bwd(const float* v, float e, float glo, float ghi, float* d) {
  const RpMoment r = rp_moment<K>(v, e);
  const float dhalf = ghi - glo;          // lo = mean - half, hi = mean + half
  const float dmean0 = glo + ghi;
  const float dstd = dhalf * e;
  const float dv = dstd * (0.5f / r.std);   // sqrt: 0.5 / out; std = 0 gives 0 * inf = NaN as the expression does
  const float dq = dv / (float)K;
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    d[k] = dq * (2.0f * (v[k] - r.mean));
    s = s + d[k];
  }
  const float dm = (dmean0 - s) / (float)K;
#pragma unroll
  for (int k = 0; k < K; ++k) d[k] = d[k] + dm;
  return dhalf * r.std;
}

template <int K, int TR>
__global__ __launch_bounds__(kRpT) void rp_loss_bwd_kernel(RpLossArgs a) {
  __shared__ float sh[kRpWaves];
  const unsigned i = blockIdx.x * kRpT + threadIdx.x;
  const bool live = i < (unsigned)a.N * (unsigned)a.g.P;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  if (live) {
    const RpLoc q = rp_loc(a.g, i);
    float e0 = 1.f, e1 = 1.f;
    if (TR == kRpMoment) { e0 = expf(a.mt[0]); e1 = expf(a.mt[1]); }
    const float nt = q.s * a.scale;
#pragma unroll
    for (int st = 0; st < 2; ++st) {
      float x[K], y[K], box[4], gb[4], dx[K], dy[K];
      rp_abs_points<K>(a, st, q, x, y);
      rp_points2bbox<K, TR>(x, y, e0, e1, box);
      // MakeLoss writes grad_scale, BBoxNorm divides by its count + 1, then the weight, smooth-L1, the normaliser
      const float g0 = a.grad_scale[st] / __int_as_float(a.state[2 + st]);
      const float w = a.label[st][i] > 0.f ? 1.0f : 0.0f;
      const float* g = a.gtb[st] + (long)i * 4;
#pragma unroll
      for (int e = 0; e < 4; ++e) gb[e] = ((g0 * w) * smooth_l1_grad((box[e] - g[e]) / nt, kRpBsq, kRpIbsq)) / nt;
      if (TR == kRpMoment) {
        acc[2 * st] = rp_moment_bwd<K>(x, e0, gb[0], gb[2], dx);
        acc[2 * st + 1] = rp_moment_bwd<K>(y, e1, gb[1], gb[3], dy);
      } else {
        constexpr int Q = TR == kRpPartial ? (K < 4 ? K : 4) : K;
        rp_minmax_bwd<K, Q>(x, box[0], box[2], gb[0], gb[2], dx);
        rp_minmax_bwd<K, Q>(y, box[1], box[3], gb[1], gb[3], dy);
      }
      float* d = a.dpts[st][q.l] + (long)q.n * 2 * K * q.hw + q.p;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float vy = dy[k] * q.s, vx = dx[k] * q.s;
        float* py = d + (long)(2 * k) * q.hw;
        float* px = d + (long)(2 * k + 1) * q.hw;
        if (a.add) { *py = *py + vy; *px = *px + vx; } else { *py = vy; *px = vx; }
      }
    }
  }
  if (TR == kRpMoment) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const float v = block_sum_f32<kRpT>(acc[c], sh);
      if (threadIdx.x == 0) a.part[4 * blockIdx.x + c] = v;
    }
  }
}

// d_moment_transfer[k] = S_init[k] * exp(mt[k]) + S_refine[k] * exp(mt[k]): the partials in a fixed order
__global__ __launch_bounds__(kRpT) void rp_dmt_kernel(const float* __restrict__ part, int blocks, const float* __restrict__ mt,
                                                      float* __restrict__ dmt, int moment, int add) {
  __shared__ float sh[kRpWaves];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  if (moment) {
    for (int b = threadIdx.x; b < blocks; b += kRpT)
      for (int c = 0; c < 4; ++c) s[c] += part[4 * b + c];
    for (int c = 0; c < 4; ++c) s[c] = block_sum_f32<kRpT>(s[c], sh);
  }
  if (threadIdx.x == 0) {
    for (int k = 0; k < 2; ++k) {
      float v = 0.f;
      if (moment) {
        const float e = expf(mt[k]);
        v = s[k] * e + s[2 + k] * e;
      }
      dmt[k] = add ? dmt[k] + v : v;
    }
  }
}

static char* rp_align256(void* p) { return reinterpret_cast<char*>(((uintptr_t)p + 255) & ~(uintptr_t)255); }

// the level table shared by every entry point; *empty when there is nothing to do
static int rp_levels(RpLevels& g, const int* h, const int* w, const int* strides, int L, int N, int num_points,
                     int transform, bool* empty) {
  SD_REQUIRE(N >= 0 && L >= 0, "negative dimension (N=%d L=%d)", N, L);
  if (L > kRpMaxL) return fail(SD_ERR_UNSUPPORTED, "L=%d levels exceed the limit %d", L, kRpMaxL);
  SD_REQUIRE(transform >= kRpMinmax && transform <= kRpMoment, "transform=%d is none of minmax (0), partial_minmax (1), moment (2)", transform);
  if (num_points != 1 && num_points != 9 && num_points != 25)
    return fail(SD_ERR_UNSUPPORTED, "num_points=%d is not the square of an odd number up to 25", num_points);
  SD_REQUIRE(transform != kRpPartial || num_points >= 4, "partial_minmax takes the first four points, num_points=%d", num_points);
  SD_REQUIRE(L == 0 || (h && w && strides), "null level table");
  long total = 0;
  g.L = 0;
  g.begin[0] = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(h[l] >= 0 && w[l] >= 0, "level %d has a negative size %d x %d", l, h[l], w[l]);
    SD_REQUIRE(strides[l] >= 1, "stride %d of level %d is not positive", strides[l], l);
    const long hw = (long)h[l] * w[l];
    total += hw;
    if (total > kRpMaxElems) return fail(SD_ERR_UNSUPPORTED, "more than %ld points", kRpMaxElems);
    if ((double)(h[l] > w[l] ? h[l] : w[l]) * strides[l] > 16777216.0)
      return fail(SD_ERR_UNSUPPORTED, "level %d: a coordinate beyond 2^24 is not exact in float32", l);
  }
  if ((double)N * 2.0 * (num_points > 2 ? num_points : 2) * (double)total > (double)kRpMaxElems)
    return fail(SD_ERR_UNSUPPORTED, "N * 2 * num_points * P elements exceed the limit %ld", kRpMaxElems);
  if (N > kRpMaxImages) return fail(SD_ERR_UNSUPPORTED, "N=%d images exceed the limit %d", N, kRpMaxImages);
  for (int l = 0; l < L; ++l) {
    const long hw = (long)h[l] * w[l];
    if (hw == 0) continue;   // an empty level holds nothing
    const int i = g.L++;
    g.stride[i] = strides[l]; g.gw[i] = w[l]; g.hw[i] = (int)hw;
    g.begin[i + 1] = g.begin[i] + (int)hw;
    g.lvl[i] = floorf(log2f((float)strides[l]));
  }
  g.P = (int)total;
  *empty = N == 0 || total == 0;
  return SD_OK;
}

// copies the non-empty levels' pointers next to the compacted level table
template <typename T>
static int rp_pointers(T* dst, T const* src, const int* h, const int* w, int L, const char* what) {
  SD_REQUIRE(src, "null level table (%s)", what);
  int i = 0;
  for (int l = 0; l < L; ++l) {
    if ((long)h[l] * w[l] == 0) continue;
    SD_REQUIRE(src[l], "null pointer in level %d (%s)", l, what);
    dst[i++] = src[l];
  }
  return SD_OK;
}

#define RP_DISPATCH(KERNEL, num_points, transform, grid, st, args)                                              \
  do {                                                                                                          \
    if (num_points == 1) {                                                                                      \
      if (transform == kRpMoment) hipLaunchKernelGGL((KERNEL<1, kRpMoment>), grid, dim3(kRpT), 0, st, args);    \
      else hipLaunchKernelGGL((KERNEL<1, kRpMinmax>), grid, dim3(kRpT), 0, st, args);                           \
    } else if (num_points == 9) {                                                                               \
      if (transform == kRpMoment) hipLaunchKernelGGL((KERNEL<9, kRpMoment>), grid, dim3(kRpT), 0, st, args);    \
      else if (transform == kRpPartial) hipLaunchKernelGGL((KERNEL<9, kRpPartial>), grid, dim3(kRpT), 0, st, args); \
      else hipLaunchKernelGGL((KERNEL<9, kRpMinmax>), grid, dim3(kRpT), 0, st, args);                           \
    } else {                                                                                                    \
      if (transform == kRpMoment) hipLaunchKernelGGL((KERNEL<25, kRpMoment>), grid, dim3(kRpT), 0, st, args);   \
      else if (transform == kRpPartial) hipLaunchKernelGGL((KERNEL<25, kRpPartial>), grid, dim3(kRpT), 0, st, args); \
      else hipLaunchKernelGGL((KERNEL<25, kRpMinmax>), grid, dim3(kRpT), 0, st, args);                          \
    }                                                                                                           \
  } while (0)

struct RpWorkspace { size_t boxes, keys, colmax, part, total; };
static RpWorkspace rp_target_layout(int N, int M, long P) {
  RpWorkspace w;
  const size_t np = (size_t)N * (size_t)P, blocks = (size_t)N * (size_t)((P + kRpT - 1) / kRpT);
  w.boxes = 0;
  w.keys = w.boxes + np * 16;
  w.colmax = w.keys + np * 8;
  w.part = w.colmax + (((size_t)N * (size_t)M * 4 + 15) & ~(size_t)15);
  w.total = w.part + blocks * 8;
  return w;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_reppoints_target_workspace_bytes(int N, int M, long P) {
  if (N < 0 || M < 0 || P < 0) return 0;
  return 256 + rp_target_layout(N, M, P).total;
}

extern "C" int sd_reppoints_target(const float* const* pts_init_ptrs_host, const int* H_host, const int* W_host,
                                   const int* stride_host, int L, const float* gt_bbox,
                                   const float* moment_transfer_or_null, float* label_init, float* gt_init,
                                   float* label_refine, float* gt_refine, int* state, int N, int M, int num_points,
                                   int transform, float target_scale, int num_pos, float pos_iou_thr,
                                   float neg_iou_thr, float min_pos_iou, void* workspace, size_t workspace_bytes,
                                   void* stream) {
  SD_REQUIRE(M >= 0, "negative dimension (M=%d)", M);
  RpTargetArgs a{};
  bool empty = false;
  if (int e = rp_levels(a.g, H_host, W_host, stride_host, L, N, num_points, transform, &empty)) return e;
  if (M > kRpMaxM) return fail(SD_ERR_UNSUPPORTED, "M=%d gt rows exceed the limit %d", M, kRpMaxM);
  if (num_pos < 1 || num_pos > kRpMaxPos) return fail(SD_ERR_UNSUPPORTED, "num_pos=%d lies outside 1..%d", num_pos, kRpMaxPos);
  SD_REQUIRE(target_scale == target_scale && pos_iou_thr == pos_iou_thr && neg_iou_thr == neg_iou_thr && min_pos_iou == min_pos_iou,
             "target_scale, pos_iou_thr, neg_iou_thr or min_pos_iou is NaN");
  SD_REQUIRE(target_scale > 0.f, "target_scale=%g must be positive", (double)target_scale);
  if (empty) return SD_OK;
  SD_REQUIRE(M >= 1, "M=0: the arg-max over the gt rows needs at least one row per image");
  SD_REQUIRE(gt_bbox && label_init && gt_init && label_refine && gt_refine && state, "null pointer");
  SD_REQUIRE(transform != kRpMoment || moment_transfer_or_null, "null pointer: the moment transform needs moment_transfer");
  if (int e = rp_pointers(a.pts, pts_init_ptrs_host, H_host, W_host, L, "pts_init")) return e;
  const size_t need = sd_reppoints_target_workspace_bytes(N, M, a.g.P);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "reppoints_target workspace too small: %zu < %zu bytes", workspace_bytes, need);
  const RpWorkspace lay = rp_target_layout(N, M, a.g.P);
  char* base = rp_align256(workspace);
  a.boxes = reinterpret_cast<float*>(base + lay.boxes);
  a.keys = reinterpret_cast<unsigned long long*>(base + lay.keys);
  a.colmax = reinterpret_cast<unsigned*>(base + lay.colmax);
  a.part = reinterpret_cast<int*>(base + lay.part);
  a.gt = gt_bbox; a.mt = moment_transfer_or_null;
  a.label_init = label_init; a.gt_init = gt_init; a.label_refine = label_refine; a.gt_refine = gt_refine;
  a.N = N; a.M = M; a.num_pos = num_pos;
  a.scale = target_scale; a.pos_thr = pos_iou_thr; a.neg_thr = neg_iou_thr; a.min_pos = min_pos_iou;
  a.lvl_min = a.lvl_max = a.g.lvl[0];
  for (int l = 1; l < a.g.L; ++l) {
    a.lvl_min = fminr(a.lvl_min, a.g.lvl[l]);
    a.lvl_max = fmaxr(a.lvl_max, a.g.lvl[l]);
  }
  hipStream_t st = (hipStream_t)stream;
  const int bx = cdiv(a.g.P, kRpT), blocks = bx * N;
  const long nkeys = (long)N * a.g.P, ncol = (long)N * M;
  const int init_blocks = (int)(cdiv(nkeys, kRpT) > kNumCU * 4 ? kNumCU * 4 : cdiv(nkeys, kRpT));
  hipLaunchKernelGGL(rp_init_kernel, dim3(init_blocks), dim3(kRpT), 0, st, a.keys, nkeys, a.colmax, ncol);
  hipLaunchKernelGGL(rp_point_kernel, dim3(M, N), dim3(kRpT), 0, st, a);
  RP_DISPATCH(rp_box_kernel, num_points, transform, dim3(bx, N), st, a);
  hipLaunchKernelGGL(rp_assign_kernel, dim3(bx, N), dim3(kRpT), 0, st, a);
  hipLaunchKernelGGL(rp_state_kernel, dim3(1), dim3(kRpT), 0, st, a.part, blocks, state);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

static int rp_loss_args(RpLossArgs& a, const float* const* pi, const float* const* pr, const int* H, const int* W,
                        const int* strides, int L, const float* mt, const float* label_init, const float* gt_init,
                        const float* label_refine, const float* gt_refine, int N, int num_points, int transform,
                        float scale, bool* empty) {
  if (int e = rp_levels(a.g, H, W, strides, L, N, num_points, transform, empty)) return e;
  SD_REQUIRE(scale == scale && scale > 0.f, "scale=%g must be positive", (double)scale);
  if (*empty) return SD_OK;
  SD_REQUIRE(label_init && gt_init && label_refine && gt_refine, "null pointer");
  SD_REQUIRE(transform != kRpMoment || mt, "null pointer: the moment transform needs moment_transfer");
  if (int e = rp_pointers(a.pts[0], pi, H, W, L, "pts_init")) return e;
  if (int e = rp_pointers(a.pts[1], pr, H, W, L, "pts_refine")) return e;
  a.label[0] = label_init; a.label[1] = label_refine; a.gtb[0] = gt_init; a.gtb[1] = gt_refine;
  a.mt = mt; a.N = N; a.scale = scale;
  return SD_OK;
}

extern "C" int sd_reppoints_box_loss_fwd(const float* const* pts_init_ptrs_host, const float* const* pts_refine_ptrs_host,
                                         const int* H_host, const int* W_host, const int* stride_host, int L,
                                         const float* moment_transfer_or_null, const float* label_init,
                                         const float* gt_init, const float* label_refine, const float* gt_refine,
                                         float* loss_init, float* loss_refine, int N, int num_points, int transform,
                                         float scale, void* stream) {
  RpLossArgs a{};
  bool empty = false;
  if (int e = rp_loss_args(a, pts_init_ptrs_host, pts_refine_ptrs_host, H_host, W_host, stride_host, L,
                           moment_transfer_or_null, label_init, gt_init, label_refine, gt_refine, N, num_points,
                           transform, scale, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(loss_init && loss_refine, "null pointer");
  a.loss[0] = loss_init; a.loss[1] = loss_refine;
  hipStream_t st = (hipStream_t)stream;
  const int grid = cdiv((long)N * a.g.P, kRpT);
  RP_DISPATCH(rp_loss_fwd_kernel, num_points, transform, dim3(grid), st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" size_t sd_reppoints_box_loss_workspace_bytes(int N, long P) {
  if (N < 0 || P < 0) return 0;
  return 256 + (size_t)(((long)N * P + kRpT - 1) / kRpT) * 4 * sizeof(float);
}

extern "C" int sd_reppoints_box_loss_bwd(const float* const* pts_init_ptrs_host, const float* const* pts_refine_ptrs_host,
                                         const int* H_host, const int* W_host, const int* stride_host, int L,
                                         const float* moment_transfer_or_null, const float* label_init,
                                         const float* gt_init, const float* label_refine, const float* gt_refine,
                                         const int* state, float* const* d_init_ptrs_host,
                                         float* const* d_refine_ptrs_host, float* d_moment_transfer, int N,
                                         int num_points, int transform, float scale, float grad_scale_init,
                                         float grad_scale_refine, int req, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  RpLossArgs a{};
  bool empty = false;
  if (int e = rp_loss_args(a, pts_init_ptrs_host, pts_refine_ptrs_host, H_host, W_host, stride_host, L,
                           moment_transfer_or_null, label_init, gt_init, label_refine, gt_refine, N, num_points,
                           transform, scale, &empty)) return e;
  SD_REQUIRE(req == 1 || req == 3, "req=%d is neither write (1) nor add (3)", req);
  SD_REQUIRE(grad_scale_init == grad_scale_init && grad_scale_refine == grad_scale_refine, "a grad_scale is NaN");
  if (empty) return SD_OK;
  SD_REQUIRE(state && d_moment_transfer, "null pointer");
  if (int e = rp_pointers(a.dpts[0], d_init_ptrs_host, H_host, W_host, L, "d_pts_init")) return e;
  if (int e = rp_pointers(a.dpts[1], d_refine_ptrs_host, H_host, W_host, L, "d_pts_refine")) return e;
  const size_t need = sd_reppoints_box_loss_workspace_bytes(N, a.g.P);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "reppoints_box_loss_bwd workspace too small: %zu < %zu bytes", workspace_bytes, need);
  a.state = state; a.add = req == 3;
  a.grad_scale[0] = grad_scale_init; a.grad_scale[1] = grad_scale_refine;
  a.part = reinterpret_cast<float*>(rp_align256(workspace));
  hipStream_t st = (hipStream_t)stream;
  const int grid = cdiv((long)N * a.g.P, kRpT);
  RP_DISPATCH(rp_loss_bwd_kernel, num_points, transform, dim3(grid), st, a);
  hipLaunchKernelGGL(rp_dmt_kernel, dim3(1), dim3(kRpT), 0, st, a.part, grid, moment_transfer_or_null,
                     d_moment_transfer, (int)(transform == kRpMoment), a.add);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
