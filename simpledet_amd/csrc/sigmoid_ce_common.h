// The element, unit and reduction code of SigmoidCrossEntropy, shared by sigmoid_ce.hip (the drop-in operator and
// the fused Mask R-CNN mask loss) and msrcnn_head.hip (the Mask Scoring R-CNN mask loss, which also writes the
// gathered sigmoid and takes a second gradient into the selected plane).  Both files run THESE functions, so the
// bit-equalities between their entry points hold by construction.  The rules are stated at the top of
// sigmoid_ce.hip.
#pragma once
#include "common.h"
#include "loss_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {

constexpr int kCeT = 256;
constexpr int kCeWaves = kCeT / kWave;
constexpr unsigned kCeUnit = 4 * kWave;        // elements per unit (one wave, four per lane)
constexpr int kCeMaxBlocks = kNumCU * 8;       // memory-bound grid: 8 workgroups per CU, stride the rest
constexpr long kCeMaxElems = 2147483647L;      // element and unit indices are 32-bit inside the kernels

__device__ __forceinline__ float ce_loss(float x, float t) {
  const float ge = x >= 0.0f ? 1.0f : 0.0f;
  const float lg = logf(1.0f + expf(x - (2.0f * x) * ge));
  return (float)((-1.0 * (double)x) * (double)(t - ge) + (double)lg);
}

__device__ __forceinline__ float ce_grad(float x, float t, float count_sum, float scale) {
  const float g = (float)(1.0 / (1.0 + (double)expf(-x)) - (double)t);
  return (g / count_sum) * scale;
}

// (int)cls when it names a plane, -1 otherwise (NaN fails both comparisons)
__device__ __forceinline__ int mask_class(float c, unsigned K) {
  return c >= 0.0f && c < (float)K ? (int)c : -1;
}

template <bool VEC>
__device__ __forceinline__ float4 ce_load4(const float* __restrict__ p, unsigned cnt) {
  if (VEC) return *reinterpret_cast<const float4*>(p);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  if (cnt > 0) v.x = p[0];
  if (cnt > 1) v.y = p[1];
  if (cnt > 2) v.z = p[2];
  if (cnt > 3) v.w = p[3];
  return v;
}

template <bool VEC>
__device__ __forceinline__ void ce_store4(float* __restrict__ p, unsigned cnt, const float4& v) {
  if (VEC) {
    *reinterpret_cast<float4*>(p) = v;
    return;
  }
  if (cnt > 0) p[0] = v.x;
  if (cnt > 1) p[1] = v.y;
  if (cnt > 2) p[2] = v.z;
  if (cnt > 3) p[3] = v.w;
}

// The two sources of (x, t) for `cnt` (1..4) consecutive elements of row `row` from element e0 on.
// Absent elements and ignored ones come back with t = -1 and x = 0.
struct CeRows {            // the drop-in operator: (n, k) rows
  const float* data;
  const float* label;
  unsigned k;
  template <bool VEC>
  __device__ __forceinline__ float4 targets(unsigned row, unsigned e0, unsigned cnt) const {
    float4 t = ce_load4<VEC>(label + (size_t)row * k + e0, cnt);
    if (!VEC) {
      if (cnt < 2) t.y = -1.0f;
      if (cnt < 3) t.z = -1.0f;
      if (cnt < 4) t.w = -1.0f;
    }
    return t;
  }
  template <bool VEC>
  __device__ __forceinline__ float4 logits_at(unsigned row, unsigned e0, unsigned cnt, const float4&) const {
    return ce_load4<VEC>(data + (size_t)row * k + e0, cnt);
  }
};

struct CeMask {            // the fused op: element e of the one row is (r, p) = (e / P, e % P) of plane cls[r]
  const float* logits;
  const float* cls;
  const float* target;
  unsigned K, P;
  __device__ __forceinline__ float one_target(unsigned e) const {
    return mask_class(cls[e / P], K) < 0 ? -1.0f : target[e];
  }
  __device__ __forceinline__ float one_logit(unsigned e) const {
    const unsigned r = e / P;
    const int c = mask_class(cls[r], K);
    return logits[((size_t)r * K + (unsigned)c) * P + (e - r * P)];
  }
  template <bool VEC>
  __device__ __forceinline__ float4 targets(unsigned, unsigned e0, unsigned cnt) const {
    if (VEC) {   // P % 4 == 0: the four elements lie in one RoI
      const float4 t = *reinterpret_cast<const float4*>(target + e0);
      return mask_class(cls[e0 / P], K) < 0 ? make_float4(-1.f, -1.f, -1.f, -1.f) : t;
    }
    float4 t = make_float4(-1.f, -1.f, -1.f, -1.f);
    if (cnt > 0) t.x = one_target(e0);
    if (cnt > 1) t.y = one_target(e0 + 1);
    if (cnt > 2) t.z = one_target(e0 + 2);
    if (cnt > 3) t.w = one_target(e0 + 3);
    return t;
  }
  // (a rejected row's logits are not read: its targets came back as -1)
  template <bool VEC>
  __device__ __forceinline__ float4 logits_at(unsigned, unsigned e0, unsigned cnt, const float4& t) const {
    float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
      const unsigned r = e0 / P;
      const int c = mask_class(cls[r], K);
      if (c >= 0) x = *reinterpret_cast<const float4*>(logits + ((size_t)r * K + (unsigned)c) * P + (e0 - r * P));
      return x;
    }
    if (cnt > 0 && t.x != -1.0f) x.x = one_logit(e0);
    if (cnt > 1 && t.y != -1.0f) x.y = one_logit(e0 + 1);
    if (cnt > 2 && t.z != -1.0f) x.z = one_logit(e0 + 2);
    if (cnt > 3 && t.w != -1.0f) x.w = one_logit(e0 + 3);
    return x;
  }
};

struct CeUnits {
  unsigned units, per_row, k;   // units = n * per_row, per_row = ceil(k / kCeUnit)
};

// elements of the lane in unit u: row, first element, how many (0..4)
__device__ __forceinline__ void ce_lane_span(const CeUnits& g, unsigned u, unsigned& row, unsigned& e0, unsigned& cnt) {
  row = u / g.per_row;
  e0 = (u - row * g.per_row) * kCeUnit + 4u * (threadIdx.x & (kWave - 1));
  cnt = e0 >= g.k ? 0u : (g.k - e0 < 4u ? g.k - e0 : 4u);
}

// One unit of the forward, whole wave: loss / count elements (when asked for) and the unit's partial loss sum and
// count.  The lane's span and what it loaded come back for a caller that has more to do with them.
template <class Src, bool VEC>
__device__ __forceinline__ void ce_fwd_unit(const Src& s, const CeUnits& g, unsigned u, float* __restrict__ loss,
                                            float* __restrict__ count, float* __restrict__ lpart,
                                            int* __restrict__ cpart, unsigned& e0, unsigned& cnt, float4& t,
                                            float4& x) {
  unsigned row;
  ce_lane_span(g, u, row, e0, cnt);
  float4 l = make_float4(0.f, 0.f, 0.f, 0.f), c = l;
  t = make_float4(-1.f, -1.f, -1.f, -1.f);
  x = l;
  if (cnt) {
    t = s.template targets<VEC>(row, e0, cnt);
    x = s.template logits_at<VEC>(row, e0, cnt, t);
    if (t.x != -1.0f) { l.x = ce_loss(x.x, t.x); c.x = 1.0f; }
    if (t.y != -1.0f) { l.y = ce_loss(x.y, t.y); c.y = 1.0f; }
    if (t.z != -1.0f) { l.z = ce_loss(x.z, t.z); c.z = 1.0f; }
    if (t.w != -1.0f) { l.w = ce_loss(x.w, t.w); c.w = 1.0f; }
    const size_t at = (size_t)row * g.k + e0;
    if (loss) ce_store4<VEC>(loss + at, cnt, l);
    if (count) ce_store4<VEC>(count + at, cnt, c);
  }
  const float a = wave_sum_f32(((l.x + l.y) + l.z) + l.w);
  const int n = wave_sum_i32((int)c.x + (int)c.y + (int)c.z + (int)c.w);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    lpart[u] = a;
    cpart[u] = n;
  }
}

// forward: every unit
template <class Src, bool VEC>
__global__ __launch_bounds__(kCeT) void ce_fwd_units_kernel(Src s, CeUnits g, float* __restrict__ loss,
                                                            float* __restrict__ count, float* __restrict__ lpart,
                                                            int* __restrict__ cpart) {
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned u = blockIdx.x * kCeWaves + threadIdx.x / kWave; u < g.units; u += step) {
    unsigned e0, cnt;
    float4 t, x;
    ce_fwd_unit<Src, VEC>(s, g, u, loss, count, lpart, cpart, e0, cnt, t, x);
  }
}

// backward, first pass: the unit's count (and the count elements when asked for)
template <class Src, bool VEC>
__global__ __launch_bounds__(kCeT) void ce_count_units_kernel(Src s, CeUnits g, float* __restrict__ count,
                                                              int* __restrict__ cpart) {
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned u = blockIdx.x * kCeWaves + threadIdx.x / kWave; u < g.units; u += step) {
    unsigned row, e0, cnt;
    ce_lane_span(g, u, row, e0, cnt);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (cnt) {
      const float4 t = s.template targets<VEC>(row, e0, cnt);
      c = make_float4(t.x != -1.0f ? 1.f : 0.f, t.y != -1.0f ? 1.f : 0.f, t.z != -1.0f ? 1.f : 0.f,
                      t.w != -1.0f ? 1.f : 0.f);
      if (count) ce_store4<VEC>(count + (size_t)row * g.k + e0, cnt, c);
    }
    const int n = wave_sum_i32((int)c.x + (int)c.y + (int)c.z + (int)c.w);
    if ((threadIdx.x & (kWave - 1)) == 0) cpart[u] = n;
  }
}

// a wave per row: the partials in a fixed order.  lpart null: counts only (the backward)
static __global__ __launch_bounds__(kCeT) void ce_rows_kernel(const float* __restrict__ lpart,
                                                              const int* __restrict__ cpart, unsigned n,
                                                              unsigned per_row, float* __restrict__ out,
                                                              float* __restrict__ loss_sum,
                                                              float* __restrict__ count_sum) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned row = blockIdx.x * kCeWaves + threadIdx.x / kWave; row < n; row += step) {
    const size_t base = (size_t)row * per_row;
    float a = 0.f;
    int c = 0;
    for (unsigned i = lane; i < per_row; i += kWave) {
      if (lpart) a += lpart[base + i];
      c += cpart[base + i];
    }
    a = wave_sum_f32(a);
    c = wave_sum_i32(c);
    if (lane == 0) {
      const float cs = (float)c + 1e-5f;
      count_sum[row] = cs;
      if (lpart) {
        if (loss_sum) loss_sum[row] = a;
        out[row] = a / cs;
      }
    }
  }
}

// fused backward, second pass: a workgroup per plane (r, kk) of d_logits, every plane written exactly once.
// VST: 16-byte stores; VLD: 16-byte loads of the selected plane, its targets and (DP) its d_prob row.
// DP: the selected plane also receives d_prob * (p * (1 - p)), p = sigmoid_f32(x) -- the gradient that arrives
// through the gathered sigmoid (msrcnn_head.hip); at an ignored element (t == -1) that term stands alone.
template <bool VST, bool VLD, bool DP>
__global__ __launch_bounds__(kCeT) void mask_loss_bwd_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ cls,
                                                             const float* __restrict__ target,
                                                             const float* __restrict__ d_prob,
                                                             float* __restrict__ d_logits,
                                                             const float* __restrict__ count_sum, unsigned planes,
                                                             unsigned K, unsigned P, float scale) {
  const float cs = *count_sum;
  unsigned pl = blockIdx.x;
  float cv = pl < planes ? cls[pl / K] : 0.f;
  while (pl < planes) {
    // the next plane's class is asked for before this plane's stores are issued
    const unsigned next = pl + gridDim.x;
    const float cn = next < planes ? cls[next / K] : 0.f;
    const unsigned r = pl / K;
    const bool sel = mask_class(cv, K) == (int)(pl - r * K);
    const size_t base = (size_t)pl * P;
    const float* tp = target + (size_t)r * P;
    const float* dp = DP ? d_prob + (size_t)r * P : nullptr;
    if (VST) {
      for (unsigned i = 4u * threadIdx.x; i < P; i += 4u * kCeT) {
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sel) {
          const float4 t = ce_load4<VLD>(tp + i, 4);
          const float4 x = ce_load4<VLD>(logits + base + i, 4);
          // (asked for next to the other two loads: behind the branches below it would wait out a second latency)
          const float4 g = DP ? ce_load4<VLD>(dp + i, 4) : make_float4(0.f, 0.f, 0.f, 0.f);
          if (t.x != -1.0f) d.x = ce_grad(x.x, t.x, cs, scale);
          if (t.y != -1.0f) d.y = ce_grad(x.y, t.y, cs, scale);
          if (t.z != -1.0f) d.z = ce_grad(x.z, t.z, cs, scale);
          if (t.w != -1.0f) d.w = ce_grad(x.w, t.w, cs, scale);
          if (DP) {
            const float4 p = make_float4(sigmoid_f32(x.x), sigmoid_f32(x.y), sigmoid_f32(x.z), sigmoid_f32(x.w));
            d.x = d.x + g.x * (p.x * (1.0f - p.x));
            d.y = d.y + g.y * (p.y * (1.0f - p.y));
            d.z = d.z + g.z * (p.z * (1.0f - p.z));
            d.w = d.w + g.w * (p.w * (1.0f - p.w));
          }
        }
        *reinterpret_cast<float4*>(d_logits + base + i) = d;
      }
    } else {
      for (unsigned i = threadIdx.x; i < P; i += kCeT) {
        float d = 0.f;
        if (sel) {
          const float t = tp[i];
          if (DP) {
            const float x = logits[base + i];
            const float g = dp[i];
            if (t != -1.0f) d = ce_grad(x, t, cs, scale);
            const float p = sigmoid_f32(x);
            d = d + g * (p * (1.0f - p));
          } else if (t != -1.0f) {
            d = ce_grad(logits[base + i], t, cs, scale);
          }
        }
        d_logits[base + i] = d;
      }
    }
    cv = cn;
    pl = next;
  }
}

static bool ce_aligned16(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

static int ce_grid(long items, int per_block) {
  const long b = (items + per_block - 1) / per_block;
  return (int)(b < 1 ? 1 : b > kCeMaxBlocks ? kCeMaxBlocks : b);
}

static long ce_units_per_row(long k) { return (k + kCeUnit - 1) / kCeUnit; }

// workspace: [256-byte alignment slack][units floats][units ints][one float: the fused backward's count_sum]
static size_t ce_workspace_bytes(long n, long k) {
  if (n <= 0 || k <= 0 || n > kCeMaxElems / k) return 512;
  const size_t units = (size_t)n * (size_t)ce_units_per_row(k);
  return 256 + ((units * 8 + 255) & ~(size_t)255) + 256;
}

struct CeWorkspace {
  float* lpart;
  int* cpart;
  float* count_sum;
};

static int ce_carve(void* workspace, size_t workspace_bytes, long n, long k, const char* who, CeWorkspace* w) {
  const size_t need = ce_workspace_bytes(n, k);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "%s workspace too small: %zu < %zu bytes", who, workspace_bytes, need);
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  const size_t units = (size_t)n * (size_t)ce_units_per_row(k);
  w->lpart = reinterpret_cast<float*>(base);
  w->cpart = reinterpret_cast<int*>(base + units * 4);
  w->count_sum = reinterpret_cast<float*>(base + ((units * 8 + 255) & ~(size_t)255));
  return SD_OK;
}

static CeUnits ce_units(long n, long k) {
  CeUnits g;
  g.per_row = (unsigned)ce_units_per_row(k);
  g.units = (unsigned)(n * ce_units_per_row(k));
  g.k = (unsigned)k;
  return g;
}

template <class Src>
static void launch_fwd_units(const Src& s, const CeUnits& g, bool vec, float* loss, float* count,
                             const CeWorkspace& w, hipStream_t st) {
  const int grid = ce_grid(g.units, kCeWaves);
  if (vec)
    hipLaunchKernelGGL((ce_fwd_units_kernel<Src, true>), dim3(grid), dim3(kCeT), 0, st, s, g, loss, count, w.lpart,
                       w.cpart);
  else
    hipLaunchKernelGGL((ce_fwd_units_kernel<Src, false>), dim3(grid), dim3(kCeT), 0, st, s, g, loss, count, w.lpart,
                       w.cpart);
}

template <class Src>
static void launch_count_units(const Src& s, const CeUnits& g, bool vec, float* count, const CeWorkspace& w,
                               hipStream_t st) {
  const int grid = ce_grid(g.units, kCeWaves);
  if (vec)
    hipLaunchKernelGGL((ce_count_units_kernel<Src, true>), dim3(grid), dim3(kCeT), 0, st, s, g, count, w.cpart);
  else
    hipLaunchKernelGGL((ce_count_units_kernel<Src, false>), dim3(grid), dim3(kCeT), 0, st, s, g, count, w.cpart);
}

static void launch_rows(const float* lpart, const CeWorkspace& w, const CeUnits& g, long n, float* out,
                        float* loss_sum, float* count_sum, hipStream_t st) {
  hipLaunchKernelGGL(ce_rows_kernel, dim3(ce_grid(n, kCeWaves)), dim3(kCeT), 0, st, lpart, w.cpart, (unsigned)n,
                     g.per_row, out, loss_sum, count_sum);
}

// the fused backward's three launches: the count of the gathered row, its count_sum, the dense gradient.
// d_prob null: the mask loss alone (sd_mask_loss_bwd); else the sigmoid's gradient joins in the selected plane.
static void launch_mask_bwd(const float* logits, const float* cls, const float* target, const float* d_prob,
                            float* d_logits, int R, int K, long P, float grad_scale, const CeWorkspace& w,
                            hipStream_t st) {
  const CeUnits g = ce_units(1, (long)R * P);
  const CeMask s{logits, cls, target, (unsigned)K, (unsigned)P};
  const bool vcount = P % 4 == 0 && ce_aligned16(logits, target);
  launch_count_units(s, g, vcount, nullptr, w, st);
  launch_rows(nullptr, w, g, 1, nullptr, nullptr, w.count_sum, st);
  const unsigned planes = (unsigned)((long)R * K);
  const int grid = ce_grid(planes, 1);
  const bool vld = vcount && ce_aligned16(d_prob);
  const bool vst = P % 4 == 0 && ce_aligned16(d_logits);
#define SD_MASK_BWD(VST, VLD, DP)                                                                               \
  hipLaunchKernelGGL((mask_loss_bwd_kernel<VST, VLD, DP>), dim3(grid), dim3(kCeT), 0, st, logits, cls, target,  \
                     d_prob, d_logits, (const float*)w.count_sum, planes, (unsigned)K, (unsigned)P, grad_scale)
  if (d_prob) {
    if (vst && vld) SD_MASK_BWD(true, true, true);
    else if (vst) SD_MASK_BWD(true, false, true);
    else SD_MASK_BWD(false, false, true);
  } else {
    if (vst && vld) SD_MASK_BWD(true, true, false);
    else if (vst) SD_MASK_BWD(true, false, false);
    else SD_MASK_BWD(false, false, false);
  }
#undef SD_MASK_BWD
}

static int mask_check_dims(int R, int K, long P) {
  SD_REQUIRE(R >= 0 && K >= 0 && P >= 0, "negative dimension (R=%d K=%d P=%ld)", R, K, P);
  const long planes = (long)R * K;
  if (P > 0 && planes > kCeMaxElems / P)
    return fail(SD_ERR_UNSUPPORTED, "R*K*P = %d x %d x %ld elements exceed the limit %ld", R, K, P, kCeMaxElems);
  return SD_OK;
}

static size_t mask_workspace_bytes(int R, int K, long P) {
  if (R <= 0 || K <= 0 || P <= 0) return 512;
  return ce_workspace_bytes(1, (long)R * P > kCeMaxElems ? 0 : (long)R * P);
}

}  // namespace sd
