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
#include "common.h"
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

// forward: loss / count elements (when asked for) and the unit's partial loss sum and count
template <class Src, bool VEC>
__global__ __launch_bounds__(kCeT) void ce_fwd_units_kernel(Src s, CeUnits g, float* __restrict__ loss,
                                                            float* __restrict__ count, float* __restrict__ lpart,
                                                            int* __restrict__ cpart) {
  const unsigned step = gridDim.x * kCeWaves;
  for (unsigned u = blockIdx.x * kCeWaves + threadIdx.x / kWave; u < g.units; u += step) {
    unsigned row, e0, cnt;
    ce_lane_span(g, u, row, e0, cnt);
    float4 l = make_float4(0.f, 0.f, 0.f, 0.f), c = l;
    if (cnt) {
      const float4 t = s.template targets<VEC>(row, e0, cnt);
      const float4 x = s.template logits_at<VEC>(row, e0, cnt, t);
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
__global__ __launch_bounds__(kCeT) void ce_rows_kernel(const float* __restrict__ lpart, const int* __restrict__ cpart,
                                                       unsigned n, unsigned per_row, float* __restrict__ out,
                                                       float* __restrict__ loss_sum, float* __restrict__ count_sum) {
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

// fused backward, second pass: a workgroup per plane (r, kk) of d_logits, every plane written exactly once.
// VST: 16-byte stores; VLD: 16-byte loads of the selected plane and its targets.
template <bool VST, bool VLD>
__global__ __launch_bounds__(kCeT) void mask_loss_bwd_kernel(const float* __restrict__ logits,
                                                             const float* __restrict__ cls,
                                                             const float* __restrict__ target,
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
    if (VST) {
      for (unsigned i = 4u * threadIdx.x; i < P; i += 4u * kCeT) {
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
        if (sel) {
          const float4 t = ce_load4<VLD>(tp + i, 4);
          const float4 x = ce_load4<VLD>(logits + base + i, 4);
          if (t.x != -1.0f) d.x = ce_grad(x.x, t.x, cs, scale);
          if (t.y != -1.0f) d.y = ce_grad(x.y, t.y, cs, scale);
          if (t.z != -1.0f) d.z = ce_grad(x.z, t.z, cs, scale);
          if (t.w != -1.0f) d.w = ce_grad(x.w, t.w, cs, scale);
        }
        *reinterpret_cast<float4*>(d_logits + base + i) = d;
      }
    } else {
      for (unsigned i = threadIdx.x; i < P; i += kCeT) {
        float d = 0.f;
        if (sel) {
          const float t = tp[i];
          if (t != -1.0f) d = ce_grad(logits[base + i], t, cs, scale);
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
static int mask_check_dims(int R, int K, long P) {
  SD_REQUIRE(R >= 0 && K >= 0 && P >= 0, "negative dimension (R=%d K=%d P=%ld)", R, K, P);
  const long planes = (long)R * K;
  if (P > 0 && planes > kCeMaxElems / P)
    return fail(SD_ERR_UNSUPPORTED, "R*K*P = %d x %d x %ld elements exceed the limit %ld", R, K, P, kCeMaxElems);
  return SD_OK;
}

extern "C" size_t sd_mask_loss_workspace_bytes(int R, int K, long P) {
  if (R <= 0 || K <= 0 || P <= 0) return 512;
  return ce_workspace_bytes(1, (long)R * P > kCeMaxElems ? 0 : (long)R * P);
}

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
  const long k = (long)R * P;
  CeWorkspace w;
  if (int e = ce_carve(workspace, workspace_bytes, 1, k, "mask_loss_bwd", &w)) return e;
  hipStream_t st = (hipStream_t)stream;
  const CeUnits g = ce_units(1, k);
  const CeMask s{logits, cls, target, (unsigned)K, (unsigned)P};
  const bool vld = P % 4 == 0 && ce_aligned16(logits, target);
  launch_count_units(s, g, vld, nullptr, w, st);
  launch_rows(nullptr, w, g, 1, nullptr, nullptr, w.count_sum, st);
  const unsigned planes = (unsigned)((long)R * K);
  const int grid = ce_grid(planes, 1);
  const bool vst = P % 4 == 0 && ce_aligned16(d_logits);
#define SD_MASK_BWD(VST, VLD)                                                                                  \
  hipLaunchKernelGGL((mask_loss_bwd_kernel<VST, VLD>), dim3(grid), dim3(kCeT), 0, st, logits, cls, target,     \
                     d_logits, (const float*)w.count_sum, planes, (unsigned)K, (unsigned)P, grad_scale)
  if (vst && vld) SD_MASK_BWD(true, true);
  else if (vst) SD_MASK_BWD(true, false);
  else SD_MASK_BWD(false, false);
#undef SD_MASK_BWD
  SD_LAUNCH_CHECK();
  return SD_OK;
}
