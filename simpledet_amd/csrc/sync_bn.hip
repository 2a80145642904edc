// _contrib_SyncBatchNorm forward and backward for gfx950, fp32 and fp16, NCHW, with the rank exchange left to the
// caller between two entry points.
//
// The reference (operator_cxx/contrib/sync_batch_norm-inl.h) spends, per layer and direction, three to five
// tensor passes, two device-to-host copies, a host barrier with a host-side add and two copies back
// (:325-351 forward, :464-494 backward).  Here a direction is two entry points with the exchange of a (2, C)
// float32 block between them; with one rank the exchange is the identity and the two follow back to back.
//
// Contract.  x / y / dy / dx (N, C, HxW); gamma, beta, mean, var, moving_*, dgamma, dbeta (C) float32;
// n = N * HxW; W ranks with the same n (the reference's SharedND::MeanReady divides by ndev, :146-158);
// g = fix_gamma ? 1 : gamma[c].  Every float32 step is rounded on its own (-ffp-contract=off).
//   sd_sync_bn_stats       part[0, c] = the mean of the rank's n elements, part[1, c] = their biased variance
//                          ABOUT THAT MEAN.  x is read once: a chunk is resident in registers.
//   sd_sync_bn_apply       parts (W, 2, C) in rank order.  Per channel in double, ranks in order:
//                            m = (sum_r mean_r) / W,  v = (sum_r (var_r + (mean_r - m)^2)) / W
//                          mean = (float)m, var = (float)v (both outputs; exact copies of part for W = 1);
//                          inv = 1.0f / sqrtf(var + eps);  y = (g * (x - mean)) * inv + beta[c]        (:354-357)
//   sd_sync_bn_infer_fwd   a = g / sqrtf(moving_var + eps);  b = beta - (g * moving_mean) / sqrtf(moving_var + eps);
//                          y = a * x + b                                                             (:359-363)
//   sd_sync_bn_bwd_stats   bpart[0, c] = sum dy, bpart[1, c] = sum dy * (x - mean)                    (:476-477)
//   sd_sync_bn_bwd_apply   bparts (W, 2, C).  Per channel in double: SG = sum_r bpart_r[0], SP = sum_r bpart_r[1],
//                          sg = (float)(SG / (W * n)), sp = (float)(SP / (W * n)); then in float32
//                            inv = 1.0f / sqrtf(var + eps);  a = g * inv;  b = -(g * sp) * ((inv * inv) * inv);
//                            c = -(g * sg) * inv;  dx = (dy * a + b * (x - mean)) + c
//                          -- :496-513 with the averaged sums and scale = 1 / n multiplied out.
//                          dbeta[c] = bparts[rank][0][c];  dgamma[c] = fix_gamma ? 0 : bparts[rank][1][c] * inv
//                          (per rank, as :503 and :514: the gradient all-reduce sums them).
//                          moving = moving * momentum + stat * (1.0f - momentum), here in the backward and with the
//                          biased variance, as :471-472.
// Departures from the reference, all deliberate: (1) the variance is taken about the mean; its fp32
// E[x^2] - mean^2 (:333-334, :353) cancels when |mean| >> sigma (the decision of group_norm.hip); (2) the
// operator multiplies by inv where the reference divides per element (:355-356); (3) dgamma is
// (sum dy * (x - mean)) * inv where the reference sums dy * (x - mean) / sqrt(...) (:503); (4) gamma is never
// written: the reference's slope = 1.f under fix_gamma stores ones into the input (:320, :460).
// Not provided: kAddTo, the backward under use_global_stats, gradients arriving on mean / var.
//
// Kernels.  A channel's elements are N runs of HxW at stride C * HxW.  They are cut into ITEMS of L elements,
// L = 8 where HxW % 8 == 0, 4 where HxW % 4 == 0, else 1: L depends on the shape alone, NOT on the element type or
// the pointers, and every sum is defined on items (an item's elements pairwise, a thread's items in order, the wave
// butterfly, the four waves left to right, the partials in index order).  How an item is moved does depend on
// them -- 16-byte accesses where the pointers are 16-byte aligned (two per item for L = 8 floats, one for L = 4
// floats or L = 8 halves), element accesses otherwise -- so an offset pointer, or halves in place of the floats
// they convert to, change no bit.
//   sbn_stats_kernel<wave>      channels of <= 64 * PER items: a wave per channel, four channels per workgroup
//   sbn_stats_kernel<block>     <= 256 * PER items: a workgroup per channel
//   ... (split)                 above that a workgroup per chunk of 256 * PER items: (mean, M2 about the chunk's
//                               mean) -> the workspace; sbn_stats_merge_kernel, a wave per channel, merges them by
//                               Chan's rule in double in a fixed order
//   sbn_bwd_stats_kernel        the same three regimes; sbn_bwd_merge_kernel adds the partial sums in double
//   sbn_fwd_coef_kernel / sbn_bwd_coef_kernel   a thread per channel: the combine over the ranks and the channel's
//                               coefficients -> the workspace; mean / var, dgamma / dbeta, moving_*
//   sbn_map_kernel              the element rules over the flat tensor, an item's channel by two divisions
// No floating-point atomics, no memset, no host read: every workspace word that is read was written by a kernel of
// the same call, and every grid depends on the shapes alone.
#include "common.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>
#include <initializer_list>
#include <type_traits>

namespace sd {
namespace {

constexpr int kSbnT = 256;
constexpr long kSbnMaxElems = 2147483647L;   // element indices are 32-bit inside the kernels
constexpr int kSbnMinChunk = kSbnT * 8;      // elements of the smallest chunk (L = 1): bounds the partials

template <int L> constexpr int sbn_per() { return L == 8 ? 4 : 8; }   // resident items per thread
template <int L> constexpr int sbn_map_per() { return L == 8 ? 2 : 4; }

struct SbnArgs {
  const void* x;
  const void* dy;          // backward
  void* y;                 // forward: y; backward: dx
  const float* mean_in;    // backward statistics
  float* out;              // (2, C): part / bpart
  float2* partial;         // (C, S), split path
  const float4* coef;      // (C), the element kernels
  const float* gamma;      // inference
  const float* beta;
  const float* mmean;
  const float* mvar;
  unsigned N, C, HxW;
  unsigned ipr, ipc;       // items per row / per channel
  unsigned S;              // chunks per channel
  unsigned chunk;          // items per chunk
  unsigned items;          // items of the whole tensor
  float n;                 // N * HxW
  float eps;
  int fix_gamma;
};

template <int L> struct SbnItem { float v[L]; };
struct alignas(16) SbnH8 { _Float16 h[8]; };

// how an item of L elements of type T is moved; VEC: by 16-byte accesses
template <typename T, int L, bool VEC>
struct SbnIO {
  static_assert(!VEC || L * sizeof(T) >= 16, "a 16-byte item");
  using Item = SbnItem<L>;
  static __device__ __forceinline__ Item ld(const T* p) {
    Item r;
    if constexpr (VEC && sizeof(T) == 4) {
#pragma unroll
      for (int q = 0; q < L / 4; ++q) {
        const float4 f = reinterpret_cast<const float4*>(p)[q];
        r.v[4 * q] = f.x; r.v[4 * q + 1] = f.y; r.v[4 * q + 2] = f.z; r.v[4 * q + 3] = f.w;
      }
    } else if constexpr (VEC) {
      const SbnH8 h = *reinterpret_cast<const SbnH8*>(p);
#pragma unroll
      for (int k = 0; k < 8; ++k) r.v[k] = (float)h.h[k];
    } else {
#pragma unroll
      for (int k = 0; k < L; ++k) r.v[k] = (float)p[k];
    }
    return r;
  }
  static __device__ __forceinline__ void st(T* p, const Item& r) {
    if constexpr (VEC && sizeof(T) == 4) {
#pragma unroll
      for (int q = 0; q < L / 4; ++q)
        reinterpret_cast<float4*>(p)[q] = make_float4(r.v[4 * q], r.v[4 * q + 1], r.v[4 * q + 2], r.v[4 * q + 3]);
    } else if constexpr (VEC) {
      SbnH8 h;
#pragma unroll
      for (int k = 0; k < 8; ++k) h.h[k] = (_Float16)r.v[k];
      *reinterpret_cast<SbnH8*>(p) = h;
    } else {
#pragma unroll
      for (int k = 0; k < L; ++k) p[k] = (T)r.v[k];
    }
  }
};

// the sum of an item's L terms, pairwise
template <int L>
__device__ __forceinline__ float sbn_tree(float (&f)[L]) {
#pragma unroll
  for (int w = 1; w < L; w *= 2)
#pragma unroll
    for (int j = 0; j < L; j += 2 * w) f[j] = f[j] + f[j + w];
  return f[0];
}
template <int L>
__device__ __forceinline__ float sbn_hsum(const SbnItem<L>& a) {
  float f[L];
#pragma unroll
  for (int k = 0; k < L; ++k) f[k] = a.v[k];
  return sbn_tree<L>(f);
}
template <int L>
__device__ __forceinline__ float sbn_sq(const SbnItem<L>& a, float m) {
  float f[L];
#pragma unroll
  for (int k = 0; k < L; ++k) {
    const float d = a.v[k] - m;
    f[k] = d * d;
  }
  return sbn_tree<L>(f);
}
template <int L>
__device__ __forceinline__ float sbn_dot(const SbnItem<L>& g, const SbnItem<L>& x, float m) {
  float f[L];
#pragma unroll
  for (int k = 0; k < L; ++k) f[k] = g.v[k] * (x.v[k] - m);
  return sbn_tree<L>(f);
}

// sum over the TG threads that share a channel (chunk); `slot`: four floats of LDS of its own
template <int TG>
__device__ __forceinline__ float sbn_group_sum(float v, float* slot) {
  if constexpr (TG == kWave) return wave_sum_f32(v);
  else return block_sum_f32<TG, false>(v, slot);
}

// element index of item i of chunk-local order: item j of channel c lies in row n = j / ipr
__device__ __forceinline__ size_t sbn_item_at(const SbnArgs& a, unsigned c, unsigned j, unsigned L) {
  const unsigned n = j / a.ipr, r = j - n * a.ipr;
  return ((size_t)n * a.C + c) * a.HxW + (size_t)r * L;
}

template <typename T, int L, bool VEC, int TG>
__global__ __launch_bounds__(kSbnT) void sbn_stats_kernel(SbnArgs a) {
  using IO = SbnIO<T, L, VEC>;
  constexpr int PER = sbn_per<L>();
  __shared__ float red[8];
  const unsigned t = threadIdx.x % TG;
  const unsigned u = blockIdx.x * (kSbnT / TG) + threadIdx.x / TG;
  if (u >= a.C * a.S) return;   // (a whole wave, TG == 64; never taken for TG == 256)
  const unsigned c = u / a.S, s = u - c * a.S;
  const unsigned first = s * (unsigned)(TG * PER);
  const unsigned cnt = a.ipc - first < (unsigned)(TG * PER) ? a.ipc - first : (unsigned)(TG * PER);
  const T* x = static_cast<const T*>(a.x);
  SbnItem<L> v[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < cnt) {
      v[k] = IO::ld(x + sbn_item_at(a, c, first + i, L));
    } else {
#pragma unroll
      for (int q = 0; q < L; ++q) v[k].v[q] = 0.f;
    }
  }
  float sm = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) sm += sbn_hsum<L>(v[k]);
  const float mean = sbn_group_sum<TG>(sm, red) / (float)(cnt * L);
  float q2 = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (t + k * TG < cnt) q2 += sbn_sq<L>(v[k], mean);
  const float m2 = sbn_group_sum<TG>(q2, red + 4);
  if (t == 0) {
    if (a.S == 1) {
      a.out[c] = mean;
      a.out[a.C + c] = m2 / a.n;
    } else {
      a.partial[u] = make_float2(mean, m2);
    }
  }
}

// Chan, Golub, LeVeque: (na, ma, Ma) + (nb, mb, Mb)
__device__ __forceinline__ void sbn_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; Ma = Mb; return; }
  const double n = na + nb, d = mb - ma;
  ma = ma + d * (nb / n);
  Ma = Ma + Mb + d * d * (na * nb / n);
  na = n;
}

// a wave per channel: lanes stride its S partials, then a fixed tree over the lanes
__global__ __launch_bounds__(kSbnT) void sbn_stats_merge_kernel(SbnArgs a, unsigned L) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned c = blockIdx.x * (kSbnT / kWave) + threadIdx.x / kWave;
  if (c >= a.C) return;
  const float2* p = a.partial + (size_t)c * a.S;
  double n = 0.0, m = 0.0, M = 0.0;
  for (unsigned s = lane; s < a.S; s += kWave) {
    const unsigned first = s * a.chunk;
    const unsigned cnt = a.ipc - first < a.chunk ? a.ipc - first : a.chunk;
    const float2 v = p[s];
    sbn_merge(n, m, M, (double)cnt * (double)L, (double)v.x, (double)v.y);
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double nb = __shfl_down(n, off), mb = __shfl_down(m, off), Mb = __shfl_down(M, off);
    if (lane + off < (unsigned)kWave) sbn_merge(n, m, M, nb, mb, Mb);
  }
  if (lane == 0) {
    a.out[c] = (float)m;
    a.out[a.C + c] = (float)(M / n);
  }
}

template <typename T, int L, bool VEC, int TG>
__global__ __launch_bounds__(kSbnT) void sbn_bwd_stats_kernel(SbnArgs a) {
  using IO = SbnIO<T, L, VEC>;
  constexpr int PER = sbn_per<L>();
  __shared__ float red[8];
  const unsigned t = threadIdx.x % TG;
  const unsigned u = blockIdx.x * (kSbnT / TG) + threadIdx.x / TG;
  if (u >= a.C * a.S) return;
  const unsigned c = u / a.S, s = u - c * a.S;
  const unsigned first = s * (unsigned)(TG * PER);
  const unsigned cnt = a.ipc - first < (unsigned)(TG * PER) ? a.ipc - first : (unsigned)(TG * PER);
  const T* x = static_cast<const T*>(a.x);
  const T* dy = static_cast<const T*>(a.dy);
  const float mean = a.mean_in[c];
  SbnItem<L> xv[PER], gv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < cnt) {
      const size_t e = sbn_item_at(a, c, first + i, L);
      xv[k] = IO::ld(x + e);
      gv[k] = IO::ld(dy + e);
    }
  }
  float sg = 0.f, sp = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (t + k * TG < cnt) {
      sg += sbn_hsum<L>(gv[k]);
      sp += sbn_dot<L>(gv[k], xv[k], mean);
    }
  sg = sbn_group_sum<TG>(sg, red);
  sp = sbn_group_sum<TG>(sp, red + 4);
  if (t == 0) {
    if (a.S == 1) {
      a.out[c] = sg;
      a.out[a.C + c] = sp;
    } else {
      a.partial[u] = make_float2(sg, sp);
    }
  }
}

// a wave per channel: lanes stride its S partial sums, in double, then a fixed tree over the lanes
__global__ __launch_bounds__(kSbnT) void sbn_bwd_merge_kernel(SbnArgs a) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned c = blockIdx.x * (kSbnT / kWave) + threadIdx.x / kWave;
  if (c >= a.C) return;
  const float2* p = a.partial + (size_t)c * a.S;
  double sg = 0.0, sp = 0.0;
  for (unsigned s = lane; s < a.S; s += kWave) {
    const float2 v = p[s];
    sg += (double)v.x;
    sp += (double)v.y;
  }
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double gb = __shfl_down(sg, off), pb = __shfl_down(sp, off);
    if (lane + off < (unsigned)kWave) { sg += gb; sp += pb; }
  }
  if (lane == 0) {
    a.out[c] = (float)sg;
    a.out[a.C + c] = (float)sp;
  }
}

// a thread per channel: the combine over the ranks (double, rank order), mean / var, the coefficients of the
// element rule (mean, inv, g, beta)
__global__ __launch_bounds__(kSbnT) void sbn_fwd_coef_kernel(const float* parts, int W, const float* gamma,
                                                             const float* beta, float* mean, float* var, float4* coef,
                                                             unsigned C, float eps, int fix_gamma) {
  const unsigned c = blockIdx.x * kSbnT + threadIdx.x;
  if (c >= C) return;
  double sm = 0.0;
  for (int r = 0; r < W; ++r) sm += (double)parts[((size_t)r * 2) * C + c];
  const double m = sm / (double)W;
  double sv = 0.0;
  for (int r = 0; r < W; ++r) {
    const double d = (double)parts[((size_t)r * 2) * C + c] - m;
    sv += (double)parts[((size_t)r * 2 + 1) * C + c] + d * d;
  }
  const double v = sv / (double)W;
  const float m32 = (float)m, v32 = (float)v;
  mean[c] = m32;
  var[c] = v32;
  const float inv = 1.0f / sqrtf(v32 + eps);
  coef[c] = make_float4(m32, inv, fix_gamma ? 1.0f : gamma[c], beta[c]);
}

// a thread per channel: the sums over the ranks, (a, b, c, mean) of the element rule, the parameter gradients of
// this rank and the moving statistics
__global__ __launch_bounds__(kSbnT) void sbn_bwd_coef_kernel(const float* bparts, int W, int rank, const float* mean,
                                                             const float* var, const float* gamma, float* dgamma,
                                                             float* dbeta, float* mmean, float* mvar, float momentum,
                                                             float4* coef, unsigned C, double wn, float eps,
                                                             int fix_gamma) {
  const unsigned c = blockIdx.x * kSbnT + threadIdx.x;
  if (c >= C) return;
  double SG = 0.0, SP = 0.0;
  for (int r = 0; r < W; ++r) {
    SG += (double)bparts[((size_t)r * 2) * C + c];
    SP += (double)bparts[((size_t)r * 2 + 1) * C + c];
  }
  const float sg = (float)(SG / wn), sp = (float)(SP / wn);
  const float mu = mean[c], vr = var[c];
  const float g = fix_gamma ? 1.0f : gamma[c];
  const float inv = 1.0f / sqrtf(vr + eps);
  const float ka = g * inv;
  const float kb = -(g * sp) * ((inv * inv) * inv);
  const float kc = -(g * sg) * inv;
  coef[c] = make_float4(ka, kb, kc, mu);
  if (dgamma) {
    dbeta[c] = bparts[((size_t)rank * 2) * C + c];
    dgamma[c] = fix_gamma ? 0.0f : bparts[((size_t)rank * 2 + 1) * C + c] * inv;
  }
  if (mmean) {
    mmean[c] = mmean[c] * momentum + mu * (1.0f - momentum);
    mvar[c] = mvar[c] * momentum + vr * (1.0f - momentum);
  }
}

enum { kSbnFwd = 0, kSbnBwd = 1, kSbnInfer = 2 };

// the element rules over the flat tensor: item e lies in plane e / ipr, channel plane % C
template <typename T, int L, bool VEC, int KIND>
__global__ __launch_bounds__(kSbnT) void sbn_map_kernel(SbnArgs a) {
  using IO = SbnIO<T, L, VEC>;
  constexpr int U = sbn_map_per<L>();
  const T* x = static_cast<const T*>(a.x);
  const T* dy = static_cast<const T*>(a.dy);
  T* y = static_cast<T*>(a.y);
  const unsigned e0 = blockIdx.x * (unsigned)(kSbnT * U) + threadIdx.x;
  SbnItem<L> xv[U], gv[U];
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const unsigned e = e0 + k * kSbnT;
    if (e < a.items) {
      xv[k] = IO::ld(x + (size_t)e * L);
      if (KIND == kSbnBwd) gv[k] = IO::ld(dy + (size_t)e * L);
    }
  }
#pragma unroll
  for (int k = 0; k < U; ++k) {
    const unsigned e = e0 + k * kSbnT;
    if (e >= a.items) continue;
    const unsigned plane = e / a.ipr;
    const unsigned c = plane % a.C;
    SbnItem<L> r;
    if (KIND == kSbnFwd) {
      const float4 k4 = a.coef[c];   // mean, inv, g, beta
#pragma unroll
      for (int q = 0; q < L; ++q) r.v[q] = (k4.z * (xv[k].v[q] - k4.x)) * k4.y + k4.w;
    } else if (KIND == kSbnBwd) {
      const float4 k4 = a.coef[c];   // a, b, c, mean
#pragma unroll
      for (int q = 0; q < L; ++q) r.v[q] = (gv[k].v[q] * k4.x + k4.y * (xv[k].v[q] - k4.w)) + k4.z;
    } else {
      const float g = a.fix_gamma ? 1.0f : a.gamma[c];
      const float sd_ = sqrtf(a.mvar[c] + a.eps);
      const float ka = g / sd_;
      const float kb = a.beta[c] - (g * a.mmean[c]) / sd_;
#pragma unroll
      for (int q = 0; q < L; ++q) r.v[q] = ka * xv[k].v[q] + kb;
    }
    IO::st(y + (size_t)e * L, r);
  }
}

// ---------------------------------------------------------------------------------------------- host --
struct SbnPlan {
  long n;            // N * HxW
  int L;
  unsigned ipr, ipc, items;
  size_t coef_bytes, partial_bytes;
};

static int sbn_plan(int N, int C, long HxW, SbnPlan* p, bool* empty) {
  SD_REQUIRE(N >= 0 && C >= 0 && HxW >= 0, "negative dimension (N=%d C=%d HxW=%ld)", N, C, HxW);
  const long nc = (long)N * C;
  *empty = nc == 0 || HxW == 0;
  if (*empty) return SD_OK;
  if (HxW > kSbnMaxElems / nc)
    return fail(SD_ERR_UNSUPPORTED, "N*C*HxW = %ld x %ld elements exceed the limit %ld", nc, HxW, kSbnMaxElems);
  p->n = (long)N * HxW;
  p->L = HxW % 8 == 0 ? 8 : HxW % 4 == 0 ? 4 : 1;
  p->ipr = (unsigned)(HxW / p->L);
  p->ipc = (unsigned)(p->n / p->L);
  p->items = (unsigned)(nc * HxW / p->L);
  p->coef_bytes = (size_t)C * sizeof(float4);
  // sized for the smallest chunk (L = 1) whatever path is taken
  p->partial_bytes = (size_t)C * (size_t)((p->n + kSbnMinChunk - 1) / kSbnMinChunk) * sizeof(float2);
  return SD_OK;
}

struct SbnWs {
  float4* coef;
  float2* partial;
  size_t need;
};
static SbnWs sbn_carve(const SbnPlan& p, void* workspace) {
  WsCarver w(workspace);
  SbnWs r;
  r.coef = w.take<float4>(p.coef_bytes);
  r.partial = w.take<float2>(p.partial_bytes);
  r.need = w.need();
  return r;
}
static size_t sbn_need(const SbnPlan& p) { return 256 + sbn_carve(p, nullptr).need; }

static bool sbn_aligned(size_t to, std::initializer_list<const void*> ps) {
  for (const void* q : ps)
    if ((uintptr_t)q % to) return false;
  return true;
}

static void sbn_fill(SbnArgs& a, const SbnPlan& p, int N, int C, long HxW) {
  a.N = (unsigned)N; a.C = (unsigned)C; a.HxW = (unsigned)HxW;
  a.ipr = p.ipr; a.ipc = p.ipc; a.items = p.items;
  a.n = (float)p.n;
}

template <typename T> static const char* sbn_tn() { return sizeof(T) == 4 ? "f32" : "f16"; }

// calls f with SbnIO's <L, VEC> as integral constants
template <typename T, typename F>
static void sbn_with_io(int L, bool vec, F&& f) {
  using std::integral_constant;
  if (L == 8) {
    if (vec) f(integral_constant<int, 8>{}, integral_constant<bool, true>{});
    else f(integral_constant<int, 8>{}, integral_constant<bool, false>{});
  } else if (L == 4) {
    if constexpr (sizeof(T) == 4) {
      if (vec) { f(integral_constant<int, 4>{}, integral_constant<bool, true>{}); return; }
    }
    f(integral_constant<int, 4>{}, integral_constant<bool, false>{});   // (four halves are 8 bytes: element accesses)
  } else {
    f(integral_constant<int, 1>{}, integral_constant<bool, false>{});
  }
}

// the three regimes of the two reductions; BWD: sums of dy and dy * (x - mean), else mean and variance
template <typename T, bool BWD>
static void sbn_reduce(SbnArgs& a, const SbnPlan& p, bool vec, hipStream_t st) {
  sbn_with_io<T>(p.L, vec, [&](auto l, auto v) {
    constexpr int L = decltype(l)::value;
    constexpr bool VEC = decltype(v)::value;
    constexpr int PER = sbn_per<L>();
    const char* name = BWD ? "sbn_bwd_stats_kernel" : "sbn_stats_kernel";
    const char* mv = VEC ? "vec" : "narrow";
    if (a.ipc <= (unsigned)(kWave * PER)) {
      a.S = 1;
      a.chunk = kWave * PER;
      const dim3 grid(cdiv(a.C, kSbnT / kWave));
      if (BWD) hipLaunchKernelGGL((sbn_bwd_stats_kernel<T, L, VEC, kWave>), grid, dim3(kSbnT), 0, st, a);
      else hipLaunchKernelGGL((sbn_stats_kernel<T, L, VEC, kWave>), grid, dim3(kSbnT), 0, st, a);
      note_dispatch("sd::%s<%s,L%d,%s,wave>", name, sbn_tn<T>(), L, mv);
      return;
    }
    a.chunk = kSbnT * PER;
    a.S = (a.ipc + a.chunk - 1) / a.chunk;
    const dim3 grid(a.C * a.S);
    if (BWD) hipLaunchKernelGGL((sbn_bwd_stats_kernel<T, L, VEC, kSbnT>), grid, dim3(kSbnT), 0, st, a);
    else hipLaunchKernelGGL((sbn_stats_kernel<T, L, VEC, kSbnT>), grid, dim3(kSbnT), 0, st, a);
    if (a.S == 1) {
      note_dispatch("sd::%s<%s,L%d,%s,block>", name, sbn_tn<T>(), L, mv);
      return;
    }
    const dim3 mgrid(cdiv(a.C, kSbnT / kWave));
    if (BWD) hipLaunchKernelGGL(sbn_bwd_merge_kernel, mgrid, dim3(kSbnT), 0, st, a);
    else hipLaunchKernelGGL(sbn_stats_merge_kernel, mgrid, dim3(kSbnT), 0, st, a, (unsigned)L);
    note_dispatch("sd::%s<%s,L%d,%s,block> x %u chunks + sd::%s (split)", name, sbn_tn<T>(), L, mv, a.S,
                  BWD ? "sbn_bwd_merge_kernel" : "sbn_stats_merge_kernel");
  });
}

template <typename T, int KIND>
static void sbn_map(SbnArgs& a, const SbnPlan& p, bool vec, hipStream_t st, const char* lead) {
  sbn_with_io<T>(p.L, vec, [&](auto l, auto v) {
    constexpr int L = decltype(l)::value;
    constexpr bool VEC = decltype(v)::value;
    const int per = kSbnT * sbn_map_per<L>();
    hipLaunchKernelGGL((sbn_map_kernel<T, L, VEC, KIND>), dim3(cdiv(a.items, per)), dim3(kSbnT), 0, st, a);
    note_dispatch("%ssd::sbn_map_kernel<%s,L%d,%s,%s>", lead, sbn_tn<T>(), L, VEC ? "vec" : "narrow",
                  KIND == kSbnFwd ? "fwd" : KIND == kSbnBwd ? "bwd" : "infer");
  });
}

#define SBN_WORKSPACE(p, name)                                                                              \
  if (!(workspace && workspace_bytes >= sbn_need(p)))                                                       \
    return fail(SD_ERR_WORKSPACE, name " workspace too small: %zu < %zu bytes",                           \
                workspace ? workspace_bytes : (size_t)0, sbn_need(p))

template <typename T>
static int sbn_stats(const void* x, float* part, int N, int C, long HxW, void* workspace, size_t workspace_bytes,
                     void* stream) {
  SbnPlan p{};
  bool empty = false;
  if (int e = sbn_plan(N, C, HxW, &p, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(x && part, "null pointer");
  SD_REQUIRE(sbn_aligned(sizeof(T), {x}) && sbn_aligned(4, {part}), "a pointer is not aligned to its elements");
  SBN_WORKSPACE(p, "sync_bn_stats");
  SbnArgs a{};
  sbn_fill(a, p, N, C, HxW);
  a.x = x; a.out = part;
  a.partial = sbn_carve(p, workspace).partial;
  sbn_reduce<T, false>(a, p, sbn_aligned(16, {x}), (hipStream_t)stream);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int sbn_apply(const void* x, const float* parts, int W, const float* gamma, const float* beta, void* y,
                     float* mean, float* var, int N, int C, long HxW, float eps, int fix_gamma, void* workspace,
                     size_t workspace_bytes, void* stream) {
  SbnPlan p{};
  bool empty = false;
  if (int e = sbn_plan(N, C, HxW, &p, &empty)) return e;
  SD_REQUIRE(W >= 1, "W=%d ranks: at least one", W);
  if (empty) return SD_OK;
  SD_REQUIRE(x && parts && gamma && beta && y && mean && var, "null pointer");
  SD_REQUIRE(sbn_aligned(sizeof(T), {x, y}) && sbn_aligned(4, {parts, gamma, beta, mean, var}),
             "a pointer is not aligned to its elements");
  SBN_WORKSPACE(p, "sync_bn_apply");
  hipStream_t st = (hipStream_t)stream;
  const SbnWs ws = sbn_carve(p, workspace);
  hipLaunchKernelGGL(sbn_fwd_coef_kernel, dim3(cdiv(C, kSbnT)), dim3(kSbnT), 0, st, parts, W, gamma, beta, mean, var,
                     ws.coef, (unsigned)C, eps, fix_gamma);
  SbnArgs a{};
  sbn_fill(a, p, N, C, HxW);
  a.x = x; a.y = y; a.coef = ws.coef;
  sbn_map<T, kSbnFwd>(a, p, sbn_aligned(16, {x, y}), st, "sd::sbn_fwd_coef_kernel + ");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int sbn_infer(const void* x, const float* gamma, const float* beta, const float* mmean, const float* mvar,
                     void* y, int N, int C, long HxW, float eps, int fix_gamma, void* stream) {
  SbnPlan p{};
  bool empty = false;
  if (int e = sbn_plan(N, C, HxW, &p, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(x && gamma && beta && mmean && mvar && y, "null pointer");
  SD_REQUIRE(sbn_aligned(sizeof(T), {x, y}) && sbn_aligned(4, {gamma, beta, mmean, mvar}),
             "a pointer is not aligned to its elements");
  SbnArgs a{};
  sbn_fill(a, p, N, C, HxW);
  a.x = x; a.y = y; a.gamma = gamma; a.beta = beta; a.mmean = mmean; a.mvar = mvar;
  a.eps = eps; a.fix_gamma = fix_gamma;
  sbn_map<T, kSbnInfer>(a, p, sbn_aligned(16, {x, y}), (hipStream_t)stream, "");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int sbn_bwd_stats(const void* dy, const void* x, const float* mean, float* bpart, int N, int C, long HxW,
                         void* workspace, size_t workspace_bytes, void* stream) {
  SbnPlan p{};
  bool empty = false;
  if (int e = sbn_plan(N, C, HxW, &p, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(dy && x && mean && bpart, "null pointer");
  SD_REQUIRE(sbn_aligned(sizeof(T), {dy, x}) && sbn_aligned(4, {mean, bpart}),
             "a pointer is not aligned to its elements");
  SBN_WORKSPACE(p, "sync_bn_bwd_stats");
  SbnArgs a{};
  sbn_fill(a, p, N, C, HxW);
  a.x = x; a.dy = dy; a.mean_in = mean; a.out = bpart;
  a.partial = sbn_carve(p, workspace).partial;
  sbn_reduce<T, true>(a, p, sbn_aligned(16, {dy, x}), (hipStream_t)stream);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int sbn_bwd_apply(const void* dy, const void* x, const float* mean, const float* var, const float* gamma,
                         const float* bparts, int W, int rank, void* dx, float* dgamma, float* dbeta, float* mmean,
                         float* mvar, float momentum, int N, int C, long HxW, float eps, int fix_gamma,
                         void* workspace, size_t workspace_bytes, void* stream) {
  SbnPlan p{};
  bool empty = false;
  if (int e = sbn_plan(N, C, HxW, &p, &empty)) return e;
  SD_REQUIRE(W >= 1, "W=%d ranks: at least one", W);
  SD_REQUIRE(rank >= 0 && rank < W, "rank=%d is outside 0..%d", rank, W - 1);
  SD_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "dgamma and dbeta must be given, or be NULL, together");
  SD_REQUIRE((mmean == nullptr) == (mvar == nullptr),
             "moving_mean and moving_var must be given, or be NULL, together");
  if (empty) return SD_OK;   // (the sums are over nothing; like every empty call, nothing is written)
  SD_REQUIRE(dy && x && mean && var && gamma && bparts && dx, "null pointer");
  SD_REQUIRE(sbn_aligned(sizeof(T), {dy, x, dx}) &&
                 sbn_aligned(4, {mean, var, gamma, bparts, dgamma, dbeta, mmean, mvar}),
             "a pointer is not aligned to its elements");
  SBN_WORKSPACE(p, "sync_bn_bwd_apply");
  hipStream_t st = (hipStream_t)stream;
  const SbnWs ws = sbn_carve(p, workspace);
  hipLaunchKernelGGL(sbn_bwd_coef_kernel, dim3(cdiv(C, kSbnT)), dim3(kSbnT), 0, st, bparts, W, rank, mean, var, gamma,
                     dgamma, dbeta, mmean, mvar, momentum, ws.coef, (unsigned)C, (double)W * (double)p.n, eps,
                     fix_gamma);
  SbnArgs a{};
  sbn_fill(a, p, N, C, HxW);
  a.x = x; a.dy = dy; a.y = dx; a.coef = ws.coef;
  sbn_map<T, kSbnBwd>(a, p, sbn_aligned(16, {dy, x, dx}), st, "sd::sbn_bwd_coef_kernel + ");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_sync_bn_workspace_bytes(int N, int C, long HxW) {
  SbnPlan p{};
  bool empty = false;
  if (sbn_plan(N, C, HxW, &p, &empty) != SD_OK || empty) return 256;
  return sbn_need(p);
}

extern "C" int sd_sync_bn_stats(const float* x, float* part, int N, int C, long HxW, void* workspace,
                                size_t workspace_bytes, void* stream) {
  return sbn_stats<float>(x, part, N, C, HxW, workspace, workspace_bytes, stream);
}
extern "C" int sd_sync_bn_stats_f16(const void* x, float* part, int N, int C, long HxW, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  return sbn_stats<_Float16>(x, part, N, C, HxW, workspace, workspace_bytes, stream);
}
extern "C" int sd_sync_bn_apply(const float* x, const float* parts, int W, const float* gamma, const float* beta,
                                float* y, float* mean, float* var, int N, int C, long HxW, float eps, int fix_gamma,
                                void* workspace, size_t workspace_bytes, void* stream) {
  return sbn_apply<float>(x, parts, W, gamma, beta, y, mean, var, N, C, HxW, eps, fix_gamma, workspace,
                          workspace_bytes, stream);
}
extern "C" int sd_sync_bn_apply_f16(const void* x, const float* parts, int W, const float* gamma, const float* beta,
                                    void* y, float* mean, float* var, int N, int C, long HxW, float eps,
                                    int fix_gamma, void* workspace, size_t workspace_bytes, void* stream) {
  return sbn_apply<_Float16>(x, parts, W, gamma, beta, y, mean, var, N, C, HxW, eps, fix_gamma, workspace,
                             workspace_bytes, stream);
}
extern "C" int sd_sync_bn_infer_fwd(const float* x, const float* gamma, const float* beta, const float* moving_mean,
                                    const float* moving_var, float* y, int N, int C, long HxW, float eps,
                                    int fix_gamma, void* stream) {
  return sbn_infer<float>(x, gamma, beta, moving_mean, moving_var, y, N, C, HxW, eps, fix_gamma, stream);
}
extern "C" int sd_sync_bn_infer_fwd_f16(const void* x, const float* gamma, const float* beta,
                                        const float* moving_mean, const float* moving_var, void* y, int N, int C,
                                        long HxW, float eps, int fix_gamma, void* stream) {
  return sbn_infer<_Float16>(x, gamma, beta, moving_mean, moving_var, y, N, C, HxW, eps, fix_gamma, stream);
}
extern "C" int sd_sync_bn_bwd_stats(const float* dy, const float* x, const float* mean, float* bpart, int N, int C,
                                    long HxW, void* workspace, size_t workspace_bytes, void* stream) {
  return sbn_bwd_stats<float>(dy, x, mean, bpart, N, C, HxW, workspace, workspace_bytes, stream);
}
extern "C" int sd_sync_bn_bwd_stats_f16(const void* dy, const void* x, const float* mean, float* bpart, int N, int C,
                                        long HxW, void* workspace, size_t workspace_bytes, void* stream) {
  return sbn_bwd_stats<_Float16>(dy, x, mean, bpart, N, C, HxW, workspace, workspace_bytes, stream);
}
extern "C" int sd_sync_bn_bwd_apply(const float* dy, const float* x, const float* mean, const float* var,
                                    const float* gamma, const float* bparts, int W, int rank, float* dx,
                                    float* dgamma, float* dbeta, float* moving_mean, float* moving_var,
                                    float momentum, int N, int C, long HxW, float eps, int fix_gamma,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  return sbn_bwd_apply<float>(dy, x, mean, var, gamma, bparts, W, rank, dx, dgamma, dbeta, moving_mean, moving_var,
                              momentum, N, C, HxW, eps, fix_gamma, workspace, workspace_bytes, stream);
}
extern "C" int sd_sync_bn_bwd_apply_f16(const void* dy, const void* x, const float* mean, const float* var,
                                        const float* gamma, const float* bparts, int W, int rank, void* dx,
                                        float* dgamma, float* dbeta, float* moving_mean, float* moving_var,
                                        float momentum, int N, int C, long HxW, float eps, int fix_gamma,
                                        void* workspace, size_t workspace_bytes, void* stream) {
  return sbn_bwd_apply<_Float16>(dy, x, mean, var, gamma, bparts, W, rank, dx, dgamma, dbeta, moving_mean,
                                 moving_var, momentum, N, C, HxW, eps, fix_gamma, workspace, workspace_bytes, stream);
}
