// The statistics toolkit of the normalisation kernels: GroupNorm, SyncBatchNorm, pyramid batch norm,
// and the 16-byte item, head length and host checks that the merged-BN affine, the SE block, the FPN top-down pathway
// and Quantization_int8 share with them.  These kernels promise bits, and the rank combine of pyramid batch norm IS
// the one of SyncBatchNorm, so an operator file calls these and holds no copy.  (group_sum_f32 is in wg_common.h.)
#pragma once
#include "wg_common.h"
#include <math.h>
#include <initializer_list>

namespace sd {

// ------------------------------------------------------------------------------------------------ items --
// 16 bytes of T on a 16-byte boundary: one access
template <typename T>
struct alignas(16) Vec16 {
  static constexpr int N = 16 / sizeof(T);
  T e[N];
};
template <typename T>
__device__ __forceinline__ Vec16<T> vec16_ld(const T* p) { return *reinterpret_cast<const Vec16<T>*>(p); }
template <typename T>
__device__ __forceinline__ void vec16_st(T* p, const Vec16<T>& v) { *reinterpret_cast<Vec16<T>*>(p) = v; }

// an item of L elements of T at a 16-byte boundary <-> L floats, by 16-byte accesses
template <typename T, int L>
__device__ __forceinline__ void vec16_ld_f32(const T* p, float (&v)[L]) {
  constexpr int V = Vec16<T>::N;
  static_assert(L % V == 0, "whole 16-byte accesses");
#pragma unroll
  for (int q = 0; q < L / V; ++q) {
    const Vec16<T> a = vec16_ld(p + q * V);
#pragma unroll
    for (int k = 0; k < V; ++k) v[q * V + k] = (float)a.e[k];
  }
}
template <typename T, int L>
__device__ __forceinline__ void vec16_st_f32(T* p, const float (&v)[L]) {
  constexpr int V = Vec16<T>::N;
  static_assert(L % V == 0, "whole 16-byte accesses");
#pragma unroll
  for (int q = 0; q < L / V; ++q) {
    Vec16<T> a;
#pragma unroll
    for (int k = 0; k < V; ++k) a.e[k] = (T)v[q * V + k];
    *reinterpret_cast<Vec16<T>*>(p + q * V) = a;
  }
}

// elements of a run of `len` in front of its first 16-byte boundary (p is aligned to its elements)
template <typename T, typename I>
__host__ __device__ __forceinline__ I head_to_16(const T* p, I len) {
  const I h = (I)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / (unsigned)sizeof(T));
  return h < len ? h : len;
}

// ------------------------------------------------------------------------------------------------- sums --
// the sum of an item's L terms, pairwise (f is used up)
template <int L>
__device__ __forceinline__ float tree_sum(float (&f)[L]) {
#pragma unroll
  for (int w = 1; w < L; w *= 2)
#pragma unroll
    for (int j = 0; j < L; j += 2 * w) f[j] = f[j] + f[j + w];
  return f[0];
}

// Chan, Golub, LeVeque for unequal counts: (na, ma, Ma) + (nb, mb, Mb)
__device__ __forceinline__ void chan_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; Ma = Mb; return; }
  const double n = na + nb, d = mb - ma;
  ma = ma + d * (nb / n);
  Ma = Ma + Mb + d * d * (na * nb / n);
  na = n;
}

// the lanes of a wave in a fixed tree: lane l takes lane l + off, off = 32 .. 1; lane 0 ends with the whole wave
__device__ __forceinline__ void wave_tree_chan(unsigned lane, double& n, double& m, double& M) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double nb = __shfl_down(n, off), mb = __shfl_down(m, off), Mb = __shfl_down(M, off);
    if (lane + off < (unsigned)kWave) chan_merge(n, m, M, nb, mb, Mb);
  }
}
__device__ __forceinline__ double2 wave_tree_sum2(unsigned lane, double a, double b) {
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double ab = __shfl_down(a, off), bb = __shfl_down(b, off);
    if (lane + off < (unsigned)kWave) { a += ab; b += bb; }
  }
  return make_double2(a, b);
}

// ------------------------------------------------------------------- the rank combine of the batch norms --
// Launched by sync_bn.hip and pyramid_bn.hip with THREADS = their workgroup size (a template, so that a file that
// launches none holds none; static, so that each of the two holds its own).
// a wave per channel: lanes stride its S partial sums (sum dy, sum dy * (x - mean)), in double, then the tree
template <int THREADS>
static __global__ __launch_bounds__(THREADS) void bn_bwd_merge_kernel(const float2* partial, float* out, unsigned C,
                                                                      unsigned S) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned c = blockIdx.x * (THREADS / kWave) + threadIdx.x / kWave;
  if (c >= C) return;
  const float2* p = partial + (size_t)c * S;
  double sg = 0.0, sp = 0.0;
  for (unsigned s = lane; s < S; s += kWave) {
    const float2 v = p[s];
    sg += (double)v.x;
    sp += (double)v.y;
  }
  const double2 t = wave_tree_sum2(lane, sg, sp);
  if (lane == 0) {
    out[c] = (float)t.x;
    out[C + c] = (float)t.y;
  }
}

// a thread per channel: the combine over the ranks (double, rank order), mean / var, the coefficients of the
// element rule (mean, inv, g, beta)
template <int THREADS>
static __global__ __launch_bounds__(THREADS) void bn_fwd_coef_kernel(const float* parts, int W, const float* gamma,
                                                                     const float* beta, float* mean, float* var,
                                                                     float4* coef, unsigned C, float eps,
                                                                     int fix_gamma) {
  const unsigned c = blockIdx.x * THREADS + threadIdx.x;
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
// this rank and the moving statistics; coef2, where not null, takes the forward's coefficients (beta is read for it)
template <int THREADS>
static __global__ __launch_bounds__(THREADS) void bn_bwd_coef_kernel(const float* bparts, int W, int rank,
                                                                     const float* mean, const float* var,
                                                                     const float* gamma, const float* beta,
                                                                     float* dgamma, float* dbeta, float* mmean,
                                                                     float* mvar, float momentum, float4* coef,
                                                                     float4* coef2, unsigned C, double wn, float eps,
                                                                     int fix_gamma) {
  const unsigned c = blockIdx.x * THREADS + threadIdx.x;
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
  if (coef2) coef2[c] = make_float4(mu, inv, g, beta[c]);
  if (dgamma) {
    dbeta[c] = bparts[((size_t)rank * 2) * C + c];
    dgamma[c] = fix_gamma ? 0.0f : bparts[((size_t)rank * 2 + 1) * C + c] * inv;
  }
  if (mmean) {
    mmean[c] = mmean[c] * momentum + mu * (1.0f - momentum);
    mvar[c] = mvar[c] * momentum + vr * (1.0f - momentum);
  }
}

// ------------------------------------------------------------------------------------------------- host --
// every pointer is a multiple of `to` (a null one is)
static inline bool ptrs_aligned(size_t to, std::initializer_list<const void*> ps) {
  for (const void* q : ps)
    if ((uintptr_t)q % to) return false;
  return true;
}

// the element type as the dispatch note spells it
template <typename T> static const char* elem_type_name() { return sizeof(T) == 4 ? "f32" : "f16"; }

// SD_OK, or entry point `name`'s error for a workspace below `need` bytes
static inline int workspace_check(const void* workspace, size_t workspace_bytes, size_t need, const char* name) {
  if (workspace && workspace_bytes >= need) return SD_OK;
  return fail(SD_ERR_WORKSPACE, "%s workspace too small: %zu < %zu bytes", name,
              workspace ? workspace_bytes : (size_t)0, need);
}

}  // namespace sd
