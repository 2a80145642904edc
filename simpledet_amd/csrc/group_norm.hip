// _contrib_GroupNorm forward and backward for gfx950, fp32, NCHW.
//
// The reference (operator_cxx/contrib/group_norm.cu:71-298, group_norm_helper.cu:36-63,258-268) spends five
// launches: Moments + InvStd + the normalising kernel forward (X read twice), ComputeInternalGradients +
// GroupNormBackward + GammaBetaBackward backward (dY and X read three times).  A group (n, g) is ONE contiguous
// span of D * HxW floats (D = C / G), so the whole operator is a reduction over contiguous spans followed by an
// element rule.  An "item" below is four floats (HxW % 4 == 0: an item then lies inside one channel; moved
// by one 16-byte access when every data pointer is 16-byte aligned, by 4-byte accesses otherwise) or one float
// (HxW % 4 != 0: 7x7 = 49, 25x42 = 1050).
//
// Small groups (the heads: a group fits in the registers of a wave or a workgroup) -- one launch each way,
// X (and dY) read once, Y (dX) written once:
//   gn_fwd_small   the group's items sit in registers; sum -> mu; sum (x - mu)^2 -> rsig (the variance ABOUT THE
//                  MEAN, the one deliberate departure from the reference's E[x^2] - mu^2); y from the registers.
//                  <64, 8>: a wave per group, four groups per workgroup, no barrier; <256, 16>: a workgroup per group
//   gn_bwd_small   x and dy in registers; ds, db by one group reduction; dx from the registers.  For dgamma / dbeta
//                  the per-item sums go through LDS and come back summed per channel into the (N, C, 2) table
// Large groups (neck and backbone: 64 groups of 537 600 floats against 256 CUs) -- a group is split over workgroups:
//   gn_fwd_partial   a workgroup per chunk of 2048 items, resident in registers: (mean, M2) about the chunk's mean
//   gn_fwd_combine   a wave per group merges the partials by Chan's rule in double, in a fixed order -> mu, rsig
//   gn_fwd_apply     the element rule
//   gn_bwd_rows      per (n, c) row: sum dy * (x - mu), sum dy -> the (N, C, 2) table
//   gn_bwd_group     ds, db per group from its D table rows (a wave per group, lanes striding D, the butterfly)
//   gn_bwd_dx        the element rule
// Both:
//   gn_bwd_param     dgamma[c] = sum_n table[n, c, 0] * rsig[n, g], dbeta[c] = sum_n table[n, c, 1]
//
// The backward sums are taken about mu (sum dy * (x - mu), not sum dy * x): the reference's
// (db * mu - ds) is then -ds, without the cancellation, and dgamma's row sum is the reference's own
// per-element expression dy * (x - mu) up to the common factor rsig.
// Every reduction has a fixed order (a lane's serial sum over its items, the DPP butterfly, the four wave results
// left to right, the partials in index order): no floating-point atomics anywhere, two calls give equal bits.
// Every workspace word that is read was written by a kernel of the same call: nothing to clear, no memset node.
#include "common.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>
#include <type_traits>

namespace sd {

constexpr int kGnT = 256;
constexpr long kGnMaxElems = 2147483647L;   // element indices are 32-bit inside the kernels
constexpr int kGnWavePer = 8;               // items per lane, wave per group:      <= 512 items
constexpr int kGnBlockPerFwd = 16;          // items per thread, workgroup per group, forward:  <= 4096 items
constexpr int kGnBlockPerBwd = 8;           // ... backward (x AND dy are resident):            <= 2048 items
constexpr int kGnChunk = kGnT * 8;          // items per chunk of a split group (forward statistics)
constexpr int kGnApplyPer = 4;              // items per thread of the element kernels of the split path

struct GnArgs {
  const float* x;
  const float* dy;      // backward only
  const float* gamma;
  const float* beta;    // forward only
  const float* mu_in;   // backward only
  const float* rsig_in; // backward only
  float* y;             // forward: y; backward: dx
  float* mu;            // forward outputs
  float* rsig;
  float* table;         // backward: (N, C, 2), null when dgamma / dbeta are skipped on the small path
  float* gsum;          // backward, split path: (N * G, 2) = ds, db
  float2* part;         // forward, split path: (N * G, S) = (mean, M2) of every chunk
  unsigned NG, G, D, C;
  unsigned ipc, ipg;    // items per channel / per group
  unsigned S;           // workgroups per group of the split kernels
  float n;              // D * HxW
  float eps;
};

// How an item is moved.  kGnVec4: one 16-byte access.  kGnQuad: the same four-float items through 4-byte
// accesses (HxW % 4 == 0 but a pointer off its 16-byte boundary): the sums keep the order of kGnVec4, so an
// offset pointer changes no bit of any result.  kGnScalar: one float per item (HxW % 4 != 0).
enum { kGnScalar = 0, kGnVec4 = 1, kGnQuad = 2 };
// An element index the compiler knows nothing about: four accesses at such indices cannot be merged back into one
// 16-byte access (left alone, LLVM turns four adjacent 4-byte accesses into a dwordx4, which gfx950 accepts at
// any 4-byte boundary; kGnQuad exists to issue none).  The pointer itself keeps its global address space.
__device__ __forceinline__ size_t gn_opaque(size_t j) {
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("" : "+v"(j));
#endif
  return j;
}
template <int MODE> struct GnIO;
template <> struct GnIO<kGnScalar> {
  using Item = float;
  static constexpr unsigned W = 1;
  static __device__ __forceinline__ float ld(const float* p, unsigned i) { return p[i]; }
  static __device__ __forceinline__ void st(float* p, unsigned i, float v) { p[i] = v; }
};
template <> struct GnIO<kGnVec4> {
  using Item = float4;
  static constexpr unsigned W = 4;
  static __device__ __forceinline__ float4 ld(const float* p, unsigned i) { return reinterpret_cast<const float4*>(p)[i]; }
  static __device__ __forceinline__ void st(float* p, unsigned i, const float4& v) { reinterpret_cast<float4*>(p)[i] = v; }
};
template <> struct GnIO<kGnQuad> {
  using Item = float4;
  static constexpr unsigned W = 4;
  static __device__ __forceinline__ float4 ld(const float* p, unsigned i) {
    const size_t j = 4 * (size_t)i;
    const float x = p[gn_opaque(j)], y = p[gn_opaque(j + 1)], z = p[gn_opaque(j + 2)], w = p[gn_opaque(j + 3)];
    return make_float4(x, y, z, w);
  }
  static __device__ __forceinline__ void st(float* p, unsigned i, const float4& v) {
    const size_t j = 4 * (size_t)i;
    p[gn_opaque(j)] = v.x;
    p[gn_opaque(j + 1)] = v.y;
    p[gn_opaque(j + 2)] = v.z;
    p[gn_opaque(j + 3)] = v.w;
  }
};
static const char* gn_mode_name(int mode) { return mode == kGnVec4 ? "vec4" : mode == kGnQuad ? "quad" : "scalar"; }

__device__ __forceinline__ float gn_hsum(float v) { return v; }
__device__ __forceinline__ float gn_hsum(const float4& v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float gn_sq(float v, float m) { const float d = v - m; return d * d; }
__device__ __forceinline__ float gn_sq(const float4& v, float m) {
  const float a = v.x - m, b = v.y - m, c = v.z - m, d = v.w - m;
  return (a * a + b * b) + (c * c + d * d);
}
__device__ __forceinline__ void gn_zero(float& v) { v = 0.f; }
__device__ __forceinline__ void gn_zero(float4& v) { v = make_float4(0.f, 0.f, 0.f, 0.f); }

// y = gamma * (x - mu) * rsig + beta, the reference's order (group_norm.cu:87-89)
__device__ __forceinline__ float gn_norm(float x, float mu, float rsig, float g, float b) {
  return g * (x - mu) * rsig + b;
}
__device__ __forceinline__ float4 gn_norm(const float4& x, float mu, float rsig, float g, float b) {
  return make_float4(gn_norm(x.x, mu, rsig, g, b), gn_norm(x.y, mu, rsig, g, b), gn_norm(x.z, mu, rsig, g, b),
                     gn_norm(x.w, mu, rsig, g, b));
}
// sum over an item of dy * (x - mu) and of dy
__device__ __forceinline__ float gn_dot(float dy, float x, float mu) { return dy * (x - mu); }
__device__ __forceinline__ float gn_dot(const float4& dy, const float4& x, float mu) {
  return (dy.x * (x.x - mu) + dy.y * (x.y - mu)) + (dy.z * (x.z - mu) + dy.w * (x.w - mu));
}
// dx = gamma * dy * rsig + (u - v) * denom, u = (-ds) * (x - mu) * rsig^3, v = db * rsig (group_norm.cu:152-158;
// ds here is the sum about mu, so the reference's (db * mu - ds) is -ds)
struct GnDx {
  float mu, rsig, nds, v, denom;
  __device__ __forceinline__ GnDx(float mu_, float rsig_, float ds, float db, float n)
      : mu(mu_), rsig(rsig_), nds(-ds), v(db * rsig_), denom(1.0f / n) {}
  __device__ __forceinline__ float one(float dy, float x, float g) const {
    const float u = nds * (x - mu) * (rsig * rsig * rsig);
    return g * dy * rsig + (u - v) * denom;
  }
  __device__ __forceinline__ float at(float dy, float x, float g) const { return one(dy, x, g); }
  __device__ __forceinline__ float4 at(const float4& dy, const float4& x, float g) const {
    return make_float4(one(dy.x, x.x, g), one(dy.y, x.y, g), one(dy.z, x.z, g), one(dy.w, x.w, g));
  }
};

// sum over the TG threads that share a group: the wave's butterfly, then (TG == 256) the four wave results in
// order.  `slot`: four floats of LDS that no other reduction in flight uses.
template <int TG>
__device__ __forceinline__ float gn_group_sum(float v, float* slot) {
  if constexpr (TG == kWave) return wave_sum_f32(v);
  else return block_sum_f32<TG, false>(v, slot);   // (no barrier behind the read: every reduction in flight has its own slot)
}
template <int TG>
__device__ __forceinline__ void gn_group_sync() {
  if (TG == kWave) wave_lds_sync(); else __syncthreads();
}

// mean and M2 = sum (x - mean)^2 of `cnt` floats held as v[PER] by TG threads (items past the end are zero and masked)
template <int TG, int PER, typename Item>
__device__ __forceinline__ void gn_moments(const Item (&v)[PER], unsigned t, unsigned items, float cnt, float* red,
                                           float& mean, float& m2) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) s += gn_hsum(v[k]);
  mean = gn_group_sum<TG>(s, red) / cnt;
  float q = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k)
    if (t + k * TG < items) q += gn_sq(v[k], mean);
  m2 = gn_group_sum<TG>(q, red + 4);
}

template <int TG, int PER, int MODE>
__global__ __launch_bounds__(kGnT) void gn_fwd_small_kernel(GnArgs a) {
  using IO = GnIO<MODE>;
  using Item = typename IO::Item;
  __shared__ float red[8];
  const unsigned t = threadIdx.x % TG;
  const unsigned ng = blockIdx.x * (kGnT / TG) + threadIdx.x / TG;
  if (ng >= a.NG) return;   // (a whole wave, TG == 64; never taken for TG == 256)
  const float* xg = a.x + ((size_t)ng * a.ipg) * IO::W;
  float* yg = a.y + ((size_t)ng * a.ipg) * IO::W;
  Item v[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < a.ipg) v[k] = IO::ld(xg, i); else gn_zero(v[k]);
  }
  float mean, m2;
  gn_moments<TG, PER>(v, t, a.ipg, a.n, red, mean, m2);
  const float rsig = 1.0f / sqrtf(m2 / a.n + a.eps);
  const unsigned c0 = (ng % a.G) * a.D;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < a.ipg) {
      const unsigned c = c0 + i / a.ipc;
      IO::st(yg, i, gn_norm(v[k], mean, rsig, a.gamma[c], a.beta[c]));
    }
  }
  if (t == 0) {
    a.mu[ng] = mean;
    a.rsig[ng] = rsig;
  }
}

template <int MODE>
__global__ __launch_bounds__(kGnT) void gn_fwd_partial_kernel(GnArgs a) {
  using IO = GnIO<MODE>;
  using Item = typename IO::Item;
  constexpr int PER = kGnChunk / kGnT;
  __shared__ float red[8];
  const unsigned ng = blockIdx.x / a.S, s = blockIdx.x - ng * a.S;
  const unsigned first = s * kGnChunk;
  const unsigned items = a.ipg - first < (unsigned)kGnChunk ? a.ipg - first : (unsigned)kGnChunk;
  const float* xg = a.x + ((size_t)ng * a.ipg + first) * IO::W;
  Item v[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = threadIdx.x + k * kGnT;
    if (i < items) v[k] = IO::ld(xg, i); else gn_zero(v[k]);
  }
  float mean, m2;
  gn_moments<kGnT, PER>(v, threadIdx.x, items, (float)(items * IO::W), red, mean, m2);
  if (threadIdx.x == 0) a.part[blockIdx.x] = make_float2(mean, m2);
}

// Chan, Golub, LeVeque: (na, ma, Ma) + (nb, mb, Mb)
__device__ __forceinline__ void gn_merge(double& na, double& ma, double& Ma, double nb, double mb, double Mb) {
  if (nb == 0.0) return;
  if (na == 0.0) { na = nb; ma = mb; Ma = Mb; return; }
  const double n = na + nb, d = mb - ma;
  ma = ma + d * (nb / n);
  Ma = Ma + Mb + d * d * (na * nb / n);
  na = n;
}

template <int MODE>
__global__ __launch_bounds__(kGnT) void gn_fwd_combine_kernel(GnArgs a) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned ng = blockIdx.x * (kGnT / kWave) + threadIdx.x / kWave;
  if (ng >= a.NG) return;
  const float2* p = a.part + (size_t)ng * a.S;
  const unsigned per = GnIO<MODE>::W;
  double n = 0.0, m = 0.0, M = 0.0;
  for (unsigned s = lane; s < a.S; s += kWave) {
    const unsigned first = s * kGnChunk;
    const unsigned items = a.ipg - first < (unsigned)kGnChunk ? a.ipg - first : (unsigned)kGnChunk;
    const float2 v = p[s];
    gn_merge(n, m, M, (double)(items * per), (double)v.x, (double)v.y);
  }
  // lanes in a fixed tree: lane l takes lane l + off; lane 0 ends with the whole group
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double nb = __shfl_down(n, off), mb = __shfl_down(m, off), Mb = __shfl_down(M, off);
    if (lane + off < (unsigned)kWave) gn_merge(n, m, M, nb, mb, Mb);
  }
  if (lane == 0) {
    a.mu[ng] = (float)m;
    a.rsig[ng] = 1.0f / sqrtf((float)(M / n) + a.eps);
  }
}

template <int MODE>
__global__ __launch_bounds__(kGnT) void gn_fwd_apply_kernel(GnArgs a) {
  using IO = GnIO<MODE>;
  using Item = typename IO::Item;
  const unsigned ng = blockIdx.x / a.S, s = blockIdx.x - ng * a.S;
  const float mu = a.mu[ng], rsig = a.rsig[ng];
  const unsigned c0 = (ng % a.G) * a.D;
  const float* xg = a.x + ((size_t)ng * a.ipg) * IO::W;
  float* yg = a.y + ((size_t)ng * a.ipg) * IO::W;
  Item v[kGnApplyPer];
  const unsigned i0 = s * (kGnT * kGnApplyPer) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kGnApplyPer; ++k)
    if (i0 + k * kGnT < a.ipg) v[k] = IO::ld(xg, i0 + k * kGnT);
#pragma unroll
  for (int k = 0; k < kGnApplyPer; ++k) {
    const unsigned i = i0 + k * kGnT;
    if (i < a.ipg) {
      const unsigned c = c0 + i / a.ipc;
      IO::st(yg, i, gn_norm(v[k], mu, rsig, a.gamma[c], a.beta[c]));
    }
  }
}

// ------------------------------------------------------------------------------------------ backward --
template <int TG, int PER, int MODE>
__global__ __launch_bounds__(kGnT) void gn_bwd_small_kernel(GnArgs a) {
  using IO = GnIO<MODE>;
  using Item = typename IO::Item;
  __shared__ float red[8];
  __shared__ float item_sum[2][kGnT * PER];   // per item: sum dy * (x - mu), sum dy
  const unsigned t = threadIdx.x % TG;
  const unsigned slot = threadIdx.x / TG;
  const unsigned ng = blockIdx.x * (kGnT / TG) + slot;
  if (ng >= a.NG) return;
  const float* xg = a.x + ((size_t)ng * a.ipg) * IO::W;
  const float* gg = a.dy + ((size_t)ng * a.ipg) * IO::W;
  float* dg = a.y + ((size_t)ng * a.ipg) * IO::W;
  const float mu = a.mu_in[ng], rsig = a.rsig_in[ng];
  const unsigned c0 = (ng % a.G) * a.D;
  float* ia = item_sum[0] + slot * (TG * PER);
  float* ib = item_sum[1] + slot * (TG * PER);
  Item xv[PER], gv[PER];
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < a.ipg) { xv[k] = IO::ld(xg, i); gv[k] = IO::ld(gg, i); } else { gn_zero(xv[k]); gn_zero(gv[k]); }
  }
  float sa = 0.f, sb = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < a.ipg) {
      const float g = a.gamma[c0 + i / a.ipc];
      const float pa = gn_dot(gv[k], xv[k], mu), pb = gn_hsum(gv[k]);
      sa += g * pa;
      sb += g * pb;
      if (a.table) { ia[i] = pa; ib[i] = pb; }
    }
  }
  const float ds = gn_group_sum<TG>(sa, red), db = gn_group_sum<TG>(sb, red + 4);
  const GnDx rule(mu, rsig, ds, db, a.n);
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const unsigned i = t + k * TG;
    if (i < a.ipg) IO::st(dg, i, rule.at(gv[k], xv[k], a.gamma[c0 + i / a.ipc]));
  }
  if (a.table) {
    // channel d of the group: its ipc item sums, a wave per channel, lanes striding, then the butterfly
    gn_group_sync<TG>();
    const unsigned lane = threadIdx.x & (kWave - 1);
    for (unsigned d = t / kWave; d < a.D; d += TG / kWave) {
      float ca = 0.f, cb = 0.f;
      for (unsigned j = lane; j < a.ipc; j += kWave) {
        ca += ia[d * a.ipc + j];
        cb += ib[d * a.ipc + j];
      }
      ca = wave_sum_f32(ca);
      cb = wave_sum_f32(cb);
      if (lane == 0) {
        float* row = a.table + 2 * ((size_t)ng * a.D + d);   // (n * C + g * D + d): ng * D = n * C + g * D
        row[0] = ca;
        row[1] = cb;
      }
    }
  }
}

// split path: a worker of TG threads per (n, c) row
template <int TG, int MODE>
__global__ __launch_bounds__(kGnT) void gn_bwd_rows_kernel(GnArgs a) {
  using IO = GnIO<MODE>;
  using Item = typename IO::Item;
  __shared__ float red[8];
  const unsigned t = threadIdx.x % TG;
  const unsigned row = blockIdx.x * (kGnT / TG) + threadIdx.x / TG;
  if (row >= a.NG * a.D) return;
  const float mu = a.mu_in[row / a.D];
  const float* xr = a.x + ((size_t)row * a.ipc) * IO::W;
  const float* gr = a.dy + ((size_t)row * a.ipc) * IO::W;
  float sa = 0.f, sb = 0.f;
  unsigned i = t;
  for (; i + 3 * TG < a.ipc; i += 4 * TG) {   // four items in flight per stream
    const Item x0 = IO::ld(xr, i), x1 = IO::ld(xr, i + TG), x2 = IO::ld(xr, i + 2 * TG), x3 = IO::ld(xr, i + 3 * TG);
    const Item g0 = IO::ld(gr, i), g1 = IO::ld(gr, i + TG), g2 = IO::ld(gr, i + 2 * TG), g3 = IO::ld(gr, i + 3 * TG);
    sa += gn_dot(g0, x0, mu); sb += gn_hsum(g0);
    sa += gn_dot(g1, x1, mu); sb += gn_hsum(g1);
    sa += gn_dot(g2, x2, mu); sb += gn_hsum(g2);
    sa += gn_dot(g3, x3, mu); sb += gn_hsum(g3);
  }
  for (; i < a.ipc; i += TG) {
    const Item x0 = IO::ld(xr, i), g0 = IO::ld(gr, i);
    sa += gn_dot(g0, x0, mu);
    sb += gn_hsum(g0);
  }
  sa = gn_group_sum<TG>(sa, red);
  sb = gn_group_sum<TG>(sb, red + 4);
  if (t == 0) {
    a.table[2 * (size_t)row] = sa;
    a.table[2 * (size_t)row + 1] = sb;
  }
}

// a wave per group: lanes stride its D table rows, then the butterfly
__global__ __launch_bounds__(kGnT) void gn_bwd_group_kernel(GnArgs a) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned ng = blockIdx.x * (kGnT / kWave) + threadIdx.x / kWave;
  if (ng >= a.NG) return;
  const float* row = a.table + 2 * (size_t)ng * a.D;
  const float* gam = a.gamma + (ng % a.G) * a.D;
  float ds = 0.f, db = 0.f;
  for (unsigned d = lane; d < a.D; d += kWave) {
    ds += gam[d] * row[2 * d];
    db += gam[d] * row[2 * d + 1];
  }
  ds = wave_sum_f32(ds);
  db = wave_sum_f32(db);
  if (lane == 0) {
    a.gsum[2 * ng] = ds;
    a.gsum[2 * ng + 1] = db;
  }
}

template <int MODE>
__global__ __launch_bounds__(kGnT) void gn_bwd_dx_kernel(GnArgs a) {
  using IO = GnIO<MODE>;
  using Item = typename IO::Item;
  const unsigned ng = blockIdx.x / a.S, s = blockIdx.x - ng * a.S;
  const GnDx rule(a.mu_in[ng], a.rsig_in[ng], a.gsum[2 * ng], a.gsum[2 * ng + 1], a.n);
  const unsigned c0 = (ng % a.G) * a.D;
  const float* xg = a.x + ((size_t)ng * a.ipg) * IO::W;
  const float* gg = a.dy + ((size_t)ng * a.ipg) * IO::W;
  float* dg = a.y + ((size_t)ng * a.ipg) * IO::W;
  Item xv[kGnApplyPer], gv[kGnApplyPer];
  const unsigned i0 = s * (kGnT * kGnApplyPer) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kGnApplyPer; ++k)
    if (i0 + k * kGnT < a.ipg) { xv[k] = IO::ld(xg, i0 + k * kGnT); gv[k] = IO::ld(gg, i0 + k * kGnT); }
#pragma unroll
  for (int k = 0; k < kGnApplyPer; ++k) {
    const unsigned i = i0 + k * kGnT;
    if (i < a.ipg) IO::st(dg, i, rule.at(gv[k], xv[k], a.gamma[c0 + i / a.ipc]));
  }
}

// a wave per channel: lanes stride the batch, then the butterfly
__global__ __launch_bounds__(kGnT) void gn_bwd_param_kernel(const float* __restrict__ table,
                                                            const float* __restrict__ rsig, float* __restrict__ dgamma,
                                                            float* __restrict__ dbeta, unsigned N, unsigned C,
                                                            unsigned G, unsigned D) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned c = blockIdx.x * (kGnT / kWave) + threadIdx.x / kWave;
  if (c >= C) return;
  const unsigned g = c / D;
  float dg = 0.f, db = 0.f;
  for (unsigned n = lane; n < N; n += kWave) {
    const float* row = table + 2 * ((size_t)n * C + c);
    dg += row[0] * rsig[(size_t)n * G + g];
    db += row[1];
  }
  dg = wave_sum_f32(dg);
  db = wave_sum_f32(db);
  if (lane == 0) {
    dgamma[c] = dg;
    dbeta[c] = db;
  }
}

struct GnPlan {
  long n;            // floats per group
  unsigned NG, D;
  size_t part_bytes, table_bytes, gsum_bytes;
};

// argument checks shared by the three entry points; *empty: nothing to do
static int gn_plan(int N, int C, long HxW, int G, GnPlan* p, bool* empty) {
  SD_REQUIRE(N >= 0 && C >= 0 && HxW >= 0, "negative dimension (N=%d C=%d HxW=%ld)", N, C, HxW);
  SD_REQUIRE(G > 0, "num_group=%d is not positive", G);
  SD_REQUIRE(C % G == 0, "C=%d is not divisible by num_group=%d", C, G);
  const long nc = (long)N * C;
  *empty = nc == 0 || HxW == 0;
  if (!*empty && HxW > kGnMaxElems / nc)
    return fail(SD_ERR_UNSUPPORTED, "N*C*HxW = %ld x %ld elements exceed the limit %ld", nc, HxW, kGnMaxElems);
  p->D = (unsigned)(C / G);
  p->NG = (unsigned)((long)N * G);
  p->n = (long)p->D * HxW;
  // sized for the one-float chunking (2048 floats per chunk) whatever path is taken: four times what the
  // four-float paths use; it stays below the backward's table, which sets the size
  p->part_bytes = (size_t)p->NG * (size_t)((p->n + kGnChunk - 1) / kGnChunk) * sizeof(float2);
  p->table_bytes = (size_t)nc * 2 * sizeof(float);
  p->gsum_bytes = (size_t)p->NG * 2 * sizeof(float);
  return SD_OK;
}

static size_t gn_round(size_t b) { return (b + 255) & ~(size_t)255; }
static size_t gn_need(const GnPlan& p) {
  const size_t bwd = gn_round(p.table_bytes) + gn_round(p.gsum_bytes);
  const size_t fwd = gn_round(p.part_bytes);
  return 256 + (bwd > fwd ? bwd : fwd);
}

static bool gn_aligned16(const void* a, const void* b, const void* c = nullptr) {
  return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 15) == 0;
}

template <int MODE>
static void gn_forward(GnArgs& a, hipStream_t st) {
  const char* v = gn_mode_name(MODE);
  if (a.ipg <= (unsigned)(kWave * kGnWavePer)) {
    hipLaunchKernelGGL((gn_fwd_small_kernel<kWave, kGnWavePer, MODE>), dim3(cdiv(a.NG, kGnT / kWave)), dim3(kGnT), 0,
                       st, a);
    note_dispatch("sd::gn_fwd_small_kernel<64,%d,%s>", kGnWavePer, v);
  } else if (a.ipg <= (unsigned)(kGnT * kGnBlockPerFwd)) {
    hipLaunchKernelGGL((gn_fwd_small_kernel<kGnT, kGnBlockPerFwd, MODE>), dim3(a.NG), dim3(kGnT), 0, st, a);
    note_dispatch("sd::gn_fwd_small_kernel<256,%d,%s>", kGnBlockPerFwd, v);
  } else {
    a.S = (a.ipg + kGnChunk - 1) / kGnChunk;
    hipLaunchKernelGGL(gn_fwd_partial_kernel<MODE>, dim3(a.NG * a.S), dim3(kGnT), 0, st, a);
    hipLaunchKernelGGL(gn_fwd_combine_kernel<MODE>, dim3(cdiv(a.NG, kGnT / kWave)), dim3(kGnT), 0, st, a);
    a.S = (a.ipg + kGnT * kGnApplyPer - 1) / (kGnT * kGnApplyPer);
    hipLaunchKernelGGL(gn_fwd_apply_kernel<MODE>, dim3(a.NG * a.S), dim3(kGnT), 0, st, a);
    note_dispatch("sd::gn_fwd_partial_kernel<%s> + sd::gn_fwd_combine_kernel + sd::gn_fwd_apply_kernel<%s> (split)",
                  v, v);
  }
}

template <int MODE>
static void gn_backward(GnArgs& a, hipStream_t st) {
  const char* v = gn_mode_name(MODE);
  if (a.ipg <= (unsigned)(kWave * kGnWavePer)) {
    hipLaunchKernelGGL((gn_bwd_small_kernel<kWave, kGnWavePer, MODE>), dim3(cdiv(a.NG, kGnT / kWave)), dim3(kGnT), 0,
                       st, a);
    note_dispatch("sd::gn_bwd_small_kernel<64,%d,%s>", kGnWavePer, v);
  } else if (a.ipg <= (unsigned)(kGnT * kGnBlockPerBwd)) {
    hipLaunchKernelGGL((gn_bwd_small_kernel<kGnT, kGnBlockPerBwd, MODE>), dim3(a.NG), dim3(kGnT), 0, st, a);
    note_dispatch("sd::gn_bwd_small_kernel<256,%d,%s>", kGnBlockPerBwd, v);
  } else {
    const unsigned rows = a.NG * a.D;
    if (a.ipc <= 4u * kWave)
      hipLaunchKernelGGL((gn_bwd_rows_kernel<kWave, MODE>), dim3(cdiv(rows, kGnT / kWave)), dim3(kGnT), 0, st, a);
    else
      hipLaunchKernelGGL((gn_bwd_rows_kernel<kGnT, MODE>), dim3(rows), dim3(kGnT), 0, st, a);
    hipLaunchKernelGGL(gn_bwd_group_kernel, dim3(cdiv(a.NG, kGnT / kWave)), dim3(kGnT), 0, st, a);
    a.S = (a.ipg + kGnT * kGnApplyPer - 1) / (kGnT * kGnApplyPer);
    hipLaunchKernelGGL(gn_bwd_dx_kernel<MODE>, dim3(a.NG * a.S), dim3(kGnT), 0, st, a);
    note_dispatch("sd::gn_bwd_rows_kernel<%d,%s> + sd::gn_bwd_group_kernel + sd::gn_bwd_dx_kernel<%s> (split)",
                  a.ipc <= 4u * kWave ? kWave : kGnT, v, v);
  }
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_group_norm_workspace_bytes(int N, int C, long HxW, int G) {
  GnPlan p{};
  bool empty = false;
  if (gn_plan(N, C, HxW, G, &p, &empty) != SD_OK || empty) return 256;
  return gn_need(p);
}

extern "C" int sd_group_norm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mu,
                                 float* rsig, int N, int C, long HxW, int G, float eps, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  GnPlan p{};
  bool empty = false;
  if (int e = gn_plan(N, C, HxW, G, &p, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(x && gamma && beta && y && mu && rsig, "null pointer");
  SD_REQUIRE(workspace && workspace_bytes >= gn_need(p), "group_norm_fwd workspace too small: %zu < %zu bytes",
             workspace ? workspace_bytes : (size_t)0, gn_need(p));
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  GnArgs a{};
  a.x = x; a.gamma = gamma; a.beta = beta; a.y = y; a.mu = mu; a.rsig = rsig;
  a.part = reinterpret_cast<float2*>(base);
  a.NG = p.NG; a.G = (unsigned)G; a.D = p.D; a.C = (unsigned)C;
  a.n = (float)p.n; a.eps = eps;
  hipStream_t st = (hipStream_t)stream;
  const bool quad = HxW % 4 == 0;
  a.ipc = (unsigned)(quad ? HxW / 4 : HxW);
  a.ipg = (unsigned)(quad ? p.n / 4 : p.n);
  if (!quad) gn_forward<kGnScalar>(a, st);
  else if (gn_aligned16(x, y)) gn_forward<kGnVec4>(a, st);
  else gn_forward<kGnQuad>(a, st);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_group_norm_bwd(const float* dy, const float* x, const float* mu, const float* rsig,
                                 const float* gamma, float* dx, float* dgamma, float* dbeta, int N, int C, long HxW,
                                 int G, void* workspace, size_t workspace_bytes, void* stream) {
  GnPlan p{};
  bool empty = false;
  if (int e = gn_plan(N, C, HxW, G, &p, &empty)) return e;
  SD_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "dgamma and dbeta must be given, or be NULL, together");
  if (empty) return SD_OK;   // (dgamma / dbeta are sums over nothing; like every empty call, nothing is written)
  SD_REQUIRE(dy && x && mu && rsig && gamma && dx, "null pointer");
  SD_REQUIRE(workspace && workspace_bytes >= gn_need(p), "group_norm_bwd workspace too small: %zu < %zu bytes",
             workspace ? workspace_bytes : (size_t)0, gn_need(p));
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
  GnArgs a{};
  a.x = x; a.dy = dy; a.gamma = gamma; a.mu_in = mu; a.rsig_in = rsig; a.y = dx;
  float* table = reinterpret_cast<float*>(base);
  a.gsum = reinterpret_cast<float*>(base + gn_round(p.table_bytes));
  a.NG = p.NG; a.G = (unsigned)G; a.D = p.D; a.C = (unsigned)C;
  a.n = (float)p.n;
  hipStream_t st = (hipStream_t)stream;
  const bool quad = HxW % 4 == 0;
  a.ipc = (unsigned)(quad ? HxW / 4 : HxW);
  a.ipg = (unsigned)(quad ? p.n / 4 : p.n);
  // the split path derives ds / db from the table; the small path needs it for dgamma / dbeta only
  const bool split = a.ipg > (unsigned)(kGnT * kGnBlockPerBwd);
  a.table = (dgamma || split) ? table : nullptr;
  if (!quad) gn_backward<kGnScalar>(a, st);
  else if (gn_aligned16(dy, x, dx)) gn_backward<kGnVec4>(a, st);
  else gn_backward<kGnQuad>(a, st);
  if (dgamma)
    hipLaunchKernelGGL(gn_bwd_param_kernel, dim3(cdiv(C, kGnT / kWave)), dim3(kGnT), 0, st, table, rsig, dgamma, dbeta,
                       (unsigned)N, (unsigned)C, (unsigned)G, p.D);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
