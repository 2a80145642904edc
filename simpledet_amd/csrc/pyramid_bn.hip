// Pyramid batch norm for gfx950, fp32 and fp16: SEPC's integrated batch norm (models/sepc/sepc_neck.py:112-119,
// `ibn_func`) with the caller's ReLU (:108, :50) in the same pass.  The reduction domain of a channel is a LIST of
// 1..8 tensors, the pyramid levels; each is read in place and written in place.
//
// The reference's graph is reshape + Concat over the last axis, SyncBatchNorm on (N, C, 1, sum HxW), five
// slice_axis, five reshape_like and five relu: nine tensor passes forward.  Here a direction is the two entry
// points of sync_bn.hip (the exchange of a (2, C) float32 block lies between them) over a level table that travels
// in the kernel arguments: three passes forward, five backward, kernel nodes only under capture.
//
// Contract.  Level l: x_l / y_l / dy_l / dx_l (N, C, HxW_l) contiguous; N and C shared; n = N * sum_l HxW_l.
// gamma, beta, mean, var, moving_*, dgamma, dbeta (C) float32; g = fix_gamma ? 1 : gamma[c].  Every float32 step is
// rounded on its own (-ffp-contract=off).  T is the element type.
//   sd_pyramid_bn_stats      part[0, c] = the mean of the rank's n elements, part[1, c] = their biased variance
//                            ABOUT THAT MEAN.  Every level is read once: a unit is resident in registers.
//   sd_pyramid_bn_apply      parts (W, 2, C) -> mean, var: the combine of sd_sync_bn_apply (double, rank order);
//                            inv = 1.0f / sqrtf(var + eps);  z = (g * (x - mean)) * inv + beta[c];  zt = (T)z;
//                            y = relu ? (zt > 0 ? zt : 0) : zt
//   sd_pyramid_bn_infer_fwd  a = g / sqrtf(moving_var + eps);  b = beta - (g * moving_mean) / sqrtf(moving_var + eps);
//                            z = a * x + b, then as above
//   sd_pyramid_bn_bwd_stats  dy' = dy, or with relu 0 wherever the forward STORED y <= 0: zt is recomputed from x,
//                            mean, var, gamma, beta by the forward's own expression and rounding, so a z that
//                            underflows in T is masked too and y is no input.
//                            bpart[0, c] = sum dy', bpart[1, c] = sum dy' * (x - mean)
//   sd_pyramid_bn_bwd_apply  bparts (W, 2, C), rank -> dx_l, dgamma, dbeta, moving_*: the rules of
//                            sd_sync_bn_bwd_apply with this n and dy' in the place of dy.
// Not provided: kAddTo.
//
// Items.  A level is contiguous, so its ITEMS are the aligned groups of 8 elements of its flat index space,
// [8G, 8G + 8).  A channel's row of HxW_l elements starting at s = (n * C + c) * HxW_l meets the items
// G = s / 8 + j, j < ipr_l, each with the element range [max(8G, s), min(8G + 8, s + HxW_l)): a partial head, whole
// items, a partial tail.  ipr_l = (HxW_l + 7 - gcd(HxW_l, 8)) / 8 + 1 bounds the items a row can meet (a row start
// is a multiple of gcd(HxW_l, 8)); a row that meets fewer leaves its last SLOT empty.  Whole items move as 16 bytes
// (two accesses for floats) where every level pointer of the call is 16-byte aligned, everything else by element.
// Every sum is defined on slots -- an item's eight terms pairwise with 0 outside the row, a thread's slots in order,
// the wave butterfly, the four waves left to right, the partials in index order -- so no bit depends on the element
// type or on a pointer's alignment.
//
// Units.  Levels are sorted by size, largest first.  The smallest levels whose slots per channel, N * ipr_l, sum to
// <= 256 form the WAVE GROUP: one wave takes a channel's rows of all of them (P6 and P7 of the 800 x 1333 pyramid:
// 184 slots).  Every other level is cut per channel into chunks of 1024 slots, a workgroup each.  One launch holds
// all of them, the chunks of the largest level first, the wave units (four channels per workgroup) last.
//   pbn_reduce_kernel       a unit -> (count, mean, M2 about its own mean), or (sum dy', sum dy' (x - mean))
//   pbn_stats_merge_kernel  a wave per channel: Chan's rule for unequal counts, in double, in a fixed order
//   bn_bwd_merge_kernel     a wave per channel: the partial sums in double, in a fixed order
//   bn_fwd_coef_kernel / bn_bwd_coef_kernel   a thread per channel: the combine over the ranks, the coefficients
//                           (these three are norm_common.h's, the ones sync_bn.hip launches; so are the merge and
//                           the sums)
//   pbn_map_kernel          the element rules, flat over each level, a thread per item.  An item inside one row
//                           takes one coefficient; an item that straddles rows (any HxW_l % 8 != 0) takes its
//                           channel per element.  Both read a C x float4 table in LDS (two tables for the backward
//                           under relu); channels past 1024 read the workspace.
// No floating-point atomics, no memset, no copy, no host read: every workspace word that is read was written by a
// kernel of the same call, and every grid depends on the shapes alone.
#include "common.h"
#include "norm_common.h"
#include "../../include/simpledet_ops.h"

namespace sd {
namespace {

constexpr int kPbnT = 256;
constexpr int kPbnMaxL = 8;
constexpr int kPbnPer = 4;                     // resident slots per thread of a reduction unit
constexpr int kPbnChunk = kPbnT * kPbnPer;     // slots of a workgroup's unit: 8192 elements
constexpr int kPbnWaveCap = kWave * kPbnPer;   // slots of a wave's unit
constexpr int kPbnMapPer = 2;                  // items per thread of the element kernels
constexpr int kPbnLdsC = 1024;                 // channels of the LDS coefficient tables
constexpr long kPbnMaxElems = 2147483647L;     // element indices are 32-bit inside the kernels

struct PbnLevel {
  const void* x;
  const void* dy;     // backward
  void* y;            // forward: y; backward: dx
  unsigned HxW;
  unsigned elems;     // N * C * HxW
  unsigned ipr;       // slots per row
  unsigned slots;     // N * ipr: slots per channel
  unsigned chunks;    // workgroup units per channel (0: in the wave group)
  unsigned unit0;     // the first of them among the channel's S partials
  unsigned rblk0;     // the level's first workgroup in the reductions ...
  unsigned mblk0;     // ... and in the element kernels
};

struct PbnArgs {
  PbnLevel lv[kPbnMaxL];   // largest first
  unsigned L, nbig;        // levels [0, nbig) have workgroup units, [nbig, L) are the wave group
  unsigned N, C, S;        // S: partials per channel
  unsigned rblk_wave;      // the first workgroup of the wave units
  unsigned wslots;         // slots per channel of the wave group
  void* partial;           // (C, S) float4 (statistics) or float2 (backward)
  float* out;              // (2, C)
  const float4* coef;      // (C): forward (mean, inv, g, beta); backward (a, b, c, mean)
  const float4* coef2;     // (C): the forward's, for the backward's mask
  const float* mean;
  const float* var;
  const float* gamma;
  const float* beta;
  const float* mmean;      // inference
  const float* mvar;
  double n;                // N * sum HxW
  float eps;
  int fix_gamma, relu;
};

// elements [lo, hi) of the item [e0, e0 + 8) of a level; 0 outside
template <typename T, bool VEC>
__device__ __forceinline__ void pbn_ld(const T* p, unsigned e0, unsigned lo, unsigned hi, float (&v)[8]) {
  if (VEC && hi - lo == 8u) {
    vec16_ld_f32(p + e0, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const unsigned e = e0 + k;
    v[k] = (e >= lo && e < hi) ? (float)p[e] : 0.f;
  }
}

// v holds values of T already (the caller rounded them)
template <typename T, bool VEC>
__device__ __forceinline__ void pbn_st(T* p, unsigned e0, unsigned cnt, const float (&v)[8]) {
  if (VEC && cnt == 8u) {
    vec16_st_f32(p + e0, v);
    return;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if ((unsigned)k < cnt) p[e0 + k] = (T)v[k];
}

// the forward's stored value: z rounded to T, then the ReLU
template <typename T>
__device__ __forceinline__ float pbn_act(float z, int relu) {
  const float zt = (float)(T)z;
  return relu ? (zt > 0.f ? zt : 0.f) : zt;
}

struct PbnRow {          // what a slot needs of its level
  const void* x;
  const void* dy;
  unsigned HxW, ipr, q;  // q: the slot inside the level
};

// One reduction unit of TG threads: slots [first, first + TG * kPbnPer) of channel c.  TG = 256: inside level `lvl`
// (uniform); TG = 64: inside the wave group, the level chosen per slot.
template <typename T, bool VEC, int TG, bool BWD>
__device__ __forceinline__ void pbn_unit(const PbnArgs& a, unsigned c, unsigned lvl, unsigned first, unsigned total,
                                         unsigned pidx, float* red) {
  const unsigned t = threadIdx.x % TG;
  float xv[kPbnPer][8], gv[BWD ? kPbnPer : 1][8];
  unsigned char lo8[kPbnPer], hi8[kPbnPer];   // the valid range of a slot, relative to its item
  // (the loop over the levels is unrolled with constant indices: the table stays in scalar registers)
  PbnRow blk{};
  if (TG == kPbnT) {
#pragma unroll
    for (int l = 0; l < kPbnMaxL; ++l)
      if ((unsigned)l == lvl) { blk.x = a.lv[l].x; blk.dy = a.lv[l].dy; blk.HxW = a.lv[l].HxW; blk.ipr = a.lv[l].ipr; }
  }
#pragma unroll
  for (int k = 0; k < kPbnPer; ++k) {
    const unsigned q = first + t + k * TG;
    bool ok = q < total;
    PbnRow r = blk;
    r.q = q;
    if (TG == kWave) {
      unsigned off = 0;
#pragma unroll
      for (int l = 0; l < kPbnMaxL; ++l) {
        const bool in = (unsigned)l >= a.nbig && (unsigned)l < a.L && q >= off;
        if (in) { r.x = a.lv[l].x; r.dy = a.lv[l].dy; r.HxW = a.lv[l].HxW; r.ipr = a.lv[l].ipr; r.q = q - off; }
        if ((unsigned)l >= a.nbig && (unsigned)l < a.L) off += a.lv[l].slots;
      }
    }
    unsigned e0 = 0, lo = 0, hi = 0;
    if (ok) {
      const unsigned n = r.q / r.ipr, j = r.q - n * r.ipr;
      const unsigned s = (n * a.C + c) * r.HxW;
      e0 = (s / 8u + j) * 8u;
      lo = e0 > s ? e0 : s;
      hi = e0 + 8u < s + r.HxW ? e0 + 8u : s + r.HxW;
      ok = hi > lo;
    }
    if (ok) {
      pbn_ld<T, VEC>(static_cast<const T*>(r.x), e0, lo, hi, xv[k]);
      if (BWD) pbn_ld<T, VEC>(static_cast<const T*>(r.dy), e0, lo, hi, gv[BWD ? k : 0]);
      lo8[k] = (unsigned char)(lo - e0);
      hi8[k] = (unsigned char)(hi - e0);
    } else {
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xv[k][i] = 0.f;
        if (BWD) gv[BWD ? k : 0][i] = 0.f;
      }
      lo8[k] = hi8[k] = 0;
    }
  }
  if constexpr (!BWD) {
    float sm = 0.f, cn = 0.f;
#pragma unroll
    for (int k = 0; k < kPbnPer; ++k) {
      float f[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) f[i] = xv[k][i];
      sm += tree_sum(f);
      cn += (float)(hi8[k] - lo8[k]);
    }
    sm = group_sum_f32<TG>(sm, red);
    cn = group_sum_f32<TG>(cn, red + 4);       // (whole numbers below 2^24: exact)
    const float mean = cn > 0.f ? sm / cn : 0.f;
    float q2 = 0.f;
#pragma unroll
    for (int k = 0; k < kPbnPer; ++k) {
      float f[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = xv[k][i] - mean;
        f[i] = (i >= lo8[k] && i < hi8[k]) ? d * d : 0.f;
      }
      q2 += tree_sum(f);
    }
    const float m2 = group_sum_f32<TG>(q2, red + 8);
    if (t == 0) static_cast<float4*>(a.partial)[(size_t)c * a.S + pidx] = make_float4(cn, mean, m2, 0.f);
  } else {
    const float mean = a.mean[c];
    float inv = 0.f, g = 0.f, beta = 0.f;
    if (a.relu) {
      inv = 1.0f / sqrtf(a.var[c] + a.eps);
      g = a.fix_gamma ? 1.0f : a.gamma[c];
      beta = a.beta[c];
    }
    float sg = 0.f, sp = 0.f;
#pragma unroll
    for (int k = 0; k < kPbnPer; ++k) {
      float f[8], h[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const float d = xv[k][i] - mean;
        float dy = gv[BWD ? k : 0][i];
        if (a.relu) {
          const float zt = (float)(T)((g * d) * inv + beta);
          if (!(zt > 0.f)) dy = 0.f;
        }
        f[i] = dy;
        h[i] = dy * d;
      }
      sg += tree_sum(f);
      sp += tree_sum(h);
    }
    sg = group_sum_f32<TG>(sg, red);
    sp = group_sum_f32<TG>(sp, red + 4);
    if (t == 0) static_cast<float2*>(a.partial)[(size_t)c * a.S + pidx] = make_float2(sg, sp);
  }
}

template <typename T, bool VEC, bool BWD>
__global__ __launch_bounds__(kPbnT) void pbn_reduce_kernel(PbnArgs a) {
  __shared__ float red[12];
  const unsigned b = blockIdx.x;
  if (b < a.rblk_wave) {
    unsigned lvl = 0, b0 = 0, chunks = 1, unit0 = 0, slots = 0;
#pragma unroll
    for (int l = 0; l < kPbnMaxL; ++l)
      if ((unsigned)l < a.nbig && b >= a.lv[l].rblk0) {
        lvl = l; b0 = a.lv[l].rblk0; chunks = a.lv[l].chunks; unit0 = a.lv[l].unit0; slots = a.lv[l].slots;
      }
    const unsigned rb = b - b0, c = rb / chunks, k = rb - c * chunks;
    pbn_unit<T, VEC, kPbnT, BWD>(a, c, lvl, k * (unsigned)kPbnChunk, slots, unit0 + k, red);
  } else {
    const unsigned c = (b - a.rblk_wave) * (kPbnT / kWave) + threadIdx.x / kWave;
    if (c >= a.C) return;   // (a whole wave)
    pbn_unit<T, VEC, kWave, BWD>(a, c, 0, 0, a.wslots, a.S - 1, red);
  }
}

// a wave per channel: lanes stride its S partials, then a fixed tree over the lanes
__global__ __launch_bounds__(kPbnT) void pbn_stats_merge_kernel(const float4* partial, float* out, unsigned C,
                                                                unsigned S) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned c = blockIdx.x * (kPbnT / kWave) + threadIdx.x / kWave;
  if (c >= C) return;
  const float4* p = partial + (size_t)c * S;
  double n = 0.0, m = 0.0, M = 0.0;
  for (unsigned s = lane; s < S; s += kWave) {
    const float4 v = p[s];
    chan_merge(n, m, M, (double)v.x, (double)v.y, (double)v.z);
  }
  wave_tree_chan(lane, n, m, M);
  if (lane == 0) {
    out[c] = (float)m;
    out[C + c] = (float)(M / n);
  }
}

enum { kPbnFwd = 0, kPbnBwd = 1, kPbnInfer = 2 };

// the coefficients of channel c as the tables hold them; `second`: the backward's mask table
template <int KIND>
__device__ __forceinline__ float4 pbn_coef(const PbnArgs& a, unsigned c, bool second) {
  if (KIND == kPbnInfer) {
    const float g = a.fix_gamma ? 1.0f : a.gamma[c];
    const float sd_ = sqrtf(a.mvar[c] + a.eps);
    return make_float4(g / sd_, a.beta[c] - (g * a.mmean[c]) / sd_, 0.f, 0.f);
  }
  return second ? a.coef2[c] : a.coef[c];
}

// the element rules, flat over each level: a thread per item, an item's channel by one division, per element where
// the item straddles rows
template <typename T, bool VEC, int KIND>
__global__ __launch_bounds__(kPbnT) void pbn_map_kernel(PbnArgs a) {
  extern __shared__ float4 tab[];
  const unsigned nl = a.C < (unsigned)kPbnLdsC ? a.C : (unsigned)kPbnLdsC;
  const bool two = KIND == kPbnBwd && a.relu;
  for (unsigned c = threadIdx.x; c < nl; c += kPbnT) {
    tab[c] = pbn_coef<KIND>(a, c, false);
    if (two) tab[nl + c] = pbn_coef<KIND>(a, c, true);
  }
  __syncthreads();
  const T* x = nullptr;
  const T* dy = nullptr;
  T* y = nullptr;
  unsigned HxW = 1, elems = 0, b0 = 0;
#pragma unroll
  for (int l = 0; l < kPbnMaxL; ++l)
    if ((unsigned)l < a.L && blockIdx.x >= a.lv[l].mblk0) {
      x = static_cast<const T*>(a.lv[l].x); dy = static_cast<const T*>(a.lv[l].dy); y = static_cast<T*>(a.lv[l].y);
      HxW = a.lv[l].HxW; elems = a.lv[l].elems; b0 = a.lv[l].mblk0;
    }
  const unsigned i0 = (blockIdx.x - b0) * (unsigned)(kPbnT * kPbnMapPer) + threadIdx.x;
  float xv[kPbnMapPer][8], gv[KIND == kPbnBwd ? kPbnMapPer : 1][8];
  unsigned cnt[kPbnMapPer];
#pragma unroll
  for (int k = 0; k < kPbnMapPer; ++k) {
    const unsigned i = i0 + k * kPbnT;
    const unsigned e0 = i * 8u;   // (i < 2^28 wherever it is used: elems < 2^31)
    cnt[k] = (i < (elems + 7u) / 8u) ? (elems - e0 < 8u ? elems - e0 : 8u) : 0u;
    if (cnt[k]) {
      pbn_ld<T, VEC>(x, e0, e0, e0 + cnt[k], xv[k]);
      if (KIND == kPbnBwd) pbn_ld<T, VEC>(dy, e0, e0, e0 + cnt[k], gv[KIND == kPbnBwd ? k : 0]);
    }
  }
#pragma unroll
  for (int k = 0; k < kPbnMapPer; ++k) {
    if (!cnt[k]) continue;
    const unsigned e0 = (i0 + k * kPbnT) * 8u;
    const unsigned plane = e0 / HxW;
    unsigned r = e0 - plane * HxW, c = plane % a.C;
    const bool one = r + 8u <= HxW;   // the item lies inside one row
    float4 k4 = c < nl ? tab[c] : pbn_coef<KIND>(a, c, false);
    float4 m4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (two) m4 = c < nl ? tab[nl + c] : pbn_coef<KIND>(a, c, true);
    float out[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      if (!one && q > 0) {
        if (++r == HxW) {
          r = 0;
          c = c + 1 == a.C ? 0 : c + 1;
          k4 = c < nl ? tab[c] : pbn_coef<KIND>(a, c, false);
          if (two) m4 = c < nl ? tab[nl + c] : pbn_coef<KIND>(a, c, true);
        }
      }
      const float xq = xv[k][q];
      if (KIND == kPbnFwd) {          // mean, inv, g, beta
        out[q] = pbn_act<T>((k4.z * (xq - k4.x)) * k4.y + k4.w, a.relu);
      } else if (KIND == kPbnInfer) {
        out[q] = pbn_act<T>(k4.x * xq + k4.y, a.relu);
      } else {                        // a, b, c, mean
        float g = gv[KIND == kPbnBwd ? k : 0][q];
        if (two) {
          const float zt = (float)(T)((m4.z * (xq - m4.x)) * m4.y + m4.w);
          if (!(zt > 0.f)) g = 0.f;
        }
        out[q] = (g * k4.x + k4.y * (xq - k4.w)) + k4.z;
      }
    }
    pbn_st<T, VEC>(y, e0, cnt[k], out);
  }
}

// ---------------------------------------------------------------------------------------------- host --
struct PbnPlan {
  PbnArgs a;              // the tables, without pointers
  int order[kPbnMaxL];    // a.lv[i] is the caller's level order[i]
  bool empty;
  unsigned rgrid, mgrid;
  size_t coef_bytes, partial_bytes;
};

static unsigned pbn_gcd8(long v) { return v % 8 == 0 ? 8u : v % 4 == 0 ? 4u : v % 2 == 0 ? 2u : 1u; }

static int pbn_plan(int N, int C, const long* HxW, int L, PbnPlan* p) {
  SD_REQUIRE(N >= 0 && C >= 0 && L >= 0, "negative dimension (N=%d C=%d L=%d)", N, C, L);
  if (L > kPbnMaxL) return fail(SD_ERR_UNSUPPORTED, "L=%d levels: at most %d", L, kPbnMaxL);
  SD_REQUIRE(L == 0 || HxW, "null pointer (HxW)");
  for (int l = 0; l < L; ++l) SD_REQUIRE(HxW[l] >= 0, "negative dimension (HxW[%d]=%ld)", l, HxW[l]);
  PbnArgs& a = p->a;
  a = PbnArgs{};
  const long nc = (long)N * C;
  long sum = 0;
  int n = 0;
  for (int l = 0; l < L && nc > 0; ++l) {
    if (HxW[l] == 0) continue;   // (an empty tensor: nothing is done for it)
    if (HxW[l] > kPbnMaxElems / nc || (sum += HxW[l]) > kPbnMaxElems / nc)
      return fail(SD_ERR_UNSUPPORTED, "N*C*sum(HxW) elements exceed the limit %ld", kPbnMaxElems);
    int i = n++;   // insertion by size, largest first, equal sizes in the caller's order
    for (; i > 0 && HxW[p->order[i - 1]] < HxW[l]; --i) p->order[i] = p->order[i - 1];
    p->order[i] = l;
  }
  p->empty = n == 0;
  if (p->empty) return SD_OK;
  a.L = (unsigned)n; a.N = (unsigned)N; a.C = (unsigned)C;
  a.n = (double)N * (double)sum;
  for (int i = 0; i < n; ++i) {
    const long h = HxW[p->order[i]];
    PbnLevel& v = a.lv[i];
    v.HxW = (unsigned)h;
    v.elems = (unsigned)(nc * h);
    v.ipr = (unsigned)((h + 7 - pbn_gcd8(h)) / 8 + 1);
    v.slots = (unsigned)N * v.ipr;
  }
  // the wave group: the smallest levels that fit one wave's unit together
  a.nbig = a.L;
  unsigned long ws = 0;
  while (a.nbig > 0 && ws + (unsigned long)N * a.lv[a.nbig - 1].ipr <= (unsigned long)kPbnWaveCap)
    ws += a.lv[--a.nbig].slots;
  a.wslots = (unsigned)ws;
  unsigned long units = 0, mblk = 0;
  for (unsigned i = 0; i < a.L; ++i) {
    PbnLevel& v = a.lv[i];
    v.chunks = i < a.nbig ? (unsigned)cdiv((long)N * v.ipr, kPbnChunk) : 0u;
    v.unit0 = (unsigned)units;
    if ((unsigned long)C * (units + v.chunks + 1) > 0x7fffffffUL)
      return fail(SD_ERR_UNSUPPORTED, "N*C*sum(HxW) elements exceed the limit %ld", kPbnMaxElems);
    v.rblk0 = (unsigned)((unsigned long)C * units);
    units += v.chunks;
    v.mblk0 = (unsigned)mblk;
    mblk += (unsigned long)cdiv(cdiv((long)v.elems, 8), kPbnT * kPbnMapPer);
  }
  a.rblk_wave = (unsigned)((unsigned long)C * units);
  a.S = (unsigned)units + (a.nbig < a.L ? 1u : 0u);
  p->rgrid = a.rblk_wave + (a.nbig < a.L ? (unsigned)cdiv(C, kPbnT / kWave) : 0u);
  p->mgrid = (unsigned)mblk;
  p->coef_bytes = (size_t)C * sizeof(float4);
  p->partial_bytes = (size_t)C * a.S * sizeof(float4);
  return SD_OK;
}

struct PbnWs {
  float4* coef;
  float4* coef2;
  void* partial;
  size_t need;
};
static PbnWs pbn_carve(const PbnPlan& p, void* workspace) {
  WsCarver w(workspace);
  PbnWs r;
  r.coef = w.take<float4>(p.coef_bytes);
  r.coef2 = w.take<float4>(p.coef_bytes);
  r.partial = w.take<char>(p.partial_bytes);
  r.need = w.need();
  return r;
}
static size_t pbn_need(const PbnPlan& p) { return 256 + pbn_carve(p, nullptr).need; }

// Sets the plan's level pointers from the caller's tables (in the caller's order; `dy` / `y` may be null tables).
// -> 0, or 1: a null pointer, 2: a pointer off its element alignment.  *vec: all of them are 16-byte aligned.
static int pbn_tables(PbnPlan& p, size_t esz, const void* const* x, const void* const* dy, void* const* y,
                      bool want_dy, bool want_y, bool* vec) {
  if (!x || (want_dy && !dy) || (want_y && !y)) return 1;
  *vec = true;
  for (unsigned i = 0; i < p.a.L; ++i) {
    const int l = p.order[i];
    PbnLevel& v = p.a.lv[i];
    v.x = x[l];
    v.dy = want_dy ? dy[l] : nullptr;
    v.y = want_y ? y[l] : nullptr;
    for (const void* q : {v.x, want_dy ? v.dy : v.x, want_y ? (const void*)v.y : v.x}) {
      if (!q) return 1;
      if ((uintptr_t)q % esz) return 2;
      if ((uintptr_t)q % 16) *vec = false;
    }
  }
  return 0;
}
#define PBN_TABLES(...)                                                                     \
  do {                                                                                      \
    const int e_ = pbn_tables(__VA_ARGS__);                                                 \
    SD_REQUIRE(e_ != 1, "null pointer");                                                    \
    SD_REQUIRE(e_ != 2, "a pointer is not aligned to its elements");                        \
  } while (0)

template <typename T, bool BWD>
static void pbn_reduce(const PbnPlan& p, bool vec, float* out, void* partial, hipStream_t st) {
  const PbnArgs& a = p.a;
  if (vec) hipLaunchKernelGGL((pbn_reduce_kernel<T, true, BWD>), dim3(p.rgrid), dim3(kPbnT), 0, st, a);
  else hipLaunchKernelGGL((pbn_reduce_kernel<T, false, BWD>), dim3(p.rgrid), dim3(kPbnT), 0, st, a);
  const dim3 mgrid(cdiv(a.C, kPbnT / kWave));
  if (BWD) hipLaunchKernelGGL(bn_bwd_merge_kernel<kPbnT>, mgrid, dim3(kPbnT), 0, st, static_cast<const float2*>(partial), out,
                              a.C, a.S);
  else hipLaunchKernelGGL(pbn_stats_merge_kernel, mgrid, dim3(kPbnT), 0, st, static_cast<const float4*>(partial), out,
                          a.C, a.S);
  note_dispatch("sd::pbn_reduce_kernel<%s,%s,%s> %u levels, %u in the wave group, %u units per channel + sd::%s",
                elem_type_name<T>(), vec ? "vec" : "narrow", BWD ? "bwd" : "stats", a.L, a.L - a.nbig, a.S,
                BWD ? "bn_bwd_merge_kernel" : "pbn_stats_merge_kernel");
}

template <typename T, int KIND>
static void pbn_map(const PbnPlan& p, bool vec, hipStream_t st, const char* lead) {
  const PbnArgs& a = p.a;
  const unsigned nl = a.C < (unsigned)kPbnLdsC ? a.C : (unsigned)kPbnLdsC;
  const size_t lds = (size_t)nl * sizeof(float4) * (KIND == kPbnBwd && a.relu ? 2 : 1);
  if (vec) hipLaunchKernelGGL((pbn_map_kernel<T, true, KIND>), dim3(p.mgrid), dim3(kPbnT), lds, st, a);
  else hipLaunchKernelGGL((pbn_map_kernel<T, false, KIND>), dim3(p.mgrid), dim3(kPbnT), lds, st, a);
  note_dispatch("%ssd::pbn_map_kernel<%s,%s,%s%s> %u levels", lead, elem_type_name<T>(), vec ? "vec" : "narrow",
                KIND == kPbnFwd ? "fwd" : KIND == kPbnBwd ? "bwd" : "infer", a.relu ? ",relu" : "", a.L);
}

template <typename T>
static int pbn_stats(const void* const* x, float* part, int N, int C, const long* HxW, int L, void* workspace,
                     size_t workspace_bytes, void* stream) {
  PbnPlan p{};
  if (int e = pbn_plan(N, C, HxW, L, &p)) return e;
  if (p.empty) return SD_OK;
  bool vec = false;
  PBN_TABLES(p, sizeof(T), x, nullptr, nullptr, false, false, &vec);
  SD_REQUIRE(part, "null pointer");
  SD_REQUIRE(ptrs_aligned(4, {part}), "a pointer is not aligned to its elements");
  if (int e = workspace_check(workspace, workspace_bytes, pbn_need(p), "pyramid_bn_stats")) return e;
  p.a.partial = pbn_carve(p, workspace).partial;
  pbn_reduce<T, false>(p, vec, part, p.a.partial, (hipStream_t)stream);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int pbn_apply(const void* const* x, const float* parts, int W, const float* gamma, const float* beta,
                     void* const* y, float* mean, float* var, int N, int C, const long* HxW, int L, float eps,
                     int fix_gamma, int relu, void* workspace, size_t workspace_bytes, void* stream) {
  PbnPlan p{};
  if (int e = pbn_plan(N, C, HxW, L, &p)) return e;
  SD_REQUIRE(W >= 1, "W=%d ranks: at least one", W);
  if (p.empty) return SD_OK;
  bool vec = false;
  PBN_TABLES(p, sizeof(T), x, nullptr, y, false, true, &vec);
  SD_REQUIRE(parts && gamma && beta && mean && var, "null pointer");
  SD_REQUIRE(ptrs_aligned(4, {parts, gamma, beta, mean, var}), "a pointer is not aligned to its elements");
  if (int e = workspace_check(workspace, workspace_bytes, pbn_need(p), "pyramid_bn_apply")) return e;
  hipStream_t st = (hipStream_t)stream;
  const PbnWs ws = pbn_carve(p, workspace);
  hipLaunchKernelGGL(bn_fwd_coef_kernel<kPbnT>, dim3(cdiv(C, kPbnT)), dim3(kPbnT), 0, st, parts, W, gamma, beta, mean, var,
                     ws.coef, (unsigned)C, eps, fix_gamma);
  p.a.coef = ws.coef;
  p.a.relu = relu != 0;
  pbn_map<T, kPbnFwd>(p, vec, st, "sd::bn_fwd_coef_kernel + ");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int pbn_infer(const void* const* x, const float* gamma, const float* beta, const float* mmean,
                     const float* mvar, void* const* y, int N, int C, const long* HxW, int L, float eps, int fix_gamma,
                     int relu, void* stream) {
  PbnPlan p{};
  if (int e = pbn_plan(N, C, HxW, L, &p)) return e;
  if (p.empty) return SD_OK;
  bool vec = false;
  PBN_TABLES(p, sizeof(T), x, nullptr, y, false, true, &vec);
  SD_REQUIRE(gamma && beta && mmean && mvar, "null pointer");
  SD_REQUIRE(ptrs_aligned(4, {gamma, beta, mmean, mvar}), "a pointer is not aligned to its elements");
  p.a.gamma = gamma; p.a.beta = beta; p.a.mmean = mmean; p.a.mvar = mvar;
  p.a.eps = eps; p.a.fix_gamma = fix_gamma; p.a.relu = relu != 0;
  pbn_map<T, kPbnInfer>(p, vec, (hipStream_t)stream, "");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int pbn_bwd_stats(const void* const* dy, const void* const* x, const float* mean, const float* var,
                         const float* gamma, const float* beta, float* bpart, int N, int C, const long* HxW, int L,
                         float eps, int fix_gamma, int relu, void* workspace, size_t workspace_bytes, void* stream) {
  PbnPlan p{};
  if (int e = pbn_plan(N, C, HxW, L, &p)) return e;
  if (p.empty) return SD_OK;
  bool vec = false;
  PBN_TABLES(p, sizeof(T), x, dy, nullptr, true, false, &vec);
  SD_REQUIRE(mean && var && gamma && beta && bpart, "null pointer");
  SD_REQUIRE(ptrs_aligned(4, {mean, var, gamma, beta, bpart}), "a pointer is not aligned to its elements");
  if (int e = workspace_check(workspace, workspace_bytes, pbn_need(p), "pyramid_bn_bwd_stats")) return e;
  p.a.partial = pbn_carve(p, workspace).partial;
  p.a.mean = mean; p.a.var = var; p.a.gamma = gamma; p.a.beta = beta;
  p.a.eps = eps; p.a.fix_gamma = fix_gamma; p.a.relu = relu != 0;
  pbn_reduce<T, true>(p, vec, bpart, p.a.partial, (hipStream_t)stream);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int pbn_bwd_apply(const void* const* dy, const void* const* x, const float* mean, const float* var,
                         const float* gamma, const float* beta, const float* bparts, int W, int rank, void* const* dx,
                         float* dgamma, float* dbeta, float* mmean, float* mvar, float momentum, int N, int C,
                         const long* HxW, int L, float eps, int fix_gamma, int relu, void* workspace,
                         size_t workspace_bytes, void* stream) {
  PbnPlan p{};
  if (int e = pbn_plan(N, C, HxW, L, &p)) return e;
  SD_REQUIRE(W >= 1, "W=%d ranks: at least one", W);
  SD_REQUIRE(rank >= 0 && rank < W, "rank=%d is outside 0..%d", rank, W - 1);
  SD_REQUIRE((dgamma == nullptr) == (dbeta == nullptr), "dgamma and dbeta must be given, or be NULL, together");
  SD_REQUIRE((mmean == nullptr) == (mvar == nullptr),
             "moving_mean and moving_var must be given, or be NULL, together");
  if (p.empty) return SD_OK;
  bool vec = false;
  PBN_TABLES(p, sizeof(T), x, dy, dx, true, true, &vec);
  SD_REQUIRE(mean && var && gamma && beta && bparts, "null pointer");
  SD_REQUIRE(ptrs_aligned(4, {mean, var, gamma, beta, bparts, dgamma, dbeta, mmean, mvar}),
             "a pointer is not aligned to its elements");
  if (int e = workspace_check(workspace, workspace_bytes, pbn_need(p), "pyramid_bn_bwd_apply")) return e;
  hipStream_t st = (hipStream_t)stream;
  const PbnWs ws = pbn_carve(p, workspace);
  hipLaunchKernelGGL(bn_bwd_coef_kernel<kPbnT>, dim3(cdiv(C, kPbnT)), dim3(kPbnT), 0, st, bparts, W, rank, mean, var, gamma,
                     beta, dgamma, dbeta, mmean, mvar, momentum, ws.coef, ws.coef2, (unsigned)C, (double)W * p.a.n, eps,
                     fix_gamma);
  p.a.coef = ws.coef; p.a.coef2 = ws.coef2;
  p.a.relu = relu != 0;
  pbn_map<T, kPbnBwd>(p, vec, st, "sd::bn_bwd_coef_kernel + ");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_pyramid_bn_workspace_bytes(int N, int C, const long* HxW, int L) {
  PbnPlan p{};
  if (pbn_plan(N, C, HxW, L, &p) != SD_OK || p.empty) return 256;
  return pbn_need(p);
}

#define PBN_TABLE(p) reinterpret_cast<const void* const*>(p)
#define PBN_OUT_TABLE(p) reinterpret_cast<void* const*>(p)

extern "C" int sd_pyramid_bn_stats(const float* const* x, float* part, int N, int C, const long* HxW, int L,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return pbn_stats<float>(PBN_TABLE(x), part, N, C, HxW, L, workspace, workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_stats_f16(const void* const* x, float* part, int N, int C, const long* HxW, int L,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return pbn_stats<_Float16>(x, part, N, C, HxW, L, workspace, workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_apply(const float* const* x, const float* parts, int W, const float* gamma,
                                   const float* beta, float* const* y, float* mean, float* var, int N, int C,
                                   const long* HxW, int L, float eps, int fix_gamma, int relu, void* workspace,
                                   size_t workspace_bytes, void* stream) {
  return pbn_apply<float>(PBN_TABLE(x), parts, W, gamma, beta, PBN_OUT_TABLE(y), mean, var, N, C, HxW, L, eps,
                          fix_gamma, relu, workspace, workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_apply_f16(const void* const* x, const float* parts, int W, const float* gamma,
                                       const float* beta, void* const* y, float* mean, float* var, int N, int C,
                                       const long* HxW, int L, float eps, int fix_gamma, int relu, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return pbn_apply<_Float16>(x, parts, W, gamma, beta, y, mean, var, N, C, HxW, L, eps, fix_gamma, relu, workspace,
                             workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_infer_fwd(const float* const* x, const float* gamma, const float* beta,
                                       const float* moving_mean, const float* moving_var, float* const* y, int N,
                                       int C, const long* HxW, int L, float eps, int fix_gamma, int relu,
                                       void* stream) {
  return pbn_infer<float>(PBN_TABLE(x), gamma, beta, moving_mean, moving_var, PBN_OUT_TABLE(y), N, C, HxW, L, eps,
                          fix_gamma, relu, stream);
}
extern "C" int sd_pyramid_bn_infer_fwd_f16(const void* const* x, const float* gamma, const float* beta,
                                           const float* moving_mean, const float* moving_var, void* const* y, int N,
                                           int C, const long* HxW, int L, float eps, int fix_gamma, int relu,
                                           void* stream) {
  return pbn_infer<_Float16>(x, gamma, beta, moving_mean, moving_var, y, N, C, HxW, L, eps, fix_gamma, relu, stream);
}
extern "C" int sd_pyramid_bn_bwd_stats(const float* const* dy, const float* const* x, const float* mean,
                                       const float* var, const float* gamma, const float* beta, float* bpart, int N,
                                       int C, const long* HxW, int L, float eps, int fix_gamma, int relu,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  return pbn_bwd_stats<float>(PBN_TABLE(dy), PBN_TABLE(x), mean, var, gamma, beta, bpart, N, C, HxW, L, eps,
                              fix_gamma, relu, workspace, workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_bwd_stats_f16(const void* const* dy, const void* const* x, const float* mean,
                                           const float* var, const float* gamma, const float* beta, float* bpart,
                                           int N, int C, const long* HxW, int L, float eps, int fix_gamma, int relu,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return pbn_bwd_stats<_Float16>(dy, x, mean, var, gamma, beta, bpart, N, C, HxW, L, eps, fix_gamma, relu, workspace,
                                 workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_bwd_apply(const float* const* dy, const float* const* x, const float* mean,
                                       const float* var, const float* gamma, const float* beta, const float* bparts,
                                       int W, int rank, float* const* dx, float* dgamma, float* dbeta,
                                       float* moving_mean, float* moving_var, float momentum, int N, int C,
                                       const long* HxW, int L, float eps, int fix_gamma, int relu, void* workspace,
                                       size_t workspace_bytes, void* stream) {
  return pbn_bwd_apply<float>(PBN_TABLE(dy), PBN_TABLE(x), mean, var, gamma, beta, bparts, W, rank,
                              PBN_OUT_TABLE(dx), dgamma, dbeta, moving_mean, moving_var, momentum, N, C, HxW, L, eps,
                              fix_gamma, relu, workspace, workspace_bytes, stream);
}
extern "C" int sd_pyramid_bn_bwd_apply_f16(const void* const* dy, const void* const* x, const float* mean,
                                           const float* var, const float* gamma, const float* beta,
                                           const float* bparts, int W, int rank, void* const* dx, float* dgamma,
                                           float* dbeta, float* moving_mean, float* moving_var, float momentum, int N,
                                           int C, const long* HxW, int L, float eps, int fix_gamma, int relu,
                                           void* workspace, size_t workspace_bytes, void* stream) {
  return pbn_bwd_apply<_Float16>(dy, x, mean, var, gamma, beta, bparts, W, rank, dx, dgamma, dbeta, moving_mean,
                                 moving_var, momentum, N, C, HxW, L, eps, fix_gamma, relu, workspace, workspace_bytes,
                                 stream);
}
