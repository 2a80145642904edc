// The merged-BN affine for gfx950: _contrib_BroadcastScale and the chain the reference's merge_bn builds behind
// every fixbn convolution, fp32 and fp16, NCHW.
//   reference (the spec): operator_cxx/contrib/broadcast_scale-inl.h:57-103 (y = data * scaler broadcast over the
//   channel axis; the backward writes the data gradient only) followed by upstream broadcast_add(beta), the
//   shortcut's elemwise add and relu (mshadow_op::relu: a > 0 ? a : 0): two to four full-size nodes forward, each
//   reading and writing the whole activation, and as many backward.
// MI355X design: one launch forward, one backward; x (and the shortcut) read once, y written once.
//   The tensor is ONE flat run of N*C*HxW elements cut into 16-byte items (4 floats, 8 halves) that start at the
//   first 16-byte boundary of the output (forward: y, backward: dx); the elements in front of that boundary and
//   behind the last whole item are done one by one by the first workgroup.  An input, or the backward's second
//   output, whose phase differs from the output's is moved by element accesses: pointers need element alignment
//   only, every tensor's phase is its own, and no bit depends on any of them.  A tile is 256 x 2 items (both
//   items of a thread are loaded before either is stored); the grid is capped at 2048 workgroups that stride over
//   the tiles.  The channel of an item is (e / HxW) % C of its first element e by two multiply-high divisions
//   (Granlund-Montgomery, exact for every 32-bit e); an item that crosses a plane boundary -- HxW is often odd --
//   takes the next channel's gamma / beta for the elements behind it (planes shorter than an item, HxW < 4 or 8,
//   repeat the division per element).  No 64-bit divide anywhere.
//   Every element depends on the inputs at its own index alone and a thread has loaded them before it stores, so
//   y may be x or the residual, and dx / dres may be dy.
//   Arithmetic: every step is rounded on its own (-ffp-contract=off; in fp16 the native half operations, which
//   are the float operation rounded once to half -- mshadow's half_t and numpy's float16).
//   dbeta (normally not requested: fixed_param holds beta) is a sum in a fixed order, taken BEFORE the element
//   kernel because dx may overwrite dy:
//     sba_dbeta_partial_kernel  a workgroup per (plane, segment of 8192 elements): each thread sums its items
//                               in order (an item's elements pairwise), then the butterfly and the four waves left
//                               to right -> one float of the workspace, which therefore needs no clearing
//     sba_dbeta_finish_kernel   a wave per channel: lanes stride the channel's N x segments partials, the butterfly
//   Items there start at the segment's first element whatever the pointers' phase, so the order, and with it every
//   bit, is independent of alignment.  No floating-point atomics: two calls give equal bits.
#include "common.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <initializer_list>

namespace sd {
namespace {

constexpr int kSbaT = 256;
constexpr int kSbaU = 2;                     // items per thread and tile
constexpr int kSbaMaxGrid = 2048;
constexpr long kSbaMaxElems = 2147483647L;   // element indices are 32-bit inside the kernels
constexpr unsigned kSbaSeg = 8192;           // elements per dbeta segment
constexpr int kSbaSumGrid = 8192;

// n / d for every 32-bit n by one multiply-high (Granlund, Montgomery 1994, figure 4.1)
struct SbaDiv {
  unsigned d, m, s1, s2;
};
static SbaDiv sba_div(unsigned d) {
  unsigned L = 0;
  while ((1ull << L) < d) ++L;
  SbaDiv r;
  r.d = d;
  r.m = (unsigned)(((1ull << 32) * ((1ull << L) - d)) / d + 1);
  r.s1 = L < 1 ? L : 1;
  r.s2 = L > 1 ? L - 1 : 0;
  return r;
}
__device__ __forceinline__ unsigned sba_quot(unsigned n, const SbaDiv& d) {
  const unsigned t = __umulhi(d.m, n);
  return (t + ((n - t) >> d.s1)) >> d.s2;
}

struct SbaArgs {
  const void* in0;    // forward: x          backward: dy
  const void* in1;    // forward: residual   backward: y      (may be null)
  const void* gamma;
  const void* beta;   // forward only, may be null
  void* out0;         // forward: y          backward: dx
  void* out1;         // backward: dres, may be null
  SbaDiv hw, c;
  unsigned total, head, nv, tail, tiles;
  int act;
  int vec_in0, vec_in1, vec_out1;   // this tensor's items lie on 16-byte boundaries
};

template <typename T>
struct alignas(16) SbaItem {
  T v[16 / sizeof(T)];
};

template <typename T>
__device__ __forceinline__ SbaItem<T> sba_ld(const T* p, bool vec) {
  constexpr int V = 16 / sizeof(T);
  if (vec) return *reinterpret_cast<const SbaItem<T>*>(p);
  SbaItem<T> r;
#pragma unroll
  for (int k = 0; k < V; ++k) r.v[k] = p[k];
  return r;
}
template <typename T>
__device__ __forceinline__ void sba_st(T* p, bool vec, const SbaItem<T>& r) {
  constexpr int V = 16 / sizeof(T);
  if (vec) {
    *reinterpret_cast<SbaItem<T>*>(p) = r;
    return;
  }
#pragma unroll
  for (int k = 0; k < V; ++k) p[k] = r.v[k];
}

__device__ __forceinline__ unsigned sba_channel(unsigned e, const SbaArgs& a, unsigned* rem = nullptr) {
  const unsigned p = sba_quot(e, a.hw);
  if (rem) *rem = e - p * a.hw.d;
  return p - sba_quot(p, a.c) * a.c.d;
}

// t = x * g; u = t + b; v = u + r; relu: four operations, each rounded to T
template <typename T>
__device__ __forceinline__ T sba_fwd_one(T x, T g, T b, T r, bool has_b, bool has_r, bool act) {
  const T t = x * g;
  const T u = has_b ? (T)(t + b) : t;
  const T v = has_r ? (T)(u + r) : u;
  return act ? (v > (T)0 ? v : (T)0) : v;
}
// g1 = dy * relu_grad(y) as a product: an infinite dy over a dead unit gives NaN, as the reference's expression does
template <typename T>
__device__ __forceinline__ T sba_g1(T dy, T y, bool act) {
  return act ? (T)(dy * (y > (T)0 ? (T)1 : (T)0)) : dy;
}

template <typename T, bool BWD>
__device__ __forceinline__ void sba_one(const SbaArgs& a, unsigned e) {
  const T* in0 = static_cast<const T*>(a.in0);
  const T* in1 = static_cast<const T*>(a.in1);
  const unsigned c = sba_channel(e, a);
  const T g = static_cast<const T*>(a.gamma)[c];
  if (BWD) {
    const T g1 = sba_g1<T>(in0[e], a.act ? in1[e] : (T)0, a.act != 0);
    if (a.out1) static_cast<T*>(a.out1)[e] = g1;
    static_cast<T*>(a.out0)[e] = g1 * g;
  } else {
    const T b = a.beta ? static_cast<const T*>(a.beta)[c] : (T)0;
    const T r = in1 ? in1[e] : (T)0;
    static_cast<T*>(a.out0)[e] = sba_fwd_one<T>(in0[e], g, b, r, a.beta != nullptr, in1 != nullptr, a.act != 0);
  }
}

template <typename T, bool BWD>
__global__ __launch_bounds__(kSbaT) void sba_map_kernel(SbaArgs a) {
  constexpr int V = 16 / sizeof(T);
  using Item = SbaItem<T>;
  const T* in0 = static_cast<const T*>(a.in0);
  const T* in1 = static_cast<const T*>(a.in1);
  const T* gam = static_cast<const T*>(a.gamma);
  const T* bet = static_cast<const T*>(a.beta);
  T* out0 = static_cast<T*>(a.out0);
  T* out1 = static_cast<T*>(a.out1);
  const bool use1 = BWD ? a.act != 0 : in1 != nullptr;   // the backward reads y only under act
  if (blockIdx.x == 0 && threadIdx.x < a.head + a.tail) {
    const unsigned t = threadIdx.x;
    sba_one<T, BWD>(a, t < a.head ? t : a.total - a.tail + (t - a.head));
  }
  for (unsigned tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const unsigned i0 = tile * (unsigned)(kSbaT * kSbaU) + threadIdx.x;
    Item A[kSbaU], B[kSbaU];
#pragma unroll
    for (int k = 0; k < kSbaU; ++k) {
      const unsigned i = i0 + k * kSbaT;
      if (i < a.nv) {
        const unsigned e = a.head + i * V;
        A[k] = sba_ld<T>(in0 + e, a.vec_in0);
        if (use1) B[k] = sba_ld<T>(in1 + e, a.vec_in1);
      }
    }
#pragma unroll
    for (int k = 0; k < kSbaU; ++k) {
      const unsigned i = i0 + k * kSbaT;
      if (i >= a.nv) continue;
      const unsigned e = a.head + i * V;
      unsigned rem;
      const unsigned c0 = sba_channel(e, a, &rem);
      T g[V], b[V];
      if (a.hw.d >= (unsigned)V) {
        // at most one plane boundary inside the item: the elements behind it belong to the next channel
        const bool cross = rem + V > a.hw.d;
        const unsigned c1 = !cross ? c0 : c0 + 1 == a.c.d ? 0u : c0 + 1;
        const T g0 = gam[c0], g1 = gam[c1];
        const T b0 = (!BWD && bet) ? bet[c0] : (T)0, b1 = (!BWD && bet) ? bet[c1] : (T)0;
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const bool next = rem + j >= a.hw.d;
          g[j] = next ? g1 : g0;
          b[j] = next ? b1 : b0;
        }
      } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
          const unsigned c = sba_channel(e + j, a);
          g[j] = gam[c];
          b[j] = (!BWD && bet) ? bet[c] : (T)0;
        }
      }
      Item r0, r1;
#pragma unroll
      for (int j = 0; j < V; ++j) {
        if (BWD) {
          const T g1 = sba_g1<T>(A[k].v[j], use1 ? B[k].v[j] : (T)0, a.act != 0);
          r1.v[j] = g1;
          r0.v[j] = g1 * g[j];
        } else {
          r0.v[j] = sba_fwd_one<T>(A[k].v[j], g[j], b[j], use1 ? B[k].v[j] : (T)0, bet != nullptr, use1, a.act != 0);
        }
      }
      if (BWD && out1) sba_st<T>(out1 + e, a.vec_out1, r1);
      sba_st<T>(out0 + e, true, r0);
    }
  }
}

// sum of g1 over one (plane, segment), in float, in an order the pointers' phase does not enter
template <typename T>
__global__ __launch_bounds__(kSbaT) void sba_dbeta_partial_kernel(const T* dy, const T* y, float* part, unsigned HW,
                                                                  unsigned S, unsigned units, int act) {
  constexpr int V = 16 / sizeof(T);
  __shared__ float red[kSbaT / kWave];
  for (unsigned u = blockIdx.x; u < units; u += gridDim.x) {
    const unsigned plane = u / S, s = u - plane * S;
    const unsigned first = s * kSbaSeg;
    const unsigned len = HW - first < kSbaSeg ? HW - first : kSbaSeg;
    const T* gp = dy + ((size_t)plane * HW + first);
    const T* yp = act ? y + ((size_t)plane * HW + first) : nullptr;
    const bool gvec = ((uintptr_t)gp & 15) == 0, yvec = ((uintptr_t)yp & 15) == 0;
    const unsigned nv = len / V;
    float acc = 0.f;
    for (unsigned i = threadIdx.x; i < nv; i += kSbaT) {
      const SbaItem<T> g = sba_ld<T>(gp + i * V, gvec);
      SbaItem<T> w;
      if (act) w = sba_ld<T>(yp + i * V, yvec);
      float f[V];
#pragma unroll
      for (int j = 0; j < V; ++j) f[j] = (float)sba_g1<T>(g.v[j], act ? w.v[j] : (T)0, act != 0);
#pragma unroll
      for (int w2 = 1; w2 < V; w2 *= 2)
#pragma unroll
        for (int j = 0; j < V; j += 2 * w2) f[j] = f[j] + f[j + w2];
      acc += f[0];
    }
    const unsigned done = nv * V;
    if (threadIdx.x < len - done) {
      const unsigned j = done + threadIdx.x;
      acc += (float)sba_g1<T>(gp[j], act ? yp[j] : (T)0, act != 0);
    }
    acc = block_sum_f32<kSbaT, true>(acc, red);
    if (threadIdx.x == 0) part[u] = acc;
  }
}

// a wave per channel: lanes stride its N * S partials (n outer, segment inner), then the butterfly
__global__ __launch_bounds__(kSbaT) void sba_dbeta_finish_kernel(const float* part, float* dbeta, unsigned N,
                                                                 unsigned C, unsigned S) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  const unsigned c = blockIdx.x * (kSbaT / kWave) + threadIdx.x / kWave;
  if (c >= C) return;
  float acc = 0.f;
  unsigned n = lane / S, s = lane - n * S;   // j = n * S + s, j = lane, lane + 64, ...
  const unsigned dn = kWave / S, ds = kWave - dn * S;
  while (n < N) {
    acc += part[((size_t)n * C + c) * S + s];
    n += dn;
    s += ds;
    if (s >= S) { s -= S; ++n; }
  }
  acc = wave_sum_f32(acc);
  if (lane == 0) dbeta[c] = acc;
}

struct SbaPlan {
  long total;
  unsigned S;        // dbeta segments per plane
  size_t part_bytes;
};

static int sba_plan(int N, int C, long HxW, int act, SbaPlan* p, bool* empty) {
  SD_REQUIRE(N >= 0 && C >= 0 && HxW >= 0, "negative dimension (N=%d C=%d HxW=%ld)", N, C, HxW);
  SD_REQUIRE(act == 0 || act == 1, "act=%d is neither 0 (none) nor 1 (relu)", act);
  const long nc = (long)N * C;
  *empty = nc == 0 || HxW == 0;
  if (*empty) return SD_OK;
  if (HxW > kSbaMaxElems / nc)
    return fail(SD_ERR_UNSUPPORTED, "N*C*HxW = %ld x %ld elements exceed the limit %ld", nc, HxW, kSbaMaxElems);
  p->total = nc * HxW;
  p->S = (unsigned)((HxW + kSbaSeg - 1) / kSbaSeg);
  p->part_bytes = (size_t)nc * p->S * sizeof(float);
  return SD_OK;
}
static size_t sba_need(const SbaPlan& p) { return 256 + round256(p.part_bytes); }

static bool sba_elem_aligned(size_t esz, std::initializer_list<const void*> ps) {
  for (const void* q : ps)
    if ((uintptr_t)q % esz) return false;
  return true;
}

// the flat cut of the element kernels about out0's first 16-byte boundary
template <typename T>
static void sba_cut(SbaArgs& a, const SbaPlan& p, int C, long HxW) {
  constexpr unsigned V = 16 / sizeof(T);
  a.hw = sba_div((unsigned)HxW);
  a.c = sba_div((unsigned)C);
  a.total = (unsigned)p.total;
  const unsigned h = (unsigned)(((16u - (unsigned)((uintptr_t)a.out0 & 15u)) & 15u) / sizeof(T));
  a.head = h < a.total ? h : a.total;
  a.nv = (a.total - a.head) / V;
  a.tail = a.total - a.head - a.nv * V;
  a.tiles = (a.nv + kSbaT * kSbaU - 1) / (kSbaT * kSbaU);
  auto vec = [&](const void* q) { return q && (((uintptr_t)q + a.head * sizeof(T)) & 15u) == 0; };
  a.vec_in0 = vec(a.in0);
  a.vec_in1 = vec(a.in1);
  a.vec_out1 = vec(a.out1);
}
static int sba_grid(const SbaArgs& a) { return a.tiles < (unsigned)kSbaMaxGrid ? (a.tiles ? (int)a.tiles : 1) : kSbaMaxGrid; }
static const char* sba_ph(const void* q, int vec) { return !q ? "-" : vec ? "vec" : "narrow"; }

template <typename T>
static int sba_fwd(const void* x, const void* gamma, const void* beta, const void* residual, void* y, int N, int C,
                   long HxW, int act, void* stream) {
  SbaPlan p{};
  bool empty = false;
  if (int e = sba_plan(N, C, HxW, act, &p, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(x && gamma && y, "null pointer");
  SD_REQUIRE(sba_elem_aligned(sizeof(T), {x, gamma, beta, residual, y}), "a pointer is not aligned to its %zu-byte elements",
             sizeof(T));
  SbaArgs a{};
  a.in0 = x; a.in1 = residual; a.gamma = gamma; a.beta = beta; a.out0 = y; a.act = act;
  sba_cut<T>(a, p, C, HxW);
  const int grid = sba_grid(a);
  hipLaunchKernelGGL((sba_map_kernel<T, false>), dim3(grid), dim3(kSbaT), 0, (hipStream_t)stream, a);
  note_dispatch("sd::sba_fwd_kernel<%s> grid=%d tiles=%u (x:%s residual:%s)", sizeof(T) == 4 ? "f32" : "f16", grid,
                a.tiles, sba_ph(x, a.vec_in0), sba_ph(residual, a.vec_in1));
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int sba_bwd(const void* dy, const void* y, const void* gamma, void* dx, void* dres, float* dbeta, int N, int C,
                   long HxW, int act, void* workspace, size_t workspace_bytes, void* stream) {
  SbaPlan p{};
  bool empty = false;
  if (int e = sba_plan(N, C, HxW, act, &p, &empty)) return e;
  if (empty) return SD_OK;   // (dbeta is a sum over nothing; like every empty call, nothing is written)
  SD_REQUIRE(dy && gamma && dx, "null pointer");
  SD_REQUIRE(!act || y, "null pointer: act = 1 reads y");
  SD_REQUIRE(sba_elem_aligned(sizeof(T), {dy, y, gamma, dx, dres}), "a pointer is not aligned to its %zu-byte elements",
             sizeof(T));
  SD_REQUIRE(sba_elem_aligned(sizeof(float), {dbeta}), "dbeta is not aligned to 4 bytes");
  if (dbeta && !(workspace && workspace_bytes >= sba_need(p)))
    return fail(SD_ERR_WORKSPACE, "scale_bias_act_bwd workspace too small for dbeta: %zu < %zu bytes",
                workspace ? workspace_bytes : (size_t)0, sba_need(p));
  hipStream_t st = (hipStream_t)stream;
  const char* tn = sizeof(T) == 4 ? "f32" : "f16";
  if (dbeta) {
    float* part = reinterpret_cast<float*>(round256((size_t)(uintptr_t)workspace));
    const long units = (long)N * C * p.S;
    const int grid = units < kSbaSumGrid ? (int)units : kSbaSumGrid;
    hipLaunchKernelGGL(sba_dbeta_partial_kernel<T>, dim3(grid), dim3(kSbaT), 0, st, static_cast<const T*>(dy),
                       static_cast<const T*>(y), part, (unsigned)HxW, p.S, (unsigned)units, act);
    hipLaunchKernelGGL(sba_dbeta_finish_kernel, dim3(cdiv(C, kSbaT / kWave)), dim3(kSbaT), 0, st, part, dbeta,
                       (unsigned)N, (unsigned)C, p.S);
  }
  SbaArgs a{};
  a.in0 = dy; a.in1 = act ? y : nullptr; a.gamma = gamma; a.out0 = dx; a.out1 = dres; a.act = act;
  sba_cut<T>(a, p, C, HxW);
  const int grid = sba_grid(a);
  hipLaunchKernelGGL((sba_map_kernel<T, true>), dim3(grid), dim3(kSbaT), 0, st, a);
  note_dispatch("%ssd::sba_bwd_kernel<%s> grid=%d tiles=%u (dy:%s y:%s dres:%s)",
                dbeta ? "sd::sba_dbeta_partial_kernel + sd::sba_dbeta_finish_kernel + " : "", tn, grid, a.tiles,
                sba_ph(dy, a.vec_in0), sba_ph(a.in1, a.vec_in1), sba_ph(dres, a.vec_out1));
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_scale_bias_act_workspace_bytes(int N, int C, long HxW) {
  SbaPlan p{};
  bool empty = false;
  if (sba_plan(N, C, HxW, 0, &p, &empty) != SD_OK || empty) return 256;
  return sba_need(p);
}

extern "C" int sd_scale_bias_act_fwd(const float* x, const float* gamma, const float* beta, const float* residual,
                                     float* y, int N, int C, long HxW, int act, void* stream) {
  return sba_fwd<float>(x, gamma, beta, residual, y, N, C, HxW, act, stream);
}
extern "C" int sd_scale_bias_act_bwd(const float* dy, const float* y, const float* gamma, float* dx, float* dres,
                                     float* dbeta, int N, int C, long HxW, int act, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  return sba_bwd<float>(dy, y, gamma, dx, dres, dbeta, N, C, HxW, act, workspace, workspace_bytes, stream);
}
extern "C" int sd_scale_bias_act_fwd_f16(const void* x, const void* gamma, const void* beta, const void* residual,
                                         void* y, int N, int C, long HxW, int act, void* stream) {
  return sba_fwd<_Float16>(x, gamma, beta, residual, y, N, C, HxW, act, stream);
}
extern "C" int sd_scale_bias_act_bwd_f16(const void* dy, const void* y, const void* gamma, void* dx, void* dres,
                                         float* dbeta, int N, int C, long HxW, int act, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  return sba_bwd<_Float16>(dy, y, gamma, dx, dres, dbeta, N, C, HxW, act, workspace, workspace_bytes, stream);
}
