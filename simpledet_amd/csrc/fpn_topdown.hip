// The FPN top-down pathway for gfx950: UpSampling(scale=2, nearest) -> slice_like(., lateral) -> add_n, the chain
// every FPN-style neck of the reference repeats per level (models/FPN/builder.py:444-524 three times,
// models/retinanet/builder.py:498-543 twice, ...), fp32 and fp16, NCHW.
//   the arithmetic (upstream MXNet operators, restated; they are not in the reference tree):
//     forward   out_l[n,c,y,x] = p_{l-1}[n,c,y>>1,x>>1] + lateral_l[n,c,y,x],  p_0 = top, p_l = out_l
//     backward  D_{L-1} = g_{L-1};  D_l = g_l + S_l;  d_top = S_0;  d_lateral_l = D_l
//               S_l[i,j] = (((+0.0f + D[2i,2j]) + D[2i,2j+1]) + D[2i+1,2j]) + D[2i+1,2j+1] over D = D_{l+1}, a
//               position at or beyond H_{l+1}, W_{l+1} skipped: mshadow's pool<red::sum> under the crop
// MI355X design: ONE launch each way for the whole chain; every tensor is read or written once.
//   A workgroup owns plane (n, c) and a tile of BR x BC elements of level 0, and with it, at level l, the rows
//   [r0 << l, r1 << l) and columns [c0 << l, c1 << l) clipped to H_l x W_l: every element of every level belongs
//   to exactly one workgroup, and everything it needs from the neighbouring level lies in the same workgroup's
//   tile.  The tile of an inner level (1 .. L-2) is kept in LDS as it is produced -- the rounded value that is
//   also stored -- and read from there by the next level; only level 0 (forward) and level L-1 (backward) are
//   read from memory.  BR x BC <= 16384 / 4^(L-1), so the finest tile has at most 16384 elements, the tile of
//   level L-2 4096 (LDS buffer A) and that of L-3 1024 (buffer B; the levels alternate): 20 KB in fp32.
//   BC covers the whole width where W_0 allows; the tile of a level is then one contiguous run of the plane.
//   Forward: a run is cut into 16-byte items (4 floats, 8 halves) from the first 16-byte boundary of the OUTPUT;
//   the elements in front of it and behind the last whole item go one by one.  The lateral is loaded by items
//   where it shares the output's phase and by elements where not; every run has its own phase (rows of 167 or 334
//   floats are no 16-byte multiples, and planes start anywhere), and no bit depends on any of them.
//   Backward: a thread makes two (fp32) or four (fp16) coarse elements from the 2 x 4 (2 x 8) fine ones above
//   them: 16 bytes per fine row where that row's phase allows, two 8-byte loads, halves two by two, or element
//   loads where not (a row of 334 floats puts every other row 8 bytes off), and 8 bytes of g_l and of the result.  The sums are fp32, in
//   the order above, whatever the access width.
//   fp16: one rounding to half per stored element, and the next level reads the rounded half (cast -> fp32 level
//   -> cast): an L-level call equals L-1 chained two-level calls bit for bit (the fp16 backward where the inner
//   g_l are NULL: a chain has to round S_l to half before an add outside it rounds again).
//   No workspace, no atomics, no host read: graph-capturable, and two calls give equal bits.
#include "common.h"
#include "../../include/simpledet_ops.h"

namespace sd {
namespace {

constexpr int kFtdT = 256;
constexpr int kFtdMaxL = 6;
constexpr int kFtdFinest = 16384;              // elements of a workgroup's finest tile, at most
constexpr int kFtdStageA = kFtdFinest / 4;     // level L-2, L-4
constexpr int kFtdStageB = kFtdFinest / 16;    // level L-3, L-5
constexpr long kFtdMaxElems = 2147483647L;     // element indices inside a tensor are 32-bit

struct FtdArgs {
  const void* in[kFtdMaxL];   // forward: top, lateral_1 ..      backward: -, g_1 .. g_{L-1} (inner ones may be null)
  void* out[kFtdMaxL];        // forward: -, out_1 ..            backward: d_top, d_lateral_1 .. (any may be null)
  int H[kFtdMaxL], W[kFtdMaxL];
  int L, BR, BC;
  unsigned tr, tc;            // tiles of a plane along its rows and columns
};

template <typename T>
struct alignas(16) FtdItem {
  T v[16 / sizeof(T)];
};
template <typename T>
struct alignas(8) FtdHalfItem {
  T v[8 / sizeof(T)];
};

template <typename T>
struct alignas(2 * sizeof(T)) FtdPair {
  T v[2];
};

struct FtdTile {
  int y0, y1, x0, x1;   // empty where the crop took everything: y1 <= y0 or x1 <= x0
  __device__ int rows() const { return y1 > y0 ? y1 - y0 : 0; }
  __device__ int cols() const { return x1 > x0 ? x1 - x0 : 0; }
};
__device__ __forceinline__ FtdTile ftd_tile(const FtdArgs& a, int l, int r0, int c0) {
  FtdTile t;
  const long y1 = (long)(r0 + a.BR) << l, x1 = (long)(c0 + a.BC) << l;
  const long y0 = (long)r0 << l, x0 = (long)c0 << l;
  t.y0 = (int)(y0 < a.H[l] ? y0 : a.H[l]);
  t.x0 = (int)(x0 < a.W[l] ? x0 : a.W[l]);
  t.y1 = (int)(y1 < a.H[l] ? y1 : a.H[l]);
  t.x1 = (int)(x1 < a.W[l] ? x1 : a.W[l]);
  return t;
}
__device__ __forceinline__ size_t ftd_plane(const FtdArgs& a, int l, unsigned plane) {
  return (size_t)plane * ((size_t)a.H[l] * (size_t)a.W[l]);
}

// ------------------------------------------------------------------------------------ forward ----
// one level: out = coarse[y >> 1, x >> 1] + lateral over the tile `t` of level l.  The coarse level is the plane
// `cg` in memory (pitch cw) or the LDS tile `cs` of origin (ct.y0, ct.x0) and pitch ct.cols(); `stage`, where not
// null, receives the tile as well.
template <typename T>
__device__ __forceinline__ void ftd_fwd_level(const T* cg, int cw, const T* cs, const FtdTile ct, const T* lat, T* out,
                                              T* stage, const FtdTile t, int W) {
  constexpr int V = 16 / sizeof(T);
  const int rows = t.rows(), cols = t.cols();
  if (rows == 0 || cols == 0) return;
  const int cpitch = ct.cols();
  auto coarse = [&](int y, int x) -> T {
    const int cy = y >> 1, cx = x >> 1;
    return cs ? cs[(cy - ct.y0) * cpitch + (cx - ct.x0)] : cg[(unsigned)cy * (unsigned)cw + (unsigned)cx];
  };
  const bool full = cols == W;                    // the tile is one contiguous run of the plane
  const int nruns = full ? 1 : rows;
  const unsigned runlen = full ? (unsigned)rows * (unsigned)W : (unsigned)cols;
  for (int r = 0; r < nruns; ++r) {
    const unsigned f0 = (unsigned)(t.y0 + r) * (unsigned)W + (unsigned)t.x0;
    unsigned head = (unsigned)(((16u - (unsigned)((uintptr_t)(out + f0) & 15u)) & 15u) / sizeof(T));
    if (head > runlen) head = runlen;
    const unsigned nv = (runlen - head) / V;
    const unsigned tail = runlen - head - nv * V;
    if (threadIdx.x < head + tail) {
      const unsigned k = threadIdx.x < head ? threadIdx.x : runlen - tail + (threadIdx.x - head);
      const unsigned f = f0 + k;
      const int y = (int)(f / (unsigned)W), x = (int)(f - (unsigned)y * (unsigned)W);
      const T v = coarse(y, x) + lat[f];
      out[f] = v;
      if (stage) stage[(y - t.y0) * cols + (x - t.x0)] = v;
    }
    const bool latvec = ((uintptr_t)(lat + f0 + head) & 15u) == 0;
    for (unsigned i = threadIdx.x; i < nv; i += kFtdT) {
      const unsigned f = f0 + head + i * V;
      FtdItem<T> a;
      if (latvec) {
        a = *reinterpret_cast<const FtdItem<T>*>(lat + f);
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) a.v[k] = lat[f + k];
      }
      int y = (int)(f / (unsigned)W), x = (int)(f - (unsigned)y * (unsigned)W);
      T o[V];
      if (x + V <= W) {
        // no row end inside the item: its V elements lie under V/2 coarse ones, or V/2 + 1 from an odd column
        const int cy = y >> 1, cx = x >> 1;
        const bool odd = (x & 1) != 0;
        T c[V / 2 + 1];
        if (cs) {   // (two branches: an LDS pointer and a global one stay what they are)
          const T* cp = cs + ((cy - ct.y0) * cpitch + (cx - ct.x0));
#pragma unroll
          for (int k = 0; k < V / 2; ++k) c[k] = cp[k];
          T last = c[V / 2 - 1];
          if (odd) last = cp[V / 2];
          c[V / 2] = last;
        } else {
          const T* cp = cg + ((unsigned)cy * (unsigned)cw + (unsigned)cx);
#pragma unroll
          for (int k = 0; k < V / 2; ++k) c[k] = cp[k];
          T last = c[V / 2 - 1];
          if (odd) last = cp[V / 2];
          c[V / 2] = last;
        }
#pragma unroll
        for (int k = 0; k < V; ++k) {
          const T ce = c[k >> 1], co = c[(k + 1) >> 1];
          o[k] = (odd ? co : ce) + a.v[k];
        }
      } else {
#pragma unroll
        for (int k = 0; k < V; ++k) {
          o[k] = coarse(y, x) + a.v[k];
          if (++x == W) { x = 0; ++y; }   // (only a full-width run crosses a row end)
        }
      }
      if (stage) {
        // the staged tile is laid out like the runs: row r of the tile, the run's elements in order
        T* sp = stage + ((unsigned)r * (unsigned)cols + (f - f0));
#pragma unroll
        for (int k = 0; k < V; ++k) sp[k] = o[k];
      }
      FtdItem<T> q;
#pragma unroll
      for (int k = 0; k < V; ++k) q.v[k] = o[k];
      *reinterpret_cast<FtdItem<T>*>(out + f) = q;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kFtdT) void ftd_fwd_kernel(FtdArgs a) {
  __shared__ T stA[kFtdStageA];
  __shared__ T stB[kFtdStageB];
  const unsigned tiles = a.tr * a.tc;
  const unsigned plane = blockIdx.x / tiles, tt = blockIdx.x - plane * tiles;
  const int r0 = (int)(tt / a.tc) * a.BR, c0 = (int)(tt % a.tc) * a.BC;
  FtdTile ct = ftd_tile(a, 0, r0, c0);
  const T* cs = nullptr;
  for (int l = 1; l < a.L; ++l) {
    const FtdTile t = ftd_tile(a, l, r0, c0);
    T* stage = l <= a.L - 2 ? (((a.L - 2 - l) & 1) ? stB : stA) : nullptr;
    const T* cg = static_cast<const T*>(a.in[0]) + ftd_plane(a, 0, plane);   // (read at l = 1 only)
    ftd_fwd_level<T>(cg, a.W[0], cs, ct, static_cast<const T*>(a.in[l]) + ftd_plane(a, l, plane),
                     static_cast<T*>(a.out[l]) + ftd_plane(a, l, plane), stage, t, a.W[l]);
    if (stage) __syncthreads();
    cs = stage;
    ct = t;
  }
}

// ----------------------------------------------------------------------------------- backward ----
// one level: D_l = g_l + S_l over the tile `t` of level l, S_l from the fine level l + 1 (H x W = fh x fw), which
// is the plane `fg` in memory or the LDS tile `fs` (origin ft.y0 / ft.x0, pitch ft.cols()).
template <typename T>
__device__ __forceinline__ void ftd_bwd_level(const T* fg, const T* fs, const FtdTile ft, int fh, int fw, const T* g,
                                              T* d, T* stage, const FtdTile t, int W) {
  constexpr int CO = 8 / sizeof(T);    // coarse elements of a thread: 2 floats, 4 halves (8 bytes)
  constexpr int FV = 2 * CO;           // fine elements per row above them: 16 bytes
  const int rows = t.rows(), cols = t.cols();
  if (rows == 0 || cols == 0) return;
  const int fpitch = ft.cols();
  const unsigned upr = (unsigned)(cols + CO - 1) / CO;
  const unsigned total = (unsigned)rows * upr;
  for (unsigned u = threadIdx.x; u < total; u += kFtdT) {
    const unsigned ry = u / upr;
    const int i = t.y0 + (int)ry, j = t.x0 + (int)(u - ry * upr) * CO;
    float D[2][FV];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int y = 2 * i + r, x = 2 * j;
#pragma unroll
      for (int k = 0; k < FV; ++k) D[r][k] = 0.f;
      if (y >= fh) continue;
      if (fs) {
        const T* p = fs + (y - ft.y0) * fpitch + (x - ft.x0);
#pragma unroll
        for (int k = 0; k < FV; ++k)
          if (x + k < fw) D[r][k] = (float)p[k];
      } else {
        const T* p = fg + ((unsigned)y * (unsigned)fw + (unsigned)x);
        if (x + FV <= fw && ((uintptr_t)p & 15u) == 0) {
          const FtdItem<T> q = *reinterpret_cast<const FtdItem<T>*>(p);
#pragma unroll
          for (int k = 0; k < FV; ++k) D[r][k] = (float)q.v[k];
        } else if (x + FV <= fw && ((uintptr_t)p & 7u) == 0) {
          const FtdHalfItem<T> q0 = *reinterpret_cast<const FtdHalfItem<T>*>(p);
          const FtdHalfItem<T> q1 = *reinterpret_cast<const FtdHalfItem<T>*>(p + CO);
#pragma unroll
          for (int k = 0; k < CO; ++k) {
            D[r][k] = (float)q0.v[k];
            D[r][CO + k] = (float)q1.v[k];
          }
        } else if (sizeof(T) == 2 && x + FV <= fw && ((uintptr_t)p & 3u) == 0) {
          // halves two by two: rows of 334 halves lie 4 or 12 bytes off every other time
#pragma unroll
          for (int k = 0; k < FV; k += 2) {
            const FtdPair<T> q = *reinterpret_cast<const FtdPair<T>*>(p + k);
            D[r][k] = (float)q.v[0];
            D[r][k + 1] = (float)q.v[1];
          }
        } else {
#pragma unroll
          for (int k = 0; k < FV; ++k)
            if (x + k < fw) D[r][k] = (float)p[k];
        }
      }
    }
    const unsigned f = (unsigned)i * (unsigned)W + (unsigned)j;
    const bool whole = j + CO <= t.x1;
    FtdHalfItem<T> gv, dv;
    if (g) {
      if (whole && ((uintptr_t)(g + f) & 7u) == 0) {
        gv = *reinterpret_cast<const FtdHalfItem<T>*>(g + f);
      } else {
#pragma unroll
        for (int c = 0; c < CO; ++c)
          if (j + c < t.x1) gv.v[c] = g[f + c];
      }
    }
#pragma unroll
    for (int c = 0; c < CO; ++c) {
      if (j + c >= t.x1) continue;
      // the window in row-major order from +0.0f.  A position beyond the fine level holds +0.0f here, and adding it
      // is leaving it out: S is never -0.0 (it starts at +0.0, and +0.0 + -0.0 = +0.0), so S + +0.0 = S in every bit
      float S = 0.f;
#pragma unroll
      for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int b = 0; b < 2; ++b) S = S + D[r][2 * c + b];
      dv.v[c] = g ? (T)((float)gv.v[c] + S) : (T)S;
      if (stage) stage[(i - t.y0) * cols + (j + c - t.x0)] = dv.v[c];
    }
    if (d) {
      if (whole && ((uintptr_t)(d + f) & 7u) == 0) {
        *reinterpret_cast<FtdHalfItem<T>*>(d + f) = dv;
      } else {
#pragma unroll
        for (int c = 0; c < CO; ++c)
          if (j + c < t.x1) d[f + c] = dv.v[c];
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kFtdT) void ftd_bwd_kernel(FtdArgs a) {
  __shared__ T stA[kFtdStageA];
  __shared__ T stB[kFtdStageB];
  const unsigned tiles = a.tr * a.tc;
  const unsigned plane = blockIdx.x / tiles, tt = blockIdx.x - plane * tiles;
  const int r0 = (int)(tt / a.tc) * a.BR, c0 = (int)(tt % a.tc) * a.BC;
  FtdTile ft = ftd_tile(a, a.L - 1, r0, c0);
  const T* fs = nullptr;
  for (int l = a.L - 2; l >= 0; --l) {
    const FtdTile t = ftd_tile(a, l, r0, c0);
    T* stage = l >= 1 ? (((a.L - 2 - l) & 1) ? stB : stA) : nullptr;
    const T* fg = static_cast<const T*>(a.in[a.L - 1]) + ftd_plane(a, a.L - 1, plane);   // (read at l = L-2 only)
    const T* g = (l >= 1 && a.in[l]) ? static_cast<const T*>(a.in[l]) + ftd_plane(a, l, plane) : nullptr;
    T* d = a.out[l] ? static_cast<T*>(a.out[l]) + ftd_plane(a, l, plane) : nullptr;
    ftd_bwd_level<T>(fg, fs, ft, a.H[l + 1], a.W[l + 1], g, d, stage, t, a.W[l]);
    if (stage) __syncthreads();
    fs = stage;
    ft = t;
  }
}

// plain copy of the finest gradient, for the caller that wants d_lateral_{L-1} as a buffer of its own
template <typename T>
__global__ __launch_bounds__(kFtdT) void ftd_copy_kernel(const T* src, T* dst, unsigned n) {
  constexpr unsigned V = 16 / sizeof(T);
  unsigned head = (unsigned)(((16u - (unsigned)((uintptr_t)dst & 15u)) & 15u) / sizeof(T));
  if (head > n) head = n;
  const unsigned nv = (n - head) / V, tail = n - head - nv * V;
  if (blockIdx.x == 0 && threadIdx.x < head + tail) {
    const unsigned k = threadIdx.x < head ? threadIdx.x : n - tail + (threadIdx.x - head);
    dst[k] = src[k];
  }
  const bool vec = ((uintptr_t)(src + head) & 15u) == 0;
  for (unsigned i = blockIdx.x * kFtdT + threadIdx.x; i < nv; i += gridDim.x * kFtdT) {
    const unsigned e = head + i * V;
    FtdItem<T> q;
    if (vec) {
      q = *reinterpret_cast<const FtdItem<T>*>(src + e);
    } else {
#pragma unroll
      for (unsigned k = 0; k < V; ++k) q.v[k] = src[e + k];
    }
    *reinterpret_cast<FtdItem<T>*>(dst + e) = q;
  }
}

// --------------------------------------------------------------------------------------- host ----
struct FtdRange {
  uintptr_t lo, hi;
  const char* what;
  int level;
};

static int ftd_plan(int N, int C, const int* hs, const int* ws, int L, FtdArgs* a, long* elems, bool* empty) {
  SD_REQUIRE(L >= 2 && L <= kFtdMaxL, "L=%d is outside 2..%d", L, kFtdMaxL);
  SD_REQUIRE(N >= 0 && C >= 0, "negative dimension (N=%d C=%d)", N, C);
  SD_REQUIRE(hs && ws, "null pointer: hs / ws");
  const long nc = (long)N * C;
  *empty = nc == 0;
  if (*empty) return SD_OK;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(hs[l] > 0 && ws[l] > 0, "level %d has a non-positive dimension (%d x %d)", l, hs[l], ws[l]);
    if (l)
      SD_REQUIRE((long)hs[l] <= 2L * hs[l - 1] && (long)ws[l] <= 2L * ws[l - 1],
                 "level %d (%d x %d) is larger than twice level %d (%d x %d)", l, hs[l], ws[l], l - 1, hs[l - 1],
                 ws[l - 1]);
  }
  for (int l = 0; l < L; ++l) {
    const long hw = (long)hs[l] * ws[l];
    if (hw > kFtdMaxElems / nc)
      return fail(SD_ERR_UNSUPPORTED, "level %d: N*C*H*W = %ld x %ld elements exceed the limit %ld", l, nc, hw,
                  kFtdMaxElems);
    elems[l] = nc * hw;
    a->H[l] = hs[l];
    a->W[l] = ws[l];
  }
  a->L = L;
  const int cap = kFtdFinest >> (2 * (L - 1));                 // elements of a level-0 tile: 4096 (L = 2) .. 16
  a->BC = ws[0] <= cap ? (ws[0] + 1) / 2 * 2 : cap;            // even: a fine tile starts on a multiple of 4
  a->BR = cap / a->BC < 1 ? 1 : cap / a->BC;
  if (a->BR > hs[0]) a->BR = hs[0];
  a->tr = (unsigned)cdiv(hs[0], a->BR);
  a->tc = (unsigned)cdiv(ws[0], a->BC);
  const long grid = nc * (long)a->tr * (long)a->tc;
  if (grid > kFtdMaxElems) return fail(SD_ERR_UNSUPPORTED, "%ld workgroups exceed the limit %ld", grid, kFtdMaxElems);
  return SD_OK;
}

static int ftd_check_ranges(const FtdRange* in, int nin, const FtdRange* out, int nout, size_t esz) {
  for (int i = 0; i < nin; ++i)
    SD_REQUIRE(in[i].lo % esz == 0, "%s %d is not aligned to its %zu-byte elements", in[i].what, in[i].level, esz);
  for (int o = 0; o < nout; ++o) {
    SD_REQUIRE(out[o].lo % esz == 0, "%s %d is not aligned to its %zu-byte elements", out[o].what, out[o].level, esz);
    for (int i = 0; i < nin; ++i)
      SD_REQUIRE(out[o].hi <= in[i].lo || in[i].hi <= out[o].lo, "%s %d overlaps %s %d", out[o].what, out[o].level,
                 in[i].what, in[i].level);
  }
  return SD_OK;
}

template <typename T>
static int ftd_fwd(const void* top, const void* const* lateral, void* const* out, int N, int C, const int* hs,
                   const int* ws, int L, void* stream) {
  FtdArgs a{};
  long elems[kFtdMaxL];
  bool empty = false;
  if (int e = ftd_plan(N, C, hs, ws, L, &a, elems, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(top && lateral && out, "null pointer");
  FtdRange in[kFtdMaxL], ou[kFtdMaxL];
  in[0] = {(uintptr_t)top, (uintptr_t)top + elems[0] * sizeof(T), "top", 0};
  a.in[0] = top;
  for (int l = 1; l < L; ++l) {
    SD_REQUIRE(lateral[l - 1] && out[l - 1], "null pointer: lateral / out of level %d", l);
    a.in[l] = lateral[l - 1];
    a.out[l] = out[l - 1];
    in[l] = {(uintptr_t)a.in[l], (uintptr_t)a.in[l] + elems[l] * sizeof(T), "lateral", l};
    ou[l - 1] = {(uintptr_t)a.out[l], (uintptr_t)a.out[l] + elems[l] * sizeof(T), "out", l};
  }
  if (int e = ftd_check_ranges(in, L, ou, L - 1, sizeof(T))) return e;
  const unsigned grid = (unsigned)((long)N * C * a.tr * a.tc);
  hipLaunchKernelGGL(ftd_fwd_kernel<T>, dim3(grid), dim3(kFtdT), 0, (hipStream_t)stream, a);
  note_dispatch("sd::ftd_fwd_kernel<%s> L=%d grid=%u tile=%dx%d tiles=%ux%u", sizeof(T) == 4 ? "f32" : "f16", L, grid,
                a.BR, a.BC, a.tr, a.tc);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int ftd_bwd(const void* const* g, void* d_top, void* const* d_lateral, int N, int C, const int* hs,
                   const int* ws, int L, void* stream) {
  FtdArgs a{};
  long elems[kFtdMaxL];
  bool empty = false;
  if (int e = ftd_plan(N, C, hs, ws, L, &a, elems, &empty)) return e;
  if (empty) return SD_OK;
  SD_REQUIRE(g && d_top, "null pointer");
  SD_REQUIRE(g[L - 2], "null pointer: the gradient of the finest level %d", L - 1);
  FtdRange in[kFtdMaxL], ou[kFtdMaxL];
  int nin = 0, nout = 0;
  a.out[0] = d_top;
  ou[nout++] = {(uintptr_t)d_top, (uintptr_t)d_top + elems[0] * sizeof(T), "d_top", 0};
  for (int l = 1; l < L; ++l) {
    a.in[l] = g[l - 1];
    if (a.in[l]) in[nin++] = {(uintptr_t)a.in[l], (uintptr_t)a.in[l] + elems[l] * sizeof(T), "g", l};
    a.out[l] = d_lateral ? d_lateral[l - 1] : nullptr;
    if (a.out[l]) ou[nout++] = {(uintptr_t)a.out[l], (uintptr_t)a.out[l] + elems[l] * sizeof(T), "d_lateral", l};
  }
  if (int e = ftd_check_ranges(in, nin, ou, nout, sizeof(T))) return e;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)((long)N * C * a.tr * a.tc);
  T* finest = static_cast<T*>(a.out[L - 1]);
  a.out[L - 1] = nullptr;   // the chain kernel writes levels 0 .. L-2; the finest gradient is a copy
  hipLaunchKernelGGL(ftd_bwd_kernel<T>, dim3(grid), dim3(kFtdT), 0, st, a);
  if (finest) {
    const unsigned n = (unsigned)elems[L - 1];
    const int cgrid = cdiv(cdiv(n, 16 / sizeof(T)), kFtdT * 4) < 2048 ? cdiv(cdiv(n, 16 / sizeof(T)), kFtdT * 4) : 2048;
    hipLaunchKernelGGL(ftd_copy_kernel<T>, dim3(cgrid), dim3(kFtdT), 0, st, static_cast<const T*>(a.in[L - 1]), finest,
                       n);
  }
  note_dispatch("sd::ftd_bwd_kernel<%s> L=%d grid=%u tile=%dx%d tiles=%ux%u%s", sizeof(T) == 4 ? "f32" : "f16", L,
                grid, a.BR, a.BC, a.tr, a.tc, finest ? " + sd::ftd_copy_kernel" : "");
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" int sd_fpn_topdown_fwd(const float* top, const float* const* lateral, float* const* out, int N, int C,
                                  const int* hs, const int* ws, int L, void* stream) {
  return ftd_fwd<float>(top, (const void* const*)lateral, (void* const*)out, N, C, hs, ws, L, stream);
}
extern "C" int sd_fpn_topdown_bwd(const float* const* g, float* d_top, float* const* d_lateral, int N, int C,
                                  const int* hs, const int* ws, int L, void* stream) {
  return ftd_bwd<float>((const void* const*)g, d_top, (void* const*)d_lateral, N, C, hs, ws, L, stream);
}
extern "C" int sd_fpn_topdown_fwd_f16(const void* top, const void* const* lateral, void* const* out, int N, int C,
                                      const int* hs, const int* ws, int L, void* stream) {
  return ftd_fwd<_Float16>(top, lateral, out, N, C, hs, ws, L, stream);
}
extern "C" int sd_fpn_topdown_bwd_f16(const void* const* g, void* d_top, void* const* d_lateral, int N, int C,
                                      const int* hs, const int* ws, int L, void* stream) {
  return ftd_bwd<_Float16>(g, d_top, d_lateral, N, C, hs, ws, L, stream);
}
