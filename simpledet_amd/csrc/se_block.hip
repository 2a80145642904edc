// The squeeze-and-excitation block of the SE-ResNet / EfficientNet backbones and the SE mask head for gfx950, fp32 and
// fp16, NCHW, forward and backward (include/simpledet_ops.h has the contract).
//
// The reference's se() (models/efficientnet/builder.py:17-27) is seven graph nodes: mean over W, mean over H, a 1x1
// conv, relu6, a 1x1 conv, sigmoid, broadcast_mul.  Here:
//   gap[n,c] = (sum of the plane) / (float)HW;  z1 = w1 gap + b1;  h = min(max(z1, 0), 6);  z2 = w2 h + b2;
//   a = 1 / (1 + expf(-z2));  y = x * a[n,c]
//   s[n,c] = sum dy * x;  dz2 = s * (a * (1 - a));  dh = w2^T dz2;  dz1 = 0 <= z1 <= 6 ? dh : 0;
//   g[n,c] = (w1^T dz1)[n,c] / (float)HW;  dx = dy * a[n,c] + g[n,c]
//   dw2 = sum_n dz2 (x) h;  db2 = sum_n dz2;  dw1 = sum_n dz1 (x) gap;  db1 = sum_n dz1   (images in order)
// all in fp32, every step rounded on its own (-ffp-contract=off), halves widened on load and rounded once on store.
//
// Two-pass path.
//   se_reduce_kernel<T, BWD>   the plane sums (x, or dy * x).  Planes of up to kSeWavePlane elements: a wave per plane,
//                              four planes of ONE image per workgroup, the cross-lane sum on the VALU.  Larger planes
//                              (or a forced split): a workgroup per (plane, chunk).  Every sum goes to the workspace as
//                              a partial; a workgroup then takes an integer ticket of its image, and the one that
//                              draws the last ticket runs the image's gate: the partials of a plane are added in chunk
//                              order, so no bit depends on who finishes last.
//                                forward:  gap, and z1 = w1 gap + b1 (a wave per row of w1, four rows in flight)
//                                backward: dz2, dh = w2^T dz2 (a thread per column, the rows cut into segments that
//                                          are added in order), dz1
//   se_apply_kernel<T, BWD>    y = x * a / dx = dy * a + g.  The per-plane half of the gate lives HERE, where it is
//                              parallel over all planes: every wave that works on plane (n, c) first forms
//                              a[n,c] = sigmoid(w2[c,:] . h[n,:] + b2[c]) (forward) or g[n,c] = (w1[:,c] . dz1[n,:]) / HW
//                              (backward) in one fixed order, so every chunk of a plane uses equal bits; the first
//                              chunk stores them.
//   se_wgrad_kernel            a thread per weight-gradient element, images added in order from dz2 / dz1 / gap / z1:
//                              the (N, C, Cr) partial blocks are never materialised.
// Resident path.  One workgroup per image whose C * HW elements fit in LDS next to the gate's vectors: x (backward:
//   dy; x itself is needed by the sum alone) is read once into LDS while it is summed, the whole gate runs in the
//   workgroup, and the result is written from LDS: two tensor passes forward, three backward.  No ticket.
// Loads and stores are 16-byte vectors from the first 16-byte boundary of a run, with element accesses in front and
// behind, so pointers need element alignment only.  No floating-point atomics, no memset, no host read: the tickets are
// cleared by a kernel at the head of a call (a fresh workspace holds arbitrary bytes), everything else that is read was
// written by the same call.
#include "common.h"
#include "norm_common.h"
#include "../../include/simpledet_ops.h"

namespace sd {
namespace {

constexpr int kSeT = 256;                  // threads of the two-pass kernels
constexpr int kSeResT = 512;               // threads of the resident kernels
constexpr int kSeMaxC = 4096, kSeMaxCr = 512;
constexpr long kSeMaxElems = 2147483647L;
constexpr unsigned kSeWavePlane = 4096;    // planes up to this many elements take one wave each
constexpr unsigned kSeApplyChunk = 8192;   // elements of a workgroup of the apply kernel on larger planes
constexpr unsigned kSeReduceChunk = 8192;  // smallest chunk the automatic split makes
constexpr int kSeMaxSplit = 1024;
constexpr size_t kSeLds = 160 * 1024;
constexpr unsigned kSeResHead = kSeMaxCr + kSeResT;   // floats in front of the resident gate's per-channel vector

struct SeArgs {
  const void* x;
  const void* dy;          // backward
  void* out;               // y / dx
  const void *w1, *b1, *w2, *b2;
  float *gap, *z1, *a, *g; // forward: gap, z1, a are written; backward: read, and g written
  float* partial;          // (N, C, S)
  int* ticket;             // (N)
  float *dz2, *dz1;        // (N, C), (N, Cr): what se_wgrad_kernel reads
  unsigned N, C, Cr, HW;
  unsigned S, chunk;       // chunks per plane of the reduction, elements per chunk
  unsigned bpi;            // workgroups of the reduction per image
  unsigned acp;            // chunks per plane of the apply kernel
  float hw;                // (float)HW
};

// This thread's share of the sum of x (MUL: of dy * x) over a run of `len` elements worked on by G threads: the
// element in front of the boundary, its vectors in order (a vector's terms pairwise), the element behind.  STASH keeps
// the run (MUL: dy's) in `stash`.
template <typename T, int G, bool MUL, bool STASH>
__device__ __forceinline__ float se_run_sum(const T* x, const T* dy, unsigned len, unsigned t, T* stash) {
  constexpr unsigned V = 16 / sizeof(T);
  const unsigned head = head_to_16(x, len);
  const bool dyvec = MUL && (((uintptr_t)(dy + head)) & 15u) == 0;
  float acc = 0.f;
  auto one = [&](unsigned i) {
    const T xv = x[i];
    if (MUL) {
      const T dv = dy[i];
      if (STASH) stash[i] = dv;
      acc += (float)dv * (float)xv;
    } else {
      if (STASH) stash[i] = xv;
      acc += (float)xv;
    }
  };
  if (t < head) one(t);
  const unsigned nv = (len - head) / V;
  const Vec16<T>* xp = reinterpret_cast<const Vec16<T>*>(x + head);
  for (unsigned j = t; j < nv; j += G) {
    const Vec16<T> a = xp[j];
    Vec16<T> b;
    if (MUL) {
      if (dyvec) {
        b = reinterpret_cast<const Vec16<T>*>(dy + head)[j];
      } else {
#pragma unroll
        for (unsigned k = 0; k < V; ++k) b.e[k] = dy[head + j * V + k];
      }
    }
    float f[V];
#pragma unroll
    for (unsigned k = 0; k < V; ++k) f[k] = MUL ? (float)b.e[k] * (float)a.e[k] : (float)a.e[k];
#pragma unroll
    for (unsigned w = 1; w < V; w *= 2)
#pragma unroll
      for (unsigned k = 0; k < V; k += 2 * w) f[k] = f[k] + f[k + w];
    acc += f[0];
    if (STASH) {
#pragma unroll
      for (unsigned k = 0; k < V; ++k) stash[head + j * V + k] = MUL ? b.e[k] : a.e[k];
    }
  }
  const unsigned done = head + nv * V;
  if (t < len - done) one(done + t);
  return acc;
}

// out = in * a (ADD: + g) over a run, rounded once; 16-byte stores from out's boundary, 16-byte loads where `in`
// shares its phase (never from LDS, whose copy has no phase to share)
template <typename T, int G, bool ADD, bool LDS_IN>
__device__ __forceinline__ void se_run_apply(const T* in, T* out, unsigned len, unsigned t, float a, float g) {
  constexpr unsigned V = 16 / sizeof(T);
  const unsigned head = head_to_16(out, len);
  const bool invec = !LDS_IN && (((uintptr_t)(in + head)) & 15u) == 0;
  auto f = [&](T v) -> T {
    float r = (float)v * a;
    if (ADD) r = r + g;
    return (T)r;
  };
  if (t < head) out[t] = f(in[t]);
  const unsigned nv = (len - head) / V;
  Vec16<T>* op = reinterpret_cast<Vec16<T>*>(out + head);
  for (unsigned j = t; j < nv; j += G) {
    Vec16<T> v;
    if (invec) {
      v = reinterpret_cast<const Vec16<T>*>(in + head)[j];
    } else {
#pragma unroll
      for (unsigned k = 0; k < V; ++k) v.e[k] = in[head + j * V + k];
    }
#pragma unroll
    for (unsigned k = 0; k < V; ++k) v.e[k] = f(v.e[k]);
    op[j] = v;
  }
  const unsigned done = head + nv * V;
  if (t < len - done) out[done + t] = f(in[done + t]);
}

__device__ __forceinline__ float se_clip(float z) { return fminr(fmaxr(z, 0.f), 6.f); }

// a[n,c] by one wave: the lanes stride row c of w2 against h = clip(z1[n,:]), the wave sum, the bias, the sigmoid
template <typename T>
__device__ __forceinline__ float se_plane_a(const SeArgs& p, unsigned c, const float* z1n, unsigned lane) {
  const T* row = static_cast<const T*>(p.w2) + (size_t)c * p.Cr;
  float acc = 0.f;
  for (unsigned j = lane; j < p.Cr; j += kWave) acc += (float)row[j] * se_clip(z1n[j]);
  float z = wave_sum_f32(acc);
  if (p.b2) z = z + (float)static_cast<const T*>(p.b2)[c];
  return 1.0f / (1.0f + expf(-z));
}

// g[n,c] by one wave: the lanes stride column c of w1 against dz1[n,:]
template <typename T>
__device__ __forceinline__ float se_plane_g(const SeArgs& p, unsigned c, const float* dz1n, unsigned lane) {
  const T* col = static_cast<const T*>(p.w1) + c;
  float acc = 0.f;
  for (unsigned j = lane; j < p.Cr; j += kWave) acc += (float)col[(size_t)j * p.C] * dz1n[j];
  return wave_sum_f32(acc) / p.hw;
}

// z1[n,:] = w1 gap + b1 by NT threads: a wave per row, four rows in flight; s_z1 (LDS, may be null) keeps a copy
template <typename T, int NT>
__device__ __forceinline__ void se_gate_z1(const SeArgs& p, unsigned n, const float* s_gap, float* s_z1) {
  constexpr unsigned NW = NT / kWave, R = 4;
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const T* w1 = static_cast<const T*>(p.w1);
  for (unsigned j0 = wave * R; j0 < p.Cr; j0 += NW * R) {
    float acc[R];
#pragma unroll
    for (unsigned r = 0; r < R; ++r) acc[r] = 0.f;
    for (unsigned c = lane; c < p.C; c += kWave) {
      const float gv = s_gap[c];
#pragma unroll
      for (unsigned r = 0; r < R; ++r)
        if (j0 + r < p.Cr) acc[r] += (float)w1[(size_t)(j0 + r) * p.C + c] * gv;
    }
#pragma unroll
    for (unsigned r = 0; r < R; ++r) {
      float z = wave_sum_f32(acc[r]);
      if (j0 + r < p.Cr) {
        if (p.b1) z = z + (float)static_cast<const T*>(p.b1)[j0 + r];
        if (lane == 0) {
          p.z1[(size_t)n * p.Cr + j0 + r] = z;
          if (s_z1) s_z1[j0 + r] = z;
        }
      }
    }
  }
}

// The backward gate behind s_c[c] = dz2[n,c] (LDS): dh = w2^T dz2 with a thread per column and the rows cut into
// NT / roundup(Cr, 64) segments whose sums are added in order; dz1 by the clip's inclusive rule.  s_p: NT floats;
// s_dz1 (LDS, may be null) keeps a copy of dz1.  Ends behind a barrier.
template <typename T, int NT>
__device__ __forceinline__ void se_gate_bwd(const SeArgs& p, unsigned n, const float* s_c, float* s_p, float* s_dz1) {
  const unsigned t = threadIdx.x;
  const T* w2 = static_cast<const T*>(p.w2);
  const unsigned crp = (p.Cr + kWave - 1) / kWave * kWave;
  const unsigned ng = crp <= (unsigned)NT ? NT / crp : 1;
  const unsigned seg = (p.C + ng - 1) / ng;
  if (crp <= (unsigned)NT) {
    const unsigned grp = t / crp, j = t - grp * crp;
    if (grp < ng) {
      float acc = 0.f;
      if (j < p.Cr) {
        const unsigned c1 = (grp + 1) * seg < p.C ? (grp + 1) * seg : p.C;
        for (unsigned c = grp * seg; c < c1; ++c) acc += (float)w2[(size_t)c * p.Cr + j] * s_c[c];
      }
      s_p[t] = acc;
    }
  }
  __syncthreads();
  for (unsigned j = t; j < p.Cr; j += NT) {
    float dh = 0.f;
    if (crp <= (unsigned)NT) {
      dh = s_p[j];
      for (unsigned q = 1; q < ng; ++q) dh = dh + s_p[q * crp + j];
    } else {
      for (unsigned c = 0; c < p.C; ++c) dh += (float)w2[(size_t)c * p.Cr + j] * s_c[c];
    }
    const float z = p.z1[(size_t)n * p.Cr + j];
    const float d = (z >= 0.f && z <= 6.f) ? dh : 0.f;
    p.dz1[(size_t)n * p.Cr + j] = d;
    if (s_dz1) s_dz1[j] = d;
  }
  __syncthreads();
}

__device__ __forceinline__ float se_dz2(float s, float av) { return s * (av * (1.0f - av)); }

template <typename T, bool BWD>
__global__ __launch_bounds__(kSeT) void se_reduce_kernel(SeArgs p, int wave_mode) {
  __shared__ float s_c[kSeMaxC];
  __shared__ float s_p[kSeT];
  __shared__ float s_red[kSeT / kWave];
  __shared__ int s_ticket;
  const unsigned t = threadIdx.x, lane = t & (kWave - 1), wave = t / kWave;
  const T* x = static_cast<const T*>(p.x);
  const T* dy = static_cast<const T*>(p.dy);
  unsigned n;
  if (wave_mode) {
    n = blockIdx.x / p.bpi;
    const unsigned c = (blockIdx.x - n * p.bpi) * (kSeT / kWave) + wave;
    if (c < p.C) {   // (a whole wave)
      const size_t e = ((size_t)n * p.C + c) * p.HW;
      const float v = wave_sum_f32(se_run_sum<T, kWave, BWD, false>(x + e, dy + e, p.HW, lane, nullptr));
      if (lane == 0)
        __hip_atomic_store(p.partial + (size_t)n * p.C + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  } else {
    const unsigned plane = blockIdx.x / p.S, s = blockIdx.x - plane * p.S;
    n = plane / p.C;
    const unsigned first = s * p.chunk;
    const unsigned len = p.HW - first < p.chunk ? p.HW - first : p.chunk;
    const size_t e = (size_t)plane * p.HW + first;
    const float v = block_sum_f32<kSeT>(se_run_sum<T, kSeT, BWD, false>(x + e, dy + e, len, t, nullptr), s_red);
    if (t == 0) __hip_atomic_store(p.partial + blockIdx.x, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // The partials leave as device-scope stores and have been performed (vmcnt(0)) before the barrier behind which the
  // ticket is taken, and the last ticket's workgroup reads them back with device-scope loads: no cache write-back or
  // invalidate per workgroup, which a release / acquire fence pair here would cost 2 * N * bpi times.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (t == 0) s_ticket = __hip_atomic_fetch_add(p.ticket + n, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __syncthreads();
  if (s_ticket != (int)p.bpi - 1) return;
  for (unsigned c = t; c < p.C; c += kSeT) {
    const float* q = p.partial + ((size_t)n * p.C + c) * p.S;
    float v = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (unsigned s = 1; s < p.S; ++s) v = v + __hip_atomic_load(q + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (BWD) {
      v = se_dz2(v, p.a[(size_t)n * p.C + c]);
      p.dz2[(size_t)n * p.C + c] = v;
    } else {
      v = v / p.hw;
      p.gap[(size_t)n * p.C + c] = v;
    }
    s_c[c] = v;
  }
  __syncthreads();
  if (BWD) se_gate_bwd<T, kSeT>(p, n, s_c, s_p, nullptr);
  else se_gate_z1<T, kSeT>(p, n, s_c, nullptr);
}

// G == kWave: a wave per plane, four planes per workgroup; G == kSeT: a workgroup per (plane, chunk)
template <typename T, int G, bool BWD>
__global__ __launch_bounds__(kSeT) void se_apply_kernel(SeArgs p) {
  const unsigned t = threadIdx.x % G, lane = threadIdx.x & (kWave - 1);
  const unsigned u = blockIdx.x * (kSeT / G) + threadIdx.x / G;
  const unsigned plane = G == kWave ? u : u / p.acp;
  if (plane >= p.N * p.C) return;   // (a whole wave; G == kWave only)
  const unsigned k = G == kWave ? 0 : u - plane * p.acp;
  const unsigned n = plane / p.C, c = plane - n * p.C;
  float av, gv = 0.f;
  if (BWD) {
    av = p.a[plane];
    gv = se_plane_g<T>(p, c, p.dz1 + (size_t)n * p.Cr, lane);
    if (k == 0 && threadIdx.x % G == 0) p.g[plane] = gv;
  } else {
    av = se_plane_a<T>(p, c, p.z1 + (size_t)n * p.Cr, lane);
    if (k == 0 && threadIdx.x % G == 0) p.a[plane] = av;
  }
  const unsigned first = G == kWave ? 0 : k * kSeApplyChunk;
  const unsigned len = G == kWave ? p.HW : (p.HW - first < kSeApplyChunk ? p.HW - first : kSeApplyChunk);
  const size_t e = (size_t)plane * p.HW + first;
  const T* in = static_cast<const T*>(BWD ? p.dy : p.x) + e;
  se_run_apply<T, G, BWD, false>(in, static_cast<T*>(p.out) + e, len, t, av, gv);
}

// One workgroup per image.  LDS: kSeMaxCr floats (z1 / dz1), kSeResT floats (the backward's segments), C floats
// (gap / dz2), then the image.
template <typename T, bool BWD>
__global__ __launch_bounds__(kSeResT) void se_resident_kernel(SeArgs p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char se_lds[];
  float* s_r = reinterpret_cast<float*>(se_lds);
  float* s_p = s_r + kSeMaxCr;
  float* s_c = s_p + kSeResT;
  T* img = reinterpret_cast<T*>(s_c + (p.C + 3) / 4 * 4);
  const unsigned lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned n = blockIdx.x;
  const T* x = static_cast<const T*>(p.x);
  const T* dy = static_cast<const T*>(p.dy);
  for (unsigned c = wave; c < p.C; c += kSeResT / kWave) {
    const size_t e = ((size_t)n * p.C + c) * p.HW;
    const float v = wave_sum_f32(se_run_sum<T, kWave, BWD, true>(x + e, dy + e, p.HW, lane, img + (size_t)c * p.HW));
    if (lane == 0) {
      if (BWD) {
        const float d = se_dz2(v, p.a[(size_t)n * p.C + c]);
        p.dz2[(size_t)n * p.C + c] = d;
        s_c[c] = d;
      } else {
        const float m = v / p.hw;
        p.gap[(size_t)n * p.C + c] = m;
        s_c[c] = m;
      }
    }
  }
  __syncthreads();
  if (BWD) {
    se_gate_bwd<T, kSeResT>(p, n, s_c, s_p, s_r);
  } else {
    se_gate_z1<T, kSeResT>(p, n, s_c, s_r);
    __syncthreads();
  }
  for (unsigned c = wave; c < p.C; c += kSeResT / kWave) {
    const size_t plane = (size_t)n * p.C + c;
    float av, gv = 0.f;
    if (BWD) {
      av = p.a[plane];
      gv = se_plane_g<T>(p, c, s_r, lane);
      if (lane == 0) p.g[plane] = gv;
    } else {
      av = se_plane_a<T>(p, c, s_r, lane);
      if (lane == 0) p.a[plane] = av;
    }
    se_run_apply<T, kWave, BWD, true>(img + (size_t)c * p.HW, static_cast<T*>(p.out) + plane * p.HW, p.HW, lane, av,
                                      gv);
  }
}

// a thread per element of dw2 (C, Cr), dw1 (Cr, C), db2 (C), db1 (Cr); the images are added in order
__global__ __launch_bounds__(kSeT) void se_wgrad_kernel(SeArgs p, float* dw1, float* db1, float* dw2, float* db2) {
  const unsigned cc = p.C * p.Cr;
  const unsigned i = blockIdx.x * kSeT + threadIdx.x;
  if (i < cc) {                       // dw2[c][j] = sum_n dz2[n,c] * h[n,j]
    const unsigned c = i / p.Cr, j = i - c * p.Cr;
    float acc = 0.f;
    for (unsigned n = 0; n < p.N; ++n) acc += p.dz2[(size_t)n * p.C + c] * se_clip(p.z1[(size_t)n * p.Cr + j]);
    dw2[i] = acc;
  } else if (i < 2 * cc) {            // dw1[j][c] = sum_n dz1[n,j] * gap[n,c]
    const unsigned q = i - cc, j = q / p.C, c = q - j * p.C;
    float acc = 0.f;
    for (unsigned n = 0; n < p.N; ++n) acc += p.dz1[(size_t)n * p.Cr + j] * p.gap[(size_t)n * p.C + c];
    dw1[q] = acc;
  } else if (i < 2 * cc + p.C) {
    const unsigned c = i - 2 * cc;
    if (db2) {
      float acc = 0.f;
      for (unsigned n = 0; n < p.N; ++n) acc += p.dz2[(size_t)n * p.C + c];
      db2[c] = acc;
    }
  } else if (i < 2 * cc + p.C + p.Cr) {
    const unsigned j = i - 2 * cc - p.C;
    if (db1) {
      float acc = 0.f;
      for (unsigned n = 0; n < p.N; ++n) acc += p.dz1[(size_t)n * p.Cr + j];
      db1[j] = acc;
    }
  }
}

// ---------------------------------------------------------------------------------------------- host --
struct SePlan {
  bool wave;           // the two-pass reduction: a wave per plane
  unsigned S, chunk, bpi, acp;
  size_t lds32, lds16; // dynamic LDS of the resident kernels per element size
  size_t ticket_bytes, partial_bytes, dz2_bytes, dz1_bytes;
};

static size_t se_lds_bytes(int C, long HxW, size_t esz) {
  return ((size_t)kSeResHead + (size_t)(C + 3) / 4 * 4) * sizeof(float) + ((size_t)C * HxW * esz + 15) / 16 * 16;
}

static int se_plan(int N, int C, int Cr, long HxW, int path, int split, SePlan* p) {
  SD_REQUIRE(N >= 1 && C >= 1 && Cr >= 1 && HxW >= 1, "se_block: N=%d C=%d Cr=%d HxW=%ld must all be at least 1", N, C,
             Cr, HxW);
  SD_REQUIRE(path >= 0 && path <= 2, "se_block: path=%d is not 0 (automatic), 1 (two-pass) or 2 (resident)", path);
  SD_REQUIRE(split >= 0 && split <= kSeMaxSplit, "se_block: split=%d is outside 0..%d", split, kSeMaxSplit);
  if (C > kSeMaxC || Cr > kSeMaxCr)
    return fail(SD_ERR_UNSUPPORTED, "se_block: C=%d Cr=%d exceed the limits %d and %d", C, Cr, kSeMaxC, kSeMaxCr);
  if (HxW > kSeMaxElems / ((long)N * C))
    return fail(SD_ERR_UNSUPPORTED, "se_block: N*C*HxW = %ld x %ld elements exceed the limit %ld", (long)N * C, HxW,
                kSeMaxElems);
  p->wave = split == 0 && HxW <= (long)kSeWavePlane;
  if (p->wave) {
    p->S = 1;
    p->chunk = (unsigned)HxW;
    p->bpi = (unsigned)cdiv(C, kSeT / kWave);
  } else {
    long S = split;
    if (S == 0) {   // enough workgroups to fill the device, chunks no smaller than kSeReduceChunk
      const long want = cdiv(8 * kNumCU, (long)N * C), most = cdiv(HxW, kSeReduceChunk);
      S = want < most ? want : most;
      if (S > kSeMaxSplit) S = kSeMaxSplit;
    }
    if (S > HxW) S = HxW;
    long chunk = (HxW + S - 1) / S;
    if (split == 0) chunk = (chunk + 63) / 64 * 64;
    p->chunk = (unsigned)chunk;
    p->S = (unsigned)((HxW + chunk - 1) / chunk);
    p->bpi = (unsigned)C * p->S;
  }
  p->acp = (unsigned)cdiv(HxW, kSeApplyChunk);
  p->lds32 = se_lds_bytes(C, HxW, 4);
  p->lds16 = se_lds_bytes(C, HxW, 2);
  p->ticket_bytes = (size_t)N * sizeof(int);
  p->partial_bytes = (size_t)N * C * p->S * sizeof(float);
  p->dz2_bytes = (size_t)N * C * sizeof(float);
  p->dz1_bytes = (size_t)N * Cr * sizeof(float);
  return SD_OK;
}

static size_t se_carve(const SePlan& p, void* workspace, SeArgs* a) {
  WsCarver w(workspace);
  int* ticket = w.take<int>(p.ticket_bytes);
  float* partial = w.take<float>(p.partial_bytes);
  float* dz2 = w.take<float>(p.dz2_bytes);
  float* dz1 = w.take<float>(p.dz1_bytes);
  if (a) { a->ticket = ticket; a->partial = partial; a->dz2 = dz2; a->dz1 = dz1; }
  return w.need();
}
static size_t se_need(const SePlan& p) { return 256 + se_carve(p, nullptr, nullptr); }

// checks shared by both directions; *resident says which path runs
template <typename T>
static int se_begin(int N, int C, int Cr, long HxW, int path, int split, const void* workspace, size_t workspace_bytes,
                    SePlan* p, bool* resident) {
  if (int e = se_plan(N, C, Cr, HxW, path, split, p)) return e;
  const size_t lds = sizeof(T) == 4 ? p->lds32 : p->lds16;
  if (path == 2 && lds > kSeLds)
    return fail(SD_ERR_UNSUPPORTED, "se_block: path 2 (resident) needs %zu B of LDS for an image of %d x %ld %s (limit %zu)",
                lds, C, HxW, elem_type_name<T>(), kSeLds);
  *resident = path == 2 || (path == 0 && lds <= kSeLds);
  return workspace_check(workspace, workspace_bytes, se_need(*p), "se_block");
}

static void se_fill(SeArgs& a, const SePlan& p, int N, int C, int Cr, long HxW) {
  a.N = (unsigned)N; a.C = (unsigned)C; a.Cr = (unsigned)Cr; a.HW = (unsigned)HxW;
  a.S = p.S; a.chunk = p.chunk; a.bpi = p.bpi; a.acp = p.acp;
  a.hw = (float)HxW;
}

template <typename T, bool BWD>
static int se_launch(SeArgs& a, const SePlan& p, bool resident, hipStream_t st) {
  const char* dir = BWD ? "bwd" : "fwd";
  if (resident) {
    const size_t lds = sizeof(T) == 4 ? p.lds32 : p.lds16;
    static bool raised = false;   // (per instance; the call is idempotent, so a race costs a second one)
    if (lds > 64 * 1024 && !raised) {
      SD_HIP_CHECK(hipFuncSetAttribute((const void*)se_resident_kernel<T, BWD>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSeLds));
      raised = true;
    }
    hipLaunchKernelGGL((se_resident_kernel<T, BWD>), dim3(a.N), dim3(kSeResT), lds, st, a);
    note_dispatch("sd::se_resident_kernel<%s,%s> x %u images, %zu B LDS%s", elem_type_name<T>(), dir, a.N, lds,
                  BWD ? " + sd::se_wgrad_kernel" : "");
    return SD_OK;
  }
  zero_counters(a.ticket, (long)a.N, st);
  hipLaunchKernelGGL((se_reduce_kernel<T, BWD>), dim3(a.N * p.bpi), dim3(kSeT), 0, st, a, p.wave ? 1 : 0);
  if (p.wave) {
    hipLaunchKernelGGL((se_apply_kernel<T, kWave, BWD>), dim3(cdiv((long)a.N * a.C, kSeT / kWave)), dim3(kSeT), 0, st,
                       a);
    note_dispatch("sd::se_reduce_kernel<%s,%s,wave> + sd::se_apply_kernel<%s,%s,wave>%s", elem_type_name<T>(), dir, elem_type_name<T>(),
                  dir, BWD ? " + sd::se_wgrad_kernel" : "");
  } else {
    hipLaunchKernelGGL((se_apply_kernel<T, kSeT, BWD>), dim3(a.N * a.C * p.acp), dim3(kSeT), 0, st, a);
    note_dispatch("sd::se_reduce_kernel<%s,%s,block> x %u chunks of %u + sd::se_apply_kernel<%s,%s,block>%s",
                  elem_type_name<T>(), dir, p.S, p.chunk, elem_type_name<T>(), dir, BWD ? " + sd::se_wgrad_kernel" : "");
  }
  return SD_OK;
}

template <typename T>
static int se_fwd(const void* x, const void* w1, const void* b1, const void* w2, const void* b2, void* y, float* gap,
                  float* z1, float* av, int N, int C, int Cr, long HxW, int path, int split, void* workspace,
                  size_t workspace_bytes, void* stream) {
  SePlan p{};
  bool resident = false;
  SD_REQUIRE(x && w1 && w2 && y && gap && z1 && av, "se_block_fwd: null pointer");
  SD_REQUIRE(ptrs_aligned(sizeof(T), {x, w1, b1, w2, b2, y}) && ptrs_aligned(4, {gap, z1, av}),
             "se_block_fwd: a pointer is not aligned to its elements");
  if (int e = se_begin<T>(N, C, Cr, HxW, path, split, workspace, workspace_bytes, &p, &resident)) return e;
  SeArgs a{};
  se_fill(a, p, N, C, Cr, HxW);
  se_carve(p, workspace, &a);
  a.x = x; a.out = y; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.gap = gap; a.z1 = z1; a.a = av;
  if (int e = se_launch<T, false>(a, p, resident, (hipStream_t)stream)) return e;
  SD_LAUNCH_CHECK();
  return SD_OK;
}

template <typename T>
static int se_bwd(const void* dy, const void* x, const float* gap, const float* z1, const float* av, const void* w1,
                  const void* w2, void* dx, float* g, float* dw1, float* db1, float* dw2, float* db2, int N, int C,
                  int Cr, long HxW, int path, int split, void* workspace, size_t workspace_bytes, void* stream) {
  SePlan p{};
  bool resident = false;
  SD_REQUIRE(dy && x && gap && z1 && av && w1 && w2 && dx && g && dw1 && dw2, "se_block_bwd: null pointer");
  SD_REQUIRE(ptrs_aligned(sizeof(T), {dy, x, w1, w2, dx}) && ptrs_aligned(4, {gap, z1, av, g, dw1, db1, dw2, db2}),
             "se_block_bwd: a pointer is not aligned to its elements");
  if (int e = se_begin<T>(N, C, Cr, HxW, path, split, workspace, workspace_bytes, &p, &resident)) return e;
  SeArgs a{};
  se_fill(a, p, N, C, Cr, HxW);
  se_carve(p, workspace, &a);
  a.x = x; a.dy = dy; a.out = dx; a.w1 = w1; a.w2 = w2;
  a.gap = const_cast<float*>(gap); a.z1 = const_cast<float*>(z1); a.a = const_cast<float*>(av); a.g = g;
  hipStream_t st = (hipStream_t)stream;
  if (int e = se_launch<T, true>(a, p, resident, st)) return e;
  const long outs = 2L * C * Cr + C + Cr;
  hipLaunchKernelGGL(se_wgrad_kernel, dim3(cdiv(outs, kSeT)), dim3(kSeT), 0, st, a, dw1, db1, dw2, db2);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_se_block_workspace_bytes(int N, int C, int Cr, long HxW, int path, int split) {
  SePlan p{};
  if (se_plan(N, C, Cr, HxW, path, split, &p) != SD_OK) return 256;
  return se_need(p);
}

extern "C" int sd_se_block_fwd(const float* x, const float* w1, const float* b1, const float* w2, const float* b2,
                               float* y, float* gap, float* z1, float* a, int N, int C, int Cr, long HxW, int path,
                               int split, void* workspace, size_t workspace_bytes, void* stream) {
  return se_fwd<float>(x, w1, b1, w2, b2, y, gap, z1, a, N, C, Cr, HxW, path, split, workspace, workspace_bytes, stream);
}
extern "C" int sd_se_block_fwd_f16(const void* x, const void* w1, const void* b1, const void* w2, const void* b2,
                                   void* y, float* gap, float* z1, float* a, int N, int C, int Cr, long HxW, int path,
                                   int split, void* workspace, size_t workspace_bytes, void* stream) {
  return se_fwd<_Float16>(x, w1, b1, w2, b2, y, gap, z1, a, N, C, Cr, HxW, path, split, workspace, workspace_bytes,
                          stream);
}
extern "C" int sd_se_block_bwd(const float* dy, const float* x, const float* gap, const float* z1, const float* a,
                               const float* w1, const float* w2, float* dx, float* g, float* dw1, float* db1,
                               float* dw2, float* db2, int N, int C, int Cr, long HxW, int path, int split,
                               void* workspace, size_t workspace_bytes, void* stream) {
  return se_bwd<float>(dy, x, gap, z1, a, w1, w2, dx, g, dw1, db1, dw2, db2, N, C, Cr, HxW, path, split, workspace,
                       workspace_bytes, stream);
}
extern "C" int sd_se_block_bwd_f16(const void* dy, const void* x, const float* gap, const float* z1, const float* a,
                                   const void* w1, const void* w2, void* dx, float* g, float* dw1, float* db1,
                                   float* dw2, float* db2, int N, int C, int Cr, long HxW, int path, int split,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  return se_bwd<_Float16>(dy, x, gap, z1, a, w1, w2, dx, g, dw1, db1, dw2, db2, N, C, Cr, HxW, path, split, workspace,
                          workspace_bytes, stream);
}
