// _contrib_Quantization_int8 for gfx950: fused abs-max, EMA / step state and fake-quantise, fp32.
//   reference (the spec): operator_cxx/contrib/quantization_int8-inl.h:113-226 (Forward: a min reduce, a max
//   reduce, a one-thread kernel, a blocking copy of the threshold to the host, a third pass over the data) and
//   :229-294 (Backward: "ste" copies, "clip" builds two full-size temporaries and a where()).
// MI355X design (every launch on the caller's stream, nothing read back by the host, graph-capturable):
//   The tensor -- or, in the multi-tensor call, every tensor -- is cut into units of `unit` elements, one
//   workgroup each; find_seg() maps a workgroup to (tensor, span) from the element counts alone, so both
//   passes rebuild the same table on the device and the host never sees a count.
//   1. quant_absmax_kernel  every workgroup first reads countdown from `state` (thread 0, broadcast through LDS
//        behind a barrier) and derives the mode: copy
//        (is_train && countdown > 0) or quantise.  Only a training call that quantises without fix_act_scale
//        reads its span (16-byte loads, scalar head and tail) and reduces |x| as the unsigned maximum of the
//        floats' bit patterns.  Thread 0 then folds the workgroup's maximum into the tensor's word with an
//        agent-scope atomic max, waits for it, and takes a ticket with an agent-scope atomic add.  The
//        workgroup whose ticket is the last reads the word back with another atomic (read-modify-write on both
//        sides: no cache holds a copy), applies the state transition and writes minmax, state and the record
//        {mode, t, u = t / 127} pass 2 reads behind the kernel boundary.  `state` changes only there, after
//        every workgroup of that tensor has arrived, hence after every one of them has read it.
//        A tensor of one unit has no ticket; calls the host knows to need no reduction (eval, fix_act_scale)
//        run one workgroup per tensor.  The (max, ticket) words are cleared by quant_clear_kernel in front of
//        the launch whenever a tensor can have more than one unit (a kernel, not hipMemsetAsync: a memset node
//        is not repeated on replays of a captured graph).
//   2. quant_apply_kernel   streams data to out: a copy in copy mode, else roundf(c / u) * u with c = x for
//        weights and x clipped to [-t, t] for activations (NaN passes through).  Divide and product are two
//        IEEE roundings (-ffp-contract=off, correctly rounded divide).
//   Backward: quant_bwd_kernel, one launch: dgrad (+)= ograd, under "clip" only where -t <= x <= t, t read
//   from minmax on the device.
//   Stores go in 16-byte items from the first 16-byte boundary of the OUTPUT span; an input whose phase
//   differs is loaded by 4-byte accesses, so pointers need 4-byte alignment only and the bits do not depend on it.
#include "common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {
namespace {

constexpr int kRedT = 512;                  // pass 1 workgroup
constexpr int kRedTrip = kRedT * 4 * 4;     // elements of one trip: four 16-byte loads in flight per lane
constexpr int kRedUnits = 512;              // units (= tickets on one word) per call, two workgroups per CU
constexpr int kMapT = 256;                  // pass 2 / backward workgroup
constexpr int kMapTrip = kMapT * 4 * 4;
constexpr int kMapUnits = 2048;
constexpr int kMaxT = 1024;                 // tensors of one multi-tensor call
constexpr int kCtrStride = 16;              // words between two tensors' (max, ticket) pairs: 64 bytes
constexpr long kMaxN = 1L << 40;

struct QRec {
  int quantise;  // 0: copy mode
  float t, u;
  int pad;
};

struct QArgs {
  // one tensor ...
  const float* data;
  float* out;
  float* minmax;
  int* state;
  long n;
  // ... or T of them through device arrays (datas != nullptr)
  const float* const* datas;
  float* const* outs;
  float* const* minmaxes;
  int* const* states;
  const long* counts;
  int T;
  long unit;
  int is_weight, is_train, fix_scale;
  float decay;
  unsigned* ctr;  // (T, kCtrStride): [0] max of the bit patterns, [1] arrivals
  QRec* rec;      // (T)
};

struct Seg {
  int t, units;
  long len;  // 0: this workgroup has no span
  const float* data;
  float* out;
  float* minmax;
  int* state;
};

// workgroup -> (tensor, span).  s_pref holds kMaxT + 1 ints.
__device__ __forceinline__ Seg find_seg(const QArgs& a, int* s_pref) {
  Seg s{};
  const long b = blockIdx.x;
  if (!a.datas) {
    const long units = (a.n + a.unit - 1) / a.unit;
    if (b >= units) return s;
    const long begin = b * a.unit;
    s.t = 0;
    s.units = (int)units;
    s.len = a.n - begin < a.unit ? a.n - begin : a.unit;
    s.data = a.data + begin;
    s.out = a.out + begin;
    s.minmax = a.minmax;
    s.state = a.state;
    return s;
  }
  for (int i = threadIdx.x; i < a.T; i += blockDim.x) {
    const long c = a.counts[i];
    s_pref[i + 1] = c > 0 ? (int)((c + a.unit - 1) / a.unit) : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    s_pref[0] = 0;
    for (int i = 1; i <= a.T; ++i) {
      run += s_pref[i];
      s_pref[i] = run;
    }
  }
  __syncthreads();
  if (b >= s_pref[a.T]) return s;
  int lo = 0, hi = a.T - 1;  // the tensor t with pref[t] <= b < pref[t + 1]
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (s_pref[mid + 1] <= (int)b) lo = mid + 1; else hi = mid;
  }
  const long begin = (b - s_pref[lo]) * a.unit;
  const long cnt = a.counts[lo];
  s.t = lo;
  s.units = s_pref[lo + 1] - s_pref[lo];
  s.len = cnt - begin < a.unit ? cnt - begin : a.unit;
  s.data = a.datas[lo] + begin;
  s.out = a.outs[lo] + begin;
  s.minmax = a.minmaxes[lo];
  s.state = a.states[lo];
  return s;
}

// floats in front of the first 16-byte boundary of p (p is 4-byte aligned), at most len
__device__ __forceinline__ long head_len(const void* p, long len) {
  const long h = (long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  return h < len ? h : len;
}

// max of the bit patterns of |p[0 .. len)| over the workgroup; valid in thread 0.  Every thread calls it.
__device__ __forceinline__ unsigned block_absmax(const float* p, long len, unsigned* s_red) {
  const int tid = threadIdx.x;
  const long head = head_len(p, len);
  unsigned m = 0;
  if (tid < head) m = absbits(p[tid]);
  const float4* v = reinterpret_cast<const float4*>(p + head);
  const long nv = (len - head) >> 2;
  long i = tid;
  for (; i + 3 * kRedT < nv; i += 4 * kRedT) {
    const float4 x0 = v[i], x1 = v[i + kRedT], x2 = v[i + 2 * kRedT], x3 = v[i + 3 * kRedT];
    m = umaxr(m, umaxr(umaxr(absbits4(x0), absbits4(x1)), umaxr(absbits4(x2), absbits4(x3))));
  }
  for (; i < nv; i += kRedT) m = umaxr(m, absbits4(v[i]));
  const long done = head + nv * 4;
  if (tid < len - done) m = umaxr(m, absbits(p[done + tid]));
  m = wave_max_u32(m);
  if ((tid & (kWave - 1)) == 0) s_red[tid / kWave] = m;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < kRedT / kWave; ++w) m = umaxr(m, s_red[w]);
  return m;
}

// the (max, ticket) pair of every tensor; pass 1 reaches them by atomics behind the kernel boundary
__global__ __launch_bounds__(kMapT) void quant_clear_kernel(unsigned* ctr, int T) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < T) {
    ctr[(long)i * kCtrStride] = 0u;
    ctr[(long)i * kCtrStride + 1] = 0u;
  }
}

__global__ __launch_bounds__(kRedT) void quant_absmax_kernel(QArgs a) {
  __shared__ int s_pref[kMaxT + 1];
  __shared__ unsigned s_red[kRedT / kWave];
  const Seg s = find_seg(a, s_pref);
  if (s.len <= 0) return;
  // thread 0 reads before this workgroup arrives (only the last arriver rewrites state, after every arrival) and
  // hands the value to the other waves through LDS: one decision per workgroup, whatever thread 0 stores later
  __shared__ int s_countdown;
  if (threadIdx.x == 0) s_countdown = s.state[0];
  __syncthreads();
  const int countdown = s_countdown;
  const bool copy = a.is_train && countdown > 0;
  const bool reduce = !copy && a.is_train && !a.fix_scale;
  unsigned m = 0;
  if (reduce) m = block_absmax(s.data, s.len, s_red);
  if (threadIdx.x != 0) return;
  if (s.units > 1) {
    unsigned* word = a.ctr + (long)s.t * kCtrStride;
    // the word only grows inside a call, so a stale (lower) value read here costs one atomic, never a maximum
    if (reduce && m > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      __hip_atomic_fetch_max(word, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the max has been performed before the ticket is taken
    const unsigned ticket = __hip_atomic_fetch_add(word + 1, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (ticket != (unsigned)(s.units - 1)) return;
    m = __hip_atomic_fetch_max(word, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  // the state transition of quantization_int8-inl.h:144-220, once per tensor
  float mm = s.minmax[0];
  QRec r{};
  if (copy) {
    s.state[0] = countdown - 1;
  } else {
    if (reduce) {
      const float mx = __uint_as_float(m);
      if (a.is_weight) {
        mm = mx;
      } else if (s.state[1] != 0) {
        if ((double)mm < 1e-6) mm = mx;  // :196: a float against a double literal
        s.state[1] = 0;
      } else {
        const float keep = a.decay * mm;  // two rounded products and a rounded sum (-ffp-contract=off)
        const float take = (1.0f - a.decay) * mx;
        mm = keep + take;
      }
      s.minmax[0] = mm;
    }
    r.quantise = 1;
    r.u = mm / 127.0f;
  }
  r.t = mm;
  a.rec[s.t] = r;
}

__device__ __forceinline__ float4 ld4(const float* p, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

// q[i] = f(x[i], y[i], q[i]) over one span; y is read when kY, q when kOld.  Stores are 16-byte items from q's
// first 16-byte boundary; x and y follow with 16-byte loads where their phase agrees.
template <bool kY, bool kOld, class F>
__device__ __forceinline__ void map_span(const float* x, const float* y, float* q, long len, F f) {
  const int tid = threadIdx.x;
  const long head = head_len(q, len);
  if (tid < head) q[tid] = f(x[tid], kY ? y[tid] : 0.0f, kOld ? q[tid] : 0.0f);
  const long nv = (len - head) >> 2;
  const float* xb = x + head;
  const float* yb = kY ? y + head : nullptr;
  float4* qv = reinterpret_cast<float4*>(q + head);
  const bool xvec = ((uintptr_t)xb & 15u) == 0, yvec = kY && ((uintptr_t)yb & 15u) == 0;
  auto f4 = [&](const float4& xs, const float4& ys, const float4& os) {
    return make_float4(f(xs.x, ys.x, os.x), f(xs.y, ys.y, os.y), f(xs.z, ys.z, os.z), f(xs.w, ys.w, os.w));
  };
  const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  long i = tid;
  for (; i + 3 * kMapT < nv; i += 4 * kMapT) {
    float4 xs[4], ys[4], os[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long j = i + k * kMapT;
      xs[k] = ld4(xb + 4 * j, xvec);
      ys[k] = kY ? ld4(yb + 4 * j, yvec) : zero;
      os[k] = kOld ? qv[j] : zero;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) qv[i + k * kMapT] = f4(xs[k], ys[k], os[k]);
  }
  for (; i < nv; i += kMapT)
    qv[i] = f4(ld4(xb + 4 * i, xvec), kY ? ld4(yb + 4 * i, yvec) : zero, kOld ? qv[i] : zero);
  const long done = head + nv * 4;
  if (tid < len - done) {
    const long j = done + tid;
    q[j] = f(x[j], kY ? y[j] : 0.0f, kOld ? q[j] : 0.0f);
  }
}

__global__ __launch_bounds__(kMapT) void quant_apply_kernel(QArgs a) {
  __shared__ int s_pref[kMaxT + 1];
  const Seg s = find_seg(a, s_pref);
  if (s.len <= 0) return;
  const QRec r = a.rec[s.t];
  const float t = r.t, u = r.u;
  if (!r.quantise)
    map_span<false, false>(s.data, nullptr, s.out, s.len, [](float x, float, float) { return x; });
  else if (a.is_weight)  // :187-191: weights are not clipped
    map_span<false, false>(s.data, nullptr, s.out, s.len, [u](float x, float, float) { return roundf(x / u) * u; });
  else
    map_span<false, false>(s.data, nullptr, s.out, s.len, [t, u](float x, float, float) {
      const float c = x > t ? t : (x < -t ? -t : x);  // mshadow_op::clip: a NaN passes through
      return roundf(c / u) * u;
    });
}

struct QBwdArgs {
  const float* ograd;
  const float* data;
  const float* minmax;
  float* dgrad;
  long n, unit;
  int clip, add;
};

__global__ __launch_bounds__(kMapT) void quant_bwd_kernel(QBwdArgs a) {
  const long begin = (long)blockIdx.x * a.unit;
  if (begin >= a.n) return;
  const long len = a.n - begin < a.unit ? a.n - begin : a.unit;
  const float* g = a.ograd + begin;
  float* q = a.dgrad + begin;
  if (!a.clip) {
    if (a.add) map_span<false, true>(g, nullptr, q, len, [](float og, float, float old) { return old + og; });
    else map_span<false, false>(g, nullptr, q, len, [](float og, float, float) { return og; });
    return;
  }
  const float t = a.minmax[0];
  const float* x = a.data + begin;
  // :283-287: ge(x, -t) * le(x, t) selects ograd, else +0.0; a NaN x fails both tests
  if (a.add)
    map_span<true, true>(g, x, q, len,
                         [t](float og, float xv, float old) { return old + ((xv >= -t && xv <= t) ? og : 0.0f); });
  else
    map_span<true, false>(g, x, q, len, [t](float og, float xv, float) { return (xv >= -t && xv <= t) ? og : 0.0f; });
}

long unit_for(long n, int trip, int max_units) {
  const long trips = (n + trip - 1) / trip;
  const long per = (trips + max_units - 1) / max_units;
  return (long)trip * (per > 1 ? per : 1);
}

struct QWs {
  unsigned* ctr;
  QRec* rec;
};
size_t quant_layout(int T, QWs* ws, char* base) {
  const size_t ctr_bytes = ((size_t)T * kCtrStride * sizeof(unsigned) + 255) / 256 * 256;
  const size_t rec_bytes = ((size_t)T * sizeof(QRec) + 255) / 256 * 256;
  if (ws) {
    ws->ctr = reinterpret_cast<unsigned*>(base);
    ws->rec = reinterpret_cast<QRec*>(base + ctr_bytes);
  }
  return ctr_bytes + rec_bytes;
}

bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

// the clearing kernel (only where a tensor can have several units), pass 1, pass 2
int launch_fwd(QArgs a, long n_total, void* workspace, size_t workspace_bytes, const char* who, hipStream_t st) {
  QWs ws;
  char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) / 256 * 256);
  const size_t need = quant_layout(a.T, &ws, base) + (size_t)(base - (char*)workspace);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "%s workspace too small: %zu < %zu bytes", who, workspace_bytes, need);
  a.ctr = ws.ctr;
  a.rec = ws.rec;
  const bool reduce = a.is_train && !a.fix_scale;
  // without a reduction one workgroup per tensor settles the state: no tickets, nothing to clear
  a.unit = reduce ? unit_for(n_total, kRedTrip, kRedUnits) : (n_total + kRedTrip - 1) / kRedTrip * kRedTrip;
  const long extra = a.datas ? a.T : 0;  // sum of ceil(n_t / unit) <= n_total / unit + T
  const long g1 = a.datas ? n_total / a.unit + extra : (n_total + a.unit - 1) / a.unit;
  if (reduce && n_total > a.unit) {
    hipLaunchKernelGGL(quant_clear_kernel, dim3((unsigned)((a.T + kMapT - 1) / kMapT)), dim3(kMapT), 0, st, ws.ctr,
                       a.T);
    SD_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(quant_absmax_kernel, dim3((unsigned)g1), dim3(kRedT), 0, st, a);
  SD_LAUNCH_CHECK();
  a.unit = unit_for(n_total, kMapTrip, kMapUnits);
  const long g2 = a.datas ? n_total / a.unit + extra : (n_total + a.unit - 1) / a.unit;
  hipLaunchKernelGGL(quant_apply_kernel, dim3((unsigned)g2), dim3(kMapT), 0, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_quant_int8_workspace_bytes(long n) {
  (void)n;  // one (max, ticket) pair and one record, whatever the size
  return quant_layout(1, nullptr, nullptr) + 256;
}

extern "C" size_t sd_quant_int8_weights_workspace_bytes(int T, long n_total) {
  (void)n_total;
  if (T <= 0 || T > kMaxT) return 256;
  return quant_layout(T, nullptr, nullptr) + 256;
}

extern "C" int sd_quant_int8_fwd(const float* data, float* out, float* minmax, int* state, long n, int is_weight,
                                 int is_train, int fix_act_scale, double ema_decay, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  SD_REQUIRE(n >= 0, "Quantization_int8: negative element count %ld", n);
  SD_REQUIRE(ema_decay >= 0.0 && ema_decay <= 1.0, "Quantization_int8: ema_decay %g is outside [0, 1]", ema_decay);
  SD_REQUIRE(data && out && minmax && state, "Quantization_int8: null data / out / minmax / state pointer");
  SD_REQUIRE(aligned4(data) && aligned4(out) && aligned4(minmax) && aligned4(state),
             "Quantization_int8: pointers must be 4-byte aligned");
  if (n > kMaxN) return fail(SD_ERR_UNSUPPORTED, "Quantization_int8: %ld elements exceed the limit of %ld", n, kMaxN);
  if (n == 0) return SD_OK;
  QArgs a{};
  a.data = data; a.out = out; a.minmax = minmax; a.state = state; a.n = n;
  a.T = 1;
  a.is_weight = is_weight ? 1 : 0; a.is_train = is_train ? 1 : 0; a.fix_scale = fix_act_scale ? 1 : 0;
  a.decay = (float)ema_decay;
  return launch_fwd(a, n, workspace, workspace_bytes, "Quantization_int8", (hipStream_t)stream);
}

extern "C" int sd_quant_int8_weights_fwd(const float* const* data_ptrs, float* const* out_ptrs,
                                         float* const* minmax_ptrs, int* const* state_ptrs, const long* counts,
                                         int T, long n_total, int is_train, int fix_act_scale, void* workspace,
                                         size_t workspace_bytes, void* stream) {
  SD_REQUIRE(T >= 0 && n_total >= 0, "Quantization_int8 weights: negative tensor or element count");
  SD_REQUIRE(data_ptrs && out_ptrs && minmax_ptrs && state_ptrs && counts,
             "Quantization_int8 weights: null pointer table");
  if (T > kMaxT)
    return fail(SD_ERR_UNSUPPORTED, "Quantization_int8 weights: %d tensors exceed the limit of %d", T, kMaxT);
  if (n_total > kMaxN)
    return fail(SD_ERR_UNSUPPORTED, "Quantization_int8 weights: %ld elements exceed the limit of %ld", n_total, kMaxN);
  if (T == 0 || n_total == 0) return SD_OK;
  QArgs a{};
  a.datas = data_ptrs; a.outs = out_ptrs; a.minmaxes = minmax_ptrs; a.states = state_ptrs; a.counts = counts;
  a.T = T;
  a.is_weight = 1; a.is_train = is_train ? 1 : 0; a.fix_scale = fix_act_scale ? 1 : 0;
  return launch_fwd(a, n_total, workspace, workspace_bytes, "Quantization_int8 weights", (hipStream_t)stream);
}

extern "C" int sd_quant_int8_bwd(const float* ograd, const float* data, const float* minmax, float* dgrad, long n,
                                 int grad_clip, int req, void* stream) {
  SD_REQUIRE(n >= 0, "Quantization_int8 backward: negative element count %ld", n);
  SD_REQUIRE(req == SD_REQ_NULL || req == SD_REQ_WRITE || req == SD_REQ_ADD,
             "Quantization_int8 backward: unknown req %d", req);
  SD_REQUIRE(ograd && dgrad, "Quantization_int8 backward: null ograd / dgrad pointer");
  SD_REQUIRE(!grad_clip || (data && minmax), "Quantization_int8 backward: the clip mode needs data and minmax");
  SD_REQUIRE(aligned4(ograd) && aligned4(dgrad) && aligned4(data) && aligned4(minmax),
             "Quantization_int8 backward: pointers must be 4-byte aligned");
  if (n > kMaxN)
    return fail(SD_ERR_UNSUPPORTED, "Quantization_int8 backward: %ld elements exceed the limit of %ld", n, kMaxN);
  if (n == 0 || req == SD_REQ_NULL) return SD_OK;
  QBwdArgs a{};
  a.ograd = ograd; a.data = data; a.minmax = minmax; a.dgrad = dgrad; a.n = n;
  a.clip = grad_clip ? 1 : 0;
  a.add = req == SD_REQ_ADD;
  a.unit = unit_for(n, kMapTrip, kMapUnits);
  hipLaunchKernelGGL(quant_bwd_kernel, dim3((unsigned)((n + a.unit - 1) / a.unit)), dim3(kMapT), 0,
                     (hipStream_t)stream, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
