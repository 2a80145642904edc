// Shared host/device helpers for the simpledet_amd HIP library (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>

// error codes returned through the C ABI (include/simpledet_ops.h)
#define SD_OK 0
#define SD_ERR_INVALID_ARG (-1)
#define SD_ERR_UNSUPPORTED (-2)
#define SD_ERR_HIP (-3)
#define SD_ERR_WORKSPACE (-4)

namespace sd {

// thread-local last-error message, read through sd_last_error()
char* err_buf();
int fail(int code, const char* fmt, ...);
// names of the kernels an entry point launches (sd_last_dispatch(): bench.py labels its roofline with them)
void note_dispatch(const char* fmt, ...);

#define SD_REQUIRE(cond, ...)                                    \
  do {                                                           \
    if (!(cond)) return ::sd::fail(SD_ERR_INVALID_ARG, __VA_ARGS__); \
  } while (0)

#define SD_HIP_CHECK(expr)                                                              \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess)                                                               \
      return ::sd::fail(SD_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                        __FILE__, __LINE__);                                            \
  } while (0)

#define SD_LAUNCH_CHECK() SD_HIP_CHECK(hipGetLastError())

// Kernel-VARIANT knobs (A/B of correct implementations from bench.py / the tests), THE list: one row per knob,
// X(identifier = key, default, lowest, highest, what it selects).  The default is the shipped path and the value a knob
// holds until sd_set_tuning changes it (to any integer); a read clamps the value to [lowest, highest].  Every product key
// selects a kernel that some shape or entry point reaches without it (workspace-free calls, C % 4 != 0, ...): tests force it.
constexpr int kBandXcdDefault = 1, kBandStaffDefault = 0;   // (the band forward's plan, roi_align_common.h)
#define SD_PRODUCT_KNOBS(X)                                                                                             \
  X(roi_align_fwd, 1, INT_MIN, INT_MAX, "1: band-resident kernel / tiled kernels where it does not apply; 0: naive per-element kernel") \
  X(roi_align_fwd_band, 1, INT_MIN, INT_MAX, "1: band-resident forward, planes streamed through LDS, no gathers; 0: the tiled fallback kernels") \
  X(roi_align_fwd_quad, 1, INT_MIN, INT_MAX, "1: single-level float arg-max forward with four channel-last planes per workgroup when they fit (the C4 family); 0: the band kernel") \
  X(roi_align_plan_tail, 1, INT_MIN, INT_MAX, "1: the band forward's pre-pass builds only what that kernel reads; the coordinate table and the backward's plan are tasks in the band kernel's tail; 0: all of it in the (merged) pre-pass launch") \
  X(roi_align_fwd_xcd, kBandXcdDefault, 0, 2, "band forward, which share of the cost prefix a block starts on: 0 linear in blockIdx; 1 XCD-contiguous (a unit's workgroups write through one L2); 2 the same, unit table interleaving the levels") \
  X(roi_align_fwd_staff, kBandStaffDefault, 0, 1, "band forward, which virtual unit a workgroup starts on: 0 where the midpoint of its share of the cost prefix falls; 1 whole workgroups per unit, chosen so that the units end together after whole reservations (band_staffing, roi_align_common.h)") \
  X(roi_align_fwd_grab, 0, 0, 64, "band forward: channels a workgroup reserves at a time, rounded up to whole fills; 0: the launcher's choice (2 for the fp32 packed arg-max forward, else 4)") \
  X(roi_align_fwd_tail, 0, 0, 100, "band forward: last per cent of a unit's channels handed out in smaller pieces") \
  X(roi_align_fwd_tail_planes, 8, 1, 8, "band forward: planes of such a piece; 8: whole fills")                        \
  X(roi_align_bwd, 2, INT_MIN, INT_MAX, "2 fused all-level kernel; 1 per-level LDS planes; 0 global atomics")          \
  X(roi_align_bwd_flt4, 1, INT_MIN, INT_MAX, "1: single-level float arg-max backward with four channel planes per workgroup when they fit") \
  X(roi_align_bwd_fx, 1, INT_MIN, INT_MAX, "1: band sums in 32-bit fixed point (bit-reproducible); 0: fp32 compare-and-swap adds, hardware order") \
  X(roi_align_bwd_pixbound, 1, INT_MIN, INT_MAX, "1: the list pre-pass bounds the weight per 4 x 4 pixel cell of a band (2-D difference array); 0: summed over the band's RoIs (what workspace-free calls get)") \
  X(roi_align_bwd_lists, 1, INT_MIN, INT_MAX, "workspace pre-pass: 1 RoI lists + tap tables per band unit, 2 lists only, 0 none") \
  X(roi_pool_fwd, 1, INT_MIN, INT_MAX, "1 four planes in LDS per workgroup when they fit, 2 one plane, 0 wave per (roi, channel)") \
  X(roi_pool_bwd, 1, INT_MIN, INT_MAX, "1 LDS planes, four channels per workgroup, 2 one channel, 0 global atomics")   \
  X(deform_psroi_bwd_patch, 1, INT_MIN, INT_MAX, "1 (RoI, channel) patch summed in LDS, one atomic per touched pixel; 0 one global atomic per tap") \
  X(proposal_topk, 0, INT_MIN, INT_MAX, "0 by level size, 1 single workgroup, 2 multi-workgroup")                      \
  X(soft_nms_threads, 256, INT_MIN, INT_MAX, "threads per problem: 64, 128 or 256")                                    \
  X(deform_gemm_split, 2, INT_MIN, INT_MAX, "2: scaled fp16 hi/lo split (needs operand maxima); 1: bf16 hi/lo split; 0: fp32 MFMA") \
  X(deform_gemm_vecstore, 1, INT_MIN, INT_MAX, "1: whole-tile plain stores of the split GEMM leave as 512-byte tile rows through LDS; 0: element stores from the accumulator layout (what unaligned C gets)") \
  X(deform_gemm_nt, 1, INT_MIN, INT_MAX, "1: those whole-tile stores are non-temporal; 0: plain")                      \
  X(deform_gemm_ksplit, 1, INT_MIN, INT_MAX, "1: tiles of a mostly empty last round are cut into k slices (atomic adds)") \
  X(dcn_im2col, 1, INT_MIN, INT_MAX, "1 LDS-plane im2col, 0 per-lane global gathers")                                  \
  X(dcn_window, 1, INT_MIN, INT_MAX, "1 stage only the touched range of each plane")                                   \
  X(dcn_im2col_pipe, 1, INT_MIN, INT_MAX, "1: 3x3 im2col with the next window loads before this channel is sampled, col rows stored as 1 KB pieces behind them (s_waitcnt vmcnt(3)); 0: stores in place") \
  X(dcn_col2im, 1, INT_MIN, INT_MAX, "1 four channels per workgroup, shared sample geometry, 0 one channel")           \
  X(dcn_col2im_fx, 1, INT_MIN, INT_MAX, "1: the layer's backward sums dX in fixed point (integer LDS adds), 0 fp32 compare-and-swap") \
  X(dcn_coord, 1, INT_MIN, INT_MAX, "1 LDS-plane offset gradient, 0 per-lane gathers")                                 \
  X(dcn_fused, 1, INT_MIN, INT_MAX, "1: the col-free entry points sample inside the GEMM; 0: im2col + GEMM")           \
  X(dcn_fused_tile, 0, INT_MIN, INT_MAX, "pixels per tile of the fused kernels (1..96), 0 = balanced over the CUs: partial-tile tests") \
  X(crowdhuman_front, 0, INT_MIN, INT_MAX, "0: ch_finish traces each front entry back through the swaps; 1: LDS replay")
// Knobs that switch parts of a kernel OFF for profiling (results are WRONG off their default) are rows only in the
// -DSD_PROFILING build (tools/libsimpledet_ops_hip_prof.so, `make prof`).  The product library cannot set them:
// there SD_PROF_TUNING(knob) is the default as a compile-time constant and the ablated branches are not in the code.
#define SD_PROF_KNOBS(X)                                                                                                \
  X(roi_align_fwd_ablate, 0, INT_MIN, INT_MAX, "parts of the RoIAlign forward switched off")                           \
  X(roi_pool_fwd_ablate, 0, INT_MIN, INT_MAX, "parts of the RoIPool forward switched off")                             \
  X(crowdhuman_target_stop, 0, INT_MIN, INT_MAX, "k in 1..3: sd_crowdhuman_target launches its first k kernels only")  \
  X(roi_align_bwd_ablate, 0, INT_MIN, INT_MAX, "parts of the RoIAlign backward switched off")                          \
  X(roi_align_dbg_lo, 0, INT_MIN, INT_MAX, "device buffer for per-wave phase clocks, low word of its address")         \
  X(roi_align_dbg_hi, 0, INT_MIN, INT_MAX, "the high word")                                                            \
  X(gemm_ablate, 0, INT_MIN, INT_MAX, "skip the A (1) / B (2) prefetch of the split GEMM")                             \
  X(gemm_dbg_cap, 0, INT_MIN, INT_MAX, "waves the buffer above has room for (split GEMM)")                             \
  X(dcn_im2col_nt, 1, INT_MIN, INT_MAX, "bits 1-2: parts of the LDS im2col switched off")                              \
  X(dcn_fused_ablate, 0, INT_MIN, INT_MAX, "parts of the fused forward switched off")
#ifdef SD_PROFILING
#define SD_KNOBS(X) SD_PRODUCT_KNOBS(X) SD_PROF_KNOBS(X)
#define SD_PROF_TUNING(knob) ::sd::tuning(::sd::Knob::knob)
#define SD_ABLATE(args, bits) ((args).ablate & (bits))
#else
#define SD_KNOBS(X) SD_PRODUCT_KNOBS(X)
namespace prof_default {
#define SD_KNOB_DEFAULT(id, dflt, lo, hi, what) constexpr int id = dflt;
SD_PROF_KNOBS(SD_KNOB_DEFAULT)
#undef SD_KNOB_DEFAULT
}  // namespace prof_default
#define SD_PROF_TUNING(knob) (::sd::prof_default::knob)
#define SD_ABLATE(args, bits) 0  // the ablated branches are not in the product code at all
#endif
// the value in effect, clamped to the row's range: one relaxed load (runtime.hip); a knob that is not in the list is
// no enumerator, so a mistyped read does not compile
#define SD_KNOB_ENUM(id, dflt, lo, hi, what) id,
enum class Knob : int { SD_KNOBS(SD_KNOB_ENUM) kCount };
#undef SD_KNOB_ENUM
int tuning(Knob knob);

static inline int cdiv(long a, long b) { return (int)((a + b - 1) / b); }

// Carves a caller's workspace into 256-byte aligned buffers.  A layout function takes its buffers from one
// carver in one order, so the size query (a null workspace: every take() is null and only counts) and the call
// (real pointers) cannot disagree.
static inline size_t round256(size_t v) { return (v + 255) / 256 * 256; }
struct WsCarver {
  char* base;      // the workspace rounded up to 256 bytes
  size_t off = 0;  // bytes taken from base
  size_t slack;    // bytes between the workspace and base
  explicit WsCarver(void* workspace)
      : base(reinterpret_cast<char*>(round256((size_t)(uintptr_t)workspace))),
        slack((size_t)(base - (char*)workspace)) {}
  template <typename T>
  T* take(size_t bytes) {
    T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
    off = round256(off + bytes);
    return p;
  }
  size_t need() const { return off + slack; }  // bytes of the caller's workspace in use
};

// clears n int counters on the stream with a kernel (runtime.hip)
void zero_counters(int* p, long n, hipStream_t stream);

// mshadow_op::maximum / minimum semantics (a > b ? a : b), kept explicit for NaN parity
__host__ __device__ static inline float fmaxr(float a, float b) { return a > b ? a : b; }
__host__ __device__ static inline float fminr(float a, float b) { return a < b ? a : b; }
__host__ __device__ static inline int imaxr(int a, int b) { return a > b ? a : b; }
__host__ __device__ static inline int iminr(int a, int b) { return a < b ? a : b; }

constexpr int kWave = 64;      // CDNA wavefront
constexpr int kNumXCD = 8;     // MI355X: 8 XCDs, block b is dispatched to XCD b % 8

// Compiler-level ordering of the LDS accesses of the lanes of ONE wave (the hardware already
// executes a wave's LDS instructions in order): without it a lane's loads may be hoisted above
// the stores other lanes issue in the same instruction stream.  Emits no instruction.
#if defined(__HIPCC__)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Wave-wide reductions on the VALU only (DPP butterfly inside each row of 16 lanes, then the four
// row results through v_readlane): no LDS traffic, unlike __shfl_xor (ds_bpermute_b32).  The result
// is wave-uniform.  Every lane must be active.
#define SD_DPP_STEP(x, ctrl) __builtin_amdgcn_update_dpp((x), (x), (ctrl), 0xf, 0xf, false)
__device__ __forceinline__ float wave_max_f32(float v) {
  v = fmaxr(v, __int_as_float(SD_DPP_STEP(__float_as_int(v), 0xB1)));   // quad_perm [1,0,3,2]
  v = fmaxr(v, __int_as_float(SD_DPP_STEP(__float_as_int(v), 0x4E)));   // quad_perm [2,3,0,1]
  v = fmaxr(v, __int_as_float(SD_DPP_STEP(__float_as_int(v), 0x141)));  // row_half_mirror
  v = fmaxr(v, __int_as_float(SD_DPP_STEP(__float_as_int(v), 0x140)));  // row_mirror
  const int x = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(x, 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(x, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(x, 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(x, 48));
  return fmaxr(fmaxr(r0, r1), fmaxr(r2, r3));
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += SD_DPP_STEP(v, 0xB1);
  v += SD_DPP_STEP(v, 0x4E);
  v += SD_DPP_STEP(v, 0x141);
  v += SD_DPP_STEP(v, 0x140);
  return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) +
         __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

// fp32 sum in a FIXED order (the butterfly's pairs, then the four rows left to right): equal bits on every call
__device__ __forceinline__ float wave_sum_f32(float v) {
  v += __int_as_float(SD_DPP_STEP(__float_as_int(v), 0xB1));
  v += __int_as_float(SD_DPP_STEP(__float_as_int(v), 0x4E));
  v += __int_as_float(SD_DPP_STEP(__float_as_int(v), 0x141));
  v += __int_as_float(SD_DPP_STEP(__float_as_int(v), 0x140));
  const int x = __float_as_int(v);
  const float r0 = __int_as_float(__builtin_amdgcn_readlane(x, 0));
  const float r1 = __int_as_float(__builtin_amdgcn_readlane(x, 16));
  const float r2 = __int_as_float(__builtin_amdgcn_readlane(x, 32));
  const float r3 = __int_as_float(__builtin_amdgcn_readlane(x, 48));
  return (r0 + r1) + (r2 + r3);
}

// max|.| of four gradients as the maximum of the BIT PATTERNS of |.| (non-negative floats order like unsigned
// integers; a NaN's pattern lies above inf's, so it survives every maximum -- `a > b ? a : b` on floats drops a NaN
// in its first operand, which let NaN gradients slip past the "non-finite -> float adds" test until round 6)
constexpr unsigned kFltMaxBits = 0x7f7fffffu;
__device__ __forceinline__ unsigned umaxr(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned absbits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
__device__ __forceinline__ unsigned absbits4(const float4& v) {
  return umaxr(umaxr(absbits(v.x), absbits(v.y)), umaxr(absbits(v.z), absbits(v.w)));
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
  v = umaxr(v, (unsigned)SD_DPP_STEP((int)v, 0xB1));
  v = umaxr(v, (unsigned)SD_DPP_STEP((int)v, 0x4E));
  v = umaxr(v, (unsigned)SD_DPP_STEP((int)v, 0x141));
  v = umaxr(v, (unsigned)SD_DPP_STEP((int)v, 0x140));
  const int x = (int)v;
  return umaxr(umaxr((unsigned)__builtin_amdgcn_readlane(x, 0), (unsigned)__builtin_amdgcn_readlane(x, 16)),
               umaxr((unsigned)__builtin_amdgcn_readlane(x, 32), (unsigned)__builtin_amdgcn_readlane(x, 48)));
}

// inclusive prefix sum over the 64 lanes on the VALU: row_shr 1 / 2 / 4 / 8 inside each row of 16 lanes (a lane
// whose source lies before its row keeps 0), then row_bcast:15 into rows 1 and 3 and row_bcast:31 into rows 2
// and 3.  Every lane must be active.
__device__ __forceinline__ int wave_scan_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return v;
}

// 32-bit fixed-point LDS sums have ONE unit per workgroup: 2^-30 .. 2^-29 of (max|g| x weight bound).  That is
// fine while the gradients of a workgroup span a few octaves; under heavy tails -- one element 10^4 x the
// typical one -- the typical elements would be rounded to a few units.  So every fixed-point backward looks at
// the dynamic range it actually streams and keeps the integer adds only while the unit is below ~2^-13 of the
// GEOMETRIC mean of its non-zero gradients (the mean itself is useless here: a lognormal's mean sits far out in
// its tail).  In exponents, all integer and therefore independent of any summation order:
//     E(max|g|) + ceil(log2(weight bound)) <= mean E(g) + kFxRangeBits - 1  (E = biased fp32 exponent field),
// the mean taken over a fixed sample of the stream (the first element of a 16-byte item, on the trips
// fx_range_stride_mask picks: every fourth trip of the band kernel at the baseline), zeros and denormals not
// counted.  Near-Gaussian gradients: E(max) - mean E ~ 3.5-4, so weight bounds up to ~2^11 pass;
// a loss scale cancels out.  A workgroup that fails takes the fp32 compare-and-swap adds -- the reference's own
// arithmetic (roi_align_v2.cu:67-83, upstream deformable_col2im: a float atomicAdd per tap).
constexpr int kFxRangeBits = 16;   // (the threshold below adds one bit for the optimistic maximum: 15 against the true one)
__device__ __forceinline__ int fp32_exponent_field(float v) { return (int)((__float_as_uint(v) >> 23) & 255u); }
__device__ __forceinline__ int ceil_log2_i32(int b) { return b <= 1 ? 0 : 32 - __builtin_clz((unsigned)(b - 1)); }
// The statistic travels as ONE integer per thread / wave / workgroup (one wave reduction, one LDS atomic, one LDS
// read behind the barrier that ends the scatter anyway -- every instruction in a short-lived workgroup's chain
// counts: two reductions and a 64-bit verdict cost the headline backward 2 us): per non-zero sample
//     ((E(g) - 127) << 12) + 1,
// so the upper bits sum the exponents about 127 and the low 12 bits count the samples.  The callers thin their
// sampling to fewer than 4096 samples per workgroup, so the count never carries, and |E - 127| <= 127 keeps the
// exponent sum below 2^19 in magnitude: the int32 never wraps, whatever the data (a threshold taken from the
// optimistic maximum would not do: a first trip of zeros puts it ~140 below every sample).  The threshold
//     e_thr = E(optimistic max|g|) + 1 + ceil(log2(weight bound)) - kFxRangeBits
// enters only in fx_range_fine: fine <=> the margins E(g) - e_thr sum to >= 0; when the true maximum turns out
// more than twice the optimistic one they are corrected by the difference of the exponents times the count.
__device__ __forceinline__ int fx_range_thr(float gmax_used, int bound) {
  return fp32_exponent_field(gmax_used) + 1 + ceil_log2_i32(bound) - kFxRangeBits;
}
__device__ __forceinline__ int fx_range_sample(float v) {
  const int ex = fp32_exponent_field(v);
  return ex ? ((ex - 127) << 12) + 1 : 0;
}
__device__ __forceinline__ bool fx_range_fine(int packed, int e_thr, float gmax_used, float gmax_true) {
  const int cnt = packed & 4095, esum = packed >> 12;   // esum = sum of (E - 127), |esum| < 2^19
  const int extra = fp32_exponent_field(gmax_true) - (fp32_exponent_field(gmax_used) + 1);
  // sum of the margins minus the correction, exact in int32: |127 - e_thr - extra| < 2^10, cnt < 2^12
  return esum + cnt * (127 - e_thr - (extra > 0 ? extra : 0)) >= 0;
}
// trips between samples (a power of two minus one) so that `per_trip` samples per trip over `trips` trips stay < 4096
__device__ __forceinline__ int fx_range_stride_mask(long per_trip, long trips, int at_least = 0) {
  int m = at_least;
  while (per_trip * ((trips + m) / (m + 1)) > 4000) m = 2 * m + 1;
  return m;
}

// fp32 add into an LDS word by compare-and-swap.  ds_add_f32 runs at ~0.33 lane-ops/clk/CU on
// gfx950 against ~2 for this loop and 4-9 for the integer LDS atomics (tools/lds_atomic_bench.hip,
// tools/lds_scatter_bench.hip), so every gradient plane kept in LDS is accumulated this way.
__device__ __forceinline__ void lds_add_cas(float* p, float v) {
  int* ip = reinterpret_cast<int*>(p);
  int old = *ip;
  while (true) {
    const int assumed = old;
    old = atomicCAS(ip, assumed, __float_as_int(__int_as_float(assumed) + v));
    if (old == assumed) break;
  }
}
#endif
constexpr int kNumCU = 256;

}  // namespace sd
