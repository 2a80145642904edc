// Hard NMS in the reference's float32 numpy arithmetic, batched, and the BboxPostProcessing operator of
// Mask R-CNN's test graph (filter -> per-class hard NMS -> image top-k) for gfx950.
//   reference: operator_py/nms.py:41-75 (nms: numpy, float32 throughout) through py_nms_wrapper :19-22;
//              models/maskrcnn/bbox_post_processing.py:6-32 (multiclass_nms), :43-72 (operator forward),
//              :74-76 / :110-111 (zero gradients, no entry point here); node built at
//              models/maskrcnn/builder.py:65-84; the same nms is the default of detection_test.py:224-267
//              with "keep the best max_det_per_image" at :290.
// This is NOT sd_soft_nms_batched(method 0): the Cython soft_nms adds 1 in double and picks by a running
// arg-max; here every operation is a float32 operation (nms.py:55, :62-70):
//     area = (x2 - x1 + 1) * (y2 - y1 + 1)      w = max(0, min(x2i, x2j) - max(x1i, x1j) + 1)   (h likewise)
//     ovr  = w * h / (area_i + area_j - w * h)  kept iff ovr <= float32(thresh): a NaN ovr suppresses
// (np.maximum / np.minimum hand a NaN operand on).  The library is built with -ffp-contract=off and the
// correctly rounded divide, so the expressions below are those operations one for one.
// Order: boxes are visited by descending score; AMONG EQUAL SCORES THE ROW LATER IN THE INPUT COMES FIRST
// (what argsort(kind="stable")[::-1] gives; the reference's own order of equal scores is whatever numpy's
// unstable sort leaves).  That is the opposite of sd_nms, whose stable sort keeps the lower row first.
// A NaN score (sd_hard_nms_batched only; the operator's `score > min_det_score` drops them) sorts before
// every number, as numpy's sort places NaNs last and the reversal first.
//
// One workgroup per problem, everything in LDS:
//   1. the rows over the threshold become 64-bit keys (order-preserving score bits | row) -- compacted by
//      wave ballots, an empty problem returns at once (most classes of an image are empty at 0.05);
//   2. bitonic sort (select_common.h sorts ascending, so the keys are held complemented: the best key
//      first, and the row in the low word gives the tie rule for free);
//   3. greedy suppression in chunks of 64 sorted boxes: the waves ballot the chunk's 64 x 64 triangle row by
//      row (rows of boxes already dead are skipped), every wave replays the greedy pass over those 64 words
//      in scalar code, then all waves strike the later boxes against the chunk's kept ones.  No n^2 / 8
//      byte matrix; two workgroup barriers per chunk.
// The operator's kept records (the sorted keys, in NMS order) go to the workspace; a second launch, one
// workgroup per image, takes the max_det_per_image best of them: a kernel boundary is the hand-over.
#include "common.h"
#include "select_common.h"
#include "../../include/simpledet_ops.h"

namespace sd {

constexpr int kBpThreads = 256;
constexpr int kBpMaxRows = 4096;      // sorted boxes of one problem in LDS; 12 bits of rank in the top-k key
constexpr int kBpMaxClasses = 256;
constexpr int kBpMaxDet = 1024;

// a key is (order-preserving score bits << 32 | low word), larger = better; LDS and the workspace hold the
// COMPLEMENT (ascending sort = best first), ~0 = "no entry"
typedef unsigned long long BpKey;
constexpr BpKey kBpNone = ~0ull;

// np.maximum / np.minimum: a NaN operand is handed on (only its NaN-ness matters below)
__device__ __forceinline__ float bp_np_max(float a, float b) { return (a > b || a != a) ? a : b; }
__device__ __forceinline__ float bp_np_min(float a, float b) { return (a < b || a != a) ? a : b; }

// monotone in the score over the non-NaN floats (-0.0 == +0.0), every NaN above +inf; never 0
__device__ __forceinline__ unsigned bp_score_ord(float s) {
  if (s != s) return 0xffffffffu;
  const unsigned b = __float_as_uint(s + 0.0f);
  return b ^ ((unsigned)((int)b >> 31) | 0x80000000u);
}
__device__ __forceinline__ BpKey bp_key(float s, unsigned low) { return ~(((BpKey)bp_score_ord(s) << 32) | low); }
__device__ __forceinline__ unsigned bp_low(BpKey inv) { return ~(unsigned)inv; }

// true when box j does NOT survive box i (nms.py:62-72): !(ovr <= thresh)
__device__ __forceinline__ bool bp_suppresses(float ix1, float iy1, float ix2, float iy2, float jx1, float jy1,
                                              float jx2, float jy2, float thresh) {
  const float area_i = (ix2 - ix1 + 1.f) * (iy2 - iy1 + 1.f);
  const float area_j = (jx2 - jx1 + 1.f) * (jy2 - jy1 + 1.f);
  const float w = bp_np_max(0.f, bp_np_min(ix2, jx2) - bp_np_max(ix1, jx1) + 1.f);
  const float h = bp_np_max(0.f, bp_np_min(iy2, jy2) - bp_np_max(iy1, jy1) + 1.f);
  const float inter = w * h;
  const float ovr = inter / (area_i + area_j - inter);
  return !(ovr <= thresh);
}

__device__ __forceinline__ unsigned long long bp_readlane64(unsigned long long v, int l) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, l);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), l);
  return ((unsigned long long)hi << 32) | lo;
}
__device__ __forceinline__ unsigned long long bp_uniform64(unsigned long long v) {
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
  const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
  return ((unsigned long long)hi << 32) | lo;
}

struct HardNmsArgs {
  // mode 0: sd_hard_nms_batched
  const float* dets;
  const int* counts;
  float* out_dets;
  int* out_inds;
  int* out_counts;
  // mode 1: the operator's per-(image, foreground class) pass
  const float* cls_score;
  const float* bbox;
  BpKey* ws_keys;   // (B * (K - 1), R): kept keys in NMS order
  int* ws_counts;   // (B * (K - 1))
  int K, Kb;
  float min_score;
  int mode;
  int N;            // rows per problem (Nmax, or R)
  float thresh;
};

__global__ __launch_bounds__(kBpThreads) void bbox_post_hard_nms_kernel(HardNmsArgs a) {
  constexpr int NW = kBpThreads / kWave;
  extern __shared__ __attribute__((aligned(16))) unsigned char bp_smem[];
  const int N = a.N;
  int np2cap = 1;
  while (np2cap < N) np2cap <<= 1;
  BpKey* KEY = reinterpret_cast<BpKey*>(bp_smem);              // [np2cap]
  unsigned long long* ALIVE = KEY + np2cap;                    // [(N + 63) / 64]
  unsigned long long* ROWM = ALIVE + (N + 63) / 64;            // [64]
  float* X1 = reinterpret_cast<float*>(ROWM + kWave);          // [N] each
  float* Y1 = X1 + N;
  float* X2 = Y1 + N;
  float* Y2 = X2 + N;
  int* PREF = reinterpret_cast<int*>(Y2 + N);                  // [64]
  int* CTRL = PREF + kWave;                                    // [0] candidates, [1] kept

  const int p = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const unsigned long long lt_mask = (1ull << lane) - 1;

  // ---- 1. keys of the candidate rows ----
  int n;
  int img = 0, cls = 0;
  if (a.mode == 0) {
    n = a.counts ? a.counts[p] : N;
    n = n < 0 ? 0 : (n > N ? N : n);
    if (n == 0) {
      if (tid == 0) a.out_counts[p] = 0;
      return;
    }
    const float* src = a.dets + (long)p * N * 5;
    for (int r = tid; r < n; r += kBpThreads) KEY[r] = bp_key(src[(long)r * 5 + 4], (unsigned)r);
  } else {
    img = p / (a.K - 1);
    cls = p % (a.K - 1) + 1;   // column of cls_score; the emitted class id is cls - 1
    if (tid == 0) CTRL[0] = 0;
    __syncthreads();
    const float* sc = a.cls_score + (long)img * N * a.K + cls;
    for (int base = 0; base < N; base += kBpThreads) {
      const int r = base + tid;
      float s = 0.f;
      bool pass = false;
      if (r < N) {
        s = sc[(long)r * a.K];
        pass = s > a.min_score;   // NaN fails
      }
      const unsigned long long bal = __ballot(pass);
      if (bal) {   // wave-uniform
        int wbase = 0;
        if (lane == 0) wbase = atomicAdd(&CTRL[0], __popcll(bal));
        wbase = __builtin_amdgcn_readfirstlane(wbase);
        // the position among the candidates is irrelevant: the sort orders them by (score, row)
        if (pass) KEY[wbase + __popcll(bal & lt_mask)] = bp_key(s, (unsigned)r);
      }
    }
    __syncthreads();
    n = CTRL[0];
    if (n == 0) {
      if (tid == 0) a.ws_counts[p] = 0;
      return;
    }
  }

  // ---- 2. sort: score descending, later row first ----
  int np2 = 1;
  while (np2 < n) np2 <<= 1;
  for (int r = n + tid; r < np2; r += kBpThreads) KEY[r] = kBpNone;
  const int nwords = (n + 63) >> 6;
  for (int w = tid; w < nwords; w += kBpThreads)
    ALIVE[w] = (w + 1) * 64 <= n ? ~0ull : ((1ull << (n & 63)) - 1);
  __syncthreads();
  bitonic_sort_lds(KEY, np2, tid, kBpThreads);
  __syncthreads();

  // ---- boxes in sorted order ----
  for (int j = tid; j < n; j += kBpThreads) {
    const int r = (int)bp_low(KEY[j]);
    const float* bx = a.mode == 0 ? a.dets + ((long)p * N + r) * 5
                                  : a.bbox + ((long)img * N + r) * 4 * a.Kb + (a.Kb == 1 ? 0 : 4 * cls);
    X1[j] = bx[0];
    Y1[j] = bx[1];
    X2[j] = bx[2];
    Y2[j] = bx[3];
  }
  __syncthreads();

  // ---- 3. greedy suppression, 64 sorted boxes at a time ----
  const float thr = a.thresh;
  for (int c = 0; c < nwords; ++c) {
    // the strikes of the earlier chunks are behind a barrier
    const unsigned long long start = bp_uniform64(ALIVE[c]);
    if (start == 0) continue;
    const int base = c << 6;
    const int m = n - base < kWave ? n - base : kWave;
    // the triangle: row i = the boxes j > i of this chunk that box i suppresses
    {
      const int j = base + lane;
      const bool inr = lane < m;
      const float jx1 = inr ? X1[j] : 0.f, jy1 = inr ? Y1[j] : 0.f, jx2 = inr ? X2[j] : 0.f, jy2 = inr ? Y2[j] : 0.f;
      for (int i = wave; i < m; i += NW) {
        if (!((start >> i) & 1ull)) continue;
        const float ix1 = X1[base + i], iy1 = Y1[base + i], ix2 = X2[base + i], iy2 = Y2[base + i];
        const bool sup = inr && lane > i && bp_suppresses(ix1, iy1, ix2, iy2, jx1, jy1, jx2, jy2, thr);
        const unsigned long long row = __ballot(sup);
        if (lane == 0) ROWM[i] = row;
      }
    }
    __syncthreads();
    // every wave replays the greedy pass over the rows (scalar code on v_readlane)
    unsigned long long kept = start;
    {
      const unsigned long long myrow = (lane < m && ((start >> lane) & 1ull)) ? ROWM[lane] : 0ull;
      for (int i = 0; i < m; ++i) {
        const unsigned long long row = bp_readlane64(myrow, i);
        if ((kept >> i) & 1ull) kept &= ~row;
      }
    }
    if (tid == 0) ALIVE[c] = kept;
    // strike the later boxes; word wd belongs to exactly one wave
    for (int wd = c + 1 + wave; wd < nwords; wd += NW) {
      const unsigned long long aw = bp_uniform64(ALIVE[wd]);
      if (aw == 0) continue;
      const int j = (wd << 6) + lane;
      bool alive = (aw >> lane) & 1ull;   // bits past n are clear
      float jx1 = 0.f, jy1 = 0.f, jx2 = 0.f, jy2 = 0.f;
      if (alive) {
        jx1 = X1[j]; jy1 = Y1[j]; jx2 = X2[j]; jy2 = Y2[j];
      }
      unsigned long long k = kept;
      while (k) {
        const int i = base + __ffsll((long long)k) - 1;
        k &= k - 1;
        if (alive && bp_suppresses(X1[i], Y1[i], X2[i], Y2[i], jx1, jy1, jx2, jy2, thr)) alive = false;
        if (!__any(alive)) break;
      }
      const unsigned long long nw = __ballot(alive);
      if (lane == 0) ALIVE[wd] = nw;
    }
    __syncthreads();
  }

  // ---- output: the kept boxes in sorted order ----
  if (wave == 0) {
    const int cnt = lane < nwords ? __popcll(ALIVE[lane]) : 0;
    const int incl = wave_scan_i32(cnt);
    PREF[lane] = incl - cnt;
    if (lane == kWave - 1) CTRL[1] = incl;
  }
  __syncthreads();
  const int total = CTRL[1];
  if (tid == 0) {
    if (a.mode == 0) a.out_counts[p] = total;
    else a.ws_counts[p] = total;
  }
  for (int j = tid; j < n; j += kBpThreads) {
    const unsigned long long w = ALIVE[j >> 6];
    if (!((w >> (j & 63)) & 1ull)) continue;
    const int pos = PREF[j >> 6] + __popcll(w & ((1ull << (j & 63)) - 1));
    if (a.mode == 0) {
      const int r = (int)bp_low(KEY[j]);
      const float* src = a.dets + ((long)p * N + r) * 5;
      float* dst = a.out_dets + ((long)p * N + pos) * 5;
#pragma unroll
      for (int f = 0; f < 5; ++f) dst[f] = src[f];
      a.out_inds[(long)p * N + pos] = r;
    } else {
      a.ws_keys[(long)p * N + pos] = KEY[j];
    }
  }
}

// ---- the image's max_det best of the kept records (bbox_post_processing.py:29-32, :58-68) ----
// key: score bits | class << 12 | rank in the class's NMS order -- the low word grows with the position in the
// stacked (class, NMS order) list, so "best key first" IS "score descending, later entry first".
// The best `top` keys live in BUF[0, top); candidates better than the current top-th key are staged from
// BUF[top2] on and merged by a sort whenever the staging area cannot take another trip.
struct BpTopkArgs {
  const float* cls_score;
  const float* bbox;
  const BpKey* ws_keys;
  const int* ws_counts;
  float* post_score;
  float* post_bbox;
  float* post_cls;
  int R, K, Kb, top, top2, bufn;
};

__global__ __launch_bounds__(kBpThreads) void bbox_post_topk_kernel(BpTopkArgs a) {
  constexpr int NW = kBpThreads / kWave;
  extern __shared__ __attribute__((aligned(16))) unsigned char bp_smem[];
  BpKey* BUF = reinterpret_cast<BpKey*>(bp_smem);             // [bufn]
  int* OFF = reinterpret_cast<int*>(BUF + a.bufn);            // [kBpMaxClasses + 1] exclusive offsets
  int* WSUM = OFF + kBpMaxClasses + 1;                        // [NW]
  int* CTRL = WSUM + NW;                                      // [0] staged

  const int img = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int nc = a.K - 1;   // <= 255 problems per image
  const int* counts = a.ws_counts + (long)img * nc;

  // exclusive offsets of the classes in the stacked list
  {
    const int cnt = tid < nc ? counts[tid] : 0;
    const int incl = wave_scan_i32(cnt);
    if (lane == kWave - 1) WSUM[wave] = incl;
    for (int i = tid; i < a.bufn; i += kBpThreads) BUF[i] = kBpNone;
    if (tid == 0) CTRL[0] = 0;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += WSUM[w];
    OFF[tid + 1] = before + incl;
    if (tid == 0) OFF[0] = 0;
    __syncthreads();
  }
  const int M = OFF[nc];
  const int stage_cap = a.bufn - a.top2;   // >= kBpThreads
  const unsigned long long lt_mask = (1ull << lane) - 1;
  BpKey bar = kBpNone;   // the top-th best so far ("none" while fewer are held); keys are pairwise distinct
  for (int g0 = 0; g0 < M; g0 += kBpThreads) {
    const int g = g0 + tid;
    BpKey key = kBpNone;
    if (g < M) {
      int lo = 0, hi = nc - 1;   // the last class whose offset is <= g
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (OFF[mid] <= g) lo = mid; else hi = mid - 1;
      }
      const int rank = g - OFF[lo];
      const BpKey rec = a.ws_keys[((long)img * nc + lo) * a.R + rank];
      key = (rec & 0xffffffff00000000ull) | (unsigned)~(unsigned)((lo << 12) | rank);
    }
    const bool want = key < bar;
    const unsigned long long bal = __ballot(want);
    if (bal) {
      int wbase = 0;
      if (lane == 0) wbase = atomicAdd(&CTRL[0], __popcll(bal));
      wbase = __builtin_amdgcn_readfirstlane(wbase);
      if (want) BUF[a.top2 + wbase + __popcll(bal & lt_mask)] = key;
    }
    __syncthreads();
    const int staged = CTRL[0];
    __syncthreads();   // everyone has read the count before the next trip adds to it
    if (staged + kBpThreads > stage_cap || g0 + kBpThreads >= M) {
      bitonic_sort_lds(BUF, a.bufn, tid, kBpThreads);
      __syncthreads();
      bar = BUF[a.top - 1];
      __syncthreads();
      for (int i = a.top + tid; i < a.bufn; i += kBpThreads) BUF[i] = kBpNone;
      if (tid == 0) CTRL[0] = 0;
      __syncthreads();
    }
  }

  for (int t = tid; t < a.top; t += kBpThreads) {
    const BpKey key = BUF[t];
    float s = 0.f, c = -1.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    if (key != kBpNone) {
      const unsigned low = bp_low(key);
      const int ci = (int)(low >> 12), rank = (int)(low & 4095u);
      const int r = (int)bp_low(a.ws_keys[((long)img * nc + ci) * a.R + rank]);
      s = a.cls_score[((long)img * a.R + r) * a.K + ci + 1];
      const float* bx = a.bbox + ((long)img * a.R + r) * 4 * a.Kb + (a.Kb == 1 ? 0 : 4 * (ci + 1));
      b0 = bx[0]; b1 = bx[1]; b2 = bx[2]; b3 = bx[3];
      c = (float)ci;
    }
    const long o = (long)img * a.top + t;
    a.post_score[o] = s;
    a.post_cls[o] = c;
    a.post_bbox[o * 4 + 0] = b0;
    a.post_bbox[o * 4 + 1] = b1;
    a.post_bbox[o * 4 + 2] = b2;
    a.post_bbox[o * 4 + 3] = b3;
  }
}

static size_t hard_nms_lds_bytes(int N) {
  size_t np2 = 1;
  while (np2 < (size_t)N) np2 <<= 1;
  return np2 * 8 + ((size_t)(N + 63) / 64) * 8 + 64 * 8 + (size_t)N * 16 + 64 * 4 + 16;
}

static int launch_hard_nms(const HardNmsArgs& a, int P, hipStream_t stream) {
  const size_t lds = hard_nms_lds_bytes(a.N);
  if (lds > 64 * 1024)
    SD_HIP_CHECK(hipFuncSetAttribute((const void*)bbox_post_hard_nms_kernel,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(bbox_post_hard_nms_kernel, dim3(P), dim3(kBpThreads), lds, stream, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

static size_t bp_counts_offset(int B, int R, int K) {
  return (size_t)B * (size_t)(K - 1) * (size_t)R * sizeof(BpKey);
}

}  // namespace sd

using namespace sd;

extern "C" int sd_hard_nms_batched(const float* dets, const int32_t* counts, int P, int Nmax, float thresh,
                                   float* out_dets, int32_t* out_inds, int32_t* out_counts, void* stream) {
  SD_REQUIRE(P >= 0 && Nmax >= 0, "negative dimension");
  if (Nmax > kBpMaxRows)
    return fail(SD_ERR_UNSUPPORTED, "hard_nms: Nmax=%d above %d rows per problem", Nmax, kBpMaxRows);
  if (P == 0) return SD_OK;
  SD_REQUIRE(out_counts, "out_counts is null");
  if (Nmax == 0) {
    SD_HIP_CHECK(hipMemsetAsync(out_counts, 0, sizeof(int) * (size_t)P, (hipStream_t)stream));
    return SD_OK;
  }
  SD_REQUIRE(dets && out_dets && out_inds, "null tensor pointer");
  HardNmsArgs a{};
  a.dets = dets;
  a.counts = counts;
  a.out_dets = out_dets;
  a.out_inds = out_inds;
  a.out_counts = out_counts;
  a.mode = 0;
  a.N = Nmax;
  a.thresh = thresh;
  return launch_hard_nms(a, P, (hipStream_t)stream);
}

extern "C" size_t sd_bbox_post_processing_workspace_bytes(int B, int R, int K, int bbox_classes, int max_det) {
  (void)bbox_classes;
  (void)max_det;
  if (B <= 0 || R <= 0 || K <= 1) return 16;
  return bp_counts_offset(B, R, K) + (size_t)B * (size_t)(K - 1) * sizeof(int) + 16;
}

extern "C" int sd_bbox_post_processing(const float* cls_score, const float* bbox_xyxy, int B, int R, int K,
                                       int bbox_classes, float min_det_score, float nms_thr,
                                       int max_det_per_image, float* post_score, float* post_bbox,
                                       float* post_cls, void* workspace, size_t workspace_bytes, void* stream) {
  SD_REQUIRE(B >= 0 && R >= 0 && K >= 1 && max_det_per_image >= 0, "negative dimension");
  if (R > kBpMaxRows || K > kBpMaxClasses || max_det_per_image > kBpMaxDet)
    return fail(SD_ERR_UNSUPPORTED, "bbox_post_processing: R=%d K=%d max_det_per_image=%d outside R <= %d, "
                "K <= %d, max_det_per_image <= %d", R, K, max_det_per_image, kBpMaxRows, kBpMaxClasses, kBpMaxDet);
  if (bbox_classes != 1 && bbox_classes != K)
    return fail(SD_ERR_UNSUPPORTED, "bbox_post_processing: bbox_classes=%d is neither 1 nor K=%d", bbox_classes, K);
  if (B == 0 || max_det_per_image == 0) return SD_OK;
  SD_REQUIRE(post_score && post_bbox && post_cls, "null output pointer");
  const size_t need = sd_bbox_post_processing_workspace_bytes(B, R, K, bbox_classes, max_det_per_image);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "bbox_post_processing: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  SD_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace must be 8-byte aligned");
  const bool any = R > 0 && K > 1;
  SD_REQUIRE(!any || (cls_score && bbox_xyxy), "null tensor pointer");
  BpKey* ws_keys = reinterpret_cast<BpKey*>(workspace);
  int* ws_counts = any ? reinterpret_cast<int*>(reinterpret_cast<unsigned char*>(workspace) + bp_counts_offset(B, R, K))
                       : reinterpret_cast<int*>(workspace);
  if (any) {
    HardNmsArgs a{};
    a.cls_score = cls_score;
    a.bbox = bbox_xyxy;
    a.ws_keys = ws_keys;
    a.ws_counts = ws_counts;
    a.K = K;
    a.Kb = bbox_classes;
    a.min_score = min_det_score;
    a.mode = 1;
    a.N = R;
    a.thresh = nms_thr;
    const int rc = launch_hard_nms(a, B * (K - 1), (hipStream_t)stream);
    if (rc != SD_OK) return rc;
  }
  BpTopkArgs t{};
  t.cls_score = cls_score;
  t.bbox = bbox_xyxy;
  t.ws_keys = ws_keys;
  t.ws_counts = ws_counts;
  t.post_score = post_score;
  t.post_bbox = post_bbox;
  t.post_cls = post_cls;
  t.R = R;
  t.K = any ? K : 1;   // no candidate anywhere: the launch writes the padding only
  t.Kb = bbox_classes;
  t.top = max_det_per_image;
  t.top2 = 1;
  while (t.top2 < t.top) t.top2 <<= 1;
  t.bufn = 2 * t.top2 < 2 * kBpThreads ? 2 * kBpThreads : 2 * t.top2;
  const size_t lds = (size_t)t.bufn * 8 + (kBpMaxClasses + 1 + kBpThreads / kWave + 4) * sizeof(int);
  hipLaunchKernelGGL(bbox_post_topk_kernel, dim3(B), dim3(kBpThreads), lds, (hipStream_t)stream, t);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
