// RepPoints test-time decode for gfx950, fp32: per-level top-k of the best class score, the boxes of the selected
// locations and their score rows in ONE call.
//
// The reference (the spec) is RepPointsHead.get_prediction (models/RepPoints/builder.py:486-576): per level two
// transposes and reshapes, a sigmoid over all N*HW*C scores, a max, a full topk and per image a chain of slice,
// reshape, three take, concat, scale, add and four clip chains; then a padded column and the concat of the levels.
// Per level l and image i, with p = y*W + x and s = stride_l:
//   builder.py:518      score[p, c] = cls[i, c, y, x] (input_logits = 0) or 1.0f / (1.0f + expf(-cls)) per element
//                       (input_logits = 1; loss_common.h sigmoid_f32: the expression sd_fcos_sigmoid computes, equal bits).  The
//                       sigmoid is NOT taken of the maximum logit: nothing says expf is monotone to the last bit.
//   builder.py:519      m[p] = max_c score[p, c]
//   builder.py:520      the K_l best m in descending order, K_l = k_l > 0 ? k_l : H_l*W_l (MXNet topk, k < 1 = all).
//                       Ties (MXNet's order among equal keys is not documented; the project's rule, select_common.h):
//                       the lower p first; -0.0 == +0.0; NaN is ordered by its bits and is not part of the contract.
//   builder.py:569-574  rank r of level l is output row (sum_{l' < l} K_l') + r: the levels are concatenated in the
//                       order given and there is NO batch sort.
//   builder.py:559-562  cls_score[i, row, 0] = 0, cls_score[i, row, 1 + c] = score[p, c]
//   builder.py:504-509  box = _points2bbox(pts_out_refine, transform, y_first=True) at p (reppoints_common.h)
//   builder.py:541      b = box * s + (x*s, y*s, x*s, y*s): a float32 product, then a float32 add
//   builder.py:545-548  max(min(b, lim), 0) with lim = im_info[i, 1] - 1 for x and im_info[i, 0] - 1 for y
//
// MI355X design (all launches on the caller's stream, nothing read back by the host, no device allocation, no
// atomics on global memory, no counter to clear: every call and every graph replay gives equal bits).  The work is
// launch- and latency-bound (about 9 MB in, 1.1 MB out at the config's shapes):
//   1. rd_max_kernel     grid over (64-location chunk of a level, image), all levels in one grid.  A lane owns a
//                        location, so the loads of a wave are coalesced along W; the four waves of a workgroup split
//                        the C channel planes (eight independent scalar loads in flight per lane) and combine their
//                        maxima through LDS.  cls is streamed once here; m goes to the workspace as (N, P) floats.
//                        The order of a float maximum matters only for the sign of a zero, which the selection
//                        ignores, and the outputs never hold m.
//   2. rd_select_kernel  one workgroup per (level, image): a radix select of the K_l-th best key over the level's
//                        H_l*W_l maxima, ties by location, and an LDS sort of the K_l selected (key, location) words;
//                        the locations go to the workspace as (N, R) ints.  Levels up to 24,576 locations (the
//                        config's largest has 16,700) are selected from registers (rd_select_regs), larger ones by
//                        select_sort_topk (select_common.h); both follow the same rule.
//   3. rd_gather_kernel  workgroups over 16 output rows: one lane per row reads the 2 * num_points point channels of
//                        its location (H*W apart) and forms the box; then all lanes read the rows' C scores (H*W
//                        apart, sigmoid again when fused: same expression, same bits) and store the (C + 1)-float
//                        rows coalesced.
// Every element of both outputs is written by every call.  Loads are scalar, so any 4-byte aligned pointer gives
// the same bits.  Arithmetic: -ffp-contract=off, correctly rounded divide and sqrt (Makefile).
#include "loss_common.h"
#include "reppoints_common.h"
#include "select_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {
namespace {

constexpr int kRdMaxL = SD_MAX_FPN_LEVELS;
constexpr int kRdT = 256;
constexpr int kRdWaves = kRdT / kWave;
static_assert(kRdWaves == 4, "rd_max_kernel combines four per-wave maxima");
constexpr int kRdUnroll = 8;                  // scalar loads in flight per lane
constexpr int kRdSelT = 1024;                  // threads of the selecting workgroup
constexpr int kRdRegKeys = 24;                 // keys a selecting thread holds in registers: levels up to 24,576
constexpr int kRdRep = 8;                      // copies of the radix histogram (a power of two)
constexpr int kRdRows = 16;                   // output rows per gather workgroup
constexpr int kRdCap = kMaxSortKeys;           // words the LDS sort holds
constexpr long kRdMaxHW = 1L << 24;            // select_sort_topk's tie select holds row indices below 2^24
constexpr int kRdMaxImages = 65535;            // gridDim.y
constexpr long kRdMaxElems = 2147483647L;

struct RdArgs {
  const float* cls[kRdMaxL];
  const float* pts[kRdMaxL];
  int H[kRdMaxL], W[kRdMaxL], stride[kRdMaxL], K[kRdMaxL];
  int m_begin[kRdMaxL];            // first location of the level in an image's m
  int row_begin[kRdMaxL + 1];      // first output row of the level
  int wg_begin[kRdMaxL + 1];       // first workgroup of the level in rd_max_kernel's grid
  const float* im_info;
  const float* mt;
  int L, N, C, num_points, transform, logits, R;
  long P;
  float* cls_score;
  float* bbox;
  float* m;                        // workspace (N, P)
  int* sel;                        // workspace (N, R)
};

// step 1, grid (sum of the levels' chunks, N)
__global__ __launch_bounds__(kRdT) void rd_max_kernel(RdArgs a) {
  __shared__ float sm[kRdWaves][kWave];
  int l = 0;
  while (l + 1 < a.L && (int)blockIdx.x >= a.wg_begin[l + 1]) ++l;
  const int img = blockIdx.y, lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int HW = a.H[l] * a.W[l], C = a.C;
  const int p = ((int)blockIdx.x - a.wg_begin[l]) * kWave + lane;
  const bool live = p < HW;
  const float* sc = a.cls[l] + (long)img * C * HW + p;
  float best = -INFINITY;
  for (int c0 = wave; c0 < C; c0 += kRdWaves * kRdUnroll) {
    float v[kRdUnroll];
#pragma unroll
    for (int u = 0; u < kRdUnroll; ++u) {
      const int c = c0 + u * kRdWaves;
      v[u] = live && c < C ? sc[(long)c * HW] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < kRdUnroll; ++u) {
      const int c = c0 + u * kRdWaves;
      if (c < C) best = fmaxr(best, a.logits ? sigmoid_f32(v[u]) : v[u]);
    }
  }
  sm[wave][lane] = best;
  __syncthreads();
  if (wave == 0 && live)
    a.m[(long)img * a.P + a.m_begin[l] + p] = fmaxr(fmaxr(sm[0][lane], sm[1][lane]), fmaxr(sm[2][lane], sm[3][lane]));
}

// The stable top-`pre` of `count` <= kRdSelT * kRdRegKeys scores by one workgroup of kRdSelT threads, the keys held
// in REGISTERS: thread t owns the U = ceil(count / kRdSelT) consecutive rows from t * U, so thread order is row
// order.  Four 8-bit radix passes find the pre-th best key (one LDS add per key into a histogram kept in kRdRep
// copies, the copy chosen by the lane, so that the lanes of a wave that share a digit -- sigmoid maxima share a few
// exponents -- spread over banks); the ties at that key are ranked by a workgroup prefix sum, the lowest rows win;
// the selected rows are appended unordered as composite (key, row) words and sorted in LDS.  Same result as
// select_sort_topk (select_common.h), whose per-key ballot rounds cost this single workgroup ~50 us on the 16,700
// keys of the config's first level; this form takes a fifth of it.  keys[0 .. pre) end up in descending score order.
__device__ __forceinline__ void rd_select_regs(const float* __restrict__ sc, int count, int pre, int P2,
                                               unsigned long long* keys, int* hist, int* sum, int* sh, int* ncand) {
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int U = (count + kRdSelT - 1) / kRdSelT, i0 = tid * U;
  unsigned k[kRdRegKeys];
#pragma unroll
  for (int u = 0; u < kRdRegKeys; ++u) k[u] = u < U && i0 + u < count ? ordered_desc_bits(sc[i0 + u]) : 0xffffffffu;
  unsigned prefix = 0, mask = 0;
  int want = pre, n_eq = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int j = tid; j < 256 * kRdRep; j += kRdSelT) hist[j] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kRdRegKeys; ++u)
      if (u < U && i0 + u < count && (k[u] & mask) == prefix)
        atomicAdd(&hist[((k[u] >> shift) & 255u) * kRdRep + (lane & (kRdRep - 1))], 1);
    __syncthreads();
    if (tid < 256) {
      int s = 0;
#pragma unroll
      for (int r = 0; r < kRdRep; ++r) s += hist[tid * kRdRep + r];
      sum[tid] = s;
    }
    __syncthreads();
    if (wave == 0)  // the digit where the running count reaches `want`: exactly one lane finds it
      rank_pick256(lane, sum, want, sh, [](int, int tot) { return wave_scan_i32(tot); });
    __syncthreads();
    want -= sh[1];
    n_eq = sh[2];
    prefix |= (unsigned)sh[0] << shift;
    mask |= 255u << shift;
  }
  const unsigned Tkey = prefix;  // `want` of the n_eq rows with this key are still needed: the lowest rows
  int tie = 0;                   // rank of this thread's first tied row among all tied rows, in row order
  if (want < n_eq) {             // uniform
    int nt = 0;
#pragma unroll
    for (int u = 0; u < kRdRegKeys; ++u) nt += u < U && i0 + u < count && k[u] == Tkey;
    const int incl = wave_scan_i32(nt);
    if (lane == kWave - 1) sum[wave] = incl;
    __syncthreads();
    for (int w = 0; w < wave; ++w) tie += sum[w];
    tie += incl - nt;
  }
  if (tid == 0) *ncand = 0;
  for (int i = tid; i < P2; i += kRdSelT) keys[i] = ~0ull;
  __syncthreads();
#pragma unroll
  for (int u = 0; u < kRdRegKeys; ++u) {
    if (u < U) {  // uniform: every lane of a wave appends together
      bool take = false;
      if (i0 + u < count) {
        if (k[u] < Tkey) take = true;
        else if (k[u] == Tkey) take = tie++ < want;
      }
      const int pos = wave_append(take, ncand);
      if (take && pos < P2) keys[pos] = ((unsigned long long)k[u] << 32) | (unsigned)(i0 + u);
    }
  }
  __syncthreads();
  bitonic_sort_lds(keys, P2, tid, kRdSelT);
}

// step 2, grid (L, N)
__global__ __launch_bounds__(kRdSelT) void rd_select_kernel(RdArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  __shared__ __attribute__((aligned(16))) int hist[256 * kRdRep];
  __shared__ __attribute__((aligned(16))) int sum[256];
  __shared__ int sh[4], ncand;
  const int l = blockIdx.x, img = blockIdx.y;
  const int HW = a.H[l] * a.W[l], K = a.K[l];
  const float* m = a.m + (long)img * a.P + a.m_begin[l];
  if (HW <= kRdSelT * kRdRegKeys)
    rd_select_regs(m, HW, K, sort_size(K, 64), keys, hist, sum, sh, &ncand);
  else  // a level too large for the registers: the shared select, its keys re-read per pass
    select_sort_topk<1>(m, HW, K, sort_size(K, 64), keys, hist, &ncand);
  __syncthreads();
  int* sel = a.sel + (long)img * a.R + a.row_begin[l];
  for (int j = threadIdx.x; j < K; j += blockDim.x) sel[j] = (int)(unsigned)(keys[j] & 0xffffffffu);
}

// step 3, grid (chunks of kRdRows rows, N)
__global__ __launch_bounds__(kRdT) void rd_gather_kernel(RdArgs a) {
  __shared__ int sp[kRdRows], sl[kRdRows];
  const int img = blockIdx.y, tid = threadIdx.x;
  const int r0 = blockIdx.x * kRdRows, nr = iminr(kRdRows, a.R - r0);
  if (tid < nr) {
    const int row = r0 + tid;
    int l = 0;
    while (l + 1 < a.L && row >= a.row_begin[l + 1]) ++l;
    const int W = a.W[l], HW = a.H[l] * W;
    int p = a.sel[(long)img * a.R + row];
    if ((unsigned)p >= (unsigned)HW) p = HW - 1;   // never taken: the sorted words are real locations
    sp[tid] = p;
    sl[tid] = l;
    const int y = p / W, x = p - y * W;
    const float* base = a.pts[l] + (long)img * 2 * a.num_points * HW + p;   // channels (y0, x0, y1, x1, ...)
    float e0 = 0.f, e1 = 0.f;
    if (a.transform == kRpMoment) { e0 = expf(a.mt[0]); e1 = expf(a.mt[1]); }
    float box[4];
    rp_points2bbox_n(base + HW, base, 2L * HW, a.num_points, a.transform, e0, e1, box);
    const float fs = (float)a.stride[l], px = (float)x * fs, py = (float)y * fs;
    const float lim_x = a.im_info[img * 3 + 1] - 1.0f, lim_y = a.im_info[img * 3 + 0] - 1.0f;
    float* ob = a.bbox + ((long)img * a.R + row) * 4;
    ob[0] = fmaxr(fminr(box[0] * fs + px, lim_x), 0.0f);
    ob[1] = fmaxr(fminr(box[1] * fs + py, lim_y), 0.0f);
    ob[2] = fmaxr(fminr(box[2] * fs + px, lim_x), 0.0f);
    ob[3] = fmaxr(fminr(box[3] * fs + py, lim_y), 0.0f);
  }
  __syncthreads();
  const int C1 = a.C + 1, total = nr * C1;
  float* os = a.cls_score + ((long)img * a.R + r0) * C1;
  for (int e = tid; e < total; e += kRdT) {
    const int j = e / C1, q = e - j * C1;
    float v = 0.0f;
    if (q > 0) {
      const int l = sl[j], HW = a.H[l] * a.W[l];
      v = a.cls[l][((long)img * a.C + (q - 1)) * HW + sp[j]];
      if (a.logits) v = sigmoid_f32(v);
    }
    os[e] = v;
  }
}

struct RdWs {
  float* m;
  int* sel;
};

// bytes of the workspace in use; the size query passes a null workspace and gets null pointers
size_t rd_layout(int N, long P, long R, RdWs* ws, void* workspace) {
  WsCarver c(workspace);
  ws->m = c.take<float>((size_t)N * P * sizeof(float));
  ws->sel = c.take<int>((size_t)N * R * sizeof(int));
  return c.need();
}

// the argument checks the workspace query and the call share; Kl[l] = rows kept of level l, *P = sum H_l*W_l,
// *R = sum K_l
int rd_dims(int N, int C, int L, const long* hw, const int* k, int* Kl, long* P, long* R) {
  SD_REQUIRE(L >= 1 && L <= kRdMaxL, "reppoints_decode: L=%d levels, expected 1..%d", L, kRdMaxL);
  SD_REQUIRE(N >= 0 && C >= 1, "reppoints_decode: bad dimensions (N=%d C=%d)", N, C);
  SD_REQUIRE(hw && k, "reppoints_decode: null level table");
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(hw[l] >= 1, "reppoints_decode: level %d has H*W = %ld", l, hw[l]);
    SD_REQUIRE(k[l] <= hw[l], "reppoints_decode: level %d keeps k = %d of %ld locations", l, k[l], hw[l]);
  }
  if (N > kRdMaxImages)
    return fail(SD_ERR_UNSUPPORTED, "reppoints_decode: N=%d images exceed the limit %d", N, kRdMaxImages);
  long p = 0, r = 0;
  for (int l = 0; l < L; ++l) {
    if (hw[l] > kRdMaxHW)
      return fail(SD_ERR_UNSUPPORTED, "reppoints_decode: level %d has H*W = %ld locations, more than 2^24", l, hw[l]);
    const long kl = k[l] > 0 ? k[l] : hw[l];
    if (kl > kRdCap)
      return fail(SD_ERR_UNSUPPORTED, "reppoints_decode: level %d keeps %ld rows, more than %d", l, kl, kRdCap);
    if ((long)N * C * hw[l] > kRdMaxElems)
      return fail(SD_ERR_UNSUPPORTED, "reppoints_decode: level %d holds N*C*H*W = %ld scores, more than 2^31 - 1", l,
                  (long)N * C * hw[l]);
    Kl[l] = (int)kl;
    p += hw[l];
    r += kl;
  }
  if ((long)N * r * (C + 1L) > kRdMaxElems)
    return fail(SD_ERR_UNSUPPORTED, "reppoints_decode: cls_score holds N*R*(C+1) = %ld elements, more than 2^31 - 1",
                (long)N * r * (C + 1L));
  *P = p;
  *R = r;
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_reppoints_decode_workspace_bytes(int N, int C, int L, const long* hw_host, const int* k_host) {
  int Kl[kRdMaxL];
  long P = 0, R = 0;
  if (rd_dims(N, C, L, hw_host, k_host, Kl, &P, &R) != SD_OK || N == 0) return 256;
  RdWs ws;
  return rd_layout(N, P, R, &ws, nullptr) + 256;
}

extern "C" int sd_reppoints_decode(const float* const* cls, const float* const* pts, const float* im_info,
                                   const float* moment_transfer, const int* H_host, const int* W_host,
                                   const int* stride_host, const int* k_host, int L, int N, int C, int num_points,
                                   int transform, int input_logits, float* cls_score, float* bbox_xyxy,
                                   void* workspace, size_t workspace_bytes, void* stream) {
  SD_REQUIRE(L >= 1 && L <= kRdMaxL, "reppoints_decode: L=%d levels, expected 1..%d", L, kRdMaxL);
  SD_REQUIRE(H_host && W_host && stride_host && k_host, "reppoints_decode: null level table");
  long hw[kRdMaxL];
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(H_host[l] >= 1 && W_host[l] >= 1, "reppoints_decode: level %d is %d x %d", l, H_host[l], W_host[l]);
    SD_REQUIRE(stride_host[l] >= 1, "reppoints_decode: stride %d of level %d is not positive", stride_host[l], l);
    hw[l] = (long)H_host[l] * W_host[l];
  }
  SD_REQUIRE(num_points >= 1, "reppoints_decode: num_points=%d must be >= 1", num_points);
  SD_REQUIRE(transform >= kRpMinmax && transform <= kRpMoment,
             "reppoints_decode: transform=%d is none of minmax (0), partial_minmax (1), moment (2)", transform);
  SD_REQUIRE(transform != kRpPartial || num_points >= 4,
             "reppoints_decode: partial_minmax takes the first four points, num_points=%d", num_points);
  SD_REQUIRE(transform != kRpMoment || moment_transfer,
             "reppoints_decode: null pointer: the moment transform needs moment_transfer");
  SD_REQUIRE(input_logits == 0 || input_logits == 1, "reppoints_decode: input_logits=%d, expected 0 or 1", input_logits);
  int Kl[kRdMaxL];
  long P = 0, R = 0;
  if (int e = rd_dims(N, C, L, hw, k_host, Kl, &P, &R)) return e;
  if (N == 0) return SD_OK;  // every output is empty
  SD_REQUIRE(cls && pts, "reppoints_decode: null level table");
  for (int l = 0; l < L; ++l) SD_REQUIRE(cls[l] && pts[l], "reppoints_decode: null pointer in level %d", l);
  SD_REQUIRE(im_info && cls_score && bbox_xyxy, "reppoints_decode: null tensor pointer");
  if (!workspace) return fail(SD_ERR_WORKSPACE, "reppoints_decode: null workspace");
  SD_REQUIRE(((uintptr_t)workspace & 15) == 0, "reppoints_decode: workspace must be 16-byte aligned");
  RdWs ws;
  const size_t need = rd_layout(N, P, R, &ws, workspace);
  if (workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "reppoints_decode workspace too small: %zu < %zu bytes", workspace_bytes, need);
  RdArgs a{};
  a.im_info = im_info;
  a.mt = moment_transfer;
  a.L = L; a.N = N; a.C = C; a.num_points = num_points; a.transform = transform; a.logits = input_logits;
  a.R = (int)R; a.P = P;
  a.cls_score = cls_score; a.bbox = bbox_xyxy; a.m = ws.m; a.sel = ws.sel;
  int max_keys = 0;
  a.row_begin[0] = 0;
  a.wg_begin[0] = 0;
  long pb = 0;
  for (int l = 0; l < L; ++l) {
    a.cls[l] = cls[l]; a.pts[l] = pts[l];
    a.H[l] = H_host[l]; a.W[l] = W_host[l]; a.stride[l] = stride_host[l]; a.K[l] = Kl[l];
    a.m_begin[l] = (int)pb;
    pb += hw[l];
    a.row_begin[l + 1] = a.row_begin[l] + Kl[l];
    a.wg_begin[l + 1] = a.wg_begin[l] + cdiv(hw[l], kWave);
    if (Kl[l] > max_keys) max_keys = Kl[l];
  }
  const size_t lds = (size_t)sort_size(max_keys, 64) * sizeof(unsigned long long);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(rd_max_kernel, dim3(a.wg_begin[L], N), dim3(kRdT), 0, st, a);
  SD_LAUNCH_CHECK();
  // the attribute is one constant (the sort's capacity), never this call's size: host threads that decode different
  // shapes at the same time cannot lower it for each other
  constexpr int kMaxLds = kRdCap * (int)sizeof(unsigned long long);
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)rd_select_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
  hipLaunchKernelGGL(rd_select_kernel, dim3(L, N), dim3(kRdSelT), lds, st, a);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(rd_gather_kernel, dim3(cdiv(R, kRdRows), N), dim3(kRdT), 0, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
