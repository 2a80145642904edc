// FCOS test-time decode for gfx950, fp32: per-level top-k, boxes and the batch sort in ONE call.
//
// The reference (the spec, quirks included) is FCOSFPNHead.get_all_proposal (models/FCOS/builder.py:234-259): ten
// sigmoid nodes, five Python CustomOps get_proposal_single_stage (models/FCOS/utils.py:7-94), a concat and the
// Python CustomOp get_batch_proposal (utils.py:99-149).  Per level and image:
//   utils.py:17-19  cand = cls > thresh, a float32 compare (equality is NOT a candidate); fused = cls * ctr, a
//                   float32 product with ctr broadcast over the channels.
//   utils.py:32-36  DENSE branch when count(cand) >= top_n: the top_n best of ALL C*H*W fused scores -- not only
//                   of the candidates -- in descending order; flat index idx = (c*H + y)*W + x, cls = c + 1.  The
//                   reference derives x, y, c from a float32 idx by float divisions; integer arithmetic gives the
//                   same for C*H*W <= 2^24 (the fixture script checks every idx of its shapes), beyond that the
//                   float32 idx is not exact and the call is SD_ERR_UNSUPPORTED.
//   utils.py:38-46  SPARSE branch when 0 < count < top_n: the candidates in ascending flat index order (np.nonzero)
//                   with their fused scores; count == 0 leaves the level's rows at -1 (:40-41).
//   utils.py:49-55  cx = x*stride + stride/2, cy likewise (float32); x1 = clip(cx - off[0,y,x], 0, img_w),
//                   y1 = clip(cy - off[1], 0, img_h), x2 = clip(cx + off[2], 0, img_w), y2 = clip(cy + off[3], 0,
//                   img_h) with img_h, img_w = im_info[i, 0:2]; row = [cls, fused, x1, y1, x2, y2].
//   utils.py:61-64  "remove small bboxes" is computed on the 6-column row, so the mask is
//                   (cls >= x1) && (fused >= y1): such a row becomes six -1, any other row keeps its values.
//   utils.py:66     rows past the selected ones stay -1 (builder.py:255 concatenates the levels: `stage_out`).
//   utils.py:110-124 per image the R = L*top_n rows are put in descending order of column 1; bbox = columns 2..5,
//                   cls_id = column 0, score (N, R, 81) is zero except score[i, r, int(cls_r)] =
//                   sqrt(clip(fused_r, 1e-20, 1)) for EVERY row: a padding or masked row has cls = -1, which numpy
//                   reads as the LAST column, so column 80 of such rows holds sqrt(float32(1e-20)).  Column 0 is
//                   never written by a real row.  81 is the reference's constant: C > 80 is SD_ERR_UNSUPPORTED.
// Ties are the project's choice (MXNet's topk / argsort order among equal keys is not documented): equal fused
// scores inside a level -> the lower flat index first; in the batch sort -> stable in concat order (the lower
// level, then the lower row, first); -0.0 and +0.0 compare equal (select_common.h).
// NaN (not pinned by the spec; what this code does): a NaN cls is no candidate; a NaN fused score is ordered by its
// bits (positive NaN before +inf, negative NaN after -inf) in the level top-k and in the batch sort alike; NaN
// offsets give NaN coordinates (the clip passes NaN on) and a comparison with NaN never masks a row; inf offsets
// clip.  clip(v, 0, hi) is min(max(v, 0), hi), numpy's order, which matters only for a negative image size.
//
// MI355X design (all launches on the caller's stream, nothing read back by the host, no device allocation, no float
// atomics -- integer atomics only, for counts, histograms and list appends whose order the sorts restore):
//   1. zero_counters             clears the per-(image, level) counters (runtime.hip: a kernel, not a memset node).
//   2. fcos_decode_scan_kernel   grid over (level chunk, image): streams cls once, counts the candidates, appends
//                                their flat indices to the level's sparse list while it has room (top_n words),
//                                and builds a 4096-bin histogram of the top 12 bits of ordered_desc_bits(fused).
//   3. fcos_decode_collect_kernel same grid: leaves at once unless the level is dense; resolves the cut-off bin of
//                                the top_n-th best score from the histogram and re-streams cls, appending the
//                                (key, idx) words of the bins up to the cut-off (<= 16384 of them).  When those
//                                bins hold more (heavily tied scores on a large level) it writes every fused score
//                                to the workspace instead and step 4 runs the shared single-workgroup radix select.
//   4. fcos_decode_level_kernel  one workgroup per (level, image): LDS bitonic sort of the collected words (dense: by
//                                (key, idx); sparse: by idx), decode of the first top_n rows, the mask quirk, the
//                                six-column rows written to stage_out (or to the workspace when it is NULL).
//   5. fcos_decode_batch_kernel  one workgroup per image: LDS bitonic sort of (key(column 1), concat row) -- a masked
//                                row already holds score -1 here, as in the reference -- then bbox, cls_id and the
//                                per-row (column, sqrt) pair.
//   6. fcos_decode_score_kernel  fills score (N, R, 81) from those pairs with coalesced stores.
// Every element of bbox, score, cls_id and stage_out is written by every call.  Loads are scalar, so any 4-byte
// aligned pointer gives the same bits.  Arithmetic: -ffp-contract=off, correctly rounded divide and sqrt (Makefile).
#include "loss_common.h"
#include "select_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {
namespace {

constexpr int kDcMaxL = SD_MAX_FPN_LEVELS;
constexpr int kDcT = 256;
constexpr int kDcUnroll = 16;                  // scalar loads in flight per lane
constexpr int kDcTrip = kDcT * kDcUnroll;      // elements per workgroup trip
constexpr int kDcMaxChunks = 512;              // workgroups per (level, image)
constexpr int kDcBins = 4096;                  // top 12 bits of the key: sign, exponent, 3 mantissa bits
constexpr int kDcBinShift = 20;
constexpr int kDcCap = kMaxSortKeys;           // words the LDS sorts hold
constexpr int kDcCtr = 4;                      // ints per (image, level): [0] candidates, [1] collected words
constexpr int kDcScoreCols = 81;               // utils.py:108
constexpr long kDcMaxCount = 1L << 24;         // a float32 idx is exact up to here (utils.py:34-36)
constexpr int kDcMaxImages = 65535;            // gridDim.y

struct DecodeArgs {
  const float* cls[kDcMaxL];
  const float* ctr[kDcMaxL];
  const float* off[kDcMaxL];
  int H[kDcMaxL], W[kDcMaxL], stride[kDcMaxL], count[kDcMaxL], chunk[kDcMaxL], wg_begin[kDcMaxL + 1];
  long eff_begin[kDcMaxL], eff_img;
  const float* im_info;
  int L, N, C, top_n, R, logits;
  float thresh;
  float* bbox;
  float* score;
  float* cls_id;
  float* stage;              // (N, R, 6): stage_out or the workspace
  int* hist;                 // (N, L, kDcBins)
  int* gctr;                 // (N, L, kDcCtr)
  unsigned* sparse;          // (N, L, top_n) flat indices of candidates
  unsigned long long* cand;  // (N, L, kDcCap) (key, idx) words
  float* eff;                // (N, sum count) fused scores (tied-bin path)
  float* val;                // (N, R) sqrt(clip(fused)) of the sorted rows
};

// cls and fused score of flat element e (hw = e % HW) whose raw class value is `craw`
__device__ __forceinline__ void dc_scores(const DecodeArgs& a, const float* __restrict__ ct, int hw, float craw,
                                          float* cls, float* fused) {
  float t = ct[hw];
  if (a.logits) {
    craw = sigmoid_f32(craw);
    t = sigmoid_f32(t);
  }
  *cls = craw;
  *fused = craw * t;
}

__device__ __forceinline__ int dc_level(const DecodeArgs& a, int wg) {
  int l = 0;
  while (l + 1 < a.L && wg >= a.wg_begin[l + 1]) ++l;
  return l;
}

__device__ __forceinline__ float dc_clip(float v, float hi) {  // np.clip(v, 0, hi): NaN passes
  v = v < 0.0f ? 0.0f : v;
  return v > hi ? hi : v;
}

// step 2, grid (sum of the levels' chunks, N)
__global__ __launch_bounds__(kDcT) void fcos_decode_scan_kernel(DecodeArgs a) {
  __shared__ int lh[kDcBins];
  __shared__ unsigned ll[kDcTrip];
  __shared__ int nl, base;
  const int l = dc_level(a, blockIdx.x), img = blockIdx.y, tid = threadIdx.x;
  const int count = a.count[l], HW = a.H[l] * a.W[l], hw_step = kDcT % HW;
  const int lo = ((int)blockIdx.x - a.wg_begin[l]) * a.chunk[l];
  const int hi = (long)lo + a.chunk[l] < count ? lo + a.chunk[l] : count;
  const float* sc = a.cls[l] + (long)img * count;
  const float* ct = a.ctr[l] + (long)img * HW;
  const long il = (long)img * a.L + l;
  int* gc = a.gctr + il * kDcCtr;
  unsigned* sp = a.sparse + il * a.top_n;
  for (int i = tid; i < kDcBins; i += kDcT) lh[i] = 0;
  if (tid == 0) nl = 0;
  __syncthreads();
  for (int t0 = lo; t0 < hi; t0 += kDcTrip) {
    float v[kDcUnroll];
#pragma unroll
    for (int u = 0; u < kDcUnroll; ++u) {
      const int e = t0 + u * kDcT + tid;
      v[u] = e < hi ? sc[e] : 0.0f;
    }
    int hw = (t0 + tid) % HW;  // a lane's elements step by kDcT: one modulo per trip, then carried
#pragma unroll
    for (int u = 0; u < kDcUnroll; ++u) {
      const int e = t0 + u * kDcT + tid;
      bool is_cand = false;
      if (e < hi) {
        float c, f;
        dc_scores(a, ct, hw, v[u], &c, &f);
        is_cand = c > a.thresh;
        atomicAdd(&lh[ordered_desc_bits(f) >> kDcBinShift], 1);
      }
      hw += hw_step;
      if (hw >= HW) hw -= HW;
      const int pos = wave_append(is_cand, &nl);  // < kDcTrip: the list is flushed every trip
      if (is_cand) ll[pos] = (unsigned)e;
    }
    __syncthreads();
    const int n = nl;
    if (n > 0) wg_list_flush<kDcT>(ll, n, &nl, &base, &gc[0], sp, a.top_n);
    __syncthreads();
  }
  int* gh = a.hist + il * kDcBins;
  for (int i = tid; i < kDcBins; i += kDcT)
    if (lh[i]) atomicAdd(&gh[i], lh[i]);
}

// step 3, same grid
__global__ __launch_bounds__(kDcT) void fcos_decode_collect_kernel(DecodeArgs a) {
  __shared__ unsigned long long lc[kDcTrip];
  __shared__ int sh[4], nl, base;
  const int l = dc_level(a, blockIdx.x), img = blockIdx.y, tid = threadIdx.x;
  const long il = (long)img * a.L + l;
  int* gc = a.gctr + il * kDcCtr;
  if (gc[0] < a.top_n) return;  // sparse or empty level: step 2 left everything step 4 needs
  int bstar, below, nb;
  hist_cut_bin<kDcBins>(a.hist + il * kDcBins, a.top_n, sh, &bstar, &below, &nb);
  const int count = a.count[l], HW = a.H[l] * a.W[l], hw_step = kDcT % HW;
  const int lo = ((int)blockIdx.x - a.wg_begin[l]) * a.chunk[l];
  const int hi = (long)lo + a.chunk[l] < count ? lo + a.chunk[l] : count;
  const float* sc = a.cls[l] + (long)img * count;
  const float* ct = a.ctr[l] + (long)img * HW;
  const bool tied = below + nb > kDcCap;
  float* eff = a.eff + (long)img * a.eff_img + a.eff_begin[l];
  unsigned long long* cand = a.cand + il * kDcCap;
  if (tid == 0) nl = 0;
  __syncthreads();
  for (int t0 = lo; t0 < hi; t0 += kDcTrip) {
    float v[kDcUnroll];
#pragma unroll
    for (int u = 0; u < kDcUnroll; ++u) {
      const int e = t0 + u * kDcT + tid;
      v[u] = e < hi ? sc[e] : 0.0f;
    }
    int hw = (t0 + tid) % HW;
#pragma unroll
    for (int u = 0; u < kDcUnroll; ++u) {
      const int e = t0 + u * kDcT + tid;
      bool take = false;
      unsigned key = 0;
      if (e < hi) {
        float c, f;
        dc_scores(a, ct, hw, v[u], &c, &f);
        if (tied) {
          eff[e] = f;
        } else {
          key = ordered_desc_bits(f);
          take = (int)(key >> kDcBinShift) <= bstar;
        }
      }
      hw += hw_step;
      if (hw >= HW) hw -= HW;
      const int pos = wave_append(take, &nl);
      if (take) lc[pos] = ((unsigned long long)key << 32) | (unsigned)e;
    }
    __syncthreads();
    const int n = nl;
    if (n > 0) wg_list_flush<kDcT>(lc, n, &nl, &base, &gc[1], cand, kDcCap);
    __syncthreads();
  }
}

// step 4, grid (L, N)
__global__ __launch_bounds__(1024) void fcos_decode_level_kernel(DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  __shared__ int hist[260];
  __shared__ int sh[4], ncand;
  const int l = blockIdx.x, img = blockIdx.y, tid = threadIdx.x, T = blockDim.x;
  const long il = (long)img * a.L + l;
  const int* gc = a.gctr + il * kDcCtr;
  const int count = a.count[l], H = a.H[l], W = a.W[l], HW = H * W;
  const int nc = gc[0];
  int nsel = 0;
  if (nc >= a.top_n) {  // dense (utils.py:32-36)
    int bstar, below, nb;
    hist_cut_bin<kDcBins>(a.hist + il * kDcBins, a.top_n, sh, &bstar, &below, &nb);
    if (below + nb > kDcCap) {
      select_sort_topk<1>(a.eff + (long)img * a.eff_img + a.eff_begin[l], count, a.top_n, sort_size(a.top_n, 64),
                          keys, hist, &ncand);
    } else {
      const int n = iminr(gc[1], kDcCap);  // == below + nb >= top_n
      const int P2 = sort_size(n, 64);
      const unsigned long long* cand = a.cand + il * kDcCap;
      for (int i = tid; i < P2; i += T) keys[i] = i < n ? cand[i] : ~0ull;
      __syncthreads();
      bitonic_sort_lds(keys, P2, tid, T);
    }
    nsel = a.top_n;
  } else if (nc > 0) {  // sparse (utils.py:38-46): ascending flat index
    const int P2 = sort_size(nc, 64);
    const unsigned* sp = a.sparse + il * a.top_n;
    for (int i = tid; i < P2; i += T) keys[i] = i < nc ? (unsigned long long)sp[i] : ~0ull;
    __syncthreads();
    bitonic_sort_lds(keys, P2, tid, T);
    nsel = nc;
  }
  __syncthreads();
  const float* sc = a.cls[l] + (long)img * count;
  const float* ct = a.ctr[l] + (long)img * HW;
  const float* of = a.off[l] + (long)img * 4 * HW;
  const float img_h = a.im_info[img * 3 + 0], img_w = a.im_info[img * 3 + 1];
  const float fs = (float)a.stride[l], half = (float)(0.5 * (double)a.stride[l]);
  float* st = a.stage + ((long)img * a.R + (long)l * a.top_n) * 6;
  for (int j = tid; j < a.top_n; j += T) {
    float r0 = -1.0f, r1 = -1.0f, r2 = -1.0f, r3 = -1.0f, r4 = -1.0f, r5 = -1.0f;
    const int idx = j < nsel ? (int)(unsigned)(keys[j] & 0xffffffffu) : count;
    if (idx < count) {  // always true for j < nsel: the sorted words are real rows
      const int c = idx / HW, hw = idx - c * HW, y = hw / W, x = hw - y * W;
      float cv, f;
      dc_scores(a, ct, hw, sc[idx], &cv, &f);
      const float cx = (float)x * fs + half, cy = (float)y * fs + half;
      const float x1 = dc_clip(cx - of[hw], img_w), y1 = dc_clip(cy - of[HW + hw], img_h);
      const float x2 = dc_clip(cx + of[2 * HW + hw], img_w), y2 = dc_clip(cy + of[3 * HW + hw], img_h);
      const float cf = (float)(c + 1);
      if (!(cf >= x1 && f >= y1)) {  // utils.py:61-64
        r0 = cf; r1 = f; r2 = x1; r3 = y1; r4 = x2; r5 = y2;
      }
    }
    float* o = st + (long)j * 6;
    o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3; o[4] = r4; o[5] = r5;
  }
}

// step 5, grid (N)
__global__ __launch_bounds__(1024) void fcos_decode_batch_kernel(DecodeArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];
  const int img = blockIdx.x, tid = threadIdx.x, T = blockDim.x, R = a.R;
  const float* st = a.stage + (long)img * R * 6;
  const int P2 = sort_size(R, 64);
  for (int r = tid; r < P2; r += T)
    keys[r] = r < R ? ((unsigned long long)ordered_desc_bits(st[(long)r * 6 + 1]) << 32) | (unsigned)r : ~0ull;
  __syncthreads();
  bitonic_sort_lds(keys, P2, tid, T);
  float* ob = a.bbox + (long)img * R * 4;
  float* oc = a.cls_id + (long)img * R;
  float* ov = a.val + (long)img * R;
  for (int j = tid; j < R; j += T) {
    const float* row = st + (long)(unsigned)(keys[j] & 0xffffffffu) * 6;
    const float cf = row[0], f = row[1];
    ob[(long)j * 4 + 0] = row[2];
    ob[(long)j * 4 + 1] = row[3];
    ob[(long)j * 4 + 2] = row[4];
    ob[(long)j * 4 + 3] = row[5];
    oc[j] = cf;
    const float cl = f < 1e-20f ? 1e-20f : f > 1.0f ? 1.0f : f;  // np.clip: NaN passes
    ov[j] = sqrtf(cl);
  }
}

// step 6, grid (chunks of R*81, N): score[i, r, int(cls_r)] = val_r, every other element zero; cls = -1 indexes
// the last column (utils.py:119)
__global__ __launch_bounds__(256) void fcos_decode_score_kernel(DecodeArgs a) {
  const int img = blockIdx.y, total = a.R * kDcScoreCols;
  const float* oc = a.cls_id + (long)img * a.R;
  const float* ov = a.val + (long)img * a.R;
  float* os = a.score + (long)img * total;
  for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
    const int r = e / kDcScoreCols, q = e - r * kDcScoreCols;
    int col = (int)oc[r];
    if (col < 0) col += kDcScoreCols;
    os[e] = q == col ? ov[r] : 0.0f;
  }
}

__global__ __launch_bounds__(256) void fcos_sigmoid_kernel(const float* __restrict__ x, float* __restrict__ p, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    p[i] = sigmoid_f32(x[i]);
}

struct DecodeWs {
  int* hist;
  int* gctr;
  unsigned* sparse;
  unsigned long long* cand;
  float* eff;
  float* stage;
  float* val;
};

// bytes of the workspace in use; the size query passes a null workspace and gets null pointers
size_t decode_layout(int N, int L, long total, int top_n, DecodeWs* ws, void* workspace) {
  WsCarver c(workspace);
  const size_t NL = (size_t)N * L, R = (size_t)L * top_n;
  ws->hist = c.take<int>(NL * (kDcBins + kDcCtr) * sizeof(int));
  ws->gctr = ws->hist ? ws->hist + NL * kDcBins : nullptr;
  ws->sparse = c.take<unsigned>(NL * top_n * sizeof(unsigned));
  ws->cand = c.take<unsigned long long>(NL * kDcCap * sizeof(unsigned long long));
  ws->eff = c.take<float>((size_t)N * total * sizeof(float));
  ws->stage = c.take<float>((size_t)N * R * 6 * sizeof(float));
  ws->val = c.take<float>((size_t)N * R * sizeof(float));
  return c.need();
}

// the argument checks the workspace query and the call share; *total = sum of C*H_l*W_l
int decode_dims(int N, int C, int L, const long* hw, int top_n, long* total) {
  SD_REQUIRE(N >= 0 && C >= 1, "fcos_decode: bad dimensions (N=%d C=%d)", N, C);
  SD_REQUIRE(L >= 1 && L <= kDcMaxL, "fcos_decode: L=%d levels, expected 1..%d", L, kDcMaxL);
  SD_REQUIRE(top_n >= 1, "fcos_decode: top_n=%d must be >= 1", top_n);
  SD_REQUIRE(hw, "fcos_decode: null level table");
  if (C > kDcScoreCols - 1)
    return fail(SD_ERR_UNSUPPORTED, "fcos_decode: C=%d classes exceed the score tensor's %d columns", C,
                kDcScoreCols - 1);
  if ((long)L * top_n > kDcCap)
    return fail(SD_ERR_UNSUPPORTED, "fcos_decode: R = L*top_n = %ld rows exceed the limit %d", (long)L * top_n,
                kDcCap);
  if (N > kDcMaxImages) return fail(SD_ERR_UNSUPPORTED, "fcos_decode: N=%d images exceed the limit %d", N, kDcMaxImages);
  long t = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(hw[l] >= 1, "fcos_decode: level %d has H*W = %ld", l, hw[l]);
    if ((long)C * hw[l] > kDcMaxCount)
      return fail(SD_ERR_UNSUPPORTED, "fcos_decode: level %d has C*H*W = %ld scores, more than 2^24", l, (long)C * hw[l]);
    t += (long)C * hw[l];
  }
  *total = t;
  return SD_OK;
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_fcos_decode_workspace_bytes(int N, int C, int L, const long* hw_host, int top_n) {
  long total = 0;
  if (decode_dims(N, C, L, hw_host, top_n, &total) != SD_OK || N == 0) return 256;
  DecodeWs ws;
  return decode_layout(N, L, total, top_n, &ws, nullptr) + 256;
}

extern "C" int sd_fcos_decode(const float* const* cls, const float* const* ctr, const float* const* off,
                              const float* im_info, const int* H_host, const int* W_host, const int* stride_host,
                              int L, int N, int C, int top_n, float pre_nms_thresh, int input_logits, float* bbox,
                              float* score, float* cls_id, float* stage_out, void* workspace, size_t workspace_bytes,
                              void* stream) {
  SD_REQUIRE(L >= 1 && L <= kDcMaxL, "fcos_decode: L=%d levels, expected 1..%d", L, kDcMaxL);
  SD_REQUIRE(H_host && W_host && stride_host, "fcos_decode: null level table");
  long hw[kDcMaxL];
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(H_host[l] >= 1 && W_host[l] >= 1, "fcos_decode: level %d is %d x %d", l, H_host[l], W_host[l]);
    SD_REQUIRE(stride_host[l] >= 1, "fcos_decode: stride %d of level %d is not positive", stride_host[l], l);
    hw[l] = (long)H_host[l] * W_host[l];
  }
  long total = 0;
  if (int e = decode_dims(N, C, L, hw, top_n, &total)) return e;
  SD_REQUIRE(!isnan(pre_nms_thresh), "fcos_decode: pre_nms_thresh is NaN");
  SD_REQUIRE(input_logits == 0 || input_logits == 1, "fcos_decode: input_logits=%d, expected 0 or 1", input_logits);
  if (N == 0) return SD_OK;  // every output is empty
  SD_REQUIRE(cls && ctr && off, "fcos_decode: null level table");
  for (int l = 0; l < L; ++l)
    SD_REQUIRE(cls[l] && ctr[l] && off[l], "fcos_decode: null pointer in level %d", l);
  SD_REQUIRE(im_info && bbox && score && cls_id, "fcos_decode: null tensor pointer");
  if (!workspace) return fail(SD_ERR_WORKSPACE, "fcos_decode: null workspace");
  SD_REQUIRE(((uintptr_t)workspace & 15) == 0, "fcos_decode: workspace must be 16-byte aligned");
  DecodeWs ws;
  const size_t need = decode_layout(N, L, total, top_n, &ws, workspace);
  if (workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "fcos_decode workspace too small: %zu < %zu bytes", workspace_bytes, need);
  DecodeArgs a{};
  a.im_info = im_info;
  a.L = L; a.N = N; a.C = C; a.top_n = top_n; a.R = L * top_n; a.logits = input_logits;
  a.thresh = pre_nms_thresh;
  a.bbox = bbox; a.score = score; a.cls_id = cls_id;
  a.stage = stage_out ? stage_out : ws.stage;
  a.hist = ws.hist; a.gctr = ws.gctr; a.sparse = ws.sparse; a.cand = ws.cand; a.eff = ws.eff; a.val = ws.val;
  a.eff_img = total;
  int max_keys = a.R > top_n ? a.R : top_n;
  long eb = 0;
  a.wg_begin[0] = 0;
  for (int l = 0; l < L; ++l) {
    const long count = (long)C * hw[l];
    a.cls[l] = cls[l]; a.ctr[l] = ctr[l]; a.off[l] = off[l];
    a.H[l] = H_host[l]; a.W[l] = W_host[l]; a.stride[l] = stride_host[l]; a.count[l] = (int)count;
    a.eff_begin[l] = eb;
    eb += count;
    // one kDcTrip-element trip or more per workgroup, at most kDcMaxChunks workgroups per (level, image)
    long G = (count + kDcTrip - 1) / kDcTrip;
    if (G > kDcMaxChunks) G = kDcMaxChunks;
    const long chunk = ((count + G - 1) / G + kDcTrip - 1) / kDcTrip * kDcTrip;
    a.chunk[l] = (int)chunk;
    a.wg_begin[l + 1] = a.wg_begin[l] + (int)((count + chunk - 1) / chunk);
    const int held = (int)(count < kDcCap ? count : kDcCap);
    if (held > max_keys) max_keys = held;
  }
  const size_t lds = (size_t)sort_size(max_keys, 64) * sizeof(unsigned long long);
  hipStream_t st = (hipStream_t)stream;
  zero_counters(ws.hist, (long)N * L * (kDcBins + kDcCtr), st);  // < 2^31 * 1.01 counters
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(fcos_decode_scan_kernel, dim3(a.wg_begin[L], N), dim3(kDcT), 0, st, a);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(fcos_decode_collect_kernel, dim3(a.wg_begin[L], N), dim3(kDcT), 0, st, a);
  SD_LAUNCH_CHECK();
  // the attribute is one constant (the sorts' capacity), never this call's size: host threads that decode different
  // shapes at the same time cannot lower it for each other
  constexpr int kMaxLds = kDcCap * (int)sizeof(unsigned long long);
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)fcos_decode_level_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
  hipLaunchKernelGGL(fcos_decode_level_kernel, dim3(L, N), dim3(1024), lds, st, a);
  SD_LAUNCH_CHECK();
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)fcos_decode_batch_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, kMaxLds));
  hipLaunchKernelGGL(fcos_decode_batch_kernel, dim3(N), dim3(1024), lds, st, a);
  SD_LAUNCH_CHECK();
  const int sblocks = cdiv((long)a.R * kDcScoreCols, 256 * 8);
  hipLaunchKernelGGL(fcos_decode_score_kernel, dim3(sblocks, N), dim3(256), 0, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_fcos_sigmoid(const float* x, float* p, long n, void* stream) {
  SD_REQUIRE(n >= 0, "fcos_sigmoid: n=%ld is negative", n);
  if (n == 0) return SD_OK;
  SD_REQUIRE(x && p, "fcos_sigmoid: null pointer");
  long blocks = (n + 255) / 256;
  if (blocks > kNumCU * 8) blocks = kNumCU * 8;
  hipLaunchKernelGGL(fcos_sigmoid_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, x, p, n);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
