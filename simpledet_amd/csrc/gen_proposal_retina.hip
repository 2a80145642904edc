// _contrib_GenProposalRetina for gfx950: RetinaNet per-level decode, threshold and stable top-k.
//   reference (the spec): operator_cxx/contrib/generate_proposal_retina.cu:66-94 (ProposalGridKernel:
//   row i = (h*W + w)*AK + c, c = anchor*K + class, anchor row (h*W + w)*A + c/K), :96-159
//   (BBoxPredKernel, +1 convention, delta*std + mean), :161-209 (IoUPredKernel), :211-233
//   (FilterBoxKernel: the whole row zeroed), :301-468 (Forward: im_info copied to the host, every
//   (anchor, class, y, x) score thrust::stable_sort'ed descending, the first pre rows kept,
//   PrepareOutput writes the score to column min(out_channel-1, class+1)).
//   The .cc file is a stale RPN-style copy and is NOT the spec.
// MI355X design (per image; all launches on the caller's stream, nothing read back by the host):
//   key(row) = ordered_desc_bits(filtered ? 0 : score); a row is "live" when its key is better than
//   the key of 0 (an unfiltered positive score).  With thresh >= 0 every unfiltered row is live and
//   every filtered row outputs zeros, so the output is the stable top-min(pre, live) of the live
//   rows followed by zero rows.
//   1. retina_scan_kernel     streams cls_prob once (float4 loads), decodes only the rows above the
//                             threshold (the min-size test needs the box), counts live keys in a
//                             4096-bin LDS histogram of their top 12 bits (flushed to global) and
//                             appends live (key, row) words to a candidate list while it has room.
//   2. retina_compact_kernel  exits at once when the pass-1 list holds every live row (sparse levels);
//                             otherwise resolves the cut-off bin from the histogram and re-streams
//                             cls_prob, appending the live rows of the bins up to the cut-off.
//   3. retina_finish_kernel   one workgroup: the <= 16384 candidates bitonic-sorted in LDS as composite
//                             (key, row) words (== a stable descending sort), the first pre rows
//                             re-decoded and written, zero rows after them.
//   General path (thresh < 0, where filtered rows at key 0 can rank above negative survivors, or a
//   cut-off bin holding more than 16384 live rows, e.g. heavily tied scores): the pass writes the
//   effective score (0 if filtered) of every row and the finishing workgroup runs the shared
//   single-workgroup radix select (select_common.h) over it.  Exact, but bound by one CU.
// Rounding follows the repo's convention (Proposal_v3 decode, nms.hip): no FMA contraction
// (-ffp-contract=off) and exp as (float)exp((double)d).
#include "select_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {
namespace {

constexpr int kCap = kMaxSortKeys;      // candidates the finishing LDS sort holds
constexpr int kBins = 4096;             // histogram of the top 12 bits of live keys (< 2^31)
constexpr int kBinShift = 19;
constexpr unsigned kKey0 = 0x7fffffffu; // ordered_desc_bits(0.0f)
constexpr int kScanT = 256;
constexpr int kUnroll = 4;              // float4 loads in flight per lane
constexpr int kTrip = kScanT * 4 * kUnroll;  // elements per workgroup trip
constexpr int kLocal1 = 2048;           // pass-1 per-workgroup list (flushed once at the end)
constexpr int kLocal2 = 6144;           // pass-2 per-workgroup list (flushed past kLocal2 - kTrip)
constexpr long kMaxRows = 1L << 28;     // rows (A*K*H*W) per image

struct RetinaArgs {
  const float* cls_prob;   // (B, AK, H, W)
  const float* bbox_pred;  // (B, 4A, H, W)
  const float* im_info;    // (B, 3)
  const float* anchors;    // (H*W*A, 4), or (B, H*W*A, 4) when batch_wise_anchor
  float* out;              // (B, top_n, 4)
  float* score;            // (B, top_n, oc)
  float mean[4], stdv[4];
  int AK, K, A, HW, count, pre, top_n, oc;
  long anchor_img;         // floats between two images' anchors
  float min_size, thresh;
  int iou_loss, vec, general, G, chunk;
  int* ghist;              // (B, kBins)
  int* gctr;               // (B, 4): live rows, pass-1 local overflow, pass-2 list length, unused
  unsigned long long* cand;  // (B, kCap)
  float* eff;              // (B, count) effective scores (general path)
};

// the box of row (c, hw) and whether it survives FilterBoxKernel; s is its score
__device__ __forceinline__ bool retina_row(const RetinaArgs& a, int img, int c, int hw, float s,
                                           float4* box) {
  if (!(s > a.thresh)) return false;  // score <= thresh; NaN scores count as filtered (DESIGN)
  const float im_h = a.im_info[img * 3 + 0], im_w = a.im_info[img * 3 + 1];
  const float min_size = a.min_size * a.im_info[img * 3 + 2];
  const int an = c / a.K;
  const float* ap = a.anchors + (long)img * a.anchor_img + ((long)hw * a.A + an) * 4;
  const float x1 = ap[0], y1 = ap[1], x2 = ap[2], y2 = ap[3];
  const float* dl = a.bbox_pred + ((long)img * 4 * a.A + 4 * an) * a.HW + hw;
  const float d0 = dl[0], d1 = dl[a.HW], d2 = dl[2L * a.HW], d3 = dl[3L * a.HW];
  float px1, py1, px2, py2;
  if (a.iou_loss) {  // IoUPredKernel (:161-209), K == 1 only
    px1 = x1 + d0;
    py1 = y1 + d1;
    px2 = x2 + d2;
    py2 = y2 + d3;
  } else {  // BBoxPredKernel (:96-159)
    const float width = x2 - x1 + 1.0f, height = y2 - y1 + 1.0f;
    const float ctr_x = x1 + 0.5f * (width - 1.0f), ctr_y = y1 + 0.5f * (height - 1.0f);
    const float dx = d0 * a.stdv[0] + a.mean[0];
    const float dy = d1 * a.stdv[1] + a.mean[1];
    const float dw = d2 * a.stdv[2] + a.mean[2];
    const float dh = d3 * a.stdv[3] + a.mean[3];
    const float pcx = dx * width + ctr_x, pcy = dy * height + ctr_y;
    const float pw = (float)exp((double)dw) * width, ph = (float)exp((double)dh) * height;
    px1 = pcx - 0.5f * (pw - 1.0f);
    py1 = pcy - 0.5f * (ph - 1.0f);
    px2 = pcx + 0.5f * (pw - 1.0f);
    py2 = pcy + 0.5f * (ph - 1.0f);
  }
  // max(min(v, im - 1), 0) of the CUDA source: fminf / fmaxf
  px1 = fmaxf(fminf(px1, im_w - 1.0f), 0.0f);
  py1 = fmaxf(fminf(py1, im_h - 1.0f), 0.0f);
  px2 = fmaxf(fminf(px2, im_w - 1.0f), 0.0f);
  py2 = fmaxf(fminf(py2, im_h - 1.0f), 0.0f);
  const float iw = px2 - px1 + 1.0f, ih = py2 - py1 + 1.0f;
  if (iw < min_size || ih < min_size) return false;
  *box = make_float4(px1, py1, px2, py2);
  return true;
}

// key of element e = c*HW + hw of the image's cls_prob slab (kKey0 when filtered); row out
__device__ __forceinline__ unsigned retina_key(const RetinaArgs& a, int img, int e, float s,
                                               int* row, bool* keep) {
  const int c = e / a.HW, hw = e - c * a.HW;
  *row = hw * a.AK + c;
  float4 box;
  *keep = retina_row(a, img, c, hw, s, &box);
  return *keep ? ordered_desc_bits(s) : kKey0;
}

// the elements [lo, hi) of this workgroup's chunk, kUnroll float4 (or scalar) loads per lane a trip
template <typename Fn>
__device__ __forceinline__ void stream_trip(const RetinaArgs& a, const float* __restrict__ sc,
                                            int t0, int hi, Fn&& fn) {
  const int tid = threadIdx.x;
  float v[kUnroll][4];
  if (a.vec) {  // count % 4 == 0 and a 16-byte aligned slab: lo, hi and t0 are multiples of 4
#pragma unroll
    for (int u = 0; u < kUnroll; ++u) {
      const int e = t0 + (u * kScanT + tid) * 4;
      float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
      if (e < hi) f = *reinterpret_cast<const float4*>(sc + e);
      v[u][0] = f.x; v[u][1] = f.y; v[u][2] = f.z; v[u][3] = f.w;
    }
  } else {
#pragma unroll
    for (int u = 0; u < kUnroll; ++u)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int e = t0 + (u * kScanT + tid) * 4 + q;
        v[u][q] = e < hi ? sc[e] : 0.f;
      }
  }
#pragma unroll
  for (int u = 0; u < kUnroll; ++u)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = t0 + (u * kScanT + tid) * 4 + q;
      if (e < hi) fn(e, v[u][q]);
    }
}

// pass 1, grid (G, B)
__global__ __launch_bounds__(kScanT) void retina_scan_kernel(RetinaArgs a) {
  __shared__ int lh[kBins];
  __shared__ unsigned long long lc[kLocal1];
  __shared__ int nl, base;
  const int img = blockIdx.y, tid = threadIdx.x;
  const float* sc = a.cls_prob + (long)img * a.count;
  for (int i = tid; i < kBins; i += kScanT) lh[i] = 0;
  if (tid == 0) nl = 0;
  __syncthreads();
  const int lo = blockIdx.x * a.chunk;
  const int hi = (int)((long)lo + a.chunk < a.count ? lo + a.chunk : a.count);
  float* eff = a.eff + (long)img * a.count;
  for (int t0 = lo; t0 < hi; t0 += kTrip)
    stream_trip(a, sc, t0, hi, [&](int e, float s) {
      if (a.general) {  // every row's effective score
        int row;
        bool keep;
        retina_key(a, img, e, s, &row, &keep);
        eff[row] = keep ? s : 0.0f;
        return;
      }
      if (!(s > a.thresh) || !(s > 0.0f)) return;  // never live
      int row;
      bool keep;
      const unsigned key = retina_key(a, img, e, s, &row, &keep);
      if (!keep) return;
      atomicAdd(&lh[key >> kBinShift], 1);
      const int pos = atomicAdd(&nl, 1);
      if (pos < kLocal1) lc[pos] = ((unsigned long long)key << 32) | (unsigned)row;
    });
  if (a.general) return;
  __syncthreads();
  int* gh = a.ghist + (long)img * kBins;
  for (int i = tid; i < kBins; i += kScanT)
    if (lh[i]) atomicAdd(&gh[i], lh[i]);
  const int n = nl;
  if (n == 0) return;
  int* gc = a.gctr + img * 4;
  if (tid == 0) {
    base = atomicAdd(&gc[0], n);
    if (n > kLocal1) atomicAdd(&gc[1], 1);  // this workgroup's list is incomplete
  }
  __syncthreads();
  if (n > kLocal1) return;
  unsigned long long* cand = a.cand + (long)img * kCap;
  for (int j = tid; j < n; j += kScanT)
    if (base + j < kCap) cand[base + j] = lc[j];
}

// pass 2, grid (G, B)
__global__ __launch_bounds__(kScanT) void retina_compact_kernel(RetinaArgs a) {
  __shared__ unsigned long long lc[kLocal2];
  __shared__ int sh[4], nl, base;
  const int img = blockIdx.y, tid = threadIdx.x;
  if (a.general) return;
  const int* gc = a.gctr + img * 4;
  const int nlive = gc[0];
  if (nlive <= kCap && gc[1] == 0) return;  // the pass-1 list holds every live row
  int bstar, below, nb;
  hist_cut_bin<kBins>(a.ghist + (long)img * kBins, a.pre < nlive ? a.pre : nlive, sh, &bstar, &below, &nb);
  const bool overflow = below + nb > kCap;
  const float* sc = a.cls_prob + (long)img * a.count;
  const int lo = blockIdx.x * a.chunk;
  const int hi = (int)((long)lo + a.chunk < a.count ? lo + a.chunk : a.count);
  if (overflow) {  // general path: every row's effective score
    float* eff = a.eff + (long)img * a.count;
    for (int t0 = lo; t0 < hi; t0 += kTrip)
      stream_trip(a, sc, t0, hi, [&](int e, float s) {
        int row;
        bool keep;
        retina_key(a, img, e, s, &row, &keep);
        eff[row] = keep ? s : 0.0f;
      });
    return;
  }
  if (tid == 0) nl = 0;
  __syncthreads();
  unsigned long long* cand = a.cand + (long)img * kCap;
  int* n2 = a.gctr + img * 4 + 2;
  for (int t0 = lo; t0 < hi; t0 += kTrip) {
    stream_trip(a, sc, t0, hi, [&](int e, float s) {
      if (!(s > a.thresh) || !(s > 0.0f)) return;
      if ((int)(ordered_desc_bits(s) >> kBinShift) > bstar) return;  // below the cut-off bin
      int row;
      bool keep;
      const unsigned key = retina_key(a, img, e, s, &row, &keep);
      if (!keep) return;
      const int pos = atomicAdd(&nl, 1);  // < kLocal2: at most kTrip per trip, flushed below
      lc[pos] = ((unsigned long long)key << 32) | (unsigned)row;
    });
    __syncthreads();
    const int n = nl;
    if (n > kLocal2 - kTrip || (t0 + kTrip >= hi && n > 0))
      wg_list_flush<kScanT>(lc, n, &nl, &base, n2, cand, kCap);
    __syncthreads();
  }
}

// one workgroup per image
__global__ __launch_bounds__(1024) void retina_finish_kernel(RetinaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long keys[];  // kCap words
  __shared__ int hist[260];
  __shared__ int sh[4], ncand;
  const int img = blockIdx.x, tid = threadIdx.x, T = blockDim.x;
  const int* gc = a.gctr + img * 4;
  bool general = a.general;
  int nsel = 0;
  if (!general) {
    const int nlive = gc[0];
    if (nlive > 0) {
      const int want = a.pre < nlive ? a.pre : nlive;
      int bstar, below, nb;
      hist_cut_bin<kBins>(a.ghist + (long)img * kBins, want, sh, &bstar, &below, &nb);
      const bool from1 = nlive <= kCap && gc[1] == 0;
      if (!from1 && below + nb > kCap) {
        general = true;
      } else {
        const int n = from1 ? nlive : gc[2];
        const unsigned long long* cand = a.cand + (long)img * kCap;
        if (tid == 0) ncand = 0;
        __syncthreads();
        for (int i = tid; i < n && i < kCap; i += T) {
          const unsigned long long k = cand[i];
          if ((int)((unsigned)(k >> 32) >> kBinShift) <= bstar) keys[atomicAdd(&ncand, 1)] = k;
        }
        __syncthreads();
        const int m = ncand;
        const int P2 = sort_size(m, 64);
        for (int i = m + tid; i < P2; i += T) keys[i] = ~0ull;
        __syncthreads();
        bitonic_sort_lds(keys, P2, tid, T);
        nsel = want < m ? want : m;  // == want (the bins up to the cut-off hold >= want live rows)
      }
    }
  }
  if (general) {
    const int P2 = sort_size(a.pre, 64);
    select_sort_topk<1>(a.eff + (long)img * a.count, a.count, a.pre, P2, keys, hist, &ncand);
    nsel = a.pre;
  }
  __syncthreads();
  // PrepareOutput (:275-297): every row of out / score written (zeros past the selected rows)
  const float* sc = a.cls_prob + (long)img * a.count;
  float* o4 = a.out + (long)img * a.top_n * 4;
  float* os = a.score + (long)img * a.top_n * a.oc;
  for (int j = tid; j < a.top_n; j += T) {
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    float s = 0.0f;
    int col = 0;
    bool keep = false;
    if (j < nsel) {
      const int row = (int)(unsigned)(keys[j] & 0xffffffffu);
      const int c = row % a.AK, hw = row / a.AK;
      s = sc[(long)c * a.HW + hw];
      keep = retina_row(a, img, c, hw, s, &box);
      col = iminr(a.oc - 1, c % a.K + 1);
    }
    if (!keep) {
      box = make_float4(0.f, 0.f, 0.f, 0.f);
      s = 0.0f;
    }
    o4[(long)j * 4 + 0] = box.x;
    o4[(long)j * 4 + 1] = box.y;
    o4[(long)j * 4 + 2] = box.z;
    o4[(long)j * 4 + 3] = box.w;
    float* srow = os + (long)j * a.oc;
    for (int q = 0; q < a.oc; ++q) srow[q] = q == col ? s : 0.0f;
  }
}

struct RetinaWs {
  int* ghist;
  int* gctr;
  unsigned long long* cand;
  float* eff;
};

// bytes of the workspace in use; the size query passes a null workspace and gets null pointers
size_t retina_layout(int B, long count, RetinaWs* ws, void* workspace) {
  WsCarver c(workspace);
  ws->ghist = c.take<int>((size_t)B * (kBins + 4) * sizeof(int));
  ws->gctr = ws->ghist ? ws->ghist + (size_t)B * kBins : nullptr;
  ws->cand = c.take<unsigned long long>((size_t)B * kCap * sizeof(unsigned long long));
  ws->eff = c.take<float>((size_t)B * count * sizeof(float));
  return c.need();
}

}  // namespace
}  // namespace sd

using namespace sd;

extern "C" size_t sd_gen_proposal_retina_workspace_bytes(int B, int AK, int H, int W) {
  if (B <= 0 || AK <= 0 || H <= 0 || W <= 0) return 256;
  RetinaWs ws;
  return retina_layout(B, (long)AK * H * W, &ws, nullptr) + 256;
}

extern "C" int sd_gen_proposal_retina(const float* cls_prob, const float* bbox_pred,
                                      const float* im_info, const float* anchors, float* out,
                                      float* score, int B, int AK, int H, int W, int num_anchors,
                                      int rpn_pre_nms_top_n, int rpn_min_size, float thresh,
                                      const float* mean_host, const float* std_host, int iou_loss,
                                      int output_one_hot, int batch_wise_anchor, void* workspace,
                                      size_t workspace_bytes, void* stream) {
  SD_REQUIRE(B >= 0 && AK > 0 && H > 0 && W > 0, "GenProposalRetina: bad dimensions");
  SD_REQUIRE(num_anchors > 0 && AK % num_anchors == 0,
             "GenProposalRetina: cls_prob channels (%d) must be a multiple of num_anchors (%d)", AK,
             num_anchors);
  SD_REQUIRE(rpn_pre_nms_top_n > 0, "GenProposalRetina: rpn_pre_nms_top_n must be > 0");
  SD_REQUIRE(!isnan(thresh), "GenProposalRetina: thresh is NaN");
  SD_REQUIRE(mean_host && std_host, "GenProposalRetina: null anchor_mean / anchor_std");
  const int K = AK / num_anchors;
  const long count = (long)AK * H * W;
  if (count > kMaxRows)
    return fail(SD_ERR_UNSUPPORTED, "GenProposalRetina: %ld rows per image (A*K*H*W) exceed the "
                "limit of %ld", count, kMaxRows);
  if (iou_loss && K > 1)  // IoUPredKernel reads deltas past the (4A, H, W) slab (:161-209)
    return fail(SD_ERR_UNSUPPORTED, "GenProposalRetina: iou_loss needs one class (K=%d)", K);
  if (batch_wise_anchor && B > 1 && K > 1)  // anchor offset i*count*4 with count = A*K*H*W (:383)
    return fail(SD_ERR_UNSUPPORTED, "GenProposalRetina: batch_wise_anchor with B=%d > 1 and K=%d > 1",
                B, K);
  const int pre = rpn_pre_nms_top_n < count ? rpn_pre_nms_top_n : (int)count;
  if (pre > kCap)
    return fail(SD_ERR_UNSUPPORTED, "GenProposalRetina: min(rpn_pre_nms_top_n, rows) = %d exceeds %d",
                pre, kCap);
  if (B == 0) return SD_OK;
  SD_REQUIRE(cls_prob && bbox_pred && im_info && anchors && out && score,
             "GenProposalRetina: null tensor pointer");
  RetinaWs ws;
  const size_t need = retina_layout(B, count, &ws, workspace);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "GenProposalRetina workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  RetinaArgs a{};
  a.cls_prob = cls_prob; a.bbox_pred = bbox_pred; a.im_info = im_info; a.anchors = anchors;
  a.out = out; a.score = score;
  for (int q = 0; q < 4; ++q) {
    a.mean[q] = mean_host[q];
    a.stdv[q] = std_host[q];
  }
  a.AK = AK; a.K = K; a.A = num_anchors; a.HW = H * W; a.count = (int)count; a.pre = pre;
  a.top_n = rpn_pre_nms_top_n;
  a.oc = output_one_hot ? K + 1 : 1;
  a.anchor_img = batch_wise_anchor ? (long)H * W * num_anchors * 4 : 0;
  a.min_size = (float)rpn_min_size;
  a.thresh = thresh;
  a.iou_loss = iou_loss ? 1 : 0;
  a.vec = (count % 4 == 0) && (((uintptr_t)cls_prob & 15) == 0);
  a.general = thresh < 0.0f;
  // one kTrip-element trip or more per workgroup, at most 512 workgroups per image
  long G = (count + kTrip - 1) / kTrip;
  if (G > 512) G = 512;
  const long chunk = ((count + G - 1) / G + kTrip - 1) / kTrip * kTrip;
  a.chunk = (int)chunk;
  a.G = (int)((count + chunk - 1) / chunk);
  a.ghist = ws.ghist; a.gctr = ws.gctr; a.cand = ws.cand; a.eff = ws.eff;
  hipStream_t st = (hipStream_t)stream;
  zero_counters(ws.ghist, (long)B * (kBins + 4), st);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(retina_scan_kernel, dim3(a.G, B), dim3(kScanT), 0, st, a);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(retina_compact_kernel, dim3(a.G, B), dim3(kScanT), 0, st, a);
  SD_LAUNCH_CHECK();
  const size_t lds = (size_t)kCap * sizeof(unsigned long long);
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)retina_finish_kernel,
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(retina_finish_kernel, dim3(B), dim3(1024), lds, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
