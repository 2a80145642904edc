// The FreeAnchor training head: FreeAnchorRetinaNetHead.get_loss (models/FreeAnchor/builder.py:67-148)
// with _prepare_anchors, _positive_loss and _negative_loss (models/FreeAnchor/ops.py:44-210) -- about 120 graph
// nodes, two (M, anchors) IoU matrices per image, a full top-k per gt row, a (N, anchors, K) one-hot and ten
// element-wise passes over the class probabilities behind a concat + transpose of every level.  Here every input is
// read where the head left it: logits (N, A*K, H_l, W_l), deltas (N, A*4, H_l, W_l), the loader's anchors
// (1, 1, S_l, S_l, A*4) cropped by their row pitch.  Anchor i = (off_l + y*W_l + x)*A + a, class c in channel a*K + c.
//
//   forward   fa_bag_kernel     one workgroup per (gt, image): every anchor's IoU streamed once, a streaming top-k
//                               over an LDS list of 64-bit (IoU key, index) words behind a rising threshold
//             fa_gtmax_kernel   one anchor per thread: decode once, the M IoUs against the gt rows in LDS, per-gt
//                               maxima by wave, LDS and global integer atomicMax on the IoU's bits
//             fa_anchor_kernel  the same thread mapping: first arg-max over the gts and box_prob kept per anchor
//                               (8 bytes), the K classes of the negative loss, per-workgroup partials
//             fa_pos_kernel     one wave per (gt, image): the bag's loss term and five gradient coefficients per entry
//             fa_finish_kernel  one workgroup: #valid gt, both losses from the partials in index order
//   backward  fa_anchor_kernel<BWD>  every element of d_cls_logit (the negative part), zeros into d_bbox_delta
//             fa_sparse_kernel  one workgroup per image: the bag entries sorted by (anchor, gt, rank) in LDS, the first
//                               thread of an anchor's run adds the run's coefficients in key order
//
// Integer atomics only, no memset node, no host read: graph-capturable, equal bits on every call.  fp32.
#include "../../include/simpledet_ops.h"
#include "box_common.h"
#include "loss_common.h"
#include "select_common.h"
#include "wg_common.h"
#include <math.h>

namespace sd {

constexpr int kFaT = 256;
constexpr int kFaWaves = kFaT / kWave;
constexpr int kFaMaxL = SD_MAX_FPN_LEVELS;
constexpr int kFaMaxM = 256;                        // gt rows in LDS
constexpr int kFaCap = 1024;                        // keys of the bag kernel's candidate list
constexpr int kFaUn = 2;                            // anchors per thread and trip of the bag kernel
// (tests/free_anchor_ref.py:prunes counts the cuts of its `prune` case with kFaCap and kFaUn * kFaT: change them together)
constexpr int kFaMaxTop = kFaCap - kFaUn * kFaT;    // a pruned list + one trip's candidates fit: top_n <= 512
constexpr int kFaCoef = 5;                          // per bag entry: dL/d logit, dL/d delta[0..4)
constexpr float kFaBoxWeight = 0.75f;               // bbox_loss_weight, ops.py:117

struct FaRecord {   // per anchor, forward -> backward
  int gt;           // the arg-max gt row, -1 where its label is <= 0 (the anchor does not count)
  float box_prob;
};

struct FaArgs {
  const float* cls[kFaMaxL];
  const float* delta[kFaMaxL];
  const float* anchor[kFaMaxL];
  float* dcls[kFaMaxL];
  float* ddelta[kFaMaxL];
  long off[kFaMaxL + 1];    // locations in front of level l; off[L] = HW
  long pitch[kFaMaxL];      // locations per row of the level's anchor tensor (S_l >= W_l)
  int w[kFaMaxL];
  int L, N, A, K, M, top_n, aligned;
  long HW, NA;              // locations and anchors per image
  const float *gt, *im_info;
  float thr, thr2, alpha, gamma, bsq, ibsq, grad_scale;
  float means[4], stds[4];
  float* loss;
  int* bags_out;
  // workspace
  int* bags;                // (N, M, top_n), -1 in the rows of invalid gts
  unsigned* gtmax;          // (N, M) bits of the largest IoU(gt, decoded box)
  FaRecord* rec;            // (N, NA) in the thread order of the anchor pass
  float* coef;              // (N, M, top_n, 5), not scaled by 1 / #valid
  float* pos_part;          // (N, M)
  float* neg_part;          // (N, nblocks)
  int* state;               // [#valid gt of the batch]
  int nblocks;
};

struct FaLevel { int l, w; long first, hw, pitch; };
__device__ __forceinline__ FaLevel fa_level(const FaArgs& a, long q) {
  FaLevel r{0, a.w[0], 0, a.off[1], a.pitch[0]};
#pragma unroll
  for (int l = 1; l < kFaMaxL; ++l)
    if (l < a.L && q >= a.off[l]) r = FaLevel{l, a.w[l], a.off[l], a.off[l + 1] - a.off[l], a.pitch[l]};
  return r;
}
template <typename T>
__device__ __forceinline__ T* fa_pick(T* const (&tab)[kFaMaxL], int lv) {
  T* p = tab[0];
#pragma unroll
  for (int l = 1; l < kFaMaxL; ++l)
    if (lv == l) p = tab[l];
  return p;
}

// anchor `an` of location p of a level: slice_like is the row pitch
__device__ __forceinline__ float4 fa_anchor(const FaArgs& a, const FaLevel& lv, long p, int an) {
  const long y = p / lv.w, x = p - y * lv.w;
  const float* s = fa_pick(a.anchor, lv.l) + ((y * lv.pitch + x) * a.A + an) * 4;
  if (a.aligned) return *reinterpret_cast<const float4*>(s);
  return make_float4(s[0], s[1], s[2], s[3]);
}

__device__ __forceinline__ bool fa_valid(float label) { return label > 0.f; }
// gt_index = maximum(label - 1, 0); a label above K would gather out of bounds in the reference: the last class here
__device__ __forceinline__ int fa_class(float label, int K) { return iminr(imaxr((int)label - 1, 0), K - 1); }

// ---- 1. bags -----------------------------------------------------------------------------------------------
// sort the list, keep the top_n best, return the top_n-th key: later candidates must beat it
__device__ __forceinline__ unsigned long long fa_prune(unsigned long long* keys, int* cnt, int top_n) {
  const int tid = threadIdx.x, c = *cnt;
  for (int i = c + tid; i < kFaCap; i += kFaT) keys[i] = ~0ull;
  __syncthreads();
  bitonic_sort_lds(keys, kFaCap, tid, kFaT);
  const unsigned long long thr = keys[top_n - 1];
  __syncthreads();
  if (tid == 0) *cnt = iminr(c, top_n);
  __syncthreads();
  return thr;
}

__global__ __launch_bounds__(kFaT) void fa_bag_kernel(FaArgs a) {
  __shared__ unsigned long long keys[kFaCap];
  __shared__ int cnt;
  const int m = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const long row = (long)n * a.M + m;
  const float* g = a.gt + row * 5;
  int* bag = a.bags + row * a.top_n;
  int* out = a.bags_out ? a.bags_out + row * a.top_n : nullptr;
  if (tid == 0) a.gtmax[row] = 0u;
  if (!fa_valid(g[4])) {
    for (int k = tid; k < a.top_n; k += kFaT) {
      bag[k] = -1;
      if (out) out[k] = -1;
    }
    return;
  }
  const float gb[4] = {g[0], g[1], g[2], g[3]};
  if (tid == 0) cnt = 0;
  unsigned long long thr = ~0ull;
  for (long base = 0; base < a.NA; base += kFaUn * kFaT) {
    __syncthreads();
    const int c = cnt;
    __syncthreads();   // everybody has read the count before anybody appends
    if (c + kFaUn * kFaT > kFaCap) thr = fa_prune(keys, &cnt, a.top_n);
    unsigned long long key[kFaUn];
    bool take[kFaUn];
#pragma unroll
    for (int u = 0; u < kFaUn; ++u) {
      const long i = base + u * kFaT + tid;
      take[u] = false;
      key[u] = 0;
      if (i < a.NA) {
        const long q = i / a.A;
        const FaLevel lv = fa_level(a, q);
        const float4 b = fa_anchor(a, lv, q - lv.first, (int)(i - q * a.A));
        const float bb[4] = {b.x, b.y, b.z, b.w};
        key[u] = ((unsigned long long)ordered_desc_bits(box_iou_corner(gb, bb)) << 32) | (unsigned)i;
        take[u] = key[u] < thr;
      }
    }
#pragma unroll
    for (int u = 0; u < kFaUn; ++u) {
      const int pos = wave_append(take[u], &cnt);
      if (take[u]) keys[pos] = key[u];
    }
  }
  __syncthreads();
  fa_prune(keys, &cnt, a.top_n);
  for (int k = tid; k < a.top_n; k += kFaT) {
    const int i = (int)(unsigned)(keys[k] & 0xffffffffull);
    bag[k] = i;
    if (out) out[k] = i;
  }
}

// ---- 2 / 3 / 5. one anchor per thread ---------------------------------------------------------------------------
// thread j of image n: anchor a = j / HW at concat position q = j % HW, so consecutive threads read consecutive
// locations of every channel
struct FaThread { bool live; int an; long p; FaLevel lv; };
__device__ __forceinline__ FaThread fa_thread(const FaArgs& a) {
  FaThread t;
  const long j = (long)blockIdx.x * kFaT + threadIdx.x;
  t.live = j < a.NA;
  const long jj = t.live ? j : 0;
  t.an = (int)(jj / a.HW);
  const long q = jj - t.an * a.HW;
  t.lv = fa_level(a, q);
  t.p = q - t.lv.first;
  return t;
}

__device__ __forceinline__ void fa_decode(const FaArgs& a, int n, const FaThread& t, float* box) {
  const float* d = fa_pick(a.delta, t.lv.l) + ((long)n * 4 * a.A + t.an * 4) * t.lv.hw + t.p;
  const float4 dd = make_float4(d[0], d[t.lv.hw], d[2 * t.lv.hw], d[3 * t.lv.hw]);
  const float wm = a.im_info[n * 3 + 1] - 1.0f, hm = a.im_info[n * 3 + 0] - 1.0f;
  const float4 o = decode_box(fa_anchor(a, t.lv, t.p, t.an), dd, a.means, a.stds, true, wm, hm);
  box[0] = o.x; box[1] = o.y; box[2] = o.z; box[3] = o.w;
}

__global__ __launch_bounds__(kFaT) void fa_gtmax_kernel(FaArgs a) {
  __shared__ float sgt[kFaMaxM * 5];
  __shared__ unsigned smax[kFaMaxM];
  const int n = blockIdx.y;
  for (int i = threadIdx.x; i < a.M * 5; i += kFaT) sgt[i] = a.gt[(long)n * a.M * 5 + i];
  for (int i = threadIdx.x; i < a.M; i += kFaT) smax[i] = 0u;
  __syncthreads();
  const FaThread t = fa_thread(a);
  float box[4];
  fa_decode(a, n, t, box);
  for (int m = 0; m < a.M; ++m) {
    const float v = box_iou_corner(sgt + m * 5, box);
    const unsigned wm = wave_max_u32(t.live ? __float_as_uint(v) : 0u);   // an IoU is >= 0: unsigned order is float order
    if ((threadIdx.x & (kWave - 1)) == 0 && wm) atomicMax(smax + m, wm);
  }
  __syncthreads();
  for (int m = threadIdx.x; m < a.M; m += kFaT)
    if (smax[m]) atomicMax(a.gtmax + (long)n * a.M + m, smax[m]);
}

// -prob^gamma * log(clip(1 - prob, 1e-12, 1)) and its derivative in prob (clip passes the gradient on [1e-12, 1])
template <int GAMMA>
__device__ __forceinline__ float fa_neg_term(float prob, float gamma) {
  const float om = 1.0f - prob;
  const float c = om > 1.0f ? 1.0f : (om < 1e-12f ? 1e-12f : om);
  return -pow_gamma<GAMMA>(prob, gamma) * logf(c);
}
template <int GAMMA>
__device__ __forceinline__ float fa_neg_grad(float prob, float gamma) {
  const float om = 1.0f - prob;
  const float c = om > 1.0f ? 1.0f : (om < 1e-12f ? 1e-12f : om);
  const float dpow = GAMMA == 2 ? 2.0f * prob : gamma * powf(prob, gamma - 1.0f);
  const float pass = (om >= 1e-12f && om <= 1.0f) ? 1.0f : 0.0f;
  return -dpow * logf(c) + pow_gamma<GAMMA>(prob, gamma) * (pass / c);
}

template <int GAMMA, bool BWD>
__global__ __launch_bounds__(kFaT) void fa_anchor_kernel(FaArgs a) {
  const int n = blockIdx.y;
  const FaThread t = fa_thread(a);
  const long j = (long)blockIdx.x * kFaT + threadIdx.x;
  FaRecord r{-1, 0.f};
  if (!BWD) {   // the gt rows live in LDS in the forward only: the backward reads the per-anchor record
    __shared__ float sgt[kFaMaxM * 5];
    __shared__ float smax[kFaMaxM];
    for (int i = threadIdx.x; i < a.M * 5; i += kFaT) sgt[i] = a.gt[(long)n * a.M * 5 + i];
    for (int i = threadIdx.x; i < a.M; i += kFaT)
      smax[i] = fmaxr(__uint_as_float(a.gtmax[(long)n * a.M + i]), a.thr2);   // t2 = maximum(max IoU, t1 + 1e-12)
    __syncthreads();
    float box[4];
    fa_decode(a, n, t, box);
    float best = 0.f;
    int arg = 0;
    for (int m = 0; m < a.M; ++m) {
      float v = (box_iou_corner(sgt + m * 5, box) - a.thr) / (smax[m] - a.thr);
      v = v > 1.0f ? 1.0f : (v < 0.0f ? 0.0f : v);
      if (m == 0 || v > best) { best = v; arg = m; }   // the first arg-max: all zeros leave row 0
    }
    const float label = sgt[arg * 5 + 4];
    r.gt = fa_valid(label) ? arg : -1;
    r.box_prob = best;
    if (t.live) a.rec[(long)n * a.NA + j] = r;
  } else if (t.live) {
    r = a.rec[(long)n * a.NA + j];
  }
  // one_hot(label - 1, depth = K): a label above K hits no class
  int hit = -1;
  if (r.gt >= 0) hit = (int)a.gt[((long)n * a.M + r.gt) * 5 + 4] - 1;
  float acc = 0.f, scale = 0.f;
  if (BWD) scale = a.grad_scale * (1.0f - a.alpha) / (float)imaxr(a.state[0] * a.top_n, 1);
  if (t.live) {
    const long e0 = ((long)n * a.A * a.K + (long)t.an * a.K) * t.lv.hw + t.p;
    const float* x = fa_pick(a.cls, t.lv.l) + e0;
    float* dx = BWD ? fa_pick(a.dcls, t.lv.l) + e0 : nullptr;
    if (r.gt < 0) {   // where(valid, prob, 0): the terms and their gradients are exactly 0
      if (BWD)
        for (int c = 0; c < a.K; ++c) dx[c * t.lv.hw] = 0.f;
    } else {
      for (int c = 0; c < a.K; ++c) {
        const float p = sigmoid_f32(x[c * t.lv.hw]);
        const float keep = c == hit ? 1.0f - r.box_prob : 1.0f;
        const float prob = p * keep;
        if (!BWD)
          acc += fa_neg_term<GAMMA>(prob, a.gamma);
        else
          dx[c * t.lv.hw] = ((fa_neg_grad<GAMMA>(prob, a.gamma) * scale) * keep) * (p * (1.0f - p));
      }
    }
    if (BWD) {
      float* dd = fa_pick(a.ddelta, t.lv.l) + ((long)n * 4 * a.A + t.an * 4) * t.lv.hw + t.p;
#pragma unroll
      for (int k = 0; k < 4; ++k) dd[k * t.lv.hw] = 0.f;
    }
  }
  if (!BWD) {
    __shared__ float shf[kFaWaves];
    const float s = block_sum_f32<kFaT, false>(acc, shf);
    if (threadIdx.x == 0) a.neg_part[(long)n * a.nblocks + blockIdx.x] = s;
  }
}

// ---- 4. the bags' loss terms and coefficients ------------------------------------------------------------------
// what a bag entry touches: its level, the element of its class logit and of its first delta
struct FaEntry { int l; long hw, ecls, edelta; float4 anchor; };
__device__ __forceinline__ FaEntry fa_entry(const FaArgs& a, int n, int i, int c) {
  const long q = i / a.A;
  const int an = i - (int)q * a.A;
  const FaLevel lv = fa_level(a, q);
  const long p = q - lv.first;
  FaEntry e;
  e.l = lv.l;
  e.hw = lv.hw;
  e.ecls = ((long)n * a.A * a.K + (long)an * a.K + c) * lv.hw + p;
  e.edelta = ((long)n * 4 * a.A + an * 4) * lv.hw + p;
  e.anchor = fa_anchor(a, lv, p, an);
  return e;
}

__global__ __launch_bounds__(kWave) void fa_pos_kernel(FaArgs a) {
  __shared__ float sp[kFaMaxTop], sb[kFaMaxTop], sw[kFaMaxTop], sg[4][kFaMaxTop];
  const int m = blockIdx.x, n = blockIdx.y, lane = threadIdx.x;
  const long row = (long)n * a.M + m;
  const float* g = a.gt + row * 5;
  if (!fa_valid(g[4])) {   // where(valid, ., 1): bag_prob = 1, loss 0, no gradient
    if (lane == 0) a.pos_part[row] = 0.f;
    return;
  }
  const int c = fa_class(g[4], a.K);
  const float gw = g[2] - g[0] + 1.0f, gh = g[3] - g[1] + 1.0f;
  const float gcx = g[0] + 0.5f * (gw - 1.0f), gcy = g[1] + 0.5f * (gh - 1.0f);
  float wsum = 0.f;
  for (int k = lane; k < a.top_n; k += kWave) {
    const FaEntry e = fa_entry(a, n, a.bags[row * a.top_n + k], c);
    const float p = sigmoid_f32(fa_pick(a.cls, e.l)[e.ecls]);
    const float* d = fa_pick(a.delta, e.l) + e.edelta;
    // _bbox_encode (ops.py:6-41)
    const float ew = e.anchor.z - e.anchor.x + 1.0f, eh = e.anchor.w - e.anchor.y + 1.0f;
    const float ecx = e.anchor.x + 0.5f * (ew - 1.0f), ecy = e.anchor.y + 0.5f * (eh - 1.0f);
    float tg[4];
    tg[0] = ((gcx - ecx) / (ew + 1e-14f) - a.means[0]) / a.stds[0];
    tg[1] = ((gcy - ecy) / (eh + 1e-14f) - a.means[1]) / a.stds[1];
    tg[2] = (logf(gw / ew) - a.means[2]) / a.stds[2];
    tg[3] = (logf(gh / eh) - a.means[3]) / a.stds[3];
    float s = 0.f;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float v = d[t * e.hw] - tg[t];
      const float l = smooth_l1(v, a.bsq, a.ibsq) * kFaBoxWeight;
      s = t == 0 ? l : s + l;
      sg[t][k] = smooth_l1_grad(v, a.bsq, a.ibsq);
    }
    const float b = expf(-s);
    const float w = 1.0f / fmaxr(1.0f - p * b, 1e-12f);
    sp[k] = p; sb[k] = b; sw[k] = w;
    wsum += w;
  }
  const float W = wave_sum_f32(wsum);
  float bsum = 0.f;
  for (int k = lane; k < a.top_n; k += kWave) bsum += (sw[k] / W) * (sp[k] * sb[k]);
  const float bag = wave_sum_f32(bsum);
  const float cb = bag > 1.0f ? 1.0f : (bag < 1e-12f ? 1e-12f : bag);
  if (lane == 0) a.pos_part[row] = -a.alpha * logf(cb);
  // d loss / d bag_prob; the weights are differentiated too (no BlockGrad on them in the reference):
  // d bag / d q_k = w_k / W + (q_k - bag) / W * w_k^2 [1 - q_k >= 1e-12]
  const float dbag = (bag >= 1e-12f && bag <= 1.0f) ? -a.alpha / cb : 0.f;
  for (int k = lane; k < a.top_n; k += kWave) {
    const float p = sp[k], b = sb[k], w = sw[k], q = p * b;
    const float dw = (1.0f - q >= 1e-12f) ? w * w : 0.f;
    const float gq = dbag * (w / W + ((q - bag) / W) * dw);
    float* o = a.coef + (row * a.top_n + k) * kFaCoef;
    o[0] = (gq * b) * (p * (1.0f - p));
    const float gs = -(gq * p) * b * kFaBoxWeight;   // through exp(-sum) and the loss weight
#pragma unroll
    for (int t = 0; t < 4; ++t) o[1 + t] = gs * sg[t][k];
  }
}

// ONE workgroup: #valid gt, then both losses; thread t adds partials t, t + 256, ... in order
__global__ __launch_bounds__(kFaT) void fa_finish_kernel(FaArgs a) {
  __shared__ int shi[kFaWaves];
  __shared__ float shf[kFaWaves];
  int v = 0;
  float pos = 0.f, neg = 0.f;
  for (int i = threadIdx.x; i < a.N * a.M; i += kFaT) {
    v += fa_valid(a.gt[(long)i * 5 + 4]) ? 1 : 0;
    pos += a.pos_part[i];
  }
  for (int i = threadIdx.x; i < a.N * a.nblocks; i += kFaT) neg += a.neg_part[i];
  v = block_sum_i32<kFaT>(v, shi);
  pos = block_sum_f32<kFaT>(pos, shf);
  neg = block_sum_f32<kFaT, false>(neg, shf);
  if (threadIdx.x == 0) {
    a.state[0] = v;
    a.loss[0] = pos / (float)imaxr(v, 1);
    a.loss[1] = ((1.0f - a.alpha) * neg) / (float)imaxr(v * a.top_n, 1);
  }
}

// ---- 6. the bags' gradients ------------------------------------------------------------------------------------
// Two gts may hold the same anchor, with equal labels the same logit: the image's entries are sorted by
// (anchor, gt, rank), and the thread on the first entry of an anchor's run adds the whole run, in key order, to what
// fa_anchor_kernel<BWD> wrote.  One owner per element, one order.
__global__ __launch_bounds__(kFaT) void fa_sparse_kernel(FaArgs a, int P2) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long fa_keys[];
  const int n = blockIdx.x, tid = threadIdx.x, E = a.M * a.top_n;
  const int* bags = a.bags + (long)n * E;
  for (int e = tid; e < P2; e += kFaT) {
    const int i = e < E ? bags[e] : -1;
    fa_keys[e] = i >= 0 ? ((unsigned long long)(unsigned)i << 32) | (unsigned)e : ~0ull;
  }
  __syncthreads();
  bitonic_sort_lds(fa_keys, P2, tid, kFaT);
  const float scale = a.grad_scale / (float)imaxr(a.state[0], 1);
  for (int t = tid; t < E; t += kFaT) {
    const unsigned long long key = fa_keys[t];
    if (key == ~0ull) continue;
    const unsigned i = (unsigned)(key >> 32);
    if (t > 0 && (unsigned)(fa_keys[t - 1] >> 32) == i) continue;
    float dd[4] = {0.f, 0.f, 0.f, 0.f};
    FaEntry en{};
    for (int u = t; u < E && (unsigned)(fa_keys[u] >> 32) == i; ++u) {
      const int e = (int)(unsigned)(fa_keys[u] & 0xffffffffull);
      const int c = fa_class(a.gt[((long)n * a.M + e / a.top_n) * 5 + 4], a.K);
      en = fa_entry(a, n, (int)i, c);
      const float* co = a.coef + ((long)n * E + e) * kFaCoef;
      float* dx = fa_pick(a.dcls, en.l) + en.ecls;
      *dx = *dx + co[0] * scale;
#pragma unroll
      for (int k = 0; k < 4; ++k) dd[k] += co[1 + k] * scale;
    }
    float* d = fa_pick(a.ddelta, en.l) + en.edelta;
#pragma unroll
    for (int k = 0; k < 4; ++k) d[k * en.hw] = dd[k];
  }
}

// ---- host --------------------------------------------------------------------------------------------------
static int fa_blocks(long NA) { return cdiv(NA, kFaT); }

// the buffers of the workspace, in one order for the query (a null workspace) and the call
static size_t fa_carve(FaArgs& a, void* workspace) {
  WsCarver c(workspace);
  const size_t rows = (size_t)a.N * a.M;
  a.bags = c.take<int>(rows * a.top_n * sizeof(int));
  a.gtmax = c.take<unsigned>(rows * sizeof(unsigned));
  a.rec = c.take<FaRecord>((size_t)a.N * a.NA * sizeof(FaRecord));
  a.coef = c.take<float>(rows * a.top_n * kFaCoef * sizeof(float));
  a.pos_part = c.take<float>(rows * sizeof(float));
  a.neg_part = c.take<float>((size_t)a.N * a.nblocks * sizeof(float));
  a.state = c.take<int>(4 * sizeof(int));
  return c.need();
}

static int fa_dims(FaArgs& a, int N, int L, const long* hw_host, const long* w_host, int A, int K, int M, int top_n) {
  SD_REQUIRE(L >= 1 && L <= kFaMaxL, "L = %d outside [1,%d]", L, kFaMaxL);
  SD_REQUIRE(N >= 0 && A >= 1 && K >= 1 && M >= 1 && top_n >= 1, "bad N / A / K / M / top_n");
  SD_REQUIRE(hw_host, "null level sizes");
  if (M > kFaMaxM) return fail(SD_ERR_UNSUPPORTED, "free_anchor: M = %d > %d", M, kFaMaxM);
  if (top_n > kFaMaxTop) return fail(SD_ERR_UNSUPPORTED, "free_anchor: top_n = %d > %d", top_n, kFaMaxTop);
  if ((long)M * top_n > kMaxSortKeys)
    return fail(SD_ERR_UNSUPPORTED, "free_anchor: M * top_n = %ld > %d", (long)M * top_n, kMaxSortKeys);
  long hw = 0;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(hw_host[l] >= 1, "level %d is empty", l);
    if (w_host) SD_REQUIRE(w_host[l] >= 1 && hw_host[l] % w_host[l] == 0, "level %d: H * W = %ld, W = %ld", l, hw_host[l], w_host[l]);
    a.off[l] = hw;
    a.w[l] = w_host ? (int)w_host[l] : 1;
    hw += hw_host[l];
    if ((double)(N > 0 ? N : 1) * A * (K > 4 ? K : 4) * (double)hw > 2147483647.0)
      return fail(SD_ERR_UNSUPPORTED, "free_anchor: more than 2^31 - 1 elements");
  }
  for (int l = L; l <= kFaMaxL; ++l) a.off[l] = hw;
  a.L = L; a.N = N; a.A = A; a.K = K; a.M = M; a.top_n = top_n;
  a.HW = hw; a.NA = hw * A;
  a.nblocks = fa_blocks(a.NA);
  SD_REQUIRE(top_n <= a.NA, "top_n = %d above the %ld anchors", top_n, a.NA);
  return SD_OK;
}

static int fa_args(FaArgs& a, const float* const* cls_ptrs_host, const float* const* delta_ptrs_host,
                   const float* const* anchor_ptrs_host, const long* anchor_pitch_host, const float* gt_bbox,
                   const float* im_info, int N, int L, const long* hw_host, const long* w_host, int A, int K, int M,
                   int top_n, float bbox_thr, float alpha, float gamma, const float* mean_host, const float* std_host,
                   void* workspace, size_t workspace_bytes) {
  SD_REQUIRE(w_host && anchor_pitch_host, "null level widths / anchor pitches");
  if (int e = fa_dims(a, N, L, hw_host, w_host, A, K, M, top_n)) return e;
  SD_REQUIRE(cls_ptrs_host && delta_ptrs_host && anchor_ptrs_host, "null level table");
  SD_REQUIRE(mean_host && std_host, "null mean / std");
  a.aligned = 1;
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(cls_ptrs_host[l] && delta_ptrs_host[l] && anchor_ptrs_host[l], "null pointer in level %d", l);
    SD_REQUIRE(anchor_pitch_host[l] >= w_host[l], "level %d: anchor pitch %ld below its width %ld", l,
               anchor_pitch_host[l], w_host[l]);
    a.cls[l] = cls_ptrs_host[l]; a.delta[l] = delta_ptrs_host[l]; a.anchor[l] = anchor_ptrs_host[l];
    a.pitch[l] = anchor_pitch_host[l];
    if ((uintptr_t)anchor_ptrs_host[l] & 15) a.aligned = 0;
  }
  SD_REQUIRE(gt_bbox && im_info, "null pointer (gt_bbox / im_info)");
  a.gt = gt_bbox; a.im_info = im_info;
  a.thr = bbox_thr;
  a.thr2 = (float)((double)bbox_thr + 1e-12);
  a.alpha = alpha; a.gamma = gamma;
  const float sigma = (float)sqrt(1.0 / 0.11);   // ops.py:116-119
  a.bsq = sigma * sigma; a.ibsq = 1.0f / a.bsq;
  for (int i = 0; i < 4; ++i) {
    SD_REQUIRE(std_host[i] != 0.f, "std[%d] is 0", i);
    a.means[i] = mean_host[i]; a.stds[i] = std_host[i];
  }
  if (N == 0) return SD_OK;
  const size_t need = fa_carve(a, workspace);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "free_anchor workspace too small: %zu < %zu bytes", workspace_bytes, need);
  return SD_OK;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_free_anchor_workspace_bytes(int N, int L, const long* hw_host, int A, int K, int M, int top_n) {
  FaArgs a{};
  if (N <= 0 || fa_dims(a, N, L, hw_host, nullptr, A, K, M, top_n) != SD_OK) return 256;
  return fa_carve(a, nullptr) + 256;
}

extern "C" int sd_free_anchor_loss_fwd(const float* const* cls_ptrs_host, const float* const* delta_ptrs_host,
                                       const float* const* anchor_ptrs_host, const long* anchor_pitch_host,
                                       const float* gt_bbox, const float* im_info, int N, int L, const long* hw_host,
                                       const long* w_host, int A, int K, int M, int top_n, float bbox_thr, float alpha,
                                       float gamma, const float* mean_host, const float* std_host, float* loss,
                                       int32_t* bags, void* workspace, size_t workspace_bytes, void* stream) {
  FaArgs a{};
  if (int e = fa_args(a, cls_ptrs_host, delta_ptrs_host, anchor_ptrs_host, anchor_pitch_host, gt_bbox, im_info, N, L,
                      hw_host, w_host, A, K, M, top_n, bbox_thr, alpha, gamma, mean_host, std_host, workspace,
                      workspace_bytes))
    return e;
  if (N == 0) return SD_OK;
  SD_REQUIRE(loss, "null pointer (loss)");
  a.loss = loss;
  a.bags_out = bags;
  hipStream_t st = (hipStream_t)stream;
  const dim3 rows(M, N), grid(a.nblocks, N);
  hipLaunchKernelGGL(fa_bag_kernel, rows, dim3(kFaT), 0, st, a);
  hipLaunchKernelGGL(fa_gtmax_kernel, grid, dim3(kFaT), 0, st, a);
  if (gamma == 2.0f)
    hipLaunchKernelGGL((fa_anchor_kernel<2, false>), grid, dim3(kFaT), 0, st, a);
  else
    hipLaunchKernelGGL((fa_anchor_kernel<-1, false>), grid, dim3(kFaT), 0, st, a);
  hipLaunchKernelGGL(fa_pos_kernel, rows, dim3(kWave), 0, st, a);
  hipLaunchKernelGGL(fa_finish_kernel, dim3(1), dim3(kFaT), 0, st, a);
  SD_LAUNCH_CHECK();
  note_dispatch("fa_bag_kernel grid=%dx%d + fa_gtmax_kernel + fa_anchor_kernel<%d,fwd> grid=%dx%d + fa_pos_kernel + "
                "fa_finish_kernel", M, N, gamma == 2.0f ? 2 : -1, a.nblocks, N);
  return SD_OK;
}

extern "C" int sd_free_anchor_loss_bwd(const float* const* cls_ptrs_host, const float* const* delta_ptrs_host,
                                       const float* const* anchor_ptrs_host, const long* anchor_pitch_host,
                                       const float* gt_bbox, const float* im_info, int N, int L, const long* hw_host,
                                       const long* w_host, int A, int K, int M, int top_n, float bbox_thr, float alpha,
                                       float gamma, const float* mean_host, const float* std_host, void* workspace,
                                       size_t workspace_bytes, float grad_scale, float* const* dcls_ptrs_host,
                                       float* const* ddelta_ptrs_host, void* stream) {
  FaArgs a{};
  if (int e = fa_args(a, cls_ptrs_host, delta_ptrs_host, anchor_ptrs_host, anchor_pitch_host, gt_bbox, im_info, N, L,
                      hw_host, w_host, A, K, M, top_n, bbox_thr, alpha, gamma, mean_host, std_host, workspace,
                      workspace_bytes))
    return e;
  SD_REQUIRE(dcls_ptrs_host && ddelta_ptrs_host, "null gradient table");
  for (int l = 0; l < L; ++l) {
    SD_REQUIRE(dcls_ptrs_host[l] && ddelta_ptrs_host[l], "null gradient pointer in level %d", l);
    a.dcls[l] = dcls_ptrs_host[l]; a.ddelta[l] = ddelta_ptrs_host[l];
  }
  if (N == 0) return SD_OK;
  a.grad_scale = grad_scale;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a.nblocks, N);
  if (gamma == 2.0f)
    hipLaunchKernelGGL((fa_anchor_kernel<2, true>), grid, dim3(kFaT), 0, st, a);
  else
    hipLaunchKernelGGL((fa_anchor_kernel<-1, true>), grid, dim3(kFaT), 0, st, a);
  const int P2 = sort_size(M * top_n, 128);
  const size_t lds = (size_t)P2 * sizeof(unsigned long long);
  // more than 64 KB of dynamic LDS (M * top_n > 8192) needs the kernel's limit raised: once per process, to the most
  // the kernel ever asks for, so that no later call -- one under stream capture among them -- touches the attribute
  static bool raised = false;
  if (lds > 64 * 1024 && !raised) {
    SD_HIP_CHECK(hipFuncSetAttribute((const void*)fa_sparse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)(kMaxSortKeys * sizeof(unsigned long long))));
    raised = true;
  }
  hipLaunchKernelGGL(fa_sparse_kernel, dim3(N), dim3(kFaT), lds, st, a, P2);
  SD_LAUNCH_CHECK();
  note_dispatch("fa_anchor_kernel<%d,bwd> grid=%dx%d + fa_sparse_kernel keys=%d", gamma == 2.0f ? 2 : -1, a.nblocks, N, P2);
  return SD_OK;
}
