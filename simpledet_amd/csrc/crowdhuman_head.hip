// The CrowdHuman double-prediction head's training side for gfx950, device resident.
//
// The reference runs it through Python CustomOps that copy to the host every step: `bbox_target`
// (models/crowdhuman/bbox_target.py:12-81, :121-178) and `doublebbox_target` (models/crowdhuman/bbox_sec_target.py:
// 13-120, :159-224) sample the RoIs in numpy -- IoU through the Cython bbox_overlaps, two np.random.choice(...,
// replace=False) per image on numpy's global MT19937 -- and `softmax_entropy` (softmax_entropy_op.py:8-31) runs four
// times inside DoublePredBboxHead.emd_loss (builder.py:254-306), a graph of ~30 element-wise nodes.
//
// sd_crowdhuman_target, four kernels on one stream, no host involvement:
//   ch_match    one thread per raw candidate row (the P proposals, then the M ground-truth rows): validity (y2 != 0 /
//               class != -1), IoU against the non-padding gt boxes held in LDS with the Cython arithmetic (rpn_iou),
//               mode 0: first maximum over the non-ignore rows; mode 1: per class first and second maximum, a class
//               replacing the running assignment only where it is strictly greater; the fg / bg flags
//   ch_lists    one workgroup per image: the ordered lists np.where would return (the candidate list of the reference is
//               the raw rows with the padding dropped, so the ORDER of the raw rows is the order of its indices)
//   ch_sample   ONE workgroup, images in order, mt19937.h's producer / consumer MT19937 (mt_consume): per non-empty list one
//               permutation(n), every accepted draw j_i recorded (n - 1 <= 4095 16-bit words per list)
//   ch_finish   one workgroup per image, one thread per output row: the wanted FRONT entry p of the permutation is
//               traced back through the recorded swaps (the swaps in reverse order of execution, i = 1 .. n - 1:
//               q == i -> j_i, q == j_i -> i), then labels, float32 box encoding, and the expanded rows written
//               coalesced from LDS.  Rows >= count are zero.
// sd_emd_loss_fwd / _bwd: one row per thread; the forward is one workgroup with a fixed-order sum.
#include "common.h"
#include "bbox_iou.h"
#include "loss_common.h"
#include "mt19937.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {

constexpr int kChMaxCand = 4096;   // P + M raw candidate rows per image
constexpr int kChMaxGt = 1024;     // M
constexpr int kChMaxRois = 1024;   // image_rois
constexpr int kChT = 256;

struct ChArgs {
  const float* prop;  // (B,P,4)
  const float* gt;    // (B,M,5)
  int B, P, M, N;     // N = P + M raw rows
  int mode, nrc, add_gt, S, fgq;
  int front;          // how ch_finish resolves the permutation's front: 0 trace (default), 1 LDS replay
  double fg_thr, bg_hi, bg_lo;
  float istd[4];
  int* mt;
  float *rois, *cls, *tgt, *wgt, *scls, *stgt, *swgt;
  int* count;
  // workspace, (B,N) each unless noted
  float* maxov;
  float* lab;            // assigned class
  int* gidx;             // raw gt row of the assigned box
  float* siou;           // mode 1: second maximum
  int* sidx;             // mode 1: raw gt row of the second box
  unsigned char* flag;   // bit 0 foreground, bit 1 background; 0 for a padding row
  int* fg_list;
  int* bg_list;
  int* counts;           // (B,2) list lengths, then one overrun word
  unsigned short* jrec;  // (B,2,kChMaxCand) accepted draws of the two permutations
};

// non-padding gt rows (class != -1), order preserved, into LDS: box, class, raw row; returns their number
template <int THREADS>
__device__ int ch_load_gt(const ChArgs& a, int img, float4* gbox, float* gcls, int* graw, int* wsum) {
  float4 g;
  float c;
  const int n_gt = block_compact_rows<THREADS>(
      a.M, wsum,
      [&](int j) {
        const float* p = a.gt + ((long)img * a.M + j) * 5;
        g = make_float4(p[0], p[1], p[2], p[3]);
        c = p[4];
        return c != -1.f;
      },
      [&](int j, int k) {
        gbox[k] = g;
        gcls[k] = c;
        graw[k] = j;
      });
  __syncthreads();
  return n_gt;
}

__global__ __launch_bounds__(kChT) void ch_match_kernel(ChArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 gbox[];
  __shared__ int wsum[kChT / kWave];
  float* gcls = reinterpret_cast<float*>(gbox + a.M);
  int* graw = reinterpret_cast<int*>(gcls + a.M);
  const int img = blockIdx.y;
  const int r = blockIdx.x * kChT + threadIdx.x;
  const int n_gt = ch_load_gt<kChT>(a, img, gbox, gcls, graw, wsum);
  if (r >= a.N) return;
  float4 box;
  bool valid;
  if (r < a.P) {
    const float* p = a.prop + ((long)img * a.P + r) * 4;
    box = make_float4(p[0], p[1], p[2], p[3]);
    valid = box.w != 0.f;                                   // y2 == 0 indicates padding
  } else {
    const float* p = a.gt + ((long)img * a.M + (r - a.P)) * 5;
    box = make_float4(p[0], p[1], p[2], p[3]);
    valid = a.add_gt && p[4] != -1.f;                       // every non-padding gt, the ignore rows included
  }
  float maxv = 0.f, cls = 0.f, m2 = 0.f;
  int idx = n_gt > 0 ? graw[0] : 0, idx2 = idx;
  bool fg = false, bg = false;
  if (valid) {
    if (a.mode == 0) {
      // bbox_target.py:20-35: the ignore rows leave the matching; first maximum; the label is the gt's class
      bool first = true;
      for (int j = 0; j < n_gt; ++j) {
        if (gcls[j] == -2.f) continue;
        const float o = rpn_iou(box, gbox[j]);
        if (first || o > maxv) {
          maxv = o; idx = graw[j]; cls = gcls[j];
          first = false;
        }
      }
      // (numpy 2: a float32 array against a python float compares in float32)
      fg = maxv >= (float)a.fg_thr;
      bg = maxv < (float)a.bg_hi && maxv >= (float)a.bg_lo;
    } else {
      // bbox_sec_target.py:19-58: ignore rows stay in place with class -1; per class the first maximum and, with
      // the winner set to -1, the first maximum of the rest (a lone gt: -1 at index 0 of the class = itself)
      for (int cid = 1; cid < a.nrc; ++cid) {
        float c1 = 0.f, c2 = -1.f;
        int i1 = -1, i2 = -1;
        for (int j = 0; j < n_gt; ++j) {
          if (gcls[j] != (float)cid) continue;
          const float o = rpn_iou(box, gbox[j]);
          if (i1 < 0) {
            c1 = o; i1 = j; i2 = j;
          } else if (o > c1) {
            c2 = c1; i2 = i1;      // the old winner is the first maximum of the rest: it lies before every equal
            c1 = o; i1 = j;
          } else if (o > c2) {
            c2 = o; i2 = j;
          }
        }
        if (i1 >= 0 && c1 > maxv) {   // strictly greater than the running maximum, which starts at 0
          cls = (float)cid; maxv = c1; idx = graw[i1]; idx2 = graw[i2]; m2 = c2;
        }
      }
      // (the running maxima are float64 arrays there: the thresholds compare in double)
      fg = (double)maxv >= a.fg_thr;
      bg = (double)maxv < a.bg_hi && (double)maxv >= a.bg_lo;
    }
  }
  const long o = (long)img * a.N + r;
  a.maxov[o] = maxv;
  a.lab[o] = cls;
  a.gidx[o] = idx;
  a.siou[o] = m2;
  a.sidx[o] = idx2;
  a.flag[o] = (unsigned char)((fg ? 1 : 0) | (bg ? 2 : 0));
}

// the ordered fg / bg lists of an image (one workgroup of 1024 threads per image)
__global__ __launch_bounds__(1024) void ch_lists_kernel(ChArgs a) {
  __shared__ int wcnt[2][16];
  const int img = blockIdx.x, tid = threadIdx.x;
  int run0 = 0, run1 = 0;
  for (int base = 0; base < a.N; base += 1024) {
    const int r = base + tid;
    const int f = r < a.N ? (int)a.flag[(long)img * a.N + r] : 0;
    const bool flag[2] = {(f & 1) != 0, (f & 2) != 0};
    int off[2] = {run0, run1}, tot[2];
    block_scan_flags<1024, 2>(flag, wcnt, off, tot);
    if (f & 1) a.fg_list[(long)img * a.N + off[0]] = r;
    if (f & 2) a.bg_list[(long)img * a.N + off[1]] = r;
    run0 += tot[0]; run1 += tot[1];
  }
  if (tid == 0) {
    a.counts[img * 2] = run0;
    a.counts[img * 2 + 1] = run1;
  }
}

// permutation(n) of the legacy RandomState: every accepted draw j of step i = n - 1 .. 1 goes to jrec[n - 1 - i]
// and the generator advances by exactly the draws numpy consumes.  n <= kChMaxCand: batch by batch.
__device__ void ch_sample(MtStream& m, int n, unsigned short* jrec, int lane) {
  mt_permutation_draws(m, n, lane, [](int, int) { return 1; },
                       [&](int step, unsigned v) { jrec[step] = (unsigned short)v; });
}

__global__ __launch_bounds__(kMtThreads) void ch_sample_kernel(ChArgs a) {
  const int lane = threadIdx.x & (kWave - 1);
  const int overrun = mt_consume(a.mt, a.B, [&](MtStream& m, int img) {
    // npr.choice(inds, size, replace=False) = inds[permutation(n)[:size]] whenever the list is not empty, whatever
    // the size (also 0, also n); permutation(1) draws nothing
    for (int l = 0; l < 2; ++l) {
      const int n = a.counts[img * 2 + l];
      if (n >= 2) ch_sample(m, n, a.jrec + ((long)img * 2 + l) * kChMaxCand, lane);
    }
  });
  if (overrun != kMtProducer && lane == 0) a.counts[a.B * 2] = overrun;
}

// bbox_transform_inv (operator_py/detectron_bbox_utils.py:205-219) on float32 boxes: every operation in float32
// (the python scalars are weak), the inverse stds as (float)(1.0 / std), ix * (gcx - ecx) / ew left to right
__device__ __forceinline__ void ch_encode(const float4 e, const float4 g, const float* istd, float* t) {
  const float ew = e.z - e.x + 1.0f, eh = e.w - e.y + 1.0f;
  const float ecx = e.x + 0.5f * ew, ecy = e.y + 0.5f * eh;
  const float gw = g.z - g.x + 1.0f, gh = g.w - g.y + 1.0f;
  const float gcx = g.x + 0.5f * gw, gcy = g.y + 0.5f * gh;
  t[0] = istd[0] * (gcx - ecx) / ew;
  t[1] = istd[1] * (gcy - ecy) / eh;
  t[2] = istd[2] * logf(gw / ew);
  t[3] = istd[3] * logf(gh / eh);
}

__global__ __launch_bounds__(1024) void ch_finish_kernel(ChArgs a) {
  __shared__ unsigned short jr[2][kChMaxCand];
  __shared__ float rowv[kChMaxRois][10];   // cls, target[4], second cls, second target[4] (the class already binarised)
  const int img = blockIdx.x, s = threadIdx.x;
  const int n_fg = a.counts[img * 2], n_bg = a.counts[img * 2 + 1];
  const int fg_this = iminr(a.fgq, n_fg);
  const int bg_this = iminr(a.S - fg_this, n_bg);
  const bool overrun = a.counts[a.B * 2] != 0;   // the generator stalled: the recorded draws are not valid
  const int cnt = overrun ? 0 : fg_this + bg_this;
  for (int l = 0; l < 2; ++l) {
    const int n = l ? n_bg : n_fg;
    const unsigned short* src = a.jrec + ((long)img * 2 + l) * kChMaxCand;
    for (int k = s; k < n - 1; k += 1024) jr[l][k] = src[k];
  }
  __syncthreads();
  // Variant (tuning crowdhuman_front = 1, measured against the trace by tools/crowdhuman_head_time.py): replay all
  // n - 1 swaps of either list on an LDS array, one lane per list, and read the front off it.  The array borrows
  // rowv, which is not written before the barrier behind the look-up.
  int q_replayed = 0;
  if (a.front == 1) {
    unsigned short* perm = reinterpret_cast<unsigned short*>(&rowv[0][0]);   // [2][kChMaxCand] = 16 KB of rowv's 40
    for (int k = s; k < 2 * kChMaxCand; k += 1024) perm[k] = (unsigned short)(k & (kChMaxCand - 1));
    __syncthreads();
    if ((s == 0 || s == kWave) && !overrun) {
      const int l = s / kWave, n = l ? n_bg : n_fg;
      unsigned short* pl = perm + l * kChMaxCand;
      for (int step = 0; step < n - 1; ++step) {
        const int i = n - 1 - step, j = iminr(jr[l][step], i);
        const unsigned short t = pl[i];
        pl[i] = pl[j];
        pl[j] = t;
      }
    }
    __syncthreads();
    if (s < cnt) q_replayed = perm[(s < fg_this ? 0 : 1) * kChMaxCand + (s < fg_this ? s : s - fg_this)];
    __syncthreads();
  }
  if (s < a.S) {
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f);
    float lab = 0.f, slab = 0.f;
    float* rv = rowv[s];
    for (int k = 0; k < 10; ++k) rv[k] = 0.f;
    if (s < cnt) {
      const int l = s < fg_this ? 0 : 1;
      const int n = l ? n_bg : n_fg;
      int q = l ? s - fg_this : s;
      const unsigned short* j = jr[l];
      if (a.front == 1) {
        q = q_replayed;
      } else {
        for (int i = 1; i < n; ++i) {   // the swaps backwards: where the entry at q came from
          const int ji = j[n - 1 - i];
          q = q == i ? ji : q == ji ? i : q;
        }
      }
      q = iminr(q, n - 1);
      const long o = (long)img * a.N + (l ? a.bg_list : a.fg_list)[(long)img * a.N + q];
      const int raw = (int)(o - (long)img * a.N);
      const float* bp = raw < a.P ? a.prop + ((long)img * a.P + raw) * 4 : a.gt + ((long)img * a.M + (raw - a.P)) * 5;
      box = make_float4(bp[0], bp[1], bp[2], bp[3]);
      const float c = a.lab[o];
      lab = l ? 0.f : c;                                    // background rows get label 0
      const float* gp = a.gt + ((long)img * a.M + a.gidx[o]) * 5;
      ch_encode(box, make_float4(gp[0], gp[1], gp[2], gp[3]), a.istd, rv + 1);
      rv[0] = a.nrc == 2 ? (lab > 0.f ? 1.f : 0.f) : lab;
      if (a.mode == 1) {
        slab = (double)a.siou[o] < a.fg_thr ? 0.f : c;      // :99-103: the assigned class unless the second IoU is low
        const float* sp = a.gt + ((long)img * a.M + a.sidx[o]) * 5;
        ch_encode(box, make_float4(sp[0], sp[1], sp[2], sp[3]), a.istd, rv + 6);
        rv[5] = a.nrc == 2 ? (slab > 0.f ? 1.f : 0.f) : slab;
      }
    }
    const long ro = (long)img * a.S + s;
    a.rois[ro * 4] = box.x; a.rois[ro * 4 + 1] = box.y; a.rois[ro * 4 + 2] = box.z; a.rois[ro * 4 + 3] = box.w;
    a.cls[ro] = lab;
    if (a.mode == 1) a.scls[ro] = slab;
  }
  __syncthreads();
  // _expand_bbox_targets: columns 4c .. 4c + 3 of class c > 0, everything else zero
  const int W = 4 * a.nrc;
  for (int e = s; e < a.S * W; e += 1024) {
    const int row = e / W, col = e - row * W;
    const float* rv = rowv[row];
    const long o = ((long)img * a.S + row) * W + col;
    for (int h = 0; h < (a.mode == 1 ? 2 : 1); ++h) {
      const float c = rv[5 * h];
      const bool on = c > 0.f && (int)c < a.nrc && (col >> 2) == (int)c;
      (h ? a.stgt : a.tgt)[o] = on ? rv[5 * h + 1 + (col & 3)] : 0.f;
      (h ? a.swgt : a.wgt)[o] = on ? 1.f : 0.f;
    }
  }
  if (s == 0) a.count[img] = overrun ? -1 : cnt;
}

static size_t ch_layout(int B, int N, ChArgs* a, void* workspace) {
  WsCarver c(workspace);
  const size_t bn = (size_t)B * N;
  a->maxov = c.take<float>(bn * 4);
  a->lab = c.take<float>(bn * 4);
  a->gidx = c.take<int>(bn * 4);
  a->siou = c.take<float>(bn * 4);
  a->sidx = c.take<int>(bn * 4);
  a->flag = c.take<unsigned char>(bn);
  a->fg_list = c.take<int>(bn * 4);
  a->bg_list = c.take<int>(bn * 4);
  a->counts = c.take<int>((size_t)(B * 2 + 1) * 4);
  a->jrec = c.take<unsigned short>((size_t)B * 2 * kChMaxCand * 2);
  return c.need();
}

// ---- EMD loss (builder.py:254-306) ------------------------------------------------------------------
struct EmdArgs {
  const float *x1, *x2;   // cls_logit, cls_sec_logit (R,K)
  const float *y1, *y2;   // cls_label, cls_sec_label (R)
  const float *d1, *d2, *t1, *t2, *w1, *w2;   // (R,D)
  int R, K, D;
  float bsq, ibsq, g;     // sigma^2, 1 / sigma^2, grad_scale / R
  float* loss;
  int* pairing;
  float *gx1, *gx2, *gd1, *gd2;
};

// the column a float label names (mx.nd.one_hot: none outside [0, K))
__device__ __forceinline__ int emd_col(float y, int K) { return y >= 0.f && y < (float)K ? (int)y : -1; }

// softmax of a row: its maximum and the sum of exp(x - max)
__device__ __forceinline__ void emd_softmax(const float* x, int K, float& mx, float& sum) {
  mx = x[0];
  for (int k = 1; k < K; ++k) mx = fmaxr(mx, x[k]);
  sum = 0.f;
  for (int k = 0; k < K; ++k) sum += expf(x[k] - mx);
}
// softmax_entropy's forward summed over the row: -log(softmax + 1e-10) at the label, 0 without one
__device__ __forceinline__ float emd_ce(const float* x, float mx, float sum, int col) {
  return col < 0 ? 0.f : -logf(expf(x[col] - mx) / sum + 1e-10f);
}

// the two sums of a row; returns the pairing that wins (1: L1 <= L2, MXNet's _backward_minimum gives ties to the left)
__device__ __forceinline__ int emd_row(const EmdArgs& a, int r, float& lmin) {
  const float* x1 = a.x1 + (long)r * a.K;
  const float* x2 = a.x2 + (long)r * a.K;
  const int c1 = emd_col(a.y1[r], a.K), c2 = emd_col(a.y2[r], a.K);
  float m1, s1, m2, s2;
  emd_softmax(x1, a.K, m1, s1);
  emd_softmax(x2, a.K, m2, s2);
  const float cls1 = emd_ce(x1, m1, s1, c1) + emd_ce(x2, m2, s2, c2);
  const float cls2 = emd_ce(x1, m1, s1, c2) + emd_ce(x2, m2, s2, c1);
  const long o = (long)r * a.D;
  float reg1 = 0.f, reg2 = 0.f;
  for (int d = 0; d < a.D; ++d) {
    const float p1 = a.d1[o + d], p2 = a.d2[o + d], t1 = a.t1[o + d], t2 = a.t2[o + d];
    const float w1 = a.w1[o + d], w2 = a.w2[o + d];
    reg1 += w1 * smooth_l1(p1 - t1, a.bsq, a.ibsq) + w2 * smooth_l1(p2 - t2, a.bsq, a.ibsq);
    reg2 += w2 * smooth_l1(p1 - t2, a.bsq, a.ibsq) + w1 * smooth_l1(p2 - t1, a.bsq, a.ibsq);
  }
  const float L1 = cls1 + reg1, L2 = cls2 + reg2;
  const bool first = L1 <= L2;
  lmin = first ? L1 : L2;
  return first ? 1 : 2;
}

// ONE workgroup: thread t sums rows t, t + 1024, ... in order, the waves' sums are added in order
__global__ __launch_bounds__(1024) void emd_loss_fwd_kernel(EmdArgs a) {
  __shared__ float wsum[16];
  const int tid = threadIdx.x;
  float acc = 0.f;
  for (int r = tid; r < a.R; r += 1024) {
    float l;
    const int p = emd_row(a, r, l);
    acc += l;
    if (a.pairing) a.pairing[r] = p;
  }
  const float w = wave_sum_f32(acc);
  if ((tid & 63) == 0) wsum[tid >> 6] = w;
  __syncthreads();
  if (tid == 0) {
    float t = 0.f;
    for (int k = 0; k < 16; ++k) t += wsum[k];
    a.loss[0] = t / (float)a.R;
  }
}

__global__ __launch_bounds__(kChT) void emd_loss_bwd_kernel(EmdArgs a) {
  const int r = blockIdx.x * kChT + threadIdx.x;
  if (r >= a.R) return;
  float l;
  const bool first = emd_row(a, r, l) == 1;
  // softmax_entropy's backward: (softmax - onehot) * out_grad, the head paired with the label the winner gave it
  const int c1 = emd_col(a.y1[r], a.K), c2 = emd_col(a.y2[r], a.K);
  for (int h = 0; h < 2; ++h) {
    const float* x = (h ? a.x2 : a.x1) + (long)r * a.K;
    float* gx = (h ? a.gx2 : a.gx1) + (long)r * a.K;
    const int col = (h == 0) == first ? c1 : c2;
    float mx, sum;
    emd_softmax(x, a.K, mx, sum);
    for (int k = 0; k < a.K; ++k) gx[k] = (expf(x[k] - mx) / sum - (k == col ? 1.f : 0.f)) * a.g;
  }
  const long o = (long)r * a.D;
  for (int d = 0; d < a.D; ++d) {
    const float p1 = a.d1[o + d], p2 = a.d2[o + d], t1 = a.t1[o + d], t2 = a.t2[o + d];
    const float w1 = a.w1[o + d], w2 = a.w2[o + d];
    a.gd1[o + d] = first ? (a.g * w1) * smooth_l1_grad(p1 - t1, a.bsq, a.ibsq)
                         : (a.g * w2) * smooth_l1_grad(p1 - t2, a.bsq, a.ibsq);
    a.gd2[o + d] = first ? (a.g * w2) * smooth_l1_grad(p2 - t2, a.bsq, a.ibsq)
                         : (a.g * w1) * smooth_l1_grad(p2 - t1, a.bsq, a.ibsq);
  }
}

static int emd_check(const EmdArgs& a, float sigma) {
  SD_REQUIRE(a.R >= 0 && a.K >= 1 && a.D >= 0, "bad R / K / D");
  SD_REQUIRE(sigma > 0.f, "smooth_l1_scalar must be positive");
  if ((long)a.R * (a.K > a.D ? a.K : a.D) > 2147483647L)
    return fail(SD_ERR_UNSUPPORTED, "emd_loss: more than 2^31 - 1 elements");
  if (a.R == 0) return SD_OK;
  SD_REQUIRE(a.x1 && a.x2 && a.y1 && a.y2, "null pointer");
  SD_REQUIRE(a.D == 0 || (a.d1 && a.d2 && a.t1 && a.t2 && a.w1 && a.w2), "null pointer");
  return SD_OK;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_crowdhuman_target_workspace_bytes(int B, int P, int M) {
  if (B <= 0 || P < 0 || M < 0) return 256;
  ChArgs a{};
  return ch_layout(B, P + M, &a, nullptr) + 256;
}

extern "C" int sd_crowdhuman_target(const float* proposal, const float* gt_bbox, int B, int P, int M, int mode,
                                    const sd_crowdhuman_target_param* param_host, int32_t* mt_state,
                                    float* sampled_proposal, float* bbox_cls, float* bbox_target,
                                    float* bbox_target_weight, float* bbox_sec_cls, float* bbox_sec_target,
                                    float* bbox_sec_target_weight, int32_t* count, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  SD_REQUIRE(param_host, "param is null");
  const sd_crowdhuman_target_param& p = *param_host;
  SD_REQUIRE(mode == 0 || mode == 1, "mode must be 0 (bbox_target) or 1 (doublebbox_target)");
  SD_REQUIRE(B >= 0 && P >= 0 && M >= 1, "bad B / P / M");
  SD_REQUIRE(M <= kChMaxGt && P + M <= kChMaxCand, "M=%d > %d or P + M = %d > %d", M, kChMaxGt, P + M, kChMaxCand);
  SD_REQUIRE(p.image_rois >= 1 && p.image_rois <= kChMaxRois, "image_rois outside [1,%d]", kChMaxRois);
  SD_REQUIRE(p.num_reg_class >= 2 && p.num_reg_class <= 1024, "num_reg_class outside [2,1024]");
  SD_REQUIRE(p.fg_fraction >= 0.0 && p.fg_fraction <= 1.0, "fg_fraction outside [0,1]");
  for (int k = 0; k < 4; ++k) SD_REQUIRE(p.bbox_target_std[k] != 0.0, "bbox_target_std[%d] is zero", k);
  if (B == 0) return SD_OK;
  SD_REQUIRE(proposal || P == 0, "null pointer");
  SD_REQUIRE(gt_bbox && mt_state && sampled_proposal && bbox_cls && bbox_target && bbox_target_weight && count,
             "null pointer");
  SD_REQUIRE(mode == 0 || (bbox_sec_cls && bbox_sec_target && bbox_sec_target_weight), "null pointer (second outputs)");
  ChArgs a{};
  a.prop = proposal; a.gt = gt_bbox; a.B = B; a.P = P; a.M = M; a.N = P + M;
  a.mode = mode; a.nrc = p.num_reg_class; a.add_gt = p.add_gt_to_proposal ? 1 : 0; a.S = p.image_rois;
  a.fgq = (int)nearbyint(p.fg_fraction * (double)p.image_rois);   // int(np.round(.)): half to even
  a.fg_thr = p.fg_thresh; a.bg_hi = p.bg_thresh_hi; a.bg_lo = p.bg_thresh_lo;
  for (int k = 0; k < 4; ++k) a.istd[k] = (float)(1.0 / p.bbox_target_std[k]);
  a.mt = mt_state;
  a.front = tuning(Knob::crowdhuman_front) == 1 ? 1 : 0;
  a.rois = sampled_proposal; a.cls = bbox_cls; a.tgt = bbox_target; a.wgt = bbox_target_weight;
  a.scls = bbox_sec_cls; a.stgt = bbox_sec_target; a.swgt = bbox_sec_target_weight; a.count = count;
  const size_t need = ch_layout(B, a.N, &a, workspace);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "crowdhuman_target workspace too small: %zu < %zu bytes", workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const size_t lds = (size_t)M * (sizeof(float4) + sizeof(float) + sizeof(int));
  // (profiling build only: tools/crowdhuman_head_time.py times the chain cut short to apportion it)
  const int stop = SD_PROF_TUNING(crowdhuman_target_stop);
  const int nk = stop >= 1 && stop <= 3 ? stop : 4;
  hipLaunchKernelGGL(ch_match_kernel, dim3(cdiv(a.N, kChT), B), dim3(kChT), lds, st, a);
  if (nk >= 2) hipLaunchKernelGGL(ch_lists_kernel, dim3(B), dim3(1024), 0, st, a);
  if (nk >= 3) hipLaunchKernelGGL(ch_sample_kernel, dim3(1), dim3(kMtThreads), 0, st, a);
  if (nk >= 4) hipLaunchKernelGGL(ch_finish_kernel, dim3(B), dim3(1024), 0, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_emd_loss_fwd(const float* cls_logit, const float* cls_sec_logit, const float* cls_label,
                               const float* cls_sec_label, const float* bbox_delta, const float* bbox_sec_delta,
                               const float* bbox_target, const float* bbox_sec_target, const float* bbox_weight,
                               const float* bbox_sec_weight, int R, int K, int D, float smooth_l1_scalar,
                               float* loss, int32_t* pairing, void* stream) {
  EmdArgs a{};
  a.x1 = cls_logit; a.x2 = cls_sec_logit; a.y1 = cls_label; a.y2 = cls_sec_label;
  a.d1 = bbox_delta; a.d2 = bbox_sec_delta; a.t1 = bbox_target; a.t2 = bbox_sec_target;
  a.w1 = bbox_weight; a.w2 = bbox_sec_weight; a.R = R; a.K = K; a.D = D;
  if (int e = emd_check(a, smooth_l1_scalar)) return e;
  if (R == 0) return SD_OK;
  SD_REQUIRE(loss, "null pointer");
  a.bsq = smooth_l1_scalar * smooth_l1_scalar; a.ibsq = 1.0f / a.bsq;
  a.loss = loss; a.pairing = pairing;
  hipLaunchKernelGGL(emd_loss_fwd_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" int sd_emd_loss_bwd(const float* cls_logit, const float* cls_sec_logit, const float* cls_label,
                               const float* cls_sec_label, const float* bbox_delta, const float* bbox_sec_delta,
                               const float* bbox_target, const float* bbox_sec_target, const float* bbox_weight,
                               const float* bbox_sec_weight, int R, int K, int D, float smooth_l1_scalar,
                               float grad_scale, float* d_cls_logit, float* d_cls_sec_logit, float* d_bbox_delta,
                               float* d_bbox_sec_delta, void* stream) {
  EmdArgs a{};
  a.x1 = cls_logit; a.x2 = cls_sec_logit; a.y1 = cls_label; a.y2 = cls_sec_label;
  a.d1 = bbox_delta; a.d2 = bbox_sec_delta; a.t1 = bbox_target; a.t2 = bbox_sec_target;
  a.w1 = bbox_weight; a.w2 = bbox_sec_weight; a.R = R; a.K = K; a.D = D;
  if (int e = emd_check(a, smooth_l1_scalar)) return e;
  if (R == 0) return SD_OK;
  SD_REQUIRE(d_cls_logit && d_cls_sec_logit && (D == 0 || (d_bbox_delta && d_bbox_sec_delta)), "null pointer");
  a.bsq = smooth_l1_scalar * smooth_l1_scalar; a.ibsq = 1.0f / a.bsq;
  a.g = grad_scale / (float)R;
  a.gx1 = d_cls_logit; a.gx2 = d_cls_sec_logit; a.gd1 = d_bbox_delta; a.gd2 = d_bbox_sec_delta;
  hipLaunchKernelGGL(emd_loss_bwd_kernel, dim3(cdiv(R, kChT)), dim3(kChT), 0, (hipStream_t)stream, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
