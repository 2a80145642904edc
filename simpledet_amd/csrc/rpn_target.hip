// RPN anchor-target assignment for gfx950, device resident.
//
// The reference computes these targets in its data loader, per image, in numpy on the host
// (core/detection_input.py AnchorTarget2D :345-565, models/FPN/input.py PyramidAnchorTarget2D
// :9-146, IoU operator_py/cython/bbox.pyx:31-72, box encoding operator_py/bbox_transform.py:52-77)
// and it is the loader bottleneck it works around with a TVM op elsewhere.  Here the whole
// assignment runs on the GPU and reproduces the reference bit for bit, INCLUDING the random
// subsampling: np.random.choice(inds, size, replace=False) of the legacy RandomState is
// inds[permutation(n)[:size]], permutation = Fisher-Yates from the top over MT19937 with masked
// rejection sampling, and the generator state lives in device memory and is advanced exactly as
// numpy would advance it (624 key words + position).
//
// Kernels (one stream, no host involvement):
//   rpn_overlap   one thread per anchor: the anchor box from (level, y, x, a), the inside-image
//                 test, IoU against the valid gt boxes held in LDS with the Cython arithmetic
//                 (float ops, the literal "+ 1" as a double add), first-maximum arg-max; per-gt
//                 maximum over the valid anchors through LDS then global atomic max on the bits
//   rpn_label     label -1/0/1 per anchor (:462-477, including the reference's own looseness: every
//                 anchor whose overlap EQUALS a gt's maximum and is >= min_pos_thr is positive --
//                 with min_pos_thr = 0 a gt box nothing overlaps makes every valid anchor positive),
//                 per-block fg / bg counts; rpn_scan + rpn_lists (block_scan_flags, wg_common.h) turn them
//                 into the ordered index lists np.where would return
//   rpn_sample    ONE workgroup, images in order (the generator state carries from image to image); round 6: five
//                 waves that meet through LDS counters only --
//                 * four PRODUCER waves make MT19937's raw sequence (X[j] = X[j-227] ^ tw(X[j-624], X[j-623]):
//                   227 consecutive words are independent, and two steps fit between hand-shakes) into an LDS ring,
//                   raw and tempered, as far ahead as the ring allows
//                 * the CONSUMER wave takes up to 1024 draws per dependent step: candidates (v & mask <= i) by
//                   ballot, sure accepts by a rank bound, the handful of unsettled ones in order with their exact
//                   rank; batch by batch (ballot / popcount fixed point, exact) where the rejection mask is small,
//                   near a mask segment's end and inside the recorded swaps
//                 * only the last `keep` positions of the permutation survive, and they are final
//                   after the first `keep` swaps: those swaps are replayed on a sparse array
//                 so ~330 k dependent draws per image cost ~700 wave steps (2.7 -> 1.4 ms for two images; the rest is
//                 the single consumer wave's ~12 clocks per instruction)
//   rpn_encode    final label, box deltas in double (nonlinear_transform on float64 anchors),
//                 weights; written either in flat all-anchor order or in the loader's final
//                 (A, sum h*w) / (4A, sum h*w) layout
#include "common.h"
#include "bbox_iou.h"
#include "mt19937.h"
#include "wg_common.h"
#include "../../include/simpledet_ops.h"
#include <math.h>

namespace sd {

constexpr int kRpnMaxLvl = SD_MAX_FPN_LEVELS;
constexpr int kRpnMaxA = 16;  // (kernel arguments are limited to 4 KB: base anchors travel in them)

struct RpnArgs {
  sd_rpn_target_param p;
  float base[kRpnMaxLvl][kRpnMaxA][4];  // base anchors per level (exactly representable)
  int num_fg;                           // int(pos_fraction * image_anchor), evaluated in double
  int A;                                // anchors per location
  int N;                                // anchors per image
  int sumHW;
  const float* im_info;  // (B,3)
  const float* gt;       // (B,M,G)
  int B, M, G;
  int* mt;               // 625 words
  float* cls;
  float* tgt;
  float* wgt;
  int layout;
  // workspace
  float* maxov;          // (B,N)
  int* argmax;           // (B,N)
  signed char* label;    // (B,N)
  unsigned char* keep;   // (B,N) survivors of the subsampling
  unsigned* gtmax;       // (B,M) float bits
  int* blk;              // (B, nblk, 2) fg / bg counts, then exclusive offsets
  int* fg_list;          // (B,N)
  int* bg_list;          // (B,N)
  int* counts;           // (B,4): n_fg, n_bg, fg_sampled, bg_sampled
  int nblk;
  const double* base64;  // retina: (nlvl, kRpnMaxA, 4) base anchors in double, device memory
};

struct AnchorRef {
  float4 box;
  int lvl, y, x, a, fh, fw, hwoff;
};

// anchor n of an image whose orientation is `portrait` (h >= w: fh = long, fw = short).
// F64 (retina): the reference's anchors are float64 = float32 grid + float64 base (detection_input.py:409-415),
// and RetinaNet's scales 4 * 2^(k/3) make the base irrational: the float64 box goes to `dbox` (validity test and
// encoding), and r.box is its float32 rounding, the `valid_anchor.astype(np.float32)` the IoU sees.
template <bool F64 = false>
__device__ __forceinline__ AnchorRef rpn_anchor(const RpnArgs& a, int n, bool portrait, double* dbox = nullptr) {
  AnchorRef r;
  int off = 0, hwoff = 0, l = 0, fh = 0, fw = 0;
  for (; l < a.p.nlvl; ++l) {
    fh = portrait ? a.p.long_side[l] : a.p.short_side[l];
    fw = portrait ? a.p.short_side[l] : a.p.long_side[l];
    const int cnt = fh * fw * a.A;
    if (n < off + cnt) break;
    off += cnt;
    hwoff += fh * fw;
  }
  const int idx = n - off;
  r.lvl = l; r.fh = fh; r.fw = fw; r.hwoff = hwoff;
  r.a = idx % a.A;
  const int cell = idx / a.A;
  r.x = cell % fw;
  r.y = cell / fw;
  const float sx = (float)r.x * (float)a.p.stride[l], sy = (float)r.y * (float)a.p.stride[l];
  if (F64) {
    const double* b = a.base64 + (l * kRpnMaxA + r.a) * 4;
    dbox[0] = (double)sx + b[0]; dbox[1] = (double)sy + b[1];
    dbox[2] = (double)sx + b[2]; dbox[3] = (double)sy + b[3];
    r.box = make_float4((float)dbox[0], (float)dbox[1], (float)dbox[2], (float)dbox[3]);
    return r;
  }
  const float* b = a.base[l][r.a];
  r.box = make_float4(sx + b[0], sy + b[1], sx + b[2], sy + b[3]);
  return r;
}

// valid gt rows (gt[:,0] != -1), order preserved, into LDS; returns their number (all threads)
template <int THREADS>
__device__ int rpn_load_gt(const RpnArgs& a, int img, float4* gbox, int* wsum, float* gcls = nullptr) {
  float4 g;
  const int n_gt = block_compact_rows<THREADS>(
      a.M, wsum,
      [&](int j) {
        const float* p = a.gt + ((long)img * a.M + j) * a.G;
        g = make_float4(p[0], p[1], p[2], p[3]);
        return g.x != -1.f;
      },
      [&](int j, int k) {
        gbox[k] = g;
        if (gcls) gcls[k] = a.gt[((long)img * a.M + j) * a.G + 4];  // (retina: the class column, G = 5)
      });
  __syncthreads();
  return n_gt;
}

__device__ __forceinline__ bool rpn_valid(const RpnArgs& a, const float4 b, float h, float w) {
  const float ab = (float)a.p.allowed_border;
  return b.x >= -ab && b.y >= -ab && b.z < w + ab && b.w < h + ab;
}

// float64 anchors against float32 bounds (w + allowed_border is a float32 sum in numpy, then promoted)
__device__ __forceinline__ bool rpn_valid64(const RpnArgs& a, const double* b, float h, float w) {
  const float ab = (float)a.p.allowed_border;
  return b[0] >= (double)-ab && b[1] >= (double)-ab && b[2] < (double)(w + ab) && b[3] < (double)(h + ab);
}

constexpr int kRpnT = 256;

template <bool F64 = false>
__global__ __launch_bounds__(kRpnT) void rpn_overlap_kernel(RpnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 gbox[];
  __shared__ int wsum[kRpnT / kWave];
  unsigned* gmax = reinterpret_cast<unsigned*>(gbox + a.M);
  const int img = blockIdx.y, tid = threadIdx.x;
  const int n = blockIdx.x * kRpnT + tid;
  const int n_gt = rpn_load_gt<kRpnT>(a, img, gbox, wsum);
  for (int j = tid; j < n_gt; j += kRpnT) gmax[j] = 0u;
  __syncthreads();
  const float h = a.im_info[img * 3], w = a.im_info[img * 3 + 1];
  if (n < a.N) {
    double d[4];
    const AnchorRef r = rpn_anchor<F64>(a, n, h >= w, d);
    float maxv = 0.f;
    int maxi = 0;
    if (F64 ? rpn_valid64(a, d, h, w) : rpn_valid(a, r.box, h, w)) {
      for (int j = 0; j < n_gt; ++j) {
        const float o = rpn_iou(r.box, gbox[j]);
        if (j == 0 || o > maxv) {  // np.argmax: first maximum
          maxv = o;
          maxi = j;
        }
        if (o > 0.f) atomicMax(&gmax[j], __float_as_uint(o));
      }
    }
    a.maxov[(long)img * a.N + n] = maxv;
    a.argmax[(long)img * a.N + n] = maxi;
    a.keep[(long)img * a.N + n] = 0;
  }
  __syncthreads();
  for (int j = tid; j < n_gt; j += kRpnT)
    if (gmax[j]) atomicMax(&a.gtmax[(long)img * a.M + j], gmax[j]);
}

__global__ __launch_bounds__(kRpnT) void rpn_label_kernel(RpnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 gbox[];
  __shared__ int wsum[kRpnT / kWave];
  __shared__ int cnt[2];
  const int img = blockIdx.y, tid = threadIdx.x;
  const int n = blockIdx.x * kRpnT + tid;
  const int n_gt = rpn_load_gt<kRpnT>(a, img, gbox, wsum);
  if (tid < 2) cnt[tid] = 0;
  __syncthreads();
  const float h = a.im_info[img * 3], w = a.im_info[img * 3 + 1];
  int lab = -1;
  if (n < a.N) {
    const AnchorRef r = rpn_anchor(a, n, h >= w);
    if (rpn_valid(a, r.box, h, w)) {
      if (n_gt > 0) {
        const float mo = a.maxov[(long)img * a.N + n];
        if (mo < a.p.neg_thr) lab = 0;
        bool is_gt_arg = false;
        for (int j = 0; j < n_gt; ++j) {
          const float o = rpn_iou(r.box, gbox[j]);
          const float gm = __uint_as_float(a.gtmax[(long)img * a.M + j]);
          if (o == gm && o >= a.p.min_pos_thr) is_gt_arg = true;
        }
        if (is_gt_arg) lab = 1;
        if (mo >= a.p.pos_thr) lab = 1;
      } else {
        lab = 0;
      }
    }
    a.label[(long)img * a.N + n] = (signed char)lab;
  }
  const unsigned long long mf = __ballot(lab == 1), mb = __ballot(lab == 0);
  if ((tid & (kWave - 1)) == 0) {
    atomicAdd(&cnt[0], __popcll(mf));
    atomicAdd(&cnt[1], __popcll(mb));
  }
  __syncthreads();
  if (tid < 2) a.blk[((long)img * a.nblk + blockIdx.x) * 2 + tid] = cnt[tid];
}

// exclusive scan of the per-block counts (one workgroup per image); totals into counts
__global__ __launch_bounds__(1024) void rpn_scan_kernel(RpnArgs a) {
  __shared__ int wtot[2][16];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int run[2] = {0, 0};
  for (int base = 0; base < a.nblk; base += 1024) {
    const int b = base + tid;
    int v[2] = {0, 0};
    if (b < a.nblk) {
      v[0] = a.blk[((long)img * a.nblk + b) * 2];
      v[1] = a.blk[((long)img * a.nblk + b) * 2 + 1];
    }
    int incl[2] = {v[0], v[1]};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t0 = __shfl_up(incl[0], o), t1 = __shfl_up(incl[1], o);
      if (lane >= o) { incl[0] += t0; incl[1] += t1; }
    }
    __syncthreads();
    if (lane == 63) { wtot[0][wave] = incl[0]; wtot[1][wave] = incl[1]; }
    __syncthreads();
    int off[2] = {run[0], run[1]}, tot[2] = {0, 0};
    for (int wv = 0; wv < 16; ++wv) {
      if (wv < wave) { off[0] += wtot[0][wv]; off[1] += wtot[1][wv]; }
      tot[0] += wtot[0][wv]; tot[1] += wtot[1][wv];
    }
    if (b < a.nblk) {
      a.blk[((long)img * a.nblk + b) * 2] = off[0] + incl[0] - v[0];
      a.blk[((long)img * a.nblk + b) * 2 + 1] = off[1] + incl[1] - v[1];
    }
    run[0] += tot[0]; run[1] += tot[1];
  }
  if (tid == 0) {
    a.counts[img * 4] = run[0];
    a.counts[img * 4 + 1] = run[1];
    a.counts[img * 4 + 2] = 0;
    a.counts[img * 4 + 3] = 0;
  }
}

__global__ __launch_bounds__(kRpnT) void rpn_lists_kernel(RpnArgs a) {
  __shared__ int wcnt[2][kRpnT / kWave];
  const int img = blockIdx.y;
  const int n = blockIdx.x * kRpnT + threadIdx.x;
  const int lab = n < a.N ? (int)a.label[(long)img * a.N + n] : -1;
  const bool flag[2] = {lab == 1, lab == 0};
  int off[2] = {0, 0}, tot[2];
  block_scan_flags<kRpnT, 2, false>(flag, wcnt, off, tot);   // (one scan per workgroup: no barrier in front)
  const int* blk = a.blk + ((long)img * a.nblk + blockIdx.x) * 2;   // this workgroup's offsets from rpn_scan
  if (lab == 1) a.fg_list[(long)img * a.N + blk[0] + off[0]] = n;
  if (lab == 0) a.bg_list[(long)img * a.N + blk[1] + off[1]] = n;
}

// ---- MT19937 (numpy legacy RandomState): producer waves and a consumer wave, mt19937.h -------------
constexpr int kRpnMaxKeep = 1024;

// permutation(n) of the legacy RandomState, of which only the last `keep` entries are wanted
// (choice(inds, n - keep, replace=False) disables the FIRST n - keep): fills surv[0..keep) with the
// list positions that survive and advances the generator by exactly the draws numpy consumes.
__device__ void rpn_sample(MtStream& m, int n, int keep, int* jrec, int* hp, int* hv, int* surv, int lane) {
  // Trip size by mask: the unsettled candidates of an L-draw trip number ~L * (L / 2) / mask -- a handful for 1024
  // draws from mask 2^17 on (where four fifths of the draws are spent), for 512 from 2^15, for 128 from 2^11;
  // below that, and inside the recorded swaps, batch by batch.
  auto trip_size = [&](int i, int step) {
    const bool past = step >= keep;
    return !past || i < 1024 ? 1 : i < 16384 ? 2 : i < 65536 ? 8 : 16;
  };
  auto record = [&](int step, unsigned v) {
    if (step < keep) jrec[step] = (int)v;
  };
  if (!mt_permutation_draws(m, n, lane, trip_size, record)) return;
  wave_lds_sync();
  // replay the first `keep` swaps on a sparse array: position p holds p unless a swap wrote it
  for (int s = 0; s < keep; ++s) {
    const int is = n - 1 - s, js = jrec[s];
    int vi = is, vj = js, fi = -1, fj = -1;
    for (int base = ((s - 1) / kWave) * kWave; base >= 0 && s > 0; base -= kWave) {
      const int e = base + lane;
      const int hpe = e < s ? hp[e] : -2;
      if (fi < 0) {
        const unsigned long long mi = __ballot(hpe == is);
        if (mi) fi = base + 63 - __clzll((long long)mi);
      }
      if (fj < 0) {
        const unsigned long long mj = __ballot(hpe == js);
        if (mj) fj = base + 63 - __clzll((long long)mj);
      }
      if (fi >= 0 && fj >= 0) break;
    }
    if (fi >= 0) vi = hv[fi];
    if (fj >= 0) vj = hv[fj];
    if (lane == 0) {
      surv[s] = vj;  // position is is final: it holds what position js held
      hp[s] = js;    // ... and js now holds what is held
      hv[s] = vi;
    }
    wave_lds_sync();
  }
}

__global__ __launch_bounds__(kMtThreads) void rpn_sample_kernel(RpnArgs a) {
  __shared__ int jrec[kRpnMaxKeep], hp[kRpnMaxKeep], hv[kRpnMaxKeep], surv[kRpnMaxKeep];
  const int lane = threadIdx.x & (kWave - 1);
  const int num = a.p.image_anchor;
  const int overrun = mt_consume(a.mt, a.B, [&](MtStream& m, int img) {
    int* c = a.counts + img * 4;
    const int n_fg = c[0], n_bg = c[1];
    int fg_left = n_fg;
    if (n_fg > a.num_fg) {
      rpn_sample(m, n_fg, a.num_fg, jrec, hp, hv, surv, lane);
      for (int s = lane; s < a.num_fg; s += kWave)
        a.keep[(long)img * a.N + a.fg_list[(long)img * a.N + surv[s]]] = 1;
      if (lane == 0) c[2] = 1;
      fg_left = a.num_fg;
    }
    const int num_bg = num - fg_left;
    if (n_bg > num_bg) {
      if (num_bg > 0) {
        rpn_sample(m, n_bg, num_bg, jrec, hp, hv, surv, lane);
        for (int s = lane; s < num_bg; s += kWave)
          a.keep[(long)img * a.N + a.bg_list[(long)img * a.N + surv[s]]] = 1;
      } else {
        rpn_sample(m, n_bg, 0, jrec, hp, hv, surv, lane);  // every bg is disabled; draws still consumed
      }
      if (lane == 0) c[3] = 1;
    }
    wave_lds_sync();
  });
  if (overrun == 1 && lane == 0) a.counts[a.B * 4] = 1;   // the sample is not valid
}

// nonlinear_transform (operator_py/bbox_transform.py:52-77) on a float64 anchor / float32 gt box
__device__ __forceinline__ void rpn_encode_box(const double* box, const float4 g, float* t) {
  const double ex0 = box[0], ey0 = box[1], ex1 = box[2], ey1 = box[3];
  const double ew = ex1 - ex0 + 1.0, eh = ey1 - ey0 + 1.0;
  const double ecx = ex0 + 0.5 * (ew - 1.0), ecy = ey0 + 0.5 * (eh - 1.0);
  // gt is float32: gt[:,2] - gt[:,0] is a float32 subtraction, "+ 1.0" promotes per numpy 2 rules
  // (python float is weak: stays float32)
  const float gwf = g.z - g.x + 1.0f, ghf = g.w - g.y + 1.0f;
  const float gcxf = g.x + 0.5f * (gwf - 1.0f), gcyf = g.y + 0.5f * (ghf - 1.0f);
  t[0] = (float)(((double)gcxf - ecx) / (ew + 1e-14));
  t[1] = (float)(((double)gcyf - ecy) / (eh + 1e-14));
  t[2] = (float)log((double)gwf / ew);
  t[3] = (float)log((double)ghf / eh);
}

__global__ __launch_bounds__(kRpnT) void rpn_encode_kernel(RpnArgs a) {
  const int img = blockIdx.y;
  const int n = blockIdx.x * kRpnT + threadIdx.x;
  if (n >= a.N) return;
  const float h = a.im_info[img * 3], w = a.im_info[img * 3 + 1];
  const AnchorRef r = rpn_anchor(a, n, h >= w);
  const int* c = a.counts + img * 4;
  int lab = (int)a.label[(long)img * a.N + n];
  const bool kept = a.keep[(long)img * a.N + n] != 0;
  if (lab == 1 && c[2] && !kept) lab = -1;
  if (lab == 0 && c[3] && !kept) lab = -1;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  const float wv = lab == 1 ? 1.f : 0.f;
  if (lab == 1) {
    // nonlinear_transform (operator_py/bbox_transform.py:52-77) on float64 anchors / float32 gt
    const int g = a.argmax[(long)img * a.N + n];
    // the g-th VALID gt row
    int seen = -1;
    const float* gp = nullptr;
    for (int j = 0; j < a.M; ++j) {
      const float* p = a.gt + ((long)img * a.M + j) * a.G;
      if (p[0] != -1.f && ++seen == g) { gp = p; break; }
    }
    const double d[4] = {r.box.x, r.box.y, r.box.z, r.box.w};
    rpn_encode_box(d, make_float4(gp[0], gp[1], gp[2], gp[3]), t);
  }
  if (a.layout == 0) {
    a.cls[(long)img * a.N + n] = (float)lab;
    float4* tp = reinterpret_cast<float4*>(a.tgt) + (long)img * a.N + n;
    float4* wp = reinterpret_cast<float4*>(a.wgt) + (long)img * a.N + n;
    *tp = make_float4(t[0], t[1], t[2], t[3]);
    *wp = make_float4(wv, wv, wv, wv);
  } else {
    const int col = r.hwoff + r.y * r.fw + r.x;
    a.cls[(long)img * a.N + (long)r.a * a.sumHW + col] = (float)lab;
    for (int k = 0; k < 4; ++k) {
      const long o = ((long)img * a.A * 4 + r.a * 4 + k) * a.sumHW + col;
      a.tgt[o] = t[k];
      a.wgt[o] = wv;
    }
  }
}

// ---- RetinaNet anchor targets (models/retinanet/input.py:42-104, :149-199) -------------------------
// After rpn_overlap (per-anchor max / first arg-max, per-gt max over the valid anchors) ONE kernel
// does the rest: there is no sampling between the labels and the encoding.  RpnArgs carries the
// per-image foreground counters in `counts`; retina_fg turns them into max(1, count) floats.
__global__ __launch_bounds__(kRpnT) void retina_encode_kernel(RpnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float4 gbox[];
  __shared__ int wsum[kRpnT / kWave];
  float* gcls = reinterpret_cast<float*>(gbox + a.M);
  const int img = blockIdx.y, tid = threadIdx.x;
  const int n = blockIdx.x * kRpnT + tid;
  const int n_gt = rpn_load_gt<kRpnT>(a, img, gbox, wsum, gcls);
  const float h = a.im_info[img * 3], w = a.im_info[img * 3 + 1];
  float lab = -1.f, wv = 0.f;
  float t[4] = {0.f, 0.f, 0.f, 0.f};
  AnchorRef r{};
  if (n < a.N) {
    double d[4];
    r = rpn_anchor<true>(a, n, h >= w, d);
    if (rpn_valid64(a, d, h, w)) {
      if (n_gt > 0) {
        const float mo = a.maxov[(long)img * a.N + n];
        const int am = a.argmax[(long)img * a.N + n];
        if (mo < a.p.neg_thr) lab = 0.f;                                        // :62
        for (int j = 0; j < n_gt; ++j) {                                        // :59-64, the last j wins
          const float o = rpn_iou(r.box, gbox[j]);
          const float gm = __uint_as_float(a.gtmax[(long)img * a.M + j]);
          if (o == gm && o >= a.p.min_pos_thr) lab = gcls[j];
        }
        if (mo >= a.p.pos_thr) lab = gcls[am];                                  // :66
        rpn_encode_box(d, gbox[am], t);                                         // :69, every valid anchor
        if (lab >= 1.f) wv = 1.f;                                               // :70
      } else {
        lab = 0.f;                                                              // :72
      }
    }
  }
  const unsigned long long mf = __ballot(lab > 0.f);                            // :192
  if ((tid & (kWave - 1)) == 0 && mf) atomicAdd(&a.counts[img], __popcll(mf));
  if (n >= a.N) return;
  if (a.layout == 0) {
    a.cls[(long)img * a.N + n] = lab;
    reinterpret_cast<float4*>(a.tgt)[(long)img * a.N + n] = make_float4(t[0], t[1], t[2], t[3]);
    reinterpret_cast<float4*>(a.wgt)[(long)img * a.N + n] = make_float4(wv, wv, wv, wv);
  } else {
    // label: per level (A, fh, fw), levels concatenated (:176, :187); targets (4A, sumHW) (:177-189)
    const int cell = r.y * r.fw + r.x;
    a.cls[(long)img * a.N + (long)r.hwoff * a.A + (long)r.a * r.fh * r.fw + cell] = lab;
    for (int k = 0; k < 4; ++k) {
      const long o = ((long)img * a.A * 4 + r.a * 4 + k) * a.sumHW + r.hwoff + cell;
      a.tgt[o] = t[k];
      a.wgt[o] = wv;
    }
  }
}

// base anchors in double from the host's (ws, hs) (detection_input.py:392-397; 2 KB of arguments: together
// with RpnArgs they would pass the 4 KB a kernel may take, so they go through device memory)
struct RetinaBaseWH {
  double ws[kRpnMaxLvl][kRpnMaxA], hs[kRpnMaxLvl][kRpnMaxA];
  int stride[kRpnMaxLvl];
};
__global__ void retina_base_kernel(RetinaBaseWH p, double* base64, unsigned* clear, int nclear) {
  // ... and clears the per-gt maxima and the per-image counters behind them (a captured graph then holds kernel
  // nodes only)
  for (int k = threadIdx.x; k < nclear; k += blockDim.x) clear[k] = 0u;
  const int l = threadIdx.x / kRpnMaxA, i = threadIdx.x % kRpnMaxA;
  const double s = p.stride[l];
  const double x_ctr = 0.5 * (s - 1), y_ctr = 0.5 * (s - 1);
  double* b = base64 + (l * kRpnMaxA + i) * 4;
  b[0] = x_ctr - 0.5 * (p.ws[l][i] - 1);
  b[1] = y_ctr - 0.5 * (p.hs[l][i] - 1);
  b[2] = x_ctr + 0.5 * (p.ws[l][i] - 1);
  b[3] = y_ctr + 0.5 * (p.hs[l][i] - 1);
}

__global__ void retina_fg_kernel(const int* counts, float* fg_count, int B) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) fg_count[b] = (float)imaxr(1, counts[b]);
}

// the layouts return the bytes of the workspace in use; the size queries pass a null workspace and get null pointers
static size_t retina_layout(int B, int N, int M, RpnArgs* a, void* workspace) {
  WsCarver c(workspace);
  a->maxov = c.take<float>((size_t)B * N * 4);
  a->argmax = c.take<int>((size_t)B * N * 4);
  a->keep = c.take<unsigned char>((size_t)B * N);   // (written by rpn_overlap, not read)
  // gtmax and the per-image counters are adjacent: retina_base clears both
  a->gtmax = c.take<unsigned>((size_t)B * (M > 0 ? M : 1) * 4);
  a->counts = c.take<int>((size_t)B * 4);
  a->base64 = c.take<const double>((size_t)kRpnMaxLvl * kRpnMaxA * 4 * sizeof(double));
  return c.need();
}

static size_t rpn_layout(int B, int N, int M, int nblk, RpnArgs* a, void* workspace) {
  WsCarver c(workspace);
  a->maxov = c.take<float>((size_t)B * N * 4);
  a->argmax = c.take<int>((size_t)B * N * 4);
  a->label = c.take<signed char>((size_t)B * N);
  a->keep = c.take<unsigned char>((size_t)B * N);
  a->gtmax = c.take<unsigned>((size_t)B * (M > 0 ? M : 1) * 4);
  a->blk = c.take<int>((size_t)B * nblk * 2 * 4);
  a->fg_list = c.take<int>((size_t)B * N * 4);
  a->bg_list = c.take<int>((size_t)B * N * 4);
  a->counts = c.take<int>((size_t)(B * 4 + 1) * 4);
  return c.need();
}

static int rpn_count(const sd_rpn_target_param& p, int* A, int* N, int* sumHW) {
  SD_REQUIRE(p.nlvl >= 1 && p.nlvl <= kRpnMaxLvl, "nlvl=%d outside [1,%d]", p.nlvl, kRpnMaxLvl);
  SD_REQUIRE(p.n_scales >= 1 && p.n_aspects >= 1 && p.n_scales * p.n_aspects <= kRpnMaxA,
             "scales x aspects must be in [1,%d]", kRpnMaxA);
  *A = p.n_scales * p.n_aspects;
  long n = 0, hw = 0;
  for (int l = 0; l < p.nlvl; ++l) {
    SD_REQUIRE(p.stride[l] > 0 && p.short_side[l] > 0 && p.long_side[l] > 0, "level %d: bad size", l);
    hw += (long)p.short_side[l] * p.long_side[l];
  }
  n = hw * *A;
  SD_REQUIRE(n < (1L << 28), "too many anchors");
  *N = (int)n;
  *sumHW = (int)hw;
  return SD_OK;
}

// base anchors: core/detection_input.py:373-399 in double (np.round = rint, half to even)
static void rpn_base_anchors(RpnArgs* a) {
  for (int l = 0; l < a->p.nlvl; ++l) {
    const double s = a->p.stride[l];
    const double w = s, h = s, x_ctr = 0.5 * (w - 1), y_ctr = 0.5 * (h - 1);
    for (int i = 0; i < a->p.n_aspects; ++i) {
      const double wr = rint(sqrt(w * h / a->p.aspects[i]));
      const double hr = rint(wr * a->p.aspects[i]);
      for (int j = 0; j < a->p.n_scales; ++j) {
        const double ws = wr * a->p.scales[j], hs = hr * a->p.scales[j];
        float* b = a->base[l][i * a->p.n_scales + j];
        b[0] = (float)(x_ctr - 0.5 * (ws - 1));
        b[1] = (float)(y_ctr - 0.5 * (hs - 1));
        b[2] = (float)(x_ctr + 0.5 * (ws - 1));
        b[3] = (float)(y_ctr + 0.5 * (hs - 1));
      }
    }
  }
}

}  // namespace sd

using namespace sd;

extern "C" int sd_rpn_target_num_anchors(const sd_rpn_target_param* p) {
  int A, N, S;
  if (!p || rpn_count(*p, &A, &N, &S)) return -1;
  return N;
}

extern "C" size_t sd_rpn_target_workspace_bytes(const sd_rpn_target_param* p, int B, int M) {
  int A, N, S;
  if (!p || B <= 0 || rpn_count(*p, &A, &N, &S)) return 256;
  RpnArgs a{};
  return rpn_layout(B, N, M, cdiv(N, kRpnT), &a, nullptr) + 256;
}

// numpy MT19937 seeding (init_genrand via _legacy_seeding(seed)): key[624] + pos = 624
extern "C" int sd_mt19937_seed_host(uint32_t seed, int32_t* state_host) {
  SD_REQUIRE(state_host, "state_host is null");
  uint32_t k = seed;
  for (int i = 0; i < 624; ++i) {
    state_host[i] = (int32_t)k;
    k = 1812433253u * (k ^ (k >> 30)) + (uint32_t)(i + 1);
  }
  state_host[624] = 624;
  return SD_OK;
}

extern "C" int sd_rpn_anchor_target(const float* im_info, const float* gt_bbox, int B, int M, int G,
                                    const sd_rpn_target_param* param_host, int32_t* mt_state,
                                    float* cls_label, float* reg_target, float* reg_weight,
                                    int layout, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  SD_REQUIRE(param_host, "param is null");
  RpnArgs a{};
  a.p = *param_host;
  if (int e = rpn_count(a.p, &a.A, &a.N, &a.sumHW)) return e;
  SD_REQUIRE(B >= 0 && M >= 0 && (G == 4 || G == 5), "bad B / M / gt row width (4 or 5)");
  SD_REQUIRE(layout == 0 || layout == 1, "layout must be 0 (flat) or 1 (loader layout)");
  SD_REQUIRE(a.p.image_anchor >= 0 && a.p.image_anchor <= kRpnMaxKeep, "image_anchor outside [0,%d]",
             kRpnMaxKeep);
  SD_REQUIRE(a.p.pos_fraction >= 0.0 && a.p.pos_fraction <= 1.0, "pos_fraction outside [0,1]");
  if (B == 0) return SD_OK;
  SD_REQUIRE(im_info && (gt_bbox || M == 0) && mt_state && cls_label && reg_target && reg_weight,
             "null pointer");
  SD_REQUIRE((((uintptr_t)reg_target | (uintptr_t)reg_weight) & 15) == 0, "outputs must be 16-B aligned");
  // num_fg = int(fg_fraction * num) with a python float fraction: evaluated in double
  a.num_fg = (int)(a.p.pos_fraction * (double)a.p.image_anchor);
  rpn_base_anchors(&a);
  a.im_info = im_info; a.gt = gt_bbox; a.B = B; a.M = M; a.G = G; a.mt = mt_state;
  a.cls = cls_label; a.tgt = reg_target; a.wgt = reg_weight; a.layout = layout;
  a.nblk = cdiv(a.N, kRpnT);
  const size_t need = rpn_layout(B, a.N, M, a.nblk, &a, workspace);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "rpn_anchor_target workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  SD_HIP_CHECK(hipMemsetAsync(a.gtmax, 0, (size_t)B * (M > 0 ? M : 1) * 4, st));
  const size_t lds = (size_t)(M > 0 ? M : 1) * (sizeof(float4) + sizeof(unsigned));
  SD_REQUIRE(lds <= 64 * 1024, "too many gt boxes per image (M=%d)", M);
  const dim3 grid(a.nblk, B);
  hipLaunchKernelGGL(rpn_overlap_kernel<false>, grid, dim3(kRpnT), lds, st, a);
  hipLaunchKernelGGL(rpn_label_kernel, grid, dim3(kRpnT), lds, st, a);
  hipLaunchKernelGGL(rpn_scan_kernel, dim3(B), dim3(1024), 0, st, a);
  hipLaunchKernelGGL(rpn_lists_kernel, grid, dim3(kRpnT), 0, st, a);
  hipLaunchKernelGGL(rpn_sample_kernel, dim3(1), dim3(kMtThreads), 0, st, a);
  hipLaunchKernelGGL(rpn_encode_kernel, grid, dim3(kRpnT), 0, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" size_t sd_retina_target_workspace_bytes(const sd_rpn_target_param* p, int B, int M) {
  int A, N, S;
  if (!p || B <= 0 || M < 0 || rpn_count(*p, &A, &N, &S)) return 256;
  RpnArgs a{};
  return retina_layout(B, N, M, &a, nullptr) + 256;
}

extern "C" int sd_retina_anchor_target(const float* im_info, const float* gt_bbox, int B, int M,
                                       const sd_rpn_target_param* param_host, float* cls_label,
                                       float* reg_target, float* reg_weight, float* fg_count, int layout,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  SD_REQUIRE(param_host, "param is null");
  RpnArgs a{};
  a.p = *param_host;
  if (int e = rpn_count(a.p, &a.A, &a.N, &a.sumHW)) return e;
  SD_REQUIRE(B >= 0 && M >= 0, "bad B / M");
  SD_REQUIRE(layout == 0 || layout == 1, "layout must be 0 (flat) or 1 (loader layout)");
  const size_t lds = (size_t)(M > 0 ? M : 1) * (sizeof(float4) + sizeof(unsigned));
  SD_REQUIRE(lds <= 64 * 1024, "too many gt boxes per image (M=%d)", M);
  if (B == 0) return SD_OK;
  SD_REQUIRE(im_info && (gt_bbox || M == 0) && cls_label && reg_target && reg_weight && fg_count,
             "null pointer");
  SD_REQUIRE((((uintptr_t)reg_target | (uintptr_t)reg_weight) & 15) == 0, "outputs must be 16-B aligned");
  RetinaBaseWH wh{};
  for (int l = 0; l < a.p.nlvl; ++l) {
    const double s = a.p.stride[l];
    wh.stride[l] = a.p.stride[l];
    for (int i = 0; i < a.p.n_aspects; ++i) {
      const double wr = rint(sqrt(s * s / a.p.aspects[i]));   // np.round: half to even (:387-390)
      const double hr = rint(wr * a.p.aspects[i]);
      for (int j = 0; j < a.p.n_scales; ++j) {
        wh.ws[l][i * a.p.n_scales + j] = wr * a.p.scales[j];
        wh.hs[l][i * a.p.n_scales + j] = hr * a.p.scales[j];
      }
    }
  }
  a.im_info = im_info; a.gt = gt_bbox; a.B = B; a.M = M; a.G = 5;
  a.cls = cls_label; a.tgt = reg_target; a.wgt = reg_weight; a.layout = layout;
  a.nblk = cdiv(a.N, kRpnT);
  const size_t need = retina_layout(B, a.N, M, &a, workspace);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "retina_anchor_target workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(a.nblk, B);
  hipLaunchKernelGGL(retina_base_kernel, dim3(1), dim3(kRpnMaxLvl * kRpnMaxA), 0, st, wh,
                     const_cast<double*>(a.base64), a.gtmax, (int)(reinterpret_cast<unsigned*>(a.counts + B) - a.gtmax));
  hipLaunchKernelGGL(rpn_overlap_kernel<true>, grid, dim3(kRpnT), lds, st, a);
  hipLaunchKernelGGL(retina_encode_kernel, grid, dim3(kRpnT), lds, st, a);
  hipLaunchKernelGGL(retina_fg_kernel, dim3(cdiv(B, kRpnT)), dim3(kRpnT), 0, st, a.counts, fg_count, B);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
