// _contrib_DeformablePSROIPooling forward / backward and TSD's fused FPN extractor for gfx950.
//   operator: mx.sym.contrib.DeformablePSROIPooling (upstream MXNet; the arithmetic is restated in
//             DESIGN.md 4.15 and tests/deform_psroi_ref.py, which are the spec here)
//   fused:    FPNRoIAlign_DeltaC / FPNRoIAlign_DeltaR.get_roi_feature, models/TSD/poolings.py:51-174 with
//             fpn_roi_assign_offset :12-47 -- four masked operator calls and an add_n per extractor
//
// Both run on ONE kernel pair, workgroup = RoI.  Sample coordinates depend on (RoI, bin, class) only, so
// the workgroup first builds a tap table in LDS -- one thread per (class, bin), S*S entries each:
// {pixel index | neighbour flags, dx, dy}, laid out [sample][unit] so that lanes on neighbouring bins read
// neighbouring words -- and then runs its lanes over (channel, bin): the reference repeats the coordinate
// work for each of the C channels.
//
// The fused form loops over the levels.  A RoI's own level (fpn_level, the arithmetic of
// fpn_roi_assign_offset) is pooled with the RoI and its offsets; on every other level the reference pools
// the masked RoI (-1,-1,-1,-1) with zero offsets, which is NOT nothing: the width clamp max(., 0.1) pushes
// the last bins of a level with scale < 0.1 inside the map's border, so they average feat[b, c, 0, 0].
// The same table builder is run on that RoI, so whatever bins a stride list produces are reproduced
// (levels whose table is empty are skipped by a workgroup-uniform flag).  Levels are summed in order, as
// add_n does.
//
// Backward: a wave takes one output channel at a time.  Its (RoI, channel) patch -- the bounding box of the
// table's pixels -- lives in LDS; the 4 x S*S x P*P tap gradients are added there (ds_add_f32, no return value)
// and every touched pixel is flushed ONCE with a global float atomic, lanes along the rows of the patch.
// RoIs whose patch exceeds the wave's share of LDS, and group_size > 1 (the bins of one output channel go
// to different planes), add each tap to memory directly; a table that touches a single pixel (the masked
// RoI's) is summed in registers and one wave reduction instead.  d_data therefore depends on the order in which
// the hardware serves the atomics, like the reference's.  d_trans does not: every lane owns its bins' sums
// (over its wave's channels, in channel order), and one thread per element adds the waves' partial sums in
// a fixed order and stores the result.
#include "roi_align_common.h"
#include <limits.h>

namespace sd {

constexpr int kDpT = 256, kDpNW = kDpT / kWave;
constexpr int kDpMaxTaps = 4096;       // table entries per level: 48 KB
constexpr int kDpLds = 64 * 1024;      // everything fits the default dynamic LDS limit
constexpr int kDpPatchMax = 2048;      // floats per wave (45 x 45 pixels): three workgroups per CU at 7x7x16
constexpr int kDpPatchMin = 64;

// LDS of the forward: tables + the counts of every level; of the backward without its patches: tables + the
// bounding box + the per-wave d_trans sums.  With at most five levels the backward's is the larger.
static size_t dp_fwd_lds_bytes(long ncls, long P, long S, long nlvl) {
  const long U = ncls * P * P;
  return (size_t)(U * S * S * 3 + nlvl * U + SD_MAX_FPN_LEVELS) * 4;
}
static size_t dp_bwd_fixed_lds_bytes(long ncls, long P, long S) {
  const long U = ncls * P * P;
  return (size_t)(U * S * S * 3 + 8 + kDpNW * U * 2) * 4;
}
// THE supported set: one predicate for the forward, the backward and the adapter's sd_supports
static bool dp_supported(long ncls, long P, long S) {
  if (ncls < 1 || P < 1 || S < 1 || P > 4096 || S > 4096 || ncls > 4096) return false;
  return ncls * P * P * S * S <= kDpMaxTaps && dp_fwd_lds_bytes(ncls, P, S, 5) <= (size_t)kDpLds &&
         dp_bwd_fixed_lds_bytes(ncls, P, S) <= (size_t)kDpLds;
}

struct DpArgs {
  RoiLevels L;                         // data / H / W / scale per level; the level rule's constants
  float* ddata[SD_MAX_FPN_LEVELS];
  const float* rois;                   // single: (K,5) [batch, x1, y1, x2, y2]; fused: (B*R,4)
  const float* trans;                  // (K, 2*ncls, tpart, tpart)
  float* out;
  float* top_count;                    // single: (K,OD,P,P); fused: (K,nlvl,P,P)
  const float* dy;
  const float* tc;                     // top_count as the backward reads it
  float* dtrans;
  int K, B, R, C, OD, G, P, part, S, ncls, cpc;
  int tpart;                           // side of the stored offset map: part, or 1 (one offset per RoI)
  float trans_std;
  int no_trans, fused, req_trans;
};

// Table of level l for RoI n, one thread per unit (class, bin).  own: the RoI is pooled as itself;
// otherwise (fused form, another level) as (-1,-1,-1,-1) with zero offsets.  fill = false: counts only.
// cnt[unit] = kept samples (cnt may be null); *any is set when some unit keeps one; bb (fill only) = bounding box of the pixels.
__device__ __forceinline__ void dp_build(const DpArgs& a, int n, int l, bool own, bool fill, int* tp,
                                         float* tdx, float* tdy, int* cnt, int* any, int* bb) {
  const int P = a.P, PP = P * P, U = a.ncls * PP, S = a.S;
  const int H = a.L.H[l], W = a.L.W[l];
  const float scale = a.L.scale[l];
  float x1 = -1.f, y1 = -1.f, x2 = -1.f, y2 = -1.f;
  bool ok = true;
  if (a.fused) {
    if (own) {
      const float* r = a.rois + (long)n * 4;
      x1 = r[0]; y1 = r[1]; x2 = r[2]; y2 = r[3];
    }
  } else {
    const float* r = a.rois + (long)n * 5;
    ok = r[0] >= 0.f && r[0] < (float)a.B;   // (a batch index that names no image pools nothing)
    x1 = r[1]; y1 = r[2]; x2 = r[3]; y2 = r[4];
  }
  // roundf: half away from zero
  const float rsw = roundf(x1) * scale - 0.5f, rsh = roundf(y1) * scale - 0.5f;
  const float rew = (roundf(x2) + 1.f) * scale - 0.5f, reh = (roundf(y2) + 1.f) * scale - 0.5f;
  const float rw = fmaxr(rew - rsw, 0.1f), rh = fmaxr(reh - rsh, 0.1f);
  const float bin_w = rw / (float)P, bin_h = rh / (float)P;
  const float sub_w = bin_w / (float)S, sub_h = bin_h / (float)S;
  const float wlim = (float)W - 0.5f, hlim = (float)H - 0.5f;
  const bool with_trans = !a.no_trans && own;
  for (int u = threadIdx.x; u < U; u += kDpT) {
    const int cls = u / PP, bin = u - cls * PP, ph = bin / P, pw = bin - ph * P;
    float trans_x = 0.f, trans_y = 0.f;
    if (with_trans) {
      const int part_h = (int)floorf((float)ph / (float)P * (float)a.part);
      const int part_w = (int)floorf((float)pw / (float)P * (float)a.part);
      const int cells = a.tpart * a.tpart, cell = a.tpart == 1 ? 0 : part_h * a.tpart + part_w;
      const float* t = a.trans + ((long)n * a.ncls + cls) * 2 * cells + cell;
      trans_x = t[0] * a.trans_std;
      trans_y = t[cells] * a.trans_std;
    }
    float wstart = (float)pw * bin_w + rsw;
    wstart += trans_x * rw;
    float hstart = (float)ph * bin_h + rsh;
    hstart += trans_y * rh;
    int count = 0, xmin = INT_MAX, xmax = -1, ymin = INT_MAX, ymax = -1;
    for (int ih = 0; ih < S; ++ih)
      for (int iw = 0; iw < S; ++iw) {
        float w = wstart + (float)iw * sub_w;
        float h = hstart + (float)ih * sub_h;
        // (written so that a NaN coordinate is skipped as well: nothing below may index with it)
        const bool keep = ok && w >= -0.5f && w <= wlim && h >= -0.5f && h <= hlim;
        int p = -1;
        float dx = 0.f, dy = 0.f;
        if (keep) {
          w = fminr(fmaxr(w, 0.f), (float)W - 1.f);
          h = fminr(fmaxr(h, 0.f), (float)H - 1.f);
          const int x0 = (int)floorf(w), xb = (int)ceilf(w), y0 = (int)floorf(h), yb = (int)ceilf(h);
          dx = w - (float)x0;
          dy = h - (float)y0;
          p = (y0 * W + x0) | ((xb > x0) << 29) | ((yb > y0) << 30);
          ++count;
          xmin = iminr(xmin, x0); xmax = imaxr(xmax, xb);
          ymin = iminr(ymin, y0); ymax = imaxr(ymax, yb);
        }
        if (fill) {
          const int e = (ih * S + iw) * U + u;
          tp[e] = p;
          tdx[e] = dx;
          tdy[e] = dy;
        }
      }
    if (cnt) cnt[u] = count;
    if (count > 0) {
      *any = 1;
      if (fill && bb) {
        atomicMin(bb + 0, xmin); atomicMax(bb + 1, xmax);
        atomicMin(bb + 2, ymin); atomicMax(bb + 3, ymax);
      }
    }
  }
}

__device__ __forceinline__ int dp_own_level(const DpArgs& a, int n) {
  if (!a.fused) return 0;
  const float* r = a.rois + (long)n * 4;
  return fpn_level(r[0], r[1], r[2], r[3], a.L);
}

// data channel of output channel ctop at bin (ph, pw): position-sensitive groups
__device__ __forceinline__ int dp_channel(const DpArgs& a, int ctop, int ph, int pw) {
  if (a.G == 1) return ctop;
  int gw = (int)floorf((float)pw * (float)a.G / (float)a.P);
  int gh = (int)floorf((float)ph * (float)a.G / (float)a.P);
  gw = iminr(imaxr(gw, 0), a.G - 1);
  gh = iminr(imaxr(gh, 0), a.G - 1);
  return (ctop * a.G + gh) * a.G + gw;
}

__global__ __launch_bounds__(kDpT) void deform_psroi_fwd_kernel(DpArgs a) {
  extern __shared__ __attribute__((aligned(16))) int dp_smem[];
  const int tid = threadIdx.x, n = blockIdx.x;
  const int P = a.P, PP = P * P, U = a.ncls * PP, SS = a.S * a.S, NT = U * SS, nlvl = a.L.nlvl;
  int* tp = dp_smem;
  float* tdx = reinterpret_cast<float*>(dp_smem + NT);
  float* tdy = tdx + NT;
  int* cnt = reinterpret_cast<int*>(tdy + NT);   // [nlvl][U]
  int* any = cnt + nlvl * U;                      // [SD_MAX_FPN_LEVELS]
  const int own = dp_own_level(a, n);
  if (tid < SD_MAX_FPN_LEVELS) any[tid] = 0;
  __syncthreads();
  for (int l = 0; l < nlvl; ++l) dp_build(a, n, l, l == own, false, tp, tdx, tdy, cnt + l * U, any + l, nullptr);
  __syncthreads();
  const long obase = (long)n * a.OD * PP;
  const int items = a.OD * PP;
  const int batch = a.fused ? n / a.R : (int)a.rois[(long)n * 5];   // (used only where a sample was kept)
  for (int l = 0; l < nlvl; ++l) {
    if (!any[l]) continue;   // workgroup-uniform
    __syncthreads();
    dp_build(a, n, l, l == own, true, tp, tdx, tdy, cnt + l * U, any + l, nullptr);
    __syncthreads();
    const int W = a.L.W[l];
    const long HW = (long)a.L.H[l] * W;
    const float* data = a.L.data[l] + (long)batch * a.C * HW;
    for (int i = tid; i < items; i += kDpT) {
      const int ctop = i / PP, bin = i - ctop * PP, ph = bin / P, pw = bin - ph * P;
      const int u = (ctop / a.cpc) * PP + bin;
      const int count = cnt[l * U + u];
      if (count == 0) continue;
      const float* plane = data + (long)dp_channel(a, ctop, ph, pw) * HW;
      float sum = 0.f;
      for (int s = 0; s < SS; ++s) {
        const int p = tp[s * U + u];
        if (p < 0) continue;
        const float dx = tdx[s * U + u], dy = tdy[s * U + u];
        const int i00 = p & 0x1fffffff, ox = (p >> 29) & 1, oy = ((p >> 30) & 1) * W;
        const float v00 = plane[i00], v01 = plane[i00 + oy], v10 = plane[i00 + ox], v11 = plane[i00 + oy + ox];
        const float val = (1.f - dx) * (1.f - dy) * v00 + (1.f - dx) * dy * v01 + dx * (1.f - dy) * v10 +
                          dx * dy * v11;
        sum += val;
      }
      const float v = sum / (float)count;
      bool earlier = false;
      for (int l2 = 0; l2 < l; ++l2) earlier |= cnt[l2 * U + u] > 0;
      float* o = a.out + obase + i;
      *o = earlier ? *o + v : v;   // (this thread wrote *o itself)
    }
  }
  for (int i = tid; i < items; i += kDpT) {
    const int ctop = i / PP, bin = i - ctop * PP;
    const int u = (ctop / a.cpc) * PP + bin;
    bool some = false;
    for (int l = 0; l < nlvl; ++l) some |= cnt[l * U + u] > 0;
    if (!some) a.out[obase + i] = 0.f;
    if (!a.fused) a.top_count[obase + i] = (float)cnt[u];
  }
  if (a.fused)   // ncls = 1: one count per (RoI, level, bin)
    for (int i = tid; i < nlvl * PP; i += kDpT) a.top_count[(long)n * nlvl * PP + i] = (float)cnt[i];
}

__global__ __launch_bounds__(kDpT) void deform_psroi_bwd_kernel(DpArgs a, int cap) {
  extern __shared__ __attribute__((aligned(16))) int dp_smem[];
  const int tid = threadIdx.x, n = blockIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid / kWave);
  const int P = a.P, PP = P * P, U = a.ncls * PP, SS = a.S * a.S, NT = U * SS, nlvl = a.L.nlvl;
  int* tp = dp_smem;
  float* tdx = reinterpret_cast<float*>(dp_smem + NT);
  float* tdy = tdx + NT;
  int* bb = reinterpret_cast<int*>(tdy + NT);     // x min / max, y min / max, any
  float* dtr = reinterpret_cast<float*>(bb + 8);  // [wave][U][2]
  float* patch = dtr + kDpNW * U * 2 + (long)wave * cap;
  const int own = dp_own_level(a, n);
  const bool want_tr = !a.no_trans && a.req_trans != SD_REQ_NULL;
  for (int i = tid; i < kDpNW * U * 2; i += kDpT) dtr[i] = 0.f;
  for (int i = lane; i < cap; i += kWave) patch[i] = 0.f;
  const int batch = a.fused ? n / a.R : (int)a.rois[(long)n * 5];
  for (int l = 0; l < nlvl; ++l) {
    __syncthreads();
    if (tid == 0) {
      bb[0] = INT_MAX; bb[1] = -1; bb[2] = INT_MAX; bb[3] = -1; bb[4] = 0;
    }
    __syncthreads();
    dp_build(a, n, l, l == own, true, tp, tdx, tdy, nullptr, bb + 4, bb);  // (the divisor is top_count)
    __syncthreads();
    if (!bb[4]) continue;   // workgroup-uniform
    const bool tr_here = want_tr && l == own;
    float* ddata = a.ddata[l];
    if (!ddata && !tr_here) continue;
    const int W = a.L.W[l];
    const long HW = (long)a.L.H[l] * W;
    const int bx = bb[0], by = bb[2], bw = bb[1] - bb[0] + 1, area = bw * (bb[3] - bb[2] + 1);
    // a table that touches ONE pixel (the masked RoI on a level with scale < 0.1: every kept sample clamps to
    // pixel (0, 0)): all lanes would add to one LDS word, and a compare-and-swap loop serialises them; the lanes
    // sum their own terms instead and one wave reduction feeds a single atomic (fixed order)
    const bool one_pixel = ddata && a.G == 1 && area == 1;
    const bool use_patch = ddata && a.G == 1 && area > 1 && area <= cap;   // (cap = 0: knob deform_psroi_bwd_patch = 0)
    for (int ctop = wave; ctop < a.OD; ctop += kDpNW) {
      const int cls = ctop / a.cpc;
      float acc = 0.f;
      for (int bin = lane; bin < PP; bin += kWave) {
        const int u = cls * PP + bin, ph = bin / P, pw = bin - ph * P;
        const float count = a.fused ? a.tc[((long)n * nlvl + l) * PP + bin] : a.tc[((long)n * a.OD + ctop) * PP + bin];
        if (!(count > 0.f)) continue;
        const float g = a.dy[((long)n * a.OD + ctop) * PP + bin] / count;
        const long poff = ((long)batch * a.C + dp_channel(a, ctop, ph, pw)) * HW;
        // two passes over the bin's taps.  First the gathers of the offset gradient with nothing between them
        // that waits on LDS or on an atomic, so that the loads of all samples are in flight together as in the
        // forward (inside one loop with the scatter every sample waited a memory round trip of its own: the
        // backward took the same ~20 ms with and without the LDS patch).  Then the scatter, which loads nothing.
        float gx = 0.f, gy = 0.f;
        if (tr_here) {
          const float* dl = a.L.data[l] + poff;
          for (int s = 0; s < SS; ++s) {
            const int p = tp[s * U + u];
            if (p < 0) continue;
            const float dx = tdx[s * U + u], dy = tdy[s * U + u];
            const int i00 = p & 0x1fffffff, ox = (p >> 29) & 1, oy = ((p >> 30) & 1) * W;
            const float u00 = dl[i00], u01 = dl[i00 + oy], u10 = dl[i00 + ox], u11 = dl[i00 + oy + ox];
            gx += (u11 * dy + u10 * (1.f - dy) - u01 * dy - u00 * (1.f - dy)) * a.trans_std * g;
            gy += (u11 * dx + u01 * (1.f - dx) - u10 * dx - u00 * (1.f - dx)) * a.trans_std * g;
          }
        }
        for (int s = 0; ddata && s < SS; ++s) {
          const int p = tp[s * U + u];
          if (p < 0) continue;
          const float dx = tdx[s * U + u], dy = tdy[s * U + u];
          const int i00 = p & 0x1fffffff, ox = (p >> 29) & 1, oyr = (p >> 30) & 1, oy = oyr * W;
          const float q00 = (1.f - dx) * (1.f - dy), q01 = (1.f - dx) * dy, q10 = dx * (1.f - dy), q11 = dx * dy;
          if (one_pixel) {
            acc += g * q00;
            acc += g * q01;
            acc += g * q10;
            acc += g * q11;
          } else if (use_patch) {
            const int y0 = i00 / W, x0 = i00 - y0 * W;
            float* q = patch + (y0 - by) * bw + (x0 - bx);
            // (a zero term changes nothing: dx or dy is 0 on a pixel centre and at a clamped border)
            // ds_add_f32 without a return value: nothing waits for it.  (The compare-and-swap loop of the other
            // LDS planes of this library has the higher peak rate, but a lane here walks 64 dependent adds per
            // (channel, bin) with twelve waves per CU, and each round trip of the loop was paid in full.)
            if (g * q00 != 0.f) atomicAdd(q, g * q00);
            if (g * q01 != 0.f) atomicAdd(q + oyr * bw, g * q01);
            if (g * q10 != 0.f) atomicAdd(q + ox, g * q10);
            if (g * q11 != 0.f) atomicAdd(q + oyr * bw + ox, g * q11);
          } else {
            float* q = ddata + poff + i00;
            atomicAdd(q, g * q00);
            atomicAdd(q + oy, g * q01);
            atomicAdd(q + ox, g * q10);
            atomicAdd(q + oy + ox, g * q11);
          }
        }
        if (tr_here) {   // this lane owns (wave, u): channel order, no atomics
          dtr[(wave * U + u) * 2 + 0] += gx;
          dtr[(wave * U + u) * 2 + 1] += gy;
        }
      }
      if (one_pixel) {
        const float tot = wave_sum_f32(acc);
        if (lane == 0 && tot != 0.f) atomicAdd(ddata + ((long)batch * a.C + ctop) * HW + (long)by * W + bx, tot);
      }
      if (use_patch) {
        wave_lds_sync();
        float* dst = ddata + ((long)batch * a.C + ctop) * HW;
        for (int i = lane; i < area; i += kWave) {
          const float v = patch[i];
          if (v != 0.f) {
            const int y = i / bw, x = i - y * bw;
            atomicAdd(dst + (long)(by + y) * W + bx + x, v);
            patch[i] = 0.f;
          }
        }
        wave_lds_sync();
      }
    }
  }
  if (!want_tr) return;
  __syncthreads();
  // roi_w / roi_h of the own level: the factor the per-sample terms share
  float rw = 0.f, rh = 0.f;
  if (own >= 0) {
    const float scale = a.L.scale[own];
    const float* r = a.fused ? a.rois + (long)n * 4 : a.rois + (long)n * 5 + 1;
    const float rsw = roundf(r[0]) * scale - 0.5f, rsh = roundf(r[1]) * scale - 0.5f;
    const float rew = (roundf(r[2]) + 1.f) * scale - 0.5f, reh = (roundf(r[3]) + 1.f) * scale - 0.5f;
    rw = fmaxr(rew - rsw, 0.1f);
    rh = fmaxr(reh - rsh, 0.1f);
  }
  const int cells = a.tpart * a.tpart;
  for (int e = tid; e < a.ncls * 2 * cells; e += kDpT) {
    const int cls = e / (2 * cells), xy = (e / cells) & 1, cell = e % cells;
    float sum = 0.f;
    for (int bin = 0; bin < PP; ++bin) {
      const int ph = bin / P, pw = bin - ph * P;
      const int part_h = (int)floorf((float)ph / (float)P * (float)a.part);
      const int part_w = (int)floorf((float)pw / (float)P * (float)a.part);
      if ((a.tpart == 1 ? 0 : part_h * a.tpart + part_w) != cell) continue;
      for (int w = 0; w < kDpNW; ++w) sum += dtr[(w * U + cls * PP + bin) * 2 + xy];
    }
    sum *= xy ? rh : rw;
    float* dst = a.dtrans + (long)n * a.ncls * 2 * cells + e;
    *dst = a.req_trans == SD_REQ_ADD ? *dst + sum : sum;
  }
}

static int dp_check_req(int r) { return r == SD_REQ_NULL || r == SD_REQ_WRITE || r == SD_REQ_ADD; }

// argument checks both forms share; fills the scalar fields
static int dp_common(DpArgs& a, int K, int B, int C, int output_dim, int group_size, int pooled_size, int part_size,
                     int sample_per_part, int num_classes, float trans_std, int no_trans) {
  SD_REQUIRE(K >= 0 && B >= 0 && C >= 0, "negative dimension");
  SD_REQUIRE(pooled_size >= 1, "pooled_size must be at least 1");
  SD_REQUIRE(part_size >= 0, "part_size must not be negative");
  SD_REQUIRE(sample_per_part >= 1, "sample_per_part must be at least 1");
  SD_REQUIRE(group_size >= 1 && output_dim >= 1, "group_size and output_dim must be at least 1");
  SD_REQUIRE((long)C == (long)output_dim * group_size * group_size,
             "data has %d channels, output_dim * group_size^2 = %ld", C, (long)output_dim * group_size * group_size);
  const int ncls = no_trans ? 1 : num_classes;
  SD_REQUIRE(ncls >= 1, "num_classes must be at least 1");
  SD_REQUIRE(output_dim % ncls == 0, "output_dim %d is not a multiple of num_classes %d", output_dim, ncls);
  a.K = K; a.B = B; a.C = C; a.OD = output_dim; a.G = group_size; a.P = pooled_size;
  a.part = part_size ? part_size : pooled_size;
  a.tpart = a.part;
  a.S = sample_per_part; a.ncls = ncls; a.cpc = output_dim / ncls;
  a.trans_std = trans_std; a.no_trans = no_trans ? 1 : 0;
  a.R = 0; a.fused = 0; a.req_trans = SD_REQ_NULL;
  if (!dp_supported(ncls, pooled_size, sample_per_part))
    return fail(SD_ERR_UNSUPPORTED,
                "num_classes %d, pooled_size %d, sample_per_part %d: the RoI's tap table (at most %d entries) and the "
                "backward's sums do not fit in LDS (sd_deform_psroi_pool_supported)", ncls, pooled_size,
                sample_per_part, kDpMaxTaps);
  if ((long)K * output_dim * pooled_size * pooled_size >= (1L << 31))
    return fail(SD_ERR_UNSUPPORTED, "output has >= 2^31 elements");
  return SD_OK;
}

static int dp_check_plane(int H, int W) {
  SD_REQUIRE(H > 0 && W > 0, "bad feature map size");
  if ((long)H * W >= (1L << 29)) return fail(SD_ERR_UNSUPPORTED, "plane of >= 2^29 pixels");
  return SD_OK;
}

static size_t dp_fwd_lds(const DpArgs& a) { return dp_fwd_lds_bytes(a.ncls, a.P, a.S, a.L.nlvl); }

// backward: tables + per-wave d_trans sums + as much patch as fits (0: direct adds only)
static size_t dp_bwd_lds(const DpArgs& a, int* cap) {
  const long fixed = (long)dp_bwd_fixed_lds_bytes(a.ncls, a.P, a.S);
  long c = (kDpLds - fixed) / (4 * kDpNW);
  c = c > kDpPatchMax ? kDpPatchMax : (c < kDpPatchMin ? 0 : c & ~63L);
  if (tuning(Knob::deform_psroi_bwd_patch) == 0) c = 0;   // every tap straight to memory (A/B measurements)
  *cap = (int)c;
  return (size_t)(fixed + c * 4 * kDpNW);
}

static int dp_launch_fwd(const DpArgs& a, hipStream_t st) {
  const size_t lds = dp_fwd_lds(a);
  if (lds > (size_t)kDpLds) return fail(SD_ERR_UNSUPPORTED, "tap tables of %zu bytes do not fit in LDS", lds);
  hipLaunchKernelGGL(deform_psroi_fwd_kernel, dim3(a.K), dim3(kDpT), lds, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

static int dp_launch_bwd(const DpArgs& a, hipStream_t st) {
  int cap = 0;
  const size_t lds = dp_bwd_lds(a, &cap);
  if (lds > (size_t)kDpLds) return fail(SD_ERR_UNSUPPORTED, "tap tables of %zu bytes do not fit in LDS", lds);
  hipLaunchKernelGGL(deform_psroi_bwd_kernel, dim3(a.K), dim3(kDpT), lds, st, a, cap);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

static void dp_single_level(DpArgs& a, const float* data, int H, int W, float spatial_scale) {
  a.L.nlvl = 1;
  a.L.data[0] = data;
  a.L.H[0] = H;
  a.L.W[0] = W;
  a.L.stride[0] = 1;
  a.L.scale[0] = spatial_scale;
  a.L.canon_scale = a.L.canon_level = a.L.k_min = a.L.k_max = 0.f;
}

static int dp_fused_common(DpArgs& a, const float* const* feats, const int* Hs, const int* Ws, const int* strides,
                           int nlvl, int B, int C, int R, int pooled_size, int trans_part, int sample_per_part,
                           float trans_std, float canon_scale, float canon_level) {
  SD_REQUIRE(Hs && Ws && strides, "null pointer");
  SD_REQUIRE(nlvl >= 1 && nlvl <= 5, "nlvl=%d out of range [1,5]", nlvl);
  SD_REQUIRE(R >= 0 && B >= 0, "negative dimension");
  SD_REQUIRE((long)B * R < (1L << 31), "too many RoIs");
  SD_REQUIRE(C >= 1, "C must be at least 1");
  if (int e = dp_common(a, B * R, B, C, C, 1, pooled_size, 0, sample_per_part, 1, trans_std, 0)) return e;
  SD_REQUIRE(trans_part == 1 || trans_part == pooled_size, "trans_part must be 1 or pooled_size, got %d", trans_part);
  if (int e = fill_levels(a.L, feats, Hs, Ws, strides, nlvl, canon_scale, canon_level)) return e;
  for (int l = 0; l < nlvl; ++l)
    if (int e = dp_check_plane(Hs[l], Ws[l])) return e;
  a.R = R;
  a.fused = 1;
  a.tpart = trans_part;
  return SD_OK;
}

}  // namespace sd

using namespace sd;

extern "C" int sd_deform_psroi_pool_supported(int num_classes, int pooled_size, int sample_per_part) {
  return dp_supported(num_classes, pooled_size, sample_per_part) ? 1 : 0;
}

extern "C" int sd_deform_psroi_pool_fwd(const float* data, const float* rois, const float* trans, float* out,
                                        float* top_count, int B, int C, int H, int W, int K, int num_classes,
                                        float spatial_scale, int output_dim, int group_size, int pooled_size,
                                        int part_size, int sample_per_part, float trans_std, int no_trans,
                                        void* stream) {
  DpArgs a{};
  if (int e = dp_common(a, K, B, C, output_dim, group_size, pooled_size, part_size, sample_per_part, num_classes,
                        trans_std, no_trans))
    return e;
  if (int e = dp_check_plane(H, W)) return e;
  if (K == 0) return SD_OK;
  SD_REQUIRE(data && rois && out && top_count && (no_trans || trans), "null pointer");
  dp_single_level(a, data, H, W, spatial_scale);
  a.rois = rois; a.trans = trans; a.out = out; a.top_count = top_count;
  return dp_launch_fwd(a, (hipStream_t)stream);
}

extern "C" int sd_deform_psroi_pool_bwd(const float* out_grad, const float* data, const float* rois,
                                        const float* trans, const float* top_count, float* d_data, float* d_rois,
                                        float* d_trans, int req_data, int req_rois, int req_trans, int B, int C,
                                        int H, int W, int K, int num_classes, float spatial_scale, int output_dim,
                                        int group_size, int pooled_size, int part_size, int sample_per_part,
                                        float trans_std, int no_trans, void* stream) {
  DpArgs a{};
  if (int e = dp_common(a, K, B, C, output_dim, group_size, pooled_size, part_size, sample_per_part, num_classes,
                        trans_std, no_trans))
    return e;
  if (int e = dp_check_plane(H, W)) return e;
  SD_REQUIRE(dp_check_req(req_data) && dp_check_req(req_rois) && dp_check_req(req_trans),
             "req must be null, write or add");
  if (no_trans) req_trans = SD_REQ_NULL;
  hipStream_t st = (hipStream_t)stream;
  const size_t dx_bytes = (size_t)B * C * H * W * sizeof(float);
  SD_REQUIRE(req_data == SD_REQ_NULL || dx_bytes == 0 || d_data, "null pointer");
  SD_REQUIRE(req_rois != SD_REQ_WRITE || K == 0 || d_rois, "null pointer");
  SD_REQUIRE(req_trans == SD_REQ_NULL || K == 0 || (d_trans && trans), "null pointer");
  SD_REQUIRE(K == 0 || (req_data == SD_REQ_NULL && req_trans == SD_REQ_NULL) || (out_grad && data && rois && top_count),
             "null pointer");
  if (req_data == SD_REQ_WRITE && dx_bytes) SD_HIP_CHECK(hipMemsetAsync(d_data, 0, dx_bytes, st));
  if (req_rois == SD_REQ_WRITE && K > 0) SD_HIP_CHECK(hipMemsetAsync(d_rois, 0, (size_t)K * 5 * sizeof(float), st));
  if (K == 0 || (req_data == SD_REQ_NULL && req_trans == SD_REQ_NULL)) return SD_OK;
  dp_single_level(a, data, H, W, spatial_scale);
  a.ddata[0] = req_data == SD_REQ_NULL ? nullptr : d_data;
  a.rois = rois; a.trans = trans; a.dy = out_grad; a.tc = top_count; a.dtrans = d_trans;
  a.req_trans = req_trans;
  return dp_launch_bwd(a, st);
}

extern "C" int sd_fpn_deform_roi_pool_fwd(const float* const* feats_host, const int* Hs_host, const int* Ws_host,
                                          const int* strides_host, int nlvl, const float* rois, const float* trans,
                                          float* out, float* top_count, int B, int C, int R, int pooled_size,
                                          int trans_part, int sample_per_part, float trans_std,
                                          float roi_canonical_scale, float roi_canonical_level, void* stream) {
  DpArgs a{};
  SD_REQUIRE(feats_host, "null pointer");
  if (int e = dp_fused_common(a, feats_host, Hs_host, Ws_host, strides_host, nlvl, B, C, R, pooled_size, trans_part,
                              sample_per_part, trans_std, roi_canonical_scale, roi_canonical_level))
    return e;
  if (a.K == 0) return SD_OK;
  for (int l = 0; l < nlvl; ++l) SD_REQUIRE(feats_host[l], "null pointer");
  SD_REQUIRE(rois && trans && out && top_count, "null pointer");
  a.rois = rois; a.trans = trans; a.out = out; a.top_count = top_count;
  return dp_launch_fwd(a, (hipStream_t)stream);
}

extern "C" int sd_fpn_deform_roi_pool_bwd(const float* out_grad, const float* const* feats_host,
                                          float* const* d_feats_host, const int* Hs_host, const int* Ws_host,
                                          const int* strides_host, int nlvl, const float* rois, const float* trans,
                                          const float* top_count, float* d_trans, int req_data, int req_trans, int B,
                                          int C, int R, int pooled_size, int trans_part, int sample_per_part,
                                          float trans_std, float roi_canonical_scale, float roi_canonical_level,
                                          void* stream) {
  DpArgs a{};
  SD_REQUIRE(feats_host, "null pointer");
  if (int e = dp_fused_common(a, feats_host, Hs_host, Ws_host, strides_host, nlvl, B, C, R, pooled_size, trans_part,
                              sample_per_part, trans_std, roi_canonical_scale, roi_canonical_level))
    return e;
  SD_REQUIRE(dp_check_req(req_data) && dp_check_req(req_trans), "req must be null, write or add");
  SD_REQUIRE(req_data == SD_REQ_NULL || d_feats_host, "null pointer");
  for (int l = 0; l < nlvl; ++l) {
    SD_REQUIRE(feats_host[l], "null pointer");
    SD_REQUIRE(req_data == SD_REQ_NULL || B == 0 || d_feats_host[l], "null pointer");
  }
  SD_REQUIRE(a.K == 0 || (out_grad && rois && trans && top_count), "null pointer");
  SD_REQUIRE(req_trans == SD_REQ_NULL || a.K == 0 || d_trans, "null pointer");
  hipStream_t st = (hipStream_t)stream;
  for (int l = 0; l < nlvl; ++l) {
    a.ddata[l] = req_data == SD_REQ_NULL ? nullptr : d_feats_host[l];
    const size_t bytes = (size_t)B * C * Hs_host[l] * Ws_host[l] * sizeof(float);
    if (req_data == SD_REQ_WRITE && bytes) SD_HIP_CHECK(hipMemsetAsync(d_feats_host[l], 0, bytes, st));
  }
  if (a.K == 0 || (req_data == SD_REQ_NULL && req_trans == SD_REQ_NULL)) return SD_OK;
  a.rois = rois; a.trans = trans; a.dy = out_grad; a.tc = top_count; a.dtrans = d_trans;
  a.req_trans = req_trans;
  return dp_launch_bwd(a, st);
}
