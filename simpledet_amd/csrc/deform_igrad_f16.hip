// DeformableConvolution in fp16 for gfx950: the data and offset gradients on the half operands as they lie
// (DESIGN 4.29), and the backward entry point that uses them.
//   dcn_igrad_f16_prep_weight_kernel   W^T in matrix-core fragment order, once per call
//   dcn_dcol_doff_f16_kernel           dcol = W^T dY per (image, group, 64-pixel tile); d_offset taken from the fp32
//                                      accumulators in the tile, dcol rounded once to fp16 for the data gradient
//   dcn_col2im_f16_kernel              d_data from the fp16 dcol, fp32 sums of a band in LDS
//   dcn_bias_grad_f16_kernel           d_bias from dY as it lies (dcn_bias_grad_kernel's order on widened loads)
#include "deform_f16_common.h"
#pragma clang fp contract(off)

namespace sd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kIN = 64, kIThreads = 256;
constexpr int kIFc = 256;                          // filters of one dY chunk in LDS
constexpr int kIRowB = kIFc * 2 + 16;              // bytes of a B row: [pixel][filter] + the bank shift of 4.28
constexpr int kIBBytes = kIN * kIRowB;             // 33792
constexpr int kIWinPos = 1280;                     // positions of the largest x window
constexpr int kIXBytes = kIWinPos / 8 * 9 * 32;    // 46080: 4.27's channel-interleaved slots
constexpr int kIDBytes = 9 * kIN * 16 * 4;         // 36864: the fp32 dcol block [tap][pixel][16 channels]
constexpr int kISmem = kIBBytes + kIXBytes + kIDBytes + 64;   // 116800: one workgroup per CU
constexpr int kISt = (9 * kIN + kIThreads - 1) / kIThreads;   // (tap, pixel) items of a thread

// ------------------------------------------------------------------------------------------------
// The A operand of dcol[144 x 64] = W^T[144 x F] . dY[F x 64]: rows are (tap, channel of a 16-channel slab), one
// 16-row block per tap, k is the filter -- stride 9 C in weight (F, C, 3, 3).  wre[slab][k step of 32][tap][lane]
// holds lane l's fragment of v_mfma_f32_16x16x32_f16: row l % 16 = channel, k = (l / 16) * 8 .. + 7.  A copy: the
// halves are untouched; filters beyond F are zero.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dcn_igrad_f16_prep_weight_kernel(const unsigned short* __restrict__ w,
                                                                        u32x4* __restrict__ wre, int F, int C,
                                                                        int ksteps, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int lane = (int)(e & 63);
  long r = e >> 6;
  const int tap = (int)(r % 9);
  r /= 9;
  const int ks = (int)(r % ksteps), slab = (int)(r / ksteps);
  const int c = slab * 16 + (lane & 15), f0 = ks * 32 + (lane >> 4) * 8;
  u32x4 v = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned h = f0 + j < F ? w[((long)(f0 + j) * C + c) * 9 + tap] : 0u;
    v[j >> 1] |= h << (16 * (j & 1));
  }
  wre[e] = v;
}

struct DcnIgradArgs {
  const __half* x;
  const __half* offset;
  const __half* dy;
  const u32x4* wre;
  __half* dcol;          // [image][slab][tap][pixel][16 channels], or null: d_offset alone
  __half* doff;
  DcnGeom g;
  int F, ksteps, nslab, tiles, req_off;
};

// ------------------------------------------------------------------------------------------------
// A workgroup of four waves owns (image, deformable group, 64-pixel tile) and walks the group's 16-channel slabs.
//   B      the (F x 64) tile of dY, loaded once (ldg8_f16: pixels behind the plane's end are zero, never read) and
//          written TRANSPOSED into LDS, B[pixel][filter]: a matrix-core lane reads one pixel x 8 consecutive filters
//          as one 16-byte read.  F > 256 runs in chunks of 256 filters, reloaded per slab, the accumulators carried.
//   mma    wave w owns pixels 16 w .. 16 w + 15 and all nine taps: nine 16 x 16 blocks, 36 accumulator registers;
//          A from the pre-laid weights (L2 / L1).  A lane's four rows are four consecutive channels of one tap.
//   dcol16 each accumulator rounded once (RNE), one 8-byte store per lane and tap, channel-last: a (tap, pixel)
//          item of the data gradient is 32 contiguous bytes.
//   doff   the unrounded block goes to LDS [tap][pixel][16]; thread t owns the (tap, pixel) items t, t + 256, t + 512:
//          deform_col2im_coord_kernel's sampling state in registers (computed once), the slab's x window in LDS
//          (4.27's layout; a window of more than 1280 positions: corners from global memory, workgroup-uniform), and
//          per channel, ascending, weight = f1 x1 + f2 x2 + f3 x3 + f4 x4 in that kernel's order, val += weight *
//          dcol32 -- the sums stay in the owner's registers across the slabs.  One rounding at the end.
// No atomics, a fixed order: two calls give equal bits.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kIThreads) void dcn_dcol_doff_f16_kernel(DcnIgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ism[];
  char* const Bs = ism;
  char* const xs = ism + kIBBytes;
  float* const dcs = reinterpret_cast<float*>(ism + kIBBytes + kIXBytes);
  int* const rng = reinterpret_cast<int*>(ism + kIBBytes + kIXBytes + kIDBytes);
  const DcnGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = g.Ho * g.Wo, plane = g.H * g.W;
  const int tile = (int)blockIdx.x % a.tiles, ng = (int)blockIdx.x / a.tiles;
  const int grp = ng % g.dgroup, n = ng / g.dgroup;
  const int p0 = tile * kIN;
  const int cpg = g.C / g.dgroup, ns = cpg / 16;
  const __half* const dyn = a.dy + (long)n * a.F * P;
  const bool want_off = a.req_off != SD_REQ_NULL;

  // ---- the sampling state of the thread's (tap, pixel) items: deform_col2im_coord_kernel's arithmetic ----
  int sbase[kISt], sflag[kISt];
  float fa[kISt], fb[kISt], fc[kISt], fd[kISt], val[kISt][2];
  int wstart = 0, wcount = 0;
  bool fits = true;
#pragma unroll
  for (int k = 0; k < kISt; ++k) {
    sbase[k] = 0; sflag[k] = 0;
    fa[k] = fb[k] = fc[k] = fd[k] = 0.f;
    val[k][0] = val[k][1] = 0.f;
  }
  if (want_off) {
#pragma unroll
    for (int k = 0; k < kISt; ++k) {
      const int item = tid + k * kIThreads;
      const int tap = item / kIN, p = p0 + item % kIN;
      if (item < 9 * kIN && p < P) {
        const int h_out = p / g.Wo, w_out = p % g.Wo;
        const int h_in = h_out * g.stride_h - g.pad_h, w_in = w_out * g.stride_w - g.pad_w;
        const __half* off = a.offset + (((long)n * g.dgroup + grp) * 18 + 2 * tap) * P + p;
        const float offset_h = __half2float(off[0]), offset_w = __half2float(off[P]);
        const int i = tap / 3, j = tap - 3 * i;
        float inv_h = h_in + i * g.dil_h + offset_h;
        float inv_w = w_in + j * g.dil_w + offset_w;
        if (inv_h < 0 || inv_w < 0 || inv_h >= g.H || inv_w >= g.W) inv_h = inv_w = -1;
        float argmax_h = inv_h, argmax_w = inv_w;
        const bool zero = argmax_h < 0 || argmax_h > g.H || argmax_w < 0 || argmax_w > g.W;
        if (!zero) {
          int hl = (int)argmax_h, wl = (int)argmax_w, hh, wh;
          if (hl >= g.H - 1) {
            hh = hl = g.H - 1;
            argmax_h = (float)hl;
          } else {
            hh = hl + 1;
          }
          if (wl >= g.W - 1) {
            wh = wl = g.W - 1;
            argmax_w = (float)wl;
          } else {
            wh = wl + 1;
          }
          fa[k] = (wl + 1 - argmax_w); fb[k] = (argmax_w - wl);
          fc[k] = (hl + 1 - argmax_h); fd[k] = (argmax_h - hl);
          // (a NaN offset passes the tests above: its corners are clamped into the plane, its factors are NaN)
          hl = iminr(imaxr(hl, 0), g.H - 1); hh = iminr(imaxr(hh, 0), g.H - 1);
          wl = iminr(imaxr(wl, 0), g.W - 1); wh = iminr(imaxr(wh, 0), g.W - 1);
          sbase[k] = hl * g.W + wl;
          sflag[k] = (wh > wl ? 1 : 0) | (hh > hl ? 2 : 0) | 4;
        }
      }
    }
    // the contiguous range of plane positions the tile's corners touch: the x window of every slab
    if (tid == 0) {
      rng[0] = 0x7fffffff;
      rng[1] = -1;
    }
    int lo = 0x7fffffff, hi = -1;
#pragma unroll
    for (int k = 0; k < kISt; ++k)
      if (sflag[k]) {
        lo = iminr(lo, sbase[k]);
        hi = imaxr(hi, sbase[k] + ((sflag[k] & 2) ? g.W : 0) + (sflag[k] & 1));
      }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      lo = iminr(lo, __shfl_xor(lo, o));
      hi = imaxr(hi, __shfl_xor(hi, o));
    }
    __syncthreads();
    if (lane == 0 && hi >= 0) {
      atomicMin(&rng[0], lo);
      atomicMax(&rng[1], hi);
    }
    __syncthreads();
    lo = rng[0];
    hi = rng[1];
    wstart = hi >= 0 ? (lo & ~7) : 0;
    wcount = hi >= 0 ? ((hi + 1 - wstart + 7) & ~7) : 0;   // (the last group of eight may end behind the plane)
    fits = wcount <= kIWinPos;
#pragma unroll
    for (int k = 0; k < kISt; ++k) sbase[k] -= sflag[k] ? wstart : 0;
  }

  const int nchunk = (a.F + kIFc - 1) / kIFc;
  const int pl = wave * 16 + (lane & 15), cq = lane >> 4;   // the lane's pixel and channel quad in the D blocks
  for (int sl = 0; sl < ns; ++sl) {
    const int slab = grp * ns + sl;
    const __half* const xg = a.x + ((long)n * g.C + slab * 16) * plane;   // channel 0 of the slab
    __syncthreads();   // the previous slab is done with the window, the dcol block and B
    if (want_off && fits)
      for (int it = tid; it < wcount; it += kIThreads) {   // item -> (position group, channel pair)
        const int pg = it >> 3, cp = it & 7;
        const __half* src = xg + (long)(2 * cp) * plane + wstart + 8 * pg;
        const int nv = plane - (wstart + 8 * pg);
        const u32x4 va = ldg8_f16(src, nv), vb = ldg8_f16(src + plane, nv);
        xwin_store(xs, pg, cp, va, vb);
      }
    f32x4 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[tap] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ch = 0; ch < nchunk; ++ch) {
      const int kc = iminr(kIFc / 32, a.ksteps - ch * (kIFc / 32));   // k steps of the chunk
      if (nchunk > 1 || sl == 0) {
        if (ch > 0) __syncthreads();   // every wave is done with the previous chunk
        for (int it = tid; it < kc * 32 * 8; it += kIThreads) {   // item -> (filter row, group of eight pixels)
          const int row = it >> 3, pg = it & 7;
          const int f = ch * kIFc + row, p = p0 + pg * 8;
          u32x4 v = {0u, 0u, 0u, 0u};
          if (f < a.F) v = ldg8_f16(dyn + (long)f * P + p, P - p);
          unsigned short* bw = reinterpret_cast<unsigned short*>(Bs + (pg * 8) * kIRowB) + row;
#pragma unroll
          for (int j = 0; j < 8; ++j) bw[j * (kIRowB / 2)] = (unsigned short)((v[j >> 1] >> (16 * (j & 1))) & 0xffffu);
        }
        __syncthreads();
      }
      const char* brd = Bs + pl * kIRowB + cq * 16;
      const u32x4* ap = a.wre + ((long)(slab * a.ksteps + ch * (kIFc / 32)) * 9) * 64 + lane;
      for (int ks = 0; ks < kc; ++ks) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(brd + ks * 64);
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
          acc[tap] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8, ap[(ks * 9 + tap) * 64]),
                                                            __builtin_bit_cast(halfx8, b), acc[tap], 0, 0, 0);
      }
    }
    // ---- D layout of a 16x16 block: element e of lane l -> row (channel) (l / 16) * 4 + e, column (pixel) l % 16 ----
    if (a.dcol && p0 + pl < P) {
      __half* dc = a.dcol + ((((long)n * a.nslab + slab) * 9) * P + p0 + pl) * 16 + cq * 4;
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const floatx2 v0 = {acc[tap][0], acc[tap][1]}, v1 = {acc[tap][2], acc[tap][3]};
        u32x2 o;
        o[0] = __builtin_bit_cast(unsigned, __builtin_convertvector(v0, halfx2));
        o[1] = __builtin_bit_cast(unsigned, __builtin_convertvector(v1, halfx2));
        *reinterpret_cast<u32x2*>(dc + (long)tap * P * 16) = o;
      }
    }
    if (!want_off) continue;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) *reinterpret_cast<f32x4*>(dcs + (tap * kIN + pl) * 16 + cq * 4) = acc[tap];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kISt; ++k) {
      if (!sflag[k]) continue;   // outside the image, behind the plane's end, or no such item: the sum stays 0
      const int item = tid + k * kIThreads;
      const float* dv = dcs + ((item / kIN) * kIN + item % kIN) * 16;
      const int c1 = sbase[k], c2 = c1 + (sflag[k] & 1), c3 = c1 + ((sflag[k] & 2) ? g.W : 0), c4 = c3 + (sflag[k] & 1);
      const float h1 = -1 * fa[k], h2 = -1 * fb[k], h3 = fa[k], h4 = fb[k];   // bp_dir 0
      const float w1 = -1 * fc[k], w2 = fc[k], w3 = -1 * fd[k], w4 = fd[k];   // bp_dir 1
      float v0 = val[k][0], v1 = val[k][1];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        u32x4 va = {0u, 0u, 0u, 0u}, vb = va, vc = va, vd = va;
        if (fits) {
          const char* xh = xs + hf * 16;
          va = *reinterpret_cast<const u32x4*>(xh + (c1 + (c1 >> 3)) * 32);
          vb = *reinterpret_cast<const u32x4*>(xh + (c2 + (c2 >> 3)) * 32);
          vc = *reinterpret_cast<const u32x4*>(xh + (c3 + (c3 >> 3)) * 32);
          vd = *reinterpret_cast<const u32x4*>(xh + (c4 + (c4 >> 3)) * 32);
        } else {   // every address inside the plane
          const unsigned short* xc = reinterpret_cast<const unsigned short*>(xg + (long)(hf * 8) * plane + wstart);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const unsigned short* e0 = xc + (long)(2 * q) * plane;
            const unsigned short* e1 = e0 + plane;
            va[q] = (unsigned)e0[c1] | ((unsigned)e1[c1] << 16);
            vb[q] = (unsigned)e0[c2] | ((unsigned)e1[c2] << 16);
            vc[q] = (unsigned)e0[c3] | ((unsigned)e1[c3] << 16);
            vd[q] = (unsigned)e0[c4] | ((unsigned)e1[c4] << 16);
          }
        }
        const f32x4 d0 = *reinterpret_cast<const f32x4*>(dv + hf * 8), d1 = *reinterpret_cast<const f32x4*>(dv + hf * 8 + 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          // (by value: __builtin_bit_cast on the element expression itself reads element 0 of the vector)
          const unsigned ua = va[q], ub = vb[q], uc = vc[q], ud = vd[q];
          const floatx2 x1 = __builtin_convertvector(__builtin_bit_cast(halfx2, ua), floatx2);
          const floatx2 x2 = __builtin_convertvector(__builtin_bit_cast(halfx2, ub), floatx2);
          const floatx2 x3 = __builtin_convertvector(__builtin_bit_cast(halfx2, uc), floatx2);
          const floatx2 x4 = __builtin_convertvector(__builtin_bit_cast(halfx2, ud), floatx2);
#pragma unroll
          for (int e = 0; e < 2; ++e) {   // channels hf * 8 + 2 q + e, ascending
            const float dc32 = q < 2 ? d0[2 * q + e] : d1[2 * q - 4 + e];
            float weight = 0;
            weight += h1 * x1[e];
            weight += h2 * x2[e];
            weight += h3 * x3[e];
            weight += h4 * x4[e];
            v0 += weight * dc32;
            weight = 0;
            weight += w1 * x1[e];
            weight += w2 * x2[e];
            weight += w3 * x3[e];
            weight += w4 * x4[e];
            v1 += weight * dc32;
          }
        }
      }
      val[k][0] = v0;
      val[k][1] = v1;
    }
  }
  if (!want_off) return;
#pragma unroll
  for (int k = 0; k < kISt; ++k) {
    const int item = tid + k * kIThreads;
    const int tap = item / kIN, p = p0 + item % kIN;
    if (item < 9 * kIN && p < P) {
      __half* out = a.doff + (((long)n * g.dgroup + grp) * 18 + 2 * tap) * P + p;
      out[0] = __float2half(a.req_off == SD_REQ_ADD ? __half2float(out[0]) + val[k][0] : val[k][0]);
      out[P] = __float2half(a.req_off == SD_REQ_ADD ? __half2float(out[P]) + val[k][1] : val[k][1]);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// The data gradient from dcol16, organised as deform_col2im_chunk_kernel (overlapping windows cannot
// stay in the producer's tile).  A workgroup owns (image, 16-channel slab, band of rows x columns) and keeps the
// band's 16 planes in LDS as fp32, plane-major.  It walks the 9 Ho Wo (tap, pixel) items of its image, rejects those
// whose rows miss the band, works the landing index and the 2 + 2 factors out once per item (col2im_geom; a factor
// whose column lies outside the band's columns is zero), reads the item's 16 channels as one 32-byte read, widens
// them and adds factor * value into the planes; then the band is written once, rounded once (req = add: onto the
// widened destination).  No global atomics.
// The LDS adds are NATIVE float adds (ds_add_f32) in hardware order: the last bits of the fp32 sums, and so a
// rounding of the fp16 result here and there, can differ between two calls.  Sums that are exact in fp32 do not.
// Band rule: at most kCBandPos positions per plane (64 KiB for 16 planes, two workgroups per CU).  W <= kCBandPos:
// whole rows, H split evenly into bands of <= kCBandPos / W rows.  Wider planes: one-row bands split evenly in
// columns of <= kCBandPos.
// ------------------------------------------------------------------------------------------------
constexpr int kCBandPos = 1024, kCThreads = 256;

struct DcnC2iArgs {
  const __half* dcol;
  const __half* offset;
  __half* dx;
  DcnGeom g;
  int nslab, band_rows, band_w, ncs, req_add;
};

__global__ __launch_bounds__(kCThreads) void dcn_col2im_f16_kernel(DcnC2iArgs a) {
  extern __shared__ __attribute__((aligned(16))) float cplane[];
  const DcnGeom& g = a.g;
  const int P = g.Ho * g.Wo, tid = threadIdx.x;
  const int slab = blockIdx.y, n = blockIdx.z;
  const int rb = (int)blockIdx.x / a.ncs, cs = (int)blockIdx.x % a.ncs;
  const int row0 = rb * a.band_rows, row1 = iminr(row0 + a.band_rows, g.H);
  const int col0 = cs * a.band_w, col1 = iminr(col0 + a.band_w, g.W);
  const int bw = col1 - col0, be = (row1 - row0) * bw;
  for (int i = tid; i < 16 * be; i += kCThreads) cplane[i] = 0.f;
  __syncthreads();
  const int grp = slab * 16 / (g.C / g.dgroup);
  const __half* off = a.offset + ((long)n * g.dgroup + grp) * 18 * P;
  const __half* dc = a.dcol + (((long)n * a.nslab + slab) * 9) * P * 16;
  for (int item = tid; item < 9 * P; item += kCThreads) {
    const int tap = item / P, p = item - tap * P;
    const int h_out = p / g.Wo, w_out = p - h_out * g.Wo;
    const int i = tap / 3, j = tap - 3 * i;
    const float offset_h = __half2float(off[(long)(2 * tap) * P + p]);
    const float offset_w = __half2float(off[(long)(2 * tap + 1) * P + p]);
    const float inv_h = h_out * g.stride_h - g.pad_h + i * g.dil_h + offset_h;
    const float inv_w = w_out * g.stride_w - g.pad_w + j * g.dil_w + offset_w;
    const int cur_h = (int)inv_h;
    if (cur_h + 1 < row0 || cur_h - 1 >= row1) continue;   // every touched row lies in [cur_h - 1, cur_h + 1]
    int base;
    float fhv[2], fwv[2];
    col2im_geom(g, inv_h, inv_w, row0, row1, base, fhv, fwv);
    const int fh = (int)floorf(inv_h), fw = (int)floorf(inv_w);
#pragma unroll
    for (int d = 0; d < 2; ++d)
      if (fw + d < col0 || fw + d >= col1) fwv[d] = 0.f;
    float wt[4];
    bool any = false;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      wt[d] = fhv[d >> 1] * fwv[d & 1];
      any = any || wt[d] != 0.f;
    }
    if (!any) continue;
    const u32x4* src = reinterpret_cast<const u32x4*>(dc + ((long)tap * P + p) * 16);
    const u32x4 q0 = src[0], q1 = src[1];
    float v[16];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const floatx2 f = __builtin_convertvector(__builtin_bit_cast(halfx2, k < 4 ? q0[k & 3] : q1[k & 3]), floatx2);
      v[2 * k] = f[0];
      v[2 * k + 1] = f[1];
    }
    const int idx0 = (fh - row0) * bw + (fw - col0);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (wt[d] != 0.f) {   // a nonzero factor: its row and column lie inside the band
        float* q = cplane + idx0 + (d >> 1) * bw + (d & 1);
#pragma unroll
        for (int c = 0; c < 16; ++c)
          __hip_atomic_fetch_add(q + c * be, wt[d] * v[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      }
  }
  __syncthreads();
  for (int c = 0; c < 16; ++c) {
    __half* d = a.dx + (((long)n * g.C + slab * 16 + c) * g.H + row0) * g.W + col0;
    const float* pln = cplane + c * be;
    for (int i = tid; i < be; i += kCThreads) {
      const int r = i / bw;
      __half* o = d + (long)r * g.W + (i - r * bw);
      *o = __float2half(a.req_add ? __half2float(*o) + pln[i] : pln[i]);
    }
  }
}

// d_bias[f] (+)= sum over n, pixels of dY: dcn_bias_grad_kernel's order and tree on widened loads, one rounding --
// the bits of the default route (widen dY, that kernel, sd_cast_f32_to_f16)
__global__ __launch_bounds__(256) void dcn_bias_grad_f16_kernel(const __half* __restrict__ dy, __half* __restrict__ dbias,
                                                                int N, int F, int P, int add) {
  const int f = blockIdx.x;
  float acc = 0.f;
  for (int n = 0; n < N; ++n) {
    const __half* r = dy + ((long)n * F + f) * P;
    for (int p = threadIdx.x; p < P; p += 256) acc += __half2float(r[p]);
  }
  __shared__ float sm[256];
  sm[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int o = 128; o >= 1; o >>= 1) {
    if ((int)threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) dbias[f] = __float2half(add ? __half2float(dbias[f]) + sm[0] : sm[0]);
}

static size_t igrad_wre_bytes(int C, int F) { return (size_t)(C / 16) * ((F + 31) / 32) * 9 * 64 * sizeof(u32x4); }

}  // namespace sd

using namespace sd;

static size_t igrad_base_bytes(int N, int C, int H, int W, int F, int kh, int kw, int pad, int stride, int dil,
                               int dgroup, int num_group, int fused_weight_grad, int pixel_runs) {
  return fused_weight_grad ? sd_deform_convolution_bwd_workspace_bytes_f16_fused(N, C, H, W, F, kh, kw, pad, stride, dil,
                                                                                 dgroup, num_group, pixel_runs)
                           : sd_deform_convolution_bwd_workspace_bytes_f16(N, C, H, W, F, kh, kw, pad, stride, dil,
                                                                           dgroup, num_group);
}

extern "C" size_t sd_deform_convolution_bwd_workspace_bytes_f16_native(int N, int C, int H, int W, int F, int kh,
                                                                       int kw, int pad, int stride, int dil,
                                                                       int dgroup, int num_group,
                                                                       int fused_weight_grad, int pixel_runs) {
  const size_t base = igrad_base_bytes(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group, fused_weight_grad,
                                       pixel_runs);
  long Ho, Wo;
  if (N <= 0 || C <= 0 || F <= 0 || pixel_runs < 0 || !dcn_f16_fused_ok(C, H, W, kh, kw, dgroup, num_group) ||
      !out_hw(H, W, kh, kw, pad, stride, dil, Ho, Wo))
    return base;
  return round256(base) + round256(igrad_wre_bytes(C, F)) + (size_t)N * (C / 16) * 9 * Ho * Wo * 16 * sizeof(__half) +
         512;
}

extern "C" int sd_deform_convolution_bwd_f16_native(const void* out_grad, const void* x, const void* offset,
                                                    const void* weight, void* d_x, void* d_offset, void* d_weight,
                                                    void* d_bias, int req_x, int req_offset, int req_weight,
                                                    int req_bias, int N, int C, int H, int W, int F, int kh, int kw,
                                                    int pad, int stride, int dil, int dgroup, int num_group,
                                                    int fused_weight_grad, int pixel_runs, void* workspace,
                                                    size_t workspace_bytes, void* stream) {
  SD_REQUIRE(pixel_runs >= 0, "pixel_runs must be >= 0");
  auto parent = [&](int rx, int ro, int rw, int rb, size_t bytes) {
    return fused_weight_grad
               ? sd_deform_convolution_bwd_f16_fused(out_grad, x, offset, weight, d_x, d_offset, d_weight, d_bias, rx,
                                                     ro, rw, rb, N, C, H, W, F, kh, kw, pad, stride, dil, dgroup,
                                                     num_group, pixel_runs, workspace, bytes, stream)
               : sd_deform_convolution_bwd_f16(out_grad, x, offset, weight, d_x, d_offset, d_weight, d_bias, rx, ro,
                                               rw, rb, N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group,
                                               workspace, bytes, stream);
  };
  if (!dcn_f16_fused_ok(C, H, W, kh, kw, dgroup, num_group) || N <= 0 ||
      (req_x == SD_REQ_NULL && req_offset == SD_REQ_NULL))
    return parent(req_x, req_offset, req_weight, req_bias, workspace_bytes);
  DcnGeom g;
  if (int e = make_geom(g, N, C, H, W, kh, kw, pad, pad, stride, stride, dil, dil, dgroup)) return e;
  SD_REQUIRE(F > 0, "num_filter must be positive");
  const int reqs[4] = {req_x, req_offset, req_weight, req_bias};
  void* const dst[4] = {d_x, d_offset, d_weight, d_bias};
  for (int i = 0; i < 4; ++i) {
    SD_REQUIRE(reqs[i] == SD_REQ_NULL || reqs[i] == SD_REQ_WRITE || reqs[i] == SD_REQ_ADD, "bad req %d", reqs[i]);
    SD_REQUIRE(reqs[i] == SD_REQ_NULL || dst[i], "a requested gradient is null");
  }
  SD_REQUIRE(out_grad && x && offset && weight, "null tensor pointer");
  SD_REQUIRE((((uintptr_t)out_grad | (uintptr_t)x | (uintptr_t)offset | (uintptr_t)weight | (uintptr_t)d_x |
               (uintptr_t)d_offset | (uintptr_t)d_weight | (uintptr_t)d_bias) & 1) == 0,
             "half tensors must be aligned to 2 bytes");
  const size_t base = igrad_base_bytes(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group, fused_weight_grad,
                                       pixel_runs);
  const size_t need = sd_deform_convolution_bwd_workspace_bytes_f16_native(N, C, H, W, F, kh, kw, pad, stride, dil,
                                                                           dgroup, num_group, fused_weight_grad,
                                                                           pixel_runs);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "DeformableConvolution (fp16 backward, native) workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const long P = (long)g.Ho * g.Wo;
  // d_weight: 4.28's kernel or the default route, in the front part of the workspace
  if (req_weight != SD_REQ_NULL)
    if (int e = parent(SD_REQ_NULL, SD_REQ_NULL, req_weight, SD_REQ_NULL, base)) return e;
  if (req_bias != SD_REQ_NULL) {
    hipLaunchKernelGGL(dcn_bias_grad_f16_kernel, dim3(F), dim3(256), 0, st, (const __half*)out_grad, (__half*)d_bias,
                       N, F, (int)P, req_bias == SD_REQ_ADD ? 1 : 0);
    SD_LAUNCH_CHECK();
  }
  const int nslab = C / 16, ksteps = (F + 31) / 32, tiles = cdiv(P, kIN);
  SD_REQUIRE(N < 65536 && nslab < 65536 && (long)N * dgroup * tiles < (1L << 31) &&
                 (long)nslab * ksteps * 9 * 64 < (1L << 31),
             "too many workgroups");
  u32x4* wre = reinterpret_cast<u32x4*>(round256((size_t)(uintptr_t)workspace + round256(base)));
  __half* dcol = reinterpret_cast<__half*>(reinterpret_cast<char*>(wre) + round256(igrad_wre_bytes(C, F)));
  {
    const long total = (long)nslab * ksteps * 9 * 64;
    hipLaunchKernelGGL(dcn_igrad_f16_prep_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const unsigned short*)weight, wre, F, C, ksteps, total);
    SD_LAUNCH_CHECK();
  }
  DcnIgradArgs a{};
  a.x = (const __half*)x; a.offset = (const __half*)offset; a.dy = (const __half*)out_grad; a.wre = wre;
  a.dcol = req_x != SD_REQ_NULL ? dcol : nullptr;
  a.doff = (__half*)d_offset; a.g = g; a.F = F; a.ksteps = ksteps; a.nslab = nslab; a.tiles = tiles;
  a.req_off = req_offset;
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)dcn_dcol_doff_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kISmem));
  hipLaunchKernelGGL(dcn_dcol_doff_f16_kernel, dim3((unsigned)((long)N * dgroup * tiles)), dim3(kIThreads), kISmem, st,
                     a);
  SD_LAUNCH_CHECK();
  if (req_x == SD_REQ_NULL) return SD_OK;
  DcnC2iArgs c{};
  c.dcol = dcol; c.offset = (const __half*)offset; c.dx = (__half*)d_x; c.g = g; c.nslab = nslab;
  c.req_add = req_x == SD_REQ_ADD ? 1 : 0;
  int nrb;
  if (W <= kCBandPos) {
    nrb = cdiv(H, kCBandPos / W);
    c.band_rows = cdiv(H, nrb);
    c.band_w = W;
    c.ncs = 1;
  } else {
    nrb = H;
    c.band_rows = 1;
    c.ncs = cdiv(W, kCBandPos);
    c.band_w = cdiv(W, c.ncs);
  }
  nrb = cdiv(H, c.band_rows);
  SD_REQUIRE((long)nrb * c.ncs < (1L << 31), "too many bands");
  const size_t smem = sizeof(float) * 16 * (size_t)c.band_rows * c.band_w;
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)dcn_col2im_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)smem));
  hipLaunchKernelGGL(dcn_col2im_f16_kernel, dim3((unsigned)(nrb * c.ncs), (unsigned)nslab, (unsigned)N), dim3(kCThreads),
                     smem, st, c);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
