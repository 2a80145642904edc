// DeformableConvolution in fp16 for gfx950: a col-free forward on native-half matrix-core operands
// (DESIGN 4.27), and the operator's fp16 entry points around it.
#include "deform_f16_common.h"
#pragma clang fp contract(off)

// the variant (DESIGN 4.27 has the alternatives and their times): pixel slots of a tile and matrix-core waves
#ifndef SD_DCNH_NP
#define SD_DCNH_NP 64
#endif
#ifndef SD_DCNH_MMA
#define SD_DCNH_MMA 4
#endif

namespace sd {

// ------------------------------------------------------------------------------------------------
// y = W . col(x, offset) on halves, without the col matrix.  A workgroup owns (image, tile of <= kHN
// output pixels) and 256 filters, as the fp32 kernel of deform_fused.hip does, but the pipeline is
// re-planned around what halves change: one matrix-core term per product instead of three, so the
// sampling waves, not the matrix cores, set the pace (DESIGN 4.27 has the wave splits measured).
//   K order   k = (slab of 16 channels, tap, channel): one k16 matrix-core step = one (slab, tap) unit.
//   x         the window of a slab's 16 channel planes that the tile's samples of a deformable group
//             touch, in LDS as halves, the 16 channels of a position side by side (32 bytes): a corner's
//             eight channels are ONE 16-byte read.  Every eight positions are followed by one empty slot,
//             so the loaders' 4-byte stores (eight channel pairs x eight position groups per wave) and
//             the samplers' 16-byte reads spread over all banks.  Two window buffers.
//   B         a whole SLAB of B at a time: 9 taps x kHN pixels x 16 k, one 16-byte granule per
//             (tap, pixel, k8), sample rounded once to fp16.  Two slab buffers, so the pipeline hands over
//             once per slab: ONE workgroup barrier per nine matrix-core steps.
//   A         the fp16 weights as they are, re-ordered once per call by dcn_f16_prep_weight_kernel into
//             the per-lane fragment order; each matrix-core wave loads its filter rows from L2 one step
//             ahead.
//   roles     waves 0..kHMma-1: matrix cores (256 / kHMma filter rows x kHN pixels each);
//             the other waves: in interval s they load the window of slab s + 2 into registers, sample
//             slab s + 1 out of its window into B[(s + 1) & 1] while the matrix cores consume B[s & 1],
//             then store the registers into the window buffer slab s was sampled from.  A sampling lane
//             keeps ONE (pixel, k8) for the whole kernel and walks the taps.
//   A group whose window does not fit a buffer (wild offsets) samples its corners from global memory
//   instead, in the same kernel, the same pipeline and the same arithmetic: a workgroup-uniform branch.
// Arithmetic: offsets and corners widened to fp32, sd_deform_im2col's expression in its order, one RNE to
// fp16 (the B element); fp16 weights untouched; single-term v_mfma_f32_32x32x16_f16 into fp32; bias
// widened and added in fp32; one RNE to fp16.
// ------------------------------------------------------------------------------------------------
constexpr int kHN = SD_DCNH_NP, kHMma = SD_DCNH_MMA, kHThreads = 512;
constexpr int kHLanes = kHThreads - 64 * kHMma;      // sampling lanes
constexpr int kHPB = kHN / 32;                       // 32-pixel blocks of a tile
constexpr int kHFr = 8 / kHMma;                      // 32-filter fragments per matrix-core wave
constexpr int kHTapStride = kHLanes / (2 * kHN);     // a sampling lane takes every kHTapStride-th tap
constexpr int kHTapIters = (9 + kHTapStride - 1) / kHTapStride;
static_assert(kHN % 32 == 0 && 8 % kHMma == 0 && kHLanes % (2 * kHN) == 0, "variant does not tile");
constexpr int kHBHalf = kHN * 16 + 64;               // granules of one k8 of a step (+ a bank shift)
constexpr int kHBStep = 2 * kHBHalf, kHBBuf = 9 * kHBStep;
constexpr int kHStateBytes = 9 * 3 * kHN * 8;        // sampling state [tap][word][pixel], 8-byte words
constexpr int kHXSlots = (160 * 1024 - 2 * kHBBuf - kHStateBytes - 64) / 64;   // 32-byte slots of one window buffer
constexpr int kHMaxW = (kHXSlots * 8 / 9) & ~7;      // positions of the largest window
constexpr int kHStage = (kHMaxW + kHLanes - 1) / kHLanes;   // (position group, channel pair) items per sampling lane
constexpr int kHSmem = 2 * kHXSlots * 32 + 2 * kHBBuf + kHStateBytes + 64;

struct DcnF16Args {
  const __half* x;
  const __half* offset;
  const u32x4* wre;      // weights in fragment order (dcn_f16_prep_weight_kernel)
  const __half* bias;    // (F) or null
  __half* y;
  DcnGeom g;
  int F, mtiles, nslab, tiles_per_image, tile_w;
  int by_xcd;            // 1: tile t of image n runs on XCD n % 8 (N >= 8); 0: tiles dealt over all XCDs
};

// weights (F, C, 9) -> wre[mt][slab][tap][fragment 0..7][lane] (16 bytes each): lane l of fragment r holds
// filter row mt*256 + r*32 + (l & 31) and channels slab*16 + (l >> 5)*8 .. +7 of the tap; rows past F are 0
__global__ __launch_bounds__(256) void dcn_f16_prep_weight_kernel(const unsigned short* __restrict__ w,
                                                                  u32x4* __restrict__ wre, int F, int C, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int lane = (int)(e & 63), frag = (int)((e >> 6) & 7);
  long r = e >> 9;
  const int tap = (int)(r % 9); r /= 9;
  const int nslab = C / 16;
  const int slab = (int)(r % nslab), mt = (int)(r / nslab);
  const int f = mt * 256 + frag * 32 + (lane & 31), c0 = slab * 16 + (lane >> 5) * 8;
  u32x4 o = {0u, 0u, 0u, 0u};
  if (f < F) {
    const unsigned short* s = w + ((long)f * C + c0) * 9 + tap;
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = (unsigned)s[(2 * k) * 9] | ((unsigned)s[(2 * k + 1) * 9] << 16);
  }
  wre[e] = o;
}

__global__ __launch_bounds__(kHThreads) void dcn_fwd_fused_f16_kernel(DcnF16Args a) {
  extern __shared__ __attribute__((aligned(16))) char hsm[];
  char* const xs = hsm;                                  // two window buffers
  char* const Bs = hsm + 2 * kHXSlots * 32;              // two slab buffers of B
  float2* const sst = reinterpret_cast<float2*>(Bs + 2 * kHBBuf);
  int* const rng = reinterpret_cast<int*>(Bs + 2 * kHBBuf + kHStateBytes);
  const DcnGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = g.Ho * g.Wo, plane = g.H * g.W;
  // block -> (filter tile, image, pixel tile); the tiles of image n run on XCD n % 8
  const int per_mt = (int)gridDim.x / a.mtiles;
  const int mt = (int)blockIdx.x / per_mt, bb = (int)blockIdx.x % per_mt;
  // (with fewer than eight images that would leave XCDs idle: the tiles are then dealt over all of them)
  const int xcd = bb & 7, slot = bb >> 3;
  const int n = a.by_xcd ? (slot / a.tiles_per_image) * 8 + xcd : bb / a.tiles_per_image;
  const int t = a.by_xcd ? slot % a.tiles_per_image : bb % a.tiles_per_image;
  if (n >= g.N) return;
  const int p0 = t * a.tile_w, p1 = iminr(p0 + a.tile_w, P);
  if (p0 >= P) return;
  const int cpg = g.C / g.dgroup, ns = cpg / 16;
  const bool mma = wave < kHMma;
  // a sampling lane's (pixel, k8) and first tap
  const int sid = mma ? 0 : tid - 64 * kHMma;
  const int pl = (sid % (2 * kHN)) >> 1, half = sid & 1, tap0 = sid / (2 * kHN);
  // a matrix-core wave's fragments: rows mt*256 + (wave*kHFr + i)*32 .. +31, those below F only
  const int frag0 = (mma ? wave : 0) * kHFr;
  const int nf = imaxr(0, iminr(kHFr, (a.F - mt * 256 - frag0 * 32 + 31) / 32));

  // ---- per group, every wave (same barriers in every role): the sampling state of the 9 taps into LDS, the
  // window the samples touch, slab 0 of it ----
  struct Grp { int wstart, wcount; bool fits; const __half* xg; };
  auto win_load = [&](const Grp& G, int it, int slab, u32x4& va, u32x4& vb) {   // item -> (position group, channel pair)
    const int pg = it >> 3, cp = it & 7;
    const __half* src = G.xg + (long)(slab * 16 + 2 * cp) * plane + G.wstart + 8 * pg;
    const int nv = plane - (G.wstart + 8 * pg);
    va = ldg8_f16(src, nv);
    vb = ldg8_f16(src + plane, nv);
  };
  auto group_begin = [&](int grp) -> Grp {
    // sampling state of the group's (tap, pixel) pairs, by everybody
    int sbase[2], sflag[2];
    float sw[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int item = tid + k * kHThreads;
      const int tap = item / kHN, p = p0 + item % kHN;
      sbase[k] = 0; sflag[k] = 0;
      sw[k][0] = sw[k][1] = sw[k][2] = sw[k][3] = 0.f;
      if (item < 9 * kHN && p < p1) {
        const int h_col = p / g.Wo, w_col = p % g.Wo;
        const __half* off = a.offset + (((long)n * g.dgroup + grp) * 18 + 2 * tap) * P + p;
        const float oh = __half2float(off[0]), ow = __half2float(off[P]);
        const int ti = tap / 3;
        const Sample s = im2col_sample(g, h_col * g.stride_h - g.pad_h, w_col * g.stride_w - g.pad_w, ti,
                                       tap - 3 * ti, oh, ow);
        if (s.ok) {
          sbase[k] = s.h_low * g.W + s.w_low;
          sflag[k] = (s.w_high - s.w_low) | ((s.h_high - s.h_low) << 1) | 4;
          sw[k][0] = s.w1; sw[k][1] = s.w2; sw[k][2] = s.w3; sw[k][3] = s.w4;
        }
      }
    }
    __syncthreads();   // (the previous group is done with the state, the windows and B)
    if (tid == 0) {
      rng[0] = 0x7fffffff;
      rng[1] = -1;
    }
    int lo = 0x7fffffff, hi = -1;
#pragma unroll
    for (int k = 0; k < 2; ++k)
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
    // the window: positions [wstart, wstart + wcount) of a plane, whole groups of eight (the last group may end
    // behind the plane: its tail is neither loaded nor read)
    const int wstart = hi >= 0 ? (lo & ~7) : 0;
    const int wcount = hi >= 0 ? ((hi + 1 - wstart + 7) & ~7) : 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int item = tid + k * kHThreads;
      if (item < 9 * kHN) {
        float2* d = sst + (item / kHN) * 3 * kHN + item % kHN;
        d[0] = make_float2(__int_as_float(sflag[k] ? sbase[k] - wstart : 0), __int_as_float(sflag[k]));
        d[kHN] = make_float2(sw[k][0], sw[k][1]);
        d[2 * kHN] = make_float2(sw[k][2], sw[k][3]);
      }
    }
    Grp G;
    G.wstart = wstart; G.wcount = wcount;
    G.fits = wcount <= kHMaxW;   // else: corners from global memory
    G.xg = a.x + ((long)n * g.C + (long)grp * cpg) * plane;   // channel 0 of the group
    if (G.fits)   // slab 0, by everybody
      for (int it = tid; it < wcount; it += kHThreads) {
        u32x4 va, vb;
        win_load(G, it, 0, va, vb);
        xwin_store(xs, it >> 3, it & 7, va, vb);
      }
    __syncthreads();
    return G;
  };

  if (mma) {
    // ================= matrix-core waves: acc += A(slab, tap) . B(slab, tap) ===========================
    floatx16 acc[kHFr][kHPB];
#pragma unroll
    for (int i = 0; i < kHFr; ++i)
#pragma unroll
      for (int q = 0; q < kHPB; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][q][e] = 0.f;
    u32x4 anxt[kHFr];
#pragma unroll
    for (int i = 0; i < kHFr; ++i) anxt[i] = u32x4{0u, 0u, 0u, 0u};
    for (int grp = 0; grp < g.dgroup; ++grp) {
      group_begin(grp);
      const u32x4* const abase = a.wre + ((long)(mt * a.nslab + grp * ns) * 9) * 512 + frag0 * 64 + lane;   // + step * 512
      auto load_a = [&](int step) {   // (past the group's end: the last step again, in vain)
        const u32x4* q = abase + (long)iminr(step, ns * 9 - 1) * 512;
#pragma unroll
        for (int i = 0; i < kHFr; ++i)
          if (i < nf) anxt[i] = q[i * 64];
      };
      load_a(0);
      f16_lds_barrier();   // (the samplers' B of slab 0)
      for (int s = 0; s < ns; ++s) {
        const char* brd = Bs + (s & 1) * kHBBuf + (lane >> 5) * kHBHalf + (lane & 31) * 16;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
          u32x4 acur[kHFr], b[kHPB];
#pragma unroll
          for (int i = 0; i < kHFr; ++i) acur[i] = anxt[i];
          load_a(s * 9 + tap + 1);
#pragma unroll
          for (int q = 0; q < kHPB; ++q) b[q] = *reinterpret_cast<const u32x4*>(brd + tap * kHBStep + q * 512);
#pragma unroll
          for (int i = 0; i < kHFr; ++i)
            if (i < nf)
#pragma unroll
              for (int q = 0; q < kHPB; ++q)
                acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, acur[i]),
                                                                   __builtin_bit_cast(halfx8, b[q]), acc[i][q], 0, 0, 0);
        }
        if (s + 1 < ns) f16_lds_barrier();
      }
    }
    // ---- y[n, f, p] = RNE(acc + bias[f]); D layout of a 32x32 tile: element e of lane l -> row
    // (e / 4) * 8 + (l / 32) * 4 + e % 4, column l % 32 ----
    __half* yn = a.y + (long)n * a.F * P;
#pragma unroll
    for (int i = 0; i < kHFr; ++i)
      if (i < nf)
#pragma unroll
        for (int q = 0; q < kHPB; ++q) {
          const int pp = p0 + q * 32 + (lane & 31);
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int f = mt * 256 + (frag0 + i) * 32 + (e >> 2) * 8 + (lane >> 5) * 4 + (e & 3);
            if (f < a.F && pp < p1) {
              const float v = acc[i][q][e];
              yn[(long)f * P + pp] = __float2half(a.bias ? v + __half2float(a.bias[f]) : v);
            }
          }
        }
  } else {
    // ================= sampling waves: window of slab s + 2, B of slab s + 1 ============================
    for (int grp = 0; grp < g.dgroup; ++grp) {
      const Grp G = group_begin(grp);
      const int wcount = G.wcount;
      const bool fits = G.fits;
      u32x4 stg[kHStage][2];
      auto win_issue = [&](int slab) {
#pragma unroll
        for (int k = 0; k < kHStage; ++k) {
          const int it = sid + k * kHLanes;
          if (it < wcount) win_load(G, it, slab, stg[k][0], stg[k][1]);
        }
      };
      auto win_store = [&](char* xb) {
#pragma unroll
        for (int k = 0; k < kHStage; ++k) {
          const int it = sid + k * kHLanes;
          if (it < wcount) xwin_store(xb, it >> 3, it & 7, stg[k][0], stg[k][1]);
        }
      };
      auto sample_slab = [&](int slab, const char* xb, char* bbuf) {
#pragma unroll
        for (int i = 0; i < kHTapIters; ++i) {
          const int tap = kHTapStride * i + tap0;
          if (tap < 9) {
            const float2* sp = sst + tap * 3 * kHN + pl;
            const float2 q0 = sp[0], q1 = sp[kHN], q2 = sp[2 * kHN];
            const int base = __float_as_int(q0.x), flag = __float_as_int(q0.y);
            const int c1 = base, c2 = base + (flag & 1), c3 = base + ((flag & 2) ? g.W : 0), c4 = c3 + (flag & 1);
            u32x4 va, vb, vc, vd;
            if (fits) {
              const char* xh = xb + half * 16;
              va = *reinterpret_cast<const u32x4*>(xh + (c1 + (c1 >> 3)) * 32);
              vb = *reinterpret_cast<const u32x4*>(xh + (c2 + (c2 >> 3)) * 32);
              vc = *reinterpret_cast<const u32x4*>(xh + (c3 + (c3 >> 3)) * 32);
              vd = *reinterpret_cast<const u32x4*>(xh + (c4 + (c4 >> 3)) * 32);
            } else {
              // every address inside the plane; an outside sample reads nothing
              const unsigned short* xc =
                  reinterpret_cast<const unsigned short*>(G.xg + (long)(slab * 16 + half * 8) * plane + G.wstart);
              va = vb = vc = vd = u32x4{0u, 0u, 0u, 0u};
              if (flag) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                  const unsigned short* e0 = xc + (long)(2 * k) * plane;
                  const unsigned short* e1 = e0 + plane;
                  va[k] = (unsigned)e0[c1] | ((unsigned)e1[c1] << 16);
                  vb[k] = (unsigned)e0[c2] | ((unsigned)e1[c2] << 16);
                  vc[k] = (unsigned)e0[c3] | ((unsigned)e1[c3] << 16);
                  vd[k] = (unsigned)e0[c4] | ((unsigned)e1[c4] << 16);
                }
              }
            }
            u32x4 o;
            o[0] = bilerp2_f16(va[0], vb[0], vc[0], vd[0], q1.x, q1.y, q2.x, q2.y, flag != 0);
            o[1] = bilerp2_f16(va[1], vb[1], vc[1], vd[1], q1.x, q1.y, q2.x, q2.y, flag != 0);
            o[2] = bilerp2_f16(va[2], vb[2], vc[2], vd[2], q1.x, q1.y, q2.x, q2.y, flag != 0);
            o[3] = bilerp2_f16(va[3], vb[3], vc[3], vd[3], q1.x, q1.y, q2.x, q2.y, flag != 0);
            *reinterpret_cast<u32x4*>(bbuf + tap * kHBStep + half * kHBHalf + pl * 16) = o;
          }
        }
      };
      if (fits && ns > 1) win_issue(1);
      sample_slab(0, xs, Bs);
      if (fits && ns > 1) win_store(xs + kHXSlots * 32);
      f16_lds_barrier();
      for (int s = 0; s + 1 < ns; ++s) {
        const bool more = fits && s + 2 < ns;
        if (more) win_issue(s + 2);
        sample_slab(s + 1, xs + ((s + 1) & 1) * (kHXSlots * 32), Bs + ((s + 1) & 1) * kHBBuf);
        if (more) win_store(xs + (s & 1) * (kHXSlots * 32));
        f16_lds_barrier();
      }
    }
  }
}

// element-wise widening of a half buffer aligned to 2 bytes only (sd_cast_f16_to_f32 wants 16)
__global__ __launch_bounds__(256) void dcn_f16_widen_kernel(const __half* __restrict__ src, float* __restrict__ dst,
                                                            size_t n) {
  size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  for (; i < n; i += (size_t)gridDim.x * 256) dst[i] = __half2float(src[i]);
}

static int widen(const void* src, float* dst, size_t n, void* stream) {
  if (n == 0 || !src) return SD_OK;
  if (((uintptr_t)src & 15) == 0) return sd_cast_f16_to_f32(src, dst, n, stream);
  dcn_f16_widen_kernel<<<kNumCU * 8, 256, 0, (hipStream_t)stream>>>((const __half*)src, dst, n);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

// the buffers of the widened calls, carved in one order by the size query and the call
struct F16FwdWs { float *x, *off, *w, *b, *y; void* inner; size_t inner_bytes; };
static size_t fwd_ws_layout(void* ws, F16FwdWs& L, int N, int C, int H, int W, int F, int kh, int kw, int pad,
                            int stride, int dil, int dgroup, int num_group, long Ho, long Wo) {
  WsCarver cv(ws);
  const size_t P = (size_t)Ho * Wo;
  L.x = cv.take<float>(sizeof(float) * N * C * H * W);
  L.off = cv.take<float>(sizeof(float) * N * dgroup * 2 * kh * kw * P);
  L.w = cv.take<float>(sizeof(float) * F * (C / num_group) * kh * kw);
  L.b = cv.take<float>(sizeof(float) * F);
  L.y = cv.take<float>(sizeof(float) * N * F * P);
  L.inner_bytes = sd_deform_convolution_fwd_workspace_bytes(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup,
                                                            num_group, 0);
  L.inner = cv.take<char>(L.inner_bytes);
  return cv.need();
}

struct F16BwdWs { float *og, *x, *off, *w, *dx, *doff, *dw, *db; void* inner; size_t inner_bytes; };
static size_t bwd_ws_layout(void* ws, F16BwdWs& L, int N, int C, int H, int W, int F, int kh, int kw, int pad,
                            int stride, int dil, int dgroup, int num_group, long Ho, long Wo) {
  WsCarver cv(ws);
  const size_t P = (size_t)Ho * Wo, nx = (size_t)N * C * H * W, noff = (size_t)N * dgroup * 2 * kh * kw * P,
               nw = (size_t)F * (C / num_group) * kh * kw;
  L.og = cv.take<float>(sizeof(float) * N * F * P);
  L.x = cv.take<float>(sizeof(float) * nx);
  L.off = cv.take<float>(sizeof(float) * noff);
  L.w = cv.take<float>(sizeof(float) * nw);
  L.dx = cv.take<float>(sizeof(float) * nx);
  L.doff = cv.take<float>(sizeof(float) * noff);
  L.dw = cv.take<float>(sizeof(float) * nw);
  L.db = cv.take<float>(sizeof(float) * F);
  L.inner_bytes = sd_deform_conv_workspace_bytes(N, C, H, W, kh, kw, pad, stride, dil);
  L.inner = cv.take<char>(L.inner_bytes);
  return cv.need();
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_deform_convolution_fwd_workspace_bytes_f16(int N, int C, int H, int W, int F, int kh, int kw,
                                                                int pad, int stride, int dil, int dgroup,
                                                                int num_group) {
  long Ho, Wo;
  if (N <= 0 || C <= 0 || F <= 0 || kh <= 0 || kw <= 0 || dgroup <= 0 || num_group <= 0 || C % num_group ||
      !out_hw(H, W, kh, kw, pad, stride, dil, Ho, Wo))
    return 256;   // (the call itself fails or has nothing to do)
  if (dcn_f16_fused_ok(C, H, W, kh, kw, dgroup, num_group))
    return (size_t)((F + 255) / 256) * (C / 16) * 9 * 512 * sizeof(u32x4) + 256;
  F16FwdWs L;
  return fwd_ws_layout(nullptr, L, N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group, Ho, Wo) + 256;
}

extern "C" int sd_deform_convolution_fwd_f16(const void* x, const void* offset, const void* weight, const void* bias,
                                             void* y, int N, int C, int H, int W, int F, int kh, int kw, int pad,
                                             int stride, int dil, int dgroup, int num_group, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  DcnGeom g;
  if (int e = make_geom(g, N, C, H, W, kh, kw, pad, pad, stride, stride, dil, dil, dgroup)) return e;
  SD_REQUIRE(F > 0, "num_filter must be positive");
  SD_REQUIRE(num_group >= 1 && C % num_group == 0 && F % num_group == 0, "num_group must divide the input channels and num_filter");
  if (N == 0) return SD_OK;
  SD_REQUIRE(x && offset && weight && y, "null tensor pointer");
  SD_REQUIRE((((uintptr_t)x | (uintptr_t)offset | (uintptr_t)weight | (uintptr_t)bias | (uintptr_t)y) & 1) == 0,
             "half tensors must be aligned to 2 bytes");
  const size_t need = sd_deform_convolution_fwd_workspace_bytes_f16(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup,
                                                                    num_group);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "DeformableConvolution (fp16 forward) workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  hipStream_t st = (hipStream_t)stream;
  const long P = (long)g.Ho * g.Wo;
  if (!dcn_f16_fused_ok(C, H, W, kh, kw, dgroup, num_group)) {
    // every other shape: the fp32 operator on widened operands, its result rounded once
    F16FwdWs L;
    fwd_ws_layout(workspace, L, N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group, g.Ho, g.Wo);
    if (int e = widen(x, L.x, (size_t)N * C * H * W, stream)) return e;
    if (int e = widen(offset, L.off, (size_t)N * dgroup * 2 * kh * kw * P, stream)) return e;
    if (int e = widen(weight, L.w, (size_t)F * (C / num_group) * kh * kw, stream)) return e;
    if (int e = widen(bias, L.b, (size_t)F, stream)) return e;
    if (int e = sd_deform_convolution_fwd(L.x, L.off, L.w, bias ? L.b : nullptr, L.y, N, C, H, W, F, kh, kw, pad,
                                          stride, dil, dgroup, num_group, 0, L.inner, L.inner_bytes, stream))
      return e;
    return sd_cast_f32_to_f16(L.y, y, (size_t)N * F * P, SD_REQ_WRITE, stream);
  }
  const int mtiles = (F + 255) / 256, nslab = C / 16;
  u32x4* wre = reinterpret_cast<u32x4*>(round256((size_t)(uintptr_t)workspace));
  {
    const long total = (long)mtiles * nslab * 9 * 512;
    hipLaunchKernelGGL(dcn_f16_prep_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       (const unsigned short*)weight, wre, F, C, total);
    SD_LAUNCH_CHECK();
  }
  DcnF16Args a{};
  a.x = (const __half*)x; a.offset = (const __half*)offset; a.wre = wre; a.bias = (const __half*)bias;
  a.y = (__half*)y; a.g = g; a.F = F; a.mtiles = mtiles; a.nslab = nslab;
  // tiles per image: enough for <= kHN pixels each, then as many more as keeps the launch at the same whole
  // number of rounds of the CUs (one workgroup per CU)
  int T = cdiv(P, kHN);
  const long rounds = ((long)N * T * mtiles + kNumCU - 1) / kNumCU;
  const long fit = rounds * kNumCU / ((long)N * mtiles);
  if (fit > T) T = (int)(fit < P ? fit : P);
  a.tile_w = cdiv(P, T);
  a.tiles_per_image = cdiv(P, a.tile_w);
  a.by_xcd = N >= 8;
  const long nblocks = (long)a.tiles_per_image * (a.by_xcd ? 8 * cdiv(N, 8) : N) * mtiles;
  SD_REQUIRE(nblocks < (1L << 31), "too many tiles");
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)dcn_fwd_fused_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kHSmem));
  const dim3 grid((unsigned)nblocks);
  hipLaunchKernelGGL(dcn_fwd_fused_f16_kernel, grid, dim3(kHThreads), kHSmem, st, a);
  SD_LAUNCH_CHECK();
  return SD_OK;
}

extern "C" size_t sd_deform_convolution_bwd_workspace_bytes_f16(int N, int C, int H, int W, int F, int kh, int kw,
                                                                int pad, int stride, int dil, int dgroup,
                                                                int num_group) {
  long Ho, Wo;
  if (N <= 0 || C <= 0 || F <= 0 || kh <= 0 || kw <= 0 || dgroup <= 0 || num_group <= 0 || C % num_group ||
      !out_hw(H, W, kh, kw, pad, stride, dil, Ho, Wo))
    return 256;
  F16BwdWs L;
  return bwd_ws_layout(nullptr, L, N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group, Ho, Wo) + 256;
}

extern "C" int sd_deform_convolution_bwd_f16(const void* out_grad, const void* x, const void* offset,
                                             const void* weight, void* d_x, void* d_offset, void* d_weight,
                                             void* d_bias, int req_x, int req_offset, int req_weight, int req_bias,
                                             int N, int C, int H, int W, int F, int kh, int kw, int pad, int stride,
                                             int dil, int dgroup, int num_group, void* workspace,
                                             size_t workspace_bytes, void* stream) {
  DcnGeom g;
  if (int e = make_geom(g, N, C, H, W, kh, kw, pad, pad, stride, stride, dil, dil, dgroup)) return e;
  SD_REQUIRE(F > 0, "num_filter must be positive");
  SD_REQUIRE(num_group >= 1 && C % num_group == 0 && F % num_group == 0, "num_group must divide the input channels and num_filter");
  const int reqs[4] = {req_x, req_offset, req_weight, req_bias};
  void* const dst[4] = {d_x, d_offset, d_weight, d_bias};
  for (int i = 0; i < 4; ++i) {
    SD_REQUIRE(reqs[i] == SD_REQ_NULL || reqs[i] == SD_REQ_WRITE || reqs[i] == SD_REQ_ADD, "bad req %d", reqs[i]);
    SD_REQUIRE(reqs[i] == SD_REQ_NULL || dst[i], "a requested gradient is null");
  }
  if (N == 0) return SD_OK;
  SD_REQUIRE(out_grad && x && offset && weight, "null tensor pointer");
  SD_REQUIRE((((uintptr_t)out_grad | (uintptr_t)x | (uintptr_t)offset | (uintptr_t)weight | (uintptr_t)d_x |
               (uintptr_t)d_offset | (uintptr_t)d_weight | (uintptr_t)d_bias) & 1) == 0,
             "half tensors must be aligned to 2 bytes");
  const size_t need = sd_deform_convolution_bwd_workspace_bytes_f16(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup,
                                                                    num_group);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "DeformableConvolution (fp16 backward) workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  F16BwdWs L;
  bwd_ws_layout(workspace, L, N, C, H, W, F, kh, kw, pad, stride, dil, dgroup, num_group, g.Ho, g.Wo);
  const size_t P = (size_t)g.Ho * g.Wo, nx = (size_t)N * C * H * W, noff = (size_t)N * dgroup * 2 * kh * kw * P,
               nw = (size_t)F * (C / num_group) * kh * kw;
  if (int e = widen(out_grad, L.og, (size_t)N * F * P, stream)) return e;
  if (int e = widen(x, L.x, nx, stream)) return e;
  if (int e = widen(offset, L.off, noff, stream)) return e;
  if (int e = widen(weight, L.w, nw, stream)) return e;
  // the fp32 backward writes fp32 gradients; each is rounded once (req = add: onto the widened destination)
  const int wr = SD_REQ_WRITE;
  if (int e = sd_deform_convolution_bwd(L.og, L.x, L.off, L.w, nullptr, L.dx, L.doff, L.dw, L.db, req_x ? wr : 0,
                                        req_offset ? wr : 0, req_weight ? wr : 0, req_bias ? wr : 0, N, C, H, W, F,
                                        kh, kw, pad, stride, dil, dgroup, num_group, L.inner, L.inner_bytes, stream))
    return e;
  const float* src[4] = {L.dx, L.doff, L.dw, L.db};
  const size_t cnt[4] = {nx, noff, nw, (size_t)F};
  for (int i = 0; i < 4; ++i)
    if (int e = sd_cast_f32_to_f16(src[i], dst[i], cnt[i], reqs[i], stream)) return e;
  return SD_OK;
}
