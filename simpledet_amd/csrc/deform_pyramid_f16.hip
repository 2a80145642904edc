// DeformableConvolution in fp16 for gfx950: a list of independent problems in ONE launch, each with up to two
// sources summed in the accumulator and an optional (upsampled) residual in the epilogue.  The SEPC
// neck's pyramid convolutions are dozens of tiny calls of the col-free forward (deform_fused_f16.hip);
// here they share one grid, one weight re-order per distinct weight and one rounding per output.
#include "deform_f16_common.h"
#pragma clang fp contract(off)

namespace sd {

// ------------------------------------------------------------------------------------------------
// The pipeline is 4.27's, tile for tile: 4 matrix-core + 4 sampling waves on tiles of <= kYN pixels, the x window
// of a 16-channel slab in LDS as halves with the channels of a position side by side, B a slab at a time with one
// barrier per slab, the no-LDS branch for windows that do not fit.  The K order, the fragment order of the weights
// and the sampling arithmetic are its own, so a single-source problem without a residual gives its bits.
// What is new:
//   table     the problems travel in the kernel arguments, by value (PyrArgs, 3 KB): no copy to the device, no
//             memset, kernel nodes only under graph capture.
//   blocks    block -> (problem, filter tile, image, pixel tile) through the prefix `start` of the table, a scalar
//             search over <= 16 entries.  The host sorts the table by slabs per tile, heaviest first, so the
//             dual-source tiles start before the single-source ones; blocks are linear, so consecutive tiles land
//             on consecutive XCDs.  One tile width for the whole launch (pyr_tile_width).
//   loop      for source: for group: around the slab pipeline; the fp32 accumulators and the A prefetch registers
//             live across both loops.  group_begin works on the source's own geometry, offsets and planes.
//   epilogue  acc + bias_0 + bias_1 + residual[h >> shift, w >> shift] in fp32, in that order, one RNE to fp16.
// Both roles pass the same barriers: every trip count (sources, groups, slabs) and `fits` come from the table or
// from LDS words the whole workgroup reads, never from a lane's own data.
// ------------------------------------------------------------------------------------------------
constexpr int kYN = 64, kYMma = 4, kYThreads = 512;   // (4.27's shipped variant; the weights' fragment order is tied to it)
constexpr int kYLanes = kYThreads - 64 * kYMma;      // sampling lanes
constexpr int kYPB = kYN / 32;                       // 32-pixel blocks of a tile
constexpr int kYFr = 8 / kYMma;                      // 32-filter fragments per matrix-core wave
constexpr int kYTapStride = kYLanes / (2 * kYN);     // a sampling lane takes every kYTapStride-th tap
constexpr int kYTapIters = (9 + kYTapStride - 1) / kYTapStride;
constexpr int kYBHalf = kYN * 16 + 64;               // bytes of one k8 of a step (+ a bank shift)
constexpr int kYBStep = 2 * kYBHalf, kYBBuf = 9 * kYBStep;
constexpr int kYStateBytes = 9 * 3 * kYN * 8;        // sampling state [tap][word][pixel], 8-byte words
constexpr int kYXSlots = (160 * 1024 - 2 * kYBBuf - kYStateBytes - 64) / 64;   // 32-byte slots of one window buffer
constexpr int kYMaxW = (kYXSlots * 8 / 9) & ~7;      // positions of the largest window
constexpr int kYStage = (kYMaxW + kYLanes - 1) / kYLanes;
constexpr int kYSmem = 2 * kYXSlots * 32 + 2 * kYBBuf + kYStateBytes + 64;
constexpr int kYMaxProblems = 16, kYMaxSources = 2, kYMaxWeights = kYMaxProblems * kYMaxSources;

struct PyrSrc {            // 64 bytes
  const __half* x;
  const __half* offset;
  const u32x4* wre;        // weights in fragment order (dcn_pyramid_prep_weight_kernel)
  const __half* bias;      // (F) or null
  int C, H, W, dgroup, pad, stride, dil, nslab;
};
struct PyrProb {           // 192 bytes
  __half* y;
  const __half* res;       // (N, F, Hr, Wr) or null
  int N, F, Ho, Wo, Hr, Wr, shift, nsrc, mtiles, tiles, start, spare;   // start: first block of the problem
  PyrSrc s[kYMaxSources];
};
struct PyrArgs {
  int count, tile_w, spare0, spare1;
  PyrProb p[kYMaxProblems];
};
static_assert(sizeof(PyrArgs) <= 4096, "the table must fit the kernel-argument segment");

struct PyrWSeg { const unsigned short* w; u32x4* wre; int F, C; long start, end; };   // [start, end) of the launch's items
struct PyrWArgs { int count, spare; PyrWSeg s[kYMaxWeights]; };

// every distinct weight of the launch (F, C, 9) -> its wre[mt][slab][tap][fragment 0..7][lane], 4.27's order: lane l
// of fragment r holds filter row mt*256 + r*32 + (l & 31) and channels slab*16 + (l >> 5)*8 .. +7 of the tap; rows
// past F are 0.  A segment is a whole number of 512-item units, so a block of 256 lies in one segment.
__global__ __launch_bounds__(256) void dcn_pyramid_prep_weight_kernel(PyrWArgs a) {
  const long b0 = (long)blockIdx.x * 256;
  int k = 0;
#pragma unroll 1
  for (int j = 1; j < a.count; ++j)
    if (b0 >= a.s[j].start) k = j;
  const PyrWSeg& sg = a.s[k];
  const long e = b0 + threadIdx.x - sg.start;
  if (e >= sg.end - sg.start) return;
  const int F = sg.F, C = sg.C;
  const int lane = (int)(e & 63), frag = (int)((e >> 6) & 7);
  long r = e >> 9;
  const int tap = (int)(r % 9); r /= 9;
  const int nslab = C / 16;
  const int slab = (int)(r % nslab), mt = (int)(r / nslab);
  const int f = mt * 256 + frag * 32 + (lane & 31), c0 = slab * 16 + (lane >> 5) * 8;
  u32x4 o = {0u, 0u, 0u, 0u};
  if (f < F) {
    const unsigned short* s = sg.w + ((long)f * C + c0) * 9 + tap;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = (unsigned)s[(2 * q) * 9] | ((unsigned)s[(2 * q + 1) * 9] << 16);
  }
  sg.wre[e] = o;
}

// a source of the block's problem, as the loops see it
struct PyrSrcV {
  DcnGeom g;
  const __half* x;         // image n, channel 0
  const __half* offset;    // image n
  const u32x4* wre;
  int cpg, ns, plane, nslab;
};
struct PyrGrp { int wstart, wcount; bool fits; const __half* xg; };

__global__ __launch_bounds__(kYThreads) void dcn_pyramid_fwd_f16_kernel(PyrArgs a) {
  extern __shared__ __attribute__((aligned(16))) char ysm[];
  char* const xs = ysm;                                  // two window buffers
  char* const Bs = ysm + 2 * kYXSlots * 32;              // two slab buffers of B
  float2* const sst = reinterpret_cast<float2*>(Bs + 2 * kYBBuf);
  int* const rng = reinterpret_cast<int*>(Bs + 2 * kYBBuf + kYStateBytes);
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // block -> problem: the last table entry that starts at or before this block
  int pi = 0;
#pragma unroll 1
  for (int k = 1; k < a.count; ++k)
    if ((int)blockIdx.x >= a.p[k].start) pi = k;
  const PyrProb& pb = a.p[pi];
  // -> (filter tile, image, pixel tile); linear, so the tiles are dealt over all XCDs
  const int P = pb.Ho * pb.Wo, F = pb.F, nsrc = pb.nsrc;
  const int local = (int)blockIdx.x - pb.start, per_mt = pb.N * pb.tiles;
  const int mt = local / per_mt, bb = local % per_mt;
  const int n = bb / pb.tiles, t = bb % pb.tiles;
  if (mt >= pb.mtiles) return;
  const int p0 = t * a.tile_w, p1 = iminr(p0 + a.tile_w, P);
  if (p0 >= P) return;
  const bool mma = wave < kYMma;
  // a sampling lane's (pixel, k8) and first tap
  const int sid = mma ? 0 : tid - 64 * kYMma;
  const int pl = (sid % (2 * kYN)) >> 1, half = sid & 1, tap0 = sid / (2 * kYN);
  // a matrix-core wave's fragments: rows mt*256 + (wave*kYFr + i)*32 .. +31, those below F only
  const int frag0 = (mma ? wave : 0) * kYFr;
  const int nf = imaxr(0, iminr(kYFr, (F - mt * 256 - frag0 * 32 + 31) / 32));

  auto source = [&](int si) -> PyrSrcV {
    const PyrSrc& s = pb.s[si];
    PyrSrcV v;
    v.g = DcnGeom{pb.N, s.C, s.H, s.W, 3, 3, s.pad, s.pad, s.stride, s.stride, s.dil, s.dil, s.dgroup, pb.Ho, pb.Wo};
    v.plane = s.H * s.W;
    v.cpg = s.C / s.dgroup;
    v.ns = v.cpg / 16;
    v.nslab = s.nslab;
    v.x = s.x + (long)n * s.C * v.plane;
    v.offset = s.offset + (long)n * s.dgroup * 18 * P;
    v.wre = s.wre;
    return v;
  };
  auto win_load = [&](const PyrSrcV& S, const PyrGrp& G, int it, int slab, u32x4& va, u32x4& vb) {
    const int pg = it >> 3, cp = it & 7;   // item -> (position group, channel pair)
    const __half* src = G.xg + (long)(slab * 16 + 2 * cp) * S.plane + G.wstart + 8 * pg;
    const int nv = S.plane - (G.wstart + 8 * pg);
    va = ldg8_f16(src, nv);
    vb = ldg8_f16(src + S.plane, nv);
  };
  // ---- per (source, group), every wave (same barriers in every role): the sampling state of the 9 taps into LDS,
  // the window the samples touch, slab 0 of it ----
  auto group_begin = [&](const PyrSrcV& S, int grp) -> PyrGrp {
    const DcnGeom& g = S.g;
    int sbase[2], sflag[2];
    float sw[2][4];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int item = tid + k * kYThreads;
      const int tap = item / kYN, p = p0 + item % kYN;
      sbase[k] = 0; sflag[k] = 0;
      sw[k][0] = sw[k][1] = sw[k][2] = sw[k][3] = 0.f;
      if (item < 9 * kYN && p < p1) {
        const int h_col = p / g.Wo, w_col = p % g.Wo;
        const __half* off = S.offset + ((long)grp * 18 + 2 * tap) * P + p;
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
    __syncthreads();   // (the previous group or source is done with the state, the windows and B)
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
    if (lane == 0 && hi >= 0) {   // (LDS words)
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
      const int item = tid + k * kYThreads;
      if (item < 9 * kYN) {
        float2* d = sst + (item / kYN) * 3 * kYN + item % kYN;
        d[0] = make_float2(__int_as_float(sflag[k] ? sbase[k] - wstart : 0), __int_as_float(sflag[k]));
        d[kYN] = make_float2(sw[k][0], sw[k][1]);
        d[2 * kYN] = make_float2(sw[k][2], sw[k][3]);
      }
    }
    PyrGrp G;
    G.wstart = wstart; G.wcount = wcount;
    G.fits = wcount <= kYMaxW;   // else: corners from global memory
    G.xg = S.x + (long)grp * S.cpg * S.plane;   // channel 0 of the group
    if (G.fits)   // slab 0, by everybody
      for (int it = tid; it < wcount; it += kYThreads) {
        u32x4 va, vb;
        win_load(S, G, it, 0, va, vb);
        xwin_store(xs, it >> 3, it & 7, va, vb);
      }
    __syncthreads();
    return G;
  };

  if (mma) {
    // ================= matrix-core waves: acc += A(source, slab, tap) . B(slab, tap) ====================
    floatx16 acc[kYFr][kYPB];
#pragma unroll
    for (int i = 0; i < kYFr; ++i)
#pragma unroll
      for (int q = 0; q < kYPB; ++q)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][q][e] = 0.f;
    u32x4 anxt[kYFr];
#pragma unroll
    for (int i = 0; i < kYFr; ++i) anxt[i] = u32x4{0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int si = 0; si < nsrc; ++si) {
      const PyrSrcV S = source(si);
      const int ns = S.ns;
#pragma unroll 1
      for (int grp = 0; grp < S.g.dgroup; ++grp) {
        group_begin(S, grp);
        const u32x4* const abase = S.wre + ((long)(mt * S.nslab + grp * ns) * 9) * 512 + frag0 * 64 + lane;   // + step * 512
        auto load_a = [&](int step) {   // (past the group's end: the last step again, in vain)
          const u32x4* q = abase + (long)iminr(step, ns * 9 - 1) * 512;
#pragma unroll
          for (int i = 0; i < kYFr; ++i)
            if (i < nf) anxt[i] = q[i * 64];
        };
        load_a(0);
        f16_lds_barrier();   // (the samplers' B of slab 0)
        for (int s = 0; s < ns; ++s) {
          const char* brd = Bs + (s & 1) * kYBBuf + (lane >> 5) * kYBHalf + (lane & 31) * 16;
#pragma unroll
          for (int tap = 0; tap < 9; ++tap) {
            u32x4 acur[kYFr], b[kYPB];
#pragma unroll
            for (int i = 0; i < kYFr; ++i) acur[i] = anxt[i];
            load_a(s * 9 + tap + 1);
#pragma unroll
            for (int q = 0; q < kYPB; ++q) b[q] = *reinterpret_cast<const u32x4*>(brd + tap * kYBStep + q * 512);
#pragma unroll
            for (int i = 0; i < kYFr; ++i)
              if (i < nf)
#pragma unroll
                for (int q = 0; q < kYPB; ++q)
                  acc[i][q] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, acur[i]),
                                                                     __builtin_bit_cast(halfx8, b[q]), acc[i][q], 0, 0, 0);
          }
          if (s + 1 < ns) f16_lds_barrier();
        }
      }
    }
    // ---- y[n, f, p] = RNE(acc + bias_0[f] + bias_1[f] + res[n, f, h >> shift, w >> shift]); D layout of a 32x32
    // tile: element e of lane l -> row (e / 4) * 8 + (l / 32) * 4 + e % 4, column l % 32 ----
    __half* yn = pb.y + (long)n * F * P;
    const __half* const b0 = pb.s[0].bias;
    const __half* const b1 = nsrc > 1 ? pb.s[1].bias : nullptr;
    const int rplane = pb.Hr * pb.Wr;
    const __half* const rn = pb.res ? pb.res + (long)n * F * rplane : nullptr;
#pragma unroll
    for (int i = 0; i < kYFr; ++i)
      if (i < nf)
#pragma unroll
        for (int q = 0; q < kYPB; ++q) {
          const int pp = p0 + q * 32 + (lane & 31);
          const int roff = pp < p1 ? ((pp / pb.Wo) >> pb.shift) * pb.Wr + ((pp % pb.Wo) >> pb.shift) : 0;
#pragma unroll
          for (int e = 0; e < 16; ++e) {
            const int f = mt * 256 + (frag0 + i) * 32 + (e >> 2) * 8 + (lane >> 5) * 4 + (e & 3);
            if (f < F && pp < p1) {
              float v = acc[i][q][e];
              if (b0) v = v + __half2float(b0[f]);
              if (b1) v = v + __half2float(b1[f]);
              if (rn) v = v + __half2float(rn[(long)f * rplane + roff]);
              yn[(long)f * P + pp] = __float2half(v);
            }
          }
        }
  } else {
    // ================= sampling waves: window of slab s + 2, B of slab s + 1 ============================
#pragma unroll 1
    for (int si = 0; si < nsrc; ++si) {
      const PyrSrcV S = source(si);
      const int ns = S.ns, gW = S.g.W;
#pragma unroll 1
      for (int grp = 0; grp < S.g.dgroup; ++grp) {
        const PyrGrp G = group_begin(S, grp);
        const int wcount = G.wcount;
        const bool fits = G.fits;
        u32x4 stg[kYStage][2];
        auto win_issue = [&](int slab) {
#pragma unroll
          for (int k = 0; k < kYStage; ++k) {
            const int it = sid + k * kYLanes;
            if (it < wcount) win_load(S, G, it, slab, stg[k][0], stg[k][1]);
          }
        };
        auto win_store = [&](char* xb) {
#pragma unroll
          for (int k = 0; k < kYStage; ++k) {
            const int it = sid + k * kYLanes;
            if (it < wcount) xwin_store(xb, it >> 3, it & 7, stg[k][0], stg[k][1]);
          }
        };
        auto sample_slab = [&](int slab, const char* xb, char* bbuf) {
#pragma unroll
          for (int i = 0; i < kYTapIters; ++i) {
            const int tap = kYTapStride * i + tap0;
            if (tap < 9) {
              const float2* sp = sst + tap * 3 * kYN + pl;
              const float2 q0 = sp[0], q1 = sp[kYN], q2 = sp[2 * kYN];
              const int base = __float_as_int(q0.x), flag = __float_as_int(q0.y);
              const int c1 = base, c2 = base + (flag & 1), c3 = base + ((flag & 2) ? gW : 0), c4 = c3 + (flag & 1);
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
                    reinterpret_cast<const unsigned short*>(G.xg + (long)(slab * 16 + half * 8) * S.plane + G.wstart);
                va = vb = vc = vd = u32x4{0u, 0u, 0u, 0u};
                if (flag) {
#pragma unroll
                  for (int k = 0; k < 4; ++k) {
                    const unsigned short* e0 = xc + (long)(2 * k) * S.plane;
                    const unsigned short* e1 = e0 + S.plane;
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
              *reinterpret_cast<u32x4*>(bbuf + tap * kYBStep + half * kYBHalf + pl * 16) = o;
            }
          }
        };
        if (fits && ns > 1) win_issue(1);
        sample_slab(0, xs, Bs);
        if (fits && ns > 1) win_store(xs + kYXSlots * 32);
        f16_lds_barrier();
        for (int s = 0; s + 1 < ns; ++s) {
          const bool more = fits && s + 2 < ns;
          if (more) win_issue(s + 2);
          sample_slab(s + 1, xs + ((s + 1) & 1) * (kYXSlots * 32), Bs + ((s + 1) & 1) * kYBBuf);
          if (more) win_store(xs + (s & 1) * (kYXSlots * 32));
          f16_lds_barrier();
        }
      }
    }
  }
}

// ---- host: checks, the two tables, the workspace ----
struct PyrPlan {
  PyrArgs ka;
  PyrWArgs wa;
  long nblocks, witems;
  size_t ws_need;
};

static bool aligned2(const void* p) { return ((uintptr_t)p & 1) == 0; }

// the launch's one tile width: kYN-pixel tiles first, then as narrow as keeps the launch at the same whole number of
// rounds of the CUs (4.27's `fit` rule on the sum over the problems)
static int pyr_tile_width(const PyrArgs& ka) {
  auto blocks = [&](int w) {
    long b = 0;
    for (int i = 0; i < ka.count; ++i)
      b += (long)ka.p[i].mtiles * ka.p[i].N * cdiv((long)ka.p[i].Ho * ka.p[i].Wo, w);
    return b;
  };
  const long cap = (blocks(kYN) + kNumCU - 1) / kNumCU * kNumCU;
  int w = kYN;
  while (w > 1 && blocks(w - 1) <= cap) --w;
  return w;
}

// checks every problem and lays out both kernels' tables; ws null: sizes only.  Nothing is launched here.
static int pyr_plan(const sd_dcn_pyramid_problem* pr, int count, void* ws, PyrPlan& pl) {
  SD_REQUIRE(count >= 0, "negative problem count");
  if (count > kYMaxProblems)
    return fail(SD_ERR_UNSUPPORTED, "DeformableConvolution pyramid: %d problems, at most %d per call", count, kYMaxProblems);
  SD_REQUIRE(count == 0 || pr, "null problem list");
  pl = PyrPlan{};
  WsCarver cv(ws);
  int order[kYMaxProblems];
  long weight[kYMaxProblems];
  for (int i = 0; i < count; ++i) {
    const sd_dcn_pyramid_problem& q = pr[i];
    if (q.num_sources < 1 || q.num_sources > kYMaxSources)
      return fail(SD_ERR_UNSUPPORTED, "DeformableConvolution pyramid: problem %d has %d sources, 1 or 2 are served", i,
                  q.num_sources);
    SD_REQUIRE(q.N > 0 && q.F > 0 && q.Ho > 0 && q.Wo > 0, "problem %d: bad output dimensions", i);
    SD_REQUIRE(q.y && aligned2(q.y), "problem %d: y is null or not aligned to 2 bytes", i);
    SD_REQUIRE((long)q.N * q.F * q.Ho * q.Wo < (1L << 31), "problem %d: output of 2^31 elements or more", i);
    weight[i] = 0;
    for (int s = 0; s < q.num_sources; ++s) {
      const sd_dcn_pyramid_source& u = q.sources[s];
      DcnGeom g;
      if (int e = make_geom(g, q.N, u.C, u.H, u.W, u.kh, u.kw, u.pad, u.pad, u.stride, u.stride, u.dil, u.dil, u.dgroup))
        return e;
      if (!dcn_f16_fused_ok(u.C, u.H, u.W, u.kh, u.kw, u.dgroup, u.num_group))
        return fail(SD_ERR_UNSUPPORTED, "DeformableConvolution pyramid: problem %d source %d is no shape of the "
                    "native-half kernel (3x3, num_group 1, C / dgroup %% 16 == 0)", i, s);
      SD_REQUIRE(g.Ho == q.Ho && g.Wo == q.Wo, "problem %d source %d: output %d x %d, the problem's is %d x %d", i, s,
                 g.Ho, g.Wo, q.Ho, q.Wo);
      SD_REQUIRE(u.x && u.offset && u.weight, "problem %d source %d: null tensor pointer", i, s);
      SD_REQUIRE(aligned2(u.x) && aligned2(u.offset) && aligned2(u.weight) && aligned2(u.bias),
                 "problem %d source %d: half tensors must be aligned to 2 bytes", i, s);
      SD_REQUIRE((long)q.N * u.C * u.H * u.W < (1L << 31), "problem %d source %d: input of 2^31 elements or more", i, s);
      weight[i] += u.C / 16;
    }
    if (q.residual) {
      SD_REQUIRE(aligned2(q.residual), "problem %d: residual not aligned to 2 bytes", i);
      SD_REQUIRE(q.shift == 0 || q.shift == 1, "problem %d: residual shift %d, 0 or 1", i, q.shift);
      SD_REQUIRE(q.Hr > 0 && q.Wr > 0 && ((long)q.Hr << q.shift) >= q.Ho && ((long)q.Wr << q.shift) >= q.Wo,
                 "problem %d: residual %d x %d (shift %d) does not cover the output %d x %d", i, q.Hr, q.Wr, q.shift,
                 q.Ho, q.Wo);
      SD_REQUIRE((long)q.N * q.F * q.Hr * q.Wr < (1L << 31), "problem %d: residual of 2^31 elements or more", i);
    }
    // heaviest first (slabs a tile walks, all sources), equal ones in the caller's order
    int at = i;
    while (at > 0 && weight[order[at - 1]] < weight[i]) {
      order[at] = order[at - 1];
      --at;
    }
    order[at] = i;
  }
  pl.ka.count = count;
  for (int k = 0; k < count; ++k) {
    const sd_dcn_pyramid_problem& q = pr[order[k]];
    PyrProb& d = pl.ka.p[k];
    d.y = (__half*)q.y;
    d.res = (const __half*)q.residual;
    d.N = q.N; d.F = q.F; d.Ho = q.Ho; d.Wo = q.Wo;
    d.Hr = q.residual ? q.Hr : 1; d.Wr = q.residual ? q.Wr : 1; d.shift = q.residual ? q.shift : 0;
    d.nsrc = q.num_sources;
    d.mtiles = (q.F + 255) / 256;
    for (int s = 0; s < q.num_sources; ++s) {
      const sd_dcn_pyramid_source& u = q.sources[s];
      PyrSrc& v = d.s[s];
      v.x = (const __half*)u.x; v.offset = (const __half*)u.offset; v.bias = (const __half*)u.bias;
      v.C = u.C; v.H = u.H; v.W = u.W; v.dgroup = u.dgroup; v.pad = u.pad; v.stride = u.stride; v.dil = u.dil;
      v.nslab = u.C / 16;
      // one re-ordered copy per distinct (weight, F, C)
      int w = 0;
      while (w < pl.wa.count && !(pl.wa.s[w].w == u.weight && pl.wa.s[w].F == q.F && pl.wa.s[w].C == u.C)) ++w;
      if (w == pl.wa.count) {
        PyrWSeg& sg = pl.wa.s[pl.wa.count++];
        const long items = (long)d.mtiles * v.nslab * 9 * 512;
        sg.w = (const unsigned short*)u.weight; sg.F = q.F; sg.C = u.C;
        sg.start = pl.witems; sg.end = pl.witems += items;
        sg.wre = cv.take<u32x4>(items * sizeof(u32x4));
      }
      v.wre = pl.wa.s[w].wre;
    }
  }
  pl.ka.tile_w = count ? pyr_tile_width(pl.ka) : kYN;
  for (int k = 0; k < count; ++k) {
    PyrProb& d = pl.ka.p[k];
    d.tiles = cdiv((long)d.Ho * d.Wo, pl.ka.tile_w);
    d.start = (int)pl.nblocks;
    pl.nblocks += (long)d.mtiles * d.N * d.tiles;
    SD_REQUIRE(pl.nblocks < (1L << 31) && pl.witems < (1L << 38), "too many tiles");
  }
  pl.ws_need = cv.need();
  return SD_OK;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_deform_convolution_pyramid_fwd_workspace_bytes_f16(const sd_dcn_pyramid_problem* problems,
                                                                        int count) {
  PyrPlan pl;
  if (pyr_plan(problems, count, nullptr, pl) != SD_OK) return 256;   // (the call itself fails)
  return pl.ws_need + 256;
}

extern "C" int sd_deform_convolution_pyramid_fwd_f16(const sd_dcn_pyramid_problem* problems, int count,
                                                     void* workspace, size_t workspace_bytes, void* stream) {
  PyrPlan pl;
  if (int e = pyr_plan(problems, count, nullptr, pl)) return e;
  if (count == 0) return SD_OK;
  const size_t need = pl.ws_need + 256;
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "DeformableConvolution pyramid (fp16 forward) workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  if (int e = pyr_plan(problems, count, workspace, pl)) return e;
  hipStream_t st = (hipStream_t)stream;
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)dcn_pyramid_fwd_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kYSmem));
  hipLaunchKernelGGL(dcn_pyramid_prep_weight_kernel, dim3((unsigned)(pl.witems / 256)), dim3(256), 0, st, pl.wa);
  SD_LAUNCH_CHECK();
  hipLaunchKernelGGL(dcn_pyramid_fwd_f16_kernel, dim3((unsigned)pl.nblocks), dim3(kYThreads), kYSmem, st, pl.ka);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
