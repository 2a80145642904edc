// DeformableConvolution in fp16 for gfx950: the weight gradient dW = sum_{n,p} dY . col^T on native-half
// matrix-core operands, the col matrix sampled in the kernel and never stored, and the backward
// entry point that uses it.
#include "deform_f16_common.h"
#pragma clang fp contract(off)

namespace sd {

// ------------------------------------------------------------------------------------------------
// The reduction runs over pixels, so -- the opposite of the forward -- the accumulators stay put and the pixels
// stream by.  A workgroup owns (filter tile of <= 256 filters, 16-channel slab, image, run of pixel steps): a
// 256 x 144 block of dW (144 = 9 taps x 16 channels), as 16 x 9 accumulator blocks of v_mfma_f32_16x16x32_f16, four
// filter row blocks x nine taps (144 registers) on each of its four waves.  Per step of kWN = 64 pixels:
//   A      dY as it lies: a lane's fragment is one filter row x 8 consecutive pixels, loaded from memory (ldg8_f16:
//          2-byte alignment, pixels behind the run's end masked to zero, never read) once the step's samples are
//          written, ahead of the barrier that hands B over (loaded at the head of the step they spill: DESIGN 4.28).
//   state  the (tap, pixel) sampling state of the slab's deformable group, by everybody, into LDS; the contiguous
//          range of plane positions the samples touch is the step's x window.
//   x      the window of the slab's 16 channel planes in LDS, the forward's layout (16 channels of a position side by
//          side, one empty slot after eight): a corner's eight channels are one 16-byte read.  A window that does not
//          fit samples its corners from global memory instead, the same arithmetic (workgroup-uniform branch).
//   B      a lane samples (tap, pixel, 8 channels) -- the forward's B element bit for bit -- and writes it TRANSPOSED,
//          B[tap][channel][pixel], rows of kWN halves + 16 bytes (the row stride that spreads the matrix cores'
//          16-byte reads of 16 rows over all banks): a matrix-core lane reads one (tap, channel) column x 8
//          consecutive pixels as ONE 16-byte read.
//   mma    every wave: 9 taps x 2 k32 steps x its 4 row blocks.
// The phases of a step are separated by workgroup barriers; every wave takes part in every phase.  The kernel is sized
// (four waves of <= 256 registers, < 80 KiB LDS) so that TWO workgroups share a CU and one samples while the other is
// on the matrix cores.
// The 256 x 144 fp32 block goes to the workspace; dcn_wgrad_f16_reduce_kernel sums the blocks of all (image, run)
// in index order and rounds once.  No atomics: the bits depend on the launch geometry only.
// ------------------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kWN = 64, kWThreads = 256, kWCols = 144, kWRows = 256;
constexpr int kWRb = kWRows / 16 / (kWThreads / 64);   // 16-filter row blocks of a wave
constexpr int kWSt = (9 * kWN + kWThreads - 1) / kWThreads;   // (tap, pixel) state items of a thread
constexpr int kWRowB = kWN * 2 + 16;                  // bytes of a B row
constexpr int kWBBytes = kWCols * kWRowB;
constexpr int kWStateBytes = 9 * 3 * kWN * 8;         // sampling state [tap][word][pixel], 8-byte words
constexpr int kWXSlots = (79 * 1024 - kWBBytes - kWStateBytes - 64) / 32;   // 32-byte slots of the window buffer
constexpr int kWMaxW = (kWXSlots * 8 / 9) & ~7;       // positions of the largest window
constexpr int kWSmem = kWXSlots * 32 + kWBBytes + kWStateBytes + 64;
constexpr int kWItems = 9 * kWN * 2;                  // (tap, pixel, k8) sampling items of a step
constexpr int kWIters = (kWItems + kWThreads - 1) / kWThreads;
constexpr long kWBlock = (long)kWRows * kWCols;       // floats of one partial block

struct DcnWgradArgs {
  const __half* x;
  const __half* offset;
  const __half* dy;
  float* part;           // [part][filter tile][slab][256][144]
  DcnGeom g;
  int F, mtiles, nslab, parts, runs, steps;
};

__global__ __launch_bounds__(kWThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void dcn_wgrad_f16_kernel(DcnWgradArgs a) {
  extern __shared__ __attribute__((aligned(16))) char wsm[];
  char* const xs = wsm;
  char* const Bs = wsm + kWXSlots * 32;
  float2* const sst = reinterpret_cast<float2*>(Bs + kWBBytes);
  int* const rng = reinterpret_cast<int*>(Bs + kWBBytes + kWStateBytes);
  const DcnGeom& g = a.g;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int P = g.Ho * g.Wo, plane = g.H * g.W;
  // block -> (filter tile, part = (image, run), slab): the slabs of a part run on XCD part % 8 and share its dY in
  // that XCD's L2
  const int per_mt = (int)gridDim.x / a.mtiles;
  const int mt = (int)blockIdx.x / per_mt, bb = (int)blockIdx.x % per_mt;
  const int j = bb >> 3;
  const int part = (j / a.nslab) * 8 + (bb & 7), slab = j % a.nslab;
  if (part >= a.parts) return;
  const int n = part / a.runs, run = part % a.runs;
  const int q0 = (int)((long)run * a.steps / a.runs) * kWN;
  const int q1 = iminr((int)((long)(run + 1) * a.steps / a.runs) * kWN, P);
  const int cpg = g.C / g.dgroup, ns = cpg / 16;
  const int grp = slab / ns, sl = slab % ns;
  const __half* const xg = a.x + ((long)n * g.C + (long)grp * cpg + sl * 16) * plane;   // channel 0 of the slab
  const __half* const dyn = a.dy + (long)n * a.F * P;
  // the wave's filter row blocks: rows mt*256 + wave*32 + rb*16 .. +15, those below F only
  const int row0 = mt * kWRows + wave * (16 * kWRb);
  const int nrb = imaxr(0, iminr(kWRb, (a.F - row0 + 15) / 16));

  f32x4 acc[kWRb][9];
#pragma unroll
  for (int rb = 0; rb < kWRb; ++rb)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[rb][tap] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int pt = q0; pt < q1; pt += kWN) {
    // ---- the sampling state of the step's (tap, pixel) pairs ----
    int sbase[kWSt], sflag[kWSt];
    float sw[kWSt][4];
#pragma unroll
    for (int k = 0; k < kWSt; ++k) {
      const int item = tid + k * kWThreads;
      const int tap = item / kWN, p = pt + item % kWN;
      sbase[k] = 0; sflag[k] = 0;
      sw[k][0] = sw[k][1] = sw[k][2] = sw[k][3] = 0.f;
      if (item < 9 * kWN && p < q1) {
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
    __syncthreads();   // (the previous step is done with the state, the window and B)
    if (tid == 0) {
      rng[0] = 0x7fffffff;
      rng[1] = -1;
    }
    int lo = 0x7fffffff, hi = -1;
#pragma unroll
    for (int k = 0; k < kWSt; ++k)
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
    const bool fits = wcount <= kWMaxW;   // else: corners from global memory
#pragma unroll
    for (int k = 0; k < kWSt; ++k) {
      const int item = tid + k * kWThreads;
      if (item < 9 * kWN) {
        float2* d = sst + (item / kWN) * 3 * kWN + item % kWN;
        d[0] = make_float2(__int_as_float(sflag[k] ? sbase[k] - wstart : 0), __int_as_float(sflag[k]));
        d[kWN] = make_float2(sw[k][0], sw[k][1]);
        d[2 * kWN] = make_float2(sw[k][2], sw[k][3]);
      }
    }
    if (fits)
      for (int it = tid; it < wcount; it += kWThreads) {   // item -> (position group, channel pair)
        const int pg = it >> 3, cp = it & 7;
        const __half* src = xg + (long)(2 * cp) * plane + wstart + 8 * pg;
        const int nv = plane - (wstart + 8 * pg);
        const u32x4 va = ldg8_f16(src, nv), vb = ldg8_f16(src + plane, nv);
        xwin_store(xs, pg, cp, va, vb);
      }
    __syncthreads();
    // ---- B[tap][channel][pixel]: every (tap, pixel, k8) of the step, sampled as the forward samples it ----
#pragma unroll 1
    for (int i = 0; i < kWIters; ++i) {
      const int item = tid + i * kWThreads;
      if (item < kWItems) {
        const int tap = item / (2 * kWN), pl = (item % (2 * kWN)) >> 1, half = item & 1;
        const float2* sp = sst + tap * 3 * kWN + pl;
        const float2 s0 = sp[0], s1 = sp[kWN], s2 = sp[2 * kWN];
        const int base = __float_as_int(s0.x), flag = __float_as_int(s0.y);
        const int c1 = base, c2 = base + (flag & 1), c3 = base + ((flag & 2) ? g.W : 0), c4 = c3 + (flag & 1);
        u32x4 va, vb, vc, vd;
        if (fits) {
          const char* xh = xs + half * 16;
          va = *reinterpret_cast<const u32x4*>(xh + (c1 + (c1 >> 3)) * 32);
          vb = *reinterpret_cast<const u32x4*>(xh + (c2 + (c2 >> 3)) * 32);
          vc = *reinterpret_cast<const u32x4*>(xh + (c3 + (c3 >> 3)) * 32);
          vd = *reinterpret_cast<const u32x4*>(xh + (c4 + (c4 >> 3)) * 32);
        } else {
          // every address inside the plane; an outside sample reads nothing
          const unsigned short* xc = reinterpret_cast<const unsigned short*>(xg + (long)(half * 8) * plane + wstart);
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
        unsigned short* bw = reinterpret_cast<unsigned short*>(Bs + (tap * 16 + half * 8) * kWRowB) + pl;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const unsigned o = bilerp2_f16(va[k], vb[k], vc[k], vd[k], s1.x, s1.y, s2.x, s2.y, flag != 0);
          bw[(2 * k) * (kWRowB / 2)] = (unsigned short)(o & 0xffffu);
          bw[(2 * k + 1) * (kWRowB / 2)] = (unsigned short)(o >> 16);
        }
      }
    }
    // ---- A: dY[n, row, pt + ks*32 + (lane / 16) * 8 .. + 7], pixels from q1 on are zero ----
    u32x4 afr[kWRb][2];
#pragma unroll
    for (int rb = 0; rb < kWRb; ++rb)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int f = row0 + rb * 16 + (lane & 15), p = pt + ks * 32 + (lane >> 4) * 8;
        afr[rb][ks] = u32x4{0u, 0u, 0u, 0u};
        if (rb < nrb && f < a.F) afr[rb][ks] = ldg8_f16(dyn + (long)f * P + p, q1 - p);
      }
    __syncthreads();
    // ---- acc[row block][tap] += dY(16 rows x 32 pixels) . B(32 pixels x 16 channels of the tap) ----
    const char* brd = Bs + (lane & 15) * kWRowB + (lane >> 4) * 16;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4 b = *reinterpret_cast<const u32x4*>(brd + tap * 16 * kWRowB + ks * 64);
#pragma unroll
        for (int rb = 0; rb < kWRb; ++rb)   // (row blocks past F: A is zero)
          acc[rb][tap] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8, afr[rb][ks]),
                                                                __builtin_bit_cast(halfx8, b), acc[rb][tap], 0, 0, 0);
      }
  }
  // ---- the partial block; D layout of a 16x16 tile: element e of lane l -> row (l / 16) * 4 + e, column l % 16 ----
  float* const pb = a.part + (((long)part * a.mtiles + mt) * a.nslab + slab) * kWBlock;
#pragma unroll
  for (int rb = 0; rb < kWRb; ++rb)
    if (rb < nrb)
#pragma unroll
      for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int fl = wave * (16 * kWRb) + rb * 16 + (lane >> 4) * 4 + e;
          if (mt * kWRows + fl < a.F) pb[(long)fl * kWCols + tap * 16 + (lane & 15)] = acc[rb][tap][e];
        }
}

// dW[f, c, tap] (+)= sum over the parts, in index order, of their partial blocks; one rounding to fp16
__global__ __launch_bounds__(256) void dcn_wgrad_f16_reduce_kernel(const float* __restrict__ part,
                                                                   __half* __restrict__ dw, int C, int mtiles,
                                                                   int nslab, int parts, int req, long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int col = (int)(e % kWCols);
  const long r = e / kWCols;
  const int slab = (int)(r % nslab), f = (int)(r / nslab);
  const float* s = part + ((long)(f >> 8) * nslab + slab) * kWBlock + (long)(f & 255) * kWCols + col;
  const long stride = (long)mtiles * nslab * kWBlock;
  float sum = 0.f;
  for (int k = 0; k < parts; ++k) sum += s[k * stride];
  __half* d = dw + ((long)f * C + slab * 16 + (col & 15)) * 9 + (col >> 4);
  *d = __float2half(req == SD_REQ_ADD ? __half2float(*d) + sum : sum);
}

// pixel runs per image: the caller's, or as many as bring the launch to two workgroups per CU
static int wgrad_runs(int N, int C, int F, long P, int pixel_runs) {
  const int steps = cdiv(P, kWN);
  if (pixel_runs > 0) return pixel_runs < steps ? pixel_runs : steps;
  const long base = (long)N * (C / 16) * ((F + kWRows - 1) / kWRows);
  const long want = (2L * kNumCU + base - 1) / base;
  return (int)(want < steps ? want : steps);
}

static size_t wgrad_part_bytes(int N, int C, int F, long P, int pixel_runs) {
  return sizeof(float) * (size_t)N * wgrad_runs(N, C, F, P, pixel_runs) * ((F + kWRows - 1) / kWRows) * (C / 16) *
         kWBlock;
}

}  // namespace sd

using namespace sd;

extern "C" size_t sd_deform_convolution_bwd_workspace_bytes_f16_fused(int N, int C, int H, int W, int F, int kh,
                                                                      int kw, int pad, int stride, int dil,
                                                                      int dgroup, int num_group, int pixel_runs) {
  const size_t inner = sd_deform_convolution_bwd_workspace_bytes_f16(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup,
                                                                     num_group);
  long Ho, Wo;
  if (N <= 0 || C <= 0 || F <= 0 || pixel_runs < 0 || !dcn_f16_fused_ok(C, H, W, kh, kw, dgroup, num_group) ||
      !out_hw(H, W, kh, kw, pad, stride, dil, Ho, Wo))
    return inner;
  return round256(inner) + wgrad_part_bytes(N, C, F, Ho * Wo, pixel_runs) + 256;
}

extern "C" int sd_deform_convolution_bwd_f16_fused(const void* out_grad, const void* x, const void* offset,
                                                   const void* weight, void* d_x, void* d_offset, void* d_weight,
                                                   void* d_bias, int req_x, int req_offset, int req_weight,
                                                   int req_bias, int N, int C, int H, int W, int F, int kh, int kw,
                                                   int pad, int stride, int dil, int dgroup, int num_group,
                                                   int pixel_runs, void* workspace, size_t workspace_bytes,
                                                   void* stream) {
  SD_REQUIRE(pixel_runs >= 0, "pixel_runs must be >= 0");
  if (!dcn_f16_fused_ok(C, H, W, kh, kw, dgroup, num_group) || req_weight == SD_REQ_NULL || N <= 0)
    return sd_deform_convolution_bwd_f16(out_grad, x, offset, weight, d_x, d_offset, d_weight, d_bias, req_x,
                                         req_offset, req_weight, req_bias, N, C, H, W, F, kh, kw, pad, stride, dil,
                                         dgroup, num_group, workspace, workspace_bytes, stream);
  DcnGeom g;
  if (int e = make_geom(g, N, C, H, W, kh, kw, pad, pad, stride, stride, dil, dil, dgroup)) return e;
  SD_REQUIRE(F > 0, "num_filter must be positive");
  SD_REQUIRE(req_weight == SD_REQ_WRITE || req_weight == SD_REQ_ADD, "bad req %d", req_weight);
  SD_REQUIRE(out_grad && x && offset && weight && d_weight, "null tensor pointer");
  SD_REQUIRE((((uintptr_t)out_grad | (uintptr_t)x | (uintptr_t)offset | (uintptr_t)d_weight) & 1) == 0,
             "half tensors must be aligned to 2 bytes");
  const size_t inner = sd_deform_convolution_bwd_workspace_bytes_f16(N, C, H, W, F, kh, kw, pad, stride, dil, dgroup,
                                                                     num_group);
  const size_t need = sd_deform_convolution_bwd_workspace_bytes_f16_fused(N, C, H, W, F, kh, kw, pad, stride, dil,
                                                                          dgroup, num_group, pixel_runs);
  if (!workspace || workspace_bytes < need)
    return fail(SD_ERR_WORKSPACE, "DeformableConvolution (fp16 backward, fused dW) workspace too small: %zu < %zu bytes",
                workspace_bytes, need);
  // d_x, d_offset, d_bias: the float32 backward on widened operands without its im2col and dW product
  if (req_x != SD_REQ_NULL || req_offset != SD_REQ_NULL || req_bias != SD_REQ_NULL)
    if (int e = sd_deform_convolution_bwd_f16(out_grad, x, offset, weight, d_x, d_offset, nullptr, d_bias, req_x,
                                              req_offset, SD_REQ_NULL, req_bias, N, C, H, W, F, kh, kw, pad, stride,
                                              dil, dgroup, num_group, workspace, inner, stream))
      return e;
  const long P = (long)g.Ho * g.Wo;
  DcnWgradArgs a{};
  a.x = (const __half*)x; a.offset = (const __half*)offset; a.dy = (const __half*)out_grad;
  a.part = reinterpret_cast<float*>(round256((size_t)(uintptr_t)workspace + round256(inner)));
  a.g = g; a.F = F; a.mtiles = (F + kWRows - 1) / kWRows; a.nslab = C / 16;
  a.steps = cdiv(P, kWN);
  a.runs = wgrad_runs(N, C, F, P, pixel_runs);
  a.parts = N * a.runs;
  const long nblocks = 8L * cdiv(a.parts, 8) * a.nslab * a.mtiles;
  SD_REQUIRE(nblocks < (1L << 31) && (long)N * a.runs < (1L << 31), "too many workgroups");
  hipStream_t st = (hipStream_t)stream;
  SD_HIP_CHECK(hipFuncSetAttribute((const void*)dcn_wgrad_f16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   kWSmem));
  hipLaunchKernelGGL(dcn_wgrad_f16_kernel, dim3((unsigned)nblocks), dim3(kWThreads), kWSmem, st, a);
  SD_LAUNCH_CHECK();
  const long total = (long)F * a.nslab * kWCols;
  hipLaunchKernelGGL(dcn_wgrad_f16_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, a.part,
                     (__half*)d_weight, C, a.mtiles, a.nslab, a.parts, req_weight, total);
  SD_LAUNCH_CHECK();
  return SD_OK;
}
