// What the fp16 DeformableConvolution kernels share (deform_fused_f16.hip: the forward, DESIGN 4.27;
// deform_wgrad_f16.hip: the weight gradient): unaligned half loads, the channel-interleaved x window
// in LDS, the bilinear sample rounded once to fp16.
#pragma once
#include "deform_split.h"
#include <hip/hip_fp16.h>
#pragma clang fp contract(off)

namespace sd {

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// eight consecutive halves from a pointer aligned to 2 bytes only: the widest loads its address allows,
// never a byte outside [p, p + nvalid)
__device__ __forceinline__ u32x4 ldg8_f16(const __half* p, int nvalid) {
  u32x4 r = {0u, 0u, 0u, 0u};
  const unsigned short* us = reinterpret_cast<const unsigned short*>(p);
  const uintptr_t ad = (uintptr_t)p;
  if (nvalid >= 8) {
    if ((ad & 15) == 0) {
      r = *reinterpret_cast<const u32x4*>(p);
    } else if ((ad & 7) == 0) {
      const u32x2 lo = reinterpret_cast<const u32x2*>(p)[0], hi = reinterpret_cast<const u32x2*>(p)[1];
      r[0] = lo[0]; r[1] = lo[1]; r[2] = hi[0]; r[3] = hi[1];
    } else if ((ad & 3) == 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = reinterpret_cast<const unsigned*>(p)[k];
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = (unsigned)us[2 * k] | ((unsigned)us[2 * k + 1] << 16);
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const unsigned lo = 2 * k < nvalid ? us[2 * k] : 0u, hi = 2 * k + 1 < nvalid ? us[2 * k + 1] : 0u;
      r[k] = lo | (hi << 16);
    }
  }
  return r;
}

// eight positions x one channel pair (planar in a, b) into the window buffer: position j of group pg lives in
// slot 9 pg + j
__device__ __forceinline__ void xwin_store(char* xb, int pg, int cp, u32x4 a, u32x4 b) {
  unsigned* d = reinterpret_cast<unsigned*>(xb + (pg * 9) * 32 + cp * 4);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const unsigned wa = a[j >> 1], wb = b[j >> 1];
    d[j * 8] = (j & 1) ? ((wa >> 16) | (wb & 0xffff0000u)) : ((wa & 0xffffu) | (wb << 16));
  }
}

// two channels of one sample: the four corners widened, sd_deform_im2col's expression in its order, 0 outside the
// image, one RNE to fp16 each
__device__ __forceinline__ unsigned bilerp2_f16(unsigned a, unsigned b, unsigned c, unsigned d, float w1, float w2,
                                                float w3, float w4, bool inside) {
  const floatx2 fa = __builtin_convertvector(__builtin_bit_cast(halfx2, a), floatx2);
  const floatx2 fb = __builtin_convertvector(__builtin_bit_cast(halfx2, b), floatx2);
  const floatx2 fc = __builtin_convertvector(__builtin_bit_cast(halfx2, c), floatx2);
  const floatx2 fd = __builtin_convertvector(__builtin_bit_cast(halfx2, d), floatx2);
  float v0 = (w1 * fa[0] + w2 * fb[0] + w3 * fc[0] + w4 * fd[0]);
  float v1 = (w1 * fa[1] + w2 * fb[1] + w3 * fc[1] + w4 * fd[1]);
  if (!inside) v0 = v1 = 0.f;
  const floatx2 v = {v0, v1};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, halfx2));
}

__device__ __forceinline__ void f16_lds_barrier() {   // LDS hand-over: does not wait for global loads in flight
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

// the shapes the native-half kernels take (every other shape runs the float32 operator on widened operands)
static inline bool dcn_f16_fused_ok(int C, int H, int W, int kh, int kw, int dgroup, int num_group) {
  return kh == 3 && kw == 3 && num_group == 1 && dgroup > 0 && C % dgroup == 0 && (C / dgroup) % 16 == 0 &&
         (long)H * W < (1L << 28);
}

static inline bool out_hw(int H, int W, int kh, int kw, int pad, int stride, int dil, long& Ho, long& Wo) {
  if (stride <= 0) return false;
  Ho = (H + 2 * pad - (dil * (kh - 1) + 1)) / stride + 1;
  Wo = (W + 2 * pad - (dil * (kw - 1) + 1)) / stride + 1;
  return Ho > 0 && Wo > 0;
}

}  // namespace sd
