// Stable descending top-k pieces shared by the selection kernels (nms.hip: NMS, Proposal_v3;
// gen_proposal_retina.hip): the score -> sort-key map, the LDS bitonic sort of composite
// (key, row) words, one 8-bit digit of a workgroup radix select and the single-workgroup
// stable top-k built from them.
#pragma once
#include "common.h"

namespace sd {

constexpr int kMaxSortKeys = 16384;

// Sort key of a score: smaller key = better score.  -0.0 and +0.0 get the SAME key (the reference's
// thrust::stable_sort_by_key(greater<float>) and MXNet's SortByKey compare them equal and keep
// their input order; the index in the low half of the 64-bit key does the same here).  NaN scores,
// which the reference's comparator leaves in an unspecified place, are ordered by their bits:
// positive NaNs before +inf, negative NaNs after -inf.
__device__ __forceinline__ unsigned ordered_desc_bits(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;                     // -0.0 == +0.0
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending-order-preserving map
  return ~u;                                        // descending
}

// position of this lane's item in an LDS list when the lanes with `take` append one item each: one LDS atomic
// per wave.  Every lane of the wave must call it.
__device__ __forceinline__ int wave_append(bool take, int* counter) {
  const unsigned long long m = __ballot(take);
  if (m == 0) return 0;
  const int lane = threadIdx.x & (kWave - 1);
  const int leader = __ffsll((long long)m) - 1;
  int wbase = 0;
  if (lane == leader) wbase = atomicAdd(counter, __popcll(m));
  wbase = __shfl(wbase, leader);
  return wbase + __popcll(m & ((1ull << lane) - 1ull));
}

// ascending bitonic sort of P2 (power of two) 64-bit keys in LDS by the whole workgroup.
// Stages with a pair distance j <= 64 only exchange inside aligned 128-key blocks, so a wave that
// owns such a block runs them back to back with no workgroup barrier (the LDS accesses of one wave
// are ordered): 2048 keys need 15 barriers instead of 66.
__device__ __forceinline__ void bitonic_stage(unsigned long long* keys, int t, int j, int k) {
  // pair (lo, lo + j) of the bitonic network; direction from bit k of lo
  const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
  const int hi = lo + j;
  const unsigned long long x = keys[lo], y = keys[hi];
  const bool up = (lo & k) == 0;
  if ((x > y) == up) {
    keys[lo] = y;
    keys[hi] = x;
  }
}

__device__ __forceinline__ void bitonic_sort_lds(unsigned long long* keys, int P2, int tid, int T) {
  if (P2 < 128 || (T & (kWave - 1))) {  // tiny inputs: every stage with a barrier
    for (int k = 2; k <= P2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < P2 / 2; t += T) bitonic_stage(keys, t, j, k);
        __syncthreads();
      }
    return;
  }
  const int lane = tid & (kWave - 1), wave = tid / kWave, nwaves = T / kWave;
  // phases 2 .. 128: every aligned 128-key block is sorted by one wave on its own
  for (int b = wave; b < P2 / 128; b += nwaves)
    for (int k = 2; k <= 128; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        bitonic_stage(keys, b * kWave + lane, j, k);
        wave_lds_sync();
      }
  __syncthreads();
  for (int k = 256; k <= P2; k <<= 1) {
    for (int j = k >> 1; j >= 128; j >>= 1) {  // pairs across blocks: whole workgroup + barrier
      for (int t = tid; t < P2 / 2; t += T) bitonic_stage(keys, t, j, k);
      __syncthreads();
    }
    for (int b = wave; b < P2 / 128; b += nwaves)  // j = 64 .. 1 inside the blocks
      for (int j = 64; j > 0; j >>= 1) {
        bitonic_stage(keys, b * kWave + lane, j, k);
        wave_lds_sync();
      }
    __syncthreads();
  }
}

// one 8-bit digit of a radix select among the elements whose key matches `prefix` under `mask`:
// returns the digit where the running count reaches `want` (1-based rank inside the matching set)
// and updates below (elements before that digit) -- all threads get the same values
template <typename KeyFn>
__device__ __forceinline__ int radix_digit(int count, int shift, unsigned mask, unsigned prefix,
                                           int want, int* hist, int* below, int* bucket,
                                           KeyFn key_of) {
  const int tid = threadIdx.x, T = blockDim.x;
  for (int i = tid; i < 256; i += T) hist[i] = 0;
  __syncthreads();
  // RPN scores share a handful of exponent bytes, so plain per-lane LDS atomics would serialise on
  // a few counters: lanes with the same digit are merged (ballot) into one atomic per wave
  constexpr int UN = 8;  // keys fetched per thread before any of them is counted (latency)
  for (int i0 = 0; i0 < count; i0 += UN * T) {
    unsigned kk[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int i = i0 + u * T + tid;
      kk[u] = i < count ? key_of(i) : ~prefix;  // ~prefix never matches under a non-empty mask
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int i = i0 + u * T + tid;
      int dg = -1;
      if (i < count && (kk[u] & mask) == prefix) dg = (int)((kk[u] >> shift) & 255);
      unsigned long long todo = __ballot(dg >= 0);
      for (int round = 0; round < 4 && todo; ++round) {  // popular digits first, merged
        const int leader = __ffsll((long long)todo) - 1;
        const int d0 = __builtin_amdgcn_readlane(dg, leader);
        const unsigned long long same = __ballot(dg == d0);
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[d0], __popcll(same));
        if (dg == d0) dg = -1;
        todo &= ~same;
      }
      if (dg >= 0) atomicAdd(&hist[dg], 1);  // whatever is left is spread over many counters
    }
  }
  __syncthreads();
  // wave 0 scans the 256 counters (4 per lane + a wave prefix sum) and publishes the digit where
  // the running count reaches `want`
  if (threadIdx.x < kWave) {
    const int lane = threadIdx.x;
    const int c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2],
              c3 = hist[4 * lane + 3];
    const int tot = c0 + c1 + c2 + c3;
    int incl = tot;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const int t = __shfl_up(incl, o);
      if (lane >= o) incl += t;
    }
    const int excl = incl - tot;
    if (excl < want && want <= incl) {  // exactly one lane
      int run = excl, d = 4 * lane, sz = c0;
      if (run + c0 < want) { run += c0; d = 4 * lane + 1; sz = c1;
        if (run + c1 < want) { run += c1; d = 4 * lane + 2; sz = c2;
          if (run + c2 < want) { run += c2; d = 4 * lane + 3; sz = c3; } } }
      hist[256] = d;
      hist[257] = run;
      hist[258] = sz;
    }
  }
  __syncthreads();
  const int digit = hist[256], lower = hist[257], size = hist[258];
  *below = lower;
  *bucket = size;
  __syncthreads();
  return digit;
}

// Stable top-`pre` of `count` scores by one workgroup: 8-bit radix select of the pre-th best score
// key, a second select on the row index when the ties at that key are only partly taken, unordered
// compaction of the selected rows into composite (key, row) words and an LDS sort of the P2 >= pre
// words.  keys[0 .. pre) end up in the order of a stable descending sort.
template <int STRIDE = 1>  // score of row i at sc[i * STRIDE]
__device__ __forceinline__ void select_sort_topk(const float* __restrict__ sc, int count, int pre,
                                                 int P2, unsigned long long* keys, int* hist,
                                                 int* ncand) {
  const int tid = threadIdx.x, T = blockDim.x;
  auto skey = [&](int i) { return ordered_desc_bits(sc[(long)i * STRIDE]); };  // ascending key = best score first
  // ---- the pre-th smallest score key ----
  unsigned prefix = 0, mask = 0;
  int want = pre, last_bucket = 0;
  for (int shift = 24; shift >= 0; shift -= 8) {
    int below;
    const int d = radix_digit(count, shift, mask, prefix, want, hist, &below, &last_bucket, skey);
    want -= below;
    prefix |= (unsigned)d << shift;
    mask |= 255u << shift;
  }
  const unsigned Tkey = prefix;  // `want` of the elements with this key are still needed
  const int n_eq = last_bucket;  // how many elements carry exactly this key
  // ---- ties on the score: the lowest rows win (stable sort); select the want-th smallest row
  //      (skipped when every tied element is taken, the usual case) ----
  unsigned Irow = 0xffffffffu;  // ties with row <= Irow are taken
  if (want < n_eq) {
    unsigned ipre = 0, imask = 0;
    int iwant = want;
    auto ikey = [&](int i) { return skey(i) == Tkey ? (unsigned)i : 0xffffffffu; };
    for (int shift = 24; shift >= 0; shift -= 8) {
      int below, bucket;
      // rows that do not carry Tkey map to 0xffffffff and never match a prefix below 2^24 rows
      const int d = radix_digit(count, shift, imask, ipre, iwant, hist, &below, &bucket, ikey);
      iwant -= below;
      ipre |= (unsigned)d << shift;
      imask |= 255u << shift;
    }
    Irow = ipre;
  }
  // ---- unordered compaction of the selected rows into composite keys, then sort ----
  if (tid == 0) *ncand = 0;
  for (int i = tid; i < P2; i += T) keys[i] = ~0ull;
  __syncthreads();
  for (int i0 = 0; i0 < count; i0 += 8 * T) {
    unsigned kk[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * T + tid;
      kk[u] = i < count ? skey(i) : 0xffffffffu;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int i = i0 + u * T + tid;
      const unsigned k = kk[u];
      if (i < count && (k < Tkey || (k == Tkey && (unsigned)i <= Irow))) {
        const int pos = atomicAdd(ncand, 1);
        if (pos < P2) keys[pos] = ((unsigned long long)k << 32) | (unsigned)i;
      }
    }
  }
  __syncthreads();
  bitonic_sort_lds(keys, P2, tid, T);
}

}  // namespace sd
