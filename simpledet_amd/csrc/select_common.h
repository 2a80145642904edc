// The single implementation of the stable descending top-k ("Selection rule"): the
// score -> sort-key map, the size and the LDS bitonic sort of composite (key, row) words, the pick of
// the counter that holds a rank (256 digit counters or a histogram of bins), one 8-bit digit of a
// workgroup radix select, the row select among partly taken ties, the single-workgroup stable top-k
// built from them and the flush of a workgroup's candidate list.
// Users: nms.hip (_contrib_NMS, Proposal / Proposal_v2 / Proposal_v3, get_top_proposal),
// gen_proposal_retina.hip (GenProposalRetina), fcos_decode.hip (FCOS decode), reppoints_decode.hip
// (RepPoints decode) and bbox_post.hip (BboxPostProcessing: the LDS sort).
#pragma once
#include "common.h"

namespace sd {

constexpr int kMaxSortKeys = 16384;

// keys an LDS sort of n words runs over: the first power of two >= n, counted up from `start`
__host__ __device__ __forceinline__ int sort_size(int n, int start) {
  int p = start;
  while (p < n) p <<= 1;
  return p;
}

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

// inclusive prefix sum over wave 0 (lane = threadIdx.x) through __shfl_up
__device__ __forceinline__ int wave0_scan_shfl(int lane, int tot) {
  int incl = tot;
#pragma unroll
  for (int o = 1; o < kWave; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  return incl;
}

// The digit or bin where the running count of 256 counters reaches `want` (1-based): the 64 lanes of wave 0 scan
// them (4 per lane + the wave prefix sum `scan(lane, total)`), and the one lane whose four counters hold the rank
// publishes (digit, count below it, its size) in out[0 .. 3).  Called by wave 0 only, between two barriers.
template <typename Scan>
__device__ __forceinline__ void rank_pick256(int lane, const int* ctr, int want, int* out, Scan scan) {
  const int c0 = ctr[4 * lane], c1 = ctr[4 * lane + 1], c2 = ctr[4 * lane + 2], c3 = ctr[4 * lane + 3];
  const int tot = c0 + c1 + c2 + c3, incl = scan(lane, tot), excl = incl - tot;
  if (excl < want && want <= incl) {  // exactly one lane
    int run = excl, d = 4 * lane, sz = c0;
    if (run + c0 < want) { run += c0; d = 4 * lane + 1; sz = c1;
      if (run + c1 < want) { run += c1; d = 4 * lane + 2; sz = c2;
        if (run + c2 < want) { run += c2; d = 4 * lane + 3; sz = c3; } } }
    out[0] = d;
    out[1] = run;
    out[2] = sz;
  }
}
// with the __shfl_up scan (radix_digit, nms.hip's topk_resolve); reppoints_decode.hip passes its DPP scan
__device__ __forceinline__ void rank_pick256(const int* ctr, int want, int* out) {
  rank_pick256(threadIdx.x, ctr, want, out, wave0_scan_shfl);
}

// cut-off bin of the `want`-th best key from a global histogram of BINS bins (total >= want); wave 0
// scans, every thread of the workgroup gets the result; sh: LDS scratch of 3 ints
template <int BINS>
__device__ __forceinline__ void hist_cut_bin(const int* __restrict__ gh, int want, int* sh, int* bstar,
                                             int* below, int* nb) {
  __syncthreads();
  if (threadIdx.x < kWave) {
    const int lane = threadIdx.x;
    const int4* h4 = reinterpret_cast<const int4*>(gh + lane * (BINS / kWave));
    int tot = 0;
#pragma unroll
    for (int q = 0; q < BINS / kWave / 4; ++q) {
      const int4 v = h4[q];
      tot += v.x + v.y + v.z + v.w;
    }
    const int incl = wave0_scan_shfl(lane, tot), excl = incl - tot;
    if (excl < want && want <= incl) {  // exactly one lane
      int run = excl, b = lane * (BINS / kWave);
      const int bend = b + BINS / kWave - 1;
      while (b < bend && run + gh[b] < want) run += gh[b++];
      sh[0] = b;
      sh[1] = run;
      sh[2] = gh[b];
    }
  }
  __syncthreads();
  *bstar = sh[0];
  *below = sh[1];
  *nb = sh[2];
  __syncthreads();
}

// A workgroup of T threads moves its LDS list of n > 0 items (n read from *nl behind a barrier, the same in every
// thread) to a global list: one reservation on *gcount for the whole workgroup, the items that land below `cap`
// copied out, the LDS count reset.  The caller's next barrier orders the reset.
template <int T, typename W>
__device__ __forceinline__ void wg_list_flush(const W* list, int n, int* nl, int* base, int* gcount, W* dst,
                                              int cap) {
  const int tid = threadIdx.x;
  if (tid == 0) *base = atomicAdd(gcount, n);
  __syncthreads();
  const int b = *base;
  for (int j = tid; j < n; j += T)
    if (b + j < cap) dst[b + j] = list[j];
  __syncthreads();
  if (tid == 0) *nl = 0;
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
  if (threadIdx.x < kWave) rank_pick256(hist, want, hist + 256);
  __syncthreads();
  const int digit = hist[256], lower = hist[257], size = hist[258];
  *below = lower;
  *bucket = size;
  __syncthreads();
  return digit;
}

// Ties on the score key Tkey that are only partly taken: the lowest rows win (stable sort).  Returns the
// want-th smallest row among the rows whose key skey(i) is Tkey; ties with row <= that row are taken.
template <typename KeyFn>
__device__ __forceinline__ unsigned select_tie_row(int count, int want, unsigned Tkey, int* hist,
                                                   KeyFn skey) {
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
  return ipre;
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
  // ---- ties on the score: select the want-th smallest tied row (skipped when every tied element
  //      is taken, the usual case) ----
  unsigned Irow = 0xffffffffu;  // ties with row <= Irow are taken
  if (want < n_eq) Irow = select_tie_row(count, want, Tkey, hist, skey);
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
