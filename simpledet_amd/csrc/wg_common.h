// Workgroup primitives of the target and loss kernels, device only: ordered compaction of flagged lists
// (thread order is list order, one barrier pair per scan, totals carried from trip to trip) and fixed-order sums.
// Bit parity with the reference rests on their order of operations, so an operator file calls these and holds no copy.
#pragma once
#include "common.h"

namespace sd {

// flagged lanes in front of `lane` in a ballot: the rank of a flagged lane inside its wave
__device__ __forceinline__ int lanes_before(unsigned long long ballot, int lane) {
  return __popcll(ballot & ((1ull << lane) - 1));
}

// block-wide exclusive prefix sum of a 0/1 flag in thread order; returns this thread's offset and
// the block total (all threads must call)
template <int THREADS>
__device__ __forceinline__ int block_scan_flag(bool flag, int* wave_sums, int* total) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const unsigned long long b = __ballot(flag);
  const int within = lanes_before(b, lane);
  __syncthreads();  // wave_sums may still be read from a previous call
  if (lane == 0) wave_sums[wave] = __popcll(b);
  __syncthreads();
  int off = 0, tot = 0;
  for (int w = 0; w < THREADS / kWave; ++w) {
    const int v = wave_sums[w];
    if (w < wave) off += v;
    tot += v;
  }
  *total = tot;
  return off + within;
}

// The same for NF flags at once (the fg / bg list pairs): one ballot per flag, one barrier pair for all of them.
// off[f] comes in as the list's base (a scanned global offset, a running total) and goes out as base + this thread's
// offset; tot[f] is the block total.  REUSE = false drops the leading barrier: for a kernel that scans once, so that
// nobody can still be reading wave_sums.
template <int THREADS, int NF, bool REUSE = true>
__device__ __forceinline__ void block_scan_flags(const bool (&flag)[NF], int (*wave_sums)[THREADS / kWave],
                                                 int (&off)[NF], int (&tot)[NF]) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  unsigned long long b[NF];
#pragma unroll
  for (int f = 0; f < NF; ++f) b[f] = __ballot(flag[f]);
  if (REUSE) __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int f = 0; f < NF; ++f) wave_sums[f][wave] = __popcll(b[f]);
  }
  __syncthreads();
#pragma unroll
  for (int f = 0; f < NF; ++f) {
    tot[f] = 0;
    for (int w = 0; w < THREADS / kWave; ++w) {
      const int v = wave_sums[f][w];
      if (w < wave) off[f] += v;
      tot[f] += v;
    }
    off[f] += lanes_before(b[f], lane);
  }
}

// Ordered compaction of the rows of a list that pass a test, whatever its length: trips of THREADS rows, one
// block_scan_flag per trip, the count carried from trip to trip.  take(j) reads row j < n and says whether it stays,
// put(j, k) stores it as survivor k; survivors are numbered from `first` on.  Returns first + the number of
// survivors (all threads must call).  No barrier behind the last put: the caller places the one its readers need.
template <int THREADS, typename Take, typename Put>
__device__ __forceinline__ int block_compact_rows(int n, int* wave_sums, Take take, Put put, int first = 0) {
  int kept = first;
  for (int base = 0; base < n; base += THREADS) {
    const int j = base + (int)threadIdx.x;
    const bool ok = j < n && take(j);
    int tot;
    const int off = block_scan_flag<THREADS>(ok, wave_sums, &tot);
    if (ok) put(j, kept + off);
    kept += tot;
  }
  return kept;
}

// Fixed-order sums over a workgroup of THREADS threads: the wave butterflies (wave_sum_*), then the per-wave
// results pairwise, left to right -- (s0 + s1) + (s2 + s3) for the 256 threads of the FCOS, RepPoints and
// GroupNorm kernels.  `sh`: THREADS / kWave words of LDS that no other reduction in flight uses.  TRAIL = false
// leaves out the barrier behind the read (the caller does not write sh again before its next barrier).
template <int THREADS, bool TRAIL, typename T>
__device__ __forceinline__ T block_sum_waves(T wave_total, T* sh) {
  static_assert(THREADS % (2 * kWave) == 0, "an even number of waves");
  if ((threadIdx.x & (kWave - 1)) == 0) sh[threadIdx.x / kWave] = wave_total;
  __syncthreads();
  T r = sh[0] + sh[1];
#pragma unroll
  for (int w = 2; w < THREADS / kWave; w += 2) r = r + (sh[w] + sh[w + 1]);
  if (TRAIL) __syncthreads();
  return r;
}
template <int THREADS, bool TRAIL = true>
__device__ __forceinline__ float block_sum_f32(float v, float* sh) {
  return block_sum_waves<THREADS, TRAIL>(wave_sum_f32(v), sh);
}
template <int THREADS>
__device__ __forceinline__ int block_sum_i32(int v, int* sh) {
  return block_sum_waves<THREADS, true>(wave_sum_i32(v), sh);
}

}  // namespace sd
