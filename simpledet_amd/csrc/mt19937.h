// MT19937 of numpy's legacy RandomState on the device: producer waves and a consumer wave.  Shared by the RPN
// anchor targets (rpn_target.hip) and the CrowdHuman RoI targets (crowdhuman_head.hip); the code is the RPN's of
// round 6, moved here so that both draw from one implementation: the stream, the producer, mt_need and mt_trip as
// they were, mt_batch / mt_open / mt_close, the draw loop (mt_permutation_draws) and the kernel's shell (mt_consume)
// cut out of rpn_sample and rpn_sample_kernel, statement for statement.
//
// Until round 5 ONE wave twisted the state and consumed it (2.7 ms for two images: a lone wave pays
// ~12 clocks per dependent instruction, and twist and rejection chain were one dependency chain).  The generator's
// raw output is a pure sequence -- X[j] = X[j - 227] ^ tw(X[j - 624], X[j - 623]) for j >= 624, X[0 .. 623] = the
// state's key words; all three sources lie >= 227 words back, so 227 consecutive words are independent -- and only
// WHERE in it each draw is taken depends on the data.  So the other waves of the workgroup produce the sequence
// into an LDS ring, 227 words per step, as far ahead as the ring allows, and the first wave consumes it (tempering
// on read); four waves share the production, 57 words of a step each.  The two meet through LDS counters only (release / acquire at workgroup scope; no s_barrier: the waves
// of one workgroup are co-resident by construction, the same guarantee a barrier rests on).  Every wait is a bounded
// spin: on overrun the kernel stops and raises its caller's overrun flag (the host entry point does not read it back --
// a wrong sample shows in the tests, a hang would cost a GPU).
#pragma once
#include "common.h"

namespace sd {

constexpr int kMtRing = 4096;        // words (16 KB raw + 16 KB tempered); the producers stay < kMtRing ahead of what the consumer still needs
constexpr int kMtSpinCap = 1 << 22;  // ~seconds of s_sleep polling
constexpr int kMtProd = 4;           // producer waves: wave w makes elements [57 w, 57 w + 57) of every 227-word step
constexpr int kMtSlice = 57;         // (227 = 3 * 57 + 56)
constexpr int kMtThreads = (1 + kMtProd) * kWave;   // the workgroup of a sampling kernel: the consumer wave first

struct MtStream {
  unsigned* ring;   // LDS: word j of the sequence at ring[j & (kMtRing - 1)] (raw: what the recurrence and the state need)
  unsigned* tring;  // LDS: the same word tempered (what a draw returns), written by the producers beside it
  int* ctl;         // LDS: [0..3] steps completed by the producer waves, [4] first word the consumer still needs,
                    //      [5] stop, [6] overrun
  int pos;          // consumer: index of the next output (wave uniform)
};

__device__ __forceinline__ int mt_ld(const int* p) {
  return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ void mt_st(int* p, int v) {
  __hip_atomic_store(p, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
}
// steps every producer wave has completed (one 16-byte LDS read)
__device__ __forceinline__ int mt_steps_done(const int* ctl) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i d = *reinterpret_cast<const volatile v4i*>(ctl);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  return iminr(iminr(d.x, d.y), iminr(d.z, d.w));
}

__device__ __forceinline__ unsigned mt_temper(unsigned y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

// Producer wave w: elements [57 w, 57 w + 57) of every step, TWO steps per hand-shake.  Word j = 624 + 227 s + e
// reads j - 227 (the same element of step s - 1: this wave's own word -- inside a pair it never leaves the
// register) and j - 624 / j - 623 = elements e + 57 / e + 58 of step s - 3 (or e - 170 / e - 169 of step s - 2):
// other waves' words, at least two steps back.  So once every wave has completed step s - 1, steps s AND s + 1 can
// be made without another look at the others: one round of flag reads per 454 words.  (A hand-shake is two or three
// dependent LDS round trips of a wave that issues an instruction every ~12 clocks: with one per step the four
// producers delivered 0.23 words per clock against the 0.45 the consumer takes.)  Runs until ctl[5] is raised.
__device__ inline void mt_produce(unsigned* ring, unsigned* tring, int* ctl, int w, int lane) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  const int e = w * kMtSlice + lane;
  const bool mine = lane < kMtSlice && e < 227;
  auto tw = [](unsigned far, unsigned a, unsigned b) {
    const unsigned y = (a & 0x80000000u) | (b & 0x7fffffffu);
    return far ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  };
  for (int s = 0;; s += 2) {
    const int made = 624 + 227 * s;   // first word of the pair of steps
    int spins = 0;
    while (true) {
      const v4i d = *reinterpret_cast<const volatile v4i*>(ctl);       // steps completed by the four producers
      const v4i c = *reinterpret_cast<const volatile v4i*>(ctl + 4);   // consumer floor, stop, overrun
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      if (c.y) return;
      // word j overwrites word j - kMtRing: everything from the consumer's floor on stays
      if (made + 454 <= c.x + kMtRing - 64 && iminr(iminr(d.x, d.y), iminr(d.z, d.w)) >= s) break;
      __builtin_amdgcn_s_sleep(1);
      if (++spins > kMtSpinCap) { mt_st(ctl + 6, 1); return; }
    }
    if (mine) {
      const int j = made + e, j1 = j + 227;
      const unsigned f0 = ring[(j - 227) & (kMtRing - 1)];
      const unsigned a0 = ring[(j - 624) & (kMtRing - 1)], b0 = ring[(j - 623) & (kMtRing - 1)];
      const unsigned a1 = ring[(j1 - 624) & (kMtRing - 1)], b1 = ring[(j1 - 623) & (kMtRing - 1)];
      const unsigned x0 = tw(f0, a0, b0), x1 = tw(x0, a1, b1);
      ring[j & (kMtRing - 1)] = x0;
      ring[j1 & (kMtRing - 1)] = x1;
      // (tempered beside it: the consumer is a lone wave too, every instruction taken off it counts)
      tring[j & (kMtRing - 1)] = mt_temper(x0);
      tring[j1 & (kMtRing - 1)] = mt_temper(x1);
    }
    mt_st(ctl + w, s + 2);   // (release: behind the ring writes)
  }
}

// consumer: words [pos, pos + n) are there (false on overrun)
__device__ __forceinline__ bool mt_need(MtStream& m, int n) {
  int spins = 0;
  while (624 + 227 * mt_steps_done(m.ctl) < m.pos + n) {
    __builtin_amdgcn_s_sleep(1);
    if (++spins > kMtSpinCap || mt_ld(m.ctl + 6)) { mt_st(m.ctl + 6, 1); return false; }
  }
  return true;
}

// the rejection mask of Fisher-Yates step i (rk_interval(i)): the smallest 2^k - 1 >= i
__device__ __forceinline__ unsigned mt_mask(int i) {
  unsigned mask = (unsigned)i;
  mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
  return mask;
}

// NB batches of 64 draws in ONE dependent step, exactly.  Draw t accepts iff v_t <= i - A(t), A(t) = accepts in
// front of it.  The CANDIDATES (v <= i) are the only draws that can accept, and the number of candidates up to the
// end of a draw's batch bounds its A(t) from above: v <= i - that is a sure accept.  What is left -- candidates
// with i - bound < v <= i, about bound / mask of them -- is a handful per trip; they are settled one after the
// other in order with their exact rank (each rejection lowers the A of everything behind it by one).  Per batch
// that is one LDS read, two compares and a few scalar operations, independent of the other batches.  Returns the
// number of accepts, or -1 when the trip would leave the mask's segment (the caller then goes batch by batch).
template <int NB>
__device__ __forceinline__ int mt_trip(const MtStream& m, int i, int lo, unsigned mask, int lane) {
  int vv[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) vv[j] = (int)(m.tring[(m.pos + j * kWave + lane) & (kMtRing - 1)] & mask);
  unsigned long long cand[NB], amb[NB];
  int base[NB + 1];
  base[0] = 0;
  unsigned long long anyamb = 0;
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    cand[j] = __ballot(vv[j] <= i);
    base[j + 1] = base[j] + __popcll(cand[j]);
    amb[j] = __ballot(vv[j] > i - base[j + 1]) & cand[j];
    anyamb |= amb[j];
  }
  int K = base[NB];
  if (anyamb) {
    int rej = 0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      unsigned long long todo = amb[j];
      while (todo) {
        const int t = __builtin_ctzll(todo);
        todo &= todo - 1;
        const int vt = __builtin_amdgcn_readlane(vv[j], t);
        const int rt = base[j] + __popcll(cand[j] & ((1ull << t) - 1));
        if (vt > i - rt + rej) ++rej;
      }
    }
    K -= rej;
  }
  return K < i - lo + 1 ? K : -1;
}

// ONE batch of 64 draws at Fisher-Yates step i, exactly, with every accepted draw known: lane t holds draw t
// (v = its masked value) and `acc` says whether it is accepted; an accepted lane's step is i - popcount(bits below
// it).  Steps i in [lo, mask] share the rejection mask; when the batch would leave that segment it ends behind the
// accept that closes it (`consumed` < 64 draws are taken, the rest is re-read with the next mask).  Returns the
// number of accepts.  The words [pos, pos + 64) must be there (mt_need).
__device__ __forceinline__ int mt_batch(const MtStream& m, int i, int lo, unsigned mask, int lane, unsigned& v,
                                        bool& acc, unsigned long long& bits, int& consumed) {
  const unsigned long long lt = (1ull << lane) - 1;
  v = m.tring[(m.pos + lane) & (kMtRing - 1)] & mask;
  acc = v <= (unsigned)i;
  bits = __ballot(acc);
  while (true) {  // ballot / popcount fixed point: exact, 1-2 rounds
    const int c = __popcll(bits & lt);
    const bool acc2 = (long)v <= (long)i - c;
    const unsigned long long b2 = __ballot(acc2);
    acc = acc2;
    if (b2 == bits) break;
    bits = b2;
  }
  int K = __popcll(bits);
  const int R = i - lo + 1;  // accepts this mask still serves
  consumed = kWave;
  if (K >= R) {
    // the R-th accept ends the segment; later draws of the batch are re-read with the next mask
    // (also when it is the batch's last accept: the rejected draws behind it were judged with
    // the old mask, numpy judges them with the halved one -- found by the generator fuzz test)
    unsigned long long b = bits;
    for (int s = 1; s < R; ++s) b &= b - 1;
    const int last = __ffsll((long long)b) - 1;
    consumed = last + 1;
    bits &= (2ull << last) - 1ull;
    acc = acc && lane <= last;
    K = R;
  }
  return K;
}

// Start of a sampling kernel, all kMtThreads threads: the key words are the first 624 words of the sequence (a
// stored position of 624, "twist before the next draw", is simply the next word); clears the control words.  The
// caller's __syncthreads() behind it is the kernel's only barrier: then the waves part.
__device__ __forceinline__ void mt_open(unsigned* ring, unsigned* tring, int* ctl, const int* mt) {
  for (int k = threadIdx.x; k < 624; k += kMtThreads) {
    ring[k] = (unsigned)mt[k];
    tring[k] = mt_temper(ring[k]);
  }
  if (threadIdx.x < 8) ctl[threadIdx.x] = 0;
}

// End of the consumer wave: the state numpy would hold now -- the block the last draw came from and the position
// behind it (624 = "twist before the next draw"); untouched when nothing was drawn.  The block is still in the
// ring: the producer never overwrites anything from ctl[4] = pos - 624 on.  Then the producers may leave.
// Returns whether the stream overran (the sample is not valid).
__device__ __forceinline__ bool mt_close(MtStream& m, int pos0, int* mt, int lane) {
  if (m.pos != pos0 && !mt_ld(m.ctl + 6)) {
    const int b0 = ((m.pos - 1) / 624) * 624;
    int spins = 0;   // (the block's tail may still be on its way)
    while (624 + 227 * mt_steps_done(m.ctl) < b0 + 624 && ++spins <= kMtSpinCap) __builtin_amdgcn_s_sleep(1);
    for (int k = lane; k < 624; k += kWave) mt[k] = (int)m.ring[(b0 + k) & (kMtRing - 1)];
    if (lane == 0) mt[624] = m.pos - b0;
  }
  const bool overrun = mt_ld(m.ctl + 6) != 0;
  mt_st(m.ctl + 5, 1);
  return overrun;
}

// permutation(n) of the legacy RandomState, consumer wave: Fisher-Yates step s = 0 .. n - 2 swaps position
// i = n - 1 - s with an accepted draw v, handed to record(s, v) by the lane that holds it; the generator advances by
// exactly the draws numpy consumes.  trip_size(i, s): batches of 64 draws in the next dependent step -- 2, 8 or 16
// (mt_trip: accepts counted, not recorded) or 1 (mt_batch: every accept recorded; also the fall-back when a trip
// would leave its mask's segment).  A constant 1 compiles the trips out.  False when the stream overran.
template <typename TripSize, typename Record>
__device__ __forceinline__ bool mt_permutation_draws(MtStream& m, int n, int lane, TripSize trip_size, Record record) {
  int i = n - 1;
  const unsigned long long lt = (1ull << lane) - 1;
  while (i >= 1) {
    // the consumer no longer needs anything before the block its last draw came from (the final state is that block)
    mt_st(m.ctl + 4, m.pos > 624 ? m.pos - 624 : 0);
    const int nb = trip_size(i, (n - 1) - i);
    if (!mt_need(m, nb * kWave)) return false;
    const unsigned mask = mt_mask(i);
    const int lo = (int)(mask >> 1) + 1;  // steps i in [lo, mask] share this rejection mask
    if (nb > 1) {
      const int K = nb == 16 ? mt_trip<16>(m, i, lo, mask, lane) : nb == 8 ? mt_trip<8>(m, i, lo, mask, lane)
                                                                          : mt_trip<2>(m, i, lo, mask, lane);
      if (K >= 0) {
        i -= K;
        m.pos += nb * kWave;
        continue;
      }
    }
    unsigned v;
    bool acc;
    unsigned long long bits;
    int consumed;
    const int K = mt_batch(m, i, lo, mask, lane, v, acc, bits, consumed);
    if (acc) record((n - 1) - (i - __popcll(bits & lt)), v);  // 0-based index of this swap
    i -= K;
    m.pos += consumed;
  }
  return true;
}

// The shell of a sampling kernel (ONE workgroup of kMtThreads): ring and control words in LDS, mt_open, the kernel's
// only barrier, then the waves part.  Waves 1 .. kMtProd produce until the consumer closes the stream and get
// kMtProducer back.  Wave 0 calls body(m, img) for the images in order (the generator state carries from image to
// image) until one stalls the stream, writes back the state numpy would hold now (mt_close) and gets 1 if the stream
// overran (the sample is not valid), 0 if not.
constexpr int kMtProducer = -1;
template <typename Body>
__device__ __forceinline__ int mt_consume(int* mt, int B, Body body) {
  __shared__ unsigned ring[kMtRing], tring[kMtRing];
  __shared__ __attribute__((aligned(16))) int ctl[8];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  mt_open(ring, tring, ctl, mt);
  __syncthreads();   // (the only barrier: before the waves part)
  if (wave >= 1) {
    mt_produce(ring, tring, ctl, wave - 1, lane);
    return kMtProducer;
  }
  MtStream m{ring, tring, ctl, mt[624]};
  const int pos0 = m.pos;
  for (int img = 0; img < B && !mt_ld(ctl + 6); ++img) body(m, img);
  return mt_close(m, pos0, mt, lane) ? 1 : 0;
}

}  // namespace sd
