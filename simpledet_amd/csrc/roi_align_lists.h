// Band list of the RoIAlign backward: shared by the rois-only pre-pass (roi_align_prep.hip) and by the
// workgroups of roi_align_bwd_packed4 that run without a workspace (roi_align_bwd.hip).  And the two rois-only
// blocks that run either in a pre-pass launch (roi_align_prep.hip) or as tasks in the tail of the band forward
// (roi_align_fwd.hip): the packed arg-max's coordinate table and the backward's per-unit lists / tap tables.
#pragma once
#include "roi_align_common.h"

namespace sd {

// RoIs of image `img` whose taps can fall on rows [row0, row1) of level `lvl`, in RoI order (ballot
// + prefix over the waves, no atomic slot counter: the list and everything derived from it are a
// deterministic function of the inputs), and the band's weight bound (see roi_align_bwd_packed4).
// list[0 .. count), nlist[0] = count, nlist[1] = bound; wcnt: THREADS / 64 words of scratch.
// Ends with a barrier.
template <int PH, int PW, int THREADS>
__device__ __forceinline__ void bwd_band_list(const BwdFusedArgs& a, int lvl, int img, int nbands, int row0,
                                              int row1, float4 rb0, int* list, int* nlist, int* wcnt) {
  constexpr int NW = THREADS / kWave;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
  const int H = a.L.H[lvl];
  const float scale = a.L.scale[lvl];
  int base = 0, bound_sum = 0;
  for (int r0 = 0; r0 < a.R; r0 += THREADS) {
    const int r = r0 + tid;
    bool take = r < a.R && !(SD_ABLATE(a, 4));  // (profiling build, 4: empty lists)
    int weight = 0;
    if (take) {
      // (a copy, then an overwrite: `r0 == 0 ? rb0 : *p` selects between two lvalues, takes rb0's address
      // and puts it -- 32 bytes per lane -- in scratch)
      float4 rb = rb0;
      if (r0 != 0) rb = *reinterpret_cast<const float4*>(a.rois + ((long)img * a.R + r) * 4);
      if (a.filter) take = fpn_level(rb.x, rb.y, rb.z, rb.w, a.L) == lvl;
      if (take && nbands > 1) {
        // conservative row range of every tap of this RoI (taps lie within the clipped bins +-1)
        float s = fminr(fmaxr(rb.y * scale, 0.f), (float)(H - 1));
        float e = fminr(fmaxr(rb.w * scale, 0.f), (float)(H - 1));
        float lo = fminr(s, e) - 2.f, hi = fmaxr(s, e) + 2.f;
        if (hi < (float)row0 || lo > (float)(row1 - 1)) take = false;
      }
      if (take) {
        // bins of this RoI that can put weight on one pixel (see the header comment); a degenerate
        // or NaN width compares false and counts every bin
        // (hardware reciprocal, 1 ulp, with a 1e-5 safety factor: the count may only err upwards)
        const float bwx = (rb.z - rb.x) * scale * (1.f / (float)PW), bwy = (rb.w - rb.y) * scale * (1.f / (float)PH);
        const float fx = 2.00002f * __builtin_amdgcn_rcpf(bwx), fy = 2.00002f * __builtin_amdgcn_rcpf(bwy);
        const int nx = (bwx > 0.f && fx < (float)PW) ? iminr((int)fx + 2, PW) : PW;
        const int ny = (bwy > 0.f && fy < (float)PH) ? iminr((int)fy + 2, PH) : PH;
        weight = nx * ny;
      }
    }
    const unsigned long long mask = __ballot(take);
    bound_sum += wave_sum_i32(weight);
    if (r0 > 0) __syncthreads();  // wcnt of the previous sweep has been read
    if (lane == 0) wcnt[wave] = __popcll(mask);
    __syncthreads();
    int off = base, total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      const int n = wcnt[w];
      if (w < wave) off += n;
      total += n;
    }
    if (take) list[off + __popcll(mask & ((1ull << lane) - 1))] = r;
    base += total;
  }
  if (lane == 0) atomicAdd(nlist + 1, bound_sum);
  if (tid == 0) nlist[0] = base;
  __syncthreads();
}

// ---- packed arg-max: the per-RoI sample-coordinate table (what roi_coords_kernel writes), block `cb` of
// kBandThreads (RoI, coordinate) pairs.  An output of the op that no forward kernel reads: a block of the pre-pass
// (band_prep_block) or a task in the tail of the band kernel.  G: a.L, as the memory the per-lane level index reads
// the geometry from. ----
template <int POOL>
__device__ __forceinline__ void coords_block(const FwdArgs& a, const RoiLevels& G, int cb) {
  const long e = (long)cb * kBandThreads + threadIdx.x;
  if (e >= (long)a.B * a.R * 6 * POOL) return;
  const int j = (int)(e % (6 * POOL)), n = (int)(e / (6 * POOL));
  const float4 bx = *reinterpret_cast<const float4*>(a.rois + (long)n * 4);
  const int lvl = a.L.nlvl > 1 ? fpn_level(bx.x, bx.y, bx.z, bx.w, a.L) : 0;
  if (lvl < 0) return;
  // (lvl differs from lane to lane: the geometry comes through G, see the band kernel)
  const float scale = G.scale[lvl];
  const int H = G.H[lvl], W = G.W[lvl];
  const bool row = j < 3 * POOL;
  const int jj = row ? j : j - 3 * POOL;
  const float v = row ? sample_coord(jj / 3, POOL, bx.y, bx.w, scale, H, jj % 3)
                      : sample_coord(jj / 3, POOL, bx.x, bx.z, scale, W, jj % 3);
  float* cbase = a.coords + (long)n * kCoordWords * (POOL + POOL);
  cbase[j] = v;
  store_tap(cbase + 3 * (POOL + POOL) + 2 * j, v, row ? H : W);
}

// Pre-pass per (level, image, band) unit: its list into the workspace, read by the 256 channel
// workgroups of roi_align_bwd_packed4 instead of being rebuilt by each of them.
// A pure function of `rois` (and the level geometry): the sample coordinates are recomputed with
// sample_coord() -- the very expression the forward fills its coordinate table with -- instead of
// being read from that table, so these blocks depend on nothing the forward builds and can run in the
// forward's own launches: as blocks of the merged pre-pass (roi_prep_merged_kernel) or as tasks in the
// tail of the band kernel (roi_align_fwd_band).  Every path out of the block is workgroup-uniform.
template <int PH, int PW, int THREADS, int PARTS>
__device__ __forceinline__ void bwd_lists_block(const BwdFusedArgs& a, int block, float* smem) {
  int* list = reinterpret_cast<int*>(smem);
  int* nlist = list + a.R;
  const int tid = threadIdx.x;
  // PARTS workgroups per unit: each builds the (cheap) list, the first stores it, all share
  // the tap entries -- the entry loop is a chain of dependent round trips (list -> box ->
  // entry), so more workgroups shorten the pre-pass
  // (round 6: one more workgroup per unit when the bands get a per-pixel weight bound -- it builds the list and
  // the bound and no tap entries, so the bound is off the tap workgroups' chain)
  const int NP = PARTS + (a.pix_bound_words > 0 ? 1 : 0);
  const int unit = block / NP, part = block % NP;
  int li = 0;
  while (li + 1 < a.nlaunch && unit >= a.unit_base[li + 1]) ++li;
  const int lvl = a.order[li];
  const int u = unit - a.unit_base[li];
  const int nbands = a.nbands[lvl];
  const int img = u / nbands, band = u % nbands;
  const int row0 = band * a.band_rows[lvl];
  const int row1 = iminr(row0 + a.band_rows[lvl], a.L.H[lvl]);
  float4 rb0 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < a.R) rb0 = *reinterpret_cast<const float4*>(a.rois + ((long)img * a.R + tid) * 4);
  if (tid < 8) nlist[tid] = 0;
  __syncthreads();
  bwd_band_list<PH, PW, THREADS>(a, lvl, img, nbands, row0, row1, rb0, list, nlist, nlist + 8);
  int* dst = a.ws_list + (long)unit * (a.R + 2);
  const int nl = nlist[0];
  // Round 6: the weight bound per CELL of 4 x 4 pixels.  bwd_band_list sums nx * ny over every RoI of the band
  // (1,000-1,800 at the baseline), but a RoI can put weight only on the pixels of its own clipped box +-2: every RoI
  // adds its nx * ny to the rectangle of cells its footprint touches in a 2-D difference array of the band, a row
  // prefix (wave scans) and a column prefix (only its maximum is kept) give the largest bound any cell -- hence any
  // pixel -- of the band can reach: typically 30-150.  The fixed-point unit of the channel workgroups is 2^-30 of
  // (max|dY| x this bound): an order of magnitude finer, and an order of magnitude more dynamic range before a
  // workgroup has to take the float adds (kFxRangeBits).  (Per pixel the array is 7 k words for a P2 band and its
  // scans put 2 us on the pre-pass, which the forward waits for; per cell it is 600 words and costs nothing
  // measurable.)  Done by the unit's extra workgroup (part == PARTS), once per unit and launch.
  const int H = a.L.H[lvl], W = a.L.W[lvl];
  constexpr int CS = 2;   // log2 of the cell edge
  const int DW = ((W - 1) >> CS) + 2, DH = ((row1 - row0 - 1) >> CS) + 2;
  const bool pix = DW * DH <= a.pix_bound_words;
  if (part == 0) {
    if (tid == 0) dst[0] = nl;
    if (tid == 1 && !pix) dst[1] = nlist[1];
    for (int i = tid; i < nl; i += THREADS) dst[2 + i] = list[i];
  }
  if (part == PARTS && !pix) return;   // this level's bands are too large for the difference array
  if (part == PARTS) {
    constexpr int NW = THREADS / kWave;
    const int wave = tid / kWave, lane = tid & (kWave - 1);
    int* D = nlist + 8 + 16;
    for (int i = tid; i < DW * DH; i += THREADS) D[i] = 0;
    __syncthreads();
    const float scale = a.L.scale[lvl];
    for (int j = tid; j < nl; j += THREADS) {
      const float4 rb = *reinterpret_cast<const float4*>(a.rois + ((long)img * a.R + list[j]) * 4);
      // pixels the taps of this RoI can reach: the clipped box +-2 (the list's own row test); anything else
      // (NaN / inf coordinates) counts on the whole band
      const float xs = fminr(fmaxr(rb.x * scale, 0.f), (float)(W - 1)), xe = fminr(fmaxr(rb.z * scale, 0.f), (float)(W - 1));
      const float ys = fminr(fmaxr(rb.y * scale, 0.f), (float)(H - 1)), ye = fminr(fmaxr(rb.w * scale, 0.f), (float)(H - 1));
      const float xlo = fminr(xs, xe) - 2.f, xhi = fmaxr(xs, xe) + 2.f;
      const float ylo = fminr(ys, ye) - 2.f, yhi = fmaxr(ys, ye) + 2.f;
      int x0 = 0, x1 = W - 1, y0 = 0, y1 = H - 1;
      if (xlo >= -2.f && xhi <= (float)(W + 1)) { x0 = imaxr((int)floorf(xlo), 0); x1 = iminr((int)ceilf(xhi), W - 1); }
      if (ylo >= -2.f && yhi <= (float)(H + 1)) { y0 = imaxr((int)floorf(ylo), 0); y1 = iminr((int)ceilf(yhi), H - 1); }
      y0 = imaxr(y0, row0) - row0;
      y1 = iminr(y1, row1 - 1) - row0;
      if (y0 > y1) continue;
      x0 >>= CS; x1 >>= CS; y0 >>= CS; y1 >>= CS;   // cells
      const float bwx = (rb.z - rb.x) * scale * (1.f / (float)PW), bwy = (rb.w - rb.y) * scale * (1.f / (float)PH);
      const float fx = 2.00002f * __builtin_amdgcn_rcpf(bwx), fy = 2.00002f * __builtin_amdgcn_rcpf(bwy);
      const int nx = (bwx > 0.f && fx < (float)PW) ? iminr((int)fx + 2, PW) : PW;
      const int ny = (bwy > 0.f && fy < (float)PH) ? iminr((int)fy + 2, PH) : PH;
      const int w = nx * ny;
      atomicAdd(D + y0 * DW + x0, w);
      atomicAdd(D + y0 * DW + x1 + 1, -w);
      atomicAdd(D + (y1 + 1) * DW + x0, -w);
      atomicAdd(D + (y1 + 1) * DW + x1 + 1, w);
    }
    __syncthreads();
    for (int y = wave; y < DH; y += NW) {  // inclusive prefix along the row, 64 columns per step
      int carry = 0;
      for (int xb = 0; xb < DW; xb += kWave) {
        const int x = xb + lane;
        const int v = wave_scan_i32(x < DW ? D[y * DW + x] : 0) + carry;
        if (x < DW) D[y * DW + x] = v;
        carry = __builtin_amdgcn_readlane(v, kWave - 1);
      }
    }
    __syncthreads();
    int m = 0;
    for (int x = tid; x < DW; x += THREADS) {  // prefix down the columns: only its maximum is kept
      int run = 0;
      for (int y = 0; y < DH; ++y) {
        run += D[y * DW + x];
        m = imaxr(m, run);
      }
    }
    if (m > 0) atomicMax(nlist + 5, m);
    __syncthreads();
    if (tid == 0) dst[1] = iminr(nlist[1], nlist[5]);
    return;
  }
  // ... and the tap entries of the listed RoIs (see roi_align_bwd_packed4): per sample coordinate
  // {neighbours, fraction} with the backward's own expressions, the row neighbours as offsets
  // inside this band (0xffff: outside), 8 bytes each, in list order.  A unit's block of R * 2 * NE words is
  // split in two (BwdFusedArgs::ws_taps): the MAIN table, candidates 0 and 1 of every bin -- all the reference's
  // sample loop makes unless the sample stride is <= 0.01 px -- which the channel workgroups stage into LDS, and
  // the SIDE table, candidate 2, which they read from here only for a bin whose code names it.
  if (a.ws_taps) {
    constexpr int NE = 3 * (PH + PW), TS = kTapMainWords * (PH + PW), SS = kTapSideWords * (PH + PW);
    const float scale = a.L.scale[lvl];
    float* tdst = a.ws_taps + (long)unit * a.R * (2 * NE);
    float* sdst = tdst + (long)a.R * TS;
    for (int i = part * THREADS + tid; i < nl * NE; i += PARTS * THREADS) {
      const int j = i / NE, e = i - j * NE;
      const bool row = e < 3 * PH;
      const int ee = row ? e : e - 3 * PH;
      const float4 bx = *reinterpret_cast<const float4*>(a.rois + ((long)img * a.R + list[j]) * 4);
      // == the forward's coords[roi][e] (coords_block / roi_coords_kernel), bit for bit
      const float v = row ? sample_coord(ee / 3, PH, bx.y, bx.w, scale, H, ee % 3)
                          : sample_coord(ee / 3, PW, bx.x, bx.z, scale, W, ee % 3);
      const int size = row ? H : W;
      const int lo = iminr(imaxr((int)floorf(v), 0), size - 1);
      const int hi = iminr(imaxr((int)ceilf(v), 0), size - 1);
      const float frac = (lo == hi) ? 0.5f : (v - (float)lo);  // (v - low) / (high - low), high - low == 1
      // (byte offsets into the band, so that a bin's LDS address is one add: 4 * col, 4 * (row - row0) * W < 65535)
      unsigned w0 = (unsigned)(4 * lo) | ((unsigned)(4 * hi) << 16);
      if (row) {
        const unsigned o0 = (lo >= row0 && lo < row1) ? (unsigned)(4 * (lo - row0) * W) : 0xffffu;
        const unsigned o1 = (hi >= row0 && hi < row1) ? (unsigned)(4 * (hi - row0) * W) : 0xffffu;
        w0 = o0 | (o1 << 16);
      }
      const int bin = (row ? 0 : PH) + ee / 3, cand = ee % 3;   // axis bin (rows, then columns) and its candidate
      float* dstp = cand < 2 ? tdst + (long)j * TS + 2 * (2 * bin + cand) : sdst + (long)j * SS + 2 * bin;
      *reinterpret_cast<float2*>(dstp) = make_float2(__uint_as_float(w0), frac);
    }
  }
}

}  // namespace sd
