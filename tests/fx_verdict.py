"""numpy statements of what the fixed-point backwards decide per workgroup, shared by test modules (not a conftest).

band_units: the RoI list and the weight bound of every (level, image, band) unit of the fused FPN backward, as
    `bwd_band_list` and the list pre-pass (`bwd_lists_block`, 4 x 4 pixel cells) build them.
packed4_verdict / flt4_verdict / col2im_verdict: the dynamic-range verdict (`fx_range_*`, csrc/common.h) of one
    workgroup of roi_align_bwd_packed4 / roi_align_bwd_flt4_kernel / deform_col2im_chunk_kernel, in two forms:
      "intended": what the design asks -- the sampling `fx_range_stride_mask` plans, sums in int64;
      "head":     what the kernels computed until the verdict was made wrap-free -- packed4 sampled every trip
                  of every chunk (its trip index restarted per chunk), and the sum travelled as ONE int32,
                  (sum of margins << 12) + sample count, so the count wrapped into the margins past 4095 samples
                  and the int32 wrapped when the margins were large (a first trip of zeros: e_thr ~ -11).
    A GPU case is only evidence of the wrap when its numpy verdicts differ; the CPU tests assert that they do.
"""
import numpy as np

f32 = np.float32
FX_RANGE_BITS = 16
THREADS = 512


# ------------------------------------------------------------------------------------------------ plan
def band_plan(shapes, taps=True):
    """launch_bwd_fused's band plan: 27 KB bands with tap tables (lists + taps), 36 KB without -> (nbands,
    band rows, launch order) per level."""
    budget = (27 if taps else 36) * 1024
    nbands, rows = [], []
    for (H, W) in shapes:
        nb = max(1, -(-(H * W * 4) // budget))
        r = -(-H // nb)
        nbands.append(-(-H // r))
        rows.append(r)
    order = sorted(range(len(shapes)), key=lambda l: (nbands[l], -shapes[l][0] * shapes[l][1]))
    return nbands, rows, order


def _nbins(bw, P):
    if not bw > 0:
        return P
    fx = f32(f32(2.00002) * f32(f32(1) / bw))
    return min(int(fx) + 2, P) if fx < P else P


def band_units(rois, level, shapes, strides, pooled=7, taps=True):
    """-> list of dicts in unit order (level in launch order, image, band): lvl, img, band, list (ascending RoI
    indices), total (the band-summed bound of bwd_band_list), pixel (the 4 x 4 cell bound of the pre-pass:
    min(total, max over cells)).  The device's pixel bound takes 1 / bin width from v_rcp_f32 (1 ulp) and may
    exceed this one by up to one bin row / column of one RoI."""
    B = rois.shape[0]
    R = rois.shape[1]
    nbands, rows, order = band_plan(shapes, taps)
    units = []
    for l in order:
        H, W = shapes[l]
        scale = f32(1.0 / strides[l])
        for img in range(B):
            for band in range(nbands[l]):
                row0, row1 = band * rows[l], min(band * rows[l] + rows[l], H)
                DW, DH = ((W - 1) >> 2) + 2, ((row1 - row0 - 1) >> 2) + 2
                D = np.zeros((DH + 1, DW + 1), np.int64)
                total, lst = 0, []
                for r in range(R):
                    if level[img, r] != l:
                        continue
                    x1, y1, x2, y2 = rois[img, r]
                    clip = lambda v, hi: min(max(f32(v) * scale, f32(0)), f32(hi))
                    ys, ye = clip(y1, H - 1), clip(y2, H - 1)
                    ylo, yhi = f32(min(ys, ye) - f32(2)), f32(max(ys, ye) + f32(2))
                    if nbands[l] > 1 and (yhi < row0 or ylo > row1 - 1):
                        continue
                    lst.append(r)
                    xs, xe = clip(x1, W - 1), clip(x2, W - 1)
                    xlo, xhi = f32(min(xs, xe) - f32(2)), f32(max(xs, xe) + f32(2))
                    bwx = f32(f32(f32(x2 - x1) * scale) * f32(1.0 / pooled))
                    bwy = f32(f32(f32(y2 - y1) * scale) * f32(1.0 / pooled))
                    w = _nbins(bwx, pooled) * _nbins(bwy, pooled)
                    total += w
                    X0, X1 = max(int(np.floor(xlo)), 0), min(int(np.ceil(xhi)), W - 1)
                    Y0, Y1 = max(int(np.floor(ylo)), 0), min(int(np.ceil(yhi)), H - 1)
                    Y0, Y1 = max(Y0, row0) - row0, min(Y1, row1 - 1) - row0
                    if Y0 > Y1:
                        continue
                    D[Y0 >> 2:(Y1 >> 2) + 1, X0 >> 2:(X1 >> 2) + 1] += w
                units.append(dict(lvl=l, img=img, band=band, list=lst, total=total, pixel=min(total, int(D.max()))))
    return units


# ------------------------------------------------------------------------------------------------ verdict
def exponent_field(v):
    return ((np.abs(np.asarray(v, np.float32)).view(np.uint32) >> 23) & 255).astype(np.int64)


def ceil_log2(b):
    return 0 if b <= 1 else int(b - 1).bit_length()


def fx_range_thr(gmax_used, bound):
    return int(exponent_field(gmax_used)) + 1 + ceil_log2(bound) - FX_RANGE_BITS


def stride_mask(per_trip, trips, at_least=0):
    m = at_least
    while per_trip * ((trips + m) // (m + 1)) > 4000:
        m = 2 * m + 1
    return m


def _wrap32(v):
    return int((int(v) + 2 ** 31) % 2 ** 32 - 2 ** 31)


def verdict(samples, e_thr, gmax_used, gmax_true, wrap):
    """fx_range_fine over the samples: True = the fixed-point unit is fine enough.  wrap=True restates the one
    packed int32 ((margins << 12) + count per sample, summed modulo 2^32); wrap=False the exact int64 sums."""
    ex = exponent_field(samples)
    ex = ex[ex > 0]
    margins, cnt = int((ex - e_thr).sum()), int(ex.size)
    if wrap:
        packed = _wrap32(margins * 4096 + cnt)
        cnt, margins = packed & 4095, packed >> 12
    extra = int(exponent_field(gmax_true)) - (int(exponent_field(gmax_used)) + 1)
    return margins - (extra * cnt if extra > 0 else 0) >= 0


def _result(head_samples, samples, e_thr, gu, gt):
    return dict(intended=verdict(samples, e_thr, gu, gt, False), head=verdict(head_samples, e_thr, gu, gt, True),
                head_exact=verdict(head_samples, e_thr, gu, gt, False), n_head=int((exponent_field(head_samples) > 0).sum()),
                n=int((exponent_field(samples) > 0).sum()), e_thr=e_thr, gmax_used=float(gu), gmax_true=float(gt))


def packed4_verdict(g, bound, flt=False):
    """One workgroup of roi_align_bwd_packed4: g (nl, PP) = dY of the listed RoIs (list order) of one channel, as
    fp32 (fp16 I/O: the converted values).  Items are 16-byte lanes of a RoI row: item (j, k) holds bins
    4k .. min(4k + 3, PP - 1) (tail4 keeps the row's last PP % 4 bins), its sample is bin 4k.  The workgroup
    streams chunks of TCH RoIs (32 at 7x7, 16 at 14x14; MODE 2 has no tables: one chunk), one trip = 512 items;
    gmax_used = max |dY| of the first trip of the first chunk."""
    g = np.asarray(g, np.float32)
    nl, PP = g.shape
    GP = -(-PP // 4)
    tch = max(nl, 1) if flt else (32 if PP == 49 else 16)
    pad = np.zeros((nl, 4 * GP), np.float32)
    pad[:, :PP] = g
    item_max = np.abs(pad).reshape(nl, GP, 4).max(2)
    item_x = pad.reshape(nl, GP, 4)[:, :, 0]
    chunks = [(cb, min(tch, nl - cb)) for cb in range(0, nl, tch)]
    gu = f32(item_max[:chunks[0][1]].ravel()[:THREADS].max()) if nl else f32(0)
    gt = f32(item_max.max()) if nl else f32(0)
    e_thr = fx_range_thr(gu, bound)
    head_mask = stride_mask(THREADS, -(-nl * GP // THREADS), 3)
    trips = sum(-(-n * GP // THREADS) for _, n in chunks)
    mask = stride_mask(THREADS, trips, 3)
    head, want, trip = [], [], 0
    for cb, n in chunks:
        x = item_x[cb:cb + n].ravel()
        for t0 in range(0, x.size, THREADS):
            if ((t0 // THREADS) & head_mask) == 0:
                head.append(x[t0:t0 + THREADS])
            if (trip & mask) == 0:
                want.append(x[t0:t0 + THREADS])
            trip += 1
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.float32)
    return _result(cat(head), cat(want), e_thr, gu, gt)


def flt4_bound(rois_img, H, W, scale, pooled=7):
    """the per-pixel weight bound of roi_align_bwd_flt4_kernel (difference array of nx * ny over each RoI's
    clipped box +-2) for one image."""
    D = np.zeros((H + 1, W + 1), np.int64)
    for x1, y1, x2, y2 in np.asarray(rois_img, np.float32):
        sc = f32(scale)
        xs, xe = [min(max(f32(v) * sc, f32(0)), f32(W - 1)) for v in (x1, x2)]
        ys, ye = [min(max(f32(v) * sc, f32(0)), f32(H - 1)) for v in (y1, y2)]
        xlo, xhi = f32(min(xs, xe) - f32(2)), f32(max(xs, xe) + f32(2))
        ylo, yhi = f32(min(ys, ye) - f32(2)), f32(max(ys, ye) + f32(2))
        X0, X1 = max(int(np.floor(xlo)), 0), min(int(np.ceil(xhi)), W - 1)
        Y0, Y1 = max(int(np.floor(ylo)), 0), min(int(np.ceil(yhi)), H - 1)
        bwx = f32(f32(f32(x2 - x1) * sc) * f32(1.0 / pooled))
        bwy = f32(f32(f32(y2 - y1) * sc) * f32(1.0 / pooled))
        D[Y0:Y1 + 1, X0:X1 + 1] += _nbins(bwx, pooled) * _nbins(bwy, pooled)
    return int(D.max())


def flt4_verdict(dy_img, c, bound):
    """One workgroup of roi_align_bwd_flt4_kernel: dy_img (R, C, PP) of one image, channels c .. c+3.  Unit u of
    the workgroup = 16 bytes of the RoI row of the four channels; sample = its first value; gmax_used = max |dY|
    of the first 512 units; sampled trips (u / 512) & mask == 0."""
    x = np.ascontiguousarray(np.asarray(dy_img, np.float32)[:, c:c + 4]).reshape(-1, 4)
    n = x.shape[0]
    gu = f32(np.abs(x[:THREADS]).max())
    gt = f32(np.abs(x).max())
    e_thr = fx_range_thr(gu, bound)
    mask = stride_mask(THREADS, -(-n // THREADS), 7)
    trips = np.arange(n) // THREADS
    s = x[(trips & mask) == 0, 0]
    return _result(s, s, e_thr, gu, gt)


def col2im_verdict(col_tap0, cb, gmax_true=None, T=512):
    """One workgroup of deform_col2im_chunk_kernel<4, T, true>: col_tap0 (4, P) = the workgroup's four channels of
    tap 0; cb = ceil(log2(ceil(weight sum))) of its (image, group).  gmax_used = max |col| of the first trip
    (pixels < 4 T of tap 0), samples = channel 0 at pixels 0, 4, 8, .. < 16000; e_thr two more than
    fx_range_thr (the unit is 2^-28 of the bound).  gmax_true: max |col| over all taps of the four channels
    (default: tap 0's)."""
    v = np.asarray(col_tap0, np.float32)
    gu = f32(np.abs(v[:, :4 * T]).max())
    gt = f32(np.abs(v).max() if gmax_true is None else gmax_true)
    e_thr = int(exponent_field(gu)) + 1 + cb - FX_RANGE_BITS + 2
    s = v[0, 0:min(v.shape[1], 16000):4]
    return _result(s, s, e_thr, gu, gt)
