#!/usr/bin/env python
"""CPU model (numpy, no GPU) of two costs of the band-resident RoIAlign forward, roi_align_fwd_band, on the
benchmark's inputs: the bytes it writes per launch and the cycles its tap reads keep the LDS busy.

It restates the launcher's band plan (launch_fwd), the pre-pass's item lists (band_prep_block: the items of a unit in
RoI order, a RoI's bin rows adjacent), the kernel's table of virtual units with its cost prefix, and the start unit
of each of the 256 persistent workgroups, for every value of roi_align_fwd_xcd.  What it leaves out: workgroups that
move on when their unit runs dry (a unit's channel grabs are dealt round-robin to the workgroups that START on it),
the RoIs of the exact per-element path, and the tables of the kernel's tail.

  written bytes   64 bytes for every distinct (64-byte line of `out` or of the packed arg-max, XCD) pair over all
                  items and channel grabs: the L2s of the eight XCDs are not coherent, so a line that workgroups on two
                  XCDs write parts of leaves as two partial write-backs.
  LDS cycles      per pass (9 consecutive list items x 7 lanes) and ds_read2_b32: for each of its two dwords and
                  each half of the wave, the largest number of distinct addresses that fall into one of the 32 banks
                  ((byte address / 4) % 32), at least one cycle.  Conflict cycles are what exceeds that minimum.
                  --reads shared models the reads of rows the lane has already read as not issued (lane-masked);
                  --empty-cost says what a half with no active lane costs then (0 or 1).

Against the counters of profiles/r06z_pmc_summary.json (xcd 0, all reads): WRITE_SIZE 83.98 MB, SQ_LDS_IDX_ACTIVE
17.90 M, SQ_LDS_BANK_CONFLICT 11.03 M; tests/test_fwd_traffic_model.py holds the model within 10 % of each.
What the model PREDICTED and what was then measured (profiles/fwd_xcd_rowshare_ab.txt):
  LDS cycles with --reads shared   12.6 .. 13.9 M; measured 13.45 M (and 7.57 M conflict cycles against 6.0 .. 7.4 M): right
  written bytes with --xcd 1       68 MB; measured WRITE_SIZE 84.5 MB, unchanged from xcd 0: WRONG.  Matching the 84 MB of
                                   xcd 0 does not make partial write-backs of lines shared across XCDs the mechanism behind
                                   them; treat the written-bytes half as a count of shared lines, not as a traffic forecast.

    python tools/fwd_traffic_model.py [--xcd 0|1|2] [--reads all|shared] [--empty-cost 0|1]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

f32 = np.float32
WAVE, BAND_WAVES, BAND_NP, BUF_FLOATS, HALO, MAX_BANDS = 64, 16, 4, 16896, 8, 16
FILL_COST, PLANE_COST, SETUP_COST = 140, 60, 1500
NWG, NXCD, GRAB, LINE, BANKS = 256, 8, 4, 64, 32


def band_plan(shapes, C, R, P):
    """launch_fwd's plan for the packed fp32 form: per level (bands, rows a band owns, planes per fill)"""
    out = []
    for H, W in shapes:
        halo = HALO
        if H <= 128:
            halo = max(HALO, min((H + P - 1) // P + 2, 12))
        rb = (BUF_FLOATS - 16) // W
        nbn = 1 if H <= rb else -(-H // (rb - halo))
        cap = BAND_NP * BAND_WAVES * (WAVE // P)
        by_items = (R * P // len(shapes) * 5 + 4 * cap - 1) // (4 * cap)
        nbn = min(max(nbn, by_items), H, MAX_BANDS)
        owned = -(-H // nbn)
        if nbn > 1:
            for o in range(owned, owned + 4):
                if o + halo > rb:
                    break
                if (o * W) % 4 == 0:
                    owned = o
                    break
        owned = min(owned, rb - halo)
        nbn = -(-H // owned)
        rows = H if nbn == 1 else min(owned + halo, H)
        bstride = (rows * W + 4 + 3) & ~3
        g = 1
        for c in (2, 4, 8):
            if C % c == 0 and c * bstride <= BUF_FLOATS:
                g = c
        out.append(dict(nbands=nbn, owned=H if nbn == 1 else owned, g=g, halo=halo))
    return out


def fpn_level(rois, strides, canon_scale=224.0, canon_level=4.0):
    """assign_layer_fpn in float32 -> index into strides"""
    w, h = rois[..., 2] - rois[..., 0] + f32(1), rois[..., 3] - rois[..., 1] + f32(1)
    with np.errstate(all="ignore"):
        t = np.floor(f32(canon_level) + np.log2(np.sqrt(w * h) / f32(canon_scale) + f32(1e-6)))
    t = np.clip(t, np.log2(min(strides)), np.log2(max(strides)))
    return np.searchsorted(np.asarray(strides), np.exp2(np.nan_to_num(t, nan=2.0)).astype(np.int64))


def axis_samples(start, end, scale, size, P):
    """the reference's sample loop along one axis for all RoIs and bins -> count (-1 empty bin), low and high
    neighbour of samples 0 and 1 (float32 expressions of axis_samples in roi_align_common.h)"""
    a, e = (start * f32(scale))[:, None], (end * f32(scale))[:, None]
    b = (e - a) / f32(P)
    p = np.arange(P, dtype=f32)[None]
    lo = np.clip(p * b + a, f32(0), f32(size - 1))
    hi = np.clip((p + f32(1)) * b + a, f32(0), f32(size - 1))
    st = (hi - lo) / f32(3)
    lim = (hi - st).astype(np.float64) + 0.01
    step = np.maximum(st, f32(0.01))
    v0 = lo + st
    v1 = v0 + step
    v2 = v1 + step
    cnt = (v0 <= lim).astype(int) + ((v0 <= lim) & (v1 <= lim)) + ((v0 <= lim) & (v1 <= lim) & (v2 <= lim))
    cnt = np.where(hi <= lo, -1, cnt)
    nb = lambda v: (np.clip(np.floor(v), 0, size - 1).astype(int), np.clip(np.ceil(v), 0, size - 1).astype(int))
    return cnt, nb(v0), nb(v1)


def unit_order(nunits_per_level, xcd):
    """units in table order: level-major, or (xcd = 2) by the key (j + 1/2) / n_l, ties by level then j"""
    units = [(l, j) for l, n in enumerate(nunits_per_level) for j in range(n)]
    if xcd >= 2:
        units.sort(key=lambda u: ((2 * u[1] + 1) * np.prod([n for k, n in enumerate(nunits_per_level) if k != u[0] and n]),
                                  u[0], u[1]))
    return units


def xcd_slot(wg, nwg):
    return (wg % NXCD) * (nwg // NXCD) + wg // NXCD if nwg % NXCD == 0 else wg


def virtual_units(rois, shapes, strides, C, P=7, xcd=0):
    """the kernel's table of virtual units in table order: per entry the unit's lists (`unit`, with its planes per
    fill `g` and its `level`), the first item and the items of the round, and the cost the prefix is built from;
    also the number of units"""
    B, R = rois.shape[:2]
    plan = band_plan(shapes, C, R, P)
    level = fpn_level(rois, strides)
    cap = BAND_NP * BAND_WAVES * (WAVE // P)
    ipp = WAVE // P
    # ---- per level the item lists of every (image, band) unit, in RoI order
    per_unit = {}
    for l, ((H, W), pl) in enumerate(zip(shapes, plan)):
        for img in range(B):
            idx = np.nonzero(level[img] == l)[0]
            bx = rois[img, idx]
            cr, r0s, r1s = axis_samples(bx[:, 1], bx[:, 3], 1.0 / strides[l], H, P)
            cc, c0s, c1s = axis_samples(bx[:, 0], bx[:, 2], 1.0 / strides[l], W, P)
            last = np.where(cr >= 2, r1s[1], r0s[1])
            bad = ((cr >= 3).any(1) | (cc >= 3).any(1) | ((pl["nbands"] > 1) & (last - r0s[0] > pl["halo"]) & (cr >= 1)).any(1)
                   | (cr < 0).all(1) | (cc < 0).all(1))
            band = np.where(cr >= 1, r0s[0] // pl["owned"], 0)
            for b in range(pl["nbands"]):
                sel = (band == b) & ~bad[:, None]
                ri, pi = np.nonzero(sel)
                r0w = b * pl["owned"] * W
                lo0 = np.where(cr[ri, pi] >= 1, np.maximum(r0s[0][ri, pi] * W - r0w, 0), 0)
                hi0 = lo0 + np.where((cr[ri, pi] >= 1) & (r0s[1][ri, pi] != r0s[0][ri, pi]), W, 0)
                lo1 = np.where(cr[ri, pi] >= 2, np.maximum(r1s[0][ri, pi] * W - r0w, 0), 0)
                hi1 = lo1 + np.where((cr[ri, pi] >= 2) & (r1s[1][ri, pi] != r1s[0][ri, pi]), W, 0)
                left0 = np.where(cc[ri] >= 1, c0s[0][ri], 0)     # (items, P) columns of the RoI's bins
                left1 = np.where(cc[ri] >= 2, c1s[0][ri], 0)
                per_unit[(l, img * pl["nbands"] + b)] = dict(
                    n=img * R + idx[ri], p=pi, rows=np.stack([lo0, hi0, lo1, hi1], 1), left0=left0, left1=left1, g=pl["g"],
                    level=l)
    # ---- virtual units, cost prefix, start unit of every workgroup
    nper = [B * pl["nbands"] for pl in plan]
    vus = []
    for (l, j) in unit_order(nper, xcd):
        u = per_unit[(l, j)]
        cnt = len(u["n"])
        for r in range(-(-cnt // cap)):
            it = min(cap, cnt - r * cap)
            vus.append(dict(unit=u, first=r * cap, items=it, cost=SETUP_COST + (FILL_COST // u["g"] + PLANE_COST + it) * C))
    return vus, len(per_unit)


def model(rois, shapes, strides, C, P=7, xcd=0, reads="all", empty_cost=1):
    vus, nunits = virtual_units(rois, shapes, strides, C, P, xcd)
    ipp = WAVE // P
    start = np.concatenate([[0], np.cumsum([v["cost"] for v in vus])])
    wgs = [[] for _ in vus]
    for wg in range(NWG):
        share = xcd_slot(wg, NWG) if xcd >= 1 else wg
        pos = int(start[-1]) * (2 * share + 1) // (2 * NWG)
        wgs[max(int((start[:-1] <= pos).sum()) - 1, 0)].append(wg)
    for v in range(len(vus)):       # (a unit nobody starts on is taken by a workgroup that has run dry: the nearest)
        if not wgs[v]:
            near = min((w for w in range(len(vus)) if wgs[w]), key=lambda w: abs(w - v))
            wgs[v] = [wgs[near][-1 if near < v else 0]]
    # ---- written bytes and LDS cycles
    keys = []
    lds_active = 0
    lds_min = 0
    for v, mine in zip(vus, wgs):
        u = v["unit"]
        sl = slice(v["first"], v["first"] + v["items"])
        n, p = u["n"][sl], u["p"][sl]
        gr = -(-GRAB // u["g"]) * u["g"]
        chan = np.arange(C)
        x = np.asarray(mine)[(chan // gr) % len(mine)] % NXCD
        row = (n[:, None] * C + chan[None]).astype(np.int64)
        for base, first, length in ((0, (row * P * P + p[:, None] * P) * 4, 4 * P),
                                    (1, row * ((P * P + 3) & ~3) + p[:, None] * P, P)):
            for line in (first // LINE, (first + length - 1) // LINE):
                keys.append(((line * 2 + base) * NXCD + x[None]).ravel())
        # passes: 9 consecutive items x 7 lanes; idle lanes read address 0
        npass = -(-v["items"] // ipp)
        pad = npass * ipp - v["items"]
        rows = np.concatenate([u["rows"][sl], np.zeros((pad, 4), int)])
        l0 = np.concatenate([u["left0"][sl], np.zeros((pad, P), int)])
        l1 = np.concatenate([u["left1"][sl], np.zeros((pad, P), int)])
        # addr[pass, instr, lane]: instr = 2 * row + (left0 | left1)
        addr = np.zeros((npass, 8, WAVE), np.int64)
        active = np.zeros((npass, 8, WAVE), bool)
        for r in range(4):
            for k, lf in enumerate((l0, l1)):
                a = (rows[:, r][:, None] + lf).reshape(npass, ipp * P)
                addr[:, 2 * r + k, :ipp * P] = a
                active[:, 2 * r + k, :ipp * P] = True
        if reads == "shared":
            for r in (2, 3):
                for k in (0, 1):
                    dup = (addr[:, 2 * r + k] == addr[:, k]) | (addr[:, 2 * r + k] == addr[:, 2 + k])
                    active[:, 2 * r + k] &= ~dup
        cyc = 0
        for d in (0, 1):
            a = (addr + d).reshape(-1, 2, WAVE // 2)
            act = active.reshape(-1, 2, WAVE // 2)
            a = np.where(act, a, -1)
            a = np.sort(a, -1)
            new = np.concatenate([np.ones(a.shape[:2] + (1,), bool), a[..., 1:] != a[..., :-1]], -1) & (a >= 0)
            counts = np.zeros(a.shape[:2] + (BANKS,), int)
            i0, i1, _ = np.nonzero(new)
            np.add.at(counts, (i0, i1, (a[new] % BANKS)), 1)
            worst = counts.max(-1)
            cyc += np.where(act.any(-1), worst, empty_cost).sum()
        lds_active += int(cyc) * C
        lds_min += npass * 8 * 4 * C
    written = LINE * len(np.unique(np.concatenate(keys)))
    items = sum(v["items"] for v in vus)
    return dict(written_bytes=written, lds_active=lds_active, lds_conflict=lds_active - lds_min, items=items,
                units=nunits, virtual_units=len(vus), output_bytes=items * C * (4 * P + P),
                lds_per_item_channel=lds_active / float(items * C))


def benchmark_inputs(seed=0, images=2, rois=512):
    from simpledet_amd import synth
    return synth.random_rois(seed, images, rois), list(synth.FPN_SHAPES), list(synth.FPN_STRIDES)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--xcd", type=int, default=0, choices=(0, 1, 2))
    ap.add_argument("--reads", default="all", choices=("all", "shared"))
    ap.add_argument("--empty-cost", type=int, default=1, choices=(0, 1))
    ap.add_argument("--channels", type=int, default=256)
    a = ap.parse_args()
    rois, shapes, strides = benchmark_inputs()
    m = model(rois, shapes, strides, a.channels, xcd=a.xcd, reads=a.reads, empty_cost=a.empty_cost)
    print("roi_align_fwd_xcd = %d, reads = %s: %d units, %d virtual units, %d items" %
          (a.xcd, a.reads, m["units"], m["virtual_units"], m["items"]))
    print("  written bytes per launch  %.1f MB (the outputs of these items: %.1f MB)" %
          (m["written_bytes"] / 1e6, m["output_bytes"] / 1e6))
    print("  LDS-active cycles         %.2f M (%.2f per item and channel)" % (m["lds_active"] / 1e6, m["lds_per_item_channel"]))
    print("  LDS conflict cycles       %.2f M (%.0f %%)" % (m["lds_conflict"] / 1e6, 100.0 * m["lds_conflict"] / m["lds_active"]))


if __name__ == "__main__":
    main()
