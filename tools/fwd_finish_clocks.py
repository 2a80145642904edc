#!/usr/bin/env python
"""When the persistent workgroups of the band-resident forward finish (profiling build only): per launch and workgroup
the virtual unit it starts on (level, items, workgroups that start there), the reservations and fills it did, its
visits, the tick at the end of its band work and the tick at its exit, at the benchmark's shape; then the per-fill
cost refitted from the visits.  profiles/fwd_finish_clocks.txt is this tool's output.

usage: python tools/fwd_finish_clocks.py [--launches N] [--out FILE] [key=value ...]     (knobs, e.g. roi_align_fwd_staff=1)
"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("SIMPLEDET_AMD_LIB", os.path.join(ROOT, "tools", "libsimpledet_ops_hip_prof.so"))
import numpy as np

NBLK = 256


def one_launch(lib, ops, torch, feats, rois, strides):
    dbg = torch.zeros(NBLK * 16 * 8 + NBLK * 4 * 8, dtype=torch.int64, device="cuda")
    p = dbg.data_ptr()
    lo = p & 0xffffffff
    with lib().tuned(roi_align_dbg_lo=lo - (1 << 32) if lo & 0x80000000 else lo, roi_align_dbg_hi=p >> 32):
        ops.fpn_roi_align_forward_packed(feats, rois, strides, (7, 7))
        torch.cuda.synchronize()
    raw = dbg.cpu().numpy()
    return raw[:NBLK * 16 * 8].reshape(NBLK, 16, 8), raw[NBLK * 16 * 8:].reshape(NBLK, 4, 8)


def table(waves, visits, out):
    """prints one launch; returns (mean finish, max finish, per-visit rows for the fit)"""
    # the tick counters of different XCDs do not share an origin (blocks 8 apart agree, neighbours are up to 2e12
    # apart), so every tick is taken from the workgroup's OWN entry: the 256 workgroups are the whole grid, one per
    # CU, and enter within the launch's ramp of one another
    entry = waves[:, 0, 7] - waves[:, 0, 5]
    exit_ = (waves[:, :, 7] + waves[:, :, 4]).max(1) - entry
    whole = visits[:, 3]
    assert (whole[:, 4] == 2).all(), "the profiling build writes a whole-workgroup record per block"
    band_end = whole[:, 0] - entry
    xcd_ramp = max(int(np.ptp(entry[x::8])) for x in range(8))
    vu0 = whole[:, 3]
    first = visits[:, 0]
    staffed = int(whole[:, 5].max())
    m = np.bincount(vu0[vu0 >= 0], minlength=int(vu0.max()) + 1)
    out.write("staffed by band_staffing: %d;  workgroups that start on each virtual unit: %s\n" % (staffed, m.tolist()))
    out.write("entry ticks inside one XCD (blocks 8 apart) differ by at most %d\n" % xcd_ramp)
    out.write("  wg vu0 lvl items  m  res fills visits  head  band_end    exit   (ticks from the workgroup's entry)\n")
    for b in range(NBLK):
        v = int(vu0[b])
        out.write("%4d %3d %3d %5d %2d %4d %5d %6d %6d %9d %7d\n" % (
            b, v, first[b, 0] if v >= 0 else -1, first[b, 2] if v >= 0 else 0, m[v] if v >= 0 else 0, whole[b, 1], whole[b, 2],
            waves[b, 0, 6], waves[b, 0, 5], band_end[b], exit_[b]))
    out.write("band work ends: mean %.0f max %d;  exit: mean %.0f p90 %.0f max %d;  max / mean exit %.3f\n" % (
        band_end.mean(), band_end.max(), exit_.mean(), np.percentile(exit_, 90), exit_.max(), exit_.max() / exit_.mean()))
    # when each virtual unit was finished (latest end of a recorded visit to it), against its first start
    rec = visits[:, :3].reshape(-1, 8)
    rec = rec[rec[:, 4] == 1]
    own = np.repeat(entry, 3)[(visits[:, :3].reshape(-1, 8)[:, 4] == 1)]
    out.write("virtual unit: level items workgroups-starting  visits  latest end of a visit to it (ticks from that workgroup's entry)\n")
    for v in sorted(set(rec[:, 6].tolist())):
        sel = rec[:, 6] == v
        r = rec[sel]
        out.write("  vu %3d  P%d %4d  m %2d  %3d  %7d\n" % (v, r[0, 0] + 2, r[0, 2], m[v] if v < len(m) else 0, len(r),
                                                         (r[:, 5] - own[sel]).max()))
    return float(exit_.mean()), int(exit_.max()), float(band_end.mean()), int(band_end.max()), rec


def fit(rec, planes, out):
    """visit = S + fills * k * (F0 + G * (F1 + items)) ticks, least squares over the visits of >= 2 fills"""
    r = rec[rec[:, 1] >= 2]
    G = np.asarray([planes[int(l)] for l in r[:, 0]], float)
    f = r[:, 1].astype(float)
    dt = (r[:, 5] - r[:, 3]).astype(float)
    A = np.stack([np.ones(len(r)), f, f * G, f * G * r[:, 2]], 1)
    (S, a, b, k), *_ = np.linalg.lstsq(A, dt, rcond=None)
    res = dt - A @ np.asarray([S, a, b, k])
    out.write("refit over %d visits of >= 2 fills: visit = %.0f + fills * %.2f * (%.0f + G * (%.0f + items)) ticks  "
              "(set-up S = %.0f ticks, k = %.2f ticks per item, F0 = %.0f k, F1 = %.0f k; residual rms %.0f ticks = %.1f %% "
              "of the mean visit)\n" % (len(r), S, k, a / k, b / k, S, k, a / k, b / k, np.sqrt((res ** 2).mean()),
                                        100 * np.sqrt((res ** 2).mean()) / dt.mean()))
    return S, a / k, b / k, k


def main():
    import torch
    from simpledet_amd import ops, synth
    from simpledet_amd._lib import lib
    args = sys.argv[1:]
    launches, path, knobs = 3, None, []
    while args:
        a = args.pop(0)
        if a == "--launches":
            launches = int(args.pop(0))
        elif a == "--out":
            path = args.pop(0)
        else:
            knobs.append(a.split("="))
    for k, v in knobs:
        lib().set_tuning(k, int(v))
    out = open(path, "w") if path else sys.stdout
    feats = [torch.from_numpy(f).cuda() for f in synth.feature_maps(0, 2, 256)]
    rois = torch.from_numpy(synth.random_rois(0, 2, 512)).cuda()
    strides = list(synth.FPN_STRIDES)
    for _ in range(3):
        ops.fpn_roi_align_forward_packed(feats, rois, strides, (7, 7))
    out.write("band-resident forward, benchmark shape (2 x 512 RoIs, 256 channels, 7x7, packed arg-max), knobs: %s\n" % (
        " ".join("%s=%s" % (k, v) for k, v in knobs) or "defaults"))
    out.write("dispatch: %s\n" % (lib().cdll.sd_last_dispatch() or b"").decode())
    sums, recs = [], []
    for i in range(launches):
        waves, visits = one_launch(lib, ops, torch, feats, rois, strides)
        out.write("\n== launch %d\n" % (i + 1))
        mean, mx, bmean, bmax, rec = table(waves, visits, out)
        sums.append((mean, mx, bmean, bmax))
        recs.append(rec)
    s = np.asarray(sums)
    out.write("\n== summary over %d launches\n" % launches)
    for i, (mean, mx, bmean, bmax) in enumerate(sums):
        out.write("launch %d: exit mean %.0f max %d; band work ends mean %.0f max %d\n" % (i + 1, mean, mx, bmean, bmax))
    out.write("exit max: mean over the launches %.0f, launch-to-launch spread (largest - smallest) %d\n" % (
        s[:, 1].mean(), s[:, 1].max() - s[:, 1].min()))
    out.write("exit mean: mean over the launches %.0f, spread %.0f\n" % (s[:, 0].mean(), s[:, 0].max() - s[:, 0].min()))
    fit(np.concatenate(recs), {0: 1, 1: 1, 2: 4, 3: 8}, out)
    if path:
        out.close()


if __name__ == "__main__":
    main()
