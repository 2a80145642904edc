#!/usr/bin/env python
"""TSD RoI extraction timing (simpledet_amd/csrc/deform_psroi.hip) at the shape of config/TSD/tsd_r50_rpn_1x.py:
B = 2, R = 512 RoIs per image, C = 256, 800 x 1333 (levels 200x334 .. 25x42, strides 4-32), 7 x 7 bins of 4 x 4
samples, trans_std 0.1; offsets ~ N(0, 1) and zeros.

Timed from device events, eagerly and as one captured HIP graph, forward, backward and both, for the DeltaC
extractor (offsets (B*R, 2, 7, 7)), the DeltaR extractor (offsets (B*R, 2)) and the two of a step together.  In the
same run, on the same tensors: the reference's composition built from the device's OWN single-level operator --
level rule, the eight masked copies of rois and offsets (where), the batch column (concat), the tile of DeltaR,
four sd_deform_psroi_pool calls, add_n; its backward: four operator backwards, the masks' where on d_trans, the
sum over the tile, the sum of the four d_trans.  Nothing at the parent commit runs this path, so the composition
is the baseline.

For the backward the file reports
  - composition_ratio: composition / fused;
  - algorithmic bytes / time: dY read once + d_trans written + every level's d_data zero-filled and the touched
    pixels updated (taken as one read-modify-write of every level: an upper bound on what has to move);
  - atomic bytes / time: global float atomics x 4 bytes against the ~1.3 TB/s chip-wide atomic rate of the
    programming guide.  The count is MODELLED on the host, not measured: from the restatement's tap tables of every
    eighth RoI, one atomic per touched pixel of a (RoI, channel) patch -- or one per tap where the patch's bounding
    box exceeds the 2048 floats a wave holds, as the kernel decides --, scaled by eight; next to it what one atomic
    per tap would issue everywhere;
  - fused_bwd_d_data_only / fused_bwd_d_trans_only: the backward with the other output's req null (the feature
    gradients with their scatter, or the offset gradients with their gathers, alone);
  - direct_bwd: the same backward with sd_set_tuning("deform_psroi_bwd_patch", 0), i.e. every tap added to memory
    with its own global atomic and no LDS patch -- the alternative the patch path has to beat.
The forward rotates two input sets; the backward and forward + backward are timed on ONE set (the backward reads the
state its own forward left).
Also stored: k_ref / k_gpu of tests/test_deform_psroi.py's margin on its fixtures.

    python tools/tsd_pool_time.py [--iters 30] [--out profiles/tsd_pool_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops, synth  # noqa: E402
from simpledet_amd._lib import lib  # noqa: E402
from tests import deform_psroi_ref as dr  # noqa: E402

PEAK, ATOMIC_RATE = 8.0e12, 1.3e12
B, R, C, P, S, STD = 2, 512, 256, 7, 4, 0.1
STRIDES = synth.FPN_STRIDES
NSETS = 2


def time_events(fn, iters, nsets=NSETS):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(3):
        fn(i % nsets)
    torch.cuda.synchronize()
    ts = []
    for i in range(iters):
        start.record()
        fn(i % nsets)
        end.record()
        end.synchronize()
        ts.append(start.elapsed_time(end) * 1e3)
    return float(np.median(ts))


def graphs_of(fn, nsets=NSETS):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    out = []
    for i in range(nsets):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn(i)
        out.append(g)
    return out


def both_ways(fn, iters):
    e = time_events(fn, iters)
    gs = graphs_of(fn)
    g = time_events(lambda i: gs[i].replay(), iters)
    del gs
    return dict(eager_us=round(e, 1), graph_us=round(g, 1))


class Composition:
    """get_roi_feature of models/TSD/poolings.py with the device's single-level operator in the four calls"""

    def __init__(self, feats, rois, trans):
        self.feats, self.rois, self.trans = feats, rois, trans
        self.per_roi = trans.dim() == 2
        n = B * R
        self.batch_pad = torch.arange(B, device="cuda", dtype=torch.float32).repeat_interleave(R).view(-1, 1)
        self.kw = [dict(spatial_scale=1.0 / s, output_dim=C, group_size=1, pooled_size=P, part_size=0,
                        sample_per_part=S, trans_std=STD, no_trans=False) for s in STRIDES]
        self.k_min, self.k_max = float(np.log2(min(STRIDES))), float(np.log2(max(STRIDES)))
        self.state = None
        self.n = n

    def masks(self):
        x1, y1, x2, y2 = self.rois.unbind(-1)
        scale = torch.sqrt((x2 - x1 + 1) * (y2 - y1 + 1))
        lv = torch.clip(torch.floor(4 + torch.log2(scale / 224 + 1e-6)), self.k_min, self.k_max)
        return torch.pow(2, lv).to(torch.uint8)

    def forward(self):
        target = self.masks()
        tr = self.trans.view(B, R, -1)
        out, state = None, []
        for l, s in enumerate(STRIDES):
            own = (target == s).unsqueeze(-1)
            lr = torch.where(own, self.rois, torch.full_like(self.rois, -1.0)).view(-1, 4)
            lo = torch.where(own, tr, torch.zeros_like(tr))
            lo = lo.view(-1, 2, 1, 1).repeat(1, 1, P, P) if self.per_roi else lo.view(-1, 2, P, P)
            lr = torch.cat([self.batch_pad, lr], 1)
            o, tc = ops.deform_psroi_pool_forward(self.feats[l], lr, lo.contiguous(), **self.kw[l])
            out = o if out is None else out + o
            state.append((lr, lo, tc, own))
        self.state = state
        return out

    def backward(self, dy):
        d_feats, d_trans = [], None
        for l, (lr, lo, tc, own) in enumerate(self.state):
            dd, _, dl = ops.deform_psroi_pool_backward(dy, self.feats[l], lr, lo, tc, req_rois="null", **self.kw[l])
            d_feats.append(dd)
            if self.per_roi:
                dl = dl.sum((2, 3))
            dl = torch.where(own, dl.view(B, R, -1), torch.zeros((), device="cuda")).view(self.trans.shape)
            d_trans = dl if d_trans is None else d_trans + dl
        return d_feats, d_trans


PATCH_CAP = 2048    # floats of LDS patch per wave at 7 x 7 x 16 (kDpPatchMax of csrc/deform_psroi.hip)


def atomic_counts(rois, trans, form, step=8):
    """A MODEL of the global float atomics of one backward, per channel: touched pixels of every (RoI, level) patch,
    or the taps where the patch's bounding box exceeds PATCH_CAP -- and the taps everywhere, i.e. what one atomic per
    tap would issue (float64 restatement of the tap tables, own level + masked levels).  Counted on every `step`-th
    RoI and scaled.  -> (modelled atomics, taps, RoIs whose patch does not fit)"""
    target = dr.assign_levels(rois, STRIDES, 224, 4, np.float32).reshape(-1)
    r4, pixels, taps, misses = rois.reshape(-1, 4), 0, 0, 0
    tr = trans.reshape(B * R, 2, -1)
    shapes = synth.FPN_SHAPES
    quirk = [dr.quirk_bins(h, w, s, P, S)[0] for (h, w), s in zip(shapes, STRIDES)]
    for n in range(0, B * R, step):
        for l, s in enumerate(STRIDES):
            if target[n] != s:
                pixels += 1 if quirk[l] else 0
                taps += 4 * S * S * len(quirk[l])     # (an upper bound: every sample of a kept bin)
                continue
            prm = dr.params(1.0 / s, 1, 1, P, 0, S, STD, False)
            seen, own_taps = set(), 0
            for ph in range(P):
                for pw in range(P):
                    t = tr[n, :, 0] if form == "R" else tr[n, :, ph * P + pw]
                    tp, _, _ = dr.unit_taps(r4[n], t, shapes[l][0], shapes[l][1], ph, pw, prm, P, np.float64)
                    own_taps += 4 * len(tp)
                    for y0, yb, x0, xb, dx, dy in tp:
                        seen |= {(y0, x0), (yb, x0), (y0, xb), (yb, xb)}
            taps += own_taps
            area = 0
            if seen:
                ys, xs = [p_[0] for p_ in seen], [p_[1] for p_ in seen]
                area = (max(ys) - min(ys) + 1) * (max(xs) - min(xs) + 1)
            if area > PATCH_CAP:
                misses += 1
                pixels += own_taps
            else:
                pixels += len(seen)
    return pixels * step, taps * step, misses * step


def k_margin():
    """the worst k of the GPU over the fixtures of tests/test_deform_psroi.py, and the restatement's k there"""
    from tests import test_deform_psroi as T
    cu = lambda a: torch.from_numpy(np.array(a, np.float32)).cuda()
    worst = {}

    def note(key, name, got, truth, tt, ref):
        k, kr = dr.k_of(got.cpu().numpy(), truth, tt), dr.k_of(ref, truth, tt)
        w = worst.setdefault(key, dict(k_gpu=-1.0))
        if k - (2 * kr + 2) > w["k_gpu"] - (2 * w.get("k_ref_there", 0.0) + 2) or w["k_gpu"] < 0:
            w.update(k_gpu=round(k, 3), k_ref_there=round(kr, 3), case=name)
    for name in T.SINGLE:
        c = T._single(name)
        kw = T._single_kw(c)
        trans = None if c["no_trans"] else cu(c["trans"])
        out, cnt = ops.deform_psroi_pool_forward(cu(c["data"]), cu(c["rois"]), trans, **kw)
        note("out", name, out, c["truth"][0], c["truth"][2], c["ref"][0])
        dd, _, dt = ops.deform_psroi_pool_backward(cu(c["dy"]), cu(c["data"]), cu(c["rois"]), trans, cnt, **kw)
        note("d_data", name, dd, c["btruth"][0], c["btruth"][2], c["bref"][0])
        if dt is not None:
            note("d_trans", name, dt, c["btruth"][1], c["btruth"][3], c["bref"][1])
    for form in "CR":
        c = T._fused(form)
        feats = [cu(f) for f in c["feats"]]
        out, cnt = ops.fpn_deform_roi_pool_forward(feats, cu(c["rois"]), cu(c["trans"]), T.FSTRIDES, c["P"],
                                                   roi_canonical_scale=16)
        note("fused_out", form, out, c["truth"][0], c["truth"][2], c["ref"][0])
        dfs, dt = ops.fpn_deform_roi_pool_backward(cu(c["dy"]), feats, cu(c["rois"]), cu(c["trans"]), cnt, T.FSTRIDES,
                                                   c["P"], roi_canonical_scale=16)
        for l, d in enumerate(dfs):
            note("fused_d_feat", "%s level %d" % (form, l), d, c["btruth"][0][l], c["btruth"][2][l], c["bref"][0][l])
        note("fused_d_trans", form, dt, c["btruth"][1], c["btruth"][3], c["bref"][1])
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsd_pool_time.json"))
    ap.add_argument("--no-margin", action="store_true")
    args = ap.parse_args()
    gen = torch.Generator(device="cuda").manual_seed(1)
    feats = [[torch.from_numpy(f).cuda() for f in synth.feature_maps(i, batch=B, channels=C)] for i in range(NSETS)]
    rois_np = [synth.random_rois(i, B, R) for i in range(NSETS)]
    rois = [torch.from_numpy(r).cuda() for r in rois_np]
    dys = [torch.randn((B * R, C, P, P), device="cuda", generator=gen) for _ in range(NSETS)]
    res = {}
    feat_bytes = sum(4 * B * C * h * w for h, w in synth.FPN_SHAPES)
    for dist in ("normal", "zeros"):
        mk = (lambda shape: torch.randn(shape, device="cuda", generator=gen)) if dist == "normal" else \
            (lambda shape: torch.zeros(shape, device="cuda"))
        tc_ = [mk((B * R, 2, P, P)) for _ in range(NSETS)]
        tr_ = [mk((B * R, 2)) for _ in range(NSETS)]
        out = {f: torch.empty((B * R, C, P, P), device="cuda") for f in "CR"}
        cnt = {f: torch.empty((B * R, len(STRIDES), P, P), device="cuda") for f in "CR"}
        d_feats = {f: [torch.empty_like(x) for x in feats[0]] for f in "CR"}
        d_tr = {"C": torch.empty_like(tc_[0]), "R": torch.empty_like(tr_[0])}
        trans = {"C": tc_, "R": tr_}
        comps = {f: [Composition(feats[i], rois[i], trans[f][i]) for i in range(NSETS)] for f in "CR"}

        def fwd(i, forms="CR"):
            for f in forms:
                ops.fpn_deform_roi_pool_forward(feats[i], rois[i], trans[f][i], STRIDES, P, S, STD, out=out[f],
                                                top_count=cnt[f])

        def bwd(i, forms="CR"):
            for f in forms:
                ops.fpn_deform_roi_pool_backward(dys[i], feats[i], rois[i], trans[f][i], cnt[f], STRIDES, P, S, STD,
                                                 d_feats=d_feats[f], d_trans=d_tr[f])

        def bwd_part(i, forms, req_data, req_trans):
            for f in forms:
                ops.fpn_deform_roi_pool_backward(dys[i], feats[i], rois[i], trans[f][i], cnt[f], STRIDES, P, S, STD,
                                                 req_data=req_data, req_trans=req_trans,
                                                 d_feats=d_feats[f] if req_data != "null" else None,
                                                 d_trans=d_tr[f] if req_trans != "null" else None)

        def cfwd(i, forms="CR"):
            for f in forms:
                comps[f][i].forward()

        def cbwd(i, forms="CR"):
            for f in forms:
                comps[f][i].backward(dys[i])
        r = {}
        for forms, key in (("C", "delta_c"), ("R", "delta_r"), ("CR", "both_extractors")):
            e = {}
            # the backward reads the forward's top_count (the composition its per-call state): run the forward first
            for i in range(NSETS):
                fwd(i, forms)
                cfwd(i, forms)
            # (with NSETS > 1 the state of set i must be the one the backward of set i reads: one set per timing)
            e["fused_fwd"] = both_ways(lambda i: fwd(i, forms), args.iters)
            e["composition_fwd"] = both_ways(lambda i: cfwd(i, forms), args.iters)
            fwd(0, forms)
            cfwd(0, forms)
            for c in forms:
                comps[c][1].state = None
            e["fused_bwd"] = both_ways(lambda i: bwd(0, forms), args.iters)
            e["composition_bwd"] = both_ways(lambda i: cbwd(0, forms), args.iters)
            e["fused_fwd_bwd"] = both_ways(lambda i: (fwd(0, forms), bwd(0, forms)), args.iters)
            e["composition_fwd_bwd"] = both_ways(lambda i: (cfwd(0, forms), cbwd(0, forms)), args.iters)
            e["composition_ratio"] = {k: {m: round(e["composition_" + k][m] / e["fused_" + k][m], 2)
                                          for m in ("eager_us", "graph_us")} for k in ("fwd", "bwd", "fwd_bwd")}
            # the alternative inside the same kernel: no LDS patch, one global atomic per tap
            with lib().tuned(deform_psroi_bwd_patch=0):
                e["direct_bwd"] = both_ways(lambda i: bwd(0, forms), args.iters)
            # where the backward's time goes: each of its two outputs alone (the other's req is null)
            e["fused_bwd_d_data_only"] = both_ways(lambda i: bwd_part(0, forms, "write", "null"), args.iters)
            e["fused_bwd_d_trans_only"] = both_ways(lambda i: bwd_part(0, forms, "null", "write"), args.iters)
            e["direct_over_patch"] = {m: round(e["direct_bwd"][m] / e["fused_bwd"][m], 2) for m in ("eager_us", "graph_us")}
            e["not_slower_than_composition"] = all(v >= 1.0 for k in e["composition_ratio"].values() for v in k.values())
            nx = len(forms)
            bwd_bytes = nx * (4 * B * R * C * P * P + 3 * feat_bytes)
            e["bwd_algorithmic_bytes"] = bwd_bytes
            e["bwd_fraction_of_8TBps"] = round(bwd_bytes / PEAK * 1e6 / e["fused_bwd"]["graph_us"], 3)
            r[key] = e
            print(dist, key, json.dumps(e), flush=True)
        # atomics of one backward (set 0), both forms
        for form, key in (("C", "delta_c"), ("R", "delta_r")):
            px, taps, misses = atomic_counts(rois_np[0], trans[form][0].cpu().numpy(), form)
            t = r[key]["fused_bwd"]["graph_us"]
            r[key]["bwd_atomics"] = dict(
                what="modelled on the host from every eighth RoI's tap tables, not measured",
                rois_whose_patch_does_not_fit=misses, issued=px * C, issued_bytes=4 * px * C, one_per_tap=taps * C, one_per_tap_bytes=4 * taps * C,
                issued_bytes_per_s=round(4 * px * C / (t * 1e-6), 1),
                fraction_of_guide_rate=round(4 * px * C / (t * 1e-6) / ATOMIC_RATE, 3),
                one_per_tap_ms_at_guide_rate=round(4 * taps * C / ATOMIC_RATE * 1e3, 3))
        # the two paths agree
        fwd(0)
        bwd(0)
        agree = {}
        for f in "CR":
            o = comps[f][0].forward()
            df, dt_ = comps[f][0].backward(dys[0])
            agree[f] = dict(out_equal_bits=bool(torch.equal(o, out[f])),
                            d_trans_max_abs_diff=float((dt_ - d_tr[f]).abs().max()),
                            d_feat_max_abs_diff=max(float((a - b).abs().max()) for a, b in zip(df, d_feats[f])))
        r["fused_vs_composition"] = agree
        res[dist] = r
        del comps
        torch.cuda.empty_cache()
    if not args.no_margin:
        res["margin"] = k_margin()
    res["config"] = dict(B=B, R=R, C=C, pooled=P, sample_per_part=S, trans_std=STD, strides=list(STRIDES),
                         iters=args.iters, input_sets=NSETS)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tsd_pool": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"tsd_pool_margin": res.get("margin")}))


if __name__ == "__main__":
    main()
