#!/usr/bin/env python
"""GenProposalRetina timing: one 800x1333 test image, B=1, A=9, K=80, P3-P7, pre=1000, thresh 0.05
(0 at stride 128, models/retinanet/builder.py:373).

Variants: "prior" cls_prob = sigmoid(N(-4.595, 1)) (the RetinaNet prior bias, ~5 % over 0.05),
"sparse" sigmoid(N(-6, 1)), "dense" the prior scores with thresh 0 on every level.
Reported per variant: per-level and five-level times from device events, the five levels with their
GenAnchor as one captured HIP graph, the algorithmic bytes (cls_prob + the deltas and anchors of the
rows above the threshold + the outputs), the fraction of 8 TB/s, and the numpy restatement's host
time.  One image's cls_prob (64 MB) fits the 256 MB MALL, so NSETS input sets are rotated between
replays.

    python tools/retina_decode_time.py [--iters 50] [--sets 6] [--no-host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops  # noqa: E402

STRIDES = (8, 16, 32, 64, 128)
SHAPES = ((100, 167), (50, 84), (25, 42), (13, 21), (7, 11))
SCALES = (4 * 2 ** 0, 4 * 2 ** (1.0 / 3.0), 4 * 2 ** (2.0 / 3.0))
RATIOS = (0.5, 1.0, 2.0)
A, K, PRE = 9, 80, 1000
PEAK = 8.0e12


def make_sets(mu, nsets, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    sets = []
    for _ in range(nsets):
        lv = []
        for H, W in SHAPES:
            cls = torch.sigmoid(torch.randn((1, A * K, H, W), device="cuda", generator=g) + mu)
            dl = torch.randn((1, 4 * A, H, W), device="cuda", generator=g) * 0.2
            lv.append((cls.contiguous(), dl.contiguous()))
        sets.append(lv)
    return sets


def thresholds(dense):
    return [0.0 if (dense or s == 128) else 0.05 for s in STRIDES]


def run_level(cls, dl, info, anc, thr, ws):
    return ops.gen_proposal_retina(cls, dl, info, anc, num_anchors=A, rpn_pre_nms_top_n=PRE, rpn_min_size=0,
                                   thresh=thr, workspace=ws)


def algorithmic_bytes(sets, thr):
    total = 0
    for (cls, _), t in zip(sets[0], thr):
        surv = int((cls > t).sum())
        total += cls.numel() * 4 + surv * (16 + 16)     # scores + the survivors' 4 deltas and anchor
        total += PRE * 4 * 4 + PRE * (K + 1) * 4         # out + score
    return total


def time_events(fn, iters, nsets):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    nsets = max(5, args.sets)
    info = torch.tensor([[800.0, 1333.0, 1.0]], device="cuda")
    anchors = ops.gen_anchor_levels(SHAPES, STRIDES, SCALES, RATIOS)
    wsb = max(ops.gen_proposal_retina_workspace_bytes(1, A * K, H, W) for H, W in SHAPES)
    ws = [torch.empty(wsb, device="cuda", dtype=torch.uint8) for _ in SHAPES]
    print("input sets rotated between timed calls / replays: %d (one image's cls_prob = 64 MB; MALL 256 MB)"
          % nsets)
    results = {}
    for name, mu, dense in (("prior", -4.595, False), ("sparse", -6.0, False), ("dense", -4.595, True)):
        sets = make_sets(mu, nsets, 1)
        thr = thresholds(dense)
        per_level = []
        for lvl in range(5):
            per_level.append(time_events(
                lambda i, l=lvl: run_level(sets[i][l][0], sets[i][l][1], info, anchors[l], thr[l], ws[l]),
                args.iters, nsets))

        def five(i):
            for l in range(5):
                run_level(sets[i][l][0], sets[i][l][1], info, anchors[l], thr[l], ws[l])
        t5 = time_events(five, args.iters, nsets)
        # one graph per input set: GenAnchor (all levels) + the five GenProposalRetina calls
        graphs = []
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            five(0)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        for i in range(nsets):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                anc = ops.gen_anchor_levels(SHAPES, STRIDES, SCALES, RATIOS)
                for l in range(5):
                    run_level(sets[i][l][0], sets[i][l][1], info, anc[l], thr[l], ws[l])
            graphs.append(g)
        tg = time_events(lambda i: graphs[i].replay(), args.iters, nsets)
        nbytes = algorithmic_bytes(sets, thr)
        host = None
        if not args.no_host:
            from tests import retina_ref
            cpu = [(c.cpu().numpy(), d.cpu().numpy()) for c, d in sets[0]]
            anc_np = [a.cpu().numpy() for a in anchors]
            t0 = time.perf_counter()
            for (c, d), a, t in zip(cpu, anc_np, thr):
                retina_ref.gen_proposal_retina(c, d, info.cpu().numpy(), a, A, rpn_pre_nms_top_n=PRE,
                                               rpn_min_size=0, thresh=t)
            host = (time.perf_counter() - t0) * 1e6
        r = dict(per_level_us=[round(v, 1) for v in per_level], five_levels_us=round(t5, 1),
                 graph_us=round(tg, 1), algorithmic_bytes=nbytes,
                 roofline_us=round(nbytes / PEAK * 1e6, 2),
                 fraction_of_8TBps_graph=round(nbytes / PEAK * 1e6 / tg, 3),
                 numpy_host_us=None if host is None else round(host, 0))
        results[name] = r
        print(name, json.dumps(r))
        del graphs
    print(json.dumps({"retina_decode": results}))


if __name__ == "__main__":
    main()
