#!/usr/bin/env python
"""BboxPostProcessing timing (sd_bbox_post_processing: per-class hard NMS + image top-k, two launches).

Shapes (tests/bbox_post_cases.py): mask_r50 = B=2, R=1000, K=81, class-specific boxes, min_det_score 0.05,
max_det 100, thr 0.5 (config/mask_r50v1_fpn_1x.py:161-174); mask_r50_low = the same at 0.001; r2000 = B=1,
R=2000, thr 0.3, max_det 300; mask_r50_b1 = one image of mask_r50 (the existing test chain's shape).

Per shape, medians of device events, A and B interleaved call by call, NSETS input sets rotated (copied into
the buffers the calls read before the timed region):
  fused_us / fused_graph_us        ops.bbox_post_processing, eager and as a captured HIP graph
  composed_us / composed_graph_us  what the parent commit offers for the same job: det_filter ->
                                   soft_nms_batched(method 0, Nt = thr) over the same classes + a torch top-k
                                   of the surviving scores (not the same arithmetic: the Cython soft_nms adds
                                   1 in double; it is the nearest device path, not a reference)
and the Mask R-CNN test chain (ops.maskrcnn_test_chain, B=1, R=1000, 256 channels) as one graph, with the
fused op's share of it.

    python tools/bbox_post_time.py [--iters 50] [--sets 4] [--no-chain]
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
from tests import bbox_post_cases as cases  # noqa: E402

SHAPES = {  # name -> (B, R, K, parameters)
    "mask_r50": (2, 1000, 81, dict(max_det_per_image=100, min_det_score=0.05, nms_thr=0.5)),
    "mask_r50_low": (2, 1000, 81, dict(max_det_per_image=100, min_det_score=0.001, nms_thr=0.5)),
    "r2000": (1, 2000, 81, dict(max_det_per_image=300, min_det_score=0.01, nms_thr=0.3)),
    "mask_r50_b1": (1, 1000, 81, dict(max_det_per_image=100, min_det_score=0.05, nms_thr=0.5)),
}


def make_sets(name, nsets):
    B, R, K, par = SHAPES[name]
    out = []
    for k in range(nsets):
        score, bbox = cases.random_inputs(9000 + 17 * k, B, R, K, True, par["min_det_score"])
        out.append((torch.from_numpy(score).cuda(), torch.from_numpy(bbox).cuda()))
    return out


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def interleaved(fns, load, nsets, iters):
    """median microseconds of every fn, the fns taking turns on the same input set"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = [[] for _ in fns]
    for i in range(-3, iters):
        load(i % nsets)
        for k, fn in enumerate(fns):
            start.record()
            fn()
            end.record()
            end.synchronize()
            if i >= 0:
                ts[k].append(start.elapsed_time(end) * 1e3)
    return [round(float(np.median(t)), 1) for t in ts]


def time_shape(name, nsets, iters):
    B, R, K, par = SHAPES[name]
    sets = make_sets(name, nsets)
    ts, tb = torch.empty_like(sets[0][0]), torch.empty_like(sets[0][1])
    top = par["max_det_per_image"]
    ws = torch.empty(ops.bbox_post_processing_workspace_bytes(B, R, K, K, top), device="cuda", dtype=torch.uint8)
    out = (torch.empty((B, top, 1), device="cuda"), torch.empty((B, top, 4), device="cuda"),
           torch.empty((B, top, 1), device="cuda"))

    def load(i):
        ts.copy_(sets[i][0])
        tb.copy_(sets[i][1])

    def fused():
        return ops.bbox_post_processing(ts, tb, workspace=ws, out=out, **par)

    def composed():
        dets, counts = ops.det_filter(tb, ts, par["min_det_score"])
        od, oi, oc = ops.soft_nms_batched(dets, counts, 0.5, par["nms_thr"], 0.001, 0)
        # the image's best `top` of the kept scores of the foreground classes
        live = torch.arange(R, device="cuda")[None, None, :] < oc.view(B, K, 1)
        sc = torch.where(live, od.view(B, K, R, 5)[..., 4], torch.full((), -1.0, device="cuda"))
        return torch.topk(sc[:, 1:].reshape(B, -1), top, dim=1)

    load(0)
    g_fused, g_comp = capture(fused), capture(composed)
    f, c, fg, cg = interleaved([fused, composed, g_fused.replay, g_comp.replay], load, nsets, iters)
    load(0)
    fused()
    torch.cuda.synchronize()
    return {"B": B, "R": R, "K": K, **par,
            "candidates": int((sets[0][0][:, :, 1:] > par["min_det_score"]).sum()),
            "detections": int((out[2] >= 0).sum()),
            "fused_us": f, "fused_graph_us": fg, "composed_us": c, "composed_graph_us": cg,
            "fused_over_composed_graph": round(fg / cg, 3)}


def time_chain(iters):
    B, R, K, C = 1, 1000, 81, 256
    strides = list(synth.FPN_STRIDES)
    feats = [torch.randn((B, C, h, w), device="cuda") for h, w in synth.FPN_SHAPES]
    rois = torch.from_numpy(synth.random_rois(31, B, R, degenerate=False)).cuda()
    rs = np.random.RandomState(31)
    deltas = torch.from_numpy((rs.standard_normal((B, R, 4 * K)) * 0.5).astype(np.float32)).cuda()
    score = torch.from_numpy(cases.random_inputs(31, B, R, K, True, 0.05)[0]).cuda()
    info = torch.tensor([[800, 1333, 1.0]], device="cuda")
    boxes = ops.decode_bbox(rois, deltas, info, class_agnostic=False)

    def chain():
        return ops.maskrcnn_test_chain(feats, rois, score, deltas, info, strides, 100, 0.05, 0.5)

    def post():
        return ops.bbox_post_processing(score, boxes, 100, 0.05, 0.5)

    g_chain, g_post = capture(chain), capture(post)
    eager, graph, post_us = interleaved([chain, g_chain.replay, g_post.replay], lambda i: None, 1, iters)
    return {"config": "B=1, R=1000, 81 classes, 256 channels: fused FPN RoIAlign 7x7 -> DecodeBBox -> "
                      "BboxPostProcessing (0.05 / 100 / 0.5) -> fused FPN RoIAlign 14x14 of the 100 boxes; one HIP graph",
            "eager_us": eager, "graph_us": graph, "bbox_post_graph_us": post_us,
            "bbox_post_share": round(post_us / graph, 3), "host_syncs_in_chain": 0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--no-chain", action="store_true")
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    res = {"op": "bbox_post_processing", "device": torch.cuda.get_device_name(0), "iters": args.iters,
           "sets": max(2, args.sets), "shapes": {}}
    for name in args.shapes.split(","):
        res["shapes"][name] = time_shape(name, max(2, args.sets), args.iters)
    if not args.no_chain:
        res["maskrcnn_test_chain"] = time_chain(args.iters)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
