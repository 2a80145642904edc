#!/usr/bin/env python
"""Timing of the FreeAnchor training head (simpledet_amd/csrc/free_anchor.hip).

Shapes (config/FreeAnchor/free_anchor_r50v1_fpn_1x.py: strides 8..128 on 800 x 1333, A = 9 -> 200,700 anchors, K = 80,
M = 100 gt rows, pre_anchor_top_n 50, bbox_thr 0.6, alpha 0.5, gamma 2)
  bench    N = 2, 40 valid gt rows per image
  n1       N = 1, 40 valid
  valid8   N = 2, 8 valid
Timed from device events in the same run on the same inputs, the variants alternating call by call:
  forward + backward of the device call as ONE captured HIP graph, and eagerly,
  and a torch composition of the reference's graph (concat + transpose, both IoU matrices, topk, one-hot, the
  element-wise passes, autograd), eagerly: its backward clears buffers with memset nodes, which this tool does not
  record into a graph.
`not_slower_than_torch` per shape: the device call against the torch composition, both eager.

    python tools/free_anchor_time.py [--iters 20] [--out profiles/free_anchor_time.json]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import free_anchor as fa  # noqa: E402

STRIDES = (8, 16, 32, 64, 128)
IMAGE = (800, 1333)
A, K, M = 9, 80, 100
KW = dict(top_n=50, bbox_thr=0.6, alpha=0.5, gamma=2.0, mean=(0.0, 0.0, 0.0, 0.0), std=(0.1, 0.1, 0.2, 0.2))
SHAPES = dict(bench=(2, 40), n1=(1, 40), valid8=(2, 8))
BSQ = float(np.float32(math.sqrt(1 / 0.11)) ** 2)     # smooth_l1's scalar squared in float, as the kernel has it
IBSQ = float(np.float32(1) / np.float32(BSQ))


def make_anchors(stride, S):
    ctr = (np.arange(S) * stride + (stride - 1) / 2).astype(np.float64)
    out = np.zeros((S, S, A, 4))
    a = 0
    for ratio in (0.5, 1.0, 2.0):
        for k in range(3):
            size = stride * 4 * 2 ** (k / 3.0)
            w, h = size / math.sqrt(ratio), size * math.sqrt(ratio)
            out[:, :, a] = np.stack(np.broadcast_arrays(ctr[None] - (w - 1) / 2, ctr[:, None] - (h - 1) / 2,
                                                        ctr[None] + (w - 1) / 2, ctr[:, None] + (h - 1) / 2), -1)
            a += 1
    return torch.from_numpy(out.reshape(1, 1, S, S, A * 4).astype(np.float32)).cuda()


def inputs(N, valid, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    rs = np.random.RandomState(seed)
    sizes = [(-(-IMAGE[0] // s), -(-IMAGE[1] // s)) for s in STRIDES]
    cls = [torch.randn((N, A * K, h, w), device="cuda", generator=gen) - 4 for h, w in sizes]
    delta = [torch.randn((N, A * 4, h, w), device="cuda", generator=gen) * 0.5 for h, w in sizes]
    anchors = [make_anchors(s, 1440 // s) for s in STRIDES]
    gt = np.full((N, M, 5), -1, np.float32)
    for n in range(N):
        w, h = rs.uniform(32, 400, valid), rs.uniform(32, 400, valid)
        cx, cy = rs.uniform(0, IMAGE[1], valid), rs.uniform(0, IMAGE[0], valid)
        gt[n, :valid] = np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2, rs.randint(1, K + 1, valid)], 1)
    im_info = torch.tensor([[IMAGE[0], IMAGE[1], 1.0]] * N, device="cuda")
    return cls, delta, anchors, torch.from_numpy(gt).cuda(), im_info


def box_iou(a, g):
    a, g = a[:, None, :], g[None, :, :]
    w = (torch.minimum(a[..., 2], g[..., 2]) - torch.maximum(a[..., 0], g[..., 0])).clamp(min=0)
    h = (torch.minimum(a[..., 3], g[..., 3]) - torch.maximum(a[..., 1], g[..., 1])).clamp(min=0)
    i = w * h
    u = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])) - i
    return torch.where(u <= 0, torch.zeros_like(u), i / u)


def torch_free_anchor(cls, delta, anchors, gt, im_info, grad_scale=1.0):
    """the reference's graph (builder.py:67-148, ops.py:44-210): (positive, negative, gradients of every level)"""
    N, top_n, mean, std = gt.shape[0], KW["top_n"], KW["mean"], KW["std"]
    cat = lambda ts, c: torch.cat([t.reshape(N, t.shape[1], -1) for t in ts], 2).transpose(1, 2).reshape(N, -1, c)
    cls_prob, deltas = torch.sigmoid(cat(cls, K)), cat(delta, 4)
    anc = torch.cat([a[:, :, :t.shape[2], :t.shape[3]].reshape(1, -1, 4) for a, t in zip(anchors, cls)], 1)
    anc = anc.expand(N, -1, 4)
    labels, boxes = gt[..., 4], gt[..., :4]
    nvalid = (labels > 0).sum().clamp(min=1)
    bags = torch.stack([box_iou(boxes[n], anc[n]) for n in range(N)]).topk(top_n, dim=2).indices
    bi = torch.arange(N, device=gt.device)[:, None, None].expand_as(bags)
    ci = (labels - 1).clamp(min=0).long()[..., None].expand_as(bags)
    p, d, ex = cls_prob[bi, bags, ci], deltas[bi, bags], anc[bi, bags]
    g = boxes[:, :, None, :].expand_as(ex)
    ew, eh = ex[..., 2] - ex[..., 0] + 1, ex[..., 3] - ex[..., 1] + 1
    gw, gh = g[..., 2] - g[..., 0] + 1, g[..., 3] - g[..., 1] + 1
    t = [(g[..., 0] + 0.5 * (gw - 1) - ex[..., 0] - 0.5 * (ew - 1)) / ew,
         (g[..., 1] + 0.5 * (gh - 1) - ex[..., 1] - 0.5 * (eh - 1)) / eh, torch.log(gw / ew), torch.log(gh / eh)]
    v = d - torch.stack([(t[j] - mean[j]) / std[j] for j in range(4)], -1)
    sl1 = torch.where(v.abs() > IBSQ, v.abs() - 0.5 * IBSQ, v * v * (0.5 * BSQ)) * 0.75
    q = p * torch.exp(-sl1.sum(-1))
    q = torch.where((labels > 0)[..., None], q, torch.ones_like(q))
    w = 1.0 / (1.0 - q).clamp(min=1e-12)
    pos = (-KW["alpha"] * torch.log(((w / w.sum(-1, keepdim=True)) * q).sum(-1).clamp(1e-12, 1.0)) / nvalid).sum()
    width, height = anc[..., 2] - anc[..., 0] + 1, anc[..., 3] - anc[..., 1] + 1
    dd = deltas.detach()
    lim = [(im_info[:, 1] - 1)[:, None], (im_info[:, 0] - 1)[:, None]]
    pred = torch.stack([torch.minimum(anc[..., j] + (dd[..., j] * std[j] + mean[j]) * (width, height)[j % 2],
                                      lim[j % 2]).clamp(min=0) for j in range(4)], -1)
    iou2 = torch.stack([box_iou(boxes[n], pred[n]) for n in range(N)])
    t2 = iou2.max(2, keepdim=True).values.clamp(min=KW["bbox_thr"] + 1e-12)
    gpp = ((iou2 - KW["bbox_thr"]) / (t2 - KW["bbox_thr"])).clamp(0.0, 1.0)
    best, arg = gpp.max(1)
    lab = torch.gather(labels, 1, arg)
    box_prob = torch.nn.functional.one_hot((lab - 1).clamp(min=0).long(), K) * ((lab > 0)[..., None] * best[..., None])
    prob = torch.where((lab > 0)[..., None], cls_prob * (1.0 - box_prob), torch.zeros_like(cls_prob))
    neg = ((1.0 - KW["alpha"]) * (-prob ** KW["gamma"] * torch.log((1.0 - prob).clamp(1e-12, 1.0)))
           / (nvalid * top_n)).sum()
    return pos, neg, torch.autograd.grad((pos + neg) * grad_scale, list(cls) + list(delta))


def time_pair(fns, iters):
    """median microseconds of each function, the calls alternating"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for fn in fns * 3:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(iters):
        for t, fn in zip(ts, fns):
            start.record()
            fn()
            end.record()
            end.synchronize()
            t.append(start.elapsed_time(end) * 1e3)
    return [round(float(np.median(t)), 1) for t in ts]


def graph_of(fn):
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


def time_shape(name, iters):
    N, valid = SHAPES[name]
    cls, delta, anchors, gt, im_info = inputs(N, valid, 3)
    hws = [t.shape[2] * t.shape[3] for t in cls]
    ws = torch.empty(fa.workspace_bytes(N, hws, A, K, M, KW["top_n"]), dtype=torch.uint8, device="cuda")
    d_cls, d_delta = [torch.empty_like(t) for t in cls], [torch.empty_like(t) for t in delta]
    out = {}

    def device():
        out["loss"] = fa.free_anchor_loss_forward(cls, delta, anchors, gt, im_info, workspace=ws, **KW)[0]
        fa.free_anchor_loss_backward(cls, delta, anchors, gt, im_info, ws, d_cls=d_cls, d_delta=d_delta, **KW)
    req = [t.clone().requires_grad_() for t in cls + delta]

    def composition():
        out["torch"] = torch_free_anchor(req[:len(cls)], req[len(cls):], anchors, gt, im_info)
    g = graph_of(device)
    graph, eager, torch_eager = time_pair([g.replay, device, composition], iters)
    torch.cuda.synchronize()
    tp, tn, tg = out["torch"]
    res = dict(shape=dict(N=N, anchors=sum(hws) * A, K=K, M=M, valid=valid, top_n=KW["top_n"]),
               device=dict(eager_us=eager, graph_us=graph), torch_composition=dict(eager_us=torch_eager),
               vs_torch=dict(positive=[float(out["loss"][0]), float(tp.detach())],
                             negative=[float(out["loss"][1]), float(tn.detach())],
                             grad_max_diff=max(float((a - b).abs().max()) for a, b in zip(d_cls + d_delta, tg)),
                             grad_max=max(float(b.abs().max()) for b in tg)))
    res["not_slower_than_torch"] = res["device"]["eager_us"] <= res["torch_composition"]["eager_us"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "free_anchor_time.json"))
    args = ap.parse_args()
    res = {name: time_shape(name, args.iters) for name in SHAPES}
    res["not_slower_than_torch"] = {k: res[k]["not_slower_than_torch"] for k in SHAPES}
    res["run"] = dict(iters=args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"free_anchor": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"free_anchor": res}))


if __name__ == "__main__":
    main()
