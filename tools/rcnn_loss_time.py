#!/usr/bin/env python
"""Timing of the Faster / Mask R-CNN loss heads (simpledet_amd/csrc/rcnn_loss.hip).

Shapes
  rpn_bench   config/faster_r50v1_fpn_1x.py: N = 2, A = 3, P2-P6 of 800 x 1333 (200x334 ... 13x21), image_anchor 256
  rpn_n1      the same with N = 1
  rpn_c4      one level of stride 16 (50 x 84), A = 15, N = 2: the C4 head of symbol/builder.py
  rcnn_1024   (R, K) = (1024, 81), D = 324;   rcnn_512   (512, 81)
Each head is timed from device events, all in the same run on the same inputs,
  forward + backward of the device call as ONE captured HIP graph, and eagerly,
  and a torch composition of the reference's graph both ways: reshape + cat of the levels, softmax (the node's
  output), the cross-entropy gradient by autograd with ignore_index, and the smooth-L1 chain behind the weight.
Also the chains rpn_anchor_target -> rpn_loss forward -> backward and proposal_target -> rcnn_loss forward ->
backward, one graph each.  These shapes are launch bound: no fraction of the memory bandwidth is claimed.
`not_slower_than_torch` per shape: the device call as a graph against the torch composition as a graph.

    python tools/rcnn_loss_time.py [--iters 50] [--sets 3] [--out profiles/rcnn_loss_time.json]
    python tools/rcnn_loss_time.py --kernels-only      (a short run of the device calls, for a kernel trace)
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

FPN_SIZES = ((200, 334), (100, 167), (50, 84), (25, 42), (13, 21))
RPN_SHAPES = dict(rpn_bench=(2, 3, FPN_SIZES), rpn_n1=(1, 3, FPN_SIZES), rpn_c4=(2, 15, ((50, 84),)))
RCNN_SHAPES = dict(rcnn_1024=(1024, 81), rcnn_512=(512, 81))
IMAGE_ANCHOR = 256


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


def graphs_of(fn, nsets):
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


def both_ways(fn, iters, nsets):
    e = time_events(fn, iters, nsets)
    gs = graphs_of(fn, nsets)
    g = time_events(lambda i: gs[i].replay(), iters, nsets)
    del gs
    return dict(eager_us=round(e, 1), graph_us=round(g, 1))


def smooth_l1(v, sigma):
    s2 = sigma * sigma
    return torch.where(v.abs() > 1 / s2, v.abs() - 0.5 / s2, 0.5 * s2 * v * v)


# ------------------------------------------------------------------------------------------- RPN --
def rpn_inputs(N, A, sizes, nsets):
    gen = torch.Generator(device="cuda").manual_seed(3)
    HW = sum(h * w for h, w in sizes)
    rs = np.random.RandomState(4)
    sets = []
    for _ in range(nsets):
        cls = [torch.randn((N, 2 * A, h, w), device="cuda", generator=gen) * 2 for h, w in sizes]
        delta = [torch.randn((N, 4 * A, h, w), device="cuda", generator=gen) * 0.5 for h, w in sizes]
        label = np.full((N, A * HW), -1, np.float32)
        weight = np.zeros((N, A, 4, HW), np.float32)
        for n in range(N):
            pick = rs.choice(A * HW, IMAGE_ANCHOR, replace=False)
            label[n, pick] = 0
            label[n, pick[:IMAGE_ANCHOR // 4]] = 1
            a, q = np.divmod(pick[:IMAGE_ANCHOR // 4], HW)
            weight[n, a, :, q] = 1
        target = torch.randn((N, 4 * A, HW), device="cuda", generator=gen) * 0.5
        sets.append((cls, delta, torch.from_numpy(label).cuda(), target,
                     torch.from_numpy(weight.reshape(N, 4 * A, HW)).cuda()))
    return sets


def torch_rpn(cls, delta, label, target, weight, cls_gs, reg_gs):
    """the reference's graph: (prob, reg_loss, gradients of every level tensor)"""
    N, A = cls[0].shape[0], cls[0].shape[1] // 2
    x = torch.cat([c.reshape(N, 2, A, -1) for c in cls], dim=-1)
    d = torch.cat([t.reshape(N, 4 * A, -1) for t in delta], dim=2)
    prob = torch.softmax(x, dim=1)
    valid = (label != -1).sum().clamp(min=1)
    ce = torch.nn.functional.cross_entropy(x.reshape(N, 2, -1), label.long(), ignore_index=-1, reduction="sum")
    reg = weight * smooth_l1(d - target, 3.0)
    total = ce * (cls_gs / valid) + reg.sum() * reg_gs
    return prob, reg, torch.autograd.grad(total, list(cls) + list(delta))


def time_rpn(name, iters, nsets):
    N, A, sizes = RPN_SHAPES[name]
    HW = sum(h * w for h, w in sizes)
    sets = rpn_inputs(N, A, sizes, nsets)
    reg_gs = 1.0 / (N * IMAGE_ANCHOR)
    prob = torch.empty((N, 2, A, HW), device="cuda")
    reg = torch.empty((N, 4 * A, HW), device="cuda")
    state = ops.loss_state()
    ws = torch.empty(ops.rpn_loss_workspace_bytes(N, A, HW), dtype=torch.uint8, device="cuda")
    d_cls = [torch.empty_like(t) for t in sets[0][0]]
    d_delta = [torch.empty_like(t) for t in sets[0][1]]

    def fwd_bwd(i):
        s = sets[i]
        ops.rpn_loss_forward(*s, prob=prob, reg_loss=reg, state=state, workspace=ws)
        ops.rpn_loss_backward(*s, state, cls_grad_scale=1.0, reg_grad_scale=reg_gs, d_cls=d_cls, d_delta=d_delta)
    req = [([t.clone().requires_grad_() for t in s[0]], [t.clone().requires_grad_() for t in s[1]]) for s in sets]

    def t_fwd_bwd(i):
        return torch_rpn(req[i][0], req[i][1], *sets[i][2:], 1.0, reg_gs)
    res = dict(shape=dict(N=N, A=A, levels=[list(s) for s in sizes], HW=HW, rows=N * A * HW),
               device=both_ways(fwd_bwd, iters, nsets), torch_composition=both_ways(t_fwd_bwd, iters, nsets))
    fwd_bwd(0)
    tp, tr, tg = [t.detach() if isinstance(t, torch.Tensor) else t for t in t_fwd_bwd(0)]
    torch.cuda.synchronize()
    m = [float(v) for v in ops.rpn_loss_metrics(state)]
    res["vs_torch"] = dict(prob_max_diff=float((prob - tp).abs().max()), reg_loss_max_diff=float((reg - tr).abs().max()),
                           d_cls_max_diff=max(float((a - b).abs().max()) for a, b in zip(d_cls, tg[:len(d_cls)])),
                           d_delta_max_diff=max(float((a - b).abs().max()) for a, b in zip(d_delta, tg[len(d_cls):])),
                           metrics=m)
    res["not_slower_than_torch"] = res["device"]["graph_us"] <= res["torch_composition"]["graph_us"]
    return res, fwd_bwd


def time_rpn_chain(iters):
    N, A = 2, 3
    prm = ops.rpn_target_param(stride=(4, 8, 16, 32, 64), short=tuple(h for h, _ in FPN_SIZES),
                               long=tuple(w for _, w in FPN_SIZES), scales=(8,), aspects=(0.5, 1.0, 2.0),
                               image_anchor=IMAGE_ANCHOR)
    cls, delta = rpn_inputs(N, A, FPN_SIZES, 1)[0][:2]
    im_info = torch.tensor([[800, 1333, 1.0]] * N, device="cuda")
    gt = torch.from_numpy(np.ascontiguousarray(synth.gt_boxes(3, N, 100))).cuda()
    st = ops.mt19937_state(seed=7)

    def chain(i):
        label, target, weight = ops.rpn_anchor_target(im_info, gt, prm, st, layout=1)
        out = ops.rpn_loss_forward(cls, delta, label, target, weight)
        ops.rpn_loss_backward(cls, delta, label, target, weight, out.state, reg_grad_scale=1.0 / (N * IMAGE_ANCHOR))
    return both_ways(chain, iters, 1)


# ----------------------------------------------------------------------------------------- R-CNN --
def rcnn_inputs(R, K, nsets):
    gen = torch.Generator(device="cuda").manual_seed(5)
    rs = np.random.RandomState(6)
    sets = []
    for _ in range(nsets):
        label = np.where(rs.uniform(size=R) < 0.25, rs.randint(1, K, size=R), 0).astype(np.float32)
        weight = np.zeros((R, K, 4), np.float32)
        weight[np.arange(R)[label > 0], label[label > 0].astype(int)] = 1
        sets.append((torch.randn((R, K), device="cuda", generator=gen) * 2, torch.from_numpy(label).cuda(),
                     torch.randn((R, 4 * K), device="cuda", generator=gen) * 0.5,
                     torch.randn((R, 4 * K), device="cuda", generator=gen) * 0.5,
                     torch.from_numpy(weight.reshape(R, 4 * K)).cuda()))
    return sets


def torch_rcnn(x, label, delta, target, weight, cls_gs, reg_gs):
    prob = torch.softmax(x, dim=1)
    ce = torch.nn.functional.cross_entropy(x, label.long(), reduction="sum")
    reg = weight * smooth_l1(delta - target, 1.0)
    total = ce * (cls_gs / x.shape[0]) + reg.sum() * reg_gs
    return prob, reg, torch.autograd.grad(total, [x, delta])


def time_rcnn(name, iters, nsets):
    R, K = RCNN_SHAPES[name]
    sets = rcnn_inputs(R, K, nsets)
    prob, reg = torch.empty((R, K), device="cuda"), torch.empty((R, 4 * K), device="cuda")
    gx, gd = torch.empty((R, K), device="cuda"), torch.empty((R, 4 * K), device="cuda")
    state = ops.loss_state()
    ws = torch.empty(ops.rcnn_loss_workspace_bytes(R), dtype=torch.uint8, device="cuda")

    def fwd_bwd(i):
        ops.rcnn_loss_forward(*sets[i], prob=prob, reg_loss=reg, state=state, workspace=ws)
        ops.rcnn_loss_backward(*sets[i], state, reg_grad_scale=1.0 / R, d_cls_logit=gx, d_bbox_delta=gd)
    req = [(s[0].clone().requires_grad_(), s[2].clone().requires_grad_()) for s in sets]

    def t_fwd_bwd(i):
        s = sets[i]
        return torch_rcnn(req[i][0], s[1], req[i][1], s[3], s[4], 1.0, 1.0 / R)
    res = dict(shape=dict(R=R, K=K, D=4 * K), device=both_ways(fwd_bwd, iters, nsets),
               torch_composition=both_ways(t_fwd_bwd, iters, nsets))
    fwd_bwd(0)
    tp, tr, tg = [t.detach() if isinstance(t, torch.Tensor) else t for t in t_fwd_bwd(0)]
    torch.cuda.synchronize()
    res["vs_torch"] = dict(prob_max_diff=float((prob - tp).abs().max()), reg_loss_max_diff=float((reg - tr).abs().max()),
                           d_cls_max_diff=float((gx - tg[0]).abs().max()), d_delta_max_diff=float((gd - tg[1]).abs().max()),
                           metrics=[float(v) for v in ops.rcnn_loss_metrics(state)])
    res["not_slower_than_torch"] = res["device"]["graph_us"] <= res["torch_composition"]["graph_us"]
    return res, fwd_bwd


def time_rcnn_chain(iters):
    B, S, K = 2, 512, 81
    prois, gt = synth.proposal_target_inputs(0, B, 2000, 100)
    rois, gts = torch.from_numpy(prois).cuda(), torch.from_numpy(gt).cuda()
    x, _, d = rcnn_inputs(B * S, K, 1)[0][:3]
    rng = ops.glibc_rand_state(1)

    def chain(i):
        pt = ops.proposal_target(rois, gts, K, B, S, rng_state=rng)
        label, target, weight = pt[1].reshape(-1), pt[2].reshape(B * S, -1), pt[3].reshape(B * S, -1)
        out = ops.rcnn_loss_forward(x, label, d, target, weight)
        ops.rcnn_loss_backward(x, label, d, target, weight, out.state, reg_grad_scale=1.0 / (B * S))
    return both_ways(chain, iters, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rcnn_loss_time.json"))
    ap.add_argument("--kernels-only", action="store_true", help="run the device calls a few times and exit")
    args = ap.parse_args()
    nsets = max(1, args.sets)
    if args.kernels_only:
        for name in ("rpn_bench", "rcnn_1024"):
            fn = (time_rpn if name in RPN_SHAPES else time_rcnn)(name, 3, 1)[1]
            for _ in range(20):
                fn(0)
        torch.cuda.synchronize()
        return
    res = dict(event_floor_us=round(time_events(lambda i: None, args.iters, 1), 1))
    for name in RPN_SHAPES:
        res[name] = time_rpn(name, args.iters, nsets)[0]
    for name in RCNN_SHAPES:
        res[name] = time_rcnn(name, args.iters, nsets)[0]
    res["chain_rpn_anchor_target_rpn_loss"] = time_rpn_chain(args.iters)
    res["chain_proposal_target_rcnn_loss"] = time_rcnn_chain(args.iters)
    res["not_slower_than_torch"] = {k: res[k]["not_slower_than_torch"] for k in list(RPN_SHAPES) + list(RCNN_SHAPES)}
    res["run"] = dict(input_sets=nsets, iters=args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"rcnn_loss": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"rcnn_loss": res}))


if __name__ == "__main__":
    main()
