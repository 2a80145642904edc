#!/usr/bin/env python
"""RetinaNet training-head timing at the config's shape (config/retina_r50v1_fpn_1x.py): B = 2,
200 700 anchors, 80 classes, alpha 0.25, gamma 2, normalization 'valid'.

Timed from device events, eagerly and as one captured HIP graph each: focal forward, focal backward,
BBoxNorm backward, the anchor targets, and the chain retina_anchor_target -> focal_loss_bwd +
bbox_norm_bwd as one graph.  Algorithmic bytes: focal backward 8 * B * nbox * nclass + 4 * B * nbox,
forward 8 * B * nbox * nclass, BBoxNorm 8 * B * 4A * sumHW + 4 * B * nbox; reported as a fraction of
8 TB/s.  The (B, nbox, nclass) tensors are 128 MB each and the MALL holds 256 MB, so NSETS input sets
are rotated between replays.  In the same run: the same expressions composed from torch element-wise
ops on the device (the nearest thing possible without these kernels); for the anchor targets the numpy
reference's host time is the figure recorded with tests/golden/retina_target.npz.
Also stored: k_ref / k_gpu of tests/test_focal_loss.py's margin (see tests/focal_ref.py).

    python tools/retina_loss_time.py [--iters 30] [--sets 3] [--out profiles/retina_loss_time.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops  # noqa: E402
from simpledet_amd._lib import lib  # noqa: E402
from tests import focal_ref as fr, retinacases  # noqa: E402

B, NBOX, K, A, SUMHW = 2, 200700, 80, 9, 22300
ALPHA, GAMMA = 0.25, 2.0
PEAK = 8.0e12


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


def torch_focal_bwd(out, label, gdata):
    """focal_loss-inl.h:186-230 from torch element-wise ops (every line a full-size pass)"""
    eps = 1e-14
    positive = ALPHA * (1 - out) ** GAMMA * (GAMMA * out * torch.log(out + eps) + out - 1)
    negative = -((1 - ALPHA) * out ** GAMMA * (GAMMA * (1 - out) * torch.log(1 - out + eps) - out))
    hot = (label - 1).to(torch.int64).unsqueeze(-1) == torch.arange(K, device=out.device)
    grad = torch.where(hot, positive, negative)
    grad = torch.where((label == -1).unsqueeze(-1), torch.zeros((), device=out.device), grad)
    norm = (label >= 1).sum().to(torch.float32) + 1
    torch.div(grad, norm, out=gdata)


def k_margin():
    """max k of the GPU and of the float32 host restatement over the cases of tests/focal_ref.py"""
    k_ref = k_gpu = 0.0
    for _, c in fr.cases():
        truth, T, s, _ = fr.focal_bwd_truth(**c)
        k_ref = max(k_ref, fr.k_of(fr.focal_bwd_f32(**c), truth, T, s))
        cu = lambda a: None if a is None else torch.from_numpy(a).cuda()
        got = ops.focal_loss_backward(cu(c["out"]), cu(c["label"]), cu(c["ograd"]), alpha=c["alpha"], gamma=c["gamma"],
                                      grad_scale=c["grad_scale"], normalization=c["normalization"]).cpu().numpy()
        k_gpu = max(k_gpu, fr.k_of(got, truth, T, s))
    x = fr.logits(np.random.RandomState(5), (2, 4099, 80))
    ks_ref = fr.k_sigmoid(fr.sigmoid_f32(x), x)
    ks_gpu = fr.k_sigmoid(ops.focal_loss_forward(torch.from_numpy(x).cuda()).cpu().numpy(), x)
    return dict(k_ref_backward=round(k_ref, 3), k_gpu_backward=round(k_gpu, 3), k_ref_sigmoid=round(ks_ref, 3),
                k_gpu_sigmoid=round(ks_gpu, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retina_loss_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    # anchor targets of two config images: their labels feed the loss ops
    cfg = retinacases.RETINA
    ins = [retinacases.inputs(retinacases.CASES[n])[0] for n in ("cfg_landscape", "cfg_duplicate_gt_holes")]
    im = torch.from_numpy(np.stack([x[0] for x in ins])).cuda()
    gt = torch.from_numpy(np.stack([x[1] for x in ins])).cuda()
    prm = ops.rpn_target_param(cfg["stride"], cfg["short"], cfg["long"], cfg["scales"], cfg["aspects"],
                               cfg["allowed_border"], cfg["pos_thr"], cfg["neg_thr"], cfg["min_pos_thr"])
    label = ops.retina_anchor_target(im, gt, prm, layout=1)[0]
    logit = [torch.randn((B, NBOX, K), device="cuda", generator=gen) * 2 - 4.6 for _ in range(nsets)]
    out = [ops.focal_loss_forward(x) for x in logit]
    gdata = torch.empty_like(out[0])
    gout = [torch.randn((B, 4 * A, SUMHW), device="cuda", generator=gen) for _ in range(nsets)]
    gbox = torch.empty_like(gout[0])
    ws = [torch.empty(ops.focal_loss_workspace_bytes(), device="cuda", dtype=torch.uint8) for _ in range(2)]
    lib().cdll.sd_retina_target_workspace_bytes.restype = ctypes.c_size_t
    tws = torch.empty(int(lib().cdll.sd_retina_target_workspace_bytes(ctypes.byref(prm), B, gt.shape[1])),
                      device="cuda", dtype=torch.uint8)
    n = B * NBOX * K
    bytes_ = dict(focal_fwd=8 * n, focal_bwd=8 * n + 4 * B * NBOX, bbox_norm_bwd=8 * B * 4 * A * SUMHW + 4 * B * NBOX)
    kw = dict(alpha=ALPHA, gamma=GAMMA, grad_scale=1.0, normalization="valid")
    fns = dict(
        focal_fwd=lambda i: ops.focal_loss_forward(logit[i], out=gdata),
        focal_bwd=lambda i: ops.focal_loss_backward(out[i], label, gdata=gdata, workspace=ws[0], **kw),
        bbox_norm_bwd=lambda i: ops.bbox_norm_backward(gout[i], label, gdata=gbox, workspace=ws[1]),
        anchor_target=lambda i: ops.retina_anchor_target(im, gt, prm, layout=1, workspace=tws),
        torch_focal_fwd=lambda i: torch.sigmoid(logit[i], out=gdata),
        torch_focal_bwd=lambda i: torch_focal_bwd(out[i], label, gdata),
        torch_bbox_norm_bwd=lambda i: torch.div(gout[i], torch.clamp((label >= 1).sum().float() + 1, min=1), out=gbox),
    )

    def chain(i):
        lab = ops.retina_anchor_target(im, gt, prm, layout=1, workspace=tws)[0]
        ops.focal_loss_backward(out[i], lab, gdata=gdata, workspace=ws[0], **kw)
        ops.bbox_norm_backward(gout[i], lab, gdata=gbox, workspace=ws[1])
    fns["chain_target_focal_bbox"] = chain
    res = {}
    for name, fn in fns.items():
        r = dict(eager_us=round(time_events(fn, args.iters, nsets), 1))
        if not name.startswith("torch_"):
            gs = graphs_of(fn, nsets)
            r["graph_us"] = round(time_events(lambda i: gs[i].replay(), args.iters, nsets), 1)
            del gs
        if name in bytes_:
            r["algorithmic_bytes"] = bytes_[name]
            r["roofline_us_at_8TBps"] = round(bytes_[name] / PEAK * 1e6, 2)
            r["fraction_of_8TBps"] = round(bytes_[name] / PEAK * 1e6 / r.get("graph_us", r["eager_us"]), 3)
        res[name] = r
        print(name, json.dumps(r), flush=True)
    gold = np.load(os.path.join(ROOT, "tests", "golden", "retina_target.npz"))
    res["anchor_target"]["numpy_reference_host_us"] = round(
        1e6 * sum(float(gold[k + "/0/host_seconds"][0]) for k in ("cfg_landscape", "cfg_duplicate_gt_holes")), 0)
    res["margin"] = k_margin()
    res["shape"] = dict(B=B, nbox=NBOX, nclass=K, alpha=ALPHA, gamma=GAMMA, normalization="valid", input_sets=nsets)
    res["fused_focal_bwd_faster_than_torch"] = res["focal_bwd"]["eager_us"] < res["torch_focal_bwd"]["eager_us"]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"retina_loss": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"retina_loss": res}))
    assert res["fused_focal_bwd_faster_than_torch"], "the fused focal backward lost to the composed torch form"


if __name__ == "__main__":
    main()
