#!/usr/bin/env python
"""Mask R-CNN mask loss timing (simpledet_amd/csrc/sigmoid_ce.hip) at the shapes of config/mask_r50v1_fpn_1x.py:
(R, K, P) = (256, 81, 784) -- two images of 128 foreground RoIs --, (1024, 81, 784) and the class-agnostic
(256, 1, 784).

Timed from device events, eagerly and as one captured HIP graph: the fused forward, the fused backward and both
together; the drop-in SigmoidCrossEntropy at n = 1, k = R * P on the gathered row (forward + backward).  In the
same run, on the same tensors, a torch composition of what the reference's graph does: index every RoI's class
plane, binary_cross_entropy_with_logits with a mask for the -1 targets, divide by the count, and the autograd
backward into a dense (R, K, P) gradient.  The parent commit has no mask loss, so this is the baseline.
The fused backward's algorithmic bytes are 4 R K P (the gradient, written once) + 8 R P (the selected planes and
their targets, read once) + 4 R (the classes); reported as a fraction of 8 TB/s.  NSETS input sets are rotated
between calls.  Also stored: k_ref / k_gpu of tests/test_sigmoid_ce.py's margin (tests/sigmoid_ce_ref.py).

    python tools/mask_loss_time.py [--iters 50] [--sets 3] [--out profiles/mask_loss_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops  # noqa: E402
from tests import sigmoid_ce_ref as sr  # noqa: E402

PEAK = 8.0e12
SHAPES = (("b2", (256, 81, 784)), ("b8", (1024, 81, 784)), ("agnostic", (256, 1, 784)))
SCALE = 1.0


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


def torch_mask_loss(logits, cls, target):
    """forward + autograd backward of the composition; returns (loss, dense gradient)"""
    R = logits.shape[0]
    picked = logits[torch.arange(R, device=logits.device), cls.long()]
    on = target != -1.0
    per = torch.nn.functional.binary_cross_entropy_with_logits(picked, target.clamp(min=0.0), reduction="none")
    loss = (per * on).sum() / (on.sum() + 1e-5)
    (grad,) = torch.autograd.grad(loss, logits)
    return loss, grad


def k_margin():
    """per output: the worst k of the GPU over the cases of tests/sigmoid_ce_ref.py and the restatement's k there"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    worst = {o: dict(k_gpu=0.0, k_ref_there=0.0, case=None) for o in sr.OUTPUTS}

    def note(name, got, x, t, scale, outputs):
        truth, T = sr.truth(x, t, scale)
        kr = sr.k_ref(x, t, scale)
        for o in outputs:
            k = sr.k_of(got[o].cpu().numpy(), truth[o], T[o])
            if k >= worst[o]["k_gpu"] and np.isfinite(kr[o]):
                worst[o].update(k_gpu=k, k_ref_there=kr[o], case=name)
    for name, c in sr.dropin_cases():
        x, t = cu(c["x"]), cu(c["t"])
        out, loss, loss_sum, _, _ = ops.sigmoid_cross_entropy_forward(x, t, full=True)
        d, _ = ops.sigmoid_cross_entropy_backward(x, t, c["scale"])
        note(name, dict(out=out, loss=loss, loss_sum=loss_sum, d=d), c["x"], c["t"], c["scale"], sr.OUTPUTS)
    for name, c in sr.fused_cases():
        x, t, plane = sr.gather(c["logits"], c["cls"], c["target"])
        lg, cl, tg = cu(c["logits"]), cu(c["cls"]), cu(c["target"])
        out, _ = ops.mask_loss_forward(lg, cl, tg)
        d = ops.mask_loss_backward(lg, cl, tg, c["scale"])
        R = lg.shape[0]
        picked = d[torch.arange(R, device="cuda"), cu(np.maximum(plane, 0))] * cu((plane >= 0).astype(np.float32))[:, None]
        note("fused-" + name, dict(out=out, d=picked.reshape(1, -1)), x, t, c["scale"], ("out", "d"))
    return {o: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in w.items()} for o, w in worst.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mask_loss_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for name, (R, K, P) in SHAPES:
        lgs = [torch.randn((R, K, P), device="cuda", generator=gen) * 3.0 for _ in range(nsets)]
        cls = torch.randint(0, K, (R,), device="cuda", generator=gen).float()
        tgs = [torch.randint(-1, 2, (R, P), device="cuda", generator=gen).float() for _ in range(nsets)]
        out, cs = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
        d = torch.empty((R, K, P), device="cuda")
        ws = [torch.empty(ops.mask_loss_workspace_bytes(R, K, P), device="cuda", dtype=torch.uint8) for _ in range(2)]

        def fwd(i):
            ops.mask_loss_forward(lgs[i], cls, tgs[i], out=out, count_sum=cs, workspace=ws[0])

        def bwd(i):
            ops.mask_loss_backward(lgs[i], cls, tgs[i], SCALE, d_logits=d, workspace=ws[1])

        def both(i):
            fwd(i)
            bwd(i)
        bwd_bytes = 4 * R * K * P + 8 * R * P + 4 * R
        r = dict(shape=[R, K, P], bwd_algorithmic_bytes=bwd_bytes)
        for key, fn in (("fwd", fwd), ("bwd", bwd), ("fwd_bwd", both)):
            e = time_events(fn, args.iters, nsets)
            gs = graphs_of(fn, nsets)
            g_us = time_events(lambda i: gs[i].replay(), args.iters, nsets)
            del gs
            r[key] = dict(eager_us=round(e, 1), graph_us=round(g_us, 1))
        r["bwd"]["fraction_of_8TBps"] = round(bwd_bytes / PEAK * 1e6 / r["bwd"]["graph_us"], 3)
        # the drop-in operator on the gathered row, n = 1, k = R * P
        rows = [lg[torch.arange(R, device="cuda"), cls.long()].reshape(1, -1).contiguous() for lg in lgs]
        trow = [t.reshape(1, -1) for t in tgs]
        o1, ls1, cs1 = (torch.empty(1, device="cuda") for _ in range(3))
        dd = torch.empty((1, R * P), device="cuda")
        ws1 = [torch.empty(ops.sigmoid_cross_entropy_workspace_bytes(1, R * P), device="cuda", dtype=torch.uint8)
               for _ in range(2)]

        def drop(i):
            ops.sigmoid_cross_entropy_forward(rows[i], trow[i], out=o1, loss_sum=ls1, count_sum=cs1, workspace=ws1[0])
            ops.sigmoid_cross_entropy_backward(rows[i], trow[i], SCALE, d_data=dd, count_sum=cs1, workspace=ws1[1])
        e = time_events(drop, args.iters, nsets)
        gs = graphs_of(drop, nsets)
        r["dropin_n1_fwd_bwd"] = dict(k=R * P, eager_us=round(e, 1),
                                      graph_us=round(time_events(lambda i: gs[i].replay(), args.iters, nsets), 1))
        del gs
        # the baseline: a torch composition, forward + autograd backward into the dense gradient
        lgr = [lg.clone().requires_grad_() for lg in lgs]

        def torch_fn(i):
            torch_mask_loss(lgr[i], cls, tgs[i])
        e = time_events(torch_fn, args.iters, nsets)
        r["torch_composition_fwd_bwd"] = dict(eager_us=round(e, 1))
        try:
            gs = graphs_of(torch_fn, nsets)
            r["torch_composition_fwd_bwd"]["graph_us"] = round(time_events(lambda i: gs[i].replay(), args.iters, nsets), 1)
            del gs
        except Exception as ex:    # a composition that cannot be captured is compared eagerly
            torch.cuda.synchronize()
            r["torch_composition_fwd_bwd"]["graph_us"] = None
            r["torch_composition_fwd_bwd"]["graph_error"] = str(ex).splitlines()[0][:200]
        # the results agree: same loss, same gradient up to rounding
        both(0)
        tl, tg_ = torch_mask_loss(lgr[0], cls, tgs[0])
        r["max_abs_diff_vs_torch"] = dict(loss=float((out[0] - tl).abs()), grad=float((d - tg_).abs().max()))
        t = r["torch_composition_fwd_bwd"]
        t_graph = t["graph_us"] if t["graph_us"] is not None else t["eager_us"]
        r["not_slower_than_torch"] = dict(
            bwd_eager=r["bwd"]["eager_us"] <= t["eager_us"], bwd_graph=r["bwd"]["graph_us"] <= t_graph,
            fwd_bwd_eager=r["fwd_bwd"]["eager_us"] <= t["eager_us"], fwd_bwd_graph=r["fwd_bwd"]["graph_us"] <= t_graph)
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del lgs, tgs, lgr, d, rows, trow
        torch.cuda.empty_cache()
    res["margin"] = k_margin()
    res["config"] = dict(input_sets=nsets, iters=args.iters, grad_scale=SCALE)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"mask_loss": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"mask_loss": res["margin"]}))


if __name__ == "__main__":
    main()
