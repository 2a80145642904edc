#!/usr/bin/env python
"""Mask Scoring R-CNN training head timing (simpledet_amd/csrc/msrcnn_head.hip) at (R, K, P) = (256, 81, 784) -- the
config's two images of 128 foreground RoIs --, (128, 81, 784) and (1024, 81, 784).

The chain: mask-loss forward (loss + prob) -> MaskIoU forward -> MaskIoU backward -> mask-loss backward with a d_prob.
Timed from device events, eagerly and as one captured HIP graph, NSETS input sets rotated between calls.  In the same
run, on the same tensors:
  (a) a torch composition of the reference's two subgraphs with autograd: index every RoI's class plane, sigmoid,
      the masked cross-entropy, the indexed IoU prediction, the MaskIoU target computed ON THE HOST from four .cpu()
      copies (what the reference's Python CustomOp does with asnumpy()) and copied back, the loss arithmetic, and
      the backward into the dense (R, K, P) and (R, K) gradients, d_prob injected as sum(prob * d_prob).  The host
      round trip cannot be captured, so it is timed eagerly and both forms of the chain are compared with that.
  (b) sd_mask_loss_bwd alone against the new mask backward with a d_prob, as graphs: the ratio.  The new one reads
      4 R P more bytes (d_prob) on 4 R K P written.
The mask backward's algorithmic bytes are 4 R K P (the gradient, written once) + 12 R P (the selected planes, their
targets and d_prob, read once) + 4 R (the classes); reported as a fraction of 8 TB/s.
Also stored: the worst k_gpu and the k_ref there of tests/test_msrcnn_head.py's margin over its cases.

    python tools/msrcnn_head_time.py [--iters 50] [--sets 3] [--out profiles/msrcnn_head_time.json]
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
from tests import msrcnn_ref as mr  # noqa: E402
from tools.mask_loss_time import graphs_of, time_events  # noqa: E402

PEAK = 8.0e12
SHAPES = (("b2", (256, 81, 784)), ("b1", (128, 81, 784)), ("b8", (1024, 81, 784)))
SCALE = 1.0


def torch_chain(logits, iou_pred, cls, target, ratio, d_prob):
    """the reference's two subgraphs, forward + autograd backward; returns (mask_loss, iou_loss, d_logits, d_iou_pred)"""
    R = logits.shape[0]
    rows = torch.arange(R, device=logits.device)
    idx = cls.long()
    picked = logits[rows, idx]
    prob = torch.sigmoid(picked)
    on = target != -1.0
    per = torch.nn.functional.binary_cross_entropy_with_logits(picked, target.clamp(min=0.0), reduction="none")
    mask_loss = (per * on).sum() / (on.sum() + 1e-5) * SCALE
    p = iou_pred[rows, idx]
    # the CustomOp: four copies to the host, numpy, two copies back
    it, w = mr.maskiou_compute(prob.detach().cpu().numpy(), target.cpu().numpy(), ratio.cpu().numpy(),
                               cls.cpu().numpy())
    it, w = torch.from_numpy(it).to(logits.device), torch.from_numpy(w).to(logits.device)
    iou_loss = 0.5 * (((it - p) ** 2) * w).sum() / torch.clamp(w.sum(), min=1.0)
    d_logits, d_iou = torch.autograd.grad(mask_loss + iou_loss + (prob * d_prob).sum(), [logits, iou_pred])
    return mask_loss / SCALE, iou_loss, d_logits, d_iou


def k_margin():
    """per output: the worst k of the GPU over the cases of tests/test_msrcnn_head.py and the restatement's k there"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    worst = {o: dict(k_gpu=0.0, k_ref_there=0.0, case=None) for o in ("prob", "d_logits", "loss", "d_iou_pred")}

    def note(o, name, k, kr):
        if k >= worst[o]["k_gpu"] and np.isfinite(kr):
            worst[o].update(k_gpu=k, k_ref_there=kr, case=name)
    for P in mr.PS:
        for R in mr.RS:
            for v in mr.VARIANTS:
                c = mr.make_case(R, P, v)
                name = "R%d-P%d-v%d" % (R, P, v)
                t = {k: cu(c[k]) for k in ("logits", "cls", "target", "ratio", "iou_pred", "d_prob")}
                _, _, prob = ops.msrcnn_mask_loss_forward(t["logits"], t["cls"], t["target"])
                it, w, loss, wsum = ops.maskiou_loss_forward(t["iou_pred"], prob, t["target"], t["ratio"], t["cls"])
                di = ops.maskiou_loss_backward(t["iou_pred"], t["cls"], it, w, wsum, c["scale"])
                d = ops.msrcnn_mask_loss_backward(t["logits"], t["cls"], t["target"], t["d_prob"], c["scale"])
                pl = mr.planes(c["cls"], mr.K)
                sel = np.zeros((R, mr.K), bool)
                sel[np.arange(R)[pl >= 0], pl[pl >= 0]] = True
                dense = np.where(sel[:, :, None], d.cpu().numpy(), 0).sum(axis=1)
                truth, T = mr.mask_truth(c["logits"], c["cls"], c["target"], c["d_prob"], c["scale"])
                kr = mr.mask_k_ref(c["logits"], c["cls"], c["target"], c["d_prob"], c["scale"])
                note("prob", name, mr.k_of(prob.cpu().numpy(), truth["prob"], T["prob"]), kr["prob"])
                note("d_logits", name, mr.k_of(dense, truth["d"], T["d"]), kr["d"])
                ith, wh = it.cpu().numpy(), w.cpu().numpy()
                truth, T = mr.loss_truth(c["iou_pred"], c["cls"], ith, wh, c["scale"])
                kr = mr.loss_k_ref(c["iou_pred"], c["cls"], ith, wh, c["scale"])
                note("loss", name, mr.k_of(loss.cpu().numpy(), truth["loss"], T["loss"]), kr["loss"])
                note("d_iou_pred", name, mr.k_of(di.cpu().numpy(), truth["d"], T["d"]), kr["d"])
    return {o: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in w.items()} for o, w in worst.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msrcnn_head_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for name, (R, K, P) in SHAPES:
        rnd = lambda *s: torch.randn(s, device="cuda", generator=gen)
        lgs = [rnd(R, K, P) * 3.0 for _ in range(nsets)]
        cls = torch.randint(0, K, (R,), device="cuda", generator=gen).float()
        tgs = [torch.randint(-1, 2, (R, P), device="cuda", generator=gen).float() for _ in range(nsets)]
        ratio = torch.rand(R, device="cuda", generator=gen) * 0.8 + 0.2
        ips = [rnd(R, K) for _ in range(nsets)]
        dps = [rnd(R, P) for _ in range(nsets)]
        one = lambda: torch.empty(1, device="cuda")
        out, cs, loss, wsum = one(), one(), one(), one()
        prob, it, w = torch.empty((R, P), device="cuda"), torch.empty(R, device="cuda"), torch.empty(R, device="cuda")
        d, d_ml, di = torch.empty((R, K, P), device="cuda"), torch.empty((R, K, P), device="cuda"), torch.empty((R, K), device="cuda")
        u8 = lambda n: torch.empty(n, device="cuda", dtype=torch.uint8)
        ws = [u8(ops.msrcnn_mask_loss_workspace_bytes(R, K, P)), u8(ops.maskiou_loss_workspace_bytes(R, K, P)),
              u8(ops.msrcnn_mask_loss_workspace_bytes(R, K, P)), u8(ops.mask_loss_workspace_bytes(R, K, P))]

        def mask_fwd(i):
            ops.msrcnn_mask_loss_forward(lgs[i], cls, tgs[i], out=out, count_sum=cs, prob=prob, workspace=ws[0])

        def iou_fwd(i):
            ops.maskiou_loss_forward(ips[i], prob, tgs[i], ratio, cls, iou_target=it, weight=w, loss=loss,
                                     weight_sum=wsum, workspace=ws[1])

        def iou_bwd(i):
            ops.maskiou_loss_backward(ips[i], cls, it, w, wsum, 1.0, d_iou_pred=di)

        def mask_bwd(i):
            ops.msrcnn_mask_loss_backward(lgs[i], cls, tgs[i], dps[i], SCALE, d_logits=d, workspace=ws[2])

        def old_bwd(i):
            ops.mask_loss_backward(lgs[i], cls, tgs[i], SCALE, d_logits=d_ml, workspace=ws[3])

        def chain(i):
            mask_fwd(i)
            iou_fwd(i)
            iou_bwd(i)
            mask_bwd(i)
        bwd_bytes = 4 * R * K * P + 12 * R * P + 4 * R
        r = dict(shape=[R, K, P], mask_bwd_algorithmic_bytes=bwd_bytes)
        chain(0)
        for key, fn in (("mask_fwd", mask_fwd), ("maskiou_fwd", iou_fwd), ("maskiou_bwd", iou_bwd),
                        ("mask_bwd_with_d_prob", mask_bwd), ("sd_mask_loss_bwd", old_bwd), ("chain", chain)):
            e = time_events(fn, args.iters, nsets)
            gs = graphs_of(fn, nsets)
            g_us = time_events(lambda i: gs[i].replay(), args.iters, nsets)
            del gs
            r[key] = dict(eager_us=round(e, 1), graph_us=round(g_us, 1))
        nb, ob = r["mask_bwd_with_d_prob"], r["sd_mask_loss_bwd"]
        nb["fraction_of_8TBps"] = round(bwd_bytes / PEAK * 1e6 / nb["graph_us"], 3)
        r["mask_bwd_ratio_new_over_sd_mask_loss_bwd"] = dict(graph=round(nb["graph_us"] / ob["graph_us"], 3),
                                                             eager=round(nb["eager_us"] / ob["eager_us"], 3))
        # (a) the torch composition with the host round trip, eager
        lgr = [lg.clone().requires_grad_() for lg in lgs]
        ipr = [ip.clone().requires_grad_() for ip in ips]

        def torch_fn(i):
            torch_chain(lgr[i], ipr[i], cls, tgs[i], ratio, dps[i])
        r["torch_composition"] = dict(eager_us=round(time_events(torch_fn, args.iters, nsets), 1), graph_us=None,
                                      graph_error="the MaskIoU target is computed on the host: not capturable")
        chain(0)
        tm, ti, tdl, tdi = torch_chain(lgr[0], ipr[0], cls, tgs[0], ratio, dps[0])
        r["max_abs_diff_vs_torch"] = dict(mask_loss=float((out[0] - tm).abs()), iou_loss=float((loss[0] - ti).abs()),
                                          d_logits=float((d - tdl).abs().max()), d_iou_pred=float((di - tdi).abs().max()))
        t_us = r["torch_composition"]["eager_us"]
        r["not_slower_than_torch"] = dict(chain_eager=r["chain"]["eager_us"] <= t_us,
                                          chain_graph=r["chain"]["graph_us"] <= t_us)
        r["speedup_over_torch"] = dict(chain_eager=round(t_us / r["chain"]["eager_us"], 2),
                                       chain_graph=round(t_us / r["chain"]["graph_us"], 2))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del lgs, tgs, lgr, ipr, d, d_ml, dps
        torch.cuda.empty_cache()
    res["margin"] = k_margin()
    res["config"] = dict(input_sets=nsets, iters=args.iters, grad_scale=SCALE)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"msrcnn_head": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"msrcnn_head": res["margin"]}))


if __name__ == "__main__":
    main()
