#!/usr/bin/env python
"""FCOS training head timing (simpledet_amd/csrc/fcos_head.hip) at the shape of config/fcos_r50v1_fpn_1x.py:
N = 2 images, M = 100 gt rows, data_size 800 x 1333 (HW = 22300 over strides 8..128), K = 80; secondary shapes
N = 1 and M = 8.

Timed from device events, eagerly and as one captured HIP graph: the targets, the loss forward, the loss backward and
the chain targets -> forward -> backward.  In the same run, on the same inputs, a torch composition of what the
reference's graphs do: make_fcos_gt with its (N, 4, M, HW) intermediates, the per-level reshape + concat of the
logits, the three losses and the autograd backward through the concat into per-level gradients.  The parent commit
has no FCOS head, so this is the baseline; the expectation is that no measured shape is slower than it.
Algorithmic bytes: targets 20 N M + 4 N HW (6 + K with the dense one-hot; the compact form is what the losses
read); loss backward 8 N (K + 5) HW for logits and gradients + 24 N HW of targets; reported as a fraction of
8 TB/s -- a ratio of algorithmic bytes to the HBM peak, not an HBM rate: the rotated sets fit the Infinity Cache
(`fits_infinity_cache`).  NSETS input sets are rotated between calls.  Also stored: k_ref / k_gpu of tests/test_fcos_head.py's margin.

    python tools/fcos_head_time.py [--iters 50] [--sets 3] [--out profiles/fcos_head_time.json]
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
from tests import fcos_ref as fr  # noqa: E402

PEAK = 8.0e12
DATA_SIZE, STRIDES, K = (800, 1333), fr.STRIDES, 80
SHAPES = (("config", 2, 100), ("n1", 1, 100), ("m8", 2, 8))


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


def event_floor(iters):
    """an empty interval between two events: the resolution every number below is read against"""
    return time_events(lambda i: None, iters, 1)


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
    try:
        gs = graphs_of(fn, nsets)
        g = round(time_events(lambda i: gs[i].replay(), iters, nsets), 1)
        del gs
        return dict(eager_us=round(e, 1), graph_us=g)
    except Exception as ex:    # a composition that cannot be captured is compared eagerly
        torch.cuda.synchronize()
        return dict(eager_us=round(e, 1), graph_us=None, graph_error=str(ex).splitlines()[0][:200])


def torch_grid(data_size, strides, dev):
    h, w = data_size
    lx, ly, lo, up = [], [], [], []
    for i, s in enumerate(strides):
        x = torch.arange(0, w, s, device=dev, dtype=torch.float32) + s / 2.
        y = torch.arange(0, h, s, device=dev, dtype=torch.float32) + s / 2.
        yy, xx = torch.meshgrid(y, x, indexing="ij")
        lx.append(xx.reshape(-1)); ly.append(yy.reshape(-1))
        lo.append(torch.full((xx.numel(),), fr.STAGE_LOWER[i], device=dev)); up.append(torch.full((xx.numel(),), fr.STAGE_UPPER[i], device=dev))
    return torch.cat(lx), torch.cat(ly), torch.cat(lo), torch.cat(up)


def torch_targets(gt, im_info, grid, num_classes, io=-1.0, il=-1.0):
    """make_fcos_gt, node for node (landscape grid; im_info stays on the device)"""
    loc_x, loc_y, lo, up = grid
    nonignore = ((loc_x < im_info[0, 1]) & (loc_y < im_info[0, 0])).float()
    l = loc_x - gt[:, :, 0:1]; t = loc_y - gt[:, :, 1:2]; r = gt[:, :, 2:3] - loc_x; b = gt[:, :, 3:4] - loc_y
    off = torch.stack([l, t, r, b], dim=1)
    inbox = (off.min(dim=1, keepdim=True).values >= 0).float()
    off = off * inbox + (1 - inbox) * io
    great = off.max(dim=1, keepdim=True).values
    stage = ((great >= lo) & (great < up)).float()
    off = off * stage + (1 - stage) * io
    size = (off[:, 0:1] + off[:, 2:3]) * (off[:, 1:2] + off[:, 3:4])
    size = size * stage + (1 - stage) * 1e10
    best = size.argmin(dim=2)
    off = torch.gather(off, 2, best.repeat(1, 4, 1)[:, :, None, :])[:, :, 0, :]
    inb = (off != io).float()
    lr, tb = torch.sort(off[:, 0:3:2], dim=1).values, torch.sort(off[:, 1:4:2], dim=1).values
    c = torch.sqrt(lr[:, 0] * tb[:, 0] / (lr[:, 1] * tb[:, 1])) * inb[:, 0]
    cls = torch.gather(gt[:, :, 4], 1, best[:, 0]) - 1
    hot = torch.nn.functional.one_hot(cls.clamp(min=0).long(), num_classes).float() * (cls >= 0).float()[..., None]
    cls_gt = hot.permute(0, 2, 1) * inb[:, 0:1]
    c = c * nonignore + (1 - nonignore) * il
    cls_gt = cls_gt * nonignore + (1 - nonignore) * il
    return c, cls_gt.reshape(gt.shape[0], -1), off


def torch_losses(cls_lv, ctr_lv, off_lv, c, labels, y, alpha=0.25, gamma=2.0, io=-1.0, il=-1.0):
    """builder.py:207-230 + loss.py: reshape / concat, the three losses; returns the three scalars"""
    cat = lambda lv, shape: torch.cat([v.reshape(v.shape[0], v.shape[1], -1) for v in lv], dim=2).reshape(shape)
    N = c.shape[0]
    logits, ctr, offp = cat(cls_lv, (N, -1)), cat(ctr_lv, (N, -1)), cat(off_lv, (N, 4, -1))
    mask = (labels != il).float()
    p = torch.sigmoid(logits)
    minus_log = -logits.clamp(min=0) - torch.log1p(torch.exp(-logits.abs()))
    norm = (labels * mask).sum() + 1
    cls_loss = (-(alpha * (1 - p) ** gamma * labels * torch.log(p.clamp(1e-5, 1))
                  + (1 - alpha) * p ** gamma * (1 - labels) * minus_log) * mask).sum() / norm
    mc = ((c != il) & (c > 0)).float()
    pc = torch.sigmoid(ctr)
    bce = -c * torch.log(pc.clamp(1e-5, 1)) - (1 - c) * torch.log((1 - pc).clamp(1e-5, 1))
    ctr_loss = (bce * mc).sum() / (mc.sum() + 1e-30)
    c3 = c[:, None, :]
    mi = ((y[:, 0:1] != io) & (c3 > 0)).float()
    x = offp.clamp(0, 1e4) * mi
    cm = c3 * mi
    ta = (y[:, 0:1] + y[:, 2:3]) * (y[:, 1:2] + y[:, 3:4])
    pa = (x[:, 0:1] + x[:, 2:3]) * (x[:, 1:2] + x[:, 3:4])
    wi = torch.minimum(x[:, 0:1], y[:, 0:1]) + torch.minimum(x[:, 2:3], y[:, 2:3])
    hi = torch.minimum(x[:, 3:4], y[:, 3:4]) + torch.minimum(x[:, 1:2], y[:, 1:2])
    ai = wi * hi
    off_loss = (-torch.log((ai + 1.0) / (ta + pa - ai + 1.0)) * cm).sum() / (cm.sum() + 1e-30)
    return ctr_loss, cls_loss, off_loss


def k_margin():
    """the margins of tests/test_fcos_head.py on its own cases: (k_ref, k_gpu) of the gradients and of the scalars"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = dict(gradients=dict(k_ref=0.0, k_gpu=0.0), scalars=dict(k_ref=0.0, k_gpu=0.0))

    def k(res, truth):
        return (max(fr.k_of(res[d], truth[d], truth["T" + d[1:]], truth["s" + d[1:]]) for d in ("d_cls", "d_ctr", "d_off")),
                fr.k_losses(res["losses"], truth))
    for name, c in fr.loss_cases():
        case, kw = c["case"], dict(alpha=c["alpha"], gamma=c["gamma"])
        truth = fr.losses_truth(c["cls"], c["ctr"], c["off"], c["tg"], **kw)
        r32 = fr.losses_f32(c["cls"], c["ctr"], c["off"], c["tg"], **kw)
        tg = ops.fcos_target(cu(case["gt_bbox"]), cu(case["im_info"]), case["data_size"], case["strides"], case["K"])
        lv = [[cu(c["cls"])], [cu(c["ctr"])], [cu(c["off"])]]
        got = dict(losses=ops.fcos_loss_forward(*lv, tg, **kw).cpu().numpy())
        for d, g in zip(("d_cls", "d_ctr", "d_off"), ops.fcos_loss_backward(*lv, tg, **kw)):
            got[d] = g[0].cpu().numpy()
        for res, key in ((r32, "k_ref"), (got, "k_gpu")):
            kg, ks = k(res, truth)
            out["gradients"][key] = round(max(out["gradients"][key], kg), 3)
            out["scalars"][key] = round(max(out["scalars"][key], ks), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcos_head_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    HW, hws = ops.fcos_num_locations(DATA_SIZE, STRIDES)
    sizes = fr.level_sizes(DATA_SIZE, STRIDES)
    grid = torch_grid(DATA_SIZE, STRIDES, "cuda")
    res = dict(event_floor_us=round(event_floor(args.iters), 1))
    for name, N, M in SHAPES:
        rs = np.random.RandomState(7)
        gts = [torch.from_numpy(fr._boxes(rs, N, M, DATA_SIZE[1], DATA_SIZE[0], K, None)).cuda() for _ in range(nsets)]
        info = torch.tensor([[800.0, 1333.0, 1.0]] * N, device="cuda")
        gen = torch.Generator(device="cuda").manual_seed(1)
        mk = lambda C, scale, shift: [[(torch.randn((N, C, a, b), device="cuda", generator=gen) * scale + shift)
                                       for a, b in sizes] for _ in range(nsets)]
        cls, ctr = mk(K, 2.0, -4.6), mk(1, 2.0, 0.0)
        off = [[v.exp() * 16 for v in lv] for lv in mk(4, 0.5, 0.0)]
        buf = dict(centerness=torch.empty(N, HW, device="cuda"), offset=torch.empty(N, 4, HW, device="cuda"),
                   cls_id=torch.empty(N, HW, device="cuda", dtype=torch.int32),
                   state=torch.empty(4, device="cuda", dtype=torch.int32),
                   workspace=torch.empty(ops.fcos_target_workspace_bytes(N, HW), device="cuda", dtype=torch.uint8))
        losses = torch.empty(3, device="cuda")
        ws = torch.empty(ops.fcos_loss_workspace_bytes(N, K, HW), device="cuda", dtype=torch.uint8)
        d = [[torch.empty_like(t) for t in lv] for lv in (cls[0], ctr[0], off[0])]
        tg = ops.fcos_target(gts[0], info, DATA_SIZE, STRIDES, K, **buf)

        def target(i):
            ops.fcos_target(gts[i], info, DATA_SIZE, STRIDES, K, **buf)

        def fwd(i):
            ops.fcos_loss_forward(cls[i], ctr[i], off[i], tg, losses=losses, workspace=ws)

        def bwd(i):
            ops.fcos_loss_backward(cls[i], ctr[i], off[i], tg, d_cls=d[0], d_ctr=d[1], d_off=d[2])

        def chain(i):
            target(i); fwd(i); bwd(i)
        target_bytes, bwd_bytes = 20 * N * M + 24 * N * HW, 8 * N * (K + 5) * HW + 24 * N * HW
        # the rotated logits and the one set of gradients stay far below the 256 MB Infinity Cache: the "fraction of
        # 8 TB/s" below relates algorithmic bytes to the HBM peak, it is NOT a measured HBM rate
        rotated = 4 * N * (K + 5) * HW * (nsets + 1)
        r = dict(shape=dict(N=N, M=M, K=K, HW=HW, data_size=list(DATA_SIZE)), target_algorithmic_bytes=target_bytes,
                 bwd_algorithmic_bytes=bwd_bytes, rotated_working_set_bytes=rotated,
                 fits_infinity_cache=rotated < 256 << 20)
        for key, fn in (("target", target), ("fwd", fwd), ("bwd", bwd), ("chain", chain)):
            r[key] = both_ways(fn, args.iters, nsets)
        r["target"]["fraction_of_8TBps"] = round(target_bytes / PEAK * 1e6 / r["target"]["graph_us"], 4)
        r["bwd"]["fraction_of_8TBps"] = round(bwd_bytes / PEAK * 1e6 / r["bwd"]["graph_us"], 4)
        # the baseline: the reference's graphs as a torch composition, concat included
        req = [[[t.clone().requires_grad_() for t in lv] for lv in (cls[i], ctr[i], off[i])] for i in range(nsets)]

        def t_target(i):
            return torch_targets(gts[i], info, grid, K)
        c0, lab0, y0 = t_target(0)

        def t_fwd(i):
            return torch_losses(*req[i], c0, lab0, y0)

        def t_fwd_bwd(i):
            torch.autograd.grad(sum(t_fwd(i)), [t for lv in req[i] for t in lv])

        def t_chain(i):
            c, lab, y = t_target(i)
            torch.autograd.grad(sum(torch_losses(*req[i], c, lab, y)), [t for lv in req[i] for t in lv])
        r["torch_composition"] = {key: both_ways(fn, max(10, args.iters // 2), nsets)
                                  for key, fn in (("target", t_target), ("fwd", t_fwd), ("fwd_bwd", t_fwd_bwd), ("chain", t_chain))}
        # the results agree: same targets where finite, same losses up to rounding
        target(0); fwd(0)
        tl = torch.stack(t_fwd(0)).detach()
        r["max_abs_diff_vs_torch"] = dict(losses=float((losses - tl).abs().max()),
                                          centerness=float((buf["centerness"] - c0).abs().max()))
        tc = r["torch_composition"]
        pick = lambda t: t["graph_us"] if t["graph_us"] is not None else t["eager_us"]
        r["not_slower_than_torch"] = dict(
            target_eager=r["target"]["eager_us"] <= tc["target"]["eager_us"], target_graph=r["target"]["graph_us"] <= pick(tc["target"]),
            fwd_eager=r["fwd"]["eager_us"] <= tc["fwd"]["eager_us"], fwd_graph=r["fwd"]["graph_us"] <= pick(tc["fwd"]),
            fwd_bwd_eager=r["fwd"]["eager_us"] + r["bwd"]["eager_us"] <= tc["fwd_bwd"]["eager_us"],
            fwd_bwd_graph=r["fwd"]["graph_us"] + r["bwd"]["graph_us"] <= pick(tc["fwd_bwd"]),
            chain_eager=r["chain"]["eager_us"] <= tc["chain"]["eager_us"], chain_graph=r["chain"]["graph_us"] <= pick(tc["chain"]))
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del cls, ctr, off, req, d
        torch.cuda.empty_cache()
    res["margin"] = k_margin()
    res["run"] = dict(input_sets=nsets, iters=args.iters)     # (not "config": that key is the main shape)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"fcos_head": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"fcos_head": res["margin"]}))


if __name__ == "__main__":
    main()
