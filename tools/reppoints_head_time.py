#!/usr/bin/env python
"""RepPoints training head timing (simpledet_amd/csrc/reppoints_head.hip) at the shape of
config/RepPoints/reppoints_moment_r50v1_fpn_1x.py: N = 2 images, M = 100 gt rows, 800 x 1333 (P = 22300 over strides
8..128), nine points, the moment and the minmax transform; secondary shapes N = 1 and M = 8.

Timed from device events, eagerly and as one captured HIP graph: the targets, the loss forward, the loss backward and
the chain targets -> forward -> backward.  In the same run, on the same inputs, a torch composition of what the
reference's graph does (models/RepPoints/builder.py:311-484): per image the (M, P) distance matrix with its masks and
top-k and the (P, M) IoU matrix with its maxima, per level the transpose / reshape / flip / tile and the concat, the
two smooth-L1 chains and the autograd backward into per-level gradients.  The parent commit has no RepPoints head,
so this is the baseline; the expectation is that no measured shape is slower than it.
Algorithmic bytes: targets 72 N P of point maps + 20 N M of gt rows read, 40 N P written; loss forward 144 N P + 40 N P
read, 32 N P written; loss backward the forward's reads + 144 N P written; reported as a fraction of 8 TB/s -- a
ratio of algorithmic bytes to the HBM peak, not an HBM rate: the rotated sets fit the Infinity Cache
(`fits_infinity_cache`).  NSETS input sets are rotated between calls.  Also stored: k_ref / k_gpu of
tests/test_reppoints_head.py's margin.

    python tools/reppoints_head_time.py [--iters 50] [--sets 3] [--out profiles/reppoints_head_time.json]
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
from tests import reppoints_ref as rr  # noqa: E402

PEAK = 8.0e12
DATA_SIZE, STRIDES, K = (800, 1333), rr.STRIDES, 9
SHAPES = (("config", 2, 100, "moment"), ("config_minmax", 2, 100, "minmax"), ("n1", 1, 100, "moment"), ("m8", 2, 8, "moment"))
TARGET_KW = dict(target_scale=4, num_pos=1, pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0)


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
    try:
        gs = graphs_of(fn, nsets)
        g = round(time_events(lambda i: gs[i].replay(), iters, nsets), 1)
        del gs
        return dict(eager_us=round(e, 1), graph_us=g)
    except Exception as ex:    # a composition that cannot be captured is compared eagerly
        torch.cuda.synchronize()
        return dict(eager_us=round(e, 1), graph_us=None, graph_error=str(ex).splitlines()[0][:200])


# ------------------------------------------------------------ the reference's graph as a torch composition --
def torch_points(sizes, strides, dev):
    return torch.from_numpy(rr.gen_points(sizes, strides)).to(dev)


def torch_points2bbox(pts, transform, mt, y_first):
    """_points2bbox on (..., 2K)"""
    v = pts.reshape(pts.shape[:-1] + (-1, 2))
    y, x = (v[..., 0], v[..., 1]) if y_first else (v[..., 1], v[..., 0])
    if transform == "minmax":
        return torch.stack([x.amin(-1), y.amin(-1), x.amax(-1), y.amax(-1)], -1)
    xm, ym = x.mean(-1, keepdim=True), y.mean(-1, keepdim=True)
    xs, ys = ((x - xm) ** 2).mean(-1, keepdim=True).sqrt(), ((y - ym) ** 2).mean(-1, keepdim=True).sqrt()
    hw, hh = xs * mt[0:1].exp(), ys * mt[1:2].exp()
    return torch.cat([xm - hw, ym - hh, xm + hw, ym + hh], -1)


def torch_point_assign(points, gt, scale, num_pos):
    """_point_assign with its (M, P) matrices; the two top-k over M of the reference are one min here"""
    plvl = points[:, 2].log2().floor()
    l, t, r, b, cls = gt.unbind(1)
    gxy = torch.stack([(l + r) / 2, (t + b) / 2], -1)
    gwh = torch.stack([(r - l).clamp(min=1e-6), (b - t).clamp(min=1e-6)], -1)
    lvl = ((gwh[:, 0] / scale).log2() + (gwh[:, 1] / scale).log2()).div(2).floor()
    lvl = torch.maximum(torch.minimum(lvl, plvl.max()), plvl.min())
    d = ((points[None, :, :2] - gxy[:, None]) / gwh[:, None]).norm(dim=-1)
    inf = torch.full_like(d, float("inf"))
    mask = (lvl[:, None] == plvl[None]).float() * (cls > 0).float()[:, None]
    d = torch.where(mask > 0, d, inf)
    top = torch.zeros_like(d).scatter_(1, d.topk(num_pos, dim=-1, largest=False).indices, 1.0)
    d = torch.where(top > 0, d, inf)
    mind, mini = d.min(dim=0)
    hit = mind < float("inf")
    return torch.where(hit, cls[mini], -torch.ones_like(mind)), torch.where(hit[:, None], gt[mini, :4], torch.zeros_like(gt[mini, :4]))


def torch_iou_assign(boxes, gt, pos, neg, minpos):
    a, g = boxes[:, None], gt[None, :, :4]
    w = (torch.minimum(a[..., 2], g[..., 2]) - torch.maximum(a[..., 0], g[..., 0])).clamp(min=0)
    h = (torch.minimum(a[..., 3], g[..., 3]) - torch.maximum(a[..., 1], g[..., 1])).clamp(min=0)
    i = w * h
    u = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1]) - i
    iou = torch.where(u <= 0, torch.zeros_like(i), i / u)
    mx, arg = iou.max(dim=1)
    col = iou.max(dim=0).values
    asg = -torch.ones_like(mx)
    asg = torch.where(mx < neg, torch.zeros_like(asg), asg)
    fg = ((iou == col[None]).float() * (col[None] > minpos).float()).sum(-1)
    asg = torch.where(fg > 0, torch.ones_like(asg), asg)
    asg = torch.where(mx >= pos, torch.ones_like(asg), asg)
    return torch.where(asg > 0, gt[arg, 4], asg), torch.where((asg > 0)[:, None], gt[arg, :4], torch.zeros_like(gt[arg, :4]))


def torch_targets(pts_init, gt, mt, points, centers, transform):
    boxes = []
    for pred, s, c in zip(pts_init, STRIDES, centers):
        b = torch_points2bbox(pred.permute(0, 2, 3, 1).reshape(pred.shape[0], -1, 2 * K), transform, mt, True) * s
        boxes.append(torch.cat([c, c], -1)[None] + b)
    boxes = torch.cat(boxes, 1)
    out = [[], [], [], []]
    for n in range(gt.shape[0]):
        a, b = torch_point_assign(points, gt[n], TARGET_KW["target_scale"], TARGET_KW["num_pos"])
        c, d = torch_iou_assign(boxes[n], gt[n], TARGET_KW["pos_iou_thr"], TARGET_KW["neg_iou_thr"], TARGET_KW["min_pos_iou"])
        for lst, v in zip(out, (a, b, c, d)):
            lst.append(v)
    return [torch.stack(v) for v in out]


def torch_losses(pts_init, pts_refine, mt, tg, centers, term, transform):
    """builder.py:415-481: returns sum(loss_init * 0.5 / norm) + sum(loss_refine / norm) and the two losses"""
    total, losses = 0.0, []
    for maps, lab, gtb, gs in ((pts_init, tg[0], tg[1], 0.5), (pts_refine, tg[2], tg[3], 1.0)):
        lv = []
        for pred, s, c in zip(maps, STRIDES, centers):
            v = pred.permute(0, 2, 3, 1).reshape(pred.shape[0], -1, K, 2).flip(3).reshape(pred.shape[0], -1, 2 * K)
            lv.append(v * s + c.tile(1, K)[None])
        box = torch_points2bbox(torch.cat(lv, 1).reshape(-1, 2 * K), transform, mt, False).reshape(lab.shape + (4,))
        r = (box - gtb) / term
        ar = r.abs()
        loss = torch.where(ar > 1.0 / 9, ar - 0.5 / 9, 4.5 * r * r) * (lab > 0).float()[..., None]
        losses.append(loss)
        total = total + (loss / ((lab >= 1).sum() + 1.0)).sum() * gs
    return total, losses


def k_margin():
    """the margins of tests/test_reppoints_head.py on its own cases"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = {key: dict(k_ref=0.0, k_gpu=0.0) for key in ("forward", "gradients", "d_moment_transfer")}
    for name, c in rr.loss_cases():
        tg = rr.targets_f32(c)
        truth, r32 = rr.losses_truth(c, tg), rr.losses_f32(c, tg)
        pi, pr, mt = [cu(p) for p in c["pts_init"]], [cu(p) for p in c["pts_refine"]], cu(c["mt"])
        t = ops.reppoints_target(pi, cu(c["gt_bbox"]), c["strides"], transform=c["transform"], moment_transfer=mt,
                                 target_scale=c["target_scale"], num_pos=c["num_pos"], pos_iou_thr=c["pos_iou_thr"],
                                 neg_iou_thr=c["neg_iou_thr"], min_pos_iou=c["min_pos_iou"])
        kw = dict(transform=c["transform"], moment_transfer=mt, scale=c["scale"])
        li, lr = ops.reppoints_box_loss_forward(pi, pr, t, c["strides"], **kw)
        di, dr, dmt = ops.reppoints_box_loss_backward(pi, pr, t, c["strides"], **kw)
        got = dict(loss_init=li.cpu().numpy(), loss_refine=lr.cpu().numpy(), d_init=[d.cpu().numpy() for d in di],
                   d_refine=[d.cpu().numpy() for d in dr], d_mt=dmt.cpu().numpy())
        for res, key in ((r32, "k_ref"), (got, "k_gpu")):
            for name_, k in zip(("forward", "gradients", "d_moment_transfer"), rr.k_all(res, truth)):
                out[name_][key] = round(max(out[name_][key], k), 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reppoints_head_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    sizes = rr.level_sizes(DATA_SIZE, STRIDES)
    P = sum(a * b for a, b in sizes)
    points = torch_points(sizes, STRIDES, "cuda")
    centers = [torch_points([sz], [s], "cuda")[:, :2] for sz, s in zip(sizes, STRIDES)]
    term = torch.cat([torch.full((a * b, 4), float(s), device="cuda") for (a, b), s in zip(sizes, STRIDES)])[None] * 4
    res = dict(event_floor_us=round(time_events(lambda i: None, args.iters, 1), 1))
    for name, N, M, transform in SHAPES:
        rs = np.random.RandomState(7)
        gts = [torch.from_numpy(rr._boxes(rs, N, M, DATA_SIZE, [M * 6 // 10] * N)).cuda() for _ in range(nsets)]
        gen = torch.Generator(device="cuda").manual_seed(1)
        mk = lambda scale: [[torch.randn((N, 2 * K, a, b), device="cuda", generator=gen) * scale for a, b in sizes]
                            for _ in range(nsets)]
        pi = mk(1.5)
        pr = [[a + b for a, b in zip(x, y)] for x, y in zip(pi, mk(0.5))]
        mt = torch.tensor([0.1, -0.1], device="cuda")
        E = lambda *shape, dt=torch.float32: torch.empty(shape, device="cuda", dtype=dt)
        tb = dict(label_init=E(N, P), gt_init=E(N, P, 4), label_refine=E(N, P), gt_refine=E(N, P, 4),
                  state=E(4, dt=torch.int32), workspace=E(ops.reppoints_target_workspace_bytes(N, M, P), dt=torch.uint8))
        lo = dict(loss_init=E(N, P, 4), loss_refine=E(N, P, 4))
        gb = dict(d_init=[torch.empty_like(t) for t in pi[0]], d_refine=[torch.empty_like(t) for t in pi[0]],
                  d_moment_transfer=E(2), workspace=E(ops.reppoints_box_loss_workspace_bytes(N, P), dt=torch.uint8))
        kw = dict(transform=transform, moment_transfer=mt)
        tg = ops.reppoints_target(pi[0], gts[0], STRIDES, **kw, **TARGET_KW, **tb)

        def target(i):
            ops.reppoints_target(pi[i], gts[i], STRIDES, **kw, **TARGET_KW, **tb)

        def fwd(i):
            ops.reppoints_box_loss_forward(pi[i], pr[i], tg, STRIDES, **kw, **lo)

        def bwd(i):
            ops.reppoints_box_loss_backward(pi[i], pr[i], tg, STRIDES, **kw, **gb)

        def chain(i):
            target(i); fwd(i); bwd(i)
        bytes_ = dict(target=72 * N * P + 20 * N * M + 40 * N * P, fwd=144 * N * P + 40 * N * P + 32 * N * P,
                      bwd=144 * N * P + 40 * N * P + 144 * N * P)
        rotated = 144 * N * P * (nsets + 1) + 72 * N * P
        r = dict(shape=dict(N=N, M=M, P=P, num_points=K, transform=transform, data_size=list(DATA_SIZE)),
                 algorithmic_bytes=bytes_, rotated_working_set_bytes=rotated, fits_infinity_cache=rotated < 256 << 20)
        for key, fn in (("target", target), ("fwd", fwd), ("bwd", bwd), ("chain", chain)):
            r[key] = both_ways(fn, args.iters, nsets)
        for key in ("target", "fwd", "bwd"):
            r[key]["fraction_of_8TBps"] = round(bytes_[key] / PEAK * 1e6 / r[key]["graph_us"], 4)
        # the baseline: the reference's graph as a torch composition
        req = [([t.clone().requires_grad_() for t in pi[i]], [t.clone().requires_grad_() for t in pr[i]]) for i in range(nsets)]
        mtr = mt.clone().requires_grad_()

        def t_target(i):
            with torch.no_grad():
                return torch_targets(pi[i], gts[i], mt, points, centers, transform)
        tg0 = t_target(0)

        def t_fwd(i):
            with torch.no_grad():
                return torch_losses(pi[i], pr[i], mt, tg0, centers, term, transform)

        def t_fwd_bwd(i, tgt=None):
            total, _ = torch_losses(req[i][0], req[i][1], mtr, tgt or tg0, centers, term, transform)
            torch.autograd.grad(total, req[i][0] + req[i][1] + ([mtr] if transform == "moment" else []))

        def t_chain(i):
            t_fwd_bwd(i, t_target(i))
        r["torch_composition"] = {key: both_ways(fn, max(10, args.iters // 2), nsets)
                                  for key, fn in (("target", t_target), ("fwd", t_fwd), ("fwd_bwd", t_fwd_bwd), ("chain", t_chain))}
        # the results agree (ties and last-ulp IoUs aside): labels that differ, losses up to rounding
        target(0); fwd(0)
        _, tl = t_fwd(0)
        same_t = ops.RepPointsTargets(tg0[0], tg0[1], tg0[2], tg0[3], tg.state)
        r["vs_torch"] = dict(label_init_differ=int((tb["label_init"] != tg0[0]).sum()),
                             label_refine_differ=int((tb["label_refine"] != tg0[2]).sum()),
                             loss_max_abs_diff=float(max((a - b).abs().max() for a, b in zip(
                                 ops.reppoints_box_loss_forward(pi[0], pr[0], same_t, STRIDES, **kw), tl))))
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
        del pi, pr, req
        torch.cuda.empty_cache()
    res["margin"] = k_margin()
    res["run"] = dict(input_sets=nsets, iters=args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"reppoints_head": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"reppoints_head": res["margin"]}))


if __name__ == "__main__":
    main()
