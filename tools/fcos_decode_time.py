#!/usr/bin/env python
"""FCOS test-time decode timing (simpledet_amd/csrc/fcos_decode.hip) at the shape of config/fcos_r50v1_fpn_1x.py:
N = 1 and 2 images, C = 80, strides 8..128 on 800 x 1333 (1.78 M scores per image over five levels), top_n 1000,
thresh 0.05.

Timed from device events, eagerly and as one captured HIP graph, with input_logits 0 (probabilities in, the CustomOps'
contract) and 1 (raw logits, the ten sigmoid nodes fused).  In the same run, on the same inputs, a torch composition
of the reference's steps (models/FCOS/builder.py:234-259, models/FCOS/utils.py): sigmoid, compare / sum with the
`.item()` decision and the im_info read-back per image and level left in as the reference has them, topk or nonzero,
gather, clamp, the mask, concat, argsort, gather and the scatter into (N, R, 81).  It cannot be captured (it reads the
host), so it is timed eagerly; the parent commit has no device decode, so this is the baseline.  The expectation is that
the device call as a graph is not slower than it at any measured shape.

Two score distributions: `dense` (class logits ~ N(-3, 1.5^2): every level takes the top-k branch) and `sparse`
(~ N(-6, 1): the smaller levels take the nonzero branch; the JSON lists the branch of every level).  NSETS input sets
are rotated between calls; medians over --iters calls after a warm-up; the event floor is stored next to them.

    python tools/fcos_decode_time.py [--iters 50] [--sets 3] [--out profiles/fcos_decode_time.json]
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

SIZES = ((100, 167), (50, 84), (25, 42), (13, 21), (7, 11))
STRIDES = (8, 16, 32, 64, 128)
C, TOP_N, THRESH = 80, 1000, 0.05
DISTRIBUTIONS = (("dense", -3.0, 1.5), ("sparse", -6.0, 1.0))


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


def torch_decode(cls_l, ctr_l, off_l, info, logits):
    """the reference's steps, host decisions included"""
    stages = []
    for cls, ctr, off, s in zip(cls_l, ctr_l, off_l, STRIDES):
        if logits:
            cls, ctr = torch.sigmoid(cls), torch.sigmoid(ctr)
        cand = cls > THRESH
        fused = cls * ctr
        N, _, H, W = cls.shape
        res = torch.full((N, TOP_N, 6), -1.0, device=cls.device)
        for i in range(N):
            img_h, img_w, _ = info[i].tolist()
            flat = fused[i].reshape(-1)
            if cand[i].sum().item() >= TOP_N:
                score, idx = torch.topk(flat, TOP_N)
            else:
                idx = torch.nonzero(cand[i].reshape(-1))[:, 0]
                if idx.numel() == 0:
                    continue
                score = flat[idx]
            x, y, c = idx % W, idx // W % H, idx // (W * H) + 1
            cx, cy = x.float() * s + s / 2, y.float() * s + s / 2
            o, hw = off[i].reshape(4, -1), y * W + x
            box = torch.stack([c.float(), score, (cx - o[0, hw]).clamp(0, img_w), (cy - o[1, hw]).clamp(0, img_h),
                               (cx + o[2, hw]).clamp(0, img_w), (cy + o[3, hw]).clamp(0, img_h)], dim=1)
            small = ((box[:, 0] >= box[:, 2]) & (box[:, 1] >= box[:, 3]))[:, None]
            res[i, :box.shape[0]] = torch.where(small, torch.full_like(box, -1.0), box)
        stages.append(res)
    st = torch.cat(stages, dim=1)
    N, R = st.shape[:2]
    order = torch.argsort(st[:, :, 1], dim=1, descending=True, stable=True)
    rows = torch.gather(st, 1, order[:, :, None].expand(-1, -1, 6))
    score = torch.zeros((N, R, 81), device=st.device)
    col = torch.remainder(rows[:, :, 0].long(), 81)
    score.scatter_(2, col[:, :, None], rows[:, :, 1].clamp(1e-20, 1).sqrt()[:, :, None])
    return rows[:, :, 2:], score, rows[:, :, 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fcos_decode_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    res = dict(event_floor_us=round(time_events(lambda i: None, args.iters, 1), 1),
               shape=dict(C=C, top_n=TOP_N, thresh=THRESH, strides=list(STRIDES), sizes=[list(s) for s in SIZES],
                          scores_per_image=C * sum(h * w for h, w in SIZES)))
    hws = [h * w for h, w in SIZES]
    for dist, mean, sigma in DISTRIBUTIONS:
        for N in (1, 2):
            gen = torch.Generator(device="cuda").manual_seed(11 + N)
            R = len(SIZES) * TOP_N
            mk = lambda ch, sc, sh: [[torch.randn((N, ch, h, w), device="cuda", generator=gen) * sc + sh
                                      for h, w in SIZES] for _ in range(nsets)]
            lcls, lctr = mk(C, sigma, mean), mk(1, 1.0, 1.0)
            off = [[(v * 2.5).exp() for v in lv] for lv in mk(4, 0.5, 1.0)]
            pcls = [[ops.fcos_sigmoid(v) for v in lv] for lv in lcls]
            pctr = [[ops.fcos_sigmoid(v) for v in lv] for lv in lctr]
            info = torch.tensor([[800.0, 1333.0, 1.0]] * N, device="cuda")
            buf = dict(bbox=torch.empty(N, R, 4, device="cuda"), score=torch.empty(N, R, 81, device="cuda"),
                       cls_id=torch.empty(N, R, device="cuda"),
                       workspace=torch.empty(ops.fcos_decode_workspace_bytes(N, C, hws, TOP_N), device="cuda",
                                             dtype=torch.uint8))
            r = dict(N=N, R=R, workspace_bytes=int(buf["workspace"].numel()),
                     input_bytes_per_call=4 * N * (C + 5) * sum(hws), output_bytes_per_call=4 * N * R * 86)
            counts = [[int((v[i] > THRESH).sum()) for v in pcls[0]] for i in range(N)]
            r["candidates_per_level_set0"] = counts
            r["branch_per_level_set0"] = [["topk" if n >= TOP_N else "nonzero" if n else "empty" for n in img]
                                          for img in counts]
            for logits, cl, ct in ((0, pcls, pctr), (1, lcls, lctr)):
                def dev(i, cl=cl, ct=ct, logits=logits):
                    ops.fcos_decode(cl[i], ct[i], off[i], info, STRIDES, TOP_N, THRESH, input_logits=bool(logits), **buf)

                def ref(i, cl=cl, ct=ct, logits=logits):
                    return torch_decode(cl[i], ct[i], off[i], info, logits)
                e = time_events(dev, args.iters, nsets)
                gs = graphs_of(dev, nsets)
                g = time_events(lambda i: gs[i].replay(), args.iters, nsets)
                del gs
                t = time_events(ref, max(10, args.iters // 2), nsets)
                # the two agree: same rows wherever no two scores tie
                dev(0)
                tb, ts, tc = ref(0)
                same = float((buf["cls_id"] == tc).float().mean())
                r["input_logits_%d" % logits] = dict(
                    eager_us=round(e, 1), graph_us=round(g, 1), torch_composition_eager_us=round(t, 1),
                    torch_composition_graph_us=None, torch_composition_graph_error="reads the host (.item(), .tolist())",
                    graph_not_slower_than_torch=bool(g <= t), eager_not_slower_than_torch=bool(e <= t),
                    rows_with_the_same_cls_id_as_torch=round(same, 6),
                    max_abs_bbox_diff_vs_torch=float((buf["bbox"] - tb).abs().max()),
                    max_abs_score_diff_vs_torch=float((buf["score"] - ts).abs().max()))
            res["%s_n%d" % (dist, N)] = r
            print(dist, N, json.dumps(r), flush=True)
            del lcls, lctr, off, pcls, pctr, buf
            torch.cuda.empty_cache()
    res["run"] = dict(input_sets=nsets, iters=args.iters, timer="device events, median",
                      distributions={d: dict(cls_logit_mean=m, cls_logit_sigma=s) for d, m, s in DISTRIBUTIONS})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"fcos_decode": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"fcos_decode": {k: {m: v[m]["graph_us"] for m in ("input_logits_0", "input_logits_1")}
                                      for k, v in res.items() if isinstance(v, dict) and "N" in v}}))


if __name__ == "__main__":
    main()
