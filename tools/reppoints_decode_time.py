#!/usr/bin/env python
"""RepPoints test-time decode timing (simpledet_amd/csrc/reppoints_decode.hip) at the shape of
config/RepPoints/reppoints_moment_r50v1_fpn_1x.py: N = 1 (the config's test batch) and 2 images, C = 80, nine points,
the moment transform, strides 8..128 on 800 x 1333 (22,300 locations per image over five levels), pre_nms_top_n 1000:
R = 3 x 1000 + 273 + 77 = 3,350 rows.

Timed from device events, eagerly and as one captured HIP graph, with probabilities in (input_logits 0) and raw logits
in (1, the sigmoid fused).  In the same run, on the same inputs, a torch composition of the reference's own steps
(models/RepPoints/builder.py:486-576): per level transpose / reshape, sigmoid, max, topk, _points2bbox, per image the
takes, scale, add and clips, stack, the padded column; then the concat of the levels.  It reads nothing back, so it is
timed eagerly AND as a captured graph; the parent commit has no device decode, so this is the baseline.  The house
criterion: the device call as a graph is not slower than the composition (its faster form) at any measured shape.
Also timed: the chain decode -> bbox_post_processing (min_det_score 0.05, nms_thr 0.5, max_det 100) as one graph.

Two score distributions: `dense` (class logits ~ N(-3, 1.5^2)) and `sparse` (~ N(-6, 1)); the selection does the same
work for both (there is no threshold), the post-processing behind it does not.  NSETS input sets are rotated between
calls; medians over --iters calls after a warm-up; the event floor is stored next to them.

    python tools/reppoints_decode_time.py [--iters 50] [--sets 3] [--out profiles/reppoints_decode_time.json]

Per-kernel split: run `--trace CALLS` (the device call alone, dense, N = 1, logits in) under
`rocprofv3 --kernel-trace --stats`, then `--merge-stats <..._kernel_stats.csv>` writes the averages into the JSON.
"""
import argparse
import csv
import json
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops  # noqa: E402

SIZES = ((100, 167), (50, 84), (25, 42), (13, 21), (7, 11))
STRIDES = (8, 16, 32, 64, 128)
C, TOP_N, NUM_POINTS = 80, 1000, 9
MIN_SCORE, NMS_THR, MAX_DET = 0.05, 0.5, 100
DISTRIBUTIONS = (("dense", -3.0, 1.5), ("sparse", -6.0, 1.0))
KS = ops.reppoints_topk_table(STRIDES, TOP_N)
HWS = [h * w for h, w in SIZES]
R = sum(k if k > 0 else hw for k, hw in zip(KS, HWS))


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
            keep = fn(i)
        out.append((g, keep))
    return out


def torch_decode(cls_l, pts_l, info, mt, logits):
    """the reference's steps, level by level and image by image as it has them"""
    scores, boxes = [], []
    e = mt.exp()
    for cls, pts, s, k in zip(cls_l, pts_l, STRIDES, KS):
        N, _, H, W = cls.shape
        HW = H * W
        score = cls.permute(0, 2, 3, 1).reshape(N, HW, -1)
        if logits:
            score = torch.sigmoid(score)
        idx = torch.topk(score.max(-1).values, k if k > 0 else HW, dim=1).indices
        pp = pts.reshape(N, NUM_POINTS, 2, HW)
        y, x = pp[:, :, 0], pp[:, :, 1]
        my, mx = y.mean(1, keepdim=True), x.mean(1, keepdim=True)
        sy, sx = ((y - my) ** 2).mean(1, keepdim=True).sqrt(), ((x - mx) ** 2).mean(1, keepdim=True).sqrt()
        hx, hy = sx * e[0], sy * e[1]
        box = torch.cat([mx - hx, my - hy, mx + hx, my + hy], 1).permute(0, 2, 1)          # (N, HW, 4)
        px = (torch.arange(W, device=cls.device, dtype=torch.float32) * s)[None, :].expand(H, W).reshape(-1)
        py = (torch.arange(H, device=cls.device, dtype=torch.float32) * s)[:, None].expand(H, W).reshape(-1)
        point = torch.stack([px, py, px, py], 1)
        si, bi = [], []
        for i in range(N):
            b = box[i][idx[i]] * s + point[idx[i]]
            lim = torch.stack([info[i, 1], info[i, 0], info[i, 1], info[i, 0]]) - 1.0
            bi.append(torch.clamp(torch.minimum(b, lim), min=0.0))
            si.append(score[i][idx[i]])
        sc = torch.stack(si)
        scores.append(torch.cat([torch.zeros_like(sc[:, :, :1]), sc], -1))
        boxes.append(torch.stack(bi))
    return torch.cat(scores, 1), torch.cat(boxes, 1)


def make_inputs(N, mean, sigma, nsets, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    mk = lambda ch, sc, sh: [[torch.randn((N, ch, h, w), device="cuda", generator=gen) * sc + sh for h, w in SIZES]
                             for _ in range(nsets)]
    lcls, pts = mk(C, sigma, mean), mk(2 * NUM_POINTS, 2.0, 0.0)
    pcls = [[ops.fcos_sigmoid(v) for v in lv] for lv in lcls]
    info = torch.tensor([[800.0, 1333.0, 1.0]] * N, device="cuda")
    mt = torch.tensor([0.1, -0.1], device="cuda")
    buf = dict(cls_score=torch.empty(N, R, C + 1, device="cuda"), bbox_xyxy=torch.empty(N, R, 4, device="cuda"),
               workspace=torch.empty(ops.reppoints_decode_workspace_bytes(N, C, HWS, KS), device="cuda", dtype=torch.uint8))
    return lcls, pcls, pts, info, mt, buf


def trace(calls):
    lcls, _, pts, info, mt, buf = make_inputs(1, -3.0, 1.5, 1, 12)
    for _ in range(calls):
        ops.reppoints_decode(lcls[0], pts[0], info, STRIDES, KS, moment_transfer=mt, input_logits=True, **buf)
    torch.cuda.synchronize()


def merge_stats(path, out):
    with open(out) as f:
        doc = json.load(f)
    split = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            m = re.search(r"\brd_\w+", name)
            if m:
                short = m.group(0)
                split[short] = dict(calls=int(row["Calls"]), average_us=round(float(row["AverageNs"]) / 1e3, 2),
                                    min_us=round(float(row["MinNs"]) / 1e3, 2), max_us=round(float(row["MaxNs"]) / 1e3, 2))
    if not split:
        raise SystemExit("no rd_* kernel in %s" % path)
    doc["reppoints_decode"]["kernel_split_dense_n1_logits"] = dict(
        source="rocprofv3 --kernel-trace --stats, one run of --trace", kernels=split,
        sum_of_averages_us=round(sum(v["average_us"] for v in split.values()), 2))
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(doc["reppoints_decode"]["kernel_split_dense_n1_logits"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reppoints_decode_time.json"))
    ap.add_argument("--trace", type=int, default=0, help="only run this many device calls (for a kernel trace)")
    ap.add_argument("--merge-stats", default=None, help="kernel_stats.csv of a rocprofv3 run of --trace")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out)
    if args.trace:
        return trace(args.trace)
    nsets = max(3, args.sets)
    res = dict(event_floor_us=round(time_events(lambda i: None, args.iters, 1), 1),
               shape=dict(C=C, num_points=NUM_POINTS, transform="moment", pre_nms_top_n=TOP_N, strides=list(STRIDES),
                          sizes=[list(s) for s in SIZES], rows_kept=[k if k > 0 else hw for k, hw in zip(KS, HWS)], R=R,
                          locations_per_image=sum(HWS)))
    ok = True
    for dist, mean, sigma in DISTRIBUTIONS:
        for N in (1, 2):
            lcls, pcls, pts, info, mt, buf = make_inputs(N, mean, sigma, nsets, 11 + N)
            r = dict(N=N, R=R, workspace_bytes=int(buf["workspace"].numel()),
                     input_bytes_per_call=4 * N * (C + 2 * NUM_POINTS) * sum(HWS), output_bytes_per_call=4 * N * R * (C + 5))
            post = (torch.empty(N, MAX_DET, 1, device="cuda"), torch.empty(N, MAX_DET, 4, device="cuda"),
                    torch.empty(N, MAX_DET, 1, device="cuda"))
            for logits, cl in ((0, pcls), (1, lcls)):
                def dev(i, cl=cl, logits=logits):
                    ops.reppoints_decode(cl[i], pts[i], info, STRIDES, KS, moment_transfer=mt, input_logits=bool(logits), **buf)

                def chain(i, cl=cl, logits=logits):
                    dev(i)
                    ops.bbox_post_processing(buf["cls_score"], buf["bbox_xyxy"], max_det_per_image=MAX_DET,
                                             min_det_score=MIN_SCORE, nms_thr=NMS_THR, out=post)

                def ref(i, cl=cl, logits=logits):
                    return torch_decode(cl[i], pts[i], info, mt, logits)
                e = time_events(dev, args.iters, nsets)
                gs = graphs_of(dev, nsets)
                g = time_events(lambda i: gs[i][0].replay(), args.iters, nsets)
                del gs
                cs = graphs_of(chain, nsets)
                cg = time_events(lambda i: cs[i][0].replay(), args.iters, nsets)
                del cs
                t = time_events(ref, max(10, args.iters // 2), nsets)
                ts = graphs_of(ref, nsets)
                tg = time_events(lambda i: ts[i][0].replay(), args.iters, nsets)
                del ts
                # the two agree: the same rows wherever no two maxima tie, boxes up to the rounding of the sums
                dev(0)
                rs, rb = ref(0)
                same = float((buf["cls_score"] == rs).all(-1).float().mean())
                best = min(t, tg)
                ok = ok and g <= best
                r["input_logits_%d" % logits] = dict(
                    eager_us=round(e, 1), graph_us=round(g, 1), chain_with_bbox_post_graph_us=round(cg, 1),
                    torch_composition_eager_us=round(t, 1), torch_composition_graph_us=round(tg, 1),
                    not_slower_than_torch=bool(g <= best), eager_not_slower_than_torch_eager=bool(e <= t),
                    rows_with_the_same_scores_as_torch=round(same, 6),
                    max_abs_bbox_diff_vs_torch=float((buf["bbox_xyxy"] - rb).abs().max()))
            res["%s_n%d" % (dist, N)] = r
            print(dist, N, json.dumps(r), flush=True)
            del lcls, pcls, pts, buf
            torch.cuda.empty_cache()
    res["not_slower_than_torch_at_every_shape"] = bool(ok)
    res["run"] = dict(input_sets=nsets, iters=args.iters, timer="device events, median",
                      distributions={d: dict(cls_logit_mean=m, cls_logit_sigma=s) for d, m, s in DISTRIBUTIONS})
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"reppoints_decode": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"reppoints_decode": {k: {m: v[m]["graph_us"] for m in ("input_logits_0", "input_logits_1")}
                                           for k, v in res.items() if isinstance(v, dict) and "N" in v}}))


if __name__ == "__main__":
    main()
