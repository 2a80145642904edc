#!/usr/bin/env python
"""CrowdHuman double-prediction head timing (simpledet_amd/csrc/crowdhuman_head.hip) at the shape of
config/crowdhuman/doublepred_r50v1b_fpn_1x.py: B = 2 images, P = 2000 proposals, M = 500 gt rows of which 40 are real,
image_rois = 512, two classes (R = 1024 rows, K = 2, D = 8 for the loss).

Timed from device events, eagerly and as one captured HIP graph, all in the same run on the same inputs: the targets
(doublebbox_target), the EMD loss forward + backward, and the chain targets -> loss.  Compared with
  targets  the reference's algorithm on the host as it runs there: two device-to-host copies, per image numpy (a
           vectorised IoU in place of the Cython loop, the same np.random.choice calls, the same expansion loops), seven
           host-to-device copies.  A host clock around it, ending in a device synchronise; it cannot be captured.
  loss     a torch composition of the reference's graph (four softmax cross-entropies, four smooth-L1, the minimum and
           the mean) with autograd; `not_slower_than_torch` covers this one.
`sampling_share`: the targets are four kernels, of which the third is ONE workgroup that replays numpy's MT19937 for
all images in order.  A child process on the profiling build of the library (tools/libsimpledet_ops_hip_prof.so, knob
crowdhuman_target_stop) times the chain cut after two and after three kernels; the difference over the whole chain is
the share of the serial sampling wave.  Missing when that library is not built.

    python tools/crowdhuman_head_time.py [--iters 50] [--sets 3] [--out profiles/crowdhuman_head_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import _lib, ops  # noqa: E402
from tests import crowdhuman_ref as cr  # noqa: E402

B, P, M, REAL, S, K = 2, 2000, 500, 40, 512, 2
CFG = dict(cr.CONFIG, image_rois=S)
PROF_LIB = os.path.join(ROOT, "tools", "libsimpledet_ops_hip_prof.so")


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


def time_host(fn, iters, nsets):
    for i in range(2):
        fn(i % nsets)
    torch.cuda.synchronize()
    ts = []
    for i in range(iters):
        t = time.perf_counter()
        fn(i % nsets)
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e6)
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


def inputs(nsets):
    rs = np.random.RandomState(5)
    sets = []
    for _ in range(nsets):
        imgs = [cr._image(rs, P, M, [1] * (REAL - 2) + [-2] * 2, near=300, mid=500, pad_prop=31) for _ in range(B)]
        sets.append((torch.from_numpy(np.stack([p for p, _ in imgs])).cuda(),
                     torch.from_numpy(np.stack([g for _, g in imgs])).cuda()))
    return sets


# ------------------------------------------------------------------ the reference's algorithm on the host --
def _iou(boxes, query):
    """bbox_overlaps (operator_py/cython/bbox.pyx) vectorised: (n, k)"""
    qa = (query[:, 2] - query[:, 0] + 1) * (query[:, 3] - query[:, 1] + 1)
    ba = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    iw = np.minimum(boxes[:, None, 2], query[None, :, 2]) - np.maximum(boxes[:, None, 0], query[None, :, 0]) + 1
    ih = np.minimum(boxes[:, None, 3], query[None, :, 3]) - np.maximum(boxes[:, None, 1], query[None, :, 1]) + 1
    inter = np.where((iw > 0) & (ih > 0), iw * ih, 0)
    return (inter / (ba[:, None] + qa[None] - inter)).astype(np.float32)


def _expand(cls, t, nrc):
    out, w = np.zeros((len(cls), 4 * nrc)), np.zeros((len(cls), 4 * nrc))
    for i in np.where(cls > 0)[0]:
        c = int(cls[i])
        out[i, 4 * c:4 * c + 4] = t[i]
        w[i, 4 * c:4 * c + 4] = 1.0
    return out, w


def host_targets(prop_dev, gt_dev, cfg):
    """doublebbox_target as the reference runs it: asnumpy(), numpy per image, copies back"""
    props, gts = prop_dev.cpu().numpy(), gt_dev.cpu().numpy()
    nrc, S_ = cfg["num_reg_class"], cfg["image_rois"]
    inv = [1.0 / s for s in cfg["bbox_target_std"]]
    res = [[] for _ in range(7)]
    for p, g in zip(props, gts):
        g = g[g[:, 4] != -1].copy()
        p = np.append(p[p[:, 3] != 0], g[:, :4], axis=0)
        g[g[:, 4] == -2, 4] = -1
        n = len(p)
        cls, mx, idx, smx, sidx = np.zeros(n), np.zeros(n), np.zeros(n, np.int64), np.zeros(n), np.zeros(n, np.int64)
        for cid in range(1, nrc):
            gi = np.where(g[:, 4] == cid)[0]
            if len(gi) == 0:
                continue
            ov = _iou(p, g[gi])
            a1, m1 = ov.argmax(1), ov.max(1)
            ov[np.arange(n), a1] = -1
            m2, a2 = ov.max(1), ov.argmax(1)
            v = np.where(m1 > mx)[0]
            cls[v], mx[v], idx[v], sidx[v], smx[v] = cid, m1[v], gi[a1[v]], gi[a2[v]], m2[v]
        fgq = int(np.round(cfg["fg_fraction"] * S_))
        fg = np.where(mx >= cfg["fg_thresh"])[0]
        nfg = min(fgq, fg.size)
        if fg.size > 0:
            fg = np.random.choice(fg, size=nfg, replace=False)
        bg = np.where((mx < cfg["bg_thresh_hi"]) & (mx >= cfg["bg_thresh_lo"]))[0]
        nbg = min(S_ - nfg, bg.size)
        if bg.size > 0:
            bg = np.random.choice(bg, size=nbg, replace=False)
        keep = np.append(fg, bg)
        lab = cls[keep]
        lab[nfg:] = 0
        slab = cls[keep]
        slab[smx[keep] < cfg["fg_thresh"]] = 0
        t1, _ = cr.encode_truth(p[keep], g[idx[keep], :4], inv)
        t2, _ = cr.encode_truth(p[keep], g[sidx[keep], :4], inv)
        e1, e2 = _expand(lab, t1, nrc), _expand(slab, t2, nrc)
        for lst, v in zip(res, (p[keep], lab, e1[0], e1[1], slab, e2[0], e2[1])):
            lst.append(v)
    return [torch.from_numpy(np.array(v, dtype=np.float32)).cuda() for v in res]


# ------------------------------------------------------------ the reference's loss graph as a torch composition --
def torch_emd(x1, x2, y1, y2, d1, d2, t1, t2, w1, w2, sigma=1.0):
    s2 = sigma * sigma

    def ce(x, y):
        oh = (torch.arange(x.shape[1], device=x.device)[None] == y[:, None]).float()
        return -oh * torch.log(torch.softmax(x, -1) + 1e-10)

    def sl1(v):
        return torch.where(v.abs() > 1 / s2, v.abs() - 0.5 / s2, 0.5 * s2 * v * v)
    L1 = (ce(x1, y1) + ce(x2, y2)).sum(-1) + (w1 * sl1(d1 - t1) + w2 * sl1(d2 - t2)).sum(-1)
    L2 = (ce(x1, y2) + ce(x2, y1)).sum(-1) + (w2 * sl1(d1 - t2) + w1 * sl1(d2 - t1)).sum(-1)
    return torch.minimum(L1, L2).mean()


def sampling_share(iters):
    """child process on the profiling build: graph time of the chain cut after 2, 3 and all 4 kernels"""
    sets = inputs(1)
    st = ops.mt19937_state(seed=3)
    ws = torch.empty(ops.crowdhuman_target_workspace_bytes(B, P, M), dtype=torch.uint8, device="cuda")
    out = {}
    for stop in (2, 3, 0):
        _lib.lib().set_tuning("crowdhuman_target_stop", stop)
        fn = lambda i: ops.crowdhuman_target(sets[0][0], sets[0][1], st, workspace=ws, **CFG)
        gs = graphs_of(fn, 1)
        out["kernels_%d" % (stop or 4)] = round(time_events(lambda i: gs[0].replay(), iters, 1), 1)
    out["sampling_kernel_us"] = round(out["kernels_3"] - out["kernels_2"], 1)
    out["sampling_share"] = round(out["sampling_kernel_us"] / out["kernels_4"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crowdhuman_head_time.json"))
    ap.add_argument("--share-only", action="store_true", help="(internal) print the sampling share as JSON")
    args = ap.parse_args()
    if args.share_only:
        print("SHARE " + json.dumps(sampling_share(args.iters)))
        return
    nsets = max(1, args.sets)
    sets = inputs(nsets)
    st = ops.mt19937_state(seed=3)
    ws = torch.empty(ops.crowdhuman_target_workspace_bytes(B, P, M), dtype=torch.uint8, device="cuda")
    res = dict(shape=dict(B=B, P=P, M=M, real_gt=REAL, image_rois=S, K=K, R=B * S, D=4 * K),
               event_floor_us=round(time_events(lambda i: None, args.iters, 1), 1))

    def target(i):
        return ops.crowdhuman_target(sets[i][0], sets[i][1], st, workspace=ws, **CFG)
    tg = target(0)
    torch.cuda.synchronize()
    assert bool((tg.count == S).all()), "an image did not fill its rows"
    R = B * S
    gen = torch.Generator(device="cuda").manual_seed(1)
    heads = [[torch.randn((R, n), device="cuda", generator=gen) * s for n, s in ((K, 2.0), (K, 2.0), (4 * K, 0.5), (4 * K, 0.5))]
             for _ in range(nsets)]
    grads = [torch.empty((R, K), device="cuda"), torch.empty((R, K), device="cuda"),
             torch.empty((R, 4 * K), device="cuda"), torch.empty((R, 4 * K), device="cuda")]
    loss = torch.empty((1,), device="cuda")

    def loss_args(i, t):
        x1, x2, d1, d2 = heads[i]
        return (x1, x2, t.bbox_cls.view(-1), t.bbox_sec_cls.view(-1), d1, d2, t.bbox_target.view(R, -1),
                t.bbox_sec_target.view(R, -1), t.bbox_target_weight.view(R, -1), t.bbox_sec_target_weight.view(R, -1))

    def fwd_bwd(i, t=None):
        a = loss_args(i, t or tg)
        ops.emd_loss_forward(*a, 1.0, loss=loss)
        ops.emd_loss_backward(*a, 1.0, 128.0, d_cls_logit=grads[0], d_cls_sec_logit=grads[1], d_bbox_delta=grads[2],
                              d_bbox_sec_delta=grads[3])

    def chain(i):
        fwd_bwd(i, target(i))
    for key, fn in (("target", target), ("loss_fwd_bwd", fwd_bwd), ("chain", chain)):
        res[key] = both_ways(fn, args.iters, nsets)
    # the other way to resolve the front of the permutations: all swaps replayed on an LDS array, one lane per list
    with _lib.lib().tuned(crowdhuman_front=1):
        res["target_front_lds_replay"] = both_ways(target, args.iters, nsets)
    # the host algorithm of the reference (cannot be captured: it synchronises by construction)
    res["host_reference"] = dict(target_us=round(time_host(lambda i: host_targets(sets[i][0], sets[i][1], CFG),
                                                           max(5, args.iters // 5), nsets), 1))
    req = [[t.clone().requires_grad_() for t in heads[i]] for i in range(nsets)]

    def t_fwd_bwd(i):
        a = loss_args(i, tg)
        x1, x2, d1, d2 = req[i]
        total = torch_emd(x1, x2, a[2], a[3], d1, d2, *a[6:]) * 128.0
        torch.autograd.grad(total, req[i])
    res["torch_composition"] = dict(loss_fwd_bwd=both_ways(t_fwd_bwd, args.iters, nsets))
    tl = float(torch_emd(*loss_args(0, tg)))
    fwd_bwd(0)
    res["vs_torch"] = dict(loss=float(loss), torch_loss=tl, rel_diff=abs(float(loss) - tl) / abs(tl))
    tc = res["torch_composition"]["loss_fwd_bwd"]
    res["not_slower_than_torch"] = dict(loss_eager=res["loss_fwd_bwd"]["eager_us"] <= tc["eager_us"],
                                        loss_graph=res["loss_fwd_bwd"]["graph_us"] <= tc["graph_us"])
    res["target_vs_host"] = dict(eager_ratio=round(res["host_reference"]["target_us"] / res["target"]["eager_us"], 1),
                                 graph_ratio=round(res["host_reference"]["target_us"] / res["target"]["graph_us"], 1))
    if os.path.exists(PROF_LIB):
        env = dict(os.environ, SIMPLEDET_AMD_LIB=PROF_LIB)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--share-only", "--iters", str(args.iters)],
                             env=env, capture_output=True, text=True, timeout=300)
        line = [l for l in out.stdout.splitlines() if l.startswith("SHARE ")]
        res["sampling"] = json.loads(line[0][6:]) if line else dict(error=(out.stderr or out.stdout)[-300:])
    else:
        res["sampling"] = dict(error="tools/libsimpledet_ops_hip_prof.so is not built (make -C simpledet_amd/csrc prof)")
    res["run"] = dict(input_sets=nsets, iters=args.iters)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"crowdhuman_head": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"crowdhuman_head": res}))


if __name__ == "__main__":
    main()
