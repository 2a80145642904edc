#!/usr/bin/env python
"""Squeeze-and-excitation block timing: the SE-v2 ResNet-50 sites at 800 x 1333 with two images (float32), the SE mask
head (256, 256, 14, 14) in float32 and float16, and a stage-3, a stage-5 and a stage-7 MBConv of EfficientNet-B5 at
400 x 667 with eight images (float16; C = 6 f_in, Cr = f_in / 4 from the builder's table).

Timed from device events, eagerly and as a captured HIP graph: forward, backward, and forward + backward as one graph.
NSETS input sets are rotated between calls.  In the same run, on the same tensors, ALTERNATING (one call of each
variant per round, so that clocks and neighbours drift for all alike):
  1. se_block with the automatic path;  2. path 1 (two-pass);  3. path 2 (resident), where the image fits;
  4. the torch composition of the reference's seven nodes (autograd for the backward, its forward graph built outside
     the timed region except in forward + backward);
  5. a device-to-device copy that moves the two-pass algorithmic bytes (3 tensor passes forward, 5 backward).
`fraction_of_8TBps` is over the algorithmic bytes of the path that ran (2 / 3 passes resident).  A second read of a
tensor under 256 MB may come from the Infinity Cache, so a fraction above what HBM gives is no error.
`not_slower_than_torch` per row and direction: the captured automatic call takes no longer than the captured
composition.  No time or fraction is asserted here.

    python tools/se_block_time.py [--iters 20] [--sets 3] [--out profiles/se_block_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as Fn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import se_block as se  # noqa: E402
from simpledet_amd._lib import SimpleDetOpsError, lib  # noqa: E402

F32, F16 = torch.float32, torch.float16
SHAPES = (("se_r50_c2", (2, 64, 200, 334), 16, F32), ("se_r50_c3", (2, 128, 100, 167), 32, F32),
          ("se_r50_c4", (2, 256, 50, 84), 64, F32), ("se_r50_c5", (2, 512, 25, 42), 128, F32),
          ("mask_head", (256, 256, 14, 14), 64, F32), ("mask_head", (256, 256, 14, 14), 64, F16),
          ("b5_stage3", (8, 240, 100, 167), 10, F16), ("b5_stage5", (8, 768, 25, 42), 32, F16),
          ("b5_stage7", (8, 1824, 13, 21), 76, F16))


def time_round_robin(fns, iters, nsets):
    """one call of every variant per round; the median per variant, in microseconds"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for i in range(3):
        for fn in fns:
            fn(i % nsets)
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for i in range(iters):
        for k, fn in enumerate(fns):
            start.record()
            fn(i % nsets)
            end.record()
            end.synchronize()
            ts[k].append(start.elapsed_time(end) * 1e3)
    return [round(float(np.median(t)), 1) for t in ts]


def graphs_of(fn, nsets):
    fn(0)
    torch.cuda.synchronize()
    out = []
    for i in range(nsets):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.current_stream()):
            fn(i)
        out.append(g)
    return lambda i: out[i].replay()


def composition(x, w1, w2):
    gap = x.mean(dim=-1, keepdim=True).mean(dim=-2, keepdim=True)
    h = torch.clamp(Fn.conv2d(gap, w1), 0.0, 6.0)
    return x * torch.sigmoid(Fn.conv2d(h, w2))


def measure(shape, Cr, dt, iters, nsets, gen):
    N, C = shape[:2]
    esz = 4 if dt == F32 else 2
    tensor = int(np.prod(shape)) * esz
    rnd = lambda s, k=1.0: (torch.randn(s, device="cuda", generator=gen) * k).to(dt)   # noqa: E731
    xs, dys = [rnd(shape) for _ in range(nsets)], [rnd(shape) for _ in range(nsets)]
    w1, w2 = rnd((Cr, C, 1, 1), 6.0 / C ** 0.5), rnd((C, Cr, 1, 1), 0.5 / Cr ** 0.5)
    y, dx = torch.empty_like(xs[0]), torch.empty_like(xs[0])
    paths = [0, 1]
    try:
        se.se_block_forward(xs[0], w1, None, w2, None, 2, y=y)
        paths.append(2)
    except SimpleDetOpsError:
        pass
    ws = {p: torch.empty(se.workspace_bytes(N, C, Cr, tensor // esz // (N * C), p), dtype=torch.uint8, device="cuda")
          for p in paths}
    saved = [se.se_block_forward(x, w1, None, w2, None, 1)[1:] for x in xs]
    dispatch = {}
    for p in paths:
        se.se_block_forward(xs[0], w1, None, w2, None, p, workspace=ws[p], y=y)
        dispatch[p] = (lib().cdll.sd_last_dispatch() or b"").decode()
    resident_auto = "resident" in dispatch[0]

    def fwd(p):
        return lambda i: se.se_block_forward(xs[i], w1, None, w2, None, p, workspace=ws[p], y=y)

    def bwd(p):
        return lambda i: se.se_block_backward(dys[i], xs[i], *saved[i], w1, w2, p, workspace=ws[p],
                                              bias_grads=(False, False), dx=dx)

    def both(p):
        def fn(i):
            f = se.se_block_forward(xs[i], w1, None, w2, None, p, workspace=ws[p], y=y)
            se.se_block_backward(dys[i], xs[i], f[1], f[2], f[3], w1, w2, p, workspace=ws[p],
                                 bias_grads=(False, False), dx=dx)
        return fn
    leaves = [[x.clone().requires_grad_(), w1.clone().requires_grad_(), w2.clone().requires_grad_()] for x in xs]
    t_out = [composition(*lv) for lv in leaves]

    def t_fwd(i):
        with torch.no_grad():
            composition(xs[i], w1, w2)

    def t_bwd(i):
        torch.autograd.grad(t_out[i], leaves[i], dys[i], retain_graph=True)

    def t_both(i):
        torch.autograd.grad(composition(*leaves[i]), leaves[i], dys[i])
    r = dict(shape=list(shape), Cr=Cr, dtype=str(dt).replace("torch.", ""), dispatch=dispatch,
             automatic_is_resident=resident_auto)
    passes = dict(fwd=(3, 2), bwd=(5, 3), fwd_bwd=(8, 5))
    for key, ours, theirs in (("fwd", fwd, t_fwd), ("bwd", bwd, t_bwd), ("fwd_bwd", both, t_both)):
        two, res = passes[key]
        half = two * tensor // 2
        src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        fns = [ours(p) for p in paths] + [theirs, lambda i: dst.copy_(src[i])]
        e = time_round_robin(fns, iters, nsets)
        g = time_round_robin([graphs_of(fn, nsets) for fn in fns], iters, nsets)
        del src, dst
        row = dict(torch_eager_us=e[-2], torch_graph_us=g[-2], copy_eager_us=e[-1], copy_graph_us=g[-1],
                   two_pass_bytes=two * tensor)
        for k, p in enumerate(paths):
            name = ("auto", "two_pass", "resident")[p]
            n_pass = res if (p == 2 or (p == 0 and resident_auto)) else two
            row[name] = dict(eager_us=e[k], graph_us=g[k], algorithmic_bytes=n_pass * tensor,
                             fraction_of_8TBps=round(n_pass * tensor / g[k] * 1e-6 / 8.0, 3))
        row["speedup_over_torch_graph"] = round(g[-2] / g[0], 2)
        row["not_slower_than_torch"] = bool(g[0] <= g[-2])
        r[key] = row
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "se_block_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        for site, shape, Cr, dt in SHAPES:
            name = "%s_%s" % (site, "f32" if dt == F32 else "f16")
            res[name] = measure(shape, Cr, dt, args.iters, nsets, gen)
            print(name, json.dumps(res[name]), flush=True)
            torch.cuda.empty_cache()
    dirs = ("fwd", "bwd", "fwd_bwd")
    slower = sorted("%s.%s" % (k, d) for k, v in res.items() for d in dirs if not v[d]["not_slower_than_torch"])
    res["summary"] = dict(not_slower_than_torch_everywhere=not slower, slower_than_torch=slower)
    res["config"] = dict(input_sets=nsets, iters=args.iters, device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"se_block": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"se_block": res["summary"]}))


if __name__ == "__main__":
    main()
