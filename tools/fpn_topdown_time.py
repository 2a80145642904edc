#!/usr/bin/env python
"""FPN top-down pathway timing: the chain of faster_r50v1_fpn_1x at 800 x 1333 (25x42 -> 50x84 -> 100x167 ->
200x334, C = 256) with two images and with one, and RetinaNet's three levels, float32 and float16.

Timed from device events, eagerly and as a captured HIP graph, forward and backward each on their own.  NSETS input
sets are rotated between calls (one P2-sized tensor is 137 MB: below the 256 MB MALL).  In the same run, on the same
tensors, ALTERNATING (one call of each variant per round, so that clocks and neighbours drift for all alike):
  1. the fused call (one launch for the chain);
  2. the same work as L-1 single-step calls of the same library (two-level calls chained; the backward's add of
     g_l, which the fused call does inside, is a torch add between them);
  3. the torch composition (interpolate(nearest), slice, add; autograd for the backward, the forward's graph built
     outside the timed region), eager and captured;
  4. a device-to-device copy that moves the fused call's algorithmic bytes (a copy of B / 2 bytes reads and writes
     B).  copy_us / graph_us is the roofline figure: the share of the copy's rate the fused call reaches.
`not_slower_than_torch` per shape and direction: the captured fused call takes no longer than the captured
composition.  `one_launch_not_slower_than_per_level` likewise.  No time or fraction is asserted here.

    python tools/fpn_topdown_time.py [--iters 30] [--sets 3] [--out profiles/fpn_topdown_time.json]
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

from simpledet_amd import ops  # noqa: E402
from simpledet_amd._lib import lib  # noqa: E402

FPN = ((25, 42), (50, 84), (100, 167), (200, 334))
SHAPES = (("fpn_n2", 2, 256, FPN), ("fpn_n1", 1, 256, FPN), ("retina_n2", 2, 256, FPN[:3]))


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
    """one graph per input set, captured on the stream everything here runs on (main() makes a side stream current:
    autograd runs a backward node on the stream of its forward, which must be the capturing one)"""
    fn(0)
    torch.cuda.synchronize()
    out = []
    for i in range(nsets):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.current_stream()):
            fn(i)
        out.append(g)
    return lambda i: out[i].replay()


def dispatch():
    return (lib().cdll.sd_last_dispatch() or b"").decode()


def composition(top, lats):
    outs, p = [], top
    for lat in lats:
        p = Fn.interpolate(p, scale_factor=2, mode="nearest")[:, :, :lat.shape[2], :lat.shape[3]] + lat
        outs.append(p)
    return outs


def measure(N, C, chain, dt, iters, nsets, gen):
    L = len(chain)
    shapes = [(N, C, h, w) for h, w in chain]
    numel = [int(np.prod(s)) for s in shapes]
    esz = 4 if dt == torch.float32 else 2
    rnd = lambda s: torch.randn(s, device="cuda", generator=gen).to(dt)   # noqa: E731
    tops = [rnd(shapes[0]) for _ in range(nsets)]
    lats = [[rnd(s) for s in shapes[1:]] for _ in range(nsets)]
    grads = [[rnd(s) for s in shapes[1:]] for _ in range(nsets)]
    outs = [torch.empty(s, device="cuda", dtype=dt) for s in shapes[1:]]
    d_top = torch.empty(shapes[0], device="cuda", dtype=dt)
    d_lat = [torch.empty(s, device="cuda", dtype=dt) for s in shapes[1:-1]] + [None]
    d_mid = [torch.empty(s, device="cuda", dtype=dt) for s in shapes[1:-1]]      # the per-level chain's S_l

    def fwd(i):
        ops.fpn_topdown_forward(tops[i], lats[i], outs=outs)

    def fwd_steps(i):
        p = tops[i]
        for l in range(L - 1):
            p = ops.fpn_topdown_forward(p, [lats[i][l]], outs=[outs[l]])[0]

    def bwd(i):
        ops.fpn_topdown_backward(grads[i], shapes, d_top=d_top, d_laterals=d_lat)

    def bwd_steps(i):
        D = grads[i][L - 2]
        for l in range(L - 2, -1, -1):
            if l == 0:
                ops.fpn_topdown_backward([D], shapes[:2], d_top=d_top)
            else:
                ops.fpn_topdown_backward([D], [shapes[l], shapes[l + 1]], d_top=d_mid[l - 1])
                D = torch.add(grads[i][l - 1], d_mid[l - 1], out=d_lat[l - 1])
    fwd(0)
    d_f = dispatch()
    bwd(0)
    d_b = dispatch()

    def t_fwd(i):
        with torch.no_grad():
            composition(tops[i], lats[i])
    leaves, t_outs = [], []
    for i in range(nsets):
        lv = [tops[i].clone().requires_grad_()] + [x.clone().requires_grad_() for x in lats[i]]
        leaves.append(lv)
        t_outs.append(composition(lv[0], lv[1:]))

    def t_bwd(i):
        torch.autograd.grad(t_outs[i], leaves[i], grads[i], retain_graph=True)
    fine, inner = sum(numel[1:]), sum(numel[1:-1])
    bytes_of = dict(fwd=(numel[0] + 2 * fine) * esz, bwd=(fine + numel[0] + inner) * esz)
    r = dict(N=N, C=C, chain=[list(c) for c in chain], dtype=str(dt).replace("torch.", ""), dispatch_fwd=d_f,
             dispatch_bwd=d_b)
    for key, ours, steps, theirs in (("fwd", fwd, fwd_steps, t_fwd), ("bwd", bwd, bwd_steps, t_bwd)):
        bytes_ = bytes_of[key]
        half = bytes_ // 2
        src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        copy = lambda i: dst.copy_(src[i])   # noqa: E731
        eager = [ours, steps, theirs, copy]
        e = time_round_robin(eager, iters, nsets)
        g = time_round_robin([graphs_of(fn, nsets) for fn in eager], iters, nsets)
        del src, dst
        r[key] = dict(eager_us=e[0], graph_us=g[0], per_level_eager_us=e[1], per_level_graph_us=g[1],
                      torch_eager_us=e[2], torch_graph_us=g[2], copy_eager_us=e[3], copy_graph_us=g[3],
                      algorithmic_bytes=bytes_, TBps=round(bytes_ / g[0] * 1e-6, 3), fraction_of_copy=round(g[3] / g[0], 3),
                      speedup_over_torch_graph=round(g[2] / g[0], 2), speedup_over_per_level_graph=round(g[1] / g[0], 2),
                      not_slower_than_torch=bool(g[0] <= g[2]), one_launch_not_slower_than_per_level=bool(g[0] <= g[1]))
    r["not_slower_than_torch"] = bool(r["fwd"]["not_slower_than_torch"] and r["bwd"]["not_slower_than_torch"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fpn_topdown_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        for site, N, C, chain in SHAPES:
            for dt in (torch.float32, torch.float16):
                name = "%s_%s" % (site, "f32" if dt == torch.float32 else "f16")
                res[name] = measure(N, C, chain, dt, args.iters, nsets, gen)
                print(name, json.dumps(res[name]), flush=True)
                torch.cuda.empty_cache()
    slower = sorted("%s.%s" % (k, d) for k, v in res.items() for d in ("fwd", "bwd") if not v[d]["not_slower_than_torch"])
    per_level = sorted("%s.%s" % (k, d) for k, v in res.items() for d in ("fwd", "bwd")
                       if not v[d]["one_launch_not_slower_than_per_level"])
    res["summary"] = dict(not_slower_than_torch_everywhere=not slower, slower_than_torch=slower,
                          one_launch_slower_than_per_level=per_level)
    res["config"] = dict(input_sets=nsets, iters=args.iters, device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"fpn_topdown": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"fpn_topdown": res["summary"]}))


if __name__ == "__main__":
    main()
