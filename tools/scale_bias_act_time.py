#!/usr/bin/env python
"""Merged-BN affine timing at the sites of a ResNet-50 backbone on 800 x 1344, two images, float32 and float16:
the stem, a stage-1 inner convolution (scale + bias + relu), the four stage outputs (scale + bias + shortcut +
relu) and the plain _contrib_BroadcastScale.

Timed from device events, eagerly and as a captured HIP graph, forward and backward each on their own.  NSETS input
sets are rotated between calls (the largest tensor is 137 MB; the small sites fit the 256 MB MALL whatever is done).
In the same run, on the same tensors:
  1. the torch composition of the reference's nodes (x * g, + b, + r, where(v > 0, v, 0); autograd for the backward,
     the forward's graph built outside the timed region), eager and captured;
  2. a device-to-device copy that moves the fused call's algorithmic bytes (a copy of B / 2 bytes reads and writes
     B): forward 2 or 3 tensor passes (x, the shortcut, y), backward dy, y under relu, dx, and dres with a shortcut.
     copy_us / graph_us is the roofline figure: the share of the copy's rate the fused call reaches.
`not_slower_than_torch` per shape: the captured fused call takes no longer than the captured composition, in both
directions.  No time or fraction is asserted here.  `bwd_with_dbeta`: the backward when the beta gradient is asked for.

    python tools/scale_bias_act_time.py [--iters 30] [--sets 3] [--out profiles/scale_bias_act_time.json]
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
from simpledet_amd._lib import lib  # noqa: E402

# (site, shape, bias, residual, act)
SITES = (("stem", (2, 64, 400, 672), True, False, True),
         ("stage1_inner", (2, 64, 200, 336), True, False, True),
         ("stage1_out", (2, 256, 200, 336), True, True, True),
         ("stage2_out", (2, 512, 100, 168), True, True, True),
         ("stage3_out", (2, 1024, 50, 84), True, True, True),
         ("stage4_out", (2, 2048, 25, 42), True, True, True),
         ("broadcast_scale", (2, 256, 200, 336), False, False, False))


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
    return out


def both_ways(fn, iters, nsets):
    e = time_events(fn, iters, nsets)
    gs = graphs_of(fn, nsets)
    g = time_events(lambda i: gs[i].replay(), iters, nsets)
    del gs
    return round(e, 1), round(g, 1)


def dispatch():
    return (lib().cdll.sd_last_dispatch() or b"").decode()


def composition(x, g, b, r, act):
    v = x * g.view(1, -1, 1, 1)
    if b is not None:
        v = v + b.view(1, -1, 1, 1)
    if r is not None:
        v = v + r
    return torch.where(v > 0, v, torch.zeros_like(v)) if act else v


def measure(site, shape, bias, residual, act, dt, iters, nsets, gen):
    N, C = shape[:2]
    n = int(np.prod(shape))
    esz = 4 if dt == torch.float32 else 2
    rnd = lambda s: torch.randn(s, device="cuda", generator=gen).to(dt)
    xs = [rnd(shape) for _ in range(nsets)]
    rs = [rnd(shape) for _ in range(nsets)] if residual else [None] * nsets
    dys = [rnd(shape) for _ in range(nsets)]
    gamma, beta = (rnd((C,)) + 1).contiguous(), (rnd((C,)) if bias else None)
    a = "relu" if act else None
    y, dx = torch.empty_like(xs[0]), torch.empty_like(xs[0])
    dres = torch.empty_like(xs[0]) if residual else None
    # every set's own y: the backward of set i reads the forward of set i
    ys = [ops.scale_bias_act_forward(xs[i], gamma, beta, rs[i], a) for i in range(nsets)] if act else [None] * nsets

    def fwd(i):
        ops.scale_bias_act_forward(xs[i], gamma, beta, rs[i], a, out=y)

    def bwd(i):
        ops.scale_bias_act_backward(dys[i], ys[i], gamma, a, dx=dx, dres=dres)
    fwd(0)
    d_f = dispatch()
    bwd(0)
    d_b = dispatch()
    # the torch composition; its backward is autograd over a forward graph built once per set, outside the clock
    def t_fwd(i):
        with torch.no_grad():
            composition(xs[i], gamma, beta, rs[i], act)
    leaves, outs = [], []
    for i in range(nsets):
        xl = xs[i].clone().requires_grad_()
        rl = rs[i].clone().requires_grad_() if residual else None
        leaves.append((xl,) + ((rl,) if residual else ()))
        outs.append(composition(xl, gamma, beta, rl, act))

    def t_bwd(i):
        torch.autograd.grad(outs[i], leaves[i], dys[i], retain_graph=True)
    passes = dict(fwd=2 + int(residual), bwd=2 + int(act) + int(residual))
    r = dict(shape=list(shape), dtype=str(dt).replace("torch.", ""), bias=bias, residual=residual, act=act,
             dispatch_fwd=d_f, dispatch_bwd=d_b)
    ok = True
    for key, ours, theirs in (("fwd", fwd, t_fwd), ("bwd", bwd, t_bwd)):
        bytes_ = passes[key] * n * esz
        half = bytes_ // 2
        src = [torch.empty(half, dtype=torch.uint8, device="cuda") for _ in range(nsets)]
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        e, g = both_ways(ours, iters, nsets)
        te, tg = both_ways(theirs, iters, nsets)
        ce, cg = both_ways(lambda i: dst.copy_(src[i]), iters, nsets)
        del src, dst
        r[key] = dict(eager_us=e, graph_us=g, torch_eager_us=te, torch_graph_us=tg, copy_eager_us=ce,
                      copy_graph_us=cg, algorithmic_bytes=bytes_, tensor_passes=passes[key],
                      TBps=round(bytes_ / g * 1e-6, 3), fraction_of_copy=round(cg / g, 3),
                      speedup_over_torch_graph=round(tg / g, 2))
        ok = ok and g <= tg
    r["not_slower_than_torch"] = bool(ok)
    # the backward with the beta gradient (not the normal case: fixed_param holds beta): two more kernels in front,
    # which read dy (and y) once more
    dbeta = torch.empty(C, device="cuda")
    ws = torch.empty(ops.scale_bias_act_workspace_bytes(N, C, n // (N * C)), dtype=torch.uint8, device="cuda")

    def bwd_dbeta(i):
        ops.scale_bias_act_backward(dys[i], ys[i], gamma, a, dx=dx, dres=dres, dbeta=dbeta, workspace=ws)
    e, g = both_ways(bwd_dbeta, iters, nsets)
    r["bwd_with_dbeta"] = dict(eager_us=e, graph_us=g, dispatch=dispatch(),
                               extra_bytes=(1 + int(act)) * n * esz, over_bwd=round(g / r["bwd"]["graph_us"], 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scale_bias_act_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    with torch.cuda.stream(torch.cuda.Stream()):
        for site, shape, bias, residual, act in SITES:
            for dt in (torch.float32, torch.float16):
                name = "%s_%s" % (site, "f32" if dt == torch.float32 else "f16")
                res[name] = measure(site, shape, bias, residual, act, dt, args.iters, nsets, gen)
                print(name, json.dumps(res[name]), flush=True)
                torch.cuda.empty_cache()
    slower = sorted(k for k, v in res.items() if not v["not_slower_than_torch"])
    res["summary"] = dict(not_slower_than_torch_everywhere=not slower, slower_than_torch=slower)
    res["config"] = dict(input_sets=nsets, iters=args.iters, device=torch.cuda.get_device_name(0))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"scale_bias_act": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"scale_bias_act": res["summary"]}))


if __name__ == "__main__":
    main()
