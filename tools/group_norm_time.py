#!/usr/bin/env python
"""_contrib_GroupNorm timing at the shapes of the GN Mask R-CNN config (config/scratch/
mask_r50v1b_fpn_gn_scratch_2x.py at 800 x 1333, two images): the five FPN neck maps and the two heads, G = 32.

Timed from device events, eagerly and as one captured HIP graph: the forward, the backward, and forward + backward.
Algorithmic bytes per element: forward 8 (x read, y written) where a group is held on chip and 12 where it is split
over workgroups (x read twice); backward 12 and 20; reported as a fraction of 8 TB/s against the 8 / 12 floor.
NSETS input sets are rotated between calls so that nothing is served from the 256 MB MALL (the largest map is
137 MB per tensor).  In the same run, on the same tensors: torch.nn.functional.group_norm forward + backward, and a
torch composition that follows the reference's five passes (moments, rsqrt, normalise; internal gradients, dX,
gamma / beta gradients: operator_cxx/contrib/group_norm.cu).  The parent commit has no GroupNorm, so these two are
the baselines.  Shapes with HxW % 4 == 0 are also timed with every data pointer 4 bytes off its 16-byte boundary
(the 4-byte access kernels).  Also stored: k_ref / k_gpu of tests/test_group_norm.py's margin (tests/group_norm_ref.py).

    python tools/group_norm_time.py [--iters 30] [--sets 3] [--out profiles/group_norm_time.json]
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
from tests import group_norm_ref as gr  # noqa: E402

G, EPS = 32, 1e-5
PEAK = 8.0e12
SHAPES = (("neck_p2", (2, 256, 200, 336)), ("neck_p3", (2, 256, 100, 168)), ("neck_p4", (2, 256, 50, 84)),
          ("neck_p5", (2, 256, 25, 42)), ("neck_p6", (2, 256, 13, 21)), ("bbox_head", (1024, 256, 7, 7)),
          ("mask_head", (256, 256, 14, 14)))


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


def dispatch():
    return (lib().cdll.sd_last_dispatch() or b"").decode()


def five_pass_fwd(x, gamma, beta):
    """Moments (sum x, sum x * x), InvStd, the normalising kernel"""
    N, C = x.shape[:2]
    xg = x.reshape(N, G, -1)
    mu = xg.mean(dim=2)
    var = (xg * xg).mean(dim=2) - mu * mu
    rsig = torch.rsqrt(var + EPS)
    y = (xg - mu[..., None]) * rsig[..., None]
    y = y.reshape(x.shape) * gamma.view(1, C, 1, 1) + beta.view(1, C, 1, 1)
    return y, mu, rsig


def five_pass_bwd(dy, x, mu, rsig, gamma):
    """ComputeInternalGradients, GroupNormBackward, GammaBetaBackward"""
    N, C = x.shape[:2]
    g = gamma.view(1, C, 1, 1)
    n = x[0].numel() // G
    gdy = (g * dy).reshape(N, G, -1)
    xg = x.reshape(N, G, -1)
    ds = (gdy * xg).sum(dim=2)
    db = gdy.sum(dim=2)
    m, r = mu[..., None], rsig[..., None]
    dx = gdy * r + (((db * mu - ds)[..., None]) * (xg - m) * r ** 3 - (db * rsig)[..., None]) / n
    per = dy.reshape(N, G, -1) * (xg - m) * r
    dgamma = per.reshape(N, C, -1).sum(dim=(0, 2))
    dbeta = dy.sum(dim=(0, 2, 3))
    return dx.reshape(x.shape), dgamma, dbeta


def k_margin():
    """per output: the worst k of the GPU and the restatement's k on that case; and both maxima over the zero-offset cases"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    worst = {o: dict(k_gpu=0.0, k_ref_there=0.0, case=None, k_gpu_zero_offset=0.0, k_ref_zero_offset=0.0,
                     k_ref_max=0.0) for o in gr.OUTPUTS}
    for name, c in gr.cases():
        truth, T, k_ref, mu32, rs32 = gr.evaluate(c)
        x, g, b, dy = cu(c["x"]), cu(c["gamma"]), cu(c["beta"]), cu(c["dy"])
        y, mu, rsig = ops.group_norm_forward(x, g, b, c["G"], c["eps"])
        dx, dgamma, dbeta = ops.group_norm_backward(dy, x, cu(mu32), cu(rs32), g, c["G"])
        got = dict(y=y, mu=mu, rsig=rsig, dx=dx, dgamma=dgamma, dbeta=dbeta)
        for o in gr.OUTPUTS:
            k = gr.k_of(got[o].cpu().numpy(), truth[o], T[o])
            w = worst[o]
            w["k_ref_max"] = max(w["k_ref_max"], k_ref[o])
            if k > w["k_gpu"]:
                w.update(k_gpu=k, k_ref_there=k_ref[o], case=name)
            if c["offset"] == 0.0:
                w["k_gpu_zero_offset"] = max(w["k_gpu_zero_offset"], k)
                w["k_ref_zero_offset"] = max(w["k_ref_zero_offset"], k_ref[o])
    return {o: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in w.items()} for o, w in worst.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "group_norm_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for name, shape in SHAPES:
        N, C = shape[:2]
        HxW = shape[2] * shape[3]
        n = N * C * HxW
        xs = [torch.randn(shape, device="cuda", generator=gen) + 0.5 for _ in range(nsets)]
        dys = [torch.randn(shape, device="cuda", generator=gen) for _ in range(nsets)]
        gamma = torch.randn(C, device="cuda", generator=gen)
        beta = torch.randn(C, device="cuda", generator=gen)
        y, dx = torch.empty_like(xs[0]), torch.empty_like(xs[0])
        mu, rsig = torch.empty((N, G), device="cuda"), torch.empty((N, G), device="cuda")
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        wsb = ops.group_norm_workspace_bytes(N, C, HxW, G)
        ws = [torch.empty(wsb, device="cuda", dtype=torch.uint8) for _ in range(2)]

        def fwd(i):
            ops.group_norm_forward(xs[i], gamma, beta, G, EPS, y=y, mu=mu, rsig=rsig, workspace=ws[0])

        def bwd(i):
            ops.group_norm_backward(dys[i], xs[i], mu, rsig, gamma, G, dx=dx, dgamma=dgamma, dbeta=dbeta,
                                    workspace=ws[1])

        def both(i):
            fwd(i)
            bwd(i)
        fwd(0)
        d_f = dispatch()
        bwd(0)
        d_b = dispatch()
        split = "(split)" in d_f, "(split)" in d_b
        bytes_ = dict(fwd=(12 if split[0] else 8) * n, bwd=(20 if split[1] else 12) * n)
        bytes_["fwd_bwd"] = bytes_["fwd"] + bytes_["bwd"]
        floor = dict(fwd=8 * n, bwd=12 * n, fwd_bwd=20 * n)
        r = dict(shape=list(shape), dispatch_fwd=d_f, dispatch_bwd=d_b)
        for key, fn in (("fwd", fwd), ("bwd", bwd), ("fwd_bwd", both)):
            e = time_events(fn, args.iters, nsets)
            gs = graphs_of(fn, nsets)
            g_us = time_events(lambda i: gs[i].replay(), args.iters, nsets)
            del gs
            r[key] = dict(eager_us=round(e, 1), graph_us=round(g_us, 1), algorithmic_bytes=bytes_[key],
                          fraction_of_8TBps=round(bytes_[key] / PEAK * 1e6 / g_us, 3),
                          floor_bytes=floor[key], floor_fraction_of_8TBps=round(floor[key] / PEAK * 1e6 / g_us, 3))
        # the baselines, forward + backward on the same tensors
        xr = [x.clone().requires_grad_() for x in xs]
        gr_, br_ = gamma.clone().requires_grad_(), beta.clone().requires_grad_()

        def torch_gn(i):
            out = torch.nn.functional.group_norm(xr[i], G, gr_, br_, EPS)
            torch.autograd.grad(out, (xr[i], gr_, br_), dys[i])

        def torch_five(i):
            _, m, rs_ = five_pass_fwd(xs[i], gamma, beta)
            five_pass_bwd(dys[i], xs[i], m, rs_, gamma)
        r["torch_group_norm_fwd_bwd_us"] = round(time_events(torch_gn, args.iters, nsets), 1)
        r["torch_five_pass_fwd_bwd_us"] = round(time_events(torch_five, args.iters, nsets), 1)
        r["faster_than_torch_group_norm"] = r["fwd_bwd"]["eager_us"] < r["torch_group_norm_fwd_bwd_us"]
        if HxW % 4 == 0:
            # the same call with x, y, dy and dx 4 bytes off their 16-byte boundary: the 4-byte access kernels
            def off(t):
                buf = torch.empty(t.numel() + 1, device="cuda")
                v = buf[1:].view(t.shape)
                v.copy_(t)
                return v
            xo, dyo = [off(t) for t in xs], [off(t) for t in dys]
            yo, dxo = off(y), off(dx)

            def both_off(i):
                ops.group_norm_forward(xo[i], gamma, beta, G, EPS, y=yo, mu=mu, rsig=rsig, workspace=ws[0])
                ops.group_norm_backward(dyo[i], xo[i], mu, rsig, gamma, G, dx=dxo, dgamma=dgamma, dbeta=dbeta,
                                        workspace=ws[1])
            both_off(0)
            r["offset_pointers"] = dict(dispatch_bwd=dispatch(),
                                        fwd_bwd_eager_us=round(time_events(both_off, args.iters, nsets), 1))
            del xo, dyo, yo, dxo
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del xs, dys, xr, y, dx
        torch.cuda.empty_cache()
    res["margin"] = k_margin()
    res["config"] = dict(num_group=G, eps=EPS, input_sets=nsets, iters=args.iters)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"group_norm": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"group_norm": res["margin"]}))


if __name__ == "__main__":
    main()
