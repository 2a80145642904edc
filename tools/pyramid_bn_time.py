#!/usr/bin/env python
"""Pyramid batch norm timing at the shape of config/sepc/retina_r50v1b_fpn_sepc_1x.py: N = 4 per GPU, C = 256, levels
(100,167), (50,84), (25,42), (13,21), (7,11), float16, ReLU on, one rank.

Two variants, forward and forward + backward (autograd), on the same tensors:
  fused        simpledet_amd.pyramid_bn.pyramid_bn over the level list
  composition  what the project offered before it: torch.cat of the flattened levels -> SyncBatchNormFunction ->
               split -> relu (the reference's graph with the device SyncBatchNorm in it)
Timed from device events around BATCH calls, ALTERNATING the variants (one batch of each per round, so that clocks
and neighbours drift for both alike), NSETS input sets rotated.  The whole measurement is repeated REPEATS times in
the same process; `spread` is (max - min) / median of a variant's repeat medians, and the fused path counts as
faster only where the ratio's distance from 1 exceeds the larger spread.  Before timing, the two variants' outputs
and gradients are compared on the same inputs.  No time is asserted here.

    python tools/pyramid_bn_time.py [--iters 30] [--batch 10] [--repeats 5] [--out profiles/pyramid_bn_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops, pyramid_bn as pb  # noqa: E402
from simpledet_amd._lib import lib  # noqa: E402

N, C = 4, 256
LEVELS = ((100, 167), (50, 84), (25, 42), (13, 21), (7, 11))
EPS = 1e-3


def composition(xs, gamma, beta):
    hxw = [x.shape[2] * x.shape[3] for x in xs]
    cat = torch.cat([x.flatten(2) for x in xs], dim=2)
    y = ops.sync_batch_norm(cat, gamma, beta, eps=EPS, fix_gamma=False)
    return [torch.relu(p).view_as(x) for p, x in zip(torch.split(y, hxw, dim=2), xs)]


def fused(xs, gamma, beta):
    return list(pb.pyramid_bn(xs, gamma, beta, None, None, eps=EPS, fix_gamma=False, relu=True))


def batch_times(fns, iters, batch, nsets):
    """-> per variant the median time of one call in microseconds"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = [[] for _ in fns]
    for i in range(iters):
        for k, fn in enumerate(fns):
            start.record()
            for j in range(batch):
                fn((i + j) % nsets)
            end.record()
            end.synchronize()
            ts[k].append(start.elapsed_time(end) * 1e3 / batch)
    return [float(np.median(t)) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batch", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_bn_time.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this tool measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(1)
    rnd = lambda s: torch.randn(s, device="cuda", generator=gen).half()   # noqa: E731
    sets = [[rnd((N, C) + hw).requires_grad_() for hw in LEVELS] for _ in range(args.sets)]
    dys = [[rnd((N, C) + hw) for hw in LEVELS] for _ in range(args.sets)]
    gamma = (torch.randn(C, device="cuda", generator=gen) * 0.5 + 1.0).requires_grad_()
    beta = torch.randn(C, device="cuda", generator=gen).requires_grad_()
    tensor_bytes = 2 * N * C * sum(h * w for h, w in LEVELS)

    # the same results first: y bit for bit is not promised (the statistics are summed in another order), so the
    # largest difference is reported in units of a half's spacing at 1
    agree = {}
    outs = [v(sets[0], gamma, beta) for v in (fused, composition)]
    grads = [torch.autograd.grad(o, sets[0] + [gamma, beta], dys[0]) for o in outs]
    outs = [[t.detach() for t in o] for o in outs]
    ulp = 2.0 ** -10
    agree["y_max_diff_half_ulps_at_1"] = max(float((a.float() - b.float()).abs().max()) for a, b in zip(*outs)) / ulp
    agree["dx_max_diff_half_ulps_at_1"] = max(float((a.float() - b.float()).abs().max())
                                              for a, b in zip(grads[0][:-2], grads[1][:-2])) / ulp
    agree["dgamma_max_rel_diff"] = float(((grads[0][-2] - grads[1][-2]).abs() / (grads[1][-2].abs() + 1e-3)).max())
    agree["dbeta_max_rel_diff"] = float(((grads[0][-1] - grads[1][-1]).abs() / (grads[1][-1].abs() + 1e-3)).max())
    fused(sets[0], gamma, beta)
    dispatch = (lib().cdll.sd_last_dispatch() or b"").decode()

    def fwd(v):
        def fn(i):
            with torch.no_grad():
                v(sets[i], gamma, beta)
        return fn

    def both(v):
        return lambda i: torch.autograd.grad(v(sets[i], gamma, beta), sets[i] + [gamma, beta], dys[i])
    res = {}
    for key, make, passes in (("fwd", fwd, (3, 9)), ("fwd_bwd", both, (8, 18))):
        fns = [make(fused), make(composition)]
        batch_times(fns, 3, args.batch, args.sets)        # warm-up of both variants at this shape
        torch.cuda.synchronize()
        reps = np.array([batch_times(fns, args.iters, args.batch, args.sets) for _ in range(args.repeats)])
        med = np.median(reps, axis=0)
        spread = (reps.max(axis=0) - reps.min(axis=0)) / med
        ratio = float(med[1] / med[0])
        res[key] = dict(fused_us=round(float(med[0]), 1), composition_us=round(float(med[1]), 1),
                        ratio_composition_over_fused=round(ratio, 3),
                        spread_fused=round(float(spread[0]), 3), spread_composition=round(float(spread[1]), 3),
                        repeat_medians_us=[[round(float(v), 1) for v in r] for r in reps],
                        fused_faster_beyond_spread=bool(ratio - 1.0 > float(spread.max())),
                        tensor_passes_by_reading_the_graph=dict(fused=passes[0], composition=passes[1]),
                        fused_fraction_of_8TBps=round(passes[0] * tensor_bytes / float(med[0]) * 1e-6 / 8.0, 3))
        print(key, json.dumps(res[key]), flush=True)
    res["agreement"] = agree
    res["config"] = dict(N=N, C=C, levels=[list(l) for l in LEVELS], dtype="float16", relu=True, ranks=1,
                         tensor_bytes=tensor_bytes, iters=args.iters, batch=args.batch, repeats=args.repeats,
                         input_sets=args.sets, timing="eager, device events around a batch of calls, autograd included",
                         device=torch.cuda.get_device_name(0), fused_dispatch=dispatch)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"pyramid_bn": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"pyramid_bn": {k: res[k]["ratio_composition_over_fused"] for k in ("fwd", "fwd_bwd")}}))


if __name__ == "__main__":
    main()
