#!/usr/bin/env python
"""_contrib_SyncBatchNorm timing at the syncbn sites of the reference's configs, at each config's own batch and
image size:

  config/FPG/faster_r50v1b_pafpn3@256_syncbn_1x.py (NormalizeParam syncbn: backbone AND neck; batch_image 2,
      800 x 1333, feature maps 200x334 ... 13x21 as its RpnParam.anchor_generate lists them): the ResNet-50 stage
      outputs from the stem (64 channels at stride 2) to stage 4 (2048 channels at stride 32), and the five 256-channel
      neck maps at strides 4 to 64;
  config/FPG/faster_r50v1b_fpg6@128_syncbn_1x.py (NeckParam syncbn, dim_reduced 128): the stride-4 neck map;
  config/NASFPN/retina_r50v1b_nasfpn_640_7@256_25epoch.py (batch_image 8, 640 x 640, dim_reduced 256): the neck maps
      80x80 ... 5x5.

One rank (gather=None: no collective; RCCL between GPUs is not measured, one GPU is available per run).  Timed from
device events, eagerly and as one captured HIP graph: the forward (statistics + apply), the backward (sums + apply),
and both; float32 and float16 data.  Algorithmic bytes per element: forward 3 accesses (x twice, y once), backward 5
(dy and x twice, dx once): 12 / 20 bytes in float32, 6 / 10 in float16; reported as a fraction of 8 TB/s.  Input
sets are rotated between calls so that no call finds its inputs in the 256 MB Infinity Cache from the call before.
WITHIN a call the second read of x (and dy) of a tensor under 256 MB may still be served from that cache:
`second_read_may_hit_infinity_cache` says so per shape, and the fraction is then an effective rate over the
algorithmic bytes, NOT an HBM rate.  In the same run, on the same tensors (the parent commit has no path for this):
torch.nn.functional.batch_norm(training=True) forward + backward through autograd, and a torch composition of the
reference's passes (sync_batch_norm-inl.h:333-357, :476-513).  Also stored under 'margin': the worst k_gpu and the
k_ref there of tests/test_sync_bn.py's statistics check, for W = 1, 2, 3 (tests/sync_bn_ref.py).

    python tools/sync_bn_time.py [--iters 30] [--out profiles/sync_bn_time.json]
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
from tests import sync_bn_ref as sr  # noqa: E402

EPS = 1e-3
PEAK = 8.0e12
MALL = 256 << 20
SHAPES = (("r50_stem", (2, 64, 400, 667)), ("r50_stage1", (2, 256, 200, 334)), ("r50_stage2", (2, 512, 100, 167)),
          ("r50_stage3", (2, 1024, 50, 84)), ("r50_stage4", (2, 2048, 25, 42)),
          ("pafpn_p2", (2, 256, 200, 334)), ("pafpn_p3", (2, 256, 100, 167)), ("pafpn_p4", (2, 256, 50, 84)),
          ("pafpn_p5", (2, 256, 25, 42)), ("pafpn_p6", (2, 256, 13, 21)), ("fpg128_p2", (2, 128, 200, 334)),
          ("nasfpn_p3", (8, 256, 80, 80)), ("nasfpn_p4", (8, 256, 40, 40)), ("nasfpn_p5", (8, 256, 20, 20)),
          ("nasfpn_p6", (8, 256, 10, 10)), ("nasfpn_p7", (8, 256, 5, 5)))


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


def reference_passes(x, dy, gamma, beta):
    """the reference's tensor passes for one rank, in float32 as it computes (a half tensor is cast first, :311-314):
    E[x], E[x^2], var, the normalising pass; sum dy, sum dy * (x - mean), the gamma gradient, the data gradient"""
    x, dy = x.float(), dy.float()
    C = x.shape[1]
    v = lambda t: t.view(1, C, 1, 1)
    scale = 1.0 / (x.numel() // C)
    mean = x.sum(dim=(0, 2, 3)) * scale
    var = (x * x).sum(dim=(0, 2, 3)) * scale - mean * mean
    y = v(gamma) * (x - v(mean)) / torch.sqrt(v(var + EPS)) + v(beta)
    sum_grad = dy.sum(dim=(0, 2, 3))
    sum_prod = (dy * (x - v(mean))).sum(dim=(0, 2, 3))
    gvar = -0.5 * sum_prod * gamma * torch.pow(var + EPS, -1.5)
    gmean = sum_grad * gamma * (-1.0 / torch.sqrt(var + EPS))
    dgamma = (dy * (x - v(mean)) / torch.sqrt(v(var + EPS))).sum(dim=(0, 2, 3))
    dx = (dy * v(gamma)) * v(1.0 / torch.sqrt(var + EPS)) + v(gvar) * scale * 2.0 * (x - v(mean)) + v(gmean) * scale
    return y, dx, dgamma, sum_grad


def k_margin():
    """tests/test_sync_bn.py's statistics check: per W and output the worst k of the GPU and the restatement's k on
    that case, and both maxima over the zero-offset cases"""
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    res = {}
    cases = sr.cases()
    for W in (1, 2, 3):
        worst = {o: dict(k_gpu=0.0, k_ref_there=0.0, case=None, k_gpu_zero_offset=0.0, k_ref_zero_offset=0.0,
                         k_ref_max=0.0) for o in sr.STAT_OUTPUTS}
        for name, c in cases:
            if W > 1 and c["x"].shape[0] != 6:
                continue
            truth, T, k_ref, _, _ = sr.evaluate(c, W)
            g, b = cu(c["gamma"]), cu(c["beta"])
            xs, dys = [cu(a) for a in sr.slices(c["x"], W)], [cu(a) for a in sr.slices(c["dy"], W)]
            parts = torch.stack([ops.sync_bn_stats(x) for x in xs])
            _, mean, var = ops.sync_bn_apply(xs[0], parts, g, b, c["eps"], c["fix_gamma"])
            bparts = torch.stack([ops.sync_bn_bwd_stats(dy, x, mean) for dy, x in zip(dys, xs)])
            m, v = mean.cpu().numpy(), var.cpu().numpy()
            bt, bT = sr.bwd_truth(c["dy"], c["x"], m, v, c["gamma"], c["eps"], c["fix_gamma"], W)
            bref = sr.bwd_ref32(c["dy"], c["x"], m, v, c["gamma"], c["eps"], c["fix_gamma"], W)
            ks = dict(mean=(sr.k_of(m, truth["mean"], T["mean"]), k_ref["mean"]),
                      var=(sr.k_of(v, truth["var"], T["var"]), k_ref["var"]),
                      bpart=(sr.k_of(bparts.cpu().numpy(), bt["bpart"], bT["bpart"]),
                             sr.k_of(bref["bpart"], bt["bpart"], bT["bpart"])))
            for o, (k, kr) in ks.items():
                w = worst[o]
                w["k_ref_max"] = max(w["k_ref_max"], kr)
                if k > w["k_gpu"]:
                    w.update(k_gpu=k, k_ref_there=kr, case=name)
                if c["offset"] == 0.0:
                    w["k_gpu_zero_offset"] = max(w["k_gpu_zero_offset"], k)
                    w["k_ref_zero_offset"] = max(w["k_ref_zero_offset"], kr)
        res["W%d" % W] = {o: {k: (round(v, 3) if isinstance(v, float) else v) for k, v in w.items()}
                          for o, w in worst.items()}
    return res


def time_shape(shape, dtype, iters, gen):
    N, C = shape[:2]
    HxW = shape[2] * shape[3]
    n = N * C * HxW
    esz = 2 if dtype == torch.float16 else 4
    # enough rotating sets that a call's inputs (x and dy) were pushed out of the Infinity Cache since their last use
    nsets = int(min(12, max(3, -(-2 * MALL // (2 * n * esz)) + 1)))
    xs = [(torch.randn(shape, device="cuda", generator=gen) + 0.5).to(dtype) for _ in range(nsets)]
    dys = [torch.randn(shape, device="cuda", generator=gen).to(dtype) for _ in range(nsets)]
    gamma = torch.randn(C, device="cuda", generator=gen)
    beta = torch.randn(C, device="cuda", generator=gen)
    y, dx = torch.empty_like(xs[0]), torch.empty_like(xs[0])
    part, bpart = torch.empty((2, C), device="cuda"), torch.empty((2, C), device="cuda")
    mean, var = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    dgamma, dbeta = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
    mm, mv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    wsb = ops.sync_bn_workspace_bytes(N, C, HxW)
    ws = [torch.empty(wsb, device="cuda", dtype=torch.uint8) for _ in range(2)]

    def fwd(i):
        ops.sync_bn_stats(xs[i], part=part, workspace=ws[0])
        ops.sync_bn_apply(xs[i], part[None], gamma, beta, EPS, False, y=y, mean=mean, var=var, workspace=ws[0])

    def bwd(i):
        ops.sync_bn_bwd_stats(dys[i], xs[i], mean, bpart=bpart, workspace=ws[1])
        ops.sync_bn_bwd_apply(dys[i], xs[i], mean, var, gamma, bpart[None], 0, EPS, False, dx=dx, dgamma=dgamma,
                              dbeta=dbeta, moving_mean=mm, moving_var=mv, momentum=0.9, workspace=ws[1])

    def both(i):
        fwd(i)
        bwd(i)
    ops.sync_bn_stats(xs[0], part=part, workspace=ws[0])
    d_f = dispatch()
    fwd(0)
    ops.sync_bn_bwd_stats(dys[0], xs[0], mean, bpart=bpart, workspace=ws[1])
    d_b = dispatch()
    bytes_ = dict(fwd=3 * esz * n, bwd=5 * esz * n, fwd_bwd=8 * esz * n)
    r = dict(shape=list(shape), dispatch_stats=d_f, dispatch_bwd_stats=d_b, input_sets=nsets,
             tensor_bytes=n * esz, second_read_may_hit_infinity_cache=bool(n * esz < MALL))
    for key, fn in (("fwd", fwd), ("bwd", bwd), ("fwd_bwd", both)):
        e = time_events(fn, iters, nsets)
        gs = graphs_of(fn, nsets)
        g_us = time_events(lambda i: gs[i].replay(), iters, nsets)
        del gs
        r[key] = dict(eager_us=round(e, 1), graph_us=round(g_us, 1), algorithmic_bytes=bytes_[key],
                      fraction_of_8TBps=round(bytes_[key] / PEAK * 1e6 / g_us, 3))
    # the baselines, forward + backward on the same tensors
    xr = [x.clone().requires_grad_() for x in xs]
    gr_, br_ = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    gt, bt = (gr_, br_) if dtype == torch.float32 else (gr_.to(dtype), br_.to(dtype))

    def torch_bn(i):
        out = torch.nn.functional.batch_norm(xr[i], None, None, gt, bt, training=True, eps=EPS)
        torch.autograd.grad(out, (xr[i], gr_, br_), dys[i])

    def torch_ref(i):
        reference_passes(xs[i], dys[i], gamma, beta)
    r["torch_batch_norm_fwd_bwd_us"] = round(time_events(torch_bn, iters, nsets), 1)
    r["torch_reference_passes_fwd_bwd_us"] = round(time_events(torch_ref, iters, nsets), 1)
    r["not_slower_than_torch"] = bool(r["fwd_bwd"]["eager_us"] <= r["torch_batch_norm_fwd_bwd_us"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bn_time.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sync_bn_time.py measures on the GPU: no device found")
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for name, shape in SHAPES:
        res[name] = {}
        for tag, dtype in (("f32", torch.float32), ("f16", torch.float16)):
            res[name][tag] = time_shape(shape, dtype, args.iters, gen)
            print(name, tag, json.dumps(res[name][tag]), flush=True)
            torch.cuda.empty_cache()
    res["margin"] = k_margin()
    res["config"] = dict(eps=EPS, iters=args.iters, ranks=1, peak_bytes_per_s=PEAK, infinity_cache_bytes=MALL)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"sync_bn": res}, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"sync_bn_margin": res["margin"]}))


if __name__ == "__main__":
    main()
