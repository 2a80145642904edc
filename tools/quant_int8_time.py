#!/usr/bin/env python
"""Quantization_int8 timing (simpledet_amd/csrc/quant_int8.hip) at the shapes of config/int8/
faster_r50v1bc4_c5_512roi_1x.py: the activations (2,3,800,1344), (2,64,200,336), (2,256,200,336), (2,1024,50,84),
the weights (64,64,1,1) and (512,512,3,3), and the 53 convolution weights of a ResNet-50 through the
multi-tensor call and as 53 single calls.

Timed from device events, eagerly and as a captured HIP graph: the forward as an activation in its EMA state and
as a weight, the eval forward (no reduction: the element-wise pass alone), and the clip backward.  Algorithmic
bytes: forward 4n read twice + 4n written, backward 8n read + 4n written, 12n each; reported as a fraction of
8 TB/s.  The floor is the repository's streaming copy moving the same 12n bytes (6n copied).  The comparator,
timed in the same run on the same tensors, is a torch composition of the same expressions -- abs().amax(),
clamp, div, round, mul and the EMA, with .item() where the reference copies the threshold to the host (so it
cannot be captured).  NSETS input sets are rotated between calls.

    python tools/quant_int8_time.py [--iters 50] [--sets 3] [--out profiles/quant_int8_time.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops  # noqa: E402
from simpledet_amd._lib import lib  # noqa: E402

PEAK = 8.0e12
ACTS = ((2, 3, 800, 1344), (2, 64, 200, 336), (2, 256, 200, 336), (2, 1024, 50, 84))
WEIGHTS = ((64, 64, 1, 1), (512, 512, 3, 3))
DECAY = 0.99


def resnet50_conv_shapes():
    shapes = [(64, 3, 7, 7)]
    cin = 64
    for width, blocks in ((64, 3), (128, 4), (256, 6), (512, 3)):
        for b in range(blocks):
            shapes += [(width, cin, 1, 1), (width, width, 3, 3), (4 * width, width, 1, 1)]
            if b == 0:
                shapes.append((4 * width, cin, 1, 1))
            cin = 4 * width
    assert len(shapes) == 53
    return shapes


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


def both_ways(fn, iters, nsets, capture=True):
    r = dict(eager_us=round(time_events(fn, iters, nsets), 1), graph_us=None)
    if capture:
        gs = graphs_of(fn, nsets)
        r["graph_us"] = round(time_events(lambda i: gs[i].replay(), iters, nsets), 1)
        del gs
    return r


def torch_fwd(x, mm, is_weight):
    m = x.abs().amax()
    if is_weight:
        mm.copy_(m.reshape(1))
    else:
        mm.mul_(DECAY).add_((1.0 - DECAY) * m)
    t = mm.item()                       # the reference's blocking copy of the threshold
    u = t / 127.0
    c = x if is_weight else x.clamp(-t, t)
    return c.div(u).round().mul(u)


def torch_bwd(g, x, mm):
    t = mm.item()
    return torch.where((x >= -t) & (x <= t), g, torch.zeros((), device=g.device))


def stream_copy_us(nbytes, iters):
    src = [torch.empty(nbytes, device="cuda", dtype=torch.uint8) for _ in range(3)]
    dst = torch.empty(nbytes, device="cuda", dtype=torch.uint8)

    def fn(i):
        lib().call("sd_hbm_stream_copy", ctypes.c_void_p(src[i].data_ptr()), ctypes.c_void_p(dst.data_ptr()),
                   ctypes.c_size_t(nbytes), 16, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return round(time_events(fn, iters, 3), 1)


def one_shape(shape, is_weight, iters, nsets, gen):
    n = int(np.prod(shape))
    xs = [torch.randn(shape, device="cuda", generator=gen) for _ in range(nsets)]
    gs = [torch.randn(shape, device="cuda", generator=gen) for _ in range(nsets)]
    out, d = torch.empty(shape, device="cuda"), torch.empty(shape, device="cuda")
    mm = torch.full((1,), 3.0, device="cuda")
    state = ops.quant_int8_state(0)
    if not is_weight:
        state[1] = 0                    # past the init step: every timed call is an EMA step
    ws = torch.empty(ops.quant_int8_workspace_bytes(n), device="cuda", dtype=torch.uint8)
    r = dict(shape=list(shape), n=n, algorithmic_bytes=12 * n)

    def fwd(i):
        ops.quantization_int8_forward(xs[i], mm, state, is_weight=is_weight, ema_decay=DECAY, out=out, workspace=ws)

    def fwd_eval(i):
        ops.quantization_int8_forward(xs[i], mm, state, is_weight=is_weight, is_train=False, out=out, workspace=ws)

    def bwd(i):
        ops.quantization_int8_backward(gs[i], xs[i], mm, is_weight=False, grad_mode="clip", d_data=d)
    r["fwd"] = both_ways(fwd, iters, nsets)
    r["fwd_eval_pass2_only"] = both_ways(fwd_eval, iters, nsets)
    r["bwd_clip"] = both_ways(bwd, iters, nsets)
    for k in ("fwd", "bwd_clip"):
        r[k]["fraction_of_8TBps"] = round(12 * n / PEAK * 1e6 / r[k]["graph_us"], 3)
    r["stream_copy_same_bytes_us"] = stream_copy_us(6 * n, iters)
    tmm = torch.full((1,), 3.0, device="cuda")
    r["torch_fwd"] = both_ways(lambda i: torch_fwd(xs[i], tmm, is_weight), iters, nsets, capture=False)
    r["torch_bwd_clip"] = both_ways(lambda i: torch_bwd(gs[i], xs[i], tmm), iters, nsets, capture=False)
    r["not_slower_than_torch"] = dict(fwd_eager=r["fwd"]["eager_us"] <= r["torch_fwd"]["eager_us"],
                                      fwd_graph=r["fwd"]["graph_us"] <= r["torch_fwd"]["eager_us"],
                                      bwd_eager=r["bwd_clip"]["eager_us"] <= r["torch_bwd_clip"]["eager_us"],
                                      bwd_graph=r["bwd_clip"]["graph_us"] <= r["torch_bwd_clip"]["eager_us"])
    return r


def resnet50_weights(iters, gen):
    shapes = resnet50_conv_shapes()
    T = len(shapes)
    xs = [torch.randn(s, device="cuda", generator=gen) * 0.05 for s in shapes]
    outs = [torch.empty_like(x) for x in xs]
    mms = [torch.zeros(1, device="cuda") for _ in xs]
    sts = [ops.quant_int8_state(0) for _ in xs]
    n_total = sum(x.numel() for x in xs)
    table = ops.quant_int8_weights_table(xs, outs, mms, sts)
    wsm = torch.empty(ops.quant_int8_weights_workspace_bytes(T, n_total), device="cuda", dtype=torch.uint8)
    ws1 = torch.empty(ops.quant_int8_workspace_bytes(n_total), device="cuda", dtype=torch.uint8)

    def multi(_):
        ops.quantization_int8_weights_forward(xs, mms, sts, outs=outs, table=table, workspace=wsm)

    def singles(_):
        for x, o, m, s in zip(xs, outs, mms, sts):
            ops.quantization_int8_forward(x, m, s, is_weight=True, out=o, workspace=ws1)
    r = dict(tensors=T, n_total=n_total, algorithmic_bytes=12 * n_total)
    r["multi_tensor_call"] = both_ways(multi, iters, 1)
    multi(0)
    want = [o.clone() for o in outs]
    r["single_calls"] = both_ways(singles, iters, 1)
    r["bit_equal"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(want, outs))
    r["multi_tensor_call"]["fraction_of_8TBps"] = round(12 * n_total / PEAK * 1e6 / r["multi_tensor_call"]["graph_us"], 3)
    tmm = [torch.zeros(1, device="cuda") for _ in xs]
    r["torch_53_compositions"] = both_ways(lambda _: [torch_fwd(x, m, True) for x, m in zip(xs, tmm)], iters, 1,
                                           capture=False)
    r["multi_beats_single_calls"] = dict(eager=r["multi_tensor_call"]["eager_us"] < r["single_calls"]["eager_us"],
                                         graph=r["multi_tensor_call"]["graph_us"] < r["single_calls"]["graph_us"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_int8_time.json"))
    args = ap.parse_args()
    nsets = max(3, args.sets)
    gen = torch.Generator(device="cuda").manual_seed(1)
    res = {}
    for kind, shapes in (("activation", ACTS), ("weight", WEIGHTS)):
        for shape in shapes:
            name = "%s_%s" % (kind, "x".join(str(s) for s in shape))
            res[name] = one_shape(shape, kind == "weight", args.iters, nsets, gen)
            print(name, json.dumps(res[name]), flush=True)
            torch.cuda.empty_cache()
    res["resnet50_conv_weights"] = resnet50_weights(args.iters, gen)
    print("resnet50_conv_weights", json.dumps(res["resnet50_conv_weights"]), flush=True)
    res["config"] = dict(input_sets=nsets, iters=args.iters, ema_decay=DECAY)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"quant_int8": res}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
