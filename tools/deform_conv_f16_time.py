#!/usr/bin/env python
"""Timing of DeformableConvolution on float16 tensors (simpledet_amd/csrc/deform_fused_f16.hip).

Forward, per shape, in one run, the variants alternating pass by pass, each pass over a rotation of input sets (so
no call finds its inputs in L2 from the one before):
  f16          sd_deform_convolution_fwd_f16 (the col-free kernel on native-half matrix-core operands), eagerly and
               as ONE captured HIP graph
  composition  what a half graph had to do before: cast x / offset / weight (/ bias) to float32, the fused float32
               forward (keep_col = 0), cast y to float16; eagerly only: the float32 forward clears its operand maxima
               with hipMemsetAsync, and this project's captured graphs are kept to kernel nodes (its graph tests
               replay kernel-only graphs), so no memset node is recorded here.  `forward_speedup` is eager over eager.
Backward: sd_deform_convolution_bwd_f16 (casts + the float32 backward + casts) against the float32 backward alone,
eagerly, for the same reason (the float32 backward clears d_weight and its maxima with hipMemsetAsync).
Weight gradient without a col matrix (csrc/deform_wgrad_f16.hip), the paths alternating in one run on the
rotating inputs: (a) the whole backward, sd_deform_convolution_bwd_f16 against sd_deform_convolution_bwd_f16_fused;
(b) the weight gradient alone (req null for the rest): widen + im2col + product against the new kernel + its reduce;
(c) the parent's whole backward timed a second time in the same rotation: the run's own spread.  `--only-fused` runs
just the fused weight gradient (for a kernel trace in a run of its own).
Data and offset gradients on the half operands (csrc/deform_igrad_f16.hip), medians of `--native-iters`
(12) in the same rotation, the parent being sd_deform_convolution_bwd_f16_fused and the native route
sd_deform_convolution_bwd_f16_native with fused_weight_grad: (a) the whole backward; (b) d_data + d_offset alone (req
null for the weight); (c) the parent's two timed a second time: the spread.  `--only-native` times just these and
updates the rows of the existing file; `--only-igrad` runs the native d_data + d_offset alone (for a kernel trace).
A pyramid of problems in one launch (csrc/deform_pyramid_f16.hip), the `pconv` rows: the deformable part
of one PConv of the sepc neck (N = 2, C = F = 256, levels 100x168 .. 7x11, start_level 1) as (a) the 11 single calls
plus the fp16 torch adds / interpolate(nearest) / crop a half graph runs today and (b) the two pyramid launches, eagerly
and (b) as one captured graph; launch 2 alone against its eight single calls; (a) timed a second time in the same
rotation: the spread.  `--only-pconv` times just these and updates the existing file.

Shapes: the README's DCN row (16, 256, 50, 84) dg 4 -> 256, and the sepc neck's (2, 256, 100, 168) and
(2, 256, 50, 84) at stride 1 and 2, dg 1, with a bias.  Every shape at the two offset spreads bench_ops.py's DCN row
reports: offsets ~ N(0, 2^2) (its headline) and N(0, 0.5^2) (its trained-layer case).  The spread decides how many
(tile, group) windows fit the LDS buffers; `window_fit` is that fraction, computed on the host from the offsets the
way the kernel does (one contiguous position range per tile and deformable group, against its capacity).
Bytes: x + offset + weight + bias + y once, in halves.  fp16 MFMA fraction: 2 N F Ho Wo 9 C flop over the time over
2.5e15 flop/s (dense fp16 matrix-core peak of the MI355X).

    python tools/deform_conv_f16_time.py [--iters 20] [--out profiles/deform_conv_f16_time.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import deform_conv_f16 as d16, ops  # noqa: E402

PEAK_F16 = 2.5e15
SETS = 4
SIGMAS = (2.0, 0.5)
TILE, MAX_WINDOW, NUM_CU = 64, 1536, 256   # kHN, kHMaxW of csrc/deform_fused_f16.hip
# name: (N, C, H, W, F, dg, stride, bias)
SHAPES = dict(readme_dcn=(16, 256, 50, 84, 256, 4, 1, False),
              sepc_100x168_s1=(2, 256, 100, 168, 256, 1, 1, True), sepc_100x168_s2=(2, 256, 100, 168, 256, 1, 2, True),
              sepc_50x84_s1=(2, 256, 50, 84, 256, 1, 1, True), sepc_50x84_s2=(2, 256, 50, 84, 256, 1, 2, True))


def inputs(shape, seed, sigma):
    N, C, H, W, F, dg, stride, bias = shape
    gen = torch.Generator(device="cuda").manual_seed(seed)
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    r = lambda *s: torch.randn(s, device="cuda", generator=gen)   # noqa: E731
    return (r(N, C, H, W).half(), (r(N, 18 * dg, Ho, Wo) * sigma).half(), (r(F, C, 3, 3) * 0.05).half(),
            r(F).half() if bias else None)


def window_fit(off, shape):
    """fraction of (image, tile, group) windows of at most MAX_WINDOW positions: the host's tile rule and the kernel's
    window rule of csrc/deform_fused_f16.hip, on the real offsets"""
    N, C, H, W, F, dg, stride, _ = shape
    Ho, Wo = off.shape[2:]
    P = Ho * Wo
    T = -(-P // TILE)
    rounds = -(-N * T // NUM_CU)
    T = max(T, min(rounds * NUM_CU // N, P))
    tile_w = -(-P // T)
    o = off.float().reshape(N, dg, 9, 2, P)
    p = torch.arange(P, device=off.device)
    tap = torch.arange(9, device=off.device).reshape(1, 1, 9, 1)
    h = (p // Wo * stride - 1).reshape(1, 1, 1, P) + tap // 3 + o[:, :, :, 0]
    w = (p % Wo * stride - 1).reshape(1, 1, 1, P) + tap % 3 + o[:, :, :, 1]
    ok = (h >= 0) & (w >= 0) & (h < H) & (w < W)
    hl, wl = h.floor().clamp(0, H - 1), w.floor().clamp(0, W - 1)
    lo = torch.where(ok, hl * W + wl, torch.full_like(h, float("inf")))
    hi = torch.where(ok, (hl + 1).clamp(max=H - 1) * W + (wl + 1).clamp(max=W - 1), torch.full_like(h, -1.0))
    pad = T * tile_w - P
    lo = torch.nn.functional.pad(lo, (0, pad), value=float("inf")).reshape(N, dg, 9, T, tile_w).amin((2, 4))
    hi = torch.nn.functional.pad(hi, (0, pad), value=-1.0).reshape(N, dg, 9, T, tile_w).amax((2, 4))
    count = torch.where(hi >= 0, hi + 1 - torch.nan_to_num(lo, posinf=0.0) + 7, torch.zeros_like(hi))
    return float((count <= MAX_WINDOW).float().mean())


def f16_forward(t, shape):
    return d16.deform_conv_forward(t[0], t[1], t[2], 1, shape[6], 1, shape[5], bias=t[3])


def composition(t, shape):
    b = t[3].float() if t[3] is not None else None
    return ops.deform_conv_forward(t[0].float(), t[1].float(), t[2].float(), 1, shape[6], 1, shape[5], bias=b).half()


def capture(fn, sets, shape):
    """one graph that runs fn on every input set in turn"""
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for t in sets:
            fn(t, shape)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            outs = [fn(t, shape) for t in sets]
    return graph, outs


def time_alternating(runs, iters):
    """runs: {name: callable}; -> {name: median ms per call of the callable}, the callables alternating"""
    times = {k: [] for k in runs}
    for k, run in runs.items():
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    for _ in range(iters):
        for k, run in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b))
    return {k: sorted(v)[len(v) // 2] for k, v in times.items()}


def native_rows(sets, dy, shape, iters):
    """the parent (_bwd_f16_fused) and the native route alternating on the rotating inputs -> the row's native keys"""
    stride, dg = shape[6], shape[5]
    j = [0]

    def bwd(native, req, step=False):
        def run():
            k = j[0] % SETS
            j[0] += step
            d16.deform_conv_backward(dy[k], *sets[k][:3], 1, stride, 1, dg, req=req, fused_weight_grad=True,
                                     fused_input_grads=native)
        return run

    whole, inp = ("write",) * 3, ("write", "write", "null")
    t = time_alternating(dict(parent=bwd(False, whole), native=bwd(True, whole), parent_in=bwd(False, inp),
                              native_in=bwd(True, inp), parent_again=bwd(False, whole),
                              parent_in_again=bwd(False, inp, True)), iters)
    return dict(native_iters=iters, backward_fused_parent_ms=round(t["parent"], 4),
                backward_native_ms=round(t["native"], 4), backward_fused_parent_again_ms=round(t["parent_again"], 4),
                backward_native_speedup=round(t["parent"] / t["native"], 3),
                input_grads_parent_ms=round(t["parent_in"], 4), input_grads_native_ms=round(t["native_in"], 4),
                input_grads_parent_again_ms=round(t["parent_in_again"], 4),
                input_grads_speedup=round(t["parent_in"] / t["native_in"], 3))


PCONV_LEVELS = ((100, 168), (50, 84), (25, 42), (13, 21), (7, 11))   # P3..P7 of 800 x 1333; start_level 1


def pconv_inputs(seed, sigma, N=2, C=256):
    """one PConv's deformable part (models/sepc/sepc_neck.py:PConvModule): x of five levels, the three shared weights
    and biases, and the offsets of its 11 convolutions: sepc1 on x[1..4], sepc2 (stride 2) on x[0..3], sepc0 on x[2..4]"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    r = lambda *s: torch.randn(s, device="cuda", generator=gen)   # noqa: E731
    x = [r(N, C, h, w).half() for h, w in PCONV_LEVELS]
    off = {k: {l: (r(N, 18, *PCONV_LEVELS[l + (k == 0)]) * sigma).half() for l in range(1, 5 - (k == 0))} for k in range(3)}
    return dict(x=x, off=off, w=[(r(C, C, 3, 3) * 0.05).half() for _ in range(3)], b=[r(C).half() for _ in range(3)])


def pconv_calls(s, l):
    """the (sepc1, sepc2, sepc0) sources of output level l"""
    src = lambda k, xl, stride: (s["x"][xl], s["off"][k][l], s["w"][k], s["b"][k], 1, stride, 1, 1)   # noqa: E731
    return src(1, l, 1), src(2, l - 1, 2), (src(0, l + 1, 1) if l < 4 else None)


def _single(v):
    return d16.deform_conv_forward(v[0], v[1], v[2], v[4], v[5], v[6], v[7], bias=v[3])


def pconv_graph_route(s):
    """route (a), what a half graph runs today: 11 calls, the fp16 adds, UpSampling(nearest) -> slice_like"""
    ys = []
    for l in range(1, 5):
        one, two, zero = pconv_calls(s, l)
        t = _single(one) + _single(two)
        if zero is not None:
            up = torch.nn.functional.interpolate(_single(zero), scale_factor=2, mode="nearest")
            t = t + up[:, :, :t.shape[2], :t.shape[3]]
        ys.append(t)
    return ys


def pconv_launch1(s):
    return d16.deform_conv_pyramid_forward([dict(sources=[pconv_calls(s, l)[2]]) for l in range(1, 4)])


def pconv_launch2(s, res):
    return d16.deform_conv_pyramid_forward([dict(sources=list(pconv_calls(s, l)[:2]),
                                                 residual=(res[l - 1], 1) if l < 4 else None) for l in range(1, 5)])


def pconv_rows(iters):
    """route (a) against route (b) = the two pyramid launches, alternating on rotating input sets; (b) also as one
    captured graph; launch 2 alone against its eight single calls; route (a) a second time: the run's own spread"""
    rows = {}
    for sigma in SIGMAS:
        sets = [pconv_inputs(s, sigma) for s in range(SETS)]
        res = [pconv_launch1(s) for s in sets]
        graph, outs = capture(lambda s, _: pconv_launch2(s, pconv_launch1(s)), sets, None)
        graph.replay()
        torch.cuda.synchronize()
        want = [pconv_graph_route(s) for s in sets]
        diff = max(float((a.float() - b.float()).abs().max()) for o, w in zip(outs, want) for a, b in zip(o, w))
        over = lambda fn: (lambda: [fn(s) for s in sets])   # noqa: E731
        eight = lambda s: [_single(v) for l in range(1, 5) for v in pconv_calls(s, l)[:2]]   # noqa: E731
        launch2_alone = lambda: [pconv_launch2(s, r) for s, r in zip(sets, res)]   # noqa: E731
        t = time_alternating(dict(a=over(pconv_graph_route), b=over(lambda s: pconv_launch2(s, pconv_launch1(s))),
                                  b_graph=graph.replay, a_again=over(pconv_graph_route), eight=over(eight),
                                  launch2=launch2_alone), iters)
        t = {key: v / SETS for key, v in t.items()}
        spread = abs(t["a"] - t["a_again"])
        rows["pconv/sigma%g" % sigma] = dict(
            offset_sigma=sigma, levels=[list(v) for v in PCONV_LEVELS], N=2, C=256, F=256, start_level=1,
            graph_route_ms=round(t["a"], 4), graph_route_again_ms=round(t["a_again"], 4),
            pyramid_route_ms=round(t["b"], 4), pyramid_route_graph_ms=round(t["b_graph"], 4),
            pyramid_over_graph_route=round(t["b"] / t["a"], 3),
            pyramid_not_slower_within_spread=bool(t["b"] <= t["a"] + spread),
            launch2_ms=round(t["launch2"], 4), launch2_eight_calls_ms=round(t["eight"], 4),
            launch2_over_eight_calls=round(t["launch2"] / t["eight"], 3), max_abs_diff_between_routes=diff,
            max_abs_y=max(float(b.float().abs().max()) for w in want for b in w))
        print("pconv/sigma%g" % sigma, json.dumps(rows["pconv/sigma%g" % sigma]))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only-pconv", action="store_true", help="the pyramid routes alone, into the file's `pconv` rows")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deform_conv_f16_time.json"))
    ap.add_argument("--only-fused", action="store_true", help="the fused weight gradient alone, readme_dcn, no file")
    ap.add_argument("--native-iters", type=int, default=12)
    ap.add_argument("--only-native", action="store_true", help="the native input gradients alone, into the file's rows")
    ap.add_argument("--only-igrad", action="store_true", help="native d_data + d_offset alone, readme_dcn, no file")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    if args.only_igrad:
        shape = SHAPES["readme_dcn"]
        for sigma in SIGMAS:
            t = inputs(shape, 0, sigma)
            dy = torch.randn(f16_forward(t, shape).shape, device="cuda").half()
            for _ in range(args.iters):
                d16.deform_conv_backward(dy, *t[:3], 1, shape[6], 1, shape[5], req=("write", "write", "null"),
                                         fused_weight_grad=True, fused_input_grads=True)
        torch.cuda.synchronize()
        return
    if args.only_pconv:
        with open(args.out) as f:
            result = json.load(f)
        result["pconv"] = pconv_rows(args.iters)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    if args.only_native:
        with open(args.out) as f:
            result = json.load(f)
        for name, shape in SHAPES.items():
            for sigma in SIGMAS:
                sets = [inputs(shape, s, sigma) for s in range(SETS)]
                dy = [torch.randn(f16_forward(t, shape).shape, device="cuda").half() for t in sets]
                key = "%s/sigma%g" % (name, sigma)
                result["shapes"][key].update(native_rows(sets, dy, shape, args.native_iters))
                print(key, json.dumps(result["shapes"][key]))
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        return
    if args.only_fused:
        shape = SHAPES["readme_dcn"]
        t = inputs(shape, 0, SIGMAS[0])
        dy = torch.randn(f16_forward(t, shape).shape, device="cuda").half()
        for _ in range(args.iters):
            d16.deform_conv_backward(dy, *t[:3], 1, shape[6], 1, shape[5], req=("null", "null", "write"),
                                     fused_weight_grad=True)
        torch.cuda.synchronize()
        return
    result = dict(device=torch.cuda.get_device_name(0), iters=args.iters, input_sets=SETS, offset_sigmas=list(SIGMAS),
                  shapes={})
    for name, shape in SHAPES.items():
        for sigma in SIGMAS:
            N, C, H, W, F, dg, stride, bias = shape
            sets = [inputs(shape, s, sigma) for s in range(SETS)]
            g16, o16 = capture(f16_forward, sets, shape)
            oco = [composition(t, shape) for t in sets]
            g16.replay()
            torch.cuda.synchronize()
            diff = max(float((a.float() - b.float()).abs().max()) for a, b in zip(o16, oco))
            ymax = max(float(b.float().abs().max()) for b in oco)
            t = time_alternating(dict(graph=g16.replay, f16=lambda: [f16_forward(v, shape) for v in sets],
                                      composition=lambda: [composition(v, shape) for v in sets]), args.iters)
            f16_ms, comp_ms, graph_ms = t["f16"] / SETS, t["composition"] / SETS, t["graph"] / SETS
            Ho, Wo = o16[0].shape[2:]
            flop = 2.0 * N * F * Ho * Wo * 9 * C
            nbytes = 2 * (N * C * H * W + N * 18 * dg * Ho * Wo + F * C * 9 + (F if bias else 0) + N * F * Ho * Wo)
            dy = [torch.randn(o.shape, device="cuda").half() for o in o16]
            dyf, setsf = [d.float() for d in dy], [[v.float() if v is not None else None for v in s] for s in sets]
            i = [0]

            def bwd16():
                k = i[0] % SETS
                d16.deform_conv_backward(dy[k], *sets[k][:3], 1, stride, 1, dg, bias=bias)

            def bwd32():
                k = i[0] % SETS
                i[0] += 1
                ops.deform_conv_backward(dyf[k], *setsf[k][:3], 1, stride, 1, dg, bias=bias)

            tb = time_alternating(dict(f16=bwd16, float32=bwd32), args.iters)
            j = [0]

            def bwd(fused, req, step=False):
                def run():
                    k = j[0] % SETS
                    j[0] += step
                    d16.deform_conv_backward(dy[k], *sets[k][:3], 1, stride, 1, dg, req=req, fused_weight_grad=fused)
                return run

            whole, only_w = ("write",) * 3, ("null", "null", "write")
            tw = time_alternating(dict(parent=bwd(False, whole), fused=bwd(True, whole), parent_again=bwd(False, whole),
                                       parent_dw=bwd(False, only_w), fused_dw=bwd(True, only_w, True)), args.iters)
            key = "%s/sigma%g" % (name, sigma)
            result["shapes"][key] = dict(
                offset_sigma=sigma, window_fit=round(window_fit(sets[0][1], shape), 4),
                shape=dict(N=N, C=C, H=H, W=W, F=F, num_deformable_group=dg, stride=stride, bias=bias),
                forward_f16_graph_ms=round(graph_ms, 4), forward_f16_ms=round(f16_ms, 4),
                forward_composition_ms=round(comp_ms, 4),
                forward_speedup=round(comp_ms / f16_ms, 3), bytes_moved=nbytes,
                achieved_bytes_per_s=round(nbytes / (graph_ms * 1e-3), 0),
                f16_mfma_fraction=round(flop / (graph_ms * 1e-3) / PEAK_F16, 4),
                max_abs_diff_to_composition=diff, max_abs_y=ymax,
                backward_f16_ms=round(tb["f16"], 4), backward_float32_ms=round(tb["float32"], 4),
                backward_ratio=round(tb["f16"] / tb["float32"], 3),
                backward_parent_ms=round(tw["parent"], 4), backward_fused_ms=round(tw["fused"], 4),
                backward_parent_again_ms=round(tw["parent_again"], 4),
                backward_fused_speedup=round(tw["parent"] / tw["fused"], 3),
                weight_grad_parent_ms=round(tw["parent_dw"], 4), weight_grad_fused_ms=round(tw["fused_dw"], 4),
                weight_grad_speedup=round(tw["parent_dw"] / tw["fused_dw"], 3),
                **native_rows(sets, dy, shape, args.native_iters))
            print(key, json.dumps(result["shapes"][key]))
    result["pconv"] = pconv_rows(args.iters)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
