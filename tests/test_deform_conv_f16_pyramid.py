"""A list of fp16 DeformableConvolution problems in one launch (simpledet_amd/deform_conv_f16.py:
deform_conv_pyramid_forward / deform_conv_pyramid, csrc/deform_pyramid_f16.hip) against the fp64 forward
of tests/dcn_torch_ref.py: the sum over a problem's sources plus the residual upsampled and cropped in fp64."""
import pytest
import torch

from .dcn_torch_ref import dcn_col, dcn_forward
from .test_deform_conv_f16 import _half, _inputs


def _up64(r, shift, Ho, Wo):
    return r.double().repeat_interleave(1 << shift, 2).repeat_interleave(1 << shift, 3)[:, :, :Ho, :Wo]


def _build(problems, off1=False, share_w=False, seed=0):
    """problems: [(sources, F, residual, integer)], a source (N, C, H, W, dg, stride, bias) at pad 1 and dilation 1, residual
    None or (Hr, Wr, shift), integer the (max|x|, max|w|) of _inputs or None -> (problem dicts, fp64 results, fp64 S)"""
    g = torch.Generator().manual_seed(100 + seed)
    out, want, mags, w0 = [], [], [], None
    for i, (sources, F, res, integer) in enumerate(problems):
        srcs, y64, S, budget = [], 0, 0, 0
        for j, (N, C, H, W, dg, stride, bias) in enumerate(sources):
            x, off, w, b = _inputs(seed + 10 * i + j, N, C, H, W, F, dg, stride, 1, 1, bias, off1, integer=integer)
            w = w0 = w0 if share_w and w0 is not None else w
            y64 = y64 + dcn_forward(x, off, w, 1, stride, 1, dg, b)
            col = dcn_col(x, off, (3, 3), 1, stride, 1, dg)
            S = S + torch.einsum("fck,nckhw->nfhw", w.double().abs().reshape(F, C, 9), col.abs())
            if bias:
                S = S + b.double().abs().reshape(1, F, 1, 1)
            budget += 9 * C * float(x.abs().max()) * float(w.abs().max()) + (8 if bias else 0)
            srcs.append((x, off, w, b, 1, stride, 1, dg))
        Ho, Wo = y64.shape[2:]
        if res:
            shape = (sources[0][0], F, res[0], res[1])
            r = _half(torch.randint(-8, 9, shape, generator=g).float() if integer else torch.randn(shape, generator=g), off1)
            y64, S, budget = y64 + _up64(r, res[2], Ho, Wo), S + _up64(r, res[2], Ho, Wo).abs(), budget + 8
        if integer:   # every sample a multiple of 1/4, every partial sum exact in fp32 in any order
            assert budget <= 2048 and bool((y64 * 4 == (y64 * 4).round()).all()) and float(y64.abs().max()) <= 2048
        out.append(dict(sources=srcs, residual=(r, res[2]) if res else None))
        want.append(y64)
        mags.append(S)
    return out, want, mags


def _tensors(problems):
    return [t for p in problems for s in p["sources"] for t in s[:4] if t is not None] + \
        [p["residual"][0] for p in problems if p["residual"]]


SINGLE = ([(1, 16, 7, 13, 1, 1, False)], 8, None, (3, 3))
DUAL = ([(1, 16, 7, 11, 1, 1, True), (1, 16, 13, 21, 1, 2, True)], 8, (4, 6, 1), (2, 3))   # odd crop, less than a tile
EXACT = {
    "single": dict(problems=[SINGLE]),
    "dual_residual": dict(problems=[DUAL]),
    # N = 2, ragged last tile, partial filter block, two slabs beside one, two groups beside one; every pointer 2 bytes off
    "unequal_C_dg": dict(problems=[([(2, 32, 11, 19, 2, 1, True), (2, 16, 22, 38, 1, 2, True)], 72, (11, 19, 0), (1, 3))],
                         off1=True),
    # the no-LDS map, a second filter tile, a dual-source problem of 45 pixels: mixed branches in one launch
    "three_problems": dict(problems=[([(1, 16, 4, 2100, 1, 1, True)], 8, None, (3, 3)),
                                     ([(1, 16, 7, 13, 1, 1, True)], 264, None, (3, 3)),
                                     ([(1, 16, 5, 9, 1, 1, False), (1, 16, 9, 17, 1, 2, True)], 8, (3, 5, 1), (2, 3))]),
    "sixteen_share_a_weight": dict(problems=[SINGLE] * 16, share_w=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(EXACT))
def test_exact_cases_bit_for_bit(name):
    from simpledet_amd import deform_conv_f16 as d16
    probs, want, _ = _build(**EXACT[name])
    outs = [_half(torch.zeros(w.shape), EXACT[name].get("off1", False)) for w in want]
    ys = d16.deform_conv_pyramid_forward(probs, out=outs)
    for p, y, w in zip(probs, ys, want):
        w = w.half()
        assert y.dtype == torch.float16 and torch.equal(y.view(torch.int16), w.view(torch.int16)), \
            "%d elements differ, worst %g" % (int((y != w).sum()), float((y.double() - w.double()).abs().max()))
        if len(p["sources"]) == 1 and p["residual"] is None:
            x, off, wt, b, pad, stride, dil, dg = p["sources"][0]
            one = d16.deform_conv_forward(x, off, wt, pad, stride, dil, dg, bias=b)
            assert torch.equal(y.view(torch.int16), one.view(torch.int16))


@pytest.mark.gpu
@pytest.mark.parametrize("problem", [
    ([(2, 32, 11, 19, 2, 1, True), (2, 32, 22, 38, 2, 2, True)], 72, (6, 10, 1), None),
    ([(1, 256, 7, 13, 1, 1, False), (1, 256, 13, 25, 1, 2, False)], 256, None, None)], ids=["C32_residual", "K4608"])
def test_random_case_within_the_derived_bound(problem):
    """|y - y64| <= (1 + 2^-10) [(2^-11 + (K + 16) 2^-24) S + 2^-11 |y64| + 2^-25], K = sum_s 9 C_s + 3,
    S = sum |w col| + sum |bias_s| + |r| (include/simpledet_ops.h has the derivation).  Measured on an MI355X: 0.259
    and 0.078."""
    from simpledet_amd import deform_conv_f16 as d16
    probs, (y64,), (S,) = _build([problem], seed=3)
    y, = d16.deform_conv_pyramid_forward(probs)
    K = sum(9 * s[1] for s in problem[0]) + 3
    bound = (1 + 2.0 ** -10) * ((2.0 ** -11 + (K + 16) * 2.0 ** -24) * S + 2.0 ** -11 * y64.abs() + 2.0 ** -25)
    ratio = float(((y.double() - y64).abs() / bound).max())
    print("worst err / bound %.3f" % ratio)
    assert ratio <= 1, "worst err / bound %.3f" % ratio


@pytest.mark.gpu
@pytest.mark.parametrize("bad,code", [("17_problems", -2), ("three_sources", -2), ("output_sizes", -1), ("kernel_1x1", -2)])
def test_refused_lists_return_the_code_and_touch_no_output(bad, code):
    from simpledet_amd import _lib, deform_conv_f16 as d16
    probs, want, _ = _build([SINGLE, DUAL])
    x, off, w, b = probs[0]["sources"][0][:4]
    if bad == "17_problems":
        probs, want = [probs[0]] * 17, [want[0]] * 17
    elif bad == "three_sources":
        probs[1]["sources"] = probs[1]["sources"] + probs[1]["sources"][:1]
    elif bad == "output_sizes":   # the same map at stride 1 and at stride 2
        off2 = _half(torch.zeros(1, 18, 4, 7), False)
        probs[0]["sources"] = [(x, off, w, b, 1, 1, 1, 1), (x, off2, w, b, 1, 2, 1, 1)]
    else:
        w1, off1 = _half(torch.ones(8, 16, 1, 1), False), _half(torch.zeros(1, 2, 7, 13), False)
        probs[0]["sources"] = [(x, off1, w1, b, 0, 1, 1, 1)]
    outs = [torch.full(v.shape, 77.0, device="cuda", dtype=torch.float16) for v in want]
    with pytest.raises(_lib.SimpleDetOpsError) as e:
        d16.pyramid_call([d16._problem(p) for p in probs], outs)
    torch.cuda.synchronize()
    assert e.value.code == code and all(bool((o == 77).all()) for o in outs)
    if bad == "17_problems":   # the public function serves an unsupported list by single calls
        assert all(torch.equal(y, v.half()) for y, v in zip(d16.deform_conv_pyramid_forward(probs), want))


@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_on_changed_inputs_give_equal_bits():
    from simpledet_amd import deform_conv_f16 as d16
    (probs, (want,), _), (probs2, (want2,), _) = _build([DUAL]), _build([DUAL], seed=1)
    want, want2 = want.half(), want2.half()
    assert not torch.equal(want, want2)
    for _ in range(2):
        assert torch.equal(d16.deform_conv_pyramid_forward(probs)[0], want)
    static, _, _ = _build([DUAL])
    out = [torch.zeros_like(want)]
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d16.deform_conv_pyramid_forward(static, out=out)   # (workspace in the pool before capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            d16.deform_conv_pyramid_forward(static, out=out)
    for new, expect in ((probs2, want2), (probs, want), (probs2, want2)):
        for s, t in zip(_tensors(static), _tensors(new)):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], expect)


@pytest.mark.gpu
def test_autograd_gives_the_single_call_gradients_and_the_residual_window_sums():
    """12 x 20 outputs (Ho Wo % 4 == 0: the float32 backward sums dX in fixed point, so two calls give equal bits);
    a residual of 7 rows, whose last row the crop leaves unread"""
    from simpledet_amd import _lib, deform_conv_f16 as d16
    problem = ([(2, 32, 12, 20, 2, 1, True), (2, 32, 24, 40, 2, 2, True)], 24, (7, 10, 1), None)
    (prob,), _, _ = _build([problem], seed=5)
    srcs = [tuple((t.float() / 4).half() if k == 1 else t for k, t in enumerate(s)) for s in prob["sources"]]   # offsets ~ N(0, 0.5^2)
    prob = dict(sources=srcs, residual=prob["residual"])
    for t in _tensors([prob]):
        t.requires_grad_()
    dy = _half(torch.randn((2, 24, 12, 20), generator=torch.Generator().manual_seed(6)), False)
    with _lib.lib().tuned(deform_gemm_ksplit=0):
        y, = d16.deform_conv_pyramid([prob])
        y.backward(dy)
        for x, off, w, b, pad, stride, dil, dg in srcs:
            want = d16.deform_conv_backward(dy, x.detach(), off.detach(), w.detach(), pad, stride, dil, dg, bias=True)
            for name, t, wv in zip(("d_data", "d_offset", "d_weight", "d_bias"), (x, off, w, b), want):
                assert torch.equal(t.grad.view(torch.int16), wv.view(torch.int16)), name
    d64 = torch.zeros(2, 24, 14, 20, dtype=torch.float64, device="cuda")
    d64[:, :, :12] = dy.double()
    d64 = d64.view(2, 24, 7, 2, 10, 2).sum((3, 5))
    r = prob["residual"][0]
    assert torch.equal(r.grad.view(torch.int16), d64.half().view(torch.int16)) and bool((r.grad[:, :, 6] == 0).all())
