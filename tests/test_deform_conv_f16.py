"""DeformableConvolution on float16 tensors (simpledet_amd/deform_conv_f16.py, csrc/deform_fused_f16.hip) against
the fp64 forward of tests/dcn_torch_ref.py on widened inputs, and against the float32 operator where the fp16 entry
points are defined as cast -> float32 call -> cast."""
import numpy as np
import pytest
import torch

from . import mx_stub
from .dcn_torch_ref import dcn_col, dcn_forward


def _half(t, off1):
    """t as a contiguous float16 CUDA tensor; off1: one element (2 bytes) behind an allocation boundary"""
    t = t.half().cuda()
    if not off1:
        return t
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=torch.float16)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def _inputs(seed, N, C, H, W, F, dg, stride, dil, pad, bias, off1=False, kernel=(3, 3), G=1, integer=None):
    """integer = (max|x|, max|w|): small integers and offsets in multiples of 0.5, some far outside the image;
    None: normal values, offsets ~ N(0, 2^2)"""
    g = torch.Generator().manual_seed(seed)
    kh, kw = kernel
    Ho = (H + 2 * pad - (dil * (kh - 1) + 1)) // stride + 1
    Wo = (W + 2 * pad - (dil * (kw - 1) + 1)) // stride + 1
    oshape = (N, dg * 2 * kh * kw, Ho, Wo)
    if integer:
        xm, wm = integer
        x = torch.randint(-xm, xm + 1, (N, C, H, W), generator=g).float()
        w = torch.randint(-wm, wm + 1, (F, C // G, kh, kw), generator=g).float()
        off = torch.randint(-2 * H, 2 * H + 1, oshape, generator=g).float() / 2 if W > 1000 else \
            torch.randint(-6, 7, oshape, generator=g).float() / 2
        off[torch.rand(oshape, generator=g) < 0.05] = 20.5
        b = torch.randint(-8, 9, (F,), generator=g).float()
    else:
        x, w = torch.randn((N, C, H, W), generator=g), torch.randn((F, C // G, kh, kw), generator=g) * 0.1
        off, b = torch.randn(oshape, generator=g) * 2, torch.randn((F,), generator=g)
    return _half(x, off1), _half(off, off1), _half(w, off1), (_half(b, off1) if bias else None)


# (N, C, H, W, F, dg, stride, dil, pad, bias, every pointer 2 bytes off, (max|x|, max|w|))
EXACT = [
    (1, 16, 7, 13, 8, 1, 1, 1, 1, False, False, (3, 3)),     # one slab, one partial filter block, less than a tile
    (2, 32, 11, 19, 72, 2, 1, 1, 1, True, False, (2, 3)),    # two slabs, two groups, F = 72, ragged last tile, N = 2
    (1, 64, 11, 19, 8, 1, 2, 1, 1, True, False, (1, 3)),     # a k walk longer than the two window buffers; stride 2
    (1, 32, 11, 19, 72, 2, 1, 2, 2, False, True, (2, 3)),    # dilation 2; misaligned
    (2, 16, 7, 13, 8, 1, 2, 2, 0, True, True, (3, 3)),       # pad 0, stride 2 + dilation 2; misaligned
    (1, 16, 4, 2100, 8, 1, 1, 1, 1, True, True, (3, 3)),     # no window fits LDS: corners from global memory
    (1, 16, 7, 13, 264, 1, 1, 1, 1, True, False, (3, 3)),    # a second tile of 256 filters, 8 rows of it live
]


def _exact_case(case, seed=0):
    N, C, H, W, F, dg, stride, dil, pad, bias, off1, rng = case
    x, off, w, b = _inputs(seed, N, C, H, W, F, dg, stride, dil, pad, bias, off1, integer=rng)
    y64 = dcn_forward(x, off, w, pad, stride, dil, dg, b)
    # every sample a multiple of 1/4, every partial sum exact in fp32 in any order
    assert 9 * C * float(x.abs().max()) * float(w.abs().max()) + (8 if bias else 0) <= 2048
    assert bool((y64 * 4 == (y64 * 4).round()).all()) and float(y64.abs().max()) <= 2048
    return (x, off, w, b), dict(pad=pad, stride=stride, dilate=dil, num_deformable_group=dg), y64.half().contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("case", EXACT, ids=lambda c: "x".join(str(v) for v in c[:9]))
def test_exact_cases_bit_for_bit(case):
    from simpledet_amd import deform_conv_f16 as d16
    (x, off, w, b), kw, want = _exact_case(case)
    out = _half(torch.zeros(want.shape), case[10])
    y = d16.deform_conv_forward(x, off, w, bias=b, out=out, **kw)
    assert y.dtype == torch.float16 and torch.equal(y.view(torch.int16), want.view(torch.int16)), \
        "%d elements differ, worst %g" % (int((y != want).sum()), float((y.double() - want.double()).abs().max()))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 32, 11, 19, 72, 2), (1, 256, 7, 13, 256, 1)])
def test_random_case_within_the_derived_bound(shape):
    """|y - y64| <= (1 + 2^-10) [(2^-11 + (K + 16) 2^-24) S + 2^-11 |y64| + 2^-25]: one rounding of each sample,
    fp32 sampling and K-term accumulation, the final rounding.  Measured on an MI355X: 0.299 and 0.154."""
    from simpledet_amd import deform_conv_f16 as d16
    N, C, H, W, F, dg = shape
    x, off, w, b = _inputs(3, N, C, H, W, F, dg, 1, 1, 1, True)
    y = d16.deform_conv_forward(x, off, w, 1, 1, 1, dg, bias=b)
    y64 = dcn_forward(x, off, w, 1, 1, 1, dg, b)
    col = dcn_col(x, off, (3, 3), 1, 1, 1, dg)
    S = torch.einsum("fck,nckhw->nfhw", w.double().abs().reshape(F, C, 9), col.abs()) + b.double().abs().reshape(1, F, 1, 1)
    K = 9 * C
    bound = (1 + 2.0 ** -10) * ((2.0 ** -11 + (K + 16) * 2.0 ** -24) * S + 2.0 ** -11 * y64.abs() + 2.0 ** -25)
    ratio = float(((y.double() - y64).abs() / bound).max())
    print("worst err / bound %.3f" % ratio)
    assert ratio <= 1, "worst err / bound %.3f" % ratio


@pytest.mark.gpu
@pytest.mark.parametrize("hw,G,bias,req", [((11, 19), 1, True, "write"), ((11, 19), 1, False, "add"),
                                           ((11, 19), 2, True, "add"), ((12, 20), 1, True, "write"),
                                           ((12, 20), 1, True, "add")])
def test_backward_is_the_float32_backward_rounded_once(hw, G, bias, req):
    from simpledet_amd import _lib, ops, deform_conv_f16 as d16
    N, C, (H, W), F, dg = 2, 32, hw, 24, 2
    if H * W % 4:
        # Ho * Wo is odd here, so the float32 backward sums dX with float atomics in hardware order (its fixed-point
        # path needs Ho * Wo % 4 == 0) and two float32 calls differ in last bits on ordinary gradients.  Small integers
        # and offsets in multiples of 0.5 make every partial sum exact, hence independent of that order, on both sides.
        x, off, w, _ = _inputs(5, N, C, H, W, F, dg, 1, 1, 1, False, G=G, integer=(2, 3))
        dy = _half(torch.randint(-3, 4, (N, F, H, W), generator=torch.Generator().manual_seed(6)).float(), False)
    else:
        # ordinary data on the fixed-point dX path: normal values and gradients, offsets ~ N(0, 0.5^2)
        x, off, w, _ = _inputs(5, N, C, H, W, F, dg, 1, 1, 1, False, G=G)
        off = (off.float() / 4).half()
        dy = _half(torch.randn((N, F, H, W), generator=torch.Generator().manual_seed(6)), False)
    into = [_half(torch.randn(t.shape, generator=torch.Generator().manual_seed(7)), False)
            for t in (x, off, w, torch.empty(F))][:4 if bias else 3]
    with _lib.lib().tuned(deform_gemm_ksplit=0):
        want = ops.deform_conv_backward(dy.float(), x.float(), off.float(), w.float(), 1, 1, 1, dg, num_group=G,
                                        bias=bias)
        got = d16.deform_conv_backward(dy, x, off, w, 1, 1, 1, dg, req=(req,) * (4 if bias else 3),
                                       grads=[t.clone() for t in into], num_group=G, bias=bias)
    for name, g, wv, base in zip(("d_data", "d_offset", "d_weight", "d_bias"), got, want, into):
        wv = (base.float() + wv if req == "add" else wv).half()
        assert torch.equal(g.view(torch.int16), wv.view(torch.int16)), name


@pytest.mark.gpu
@pytest.mark.parametrize("kernel,C,dg,G", [((1, 1), 16, 1, 1), ((3, 5), 16, 1, 1), ((3, 3), 16, 2, 1),
                                           ((3, 3), 32, 1, 2)])
def test_other_shapes_equal_the_widened_float32_call(kernel, C, dg, G):
    from simpledet_amd import ops, deform_conv_f16 as d16
    x, off, w, b = _inputs(8, 2, C, 9, 11, 12, dg, 1, 1, 1, True, kernel=kernel, G=G)
    y = d16.deform_conv_forward(x, off, w, 1, 1, 1, dg, bias=b, num_group=G)
    want = ops.deform_conv_forward(x.float(), off.float(), w.float(), 1, 1, 1, dg, bias=b.float(), num_group=G).half()
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))


@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_on_changed_inputs_give_equal_bits():
    from simpledet_amd import deform_conv_f16 as d16
    ins, kw, want = _exact_case(EXACT[1])
    ins2, _, want2 = _exact_case(EXACT[1], seed=1)
    assert not torch.equal(want, want2)
    y = [d16.deform_conv_forward(*ins[:3], bias=ins[3], **kw) for _ in range(2)]
    assert torch.equal(y[0], want) and torch.equal(y[1], want)
    static = [t.clone() for t in ins]
    out = torch.zeros_like(want)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        d16.deform_conv_forward(*static[:3], bias=static[3], out=out, **kw)   # (workspace in the pool before capture)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            d16.deform_conv_forward(*static[:3], bias=static[3], out=out, **kw)
    for new, expect in ((ins2, want2), (ins, want), (ins2, want2)):
        for s, t in zip(static, new):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, expect)


def test_install_passes_float16_through_and_keeps_the_float_prop():
    from simpledet_amd import mxnet_plugin, deform_conv_f16 as d16
    mx = mx_stub.make_stub()
    base = mxnet_plugin.install(mx)["_contrib_DeformableConvolution"]
    prop_cls = d16.install(mx)[d16.F16_OP]
    for params in ({"kernel": "(3, 3)"}, {"kernel": "(3, 3)", "stride": "(1, 2)"}, {"no_such": "1"}):
        assert prop_cls.sd_supports(params) == base.sd_supports(params)
    sym = mx.sym.contrib.DeformableConvolution(mx.sym.Variable("x"), mx.sym.Variable("o"), kernel=(3, 3),
                                               num_filter=8, pad=(1, 1), num_deformable_group=1)
    assert sym.op_type == "sd_" + d16.F16_OP
    prop = prop_cls(kernel="(3, 3)", num_filter="8", pad="(1, 1)")
    for t in (np.float16, np.float32):
        assert prop.infer_type([t, None, None, None]) == ([t] * 4, [t], [])


@pytest.mark.gpu
def test_adapter_runs_half_graphs_on_the_f16_entry_points_and_float_graphs_as_before(monkeypatch):
    from simpledet_amd import _mx_adapter, mxnet_plugin, deform_conv_f16 as d16
    mx = mx_stub.make_stub()
    base = mxnet_plugin.install(mx)["_contrib_DeformableConvolution"]
    prop_cls = d16.install(mx)[d16.F16_OP]
    (x, off, w, b), kw, want = _exact_case(EXACT[1])
    params = dict(kernel="(3, 3)", num_filter=str(w.shape[0]), pad="(1, 1)", num_deformable_group="2")
    called = []
    real = _mx_adapter.lib().call
    monkeypatch.setattr(_mx_adapter.lib(), "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    out = mx_stub.wrap(torch.empty_like(want))
    op = prop_cls(**params).create_operator(None, None, None)
    op.forward(False, ["write"], [mx_stub.wrap(t) for t in (x, off, w, b)], [out], [])
    assert "sd_deform_convolution_fwd_f16" in called and torch.equal(out.t, want)
    outs = []
    for cls in (base, prop_cls):   # a float graph: the bits the plugin's own operator gives
        o = mx_stub.wrap(torch.empty(want.shape, device="cuda"))
        cls(**params).create_operator(None, None, None).forward(
            False, ["write"], [mx_stub.wrap(t.float()) for t in (x, off, w, b)], [o], [])
        outs.append(o.t)
    assert torch.equal(outs[0], outs[1]) and called[-2] == "sd_deform_convolution_fwd"
    # the half backward through the operator: the entry point and the bits of the module's own function
    dy = _half(torch.randint(-3, 4, want.shape, generator=torch.Generator().manual_seed(2)).float(), False)
    grads = [mx_stub.wrap(torch.empty_like(t)) for t in (x, off, w, b)]
    op.backward(["write"] * 4, [mx_stub.wrap(dy)], [mx_stub.wrap(t) for t in (x, off, w, b)], [out], grads, [])
    assert "sd_deform_convolution_bwd_f16" in called
    for g, wv in zip(grads, d16.deform_conv_backward(dy, x, off, w, bias=True, **kw)):
        assert torch.equal(g.t, wv)
