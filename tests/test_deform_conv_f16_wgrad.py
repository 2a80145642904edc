"""The fp16 DeformableConvolution weight gradient without a col matrix (csrc/deform_wgrad_f16.hip, DESIGN 4.28;
deform_conv_f16.deform_conv_backward(fused_weight_grad=True)) against dW64 = einsum(dy, col64) in fp64 on the widened
inputs (tests/dcn_torch_ref.py), and the other gradients against the default backward's bits."""
import pytest
import torch

from . import mx_stub
from .dcn_torch_ref import dcn_col
from .test_deform_conv_f16 import _half, _inputs

pytestmark = pytest.mark.gpu


def _dw64(dy, x, off, pad, stride, dil, dg, absolute=False):
    col = dcn_col(x, off, (3, 3), pad, stride, dil, dg)
    a, b = (dy.double().abs(), col.abs()) if absolute else (dy.double(), col)
    return torch.einsum("nfhw,nckhw->fck", a, b).reshape(dy.shape[1], x.shape[1], 3, 3)


def _dy(seed, like, off1=False, integer=True):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-3, 4, like.shape, generator=g).float() if integer else \
        torch.randn(like.shape, generator=g)
    return _half(t, off1)


# (N, C, H, W, F, dg, stride, dil, pad, every pointer 2 bytes off, req)
EXACT = [
    (1, 16, 7, 13, 8, 1, 1, 1, 1, False, "write"),     # one slab, < 16 filter rows, P = 91 odd, ragged last step
    (2, 32, 11, 19, 72, 2, 1, 1, 1, False, "add"),     # two slabs, two groups, two images into one reduction
    (1, 64, 11, 19, 8, 1, 2, 1, 1, False, "write"),    # stride 2
    (1, 32, 11, 19, 72, 2, 1, 2, 2, True, "add"),      # dilation 2; misaligned
    (2, 16, 7, 13, 8, 1, 2, 2, 0, True, "write"),      # pad 0, stride 2 + dilation 2; misaligned
    (1, 16, 4, 2100, 8, 1, 1, 1, 1, False, "add"),     # no window fits LDS; many pixel steps per run
    (1, 16, 7, 13, 264, 1, 1, 1, 1, False, "write"),   # a second filter tile with 8 live rows
]


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "x".join(str(v) for v in c[:9]))
def test_exact_cases_bit_for_bit(case):
    from simpledet_amd import deform_conv_f16 as d16
    N, C, H, W, F, dg, stride, dil, pad, off1, req = case
    x, off, _, _ = _inputs(0, N, C, H, W, F, dg, stride, dil, pad, False, off1, integer=(3, 1))
    Ho, Wo = off.shape[2:]
    dy = _dy(1, torch.empty(N, F, Ho, Wo), off1)
    # every sample a multiple of 1/4, every partial sum exact in fp32 in any order
    assert N * Ho * Wo * float(dy.abs().max()) * float(x.abs().max()) <= 2 ** 22
    into = _half(torch.randint(-8, 9, (F, C, 3, 3), generator=torch.Generator().manual_seed(2)).float() / 4, off1)
    want = _dw64(dy, x, off, pad, stride, dil, dg)
    want = ((into.double() + want) if req == "add" else want).half()
    w = _half(torch.zeros(F, C, 3, 3), off1)
    for runs in (0, 1, 3):
        dw = _half(into.clone(), off1)
        d16.deform_conv_backward(dy, x, off, w, pad, stride, dil, dg, req=("null", "null", req),
                                 grads=(torch.empty_like(x), torch.empty_like(off), dw), fused_weight_grad=True,
                                 pixel_runs=runs)
        assert torch.equal(dw.view(torch.int16), want.view(torch.int16)), "pixel_runs %d: %d elements differ, worst %g" % (
            runs, int((dw != want).sum()), float((dw.double() - want.double()).abs().max()))


@pytest.mark.parametrize("shape", [(2, 32, 11, 19, 72, 2), (1, 256, 7, 13, 256, 1)])
def test_random_case_within_the_derived_bound(shape):
    """|dW - dW64| <= (1 + 2^-10) [(2^-11 + (T + 16) 2^-24) S + 2^-11 |dW64| + 2^-25], S = sum |dy col64|, T = N Ho Wo:
    per term, the sample's own rounding to fp16 (2^-11) and its fp32 sampling arithmetic (seven operations on the four
    corner products, < 16 x 2^-24, with the offsets' fp32 coordinates), exact fp16 x fp16 products, T fp32 additions
    in any order (T 2^-24, the second-order terms inside the leading 1 + 2^-10), the final rounding of the fp32 sum
    (2^-11 |dW64|, and 2^-25 for a subnormal result).  Measured on an MI355X: 0.219 and 0.485."""
    from simpledet_amd import deform_conv_f16 as d16
    N, C, H, W, F, dg = shape
    x, off, w, _ = _inputs(3, N, C, H, W, F, dg, 1, 1, 1, False)
    dy = _dy(4, torch.empty(N, F, H, W), integer=False)
    dw = d16.deform_conv_backward(dy, x, off, w, 1, 1, 1, dg, req=("null", "null", "write"), fused_weight_grad=True)[2]
    dw64, S, T = _dw64(dy, x, off, 1, 1, 1, dg), _dw64(dy, x, off, 1, 1, 1, dg, absolute=True), N * H * W
    bound = (1 + 2.0 ** -10) * ((2.0 ** -11 + (T + 16) * 2.0 ** -24) * S + 2.0 ** -11 * dw64.abs() + 2.0 ** -25)
    ratio = float(((dw.double() - dw64).abs() / bound).max())
    print("worst err / bound %.3f" % ratio)
    assert ratio <= 1, "worst err / bound %.3f" % ratio


@pytest.mark.parametrize("kernel,G,req", [((3, 3), 1, "write"), ((3, 3), 1, "add"), ((3, 5), 1, "write"),
                                          ((3, 3), 2, "add")])
def test_the_other_gradients_keep_their_bits_and_other_shapes_fall_back(kernel, G, req):
    from simpledet_amd import _lib, deform_conv_f16 as d16
    N, C, H, W, F, dg = 2, 32, 12, 20, 24, 2
    x, off, w, _ = _inputs(5, N, C, H, W, F, dg, 1, 1, 1, False, kernel=kernel, G=G)
    off = (off.float() / 4).half()   # (ordinary data on the fixed-point dX path: deterministic)
    dy = _dy(6, torch.empty(N, F, *off.shape[2:]), integer=False)
    into = [_half(torch.randn(t.shape, generator=torch.Generator().manual_seed(7)), False)
            for t in (x, off, w, torch.empty(F))]
    with _lib.lib().tuned(deform_gemm_ksplit=0):
        got, want = [d16.deform_conv_backward(dy, x, off, w, 1, 1, 1, dg, req=(req,) * 4, num_group=G, bias=True,
                                              grads=[t.clone() for t in into], fused_weight_grad=fused)
                     for fused in (True, False)]
    fallback = kernel != (3, 3) or G != 1
    for name, g, wv in zip(("d_data", "d_offset", "d_weight", "d_bias"), got, want):
        if name != "d_weight" or fallback:
            assert torch.equal(g.view(torch.int16), wv.view(torch.int16)), name


def test_two_calls_give_equal_bits_and_the_adapter_calls_the_fused_entry_point(monkeypatch):
    from simpledet_amd import _mx_adapter, mxnet_plugin, deform_conv_f16 as d16
    x, off, w, b = _inputs(3, 2, 32, 11, 19, 72, 2, 1, 1, 1, True)
    dy = _dy(4, torch.empty(2, 72, 11, 19), integer=False)
    kw = dict(pad=1, stride=1, dilate=1, num_deformable_group=2, bias=True)
    one, two = [d16.deform_conv_backward(dy, x, off, w, fused_weight_grad=True, **kw) for _ in range(2)]
    assert torch.equal(one[2].view(torch.int16), two[2].view(torch.int16))
    mx = mx_stub.make_stub()
    mxnet_plugin.install(mx)
    prop_cls = d16.install(mx, fused_weight_grad=True)[d16.F16_OP]
    called = []
    real = _mx_adapter.lib().call
    monkeypatch.setattr(_mx_adapter.lib(), "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    try:
        op = prop_cls(kernel="(3, 3)", num_filter="72", pad="(1, 1)", num_deformable_group="2").create_operator(
            None, None, None)
        for cast, entry in ((lambda t: t, "sd_deform_convolution_bwd_f16_fused"),
                            (lambda t: t.float(), "sd_deform_convolution_bwd")):
            grads = [mx_stub.wrap(torch.empty_like(cast(t))) for t in (x, off, w, b)]
            op.backward(["write"] * 4, [mx_stub.wrap(cast(dy))], [mx_stub.wrap(cast(t)) for t in (x, off, w, b)],
                        [mx_stub.wrap(torch.empty_like(cast(dy)))], grads, [])
            assert entry in called and (cast(x).dtype == torch.float16 or not any("f16" in c for c in called))
            if cast(x).dtype == torch.float16:
                assert torch.equal(grads[2].t.view(torch.int16), one[2].view(torch.int16))
            del called[:]
    finally:
        d16.install(mx)   # (the default again for the tests after this one)
