"""The fp16 DeformableConvolution data and offset gradients on the half operands (csrc/deform_igrad_f16.hip, DESIGN 4.29;
deform_conv_f16.deform_conv_backward(fused_input_grads=True)): bit for bit against the float32 operator where every
sum is exact, within the derived bounds against fp64 autograd (tests/dcn_torch_ref.py) on random data, and the routing
of the other gradients, of other shapes and of null requests."""
import pytest
import torch

from . import mx_stub
from .dcn_torch_ref import dcn_grads
from .test_deform_conv_f16 import _half, _inputs
from .test_deform_conv_f16_wgrad import EXACT, _dy

pytestmark = pytest.mark.gpu


def _bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _exact(case):
    N, C, H, W, F, dg, stride, dil, pad, off1, req = case
    x, off, w, _ = _inputs(0, N, C, H, W, F, dg, stride, dil, pad, False, off1, integer=(3, 1))
    dy = _dy(1, torch.empty(N, F, *off.shape[2:]), off1)
    into = [_half(torch.randint(-8, 9, t.shape, generator=torch.Generator().manual_seed(2)).float() / 4, off1)
            for t in (x, off)]
    return (dy, x, off, w), (pad, stride, dil, dg), into


@pytest.mark.parametrize("case", EXACT, ids=lambda c: "x".join(str(v) for v in c[:9]))
def test_exact_cases_bit_for_bit(case):
    from simpledet_amd import ops, deform_conv_f16 as d16
    (dy, x, off, w), geom, into = _exact(case)
    F, cpg, P, req = case[4], case[1] // case[5], off.shape[2] * off.shape[3], case[10]
    # every dcol an integer <= 2048 (exact in fp16), every factor a multiple of 1/2, every partial sum exact in fp32
    m = F * float(w.abs().max()) * float(dy.abs().max())
    assert m <= 2048 and 9 * P * m <= 2 ** 22 and 2 * float(x.abs().max()) * cpg * m <= 2 ** 22
    want = ops.deform_conv_backward(dy.float(), x.float(), off.float(), w.float(), *geom)[:2]
    assert bool((want[0] * 4 == (want[0] * 4).round()).all()) and bool((want[1] * 2 == (want[1] * 2).round()).all())
    got = d16.deform_conv_backward(dy, x, off, w, *geom, req=(req, req, "null"),
                                   grads=[_half(t.clone(), case[9]) for t in into] + [torch.empty_like(w)],
                                   fused_input_grads=True)
    for name, g, wv, base in zip(("d_data", "d_offset"), got, want, into):
        wv = (base.float() + wv if req == "add" else wv).half()
        assert _bits(g, wv), "%s: %d elements differ, worst %g" % (
            name, int((g != wv).sum()), float((g.double() - wv.double()).abs().max()))


@pytest.mark.parametrize("shape", [(2, 32, 11, 19, 72, 2), (1, 256, 7, 13, 256, 1)])
def test_random_case_within_the_derived_bounds(shape):
    """The two bounds of include/simpledet_ops.h (sd_deform_convolution_bwd_f16_native) against fp64 autograd, offsets
    held off the kinks.  S_x and sum g are dcn_grads' dx on (|w|, |dy|) and on dcol = 1.  S_o is OVER-estimated as
    2 sum_c A max|x[n, c]| (|f1| + |f2| = |f3| + |f4| = 1), which only loosens the check where x is far below its
    maximum.  Measured on an MI355X (d_data, d_offset): 0.210, 0.643 and 0.216, 0.042."""
    from simpledet_amd import deform_conv_f16 as d16
    N, C, H, W, F, dg = shape
    x, off, w, _ = _inputs(3, N, C, H, W, F, dg, 1, 1, 1, False)
    o = off.float()
    off = torch.where((o - o.round()).abs() < 2.0 ** -6, o + 0.25, o).half()
    dy = _dy(4, torch.empty(N, F, H, W), integer=False)
    dx, do = d16.deform_conv_backward(dy, x, off, w, 1, 1, 1, dg, req=("write", "write", "null"),
                                      fused_input_grads=True)[:2]
    _, dx64, do64, _ = dcn_grads(x, off, w, dy, 1, 1, 1, dg)
    Sx = dcn_grads(x, off, w.abs(), dy.abs(), 1, 1, 1, dg)[1]
    sum_g = dcn_grads(x, off, torch.ones_like(w[:1]), torch.ones_like(dy[:, :1]), 1, 1, 1, dg)[1]
    A = torch.einsum("fck,nfhw->nckhw", w.double().abs().reshape(F, C, 9), dy.double().abs())
    xmax = x.double().abs().amax(dim=(2, 3)).reshape(N, C, 1, 1, 1)
    So = 2 * (A * xmax).reshape(N, dg, C // dg, 9, 1, H, W).sum(2).expand(-1, -1, -1, 2, -1, -1).reshape(do64.shape)
    T, cpg, e = 9 * H * W, C // dg, 2.0 ** -24
    bx = (1 + 2.0 ** -10) * ((2.0 ** -11 + (F + T + 16) * e) * Sx + 2.0 ** -11 * dx64.abs() + 2.0 ** -25 * (1 + sum_g))
    bo = (1 + 2.0 ** -10) * ((F + cpg + 16) * e * So + 2.0 ** -11 * do64.abs() + 2.0 ** -25)
    rx, ro = float(((dx.double() - dx64).abs() / bx).max()), float(((do.double() - do64).abs() / bo).max())
    print("worst err / bound: d_data %.3f, d_offset %.3f" % (rx, ro))
    assert rx <= 1 and ro <= 1, "worst err / bound: d_data %.3f, d_offset %.3f" % (rx, ro)


@pytest.mark.parametrize("kernel,G,req,fwg", [((3, 3), 1, "write", False), ((3, 3), 1, "add", True),
                                              ((3, 5), 1, "write", False), ((3, 3), 2, "add", True)])
def test_weight_and_bias_keep_their_bits_and_other_shapes_fall_back(kernel, G, req, fwg):
    from simpledet_amd import _lib, deform_conv_f16 as d16
    N, C, H, W, F, dg = 2, 32, 12, 20, 24, 2
    x, off, w, _ = _inputs(5, N, C, H, W, F, dg, 1, 1, 1, False, kernel=kernel, G=G)
    off = (off.float() / 4).half()   # (ordinary data on the default route's fixed-point dX path: deterministic)
    dy = _dy(6, torch.empty(N, F, *off.shape[2:]), integer=False)
    into = [_half(torch.randn(t.shape, generator=torch.Generator().manual_seed(7)), False)
            for t in (x, off, w, torch.empty(F))]
    with _lib.lib().tuned(deform_gemm_ksplit=0):
        got, want = [d16.deform_conv_backward(dy, x, off, w, 1, 1, 1, dg, req=(req,) * 4, num_group=G, bias=True,
                                              grads=[t.clone() for t in into], fused_weight_grad=fwg,
                                              fused_input_grads=native) for native in (True, False)]
    fallback = kernel != (3, 3) or G != 1
    for name, g, wv in zip(("d_data", "d_offset", "d_weight", "d_bias"), got, want):
        if name in ("d_weight", "d_bias") or fallback:
            assert _bits(g, wv), name


@pytest.mark.parametrize("null", [0, 1])
def test_a_null_request_leaves_its_destination_and_the_other_gradient_is_right(null):
    from simpledet_amd import deform_conv_f16 as d16
    ins, geom, into = _exact(EXACT[1])
    full = d16.deform_conv_backward(*ins, *geom, req=("write", "write", "null"), fused_input_grads=True)
    req = ["write", "write", "null"]
    req[null] = "null"
    got = d16.deform_conv_backward(*ins, *geom, req=req, grads=[t.clone() for t in into] + [torch.empty_like(ins[3])],
                                   fused_input_grads=True)
    assert _bits(got[null], into[null]) and _bits(got[1 - null], full[1 - null])


def test_two_calls_give_equal_offset_bits_and_the_adapter_calls_the_native_entry_point(monkeypatch):
    from simpledet_amd import _mx_adapter, mxnet_plugin, deform_conv_f16 as d16
    x, off, w, b = _inputs(3, 2, 32, 11, 19, 72, 2, 1, 1, 1, True)
    dy = _dy(4, torch.empty(2, 72, 11, 19), integer=False)
    kw = dict(pad=1, stride=1, dilate=1, num_deformable_group=2, bias=True)
    one, two = [d16.deform_conv_backward(dy, x, off, w, fused_input_grads=True, **kw) for _ in range(2)]
    assert _bits(one[1], two[1])   # (d_data: native LDS adds, no such claim)
    mx = mx_stub.make_stub()
    mxnet_plugin.install(mx)
    prop_cls = d16.install(mx, fused_input_grads=True)[d16.F16_OP]
    called = []
    real = _mx_adapter.lib().call
    monkeypatch.setattr(_mx_adapter.lib(), "call", lambda name, *a: (called.append(name), real(name, *a))[1])
    try:
        op = prop_cls(kernel="(3, 3)", num_filter="72", pad="(1, 1)", num_deformable_group="2").create_operator(
            None, None, None)
        for cast, entry in ((lambda t: t, "sd_deform_convolution_bwd_f16_native"),
                            (lambda t: t.float(), "sd_deform_convolution_bwd")):
            grads = [mx_stub.wrap(torch.empty_like(cast(t))) for t in (x, off, w, b)]
            op.backward(["write"] * 4, [mx_stub.wrap(cast(dy))], [mx_stub.wrap(cast(t)) for t in (x, off, w, b)],
                        [mx_stub.wrap(torch.empty_like(cast(dy)))], grads, [])
            assert entry in called and (cast(x).dtype == torch.float16 or not any("f16" in c for c in called))
            if cast(x).dtype == torch.float16:
                assert _bits(grads[1].t, one[1])
            del called[:]
    finally:
        d16.install(mx)   # (the default again for the tests after this one)
