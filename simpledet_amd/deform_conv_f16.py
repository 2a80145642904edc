"""DeformableConvolution on float16 tensors (the reference's fp16 graphs: the `config/sepc` RetinaNet configs build
`models/sepc/sepc_dconv.py:12-16` on half pyramid levels, the fp16 TridentNet configs the dilated deformable blocks
of `models/tridentnet/resnet_v*.py:85-90`).

    deform_conv_forward / deform_conv_backward   the `ops` functions of the same names for float16 tensors (float32
                                                 tensors go to `ops` unchanged)
    deform_conv                                  an autograd function over both
    deform_conv_pyramid_forward / deform_conv_pyramid
                                                 a list of independent forward problems in one launch, each with up
                                                 to two sources summed in the accumulator and an optional upsampled
                                                 residual (csrc/deform_pyramid_f16.hip); opt-in, the
                                                 adapter does not use it
    install(mx)                                  after mxnet_plugin.install(mx): `mx.sym.contrib.DeformableConvolution`
                                                 builds a prop whose infer_type passes float16 through and whose
                                                 operator picks the entry points by the dtype of its data

Forward, 3x3 kernels with num_group = 1 and C / num_deformable_group % 16 == 0: the col-free kernel of
csrc/deform_fused_f16.hip -- fp32 sampling rounded once to fp16, fp16 weights untouched, single-term
fp16 matrix-core products into fp32, one final rounding.  Every other shape, and the backward: the float32 operator
on widened operands, each result rounded once (bit-equal to cast -> float32 call -> cast).
Backward with fused_weight_grad=True (opt-in, same shapes as the native forward): d_weight from the col-free kernel of
csrc/deform_wgrad_f16.hip -- the forward's samples, dY as it lies, single-term fp16 matrix-core products
summed in fp32 over all images and pixels in a fixed order, one rounding; the other gradients keep their bits.
Backward with fused_input_grads=True (opt-in, same shapes): d_data and d_offset from csrc/deform_igrad_f16.hip
 -- dcol = W^T dY on single-term fp16 matrix-core products, d_offset from the fp32 accumulators in the
tile, d_data from an fp16 dcol written and read once; d_weight and d_bias keep their bits.

It stays out of `ops.py` and of mxnet_plugin's tables, like sync_bn.py and free_anchor.py: their public surfaces are
pinned."""
import collections
import ctypes

import torch

from . import ops
from ._lib import SD_ERR_UNSUPPORTED, SimpleDetOpsError
from ._mx_adapter import REQ, _call, _mx, _no_add, _ptr, _req, _sync, _wait, _ws, alias_ctor, drop_alias, put_alias, \
    register_ops
from .ops import _chk, _dcn_out_hw, _req_of

F16_OP = "_contrib_DeformableConvolution_f16"
_own = {"installed": False, "props": {}, "fused_weight_grad": False, "fused_input_grads": False}
fallbacks = []


def _geom(x, offset, weight, pad, stride, dilate, num_deformable_group, num_group, bias=None):
    for t, name in ((x, "data"), (offset, "offset"), (weight, "weight")):
        _chk(t, name, torch.float16, ndim=4)
    N, C, H, W = x.shape
    F, Cw, kh, kw = weight.shape
    num_group, dg = int(num_group), int(num_deformable_group)
    if num_group < 1 or C % num_group or F % num_group:
        raise ValueError("num_group %d must divide data channels %d and num_filter %d" % (num_group, C, F))
    if Cw * num_group != C:
        raise ValueError("weight channels %d != data channels %d / num_group %d" % (Cw, C, num_group))
    if bias is not None:
        _chk(bias, "bias", torch.float16, shape=(F,))
    Ho, Wo = _dcn_out_hw(H, W, kh, kw, pad, stride, dilate)
    if tuple(offset.shape) != (N, dg * 2 * kh * kw, Ho, Wo):
        raise ValueError("offset shape %s != %s" % (tuple(offset.shape), (N, dg * 2 * kh * kw, Ho, Wo)))
    return (N, C, H, W, F, kh, kw, int(pad), int(stride), int(dilate), dg, num_group), (Ho, Wo)


def deform_conv_forward(x, offset, weight, pad=1, stride=1, dilate=1, num_deformable_group=1, keep_col=False,
                        bias=None, num_group=1, out=None):
    """ops.deform_conv_forward for float16 tensors: y (N,F,Ho,Wo) float16.  There is no col matrix to keep:
    keep_col=True is refused for float16.  float32 tensors are handed to ops.deform_conv_forward (which takes no
    out=: refused there)."""
    if x.dtype == torch.float32:
        if out is not None:
            raise ValueError("out= is for float16 tensors; ops.deform_conv_forward allocates its float32 result")
        return ops.deform_conv_forward(x, offset, weight, pad, stride, dilate, num_deformable_group, keep_col, bias,
                                       num_group)
    if keep_col:
        raise ValueError("the float16 forward has no col matrix to keep")
    dims, (Ho, Wo) = _geom(x, offset, weight, pad, stride, dilate, num_deformable_group, num_group, bias)
    y = ops._out(out, "out", (dims[0], dims[4], Ho, Wo), x.device, torch.float16)
    ws = ops._ws(x.device, None, "sd_deform_convolution_fwd_workspace_bytes_f16", *dims)
    ops._call("sd_deform_convolution_fwd_f16", x, offset, weight, bias, y, *dims, ws, ws.numel())
    return y


def deform_conv_backward(out_grad, x, offset, weight, pad=1, stride=1, dilate=1, num_deformable_group=1,
                         req=("write", "write", "write"), grads=None, fwd_ws=None, num_group=1, bias=False,
                         fused_weight_grad=False, pixel_runs=0, fused_input_grads=False):
    """ops.deform_conv_backward for float16 tensors -> (d_data, d_offset, d_weight[, d_bias]), float16: the float32
    backward on widened operands, every gradient rounded once (req "add": onto the widened destination).
    fused_weight_grad=True: sd_deform_convolution_bwd_f16_fused -- d_weight from the col-free half kernel where the
    shape allows, in `pixel_runs` pixel runs per image (0: chosen for the device); the other gradients unchanged.
    fused_input_grads=True: sd_deform_convolution_bwd_f16_native -- d_data and d_offset from the half kernels where
    the shape allows (bounds: include/simpledet_ops.h); d_weight as fused_weight_grad says, d_bias unchanged."""
    if x.dtype == torch.float32:
        return ops.deform_conv_backward(out_grad, x, offset, weight, pad, stride, dilate, num_deformable_group, req,
                                        grads, fwd_ws, num_group, bias)
    dims, (Ho, Wo) = _geom(x, offset, weight, pad, stride, dilate, num_deformable_group, num_group)
    _chk(out_grad, "out_grad", torch.float16, shape=(dims[0], dims[4], Ho, Wo))
    r = [_req_of(v) for v in req]
    if bias and len(r) == 3:
        r.append(REQ["write"])
    if grads is None:
        grads = (torch.empty_like(x), torch.empty_like(offset), torch.empty_like(weight))
        if bias:
            grads = grads + (torch.empty(dims[4], device=x.device, dtype=torch.float16),)
    elif len(grads) != (4 if bias else 3):
        raise ValueError("grads must hold %d tensors, got %d" % (4 if bias else 3, len(grads)))
    for t, like in zip(grads, (x, offset, weight)):
        _chk(t, "gradient", torch.float16, shape=like.shape)
    tail, extra = _route(fused_weight_grad, fused_input_grads, pixel_runs)
    ws = ops._ws(x.device, None, "sd_deform_convolution_bwd_workspace_bytes_f16" + tail, *dims, *extra)
    ops._call("sd_deform_convolution_bwd_f16" + tail, out_grad, x, offset, weight, grads[0], grads[1], grads[2],
              grads[3] if bias else None, r[0], r[1], r[2], r[3] if bias else REQ["null"], *dims, *extra, ws,
              ws.numel())
    return grads


def _route(fused_weight_grad, fused_input_grads, pixel_runs):
    """the backward entry point's suffix and the arguments it takes in front of the workspace"""
    if fused_input_grads:
        return "_native", (int(bool(fused_weight_grad)), int(pixel_runs))
    return ("_fused", (int(pixel_runs),)) if fused_weight_grad else ("", ())


class _DeformConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offset, weight, bias, pad, stride, dilate, dg, num_group, fused_weight_grad,
                fused_input_grads=False):
        ctx.save_for_backward(x, offset, weight)
        ctx.geom, ctx.has_bias = (pad, stride, dilate, dg), bias is not None
        ctx.num_group, ctx.fused, ctx.fused_in = num_group, fused_weight_grad, fused_input_grads
        return deform_conv_forward(x, offset, weight, pad, stride, dilate, dg, False, bias, num_group)

    @staticmethod
    def backward(ctx, dy):
        x, offset, weight = ctx.saved_tensors
        kw = dict(fused_weight_grad=ctx.fused, fused_input_grads=ctx.fused_in) if x.dtype == torch.float16 else {}
        g = deform_conv_backward(dy.contiguous(), x, offset, weight, *ctx.geom, num_group=ctx.num_group,
                                 bias=ctx.has_bias, **kw)
        return g[0], g[1], g[2], (g[3] if ctx.has_bias else None), None, None, None, None, None, None, None


def deform_conv(x, offset, weight, bias=None, pad=1, stride=1, dilate=1, num_deformable_group=1, num_group=1,
                fused_weight_grad=False, fused_input_grads=False):
    """differentiable DeformableConvolution on float16 or float32 tensors; fused_weight_grad: the half backward's
    d_weight from the col-free kernel, fused_input_grads: its d_data and d_offset from the half kernels
    (deform_conv_backward)"""
    return _DeformConv.apply(x, offset, weight, bias, pad, stride, dilate, num_deformable_group, num_group,
                             bool(fused_weight_grad), bool(fused_input_grads))


# ------------------------------------------------------------------- a pyramid of problems, one launch ----
class _PyrSource(ctypes.Structure):
    """struct sd_dcn_pyramid_source of include/simpledet_ops.h"""
    _fields_ = [(k, ctypes.c_void_p) for k in ("x", "offset", "weight", "bias")] + \
               [(k, ctypes.c_int) for k in ("C", "H", "W", "kh", "kw", "pad", "stride", "dil", "dgroup", "num_group")]


class _PyrProblem(ctypes.Structure):
    """struct sd_dcn_pyramid_problem"""
    _fields_ = [("y", ctypes.c_void_p), ("residual", ctypes.c_void_p)] + \
               [(k, ctypes.c_int) for k in ("N", "F", "Ho", "Wo", "Hr", "Wr", "shift", "num_sources")] + \
               [("sources", _PyrSource * 2)]


PyramidProblem = collections.namedtuple("PyramidProblem", "sources residual", defaults=(None,))


def _problem(p):
    """a problem as (sources, residual): sources a list of (x, offset, weight, bias, pad, stride, dilate,
    num_deformable_group), residual None or (tensor, shift)"""
    p = PyramidProblem(**p) if isinstance(p, dict) else PyramidProblem(*p)
    if not p.sources:
        raise ValueError("a pyramid problem needs at least one source")
    return PyramidProblem([tuple(s) for s in p.sources], None if p.residual is None else tuple(p.residual))


def _pyramid_shape(p):
    """(N, F, Ho, Wo) of a problem, from its first source; every tensor of the problem checked against it"""
    dims = None
    for x, offset, weight, bias, pad, stride, dilate, dg in p.sources:
        d, (Ho, Wo) = _geom(x, offset, weight, pad, stride, dilate, dg, 1, bias)
        dims = dims or (d[0], d[4], Ho, Wo)   # (a source of another output size: the C call refuses it)
        if (d[0], d[4]) != dims[:2]:
            raise ValueError("sources of one problem must share N and num_filter")
    if p.residual is not None:
        r, shift = p.residual
        _chk(r, "residual", torch.float16, ndim=4)
        if tuple(r.shape[:2]) != dims[:2]:
            raise ValueError("residual %s does not match the output's (N, F) = %s" % (tuple(r.shape), dims[:2]))
    return dims


def pyramid_call(problems, outs):
    """sd_deform_convolution_pyramid_fwd_f16 on a list of _problem()s and their outputs, as it is: a list the entry
    point refuses raises SimpleDetOpsError with the C code, before anything is launched"""
    table = (_PyrProblem * len(problems))()
    for q, p, y in zip(table, problems, outs):
        N, F, Ho, Wo = _pyramid_shape(p)
        _chk(y, "out", torch.float16, shape=(N, F, Ho, Wo))
        q.y, q.N, q.F, q.Ho, q.Wo, q.num_sources = y.data_ptr(), N, F, Ho, Wo, len(p.sources)
        if p.residual is not None:
            r, shift = p.residual
            q.residual, q.Hr, q.Wr, q.shift = r.data_ptr(), r.shape[2], r.shape[3], int(shift)
        for s, (x, offset, weight, bias, pad, stride, dilate, dg) in zip(q.sources, p.sources):   # (the first two)
            s.x, s.offset, s.weight = x.data_ptr(), offset.data_ptr(), weight.data_ptr()
            s.bias = None if bias is None else bias.data_ptr()
            (_, s.C, s.H, s.W), (s.kh, s.kw) = x.shape, weight.shape[2:]
            s.pad, s.stride, s.dil, s.dgroup, s.num_group = int(pad), int(stride), int(dilate), int(dg), 1
    ws = ops._ws(outs[0].device, None, "sd_deform_convolution_pyramid_fwd_workspace_bytes_f16", table, len(table))
    ops._call("sd_deform_convolution_pyramid_fwd_f16", table, len(table), ws, ws.numel())


def _upsampled(r, shift, Ho, Wo):
    """the residual as the epilogue reads it: element (h >> shift, w >> shift), cropped from the origin"""
    if shift:
        r = r.repeat_interleave(2, 2).repeat_interleave(2, 3)
    return r[:, :, :Ho, :Wo]


def deform_conv_pyramid_forward(problems, out=None):
    """A list of independent float16 DeformableConvolution problems in one launch (csrc/deform_pyramid_f16.hip, DESIGN
    4.30).  A problem is a dict or PyramidProblem: sources=[(x, offset, weight, bias, pad, stride, dilate,
    num_deformable_group), ...] (one or two, 3x3, summed in the fp32 accumulator), residual=None | (tensor, shift)
    (read at (h >> shift, w >> shift): shift 1 is UpSampling(2, nearest) -> slice_like).  Returns the list of outputs
    (out: a list of tensors to write), each rounded ONCE; a single-source problem without a residual has
    deform_conv_forward's bits.  No output may be an input of the same call.
    A list the entry point refuses as unsupported (more than 16 problems or 2 sources, a shape outside the native
    kernel) runs as single deform_conv_forward calls plus float16 torch adds instead, which round per node."""
    probs = [_problem(p) for p in problems]
    if not probs:
        return []
    dims = [_pyramid_shape(p) for p in probs]
    dev = probs[0].sources[0][0].device
    if out is None:
        out = [torch.empty(d, device=dev, dtype=torch.float16) for d in dims]
    elif len(out) != len(probs):
        raise ValueError("out must hold %d tensors, got %d" % (len(probs), len(out)))
    try:
        pyramid_call(probs, out)
    except SimpleDetOpsError as e:
        if e.code != SD_ERR_UNSUPPORTED:
            raise
        for p, y, (_, _, Ho, Wo) in zip(probs, out, dims):
            acc = None
            for x, offset, weight, bias, pad, stride, dilate, dg in p.sources:
                t = deform_conv_forward(x, offset, weight, pad, stride, dilate, dg, bias=bias)
                acc = t if acc is None else acc + t
            if p.residual is not None:
                acc = acc + _upsampled(p.residual[0], p.residual[1], Ho, Wo)
            y.copy_(acc)
    return list(out)


def _d_residual(dy, shape, shift):
    """the residual's gradient: the fp32 sum of the (<= 4) dy elements that read each element, rounded once; zero
    where the crop left nothing"""
    (Hr, Wr), (Ho, Wo) = shape[2:], dy.shape[2:]
    d = torch.zeros(shape[:2] + (Hr << shift, Wr << shift), device=dy.device, dtype=torch.float32)
    d[:, :, :Ho, :Wo] = dy
    if shift:
        d = d.view(shape[0], shape[1], Hr, 2, Wr, 2).sum((3, 5))
    return d.half()


class _DeformConvPyramid(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, route, *flat):
        ctx.spec, ctx.route = spec, route
        ctx.save_for_backward(*flat)
        ys = deform_conv_pyramid_forward(_unflatten(spec, flat))
        return tuple(ys)

    @staticmethod
    def backward(ctx, *dys):
        flat, grads, at = ctx.saved_tensors, [], 0
        for (sources, shift), dy in zip(ctx.spec, dys):
            dy = dy.contiguous()
            for pad, stride, dilate, dg, has_bias in sources:
                x, offset, weight = flat[at:at + 3]
                at += 4 if has_bias else 3
                grads += deform_conv_backward(dy, x, offset, weight, pad, stride, dilate, dg, bias=has_bias, **ctx.route)
            if shift is not None:
                grads.append(_d_residual(dy, tuple(flat[at].shape), shift))
                at += 1
        return (None, None) + tuple(grads)


def _unflatten(spec, flat):
    probs, at = [], 0
    for sources, shift in spec:
        srcs = []
        for pad, stride, dilate, dg, has_bias in sources:
            x, offset, weight = flat[at:at + 3]
            srcs.append((x, offset, weight, flat[at + 3] if has_bias else None, pad, stride, dilate, dg))
            at += 4 if has_bias else 3
        probs.append(PyramidProblem(srcs, None if shift is None else (flat[at], shift)))
        at += shift is not None
    return probs


def deform_conv_pyramid(problems, fused_weight_grad=False, fused_input_grads=False):
    """differentiable deform_conv_pyramid_forward -> tuple of outputs.  The backward adds no kernel: per source it is
    deform_conv_backward(dy, ...) on the problem's dy (fused_weight_grad / fused_input_grads choose its route), so its
    bits are the single call's; the residual's gradient is _d_residual."""
    spec, flat = [], []
    for p in (_problem(p) for p in problems):
        sources = []
        for x, offset, weight, bias, pad, stride, dilate, dg in p.sources:
            flat += [x, offset, weight] + ([] if bias is None else [bias])
            sources.append((pad, stride, dilate, dg, bias is not None))
        if p.residual is not None:
            flat.append(p.residual[0])
        spec.append((sources, None if p.residual is None else int(p.residual[1])))
    route = dict(fused_weight_grad=bool(fused_weight_grad), fused_input_grads=bool(fused_input_grads))
    return _DeformConvPyramid.apply(spec, route, *flat)


# ----------------------------------------------------------------------------------- MXNet adapter ----
def _is_half(nd):
    """an NDArray's dtype is a numpy type; the test stub's arrays wrap torch tensors"""
    d = getattr(nd, "dtype", None)
    return "float16" in str(d if d is not None else nd.t.dtype)


def _build_ops(mx):
    from .mxnet_plugin import _deform_conv_ops
    base = _deform_conv_ops(mx)["_contrib_DeformableConvolution"][0]

    class DeformConvF16(base.OP):
        """half data: the `_f16` entry points; float data: the adapter's operator as it is (cache_col included)"""

        def _dims(self, x):
            g = self.g
            return tuple(x.shape) + (g["F"], g["kh"], g["kw"], g["pad"], g["stride"], g["dil"], g["dg"], g["G"])

        def forward(self, is_train, req, in_data, out_data, aux):
            if not _is_half(in_data[0]):
                return super().forward(is_train, req, in_data, out_data, aux)
            _no_add(req)
            _wait(*in_data)
            x, off, w = in_data[:3]
            b = in_data[3] if self.g["bias"] else None
            dims = self._dims(x)
            ws, wsp, wsn = _ws(x, "sd_deform_convolution_fwd_workspace_bytes_f16", *dims)
            _call("sd_deform_convolution_fwd_f16", _ptr(x), _ptr(off), _ptr(w), _ptr(b), _ptr(out_data[0]), *dims,
                  wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            if not _is_half(in_data[0]):
                return super().backward(req, out_grad, in_data, out_data, in_grad, aux)
            _wait(out_grad[0], *in_data)
            x, off, w = in_data[:3]
            has_b = self.g["bias"]
            dims = self._dims(x)
            tail, extra = _route(_own["fused_weight_grad"], _own["fused_input_grads"], 0)   # (pixel_runs: the host's)
            ws, wsp, wsn = _ws(x, "sd_deform_convolution_bwd_workspace_bytes_f16" + tail, *dims, *extra)
            _call("sd_deform_convolution_bwd_f16" + tail, _ptr(out_grad[0]), _ptr(x), _ptr(off), _ptr(w),
                  _ptr(in_grad[0]), _ptr(in_grad[1]), _ptr(in_grad[2]), _ptr(in_grad[3]) if has_b else None,
                  _req(req[0]), _req(req[1]), _req(req[2]), _req(req[3]) if has_b else REQ["null"], *dims, *extra,
                  wsp, wsn, None)
            _sync()

    class DeformConvF16Prop(base):
        OP = DeformConvF16

        def infer_type(self, in_type):
            """every input and the output take the data's type: float16 passes through, as float32 does"""
            n = len(self.list_arguments())
            return [in_type[0]] * n, [in_type[0]], []

    return {F16_OP: DeformConvF16Prop}


def register(mx=None):
    """Register `sd__contrib_DeformableConvolution_f16`.  Returns {name: PropClass}."""
    mx = _mx(mx)
    return register_ops(mx, _build_ops(mx), _own)


def install(mx=None, fused_weight_grad=False, fused_input_grads=False):
    """After mxnet_plugin.install(mx): register() + point the `DeformableConvolution` alias of every contrib
    namespace at the dtype-dispatching operator.  The constructor the plugin's alias replaced stays the fallback for
    parameter sets `sd_supports` (unchanged) does not take; stream and sync are the plugin's.
    fused_weight_grad=True: the half operator's backward calls sd_deform_convolution_bwd_f16_fused;
    fused_input_grads=True: sd_deform_convolution_bwd_f16_native (with fused_weight_grad as its argument)."""
    mx = _mx(mx)
    props = register(mx)
    _own["fused_weight_grad"], _own["fused_input_grads"] = bool(fused_weight_grad), bool(fused_input_grads)
    del fallbacks[:]
    put_alias(mx, "contrib", "DeformableConvolution",
              lambda original: alias_ctor(mx, F16_OP, props[F16_OP], original,
                                          lambda *fallback: fallbacks.append(fallback),
                                          label="DeformableConvolution", native_drop=("cache_col",)))
    _own["installed"] = True
    return props


def uninstall(mx=None):
    """Put back the constructor `DeformableConvolution` had before any alias (mxnet_plugin.install(mx) re-creates
    the plugin's own)."""
    drop_alias(_mx(mx), "contrib", "DeformableConvolution")
    _own["installed"] = False
