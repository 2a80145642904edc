"""Torch-tensor harness over the C ABI (include/simpledet_ops.h).

PyTorch is plumbing here: it owns device memory and the HIP stream; every function passes raw
device pointers + the current stream to libsimpledet_ops_hip.so.  Nothing in this module computes
on the CPU and nothing falls back: non-CUDA tensors raise.

Function names/arguments mirror the reference operators (operator_cxx/, see each docstring).
"""
import collections
import ctypes
import math

import torch

from ._lib import SD_ERR_UNSUPPORTED, SimpleDetOpsError, lib

REQ = {"null": 0, "write": 1, "add": 3}


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# The marshalling lives in _lib: every argument is converted by the type the header gives its parameter, so the
# calls below pass tensors (or None), Python numbers, ctypes arrays and byref()s as they are.  _p and _stream
# remain for callers outside this module that wrap their arguments themselves.
def _call(name, *args):
    """lib().call, with the current torch stream appended where the entry point's last parameter is `void* stream`"""
    L = lib()
    entry = L.entry(name)
    if entry.stream:
        args += (_stream(),)
    return L.check(name, entry(args))


def _query(name, *args):
    """The value of a function that returns no status: a *_workspace_bytes / *_plan_bytes size, a stride, a count.
    Its arguments are ints, ctypes arrays and byref()s, which ctypes takes by the argument and return types _lib
    set from the header."""
    return int(getattr(lib().cdll, name)(*args))


def _ws(dev, workspace, need, *args):
    """The uint8 workspace of a call: `need` names its size query (`args` that query's arguments) or, where there
    is none, is the byte count itself.  The caller's tensor when it holds that much, a fresh one when there is
    none."""
    wsb = _query(need, *args) if isinstance(need, str) else need
    if workspace is None:
        return torch.empty(wsb, device=dev, dtype=torch.uint8)
    if workspace.numel() < wsb:
        raise ValueError("workspace needs %d bytes, got %d" % (wsb, workspace.numel()))
    return workspace


def _req_of(r):
    return REQ[r] if isinstance(r, str) else int(r)


def _fn(name, t):
    """the entry point of t's dtype: `name` for float32, its `_f16` twin otherwise"""
    return name if t.dtype == torch.float32 else name + "_f16"


def _chk(t, name, dtype=torch.float32, ndim=None, shape=None, numel=None, at_least=None):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise RuntimeError("%s must live on the GPU (simpledet_amd has no CPU path)" % name)
    if t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if ndim is not None and t.dim() != ndim:
        raise ValueError("%s should be a %dD tensor, got shape %s" % (name, ndim, tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError("%s must have shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    if numel is not None and t.numel() != numel:
        raise ValueError("%s needs %d elements, got %d" % (name, numel, t.numel()))
    if at_least is not None and t.numel() < at_least:
        raise ValueError("%s needs at least %d elements, got %d" % (name, at_least, t.numel()))
    return t


def _out(t, name, shape, dev, dtype=torch.float32, flat=False):
    """An output: a fresh tensor of `shape` when the caller gave none, else the caller's, checked -- of that shape,
    or with flat=True of any shape that holds as many elements (the entry points take flat buffers)."""
    if t is None:
        return torch.empty(shape, device=dev, dtype=dtype)
    if flat:
        return _chk(t, name, dtype, numel=math.prod(shape))
    return _chk(t, name, dtype, shape=shape)


def _pair(v):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("pooled_size must have 2 entries (h, w)")
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _iarr(vals):
    return (ctypes.c_int * len(vals))(*[int(v) for v in vals])


def _parr(tensors):
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


# --------------------------------------------------------------------------------------------------
# ROIAlign_v2  (operator_cxx/contrib/roi_align_v2{-inl.h,.cc,.cu})
# --------------------------------------------------------------------------------------------------
def roi_align_v2_forward(data, rois, pooled_size, spatial_scale):
    """_contrib_ROIAlign_v2 forward (roi_align_v2-inl.h:157-195).

    data (B,C,H,W), rois (B,R,4) -> output, maxidx_x, maxidx_y each (B,R,C,ph,pw)
    (shape inference roi_align_v2.cc:187-208).
    """
    _chk(data, "data", ndim=4)
    _chk(rois, "rois", ndim=3)
    if rois.shape[2] != 4:
        raise ValueError("bbox should be a 3D tensor of shape [batch, rois, 4]")
    if rois.shape[0] != data.shape[0]:
        raise ValueError("rois batch %d != data batch %d" % (rois.shape[0], data.shape[0]))
    ph, pw = _pair(pooled_size)
    B, C, H, W = data.shape
    R = rois.shape[1]
    shape = (B, R, C, ph, pw)
    out = torch.empty(shape, device=data.device, dtype=torch.float32)
    mx = torch.empty(shape, device=data.device, dtype=torch.float32)
    my = torch.empty(shape, device=data.device, dtype=torch.float32)
    ws = _ws(data.device, None, "sd_roi_align_v2_workspace_bytes", B, R)
    _call("sd_roi_align_v2_fwd_ws", data, rois, out, mx, my, B, C, H, W, R, ph, pw, spatial_scale, ws, ws.numel())
    return out, mx, my


def roi_align_v2_backward(out_grad, rois, maxidx_x, maxidx_y, data_shape, spatial_scale,
                          req_data="write", req_rois="write", d_data=None):
    """_backward_ROIAlign_v2 (roi_align_v2.cu:87-143): [dY, rois, maxidx_x, maxidx_y] -> [dX, d_rois]."""
    _chk(out_grad, "out_grad", ndim=5)
    _chk(rois, "rois", ndim=3)
    _chk(maxidx_x, "maxidx_x", ndim=5)
    _chk(maxidx_y, "maxidx_y", ndim=5)
    B, C, H, W = [int(v) for v in data_shape]
    Bo, R, Co, ph, pw = out_grad.shape
    if (Bo, Co) != (B, C) or rois.shape[:2] != (B, R):
        raise ValueError("shape mismatch between out_grad %s, rois %s and data %s"
                         % (tuple(out_grad.shape), tuple(rois.shape), (B, C, H, W)))
    rd, rr = _req_of(req_data), _req_of(req_rois)
    if d_data is None:
        if rd == REQ["add"]:
            raise ValueError("req_data='add' needs the d_data tensor to accumulate into")
        d_data = torch.empty((B, C, H, W), device=out_grad.device, dtype=torch.float32)
    _chk(d_data, "d_data", ndim=4)
    d_rois = torch.empty_like(rois) if rr != 0 else None
    _call("sd_roi_align_v2_bwd", out_grad, rois, maxidx_x, maxidx_y, d_data, d_rois, rd, rr, B, C, H, W, R, ph, pw,
          spatial_scale)
    return d_data, d_rois


# --------------------------------------------------------------------------------------------------
# FPN RoI extractor (models/FPN/builder.py:567-610) fused into one launch
# --------------------------------------------------------------------------------------------------
def fpn_roi_assign(rois, rcnn_stride, roi_canonical_scale=224, roi_canonical_level=4):
    """assign_layer_fpn CustomOp (models/FPN/assign_layer_fpn.py:17-41).

    rois (B,R,4) -> (list of len(rcnn_stride) zero-masked (B,R,4) tensors, level (B,R) int32)
    """
    _chk(rois, "rois", ndim=3)
    B, R, _ = rois.shape
    n = len(rcnn_stride)
    per = torch.empty((n, B, R, 4), device=rois.device, dtype=torch.float32)
    level = torch.empty((B, R), device=rois.device, dtype=torch.int32)
    _call("sd_fpn_roi_assign", rois, B * R, _iarr(rcnn_stride), n, roi_canonical_scale, roi_canonical_level, per,
          level)
    return [per[i] for i in range(n)], level


def _fpn_levels(feats, rois, rcnn_stride, dtype=torch.float32):
    """The argument check of the FPN extractors: one (B,C,H_l,W_l) map of `dtype` per stride, rois (B,R,..) of the
    same batch -> B, C, R and the H_l / W_l tables as the entry points take them."""
    _chk(rois, "rois", ndim=3)
    if len(feats) != len(rcnn_stride):
        raise ValueError("one feature map per stride expected")
    B, C = feats[0].shape[:2]
    for i, f in enumerate(feats):
        _chk(f, "feats[%d]" % i, dtype=dtype, ndim=4)
        if tuple(f.shape[:2]) != (B, C):
            raise ValueError("all levels must share (B,C)")
    if rois.shape[0] != B:
        raise ValueError("rois batch mismatch")
    return B, C, rois.shape[1], _iarr([f.shape[2] for f in feats]), _iarr([f.shape[3] for f in feats])


def fpn_roi_align_forward(feats, rois, rcnn_stride, pooled_size, roi_canonical_scale=224,
                          roi_canonical_level=4):
    """FPNRoiAlign.get_roi_feature (models/FPN/builder.py:567-610) as one op.

    feats: list of (B,C,H_l,W_l); rois (B,R,4) -> out, maxidx_x, maxidx_y (B,R,C,ph,pw).
    """
    B, C, R, Hs, Ws = _fpn_levels(feats, rois, rcnn_stride)
    ph, pw = _pair(pooled_size)
    shape = (B, R, C, ph, pw)
    out = torch.empty(shape, device=rois.device, dtype=torch.float32)
    mx = torch.empty(shape, device=rois.device, dtype=torch.float32)
    my = torch.empty(shape, device=rois.device, dtype=torch.float32)
    ws = _ws(rois.device, None, "sd_fpn_roi_align_workspace_bytes", B, R)
    _call("sd_fpn_roi_align_fwd", _parr(feats), Hs, Ws, _iarr(rcnn_stride), len(feats), rois, out, mx, my, B, C, R,
          ph, pw, roi_canonical_scale, roi_canonical_level, ws, ws.numel())
    return out, mx, my


def argmax_stride(ph, pw):
    """bytes per (RoI, channel) row of the packed arg-max (sd_fpn_roi_align_argmax_stride)."""
    return _query("sd_fpn_roi_align_argmax_stride", int(ph), int(pw))


def argmax_codes(argmax, pooled_size):
    """(B,R,C,S) packed arg-max -> (B,R,C,ph,pw) codes (drops the row padding)."""
    ph, pw = _pair(pooled_size)
    return argmax[..., :ph * pw].reshape(tuple(argmax.shape[:3]) + (ph, pw))


def _packed_forward(fn, feats, rois, rcnn_stride, pooled_size, scale, level, dtype=torch.float32, plan=False):
    """The three packed forwards behind one body: the argument check, out (of the maps' dtype) / arg-max / coords,
    the workspace and the call of entry point `fn` -> out, (argmax, coords[, plan_buf])."""
    B, C, R, Hs, Ws = _fpn_levels(feats, rois, rcnn_stride, dtype)
    ph, pw = _pair(pooled_size)
    dev = rois.device
    out = torch.empty((B, R, C, ph, pw), device=dev, dtype=dtype)
    amax = torch.empty((B, R, C, argmax_stride(ph, pw)), device=dev, dtype=torch.uint8)
    coords = torch.empty((B, R, 9 * (ph + pw)), device=dev, dtype=torch.float32)
    ws = _ws(dev, None, "sd_fpn_roi_align_workspace_bytes", B, R)
    state = (amax, coords)
    tail = ()
    if plan:
        # one rois-only pre-pass for the whole step: the backward's band lists / tap tables are built
        # here too and travel to fpn_roi_align_backward_packed as the third element of the state
        plan_buf = _ws(dev, None, "sd_fpn_roi_align_plan_bytes", Hs, Ws, len(feats), B, R)
        state, tail = state + (plan_buf,), (plan_buf, plan_buf.numel())
    _call(fn, _parr(feats), Hs, Ws, _iarr(rcnn_stride), len(feats), rois, out, amax, coords, B, C, R, ph, pw, scale,
          level, ws, ws.numel(), *tail)
    return out, state


def fpn_roi_align_forward_packed(feats, rois, rcnn_stride, pooled_size, roi_canonical_scale=224,
                                 roi_canonical_level=4, plan=False):
    """The fused extractor with a one-byte arg-max: -> out (B,R,C,ph,pw) fp32, argmax (B,R,C,S)
    uint8 (S = ph*pw rounded up to a multiple of 4; code = row sample * 3 + column sample, 255 =
    nothing pooled; unpack with argmax_codes()), coords (B,R,9*(ph+pw)) 4-byte
    words: per RoI 3*(ph+pw) fp32 sample coordinates, then 3*(ph+pw) {neighbours, fraction} pairs.  (argmax, coords) are state between this op's forward and backward
    only; fpn_roi_align_backward_packed decodes them."""
    return _packed_forward("sd_fpn_roi_align_fwd_packed_plan" if plan else "sd_fpn_roi_align_fwd_packed", feats, rois,
                           rcnn_stride, pooled_size, roi_canonical_scale, roi_canonical_level, plan=plan)


def fpn_roi_align_forward_packed_f16(feats, rois, rcnn_stride, pooled_size, roi_canonical_scale=224,
                                     roi_canonical_level=4):
    """fp16 I/O variant of fpn_roi_align_forward_packed: feats fp16 (B,C,H_l,W_l), rois fp32 (B,R,4)
    -> out fp16 (B,R,C,ph,pw), (argmax, coords).  Bit-equal to feats.float() -> the fp32 op ->
    out.half() (models/FPN/builder.py:581-586, 607-608 wraps the op in exactly those casts)."""
    try:
        return _packed_forward("sd_fpn_roi_align_fwd_packed_f16", feats, rois, rcnn_stride, pooled_size,
                               roi_canonical_scale, roi_canonical_level, dtype=torch.float16)
    except SimpleDetOpsError as e:
        if e.code != SD_ERR_UNSUPPORTED:
            raise
    # shapes the band-resident kernel does not take (too many units, W < 2, ...): the graph's own
    # cast -> fp32 op -> cast (models/FPN/builder.py:581-586, 607-608), same bits
    f32 = [cast_f16_to_f32(f) for f in feats]
    o32, state = fpn_roi_align_forward_packed(f32, rois, rcnn_stride, pooled_size, roi_canonical_scale,
                                              roi_canonical_level)
    return cast_f32_to_f16(o32), state


def fpn_roi_align_backward_packed(out_grad, rois, argmax, feat_shapes, rcnn_stride,
                                  roi_canonical_scale=224, roi_canonical_level=4, req_data="write",
                                  d_feats=None):
    _chk(out_grad, "out_grad", ndim=5)
    _chk(rois, "rois", ndim=3)
    plan_buf = argmax[2] if len(argmax) > 2 else None   # forward(plan=True): lists / tap tables are built
    argmax, coords = argmax[0], argmax[1]
    _chk(argmax, "argmax", dtype=torch.uint8, ndim=4)
    _chk(coords, "coords", ndim=3)
    B, R, C, ph, pw = out_grad.shape
    if tuple(argmax.shape) != (B, R, C, argmax_stride(ph, pw)):
        raise ValueError("argmax must be (B,R,C,%d) uint8" % argmax_stride(ph, pw))
    rd = _req_of(req_data)
    if d_feats is None:
        if rd == REQ["add"]:
            raise ValueError("req_data='add' needs d_feats")
        d_feats = [torch.empty(tuple(s), device=out_grad.device, dtype=torch.float32)
                   for s in feat_shapes]
    for i, f in enumerate(d_feats):
        _chk(f, "d_feats[%d]" % i, ndim=4)
    hs, ws_ = _iarr([f.shape[2] for f in d_feats]), _iarr([f.shape[3] for f in d_feats])
    if plan_buf is not None:
        _call("sd_fpn_roi_align_bwd_packed_plan", out_grad, rois, argmax, coords, _parr(d_feats), hs, ws_,
              _iarr(rcnn_stride), len(d_feats), rd, B, C, R, ph, pw, roi_canonical_scale, roi_canonical_level,
              plan_buf, plan_buf.numel())
        return d_feats
    # the entry point wants its workspace 4-byte aligned, 16 for the tap tables (roi_align_bwd.hip); every tensor of
    # the torch allocator is, and the query answers in multiples of 16, so the common uint8 helper serves.  An empty
    # problem (B or R zero) asks for nothing and gets NULL, which the header allows.
    work = _ws(out_grad.device, None, "sd_fpn_roi_align_bwd_workspace_bytes", hs, ws_, len(d_feats), B, R)
    _call("sd_fpn_roi_align_bwd_packed_ws", out_grad, rois, argmax, coords, _parr(d_feats), hs, ws_,
          _iarr(rcnn_stride), len(d_feats), rd, B, C, R, ph, pw, roi_canonical_scale, roi_canonical_level, work,
          work.numel())
    return d_feats


def cast_f16_to_f32(src, out=None):
    _chk(src, "src", dtype=torch.float16)
    out = torch.empty(src.shape, device=src.device, dtype=torch.float32) if out is None else out
    _call("sd_cast_f16_to_f32", src, out, src.numel())
    return out


def cast_f32_to_f16(src, out=None, req="write"):
    _chk(src, "src")
    out = torch.empty(src.shape, device=src.device, dtype=torch.float16) if out is None else out
    _call("sd_cast_f32_to_f16", src, out, src.numel(), _req_of(req))
    return out


def fpn_roi_align_backward_packed_f16(out_grad, rois, argmax, feat_shapes, rcnn_stride,
                                      roi_canonical_scale=224, roi_canonical_level=4, req_data="write",
                                      d_feats=None, native=True):
    """Backward of fpn_roi_align_forward_packed_f16: out_grad fp16 -> gradients fp16, by the backward
    kernel's fp16-I/O instance (sd_fpn_roi_align_bwd_packed_f16: fp32 tap values, fixed-point sums,
    fp16 only at the two ends).  native=False, or a shape the wide kernel does not take: the two
    op-boundary casts of the reference's fp16 graphs around the fp32 kernel (same bits)."""
    _chk(out_grad, "out_grad", dtype=torch.float16, ndim=5)
    _chk(rois, "rois", ndim=3)
    rd = _req_of(req_data)
    if d_feats is None:
        if rd == REQ["add"]:
            raise ValueError("req_data='add' needs d_feats")
        d_feats = [torch.empty(tuple(s), device=out_grad.device, dtype=torch.float16) for s in feat_shapes]
    for d in d_feats:
        _chk(d, "d_feats", dtype=torch.float16, ndim=4)
    if native:
        am, coords = argmax[0], argmax[1]
        B, R, C, ph, pw = out_grad.shape
        hs, ws_ = _iarr([f.shape[2] for f in d_feats]), _iarr([f.shape[3] for f in d_feats])
        work = _ws(out_grad.device, None, "sd_fpn_roi_align_bwd_workspace_bytes", hs, ws_, len(d_feats), B, R)
        try:
            _call("sd_fpn_roi_align_bwd_packed_f16", out_grad, rois, am, coords, _parr(d_feats), hs, ws_,
                  _iarr(rcnn_stride), len(d_feats), rd, B, C, R, ph, pw, roi_canonical_scale, roi_canonical_level,
                  work, work.numel())
            return d_feats
        except SimpleDetOpsError as e:
            if e.code != SD_ERR_UNSUPPORTED:
                raise
    g32 = fpn_roi_align_backward_packed(cast_f16_to_f32(out_grad), rois, argmax, feat_shapes, rcnn_stride,
                                        roi_canonical_scale, roi_canonical_level)
    for g, d in zip(g32, d_feats):
        cast_f32_to_f16(g, d, rd)
    return d_feats


def fpn_roi_align_backward(out_grad, rois, maxidx_x, maxidx_y, feat_shapes, rcnn_stride,
                           roi_canonical_scale=224, roi_canonical_level=4, req_data="write",
                           d_feats=None):
    _chk(out_grad, "out_grad", ndim=5)
    _chk(rois, "rois", ndim=3)
    _chk(maxidx_x, "maxidx_x", ndim=5)
    _chk(maxidx_y, "maxidx_y", ndim=5)
    B, R, C, ph, pw = out_grad.shape
    rd = _req_of(req_data)
    if d_feats is None:
        if rd == REQ["add"]:
            raise ValueError("req_data='add' needs d_feats")
        d_feats = [torch.empty(tuple(s), device=out_grad.device, dtype=torch.float32)
                   for s in feat_shapes]
    for i, f in enumerate(d_feats):
        _chk(f, "d_feats[%d]" % i, ndim=4)
    _call("sd_fpn_roi_align_bwd", out_grad, rois, maxidx_x, maxidx_y, _parr(d_feats),
          _iarr([f.shape[2] for f in d_feats]), _iarr([f.shape[3] for f in d_feats]), _iarr(rcnn_stride),
          len(d_feats), rd, B, C, R, ph, pw, roi_canonical_scale, roi_canonical_level)
    return d_feats


# --------------------------------------------------------------------------------------------------
# ROIPooling_v1  (operator_cxx/roi_pooling_v1{-inl.h,.cc,.cu})
# --------------------------------------------------------------------------------------------------
def roi_pool_v1_forward(data, rois, pooled_size, spatial_scale):
    """ROIPooling_v1 forward: data (B,C,H,W), rois (K,5) -> output, maxidx (K,C,ph,pw)
    (shape inference roi_pooling_v1-inl.h:172-199)."""
    _chk(data, "data", ndim=4)
    _chk(rois, "rois", ndim=2)
    if rois.shape[1] != 5:
        raise ValueError("bbox should be a 2D tensor of shape [batch, 5]")
    ph, pw = _pair(pooled_size)
    B, C, H, W = data.shape
    K = rois.shape[0]
    out = torch.empty((K, C, ph, pw), device=data.device, dtype=torch.float32)
    idx = torch.empty_like(out)
    _call("sd_roi_pool_v1_fwd", data, rois, out, idx, B, C, H, W, K, ph, pw, spatial_scale)
    return out, idx


def roi_pool_v1_backward(out_grad, rois, maxidx, data_shape, spatial_scale, req_data="write",
                         req_rois="write", d_data=None):
    """_backward_ROIPooling_v1: [dY, rois, maxidx] -> [dX, d_rois] (roi_pooling_v1-inl.h:96-133)."""
    _chk(out_grad, "out_grad", ndim=4)
    _chk(rois, "rois", ndim=2)
    _chk(maxidx, "maxidx", ndim=4)
    B, C, H, W = [int(v) for v in data_shape]
    K, Co, ph, pw = out_grad.shape
    if Co != C or rois.shape[0] != K:
        raise ValueError("shape mismatch")
    rd, rr = _req_of(req_data), _req_of(req_rois)
    if d_data is None:
        if rd == REQ["add"]:
            raise ValueError("req_data='add' needs the d_data tensor to accumulate into")
        d_data = torch.empty((B, C, H, W), device=out_grad.device, dtype=torch.float32)
    d_rois = torch.empty_like(rois) if rr != 0 else None
    _call("sd_roi_pool_v1_bwd", out_grad, rois, maxidx, d_data, d_rois, rd, rr, B, C, H, W, K, ph, pw, spatial_scale)
    return d_data, d_rois


# --------------------------------------------------------------------------------------------------
# _contrib_DeformablePSROIPooling (upstream MXNet) and TSD's fused FPN extractor
# (models/TSD/poolings.py:51-174)
# --------------------------------------------------------------------------------------------------
def _grad_buf(t, name, shape, rd, dev):
    """_out for a gradient written under req `rd`: 'add' has nothing to add to in a fresh tensor"""
    if t is None and rd == REQ["add"]:
        raise ValueError("req 'add' needs the %s tensor to accumulate into" % name)
    return _out(t, name, shape, dev)


def _dpsroi_dims(data, rois, trans, output_dim, pooled_size, part_size, no_trans):
    _chk(data, "data", ndim=4)
    _chk(rois, "rois", ndim=2)
    if rois.shape[1] != 5:
        raise ValueError("rois should be a 2D tensor of shape [K, 5]")
    K, P = rois.shape[0], int(pooled_size)
    part = int(part_size) or P
    ncls = 1
    if not no_trans:
        _chk(trans, "trans", ndim=4)
        if trans.shape[0] != K or trans.shape[1] % 2 or trans.shape[1] < 2 or tuple(trans.shape[2:]) != (part, part):
            raise ValueError("trans should have shape (K, 2 * num_classes, %d, %d), got %s"
                             % (part, part, tuple(trans.shape)))
        ncls = trans.shape[1] // 2
    return K, P, ncls


def deform_psroi_pool_forward(data, rois, trans=None, *, spatial_scale, output_dim, group_size, pooled_size,
                              part_size=0, sample_per_part=1, trans_std=0.0, no_trans=False, out=None,
                              top_count=None):
    """_contrib_DeformablePSROIPooling forward: data (B,C,H,W), rois (K,5), trans (K,2*num_classes,part,part)
    -> out, top_count (K,output_dim,P,P).  top_count is the operator's hidden output, the backward's state."""
    K, P, ncls = _dpsroi_dims(data, rois, trans, output_dim, pooled_size, part_size, no_trans)
    B, C, H, W = data.shape
    shape = (K, int(output_dim), P, P)
    out = _out(out, "out", shape, data.device)
    top_count = _out(top_count, "top_count", shape, data.device)
    _call("sd_deform_psroi_pool_fwd", data, rois, None if no_trans else trans, out, top_count, B, C, H, W, K, ncls,
          spatial_scale, int(output_dim), int(group_size), P, int(part_size), int(sample_per_part), trans_std,
          bool(no_trans))
    return out, top_count


def deform_psroi_pool_backward(out_grad, data, rois, trans, top_count, *, spatial_scale, output_dim, group_size,
                               pooled_size, part_size=0, sample_per_part=1, trans_std=0.0, no_trans=False,
                               req_data="write", req_rois="write", req_trans="write", d_data=None, d_trans=None):
    """-> d_data, d_rois (zeros on write, None otherwise), d_trans (None when no_trans or req_trans null)"""
    K, P, ncls = _dpsroi_dims(data, rois, trans, output_dim, pooled_size, part_size, no_trans)
    B, C, H, W = data.shape
    shape = (K, int(output_dim), P, P)
    _chk(out_grad, "out_grad", ndim=4)
    _chk(top_count, "top_count", ndim=4)
    if tuple(out_grad.shape) != shape or tuple(top_count.shape) != shape:
        raise ValueError("out_grad / top_count should have shape %s" % (shape,))
    rd, rr, rt = _req_of(req_data), _req_of(req_rois), _req_of(req_trans)
    if no_trans:
        rt = 0
    if rd:
        d_data = _grad_buf(d_data, "d_data", tuple(data.shape), rd, data.device)
    if rt:
        d_trans = _grad_buf(d_trans, "d_trans", tuple(trans.shape), rt, data.device)
    d_rois = torch.empty_like(rois) if rr == REQ["write"] else None
    _call("sd_deform_psroi_pool_bwd", out_grad, data, rois, None if no_trans else trans, top_count,
          d_data if rd else None, d_rois, d_trans if rt else None, rd, rr, rt, B, C, H, W, K, ncls, spatial_scale,
          int(output_dim), int(group_size), P, int(part_size), int(sample_per_part), trans_std, bool(no_trans))
    return (d_data if rd else None), d_rois, (d_trans if rt else None)


class DeformPSROIPoolFunction(torch.autograd.Function):
    """out = f(data, rois, trans); rois gets a zero gradient like the operator's"""

    @staticmethod
    def forward(ctx, data, rois, trans, kw):
        kw = dict(kw)
        out, top_count = deform_psroi_pool_forward(data, rois, trans, **kw)
        ctx.kw = kw
        ctx.save_for_backward(data, rois, trans, top_count)
        return out

    @staticmethod
    def backward(ctx, dy):
        data, rois, trans, top_count = ctx.saved_tensors
        need_t = trans is not None and ctx.needs_input_grad[2]
        dd, dr, dt = deform_psroi_pool_backward(dy.contiguous(), data, rois, trans, top_count,
                                                req_data="write" if ctx.needs_input_grad[0] else "null",
                                                req_rois="write" if ctx.needs_input_grad[1] else "null",
                                                req_trans="write" if need_t else "null", **ctx.kw)
        return dd, dr, dt, None


def deform_psroi_pool(data, rois, trans=None, **kw):
    return DeformPSROIPoolFunction.apply(data, rois, trans, kw)


def _fpn_dpool_dims(feats, rois, trans, rcnn_stride, pooled_size):
    _chk(rois, "rois", ndim=3)
    if rois.shape[2] != 4:
        raise ValueError("rois should be a 3D tensor of shape [batch, rois, 4]")
    B, C, R, Hs, Ws = _fpn_levels(feats, rois, rcnn_stride)
    P = int(pooled_size)
    _chk(trans, "trans")
    if tuple(trans.shape) == (B * R, 2, P, P):
        tpart = P
    elif tuple(trans.shape) in ((B * R, 2), (B * R, 2, 1, 1)):
        tpart = 1
    else:
        raise ValueError("trans should have shape (B*R, 2, P, P) or (B*R, 2), got %s" % (tuple(trans.shape),))
    return B, C, R, P, tpart, Hs, Ws


def fpn_deform_roi_pool_forward(feats, rois, trans, rcnn_stride, pooled_size, sample_per_part=4, trans_std=0.1,
                                roi_canonical_scale=224, roi_canonical_level=4, out=None, top_count=None):
    """FPNRoIAlign_DeltaC / DeltaR.get_roi_feature (models/TSD/poolings.py:51-174) as one launch.

    feats: list of (B,C,H_l,W_l); rois (B,R,4); trans (B*R,2,P,P) (DeltaC) or (B*R,2) (DeltaR)
    -> out (B*R,C,P,P), top_count (B*R,nlvl,P,P)."""
    B, C, R, P, tpart, Hs, Ws = _fpn_dpool_dims(feats, rois, trans, rcnn_stride, pooled_size)
    out = _out(out, "out", (B * R, C, P, P), rois.device)
    top_count = _out(top_count, "top_count", (B * R, len(feats), P, P), rois.device)
    _call("sd_fpn_deform_roi_pool_fwd", _parr(feats), Hs, Ws, _iarr(rcnn_stride), len(feats), rois, trans, out,
          top_count, B, C, R, P, tpart, int(sample_per_part), trans_std, roi_canonical_scale, roi_canonical_level)
    return out, top_count


def fpn_deform_roi_pool_backward(out_grad, feats, rois, trans, top_count, rcnn_stride, pooled_size,
                                 sample_per_part=4, trans_std=0.1, roi_canonical_scale=224, roi_canonical_level=4,
                                 req_data="write", req_trans="write", d_feats=None, d_trans=None):
    """-> [d_feat per level] (None when req_data null), d_trans (None when req_trans null)"""
    B, C, R, P, tpart, Hs, Ws = _fpn_dpool_dims(feats, rois, trans, rcnn_stride, pooled_size)
    _chk(out_grad, "out_grad", ndim=4)
    _chk(top_count, "top_count", ndim=4)
    if tuple(out_grad.shape) != (B * R, C, P, P) or tuple(top_count.shape) != (B * R, len(feats), P, P):
        raise ValueError("out_grad / top_count shape mismatch")
    rd, rt = _req_of(req_data), _req_of(req_trans)
    if rd:
        if d_feats is None:
            d_feats = [None] * len(feats)
        d_feats = [_grad_buf(d, "d_feats[%d]" % i, tuple(f.shape), rd, rois.device)
                   for i, (d, f) in enumerate(zip(d_feats, feats))]
    if rt:
        d_trans = _grad_buf(d_trans, "d_trans", tuple(trans.shape), rt, rois.device)
    _call("sd_fpn_deform_roi_pool_bwd", out_grad, _parr(feats), _parr(d_feats) if rd else None, Hs, Ws,
          _iarr(rcnn_stride), len(feats), rois, trans, top_count, d_trans if rt else None, rd, rt, B, C, R, P, tpart,
          int(sample_per_part), trans_std, roi_canonical_scale, roi_canonical_level)
    return (d_feats if rd else None), (d_trans if rt else None)


class FpnDeformRoiPoolFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, trans, kw, *feats):
        kw = dict(kw)
        out, top_count = fpn_deform_roi_pool_forward(list(feats), rois, trans, **kw)
        ctx.kw = kw
        ctx.save_for_backward(rois, trans, top_count, *feats)
        return out

    @staticmethod
    def backward(ctx, dy):
        rois, trans, top_count, *feats = ctx.saved_tensors
        need_d = any(ctx.needs_input_grad[3:])
        dfs, dt = fpn_deform_roi_pool_backward(dy.contiguous(), feats, rois, trans, top_count,
                                               req_data="write" if need_d else "null",
                                               req_trans="write" if ctx.needs_input_grad[1] else "null", **ctx.kw)
        return (None, dt, None) + tuple(dfs if need_d else [None] * len(feats))


def fpn_deform_roi_pool(feats, rois, trans, rcnn_stride, pooled_size, **kw):
    kw = dict(kw, rcnn_stride=list(rcnn_stride), pooled_size=pooled_size)
    return FpnDeformRoiPoolFunction.apply(rois, trans, kw, *feats)


# --------------------------------------------------------------------------------------------------
# _contrib_GenAnchor  (operator_cxx/contrib/generate_anchor{-inl.h,.cc,.cu})
# --------------------------------------------------------------------------------------------------
def _darr(vals):
    return (ctypes.c_double * len(vals))(*[float(v) for v in vals])


def gen_anchor(height, width, feature_stride, scales, ratios, device=None):
    """GenAnchor: (H*W*A, 4) fp32 anchors, row (h*W + w)*A + a, A ratio-major
    (generate_anchor-inl.h:176-180; shape generate_anchor-inl.h:92-106)."""
    scales, ratios = list(scales), list(ratios)
    device = device or torch.device("cuda", torch.cuda.current_device())
    A = len(scales) * len(ratios)
    out = torch.empty((int(height) * int(width) * A, 4), device=device, dtype=torch.float32)
    _call("sd_gen_anchor", out, int(height), int(width), int(feature_stride), _darr(scales), len(scales),
          _darr(ratios), len(ratios))
    return out


def gen_anchor_levels(shapes, strides, scales, ratios, device=None):
    """GenAnchor for every pyramid level in one launch: shapes [(H, W), ...], strides [...] ->
    list of (H*W*A, 4) tensors (each equal to gen_anchor of that level)."""
    scales, ratios = list(scales), list(ratios)
    device = device or torch.device("cuda", torch.cuda.current_device())
    A = len(scales) * len(ratios)
    outs = [torch.empty((int(h) * int(w) * A, 4), device=device, dtype=torch.float32) for h, w in shapes]
    _call("sd_gen_anchor_levels", _parr(outs), _iarr([h for h, _ in shapes]), _iarr([w for _, w in shapes]),
          _iarr(strides), len(outs), _darr(scales), len(scales), _darr(ratios), len(ratios))
    return outs


# --------------------------------------------------------------------------------------------------
# ProposalTarget  (operator_cxx/proposal_target{-inl.h,.cc})
# --------------------------------------------------------------------------------------------------
class ProposalTargetParam(ctypes.Structure):
    """sd_proposal_target_param == ProposalTargetParam (proposal_target-inl.h:81-114)."""
    _fields_ = [("num_classes", ctypes.c_int), ("batch_images", ctypes.c_int),
                ("image_rois", ctypes.c_int), ("fg_fraction", ctypes.c_float),
                ("fg_thresh", ctypes.c_float), ("bg_thresh_hi", ctypes.c_float),
                ("bg_thresh_lo", ctypes.c_float), ("proposal_without_gt", ctypes.c_int),
                ("class_agnostic", ctypes.c_int), ("bbox_mean", ctypes.c_float * 4),
                ("bbox_std", ctypes.c_float * 4), ("bbox_weight", ctypes.c_float * 4)]


def glibc_rand_state(seed=1, device=None):
    """Device copy of libc's rand() state after srand(seed) (33 int32).  seed=1 is the state of a
    process that never called srand -- what the reference op sees (no srand anywhere in it)."""
    host = (ctypes.c_int32 * 33)()
    _call("sd_glibc_srand_host", seed, host)
    device = device or torch.device("cuda", torch.cuda.current_device())
    return torch.tensor(list(host), dtype=torch.int32, device=device)


_default_rng = {}


def default_rng_state(device=None, reset_seed=None):
    """The process-wide (per device) glibc rand() state ProposalTarget advances when the caller
    passes none -- libc's global state in the reference.  reset_seed re-seeds it (srand)."""
    device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if reset_seed is not None or device not in _default_rng:
        _default_rng[device] = glibc_rand_state(1 if reset_seed is None else reset_seed, device)
    return _default_rng[device]


def proposal_target(rois, gt_boxes, num_classes, batch_images, image_rois, fg_fraction=0.25,
                    fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, proposal_without_gt=False,
                    class_agnostic=False, bbox_mean=(0., 0., 0., 0.), bbox_std=(.1, .1, .2, .2),
                    bbox_weight=(1., 1., 1., 1.), rng_state=None, return_index=False,
                    valid_ranges=None, filter_scales=False):
    """ProposalTarget: rois (B,N,4), gt_boxes (B,M,5) -> roi_output (B,S,4), label (B,S),
    bbox_target (B,S,4K), bbox_weight (B,S,4K), match_gt_iou (B,S)  (proposal_target-inl.h:297-330).
    rng_state: int32[33] device tensor from glibc_rand_state(); advanced in place.
    valid_ranges (B,2) selects ProposalTarget_v2 (proposal_target_v2-inl.h), with filter_scales."""
    _chk(rois, "rois", ndim=3)
    _chk(gt_boxes, "gt_boxes", ndim=3)
    B, N, _ = rois.shape
    if rois.shape[2] != 4 or gt_boxes.shape[2] != 5 or gt_boxes.shape[0] != B:
        raise ValueError("rois must be (B,N,4) and gt_boxes (B,M,5)")
    if B != int(batch_images):
        raise ValueError("batch_images=%d but rois has batch %d" % (batch_images, B))
    M = gt_boxes.shape[1]
    p = ProposalTargetParam()
    p.num_classes, p.batch_images, p.image_rois = int(num_classes), int(batch_images), int(image_rois)
    p.fg_fraction, p.fg_thresh = float(fg_fraction), float(fg_thresh)
    p.bg_thresh_hi, p.bg_thresh_lo = float(bg_thresh_hi), float(bg_thresh_lo)
    p.proposal_without_gt, p.class_agnostic = int(bool(proposal_without_gt)), int(bool(class_agnostic))
    for i in range(4):
        p.bbox_mean[i], p.bbox_std[i], p.bbox_weight[i] = bbox_mean[i], bbox_std[i], bbox_weight[i]
    if rng_state is None:
        # the reference never calls srand: libc's global state starts at seed 1 and ADVANCES from
        # call to call, so every step draws a fresh stretch of the rand() stream.  Keep one such
        # state per device for callers that do not manage their own (mx.sym.ProposalTarget has no
        # rng argument).
        rng_state = default_rng_state(rois.device)
    _chk(rng_state, "rng_state", dtype=torch.int32, ndim=1)
    if rng_state.numel() != 33:
        raise ValueError("rng_state must hold 33 int32 words (glibc_rand_state), got %d"
                         % rng_state.numel())
    S, K4 = int(image_rois), 4 * int(num_classes)
    dev = rois.device
    ro = torch.empty((B, S, 4), device=dev, dtype=torch.float32)
    lb = torch.empty((B, S), device=dev, dtype=torch.float32)
    bt = torch.empty((B, S, K4), device=dev, dtype=torch.float32)
    bw = torch.empty((B, S, K4), device=dev, dtype=torch.float32)
    iou = torch.empty((B, S), device=dev, dtype=torch.float32)
    kept = torch.empty((B, S), device=dev, dtype=torch.int32) if return_index else None
    ws = _ws(dev, None, "sd_proposal_target_workspace_bytes", B, N, M)
    if valid_ranges is not None:
        _chk(valid_ranges, "valid_ranges", ndim=2)
        if tuple(valid_ranges.shape) != (B, 2):
            raise ValueError("valid_ranges must be (B,2)")
        _call("sd_proposal_target_v2", rois, gt_boxes, valid_ranges, bool(filter_scales), N, M, ctypes.byref(p),
              rng_state, ro, lb, bt, bw, iou, kept, ws, ws.numel())
    else:
        _call("sd_proposal_target", rois, gt_boxes, N, M, ctypes.byref(p), rng_state, ro, lb, bt, bw, iou, kept, ws,
              ws.numel())
    res = (ro, lb, bt, bw, iou)
    return res + (kept,) if return_index else res


def proposal_mask_target(rois, gt_boxes, gt_polys, num_classes, batch_images, image_rois, mask_size=28,
                         fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0,
                         proposal_without_gt=False, class_agnostic=False, bbox_mean=(0., 0., 0., 0.),
                         bbox_std=(.1, .1, .2, .2), bbox_weight=(1., 1., 1., 1.), rng_state=None,
                         valid_ranges=None, filter_scales=False, return_index=False, output_ratio=False,
                         max_raster_pixels=1408 * 1408):
    """ProposalMaskTarget (proposal_mask_target-inl.h): ProposalTarget_v2's five outputs plus
    mask_target (B, int(image_rois*fg_fraction), mask_size, mask_size): the 0/1 mask of each sampled
    foreground RoI's gt polygon in the RoI's frame, -1 rows past the sampled foreground.
    gt_polys (B,M,L): [category, n_seg, len_1..len_n, x,y,...] padded with -1.
    output_ratio=True (mask scoring R-CNN, proposal_mask_target.cc:20-152) appends mask_ratio (B, FG)
    after mask_target; max_raster_pixels bounds the image-resolution rasters it counts (a row whose
    RoI or RoI-and-polygon bounding box has more pixels gets NaN)."""
    _chk(rois, "rois", ndim=3)
    _chk(gt_boxes, "gt_boxes", ndim=3)
    _chk(gt_polys, "gt_polys", ndim=3)
    B, N, _ = rois.shape
    M, L = gt_boxes.shape[1], gt_polys.shape[2]
    if gt_polys.shape[:2] != gt_boxes.shape[:2] or B != int(batch_images):
        raise ValueError("gt_polys must be (B,M,L) like gt_boxes (B,M,5), B = batch_images")
    p = ProposalTargetParam()
    p.num_classes, p.batch_images, p.image_rois = int(num_classes), int(batch_images), int(image_rois)
    p.fg_fraction, p.fg_thresh = float(fg_fraction), float(fg_thresh)
    p.bg_thresh_hi, p.bg_thresh_lo = float(bg_thresh_hi), float(bg_thresh_lo)
    p.proposal_without_gt, p.class_agnostic = int(bool(proposal_without_gt)), int(bool(class_agnostic))
    for i in range(4):
        p.bbox_mean[i], p.bbox_std[i], p.bbox_weight[i] = bbox_mean[i], bbox_std[i], bbox_weight[i]
    if rng_state is None:
        rng_state = default_rng_state(rois.device)
    _chk(rng_state, "rng_state", dtype=torch.int32, ndim=1)
    if rng_state.numel() != 33:
        raise ValueError("rng_state must hold 33 int32 words")
    if valid_ranges is not None:
        _chk(valid_ranges, "valid_ranges", ndim=2)
    S, K4 = int(image_rois), 4 * int(num_classes)
    FG = int(torch.tensor(S, dtype=torch.float32) * torch.tensor(fg_fraction, dtype=torch.float32))
    dev = rois.device
    ro = torch.empty((B, S, 4), device=dev, dtype=torch.float32)
    lb = torch.empty((B, S), device=dev, dtype=torch.float32)
    bt = torch.empty((B, S, K4), device=dev, dtype=torch.float32)
    bw = torch.empty((B, S, K4), device=dev, dtype=torch.float32)
    iou = torch.empty((B, S), device=dev, dtype=torch.float32)
    mask = torch.empty((B, FG, int(mask_size), int(mask_size)), device=dev, dtype=torch.float32)
    kept = torch.empty((B, S), device=dev, dtype=torch.int32) if return_index else None
    if output_ratio:
        ratio = torch.empty((B, FG), device=dev, dtype=torch.float32)
        ws = _ws(dev, None, "sd_proposal_mask_target_ratio_workspace_bytes", B, N, M, S, fg_fraction,
                 int(max_raster_pixels))
        _call("sd_proposal_mask_target_ratio", rois, gt_boxes, gt_polys, valid_ranges, bool(filter_scales), N, M, L,
              int(mask_size), ctypes.byref(p), rng_state, ro, lb, bt, bw, iou, mask, ratio, int(max_raster_pixels),
              kept, ws, ws.numel())
        res = (ro, lb, bt, bw, iou, mask, ratio)
        return res + (kept,) if return_index else res
    ws = _ws(dev, None, "sd_proposal_target_workspace_bytes", B, N, M)
    _call("sd_proposal_mask_target", rois, gt_boxes, gt_polys, valid_ranges, bool(filter_scales), N, M, L,
          int(mask_size), ctypes.byref(p), rng_state, ro, lb, bt, bw, iou, mask, kept, ws, ws.numel())
    res = (ro, lb, bt, bw, iou, mask)
    return res + (kept,) if return_index else res


# --------------------------------------------------------------------------------------------------
# RPN anchor-target assignment (core/detection_input.py:345-565, models/FPN/input.py:9-146)
# --------------------------------------------------------------------------------------------------
class RpnTargetParam(ctypes.Structure):
    """sd_rpn_target_param"""
    _fields_ = [("nlvl", ctypes.c_int), ("stride", ctypes.c_int * 8), ("short_side", ctypes.c_int * 8),
                ("long_side", ctypes.c_int * 8), ("n_scales", ctypes.c_int), ("n_aspects", ctypes.c_int),
                ("scales", ctypes.c_double * 16), ("aspects", ctypes.c_double * 16),
                ("allowed_border", ctypes.c_int), ("pos_thr", ctypes.c_float), ("neg_thr", ctypes.c_float),
                ("min_pos_thr", ctypes.c_float), ("image_anchor", ctypes.c_int),
                ("pos_fraction", ctypes.c_double)]


def _seq(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


def rpn_target_param(stride, short, long, scales, aspects, allowed_border=0, pos_thr=0.7, neg_thr=0.3,
                     min_pos_thr=0.0, image_anchor=256, pos_fraction=0.5):
    """the AnchorTarget2DParam of a config (config/faster_r50v1_fpn_1x.py:212-232) as the C struct"""
    p = RpnTargetParam()
    st, sh, lg, sc, asp = _seq(stride), _seq(short), _seq(long), _seq(scales), _seq(aspects)
    if not (len(st) == len(sh) == len(lg)) or len(st) > 8 or len(sc) * len(asp) > 16:
        raise ValueError("bad pyramid / anchor description")
    p.nlvl, p.n_scales, p.n_aspects = len(st), len(sc), len(asp)
    for i in range(len(st)):
        p.stride[i], p.short_side[i], p.long_side[i] = int(st[i]), int(sh[i]), int(lg[i])
    for i, v in enumerate(sc):
        p.scales[i] = float(v)
    for i, v in enumerate(asp):
        p.aspects[i] = float(v)
    p.allowed_border = int(allowed_border)
    p.pos_thr, p.neg_thr, p.min_pos_thr = float(pos_thr), float(neg_thr), float(min_pos_thr)
    p.image_anchor, p.pos_fraction = int(image_anchor), float(pos_fraction)
    return p


def mt19937_state(seed=None, numpy_state=None, device=None):
    """Device copy (int32[625]) of a numpy RandomState: np.random.seed(seed), or an explicit
    RandomState.get_state() tuple."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    host = (ctypes.c_int32 * 625)()
    if numpy_state is not None:
        key, pos = numpy_state[1], int(numpy_state[2])
        vals = [int(k) - (1 << 32) if int(k) >= (1 << 31) else int(k) for k in key] + [pos]
        return torch.tensor(vals, dtype=torch.int32, device=device)
    _call("sd_mt19937_seed_host", int(seed), host)
    return torch.tensor(list(host), dtype=torch.int32, device=device)


def rpn_anchor_target(im_info, gt_bbox, param, mt_state, layout=1):
    """RPN labels / box targets / weights for a batch of images, the reference loader's
    (Pyramid)AnchorTarget2D on the device.  im_info (B,3), gt_bbox (B,M,4|5) padded with -1 rows.
    layout 1: cls_label (B, A*sumHW), reg_target / reg_weight (B, 4A, sumHW); layout 0: (B,N), (B,N,4).
    mt_state: mt19937_state(...), advanced in place like np.random."""
    _chk(im_info, "im_info", ndim=2)
    _chk(gt_bbox, "gt_bbox", ndim=3)
    _chk(mt_state, "mt_state", dtype=torch.int32, ndim=1)
    if mt_state.numel() != 625:
        raise ValueError("mt_state must hold 625 int32 words")
    B, M, G = gt_bbox.shape
    N = _query("sd_rpn_target_num_anchors", ctypes.byref(param))
    if N < 0:
        raise ValueError("bad rpn target parameters")
    A = param.n_scales * param.n_aspects
    dev = im_info.device
    if layout == 1:
        cls = torch.empty((B, N), device=dev, dtype=torch.float32)
        tgt = torch.empty((B, 4 * A, N // A), device=dev, dtype=torch.float32)
        wgt = torch.empty_like(tgt)
    else:
        cls = torch.empty((B, N), device=dev, dtype=torch.float32)
        tgt = torch.empty((B, N, 4), device=dev, dtype=torch.float32)
        wgt = torch.empty_like(tgt)
    ws = _ws(dev, None, "sd_rpn_target_workspace_bytes", ctypes.byref(param), B, M)
    _call("sd_rpn_anchor_target", im_info, gt_bbox, B, M, G, ctypes.byref(param), mt_state, cls, tgt, wgt,
          int(layout), ws, ws.numel())
    return cls, tgt, wgt


def retina_anchor_target(im_info, gt_bbox, param, layout=1, workspace=None):
    """RetinaNet labels / box targets / weights / foreground counts for a batch of images: the loader's
    PyramidAnchorTarget2D of models/retinanet/input.py:33-199 on the device (class-valued labels, no
    subsampling, a target for every valid anchor).  im_info (B,3), gt_bbox (B,M,5) padded with -1 rows;
    param: rpn_target_param(...), of which image_anchor / pos_fraction are ignored.
    layout 1: cls_label (B, N) as per-level (A, fh, fw) blocks, reg_target / reg_weight (B, 4A, sumHW);
    layout 0: (B,N), (B,N,4) in all-anchor order.  fg_count (B,) = max(1, #(label > 0))."""
    _chk(im_info, "im_info", ndim=2)
    _chk(gt_bbox, "gt_bbox", ndim=3)
    B, M, G = gt_bbox.shape
    if G != 5 or im_info.shape != (B, 3):
        raise ValueError("gt_bbox must be (B,M,5) and im_info (B,3)")
    N = _query("sd_rpn_target_num_anchors", ctypes.byref(param))
    if N < 0:
        raise ValueError("bad anchor target parameters")
    A = param.n_scales * param.n_aspects
    dev = im_info.device
    cls = torch.empty((B, N), device=dev, dtype=torch.float32)
    tgt = torch.empty((B, 4 * A, N // A) if layout == 1 else (B, N, 4), device=dev, dtype=torch.float32)
    wgt = torch.empty_like(tgt)
    fg = torch.empty((B,), device=dev, dtype=torch.float32)
    ws = _ws(dev, workspace, "sd_retina_target_workspace_bytes", ctypes.byref(param), B, M)
    _call("sd_retina_anchor_target", im_info, gt_bbox, B, M, ctypes.byref(param), cls, tgt, wgt, fg, int(layout), ws,
          ws.numel())
    return cls, tgt, wgt, fg


# --------------------------------------------------------------------------------------------------
# _contrib_FocalLoss / _contrib_BBoxNorm  (operator_cxx/contrib/focal_loss-inl.h, bbox_norm-inl.h;
# models/retinanet/builder.py:289-324)
# --------------------------------------------------------------------------------------------------
NORMALIZATION = {"null": 0, "batch": 1, "valid": 2}


def focal_loss_workspace_bytes():
    return _query("sd_focal_loss_workspace_bytes")


def focal_loss_forward(data, out=None):
    """FocalLoss forward: out = sigmoid(data), any shape (focal_loss-inl.h:113)."""
    _chk(data, "data")
    if out is None:
        out = torch.empty_like(data)
    else:
        _chk(out, "out")
        if out.shape != data.shape:
            raise ValueError("out must have the shape of data")
    _call("sd_focal_loss_fwd", data, out, data.numel())
    return out


def focal_loss_backward(out, label, ograd=None, *, alpha=0.25, gamma=2.0, grad_scale=1.0,
                        normalization="valid", gdata=None, workspace=None):
    """FocalLoss backward (focal_loss-inl.h:186-230): out (B,nbox,nclass) = the forward's sigmoid,
    label (B,nbox) in {-1 ignore, 0 background, 1..nclass}; ograd (same shape as out) only for the
    op's out_grad=True.  normalization 'valid' divides by (#(label >= 1) over the batch + 1), counted
    on the device; 'batch' by B; 'null' by nothing.  Returns gdata."""
    _chk(out, "out", ndim=3)
    _chk(label, "label", ndim=2)
    B, nbox, nclass = out.shape
    if label.shape != (B, nbox):
        raise ValueError("label must be (B, nbox) = %s, got %s" % ((B, nbox), tuple(label.shape)))
    if ograd is not None:
        _chk(ograd, "ograd", ndim=3)
        if ograd.shape != out.shape:
            raise ValueError("ograd must have the shape of out")
    if normalization not in NORMALIZATION:
        raise ValueError("normalization must be one of %s" % sorted(NORMALIZATION))
    if gdata is None:
        gdata = torch.empty_like(out)
    else:
        _chk(gdata, "gdata", ndim=3)
        if gdata.shape != out.shape:
            raise ValueError("gdata must have the shape of out")
    ws = _ws(out.device, workspace, "sd_focal_loss_workspace_bytes")
    _call("sd_focal_loss_bwd", out, label, ograd, gdata, B, nbox, nclass, alpha, gamma, grad_scale,
          NORMALIZATION[normalization], ws, ws.numel())
    return gdata


def bbox_norm_backward(gout, label, gdata=None, workspace=None):
    """BBoxNorm backward (bbox_norm-inl.h:116-126): gout (B, ...), label (B, ...);
    gdata = gout / max(1, #(label >= 1) over the batch + 1).  The forward is the identity."""
    _chk(gout, "gout")
    _chk(label, "label")
    if gout.dim() < 1 or label.dim() < 1 or gout.shape[0] != label.shape[0]:
        raise ValueError("gout and label must share the batch dimension")
    B = gout.shape[0]
    if gdata is None:
        gdata = torch.empty_like(gout)
    else:
        _chk(gdata, "gdata")
        if gdata.shape != gout.shape:
            raise ValueError("gdata must have the shape of gout")
    ws = _ws(gout.device, workspace, "sd_focal_loss_workspace_bytes")
    _call("sd_bbox_norm_bwd", gout, label, gdata, B, gout.numel() // B if B else 0, label.numel() // B if B else 0,
          ws, ws.numel())
    return gdata


# --------------------------------------------------------------------------------------------------
# _contrib_GroupNorm  (operator_cxx/contrib/group_norm{-inl.h,.cu}, group_norm_helper.cu)
# --------------------------------------------------------------------------------------------------
def group_norm_workspace_bytes(N, C, HxW, num_group):
    return _query("sd_group_norm_workspace_bytes", int(N), int(C), int(HxW), int(num_group))


def _gn_dims(x, gamma, num_group):
    _chk(x, "data")
    if x.dim() < 2:
        raise ValueError("data should be (batch, channel, ...), got shape %s" % (tuple(x.shape),))
    N, C = int(x.shape[0]), int(x.shape[1])
    G = int(num_group)
    if G <= 0 or C % G:
        raise ValueError("channels (%d) are not divisible by num_group (%d)" % (C, G))
    _chk(gamma, "gamma", ndim=1)
    if gamma.shape[0] != C:
        raise ValueError("gamma must have %d entries, got %d" % (C, gamma.shape[0]))
    return N, C, (x.numel() // (N * C) if N * C else 0), G


def group_norm_forward(x, gamma, beta, num_group=32, eps=1e-5, y=None, mu=None, rsig=None, workspace=None):
    """_contrib_GroupNorm forward (group_norm.cu:71-91,198-233): x (N,C,...) NCHW, gamma / beta (C,)
    -> y (the shape of x), mu (N,G), rsig (N,G) = 1 / sqrt(biased variance + eps), the variance taken about
    the mean.  mu / rsig passed in may be larger (the reference declares them (N,C)): the first N*G floats are
    written, the rest is left alone."""
    N, C, HxW, G = dims = _gn_dims(x, gamma, num_group)
    _chk(beta, "beta", ndim=1)
    if beta.shape[0] != C:
        raise ValueError("beta must have %d entries, got %d" % (C, beta.shape[0]))
    y = _out(y, "y", x.shape, x.device)
    # mu / rsig the caller passes may be larger than (N,G): only their size is checked
    mu = torch.empty((N, G), device=x.device, dtype=torch.float32) if mu is None else _chk(mu, "mu", at_least=N * G)
    rsig = (torch.empty((N, G), device=x.device, dtype=torch.float32) if rsig is None
            else _chk(rsig, "rsig", at_least=N * G))
    ws = _ws(x.device, workspace, "sd_group_norm_workspace_bytes", *dims)
    _call("sd_group_norm_fwd", x, gamma, beta, y, mu, rsig, N, C, HxW, G, eps, ws, ws.numel())
    return y, mu, rsig


def group_norm_backward(dy, x, mu, rsig, gamma, num_group=32, dx=None, dgamma=None, dbeta=None, param_grads=True,
                        workspace=None):
    """_contrib_GroupNorm backward (group_norm.cu:93-196,235-298): dy / x (N,C,...), mu / rsig the forward's
    (their first N*G floats are read), gamma (C,) -> dx, dgamma, dbeta (written, not accumulated).
    param_grads=False skips dgamma / dbeta and returns None for them."""
    N, C, HxW, G = dims = _gn_dims(x, gamma, num_group)
    _chk(dy, "dy", shape=x.shape)
    _chk(mu, "mu", at_least=N * G)
    _chk(rsig, "rsig", at_least=N * G)
    dx = _out(dx, "dx", x.shape, x.device)
    if param_grads:
        dgamma = _out(dgamma, "dgamma", gamma.shape, x.device)
        dbeta = _out(dbeta, "dbeta", gamma.shape, x.device)
        if N * HxW == 0:   # sums over nothing (the entry point writes nothing on an empty problem)
            dgamma.zero_()
            dbeta.zero_()
    elif dgamma is not None or dbeta is not None:
        raise ValueError("param_grads=False takes no dgamma / dbeta")
    ws = _ws(x.device, workspace, "sd_group_norm_workspace_bytes", *dims)
    _call("sd_group_norm_bwd", dy, x, mu, rsig, gamma, dx, dgamma, dbeta, N, C, HxW, G, ws, ws.numel())
    return dx, dgamma, dbeta


class GroupNormFunction(torch.autograd.Function):
    """y, mu, rsig = GroupNormFunction.apply(x, gamma, beta, num_group, eps); mu and rsig carry no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, num_group, eps):
        y, mu, rsig = group_norm_forward(x, gamma, beta, num_group, eps)
        ctx.save_for_backward(x, gamma, mu, rsig)
        ctx.num_group = int(num_group)
        ctx.mark_non_differentiable(mu, rsig)
        return y, mu, rsig

    @staticmethod
    def backward(ctx, dy, _dmu, _drsig):
        x, gamma, mu, rsig = ctx.saved_tensors
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dgamma, dbeta = group_norm_backward(dy.contiguous(), x, mu, rsig, gamma, ctx.num_group, param_grads=need)
        return (dx if ctx.needs_input_grad[0] else None, dgamma if ctx.needs_input_grad[1] else None,
                dbeta if ctx.needs_input_grad[2] else None, None, None)


def group_norm(x, gamma, beta, num_group=32, eps=1e-5, return_stats=False):
    """mx.sym.contrib.GroupNorm(data, gamma, beta, num_group=32, eps=1e-5) with autograd: y, or
    (y, mu, rsig) with return_stats=True (the operator's two hidden outputs)."""
    y, mu, rsig = GroupNormFunction.apply(x, gamma, beta, int(num_group), float(eps))
    return (y, mu, rsig) if return_stats else y


# --------------------------------------------------------------------------------------------------
# _contrib_BroadcastScale and the merged-BN affine  (operator_cxx/contrib/broadcast_scale-inl.h;
# utils/graph_optimize.py:merge_bn -> BroadcastScale, broadcast_add, the shortcut's add, relu)
# --------------------------------------------------------------------------------------------------
_SBA_DTYPES = (torch.float32, torch.float16)


def scale_bias_act_workspace_bytes(N, C, HxW):
    return _query("sd_scale_bias_act_workspace_bytes", int(N), int(C), int(HxW))


def _sba_act(act):
    if act is None or act == 0:
        return 0
    if act == "relu" or act == 1:
        return 1
    raise ValueError("act must be None or 'relu', got %r" % (act,))


def _sba_dims(x, gamma, name="data"):
    if not isinstance(x, torch.Tensor) or x.dtype not in _SBA_DTYPES:
        raise TypeError("%s must be a float32 or float16 torch.Tensor" % name)
    _chk(x, name, dtype=x.dtype)
    if x.dim() < 2:
        raise ValueError("%s should be (batch, channel, ...), got shape %s" % (name, tuple(x.shape)))
    N, C = int(x.shape[0]), int(x.shape[1])
    gamma = _sba_param(gamma, "gamma", x, C)
    return N, C, (x.numel() // (N * C) if N * C else 0), gamma


def _sba_param(p, name, x, C):
    """(C,) or (1,C,1,1) of x's dtype -> the flat view (two shapes and a reshape: more than _chk's shape= does)"""
    _chk(p, name, dtype=x.dtype)
    if p.numel() != C or (p.dim() != 1 and (p.dim() < 2 or p.shape[1] != C)):
        raise ValueError("%s must have shape (%d,) or (1,%d,1,...), got %s" % (name, C, C, tuple(p.shape)))
    return p.reshape(-1)


def scale_bias_act_forward(x, gamma, beta=None, residual=None, act=None, out=None):
    """y = act((x * gamma[c] + beta[c]) + residual), every step rounded on its own: the nodes merge_bn leaves
    behind a convolution, in one launch.  x (N,C,...) NCHW float32 or float16, gamma / beta (C,) or (1,C,1,1),
    residual like x; beta and residual may be None; act None or "relu" (v > 0 ? v : 0).  out: the output buffer
    (it may be x or residual: the in-place forms)."""
    N, C, HxW, gamma = _sba_dims(x, gamma)
    beta = None if beta is None else _sba_param(beta, "beta", x, C)
    residual = None if residual is None else _chk(residual, "residual", x.dtype, shape=x.shape)
    y = _out(out, "out", x.shape, x.device, x.dtype)
    _call(_fn("sd_scale_bias_act_fwd", x), x, gamma, beta, residual, y, N, C, HxW, _sba_act(act))
    return y


def scale_bias_act_backward(dy, y, gamma, act=None, dx=None, dres=None, dbeta=None, need_dres=False,
                            need_dbeta=False, workspace=None):
    """dy, y (the forward's output; read only under act, may be None without) -> dx, dres, dbeta.
    g1 = dy * (y > 0) under act, dy otherwise; dx = g1 * gamma[c]; dres = g1 (need_dres or a dres buffer);
    dbeta[c] = sum of g1, always float32 (need_dbeta or a dbeta buffer).  dx and dres may be dy.  There is no
    gradient for gamma (the reference writes none)."""
    N, C, HxW, gamma = _sba_dims(dy, gamma, "dy")
    a = _sba_act(act)
    if a:
        if y is None:
            raise ValueError("act='relu' needs y, the forward's output")
        _chk(y, "y", dy.dtype, shape=dy.shape)
    else:
        y = None
    dx = _out(dx, "dx", dy.shape, dy.device, dy.dtype)
    if dres is not None or need_dres:
        dres = _out(dres, "dres", dy.shape, dy.device, dy.dtype)
    if dbeta is None and need_dbeta:
        dbeta = torch.empty(C, device=dy.device, dtype=torch.float32)
    elif dbeta is not None:
        _chk(dbeta, "dbeta", ndim=1)
        if dbeta.shape[0] != C:
            raise ValueError("dbeta must have %d entries, got %d" % (C, dbeta.shape[0]))
    ws = None
    if dbeta is not None:
        if N * HxW == 0:   # a sum over nothing (the entry point writes nothing on an empty problem)
            dbeta.zero_()
        ws = _ws(dy.device, workspace, "sd_scale_bias_act_workspace_bytes", N, C, HxW)
    _call(_fn("sd_scale_bias_act_bwd", dy), dy, y, gamma, dx, dres, dbeta, N, C, HxW, a, ws,
          ws.numel() if ws is not None else 0)
    return dx, dres, dbeta


class ScaleBiasActFunction(torch.autograd.Function):
    """y = ScaleBiasActFunction.apply(x, gamma, beta, residual, act); gamma's gradient is None."""

    @staticmethod
    def forward(ctx, x, gamma, beta, residual, act):
        y = scale_bias_act_forward(x, gamma, beta, residual, act)
        ctx.act = _sba_act(act)
        ctx.beta_shape = None if beta is None else beta.shape
        ctx.beta_dtype = None if beta is None else beta.dtype
        ctx.save_for_backward(gamma, y if ctx.act else None)   # x is never kept
        return y

    @staticmethod
    def backward(ctx, dy):
        gamma, y = ctx.saved_tensors
        need_x, _, need_b, need_r, _ = ctx.needs_input_grad
        need_b = need_b and ctx.beta_shape is not None
        dx, dres, dbeta = scale_bias_act_backward(dy.contiguous(), y, gamma, ctx.act, need_dres=need_r,
                                                  need_dbeta=need_b)
        if dbeta is not None:
            dbeta = dbeta.to(ctx.beta_dtype).reshape(ctx.beta_shape)
        return dx if need_x else None, None, dbeta, dres, None


def scale_bias_act(x, gamma, beta=None, residual=None, act=None):
    """The fused merged-BN node with autograd: act((x * gamma + beta) + residual), gamma / beta per channel.
    Gradients reach x, beta and residual; gamma's is None (BroadcastScaleOp::Backward writes none)."""
    return ScaleBiasActFunction.apply(x, gamma, beta, residual, act)


class BroadcastScaleFunction(torch.autograd.Function):
    """y = BroadcastScaleFunction.apply(x, scaler); scaler's gradient is None."""

    @staticmethod
    def forward(ctx, x, scaler):
        ctx.save_for_backward(scaler)
        return scale_bias_act_forward(x, scaler)

    @staticmethod
    def backward(ctx, dy):
        scaler, = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None
        return scale_bias_act_backward(dy.contiguous(), None, scaler)[0], None


def broadcast_scale(x, scaler):
    """mx.sym.contrib.BroadcastScale(data, scaler) with autograd (broadcast_scale-inl.h:57-103):
    x (N,C,...), scaler (C,) or (1,C,1,1) -> x * scaler over the channel axis."""
    return BroadcastScaleFunction.apply(x, scaler)


# --------------------------------------------------------------------------------------------------
# The FPN top-down pathway  (UpSampling(scale=2, nearest) -> slice_like -> add_n per level:
# models/FPN/builder.py:444-524, models/retinanet/builder.py:498-543, ...)
# --------------------------------------------------------------------------------------------------
FPN_TOPDOWN_MAX_LEVELS = 6


def _ftd_shapes(shapes):
    """[(N,C,H_0,W_0), ..]: level 0 the coarsest, each level at most twice the one before -> N, C, hs, ws"""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    if not 2 <= len(shapes) <= FPN_TOPDOWN_MAX_LEVELS:
        raise ValueError("fpn_topdown takes 2..%d levels (top and 1..%d laterals), got %d"
                         % (FPN_TOPDOWN_MAX_LEVELS, FPN_TOPDOWN_MAX_LEVELS - 1, len(shapes)))
    if any(len(s) != 4 for s in shapes):
        raise ValueError("fpn_topdown: every level should be (N,C,H,W), got %s" % (shapes,))
    N, C = shapes[0][:2]
    for l, s in enumerate(shapes):
        if s[:2] != (N, C):
            raise ValueError("fpn_topdown: level %d has (N,C) = %s, level 0 %s" % (l, s[:2], (N, C)))
        if l and (s[2] > 2 * shapes[l - 1][2] or s[3] > 2 * shapes[l - 1][3]):
            raise ValueError("fpn_topdown: level %d (%d x %d) is larger than twice level %d (%d x %d)"
                             % (l, s[2], s[3], l - 1, shapes[l - 1][2], shapes[l - 1][3]))
    return N, C, [s[2] for s in shapes], [s[3] for s in shapes]


def _ftd_tensor(t, name, dtype, shape=None):
    """_chk for a 4D level that may be float32 or float16: of `dtype`, or with dtype None of either"""
    if not isinstance(t, torch.Tensor) or t.dtype not in _SBA_DTYPES:
        raise TypeError("%s must be a float32 or float16 torch.Tensor" % name)
    return _chk(t, name, dtype=dtype or t.dtype, ndim=4, shape=shape)


def fpn_topdown_forward(top, laterals, outs=None):
    """The whole top-down pathway in one launch: out_l = up2(p_{l-1})[:H_l, :W_l] + lateral_l with p_0 = top and
    p_l = out_l, nearest neighbour (y >> 1, x >> 1), the crop from the origin that slice_like makes.
    top (N,C,H_0,W_0), laterals [lateral_1 .. lateral_{L-1}] from coarse to fine, float32 or float16, each level at
    most twice the one before.  outs: the output buffers (none may overlap an input).  Returns [out_1 .. out_{L-1}]."""
    _ftd_tensor(top, "top", None)
    laterals = list(laterals)
    for k, t in enumerate(laterals):
        _ftd_tensor(t, "laterals[%d]" % k, top.dtype)
    shapes = [top.shape] + [t.shape for t in laterals]
    N, C, hs, ws = _ftd_shapes(shapes)
    if outs is None:
        outs = [torch.empty_like(t) for t in laterals]
    else:
        outs = list(outs)
        if len(outs) != len(laterals):
            raise ValueError("outs must have %d entries, got %d" % (len(laterals), len(outs)))
        for k, t in enumerate(outs):
            _ftd_tensor(t, "outs[%d]" % k, top.dtype, laterals[k].shape)
    _call(_fn("sd_fpn_topdown_fwd", top), top, _parr(laterals), _parr(outs), N, C, _iarr(hs), _iarr(ws), len(shapes))
    return outs


def fpn_topdown_backward(grads, shapes, d_top=None, d_laterals=None, want_finest=False):
    """The pathway's backward in one launch, from the gradients alone (no forward tensor).
    grads [g_1 .. g_{L-1}]: the gradients the consumers of out_l send; an inner one may be None (that output had no
    other consumer), the finest may not.  shapes: the L input shapes, top first.
    D_{L-1} = g_{L-1}; D_l = g_l + S_l; d_top = S_0; d_lateral_l = D_l, S_l the 2 x 2 window sums of D_{l+1} under
    the crop.  d_top / d_laterals: output buffers; an entry of d_laterals may be None (a fresh buffer) or False (not
    wanted: not stored, returned as None).  The finest lateral gradient is grads[-1] itself, no copy, unless
    want_finest or a buffer asks for one.  Returns (d_top, [d_lateral_1 .. d_lateral_{L-1}])."""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    N, C, hs, ws = _ftd_shapes(shapes)
    L = len(shapes)
    grads = list(grads)
    if len(grads) != L - 1:
        raise ValueError("grads must have %d entries, got %d" % (L - 1, len(grads)))
    if grads[-1] is None:
        raise ValueError("the gradient of the finest level must be given")
    g_fin = _ftd_tensor(grads[-1], "grads[%d]" % (L - 2), None, shapes[-1])
    for k, t in enumerate(grads[:-1]):
        if t is not None:
            _ftd_tensor(t, "grads[%d]" % k, g_fin.dtype, shapes[k + 1])
    d_top = (torch.empty(shapes[0], device=g_fin.device, dtype=g_fin.dtype) if d_top is None
             else _ftd_tensor(d_top, "d_top", g_fin.dtype, shapes[0]))
    d_laterals = [None] * (L - 1) if d_laterals is None else list(d_laterals)
    if len(d_laterals) != L - 1:
        raise ValueError("d_laterals must have %d entries, got %d" % (L - 1, len(d_laterals)))
    table, result = [], []
    for k, t in enumerate(d_laterals):
        finest = k == L - 2
        if t is False:
            buf = ret = None
        elif t is None:
            if finest and not want_finest:
                buf, ret = None, g_fin
            else:
                buf = ret = torch.empty(shapes[k + 1], device=g_fin.device, dtype=g_fin.dtype)
        else:
            buf = ret = _ftd_tensor(t, "d_laterals[%d]" % k, g_fin.dtype, shapes[k + 1])
        table.append(buf)
        result.append(ret)
    _call(_fn("sd_fpn_topdown_bwd", g_fin), _parr(grads), d_top, _parr(table), N, C, _iarr(hs), _iarr(ws), L)
    return d_top, result


class FpnTopdownFunction(torch.autograd.Function):
    """outs = FpnTopdownFunction.apply(top, lateral_1, .., lateral_{L-1}); nothing is saved for the backward."""

    @staticmethod
    def forward(ctx, top, *laterals):
        ctx.shapes = [tuple(top.shape)] + [tuple(t.shape) for t in laterals]
        ctx.set_materialize_grads(False)
        return tuple(fpn_topdown_forward(top, laterals))

    @staticmethod
    def backward(ctx, *grads):
        grads = [None if g is None else g.contiguous() for g in grads]
        if all(g is None for g in grads):
            return (None,) * len(ctx.shapes)
        if grads[-1] is None:     # the finest output went unused: its gradient is zero
            ref = next(g for g in grads if g is not None)
            grads[-1] = torch.zeros(ctx.shapes[-1], device=ref.device, dtype=ref.dtype)
        need = ctx.needs_input_grad
        d_top, d_lat = fpn_topdown_backward(grads, ctx.shapes, d_laterals=[None if n else False for n in need[1:]])
        return (d_top if need[0] else None,) + tuple(d_lat)


def fpn_topdown(top, laterals):
    """The FPN top-down pathway with autograd: [out_1 .. out_{L-1}] of fpn_topdown_forward; the backward is
    fpn_topdown_backward on the incoming gradients, and no forward tensor is kept alive for it."""
    return list(FpnTopdownFunction.apply(top, *laterals))


# --------------------------------------------------------------------------------------------------
# _contrib_SyncBatchNorm  (operator_cxx/contrib/sync_batch_norm-inl.h)
# --------------------------------------------------------------------------------------------------
def sync_bn_workspace_bytes(N, C, HxW):
    return _query("sd_sync_bn_workspace_bytes", int(N), int(C), int(HxW))


def _sbn_dims(x, name="data"):
    if not isinstance(x, torch.Tensor) or x.dtype not in _SBA_DTYPES:
        raise TypeError("%s must be a float32 or float16 torch.Tensor" % name)
    if x.dim() < 2:
        raise ValueError("%s should be (batch, channel, ...), got shape %s" % (name, tuple(x.shape)))
    _chk(x, name, dtype=x.dtype)
    N, C = int(x.shape[0]), int(x.shape[1])
    return N, C, (x.numel() // (N * C) if N * C else 0)


def _sbn_parts(t, name, C):
    _chk(t, name, ndim=3)
    if t.shape[0] < 1 or tuple(t.shape[1:]) != (2, C):
        raise ValueError("%s must have shape (W, 2, %d) with W >= 1, got %s" % (name, C, tuple(t.shape)))
    return int(t.shape[0])


def sync_bn_stats(x, part=None, workspace=None):
    """sd_sync_bn_stats: x (N,C,...) -> part (2,C) float32 = the rank's per-channel mean and biased variance about
    that mean."""
    N, C, HxW = _sbn_dims(x)
    part = _out(part, "part", (2, C), x.device)
    ws = _ws(x.device, workspace, "sd_sync_bn_workspace_bytes", N, C, HxW)
    _call(_fn("sd_sync_bn_stats", x), x, part, N, C, HxW, ws, ws.numel())
    return part


def sync_bn_apply(x, parts, gamma, beta, eps=1e-3, fix_gamma=True, y=None, mean=None, var=None, workspace=None):
    """sd_sync_bn_apply: parts (W,2,C), the ranks' statistics in rank order -> y, mean (C), var (C)."""
    N, C, HxW = _sbn_dims(x)
    W = _sbn_parts(parts, "parts", C)
    _chk(gamma, "gamma", shape=(C,))
    _chk(beta, "beta", shape=(C,))
    y = _out(y, "y", x.shape, x.device, x.dtype)
    mean = _out(mean, "mean", (C,), x.device)
    var = _out(var, "var", (C,), x.device)
    ws = _ws(x.device, workspace, "sd_sync_bn_workspace_bytes", N, C, HxW)
    _call(_fn("sd_sync_bn_apply", x), x, parts, W, gamma, beta, y, mean, var, N, C, HxW, eps, bool(fix_gamma), ws,
          ws.numel())
    return y, mean, var


def sync_bn_infer_forward(x, gamma, beta, moving_mean, moving_var, eps=1e-3, fix_gamma=True, y=None):
    """sd_sync_bn_infer_fwd: the scale-shift of the moving statistics (sync_batch_norm-inl.h:359-363)."""
    N, C, HxW = _sbn_dims(x)
    for t, name in ((gamma, "gamma"), (beta, "beta"), (moving_mean, "moving_mean"), (moving_var, "moving_var")):
        _chk(t, name, shape=(C,))
    y = _out(y, "y", x.shape, x.device, x.dtype)
    _call(_fn("sd_sync_bn_infer_fwd", x), x, gamma, beta, moving_mean, moving_var, y, N, C, HxW, eps,
          bool(fix_gamma))
    return y


def sync_bn_bwd_stats(dy, x, mean, bpart=None, workspace=None):
    """sd_sync_bn_bwd_stats: -> bpart (2,C) float32 = sum dy and sum dy * (x - mean) over the rank's elements."""
    N, C, HxW = _sbn_dims(x)
    _chk(dy, "dy", x.dtype, shape=x.shape)
    _chk(mean, "mean", shape=(C,))
    bpart = _out(bpart, "bpart", (2, C), x.device)
    ws = _ws(x.device, workspace, "sd_sync_bn_workspace_bytes", N, C, HxW)
    _call(_fn("sd_sync_bn_bwd_stats", x), dy, x, mean, bpart, N, C, HxW, ws, ws.numel())
    return bpart


def sync_bn_bwd_apply(dy, x, mean, var, gamma, bparts, rank=0, eps=1e-3, fix_gamma=True, dx=None, dgamma=None,
                      dbeta=None, param_grads=True, moving_mean=None, moving_var=None, momentum=0.9,
                      workspace=None):
    """sd_sync_bn_bwd_apply: bparts (W,2,C) in rank order -> dx, dgamma, dbeta (this rank's, written not
    accumulated; None with param_grads=False).  moving_mean / moving_var, when given, are updated in place."""
    N, C, HxW = _sbn_dims(x)
    _chk(dy, "dy", x.dtype, shape=x.shape)
    W = _sbn_parts(bparts, "bparts", C)
    if not 0 <= int(rank) < W:
        raise ValueError("rank %d is outside 0..%d" % (rank, W - 1))
    for t, name in ((mean, "mean"), (var, "var"), (gamma, "gamma")):
        _chk(t, name, shape=(C,))
    dx = _out(dx, "dx", x.shape, x.device, x.dtype)
    if param_grads:
        dgamma = _out(dgamma, "dgamma", (C,), x.device)
        dbeta = _out(dbeta, "dbeta", (C,), x.device)
        if N * HxW == 0:   # sums over nothing (the entry point writes nothing on an empty problem)
            dgamma.zero_()
            dbeta.zero_()
    elif dgamma is not None or dbeta is not None:
        raise ValueError("param_grads=False takes no dgamma / dbeta")
    if (moving_mean is None) != (moving_var is None):
        raise ValueError("moving_mean and moving_var go together")
    if moving_mean is not None:
        _chk(moving_mean, "moving_mean", shape=(C,))
        _chk(moving_var, "moving_var", shape=(C,))
    ws = _ws(x.device, workspace, "sd_sync_bn_workspace_bytes", N, C, HxW)
    _call(_fn("sd_sync_bn_bwd_apply", x), dy, x, mean, var, gamma, bparts, W, int(rank), dx, dgamma, dbeta,
          moving_mean, moving_var, momentum, N, C, HxW, eps, bool(fix_gamma), ws, ws.numel())
    return dx, dgamma, dbeta


def _sbn_gather(gather, part):
    """gather(part) -> (parts (W,2,C) in rank order, rank); None: one rank, no collective"""
    if gather is None:
        return part[None], 0
    parts, rank = gather(part)
    return parts.contiguous(), int(rank)


def sync_batch_norm_forward(x, gamma, beta, *, eps=1e-3, fix_gamma=True, gather=None, workspace=None):
    """mx.sym.contrib.SyncBatchNorm training forward -> (y, mean, var): the statistics, the exchange
    (gather: part -> (parts, rank), e.g. simpledet_amd.dist.all_gather_stats), the element rule.  With
    gather=None the two launches follow back to back and can be captured in a graph."""
    part = sync_bn_stats(x, workspace=workspace)
    parts, _ = _sbn_gather(gather, part)
    return sync_bn_apply(x, parts, gamma, beta, eps, fix_gamma, workspace=workspace)


def sync_batch_norm_backward(dy, x, mean, var, gamma, *, eps=1e-3, fix_gamma=True, gather=None, param_grads=True,
                             moving_mean=None, moving_var=None, momentum=0.9, workspace=None):
    """mx.sym.contrib.SyncBatchNorm training backward -> (dx, dgamma, dbeta); dgamma / dbeta are this rank's
    share.  moving_mean / moving_var are updated here, as in the reference (sync_batch_norm-inl.h:471-472)."""
    bpart = sync_bn_bwd_stats(dy, x, mean, workspace=workspace)
    bparts, rank = _sbn_gather(gather, bpart)
    return sync_bn_bwd_apply(dy, x, mean, var, gamma, bparts, rank, eps, fix_gamma, param_grads=param_grads,
                             moving_mean=moving_mean, moving_var=moving_var, momentum=momentum, workspace=workspace)


class SyncBatchNormFunction(torch.autograd.Function):
    """y, mean, var = SyncBatchNormFunction.apply(x, gamma, beta, eps, fix_gamma, gather, moving_mean, moving_var,
    momentum); mean and var carry no gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, fix_gamma, gather, moving_mean, moving_var, momentum):
        y, mean, var = sync_batch_norm_forward(x, gamma, beta, eps=eps, fix_gamma=fix_gamma, gather=gather)
        ctx.save_for_backward(x, gamma, mean, var)
        ctx.conf = (float(eps), bool(fix_gamma), gather, moving_mean, moving_var, float(momentum))
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, _dmean, _dvar):
        x, gamma, mean, var = ctx.saved_tensors
        eps, fix_gamma, gather, mm, mv, momentum = ctx.conf
        need = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        dx, dgamma, dbeta = sync_batch_norm_backward(dy.contiguous(), x, mean, var, gamma, eps=eps,
                                                     fix_gamma=fix_gamma, gather=gather, param_grads=need,
                                                     moving_mean=mm, moving_var=mv, momentum=momentum)
        return (dx if ctx.needs_input_grad[0] else None, dgamma if ctx.needs_input_grad[1] else None,
                dbeta if ctx.needs_input_grad[2] else None, None, None, None, None, None, None)


def sync_batch_norm(x, gamma, beta, eps=1e-3, fix_gamma=True, gather=None, moving_mean=None, moving_var=None,
                    momentum=0.9, return_stats=False):
    """mx.sym.contrib.SyncBatchNorm(data, gamma, beta, eps=1e-3, momentum=0.9, fix_gamma=True) in training, with
    autograd: y, or (y, mean, var) with return_stats=True (output_mean_var).  moving_mean / moving_var, when given,
    move in the backward."""
    y, mean, var = SyncBatchNormFunction.apply(x, gamma, beta, float(eps), bool(fix_gamma), gather, moving_mean,
                                               moving_var, float(momentum))
    return (y, mean, var) if return_stats else y


# --------------------------------------------------------------------------------------------------
# _contrib_SigmoidCrossEntropy and the fused Mask R-CNN mask loss  (operator_cxx/contrib/
# sigmoid_cross_entropy{-inl.h,.cu}; models/maskrcnn/builder.py:278-313)
# --------------------------------------------------------------------------------------------------
def sigmoid_cross_entropy_workspace_bytes(n, k):
    return _query("sd_sigmoid_ce_workspace_bytes", int(n), int(k))


def mask_loss_workspace_bytes(R, K, P):
    return _query("sd_mask_loss_workspace_bytes", int(R), int(K), int(P))


def _ce_rows(data, label):
    """(n, k) of the operator: n = shape[0], k = everything else (sigmoid_cross_entropy-inl.h:80-84)"""
    _chk(data, "data")
    _chk(label, "label")
    if data.dim() < 1 or label.numel() != data.numel():
        raise ValueError("data %s and label %s must hold (n, k) rows of the same size"
                         % (tuple(data.shape), tuple(label.shape)))
    n = int(data.shape[0])
    return n, (data.numel() // n if n else 0)


def sigmoid_cross_entropy_forward(data, label, *, full=False, out=None, loss=None, loss_sum=None, count=None,
                                  count_sum=None, workspace=None):
    """SigmoidCrossEntropy forward (sigmoid_cross_entropy.cu:44-104): data / label (n, ...) rows -> out, loss_sum,
    count_sum (n,); with full=True (or loss / count passed in) also the operator's hidden full-size outputs
    loss and count, returned as (out, loss, loss_sum, count, count_sum) in the operator's order.  A label of -1
    ignores its element whatever the logit is.  out is NOT scaled by grad_scale (only the gradient is)."""
    n, k = _ce_rows(data, label)
    dev = data.device
    out = _out(out, "out", (n,), dev, flat=True)
    loss_sum = _out(loss_sum, "loss_sum", (n,), dev, flat=True)
    count_sum = _out(count_sum, "count_sum", (n,), dev, flat=True)
    if full or loss is not None or count is not None:
        loss = _out(loss, "loss", data.shape, dev, flat=True)
        count = _out(count, "count", data.shape, dev, flat=True)
    if n * k == 0:        # rows of nothing: an empty sum over an empty count (the entry point writes nothing)
        out.zero_()
        loss_sum.zero_()
        count_sum.fill_(1e-5)
        return (out, loss, loss_sum, count, count_sum) if loss is not None else (out, loss_sum, count_sum)
    ws = _ws(dev, workspace, "sd_sigmoid_ce_workspace_bytes", n, k)
    _call("sd_sigmoid_ce_fwd", data, label, out, loss, loss_sum, count, count_sum, n, k, ws, ws.numel())
    if loss is not None:
        return out, loss, loss_sum, count, count_sum
    return out, loss_sum, count_sum


def sigmoid_cross_entropy_backward(data, label, grad_scale=1.0, *, d_data=None, count=None, count_sum=None,
                                   workspace=None):
    """SigmoidCrossEntropy backward (sigmoid_cross_entropy.cu:66-122): d = ((sigmoid(x) - t) / count_sum) *
    grad_scale, 0 where the label is -1; the count is recomputed, as the reference does.  The head gradient has
    no part in it.  Returns (d_data, count_sum); `count` (full size) is written only when passed in."""
    n, k = _ce_rows(data, label)
    dev = data.device
    d_data = _out(d_data, "d_data", data.shape, dev, flat=True)
    count_sum = _out(count_sum, "count_sum", (n,), dev, flat=True)
    if count is not None:
        count = _chk(count, "count", numel=n * k)
    if n * k == 0:
        count_sum.fill_(1e-5)
        return d_data, count_sum
    ws = _ws(dev, workspace, "sd_sigmoid_ce_workspace_bytes", n, k)
    _call("sd_sigmoid_ce_bwd", data, label, d_data, count, count_sum, n, k, grad_scale, ws, ws.numel())
    return d_data, count_sum


def _mask_dims(logits, cls, target):
    _chk(logits, "logits")
    _chk(cls, "cls")
    _chk(target, "target")
    if logits.dim() < 2:
        raise ValueError("logits should be (roi, class, ...), got shape %s" % (tuple(logits.shape),))
    R, K = int(logits.shape[0]), int(logits.shape[1])
    P = logits.numel() // (R * K) if R * K else 0
    if cls.numel() != R or target.numel() != R * P:
        raise ValueError("cls must hold %d floats and target %d, got %d and %d" % (R, R * P, cls.numel(),
                                                                                   target.numel()))
    return R, K, P


def mask_loss_forward(logits, cls, target, *, out=None, count_sum=None, workspace=None):
    """The mask loss of MaskFasterRcnnHead.get_loss (models/maskrcnn/builder.py:278-313) in one op: logits
    (R, K, h, w), cls (R,) float -- the builder's mask_label --, target (R, h, w).  Plane int(cls[r]) of every RoI
    goes through SigmoidCrossEntropy as ONE row of R*h*w elements; bit-equal to sigmoid_cross_entropy_forward on
    the gathered row.  A cls that is NaN, negative or >= K ignores its RoI.  Returns (out, count_sum), (1,) each."""
    R, K, P = _mask_dims(logits, cls, target)
    dev = logits.device
    out = _out(out, "out", (1,), dev, flat=True)
    count_sum = _out(count_sum, "count_sum", (1,), dev, flat=True)
    if R * K * P == 0:    # an empty sum over an empty count (the entry point writes nothing)
        out.zero_()
        count_sum.fill_(1e-5)
        return out, count_sum
    ws = _ws(dev, workspace, "sd_mask_loss_workspace_bytes", R, K, P)
    _call("sd_mask_loss_fwd", logits, cls, target, out, count_sum, R, K, P, ws, ws.numel())
    return out, count_sum


def mask_loss_backward(logits, cls, target, grad_scale=1.0, *, d_logits=None, workspace=None):
    """Backward of mask_loss_forward: ALL of d_logits (the shape of logits) is written once -- +0.0 in the planes
    that are not selected and in ignored RoIs, the SigmoidCrossEntropy gradient in plane int(cls[r])."""
    R, K, P = _mask_dims(logits, cls, target)
    d_logits = _out(d_logits, "d_logits", logits.shape, logits.device, flat=True)
    ws = _ws(logits.device, workspace, "sd_mask_loss_workspace_bytes", R, K, P)
    _call("sd_mask_loss_bwd", logits, cls, target, d_logits, R, K, P, grad_scale, ws, ws.numel())
    return d_logits


# --------------------------------------------------------------------------------------------------
# The Mask Scoring R-CNN training head  (models/msrcnn/builder.py:143-168, :383-424; models/msrcnn/maskiou_compute.py)
# --------------------------------------------------------------------------------------------------
def msrcnn_mask_loss_workspace_bytes(R, K, P):
    return _query("sd_msrcnn_mask_loss_workspace_bytes", int(R), int(K), int(P))


def maskiou_loss_workspace_bytes(R, K, P):
    return _query("sd_maskiou_loss_workspace_bytes", int(R), int(K), int(P))


def msrcnn_mask_loss_forward(logits, cls, target, *, out=None, count_sum=None, prob=None, workspace=None):
    """The mask loss of Mask Scoring R-CNN's MaskFasterRcnnHead.get_loss (models/msrcnn/builder.py:383-424) in one
    op: mask_loss_forward's (out, count_sum), bit for bit, and prob (R, h, w) = sigmoid of plane int(cls[r]) of every
    RoI -- the builder's mask_pred_prob, written for every pixel of a valid RoI (target -1 included) and +0.0 for a
    RoI whose cls is NaN, negative or >= K.  Returns (out, count_sum, prob)."""
    R, K, P = _mask_dims(logits, cls, target)
    dev = logits.device
    out = _out(out, "out", (1,), dev, flat=True)
    count_sum = _out(count_sum, "count_sum", (1,), dev, flat=True)
    prob = _out(prob, "prob", (R,) + tuple(logits.shape[2:]), dev, flat=True)
    if R * K * P == 0:    # an empty sum over an empty count (the entry point writes nothing)
        out.zero_()
        count_sum.fill_(1e-5)
        prob.zero_()
        return out, count_sum, prob
    ws = _ws(dev, workspace, "sd_msrcnn_mask_loss_workspace_bytes", R, K, P)
    _call("sd_msrcnn_mask_loss_fwd", logits, cls, target, out, count_sum, prob, R, K, P, ws, ws.numel())
    return out, count_sum, prob


def msrcnn_mask_loss_backward(logits, cls, target, d_prob=None, grad_scale=1.0, *, d_logits=None, workspace=None):
    """Backward of msrcnn_mask_loss_forward: ALL of d_logits is written once -- +0.0 in the planes that are not
    selected, mask_loss_backward's gradient plus d_prob * p * (1 - p) in plane int(cls[r]).  d_prob (R, h, w) is the
    gradient that reached prob (None: none did; the result is then mask_loss_backward's, bit for bit)."""
    R, K, P = _mask_dims(logits, cls, target)
    if d_prob is not None:
        _chk(d_prob, "d_prob", numel=R * P)
    d_logits = _out(d_logits, "d_logits", logits.shape, logits.device, flat=True)
    ws = _ws(logits.device, workspace, "sd_msrcnn_mask_loss_workspace_bytes", R, K, P)
    _call("sd_msrcnn_mask_loss_bwd", logits, cls, target, d_prob, d_logits, R, K, P, grad_scale, ws, ws.numel())
    return d_logits


def _maskiou_dims(iou_pred, cls, prob=None, target=None, ratio=None):
    _chk(iou_pred, "iou_pred")
    _chk(cls, "cls")
    if iou_pred.dim() != 2:
        raise ValueError("iou_pred should be (roi, class), got shape %s" % (tuple(iou_pred.shape),))
    R, K = int(iou_pred.shape[0]), int(iou_pred.shape[1])
    if cls.numel() != R:
        raise ValueError("cls must hold %d floats, got %d" % (R, cls.numel()))
    if prob is None:
        return R, K, 0
    _chk(prob, "prob")
    _chk(target, "target")
    _chk(ratio, "ratio")
    P = prob.numel() // R if R else 0
    if prob.numel() != R * P or target.numel() != R * P or ratio.numel() != R:
        raise ValueError("prob and target must hold (%d, P) floats and ratio %d, got %d, %d and %d"
                         % (R, R, prob.numel(), target.numel(), ratio.numel()))
    return R, K, P


def maskiou_loss_forward(iou_pred, prob, target, ratio, cls, *, iou_target=None, weight=None, loss=None,
                         weight_sum=None, workspace=None):
    """MaskIoUConvHead.get_loss behind its conv / FC tower (models/msrcnn/builder.py:146-167) in one op: iou_pred
    (R, K), prob and target (R, h, w), ratio (R,), cls (R,) float -> (iou_target (R,), weight (R,), loss (1,),
    weight_sum (1,)).  iou_target and weight are maskiou_compute.py's outputs computed on the device (no host round
    trip); loss = 0.5 * sum((iou_target - iou_pred[r, int(cls[r])])^2 * weight) / max(sum weight, 1) over the rows
    whose cls names a column."""
    R, K, P = _maskiou_dims(iou_pred, cls, prob, target, ratio)
    dev = iou_pred.device
    iou_target = _out(iou_target, "iou_target", (R,), dev, flat=True)
    weight = _out(weight, "weight", (R,), dev, flat=True)
    loss = _out(loss, "loss", (1,), dev, flat=True)
    weight_sum = _out(weight_sum, "weight_sum", (1,), dev, flat=True)
    if R * K * P == 0:    # nothing to look at: empty sums (the entry point writes nothing)
        for t in (iou_target, weight, loss, weight_sum):
            t.zero_()
        return iou_target, weight, loss, weight_sum
    ws = _ws(dev, workspace, "sd_maskiou_loss_workspace_bytes", R, K, P)
    _call("sd_maskiou_loss_fwd", iou_pred, prob, target, ratio, cls, iou_target, weight, loss, weight_sum, R, K, P,
          ws, ws.numel())
    return iou_target, weight, loss, weight_sum


def maskiou_loss_backward(iou_pred, cls, iou_target, weight, weight_sum, grad_scale=1.0, *, d_iou_pred=None):
    """Backward of maskiou_loss_forward: d_iou_pred (R, K), written once -- -(iou_target - p) * weight /
    max(weight_sum, 1) * grad_scale in column int(cls[r]), +0.0 everywhere else.  Nothing flows to prob, target or
    ratio."""
    R, K, _ = _maskiou_dims(iou_pred, cls)
    for t, name, n in ((iou_target, "iou_target", R), (weight, "weight", R), (weight_sum, "weight_sum", 1)):
        _chk(t, name, numel=n)
    d_iou_pred = _out(d_iou_pred, "d_iou_pred", iou_pred.shape, iou_pred.device, flat=True)
    _call("sd_maskiou_loss_bwd", iou_pred, cls, iou_target, weight, weight_sum, d_iou_pred, R, K, grad_scale)
    return d_iou_pred


# --------------------------------------------------------------------------------------------------
# The CrowdHuman double-prediction head (models/crowdhuman: bbox_target.py, bbox_sec_target.py,
# softmax_entropy_op.py, builder.py:254-306)
# --------------------------------------------------------------------------------------------------
class CrowdHumanTargetParam(ctypes.Structure):
    """sd_crowdhuman_target_param"""
    _fields_ = [("num_reg_class", ctypes.c_int), ("add_gt_to_proposal", ctypes.c_int), ("image_rois", ctypes.c_int),
                ("fg_fraction", ctypes.c_double), ("fg_thresh", ctypes.c_double), ("bg_thresh_hi", ctypes.c_double),
                ("bg_thresh_lo", ctypes.c_double), ("bbox_target_std", ctypes.c_double * 4)]


CrowdHumanTargets = collections.namedtuple(
    "CrowdHumanTargets", "sampled_proposal bbox_cls bbox_target bbox_target_weight bbox_sec_cls bbox_sec_target "
                         "bbox_sec_target_weight count")


def crowdhuman_target_workspace_bytes(B, P, M):
    return _query("sd_crowdhuman_target_workspace_bytes", int(B), int(P), int(M))


def crowdhuman_target(proposal, gt_bbox, mt_state, *, num_reg_class, image_rois, fg_fraction, fg_thresh,
                      bg_thresh_hi, bg_thresh_lo, bbox_target_std, add_gt_to_proposal=True, double=True,
                      workspace=None):
    """The CustomOps `doublebbox_target` (double=True: models/crowdhuman/bbox_sec_target.py) and `bbox_target`
    (double=False: models/crowdhuman/bbox_target.py) on the device: proposal (B, P, 4) with y2 == 0 padding, gt_bbox
    (B, M, 5) with class -1 padding and -2 ignore rows -> CrowdHumanTargets(sampled_proposal (B, S, 4), bbox_cls
    (B, S), bbox_target / bbox_target_weight (B, S, 4 * num_reg_class), the three second outputs (None when not
    double), count (B,) int32 = rows filled; the rows behind are zero).  mt_state: mt19937_state(...), advanced in
    place like np.random over the two np.random.choice calls per image.  No host synchronisation."""
    _chk(proposal, "proposal", ndim=3)
    _chk(gt_bbox, "gt_bbox", ndim=3)
    _chk(mt_state, "mt_state", dtype=torch.int32, ndim=1)
    if mt_state.numel() != 625:
        raise ValueError("mt_state must hold 625 int32 words")
    B, P, _four = proposal.shape
    M = int(gt_bbox.shape[1])
    if _four != 4 or tuple(gt_bbox.shape) != (B, M, 5):
        raise ValueError("proposal must be (B, P, 4) and gt_bbox (B, M, 5), got %s and %s"
                         % (tuple(proposal.shape), tuple(gt_bbox.shape)))
    prm = CrowdHumanTargetParam()
    prm.num_reg_class, prm.add_gt_to_proposal, prm.image_rois = int(num_reg_class), int(bool(add_gt_to_proposal)), \
        int(image_rois)
    prm.fg_fraction, prm.fg_thresh = float(fg_fraction), float(fg_thresh)
    prm.bg_thresh_hi, prm.bg_thresh_lo = float(bg_thresh_hi), float(bg_thresh_lo)
    std = [float(v) for v in bbox_target_std]
    if len(std) != 4:
        raise ValueError("bbox_target_std must have 4 entries")
    for i, v in enumerate(std):
        prm.bbox_target_std[i] = v
    dev, S, W = proposal.device, int(image_rois), 4 * int(num_reg_class)
    f32 = dict(device=dev, dtype=torch.float32)
    outs = [torch.empty((B, S, 4), **f32), torch.empty((B, S), **f32), torch.empty((B, S, W), **f32),
            torch.empty((B, S, W), **f32)]
    sec = [torch.empty((B, S), **f32), torch.empty((B, S, W), **f32), torch.empty((B, S, W), **f32)] if double \
        else [None, None, None]
    count = torch.empty((B,), device=dev, dtype=torch.int32)
    ws = _ws(dev, workspace, "sd_crowdhuman_target_workspace_bytes", B, P, M)
    _call("sd_crowdhuman_target", proposal, gt_bbox, B, P, M, 1 if double else 0, ctypes.byref(prm), mt_state,
          *outs, *sec, count, ws, ws.numel())
    return CrowdHumanTargets(*(outs + sec + [count]))


def _emd_args(cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta, bbox_target,
              bbox_sec_target, bbox_weight, bbox_sec_weight):
    _chk(cls_logit, "cls_logit", ndim=2)
    R, K = int(cls_logit.shape[0]), int(cls_logit.shape[1])
    _chk(bbox_delta, "bbox_delta", ndim=2)
    D = int(bbox_delta.shape[1])
    for t, name, n in ((cls_sec_logit, "cls_sec_logit", R * K), (cls_label, "cls_label", R),
                       (cls_sec_label, "cls_sec_label", R), (bbox_delta, "bbox_delta", R * D),
                       (bbox_sec_delta, "bbox_sec_delta", R * D), (bbox_target, "bbox_target", R * D),
                       (bbox_sec_target, "bbox_sec_target", R * D), (bbox_weight, "bbox_weight", R * D),
                       (bbox_sec_weight, "bbox_sec_weight", R * D)):
        _chk(t, name, numel=n)
    return R, K, D


def emd_loss_forward(cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta, bbox_target,
                     bbox_sec_target, bbox_weight, bbox_sec_weight, smooth_l1_scalar=1.0, *, loss=None, pairing=None,
                     return_pairing=False):
    """DoublePredBboxHead.emd_loss (models/crowdhuman/builder.py:254-306) in one launch: logits (R, K), labels (R,),
    deltas / targets / weights (R, 4 K') -> loss (1,) = mean over the rows of min(L1, L2), the sums of the two ways
    to pair the heads with the labels.  return_pairing: also pairing (R,) int32, 1 where L1 <= L2, else 2."""
    ts = (cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta, bbox_target,
          bbox_sec_target, bbox_weight, bbox_sec_weight)
    R, K, D = _emd_args(*ts)
    dev = cls_logit.device
    loss = _out(loss, "loss", (1,), dev, flat=True)
    if return_pairing or pairing is not None:
        if pairing is None:
            pairing = torch.empty((R,), device=dev, dtype=torch.int32)
        _chk(pairing, "pairing", dtype=torch.int32, numel=R)
    if R == 0:
        loss.zero_()
    _call("sd_emd_loss_fwd", *ts, R, K, D, smooth_l1_scalar, loss, pairing)
    return (loss, pairing) if return_pairing else loss


def emd_loss_backward(cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta, bbox_target,
                      bbox_sec_target, bbox_weight, bbox_sec_weight, smooth_l1_scalar=1.0, grad_scale=1.0, *,
                      d_cls_logit=None, d_cls_sec_logit=None, d_bbox_delta=None, d_bbox_sec_delta=None):
    """The four gradients of emd_loss_forward, written once: (d_cls_logit, d_cls_sec_logit, d_bbox_delta,
    d_bbox_sec_delta); only the winning pairing of a row contributes, scaled by grad_scale / R."""
    ts = (cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta, bbox_target,
          bbox_sec_target, bbox_weight, bbox_sec_weight)
    R, K, D = _emd_args(*ts)
    dev = cls_logit.device
    d_cls_logit = _out(d_cls_logit, "d_cls_logit", (R, K), dev, flat=True)
    d_cls_sec_logit = _out(d_cls_sec_logit, "d_cls_sec_logit", (R, K), dev, flat=True)
    d_bbox_delta = _out(d_bbox_delta, "d_bbox_delta", (R, D), dev, flat=True)
    d_bbox_sec_delta = _out(d_bbox_sec_delta, "d_bbox_sec_delta", (R, D), dev, flat=True)
    _call("sd_emd_loss_bwd", *ts, R, K, D, smooth_l1_scalar, grad_scale, d_cls_logit, d_cls_sec_logit, d_bbox_delta,
          d_bbox_sec_delta)
    return d_cls_logit, d_cls_sec_logit, d_bbox_delta, d_bbox_sec_delta


class EmdLossFunction(torch.autograd.Function):
    """loss = EmdLossFunction.apply(cls_logit, cls_sec_logit, bbox_delta, bbox_sec_delta, cls_label, cls_sec_label,
    bbox_target, bbox_sec_target, bbox_weight, bbox_sec_weight, smooth_l1_scalar, grad_scale).  Like the reference's
    MakeLoss node the backward does not look at the incoming gradient."""

    @staticmethod
    def forward(ctx, cls_logit, cls_sec_logit, bbox_delta, bbox_sec_delta, cls_label, cls_sec_label, bbox_target,
                bbox_sec_target, bbox_weight, bbox_sec_weight, smooth_l1_scalar, grad_scale):
        ts = [t.contiguous() for t in (cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta,
                                       bbox_target, bbox_sec_target, bbox_weight, bbox_sec_weight)]
        ctx.save_for_backward(*ts)
        ctx.scalar, ctx.grad_scale = float(smooth_l1_scalar), float(grad_scale)
        return emd_loss_forward(*ts, ctx.scalar)

    @staticmethod
    def backward(ctx, _out_grad):
        g1, g2, gd1, gd2 = emd_loss_backward(*ctx.saved_tensors, ctx.scalar, ctx.grad_scale)
        return (g1, g2, gd1, gd2) + (None,) * 8


def emd_loss(cls_logit, cls_sec_logit, cls_label, cls_sec_label, bbox_delta, bbox_sec_delta, bbox_target,
             bbox_sec_target, bbox_weight, bbox_sec_weight, smooth_l1_scalar=1.0, grad_scale=1.0):
    """emd_loss_forward with autograd to the two logits and the two deltas (the argument order of the forward)."""
    return EmdLossFunction.apply(cls_logit, cls_sec_logit, bbox_delta, bbox_sec_delta, cls_label, cls_sec_label,
                                 bbox_target, bbox_sec_target, bbox_weight, bbox_sec_weight, smooth_l1_scalar,
                                 grad_scale)


# --------------------------------------------------------------------------------------------------
# The Faster / Mask R-CNN loss heads  (symbol/builder.py RpnHead / BboxHead .get_loss, models/FPN/builder.py
# FPNRpnHead.get_loss; core/detection_metric.py AccWithIgnore / L1)
# --------------------------------------------------------------------------------------------------
RpnLossOut = collections.namedtuple("RpnLossOut", "prob reg_loss state")


def rpn_loss_workspace_bytes(N, A, HW):
    return _query("sd_rpn_loss_workspace_bytes", int(N), int(A), int(HW))


def rcnn_loss_workspace_bytes(R):
    return _query("sd_rcnn_loss_workspace_bytes", int(R))


def loss_state(device=None):
    """A zeroed state block of the loss heads: int32[4] = {valid, correct, fg, the bits of the float reg_sum}."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    return torch.zeros(4, device=device, dtype=torch.int32)


def _loss_metrics(state):
    _chk(state, "state", dtype=torch.int32)
    if state.numel() < 4:
        raise ValueError("state must hold 4 int32 words")
    s = state.reshape(-1)
    return s[1:2], s[0:1], s[3:4].view(torch.float32), s[2:3]


def rpn_loss_metrics(state):
    """(acc numerator, acc denominator, L1 numerator, L1 denominator) of the config's RpnAcc / RpnL1 metrics
    (AccWithIgnore and L1, core/detection_metric.py:40-66,134-156) as one-element device views of the state block:
    correct, valid (int32), reg_sum (float32), fg (int32).  Nothing is copied and no big tensor is touched."""
    return _loss_metrics(state)


def rcnn_loss_metrics(state):
    """The same four numbers for RcnnAcc / RcnnL1; they are the reference's as long as no label is -1 (the metric
    drops such rows, normalization='batch' counts them: valid = R)."""
    return _loss_metrics(state)


def _loss_opts(normalization, want, smooth_alpha, out_grad):
    if normalization != want:
        raise NotImplementedError("normalization=%r is not built (this head is %r)" % (normalization, want))
    if smooth_alpha:
        raise NotImplementedError("smooth_alpha is not built")
    if out_grad:
        raise NotImplementedError("out_grad is not built")


def _rpn_loss_levels(cls_logits, bbox_deltas, cls_label, reg_target, reg_weight):
    """(N, A, HW, hw table) of the level lists; either list may be None (that half is left out)"""
    lead = cls_logits if cls_logits is not None else bbox_deltas
    if lead is None or len(lead) == 0:
        raise ValueError("cls_logits or bbox_deltas must hold one tensor per level")
    L = len(lead)
    if L > 8 or (cls_logits is not None and bbox_deltas is not None and len(cls_logits) != len(bbox_deltas)):
        raise ValueError("cls_logits and bbox_deltas need one tensor per level each, 8 levels at the most")
    per = 2 if cls_logits is not None else 4
    _chk(lead[0], "level 0")
    if lead[0].dim() < 3 or int(lead[0].shape[1]) % per:
        raise ValueError("level tensors should be (N, %dA, H, W), got %s" % (per, tuple(lead[0].shape)))
    N, A = int(lead[0].shape[0]), int(lead[0].shape[1]) // per
    hws = []
    for i in range(L):
        hw = lead[i].numel() // (N * per * A) if N * A else 0
        for lst, c, name in ((cls_logits, 2 * A, "cls_logits"), (bbox_deltas, 4 * A, "bbox_deltas")):
            if lst is None:
                continue
            _chk(lst[i], "%s[%d]" % (name, i))
            if lst[i].dim() < 3 or int(lst[i].shape[0]) != N or int(lst[i].shape[1]) != c or lst[i].numel() != N * c * hw:
                raise ValueError("%s[%d] should be (%d, %d, H, W) with H * W = %d, got %s"
                                 % (name, i, N, c, hw, tuple(lst[i].shape)))
        hws.append(hw)
    HW = sum(hws)
    if cls_logits is not None:
        _chk(cls_label, "cls_label", numel=N * A * HW)
    if bbox_deltas is not None:
        _chk(reg_target, "reg_target", numel=N * 4 * A * HW)
        _chk(reg_weight, "reg_weight", numel=N * 4 * A * HW)
    return N, A, HW, (ctypes.c_long * L)(*hws)


def rpn_loss_forward(cls_logits, bbox_deltas, cls_label, reg_target, reg_weight, *, ignore_label=-1.0, sigma=3.0,
                     normalization="valid", smooth_alpha=0.0, out_grad=False, want_prob=True, want_reg_loss=True,
                     prob=None, reg_loss=None, state=None, workspace=None):
    """The RPN losses of RpnHead / FPNRpnHead.get_loss over per-level tensors, no reshape and no concat:
    cls_logits[l] (N, 2A, H_l, W_l), bbox_deltas[l] (N, 4A, H_l, W_l), cls_label (N, A * HW), reg_target /
    reg_weight (N, 4A, HW) -- rpn_anchor_target(layout=1)'s outputs.  Returns RpnLossOut: prob (N, 2, A, HW) =
    SoftmaxOutput's output, reg_loss (N, 4A, HW) = weight * smooth_l1(delta - target, sigma), and the state block
    (rpn_loss_metrics).  A list that is None leaves its half out; want_prob / want_reg_loss = False skips the store
    of the big tensor but keeps the state."""
    _loss_opts(normalization, "valid", smooth_alpha, out_grad)
    N, A, HW, hws = _rpn_loss_levels(cls_logits, bbox_deltas, cls_label, reg_target, reg_weight)
    lead = cls_logits if cls_logits is not None else bbox_deltas
    dev = lead[0].device
    if cls_logits is not None and (want_prob or prob is not None):
        prob = _out(prob, "prob", (N, 2, A, HW), dev, flat=True)
    else:
        prob = None
    if bbox_deltas is not None and (want_reg_loss or reg_loss is not None):
        reg_loss = _out(reg_loss, "reg_loss", (N, 4 * A, HW), dev, flat=True)
    else:
        reg_loss = None
    state = _out(state, "state", (4,), dev, torch.int32, flat=True)
    if N * A * HW == 0:
        state.zero_()
        return RpnLossOut(prob, reg_loss, state)
    ws = _ws(dev, workspace, "sd_rpn_loss_workspace_bytes", N, A, HW)
    _call("sd_rpn_loss_fwd", None if cls_logits is None else _parr(cls_logits),
          None if bbox_deltas is None else _parr(bbox_deltas), hws, len(lead), cls_label, reg_target, reg_weight, N, A,
          ignore_label, sigma, prob, reg_loss, state, ws, ws.numel())
    return RpnLossOut(prob, reg_loss, state)


def _grad_levels(given, like, name):
    if given is None:
        given = [torch.empty_like(t) for t in like]
    if len(given) != len(like):
        raise ValueError("%s needs one tensor per level" % name)
    for g, t in zip(given, like):
        _chk(g, name)
        if g.numel() != t.numel():
            raise ValueError("%s must have the sizes of the inputs" % name)
    return list(given)


def rpn_loss_backward(cls_logits, bbox_deltas, cls_label, reg_target, reg_weight, state, *, cls_grad_scale=1.0,
                      reg_grad_scale=1.0, ignore_label=-1.0, sigma=3.0, normalization="valid", smooth_alpha=0.0,
                      out_grad=False, d_cls=None, d_delta=None):
    """The gradients of rpn_loss_forward in ONE launch, written into per-level tensors of the inputs' shapes:
    (d_cls list, d_delta list); the list of a half that is None is None.  The class gradient is
    (p - onehot) * cls_grad_scale / max(1, state valid), zeros where the label is ignore_label; the box gradient
    smooth_l1'(delta - target) * (weight * reg_grad_scale).  No top gradient enters."""
    _loss_opts(normalization, "valid", smooth_alpha, out_grad)
    N, A, HW, hws = _rpn_loss_levels(cls_logits, bbox_deltas, cls_label, reg_target, reg_weight)
    d_cls = None if cls_logits is None else _grad_levels(d_cls, cls_logits, "d_cls")
    d_delta = None if bbox_deltas is None else _grad_levels(d_delta, bbox_deltas, "d_delta")
    if N * A * HW == 0:
        return d_cls, d_delta
    if cls_logits is not None:
        _chk(state, "state", dtype=torch.int32)
    lead = cls_logits if cls_logits is not None else bbox_deltas
    _call("sd_rpn_loss_bwd", None if cls_logits is None else _parr(cls_logits),
          None if bbox_deltas is None else _parr(bbox_deltas), hws, len(lead), cls_label, reg_target, reg_weight, N, A,
          ignore_label, sigma, cls_grad_scale, reg_grad_scale, state, None if d_cls is None else _parr(d_cls),
          None if d_delta is None else _parr(d_delta))
    return d_cls, d_delta


class RpnLossFunction(torch.autograd.Function):
    """prob, reg_loss, state = RpnLossFunction.apply(cls_label, reg_target, reg_weight, cls_grad_scale,
    reg_grad_scale, ignore_label, sigma, L, *cls_logits, *bbox_deltas).  Like the reference's SoftmaxOutput and
    MakeLoss nodes the backward does not look at the incoming gradients."""

    @staticmethod
    def forward(ctx, cls_label, reg_target, reg_weight, cls_grad_scale, reg_grad_scale, ignore_label, sigma, L,
                *levels):
        if len(levels) != 2 * L:
            raise ValueError("expected %d level tensors, got %d" % (2 * L, len(levels)))
        levels = [t.contiguous() for t in levels]
        fixed = [t.contiguous() for t in (cls_label, reg_target, reg_weight)]
        ctx.kw = dict(ignore_label=ignore_label, sigma=sigma)
        ctx.gs, ctx.L = (cls_grad_scale, reg_grad_scale), L
        out = rpn_loss_forward(levels[:L], levels[L:], *fixed, **ctx.kw)
        ctx.save_for_backward(out.state, *fixed, *levels)
        ctx.mark_non_differentiable(out.state)
        return out.prob, out.reg_loss, out.state

    @staticmethod
    def backward(ctx, _dprob, _dreg, _dstate):
        state, label, target, weight = ctx.saved_tensors[:4]
        levels, L = list(ctx.saved_tensors[4:]), ctx.L
        d_cls, d_delta = rpn_loss_backward(levels[:L], levels[L:], label, target, weight, state,
                                           cls_grad_scale=ctx.gs[0], reg_grad_scale=ctx.gs[1], **ctx.kw)
        return (None,) * 8 + tuple(d_cls) + tuple(d_delta)


def rpn_loss(cls_logits, bbox_deltas, cls_label, reg_target, reg_weight, *, cls_grad_scale=1.0, reg_grad_scale=1.0,
             ignore_label=-1.0, sigma=3.0):
    """rpn_loss_forward with autograd over the two lists of level tensors: RpnLossOut(prob, reg_loss, state).
    reg_grad_scale is the head's 1 / (batch_image * image_anchor); both scales carry fp16's 128."""
    L = len(cls_logits)
    return RpnLossOut(*RpnLossFunction.apply(cls_label, reg_target, reg_weight, float(cls_grad_scale),
                                             float(reg_grad_scale), float(ignore_label), float(sigma), L,
                                             *cls_logits, *bbox_deltas))


def _rcnn_loss_args(cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight):
    R = K = D = None
    if cls_logit is not None:
        _chk(cls_logit, "cls_logit", ndim=2)
        R, K = int(cls_logit.shape[0]), int(cls_logit.shape[1])
        _chk(cls_label, "cls_label", numel=R)
    if bbox_delta is not None:
        _chk(bbox_delta, "bbox_delta", ndim=2)
        if R is not None and int(bbox_delta.shape[0]) != R:
            raise ValueError("bbox_delta should have %d rows, got %d" % (R, int(bbox_delta.shape[0])))
        R, D = int(bbox_delta.shape[0]), int(bbox_delta.shape[1])
        _chk(bbox_target, "bbox_target", numel=R * D)
        _chk(bbox_weight, "bbox_weight", numel=R * D)
    if R is None:
        raise ValueError("cls_logit or bbox_delta must be given")
    return R, K if K is not None else 1, D if D is not None else 0


def rcnn_loss_forward(cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight, *, smooth_l1_scalar=1.0,
                      normalization="batch", smooth_alpha=0.0, out_grad=False, want_prob=True, want_reg_loss=True,
                      prob=None, reg_loss=None, state=None, workspace=None):
    """The R-CNN losses of BboxHead.get_loss: cls_logit (R, K), cls_label (R,), bbox_delta / bbox_target /
    bbox_weight (R, D) -> RpnLossOut(prob (R, K), reg_loss (R, D), state).  cls_logit or bbox_delta may be None
    (that half is left out)."""
    _loss_opts(normalization, "batch", smooth_alpha, out_grad)
    R, K, D = _rcnn_loss_args(cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight)
    dev = (cls_logit if cls_logit is not None else bbox_delta).device
    if cls_logit is not None and (want_prob or prob is not None):
        prob = _out(prob, "prob", (R, K), dev, flat=True)
    else:
        prob = None
    if bbox_delta is not None and (want_reg_loss or reg_loss is not None):
        reg_loss = _out(reg_loss, "reg_loss", (R, D), dev, flat=True)
    else:
        reg_loss = None
    state = _out(state, "state", (4,), dev, torch.int32, flat=True)
    if R == 0:
        state.zero_()
        return RpnLossOut(prob, reg_loss, state)
    ws = _ws(dev, workspace, "sd_rcnn_loss_workspace_bytes", R)
    _call("sd_rcnn_loss_fwd", cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight, R, K, D, smooth_l1_scalar,
          prob, reg_loss, state, ws, ws.numel())
    return RpnLossOut(prob, reg_loss, state)


def rcnn_loss_backward(cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight, state, *, cls_grad_scale=1.0,
                       reg_grad_scale=1.0, smooth_l1_scalar=1.0, normalization="batch", smooth_alpha=0.0,
                       out_grad=False, d_cls_logit=None, d_bbox_delta=None):
    """The gradients of rcnn_loss_forward in one launch: (d_cls_logit, d_bbox_delta), None for a half that is None.
    (p - onehot) * cls_grad_scale / R and smooth_l1'(delta - target) * (weight * reg_grad_scale)."""
    _loss_opts(normalization, "batch", smooth_alpha, out_grad)
    R, K, D = _rcnn_loss_args(cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight)
    dev = (cls_logit if cls_logit is not None else bbox_delta).device
    if cls_logit is not None:
        d_cls_logit = _out(d_cls_logit, "d_cls_logit", (R, K), dev, flat=True)
        _chk(state, "state", dtype=torch.int32)
    else:
        d_cls_logit = None
    d_bbox_delta = None if bbox_delta is None else _out(d_bbox_delta, "d_bbox_delta", (R, D), dev, flat=True)
    if R == 0:
        return d_cls_logit, d_bbox_delta
    _call("sd_rcnn_loss_bwd", cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight, R, K, D, smooth_l1_scalar,
          cls_grad_scale, reg_grad_scale, state, d_cls_logit, d_bbox_delta if D else None)
    return d_cls_logit, d_bbox_delta


class RcnnLossFunction(torch.autograd.Function):
    """prob, reg_loss, state = RcnnLossFunction.apply(cls_logit, bbox_delta, cls_label, bbox_target, bbox_weight,
    cls_grad_scale, reg_grad_scale, smooth_l1_scalar); the backward does not look at the incoming gradients."""

    @staticmethod
    def forward(ctx, cls_logit, bbox_delta, cls_label, bbox_target, bbox_weight, cls_grad_scale, reg_grad_scale,
                smooth_l1_scalar):
        ts = [t.contiguous() for t in (cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight)]
        ctx.gs, ctx.scalar = (float(cls_grad_scale), float(reg_grad_scale)), float(smooth_l1_scalar)
        out = rcnn_loss_forward(*ts, smooth_l1_scalar=ctx.scalar)
        ctx.save_for_backward(out.state, *ts)
        ctx.mark_non_differentiable(out.state)
        return out.prob, out.reg_loss, out.state

    @staticmethod
    def backward(ctx, _dprob, _dreg, _dstate):
        state = ctx.saved_tensors[0]
        gx, gd = rcnn_loss_backward(*ctx.saved_tensors[1:], state, cls_grad_scale=ctx.gs[0],
                                    reg_grad_scale=ctx.gs[1], smooth_l1_scalar=ctx.scalar)
        return (gx, gd) + (None,) * 6


def rcnn_loss(cls_logit, cls_label, bbox_delta, bbox_target, bbox_weight, *, cls_grad_scale=1.0, reg_grad_scale=1.0,
              smooth_l1_scalar=1.0):
    """rcnn_loss_forward with autograd to cls_logit and bbox_delta: RpnLossOut(prob, reg_loss, state).
    reg_grad_scale is the head's 1 / batch_roi; both scales carry fp16's 128 and the cascade's stage weight."""
    return RpnLossOut(*RcnnLossFunction.apply(cls_logit, bbox_delta, cls_label, bbox_target, bbox_weight,
                                              cls_grad_scale, reg_grad_scale, smooth_l1_scalar))


# --------------------------------------------------------------------------------------------------
# _contrib_Quantization_int8  (operator_cxx/contrib/quantization_int8{-inl.h,.cu}; utils/graph_optimize.py)
# --------------------------------------------------------------------------------------------------
QUANT_GRAD_MODES = ("ste", "clip")


def quant_int8_state(delay_quant=0, device=None):
    """The operator's step state on the device: int32 {countdown, init} = {delay_quant, 1}, as the reference's
    Operator object starts (quantization_int8-inl.h:103-108)."""
    if int(delay_quant) < 0:
        raise ValueError("delay_quant must be >= 0, got %d" % int(delay_quant))
    return torch.tensor([int(delay_quant), 1], dtype=torch.int32, device="cuda" if device is None else device)


def quant_int8_workspace_bytes(n):
    return _query("sd_quant_int8_workspace_bytes", int(n))


def quant_int8_weights_workspace_bytes(T, n_total):
    return _query("sd_quant_int8_weights_workspace_bytes", int(T), int(n_total))


def _q_aux(minmax, state):
    _chk(minmax, "minmax")
    _chk(state, "state", dtype=torch.int32)
    if minmax.numel() != 1 or state.numel() != 2:
        raise ValueError("minmax holds 1 float and state 2 ints, got %d and %d" % (minmax.numel(), state.numel()))


def quantization_int8_forward(data, minmax, state, *, is_weight, is_train=True, fix_act_scale=False,
                              ema_decay=0.99, out=None, workspace=None):
    """Quantization_int8 forward (quantization_int8-inl.h:113-226): data (any shape, fp32), minmax (1,) the
    operator's aux state, state = quant_int8_state(delay_quant).  minmax and state are updated in place on the
    device (a delay step copies and counts down; a training step tracks max|data| -- directly for weights, with
    the init rule and then the EMA for activations); out = round(clip(data) / u) * u with u = minmax / 127,
    weights unclipped.  Nothing is read back: the call can be captured in a graph.  Returns out."""
    _chk(data, "data")
    _q_aux(minmax, state)
    if out is None:
        out = torch.empty_like(data)
    else:
        _chk(out, "out")
        if out.shape != data.shape:
            raise ValueError("out must have the shape of data")
    if not 0.0 <= float(ema_decay) <= 1.0:
        raise ValueError("ema_decay must lie in [0, 1], got %r" % (ema_decay,))
    n = data.numel()
    if n == 0:
        return out
    ws = _ws(data.device, workspace, "sd_quant_int8_workspace_bytes", n)
    _call("sd_quant_int8_fwd", data, out, minmax, state, n, bool(is_weight), bool(is_train), bool(fix_act_scale),
          ema_decay, ws, ws.numel())
    return out


def quantization_int8_backward(out_grad, data, minmax, *, is_weight, grad_mode="ste", req="write", d_data=None):
    """Quantization_int8 backward (quantization_int8-inl.h:229-294): "ste" and every weight pass out_grad on;
    "clip" keeps it where -minmax <= data <= minmax (a NaN gives 0), minmax read on the device.  req 'write',
    'add' (d_data += ...; d_data required) or 'null' (nothing runs).  Returns d_data."""
    if grad_mode not in QUANT_GRAD_MODES:
        raise ValueError("grad_mode must be one of %s, got %r" % (QUANT_GRAD_MODES, grad_mode))
    if req not in REQ:
        raise ValueError("req must be one of %s, got %r" % (sorted(REQ), req))
    _chk(out_grad, "out_grad")
    clip = grad_mode == "clip" and not is_weight
    if clip:
        _chk(data, "data")
        _chk(minmax, "minmax")
        if data.numel() != out_grad.numel() or minmax.numel() != 1:
            raise ValueError("data must have the size of out_grad and minmax 1 float")
    if d_data is None:
        if req == "add":
            raise ValueError("req='add' accumulates into d_data: pass it")
        d_data = torch.empty_like(out_grad)
    else:
        _chk(d_data, "d_data")
        if d_data.numel() != out_grad.numel():
            raise ValueError("d_data must have the size of out_grad")
    _call("sd_quant_int8_bwd", out_grad, data if clip else None, minmax if clip else None, d_data, out_grad.numel(),
          clip, REQ[req])
    return d_data


def quant_int8_weights_table(datas, outs, minmaxes, states):
    """The device table of quantization_int8_weights_forward: (5, T) int64 -- data, out, minmax and state
    addresses and element counts.  Build it once per set of buffers (it is copied from the host) and pass it as
    `table=` to every step; the tensors must stay alive while it is used."""
    T = len(datas)
    if not (len(outs) == len(minmaxes) == len(states) == T):
        raise ValueError("datas, outs, minmaxes and states must have one entry per tensor")
    for d, o, m, s in zip(datas, outs, minmaxes, states):
        _chk(d, "data")
        _chk(o, "out")
        _q_aux(m, s)
        if o.shape != d.shape:
            raise ValueError("out must have the shape of data")
    dev = datas[0].device if T else "cuda"
    rows = [[t.data_ptr() for t in col] for col in (datas, outs, minmaxes, states)] + [[d.numel() for d in datas]]
    return torch.tensor(rows, dtype=torch.int64).reshape(5, T).to(dev)


def quantization_int8_weights_forward(datas, minmaxes, states, *, is_train=True, fix_act_scale=False, outs=None,
                                      table=None, workspace=None):
    """The weight forward of quantization_int8_forward for a list of tensors in two kernels in all (behind a
    one-workgroup clearing kernel when a tensor spans several workgroups): a segmented abs-max with one state
    transition per tensor, then one element-wise pass over the segment table.  Outputs,
    minmax and state are bit-equal to one call per tensor.  Returns the list of outputs."""
    T = len(datas)
    if table is None:
        if outs is None:
            outs = [torch.empty_like(d) for d in datas]
        table = quant_int8_weights_table(datas, outs, minmaxes, states)
    else:
        # the kernels write what the table names: it is taken on trust (checking it would be a copy to the host per
        # step), so the outputs it was built from must be named too
        if outs is None or len(outs) != T:
            raise ValueError("a table names its outputs: pass the outs it was built from")
        _chk(table, "table", dtype=torch.int64, ndim=2)
        if tuple(table.shape) != (5, T):
            raise ValueError("table must be (5, %d), got %s" % (T, tuple(table.shape)))
    n_total = sum(int(d.numel()) for d in datas)
    if T == 0 or n_total == 0:
        return outs
    ws = _ws(table.device, workspace, "sd_quant_int8_weights_workspace_bytes", T, n_total)
    _call("sd_quant_int8_weights_fwd", *table, T, n_total, bool(is_train), bool(fix_act_scale), ws, ws.numel())
    return outs


class QuantizationInt8Function(torch.autograd.Function):
    """out = QuantizationInt8Function.apply(data, minmax, state, is_weight, is_train, fix_act_scale, ema_decay,
    grad_mode); minmax and state are updated in place and carry no gradient."""

    @staticmethod
    def forward(ctx, data, minmax, state, is_weight, is_train, fix_act_scale, ema_decay, grad_mode):
        if grad_mode not in QUANT_GRAD_MODES:
            raise ValueError("grad_mode must be one of %s, got %r" % (QUANT_GRAD_MODES, grad_mode))
        data = data.contiguous()
        out = quantization_int8_forward(data, minmax, state, is_weight=is_weight, is_train=is_train,
                                        fix_act_scale=fix_act_scale, ema_decay=ema_decay)
        ctx.save_for_backward(data, minmax)
        ctx.is_weight, ctx.grad_mode = bool(is_weight), grad_mode
        return out

    @staticmethod
    def backward(ctx, out_grad):
        data, minmax = ctx.saved_tensors
        d = quantization_int8_backward(out_grad.contiguous(), data, minmax, is_weight=ctx.is_weight,
                                       grad_mode=ctx.grad_mode).view(data.shape)
        return (d,) + (None,) * 7


def quantization_int8(data, minmax, state, *, is_weight=True, is_train=True, fix_act_scale=False, ema_decay=0.99,
                      grad_mode="ste"):
    """mx.sym.contrib.Quantization_int8 with autograd (the reference's defaults)."""
    return QuantizationInt8Function.apply(data, minmax, state, bool(is_weight), bool(is_train), bool(fix_act_scale),
                                          float(ema_decay), grad_mode)


# --------------------------------------------------------------------------------------------------
# FCOS training head  (models/FCOS/input.py make_fcos_gt, models/FCOS/loss.py, models/FCOS/builder.py get_loss)
# --------------------------------------------------------------------------------------------------
FcosTargets = collections.namedtuple("FcosTargets", "centerness offset cls_id state cls_dense")


def fcos_num_locations(data_size, strides):
    """(HW, [H_l * W_l per level]) of the reference's location grid (input.py:99-107)."""
    h, w = (int(v) for v in data_size)
    L = len(strides)
    levels, total = (ctypes.c_long * max(L, 1))(), (ctypes.c_long * 1)()
    _call("sd_fcos_num_locations", h, w, _iarr(strides), L, levels, total)
    return int(total[0]), [int(levels[i]) for i in range(L)]


def fcos_target_workspace_bytes(N, HW):
    return _query("sd_fcos_target_workspace_bytes", int(N), int(HW))


def fcos_loss_workspace_bytes(N, K, HW):
    return _query("sd_fcos_loss_workspace_bytes", int(N), int(K), int(HW))


def fcos_target(gt_bbox, im_info, data_size, strides, num_classifier, *, ignore_offset=-1.0, ignore_label=-1.0,
                stage_lower=None, stage_upper=None, dense=False, centerness=None, offset=None, cls_id=None,
                cls_dense=None, state=None, workspace=None):
    """make_fcos_gt (models/FCOS/input.py:180-263) in one kernel: gt_bbox (N, M, 5) [x1, y1, x2, y2, cls],
    im_info (N, 3), data_size (h, w), the FPN strides.  Returns FcosTargets: centerness (N, HW), offset (N, 4, HW),
    the compact cls_id (N, HW) int32 (-1 ignored, 0 background, 1..K class), the state block int32[4] with the three
    normalisers of the losses (state[0] = the foreground count), and with dense=True the reference's one-hot
    cls_gt (N, K * HW).  Nothing is read back from the device."""
    _chk(gt_bbox, "gt_bbox", ndim=3)
    _chk(im_info, "im_info", ndim=2)
    N, M = int(gt_bbox.shape[0]), int(gt_bbox.shape[1])
    if gt_bbox.shape[2] != 5 or tuple(im_info.shape) != (N, 3):
        raise ValueError("gt_bbox should be (N, M, 5) and im_info (N, 3), got %s and %s"
                         % (tuple(gt_bbox.shape), tuple(im_info.shape)))
    if (stage_lower is None) != (stage_upper is None):
        raise ValueError("stage_lower and stage_upper go together")
    L, K = len(strides), int(num_classifier)
    if stage_lower is not None and not (len(stage_lower) == len(stage_upper) == L):
        raise ValueError("the stage bounds need one entry per stride")
    HW, _ = fcos_num_locations(data_size, strides)
    dev = gt_bbox.device
    centerness = _out(centerness, "centerness", (N, HW), dev, flat=True)
    offset = _out(offset, "offset", (N, 4, HW), dev, flat=True)
    cls_id = _out(cls_id, "cls_id", (N, HW), dev, torch.int32, flat=True)
    state = _out(state, "state", (4,), dev, torch.int32, flat=True)
    if dense or cls_dense is not None:
        cls_dense = _out(cls_dense, "cls_dense", (N, K * HW), dev, flat=True)
    if N * HW == 0:       # the entry point writes nothing: the normalisers of an empty problem are zero
        state.zero_()
    ws = _ws(dev, workspace, "sd_fcos_target_workspace_bytes", N, HW)
    _call("sd_fcos_target", gt_bbox, im_info, centerness, offset, cls_id, cls_dense, state, N, M, K,
          int(data_size[0]), int(data_size[1]), _iarr(strides), None if stage_lower is None else _farr(stage_lower),
          None if stage_upper is None else _farr(stage_upper), L, ignore_offset, ignore_label, ws, ws.numel())
    return FcosTargets(centerness, offset, cls_id, state, cls_dense)


def _fcos_levels(cls_logits, ctr_logits, off_preds, targets):
    """(N, K, HW, hw table) of three lists of level tensors (N, K, H, W) / (N, 1, H, W) / (N, 4, H, W); a single
    level may also be the concatenated (N, K, HW) / (N, 1, HW) / (N, 4, HW) form."""
    L = len(cls_logits)
    if not (len(ctr_logits) == len(off_preds) == L) or L == 0:
        raise ValueError("cls_logits, ctr_logits and off_preds need one tensor per level each")
    N, K = int(cls_logits[0].shape[0]), int(cls_logits[0].shape[1])
    hws = []
    for i, (c, t, o) in enumerate(zip(cls_logits, ctr_logits, off_preds)):
        for v, name in ((c, "cls_logits"), (t, "ctr_logits"), (o, "off_preds")):
            _chk(v, "%s[%d]" % (name, i))
            if v.dim() < 3 or int(v.shape[0]) != N:
                raise ValueError("%s[%d] should be (N, C, ...), got %s" % (name, i, tuple(v.shape)))
        hw = c.numel() // (N * K) if N * K else 0
        if int(c.shape[1]) != K or t.numel() != N * hw or o.numel() != 4 * N * hw or int(o.shape[1]) != 4:
            raise ValueError("level %d: cls %s, centerness %s and offset %s do not belong together"
                             % (i, tuple(c.shape), tuple(t.shape), tuple(o.shape)))
        hws.append(hw)
    HW = sum(hws)
    _chk(targets.centerness, "centerness")
    _chk(targets.offset, "offset")
    _chk(targets.cls_id, "cls_id", dtype=torch.int32)
    _chk(targets.state, "state", dtype=torch.int32)
    if (targets.centerness.numel() != N * HW or targets.offset.numel() != 4 * N * HW
            or targets.cls_id.numel() != N * HW or targets.state.numel() < 4):
        raise ValueError("the targets do not hold N = %d images of HW = %d locations" % (N, HW))
    return N, K, HW, (ctypes.c_long * L)(*hws)


def fcos_loss_forward(cls_logits, ctr_logits, off_preds, targets, *, alpha=0.25, gamma=2.0, ignore_offset=-1.0,
                      ignore_label=-1.0, losses=None, workspace=None):
    """The three FCOS losses (models/FCOS/loss.py:86-196) over per-level tensors, without reshape / concat and
    without the one-hot labels: returns (3,) = centerness BCE, sigmoid focal, IoU -- the order of get_loss."""
    N, K, HW, hws = _fcos_levels(cls_logits, ctr_logits, off_preds, targets)
    dev = cls_logits[0].device
    losses = _out(losses, "losses", (3,), dev, flat=True)
    if N * K * HW == 0:
        return losses.zero_()
    ws = _ws(dev, workspace, "sd_fcos_loss_workspace_bytes", N, K, HW)
    _call("sd_fcos_loss_fwd", _parr(cls_logits), _parr(ctr_logits), _parr(off_preds), hws, len(cls_logits),
          targets.centerness, targets.offset, targets.cls_id, targets.state, losses, N, K, alpha, gamma, ignore_offset,
          ignore_label, ws, ws.numel())
    return losses


def fcos_loss_backward(cls_logits, ctr_logits, off_preds, targets, *, alpha=0.25, gamma=2.0, ignore_offset=-1.0,
                       ignore_label=-1.0, d_cls=None, d_ctr=None, d_off=None):
    """The gradients of fcos_loss_forward, written straight into per-level tensors of the inputs' shapes in ONE
    launch: (d_cls list, d_ctr list, d_off list).  No top gradient enters (the reference's losses ignore it)."""
    N, K, HW, hws = _fcos_levels(cls_logits, ctr_logits, off_preds, targets)
    outs = (_grad_levels(d_cls, cls_logits, "d_cls"), _grad_levels(d_ctr, ctr_logits, "d_ctr"),
            _grad_levels(d_off, off_preds, "d_off"))
    if N * K * HW == 0:
        return outs
    _call("sd_fcos_loss_bwd", _parr(cls_logits), _parr(ctr_logits), _parr(off_preds), _parr(outs[0]), _parr(outs[1]),
          _parr(outs[2]), hws, len(cls_logits), targets.centerness, targets.offset, targets.cls_id, targets.state, N,
          K, alpha, gamma, ignore_offset, ignore_label)
    return outs


class FcosLossFunction(torch.autograd.Function):
    """losses = FcosLossFunction.apply(targets, alpha, gamma, ignore_offset, ignore_label, L, *cls, *ctr, *off) with
    3 * L level tensors.  The backward returns the reference's gradients as they are: like the reference's loss
    nodes it does not look at the incoming gradient."""

    @staticmethod
    def forward(ctx, targets, alpha, gamma, ignore_offset, ignore_label, L, *levels):
        if len(levels) != 3 * L:
            raise ValueError("expected %d level tensors, got %d" % (3 * L, len(levels)))
        levels = [t.contiguous() for t in levels]
        ctx.kw = dict(alpha=alpha, gamma=gamma, ignore_offset=ignore_offset, ignore_label=ignore_label)
        ctx.targets, ctx.L = targets, L
        ctx.save_for_backward(*levels)
        return fcos_loss_forward(levels[:L], levels[L:2 * L], levels[2 * L:], targets, **ctx.kw)

    @staticmethod
    def backward(ctx, _out_grad):
        levels, L = list(ctx.saved_tensors), ctx.L
        d = fcos_loss_backward(levels[:L], levels[L:2 * L], levels[2 * L:], ctx.targets, **ctx.kw)
        return (None,) * 6 + tuple(d[0]) + tuple(d[1]) + tuple(d[2])


def fcos_loss(cls_logits, ctr_logits, off_preds, targets, *, alpha=0.25, gamma=2.0, ignore_offset=-1.0,
              ignore_label=-1.0):
    """The FCOS head's three losses with autograd over lists of level tensors: (3,) = centerness, classification,
    offset.  `targets` is what fcos_target returned; off_preds are the offsets after the graph's exp."""
    L = len(cls_logits)
    return FcosLossFunction.apply(targets, float(alpha), float(gamma), float(ignore_offset), float(ignore_label), L,
                                  *cls_logits, *ctr_logits, *off_preds)


# --------------------------------------------------------------------------------------------------
# RepPoints training head  (models/RepPoints/point_ops.py, models/RepPoints/builder.py get_loss)
# --------------------------------------------------------------------------------------------------
RepPointsTargets = collections.namedtuple("RepPointsTargets", "label_init gt_init label_refine gt_refine state")
REPPOINTS_TRANSFORMS = {"minmax": 0, "partial_minmax": 1, "moment": 2}


def reppoints_target_workspace_bytes(N, M, P):
    return _query("sd_reppoints_target_workspace_bytes", int(N), int(M), int(P))


def reppoints_box_loss_workspace_bytes(N, P):
    return _query("sd_reppoints_box_loss_workspace_bytes", int(N), int(P))


def _reppoints_levels(maps, strides, name, like=None):
    """(N, num_points, P, H table, W table, stride table) of a list of point maps (N, 2 * num_points, H_l, W_l)"""
    L = len(maps)
    if L == 0 or len(strides) != L:
        raise ValueError("%s needs one map per stride" % name)
    N, C = int(maps[0].shape[0]), int(maps[0].shape[1])
    for i, t in enumerate(maps):
        _chk(t, "%s[%d]" % (name, i), ndim=4)
        if int(t.shape[0]) != N or int(t.shape[1]) != C or C % 2:
            raise ValueError("%s[%d] should be (N, 2 * num_points, H, W), got %s" % (name, i, tuple(t.shape)))
        if like is not None and tuple(t.shape) != tuple(like[i].shape):
            raise ValueError("%s[%d] has shape %s, expected %s" % (name, i, tuple(t.shape), tuple(like[i].shape)))
    Hs, Ws = [int(t.shape[2]) for t in maps], [int(t.shape[3]) for t in maps]
    return N, C // 2, sum(h * w for h, w in zip(Hs, Ws)), _iarr(Hs), _iarr(Ws), _iarr(strides)


def _reppoints_transform(transform, moment_transfer):
    if transform not in REPPOINTS_TRANSFORMS:
        raise ValueError("transform %r is none of %s" % (transform, sorted(REPPOINTS_TRANSFORMS)))
    if moment_transfer is not None:
        _chk(moment_transfer, "moment_transfer")
        if moment_transfer.numel() != 2:
            raise ValueError("moment_transfer holds 2 values")
    elif transform == "moment":
        raise ValueError("the moment transform needs moment_transfer")
    return REPPOINTS_TRANSFORMS[transform]


def reppoints_target(pts_init, gt_bbox, strides, *, transform="moment", moment_transfer=None, target_scale=4,
                     num_pos=1, pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0, label_init=None, gt_init=None,
                     label_refine=None, gt_refine=None, state=None, workspace=None):
    """Both assigners of RepPointsHead.get_loss (models/RepPoints/builder.py:328-388) in one call: pts_init is the
    list of init-stage point maps (N, 2 * num_points, H_l, W_l), gt_bbox (N, M, 5) [x1, y1, x2, y2, cls].  Returns
    RepPointsTargets: label_init (N, P), gt_init (N, P, 4) of the point assigner, label_refine, gt_refine of the IoU
    assigner on the init boxes, and the state block int32[4] with the two BBoxNorm counts and denominators.
    Nothing is read back from the device."""
    N, K, P, Hs, Ws, st = _reppoints_levels(pts_init, strides, "pts_init")
    _chk(gt_bbox, "gt_bbox", ndim=3)
    if int(gt_bbox.shape[0]) != N or int(gt_bbox.shape[2]) != 5:
        raise ValueError("gt_bbox should be (N, M, 5) with N = %d, got %s" % (N, tuple(gt_bbox.shape)))
    M = int(gt_bbox.shape[1])
    tr = _reppoints_transform(transform, moment_transfer)
    dev = gt_bbox.device
    label_init = _out(label_init, "label_init", (N, P), dev, flat=True)
    gt_init = _out(gt_init, "gt_init", (N, P, 4), dev, flat=True)
    label_refine = _out(label_refine, "label_refine", (N, P), dev, flat=True)
    gt_refine = _out(gt_refine, "gt_refine", (N, P, 4), dev, flat=True)
    state = _out(state, "state", (4,), dev, torch.int32, flat=True)
    if N * P == 0:        # the entry point writes nothing: no label, and the denominators are 0 + 1
        state.copy_(torch.tensor([0, 0, 0x3f800000, 0x3f800000], dtype=torch.int32))
    ws = _ws(dev, workspace, "sd_reppoints_target_workspace_bytes", N, M, P)
    _call("sd_reppoints_target", _parr(pts_init), Hs, Ws, st, len(pts_init), gt_bbox, moment_transfer, label_init,
          gt_init, label_refine, gt_refine, state, N, M, K, tr, target_scale, int(num_pos), pos_iou_thr, neg_iou_thr,
          min_pos_iou, ws, ws.numel())
    return RepPointsTargets(label_init, gt_init, label_refine, gt_refine, state)


def _reppoints_loss_args(pts_init, pts_refine, targets, strides, transform, moment_transfer):
    N, K, P, Hs, Ws, st = _reppoints_levels(pts_init, strides, "pts_init")
    _reppoints_levels(pts_refine, strides, "pts_refine", like=pts_init)
    tr = _reppoints_transform(transform, moment_transfer)
    for name in ("label_init", "gt_init", "label_refine", "gt_refine"):
        t = _chk(getattr(targets, name), name)
        if t.numel() != N * P * (4 if name.startswith("gt") else 1):
            raise ValueError("the targets do not hold N = %d images of P = %d points" % (N, P))
    _chk(targets.state, "state", dtype=torch.int32)
    return N, K, P, Hs, Ws, st, tr


def reppoints_box_loss_forward(pts_init, pts_refine, targets, strides, *, transform="moment", moment_transfer=None,
                               scale=4, loss_init=None, loss_refine=None):
    """pts_init_loss and pts_refine_loss of RepPointsHead.get_loss (builder.py:415-481), each (N, P, 4), over
    per-level point maps in one launch: smooth_l1((box - gt) / (stride * scale), 3) * (label > 0)."""
    N, K, P, Hs, Ws, st, tr = _reppoints_loss_args(pts_init, pts_refine, targets, strides, transform, moment_transfer)
    dev = pts_init[0].device
    loss_init = _out(loss_init, "loss_init", (N, P, 4), dev, flat=True)
    loss_refine = _out(loss_refine, "loss_refine", (N, P, 4), dev, flat=True)
    _call("sd_reppoints_box_loss_fwd", _parr(pts_init), _parr(pts_refine), Hs, Ws, st, len(pts_init), moment_transfer,
          targets.label_init, targets.gt_init, targets.label_refine, targets.gt_refine, loss_init, loss_refine, N, K,
          tr, scale)
    return loss_init, loss_refine


def reppoints_box_loss_backward(pts_init, pts_refine, targets, strides, *, transform="moment", moment_transfer=None,
                                scale=4, grad_scale_init=0.5, grad_scale_refine=1.0, req="write", d_init=None,
                                d_refine=None, d_moment_transfer=None, workspace=None):
    """The gradients of both box losses in one launch: (d_pts_init list, d_pts_refine list, d_moment_transfer (2,)).
    No top gradient enters (MakeLoss); the head gradient is grad_scale / the BBoxNorm denominator of the state block.
    req = 'add' accumulates into the tensors given."""
    N, K, P, Hs, Ws, st, tr = _reppoints_loss_args(pts_init, pts_refine, targets, strides, transform, moment_transfer)
    if req not in ("write", "add"):
        raise ValueError("req is 'write' or 'add'")
    dev = pts_init[0].device
    outs = []
    for given, like, name in ((d_init, pts_init, "d_init"), (d_refine, pts_refine, "d_refine")):
        if given is None:
            if req == "add":
                raise ValueError("req='add' needs the tensors to add to")
            given = [torch.empty_like(t) for t in like]
        _reppoints_levels(given, strides, name, like=like)
        outs.append(list(given))
    if d_moment_transfer is None and req == "add":
        raise ValueError("req='add' needs the tensors to add to")
    d_moment_transfer = _out(d_moment_transfer, "d_moment_transfer", (2,), dev, flat=True)
    if N * P == 0:
        return outs[0], outs[1], d_moment_transfer if req == "add" else d_moment_transfer.zero_()
    ws = _ws(dev, workspace, "sd_reppoints_box_loss_workspace_bytes", N, P)
    _call("sd_reppoints_box_loss_bwd", _parr(pts_init), _parr(pts_refine), Hs, Ws, st, len(pts_init), moment_transfer,
          targets.label_init, targets.gt_init, targets.label_refine, targets.gt_refine, targets.state,
          _parr(outs[0]), _parr(outs[1]), d_moment_transfer, N, K, tr, scale, grad_scale_init, grad_scale_refine,
          REQ[req], ws, ws.numel())
    return outs[0], outs[1], d_moment_transfer


class RepPointsBoxLossFunction(torch.autograd.Function):
    """loss_init, loss_refine = RepPointsBoxLossFunction.apply(targets, strides, kw, moment_transfer, *pts_init,
    *pts_refine).  Like the reference's MakeLoss nodes the backward does not look at the incoming gradient."""

    @staticmethod
    def forward(ctx, targets, strides, kw, moment_transfer, *maps):
        L = len(strides)
        maps = [t.contiguous() for t in maps]
        ctx.targets, ctx.strides, ctx.kw, ctx.has_mt = targets, strides, kw, moment_transfer is not None
        ctx.save_for_backward(*([moment_transfer] if ctx.has_mt else []), *maps)
        fkw = {k: v for k, v in kw.items() if not k.startswith("grad_scale")}
        return reppoints_box_loss_forward(maps[:L], maps[L:], targets, strides, moment_transfer=moment_transfer, **fkw)

    @staticmethod
    def backward(ctx, *_out_grads):
        saved, L = list(ctx.saved_tensors), len(ctx.strides)
        mt = saved.pop(0) if ctx.has_mt else None
        di, dr, dmt = reppoints_box_loss_backward(saved[:L], saved[L:], ctx.targets, ctx.strides, moment_transfer=mt,
                                                  **ctx.kw)
        return (None, None, None, dmt if ctx.has_mt else None) + tuple(di) + tuple(dr)


def reppoints_box_loss(pts_init, pts_refine, targets, strides, *, transform="moment", moment_transfer=None, scale=4,
                       grad_scale_init=0.5, grad_scale_refine=1.0):
    """Both RepPoints box losses with autograd over lists of level maps: (loss_init, loss_refine), each (N, P, 4).
    `targets` is what reppoints_target returned."""
    kw = dict(transform=transform, scale=scale, grad_scale_init=grad_scale_init, grad_scale_refine=grad_scale_refine)
    return RepPointsBoxLossFunction.apply(targets, tuple(strides), kw, moment_transfer, *pts_init, *pts_refine)


# --------------------------------------------------------------------------------------------------
# FCOS test-time decode  (models/FCOS/builder.py get_all_proposal, models/FCOS/utils.py: the CustomOps
# get_proposal_single_stage and get_batch_proposal)
# --------------------------------------------------------------------------------------------------
def fcos_decode_workspace_bytes(N, C, hws, top_n):
    """bytes of workspace of fcos_decode; hws = H_l * W_l per level"""
    L = len(hws)
    return _query("sd_fcos_decode_workspace_bytes", int(N), int(C), L, (ctypes.c_long * max(L, 1))(*hws), int(top_n))


def fcos_sigmoid(x, out=None):
    """1.0f / (1.0f + expf(-x)) element-wise: the sigmoid fcos_decode(input_logits=True) applies, same bits."""
    _chk(x, "x")
    out = _out(out, "out", x.shape, x.device, flat=True)
    _call("sd_fcos_sigmoid", x, out, x.numel())
    return out


def fcos_decode(cls_list, ctr_list, off_list, im_info, strides, top_n, pre_nms_thresh, input_logits=False,
                return_stage=False, *, bbox=None, score=None, cls_id=None, stage=None, workspace=None):
    """FCOSFPNHead.get_all_proposal (models/FCOS/builder.py:234-259) in one call: per level cls (N, C, H, W),
    ctr (N, 1, H, W), off (N, 4, H, W); im_info (N, 3) on the device; strides, top_n = pre_nms_top_n and
    pre_nms_thresh as the reference's CustomOp takes them.  input_logits=False: cls and ctr are probabilities (the
    CustomOps' contract); True: raw logits, the sigmoid is fused.  Returns (bbox (N, R, 4), score (N, R, 81),
    cls_id (N, R)) with R = L * top_n, and with return_stage=True also the concat of the per-level (N, top_n, 6)
    rows.  Nothing is read back from the device."""
    L = len(cls_list)
    if L == 0 or not (len(ctr_list) == len(off_list) == len(strides) == L):
        raise ValueError("cls_list, ctr_list, off_list and strides need one entry per level each")
    _chk(im_info, "im_info", ndim=2)
    N, C = int(cls_list[0].shape[0]), int(cls_list[0].shape[1])
    if tuple(im_info.shape) != (N, 3):
        raise ValueError("im_info should be (N, 3) = (%d, 3), got %s" % (N, tuple(im_info.shape)))
    Hs, Ws = [], []
    for i, (c, t, o) in enumerate(zip(cls_list, ctr_list, off_list)):
        for v, name in ((c, "cls_list"), (t, "ctr_list"), (o, "off_list")):
            _chk(v, "%s[%d]" % (name, i), ndim=4)
        H, W = int(c.shape[2]), int(c.shape[3])
        if tuple(c.shape) != (N, C, H, W) or tuple(t.shape) != (N, 1, H, W) or tuple(o.shape) != (N, 4, H, W):
            raise ValueError("level %d: cls %s, centerness %s and offset %s do not belong together"
                             % (i, tuple(c.shape), tuple(t.shape), tuple(o.shape)))
        Hs.append(H)
        Ws.append(W)
    top_n = int(top_n)
    R = L * max(top_n, 0)
    dev = im_info.device
    bbox = _out(bbox, "bbox", (N, R, 4), dev, flat=True)
    score = _out(score, "score", (N, R, 81), dev, flat=True)
    cls_id = _out(cls_id, "cls_id", (N, R), dev, flat=True)
    if return_stage or stage is not None:
        stage = _out(stage, "stage", (N, R, 6), dev, flat=True)
    hws = [h * w for h, w in zip(Hs, Ws)]
    ws = _ws(dev, workspace, fcos_decode_workspace_bytes(N, C, hws, top_n))
    _call("sd_fcos_decode", _parr(cls_list), _parr(ctr_list), _parr(off_list), im_info, _iarr(Hs), _iarr(Ws),
          _iarr(strides), L, N, C, top_n, pre_nms_thresh, bool(input_logits), bbox, score, cls_id, stage, ws,
          ws.numel())
    return (bbox, score, cls_id, stage) if return_stage else (bbox, score, cls_id)


# --------------------------------------------------------------------------------------------------
# RepPoints test-time decode  (models/RepPoints/builder.py RepPointsHead.get_prediction)
# --------------------------------------------------------------------------------------------------
def reppoints_topk_table(strides, pre_nms_top_n):
    """rows kept per level as get_prediction chooses them (builder.py:499-502): pre_nms_top_n if stride <= 32 else
    -1 (= all locations of the level)"""
    return [int(pre_nms_top_n) if int(s) <= 32 else -1 for s in strides]


def reppoints_decode_workspace_bytes(N, C, hws, ks):
    """bytes of workspace of reppoints_decode; hws = H_l * W_l and ks = rows kept (<= 0: all) per level"""
    L = len(hws)
    if len(ks) != L:
        raise ValueError("hws and ks need one entry per level each")
    return _query("sd_reppoints_decode_workspace_bytes", int(N), int(C), L, (ctypes.c_long * max(L, 1))(*hws),
                  _iarr(ks))


def reppoints_decode(cls_list, pts_refine_list, im_info, strides, ks, *, transform="moment", moment_transfer=None,
                     input_logits=False, cls_score=None, bbox_xyxy=None, workspace=None):
    """RepPointsHead.get_prediction (models/RepPoints/builder.py:486-576) in one call: per level cls (N, C, H, W) and
    pts_out_refine (N, 2 * num_points, H, W); im_info (N, 3) on the device; ks = rows kept per level, <= 0 keeps
    every location (reppoints_topk_table gives the reference's rule).  input_logits=False: cls holds probabilities;
    True: raw logits, the sigmoid is fused.  Returns (cls_score (N, R, C + 1), bbox_xyxy (N, R, 4)) with R the sum
    of the rows kept, levels in the order given, each in descending order of its best class score.  Nothing is read
    back from the device."""
    L = len(cls_list)
    if L == 0 or not (len(pts_refine_list) == len(strides) == len(ks) == L):
        raise ValueError("cls_list, pts_refine_list, strides and ks need one entry per level each")
    _chk(im_info, "im_info", ndim=2)
    N, C = int(cls_list[0].shape[0]), int(cls_list[0].shape[1])
    if tuple(im_info.shape) != (N, 3):
        raise ValueError("im_info should be (N, 3) = (%d, 3), got %s" % (N, tuple(im_info.shape)))
    K2 = int(pts_refine_list[0].shape[1]) if pts_refine_list[0].dim() == 4 else 0
    if K2 < 2 or K2 % 2:
        raise ValueError("pts_refine_list[0] should be (N, 2 * num_points, H, W), got %s" % (tuple(pts_refine_list[0].shape),))
    Hs, Ws = [], []
    for i, (c, t) in enumerate(zip(cls_list, pts_refine_list)):
        _chk(c, "cls_list[%d]" % i, ndim=4)
        _chk(t, "pts_refine_list[%d]" % i, ndim=4)
        H, W = int(c.shape[2]), int(c.shape[3])
        if tuple(c.shape) != (N, C, H, W) or tuple(t.shape) != (N, K2, H, W):
            raise ValueError("level %d: cls %s and points %s do not belong together" % (i, tuple(c.shape), tuple(t.shape)))
        Hs.append(H)
        Ws.append(W)
    tr = _reppoints_transform(transform, moment_transfer)
    hws = [h * w for h, w in zip(Hs, Ws)]
    ks = [int(k) for k in ks]
    R = sum(k if k > 0 else hw for k, hw in zip(ks, hws))
    dev = im_info.device
    cls_score = _out(cls_score, "cls_score", (N, R, C + 1), dev, flat=True)
    bbox_xyxy = _out(bbox_xyxy, "bbox_xyxy", (N, R, 4), dev, flat=True)
    ws = _ws(dev, workspace, reppoints_decode_workspace_bytes(N, C, hws, ks))
    _call("sd_reppoints_decode", _parr(cls_list), _parr(pts_refine_list), im_info, moment_transfer, _iarr(Hs),
          _iarr(Ws), _iarr(strides), _iarr(ks), L, N, C, K2 // 2, tr, bool(input_logits), cls_score, bbox_xyxy, ws,
          ws.numel())
    return cls_score, bbox_xyxy


# --------------------------------------------------------------------------------------------------
# _contrib_NMS (operator_cxx/contrib/nms{-inl.h,.cu}) and the Cython soft-NMS family
# --------------------------------------------------------------------------------------------------
def nms(dets, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, threshold=0.7, already_sorted=False,
        threshold_ge=False, return_index=False):
    """_contrib_NMS (GPU path nms.cu:249-365): dets (B,N,5) -> out (B,post,4), score (B,post,1)
    (shape nms-inl.h:96-107; post = min(rpn_post_nms_top_n, pre))."""
    _chk(dets, "dets", ndim=3)
    if dets.shape[2] != 5:
        raise ValueError("bbox should be (batch, rois, 5)")
    B, N, _ = dets.shape
    pre = int(rpn_pre_nms_top_n) if rpn_pre_nms_top_n > 0 else N
    pre = min(pre, N)
    post = min(int(rpn_post_nms_top_n), pre)
    out = torch.empty((B, post, 4), device=dets.device, dtype=torch.float32)
    score = torch.empty((B, post, 1), device=dets.device, dtype=torch.float32)
    keep = torch.empty((B, post), device=dets.device, dtype=torch.int32) if return_index else None
    ws = _ws(dets.device, None, "sd_nms_workspace_bytes", B, N, int(rpn_pre_nms_top_n))
    _call("sd_nms", dets, B, N, int(rpn_pre_nms_top_n), int(rpn_post_nms_top_n), threshold, bool(threshold_ge),
          bool(already_sorted), out, score, keep, ws, ws.numel())
    return (out, score, keep) if return_index else (out, score)


SOFT_NMS_METHODS = {"hard": 0, "linear": 1, "gaussian": 2}


def soft_nms_batched(dets, counts=None, sigma=0.5, Nt=0.3, threshold=0.001, method=0):
    """soft_nms (cpu_nms.pyx:98-203) on P problems at once: dets (P,Nmax,5), counts (P) int32 ->
    out_dets (P,Nmax,5), out_inds (P,Nmax) int32, out_counts (P) int32 (rows past the count are
    unspecified)."""
    _chk(dets, "dets", ndim=3)
    if dets.shape[2] != 5:
        raise ValueError("dets should be (problems, boxes, 5)")
    P, Nmax, _ = dets.shape
    if counts is not None:
        _chk(counts, "counts", dtype=torch.int32, ndim=1)
    if isinstance(method, str):
        if method not in SOFT_NMS_METHODS:
            raise ValueError("Unknown soft_nms method: {}".format(method))
        method = SOFT_NMS_METHODS[method]
    od = torch.empty_like(dets)
    oi = torch.empty((P, Nmax), device=dets.device, dtype=torch.int32)
    oc = torch.empty((P,), device=dets.device, dtype=torch.int32)
    _call("sd_soft_nms_batched", dets, counts, P, Nmax, sigma, Nt, threshold, int(method), od, oi, oc)
    return od, oi, oc


def bbox_overlaps(boxes, query_boxes):
    """bbox_overlaps_cython (bbox.pyx:31-72): boxes (n,4), query_boxes (k,4) -> overlaps (n,k)."""
    _chk(boxes, "boxes", ndim=2)
    _chk(query_boxes, "query_boxes", ndim=2)
    n, k = boxes.shape[0], query_boxes.shape[0]
    ov = torch.empty((n, k), device=boxes.device, dtype=torch.float32)
    _call("sd_bbox_overlaps", boxes, n, query_boxes, k, ov)
    return ov


# --------------------------------------------------------------------------------------------------
# DeformableConvolution v1 (mx.sym.contrib.DeformableConvolution, models/dcn/builder.py:14-17)
# --------------------------------------------------------------------------------------------------
def _dcn_hw(v, name):
    """an int (both axes) or an (h, w) pair -> (h, w)"""
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError("%s must be an int or have 2 entries (h, w)" % name)
        return int(v[0]), int(v[1])
    return int(v), int(v)


def _dcn_out_hw(H, W, kh, kw, pad, stride, dil):
    (ph, pw), (sh, sw), (dh, dw) = _dcn_hw(pad, "pad"), _dcn_hw(stride, "stride"), _dcn_hw(dil, "dilate")
    return ((H + 2 * ph - (dh * (kh - 1) + 1)) // sh + 1,
            (W + 2 * pw - (dw * (kw - 1) + 1)) // sw + 1)


def _dcn_geom(pad, stride, dilate):
    """the six per-axis geometry arguments of the piece entry points, in the C ABI's order"""
    return _dcn_hw(pad, "pad") + _dcn_hw(stride, "stride") + _dcn_hw(dilate, "dilate")


def deform_im2col(x, offset, kernel=(3, 3), pad=1, stride=1, dilate=1, num_deformable_group=1):
    """deformable_im2col: x (N,C,H,W), offset (N,dg*2*kh*kw,Ho,Wo) -> col (N, C*kh*kw, Ho*Wo).
    pad, stride and dilate are each an int (both axes) or an (h, w) pair, here and in the two col2im pieces."""
    _chk(x, "x", ndim=4)
    _chk(offset, "offset", ndim=4)
    N, C, H, W = x.shape
    kh, kw = kernel
    Ho, Wo = _dcn_out_hw(H, W, kh, kw, pad, stride, dilate)
    col = torch.empty((N, C * kh * kw, Ho * Wo), device=x.device, dtype=torch.float32)
    _call("sd_deform_im2col", x, offset, col, N, C, H, W, kh, kw, *_dcn_geom(pad, stride, dilate),
          int(num_deformable_group))
    return col


def deform_col2im(col, offset, x_shape, kernel=(3, 3), pad=1, stride=1, dilate=1,
                  num_deformable_group=1, workspace=True):
    _chk(col, "col", ndim=3)
    _chk(offset, "offset", ndim=4)
    N, C, H, W = [int(v) for v in x_shape]
    kh, kw = kernel
    dx = torch.empty((N, C, H, W), device=col.device, dtype=torch.float32)
    if not workspace:   # fp32 compare-and-swap adds (what a caller without a workspace gets)
        _call("sd_deform_col2im", col, offset, dx, REQ["write"], N, C, H, W, kh, kw, *_dcn_geom(pad, stride, dilate),
              int(num_deformable_group))
        return dx
    ws = _ws(col.device, None, "sd_deform_col2im_workspace_bytes", N, int(num_deformable_group))
    _call("sd_deform_col2im_ws", col, offset, dx, REQ["write"], N, C, H, W, kh, kw, *_dcn_geom(pad, stride, dilate),
          int(num_deformable_group), ws, ws.numel())
    return dx


def deform_col2im_coord(col, x, offset, kernel=(3, 3), pad=1, stride=1, dilate=1,
                        num_deformable_group=1):
    _chk(col, "col", ndim=3)
    _chk(x, "x", ndim=4)
    _chk(offset, "offset", ndim=4)
    N, C, H, W = x.shape
    kh, kw = kernel
    doff = torch.empty_like(offset)
    _call("sd_deform_col2im_coord", col, x, offset, doff, REQ["write"], N, C, H, W, kh, kw,
          *_dcn_geom(pad, stride, dilate), int(num_deformable_group))
    return doff


def gemm_f32(a, b, trans_a=False, trans_b=False, out=None, accumulate=0):
    """Batched fp32-in / fp32-out matrix-core GEMM: a (Bt,M,K) or its transpose, b (Bt,K,N) or its
    transpose.  Default arithmetic: scaled fp16 hi/lo split on the f16 matrix cores after a max|.|
    pre-pass over both operands (accuracy of the fp32 MFMA path); tuning key `deform_gemm_split` = 1:
    bf16 split (4.5e-6 x max|C|), 0: fp32 MFMA; see include/simpledet_ops.h."""
    _chk(a, "a", ndim=3)
    _chk(b, "b", ndim=3)
    Bt = a.shape[0]
    M, K = (a.shape[2], a.shape[1]) if trans_a else (a.shape[1], a.shape[2])
    K2, N = (b.shape[2], b.shape[1]) if trans_b else (b.shape[1], b.shape[2])
    if K != K2 or b.shape[0] != Bt:
        raise ValueError("GEMM shape mismatch")
    if out is None:
        out = torch.empty((Bt, M, N), device=a.device, dtype=torch.float32)
    ws = _ws(a.device, None, 64)
    _call("sd_gemm_f32_ws", trans_a, trans_b, M, N, K, a, a.shape[2], a.shape[1] * a.shape[2], b,
          b.shape[2], b.shape[1] * b.shape[2], out, N, M * N, Bt, int(accumulate), ws, ws.numel())
    return out


def deform_conv_forward(x, offset, weight, pad=1, stride=1, dilate=1, num_deformable_group=1,
                        keep_col=False, bias=None, num_group=1):
    """DeformableConvolution forward: y (N,F,Ho,Wo).  weight (F, C / num_group, kh, kw); bias (F) or None
    (= no_bias).  keep_col=True returns (y, workspace): the workspace holds the col matrix; handed to
    deform_conv_backward(fwd_ws=...) it saves the backward its own im2col."""
    _chk(x, "data", ndim=4)
    _chk(offset, "offset", ndim=4)
    _chk(weight, "weight", ndim=4)
    N, C, H, W = x.shape
    F, Cw, kh, kw = weight.shape
    num_group = int(num_group)
    if num_group < 1 or C % num_group or F % num_group:
        raise ValueError("num_group %d must divide data channels %d and num_filter %d" % (num_group, C, F))
    if Cw * num_group != C:
        raise ValueError("weight channels %d != data channels %d / num_group %d" % (Cw, C, num_group))
    if bias is not None:
        _chk(bias, "bias", ndim=1)
        if bias.shape[0] != F:
            raise ValueError("bias has %d entries, num_filter is %d" % (bias.shape[0], F))
    Ho, Wo = _dcn_out_hw(H, W, kh, kw, pad, stride, dilate)
    if tuple(offset.shape) != (N, num_deformable_group * 2 * kh * kw, Ho, Wo):
        raise ValueError("offset shape %s != %s" % (tuple(offset.shape),
                                                     (N, num_deformable_group * 2 * kh * kw, Ho, Wo)))
    y = torch.empty((N, F, Ho, Wo), device=x.device, dtype=torch.float32)
    # keep_col = False: no col matrix where the shape allows -- sampling fused into the GEMM (3x3, num_group 1,
    # C / groups % 16 == 0, H*W % 4 == 0); other shapes run im2col + GEMM behind the same entry point, which
    # its workspace size accounts for
    ws = _ws(x.device, None, "sd_deform_convolution_fwd_workspace_bytes", N, C, H, W, F, kh, kw, pad, stride, dilate,
             int(num_deformable_group), num_group, bool(keep_col))
    _call("sd_deform_convolution_fwd", x, offset, weight, bias, y, N, C, H, W, F, kh, kw, pad, stride, dilate,
          int(num_deformable_group), num_group, bool(keep_col), ws, ws.numel())
    return (y, ws) if keep_col else y


def deform_conv_backward(out_grad, x, offset, weight, pad=1, stride=1, dilate=1,
                         num_deformable_group=1, req=("write", "write", "write"), grads=None,
                         fwd_ws=None, num_group=1, bias=False):
    """-> (d_data, d_offset, d_weight[, d_bias]).  fwd_ws: the workspace deform_conv_forward(keep_col=True)
    returned for the same (x, offset): its col matrix is reused.  bias=True (the op had a bias): a fourth
    req / gradient, d_bias (F) = sum over images and pixels of out_grad."""
    _chk(out_grad, "out_grad", ndim=4)
    N, C, H, W = x.shape
    F, _, kh, kw = weight.shape
    r = [_req_of(v) for v in req]
    if bias and len(r) == 3:
        r.append(REQ["write"])
    if grads is None:
        grads = (torch.empty_like(x), torch.empty_like(offset), torch.empty_like(weight))
        if bias:
            grads = grads + (torch.empty(F, device=x.device, dtype=torch.float32),)
    elif len(grads) != (4 if bias else 3):
        raise ValueError("grads must hold %d tensors (d_data, d_offset, d_weight%s), got %d"
                         % (4 if bias else 3, ", d_bias" if bias else "", len(grads)))
    ws = _ws(x.device, None, "sd_deform_conv_workspace_bytes", N, C, H, W, kh, kw, pad, stride, dilate)
    col = None
    if fwd_ws is not None:
        col = (fwd_ws.data_ptr() + 255) & ~255  # sd_deform_conv_col_of_workspace
    _call("sd_deform_convolution_bwd", out_grad, x, offset, weight, col, grads[0], grads[1], grads[2],
          grads[3] if bias else None, r[0], r[1], r[2], r[3] if bias else REQ["null"], N, C, H, W, F, kh, kw, pad,
          stride, dilate, int(num_deformable_group), int(num_group), ws, ws.numel())
    return grads


# --------------------------------------------------------------------------------------------------
# _contrib_Proposal_v3 + get_top_proposal  (operator_cxx/contrib/proposal_v3{-inl.h,.cu},
# models/FPN/get_top_proposal.py) -- SURVEY 8(f) rank 1
# --------------------------------------------------------------------------------------------------
def _farr(vals):
    return (ctypes.c_float * len(vals))(*[float(v) for v in vals])


def proposal_v3(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
                threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.), ratios=(0.5, 1., 2.),
                feature_stride=16, is_train=False, iou_loss=False):
    """Proposal_v3: cls_prob (B,2A,H,W), bbox_pred (B,4A,H,W), im_info (B,3) ->
    output (B,post,4), score (B,post,1)   (shapes proposal_v3-inl.h:196-214)."""
    _chk(cls_prob, "cls_prob", ndim=4)
    _chk(bbox_pred, "bbox_pred", ndim=4)
    _chk(im_info, "im_info", ndim=2)
    B, A2, H, W = cls_prob.shape
    A = A2 // 2
    if bbox_pred.shape != (B, 4 * A, H, W) or im_info.shape != (B, 3):
        raise ValueError("bbox_pred must be (B,4A,H,W) and im_info (B,3)")
    scales, ratios = list(scales), list(ratios)
    count = A * H * W
    pre = rpn_pre_nms_top_n if rpn_pre_nms_top_n > 0 else count
    pre = min(pre, count)
    post = int(rpn_post_nms_top_n) if not is_train else min(int(rpn_post_nms_top_n), pre)
    out = torch.empty((B, post, 4), device=cls_prob.device, dtype=torch.float32)
    score = torch.empty((B, post, 1), device=cls_prob.device, dtype=torch.float32)
    ws = _ws(cls_prob.device, None, "sd_proposal_v3_workspace_bytes", B, A, H, W, int(rpn_pre_nms_top_n))
    _call("sd_proposal_v3_iou" if iou_loss else "sd_proposal_v3", cls_prob, bbox_pred, im_info, out, score, B, A, H, W,
          int(rpn_pre_nms_top_n), int(rpn_post_nms_top_n), threshold, int(rpn_min_size), _farr(scales), len(scales),
          _farr(ratios), len(ratios), int(feature_stride), bool(is_train), ws, ws.numel())
    return out, score


# --------------------------------------------------------------------------------------------------
# _contrib_Proposal_v2 (TridentNet) and _contrib_Proposal  (operator_cxx/contrib/proposal_v2.cu,
# proposal.cu): filters before the top-k, NMS with IoU > threshold
# --------------------------------------------------------------------------------------------------
def _proposal_v12_args(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n, rpn_post_nms_top_n):
    _chk(cls_prob, "cls_prob", ndim=4)
    _chk(bbox_pred, "bbox_pred", ndim=4)
    _chk(im_info, "im_info", ndim=2)
    B, A2, H, W = cls_prob.shape
    A = A2 // 2
    if bbox_pred.shape != (B, 4 * A, H, W) or im_info.shape != (B, 3):
        raise ValueError("bbox_pred must be (B,4A,H,W) and im_info (B,3)")
    post = int(rpn_post_nms_top_n)
    out = torch.empty((B, post, 4), device=cls_prob.device, dtype=torch.float32)
    score = torch.empty((B, post, 1), device=cls_prob.device, dtype=torch.float32)
    return B, A, H, W, out, score


def proposal_v2(cls_prob, bbox_pred, im_info, valid_ranges, rpn_pre_nms_top_n=6000,
                rpn_post_nms_top_n=300, threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.),
                ratios=(0.5, 1., 2.), feature_stride=16, filter_scales=False, iou_loss=False,
                workspace=None):
    """Proposal_v2: cls_prob (B,2A,H,W), bbox_pred (B,4A,H,W), im_info (B,3), valid_ranges (B,2) ->
    output (B,post,4), score (B,post,1)  (proposal_v2-inl.h:196-220), zero padded.
    rpn_post_nms_top_n > min(rpn_pre_nms_top_n, A*H*W) is refused (SimpleDetOpsError).
    workspace: an optional uint8 tensor of at least sd_proposal_v2_workspace_bytes() bytes."""
    B, A, H, W, out, score = _proposal_v12_args(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n,
                                                rpn_post_nms_top_n)
    _chk(valid_ranges, "valid_ranges", ndim=2)
    if valid_ranges.shape != (B, 2):
        raise ValueError("valid_ranges must be (B,2)")
    scales, ratios = list(scales), list(ratios)
    ws = _ws(cls_prob.device, workspace, "sd_proposal_v2_workspace_bytes", B, A, H, W, int(rpn_pre_nms_top_n))
    _call("sd_proposal_v2", cls_prob, bbox_pred, im_info, valid_ranges, out, score, B, A, H, W,
          int(rpn_pre_nms_top_n), int(rpn_post_nms_top_n), threshold, int(rpn_min_size), _farr(scales), len(scales),
          _farr(ratios), len(ratios), int(feature_stride), bool(filter_scales), bool(iou_loss), ws, ws.numel())
    return out, score


def proposal(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
             threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.), ratios=(0.5, 1., 2.),
             feature_stride=16, is_train=False, iou_loss=False, workspace=None):
    """Proposal: cls_prob (B,2A,H,W), bbox_pred (B,4A,H,W), im_info (B,3) -> output (B,post,4),
    score (B,post,1)  (proposal-inl.h:196-214); padding: the kept boxes repeated when is_train,
    else zeros.  rpn_post_nms_top_n > min(rpn_pre_nms_top_n, A*H*W) is refused."""
    B, A, H, W, out, score = _proposal_v12_args(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n,
                                                rpn_post_nms_top_n)
    scales, ratios = list(scales), list(ratios)
    ws = _ws(cls_prob.device, workspace, "sd_proposal_workspace_bytes", B, A, H, W, int(rpn_pre_nms_top_n))
    _call("sd_proposal", cls_prob, bbox_pred, im_info, out, score, B, A, H, W, int(rpn_pre_nms_top_n),
          int(rpn_post_nms_top_n), threshold, int(rpn_min_size), _farr(scales), len(scales), _farr(ratios),
          len(ratios), int(feature_stride), bool(is_train), bool(iou_loss), ws, ws.numel())
    return out, score


def get_top_proposal(bbox, score, top_n):
    """get_top_proposal CustomOp: bbox (B,N,4), score (B,N,1) -> (B,top_n,4), (B,top_n,1)."""
    _chk(bbox, "bbox", ndim=3)
    _chk(score, "score", ndim=3)
    B, N, _ = bbox.shape
    ob = torch.empty((B, int(top_n), 4), device=bbox.device, dtype=torch.float32)
    os_ = torch.empty((B, int(top_n), 1), device=bbox.device, dtype=torch.float32)
    _call("sd_get_top_proposal", bbox, score, B, N, int(top_n), ob, os_)
    return ob, os_


# --------------------------------------------------------------------------------------------------
# _contrib_GenProposalRetina  (operator_cxx/contrib/generate_proposal_retina{-inl.h,.cu},
# models/retinanet/builder.py:358-389)
# --------------------------------------------------------------------------------------------------
def gen_proposal_retina_workspace_bytes(B, AK, H, W):
    return _query("sd_gen_proposal_retina_workspace_bytes", B, AK, H, W)


def gen_proposal_retina(cls_prob, bbox_pred, im_info, anchors, *, num_anchors, rpn_pre_nms_top_n=6000,
                        rpn_min_size=16, thresh=0., anchor_mean=(0.,) * 4, anchor_std=(1.,) * 4,
                        iou_loss=False, output_one_hot=True, batch_wise_anchor=False,
                        feature_stride=16, workspace=None):
    """GenProposalRetina: cls_prob (B,A*K,H,W), bbox_pred (B,4A,H,W), im_info (B,3), anchors (H*W*A,4)
    [(B,H*W*A,4) with batch_wise_anchor] -> out (B,rpn_pre_nms_top_n,4),
    score (B,rpn_pre_nms_top_n,K+1 if output_one_hot else 1)  (generate_proposal_retina-inl.h:106-140).
    feature_stride only feeds a host-side size check in the reference and is not used.
    workspace: an optional uint8 tensor of at least gen_proposal_retina_workspace_bytes() bytes."""
    _chk(cls_prob, "cls_prob", ndim=4)
    _chk(bbox_pred, "bbox_pred", ndim=4)
    _chk(im_info, "im_info", ndim=2)
    _chk(anchors, "anchors")
    B, AK, H, W = cls_prob.shape
    A = int(num_anchors)
    if A <= 0 or AK % A:
        raise ValueError("cls_prob channels (%d) must be a multiple of num_anchors (%d)" % (AK, A))
    K = AK // A
    if bbox_pred.shape != (B, 4 * A, H, W) or im_info.shape != (B, 3):
        raise ValueError("bbox_pred must be (B,4A,H,W) and im_info (B,3)")
    want = (B, H * W * A, 4) if batch_wise_anchor else (H * W * A, 4)
    if tuple(anchors.shape) != want:
        raise ValueError("anchors must be %s, got %s" % (want, tuple(anchors.shape)))
    if len(anchor_mean) != 4 or len(anchor_std) != 4:
        raise ValueError("anchor_mean / anchor_std need 4 values")
    top_n = int(rpn_pre_nms_top_n)
    oc = K + 1 if output_one_hot else 1
    out = torch.empty((B, top_n, 4), device=cls_prob.device, dtype=torch.float32)
    score = torch.empty((B, top_n, oc), device=cls_prob.device, dtype=torch.float32)
    ws = _ws(cls_prob.device, workspace, "sd_gen_proposal_retina_workspace_bytes", B, AK, H, W)
    _call("sd_gen_proposal_retina", cls_prob, bbox_pred, im_info, anchors, out, score, B, AK, H, W, A, top_n,
          int(rpn_min_size), thresh, _farr(anchor_mean), _farr(anchor_std), bool(iou_loss), bool(output_one_hot),
          bool(batch_wise_anchor), ws, ws.numel())
    return out, score


# --------------------------------------------------------------------------------------------------
# _contrib_DecodeBBox + test-time detection filter  (operator_cxx/contrib/decodebbox{-inl.h,.cc},
# detection_test.py:233-247) -- SURVEY 8(f) rank 2
# --------------------------------------------------------------------------------------------------
def decode_bbox(rois, bbox_pred, im_info, bbox_mean=(0., 0., 0., 0.), bbox_std=(.1, .1, .2, .2),
                class_agnostic=True, bbox_decode_type="xywh"):
    """DecodeBBox: rois (B,R,4), bbox_pred (B,R,4K), im_info (B,3) -> (B,R,4) if class_agnostic
    else (B,R,4K)  (decodebbox-inl.h:85-107)."""
    _chk(rois, "rois", ndim=3)
    _chk(bbox_pred, "bbox_pred", ndim=3)
    _chk(im_info, "im_info", ndim=2)
    if bbox_decode_type not in ("xywh", "xyxy"):
        raise ValueError("bbox_decode_type must be 'xywh' or 'xyxy'")
    B, R, _ = rois.shape
    K = bbox_pred.shape[2] // 4
    out = torch.empty((B, R, 4 if class_agnostic else 4 * K), device=rois.device,
                      dtype=torch.float32)
    _call("sd_decode_bbox", rois, bbox_pred, im_info, out, B, R, K, _farr(bbox_mean), _farr(bbox_std),
          bool(class_agnostic), bbox_decode_type == "xyxy")
    return out


def det_filter(bbox_xyxy, cls_score, min_det_score):
    """Per (image, class) rows with score > min_det_score as [box, score] (detection_test.py:
    236-247), in sd_soft_nms_batched's layout: dets (B*K,R,5), counts (B*K) int32."""
    _chk(bbox_xyxy, "bbox_xyxy", ndim=3)
    _chk(cls_score, "cls_score", ndim=3)
    B, R, K = cls_score.shape
    Kb = bbox_xyxy.shape[2] // 4
    dets = torch.empty((B * K, R, 5), device=cls_score.device, dtype=torch.float32)
    counts = torch.empty((B * K,), device=cls_score.device, dtype=torch.int32)
    _call("sd_det_filter", bbox_xyxy, cls_score, B, R, K, Kb, min_det_score, dets, counts)
    return dets, counts


# --------------------------------------------------------------------------------------------------
# numpy nms, batched, and the BboxPostProcessing CustomOp of Mask R-CNN's test graph
# (operator_py/nms.py:41-75, models/maskrcnn/bbox_post_processing.py:6-111)
# --------------------------------------------------------------------------------------------------
def hard_nms_batched(dets, counts=None, thresh=0.5):
    """nms (operator_py/nms.py:41-75, float32 numpy arithmetic, keeps ovr <= thresh) on P problems at
    once: dets (P,Nmax,5), counts (P) int32 -> out_dets (P,Nmax,5), out_inds (P,Nmax) int32 (input
    rows), out_counts (P) int32; rows past the count are unspecified.  Equal scores: the later input
    row first.  The layout is det_filter's, so do_nms of detection_test.py is
    hard_nms_batched(*det_filter(boxes, scores, min_det_score), thresh)."""
    _chk(dets, "dets", ndim=3)
    if dets.shape[2] != 5:
        raise ValueError("dets should be (problems, boxes, 5)")
    P, Nmax, _ = dets.shape
    if counts is not None:
        _chk(counts, "counts", dtype=torch.int32, ndim=1)
        if counts.shape[0] != P:
            raise ValueError("counts should have one entry per problem")
    od = torch.empty_like(dets)
    oi = torch.empty((P, Nmax), device=dets.device, dtype=torch.int32)
    oc = torch.empty((P,), device=dets.device, dtype=torch.int32)
    _call("sd_hard_nms_batched", dets, counts, P, Nmax, thresh, od, oi, oc)
    return od, oi, oc


def multiclass_nms(cls_score, bbox_xyxy, min_det_score=0.05, nms_thr=0.5, skip_background=False):
    """The per-class kept lists of multiclass_nms / do_nms before the image top-k: det_filter ->
    hard_nms_batched.  cls_score (B,R,K), bbox_xyxy (B,R,4) or (B,R,4K) -> out_dets (B,K',R,5),
    out_inds (B,K',R) int32 (rows of the image), out_counts (B,K') int32.  detection_test.py:233-267
    treats every column as a class (K' = K); skip_background drops column 0 as
    bbox_post_processing.py:8-10 does (K' = K - 1, views of the same buffers)."""
    dets, counts = det_filter(bbox_xyxy, cls_score, min_det_score)
    B, R, K = cls_score.shape
    od, oi, oc = hard_nms_batched(dets, counts, nms_thr)
    od, oi, oc = od.view(B, K, R, 5), oi.view(B, K, R), oc.view(B, K)
    if skip_background:
        od, oi, oc = od[:, 1:], oi[:, 1:], oc[:, 1:]
    return od, oi, oc


def bbox_post_processing_workspace_bytes(B, R, K, bbox_classes, max_det_per_image):
    return _query("sd_bbox_post_processing_workspace_bytes", B, R, K, bbox_classes, int(max_det_per_image))


def bbox_post_processing(cls_score, bbox_xyxy, max_det_per_image=100, min_det_score=0.05, nms_thr=0.5,
                         workspace=None, out=None):
    """BboxPostProcessing (models/maskrcnn/bbox_post_processing.py:43-72): cls_score (B,R,K) with the
    background in column 0, bbox_xyxy (B,R,4) or (B,R,4K) -> post_score (B,max_det,1),
    post_bbox_xyxy (B,max_det,4) (zero padded), post_cls (B,max_det,1) (-1 padded).
    workspace: an optional uint8 tensor of at least bbox_post_processing_workspace_bytes() bytes;
    out: optional (post_score, post_bbox_xyxy, post_cls) to write into."""
    _chk(cls_score, "cls_score", ndim=3)
    _chk(bbox_xyxy, "bbox_xyxy", ndim=3)
    B, R, K = cls_score.shape
    if bbox_xyxy.shape[0] != B or bbox_xyxy.shape[1] != R or bbox_xyxy.shape[2] % 4:
        raise ValueError("bbox_xyxy must be (B,R,4) or (B,R,4K), got %s" % (tuple(bbox_xyxy.shape),))
    Kb = bbox_xyxy.shape[2] // 4
    top = int(max_det_per_image)
    if out is None:
        out = (torch.empty((B, top, 1), device=cls_score.device, dtype=torch.float32),
               torch.empty((B, top, 4), device=cls_score.device, dtype=torch.float32),
               torch.empty((B, top, 1), device=cls_score.device, dtype=torch.float32))
    ps, pb, pc = out
    for t, name, last in ((ps, "post_score", 1), (pb, "post_bbox_xyxy", 4), (pc, "post_cls", 1)):
        _chk(t, name, ndim=3)
        if tuple(t.shape) != (B, top, last):
            raise ValueError("%s must be %s" % (name, (B, top, last)))
    wsb = bbox_post_processing_workspace_bytes(B, R, K, Kb, top) if K >= 1 and Kb in (1, K) else 16
    ws = _ws(cls_score.device, workspace, wsb)
    _call("sd_bbox_post_processing", cls_score, bbox_xyxy, B, R, K, Kb, min_det_score, nms_thr, top, ps, pb, pc, ws,
          ws.numel())
    return ps, pb, pc


def maskrcnn_test_chain(feats, rois, cls_score, bbox_pred, im_info, rcnn_stride, max_det_per_image=100,
                        min_det_score=0.05, nms_thr=0.5, bbox_mean=(0., 0., 0., 0.),
                        bbox_std=(.1, .1, .2, .2), class_agnostic=False, roi_canonical_scale=224,
                        roi_canonical_level=4):
    """The device side of MaskFasterRcnn.get_test_symbol (models/maskrcnn/builder.py:41-58) around the
    caller's heads: fused FPN RoIAlign 7x7 of `rois` -> [bbox head: cls_score (B,R,K), bbox_pred
    (B,R,4K) are the caller's] -> decode_bbox -> bbox_post_processing -> fused FPN RoIAlign 14x14 on
    post_bbox_xyxy.  No host synchronisation: capturable as one HIP graph.
    Returns (roi_feat (B,R,C,7,7), bbox_xyxy, post_score, post_bbox_xyxy, post_cls,
    mask_roi_feat (B,max_det,C,14,14)).  A padded row of post_bbox_xyxy is the box (0,0,0,0), an
    ordinary RoI to the extractor as it is to the reference's: it is assigned a pyramid level like any
    other tiny box and its 14x14 feature is whatever RoIAlign pools at the image's origin (NOT zeros);
    callers tell padding by post_cls == -1."""
    roi_feat, _ = fpn_roi_align_forward_packed(feats, rois, rcnn_stride, (7, 7), roi_canonical_scale,
                                               roi_canonical_level)
    boxes = decode_bbox(rois, bbox_pred, im_info, bbox_mean, bbox_std, class_agnostic=class_agnostic)
    ps, pb, pc = bbox_post_processing(cls_score, boxes, max_det_per_image, min_det_score, nms_thr)
    mask_feat, _ = fpn_roi_align_forward_packed(feats, pb, rcnn_stride, (14, 14), roi_canonical_scale,
                                                roi_canonical_level)
    return roi_feat, boxes, ps, pb, pc, mask_feat
