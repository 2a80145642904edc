"""MXNet CustomOp adapter: the reference's operator names on top of the HIP C ABI.

The reference (tusen-ai/simpledet) reaches its detection ops by NAME from the symbol graph
(`mx.sym.contrib.ROIAlign_v2`, `mx.sym.ROIPooling_v1`, `mx.sym.ProposalTarget`,
`mx.sym.contrib.GenAnchor`, `mx.sym.contrib.NMS`, `mx.sym.contrib.DeformableConvolution`, and the
Python CustomOp `assign_layer_fpn`).  Its only run-time extension hook is `mx.operator.CustomOp`
(canonical example operator_py/bbox_target.py:96-219), so this module

  1. registers one CustomOp per operator under the name  sd_<reference op name>, with the
     reference's argument names, output names, NUMBER OF VISIBLE OUTPUTS and parameter names
     (roi_align_v2.cc:170-186, roi_pooling_v1-inl.h:144-237, proposal_target-inl.h:283-330,
     generate_anchor-inl.h:70-118, nms-inl.h:124-160), and
  2. `install()` aliases the reference names to `mx.sym.Custom(op_type=...)` so symbol/builder.py,
     models/ and config/ run unchanged.

Layout: the helpers every adapter module shares (state, pointer path, workspace, prop base, alias path) live in
_mx_adapter.py and are re-exported here; the operators come one function per family (`_roi_pool_ops` ...
`_crowdhuman_ops`, each returning {name: (PropClass, where)}), merged by `_build_ops`; then registration, and the
opt-in features.

`import mxnet` happens inside `register()`: importing this module never needs MXNet (it is absent
in the build container; tests drive the adapter through a tiny stub of the mx.operator interface).

Data path: NDArray -> raw device pointer through MXNet's C API (MXNDArrayGetData) -> C ABI on the
stream `install(stream=...)` names (default: the NULL stream) -> sd_stream_synchronize on that stream before
forward()/backward() return, because MXNet treats a CustomOp's outputs as written when the callback returns
(threading).

The ordering ASSUMPTION of the default (stated because no MXNet build is available here to check it): MXNet's
engine has made the inputs ready before it calls the callback (`wait_to_read` on every input is a no-op then, and is
issued anyway); the kernels are launched on the legacy NULL stream, which the HIP runtime orders against every
blocking stream of the device -- MXNet's per-device compute streams are created blocking
(`mshadow::Stream<gpu>`: hipStreamCreate, not hipStreamNonBlocking) -- and the host-side synchronise at the end
makes the outputs complete before the engine marks them written.  That serialises the device per op, which is
the price of the only run-time hook the reference has.  The library itself needs none of it: every entry point
takes the stream and neither synchronises nor touches another stream (tests/test_mxnet_plugin.py runs the adapter's
ops back to back on a side stream with the per-op synchronise switched off).  A host that can hand the adapter
the stream MXNet orders the op's outputs on -- `install(stream=<int | callable>, sync=False)` -- gets asynchronous
launches; the FCompute shim of INTEGRATION.md (B) is that design inside MXNet (`ctx.get_stream<gpu>()`,
roi_align_v2-inl.h:182).
"""
import collections
import ctypes
import importlib
import os
import sys

from ._lib import SD_ERR_UNSUPPORTED, SimpleDetOpsError, lib
# the shared helpers, under the names this module has always had them (tests, tools and the satellites reach them here)
from ._mx_adapter import (IN_DATA, OUT_DATA, OUT_GRAD, REQ, _PREFIX, _bool, _call, _darr, _iarr,  # noqa: F401
                          _is_symbol, _namespaces, _no_add, _numel, _param_str, _ptr, _req, _require_write, _scratch,
                          _state, _stream, _sync, _table, _tuple, _wait, _ws, alias_ctor, drop_alias, op_base,
                          prop_base, put_alias, register_ops)


# ---------------------------------------------------------------------------------- operators ----
def _roi_pool_ops(mx):
    """RoI pooling: ROIAlign_v2, ROIPooling_v1, assign_layer_fpn, the fused FPN extractor, the deformable pools"""
    CustomOp, Op, Prop = mx.operator.CustomOp, op_base(mx), prop_base(mx)
    ops = {}

    # ---- _contrib_ROIAlign_v2: 2 inputs, 3 outputs (1 visible) ----
    class ROIAlignV2(CustomOp):
        def __init__(self, pooled_size, spatial_scale):
            super().__init__()
            self.ph, self.pw = pooled_size
            self.scale = spatial_scale

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            data, rois = in_data
            _wait(data, rois)
            B, C, H, W = data.shape
            R = rois.shape[1]
            ws, wsp, wsn = _ws(data, "sd_roi_align_v2_workspace_bytes", B, R)
            _call("sd_roi_align_v2_fwd_ws", _ptr(data), _ptr(rois), _ptr(out_data[0]),
                       _ptr(out_data[1]), _ptr(out_data[2]), B, C, H, W, R, self.ph, self.pw,
                       float(self.scale), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            data, rois = in_data
            _wait(out_grad[0], rois, out_data[1], out_data[2])
            B, C, H, W = data.shape
            R = rois.shape[1]
            _call("sd_roi_align_v2_bwd", _ptr(out_grad[0]), _ptr(rois), _ptr(out_data[1]),
                       _ptr(out_data[2]), _ptr(in_grad[0]), _ptr(in_grad[1]), _req(req[0]),
                       _req(req[1]), B, C, H, W, R, self.ph, self.pw, float(self.scale), None)
            _sync()

    class ROIAlignV2Prop(Prop):
        ARGS = ("data", "rois")
        OUTS = ("output", "maxidx_x", "maxidx_y")
        num_visible_outputs = 1
        OP, OP_ARGS = ROIAlignV2, ("pooled_size", "spatial_scale")
        # ROIAlignGrad_v2 (roi_align_v2-inl.h:206-218): dY, rois, maxidx_x, maxidx_y
        DEPS = ((OUT_GRAD, 0), (IN_DATA, 1), (OUT_DATA, 1), (OUT_DATA, 2))

        def __init__(self, pooled_size, spatial_scale):
            super().__init__(need_top_grad=True)
            self.pooled_size = _tuple(pooled_size, 2, int)
            self.spatial_scale = float(spatial_scale)
            if self.pooled_size[0] <= 0 or self.pooled_size[1] <= 0:
                raise ValueError("ROIAlignParam: pooled_size must be nonzero")
            if not 0.0 <= self.spatial_scale <= 1.0:
                raise ValueError("spatial_scale must be in [0, 1]")

        def infer_shape(self, in_shape):
            d, b = in_shape
            if len(d) != 4:
                raise ValueError("data should be a 4D tensor")
            if len(b) != 3 or b[2] != 4:
                raise ValueError("bbox should be a 3D tensor of shape [batch, rois, 4]")
            o = (b[0], b[1], d[1], self.pooled_size[0], self.pooled_size[1])
            return [d, b], [o, o, o]

    ops["_contrib_ROIAlign_v2"] = (ROIAlignV2Prop, ("contrib", "ROIAlign_v2"))

    # ---- ROIPooling_v1: 2 inputs, 2 outputs (1 visible) ----
    class ROIPoolingV1(CustomOp):
        def __init__(self, pooled_size, spatial_scale):
            super().__init__()
            self.ph, self.pw = pooled_size
            self.scale = spatial_scale

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            data, rois = in_data
            _wait(data, rois)
            B, C, H, W = data.shape
            _call("sd_roi_pool_v1_fwd", _ptr(data), _ptr(rois), _ptr(out_data[0]),
                       _ptr(out_data[1]), B, C, H, W, rois.shape[0], self.ph, self.pw,
                       float(self.scale), None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            data, rois = in_data
            _wait(out_grad[0], rois, out_data[1])
            B, C, H, W = data.shape
            _call("sd_roi_pool_v1_bwd", _ptr(out_grad[0]), _ptr(rois), _ptr(out_data[1]),
                       _ptr(in_grad[0]), _ptr(in_grad[1]), _req(req[0]), _req(req[1]), B, C, H, W,
                       rois.shape[0], self.ph, self.pw, float(self.scale), None)
            _sync()

    class ROIPoolingV1Prop(Prop):
        ARGS = ("data", "rois")
        OUTS = ("output", "maxidx")
        num_visible_outputs = 1
        OP, OP_ARGS = ROIPoolingV1, ("pooled_size", "spatial_scale")
        DEPS = ((OUT_GRAD, 0), (IN_DATA, 1), (OUT_DATA, 1))

        def __init__(self, pooled_size, spatial_scale):
            super().__init__(need_top_grad=True)
            self.pooled_size = _tuple(pooled_size, 2, int)
            self.spatial_scale = float(spatial_scale)

        def infer_shape(self, in_shape):
            d, b = in_shape
            if len(d) != 4:
                raise ValueError("data should be a 4D tensor")
            if len(b) != 2 or b[1] != 5:
                raise ValueError("bbox should be a 2D tensor of shape [batch, 5]")
            o = (b[0], d[1], self.pooled_size[0], self.pooled_size[1])
            return [d, b], [o, o]

    ops["ROIPooling_v1"] = (ROIPoolingV1Prop, (None, "ROIPooling_v1"))

    # ---- assign_layer_fpn (models/FPN/assign_layer_fpn.py): 1 input, len(rcnn_stride) outputs ----
    class AssignLayerFPN(CustomOp):
        def __init__(self, strides, scale0, lvl0):
            super().__init__()
            self.strides, self.scale0, self.lvl0 = strides, scale0, lvl0

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            rois = in_data[0]
            _wait(rois)
            n = 1
            for s in rois.shape[:-1]:
                n *= int(s)
            mx_ = _state["mx"]
            per = mx_.nd.empty((len(self.strides),) + tuple(rois.shape), ctx=rois.context)
            _call("sd_fpn_roi_assign", _ptr(rois), n, _iarr(self.strides), len(self.strides),
                       float(self.scale0), float(self.lvl0), _ptr(per), None, None)
            _sync()
            for i in range(len(self.strides)):
                self.assign(out_data[i], req[i], per[i])

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            self.assign(in_grad[0], req[0], 0)

    class AssignLayerFPNProp(Prop):
        ARGS = ("rois",)
        OP, OP_ARGS = AssignLayerFPN, ("rcnn_stride", "roi_canonical_scale", "roi_canonical_level")

        def __init__(self, rcnn_stride, roi_canonical_scale, roi_canonical_level):
            super().__init__(need_top_grad=False)
            self.rcnn_stride = _tuple(rcnn_stride, typ=int)
            self.roi_canonical_scale = int(roi_canonical_scale)
            self.roi_canonical_level = int(roi_canonical_level)

        def list_outputs(self):
            return ["rois_s{}".format(s) for s in self.rcnn_stride]

        def infer_shape(self, in_shape):
            return [in_shape[0]], [in_shape[0]] * len(self.rcnn_stride)

    ops["assign_layer_fpn"] = (AssignLayerFPNProp, None)

    def _fpn_packed(pooled):
        return tuple(pooled) in ((7, 7), (14, 14))

    # ---- fpn_roi_align: the whole FPNRoiAlign.get_roi_feature subgraph (models/FPN/builder.py:
    #      567-610: assign -> per level ROIAlign_v2 -> add_n) as ONE op: feats..., rois -> output ----
    class FPNRoIAlign(CustomOp):
        """outputs: output, then the op's private forward -> backward state.  7x7 / 14x14 pooling:
        one-byte arg-max + the per-RoI coordinate / tap table (sd_fpn_roi_align_fwd_packed);
        other sizes: the reference's two fp32 arg-max planes."""

        def __init__(self, strides, pooled, scale0, lvl0, fp16=False):
            super().__init__()
            self.strides, self.pooled, self.scale0, self.lvl0 = strides, pooled, scale0, lvl0
            self.packed = _fpn_packed(pooled)
            self.fp16 = fp16  # fp16 feature maps in, fp16 output out (packed pooling sizes only)

        def _levels(self, feats):
            ptrs = (ctypes.c_void_p * len(feats))(*[_ptr(f).value for f in feats])
            return ptrs, _iarr([f.shape[2] for f in feats]), _iarr([f.shape[3] for f in feats])

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            feats, rois = in_data[:-1], in_data[-1]
            _wait(*in_data)
            B, C = feats[0].shape[:2]
            ptrs, Hs, Ws = self._levels(feats)
            ws, wsp, wsn = _ws(rois, "sd_fpn_roi_align_workspace_bytes", B, rois.shape[1])
            fn = "sd_fpn_roi_align_fwd_packed" if self.packed else "sd_fpn_roi_align_fwd"

            def run(name, level_ptrs, out0):
                _call(name, level_ptrs, Hs, Ws, _iarr(self.strides), len(feats), _ptr(rois),
                           _ptr(out0), _ptr(out_data[1]), _ptr(out_data[2]), B, C, rois.shape[1],
                           self.pooled[0], self.pooled[1], float(self.scale0), float(self.lvl0),
                           wsp, wsn, None)

            if not self.fp16 and self.packed and is_train:
                # training: ONE rois-only pre-pass for the step -- the backward's band lists / tap
                # tables are built here, into the op's fourth (private) output
                plan = out_data[3]
                _call(fn + "_plan", ptrs, Hs, Ws, _iarr(self.strides), len(feats), _ptr(rois),
                           _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), B, C, rois.shape[1],
                           self.pooled[0], self.pooled[1], float(self.scale0), float(self.lvl0),
                           wsp, wsn, _ptr(plan), ctypes.c_size_t(plan.size), None)
                self._planned = True
            elif not self.fp16:
                self._planned = False
                run(fn, ptrs, out_data[0])
            else:
                try:
                    run(fn + "_f16", ptrs, out_data[0])
                except SimpleDetOpsError as e:
                    if e.code != SD_ERR_UNSUPPORTED:
                        raise
                    # a shape the band-resident kernel does not take: the casts the reference graph
                    # carries itself (models/FPN/builder.py:581-586, 607-608) around the fp32 op
                    f32 = [_scratch(rois, f.size * 4).reshape(f.shape) for f in feats]
                    for f, g in zip(feats, f32):
                        _call("sd_cast_f16_to_f32", _ptr(f), _ptr(g), ctypes.c_size_t(f.size), None)
                    o32 = _scratch(rois, out_data[0].size * 4).reshape(out_data[0].shape)
                    p32 = (ctypes.c_void_p * len(f32))(*[_ptr(g).value for g in f32])
                    run(fn, p32, o32)
                    _call("sd_cast_f32_to_f16", _ptr(o32), _ptr(out_data[0]),
                               ctypes.c_size_t(o32.size), REQ["write"], None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            feats, rois = in_data[:-1], in_data[-1]
            _wait(out_grad[0], rois, *out_data[1:])
            rq = {_req(r) for r in req[:-1]}
            if len(rq) != 1:
                raise RuntimeError("fpn_roi_align: all feature gradients must share one req")
            B, C = feats[0].shape[:2]
            req_data = rq.pop()
            og, grads16 = out_grad[0], None
            if self.fp16 and self.packed:
                # the backward kernel's fp16-I/O instance: the graph's to_fp32 / to_fp16 casts
                # (models/FPN/builder.py:581-586, 607-608) happen inside the kernel
                ptrs16, Hs16, Ws16 = self._levels(in_grad[:-1])
                ws, wsp, wsn = _ws(rois, "sd_fpn_roi_align_bwd_workspace_bytes", Hs16, Ws16, len(feats), B,
                                         rois.shape[1])
                try:
                    _call("sd_fpn_roi_align_bwd_packed_f16", _ptr(out_grad[0]), _ptr(rois), _ptr(out_data[1]),
                               _ptr(out_data[2]), ptrs16, Hs16, Ws16, _iarr(self.strides), len(feats), req_data,
                               B, C, rois.shape[1], self.pooled[0], self.pooled[1], float(self.scale0),
                               float(self.lvl0), wsp, wsn, None)
                    _sync()
                    self.assign(in_grad[-1], req[-1], 0)
                    return
                except SimpleDetOpsError as e:
                    if e.code != SD_ERR_UNSUPPORTED:
                        raise
            if self.fp16:
                # the sums are formed by the fp32 kernel: the graph's to_fp32 / to_fp16 casts
                # (models/FPN/builder.py:581-586, 607-608) happen here, at the op boundary
                og = _scratch(rois, out_grad[0].size * 4).reshape(out_grad[0].shape)
                _call("sd_cast_f16_to_f32", _ptr(out_grad[0]), _ptr(og), ctypes.c_size_t(out_grad[0].size), None)
                grads16 = in_grad[:-1]
                in_grad = [_scratch(rois, g.size * 4).reshape(g.shape) for g in grads16] + [in_grad[-1]]
                rq = {REQ["write"]}
            else:
                rq = {req_data}
            ptrs, Hs, Ws = self._levels(in_grad[:-1])
            out_grad = [og]
            if self.packed and not self.fp16 and getattr(self, "_planned", False):
                plan = out_data[3]   # lists / tap tables left by this op's forward
                _call("sd_fpn_roi_align_bwd_packed_plan", _ptr(out_grad[0]), _ptr(rois), _ptr(out_data[1]),
                           _ptr(out_data[2]), ptrs, Hs, Ws, _iarr(self.strides), len(feats), rq.pop(), B, C,
                           rois.shape[1], self.pooled[0], self.pooled[1], float(self.scale0),
                           float(self.lvl0), _ptr(plan), ctypes.c_size_t(plan.size), None)
            elif self.packed:  # with the workspace the per-band RoI lists are built once, not per channel
                ws, wsp, wsn = _ws(rois, "sd_fpn_roi_align_bwd_workspace_bytes", Hs, Ws, len(feats), B, rois.shape[1])
                _call("sd_fpn_roi_align_bwd_packed_ws", _ptr(out_grad[0]), _ptr(rois), _ptr(out_data[1]),
                           _ptr(out_data[2]), ptrs, Hs, Ws, _iarr(self.strides), len(feats), rq.pop(), B, C,
                           rois.shape[1], self.pooled[0], self.pooled[1], float(self.scale0),
                           float(self.lvl0), wsp, wsn, None)
            else:
                _call("sd_fpn_roi_align_bwd", _ptr(out_grad[0]), _ptr(rois), _ptr(out_data[1]),
                           _ptr(out_data[2]), ptrs, Hs, Ws, _iarr(self.strides), len(feats), rq.pop(), B, C,
                           rois.shape[1], self.pooled[0], self.pooled[1], float(self.scale0),
                           float(self.lvl0), None)
            if self.fp16:
                for g32, g16 in zip(in_grad[:-1], grads16):
                    _call("sd_cast_f32_to_f16", _ptr(g32), _ptr(g16), ctypes.c_size_t(g16.size), req_data, None)
            _sync()
            self.assign(in_grad[-1], req[-1], 0)

    class FPNRoIAlignProp(Prop):
        num_visible_outputs = 1
        OP, OP_ARGS = FPNRoIAlign, ("rcnn_stride", "pooled_size", "scale0", "lvl0", "fp16")

        def __init__(self, rcnn_stride, pooled_size="(7, 7)", roi_canonical_scale="224",
                     roi_canonical_level="4", fp16="False"):
            super().__init__(need_top_grad=True)
            self.rcnn_stride = _tuple(rcnn_stride, typ=int)
            self.pooled_size = _tuple(pooled_size, 2, int)
            self.scale0, self.lvl0 = float(roi_canonical_scale), float(roi_canonical_level)
            self.packed = _fpn_packed(self.pooled_size)
            self.fp16 = _bool(fp16)
            if self.fp16 and not self.packed:
                raise ValueError("fpn_roi_align: fp16 I/O is provided for 7x7 and 14x14 pooling")

        def list_arguments(self):
            return ["data_s{}".format(s) for s in self.rcnn_stride] + ["rois"]

        def list_outputs(self):
            # packed: output, then private forward -> backward state (arg-max codes, coordinate table,
            # the backward's band lists / tap tables built by the forward's pre-pass)
            return ["output", "argmax", "coords", "plan"] if self.packed else ["output", "maxidx_x", "maxidx_y"]

        def infer_shape(self, in_shape):
            feats, b = in_shape[:-1], in_shape[-1]
            if len(b) != 3 or b[2] != 4:
                raise ValueError("bbox should be a 3D tensor of shape [batch, rois, 4]")
            o = (b[0], b[1], feats[0][1], self.pooled_size[0], self.pooled_size[1])
            if self.packed:
                stride = int(lib().cdll.sd_fpn_roi_align_argmax_stride(*self.pooled_size))
                pb = int(lib().cdll.sd_fpn_roi_align_plan_bytes(_iarr([f[2] for f in feats]),
                                                                _iarr([f[3] for f in feats]), len(feats),
                                                                int(b[0]), int(b[1])))
                return in_shape, [o, (b[0], b[1], feats[0][1], stride),
                                  (b[0], b[1], 9 * (self.pooled_size[0] + self.pooled_size[1])),
                                  ((pb + 15) // 16 * 16,)]
            return in_shape, [o, o, o]

        def infer_type(self, in_type):
            import numpy as np
            f32 = np.float32
            if self.fp16:  # feature maps fp16, rois fp32 -> output fp16; the state keeps its types
                return [np.float16] * (len(in_type) - 1) + [f32], [np.float16, np.uint8, f32, np.uint8], []
            if self.packed:
                return in_type, [f32, np.uint8, f32, np.uint8], []
            return in_type, [f32, f32, f32], []

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return [out_grad[0], in_data[-1]] + list(out_data[1:])

    ops["fpn_roi_align"] = (FPNRoIAlignProp, None)

    def _dpsroi_supported(ncls, pooled, samples):
        """the set forward AND backward take: the library's predicate, not a copy of its limits"""
        if min(ncls, pooled, samples) < 1 or max(ncls, pooled, samples) > 4096:
            return False
        return bool(lib().cdll.sd_deform_psroi_pool_supported(int(ncls), int(pooled), int(samples)))

    # ---- _contrib_DeformablePSROIPooling (upstream MXNet; models/TSD/poolings.py:87-100, 151-164):
    #      data, rois[, trans] -> output, top_count (1 visible) ----
    class DeformablePSROIPooling(Op):
        def _tail(self, data, rois, trans):
            g = self.g
            B, C, H, W = data.shape
            ncls = 1 if g["no_trans"] else trans.shape[1] // 2
            return (B, C, H, W, rois.shape[0], ncls, float(g["spatial_scale"]), g["output_dim"], g["group_size"],
                    g["pooled_size"], g["part_size"], g["sample_per_part"], float(g["trans_std"]), int(g["no_trans"]),
                    None)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            data, rois = in_data[:2]
            trans = None if self.g["no_trans"] else in_data[2]
            _wait(*in_data)
            _call("sd_deform_psroi_pool_fwd", _ptr(data), _ptr(rois), _ptr(trans), _ptr(out_data[0]),
                  _ptr(out_data[1]), *self._tail(data, rois, trans))
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            data, rois = in_data[:2]
            no_trans = self.g["no_trans"]
            trans = None if no_trans else in_data[2]
            _wait(out_grad[0], out_data[1], *in_data)
            _call("sd_deform_psroi_pool_bwd", _ptr(out_grad[0]), _ptr(data), _ptr(rois), _ptr(trans),
                  _ptr(out_data[1]), _ptr(in_grad[0]), _ptr(in_grad[1]), None if no_trans else _ptr(in_grad[2]),
                  _req(req[0]), _req(req[1]), REQ["null"] if no_trans else _req(req[2]),
                  *self._tail(data, rois, trans))
            _sync()

    class DeformablePSROIPoolingProp(Prop):
        OUTS = ("output", "top_count")
        num_visible_outputs = 1
        OP = DeformablePSROIPooling
        PARAMS = ("spatial_scale", "output_dim", "group_size", "pooled_size", "part_size", "sample_per_part",
                  "trans_std", "no_trans")

        def __init__(self, spatial_scale, output_dim, group_size, pooled_size, part_size="0", sample_per_part="1",
                     trans_std="0.0", no_trans="False"):
            super().__init__(need_top_grad=True)
            params = dict(spatial_scale=spatial_scale, output_dim=output_dim, group_size=group_size,
                          pooled_size=pooled_size, part_size=part_size, sample_per_part=sample_per_part,
                          trans_std=trans_std, no_trans=no_trans)
            why = self.sd_supports({k: str(v) for k, v in params.items()})
            if why:
                raise ValueError("DeformablePSROIPooling: " + why)
            self.g = dict(spatial_scale=float(spatial_scale), output_dim=int(output_dim), group_size=int(group_size),
                          pooled_size=int(pooled_size), part_size=int(part_size), sample_per_part=int(sample_per_part),
                          trans_std=float(trans_std), no_trans=_bool(no_trans))

        @classmethod
        def sd_supports(cls, params):
            """'' when the kernels take this parameter set, else the reason (install()'s alias then falls back to
            the native constructor)."""
            for k in params:
                if k not in cls.PARAMS:
                    return "parameter %r is not one this operator takes" % k
            try:
                float(params["spatial_scale"])
                float(params.get("trans_std", "0.0"))
                od, G, P = int(params["output_dim"]), int(params["group_size"]), int(params["pooled_size"])
                part, S = int(params.get("part_size", "0")), int(params.get("sample_per_part", "1"))
            except Exception as e:
                return "missing or unparsable parameter (%s)" % e
            if od < 1 or G < 1 or P < 1 or S < 1 or part < 0:
                return "output_dim, group_size, pooled_size, sample_per_part must be >= 1 and part_size >= 0"
            # the library's own predicate, here for ONE class: the class count is known only from the offsets' shape
            # (infer_shape asks again with it, and can only raise by then)
            if not _dpsroi_supported(1, P, S):
                return ("pooled_size %d with sample_per_part %d: the RoI's tap table and the backward's sums do not "
                        "fit in LDS (sd_deform_psroi_pool_supported)" % (P, S))
            return ""

        def list_arguments(self):
            return ["data", "rois"] if self.g["no_trans"] else ["data", "rois", "trans"]

        def infer_shape(self, in_shape):
            g = self.g
            d, b = in_shape[:2]
            if len(d) != 4:
                raise ValueError("data should be a 4D tensor")
            if len(b) != 2 or b[1] != 5:
                raise ValueError("bbox should be a 2D tensor of shape [batch, 5]")
            if d[1] != g["output_dim"] * g["group_size"] ** 2:
                raise ValueError("data has %d channels, output_dim * group_size^2 = %d"
                                 % (d[1], g["output_dim"] * g["group_size"] ** 2))
            if not g["no_trans"]:
                t = in_shape[2]
                part = g["part_size"] or g["pooled_size"]
                if len(t) != 4 or t[0] != b[0] or t[1] % 2 or t[1] < 2 or tuple(t[2:]) != (part, part):
                    raise ValueError("trans should have shape (rois, 2 * num_classes, %d, %d)" % (part, part))
                if g["output_dim"] % (t[1] // 2):
                    raise ValueError("output_dim is not a multiple of num_classes")
                if not _dpsroi_supported(t[1] // 2, g["pooled_size"], g["sample_per_part"]):
                    raise ValueError("DeformablePSROIPooling: %d classes with pooled_size %d and sample_per_part %d do "
                                     "not fit the kernels' LDS (sd_deform_psroi_pool_supported)"
                                     % (t[1] // 2, g["pooled_size"], g["sample_per_part"]))
            o = (b[0], g["output_dim"], g["pooled_size"], g["pooled_size"])
            return list(in_shape), [o, o]

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return [out_grad[0]] + list(in_data) + [out_data[1]]

    ops["_contrib_DeformablePSROIPooling"] = (DeformablePSROIPoolingProp, ("contrib", "DeformablePSROIPooling"))

    # ---- fpn_deform_roi_pool: the whole FPNRoIAlign_DeltaC / DeltaR.get_roi_feature subgraph
    #      (models/TSD/poolings.py:51-174: fpn_roi_assign_offset -> per level DeformablePSROIPooling on masked
    #      rois / offsets -> add_n) as ONE op: feats..., rois (B,R,4), trans (B*R,2,P,P) | (B*R,2) -> output ----
    class FPNDeformRoIPool(Op):
        def _levels(self, feats):
            ptrs = (ctypes.c_void_p * len(feats))(*[_ptr(f).value for f in feats])
            return ptrs, _iarr([f.shape[2] for f in feats]), _iarr([f.shape[3] for f in feats])

        def _tail(self, feats, rois, trans):
            g = self.g
            B, C = feats[0].shape[:2]
            return (B, C, rois.shape[1], g["pooled_size"], g["pooled_size"] if len(trans.shape) == 4 else 1,
                    g["sample_per_part"], float(g["trans_std"]), float(g["scale0"]), float(g["lvl0"]), None)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            feats, rois, trans = in_data[:-2], in_data[-2], in_data[-1]
            _wait(*in_data)
            ptrs, Hs, Ws = self._levels(feats)
            _call("sd_fpn_deform_roi_pool_fwd", ptrs, Hs, Ws, _iarr(self.g["stride"]), len(feats), _ptr(rois),
                  _ptr(trans), _ptr(out_data[0]), _ptr(out_data[1]), *self._tail(feats, rois, trans))
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            feats, rois, trans = in_data[:-2], in_data[-2], in_data[-1]
            _wait(out_grad[0], out_data[1], *in_data)
            rq = {_req(r) for r in req[:-2]}
            if len(rq) != 1:
                raise RuntimeError("fpn_deform_roi_pool: all feature gradients must share one req")
            ptrs, Hs, Ws = self._levels(feats)
            dptrs = self._levels(in_grad[:-2])[0]
            _call("sd_fpn_deform_roi_pool_bwd", _ptr(out_grad[0]), ptrs, dptrs, Hs, Ws, _iarr(self.g["stride"]),
                  len(feats), _ptr(rois), _ptr(trans), _ptr(out_data[1]), _ptr(in_grad[-1]), rq.pop(),
                  _req(req[-1]), *self._tail(feats, rois, trans))
            _sync()
            self.assign(in_grad[-2], req[-2], 0)

    class FPNDeformRoIPoolProp(Prop):
        OUTS = ("output", "top_count")
        num_visible_outputs = 1
        OP = FPNDeformRoIPool

        def __init__(self, rcnn_stride, pooled_size="7", sample_per_part="4", trans_std="0.1",
                     roi_canonical_scale="224", roi_canonical_level="4"):
            super().__init__(need_top_grad=True)
            self.g = dict(stride=_tuple(rcnn_stride, typ=int), pooled_size=int(pooled_size),
                          sample_per_part=int(sample_per_part), trans_std=float(trans_std),
                          scale0=float(roi_canonical_scale), lvl0=float(roi_canonical_level))
            g = self.g
            if not 1 <= len(g["stride"]) <= 5:
                raise ValueError("fpn_deform_roi_pool: 1 to 5 levels, got %d" % len(g["stride"]))
            if not _dpsroi_supported(1, g["pooled_size"], g["sample_per_part"]):
                raise ValueError("fpn_deform_roi_pool: pooled_size %d with sample_per_part %d does not fit the kernels' "
                                 "LDS (sd_deform_psroi_pool_supported)" % (g["pooled_size"], g["sample_per_part"]))

        def list_arguments(self):
            return ["data_s{}".format(s) for s in self.g["stride"]] + ["rois", "trans"]

        def infer_shape(self, in_shape):
            feats, b, t = in_shape[:-2], in_shape[-2], in_shape[-1]
            P = self.g["pooled_size"]
            if len(feats) != len(self.g["stride"]):
                raise ValueError("one feature map per stride expected")
            if len(b) != 3 or b[2] != 4:
                raise ValueError("bbox should be a 3D tensor of shape [batch, rois, 4]")
            n = b[0] * b[1]
            if tuple(t) not in ((n, 2, P, P), (n, 2)):
                raise ValueError("trans should have shape (%d, 2, %d, %d) or (%d, 2), got %s" % (n, P, P, n, tuple(t)))
            for f in feats:
                if len(f) != 4 or tuple(f[:2]) != (b[0], feats[0][1]):
                    raise ValueError("every level should be (batch, C, H, W)")
            return list(in_shape), [(n, feats[0][1], P, P), (n, len(feats), P, P)]

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return [out_grad[0]] + list(in_data) + [out_data[1]]

    ops["fpn_deform_roi_pool"] = (FPNDeformRoIPoolProp, None)
    return ops


def _target_ops(mx):
    """ProposalTarget, ProposalTarget_v2, ProposalMaskTarget"""
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)
    ops = {}

    def target_param(p):
        """the C ABI's ProposalTargetParam from a prop's parsed parameters"""
        from .ops import ProposalTargetParam
        cp = ProposalTargetParam()
        cp.num_classes, cp.batch_images, cp.image_rois = p["num_classes"], p["batch_images"], p["image_rois"]
        cp.fg_fraction, cp.fg_thresh = p["fg_fraction"], p["fg_thresh"]
        cp.bg_thresh_hi, cp.bg_thresh_lo = p["bg_thresh_hi"], p["bg_thresh_lo"]
        cp.proposal_without_gt, cp.class_agnostic = int(p["proposal_without_gt"]), int(p["class_agnostic"])
        for i in range(4):
            cp.bbox_mean[i], cp.bbox_std[i], cp.bbox_weight[i] = (p["bbox_mean"][i], p["bbox_std"][i],
                                                                   p["bbox_weight"][i])
        return cp

    def rand_state(context):
        """libc's global rand() state of a process that never called srand (seed 1): one stream per device,
        shared by every ProposalTarget / ProposalMaskTarget node like the libc global is"""
        key = str(context)
        if key not in _state["rng"]:
            host = (ctypes.c_int32 * 33)()
            _call("sd_glibc_srand_host", ctypes.c_uint32(1), host)
            _state["rng"][key] = _state["mx"].nd.array(list(host), ctx=context, dtype="int32")
        return _state["rng"][key]

    # ---- ProposalTarget: 2 inputs, 5 outputs (4 visible unless output_iou) ----
    class ProposalTarget(CustomOp):
        def __init__(self, p):
            super().__init__()
            self.p = p

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _require_write(req[:4], ["roi_output", "label", "bbox_target", "bbox_weight"])
            rois, gt = in_data[0], in_data[1]
            vr = in_data[2] if len(in_data) > 2 else None  # ProposalTarget_v2: valid_ranges
            _wait(*in_data)
            p = self.p
            B = p["batch_images"]
            N = int(_numel(rois.shape) // (B * 4))
            M = int(_numel(gt.shape) // (B * 5))
            cp, rng = target_param(p), rand_state(rois.context)
            ws, wsp, wsn = _ws(rois, "sd_proposal_target_workspace_bytes", B, N, M)
            if vr is not None:
                _call("sd_proposal_target_v2", _ptr(rois), _ptr(gt), _ptr(vr),
                           int(p.get("filter_scales", False)), N, M, ctypes.byref(cp), _ptr(rng),
                           _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), _ptr(out_data[3]),
                           _ptr(out_data[4]), None, wsp, wsn, None)
            else:
                _call("sd_proposal_target", _ptr(rois), _ptr(gt), N, M, ctypes.byref(cp), _ptr(rng),
                           _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), _ptr(out_data[3]),
                           _ptr(out_data[4]), None, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # proposal_target-inl.h:272-276 / proposal_target_v2-inl.h:298-311: input gradients are zero
            for i in range(len(in_grad)):
                self.assign(in_grad[i], req[i], 0)

    class ProposalTargetProp(Prop):
        ARGS = ("rois", "gt_boxes")
        OUTS = ("roi_output", "label", "bbox_target", "bbox_weight", "match_gt_iou")
        OP, OP_ARGS = ProposalTarget, ("p",)

        def __init__(self, num_classes, batch_images, image_rois, fg_thresh, bg_thresh_hi,
                     bg_thresh_lo, fg_fraction="0.25", proposal_without_gt="False",
                     class_agnostic="False", output_iou="False", bbox_mean="(0,0,0,0)",
                     bbox_std="(0.1,0.1,0.2,0.2)", bbox_weight="(1,1,1,1)"):
            super().__init__(need_top_grad=False)
            self.p = dict(num_classes=int(num_classes), batch_images=int(batch_images),
                          image_rois=int(image_rois), fg_thresh=float(fg_thresh),
                          bg_thresh_hi=float(bg_thresh_hi), bg_thresh_lo=float(bg_thresh_lo),
                          fg_fraction=float(fg_fraction),
                          proposal_without_gt=_bool(proposal_without_gt),
                          class_agnostic=_bool(class_agnostic), output_iou=_bool(output_iou),
                          bbox_mean=_tuple(bbox_mean, 4), bbox_std=_tuple(bbox_std, 4),
                          bbox_weight=_tuple(bbox_weight, 4))
            self.num_visible_outputs = 5 if self.p["output_iou"] else 4

        def infer_shape(self, in_shape):
            p = self.p
            B, S, K = p["batch_images"], p["image_rois"], p["num_classes"]
            return in_shape, [(B, S, 4), (B, S), (B, S, K * 4), (B, S, K * 4), (B, S)]

    ops["ProposalTarget"] = (ProposalTargetProp, (None, "ProposalTarget"))

    # ---- ProposalTarget_v2 (proposal_target_v2-inl.h): + valid_ranges input, filter_scales ----
    class ProposalTargetV2Prop(ProposalTargetProp):
        ARGS = ("rois", "gt_boxes", "valid_ranges")

        def __init__(self, num_classes, batch_images, image_rois, fg_thresh, bg_thresh_hi,
                     bg_thresh_lo, proposal_without_gt, fg_fraction="0.25", class_agnostic="False",
                     ohem="False", output_iou="False", bbox_mean="(0,0,0,0)",
                     bbox_std="(0.1,0.1,0.2,0.2)", bbox_weight="(1,1,1,1)", filter_scales="False"):
            super().__init__(num_classes, batch_images, image_rois, fg_thresh, bg_thresh_hi,
                             bg_thresh_lo, fg_fraction, proposal_without_gt, class_agnostic,
                             output_iou, bbox_mean, bbox_std, bbox_weight)
            if _bool(ohem):
                raise ValueError("ProposalTarget_v2: OHEM not Implemented.")  # as the reference (:216-217)
            if self.p["image_rois"] < 0:
                raise ValueError("ProposalTarget_v2: image_rois=-1 is undefined in the reference")
            self.p["filter_scales"] = _bool(filter_scales)

    ops["ProposalTarget_v2"] = (ProposalTargetV2Prop, (None, "ProposalTarget_v2"))

    # ---- ProposalMaskTarget (proposal_mask_target-inl.h): rois, gt_boxes, gt_polys [, valid_ranges]
    #      -> the five ProposalTarget outputs + mask_target (+ mask_ratio with output_ratio) ----
    class ProposalMaskTarget(CustomOp):
        def __init__(self, p):
            super().__init__()
            self.p = p

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _require_write(req[:6], ["roi_output", "label", "bbox_target", "bbox_weight", "match_gt_iou",
                                     "mask_target"])
            rois, gt, polys = in_data[0], in_data[1], in_data[2]
            vr = in_data[3] if len(in_data) > 3 else None
            _wait(*in_data)
            p = self.p
            B = p["batch_images"]
            N = int(_numel(rois.shape) // (B * 4))
            M = int(_numel(gt.shape) // (B * 5))
            L = int(polys.shape[2])
            cp, rng = target_param(p), rand_state(rois.context)
            if p["output_ratio"]:  # proposal_mask_target-inl.h:159-161: the seventh output, kWriteTo
                _require_write(req[6:7], ["mask_ratio"])
                mp = p["max_raster_pixels"]
                ws, wsp, wsn = _ws(rois, "sd_proposal_mask_target_ratio_workspace_bytes", B, N, M, p["image_rois"],
                                         ctypes.c_float(p["fg_fraction"]), mp)
                _call("sd_proposal_mask_target_ratio", _ptr(rois), _ptr(gt), _ptr(polys), _ptr(vr),
                           int(p["filter_scales"]), N, M, L, p["mask_size"], ctypes.byref(cp), _ptr(rng),
                           _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), _ptr(out_data[3]),
                           _ptr(out_data[4]), _ptr(out_data[5]), _ptr(out_data[6]), mp, None, wsp, wsn, None)
                _sync()
                return
            ws, wsp, wsn = _ws(rois, "sd_proposal_target_workspace_bytes", B, N, M)
            _call("sd_proposal_mask_target", _ptr(rois), _ptr(gt), _ptr(polys), _ptr(vr),
                       int(p["filter_scales"]), N, M, L, p["mask_size"], ctypes.byref(cp), _ptr(rng),
                       _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), _ptr(out_data[3]),
                       _ptr(out_data[4]), _ptr(out_data[5]), None, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(in_grad)):
                self.assign(in_grad[i], req[i], 0)

    class ProposalMaskTargetProp(ProposalTargetProp):
        OP, OP_ARGS = ProposalMaskTarget, ("p",)

        def __init__(self, num_classes, batch_images, image_rois, mask_size, fg_thresh,
                     bg_thresh_hi, bg_thresh_lo, proposal_without_gt, fg_fraction="0.25",
                     class_agnostic="False", ohem="False", output_ratio="False", output_iou="False",
                     filter_scales="False", bbox_mean="(0,0,0,0)", bbox_std="(0.1,0.1,0.2,0.2)",
                     bbox_weight="(1,1,1,1)", num_args=None, max_raster_pixels="1982464"):
            # num_args is the reference op's key_var_num_args (proposal_mask_target.cc:485): MXNet's
            # front end fills it in from the number of symbol inputs and no call site passes it
            # (models/maskrcnn/builder.py:115,184), so it defaults to what filter_scales implies
            super().__init__(num_classes, batch_images, image_rois, fg_thresh, bg_thresh_hi,
                             bg_thresh_lo, fg_fraction, proposal_without_gt, class_agnostic,
                             output_iou, bbox_mean, bbox_std, bbox_weight)
            if _bool(ohem):
                raise ValueError("ProposalMaskTarget: OHEM not Implemented.")
            # output_ratio (mask scoring R-CNN, models/msrcnn/builder.py:219-237): the seventh output.
            # max_raster_pixels is this adapter's own attribute (not the reference's): the bound on
            # the image-resolution rasters the ratio counts, default 1408 x 1408
            self.p["output_ratio"] = _bool(output_ratio)
            self.p["max_raster_pixels"] = int(max_raster_pixels)
            if self.p["image_rois"] < 0:
                raise ValueError("ProposalMaskTarget: image_rois=-1 is undefined in the reference")
            self.p["filter_scales"] = _bool(filter_scales)
            self.p["mask_size"] = int(mask_size)
            want = 4 if self.p["filter_scales"] else 3
            self.num_args = want if num_args is None else int(num_args)
            if self.num_args != want:
                raise ValueError("num_args=%d but filter_scales=%s takes %d inputs"
                                 % (self.num_args, self.p["filter_scales"], want))
            # proposal_mask_target-inl.h:387-409 (the graph unpacks match_gt_iou either way:
            # models/maskrcnn/builder.py:115, models/msrcnn/builder.py:219)
            self.num_visible_outputs = 7 if self.p["output_ratio"] else 6

        def list_arguments(self):
            base = ["rois", "gt_boxes", "gt_polys"]
            return base + ["valid_ranges"] if self.p["filter_scales"] else base

        def list_outputs(self):
            base = ["roi_output", "label", "bbox_target", "bbox_weight", "match_gt_iou", "mask_target"]
            return base + ["mask_ratio"] if self.p["output_ratio"] else base

        def infer_shape(self, in_shape):
            p = self.p
            B, S, K = p["batch_images"], p["image_rois"], p["num_classes"]
            import numpy as np
            FG = int(np.float32(S) * np.float32(p["fg_fraction"]))
            out = [(B, S, 4), (B, S), (B, S, K * 4), (B, S, K * 4), (B, S),
                   (B, FG, p["mask_size"], p["mask_size"])]
            if p["output_ratio"]:
                out.append((B, FG))  # -inl.h:453-456
            return in_shape, out

    ops["ProposalMaskTarget"] = (ProposalMaskTargetProp, (None, "ProposalMaskTarget"))
    return ops


def _proposal_ops(mx):
    """anchors and proposals: GenAnchor, NMS, Proposal_v3 / _v2 / v1, GenProposalRetina, get_top_proposal, DecodeBBox,
    BboxPostProcessing"""
    CustomOp, Op, Prop = mx.operator.CustomOp, op_base(mx), prop_base(mx)
    ops = {}

    # ---- _contrib_GenAnchor: 1 input (shape only), 1 output ----
    class GenAnchor(CustomOp):
        def __init__(self, scales, ratios, stride):
            super().__init__()
            self.scales, self.ratios, self.stride = scales, ratios, stride

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _require_write(req[:1], ["output"])
            H, W = in_data[0].shape[2], in_data[0].shape[3]
            _call("sd_gen_anchor", _ptr(out_data[0]), H, W, self.stride, _darr(self.scales),
                       len(self.scales), _darr(self.ratios), len(self.ratios), None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            self.assign(in_grad[0], req[0], 0)

    class GenAnchorProp(Prop):
        ARGS = ("cls_prob",)
        OP, OP_ARGS = GenAnchor, ("scales", "ratios", "stride")

        def __init__(self, scales="(4,8,16,32)", ratios="(0.5,1,2)", feature_stride="16"):
            super().__init__(need_top_grad=False)
            self.scales, self.ratios = _tuple(scales), _tuple(ratios)
            self.stride = int(feature_stride)

        def infer_shape(self, in_shape):
            d = in_shape[0]
            if len(d) != 4:
                raise ValueError("cls_prob should be a 4D tensor")
            A = len(self.scales) * len(self.ratios)
            return in_shape, [(d[2] * d[3] * A, 4)]

    ops["_contrib_GenAnchor"] = (GenAnchorProp, ("contrib", "GenAnchor"))

    # ---- _contrib_NMS: 1 input, 2 outputs (score visible only with output_score) ----
    class NMS(CustomOp):
        def __init__(self, pre, post, thr, already_sorted):
            super().__init__()
            self.pre, self.post, self.thr, self.sorted = pre, post, thr, already_sorted

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            rois = in_data[0]
            _wait(rois)
            B, N, _ = rois.shape
            ws, wsp, wsn = _ws(rois, "sd_nms_workspace_bytes", B, N, self.pre)
            pre = min(self.pre if self.pre > 0 else N, N)
            if self.post > pre:
                # NMSProp::InferShape always declares (B, post, .) but the op writes min(post, pre)
                # rows per image, image i at row offset i*min(post, pre) of the flat buffer
                # (nms.cu:277,352-354), and never touches the tail.  Same bytes here; the tail
                # (uninitialised in the reference) is zeroed.
                self.assign(out_data[0], "write", 0)
                self.assign(out_data[1], "write", 0)
            _call("sd_nms", _ptr(rois), B, N, self.pre, self.post, float(self.thr), 0,
                       int(self.sorted), _ptr(out_data[0]), _ptr(out_data[1]), None, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            self.assign(in_grad[0], req[0], 0)  # nms.cu:379-381

    class NMSProp(Prop):
        ARGS = ("rois",)
        OUTS = ("output", "score")
        OP, OP_ARGS = NMS, ("pre", "post", "thr", "sorted")

        def __init__(self, rpn_pre_nms_top_n="6000", rpn_post_nms_top_n="300", threshold="0.7",
                     output_score="False", already_sorted="False", workspace="256"):
            super().__init__(need_top_grad=False)
            self.pre, self.post = int(rpn_pre_nms_top_n), int(rpn_post_nms_top_n)
            self.thr = float(threshold)
            self.sorted = _bool(already_sorted)
            self.num_visible_outputs = 2 if _bool(output_score) else 1

        def infer_shape(self, in_shape):
            d = in_shape[0]
            if len(d) != 3 or d[2] != 5:
                raise ValueError("Input:[bbox] must be (batch, rois, 5)")
            return in_shape, [(d[0], self.post, 4), (d[0], self.post, 1)]

    ops["_contrib_NMS"] = (NMSProp, ("contrib", "NMS"))

    # ---- _contrib_Proposal_v3: cls_prob, bbox_pred, im_info -> output [, score] ----
    class ProposalV3(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            cls_prob, bbox_pred, im_info = in_data
            _wait(cls_prob, bbox_pred, im_info)
            g = self.g
            B, A2, H, W = cls_prob.shape
            A = A2 // 2
            ws, wsp, wsn = _ws(cls_prob, "sd_proposal_v3_workspace_bytes", B, A, H, W, g["pre"])
            count = A * H * W
            pre = min(g["pre"] if g["pre"] > 0 else count, count)
            if g["is_train"] and g["post"] > pre:
                # same quirk as _contrib_NMS (proposal_v3.cu:474-479,626-632): declared
                # (B, post, .), written min(post, pre) rows per image, packed; tail zeroed here
                self.assign(out_data[0], "write", 0)
                self.assign(out_data[1], "write", 0)
            fa = lambda v: (ctypes.c_float * len(v))(*v)
            _call("sd_proposal_v3_iou" if g["iou_loss"] else "sd_proposal_v3",
                       _ptr(cls_prob), _ptr(bbox_pred), _ptr(im_info),
                       _ptr(out_data[0]), _ptr(out_data[1]), B, A, H, W, g["pre"], g["post"],
                       float(g["thr"]), g["min_size"], fa(g["scales"]), len(g["scales"]),
                       fa(g["ratios"]), len(g["ratios"]), g["stride"], int(g["is_train"]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(3):
                self.assign(in_grad[i], req[i], 0)

    class ProposalV3Prop(Prop):
        ARGS = ("cls_prob", "bbox_pred", "im_info")
        OUTS = ("output", "score")
        OP = ProposalV3

        def __init__(self, rpn_pre_nms_top_n="6000", rpn_post_nms_top_n="300", threshold="0.7",
                     rpn_min_size="16", scales="(4,8,16,32)", ratios="(0.5,1,2)",
                     feature_stride="16", output_score="False", iou_loss="False", is_train="False",
                     workspace="256"):
            super().__init__(need_top_grad=False)
            self.g = dict(pre=int(rpn_pre_nms_top_n), post=int(rpn_post_nms_top_n),
                          thr=float(threshold), min_size=int(rpn_min_size), scales=_tuple(scales),
                          ratios=_tuple(ratios), stride=int(feature_stride),
                          is_train=_bool(is_train), iou_loss=_bool(iou_loss))  # proposal_v3.cu:536
            self.num_visible_outputs = 2 if _bool(output_score) else 1

        def infer_shape(self, in_shape):
            d = in_shape[0]
            if len(d) != 4:
                raise ValueError("cls_prob should be (batch, 2 * num_anchors, H, W)")
            g = self.g
            A = d[1] // 2
            if A != len(g["scales"]) * len(g["ratios"]):
                raise ValueError("num_anchors != len(ratios) * len(scales)")
            count = A * d[2] * d[3]
            post = g["post"]  # ProposalProp_v3::InferShape (proposal_v3-inl.h:199-218)
            return [d, (d[0], 4 * A, d[2], d[3]), (d[0], 3)], [(d[0], post, 4), (d[0], post, 1)]

    ops["_contrib_Proposal_v3"] = (ProposalV3Prop, ("contrib", "Proposal_v3"))

    # ---- _contrib_Proposal_v2 (cls_prob, bbox_pred, im_info, valid_ranges) and _contrib_Proposal
    #      (cls_prob, bbox_pred, im_info) -> output [, score]  (registered only by install(...,
    #      proposal=True)) ----
    class ProposalV12(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            g = self.g
            cls_prob, bbox_pred, im_info = in_data[:3]
            B, A2, H, W = cls_prob.shape
            A = A2 // 2
            fn = "sd_proposal_v2" if g["v2"] else "sd_proposal"
            ws, wsp, wsn = _ws(cls_prob, fn + "_workspace_bytes", B, A, H, W, g["pre"])
            fa = lambda v: (ctypes.c_float * len(v))(*v)
            common = (B, A, H, W, g["pre"], g["post"], float(g["thr"]), g["min_size"], fa(g["scales"]),
                      len(g["scales"]), fa(g["ratios"]), len(g["ratios"]), g["stride"])
            if g["v2"]:
                _call(fn, _ptr(cls_prob), _ptr(bbox_pred), _ptr(im_info), _ptr(in_data[3]),
                      _ptr(out_data[0]), _ptr(out_data[1]), *common, int(g["filter_scales"]),
                      int(g["iou_loss"]), wsp, wsn, None)
            else:
                _call(fn, _ptr(cls_prob), _ptr(bbox_pred), _ptr(im_info), _ptr(out_data[0]),
                      _ptr(out_data[1]), *common, int(g["is_train"]), int(g["iou_loss"]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(in_grad)):  # proposal_v2.cu:617-639, proposal.cu: all zeros
                self.assign(in_grad[i], req[i], 0)

    class _ProposalV12Prop(Prop):
        OUTS = ("output", "score")
        OP = ProposalV12
        V2 = True

        def _init(self, rpn_pre_nms_top_n, rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                  feature_stride, output_score, iou_loss, is_train="False", filter_scales="False"):
            super().__init__(need_top_grad=False)
            self.g = dict(pre=int(rpn_pre_nms_top_n), post=int(rpn_post_nms_top_n), thr=float(threshold),
                          min_size=int(rpn_min_size), scales=_tuple(scales), ratios=_tuple(ratios),
                          stride=int(feature_stride), iou_loss=_bool(iou_loss), is_train=_bool(is_train),
                          filter_scales=_bool(filter_scales), v2=self.V2)
            self.num_visible_outputs = 2 if _bool(output_score) else 1

        def list_arguments(self):
            return ["cls_prob", "bbox_pred", "im_info"] + (["valid_ranges"] if self.V2 else [])

        def infer_shape(self, in_shape):
            # ProposalProp(_v2)::InferShape (proposal_v2-inl.h:199-220, proposal-inl.h:199-217)
            d = in_shape[0]
            if len(d) != 4:
                raise ValueError("cls_prob should be (batch, 2 * num_anchors, H, W)")
            g = self.g
            A = d[1] // 2
            if A != len(g["scales"]) * len(g["ratios"]):
                raise ValueError("num_anchors != len(ratios) * len(scales)")
            ins = [d, (d[0], 4 * A, d[2], d[3]), (d[0], 3)] + ([(d[0], 2)] if self.V2 else [])
            return ins, [(d[0], g["post"], 4), (d[0], g["post"], 1)]

    class ProposalV2Prop(_ProposalV12Prop):
        V2 = True

        def __init__(self, rpn_pre_nms_top_n="6000", rpn_post_nms_top_n="300", threshold="0.7",
                     rpn_min_size="16", scales="(4,8,16,32)", ratios="(0.5,1,2)", feature_stride="16",
                     output_score="False", iou_loss="False", workspace="256", filter_scales="False"):
            # defaults: proposal_v2-inl.h:141-183
            self._init(rpn_pre_nms_top_n, rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                       feature_stride, output_score, iou_loss, filter_scales=filter_scales)

    class ProposalV1Prop(_ProposalV12Prop):
        V2 = False

        def __init__(self, rpn_pre_nms_top_n="6000", rpn_post_nms_top_n="300", threshold="0.7",
                     rpn_min_size="16", scales="(4,8,16,32)", ratios="(0.5,1,2)", feature_stride="16",
                     output_score="False", iou_loss="False", workspace="256", is_train="False"):
            # defaults: proposal-inl.h:141-183
            self._init(rpn_pre_nms_top_n, rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                       feature_stride, output_score, iou_loss, is_train=is_train)

    ops["_contrib_Proposal_v2"] = (ProposalV2Prop, ("contrib", "Proposal_v2"))
    ops["_contrib_Proposal"] = (ProposalV1Prop, ("contrib", "Proposal"))

    # ---- _contrib_GenProposalRetina: cls_prob, bbox_pred, im_info, anchors -> output, scores ----
    #      (registered only by install(..., retina=True))
    class GenProposalRetina(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            cls_prob, bbox_pred, im_info, anchors = in_data
            _wait(cls_prob, bbox_pred, im_info, anchors)
            g = self.g
            B, AK, H, W = cls_prob.shape
            ws, wsp, wsn = _ws(cls_prob, "sd_gen_proposal_retina_workspace_bytes", B, AK, H, W)
            fa = lambda v: (ctypes.c_float * len(v))(*v)
            _call("sd_gen_proposal_retina", _ptr(cls_prob), _ptr(bbox_pred), _ptr(im_info), _ptr(anchors),
                  _ptr(out_data[0]), _ptr(out_data[1]), B, AK, H, W, g["A"], g["pre"], g["min_size"],
                  float(g["thresh"]), fa(g["mean"]), fa(g["std"]), int(g["iou_loss"]), int(g["one_hot"]),
                  int(g["bwa"]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(4):  # generate_proposal_retina.cu:471-493
                self.assign(in_grad[i], req[i], 0)

    class GenProposalRetinaProp(Prop):
        ARGS = ("cls_prob", "bbox_pred", "im_info", "anchors")
        OUTS = ("output", "scores")
        OP = GenProposalRetina
        PARAMS = ("rpn_pre_nms_top_n", "rpn_min_size", "feature_stride", "num_anchors", "thresh", "anchor_mean",
                  "anchor_std", "iou_loss", "output_one_hot", "batch_wise_anchor", "workspace")

        def __init__(self, num_anchors, rpn_pre_nms_top_n="6000", rpn_min_size="16", feature_stride="16",
                     thresh="0", anchor_mean="(0,0,0,0)", anchor_std="(1,1,1,1)", iou_loss="False",
                     output_one_hot="True", batch_wise_anchor="False", workspace="256"):
            # defaults: generate_proposal_retina-inl.h:62-89
            super().__init__(need_top_grad=False)
            why = self.sd_supports(dict(num_anchors=num_anchors, rpn_pre_nms_top_n=rpn_pre_nms_top_n,
                                        iou_loss=iou_loss, batch_wise_anchor=batch_wise_anchor,
                                        anchor_mean=anchor_mean, anchor_std=anchor_std))
            if why:
                raise ValueError("GenProposalRetina: " + why)
            self.g = dict(A=int(num_anchors), pre=int(rpn_pre_nms_top_n), min_size=int(rpn_min_size),
                          thresh=float(thresh), mean=_tuple(anchor_mean, 4), std=_tuple(anchor_std, 4),
                          iou_loss=_bool(iou_loss), one_hot=_bool(output_one_hot), bwa=_bool(batch_wise_anchor))

        @classmethod
        def sd_supports(cls, params):
            """'' when the kernels take this parameter set, else the reason (install()'s alias then falls
            back to the native constructor)."""
            for k in params:
                if k not in cls.PARAMS:
                    return "parameter %r is not one this operator takes" % k
            try:
                A = int(params.get("num_anchors", "0"))
                pre = int(params.get("rpn_pre_nms_top_n", "6000"))
                _tuple(params.get("anchor_mean", "(0,0,0,0)"), 4)
                _tuple(params.get("anchor_std", "(1,1,1,1)"), 4)
            except Exception as e:
                return "unparsable parameter (%s)" % e
            if A <= 0:
                return "num_anchors must be > 0"
            if not 0 < pre <= 16384:
                return "rpn_pre_nms_top_n=%d outside 1..16384" % pre
            # the class count is only known from the input shape: the reference reads out of bounds for
            # K > 1 in both of these (generate_proposal_retina.cu:161-209, :383)
            if _bool(params.get("iou_loss", "False")):
                return "iou_loss is taken only for one class, unknown when the graph is built"
            if _bool(params.get("batch_wise_anchor", "False")):
                return "batch_wise_anchor is taken only for one class or one image, unknown when the graph is built"
            return ""

        def infer_shape(self, in_shape):
            # GenProposalRetinaProp::InferShape (generate_proposal_retina-inl.h:106-140)
            d = in_shape[0]
            if len(d) != 4:
                raise ValueError("cls_prob should be (batch, num_anchors * num_classes, H, W)")
            g = self.g
            A = g["A"]
            if d[1] % A:
                raise ValueError("cls_prob channels (%d) are not a multiple of num_anchors (%d)" % (d[1], A))
            anchors = (d[0], d[2] * d[3] * A, 4) if g["bwa"] else (d[2] * d[3] * A, 4)
            oc = d[1] // A + 1 if g["one_hot"] else 1
            return ([d, (d[0], 4 * A, d[2], d[3]), (d[0], 3), anchors],
                    [(d[0], g["pre"], 4), (d[0], g["pre"], oc)])

    ops["_contrib_GenProposalRetina"] = (GenProposalRetinaProp, ("contrib", "GenProposalRetina"))

    # ---- get_top_proposal (models/FPN/get_top_proposal.py): bbox, score -> top_n of each ----
    class GetTopProposal(CustomOp):
        def __init__(self, top_n):
            super().__init__()
            self.top_n = top_n

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            bbox, score = in_data
            _wait(bbox, score)
            _call("sd_get_top_proposal", _ptr(bbox), _ptr(score), bbox.shape[0], bbox.shape[1],
                       self.top_n, _ptr(out_data[0]), _ptr(out_data[1]), None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            self.assign(in_grad[0], req[0], 0)
            self.assign(in_grad[1], req[1], 0)

    class GetTopProposalProp(Prop):
        ARGS = ("bbox", "score")
        OUTS = ("bbox", "score")
        OP, OP_ARGS = GetTopProposal, ("top_n",)

        def __init__(self, top_n):
            super().__init__(need_top_grad=False)
            self.top_n = int(top_n)

        def infer_shape(self, in_shape):
            b = in_shape[0]
            return in_shape, [(b[0], self.top_n, b[2]), (b[0], self.top_n, 1)]

    ops["get_top_proposal"] = (GetTopProposalProp, None)

    # ---- _contrib_DecodeBBox: rois, bbox_pred, im_info -> output ----
    class DecodeBBox(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _require_write(req[:1], ["output"])
            rois, pred, info = in_data
            _wait(rois, pred, info)
            g = self.g
            fa = lambda v: (ctypes.c_float * 4)(*v)
            _call("sd_decode_bbox", _ptr(rois), _ptr(pred), _ptr(info), _ptr(out_data[0]),
                       rois.shape[0], rois.shape[1], pred.shape[2] // 4, fa(g["mean"]), fa(g["std"]),
                       int(g["agnostic"]), int(g["xyxy"]), None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(3):
                self.assign(in_grad[i], req[i], 0)

    class DecodeBBoxProp(Prop):
        ARGS = ("rois", "bbox_pred", "im_info")
        OP = DecodeBBox

        def __init__(self, bbox_mean="(0,0,0,0)", bbox_std="(0.1,0.1,0.2,0.2)",
                     class_agnostic="True", bbox_decode_type="xywh"):
            super().__init__(need_top_grad=False)
            if bbox_decode_type not in ("xywh", "xyxy"):
                raise ValueError("bbox_decode_type must be 'xywh' or 'xyxy'")
            self.g = dict(mean=_tuple(bbox_mean, 4), std=_tuple(bbox_std, 4),
                          agnostic=_bool(class_agnostic), xyxy=bbox_decode_type == "xyxy")

        def infer_shape(self, in_shape):
            d = in_shape[1]
            out = (d[0], d[1], 4) if self.g["agnostic"] else tuple(d)
            return in_shape, [out]

    ops["_contrib_DecodeBBox"] = (DecodeBBoxProp, ("contrib", "DecodeBBox"))

    # ---- BboxPostProcessing (models/maskrcnn/bbox_post_processing.py:35-111): cls_score, bbox_xyxy ->
    # post_score, post_bbox_xyxy, post_cls.  The reference's is itself a Python CustomOp reached through
    # mx.sym.Custom, so there is no constructor to alias: patch_bbox_post rebinds the builder method ----
    class BboxPostProcessing(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _require_write(req[:3], ["post_score", "post_bbox_xyxy", "post_cls"])
            score, bbox = in_data
            _wait(score, bbox)
            g = self.g
            B, R, K = score.shape
            Kb = bbox.shape[2] // 4
            ws, wsp, wsn = _ws(score, "sd_bbox_post_processing_workspace_bytes", B, R, K, Kb, g["max_det"])
            _call("sd_bbox_post_processing", _ptr(score), _ptr(bbox), B, R, K, Kb, g["min_score"], g["thr"],
                  g["max_det"], _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            self.assign(in_grad[0], req[0], 0)
            self.assign(in_grad[1], req[1], 0)

    class BboxPostProcessingProp(Prop):
        ARGS = ("cls_score", "bbox_xyxy")
        OUTS = ("post_score", "post_bbox_xyxy", "post_cls")
        OP = BboxPostProcessing
        LIMITS = dict(rows=4096, classes=256, max_det=1024)

        def __init__(self, max_det_per_image, min_det_score, nms_type, nms_thr):
            super().__init__(need_top_grad=False)
            # parsed as BboxPostProcessingProp.__init__ does (bbox_post_processing.py:81-86)
            self.g = dict(max_det=int(max_det_per_image), min_score=float(min_det_score),
                          nms_type=str(nms_type), thr=float(nms_thr))
            if self.g["nms_type"] != "nms":
                raise NotImplementedError("BboxPostProcessing: nms_type %r (the reference takes 'nms' only)"
                                          % self.g["nms_type"])

        @classmethod
        def sd_supports(cls, params):
            """'' when the kernels take this parameter set, else the reason (patch_bbox_post then hands the
            call back to the reference's method)."""
            try:
                top = int(params["max_det_per_image"])
                float(params["min_det_score"])
                float(params["nms_thr"])
            except Exception as e:
                return "unparsable parameter (%s)" % e
            if str(params.get("nms_type")) != "nms":
                return "nms_type %r is not 'nms'" % (params.get("nms_type"),)
            if not 0 <= top <= cls.LIMITS["max_det"]:
                return "max_det_per_image=%d outside 0..%d" % (top, cls.LIMITS["max_det"])
            return ""

        def infer_shape(self, in_shape):
            s, b = in_shape[0], in_shape[1]
            if len(s) != 3 or len(b) != 3:
                raise ValueError("cls_score should be (batch, rois, classes), bbox_xyxy (batch, rois, 4 or 4 * classes)")
            if s[1] > self.LIMITS["rows"] or s[2] > self.LIMITS["classes"] or b[2] not in (4, 4 * s[2]):
                raise ValueError("BboxPostProcessing: cls_score %s / bbox_xyxy %s outside rois <= %d, classes <= %d, "
                                 "boxes (.,.,4) or (.,.,4 * classes)" % (tuple(s), tuple(b), self.LIMITS["rows"],
                                                                         self.LIMITS["classes"]))
            top = self.g["max_det"]
            return [s, b], [(s[0], top, 1), (s[0], top, 4), (s[0], top, 1)]

    ops["BboxPostProcessing"] = (BboxPostProcessingProp, None)
    return ops


def _deform_conv_ops(mx):
    """DeformableConvolution"""
    Op, Prop = op_base(mx), prop_base(mx)
    ops = {}

    # ---- _contrib_DeformableConvolution: data, offset, weight[, bias] -> output.  Upstream MXNet 1.6
    #      DeformableConvolutionParam: kernel, stride, dilate, pad, num_filter, num_group,
    #      num_deformable_group, workspace, no_bias (default False), layout.  Call sites:
    #      models/dcn/builder.py:14-17 (no_bias=True), models/RepPoints/builder.py:215-245 (bias),
    #      models/sepc/sepc_dconv.py:12-16 (num_group / bias passed through),
    #      models/tridentnet/resnet_v1.py:85-90 (weight / bias shared between branches) ----
    class DeformConv(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            x, off, w = in_data[:3]
            b = in_data[3] if self.g["bias"] else None
            _wait(*in_data)
            g = self.g
            N, C, H, W = x.shape
            # training with cache_col: im2col + GEMM, the col matrix stays alive until this node's backward,
            # which then skips its own im2col (620 MB per layer at the baseline; cache_col="False" trades it
            # for the fused col-free forward and a backward that recomputes col).  Otherwise no col matrix:
            # deformable sampling fused into the GEMM (a few MB of workspace instead of N*C*9*Ho*Wo*4 bytes;
            # shapes the fused kernel does not take run im2col + GEMM behind the same entry point)
            keep = 1 if (is_train and g["cache_col"]) else 0
            ws, wsp, wsn = _ws(x, "sd_deform_convolution_fwd_workspace_bytes", N, C, H, W, g["F"], g["kh"], g["kw"],
                               g["pad"], g["stride"], g["dil"], g["dg"], g["G"], keep)
            _call("sd_deform_convolution_fwd", _ptr(x), _ptr(off), _ptr(w), _ptr(b), _ptr(out_data[0]), N, C,
                       H, W, g["F"], g["kh"], g["kw"], g["pad"], g["stride"], g["dil"], g["dg"], g["G"], keep,
                       wsp, wsn, None)
            self._fwd_ws = (ws, tuple(x.shape)) if keep else None
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            x, off, w = in_data[:3]
            _wait(out_grad[0], *in_data)
            g = self.g
            N, C, H, W = x.shape
            ws, wsp, wsn = _ws(x, "sd_deform_conv_workspace_bytes", N, C, H, W, g["kh"], g["kw"], g["pad"], g["stride"],
                               g["dil"])
            kept = getattr(self, "_fwd_ws", None)
            self._fwd_ws = None
            col = None
            if kept is not None and kept[1] == tuple(x.shape):
                col = ctypes.c_void_p(lib().cdll.sd_deform_conv_col_of_workspace(_ptr(kept[0])))
            has_b = g["bias"]
            _call("sd_deform_convolution_bwd", _ptr(out_grad[0]), _ptr(x), _ptr(off), _ptr(w), col,
                       _ptr(in_grad[0]), _ptr(in_grad[1]), _ptr(in_grad[2]), _ptr(in_grad[3]) if has_b else None,
                       _req(req[0]), _req(req[1]), _req(req[2]), _req(req[3]) if has_b else REQ["null"],
                       N, C, H, W, g["F"], g["kh"], g["kw"], g["pad"], g["stride"], g["dil"], g["dg"], g["G"],
                       wsp, wsn, None)
            _sync()

    class DeformConvProp(Prop):
        OP = DeformConv
        # (the bias itself is not needed by the backward: deformable_convolution-inl.h Backward reads
        # out_grad, data, offset, weight)
        DEPS = ((OUT_GRAD, 0), (IN_DATA, 0), (IN_DATA, 1), (IN_DATA, 2))
        # the op's own parameter names (+ cache_col, this adapter's attribute); anything else, and any
        # value the kernels do not take, makes install()'s alias hand the call back to the constructor it
        # replaced (sd_supports) -- the graph then holds the native operator for that node
        PARAMS = ("kernel", "num_filter", "stride", "dilate", "pad", "num_group", "num_deformable_group", "no_bias",
                  "workspace", "layout", "cache_col")

        def __init__(self, kernel, num_filter, stride="(1,1)", dilate="(1,1)", pad="(0,0)",
                     num_group="1", num_deformable_group="1", no_bias="False", workspace="1024",
                     layout="None", cache_col="True"):
            # cache_col is this adapter's own attribute: keep the forward's col matrix for the
            # backward of the same node (training only)
            super().__init__(need_top_grad=True)
            why = self.sd_supports(dict(kernel=kernel, num_filter=num_filter, stride=stride, dilate=dilate, pad=pad,
                                        num_group=num_group, num_deformable_group=num_deformable_group,
                                        layout=layout))
            if why:
                raise ValueError("DeformableConvolution: " + why)
            k, s, d, p = (_tuple(kernel, 2, int), _tuple(stride, 2, int), _tuple(dilate, 2, int),
                          _tuple(pad, 2, int))
            self.g = dict(kh=k[0], kw=k[1], stride=s[0], dil=d[0], pad=p[0], F=int(num_filter),
                          dg=int(num_deformable_group), G=int(num_group), bias=not _bool(no_bias),
                          # SIMPLEDET_AMD_DCN_CACHE_COL=0: process-wide off switch (no node keeps 620 MB
                          # between its forward and backward, whatever its attribute says)
                          cache_col=_bool(cache_col) and os.environ.get("SIMPLEDET_AMD_DCN_CACHE_COL", "1") != "0")

        @classmethod
        def sd_supports(cls, params):
            """'' when the kernels take this parameter set, else the reason (install()'s alias then falls
            back to the native constructor).  params: str-valued, as MXNet hands them to a CustomOpProp."""
            for k in params:
                if k not in cls.PARAMS:
                    return "parameter %r is not one this operator takes" % k
            try:
                k = _tuple(params.get("kernel", "(0,0)"), 2, int)
                s, d, p = (_tuple(params.get(n, dflt), 2, int) for n, dflt in
                           (("stride", "(1,1)"), ("dilate", "(1,1)"), ("pad", "(0,0)")))
                int(params.get("num_filter", "0")), int(params.get("num_group", "1"))
                int(params.get("num_deformable_group", "1"))
            except Exception as e:
                return "unparsable parameter (%s)" % e
            if len(k) != 2 or len(s) != 2 or len(d) != 2 or len(p) != 2:
                return "2-D convolutions only"
            if s[0] != s[1] or d[0] != d[1] or p[0] != p[1]:
                return "square stride/dilate/pad only"
            if str(params.get("layout", "None")) not in ("None", "NCHW"):
                return "layout NCHW only"
            if int(params.get("num_group", "1")) < 1 or int(params.get("num_deformable_group", "1")) < 1:
                return "num_group / num_deformable_group must be positive"
            return ""

        def list_arguments(self):
            return ["data", "offset", "weight"] + (["bias"] if self.g["bias"] else [])

        def infer_shape(self, in_shape):
            g = self.g
            d = in_shape[0]
            if len(d) != 4:
                raise ValueError("Input data should be 4D in batch-num_filter-y-x")
            if d[1] % g["G"] or g["F"] % g["G"]:
                raise ValueError("input / output num_filter must divide group size")
            if d[1] % g["dg"]:
                raise ValueError("input num_filter must divide deformable group size")
            Ho = (d[2] + 2 * g["pad"] - (g["dil"] * (g["kh"] - 1) + 1)) // g["stride"] + 1
            Wo = (d[3] + 2 * g["pad"] - (g["dil"] * (g["kw"] - 1) + 1)) // g["stride"] + 1
            off = (d[0], g["dg"] * 2 * g["kh"] * g["kw"], Ho, Wo)
            w = (g["F"], d[1] // g["G"], g["kh"], g["kw"])
            ins = [d, off, w] + ([(g["F"],)] if g["bias"] else [])
            return ins, [(d[0], g["F"], Ho, Wo)]

    ops["_contrib_DeformableConvolution"] = (DeformConvProp, ("contrib", "DeformableConvolution"))
    return ops


def _retina_norm_ops(mx):
    """FocalLoss, BBoxNorm, GroupNorm, Quantization_int8"""
    CustomOp, Op, Prop = mx.operator.CustomOp, op_base(mx), prop_base(mx)
    ops = {}

    # ---- _contrib_FocalLoss / _contrib_BBoxNorm: data, label -> output ----
    #      (registered only by install(..., retina_loss=True))
    NORMALIZATION = {"null": 0, "batch": 1, "valid": 2}

    class FocalLoss(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            data = in_data[0]
            _wait(data)
            _call("sd_focal_loss_fwd", _ptr(data), _ptr(out_data[0]), ctypes.c_long(_numel(data.shape)), None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # focal_loss-inl.h:116-231: kWriteTo on the data gradient (:129); the label gradient is not written
            _require_write(req[:1], ["FocalLoss data gradient"])
            g = self.g
            label, out = in_data[1], out_data[0]
            ograd = out_grad[0] if g["out_grad"] else None
            _wait(label, out, ograd)
            if _req(req[0]) != REQ["null"]:
                B, nbox, nclass = out.shape
                ws, wsp, wsn = _ws(out, "sd_focal_loss_workspace_bytes")
                _call("sd_focal_loss_bwd", _ptr(out), _ptr(label), _ptr(ograd), _ptr(in_grad[0]), B, nbox, nclass,
                      float(g["alpha"]), float(g["gamma"]), float(g["grad_scale"]), g["normalization"], wsp, wsn, None)
            _sync()

    class FocalLossProp(Prop):
        ARGS = ("data", "label")
        OP = FocalLoss

        def __init__(self, alpha="0.25", gamma="2.0", grad_scale="1.0", normalization="null", out_grad="False",
                     workspace="256"):
            # defaults: focal_loss-inl.h:59-80.  `workspace` (MB of temporaries in the reference) is accepted and unused.
            out_grad = _bool(out_grad)
            super().__init__(need_top_grad=out_grad)
            if normalization not in NORMALIZATION:
                raise ValueError("FocalLoss: normalization must be one of %s" % sorted(NORMALIZATION))
            self.g = dict(alpha=float(alpha), gamma=float(gamma), grad_scale=float(grad_scale),
                          normalization=NORMALIZATION[normalization], out_grad=out_grad)

        def infer_shape(self, in_shape):
            # FocalLossProp::InferShape (focal_loss-inl.h:258-272): data (B, nbox, nclass), label (B, nbox)
            d = in_shape[0]
            if len(d) != 3:
                raise ValueError("FocalLoss: data should be (batch, box, class)")
            return [d, (d[0], d[1])], [d]

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            # focal_loss-inl.h:314-324
            deps = [in_data[1], out_data[0]]
            return deps + [out_grad[0]] if self.g["out_grad"] else deps

    ops["_contrib_FocalLoss"] = (FocalLossProp, ("contrib", "FocalLoss"))

    class BBoxNorm(CustomOp):
        def forward(self, is_train, req, in_data, out_data, aux):
            self.assign(out_data[0], req[0], in_data[0])   # F<identity> (bbox_norm-inl.h:96)

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            _require_write(req[:1], ["BBoxNorm data gradient"])
            gout, label = out_grad[0], in_data[1]
            _wait(gout, label)
            if _req(req[0]) != REQ["null"]:
                B = gout.shape[0]
                ws, wsp, wsn = _ws(gout, "sd_focal_loss_workspace_bytes")    # (the two losses share one size)
                _call("sd_bbox_norm_bwd", _ptr(gout), _ptr(label), _ptr(in_grad[0]), B,
                      ctypes.c_long(_numel(gout.shape) // B if B else 0),
                      ctypes.c_long(_numel(label.shape) // B if B else 0), wsp, wsn, None)
            if len(req) > 1:
                self.assign(in_grad[1], req[1], 0)         # :128
            _sync()

    class BBoxNormProp(Prop):
        ARGS = ("data", "label")
        OP, OP_ARGS = BBoxNorm, ()
        DEPS = ((IN_DATA, 1), (OUT_GRAD, 0))  # bbox_norm-inl.h:212-217

        def __init__(self, normalization="null"):
            # bbox_norm-inl.h:52-65: the parameter is declared and never read by the operator
            super().__init__(need_top_grad=True)
            if normalization not in NORMALIZATION:
                raise ValueError("BBoxNorm: normalization must be one of %s" % sorted(NORMALIZATION))

        def infer_shape(self, in_shape):
            # BBoxNormProp::InferShape: data (B, 4A, npos), label (B, A * npos); the output has data's shape
            d = in_shape[0]
            if len(d) < 2:
                raise ValueError("BBoxNorm: data should be (batch, 4 * anchor, position)")
            label = tuple(in_shape[1]) if len(in_shape) > 1 and in_shape[1] else (d[0], _numel(d[1:]) // 4)
            return [d, label], [d]

    ops["_contrib_BBoxNorm"] = (BBoxNormProp, ("contrib", "BBoxNorm"))

    # ---- _contrib_GroupNorm: data, gamma, beta -> output, mean, var (1 visible) ----
    #      (registered only by install(..., group_norm=True))
    class GroupNorm(Op):
        def _dims(self, data):
            N, C = int(data.shape[0]), int(data.shape[1])
            return N, C, (_numel(data.shape) // (N * C) if N * C else 0), self.g["num_group"]

        def _workspace(self, like, dims):
            return _ws(like, "sd_group_norm_workspace_bytes", dims[0], dims[1], ctypes.c_long(dims[2]), dims[3])

        def forward(self, is_train, req, in_data, out_data, aux):
            # group_norm-inl.h:88-122.  mean / var are declared (N, C) and receive N * G floats (:199-200): the
            # first N * G floats of the buffers are written, the rest is left as it was.
            _no_add(req)
            data, gamma, beta = in_data[:3]
            _wait(data, gamma, beta)
            N, C, HxW, G = dims = self._dims(data)
            ws, wsp, wsn = self._workspace(data, dims)
            _call("sd_group_norm_fwd", _ptr(data), _ptr(gamma), _ptr(beta), _ptr(out_data[0]), _ptr(out_data[1]),
                  _ptr(out_data[2]), N, C, ctypes.c_long(HxW), G, float(self.g["eps"]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # group_norm-inl.h:124-164: dX, dgamma and dbeta are plain stores (no Assign with req): kWriteTo
            _require_write(req[:3], ["GroupNorm data gradient", "GroupNorm gamma gradient", "GroupNorm beta gradient"])
            data, gamma = in_data[0], in_data[1]
            _wait(out_grad[0], data, gamma, out_data[1], out_data[2])
            N, C, HxW, G = dims = self._dims(data)
            want_dx = _req(req[0]) != REQ["null"]
            want = [_req(r) != REQ["null"] for r in req[1:3]]
            if want[0] != want[1]:
                raise RuntimeError("GroupNorm: the gamma and beta gradients are written together or not at all")
            if want_dx or want[0]:
                # (a frozen input with trainable gamma / beta: dX goes to scratch, as the reference always writes it)
                dx = in_grad[0] if want_dx else _scratch(data, 4 * _numel(data.shape))
                ws, wsp, wsn = self._workspace(data, dims)
                _call("sd_group_norm_bwd", _ptr(out_grad[0]), _ptr(data), _ptr(out_data[1]), _ptr(out_data[2]),
                      _ptr(gamma), _ptr(dx), _ptr(in_grad[1]) if want[0] else None,
                      _ptr(in_grad[2]) if want[0] else None, N, C, ctypes.c_long(HxW), G, wsp, wsn, None)
            _sync()

    class GroupNormProp(Prop):
        ARGS = ("data", "gamma", "beta")
        OUTS = ("output", "mean", "var")
        num_visible_outputs = 1
        OP = GroupNorm
        # group_norm-inl.h:211-220
        DEPS = ((OUT_GRAD, 0), (OUT_DATA, 1), (OUT_DATA, 2), (IN_DATA, 0), (IN_DATA, 1))

        def __init__(self, num_group="32", eps="1e-5"):
            # defaults: group_norm-inl.h:70-77
            super().__init__(need_top_grad=True)
            self.g = dict(num_group=int(num_group), eps=float(eps))
            if self.g["num_group"] <= 0:
                raise ValueError("GroupNorm: num_group must be positive, got %d" % self.g["num_group"])

        def infer_shape(self, in_shape):
            # GroupNormProp::InferShape (group_norm-inl.h:185-202): gamma / beta (C,); mean / var (N, C)
            d = tuple(in_shape[0])
            if len(d) < 2:
                raise ValueError("GroupNorm: data should be (batch, channel, ...)")
            if d[1] % self.g["num_group"]:
                raise ValueError("GroupNorm: channels (%d) are not divisible by num_group (%d)"
                                 % (d[1], self.g["num_group"]))
            return [d, (d[1],), (d[1],)], [d, (d[0], d[1]), (d[0], d[1])]

    ops["_contrib_GroupNorm"] = (GroupNormProp, ("contrib", "GroupNorm"))
    # ---- _contrib_Quantization_int8: data -> output, aux minmax ----
    #      (registered only by install(..., quant_int8=True))
    class QuantizationInt8(CustomOp):
        """Owns the step state {countdown, init} the reference keeps in its Operator object
        (quantization_int8-inl.h:103-108), as two ints on the device; made on the first forward, on the data's
        context (create_operator only knows the context's name)."""

        def __init__(self, q):
            super().__init__()
            self.q = q
            self.state = None

        def forward(self, is_train, req, in_data, out_data, aux):
            # quantization_int8-inl.h:125: CHECK_EQ(req[kOut], kWriteTo)
            _require_write(req[:1], ["Quantization_int8 output"])
            data, minmax = in_data[0], aux[0]
            _wait(data, minmax)
            if self.state is None:
                self.state = _state["mx"].nd.array([self.q["delay_quant"], 1], ctx=data.context, dtype="int32")
            n = _numel(data.shape)
            if n and _req(req[0]) != REQ["null"]:
                ws, wsp, wsn = _ws(data, "sd_quant_int8_workspace_bytes", ctypes.c_long(n))
                _call("sd_quant_int8_fwd", _ptr(data), _ptr(out_data[0]), _ptr(minmax), _ptr(self.state),
                      ctypes.c_long(n), int(self.q["is_weight"]), int(bool(is_train)), int(self.q["fix_act_scale"]),
                      float(self.q["ema_decay"]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # :229-294: the reference only writes; add is this adapter's usual extension
            r = _req(req[0])
            clip = self.q["grad_mode"] == "clip" and not self.q["is_weight"]
            _wait(out_grad[0], in_data[0], aux[0])
            n = _numel(in_data[0].shape)
            if n and r != REQ["null"]:
                _call("sd_quant_int8_bwd", _ptr(out_grad[0]), _ptr(in_data[0]) if clip else None,
                      _ptr(aux[0]) if clip else None, _ptr(in_grad[0]), ctypes.c_long(n), int(clip), r, None)
            _sync()

    class QuantizationInt8Prop(Prop):
        ARGS = ("data",)
        AUX = ("minmax",)
        OP, OP_ARGS = QuantizationInt8, ("q",)
        DEPS = ((OUT_GRAD, 0), (IN_DATA, 0))
        PARAMS = ("quant_mode", "is_weight", "is_weight_perchannel", "delay_quant", "ema_decay", "grad_mode",
                  "fix_act_scale")

        def __init__(self, quant_mode="minmax", is_weight="True", is_weight_perchannel="False", delay_quant="0",
                     ema_decay="0.99", grad_mode="ste", fix_act_scale="False"):
            # defaults: quantization_int8-inl.h:85-100
            super().__init__(need_top_grad=True)
            self.q = dict(quant_mode=str(quant_mode), is_weight=_bool(is_weight),
                          is_weight_perchannel=_bool(is_weight_perchannel), delay_quant=int(delay_quant),
                          ema_decay=float(ema_decay), grad_mode=str(grad_mode), fix_act_scale=_bool(fix_act_scale))
            why = self.sd_supports({k: str(v) for k, v in self.q.items()})
            if why:
                raise ValueError("Quantization_int8: " + why)

        @classmethod
        def sd_supports(cls, params):
            """'' when the kernels take this parameter set, else the reason (install()'s alias then falls
            back to the native constructor)."""
            for k in params:
                if k not in cls.PARAMS:
                    return "parameter %r is not one this operator takes" % k
            try:
                delay = int(params.get("delay_quant", "0"))
                decay = float(params.get("ema_decay", "0.99"))
            except Exception as e:
                return "unparsable parameter (%s)" % e
            if params.get("quant_mode", "minmax") != "minmax":
                return "quant_mode %r is not 'minmax'" % (params.get("quant_mode"),)
            if _bool(params.get("is_weight", "True")) and _bool(params.get("is_weight_perchannel", "False")):
                return "per-channel weights are not supported"
            if params.get("grad_mode", "ste") not in ("ste", "clip"):
                return "grad_mode %r is neither 'ste' nor 'clip'" % (params.get("grad_mode"),)
            if delay < 0 or not 0.0 <= decay <= 1.0:
                return "delay_quant=%d / ema_decay=%g out of range" % (delay, decay)
            return ""

        def infer_shape(self, in_shape):
            # Quantization_int8Prop::InferShape: data of rank 2 or 4, the output has its shape, the aux is (1,)
            d = tuple(in_shape[0])
            if len(d) not in (2, 4):
                raise ValueError("Quantization_int8: data should be 2D or 4D, got shape %s" % (d,))
            return [d], [d], [(1,)]

    ops["_contrib_Quantization_int8"] = (QuantizationInt8Prop, ("contrib", "Quantization_int8"))
    return ops


def _mask_loss_ops(mx):
    """SigmoidCrossEntropy, MaskLoss and the Mask Scoring R-CNN pair"""
    Op, Prop = op_base(mx), prop_base(mx)
    ops = {}

    # ---- _contrib_SigmoidCrossEntropy: data, label -> output, loss, loss_sum, count, count_sum (1 visible) and
    #      the fused MaskLoss: logits, cls, target -> output, count_sum (1 visible)
    #      (registered only by install(..., mask_loss=True)) ----
    class SigmoidCrossEntropy(Op):
        @staticmethod
        def _rows(data):
            n = int(data.shape[0])
            return n, (_numel(data.shape) // n if n else 0)

        def _workspace(self, like, n, k):
            return _ws(like, "sd_sigmoid_ce_workspace_bytes", ctypes.c_long(n), ctypes.c_long(k))

        def forward(self, is_train, req, in_data, out_data, aux):
            # sigmoid_cross_entropy-inl.h:68-92: all five outputs are plain stores
            _no_add(req)
            data, label = in_data[:2]
            _wait(data, label)
            n, k = self._rows(data)
            ws, wsp, wsn = self._workspace(data, n, k)
            _call("sd_sigmoid_ce_fwd", _ptr(data), _ptr(label), _ptr(out_data[0]), _ptr(out_data[1]),
                  _ptr(out_data[2]), _ptr(out_data[3]), _ptr(out_data[4]), ctypes.c_long(n), ctypes.c_long(k),
                  wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # :94-119: d_data is a plain store (kWriteTo), count / count_sum are written again, out_grad is
            # never read; the label gradient is not written by the reference and is zeroed here
            _require_write(req[:1], ["SigmoidCrossEntropy data gradient"])
            data, label = in_data[:2]
            _wait(data, label)
            if _req(req[0]) != REQ["null"]:
                n, k = self._rows(data)
                ws, wsp, wsn = self._workspace(data, n, k)
                _call("sd_sigmoid_ce_bwd", _ptr(data), _ptr(label), _ptr(in_grad[0]), _ptr(out_data[3]),
                      _ptr(out_data[4]), ctypes.c_long(n), ctypes.c_long(k), float(self.g["grad_scale"]), wsp, wsn,
                      None)
            if len(req) > 1:
                self.assign(in_grad[1], req[1], 0)
            _sync()

    class SigmoidCrossEntropyProp(Prop):
        ARGS = ("data", "label")
        OUTS = ("output", "loss", "loss_sum", "count", "count_sum")
        num_visible_outputs = 1
        OP = SigmoidCrossEntropy
        DEPS = ((IN_DATA, 0), (IN_DATA, 1), (OUT_DATA, 3), (OUT_DATA, 4))  # :200-206

        def __init__(self, grad_scale="1.0", normalization="valid"):
            # defaults: sigmoid_cross_entropy-inl.h:52-60.  `normalization` is parsed and never used by the
            # reference's operator (the division by the count always happens): accepted and unused here as well
            super().__init__(need_top_grad=False)
            if normalization not in ("null", "valid"):
                raise ValueError("SigmoidCrossEntropy: normalization must be 'null' or 'valid'")
            self.g = dict(grad_scale=float(grad_scale), normalization=normalization)

        def infer_shape(self, in_shape):
            # SigmoidCrossEntropyProp::InferShape (:152-172): out / loss_sum / count_sum (n,), loss / count as data
            d = tuple(in_shape[0])
            if len(d) < 2:
                raise ValueError("SigmoidCrossEntropy: data should be (row, ...) with at least 2 dimensions")
            label = tuple(in_shape[1]) if len(in_shape) > 1 and in_shape[1] else d
            if len(label) < 2:
                raise ValueError("SigmoidCrossEntropy: label should have at least 2 dimensions")
            o = (d[0],)
            return [d, label], [o, d, o, d, o]

    class MaskLoss(Op):
        @staticmethod
        def _dims(logits):
            R, K = int(logits.shape[0]), int(logits.shape[1])
            return R, K, (_numel(logits.shape) // (R * K) if R * K else 0)

        def _workspace(self, like, dims):
            return _ws(like, "sd_mask_loss_workspace_bytes", dims[0], dims[1], ctypes.c_long(dims[2]))

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            logits, cls, target = in_data[:3]
            _wait(logits, cls, target)
            R, K, P = dims = self._dims(logits)
            ws, wsp, wsn = self._workspace(logits, dims)
            _call("sd_mask_loss_fwd", _ptr(logits), _ptr(cls), _ptr(target), _ptr(out_data[0]), _ptr(out_data[1]),
                  R, K, ctypes.c_long(P), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            _require_write(req[:1], ["MaskLoss logits gradient"])
            logits, cls, target = in_data[:3]
            _wait(logits, cls, target)
            if _req(req[0]) != REQ["null"]:
                R, K, P = dims = self._dims(logits)
                ws, wsp, wsn = self._workspace(logits, dims)
                _call("sd_mask_loss_bwd", _ptr(logits), _ptr(cls), _ptr(target), _ptr(in_grad[0]), R, K,
                      ctypes.c_long(P), float(self.g["grad_scale"]), wsp, wsn, None)
            for i in (1, 2):
                if len(req) > i:
                    self.assign(in_grad[i], req[i], 0)
            _sync()

    class MaskLossProp(Prop):
        ARGS = ("logits", "cls", "target")
        OUTS = ("output", "count_sum")
        num_visible_outputs = 1
        OP = MaskLoss
        DEPS = ((IN_DATA, 0), (IN_DATA, 1), (IN_DATA, 2))

        def __init__(self, grad_scale="1.0"):
            super().__init__(need_top_grad=False)
            self.g = dict(grad_scale=float(grad_scale))

        def infer_shape(self, in_shape):
            # logits (R, K, h, w); cls R floats in any shape (the builder's mask_label is (batch, fg)); target R*h*w
            d = tuple(in_shape[0])
            if len(d) < 2:
                raise ValueError("MaskLoss: logits should be (roi, class, ...)")
            cls = tuple(in_shape[1]) if len(in_shape) > 1 and in_shape[1] else (d[0],)
            target = tuple(in_shape[2]) if len(in_shape) > 2 and in_shape[2] else (d[0],) + d[2:]
            if _numel(cls) != d[0] or _numel(target) != d[0] * _numel(d[2:]):
                raise ValueError("MaskLoss: cls %s / target %s do not match logits %s" % (cls, target, d))
            return [d, cls, target], [(1,), (1,)]

    ops["_contrib_SigmoidCrossEntropy"] = (SigmoidCrossEntropyProp, ("contrib", "SigmoidCrossEntropy"))
    ops["MaskLoss"] = (MaskLossProp, None)

    # ---- the Mask Scoring R-CNN training head (registered only by install(..., msrcnn=True)):
    #      MsrcnnMaskLoss: logits, cls, target -> output (the mask loss), mask_pred_prob (the gathered sigmoid)
    #      MaskIoULoss:    iou_pred, prob, target, ratio, cls -> output, iou_target, weight, weight_sum (1 visible) ----
    class MsrcnnMaskLoss(Op):
        def _workspace(self, like, dims):
            return _ws(like, "sd_msrcnn_mask_loss_workspace_bytes", dims[0], dims[1], ctypes.c_long(dims[2]))

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            logits, cls, target = in_data[:3]
            _wait(logits, cls, target)
            R, K, P = dims = MaskLoss._dims(logits)
            ws, wsp, wsn = self._workspace(logits, dims)
            count_sum = _scratch(logits, 4)      # the reference's hidden output; nothing downstream reads it
            _call("sd_msrcnn_mask_loss_fwd", _ptr(logits), _ptr(cls), _ptr(target), _ptr(out_data[0]),
                  _ptr(count_sum), _ptr(out_data[1]), R, K, ctypes.c_long(P), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # the loss output's head gradient is never read (a loss operator); the one that reached mask_pred_prob
            # joins the selected plane in the same pass
            _require_write(req[:1], ["MsrcnnMaskLoss logits gradient"])
            logits, cls, target = in_data[:3]
            d_prob = out_grad[1] if len(out_grad) > 1 else None
            _wait(logits, cls, target, d_prob)
            if _req(req[0]) != REQ["null"]:
                R, K, P = dims = MaskLoss._dims(logits)
                ws, wsp, wsn = self._workspace(logits, dims)
                _call("sd_msrcnn_mask_loss_bwd", _ptr(logits), _ptr(cls), _ptr(target), _ptr(d_prob),
                      _ptr(in_grad[0]), R, K, ctypes.c_long(P), float(self.g["grad_scale"]), wsp, wsn, None)
            for i in (1, 2):
                if len(req) > i:
                    self.assign(in_grad[i], req[i], 0)
            _sync()

    class MsrcnnMaskLossProp(Prop):
        ARGS = ("logits", "cls", "target")
        OUTS = ("output", "mask_pred_prob")
        OP = MsrcnnMaskLoss
        DEPS = ((OUT_GRAD, 1), (IN_DATA, 0), (IN_DATA, 1), (IN_DATA, 2))

        def __init__(self, grad_scale="1.0"):
            super().__init__(need_top_grad=True)
            self.g = dict(grad_scale=float(grad_scale))

        def infer_shape(self, in_shape):
            # as MaskLoss; mask_pred_prob is the gathered plane of every RoI: (R, h, w)
            d = tuple(in_shape[0])
            if len(d) < 2:
                raise ValueError("MsrcnnMaskLoss: logits should be (roi, class, ...)")
            cls = tuple(in_shape[1]) if len(in_shape) > 1 and in_shape[1] else (d[0],)
            target = tuple(in_shape[2]) if len(in_shape) > 2 and in_shape[2] else (d[0],) + d[2:]
            if _numel(cls) != d[0] or _numel(target) != d[0] * _numel(d[2:]):
                raise ValueError("MsrcnnMaskLoss: cls %s / target %s do not match logits %s" % (cls, target, d))
            return [d, cls, target], [(1,), (d[0],) + d[2:]]

    class MaskIoULoss(Op):
        @staticmethod
        def _dims(iou_pred, prob):
            R, K = int(iou_pred.shape[0]), int(iou_pred.shape[1])
            return R, K, (_numel(prob.shape) // R if R else 0)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            iou_pred, prob, target, ratio, cls = in_data[:5]
            _wait(iou_pred, prob, target, ratio, cls)
            R, K, P = self._dims(iou_pred, prob)
            ws, wsp, wsn = _ws(iou_pred, "sd_maskiou_loss_workspace_bytes", R, K, ctypes.c_long(P))
            _call("sd_maskiou_loss_fwd", _ptr(iou_pred), _ptr(prob), _ptr(target), _ptr(ratio), _ptr(cls),
                  _ptr(out_data[1]), _ptr(out_data[2]), _ptr(out_data[0]), _ptr(out_data[3]), R, K, ctypes.c_long(P),
                  wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # MakeLoss: the head gradient is not read.  prob, target, ratio and cls get zeros: the reference
            # BlockGrads the CustomOp's outputs and its backward assigns 0
            _require_write(req[:1], ["MaskIoULoss iou_pred gradient"])
            iou_pred, cls = in_data[0], in_data[4]
            _wait(iou_pred, cls, out_data[1], out_data[2], out_data[3])
            if _req(req[0]) != REQ["null"]:
                R, K = int(iou_pred.shape[0]), int(iou_pred.shape[1])
                _call("sd_maskiou_loss_bwd", _ptr(iou_pred), _ptr(cls), _ptr(out_data[1]), _ptr(out_data[2]),
                      _ptr(out_data[3]), _ptr(in_grad[0]), R, K, float(self.g["grad_scale"]), None)
            for i in (1, 2, 3, 4):
                if len(req) > i:
                    self.assign(in_grad[i], req[i], 0)
            _sync()

    class MaskIoULossProp(Prop):
        ARGS = ("iou_pred", "prob", "target", "ratio", "cls")
        OUTS = ("output", "iou_target", "weight", "weight_sum")
        num_visible_outputs = 1
        OP = MaskIoULoss
        DEPS = ((IN_DATA, 0), (IN_DATA, 4), (OUT_DATA, 1), (OUT_DATA, 2), (OUT_DATA, 3))

        def __init__(self, grad_scale="1.0"):
            super().__init__(need_top_grad=False)
            self.g = dict(grad_scale=float(grad_scale))

        def infer_shape(self, in_shape):
            # iou_pred (R, K); prob / target R * h * w floats; ratio and cls R floats in any shape (the builder's
            # mask_ratio and mask_label are (batch, fg))
            d = tuple(in_shape[0])
            if len(d) != 2:
                raise ValueError("MaskIoULoss: iou_pred should be (roi, class)")
            R = d[0]
            prob = tuple(in_shape[1]) if len(in_shape) > 1 and in_shape[1] else None
            if prob is None or len(prob) < 2 or prob[0] != R:
                raise ValueError("MaskIoULoss: prob %s should be (roi, ...) with %d rows" % (prob, R))
            target = tuple(in_shape[2]) if len(in_shape) > 2 and in_shape[2] else prob
            ratio = tuple(in_shape[3]) if len(in_shape) > 3 and in_shape[3] else (R,)
            cls = tuple(in_shape[4]) if len(in_shape) > 4 and in_shape[4] else (R,)
            if _numel(target) != _numel(prob) or _numel(ratio) != R or _numel(cls) != R:
                raise ValueError("MaskIoULoss: target %s / ratio %s / cls %s do not match prob %s"
                                 % (target, ratio, cls, prob))
            return [d, prob, target, ratio, cls], [(1,), (R,), (R,), (1,)]

    ops["MsrcnnMaskLoss"] = (MsrcnnMaskLossProp, None)
    ops["MaskIoULoss"] = (MaskIoULossProp, None)
    return ops


def _fcos_ops(mx):
    """the FCOS training head and test-time decode"""
    Op, Prop = op_base(mx), prop_base(mx)
    ops = {}

    # ---- the FCOS training head (registered only by install(..., fcos=True)):
    #      fcos_target: gt_bbox, im_info -> centerness, offset, cls_id (int32), state (int32[4])
    #      fcos_loss:   3 * L level tensors + the four targets -> centerness_loss, cls_loss, offset_loss ----
    def _fcos_strides(v):
        return _tuple(v, typ=int)

    class FCOSTarget(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            gt, info = in_data[:2]
            _wait(gt, info)
            g = self.g
            N, M = int(gt.shape[0]), int(gt.shape[1])
            HW = int(out_data[0].shape[1])
            ws, wsp, wsn = _ws(gt, "sd_fcos_target_workspace_bytes", N, ctypes.c_long(HW))
            _call("sd_fcos_target", _ptr(gt), _ptr(info), _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]),
                  None, _ptr(out_data[3]), N, M, g["num_classifier"], g["data_size"][0], g["data_size"][1],
                  _iarr(g["stride"]), None, None, len(g["stride"]), float(g["ignore_offset"]),
                  float(g["ignore_label"]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(req)):       # targets carry no gradient (the reference blocks it)
                self.assign(in_grad[i], req[i], 0)

    class FCOSTargetProp(Prop):
        ARGS = ("gt_bbox", "im_info")
        OUTS = ("centerness", "offset", "cls_id", "state")
        OP = FCOSTarget

        def __init__(self, data_size, stride, num_classifier, ignore_offset="-1", ignore_label="-1"):
            super().__init__(need_top_grad=False)
            self.g = dict(data_size=_tuple(data_size, typ=int), stride=_fcos_strides(stride),
                          num_classifier=int(num_classifier), ignore_offset=float(ignore_offset),
                          ignore_label=float(ignore_label))
            if len(self.g["data_size"]) != 2 or not 1 <= len(self.g["stride"]) <= 5:
                raise ValueError("fcos_target: data_size is (h, w) and stride has 1 to 5 entries")

        def infer_shape(self, in_shape):
            # PreMakeFCOSGTProp.infer_shape (models/FCOS/input.py:99-107)
            gt = tuple(in_shape[0])
            if len(gt) != 3 or gt[2] != 5:
                raise ValueError("fcos_target: gt_bbox should be (N, M, 5), got %s" % (gt,))
            n, (h, w) = gt[0], self.g["data_size"]
            hw = sum(len(range(0, w, s)) * len(range(0, h, s)) for s in self.g["stride"])
            info = tuple(in_shape[1]) if len(in_shape) > 1 and in_shape[1] else (n, 3)
            return [gt, info], [(n, hw), (n, 4, hw), (n, hw), (4,)]

        def infer_type(self, in_type):
            import numpy as np
            return [in_type[0]] * 2, [in_type[0], in_type[0], np.int32, np.int32], []

    class FCOSLoss(Op):
        def _tables(self, in_data):
            L = self.g["num_levels"]
            cls, ctr, off = in_data[:L], in_data[L:2 * L], in_data[2 * L:3 * L]
            N, K = int(cls[0].shape[0]), int(cls[0].shape[1])
            hws = [_numel(c.shape) // (N * K) if N * K else 0 for c in cls]
            tab = lambda arrs: (ctypes.c_void_p * L)(*[_ptr(a).value for a in arrs])
            return L, N, K, hws, tab, (cls, ctr, off), in_data[3 * L:3 * L + 4]

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            L, N, K, hws, tab, (cls, ctr, off), (cen, offs, cid, state) = self._tables(in_data)
            g = self.g
            ws, wsp, wsn = _ws(cls[0], "sd_fcos_loss_workspace_bytes", N, K, ctypes.c_long(sum(hws)))
            losses = _scratch(cls[0], 12)
            _call("sd_fcos_loss_fwd", tab(cls), tab(ctr), tab(off), (ctypes.c_long * L)(*hws), L, _ptr(cen),
                  _ptr(offs), _ptr(cid), _ptr(state), _ptr(losses), N, K, g["alpha"], g["gamma"],
                  float(g["ignore_offset"]), float(g["ignore_label"]), wsp, wsn, None)
            _sync()
            for i in range(3):
                self.assign(out_data[i], req[i], losses[i:i + 1])

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # the gradients do not depend on out_grad (compute_focal_loss / compute_bce_loss ignore it and
            # MakeLoss has grad_scale = 1); all three are plain stores, one launch for every level
            L, N, K, hws, tab, (cls, ctr, off), (cen, offs, cid, state) = self._tables(in_data)
            _require_write(req[:3 * L], ["FCOSLoss logits gradient"] * (3 * L))
            _wait(*in_data)
            live = [_req(r) != REQ["null"] for r in req[:3 * L]]
            if any(live):
                if not all(live):
                    raise RuntimeError("FCOSLoss writes the gradients of all levels in one launch: req must be "
                                       "'write' for every logit tensor or 'null' for every one")
                g = self.g
                _call("sd_fcos_loss_bwd", tab(cls), tab(ctr), tab(off), tab(in_grad[:L]), tab(in_grad[L:2 * L]),
                      tab(in_grad[2 * L:3 * L]), (ctypes.c_long * L)(*hws), L, _ptr(cen), _ptr(offs), _ptr(cid),
                      _ptr(state), N, K, g["alpha"], g["gamma"], float(g["ignore_offset"]),
                      float(g["ignore_label"]), None)
            for i in range(3 * L, len(req)):
                self.assign(in_grad[i], req[i], 0)
            _sync()

    class FCOSLossProp(Prop):
        OUTS = ("centerness_loss", "cls_loss", "offset_loss")
        OP = FCOSLoss

        def __init__(self, num_levels, alpha="0.25", gamma="2.0", ignore_offset="-1", ignore_label="-1"):
            super().__init__(need_top_grad=False)
            self.g = dict(num_levels=int(num_levels), alpha=float(alpha), gamma=float(gamma),
                          ignore_offset=float(ignore_offset), ignore_label=float(ignore_label))
            if not 1 <= self.g["num_levels"] <= 8:
                raise ValueError("fcos_loss: num_levels must lie in 1..8")

        def list_arguments(self):
            L = self.g["num_levels"]
            return (["cls_logit_%d" % i for i in range(L)] + ["centerness_logit_%d" % i for i in range(L)]
                    + ["offset_logit_%d" % i for i in range(L)] + ["centerness", "offset", "cls_id", "state"])

        def infer_shape(self, in_shape):
            L = self.g["num_levels"]
            shapes = [tuple(s) for s in in_shape]
            if len(shapes) != 3 * L + 4:
                raise ValueError("fcos_loss: expected %d inputs, got %d" % (3 * L + 4, len(shapes)))
            n, k, hw = shapes[0][0], shapes[0][1], 0
            for i in range(L):
                c, t, o = shapes[i], shapes[L + i], shapes[2 * L + i]
                if not (len(c) >= 3 and c[:2] == (n, k) and t == (n, 1) + c[2:] and o == (n, 4) + c[2:]):
                    raise ValueError("fcos_loss: level %d shapes %s / %s / %s do not belong together" % (i, c, t, o))
                hw += _numel(c[2:])
            targets = [(n, hw), (n, 4, hw), (n, hw), (4,)]
            for want, got in zip(targets, shapes[3 * L:]):
                if got and got != want:
                    raise ValueError("fcos_loss: target shape %s, expected %s" % (got, want))
            return shapes[:3 * L] + targets, [(1,)] * 3

        def infer_type(self, in_type):
            import numpy as np
            L = self.g["num_levels"]
            return [in_type[0]] * (3 * L + 2) + [np.int32, np.int32], [in_type[0]] * 3, []

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return list(in_data)

    ops["fcos_target"] = (FCOSTargetProp, None)
    ops["fcos_loss"] = (FCOSLossProp, None)

    # ---- the FCOS test-time decode (registered only by install(..., fcos_decode=True)):
    #      fcos_decode: 3 * L level tensors (class logits, centerness logits, offsets) + im_info -> bbox, score, cls_id
    class FCOSDecode(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            g = self.g
            L = g["num_levels"]
            cls, ctr, off, info = in_data[:L], in_data[L:2 * L], in_data[2 * L:3 * L], in_data[3 * L]
            N, C = int(cls[0].shape[0]), int(cls[0].shape[1])
            Hs, Ws = [int(c.shape[2]) for c in cls], [int(c.shape[3]) for c in cls]
            tab = lambda arrs: (ctypes.c_void_p * L)(*[_ptr(a).value for a in arrs])
            hws = (ctypes.c_long * L)(*[h * w for h, w in zip(Hs, Ws)])
            ws, wsp, wsn = _ws(cls[0], "sd_fcos_decode_workspace_bytes", N, C, L, hws, g["pre_nms_top_n"])
            _call("sd_fcos_decode", tab(cls), tab(ctr), tab(off), _ptr(info), _iarr(Hs), _iarr(Ws), _iarr(g["stride"]),
                  L, N, C, g["pre_nms_top_n"], float(g["pre_nms_thresh"]), int(g["input_logits"]), _ptr(out_data[0]),
                  _ptr(out_data[1]), _ptr(out_data[2]), None, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(req)):       # the reference's CustomOps have an empty backward (utils.py:70,127)
                self.assign(in_grad[i], req[i], 0)

    class FCOSDecodeProp(Prop):
        OUTS = ("bbox", "score", "cls_id")
        OP = FCOSDecode

        def __init__(self, stride, pre_nms_top_n, pre_nms_thresh, input_logits="1"):
            super().__init__(need_top_grad=False)
            self.g = dict(stride=_fcos_strides(stride), pre_nms_top_n=int(pre_nms_top_n),
                          pre_nms_thresh=float(pre_nms_thresh), input_logits=_bool(input_logits))
            self.g["num_levels"] = len(self.g["stride"])
            if not 1 <= self.g["num_levels"] <= 8 or self.g["pre_nms_top_n"] < 1:
                raise ValueError("fcos_decode: stride has 1 to 8 entries and pre_nms_top_n is >= 1")

        def list_arguments(self):
            L = self.g["num_levels"]
            return (["cls_logit_%d" % i for i in range(L)] + ["centerness_logit_%d" % i for i in range(L)]
                    + ["offset_logit_%d" % i for i in range(L)] + ["im_info"])

        def infer_shape(self, in_shape):
            L = self.g["num_levels"]
            shapes = [tuple(s) for s in in_shape]
            if len(shapes) != 3 * L + 1:
                raise ValueError("fcos_decode: expected %d inputs, got %d" % (3 * L + 1, len(shapes)))
            n, k = shapes[0][0], shapes[0][1]
            for i in range(L):
                c, t, o = shapes[i], shapes[L + i], shapes[2 * L + i]
                if not (len(c) == 4 and c[:2] == (n, k) and t == (n, 1) + c[2:] and o == (n, 4) + c[2:]):
                    raise ValueError("fcos_decode: level %d shapes %s / %s / %s do not belong together" % (i, c, t, o))
            if shapes[3 * L] and shapes[3 * L] != (n, 3):
                raise ValueError("fcos_decode: im_info shape %s, expected %s" % (shapes[3 * L], (n, 3)))
            r = L * self.g["pre_nms_top_n"]
            return shapes[:3 * L] + [(n, 3)], [(n, r, 4), (n, r, 81), (n, r)]

        def infer_type(self, in_type):
            return [in_type[0]] * (3 * self.g["num_levels"] + 1), [in_type[0]] * 3, []

    ops["fcos_decode"] = (FCOSDecodeProp, None)
    return ops


def _reppoints_ops(mx):
    """the RepPoints training head and test-time decode"""
    Op, Prop = op_base(mx), prop_base(mx)
    ops = {}

    # ---- the RepPoints training head (registered only by install(..., reppoints=True)):
    #      reppoints_target:   L init point maps, gt_bbox, moment_transfer -> label_init, gt_init, label_refine,
    #                          gt_refine, state (int32[4])
    #      reppoints_box_loss: L init maps, L refine maps, moment_transfer, the five targets -> pts_init_loss,
    #                          pts_refine_loss (N, P, 4) ----
    _RP_TRANSFORMS = {"minmax": 0, "partial_minmax": 1, "moment": 2}

    def _rp_geometry(stride, num_points, transform, who):
        g = dict(stride=_tuple(stride, typ=int), num_points=int(num_points), transform=str(transform))
        if not 1 <= len(g["stride"]) <= 8 or g["num_points"] not in (1, 9, 25) or g["transform"] not in _RP_TRANSFORMS:
            raise ValueError("%s: stride has 1 to 8 entries, num_points is 1, 9 or 25 and transform one of %s"
                             % (who, sorted(_RP_TRANSFORMS)))
        return g

    def _rp_levels(g, maps):
        """(N, P, H table, W table, stride table) of L level maps (N, 2 * num_points, H_l, W_l)"""
        Hs, Ws = [int(m.shape[2]) for m in maps], [int(m.shape[3]) for m in maps]
        return int(maps[0].shape[0]), sum(h * w for h, w in zip(Hs, Ws)), _iarr(Hs), _iarr(Ws), _iarr(g["stride"])

    def _rp_map_shapes(g, shapes, who):
        """checks L level shapes; returns (N, P)"""
        n, c = shapes[0][0], 2 * g["num_points"]
        for i, sh in enumerate(shapes):
            if len(sh) != 4 or sh[0] != n or sh[1] != c:
                raise ValueError("%s: level %d should be (N, %d, H, W), got %s" % (who, i, c, sh))
        return n, sum(sh[2] * sh[3] for sh in shapes)

    class RepPointsTarget(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            g = self.g
            L = len(g["stride"])
            maps, gt, mt = in_data[:L], in_data[L], in_data[L + 1]
            N, P, Hs, Ws, st = _rp_levels(g, maps)
            M = int(gt.shape[1])
            ws, wsp, wsn = _ws(gt, "sd_reppoints_target_workspace_bytes", N, M, ctypes.c_long(P))
            tab = (ctypes.c_void_p * L)(*[_ptr(a).value for a in maps])
            _call("sd_reppoints_target", tab, Hs, Ws, st, L, _ptr(gt), _ptr(mt), _ptr(out_data[0]), _ptr(out_data[1]),
                  _ptr(out_data[2]), _ptr(out_data[3]), _ptr(out_data[4]), N, M, g["num_points"],
                  _RP_TRANSFORMS[g["transform"]], g["target_scale"], g["num_pos"], g["pos_iou_thr"], g["neg_iou_thr"],
                  g["min_pos_iou"], wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(req)):       # targets carry no gradient (box_iou, topk and take of gt rows)
                self.assign(in_grad[i], req[i], 0)

    class RepPointsTargetProp(Prop):
        OUTS = ("label_init", "gt_init", "label_refine", "gt_refine", "state")
        OP = RepPointsTarget

        def __init__(self, stride, num_points="9", transform="moment", target_scale="4", num_pos="1",
                     pos_iou_thr="0.5", neg_iou_thr="0.5", min_pos_iou="0.0"):
            super().__init__(need_top_grad=False)
            self.g = _rp_geometry(stride, num_points, transform, "reppoints_target")
            self.g.update(target_scale=float(target_scale), num_pos=int(num_pos), pos_iou_thr=float(pos_iou_thr),
                          neg_iou_thr=float(neg_iou_thr), min_pos_iou=float(min_pos_iou))
            if not 1 <= self.g["num_pos"] <= 16:
                raise ValueError("reppoints_target: num_pos must lie in 1..16")

        def list_arguments(self):
            return ["pts_init_%d" % i for i in range(len(self.g["stride"]))] + ["gt_bbox", "moment_transfer"]

        def infer_shape(self, in_shape):
            L = len(self.g["stride"])
            shapes = [tuple(s) for s in in_shape]
            if len(shapes) != L + 2:
                raise ValueError("reppoints_target: expected %d inputs, got %d" % (L + 2, len(shapes)))
            n, p = _rp_map_shapes(self.g, shapes[:L], "reppoints_target")
            gt = shapes[L]
            if len(gt) != 3 or gt[0] != n or gt[2] != 5 or not 1 <= gt[1] <= 128:
                raise ValueError("reppoints_target: gt_bbox should be (%d, M <= 128, 5), got %s" % (n, gt))
            return shapes[:L] + [gt, (2,)], [(n, p), (n, p, 4), (n, p), (n, p, 4), (4,)]

        def infer_type(self, in_type):
            import numpy as np
            return [in_type[0]] * len(in_type), [in_type[0]] * 4 + [np.int32], []

    class RepPointsBoxLoss(Op):
        def _args(self, in_data):
            g = self.g
            L = len(g["stride"])
            pi, pr, mt, targets = in_data[:L], in_data[L:2 * L], in_data[2 * L], in_data[2 * L + 1:2 * L + 6]
            tab = lambda arrs: (ctypes.c_void_p * L)(*[_ptr(a).value for a in arrs])
            return L, pi, pr, mt, targets, tab, _rp_levels(g, pi)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            g = self.g
            L, pi, pr, mt, (li, gi, lr, gr, state), tab, (N, P, Hs, Ws, st) = self._args(in_data)
            _call("sd_reppoints_box_loss_fwd", tab(pi), tab(pr), Hs, Ws, st, L, _ptr(mt), _ptr(li), _ptr(gi), _ptr(lr),
                  _ptr(gr), _ptr(out_data[0]), _ptr(out_data[1]), N, g["num_points"], _RP_TRANSFORMS[g["transform"]],
                  g["scale"], None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # MakeLoss ignores the incoming gradient: the head gradient is grad_scale / the BBoxNorm denominator
            g = self.g
            L, pi, pr, mt, (li, gi, lr, gr, state), tab, (N, P, Hs, Ws, st) = self._args(in_data)
            _wait(*in_data)
            reqs = {_req(r) for r in req[:2 * L + 1]}
            if reqs != {REQ["null"]}:
                if len(reqs) != 1:
                    raise RuntimeError("RepPointsBoxLoss writes every gradient in one launch: req must be the same "
                                       "('write', 'add' or 'null') for the 2 * L point maps and moment_transfer")
                ws, wsp, wsn = _ws(pi[0], "sd_reppoints_box_loss_workspace_bytes", N, ctypes.c_long(P))
                _call("sd_reppoints_box_loss_bwd", tab(pi), tab(pr), Hs, Ws, st, L, _ptr(mt), _ptr(li), _ptr(gi),
                      _ptr(lr), _ptr(gr), _ptr(state), tab(in_grad[:L]), tab(in_grad[L:2 * L]), _ptr(in_grad[2 * L]),
                      N, g["num_points"], _RP_TRANSFORMS[g["transform"]], g["scale"], g["grad_scale_init"],
                      g["grad_scale_refine"], reqs.pop(), wsp, wsn, None)
            for i in range(2 * L + 1, len(req)):
                self.assign(in_grad[i], req[i], 0)
            _sync()

    class RepPointsBoxLossProp(Prop):
        OUTS = ("pts_init_loss", "pts_refine_loss")
        OP = RepPointsBoxLoss

        def __init__(self, stride, num_points="9", transform="moment", scale="4", grad_scale_init="0.5",
                     grad_scale_refine="1.0"):
            super().__init__(need_top_grad=False)
            self.g = _rp_geometry(stride, num_points, transform, "reppoints_box_loss")
            self.g.update(scale=float(scale), grad_scale_init=float(grad_scale_init),
                          grad_scale_refine=float(grad_scale_refine))

        def list_arguments(self):
            L = len(self.g["stride"])
            return (["pts_init_%d" % i for i in range(L)] + ["pts_refine_%d" % i for i in range(L)]
                    + ["moment_transfer", "label_init", "gt_init", "label_refine", "gt_refine", "state"])

        def infer_shape(self, in_shape):
            L = len(self.g["stride"])
            shapes = [tuple(s) for s in in_shape]
            if len(shapes) != 2 * L + 6:
                raise ValueError("reppoints_box_loss: expected %d inputs, got %d" % (2 * L + 6, len(shapes)))
            n, p = _rp_map_shapes(self.g, shapes[:L], "reppoints_box_loss")
            if shapes[L:2 * L] != shapes[:L]:
                raise ValueError("reppoints_box_loss: the refine maps %s differ from the init maps %s"
                                 % (shapes[L:2 * L], shapes[:L]))
            rest = [(2,), (n, p), (n, p, 4), (n, p), (n, p, 4), (4,)]
            for want, got in zip(rest, shapes[2 * L:]):
                if got and got != want:
                    raise ValueError("reppoints_box_loss: input shape %s, expected %s" % (got, want))
            return shapes[:2 * L] + rest, [(n, p, 4), (n, p, 4)]

        def infer_type(self, in_type):
            import numpy as np
            return [in_type[0]] * (len(in_type) - 1) + [np.int32], [in_type[0]] * 2, []

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return list(in_data)

    ops["reppoints_target"] = (RepPointsTargetProp, None)
    ops["reppoints_box_loss"] = (RepPointsBoxLossProp, None)

    # ---- the RepPoints test-time decode (registered only by install(..., reppoints_decode=True)):
    #      reppoints_decode: L class logit maps, L refine point maps, im_info, moment_transfer -> cls_score (N, R, C + 1),
    #                        bbox_xyxy (N, R, 4) ----
    class RepPointsDecode(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            g = self.g
            L = len(g["stride"])
            cls, pts, info, mt = in_data[:L], in_data[L:2 * L], in_data[2 * L], in_data[2 * L + 1]
            N, C = int(cls[0].shape[0]), int(cls[0].shape[1])
            Hs, Ws = [int(c.shape[2]) for c in cls], [int(c.shape[3]) for c in cls]
            tab = lambda arrs: (ctypes.c_void_p * L)(*[_ptr(a).value for a in arrs])
            hws = (ctypes.c_long * L)(*[h * w for h, w in zip(Hs, Ws)])
            ks = _iarr(_rp_topk_table(g))
            ws, wsp, wsn = _ws(cls[0], "sd_reppoints_decode_workspace_bytes", N, C, L, hws, ks)
            _call("sd_reppoints_decode", tab(cls), tab(pts), _ptr(info), _ptr(mt), _iarr(Hs), _iarr(Ws),
                  _iarr(g["stride"]), ks, L, N, C, g["num_points"], _RP_TRANSFORMS[g["transform"]],
                  int(g["input_logits"]), _ptr(out_data[0]), _ptr(out_data[1]), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(req)):       # a test-time head: topk and take of rows carry no gradient
                self.assign(in_grad[i], req[i], 0)

    def _rp_topk_table(g):
        """rows kept per level (builder.py:499-502): pre_nms_top_n where the stride is <= 32, else all (-1)"""
        return [g["pre_nms_top_n"] if s <= 32 else -1 for s in g["stride"]]

    class RepPointsDecodeProp(Prop):
        OUTS = ("cls_score", "bbox_xyxy")
        OP = RepPointsDecode

        def __init__(self, stride, pre_nms_top_n, transform="moment", num_points="9", input_logits="1"):
            super().__init__(need_top_grad=False)
            self.g = dict(stride=_tuple(stride, typ=int), pre_nms_top_n=int(pre_nms_top_n), transform=str(transform),
                          num_points=int(num_points), input_logits=_bool(input_logits))
            g = self.g
            if not 1 <= len(g["stride"]) <= 8 or min(g["stride"]) < 1 or g["num_points"] < 1 \
                    or g["transform"] not in _RP_TRANSFORMS or (g["transform"] == "partial_minmax" and g["num_points"] < 4):
                raise ValueError("reppoints_decode: stride has 1 to 8 positive entries, num_points is >= 1 (>= 4 for "
                                 "partial_minmax) and transform one of %s" % sorted(_RP_TRANSFORMS))

        def list_arguments(self):
            L = len(self.g["stride"])
            return ["cls_logit_%d" % i for i in range(L)] + ["pts_refine_%d" % i for i in range(L)] + ["im_info", "moment_transfer"]

        def infer_shape(self, in_shape):
            g = self.g
            L = len(g["stride"])
            shapes = [tuple(s) for s in in_shape]
            if len(shapes) != 2 * L + 2:
                raise ValueError("reppoints_decode: expected %d inputs, got %d" % (2 * L + 2, len(shapes)))
            n, c = shapes[0][0], shapes[0][1]
            r = 0
            for i, (s, k) in enumerate(zip(g["stride"], _rp_topk_table(g))):
                a, b = shapes[i], shapes[L + i]
                if not (len(a) == 4 and a[:2] == (n, c) and b == (n, 2 * g["num_points"]) + a[2:]):
                    raise ValueError("reppoints_decode: level %d shapes %s / %s do not belong together" % (i, a, b))
                hw = a[2] * a[3]
                if k > hw:
                    raise ValueError(
                        "reppoints_decode: the stride-%d level holds %d locations, fewer than pre_nms_top_n = %d.  The "
                        "reference's note (models/RepPoints/builder.py:499-501): pre_nms_top_n_ is hard-coded as -1 only "
                        "for strides above 32, because the number of proposals is less than pre_nms_top_n in these "
                        "low-resolution feature maps; one should select the appropriate params here if using "
                        "low-resolution images as input." % (s, hw, k))
                keep = k if k > 0 else hw
                if keep > 16384:
                    raise ValueError("reppoints_decode: the stride-%d level keeps %d rows, the limit is 16384" % (s, keep))
                r += keep
            if shapes[2 * L] and shapes[2 * L] != (n, 3):
                raise ValueError("reppoints_decode: im_info shape %s, expected %s" % (shapes[2 * L], (n, 3)))
            if shapes[2 * L + 1] and shapes[2 * L + 1] != (2,):
                raise ValueError("reppoints_decode: moment_transfer shape %s, expected (2,)" % (shapes[2 * L + 1],))
            return shapes[:2 * L] + [(n, 3), (2,)], [(n, r, c + 1), (n, r, 4)]

        def infer_type(self, in_type):
            return [in_type[0]] * (2 * len(self.g["stride"]) + 2), [in_type[0]] * 2, []

    ops["reppoints_decode"] = (RepPointsDecodeProp, None)
    return ops


def _crowdhuman_ops(mx):
    """the CrowdHuman double-prediction head"""
    Op, Prop = op_base(mx), prop_base(mx)
    ops = {}

    # ---- the CrowdHuman double-prediction head (registered only by install(..., crowdhuman=True)):
    #      bbox_target:       proposal, gt_bbox -> sampled_proposal, bbox_cls, bbox_target, bbox_target_weight
    #      doublebbox_target: ... and bbox_sec_cls, bbox_sec_target, bbox_sec_target_weight
    #      emd_loss:          the two logits, labels, deltas, targets and weights -> output (1,) ----
    class CrowdHumanTarget(Op):
        def forward(self, is_train, req, in_data, out_data, aux):
            from . import ops as sd_ops
            _no_add(req)
            prop_, gt = in_data[:2]
            _wait(prop_, gt)
            g = self.g
            B, P, M = int(prop_.shape[0]), int(prop_.shape[1]), int(gt.shape[1])
            prm = sd_ops.CrowdHumanTargetParam()
            prm.num_reg_class, prm.add_gt_to_proposal, prm.image_rois = g["num_class"], int(g["add_gt_to_proposal"]), \
                g["image_rois"]
            prm.fg_fraction, prm.fg_thresh = g["fg_fraction"], g["fg_thresh"]
            prm.bg_thresh_hi, prm.bg_thresh_lo = g["bg_thresh_hi"], g["bg_thresh_lo"]
            for i, v in enumerate(g["bbox_target_std"]):
                prm.bbox_target_std[i] = v
            key = "mt19937:" + str(prop_.context)
            if key not in _state["rng"]:
                # numpy's global RandomState, which the reference's np.random.choice draws from: one stream per
                # device, taken over where the process's generator stands at the first call
                import numpy as np
                st = np.random.get_state()
                words = [int(k) - (1 << 32) if int(k) >= (1 << 31) else int(k) for k in st[1]] + [int(st[2])]
                _state["rng"][key] = _state["mx"].nd.array(words, ctx=prop_.context, dtype="int32")
            rng = _state["rng"][key]
            ws, wsp, wsn = _ws(prop_, "sd_crowdhuman_target_workspace_bytes", B, P, M)
            count = _scratch(prop_, 4 * B)     # rows filled per image; the reference has no such output
            outs = [_ptr(o) for o in out_data] + [None] * (7 - len(out_data))
            _call("sd_crowdhuman_target", _ptr(prop_), _ptr(gt), B, P, M, g["mode"], ctypes.byref(prm), _ptr(rng), *outs,
                  _ptr(count), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            for i in range(len(req)):       # bbox_target.py:180-182: zeros
                self.assign(in_grad[i], req[i], 0)

    def _crowdhuman_target_prop(mode):
        outputs = ["sampled_proposal", "bbox_cls", "bbox_target", "bbox_target_weight"]
        if mode == 1:
            outputs += ["bbox_sec_cls", "bbox_sec_target", "bbox_sec_target_weight"]

        class CrowdHumanTargetProp(Prop):
            ARGS, OUTS = ("proposal", "gt_bbox"), tuple(outputs)
            OP = CrowdHumanTarget

            def __init__(self, num_class, add_gt_to_proposal, image_rois, fg_fraction, fg_thresh, bg_thresh_hi,
                         bg_thresh_lo, bbox_target_std, xywh="True"):
                super().__init__(need_top_grad=False)
                # (xywh: the reference's operator prints it and never reads it, bbox_target.py:12-81)
                self.g = dict(mode=mode, num_class=int(num_class), add_gt_to_proposal=_bool(add_gt_to_proposal),
                              image_rois=int(image_rois), fg_fraction=float(fg_fraction), fg_thresh=float(fg_thresh),
                              bg_thresh_hi=float(bg_thresh_hi), bg_thresh_lo=float(bg_thresh_lo),
                              bbox_target_std=_tuple(bbox_target_std, 4))
                if len(self.g["bbox_target_std"]) != 4 or not 1 <= self.g["image_rois"] <= 1024:
                    raise ValueError("crowdhuman target: bbox_target_std has 4 entries and image_rois is in [1, 1024]")

            def infer_shape(self, in_shape):
                p, gt = tuple(in_shape[0]), tuple(in_shape[1])
                if len(p) != 3 or p[2] != 4 or len(gt) != 3 or gt[2] != 5 or gt[0] != p[0]:
                    raise ValueError("crowdhuman target: proposal (B, P, 4) and gt_bbox (B, M, 5), got %s and %s" % (p, gt))
                if gt[1] < 1 or gt[1] > 1024 or p[1] + gt[1] > 4096:
                    raise ValueError("crowdhuman target: 1 <= M <= 1024 and P + M <= 4096, got P = %d, M = %d" % (p[1], gt[1]))
                B, S, W = p[0], self.g["image_rois"], 4 * self.g["num_class"]
                outs = [(B, S, 4), (B, S), (B, S, W), (B, S, W)]
                return [p, gt], outs + ([(B, S), (B, S, W), (B, S, W)] if mode == 1 else []), []

        return CrowdHumanTargetProp

    class EmdLoss(Op):
        @staticmethod
        def _dims(in_data):
            R, K = int(in_data[0].shape[0]), int(in_data[0].shape[1])
            return R, K, int(in_data[4].shape[1])

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data[:10])
            R, K, D = self._dims(in_data)
            _call("sd_emd_loss_fwd", *[_ptr(t) for t in in_data[:10]], R, K, D, float(self.g["smooth_l1_scalar"]),
                  _ptr(out_data[0]), None, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # MakeLoss: the head gradient is not read.  Labels, targets and weights get zeros (the reference's target
            # operator blocks the gradient)
            grads = (0, 1, 4, 5)          # cls_logit, cls_sec_logit, bbox_delta, bbox_sec_delta
            _require_write([req[i] for i in grads], ["emd_loss gradient"] * 4)
            _wait(*in_data[:10])
            R, K, D = self._dims(in_data)
            if any(_req(req[i]) == REQ["null"] for i in grads):
                raise RuntimeError("emd_loss writes all four gradients (req='null' on one of them)")
            _call("sd_emd_loss_bwd", *[_ptr(t) for t in in_data[:10]], R, K, D, float(self.g["smooth_l1_scalar"]),
                  float(self.g["grad_scale"]), *[_ptr(in_grad[i]) for i in grads], None)
            for i in (2, 3, 6, 7, 8, 9):
                if len(req) > i:
                    self.assign(in_grad[i], req[i], 0)
            _sync()

    class EmdLossProp(Prop):
        ARGS = ("cls_logit", "cls_sec_logit", "cls_label", "cls_sec_label", "bbox_delta", "bbox_sec_delta",
                "bbox_target", "bbox_sec_target", "bbox_weight", "bbox_sec_weight")
        OP = EmdLoss

        def __init__(self, smooth_l1_scalar="1.0", grad_scale="1.0"):
            super().__init__(need_top_grad=False)
            self.g = dict(smooth_l1_scalar=float(smooth_l1_scalar), grad_scale=float(grad_scale))
            if not self.g["smooth_l1_scalar"] > 0:
                raise ValueError("emd_loss: smooth_l1_scalar must be positive")

        def infer_shape(self, in_shape):
            x, d = tuple(in_shape[0]), tuple(in_shape[4])
            if len(x) != 2 or len(d) != 2 or d[0] != x[0]:
                raise ValueError("emd_loss: cls_logit (R, K) and bbox_delta (R, 4 K'), got %s and %s" % (x, d))
            want = [x, x, (x[0],), (x[0],), d, d, d, d, d, d]
            for i, (w, s) in enumerate(zip(want, in_shape)):
                if s and _numel(tuple(s)) != _numel(w):
                    raise ValueError("emd_loss: %s is %s, expected %s" % (self.list_arguments()[i], tuple(s), w))
            return [tuple(s) if s else w for w, s in zip(want, in_shape)], [(1,)], []

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return list(in_data)

    ops["bbox_target"] = (_crowdhuman_target_prop(0), None)
    ops["doublebbox_target"] = (_crowdhuman_target_prop(1), None)
    ops["emd_loss"] = (EmdLossProp, None)
    return ops


_FAMILIES = (_roi_pool_ops, _target_ops, _proposal_ops, _deform_conv_ops, _retina_norm_ops, _mask_loss_ops, _fcos_ops,
             _reppoints_ops, _crowdhuman_ops)
# the table's order -- the order the operators were added in: registration, aliasing and _state["table"] follow it,
# and a new operator goes at the end
_TABLE_ORDER = (
    "_contrib_ROIAlign_v2", "ROIPooling_v1", "ProposalTarget", "ProposalTarget_v2", "ProposalMaskTarget",
    "_contrib_GenAnchor", "_contrib_NMS", "assign_layer_fpn", "_contrib_DeformableConvolution", "fpn_roi_align",
    "_contrib_DeformablePSROIPooling", "fpn_deform_roi_pool", "_contrib_Proposal_v3", "_contrib_Proposal_v2",
    "_contrib_Proposal", "_contrib_GenProposalRetina", "_contrib_GroupNorm", "_contrib_Quantization_int8",
    "_contrib_FocalLoss", "_contrib_BBoxNorm", "get_top_proposal", "_contrib_DecodeBBox", "BboxPostProcessing",
    "_contrib_SigmoidCrossEntropy", "MaskLoss", "MsrcnnMaskLoss", "MaskIoULoss", "fcos_target", "fcos_loss",
    "fcos_decode", "reppoints_target", "reppoints_box_loss", "reppoints_decode", "bbox_target", "doublebbox_target",
    "emd_loss")


def _build_ops(mx):
    """{name: (PropClass, where)} of every operator, opt-in ones included: the families' tables, in _TABLE_ORDER.
    `where` is (namespace, attribute) of the reference constructor install() aliases, or None."""
    found = {}
    for family in _FAMILIES:
        found.update(family(mx))
    if set(found) != set(_TABLE_ORDER):
        raise RuntimeError("_TABLE_ORDER and the families disagree on %s" % sorted(set(found) ^ set(_TABLE_ORDER)))
    return {name: found[name] for name in _TABLE_ORDER}


# ------------------------------------------------------------------------------- registration ----
def _feature_flags(given):
    """{flag: bool} over FEATURE_FLAGS from the keywords a caller gave; an unknown one is a TypeError"""
    unknown = sorted(set(given) - set(FEATURE_FLAGS))
    if unknown:
        raise TypeError("unknown feature flag(s) %s; the flags are %s" % (", ".join(unknown), ", ".join(FEATURE_FLAGS)))
    return {flag: bool(given.get(flag, False)) for flag in FEATURE_FLAGS}


def register(mx=None, **features):
    """Register every CustomOp (op_type = 'sd_' + reference op name).  Returns {name: PropClass}.
    The operators that would change what an existing graph holds -- they replace a native operator, a CustomOp of the
    reference's own or a subgraph of one of its builders -- are opt-in: each keyword of FEATURE_FLAGS set to True
    also registers the operators its _FEATURES entry gates (one line per flag there; INTEGRATION.md has the detail).
    An unknown keyword raises TypeError."""
    flags = _feature_flags(features)
    if mx is None:
        import mxnet as mx  # noqa: F811  (lazy: MXNet is only needed here)
    lib()  # fail loudly now if the HIP library is missing
    table = _build_ops(mx)
    _state["all_ops"] = {name: (None, where) for name, (_, where) in table.items()}
    for feature in _FEATURES.values():
        if not flags[feature.flag]:
            for name in feature.ops:
                table.pop(name)
    out = register_ops(mx, {name: prop for name, (prop, _) in table.items()})
    _state["registered"] = True
    _state["table"] = table
    return out


def _build_ops_names():
    """{name: (None, (namespace, attribute) or None)} of every operator _build_ops knows, opt-in ones included"""
    return _state.get("all_ops") or {}


def install(mx=None, stream=None, sync=True, **features):
    """register() + alias the reference's symbol constructors to mx.sym.Custom, e.g.
    mx.sym.contrib.ROIAlign_v2(data=d, rois=r, pooled_size=(7,7), spatial_scale=0.25) builds
    mx.sym.Custom(d, r, op_type='sd__contrib_ROIAlign_v2', pooled_size='(7, 7)', ...) and returns
    only the visible outputs, so symbol/builder.py and the config/ graphs stay unchanged.

    The constructor an alias replaces is kept (`<namespace>._sd_reference_<name>`, and on the alias as
    `_sd_original`).  An operator whose prop class has `sd_supports(params)` (DeformableConvolution) hands
    a call with parameters the kernels do not take BACK to that constructor: the node is then the native
    operator, exactly what the graph held without install() (`_state["fallbacks"]` lists them).

    `stream` / `sync`: the hipStream_t every operator launches on (None: the NULL stream; an int; or a callable
    evaluated per call) and whether forward() / backward() synchronise it before they return (the module
    docstring has the ordering contract; sync=False is for a host that orders the outputs on `stream` itself).

    `features`: the keywords of FEATURE_FLAGS, all off by default because each changes which operators existing
    graphs hold; an unknown keyword raises TypeError.  `<flag>=True` also registers and aliases the operators its
    _FEATURES entry gates and, where the entry names builder classes, rebinds their methods (the `patch_*` function of
    the flag says to what) so that the reference's builders emit the device nodes without a reference file being
    edited.  A rebound method keeps the one it replaced on its class as `_sd_reference_<method>` (a second install()
    keeps the first) and hands a call the device op does not take, or whose op is not registered, back to it;
    `_state["fallbacks"]` says why, and also where a flag's builder module is not importable and nothing was rebound
    (for the flags whose entry has a fallback).  `_state["<flag>_patched"]` tells whether the methods were rebound.
    A default install() afterwards puts things back: the native constructors, the reference's methods, and no
    `_sd_reference_<method>` left on a builder class.  One line per flag sits in _FEATURES; INTEGRATION.md has the
    operators' arguments, limits and the reference lines they stand for."""
    flags = _feature_flags(features)
    props = register(mx, **flags)
    mx = _state["mx"]
    for feature in _FEATURES.values():
        if not feature.builders and feature.state:        # what patch_mxnext reads
            _state[feature.state] = flags[feature.flag]
    _state["fallbacks"] = []
    _state["stream"], _state["sync"] = stream, bool(sync)

    def record(*fallback):
        _state["fallbacks"].append(fallback)

    for name, (_, where) in _state["table"].items():
        if where is not None:
            # (cache_col is this adapter's own attribute of DeformableConvolution: no native constructor sees it)
            put_alias(mx, *where, lambda original: alias_ctor(mx, name, props[name], original, record,
                                                              native_drop=("cache_col",)))
    # an alias an earlier opt-in install() left for an operator that is not in the table now: the constructor it
    # replaced is put back
    for name, (_, where) in _build_ops_names().items():
        if where is not None and name not in _state["table"]:
            drop_alias(mx, *where)
    # the fused FPN extractor has no single reference symbol to alias: rebind the builder method
    # that emits the subgraph (no reference file is edited)
    _state["fpn_patched"] = patch_fpn_roi_align(mx=mx)
    # ... and the mxnext wrappers the reference's builders go through, explicitly (not relying on
    # mxnext looking `mx.sym.*` up at call time)
    _state["mxnext_patched"] = patch_mxnext(mx=mx)
    for feature in _FEATURES.values():
        if not feature.builders:
            continue
        if flags[feature.flag]:
            _state[feature.state] = _rebind(feature, mx=mx)
            if feature.fallback and not _state[feature.state]:
                name, why = feature.fallback
                _state["fallbacks"].append((name, None, why % feature.builders[0]))
        else:   # a default install() after an opt-in one builds the reference's nodes again
            for module in feature.builders:
                if sys.modules.get(module) is not None:
                    _restore(feature, sys.modules[module])
            _state[feature.state] = False
    return props


# ---------------------------------------------------------------------------- opt-in features ----
# One entry of _FEATURES (at the end of this section) per opt-in flag of register() / install():
#   flag      the keyword;                      summary   the flag's line of documentation
#   ops       the _build_ops names it gates;    state     the _state key install() reports it under
#   builders  the reference module(s) whose classes it rebinds;  methods  the (class, method) pairs in each of them
#   maker     maker(mx, builder_module, originals) -> the replacement methods, in the order of `methods`
#   fallback  (operator, "... %s ..." over builders[0]) recorded in _state["fallbacks"] when nothing was rebound
#   lenient   any exception from importing a builder module means "not there" (bbox_post alone)
_Feature = collections.namedtuple("_Feature", "flag ops summary state builders methods maker fallback lenient",
                                  defaults=(None, (), (), None, None, False))


def _import_builder(name, lenient=False):
    """The reference module `name`, or None where the reference tree is not on the path: a ModuleNotFoundError for
    the module or one of its parent packages.  A missing dependency OF the builder, or any other error raised inside
    it, is the caller's to see -- unless `lenient`."""
    try:
        return importlib.import_module(name)
    except Exception as e:
        if lenient or (isinstance(e, ModuleNotFoundError) and e.name is not None and name.startswith(e.name)):
            return None
        raise


def _rebind(feature, builder_module=None, mx=None):
    """Put the feature's replacement methods on its builder classes: in `builder_module`, or in every module of
    feature.builders that imports.  False where a class is missing (nothing is touched then).  The method a
    replacement stands for is kept on its class as `_sd_reference_<method>`; a second call keeps the first one."""
    mx = mx or _state["mx"]
    if builder_module is None:
        modules = [_import_builder(name, feature.lenient) for name in feature.builders]
        return any([_rebind(feature, module, mx) for module in modules if module is not None])
    classes = [getattr(builder_module, c, None) for c, _ in feature.methods]
    if any(c is None for c in classes):
        return False
    originals = [c.__dict__.get("_sd_reference_" + m) or getattr(c, m) for c, (_, m) in zip(classes, feature.methods)]
    replacements = feature.maker(mx, builder_module, originals)
    for c, (_, m), original, fn in zip(classes, feature.methods, originals, replacements):
        fn.__name__ = m
        setattr(c, "_sd_reference_" + m, original)
        setattr(c, m, fn)
    return True


def _restore(feature, builder_module):
    """Put the reference's methods back and forget them: the classes are as they were.  True when one was restored."""
    done = False
    for cname, m in feature.methods:
        cls = getattr(builder_module, cname, None)
        original = cls.__dict__.get("_sd_reference_" + m) if cls is not None else None
        if original is not None:
            setattr(cls, m, original)
            delattr(cls, "_sd_reference_" + m)
            done = True
    return done


def _fell_back(name, why):
    """records in _state["fallbacks"] why (if at all) a rebound method hands this call to the reference's; returns why"""
    if why:
        _state.setdefault("fallbacks", []).append((name, None, why))
    return why


def _registered(name, why=None):
    """whether install() registered sd_<name>; if not, the fallback is recorded (`why`: a feature's own wording)"""
    if name in (_state.get("table") or {}):
        return True
    _fell_back(name, why or "%s%s is not registered" % (_PREFIX, name))
    return False


_CROWDHUMAN_METHODS = (("FPNRpnHeadwithIgnore", "get_sampled_proposal"), ("DoublePredFPNRpnHead", "get_sampled_proposal"),
                       ("DoublePredBboxHead", "emd_loss"))


def _crowdhuman_methods(mx, builder_module, originals):
    def reshape(sym):
        X = getattr(builder_module, "X", None)       # the builder's own `import mxnext as X`
        return X.reshape(sym, (-3, -2)) if X is not None else mx.sym.reshape(sym, shape=(-3, -2))

    def sampled(op, original):
        def get_sampled_proposal(self, conv_fpn_feat, gt_bbox, im_info):
            if not _registered(op):
                return original(self, conv_fpn_feat, gt_bbox, im_info)
            p = self.p
            (proposal, proposal_score) = self.get_all_proposal(conv_fpn_feat, im_info)
            sym = mx.sym.Custom(
                proposal=proposal, gt_bbox=gt_bbox, op_type=_PREFIX + op, name="subsample_proposal",
                num_class=_param_str(p.bbox_target.num_reg_class),
                add_gt_to_proposal=_param_str(not p.subsample_proposal.proposal_wo_gt),
                image_rois=_param_str(p.subsample_proposal.image_roi),
                fg_fraction=_param_str(p.subsample_proposal.fg_fraction),
                fg_thresh=_param_str(p.subsample_proposal.fg_thr),
                bg_thresh_hi=_param_str(p.subsample_proposal.bg_thr_hi),
                bg_thresh_lo=_param_str(p.subsample_proposal.bg_thr_lo),
                bbox_target_std=_param_str(p.bbox_target.std))
            return (sym[0],) + tuple(reshape(sym[i]) for i in range(1, 7 if op == "doublebbox_target" else 4))
        return get_sampled_proposal

    def emd_loss(self, cls_logit, cls_label, cls_sec_logit, cls_sec_label, bbox_delta, bbox_target, bbox_sec_delta,
                 bbox_sec_target, bbox_weight, bbox_sec_weight, prefix=""):
        if not _registered("emd_loss"):
            return originals[2](self, cls_logit, cls_label, cls_sec_logit, cls_sec_label, bbox_delta, bbox_target,
                                bbox_sec_delta, bbox_sec_target, bbox_weight, bbox_sec_weight, prefix=prefix)
        p = self.p
        smooth_l1_scalar = p.regress_target.smooth_l1_scalar or 1.0
        scale_loss_shift = 128.0 if p.fp16 else 1.0
        return mx.sym.Custom(cls_logit=cls_logit, cls_sec_logit=cls_sec_logit, cls_label=cls_label,
                             cls_sec_label=cls_sec_label, bbox_delta=bbox_delta, bbox_sec_delta=bbox_sec_delta,
                             bbox_target=bbox_target, bbox_sec_target=bbox_sec_target, bbox_weight=bbox_weight,
                             bbox_sec_weight=bbox_sec_weight, op_type=_PREFIX + "emd_loss",
                             smooth_l1_scalar=_param_str(smooth_l1_scalar),
                             grad_scale=_param_str(1.0 * scale_loss_shift), name=prefix + "cls_reg_loss")

    return [sampled("bbox_target", originals[0]), sampled("doublebbox_target", originals[1]), emd_loss]


def patch_crowdhuman(builder_module=None, mx=None):
    """Route the CrowdHuman train head to the device ops WITHOUT editing the reference: rebinds, in
    models/crowdhuman/builder.py,
      FPNRpnHeadwithIgnore.get_sampled_proposal (:360-400) and DoublePredFPNRpnHead.get_sampled_proposal (:406-450) to
        methods that read the same fields of `self.p`, call the reference's own `self.get_all_proposal` and emit
        mx.sym.Custom(op_type='sd_bbox_target' / 'sd_doublebbox_target', name='subsample_proposal') with the
        reference's parameters, followed by the reference's reshapes; the return tuples are the reference's;
      DoublePredBboxHead.emd_loss (:254-306) to a method of the same signature that emits ONE
        mx.sym.Custom(op_type='sd_emd_loss', name=prefix + 'cls_reg_loss') with smooth_l1_scalar =
        p.regress_target.smooth_l1_scalar or 1.0 and grad_scale = 128.0 if p.fp16 else 1.0.
    install(crowdhuman=True) calls this when the builder module is importable; returns True when the three methods
    were rebound.  The originals are kept as `_sd_reference_<method>` (a second install() keeps the first ones); a
    default install() afterwards puts them back (unpatch_crowdhuman)."""
    return _rebind(_FEATURES["crowdhuman"], builder_module, mx)


def unpatch_crowdhuman(builder_module):
    """Put the reference's three methods back (and forget them: the classes are as they were)."""
    return _restore(_FEATURES["crowdhuman"], builder_module)


def _bbox_post_methods(mx, builder_module, originals):
    def get_post_processing(self, cls_score, bbox_xyxy):
        p = self.p
        params = {"max_det_per_image": _param_str(p.max_det_per_image),
                  "min_det_score": _param_str(p.min_det_score), "nms_type": _param_str(p.nms.type),
                  "nms_thr": _param_str(p.nms.thr)}
        if not _registered("BboxPostProcessing") or \
                _fell_back("BboxPostProcessing", _state["table"]["BboxPostProcessing"][0].sd_supports(params)):
            return originals[0](self, cls_score, bbox_xyxy)
        sym = mx.sym.Custom(cls_score=cls_score, bbox_xyxy=bbox_xyxy, op_type=_PREFIX + "BboxPostProcessing",
                            **params)
        return sym[0], sym[1], sym[2]

    return [get_post_processing]


def patch_bbox_post(builder_module=None, mx=None):
    """Route Mask R-CNN's test-time post-processing to the device op WITHOUT editing the reference: rebinds
    `BboxPostProcessor.get_post_processing` of models/maskrcnn/builder.py:69-84 (and of its copy in
    models/msrcnn/builder.py:174-189), which emits mx.sym.Custom(op_type='BboxPostProcessing'), to a method that
    emits mx.sym.Custom(op_type='sd_BboxPostProcessing') over the same inputs with the same four parameters and
    returns the same three symbols.  install(bbox_post=True) calls this for the builder modules that are
    importable; returns True when a class was patched.  The original method is kept as
    `_sd_reference_get_post_processing` (a second install() keeps the first original) and is what a call the
    kernels do not take goes back to."""
    return _rebind(_FEATURES["bbox_post"], builder_module, mx)


def unpatch_bbox_post(builder_module):
    """Put the reference's get_post_processing back."""
    return _restore(_FEATURES["bbox_post"], builder_module)


def _mask_loss_methods(mx, builder_module, originals):
    def get_loss(self, conv_feat, mask_target, mask_ind):
        if not _registered("MaskLoss"):
            return originals[0](self, conv_feat, mask_target, mask_ind)
        mask_fcn_logit = self.get_output(conv_feat)
        scale_loss_shift = 128.0 if self.pMask.fp16 else 1.0
        sym = mx.sym.Custom(logits=mask_fcn_logit, cls=mask_ind, target=mask_target, op_type=_PREFIX + "MaskLoss",
                            grad_scale=_param_str(1.0 * scale_loss_shift), name="mask_loss")
        return (sym[0],)

    return [get_loss]


def patch_mask_loss(builder_module=None, mx=None):
    """Route Mask R-CNN's mask loss to the fused device op WITHOUT editing the reference: rebinds
    `MaskFasterRcnnHead.get_loss` of models/maskrcnn/builder.py:278-313 -- which splits the logits per image,
    builds stack(arange, mask_ind), gathers every RoI's class plane with gather_nd, concatenates, reshapes to
    (1, -1) and calls mx.sym.contrib.SigmoidCrossEntropy -- to a method that calls `self.get_output(conv_feat)` and
    emits ONE mx.sym.Custom(op_type='sd_MaskLoss') over (mask_fcn_logit, mask_ind, mask_target) with
    grad_scale = 128.0 if pMask.fp16 else 1.0, and returns `(mask_loss,)`.  The backward of that node writes the
    dense logits gradient once instead of a zero fill, a scatter and the backward of concat and split.
    install(mask_loss=True) calls this when the builder module is importable; returns True when the class was
    patched.  The original method is kept as `_sd_reference_get_loss` (a second install() keeps the first
    original); a default install() afterwards puts it back (unpatch_mask_loss).
    models/msrcnn/builder.py is NOT patched by this flag: its get_loss also returns the gathered sigmoid (the MaskIoU
    head reads it), so it keeps its subgraph and gets the aliased SigmoidCrossEntropy only; install(msrcnn=True)
    (patch_msrcnn_loss) is what moves that model's head onto the device."""
    return _rebind(_FEATURES["mask_loss"], builder_module, mx)


def unpatch_mask_loss(builder_module):
    """Put the reference's get_loss back."""
    return _restore(_FEATURES["mask_loss"], builder_module)


def _msrcnn_methods(mx, builder_module, originals):
    def mask_get_loss(self, conv_feat, mask_target, mask_ind):
        if not _registered("MsrcnnMaskLoss"):
            return originals[0](self, conv_feat, mask_target, mask_ind)
        mask_fcn_logit = self.get_output(conv_feat)
        scale_loss_shift = 128.0 if self.pMask.fp16 else 1.0
        sym = mx.sym.Custom(logits=mask_fcn_logit, cls=mask_ind, target=mask_target,
                            op_type=_PREFIX + "MsrcnnMaskLoss", grad_scale=_param_str(1.0 * scale_loss_shift),
                            name="mask_loss")
        return (sym[0],), sym[1]

    def iou_get_loss(self, conv_feat, mask_pred_logits, mask_target, mask_inds, mask_ratio):
        if not _registered("MaskIoULoss"):
            return originals[1](self, conv_feat, mask_pred_logits, mask_target, mask_inds, mask_ratio)
        iou_pred_logits = self._get_output(mask_pred_logits, conv_feat)
        sym = mx.sym.Custom(iou_pred=iou_pred_logits, prob=mask_pred_logits, target=mask_target, ratio=mask_ratio,
                            cls=mask_inds, op_type=_PREFIX + "MaskIoULoss", grad_scale=_param_str(1.0),
                            name="iou_head_loss")
        return (sym[0],)

    return [mask_get_loss, iou_get_loss]


def patch_msrcnn_loss(builder_module=None, mx=None):
    """Route Mask Scoring R-CNN's training head to the device ops WITHOUT editing the reference: rebinds, in
    models/msrcnn/builder.py,
      MaskFasterRcnnHead.get_loss (:383-424) -- split / stack / gather_nd / concat, Activation(sigmoid), two reshapes
        and SigmoidCrossEntropy -- to a method that calls `self.get_output(conv_feat)` and emits ONE
        mx.sym.Custom(op_type='sd_MsrcnnMaskLoss') over (mask_fcn_logit, mask_ind, mask_target) with
        grad_scale = 128.0 if pMask.fp16 else 1.0, and returns `((mask_loss,), mask_pred_prob)`;
      MaskIoUConvHead.get_loss (:143-168) -- the same gather chain on the IoU predictions, the Python CustomOp
        maskiou_compute, two BlockGrads and the loss arithmetic under MakeLoss -- to a method that calls the
        reference's own `self._get_output(mask_pred_logits, conv_feat)` and emits ONE
        mx.sym.Custom(op_type='sd_MaskIoULoss') over (iou_pred, mask_pred_logits, mask_target, mask_ratio, mask_inds)
        with grad_scale = 1.0, and returns `(maskiou_head_loss,)`.
    Signatures and return shapes are the reference's.  install(msrcnn=True) calls this when the builder module is
    importable; returns True when both classes were patched.  The original methods are kept as
    `_sd_reference_get_loss` (a second install() keeps the first originals); a default install() afterwards puts
    them back (unpatch_msrcnn_loss)."""
    return _rebind(_FEATURES["msrcnn"], builder_module, mx)


def unpatch_msrcnn_loss(builder_module):
    """Put the reference's two get_loss methods back (and forget them: the classes are as they were)."""
    return _restore(_FEATURES["msrcnn"], builder_module)


_FCOS_CONFIG = "config.fcos_r50v1_fpn_1x"     # where the reference's own CustomOpProps read throwout_param (input.py:88)


def _fcos_level_inputs(head, conv_fpn_feat):
    """(strides, {cls_logit_i, centerness_logit_i, offset_logit_i: the head's per-level outputs}): the first 3 * L
    inputs of sd_fcos_loss and sd_fcos_decode, in their order"""
    centerness_logit_dict, cls_logit_dict, offset_logit_dict = head.get_output(conv_fpn_feat)
    strides = tuple(head.p.FCOSParam.stride)
    inputs = {}
    for prefix, d in (("cls_logit_%d", cls_logit_dict), ("centerness_logit_%d", centerness_logit_dict),
                      ("offset_logit_%d", offset_logit_dict)):
        for i, stride in enumerate(strides):
            inputs[prefix % i] = d[stride]
    return strides, inputs


def _fcos_loss_methods(mx, builder_module, originals):
    def get_loss(self, conv_fpn_feat, gt_bbox, im_info):
        throwout = getattr(sys.modules.get(_FCOS_CONFIG), "throwout_param", None)
        if not _registered("fcos_loss", "sd_fcos_target / sd_fcos_loss are not registered") or \
                _fell_back("fcos_loss", "%s.throwout_param is not set" % _FCOS_CONFIG if throwout is None else ""):
            return originals[0](self, conv_fpn_feat, gt_bbox, im_info)
        p = self.p
        strides, inputs = _fcos_level_inputs(self, conv_fpn_feat)
        ignore = {"ignore_offset": _param_str(p.loss_setting.ignore_offset),
                  "ignore_label": _param_str(p.loss_setting.ignore_label)}
        # the reference binds the two inputs by name as well (builder.py:193-194)
        targets = mx.sym.Custom(gt_bbox=mx.sym.var("gt_bbox"), im_info=mx.sym.var("im_info"),
                                op_type=_PREFIX + "fcos_target", name="fcos_target",
                                data_size=_param_str(tuple(throwout.data_size)), stride=_param_str(tuple(throwout.stride)),
                                num_classifier=_param_str(p.FCOSParam.num_classifier), **ignore)
        for i, name in enumerate(("centerness", "offset", "cls_id", "state")):
            inputs[name] = targets[i]
        loss = mx.sym.Custom(op_type=_PREFIX + "fcos_loss", name="fcos_loss", num_levels=_param_str(len(strides)),
                             alpha=_param_str(p.loss_setting.focal_loss_alpha),
                             gamma=_param_str(p.loss_setting.focal_loss_gamma), **ignore, **inputs)
        return loss[0], loss[1], loss[2]

    return [get_loss]


def patch_fcos_loss(builder_module=None, mx=None):
    """Route the FCOS training head to the device ops WITHOUT editing the reference: rebinds
    `FCOSFPNHead.get_loss` of models/FCOS/builder.py:181-231 -- make_fcos_gt (two Python CustomOps and ~60 nodes),
    five reshapes and a concat per logit tensor, and three loss subgraphs behind compute_focal_loss /
    compute_bce_loss / MakeLoss -- to a method that calls `self.get_output(conv_fpn_feat)` and emits
        sd_fcos_target(gt_bbox, im_info) -> sd_fcos_loss(the 3 * L per-level tensors, the four targets)
    and returns `(centerness_loss, cls_loss, offset_loss)`, the reference's order.  The parameters come from where
    the reference reads them: data_size and stride from config.fcos_r50v1_fpn_1x.throwout_param at call time
    (input.py:88-91), ignore_offset / ignore_label / focal_loss_alpha / focal_loss_gamma from p.loss_setting,
    num_classifier and the level order from p.FCOSParam.  install(fcos=True) calls this when the builder module is
    importable; returns True when the class was patched.  The original method is kept as `_sd_reference_get_loss`
    (a second install() keeps the first original); a default install() afterwards puts it back."""
    return _rebind(_FEATURES["fcos"], builder_module, mx)


def unpatch_fcos_loss(builder_module):
    """Put the reference's get_loss back."""
    return _restore(_FEATURES["fcos"], builder_module)


def _fcos_decode_methods(mx, builder_module, originals):
    def get_all_proposal(self, conv_fpn_feat, im_info):
        if not _registered("fcos_decode"):
            return originals[0](self, conv_fpn_feat, im_info)
        p = self.p
        strides, inputs = _fcos_level_inputs(self, conv_fpn_feat)
        inputs["im_info"] = im_info
        out = mx.sym.Custom(op_type=_PREFIX + "fcos_decode", name="fcos_decode", stride=_param_str(strides),
                            pre_nms_top_n=_param_str(int(p.proposal.pre_nms_top_n)),
                            pre_nms_thresh=_param_str(p.proposal.pre_nms_thresh), input_logits="1", **inputs)
        bboxes, score = out[0], out[1]
        self._proposal = score, bboxes
        return score, bboxes

    return [get_all_proposal]


def patch_fcos_decode(builder_module=None, mx=None):
    """Route the FCOS test-time decode to the device op WITHOUT editing the reference: rebinds
    `FCOSFPNHead.get_all_proposal` of models/FCOS/builder.py:234-259 -- ten sigmoid nodes, five Python CustomOps
    get_proposal_single_stage, a concat and the Python CustomOp get_batch_proposal -- to a method that calls
    `self.get_output(conv_fpn_feat)` and emits
        sd_fcos_decode(the 3 * L per-level tensors: raw class and centerness logits, offsets; im_info)
    with input_logits = 1, sets `self._proposal` and returns `(score, bboxes)` as the reference does.  pre_nms_top_n and
    pre_nms_thresh come from p.proposal, the strides and the level order from p.FCOSParam.stride.
    install(fcos_decode=True) calls this when the builder module is importable; returns True when the class was
    patched.  The original method is kept as `_sd_reference_get_all_proposal` (a second install() keeps the first
    original); a default install() afterwards puts it back."""
    return _rebind(_FEATURES["fcos_decode"], builder_module, mx)


def unpatch_fcos_decode(builder_module):
    """Put the reference's get_all_proposal back."""
    return _restore(_FEATURES["fcos_decode"], builder_module)


def _reppoints_unsupported(p):
    """why the device ops do not take this head, or ''"""
    if p.fp16:
        return "fp16: the device ops are float32"
    if not 1 <= len(p.point_generate.stride) <= 8:
        return "%d levels, the limit is 8" % len(p.point_generate.stride)
    if p.point_generate.num_points not in (1, 9, 25):
        return "num_points=%s is not the square of an odd number up to 25" % (p.point_generate.num_points,)
    if p.point_generate.transform not in ("minmax", "partial_minmax", "moment"):
        return "transform=%s" % (p.point_generate.transform,)
    if not 1 <= int(p.point_target.num_pos) <= 16:
        return "num_pos=%s lies outside 1..16" % (p.point_target.num_pos,)
    return ""


def _reppoints_loss_methods(mx, builder_module, originals):
    def get_loss(self, conv_feat, gt_bbox):
        p = self.p
        if not _registered("reppoints_box_loss", "sd_reppoints_target / sd_reppoints_box_loss are not registered") or \
                _fell_back("reppoints_box_loss", _reppoints_unsupported(p)):
            return originals[0](self, conv_feat, gt_bbox)
        X = builder_module.X                         # the builder's own `import mxnext as X`
        stride = tuple(p.point_generate.stride)
        pts_out_inits, pts_out_refines, cls_outs = self.get_output(conv_feat)
        geometry = {"stride": _param_str(stride), "num_points": _param_str(p.point_generate.num_points),
                    "transform": _param_str(p.point_generate.transform)}
        inputs = {"pts_init_%d" % i: X.block_grad(pts_out_inits["stride%s" % s]) for i, s in enumerate(stride)}
        targets = mx.sym.Custom(op_type=_PREFIX + "reppoints_target", name="reppoints_target", **inputs,
                                gt_bbox=gt_bbox, moment_transfer=self.moment_transfer, **geometry,
                                target_scale=_param_str(p.point_target.target_scale),
                                num_pos=_param_str(p.point_target.num_pos),
                                pos_iou_thr=_param_str(p.bbox_target.pos_iou_thr),
                                neg_iou_thr=_param_str(p.bbox_target.neg_iou_thr),
                                min_pos_iou=_param_str(p.bbox_target.min_pos_iou))
        points_labels_refine = targets[2]
        # cls branch (builder.py:390-413), unchanged
        cls_flat = [X.reshape(X.transpose(data=cls_outs["stride%s" % s], axes=(0, 2, 3, 1)), (0, -3, -2)) for s in stride]
        cls_outs_concat = X.concat(cls_flat, axis=1, name="cls_concat")
        cls_loss = X.focal_loss(data=cls_outs_concat, label=points_labels_refine, normalization='valid',
                                alpha=p.focal_loss.alpha, gamma=p.focal_loss.gamma, grad_scale=1.0, workspace=1500,
                                name="cls_loss")
        inputs = {"pts_init_%d" % i: pts_out_inits["stride%s" % s] for i, s in enumerate(stride)}
        inputs.update({"pts_refine_%d" % i: pts_out_refines["stride%s" % s] for i, s in enumerate(stride)})
        inputs["moment_transfer"] = self.moment_transfer
        for i, name in enumerate(("label_init", "gt_init", "label_refine", "gt_refine", "state")):
            inputs[name] = targets[i]
        loss = mx.sym.Custom(op_type=_PREFIX + "reppoints_box_loss", name="reppoints_box_loss", **inputs, **geometry,
                             scale=_param_str(p.point_generate.scale), grad_scale_init="0.5", grad_scale_refine="1.0")
        points_init_labels = X.block_grad(points_labels_refine, name="points_init_labels")
        points_refine_labels = X.block_grad(points_labels_refine, name="point_refine_labels")
        return cls_loss, loss[0], loss[1], points_init_labels, points_refine_labels

    return [get_loss]


def patch_reppoints_loss(builder_module=None, mx=None):
    """Route the RepPoints training head to the device ops WITHOUT editing the reference: rebinds
    `RepPointsHead.get_loss` of models/RepPoints/builder.py:311-484 -- per level _gen_points, _offset_to_boxes and two
    _offset_to_pts, per image _point_assign and _iou_assign, three _points2bbox, two smooth_l1 / BBoxNorm / MakeLoss
    chains -- to a method that calls `self.get_output(conv_feat)` and emits
        sd_reppoints_target(the L init point maps, gt_bbox, moment_transfer)
        sd_reppoints_box_loss(the L init and L refine point maps, moment_transfer, the five targets)
    and keeps the class branch as it is: the per-level transpose and reshape, the concat and X.focal_loss on
    label_refine.  Every parameter is read from self.p as the reference reads it.  Returns the reference's five
    outputs in order: cls_loss, pts_init_loss, pts_refine_loss and label_refine twice behind BlockGrad.  A head
    with p.fp16 set, or beyond the limits of the device ops, goes back to the original method
    (`_state["fallbacks"]` records why).  install(reppoints=True) calls this when the builder module is importable;
    returns True when the class was patched.  The original is kept as `_sd_reference_get_loss` (a second install()
    keeps the first original); a default install() afterwards puts it back."""
    return _rebind(_FEATURES["reppoints"], builder_module, mx)


def unpatch_reppoints_loss(builder_module):
    """Put the reference's get_loss back."""
    return _restore(_FEATURES["reppoints"], builder_module)


def _reppoints_decode_unsupported(p):
    """why the device op does not take this head's test graph, or ''"""
    if p.fp16:
        return "fp16: the device op is float32"
    if not 1 <= len(p.point_generate.stride) <= 8:
        return "%d levels, the limit is 8" % len(p.point_generate.stride)
    if p.point_generate.transform not in ("minmax", "partial_minmax", "moment"):
        return "transform=%s" % (p.point_generate.transform,)
    if int(p.proposal.pre_nms_top_n) > 16384:
        return "pre_nms_top_n=%s, the limit is 16384" % (p.proposal.pre_nms_top_n,)
    return ""


def _reppoints_decode_methods(mx, builder_module, originals):
    def get_prediction(self, conv_feat, im_info):
        p = self.p
        if not _registered("reppoints_decode") or _fell_back("reppoints_decode", _reppoints_decode_unsupported(p)):
            return originals[0](self, conv_feat, im_info)
        stride = tuple(p.point_generate.stride)
        _, pts_out_refines, cls_outs = self.get_output(conv_feat)
        inputs = {"cls_logit_%d" % i: cls_outs["stride%s" % s] for i, s in enumerate(stride)}
        inputs.update({"pts_refine_%d" % i: pts_out_refines["stride%s" % s] for i, s in enumerate(stride)})
        out = mx.sym.Custom(op_type=_PREFIX + "reppoints_decode", name="reppoints_decode", **inputs, im_info=im_info,
                            moment_transfer=self.moment_transfer, stride=_param_str(stride),
                            pre_nms_top_n=_param_str(int(p.proposal.pre_nms_top_n)),
                            transform=_param_str(p.point_generate.transform),
                            num_points=_param_str(p.point_generate.num_points), input_logits="1")
        return out[0], out[1]

    return [get_prediction]


def patch_reppoints_decode(builder_module=None, mx=None):
    """Route the RepPoints test-time decode to the device op WITHOUT editing the reference: rebinds
    `RepPointsHead.get_prediction` of models/RepPoints/builder.py:486-576 -- per level _gen_points, _points2bbox, two
    transposes and reshapes, sigmoid, max and topk, per image the slice / reshape / take / concat / scale / add / clip
    chains, then stack, the padded column and the concat of the levels -- to a method that calls
    `self.get_output(conv_feat)` and emits
        sd_reppoints_decode(the L raw class logit maps, the L pts_out_refine maps, im_info, moment_transfer)
    with input_logits = 1 and returns `(cls_score, bbox_xyxy)` as the reference does.  stride, transform and num_points
    come from p.point_generate, pre_nms_top_n from p.proposal; the rule that keeps every location of a level with a
    stride above 32 (builder.py:499-502) is the op's.  A head with p.fp16 set, or beyond the limits of the op, goes
    back to the original method (`_state["fallbacks"]` records why).  install(reppoints_decode=True) calls this when
    the builder module is importable; returns True when the class was patched.  The original method is kept as
    `_sd_reference_get_prediction` (a second install() keeps the first original); a default install() afterwards
    puts it back."""
    return _rebind(_FEATURES["reppoints_decode"], builder_module, mx)


def unpatch_reppoints_decode(builder_module):
    """Put the reference's get_prediction back."""
    return _restore(_FEATURES["reppoints_decode"], builder_module)


def _tsd_pool_methods(mx, builder_module, originals):
    def make(original, tag, per_roi):
        def get_roi_feature(self, conv_fpn_feat, rois, trans, image_rois, batch_image):
            if not _registered("fpn_deform_roi_pool"):
                return original(self, conv_fpn_feat, rois, trans, image_rois, batch_image)
            p = self.p
            strides = tuple(int(s) for s in p.stride)
            out = int(p.out_size)
            fp16 = bool(getattr(p, "fp16", False))
            feats = []
            for s_ in strides:
                f = conv_fpn_feat["stride%s" % s_]
                if fp16:
                    f = mx.sym.Cast(data=f, dtype="float32", name="fpn_stride%s_to_fp32" % s_)
                feats.append(f)
            tr = mx.sym.reshape(data=trans, shape=(-1, 2) if per_roi else (-1, 2, out, out),
                                name=tag + "_offset_reshape")
            # sample_per_part 4, trans_std 0.1: the constants of poolings.py:96-97, 160-161
            sym = mx.sym.Custom(*feats, rois, tr, op_type=_PREFIX + "fpn_deform_roi_pool",
                                rcnn_stride=_param_str(strides), pooled_size=_param_str(out), sample_per_part="4",
                                trans_std="0.1", roi_canonical_scale=_param_str(p.roi_canonical_scale),
                                roi_canonical_level=_param_str(p.roi_canonical_level), name=tag + "_pooled_feat")
            roi_feat = sym[0]
            if fp16:
                roi_feat = mx.sym.Cast(data=roi_feat, dtype="float16", name=tag + "_roi_feat_to_fp16")
            return roi_feat
        return get_roi_feature

    return [make(originals[0], "delta_c", False), make(originals[1], "delta_r", True)]


def patch_tsd_pool(builder_module=None, mx=None):
    """Route TSD's two RoI extractors to the fused op WITHOUT editing the reference: rebinds
    `FPNRoIAlign_DeltaC.get_roi_feature` and `FPNRoIAlign_DeltaR.get_roi_feature` of models/TSD/poolings.py:51-174
    (fpn_roi_assign_offset -> per stride the masked rois and offsets, a concat with the batch column and
    DeformablePSROIPooling -> add_n) to a method that emits ONE
        sd_fpn_deform_roi_pool(the level features, rois (B,R,4), trans reshaped to (B*R,2,P,P) | (B*R,2))
    node and returns the same (B*R, C, out, out) symbol (fp16 graphs: cast to fp32 before, back to fp16 after, as
    :71-76, 104-105).  get_roi_feature_test calls get_roi_feature (:109-110, 173-174), so test graphs follow.
    install(tsd_pool=True) calls this when the module is importable; returns True when both classes were patched.
    The originals are kept as `_sd_reference_get_roi_feature`; a default install() afterwards puts them back."""
    return _rebind(_FEATURES["tsd_pool"], builder_module, mx)


def unpatch_tsd_pool(builder_module):
    """Put the reference's two get_roi_feature methods back."""
    return _restore(_FEATURES["tsd_pool"], builder_module)


# The opt-in features, in the order install() handles them (the order of their _state["fallbacks"] entries).  Two
# differences between the entries are kept on purpose: only the features from fcos_decode on record a fallback when
# their builder is not importable (bbox_post, mask_loss and fcos never did, and default users would see new entries),
# and bbox_post alone imports leniently (a msrcnn builder that fails to import for a reason of its own must not break
# install(bbox_post=True) for Mask R-CNN).
_FEATURES = {f.flag: f for f in (
    _Feature("retina", ("_contrib_GenProposalRetina",),
             "RetinaNet's test-time decode (models/retinanet/builder.py:358-389) in place of the native operator; "
             "iou_loss / batch_wise_anchor calls stay native"),
    _Feature("proposal", ("_contrib_Proposal_v2", "_contrib_Proposal"),
             "the TridentNet / C4 proposal operators in place of the native ones, and X.proposal where mxnext builds "
             "_contrib_Proposal", state="proposal"),
    _Feature("bbox_post", ("BboxPostProcessing",),
             "Mask R-CNN's and Mask Scoring R-CNN's test-time per-class NMS in place of the reference's numpy CustomOp",
             state="bbox_post_patched", builders=("models.maskrcnn.builder", "models.msrcnn.builder"),
             methods=(("BboxPostProcessor", "get_post_processing"),), maker=_bbox_post_methods, lenient=True),
    _Feature("retina_loss", ("_contrib_FocalLoss", "_contrib_BBoxNorm"),
             "the RetinaNet / RepPoints train losses in place of the native operators, and X.focal_loss / X.bbox_norm",
             state="retina_loss"),
    _Feature("group_norm", ("_contrib_GroupNorm",),
             "the normaliser of the GN Mask R-CNN, RepPoints and EfficientNet graphs in place of the native operator, "
             "and X.group_norm where mxnext has one", state="group_norm"),
    _Feature("mask_loss", ("_contrib_SigmoidCrossEntropy", "MaskLoss"),
             "the aliased SigmoidCrossEntropy, and ONE fused node in place of Mask R-CNN's mask-loss subgraph",
             state="mask_loss_patched", builders=("models.maskrcnn.builder",),
             methods=(("MaskFasterRcnnHead", "get_loss"),), maker=_mask_loss_methods),
    _Feature("quant_int8", ("_contrib_Quantization_int8",),
             "the fake-quantise node utils/graph_optimize.py attaches in the int8 graphs, in place of the native "
             "operator; per-channel weights and other quant / grad modes stay native"),
    _Feature("fcos", ("fcos_target", "fcos_loss"),
             "two nodes in place of the target and loss subgraphs of the FCOS train graph",
             state="fcos_patched", builders=("models.FCOS.builder",), methods=(("FCOSFPNHead", "get_loss"),),
             maker=_fcos_loss_methods),
    _Feature("fcos_decode", ("fcos_decode",),
             "ONE node in place of the sigmoids and the Python CustomOps of the FCOS test graph (independent of fcos)",
             state="fcos_decode_patched", builders=("models.FCOS.builder",),
             methods=(("FCOSFPNHead", "get_all_proposal"),), maker=_fcos_decode_methods,
             fallback=("fcos_decode", "%s.FCOSFPNHead is not importable")),
    _Feature("tsd_pool", ("_contrib_DeformablePSROIPooling", "fpn_deform_roi_pool"),
             "the aliased DeformablePSROIPooling, and ONE fused node per TSD RoI extractor",
             state="tsd_pool_patched", builders=("models.TSD.poolings",),
             methods=(("FPNRoIAlign_DeltaC", "get_roi_feature"), ("FPNRoIAlign_DeltaR", "get_roi_feature")),
             maker=_tsd_pool_methods, fallback=("fpn_deform_roi_pool", "%s is not importable")),
    _Feature("reppoints", ("reppoints_target", "reppoints_box_loss"),
             "two nodes in place of both assigners and both box-loss subgraphs of the RepPoints train graphs",
             state="reppoints_patched", builders=("models.RepPoints.builder",),
             methods=(("RepPointsHead", "get_loss"),), maker=_reppoints_loss_methods,
             fallback=("reppoints_box_loss", "%s.RepPointsHead is not importable")),
    _Feature("msrcnn", ("MsrcnnMaskLoss", "MaskIoULoss"),
             "two nodes in place of the mask-loss and MaskIoU-loss subgraphs of the Mask Scoring R-CNN train graphs "
             "(independent of mask_loss)",
             state="msrcnn_patched", builders=("models.msrcnn.builder",),
             methods=(("MaskFasterRcnnHead", "get_loss"), ("MaskIoUConvHead", "get_loss")), maker=_msrcnn_methods,
             fallback=("MaskIoULoss", "%s is not importable")),
    _Feature("reppoints_decode", ("reppoints_decode",),
             "ONE node in place of the per-level decode subgraphs of the RepPoints test graphs (independent of reppoints)",
             state="reppoints_decode_patched", builders=("models.RepPoints.builder",),
             methods=(("RepPointsHead", "get_prediction"),), maker=_reppoints_decode_methods,
             fallback=("reppoints_decode", "%s.RepPointsHead is not importable")),
    _Feature("crowdhuman", ("bbox_target", "doublebbox_target", "emd_loss"),
             "ONE device target node in place of the Python CustomOp, and ONE node per emd_loss call, in the CrowdHuman "
             "train graphs",
             state="crowdhuman_patched", builders=("models.crowdhuman.builder",), methods=_CROWDHUMAN_METHODS,
             maker=_crowdhuman_methods, fallback=("emd_loss", "%s is not importable")),
)}
FEATURE_FLAGS = tuple(_FEATURES)

def _head_op(mx, sym):
    """(operator name, attrs) of the node behind a symbol: real MXNet through the graph JSON (a
    multi-output symbol's heads all point at one node here), the graph-recording test stub through
    `op_type`.  CustomOps report ('Custom', {'op_type': ...})."""
    if hasattr(sym, "tojson"):
        try:
            import json
            g = json.loads(sym.tojson())
            node = g["nodes"][g["heads"][0][0]]
            return node.get("op"), dict(node.get("attrs", node.get("attr", node.get("param", {}))) or {})
        except Exception:
            pass
    node = sym
    while getattr(node, "op_type", None) in ("_output", "Group"):
        node = node.parent if node.op_type == "_output" else node.inputs[0]
    return getattr(node, "op_type", None), dict(getattr(node, "params", {}) or {})


def _late_contrib(mx, ctor):
    """a wrapper that looks mx.sym.contrib.<ctor> up at call time (positional and keyword inputs pass through)"""
    def wrapper(*a, **kw):
        return getattr(mx.sym.contrib, ctor)(*a, **kw)
    return wrapper


def patch_mxnext(mxnext=None, mx=None):
    """Point the mxnext wrappers on the hot path at the aliased symbol constructors WHERE THAT IS KNOWN TO
    BE A NO-OP FOR THE GRAPH'S MEANING.  mxnext (github.com/RogerChern/mxnext) is not part of the
    reference tree, so which operator a wrapper builds is not assumed: each saved original is called
    once with placeholder Variables and the reference's own keyword arguments, and the operator of the
    node it returns decides --
      * already an `sd_*` Custom node (the wrapper looks `mx.sym.*` up at call time): nothing to do;
      * the native operator this plugin replaces under the same name (`_contrib_ROIAlign_v2`,
        `ProposalTarget`, `_contrib_Proposal_v3`, `_contrib_DecodeBBox`): the wrapper captured the
        constructor before install(); it is rebound to a function with the call sites' signature that
        builds the alias;
      * with install(proposal=True) only: `_contrib_Proposal` for `X.proposal`, rebound to the
        `_contrib_Proposal` alias (the same operator, so the numbers do not change);
      * anything else (`_contrib_Proposal` without the opt-in, `_contrib_Proposal_v2`, `MultiProposal`, a TVM
        op ...), or a probe that raises: LEFT ALONE -- `proposal.cu`, `proposal_v2.cu` and `proposal_v3.cu` differ in the
        +1 box convention, the dw / dh clamp and the min-size filter, rebinding would change the RPN's
        numbers silently.
    Call sites whose signatures the probes use:
        X.roi_align(feat, rois=, out_size=, stride=, name=)      symbol/builder.py:885, models/FPN/builder.py:592
        X.proposal_target(rois=, gt_boxes=, ..., name=)           symbol/builder.py:304, models/FPN/builder.py:347
        X.proposal(cls_prob=, bbox_pred=, im_info=, ..., iou_loss=, output_score=)   symbol/builder.py:241
        X.decode_bbox(rois=, bbox_pred=, im_info=, ..., name=)    symbol/builder.py:384
        mxnext.tvm.get_top_proposal.get_top_proposal(F, bbox=, score=, top_n=, batch_size=)
                                                                  models/FPN/builder.py:319-321
    (mxnext.tvm.proposal -- the "nnvm" proposal some configs select for the fine levels -- is left
    alone: it is un-vendored and nothing in the reference tree pins its results.)
    Returns the list of rebound names ([] when mxnext is not importable); `_state["mxnext_probe"]`
    holds what every probe saw."""
    mx = mx or _state["mx"]
    if mxnext is None:
        try:
            import importlib
            mxnext = importlib.import_module("mxnext")
        except Exception:
            return []
    done = []
    seen = _state["mxnext_probe"] = {}
    V = lambda n: mx.sym.Variable("_sd_probe_" + n)

    def roi_align(feat, rois, out_size, stride, name=None, **kw):
        return mx.sym.contrib.ROIAlign_v2(data=feat, rois=rois, pooled_size=(int(out_size), int(out_size)),
                                          spatial_scale=1.0 / stride, name=name, **kw)

    def proposal_target(**kw):
        return mx.sym.ProposalTarget(**kw)

    def proposal(**kw):
        return mx.sym.contrib.Proposal_v3(**kw)

    def proposal_v1(**kw):
        return mx.sym.contrib.Proposal(**kw)

    def decode_bbox(**kw):
        return mx.sym.contrib.DecodeBBox(**kw)

    # wrapper -> (replacement, the native operator it must turn out to build, a probe call)
    table = {
        "roi_align": (roi_align, "_contrib_ROIAlign_v2",
                      lambda f: f(V("feat"), rois=V("rois"), out_size=7, stride=16, name="_sd_probe")),
        "proposal_target": (proposal_target, "ProposalTarget",
                            lambda f: f(rois=V("rois"), gt_boxes=V("gt"), num_classes=81, class_agnostic=False,
                                        batch_images=1, proposal_without_gt=False, image_rois=64, fg_fraction=0.25,
                                        fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, bbox_weight=(1., 1., 1., 1.),
                                        bbox_mean=(0., 0., 0., 0.), bbox_std=(.1, .1, .2, .2), name="_sd_probe")),
        "proposal": (proposal, "_contrib_Proposal_v3",
                     lambda f: f(cls_prob=V("cls"), bbox_pred=V("box"), im_info=V("info"), name="_sd_probe",
                                 feature_stride=16, scales=(8,), ratios=(0.5, 1.0, 2.0), rpn_pre_nms_top_n=12,
                                 rpn_post_nms_top_n=6, threshold=0.7, rpn_min_size=0, iou_loss=False,
                                 output_score=True)),
        "decode_bbox": (decode_bbox, "_contrib_DecodeBBox",
                        lambda f: f(rois=V("rois"), bbox_pred=V("box"), im_info=V("info"), name="_sd_probe",
                                    bbox_mean=(0., 0., 0., 0.), bbox_std=(.1, .1, .2, .2), class_agnostic=False)),
    }
    for attr, (fn, native, probe) in table.items():
        cur = getattr(mxnext, attr, None)
        if cur is None:
            continue
        orig = cur._sd_original if getattr(cur, "_sd_alias", False) else cur   # (a second install())
        try:
            op, attrs = _head_op(mx, probe(orig))
        except Exception as e:
            seen[attr] = "probe failed: %s" % (e,)
            continue
        short = native[len("_contrib_"):] if native.startswith("_contrib_") else native
        if op == "Custom" and str(attrs.get("op_type", "")).startswith(_PREFIX) or str(op).startswith(_PREFIX):
            seen[attr] = "late binding: already builds %s" % (attrs.get("op_type", op),)
            continue
        if attr == "proposal" and _state.get("proposal") and op in ("_contrib_Proposal", "Proposal"):
            fn, native = proposal_v1, "_contrib_Proposal"  # install(proposal=True): the same operator
        elif op not in (native, short):
            seen[attr] = "builds %s, not %s: left alone" % (op, native)
            continue
        seen[attr] = "builds %s at import-time binding: rebound" % (op,)
        fn._sd_alias, fn._sd_original = True, orig
        try:
            setattr(mxnext, "_sd_reference_" + attr, orig)
            setattr(mxnext, attr, fn)
            done.append("mxnext." + attr)
        except Exception:
            pass
    # install(retina_loss=True): X.focal_loss / X.bbox_norm build the FocalLoss / BBoxNorm aliases at call time.  The
    # wrappers' names pin the operator (models/retinanet/builder.py:296-332 passes the operators' own keyword
    # arguments), so they are bound without a probe; a default install() puts the saved originals back.
    # install(group_norm=True): the same for `X.group_norm` where mxnext has one.  That mxnext's
    # normalizer_factory(type="gn") ends in mx.sym.contrib.GroupNorm, looked up at call time, is inferred: mxnext is
    # not part of the reference tree.
    for attr, ctor, flag in (("focal_loss", "FocalLoss", "retina_loss"), ("bbox_norm", "BBoxNorm", "retina_loss"),
                             ("group_norm", "GroupNorm", "group_norm")):
        try:
            cur = getattr(mxnext, attr)
        except Exception:
            continue
        orig = cur._sd_original if getattr(cur, "_sd_alias", False) else cur
        if not _state.get(flag):
            if cur is not orig:
                setattr(mxnext, attr, orig)
            continue

        loss = _late_contrib(mx, ctor)
        loss.__name__ = attr
        loss._sd_alias, loss._sd_original = True, orig
        setattr(mxnext, "_sd_reference_" + attr, orig)
        setattr(mxnext, attr, loss)
        seen[attr] = "install(%s=True): bound to mx.sym.contrib.%s at call time" % (flag, ctor)
        done.append("mxnext." + attr)
    try:
        import importlib
        m = importlib.import_module("mxnext.tvm.get_top_proposal")
        cur = m.get_top_proposal
        orig = cur._sd_original if getattr(cur, "_sd_alias", False) else cur

        def get_top_proposal(F, bbox, score, top_n, batch_size=None, name="get_top_proposal", **kw):
            # TWO results, (bbox, score), as every call site unpacks them: models/FPN/builder.py:319-323 returns
            # the wrapper's result from get_all_proposal(), and :345 (and symbol/builder.py:36,92,302,
            # models/maskrcnn/builder.py:113,182, ...: all 18 callers) does
            # `(proposal, proposal_score) = self.get_all_proposal(...)` before `rois=proposal`.  A plain tuple
            # of two single-output symbols: nothing multi-output can reach an operator argument by accident.
            sym = mx.sym.Custom(bbox=bbox, score=score, op_type=_PREFIX + "get_top_proposal",
                                top_n=_param_str(top_n), name=name)
            return sym[0], sym[1]
        get_top_proposal._sd_alias, get_top_proposal._sd_original = True, orig
        m._sd_reference_get_top_proposal = orig
        m.get_top_proposal = get_top_proposal
        done.append("mxnext.tvm.get_top_proposal.get_top_proposal")
    except Exception:
        pass
    return done


def patch_fpn_roi_align(builder_module=None, mx=None):
    """Route the reference's FPN RoI extractor to the fused op WITHOUT editing the reference:
    rebinds `models.FPN.builder.FPNRoiAlign.get_roi_feature` (models/FPN/builder.py:567-610: fpn_roi_assign
    -> one X.roi_align per stride -> reshape -> add_n) to a method that emits ONE
    mx.sym.Custom(op_type='sd_fpn_roi_align') node over the same inputs and returns the same
    (B*R, C, out, out) symbol (fp16 graphs: cast to fp32 before, back to fp16 after, as :581-586,
    607-608).  install() calls this when `models.FPN.builder` is importable; returns True when the
    class was patched.  The original method is kept as `_sd_reference_get_roi_feature`."""
    mx = mx or _state["mx"]
    if builder_module is None:
        try:
            import importlib
            builder_module = importlib.import_module("models.FPN.builder")
        except Exception:
            return False
    cls = getattr(builder_module, "FPNRoiAlign", None)
    if cls is None or getattr(cls, "_sd_patched", False):
        return cls is not None

    def get_roi_feature(self, conv_fpn_feat, proposal):
        p = self.p
        strides = tuple(int(s) for s in p.stride)
        out = int(p.out_size)
        fp16 = bool(getattr(p, "fp16", False))
        native16 = fp16 and out in (7, 14)   # the op reads / writes fp16 itself: no cast nodes
        feats = []
        for s_ in strides:
            f = conv_fpn_feat["stride%s" % s_]
            if fp16 and not native16:
                f = mx.sym.Cast(data=f, dtype="float32", name="fpn_stride%s_to_fp32" % s_)
            feats.append(f)
        extra = {"fp16": "True"} if native16 else {}
        sym = mx.sym.Custom(*feats, proposal, op_type=_PREFIX + "fpn_roi_align",
                            rcnn_stride=_param_str(strides), pooled_size=_param_str((out, out)),
                            roi_canonical_scale=_param_str(p.roi_canonical_scale),
                            roi_canonical_level=_param_str(p.roi_canonical_level), name="fpn_roi_align",
                            **extra)
        roi_feat = mx.sym.reshape(data=sym[0], shape=(-3, -2), name="roi_feat_reshape")
        if fp16 and not native16:
            roi_feat = mx.sym.Cast(data=roi_feat, dtype="float16", name="roi_feat_to_fp16")
        return roi_feat

    cls._sd_reference_get_roi_feature = cls.get_roi_feature
    cls.get_roi_feature = get_roi_feature
    cls._sd_patched = True
    return True
