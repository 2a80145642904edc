"""The Faster / Mask R-CNN loss heads behind the reference's node names.

The reference's RPN and R-CNN heads end in `SoftmaxOutput` and `smooth_l1 -> * weight -> MakeLoss`
(symbol/builder.py:163-206, 405-446; models/FPN/builder.py:156-237), the FPN form behind five reshapes and two
concats per tensor.  This module

  1. registers four single-output CustomOps, `sd_rpn_cls_loss`, `sd_rpn_reg_loss`, `sd_bbox_cls_loss` and
     `sd_bbox_reg_loss` (need_top_grad=False: each is a loss head, as SoftmaxOutput and MakeLoss are);
  2. `patch_builders()` rebinds `RpnHead.get_loss`, `FPNRpnHead.get_loss` and `BboxHead.get_loss` to methods that
     read the same fields of `self.p` and emit ONE `mx.sym.Custom` node per reference loss node, carrying the
     reference's node name -- `rpn_cls_loss`, `rpn_reg_loss`, `bbox_cls_loss`, `bbox_reg_loss` -- so that the output
     names the configs' metrics bind to (`rpn_cls_loss_output`, ...) survive.  The FPN head hands its per-level
     tensors to the node as they are, no reshape and no concat in front.  The label outputs
     (`rpn_cls_label_blockgrad`, `bbox_label_blockgrad`) stay the reference's own nodes.  The reference's methods
     are kept on their classes as `_sd_reference_get_loss`; `unpatch_builders()` puts them back.

Left to the reference: heads that override get_loss themselves (Cascade R-CNN, TridentNet, the OHEM and
mask-rcnn variants in symbol/component.py) and the FPN head with `nnvm_rpn_target` (its labels come from a
compiled graph).  Like merged_bn it stays out of mxnet_plugin's tables: it is no flag of `mxnet_plugin.install()`,
and shares only what _mx_adapter.py holds (pointer path, stream / sync state) and the plugin's fallback record.
`import mxnet` happens inside the entry points.
"""
import ctypes
import importlib

from ._mx_adapter import REQ, _PREFIX, _bool, _call, _mx, _no_add, _numel, _param_str, _ptr, _req, _require_write, \
    _scratch, _state, _sync, _table, _wait, _ws, prop_base, register_ops
from .mxnet_plugin import _fell_back

OPS = ("rpn_cls_loss", "rpn_reg_loss", "bbox_cls_loss", "bbox_reg_loss")
# (module, class, method) of the builders patch_builders() rebinds
METHODS = (("symbol.builder", "RpnHead", "get_loss"), ("models.FPN.builder", "FPNRpnHead", "get_loss"),
           ("symbol.builder", "BboxHead", "get_loss"))
_own = {"installed": False, "props": {}}


def _softmax_opts(what, normalization, want, smooth_alpha, out_grad):
    if normalization != want:
        raise ValueError("%s: normalization=%r is not built (the head uses %r)" % (what, normalization, want))
    if float(smooth_alpha) != 0.0 or _bool(out_grad):
        raise ValueError("%s: smooth_alpha and out_grad are not built" % what)


# ---------------------------------------------------------------------------------- operators ----
def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class _Loss(CustomOp):
        """one half of a head: n_grad leading inputs get gradients, the rest (labels, targets, weights) zeros"""
        n_grad = 1

        def __init__(self, g):
            super().__init__()
            self.g = g
            self.state = None

        def _finish(self, req, in_grad):
            for i in range(self.n_grad, len(in_grad)):
                if len(req) > i:
                    self.assign(in_grad[i], req[i], 0)
            _sync()

        def _grad_req(self, req, what):
            _require_write(req[:self.n_grad], [what + " gradient"] * self.n_grad)
            if any(_req(r) == REQ["null"] for r in req[:self.n_grad]):
                raise RuntimeError("%s writes every level's gradient (req='null' on one of them)" % what)
            if self.state is None:
                raise RuntimeError("%s: backward without a forward (the normaliser comes from its state block)" % what)

    class RpnLoss(_Loss):
        def __init__(self, g, box):
            super().__init__(g)
            self.box, self.n_grad = box, g["num_level"]

        def _dims(self, in_data):
            L, per = self.g["num_level"], 4 if self.box else 2
            levels = in_data[:L]
            N, A = int(levels[0].shape[0]), int(levels[0].shape[1]) // per
            hws = [_numel(t.shape[2:]) for t in levels]
            return levels, N, A, (ctypes.c_long * L)(*hws), sum(hws)

        def _inputs(self, in_data):
            L = self.g["num_level"]
            levels = in_data[:L]
            tab = _table(levels)
            if self.box:
                return [None, tab], [None, _ptr(in_data[L]), _ptr(in_data[L + 1])]
            return [tab, None], [_ptr(in_data[L]), None, None]

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            levels, N, A, hws, HW = self._dims(in_data)
            self.state = _scratch(levels[0], 16)
            ws, wsp, wsn = _ws(levels[0], "sd_rpn_loss_workspace_bytes", N, A, ctypes.c_long(HW))
            tabs, fixed = self._inputs(in_data)
            out = _ptr(out_data[0]) if _req(req[0]) != REQ["null"] else None
            _call("sd_rpn_loss_fwd", tabs[0], tabs[1], hws, len(levels), *fixed, N, A, float(self.g["ignore_label"]),
                  float(self.g["sigma"]), None if self.box else out, out if self.box else None, _ptr(self.state),
                  wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # SoftmaxOutput / MakeLoss: the head gradient is not read
            self._grad_req(req, "rpn_reg_loss" if self.box else "rpn_cls_loss")
            _wait(*in_data)
            levels, N, A, hws, HW = self._dims(in_data)
            tabs, fixed = self._inputs(in_data)
            grads = _table(in_grad[:len(levels)])
            gs = float(self.g["grad_scale"])
            _call("sd_rpn_loss_bwd", tabs[0], tabs[1], hws, len(levels), *fixed, N, A, float(self.g["ignore_label"]),
                  float(self.g["sigma"]), gs, gs, _ptr(self.state), None if self.box else grads,
                  grads if self.box else None, None)
            self._finish(req, in_grad)

    class RcnnLoss(_Loss):
        def __init__(self, g, box):
            super().__init__(g)
            self.box = box

        def _args(self, in_data):
            R, C = int(in_data[0].shape[0]), _numel(in_data[0].shape[1:])
            if self.box:
                return [None, None] + [_ptr(t) for t in in_data[:3]], R, 1, C
            return [_ptr(in_data[0]), _ptr(in_data[1]), None, None, None], R, C, 0

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            ptrs, R, K, D = self._args(in_data)
            self.state = _scratch(in_data[0], 16)
            ws, wsp, wsn = _ws(in_data[0], "sd_rcnn_loss_workspace_bytes", R)
            out = _ptr(out_data[0]) if _req(req[0]) != REQ["null"] else None
            _call("sd_rcnn_loss_fwd", *ptrs, R, K, D, float(self.g["sigma"]), None if self.box else out,
                  out if self.box else None, _ptr(self.state), wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            self._grad_req(req, "bbox_reg_loss" if self.box else "bbox_cls_loss")
            _wait(*in_data)
            ptrs, R, K, D = self._args(in_data)
            gs = float(self.g["grad_scale"])
            g = _ptr(in_grad[0])
            _call("sd_rcnn_loss_bwd", *ptrs, R, K, D, float(self.g["sigma"]), gs, gs, _ptr(self.state),
                  None if self.box else g, g if self.box else None, None)
            self._finish(req, in_grad)

    class _Prop(Prop):
        what = ""

        def __init__(self):
            super().__init__(need_top_grad=False)

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return list(in_data)

        def _same(self, i, given, want):
            if given and 0 not in tuple(given) and _numel(given) != _numel(want):
                raise ValueError("%s: %s is %s, expected %s" % (self.what, self.list_arguments()[i], tuple(given), want))
            return tuple(int(s) for s in given) if given and 0 not in tuple(given) else want

    class _RpnProp(_Prop):
        per, first = 2, "cls_logit"

        def _levels(self, in_shape):
            L = self.g["num_level"]
            levels = [tuple(int(s) for s in in_shape[l]) for l in range(L)]
            for l, s in enumerate(levels):
                if len(s) < 3 or s[0] != levels[0][0] or s[1] != levels[0][1] or s[1] % self.per:
                    raise ValueError("%s: %s%d should be (N, %dA, H, W), got %s" % (self.what, self.first, l, self.per, s))
            N, A = levels[0][0], levels[0][1] // self.per
            return levels, N, A, sum(_numel(s[2:]) for s in levels)

    class RpnClsLossProp(_RpnProp):
        what = "rpn_cls_loss"

        def __init__(self, num_level="1", grad_scale="1.0", ignore_label="-1", normalization="valid", use_ignore="True",
                     multi_output="True", smooth_alpha="0", out_grad="False"):
            super().__init__()
            _softmax_opts(self.what, normalization, "valid", smooth_alpha, out_grad)
            if not (_bool(use_ignore) and _bool(multi_output)):
                raise ValueError("rpn_cls_loss: only use_ignore=True, multi_output=True is built")
            self.g = dict(num_level=int(num_level), grad_scale=float(grad_scale), ignore_label=float(ignore_label),
                          sigma=3.0)
            if not 1 <= self.g["num_level"] <= 8 or self.g["ignore_label"] != int(self.g["ignore_label"]):
                raise ValueError("rpn_cls_loss: num_level in 1..8 and an integer ignore_label")

        def list_arguments(self):
            return ["cls_logit%d" % l for l in range(self.g["num_level"])] + ["cls_label"]

        def infer_shape(self, in_shape):
            levels, N, A, HW = self._levels(in_shape)
            L = len(levels)
            label = self._same(L, in_shape[L] if len(in_shape) > L else (), (N, A * HW))
            # SoftmaxOutput's output has its data's shape: (N, 2, A, H, W) for the C4 head, (N, 2, A, sum HW) for FPN
            out = (N, 2, A) + levels[0][2:] if L == 1 else (N, 2, A, HW)
            return levels + [label], [out], []

        def create_operator(self, ctx, shapes, dtypes):
            return RpnLoss(self.g, box=False)

    class RpnRegLossProp(_RpnProp):
        what, per, first = "rpn_reg_loss", 4, "bbox_delta"

        def __init__(self, num_level="1", grad_scale="1.0", scalar="3.0"):
            super().__init__()
            self.g = dict(num_level=int(num_level), grad_scale=float(grad_scale), sigma=float(scalar), ignore_label=-1.0)
            if not 1 <= self.g["num_level"] <= 8 or not self.g["sigma"] > 0:
                raise ValueError("rpn_reg_loss: num_level in 1..8 and a positive scalar")

        def list_arguments(self):
            return ["bbox_delta%d" % l for l in range(self.g["num_level"])] + ["reg_target", "reg_weight"]

        def infer_shape(self, in_shape):
            levels, N, A, HW = self._levels(in_shape)
            L = len(levels)
            out = levels[0] if L == 1 else (N, 4 * A, HW)
            rest = [self._same(L + i, in_shape[L + i] if len(in_shape) > L + i else (), out) for i in range(2)]
            return levels + rest, [out], []

        def create_operator(self, ctx, shapes, dtypes):
            return RpnLoss(self.g, box=True)

    class BboxClsLossProp(_Prop):
        what, ARGS = "bbox_cls_loss", ("cls_logit", "cls_label")

        def __init__(self, grad_scale="1.0", normalization="batch", smooth_alpha="0", out_grad="False"):
            super().__init__()
            _softmax_opts(self.what, normalization, "batch", smooth_alpha, out_grad)
            self.g = dict(grad_scale=float(grad_scale), sigma=1.0)

        def infer_shape(self, in_shape):
            x = tuple(int(s) for s in in_shape[0])
            if len(x) != 2:
                raise ValueError("bbox_cls_loss: cls_logit should be (R, K), got %s" % (x,))
            return [x, self._same(1, in_shape[1] if len(in_shape) > 1 else (), (x[0],))], [x], []

        def create_operator(self, ctx, shapes, dtypes):
            return RcnnLoss(self.g, box=False)

    class BboxRegLossProp(_Prop):
        what, ARGS = "bbox_reg_loss", ("bbox_delta", "bbox_target", "bbox_weight")

        def __init__(self, grad_scale="1.0", scalar="1.0"):
            super().__init__()
            self.g = dict(grad_scale=float(grad_scale), sigma=float(scalar))
            if not self.g["sigma"] > 0:
                raise ValueError("bbox_reg_loss: scalar must be positive")

        def infer_shape(self, in_shape):
            d = tuple(int(s) for s in in_shape[0])
            if len(d) != 2:
                raise ValueError("bbox_reg_loss: bbox_delta should be (R, D), got %s" % (d,))
            return [d] + [self._same(i, in_shape[i] if len(in_shape) > i else (), d) for i in (1, 2)], [d], []

        def create_operator(self, ctx, shapes, dtypes):
            return RcnnLoss(self.g, box=True)

    return dict(rpn_cls_loss=RpnClsLossProp, rpn_reg_loss=RpnRegLossProp, bbox_cls_loss=BboxClsLossProp,
                bbox_reg_loss=BboxRegLossProp)


# ------------------------------------------------------------------------------- registration ----
def register(mx=None):
    """Register the four CustomOps.  Returns {name: PropClass}."""
    mx = _mx(mx)
    return register_ops(mx, _build_ops(mx), _own)


def install(mx=None, stream=None, sync=True):
    """register(); `stream` / `sync` are the plugin's (mxnet_plugin.install has the ordering contract).  The graph
    changes only with patch_builders()."""
    mx = _mx(mx)
    props = register(mx)
    _state["stream"], _state["sync"] = stream, bool(sync)
    _own["installed"] = True
    return props


# ----------------------------------------------------------------------------------- builders ----
def _methods(mx, modules, originals):
    def X_of(self_or_mod):
        return getattr(self_or_mod, "X")

    def custom(op, inputs, **params):
        """one node named after the reference's; `inputs`: (argument name, symbol) in the order of list_arguments"""
        kw = dict(inputs)
        kw.update({k: _param_str(v) for k, v in params.items()})
        return mx.sym.Custom(op_type=_PREFIX + op, name=op, **kw)

    def rpn_losses(p, cls_logits, bbox_deltas, cls_label, bbox_target, bbox_weight, image_anchor):
        shift = 128.0 if p.fp16 else 1.0
        L = len(cls_logits)
        cls_loss = custom("rpn_cls_loss",
                          [("cls_logit%d" % l, s) for l, s in enumerate(cls_logits)] + [("cls_label", cls_label)],
                          num_level=L, grad_scale=1.0 * shift, ignore_label=-1, normalization="valid", use_ignore=True,
                          multi_output=True)
        reg_loss = custom("rpn_reg_loss",
                          [("bbox_delta%d" % l, s) for l, s in enumerate(bbox_deltas)]
                          + [("reg_target", bbox_target), ("reg_weight", bbox_weight)],
                          num_level=L, scalar=3.0, grad_scale=1.0 / (p.batch_image * image_anchor) * shift)
        return cls_loss, reg_loss

    def rpn_get_loss(self, conv_feat, gt_bboxes, im_infos):
        p = self.p
        X = X_of(modules[0])
        cls_logit, bbox_delta = self.get_output(conv_feat)
        return rpn_losses(p, [cls_logit], [bbox_delta], X.var("rpn_cls_label"), X.var("rpn_reg_target"),
                          X.var("rpn_reg_weight"), p.anchor_generate.image_anchor)

    def fpn_rpn_get_loss(self, conv_fpn_feat, gt_bbox, im_info):
        p = self.p
        if p.nnvm_rpn_target:
            # the labels come out of a compiled graph that wants the reference's reshaped tensors: left as it is
            _fell_back("rpn_cls_loss", "nnvm_rpn_target builds its own label graph")
            return originals[1](self, conv_fpn_feat, gt_bbox, im_info)
        X = X_of(modules[1])
        cls_logit_dict, bbox_delta_dict = self.get_output(conv_fpn_feat)
        strides = p.anchor_generate.stride
        cls_label = X.var("rpn_cls_label")
        cls_loss, reg_loss = rpn_losses(p, [cls_logit_dict[s] for s in strides], [bbox_delta_dict[s] for s in strides],
                                        cls_label, X.var("rpn_reg_target"), X.var("rpn_reg_weight"),
                                        p.anchor_assign.image_anchor)
        return cls_loss, reg_loss, X.stop_grad(cls_label, "rpn_cls_label_blockgrad")

    def bbox_get_loss(self, conv_feat, cls_label, bbox_target, bbox_weight):
        p = self.p
        X = X_of(modules[2])
        batch_roi = p.image_roi * p.batch_image
        smooth_l1_scalar = p.regress_target.smooth_l1_scalar or 1.0
        cls_logit, bbox_delta = self.get_output(conv_feat)
        shift = 128.0 if p.fp16 else 1.0
        cls_loss = custom("bbox_cls_loss", [("cls_logit", cls_logit), ("cls_label", cls_label)],
                          grad_scale=1.0 * shift, normalization="batch")
        reg_loss = custom("bbox_reg_loss",
                          [("bbox_delta", bbox_delta), ("bbox_target", bbox_target), ("bbox_weight", bbox_weight)],
                          scalar=smooth_l1_scalar, grad_scale=1.0 / batch_roi * shift)
        cls_label = X.reshape(cls_label, shape=(p.batch_image, -1), name="bbox_label_reshape")
        cls_label = X.block_grad(cls_label, name="bbox_label_blockgrad")
        return cls_loss, reg_loss, cls_label

    return [rpn_get_loss, fpn_rpn_get_loss, bbox_get_loss]


def _import_builders(modules):
    if modules is not None:
        return list(modules)
    try:
        return [importlib.import_module(m) for m, _, _ in METHODS]
    except ImportError:
        return None


def patch_builders(modules=None, mx=None):
    """Rebind RpnHead.get_loss, FPNRpnHead.get_loss and BboxHead.get_loss (the reference is not edited).  `modules`:
    the three modules of METHODS in order, imported by name when None.  Returns True when the three methods were
    rebound, False when the reference's builders are not importable or lack one of the classes.  The originals are
    kept as `_sd_reference_get_loss` on their classes (a second call keeps the first ones).  Needs install()."""
    if not _own["installed"]:
        raise RuntimeError("rcnn_loss.patch_builders needs rcnn_loss.install(): the loss operators are not registered")
    mods = _import_builders(modules)
    if mods is None:
        return False
    classes = [getattr(m, c, None) for m, (_, c, _) in zip(mods, METHODS)]
    if any(c is None for c in classes):
        return False
    originals = [c.__dict__.get("_sd_reference_" + m) or c.__dict__[m] for c, (_, _, m) in zip(classes, METHODS)]
    for c, (_, _, m), original, new in zip(classes, METHODS, originals, _methods(_mx(mx), mods, originals)):
        setattr(c, "_sd_reference_" + m, original)
        setattr(c, m, new)
    return True


def unpatch_builders(modules=None):
    """Put the reference's three methods back (and forget them: the classes are as they were).  Returns True when
    something was restored."""
    mods = _import_builders(modules)
    if mods is None:
        return False
    done = False
    for mod, (_, c, m) in zip(mods, METHODS):
        cls = getattr(mod, c, None)
        original = cls.__dict__.get("_sd_reference_" + m) if cls is not None else None
        if original is not None:
            setattr(cls, m, original)
            delattr(cls, "_sd_reference_" + m)
            done = True
    return done
