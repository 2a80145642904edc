"""The FreeAnchor training head on the device: torch harness and MXNet adapter over
sd_free_anchor_loss_fwd / _bwd (csrc/free_anchor.hip).

The reference's FreeAnchorRetinaNetHead.get_loss (models/FreeAnchor/builder.py:67-148, ops.py:44-210) concatenates and
transposes every level, builds two (M, anchors) IoU matrices per image, a top-k per gt row and a (N, anchors, K) one-hot.
Here the per-level tensors go in as the head made them and the loader's anchors as they are:

  torch   free_anchor_loss(...) -> (positive_loss, negative_loss) with autograd to every level's logits and deltas;
          free_anchor_loss_forward(...) additionally returns the bags; workspace_bytes(...).
  MXNet   install(mx) registers ONE CustomOp, `sd_free_anchor_loss` (L logits, L deltas, L anchors, gt_bbox, im_info ->
          positive_loss, negative_loss; need_top_grad=False, kWriteTo only); patch_builders() rebinds
          `FreeAnchorRetinaNetHead.get_loss` to emit that node behind the reference's two MakeLoss heads, which keep
          their names (`positive_loss`, `negative_loss`: the outputs the config's metrics bind to) and no longer scale
          anything -- the node applies grad_scale itself and reads no top gradient.  The reference's method is kept as
          `_sd_reference_get_loss`; unpatch_builders() puts it back.

Like rcnn_loss it stays out of mxnet_plugin's tables and shares only what _mx_adapter.py holds.  torch and mxnet are
imported inside the entry points that need them.
"""
import ctypes
import importlib

from ._mx_adapter import REQ, _PREFIX, _call as _mx_call, _mx, _no_add, _numel, _param_str, _ptr, _req, \
    _require_write, _scratch, _state, _sync, _table, _tuple, _wait, prop_base, register_ops

OP = "free_anchor_loss"
METHOD = ("models.FreeAnchor.builder", "FreeAnchorRetinaNetHead", "get_loss")
_own = {"installed": False, "props": {}}


def _geometry(cls_shapes, delta_shapes, anchor_shapes):
    """(N, A, K, hw table, w table, anchor pitch table) of the level shapes: logits (N, A*K, H, W), deltas
    (N, A*4, H, W), anchors (1, 1, S_h, S_w, A*4) with S_h >= H and S_w >= W"""
    L = len(cls_shapes)
    if not 1 <= L <= 8 or len(delta_shapes) != L or len(anchor_shapes) != L:
        raise ValueError("free_anchor_loss: one logit, delta and anchor tensor per level, 1..8 levels")
    N, A = int(cls_shapes[0][0]), int(delta_shapes[0][1]) // 4
    K = int(cls_shapes[0][1]) // max(A, 1)
    hws, ws, pitches = [], [], []
    for l, (c, d, an) in enumerate(zip(cls_shapes, delta_shapes, anchor_shapes)):
        c, d, an = tuple(c), tuple(d), tuple(an)
        if len(c) != 4 or len(d) != 4 or c != (N, A * K) + d[2:] or d[:2] != (N, A * 4) or A < 1 or K < 1:
            raise ValueError("free_anchor_loss: level %d should be (N, A*K, H, W) and (N, A*4, H, W), got %s and %s"
                             % (l, c, d))
        if len(an) != 5 or an[:2] != (1, 1) or an[4] != A * 4 or an[2] < c[2] or an[3] < c[3]:
            raise ValueError("free_anchor_loss: anchors of level %d should be (1, 1, >=%d, >=%d, %d), got %s"
                             % (l, c[2], c[3], A * 4, an))
        hws.append(c[2] * c[3])
        ws.append(c[3])
        pitches.append(an[3])
    arr = lambda v: (ctypes.c_long * L)(*v)
    return N, A, K, arr(hws), arr(ws), arr(pitches)


def _farr(v, what):
    v = tuple(float(x) for x in v)
    if len(v) != 4:
        raise ValueError("free_anchor_loss: %s needs 4 entries" % what)
    return (ctypes.c_float * 4)(*v)


# -------------------------------------------------------------------------------------------- torch ----
def workspace_bytes(N, hws, A, K, M, top_n):
    """Bytes of the workspace of a call with these dimensions; `hws`: H_l * W_l per level."""
    from .ops import _query
    return _query("sd_free_anchor_workspace_bytes", int(N), len(hws), (ctypes.c_long * len(hws))(*hws), int(A), int(K),
                  int(M), int(top_n))


def _torch_args(cls_logits, bbox_deltas, anchors, gt_bbox, im_info, top_n, bbox_thr, alpha, gamma, mean, std):
    """the leading arguments the forward and the backward entry points share, and (N, M, hw table)"""
    from .ops import _chk, _parr
    for name, lst in (("cls_logits", cls_logits), ("bbox_deltas", bbox_deltas), ("anchors", anchors)):
        for i, t in enumerate(lst):
            _chk(t, "%s[%d]" % (name, i))
    N, A, K, hws, ws, pitches = _geometry([t.shape for t in cls_logits], [t.shape for t in bbox_deltas],
                                          [t.shape for t in anchors])
    _chk(gt_bbox, "gt_bbox", ndim=3)
    if gt_bbox.shape[0] != N or gt_bbox.shape[2] != 5:
        raise ValueError("gt_bbox should be (%d, M, 5), got %s" % (N, tuple(gt_bbox.shape)))
    _chk(im_info, "im_info", shape=(N, 3))
    M = int(gt_bbox.shape[1])
    args = (_parr(cls_logits), _parr(bbox_deltas), _parr(anchors), pitches, gt_bbox, im_info, N, len(cls_logits), hws,
            ws, A, K, M, int(top_n), float(bbox_thr), float(alpha), float(gamma), _farr(mean, "mean"), _farr(std, "std"))
    return args, (N, A, K, M, hws)


def free_anchor_loss_forward(cls_logits, bbox_deltas, anchors, gt_bbox, im_info, *, top_n, bbox_thr, alpha, gamma,
                             mean=(0.0, 0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0, 1.0), workspace=None):
    """Both FreeAnchor losses over per-level tensors, nothing concatenated: cls_logits[l] (N, A*K, H_l, W_l),
    bbox_deltas[l] (N, A*4, H_l, W_l), anchors[l] (1, 1, S_l, S_l, A*4), gt_bbox (N, M, 5), im_info (N, 3).  Returns
    (loss, bags, workspace): loss (2,) = [positive_loss, negative_loss]; bags (N, M, top_n) int32, each gt's anchors in
    rank order (-1 in the rows of gts with label <= 0); the workspace is what free_anchor_loss_backward reads."""
    import torch
    from .ops import _call, _ws
    args, (N, A, K, M, hws) = _torch_args(cls_logits, bbox_deltas, anchors, gt_bbox, im_info, top_n, bbox_thr, alpha,
                                          gamma, mean, std)
    dev = gt_bbox.device
    loss = torch.zeros(2, device=dev, dtype=torch.float32)
    bags = torch.empty((N, M, int(top_n)), device=dev, dtype=torch.int32)
    ws = _ws(dev, workspace, "sd_free_anchor_workspace_bytes", N, len(hws), hws, A, K, M, int(top_n))
    _call("sd_free_anchor_loss_fwd", *args, loss, bags, ws, ws.numel())
    return loss, bags, ws


def free_anchor_loss_backward(cls_logits, bbox_deltas, anchors, gt_bbox, im_info, workspace, *, top_n, bbox_thr, alpha,
                              gamma, mean=(0.0, 0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0, 1.0), grad_scale=1.0, d_cls=None,
                              d_delta=None):
    """grad_scale * d(positive_loss + negative_loss) for every level: (d_cls list, d_delta list), every element
    written.  `workspace` is the one the forward on the same inputs returned."""
    from .ops import _call, _grad_levels, _parr
    args, _ = _torch_args(cls_logits, bbox_deltas, anchors, gt_bbox, im_info, top_n, bbox_thr, alpha, gamma, mean, std)
    d_cls = _grad_levels(d_cls, cls_logits, "d_cls")
    d_delta = _grad_levels(d_delta, bbox_deltas, "d_delta")
    _call("sd_free_anchor_loss_bwd", *args, workspace, workspace.numel(), float(grad_scale), _parr(d_cls),
          _parr(d_delta))
    return d_cls, d_delta


def _function():
    import torch

    class FreeAnchorLossFunction(torch.autograd.Function):
        """positive, negative = apply(gt_bbox, im_info, kw, grad_scale, L, *cls_logits, *bbox_deltas, *anchors).  Both
        outputs are loss heads (MakeLoss): the backward does not look at the incoming gradients."""

        @staticmethod
        def forward(ctx, gt_bbox, im_info, kw, grad_scale, L, *levels):
            levels = [t.contiguous() for t in levels]
            gt_bbox, im_info = gt_bbox.contiguous(), im_info.contiguous()
            loss, _, ws = free_anchor_loss_forward(levels[:L], levels[L:2 * L], levels[2 * L:], gt_bbox, im_info, **kw)
            ctx.kw, ctx.gs, ctx.L = kw, grad_scale, L
            ctx.save_for_backward(gt_bbox, im_info, ws, *levels)
            return loss[0], loss[1]

        @staticmethod
        def backward(ctx, _dpos, _dneg):
            gt_bbox, im_info, ws = ctx.saved_tensors[:3]
            levels, L = list(ctx.saved_tensors[3:]), ctx.L
            d_cls, d_delta = free_anchor_loss_backward(levels[:L], levels[L:2 * L], levels[2 * L:], gt_bbox, im_info,
                                                       ws, grad_scale=ctx.gs, **ctx.kw)
            return (None,) * 5 + tuple(d_cls) + tuple(d_delta) + (None,) * L

    return FreeAnchorLossFunction


def free_anchor_loss(cls_logits, bbox_deltas, anchors, gt_bbox, im_info, *, top_n, bbox_thr, alpha, gamma,
                     mean=(0.0, 0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0, 1.0), grad_scale=1.0):
    """free_anchor_loss_forward with autograd over the lists of level tensors: (positive_loss, negative_loss), two
    scalars.  grad_scale is the head's scale_loss_shift (128 under fp16)."""
    if "fn" not in _own:
        _own["fn"] = _function()
    kw = dict(top_n=int(top_n), bbox_thr=float(bbox_thr), alpha=float(alpha), gamma=float(gamma), mean=tuple(mean),
              std=tuple(std))
    return _own["fn"].apply(gt_bbox, im_info, kw, float(grad_scale), len(cls_logits), *cls_logits, *bbox_deltas,
                            *anchors)


# -------------------------------------------------------------------------------------------- MXNet ----
def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class FreeAnchorLoss(CustomOp):
        def __init__(self, g):
            super().__init__()
            self.g = g
            self.ws = None

        def _args(self, in_data):
            g, L = self.g, self.g["num_level"]
            cls, delta, anchors = in_data[:L], in_data[L:2 * L], in_data[2 * L:3 * L]
            N, A, K, hws, ws, pitches = _geometry([t.shape for t in cls], [t.shape for t in delta],
                                                  [t.shape for t in anchors])
            gt, im_info = in_data[3 * L], in_data[3 * L + 1]
            M = int(gt.shape[1])
            args = (_table(cls), _table(delta), _table(anchors), pitches, _ptr(gt), _ptr(im_info), N, L, hws, ws, A, K,
                    M, g["top_n"], g["bbox_thr"], g["alpha"], g["gamma"], _farr(g["mean"], "mean"),
                    _farr(g["std"], "std"))
            return args, (N, A, K, M, hws)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            args, (N, A, K, M, hws) = self._args(in_data)
            from ._lib import lib
            nbytes = int(lib().cdll.sd_free_anchor_workspace_bytes(N, len(hws), hws, A, K, M, self.g["top_n"]))
            self.ws = (_scratch(in_data[0], nbytes), nbytes)
            loss = _scratch(in_data[0], 8)
            _mx_call("sd_free_anchor_loss_fwd", *args, _ptr(loss), None, _ptr(self.ws[0]), ctypes.c_size_t(nbytes),
                     None)
            _sync()
            for i in range(2):
                self.assign(out_data[i], req[i], loss[i:i + 1])

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # MakeLoss: no top gradient is read
            L = self.g["num_level"]
            _require_write(req[:2 * L], ["free_anchor_loss gradient"] * (2 * L))
            if any(_req(r) == REQ["null"] for r in req[:2 * L]):
                raise RuntimeError("free_anchor_loss writes every level's gradient (req='null' on one of them)")
            if self.ws is None:
                raise RuntimeError("free_anchor_loss: backward without a forward (the bags live in its workspace)")
            _wait(*in_data)
            args, _ = self._args(in_data)
            _mx_call("sd_free_anchor_loss_bwd", *args, _ptr(self.ws[0]), ctypes.c_size_t(self.ws[1]),
                     float(self.g["grad_scale"]), _table(in_grad[:L]), _table(in_grad[L:2 * L]), None)
            for i in range(2 * L, len(in_grad)):
                if len(req) > i:
                    self.assign(in_grad[i], req[i], 0)
            _sync()

    class FreeAnchorLossProp(Prop):
        OUTS = ("positive_loss", "negative_loss")
        OP = FreeAnchorLoss

        def __init__(self, num_level="1", top_n="50", bbox_thr="0.6", alpha="0.5", gamma="2.0", mean="(0, 0, 0, 0)",
                     std="(1, 1, 1, 1)", grad_scale="1.0"):
            super().__init__(need_top_grad=False)
            self.g = dict(num_level=int(num_level), top_n=int(top_n), bbox_thr=float(bbox_thr), alpha=float(alpha),
                          gamma=float(gamma), mean=_tuple(mean, 4), std=_tuple(std, 4), grad_scale=float(grad_scale))
            if not 1 <= self.g["num_level"] <= 8 or self.g["top_n"] < 1 or len(self.g["mean"]) != 4 or \
                    len(self.g["std"]) != 4 or 0.0 in self.g["std"]:
                raise ValueError("free_anchor_loss: num_level in 1..8, top_n >= 1, four means and four non-zero stds")

        def list_arguments(self):
            L = self.g["num_level"]
            return ["cls_logit%d" % l for l in range(L)] + ["bbox_delta%d" % l for l in range(L)] + \
                   ["anchor%d" % l for l in range(L)] + ["gt_bbox", "im_info"]

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            return list(in_data)

        def infer_shape(self, in_shape):
            L = self.g["num_level"]
            shapes = [tuple(int(s) for s in sh) for sh in in_shape]
            N = _geometry(shapes[:L], shapes[L:2 * L], shapes[2 * L:3 * L])[0]
            gt, info = shapes[3 * L], shapes[3 * L + 1] if len(shapes) > 3 * L + 1 and shapes[3 * L + 1] else (N, 3)
            if len(gt) != 3 or gt[0] != N or gt[2] != 5 or _numel(info) != N * 3:
                raise ValueError("free_anchor_loss: gt_bbox should be (%d, M, 5) and im_info (%d, 3), got %s and %s"
                                 % (N, N, gt, info))
            return shapes[:3 * L] + [gt, info], [(1,), (1,)], []

    return {OP: FreeAnchorLossProp}


def register(mx=None):
    """Register the CustomOp.  Returns {name: PropClass}."""
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


def _get_loss(mx, module):
    def get_loss(self, conv_feat, gt_bbox, im_info):
        p, X = self.p, getattr(module, "X")
        stride = p.anchor_generate.stride
        stride = stride if isinstance(stride, tuple) else (stride,)
        cls_logit_dict, bbox_delta_dict = self.get_output(conv_feat)
        shift = 128.0 if p.fp16 else 1.0
        inputs = [("cls_logit%d" % l, cls_logit_dict["stride%s" % s]) for l, s in enumerate(stride)]
        inputs += [("bbox_delta%d" % l, bbox_delta_dict["stride%s" % s]) for l, s in enumerate(stride)]
        inputs += [("anchor%d" % l, self.anchor_dict["stride%s" % s]) for l, s in enumerate(stride)]
        inputs += [("gt_bbox", gt_bbox), ("im_info", im_info)]
        params = dict(num_level=len(stride), top_n=p.anchor_assign.pre_anchor_top_n, bbox_thr=p.anchor_assign.bbox_thr,
                      alpha=p.focal_loss.alpha, gamma=p.focal_loss.gamma, mean=tuple(p.head.mean or (0, 0, 0, 0)),
                      std=tuple(p.head.std or (1, 1, 1, 1)), grad_scale=1.0 * shift)
        node = mx.sym.Custom(op_type=_PREFIX + OP, name=OP, **dict(inputs),
                             **{k: _param_str(v) for k, v in params.items()})
        # the reference's two heads under their names; the node has scaled its gradients and reads none from them
        return (X.make_loss(data=node[0], grad_scale=1.0 * shift, name="positive_loss"),
                X.make_loss(data=node[1], grad_scale=1.0 * shift, name="negative_loss"))

    return get_loss


def _builder(module):
    if module is not None:
        return module
    try:
        return importlib.import_module(METHOD[0])
    except ImportError:
        return None


def patch_builders(module=None, mx=None):
    """Rebind FreeAnchorRetinaNetHead.get_loss (the reference is not edited).  `module`: models.FreeAnchor.builder,
    imported by name when None.  Returns True when the method was rebound, False when the builder is not importable
    or lacks the class.  The original is kept as `_sd_reference_get_loss` (a second call keeps the first one).  Needs
    install()."""
    if not _own["installed"]:
        raise RuntimeError("free_anchor.patch_builders needs free_anchor.install(): the operator is not registered")
    mod = _builder(module)
    cls = getattr(mod, METHOD[1], None) if mod is not None else None
    if cls is None:
        return False
    original = cls.__dict__.get("_sd_reference_" + METHOD[2]) or cls.__dict__[METHOD[2]]
    setattr(cls, "_sd_reference_" + METHOD[2], original)
    setattr(cls, METHOD[2], _get_loss(_mx(mx), mod))
    return True


def unpatch_builders(module=None):
    """Put the reference's method back (and forget it: the class is as it was).  Returns True when it was restored."""
    mod = _builder(module)
    cls = getattr(mod, METHOD[1], None) if mod is not None else None
    original = cls.__dict__.get("_sd_reference_" + METHOD[2]) if cls is not None else None
    if original is None:
        return False
    setattr(cls, METHOD[2], original)
    delattr(cls, "_sd_reference_" + METHOD[2])
    return True
