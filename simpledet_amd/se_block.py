"""The squeeze-and-excitation block on the device: torch harness and MXNet adapter over
sd_se_block_fwd / _bwd (csrc/se_block.hip).

The reference's se() (models/efficientnet/builder.py:17-27, imported by models/se/builder.py:6) is seven graph nodes
per call -- mean, mean, 1x1 conv, relu6, 1x1 conv, sigmoid, broadcast_mul -- behind every bottleneck of
SEv2ResNetV1bFPN, every MBConv of EfficientNet-B4..B7 and four times in MaskRcnnSe4convHead.

  torch   se_block(x, w1, b1, w2, b2) -> y with autograd to all five inputs; se_block_forward / se_block_backward are
          the two entry points as they are; workspace_bytes(...).  Weights are the 1x1 convolutions' (Cr, C[, 1, 1])
          and (C, Cr[, 1, 1]) in the dtype of x; biases may be None.
  MXNet   install(mx) registers ONE CustomOp, `sd_se_block` (data, fc1_weight, fc2_weight[, fc1_bias, fc2_bias] ->
          output; gap, z1 and a are hidden outputs the backward reads; kWriteTo only).  patch_builders() rebinds `se`
          in models.efficientnet.builder AND models.se.builder (which holds its own name through `from ... import
          se`) to emit that node over variables named as the reference's graph names them, `<prefix>_fc1_weight` and
          `<prefix>_fc2_weight`, of conv shape, so checkpoints load.  The reference's functions are kept as
          `_sd_reference_se`; unpatch_builders() puts them back.  A site past the kernels' limits (C > 4096,
          Cr > 512) composes the reference's own nodes and is recorded in `fallbacks`.

Like sync_bn and free_anchor it stays out of mxnet_plugin's tables and shares only what _mx_adapter.py and _lib.py
hold.  torch and mxnet are imported inside the entry points that need them.
"""
import ctypes
import importlib

from ._mx_adapter import IN_DATA, OUT_DATA, OUT_GRAD, REQ, _PREFIX, _bool, _call as _mx_call, _is_f16, _mx, _no_add, \
    _numel, _param_str, _ptr, _req, _require_write, _scratch, _state, _sync, _wait, _ws, prop_base, register_ops

OP = "se_block"
BUILDERS = ("models.efficientnet.builder", "models.se.builder")
MAX_C, MAX_CR = 4096, 512
_own = {"installed": False, "props": {}}
fallbacks = []      # (prefix, why) of every se() site the rebound function handed back to the reference's nodes


# -------------------------------------------------------------------------------------------- torch ----
def workspace_bytes(N, C, Cr, HxW, path=0, split=0):
    """Bytes of the workspace of a call with these dimensions (one size for both directions)."""
    from .ops import _query
    return _query("sd_se_block_workspace_bytes", int(N), int(C), int(Cr), ctypes.c_long(int(HxW)), int(path), int(split))


def _dims(x, w1, b1, w2, b2):
    """checks the five inputs -> (N, C, Cr, HxW)"""
    import torch
    from .ops import _chk
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float32, torch.float16):
        raise TypeError("x must be a float32 or float16 tensor")
    _chk(x, "x", x.dtype)
    if x.dim() < 2:
        raise ValueError("x should be (batch, channel, ...), got %s" % (tuple(x.shape),))
    N, C = int(x.shape[0]), int(x.shape[1])
    HxW = x.numel() // (N * C) if N * C else 0
    Cr = int(w1.shape[0]) if isinstance(w1, torch.Tensor) and w1.dim() else 0
    _chk(w1, "w1", x.dtype, numel=Cr * C)
    _chk(w2, "w2", x.dtype, numel=C * Cr)
    if w1.shape[1] != C or tuple(w2.shape[:2]) != (C, Cr):
        raise ValueError("w1 should be (Cr, %d[, 1, 1]) and w2 (%d, Cr[, 1, 1]), got %s and %s"
                         % (C, C, tuple(w1.shape), tuple(w2.shape)))
    if b1 is not None:
        _chk(b1, "b1", x.dtype, shape=(Cr,))
    if b2 is not None:
        _chk(b2, "b2", x.dtype, shape=(C,))
    return N, C, Cr, HxW


def se_block_forward(x, w1, b1, w2, b2, path=0, split=0, workspace=None, y=None):
    """sd_se_block_fwd: -> (y, gap (N,C), z1 (N,Cr), a (N,C)); the three small float32 tensors are what the backward
    reads.  path: 0 automatic, 1 two-pass, 2 resident; split: workgroups per plane of the two-pass sums."""
    import torch
    from .ops import _call, _fn, _out, _ws as _tws
    N, C, Cr, HxW = _dims(x, w1, b1, w2, b2)
    dev = x.device
    y = _out(y, "y", tuple(x.shape), dev, x.dtype)
    gap, a = (torch.empty((N, C), device=dev, dtype=torch.float32) for _ in range(2))
    z1 = torch.empty((N, Cr), device=dev, dtype=torch.float32)
    ws = _tws(dev, workspace, workspace_bytes(N, C, Cr, HxW, path, split))
    _call(_fn("sd_se_block_fwd", x), x, w1, b1, w2, b2, y, gap, z1, a, N, C, Cr, HxW, int(path), int(split), ws,
          ws.numel())
    return y, gap, z1, a


def se_block_backward(dy, x, gap, z1, a, w1, w2, path=0, split=0, workspace=None, bias_grads=(True, True), dx=None):
    """sd_se_block_bwd: -> (dx, g (N,C), dw1, db1, dw2, db2).  The weight gradients are float32 in the weights'
    shapes; db1 / db2 are None where bias_grads says so."""
    import torch
    from .ops import _call, _chk, _fn, _out, _ws as _tws
    N, C, Cr, HxW = _dims(x, w1, None, w2, None)
    dev = x.device
    _chk(dy, "dy", x.dtype, shape=tuple(x.shape))
    _chk(gap, "gap", shape=(N, C))
    _chk(z1, "z1", shape=(N, Cr))
    _chk(a, "a", shape=(N, C))
    dx = _out(dx, "dx", tuple(x.shape), dev, x.dtype)
    f32 = dict(device=dev, dtype=torch.float32)
    g = torch.empty((N, C), **f32)
    dw1, dw2 = torch.empty(tuple(w1.shape), **f32), torch.empty(tuple(w2.shape), **f32)
    db1 = torch.empty((Cr,), **f32) if bias_grads[0] else None
    db2 = torch.empty((C,), **f32) if bias_grads[1] else None
    ws = _tws(dev, workspace, workspace_bytes(N, C, Cr, HxW, path, split))
    _call(_fn("sd_se_block_bwd", x), dy, x, gap, z1, a, w1, w2, dx, g, dw1, db1, dw2, db2, N, C, Cr, HxW, int(path),
          int(split), ws, ws.numel())
    return dx, g, dw1, db1, dw2, db2


def _function():
    import torch

    class SEBlockFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w1, b1, w2, b2):
            x, w1, w2 = x.contiguous(), w1.contiguous(), w2.contiguous()
            y, gap, z1, a = se_block_forward(x, w1, b1, w2, b2)
            ctx.bias = (b1 is not None, b2 is not None)
            ctx.save_for_backward(x, w1, w2, gap, z1, a)
            return y

        @staticmethod
        def backward(ctx, dy):
            x, w1, w2, gap, z1, a = ctx.saved_tensors
            dx, _, dw1, db1, dw2, db2 = se_block_backward(dy.contiguous(), x, gap, z1, a, w1, w2, bias_grads=ctx.bias)
            cast = lambda t: None if t is None else t.to(x.dtype)
            return dx, cast(dw1), cast(db1), cast(dw2), cast(db2)

    return SEBlockFunction


def se_block(x, w1, b1, w2, b2):
    """y = x * sigmoid(w2 relu6(w1 mean(x) + b1) + b2) with autograd to all five inputs (b1 / b2 may be None)."""
    if "fn" not in _own:
        _own["fn"] = _function()
    return _own["fn"].apply(x, w1, b1, w2, b2)


# -------------------------------------------------------------------------------------------- MXNet ----
def _store_f32(op, dst, req, src, n):
    """the first n floats of the float32 scratch `src` into the gradient array `dst` (its own dtype and shape)"""
    if hasattr(src, "t") and hasattr(dst, "t"):     # the test stand-in wraps torch tensors
        op.assign(dst, req, src.t[:n].view(dst.t.shape).to(dst.t.dtype))
    else:
        op.assign(dst, req, src[:n].reshape(dst.shape).astype(dst.dtype))


def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class SEBlock(CustomOp):
        def __init__(self, no_bias, f16):
            super().__init__()
            self.no_bias = no_bias
            self.sfx = "_f16" if f16 else ""
            self.f16 = f16

        @staticmethod
        def _dims(data, w1):
            N, C, Cr = int(data.shape[0]), int(data.shape[1]), int(w1.shape[0])
            return N, C, Cr, (_numel(data.shape) // (N * C) if N * C else 0)

        @staticmethod
        def _workspace(like, d):
            return _ws(like, "sd_se_block_workspace_bytes", d[0], d[1], d[2], ctypes.c_long(d[3]), 0, 0)

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            _wait(*in_data)
            data, w1, w2 = in_data[:3]
            b1, b2 = (None, None) if self.no_bias else in_data[3:5]
            d = self._dims(data, w1)
            ws, wsp, wsn = self._workspace(data, d)
            _mx_call("sd_se_block_fwd" + self.sfx, _ptr(data), _ptr(w1), _ptr(b1), _ptr(w2), _ptr(b2),
                     _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), _ptr(out_data[3]), d[0], d[1], d[2],
                     ctypes.c_long(d[3]), 0, 0, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            names = ["se_block data gradient", "se_block fc1_weight gradient", "se_block fc2_weight gradient",
                     "se_block fc1_bias gradient", "se_block fc2_bias gradient"]
            _require_write(req, names)
            data, w1, w2 = in_data[:3]
            _wait(out_grad[0], *in_data, *out_data[1:4])
            N, C, Cr, HxW = d = self._dims(data, w1)
            want = [_req(r) != REQ["null"] for r in req] + [False] * 5
            esz = 2 if self.f16 else 4
            dx = in_grad[0] if want[0] else _scratch(data, esz * _numel(data.shape))
            g = _scratch(data, 4 * N * C)
            direct = not self.f16       # float32 gradients are the kernel's own outputs
            dw1 = in_grad[1] if direct and want[1] else _scratch(data, 4 * C * Cr)
            dw2 = in_grad[2] if direct and want[2] else _scratch(data, 4 * C * Cr)
            db1 = db2 = None
            if not self.no_bias:
                db1 = in_grad[3] if direct and want[3] else _scratch(data, 4 * Cr)
                db2 = in_grad[4] if direct and want[4] else _scratch(data, 4 * C)
            ws, wsp, wsn = self._workspace(data, d)
            _mx_call("sd_se_block_bwd" + self.sfx, _ptr(out_grad[0]), _ptr(data), _ptr(out_data[1]), _ptr(out_data[2]),
                     _ptr(out_data[3]), _ptr(w1), _ptr(w2), _ptr(dx), _ptr(g), _ptr(dw1), _ptr(db1), _ptr(dw2),
                     _ptr(db2), N, C, Cr, ctypes.c_long(HxW), 0, 0, wsp, wsn, None)
            _sync()
            if not direct:
                for i, (src, n) in enumerate(((dw1, C * Cr), (dw2, C * Cr), (db1, Cr), (db2, C)), start=1):
                    if src is not None and want[i]:
                        _store_f32(self, in_grad[i], req[i], src, n)

    class SEBlockProp(Prop):
        OUTS = ("output", "gap", "z1", "a")
        # dy, the three small outputs, data and both weights
        DEPS = ((OUT_GRAD, 0), (OUT_DATA, 1), (OUT_DATA, 2), (OUT_DATA, 3), (IN_DATA, 0), (IN_DATA, 1), (IN_DATA, 2))

        def __init__(self, num_hidden="0", no_bias="True"):
            super().__init__(need_top_grad=True)
            self.num_hidden, self.no_bias = int(num_hidden), _bool(no_bias)
            if not 1 <= self.num_hidden <= MAX_CR:
                raise ValueError("se_block: num_hidden (the squeezed width) must be in 1..%d, got %d"
                                 % (MAX_CR, self.num_hidden))
            self.num_visible_outputs = 1

        def list_arguments(self):
            return ["data", "fc1_weight", "fc2_weight"] + ([] if self.no_bias else ["fc1_bias", "fc2_bias"])

        def infer_shape(self, in_shape):
            d = tuple(int(s) for s in in_shape[0])
            if len(d) < 2 or not 1 <= d[1] <= MAX_C:
                raise ValueError("se_block: data should be (batch, channel <= %d, ...), got %s" % (MAX_C, d))
            N, C, Cr = d[0], d[1], self.num_hidden
            ins = [d, (Cr, C, 1, 1), (C, Cr, 1, 1)] + ([] if self.no_bias else [(Cr,), (C,)])
            return ins, [d, (N, C), (N, Cr), (N, C)], []

        def infer_type(self, in_type):
            import numpy as np
            t = in_type[0]
            return [t] * len(self.list_arguments()), [t, np.float32, np.float32, np.float32], []

        def create_operator(self, ctx, shapes, dtypes):
            return SEBlock(self.no_bias, _is_f16(dtypes))

    return {OP: SEBlockProp}


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
    del fallbacks[:]
    _own["installed"] = True
    return props


def _se(mx, original, no_bias):
    def se(input, prefix, f_down, f_up):
        if not (1 <= int(f_down) <= MAX_CR and 1 <= int(f_up) <= MAX_C):
            fallbacks.append((prefix, "f_down=%s / f_up=%s exceed the kernels' limits %d / %d"
                              % (f_down, f_up, MAX_CR, MAX_C)))
            return original(input, prefix, f_down, f_up)
        Cr, C = int(f_down), int(f_up)
        inputs = dict(data=input,
                      fc1_weight=mx.sym.var(prefix + "_fc1_weight", shape=(Cr, C, 1, 1)),
                      fc2_weight=mx.sym.var(prefix + "_fc2_weight", shape=(C, Cr, 1, 1)))
        if not no_bias:
            inputs.update(fc1_bias=mx.sym.var(prefix + "_fc1_bias", shape=(Cr,)),
                          fc2_bias=mx.sym.var(prefix + "_fc2_bias", shape=(C,)))
        node = mx.sym.Custom(op_type=_PREFIX + OP, name=prefix + "_mul", num_hidden=_param_str(Cr),
                             no_bias=_param_str(bool(no_bias)), **inputs)
        return node[0]
    se._sd_alias = True
    return se


def _modules(modules):
    if modules is not None:
        return list(modules)
    out = []
    for name in BUILDERS:
        try:
            out.append(importlib.import_module(name))
        except ImportError:
            pass
    return out


def patch_builders(modules=None, mx=None, no_bias=True):
    """Rebind `se` in models.efficientnet.builder and models.se.builder (the reference is not edited; `modules`: the
    two modules, imported by name when None).  no_bias: the reference calls mxnext's conv() without `no_bias`, whose
    default is believed to be True: pass False where the checkpoints hold fc biases.  Returns the
    number of modules rebound.  Each keeps its original as `_sd_reference_se` (a second call keeps the first one).
    Needs install()."""
    if not _own["installed"]:
        raise RuntimeError("se_block.patch_builders needs se_block.install(): the operator is not registered")
    mx = _mx(mx)
    done = 0
    for mod in _modules(modules):
        cur = getattr(mod, "se", None)
        if cur is None:
            continue
        original = getattr(mod, "_sd_reference_se", None) or cur
        mod._sd_reference_se = original
        mod.se = _se(mx, original, no_bias)
        done += 1
    return done


def unpatch_builders(modules=None):
    """Put the reference's `se` back in both modules.  Returns the number restored."""
    done = 0
    for mod in _modules(modules):
        original = getattr(mod, "_sd_reference_se", None)
        if original is not None:
            mod.se = original
            del mod._sd_reference_se
            done += 1
    return done
