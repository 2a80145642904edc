"""Pyramid batch norm on the device: torch harness and MXNet adapter over sd_pyramid_bn_*
(csrc/pyramid_bn.hip).

SEPC's integrated batch norm, `ibn_func` (models/sepc/sepc_neck.py:112-119), takes per-channel statistics over all
pyramid levels together: reshape + Concat over the last axis, SyncBatchNorm on (N, C, 1, sum HxW), L slice_axis,
L reshape_like, and the caller's L relu (:108, :50) -- six times per forward of config/sepc/*.  Here the level list is
the operator's input: every level is read in place and written in place, the ReLU leaves in the same pass.

  torch   pyramid_bn(xs, gamma, beta, moving_mean, moving_var, ...) -> tuple of y_l with autograd to every x_l, gamma
          and beta; with an initialised process group the (2, C) blocks go through dist.all_gather_stats, as
          SyncBatchNormFunction's do.  stats / apply / infer_forward / bwd_stats / bwd_apply are the entry points as
          they are; workspace_bytes(N, C, HxW).
  MXNet   install(mx) registers ONE CustomOp, `sd_pyramid_bn` (data0..data{L-1}, gamma, beta; auxiliary moving_mean,
          moving_var; outputs output0..output{L-1}, mean, var, L of them visible; kWriteTo only).  ibn(fms, name) emits
          the node over variables `<name>_gamma`, `<name>_beta`, `<name>_moving_mean`, `<name>_moving_var`.  There is
          no reference operator name to alias and ibn_func's `bn` argument is an opaque mxnext partial, so ibn() is
          offered to configs and sepc_neck is NOT patched.

Like sync_bn and se_block it stays out of mxnet_plugin's tables and of ops.py, and shares only what _mx_adapter.py,
_lib.py and ops.py's marshalling hold.  torch and mxnet are imported inside the entry points that need them.
"""
import ctypes

from ._mx_adapter import IN_DATA, OUT_DATA, OUT_GRAD, REQ, _PREFIX, _bool, _call as _mx_call, _is_f16, _mx, _no_add, \
    _numel, _param_str, _ptr, _req, _require_write, _scratch, _state, _stream as _mx_stream, _sync, _table, _wait, \
    prop_base, register_ops

OP = "pyramid_bn"
MAX_LEVELS = 8
_own = {"installed": False, "props": {}}


def _larr(vals):
    return (ctypes.c_long * len(vals))(*[int(v) for v in vals])


# -------------------------------------------------------------------------------------------- torch ----
def workspace_bytes(N, C, HxW):
    """Bytes of the workspace of a call over levels of HxW[l] positions (one size for every entry point)."""
    from .ops import _query
    return _query("sd_pyramid_bn_workspace_bytes", int(N), int(C), _larr(HxW), len(HxW))


def _dims(xs, name="xs"):
    """checks the level list -> (N, C, HxW tuple)"""
    import torch
    from .ops import _chk
    xs = list(xs)
    if not 1 <= len(xs) <= MAX_LEVELS:
        raise ValueError("%s: 1..%d levels, got %d" % (name, MAX_LEVELS, len(xs)))
    x0 = xs[0]
    if not isinstance(x0, torch.Tensor) or x0.dtype not in (torch.float32, torch.float16):
        raise TypeError("%s must be float32 or float16 tensors" % name)
    if x0.dim() < 2:
        raise ValueError("%s[0] should be (batch, channel, ...), got %s" % (name, tuple(x0.shape)))
    N, C = int(x0.shape[0]), int(x0.shape[1])
    hxw = []
    for l, x in enumerate(xs):
        _chk(x, "%s[%d]" % (name, l), x0.dtype)
        if x.dim() < 2 or tuple(x.shape[:2]) != (N, C):
            raise ValueError("%s[%d] should be (%d, %d, ...), got %s" % (name, l, N, C, tuple(x.shape)))
        hxw.append(x.numel() // (N * C) if N * C else 0)
    return N, C, tuple(hxw)


def _like(ts, xs, name):
    """a list of tensors shaped and typed like xs (fresh ones where ts is None)"""
    import torch
    from .ops import _chk
    if ts is None:
        return [torch.empty_like(x) for x in xs]
    ts = list(ts)
    if len(ts) != len(xs):
        raise ValueError("%s: %d levels, xs has %d" % (name, len(ts), len(xs)))
    return [_chk(t, "%s[%d]" % (name, l), x.dtype, shape=tuple(x.shape)) for l, (t, x) in enumerate(zip(ts, xs))]


def _tab(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _workspace(xs, workspace, N, C, hxw):
    from .ops import _ws
    return _ws(xs[0].device, workspace, workspace_bytes(N, C, hxw))


def stats(xs, part=None, workspace=None):
    """sd_pyramid_bn_stats: levels -> part (2, C) float32, the rank's mean and biased variance about that mean."""
    from .ops import _call, _fn, _out
    N, C, hxw = _dims(xs)
    part = _out(part, "part", (2, C), xs[0].device)
    ws = _workspace(xs, workspace, N, C, hxw)
    _call(_fn("sd_pyramid_bn_stats", xs[0]), _tab(xs), part, N, C, _larr(hxw), len(hxw), ws, ws.numel())
    return part


def apply(xs, parts, gamma, beta, eps=1e-3, fix_gamma=True, relu=False, ys=None, mean=None, var=None, workspace=None):
    """sd_pyramid_bn_apply: parts (W, 2, C) in rank order -> (list of y_l, mean (C), var (C))."""
    from .ops import _call, _chk, _fn, _out, _sbn_parts
    N, C, hxw = _dims(xs)
    W = _sbn_parts(parts, "parts", C)
    _chk(gamma, "gamma", shape=(C,))
    _chk(beta, "beta", shape=(C,))
    ys = _like(ys, xs, "ys")
    dev = xs[0].device
    mean, var = _out(mean, "mean", (C,), dev), _out(var, "var", (C,), dev)
    ws = _workspace(xs, workspace, N, C, hxw)
    _call(_fn("sd_pyramid_bn_apply", xs[0]), _tab(xs), parts, W, gamma, beta, _tab(ys), mean, var, N, C, _larr(hxw),
          len(hxw), eps, bool(fix_gamma), bool(relu), ws, ws.numel())
    return ys, mean, var


def infer_forward(xs, gamma, beta, moving_mean, moving_var, eps=1e-3, fix_gamma=True, relu=False, ys=None):
    """sd_pyramid_bn_infer_fwd: the scale-shift of the moving statistics per level -> list of y_l."""
    from .ops import _call, _chk, _fn
    N, C, hxw = _dims(xs)
    for t, name in ((gamma, "gamma"), (beta, "beta"), (moving_mean, "moving_mean"), (moving_var, "moving_var")):
        _chk(t, name, shape=(C,))
    ys = _like(ys, xs, "ys")
    _call(_fn("sd_pyramid_bn_infer_fwd", xs[0]), _tab(xs), gamma, beta, moving_mean, moving_var, _tab(ys), N, C,
          _larr(hxw), len(hxw), eps, bool(fix_gamma), bool(relu))
    return ys


def bwd_stats(dys, xs, mean, var, gamma, beta, eps=1e-3, fix_gamma=True, relu=False, bpart=None, workspace=None):
    """sd_pyramid_bn_bwd_stats: -> bpart (2, C) float32 = sum dy' and sum dy' * (x - mean); with relu, dy' is 0
    wherever the forward stored y <= 0 (recomputed from x: y is no input)."""
    from .ops import _call, _chk, _fn, _out
    N, C, hxw = _dims(xs)
    dys = _like(dys, xs, "dys")
    for t, name in ((mean, "mean"), (var, "var"), (gamma, "gamma"), (beta, "beta")):
        _chk(t, name, shape=(C,))
    bpart = _out(bpart, "bpart", (2, C), xs[0].device)
    ws = _workspace(xs, workspace, N, C, hxw)
    _call(_fn("sd_pyramid_bn_bwd_stats", xs[0]), _tab(dys), _tab(xs), mean, var, gamma, beta, bpart, N, C, _larr(hxw),
          len(hxw), eps, bool(fix_gamma), bool(relu), ws, ws.numel())
    return bpart


def bwd_apply(dys, xs, mean, var, gamma, beta, bparts, rank=0, eps=1e-3, fix_gamma=True, relu=False, dxs=None,
              param_grads=True, moving_mean=None, moving_var=None, momentum=0.9, workspace=None):
    """sd_pyramid_bn_bwd_apply: bparts (W, 2, C) in rank order -> (list of dx_l, dgamma, dbeta) -- this rank's, None
    with param_grads=False.  moving_mean / moving_var, when given, are updated in place."""
    import torch
    from .ops import _call, _chk, _fn, _sbn_parts
    N, C, hxw = _dims(xs)
    dys = _like(dys, xs, "dys")
    W = _sbn_parts(bparts, "bparts", C)
    if not 0 <= int(rank) < W:
        raise ValueError("rank %d is outside 0..%d" % (rank, W - 1))
    for t, name in ((mean, "mean"), (var, "var"), (gamma, "gamma"), (beta, "beta")):
        _chk(t, name, shape=(C,))
    dxs = _like(dxs, xs, "dxs")
    dev = xs[0].device
    dgamma = dbeta = None
    if param_grads:
        dgamma, dbeta = (torch.zeros((C,), device=dev) if N * sum(hxw) == 0 else torch.empty((C,), device=dev)
                         for _ in range(2))
    if (moving_mean is None) != (moving_var is None):
        raise ValueError("moving_mean and moving_var go together")
    if moving_mean is not None:
        _chk(moving_mean, "moving_mean", shape=(C,))
        _chk(moving_var, "moving_var", shape=(C,))
    ws = _workspace(xs, workspace, N, C, hxw)
    _call(_fn("sd_pyramid_bn_bwd_apply", xs[0]), _tab(dys), _tab(xs), mean, var, gamma, beta, bparts, W, int(rank),
          _tab(dxs), dgamma, dbeta, moving_mean, moving_var, momentum, N, C, _larr(hxw), len(hxw), eps,
          bool(fix_gamma), bool(relu), ws, ws.numel())
    return dxs, dgamma, dbeta


def _gather(part):
    """the exchange of SyncBatchNormFunction: (parts (W, 2, C) in rank order, rank); one rank: no collective"""
    from . import dist
    parts, rank = dist.all_gather_stats(part)
    return parts.contiguous(), int(rank)


def _function():
    import torch

    class PyramidBNFunction(torch.autograd.Function):
        @staticmethod
        def forward(ctx, gamma, beta, conf, *xs):
            eps, fix_gamma, relu, mm, mv, momentum = conf
            xs = [x.contiguous() for x in xs]
            parts, _ = _gather(stats(xs))
            ys, mean, var = apply(xs, parts, gamma, beta, eps, fix_gamma, relu)
            ctx.save_for_backward(gamma, beta, mean, var, *xs)
            ctx.conf = conf
            return tuple(ys)

        @staticmethod
        def backward(ctx, *dys):
            gamma, beta, mean, var = ctx.saved_tensors[:4]
            xs = list(ctx.saved_tensors[4:])
            eps, fix_gamma, relu, mm, mv, momentum = ctx.conf
            dys = [torch.zeros_like(x) if dy is None else dy.contiguous() for dy, x in zip(dys, xs)]
            bparts, rank = _gather(bwd_stats(dys, xs, mean, var, gamma, beta, eps, fix_gamma, relu))
            need = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
            dxs, dgamma, dbeta = bwd_apply(dys, xs, mean, var, gamma, beta, bparts, rank, eps, fix_gamma, relu,
                                           param_grads=need, moving_mean=mm, moving_var=mv, momentum=momentum)
            return (dgamma if ctx.needs_input_grad[0] else None, dbeta if ctx.needs_input_grad[1] else None, None,
                    *dxs)

    return PyramidBNFunction


def pyramid_bn(xs, gamma, beta, moving_mean, moving_var, eps=1e-3, momentum=0.9, fix_gamma=True, relu=False,
               training=True):
    """Batch norm over the level list xs with statistics over all levels together, then ReLU where `relu`: the tuple of
    y_l.  training: autograd to every x_l, gamma and beta; the moving statistics (None: none) move in the backward, as
    SyncBatchNorm's do.  Otherwise the scale-shift of the moving statistics."""
    if not training:
        return tuple(infer_forward(list(xs), gamma, beta, moving_mean, moving_var, eps, fix_gamma, relu))
    if "fn" not in _own:
        _own["fn"] = _function()
    conf = (float(eps), bool(fix_gamma), bool(relu), moving_mean, moving_var, float(momentum))
    return _own["fn"].apply(gamma, beta, conf, *xs)


# -------------------------------------------------------------------------------------------- MXNet ----
def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class PyramidBN(CustomOp):
        def __init__(self, p, f16):
            super().__init__()
            self.p = p
            self.L = p["num_levels"]
            self.sfx = "_f16" if f16 else ""
            self.esz = 2 if f16 else 4

        def _dims(self, data):
            N, C = int(data[0].shape[0]), int(data[0].shape[1])
            return N, C, [(_numel(d.shape) // (N * C) if N * C else 0) for d in data]

        def _workspace(self, like, N, C, hxw):
            from ._lib import lib
            nbytes = int(lib().cdll.sd_pyramid_bn_workspace_bytes(N, C, _larr(hxw), len(hxw)))
            ws = _scratch(like, nbytes)
            return ws, _ptr(ws), ctypes.c_size_t(nbytes)

        def _exchange(self, part):
            """part (2, C) on the device -> (the array holding parts (W, 2, C), W, rank), as sync_bn's operator"""
            ndev = self.p["ndev"]
            if ndev == 1:
                return part, 1, 0
            import torch.distributed as tdist
            from . import dist
            from ._lib import lib
            from .sync_bn import _Holder, _as_torch
            world = tdist.get_world_size() if tdist.is_initialized() else 1
            if world != ndev:
                raise RuntimeError("pyramid_bn: ndev=%d, but the initialised process group has %d rank(s)"
                                   % (ndev, world))
            lib().call("sd_stream_synchronize", _mx_stream())
            parts, rank = dist.all_gather_stats(_as_torch(part).reshape(2, -1))
            if parts.is_cuda:
                import torch
                torch.cuda.current_stream(parts.device).synchronize()
            return _Holder(parts), ndev, rank

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            L = self.L
            data, gamma, beta = list(in_data[:L]), in_data[L], in_data[L + 1]
            mmean, mvar = aux[:2]
            _wait(*data, gamma, beta, mmean, mvar)
            N, C, hxw = self._dims(data)
            eps, fix, relu = float(self.p["eps"]), int(self.p["fix_gamma"]), int(self.p["relu"])
            if not is_train:
                _mx_call("sd_pyramid_bn_infer_fwd" + self.sfx, _table(data), _ptr(gamma), _ptr(beta), _ptr(mmean),
                         _ptr(mvar), _table(out_data[:L]), N, C, _larr(hxw), L, eps, fix, relu, None)
                _sync()
                return
            ws, wsp, wsn = self._workspace(data[0], N, C, hxw)
            part = _scratch(data[0], 4 * 2 * C)
            _mx_call("sd_pyramid_bn_stats" + self.sfx, _table(data), _ptr(part), N, C, _larr(hxw), L, wsp, wsn, None)
            parts, W, _ = self._exchange(part)
            _mx_call("sd_pyramid_bn_apply" + self.sfx, _table(data), _ptr(parts), W, _ptr(gamma), _ptr(beta),
                     _table(out_data[:L]), _ptr(out_data[L]), _ptr(out_data[L + 1]), N, C, _larr(hxw), L, eps, fix,
                     relu, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            L = self.L
            names = ["pyramid_bn data%d gradient" % l for l in range(L)] + ["pyramid_bn gamma gradient",
                                                                           "pyramid_bn beta gradient"]
            _require_write(req[:L + 2], names)
            data, gamma, beta = list(in_data[:L]), in_data[L], in_data[L + 1]
            dys, mean, var = list(out_grad[:L]), out_data[L], out_data[L + 1]
            mmean, mvar = aux[:2]
            _wait(*dys, *data, gamma, beta, mean, var, mmean, mvar)
            N, C, hxw = self._dims(data)
            eps, fix, relu = float(self.p["eps"]), int(self.p["fix_gamma"]), int(self.p["relu"])
            ws, wsp, wsn = self._workspace(data[0], N, C, hxw)
            bpart = _scratch(data[0], 4 * 2 * C)
            _mx_call("sd_pyramid_bn_bwd_stats" + self.sfx, _table(dys), _table(data), _ptr(mean), _ptr(var),
                     _ptr(gamma), _ptr(beta), _ptr(bpart), N, C, _larr(hxw), L, eps, fix, relu, wsp, wsn, None)
            bparts, W, rank = self._exchange(bpart)
            # (a frozen level: its dx goes to scratch; the moving statistics move whatever is frozen)
            dxs = [in_grad[l] if _req(req[l]) != REQ["null"] else _scratch(data[l], self.esz * _numel(data[l].shape))
                   for l in range(L)]
            want_g, want_b = [_req(r) != REQ["null"] for r in req[L:L + 2]]
            dgamma = dbeta = None
            if want_g or want_b:
                dgamma = in_grad[L] if want_g else _scratch(data[0], 4 * C)
                dbeta = in_grad[L + 1] if want_b else _scratch(data[0], 4 * C)
            _mx_call("sd_pyramid_bn_bwd_apply" + self.sfx, _table(dys), _table(data), _ptr(mean), _ptr(var),
                     _ptr(gamma), _ptr(beta), _ptr(bparts), W, rank, _table(dxs), _ptr(dgamma), _ptr(dbeta),
                     _ptr(mmean), _ptr(mvar), float(self.p["momentum"]), N, C, _larr(hxw), L, eps, fix, relu, wsp,
                     wsn, None)
            _sync()

    class PyramidBNProp(Prop):
        AUX = ("moving_mean", "moving_var")

        def __init__(self, num_levels="5", eps="1e-3", momentum="0.9", fix_gamma="True", ndev="1", act_type=""):
            super().__init__(need_top_grad=True)
            act = str(act_type)
            if act not in ("", "relu"):
                raise ValueError("pyramid_bn: act_type must be '' or 'relu', got %r" % act)
            self.p = dict(num_levels=int(num_levels), eps=float(eps), momentum=float(momentum),
                          fix_gamma=_bool(fix_gamma), ndev=int(ndev), relu=act == "relu")
            self.L = self.p["num_levels"]
            if not 1 <= self.L <= MAX_LEVELS:
                raise ValueError("pyramid_bn: num_levels must be 1..%d, got %r" % (MAX_LEVELS, num_levels))
            if self.p["ndev"] < 1:
                raise ValueError("pyramid_bn: ndev must be at least 1, got %d" % self.p["ndev"])
            self.num_visible_outputs = self.L

        def list_arguments(self):
            return ["data%d" % l for l in range(self.L)] + ["gamma", "beta"]

        def list_outputs(self):
            return ["output%d" % l for l in range(self.L)] + ["mean", "var"]

        def infer_shape(self, in_shape):
            L = self.L
            if len(in_shape) != L + 2:
                raise ValueError("pyramid_bn: %d inputs for num_levels=%d" % (len(in_shape), L))
            data = [tuple(int(s) for s in d) for d in in_shape[:L]]
            for l, d in enumerate(data):
                if len(d) < 2 or d[:2] != data[0][:2]:
                    raise ValueError("pyramid_bn: data%d should be (batch, channel, ...) = %s..., got %s"
                                     % (l, data[0][:2], d))
            c = (data[0][1],)
            return data + [c, c], data + [c, c], [c, c]

        def infer_type(self, in_type):
            # as SyncBatchNorm's: with float16 data the parameters and the statistics stay float32
            import numpy as np
            t = in_type[0]
            p = np.float32 if np.dtype(t) == np.float16 else t
            return [t] * self.L + [p, p], [t] * self.L + [p, p], [p, p]

        def create_operator(self, ctx, shapes, dtypes):
            return PyramidBN(self.p, _is_f16(dtypes))

        def declare_backward_dependency(self, out_grad, in_data, out_data):
            L = self.L     # every dy, mean and var, every level, gamma and beta (the mask is recomputed: no output_l)
            return list(out_grad[:L]) + [out_data[L], out_data[L + 1]] + list(in_data[:L + 2])

    return {OP: PyramidBNProp}


def register(mx=None):
    """Register the CustomOp.  Returns {name: PropClass}."""
    mx = _mx(mx)
    return register_ops(mx, _build_ops(mx), _own)


def install(mx=None, stream=None, sync=True):
    """register(); `stream` / `sync` are the plugin's (mxnet_plugin.install has the ordering contract).  No graph
    changes: the node enters one through ibn()."""
    mx = _mx(mx)
    props = register(mx)
    _state["stream"], _state["sync"] = stream, bool(sync)
    _own["installed"] = True
    return props


def ibn(fms, name, eps=1e-3, momentum=0.9, fix_gamma=True, ndev=1, act_type="relu", mx=None):
    """The fused node over the level symbols `fms` -> the list of its L outputs, in the place of
    `[relu(x) for x in ibn_func(fms, bn, name)]`.  Parameters are the variables `<name>_gamma`, `<name>_beta`,
    `<name>_moving_mean`, `<name>_moving_var`.  Needs install()."""
    if not _own["installed"]:
        raise RuntimeError("pyramid_bn.ibn needs pyramid_bn.install(): the operator is not registered")
    mx = _mx(mx)
    fms = list(fms)
    inputs = {"data%d" % l: s for l, s in enumerate(fms)}
    for k in ("gamma", "beta", "moving_mean", "moving_var"):
        inputs[k] = mx.sym.Variable("%s_%s" % (name, k))
    node = mx.sym.Custom(op_type=_PREFIX + OP, name=name, num_levels=_param_str(len(fms)), eps=_param_str(float(eps)),
                         momentum=_param_str(float(momentum)), fix_gamma=_param_str(bool(fix_gamma)),
                         ndev=_param_str(int(ndev)), act_type=act_type, **inputs)
    return [node[l] for l in range(len(fms))]
