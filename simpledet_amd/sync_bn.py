"""`_contrib_SyncBatchNorm` behind the reference's name: the CustomOp `sd__contrib_SyncBatchNorm` over the kernels
of simpledet_amd/csrc/sync_bn.hip, and `install()`, which aliases `mx.sym.contrib.SyncBatchNorm` to it.

Every `normalizer_factory(type="syncbn", ndev=...)` site of the reference (config/FPG/*_syncbn_1x.py,
config/NASFPN/*, config/scratch/tridentnet_*_syncbn_*, config/faster_r101v2c4_c5_256roi_syncbn_1x.py) builds this
operator behind every backbone and neck convolution.  The operator's arguments (data, gamma, beta), auxiliary
states (moving_mean, moving_var), outputs (output, mean, var; one visible unless output_mean_var), parameters and
defaults are those of sync_batch_norm-inl.h:49-76,556-662.

  * training (is_train and not use_global_stats): statistics kernel -> exchange -> element kernel, both ways.
    ndev = 1 has no exchange.  ndev > 1 exchanges one (2, C) float32 block per direction through
    `simpledet_amd.dist.all_gather_stats`, one process per GPU; `ndev` must be the initialised world size.
    `key` is accepted and ignored: the reference needs it to find its peers inside one process, here rank identity
    comes from the process group.
  * the moving statistics move in the BACKWARD, as the reference's do (:471-472).
  * inference (is_train false): the scale-shift of the moving statistics (:359-363).
  * `use_global_stats=True`, or a keyword the operator does not know, hands the call back to the native
    constructor (`sd_supports`), and `fallbacks` records it.  kAddTo is refused on every output and gradient.
  * gamma is never written: under fix_gamma the reference stores ones into it (:320), this operator reads 1.

It stays out of mxnet_plugin's tables on purpose, like merged_bn.py: it is no flag of `mxnet_plugin.install()`, and
shares only what _mx_adapter.py holds (the pointer path, the alias path, the stream / sync state -- one state for both).
"""
import ctypes

from ._lib import lib
from ._mx_adapter import IN_DATA, OUT_DATA, OUT_GRAD, REQ, _bool, _call, _is_f16, _mx, _no_add, _numel, _ptr, _req, \
    _require_write, _scratch, _state, _stream, _sync, _wait, _ws, alias_ctor, drop_alias, prop_base, put_alias, \
    register_ops

SYNC_BN = "_contrib_SyncBatchNorm"
_own = {"installed": False, "props": {}}
fallbacks = []      # (operator, node name, why) of every call install()'s alias handed to the native constructor


def _as_torch(nd):
    """the torch view of a device array, for the exchange: the test stand-in wraps a tensor; MXNet's goes by DLPack"""
    import torch
    if isinstance(getattr(nd, "t", None), torch.Tensor):
        return nd.t
    if hasattr(nd, "to_dlpack_for_write"):
        return torch.utils.dlpack.from_dlpack(nd.to_dlpack_for_write())
    raise TypeError("SyncBatchNorm: ndev > 1 needs arrays torch can view (DLPack), got %r" % type(nd))


class _Holder:
    """keeps the gathered tensor alive and gives the pointer path its data_ptr()"""

    def __init__(self, t):
        self.t = t

    def data_ptr(self):
        return self.t.data_ptr()


def _build_ops(mx):
    CustomOp, Prop = mx.operator.CustomOp, prop_base(mx)

    class SyncBatchNorm(CustomOp):
        def __init__(self, p, f16):
            super().__init__()
            self.p = p
            self.sfx = "_f16" if f16 else ""
            self.esz = 2 if f16 else 4

        @staticmethod
        def _dims(shape):
            N, C = int(shape[0]), int(shape[1])
            return N, C, (_numel(shape) // (N * C) if N * C else 0)

        @staticmethod
        def _workspace(like, dims):
            return _ws(like, "sd_sync_bn_workspace_bytes", dims[0], dims[1], ctypes.c_long(dims[2]))

        def _exchange(self, part):
            """part (2, C) on the device -> (the array holding parts (W, 2, C), W, rank)"""
            ndev = self.p["ndev"]
            if ndev == 1:
                return part, 1, 0
            import torch.distributed as tdist
            from . import dist
            world = tdist.get_world_size() if tdist.is_initialized() else 1
            if world != ndev:
                raise RuntimeError("SyncBatchNorm: ndev=%d, but the initialised process group has %d rank(s)"
                                   % (ndev, world))
            # the statistics kernel ran on the adapter's stream, the collective runs on torch's
            lib().call("sd_stream_synchronize", _stream())
            parts, rank = dist.all_gather_stats(_as_torch(part).reshape(2, -1))
            if parts.is_cuda:
                import torch
                torch.cuda.current_stream(parts.device).synchronize()
            return _Holder(parts), ndev, rank

        def forward(self, is_train, req, in_data, out_data, aux):
            _no_add(req)
            data, gamma, beta = in_data[:3]
            mmean, mvar = aux[:2]
            _wait(data, gamma, beta, mmean, mvar)
            N, C, HxW = dims = self._dims(data.shape)
            fix = int(self.p["fix_gamma"])
            if not is_train:
                # (use_global_stats never reaches this operator: sd_supports hands it to the native constructor)
                _call("sd_sync_bn_infer_fwd" + self.sfx, _ptr(data), _ptr(gamma), _ptr(beta), _ptr(mmean), _ptr(mvar),
                      _ptr(out_data[0]), N, C, ctypes.c_long(HxW), float(self.p["eps"]), fix, None)
                _sync()
                return
            ws, wsp, wsn = self._workspace(data, dims)
            part = _scratch(data, 4 * 2 * C)
            _call("sd_sync_bn_stats" + self.sfx, _ptr(data), _ptr(part), N, C, ctypes.c_long(HxW), wsp, wsn, None)
            parts, W, _ = self._exchange(part)
            _call("sd_sync_bn_apply" + self.sfx, _ptr(data), _ptr(parts), W, _ptr(gamma), _ptr(beta),
                  _ptr(out_data[0]), _ptr(out_data[1]), _ptr(out_data[2]), N, C, ctypes.c_long(HxW),
                  float(self.p["eps"]), fix, wsp, wsn, None)
            _sync()

        def backward(self, req, out_grad, in_data, out_data, in_grad, aux):
            # the reference Assign()s with req; the kernels store: kWriteTo or kNullOp (gradients arriving on the
            # mean / var outputs are ignored, as :372-535 ignores them)
            _require_write(req[:3], ["SyncBatchNorm data gradient", "SyncBatchNorm gamma gradient",
                                     "SyncBatchNorm beta gradient"])
            data, gamma = in_data[0], in_data[1]
            dy, mean, var = out_grad[0], out_data[1], out_data[2]
            mmean, mvar = aux[:2]
            _wait(dy, data, gamma, mean, var, mmean, mvar)
            N, C, HxW = dims = self._dims(data.shape)
            want_dx = _req(req[0]) != REQ["null"]
            want_g, want_b = [_req(r) != REQ["null"] for r in req[1:3]]
            ws, wsp, wsn = self._workspace(data, dims)
            bpart = _scratch(data, 4 * 2 * C)
            _call("sd_sync_bn_bwd_stats" + self.sfx, _ptr(dy), _ptr(data), _ptr(mean), _ptr(bpart), N, C,
                  ctypes.c_long(HxW), wsp, wsn, None)
            bparts, W, rank = self._exchange(bpart)
            # (a frozen input: dX goes to scratch; the moving statistics move whatever is frozen)
            dx = in_grad[0] if want_dx else _scratch(data, self.esz * _numel(data.shape))
            dgamma = dbeta = None
            if want_g or want_b:
                dgamma = in_grad[1] if want_g else _scratch(data, 4 * C)
                dbeta = in_grad[2] if want_b else _scratch(data, 4 * C)
            _call("sd_sync_bn_bwd_apply" + self.sfx, _ptr(dy), _ptr(data), _ptr(mean), _ptr(var), _ptr(gamma),
                  _ptr(bparts), W, rank, _ptr(dx), _ptr(dgamma), _ptr(dbeta), _ptr(mmean), _ptr(mvar),
                  float(self.p["momentum"]), N, C, ctypes.c_long(HxW), float(self.p["eps"]),
                  int(self.p["fix_gamma"]), wsp, wsn, None)
            _sync()

    class SyncBatchNormProp(Prop):
        ARGS, OUTS, AUX = ("data", "gamma", "beta"), ("output", "mean", "var"), ("moving_mean", "moving_var")
        DEPS = ((OUT_GRAD, 0), (OUT_DATA, 1), (OUT_DATA, 2), (IN_DATA, 0), (IN_DATA, 1))      # :624-634
        PARAMS = ("eps", "momentum", "fix_gamma", "use_global_stats", "output_mean_var", "ndev", "key")

        def __init__(self, eps="1e-3", momentum="0.9", fix_gamma="True", use_global_stats="False",
                     output_mean_var="False", ndev="1", key=""):
            # defaults: sync_batch_norm-inl.h:57-75
            super().__init__(need_top_grad=True)
            self.p = dict(eps=float(eps), momentum=float(momentum), fix_gamma=_bool(fix_gamma),
                          use_global_stats=_bool(use_global_stats), output_mean_var=_bool(output_mean_var),
                          ndev=int(ndev), key=str(key))
            why = self.sd_supports(dict(use_global_stats=str(use_global_stats)))
            if why:
                raise ValueError("SyncBatchNorm: " + why)
            if self.p["ndev"] < 1:
                raise ValueError("SyncBatchNorm: ndev must be at least 1, got %d" % self.p["ndev"])
            self.num_visible_outputs = 3 if self.p["output_mean_var"] else 1      # :641-646

        @classmethod
        def sd_supports(cls, params):
            """'' when the device operator takes this parameter set, else the reason (install()'s alias then calls
            the native constructor)."""
            for k in params:
                if k not in cls.PARAMS:
                    return "parameter %r is not one this operator takes" % k
            if _bool(params.get("use_global_stats", "False")):
                return "use_global_stats=True (its backward is not provided)"
            return ""

        def infer_shape(self, in_shape):
            # SyncBatchNormProp::InferShape (:556-574)
            d = tuple(int(s) for s in in_shape[0])
            if len(d) < 2:
                raise ValueError("SyncBatchNorm: data should be (batch, channel, ...), got %s" % (d,))
            c = (d[1],)
            return [d, c, c], [d, c, c], [c, c]

        def infer_type(self, in_type):
            # :576-607: with float16 data the parameters, statistics and moving statistics stay float32
            import numpy as np
            t = in_type[0]
            p = np.float32 if np.dtype(t) == np.float16 else t
            return [t, p, p], [t, p, p], [p, p]

        def create_operator(self, ctx, shapes, dtypes):
            return SyncBatchNorm(self.p, _is_f16(dtypes))

    return {SYNC_BN: SyncBatchNormProp}


# ------------------------------------------------------------------------------- registration ----
def register(mx=None):
    """Register `sd__contrib_SyncBatchNorm`.  Returns {name: PropClass}."""
    mx = _mx(mx)
    return register_ops(mx, _build_ops(mx), _own)


def _ctor(mx, prop, original):
    """the alias of `SyncBatchNorm`: the moving statistics are inputs too, every positional input is named, and an
    input the operator does not have is an error"""
    return alias_ctor(mx, SYNC_BN, prop, original, lambda *fallback: fallbacks.append(fallback), label="SyncBatchNorm",
                      aux_inputs=True, positionals="always", unknown_inputs="error", group_all=True)


def install(mx=None, stream=None, sync=True):
    """register() + alias `SyncBatchNorm` in every contrib namespace the plugin knows to the device op.  The native
    constructor is kept as `<namespace>._sd_reference_SyncBatchNorm`; uninstall() puts it back.  `stream` / `sync`
    are the plugin's (mxnet_plugin.install has the ordering contract)."""
    mx = _mx(mx)
    props = register(mx)
    _state["stream"], _state["sync"] = stream, bool(sync)
    del fallbacks[:]
    put_alias(mx, "contrib", "SyncBatchNorm", lambda original: _ctor(mx, props[SYNC_BN], original))
    _own["installed"] = True
    return props


def uninstall(mx=None):
    """Put the native `SyncBatchNorm` constructors back.  (MXNet has no way to drop a registered CustomOp: the op
    type stays known, and nothing builds it any more.)"""
    drop_alias(_mx(mx), "contrib", "SyncBatchNorm")
    _own["installed"] = False
