"""TEST INFRASTRUCTURE: an EVALUATING numpy stand-in for the dozen-odd `mx.sym` / `mx.nd` operators the
reference's FCOS target and loss graphs use (models/FCOS/input.py, models/FCOS/loss.py), so that those functions
run unmodified and produce numbers (tests/golden/make_golden_fcos.py).  tests/ref_stubs.py records graphs; this
one computes them, eagerly, in float32.

Semantics, as MXNet documents them:
  * every tensor is float32; comparisons give 0.0 / 1.0; a Python scalar operand is rounded to float32 first
    (MXNet's *_scalar operators compute in the tensor's type);
  * `argmin` returns the FIRST minimum (as float), `sort` ascends, `pick` gathers along an axis with an index
    tensor of the reduced shape, `gather_nd(data, indices)` reads data[indices[0], indices[1], ...],
    `one_hot` leaves rows of an index outside [0, depth) at zero (the index is truncated to int);
  * `reshape` understands 0 (copy the dimension) and -1 (infer);
  * `sum` is numpy's float32 sum -- the fixture's restatement (tests/fcos_ref.py) uses the same one;
  * `mx.sym.Custom` runs the registered CustomOp's forward on the spot; BlockGrad / MakeLoss are identities.
"""
import sys
import types

import numpy as np

F32 = np.float32


def _a(v):
    return v.v if isinstance(v, Arr) else F32(v)


class Arr:
    """a float32 tensor that is both the `Symbol` and the `NDArray` of this stand-in"""
    context = "cpu(0)"

    def __init__(self, v):
        self.v = np.asarray(v, F32)

    shape = property(lambda s: s.v.shape)
    T = property(lambda s: Arr(s.v.T))

    def _b(self, o, f, swap=False):
        a, b = (_a(o), self.v) if swap else (self.v, _a(o))
        with np.errstate(all="ignore"):
            return Arr(np.asarray(f(a, b)).astype(F32))

    __add__ = __radd__ = lambda s, o: s._b(o, np.add)
    __sub__ = lambda s, o: s._b(o, np.subtract)
    __rsub__ = lambda s, o: s._b(o, np.subtract, True)
    __mul__ = __rmul__ = lambda s, o: s._b(o, np.multiply)
    __truediv__ = lambda s, o: s._b(o, np.divide)
    __rtruediv__ = lambda s, o: s._b(o, np.divide, True)
    __pow__ = lambda s, o: s._b(o, np.power)
    __neg__ = lambda s: Arr(-s.v)
    __ge__ = lambda s, o: s._b(o, np.greater_equal)
    __gt__ = lambda s, o: s._b(o, np.greater)
    __le__ = lambda s, o: s._b(o, np.less_equal)
    __lt__ = lambda s, o: s._b(o, np.less)
    __ne__ = lambda s, o: s._b(o, np.not_equal)
    __eq__ = lambda s, o: s._b(o, np.equal)
    __hash__ = object.__hash__

    def __bool__(self):
        return bool(self.v)

    def __getitem__(self, k):
        return Arr(self.v[k])

    def reshape(self, *shape, **kw):
        shape = kw.get("shape", shape[0] if len(shape) == 1 and isinstance(shape[0], (tuple, list)) else shape)
        return Arr(self.v.reshape(_mx_shape(self.v.shape, shape)))

    def tile(self, reps):
        return Arr(np.tile(self.v, reps))

    def as_in_context(self, ctx):
        return self


def _mx_shape(old, new):
    return tuple(old[i] if d == 0 else d for i, d in enumerate(new))


def _slice(data, begin, end, step=None):
    step = step or (None,) * len(begin)
    return Arr(data.v[tuple(slice(b, e, s) for b, e, s in zip(begin, end, step))])


def _pick(data, index, axis, keepdims=False):
    idx = np.expand_dims(index.v.astype(np.int64), axis)
    out = np.take_along_axis(data.v, idx, axis)
    return Arr(out if keepdims else np.squeeze(out, axis))


def _one_hot(indices, depth):
    idx = np.trunc(indices.v).astype(np.int64)
    return Arr((idx[..., None] == np.arange(depth)).astype(F32))


def make_mx():
    mx = types.ModuleType("mxnet")
    registry, customs = {}, []

    class CustomOp:
        def assign(self, dst, req, src):
            dst.append(src if isinstance(src, Arr) else Arr(src))

    class CustomOpProp:
        def __init__(self, need_top_grad=True):
            self.need_top_grad_ = need_top_grad

    def register(name):
        def deco(cls):
            registry[name] = cls
            return cls
        return deco

    def Custom(*args, op_type=None, name=None, **kw):
        prop = registry[op_type]()
        ins = list(args) + [kw[k] for k in prop.list_arguments() if k in kw]
        outs = [[] for _ in prop.list_outputs()]
        prop.create_operator(None, None, None).forward(True, ["write"] * len(outs), ins, outs, [])
        customs.append((op_type, name, dict(kw)))
        res = [o[0] for o in outs]
        return res[0] if len(res) == 1 else res

    s = types.ModuleType("mxnet.symbol")
    s.Custom = Custom
    for n, f in (("sub", np.subtract), ("add", np.add), ("mul", np.multiply), ("div", np.divide),
                 ("logical_and", np.logical_and), ("greater_equal", np.greater_equal), ("lesser", np.less),
                 ("greater", np.greater), ("not_equal", np.not_equal)):
        setattr(s, "broadcast_" + n, (lambda f: lambda lhs, rhs: lhs._b(rhs, f))(f))
    s.slice = _slice
    s.slice_axis = lambda data, axis, begin, end: Arr(np.take(data.v, range(begin, end), axis))
    s.stack = lambda *a, axis=0: Arr(np.stack([x.v for x in a], axis))
    s.min = lambda d, axis=None, keepdims=False: Arr(d.v.min(axis=axis, keepdims=keepdims))
    s.max = lambda d, axis=None, keepdims=False: Arr(d.v.max(axis=axis, keepdims=keepdims))
    s.argmin = lambda d, axis: Arr(np.argmin(d.v, axis))          # numpy: the first occurrence
    s.tile = lambda d, reps: d.tile(reps)
    s.pick = _pick
    s.reshape_like = lambda a, b: Arr(a.v.reshape(b.v.shape))
    s.reshape = lambda d, shape: d.reshape(shape)
    s.sort = lambda d, axis=-1: Arr(np.sort(d.v, axis))
    s.sqrt = lambda d: d._b(0, lambda a, b: np.sqrt(a))
    s.exp = lambda d: d._b(0, lambda a, b: np.exp(a))
    s.log = lambda d: d._b(0, lambda a, b: np.log(a))
    s.clip = lambda d, a_min, a_max: Arr(np.clip(d.v, F32(a_min), F32(a_max)))
    s.sum = lambda d: Arr(np.sum(d.v, dtype=F32).reshape(1))
    s.gather_nd = lambda d, i: Arr(d.v[tuple(i.v.astype(np.int64))])
    s.one_hot = _one_hot
    s.transpose = lambda d, axes: Arr(np.transpose(d.v, axes))
    s.zeros = lambda shape: Arr(np.zeros(shape, F32))
    s.full = lambda shape, val: Arr(np.full(shape, val, F32))
    nd = types.ModuleType("mxnet.ndarray")
    nd.from_numpy = Arr
    nd.full = s.full
    nd.concat = lambda *a, dim=0: Arr(np.concatenate([x.v for x in a], dim))
    nd.logical_and = lambda lhs, rhs: lhs._b(rhs, np.logical_and)
    nd.arange = lambda n: Arr(np.arange(n))
    mx.sym = mx.symbol = s
    mx.nd = mx.ndarray = nd
    mx.operator = types.SimpleNamespace(CustomOp=CustomOp, CustomOpProp=CustomOpProp, register=register)
    mx.registry, mx.customs = registry, customs
    X = types.ModuleType("mxnext")
    X.block_grad = lambda d, **kw: d
    X.loss = lambda d, grad_scale=1, name=None: d
    return mx, X


class modules:
    """context manager: the stand-ins as `mxnet` / `mxnext`, `root` on sys.path, and a placeholder for the config
    module the FCOS CustomOpProps import their settings from (input.py:88,147)"""

    def __init__(self, root, throwout_param):
        self.root, self.param = root, throwout_param

    def __enter__(self):
        self.mx, self.X = make_mx()
        cfg_pkg = types.ModuleType("config")
        cfg_pkg.__path__ = []
        cfg = types.ModuleType("config.fcos_r50v1_fpn_1x")
        cfg.throwout_param = self.param
        self.before = dict(sys.modules)
        sys.modules.update({"mxnet": self.mx, "mxnext": self.X, "config": cfg_pkg, "config.fcos_r50v1_fpn_1x": cfg})
        sys.path.insert(0, self.root)
        return self

    def __exit__(self, *a):
        sys.path.remove(self.root)
        for k in list(sys.modules):
            if k not in self.before:
                del sys.modules[k]
        sys.modules.update(self.before)
        return False
