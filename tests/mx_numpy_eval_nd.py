"""TEST INFRASTRUCTURE: tests/mx_numpy_eval.py extended with the `mx.nd` surface the reference's FCOS test-time
CustomOps use (models/FCOS/utils.py: get_proposal_single_stage, get_batch_proposal), so that both run unmodified and
produce numbers (tests/golden/make_golden_fcos_decode.py).

Semantics, as MXNet documents them:
  * an NDArray keeps its dtype (`astype(int)` truncates toward zero and gives int64); a Python or numpy scalar operand
    is converted to the array's dtype first (MXNet's *_scalar operators compute in the tensor's type); comparisons give
    0 / 1 in the operands' dtype;
  * `topk(ret_typ='both')` returns (values, indices-as-float32) in descending order and `argsort(is_ascend=False)`
    float32 indices.  MXNet does not document the order among equal keys; this stand-in makes both STABLE, the lower
    index first (-0.0 and +0.0 compare equal) -- the fixture script asserts that no case depends on that choice;
  * `reshape` understands 0 (copy the dimension), `shape=` and a bare int; `clip` converts its bounds to the dtype;
  * indexing with NDArrays (or numpy integer arrays) is numpy's integer-array indexing, slice assignment writes in
    place, `asnumpy()` copies.
"""
import sys
import types

import numpy as np

from . import mx_numpy_eval as base

F32 = np.float32


def _idx(k):
    if isinstance(k, ND):
        return k.v.astype(np.int64)
    if isinstance(k, tuple):
        return tuple(_idx(e) for e in k)
    return k


class ND:
    """an NDArray of this stand-in: a numpy array that keeps its dtype"""
    context = "cpu(0)"

    def __init__(self, v, dtype=None):
        v = v.v if isinstance(v, (ND, base.Arr)) else v
        self.v = np.asarray(v, dtype)

    shape = property(lambda s: s.v.shape)
    size = property(lambda s: s.v.size)
    dtype = property(lambda s: s.v.dtype)

    def _o(self, o):
        return o.v if isinstance(o, (ND, base.Arr)) else np.asarray(o).astype(self.v.dtype)

    def _b(self, o, f, swap=False, compare=False):
        a, b = (self._o(o), self.v) if swap else (self.v, self._o(o))
        with np.errstate(all="ignore"):
            r = np.asarray(f(a, b))
        return ND(r.astype(self.v.dtype))

    __add__ = __radd__ = lambda s, o: s._b(o, np.add)
    __sub__ = lambda s, o: s._b(o, np.subtract)
    __rsub__ = lambda s, o: s._b(o, np.subtract, True)
    __mul__ = __rmul__ = lambda s, o: s._b(o, np.multiply)
    __truediv__ = lambda s, o: s._b(o, np.divide)
    __mod__ = lambda s, o: s._b(o, np.fmod)          # non-negative operands here: fmod == MXNet's mod
    __neg__ = lambda s: ND(-s.v)
    __ge__ = lambda s, o: s._b(o, np.greater_equal)
    __gt__ = lambda s, o: s._b(o, np.greater)
    __le__ = lambda s, o: s._b(o, np.less_equal)
    __lt__ = lambda s, o: s._b(o, np.less)
    __hash__ = object.__hash__

    def __bool__(self):
        if self.v.size != 1:
            raise ValueError("the truth value of an NDArray with more than one element is ambiguous")
        return bool(self.v.reshape(-1)[0])

    def __len__(self):
        return self.v.shape[0]

    def __getitem__(self, k):
        return ND(self.v[_idx(k)])

    def __setitem__(self, k, val):
        self.v[_idx(k)] = val.v if isinstance(val, (ND, base.Arr)) else val

    def astype(self, dtype):
        return ND(self.v.astype(np.int64 if dtype is int else dtype))

    def asnumpy(self):
        return np.array(self.v)

    def reshape(self, *shape, **kw):
        shape = kw.get("shape", shape[0] if len(shape) == 1 else shape)
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        return ND(self.v.reshape(base._mx_shape(self.v.shape, tuple(shape))))


def _desc_order(v):
    """indices of a stable descending sort: equal keys keep their order (-0.0 == +0.0)"""
    return np.argsort(-np.asarray(v), kind="stable")


def _topk(data, axis=0, ret_typ="indices", k=1):
    assert data.v.ndim == 1 and axis == 0 and ret_typ == "both"
    order = _desc_order(data.v)[:k]
    return ND(data.v[order]), ND(order.astype(F32))


def _argsort(data, axis=-1, is_ascend=True):
    assert data.v.ndim == 1
    order = np.argsort(data.v, kind="stable") if is_ascend else _desc_order(data.v)
    return ND(order.astype(F32))


def make_mx():
    """the base stand-in with `mx.nd` replaced by the dtype-keeping surface of utils.py"""
    mx, X = base.make_mx()
    nd = types.ModuleType("mxnet.ndarray")
    for n, f in (("greater", np.greater), ("mul", np.multiply), ("add", np.add)):
        setattr(nd, "broadcast_" + n, (lambda f: lambda lhs, rhs: lhs._b(rhs, f))(f))
    nd.full = lambda shape, val, ctx=None, dtype=F32: ND(np.full(tuple(shape), val, dtype))
    nd.sum = lambda d: ND(np.sum(d.v, dtype=d.v.dtype).reshape(1))
    nd.topk = _topk
    nd.argsort = _argsort
    nd.reshape = lambda d, shape: d.reshape(shape=shape)
    nd.array = lambda src, ctx=None, dtype=F32: ND(np.array(src.v if isinstance(src, ND) else src, dtype))
    nd.clip = lambda d, a_min, a_max: ND(np.clip(d.v, d.v.dtype.type(a_min), d.v.dtype.type(a_max)))
    nd.stack = lambda *a, axis=0: ND(np.stack([x.v for x in a], axis))
    nd.concat = lambda *a, dim=1: ND(np.concatenate([x.v for x in a], dim))
    mx.nd = mx.ndarray = nd

    class CustomOp:
        def assign(self, dst, req, src):
            dst.append(src if isinstance(src, ND) else ND(src))

    mx.operator = types.SimpleNamespace(CustomOp=CustomOp, CustomOpProp=mx.operator.CustomOpProp,
                                        register=mx.operator.register)
    return mx, X


def run_custom(mx, op_type, ins, **kw):
    """the registered CustomOp's forward on NDArrays `ins`; returns its outputs (a list of ND)"""
    prop = mx.registry[op_type](**kw)
    outs = [[] for _ in prop.list_outputs()]
    prop.create_operator(None, None, None).forward(False, ["write"] * len(outs), list(ins), outs, [])
    return [o[0] if isinstance(o[0], ND) else ND(o[0]) for o in outs]


class modules:
    """context manager: the stand-ins as `mxnet` / `mxnext` and `root` on sys.path"""

    def __init__(self, root):
        self.root = root

    def __enter__(self):
        self.mx, self.X = make_mx()
        self.before = dict(sys.modules)
        sys.modules.update({"mxnet": self.mx, "mxnext": self.X})
        sys.path.insert(0, self.root)
        return self

    def __exit__(self, *a):
        sys.path.remove(self.root)
        for k in list(sys.modules):
            if k not in self.before:
                del sys.modules[k]
        sys.modules.update(self.before)
        return False
