"""TEST INFRASTRUCTURE: tests/mx_numpy_eval.py (the evaluating numpy stand-in for `mx.sym` / `mx.nd`) extended by the
operators models/RepPoints/point_ops.py and the box branches of models/RepPoints/builder.py:415-437 use, so that those
functions run unmodified and produce numbers (tests/golden/make_golden_reppoints.py).  mx_numpy_eval.py is not edited.

Semantics, as MXNet documents them, float32 throughout:
  * `reshape` understands 0, -1, -2 (copy the remaining dimensions), -3 (merge two) and -4 (split one into two);
  * `topk` in its mask, value and index forms.  MXNet does not document the order among equal keys: the sort is STABLE
    here, the lower index first (the project's tie rule);
  * `mean` / `sum` over one axis and `norm` add SEQUENTIALLY along that axis (MXNet's own reduction order is not
    available; the project pins this one), `mean` divides the sum by the count;
  * `contrib.box_iou(format='corner')` restates upstream's operator (not vendored): no +1, extents clamped at 0,
    inter / (area_a + area_b - inter), 0 where the union is <= 0;
  * `min` / `max` / `argmax` (the first maximum), `take` along axis 0, `where` (condition != 0), `flip`, `repeat`,
    `split`, `arange_like`, `broadcast_like`, `log2`, `floor`, `square`, `smooth_l1` (mshadow_op::smooth_l1_loss).
"""
import types

import numpy as np

from . import mx_numpy_eval as E

F32, Arr = E.F32, E.Arr


def mx_reshape(old, spec):
    """MXNet's reshape codes"""
    old, out, i, spec, k = list(old), [], 0, list(spec), 0
    infer = None
    while k < len(spec):
        d = spec[k]
        if d == 0:
            out.append(old[i]); i += 1
        elif d == -1:
            infer = len(out); out.append(-1); i += 1
        elif d == -2:
            out.extend(old[i:]); i = len(old)
        elif d == -3:
            out.append(old[i] * old[i + 1]); i += 2
        elif d == -4:
            a, b = spec[k + 1], spec[k + 2]
            a, b = (old[i] // b if a == -1 else a), (old[i] // a if b == -1 else b)
            out.extend([a, b]); i += 1; k += 2
        else:
            out.append(d); i += 1
        k += 1
    if infer is not None:
        return tuple(-1 if j == infer else v for j, v in enumerate(out))
    return tuple(out)


def _reshape(d, shape):
    return Arr(d.v.reshape(mx_reshape(d.v.shape, shape)))


def seq_sum(v, axis, keepdims=False):
    v = np.moveaxis(v, axis, -1)
    s = np.zeros(v.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for k in range(v.shape[-1]):
            s = s + v[..., k]
    return np.expand_dims(s, axis) if keepdims else s


def _topk(d, axis=-1, k=1, ret_typ="indices", is_ascend=False):
    v = d.v if is_ascend else -d.v
    order = np.argsort(v, axis=axis, kind="stable")
    first = np.take(order, range(k), axis=axis)
    if ret_typ == "mask":
        m = np.zeros(d.v.shape, F32)
        np.put_along_axis(m, first, F32(1), axis)
        return Arr(m)
    if ret_typ == "value":
        return Arr(np.take_along_axis(d.v, first, axis))
    return Arr(first.astype(F32))


def _box_iou(lhs, rhs, format="corner"):
    assert format == "corner"
    a, g = lhs.v[..., None, :], rhs.v[None, ...]
    zero = F32(0)
    w = np.minimum(a[..., 2], g[..., 2]) - np.maximum(a[..., 0], g[..., 0])
    h = np.minimum(a[..., 3], g[..., 3]) - np.maximum(a[..., 1], g[..., 1])
    i = np.where(w < 0, zero, w) * np.where(h < 0, zero, h)
    u = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])) - i
    with np.errstate(all="ignore"):
        return Arr(np.where(u <= 0, zero, i / np.where(u <= 0, F32(1), u)))


def _smooth_l1(data, scalar=1.0, name=None):
    a, bsq = data.v, F32(scalar) * F32(scalar)
    ibsq = F32(1) / bsq
    with np.errstate(all="ignore"):
        return Arr(np.where(a > ibsq, a - F32(0.5) * ibsq, np.where(a < -ibsq, -a - F32(0.5) * ibsq, F32(0.5) * a * a * bsq)))


def _split(d, num_outputs, axis=1, squeeze_axis=False):
    parts = np.split(d.v, num_outputs, axis)
    return [Arr(np.squeeze(p, axis) if squeeze_axis else p) for p in parts]


def _broadcast_like(lhs, rhs, lhs_axes=None, rhs_axes=None):
    shape = list(lhs.v.shape)
    if lhs_axes is None:
        shape = list(rhs.v.shape)
    else:
        la, ra = (lhs_axes,) if isinstance(lhs_axes, int) else lhs_axes, (rhs_axes,) if isinstance(rhs_axes, int) else rhs_axes
        for a, b in zip(la, ra):
            shape[a] = rhs.v.shape[b]
    return Arr(np.broadcast_to(lhs.v, shape))


def _unary(f):
    def g(d):
        with np.errstate(all="ignore"):
            return Arr(f(d.v).astype(F32))
    return g


def extend(mx, X):
    """add the RepPoints operators to a stand-in made by mx_numpy_eval.make_mx(); returns the namespace `F`"""
    s = mx.sym
    s.reshape = _reshape
    s.arange = lambda start, stop=None: Arr(np.arange(start, stop) if stop is not None else np.arange(start))
    s.repeat = lambda d, repeats, axis=None: Arr(np.repeat(d.v, repeats, axis))
    s.flip = lambda d, axis: Arr(np.flip(d.v, axis))
    s.concat = lambda *a, dim=1: Arr(np.concatenate([x.v for x in a], dim))
    s.split = _split
    s.ones_like = lambda d: Arr(np.ones_like(d.v))
    s.zeros_like = lambda d: Arr(np.zeros_like(d.v))
    s.expand_dims = lambda d, axis: Arr(np.expand_dims(d.v, axis))
    s.floor, s.log2, s.square = _unary(np.floor), _unary(np.log2), _unary(np.square)
    s.maximum = lambda a, b: a._b(b, lambda x, y: np.where(x > y, x, y))
    s.broadcast_maximum = lambda a, b: a._b(b, lambda x, y: np.where(x > y, x, y))
    s.broadcast_minimum = lambda a, b: a._b(b, lambda x, y: np.where(x < y, x, y))
    s.broadcast_equal = lambda a, b: a._b(b, np.equal)
    s.broadcast_like = _broadcast_like
    s.norm = lambda d, axis=-1: Arr(np.sqrt(seq_sum(d.v * d.v, axis)))
    s.sum = lambda d, axis=None, keepdims=False: Arr(seq_sum(d.v, axis, keepdims))
    s.mean = lambda d, axis=None, keepdims=False: Arr(seq_sum(d.v, axis, keepdims) / F32(d.v.shape[axis]))
    s.argmax = lambda d, axis: Arr(np.argmax(d.v, axis).astype(F32))
    # a 1-D condition of x.shape[0] entries selects rows (MXNet's `where`)
    s.where = lambda c, x, y: Arr(np.where(c.v.reshape(c.v.shape + (1,) * (x.v.ndim - c.v.ndim)) != 0, x.v, y.v))
    s.take = lambda a, i: Arr(a.v[i.v.astype(np.int64)])
    s.topk = _topk
    s.contrib = types.SimpleNamespace(
        arange_like=lambda d, axis, start=0: Arr(np.arange(start, start + d.v.shape[axis])),
        box_iou=_box_iou)
    X.smooth_l1 = _smooth_l1
    X.concat = lambda arrs, axis=1, name=None: Arr(np.concatenate([x.v for x in arrs], axis))
    X.reshape = lambda d, shape, name=None: _reshape(d, shape)
    return s
