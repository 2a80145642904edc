"""Restatement of the nodes the reference's merge_bn leaves behind a fixbn convolution (utils/graph_optimize.py:
34-109): _contrib_BroadcastScale (operator_cxx/contrib/broadcast_scale-inl.h:57-103: data * broadcast<1>(scaler)),
broadcast_add(beta), the shortcut's elemwise add and relu (mshadow_op::relu a > 0 ? a : 0, relu_grad a > 0 ? 1 : 0,
the backward ograd * relu_grad(out)); numpy only.

  fwd / bwd          in the dtype of the data, float32 or float16, ONE rounding per step: numpy's float16
                     arithmetic is the float operation rounded once to half, which is what mshadow's half_t
                     operators do.  bwd's dbeta is numpy's float32 sum of the g1 values of a channel.
  fwd_contracted     what a kernel that contracts would give: float32 -- the product and the first sum in float64,
                     rounded once (a fused multiply-add); float16 -- the whole chain kept in float32 and rounded to
                     half at the end.  The fixtures are checked to tell the two apart (tests/test_scale_bias_act.py).
  dbeta_truth        float64 sum of g1 per channel and T = the sum of |g1|, for k_of (tests/group_norm_ref.py):
                         k = |got - truth| / (eps32 * T + tiny)
"""
import numpy as np

from .group_norm_ref import k_of  # noqa: F401  (the one margin rule of the project)

F = np.float32
H = np.float16


def chan(v, x):
    """(C,) or (1,C,1,1) -> broadcastable against x (N, C, ...)"""
    return np.asarray(v).reshape((1, -1) + (1,) * (x.ndim - 2))


def relu(v):
    with np.errstate(invalid="ignore"):
        return np.where(v > 0, v, v.dtype.type(0))


def fwd(x, gamma, beta=None, residual=None, act=False):
    dt = x.dtype
    assert dt in (F, H) and gamma.dtype == dt
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = (x * chan(gamma, x)).astype(dt)
        if beta is not None:
            v = (v + chan(beta, x)).astype(dt)
        if residual is not None:
            v = (v + residual).astype(dt)
    return relu(v) if act else v


def g1_of(dy, y, act):
    if not act:
        return dy
    with np.errstate(invalid="ignore"):
        mask = np.where(y > 0, dy.dtype.type(1), dy.dtype.type(0))
        return (dy * mask).astype(dy.dtype)


def bwd(dy, y, gamma, act=False):
    """-> dict(dx, dres, dbeta): dres = g1, dx = g1 * gamma, dbeta float32"""
    g1 = g1_of(dy, y, act)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        dx = (g1 * chan(gamma, dy)).astype(dy.dtype)
        C = dy.shape[1]
        g32 = g1.astype(F)
        dbeta = np.stack([g32[:, c].reshape(-1).sum(dtype=F) for c in range(C)]).astype(F)
    return dict(dx=dx, dres=g1, dbeta=dbeta)


def dbeta_truth(dy, y, act=False):
    g1 = g1_of(dy, y, act).astype(np.float64)
    red = (0,) + tuple(range(2, dy.ndim))
    return g1.sum(axis=red), np.abs(g1).sum(axis=red)


def fwd_contracted(x, gamma, beta, residual=None, act=False):
    dt = x.dtype
    wide = np.float64 if dt == F else F
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        v = x.astype(wide) * chan(gamma, x).astype(wide) + chan(beta, x).astype(wide)
        if dt == F:
            v = v.astype(F)
            if residual is not None:
                v = v + residual
        elif residual is not None:
            v = v + residual.astype(wide)
        v = v.astype(dt)
    return relu(v) if act else v


def same_bits(a, b):
    """equal bit patterns; a NaN matches any NaN (the payload and sign of a generated NaN are the processor's)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb]))


def mismatch(a, b):
    """a short description of the first difference, for assertion messages"""
    a, b = np.asarray(a), np.asarray(b)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(u) != b.view(u)))
    idx = np.argwhere(bad)
    if not len(idx):
        return "equal"
    i = tuple(idx[0])
    return "%d of %d differ, first at %s: %r against %r" % (len(idx), a.size, i, a[i], b[i])


# ------------------------------------------------------------------------------------------ cases --
SHAPES = (
    (1, 1, 1, 1),        # smallest
    (2, 3, 1, 1),        # planes of one element
    (2, 5, 1, 3),        # HxW below the vector width
    (3, 4, 1, 5),        # HxW between the two vector widths: 4 floats <= 5 < 8 halves
    (1, 2, 7, 9),        # odd HxW
    (2, 3, 5, 4),        # HxW % 4 == 0
    (3, 7, 13, 21),      # odd HxW = 273: every plane phase
    (1, 2, 1, 4099),     # a plane longer than a workgroup's share, ragged tail
)
# more than one sweep of the capped grid: 2048 workgroups x 512 items of 4 floats = 4 194 304 elements per sweep
# (2 x 16 x 363 x 365 = 4 239 840, HxW = 132 495, odd), of 8 halves = 8 388 608 (2 x 16 x 517 x 509 = 8 420 896,
# HxW = 263 153, odd)
LARGE = {"float32": (2, 16, 363, 365), "float16": (2, 16, 517, 509)}
FORMS = [(b, r, a) for b in (False, True) for r in (False, True) for a in (False, True)]


def make(rs, shape, dt):
    """N(0,1) data: x, residual, dy, gamma (mean 1), beta"""
    C = shape[1]
    return dict(x=rs.standard_normal(shape).astype(dt), residual=rs.standard_normal(shape).astype(dt),
                dy=rs.standard_normal(shape).astype(dt),
                gamma=(rs.standard_normal(C) * 0.5 + 1.0).astype(dt), beta=rs.standard_normal(C).astype(dt))


def all_forms(d):
    """{(bias, residual, act): dict(y, dx, dres, dbeta, dbeta_truth, dbeta_T)} for one data set; the forward's
    intermediates are shared between the forms (each is still one rounding per step), and the backward of a form
    is given that form's own y"""
    x, g, b, r, dy = d["x"], d["gamma"], d["beta"], d["residual"], d["dy"]
    dt = x.dtype
    out = {}
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        t = (x * chan(g, x)).astype(dt)
        for hb in (False, True):
            u = (t + chan(b, x)).astype(dt) if hb else t
            for hr in (False, True):
                v = (u + r).astype(dt) if hr else u
                for act in (False, True):
                    y = relu(v) if act else v
                    if not act and (False, False, False) in out:
                        back = {k: out[(False, False, False)][k] for k in ("dx", "dres", "dbeta", "dbeta_truth", "dbeta_T")}
                    else:
                        back = bwd(dy, y, g, act)
                        back["dbeta_truth"], back["dbeta_T"] = dbeta_truth(dy, y, act)
                    out[(hb, hr, act)] = dict(back, y=y)
    return out


def edge_values(dt):
    """the values every input is swept over: signed zeros, subnormals, infinities, NaN, the format's extremes"""
    fi = np.finfo(dt)
    sub = fi.tiny / 4        # a subnormal
    v = [0.0, -0.0, sub, -sub, fi.tiny, np.inf, -np.inf, np.nan, fi.max, -fi.max, 1.0, -1.0, 0.5, -3.0,
         fi.max / 2, 1.0 + fi.eps]
    return np.array(v, dt)
