"""The squeeze-and-excitation block (models/efficientnet/builder.py:17-27) restated; numpy only, in the scheme of
tests/sync_bn_ref.py (its k_of is the yardstick here too).

  fwd_truth / bwd_truth   float64, from the inputs as they are (float32, or halves widened).  The backward takes gap,
                          z1 and a as float32 INPUTS, as the operator does.  Each returns, per output element, T = the
                          sum of the absolute values of the terms of the float64 expression:
                              k = |got - truth| / (eps32 * T + tiny)                                          (k_of)
  fwd_ref32 / bwd_ref32   the reference's graph in float32: mean over W then over H, the two matrix products, clip,
                          sigmoid, multiply; backwards, broadcast_mul's gradient materialised and reduced, the
                          sigmoid's, the clip's inclusive mask (upstream MXNet's clip: 0 <= z1 <= 6 passes), the
                          products, and mean's gradient divided by W and then by H.  They exist to produce k_ref; the
                          device passes at k_gpu <= 2 * k_ref + 2 per output (`passes`).
T follows each expression with absolute values: Tgap = sum |x| / HW, Tz1 = |w1| Tgap + |b1|,
Ta = a (1 - a) (|w2| Tz1 + |b2|) + a, Ts = sum |dy| |x|, and so on through the backward.
"""
import numpy as np

from .group_norm_ref import k_of  # noqa: F401  (the yardstick of tests/group_norm_ref.py, re-exported)

F = np.float32
D = np.float64
FWD_OUTPUTS = ("gap", "z1", "a")
BWD_OUTPUTS = ("g", "dw1", "dw2", "db1", "db2")


def passes(k_gpu, k_ref):
    """the project's margin rule"""
    return k_gpu <= 2 * k_ref + 2


def _planes(x):
    return np.asarray(x).reshape(x.shape[0], x.shape[1], -1)


def _mat(w):
    return np.asarray(w).reshape(w.shape[0], w.shape[1])


def _bias(b, n, dtype):
    return np.zeros(n, dtype) if b is None else np.asarray(b).astype(dtype)


def fwd_truth(x, w1, b1, w2, b2):
    """-> dict(gap, z1, a, y) float64, dict of T for gap, z1, a"""
    p = _planes(x).astype(D)
    W1, W2 = _mat(w1).astype(D), _mat(w2).astype(D)
    B1, B2 = _bias(b1, W1.shape[0], D), _bias(b2, W2.shape[0], D)
    gap, Tgap = p.mean(axis=2), np.abs(p).mean(axis=2)
    z1 = gap @ W1.T + B1
    Tz1 = Tgap @ np.abs(W1).T + np.abs(B1)
    h = np.clip(z1, 0.0, 6.0)
    z2 = h @ W2.T + B2
    Tz2 = Tz1 @ np.abs(W2).T + np.abs(B2)
    a = 1.0 / (1.0 + np.exp(-z2))
    y = (p * a[:, :, None]).reshape(np.shape(x))
    return dict(gap=gap, z1=z1, a=a, y=y), dict(gap=Tgap, z1=Tz1, a=a * (1.0 - a) * Tz2 + a)


def bwd_truth(dy, x, gap, z1, a, w1, w2):
    """gap, z1, a: the float32 arrays the operator is given -> dict(g, dw1, dw2, db1, db2, dx) float64, dict of T"""
    p, q = _planes(x).astype(D), _planes(dy).astype(D)
    W1, W2 = _mat(w1).astype(D), _mat(w2).astype(D)
    gap, z1, a = np.asarray(gap, F).astype(D), np.asarray(z1, F).astype(D), np.asarray(a, F).astype(D)
    hw = p.shape[2]
    s, Ts = (q * p).sum(axis=2), (np.abs(q) * np.abs(p)).sum(axis=2)
    sp = a * (1.0 - a)
    dz2, Tdz2 = s * sp, Ts * sp
    mask = ((z1 >= 0.0) & (z1 <= 6.0)).astype(D)
    dz1, Tdz1 = (dz2 @ W2) * mask, (Tdz2 @ np.abs(W2)) * mask
    g, Tg = dz1 @ W1 / hw, Tdz1 @ np.abs(W1) / hw
    h = np.clip(z1, 0.0, 6.0)
    out = dict(g=g, dw2=dz2.T @ h, db2=dz2.sum(axis=0), dw1=dz1.T @ gap, db1=dz1.sum(axis=0),
               dx=(q * a[:, :, None] + g[:, :, None]).reshape(np.shape(x)))
    T = dict(g=Tg, dw2=Tdz2.T @ np.abs(h), db2=Tdz2.sum(axis=0), dw1=Tdz1.T @ np.abs(gap), db1=Tdz1.sum(axis=0))
    return out, T


def fwd_ref32(x, w1, b1, w2, b2):
    """the reference's seven nodes in float32 (x as (N, C, H, W))"""
    x = np.asarray(x).astype(F)
    W1, W2 = _mat(w1).astype(F), _mat(w2).astype(F)
    gap = x.mean(axis=-1, dtype=F).mean(axis=-1, dtype=F)
    z1 = (gap @ W1.T + _bias(b1, W1.shape[0], F)).astype(F)
    h = np.clip(z1, F(0), F(6))
    z2 = (h @ W2.T + _bias(b2, W2.shape[0], F)).astype(F)
    a = (F(1) / (F(1) + np.exp(-z2, dtype=F))).astype(F)
    return dict(gap=gap, z1=z1, a=a, y=(x * a[:, :, None, None]).astype(F))


def bwd_ref32(dy, x, gap, z1, a, w1, w2):
    """the graph's backward in float32 from the same float32 gap, z1, a"""
    x, dy = np.asarray(x).astype(F), np.asarray(dy).astype(F)
    W1, W2 = _mat(w1).astype(F), _mat(w2).astype(F)
    gap, z1, a = np.asarray(gap, F), np.asarray(z1, F), np.asarray(a, F)
    H, W = x.shape[2], x.shape[3]
    da = (dy * x).astype(F).sum(axis=(2, 3), dtype=F)                  # broadcast_mul towards the gate
    dz2 = (da * (a * (F(1) - a))).astype(F)
    mask = ((z1 >= 0) & (z1 <= 6)).astype(F)
    dz1 = ((dz2 @ W2) * mask).astype(F)
    g = ((dz1 @ W1) / F(W) / F(H)).astype(F)                           # mean over H, then over W, backwards
    h = np.clip(z1, F(0), F(6))
    return dict(g=g, dw2=dz2.T @ h, db2=dz2.sum(axis=0, dtype=F), dw1=dz1.T @ gap, db1=dz1.sum(axis=0, dtype=F),
                dx=((dy * a[:, :, None, None]).astype(F) + g[:, :, None, None]).astype(F))


def make_case(seed, shape, Cr, half=False, bias=False):
    """inputs of one case; z1 is spread over a few units about 3 so that the clip's three regions are reached (the
    tests assert that they are).  half: every input holds half-representable values."""
    rs = np.random.RandomState(seed)
    N, C = shape[:2]
    x = (rs.standard_normal(shape) + rs.standard_normal((N, C) + (1,) * (len(shape) - 2))).astype(F)
    dy = rs.standard_normal(shape).astype(F)
    w1 = (rs.standard_normal((Cr, C, 1, 1)) * (6.0 / np.sqrt(C))).astype(F)
    w2 = (rs.standard_normal((C, Cr, 1, 1)) * (0.5 / np.sqrt(Cr))).astype(F)
    b1 = (rs.standard_normal(Cr) + 3.0).astype(F) if bias else None
    b2 = rs.standard_normal(C).astype(F) if bias else None
    c = dict(x=x, dy=dy, w1=w1, b1=b1, w2=w2, b2=b2)
    if half:
        c = {k: None if v is None else v.astype(np.float16).astype(F) for k, v in c.items()}
    return c
