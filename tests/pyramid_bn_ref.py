"""The reference of pyramid batch norm IS the reference's graph (models/sepc/sepc_neck.py:112-119 with the caller's
relu, :108): concatenate the levels over the last axis, apply tests/sync_bn_ref.py to the concatenated tensor, split,
apply ReLU and its mask taken from the forward's STORED y.  Nothing else is restated; numpy only."""
import numpy as np

from . import sync_bn_ref as sr

F = np.float32
# name -> (N, C, HxW per level).  A: C odd, so rows straddle the items of 8; level sizes = 4 (mod 8), odd, and shorter
# than one item.  B: a level that is cut into chunks next to a tiny one.  C1 / C8: one level, and eight.  D (added to
# the issue's cases): a level of 264 items per channel, just past a wave's 256, so that a workgroup unit meets partial
# heads and tails (B's 16800 is a multiple of 8), next to a level that is odd.  A4: A over N = 4, for two rank slices.
SHAPES = {"A": (2, 5, (700, 175, 45, 12, 3)), "B": (3, 4, (16800, 77)), "C1": (2, 3, (64,)), "C8": (2, 3, (9,) * 8),
          "D": (2, 3, (1050, 273)), "A4": (4, 5, (700, 175, 45, 12, 3))}
TINY = 2          # the channel of case A with gamma = 1e-7, beta = 0


def concat(levels):
    return np.concatenate([np.asarray(a).reshape(a.shape[0], a.shape[1], -1) for a in levels], axis=2)


def split(a, hxw):
    return np.split(a, np.cumsum(hxw)[:-1], axis=2)


def relu(y, on):
    """mshadow_op::relu on the stored y"""
    return np.where(y > 0, y, 0).astype(y.dtype) if on else y


def masked(dy, y, on):
    """dy where the stored y is positive"""
    return np.where(y > 0, dy, 0).astype(dy.dtype) if on else dy


def make_case(name, half):
    """levels x / dy (N, C, HxW_l) float32 -- values a half holds where `half` -- with a displaced mean (offset 100,
    sigma 1) in channel 0 and the constant 1.5 in channel 1"""
    N, C, hxw = SHAPES[name]
    rs = np.random.RandomState(2032 + sum(map(ord, name)))
    xs, dys = [], []
    for h in hxw:
        x = rs.standard_normal((N, C, h))
        x[:, 0] += 100.0
        x[:, 1] = 1.5
        xs.append(x.astype(F))
        dys.append(rs.standard_normal((N, C, h)).astype(F))
    if half:
        xs, dys = ([a.astype(np.float16).astype(F) for a in v] for v in (xs, dys))
    gamma = (rs.standard_normal(C) * 0.5 + 1.0).astype(F)
    beta = rs.standard_normal(C).astype(F)
    if name.startswith("A"):
        gamma[TINY], beta[TINY] = 1e-7, 0.0
    return dict(xs=xs, dys=dys, gamma=gamma, beta=beta, eps=1e-3, N=N, C=C, hxw=hxw, n=N * sum(hxw),
                mm0=np.linspace(-1, 1, C).astype(F), mv0=np.linspace(0.5, 2, C).astype(F))


def stored(z, half):
    """z float32 -> the value the forward stores before the ReLU, as float32"""
    return z.astype(np.float16).astype(F) if half else z


def forward(c, mean, var, fix_gamma, on, half):
    """the contract's y on the concatenated tensor from the given statistics, rounded to the element type, ReLU"""
    z = sr.fwd_contract32(concat(c["xs"]), mean, var, c["gamma"], c["beta"], c["eps"], fix_gamma)
    return relu(stored(z, half), on)


def backward(c, y, mean, var, bparts, rank, fix_gamma, on, half):
    """the contract's backward on the concatenated tensor with dy masked by the stored y -> dict as bwd_contract32"""
    dy = masked(concat(c["dys"]), y, on)
    out = sr.bwd_contract32(dy, concat(c["xs"]), mean, var, c["gamma"], bparts, rank, c["n"], c["eps"], fix_gamma,
                            c["mm0"], c["mv0"], 0.9)
    out["dx"] = stored(out["dx"], half)
    return out
