"""Restatements of the reference's SyncBatchNorm (operator_cxx/contrib/sync_batch_norm-inl.h:246-535); numpy only,
in the scheme of tests/group_norm_ref.py (its k_of is the yardstick here too).  The reference's operator needs
MXNet, several GPUs in one process and a host barrier, so it is pinned by restatement.

  fwd_truth / bwd_truth     float64 batch normalisation over the WHOLE batch, from the float32 inputs.  The backward
                            takes mean and var as float32 INPUTS, as the operator does.  Each returns, per output
                            element, T = the sum of the absolute values of the terms of the float64 expression:
                                k = |got - truth| / (eps32 * T + tiny)                                        (k_of)
  fwd_ref32 / bwd_ref32     the REFERENCE's own expressions in float32 over W rank slices: per rank
                            scale * sum(x), scale * sum(x * x) (:333-334) and sum(dy), sum(dy * (x - mean))
                            (:476-477); the exchange as SharedND does it, float adds in rank order and then
                            `* 1.0f / W` (:146-158); var = E[x^2] - mean^2 (:353); the per-element divide (:354-357);
                            gvar / gmean and the data gradient of :496-513.  Reductions inside a rank are numpy's
                            float32 sums: the order of mshadow's reduction is no part of what the operator
                            promises.  They exist only to produce k_ref.
  combine_contract /        the arithmetic contract of simpledet_amd/csrc/sync_bn.hip behind the statistics, given
  *_contract32              the float32 partials as INPUTS: the combine in double in rank order, the coefficients
                            inv, a, b, c, the element rules, the parameter gradients and the moving update.  The
                            device must match these bit for bit.

T per output (x, dy, g, beta, mean stand for their absolute values; n = the whole batch's count per channel):
  mean    sum x / n
  var     W = 1: var (every term of the variance about the mean is positive).  W > 1: var +
          (2 / W) * sum_r |mean_r - mean| * (sum x_r / n_r), the first-order reach of a rank mean's own rounding
  y       g * (x + sum x / n) * inv + beta
  bpart   per rank: sum dy;  sum dy * (x + mean)
  dx      g * dy * inv + g * (sum dy * (x + mean) / n) * inv^3 * (x + mean) + g * (sum dy / n) * inv
  dgamma  sum dy * (x + mean) * inv          dbeta   sum dy
"""
import numpy as np

from .group_norm_ref import k_of  # noqa: F401  (the yardstick of tests/group_norm_ref.py, re-exported)

F = np.float32
D = np.float64


def _c(v, x):
    """(C,) -> broadcastable against x (N, C, ...)"""
    return np.asarray(v).reshape((1, -1) + (1,) * (x.ndim - 2))


def _axes(x):
    return (0,) + tuple(range(2, x.ndim))


def _g(gamma, fix_gamma, dtype):
    gamma = np.asarray(gamma, F)
    return np.ones_like(gamma, dtype=dtype) if fix_gamma else gamma.astype(dtype)


def slices(a, W):
    """the W rank slices of the batch axis (equal sizes)"""
    N = a.shape[0]
    assert N % W == 0
    return [a[r * (N // W):(r + 1) * (N // W)] for r in range(W)]


def count(x):
    return x.shape[0] * int(np.prod(x.shape[2:], dtype=np.int64))


# ------------------------------------------------------------------------------------------ truths --
def fwd_truth(x, gamma, beta, eps, fix_gamma, W=1):
    """-> dict(y, mean, var) float64, dict of T"""
    x = np.asarray(x, F)
    x64 = x.astype(D)
    ax = _axes(x)
    mean = x64.mean(axis=ax)
    var = ((x64 - _c(mean, x)) ** 2).mean(axis=ax)
    inv = 1.0 / np.sqrt(var + float(F(eps)))
    g, b = _g(gamma, fix_gamma, D), np.asarray(beta, F).astype(D)
    y = _c(g, x) * (x64 - _c(mean, x)) * _c(inv, x) + _c(b, x)
    Tmean = np.abs(x64).mean(axis=ax)
    Tvar = var.copy()
    if W > 1:
        for xr in slices(x64, W):
            Tvar += (2.0 / W) * np.abs(xr.mean(axis=ax) - mean) * np.abs(xr).mean(axis=ax)
    Ty = np.abs(_c(g, x)) * (np.abs(x64) + _c(Tmean, x)) * _c(inv, x) + np.abs(_c(b, x))
    return dict(y=y, mean=mean, var=var), dict(y=Ty, mean=Tmean, var=Tvar)


def bwd_truth(dy, x, mean, var, gamma, eps, fix_gamma, W=1):
    """mean, var: the float32 (C,) arrays the operator is given -> dict(dx, dgamma, dbeta, bpart (W, 2, C)) float64
    and the dict of T.  dgamma / dbeta are the sums over all ranks."""
    x = np.asarray(x, F)
    x64, dy64 = x.astype(D), np.asarray(dy, F).astype(D)
    ax = _axes(x)
    n = count(x)
    m, v = np.asarray(mean, F).astype(D), np.asarray(var, F).astype(D)
    inv = 1.0 / np.sqrt(v + float(F(eps)))
    g = _g(gamma, fix_gamma, D)
    xc, axc = x64 - _c(m, x), np.abs(x64) + np.abs(_c(m, x))
    SG, SP = dy64.sum(axis=ax), (dy64 * xc).sum(axis=ax)
    TSG, TSP = np.abs(dy64).sum(axis=ax), (np.abs(dy64) * axc).sum(axis=ax)
    sg, sp = SG / n, SP / n
    dx = _c(g, x) * dy64 * _c(inv, x) - _c(g * sp * inv ** 3, x) * xc - _c(g * sg * inv, x)
    ag = np.abs(g)
    Tdx = _c(ag, x) * np.abs(dy64) * _c(inv, x) + _c(ag * (TSP / n) * inv ** 3, x) * axc + _c(ag * (TSG / n) * inv, x)
    zero = np.zeros_like(SP)
    dgamma, Tdg = (zero, zero) if fix_gamma else (SP * inv, TSP * inv)
    bpart = np.stack([np.stack([dr.sum(axis=ax), (dr * (xr - _c(m, x))).sum(axis=ax)])
                      for dr, xr in zip(slices(dy64, W), slices(x64, W))])
    Tbp = np.stack([np.stack([np.abs(dr).sum(axis=ax), (np.abs(dr) * (np.abs(xr) + np.abs(_c(m, x)))).sum(axis=ax)])
                    for dr, xr in zip(slices(dy64, W), slices(x64, W))])
    return (dict(dx=dx, dgamma=dgamma, dbeta=SG, bpart=bpart), dict(dx=Tdx, dgamma=Tdg, dbeta=TSG, bpart=Tbp))


# ------------------------------------------------------------------- the reference's own arithmetic --
def _shared_mean(per_rank):
    """SharedND::MeanReady (:146-158): data_[0] += data_[i] in rank order, then * 1.0f / ndev"""
    acc = per_rank[0].astype(F)
    for p in per_rank[1:]:
        acc = (acc + p).astype(F)
    return ((acc * F(1.0)) / F(len(per_rank))).astype(F)


def fwd_ref32(x, gamma, beta, eps, fix_gamma, W=1):
    x = np.asarray(x, F)
    ax = _axes(x)
    xs = slices(x, W)
    scale = F(1.0) / F(count(xs[0]))                       # shape_[1] / Size (:278-279)
    mean = _shared_mean([(scale * xr.sum(axis=ax, dtype=F)).astype(F) for xr in xs])
    ex2 = _shared_mean([(scale * (xr * xr).sum(axis=ax, dtype=F)).astype(F) for xr in xs])
    var = (ex2 - mean * mean).astype(F)
    g, b = _g(gamma, fix_gamma, F), np.asarray(beta, F)
    with np.errstate(invalid="ignore", divide="ignore"):
        y = (_c(g, x) * (x - _c(mean, x)) / np.sqrt(_c(var + F(eps), x)) + _c(b, x)).astype(F)
    return dict(y=y, mean=mean, var=var)


def bwd_ref32(dy, x, mean, var, gamma, eps, fix_gamma, W=1):
    """-> dict(dx, dgamma, dbeta, bpart); dgamma / dbeta summed over the ranks in rank order (the all-reduce)"""
    x, dy = np.asarray(x, F), np.asarray(dy, F)
    ax = _axes(x)
    mean, var = np.asarray(mean, F), np.asarray(var, F)
    g = _g(gamma, fix_gamma, F)
    xs, ds = slices(x, W), slices(dy, W)
    scale = F(1.0) / F(count(xs[0]))
    sums = [(dr.sum(axis=ax, dtype=F), (dr * (xr - _c(mean, x))).sum(axis=ax, dtype=F)) for dr, xr in zip(ds, xs)]
    sumGrad = _shared_mean([s[0] for s in sums])
    sumProd = _shared_mean([s[1] for s in sums])
    with np.errstate(invalid="ignore", divide="ignore"):
        gvar = (F(-0.5) * sumProd * g * np.power(var + F(eps), F(-1.5))).astype(F)
        gmean = (sumGrad * g).astype(F)
        gmean = (gmean * (F(-1.0) / np.sqrt(var + F(eps)))).astype(F)
        dxs, dgs = [], []
        for dr, xr in zip(ds, xs):
            xc = xr - _c(mean, x)
            dxs.append(((dr * _c(g, x)) * _c(F(1.0) / np.sqrt(var + F(eps)), x) + _c(gvar, x) * scale * F(2.0) * xc
                        + _c(gmean, x) * scale).astype(F))
            dgs.append((dr * xc / np.sqrt(_c(var + F(eps), x))).sum(axis=ax, dtype=F))
    dgamma, dbeta = dgs[0], sums[0][0]
    for r in range(1, W):
        dgamma, dbeta = (dgamma + dgs[r]).astype(F), (dbeta + sums[r][0]).astype(F)
    if fix_gamma:
        dgamma = np.zeros_like(dbeta)
    return dict(dx=np.concatenate(dxs), dgamma=dgamma, dbeta=dbeta, bpart=np.stack([np.stack(s) for s in sums]))


# ------------------------------------------------------------------------------ the contract --
def combine_contract(parts):
    """parts (W, 2, C) float32 -> mean, var float32: double, rank order"""
    parts = np.asarray(parts, F)
    W = parts.shape[0]
    sm = np.zeros(parts.shape[2], D)
    for r in range(W):
        sm = sm + parts[r, 0].astype(D)
    m = sm / D(W)
    sv = np.zeros(parts.shape[2], D)
    for r in range(W):
        d = parts[r, 0].astype(D) - m
        sv = sv + (parts[r, 1].astype(D) + d * d)
    return m.astype(F), (sv / D(W)).astype(F)


def _inv(var, eps):
    return (F(1.0) / np.sqrt(np.asarray(var, F) + F(eps))).astype(F)


def fwd_contract32(x, mean, var, gamma, beta, eps, fix_gamma):
    x = np.asarray(x, F)
    mean = np.asarray(mean, F)
    inv, g, b = _inv(var, eps), _g(gamma, fix_gamma, F), np.asarray(beta, F)
    return ((_c(g, x) * (x - _c(mean, x))) * _c(inv, x) + _c(b, x)).astype(F)


def infer_contract32(x, gamma, beta, moving_mean, moving_var, eps, fix_gamma):
    x = np.asarray(x, F)
    g, b = _g(gamma, fix_gamma, F), np.asarray(beta, F)
    sd = np.sqrt(np.asarray(moving_var, F) + F(eps)).astype(F)
    a = (g / sd).astype(F)
    bb = (b - ((g * np.asarray(moving_mean, F)).astype(F) / sd).astype(F)).astype(F)
    return (_c(a, x) * x + _c(bb, x)).astype(F)


def bwd_contract32(dy, x, mean, var, gamma, bparts, rank, n, eps, fix_gamma, moving_mean=None, moving_var=None,
                   momentum=0.9):
    """n: the rank's count per channel -> dict(dx, dgamma, dbeta[, moving_mean, moving_var])"""
    x, dy = np.asarray(x, F), np.asarray(dy, F)
    bparts = np.asarray(bparts, F)
    mean, var = np.asarray(mean, F), np.asarray(var, F)
    W = bparts.shape[0]
    SG, SP = np.zeros(bparts.shape[2], D), np.zeros(bparts.shape[2], D)
    for r in range(W):
        SG = SG + bparts[r, 0].astype(D)
        SP = SP + bparts[r, 1].astype(D)
    wn = D(W) * D(n)
    sg, sp = (SG / wn).astype(F), (SP / wn).astype(F)
    inv, g = _inv(var, eps), _g(gamma, fix_gamma, F)
    a = (g * inv).astype(F)
    b = ((-(g * sp).astype(F)) * ((inv * inv).astype(F) * inv).astype(F)).astype(F)
    c = ((-(g * sg).astype(F)) * inv).astype(F)
    dx = ((dy * _c(a, x) + _c(b, x) * (x - _c(mean, x))) + _c(c, x)).astype(F)
    out = dict(dx=dx, dbeta=bparts[rank, 0].copy(),
               dgamma=np.zeros_like(inv) if fix_gamma else (bparts[rank, 1] * inv).astype(F))
    if moving_mean is not None:
        mom, one = F(momentum), F(F(1.0) - F(momentum))
        out["moving_mean"] = (np.asarray(moving_mean, F) * mom + mean * one).astype(F)
        out["moving_var"] = (np.asarray(moving_var, F) * mom + var * one).astype(F)
    return out


# ------------------------------------------------------------------------------------------ cases --
SHAPES = ((6, 5), (3, 7, 5, 9), (6, 16, 8, 8), (6, 1, 3, 3), (1, 4, 24, 24), (6, 8, 100, 168))
SPLIT_SHAPE = (6, 8, 100, 168)
GAMMAS = ("ones", "random", "zeros")
OFFSETS = (0.0, 3.0, 100.0)
EPSS = (1e-3, 1e-5)
OUTPUTS = ("mean", "var", "bpart", "y", "dx", "dgamma", "dbeta")
STAT_OUTPUTS = ("mean", "var", "bpart")


def make_gamma(rs, C, kind):
    if kind == "ones":
        return np.ones(C, F)
    g = (rs.standard_normal(C) * 0.5 + 1.0).astype(F)
    if kind == "zeros":
        g[::3] = 0.0
    return g


def make_case(rs, shape, gamma_kind, fix_gamma, offset, eps):
    C = shape[1]
    x = rs.standard_normal(shape).astype(D)
    # per-channel offset of the mean, in standard deviations (sigma = 1), alternating in sign over the channels
    off = offset * np.where(np.arange(C) % 2 == 0, 1.0, -1.0)
    x = (x + _c(off, x)).astype(F)
    return dict(x=x, gamma=make_gamma(rs, C, gamma_kind), beta=rs.standard_normal(C).astype(F),
                dy=rs.standard_normal(shape).astype(F), eps=eps, fix_gamma=fix_gamma, offset=offset, shape=shape)


def constant_case():
    """channel 1 is the constant 1.5 over 64 elements: every sum the reference or the device forms is exact, the
    variance is exactly 0 and inv = 1 / sqrt(eps)"""
    rs = np.random.RandomState(77)
    c = make_case(rs, (2, 4, 4, 8), "random", False, 0.0, 1e-5)
    c["x"][:, 1] = 1.5
    return c


def cases():
    """(name, case) over shapes x gamma x fix_gamma x offset x eps, then the constant channel.  The split shape
    (0.8 M elements, a fifth of a second of float64 per case) takes offset x fix_gamma in full -- the offset is what
    its statistics path can get wrong -- and walks through the gamma kinds and eps values once: the element rules
    they bear on do not know the shape."""
    rs = np.random.RandomState(20251)
    out = []
    def add(shape, gk, fix, off, eps):
        name = "%s-%s-%s-off%g-eps%g" % ("x".join(map(str, shape)), gk, "fix" if fix else "free", off, eps)
        out.append((name, make_case(rs, shape, gk, fix, off, eps)))
    for shape in SHAPES:
        if shape == SPLIT_SHAPE:
            for k, (off, fix) in enumerate((off, fix) for off in OFFSETS for fix in (True, False)):
                add(shape, GAMMAS[k % 3], fix, off, EPSS[k % 2])
            continue
        for gk in GAMMAS:
            for fix in (True, False):
                for off in OFFSETS:
                    for eps in EPSS:
                        add(shape, gk, fix, off, eps)
    out.append(("constant", constant_case()))
    return out


def evaluate(c, W=1):
    """truths, T and the reference restatement's k per output for one case over W ranks.  The backward of both the
    restatement and the truth is given the float32 roundings of the TRUE mean / var.  -> truth, T, k_ref, mean32, var32"""
    ft, fT = fwd_truth(c["x"], c["gamma"], c["beta"], c["eps"], c["fix_gamma"], W)
    mean32, var32 = ft["mean"].astype(F), ft["var"].astype(F)
    bt, bT = bwd_truth(c["dy"], c["x"], mean32, var32, c["gamma"], c["eps"], c["fix_gamma"], W)
    f32 = fwd_ref32(c["x"], c["gamma"], c["beta"], c["eps"], c["fix_gamma"], W)
    b32 = bwd_ref32(c["dy"], c["x"], mean32, var32, c["gamma"], c["eps"], c["fix_gamma"], W)
    truth, T, ref = dict(ft, **bt), dict(fT, **bT), dict(f32, **b32)
    k_ref = {o: k_of(ref[o], truth[o], T[o]) for o in OUTPUTS}
    return truth, T, k_ref, mean32, var32
