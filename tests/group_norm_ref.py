"""Two restatements of the reference's GroupNorm (operator_cxx/contrib/group_norm.cu:71-298,
group_norm_helper.cu:36-63,258-268); numpy only.  The reference has no CPU implementation of the operator
(group_norm.cc:60 constructs the GPU class only), so it is pinned the way FocalLoss is (tests/focal_ref.py).

  fwd_truth / bwd_truth   float64, from the float32 inputs.  The backward takes mu and rsig as float32 INPUTS,
                          as the operator does.  Each also returns, per output element, T = the sum of the
                          absolute values of the terms of the float64 expression, so that an error reads
                              k = |got - truth| / (eps32 * T + tiny)                                  (k_of)
  fwd_f32 / bwd_f32       the reference's own expressions in float32, in its order of operations per element:
                          mu = sum(x) * (1 / n), var = sum(x * x) * (1 / n) - mu * mu  (E[x^2] - mu^2, which
                          cancels when |mu| >> sigma), rsig = 1 / sqrt(var + eps) (for rsqrtf), and the three
                          backward kernels.  REDUCTIONS are numpy's float32 sums (pairwise): the order of the
                          CUDA block reduction (a strided serial sum per thread, then cub::BlockReduce) cannot be
                          restated on the host, and it is not part of what the operator promises.

T per output (x, dy, gamma, beta, mu, rsig stand for their absolute values; n = D * HxW):
  mu      sum x / n
  rsig    rsig           (every term of the variance about the mean is positive: no cancellation to account for)
  y       gamma * (x + sum x / n) * rsig + beta       (mu is itself a sum: its terms x_j / n are terms of y, and
          their absolute values add up to sum |x| / n, not to |mu| -- with |mu| an element whose x and mu both lie
          near 0 would be held to an error far below the rounding of the group's mean)
  dx      gamma * dy * rsig + ((Tdb * mu + Tds) * (x + mu) * rsig^3 + Tdb * rsig) / n,
          Tds = sum gamma * dy * x, Tdb = sum gamma * dy over the group
  dgamma  sum dy * (x + mu) * rsig        dbeta   sum dy
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
F = np.float32


def _grp(a, N, G):
    return a.reshape(N, G, -1)


def _chan(v, x):
    """(C,) -> broadcastable against x (N, C, ...)"""
    return v.reshape((1, -1) + (1,) * (x.ndim - 2))


def fwd_truth(x, gamma, beta, G, eps):
    """-> dict(y, mu, rsig) float64 and dict of T"""
    x = np.asarray(x, F)
    N, C = x.shape[:2]
    x64 = x.astype(np.float64)
    xg = _grp(x64, N, G)
    mu = xg.mean(axis=2)
    var = ((xg - mu[..., None]) ** 2).mean(axis=2)
    rsig = 1.0 / np.sqrt(var + float(F(eps)))
    g, b = _chan(np.asarray(gamma, F).astype(np.float64), x), _chan(np.asarray(beta, F).astype(np.float64), x)
    mub = np.broadcast_to(mu[..., None], xg.shape).reshape(x.shape)
    rsb = np.broadcast_to(rsig[..., None], xg.shape).reshape(x.shape)
    y = g * (x64 - mub) * rsb + b
    Tmu = np.abs(xg).mean(axis=2)
    Tmub = np.broadcast_to(Tmu[..., None], xg.shape).reshape(x.shape)
    T = dict(mu=Tmu, rsig=rsig, y=np.abs(g) * (np.abs(x64) + Tmub) * rsb + np.abs(b))
    return dict(y=y, mu=mu, rsig=rsig), T


def fwd_f32(x, gamma, beta, G, eps):
    """Moments (group_norm_helper.cu:36-63), InvStd (:258-268), GroupNormForwardCUDAKernel (group_norm.cu:71-91)"""
    x = np.asarray(x, F)
    N, C = x.shape[:2]
    xg = _grp(x, N, G)
    scale = F(1.0) / F(xg.shape[2])
    mu = (xg.sum(axis=2, dtype=F) * scale).astype(F)
    with np.errstate(invalid="ignore", divide="ignore"):
        var = ((xg * xg).sum(axis=2, dtype=F) * scale - mu * mu).astype(F)
        rsig = (F(1.0) / np.sqrt(var + F(eps))).astype(F)
    g, b = _chan(np.asarray(gamma, F), x), _chan(np.asarray(beta, F), x)
    mub = np.broadcast_to(mu[..., None], xg.shape).reshape(x.shape)
    rsb = np.broadcast_to(rsig[..., None], xg.shape).reshape(x.shape)
    with np.errstate(invalid="ignore"):
        y = (g * (x - mub) * rsb + b).astype(F)
    return dict(y=y, mu=mu, rsig=rsig)


def bwd_truth(dy, x, mu, rsig, gamma, G):
    """mu, rsig: the float32 (N, G) arrays the operator is given -> dict(dx, dgamma, dbeta) float64, dict of T"""
    x = np.asarray(x, F)
    N, C = x.shape[:2]
    x64, dy64 = x.astype(np.float64), np.asarray(dy, F).astype(np.float64)
    g = _chan(np.asarray(gamma, F).astype(np.float64), x)
    mu64, rs64 = np.asarray(mu, F).astype(np.float64).reshape(N, G), np.asarray(rsig, F).astype(np.float64).reshape(N, G)
    xg = _grp(x64, N, G)
    n = xg.shape[2]
    gdy = g * dy64
    ds = _grp(gdy * x64, N, G).sum(axis=2)
    db = _grp(gdy, N, G).sum(axis=2)
    Tds = _grp(np.abs(gdy * x64), N, G).sum(axis=2)
    Tdb = _grp(np.abs(gdy), N, G).sum(axis=2)

    def full(v):
        return np.broadcast_to(v[..., None], xg.shape).reshape(x.shape)
    mub, rsb = full(mu64), full(rs64)
    dx = gdy * rsb + ((full(db) * mub - full(ds)) * (x64 - mub) * rsb ** 3 - full(db) * rsb) / n
    Tdx = np.abs(gdy) * rsb + ((full(Tdb) * np.abs(mub) + full(Tds)) * (np.abs(x64) + np.abs(mub)) * rsb ** 3
                               + full(Tdb) * rsb) / n
    red = (0,) + tuple(range(2, x.ndim))
    dgamma = (dy64 * (x64 - mub) * rsb).sum(axis=red)
    Tdg = (np.abs(dy64) * (np.abs(x64) + np.abs(mub)) * rsb).sum(axis=red)
    dbeta = dy64.sum(axis=red)
    Tdb_ = np.abs(dy64).sum(axis=red)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta), dict(dx=Tdx, dgamma=Tdg, dbeta=Tdb_)


def bwd_f32(dy, x, mu, rsig, gamma, G):
    """ComputeInternalGradients (group_norm.cu:93-126), GroupNormBackward (:139-163), GammaBetaBackward (:165-196)"""
    x, dy = np.asarray(x, F), np.asarray(dy, F)
    N, C = x.shape[:2]
    g = _chan(np.asarray(gamma, F), x)
    mu, rsig = np.asarray(mu, F).reshape(N, G), np.asarray(rsig, F).reshape(N, G)
    xg = _grp(x, N, G)
    ds = _grp(g * dy * x, N, G).sum(axis=2, dtype=F)
    db = _grp(g * dy, N, G).sum(axis=2, dtype=F)
    denom = F(1.0) / F(xg.shape[2])

    def full(v):
        return np.broadcast_to(v[..., None], xg.shape).reshape(x.shape)
    mub, rsb, dsb, dbb = full(mu), full(rsig), full(ds), full(db)
    u = (dbb * mub - dsb) * (x - mub) * (rsb * rsb * rsb)
    v = dbb * rsb
    dx = (g * dy * rsb + (u - v) * denom).astype(F)
    # one channel at a time, the batch and the plane as one float32 sum (the reference's inner_size = N * HxW)
    per = (dy * (x - mub) * rsb).astype(F)
    dgamma = np.stack([per[:, c].reshape(-1).sum(dtype=F) for c in range(C)]).astype(F)
    dbeta = np.stack([dy[:, c].reshape(-1).sum(dtype=F) for c in range(C)]).astype(F)
    return dict(dx=dx, dgamma=dgamma, dbeta=dbeta)


def k_of(got, truth, T):
    """max over the elements of |got - truth| / (eps32 * T + tiny); where T is 0 the value must be the truth.
    A non-finite `got` gives inf."""
    got = np.asarray(got, np.float64).reshape(np.shape(truth))
    den = EPS32 * np.asarray(T, np.float64) + TINY32
    with np.errstate(invalid="ignore"):
        err = np.abs(got - truth)
    err = np.where(np.isfinite(got), err, np.inf)
    k = err / den
    return float(k.max()) if k.size else 0.0


# ------------------------------------------------------------------------------------------ cases --
SHAPES = (
    ("head7x7", (8, 64, 7, 7), 32),        # small groups, odd plane: a wave per group, scalar
    ("head14x14", (4, 32, 14, 14), 8),     # small groups, 16-byte items
    ("odd5x9", (2, 16, 5, 9), 4),          # odd HxW
    ("block24x24", (2, 32, 24, 24), 4),    # 4608 floats per group: a workgroup per group
    ("split100x168", (2, 64, 100, 168), 32),   # 33 600 floats per group: split over workgroups
    ("g1", (2, 64, 7, 7), 1),              # G = 1: 3136 floats per group, 64 short rows
    ("gC", (2, 16, 8, 8), 16),             # G = C
)
GAMMAS = ("ones", "random", "zeros")
OFFSETS = (0.0, 3.0, 100.0)
EPSS = (1e-5, 1e-3)


def make_gamma(rs, C, kind):
    if kind == "ones":
        return np.ones(C, F)
    g = (rs.standard_normal(C) * 0.5 + 1.0).astype(F)
    if kind == "zeros":
        g[::3] = 0.0
    return g


def make_case(rs, shape, G, gamma_kind, offset, eps):
    N, C = shape[:2]
    x = rs.standard_normal(shape).astype(np.float64)
    # per-group offset of the mean, in standard deviations (sigma = 1), alternating in sign over the groups
    off = offset * np.where(np.arange(N * G) % 2 == 0, 1.0, -1.0).reshape(N, G, 1)
    x = (x.reshape(N, G, -1) + off).reshape(shape).astype(F)
    return dict(x=x, gamma=make_gamma(rs, C, gamma_kind), beta=rs.standard_normal(C).astype(F),
                dy=rs.standard_normal(shape).astype(F), G=G, eps=eps, offset=offset)


def constant_case():
    """group (0, 1) is the constant 1.5 over 128 elements: every sum the reference or the device forms is exact,
    the variance is exactly 0 and rsig = 1 / sqrt(eps) in both"""
    rs = np.random.RandomState(77)
    c = make_case(rs, (2, 16, 4, 8), 4, "random", 0.0, 1e-5)
    c["x"][0, 4:8] = 1.5
    return c


def cases():
    """(name, dict(x, gamma, beta, dy, G, eps, offset)) over shapes x gamma x offset x eps, then the constant group"""
    rs = np.random.RandomState(20250)
    out = []
    for sname, shape, G in SHAPES:
        for gk in GAMMAS:
            for off in OFFSETS:
                for eps in EPSS:
                    out.append(("%s-%s-off%g-eps%g" % (sname, gk, off, eps), make_case(rs, shape, G, gk, off, eps)))
    out.append(("constant", constant_case()))
    return out


def evaluate(c):
    """truths, T and the restatement's k per output for one case.  The backward of both the restatement and the
    code under test is given the float32 roundings of the TRUE mu / rsig."""
    ft, fT = fwd_truth(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
    mu32, rs32 = ft["mu"].astype(F), ft["rsig"].astype(F)
    bt, bT = bwd_truth(c["dy"], c["x"], mu32, rs32, c["gamma"], c["G"])
    f32 = fwd_f32(c["x"], c["gamma"], c["beta"], c["G"], c["eps"])
    b32 = bwd_f32(c["dy"], c["x"], mu32, rs32, c["gamma"], c["G"])
    truth, T = dict(ft, **bt), dict(fT, **bT)
    k_ref = {o: k_of(dict(f32, **b32)[o], truth[o], T[o]) for o in OUTPUTS}
    return truth, T, k_ref, mu32, rs32


OUTPUTS = ("y", "mu", "rsig", "dx", "dgamma", "dbeta")
