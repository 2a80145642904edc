"""Two restatements of the reference's SigmoidCrossEntropy (operator_cxx/contrib/sigmoid_cross_entropy.cu:44-122,
-inl.h:68-119); numpy only.  The reference has no CPU implementation of the operator
(sigmoid_cross_entropy.cc:40,50 are LOG(FATAL)), so it is pinned the way FocalLoss and GroupNorm are
(tests/focal_ref.py, tests/group_norm_ref.py).

  truth(x, t, scale)   float64, from the float32 inputs; an element whose target is -1 gives 0 everywhere:
                           loss = max(x, 0) - x * t + log1p(exp(-|x|))
                           out  = sum loss / count_sum,  count_sum = float32(count) + float32(1e-5) (exact by rule)
                           d    = (sigmoid(x) - t) * scale / count_sum
                       and, per output, T = the sum of the absolute values of the terms, so that an error reads
                           k = |got - truth| / (eps32 * T + tiny)                                        (k_of)
                           loss      |x * (t - [x >= 0])| + log1p(exp(-|x|))
                           loss_sum  sum T_loss         out   sum T_loss / count_sum
                           d         (sigmoid(x) + |t|) * scale / count_sum
  f32(x, t, scale)     the reference's own expressions in its order of operations, with the promotions its double
                       literals `-1.`, `1.` and `1. /` cause (evaluated in double, rounded to float32 once); expf
                       and logf are numpy's float32 exp and log.  ROW SUMS are numpy's float32 sums: the order of
                       mshadow's reduction cannot be restated on the host and is not part of what the operator
                       promises.  The gradient is divided by count_sum and then multiplied by scale: two float32
                       roundings, as the reference's two passes.
"""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
F = np.float32
OUTPUTS = ("loss", "loss_sum", "out", "d")


def count_sum_f32(t):
    """(n,) float32: float32(number of targets != -1) + float32(1e-5), per row"""
    t = np.asarray(t, F)
    return (np.sum(t != F(-1), axis=1).astype(F) + F(1e-5)).astype(F)


def _sigmoid64(x):
    with np.errstate(over="ignore"):
        return np.where(x >= 0, 1.0 / (1.0 + np.exp(-np.abs(x))), np.exp(-np.abs(x)) / (1.0 + np.exp(-np.abs(x))))


def truth(x, t, scale):
    """x, t (n, k) float32 -> (dict of float64 truths, dict of T)"""
    x = np.asarray(x, F).astype(np.float64)
    t = np.asarray(t, F).astype(np.float64)
    on = t != -1.0
    xs = np.where(on, x, 0.0)              # an ignored logit is not looked at (NaN and inf included)
    cs = count_sum_f32(t).astype(np.float64)
    soft = np.log1p(np.exp(-np.abs(xs)))
    loss = np.where(on, np.maximum(xs, 0.0) - xs * t + soft, 0.0)
    Tl = np.where(on, np.abs(xs * (t - (xs >= 0))) + soft, 0.0)
    sig = _sigmoid64(xs)
    d = np.where(on, (sig - t) * scale / cs[:, None], 0.0)
    Td = np.where(on, (sig + np.abs(t)) * abs(scale) / cs[:, None], 0.0)
    out = dict(loss=loss, loss_sum=loss.sum(axis=1), out=loss.sum(axis=1) / cs, d=d)
    T = dict(loss=Tl, loss_sum=Tl.sum(axis=1), out=Tl.sum(axis=1) / cs, d=Td)
    return out, T


def f32(x, t, scale):
    """the reference's arithmetic -> dict(loss, count, loss_sum, count_sum, out, d) float32"""
    x = np.asarray(x, F)
    t = np.asarray(t, F)
    on = t != F(-1)
    xs = np.where(on, x, F(0))
    with np.errstate(over="ignore", invalid="ignore"):
        ge = (xs >= 0).astype(F)
        # -1. * x * (t - (x >= 0)) + logf(1 + expf(x - 2 * x * (x >= 0))): the product and the sum are double
        z = (xs - (F(2) * xs) * ge).astype(F)
        lg = np.log((F(1) + np.exp(z, dtype=F)).astype(F), dtype=F)
        loss = ((-1.0 * xs.astype(np.float64)) * (t - ge).astype(F).astype(np.float64) + lg.astype(np.float64)).astype(F)
        # 1. / (1. + expf(-x)) - t: all in double after the expf
        g = (1.0 / (1.0 + np.exp(-xs, dtype=F).astype(np.float64)) - t.astype(np.float64)).astype(F)
    loss = np.where(on, loss, F(0)).astype(F)
    count = on.astype(F)
    loss_sum = loss.sum(axis=1, dtype=F)
    cs = (count.sum(axis=1, dtype=F) + F(1e-5)).astype(F)
    with np.errstate(invalid="ignore", over="ignore"):
        out = (loss_sum / cs).astype(F)
        d = ((g / cs[:, None]).astype(F) * F(scale)).astype(F)
    d = np.where(on, d, F(0)).astype(F)
    return dict(loss=loss, count=count, loss_sum=loss_sum, count_sum=cs, out=out, d=d)


def k_of(got, truth_, T):
    """max over the elements of |got - truth| / (eps32 * T + tiny); where T is 0 the value must be the truth.
    A non-finite `got` gives inf."""
    got = np.asarray(got, np.float64).reshape(np.shape(truth_))
    den = EPS32 * np.asarray(T, np.float64) + TINY32
    with np.errstate(invalid="ignore"):
        err = np.abs(got - truth_)
    err = np.where(np.isfinite(got), err, np.inf)
    k = err / den
    return float(k.max()) if k.size else 0.0


def k_ref(x, t, scale):
    """the float32 restatement's own k per output"""
    tr, T = truth(x, t, scale)
    r = f32(x, t, scale)
    return {o: k_of(r[o], tr[o], T[o]) for o in OUTPUTS}


# ------------------------------------------------------------------------------------------ cases --
PLANTED = (0.0, -0.0, 20.0, -20.0, 90.0, -90.0, 104.0, -104.0)   # +-90 / +-104: expf overflows in the gradient and
#                                                                   underflows in the loss


def make_logits(rs, shape):
    x = (rs.standard_normal(shape) * 3.0).astype(F)
    flat = x.reshape(-1)
    m = min(flat.size, 2 * len(PLANTED))
    flat[:m] = (PLANTED + PLANTED)[:m]
    return x


def make_targets(rs, shape, kind):
    """kind: 'mix' (10 % ignored), 'ignore30', 'row' (one whole row is -1), 'soft' (0.25 and 0.5 among the targets)"""
    n = int(np.prod(shape))
    p_ign = 0.3 if kind == "ignore30" else 0.1
    vals = [-1.0, 0.0, 1.0] if kind != "soft" else [-1.0, 0.0, 1.0, 0.25, 0.5]
    rest = (1.0 - p_ign) / (len(vals) - 1)
    t = rs.choice(vals, size=n, p=[p_ign] + [rest] * (len(vals) - 1)).astype(F)
    m = min(n, 2 * len(PLANTED))
    t[:m] = ([0.0] * len(PLANTED) + [1.0] * len(PLANTED))[:m]     # every planted logit is counted, with both targets
    t = t.reshape(shape)
    if kind == "row":
        t[shape[0] // 2] = -1.0
    return t


# (name, (n, k), target kind, grad_scale)
DROPIN = (
    ("long-odd", (1, 70001), "mix", 1.0),
    ("long-odd-ign30", (1, 70001), "ignore30", 128.0),
    ("workload", (1, 200704), "mix", 128.0),
    ("short-rows", (300, 7), "mix", 1.0),
    ("short-rows-row", (300, 7), "row", 128.0),
    ("k1", (3, 1), "mix", 1.0),
    ("k1-row", (3, 1), "row", 1.0),
    ("rows4096", (5, 4096), "mix", 1.0),
    ("rows4096-soft", (5, 4096), "soft", 128.0),
    ("rows1023", (2, 1023), "mix", 128.0),
    ("rows1023-row", (2, 1023), "row", 1.0),
)


def dropin_cases():
    rs = np.random.RandomState(2718)
    return [(name, dict(x=make_logits(rs, shape), t=make_targets(rs, shape, kind), scale=scale))
            for name, shape, kind, scale in DROPIN]


# (name, (R, K, P), cls, grad_scale); cls holds 0, K - 1, 2.7 (truncated to 2) and the rejected -1, K, 1e9, NaN
NAN = float("nan")
FUSED = (
    ("r5k3p49", (5, 3, 49), [0, 2, 2.7, -1, NAN], 1.0),
    ("head", (8, 81, 784), [0, 80, 2.7, 17, -1, 81, 1e9, NAN], 128.0),
    ("agnostic", (7, 1, 196), [0, 0, 0.5, -1, 1, 1e9, NAN], 1.0),
    ("oddplane", (4, 5, 15), [2.7, 4, 5, 0], 128.0),
    ("p1", (33, 2, 1), [0, 1, -1, 2, 1e9, NAN, 1.9] + [0, 1] * 13, 1.0),
)


def fused_cases():
    rs = np.random.RandomState(3141)
    out = []
    for name, (R, K, P), cls, scale in FUSED:
        assert len(cls) == R
        out.append((name, dict(logits=make_logits(rs, (R, K, P)), cls=np.asarray(cls, F),
                               target=make_targets(rs, (R, P), "mix"), scale=scale)))
    return out


def gather(logits, cls, target):
    """the (1, R*P) row the fused op is equivalent to: plane int(cls[r]) of every RoI; a RoI whose cls is NaN,
    negative or >= K contributes zeros with targets -1 (fully ignored).  Also returns the per-RoI plane (-1: none)."""
    R, K, P = logits.shape
    with np.errstate(invalid="ignore"):
        ok = (cls >= 0) & (cls < K)
    plane = np.where(ok, np.where(ok, cls, 0).astype(np.int64), -1)
    x = np.zeros((R, P), F)
    t = np.full((R, P), -1.0, F)
    for r in range(R):
        if plane[r] >= 0:
            x[r] = logits[r, plane[r]]
            t[r] = target[r]
    return x.reshape(1, -1), t.reshape(1, -1), plane
