"""Two restatements of the reference's FocalLoss backward (operator_cxx/contrib/focal_loss-inl.h:186-230),
its forward (:113) and BBoxNorm's backward (operator_cxx/contrib/bbox_norm-inl.h:116-126).

  *_f32     float32 numpy, operation for operation in the reference's order, host libm (numpy's logf / powf
            / expf).  This is what the reference computes up to its own transcendentals.
  *_truth   the ARGUMENTS of log and pow are formed in float32 exactly as the reference forms them
            (out + eps, 1 - out, (1 - out) + eps); the functions and everything after them in float64.
            Also returns, per element, T = the sum of the absolute values of the terms of the branch taken
            and s = the scale applied after the branch, so that an error can be expressed as
                k = |got - truth| / (eps32 * T * s + tiny),   tiny = s * (smallest normal float32).
"""
import numpy as np

EPS = np.float32(1e-14)          # ScalarExp<float>(1e-14), :185
EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
NORMALIZATION = ("null", "batch", "valid")


def label_count(label):
    """#(label >= 1) over the batch: F<le>(1.f, label) summed (:218-219)"""
    return int((np.float32(1.0) <= np.asarray(label, np.float32)).sum())


def one_hot_mask(label, nclass):
    """(B, nbox, nclass) bool: class c == int(label - 1), truncated toward zero, only inside [0, nclass)
    (label_tmp = label - 1, then mxnet_op::one_hot's static_cast<int>, :198-201)"""
    idx = np.trunc(np.asarray(label, np.float32) - np.float32(1.0)).astype(np.int64)
    return idx[..., None] == np.arange(nclass)[None, None, :]


def sigmoid_f32(x):
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore"):
        return (np.float32(1.0) / (np.float32(1.0) + np.exp(-x))).astype(np.float32)


def sigmoid_truth(x):
    x = np.asarray(x, np.float32).astype(np.float64)
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def _scale_f32(g, label, B, grad_scale, normalization):
    gs = np.float32(grad_scale)
    if normalization == "valid":
        norm = np.float32(label_count(label)) + np.float32(1.0)      # no max (:220-221)
        return ((g * gs) / norm).astype(np.float32)
    if normalization == "batch":
        return (g * (gs / np.float32(B))).astype(np.float32)
    return (g * gs).astype(np.float32)


def focal_bwd_f32(out, label, ograd, alpha, gamma, grad_scale, normalization):
    out = np.asarray(out, np.float32)
    label = np.asarray(label, np.float32)
    B, nbox, nclass = out.shape
    one, a, g_ = np.float32(1.0), np.float32(alpha), np.float32(gamma)
    with np.errstate(divide="ignore", invalid="ignore"):
        positive = a * np.power(one - out, g_) * (g_ * out * np.log(out + EPS) + out - one)
        negative = -((one - a) * np.power(out, g_) * (g_ * (one - out) * np.log(one - out + EPS) - out))
    grad = np.where(one_hot_mask(label, nclass), positive, negative).astype(np.float32)
    grad = np.where((label == np.float32(-1.0))[..., None], np.float32(0.0), grad)
    if ograd is not None:
        grad = grad * np.asarray(ograd, np.float32)
    return _scale_f32(grad.astype(np.float32), label, B, grad_scale, normalization)


def focal_bwd_truth(out, label, ograd, alpha, gamma, grad_scale, normalization):
    """-> (truth float64, T float64, s float64, branch int8: +1 positive, -1 negative, 0 ignored row)"""
    out = np.asarray(out, np.float32)
    label = np.asarray(label, np.float32)
    B, nbox, nclass = out.shape
    one = np.float32(1.0)
    a, oma, g_ = float(np.float32(alpha)), float(one - np.float32(alpha)), float(np.float32(gamma))
    p = out.astype(np.float64)
    omp = (one - out).astype(np.float64)                     # float32 arguments, as the reference forms them
    lp = np.log((out + EPS).astype(np.float64))
    lq = np.log(((one - out) + EPS).astype(np.float64))
    with np.errstate(invalid="ignore"):
        pw_pos, pw_neg = np.power(omp, g_), np.power(p, g_)
    positive = a * pw_pos * (g_ * p * lp + p - 1.0)
    negative = -(oma * pw_neg * (g_ * omp * lq - p))
    t_pos = a * pw_pos * (g_ * p * np.abs(lp) + p + 1.0)
    t_neg = oma * pw_neg * (g_ * omp * np.abs(lq) + p)
    hot = one_hot_mask(label, nclass)
    ign = (label == np.float32(-1.0))[..., None]
    truth = np.where(ign, 0.0, np.where(hot, positive, negative))
    T = np.where(ign, 0.0, np.where(hot, t_pos, t_neg))
    branch = np.where(ign, 0, np.where(hot, 1, -1)).astype(np.int8) * np.ones(out.shape, np.int8)
    s = np.full(out.shape, float(np.float32(grad_scale)), np.float64)
    if ograd is not None:
        og = np.asarray(ograd, np.float32).astype(np.float64)
        truth, s = truth * og, s * np.abs(og)
    if normalization == "valid":
        s = s / (label_count(label) + 1.0)
    elif normalization == "batch":
        s = s / B
    sign = float(np.float32(grad_scale))
    norm = (label_count(label) + 1.0) if normalization == "valid" else float(B) if normalization == "batch" else 1.0
    return truth * sign / norm, T, s, branch


def k_of(got, truth, T, s):
    """max over the elements of |got - truth| / (eps32 * T * s + s * tiny); an element whose scale is 0
    (ograd == 0) must be exactly the truth (0)."""
    got = np.asarray(got, np.float64)
    den = EPS32 * T * s + s * TINY32
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))
    return float(k.max()) if k.size else 0.0


def k_sigmoid(got, x):
    t = sigmoid_truth(x)
    return float((np.abs(np.asarray(got, np.float64) - t) / (EPS32 * np.abs(t) + TINY32)).max())


def bbox_norm_bwd_f32(gout, label):
    norm = np.maximum(np.float32(1.0), np.float32(label_count(label)) + np.float32(1.0))
    return (np.asarray(gout, np.float32) / norm).astype(np.float32)


# ------------------------------------------------------------------------------------------ cases --
def logits(rs, shape):
    """N(-4.6, 2^2), the RetinaNet prior (sigmoid(-4.6) = 0.01), with planted saturating, tiny and zero logits"""
    x = (rs.standard_normal(shape) * 2.0 - 4.6).astype(np.float32)
    flat = x.reshape(-1)
    planted = np.float32([30, -30, 100, -100, 1e-4, -1e-4, 0])
    idx = rs.choice(flat.size, size=min(flat.size, 4 * planted.size), replace=False)
    flat[idx] = np.resize(planted, idx.size)
    return x


def labels(rs, B, nbox, nclass, kind):
    """kind: 'mix' {-1, 0, 1..K}, one label above K and two fractional ones; 'nopos' {-1, 0}; 'ignore' all -1"""
    if kind == "ignore":
        return np.full((B, nbox), -1, np.float32)
    lab = rs.choice([-1.0, 0.0], size=(B, nbox), p=[0.1, 0.9]).astype(np.float32)
    if kind == "mix":
        pos = rs.rand(B, nbox) < 0.15
        lab[pos] = rs.randint(1, nclass + 1, int(pos.sum()))
        lab[0, 0], lab[-1, -1], lab[0, nbox // 2] = nclass, 1, nclass + 3      # first, last, above K
        # fractional labels: one_hot is int(label - 1), truncated toward zero: 0.5 -> class 0 (and NOT counted:
        # 0.5 < 1), 1.9 -> class 0 (counted)
        lab[0, 1], lab[-1, 2] = 0.5, 1.9
    return lab


def cases():
    """the issue's sweep: (name, dict(out, label, ograd, alpha, gamma, grad_scale, normalization))"""
    rs = np.random.RandomState(20240)
    out = []
    for nclass, nbox in ((80, 257), (1, 1031), (3, 515)):
        for kind in ("mix", "nopos", "ignore"):
            for gamma in (2.0, 0.0, 1.0, 1.5):
                for alpha in (0.25, 0.5):
                    for normalization in NORMALIZATION:
                        for with_ograd in (False, True):
                            B = 2
                            o = sigmoid_f32(logits(rs, (B, nbox, nclass)))
                            og = None
                            if with_ograd:
                                og = rs.standard_normal(o.shape).astype(np.float32)
                                og[rs.rand(*o.shape) < 0.1] = 0.0
                            name = "K%d-%s-g%g-a%g-%s-%s" % (nclass, kind, gamma, alpha, normalization,
                                                            "ograd" if with_ograd else "noograd")
                            out.append((name, dict(out=o, label=labels(rs, B, nbox, nclass, kind), ograd=og,
                                                   alpha=alpha, gamma=gamma, grad_scale=1.0 if not with_ograd else 0.7,
                                                   normalization=normalization)))
    return out
