"""Restatements of the Mask Scoring R-CNN training head (models/msrcnn/builder.py:143-168, :383-424 and
models/msrcnn/maskiou_compute.py:14-38); numpy only.

  Mask loss      the loss, count_sum and the cross-entropy gradient are tests/sigmoid_ce_ref.py's on the gathered
                 row.  New here: prob = sigmoid of the selected plane and the gradient that arrives through it,
                     d = g_ce + d_prob * (p * (1 - p))
                 mask_f32: float32 in that order, p = 1 / (1 + expf(-x)) (MXNet's Activation(sigmoid); MXNet is not
                 vendored, so the expression is inferred and pinned against the float64 truth, not bit for bit).
                 mask_truth: float64, with T = the sum of the absolute values of the terms, so that an error reads
                     k = |got - truth| / (eps32 * T + tiny)                                    (sigmoid_ce_ref.k_of)
                     prob  T = p
                     d     T = T_ce + |d_prob| * p * (1 + p)     -- (1 - p) is a difference of the terms 1 and p: its
                                                                    rounding error is relative to 1, not to 1 - p
  MaskIoU target maskiou_compute: the numpy types of the reference operator, statement by statement -- bool
                 prediction, float32 products and sums, an int64 count, the target sum promoted to float64 and
                 divided by the float32 ratio, numpy.maximum (a NaN propagates), float32 / float64, rounded to
                 float32 on assignment.  tests/golden/msrcnn_maskiou.npz holds what the reference file itself gave
                 on the golden cases (tests/golden/make_golden_msrcnn.py); test_msrcnn_head.py compares.
  MaskIoU loss   loss_f32: float32 in the device's order of operations; a row whose cls names no column is left out
                     S = sum((t - p)^2 * w),  W = sum w,  loss = 0.5 * S / max(W, 1)
                     d = ((-(t - p)) * w) / max(W, 1) * scale
                 loss_truth: float64 from the float32 iou_target, with
                     loss  T = 0.5 * sum((|t| + |p|)^2 * w) / max(W, 1)
                     d     T = (|t| + |p|) * w / max(W, 1) * |scale|
"""
import numpy as np

from . import sigmoid_ce_ref as sr

F = np.float32
NAN = float("nan")
k_of = sr.k_of


def planes(cls, K):
    """per row: int(cls) when it names a plane / column, -1 otherwise (NaN, negative, >= K)"""
    cls = np.asarray(cls, F).reshape(-1)
    with np.errstate(invalid="ignore"):
        ok = (cls >= 0) & (cls < K)
    return np.where(ok, np.where(ok, cls, 0).astype(np.int64), -1)


# ---------------------------------------------------------------------------------------- mask loss --
def selected(logits, cls):
    """(R, P) selected plane of every row (zeros where the row is rejected) and the planes"""
    R, K, P = logits.shape
    pl = planes(cls, K)
    x = np.zeros((R, P), F)
    for r in range(R):
        if pl[r] >= 0:
            x[r] = logits[r, pl[r]]
    return x, pl


def mask_f32(logits, cls, target, d_prob, scale):
    """float32 restatement -> dict(prob (R, P), d (R, P): the selected plane's gradient)"""
    x, pl = selected(logits, cls)
    gx, gt, _ = sr.gather(logits, np.asarray(cls, F), target)
    g_ce = sr.f32(gx, gt, scale)["d"].reshape(x.shape)
    with np.errstate(over="ignore", invalid="ignore"):
        p = (F(1) / (F(1) + np.exp(-x, dtype=F)).astype(F)).astype(F)
        d = (g_ce + (np.asarray(d_prob, F) * (p * (F(1) - p)).astype(F)).astype(F)).astype(F)
    ok = (pl >= 0)[:, None]
    return dict(prob=np.where(ok, p, F(0)).astype(F), d=np.where(ok, d, F(0)).astype(F))


def mask_truth(logits, cls, target, d_prob, scale):
    """float64 truth -> (dict(prob, d), dict of T)"""
    x, pl = selected(logits, cls)
    gx, gt, _ = sr.gather(logits, np.asarray(cls, F), target)
    tr, T = sr.truth(gx, gt, scale)
    ok = (pl >= 0)[:, None]
    p = np.where(ok, sr._sigmoid64(x.astype(np.float64)), 0.0)
    dp = np.where(ok, np.asarray(d_prob, F).astype(np.float64), 0.0)
    d = tr["d"].reshape(x.shape) + dp * p * (1.0 - p)
    Td = T["d"].reshape(x.shape) + np.abs(dp) * p * (1.0 + p)
    return dict(prob=p, d=d), dict(prob=p, d=Td)


def mask_k_ref(logits, cls, target, d_prob, scale):
    tr, T = mask_truth(logits, cls, target, d_prob, scale)
    r = mask_f32(logits, cls, target, d_prob, scale)
    return {o: k_of(r[o], tr[o], T[o]) for o in ("prob", "d")}


# ----------------------------------------------------------------------------------- MaskIoU target --
def maskiou_compute(prob, target, ratio, cls):
    """the reference operator's forward on host arrays: prob / target (R, ...), ratio and cls R floats ->
    (iou_target (R,) float32, weight (R,) float32)"""
    prob = np.asarray(prob, F)
    R = prob.shape[0]
    prob = prob.reshape(R, 1, -1)
    target = np.asarray(target, F).reshape(R, 1, -1)
    ratio = np.asarray(ratio, F).reshape(-1)
    cls = np.asarray(cls, F).reshape(-1)
    pred = np.array(prob > 0.5, dtype=bool)
    with np.errstate(all="ignore"):
        inter = target * pred                                   # float32
        pred_sum = np.sum(pred, axis=(1, 2))                    # int64
        inter_sum = np.sum(inter, axis=(1, 2))                  # float32
        target_sum = np.sum(target, axis=(1, 2)).astype(float)  # float64
        target_sum /= ratio
        union = np.maximum(target_sum + pred_sum - inter_sum, 1)
        inter_sum = np.maximum(inter_sum, 0)
        iou = (inter_sum / union).astype(F)                     # assignment to the float32 output
        weight = np.zeros_like(cls)
        weight[np.where(cls > 0)[0]] = 1
    return iou, weight


# ------------------------------------------------------------------------------------- MaskIoU loss --
def _picked(iou_pred, cls):
    R, K = iou_pred.shape
    pl = planes(cls, K)
    p = np.zeros(R, F)
    p[pl >= 0] = iou_pred[np.arange(R)[pl >= 0], pl[pl >= 0]]
    return p, pl


def loss_f32(iou_pred, cls, iou_target, weight, scale=1.0):
    """float32 -> dict(loss, weight_sum, d (R, K))"""
    iou_pred = np.asarray(iou_pred, F)
    p, pl = _picked(iou_pred, cls)
    ok = pl >= 0
    t, w = np.asarray(iou_target, F), np.where(ok, np.asarray(weight, F), F(0)).astype(F)
    with np.errstate(all="ignore"):
        diff = (t - p).astype(F)
        s = np.where(ok, ((diff * diff).astype(F) * w).astype(F), F(0)).astype(F)
        S, W = s.sum(dtype=F), w.sum(dtype=F)
        den = max(W, F(1))
        loss = F(F(F(0.5) * S) / den)
        dsel = (((-diff * w).astype(F) / den).astype(F) * F(scale)).astype(F)
    d = np.zeros(iou_pred.shape, F)
    d[np.arange(len(pl))[ok], pl[ok]] = dsel[ok]
    return dict(loss=loss, weight_sum=W, d=d)


def loss_truth(iou_pred, cls, iou_target, weight, scale=1.0):
    """float64 -> (dict(loss, d (R, K)), dict of T)"""
    iou_pred = np.asarray(iou_pred, F)
    p, pl = _picked(iou_pred, cls)
    ok = pl >= 0
    p = p.astype(np.float64)
    t = np.asarray(iou_target, F).astype(np.float64)
    w = np.where(ok, np.asarray(weight, F), 0).astype(np.float64)
    with np.errstate(all="ignore"):
        den = max(w.sum(), 1.0)
        loss = 0.5 * np.where(ok, (t - p) ** 2 * w, 0.0).sum() / den
        Tl = 0.5 * np.where(ok, (np.abs(t) + np.abs(p)) ** 2 * w, 0.0).sum() / den
        dsel = -(t - p) * w / den * scale
        Tsel = (np.abs(t) + np.abs(p)) * w / den * abs(scale)
    d, Td = np.zeros(iou_pred.shape), np.zeros(iou_pred.shape)
    d[np.arange(len(pl))[ok], pl[ok]] = dsel[ok]
    Td[np.arange(len(pl))[ok], pl[ok]] = Tsel[ok]
    return dict(loss=loss, d=d), dict(loss=Tl, d=Td)


def loss_k_ref(iou_pred, cls, iou_target, weight, scale=1.0):
    tr, T = loss_truth(iou_pred, cls, iou_target, weight, scale)
    r = loss_f32(iou_pred, cls, iou_target, weight, scale)
    return {o: k_of(r[o], tr[o], T[o]) for o in ("loss", "d")}


# ------------------------------------------------------------------------------------------ cases --
RS = (1, 3, 5)
K = 3
PS = (8, 9, 63, 64, 65, 257, 784)     # scalar path, the wave (64) and chunk (256) boundaries of the popcount, 28 x 28
VARIANTS = (0, 1)
# what row r of variant v is: RECIPES[(5 * v + r) % 10]
RECIPES = ("plain", "target-1", "ratio0-bg", "nan-row", "cls-K", "logit0", "all-predicted", "empty-0over0",
           "nan-logit-ignored", "empty-valid")


def make_case(R, P, variant, seed=0):
    """dict(logits (R, K, P), cls, target (R, P), ratio, iou_pred (R, K), d_prob (R, P), scale, recipes)"""
    rs = np.random.RandomState(1000 * R + 10 * P + variant + seed)
    logits = sr.make_logits(rs, (R, K, P))
    target = rs.choice([-1.0, 0.0, 1.0], size=(R, P), p=[0.1, 0.45, 0.45]).astype(F)
    ratio = rs.uniform(0.2, 1.0, R).astype(F)
    cls = rs.randint(1, K, R).astype(F)
    iou_pred = rs.standard_normal((R, K)).astype(F)
    d_prob = rs.standard_normal((R, P)).astype(F)
    names = []
    for r in range(R):
        what = RECIPES[(5 * variant + r) % 10]
        names.append(what)
        if what == "plain":
            cls[r] = 1.5                      # truncated to 1
        elif what == "target-1":
            target[r] = -1.0
            cls[r] = 2
        elif what == "ratio0-bg":
            ratio[r] = 0.0
            cls[r] = 0                        # background: weight 0, column 0
            target[r] = np.abs(target[r])
            target[r, 0] = 1.0                # T > 0: the union is +inf
        elif what == "nan-row":
            cls[r] = NAN
            logits[r] = NAN                   # an ignored row's logits are not read
            ratio[r] = NAN
            d_prob[r] = NAN                   # ... nor its d_prob
        elif what == "cls-K":
            cls[r] = K
            target[r] = 0.0
            ratio[r] = 0.5
        elif what == "logit0":
            cls[r] = 1
            logits[r, 1] = 0.0                # prob == 0.5 exactly: not predicted
            logits[r, 1, ::2] = -0.0
        elif what == "all-predicted":
            cls[r] = 2
            logits[r, 2] = np.abs(logits[r, 2]) + F(0.25)
            target[r] = 1.0
            ratio[r] = 1.0
        elif what == "empty-0over0":
            cls[r] = -1
            target[r] = 0.0
            ratio[r] = 0.0                    # 0 / 0: a NaN target in a row that reaches neither S nor W
        elif what == "nan-logit-ignored":
            cls[r] = -1
            logits[r, 1, P // 2] = NAN
        elif what == "empty-valid":
            cls[r] = 2
            target[r] = 0.0
            logits[r, 2] = -np.abs(logits[r, 2]) - F(0.25)     # nothing predicted: union max(0, 1) = 1
    return dict(logits=logits, cls=cls, target=target, ratio=ratio, iou_pred=iou_pred, d_prob=d_prob,
                scale=128.0 if variant else 1.0, recipes=names)


def golden_cases():
    """inputs of the golden file: (name, prob (R, h, w), target (R, h, w), ratio (R,), cls (R,)).  prob is the
    float32 sigmoid of random logits with 0.5 (not predicted), 1 and 0 planted; the rows cover a zero ratio with a
    positive and with an empty target, a NaN ratio, a row of -1, an empty and a full prediction."""
    out = []
    for name, (R, h, w) in (("r6-4x4", (6, 4, 4)), ("r7-3x5", (7, 3, 5)), ("r9-28x28", (9, 28, 28))):
        rs = np.random.RandomState(R * 100 + h)
        x = (rs.standard_normal((R, h, w)) * 3).astype(F)
        prob = (F(1) / (F(1) + np.exp(-x, dtype=F))).astype(F)
        prob.reshape(R, -1)[:, :3] = (0.5, 1.0, 0.0)
        target = rs.choice([-1.0, 0.0, 1.0], size=(R, h, w), p=[0.1, 0.45, 0.45]).astype(F)
        ratio = rs.uniform(0.2, 1.0, R).astype(F)
        cls = rs.randint(0, 4, R).astype(F)
        ratio[0] = 0.0
        target[0, 0, 0] = 1.0
        ratio[1] = 0.0
        target[1] = 0.0
        ratio[2] = NAN
        target[3] = -1.0
        prob[4] = 0.25
        prob[5] = 0.75
        target[5] = 1.0
        cls[:4] = (0, -1, NAN, 3)
        out.append((name, prob, target, ratio, cls))
    return out
