"""Restatement of the Faster / Mask R-CNN loss heads; numpy only.

The reference's graphs (symbol/builder.py:163-206, 405-446, models/FPN/builder.py:156-237) call upstream's
SoftmaxOutput, smooth_l1 and MakeLoss, whose sources are NOT vendored with the reference.  What is written here is
the issue's specification of them; that 'valid' counts the non-ignored labels of the whole batch, that 'batch'
divides by label.shape[0], that an ignored row gets zeros and that a label outside [0, C) hits no class rests on
memory of upstream 1.6 (src/operator/softmax_output-inl.h, mshadow's SoftmaxGrad), not on a file in the tree.
The METRICS are pinned to the reference's own classes (core/detection_metric.py:40-66,134-156) by
tests/golden/rcnn_loss_metrics.npz.

  rows_f32(...)     float32, every step rounded on its own, in the order of the specification:
                       m = max x; e_c = exp(x_c - m); s = e_0 + e_1 + ... (left to right); p_c = e_c / s
                       g_c = (p_c - [c == int(label)]) * (grad_scale / float32(norm)), zeros on ignored rows
                       v = delta - target; loss = weight * smooth_l1(v); d = smooth_l1'(v) * (weight * grad_scale)
  rows_truth(...)   the same in float64 from the float32 inputs, with the error scale T per output so that an
                    error reads k = |got - truth| / (eps32 * T + tiny)  (k_of, as tests/sigmoid_ce_ref.py):
                       prob      p * (1 + |x_c - m|)      (the rounding of x - m scales e_c by eps * |x_c - m|)
                       d_cls     (T_prob + |p - onehot|) * |scale|
                       reg_loss  |w| * (|v| + 0.5 / sigma^2) beyond 1 / sigma^2, |loss| inside
                       d_delta   |d|
                       reg_sum   sum T_reg_loss
  metrics(...)      the four numbers of the state block from prob, labels and reg_loss, as AccWithIgnore and L1 do
"""
import numpy as np

from tests.sigmoid_ce_ref import EPS32, TINY32, k_of  # noqa: F401

F = np.float32
OUTPUTS = ("prob", "d_cls", "reg_loss", "d_delta", "reg_sum")


def _int_label(label):
    with np.errstate(invalid="ignore"):
        return np.asarray(label, F).astype(np.int32)


def softmax_rows_f32(x):
    """x (P, C) float32 -> p (P, C) float32"""
    x = np.asarray(x, F)
    m = x.max(axis=1, keepdims=True)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp((x - m).astype(F), dtype=F)
        s = e[:, 0].copy()
        for c in range(1, x.shape[1]):
            s = (s + e[:, c]).astype(F)
        return (e / s[:, None]).astype(F)


def smooth_l1_f32(v, sigma):
    bsq = F(sigma) * F(sigma)
    ibsq = F(1) / bsq
    with np.errstate(invalid="ignore", over="ignore"):
        quad = (((F(0.5) * v).astype(F) * v).astype(F) * bsq).astype(F)
        hi = (v - (F(0.5) * ibsq).astype(F)).astype(F)
        lo = ((-v) - (F(0.5) * ibsq).astype(F)).astype(F)
        loss = np.where(v > ibsq, hi, np.where(v < -ibsq, lo, quad)).astype(F)
        grad = np.where(v > ibsq, F(1), np.where(v < -ibsq, F(-1), (bsq * v).astype(F))).astype(F)
    return loss, grad


def norm_of(label, ignore):
    k = _int_label(label).reshape(-1)
    return k.size if ignore is None else max(1, int(np.sum(k != int(ignore))))


def rows_f32(x, label, delta, target, weight, *, ignore, sigma, cls_gs, reg_gs, norm=None):
    """x (P, C), label (P,), delta / target / weight any equal shape; ignore: the ignore label or None ('batch').
    -> dict(prob, d_cls, reg_loss, d_delta, reg_sum)"""
    out = {}
    if x is not None:
        x = np.asarray(x, F)
        k = _int_label(label).reshape(-1)
        p = softmax_rows_f32(x)
        n = norm_of(label, ignore) if norm is None else norm
        scale = F(cls_gs) / F(n)
        onehot = (np.arange(x.shape[1])[None, :] == k[:, None]).astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            g = ((p - onehot).astype(F) * scale).astype(F)
        if ignore is not None:
            g = np.where((k == int(ignore))[:, None], F(0), g).astype(F)
        out.update(prob=p, d_cls=g)
    if delta is not None:
        delta, target, weight = (np.asarray(t, F) for t in (delta, target, weight))
        with np.errstate(invalid="ignore", over="ignore"):
            v = (delta - target).astype(F)
            loss, grad = smooth_l1_f32(v, sigma)
            reg = (weight * loss).astype(F)
            d = (grad * (weight * F(reg_gs)).astype(F)).astype(F)
            out.update(reg_loss=reg, d_delta=d, reg_sum=F(reg.reshape(-1).sum(dtype=F)))
    return out


def rows_truth(x, label, delta, target, weight, *, ignore, sigma, cls_gs, reg_gs, norm=None):
    """-> (dict of float64 truths, dict of T)"""
    out, T = {}, {}
    if x is not None:
        x = np.asarray(x, F).astype(np.float64)
        k = _int_label(label).reshape(-1)
        m = x.max(axis=1, keepdims=True)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp(x - m)
            p = e / e.sum(axis=1, keepdims=True)
            n = norm_of(label, ignore) if norm is None else norm
            scale = float(F(cls_gs)) / float(n)
            onehot = (np.arange(x.shape[1])[None, :] == k[:, None]).astype(np.float64)
            g = (p - onehot) * scale
            Tp = p * (1.0 + np.abs(x - m))
            Tg = (Tp + np.abs(p - onehot)) * abs(scale)
        if ignore is not None:
            ign = (k == int(ignore))[:, None]
            g, Tg = np.where(ign, 0.0, g), np.where(ign, 0.0, Tg)
        out.update(prob=p, d_cls=g)
        T.update(prob=Tp, d_cls=Tg)
    if delta is not None:
        delta, target, weight = (np.asarray(t, F).astype(np.float64) for t in (delta, target, weight))
        bsq = float(F(sigma) * F(sigma))
        ibsq = float(F(1) / F(bsq))
        with np.errstate(invalid="ignore", over="ignore"):
            v = delta - target
            lin = np.abs(v) > ibsq
            sl = np.where(lin, np.abs(v) - 0.5 * ibsq, 0.5 * v * v * bsq)
            gr = np.where(v > ibsq, 1.0, np.where(v < -ibsq, -1.0, bsq * v))
            reg = weight * sl
            d = gr * (weight * float(F(reg_gs)))
            Tr = np.where(lin, np.abs(weight) * (np.abs(v) + 0.5 * ibsq), np.abs(reg))
        out.update(reg_loss=reg, d_delta=d, reg_sum=reg.sum())
        T.update(reg_loss=Tr, d_delta=np.abs(d), reg_sum=np.nansum(Tr))
    return out, T


# ------------------------------------------------------------------------------ the heads' layouts --
def rpn_concat(cls_levels, delta_levels):
    """the reference's reshape + concat: logits (N, 2, A, HW) and deltas (N, 4A, HW) from the level tensors"""
    N = (cls_levels or delta_levels)[0].shape[0]
    x = d = None
    if cls_levels is not None:
        A = cls_levels[0].shape[1] // 2
        x = np.concatenate([np.asarray(c, F).reshape(N, 2, A, -1) for c in cls_levels], axis=-1)
    if delta_levels is not None:
        d = np.concatenate([np.asarray(t, F).reshape(N, t.shape[1], -1) for t in delta_levels], axis=2)
    return x, d


def rpn_split(full, levels, per):
    """a concat-layout array (N, per * A, HW) or (N, 2, A, HW) back into arrays of the levels' shapes"""
    out, o = [], 0
    for t in levels:
        hw = int(np.prod(t.shape[2:]))
        out.append(np.ascontiguousarray(full[..., o:o + hw]).reshape(t.shape))
        o += hw
    return out


def rpn(fn, cls_levels, delta_levels, label, target, weight, *, ignore=-1, sigma=3.0, cls_gs=1.0, reg_gs=1.0,
        norm=None):
    """fn = rows_f32 or rows_truth on the RPN head's layout.  Returns what fn returns with prob (N, 2, A, HW),
    reg_loss (N, 4A, HW) and d_cls / d_delta as lists of level arrays."""
    x, d = rpn_concat(cls_levels, delta_levels)
    rows = None
    if x is not None:
        N, _, A, HW = x.shape
        rows = x.reshape(N, 2, A * HW).transpose(0, 2, 1).reshape(-1, 2)
    res = fn(rows, None if x is None else np.asarray(label, F).reshape(-1), d,
             None if d is None else np.asarray(target, F).reshape(d.shape),
             None if d is None else np.asarray(weight, F).reshape(d.shape),
             ignore=ignore, sigma=sigma, cls_gs=cls_gs, reg_gs=reg_gs, norm=norm)

    def back(o):
        o = dict(o)
        if x is not None:
            for key in ("prob", "d_cls"):
                o[key] = o[key].reshape(N, A * HW, 2).transpose(0, 2, 1).reshape(N, 2, A, HW)
            o["d_cls"] = rpn_split(o["d_cls"], cls_levels, 2)
        if d is not None:
            o["d_delta"] = rpn_split(o["d_delta"], delta_levels, 4)
        return o
    return tuple(back(o) for o in res) if isinstance(res, tuple) else back(res)


def rcnn(fn, cls_logit, label, delta, target, weight, *, sigma=1.0, cls_gs=1.0, reg_gs=1.0):
    return fn(cls_logit, label, delta, target, weight, ignore=None, sigma=sigma, cls_gs=cls_gs, reg_gs=reg_gs)


# ----------------------------------------------------------------------------------------- metrics --
def metrics(prob, label, reg_loss, ignore=-1):
    """(acc numerator, acc denominator, L1 numerator, L1 denominator) = (correct, valid, reg_sum, fg) as
    AccWithIgnore and L1 compute them: prob (N, C, ...) with the classes on axis 1, arg-max with ties to the lower
    class (mx.nd.argmax_channel), labels cast to int32.  ignore=None: no row is dropped ('batch': valid = rows)."""
    prob = np.asarray(prob)
    pred = np.argmax(prob.reshape(prob.shape[0], prob.shape[1], -1), axis=1).astype(np.int32).reshape(-1)
    k = _int_label(label).reshape(-1)
    keep = np.ones(k.shape, bool) if ignore is None else k != int(ignore)
    correct = int(np.sum(pred[keep] == k[keep]))
    fg = int(np.sum(keep & (k != 0)))
    reg_sum = None if reg_loss is None else F(np.asarray(reg_loss, F).reshape(-1).sum(dtype=F))
    return correct, int(keep.sum()), reg_sum, fg


def k_all(got, truth_, T, keys=OUTPUTS):
    """k per output; lists of level arrays are compared level by level (the worst counts)"""
    ks = {}
    for key in keys:
        if key not in truth_:
            continue
        g, t, s = got[key], truth_[key], T[key]
        if isinstance(t, list):
            ks[key] = max([k_of(a, b, c) for a, b, c in zip(g, t, rpn_split_like(s, t))] or [0.0])
        else:
            ks[key] = k_of(g, t, s)
    return ks


def rpn_split_like(s, t):
    return s if isinstance(s, list) else [s] * len(t)


# ------------------------------------------------------------------------------------------ cases --
IBSQ = {3.0: F(1) / (F(3) * F(3)), 1.0: F(1)}
TIE_LO = F(0.1)                                     # |x| < 0.25: one ulp is below 2^-25, so expf(-ulp) rounds to 1
TIE_HI = np.nextafter(F(0.1), F(1))


def _plant_box(d, t, w, sigma, rs):
    """into flat views of delta / target / weight: v exactly at +-1 / sigma^2 and one ulp to either side, and weights
    other than 0 / 1"""
    ib = IBSQ[float(sigma)]
    vals = [ib, -ib, np.nextafter(ib, F(1)), np.nextafter(ib, F(0)), -np.nextafter(ib, F(1)), -np.nextafter(ib, F(0))]
    n = d.size
    for i, v in enumerate(vals):
        j = (3 * i + 1) % n
        d[j], t[j], w[j] = v, F(0), F(1)
    for i, wv in enumerate((0.25, 2.5, -1.5)):
        w[(5 * i + 2) % n] = F(wv)


def _plant_rows(x, label, K):
    """x (P, K), label (P,): a label >= K, equal logits, the one-ulp tie (label = the class the logits prefer, the
    probabilities do not), +-1e4; rows P - 1, P - 2, ... so that small cases keep the later ones.  Returns the row of
    the tie or None."""
    P = x.shape[0]
    tie = None
    rows = [P - 1 - i for i in range(5)]
    if P >= 5:
        label[rows[4]] = K + 5                      # far outside
    if P >= 4:
        label[rows[3]] = K                          # the first label outside [0, K)
    if P >= 3:
        x[rows[2]] = F(0.75)                        # equal logits: the arg-max is class 0
        label[rows[2]] = 0
    if P >= 2:
        x[rows[1]] = F(-1e4)
        x[rows[1], K - 1] = F(1e4)
        label[rows[1]] = K - 1
    if K >= 2:
        lo, hi = (0, 1) if K < 6 else (3, 5)
        x[rows[0]] = F(-5)
        x[rows[0], lo], x[rows[0], hi] = TIE_LO, TIE_HI
        label[rows[0]] = hi
        tie = rows[0]
    return tie


RPN_CASES = (
    # name, N, A, level sizes, labels ('mix', 'all_ignored', 'none_ignored')
    ("fpn5", 2, 3, ((5, 7), (3, 4), (2, 2), (1, 1), (1, 1)), "mix"),          # HW = 53; 318 rows: levels share workgroups
    ("a1", 2, 1, ((4, 5), (2, 3)), "mix"),
    ("c4", 1, 3, ((6, 7),), "mix"),
    ("span3", 1, 1, ((30, 30), (3, 3)), "mix"),                                # level 0 spans four workgroups of 256 rows
    ("stride2", 1, 3, ((296, 300), (5, 5)), "mix"),                            # 266,475 rows > 1024 workgroups: second trip
    ("all_ignored", 2, 3, ((5, 7), (3, 4), (2, 2), (1, 1), (1, 1)), "all_ignored"),
    ("none_ignored", 2, 1, ((4, 5), (2, 3)), "none_ignored"),
)


def make_rpn_case(name, seed=0, nan=False):
    _, N, A, sizes, kind = [c for c in RPN_CASES if c[0] == name][0]
    rs = np.random.RandomState(sum(map(ord, name)) + 17 * seed)
    HW = sum(h * w for h, w in sizes)
    x = (rs.standard_normal((N, 2, A, HW)) * 3).astype(F)
    d = rs.standard_normal((N, 4 * A, HW)).astype(F)
    t = (rs.standard_normal((N, 4 * A, HW)) * 0.5).astype(F)
    w = (rs.uniform(size=(N, 4 * A, HW)) < 0.3).astype(F)
    label = rs.choice([-1.0, 0.0, 1.0], size=(N, A * HW), p=[0.5, 0.3, 0.2]).astype(F)
    rows = np.ascontiguousarray(x.reshape(N, 2, A * HW).transpose(0, 2, 1)).reshape(-1, 2)
    tie = _plant_rows(rows, label.reshape(-1), 2)
    x = np.ascontiguousarray(rows.reshape(N, A * HW, 2).transpose(0, 2, 1)).reshape(N, 2, A, HW)
    if kind == "all_ignored":
        label[:] = -1
    elif kind == "none_ignored":
        label[label == -1] = 0
    _plant_box(d.reshape(-1), t.reshape(-1), w.reshape(-1), 3.0, rs)
    if nan:
        j = d.size // 2
        d.reshape(-1)[j], w.reshape(-1)[j] = np.nan, 0
    cls, delta, o = [], [], 0
    for h, wd in sizes:
        cls.append(np.ascontiguousarray(x[..., o:o + h * wd]).reshape(N, 2 * A, h, wd))
        delta.append(np.ascontiguousarray(d[..., o:o + h * wd]).reshape(N, 4 * A, h, wd))
        o += h * wd
    return dict(name=name, N=N, A=A, HW=HW, sizes=sizes, cls=cls, delta=delta, label=label, target=t, weight=w,
                tie_row=tie, sigma=3.0, cls_gs=128.0, reg_gs=128.0 / (N * 256), nan_at=(d.size // 2 if nan else None))


RCNN_SHAPES = ((1, 2), (7, 81), (130, 81), (64, 65), (5, 1),      # the issue's
               (3, 200),                                         # K > 128: the sixteen-per-lane instantiation
               (4100, 3))                                        # more than 1024 workgroups of four rows: second trip


def make_rcnn_case(R, K, agnostic, seed=0, nan=False):
    """agnostic: D = 4, else D = 4 K"""
    rs = np.random.RandomState(1000 * R + K + (7 if agnostic else 0) + 31 * seed)
    D = 4 if agnostic else 4 * K
    x = (rs.standard_normal((R, K)) * 3).astype(F)
    label = rs.randint(0, K, size=R).astype(F)
    label[rs.uniform(size=R) < 0.5] = 0
    if R >= 6:
        label[0] = -1                                # no class, and no ignore in this head
        label[1] = F(2.7) if K > 2 else F(0.7)       # truncated
    tie = _plant_rows(x, label, K)
    sigma = 1.0 if (R + K) % 2 else 3.0
    d = rs.standard_normal((R, D)).astype(F)
    t = (rs.standard_normal((R, D)) * 0.5).astype(F)
    w = (rs.uniform(size=(R, D)) < 0.3).astype(F)
    _plant_box(d.reshape(-1), t.reshape(-1), w.reshape(-1), sigma, rs)
    if nan:
        j = d.size // 2
        d.reshape(-1)[j], w.reshape(-1)[j] = np.nan, 0
    return dict(R=R, K=K, D=D, x=x, label=label, delta=d, target=t, weight=w, tie_row=tie, sigma=sigma,
                cls_gs=128.0, reg_gs=128.0 / max(R, 1), nan_at=(d.size // 2 if nan else None))


def rpn_case_fn(fn, c, **over):
    kw = dict(ignore=-1, sigma=c["sigma"], cls_gs=c["cls_gs"], reg_gs=c["reg_gs"])
    kw.update(over)
    return rpn(fn, c["cls"], c["delta"], c["label"], c["target"], c["weight"], **kw)


def rcnn_case_fn(fn, c):
    return rcnn(fn, c["x"], c["label"], c["delta"], c["target"], c["weight"], sigma=c["sigma"], cls_gs=c["cls_gs"],
                reg_gs=c["reg_gs"])
