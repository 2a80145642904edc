"""Cases and restatements for the CrowdHuman double-prediction head (models/crowdhuman); numpy only.

  RoI targets    The expected values are NOT restated here: tests/golden/crowdhuman_target.npz holds what the reference's
                 own bbox_target.py / bbox_sec_target.py gave on the inputs that target_cases() builds
                 (tests/golden/make_golden_crowdhuman.py).  Here: the case builder, and the float64 truth of the box
                 encoding on the float32 operands the reference forms,
                     ew = x2 - x1 + 1, ecx = x1 + 0.5 ew (float32, as bbox_transform_inv computes them)
                     dx = ix (gcx - ecx) / ew          T = |ix| (|gcx| + |ecx|) / ew
                     dw = iw log(gw / ew)              T = |iw| (1 + |log(gw / ew)|)
                 (a relative error eps of the quotient is an absolute error eps of its logarithm, hence the 1), so that
                 an error reads k = |got - truth| / (eps32 T + tiny) (sigmoid_ce_ref.k_of).
  EMD loss       emd_f32: float32 in the device's order of operations; emd_truth: float64 with T = the sum of the
                 absolute values of the terms:
                     ce(x, y) = -log(softmax(x)[y] + 1e-10)      T = |x_y - max| + |log sum| + 1
                     w sl1(v), v = d - t                         T = |w| (sl1(v) + |v sl1'(v)| + [|v| > 1/s^2] 0.5 / s^2)
                     L = the sum of a row's terms                T = the sum of theirs;  loss: the mean over the rows
                     (softmax_k - onehot_k) g                    T = (softmax_k (|x_k - max| + |log sum| + 2) + onehot_k) |g|
                     g w sl1'(v)                                 T = |g w sl1'(v)|
                 check_loss_inputs: every row is an exact tie by construction or has |L1 - L2| >= 1e-3 max(L1, L2), so
                 float32 rounding cannot decide a pairing.
"""
import numpy as np

from . import sigmoid_ce_ref as sr

F = np.float32
k_of = sr.k_of

CONFIG = dict(num_reg_class=2, add_gt_to_proposal=True, image_rois=64, fg_fraction=0.5, fg_thresh=0.5,
              bg_thresh_hi=0.5, bg_thresh_lo=0.0, bbox_target_std=(0.1, 0.1, 0.2, 0.2))


# ------------------------------------------------------------------------------------- target cases --
def _q(v):
    """quarter-pixel coordinates (exact in float32, and the fixture compresses)"""
    return np.round(np.asarray(v, np.float64) * 4) / 4


def _gt_grid(rs, n):
    """n boxes that do not touch each other: one per 200-pixel cell, 60 .. 100 pixels wide and high"""
    out = np.zeros((n, 4))
    for k in range(n):
        x1, y1 = 200 * (k % 8) + rs.uniform(0, 40), 200 * (k // 8) + rs.uniform(0, 40)
        out[k] = (x1, y1, x1 + rs.uniform(60, 100), y1 + rs.uniform(60, 100))
    return _q(out)


def _near(rs, box, n, jitter=3.0):
    return _q(box[None] + rs.uniform(-jitter, jitter, (n, 4)))          # IoU >= 0.8 with a box of >= 60 pixels


def _mid(rs, box, n):
    w, h = box[2] - box[0], box[3] - box[1]
    s = rs.uniform(0.1, 0.6, (n, 2)) * rs.choice([-1, 1], (n, 2))
    return _q(box[None] + np.stack([s[:, 0] * w, s[:, 1] * h, s[:, 0] * w, s[:, 1] * h], 1))


def _far(rs, n):
    x1, y1 = rs.uniform(5000, 6000, n), rs.uniform(0, 1000, n)          # IoU 0 with every gt of _gt_grid
    return _q(np.stack([x1, y1, x1 + rs.uniform(20, 200, n), y1 + rs.uniform(20, 200, n)], 1))


def _image(rs, P, M, classes, near=0, mid=0, pad_prop=0, shuffle=True, gt_boxes=None, extra=None):
    """one image: proposal (P, 4), gt (M, 5).  classes: the class of every non-padding gt row, in order (-2 = ignore);
    near / mid proposals are spread over the non-ignore gts round robin, the rest lie far away; pad_prop all-zero
    proposal rows and the M - len(classes) padding gt rows sit at random places in the MIDDLE of their arrays."""
    n_gt = len(classes)
    boxes = _gt_grid(rs, n_gt) if gt_boxes is None else np.asarray(gt_boxes, np.float64)
    real = [k for k, c in enumerate(classes) if c > 0]
    rows = []
    for i in range(near):
        rows.append(_near(rs, boxes[real[i % len(real)]], 1))
    for i in range(mid):
        rows.append(_mid(rs, boxes[real[i % len(real)]], 1))
    if extra is not None:
        rows.append(np.asarray(extra, np.float64).reshape(-1, 4))
    have = sum(len(r) for r in rows)
    rows.append(_far(rs, P - pad_prop - have))
    prop = np.concatenate(rows, 0)
    if shuffle:
        prop = prop[rs.permutation(len(prop))]
    for _ in range(pad_prop):
        prop = np.insert(prop, rs.randint(1, len(prop)), 0.0, axis=0)
    gt = np.concatenate([boxes, np.asarray(classes, np.float64)[:, None]], 1)
    for _ in range(M - n_gt):
        gt = np.insert(gt, rs.randint(1, len(gt)) if len(gt) > 1 else 1, -1.0, axis=0)
    assert prop.shape == (P, 4) and gt.shape == (M, 5)
    return prop.astype(F), gt.astype(F)


def _case(name, images, mode, **cfg):
    c = dict(CONFIG)
    c.update(cfg)
    return dict(name="%s-m%d" % (name, mode), mode=mode, cfg=c,
                proposal=np.stack([p for p, _ in images]), gt=np.stack([g for _, g in images]))


def _square(x, y, w, h):
    return [x, y, x + w - 1, y + h - 1]


def target_cases(full=True):
    """every target case of test_crowdhuman_head.py: a list of dict(name, mode, cfg, proposal (B, P, 4), gt (B, M, 5)).
    n_fg of an image = its near proposals + (add_gt_to_proposal: its gts of a class > 0)."""
    out = []
    for mode in (0, 1):
        rs = np.random.RandomState(100 + mode)
        # 1. the config's parameters at small size: near, mid-IoU and far proposals, an ignore row, padding
        out.append(_case("config-small", [_image(rs, 300, 16, [1, 1, -2, 1, 1, 1, 1], near=20, mid=60, pad_prop=7)
                                          for _ in range(2)], mode))
        # 2. foreground lists of one entry (no draw) and of two
        out.append(_case("n1-n2", [_image(rs, 100, 4, [1, 1], near=n) for n in (1, 2)], mode, add_gt_to_proposal=False,
                         image_rois=16))
        # 3. n equal to, below and above the quota of 16
        out.append(_case("quota", [_image(rs, 120, 8, [1, 1, 1, 1], near=n - 4) for n in (16, 10, 24)], mode,
                         image_rois=32))
        # 4. mask-segment and wave-batch edges of the permutation
        out.append(_case("n63-64-65", [_image(rs, 200, 8, [1, 1, 1], near=n - 3) for n in (63, 64, 65)], mode))
        out.append(_case("n127-128-129", [_image(rs, 300, 8, [1, 1, 1], near=n - 3) for n in (127, 128, 129)], mode))
        # 5. a background list above 1024
        out.append(_case("bg-above-1024", [_image(rs, 1200, 8, [1, 1, 1], near=40, pad_prop=3) for _ in range(2)], mode))
        # 6. one gt in the class: second IoU -1, second label 0
        out.append(_case("single-gt", [_image(rs, 100, 4, [1], near=30, mid=20) for _ in range(2)], mode, image_rois=32))
        # 7. duplicate gt boxes: the first arg-max wins, the second is a foreground of equal IoU
        imgs = []
        for _ in range(2):
            b = _gt_grid(rs, 2)
            imgs.append(_image(rs, 100, 6, [1, 1, 1, 1], near=30, mid=10, gt_boxes=[b[0], b[1], b[0], b[1]]))
        out.append(_case("duplicate-gt", imgs, mode, image_rois=32))
        # 8. ignore rows that overlap proposals and a real gt, in front of the real rows (the two modes index the gt
        #    list differently)
        imgs = []
        for _ in range(2):
            b = _gt_grid(rs, 3)
            ign = _q(b[1] + np.array([20.0, 10.0, 20.0, 10.0]))
            imgs.append(_image(rs, 150, 8, [-2, 1, 1, -2, 1], near=24, mid=12, gt_boxes=[ign, b[0], b[1], b[2] + 900, b[2]],
                               extra=_near(rs, ign, 12)))
        out.append(_case("ignore-overlap", imgs, mode, image_rois=32))
        # 9. three classes, a class 2 box equal to a class 1 box (equal maxima: the strict > keeps class 1) and one alone
        imgs = []
        for _ in range(2):
            b = _gt_grid(rs, 3)
            imgs.append(_image(rs, 150, 8, [1, 2, 2, 1], near=40, mid=10, gt_boxes=[b[0], b[0], b[1], b[2]],
                               extra=_near(rs, b[1], 10)))
        out.append(_case("three-classes", imgs, mode, num_reg_class=3, image_rois=32))
        # 10. IoU exactly at the thresholds: gt 100 x 100, proposals of 50, 25, 24, 51, 70 and 10 rows of it
        for tag, thr in (("a", (0.5, 0.5, 0.25)), ("b", (0.7, 0.7, 0.1))):
            imgs = []
            for _ in range(2):
                ex = [_square(0, 0, 100, hh) for hh in (50, 25, 24, 51, 70, 10, 49, 26, 71, 69, 11, 9)] * 3
                imgs.append(_image(rs, 80, 4, [1, 1], near=6, gt_boxes=[_square(0, 0, 100, 100), _square(400, 0, 80, 80)],
                                   extra=ex))
            out.append(_case("thresholds-" + tag, imgs, mode, fg_thresh=thr[0], bg_thresh_hi=thr[1], bg_thresh_lo=thr[2],
                             image_rois=16))
        # 11. padding rows in the middle of both inputs
        out.append(_case("padding", [_image(rs, 200, 16, [1, 1, 1], near=30, mid=20, pad_prop=60) for _ in range(2)], mode,
                         image_rois=32))
        # 12. the gt boxes do not join the candidates
        out.append(_case("no-add-gt", [_image(rs, 200, 8, [1, -2, 1, 1], near=30, mid=30) for _ in range(2)], mode,
                         add_gt_to_proposal=False, image_rois=32))
        # 13. fg_fraction * image_rois half way between two integers: 8.5 -> 8, 9.5 -> 10
        for S in (17, 19):
            out.append(_case("half-even-%d" % S, [_image(rs, 100, 4, [1, 1], near=20) for _ in range(2)], mode,
                             image_rois=S))
        # 14. the config's full shape
        if full:
            out.append(_case("full", [_image(rs, 2000, 500, [1] * 38 + [-2] * 2, near=300, mid=500, pad_prop=31)
                                      for _ in range(2)], mode, image_rois=512))
    return out


def two_call_inputs():
    """the second call's inputs of the two-consecutive-calls test (the first call is config-small-m1)"""
    rs = np.random.RandomState(777)
    return _case("second-call", [_image(rs, 300, 16, [1, 1, 1, -2, 1], near=25, mid=50, pad_prop=5) for _ in range(2)], 1)


def short_case(mode):
    """image 0 cannot fill its 32 rows (19 candidates), image 1 can"""
    rs = np.random.RandomState(900 + mode)
    return _case("short", [_image(rs, 40, 4, [1, 1], near=5, pad_prop=23), _image(rs, 40, 4, [1, 1], near=10)], mode,
                 image_rois=32)


def encode_truth(boxes, gts, inv_stds):
    """float64 truth of bbox_transform_inv on the float32 operands it forms -> (targets (n, 4), T (n, 4))"""
    b, g = np.asarray(boxes, F), np.asarray(gts, F)
    one, half = F(1.0), F(0.5)
    ew, eh = b[:, 2] - b[:, 0] + one, b[:, 3] - b[:, 1] + one
    ecx, ecy = b[:, 0] + half * ew, b[:, 1] + half * eh
    gw, gh = g[:, 2] - g[:, 0] + one, g[:, 3] - g[:, 1] + one
    gcx, gcy = g[:, 0] + half * gw, g[:, 1] + half * gh
    ix, iy, iw, ih = [float(F(v)) for v in inv_stds]
    d = lambda a: a.astype(np.float64)
    with np.errstate(all="ignore"):
        t = np.stack([ix * (d(gcx) - d(ecx)) / d(ew), iy * (d(gcy) - d(ecy)) / d(eh),
                      iw * np.log(d(gw) / d(ew)), ih * np.log(d(gh) / d(eh))], 1)
        T = np.stack([abs(ix) * (np.abs(d(gcx)) + np.abs(d(ecx))) / d(ew), abs(iy) * (np.abs(d(gcy)) + np.abs(d(ecy))) / d(eh),
                      abs(iw) * (1 + np.abs(np.log(d(gw) / d(ew)))), abs(ih) * (1 + np.abs(np.log(d(gh) / d(eh))))], 1)
    return t, T


# ----------------------------------------------------------------------------------------- EMD loss --
def _sl1(v, s2):
    a = np.abs(v)
    return np.where(a > 1 / s2, a - 0.5 / s2, 0.5 * v * v * s2)


def _sl1g(v, s2):
    return np.where(v > 1 / s2, 1.0, np.where(v < -1 / s2, -1.0, s2 * v))


def _cols(y, K):
    y = np.asarray(y, F)
    ok = (y >= 0) & (y < K)
    return np.where(ok, np.where(ok, y, 0).astype(np.int64), -1)


def softmax_entropy(x, y, dtype=F):
    """softmax_entropy_op.py's forward summed over the row, in `dtype` -> (ce (R,), softmax (R, K), T of ce)"""
    x = np.asarray(x, F).astype(dtype)
    R, K = x.shape
    c = _cols(y, K)
    mx = x.max(1, keepdims=True)
    e = np.exp(x - mx)
    s = e.sum(1, keepdims=True, dtype=dtype)
    p = (e / s).astype(dtype)
    rows = np.arange(R)
    py = np.where(c >= 0, p[rows, np.maximum(c, 0)], 1.0).astype(dtype)
    ce = np.where(c >= 0, -np.log(py + dtype(1e-10)), 0.0).astype(dtype)
    T = np.where(c >= 0, np.abs(x[rows, np.maximum(c, 0)] - mx[:, 0]) + np.abs(np.log(s[:, 0])) + 1.0, 0.0)
    return ce, p, T


def _emd(c, dtype):
    """both pairings in `dtype`: dict(L1, L2, pairing, loss, g1, g2, gd1, gd2) and the T of each"""
    f = lambda k: np.asarray(c[k], F).astype(dtype)
    x1, x2, d1, d2, t1, t2, w1, w2 = [f(k) for k in ("x1", "x2", "d1", "d2", "t1", "t2", "w1", "w2")]
    R, K = x1.shape
    s2 = dtype(c["sigma"]) * dtype(c["sigma"])
    g = dtype(dtype(c["scale"]) / dtype(R))
    ce, Tce, p = {}, {}, {}
    for h, x in ((1, x1), (2, x2)):
        for l in (1, 2):
            ce[h, l], p[h], Tce[h, l] = softmax_entropy(x, c["y%d" % l], dtype)
    def reg(da, ta, wa, db, tb, wb):
        terms = (wa * _sl1(da - ta, s2)).astype(dtype) + (wb * _sl1(db - tb, s2)).astype(dtype)
        acc = np.zeros(R, dtype)
        for k in range(terms.shape[1]):                     # the device's order: column by column
            acc = (acc + terms[:, k]).astype(dtype)
        Tr = 0
        for d_, t_, w_ in ((da, ta, wa), (db, tb, wb)):
            v = d_ - t_
            Tr = Tr + (np.abs(w_) * (_sl1(v, s2) + np.abs(v * _sl1g(v, s2)) + (np.abs(v) > 1 / s2) * 0.5 / s2)).sum(1)
        return acc, Tr
    r1, Tr1 = reg(d1, t1, w1, d2, t2, w2)
    r2, Tr2 = reg(d1, t2, w2, d2, t1, w1)
    L1 = ((ce[1, 1] + ce[2, 2]).astype(dtype) + r1).astype(dtype)
    L2 = ((ce[1, 2] + ce[2, 1]).astype(dtype) + r2).astype(dtype)
    TL1, TL2 = Tce[1, 1] + Tce[2, 2] + Tr1, Tce[1, 2] + Tce[2, 1] + Tr2
    first = L1 <= L2
    lmin = np.where(first, L1, L2).astype(dtype)
    loss = dtype(lmin.sum(dtype=dtype) / dtype(R))
    Tloss = np.where(first, TL1, TL2).sum() / R
    c1, c2 = _cols(c["y1"], K), _cols(c["y2"], K)
    out, T = dict(L1=L1, L2=L2, pairing=np.where(first, 1, 2).astype(np.int32), loss=loss), dict(loss=Tloss)
    for h, x, name in ((1, x1, "g1"), (2, x2, "g2")):
        col = np.where(first, c1, c2) if h == 1 else np.where(first, c2, c1)
        oh = (np.arange(K)[None] == col[:, None]).astype(dtype)
        out[name] = ((p[h] - oh) * g).astype(dtype)
        mx = x.max(1, keepdims=True)
        ls = np.abs(np.log(np.exp(x - mx).sum(1, keepdims=True)))
        T[name] = (p[h] * (np.abs(x - mx) + ls + 2) + oh) * abs(g)
    f1 = first[:, None]
    out["gd1"] = np.where(f1, (g * w1) * _sl1g(d1 - t1, s2), (g * w2) * _sl1g(d1 - t2, s2)).astype(dtype)
    out["gd2"] = np.where(f1, (g * w2) * _sl1g(d2 - t2, s2), (g * w1) * _sl1g(d2 - t1, s2)).astype(dtype)
    T["gd1"], T["gd2"] = np.abs(out["gd1"]).astype(np.float64), np.abs(out["gd2"]).astype(np.float64)
    return out, T


def emd_f32(c):
    with np.errstate(all="ignore"):
        return _emd(c, F)[0]


def emd_truth(c):
    with np.errstate(all="ignore"):
        return _emd(c, np.float64)


OUTS = ("loss", "g1", "g2", "gd1", "gd2")


def emd_k_ref(c):
    tr, T = emd_truth(c)
    r = emd_f32(c)
    return {o: k_of(r[o], tr[o], T[o]) for o in OUTS}


RECIPES = ("general", "background-tie", "observable-tie", "zero-weight", "general", "linear-branch", "no-label")


def make_loss_case(R, K, seed=0, scale=1.0, sigma=1.0):
    """dict(x1, x2 (R, K), y1, y2 (R,), d1, d2, t1, t2, w1, w2 (R, 4 K), sigma, scale, recipes); row r follows
    RECIPES[r % 7]"""
    rs = np.random.RandomState(1000 * R + 10 * K + seed)
    D = 4 * K
    c = dict(sigma=float(sigma), scale=float(scale), recipes=[RECIPES[r % len(RECIPES)] for r in range(R)])
    for k in ("x1", "x2"):
        c[k] = (rs.standard_normal((R, K)) * 2).astype(F)
    for k in ("d1", "d2", "t1", "t2"):
        c[k] = (rs.standard_normal((R, D)) * 0.4 / sigma ** 2).astype(F)
    c["y1"] = rs.randint(1, K, R).astype(F)
    c["y2"] = rs.randint(0, K, R).astype(F)
    def expand(y):
        w = np.zeros((R, D), F)
        for r in range(R):
            if y[r] > 0:
                w[r, 4 * int(y[r]):4 * int(y[r]) + 4] = 1
        return w
    for r, what in enumerate(c["recipes"]):
        if what == "background-tie":                  # both labels 0, no box terms: L1 == L2 by construction
            c["y1"][r] = c["y2"][r] = 0
        elif what == "observable-tie":                # identical heads, different labels: a + b == b + a
            c["x2"][r], c["d2"][r] = c["x1"][r], c["d1"][r]
            c["y1"][r], c["y2"][r] = K - 1, 0
        elif what == "linear-branch":                 # |d - t| >= 1 / sigma^2 in every column
            c["d1"][r] += F(3.0 / sigma ** 2)
            c["d2"][r] -= F(2.5 / sigma ** 2)
        elif what == "no-label":                      # a second label that names no column
            c["y2"][r] = -1
    c["w1"], c["w2"] = expand(c["y1"]), expand(c["y2"])
    for r, what in enumerate(c["recipes"]):
        if what == "zero-weight":
            c["w1"][r] = c["w2"][r] = 0
            c["y2"][r] = (c["y1"][r] + 1) % K          # different labels, so the pairings differ
    # rows that are no tie by construction get a clear winner: pull the second head towards one pairing's targets
    # (the rows are independent: all that are still close take step s together)
    for step in range(1, 21):
        tr = emd_truth(c)[0]
        close = [r for r, what in enumerate(c["recipes"]) if "tie" not in what
                 and abs(tr["L1"][r] - tr["L2"][r]) < 2e-3 * max(tr["L1"][r], tr["L2"][r])]
        if not close:
            return c
        for r in close:
            c["x1"][r, int(c["y1"][r])] += F(0.5 * step)
            c["d1"][r, 4 * int(c["y1"][r])] += F(0.3 * step / sigma ** 2)
            if c["y2"][r] > 0:                          # (both heads on the linear branch: only the targets separate)
                c["t2"][r, 4 * int(c["y2"][r])] += F(0.3 * step / sigma ** 2)
    raise AssertionError("rows %s stay close" % close)


def check_loss_inputs(c):
    """every row: an exact tie by construction or |L1 - L2| >= 1e-3 max(L1, L2), in float64 AND in float32"""
    f32 = emd_f32(c)
    for r_ in (emd_truth(c)[0], f32):
        L1, L2 = np.asarray(r_["L1"], np.float64), np.asarray(r_["L2"], np.float64)
        for r, what in enumerate(c["recipes"]):
            if "tie" in what:
                assert f32["L1"][r] == f32["L2"][r], (r, what)
            else:
                assert abs(L1[r] - L2[r]) >= 1e-3 * max(L1[r], L2[r]), (r, what, L1[r], L2[r])


LOSS_SHAPES = ((37, 2), (37, 3), (1024, 2), (1024, 3))


def loss_cases():
    return {(R, K): make_loss_case(R, K, scale=128.0 if K == 3 else 1.0, sigma=3.0 if K == 3 else 1.0)
            for R, K in LOSS_SHAPES}


def ce_fixture_inputs():
    """inputs of the softmax_entropy fixture: (name, x (R, K), y (R,), out_grad scalar)"""
    out = []
    for R, K in ((37, 2), (64, 3)):
        rs = np.random.RandomState(R + K)
        x = (rs.standard_normal((R, K)) * 3).astype(F)
        x[0] = (30.0, -30.0) if K == 2 else (30.0, -30.0, 0.0)      # softmax underflows to ~1e-26: the 1e-10 matters
        y = rs.randint(0, K, R).astype(F)
        y[0] = 1
        out.append(("r%d-k%d" % (R, K), x, y, 0.25 / R))
    return out
