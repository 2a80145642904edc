"""A numpy restatement of the reference's FCOS training head, line by line:
make_fcos_gt with PreMakeFCOSgt / PrepareFCOS_cls_gt (models/FCOS/input.py:14-263), make_sigmoid_focal_loss,
make_binary_cross_entropy_loss and IoULoss (models/FCOS/loss.py:86-196) and the masks FCOSFPNHead.get_loss forms
in front of them (models/FCOS/builder.py:217-230).

  targets_f32        float32, the reference's operation order (mask multiplications and additions kept as they are).
  losses_f32         float32, the same order; the gradients of focal and BCE are the reference's `grad` symbols, the
                     IoU gradient is the derivative written out in the order the kernel uses (the reference leaves it
                     to MXNet's autograd).  Sums are numpy's float32 sums.
  losses_truth       the float32 TARGETS fed to float64 losses.  The IoU gradient comes from torch float64 autograd
                     on the restated forward.  Also returns, per gradient element, T = the sum of the absolute values
                     of the terms whose float32 roundings reach the element, and s = the scale applied after them:
                         k = |got - truth| / (eps32 * T * s + s * tiny)           (tests/focal_ref.py: k_of)
                     Why these T: one rounding of p = 1 / (1 + exp(-x)) is a RELATIVE error eps of p, so it is an
                     ABSOLUTE error eps in log(p) -- log terms count as |log| + 1 -- and an absolute error eps * p in
                     1 - p -- which counts as 1 + p, not as its small value.  The IoU gradient is a difference of
                     two quotients over I + 1 and U + 1, each a sum of products of sums: both quotients count with
                     their absolute values, and the areas under them with the sum of theirs.
"""
import numpy as np

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
STAGE_LOWER = (-1e-5, 64, 128, 256, 512)
STAGE_UPPER = (64, 128, 256, 512, 1e5)


def level_sizes(data_size, strides):
    """[(H_l, W_l)]: len(range(0, h, stride)), len(range(0, w, stride))  (input.py:99-107)"""
    h, w = data_size
    return [(len(range(0, h, s)), len(range(0, w, s))) for s in strides]


def num_locations(data_size, strides):
    return sum(a * b for a, b in level_sizes(data_size, strides))


def grid(data_size, strides, im_info, lower=STAGE_LOWER, upper=STAGE_UPPER):
    """PreMakeFCOSgt: loc_x, loc_y, stage_lowerbound, stage_upperbound, nonignore_area (float 0 / 1), all (HW,)"""
    h, w = data_size
    lx, ly, lxt, lyt, lo, up = [], [], [], [], [], []
    for idx, stride in enumerate(strides):
        x = np.array(range(0, w, stride), dtype=F32) + stride / 2.
        y = np.array(range(0, h, stride), dtype=F32) + stride / 2.
        x, y = np.meshgrid(x.astype(F32), y.astype(F32))
        lx.append(x.reshape(-1)); ly.append(y.reshape(-1))
        lxt.append(y.T.reshape(-1)); lyt.append(x.T.reshape(-1))
        lo.append(np.full(x.size, lower[idx], F32)); up.append(np.full(x.size, upper[idx], F32))
    ori_h, ori_w = F32(im_info[0, 0]), F32(im_info[0, 1])
    if ori_h < ori_w:
        loc_x, loc_y = np.concatenate(lx), np.concatenate(ly)
    else:
        loc_x, loc_y = np.concatenate(lxt), np.concatenate(lyt)
    nonignore = np.logical_and(loc_x < ori_w, loc_y < ori_h).astype(F32)
    return loc_x, loc_y, np.concatenate(lo), np.concatenate(up), nonignore


def targets_f32(gt_bbox, im_info, data_size, strides, num_classifier, ignore_offset=-1, ignore_label=-1,
                lower=STAGE_LOWER, upper=STAGE_UPPER):
    """-> dict(centerness (N, HW), cls_gt (N, K * HW), offset (N, 4, HW), cls_id (N, HW) int32, count int)"""
    gt = np.asarray(gt_bbox, F32)
    io, il, one = F32(ignore_offset), F32(ignore_label), F32(1)
    loc_x, loc_y, lo, up, nonignore = grid(data_size, strides, np.asarray(im_info, F32), lower, upper)
    N = gt.shape[0]
    with np.errstate(all="ignore"):
        l = loc_x - gt[:, :, 0:1]
        t = loc_y - gt[:, :, 1:2]
        r = gt[:, :, 2:3] - loc_x
        b = gt[:, :, 3:4] - loc_y
        off = np.stack([l, t, r, b], axis=1)                                   # (N, 4, M, HW)
        inbox = (off.min(axis=1, keepdims=True) >= 0).astype(F32)
        off = off * inbox + (one - inbox) * io
        greatest = off.max(axis=1, keepdims=True)
        stage = np.logical_and(greatest >= lo, greatest < up).astype(F32)
        off = off * stage + (one - stage) * io
        size = (off[:, 0:1] + off[:, 2:3]) * (off[:, 1:2] + off[:, 3:4])
        size = size * stage + (one - stage) * F32(1e10)
        best = np.argmin(size, axis=2)                                         # (N, 1, HW), the first minimum
        off = np.take_along_axis(off, np.tile(best, (1, 4, 1))[:, :, None, :], 2)[:, :, 0, :]      # (N, 4, HW)
        inbox = (off != io).astype(F32)
        lr, tb = np.sort(off[:, 0:3:2], axis=1), np.sort(off[:, 1:4:2], axis=1)
        c = np.sqrt(lr[:, 0] * tb[:, 0] / (lr[:, 1] * tb[:, 1]))
        c = c * inbox[:, 0]
        best = best.reshape(N, -1)
        cls = gt[:, :, 4][np.arange(N)[:, None], best] - one
        hot = (np.trunc(cls).astype(np.int64)[..., None] == np.arange(num_classifier)).astype(F32)   # (N, HW, K)
        cls_gt = np.transpose(hot, (0, 2, 1)) * inbox[:, 0:1]
        ni = nonignore.reshape(1, -1)
        c = c * ni + (one - ni) * il
        ni = nonignore.reshape(1, 1, -1)
        cls_gt = cls_gt * ni + (one - ni) * il
    cls_id = np.where(cls_gt[:, 0] == il, -1, (cls_gt.argmax(axis=1) + 1) * (cls_gt.max(axis=1) == 1)).astype(np.int32)
    labels = cls_gt.reshape(N, -1)
    count = int((labels * (labels != il)).sum(dtype=np.float64))
    return dict(centerness=c.astype(F32), cls_gt=labels.astype(F32), offset=off.astype(F32), cls_id=cls_id, count=count)


def concat_levels(levels):
    """builder.py:207-214: (N, C, H_l, W_l) per level -> (N, C, HW)"""
    return np.concatenate([np.asarray(v).reshape(v.shape[0], v.shape[1], -1) for v in levels], axis=2)


def split_levels(flat, hws, shapes=None):
    """the inverse: (N, C, HW) -> [(N, C, hw_l)] (reshaped to `shapes` when given)"""
    out, b = [], 0
    for i, hw in enumerate(hws):
        v = np.ascontiguousarray(flat[:, :, b:b + hw])
        out.append(v.reshape(shapes[i]) if shapes else v)
        b += hw
    return out


def _masks(xp, tg, ignore_offset, ignore_label, dt):
    labels, c = tg["cls_gt"], tg["centerness"]
    m_cls = (labels != F32(ignore_label)).astype(dt)
    m_ctr = np.logical_and(c != F32(ignore_label), c > 0).astype(dt)
    m_iou = np.logical_and(tg["offset"][:, 0:1] != F32(ignore_offset), c[:, None, :] > 0).astype(dt)
    return m_cls, m_ctr, m_iou


def losses_f32(cls_logits, ctr_logits, off_preds, tg, alpha=0.25, gamma=2.0, ignore_offset=-1, ignore_label=-1):
    """cls_logits (N, K, HW), ctr_logits (N, 1, HW), off_preds (N, 4, HW); tg = targets_f32(...).
    -> dict(losses (3,) = centerness, cls, offset; d_cls, d_ctr, d_off in the inputs' shapes)"""
    one = F32(1)
    N = cls_logits.shape[0]
    m_cls, m_ctr, m_iou = _masks(np, tg, ignore_offset, ignore_label, F32)
    with np.errstate(all="ignore"):
        # make_sigmoid_focal_loss
        logits, labels = np.asarray(cls_logits, F32).reshape(N, -1), tg["cls_gt"]
        g_, a_, oma = F32(gamma), F32(alpha), F32(1 - alpha)
        p = one / (one + np.exp(-logits))
        ge = (logits >= 0).astype(F32)
        minus_logits_mask = F32(-1.) * logits * ge
        negative_abs = logits - F32(2) * logits * ge
        minus_log = minus_logits_mask - np.log(one + np.exp(negative_abs))
        a1 = a_ * np.power(one - p, g_) * labels
        log_p_clip = np.log(np.clip(p, F32(1e-5), one))
        a2 = oma * np.power(p, g_) * (one - labels)
        norm = np.sum(labels * m_cls, dtype=F32) + one
        cls_loss = np.sum(F32(-1) * (a1 * log_p_clip + a2 * minus_log) * m_cls, dtype=F32) / norm
        bt1 = a1 * (one - p - p * g_ * log_p_clip)
        bt2 = a2 * (minus_log * (one - p) * g_ - p)
        d_cls = (F32(-1) * (bt1 + bt2) * m_cls / norm).astype(F32).reshape(cls_logits.shape)
        # make_binary_cross_entropy_loss
        x, c = np.asarray(ctr_logits, F32).reshape(N, -1), tg["centerness"]
        p = one / (one + np.exp(-x))
        bce = -c * np.log(np.clip(p, F32(1e-5), one)) - (one - c) * np.log(np.clip(one - p, F32(1e-5), one))
        nc = np.sum(m_ctr, dtype=F32) + F32(1e-30)
        ctr_loss = np.sum(bce * m_ctr, dtype=F32) / nc
        d_ctr = ((p - c) * m_ctr / nc).astype(F32).reshape(ctr_logits.shape)
        # IoULoss
        raw, y = np.asarray(off_preds, F32), tg["offset"]
        xb = np.clip(raw, F32(0), F32(1e4)) * m_iou
        cm = c[:, None, :] * m_iou
        tl, tt, tr, tb = (y[:, i:i + 1] for i in range(4))
        pl, pt, pr, pb = (xb[:, i:i + 1] for i in range(4))
        ta = (tl + tr) * (tt + tb)
        pw, ph = pl + pr, pt + pb
        pa = pw * ph
        wi = np.minimum(pl, tl) + np.minimum(pr, tr)
        hi = np.minimum(pb, tb) + np.minimum(pt, tt)
        ai = wi * hi
        au = ta + pa - ai
        i1, u1 = ai + one, au + one
        n_off = np.sum(cm, dtype=F32) + F32(1e-30)
        off_loss = np.sum(-np.log(i1 / u1) * cm, dtype=F32) / n_off
        d_off = np.zeros(raw.shape, F32)
        for e, (pe, te) in enumerate(((pl, tl), (pt, tt), (pr, tr), (pb, tb))):
            side, other = (wi, pw) if e & 1 else (hi, ph)
            d = np.where(pe <= te, side, F32(0))
            v = (other - d) / u1 - d / i1
            inside = np.logical_and(raw[:, e:e + 1] >= 0, raw[:, e:e + 1] <= F32(1e4))
            d_off[:, e:e + 1] = np.where(np.logical_and(inside, m_iou != 0), v * cm / n_off, F32(0))
    return dict(losses=np.array([ctr_loss, cls_loss, off_loss], F32).reshape(3), d_cls=d_cls, d_ctr=d_ctr, d_off=d_off)


def iou_ties(off_preds, tg, ignore_offset=-1):
    """number of unmasked elements with clip(pred) == target (the generators assert 0)"""
    m = np.logical_and(tg["offset"][:, 0:1] != F32(ignore_offset), tg["centerness"][:, None, :] > 0)
    return int(np.logical_and(np.clip(off_preds, 0, 1e4) == tg["offset"], m).sum())


def losses_truth(cls_logits, ctr_logits, off_preds, tg, alpha=0.25, gamma=2.0, ignore_offset=-1, ignore_label=-1):
    """float64 losses of the float32 targets.
    -> dict(losses (3,), d_cls, d_ctr, d_off, T_cls, T_ctr, T_off, s_cls, s_ctr, s_off (scalars), T_losses (3,))"""
    import torch
    D = np.float64
    N = cls_logits.shape[0]
    m_cls, m_ctr, m_iou = _masks(np, tg, ignore_offset, ignore_label, D)
    a_, oma, g_ = float(F32(alpha)), float(F32(1 - alpha)), float(F32(gamma))
    with np.errstate(all="ignore"):
        logits, labels = np.asarray(cls_logits, F32).astype(D).reshape(N, -1), tg["cls_gt"].astype(D)
        p = 1.0 / (1.0 + np.exp(-logits))
        minus_log = -np.maximum(logits, 0) - np.log1p(np.exp(-np.abs(logits)))
        log_p = np.log(np.clip(p, float(F32(1e-5)), 1.0))
        pos = labels == 1
        a1, a2 = a_ * np.power(1 - p, g_), oma * np.power(p, g_)
        norm = float((labels * m_cls).sum()) + 1.0
        elem = -np.where(pos, a1 * log_p, a2 * minus_log) * m_cls
        t_elem = np.where(pos, a1 * (np.abs(log_p) + 1), a2 * (np.abs(minus_log) + 1)) * m_cls
        cls_loss = elem.sum() / norm
        g = -np.where(pos, a1 * (1 - p - p * g_ * log_p), a2 * (minus_log * (1 - p) * g_ - p)) * m_cls
        T_cls = np.where(pos, a1 * (1 + p + p * g_ * (np.abs(log_p) + 1)),
                         a2 * ((np.abs(minus_log) + 1) * (1 + p) * g_ + p)) * m_cls
        x, c = np.asarray(ctr_logits, F32).astype(D).reshape(N, -1), tg["centerness"].astype(D)
        pc = 1.0 / (1.0 + np.exp(-x))
        lo = float(F32(1e-5))
        l1, l2 = np.log(np.clip(pc, lo, 1.0)), np.log(np.clip(1 - pc, lo, 1.0))
        nc = float(m_ctr.sum()) + 1e-30
        bce = np.where(m_ctr != 0, -c * l1 - (1 - c) * l2, 0.0)
        t_bce = np.where(m_ctr != 0, np.abs(c) * (np.abs(l1) + 1) + (1 + np.abs(c)) * (np.abs(l2) + 1 / np.maximum(1 - pc, lo)), 0.0)
        ctr_loss = bce.sum() / nc
        d_ctr = np.where(m_ctr != 0, (pc - c) / nc, 0.0)
        T_ctr = np.where(m_ctr != 0, pc + np.abs(c), 0.0)
    # IoU: torch float64 autograd on the restated forward
    raw = torch.tensor(np.asarray(off_preds, F32).astype(D), requires_grad=True)
    y = torch.tensor(tg["offset"].astype(D))
    mi = torch.tensor(m_iou)
    cm = torch.tensor(np.where(m_iou != 0, tg["centerness"].astype(D)[:, None, :], 0.0))
    xb = torch.clamp(raw, 0.0, 1e4) * mi
    tl, tt, tr, tb = (y[:, i:i + 1] for i in range(4))
    pl, pt, pr, pb = (xb[:, i:i + 1] for i in range(4))
    ta, pa = (tl + tr) * (tt + tb), (pl + pr) * (pt + pb)
    wi = torch.minimum(pl, tl) + torch.minimum(pr, tr)
    hi = torch.minimum(pb, tb) + torch.minimum(pt, tt)
    ai = wi * hi
    au = ta + pa - ai
    n_off = cm.sum() + 1e-30
    per = -torch.log((ai + 1.0) / (au + 1.0)) * cm
    off_loss = per.sum() / n_off
    off_loss.backward()
    d_off = raw.grad.numpy()
    with torch.no_grad():
        i1, u1 = ai + 1.0, au + 1.0
        t_area = (ta + pa + 2 * ai + 1.0)                       # the absolute values under U + 1 (and I + 1 <= it)
        T_off = torch.zeros_like(raw)
        for e in range(4):
            side, other = (wi, pl + pr) if e & 1 else (hi, pt + pb)
            # |other - d| / U1 and d / I1, each with the conditioning of its denominator
            T_off[:, e:e + 1] = ((other + side) / u1 * (t_area / u1) + side / i1 * (t_area / i1)) * cm * (mi != 0)
        T_off = T_off.numpy()
        t_per = ((torch.log(i1).abs() + torch.log(u1).abs() + t_area / i1 + t_area / u1) * cm).numpy()
    s = dict(s_cls=1.0 / norm, s_ctr=1.0 / nc, s_off=1.0 / float(n_off))
    T_losses = np.array([t_bce.sum() / nc, t_elem.sum() / norm, t_per.sum() / float(n_off)])
    return dict(losses=np.array([ctr_loss, cls_loss, float(off_loss.detach())]), d_cls=(g / norm).reshape(cls_logits.shape),
                d_ctr=d_ctr.reshape(ctr_logits.shape), d_off=d_off, T_cls=T_cls.reshape(cls_logits.shape),
                T_ctr=T_ctr.reshape(ctr_logits.shape), T_off=T_off, T_losses=T_losses, **s)


def k_of(got, truth, T, s):
    """max |got - truth| / (eps32 * T * s + s * tiny); where the scale is 0 the element must be the truth exactly"""
    got = np.asarray(got, np.float64)
    den = EPS32 * T * s + s * TINY32 * (T > 0)
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))
    return float(k.max()) if k.size else 0.0


def k_losses(got, truth):
    """the three scalars: a float32 sum of n terms of absolute sum T has error <= eps * T * O(log n) pairwise, O(n)
    sequentially; the scalars are measured in units of eps32 * T like everything else"""
    return float(np.max(np.abs(np.asarray(got, np.float64) - truth["losses"])
                        / (EPS32 * truth["T_losses"] + TINY32)))


# ---------------------------------------------------------------------------------------------- cases --
STRIDES = (8, 16, 32, 64, 128)


def _boxes(rs, N, M, w, h, K, pad_from):
    gt = np.full((N, M, 5), -1, F32)
    for n in range(N):
        m = M if pad_from is None else min(M, pad_from[n])
        if m == 0:
            continue
        x1 = rs.uniform(0, w * 0.8, m); y1 = rs.uniform(0, h * 0.8, m)
        bw = np.exp(rs.uniform(np.log(6), np.log(w), m)); bh = np.exp(rs.uniform(np.log(6), np.log(h), m))
        gt[n, :m, 0], gt[n, :m, 1] = np.round(x1 * 4) / 4, np.round(y1 * 4) / 4
        gt[n, :m, 2] = np.minimum(gt[n, :m, 0] + np.round(bw), w - 1)
        gt[n, :m, 3] = np.minimum(gt[n, :m, 1] + np.round(bh), h - 1)
        gt[n, :m, 4] = rs.randint(1, K + 1, m)
    return gt


# (image, location index, greatest offset, expected cls_id) of the "stage-bounds" case: levels begin at 0 / 96 / 120
# in the (64, 96) grid; stride 16 is 4 x 6, stride 32 is 2 x 3, stride 8 is 8 x 12
STAGE_BOUND_PROBES = ((0, 96 + 1 * 6 + 4, 64.0, 1), (0, 120 + 0 * 3 + 2, 128.0, 3), (1, 96 + 1 * 6 + 4, 128.0, 0),
                      (1, 3 * 12 + 5, 64.0, 0))


def target_cases():
    """(name, dict(gt_bbox, im_info, data_size, strides, K)): the named cases of the FCOS target tests"""
    rs = np.random.RandomState(20261)
    out = []

    def add(name, gt, im_info, data_size=(64, 96), K=3, strides=STRIDES):
        out.append((name, dict(gt_bbox=np.asarray(gt, F32), im_info=np.asarray(im_info, F32),
                               data_size=tuple(data_size), strides=tuple(strides), K=K)))
    full = [[64, 96, 1], [64, 96, 1]]
    for M, K in ((1, 3), (5, 80), (70, 3), (130, 80)):
        add("landscape-M%d-K%d" % (M, K), _boxes(rs, 2, M, 96, 64, K, (max(1, M - 2), max(1, M // 2))), full, K=K)
    # portrait: ori_h >= ori_w takes the transposed grid (data_size stays (short, long))
    add("portrait-M5", _boxes(rs, 2, 5, 64, 96, 3, None), [[96, 64, 1], [96, 64, 1]])
    add("portrait-72x40", _boxes(rs, 2, 5, 72, 40, 80, None), [[40, 36, 1], [40, 36, 1]], data_size=(72, 40), K=80)
    add("landscape-72x40", _boxes(rs, 2, 70, 40, 72, 3, (70, 9)), [[60, 65, 1], [72, 80, 1]], data_size=(72, 40))
    # image 0 smaller than data_size (its padding mask is applied to image 1 too), image 1 not
    add("pad-image0", _boxes(rs, 2, 5, 96, 64, 3, None), [[40, 70, 1], [64, 96, 1]])
    # the greatest offset exactly ON a bound of the location's own level (STAGE_BOUND_PROBES names the locations):
    #   image 0, stride-16 centre (72, 24): box 0 gives l = 72 - 8 = 64 = the level's INCLUSIVE lower bound -> class 1
    #            (box 2 is assigned there too, l = 120, but is larger);
    #   image 0, stride-32 centre (80, 16): box 2 gives l = 80 + 48 = 128 = its level's inclusive lower bound -> class 3;
    #   image 1, stride-16 centre (72, 24): box 0 gives l = 72 + 56 = 128 = the level's EXCLUSIVE upper bound -> background;
    #   image 1, stride-8 centre (44, 28): box 1 gives l = 44 + 20 = 64 = level 0's exclusive upper bound -> background.
    add("stage-bounds", [[[8, 0, 90, 60, 1], [-20, 0, 60, 60, 2], [-48, 0, 90, 60, 3]],
                         [[-56, 0, 90, 60, 2], [-20, 0, 60, 60, 1], [-1, -1, -1, -1, -1]]], full)
    # two identical boxes, and two different boxes of equal area: the lowest index wins
    add("ties", [[[8, 8, 40, 40, 1], [8, 8, 40, 40, 2], [0, 0, 0, 0, -1]],
                 [[8, 8, 40, 24, 3], [16, 4, 32, 36, 2], [8, 8, 40, 24, 1]]], full)
    # locations exactly on the box edges: x1 = 12 is a stride-8 centre column, y2 = 36 a centre row
    add("edge", [[[12, 4, 52, 36, 2]], [[12, 12, 12.5, 60, 1]]], full)
    # several workgroups per image (856 locations), a level boundary inside a workgroup
    add("multi-block", _boxes(rs, 2, 5, 256, 160, 3, None), [[150, 250, 1], [160, 256, 1]], data_size=(160, 256))
    add("padded-rows", _boxes(rs, 2, 5, 96, 64, 3, (2, 1)), full)
    add("no-box", _boxes(rs, 2, 5, 96, 64, 3, (3, 0)), full)
    # a degenerate box (x1 == x2 on a centre column): 0/0 = NaN centerness on its line
    add("degenerate", [[[20, 4, 20, 40, 1], [4, 4, 50, 50, 2]], [[4, 12, 60, 12, 3], [30, 30, 40, 40, 1]]], full)
    return out


def loss_inputs(rs, tg, hws, K):
    """logits per level for the targets tg: class logits around the FCOS prior, centerness logits N(0, 2), offset
    predictions exp(N(log target, 0.5)) with planted clip cases; asserts no pred == target tie and no NaN target"""
    N, HW = tg["centerness"].shape
    assert not np.isnan(tg["centerness"]).any() and not np.isnan(tg["offset"]).any()
    cls = (rs.standard_normal((N, K, HW)) * 2.0 - 4.6).astype(F32)
    flat = cls.reshape(-1)
    planted = F32([30, -30, 100, -100, 1e-4, -1e-4, 0])
    idx = rs.choice(flat.size, size=min(flat.size, 4 * planted.size), replace=False)
    flat[idx] = np.resize(planted, idx.size)
    ctr = (rs.standard_normal((N, 1, HW)) * 2.0).astype(F32)
    base = np.where(tg["offset"] > 0, tg["offset"], F32(8))
    off = (base * np.exp(rs.standard_normal((N, 4, HW)) * 0.5)).astype(F32)
    f = off.reshape(-1)
    f[rs.choice(f.size, 6, replace=False)] = F32([2e4, 1e4, 0, 1e-3, 3e4, 0.5])
    assert iou_ties(off, tg) == 0
    return cls, ctr, off


LOSS_CASES = (("landscape-M5-K80", 2.0, 0.25), ("landscape-M70-K3", 0.0, 0.25), ("pad-image0", 1.0, 0.5),
              ("landscape-72x40", 2.0, 0.25), ("multi-block", 1.5, 0.25))


def loss_cases():
    """(name, dict(case = the target case, tg = targets_f32 of it, cls / ctr / off in the concatenated form,
    hws, gamma, alpha)) for the target cases named in LOSS_CASES"""
    cases = dict(target_cases())
    rs = np.random.RandomState(20262)
    out = []
    for name, gamma, alpha in LOSS_CASES:
        c = cases[name]
        tg = targets_f32(c["gt_bbox"], c["im_info"], c["data_size"], c["strides"], c["K"])
        hws = [a * b for a, b in level_sizes(c["data_size"], c["strides"])]
        cls, ctr, off = loss_inputs(rs, tg, hws, c["K"])
        out.append(("%s-g%g" % (name, gamma), dict(case=c, tg=tg, cls=cls, ctr=ctr, off=off, hws=hws, gamma=gamma,
                                                   alpha=alpha)))
    return out
