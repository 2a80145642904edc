"""TEST INFRASTRUCTURE: numpy restatements of the RepPoints training head (models/RepPoints/point_ops.py,
models/RepPoints/builder.py:311-484) and the cases the tests and tests/golden/make_golden_reppoints.py share.

  targets_f32   float32, one operation at a time, in the reference's order: _gen_points, _offset_to_boxes, _point_assign,
                _iou_assign.  Equal bit for bit to the fixture the reference's own functions wrote.
  losses_f32    float32 forward and the chain rule of the expressions as written (the device's specification).
  losses_truth  float64 forward and torch autograd on it, with the condition scales T of the house margin
                k = |got - truth| / (eps32 * T + tiny).

Pinned by the project, not by MXNet (its reduction order and its order among equal keys are not documented): the sums
over the points of a set run sequentially in point order; ties take the lower flat point index (selection per gt)
and the lower gt index (winner per point, arg-max).  box_iou is upstream's (not vendored): corner format, no +1,
extents clamped at 0, inter / (area_a + area_b - inter), 0 where the union is <= 0.
"""
import numpy as np

F32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
STRIDES = (8, 16, 32, 64, 128)
TRANSFORMS = {"minmax": 0, "partial_minmax": 1, "moment": 2}
INF = F32(np.inf)


def level_sizes(data_size, strides):
    """[(H_l, W_l)] of the FPN maps of an image h x w: ceil(h / stride), ceil(w / stride)"""
    h, w = data_size
    return [(-(-h // s), -(-w // s)) for s in strides]


def gen_points(sizes, strides):
    """_gen_points per level, concatenated: (P, 3) = (w * stride, h * stride, stride), (h, w) row-major"""
    out = []
    for (H, W), s in zip(sizes, strides):
        x = np.tile(np.arange(W, dtype=F32) * F32(s), H)
        y = np.repeat(np.arange(H, dtype=F32) * F32(s), W)
        out.append(np.stack([x, y, np.full(H * W, s, F32)], axis=-1))
    return np.concatenate(out).astype(F32)


def gen_offsets(dcn_kernel=3, dcn_pad=1):
    """_gen_offsets: the (y, x) base offsets of a deformable convolution, (1, 2 * kernel^2, 1, 1)"""
    base = np.arange(-dcn_pad, dcn_pad + 1, dtype=F32)
    return np.stack([np.repeat(base, dcn_kernel), np.tile(base, dcn_kernel)], axis=1).reshape(1, -1, 1, 1)


def split_yx(pred):
    """(N, 2K, H, W) with channels (y0, x0, y1, x1, ...) -> y, x of shape (N, H * W, K)"""
    N, C, H, W = pred.shape
    v = np.asarray(pred, F32).reshape(N, C // 2, 2, H * W)
    return np.ascontiguousarray(v[:, :, 0].transpose(0, 2, 1)), np.ascontiguousarray(v[:, :, 1].transpose(0, 2, 1))


def seq_sum(v):
    s = np.zeros(v.shape[:-1], v.dtype)
    for k in range(v.shape[-1]):
        s = s + v[..., k]
    return s


def moment(v, e):
    K = v.dtype.type(v.shape[-1])
    mean = seq_sum(v) / K
    d = v - mean[..., None]
    with np.errstate(all="ignore"):
        std = np.sqrt(seq_sum(d * d) / K)
    return mean, std, std * e


def points2bbox(x, y, transform, mt):
    """_points2bbox on x, y (..., K) -> (..., 4) [left, top, right, bottom]; mt = moment_transfer (2,)"""
    if transform == "moment":
        with np.errstate(all="ignore"):
            e = np.exp(np.asarray(mt, x.dtype))
        mx, _, hx = moment(x, e[0])
        my, _, hy = moment(y, e[1])
        return np.stack([mx - hx, my - hy, mx + hx, my + hy], axis=-1)
    if transform == "partial_minmax":
        x, y = x[..., :4], y[..., :4]
    elif transform != "minmax":
        raise NotImplementedError(transform)
    return np.stack([x.min(-1), y.min(-1), x.max(-1), y.max(-1)], axis=-1)


def init_boxes_f32(pts_levels, strides, transform, mt):
    """_offset_to_boxes per level, concatenated: (N, P, 4)"""
    out = []
    for pred, s in zip(pts_levels, strides):
        H, W = pred.shape[2:]
        c = gen_points([(H, W)], [s])
        y, x = split_yx(pred)
        b = points2bbox(x, y, transform, mt) * F32(s)
        out.append(np.concatenate([c[:, :2], c[:, :2]], axis=1)[None] + b)
    return np.concatenate(out, axis=1).astype(F32)


def gt_levels(gt, scale, lvl_min, lvl_max):
    """(centre x, centre y, w, h, level, the two logarithms) of gt rows (M, 5), float32"""
    l, t, r, b = (gt[:, i] for i in range(4))
    gx, gy = (l + r) / F32(2), (t + b) / F32(2)
    gw, gh = np.maximum(r - l, F32(1e-6)), np.maximum(b - t, F32(1e-6))
    lw, lh = np.log2(gw / F32(scale)), np.log2(gh / F32(scale))
    lvl = np.floor((lw + lh) / F32(2))
    return gx, gy, gw, gh, np.maximum(np.minimum(lvl, lvl_max), lvl_min), lw, lh


def point_assign_f32(points, gt, scale, num_pos):
    """_point_assign: points (P, 3), gt (M, 5) -> label (P,), box (P, 4)"""
    points, gt = np.asarray(points, F32), np.asarray(gt, F32)
    plvl = np.floor(np.log2(points[:, 2]))
    gx, gy, gw, gh, glvl, _, _ = gt_levels(gt, scale, plvl.min(), plvl.max())
    P = points.shape[0]
    best = np.full(P, INF, F32)
    arg = np.zeros(P, np.int64)
    for m in range(gt.shape[0]):
        if not gt[m, 4] > 0:
            continue
        idx = np.nonzero(plvl == glvl[m])[0]
        dx, dy = (points[idx, 0] - gx[m]) / gw[m], (points[idx, 1] - gy[m]) / gh[m]
        d = np.sqrt(dx * dx + dy * dy)
        keep = np.argsort(d, kind="stable")[:num_pos]              # ties: the lower flat point index
        j, dj = idx[keep], d[keep]
        upd = dj < best[j]                                         # ties: the lower gt index
        best[j[upd]], arg[j[upd]] = dj[upd], m
    hit = best < INF
    return (np.where(hit, gt[arg, 4], F32(-1)).astype(F32),
            np.where(hit[:, None], gt[arg, :4], F32(0)).astype(F32))


def box_iou(a, g):
    """upstream box_iou(format='corner'): a (P, 4), g (M, 4) -> (P, M)"""
    a, g = a[:, None, :], g[None, :, :]
    w = np.minimum(a[..., 2], g[..., 2]) - np.maximum(a[..., 0], g[..., 0])
    h = np.minimum(a[..., 3], g[..., 3]) - np.maximum(a[..., 1], g[..., 1])
    zero = a.dtype.type(0)
    i = np.where(w < 0, zero, w) * np.where(h < 0, zero, h)
    u = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])) - i
    with np.errstate(all="ignore"):
        return np.where(u <= 0, zero, i / np.where(u <= 0, a.dtype.type(1), u)).astype(a.dtype)


def iou_assign_f32(boxes, gt, pos_iou_thr, neg_iou_thr, min_pos_iou):
    """_iou_assign: boxes (P, 4), gt (M, 5) -> label (P,), box (P, 4), and the IoU matrix"""
    boxes, gt = np.asarray(boxes, F32), np.asarray(gt, F32)
    iou = box_iou(boxes, gt[:, :4])
    arg, mx, col = iou.argmax(1), iou.max(1), iou.max(0)
    a = np.full(boxes.shape[0], -1, F32)
    a = np.where(mx < F32(neg_iou_thr), F32(0), a)
    a = np.where(np.logical_and(iou == col[None], col[None] > F32(min_pos_iou)).any(1), F32(1), a)
    a = np.where(mx >= F32(pos_iou_thr), F32(1), a)
    return (np.where(a > 0, gt[arg, 4], a).astype(F32), np.where((a > 0)[:, None], gt[arg, :4], F32(0)).astype(F32), iou)


def targets_f32(c):
    """the four targets and the two counts of a case (see target_cases)"""
    sizes = [p.shape[2:] for p in c["pts_init"]]
    points = gen_points(sizes, c["strides"])
    boxes = init_boxes_f32(c["pts_init"], c["strides"], c["transform"], c["mt"])
    N = c["gt_bbox"].shape[0]
    li, gi, lr, gr = [], [], [], []
    for n in range(N):
        a, b = point_assign_f32(points, c["gt_bbox"][n], c["target_scale"], c["num_pos"])
        li.append(a), gi.append(b)
        a, b, _ = iou_assign_f32(boxes[n], c["gt_bbox"][n], c["pos_iou_thr"], c["neg_iou_thr"], c["min_pos_iou"])
        lr.append(a), gr.append(b)
    tg = dict(label_init=np.stack(li), gt_init=np.stack(gi), label_refine=np.stack(lr), gt_refine=np.stack(gr), boxes=boxes)
    tg["count"] = (int((tg["label_init"] >= 1).sum()), int((tg["label_refine"] >= 1).sum()))
    return tg


# ------------------------------------------------------------------------------------------ losses --
def _abs_points(pred, s, dt):
    """_offset_to_pts: x, y (N, HW, K) absolute, and the centres (HW,)"""
    H, W = pred.shape[2:]
    c = gen_points([(H, W)], [s]).astype(dt)
    y, x = split_yx(pred)
    x, y = x.astype(dt) * dt(s) + c[None, :, 0, None], y.astype(dt) * dt(s) + c[None, :, 1, None]
    return x, y


def smooth_l1(a, dt=F32):
    bsq = dt(9)
    ibsq = dt(1) / bsq
    return np.where(a > ibsq, a - dt(0.5) * ibsq, np.where(a < -ibsq, -a - dt(0.5) * ibsq, dt(0.5) * a * a * bsq))


def smooth_l1_grad(a, dt=F32):
    bsq = dt(9)
    ibsq = dt(1) / bsq
    return np.where(a > ibsq, dt(1), np.where(a < -ibsq, dt(-1), bsq * a))


def _moment_bwd(v, e, glo, ghi):
    K = F32(v.shape[-1])
    mean, std, _ = moment(v, e)
    with np.errstate(all="ignore"):
        dhalf = ghi - glo
        dmean0 = glo + ghi
        dstd = dhalf * e
        dv = dstd * (F32(0.5) / std)
        dq = dv / K
        d = dq[..., None] * (F32(2) * (v - mean[..., None]))
        dm = (dmean0 - seq_sum(d)) / K
        return (d + dm[..., None]).astype(F32), (dhalf * std).astype(F32)


def _minmax_bwd(v, lo, hi, glo, ghi, Q):
    d = np.where(v == lo[..., None], glo[..., None], F32(0)) + np.where(v == hi[..., None], ghi[..., None], F32(0))
    d[..., Q:] = 0
    return d.astype(F32)


def block_sum_f32(vals, T=256):
    """the device's fixed order: per workgroup of 256 values a butterfly per wave of 64 (xor 1, 2, the half-row and
    the row mirror, then the four rows left to right), then the four waves left to right"""
    v = np.zeros(-(-vals.size // T) * T, F32)
    v[:vals.size] = vals
    v = v.reshape(-1, 4, 4, 16)
    for perm in (np.arange(16) ^ 1, np.arange(16) ^ 2, (np.arange(16) & 8) | (7 - (np.arange(16) & 7)), 15 - np.arange(16)):
        v = v + v[..., perm]
    r = v[..., 0]
    w = (r[..., 0] + r[..., 1]) + (r[..., 2] + r[..., 3])
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def final_sum_f32(part, T=256):
    """one workgroup over the partials: thread t adds part[t], part[t + 256], ... then the block sum"""
    acc = np.zeros(T, F32)
    for b0 in range(0, part.size, T):
        chunk = part[b0:b0 + T]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    return block_sum_f32(acc)[0]


def losses_f32(c, tg, add_to=None):
    """float32 box losses of a case on the targets tg: loss_init / loss_refine (N, P, 4), d_init / d_refine (lists of
    level arrays shaped like the inputs), d_mt (2,).  add_to = (d_init, d_refine, d_mt) for req add."""
    tr, mt, strides = c["transform"], np.asarray(c["mt"], F32), c["strides"]
    N = c["gt_bbox"].shape[0]
    with np.errstate(all="ignore"):
        e = np.exp(mt) if tr == "moment" else np.ones(2, F32)
    den = [F32(tg["count"][0]) + F32(1), F32(tg["count"][1]) + F32(1)]
    gs = [F32(0.5), F32(1.0)]
    out = dict(d_mt=np.zeros(2, F32))
    P = tg["label_init"].shape[1]
    acc = np.zeros((4, N, P), F32)
    for st, (key, lab, gtb) in enumerate((("init", tg["label_init"], tg["gt_init"]), ("refine", tg["label_refine"], tg["gt_refine"]))):
        losses, grads, begin = [], [], 0
        for pred, s in zip(c["pts_" + key], strides):
            Nn, C, H, W = pred.shape
            hw, K = H * W, C // 2
            x, y = _abs_points(pred, s, F32)
            box = points2bbox(x, y, tr, mt)
            nt = F32(s) * F32(c["scale"])
            w = (lab[:, begin:begin + hw] > 0).astype(F32)[..., None]
            with np.errstate(all="ignore"):
                r = (box - gtb[:, begin:begin + hw]) / nt
                losses.append(smooth_l1(r) * w)
                g0 = gs[st] / den[st]
                gb = ((g0 * w) * smooth_l1_grad(r)) / nt
                if tr == "moment":
                    dx, ax = _moment_bwd(x, e[0], gb[..., 0], gb[..., 2])
                    dy, ay = _moment_bwd(y, e[1], gb[..., 1], gb[..., 3])
                    acc[2 * st, :, begin:begin + hw], acc[2 * st + 1, :, begin:begin + hw] = ax, ay
                else:
                    Q = 4 if tr == "partial_minmax" else K
                    dx = _minmax_bwd(x, box[..., 0], box[..., 2], gb[..., 0], gb[..., 2], Q)
                    dy = _minmax_bwd(y, box[..., 1], box[..., 3], gb[..., 1], gb[..., 3], Q)
                d = np.stack([dy * F32(s), dx * F32(s)], axis=-1)               # (N, hw, K, 2) -> channels (y, x)
            grads.append(np.ascontiguousarray(d.reshape(Nn, hw, C).transpose(0, 2, 1)).reshape(pred.shape).astype(F32))
            begin += hw
        out["loss_" + key] = np.concatenate(losses, axis=1).astype(F32)
        out["d_" + key] = grads
    if tr == "moment":
        s4 = [final_sum_f32(block_sum_f32(acc[i].reshape(-1))) for i in range(4)]
        with np.errstate(all="ignore"):
            out["d_mt"] = np.array([s4[0] * e[0] + s4[2] * e[0], s4[1] * e[1] + s4[3] * e[1]], F32)
    if add_to is not None:
        out["d_init"] = [a + b for a, b in zip(add_to[0], out["d_init"])]
        out["d_refine"] = [a + b for a, b in zip(add_to[1], out["d_refine"])]
        out["d_mt"] = add_to[2] + out["d_mt"]
    return out


def losses_truth(c, tg):
    """float64 forward on the float32 inputs and targets, torch autograd for the gradients; T_* are the condition
    scales of the margin: the absolute values a float32 evaluation of the expressions as written carries.
      X = max_k (|p_k| * stride + |centre|) bounds the absolute coordinates of a set; a mean, a difference from
      it, a deviation and a half extent each carry eps * X (times e = exp(moment_transfer) for the half extent);
      the residual carries (T_box + |gt|) / nt; smooth-L1 passes it on with |sl1'| and its gradient with 9 inside
      the quadratic zone; the moment backward divides by std, which turns eps * X into a relative X / std."""
    import torch
    D = np.float64
    tr, strides = c["transform"], c["strides"]
    mt = torch.tensor(np.asarray(c["mt"], F32).astype(D), requires_grad=True)
    e = torch.exp(mt) if tr == "moment" else torch.ones(2, dtype=torch.float64)
    en = e.detach().numpy()
    den = [D(tg["count"][0]) + 1.0, D(tg["count"][1]) + 1.0]
    gs = [0.5, 1.0]
    out, total, T_mt = {}, 0.0, np.zeros(2)
    leaves = {}
    for st, (key, lab, gtb) in enumerate((("init", tg["label_init"], tg["gt_init"]), ("refine", tg["label_refine"], tg["gt_refine"]))):
        losses, T_loss, T_grads, begin = [], [], [], 0
        leaves[key] = []
        for pred, s in zip(c["pts_" + key], strides):
            Nn, C, H, W = pred.shape
            hw, K = H * W, C // 2
            p = torch.tensor(np.asarray(pred, F32).astype(D), requires_grad=True)
            leaves[key].append(p)
            ctr = torch.tensor(gen_points([(H, W)], [s]).astype(D))
            v = p.reshape(Nn, K, 2, hw).permute(0, 3, 1, 2)               # (N, hw, K, (y, x))
            x, y = v[..., 1] * s + ctr[None, :, 0, None], v[..., 0] * s + ctr[None, :, 1, None]
            if tr == "moment":
                mx, my = x.mean(-1), y.mean(-1)
                sx, sy = torch.sqrt(((x - mx[..., None]) ** 2).mean(-1)), torch.sqrt(((y - my[..., None]) ** 2).mean(-1))
                box = torch.stack([mx - sx * e[0], my - sy * e[1], mx + sx * e[0], my + sy * e[1]], -1)
            else:
                xs, ys = (x[..., :4], y[..., :4]) if tr == "partial_minmax" else (x, y)
                box = torch.stack([xs.amin(-1), ys.amin(-1), xs.amax(-1), ys.amax(-1)], -1)
            nt = float(s) * float(c["scale"])
            w = torch.tensor((lab[:, begin:begin + hw] > 0).astype(D))[..., None]
            r = (box - torch.tensor(gtb[:, begin:begin + hw].astype(D))) / nt
            ar = r.abs()
            loss = torch.where(ar > 1.0 / 9, ar - 0.5 / 9, 0.5 * 9 * r * r) * w
            losses.append(loss.detach().numpy())
            total = total + (loss * (gs[st] / den[st])).sum()
            # ---- condition scales
            with torch.no_grad():
                xn, yn, rn, wn = x.numpy(), y.numpy(), r.numpy(), w.numpy()
                pn = np.abs(np.asarray(pred, F32).astype(D)).reshape(Nn, K, 2, hw).transpose(0, 3, 1, 2)
                cn = np.abs(ctr.numpy())
                X = [(pn[..., 1] * s + cn[None, :, 0, None]).max(-1), (pn[..., 0] * s + cn[None, :, 1, None]).max(-1)]
                ee = en if tr == "moment" else np.zeros(2)
                Tb = np.stack([X[0] * (1 + ee[0]), X[1] * (1 + ee[1])] * 2, -1)          # (N, hw, 4)
                slope = np.where(np.abs(rn) > 1.0 / 9, 1.0, 9 * np.abs(rn))
                quad = (np.abs(rn) <= 1.0 / 9).astype(D)
                Tr = (Tb + np.abs(gtb[:, begin:begin + hw].astype(D))) / nt
                T_loss.append((np.abs(losses[-1]) + slope * Tr) * wn)
                G = (gs[st] / den[st]) * wn * (slope + 9 * quad * Tr) / nt                 # |d box| with its error
                Tg = np.zeros((Nn, hw, K, 2))
                for ax, (vals, col) in enumerate(((xn, 1), (yn, 0))):
                    Gs = G[..., ax] + G[..., ax + 2]
                    if tr == "moment":
                        mean = vals.mean(-1, keepdims=True)
                        std = np.sqrt(((vals - mean) ** 2).mean(-1))
                        with np.errstate(all="ignore"):
                            dqa = Gs * en[ax] * 0.5 / std / K
                            t = dqa[..., None] * 2 * (X[ax][..., None] + np.abs(vals - mean) * (1 + (X[ax] / std)[..., None]))
                        t = np.where(Gs[..., None] > 0, t, 0.0)
                        Tg[..., col] = s * (t + (Gs[..., None] + t.sum(-1, keepdims=True)) / K)
                        T_mt[ax] += float((Gs * en[ax] * (std + X[ax])).sum())
                    else:
                        Tg[..., col] = s * Gs[..., None]
                T_grads.append(np.ascontiguousarray(Tg.reshape(Nn, hw, C).transpose(0, 2, 1)).reshape(pred.shape))
            begin += hw
        out["loss_" + key] = np.concatenate(losses, axis=1)
        out["T_loss_" + key] = np.concatenate(T_loss, axis=1)
        out["T_d_" + key] = T_grads
    if total.requires_grad:
        total.backward()
    for key in ("init", "refine"):
        out["d_" + key] = [np.zeros(p.shape) if p.grad is None else p.grad.numpy() for p in leaves[key]]
    out["d_mt"] = np.zeros(2) if mt.grad is None else mt.grad.numpy()
    out["T_d_mt"] = T_mt
    return out


def k_of(got, truth, T):
    """max |got - truth| / (eps32 * T + tiny); where the scale is 0 the element must be the truth exactly"""
    got, truth, T = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.asarray(T, np.float64)
    den = EPS32 * T + TINY32 * (T > 0)
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        k = np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))
    return float(k.max()) if k.size else 0.0


def k_all(res, truth):
    """(k of the forward values, k of the gradient elements, k of d_moment_transfer)"""
    kf = max(k_of(res["loss_" + s], truth["loss_" + s], truth["T_loss_" + s]) for s in ("init", "refine"))
    kg = max(k_of(a, b, t) for s in ("init", "refine") for a, b, t in zip(res["d_" + s], truth["d_" + s], truth["T_d_" + s]))
    return kf, kg, k_of(res["d_mt"], truth["d_mt"], truth["T_d_mt"])


# ---------------------------------------------------------------------------------------------- cases --
def _boxes(rs, N, M, size, valid, K=80, lo=6.0):
    """random gt rows inside an image size = (h, w); rows from valid[n] on are the reference's padding, -1"""
    h, w = size
    gt = np.full((N, M, 5), -1, F32)
    for n in range(N):
        for m in range(min(M, valid[n])):
            bw, bh = np.exp(rs.uniform(np.log(lo), np.log(w))), np.exp(rs.uniform(np.log(lo), np.log(h)))
            x1, y1 = rs.uniform(-4, max(w - bw, 1)), rs.uniform(-4, max(h - bh, 1))
            gt[n, m] = [x1, y1, x1 + bw, y1 + bh, rs.randint(1, K + 1)]
    return np.round(gt * 4) / 4           # quarter pixels: sums and differences stay exact


def _pts(rs, N, K, sizes, spread=1.5):
    return [(rs.standard_normal((N, 2 * K, H, W)) * spread).astype(F32) for H, W in sizes]


def _case(seed, size=(64, 96), N=2, M=8, valid=(5, 3), K=9, transform="moment", mt=(0.0, 0.0), strides=STRIDES,
          num_pos=1, pos=0.5, neg=0.5, minpos=0.0, target_scale=4, scale=4, gt=None, pts=None, refine=False):
    rs = np.random.RandomState(seed)
    sizes = level_sizes(size, strides)
    c = dict(size=size, strides=tuple(strides), transform=transform, mt=np.asarray(mt, F32), num_points=K,
             target_scale=target_scale, num_pos=num_pos, pos_iou_thr=pos, neg_iou_thr=neg, min_pos_iou=minpos, scale=scale)
    c["gt_bbox"] = _boxes(rs, N, M, size, valid) if gt is None else np.asarray(gt, F32)
    c["pts_init"] = _pts(rs, c["gt_bbox"].shape[0], K, sizes) if pts is None else pts
    if refine:
        c["pts_refine"] = [p + (rs.standard_normal(p.shape) * 0.5).astype(F32) for p in c["pts_init"]]
    return c


def _pad(rows, M):
    return np.array([list(r) for r in rows] + [[-1] * 5] * (M - len(rows)), F32)


def _set_box(pts, n, h, w, lo, hi):
    """make the nine offsets of location (h, w) of a level map span [lo, hi] in x and in y (raw offsets)"""
    for k in range(pts.shape[1] // 2):
        v = lo if k % 2 == 0 else hi
        pts[n, 2 * k, h, w] = pts[n, 2 * k + 1, h, w] = v


def target_cases():
    """[(name, case)]: every branch of both assigners (the issue's list)"""
    out = [("moment", _case(1)), ("minmax", _case(2, transform="minmax")),
           ("partial_minmax", _case(3, transform="partial_minmax")),
           ("num-pos-3", _case(4, num_pos=3)),
           # sixteen per gt: more than the 6, 2 and 1 points of the upper levels hold
           ("num-pos-16-larger-than-a-level", _case(5, num_pos=16, M=8, valid=(8, 6))),
           ("m1", _case(6, N=1, M=1, valid=(1,))), ("m100", _case(7, M=100, valid=(60, 17), transform="minmax")),
           ("no-valid-gt", _case(8, valid=(0, 4))),
           ("band", _case(9, pos=0.6, neg=0.3)),                                   # -1 appears between the thresholds
           ("min-pos-iou", _case(10, pos=0.6, neg=0.3, minpos=0.2)),
           ("two-workgroups", _case(11, size=(320, 416), N=1, M=8, valid=(8,), num_pos=3)),
           ("one-level", _case(12, strides=(16,), size=(64, 96))),
           ("25-points", _case(13, K=25, N=1, valid=(4,))), ("1-point", _case(14, K=1, N=1, valid=(4,), transform="minmax"))]
    # levels: a 2 x 2 and a 5000 x 5000 gt clip at both ends; 64 x 64, 32 x 128, 128 x 128, 512 x 512 are exact powers of two
    gt = np.stack([_pad([[10, 10, 12, 12, 1], [-1, -1, 4999, 4999, 2], [0, 0, 64, 64, 3], [16, 8, 48, 136, 4],
                         [0, 0, 128, 128, 5], [0, 0, 512, 512, 6], [0, 0, 32, 32, 7], [0, 0, 16, 16, 8]], 8)] * 2)
    out.append(("levels-clip-and-powers-of-two", _case(15, gt=gt, num_pos=3)))
    # duplicates (the lower gt index wins the point) and a centre between four grid points of its level
    # (the lower flat index wins the selection): 32 x 32 is level 3, centre (4, 4) lies between (0, 0) .. (8, 8)
    gt = np.stack([_pad([[20, 12, 52, 44, 5], [20, 12, 52, 44, 9], [-12, -12, 20, 20, 3], [28, 28, 92, 92, 4],
                         [28, 28, 92, 92, 2]], 8)] * 2)
    out.append(("duplicates-and-centre-ties", _case(16, gt=gt, num_pos=1)))
    out.append(("duplicates-and-centre-ties-3", _case(16, gt=gt, num_pos=3)))
    # constructed boxes: every set is nine coincident points (a degenerate box, union 0 against padding) except ...
    sizes = level_sizes((64, 96), STRIDES)
    pts = [np.zeros((2, 18, H, W), F32) for H, W in sizes]
    _set_box(pts[0], 0, 0, 0, 0.0, 2.0)           # image 0, stride 8, (0, 0): [0, 0, 16, 16]
    _set_box(pts[0], 1, 0, 0, 0.0, 2.0)           # image 1: the same box and [64, 32, 80, 48]
    _set_box(pts[0], 1, 4, 8, 0.0, 2.0)
    # image 0: [0, 0, 16, 16] is the best box of gt 1 (IoU 64 / 1216) while its own arg-max is gt 0 (IoU 1)
    # image 1: IoU exactly 0.5 (= pos_iou_thr) and exactly 0.25 (= neg_iou_thr = min_pos_iou)
    gt = np.stack([_pad([[0, 0, 16, 16, 7], [8, 8, 40, 40, 3], [60, 40, 90, 60, 5]], 8),
                   _pad([[0, 0, 16, 32, 4], [64, 32, 96, 64, 6]], 8)])
    out.append(("max-fg-quirk-threshold-equality-degenerate", _case(17, gt=gt, pts=pts, transform="minmax", pos=0.5,
                                                                    neg=0.25, minpos=0.25)))
    return out


def margin_target_case():
    """a non-zero moment_transfer: exp differs between libraries by an ulp, so the fixture script ASSERTS that every
    IoU is at least 1e-3 from both thresholds and every column maximum unique by 1e-3; labels are then equal"""
    return "moment-transfer", _case(44, mt=(0.3, -0.2), pos=0.5, neg=0.4)


def loss_cases():
    """[(name, case)] with pts_refine; the targets come from targets_f32"""
    return [("moment", _case(31, refine=True, mt=(0.25, -0.125), num_pos=3)),
            ("minmax", _case(32, refine=True, transform="minmax", num_pos=3)),
            ("partial_minmax", _case(33, refine=True, transform="partial_minmax", N=1, valid=(6,), num_pos=3)),
            ("moment-m100-two-workgroups", _case(34, refine=True, size=(320, 416), N=1, M=100, valid=(40,), num_pos=3)),
            ("moment-one-level", _case(35, refine=True, strides=(8,), size=(64, 96), num_pos=16))]


def exact_loss_cases():
    """cases whose device results equal losses_f32 exactly"""
    rs = np.random.RandomState(41)
    sizes = level_sizes((64, 96), STRIDES)
    tied = [rs.randint(-2, 3, (2, 18, H, W)).astype(F32) for H, W in sizes]          # small integers: min and max tie
    tied_r = [rs.randint(-2, 3, (2, 18, H, W)).astype(F32) for H, W in sizes]
    c1 = _case(42, transform="minmax", pts=tied, num_pos=3)
    c1["pts_refine"] = tied_r
    co = _case(43, refine=True, num_pos=3)
    for key in ("pts_init", "pts_refine"):
        co[key] = [p.copy() for p in co[key]]
        co[key][0][0, :, 2, 3] = 0.75                  # nine coincident points at one location of image 0
    cz = _case(44, refine=True, valid=(0, 0))
    return [("tied-minmax", c1), ("coincident-points", co), ("all-weights-zero", cz)]
