"""The FreeAnchor training head restated in plain torch, line by line after models/FreeAnchor/builder.py:67-148 and
ops.py:44-210, with the three upstream pieces as DESIGN 4.26 fixes them: box_iou in corner format (no +1, extents
clamped at 0, 0 where the union is <= 0), decode_bbox as decodebbox.cc's class-agnostic xyxy form, topk as a stable
descending sort (the lower index first among equals).  MXNet's conventions at kinks: maximum passes the gradient to its
left operand when it is >=, clip on the closed interval.  evaluate(case, torch.float64) is the truth with the condition
scales T of k = |got - truth| / (eps32 * T + tiny); evaluate(case, torch.float32) is the restatement whose own k is k_ref.
"""
import math

import numpy as np
import torch

EPS32 = float(np.finfo(np.float32).eps)
TINY32 = float(np.finfo(np.float32).tiny)
SIGMA = np.float32(math.sqrt(1 / 0.11))
BSQ = float(SIGMA * SIGMA)                       # squared in float, as mshadow's smooth_l1 does
IBSQ = float(np.float32(1) / np.float32(BSQ))
SIZES = ((4, 4), (3, 6), (6, 3), (5, 5), (4, 7), (7, 4), (6, 6), (4, 9), (9, 4))   # A = 9 anchors, (w, h) in strides


def make_anchors(stride, S):
    """(1, 1, S, S, 36) like the loader's: every coordinate a dyadic number, so mirrored anchors tie exactly"""
    c = np.arange(S, dtype=np.float64) * stride + (stride - 1) / 2
    out = np.zeros((S, S, len(SIZES), 4))
    for a, (w, h) in enumerate(SIZES):
        hw, hh = (w * stride - 1) / 2, (h * stride - 1) / 2
        out[:, :, a] = np.stack(np.broadcast_arrays(c[None] - hw, c[:, None] - hh, c[None] + hw, c[:, None] + hh), -1)
    return out.reshape(1, 1, S, S, -1).astype(np.float32)


def _maximum(a, b):
    return torch.where(a >= b, a, torch.as_tensor(b, dtype=a.dtype).expand_as(a))


def box_iou(a, g):
    a, g = a[:, None, :], g[None, :, :]
    zero = torch.zeros((), dtype=a.dtype)
    w = torch.minimum(a[..., 2], g[..., 2]) - torch.maximum(a[..., 0], g[..., 0])
    h = torch.minimum(a[..., 3], g[..., 3]) - torch.maximum(a[..., 1], g[..., 1])
    i = torch.where(w < 0, zero, w) * torch.where(h < 0, zero, h)
    u = ((a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1]) + (g[..., 2] - g[..., 0]) * (g[..., 3] - g[..., 1])) - i
    return torch.where(u <= 0, zero, i / torch.where(u <= 0, torch.ones_like(u), u))


def decode_bbox(anchors, deltas, im_info, mean, std):
    width, height = anchors[..., 2] - anchors[..., 0] + 1, anchors[..., 3] - anchors[..., 1] + 1
    size = (width, height, width, height)
    out = []
    for j in range(4):
        v = anchors[..., j] + (deltas[..., j] * std[j] + mean[j]) * size[j]
        m = (im_info[:, 1 - j % 2] - 1)[:, None]
        out.append(torch.clamp(torch.minimum(v, m.expand_as(v)), min=0))
    return torch.stack(out, -1)


def _smooth_l1(v):
    return torch.where(v > IBSQ, v - 0.5 * IBSQ, torch.where(v < -IBSQ, -v - 0.5 * IBSQ, 0.5 * v * v * BSQ))


def _bbox_encode(ex, gt, mean, std):
    ew, eh = ex[..., 2] - ex[..., 0] + 1, ex[..., 3] - ex[..., 1] + 1
    ecx, ecy = ex[..., 0] + 0.5 * (ew - 1), ex[..., 1] + 0.5 * (eh - 1)
    gw, gh = gt[..., 2] - gt[..., 0] + 1, gt[..., 3] - gt[..., 1] + 1
    gcx, gcy = gt[..., 0] + 0.5 * (gw - 1), gt[..., 1] + 0.5 * (gh - 1)
    t = [(gcx - ecx) / (ew + 1e-14), (gcy - ecy) / (eh + 1e-14), torch.log(gw / ew), torch.log(gh / eh)]
    return torch.stack([(t[j] - mean[j]) / std[j] for j in range(4)], -1)


def forward(case, cls, delta, dtype):
    """(per-gt positive terms (N, M), negative loss, bags (N, M, top_n), iou (N, M, anchors), gt_pred_prob)"""
    N, K, top_n, mean, std = case["N"], case["K"], case["top_n"], case["mean"], case["std"]
    thr = float(np.float32(case["bbox_thr"]))
    gt = torch.from_numpy(case["gt"]).to(dtype)
    im_info = torch.from_numpy(case["im_info"]).to(dtype)
    # builder.py:86-113: (N, A*C, H, W) -> (N, A*C, HW) -> concat -> transpose -> (N, HW*A, C)
    cat = lambda ts, c: torch.cat([t.reshape(N, t.shape[1], -1) for t in ts], 2).transpose(1, 2).reshape(N, -1, c)
    cls_prob, deltas = torch.sigmoid(cat(cls, K)), cat(delta, 4)
    anchors = torch.cat([torch.from_numpy(a)[:, :, :t.shape[2], :t.shape[3]].reshape(1, -1, 4)
                         for a, t in zip(case["anchors"], cls)], 1).to(dtype).expand(N, -1, 4)
    labels, boxes = gt[..., 4], gt[..., :4]
    nvalid = max(int((labels > 0).sum()), 1)
    # ---- _positive_loss
    iou = torch.stack([box_iou(boxes[n], anchors[n]) for n in range(N)])
    bags = torch.sort(-iou, dim=2, stable=True).indices[..., :top_n]                      # (N, M, top_n)
    bi = torch.arange(N)[:, None, None].expand_as(bags)
    ci = torch.clamp(labels - 1, min=0).long()[..., None].expand_as(bags)
    p, d, ex = cls_prob[bi, bags, ci], deltas[bi, bags], anchors[bi, bags]
    target = _bbox_encode(ex, boxes[:, :, None, :].expand_as(ex), mean, std)
    q = p * torch.exp(-(_smooth_l1(d - target) * 0.75).sum(-1))
    q = torch.where((labels > 0)[..., None].expand_as(q), q, torch.ones_like(q))
    w = 1.0 / _maximum(1.0 - q, 1e-12)
    bag_prob = ((w / w.sum(-1, keepdim=True)) * q).sum(-1)
    pos = -case["alpha"] * torch.log(torch.clamp(bag_prob, 1e-12, 1.0)) / nvalid
    # ---- _negative_loss
    pred = decode_bbox(anchors, deltas.detach(), im_info, mean, std)
    iou2 = torch.stack([box_iou(boxes[n], pred[n]) for n in range(N)])
    t2 = _maximum(iou2.max(2, keepdim=True).values, thr + 1e-12)
    gpp = torch.clamp((iou2 - thr) / (t2 - thr), 0.0, 1.0)
    arg = torch.sort(-gpp, dim=1, stable=True).indices[:, 0]                              # the first arg-max
    lab = torch.gather(labels, 1, arg)
    box_prob = torch.nn.functional.one_hot(torch.clamp(lab - 1, min=0).long(), K).to(dtype) * \
        ((lab > 0) & (lab <= K)).to(dtype)[..., None] * gpp.max(1).values[..., None]
    prob = cls_prob * (1.0 - box_prob)
    prob = torch.where((lab > 0)[..., None].expand_as(prob), prob, torch.zeros_like(prob))
    neg = (1.0 - case["alpha"]) * (-prob ** case["gamma"] * torch.log(torch.clamp(1.0 - prob, 1e-12, 1.0)))
    neg = neg / max(nvalid * top_n, 1)
    return pos, neg, bags, iou, gpp


def evaluate(case, dtype):
    """losses and gradients (grad_scale = case["grad_scale"]) in `dtype`; float64 adds the scales T: the sum of the
    magnitudes of a loss's terms, and per gradient element of its per-gt positive parts and its negative part"""
    cls = [torch.from_numpy(t).to(dtype).requires_grad_() for t in case["cls"]]
    delta = [torch.from_numpy(t).to(dtype).requires_grad_() for t in case["delta"]]
    pos, neg, bags, iou, gpp = forward(case, cls, delta, dtype)
    leaves, gs = cls + delta, case["grad_scale"]
    out = dict(pos=pos.sum().item(), neg=neg.sum().item(), bags=bags.numpy().astype(np.int32), iou=iou.detach().numpy(),
               gpp=gpp.detach().numpy(), valid=case["gt"][..., 4] > 0)
    grads = torch.autograd.grad(pos.sum() + neg.sum(), leaves, retain_graph=True)
    out["grads"] = [(g * gs).numpy() for g in grads]
    if dtype == torch.float64:
        out["T_pos"], out["T_neg"] = pos.abs().sum().item(), neg.abs().sum().item()
        T = [g.abs() for g in torch.autograd.grad(neg.sum(), cls, retain_graph=True)] + [torch.zeros_like(d) for d in delta]
        for term in pos.flatten()[torch.from_numpy(out["valid"].flatten())]:
            for t, g in zip(T, torch.autograd.grad(term, leaves, retain_graph=True)):
                t += g.abs()
        out["T_grads"] = [(t * abs(gs)).numpy() for t in T]
    return out


def k_of(got, truth, T):
    """k per element; where the scale is 0 the element must be the truth exactly"""
    got, truth, T = np.asarray(got, np.float64), np.asarray(truth, np.float64), np.asarray(T, np.float64)
    den = EPS32 * T + TINY32 * (T > 0)
    err = np.abs(got - truth)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, err / den, np.where(err == 0, 0.0, np.inf))


def k_all(res, truth, case):
    """(k of the two losses, max k of the regular gradient elements, k of each of the others).  The others are the
    logits whose float32 sigmoid p or 1 - p rounds to 1 (the +-30 of the kinks cases): float32 itself is off by 1 / eps32
    there, so they are held element by element and kept out of the maximum the regular ones are held to."""
    kl = max(k_of(res["pos"], truth["pos"], truth["T_pos"]), k_of(res["neg"], truth["neg"], truth["T_neg"]))
    ks = [k_of(a, b, t).ravel() for a, b, t in zip(res["grads"], truth["grads"], truth["T_grads"])]
    p = [np.float32(1) / (np.float32(1) + np.exp(-x)) for x in case["cls"]]
    reg = [((q < 1) & (np.float32(1) - q < 1)).ravel() for q in p] + [np.ones(d.size, bool) for d in case["delta"]]
    return float(kl), max(float(k[m].max()) for k, m in zip(ks, reg)), np.concatenate([k[~m] for k, m in zip(ks, reg)])


def prunes(iou, top_n, trip=512, cap=1024):
    """how often the bag kernel's list of `cap` keys is cut to top_n while it streams one gt's IoUs, `trip` per step:
    a condition on the `prune` case's input only.  trip and cap are csrc/free_anchor.hip's kFaUn * kFaT and kFaCap and
    go stale when those change (a note there points here)."""
    count, thr, n, kept = 0, -1.0, 0, []
    for base in range(0, len(iou), trip):
        if count + trip > cap:
            kept = sorted(kept, reverse=True)[:top_n]
            thr, count, n = kept[-1], top_n, n + 1
        new = [v for v in iou[base:base + trip] if v > thr]
        kept, count = kept + new, count + len(new)
    return n


# ---------------------------------------------------------------------------------------------- cases --
def _near(rs, stride, y, x, a, label):
    """a gt row near anchor a of location (y, x) of a level: the anchor, each edge moved by up to 12 % of its size"""
    b = make_anchors(stride, max(y, x) + 1)[0, 0, y, x, 4 * a:4 * a + 4].astype(np.float64)
    size = np.array([b[2] - b[0], b[3] - b[1]] * 2)
    return list(b + rs.uniform(-0.12, 0.12, 4) * size) + [label]


PAD = [-1.0] * 5
FAR = [500.0, 500.0, 520.0, 520.0, 1.0]          # outside every anchor: all IoUs 0, the lowest indices win


def make_case(name, seed=0):
    rs = np.random.RandomState(seed + sum(map(ord, name)))
    image, K, top_n, gamma = (64, 96), 3, 5, 2.0
    near = lambda *a: _near(rs, *a)
    if name == "small":      # the padding row last in image 0 and FIRST in image 1: all-zero anchors there do not count
        gts = [[near(8, 3, 4, 0, 1), near(8, 5, 9, 4, 3), near(16, 1, 2, 2, 2), PAD],
               [PAD, near(8, 2, 7, 7, 2), near(16, 2, 4, 1, 1), near(8, 6, 2, 5, 3)]]
    elif name == "prune":    # 3,600 anchors against a list of 1,024 keys; row 0 is a band along the bottom, so the
        image, top_n = (128, 160), 50   # IoUs rise with the index and the list fills again and again
        gts = [[[0.3, 90.2, 158.6, 126.7, 1.0], near(16, 4, 5, 0, 2), near(8, 12, 15, 8, 3)]]
    elif name == "lds128":   # M * top_n = 10,240 entries: the sparse backward sorts 16,384 keys in 128 KB of LDS
        top_n = 40
        gts = [[near(8, 3, 4, 0, 1), near(8, 5, 9, 4, 3), near(16, 1, 2, 2, 2)] + [PAD] * 253]
    elif name == "ties":     # a square gt on the centre of location (3, 5) of stride 8: mirrored anchors tie exactly
        gts = [[FAR, [43.5 - 19.5, 27.5 - 19.5, 43.5 + 19.5, 27.5 + 19.5, 2.0]]]
    elif name == "shared":   # two gts of one label nearly on each other, a third label on the same spot
        g = near(8, 4, 6, 3, 1)
        gts = [[g, [g[0] + 0.7, g[1] - 0.4, g[2] + 0.9, g[3] + 0.5, 1.0], [g[0] - 1.1, g[1] + 0.6, g[2] + 0.3, g[3] - 0.8, 3.0]]]
    elif name == "row0":     # image 0: row 0 valid, most anchors below thr everywhere; image 1: no valid gt at all
        gts = [[near(8, 3, 3, 0, 2), near(16, 2, 3, 4, 1)], [PAD, PAD]]
    elif name.startswith("kinks"):
        gamma = float(name[5:])
        gts = [[near(8, 3, 4, 0, 1), near(16, 1, 3, 2, 2)]]
    N = len(gts)
    shapes = [(image[0] // s, image[1] // s) for s in (8, 16)]
    c = dict(N=N, K=K, top_n=top_n, gamma=gamma, alpha=0.5, bbox_thr=0.6, mean=(0.0, 0.0, 0.0, 0.0),
             std=(0.1, 0.1, 0.2, 0.2), grad_scale=128.0, gt=np.array(gts, np.float32),
             im_info=np.array([[image[0], image[1], 1.0]] * N, np.float32),
             anchors=[make_anchors(s, w + 1 + i) for i, (s, (h, w)) in enumerate(zip((8, 16), shapes))],
             cls=[(rs.standard_normal((N, 9 * K, h, w)) - 2).astype(np.float32) for h, w in shapes],
             delta=[rs.standard_normal((N, 36, h, w)).astype(np.float32) for h, w in shapes])
    if name.startswith("kinks"):   # 1 - prob under 1e-12 and p * (1 - p) = 0 on whole rows of both levels
        for t in c["cls"]:
            t[:, :, 1] = 30.0
            t[:, :, 2] = -30.0
    truth = evaluate(c, torch.float64)
    c["truth"], c["ref"] = truth, evaluate(c, torch.float32)
    # a fair demand on the discrete outputs.  Among the top_n + 1 best IoUs of a valid gt no two are closer than 1e-5
    # unless they are equal: mirrored anchors (`ties`), or anchors of one area that both contain the gt or lie in it
    # (the same intersection and union) -- equal in any precision, and float32's bags are float64's.  No anchor's two
    # best gt_pred_prob are closer than 1e-5 unless both are 0 -- or, in `shared` alone, both the clip's exact 1: the
    # nearly coincident gts have the same best box, and float32 puts its ones where float64 does.
    top = -np.sort(-truth["iou"], axis=2)[..., :top_n + 1]
    gap = np.abs(np.diff(top, axis=2))[truth["valid"]]
    assert np.all((gap > 1e-5) | (gap == 0)), name
    assert np.array_equal(c["ref"]["bags"][truth["valid"]], truth["bags"][truth["valid"]]), name
    two = -np.sort(-truth["gpp"], axis=1)[:, :2]
    assert np.all((two[:, 0] - two[:, 1] > 1e-5) | (two[:, 0] == 0) | ((two[:, 1] == 1) & (name == "shared"))), name
    assert np.array_equal(c["ref"]["gpp"] == 1, truth["gpp"] == 1), name
    if name == "prune":
        assert prunes(truth["iou"][0, 0], top_n) >= 3
    return c
