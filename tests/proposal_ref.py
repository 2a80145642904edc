"""Numpy restatement of _contrib_Proposal_v2 (proposal_v2.cu:413-620) and _contrib_Proposal
(proposal.cu:417-614), the .cu forwards (the .cc files are not the spec).  float32 arithmetic in
the .cu's operation order without FMA, exp as float32(exp(float64)), so it is bit-exact against
the device op.

Per image: anchors (proposal_v2-inl.h GenerateAnchors, floor(x + 0.5f) rounding), row
i = (h*W + w)*A + a, BBoxPredKernel (:92-147, no dw/dh clamp) or IoUPredKernel (:155-195), the clip
to [0, im - 1], score -1 past the unpadded image, FilterBoxKernel (:201-222) on every row, the
top-`pre` of a stable descending sort over all rows, greedy NMS with IoU > thr (boxes scored -1
take part), PrepareOutput: v2 zero pads, v1 repeats the kept boxes when is_train.

NaN rule (the header's): a NaN score is ordered by its bits (sort_key); a NaN coordinate clips to
im - 1; a NaN side or area fails no filter test; a NaN IoU suppresses nothing."""
import numpy as np

f32 = np.float32


def anchors_v12(feature_stride, scales, ratios):
    """(A, 4) float32 in the order ratio-major, scale-minor (proposal_v2-inl.h:295-321)."""
    base = [f32(0), f32(0), f32(feature_stride - 1.0), f32(feature_stride - 1.0)]
    out = []
    for ratio in ratios:
        for scale in scales:
            scale, ratio = f32(scale), f32(ratio)
            w = base[2] - base[0] + f32(1)
            h = base[3] - base[1] + f32(1)
            x_ctr = f32(float(base[0]) + 0.5 * float(w - f32(1)))
            y_ctr = f32(float(base[1]) + 0.5 * float(h - f32(1)))
            size_ratios = np.floor((w * h) / ratio)
            new_w = np.floor(np.sqrt(size_ratios) + f32(0.5)) * scale
            new_h = np.floor((new_w / scale * ratio) + f32(0.5)) * scale
            out.append([x_ctr - f32(0.5) * (new_w - f32(1)), y_ctr - f32(0.5) * (new_h - f32(1)),
                        x_ctr + f32(0.5) * (new_w - f32(1)), y_ctr + f32(0.5) * (new_h - f32(1))])
    return np.asarray(out, f32)


def sort_key(score):
    """select_common.h ordered_desc_bits: ascending key = descending score; -0 == +0; NaNs by bits."""
    u = np.asarray(score, f32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    u = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    return (~u).astype(np.uint32)


def _clip(v, hi):
    m = np.where(v < hi, v, hi)          # fminr: a NaN coordinate becomes hi
    return np.where(m > f32(0), m, f32(0)).astype(f32)


def decode(cls_prob, bbox_pred, im_info, feature_stride=16, scales=(4., 8., 16., 32.),
           ratios=(0.5, 1., 2.), rpn_min_size=16, iou_loss=False, valid_range=None,
           filter_scales=False):
    """One image: cls_prob (2A,H,W), bbox_pred (4A,H,W), im_info (3,) -> boxes (count,4) and the
    filtered scores (count,) in row order.  valid_range: (2,) of this image (v2 only)."""
    A2, H, W = cls_prob.shape
    A = A2 // 2
    anc = anchors_v12(feature_stride, scales, ratios)
    hh, ww, aa = np.meshgrid(np.arange(H), np.arange(W), np.arange(A), indexing="ij")
    hh, ww, aa = hh.reshape(-1), ww.reshape(-1), aa.reshape(-1)
    x1 = anc[aa, 0] + (ww * feature_stride).astype(f32)
    y1 = anc[aa, 1] + (hh * feature_stride).astype(f32)
    x2 = anc[aa, 2] + (ww * feature_stride).astype(f32)
    y2 = anc[aa, 3] + (hh * feature_stride).astype(f32)
    d = bbox_pred.reshape(A, 4, H, W).astype(f32)
    dx, dy, dw, dh = (d[aa, j, hh, ww] for j in range(4))
    sc = cls_prob[A:].astype(f32)[aa, hh, ww].copy()
    im_h, im_w, im_s = (f32(v) for v in im_info)
    with np.errstate(all="ignore"):
        if iou_loss:
            px1, py1, px2, py2 = x1 + dx, y1 + dy, x2 + dw, y2 + dh
        else:
            width = x2 - x1 + f32(1)
            height = y2 - y1 + f32(1)
            ctr_x = x1 + f32(0.5) * (width - f32(1))
            ctr_y = y1 + f32(0.5) * (height - f32(1))
            pcx = dx * width + ctr_x
            pcy = dy * height + ctr_y
            pw = np.exp(dw.astype(np.float64)).astype(f32) * width
            ph = np.exp(dh.astype(np.float64)).astype(f32) * height
            px1 = pcx - f32(0.5) * (pw - f32(1))
            py1 = pcy - f32(0.5) * (ph - f32(1))
            px2 = pcx + f32(0.5) * (pw - f32(1))
            py2 = pcy + f32(0.5) * (ph - f32(1))
        boxes = np.stack([_clip(px1, im_w - f32(1)), _clip(py1, im_h - f32(1)),
                          _clip(px2, im_w - f32(1)), _clip(py2, im_h - f32(1))], 1)
        real_h = int(im_h / f32(feature_stride))
        real_w = int(im_w / f32(feature_stride))
        sc[(hh >= real_h) | (ww >= real_w)] = f32(-1)
        min_size = f32(rpn_min_size) * im_s
        iw = boxes[:, 2] - boxes[:, 0] + f32(1)
        ih = boxes[:, 3] - boxes[:, 1] + f32(1)
        small = (iw < min_size) | (ih < min_size)
        half = min_size / f32(2)
        boxes[small, 0:2] -= half
        boxes[small, 2:4] += half
        sc[small] = f32(-1)
        if filter_scales:
            vmin, vmax = f32(valid_range[0]), f32(valid_range[1])
            area = iw * ih
            sc[~small & ((area < vmin * vmin) | (area > vmax * vmax))] = f32(-1)
    return boxes.astype(f32), sc.astype(f32)


def topk(score, pre):
    """Rows of the first `pre` places of a stable descending sort (thrust greater<float>)."""
    return np.argsort(sort_key(score), kind="stable")[:pre]


def iou_row(b, boxes):
    """devIoU (proposal_v2.cu:276-284) of box b (the earlier, "cur" box) against boxes, fp32."""
    with np.errstate(all="ignore"):
        left = np.maximum(b[0], boxes[:, 0])
        right = np.minimum(b[2], boxes[:, 2])
        top = np.maximum(b[1], boxes[:, 1])
        bottom = np.minimum(b[3], boxes[:, 3])
        width = np.maximum(right - left + f32(1), f32(0))
        height = np.maximum(bottom - top + f32(1), f32(0))
        inter = width * height
        sa = (b[2] - b[0] + f32(1)) * (b[3] - b[1] + f32(1))
        sb = (boxes[:, 2] - boxes[:, 0] + f32(1)) * (boxes[:, 3] - boxes[:, 1] + f32(1))
        return (inter / (sa + sb - inter)).astype(f32)


def nms_keep(boxes, thr, limit, ge=False):
    """Greedy scan of the sorted boxes: the first `limit` kept positions (IoU > thr suppresses)."""
    n = len(boxes)
    removed = np.zeros(n, bool)
    keep = []
    thr = f32(thr)
    for i in range(n):
        if removed[i]:
            continue
        keep.append(i)
        if len(keep) >= limit:
            break
        iou = iou_row(boxes[i], boxes[i + 1:])
        removed[i + 1:] |= (iou >= thr) if ge else (iou > thr)
    return np.asarray(keep, np.int64)


def dims(count, pre, post, clamp=True):
    """clamp: v2 and v1 with is_train write at stride min(post, pre) and are refused past it; v1 in
    test mode keeps post (proposal.cu:453-455) and zero pads."""
    pre = pre if pre > 0 else count
    pre = min(pre, count)
    if clamp and post > pre:
        raise ValueError("rpn_post_nms_top_n > min(pre, count) is refused")
    return pre, post


def proposal_image(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
                   threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.), ratios=(0.5, 1., 2.),
                   feature_stride=16, iou_loss=False, valid_range=None, filter_scales=False,
                   cyclic=False, clamp=True):
    """One image -> out (post,4), score (post,), order (post,) source row or -1 (padding)."""
    boxes, sc = decode(cls_prob, bbox_pred, im_info, feature_stride, scales, ratios, rpn_min_size,
                       iou_loss, valid_range, filter_scales)
    pre, post = dims(len(sc), rpn_pre_nms_top_n, rpn_post_nms_top_n, clamp)
    order = topk(sc, pre)
    keep = nms_keep(boxes[order], threshold, post)
    rows = order[keep]
    out = np.zeros((post, 4), f32)
    score = np.zeros(post, f32)
    src = np.full(post, -1, np.int64)
    n = len(rows)
    out[:n], score[:n], src[:n] = boxes[rows], sc[rows], rows
    if cyclic and n < post:
        idx = np.arange(n, post) % n
        out[n:], score[n:], src[n:] = out[idx], score[idx], src[idx]
    return out, score, src


def proposal_v2(cls_prob, bbox_pred, im_info, valid_ranges, rpn_pre_nms_top_n=6000,
                rpn_post_nms_top_n=300, threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.),
                ratios=(0.5, 1., 2.), feature_stride=16, filter_scales=False, iou_loss=False):
    """Batch: (B,post,4), (B,post,1) like ops.proposal_v2."""
    res = [proposal_image(cls_prob[i], bbox_pred[i], im_info[i], rpn_pre_nms_top_n,
                          rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                          feature_stride, iou_loss, valid_ranges[i], filter_scales, False)
           for i in range(cls_prob.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])[..., None]


def proposal(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
             threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.), ratios=(0.5, 1., 2.),
             feature_stride=16, is_train=False, iou_loss=False):
    """Batch: (B,post,4), (B,post,1) like ops.proposal."""
    res = [proposal_image(cls_prob[i], bbox_pred[i], im_info[i], rpn_pre_nms_top_n,
                          rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                          feature_stride, iou_loss, None, False, bool(is_train), bool(is_train))
           for i in range(cls_prob.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])[..., None]


# ---- TridentNet inputs (config/tridentnet_r50v2c4_c5_2x.py: 3 branches, ranges on the original
#      image; models/tridentnet/builder.py:239-255) ----
TRIDENT = dict(feature_stride=16, scales=(2., 4., 8., 16., 32.), ratios=(0.5, 1., 2.),
               threshold=0.7, rpn_min_size=0)
TRIDENT_RANGES = ((0., 90.), (30., 160.), (90., 1e5))


def rpn_inputs(seed, B, A, H, W, im_hw=None, delta_scale=0.3, ties=0.0):
    """Softmax-like fg probabilities (B,2A,H,W), deltas (B,4A,H,W), im_info (B,3).
    ties: fraction of fg scores snapped to a few shared values."""
    rs = np.random.RandomState(seed)
    fg = rs.uniform(0.0, 1.0, (B, A, H, W)).astype(f32)
    if ties:
        m = rs.uniform(size=fg.shape) < ties
        fg[m] = rs.choice(np.asarray([0.5, 0.25, 0.125], f32), m.sum())
    cls = np.concatenate([f32(1) - fg, fg], 1).astype(f32)
    bbox = (rs.standard_normal((B, 4 * A, H, W)) * delta_scale).astype(f32)
    if im_hw is None:
        im_hw = (H * 16, W * 16)
    im = np.tile(np.asarray([[im_hw[0], im_hw[1], 1.0]], f32), (B, 1))
    return cls, bbox, im
