"""numpy float32 statement of the hard NMS and of BboxPostProcessing WITH THE DEVICE'S TIE RULE, for the
inputs where the reference's own Python cannot serve (equal scores: its order is numpy's unstable sort).
tests/test_bbox_post.py first shows that it equals the reference-run fixture on every case (distinct
scores), which is what licenses its use for ties, NaNs and fuzzing.

Rules (include/simpledet_ops.h, sd_hard_nms_batched / sd_bbox_post_processing):
  * every operation of the overlap is a float32 operation; box j survives a kept box i iff
    ovr <= float32(thresh) -- a NaN ovr suppresses; max / min hand a NaN on;
  * boxes are visited by descending score, among equal scores the later row first, NaN scores before
    every number: the reverse of a stable ascending sort;
  * the operator drops column 0, keeps `score > min_det_score` per class (NaN fails), stacks the classes'
    kept rows in class order and takes the max_det best of the stack by the same order rule."""
import numpy as np

F = np.float32


def visit_order(scores):
    return np.argsort(np.asarray(scores, F), kind="stable")[::-1]


def hard_nms(dets, thresh):
    """dets (n,5) float32 -> kept row indices in visiting order."""
    dets = np.asarray(dets, F)
    n = len(dets)
    if n == 0:
        return np.zeros(0, np.int64)
    thr, one, zero = F(thresh), F(1), F(0)
    x1, y1, x2, y2 = dets[:, 0], dets[:, 1], dets[:, 2], dets[:, 3]
    with np.errstate(all="ignore"):
        area = (x2 - x1 + one) * (y2 - y1 + one)
        order = visit_order(dets[:, 4])
        dead = np.zeros(n, bool)
        kept = []
        for pos, i in enumerate(order):
            if dead[i]:
                continue
            kept.append(i)
            rest = order[pos + 1:]
            w = np.maximum(zero, np.minimum(x2[i], x2[rest]) - np.maximum(x1[i], x1[rest]) + one)
            h = np.maximum(zero, np.minimum(y2[i], y2[rest]) - np.maximum(y1[i], y1[rest]) + one)
            inter = w * h
            ovr = inter / (area[i] + area[rest] - inter)
            assert ovr.dtype == F
            dead[rest[~(ovr <= thr)]] = True
    return np.asarray(kept, np.int64)


def per_class(cls_score, bbox_xyxy, min_det_score, nms_thr):
    """One image: [(rows kept, in NMS order)] per foreground class (image row indices)."""
    cls_score, bbox_xyxy = np.asarray(cls_score, F), np.asarray(bbox_xyxy, F)
    R, K = cls_score.shape
    shared = bbox_xyxy.shape[1] == 4
    out = []
    for c in range(1, K):
        s = cls_score[:, c]
        with np.errstate(invalid="ignore"):
            rows = np.flatnonzero(s > F(min_det_score))
        box = bbox_xyxy[rows] if shared else bbox_xyxy[rows, 4 * c:4 * c + 4]
        det = np.concatenate([box.reshape(-1, 4), s[rows, None]], 1).astype(F)
        out.append(rows[hard_nms(det, nms_thr)])
    return out


def bbox_post(cls_score, bbox_xyxy, max_det_per_image, min_det_score, nms_thr):
    """(B,R,K), (B,R,4 | 4K) -> post_score (B,top,1), post_bbox_xyxy (B,top,4), post_cls (B,top,1), and the
    per-image per-class kept rows."""
    cls_score, bbox_xyxy = np.asarray(cls_score, F), np.asarray(bbox_xyxy, F)
    B, R, K = cls_score.shape
    top = int(max_det_per_image)
    shared = bbox_xyxy.shape[2] == 4
    ps, pb, pc = np.zeros((B, top, 1), F), np.zeros((B, top, 4), F), np.full((B, top, 1), -1, F)
    kept_all = []
    for b in range(B):
        kept = per_class(cls_score[b], bbox_xyxy[b], min_det_score, nms_thr) if K > 1 else []
        kept_all.append(kept)
        rows = np.concatenate(kept).astype(np.int64) if kept else np.zeros(0, np.int64)
        cid = np.concatenate([np.full(len(k), c, np.int64) for c, k in enumerate(kept)]) if kept else rows
        sc = cls_score[b, rows, cid + 1]
        pick = visit_order(sc)[:top]
        n = len(pick)
        r, c = rows[pick], cid[pick]
        ps[b, :n, 0] = sc[pick]
        pc[b, :n, 0] = c
        for t in range(n):
            pb[b, t] = bbox_xyxy[b, r[t]] if shared else bbox_xyxy[b, r[t], 4 * (c[t] + 1):4 * (c[t] + 2)]
    return ps, pb, pc, kept_all
