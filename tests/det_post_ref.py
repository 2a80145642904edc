"""numpy statement of the final detections (detection_test.py:174-178, :233-290) WITH A DEFINED TIE RULE, the one
sd_hard_nms_batched follows, for the inputs where the reference's own Python cannot serve (equal scores: its order is
numpy's unstable sort).  tests/test_det_post.py shows that it equals the reference-run fixture on every case, which
is what licenses its use for ties and NaNs.

  * nms: float32, tests/bbox_post_ref.py's hard_nms (the same rule sd_hard_nms_batched follows);
  * set_nms: FLOAT64 on the float32 inputs (detection_test.py:247-253 promotes the array); box j survives a kept
    box i iff ovr <= thresh or (ovr > thresh and set[j] == set[i]) -- a NaN ovr suppresses;
  * visiting order: descending score, among equal scores the later row first, NaN scores first;
  * det_post: box / im_scale in float32, the background dropped on request, per class `score > min_det_score`
    (NaN fails), classes stacked in class order, the max_det best of the stack by the same order rule,
    written best first."""
import numpy as np

from .bbox_post_ref import hard_nms, visit_order

F = np.float32
D = np.float64


def set_nms(dets, set_index, thresh, dtype=D):
    """dets (n,5) float32, set_index (n) -> kept row indices in visiting order; arithmetic in `dtype`
    (float64 is the device's and the reference's; float32 exists to show that it is another function)."""
    dets32 = np.asarray(dets, F)
    n = len(dets32)
    if n == 0:
        return np.zeros(0, np.int64)
    d = dets32.astype(dtype)
    sets = np.asarray(set_index)
    thr, one, zero = dtype(F(thresh)), dtype(1), dtype(0)
    x1, y1, x2, y2 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
    with np.errstate(all="ignore"):
        area = (x2 - x1 + one) * (y2 - y1 + one)
        order = visit_order(dets32[:, 4])
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
            assert ovr.dtype == dtype
            live = (ovr <= thr) | ((ovr > thr) & (sets[rest] == sets[i]))
            dead[rest[~live]] = True
    return np.asarray(kept, np.int64)


def nms_keep(dets, thresh, set_index=None):
    return hard_nms(dets, thresh) if set_index is None else set_nms(dets, set_index, thresh)


def det_post(cls, box, im_scale, max_det_per_image, min_det_score, nms_thr, nms_type="nms", set_period=0,
             skip_background=True, set_dtype=D):
    """-> out_dets (B,top,6) best first, out_counts (B) int32, kept[b][c] = image rows in NMS order"""
    cls, box = np.asarray(cls, F), np.asarray(box, F)
    B, R, K = cls.shape
    skip = int(bool(skip_background))
    C = K - skip
    shared = box.shape[2] == 4
    top = int(max_det_per_image)
    out = np.zeros((B, top, 6), F)
    out[:, :, 5] = -1
    counts = np.zeros(B, np.int32)
    kept_all = []
    for b in range(B):
        bx = box[b] if im_scale is None else box[b] / F(im_scale[b])
        assert bx.dtype == F
        kept, recs = [], []
        for c in range(C):
            s = cls[b, :, c + skip]
            with np.errstate(invalid="ignore"):
                rows = np.flatnonzero(s > F(min_det_score))
            cb = bx[rows] if shared else bx[rows, 4 * (c + skip):4 * (c + skip) + 4]
            det = np.concatenate([cb.reshape(-1, 4), s[rows, None]], 1).astype(F)
            if nms_type == "nms":
                k = hard_nms(det, nms_thr)
            else:
                k = set_nms(det, rows % set_period, nms_thr, set_dtype)
            kept.append(rows[k])
            recs += [(det[i], c) for i in k]
        kept_all.append(kept)
        sc = np.array([d[4] for d, _ in recs], F)
        pick = visit_order(sc)[:top]
        counts[b] = len(pick)
        for t, g in enumerate(pick):
            out[b, t, :5] = recs[g][0]
            out[b, t, 5] = recs[g][1]
    return out, counts, kept_all
