"""Inputs of the BboxPostProcessing / hard-NMS tests (tests/golden/bbox_post.npz stores their SHA-256 and
what the reference's own Python computed on them; tests/golden/make_golden_bbox_post.py).

Every case is (cls_score (B,R,K) with the background in column 0, bbox_xyxy (B,R,4) or (B,R,4K), and the
operator's parameters).  CONDITION asserted here: within an image the foreground scores over the threshold
are pairwise distinct -- the reference orders equal scores by numpy's unstable sort, so only then is its
result defined; float32 softmax does produce duplicates, which are nudged apart by ulps."""
import numpy as np

F = np.float32

# name -> (builder, keyword arguments of the operator)
CASES = ("edges", "edges_top", "edges_ulp", "shared", "mask_r50", "mask_r50_low", "r2000")


def iou_f32(a, b):
    """ovr of two boxes with every operation in float32 (operator_py/nms.py:55, :62-70)."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    one, zero = F(1), F(0)
    area_a = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    area_b = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    w = np.maximum(zero, np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]) + one)
    h = np.maximum(zero, np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]) + one)
    inter = w * h
    return inter / (area_a + area_b - inter)


def box_one_ulp_above_half():
    """A box [0, 0, x, 9] whose float32 IoU with [0, 0, 9, 9] is the float next above 0.5."""
    want = np.nextafter(F(0.5), F(1))
    x = F(19)
    for _ in range(64):
        x = np.nextafter(x, F(0))
        v = iou_f32([0, 0, 9, 9], [0, 0, x, 9])
        if v == want:
            return [0, 0, float(x), 9]
        assert v <= want, "stepped over the float next above 0.5"
    raise AssertionError("no box with IoU one ulp above 0.5 found")


def edges_inputs():
    """Hand-built integer boxes, one image, 5 foreground classes with class-specific boxes, min_det_score
    0.25, thr 0.5.  (class, box, score, fate):"""
    rows = [
        # class 0: IoU exactly 0.5 is kept (<=); one ulp above is suppressed
        (0, [0, 0, 9, 9], 0.95, "kept"),
        (0, [0, 0, 19, 9], 0.90, "kept: IoU 100 / 200 = 0.5 with the first"),
        (0, box_one_ulp_above_half(), 0.85, "suppressed by the first: IoU 0.5 + 1 ulp"),
        # class 1: touching / disjoint / identical / one-pixel boxes
        (1, [20, 20, 29, 29], 0.80, "kept"),
        (1, [30, 20, 39, 29], 0.79, "kept: touches, w = 29 - 30 + 1 = 0"),
        (1, [100, 100, 109, 109], 0.78, "kept: disjoint"),
        (1, [20, 20, 29, 29], 0.77, "suppressed: identical to the first"),
        (1, [25, 25, 25, 25], 0.76, "kept: one pixel, IoU 1 / 100"),
        (1, [25, 25, 25, 25], 0.75, "suppressed: the same pixel"),
        # class 2: the chain -- B is suppressed by A and therefore does not suppress C
        (2, [0, 0, 9, 9], 0.70, "kept"),
        (2, [2, 0, 11, 9], 0.69, "suppressed by A: 80 / 120"),
        (2, [4, 0, 13, 9], 0.68, "kept: 60 / 140 with A; 80 / 120 with B, which is dead"),
        # class 3: no row over the threshold; a score exactly equal to it is dropped (>)
        (3, [60, 60, 69, 69], 0.25, "dropped: equal to min_det_score"),
        (3, [70, 70, 79, 79], 0.125, "dropped"),
        # class 4: one survivor next to a score equal to the threshold
        (4, [50, 50, 59, 59], 0.60, "kept"),
        (4, [50, 50, 59, 59], 0.25, "dropped: equal to min_det_score"),
    ]
    R, K = len(rows) + 2, 6
    score = np.zeros((1, R, K), F)
    score[0, :, 0] = 0.99   # the background column is never looked at
    bbox = np.zeros((1, R, 4 * K), F)
    bbox[0, :, :4] = [0, 0, 500, 500]   # nor is its box
    for r, (c, b, s, _) in enumerate(rows):
        score[0, r, c + 1] = s
        bbox[0, r, 4 * (c + 1):4 * (c + 2)] = b
    return score, bbox


def nudge_distinct(score, above):
    """Make the foreground scores > `above` of every image pairwise distinct by moving duplicates up by
    ulps (in place); returns how many moved."""
    moved = 0
    for b in range(score.shape[0]):
        fg = score[b, :, 1:]
        idx = np.flatnonzero(fg > F(above))
        vals = fg.ravel()[idx]
        order = np.argsort(vals, kind="stable")
        sv = vals[order].copy()
        for i in range(1, len(sv)):
            if sv[i] <= sv[i - 1]:
                sv[i] = np.nextafter(sv[i - 1], F(np.inf))
                moved += 1
        vals[order] = sv
        flat = fg.reshape(-1)
        flat[idx] = vals
        score[b, :, 1:] = flat.reshape(fg.shape)
    return moved


def assert_distinct(score, above):
    for b in range(score.shape[0]):
        v = score[b, :, 1:]
        v = v[v > F(above)]
        assert len(np.unique(v)) == len(v), "duplicate scores over the threshold in image %d" % b


def random_inputs(seed, B, R, K, class_specific, distinct_above, clusters=40):
    """Softmax scores (float32) and boxes clustered so that NMS has work to do."""
    rs = np.random.RandomState(seed)
    logit = (rs.standard_normal((B, R, K)) * 3).astype(F)
    e = np.exp(logit - logit.max(-1, keepdims=True))
    score = (e / e.sum(-1, keepdims=True)).astype(F)
    centre = rs.uniform(0, 1, (B, clusters, 2)) * [1333, 800]
    size = rs.uniform(24, 320, (B, clusters, 2))
    which = rs.randint(0, clusters, (B, R))
    take = np.arange(B)[:, None]
    c = centre[take, which] + rs.standard_normal((B, R, 2)) * 12
    s = size[take, which] * rs.uniform(0.7, 1.4, (B, R, 2))
    base = np.concatenate([c - s / 2, c + s / 2], -1)
    if class_specific:
        jit = rs.standard_normal((B, R, K, 4)) * (s.mean(-1) * 0.06)[..., None, None]
        bbox = (base[:, :, None, :] + jit).reshape(B, R, 4 * K)
    else:
        bbox = base
    bbox = bbox.astype(F)
    nudge_distinct(score, distinct_above)
    return score, bbox


def case(name):
    """-> (cls_score, bbox_xyxy, dict(max_det_per_image, min_det_score, nms_thr))"""
    if name in ("edges", "edges_top", "edges_ulp"):
        score, bbox = edges_inputs()
        par = dict(max_det_per_image=100, min_det_score=0.25, nms_thr=0.5)
        if name == "edges_top":   # more survivors than max_det
            par["max_det_per_image"] = 4
        if name == "edges_ulp":   # the threshold one ulp below 0.5: IoU exactly 0.5 is one ulp above it
            par["nms_thr"] = float(np.nextafter(F(0.5), F(0)))
    elif name == "shared":        # one shared box per row, (B,R,4)
        score, bbox = random_inputs(101, 2, 300, 11, False, 0.05)
        par = dict(max_det_per_image=50, min_det_score=0.05, nms_thr=0.5)
    elif name in ("mask_r50", "mask_r50_low"):   # config/mask_r50v1_fpn_1x.py:161-174
        score, bbox = random_inputs(102, 2, 1000, 81, True, 0.001)
        par = dict(max_det_per_image=100, min_det_score=0.05 if name == "mask_r50" else 0.001, nms_thr=0.5)
    elif name == "r2000":
        score, bbox = random_inputs(103, 1, 2000, 81, True, 0.01)
        par = dict(max_det_per_image=300, min_det_score=0.01, nms_thr=0.3)
    else:
        raise KeyError(name)
    assert_distinct(score, par["min_det_score"])
    return score, bbox, par
