"""Inputs of the final-detection tests (tests/golden/det_post.npz stores their SHA-256 and what the reference's
own Python computed on them; tests/golden/make_golden_det_post.py).

A case is what detection_test.py:168 receives for a batch -- cls (B,R,K) with the background in column 0, box
(B,R,4) or (B,R,4K), im_scale (B) -- and the test parameters.  CONDITION asserted here: within an image the
foreground scores over the threshold are pairwise distinct, so the reference's unstable argsort and its cut
have one answer.

f64_pairs(): isolated box pairs whose `ovr <= 0.5` comes out differently in float32 and in float64 on the SAME
float32 coordinates -- set_nms runs in float64 (detection_test.py:247-253 promotes the array), so these are the
inputs on which a float32 set_nms is visibly another function."""
import numpy as np

from . import bbox_post_cases as bp

F = np.float32
D = np.float64

CASES = ("retina", "fcos_dense", "skip_cs", "empty", "crowd", "set_pairs")
TIMED = ("retina", "fcos_dense", "crowd")


def iou(a, b, T):
    """ovr of two boxes with every operation in dtype T (operator_py/nms.py:55 / :86, :62-70 / :94-102)."""
    a, b = np.asarray(a, F).astype(T), np.asarray(b, F).astype(T)
    one, zero = T(1), T(0)
    area_a = (a[2] - a[0] + one) * (a[3] - a[1] + one)
    area_b = (b[2] - b[0] + one) * (b[3] - b[1] + one)
    w = np.maximum(zero, np.minimum(a[2], b[2]) - np.maximum(a[0], b[0]) + one)
    h = np.maximum(zero, np.minimum(a[3], b[3]) - np.maximum(a[1], b[1]) + one)
    inter = w * h
    return inter / (area_a + area_b - inter)


def f64_pairs(want=6, seed=77):
    """-> [(box_a, box_b, kept_in_f32, kept_in_f64)] with kept_in_f32 != kept_in_f64 at thresh 0.5.
    Directed search: B is A shifted and resized; B's x2 is bisected (over float32 values) onto the point where
    the float64 ovr crosses 0.5, then the float32 neighbours of the crossing are compared in both precisions
    (about 1-2 % of the pairs within 1e-6 of the threshold disagree).  Pair k lies in x in [2500 k, 2500 (k + 1)):
    no box of one pair touches a box of another."""
    rs = np.random.RandomState(seed)
    found = []
    for _ in range(4000):
        if len(found) >= want:
            break
        y1 = rs.uniform(0, 900)
        x1 = 2500 * len(found) + rs.uniform(0, 100)   # pair k lives in its own 2500-wide slot: isolated
        w, h = rs.uniform(40, 300, 2)
        a = np.array([x1, y1, x1 + w, y1 + h], F)
        b = a.copy()
        b[1] = F(y1 + rs.uniform(-0.1, 0.1) * h)
        b[3] = F(b[1] + h * rs.uniform(0.9, 1.1))
        b[0] = F(x1 + rs.uniform(0.0, 0.1) * w)
        # growing x2 past A's right edge lowers the ovr: from "B covers A" down towards 0
        lo, hi = F(a[2]), F(x1 + 4 * w)
        b[2] = lo
        if not iou(a, b, D) > 0.5:
            continue
        b[2] = hi
        if not iou(a, b, D) <= 0.5:
            continue
        while np.nextafter(lo, F(np.inf)) < hi:      # invariant: ovr64(lo) > 0.5 >= ovr64(hi)
            mid = F((D(lo) + D(hi)) / 2)
            b[2] = mid
            if iou(a, b, D) > 0.5:
                lo = mid
            else:
                hi = mid
        x = lo
        for _ in range(8):
            x = np.nextafter(x, F(-np.inf))
        for _ in range(17):
            b[2] = x
            k32, k64 = bool(iou(a, b, F) <= F(0.5)), bool(iou(a, b, D) <= 0.5)
            if k32 != k64:
                found.append((a.copy(), b.copy(), k32, k64))
                break
            x = np.nextafter(x, F(np.inf))
    return found


def _distinct(cls, above):
    bp.nudge_distinct(cls, above)
    bp.assert_distinct(cls, above)


def _boxes(rs, B, R, clusters=60):
    centre = rs.uniform(0, 1, (B, clusters, 2)) * [1333, 800]
    size = rs.uniform(24, 320, (B, clusters, 2))
    which = rs.randint(0, clusters, (B, R))
    take = np.arange(B)[:, None]
    c = centre[take, which] + rs.standard_normal((B, R, 2)) * 12
    s = size[take, which] * rs.uniform(0.7, 1.4, (B, R, 2))
    return np.concatenate([c - s / 2, c + s / 2], -1).astype(F)


def retina_inputs(seed=201, B=2, R=5000, K=81, crowded=4300):
    """GenProposalRetina's form: one non-zero class score per row, a shared box.  Image 0 puts `crowded` rows
    into one class (more than 4096 candidates: the large path), image 1 spreads them (the in-LDS path)."""
    rs = np.random.RandomState(seed)
    cls = np.zeros((B, R, K), F)
    label = rs.randint(1, K, (B, R))
    label[0, rs.permutation(R)[:crowded]] = 4
    sc = rs.uniform(0.02, 1.0, (B, R)).astype(F)
    for b in range(B):
        cls[b, np.arange(R), label[b]] = sc[b]
    _distinct(cls, 0.05)
    return cls, _boxes(rs, B, R)


def fcos_dense_inputs(seed=202, R=5000):
    """every row of one class over the threshold: R candidates in one problem"""
    rs = np.random.RandomState(seed)
    cls = np.zeros((1, R, 2), F)
    cls[0, :, 1] = rs.uniform(0.06, 1.0, R)
    _distinct(cls, 0.05)
    return cls, _boxes(rs, 1, R, clusters=300)


def crowd_inputs(seed=205, B=2, top_n=1000):
    """the double-prediction head's form: rows r and r + top_n are the two predictions of proposal r"""
    rs = np.random.RandomState(seed)
    cls = np.zeros((B, 2 * top_n, 2), F)
    cls[:, :, 1] = rs.uniform(0.0, 1.0, (B, 2 * top_n))
    cls[:, :, 0] = 1 - cls[:, :, 1]
    _distinct(cls, 0.05)
    first = _boxes(rs, B, top_n, clusters=80)
    second = first + (rs.standard_normal(first.shape) * 6).astype(F)
    shared = np.concatenate([first, second], 1)
    return cls, np.concatenate([np.zeros_like(shared), shared], -1)   # (B,R,8): group 0 is the background's


def case(name):
    """-> (cls, box, im_scale or None, dict(max_det_per_image, min_det_score, nms_thr, nms_type, set_period))"""
    par = dict(max_det_per_image=100, min_det_score=0.05, nms_thr=0.5, nms_type="nms", set_period=0)
    if name == "retina":           # models/retinanet/builder.py:362-394: 5 levels x 1000 rows
        cls, box = retina_inputs()
        scale = np.array([1.0, 1.6], F)
    elif name == "fcos_dense":
        cls, box = fcos_dense_inputs()
        scale = None
    elif name == "skip_cs":        # class-specific boxes, background dropped, im_scale != 1
        cls, box = bp.random_inputs(203, 2, 300, 6, True, 0.05)
        scale = np.array([1.5, 0.6], F)
        par["max_det_per_image"] = 40
    elif name == "empty":          # image 1 has nothing over the threshold
        cls, box = bp.random_inputs(204, 2, 200, 4, False, 0.05)
        cls[1, :, 1:] *= F(0.01)
        scale = None
    elif name == "crowd":          # config/crowdhuman/doublepred_r50v1b_fpn_1x_refine.py:192-194: 2 x 1000 rows
        cls, box = crowd_inputs()
        scale = np.array([1.0, 1.25], F)
        par.update(max_det_per_image=300, nms_type="set_nms", set_period=1000)
    elif name == "set_pairs":      # the float64 pairs, every pair far from the others, its two boxes in two sets
        pairs = f64_pairs()
        assert len(pairs) >= 4
        cls = np.zeros((1, 64, 2), F)
        box = np.zeros((1, 64, 4), F)
        for i, (a, b, _, _) in enumerate(pairs):     # rows 2i and 2i + 1: different sets under period 32
            box[0, 2 * i], box[0, 2 * i + 1] = a, b
            cls[0, 2 * i, 1], cls[0, 2 * i + 1, 1] = 0.9 - 0.01 * i, 0.8 - 0.01 * i
        scale = None
        par.update(nms_type="set_nms", set_period=32)
    else:
        raise KeyError(name)
    bp.assert_distinct(cls, par["min_det_score"])
    return cls, box, scale, par
