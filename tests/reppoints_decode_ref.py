"""TEST INFRASTRUCTURE: the cases of the RepPoints test-time decode and a float32 numpy restatement of
RepPointsHead.get_prediction (models/RepPoints/builder.py:486-576), one operation at a time.

tests/golden/make_golden_reppoints_decode.py runs the reference's own, unmodified get_prediction on these cases and
writes tests/golden/reppoints_decode.npz; tests/test_reppoints_decode.py shows the restatement bit-equal to that
fixture and holds the device to both.

The cases feed PROBABILITIES (the stand-in's sigmoid is the identity), so no libm enters the pinned bits; all but
`mt_case` use moment_transfer = 0, whose exp is exactly 1.  The rows kept per level follow the reference's rule
(builder.py:499-502): pre_nms_top_n where stride <= 32, else every location -- so a case chooses a level's k through
its stride.  The shapes are the smallest at which each mechanism can still go wrong (64 locations per streaming
workgroup, 16 rows per gather workgroup, 24,576 locations per level selected from registers), not the workload's.
"""
import numpy as np

F32 = np.float32
TRANSFORMS = ("minmax", "partial_minmax", "moment")

CASE_NAMES = ("five_levels", "multi_wg", "exact_k", "ties", "class_edges", "one_class", "clip", "minmax",
              "partial_minmax", "moment9", "four_points_partial", "four_points_moment", "big_levels")
HAND_MADE = ("ties", "class_edges", "one_class", "clip")      # their inputs are stored in the fixture as well


def topk_table(strides, pre_nms_top_n):
    return [int(pre_nms_top_n) if s <= 32 else -1 for s in strides]


def _case(rs, N, C, sizes, strides, top_n, transform="moment", num_points=9, mt=(0.0, 0.0), im_info=None, spread=2.0):
    cls = [rs.random_sample((N, C, h, w)).astype(F32) for h, w in sizes]
    pts = [(rs.standard_normal((N, 2 * num_points, h, w)) * spread).astype(F32) for h, w in sizes]
    if im_info is None:
        im_info = [[sizes[0][0] * strides[0], sizes[0][1] * strides[0], 1.0]] * N
    return dict(cls=cls, pts=pts, im_info=np.asarray(im_info, F32).reshape(N, 3), strides=list(strides), top_n=top_n,
                ks=topk_table(strides, top_n), transform=transform, num_points=num_points, mt=np.asarray(mt, F32))


def cases():
    out = []
    # the config in small: data 128 x 160, five strides, k = (16, 16, 16, all, all); per-image sizes below the padding
    out.append(("five_levels", _case(np.random.RandomState(1), 2, 80, [(16, 20), (8, 10), (4, 5), (2, 3), (1, 2)],
                                     (8, 16, 32, 64, 128), 16, im_info=[[120, 150, 1.0], [100, 131, 1.5]])))
    # 7,200 locations = 113 streaming workgroups, the config's k; a second level with an odd W, every row kept
    out.append(("multi_wg", _case(np.random.RandomState(2), 2, 3, [(72, 100), (9, 7)], (8, 64), 1000)))
    # k == H * W, and a 1 x 1 level
    out.append(("exact_k", _case(np.random.RandomState(3), 1, 4, [(3, 5), (1, 1)], (8, 64), 15)))
    # 60 saturated maxima (exactly 1.0f) every fifth location of 300 -- they straddle the 64-location chunks -- of
    # which k = 40 are kept: the cut falls inside the run.  Level 1: five positive maxima, then 49 maxima +-0.0.
    c = _case(np.random.RandomState(4), 2, 2, [(10, 30), (6, 9)], (8, 16), 40)
    c["cls"][0] *= F32(0.9)
    flat = c["cls"][0].reshape(2, 2, 300)
    flat[0, 0, ::5] = 1.0
    flat[0, 1, 2::10] = 1.0
    flat[1, 1, ::5] = 1.0
    z = c["cls"][1].reshape(2, 2, 54)
    z[:] = 0.0
    z[:, 0, 1::2] = -0.0
    z[:, 1, 1::4] = -0.0                      # locations 1, 5, 9, ...: both classes -0.0, the maximum is -0.0
    z[0, 0, [7, 20, 33, 41, 50]] = [0.5, 0.25, 0.75, 0.125, 0.625]
    z[1, 1, [3, 4, 30, 31, 53]] = [0.5, 0.5, 0.75, 0.125, 0.625]
    out.append(("ties", c))
    # the maximum in the first class, in the last class, alternating
    c = _case(np.random.RandomState(5), 1, 5, [(3, 4), (2, 2)], (8, 64), 8)
    for x in c["cls"]:
        x *= F32(0.5)
        f = x.reshape(1, 5, -1)
        f[0, 0, 0::2] += F32(0.5)
        f[0, 4, 1::2] += F32(0.5)
    out.append(("class_edges", c))
    out.append(("one_class", _case(np.random.RandomState(6), 2, 1, [(3, 4), (2, 2)], (8, 64), 8)))
    # boxes beyond all four limits: wide point sets in an image of 20 x 12
    c = _case(np.random.RandomState(7), 2, 2, [(2, 3)], (8,), 6, transform="minmax", spread=6.0,
              im_info=[[12, 20, 1.0], [16, 24, 1.0]])
    out.append(("clip", c))
    sizes, strides = [(5, 7), (3, 4)], (16, 64)
    out.append(("minmax", _case(np.random.RandomState(8), 2, 3, sizes, strides, 12, transform="minmax")))
    out.append(("partial_minmax", _case(np.random.RandomState(9), 2, 3, sizes, strides, 12, transform="partial_minmax")))
    out.append(("moment9", _case(np.random.RandomState(10), 2, 3, sizes, strides, 12)))
    out.append(("four_points_partial", _case(np.random.RandomState(11), 2, 3, sizes, strides, 12,
                                             transform="partial_minmax", num_points=4)))
    out.append(("four_points_moment", _case(np.random.RandomState(12), 2, 3, sizes, strides, 12, num_points=4)))
    # the selection holds up to 24 keys per thread of 1,024 in registers: 24,576 locations are the last level that
    # takes that path, 25,600 the first that takes the shared select; one class, one point
    out.append(("big_levels", _case(np.random.RandomState(14), 1, 1, [(128, 192), (160, 160)], (8, 16), 16,
                                    transform="minmax", num_points=1)))
    assert tuple(n for n, _ in out) == CASE_NAMES
    return out


def mt_case():
    """a non-zero moment_transfer: exp enters, so the boxes are held to an envelope, not to bits (not in the fixture)"""
    return _case(np.random.RandomState(13), 2, 3, [(5, 7), (3, 4)], (16, 64), 12, mt=(0.3, -0.2))


def logits_case(c, seed, saturate=False):
    """logits in the shapes of case c; saturate: large logits, so that distinct logits share the probability 1.0f
    and the selection among them is by index"""
    rs = np.random.RandomState(seed)
    cls = []
    for x in c["cls"]:
        v = (rs.standard_normal(x.shape) * 2.0 - 2.0).astype(F32)
        if saturate:
            v = (v + F32(2.0)) * F32(12.0) + F32(10.0)
        cls.append(v)
    return dict(c, cls=cls)


def sigmoid32(x):
    """1.0f / (1.0f + expf(-x)) with numpy's float32 exp (the device's expf is its own)"""
    with np.errstate(all="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x.astype(F32)))).astype(F32)


def _seq_sum(v):
    s = np.zeros(v.shape[:-1], F32)
    for k in range(v.shape[-1]):
        s = s + v[..., k]
    return s


def points2bbox(x, y, transform, mt):
    """_points2bbox (point_ops.py:219-274) on (..., K) arrays -> (..., 4) [left, top, right, bottom] and, for the
    moment transform, the (mean, half) pairs it was made of"""
    if transform != "moment":
        Q = 4 if transform == "partial_minmax" else x.shape[-1]
        return np.stack([x[..., :Q].min(-1), y[..., :Q].min(-1), x[..., :Q].max(-1), y[..., :Q].max(-1)], -1), None
    K = F32(x.shape[-1])
    with np.errstate(all="ignore"):
        e = np.exp(np.asarray(mt, x.dtype))
        mx, my = _seq_sum(x) / K, _seq_sum(y) / K
        dx, dy = x - mx[..., None], y - my[..., None]
        sx, sy = np.sqrt(_seq_sum(dx * dx) / K), np.sqrt(_seq_sum(dy * dy) / K)
        hx, hy = sx * e[0], sy * e[1]
    return np.stack([mx - hx, my - hy, mx + hx, my + hy], -1), dict(mean=np.stack([mx, my, mx, my], -1),
                                                                     half=np.stack([hx, hy, hx, hy], -1))


def decode(cls, pts, im_info, strides, ks, transform, mt, detail=False):
    """get_prediction: (cls_score (N, R, C + 1), bbox_xyxy (N, R, 4)); with detail=True also, per output coordinate,
    the stride, the mean and half extent of the moment box and the point coordinate it was added to"""
    N, C = cls[0].shape[:2]
    scores_out, boxes_out, det = [], [], dict(stride=[], mean=[], half=[], point=[])
    for sc, pt, s, k in zip(cls, pts, strides, ks):
        H, W = sc.shape[2:]
        HW = H * W
        k = k if k > 0 else HW
        score = sc.transpose(0, 2, 3, 1).reshape(N, HW, C)
        m = score.max(-1)
        pp = pt.reshape(N, -1, 2, HW)
        y, x = pp[:, :, 0].transpose(0, 2, 1), pp[:, :, 1].transpose(0, 2, 1)         # (N, HW, K)
        box, mom = points2bbox(x, y, transform, mt)
        px = (np.arange(W, dtype=F32)[None, :] * F32(s) + np.zeros((H, 1), F32)).reshape(-1)
        py = (np.arange(H, dtype=F32)[:, None] * F32(s) + np.zeros((1, W), F32)).reshape(-1)
        point = np.stack([px, py, px, py], -1)
        rows_s, rows_b = [], []
        for i in range(N):
            order = np.argsort(-m[i], kind="stable")[:k]          # the lower location first among equal maxima
            b = box[i, order] * F32(s) + point[order]
            lim = np.stack([im_info[i, 1], im_info[i, 0], im_info[i, 1], im_info[i, 0]]) - F32(1)
            b = np.where(b < lim, b, lim)
            b = np.where(b > F32(0), b, F32(0))
            rows_s.append(np.concatenate([np.zeros((k, 1), F32), score[i, order]], 1))
            rows_b.append(b.astype(F32))
            det["stride"].append(np.full((k, 4), s, np.float64))
            det["point"].append(point[order])
            det["mean"].append(mom["mean"][i, order] if mom else np.zeros((k, 4), F32))
            det["half"].append(mom["half"][i, order] if mom else np.zeros((k, 4), F32))
        scores_out.append(np.stack(rows_s))
        boxes_out.append(np.stack(rows_b))
    out = dict(cls_score=np.concatenate(scores_out, 1), bbox_xyxy=np.concatenate(boxes_out, 1))
    if detail:
        # det lists run level-major, image-minor: regroup to (N, R, 4)
        L = len(cls)
        for key, v in det.items():
            out[key] = np.stack([np.concatenate([v[l * N + i] for l in range(L)], 0) for i in range(N)])
    return out


def run(c, **kw):
    return decode(c["cls"], c["pts"], c["im_info"], c["strides"], c["ks"], c["transform"], c["mt"], **kw)
