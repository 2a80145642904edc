"""TEST INFRASTRUCTURE: a float32 numpy restatement of the FCOS test-time decode (models/FCOS/utils.py:7-149 behind
models/FCOS/builder.py:234-259) with the project's tie rule, and the case lists of tests/test_fcos_decode.py.  The
inputs of every case are regenerated from RandomState seeds; tests/golden/fcos_decode.npz holds only the results the
reference's own CustomOps gave for `cases()` (tests/golden/make_golden_fcos_decode.py).

Tie rule (MXNet's order among equal keys is not documented, so it is ours): equal fused scores inside a level -> the
lower flat index first; the batch sort is stable in concat order; -0.0 == +0.0.  NaN is not restated."""
import numpy as np

F32 = np.float32
THRESH = 0.05
SCORE_COLS = 81


def sigmoid32(x):
    """1.0f / (1.0f + expf(-x)) in float32 numpy"""
    x = np.asarray(x, F32)
    with np.errstate(over="ignore"):
        return (F32(1) / (F32(1) + np.exp(-x).astype(F32))).astype(F32)


def _desc(v):
    return np.argsort(-v, kind="stable")


def decode_level(cls, ctr, off, im_info, stride, top_n, thresh):
    """get_proposal_single_stage: (N, top_n, 6) rows [cls, fused, x1, y1, x2, y2], -1 where nothing is"""
    N, C, H, W = cls.shape
    cand = cls > F32(thresh)
    fused = (cls * ctr).astype(F32)
    res = np.full((N, top_n, 6), -1, F32)
    for i in range(N):
        flat = fused[i].reshape(-1)
        count = int(cand[i].sum())
        if count >= top_n:
            idx = _desc(flat)[:top_n]
        elif count > 0:
            idx = np.nonzero(cand[i].reshape(-1))[0]
        else:
            continue
        x, y, c = idx % W, idx // W % H, idx // W // H
        half = F32(stride / 2)
        cx = x.astype(F32) * F32(stride) + half
        cy = y.astype(F32) * F32(stride) + half
        img_h, img_w = im_info[i, 0], im_info[i, 1]
        o = off[i]
        clip = lambda v, hi: np.minimum(np.maximum(v, F32(0)), hi)
        rows = np.stack([(c + 1).astype(F32), flat[idx],
                         clip(cx - o[0, y, x], img_w), clip(cy - o[1, y, x], img_h),
                         clip(cx + o[2, y, x], img_w), clip(cy + o[3, y, x], img_h)], axis=1).astype(F32)
        masked = (rows[:, 0] >= rows[:, 2]) & (rows[:, 1] >= rows[:, 3])
        rows[masked] = -1
        res[i, :len(idx)] = rows
    return res


def decode(cls_list, ctr_list, off_list, im_info, strides, top_n, thresh=THRESH):
    """-> dict(stage (N, R, 6), bbox (N, R, 4), score (N, R, 81), cls_id (N, R))"""
    stage = np.concatenate([decode_level(c, t, o, im_info, s, top_n, thresh)
                            for c, t, o, s in zip(cls_list, ctr_list, off_list, strides)], axis=1)
    N, R = stage.shape[:2]
    rows = np.stack([stage[i][_desc(stage[i, :, 1])] for i in range(N)]) if N else stage
    score = np.zeros((N, R, SCORE_COLS), F32)
    for i in range(N):
        val = np.sqrt(np.clip(rows[i, :, 1], F32(1e-20), F32(1))).astype(F32)
        score[i, np.arange(R), rows[i, :, 0].astype(np.int64)] = val      # cls = -1: the LAST column
    return dict(stage=stage, bbox=rows[:, :, 2:].copy(), score=score, cls_id=rows[:, :, 0].copy())


# ---- inputs -------------------------------------------------------------------------------------------------------
def _level(rs, N, shape, counts, off_scale=12.0):
    """probabilities with EXACTLY counts[i] candidates (cls > THRESH) in image i"""
    C, H, W = shape
    n = C * H * W
    cls = rs.uniform(0.002, 0.045, (N, n)).astype(F32)
    for i in range(N):
        pos = rs.permutation(n)[:counts[i]]
        cls[i, pos] = rs.uniform(0.06, 0.95, len(pos)).astype(F32)
    ctr = rs.uniform(0.2, 1.0, (N, 1, H, W)).astype(F32)
    off = rs.uniform(0.5, off_scale, (N, 4, H, W)).astype(F32)
    return cls.reshape(N, C, H, W), ctr, off


def _case(levels, im_info, strides, top_n, thresh=THRESH):
    return dict(cls=[l[0] for l in levels], ctr=[l[1] for l in levels], off=[l[2] for l in levels],
                im_info=np.asarray(im_info, F32).reshape(-1, 3), strides=list(strides), top_n=top_n, thresh=thresh)


SHAPES = ((3, 7, 11), (3, 13, 21), (5, 4, 6))
CONFIG_SIZES = ((100, 167), (50, 84), (25, 42), (13, 21), (7, 11))      # 800 x 1333 at strides 8 .. 128
CONFIG_STRIDES = (8, 16, 32, 64, 128)


def _branches():
    # image 0: count >= top_n, == top_n; image 1: 0 < count < top_n, == 0 (mixed branches on both levels, different
    # im_info)
    rs, t = np.random.RandomState(101), 8
    lv = [_level(rs, 2, s, c) for s, c in zip(SHAPES[:2], ((t + 5, 3), (t, 0)))]
    return _case(lv, [[60, 90, 1], [47, 71, 1.5]], (8, 4), t)


def _branches5():
    # count == top_n - 1 and count >= top_n on the five-class level
    rs, t = np.random.RandomState(111), 8
    return _case([_level(rs, 2, SHAPES[2], (t - 1, t + 20))], [[60, 90, 1], [47, 71, 1.5]], (16,), t)


def _small_level():
    # (5, 4, 6) holds 120 < top_n = 128 scores: it can never take the dense branch, not even with every score a
    # candidate (image 0); next to a level with count >= top_n (image 0) and == top_n - 1 (image 1)
    rs, t = np.random.RandomState(102), 128
    lv = [_level(rs, 2, (5, 7, 11), (200, t - 1)), _level(rs, 2, SHAPES[2], (120, 0))]
    return _case(lv, [[60, 90, 1], [50, 80, 1]], (8, 16), t)


def _mixed():
    rs, t = np.random.RandomState(103), 16
    lv = [_level(rs, 2, SHAPES[1], (40, 5))]
    return _case(lv, [[52, 84, 1], [40, 60, 2]], (4,), t)


def _noncand():
    # dense branch in which non-candidates (cls <= thresh, centerness ~ 1) outrank candidates (small centerness)
    rs, t = np.random.RandomState(104), 16
    cls, ctr, off = _level(rs, 1, SHAPES[0], (20,))
    cand = cls > F32(THRESH)
    cls[cand] = rs.uniform(0.06, 0.2, int(cand.sum())).astype(F32)
    # centerness is per location: locations that hold a candidate get ~0.05, all others ~1
    loc = cand.any(axis=1, keepdims=True)
    ctr = np.where(loc, rs.uniform(0.04, 0.06, ctr.shape), rs.uniform(0.97, 1.0, ctr.shape)).astype(F32)
    return _case([(cls, ctr, off)], [[56, 88, 1]], (8,), t)


def _thresh_eq():
    # top_n - 1 candidates and six scores EXACTLY float32(0.05): counted, they would flip the level to dense
    rs, t = np.random.RandomState(105), 8
    cls, ctr, off = _level(rs, 1, SHAPES[0], (t - 1,))
    flat = cls.reshape(-1)
    flat[np.nonzero(flat < F32(THRESH))[0][:6]] = F32(THRESH)
    return _case([(cls, ctr, off)], [[56, 88, 1]], (8,), t)


def _clip():
    # im_info smaller than the padded map (x2 / y2 clip) and offsets larger than the image (x1 / y1 clip to 0)
    rs, t = np.random.RandomState(106), 16
    lv = [_level(rs, 1, SHAPES[1], (60,), off_scale=40.0), _level(rs, 1, SHAPES[0], (9,), off_scale=200.0)]
    return _case(lv, [[37, 55, 1]], (4, 8), t)


def _mask():
    # "remove small bboxes": x1 <= cls and y1 <= fused -> -1; one of the two alone keeps the row
    rs, t = np.random.RandomState(107), 16
    cls, ctr, off = _level(rs, 1, SHAPES[1], (14,), off_scale=1.5)
    H, W = cls.shape[2:]
    kind = (np.arange(H * W) % 4).reshape(H, W)
    off[0, 0][(kind == 0) | (kind == 1)] = 500.0      # x1 clips to 0
    off[0, 1][(kind == 0) | (kind == 2)] = 500.0      # y1 clips to 0
    cls2, ctr2, off2 = _level(rs, 1, (3, 4, 6), (40,), off_scale=1.5)
    off2[0, :2] = 500.0                                 # a dense level whose every row is masked
    return _case([(cls, ctr, off), (cls2, ctr2, off2)], [[60, 90, 1]], (4, 16), t)


def _pad80():
    # C = 80: padding rows put sqrt(float32(1e-20)) into score column 80, next to a real class-80 row
    rs, t = np.random.RandomState(108), 8
    cls, ctr, off = _level(rs, 1, (80, 2, 3), (4,))
    cls[0, 79, 1, 2], ctr[0, 0, 1, 2] = 0.99, 1.0
    lv2 = _level(rs, 1, (80, 1, 2), (0,))
    return _case([(cls, ctr, off), lv2], [[40, 40, 1]], (16, 32), t)


def _multi_wg():
    rs = np.random.RandomState(109)
    return _case([_level(rs, 1, (80, 25, 42), (3000,))], [[800, 1333, 1]], (32,), 1000)


def config_logits(seed, N, mean, sigma=1.0):
    """logits of the five levels of config/fcos_r50v1_fpn_1x.py at 800 x 1333"""
    rs = np.random.RandomState(seed)
    lv = []
    for H, W in CONFIG_SIZES:
        lv.append(((mean + sigma * rs.standard_normal((N, 80, H, W))).astype(F32),
                   (1.0 + rs.standard_normal((N, 1, H, W))).astype(F32),
                   np.exp(rs.uniform(0.0, 5.0, (N, 4, H, W))).astype(F32)))
    return lv


def _config():
    # levels 0-2 dense, 3 and 4 sparse at this distribution (asserted by the fixture script)
    lv = [(sigmoid32(c), sigmoid32(t), o) for c, t, o in config_logits(110, 1, -5.0, 1.2)]
    return _case(lv, [[800, 1333, 1]], CONFIG_STRIDES, 1000)


CASE_NAMES = ("branches", "branches5", "small_level", "mixed", "noncand", "thresh_eq", "clip", "mask", "pad80", "multi_wg",
              "config")
TIE_NAMES = ("level", "cut", "across", "zeros", "tied_bins")


def cases():
    return [("branches", _branches()), ("branches5", _branches5()), ("small_level", _small_level()), ("mixed", _mixed()), ("noncand", _noncand()),
            ("thresh_eq", _thresh_eq()), ("clip", _clip()), ("mask", _mask()), ("pad80", _pad80()),
            ("multi_wg", _multi_wg()), ("config", _config())]


def small_cases():
    return [(n, c) for n, c in cases() if n not in ("multi_wg", "config")]


def _quantised(rs, N, shape, levels):
    C, H, W = shape
    cls = (rs.randint(1, levels + 1, (N, C, H, W)) / F32(levels + 1)).astype(F32)
    ctr = np.ones((N, 1, H, W), F32)
    off = rs.uniform(0.5, 6.0, (N, 4, H, W)).astype(F32)
    return cls, ctr, off


def tie_cases():
    """checked against the restatement only (the tie rule is the project's)"""
    rs = np.random.RandomState(201)
    out = []
    # equal scores inside a level and at the top-k cut: 5 distinct values over 231 scores
    out.append(("level", _case([_quantised(rs, 2, SHAPES[0], 5)], [[56, 88, 1], [50, 70, 1]], (8,), 16)))
    # the cut falls inside a run of equal scores: every score equal
    c = _quantised(rs, 1, SHAPES[1], 1)
    out.append(("cut", _case([c], [[52, 84, 1]], (4,), 16)))
    # equal scores across levels: the batch sort keeps concat order
    lv = [_quantised(rs, 1, s, 3) for s in ((3, 7, 11), (3, 13, 21), (3, 4, 6))]
    out.append(("across", _case(lv, [[60, 90, 1]], (8, 4, 16), 8)))
    # +0.0 and -0.0 fused scores compare equal: cls > thresh with centerness +-0
    cls, ctr, off = _quantised(rs, 1, SHAPES[0], 2)
    ctr = np.where(rs.rand(*ctr.shape) < 0.5, F32(0.0), F32(-0.0)).astype(F32)
    out.append(("zeros", _case([(cls, ctr, off)], [[56, 88, 1]], (8,), 16)))
    # a level larger than the sort capacity whose cut-off bin holds more words than fit: the radix-select path
    cls = np.full((1, 80, 25, 42), 0.5, F32)
    cls[0, 3, 2, 5] = 0.75
    ctr = np.ones((1, 1, 25, 42), F32)
    off = rs.uniform(0.5, 40.0, (1, 4, 25, 42)).astype(F32)
    out.append(("tied_bins", _case([(cls, ctr, off)], [[800, 1333, 1]], (32,), 1000)))
    return out
