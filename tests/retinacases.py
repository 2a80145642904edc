"""Seeded cases for the RetinaNet anchor-target assignment (models/retinanet/input.py:33-199).
tests/golden/make_golden_retina_target.py runs them through the reference's own classes; the HIP op
(sd_retina_anchor_target) is compared with those fixtures bit for bit."""
import numpy as np

from simpledet_amd import synth

# config/retina_r50v1_fpn_1x.py:189-210
RETINA = dict(stride=(8, 16, 32, 64, 128), short=(100, 50, 25, 13, 7), long=(167, 84, 42, 21, 11),
              scales=(4 * 2 ** 0, 4 * 2 ** (1.0 / 3.0), 4 * 2 ** (2.0 / 3.0)), aspects=(0.5, 1.0, 2.0),
              allowed_border=9999, pos_thr=0.5, neg_thr=0.4, min_pos_thr=0.0)
# one level, one 32 x 32 anchor per cell: small enough to work by hand
HAND = dict(stride=(16,), short=(2,), long=(3,), scales=(2,), aspects=(1.0,), allowed_border=9999,
            pos_thr=0.5, neg_thr=0.4, min_pos_thr=0.0)

CASES = {
    # the 800 x 1333 config in both orientations (h < w uses h_all_anchor, h >= w v_all_anchor)
    "cfg_landscape": dict(cfg=RETINA, images=[(800, 1333, 21)]),
    "cfg_portrait": dict(cfg=RETINA, images=[(1333, 800, 22)]),
    # min_pos_thr > 0 and no border allowance (anchors reaching outside the image are invalid)
    "cfg_thr_border0": dict(cfg=dict(RETINA, min_pos_thr=0.3, allowed_border=0), images=[(800, 1333, 23)]),
    "cfg_nogt": dict(cfg=RETINA, images=[(800, 1333, None)]),
    # a gt box no valid anchor overlaps: with min_pos_thr = 0, `overlaps == gt_max_overlaps` labels
    # every zero-overlap anchor with that box's class (the reference's own TODO, :55-60)
    "cfg_zero_overlap_gt": dict(cfg=dict(RETINA, allowed_border=0), images=[(800, 1333, "far")]),
    # two boxes given twice with different classes, and -1 rows BETWEEN the valid rows
    "cfg_duplicate_gt_holes": dict(cfg=RETINA, images=[(800, 1333, "dup")]),
    # the hand case: the gt box IS the anchor at cell (1, 1)
    "hand": dict(cfg=HAND, images=[(32, 48, "hand")]),
    # two gt boxes half a stride left and right of the middle anchor: it ties both per-gt maxima,
    # the last gt gives the class, the first (arg-max) the regression target; pos_thr out of reach
    "hand_tie": dict(cfg=dict(HAND, short=(1,), pos_thr=0.9), images=[(16, 48, "tie")]),
}


def inputs(case):
    """[(im_info float32 (3,), gt_bbox float32 (M, 5))] for the images of a case"""
    out = []
    for h, w, gseed in case["images"]:
        im_info = np.array([h, w, 1.0], np.float32)
        gt = -np.ones((100, 5), np.float32)
        if gseed == "far":
            gt = synth.gt_boxes(98, 1, 100, img_h=h, img_w=w, min_n=3, max_n=6)[0]
            n = int((gt[:, 4] != -1).sum())
            gt[n] = [5000, 5000, 5100, 5100, 7]
        elif gseed == "dup":
            g = synth.gt_boxes(97, 1, 100, img_h=h, img_w=w, min_n=5, max_n=9)[0]
            n = int((g[:, 4] != -1).sum())
            # box 0's best anchor stays below pos_thr: the LAST copy's class (7) survives step 3;
            # the largest box has anchors above pos_thr: they take the FIRST copy's class (5, arg-max)
            big = 1 + int(np.argmax((g[1:n, 2] - g[1:n, 0]) * (g[1:n, 3] - g[1:n, 1])))
            g[0, 4], g[big, 4] = 4, 5
            g[n], g[n + 1] = g[0], g[big]
            g[n, 4], g[n + 1, 4] = 7, 8
            n += 1
            gt[0:2 * (n + 1):2] = g[:n + 1]          # valid rows at 0, 2, 4, ...: holes between them
        elif gseed == "hand":
            gt = -np.ones((4, 5), np.float32)
            gt[1] = [8, 8, 39, 39, 3]                 # = base anchor [-8, -8, 23, 23] + (16, 16)
        elif gseed == "tie":
            gt = -np.ones((4, 5), np.float32)
            gt[0] = [0, -8, 31, 23, 5]                 # the middle anchor [8, -8, 39, 23] - 8
            gt[2] = [16, -8, 47, 23, 9]                # ... + 8
        elif gseed is not None:
            gt = synth.gt_boxes(gseed, 1, 100, img_h=h, img_w=w, min_n=8, max_n=30)[0]
        out.append((im_info, gt))
    return out


def to_flat(cfg, im_info, arr, per_anchor):
    """layout 1 -> layout 0 (pure indexing): arr is cls (N,) [per_anchor 1] or reg (4A, sumHW) [4]"""
    A = len(cfg["scales"]) * len(cfg["aspects"])
    portrait = im_info[0] >= im_info[1]
    out, off, hw = [], 0, 0
    for s, lg in zip(cfg["short"], cfg["long"]):
        fh, fw = (lg, s) if portrait else (s, lg)
        if per_anchor == 1:
            blk = arr[off:off + A * fh * fw].reshape(A, fh, fw).transpose(1, 2, 0).reshape(-1)
            off += A * fh * fw
        else:
            blk = arr[:, hw:hw + fh * fw].reshape(A, 4, fh, fw).transpose(2, 3, 0, 1).reshape(-1, 4)
        hw += fh * fw
        out.append(blk)
    return np.concatenate(out, 0)
