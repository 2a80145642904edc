#!/usr/bin/env python
"""Golden fixture for the RepPoints training head, produced by THE REFERENCE'S OWN FUNCTIONS.

Run where the reference checkout exists:
    python tests/golden/make_golden_reppoints.py
Imported from the reference, where it lies, and run unmodified on the evaluating numpy stand-in
(tests/mx_numpy_eval_reppoints.py): models/RepPoints/point_ops.py _gen_points, _offset_to_boxes, _point_target with
both assigners, _offset_to_pts and _points2bbox.  The box-loss expressions around them are formed as
RepPointsHead.get_loss forms them (models/RepPoints/builder.py:415-438): concat, reshape, _points2bbox(y_first=False),
(box - gt) / normalize_term, smooth_l1(scalar=3), the weight.
-> tests/golden/reppoints_head.npz: data only -- the gt rows of every case and every result (the point maps are
regenerated from seeds by tests/reppoints_ref.py).

The script also ASSERTS what the tests rely on: no gt's level sum within 4 ulp of an integer unless both logarithms
are of exact powers of two; in the moment_transfer case every IoU at least 1e-3 from both thresholds and every
positive column maximum (and the arg-max of every row that can be
assigned) unique by 1e-3; in the loss cases no residual at the smooth-L1 knee and no tied
minimum or maximum, in float32 and in float64 alike."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests import mx_numpy_eval, mx_numpy_eval_reppoints as ER, reppoints_ref as rr  # noqa: E402

A = mx_numpy_eval.Arr
F32 = np.float32


class Reference:
    def __enter__(self):
        self.ctx = mx_numpy_eval.modules(REF, None)
        m = self.ctx.__enter__()
        self.F = ER.extend(m.mx, m.X)
        self.X = m.X
        self.ops = importlib.import_module("models.RepPoints.point_ops")
        return self

    def __exit__(self, *a):
        return self.ctx.__exit__(*a)


def run_targets(R, c):
    """builder.py:328-388"""
    F, ops = R.F, R.ops
    N = c["gt_bbox"].shape[0]
    mt = A(c["mt"])
    points, boxes = [], []
    for pred, s in zip(c["pts_init"], c["strides"]):
        points.append(ops._gen_points(F, A(pred), s))
        boxes.append(ops._offset_to_boxes(F, points[-1], A(pred), s, c["transform"], moment_transfer=mt))
    proposals = F.tile(F.concat(*points, dim=1), reps=(N, 1, 1))
    li, gi, wi = ops._point_target(F, proposals, A(c["gt_bbox"]), N, "point", scale=c["target_scale"], num_pos=c["num_pos"])
    box_proposals = F.concat(*boxes, dim=1)
    lr, gr, wr = ops._point_target(F, box_proposals, A(c["gt_bbox"]), N, "box", pos_iou_thr=c["pos_iou_thr"],
                                   neg_iou_thr=c["neg_iou_thr"], min_pos_iou=c["min_pos_iou"])
    return dict(label_init=li.v, gt_init=gi.v, weight_init=wi.v, label_refine=lr.v, gt_refine=gr.v, weight_refine=wr.v,
                boxes=box_proposals.v, points=proposals.v)


def run_losses(R, c, tg):
    """builder.py:415-438 and :452-471, forward"""
    F, ops, X = R.F, R.ops, R.X
    N, K = c["gt_bbox"].shape[0], c["num_points"]
    mt = A(c["mt"])
    out = {}
    for key in ("init", "refine"):
        pts, terms = [], []
        for pred, s in zip(c["pts_" + key], c["strides"]):
            points = ops._gen_points(F, A(pred), s)
            pts.append(ops._offset_to_pts(F, points, A(pred), s, K))
            terms.append(F.ones_like(F.slice_axis(pts[-1], begin=0, end=4, axis=-1)) * s)
        concat_ = X.concat(pts, axis=1)
        concat = X.reshape(concat_, (-3, -2))
        bboxes_ = ops._points2bbox(F, concat, c["transform"], y_first=False, moment_transfer=mt)
        bboxes = X.reshape(bboxes_, (-4, N, -1, -2))
        normalize_term = X.concat(terms, axis=1) * c["scale"]
        loss = X.smooth_l1(data=(bboxes - A(tg["gt_" + key])) / normalize_term, scalar=3.0)
        weight = F.repeat(F.expand_dims(F.where(A(tg["label_" + key]) > 0, F.ones_like(A(tg["label_" + key])),
                                                F.zeros_like(A(tg["label_" + key]))), -1), repeats=4, axis=-1)
        out["loss_" + key] = (loss * weight).v
        out["pts_" + key] = concat_.v
        out["bboxes_" + key] = bboxes.v
    return out


def check_level_sums(name, c):
    for gt in c["gt_bbox"]:
        _, _, gw, gh, _, lw, lh = rr.gt_levels(gt, c["target_scale"], F32(-1e9), F32(1e9))
        for m in np.nonzero(gt[:, 4] > 0)[0]:
            half = (lw[m] + lh[m]) / F32(2)
            exact = all(float(v).is_integer() for v in (lw[m], lh[m])) and \
                all(np.frexp(v / F32(c["target_scale"]))[0] == 0.5 for v in (gw[m], gh[m]))
            near = abs(float(half) - round(float(half))) <= 4 * float(np.spacing(np.abs(half) + F32(1)))
            assert exact or not near, "%s: gt %d level sum %r within 4 ulp of an integer" % (name, m, half)


def check_margins(c, tg):
    for n in range(c["gt_bbox"].shape[0]):
        _, _, iou = rr.iou_assign_f32(tg["boxes"][n], c["gt_bbox"][n], c["pos_iou_thr"], c["neg_iou_thr"], c["min_pos_iou"])
        for thr in (c["pos_iou_thr"], c["neg_iou_thr"]):
            assert np.abs(iou - F32(thr)).min() >= 1e-3
        top = np.sort(iou, axis=0)
        assert ((top[-1] - top[-2] >= 1e-3) | (top[-1] == 0)).all()          # every positive column maximum is unique
        top = np.sort(iou, axis=1)                                             # ... and the arg-max of every row that can
        rows = (top[:, -1] >= F32(c["neg_iou_thr"])) | ((iou == iou.max(0)[None]).any(1) & (top[:, -1] > 0))   # be assigned
        assert (top[:, -1] - top[:, -2] >= 1e-3)[rows].all()
        assert np.abs(iou.max(0) - F32(c["min_pos_iou"])).min() >= 1e-3 or c["min_pos_iou"] == 0.0


def check_loss_case(name, c, tg):
    for dt in (np.float32, np.float64):
        for key in ("init", "refine"):
            begin = 0
            for pred, s in zip(c["pts_" + key], c["strides"]):
                x, y = rr._abs_points(pred, s, dt)
                hw = x.shape[1]
                if c["transform"] != "moment":
                    Q = 4 if c["transform"] == "partial_minmax" else x.shape[-1]
                    for v in (x[..., :Q], y[..., :Q]):
                        srt = np.sort(v, axis=-1)
                        assert (srt[..., 0] < srt[..., 1]).all() and (srt[..., -2] < srt[..., -1]).all(), name
                box = rr.points2bbox(x, y, c["transform"], np.asarray(c["mt"], dt))
                r = (box - tg["gt_" + key][:, begin:begin + hw].astype(dt)) / (dt(s) * dt(c["scale"]))
                w = tg["label_" + key][:, begin:begin + hw] > 0
                assert (np.abs(np.abs(r[w]) - 1.0 / 9) > 1e-5).all(), name
                begin += hw


def main():
    out, names, lnames = {}, [], []
    with Reference() as R:
        for name, c in rr.target_cases() + [rr.margin_target_case()]:
            check_level_sums(name, c)
            t = run_targets(R, c)
            for key in ("init", "refine"):      # the weights are label > 0, repeated four times (point_ops.py:213-214)
                assert np.array_equal(t["weight_" + key], np.repeat((t["label_" + key] > 0).astype(F32)[..., None], 4, -1))
            sizes = [p.shape[2:] for p in c["pts_init"]]
            assert np.array_equal(t["points"][0], rr.gen_points(sizes, c["strides"]))
            if name == "moment-transfer":
                check_margins(c, dict(boxes=t["boxes"]))
            names.append(name)
            out["t/%s/gt_bbox" % name] = c["gt_bbox"]
            for key in ("label_init", "label_refine"):
                assert np.array_equal(t[key].astype(np.int8).astype(F32), t[key])
                out["t/%s/%s" % (name, key)] = t[key].astype(np.int8)
            for key in ("gt_init", "gt_refine", "boxes"):
                out["t/%s/%s" % (name, key)] = t[key]
        for name, c in rr.loss_cases():
            check_level_sums(name, c)
            tg = rr.targets_f32(c)
            check_loss_case(name, c, tg)
            r = run_losses(R, c, tg)
            lnames.append(name)
            for key in ("loss_init", "loss_refine", "bboxes_init", "bboxes_refine"):
                out["l/%s/%s" % (name, key)] = r[key]
            if name == "minmax":
                out["l/%s/pts_init" % name] = r["pts_init"]
    out["target_cases"], out["loss_cases"] = np.array(names), np.array(lnames)
    path = os.path.join(HERE, "reppoints_head.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d target cases, %d loss cases)" % (path, os.path.getsize(path), len(names), len(lnames)))


if __name__ == "__main__":
    main()
