#!/usr/bin/env python
"""Golden fixture for the FCOS training head, produced by THE REFERENCE'S OWN FUNCTIONS.

Run where the reference checkout exists:
    python tests/golden/make_golden_fcos.py
Imported from the reference, where it lies, and run unmodified on the evaluating numpy stand-in for `mx.sym`
(tests/mx_numpy_eval.py): models/FCOS/input.py make_fcos_gt (with its CustomOps make_fcos_gt_preparation and
prepare_fcos_cls_gt) and models/FCOS/loss.py make_sigmoid_focal_loss, make_binary_cross_entropy_loss (loss and
`grad` symbols) and IoULoss (forward).  The masks in front of the losses are formed as FCOSFPNHead.get_loss forms
them (models/FCOS/builder.py:217-226).
-> tests/golden/fcos_head.npz: the inputs of the target cases and every result (inputs of the loss cases are
regenerated from seeds by tests/fcos_ref.py)."""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests import fcos_ref, mx_numpy_eval  # noqa: E402

IGNORE = -1


def run_targets(c):
    param = types.SimpleNamespace(stride=c["strides"], stages=None, data_size=list(c["data_size"]))
    with mx_numpy_eval.modules(REF, param) as m:
        mod = importlib.import_module("models.FCOS.input")
        A = mx_numpy_eval.Arr
        cen, cls, off = mod.make_fcos_gt(A(c["gt_bbox"]), A(c["im_info"]), IGNORE, IGNORE, c["K"])
        return cen.v, cls.v, off.v


def run_losses(c):
    tg, N = c["tg"], c["cls"].shape[0]
    with mx_numpy_eval.modules(REF, None) as m:
        mod = importlib.import_module("models.FCOS.loss")
        mx, A = m.mx, mx_numpy_eval.Arr
        ignore_label, ignore_offset = A(np.full((1, 1), IGNORE)), A(np.full((1, 1, 1), IGNORE))
        cls_labels, cen_labels, off_labels = A(tg["cls_gt"]), A(tg["centerness"]), A(tg["offset"])
        # builder.py:217-226
        mask = mx.sym.broadcast_not_equal(lhs=cls_labels, rhs=ignore_label)
        cls_loss = mod.make_sigmoid_focal_loss(gamma=c["gamma"], alpha=c["alpha"], logits=A(c["cls"].reshape(N, -1)),
                                               labels=cls_labels, nonignore_mask=mask)
        d_cls = mx.customs[-1][2]["grad"]
        mask = mx.sym.broadcast_logical_and(lhs=mx.sym.broadcast_not_equal(lhs=cen_labels, rhs=ignore_label),
                                            rhs=mx.sym.broadcast_greater(lhs=cen_labels, rhs=mx.sym.full((1, 1), 0)))
        ctr_loss = mod.make_binary_cross_entropy_loss(A(c["ctr"].reshape(N, -1)), cen_labels, mask)
        d_ctr = mx.customs[-1][2]["grad"]
        off_loss = mod.IoULoss(A(c["off"]), off_labels, ignore_offset, cen_labels, name="offset_loss")
        return (np.concatenate([ctr_loss.v.reshape(1), cls_loss.v.reshape(1), off_loss.v.reshape(1)]),
                d_cls.v.reshape(c["cls"].shape), d_ctr.v.reshape(c["ctr"].shape))


def main():
    out = {}
    names = []
    for name, c in fcos_ref.target_cases():
        cen, cls, off = run_targets(c)
        names.append(name)
        out["t/%s/gt_bbox" % name], out["t/%s/im_info" % name] = c["gt_bbox"], c["im_info"]
        out["t/%s/geom" % name] = np.array(list(c["data_size"]) + [c["K"]] + list(c["strides"]), np.int64)
        out["t/%s/centerness" % name], out["t/%s/offset" % name] = cen, off
        out["t/%s/cls_gt" % name] = cls.astype(np.int8)          # the values are 0, 1 and ignore_label = -1
        assert np.array_equal(cls.astype(np.int8).astype(np.float32), cls)
    lnames = []
    for name, c in fcos_ref.loss_cases():
        losses, d_cls, d_ctr = run_losses(c)
        lnames.append(name)
        out["l/%s/losses" % name], out["l/%s/d_cls" % name], out["l/%s/d_ctr" % name] = losses, d_cls, d_ctr
    out["target_cases"], out["loss_cases"] = np.array(names), np.array(lnames)
    path = os.path.join(HERE, "fcos_head.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d target cases, %d loss cases)" % (path, os.path.getsize(path), len(names), len(lnames)))


if __name__ == "__main__":
    main()
