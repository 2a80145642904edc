#!/usr/bin/env python
"""Golden fixtures for the RetinaNet anchor targets, produced by THE REFERENCE'S OWN CLASSES.

Run where the reference checkout and oracle/_ref/bbox*.so (oracle/build_ref.py) exist:
    python tests/golden/make_golden_retina_target.py
Executed from the reference, where it lies (classes loaded by name with `ast`, nothing copied):
models/retinanet/input.py PyramidAnchorTarget2DBase / PyramidAnchorTarget2D (:33-199) over
core/detection_input.py AnchorTarget2D, operator_py/bbox_transform.py nonlinear_transform and the
reference's compiled Cython bbox_overlaps_cython.
-> tests/golden/retina_target.npz (inputs are regenerated from seeds by tests/retinacases.py)

Storage: labels in full (int8: classes are < 128); targets and weights of the small cases in full,
of the 200 700-anchor cases as the SHA-256 of their float32 bytes in both layouts plus every 53rd
row of the flat layout (a committed file stays below 1 MiB)."""
import copy
import hashlib
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from tests import retinacases  # noqa: E402
from make_golden_rpn import load_defs, make_param  # noqa: E402

SAMPLE = 53


def reference_classes():
    from oracle._ref import bbox as ref_bbox
    env = {"np": np, "copy": copy, "bbox_overlaps_cython": ref_bbox.bbox_overlaps_cython}
    load_defs(os.path.join(REF, "operator_py", "bbox_transform.py"), ["nonlinear_transform"], env)
    env["bbox_transform"] = env["nonlinear_transform"]  # models/retinanet/input.py:8
    load_defs(os.path.join(REF, "core", "detection_input.py"), ["DetectionAugmentation", "AnchorTarget2D"], env)
    load_defs(os.path.join(REF, "models", "retinanet", "input.py"),
              ["PyramidAnchorTarget2DBase", "PyramidAnchorTarget2D"], env)
    return env


def sha(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).digest(), np.uint8)


def main():
    env = reference_classes()
    out = {}
    for name, case in sorted(retinacases.CASES.items()):
        cfg = dict(case["cfg"], image_anchor=None, pos_fraction=None)
        op = env["PyramidAnchorTarget2D"](make_param(cfg))
        for i, (im_info, gt) in enumerate(retinacases.inputs(case)):
            t0 = time.perf_counter()
            lab, fg, tgt, wgt = op.apply({"im_info": im_info, "gt_bbox": gt.copy()})
            dt = time.perf_counter() - t0
            flab, ftgt, fwgt = op.anchor_target_2d.apply({"im_info": im_info, "gt_bbox": gt.copy()})
            lab, flab = np.asarray(lab, np.float32), np.asarray(flab, np.float32)
            assert np.array_equal(lab, lab.astype(np.int8).astype(np.float32))
            k = "%s/%d/" % (name, i)
            out[k + "label"] = lab.astype(np.int8)
            out[k + "label_flat"] = flab.astype(np.int8)
            out[k + "fg_count"] = np.array([fg], np.float32)
            out[k + "shape"] = np.array(tgt.shape, np.int64)
            if lab.size <= 4096:
                out[k + "target"], out[k + "weight"] = np.float32(tgt), np.float32(wgt)
                out[k + "target_flat"], out[k + "weight_flat"] = np.float32(ftgt), np.float32(fwgt)
            else:
                for key, a in (("target", tgt), ("weight", wgt), ("target_flat", ftgt), ("weight_flat", fwgt)):
                    out[k + key + "_sha256"] = sha(a)
                out[k + "target_flat_sample"] = np.float32(ftgt)[::SAMPLE]
            out[k + "host_seconds"] = np.array([dt], np.float64)
            print("%-26s N %6d  fg_count %6d  labels>0 %6d  ignore %6d  classes %s  host %.3f s" % (
                name, lab.size, int(fg), int((lab > 0).sum()), int((lab < 0).sum()),
                np.unique(lab[lab > 0]).astype(int).tolist()[:6], dt))
    np.savez_compressed(os.path.join(HERE, "retina_target.npz"), **out)


if __name__ == "__main__":
    main()
