#!/usr/bin/env python
"""Pins for the hard NMS and BboxPostProcessing from THE REFERENCE'S OWN PYTHON, executed where it lies.

Run in the build container (needs the reference tree):
    python tests/golden/make_golden_bbox_post.py
Loaded by name with `ast` (tests/golden/make_golden_py_twins.py:load_defs), nothing copied:
  operator_py/nms.py                          nms, py_nms_wrapper   (the module's Cython import is never run)
  models/maskrcnn/bbox_post_processing.py     multiclass_nms, BboxPostProcessingOperator
`mx.operator.CustomOp` is the small stand-in whose assign() stores the outputs.

Inputs come from tests/bbox_post_cases.py (seeded; only their SHA-256 is stored).  Per case the fixture holds
the operator's three outputs and, per (image, foreground class), the rows multiclass_nms's `nms(det)` kept,
in its order, as image row indices (the twin's returned rows are checked to be exactly those input rows).
The scores over the threshold are pairwise distinct in every image (asserted by the case builder), so the
twin's unstable argsort has one answer.  Metadata: the numpy version, and the twin's time per call on ONE
host core for the timed shapes.
-> tests/golden/bbox_post.npz
"""
import hashlib
import os
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from make_golden_py_twins import _CustomOp, _NDArray, load_defs  # noqa: E402
from tests import bbox_post_cases as cases  # noqa: E402


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def reference_twin():
    env = {"np": np}
    load_defs(os.path.join(REF, "operator_py", "nms.py"), ["nms", "py_nms_wrapper"], env)
    env["mx"] = types.SimpleNamespace(operator=types.SimpleNamespace(CustomOp=_CustomOp))
    load_defs(os.path.join(REF, "models", "maskrcnn", "bbox_post_processing.py"),
              ["multiclass_nms", "BboxPostProcessingOperator"], env)
    return env


def twin_forward(env, score, bbox, par):
    op = env["BboxPostProcessingOperator"](par["max_det_per_image"], par["min_det_score"], "nms", par["nms_thr"])
    op.forward(False, ["write"] * 3, [_NDArray(score), _NDArray(bbox)], ["score", "bbox", "cls"], [])
    return op.outputs["score"], op.outputs["bbox"], op.outputs["cls"]


def twin_kept_rows(env, score, bbox, par):
    """What multiclass_nms's loop feeds to and gets from nms(), class by class (its own statements for the
    filter, bbox_post_processing.py:16-25), as image rows."""
    nms = env["py_nms_wrapper"](par["nms_thr"])
    B, R, K = score.shape
    counts = np.zeros((B, K - 1), np.int32)
    rows = []
    for b in range(B):
        for cid in range(K - 1):
            s = score[b, :, cid + 1]
            box = bbox[b] if bbox.shape[2] == 4 else bbox[b, :, 4 * (cid + 1):4 * (cid + 2)]
            valid = np.where(s > par["min_det_score"])[0]
            det = np.concatenate((box[valid], s[valid].reshape(-1, 1)), axis=1).astype(np.float32)
            out = nms(det)
            at = {v.tobytes(): i for i, v in zip(valid, s[valid])}   # distinct scores: score -> row
            idx = np.array([at[v.tobytes()] for v in out[:, 4]], np.int64)
            assert np.array_equal(out, np.concatenate((box[idx].reshape(-1, 4), s[idx, None]), 1))
            counts[b, cid] = len(idx)
            rows.append(idx)
    flat = np.concatenate(rows) if rows else np.zeros(0, np.int64)
    assert R < 32768
    return counts, flat.astype(np.int16)


def main():
    env = reference_twin()
    out = {"numpy_version": np.array(np.__version__), "twin_cores": np.array(1)}
    for name in cases.CASES:
        score, bbox, par = cases.case(name)
        ps, pb, pc = twin_forward(env, score, bbox, par)
        counts, rows = twin_kept_rows(env, score, bbox, par)
        # the stacked kept rows and the operator's outputs tell one story
        assert int(min(counts.sum(1).max(), par["max_det_per_image"])) == int((pc[..., 0] >= 0).sum(1).max())
        out[name + "/inputs_sha256"] = np.array(sha256(score, bbox))
        out[name + "/param"] = np.array([par["max_det_per_image"], par["min_det_score"], par["nms_thr"]], np.float64)
        out[name + "/post_score"], out[name + "/post_bbox"], out[name + "/post_cls"] = ps, pb, pc
        out[name + "/kept_counts"], out[name + "/kept_rows"] = counts, rows
        cand = int((score[:, :, 1:] > par["min_det_score"]).sum())
        out[name + "/candidates"] = np.array(cand)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            twin_forward(env, score, bbox, par)
            t.append(time.perf_counter() - t0)
        out[name + "/twin_ms"] = np.array(sorted(t)[len(t) // 2] * 1e3)
        print("%-13s B=%d R=%d K=%d candidates %d kept %d detections %d twin %.1f ms" % (
            name, score.shape[0], score.shape[1], score.shape[2], cand, int(counts.sum()),
            int((pc >= 0).sum()), float(out[name + "/twin_ms"])))
    # the existing test chain's shape: one image of the Mask R-CNN case
    score, bbox, par = cases.case("mask_r50")
    t = []
    for _ in range(5):
        t0 = time.perf_counter()
        twin_forward(env, score[:1], bbox[:1], par)
        t.append(time.perf_counter() - t0)
    out["mask_r50_b1/twin_ms"] = np.array(sorted(t)[len(t) // 2] * 1e3)
    path = os.path.join(HERE, "bbox_post.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
