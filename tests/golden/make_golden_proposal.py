#!/usr/bin/env python
"""Golden fixture for _contrib_Proposal_v2 / _contrib_Proposal, produced by THE REFERENCE'S OWN .cu
forwards run through the MXNet stand-in, plus a pin of the unfiltered path to the reference's Python
twins.

Run in the build container (needs the reference tree):
    python tests/golden/make_golden_proposal.py
1. operator_cxx/contrib/proposal_v2.{cc,cu} and proposal.{cc,cu} are compiled where they lie by
   oracle/build_ref_cxx.build_lib, into a temporary directory that is deleted afterwards (build_ref_cxx.OUT
   and refmx._REF are pointed there; nothing lands in oracle/_ref/), and run with ctx="gpu" (the .cu
   Forward on the stand-in's CUDA emulation).  A cross-check through the shim, not a pin: the emulated
   expf may differ from float32(exp(float64)) by 1 ulp.
2. The Python-twin pin: operator_py/bbox_transform.py nonlinear_pred + clip_boxes and operator_py/nms.py
   nms (keeps ovr <= thresh: v1/v2's strict >; it returns the kept rows, not indices), loaded by name with `ast` and run where they lie, over the
   grid anchors of tests/proposal_ref.py, on an unfiltered case (min size 0, no scale filter, unpadded,
   distinct scores, |dw|, |dh| < log(1000/16)).  The filters have no Python twin.
Inputs are regenerated from the seeds stored with each case (tests/proposal_ref.rpn_inputs).
-> tests/golden/proposal_ref.npz
"""
import ast
import json
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests import proposal_ref as pr  # noqa: E402

f32 = np.float32
TRI = dict(feature_stride=16, scales=(2., 4., 8., 16., 32.), ratios=(0.5, 1., 2.), threshold=0.7)

# name -> (op, seed, B, A-grid (H, W), im (h, w, scale) per image or None, params)
CASES = {
    # Trident ranges, narrow enough that the -1 run straddles pre
    "trident_ranges": ("v2", 1, 3, (20, 30), None,
                       dict(TRI, rpn_pre_nms_top_n=3000, rpn_post_nms_top_n=300, rpn_min_size=0,
                            filter_scales=True), [(0, 40), (30, 60), (50, 1e5)]),
    "all_filtered": ("v2", 2, 2, (12, 16), None,
                     dict(TRI, rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=200, rpn_min_size=0,
                          filter_scales=True), [(5000, 6000), (2000, 3000)]),
    "padded": ("v2", 3, 2, (20, 30), [(250, 400, 1.0), (307, 455, 1.0)],
               dict(TRI, rpn_pre_nms_top_n=3000, rpn_post_nms_top_n=300, rpn_min_size=0,
                    filter_scales=True), [(0, 90), (30, 160)]),
    "min_size_scale": ("v2", 4, 2, (20, 30), [(320, 480, 1.5), (320, 480, 0.75)],
                       dict(TRI, rpn_pre_nms_top_n=3000, rpn_post_nms_top_n=300, rpn_min_size=16,
                            filter_scales=False), [(0, 1e5), (0, 1e5)]),
    "iou_loss": ("v2", 5, 2, (16, 20), None,
                 dict(TRI, rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=300, rpn_min_size=0,
                      filter_scales=True, iou_loss=True), [(0, 90), (30, 160)]),
    "v1_train": ("v1", 6, 2, (10, 12), [(100, 130, 1.0), (160, 192, 1.0)],
                 dict(TRI, rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=600, rpn_min_size=4,
                      is_train=True), None),
    "v1_test": ("v1", 6, 2, (10, 12), [(100, 130, 1.0), (160, 192, 1.0)],
                dict(TRI, rpn_pre_nms_top_n=1000, rpn_post_nms_top_n=600, rpn_min_size=4,
                     is_train=False), None),
}
DELTA_SCALE = {"iou_loss": 6.0}


def case_inputs(name):
    op, seed, B, (H, W), ims, p, vr = CASES[name]
    A = len(p["scales"]) * len(p["ratios"])
    cls, bbox, im = pr.rpn_inputs(seed, B, A, H, W, delta_scale=DELTA_SCALE.get(name, 0.3))
    if ims is not None:
        im = np.asarray(ims, f32)
    vr = None if vr is None else np.asarray(vr, f32)
    return op, cls, bbox, im, vr, p


def run_reference(refmx, name):
    op, cls, bbox, im, vr, p = case_inputs(name)
    kw = dict(rpn_pre_nms_top_n=p["rpn_pre_nms_top_n"], rpn_post_nms_top_n=p["rpn_post_nms_top_n"],
              threshold=p["threshold"], rpn_min_size=p["rpn_min_size"], scales=p["scales"],
              ratios=p["ratios"], feature_stride=p["feature_stride"], output_score=True,
              iou_loss=p.get("iou_loss", False))
    if op == "v2":
        r = refmx.RefOp("proposal_v2", "_contrib_Proposal_v2", filter_scales=p["filter_scales"], **kw)
        out, score = r.forward([cls, bbox, im, vr], ctx="gpu")
    else:
        r = refmx.RefOp("proposal", "_contrib_Proposal", is_train=p["is_train"], **kw)
        out, score = r.forward([cls, bbox, im], ctx="gpu")
    return out, score


def load_defs(path, names, env):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names, [n.name for n in body])
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), env)
    return env


TWIN = dict(seed=7, H=12, W=16, scales=(4., 8., 16.), ratios=(0.5, 1., 2.), stride=16, pre=600,
            post=150, thr=0.7)


def twin_inputs():
    t = TWIN
    A = len(t["scales"]) * len(t["ratios"])
    rs = np.random.RandomState(t["seed"])
    count = A * t["H"] * t["W"]
    fg = (rs.permutation(count).astype(np.float64) / count).astype(f32)  # distinct scores
    fg = fg.reshape(t["H"], t["W"], A).transpose(2, 0, 1)
    cls = np.concatenate([f32(1) - fg, fg], 0)[None].astype(f32)
    bbox = np.clip(rs.standard_normal((1, 4 * A, t["H"], t["W"])) * 0.3, -2.0, 2.0).astype(f32)
    im = np.asarray([[t["H"] * 16, t["W"] * 16, 1.0]], f32)
    return cls, bbox, im


def python_twin():
    """nonlinear_pred + clip_boxes over the grid anchors, stable descending top-pre, nms (<= thr kept)."""
    npx = types.ModuleType("numpy")
    npx.__dict__.update(np.__dict__)
    npx.float = float
    bt = {"np": npx, "BBOX_XFORM_CLIP": np.log(1000.0 / 16.0)}
    load_defs(os.path.join(REF, "operator_py", "bbox_transform.py"), ["clip_boxes", "nonlinear_pred"], bt)
    nm = {"np": npx}
    load_defs(os.path.join(REF, "operator_py", "nms.py"), ["nms"], nm)
    t = TWIN
    cls, bbox, im = twin_inputs()
    A = len(t["scales"]) * len(t["ratios"])
    anc = pr.anchors_v12(t["stride"], t["scales"], t["ratios"])
    hh, ww, aa = np.meshgrid(np.arange(t["H"]), np.arange(t["W"]), np.arange(A), indexing="ij")
    hh, ww, aa = hh.reshape(-1), ww.reshape(-1), aa.reshape(-1)
    boxes = anc[aa] + (np.stack([ww, hh, ww, hh], 1) * t["stride"]).astype(f32)
    d = bbox[0].reshape(A, 4, t["H"], t["W"])[aa, :, hh, ww]
    pred = bt["nonlinear_pred"](boxes.astype(np.float64), d.astype(np.float64))
    pred = bt["clip_boxes"](pred, (float(im[0, 0]), float(im[0, 1])))
    sc = cls[0, A:][aa, hh, ww].astype(np.float64)
    order = np.argsort(-sc, kind="stable")[:t["pre"]]
    dets = np.hstack([pred[order], sc[order, None]])
    kept = nm["nms"](dets, t["thr"])[:t["post"]]  # the kept rows of dets (despite its docstring)
    pos = {float(v): i for i, v in enumerate(dets[:, 4])}  # scores are distinct
    rows = order[[pos[float(v)] for v in kept[:, 4]]]
    return kept[:, :4].astype(np.float64), kept[:, 4], rows


def main():
    from oracle import build_ref_cxx, refmx
    tmp = tempfile.mkdtemp(prefix="sd_golden_prop_")
    old_out, old_ref = build_ref_cxx.OUT, refmx._REF
    try:
        build_ref_cxx.OUT = refmx._REF = tmp
        work = os.path.join(tmp, "obj")
        os.makedirs(work)
        build_ref_cxx.build_lib("proposal_v2", ["contrib/proposal_v2.cc", "contrib/proposal_v2.cu"], work)
        build_ref_cxx.build_lib("proposal", ["contrib/proposal.cc", "contrib/proposal.cu"], work)
        res = {}
        for name in CASES:
            out, score = run_reference(refmx, name)
            res[name + "/out"] = out
            res[name + "/score"] = score
        refmx._libs.pop("proposal_v2", None)
        refmx._libs.pop("proposal", None)
    finally:
        build_ref_cxx.OUT, refmx._REF = old_out, old_ref
        shutil.rmtree(tmp, ignore_errors=True)
    tb, ts, tr = python_twin()
    res["twin/boxes"], res["twin/score"], res["twin/rows"] = tb, ts, tr
    res["meta"] = np.frombuffer(json.dumps({k: [v[0], v[1], v[2], list(v[3]), v[4], v[5], v[6]]
                                            for k, v in CASES.items()}).encode(), np.uint8)
    path = os.path.join(HERE, "proposal_ref.npz")
    np.savez_compressed(path, **res)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
