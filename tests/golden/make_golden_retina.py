#!/usr/bin/env python
"""Golden fixture for GenProposalRetina, produced by THE REFERENCE'S OWN PYTHON TWIN of the op.

Run in the build container (needs /root/reference):
    python tests/golden/make_golden_retina.py
Executed from the reference, where it lies (classes/functions loaded by name with `ast`, nothing
copied): models/retinanet/decode_retina.py AnchorTarget2DParam / DecodeRetinaOperator.forward,
models/retinanet/input.py PyramidAnchorTarget2DBase / PyramidAnchorTarget2D (the twin builds its own
anchors from them), core/detection_input.py DetectionAugmentation / AnchorTarget2D and
operator_py/bbox_transform.py clip_boxes / nonlinear_pred.  mx.operator.CustomOp is a small stand-in
whose assign() stores the outputs.

Inputs: one image, five seeded levels (strides 8..128) of sigmoid(N(-2, 1)) scores (continuous: no
ties at the per-level cut-off) and N(0, 0.2) deltas, A = 9, K = 3 classes, per_level_top_n = 50,
thresh 0.05 (0 at stride 128, as decode_retina.py and models/retinanet/builder.py:373 set it).
The fixture also stores the twin's per-level anchors tiled like GenAnchor's output and whether they
equal the repository's GenAnchor oracle for the same scales ("anchors_equal_gen_anchor").
-> tests/golden/retina_decode.npz
"""
import ast
import copy
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

STRIDES = (8, 16, 32, 64, 128)
SHAPES = ((24, 32), (12, 16), (6, 8), (3, 4), (2, 2))  # a 192x256 image
SCALES = (4 * 2 ** 0, 4 * 2 ** (1.0 / 3.0), 4 * 2 ** (2.0 / 3.0))
RATIOS = (0.5, 1.0, 2.0)
K = 3
TOP_N = 50
THRESH = 0.05
BOX_ATOL = 1e-3  # the twin decodes in float64 from float32 anchors; the op in float32


def load_defs(path, names, env):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names, [n.name for n in body])
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), env)
    return env


class _NDArray:
    def __init__(self, a):
        self._a = np.asarray(a)
        self.shape = self._a.shape

    def asnumpy(self):
        return self._a


class _CustomOp:
    def __init__(self):
        self.outputs = {}

    def assign(self, dst, req, src):
        self.outputs[dst] = np.asarray(src)


def reference_twin():
    npx = types.ModuleType("numpy")  # numpy with the np.float alias the reference still uses
    npx.__dict__.update(np.__dict__)
    npx.float = float
    bt = {"np": npx, "BBOX_XFORM_CLIP": np.log(1000.0 / 16.0)}
    load_defs(os.path.join(REF, "operator_py", "bbox_transform.py"), ["clip_boxes", "nonlinear_pred"], bt)
    env = {"np": npx, "copy": copy, "bbox_overlaps_cython": None, "bbox_transform": None}
    load_defs(os.path.join(REF, "core", "detection_input.py"), ["DetectionAugmentation", "AnchorTarget2D"], env)
    load_defs(os.path.join(REF, "models", "retinanet", "input.py"),
              ["PyramidAnchorTarget2DBase", "PyramidAnchorTarget2D"], env)
    env.update(mx=types.SimpleNamespace(operator=types.SimpleNamespace(CustomOp=_CustomOp)),
               clip_boxes=bt["clip_boxes"], decode_boxes=bt["nonlinear_pred"])
    load_defs(os.path.join(REF, "models", "retinanet", "decode_retina.py"),
              ["AnchorTarget2DParam", "DecodeRetinaOperator"], env)
    return env


def main():
    env = reference_twin()
    rs = np.random.RandomState(2024)
    A = len(SCALES) * len(RATIOS)
    im_info = np.array([[SHAPES[0][0] * 8, SHAPES[0][1] * 8, 1.0]], np.float32)
    cls_l, box_l = [], []
    for H, W in SHAPES:
        cls_l.append((1 / (1 + np.exp(-rs.normal(-2.0, 1.0, (1, A * K, H, W))))).astype(np.float32))
        box_l.append((rs.standard_normal((1, 4 * A, H, W)) * 0.2).astype(np.float32))
    op = env["DecodeRetinaOperator"](STRIDES, SCALES, RATIOS, TOP_N, THRESH)
    ins = [_NDArray(x) for x in cls_l + box_l + [im_info]]
    op.forward(False, ["write", "write"], ins, ["boxes", "scores"], [])
    boxes, scores = op.outputs["boxes"], op.outputs["scores"]
    from oracle import pyoracle as orc
    out = {"strides": np.array(STRIDES), "top_n": np.array(TOP_N), "im_info": im_info,
           "thresh": np.array([0.0 if s == max(STRIDES) else THRESH for s in STRIDES], np.float32),
           "boxes": boxes.astype(np.float32), "scores": scores.astype(np.float32),
           "box_atol": np.array(BOX_ATOL)}
    equal = True
    for (H, W), s, c, b in zip(SHAPES, STRIDES, cls_l, box_l):
        # the twin's own arithmetic (decode_retina.py: float32 shifts += its float64 cell anchors),
        # laid out in GenAnchor's row order (h*W + w)*A + a
        base = op._anchors_fpn["stride%s" % s]                                # (A, 4)
        shift = np.array([[x * s, y * s, x * s, y * s] for y in range(H) for x in range(W)], np.float32)
        anc = np.repeat(shift, A, axis=0)
        anc += np.tile(base, (H * W, 1))
        equal &= bool(np.array_equal(anc, orc.gen_anchor(H, W, s, SCALES, RATIOS)))
        thr = 0.0 if s == max(STRIDES) else THRESH
        out["cls_%d" % s], out["bbox_%d" % s], out["anchors_%d" % s] = c, b, anc
        out["count_%d" % s] = np.array(min(TOP_N, int((c > thr).sum())))
    out["anchors_equal_gen_anchor"] = np.array(equal)
    print("anchors equal GenAnchor:", equal)
    path = os.path.join(HERE, "retina_decode.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
