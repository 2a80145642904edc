#!/usr/bin/env python
"""Pins for the final detections from THE REFERENCE'S OWN PYTHON, executed where it lies.

Run in the build container (needs the reference tree):
    python tests/golden/make_golden_det_post.py
Loaded by name with `ast`, nothing copied:
  operator_py/nms.py    nms, set_nms, py_nms_wrapper, py_set_nms_wrapper   (make_golden_py_twins.load_defs; the
                        module's Cython import is never run)
  detection_test.py     the nested do_nms (:233-260), found by walking the tree; its free names output_dict,
                        pTest, pRpn, coco and nms are small stand-ins in the namespace it is compiled into
detection_test.py:174-178 (scale, drop the background) and :272-290 (the cut) are inline statements of a long
script, not functions; scale_and_strip() and cut() below restate those few lines, line numbers cited, with one
addition: every result entry also carries its det row, so the fixture holds x1,y1,x2,y2 and not the COCO
x,y,w,h the script converts to.

Inputs come from tests/det_post_cases.py (seeded; only their SHA-256 is stored).  Per case the fixture holds
the cut's result BEST FIRST (the script's list is ascending: reversed here, padded with zero rows of class -1)
with the counts, per (image, class) the rows do_nms's nms kept, in its order, as image rows, and the dtype of
the det that reached nms.  Scores over the threshold are pairwise distinct per image (asserted by the case
builder), so the unstable argsort and the cut have one answer.  Metadata: the numpy version, and the twin's
time per call on ONE host core for the timed shapes.
-> tests/golden/det_post.npz
"""
import ast
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

from make_golden_py_twins import load_defs  # noqa: E402
from tests import det_post_cases as cases  # noqa: E402


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def scale_and_strip(info, cls, box):
    scale = info[2]                                   # detection_test.py:174
    box = box / scale                                 # :175
    cls = cls[:, 1:]                                  # :176
    box = box[:, 4:] if box.shape[1] != 4 else box    # :178
    return cls, box


def cut(det_xyxys, iid, max_det_per_image):
    result = []                                       # :273
    for cid in det_xyxys:                             # :274
        det = det_xyxys[cid]
        if det.shape[0] == 0:                         # :276-277
            continue
        scores = det[:, 4]                            # :278
        result += [{'image_id': int(iid), 'category_id': int(cid), 'score': float(scores[k]),   # :283-289
                    'det': det[k]} for k in range(det.shape[0])]
    return sorted(result, key=lambda x: x['score'])[-max_det_per_image:]   # :290


class Twin:
    def __init__(self):
        self.nms_env = {"np": np}
        load_defs(os.path.join(REF, "operator_py", "nms.py"),
                  ["nms", "set_nms", "py_nms_wrapper", "py_set_nms_wrapper"], self.nms_env)
        path = os.path.join(REF, "detection_test.py")
        tree = ast.parse(open(path).read())
        found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == "do_nms"]
        assert len(found) == 1, len(found)
        self.do_nms_code = compile(ast.Module(body=found, type_ignores=[]), path, "exec")

    def do_nms_src(self, env):
        """the nested do_nms (:233-260) compiled into env: its free names resolve there"""
        exec(self.do_nms_code, env)
        return env["do_nms"]

    def forward(self, cls, box, scale, par, seen=None):
        """the reference's path for a batch: per image (stripped cls, scaled box, do_nms's dict, the cut's list)"""
        K = cls.shape[2]
        wrapper = {"nms": "py_nms_wrapper", "set_nms": "py_set_nms_wrapper"}[par["nms_type"]]   # :226-231
        inner = self.nms_env[wrapper](par["nms_thr"])

        def nms(det):
            if seen is not None:
                seen.append(det.dtype)
            return inner(det)
        res = []
        for b in range(cls.shape[0]):
            info = np.array([800, 1333, 1.0 if scale is None else scale[b]], np.float32)
            c, x = scale_and_strip(info, cls[b], box[b])
            env = {
                "np": np, "nms": nms,
                "output_dict": {b: dict(bbox_xyxy=x, cls_score=c)},
                "pTest": types.SimpleNamespace(min_det_score=par["min_det_score"],
                                               nms=types.SimpleNamespace(type=par["nms_type"], thr=par["nms_thr"])),
                "pRpn": types.SimpleNamespace(proposal=types.SimpleNamespace(post_nms_top_n=par["set_period"])),
                "coco": types.SimpleNamespace(getCatIds=lambda: list(range(K - 1))),
            }
            _, rec = self.do_nms_src(env)(b)
            res.append((c, x, rec["det_xyxys"], cut(rec["det_xyxys"], b, par["max_det_per_image"])))
        return res

    def run(self, cls, box, scale, par):
        """-> (out (B,top,6) best first, counts (B), kept_counts (B,C), kept_rows flat, dtype seen by nms)"""
        B, R, K = cls.shape
        top = par["max_det_per_image"]
        seen = []
        res = self.forward(cls, box, scale, par, seen)
        out = np.zeros((B, top, 6), np.float32)
        out[:, :, 5] = -1
        counts = np.zeros(B, np.int32)
        kept_counts = np.zeros((B, K - 1), np.int32)
        kept_rows = []
        for b in range(B):
            c, x, dets, result = res[b]
            for cid in range(K - 1):
                det = dets[cid]
                s = c[:, cid]
                valid = np.where(s > par["min_det_score"])[0]
                at = {v.tobytes(): i for i, v in zip(valid, s[valid])}   # distinct scores: score -> row
                idx = np.array([at[np.float32(v).tobytes()] for v in det[:, 4]], np.int64)
                cb = x if x.shape[1] == 4 else x[:, cid * 4:(cid + 1) * 4]
                assert np.array_equal(det[:, :5], np.concatenate((cb[idx].reshape(-1, 4), s[idx, None]), 1))
                if par["nms_type"] == "set_nms":
                    assert np.array_equal(det[:, 5], idx % par["set_period"])
                kept_counts[b, cid] = len(idx)
                kept_rows.append(idx)
            result = result[::-1]
            counts[b] = len(result)
            for t, r in enumerate(result):
                out[b, t, :5] = r["det"][:5]
                out[b, t, 5] = r["category_id"]
                assert np.float32(r["score"]) == out[b, t, 4]
        flat = np.concatenate(kept_rows) if kept_rows else np.zeros(0, np.int64)
        assert R < 32768 and len(set(seen)) <= 1
        return out, counts, kept_counts, flat.astype(np.int16), str(seen[0]) if seen else ""


def main():
    twin = Twin()
    out = {"numpy_version": np.array(np.__version__), "twin_cores": np.array(1)}
    for name in cases.CASES:
        cls, box, scale, par = cases.case(name)
        dets, counts, kc, rows, seen = twin.run(cls, box, scale, par)
        out[name + "/inputs_sha256"] = np.array(sha256(cls, box, scale))
        out[name + "/param"] = np.array([par["max_det_per_image"], par["min_det_score"], par["nms_thr"],
                                         {"nms": 0, "set_nms": 1}[par["nms_type"]],
                                         par["set_period"]], np.float64)
        out[name + "/out_dets"], out[name + "/out_counts"] = dets, counts
        out[name + "/kept_counts"], out[name + "/kept_rows"] = kc, rows
        out[name + "/nms_input_dtype"] = np.array(seen)
        out[name + "/candidates"] = (cls[:, :, 1:] > par["min_det_score"]).sum(1).astype(np.int32)
        line = "%-11s B=%d R=%d K=%d max candidates %d kept %d detections %s nms saw %s" % (
            name, cls.shape[0], cls.shape[1], cls.shape[2], int(out[name + "/candidates"].max()), int(kc.sum()),
            counts.tolist(), seen)
        if name in cases.TIMED:
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                twin.forward(cls, box, scale, par)
                t.append(time.perf_counter() - t0)
            out[name + "/twin_ms"] = np.array(sorted(t)[len(t) // 2] * 1e3)
            line += " twin %.1f ms" % float(out[name + "/twin_ms"])
        print(line)
    path = os.path.join(HERE, "det_post.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes; numpy", np.__version__)


if __name__ == "__main__":
    main()
