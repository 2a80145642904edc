#!/usr/bin/env python
"""Golden fixture for the FCOS test-time decode, produced by THE REFERENCE'S OWN CustomOps.

Run where the reference checkout exists:
    python tests/golden/make_golden_fcos_decode.py
models/FCOS/utils.py is imported from the reference, where it lies, and its two CustomOps get_proposal_single_stage
and get_batch_proposal run unmodified on the evaluating numpy stand-in for `mx.nd` (tests/mx_numpy_eval_nd.py),
chained as FCOSFPNHead.get_all_proposal chains them (models/FCOS/builder.py:240-256; the probabilities are the
cases' inputs).
-> tests/golden/fcos_decode.npz: per case `stage` (the concat), `bbox`, `score`, `cls_id`.  Inputs are regenerated
from seeds by tests/fcos_decode_ref.py.

Asserted per case, so that the fixture does not depend on MXNet's undocumented order among equal keys nor on the
float32 index arithmetic of utils.py:34-36:
  * no two different rows among a level's selected rows, nor the first unselected one, share a fused score; nor do two
    different non-padding rows of an image's concat;
  * (idx % w, idx / w % h, idx / w / h) in float32 equals the integer arithmetic for every idx of every shape."""
import importlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests import fcos_decode_ref as dr, mx_numpy_eval_nd as nd  # noqa: E402

F32 = np.float32


def run_reference(c):
    with nd.modules(REF) as m:
        importlib.import_module("models.FCOS.utils")
        info = nd.ND(c["im_info"])
        stages = []
        for cls, ctr, off, stride in zip(c["cls"], c["ctr"], c["off"], c["strides"]):
            out, = nd.run_custom(m.mx, "get_proposal_single_stage", [nd.ND(ctr.copy()), nd.ND(cls.copy()),
                                 nd.ND(off.copy()), info], pre_nms_top_n=c["top_n"], stride=stride,
                                 pre_nms_thresh=c["thresh"])
            stages.append(out)
        concat = m.mx.nd.concat(*stages, dim=1)
        stage = concat.asnumpy()                       # get_batch_proposal sorts its input in place
        bbox, score, cls_id = nd.run_custom(m.mx, "get_batch_proposal", [concat])
        return dict(stage=stage, bbox=bbox.asnumpy(), score=score.asnumpy(), cls_id=cls_id.asnumpy())


def check_index_arithmetic(shape):
    C, H, W = shape
    idx = np.arange(C * H * W)
    f = idx.astype(F32)
    assert C * H * W <= 1 << 24
    x = np.fmod(f, F32(W)).astype(np.int64)
    y = np.fmod((f / F32(W)).astype(F32), F32(H)).astype(np.int64)
    c = ((f / F32(W)).astype(F32) / F32(H)).astype(F32).astype(np.int64)
    assert np.array_equal(x, idx % W) and np.array_equal(y, idx // W % H) and np.array_equal(c, idx // W // H), shape


def check_no_ties(name, c):
    t = c["top_n"]
    per_image = [[] for _ in range(c["im_info"].shape[0])]
    for cls, ctr in zip(c["cls"], c["ctr"]):
        fused = (cls * ctr).astype(F32)
        for i in range(cls.shape[0]):
            flat = fused[i].reshape(-1)
            count = int((cls[i] > F32(c["thresh"])).sum())
            if count >= t:
                sel = np.sort(flat)[::-1][:t + 1]      # the selected scores and the first unselected one
                per_image[i].append(sel[:t])
            else:
                sel = flat[(cls[i] > F32(c["thresh"])).reshape(-1)]
                per_image[i].append(sel)
            assert len(np.unique(sel)) == len(sel), "%s: tied fused scores inside a level" % name
    for i, parts in enumerate(per_image):
        allrows = np.concatenate(parts)
        assert len(np.unique(allrows)) == len(allrows), "%s: tied fused scores across the levels of image %d" % (name, i)


def check_coverage(name, c, got):
    """the properties a case is there for"""
    stage = got["stage"]
    if name == "mask":
        t = c["top_n"]
        # recompute the unmasked rows: which of the two conditions held
        cls, ctr, off = c["cls"][0], c["ctr"][0], c["off"][0]
        lvl = stage[0, :t]
        assert (lvl[:, 0] == -1).any() and (lvl[:, 0] > 0).any()
        kept = lvl[lvl[:, 0] > 0]
        only_x = (kept[:, 0] >= kept[:, 2]) & ~(kept[:, 1] >= kept[:, 3])
        only_y = ~(kept[:, 0] >= kept[:, 2]) & (kept[:, 1] >= kept[:, 3])
        assert only_x.any() and only_y.any(), "mask: no kept row with exactly one of the two conditions"
        assert (stage[0, t:] == -1).all()
    if name == "clip":
        rows = stage[0][stage[0, :, 0] > 0]
        assert (rows[:, 4] == c["im_info"][0, 1]).any() and (rows[:, 5] == c["im_info"][0, 0]).any()
        assert (rows[:, 2] == 0).any() and (rows[:, 3] == 0).any()
    if name == "pad80":
        s = got["score"][0]
        assert got["cls_id"][0, 0] == 80 and s[0, 80] > 0.5
        assert (s[got["cls_id"][0] == -1, 80] == np.sqrt(F32(1e-20))).all() and (got["cls_id"][0] == -1).any()
        assert not s[:, 0].any()
    if name == "noncand":
        cls, fused = c["cls"][0][0].reshape(-1), (c["cls"][0] * c["ctr"][0]).astype(F32)[0].reshape(-1)
        sel = np.isin(fused, stage[0, :c["top_n"], 1])
        assert (sel & ~(cls > F32(c["thresh"]))).any() and (~sel & (cls > F32(c["thresh"]))).any()
    if name == "config":
        counts = [int((x > F32(c["thresh"])).sum()) for x in c["cls"]]
        assert all(n >= c["top_n"] for n in counts[:3]) and all(0 < n < c["top_n"] for n in counts[3:]), counts


def main():
    out, names = {}, []
    for name, c in dr.cases():
        for cls in c["cls"]:
            check_index_arithmetic(cls.shape[1:])
        check_no_ties(name, c)
        got = run_reference(c)
        check_coverage(name, c, got)
        want = dr.decode(c["cls"], c["ctr"], c["off"], c["im_info"], c["strides"], c["top_n"], c["thresh"])
        for k in ("stage", "bbox", "score", "cls_id"):
            assert got[k].dtype == np.float32 and np.array_equal(got[k], want[k]), (name, k)
            out["%s/%s" % (name, k)] = got[k]
        names.append(name)
    out["cases"] = np.array(names)
    path = os.path.join(HERE, "fcos_decode.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes, %d cases)" % (path, os.path.getsize(path), len(names)))


if __name__ == "__main__":
    main()
