#!/usr/bin/env python
"""Golden fixtures for the CrowdHuman double-prediction head, produced by THE REFERENCE'S OWN FILES.

Run where the reference tree is present (needs oracle/_ref/bbox*.so from oracle/build_ref.py):
    python tests/golden/make_golden_crowdhuman.py
Executed from the reference, where it lies (functions / classes loaded by name with `ast`, nothing copied):
  models/crowdhuman/bbox_target.py      _sample_proposal, _expand_bbox_targets, BboxTargetOperator   (mode 0)
  models/crowdhuman/bbox_sec_target.py  _sample_proposal, _expand_bbox_targets, BboxTargetOperator   (mode 1)
  operator_py/detectron_bbox_utils.py   bbox_transform_inv
  models/crowdhuman/softmax_entropy_op.py  SoftmaxEntropyOperator, on the numpy-evaluating stand-in
  (tests/mx_numpy_eval_nd.py) with mx.nd.one_hot / softmax / log / zeros_like added in float32
and the reference's compiled Cython bbox_overlaps_cython.  np.random is the real numpy generator, seeded per case; the
fixture stores the generator state after the call.  bbox_transform_inv is called through a wrapper that records its
operands, from which tests/crowdhuman_ref.encode_truth forms the float64 truth of the dw / dh columns.
Every stored case except `short` is asserted to fill all image_rois rows.
-> tests/golden/crowdhuman_target.npz, tests/golden/crowdhuman_softmax_entropy.npz
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)

from tests import crowdhuman_ref as cr  # noqa: E402
from tests import mx_numpy_eval_nd as mnd  # noqa: E402

FILES = {0: "bbox_target.py", 1: "bbox_sec_target.py"}
NAMES = ("sampled_proposal", "bbox_cls", "bbox_target", "bbox_target_weight", "bbox_sec_cls", "bbox_sec_target",
         "bbox_sec_target_weight")


class _ND:
    def __init__(self, a):
        self.a = np.array(a, np.float32)

    def asnumpy(self):
        return self.a.copy()


class _CustomOp:
    def assign(self, dst, req, src):
        dst.append(np.asarray(src, np.float32))


def load_defs(path, names, env):
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names, [n.name for n in body])
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), env)
    return env


def reference_env(mode, record):
    from oracle._ref import bbox as ref_bbox
    util = load_defs(os.path.join(REF, "operator_py", "detectron_bbox_utils.py"), ["bbox_transform_inv"], {"np": np})

    def transform(boxes, gt_boxes, inv_stds):
        record.append((np.array(boxes), np.array(gt_boxes)))
        return util["bbox_transform_inv"](boxes, gt_boxes, inv_stds)

    mx = types.SimpleNamespace(operator=types.SimpleNamespace(CustomOp=_CustomOp))
    env = {"np": np, "npr": np.random, "mx": mx, "bbox_overlaps": ref_bbox.bbox_overlaps_cython,
           "bbox_transform_inv": transform}
    return load_defs(os.path.join(REF, "models", "crowdhuman", FILES[mode]),
                     ["_sample_proposal", "_expand_bbox_targets", "BboxTargetOperator"], env)


def make_operator(env, mode, cfg):
    args = [cfg["num_reg_class"], cfg["add_gt_to_proposal"], cfg["image_rois"], cfg["fg_fraction"], cfg["fg_thresh"],
            cfg["bg_thresh_hi"], cfg["bg_thresh_lo"], cfg["bbox_target_std"]]
    return env["BboxTargetOperator"](*(args + [True] if mode == 0 else args))


def truth_of(env, record, outs, cfg, mode):
    """float64 truth and T of the expanded targets, through the reference's own _expand_bbox_targets"""
    inv = [1.0 / s for s in cfg["bbox_target_std"]]
    B, S = outs[1].shape
    res = []
    for h in range(2 if mode == 1 else 1):
        cls = outs[1 + 3 * h]
        cls = (cls > 0).astype(np.float64) if cfg["num_reg_class"] == 2 else cls.astype(np.float64)
        tt, TT = [], []
        for b in range(B):
            boxes, gts = record[b * (mode + 1) + h]
            t, T = cr.encode_truth(boxes, gts, inv)
            tt.append(env["_expand_bbox_targets"](np.concatenate([cls[b][:, None], t], 1), cfg["num_reg_class"])[0])
            TT.append(env["_expand_bbox_targets"](np.concatenate([cls[b][:, None], T], 1), cfg["num_reg_class"])[0])
        res += [np.array(tt), np.array(TT)]
    return res


def run_case(case, out, seed=None, prefix=None):
    """the operator's forward on one case; seeds np.random unless seed is False"""
    mode, cfg, name = case["mode"], case["cfg"], prefix or case["name"]
    record = []
    env = reference_env(mode, record)
    if seed is not False:
        np.random.seed(seed)
    outs = []
    n_out = 7 if mode == 1 else 4
    store = [[] for _ in range(n_out)]
    make_operator(env, mode, cfg).forward(True, ["write"] * n_out, [_ND(case["proposal"]), _ND(case["gt"])], store, [])
    outs = [s[0] for s in store]
    B, S = case["proposal"].shape[0], cfg["image_rois"]
    assert outs[0].shape == (B, S, 4) and outs[1].shape == (B, S), (name, outs[0].shape)   # every image filled its rows
    state = np.random.get_state()
    out[name + "/proposal"], out[name + "/gt"] = case["proposal"], case["gt"]
    out[name + "/seed"] = np.array([-1 if seed is False else seed], np.int64)
    for k, v in zip(NAMES, outs):
        out["%s/%s" % (name, k)] = v
    out[name + "/mt_key"], out[name + "/mt_pos"] = state[1].astype(np.uint32), np.array([state[2]], np.int32)
    tr = truth_of(env, record, outs, cfg, mode)
    for k, v in zip(("target_truth", "target_T", "sec_target_truth", "sec_target_T"), tr):
        out["%s/%s" % (name, k)] = v
    fg = [int((outs[1][b] > 0).sum()) for b in range(B)]
    print("%-24s mode %d  rows %s  fg rows %s  mt_pos %d" % (name, mode, outs[0].shape, fg, state[2]))


def run_short(case, out, seed):
    """the reference's per-image _sample_proposal on a case whose first image cannot fill its rows (the operator's
    np.array stacking would fail): the clean-up of forward() (padding rows out, gt boxes appended) is done here"""
    mode, cfg, name = case["mode"], case["cfg"], case["name"]
    record = []
    env = reference_env(mode, record)
    np.random.seed(seed)
    inv = [1.0 / s for s in cfg["bbox_target_std"]]
    for b in range(case["proposal"].shape[0]):
        gt = case["gt"][b][case["gt"][b][:, 4] != -1]
        prop = case["proposal"][b][case["proposal"][b][:, 3] != 0]
        if cfg["add_gt_to_proposal"]:
            prop = np.append(prop, gt[:, :4], axis=0)
        args = [prop, gt.copy(), cfg["image_rois"], cfg["fg_fraction"], cfg["fg_thresh"], cfg["bg_thresh_hi"],
                cfg["bg_thresh_lo"], inv, cfg["num_reg_class"]]
        res = env["_sample_proposal"](*(args + [True] if mode == 0 else args))
        for k, v in zip(NAMES, res):
            out["%s/%d/%s" % (name, b, k)] = np.asarray(v, np.float32)
        print("%-24s image %d rows %d" % (name, b, len(res[0])))
    assert len(out[name + "/0/sampled_proposal"]) < cfg["image_rois"] == len(out[name + "/1/sampled_proposal"])
    state = np.random.get_state()
    out[name + "/proposal"], out[name + "/gt"] = case["proposal"], case["gt"]
    out[name + "/mt_key"], out[name + "/mt_pos"] = state[1].astype(np.uint32), np.array([state[2]], np.int32)


def softmax_entropy_fixture():
    """the reference's softmax_entropy forward / backward, evaluated in float32 numpy"""
    mx, _X = mnd.make_mx()
    ND, F = mnd.ND, np.float32

    def softmax(d, axis=-1):
        x = d.v.astype(F)
        e = np.exp(x - x.max(axis, keepdims=True))
        return ND((e / e.sum(axis, keepdims=True, dtype=F)).astype(F))

    def one_hot(label, depth):
        idx = label.v.astype(np.int64)
        return ND((np.arange(depth)[None] == idx[:, None]).astype(F))

    mx.nd.softmax, mx.nd.one_hot = softmax, one_hot
    mx.nd.log = lambda d: ND(np.log(d.v).astype(F))
    mx.nd.zeros_like = lambda d: ND(np.zeros_like(d.v))
    env = load_defs(os.path.join(REF, "models", "crowdhuman", "softmax_entropy_op.py"), ["SoftmaxEntropyOperator"],
                    {"np": np, "mx": mx})
    out = {}
    for name, x, y, og in cr.ce_fixture_inputs():
        op = env["SoftmaxEntropyOperator"]()
        fwd, bwd = [[]], [[], []]
        with np.errstate(all="ignore"):
            op.forward(True, ["write"], [ND(x), ND(y)], fwd, [])
            op.backward(["write", "write"], [ND(np.full(x.shape, og, F))], [ND(x), ND(y)], fwd, bwd, [])
        out[name + "/forward"], out[name + "/backward"] = fwd[0][0].v.astype(F), bwd[0][0].v.astype(F)
    path = os.path.join(HERE, "crowdhuman_softmax_entropy.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


def main():
    out = {}
    cases = cr.target_cases()
    for i, case in enumerate(cases):
        run_case(case, out, seed=1000 + i)
    # two consecutive calls on one stream: config-small-m1 again, then the second call without reseeding
    first = [c for c in cases if c["name"] == "config-small-m1"][0]
    run_case(first, out, seed=4242, prefix="two-calls/0")
    run_case(cr.two_call_inputs(), out, seed=False, prefix="two-calls/1")
    for mode in (0, 1):
        run_short(cr.short_case(mode), out, seed=77 + mode)
    path = os.path.join(HERE, "crowdhuman_target.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))
    softmax_entropy_fixture()


if __name__ == "__main__":
    main()
