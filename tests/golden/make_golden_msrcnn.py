#!/usr/bin/env python
"""Generate tests/golden/msrcnn_maskiou.npz FROM THE REFERENCE ITSELF.

Run where the reference tree is present:
    python tests/golden/make_golden_msrcnn.py
What is executed from the reference (no source is copied; the class is loaded from the file where it lies):
  models/msrcnn/maskiou_compute.py:10-43  MaskIoUComputeOperator.forward, on a stub `mxnet` whose CustomOp.assign
  stores into a float32 array (what an NDArray of the operator's output dtype does) and whose inputs answer
  asnumpy().  numpy 2 dropped the aliases `np.float` and `np.bool` the file uses: the exec namespace's `np` is a
  view of numpy with both put back (float -> float64, bool -> bool_, their meaning when the file was written).
Stored per case of tests/msrcnn_ref.golden_cases(): the four inputs and the two outputs.
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

from tests import msrcnn_ref as mr  # noqa: E402


class _ND:
    def __init__(self, a):
        self.a = np.array(a, np.float32)

    def asnumpy(self):
        return self.a.copy()


class _CustomOp:
    def assign(self, dst, req, src):
        dst.a[...] = src          # float32 storage: the rounding an NDArray assignment performs


def load_operator():
    path = os.path.join(REF, "models", "msrcnn", "maskiou_compute.py")
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "MaskIoUComputeOperator"]
    assert len(body) == 1, path
    mx = types.SimpleNamespace(operator=types.SimpleNamespace(CustomOp=_CustomOp))
    np_old = types.ModuleType("numpy_with_old_aliases")
    np_old.__dict__.update(np.__dict__)
    np_old.float, np_old.bool = float, np.bool_
    env = {"mx": mx, "np": np_old}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), env)
    return env["MaskIoUComputeOperator"]


def main():
    Op = load_operator()
    out = {}
    with np.errstate(all="ignore"):
        for name, prob, target, ratio, cls in mr.golden_cases():
            R = prob.shape[0]
            o = [_ND(np.zeros((R, 1))), _ND(np.zeros((R, 1)))]
            Op().forward(True, ["write", "write"], [_ND(prob), _ND(target), _ND(ratio), _ND(cls)], o, [])
            for k, v in (("prob", prob), ("target", target), ("ratio", ratio), ("cls", cls),
                         ("iou_target", o[0].a.reshape(-1)), ("weight", o[1].a.reshape(-1))):
                out["%s/%s" % (name, k)] = np.asarray(v, np.float32)
    path = os.path.join(HERE, "msrcnn_maskiou.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
