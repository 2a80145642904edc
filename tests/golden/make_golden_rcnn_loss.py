#!/usr/bin/env python
"""Golden fixture for the state block of the R-CNN loss heads, produced by THE REFERENCE'S OWN METRIC CLASSES.

Run where the reference tree is present:
    python tests/golden/make_golden_rcnn_loss.py
Executed from the reference, where it lies (imported from its file, nothing copied):
  core/detection_metric.py   AccWithIgnore, L1 (and their bases EvalMetricWithSummary, LossWithIgnore,
                             FgLossWithIgnore)
on a stand-in for the two things they take from mxnet: mx.metric.EvalMetric (name, sum_metric, num_inst) and
mx.ndarray.argmax_channel.  The stand-in's argmax_channel is the arg-max over axis 1 with the first of equal maxima
(numpy's argmax): the metric compares its result element by element with a label of shape (N, rows), which only an
arg-max over the class axis of a (N, C, rows) prediction can match.  Upstream's source is not vendored, so this
rests on memory of upstream and on that shape argument.
Stored per case: the recorded pred / label / reg_loss arrays and the classes' sum_metric / num_inst.
-> tests/golden/rcnn_loss_metrics.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
F = np.float32


class _ND:
    def __init__(self, a):
        self.a = np.asarray(a)
        self.shape = self.a.shape

    def asnumpy(self):
        return self.a.copy()

    def astype(self, dtype):
        return _ND(self.a.astype(dtype))


class _EvalMetric:
    def __init__(self, name, output_names=None, label_names=None, **kwargs):
        self.name, self.output_names, self.label_names = name, output_names, label_names
        self.reset()

    def reset(self):
        self.num_inst = 0
        self.sum_metric = 0.0


def _argmax_channel(nd):
    return _ND(np.argmax(nd.a, axis=1).astype(F))


def reference_metrics():
    mx = types.ModuleType("mxnet")
    mx.metric = types.SimpleNamespace(EvalMetric=_EvalMetric)
    mx.ndarray = types.SimpleNamespace(argmax_channel=_argmax_channel)
    had = sys.modules.get("mxnet")
    sys.modules["mxnet"] = mx
    try:
        spec = importlib.util.spec_from_file_location("_ref_detection_metric",
                                                      os.path.join(REF, "core", "detection_metric.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        if had is None:
            del sys.modules["mxnet"]
        else:
            sys.modules["mxnet"] = had
    return mod.AccWithIgnore, mod.L1


def _probs(rs, shape):
    x = rs.standard_normal(shape)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(F)


def cases():
    rs = np.random.RandomState(423)
    out = {}
    # the RPN form: pred (N, 2, rows), label (N, rows) with ignored rows; ties at rows 0 and 1 of image 0
    pred = _probs(rs, (2, 2, 12))
    pred[0, :, 0] = 0.5
    pred[0, :, 1] = 0.5
    label = rs.choice([-1.0, 0.0, 1.0], size=(2, 12), p=[0.4, 0.3, 0.3]).astype(F)
    label[0, 0], label[0, 1] = 0, 1                  # the tie counts for class 0: one hit, one miss
    out["rpn"] = (pred, label, rs.uniform(size=(2, 8, 6)).astype(F))
    out["rpn_all_ignored"] = (_probs(rs, (1, 2, 9)), np.full((1, 9), -1, F), np.zeros((1, 4, 9), F))
    # a label outside the classes is valid, never correct, and foreground
    label = rs.choice([0.0, 1.0, 2.0, 7.0], size=(1, 10)).astype(F)
    out["rpn_label_outside"] = (_probs(rs, (1, 2, 10)), label, rs.uniform(size=(1, 4, 10)).astype(F))
    # the R-CNN form: pred (R, K), label (R,); a three-way tie in row 2
    pred = _probs(rs, (6, 5))
    pred[2] = [0.1, 0.3, 0.3, 0.3, 0.0]
    label = np.array([0, 3, 1, 2, 0, 4], F)
    out["rcnn"] = (pred, label, rs.uniform(size=(6, 20)).astype(F) * (label[:, None] > 0))
    # the image-batched label the head hands the metric (bbox_label_blockgrad is (batch_image, -1))
    pred = _probs(rs, (8, 3))
    out["rcnn_batched_label"] = (pred, rs.randint(0, 3, size=(2, 4)).astype(F), rs.uniform(size=(8, 4)).astype(F))
    return out


def main():
    Acc, L1 = reference_metrics()
    store = {}
    for name, (pred, label, reg) in cases().items():
        acc = Acc("acc", ["cls_loss_output"], ["label"])
        acc.update([_ND(label)], [_ND(pred)])
        l1 = L1("l1", ["reg_loss_output"], ["label"])
        l1.update([_ND(label)], [_ND(reg)])
        store[name + "/pred"], store[name + "/label"], store[name + "/reg_loss"] = pred, label, reg
        store[name + "/acc_sum"] = np.asarray(acc.sum_metric, np.float64)
        store[name + "/acc_num"] = np.asarray(acc.num_inst, np.int64)
        store[name + "/l1_sum"] = np.asarray(l1.sum_metric, np.float64)
        store[name + "/l1_num"] = np.asarray(l1.num_inst, np.int64)
        print(name, float(acc.sum_metric), int(acc.num_inst), float(l1.sum_metric), int(l1.num_inst))
    np.savez_compressed(os.path.join(HERE, "rcnn_loss_metrics.npz"), **store)


if __name__ == "__main__":
    main()
