"""The meaning of the loss heads' state block {valid, correct, fg, reg_sum}, pinned to the reference's own metric
classes: tests/golden/rcnn_loss_metrics.npz holds what AccWithIgnore and L1 (core/detection_metric.py:40-66,134-156)
computed on recorded arrays (tests/golden/make_golden_rcnn_loss.py ran them).  The restatement's four numbers must
equal them; tests/test_rcnn_loss.py pins the device to the restatement."""
import os

import numpy as np
import pytest

from tests import rcnn_loss_ref as rl

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rcnn_loss_metrics.npz")
CASES = ("rpn", "rpn_all_ignored", "rpn_label_outside", "rcnn", "rcnn_batched_label")


def _fixture():
    return np.load(GOLDEN)


def test_the_fixture_holds_every_case_with_ties_and_ignored_rows():
    fx = _fixture()
    assert sorted({k.split("/")[0] for k in fx.files}) == sorted(CASES)
    pred, label = fx["rpn/pred"], fx["rpn/label"]
    assert pred[0, 0, 0] == pred[0, 1, 0] and pred[0, 0, 1] == pred[0, 1, 1]      # two tied rows ...
    assert label[0, 0] == 0 and label[0, 1] == 1                                  # ... one for each class
    assert (label == -1).any() and (label != -1).any()
    assert (fx["rpn_all_ignored/label"] == -1).all() and int(fx["rpn_all_ignored/acc_num"]) == 0
    assert (fx["rpn_label_outside/label"] >= 2).any()
    assert np.sum(fx["rcnn/pred"][2] == fx["rcnn/pred"][2].max()) == 3


@pytest.mark.parametrize("name", CASES)
def test_the_restatement_computes_what_the_reference_metrics_compute(name):
    fx = _fixture()
    pred, label, reg = fx[name + "/pred"], fx[name + "/label"], fx[name + "/reg_loss"]
    correct, valid, reg_sum, fg = rl.metrics(pred, label, reg, ignore=-1)
    assert correct == int(fx[name + "/acc_sum"]) and valid == int(fx[name + "/acc_num"])
    assert fg == int(fx[name + "/l1_num"])
    assert float(reg_sum) == float(fx[name + "/l1_sum"])
    if not (label == -1).any():
        # normalization='batch' drops no row: the same numbers as long as no label is -1
        assert rl.metrics(pred, label, reg, ignore=None) == (correct, valid, reg_sum, fg)
        assert valid == label.size


def test_a_tie_goes_to_the_lower_class_and_the_arg_max_is_over_the_probabilities():
    fx = _fixture()
    # rows 0 and 1 of the RPN case tie: class 0 wins, so label 0 is a hit and label 1 a miss
    pred, label = fx["rpn/pred"][:1, :, :2], fx["rpn/label"][:1, :2]
    assert rl.metrics(pred, label, None)[:2] == (1, 2)
    # logits one ulp apart whose float32 probabilities tie: the logits prefer class 1, the metric says class 0
    x = np.array([[rl.TIE_LO, rl.TIE_HI]], rl.F)
    p = rl.softmax_rows_f32(x)
    assert x[0, 1] > x[0, 0] and p[0, 0] == p[0, 1] == 0.5
    assert rl.metrics(p, np.array([1.0], rl.F), None)[0] == 0
    assert rl.metrics(p, np.array([0.0], rl.F), None)[0] == 1


def test_softmax_needs_the_maximum_subtracted():
    x = np.array([[1e4, -1e4], [-1e4, 1e4]], rl.F)
    p = rl.softmax_rows_f32(x)
    assert np.array_equal(p, np.array([[1, 0], [0, 1]], rl.F))
    with np.errstate(over="ignore", invalid="ignore"):
        naive = np.exp(x) / np.exp(x).sum(axis=1, keepdims=True)
    assert not np.isfinite(naive).all()
