"""The final detections of detection_test.py (:174-178 scale and background, :233-260 do_nms, :290 the cut) pinned
for a device implementation: tests/golden/det_post.npz holds what the reference's own Python computed (written by
tests/golden/make_golden_det_post.py from inputs that tests/det_post_cases.py regenerates here), and
tests/det_post_ref.py restates it in numpy with a defined tie rule.

CPU only: fixture integrity, the restatement equals the fixture on every case (which licenses it for ties and NaNs,
where the reference's unstable sort has no single answer), the float64 fact of set_nms, and the box pairs on which
float32 and float64 disagree.  The device entry points these pins are for are not in the tree."""
import hashlib
import os

import numpy as np
import pytest

from . import det_post_cases as cases
from . import det_post_ref as ref

F = np.float32
D = np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "det_post.npz")
REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
MODES = {"nms": 0, "set_nms": 1}


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_inputs = {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = cases.case(name)
    return _inputs[name]


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fixture_kept(golden, name):
    counts, flat = golden[name + "/kept_counts"], golden[name + "/kept_rows"].astype(np.int64)
    out, at = [], 0
    for b in range(counts.shape[0]):
        out.append([])
        for c in range(counts.shape[1]):
            out[b].append(flat[at:at + counts[b, c]])
            at += counts[b, c]
    assert at == len(flat)
    return out


# ------------------------------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("name", cases.CASES)
def test_fixture_inputs_regenerate(golden, name):
    cls, box, scale, par = inputs(name)
    assert sha256(cls, box, scale) == str(golden[name + "/inputs_sha256"])
    assert list(golden[name + "/param"]) == [par["max_det_per_image"], par["min_det_score"], par["nms_thr"],
                                             MODES[par["nms_type"]], par["set_period"]]
    assert golden[name + "/out_dets"].shape == (cls.shape[0], par["max_det_per_image"], 6)


def test_fixture_covers_what_it_claims(golden):
    """both NMS paths in one batch, 5000 candidates in one problem, padding, an empty image, both nms types"""
    cand = golden["retina/candidates"]
    assert cand.shape == (2, 80) and cand[0].max() > 4096 and 0 < cand[1].max() <= 4096
    assert golden["fcos_dense/candidates"].tolist() == [[5000]]
    assert golden["empty/out_counts"].tolist() == [100, 0] and (golden["empty/out_dets"][1, :, 5] == -1).all()
    assert golden["crowd/out_counts"].tolist() == [300, 300]
    assert (golden["set_pairs/out_dets"][0, 7:, 5] == -1).all() and golden["set_pairs/out_counts"].tolist() == [7]
    for name in ("retina", "fcos_dense", "crowd"):
        assert float(golden[name + "/twin_ms"]) > 0


@pytest.mark.parametrize("name", cases.CASES)
def test_restatement_equals_the_reference_run(golden, name):
    cls, box, scale, par = inputs(name)
    out, counts, kept = ref.det_post(cls, box, scale, **par)
    assert np.array_equal(out, golden[name + "/out_dets"])
    assert np.array_equal(counts, golden[name + "/out_counts"])
    want = fixture_kept(golden, name)
    for b in range(cls.shape[0]):
        for c in range(cls.shape[2] - 1):
            assert np.array_equal(kept[b][c], want[b][c]), (b, c)


def test_the_reference_run_saw_float64_in_set_nms(golden):
    """recorded by the fixture's maker inside the reference's own do_nms: the det that reaches nms()"""
    for name in cases.CASES:
        par = inputs(name)[3]
        assert str(golden[name + "/nms_input_dtype"]) == ("float64" if par["nms_type"] == "set_nms" else "float32")


@needs_ref
def test_do_nms_hands_set_nms_a_float64_array():
    """detection_test.py:247-253, run where it lies: the int64 index column promotes the float32 det"""
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    try:
        from make_golden_det_post import Twin
    finally:
        sys.path.pop(0)
    seen = []
    cls, box, scale, par = inputs("set_pairs")
    Twin().forward(cls, box, scale, par, seen)
    assert seen and all(d == np.float64 for d in seen)
    seen = []
    Twin().forward(cls, box, scale, dict(par, nms_type="nms"), seen)
    assert seen and all(d == np.float32 for d in seen)


def test_float64_pairs_decide_differently_in_float32(golden):
    pairs = cases.f64_pairs()
    assert len(pairs) >= 4
    for k, (a, b, k32, k64) in enumerate(pairs):
        assert a.dtype == F and b.dtype == F and k32 != k64
        assert bool(cases.iou(a, b, F) <= F(0.5)) == k32 and bool(cases.iou(a, b, D) <= 0.5) == k64
        assert abs(float(cases.iou(a, b, D)) - 0.5) < 1e-6
        for a2, b2, _, _ in pairs[k + 1:]:                     # isolated: no overlap with any other pair
            for p in (a, b):
                for q in (a2, b2):
                    assert cases.iou(p, q, D) == 0
    # they are in the set_nms fixture, and a float32 set_nms gives another answer on it
    cls, box, scale, par = inputs("set_pairs")
    out64, _, _ = ref.det_post(cls, box, scale, **par)
    out32, c32, _ = ref.det_post(cls, box, scale, set_dtype=F, **par)
    assert np.array_equal(out64, golden["set_pairs/out_dets"])
    assert int(c32[0]) != int(golden["set_pairs/out_counts"][0])
    assert not np.array_equal(out32, out64)


def test_tie_rules_of_the_restatement():
    dets = np.array([[0, 0, 9, 9, .5], [0, 0, 9, 9, .5], [50, 50, 59, 59, .5], [0, 0, 9, 9, .7]], F)
    assert ref.set_nms(dets, [0, 1, 2, 3], 0.5).tolist() == [3, 2]      # all in different sets: as nms
    assert ref.set_nms(dets, [0, 1, 2, 0], 0.5).tolist() == [3, 2, 0]   # row 0 is of row 3's set and survives it
    assert ref.set_nms(dets, [0, 0, 0, 0], 0.5).tolist() == [3, 2, 1, 0]
    cls = np.zeros((1, 3, 3), F)
    cls[0, 0, 1] = cls[0, 1, 2] = cls[0, 2, 1] = .5
    box = np.array([[0, 0, 9, 9], [20, 0, 29, 9], [40, 0, 49, 9]], F).reshape(1, 3, 4)
    out, counts, _ = ref.det_post(cls, box, None, 2, 0.25, 0.5)
    assert out[0, :, 5].tolist() == [1, 0] and out[0, :, 0].tolist() == [20, 0] and counts.tolist() == [2]
