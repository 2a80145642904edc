"""Cross-checks against THE REFERENCE'S OWN C++, through oracle/mxshim (not a pin).

oracle/build_ref_cxx.py compiles the reference's operator sources (operator_cxx/**/*.cc and, through
a host emulation of the CUDA launch model, *.cu) unmodified and where they lie, against the MXNet /
CUDA stand-ins of oracle/mxshim -- our own code, so a misreading shared by the shim and the oracle
would pass here.  The pins that no code of ours sits under are in tests/test_py_twin_pins.py
(ProposalTarget and DecodeBBox against the reference's float64 Python twins); RoIAlign has no
runnable reference-side twin.  The fixtures
tests/golden/ref_cxx_{digests.json,arrays.npz} were produced by running the seeded cases of
tests/refcases.py through those libraries (tests/golden/make_golden_cxx.py).

  CPU  (-m "not gpu"): the C oracle reproduces every fixture (bit-exactly except Proposal_v3's
       expf, see refcases.py); where oracle/_ref exists the fixtures are re-derived live and the
       operator interfaces (argument / output names, visible outputs, inferred shapes) are read
       from the reference's own registration code.
  GPU  (-m gpu): the HIP kernels, called through the C ABI, reproduce the same fixtures:
       bit-exact for RoIAlign/RoIPool forward, anchors, ProposalTarget (incl. RNG replay), NMS,
       DecodeBBox; <= 1e-4 elementwise for the scatter backwards; <= 1 ulp for Proposal_v3 boxes.
"""
import json
import os

import numpy as np
import pytest

from . import refcases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLD, "ref_cxx_digests.json")) as _f:
    DIGESTS = json.load(_f)
ARRAYS = np.load(os.path.join(GOLD, "ref_cxx_arrays.npz"))
NAMES = sorted(refcases.CASES)


def _have_ref():
    from oracle import refmx
    return all(refmx.available(l) for l in ("roi_align_v2", "roi_pooling_v1", "proposal_target", "proposal_target_v2", "proposal_mask_target",
                                            "generate_anchor", "nms", "proposal_v3", "decodebbox"))


def _check(name, res, exact, hip=False):
    case = refcases.CASES[name]
    assert set(res) == set(DIGESTS[name]), (set(res), set(DIGESTS[name]))
    for k, v in res.items():
        meta = DIGESTS[name][k]
        assert list(v.shape) == meta["shape"] and str(v.dtype) == meta["dtype"], (name, k, v.shape)
        if hip and k in case["hip_close"]:
            want = ARRAYS["%s/%s" % (name, k)]
            err = np.abs(v.astype(np.float64) - want) / np.maximum(1.0, np.abs(want))
            assert err.max() <= case["hip_close"][k], "%s/%s: rel err %g" % (name, k, err.max())
            assert np.array_equal(v != 0, want != 0), "%s/%s: different rows / class slots" % (name, k)
        elif exact:
            assert refcases.digest(v) == meta["sha256"], \
                "%s/%s differs from what the reference's compiled operator produced" % (name, k)
        else:
            tol = case["kind"][1]
            want = ARRAYS["%s/%s" % (name, k)]
            err = np.abs(v.astype(np.float64) - want)
            assert err.max() <= tol, "%s/%s: max |err| %g > %g (elementwise)" % (name, k, err.max(), tol)


def test_every_case_has_a_fixture():
    assert set(DIGESTS) == set(NAMES)
    for name in NAMES:
        for k in DIGESTS[name]:
            if refcases.CASES[name]["kind"] != "exact" or k in refcases.CASES[name]["hip_close"]:
                assert "%s/%s" % (name, k) in ARRAYS.files


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_reference(name):
    """oracle/liboracle.so == the reference's compiled operator on the same seeded inputs."""
    case = refcases.CASES[name]
    res = refcases.run_case(name, "oracle")
    _check(name, res, exact=case["oracle_exact"])


def test_proposal_v3_expf_difference_is_one_ulp_and_rare():
    """The only non-bit-exact pin: CUDA's exp(float) is glibc expf in the emulation while the oracle
    (and the HIP kernel) use the correctly rounded value; scores, order and kept set are identical
    and < 0.5 % of the coordinates move by one ulp."""
    for name in [n for n in NAMES if n.startswith("proposal_v3_") and not n.endswith("_iou_loss")]:
        res = refcases.run_case(name, "oracle")
        want_b, want_s = ARRAYS[name + "/output"], ARRAYS[name + "/score"]
        np.testing.assert_array_equal(res["score"], want_s)
        d = res["output"] != want_b
        assert d.mean() < 5e-3
        ulp = np.spacing(np.maximum(np.abs(want_b), np.float32(1)))
        assert np.all(np.abs(res["output"] - want_b) <= ulp)


FAST_LIVE = [n for n in NAMES if not n.startswith(("fpn_roi_align_c256", "nms_2", "proposal_v3_4",
                                                    "proposal_v3_2"))]


@pytest.mark.skipif(not _have_ref(), reason="oracle/_ref/libref_*.so not built (needs /root/reference)")
@pytest.mark.parametrize("name", FAST_LIVE)
def test_fixture_is_what_the_reference_produces_now(name):
    res = refcases.run_case(name, "ref")
    for k, v in res.items():
        assert refcases.digest(v) == DIGESTS[name][k]["sha256"], (name, k)


@pytest.mark.skipif(not _have_ref(), reason="oracle/_ref/libref_*.so not built (needs /root/reference)")
def test_reference_cpu_backward_diverges_from_its_gpu_backward():
    """SURVEY A.2 shown on the reference's OWN two backward kernels: roi_align_v2.cc:35-106 (gather)
    drops duplicate-corner terms that roi_align_v2.cu:35-84 (scatter, the spec) keeps."""
    from oracle import pyoracle as orc
    from oracle import refmx
    op = refmx.RefOp("roi_align_v2", "_contrib_ROIAlign_v2", pooled_size=(7, 7), spatial_scale=1 / 16.0)
    rs = np.random.RandomState(0)
    data = rs.standard_normal((1, 1, 40, 40)).astype(np.float32)
    rois = np.array([[[16.0, 16.0, 16.0 + 21 * 16, 16.0 + 21 * 16]]], np.float32)  # integer samples
    out, ax, ay = op.forward([data, rois])
    dy = np.ones_like(out)
    g = op.backward([dy], [data, rois], [out, ax, ay], ctx="gpu")[0]
    c = op.backward([dy], [data, rois], [out, ax, ay], ctx="cpu")[0]
    assert abs(g.sum() - 49.0) < 1e-3 and c.sum() < 0.6 * g.sum()
    np.testing.assert_array_equal(g, orc.roi_align_v2_bwd(dy, ax, ay, data.shape))
    np.testing.assert_array_equal(c, orc.roi_align_v2_bwd_cpu_gather(dy, rois, ax, ay, data.shape, 1 / 16.0))
    # kAddTo on the reference op accumulates; kWriteInplace is refused (roi_align_v2.cu:105-108)
    acc = g.copy()
    op.backward([dy], [data, rois], [out, ax, ay], ctx="gpu", req=["add", "null"],
                in_grads=[acc, np.zeros_like(rois)])
    np.testing.assert_allclose(acc, 2 * g, rtol=1e-6)
    with pytest.raises(refmx.RefError):
        op.backward([dy], [data, rois], [out, ax, ay], ctx="gpu", req=["inplace", "write"])


@pytest.mark.skipif(not _have_ref(), reason="oracle/_ref/libref_*.so not built (needs /root/reference)")
def test_reference_roi_pool_docstring_vector():
    """roi_pooling_v1.cc:265-285 through the reference's own CPU and (emulated) GPU operators."""
    from oracle import refmx
    x = np.arange(48, dtype=np.float32).reshape(1, 1, 8, 6)
    y = np.array([[0, 0, 0, 4, 4]], np.float32)
    for ctx in ("cpu", "gpu"):
        a = refmx.RefOp("roi_pooling_v1", "ROIPooling_v1", pooled_size=(2, 2), spatial_scale=1.0
                        ).forward([x, y], ctx=ctx)[0]
        b = refmx.RefOp("roi_pooling_v1", "ROIPooling_v1", pooled_size=(2, 2), spatial_scale=0.7
                        ).forward([x, y], ctx=ctx)[0]
        assert a.ravel().tolist() == [14, 16, 26, 28] and b.ravel().tolist() == [7, 9, 19, 21]


# ------------------------------------------------------------------------------------------ GPU --
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_hip_reproduces_reference(ops, name):
    case = refcases.CASES[name]
    res = refcases.run_case(name, "hip")
    _check(name, res, exact=(case["kind"] == "exact"), hip=True)


# ------------------------------------------------------------- operator interface (drop-in) ----
IFACE = [
    ("roi_align_v2", "_contrib_ROIAlign_v2", dict(pooled_size=(7, 7), spatial_scale=0.25),
     [(2, 256, 200, 334), (2, 512, 4)]),
    ("roi_pooling_v1", "ROIPooling_v1", dict(pooled_size=(7, 7), spatial_scale=0.0625),
     [(2, 1024, 50, 84), (1024, 5)]),
    ("proposal_target", "ProposalTarget",
     dict(num_classes=81, batch_images=2, image_rois=512, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5,
          bg_thresh_lo=0.0, proposal_without_gt=False), [(2, 2000, 4), (2, 100, 5)]),
    ("proposal_target", "ProposalTarget",
     dict(num_classes=81, batch_images=2, image_rois=512, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5,
          bg_thresh_lo=0.0, proposal_without_gt=False, output_iou=True), [(2, 2000, 4), (2, 100, 5)]),
    ("proposal_target_v2", "ProposalTarget_v2",
     dict(num_classes=81, batch_images=2, image_rois=128, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5,
          bg_thresh_lo=0.0, proposal_without_gt=False, filter_scales=True), [(2, 2000, 4), (2, 100, 5), (2, 2)]),
    ("proposal_mask_target", "ProposalMaskTarget",
     dict(num_args=3, num_classes=81, batch_images=2, image_rois=512, mask_size=28, fg_fraction=0.25,
          fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, proposal_without_gt=False, output_iou=True),
     [(2, 2000, 4), (2, 100, 5), (2, 100, 2500)]),
    ("generate_anchor", "_contrib_GenAnchor", dict(scales=(8,), ratios=(0.5, 1, 2), feature_stride=4),
     [(2, 6, 200, 334)]),
    ("nms", "_contrib_NMS", dict(rpn_pre_nms_top_n=-1, rpn_post_nms_top_n=1000, threshold=0.7),
     [(2, 2000, 5)]),
    ("nms", "_contrib_NMS", dict(rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, threshold=0.7, output_score=True),
     [(2, 200, 5)]),
    ("proposal_v3", "_contrib_Proposal_v3",
     dict(rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=2000, threshold=0.7, rpn_min_size=0, scales=(8,),
          ratios=(0.5, 1, 2), feature_stride=64, output_score=True), [(2, 6, 13, 21), (2, 12, 13, 21), (2, 3)]),
    ("decodebbox", "_contrib_DecodeBBox", dict(class_agnostic=True), [(2, 300, 4), (2, 300, 8), (2, 3)]),
    ("decodebbox", "_contrib_DecodeBBox", dict(class_agnostic=False, bbox_decode_type="xyxy"),
     [(2, 300, 4), (2, 300, 324), (2, 3)]),
]


@pytest.mark.skipif(not _have_ref(), reason="oracle/_ref/libref_*.so not built (needs /root/reference)")
@pytest.mark.parametrize("lib,name,kw,in_shapes", IFACE, ids=[c[1] + str(i) for i, c in enumerate(IFACE)])
def test_adapter_interface_equals_reference_registration(lib, name, kw, in_shapes):
    """The CustomOp adapter (simpledet_amd/mxnet_plugin.py) and the reference's own registration
    code (NNVM_REGISTER_OP / OperatorProperty, executed from the reference sources) agree on
    argument names, output names, visible-output count, inferred output shapes and on which
    arrays the backward pass keeps alive."""
    from oracle import refmx
    from simpledet_amd import mxnet_plugin
    from . import mx_stub
    ref = refmx.RefOp(lib, name, **kw)
    mx = mx_stub.make_stub()
    props = mxnet_plugin._build_ops(mx)
    prop_cls = props[name][0]
    ours = prop_cls(**{k: refmx._pystr(v) for k, v in kw.items()})  # MXNet hands every kwarg over as str
    assert ours.list_arguments() == ref.list_arguments()
    assert ours.list_outputs() == ref.list_outputs()
    assert getattr(ours, "num_visible_outputs", len(ours.list_outputs())) == ref.num_visible_outputs()
    got = ours.infer_shape([list(s) for s in in_shapes])
    assert [tuple(s) for s in got[1]] == ref.infer_shape(in_shapes)
    nin, nout = len(in_shapes), len(ours.list_outputs())
    og, idt, od = list(range(nout)), list(range(nout, nout + nin)), list(range(nout + nin, 2 * nout + nin))
    mine = sorted(ours.declare_backward_dependency(og, idt, od))
    if ref.legacy:
        theirs = sorted(ref.backward_dependency(nin))
    else:
        _, codes = ref.gradient_inputs(nin)
        theirs = sorted(og[c] if c < 100 else idt[c - 100] if c < 200 else od[c - 200] for c in codes)
    assert mine == theirs


@pytest.mark.skipif(not _have_ref(), reason="oracle/_ref/libref_*.so not built (needs /root/reference)")
def test_reference_parameter_checks():
    """dmlc parameter errors of the reference registration, for the adapter's error behaviour."""
    from oracle import refmx
    with pytest.raises(refmx.RefError, match="Required parameter"):
        refmx.RefOp("roi_align_v2", "_contrib_ROIAlign_v2", pooled_size=(7, 7))
    with pytest.raises(refmx.RefError, match="Cannot find argument"):
        refmx.RefOp("roi_align_v2", "_contrib_ROIAlign_v2", pooled_size=(7, 7), spatial_scale=0.25, foo=1)
    with pytest.raises(refmx.RefError, match="exceeds bound"):
        refmx.RefOp("roi_align_v2", "_contrib_ROIAlign_v2", pooled_size=(7, 7), spatial_scale=4.0)
    op = refmx.RefOp("roi_align_v2", "_contrib_ROIAlign_v2", pooled_size=(7, 7), spatial_scale=0.25)
    with pytest.raises(refmx.RefError, match="3D tensor"):
        op.infer_shape([(2, 8, 50, 84), (64, 5)])
    op = refmx.RefOp("proposal_target", "ProposalTarget", num_classes=81, batch_images=2, image_rois=64,
                     fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0.0, proposal_without_gt=False)
    rois, gt = refcases.synth.proposal_target_inputs(0, 2, 100, 10)
    with pytest.raises(refmx.RefError, match="kWriteTo"):
        op.forward([rois, gt], req=["add"] * 5)
