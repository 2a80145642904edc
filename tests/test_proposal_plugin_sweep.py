"""The TridentNet configs of the reference with `install(mx, proposal=True)`: every Proposal_v2 node
of their symbols (models/tridentnet/builder.py:239-255, the scale-aware train symbol) arrives as an
`sd__contrib_Proposal_v2` Custom node with the reference's keyword arguments; the default install()
leaves the native operator in place.  Also the props' arguments, defaults and shape inference
(proposal_v2-inl.h / proposal-inl.h) and the patch_mxnext probe of `X.proposal` with and without the
opt-in.

The sweep is CPU only and skipped where /root/reference is absent (the GPU box), like
tests/test_retina_plugin_sweep.py."""
import collections
import importlib
import os

import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")

TRIDENT_CONFIGS = [
    "config.tridentnet_r101v1c4_c5_1x", "config.tridentnet_r101v1c4_c5_2x",
    "config.tridentnet_r101v2c4_c5_1x", "config.tridentnet_r101v2c4_c5_2x",
    "config.tridentnet_r101v2c4_c5_addminival_2x", "config.tridentnet_r101v2c4_c5_fastapprox_1x",
    "config.tridentnet_r101v2c4_c5_multiscale_addminival_3x_fp16", "config.tridentnet_r50v1c4_c5_1x",
    "config.tridentnet_r50v1c4_c5_2x", "config.tridentnet_r50v2c4_c5_1x", "config.tridentnet_r50v2c4_c5_2x",
]
# the keywords models/tridentnet/builder.py:239-255 passes (besides the four inputs and name)
KWARGS = {"feature_stride", "scales", "ratios", "rpn_pre_nms_top_n", "rpn_post_nms_top_n", "threshold",
          "rpn_min_size", "iou_loss", "filter_scales", "output_score"}


def _nodes(mod, proposal):
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin
        cfg = importlib.import_module(mod)
        mxnet_plugin._state.update(registered=False)
        props = mxnet_plugin.install(R.mx, proposal=proposal)
        nodes = {}
        for is_train in (True, False):
            for o in cfg.get_config(is_train):
                for a in ("train_symbol", "test_symbol", "rpn_test_symbol"):
                    s = getattr(o, a, None)
                    if isinstance(s, RS.Symbol):
                        RS.walk(s, nodes)
        mxnet_plugin._state.update(registered=False)
        return props, list(nodes.values())


@needs_ref
@pytest.mark.parametrize("mod", TRIDENT_CONFIGS)
def test_trident_configs_take_the_device_op(mod):
    """Every Proposal_v2 node the default graphs hold becomes an sd__contrib_Proposal_v2 node with the
    reference's keywords.  Proposal_v2 sits in the scale-aware TRAIN symbol only
    (models/tridentnet/builder.py:62-86 -> get_sampled_proposal_with_filter); the test symbols and
    a config with scaleaware = False (fastapprox) build their proposals through X.proposal."""
    _, native = _nodes(mod, False)
    props, nodes = _nodes(mod, True)
    assert "_contrib_Proposal_v2" in props and "_contrib_Proposal" in props
    want = collections.Counter(n.op_type for n in native)["Proposal_v2"]
    if "fastapprox" not in mod:
        assert want >= 1
    ops = collections.Counter(n.op_type for n in nodes)
    assert ops["sd__contrib_Proposal_v2"] == want and ops["Proposal_v2"] == 0, dict(ops)
    for n in (n for n in nodes if n.op_type == "sd__contrib_Proposal_v2"):
        p = n.params
        assert set(p) == KWARGS, sorted(p)
        assert p["filter_scales"] == "True" and p["output_score"] == "True" and p["iou_loss"] == "False"
        assert int(p["feature_stride"]) == 16
        assert len(n.inputs) == 4
    # the default install leaves every other node as it was
    assert collections.Counter(n.op_type for n in native if n.op_type != "Proposal_v2") == \
        collections.Counter(n.op_type for n in nodes if n.op_type != "sd__contrib_Proposal_v2")


@pytest.fixture()
def plugin():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, proposal=True)
    yield mx, props
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_neither():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx)
    assert "_contrib_Proposal_v2" not in props and "_contrib_Proposal" not in props
    assert "sd__contrib_Proposal_v2" not in mx.registry and "sd__contrib_Proposal" not in mx.registry
    mxnet_plugin._state.update(registered=False)


def test_props_arguments_defaults_and_shapes(plugin):
    mx, props = plugin
    assert "sd__contrib_Proposal_v2" in mx.registry and "sd__contrib_Proposal" in mx.registry
    P2, P1 = props["_contrib_Proposal_v2"], props["_contrib_Proposal"]
    p = P2()  # proposal_v2-inl.h:141-183
    assert p.g == dict(pre=6000, post=300, thr=0.7, min_size=16, scales=(4.0, 8.0, 16.0, 32.0),
                       ratios=(0.5, 1.0, 2.0), stride=16, iou_loss=False, is_train=False,
                       filter_scales=False, v2=True)
    assert p.num_visible_outputs == 1
    assert p.list_arguments() == ["cls_prob", "bbox_pred", "im_info", "valid_ranges"]
    assert p.list_outputs() == ["output", "score"]
    q = P2(rpn_pre_nms_top_n="12000", rpn_post_nms_top_n="500", scales="(2, 4, 8, 16, 32)",
           rpn_min_size="0", filter_scales="True", output_score="True", workspace="512")
    assert q.g["filter_scales"] and q.num_visible_outputs == 2
    ins, outs = q.infer_shape([(6, 30, 50, 75), (), (), ()])
    assert ins == [(6, 30, 50, 75), (6, 60, 50, 75), (6, 3), (6, 2)]
    assert outs == [(6, 500, 4), (6, 500, 1)]
    with pytest.raises(ValueError):
        q.infer_shape([(6, 24, 50, 75), (), (), ()])  # 12 anchors != 5 x 3
    r = P1(is_train="True", rpn_post_nms_top_n="2000")
    assert r.g["is_train"] and not r.g["v2"]
    assert r.list_arguments() == ["cls_prob", "bbox_pred", "im_info"]
    ins, outs = r.infer_shape([(2, 24, 38, 50), (), ()])
    assert ins == [(2, 24, 38, 50), (2, 48, 38, 50), (2, 3)] and outs == [(2, 2000, 4), (2, 2000, 1)]
    assert r.declare_backward_dependency(["g"], ["a", "b", "c"], ["o", "s"]) == []


def _frozen_proposal(**kw):
    return RS.Symbol("Proposal", [v for v in kw.values() if isinstance(v, RS.Symbol)],
                     {k: v for k, v in kw.items() if not isinstance(v, RS.Symbol)}, kw.get("name"), 2)


@needs_ref
@pytest.mark.parametrize("opt_in", [False, True])
def test_patch_mxnext_rebinds_x_proposal_only_with_the_opt_in(opt_in):
    """X.proposal that builds `_contrib_Proposal`: left alone by the default install (the probe's
    verdict is unchanged), rebound to the `_contrib_Proposal` alias with proposal=True."""
    with RS.reference_modules(late_binding=False) as R:
        mx, X = R.mx, R.X
        from simpledet_amd import mxnet_plugin as plug
        X.proposal = _frozen_proposal
        plug._state.update(registered=False)
        plug.install(mx, proposal=opt_in)
        probe = plug._state["mxnext_probe"]["proposal"]
        if not opt_in:
            assert X.proposal is _frozen_proposal and "left alone" in probe
            assert "mxnext.proposal" not in plug._state["mxnext_patched"]
        else:
            assert "rebound" in probe and "mxnext.proposal" in plug._state["mxnext_patched"]
            assert X.proposal._sd_original is _frozen_proposal
            s = X.proposal(cls_prob=mx.sym.var("c"), bbox_pred=mx.sym.var("b"), im_info=mx.sym.var("i"),
                           feature_stride=16, scales=(8,), ratios=(0.5, 1, 2), rpn_pre_nms_top_n=12,
                           rpn_post_nms_top_n=6, threshold=0.7, rpn_min_size=0, iou_loss=False,
                           output_score=True, name="rpn")
            node = RS.source(s[0] if isinstance(s, (tuple, list)) else s)
            assert node.op_type == "sd__contrib_Proposal"
        plug._state.update(registered=False, proposal=False)
