"""The RetinaNet configs of the reference with `install(mx, retina=True)`: every test symbol's five
GenProposalRetina nodes (models/retinanet/builder.py:358-389, one per level P3-P7) arrive as
`sd__contrib_GenProposalRetina` Custom nodes with the reference's keyword arguments, fed by the
`sd__contrib_GenAnchor` nodes; parameter sets the kernels do not take fall back to the native
constructor and are recorded.  Also the prop's shape inference (generate_proposal_retina-inl.h:106-140).

The sweep is CPU only and skipped where /root/reference is absent (the GPU box), like
tests/test_reference_config_sweep.py."""
import collections
import importlib
import os

import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")

# the 17 configs whose test symbol holds GenProposalRetina (5 nodes each)
RETINA_CONFIGS = [
    "config.NASFPN.retina_r50v1b_fpn_640_1@256_25epoch",
    "config.NASFPN.retina_r50v1b_nasfpn_1024_7@256_25epoch",
    "config.NASFPN.retina_r50v1b_nasfpn_1280_7@384_25epoch",
    "config.NASFPN.retina_r50v1b_nasfpn_640_7@256_25epoch",
    "config.NASFPN.retina_r50v1b_tdbu_640_3@384_25epoch",
    "config.kd.retina_r50v1b_fpn_1x_fitnet_g10",
    "config.kd.retina_r50v1b_fpn_2x_fitnet_g10",
    "config.resnet_v1b.retina_r101v1b_fpn_1x",
    "config.resnet_v1b.retina_r152v1b_fpn_1x",
    "config.resnet_v1b.retina_r50v1b_fpn_1x",
    "config.retina_r101v1_fpn_1x",
    "config.retina_r50v1_fpn_1x",
    "config.sepc.retina_r50v1b_fpn_1x",
    "config.sepc.retina_r50v1b_fpn_pconv_1x",
    "config.sepc.retina_r50v1b_fpn_pconv_ibn_1x",
    "config.sepc.retina_r50v1b_fpn_sepc_1x",
    "config.sepc.retina_r50v1b_fpn_sepclite_1x",
]


def _test_nodes(mod):
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin
        cfg = importlib.import_module(mod)
        mxnet_plugin._state.update(registered=False)
        props = mxnet_plugin.install(R.mx, retina=True)
        assert "_contrib_GenProposalRetina" in props
        assert "GenProposalRetina" in R.mx.sym.contrib.__all__  # builder.py:358 keeps the op branch
        nodes = {}
        for s in (getattr(o, "test_symbol", None) for o in cfg.get_config(False)):
            if isinstance(s, RS.Symbol):
                RS.walk(s, nodes)
        return list(nodes.values()), list(mxnet_plugin._state["fallbacks"])


@needs_ref
@pytest.mark.parametrize("mod", RETINA_CONFIGS)
def test_retina_configs_take_the_device_op(mod):
    nodes, fallbacks = _test_nodes(mod)
    assert not fallbacks, fallbacks
    ops = collections.Counter(n.op_type for n in nodes)
    assert ops["sd__contrib_GenProposalRetina"] == 5, dict(ops)
    assert ops["GenProposalRetina"] == 0
    gp = [n for n in nodes if n.op_type == "sd__contrib_GenProposalRetina"]
    strides = sorted(int(n.params["feature_stride"]) for n in gp)
    assert strides == [8, 16, 32, 64, 128]
    for n in gp:
        p = n.params
        assert float(p["thresh"]) == (0.0 if int(p["feature_stride"]) == 128 else 0.05)
        assert p["rpn_pre_nms_top_n"] == "1000" and p["num_anchors"] == "9" and p["rpn_min_size"] == "0"
        assert len(n.inputs) == 4
        anchors = RS.source(n.inputs[3])
        assert anchors.op_type == "sd__contrib_GenAnchor"
        assert anchors.params["feature_stride"] == p["feature_stride"]


@needs_ref
def test_iou_loss_falls_back_to_the_native_op():
    with RS.reference_modules() as R:
        mx = R.mx
        from simpledet_amd import mxnet_plugin
        mxnet_plugin._state.update(registered=False)
        mxnet_plugin.install(mx, retina=True)
        c, b, i, a = (mx.sym.var(v) for v in ("cls", "bbox", "info", "anc"))
        ok = mx.sym.contrib.GenProposalRetina(cls_prob=c, bbox_pred=b, im_info=i, anchors=a, num_anchors=9,
                                              rpn_pre_nms_top_n=1000, thresh=0.05, name="ok")
        assert RS.source(ok[0]).op_type == "sd__contrib_GenProposalRetina"
        assert not mxnet_plugin._state["fallbacks"]
        nat = mx.sym.contrib.GenProposalRetina(cls_prob=c, bbox_pred=b, im_info=i, anchors=a, num_anchors=9,
                                               rpn_pre_nms_top_n=1000, thresh=0.05, iou_loss=True, name="iou")
        assert RS.source(nat[0]).op_type == "GenProposalRetina"
        (name, name_kw, why), = mxnet_plugin._state["fallbacks"]
        assert name == "_contrib_GenProposalRetina" and name_kw == "iou" and "iou_loss" in why


@pytest.fixture()
def retina_plugin():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, retina=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_leaves_the_native_op(retina_plugin):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    assert "_contrib_GenProposalRetina" not in mxnet_plugin.install(mx)
    assert "sd__contrib_GenProposalRetina" not in mx.registry


def test_prop_registration_and_shape_inference(retina_plugin):
    mx, props, _ = retina_plugin
    assert "sd__contrib_GenProposalRetina" in mx.registry
    P = props["_contrib_GenProposalRetina"]
    p = P(num_anchors="9", rpn_pre_nms_top_n="1000", rpn_min_size="0", thresh="0.05", feature_stride="8",
          anchor_mean="(0, 0, 0, 0)", anchor_std="(1, 1, 1, 1)", workspace="512")
    assert p.list_arguments() == ["cls_prob", "bbox_pred", "im_info", "anchors"]
    assert p.list_outputs() == ["output", "scores"]
    ins, outs = p.infer_shape([(2, 720, 100, 167), (), (), ()])
    assert ins == [(2, 720, 100, 167), (2, 36, 100, 167), (2, 3), (100 * 167 * 9, 4)]
    assert outs == [(2, 1000, 4), (2, 1000, 81)]
    p1 = P(num_anchors="9", rpn_pre_nms_top_n="300", output_one_hot="False", batch_wise_anchor="False")
    ins, outs = p1.infer_shape([(1, 9, 7, 11), (), (), ()])
    assert outs == [(1, 300, 4), (1, 300, 1)] and ins[3] == (7 * 11 * 9, 4)
    assert p.declare_backward_dependency(["g0", "g1"], ["a", "b", "c", "d"], ["o", "s"]) == []
    assert "iou_loss" in P.sd_supports({"num_anchors": "9", "iou_loss": "True"})
    assert "batch_wise_anchor" in P.sd_supports({"num_anchors": "9", "batch_wise_anchor": "True"})
    assert P.sd_supports({"num_anchors": "9", "rpn_pre_nms_top_n": "20000"})
    assert P.sd_supports({"num_anchors": "9", "no_such": "1"})
    assert P.sd_supports({"num_anchors": "9", "rpn_pre_nms_top_n": "1000", "thresh": "0"}) == ""
