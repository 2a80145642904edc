"""`install(mx, retina_loss=True)`: RetinaNet's and RepPoints' train graphs hold `sd__contrib_FocalLoss` /
`sd__contrib_BBoxNorm` Custom nodes with the reference's keyword arguments (models/retinanet/builder.py:294-332
for both the sync_loss and the default branch, models/RepPoints/builder.py:404,439,472); without the flag
the graph is what it was.  Also the props' argument names, outputs, shape inference and backward dependencies
(focal_loss-inl.h:258-324, bbox_norm-inl.h:160-217).

The builder tests are CPU only and skipped where the reference tree is absent, like
tests/test_retina_plugin_sweep.py."""
import collections
import importlib
import os

import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")


def _train_ops(mod, **flags):
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin
        cfg = importlib.import_module(mod)
        mxnet_plugin._state.update(registered=False)
        props = mxnet_plugin.install(R.mx, **flags)
        nodes = {}
        for o in cfg.get_config(True):
            s = getattr(o, "train_symbol", None)
            if isinstance(s, RS.Symbol):
                RS.walk(s, nodes)
        probe = dict(mxnet_plugin._state["mxnext_probe"])
        mxnet_plugin._state.update(registered=False)
        return list(nodes.values()), props, probe


@needs_ref
def test_retinanet_default_branch_takes_the_device_ops():
    nodes, props, probe = _train_ops("config.retina_r50v1_fpn_1x", retina_loss=True)
    assert "_contrib_FocalLoss" in props and "_contrib_BBoxNorm" in props
    assert "focal_loss" in probe and "bbox_norm" in probe
    ops = collections.Counter(n.op_type for n in nodes)
    assert ops["sd__contrib_FocalLoss"] == 1 and ops["sd__contrib_BBoxNorm"] == 1, dict(ops)
    assert ops["X.focal_loss"] == 0 and ops["X.bbox_norm"] == 0 and ops["FocalLoss"] == 0 and ops["BBoxNorm"] == 0
    fl, = [n for n in nodes if n.op_type == "sd__contrib_FocalLoss"]
    # builder.py:307-316, config/retina_r50v1_fpn_1x.py:76-78: the parameters as the reference passes them
    assert fl.params["normalization"] == "valid" and fl.name == "cls_loss"
    assert float(fl.params["alpha"]) == 0.25 and float(fl.params["gamma"]) == 2.0
    assert fl.params["workspace"] == "1500" and float(fl.params["grad_scale"]) > 0
    assert "out_grad" not in fl.params and len(fl.inputs) == 2
    bn, = [n for n in nodes if n.op_type == "sd__contrib_BBoxNorm"]
    assert bn.name == "bbox_norm" and len(bn.inputs) == 2 and not bn.params
    assert RS.source(bn.inputs[1]) is RS.source(fl.inputs[1])       # both read cls_label


@needs_ref
def test_retinanet_sync_loss_branch_takes_the_device_op():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin
        cfg = importlib.import_module("config.retina_r50v1_fpn_1x")
        builder = importlib.import_module("models.retinanet.builder")
        mxnet_plugin._state.update(registered=False)
        mxnet_plugin.install(R.mx, retina_loss=True)
        out = cfg.get_config(True)
        head_param = [o for o in out if hasattr(o, "focal_loss") and hasattr(o, "anchor_generate")]
        assert head_param, "RpnParam of the config not found"
        p = head_param[0]
        p.sync_loss = True
        head = builder.RetinaNetHead(p)
        v = R.mx.sym.var
        feat = {"stride%s" % s: v("f%s" % s) for s in p.anchor_generate.stride}
        cls_loss, reg_loss = head.get_loss(feat, v("cls_label"), v("bbox_target"), v("bbox_weight"))
        nodes = RS.walk(R.mx.sym.Group([cls_loss, reg_loss])).values()
        ops = collections.Counter(n.op_type for n in nodes)
        # builder.py:295-305, :325-326: focal loss with out_grad, divided by the synchronised fg count; no BBoxNorm
        assert ops["sd__contrib_FocalLoss"] == 1 and ops["sd__contrib_BBoxNorm"] == 0, dict(ops)
        fl, = [n for n in nodes if n.op_type == "sd__contrib_FocalLoss"]
        assert fl.params["out_grad"] == "True" and fl.params["workspace"] == "1800"
        assert "normalization" not in fl.params and float(fl.params["alpha"]) == 0.25
        mxnet_plugin._state.update(registered=False)


@needs_ref
def test_without_the_flag_the_graph_is_unchanged():
    nodes, props, probe = _train_ops("config.retina_r50v1_fpn_1x")
    assert "_contrib_FocalLoss" not in props and "_contrib_BBoxNorm" not in props
    assert "focal_loss" not in probe and "bbox_norm" not in probe
    ops = collections.Counter(n.op_type for n in nodes)
    assert ops["sd__contrib_FocalLoss"] == 0 and ops["sd__contrib_BBoxNorm"] == 0
    assert ops["X.focal_loss"] == 1 and ops["X.bbox_norm"] == 1     # the stand-in's own wrapper nodes
    # ... also after an opt-in install() in the same process
    _train_ops("config.retina_r50v1_fpn_1x", retina_loss=True)
    nodes, _, _ = _train_ops("config.retina_r50v1_fpn_1x")
    ops = collections.Counter(n.op_type for n in nodes)
    assert ops["sd__contrib_FocalLoss"] == 0 and ops["X.focal_loss"] == 1 and ops["X.bbox_norm"] == 1


@needs_ref
def test_reppoints_three_call_sites_bind():
    nodes, _, _ = _train_ops("config.RepPoints.reppoints_moment_r50v1_fpn_1x", retina_loss=True)
    ops = collections.Counter(n.op_type for n in nodes)
    assert ops["sd__contrib_FocalLoss"] == 1 and ops["sd__contrib_BBoxNorm"] == 2, dict(ops)
    fl, = [n for n in nodes if n.op_type == "sd__contrib_FocalLoss"]
    assert fl.params["normalization"] == "valid" and len(fl.inputs) == 2


@pytest.fixture()
def loss_plugin():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, retina_loss=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_neither(loss_plugin):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx)
    assert "_contrib_FocalLoss" not in props and "_contrib_BBoxNorm" not in props
    assert "sd__contrib_FocalLoss" not in mx.registry and "sd__contrib_BBoxNorm" not in mx.registry


def test_props_mirror_the_reference_operators(loss_plugin):
    mx, props, mxnet_plugin = loss_plugin
    assert "sd__contrib_FocalLoss" in mx.registry and "sd__contrib_BBoxNorm" in mx.registry
    F, N = props["_contrib_FocalLoss"], props["_contrib_BBoxNorm"]
    f = F(alpha="0.25", gamma="2.0", normalization="valid", grad_scale="1.0", workspace="1500")
    assert f.list_arguments() == ["data", "label"] and f.list_outputs() == ["output"]
    assert f.infer_shape([(2, 200700, 80), ()]) == ([(2, 200700, 80), (2, 200700)], [(2, 200700, 80)])
    # focal_loss-inl.h:314-324: label and out; the head gradient only with out_grad
    assert f.declare_backward_dependency(["g"], ["d", "l"], ["o"]) == ["l", "o"]
    assert f.need_top_grad_ is False
    g = F(alpha="0.25", gamma="2.0", out_grad="True", workspace="1800")
    assert g.declare_backward_dependency(["g"], ["d", "l"], ["o"]) == ["l", "o", "g"]
    assert g.need_top_grad_ is True and g.g["normalization"] == 0          # default 'null' (:70-72)
    d = F()
    assert (d.g["alpha"], d.g["gamma"], d.g["grad_scale"], d.g["out_grad"]) == (0.25, 2.0, 1.0, False)
    with pytest.raises(ValueError, match="normalization"):
        F(normalization="sum")
    n = N()
    assert n.list_arguments() == ["data", "label"] and n.list_outputs() == ["output"]
    assert n.infer_shape([(2, 36, 22300), (2, 200700)]) == ([(2, 36, 22300), (2, 200700)], [(2, 36, 22300)])
    assert n.infer_shape([(2, 36, 22300), ()])[0][1] == (2, 200700)
    assert n.declare_backward_dependency(["g"], ["d", "l"], ["o"]) == ["l", "g"]   # bbox_norm-inl.h:212-217
    assert n.need_top_grad_ is True
    # the aliases build Custom nodes with string parameters
    v = mx.sym.Variable
    s = mx.sym.contrib.FocalLoss(data=v("d"), label=v("l"), alpha=0.25, gamma=2.0, normalization="valid",
                                 grad_scale=1.0, workspace=1500, name="cls_loss")
    _head_op = mxnet_plugin._head_op
    op, attrs = _head_op(mx, s)
    op_type = attrs.get("op_type", op)
    assert op_type == "sd__contrib_FocalLoss", (op, attrs)
    want = dict(alpha="0.25", gamma="2.0", normalization="valid", grad_scale="1.0", workspace="1500")
    assert {k: attrs[k] for k in want} == want
    # positional inputs go through the mxnext wrapper too
    import types
    X = types.SimpleNamespace(focal_loss=lambda **kw: None, bbox_norm=lambda **kw: None)
    done = mxnet_plugin.patch_mxnext(X, mx)
    assert "mxnext.focal_loss" in done, (done, mxnet_plugin._state.get("retina_loss"), mxnet_plugin._state["mxnext_probe"])
    op, attrs = _head_op(mx, X.focal_loss(v("d"), v("l"), alpha=0.5))
    assert attrs.get("op_type", op) == "sd__contrib_FocalLoss" and attrs["alpha"] == "0.5"
