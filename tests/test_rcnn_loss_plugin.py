"""simpledet_amd/rcnn_loss.py: the four loss CustomOps and patch_builders() / unpatch_builders().  CPU only, on
tests/mx_stub.py and tests/ref_stubs.py (the builder tests are skipped where the reference tree is absent, like
tests/test_crowdhuman_plugin.py); the GPU round trip through the adapter is the last test."""
import importlib
import os
import sys

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
NAMES = ("rpn_cls_loss", "rpn_reg_loss", "bbox_cls_loss", "bbox_reg_loss")


@pytest.fixture()
def plug():
    from simpledet_amd import mxnet_plugin, rcnn_loss
    saved = dict(mxnet_plugin._state)
    yield rcnn_loss, mxnet_plugin
    rcnn_loss._own.update(installed=False, props={})
    mxnet_plugin._state.clear()
    mxnet_plugin._state.update(saved)
    mxnet_plugin._state.update(registered=False)


def test_install_registers_four_ops_and_leaves_the_plugins_tables_alone(plug):
    rcnn_loss, mxnet_plugin = plug
    flags = tuple(mxnet_plugin.FEATURE_FLAGS)
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    before = set(mxnet_plugin.install(mx))
    everything = set(mxnet_plugin._state["all_ops"])
    registry_before = set(mx.registry)
    props = rcnn_loss.install(mx)
    assert sorted(props) == sorted(NAMES)
    assert set(mx.registry) - registry_before == {"sd_" + n for n in NAMES}
    assert mxnet_plugin.FEATURE_FLAGS == flags and tuple(mxnet_plugin._FEATURES) == flags
    mxnet_plugin._state.update(registered=False)
    assert set(mxnet_plugin.install(mx)) == before and set(mxnet_plugin._state["all_ops"]) == everything
    assert not set(NAMES) & everything
    with pytest.raises(TypeError):
        mxnet_plugin.install(mx, rcnn_loss=True)
    rcnn_loss.install(mx, stream=1234, sync=False)
    assert mxnet_plugin._state["stream"] == 1234 and mxnet_plugin._state["sync"] is False


def test_props_arguments_shapes_and_rejections(plug):
    rcnn_loss, _ = plug
    props = rcnn_loss.install(mx_stub.make_stub())
    levels = [(2, 6, 200, 334), (2, 6, 100, 167), (2, 6, 50, 84), (2, 6, 25, 42), (2, 6, 13, 21)]
    HW = sum(h * w for _, _, h, w in levels)
    C = props["rpn_cls_loss"](num_level="5", grad_scale="128.0", ignore_label="-1", normalization="valid",
                              use_ignore="True", multi_output="True")
    assert C.need_top_grad_ is False and C.list_outputs() == ["output"]
    assert C.list_arguments() == ["cls_logit%d" % l for l in range(5)] + ["cls_label"]
    assert C.g["grad_scale"] == 128.0 and C.g["ignore_label"] == -1.0
    ins, outs, _ = C.infer_shape(levels + [()])
    assert ins == levels + [(2, 3 * HW)] and outs == [(2, 2, 3, HW)]
    assert C.declare_backward_dependency(["g"], ["a", "b"], ["o"]) == ["a", "b"]
    with pytest.raises(ValueError):
        C.infer_shape(levels + [(2, 3 * HW + 1)])
    with pytest.raises(ValueError):
        C.infer_shape(levels[:4] + [(2, 5, 13, 21), ()])
    C1 = props["rpn_cls_loss"](num_level="1")
    assert C1.infer_shape([(1, 30, 38, 50), ()])[:2] == ([(1, 30, 38, 50), (1, 15 * 38 * 50)], [(1, 2, 15, 38, 50)])
    for bad in (dict(normalization="batch"), dict(normalization="null"), dict(use_ignore="False"),
                dict(multi_output="False"), dict(smooth_alpha="0.1"), dict(out_grad="True"), dict(num_level="9"),
                dict(ignore_label="-0.5")):
        with pytest.raises(ValueError):
            props["rpn_cls_loss"](**bad)
    R = props["rpn_reg_loss"](num_level="5", grad_scale=repr(128.0 / 512), scalar="3.0")
    assert R.need_top_grad_ is False and R.g["sigma"] == 3.0 and R.g["grad_scale"] == 0.25
    assert R.list_arguments() == ["bbox_delta%d" % l for l in range(5)] + ["reg_target", "reg_weight"]
    dl = [(2, 12) + s[2:] for s in levels]
    ins, outs, _ = R.infer_shape(dl + [(), ()])
    assert ins == dl + [(2, 12, HW)] * 2 and outs == [(2, 12, HW)]
    assert props["rpn_reg_loss"]().infer_shape([(1, 60, 38, 50), (), ()])[1] == [(1, 60, 38, 50)]
    with pytest.raises(ValueError):
        props["rpn_reg_loss"](scalar="0")
    B = props["bbox_cls_loss"](grad_scale="1.0", normalization="batch")
    assert B.need_top_grad_ is False and B.list_arguments() == ["cls_logit", "cls_label"]
    assert B.infer_shape([(1024, 81), ()])[:2] == ([(1024, 81), (1024,)], [(1024, 81)])
    for bad in (dict(normalization="valid"), dict(smooth_alpha="0.5"), dict(out_grad="1")):
        with pytest.raises(ValueError):
            props["bbox_cls_loss"](**bad)
    with pytest.raises(ValueError):
        B.infer_shape([(1024, 81, 1), ()])
    D = props["bbox_reg_loss"](grad_scale="0.001", scalar="1.0")
    assert D.list_arguments() == ["bbox_delta", "bbox_target", "bbox_weight"]
    assert D.infer_shape([(1024, 324), (), (1024, 324)])[:2] == ([(1024, 324)] * 3, [(1024, 324)])
    with pytest.raises(ValueError):
        D.infer_shape([(1024, 324), (1024, 4), ()])


def test_without_the_reference_the_module_imports_and_patches_nothing(plug):
    rcnn_loss, _ = plug
    with pytest.raises(RuntimeError):
        rcnn_loss.patch_builders()                     # needs install()
    rcnn_loss.install(mx_stub.make_stub())
    assert REF not in sys.path and "symbol.builder" not in sys.modules
    assert rcnn_loss.patch_builders() is False and rcnn_loss.unpatch_builders() is False


def test_the_fpn_head_with_nnvm_rpn_target_stays_the_references(plug):
    import types
    rcnn_loss, mxnet_plugin = plug
    rcnn_loss.install(mx_stub.make_stub())
    calls = []

    def original(self, *a):
        calls.append(type(self).__name__)
        return "reference"
    mods = [types.SimpleNamespace(**{c: type(c, (), {"get_loss": original})}) for _, c, _ in rcnn_loss.METHODS]
    assert rcnn_loss.patch_builders(mods) is True
    head = mods[1].FPNRpnHead()
    head.p = types.SimpleNamespace(nnvm_rpn_target=True)
    assert head.get_loss({}, None, None) == "reference" and calls == ["FPNRpnHead"]
    assert mxnet_plugin._state["fallbacks"][-1][0] == "rpn_cls_loss"
    assert rcnn_loss.unpatch_builders(mods) is True and mods[1].FPNRpnHead.get_loss is original
    assert rcnn_loss.patch_builders([types.SimpleNamespace()] * 3) is False


def _fix_bn(*a, **k):
    raise AssertionError("not called")


_fix_bn.__name__ = "fix_bn"


def _rpn_param(fp16, fpn):
    class RpnParam:
        batch_image = 2
        nnvm_rpn_target = False
        nnvm_proposal = False
        normalizer = _fix_bn

        class anchor_generate:
            scale = (8,)
            ratio = (0.5, 1.0, 2.0)
            stride = (4, 8, 16, 32, 64) if fpn else 16
            image_anchor = 256

        class anchor_assign:
            image_anchor = 256

        class head:
            conv_channel = 256
    RpnParam.fp16 = fp16
    return RpnParam


def _bbox_param(fp16, scalar=None):
    class BboxParam:
        num_class = 81
        image_roi = 512
        batch_image = 2

        class regress_target:
            class_agnostic = False
            smooth_l1_scalar = None
    BboxParam.fp16 = fp16
    BboxParam.regress_target.smooth_l1_scalar = scalar
    return BboxParam


def _heads(R, fp16, scalar=None):
    """(C4 RPN losses, FPN RPN losses, R-CNN losses) built by the reference's classes as they stand"""
    SB = importlib.import_module("symbol.builder")
    FB = importlib.import_module("models.FPN.builder")
    v = R.mx.sym.var
    c4 = SB.RpnHead(_rpn_param(fp16, False))
    c4._cls_logit, c4._bbox_delta = v("c4_logit"), v("c4_delta")
    fpn = FB.FPNRpnHead(_rpn_param(fp16, True))
    fpn.cls_logit_dict = {s: v("logit_s%d" % s) for s in (4, 8, 16, 32, 64)}
    fpn.bbox_delta_dict = {s: v("delta_s%d" % s) for s in (4, 8, 16, 32, 64)}

    class Head(SB.BboxHead):
        def get_output(self, conv_feat):
            return v("bbox_logit"), v("bbox_delta")
    box = Head(_bbox_param(fp16, scalar))
    return (c4.get_loss(v("feat"), None, None), fpn.get_loss({}, None, None),
            box.get_loss(v("feat"), v("label"), v("target"), v("weight")), (c4, fpn, box))


def _named(syms, name):
    found = [n for n in RS.walk(RS.Symbol("Group", list(syms)), {}).values() if n.name == name]
    assert len(found) == 1, (name, found)
    return found[0]


@needs_ref
@pytest.mark.parametrize("fp16", [False, True])
def test_patched_get_loss_emits_the_four_nodes_with_the_reference_names_and_parameters(plug, fp16):
    rcnn_loss, mxnet_plugin = plug
    flags = tuple(mxnet_plugin.FEATURE_FLAGS)
    shift = 128.0 if fp16 else 1.0
    with RS.reference_modules() as R:
        rcnn_loss.install(R.mx)
        SB = importlib.import_module("symbol.builder")
        FB = importlib.import_module("models.FPN.builder")
        reference = [SB.RpnHead.get_loss, FB.FPNRpnHead.get_loss, SB.BboxHead.get_loss]
        nc4, nfpn, nbox, _ = _heads(R, fp16)
        for syms, ops in ((nc4, ("SoftmaxOutput", "MakeLoss")), (nfpn, ("SoftmaxOutput", "MakeLoss")),
                          (nbox, ("SoftmaxOutput", "MakeLoss"))):
            assert tuple(RS.source(s).op_type for s in syms[:2]) == ops
        assert [n.op_type for n in RS.walk(RS.Symbol("Group", list(nfpn)), {}).values()].count("concat") == 2

        assert rcnn_loss.patch_builders() is True
        assert rcnn_loss.patch_builders() is True                  # a second call keeps the first originals
        assert [SB.RpnHead._sd_reference_get_loss, FB.FPNRpnHead._sd_reference_get_loss,
                SB.BboxHead._sd_reference_get_loss] == reference
        c4, fpn, box, heads = _heads(R, fp16, scalar=None if not fp16 else 3.0)
        assert len(c4) == 2 and len(fpn) == 3 and len(box) == 3

        # the C4 head: one level, the logits and deltas as the head made them
        n = _named(c4, "rpn_cls_loss")
        assert n is c4[0] and n.op_type == "sd_rpn_cls_loss" and n.nout == 1
        assert n.params == dict(num_level="1", grad_scale=repr(1.0 * shift), ignore_label="-1", normalization="valid",
                                use_ignore="True", multi_output="True")
        assert [(i.op_type, i.name) for i in n.inputs] == [("var", "c4_logit"), ("var", "rpn_cls_label")]
        n = _named(c4, "rpn_reg_loss")
        assert n is c4[1] and n.op_type == "sd_rpn_reg_loss"
        assert n.params == dict(num_level="1", scalar="3.0", grad_scale=repr(1.0 / (2 * 256) * shift))
        assert [i.name for i in n.inputs] == ["c4_delta", "rpn_reg_target", "rpn_reg_weight"]

        # the FPN head: the five level tensors straight into the node, no reshape and no concat in front
        n = _named(fpn, "rpn_cls_loss")
        assert n is fpn[0] and n.op_type == "sd_rpn_cls_loss" and n.params["num_level"] == "5"
        assert n.params["grad_scale"] == repr(1.0 * shift) and n.params["ignore_label"] == "-1"
        assert [i.name for i in n.inputs] == ["logit_s%d" % s for s in (4, 8, 16, 32, 64)] + ["rpn_cls_label"]
        m = _named(fpn, "rpn_reg_loss")
        assert m is fpn[1] and m.params == dict(num_level="5", scalar="3.0", grad_scale=repr(1.0 / (2 * 256) * shift))
        assert [i.name for i in m.inputs] == ["delta_s%d" % s for s in (4, 8, 16, 32, 64)] + ["rpn_reg_target",
                                                                                           "rpn_reg_weight"]
        kinds = [x.op_type for x in RS.walk(RS.Symbol("Group", list(fpn)), {}).values()]
        assert "concat" not in kinds and "reshape" not in kinds and "SoftmaxOutput" not in kinds
        # the label output stays the reference's node, on the label the loss node reads
        assert fpn[2].op_type == "BlockGrad" and fpn[2].name == "rpn_cls_label_blockgrad"
        assert fpn[2].inputs[0] is n.inputs[-1]

        # the R-CNN head
        n = _named(box, "bbox_cls_loss")
        assert n is box[0] and n.op_type == "sd_bbox_cls_loss"
        assert n.params == dict(grad_scale=repr(1.0 * shift), normalization="batch")
        assert [i.name for i in n.inputs] == ["bbox_logit", "label"]
        n = _named(box, "bbox_reg_loss")
        assert n is box[1] and n.op_type == "sd_bbox_reg_loss"
        assert n.params == dict(scalar=repr(3.0 if fp16 else 1.0), grad_scale=repr(1.0 / 1024 * shift))
        assert [i.name for i in n.inputs] == ["bbox_delta", "target", "weight"]
        assert box[2].op_type == "BlockGrad" and box[2].name == "bbox_label_blockgrad"
        assert box[2].inputs[0].op_type == "reshape" and box[2].inputs[0].name == "bbox_label_reshape"
        assert box[2].inputs[0].params["shape"] == (2, -1)

        assert mxnet_plugin.FEATURE_FLAGS == flags

        assert rcnn_loss.unpatch_builders() is True
        assert [SB.RpnHead.get_loss, FB.FPNRpnHead.get_loss, SB.BboxHead.get_loss] == reference
        assert not any("_sd_reference_get_loss" in c.__dict__ for c in (SB.RpnHead, FB.FPNRpnHead, SB.BboxHead))
        assert rcnn_loss.unpatch_builders() is False
        back = _heads(R, fp16)
        assert [RS.source(s).op_type for s in back[1][:2]] == ["SoftmaxOutput", "MakeLoss"]


@needs_ref
def test_the_train_symbol_of_the_bench_config_binds_the_same_output_names(plug):
    rcnn_loss, mxnet_plugin = plug
    with RS.reference_modules() as R:
        mxnet_plugin._state.update(registered=False)
        mxnet_plugin.install(R.mx)
        rcnn_loss.install(R.mx)

        def train():
            for mod in [m for m in sys.modules if m.startswith("config.")]:
                del sys.modules[mod]
            cfg = importlib.import_module("config.faster_r50v1_fpn_1x")
            for o in cfg.get_config(True):
                s = getattr(o, "train_symbol", None)
                if isinstance(s, RS.Symbol):
                    return s
            raise AssertionError("no train symbol")
        native = train()
        assert rcnn_loss.patch_builders()
        try:
            patched = train()
        finally:
            rcnn_loss.unpatch_builders()
        heads = lambda s: [RS.source(h) for h in (s.inputs if s.op_type == "Group" else list(s))]
        assert [h.name for h in heads(patched)] == [h.name for h in heads(native)]
        got = {h.name: h.op_type for h in heads(patched)}
        was = {h.name: h.op_type for h in heads(native)}
        assert {n: got[n] for n in NAMES} == {n: "sd_" + n for n in NAMES}
        assert [was[n] for n in NAMES] == ["SoftmaxOutput", "MakeLoss"] * 2
        # every other head, the two label outputs among them, is the node it was
        assert {n: t for n, t in got.items() if n not in NAMES} == {n: t for n, t in was.items() if n not in NAMES}
        assert got["rpn_cls_label_blockgrad"] == "BlockGrad" and got["bbox_label_blockgrad"] == "BlockGrad"


@pytest.mark.gpu
def test_adapter_round_trip_equals_the_ops_calls(plug):
    import torch
    from simpledet_amd import ops
    from . import rcnn_loss_ref as rl
    rcnn_loss, _ = plug
    mx = mx_stub.make_stub()
    props = rcnn_loss.install(mx)
    bits = lambda t: t.contiguous().view(torch.int32)
    c = rl.make_rpn_case("fpn5")
    cls = [torch.from_numpy(t).cuda() for t in c["cls"]]
    delta = [torch.from_numpy(t).cuda() for t in c["delta"]]
    label, target, weight = [torch.from_numpy(c[k]).cuda() for k in ("label", "target", "weight")]
    want = ops.rpn_loss_forward(cls, delta, label, target, weight)
    wg = ops.rpn_loss_backward(cls, delta, label, target, weight, want.state, cls_grad_scale=128.0, reg_grad_scale=0.25)
    for name, ins, kw, w, wgrad in (
            ("rpn_cls_loss", cls + [label], dict(num_level="5", grad_scale="128.0"), want.prob, wg[0]),
            ("rpn_reg_loss", delta + [target, weight], dict(num_level="5", grad_scale="0.25", scalar="3.0"),
             want.reg_loss, wg[1])):
        P = props[name](**kw)
        ishape, oshape, _ = P.infer_shape([tuple(t.shape) for t in ins])
        op = P.create_operator(None, ishape, None)
        out = [mx_stub.wrap(torch.full(oshape[0], float("nan"), device="cuda"))]
        nd = [mx_stub.wrap(t) for t in ins]
        op.forward(True, ["write"], nd, out, [])
        assert torch.equal(bits(out[0].t), bits(w.reshape(oshape[0])))
        grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7.0, device="cuda")) for t in ins]
        op.backward(["write"] * len(ins), [], nd, out, grads, [])
        for g, x in zip(grads, wgrad):
            assert torch.equal(bits(g.t), bits(x))
        assert any(bool(x.any()) for x in wgrad)          # (a level of one position may hold ignored labels only)
        assert all(not g.t.any() for g in grads[5:])
        with pytest.raises(RuntimeError):
            op.backward(["add"] + ["write"] * (len(ins) - 1), [], nd, out, grads, [])
    r = rl.make_rcnn_case(130, 81, False)
    x, lab, d, t, w = [torch.from_numpy(r[k]).cuda() for k in ("x", "label", "delta", "target", "weight")]
    want = ops.rcnn_loss_forward(x, lab, d, t, w, smooth_l1_scalar=r["sigma"])
    wg = ops.rcnn_loss_backward(x, lab, d, t, w, want.state, cls_grad_scale=128.0, reg_grad_scale=0.5,
                                smooth_l1_scalar=r["sigma"])
    for name, ins, kw, wout, wgrad in (
            ("bbox_cls_loss", [x, lab], dict(grad_scale="128.0", normalization="batch"), want.prob, wg[0]),
            ("bbox_reg_loss", [d, t, w], dict(grad_scale="0.5", scalar=repr(r["sigma"])), want.reg_loss, wg[1])):
        P = props[name](**kw)
        ishape, oshape, _ = P.infer_shape([tuple(a.shape) for a in ins])
        op = P.create_operator(None, ishape, None)
        out = [mx_stub.wrap(torch.full(oshape[0], float("nan"), device="cuda"))]
        nd = [mx_stub.wrap(a) for a in ins]
        op.forward(True, ["write"], nd, out, [])
        assert torch.equal(bits(out[0].t), bits(wout))
        grads = [mx_stub.wrap(torch.full(tuple(a.shape), 7.0, device="cuda")) for a in ins]
        op.backward(["write"] * len(ins), [], nd, out, grads, [])
        assert torch.equal(bits(grads[0].t), bits(wgrad)) and all(not g.t.any() for g in grads[1:])
    assert np.isfinite(want.prob.cpu().numpy()).all()
