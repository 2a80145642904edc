"""`install(mx, fcos=True)`: the train symbol of config/fcos_r50v1_fpn_1x.py holds ONE `sd_fcos_target` and ONE
`sd_fcos_loss` node in place of make_fcos_gt (two Python CustomOps, ~60 nodes), the per-level reshape + concat of
the logits and the three loss subgraphs with their pass-through CustomOps (models/FCOS/builder.py:181-231).  Without
the flag the graph holds what it held.  CPU only on tests/mx_stub.py and tests/ref_stubs.py (the builder tests are
skipped where the reference tree is absent, like tests/test_mask_loss_plugin.py); the GPU round trip through the
adapter is the last test."""
import collections
import importlib
import os

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
REFERENCE_ONLY = ("make_fcos_gt_preparation", "prepare_fcos_cls_gt", "compute_focal_loss", "compute_bce_loss")


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def plugin():
    mx, props, mxnet_plugin = _fresh(fcos=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_nothing_new():
    mx, props, mxnet_plugin = _fresh()
    try:
        assert "fcos_target" not in props and "fcos_loss" not in props
        assert "sd_fcos_target" not in mx.registry and "sd_fcos_loss" not in mx.registry
        assert mxnet_plugin._state["fcos_patched"] is False
        mx2, props2, _ = _fresh(**{f: True for f in mxnet_plugin.FEATURE_FLAGS if f != "fcos"})
        assert "fcos_target" not in props2 and "sd_fcos_loss" not in mx2.registry
    finally:
        mxnet_plugin._state.update(registered=False)


def test_props_shapes_types_and_arguments(plugin):
    mx, props, _ = plugin
    assert "sd_fcos_target" in mx.registry and "sd_fcos_loss" in mx.registry
    T = props["fcos_target"](data_size="(800, 1333)", stride="(8, 16, 32, 64, 128)", num_classifier="80")
    assert T.g == dict(data_size=(800, 1333), stride=(8, 16, 32, 64, 128), num_classifier=80, ignore_offset=-1.0,
                       ignore_label=-1.0)
    assert T.list_arguments() == ["gt_bbox", "im_info"] and T.need_top_grad_ is False
    assert T.list_outputs() == ["centerness", "offset", "cls_id", "state"]
    # the reference's infer_shape (models/FCOS/input.py:99-107): HW = 22300 at 800 x 1333
    assert T.infer_shape([(2, 100, 5), (2, 3)]) == ([(2, 100, 5), (2, 3)], [(2, 22300), (2, 4, 22300), (2, 22300), (4,)])
    assert T.infer_shape([(2, 100, 5), ()])[0][1] == (2, 3)
    assert T.infer_type([np.float32, np.float32])[1] == [np.float32, np.float32, np.int32, np.int32]
    assert T.declare_backward_dependency([], ["g", "i"], ["a", "b", "c", "d"]) == []
    with pytest.raises(ValueError):
        T.infer_shape([(2, 100, 4), (2, 3)])
    with pytest.raises(ValueError):
        props["fcos_target"](data_size="(800,)", stride="(8,)", num_classifier="80")
    Lp = props["fcos_loss"](num_levels="2", alpha="0.25", gamma="2.0")
    assert Lp.g == dict(num_levels=2, alpha=0.25, gamma=2.0, ignore_offset=-1.0, ignore_label=-1.0)
    assert Lp.list_arguments() == ["cls_logit_0", "cls_logit_1", "centerness_logit_0", "centerness_logit_1",
                                   "offset_logit_0", "offset_logit_1", "centerness", "offset", "cls_id", "state"]
    assert Lp.list_outputs() == ["centerness_loss", "cls_loss", "offset_loss"] and Lp.need_top_grad_ is False
    shapes = [(2, 80, 8, 12), (2, 80, 4, 6), (2, 1, 8, 12), (2, 1, 4, 6), (2, 4, 8, 12), (2, 4, 4, 6), (), (), (), ()]
    ins, outs = Lp.infer_shape(shapes)
    assert ins[6:] == [(2, 120), (2, 4, 120), (2, 120), (4,)] and outs == [(1,)] * 3
    assert Lp.infer_type([np.float32] * 10)[0][-2:] == [np.int32, np.int32]
    with pytest.raises(ValueError):
        Lp.infer_shape(shapes[:2] + [(2, 1, 8, 12), (2, 1, 4, 7)] + shapes[4:])
    with pytest.raises(ValueError):
        Lp.infer_shape(shapes[:6] + [(2, 121), (), (), ()])
    with pytest.raises(ValueError):
        props["fcos_loss"](num_levels="9")


def _train_symbol(R, **flags):
    from simpledet_amd import mxnet_plugin as plug
    plug._state.update(registered=False)
    plug.install(R.mx, **flags)
    cfg = importlib.import_module("config.fcos_r50v1_fpn_1x")
    train = test = None
    for is_train in (True, False):
        for o in cfg.get_config(is_train):
            s = getattr(o, "train_symbol" if is_train else "test_symbol", None)
            if isinstance(s, RS.Symbol):
                if is_train:
                    train = s
                else:
                    test = s
    return train, test


def _ops(sym):
    return collections.Counter(n.op_type for n in RS.walk(sym, {}).values())


def _shape_of(sym):
    """(op_type, name, params, input ops) per node in walk order: the graph node for node"""
    return [(n.op_type, n.name, sorted((k, repr(v)) for k, v in n.params.items()), [i.op_type for i in n.inputs])
            for n in RS.walk(sym, {}).values()]


@needs_ref
def test_fcos_train_symbol_holds_the_two_device_nodes():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.FCOS.builder")
        reference_get_loss = builder.FCOSFPNHead.get_loss
        native_train, native_test = _train_symbol(R)
        assert builder.FCOSFPNHead.get_loss is reference_get_loss and not plug._state["fcos_patched"]
        native = _ops(native_train)
        assert all(native[o] == 1 for o in REFERENCE_ONLY) and native["sd_fcos_loss"] == 0
        assert native["concat"] >= 3

        train, test = _train_symbol(R, fcos=True)
        assert plug._state["fcos_patched"] and builder.FCOSFPNHead._sd_reference_get_loss is reference_get_loss
        plug.install(R.mx, fcos=True)                # a second install keeps the first original
        assert builder.FCOSFPNHead._sd_reference_get_loss is reference_get_loss
        got = _ops(train)
        assert got["sd_fcos_target"] == 1 and got["sd_fcos_loss"] == 1
        assert all(got[o] == 0 for o in REFERENCE_ONLY), dict(got)
        assert got["MakeLoss"] == 0 and got["gather_nd"] == 0 and got["argmin"] == 0 and got["one_hot"] == 0
        # three outputs in the reference's order: centerness, cls, offset -- outputs 0, 1, 2 of the loss node
        heads = train.inputs if train.op_type == "Group" else list(train)
        assert [h.op_type for h in heads] == ["_output"] * 3 and [h.index for h in heads] == [0, 1, 2]
        loss = RS.source(heads[0])
        assert all(RS.source(h) is loss for h in heads) and loss.op_type == "sd_fcos_loss" and loss.nout == 3
        assert loss.params == {"num_levels": "5", "alpha": "0.25", "gamma": "2.0", "ignore_offset": "-1",
                               "ignore_label": "-1"}
        # its inputs: 5 class logits (Convolution), 5 centerness logits (Convolution), 5 offsets (exp), 4 targets
        ins = [RS.source(i) for i in loss.inputs]
        assert len(ins) == 19
        assert [n.op_type for n in ins[:10]] == ["Convolution"] * 10 and [n.op_type for n in ins[10:15]] == ["exp"] * 5
        strides = (8, 16, 32, 64, 128)
        assert [n.name for n in ins[:5]] == ["cls_conv_3x3_%d" % s for s in strides]
        assert [n.name for n in ins[5:10]] == ["center_conv_3x3_%d" % s for s in strides]
        target = ins[15]
        assert all(n is target for n in ins[15:]) and [i.index for i in loss.inputs[15:]] == [0, 1, 2, 3]
        assert target.op_type == "sd_fcos_target" and target.nout == 4
        assert target.params == {"data_size": "(800, 1333)", "stride": "(8, 16, 32, 64, 128)", "num_classifier": "80",
                                 "ignore_offset": "-1", "ignore_label": "-1"}
        assert [i.name for i in target.inputs] == ["gt_bbox", "im_info"]
        # no Concat (and no reshape) between the head convs and the loss
        between = _ops(loss)
        assert between["concat"] == 0 and between["Concat"] == 0 and between["reshape"] == 0
        # everything in front of the head is untouched
        rest = lambda c, drop: {k: v for k, v in c.items() if k not in drop}
        head_only = set(native) - set(got) | {"sd_fcos_target", "sd_fcos_loss", "_output", "var", "_mul", "_plus",
                                               "_minus", "_rminus", "_div", "_rdiv", "_power", "_neg", "reshape",
                                               "concat", "exp", "log", "clip", "sum", "stack", "slice", "min", "max",
                                               "BlockGrad", "broadcast_mul", "broadcast_add", "_greater_equal",
                                               "_not_equal_scalar", "sort", "sqrt", "zeros", "full"}
        assert rest(native, head_only) == rest(got, head_only)
        assert got["Convolution"] == native["Convolution"] and got["exp"] == 5
        # the test symbol is unchanged
        assert _shape_of(test) == _shape_of(native_test)

        # a default install() afterwards: the graph is node for node the native one
        again_train, again_test = _train_symbol(R)
        assert builder.FCOSFPNHead.get_loss is reference_get_loss and not plug._state["fcos_patched"]
        assert _shape_of(again_train) == _shape_of(native_train) and _shape_of(again_test) == _shape_of(native_test)
        plug._state.update(registered=False)


@pytest.mark.gpu
def test_adapter_round_trip_equals_the_ops_calls(plugin, ops):
    import torch
    from . import fcos_ref as fr
    mx, props, _ = plugin
    name, c = fr.loss_cases()[3]                                  # data_size (72, 40), M = 70, K = 3
    case = c["case"]
    T = props["fcos_target"](data_size=str(case["data_size"]), stride=str(case["strides"]), num_classifier=str(case["K"]))
    ishape, oshape = T.infer_shape([case["gt_bbox"].shape, case["im_info"].shape])[:2]
    dt = T.infer_type([np.float32] * 2)[1]
    op = T.create_operator(None, ishape, None)
    ins = [mx_stub.wrap(torch.from_numpy(a).cuda()) for a in (case["gt_bbox"], case["im_info"])]
    outs = [mx_stub.wrap(torch.zeros(s, device="cuda", dtype=torch.int32 if d is np.int32 else torch.float32))
            for s, d in zip(oshape, dt)]
    op.forward(True, ["write"] * 4, ins, outs, [])
    want = ops.fcos_target(ins[0].t, ins[1].t, case["data_size"], case["strides"], case["K"])
    for g, w in zip(outs, (want.centerness, want.offset, want.cls_id, want.state)):
        assert g.t.shape == w.shape and torch.equal(g.t.view(torch.int32), w.view(torch.int32))
    sizes = fr.level_sizes(case["data_size"], case["strides"])
    lv = []
    for flat, C in ((c["cls"], case["K"]), (c["ctr"], 1), (c["off"], 4)):
        shapes = [(flat.shape[0], C, a, b) for a, b in sizes]
        lv.append([torch.from_numpy(v).cuda() for v in fr.split_levels(flat, c["hws"], shapes)])
    Lp = props["fcos_loss"](num_levels="5", alpha=str(c["alpha"]), gamma=str(c["gamma"]))
    tensors = lv[0] + lv[1] + lv[2] + [o.t for o in outs]
    ishape, oshape = Lp.infer_shape([tuple(t.shape) for t in tensors])[:2]
    op = Lp.create_operator(None, ishape, None)
    ins = [mx_stub.wrap(t) for t in tensors]
    louts = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
    op.forward(True, ["write"] * 3, ins, louts, [])
    kw = dict(alpha=c["alpha"], gamma=c["gamma"])
    wl = ops.fcos_loss_forward(*lv, want, **kw)
    assert torch.equal(torch.cat([o.t for o in louts]).view(torch.int32), wl.view(torch.int32))
    grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7, device="cuda", dtype=t.dtype)) for t in tensors]
    op.backward(["write"] * 19, [], ins, louts, grads, [])
    wg = ops.fcos_loss_backward(*lv, want, **kw)
    for g, w in zip(grads[:15], [x for lst in wg for x in lst]):
        assert torch.equal(g.t.view(torch.int32), w.view(torch.int32))
    assert all(not g.t.any() for g in grads[15:])
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["add"] + ["write"] * 18, [], ins, louts, grads, [])
    with pytest.raises(RuntimeError, match="one launch"):
        op.backward(["null"] + ["write"] * 18, [], ins, louts, grads, [])
