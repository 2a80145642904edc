"""`install(mx, fcos_decode=True)`: the test symbol of config/fcos_r50v1_fpn_1x.py holds ONE `sd_fcos_decode` node in
place of the ten sigmoid nodes, the five Python CustomOps get_proposal_single_stage, the concat and the Python CustomOp
get_batch_proposal (models/FCOS/builder.py:234-259).  Without the flag -- `fcos=True` included -- the graph holds what
it held.  CPU only on tests/mx_stub.py and tests/ref_stubs.py (the builder tests are skipped where the reference tree
is absent, like tests/test_fcos_plugin.py); the GPU round trip through the adapter is the last test."""
import collections
import importlib
import os

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
REFERENCE_ONLY = ("get_proposal_single_stage", "get_batch_proposal", "sigmoid")


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def plugin():
    mx, props, mxnet_plugin = _fresh(fcos_decode=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_and_fcos_installs_register_nothing_new():
    from simpledet_amd.mxnet_plugin import FEATURE_FLAGS
    for flags in ({}, dict(fcos=True), {f: True for f in FEATURE_FLAGS if f != "fcos_decode"}):
        mx, props, mxnet_plugin = _fresh(**flags)
        try:
            assert "fcos_decode" not in props and "sd_fcos_decode" not in mx.registry
            assert mxnet_plugin._state["fcos_decode_patched"] is False
        finally:
            mxnet_plugin._state.update(registered=False)


def test_prop_shapes_types_and_arguments(plugin):
    mx, props, plug = plugin
    assert "sd_fcos_decode" in mx.registry and "sd_fcos_loss" not in mx.registry
    P = props["fcos_decode"](stride="(8, 16)", pre_nms_top_n="1000", pre_nms_thresh="0.05")
    assert P.g == dict(stride=(8, 16), pre_nms_top_n=1000, pre_nms_thresh=0.05, input_logits=True, num_levels=2)
    assert P.list_arguments() == ["cls_logit_0", "cls_logit_1", "centerness_logit_0", "centerness_logit_1",
                                   "offset_logit_0", "offset_logit_1", "im_info"]
    assert len(P.list_arguments()) == 3 * 2 + 1
    assert P.list_outputs() == ["bbox", "score", "cls_id"] and P.need_top_grad_ is False
    shapes = [(2, 80, 8, 12), (2, 80, 4, 6), (2, 1, 8, 12), (2, 1, 4, 6), (2, 4, 8, 12), (2, 4, 4, 6), ()]
    ins, outs = P.infer_shape(shapes)[:2]
    assert ins[6] == (2, 3) and outs == [(2, 2000, 4), (2, 2000, 81), (2, 2000)]
    assert P.infer_type([np.float32] * 7)[1] == [np.float32] * 3
    assert P.declare_backward_dependency([], list("abcdefg"), list("xyz")) == []
    assert props["fcos_decode"](stride="(8,)", pre_nms_top_n="5", pre_nms_thresh="0.1", input_logits="0").g["input_logits"] is False
    with pytest.raises(ValueError):
        P.infer_shape(shapes[:2] + [(2, 1, 8, 12), (2, 1, 4, 7)] + shapes[4:])
    with pytest.raises(ValueError):
        P.infer_shape(shapes[:6] + [(2, 4)])
    with pytest.raises(ValueError):
        P.infer_shape(shapes[:6])
    with pytest.raises(ValueError):
        props["fcos_decode"](stride="(1, 2, 3, 4, 5, 6, 7, 8, 9)", pre_nms_top_n="5", pre_nms_thresh="0.1")
    with pytest.raises(ValueError):
        props["fcos_decode"](stride="(8,)", pre_nms_top_n="0", pre_nms_thresh="0.1")
    # the builder module is absent here: nothing is rebound and the fallback list says so
    if not os.path.isdir(REF):
        assert plug._state["fcos_decode_patched"] is False
        assert [f[0] for f in plug._state["fallbacks"]] == ["fcos_decode"]


def _symbols(R, **flags):
    from simpledet_amd import mxnet_plugin as plug
    plug._state.update(registered=False)
    plug.install(R.mx, **flags)
    cfg = importlib.import_module("config.fcos_r50v1_fpn_1x")
    # the reference's detector keeps the first test symbol it built on its class (symbol/builder.py:26-27, 38): a
    # process builds it once; this test builds it several times
    importlib.import_module("symbol.builder").RPN._rpn_output = None
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
    return [(n.op_type, n.name, sorted((k, repr(v)) for k, v in n.params.items()), [i.op_type for i in n.inputs])
            for n in RS.walk(sym, {}).values()]


def _find(sym, op_type):
    return [n for n in RS.walk(sym, {}).values() if n.op_type == op_type]


@needs_ref
def test_fcos_test_symbol_holds_the_one_device_node():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.FCOS.builder")
        reference = builder.FCOSFPNHead.get_all_proposal
        native_train, native_test = _symbols(R)
        assert builder.FCOSFPNHead.get_all_proposal is reference and not plug._state["fcos_decode_patched"]
        native = _ops(native_test)
        assert native["get_proposal_single_stage"] == 5 and native["get_batch_proposal"] == 1
        assert native["sigmoid"] == 10 and native["sd_fcos_decode"] == 0

        # fcos=True alone: the train head only, get_all_proposal untouched
        _, only_train_flag = _symbols(R, fcos=True)
        assert builder.FCOSFPNHead.get_all_proposal is reference
        assert _shape_of(only_train_flag) == _shape_of(native_test)

        train, test = _symbols(R, fcos_decode=True)
        assert plug._state["fcos_decode_patched"] and not plug._state["fcos_patched"]
        assert builder.FCOSFPNHead._sd_reference_get_all_proposal is reference
        assert not any(f[0] == "fcos_decode" for f in plug._state["fallbacks"])
        plug.install(R.mx, fcos_decode=True)          # a second install keeps the first original
        assert builder.FCOSFPNHead._sd_reference_get_all_proposal is reference
        got = _ops(test)
        assert got["sd_fcos_decode"] == 1 and all(got[o] == 0 for o in REFERENCE_ONLY), dict(got)
        node, = _find(test, "sd_fcos_decode")
        assert node.nout == 3
        assert node.params == {"stride": "(8, 16, 32, 64, 128)", "pre_nms_top_n": "1000", "pre_nms_thresh": "0.05",
                               "input_logits": "1"}
        # its inputs: 5 class logits and 5 centerness logits straight from the convolutions, 5 offsets (exp), im_info
        ins = [RS.source(i) for i in node.inputs]
        assert len(ins) == 16
        assert [n.op_type for n in ins[:10]] == ["Convolution"] * 10 and [n.op_type for n in ins[10:15]] == ["exp"] * 5
        strides = (8, 16, 32, 64, 128)
        assert [n.name for n in ins[:5]] == ["cls_conv_3x3_%d" % s for s in strides]
        assert [n.name for n in ins[5:10]] == ["center_conv_3x3_%d" % s for s in strides]
        assert node.inputs[15].name == "im_info"
        # the two things the head hands on are outputs 1 (score) and 0 (bbox) of that node
        heads = test.inputs if test.op_type == "Group" else list(test)
        from_node = [h for h in heads if RS.source(h) is node]
        assert sorted(h.index for h in from_node) == [0, 1]
        # everything in front of the head is untouched, and so is the train symbol
        assert got["Convolution"] == native["Convolution"] and got["exp"] == native["exp"] == 5
        assert _shape_of(train) == _shape_of(native_train)

        # both flags together
        train2, test2 = _symbols(R, fcos=True, fcos_decode=True)
        assert _ops(train2)["sd_fcos_loss"] == 1 and _ops(test2)["sd_fcos_decode"] == 1

        # a default install() afterwards: the graphs are node for node the native ones
        again_train, again_test = _symbols(R)
        assert builder.FCOSFPNHead.get_all_proposal is reference and not plug._state["fcos_decode_patched"]
        assert _shape_of(again_test) == _shape_of(native_test) and _shape_of(again_train) == _shape_of(native_train)
        plug._state.update(registered=False)


@pytest.mark.gpu
def test_adapter_forward_equals_the_ops_call(plugin, ops):
    import torch
    from . import fcos_decode_ref as dr
    mx, props, _ = plugin
    c = dict(dr.cases())["branches"]
    rs = np.random.RandomState(3)
    cls = [(rs.standard_normal(x.shape) * 1.5 - 3.0).astype(np.float32) for x in c["cls"]]
    ctr = [rs.standard_normal(x.shape).astype(np.float32) for x in c["ctr"]]
    tensors = [torch.from_numpy(a).cuda() for a in cls + ctr + c["off"] + [c["im_info"]]]
    L = len(cls)
    P = props["fcos_decode"](stride=str(tuple(c["strides"])), pre_nms_top_n=str(c["top_n"]),
                             pre_nms_thresh=str(c["thresh"]))
    ishape, oshape = P.infer_shape([tuple(t.shape) for t in tensors])[:2]
    op = P.create_operator(None, ishape, None)
    ins = [mx_stub.wrap(t) for t in tensors]
    outs = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
    op.forward(False, ["write"] * 3, ins, outs, [])
    want = ops.fcos_decode(tensors[:L], tensors[L:2 * L], tensors[2 * L:3 * L], tensors[3 * L], c["strides"],
                           c["top_n"], c["thresh"], input_logits=True)
    for g, w in zip(outs, want):
        assert g.t.shape == w.shape and torch.equal(g.t.view(torch.int32), w.view(torch.int32))
    grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7.0, device="cuda")) for t in tensors]
    op.backward(["write"] * len(tensors), [], ins, outs, grads, [])
    assert all(not g.t.any() for g in grads)
    with pytest.raises(RuntimeError, match="kAddTo"):
        op.forward(False, ["add"] + ["write"] * 2, ins, outs, [])
