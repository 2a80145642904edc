"""`install(mx, mask_loss=True)`: `mx.sym.contrib.SigmoidCrossEntropy` builds an `sd__contrib_SigmoidCrossEntropy`
Custom node with the reference's arguments, five outputs (1 visible), parameters and shape inference
(sigmoid_cross_entropy-inl.h:49-61,130-206), and `MaskFasterRcnnHead.get_loss` of models/maskrcnn/builder.py:278-313
emits ONE `sd_MaskLoss` node in place of split / stack / gather_nd / concat / reshape / SigmoidCrossEntropy.  Without
the flag the graph holds what it held.  CPU only on tests/mx_stub.py and tests/ref_stubs.py (the builder tests are
skipped where /root/reference is absent, like tests/test_bbox_post_plugin.py); the GPU round trip through the
adapter is the last test."""
import collections
import importlib
import os
import types

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
SUBGRAPH = ("gather_nd", "stack", "split", "concat", "arange")


def _native(*a, **kw):
    return ("native SigmoidCrossEntropy", a, kw)


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mx.sym.contrib.SigmoidCrossEntropy = _native     # what a SimpleDet build of MXNet registers natively
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def plugin():
    mx, props, mxnet_plugin = _fresh(mask_loss=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_nothing_new_and_leaves_the_graph_alone():
    mx, props, mxnet_plugin = _fresh()
    try:
        assert "_contrib_SigmoidCrossEntropy" not in props and "MaskLoss" not in props
        assert "sd__contrib_SigmoidCrossEntropy" not in mx.registry and "sd_MaskLoss" not in mx.registry
        assert mx.sym.contrib.SigmoidCrossEntropy is _native
        assert mxnet_plugin._state["mask_loss_patched"] is False
        v = mx.sym.Variable
        assert mx.sym.contrib.SigmoidCrossEntropy(v("a"), v("b"), grad_scale=1.0, name="mask_loss")[0] \
            == "native SigmoidCrossEntropy"
        # the other opt-in flags do not bring it in either
        mx2, props2, _ = _fresh(**{f: True for f in mxnet_plugin.FEATURE_FLAGS if f != "mask_loss"})
        assert "_contrib_SigmoidCrossEntropy" not in props2 and mx2.sym.contrib.SigmoidCrossEntropy is _native
    finally:
        mxnet_plugin._state.update(registered=False)


def test_with_the_flag_the_operator_is_one_device_node(plugin):
    mx, props, mxnet_plugin = plugin
    assert "sd__contrib_SigmoidCrossEntropy" in mx.registry and "sd_MaskLoss" in mx.registry
    assert mx.sym.contrib.SigmoidCrossEntropy is not _native
    assert mx.sym.contrib._sd_reference_SigmoidCrossEntropy is _native
    v = mx.sym.Variable
    out = mx.sym.contrib.SigmoidCrossEntropy(v("a"), v("b"), grad_scale=128.0, name="mask_loss")
    assert out[0] == "out" and out[2] == 0            # one visible output: output 0 of the five-output node
    node = out[1]
    assert node.op_type == "sd__contrib_SigmoidCrossEntropy" and node.nout == 5 and len(node.inputs) == 2
    assert node.params == {"grad_scale": "128.0"}
    node = mx.sym.contrib.SigmoidCrossEntropy(data=v("a"), label=v("b"), normalization="valid")[1]
    assert node.op_type == "sd__contrib_SigmoidCrossEntropy" and node.params == {"normalization": "valid"}
    # a default install() afterwards puts the native constructor back
    mxnet_plugin._state.update(registered=False)
    mxnet_plugin.install(mx)
    assert mx.sym.contrib.SigmoidCrossEntropy is _native
    assert not hasattr(mx.sym.contrib, "_sd_reference_SigmoidCrossEntropy")


def test_props_mirror_the_reference_operator(plugin):
    mx, props, _ = plugin
    P = props["_contrib_SigmoidCrossEntropy"]
    p = P()
    assert p.g == {"grad_scale": 1.0, "normalization": "valid"}          # sigmoid_cross_entropy-inl.h:52-60
    assert p.list_arguments() == ["data", "label"]
    assert p.list_outputs() == ["output", "loss", "loss_sum", "count", "count_sum"]
    assert p.num_visible_outputs == 1 and p.need_top_grad_ is False
    # InferShape (:152-172): the reference's five shapes
    assert p.infer_shape([(1, 200704), (1, 200704)]) == (
        [(1, 200704), (1, 200704)], [(1,), (1, 200704), (1,), (1, 200704), (1,)])
    assert p.infer_shape([(4, 3, 28, 28), ()])[1] == [(4,), (4, 3, 28, 28), (4,), (4, 3, 28, 28), (4,)]
    with pytest.raises(ValueError):
        p.infer_shape([(7,), (7,)])
    # DeclareBackwardDependency (:200-206): data, label, count, count_sum; no out_grad
    assert p.declare_backward_dependency(["g"], ["x", "t"], ["o", "l", "ls", "c", "cs"]) == ["x", "t", "c", "cs"]
    q = P(grad_scale="128.0", normalization="null")                      # parsed, never used by the operator
    assert q.g["grad_scale"] == 128.0
    with pytest.raises(ValueError):
        P(normalization="batch")
    M = props["MaskLoss"]
    m = M(grad_scale="128.0")
    assert m.g == {"grad_scale": 128.0} and m.need_top_grad_ is False and m.num_visible_outputs == 1
    assert m.list_arguments() == ["logits", "cls", "target"] and m.list_outputs() == ["output", "count_sum"]
    assert m.infer_shape([(256, 81, 28, 28), (2, 128), (256, 28, 28)]) == (
        [(256, 81, 28, 28), (2, 128), (256, 28, 28)], [(1,), (1,)])
    assert m.infer_shape([(256, 81, 28, 28), (), ()])[0] == [(256, 81, 28, 28), (256,), (256, 28, 28)]
    with pytest.raises(ValueError):
        m.infer_shape([(256, 81, 28, 28), (255,), (256, 28, 28)])
    assert m.declare_backward_dependency(["g"], ["l", "c", "t"], ["o", "cs"]) == ["l", "c", "t"]


def _head(builder, fp16, batch_image=2, num_fg=128, num_class=81):
    ns = types.SimpleNamespace
    head = builder.MaskFasterRcnnHead.__new__(builder.MaskFasterRcnnHead)
    head.pBbox = ns(batch_image=batch_image, num_class=num_class)
    head.pMask = ns(fp16=fp16, num_fg_roi=num_fg)
    head.pMaskRoi = None
    head._get_mask_head_logit = lambda conv_feat: conv_feat
    return head


def _loss_nodes(head, R):
    V = R.mx.sym.var
    loss, = head.get_loss(V("conv_feat"), V("mask_target"), V("mask_ind"))
    return RS.source(loss), collections.Counter(n.op_type for n in RS.walk(loss, {}).values())


@needs_ref
def test_get_loss_holds_one_fused_node_only_with_the_opt_in():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.maskrcnn.builder")
        reference_get_loss = builder.MaskFasterRcnnHead.get_loss
        # default install(): the reference's nodes, unchanged
        plug._state.update(registered=False)
        plug.install(R.mx)
        assert builder.MaskFasterRcnnHead.get_loss is reference_get_loss and not plug._state["mask_loss_patched"]
        node, native = _loss_nodes(_head(builder, False), R)
        assert node.op_type == "SigmoidCrossEntropy" and node.name == "mask_loss"
        assert native["gather_nd"] == 2 and native["stack"] == 2 and native["split"] == 2 and native["concat"] == 1
        assert native["sd_MaskLoss"] == 0
        # opt-in: exactly one sd_MaskLoss, none of the subgraph
        plug._state.update(registered=False)
        plug.install(R.mx, mask_loss=True)
        assert plug._state["mask_loss_patched"]
        assert builder.MaskFasterRcnnHead._sd_reference_get_loss is reference_get_loss
        plug.install(R.mx, mask_loss=True)        # a second install keeps the first original
        assert builder.MaskFasterRcnnHead._sd_reference_get_loss is reference_get_loss
        for fp16, scale in ((False, 1.0), (True, 128.0)):
            node, got = _loss_nodes(_head(builder, fp16), R)
            assert node.op_type == "sd_MaskLoss" and node.nout == 2 and node.name == "mask_loss"
            assert got["sd_MaskLoss"] == 1 and got["SigmoidCrossEntropy"] == 0
            assert got["sd__contrib_SigmoidCrossEntropy"] == 0
            assert all(got[o] == 0 for o in SUBGRAPH), dict(got)
            assert float(node.params["grad_scale"]) == scale and set(node.params) == {"grad_scale"}
            # logits (through get_output: the to_fp32 cast and the mask_fcn_logit conv), mask_ind, mask_target
            assert [RS.source(i).name for i in node.inputs] == ["mask_fcn_logit", "mask_ind", "mask_target"]
            assert got["Convolution"] == native["Convolution"] and got["Cast"] == native["Cast"]
        # the aliased operator, for graphs that are not patched (models/msrcnn/builder.py)
        V = R.mx.sym.var
        a = R.mx.sym.contrib.SigmoidCrossEntropy(V("a"), V("b"), grad_scale=1.0, name="mask_loss")
        assert RS.source(a).op_type == "sd__contrib_SigmoidCrossEntropy" and RS.source(a).nout == 5
        assert a.op_type == "_output" and a.index == 0
        ms = importlib.import_module("models.msrcnn.builder")
        assert "_sd_reference_get_loss" not in ms.MaskFasterRcnnHead.__dict__
        # a later default install() restores the original method
        plug._state.update(registered=False)
        plug.install(R.mx)
        assert builder.MaskFasterRcnnHead.get_loss is reference_get_loss and not plug._state["mask_loss_patched"]
        node, again = _loss_nodes(_head(builder, False), R)
        assert node.op_type == "SigmoidCrossEntropy" and again == native
        plug._state.update(registered=False)


@needs_ref
def test_mask_r50_train_symbol_holds_the_fused_node():
    def nodes(**kw):
        with RS.reference_modules() as R:
            from simpledet_amd import mxnet_plugin as plug
            cfg = importlib.import_module("config.mask_r50v1_fpn_1x")
            plug._state.update(registered=False)
            plug.install(R.mx, **kw)
            sym = None
            for o in cfg.get_config(True):
                s = getattr(o, "train_symbol", None)
                if isinstance(s, RS.Symbol):
                    sym = s
            out = collections.Counter(n.op_type for n in RS.walk(sym, {}).values())
            plug.install(R.mx)
            plug._state.update(registered=False)
            return out
    native, fused = nodes(), nodes(mask_loss=True)
    assert native["SigmoidCrossEntropy"] == 1 and native["gather_nd"] == 2 and native["sd_MaskLoss"] == 0
    assert fused["sd_MaskLoss"] == 1 and fused["SigmoidCrossEntropy"] == 0 and fused["gather_nd"] == 0
    rest = lambda c: {k: v for k, v in c.items() if k not in SUBGRAPH + ("SigmoidCrossEntropy", "sd_MaskLoss", "reshape", "_output")}
    assert rest(native) == rest(fused)


@pytest.mark.gpu
def test_adapter_round_trip_equals_the_ops_calls(plugin, ops):
    import torch
    from . import sigmoid_ce_ref as sr
    mx, props, _ = plugin
    # the aliased operator
    name, c = sr.dropin_cases()[7]
    p = props["_contrib_SigmoidCrossEntropy"](grad_scale="128.0")
    ishape, oshape = p.infer_shape([c["x"].shape, c["t"].shape])[:2]
    op = p.create_operator(None, ishape, None)
    ins = [mx_stub.wrap(torch.from_numpy(a).cuda()) for a in (c["x"], c["t"])]
    outs = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
    op.forward(True, ["write"] * 5, ins, outs, [])
    want = ops.sigmoid_cross_entropy_forward(ins[0].t, ins[1].t, full=True)
    for g, w in zip(outs, want):
        assert torch.equal(g.t.view(torch.int32), w.view(torch.int32))
    grads = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in ishape]
    outs[3].t.fill_(float("nan"))
    outs[4].t.fill_(float("nan"))
    op.backward(["write", "write"], [], ins, outs, grads, [])
    d, cs = ops.sigmoid_cross_entropy_backward(ins[0].t, ins[1].t, 128.0)
    assert torch.equal(grads[0].t.view(torch.int32), d.view(torch.int32)) and not grads[1].t.any()
    assert torch.equal(outs[3].t, want[3]) and torch.equal(outs[4].t, cs)      # the backward writes them again
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["add", "write"], [], ins, outs, grads, [])
    # the fused node
    name, f = sr.fused_cases()[1]
    m = props["MaskLoss"](grad_scale="128.0")
    shapes = [(8, 81, 28, 28), (2, 4), (8, 28, 28)]
    ishape, oshape = m.infer_shape(shapes)[:2]
    op = m.create_operator(None, ishape, None)
    ins = [mx_stub.wrap(torch.from_numpy(f[k]).cuda().view(s)) for k, s in zip(("logits", "cls", "target"), shapes)]
    outs = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
    op.forward(True, ["write"] * 2, ins, outs, [])
    want = ops.mask_loss_forward(ins[0].t, ins[1].t, ins[2].t)
    assert torch.equal(outs[0].t.view(torch.int32), want[0].view(torch.int32)) and torch.equal(outs[1].t, want[1])
    grads = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in ishape]
    op.backward(["write"] * 3, [], ins, outs, grads, [])
    d = ops.mask_loss_backward(ins[0].t, ins[1].t, ins[2].t, 128.0)
    assert torch.equal(grads[0].t.view(torch.int32), d.view(torch.int32))
    assert not grads[1].t.any() and not grads[2].t.any()
    assert np.array_equal(ins[0].t.cpu().numpy().reshape(8, 81, 784), f["logits"])
