"""`install(mx, reppoints_decode=True)`: the test symbol of config/RepPoints/reppoints_moment_r50v1_fpn_1x.py holds ONE
`sd_reppoints_decode` node in place of, per level, the transposes, sigmoid, max and topk and, per image, the slice /
take / scale / add / clip chains of RepPointsHead.get_prediction (models/RepPoints/builder.py:486-576).  Without the
flag -- `reppoints=True` included -- the graph holds what it held.  CPU only on tests/mx_stub.py and tests/ref_stubs.py
(the builder tests are skipped where the reference tree is absent, like tests/test_fcos_decode_plugin.py); the GPU
round trip through the adapter is the last test."""
import collections
import importlib
import os

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
CONFIG = "config.RepPoints.reppoints_moment_r50v1_fpn_1x"
REFERENCE_ONLY = ("topk", "take", "X.sigmoid", "sigmoid", "max", "stack", "broadcast_minimum", "maximum", "zeros_like")
MAPS = [(100, 167), (50, 84), (25, 42), (13, 21), (7, 11)]        # 800 x 1333 at strides 8..128


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def plugin():
    mx, props, mxnet_plugin = _fresh(reppoints_decode=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_and_other_installs_register_nothing_new():
    from simpledet_amd.mxnet_plugin import FEATURE_FLAGS
    for flags in ({}, dict(reppoints=True), {f: True for f in FEATURE_FLAGS if f != "reppoints_decode"}):
        mx, props, mxnet_plugin = _fresh(**flags)
        try:
            assert "reppoints_decode" not in props and "sd_reppoints_decode" not in mx.registry
            assert mxnet_plugin._state["reppoints_decode_patched"] is False
        finally:
            mxnet_plugin._state.update(registered=False)


def _level_shapes(n, c, k2, maps=MAPS):
    return [(n, c) + m for m in maps] + [(n, k2) + m for m in maps]


def test_prop_shapes_types_and_arguments(plugin):
    mx, props, plug = plugin
    assert "sd_reppoints_decode" in mx.registry and "sd_reppoints_target" not in mx.registry
    P = props["reppoints_decode"](stride="(8, 16, 32, 64, 128)", pre_nms_top_n="1000", transform="moment", num_points="9")
    assert P.g == dict(stride=(8, 16, 32, 64, 128), pre_nms_top_n=1000, transform="moment", num_points=9, input_logits=True)
    assert P.list_arguments() == (["cls_logit_%d" % i for i in range(5)] + ["pts_refine_%d" % i for i in range(5)]
                                  + ["im_info", "moment_transfer"])
    assert P.list_outputs() == ["cls_score", "bbox_xyxy"] and P.need_top_grad_ is False
    # the config at 800 x 1333: 3 x 1000 rows and every location of the two coarse levels, 273 + 77
    ins, outs = P.infer_shape(_level_shapes(1, 80, 18) + [(), ()])[:2]
    assert ins[10:] == [(1, 3), (2,)] and outs == [(1, 3350, 81), (1, 3350, 4)]
    assert P.infer_shape(_level_shapes(2, 80, 18) + [(2, 3), (2,)])[1] == [(2, 3350, 81), (2, 3350, 4)]
    assert P.infer_type([np.float32] * 12) == ([np.float32] * 12, [np.float32] * 2, [])
    assert P.declare_backward_dependency([], list("abcdefghijkl"), list("xy")) == []
    Q = props["reppoints_decode"](stride="(8, 64)", pre_nms_top_n="-1", transform="minmax", num_points="4", input_logits="0")
    assert Q.g["input_logits"] is False
    assert Q.infer_shape([(2, 3, 5, 7), (2, 3, 2, 3), (2, 8, 5, 7), (2, 8, 2, 3), (2, 3), (2,)])[1] == [(2, 41, 4), (2, 41, 4)]
    # a level with stride <= 32 and fewer locations than pre_nms_top_n: the reference's own note
    maps = [(13, 21), (7, 11), (4, 6), (2, 3), (1, 2)]
    with pytest.raises(ValueError, match="fewer than pre_nms_top_n = 1000.*builder.py:499-501.*low-resolution images") as e:
        P.infer_shape(_level_shapes(1, 80, 18, maps) + [(), ()])
    assert "stride-8 level holds 273 locations" in str(e.value)
    for bad in (_level_shapes(1, 80, 18)[:9] + [(1, 16, 7, 11), (), ()],          # a point map of another num_points
                _level_shapes(1, 80, 18)[:9] + [(1, 18, 7, 12), (), ()],          # ... of another size
                _level_shapes(1, 80, 18) + [(2, 3), ()], _level_shapes(1, 80, 18) + [(), (3,)],
                _level_shapes(1, 80, 18) + [()]):
        with pytest.raises(ValueError):
            P.infer_shape(bad)
    for kw in (dict(stride=str(tuple(range(1, 10))), pre_nms_top_n="5"), dict(stride="(8,)", pre_nms_top_n="5", transform="median"),
               dict(stride="(8,)", pre_nms_top_n="5", num_points="0"), dict(stride="(0,)", pre_nms_top_n="5"),
               dict(stride="(8,)", pre_nms_top_n="5", transform="partial_minmax", num_points="3")):
        with pytest.raises(ValueError):
            props["reppoints_decode"](**kw)
    with pytest.raises(ValueError, match="limit is 16384"):
        props["reppoints_decode"](stride="(8,)", pre_nms_top_n="-1").infer_shape([(1, 2, 129, 128), (1, 18, 129, 128), (), ()])
    # the builder module is absent here: nothing is rebound and the fallback list says so
    if not os.path.isdir(REF):
        assert plug._state["reppoints_decode_patched"] is False
        assert [f[0] for f in plug._state["fallbacks"]] == ["reppoints_decode"]


def _symbols(R, **flags):
    from simpledet_amd import mxnet_plugin as plug
    plug._state.update(registered=False)
    plug.install(R.mx, **flags)
    cfg = importlib.import_module(CONFIG)
    train = test = None
    for is_train in (True, False):
        for o in cfg.get_config(is_train):
            s = getattr(o, "train_symbol" if is_train else "test_symbol", None)
            if isinstance(s, RS.Symbol):
                if is_train:
                    train = s
                else:
                    test = s
    assert train is not None and test is not None
    return train, test


def _ops(sym):
    return collections.Counter(n.op_type for n in RS.walk(sym, {}).values())


def _shape_of(sym):
    return [(n.op_type, n.name, sorted((k, repr(v)) for k, v in n.params.items()), [i.op_type for i in n.inputs])
            for n in RS.walk(sym, {}).values()]


def _find(sym, op_type):
    return [n for n in RS.walk(sym, {}).values() if n.op_type == op_type]


@needs_ref
def test_reppoints_test_symbol_holds_the_one_device_node():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.RepPoints.builder")
        reference = builder.RepPointsHead.get_prediction
        native_train, native_test = _symbols(R)
        assert builder.RepPointsHead.get_prediction is reference and not plug._state["reppoints_decode_patched"]
        native = _ops(native_test)
        assert native["topk"] == 5 and native["take"] == 15 and native["sd_reppoints_decode"] == 0, dict(native)

        # reppoints=True alone: the train head only, get_prediction untouched
        _, only_train_flag = _symbols(R, reppoints=True)
        assert builder.RepPointsHead.get_prediction is reference
        assert _shape_of(only_train_flag) == _shape_of(native_test)

        train, test = _symbols(R, reppoints_decode=True)
        assert plug._state["reppoints_decode_patched"] and not plug._state["reppoints_patched"]
        assert builder.RepPointsHead._sd_reference_get_prediction is reference
        assert not any(f[0] == "reppoints_decode" for f in plug._state["fallbacks"])
        plug.install(R.mx, reppoints_decode=True)     # a second install keeps the first original
        assert builder.RepPointsHead._sd_reference_get_prediction is reference
        got = _ops(test)
        assert got["sd_reppoints_decode"] == 1 and got["topk"] == 0 and got["take"] == 0, dict(got)
        assert all(got[o] == 0 or got[o] < native[o] for o in REFERENCE_ONLY), {o: (got[o], native[o]) for o in REFERENCE_ONLY}
        assert sum(got.values()) < sum(native.values()) - 100     # well over a hundred nodes at batch_image = 1
        node, = _find(test, "sd_reppoints_decode")
        assert node.nout == 2
        assert node.params == {"stride": "(8, 16, 32, 64, 128)", "pre_nms_top_n": "1000", "transform": "moment",
                               "num_points": "9", "input_logits": "1"}
        # its inputs: 5 class logit maps and 5 refine point maps straight from the head's convolutions, im_info,
        # moment_transfer
        ins = [RS.source(i) for i in node.inputs]
        assert len(ins) == 12 and [n.name for n in ins[10:]] == ["im_info", "moment_transfer"]
        assert all(n.name == "cls_out" for n in ins[:5]), [n.name for n in ins[:5]]
        for n in ins[5:10]:                           # pts_refine_out + BlockGrad(pts_init_out) (builder.py:262)
            assert RS.source(n.inputs[0]).name == "pts_refine_out", (n.op_type, [RS.source(i).name for i in n.inputs])
        # the two things the head hands on are outputs 0 (cls_score) and 1 (bbox_xyxy) of that node, in this order
        heads = test.inputs if test.op_type == "Group" else list(test)
        assert len(heads) == 5 and [RS.source(h) is node for h in heads] == [False, False, False, True, True]
        assert [h.index for h in heads[3:]] == [0, 1]
        # output shapes at 800 x 1333, the config's test batch of one image
        P = plug._state["table"]["reppoints_decode"][0](**node.params)
        assert P.infer_shape(_level_shapes(1, 80, 18) + [(1, 3), (2,)])[1] == [(1, 3350, 81), (1, 3350, 4)]
        # everything in front of the head is untouched, and so is the train symbol
        assert got["Convolution"] == native["Convolution"]
        assert _shape_of(train) == _shape_of(native_train)

        # both flags together
        train2, test2 = _symbols(R, reppoints=True, reppoints_decode=True)
        assert _ops(train2)["sd_reppoints_box_loss"] == 1 and _ops(test2)["sd_reppoints_decode"] == 1

        # a default install() afterwards: the graphs are node for node the native ones
        again_train, again_test = _symbols(R)
        assert builder.RepPointsHead.get_prediction is reference and not plug._state["reppoints_decode_patched"]
        assert _shape_of(again_test) == _shape_of(native_test) and _shape_of(again_train) == _shape_of(native_train)
        # unpatch by hand restores as well
        plug.patch_reppoints_decode(builder, R.mx)
        assert builder.RepPointsHead.get_prediction is not reference
        assert plug.unpatch_reppoints_decode(builder) and builder.RepPointsHead.get_prediction is reference
        plug._state.update(registered=False)


@needs_ref
def test_fp16_falls_back_to_the_reference():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.RepPoints.builder")
        _, native_test = _symbols(R)
        plug._state.update(registered=False)
        plug.install(R.mx, reppoints_decode=True)
        hp = [o for o in importlib.import_module(CONFIG).get_config(False) if hasattr(o, "point_generate")][0]
        v = R.mx.sym.var
        old = hp.fp16
        hp.fp16 = True
        try:
            plug._state["fallbacks"] = []
            head = builder.RepPointsHead(hp)
            feat = {"stride%s" % s: v("f%s" % s) for s in hp.point_generate.stride}
            ops = _ops(R.mx.sym.Group(list(head.get_prediction(feat, v("im_info")))))
            fb = [f for f in plug._state["fallbacks"] if f[0] == "reppoints_decode"]
            assert ops["sd_reppoints_decode"] == 0 and ops["topk"] == 5 and len(fb) == 1 and "fp16" in fb[0][2]
        finally:
            hp.fp16 = old
        plug.install(R.mx)
        assert _shape_of(_symbols(R)[1]) == _shape_of(native_test)
        plug._state.update(registered=False)


@pytest.mark.gpu
def test_adapter_forward_equals_the_ops_call(plugin, ops):
    import torch
    from . import reppoints_decode_ref as dr
    mx, props, _ = plugin
    c = dr.logits_case(dict(dr.cases())["five_levels"], 3)
    tensors = [torch.from_numpy(a).cuda() for a in c["cls"] + c["pts"] + [c["im_info"], c["mt"]]]
    L = len(c["cls"])
    P = props["reppoints_decode"](stride=str(tuple(c["strides"])), pre_nms_top_n=str(c["top_n"]), transform=c["transform"],
                                  num_points=str(c["num_points"]))
    ishape, oshape = P.infer_shape([tuple(t.shape) for t in tensors])[:2]
    op = P.create_operator(None, ishape, None)
    ins = [mx_stub.wrap(t) for t in tensors]
    outs = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
    op.forward(False, ["write"] * 2, ins, outs, [])
    want = ops.reppoints_decode(tensors[:L], tensors[L:2 * L], tensors[2 * L], c["strides"], c["ks"],
                                transform=c["transform"], moment_transfer=tensors[2 * L + 1], input_logits=True)
    for g, w in zip(outs, want):
        assert g.t.shape == w.shape and torch.equal(g.t.view(torch.int32), w.view(torch.int32))
    grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7.0, device="cuda")) for t in tensors]
    op.backward(["write"] * len(tensors), [], ins, outs, grads, [])
    assert all(not g.t.any() for g in grads)
    with pytest.raises(RuntimeError, match="kAddTo"):
        op.forward(False, ["add", "write"], ins, outs, [])
