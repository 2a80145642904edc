"""The `sd_BboxPostProcessing` CustomOp and its opt-in: `install(mx, bbox_post=True)` makes every Mask R-CNN
test symbol of the reference's configs hold an `sd_BboxPostProcessing` node where
models/maskrcnn/builder.py:69-84 (and its copy models/msrcnn/builder.py:174-189) emits
`Custom(op_type='BboxPostProcessing')`; the default install() leaves those graphs as they are.

The sweeps are CPU only and skipped where /root/reference is absent (the GPU box), like
tests/test_proposal_plugin_sweep.py; the GPU test drives the CustomOp through tests/mx_stub.py."""
import ast
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

# every config whose test symbol goes through a BboxPostProcessor
MASK_CONFIGS = [
    "config.mask_r50v1_fpn_1x", "config.ms_r50v1_fpn_1x",
    "config.resnet_v1b.mask_r50v1b_fpn_1x", "config.resnet_v1b.mask_r50v1b_fpn_2x",
    "config.resnet_v1b.mask_r101v1b_fpn_1x", "config.resnet_v1b.mask_r101v1b_fpn_2x",
    "config.resnet_v1b.mask_r152v1b_fpn_1x", "config.resnet_v1b.mask_r152v1b_fpn_2x",
    "config.resnet_v1b.ms_r50v1b_fpn_1x", "config.scratch.mask_r50v1b_fpn_gn_scratch_2x",
    "config.scratch.mask_r50v1b_fpn_bn_scratch_2x", "config.se.mask_se-r50v1b_fpn_bn_scratch_2x",
]
PARAMS = {"max_det_per_image", "min_det_score", "nms_type", "nms_thr"}


def _nodes(mod, **install_kw):
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin
        cfg = importlib.import_module(mod)
        mxnet_plugin._state.update(registered=False)
        props = mxnet_plugin.install(R.mx, **install_kw)
        per_symbol = {}
        for is_train in (True, False):
            for o in cfg.get_config(is_train):
                for a in ("train_symbol", "test_symbol", "rpn_test_symbol"):
                    s = getattr(o, a, None)
                    if isinstance(s, RS.Symbol):
                        per_symbol[(is_train, a)] = list(RS.walk(s, {}).values())
        fallbacks = list(mxnet_plugin._state["fallbacks"])
        mxnet_plugin._state.update(registered=False)
        return props, per_symbol, fallbacks


def _count(nodes):
    return collections.Counter(n.op_type for n in nodes)


@needs_ref
@pytest.mark.parametrize("mod", MASK_CONFIGS)
def test_mask_configs_take_the_device_op_only_with_the_opt_in(mod):
    props0, native, _ = _nodes(mod)
    assert "BboxPostProcessing" not in props0
    props, nodes, fallbacks = _nodes(mod, bbox_post=True)
    assert "BboxPostProcessing" in props and not [f for f in fallbacks if f[0] == "BboxPostProcessing"]
    held = 0
    for key, plain in native.items():
        want = _count(plain)["BboxPostProcessing"]
        got = _count(nodes[key])
        assert got["sd_BboxPostProcessing"] == want and got["BboxPostProcessing"] == 0, (key, dict(got))
        held += want
        # every other node is what the default install builds, node for node
        rest = lambda ns, skip: collections.Counter(n.op_type for n in ns if n.op_type != skip)
        assert rest(plain, "BboxPostProcessing") == rest(nodes[key], "sd_BboxPostProcessing"), key
        for n, ref in zip([n for n in nodes[key] if n.op_type == "sd_BboxPostProcessing"],
                          [n for n in plain if n.op_type == "BboxPostProcessing"]):
            assert set(n.params) == PARAMS and len(n.inputs) == 2
            assert {k: str(v) for k, v in ref.params.items()} == {k: str(v) for k, v in n.params.items()}
            assert n.nout == 3
    assert held >= 1   # the test symbol holds one
    assert _count(native[(False, "test_symbol")])["BboxPostProcessing"] == 1
    # a second default install() puts the reference's node back
    _, again, _ = _nodes(mod)
    assert {k: _count(v) for k, v in again.items()} == {k: _count(v) for k, v in native.items()}


@needs_ref
def test_mask_r50_parameters_reach_the_node():
    """config/mask_r50v1_fpn_1x.py:161-174: min_det_score 0.05, max_det_per_image 100, nms 'nms' 0.5"""
    _, nodes, _ = _nodes("config.mask_r50v1_fpn_1x", bbox_post=True)
    n, = [n for n in nodes[(False, "test_symbol")] if n.op_type == "sd_BboxPostProcessing"]
    assert {k: str(v) for k, v in n.params.items()} == {"max_det_per_image": "100", "min_det_score": "0.05",
                                                        "nms_type": "nms", "nms_thr": "0.5"}
    # its box output feeds the mask head's RoI extractor
    users = [m for m in nodes[(False, "test_symbol")]
             if any(RS.source(i) is n and i.op_type == "_output" and i.index == 1 for i in m.inputs)]
    assert any(m.op_type == "sd_fpn_roi_align" for m in users), [m.op_type for m in users]


@needs_ref
def test_a_non_nms_type_falls_back_and_is_recorded():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.maskrcnn.builder")
        plug._state.update(registered=False)
        plug.install(R.mx, bbox_post=True)
        assert plug._state["bbox_post_patched"]
        original = builder.BboxPostProcessor._sd_reference_get_post_processing
        plug.install(R.mx, bbox_post=True)      # a second install keeps the first original
        assert builder.BboxPostProcessor._sd_reference_get_post_processing is original
        V = R.mx.sym.var
        ns = types.SimpleNamespace

        def build(nms_type, max_det=100):
            p = ns(max_det_per_image=max_det, min_det_score=0.05, nms=ns(type=nms_type, thr=0.5))
            pp = builder.BboxPostProcessor.__new__(builder.BboxPostProcessor)
            pp.p = p
            return RS.source(pp.get_post_processing(V("s"), V("b"))[0])
        assert build("nms").op_type == "sd_BboxPostProcessing" and not plug._state["fallbacks"]
        node = build("softnms")
        assert node.op_type == "BboxPostProcessing" and node.params["nms_type"] == "softnms"
        assert plug._state["fallbacks"][-1][0] == "BboxPostProcessing" and "softnms" in plug._state["fallbacks"][-1][2]
        assert build("nms", max_det=5000).op_type == "BboxPostProcessing"     # outside the kernels' limits
        assert "5000" in plug._state["fallbacks"][-1][2]
        plug._state.update(registered=False)


def _reference_prop():
    """BboxPostProcessingProp of the reference, loaded by name (no mxnet, no Cython import)"""
    path = os.path.join(REF, "models", "maskrcnn", "bbox_post_processing.py")
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "BboxPostProcessingProp"]
    assert len(body) == 1
    body[0].decorator_list = []
    env = {"mx": types.SimpleNamespace(operator=types.SimpleNamespace(CustomOpProp=RS.CustomOpProp))}
    exec(compile(ast.Module(body=body, type_ignores=[]), path, "exec"), env)
    return env["BboxPostProcessingProp"]


@pytest.fixture()
def plugin():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, bbox_post=True)
    yield mx, props
    mxnet_plugin._state.update(registered=False)


def test_default_install_does_not_register_it():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx)
    assert "BboxPostProcessing" not in props and "sd_BboxPostProcessing" not in mx.registry
    assert mxnet_plugin._state["bbox_post_patched"] is False
    mxnet_plugin._state.update(registered=False)


def test_prop_parses_strings_and_infers_shapes(plugin):
    mx, props = plugin
    assert "sd_BboxPostProcessing" in mx.registry
    P = props["BboxPostProcessing"]
    p = P(max_det_per_image="100", min_det_score="0.05", nms_type="nms", nms_thr="0.5")
    assert p.g == dict(max_det=100, min_score=0.05, nms_type="nms", thr=0.5)
    assert p.need_top_grad_ is False
    assert p.list_arguments() == ["cls_score", "bbox_xyxy"]
    assert p.list_outputs() == ["post_score", "post_bbox_xyxy", "post_cls"]
    ins, outs = p.infer_shape([(2, 1000, 81), (2, 1000, 324)])
    assert ins == [(2, 1000, 81), (2, 1000, 324)] and outs == [(2, 100, 1), (2, 100, 4), (2, 100, 1)]
    assert p.infer_shape([(2, 1000, 81), (2, 1000, 4)])[1] == outs
    assert p.declare_backward_dependency(["a", "b", "c"], ["s", "b"], ["x", "y", "z"]) == []
    with pytest.raises(NotImplementedError):     # the reference's forward raises for anything but 'nms'
        P(max_det_per_image="100", min_det_score="0.05", nms_type="softnms", nms_thr="0.5")
    for bad in ([(1, 5000, 81), (1, 5000, 4)], [(1, 10, 300), (1, 10, 4)], [(1, 10, 5), (1, 10, 8)]):
        with pytest.raises(ValueError):
            p.infer_shape(bad)


@needs_ref
@pytest.mark.parametrize("shapes", [[(2, 1000, 81), (2, 1000, 324)], [(1, 300, 21), (1, 300, 4)]])
def test_interface_equals_the_reference_registration(plugin, shapes):
    _, props = plugin
    kw = dict(max_det_per_image="100", min_det_score="0.05", nms_type="nms", nms_thr="0.5")
    ours, ref = props["BboxPostProcessing"](**kw), _reference_prop()(**kw)
    assert ours.list_arguments() == ref.list_arguments()
    assert ours.list_outputs() == ref.list_outputs()
    assert ours.need_top_grad_ == ref.need_top_grad_ is False
    o_in, o_out = ours.infer_shape([tuple(s) for s in shapes])
    r_in, r_out = ref.infer_shape([tuple(s) for s in shapes])
    assert [tuple(s) for s in o_in] == [tuple(s) for s in r_in]
    assert [tuple(s) for s in o_out] == [tuple(s) for s in r_out]
    assert ours.declare_backward_dependency([], [], []) == ref.declare_backward_dependency([], [], [])
    assert (ours.g["max_det"], ours.g["min_score"], ours.g["nms_type"], ours.g["thr"]) == \
        (ref.max_det_per_image, ref.min_det_score, ref.nms_type, ref.nms_thr)


@pytest.mark.gpu
def test_custom_op_forward_and_backward(plugin, ops):
    import torch
    from . import bbox_post_cases as cases
    mx, props = plugin
    score, bbox, par = cases.case("shared")
    ts, tb = torch.from_numpy(score).cuda(), torch.from_numpy(bbox).cuda()
    prop = props["BboxPostProcessing"](max_det_per_image=str(par["max_det_per_image"]),
                                       min_det_score=str(par["min_det_score"]), nms_type="nms",
                                       nms_thr=str(par["nms_thr"]))
    _, out_shapes = prop.infer_shape([tuple(ts.shape), tuple(tb.shape)])
    op = prop.create_operator(None, None, None)
    outs = [mx_stub.wrap(torch.full(s, 7.0, device="cuda")) for s in out_shapes]
    op.forward(False, ["write"] * 3, [mx_stub.wrap(ts), mx_stub.wrap(tb)], outs, [])
    want = ops.bbox_post_processing(ts, tb, **par)
    for g, w in zip(outs, want):
        assert g.t.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
    grads = [mx_stub.wrap(torch.full_like(ts, 3.0)), mx_stub.wrap(torch.full_like(tb, 3.0))]
    op.backward(["write", "write"], [], [mx_stub.wrap(ts), mx_stub.wrap(tb)], outs, grads, [])
    assert not grads[0].t.any() and not grads[1].t.any()
    assert np.array_equal(ts.cpu().numpy(), score)
