"""`install(mx, reppoints=True)`: the train symbol of every config under config/RepPoints/ holds ONE
`sd_reppoints_target` and ONE `sd_reppoints_box_loss` node in place of _gen_points, _offset_to_boxes, both _point_target
subgraphs, _offset_to_pts, _points2bbox, smooth_l1, BBoxNorm and MakeLoss (models/RepPoints/builder.py:311-484), and
the focal loss node it held.  Without the flag the graph holds what it held.  CPU only on tests/mx_stub.py and
tests/ref_stubs.py (the builder tests are skipped where the reference tree is absent, like tests/test_fcos_plugin.py);
the GPU round trip through the adapter is the last test."""
import collections
import importlib
import os

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
CONFIGS = ("reppoints_minmax_r50v1_fpn_1x", "reppoints_moment_r50v1_fpn_1x", "reppoints_moment_r101v1_fpn_2x",
           "reppoints_moment_dcn_r101v1b_fpn_multiscale_2x", "reppoints_moment_dcnv2_r101v1b_fpn_multiscale_2x")
REFERENCE_ONLY = ("topk", "box_iou", "argmax", "take", "norm", "log2", "smooth_l1", "X.smooth_l1", "X.bbox_norm",
                  "X.make_loss", "flip")


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def plugin():
    mx, props, mxnet_plugin = _fresh(reppoints=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_nothing_new():
    mx, props, mxnet_plugin = _fresh()
    try:
        assert "reppoints_target" not in props and "reppoints_box_loss" not in props
        assert "sd_reppoints_target" not in mx.registry and "sd_reppoints_box_loss" not in mx.registry
        assert mxnet_plugin._state["reppoints_patched"] is False
        mx2, props2, _ = _fresh(**{f: True for f in mxnet_plugin.FEATURE_FLAGS if f != "reppoints"})
        assert "reppoints_target" not in props2 and "sd_reppoints_box_loss" not in mx2.registry
    finally:
        mxnet_plugin._state.update(registered=False)


def test_props_shapes_types_and_arguments(plugin):
    mx, props, _ = plugin
    assert "sd_reppoints_target" in mx.registry and "sd_reppoints_box_loss" in mx.registry
    T = props["reppoints_target"](stride="(8, 16, 32, 64, 128)", num_points="9", transform="moment", target_scale="4",
                                  num_pos="1", pos_iou_thr="0.5", neg_iou_thr="0.5", min_pos_iou="0.0")
    assert T.g == dict(stride=(8, 16, 32, 64, 128), num_points=9, transform="moment", target_scale=4.0, num_pos=1,
                       pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0)
    assert T.list_arguments() == ["pts_init_%d" % i for i in range(5)] + ["gt_bbox", "moment_transfer"]
    assert T.list_outputs() == ["label_init", "gt_init", "label_refine", "gt_refine", "state"] and T.need_top_grad_ is False
    # 800 x 1333 at strides 8..128: P = 22300, the reference's concat
    maps = [(2, 18, 100, 167), (2, 18, 50, 84), (2, 18, 25, 42), (2, 18, 13, 21), (2, 18, 7, 11)]
    ins, outs = T.infer_shape(maps + [(2, 100, 5), ()])[:2]
    assert ins[5:] == [(2, 100, 5), (2,)]
    assert outs == [(2, 22300), (2, 22300, 4), (2, 22300), (2, 22300, 4), (4,)]
    assert T.infer_type([np.float32] * 7)[1] == [np.float32] * 4 + [np.int32]
    assert T.declare_backward_dependency([], list("abcdefg"), list("abcde")) == []
    for bad in (maps[:4] + [(2, 16, 7, 11), (2, 100, 5), ()], maps + [(2, 100, 4), ()], maps + [(2, 129, 5), ()],
                maps + [(3, 100, 5), ()], maps + [(2, 100, 5)]):
        with pytest.raises(ValueError):
            T.infer_shape(bad)
    for kw in (dict(stride="(8,)", num_points="4"), dict(stride="(8,)", transform="median"), dict(stride="(8,)", num_pos="17"),
               dict(stride=str(tuple(range(1, 10))))):
        with pytest.raises(ValueError):
            props["reppoints_target"](**kw)
    Lp = props["reppoints_box_loss"](stride="(8, 16)", num_points="9", transform="minmax", scale="4")
    assert Lp.g == dict(stride=(8, 16), num_points=9, transform="minmax", scale=4.0, grad_scale_init=0.5, grad_scale_refine=1.0)
    assert Lp.list_arguments() == ["pts_init_0", "pts_init_1", "pts_refine_0", "pts_refine_1", "moment_transfer",
                                   "label_init", "gt_init", "label_refine", "gt_refine", "state"]
    assert Lp.list_outputs() == ["pts_init_loss", "pts_refine_loss"] and Lp.need_top_grad_ is False
    shapes = [(2, 18, 8, 12), (2, 18, 4, 6)] * 2 + [()] * 6
    ins, outs = Lp.infer_shape(shapes)[:2]
    assert ins[4:] == [(2,), (2, 120), (2, 120, 4), (2, 120), (2, 120, 4), (4,)] and outs == [(2, 120, 4)] * 2
    assert Lp.infer_type([np.float32] * 10)[0][-1] == np.int32
    with pytest.raises(ValueError):
        Lp.infer_shape([(2, 18, 8, 12), (2, 18, 4, 6), (2, 18, 8, 12), (2, 18, 4, 7)] + [()] * 6)
    with pytest.raises(ValueError):
        Lp.infer_shape(shapes[:5] + [(2, 121)] + [()] * 4)


def _train_symbol(R, mod, **flags):
    from simpledet_amd import mxnet_plugin as plug
    plug._state.update(registered=False)
    plug.install(R.mx, **flags)
    cfg = importlib.import_module(mod)
    for o in cfg.get_config(True):
        s = getattr(o, "train_symbol", None)
        if isinstance(s, RS.Symbol):
            return s
    raise AssertionError("no train symbol in %s" % mod)


def _ops(sym):
    return collections.Counter(n.op_type for n in RS.walk(sym, {}).values())


def _shape_of(sym):
    return [(n.op_type, n.name, sorted((k, repr(v)) for k, v in n.params.items()), [i.op_type for i in n.inputs])
            for n in RS.walk(sym, {}).values()]


@needs_ref
@pytest.mark.parametrize("config", CONFIGS)
def test_reppoints_train_symbol_holds_the_two_device_nodes(config):
    mod = "config.RepPoints." + config
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.RepPoints.builder")
        reference_get_loss = builder.RepPointsHead.get_loss
        native = _train_symbol(R, mod)
        assert builder.RepPointsHead.get_loss is reference_get_loss and not plug._state["reppoints_patched"]
        nat = _ops(native)
        assert nat["sd_reppoints_target"] == 0 and nat["topk"] >= 3 and nat["box_iou"] >= 1 and nat["X.focal_loss"] == 1

        train = _train_symbol(R, mod, reppoints=True)
        assert plug._state["reppoints_patched"] and builder.RepPointsHead._sd_reference_get_loss is reference_get_loss
        plug.install(R.mx, reppoints=True)            # a second install keeps the first original
        assert builder.RepPointsHead._sd_reference_get_loss is reference_get_loss
        assert not [f for f in plug._state["fallbacks"] if f[0] == "reppoints_box_loss"]
        got = _ops(train)
        assert got["sd_reppoints_target"] == 1 and got["sd_reppoints_box_loss"] == 1 and got["X.focal_loss"] == 1, dict(got)
        assert all(got[o] == 0 for o in REFERENCE_ONLY), {o: got[o] for o in REFERENCE_ONLY}
        # five outputs in the reference's order
        heads = train.inputs if train.op_type == "Group" else list(train)
        assert len(heads) == 5
        src = [RS.source(h) for h in heads]
        assert src[0].op_type == "X.focal_loss" and src[0].name == "cls_loss"
        loss = src[1]
        assert loss is src[2] and loss.op_type == "sd_reppoints_box_loss" and [heads[1].index, heads[2].index] == [0, 1]
        assert [s.name for s in src[3:]] == ["points_init_labels", "point_refine_labels"]
        target = RS.source(src[3].inputs[0])
        assert target.op_type == "sd_reppoints_target" and target.nout == 5 and src[3].inputs[0].index == 2
        assert RS.source(src[4].inputs[0]) is target and src[4].inputs[0].index == 2
        # the parameters are the head's
        hp = [o for o in importlib.import_module(mod).get_config(True) if hasattr(o, "point_generate")][0]
        transform = hp.point_generate.transform
        assert target.params == {"stride": "(8, 16, 32, 64, 128)", "num_points": "9", "transform": transform,
                                 "target_scale": "4", "num_pos": "1", "pos_iou_thr": "0.5", "neg_iou_thr": "0.5",
                                 "min_pos_iou": "0.0"}
        assert loss.params == {"stride": "(8, 16, 32, 64, 128)", "num_points": "9", "transform": transform, "scale": "4",
                               "grad_scale_init": "0.5", "grad_scale_refine": "1.0"}
        # inputs: 5 init maps behind BlockGrad, gt_bbox, moment_transfer -> targets; 5 + 5 maps, moment_transfer, 5 targets
        tin = [RS.source(i) for i in target.inputs]
        assert len(tin) == 7 and [n.name for n in tin[5:]] == ["gt_bbox", "moment_transfer"]
        lin = [RS.source(i) for i in loss.inputs]
        assert len(lin) == 16 and lin[10].name == "moment_transfer" and all(n is target for n in lin[11:])
        assert [i.index for i in loss.inputs[11:]] == [0, 1, 2, 3, 4]
        assert [RS.source(n.inputs[0]) for n in tin[:5]] == lin[:5]            # the same init maps, gradient blocked
        assert all(n.name == "pts_init_out" for n in lin[:5])
        # the focal loss reads the concat of the class logits and label_refine
        fl = src[0]
        assert RS.source(fl.inputs[0]).name == "cls_concat" and RS.source(fl.inputs[1]) is target and fl.inputs[1].index == 2
        # the shapes of the five outputs are the reference's: (N, P) labels behind the (N, P, 4) losses
        T = plug._state["table"]["reppoints_target"][0](**target.params)
        maps = [(2, 18, 100, 167), (2, 18, 50, 84), (2, 18, 25, 42), (2, 18, 13, 21), (2, 18, 7, 11)]
        touts = T.infer_shape(maps + [(2, 100, 5), (2,)])[1]
        Lp = plug._state["table"]["reppoints_box_loss"][0](**loss.params)
        louts = Lp.infer_shape(maps * 2 + [(2,)] + touts)[1]
        assert louts == [(2, 22300, 4)] * 2 and touts[2] == (2, 22300)
        # everything in front of the head is untouched
        assert got["Convolution"] == nat["Convolution"] and got["sd__contrib_DeformableConvolution"] == nat["sd__contrib_DeformableConvolution"]

        # a default install() afterwards: the graph is node for node the native one
        again = _train_symbol(R, mod)
        assert builder.RepPointsHead.get_loss is reference_get_loss and not plug._state["reppoints_patched"]
        assert _shape_of(again) == _shape_of(native)
        # unpatch by hand restores as well
        plug.patch_reppoints_loss(builder, R.mx)
        assert builder.RepPointsHead.get_loss is not reference_get_loss
        assert plug.unpatch_reppoints_loss(builder) and builder.RepPointsHead.get_loss is reference_get_loss
        plug._state.update(registered=False)


@needs_ref
def test_fp16_and_limits_fall_back_to_the_reference():
    mod = "config.RepPoints.reppoints_moment_r50v1_fpn_1x"
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        builder = importlib.import_module("models.RepPoints.builder")
        native = _train_symbol(R, mod)
        plug._state.update(registered=False)
        plug.install(R.mx, reppoints=True)
        cfg = importlib.import_module(mod)
        hp = [o for o in cfg.get_config(True) if hasattr(o, "point_generate")][0]
        v = R.mx.sym.var
        for attr, owner, value, why in (("fp16", hp, True, "fp16"), ("num_pos", hp.point_target, 17, "num_pos=17"),
                                        ("num_points", hp.point_generate, 9, "")):
            old = getattr(owner, attr)
            setattr(owner, attr, value)
            try:
                plug._state["fallbacks"] = []
                head = builder.RepPointsHead(hp)
                feat = {"stride%s" % s: v("f%s" % s) for s in hp.point_generate.stride}
                out = head.get_loss(feat, v("gt_bbox"))
                ops = _ops(R.mx.sym.Group(list(out)))
                fb = [f for f in plug._state["fallbacks"] if f[0] == "reppoints_box_loss"]
                if why:
                    assert ops["sd_reppoints_target"] == 0 and ops["topk"] >= 3 and len(fb) == 1 and why in fb[0][2]
                else:
                    assert ops["sd_reppoints_target"] == 1 and not fb
            finally:
                setattr(owner, attr, old)
        plug.install(R.mx)
        assert _shape_of(_train_symbol(R, mod)) == _shape_of(native)
        plug._state.update(registered=False)


@pytest.mark.gpu
def test_adapter_round_trip_equals_the_ops_calls():
    """targets -> box loss -> focal loss through the plugin's CustomOps equals the direct calls bit for bit"""
    import torch
    from simpledet_amd import ops
    from . import reppoints_ref as rr
    mx, props, plug = _fresh(reppoints=True, retina_loss=True)
    try:
        name, c = rr.loss_cases()[0]
        L = len(c["strides"])
        geometry = dict(stride=str(c["strides"]), num_points=str(c["num_points"]), transform=c["transform"])
        T = props["reppoints_target"](target_scale=str(c["target_scale"]), num_pos=str(c["num_pos"]),
                                      pos_iou_thr=str(c["pos_iou_thr"]), neg_iou_thr=str(c["neg_iou_thr"]),
                                      min_pos_iou=str(c["min_pos_iou"]), **geometry)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        pi, pr = [dev(p) for p in c["pts_init"]], [dev(p) for p in c["pts_refine"]]
        gt, mt = dev(c["gt_bbox"]), dev(c["mt"])
        tens = pi + [gt, mt]
        ishape, oshape = T.infer_shape([tuple(t.shape) for t in tens])[:2]
        dt = T.infer_type([np.float32] * len(tens))[1]
        op = T.create_operator(None, ishape, None)
        outs = [mx_stub.wrap(torch.zeros(s, device="cuda", dtype=torch.int32 if d is np.int32 else torch.float32))
                for s, d in zip(oshape, dt)]
        op.forward(True, ["write"] * 5, [mx_stub.wrap(t) for t in tens], outs, [])
        kw_t = dict(transform=c["transform"], target_scale=c["target_scale"], num_pos=c["num_pos"],
                    pos_iou_thr=c["pos_iou_thr"], neg_iou_thr=c["neg_iou_thr"], min_pos_iou=c["min_pos_iou"])
        want = ops.reppoints_target(pi, gt, c["strides"], moment_transfer=mt, **kw_t)
        bits = lambda t: t.contiguous().view(torch.int32)
        for g, w in zip(outs, want):
            assert g.t.shape == w.shape and torch.equal(bits(g.t), bits(w))
        assert int(want.state[1]) > 0
        Lp = props["reppoints_box_loss"](scale=str(c["scale"]), **geometry)
        tens = pi + pr + [mt] + [o.t for o in outs]
        ishape, oshape = Lp.infer_shape([tuple(t.shape) for t in tens])[:2]
        op = Lp.create_operator(None, ishape, None)
        ins = [mx_stub.wrap(t) for t in tens]
        louts = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
        op.forward(True, ["write"] * 2, ins, louts, [])
        kw_l = dict(transform=c["transform"], scale=c["scale"], moment_transfer=mt)
        wl = ops.reppoints_box_loss_forward(pi, pr, want, c["strides"], **kw_l)
        for g, w in zip(louts, wl):
            assert torch.equal(bits(g.t), bits(w))
        grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7, device="cuda", dtype=t.dtype)) for t in tens]
        op.backward(["write"] * len(tens), [], ins, louts, grads, [])
        wi, wr, wm = ops.reppoints_box_loss_backward(pi, pr, want, c["strides"], **kw_l)
        for g, w in zip(grads[:2 * L + 1], wi + wr + [wm]):
            assert torch.equal(bits(g.t), bits(w))
        assert any(bool(g.t.any()) for g in grads[:2 * L]) and all(not g.t.any() for g in grads[2 * L + 1:])
        # req add through the adapter: twice the gradient on top of zeros (by value: 0 + -0 is +0, -0 + -0 is -0)
        acc = [mx_stub.wrap(torch.zeros_like(g.t)) for g in grads]
        for _ in range(2):
            op.backward(["add"] * (2 * L + 1) + ["write"] * 5, [], ins, louts, acc, [])
        for g, w in zip(acc[:2 * L + 1], wi + wr + [wm]):
            assert torch.equal(g.t, w + w)
        with pytest.raises(RuntimeError, match="one launch"):
            op.backward(["null"] + ["write"] * (len(tens) - 1), [], ins, louts, grads, [])
        # the focal loss node on label_refine (builder.py:404-413): the existing operator on the adapter's label
        N, P = want.label_refine.shape
        logits = torch.randn(N, P, 80, device="cuda", generator=torch.Generator("cuda").manual_seed(3))
        Fp = props["_contrib_FocalLoss"](alpha="0.25", gamma="2.0", grad_scale="1.0", normalization="valid", workspace="1500")
        fop = Fp.create_operator(None, Fp.infer_shape([tuple(logits.shape), (N, P)])[0], None)
        fins, fout = [mx_stub.wrap(logits), outs[2]], [mx_stub.wrap(torch.empty_like(logits))]
        fop.forward(True, ["write"], fins, fout, [])
        fgrad = [mx_stub.wrap(torch.full_like(logits, 7)), mx_stub.wrap(torch.zeros(N, P, device="cuda"))]
        fop.backward(["write", "null"], [], fins, fout, fgrad, [])
        prob = ops.focal_loss_forward(logits)
        wgrad = ops.focal_loss_backward(prob, want.label_refine, alpha=0.25, gamma=2.0, grad_scale=1.0, normalization="valid")
        assert torch.equal(bits(fout[0].t), bits(prob)) and torch.equal(bits(fgrad[0].t), bits(wgrad)) and bool(wgrad.any())
    finally:
        plug._state.update(registered=False)
