"""`install(mx, tsd_pool=True)`: a TSD graph (config/TSD/tsd_r50_rpn_1x.py) holds TWO `sd_fpn_deform_roi_pool` nodes
in place of the two get_roi_feature subgraphs of models/TSD/poolings.py:51-174 (level rule, eight masks, eight
DeformablePSROIPooling calls, two add_n) and no DeformablePSROIPooling; without the flag it holds what it held.
`mx.sym.contrib.DeformablePSROIPooling` itself becomes `sd__contrib_DeformablePSROIPooling`, except for parameter
sets outside the kernel's range, which stay native.

The config's TRAIN symbol does not build in the reference itself (models/TSD/bbox_head.py:17 and :243 use the
undefined names `l2` and `tsd_cls_pc_loss`: tests/test_reference_config_sweep.py lists it as broken), so the
train-time form of the subgraph is built here through `TSDConvFCBBoxHead.get_output(..., is_train=True)`, the method
both of the reference's symbols reach the extractors through (bbox_head.py:198, :282), with the config's own
parameter classes; the test symbol is the config's.

CPU only, on the recording stand-in of tests/ref_stubs.py; the GPU round trip through the adapter is the last test."""
import collections
import importlib
import os

import numpy as np
import pytest

from . import mx_stub
from . import ref_stubs as RS

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
CFG = "config.TSD.tsd_r50_rpn_1x"
FUSED, SINGLE, NATIVE = "sd_fpn_deform_roi_pool", "sd__contrib_DeformablePSROIPooling", "DeformablePSROIPooling"


def _install(mx, **flags):
    from simpledet_amd import mxnet_plugin as plug
    plug._state.update(registered=False)
    return plug, plug.install(mx, **flags)


def _ops(sym):
    return collections.Counter(n.op_type for n in RS.walk(sym, {}).values())


def _shape_of(sym):
    return [(n.op_type, n.name, sorted((k, repr(v)) for k, v in n.params.items()), [i.op_type for i in n.inputs])
            for n in RS.walk(sym, {}).values()]


def _find(sym, op_type):
    return [n for n in RS.walk(sym, {}).values() if n.op_type == op_type]


def test_default_installs_register_nothing_new():
    from simpledet_amd.mxnet_plugin import FEATURE_FLAGS
    for flags in ({}, {f: True for f in FEATURE_FLAGS if f != "tsd_pool"}):
        mx = mx_stub.make_stub()
        plug, props = _install(mx, **flags)
        try:
            assert "fpn_deform_roi_pool" not in props and "_contrib_DeformablePSROIPooling" not in props
            assert FUSED not in mx.registry and SINGLE not in mx.registry
            assert plug._state["tsd_pool_patched"] is False
        finally:
            plug._state.update(registered=False)


def test_constructor_alias_and_native_fallback():
    mx = RS.make_mx()
    d, r, t = mx.sym.var("data"), mx.sym.var("rois"), mx.sym.var("trans")
    kw = dict(data=d, rois=r, trans=t, spatial_scale=0.25, output_dim=256, group_size=1, pooled_size=7, part_size=0,
              sample_per_part=4, trans_std=0.1, no_trans=False)
    plug, props = _install(mx)
    try:
        assert mx.sym.contrib.DeformablePSROIPooling(name="n", **kw).op_type == NATIVE     # default: untouched
        plug, props = _install(mx, tsd_pool=True)
        node = mx.sym.contrib.DeformablePSROIPooling(name="n", **kw)
        src = RS.source(node)
        assert src.op_type == SINGLE and src.nout == 2 and [i.name for i in src.inputs] == ["data", "rois", "trans"]
        assert src.params["pooled_size"] == "7" and src.params["spatial_scale"] == "0.25"
        assert plug._state["fallbacks"] == [] or all(f[0] != "_contrib_DeformablePSROIPooling"
                                                     for f in plug._state["fallbacks"])
        # 14 x 14 bins of 8 x 8 samples: 12544 table entries, the kernel holds 4096 -- the node stays native
        big = mx.sym.contrib.DeformablePSROIPooling(name="big", **dict(kw, pooled_size=14, sample_per_part=8))
        assert big.op_type == NATIVE and big.params["pooled_size"] == 14
        odd = mx.sym.contrib.DeformablePSROIPooling(name="odd", **dict(kw, sample_per_part=0))
        assert odd.op_type == NATIVE
        # 32 x 32 bins of 2 x 2 samples: the table alone (4096 entries) fits, the backward's sums next to it do not --
        # the forward must not take what the backward cannot: native
        wide = mx.sym.contrib.DeformablePSROIPooling(name="wide", **dict(kw, pooled_size=32, sample_per_part=2))
        assert wide.op_type == NATIVE
        fb = [(f[0], f[1]) for f in plug._state["fallbacks"] if f[0] == "_contrib_DeformablePSROIPooling"]
        assert fb == [("_contrib_DeformablePSROIPooling", n) for n in ("big", "odd", "wide")]
        P = props["_contrib_DeformablePSROIPooling"]
        assert P.sd_supports(dict(spatial_scale="0.25", output_dim="8", group_size="1", pooled_size="7")) == ""
        assert "do not fit in LDS" in P.sd_supports(dict(spatial_scale="0.25", output_dim="8", group_size="1",
                                                         pooled_size="33", sample_per_part="2"))
        # ... and it is the library's predicate, for one class, on every set of the grid
        from .test_deform_psroi import SUPPORT_GRID
        from simpledet_amd._lib import lib
        for _, pooled, samples in SUPPORT_GRID:
            why = P.sd_supports(dict(spatial_scale="1", output_dim="1", group_size="1", pooled_size=str(pooled),
                                     sample_per_part=str(samples)))
            assert (why == "") == bool(lib().cdll.sd_deform_psroi_pool_supported(1, pooled, samples))
        assert "not one this operator takes" in P.sd_supports(dict(spatial_scale="1", output_dim="1", group_size="1",
                                                                   pooled_size="1", layout="NCHW"))
        # a default install() afterwards puts the native constructor back
        plug, props = _install(mx)
        assert mx.sym.contrib.DeformablePSROIPooling(name="n", **kw).op_type == NATIVE
    finally:
        plug._state.update(registered=False)


def test_prop_shapes_and_arguments():
    mx = mx_stub.make_stub()
    plug, props = _install(mx, tsd_pool=True)
    try:
        P = props["_contrib_DeformablePSROIPooling"](spatial_scale="0.25", output_dim="8", group_size="2",
                                                     pooled_size="7", part_size="3", sample_per_part="4",
                                                     trans_std="0.1")
        assert P.list_arguments() == ["data", "rois", "trans"] and P.list_outputs() == ["output", "top_count"]
        assert P.num_visible_outputs == 1
        assert P.infer_shape([(2, 32, 13, 17), (6, 5), (6, 4, 3, 3)])[1] == [(6, 8, 7, 7)] * 2
        # six classes of 7 x 7 x 16 fit for one class but not for six: known only here, so it raises
        P6 = props["_contrib_DeformablePSROIPooling"](spatial_scale="0.25", output_dim="6", group_size="1",
                                                      pooled_size="7", sample_per_part="4", trans_std="0.1")
        with pytest.raises(ValueError, match="do not fit"):
            P6.infer_shape([(2, 6, 13, 17), (6, 5), (6, 12, 7, 7)])
        assert P6.infer_shape([(2, 6, 13, 17), (6, 5), (6, 6, 7, 7)])[1] == [(6, 6, 7, 7)] * 2
        for bad in ([(2, 31, 13, 17), (6, 5), (6, 4, 3, 3)], [(2, 32, 13, 17), (6, 4), (6, 4, 3, 3)],
                    [(2, 32, 13, 17), (6, 5), (6, 4, 7, 7)], [(2, 32, 13, 17), (6, 5), (6, 6, 3, 3)]):
            with pytest.raises(ValueError):
                P.infer_shape(bad)
        N = props["_contrib_DeformablePSROIPooling"](spatial_scale="0.25", output_dim="8", group_size="1",
                                                     pooled_size="3", no_trans="True")
        assert N.list_arguments() == ["data", "rois"] and N.infer_shape([(2, 8, 4, 4), (3, 5)])[1] == [(3, 8, 3, 3)] * 2
        with pytest.raises(ValueError):
            props["_contrib_DeformablePSROIPooling"](spatial_scale="1", output_dim="8", group_size="1",
                                                     pooled_size="14", sample_per_part="8")
        F = props["fpn_deform_roi_pool"](rcnn_stride="(4, 8, 16, 32)", pooled_size="7")
        assert F.g["sample_per_part"] == 4 and F.g["trans_std"] == 0.1 and F.g["scale0"] == 224 and F.g["lvl0"] == 4
        assert F.list_arguments() == ["data_s4", "data_s8", "data_s16", "data_s32", "rois", "trans"]
        feats = [(2, 5, 16, 20), (2, 5, 8, 10), (2, 5, 4, 5), (2, 5, 2, 3)]
        assert F.infer_shape(feats + [(2, 7, 4), (14, 2, 7, 7)])[1] == [(14, 5, 7, 7), (14, 4, 7, 7)]
        assert F.infer_shape(feats + [(2, 7, 4), (14, 2)])[1] == [(14, 5, 7, 7), (14, 4, 7, 7)]
        for bad in (feats + [(2, 7, 4), (14, 2, 3, 3)], feats + [(14, 4), (14, 2)], feats[:3] + [(2, 7, 4), (14, 2)]):
            with pytest.raises(ValueError):
                F.infer_shape(bad)
        with pytest.raises(ValueError):
            props["fpn_deform_roi_pool"](rcnn_stride="(1, 2, 3, 4, 5, 6)")
        deps = F.declare_backward_dependency(["g"], list("abcdrt"), ["o", "c"])
        assert deps == ["g"] + list("abcdrt") + ["c"]
        if not os.path.isdir(REF):    # the pooling module is absent: nothing is rebound and the fallback list says so
            assert plug._state["tsd_pool_patched"] is False
            assert [f[0] for f in plug._state["fallbacks"]] == ["fpn_deform_roi_pool"]
    finally:
        plug._state.update(registered=False)


def _test_symbol(R, **flags):
    plug, _ = _install(R.mx, **flags)
    cfg = importlib.import_module(CFG)
    importlib.import_module("symbol.builder").RPN._rpn_output = None
    out = cfg.get_config(False)
    sym, = [o.test_symbol for o in out if isinstance(getattr(o, "test_symbol", None), RS.Symbol)]
    return sym, out


def _train_subgraph(R, out):
    """bbox_head.get_output(is_train=True) over the config's own parameter classes: the train-time extractors"""
    mx = R.mx
    roi_param, = [o for o in out if getattr(o, "__name__", "") == "RoiParam"]
    bbox_param, = [o for o in out if getattr(o, "__name__", "") == "BboxParam"]
    poolings = importlib.import_module("models.TSD.poolings")
    head = importlib.import_module("models.TSD.bbox_head").TSDConvFCBBoxHead(
        bbox_param, poolings.FPNRoIAlign_DeltaC(roi_param), poolings.FPNRoIAlign_DeltaR(roi_param))
    feats = {"stride%d" % s: mx.sym.var("feat_s%d" % s) for s in roi_param.stride}
    return mx.sym.Group(list(head.get_output(feats, mx.sym.var("roi_feat"), mx.sym.var("rois"), is_train=True)))


@needs_ref
def test_tsd_graphs_hold_the_two_fused_nodes():
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        poolings = importlib.import_module("models.TSD.poolings")
        ref_c, ref_r = poolings.FPNRoIAlign_DeltaC.get_roi_feature, poolings.FPNRoIAlign_DeltaR.get_roi_feature
        try:
            # (the reference keeps built sub-graphs on its classes, symbol/builder.py:26-27, 38: the first build of a
            # process differs from every later one in how many backbone / neck nodes it shares, so it is not the baseline)
            _test_symbol(R)
            native_test, out = _test_symbol(R)
            assert poolings.FPNRoIAlign_DeltaC.get_roi_feature is ref_c and not plug._state["tsd_pool_patched"]
            native_train = _train_subgraph(R, out)
            for native in (_ops(native_test), _ops(native_train)):
                assert native[NATIVE] == 8 and native[FUSED] == 0 and native[SINGLE] == 0 and native["add_n"] >= 2
            # the reference's own train symbol: broken with and without the plugin
            with pytest.raises(NameError):
                importlib.import_module(CFG).get_config(True)

            test, out = _test_symbol(R, tsd_pool=True)
            assert plug._state["tsd_pool_patched"]
            assert poolings.FPNRoIAlign_DeltaC._sd_reference_get_roi_feature is ref_c
            assert poolings.FPNRoIAlign_DeltaR._sd_reference_get_roi_feature is ref_r
            plug.install(R.mx, tsd_pool=True)            # a second install keeps the first originals
            assert poolings.FPNRoIAlign_DeltaC._sd_reference_get_roi_feature is ref_c
            train = _train_subgraph(R, out)
            with pytest.raises(NameError):
                importlib.import_module(CFG).get_config(True)
            for sym, native in ((test, native_test), (train, native_train)):
                got = _ops(sym)
                assert got[FUSED] == 2 and got[NATIVE] == 0 and got[SINGLE] == 0, dict(got)
                assert got["where"] == 0 and got["Convolution"] == _ops(native)["Convolution"]
                nodes = {n.name: n for n in _find(sym, FUSED)}
                assert sorted(nodes) == ["delta_c_pooled_feat", "delta_r_pooled_feat"]
                for name, node in nodes.items():
                    assert node.nout == 2
                    assert node.params == {"rcnn_stride": "(4, 8, 16, 32)", "pooled_size": "7", "sample_per_part": "4",
                                           "trans_std": "0.1", "roi_canonical_scale": "224", "roi_canonical_level": "4"}
                    assert len(node.inputs) == 6
                    tr = RS.source(node.inputs[5])
                    assert tr.op_type == "reshape"
                    assert tr.params["shape"] == ((-1, 2, 7, 7) if name.startswith("delta_c") else (-1, 2))
                    # both extractors read the same four level features and the same rois
                assert [RS.source(i) for i in nodes["delta_c_pooled_feat"].inputs[:5]] == \
                       [RS.source(i) for i in nodes["delta_r_pooled_feat"].inputs[:5]]
            assert not any(f[0] == "fpn_deform_roi_pool" for f in plug._state["fallbacks"])

            # a default install() afterwards: node for node the native graphs
            again_test, out = _test_symbol(R)
            assert poolings.FPNRoIAlign_DeltaC.get_roi_feature is ref_c
            assert poolings.FPNRoIAlign_DeltaR.get_roi_feature is ref_r and not plug._state["tsd_pool_patched"]
            assert _shape_of(again_test) == _shape_of(native_test)
            assert _shape_of(_train_subgraph(R, out)) == _shape_of(native_train)
        finally:
            plug.unpatch_tsd_pool(poolings)
            plug._state.update(registered=False)


@pytest.mark.gpu
def test_adapters_equal_the_ops_calls(ops):
    import torch
    from . import deform_psroi_ref as dr
    from .test_deform_psroi import FSHAPES, FSTRIDES, _fused_rois
    mx = mx_stub.make_stub()
    plug, props = _install(mx, tsd_pool=True)
    try:
        rs = np.random.RandomState(5)
        feats = [torch.from_numpy(rs.standard_normal((2, 5) + s).astype(np.float32)).cuda() for s in FSHAPES]
        rois = torch.from_numpy(_fused_rois(rs)).cuda()
        dy = torch.from_numpy(rs.standard_normal((14, 5, 7, 7)).astype(np.float32)).cuda()
        for tshape in ((14, 2, 7, 7), (14, 2)):
            trans = torch.from_numpy(rs.standard_normal(tshape).astype(np.float32)).cuda()
            P = props["fpn_deform_roi_pool"](rcnn_stride=str(FSTRIDES), pooled_size="7", roi_canonical_scale="16")
            tensors = feats + [rois, trans]
            ishape, oshape = P.infer_shape([tuple(t.shape) for t in tensors])[:2]
            op = P.create_operator(None, ishape, None)
            ins = [mx_stub.wrap(t) for t in tensors]
            outs = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
            op.forward(True, ["write"] * 2, ins, outs, [])
            want = ops.fpn_deform_roi_pool_forward(feats, rois, trans, FSTRIDES, 7, roi_canonical_scale=16)
            for g, w in zip(outs, want):
                assert torch.equal(g.t.view(torch.int32), w.view(torch.int32))
            grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7.0, device="cuda")) for t in tensors]
            op.backward(["write"] * 6, [mx_stub.wrap(dy)], ins, outs, grads, [])
            wf, wt = ops.fpn_deform_roi_pool_backward(dy, feats, rois, trans, want[1], FSTRIDES, 7,
                                                      roi_canonical_scale=16)
            assert torch.equal(grads[5].t.view(torch.int32), wt.view(torch.int32)) and not grads[4].t.any()
            for g, w in zip(grads[:4], wf):     # float atomics: equal up to the order of a pixel's adds
                torch.testing.assert_close(g.t, w, rtol=1e-5, atol=1e-5)
        # the single-level operator
        data = torch.from_numpy(rs.standard_normal((2, 8, 13, 17)).astype(np.float32)).cuda()
        r5 = torch.tensor([[0, 9, 7, 41, 37], [1, -21, -11, 22, 26], [1, 4.5, 6.5, 30.5, 40.5]], device="cuda")
        trans = torch.from_numpy(rs.standard_normal((3, 4, 3, 3)).astype(np.float32)).cuda()
        kw = dict(spatial_scale=0.25, output_dim=8, group_size=1, pooled_size=7, part_size=3, sample_per_part=4,
                  trans_std=0.1, no_trans=False)
        P = props["_contrib_DeformablePSROIPooling"](**{k: str(v) for k, v in kw.items()})
        tensors = [data, r5, trans]
        ishape, oshape = P.infer_shape([tuple(t.shape) for t in tensors])[:2]
        op = P.create_operator(None, ishape, None)
        ins = [mx_stub.wrap(t) for t in tensors]
        outs = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in oshape]
        op.forward(True, ["write"] * 2, ins, outs, [])
        want = ops.deform_psroi_pool_forward(data, r5, trans, **kw)
        for g, w in zip(outs, want):
            assert torch.equal(g.t.view(torch.int32), w.view(torch.int32))
        g_y = torch.from_numpy(rs.standard_normal(oshape[0]).astype(np.float32)).cuda()
        grads = [mx_stub.wrap(torch.full(tuple(t.shape), 7.0, device="cuda")) for t in tensors]
        op.backward(["write"] * 3, [mx_stub.wrap(g_y)], ins, outs, grads, [])
        wd, wr, wt = ops.deform_psroi_pool_backward(g_y, data, r5, trans, want[1], **kw)
        assert torch.equal(grads[2].t.view(torch.int32), wt.view(torch.int32)) and not grads[1].t.any()
        torch.testing.assert_close(grads[0].t, wd, rtol=1e-5, atol=1e-5)
        with pytest.raises(RuntimeError, match="kAddTo"):
            op.forward(True, ["add", "write"], ins, outs, [])
    finally:
        plug._state.update(registered=False)
