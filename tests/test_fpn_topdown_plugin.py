"""simpledet_amd/fpn_topdown.py: the CustomOp, plan_topdown on graph dictionaries in MXNet's schema, rewrite and the
merge_bn wrapper.  CPU, on tests/mx_stub.py and the recording double of tests/test_merged_bn_plugin.py (real MXNet is
not installed: the rebuilt graph is checked against the double only).  Where the reference tree is present its own
FPN, RetinaNet, FCOS, RepPoints and NASFPN (FPN variant) necks are recorded unmodified and the plans' node names
compared with tests/golden/fpn_topdown_plans.json; the GPU round trip through the adapter is the last test."""
import importlib
import json
import os
import types

import numpy as np
import pytest

from . import fpn_topdown_ref as fr
from . import mx_stub, ref_stubs
from .test_merged_bn_plugin import _bottleneck, _double, _graph, _params, to_json

HAS_REFERENCE = os.path.isdir("/root/reference")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fpn_topdown_plans.json")


@pytest.fixture()
def plug():
    from simpledet_amd import fpn_topdown, merged_bn, mxnet_plugin
    saved = dict(mxnet_plugin._state)
    yield fpn_topdown, merged_bn, mxnet_plugin
    fpn_topdown._own.update(installed=False, props={})
    merged_bn._own.update(installed=False, props={})
    mxnet_plugin._state.clear()
    mxnet_plugin._state.update(saved)
    mxnet_plugin._state.update(registered=False)


# ---------------------------------------------------------------------------------- the operator --
def test_install_registers_and_leaves_the_plugin_as_it_is(plug):
    fpn_topdown, _, mxnet_plugin = plug
    flags = tuple(mxnet_plugin.FEATURE_FLAGS)
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    before = set(mxnet_plugin.install(mx))
    everything = set(mxnet_plugin._state["all_ops"])
    registry_before = set(mx.registry)
    props = fpn_topdown.install(mx)
    assert sorted(props) == ["fpn_topdown"] and set(mx.registry) - registry_before == {"sd_fpn_topdown"}
    assert mxnet_plugin.FEATURE_FLAGS == flags and tuple(mxnet_plugin._FEATURES) == flags
    mxnet_plugin._state.update(registered=False)
    assert set(mxnet_plugin.install(mx)) == before and set(mxnet_plugin._state["all_ops"]) == everything
    assert "fpn_topdown" not in everything
    with pytest.raises(TypeError):
        mxnet_plugin.install(mx, fpn_topdown=True)
    fpn_topdown.install(mx, stream=1234, sync=False)                    # the stream / sync state is the plugin's
    assert mxnet_plugin._state["stream"] == 1234 and mxnet_plugin._state["sync"] is False
    v = mx.sym.Variable
    node = fpn_topdown.fpn_topdown(v("p5"), [v("la4"), v("la3")], name="td", mx=mx)
    assert node.op_type == "sd_fpn_topdown" and node.nout == 2 and node.params == {"num_levels": "3"}
    assert [i.op_type for i in node.inputs] == ["var:p5", "var:la4", "var:la3"]


def test_rewrite_needs_install(plug):
    fpn_topdown, _, _ = plug
    with pytest.raises(RuntimeError, match="install"):
        fpn_topdown.rewrite(_double().sym.var("x"))


def test_prop_shapes_types_and_the_backward_dependency(plug):
    fpn_topdown, _, _ = plug
    P = fpn_topdown.install(mx_stub.make_stub())["fpn_topdown"]
    p = P(num_levels="4")                                               # parameters arrive as strings
    assert p.list_arguments() == ["top", "lateral1", "lateral2", "lateral3"]
    assert p.list_outputs() == ["out1", "out2", "out3"] and p.need_top_grad_ is True
    sh = [(2, 256) + hw for hw in fr.FPN_CHAIN]
    assert p.infer_shape([list(s) for s in sh]) == (sh, sh[1:], [])
    assert P().L == 4 and P(num_levels="2").list_outputs() == ["out1"]
    for bad in ("1", "7"):
        with pytest.raises(ValueError, match="num_levels"):
            P(num_levels=bad)
    with pytest.raises(ValueError, match="larger than twice"):
        p.infer_shape([sh[0], (2, 256, 51, 84), sh[2], sh[3]])
    with pytest.raises(ValueError, match="larger than twice"):
        p.infer_shape([sh[0], sh[1], (2, 256, 100, 169), sh[3]])
    with pytest.raises(ValueError, match=r"\(N,C\)"):
        p.infer_shape([sh[0], (2, 128, 50, 84), sh[2], sh[3]])
    with pytest.raises(ValueError, match="inputs"):
        p.infer_shape(sh[:3])
    with pytest.raises(ValueError, match=r"\(N,C,H,W\)"):
        p.infer_shape([sh[0], (2, 256, 50), sh[2], sh[3]])
    assert p.infer_type([np.float16] + [None] * 3) == ([np.float16] * 4, [np.float16] * 3, [])
    assert p.infer_type([np.float32] * 4) == ([np.float32] * 4, [np.float32] * 3, [])
    with pytest.raises(TypeError):
        p.infer_type([np.float64] * 4)
    # the output gradients alone: no forward tensor is kept alive
    assert p.declare_backward_dependency(["g1", "g2", "g3"], ["t", "a", "b", "c"], ["o1", "o2", "o3"]) == ["g1", "g2", "g3"]
    assert p.create_operator(None, None, [np.float16] * 4).sfx == "_f16"
    assert p.create_operator(None, None, [np.float32] * 4).sfx == "" and p.create_operator(None, None, None).sfx == ""


# ---------------------------------------------------------------------------------- plan_topdown --
UP = {"scale": "2", "sample_type": "nearest", "num_args": "1"}


def _step(coarse, lateral, tag, up=UP, clip=None, add="add_n", swap=False, extra=()):
    ops = [lateral, tag + "_clip"] if swap else [tag + "_clip", lateral]
    return [("UpSampling", tag + "_up", [coarse], up), ("slice_like", tag + "_clip", [tag + "_up", lateral], clip),
            (add, tag + "_sum", ops + list(extra), None)]


def _neck(levels, kw=None):
    """laterals la0 .. la{levels-1} (la0 the top) and the chain of steps s1 .. ; a 3x3 convolution behind every sum"""
    spec = [("null", "w", [], None)] + [("null", "la%d" % l, [], None) for l in range(levels)]
    coarse, kw = "la0", kw or {}
    for l in range(1, levels):
        spec += _step(coarse, "la%d" % l, "s%d" % l, **kw.get(l, {}))
        coarse = "s%d_sum" % l
    spec += [("Convolution", "conv%d" % l, ["s%d_sum" % l if l else "la0", "w"], None) for l in range(levels)]
    return spec, ["conv%d" % l for l in range(levels)]


def _plans(spec, heads):
    from simpledet_amd import fpn_topdown
    g, ids = _graph(spec, heads)
    frozen = json.dumps(g, sort_keys=True)
    plans = fpn_topdown.plan_topdown(g)
    assert json.dumps(g, sort_keys=True) == frozen                      # a pure function
    names = {v: k for k, v in ids.items()}
    nm = lambda e: names[e[0]] if isinstance(e, list) else names[e]     # noqa: E731
    return [dict(L=p["L"], top=nm(p["top"]), laterals=[nm(e) for e in p["laterals"]], sums=[nm(e) for e in p["sums"]],
                 folded=sorted(nm(e) for e in p["folded"])) for p in plans]


def _chain(levels):
    tags = ["s%d" % l for l in range(1, levels)]
    return dict(L=levels, top="la0", laterals=["la%d" % l for l in range(1, levels)], sums=[t + "_sum" for t in tags],
                folded=sorted(t + s for t in tags for s in ("_up", "_clip", "_sum")))


def test_plan_an_fpn_chain_is_one_plan_of_four_levels():
    assert _plans(*_neck(4)) == [_chain(4)]


def test_plan_retina_is_three_levels():
    assert _plans(*_neck(3)) == [_chain(3)]


def test_plan_accepts_every_add_in_either_operand_order():
    for add in ("add_n", "ElementWiseSum", "elemwise_add", "_Plus", "_plus"):
        for swap in (False, True):
            assert _plans(*_neck(3, {1: dict(add=add, swap=swap), 2: dict(add=add, swap=not swap)})) == [_chain(3)]
    # absent attributes of slice_like, and axes given as "all", are the same thing
    assert _plans(*_neck(3, {1: dict(clip={"axes": "()"}), 2: dict(clip={"axes": "None"})})) == [_chain(3)]


def _broken_at_2(levels=4):
    """what is left when the step into level 2 cannot be folded: la0 -> la1 alone, and la2 -> la3 alone"""
    return [dict(L=2, top="la0", laterals=["la1"], sums=["s1_sum"], folded=["s1_clip", "s1_sum", "s1_up"]),
            dict(L=2, top="s2_sum", laterals=["la3"], sums=["s3_sum"], folded=["s3_clip", "s3_sum", "s3_up"])]


def test_plan_refuses_a_second_consumer_of_the_upsampling():
    spec, heads = _neck(4)
    assert _plans(spec + [("Pooling", "peek", ["s2_up"], None)], heads + ["peek"]) == _broken_at_2()


def test_plan_refuses_a_second_consumer_of_the_slice_like():
    spec, heads = _neck(4)
    assert _plans(spec + [("Pooling", "peek", ["s2_clip"], None)], heads + ["peek"]) == _broken_at_2()


def test_plan_refuses_scale_4():
    assert _plans(*_neck(4, {2: dict(up=dict(UP, scale="4"))})) == _broken_at_2()


def test_plan_refuses_bilinear():
    assert _plans(*_neck(4, {2: dict(up=dict(UP, sample_type="bilinear"))})) == _broken_at_2()
    # ... and the two-argument form bilinear UpSampling takes
    assert _plans(*_neck(4, {2: dict(up=dict(UP, num_args="2"))})) == _broken_at_2()


def test_plan_refuses_slice_like_with_axes():
    assert _plans(*_neck(4, {2: dict(clip={"axes": "(2, 3)"})})) == _broken_at_2()


def test_plan_refuses_a_three_input_add():
    spec, heads = _neck(4, {2: dict(extra=["la0"])})
    assert _plans(spec, heads) == _broken_at_2()


def test_plan_refuses_a_head_on_an_inner_link():
    spec, heads = _neck(4)
    assert _plans(spec, heads + ["s2_up"]) == _broken_at_2()
    assert _plans(spec, heads + ["s2_clip"]) == _broken_at_2()
    # the sum itself may be a head and have any consumers
    assert _plans(spec + [("Pooling", "peek", ["s2_sum"], None)], heads + ["peek", "s2_sum"]) == [_chain(4)]


def test_plan_other_shapes_of_graph():
    # the add's other operand is not the slice_like's shape reference
    spec, heads = _neck(3)
    spec = [("null", "other", [], None)] + [n if n[1] != "s1_sum" else ("add_n", "s1_sum", ["s1_clip", "other"], None)
                                            for n in spec]
    assert [p["sums"] for p in _plans(spec, heads)] == [["s2_sum"]]
    # one sum feeds two UpSamplings: the first in node order continues the chain, the second starts its own
    spec, heads = _neck(3)
    spec += [("null", "lb", [], None)] + _step("s1_sum", "lb", "t")
    assert [(p["top"], p["sums"]) for p in _plans(spec, heads + ["t_sum"])] == [("la0", ["s1_sum", "s2_sum"]),
                                                                                   ("s1_sum", ["t_sum"])]
    # a lateral that depends on an earlier sum of the chain cannot enter the same fused node
    spec = [("null", "w", [], None), ("null", "la0", [], None), ("null", "la1", [], None)] + _step("la0", "la1", "s1")
    spec += [("Convolution", "la2", ["s1_sum", "w"], None)] + _step("s1_sum", "la2", "s2")
    assert [(p["top"], p["sums"]) for p in _plans(spec, ["s2_sum"])] == [("la0", ["s1_sum"]), ("s1_sum", ["s2_sum"])]
    # seven levels: six in the first node, the rest in a second
    got = _plans(*_neck(8))
    assert [p["L"] for p in got] == [6, 3] and got[1]["top"] == "s5_sum"
    assert _plans([("null", "x", [], None), ("relu", "y", ["x"], None)], ["y"]) == []


# --------------------------------------------------------------------------------------- rewrite --
def _fpn_symbol(mx, levels=4):
    """a neck as the reference's builders record it: lateral 1x1 convolutions, the chain, 3x3 convolutions"""
    S = mx.sym
    v = S.var
    las = [S.Convolution(v("c%d" % l), v("P%d_lateral_weight" % l), kernel=(1, 1), name="P%d_lateral" % l)
           for l in range(levels)]
    p, outs = las[0], []
    outs.append(S.Convolution(p, v("P0_conv_weight"), kernel=(3, 3), name="P0_conv"))
    for l in range(1, levels):
        up = S.UpSampling(p, scale=2, sample_type="nearest", num_args=1, name="P%d_upsampling" % l)
        clip = S.slice_like(up, las[l], name="P%d_clip" % l)
        p = S.add_n(clip, las[l], name="P%d_sum" % l)
        outs.append(S.Convolution(p, v("P%d_conv_weight" % l), kernel=(3, 3), name="P%d_conv" % l))
    return S.Group(outs)


def _by_name(sym):
    return {n.name: n for n in ref_stubs.walk(sym).values() if n.name}


def _signature(sym):
    """every node by name: (op, parameters, the names -- and output indices -- of its inputs)"""
    def inp(i):
        return (i.parent.name, i.index) if i.op_type == "_output" else (i.name, 0)
    return {n.name: (n.op_type, {k: str(v) for k, v in n.params.items()}, [inp(i) for i in n.inputs])   # (JSON's strings)
            for n in ref_stubs.walk(sym).values() if n.name}


def test_rewrite_preserves_heads_and_every_untouched_node(plug):
    fpn_topdown, _, _ = plug
    mx = _double()
    fpn_topdown.install(mx)
    sym = _fpn_symbol(mx)
    before = _signature(sym)
    out = fpn_topdown.rewrite(sym)
    after = _signature(out)
    assert out.op_type == "Group" and [h.name for h in out.inputs] == ["P%d_conv" % l for l in range(4)]
    gone = {"P%d_%s" % (l, s) for l in (1, 2, 3) for s in ("upsampling", "clip", "sum")}
    assert set(before) - set(after) == gone and set(after) - set(before) == {"P3_sum_topdown"}
    fused = _by_name(out)["P3_sum_topdown"]
    assert fused.op_type == "Custom" and fused.params == dict(op_type="sd_fpn_topdown", num_levels="4")
    assert fused.nout == 3 and [i.name for i in fused.inputs] == ["P%d_lateral" % l for l in range(4)]
    for name, sig in before.items():
        if name in gone:
            continue
        if name in ("P1_conv", "P2_conv", "P3_conv"):                  # they read the fused node's outputs instead
            l = int(name[1])
            assert after[name] == (sig[0], sig[1], [("P3_sum_topdown", l - 1), sig[2][1]])
        else:
            assert after[name] == sig, name


def test_rewrite_twice_is_a_no_op_the_second_time(plug):
    fpn_topdown, _, _ = plug
    mx = _double()
    fpn_topdown.install(mx)
    once = fpn_topdown.rewrite(_fpn_symbol(mx))
    assert fpn_topdown.plan_topdown(to_json(once)) == []
    assert fpn_topdown.rewrite(once) is once
    plain = mx.sym.Convolution(mx.sym.var("x"), mx.sym.var("w"), name="c")
    assert fpn_topdown.rewrite(plain) is plain                          # nothing to fuse: the symbol itself


# ------------------------------------------------------------------- the reference's own necks --
NECKS = {"FPN": ("models.FPN.builder", "FPNNeck", "fpn_neck"),
         "RetinaNet": ("models.retinanet.builder", "RetinaNetNeck", "get_retinanet_neck"),
         "FCOS": ("models.FCOS.builder", "FCOSFPNNeck", "fpn_neck"),
         "RepPoints": ("models.RepPoints.builder", "RepPointsNeck", "get_fpn_neck"),
         "NASFPN": ("models.NASFPN.builder", "RetinaNetNeckWithBN", "get_retinanet_neck")}


def test_golden_plans_schema():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(NECKS)
    for key, plans in golden.items():
        assert plans, key
        for p in plans:
            assert sorted(p) == ["L", "clips", "laterals", "sums", "top", "ups"]
            assert 2 <= p["L"] <= 6 and all(len(p[k]) == p["L"] - 1 for k in ("laterals", "sums", "ups", "clips"))
            assert isinstance(p["top"], str) and all(isinstance(n, str) for k in ("laterals", "sums", "ups", "clips")
                                                     for n in p[k])
    assert golden["FPN"][0]["L"] == 4 and all(golden[k][0]["L"] == 3 for k in golden if k != "FPN")


@pytest.mark.skipif(not HAS_REFERENCE, reason="/root/reference not present")
@pytest.mark.parametrize("key", sorted(NECKS))
def test_the_references_necks_give_the_recorded_plans(key):
    from simpledet_amd import fpn_topdown

    def fix_bn(sym, *a, **kw):
        return sym

    class Param:
        normalizer = staticmethod(fix_bn)
        fp16 = False

        def __getattr__(self, k):
            return None
    module, cls, method = NECKS[key]
    with ref_stubs.reference_modules() as R:
        neck = getattr(importlib.import_module(module), cls)(Param())
        out = getattr(neck, method)([R.mx.sym.var("c%d" % i) for i in (2, 3, 4, 5)])
        g = to_json(R.mx.sym.Group(ref_stubs._flatten_syms([out])))
    nm = lambda e: g["nodes"][e[0] if isinstance(e, list) else e]["name"]   # noqa: E731
    got = [dict(L=p["L"], top=nm(p["top"]), **{k: [nm(e) for e in p[k]] for k in ("laterals", "sums", "ups", "clips")})
           for p in fpn_topdown.plan_topdown(g)]
    assert got == json.load(open(GOLDEN))[key]


# -------------------------------------------------------------------------------- patch_merge_bn --
def _module(fn):
    mod = types.ModuleType("utils.graph_optimize")
    mod.merge_bn = fn
    return mod


def test_patch_merge_bn_alone_is_idempotent_and_unpatch_restores(plug):
    fpn_topdown, _, _ = plug
    mx = _double()
    fpn_topdown.install(mx)
    calls = []

    def reference(symbol, args, auxs, symbol_only=False):
        calls.append(symbol_only)
        return symbol, args, auxs
    mod = _module(reference)
    assert fpn_topdown.patch_merge_bn(mod) is mod and mod.merge_bn is not reference
    wrapper = mod.merge_bn
    fpn_topdown.patch_merge_bn(mod)                                     # a second call wraps nothing twice
    assert mod.merge_bn is wrapper and wrapper._sd_topdown_inner is reference
    args, auxs = {"a": 1}, {"b": 2}
    out, a2, x2 = mod.merge_bn(_fpn_symbol(mx), args, auxs, True)
    assert a2 is args and x2 is auxs and calls == [True]
    ops = [n.op_type for n in ref_stubs.walk(out).values()]
    assert ops.count("Custom") == 1 and not {"UpSampling", "slice_like", "add_n"} & set(ops)
    fpn_topdown.unpatch_merge_bn(mod)
    assert mod.merge_bn is reference
    fpn_topdown.unpatch_merge_bn(mod)                                   # nothing to undo: nothing happens
    assert mod.merge_bn is reference


def test_patch_merge_bn_composes_with_merged_bn(plug):
    """after merged_bn.patch_merge_bn(): both fusions in the result; merged_bn rebinding afterwards drops ours"""
    fpn_topdown, merged_bn, _ = plug
    mx = _double()
    merged_bn.install(mx)
    fpn_topdown.install(mx)

    def reference(symbol, args, auxs, symbol_only=False):
        raise AssertionError("the reference's merge_bn is not reached")
    mod = _module(reference)
    merged_bn.patch_merge_bn(mod)
    fpn_topdown.patch_merge_bn(mod)
    assert mod.merge_bn._sd_topdown_inner is merged_bn.merge_bn
    # a bottleneck (four merged-BN chains) whose output is the top of a two-level pathway
    S = mx.sym
    c5 = _bottleneck(mx).inputs[0]                                      # the pooling behind the last relu
    top = S.Convolution(c5, S.var("P5_lateral_weight"), kernel=(1, 1), name="P5_lateral")
    la = S.Convolution(S.var("c4"), S.var("P4_lateral_weight"), kernel=(1, 1), name="P4_lateral")
    up = S.UpSampling(top, scale=2, sample_type="nearest", num_args=1, name="P5_upsampling")
    p4 = S.add_n(S.slice_like(up, la, name="P4_clip"), la, name="P4_sum")
    sym = S.Convolution(p4, S.var("P4_conv_weight"), kernel=(3, 3), name="P4_conv")
    args, auxs = _params()
    out, _, _ = mod.merge_bn(sym, args, auxs)
    kinds = sorted(n.params["op_type"] for n in ref_stubs.walk(out).values() if n.op_type == "Custom")
    assert kinds == ["sd_fpn_topdown"] + ["sd_scale_bias_act"] * 4
    assert out.name == "P4_conv" and out.inputs[0].name == "P4_sum_topdown"     # (one output: the node itself)
    assert args["bn1_gamma"].shape == (1, 4, 1, 1)                      # merged_bn did its part on the parameters
    # the order matters, as documented: merged_bn.patch_merge_bn() afterwards rebinds the function and drops ours
    merged_bn.patch_merge_bn(mod)
    assert mod.merge_bn is merged_bn.merge_bn
    fpn_topdown.patch_merge_bn(mod)
    fpn_topdown.unpatch_merge_bn(mod)
    assert mod.merge_bn is merged_bn.merge_bn
    merged_bn.unpatch_merge_bn(mod)
    assert mod.merge_bn is reference


# ------------------------------------------------------------------------------------------ GPU --
@pytest.mark.gpu
@pytest.mark.parametrize("dtname", ["float32", "float16"])
def test_adapter_round_trip(plug, ops, dtname):
    import torch
    fpn_topdown, _, _ = plug
    mx = mx_stub.make_stub()
    P = fpn_topdown.install(mx)["fpn_topdown"]
    dt = np.dtype(dtname).type
    tdt = torch.float32 if dtname == "float32" else torch.float16
    top, lats, grads = fr.make(np.random.RandomState(8), fr.CHAINS["even_odd"], dt)
    shapes = [top.shape] + [x.shape for x in lats]
    w = lambda a: mx_stub.wrap(torch.from_numpy(np.ascontiguousarray(a)).cuda())             # noqa: E731
    nan = lambda s: mx_stub.wrap(torch.full(tuple(s), float("nan"), dtype=tdt, device="cuda"))  # noqa: E731
    p = P(num_levels="4")
    ishape, oshape, _ = p.infer_shape(shapes)
    op = p.create_operator(None, ishape, [dt] * 4)
    ins, outs = [w(top)] + [w(x) for x in lats], [nan(s) for s in oshape]
    op.forward(True, ["write"] * 3, ins, outs, [])
    for l, want in enumerate(fr.fwd(top, lats)):
        assert fr.same_bits(outs[l].t.cpu().numpy(), want), (dtname, "out", l + 1)
    w_top, w_lat = fr.bwd(grads, shapes)
    in_grad = [nan(s) for s in ishape]
    og = [w(g) for g in grads]
    op.backward(["write"] * 4, og, [None] * 4, [None] * 3, in_grad, [])   # no forward tensor is a dependency
    assert fr.same_bits(in_grad[0].t.cpu().numpy(), w_top)
    for l in range(3):
        assert fr.same_bits(in_grad[l + 1].t.cpu().numpy(), w_lat[l]), (dtname, "d_lateral", l + 1)
    # gradients nobody wants are not written
    in_grad = [nan(s) for s in ishape]
    op.backward(["null", "write", "null", "write"], og, [None] * 4, [None] * 3, in_grad, [])
    assert torch.isnan(in_grad[0].t).all() and torch.isnan(in_grad[2].t).all()
    assert fr.same_bits(in_grad[1].t.cpu().numpy(), w_lat[0]) and fr.same_bits(in_grad[3].t.cpu().numpy(), w_lat[2])
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["add", "write", "write", "write"], og, [None] * 4, [None] * 3, in_grad, [])
    with pytest.raises(RuntimeError, match="kAddTo"):
        op.forward(True, ["write", "add", "write"], ins, outs, [])
