"""`simpledet_amd.sync_bn.install(mx)`: `mx.sym.contrib.SyncBatchNorm` builds an `sd__contrib_SyncBatchNorm` Custom
node with the reference's arguments, auxiliary states, outputs, visible count, defaults and shape inference
(sync_batch_norm-inl.h:49-76,556-662); `use_global_stats=True` goes back to the native constructor; uninstall()
puts the constructor back; mxnet_plugin's tables are untouched.  CPU on tests/mx_stub.py and the recording stand-in
of tests/ref_stubs.py; the GPU round trips through the adapter are the last tests."""
import numpy as np
import pytest

from . import mx_stub, ref_stubs

F = np.float32


def _native(*a, **kw):
    return ("native SyncBatchNorm", a, kw)


@pytest.fixture()
def sbn():
    from simpledet_amd import mxnet_plugin, sync_bn
    flags = tuple(mxnet_plugin.FEATURE_FLAGS)
    features = tuple(mxnet_plugin._FEATURES)
    mx = mx_stub.make_stub()
    mx.sym.contrib.SyncBatchNorm = _native        # what a SimpleDet build of MXNet registers natively
    props = sync_bn.install(mx)
    yield mx, props, sync_bn
    sync_bn.uninstall(mx)
    assert tuple(mxnet_plugin.FEATURE_FLAGS) == flags and tuple(mxnet_plugin._FEATURES) == features


def test_install_aliases_and_uninstall_restores(sbn):
    mx, props, sync_bn = sbn
    from simpledet_amd import mxnet_plugin
    assert set(props) == {"_contrib_SyncBatchNorm"} and "sd__contrib_SyncBatchNorm" in mx.registry
    assert mx.sym.contrib.SyncBatchNorm is not _native and mx.sym.contrib._sd_reference_SyncBatchNorm is _native
    # it is no flag of the plugin's install() and no entry of its tables
    assert "sync_bn" not in mxnet_plugin.FEATURE_FLAGS and "syncbn" not in mxnet_plugin.FEATURE_FLAGS
    assert not any("SyncBatchNorm" in op for f in mxnet_plugin._FEATURES.values() for op in f.ops)
    v = mx.sym.Variable
    out = mx.sym.contrib.SyncBatchNorm(data=v("d"), gamma=v("g"), beta=v("b"), moving_mean=v("mm"), moving_var=v("mv"),
                                       eps=1e-5, momentum=0.9, fix_gamma=False, ndev=8, key="bn1", name="bn1")
    assert out[0] == "out" and out[2] == 0                  # one visible output of the three-output node
    node = out[1]
    assert node.op_type == "sd__contrib_SyncBatchNorm" and node.nout == 3 and len(node.inputs) == 5
    assert node.params == {"eps": "1e-05", "momentum": "0.9", "fix_gamma": "False", "ndev": "8", "key": "bn1"}
    # output_mean_var: three visible outputs
    outs = mx.sym.contrib.SyncBatchNorm(v("d"), v("g"), v("b"), output_mean_var=True)
    assert [o[2] for o in outs] == [0, 1, 2] and outs[0][1].op_type == "sd__contrib_SyncBatchNorm"
    # positional data, the rest by keyword, no parameters
    node = mx.sym.contrib.SyncBatchNorm(v("d"), gamma=v("g"), beta=v("b"))[1]
    assert node.op_type == "sd__contrib_SyncBatchNorm" and node.params == {} and len(node.inputs) == 3
    with pytest.raises(TypeError, match="positionally and by keyword"):
        mx.sym.contrib.SyncBatchNorm(v("d"), data=v("d2"))
    assert sync_bn.fallbacks == []
    # use_global_stats=True, or a keyword the operator does not know: the native constructor, recorded
    got = mx.sym.contrib.SyncBatchNorm(data=v("d"), gamma=v("g"), beta=v("b"), use_global_stats=True, name="frozen")
    assert got[0] == "native SyncBatchNorm" and got[2]["use_global_stats"] is True and got[2]["name"] == "frozen"
    got = mx.sym.contrib.SyncBatchNorm(data=v("d"), axis=1)
    assert got[0] == "native SyncBatchNorm"
    assert [(f[0], f[1]) for f in sync_bn.fallbacks] == [("_contrib_SyncBatchNorm", "frozen"),
                                                         ("_contrib_SyncBatchNorm", None)]
    assert "use_global_stats" in sync_bn.fallbacks[0][2] and "'axis'" in sync_bn.fallbacks[1][2]
    # a second install() keeps the first one's original; uninstall() puts it back
    sync_bn.install(mx)
    assert mx.sym.contrib._sd_reference_SyncBatchNorm is _native
    sync_bn.uninstall(mx)
    assert mx.sym.contrib.SyncBatchNorm is _native and not hasattr(mx.sym.contrib, "_sd_reference_SyncBatchNorm")


def test_prop_mirrors_the_reference_operator(sbn):
    mx, props, _ = sbn
    P = props["_contrib_SyncBatchNorm"]
    p = P()
    # defaults: sync_batch_norm-inl.h:57-75
    assert p.p == dict(eps=1e-3, momentum=0.9, fix_gamma=True, use_global_stats=False, output_mean_var=False, ndev=1,
                       key="")
    assert p.list_arguments() == ["data", "gamma", "beta"]
    assert p.list_outputs() == ["output", "mean", "var"]
    assert p.list_auxiliary_states() == ["moving_mean", "moving_var"]
    assert p.num_visible_outputs == 1 and p.need_top_grad_ is True
    assert P(output_mean_var="True").num_visible_outputs == 3
    # InferShape (:556-574), 4-D and 2-D data
    assert p.infer_shape([(2, 256, 200, 336), (), ()]) == (
        [(2, 256, 200, 336), (256,), (256,)], [(2, 256, 200, 336), (256,), (256,)], [(256,), (256,)])
    assert p.infer_shape([(6, 5), (5,), (5,)]) == ([(6, 5), (5,), (5,)], [(6, 5), (5,), (5,)], [(5,), (5,)])
    with pytest.raises(ValueError, match="batch, channel"):
        p.infer_shape([(7,), (), ()])
    # InferType (:576-607): float16 data keeps float32 parameters and statistics
    assert p.infer_type([np.float16, None, None]) == (
        [np.float16, np.float32, np.float32], [np.float16, np.float32, np.float32], [np.float32, np.float32])
    assert p.infer_type([np.float32, None, None])[2] == [np.float32, np.float32]
    # DeclareBackwardDependency (:624-634)
    assert p.declare_backward_dependency(["dy", "dm", "dv"], ["x", "g", "b"], ["y", "m", "v"]) == ["dy", "m", "v", "x", "g"]
    # parameters arrive as strings
    q = P(eps="1e-5", momentum="0.99", fix_gamma="False", ndev="8", key="stage1_unit1_bn1")
    assert q.p["eps"] == 1e-5 and q.p["momentum"] == 0.99 and q.p["fix_gamma"] is False and q.p["ndev"] == 8
    assert P.sd_supports({"eps": "1e-5", "ndev": "8"}) == ""
    assert "use_global_stats" in P.sd_supports({"use_global_stats": "True"})
    assert "not one this operator takes" in P.sd_supports({"axis": "1"})
    with pytest.raises(ValueError, match="use_global_stats"):
        P(use_global_stats="True")
    with pytest.raises(ValueError, match="ndev"):
        P(ndev="0")


def test_alias_on_the_recording_stand_in():
    """the graph-recording mxnet of tests/ref_stubs.py: a normalizer_factory-style call site builds the device
    node, and the frozen form builds the native operator the graph held before"""
    from simpledet_amd import sync_bn
    mx = ref_stubs.make_mx()
    sync_bn.install(mx)
    try:
        d = mx.sym.var("data")
        g, b = mx.sym.var("bn_gamma"), mx.sym.var("bn_beta")
        mm, mv = mx.sym.var("bn_moving_mean"), mx.sym.var("bn_moving_var")
        y = mx.sym.contrib.SyncBatchNorm(data=d, gamma=g, beta=b, moving_mean=mm, moving_var=mv, eps=1e-5,
                                         momentum=0.9, fix_gamma=False, use_global_stats=False, ndev=8, key="bn",
                                         name="bn")
        node = ref_stubs.source(y)
        assert node.op_type == "sd__contrib_SyncBatchNorm" and node.nout == 3 and node.name == "bn"
        assert [i.name for i in node.inputs] == ["data", "bn_gamma", "bn_beta", "bn_moving_mean", "bn_moving_var"]
        for ns in (mx.sym.contrib, mx.contrib.symbol):
            frozen = ns.SyncBatchNorm(data=d, gamma=g, beta=b, use_global_stats=True, name="frozen")
            assert frozen.op_type == "SyncBatchNorm" and frozen.params["use_global_stats"] is True
        assert len(sync_bn.fallbacks) == 2
    finally:
        sync_bn.uninstall(mx)
    again = mx.sym.contrib.SyncBatchNorm(data=mx.sym.var("data"), ndev=8)
    assert again.op_type == "SyncBatchNorm" and not hasattr(mx.sym.contrib.SyncBatchNorm, "_sd_alias")


# ------------------------------------------------------------------------------------------ GPU --
def _run(mx, props, ops, shape, params, is_train=True, reqs=None, dtype=None):
    """forward and backward through the adapter -> the wrapped arrays"""
    import torch
    p = props["_contrib_SyncBatchNorm"](**params)
    ishape, oshape, ashape = p.infer_shape([shape, (), ()])
    dt = dtype or torch.float32
    op = p.create_operator(None, ishape, [np.float16 if dt == torch.float16 else np.float32])
    rs = np.random.RandomState(3)
    ins = [mx_stub.wrap(torch.from_numpy(rs.standard_normal(s).astype(F)).cuda()) for s in ishape]
    ins[0] = mx_stub.wrap(ins[0].t.to(dt))
    aux = [mx_stub.wrap(torch.from_numpy((rs.random_sample(s) + 0.5).astype(F)).cuda()) for s in ashape]
    outs = [mx_stub.wrap(torch.full(oshape[0], -7.5, device="cuda", dtype=dt))] + \
           [mx_stub.wrap(torch.full(s, -7.5, device="cuda")) for s in oshape[1:]]
    op.forward(is_train, ["write"] * 3, ins, outs, aux)
    return op, ins, aux, outs


@pytest.mark.gpu
@pytest.mark.parametrize("fix_gamma", [True, False])
def test_adapter_round_trip(sbn, ops, fix_gamma):
    import torch
    mx, props, _ = sbn
    shape = (4, 6, 10, 12)
    params = dict(eps="1e-3", momentum="0.9", fix_gamma=str(fix_gamma), ndev="1", key="k")
    rs = np.random.RandomState(4)
    op, ins, aux, outs = _run(mx, props, ops, shape, params)
    x, g, b = [i.t for i in ins]
    gamma_before = g.clone()
    aux_before = [a.t.clone() for a in aux]
    y, mean, var = ops.sync_batch_norm_forward(x, g, b, eps=1e-3, fix_gamma=fix_gamma)
    assert torch.equal(outs[0].t, y) and torch.equal(outs[1].t, mean) and torch.equal(outs[2].t, var)
    # nothing moves in the forward, and gamma is left alone (the reference stores ones into it under fix_gamma)
    assert torch.equal(aux[0].t, aux_before[0]) and torch.equal(aux[1].t, aux_before[1])
    assert torch.equal(g, gamma_before)
    dy = mx_stub.wrap(torch.from_numpy(rs.standard_normal(shape).astype(F)).cuda())
    grads = [mx_stub.wrap(torch.full(tuple(i.shape), float("nan"), device="cuda")) for i in ins]
    op.backward(["write"] * 3, [dy], ins, outs, grads, aux)
    mm, mv = aux_before[0].clone(), aux_before[1].clone()
    dx, dgamma, dbeta = ops.sync_batch_norm_backward(dy.t, x, mean, var, g, eps=1e-3, fix_gamma=fix_gamma,
                                                     moving_mean=mm, moving_var=mv, momentum=0.9)
    assert torch.equal(grads[0].t, dx) and torch.equal(grads[1].t, dgamma) and torch.equal(grads[2].t, dbeta)
    # the moving statistics move in the backward, by the contract's rule
    assert torch.equal(aux[0].t, mm) and torch.equal(aux[1].t, mv) and not torch.equal(mm, aux_before[0])
    one = F(F(1.0) - F(0.9))
    want = (aux_before[0].cpu().numpy() * F(0.9) + mean.cpu().numpy() * one).astype(F)
    assert np.array_equal(aux[0].t.cpu().numpy(), want)
    assert torch.equal(g, gamma_before)
    if fix_gamma:
        assert torch.all(grads[1].t == 0)
    else:
        assert torch.any(grads[1].t != 0)
    # kAddTo is refused, on outputs and on gradients
    with pytest.raises(RuntimeError, match="add"):
        op.forward(True, ["add", "write", "write"], ins, outs, aux)
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["add", "write", "write"], [dy], ins, outs, grads, aux)
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["write", "write", "add"], [dy], ins, outs, grads, aux)
    # a frozen input (req null) still moves the statistics and writes the parameter gradients
    before = aux[0].t.clone()
    grads2 = [mx_stub.wrap(torch.full(tuple(i.shape), float("nan"), device="cuda")) for i in ins]
    op.backward(["null", "write", "write"], [dy], ins, outs, grads2, aux)
    assert torch.isnan(grads2[0].t).all() and torch.equal(grads2[2].t, dbeta) and not torch.equal(aux[0].t, before)


@pytest.mark.gpu
def test_adapter_inference_half_data_and_ndev_mismatch(sbn, ops):
    import torch
    mx, props, _ = sbn
    shape = (2, 8, 6, 8)
    # inference: the scale-shift of the moving statistics; mean / var outputs are left alone
    op, ins, aux, outs = _run(mx, props, ops, shape, dict(fix_gamma="False"), is_train=False)
    want = ops.sync_bn_infer_forward(ins[0].t, ins[1].t, ins[2].t, aux[0].t, aux[1].t, 1e-3, False)
    assert torch.equal(outs[0].t, want) and torch.all(outs[1].t == -7.5) and torch.all(outs[2].t == -7.5)
    # float16 data: the _f16 entry points, float32 statistics
    op, ins, aux, outs = _run(mx, props, ops, shape, dict(fix_gamma="False"), dtype=torch.float16)
    y, mean, var = ops.sync_batch_norm_forward(ins[0].t, ins[1].t, ins[2].t, eps=1e-3, fix_gamma=False)
    assert outs[0].t.dtype == torch.float16 and torch.equal(outs[0].t, y) and torch.equal(outs[1].t, mean)
    # ndev > 1 without a process group of that size is refused loudly
    with pytest.raises(RuntimeError, match="ndev=8"):
        _run(mx, props, ops, shape, dict(ndev="8"))
