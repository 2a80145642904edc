"""`install(mx, group_norm=True)`: `mx.sym.contrib.GroupNorm` builds an `sd__contrib_GroupNorm` Custom node with
the reference's arguments, outputs, visible count, defaults and shape inference (group_norm-inl.h:70-77,185-237);
without the flag the graph holds what it held.  CPU only, on tests/mx_stub.py; the GPU round trip through the
adapter is the last test."""
import types

import numpy as np
import pytest

from . import mx_stub


def _native(*a, **kw):
    return ("native GroupNorm", a, kw)


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mx.sym.contrib.GroupNorm = _native           # what a SimpleDet build of MXNet registers natively
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def gn_plugin():
    mx, props, mxnet_plugin = _fresh(group_norm=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_nothing_new_and_leaves_the_graph_alone():
    mx, props, mxnet_plugin = _fresh()
    try:
        assert "_contrib_GroupNorm" not in props and "sd__contrib_GroupNorm" not in mx.registry
        assert mx.sym.contrib.GroupNorm is _native
        v = mx.sym.Variable
        node = mx.sym.contrib.GroupNorm(data=v("d"), gamma=v("g"), beta=v("b"), num_group=32)
        assert node[0] == "native GroupNorm"
        assert not hasattr(mx.sym.contrib, "_sd_reference_GroupNorm")
        # the other opt-in flags do not bring it in either
        mx2, props2, _ = _fresh(**{f: True for f in mxnet_plugin.FEATURE_FLAGS if f != "group_norm"})
        assert "_contrib_GroupNorm" not in props2 and mx2.sym.contrib.GroupNorm is _native
        # an mxnext-level wrapper is left alone without the flag
        X = types.SimpleNamespace(group_norm=_native)
        mxnet_plugin.patch_mxnext(X, mx2)
        assert X.group_norm is _native and "group_norm" not in mxnet_plugin._state["mxnext_probe"]
    finally:
        mxnet_plugin._state.update(registered=False)


def test_with_the_flag_the_node_is_the_device_op(gn_plugin):
    mx, props, mxnet_plugin = gn_plugin
    assert "_contrib_GroupNorm" in props and "sd__contrib_GroupNorm" in mx.registry
    assert mx.sym.contrib.GroupNorm is not _native and mx.sym.contrib._sd_reference_GroupNorm is _native
    v = mx.sym.Variable
    out = mx.sym.contrib.GroupNorm(data=v("d"), gamma=v("g"), beta=v("b"), num_group=32, eps=1e-5, name="gn1")
    # one visible output: the alias returns output 0 of the three-output node
    assert out[0] == "out" and out[2] == 0
    node = out[1]
    assert node.op_type == "sd__contrib_GroupNorm" and node.nout == 3 and len(node.inputs) == 3
    assert node.params == {"num_group": "32", "eps": "1e-05"}
    # positional data, keyword parameters, no explicit num_group
    node = mx.sym.contrib.GroupNorm(v("d"), gamma=v("g"), beta=v("b"))[1]
    assert node.op_type == "sd__contrib_GroupNorm" and node.params == {}
    # the mxnext-level binding, where there is one
    X = types.SimpleNamespace(group_norm=_native)
    done = mxnet_plugin.patch_mxnext(X, mx)
    assert "mxnext.group_norm" in done and X._sd_reference_group_norm is _native
    node = X.group_norm(data=v("d"), gamma=v("g"), beta=v("b"), num_group=8)[1]
    assert node.op_type == "sd__contrib_GroupNorm" and node.params == {"num_group": "8"}
    # a default install() afterwards puts both back
    mxnet_plugin._state.update(registered=False)
    mxnet_plugin.install(mx)
    mxnet_plugin.patch_mxnext(X, mx)
    assert X.group_norm is _native


def test_prop_mirrors_the_reference_operator(gn_plugin):
    mx, props, _ = gn_plugin
    P = props["_contrib_GroupNorm"]
    p = P()
    assert p.g == {"num_group": 32, "eps": 1e-5}                     # group_norm-inl.h:70-77
    assert p.list_arguments() == ["data", "gamma", "beta"]
    assert p.list_outputs() == ["output", "mean", "var"]
    assert p.num_visible_outputs == 1 and p.need_top_grad_ is True
    # InferShape (:185-202): gamma / beta (C,), mean / var DECLARED (N, C) although N * G floats are written
    assert p.infer_shape([(2, 256, 200, 336), (), ()]) == (
        [(2, 256, 200, 336), (256,), (256,)], [(2, 256, 200, 336), (2, 256), (2, 256)])
    # DeclareBackwardDependency (:211-220)
    assert p.declare_backward_dependency(["dy"], ["x", "g", "b"], ["y", "mu", "rsig"]) == ["dy", "mu", "rsig", "x", "g"]
    # parameters arrive as strings
    q = P(num_group="8", eps="0.001")
    assert q.g == {"num_group": 8, "eps": 0.001}
    assert q.infer_shape([(1024, 256, 7, 7), (256,), (256,)])[1][1] == (1024, 256)
    # a bad num_group: C not divisible, or not positive
    with pytest.raises(ValueError, match="not divisible"):
        P(num_group="32").infer_shape([(2, 48, 7, 7), (), ()])
    with pytest.raises(ValueError, match="positive"):
        P(num_group="0")
    with pytest.raises(ValueError):
        P(num_group="many")


@pytest.mark.gpu
def test_adapter_round_trip_fills_the_first_ng_floats(gn_plugin, ops):
    import torch
    mx, props, _ = gn_plugin
    N, C, G = 4, 32, 8
    p = props["_contrib_GroupNorm"](num_group=str(G), eps="1e-5")
    (ishape, oshape) = p.infer_shape([(N, C, 14, 14), (), ()])[:2]
    op = p.create_operator(None, ishape, None)
    rs = np.random.RandomState(3)
    ins = [mx_stub.wrap(torch.from_numpy(rs.standard_normal(s).astype(np.float32)).cuda()) for s in ishape]
    outs = [mx_stub.wrap(torch.full(s, -7.5, device="cuda")) for s in oshape]
    op.forward(True, ["write"] * 3, ins, outs, [])
    y, mu, rsig = ops.group_norm_forward(ins[0].t, ins[1].t, ins[2].t, G, 1e-5)
    assert torch.equal(outs[0].t, y)
    for o, want in ((outs[1].t, mu), (outs[2].t, rsig)):
        assert o.shape == (N, C) and torch.equal(o.reshape(-1)[:N * G], want.reshape(-1))
        assert torch.all(o.reshape(-1)[N * G:] == -7.5)              # the tail of the (N, C) buffer is untouched
    dy = mx_stub.wrap(torch.randn(N, C, 14, 14, device="cuda"))
    grads = [mx_stub.wrap(torch.full(s, float("nan"), device="cuda")) for s in ishape]
    op.backward(["write"] * 3, [dy], ins, outs, grads, [])
    dx, dgamma, dbeta = ops.group_norm_backward(dy.t, ins[0].t, mu, rsig, ins[1].t, G)
    assert torch.equal(grads[0].t, dx) and torch.equal(grads[1].t, dgamma) and torch.equal(grads[2].t, dbeta)
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["add", "write", "write"], [dy], ins, outs, grads, [])
