"""`install(mx, quant_int8=True)`: `mx.sym.contrib.Quantization_int8` builds an `sd__contrib_Quantization_int8`
Custom node with the reference's argument, output, auxiliary state, defaults and shape inference
(quantization_int8-inl.h:85-100 and the Prop class); without the flag the graph holds what it held.  CPU only, on
tests/mx_stub.py (its Custom already takes the auxiliary state as a keyword Symbol); the GPU round trip through
the adapter is the last test."""
import numpy as np
import pytest

from . import mx_stub
from . import quant_int8_ref as qr

F = np.float32
NAME = "_contrib_Quantization_int8"
# utils/graph_optimize.py: the attribute dicts attach_quantize_node hands over (config/int8/)
ACT_ATTRS = {"delay_quant": 0, "ema_decay": 0.99, "grad_mode": "ste", "is_weight": False,
             "is_weight_perchannel": False, "quant_mode": "minmax"}
WEIGHT_ATTRS = {"delay_quant": 0, "ema_decay": 0.99, "grad_mode": "ste", "is_weight": True,
                "is_weight_perchannel": False, "quant_mode": "minmax"}


def _native(*a, **kw):
    return ("native Quantization_int8", a, kw)


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mx.sym.contrib.Quantization_int8 = _native      # what a SimpleDet build of MXNet registers natively
    mxnet_plugin._state.update(registered=False)
    props = mxnet_plugin.install(mx, **flags)
    return mx, props, mxnet_plugin


@pytest.fixture()
def q_plugin():
    mx, props, mxnet_plugin = _fresh(quant_int8=True)
    yield mx, props, mxnet_plugin
    mxnet_plugin._state.update(registered=False)


def test_default_install_registers_nothing_new_and_leaves_the_constructor_alone():
    mx, props, mxnet_plugin = _fresh()
    try:
        assert NAME not in props and "sd_" + NAME not in mx.registry
        assert mx.sym.contrib.Quantization_int8 is _native
        v = mx.sym.Variable
        assert mx.sym.contrib.Quantization_int8(data=v("d"), minmax=v("m"), **ACT_ATTRS)[0].startswith("native")
        assert not hasattr(mx.sym.contrib, "_sd_reference_Quantization_int8")
        mx2, props2, _ = _fresh(**{f: True for f in mxnet_plugin.FEATURE_FLAGS if f != "quant_int8"})
        assert NAME not in props2 and mx2.sym.contrib.Quantization_int8 is _native
    finally:
        mxnet_plugin._state.update(registered=False)


def test_the_flag_installs_the_constructor_and_a_default_install_restores_it():
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mx.sym.contrib.Quantization_int8 = _native
    try:
        mxnet_plugin._state.update(registered=False)
        props = mxnet_plugin.install(mx, quant_int8=True)
        assert NAME in props and "sd_" + NAME in mx.registry
        assert mx.sym.contrib.Quantization_int8 is not _native
        assert mx.sym.contrib._sd_reference_Quantization_int8 is _native
        mxnet_plugin._state.update(registered=False)
        props = mxnet_plugin.install(mx)
        assert NAME not in props
        assert mx.sym.contrib.Quantization_int8 is _native
        assert not hasattr(mx.sym.contrib, "_sd_reference_Quantization_int8")
    finally:
        mxnet_plugin._state.update(registered=False)


def test_the_three_call_shapes_of_graph_optimize_build_one_device_node(q_plugin):
    mx, props, mxnet_plugin = q_plugin
    v = mx.sym.Variable
    d, m, w, wm, p = v("data"), v("data_minmax"), v("weight"), v("weight_minmax"), v("pool")
    # :162 data=, minmax=, the activation attributes; :169 the same for a weight; :182 positional, no minmax
    act = mx.sym.contrib.Quantization_int8(data=d, minmax=m, **ACT_ATTRS, name="data")
    wgt = mx.sym.contrib.Quantization_int8(data=w, minmax=wm, **WEIGHT_ATTRS, name="weight")
    pos = mx.sym.contrib.Quantization_int8(p, **ACT_ATTRS, name="pool")
    for node, inputs, attrs in ((act, [d, m], ACT_ATTRS), (wgt, [w, wm], WEIGHT_ATTRS), (pos, [p], ACT_ATTRS)):
        assert node.op_type == "sd_" + NAME and node.nout == 1
        assert node.inputs == inputs
        # the keyword strings MXNet's front end would send
        assert node.params == {k: (repr(x) if isinstance(x, float) else str(x)) for k, x in attrs.items()}
    assert act.params["is_weight"] == "False" and wgt.params["is_weight"] == "True"
    assert act.params["ema_decay"] == "0.99" and act.params["quant_mode"] == "minmax"
    assert mxnet_plugin._state["fallbacks"] == []


def test_prop_arguments_outputs_aux_shapes_and_defaults(q_plugin):
    mx, props, _ = q_plugin
    prop = props[NAME]()
    assert prop.list_arguments() == ["data"]
    assert prop.list_outputs() == ["output"]
    assert prop.list_auxiliary_states() == ["minmax"]
    assert prop.need_top_grad_ is True
    # quantization_int8-inl.h:85-100
    assert prop.q == dict(quant_mode="minmax", is_weight=True, is_weight_perchannel=False, delay_quant=0,
                          ema_decay=0.99, grad_mode="ste", fix_act_scale=False)
    for shape in ((2, 3, 5, 7), (6, 11)):
        assert prop.infer_shape([shape]) == ([shape], [shape], [(1,)])
    for shape in ((4,), (2, 3, 4), (1, 2, 3, 4, 5)):
        with pytest.raises(ValueError):
            prop.infer_shape([shape])
    p = props[NAME](**{k: str(x) for k, x in dict(ACT_ATTRS, fix_act_scale=True, delay_quant=3).items()})
    assert p.q["is_weight"] is False and p.q["fix_act_scale"] is True and p.q["delay_quant"] == 3
    op = p.create_operator("gpu(0)", [(2, 3, 5, 7)], ["float32"])
    assert op.q is p.q and op.state is None          # the device state is made on the first forward
    assert p.declare_backward_dependency([10], [20], [30]) == [10, 20]


def test_unsupported_parameter_sets_fall_back_to_the_native_constructor(q_plugin):
    mx, props, mxnet_plugin = q_plugin
    v = mx.sym.Variable
    cases = (dict(WEIGHT_ATTRS, is_weight_perchannel=True), dict(ACT_ATTRS, quant_mode="power2"),
             dict(ACT_ATTRS, grad_mode="other"))
    for i, attrs in enumerate(cases):
        node = mx.sym.contrib.Quantization_int8(data=v("d"), minmax=v("m"), **attrs, name="n%d" % i)
        assert node[0] == "native Quantization_int8" and node[2]["name"] == "n%d" % i
        assert node[2]["quant_mode"] == attrs["quant_mode"]
        with pytest.raises(ValueError):
            props[NAME](**{k: str(x) for k, x in attrs.items()})
    assert [(f[0], f[1]) for f in mxnet_plugin._state["fallbacks"]] == [(NAME, "n0"), (NAME, "n1"), (NAME, "n2")]
    # an activation's per-channel flag is not looked at by the reference either
    node = mx.sym.contrib.Quantization_int8(v("d"), **dict(ACT_ATTRS, is_weight_perchannel=True))
    assert node.op_type == "sd_" + NAME


@pytest.mark.gpu
def test_adapter_round_trip_two_training_steps_and_one_eval():
    import torch
    mx, props, mxnet_plugin = _fresh(quant_int8=True, stream=lambda: torch.cuda.current_stream().cuda_stream)
    try:
        rng = np.random.RandomState(5)
        for attrs, grad_mode in ((ACT_ATTRS, "clip"), (WEIGHT_ATTRS, "ste")):
            attrs = dict(attrs, grad_mode=grad_mode, delay_quant=1 if not attrs["is_weight"] else 0)
            prop = props[NAME](**{k: str(x) for k, x in attrs.items()})
            op = prop.create_operator("gpu(0)", [(2, 3, 5, 7)], ["float32"])
            ref = qr.QuantInt8Ref(is_weight=attrs["is_weight"], delay_quant=attrs["delay_quant"],
                                  ema_decay=attrs["ema_decay"], grad_mode=grad_mode)
            aux = [mx_stub.wrap(torch.zeros(1, device="cuda"))]
            for step, is_train in enumerate((True, True, True, False)):
                x = (rng.standard_normal((2, 3, 5, 7)) * (step + 1)).astype(F)
                g = rng.standard_normal((2, 3, 5, 7)).astype(F)
                xd, out = mx_stub.wrap(torch.from_numpy(x).cuda()), mx_stub.wrap(torch.empty(2, 3, 5, 7, device="cuda"))
                op.forward(is_train, ["write"], [xd], [out], aux)
                want = ref.forward(x.ravel(), is_train=is_train)
                assert (out.t.cpu().numpy().ravel().view(np.uint32) == want.view(np.uint32)).all()
                assert aux[0].t.cpu().numpy().view(np.uint32)[0] == np.array([ref.minmax]).view(np.uint32)[0]
                assert op.state.t.cpu().tolist() == ref.state
                if is_train:
                    dx = mx_stub.wrap(torch.full((2, 3, 5, 7), 2.0, device="cuda"))
                    op.backward(["add"], [mx_stub.wrap(torch.from_numpy(g).cuda())], [xd], [out], [dx], aux)
                    wantg = (F(2.0) + ref.backward(g.ravel(), x.ravel())).astype(F)
                    assert (dx.t.cpu().numpy().ravel().view(np.uint32) == wantg.view(np.uint32)).all()
    finally:
        mxnet_plugin._state.update(registered=False)
