"""`se_block.install(mx)` + `patch_builders()`: the SE-ResNet mask config and an EfficientNet config of the reference
build with every se() site an `sd_se_block` node over `<prefix>_fc1_weight` / `<prefix>_fc2_weight`, no
mean / broadcast_mul of a site is left, unpatch_builders() restores both modules' `se`, and kAddTo is refused.  CPU on
the stand-ins of tests/ref_stubs.py and tests/mx_stub.py; the first test skips where the reference tree is absent."""
import importlib
import os

import pytest

from . import mx_stub, ref_stubs as RS

REF = "/root/reference"
CONFIGS = ("config.se.mask_se-r50v1b_fpn_bn_scratch_2x", "config.efficientnet.efficientnet_b5_fpn_bn_scratch_400_6x")


def _graph(mod):
    nodes = {}
    for is_train in (True, False):
        for o in importlib.import_module(mod).get_config(is_train):
            for attr in ("train_symbol", "test_symbol", "rpn_test_symbol"):
                if isinstance(getattr(o, attr, None), RS.Symbol):
                    RS.walk(getattr(o, attr), nodes)
    return list(nodes.values())


def _ops(nodes, op):
    return [n for n in nodes if n.op_type == op]


@pytest.mark.skipif(not os.path.isdir(REF), reason="/root/reference not present")
@pytest.mark.parametrize("mod", CONFIGS)
def test_every_se_site_becomes_one_node_and_unpatch_restores(mod):
    from simpledet_amd import se_block
    with RS.reference_modules():
        eff, sem = (importlib.import_module(m) for m in se_block.BUILDERS)
        reference_se, prefixes = eff.se, []
        assert sem.se is reference_se
        eff.se = sem.se = lambda input, prefix, f_down, f_up: (prefixes.append(prefix),
                                                               reference_se(input, prefix, f_down, f_up))[1]
        before = _graph(mod)
    sites = len(prefixes)                    # the train and the test symbol build each site once
    assert len(set(prefixes)) == (20 if "mask" in mod else 39) and len(_ops(before, "broadcast_mul")) == sites
    with RS.reference_modules() as R:
        eff, sem = (importlib.import_module(m) for m in se_block.BUILDERS)
        reference_se = eff.se
        se_block.install(R.mx)
        assert se_block.patch_builders() == 2 and eff.se is not reference_se and sem.se is not reference_se
        after = _graph(mod)
        nodes = _ops(after, "sd_se_block")
        assert len(nodes) == sites and not _ops(after, "broadcast_mul") and not se_block.fallbacks
        assert len(_ops(after, "mean")) == len(_ops(before, "mean")) - 2 * sites
        names = {i.name for n in nodes for i in n.inputs if i.op_type == "var"}
        assert names == {p + s for p in prefixes for s in ("_fc1_weight", "_fc2_weight")}      # no bias by default
        for n in nodes:
            w1, w2 = n.inputs[1], n.inputs[2]
            Cr, C = w1.params["shape"][:2]
            assert n.nout == 4 and n.params == {"num_hidden": str(Cr), "no_bias": "True"}
            assert w1.params["shape"] == (Cr, C, 1, 1) and w2.params["shape"] == (C, Cr, 1, 1)
        assert se_block.unpatch_builders() == 2 and eff.se is reference_se and sem.se is reference_se
        assert not hasattr(eff, "_sd_reference_se") and se_block.unpatch_builders() == 0


def test_prop_shapes_biases_limits_and_kaddto():
    from simpledet_amd import mxnet_plugin, se_block
    mx = mx_stub.make_stub()
    P = se_block.install(mx)["se_block"]
    assert "sd_se_block" in mx.registry and "se_block" not in mxnet_plugin.FEATURE_FLAGS
    p = P(num_hidden="16")
    assert p.list_arguments() == ["data", "fc1_weight", "fc2_weight"] and p.num_visible_outputs == 1
    assert p.list_outputs() == ["output", "gap", "z1", "a"]
    assert p.infer_shape([(2, 64, 200, 334), (), ()]) == (
        [(2, 64, 200, 334), (16, 64, 1, 1), (64, 16, 1, 1)], [(2, 64, 200, 334), (2, 64), (2, 16), (2, 64)], [])
    assert P(num_hidden="16", no_bias="False").list_arguments()[3:] == ["fc1_bias", "fc2_bias"]
    with pytest.raises(ValueError, match="num_hidden"):
        P(num_hidden="513")
    op = p.create_operator(None, None, [None])
    with pytest.raises(RuntimeError, match="add"):
        op.forward(True, ["add"] * 4, [], [], [])
    with pytest.raises(RuntimeError, match="kWriteTo"):
        op.backward(["add", "write", "write"], [], [], [], [], [])
    se_block._own["installed"] = False
    with pytest.raises(RuntimeError, match="install"):
        se_block.patch_builders(modules=[])
