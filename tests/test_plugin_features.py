"""The table that drives the adapter's opt-in features (`mxnet_plugin._FEATURES`) and the one rebind / restore behind
every `patch_*` / `unpatch_*` pair, on tests/mx_stub.py and a `types.SimpleNamespace` standing for a builder module.
What each feature's methods emit is the subject of its own tests/test_*_plugin.py.  CPU only."""
import importlib
import os
import types
from unittest import mock

import pytest

from . import mx_stub

FLAGS = ("retina", "proposal", "bbox_post", "retina_loss", "group_norm", "mask_loss", "quant_int8", "fcos",
         "fcos_decode", "tsd_pool", "reppoints", "msrcnn", "reppoints_decode", "crowdhuman")
PAIRS = {"bbox_post": "bbox_post", "mask_loss": "mask_loss", "fcos": "fcos_loss", "fcos_decode": "fcos_decode",
         "tsd_pool": "tsd_pool", "reppoints": "reppoints_loss", "msrcnn": "msrcnn_loss",
         "reppoints_decode": "reppoints_decode", "crowdhuman": "crowdhuman"}


def _fresh(**flags):
    from simpledet_amd import mxnet_plugin
    mx = mx_stub.make_stub()
    mxnet_plugin._state.update(registered=False)
    mxnet_plugin.install(mx, **flags)
    return mx, mxnet_plugin


def test_the_flags_and_an_unknown_one():
    from simpledet_amd import mxnet_plugin as plug
    assert plug.FEATURE_FLAGS == FLAGS and tuple(plug._FEATURES) == FLAGS
    assert sorted(f for f in FLAGS if plug._FEATURES[f].builders) == sorted(PAIRS)
    mx = mx_stub.make_stub()
    try:
        for call in (plug.install, plug.register):
            with pytest.raises(TypeError, match="no_such_flag") as e:
                call(mx, no_such_flag=True)
            assert all(f in str(e.value) for f in FLAGS)
        # every flag gates operators that a default install() leaves out and `flag=True` brings in
        plug._state.update(registered=False)
        default = plug.install(mx)
        everything = set(plug._state["all_ops"])
        gated = [name for f in FLAGS for name in plug._FEATURES[f].ops]
        assert len(gated) == len(set(gated)) and set(gated) == everything - set(default)
        for f in FLAGS:
            plug._state.update(registered=False)
            stub = mx_stub.make_stub()
            assert set(plug.install(stub, **{f: True})) - set(default) == set(plug._FEATURES[f].ops)
            assert all("sd_" + name in stub.registry for name in plug._FEATURES[f].ops)
    finally:
        plug._state.update(registered=False)


@pytest.mark.parametrize("flag", sorted(PAIRS))
def test_rebind_and_restore(flag):
    mx, plug = _fresh()
    try:
        feature = plug._FEATURES[flag]
        patch, unpatch = getattr(plug, "patch_" + PAIRS[flag]), getattr(plug, "unpatch_" + PAIRS[flag])
        calls = []

        def original(name):
            def method(self, *a, **k):
                calls.append(name)
                return name
            return method
        classes = {}
        for c, m in feature.methods:
            classes.setdefault(c, {})[m] = original(c + "." + m)
        reference = {c: dict(ms) for c, ms in classes.items()}
        # (`p`: the parameter object a head reads before it decides; any attribute will do here)
        mod = types.SimpleNamespace(**{c: type(c, (), dict(ms, p=mock.MagicMock())) for c, ms in classes.items()})
        held = lambda: {c: {m: getattr(mod, c).__dict__[m] for m in ms} for c, ms in reference.items()}
        saved = lambda: {c: {m: getattr(mod, c).__dict__.get("_sd_reference_" + m) for m in ms}
                         for c, ms in reference.items()}

        assert patch(mod, mx) is True
        assert saved() == reference
        first = held()
        for c, m in feature.methods:
            assert first[c][m] is not reference[c][m] and first[c][m].__name__ == m
        # the operators are not registered (a default install): a call goes to the reference's method
        c, m = feature.methods[-1]
        before = len(plug._state["fallbacks"])
        assert getattr(getattr(mod, c)(), m)(*range(first[c][m].__code__.co_argcount - 1)) == c + "." + m
        assert calls == [c + "." + m] and len(plug._state["fallbacks"]) == before + 1
        assert plug._state["fallbacks"][-1][0] in feature.ops and "not registered" in plug._state["fallbacks"][-1][2]
        # a second rebind keeps the first originals
        assert patch(mod, mx) is True
        assert saved() == reference and all(held()[c][m] is not reference[c][m] for c, m in feature.methods)
        # restore: the reference's methods, nothing saved, and nothing to do the second time
        assert unpatch(mod) is True
        assert held() == reference
        assert not [k for c in reference for k in getattr(mod, c).__dict__ if k.startswith("_sd_reference_")]
        assert unpatch(mod) is False and held() == reference
        # a module without the classes: nothing is rebound or restored
        assert patch(types.SimpleNamespace(), mx) is False and unpatch(types.SimpleNamespace()) is False
        if len(classes) > 1:          # one class missing: the others stay untouched
            partial = types.SimpleNamespace(**{c: getattr(mod, c) for c in list(classes)[1:]})
            assert patch(partial, mx) is False and held() == reference
    finally:
        plug._state.update(registered=False)


@pytest.mark.skipif(not os.path.isdir("/root/reference"), reason="/root/reference not present")
def test_a_default_install_leaves_the_reference_classes_as_they_were():
    """install(every flag) and then install(): every builder class holds the reference's own methods and no
    `_sd_reference_*` attribute, over the real builder modules"""
    from . import ref_stubs as RS
    with RS.reference_modules() as R:
        from simpledet_amd import mxnet_plugin as plug
        try:
            spots = [(importlib.import_module(b), c, m) for f in PAIRS for b in plug._FEATURES[f].builders
                     for c, m in plug._FEATURES[f].methods]
            reference = [getattr(mod, c).__dict__[m] for mod, c, m in spots]
            plug._state.update(registered=False)
            plug.install(R.mx, **{f: True for f in FLAGS})
            assert all(plug._state[plug._FEATURES[f].state] is True for f in PAIRS) and not plug._state["fallbacks"]
            assert [getattr(mod, c).__dict__["_sd_reference_" + m] for mod, c, m in spots] == reference
            assert all(getattr(mod, c).__dict__[m] is not ref for (mod, c, m), ref in zip(spots, reference))
            plug._state.update(registered=False)
            plug.install(R.mx)
            assert [getattr(mod, c).__dict__[m] for mod, c, m in spots] == reference
            assert not [k for mod, c, _ in spots for k in getattr(mod, c).__dict__ if k.startswith("_sd_reference_")]
            assert all(plug._state[plug._FEATURES[f].state] is False for f in PAIRS)
        finally:
            plug._state.update(registered=False)


def test_import_rule(monkeypatch):
    """a builder that is not there is None; one that breaks on import raises, unless the entry is lenient"""
    import sys
    from simpledet_amd import mxnet_plugin as plug
    assert plug._import_builder("sd_no_such_package.builder") is None
    pkg = types.ModuleType("sd_test_pkg")
    pkg.__path__ = []
    monkeypatch.setitem(sys.modules, "sd_test_pkg", pkg)
    assert plug._import_builder("sd_test_pkg.builder") is None

    class Finder:
        """sd_test_pkg.needs_dep imports a module that does not exist; sd_test_pkg.broken raises"""
        @staticmethod
        def find_spec(name, path=None, target=None):
            import importlib.machinery
            if name in ("sd_test_pkg.needs_dep", "sd_test_pkg.broken"):
                return importlib.machinery.ModuleSpec(name, Finder)
            return None

        @staticmethod
        def create_module(spec):
            return None

        @staticmethod
        def exec_module(module):
            if module.__name__.endswith("needs_dep"):
                import sd_no_such_dependency  # noqa: F401
            raise RuntimeError("broken builder")
    monkeypatch.setattr(sys, "meta_path", [Finder] + sys.meta_path)
    with pytest.raises(ModuleNotFoundError):
        plug._import_builder("sd_test_pkg.needs_dep")
    with pytest.raises(RuntimeError):
        plug._import_builder("sd_test_pkg.broken")
    assert plug._import_builder("sd_test_pkg.needs_dep", lenient=True) is None
    assert plug._import_builder("sd_test_pkg.broken", lenient=True) is None
    assert [f for f in FLAGS if plug._FEATURES[f].lenient] == ["bbox_post"]
