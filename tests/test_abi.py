"""CPU-only checks of the drop-in boundary: the shared library loads, exports every symbol that
include/simpledet_ops.h declares, and validates arguments without touching a GPU."""
import ctypes
import os

import pytest

from simpledet_amd import _lib


def test_header_parses_and_library_exports_every_symbol():
    protos = _lib.parse_header()
    assert len(protos) >= 20
    l = _lib.lib()
    for name in protos:
        assert hasattr(l.cdll, name), name
    # layout / size contracts are versioned too: library and header must agree exactly
    assert l.cdll.sd_abi_version() == _lib.header_abi_version() >= 3


def test_argument_validation_needs_no_gpu():
    l = _lib.lib()
    with pytest.raises(_lib.SimpleDetOpsError, match="pooled_size"):
        l.call("sd_roi_align_v2_fwd", None, None, None, None, None, 1, 1, 4, 4, 1, 0, 7, 0.5, None)
    with pytest.raises(_lib.SimpleDetOpsError, match="kWriteInplace"):
        l.call("sd_roi_align_v2_bwd", None, None, None, None, None, None, 2, 1, 1, 1, 4, 4, 1, 7, 7,
               0.5, None)
    with pytest.raises(_lib.SimpleDetOpsError, match="unknown tuning key"):
        l.call("sd_set_tuning", b"no_such_knob", 1)
    with pytest.raises(_lib.SimpleDetOpsError, match="method"):
        l.call("sd_soft_nms_batched", None, None, 1, 10, 0.5, 0.3, 0.001, 7, None, None, None, None)
    # empty problems are accepted without touching the device
    assert l.call("sd_nms", None, 0, 0, -1, 10, 0.5, 0, 0, None, None, None, None, 0, None) == 0
    assert l.call("sd_gen_anchor", None, 0, 0, 16, (ctypes.c_double * 1)(8.0), 1,
                  (ctypes.c_double * 1)(1.0), 1, None) == 0


class _RecordingLib:
    """Stands in for the loaded library: every attribute is a function that keeps the arguments of its last call
    and returns 0, and takes the restype / argtypes the binding sets on it."""

    class _Fn:
        def __init__(self):
            self.args = None

        def __call__(self, *args):
            self.args = args
            return 0

    def __getattr__(self, name):
        fn = self.__dict__[name] = self._Fn()
        return fn


@pytest.fixture()
def recorded():
    """(_Lib bound to a recording stand-in through the real header's prototypes, the stand-in)"""
    fake = _RecordingLib()
    return _lib._Lib(cdll=fake), fake


def test_marshaller_converts_by_the_headers_parameter_types(recorded):
    import numpy as np
    import torch

    l, fake = recorded
    # int sd_roi_pool_v1_fwd(data, rois, out, maxidx, B, C, H, W, K, pooled_h, pooled_w, float spatial_scale, stream)
    t = torch.zeros(4)
    raw = ctypes.c_void_p(1234)
    arr = (ctypes.c_int * 2)(3, 4)
    ref = ctypes.byref(ctypes.c_int(5))
    assert l.call("sd_roi_pool_v1_fwd", t, None, raw, arr, 1, np.int64(2), True, ctypes.c_int(7), 1, 7, 7, 1, ref) == 0
    got = fake.sd_roi_pool_v1_fwd.args
    assert type(got[0]) is int and got[0] == t.data_ptr()       # a tensor becomes its address
    assert got[1] is None                                       # None stays a null
    assert got[2] is raw and got[3] is arr and got[12] is ref   # ctypes values pass through untouched
    assert got[4] == 1 and type(got[4]) is int
    assert got[5] == 2 and type(got[5]) is int                  # numpy integers through __index__
    assert got[6] == 1 and type(got[6]) is int                  # and bools
    assert isinstance(got[7], ctypes.c_int) and got[7].value == 7
    assert got[11] == 1.0 and type(got[11]) is float            # a float slot receives a float
    assert fake.sd_roi_pool_v1_fwd.argtypes[11] is ctypes.c_float
    l.call("sd_roi_pool_v1_fwd", t, t, t, t, 1, 2, 3, 4, 1, 7, 7, np.float32(0.25), None)
    assert fake.sd_roi_pool_v1_fwd.args[11] == 0.25 and type(fake.sd_roi_pool_v1_fwd.args[11]) is float
    with pytest.raises(TypeError):                              # an integer slot refuses a float
        l.call("sd_roi_pool_v1_fwd", t, t, t, t, 1, 2, 3, 4, 7.5, 7, 7, 0.25, None)
    # const char* passes through; a size query has its return type from the header like everything else
    l.call("sd_set_tuning", b"knob", np.int32(1))
    assert fake.sd_set_tuning.args == (b"knob", 1)
    assert fake.sd_nms_workspace_bytes.restype is ctypes.c_size_t


def test_marshaller_refuses_a_wrong_argument_count_by_name(recorded):
    l, fake = recorded
    for args in ((None,) * 12, (None,) * 14):
        with pytest.raises(TypeError, match=r"sd_roi_pool_v1_fwd takes 13 arguments \(data, rois, .*stream\), got 1[24]"):
            l.call("sd_roi_pool_v1_fwd", *args)
    assert fake.sd_roi_pool_v1_fwd.args is None                 # the foreign function was not reached
    with pytest.raises(AttributeError, match="sd_no_such_entry"):
        l.call("sd_no_such_entry")


def test_ops_call_appends_the_stream_where_the_prototype_ends_in_one(recorded, monkeypatch):
    from simpledet_amd import ops

    l, fake = recorded
    stream = ctypes.c_void_p(77)
    monkeypatch.setattr(ops, "lib", lambda: l)
    monkeypatch.setattr(ops, "_stream", lambda: stream)
    assert l.entry("sd_bbox_overlaps").stream and not l.entry("sd_glibc_srand_host").stream
    ops._call("sd_bbox_overlaps", None, 3, None, 4, None)       # (boxes, n, query_boxes, k, overlaps, stream)
    assert fake.sd_bbox_overlaps.args == (None, 3, None, 4, None, stream)
    host = (ctypes.c_int32 * 33)()
    ops._call("sd_glibc_srand_host", 1, host)                   # (seed, state33): no stream parameter
    assert fake.sd_glibc_srand_host.args == (1, host)
    assert ops._query("sd_fpn_roi_align_argmax_stride", 7, 7) == 0 and fake.sd_fpn_roi_align_argmax_stride.args == (7, 7)


def test_glibc_srand_host_matches_oracle(oracle):
    l = _lib.lib()
    for seed in (1, 0, 12345):
        st = (ctypes.c_int32 * 33)()
        l.call("sd_glibc_srand_host", ctypes.c_uint32(seed), st)
        g = oracle.GlibcRand(seed)
        assert list(st) == list(g.state_words())


def test_no_product_code_touches_the_oracle():
    """The product path must never import/link the oracle (voids parity claims otherwise)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dp, _, files in os.walk(os.path.join(root, "simpledet_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cc", ".cpp")) or f == "Makefile":
                text = open(os.path.join(dp, f)).read()
                for bad in ("pyoracle", "liboracle", "import oracle", "from oracle", "-loracle",
                            "oracle.h", "orc_"):
                    assert bad not in text, (f, bad)
