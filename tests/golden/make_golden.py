#!/usr/bin/env python
"""Generate the golden fixtures in this directory FROM THE REFERENCE ITSELF.

Run in the build container (needs /root/reference and oracle/_ref built by oracle/build_ref.py):
    python tests/golden/make_golden.py
The fixtures are small .npz files committed next to this script; tests only read the .npz files
(/root/reference does not exist on the GPU box).

What is executed from the reference (no source is copied; functions are loaded from the files
where they lie):
  anchors.npz      symbol/builder.py:904-938  add_anchor_to_arg  (numpy; `mx.nd.array` stubbed
                   with the identity because mxnet is not installed)
  fpn_assign.npz   models/FPN/assign_layer_fpn.py:17-41  AssignLayerFPNOperator.forward, run with a
                   float32 numpy shim of the eight mx.nd functions it calls (sqrt, floor, log2,
                   clip, zeros_like, expand_dims, broadcast_like, where)
  fpn_assign_thresholds.npz   the same class and shim on the RoIs of tests/fpn_level_cases.py (the areas
                   within 400 ulp of every level threshold of two pyramids, where the last bit of log2
                   decides the level; numpy's float32 log2 is the correctly rounded one there, which
                   tests/test_fpn_level_thresholds.py asserts).  Holds the parameters, the SHA-256 of the
                   RoIs and one int8 level per RoI; written with fixed time stamps (same bytes every run)
  py_nms.npz       operator_py/nms.py:41-75  nms  (pure numpy hard NMS, suppress IoU > thresh)
  cython_nms.npz   operator_py/cython/cpu_nms.pyx soft_nms / greedy_nms and bbox.pyx
                   bbox_overlaps_cython, compiled by oracle/build_ref.py into oracle/_ref
  top_proposal.npz models/FPN/get_top_proposal.py:10-67  GetTopProposalOperator.forward and
                   GetTopProposalProp (arguments, outputs, infer_shape), run with a numpy shim of
                   mx.operator.CustomOp / mx.nd.argsort / mx.nd.stack.  The ONE thing the shim
                   decides is the order of equal scores: mx.nd.argsort(is_ascend=False) is MXNet's
                   SortByKey, a STABLE sort with a descending comparator on both devices
                   (std::stable_sort / thrust::stable_sort_by_key), i.e. equal scores keep their
                   input order -- np.argsort(-x, kind="stable").  The cases hold tied scores, so
                   the fixture pins that choice too; everything else is the reference's code.
"""
import ast
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("SIMPLEDET_REFERENCE", "/root/reference")
sys.path.insert(0, ROOT)


def load_defs(path, names, env):
    """exec only the named top-level defs/classes of a reference file into env."""
    tree = ast.parse(open(path).read())
    body = [n for n in tree.body
            if isinstance(n, (ast.FunctionDef, ast.ClassDef)) and n.name in names]
    assert len(body) == len(names), (path, names)
    mod = ast.Module(body=body, type_ignores=[])
    exec(compile(mod, path, "exec"), env)
    return env


def clustered_dets(seed, n, ncl=25, extent=600.0):
    rs = np.random.RandomState(seed)
    c = rs.rand(ncl, 2) * extent
    ctr = c[rs.randint(0, ncl, n)] + rs.randn(n, 2) * 6
    wh = rs.rand(n, 2) * 80 + 12
    sc = rs.permutation(n).astype(np.float32) / n * 0.95 + 0.05  # distinct scores
    return np.concatenate([ctr - wh / 2, ctr + wh / 2, sc[:, None]], 1).astype(np.float32)


def make_anchors():
    class _ND:
        @staticmethod
        def array(x):
            return x
    mx = types.SimpleNamespace(nd=_ND)
    env = load_defs(os.path.join(REF, "symbol", "builder.py"), ["add_anchor_to_arg"], {"mx": mx})
    out = {}
    # config/faster_r50v1_fpn_1x.py:49-53,149-154: strides (4..64), scale 8, ratios .5/1/2 (max_side
    # 320 instead of 1400 keeps the fixture small; the grid code is size independent)
    args = {}
    env["add_anchor_to_arg"](None, args, None, 320, (4, 8, 16, 32, 64), (8,), (0.5, 1.0, 2.0))
    for k, v in args.items():
        out["fpn_" + k] = np.asarray(v, np.float32)
    # C4 setting: stride 16, scales 2..32
    args = {}
    env["add_anchor_to_arg"](None, args, None, 320, 16, (2, 4, 8, 16, 32), (0.5, 1.0, 2.0))
    for k, v in args.items():
        out["c4_" + k] = np.asarray(v, np.float32)
    np.savez_compressed(os.path.join(HERE, "anchors.npz"), **out)


def _assign_layer_fpn():
    """-> (the reference's AssignLayerFPNOperator over a float32 numpy shim of mx.nd, A: ndarray -> shim array)"""
    f32 = np.float32

    class _Arr(np.ndarray):
        """float32 ndarray whose ** and astype behave like mx.nd (fp32 compute)."""
        def astype(self, t, *a, **k):
            return np.asarray(self).astype(t).view(_Arr) if t != "uint8" else \
                np.asarray(self).astype(np.uint8).view(_Arr)

    def A(x):
        return np.asarray(x, f32).view(_Arr)

    class _ND:
        sqrt = staticmethod(lambda x: A(np.sqrt(np.asarray(x, f32))))
        floor = staticmethod(lambda x: A(np.floor(np.asarray(x, f32))))
        log2 = staticmethod(lambda x: A(np.log2(np.asarray(x, f32))))
        clip = staticmethod(lambda x, lo, hi: A(np.clip(np.asarray(x, f32), f32(lo), f32(hi))))
        zeros_like = staticmethod(lambda x: A(np.zeros_like(np.asarray(x, f32))))
        expand_dims = staticmethod(lambda x, axis: np.expand_dims(np.asarray(x), axis).view(_Arr))
        broadcast_like = staticmethod(lambda x, y: A(np.broadcast_to(np.asarray(x), y.shape)))
        where = staticmethod(lambda c, a, b: A(np.where(np.asarray(c) != 0, a, b)))

    class _CustomOp:
        def __init__(self):
            pass

        def assign(self, dst, req, src):
            dst[...] = src

    class _Operator:
        CustomOp = _CustomOp
        CustomOpProp = object

        @staticmethod
        def register(name):
            return lambda c: c
    mx = types.SimpleNamespace(nd=_ND, operator=_Operator)
    env = load_defs(os.path.join(REF, "models", "FPN", "assign_layer_fpn.py"),
                    ["AssignLayerFPNOperator"], {"mx": mx, "np": np})
    return env["AssignLayerFPNOperator"], A


def make_fpn_assign():
    f32 = np.float32
    op_cls, A = _assign_layer_fpn()
    from simpledet_amd import synth
    rois = np.concatenate([synth.random_rois(s, 1, 256) for s in range(4)], 0)  # (4,256,4)
    # sizes straddling every level boundary exactly (sqrt(area) = 112, 224, 448 +- 1 px)
    edge = []
    for s in (56, 111, 112, 113, 223, 224, 225, 447, 448, 449, 900):
        edge.append([10, 20, 10 + s - 1, 20 + s - 1])
    rois[0, :len(edge)] = np.asarray(edge, f32)
    strides = (4, 8, 16, 32)
    op = op_cls(strides, 224, 4)
    outs = [np.zeros_like(rois) for _ in strides]
    op.forward(True, ["write"] * 4, [A(rois)], outs, [])
    np.savez_compressed(os.path.join(HERE, "fpn_assign.npz"), rois=rois,
                        strides=np.asarray(strides), per_level=np.stack(outs))


def save_npz_reproducible(path, **arrays):
    """np.savez_compressed with a fixed member time stamp: the same arrays give the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def make_fpn_assign_thresholds():
    """the reference's class on the RoIs of tests/fpn_level_cases.py (both pyramids: every level threshold +-400
    ulp of area, then the special rows): one int8 level per RoI, read off the masked per-level outputs"""
    from tests import fpn_level_cases as cases
    op_cls, A = _assign_layer_fpn()
    out = {"half": np.array(cases.HALF), "numpy_version": np.array(np.__version__)}
    for name in sorted(cases.PYRAMIDS):
        strides, scale0, lvl0, thr = cases.PYRAMIDS[name]
        rois = cases.rois(name)
        outs = [np.zeros_like(rois) for _ in strides]
        with np.errstate(invalid="ignore"):
            op_cls(strides, scale0, lvl0).forward(True, ["write"] * len(strides), [A(rois)], outs, [])
        level = np.full(rois.shape[1], -1, np.int8)
        taken = np.zeros(rois.shape[1], np.int32)
        for l, o in enumerate(outs):
            m = (o[0] != 0).any(1)                      # no RoI of the cases is all zeros
            assert np.array_equal(o[0][m], rois[0][m])
            level[m] = l
            taken += m
        assert taken.max() == 1
        out[name + "/strides"] = np.asarray(strides, np.int32)
        out[name + "/canonical"] = np.asarray([scale0, lvl0], np.int32)
        out[name + "/thresholds"] = np.asarray(thr, np.float64)          # rows of (c, RoI width)
        out[name + "/rois_sha256"] = np.array(cases.sha256(rois))
        out[name + "/level"] = level
        print(name, rois.shape[1], "RoIs, per level", [int((level == l).sum()) for l in range(-1, len(strides))])
    save_npz_reproducible(os.path.join(HERE, "fpn_assign_thresholds.npz"), **out)


def make_py_nms():
    env = load_defs(os.path.join(REF, "operator_py", "nms.py"), ["nms"], {"np": np})
    out = {}
    for seed in range(3):
        d = clustered_dets(seed, 300)
        out["dets%d" % seed] = d
        out["kept%d" % seed] = env["nms"](d, 0.5)
    np.savez_compressed(os.path.join(HERE, "py_nms.npz"), **out)


def make_cython_nms():
    from oracle._ref import bbox, cpu_nms
    out = {}
    for seed in range(3):
        d = clustered_dets(10 + seed, 250)
        out["dets%d" % seed] = d
        for m, name in ((0, "hard"), (1, "linear"), (2, "gaussian")):
            b, i = cpu_nms.soft_nms(d, np.float32(0.5), np.float32(0.3), np.float32(0.05),
                                    np.uint8(m))
            out["soft_%s_boxes%d" % (name, seed)] = b
            out["soft_%s_inds%d" % (name, seed)] = np.asarray(i, np.int64)
        out["greedy%d" % seed] = np.asarray(cpu_nms.greedy_nms(d, np.float32(0.45)), np.int64)
        out["overlaps%d" % seed] = bbox.bbox_overlaps_cython(d[:, :4].copy(), d[:40, :4].copy())
    np.savez_compressed(os.path.join(HERE, "cython_nms.npz"), **out)


def make_top_proposal():
    class _Arr:
        """the slice of mx.nd.NDArray the operator touches, on numpy float32"""
        def __init__(self, a):
            self.a = np.asarray(a)

        @property
        def shape(self):
            return self.a.shape

        def __getitem__(self, i):
            if isinstance(i, _Arr):
                return _Arr(self.a[i.a.astype(np.int64)])
            return _Arr(self.a[i])

    class _ND:
        @staticmethod
        def argsort(x, is_ascend=True):
            k = x.a if is_ascend else -x.a
            return _Arr(np.argsort(k, kind="stable").astype(np.float32))  # mx returns float indices

        @staticmethod
        def stack(*xs):
            return _Arr(np.stack([x.a for x in xs]))

    class _CustomOp:
        def __init__(self):
            pass

        def assign(self, dst, req, src):
            assert req == "write"
            assert dst.a.shape == src.a.shape, (dst.a.shape, src.a.shape)
            dst.a[...] = src.a

    class _CustomOpProp:
        def __init__(self, need_top_grad=True):
            self.need_top_grad_ = need_top_grad

    def register(name):
        def deco(cls):
            reg[name] = cls
            return cls
        return deco

    reg = {}
    mx = types.SimpleNamespace(nd=_ND, operator=types.SimpleNamespace(
        CustomOp=_CustomOp, CustomOpProp=_CustomOpProp, register=register))
    env = {}
    sys.modules["mxnet"] = mx  # the file's own `import mxnet as mx` finds the shim
    try:
        exec(compile(open(os.path.join(REF, "models", "FPN", "get_top_proposal.py")).read(),
                     "get_top_proposal.py", "exec"), env)
    finally:
        del sys.modules["mxnet"]
    prop_cls = reg["get_top_proposal"]
    out = {}
    prop = prop_cls(top_n="2000")
    out["iface_arguments"] = np.array(prop.list_arguments())
    out["iface_outputs"] = np.array(prop.list_outputs())
    ins, outs = prop.infer_shape([(2, 10000, 4), (2, 10000, 1)])
    out["iface_infer_in"] = np.array([list(s) + [0] * (3 - len(s)) for s in ins])
    out["iface_infer_out"] = np.array([list(s) for s in outs])
    out["iface_need_top_grad"] = np.array(prop.need_top_grad_)
    out["iface_backward_dependency"] = np.array(len(prop.declare_backward_dependency([], [], [])))
    # (seed, B, N, top_n, score quantisation: 0 = distinct floats, q = scores rounded to 1/q -> ties)
    cases = [(0, 2, 10000, 2000, 0), (1, 2, 10000, 2000, 64), (2, 1, 3000, 3000, 16), (3, 3, 257, 100, 4),
             (4, 2, 10000, 1, 0), (5, 2, 64, 64, 1)]
    out["cases"] = np.array(cases)
    for seed, B, N, top_n, q in cases:
        rs = np.random.RandomState(seed)
        bbox = (rs.rand(B, N, 4) * 800).astype(np.float32)
        score = rs.rand(B, N, 1).astype(np.float32)
        if q:
            score = (np.round(score * q) / q).astype(np.float32)
        op = prop_cls(top_n=str(top_n)).create_operator(None, None, None)
        ob, os_ = _Arr(np.zeros((B, top_n, 4), np.float32)), _Arr(np.zeros((B, top_n, 1), np.float32))
        op.forward(True, ["write", "write"], [_Arr(bbox), _Arr(score)], [ob, os_], [])
        # inputs are regenerated from the seed by the tests (same expressions); outputs are stored
        out["bbox_%d" % seed] = ob.a
        out["score_%d" % seed] = os_.a
    np.savez_compressed(os.path.join(HERE, "top_proposal.npz"), **out)


if __name__ == "__main__":
    makers = (make_top_proposal, make_anchors, make_fpn_assign, make_fpn_assign_thresholds, make_py_nms,
              make_cython_nms)
    only = sys.argv[1:]          # e.g. `make_golden.py fpn_assign_thresholds`; none: all of them
    assert all("make_" + n in [m.__name__ for m in makers] for n in only), only
    for m in makers:
        if not only or m.__name__[len("make_"):] in only:
            m()
    for f in sorted(os.listdir(HERE)):
        if f.endswith(".npz"):
            print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")
