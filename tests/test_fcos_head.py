"""FCOS training head: sd_fcos_target, sd_fcos_loss_fwd / _bwd (simpledet_amd/csrc/fcos_head.hip).

CPU: argument validation of every entry point; sd_fcos_num_locations against the reference's infer_shape formula;
     the numpy restatement (tests/fcos_ref.py) equal BIT FOR BIT to tests/golden/fcos_head.npz -- the reference's
     own make_fcos_gt / loss functions run on the evaluating stand-in (tests/golden/make_golden_fcos.py) -- on
     every stored array; a hand-worked known answer.
GPU: targets bit-equal to the fixture (every output, dense and compact, and the count; all elements); losses at
     L = 5 and L = 1 with equal bits, exact zero patterns, and every gradient element and the three scalars within
     the house margin  k = |got - truth| / (eps32 * T * s + tiny),  max k_gpu <= 2 * k_ref + 2  with k_ref the
     float32 restatement's own maximum on the same cases (as tests/test_focal_loss.py); repeatability, graph
     replay, pointers 4 bytes off their 16-byte boundary, gamma in {0, 1, 2}, red zones around every output.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from simpledet_amd import _lib
from . import fcos_ref as fr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fcos_head.npz")
F32 = np.float32


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def target_cases():
    return fr.target_cases()


@functools.lru_cache(maxsize=None)
def loss_cases():
    return fr.loss_cases()


@functools.lru_cache(maxsize=None)
def loss_refs():
    """[(name, case, float32 restatement, float64 truth)], computed once"""
    out = []
    for name, c in loss_cases():
        kw = dict(alpha=c["alpha"], gamma=c["gamma"])
        out.append((name, c, fr.losses_f32(c["cls"], c["ctr"], c["off"], c["tg"], **kw),
                    fr.losses_truth(c["cls"], c["ctr"], c["off"], c["tg"], **kw)))
    return out


def _k(res, truth):
    """(k of the gradients, k of the scalars)"""
    kg = max(fr.k_of(res["d_cls"], truth["d_cls"], truth["T_cls"], truth["s_cls"]),
             fr.k_of(res["d_ctr"], truth["d_ctr"], truth["T_ctr"], truth["s_ctr"]),
             fr.k_of(res["d_off"], truth["d_off"], truth["T_off"], truth["s_off"]))
    return kg, fr.k_losses(res["losses"], truth)


def _same_zeros(got, truth, key, r32=None):
    """The masks' zero pattern: an exact zero wherever the float64 truth is zero (masked, ignored, outside the clip
    range).  The issue asks for a pattern "exactly the truth's"; float32 cannot deliver that at saturated logits
    (1 - p rounds to 0 at x = 30, p * p underflows at x = -100, where the float64 truth is 1e-16 or 1e-87), so this
    is a stated relaxation, kept as narrow as the number format allows:
      * the device (r32 given): a zero outside the truth's pattern only where the float32 restatement of the
        reference's own arithmetic holds a zero too;
      * the restatement itself (r32 None): only where the truth is below ONE unit (eps32 * T + tiny) * s of the
        element's own margin."""
    g, t = np.asarray(got[key]), np.asarray(truth[key])
    gz, tz = g == 0, t == 0
    extra = gz & ~tz
    if r32 is not None:
        return bool(gz[tz].all()) and bool((np.asarray(r32[key]) == 0)[extra].all())
    unit = (fr.EPS32 * truth["T" + key[1:]] + fr.TINY32) * truth["s" + key[1:]]     # k_of's denominator
    return bool(gz[tz].all()) and bool((np.abs(t[extra]) <= unit[extra]).all())


@functools.lru_cache(maxsize=None)
def k_ref():
    ks = [_k(r, t) for _, _, r, t in loss_refs()]
    return max(k[0] for k in ks), max(k[1] for k in ks)


# ------------------------------------------------------------------------------------------------ CPU --
def _i(vals):
    return (ctypes.c_int * len(vals))(*vals)


def _l(vals):
    return (ctypes.c_long * len(vals))(*vals)


def _ptrs(vals):
    return (ctypes.c_void_p * len(vals))(*vals)


def test_num_locations_is_the_reference_infer_shape():
    l = _lib.lib()
    for (h, w), strides in (((800, 1333), fr.STRIDES), ((64, 96), fr.STRIDES), ((72, 40), fr.STRIDES),
                            ((1, 1), (8,)), ((17, 129), (3, 7, 128)), ((0, 5), (8, 16))):
        levels, total = _l([0] * len(strides)), ctypes.c_long(-1)
        assert l.call("sd_fcos_num_locations", h, w, _i(strides), len(strides), levels, ctypes.byref(total)) == 0
        want = [a * b for a, b in fr.level_sizes((h, w), strides)]
        assert list(levels) == want and total.value == sum(want)
    assert fr.num_locations((800, 1333), fr.STRIDES) == 22300
    assert fr.num_locations((64, 96), fr.STRIDES) == 129
    total = ctypes.c_long(0)
    with pytest.raises(_lib.SimpleDetOpsError, match="negative"):
        l.call("sd_fcos_num_locations", -1, 4, _i([8]), 1, None, ctypes.byref(total))
    with pytest.raises(_lib.SimpleDetOpsError, match="not positive"):
        l.call("sd_fcos_num_locations", 8, 8, _i([0]), 1, None, ctypes.byref(total))
    with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit 8") as e:
        l.call("sd_fcos_num_locations", 8, 8, _i([8] * 9), 9, None, ctypes.byref(total))
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="null"):
        l.call("sd_fcos_num_locations", 8, 8, _i([8]), 1, None, None)


def test_target_rejects_bad_arguments_without_a_gpu():
    l = _lib.lib()
    P = ctypes.c_void_p(4096)       # never dereferenced: every check comes before the first launch
    st = _i(fr.STRIDES)
    ws = ctypes.c_size_t(1 << 20)

    def call(gt=P, info=P, cen=P, off=P, cid=P, dense=None, state=P, N=2, M=5, K=3, h=64, w=96, strides=st,
             lo=None, up=None, L=5, io=-1.0, il=-1.0, wsp=P, wsb=ws):
        return l.call("sd_fcos_target", gt, info, cen, off, cid, dense, state, N, M, K, h, w, strides, lo, up, L,
                      io, il, wsp, wsb, None)
    for kw in (dict(N=-1), dict(M=-1), dict(K=-1), dict(h=-1), dict(L=-1)):
        with pytest.raises(_lib.SimpleDetOpsError, match="negative dimension"):
            call(**kw)
    for name in ("gt", "info", "cen", "off", "cid", "state"):
        with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
            call(**{name: None})
    for kw in (dict(io=float("nan")), dict(il=float("nan"))):
        with pytest.raises(_lib.SimpleDetOpsError, match="NaN"):
            call(**kw)
    with pytest.raises(_lib.SimpleDetOpsError, match="must be negative"):
        call(io=0.0)
    with pytest.raises(_lib.SimpleDetOpsError, match="must be negative"):
        call(il=1.0)
    nanb = (ctypes.c_float * 5)(0, 1, 2, float("nan"), 4)
    okb = (ctypes.c_float * 5)(0, 1, 2, 3, 4)
    with pytest.raises(_lib.SimpleDetOpsError, match="bound of level 3 is NaN"):
        call(lo=nanb, up=okb)
    with pytest.raises(_lib.SimpleDetOpsError, match="without the other"):
        call(lo=okb)
    with pytest.raises(_lib.SimpleDetOpsError, match="default stage bounds"):
        call(L=6, strides=_i([8] * 6))
    with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit 8") as e:
        call(L=9, strides=_i([8] * 9))
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="M=0"):
        call(M=0)
    with pytest.raises(_lib.SimpleDetOpsError, match="N=65536 images exceed the limit 65535") as e:
        call(N=65536, M=1, K=1, h=8, w=8, L=1, strides=_i([8]))
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
        call(wsb=ctypes.c_size_t(8))
    assert e.value.code == -4
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
        call(wsp=None)
    with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit") as e:     # 2 * 80 * (4096 * 4096) > 2^31 - 1
        call(K=80, h=4096 * 8, w=4096 * 8, L=1, strides=_i([8]))
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    # empty problems succeed without touching the device (the pointers may even be null)
    assert call(N=0, gt=None, cen=None) == 0
    assert call(h=0, gt=None, cen=None, wsp=None) == 0
    assert call(L=0, strides=None, off=None) == 0
    assert l.cdll.sd_fcos_target_workspace_bytes(2, ctypes.c_long(22300)) >= 2 * 88 * 12
    assert l.cdll.sd_fcos_target_workspace_bytes(-1, ctypes.c_long(5)) == 0


def test_losses_reject_bad_arguments_without_a_gpu():
    l = _lib.lib()
    P = ctypes.c_void_p(4096)
    tab, hw = _ptrs([4096] * 5), _l([96, 24, 6, 2, 1])
    ws = ctypes.c_size_t(1 << 20)

    def fwd(cls=tab, ctr=tab, off=tab, hws=hw, L=5, cen=P, offs=P, cid=P, state=P, losses=P, N=2, K=3, alpha=0.25,
            gamma=2.0, io=-1.0, il=-1.0, wsp=P, wsb=ws):
        return l.call("sd_fcos_loss_fwd", cls, ctr, off, hws, L, cen, offs, cid, state, losses, N, K, alpha, gamma, io,
                      il, wsp, wsb, None)

    def bwd(cls=tab, ctr=tab, off=tab, dcls=tab, dctr=tab, doff=tab, hws=hw, L=5, cen=P, offs=P, cid=P, state=P,
            N=2, K=3, alpha=0.25, gamma=2.0, io=-1.0, il=-1.0):
        return l.call("sd_fcos_loss_bwd", cls, ctr, off, dcls, dctr, doff, hws, L, cen, offs, cid, state, N, K, alpha,
                      gamma, io, il, None)
    for f in (fwd, bwd):
        for kw in (dict(N=-1), dict(K=-1), dict(L=-1)):
            with pytest.raises(_lib.SimpleDetOpsError, match="negative dimension"):
                f(**kw)
        with pytest.raises(_lib.SimpleDetOpsError, match="negative size"):
            f(hws=_l([96, -1, 6, 2, 1]))
        for name in ("alpha", "gamma", "io", "il"):
            with pytest.raises(_lib.SimpleDetOpsError, match="NaN"):
                f(**{name: float("nan")})
        for name in ("cls", "ctr", "off", "hws"):
            with pytest.raises(_lib.SimpleDetOpsError, match="null level table"):
                f(**{name: None})
        with pytest.raises(_lib.SimpleDetOpsError, match="null pointer in level 2"):
            f(ctr=_ptrs([4096, 4096, 0, 4096, 4096]))
        for name in ("cen", "offs", "cid", "state"):
            with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
                f(**{name: None})
        with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit 8") as e:
            f(L=9, hws=_l([1] * 9), cls=_ptrs([4096] * 9), ctr=_ptrs([4096] * 9), off=_ptrs([4096] * 9))
        assert e.value.code == _lib.SD_ERR_UNSUPPORTED
        with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit") as e:
            f(K=80, hws=_l([1 << 24, 24, 6, 2, 1]))
        assert e.value.code == _lib.SD_ERR_UNSUPPORTED
        # empty problems
        assert f(N=0, cen=None) == 0 and f(K=0, cls=None) == 0 and f(hws=_l([0] * 5), cid=None) == 0
        assert f(L=0, hws=None, cls=None) == 0
    with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
        fwd(losses=None)
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
        fwd(wsb=ctypes.c_size_t(16))
    assert e.value.code == -4
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
        fwd(wsp=None)
    with pytest.raises(_lib.SimpleDetOpsError, match="null level table"):
        bwd(dcls=None)
    with pytest.raises(_lib.SimpleDetOpsError, match="null gradient pointer in level 4"):
        bwd(doff=_ptrs([4096, 4096, 4096, 4096, 0]))
    assert l.cdll.sd_fcos_loss_workspace_bytes(2, 80, ctypes.c_long(22300)) >= 2048 * 12
    assert l.cdll.sd_fcos_loss_workspace_bytes(2, -1, ctypes.c_long(5)) == 0


def test_restatement_equals_the_reference_fixture_bit_for_bit():
    g = golden()
    names = [n for n, _ in target_cases()]
    assert list(g["target_cases"]) == names and list(g["loss_cases"]) == [n for n, _ in loss_cases()]
    for name, c in target_cases():
        assert np.array_equal(g["t/%s/gt_bbox" % name], c["gt_bbox"]) and np.array_equal(g["t/%s/im_info" % name], c["im_info"])
        assert list(g["t/%s/geom" % name]) == list(c["data_size"]) + [c["K"]] + list(c["strides"])
        tg = fr.targets_f32(c["gt_bbox"], c["im_info"], c["data_size"], c["strides"], c["K"])
        for key in ("centerness", "offset"):
            a, b = g["t/%s/%s" % (name, key)], tg[key]
            assert a.dtype == b.dtype == F32 and a.shape == b.shape
            assert np.array_equal(a.view(np.int32), b.view(np.int32)), (name, key)
        assert np.array_equal(g["t/%s/cls_gt" % name].astype(F32), tg["cls_gt"]), name
    assert np.isnan(g["t/degenerate/centerness"]).sum() > 0          # the 0/0 of a degenerate box is in the fixture
    # the stage-bounds case does what its name says: at each probe the greatest offset of the deciding box IS the bound
    # of the location's own level, and the fixture holds the inclusive-lower / exclusive-upper outcome
    c = dict(target_cases())["stage-bounds"]
    loc_x, loc_y, lo, up, _ = fr.grid(c["data_size"], c["strides"], c["im_info"])
    dense = g["t/stage-bounds/cls_gt"].astype(F32).reshape(2, c["K"], -1)
    for n, j, bound, want in fr.STAGE_BOUND_PROBES:
        box = c["gt_bbox"][n]
        great = np.max(np.stack([loc_x[j] - box[:, 0], loc_y[j] - box[:, 1], box[:, 2] - loc_x[j], box[:, 3] - loc_y[j]]), axis=0)
        assert bound in great and bound in (lo[j], up[j]), (n, j)
        assert (int(dense[n, :, j].argmax()) + 1 if dense[n, :, j].max() == 1 else 0) == want, (n, j)
        assert (g["t/stage-bounds/offset"][n, 0, j] == bound) == (want != 0), (n, j)
    for name, c, r32, _ in loss_refs():
        for key in ("losses", "d_cls", "d_ctr"):
            a, b = g["l/%s/%s" % (name, key)], r32[key]
            assert a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), (name, key)


def test_known_answer_one_box_stride_8():
    """data_size (16, 24), stride 8: centres x in {4, 12, 20}, y in {4, 12}.  Box [2, 2, 14, 14] class 2 holds (4, 4),
    (12, 4), (4, 12), (12, 12).  At (4, 4): l = t = 2, r = b = 10, centerness = sqrt(2 * 2 / (10 * 10)) = 0.2; at
    (12, 12): l = t = 10, r = b = 2, the same; at (12, 4): l = 10, r = 2, t = 2, b = 10: 0.2 as well."""
    gt = F32([[[2, 2, 14, 14, 2]]])
    tg = fr.targets_f32(gt, F32([[16, 24, 1]]), (16, 24), (8,), 3)
    want_c = F32([0.2, 0.2, 0, 0.2, 0.2, 0])
    assert np.array_equal(tg["centerness"][0], want_c)
    assert np.array_equal(tg["offset"][0, :, 0], F32([2, 2, 10, 10])) and np.array_equal(tg["offset"][0, :, 2], F32([-1] * 4))
    assert np.array_equal(tg["offset"][0, :, 4], F32([10, 10, 2, 2]))
    assert list(tg["cls_id"][0]) == [2, 2, 0, 2, 2, 0] and tg["count"] == 4
    assert np.array_equal(tg["cls_gt"].reshape(3, 6)[1], F32([1, 1, 0, 1, 1, 0])) and tg["cls_gt"].sum() == 4
    # losses at logits 0 / predictions equal to nothing special: p = 1/2 everywhere
    cls, ctr = np.zeros((1, 3, 6), F32), np.zeros((1, 1, 6), F32)
    off = np.full((1, 4, 6), 6, F32)
    r = fr.losses_f32(cls, ctr, off, tg, alpha=0.25, gamma=2.0)
    # focal: 4 positives 0.25 * 0.25 * ln 2, 14 negatives 0.75 * 0.25 * ln 2, norm 4 + 1
    assert abs(float(r["losses"][1]) - (4 * 0.0625 + 14 * 0.1875) * np.log(2) / 5) < 1e-6
    # BCE with label 0.2 at p = 1/2 is ln 2, over the 4 positive locations
    assert abs(float(r["losses"][0]) - np.log(2)) < 1e-6
    # IoU: pred 12 x 12 = target 12 x 12 area; intersection (2 + 6) * (2 + 6) = 64, union 144 + 144 - 64 = 224
    assert abs(float(r["losses"][2]) - (-np.log(65 / 225))) < 1e-6
    t = fr.losses_truth(cls, ctr, off, tg, alpha=0.25, gamma=2.0)
    assert np.allclose(r["losses"], t["losses"], rtol=1e-6) and np.allclose(r["d_off"], t["d_off"], atol=1e-7)
    # the portrait switch and the padding mask: ori (16, 10) takes the transposed grid, loc_x = [4, 12] * 3 and
    # loc_y = [4, 4, 12, 12, 20, 20]; x < 10 and y < 16 keep locations 0 and 2, both inside the box
    tp = fr.targets_f32(gt, F32([[16, 10, 1]]), (16, 24), (8,), 3)
    assert list(tp["cls_id"][0]) == [2, -1, 2, -1, -1, -1]
    assert np.array_equal(tp["offset"][0, :, 2], F32([2, 10, 10, 2]))


def test_restatements_agree_and_k_ref():
    kg, ks = k_ref()
    print("fcos k_ref: gradients %.3f  scalars %.3f" % (kg, ks))
    assert kg < 64 and ks < 64       # the float32 restatement itself stays within a few dozen units of its truth
    for name, c, r32, t in loss_refs():
        for key in ("d_cls", "d_ctr", "d_off"):
            assert _same_zeros(r32, t, key), (name, key)


# ------------------------------------------------------------------------------------------------ GPU --
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _run_target(ops, c, dense=True, **kw):
    return ops.fcos_target(_dev(c["gt_bbox"]), _dev(c["im_info"]), c["data_size"], c["strides"], c["K"], dense=dense, **kw)


def _bits(t):
    import torch
    return t.contiguous().view(torch.int32)


@pytest.mark.gpu
def test_hip_targets_equal_the_reference_fixture(ops):
    import torch
    g = golden()
    for name, c in target_cases():
        t = _run_target(ops, c)
        N, K = c["gt_bbox"].shape[0], c["K"]
        for key, got in (("centerness", t.centerness), ("offset", t.offset)):
            want = g["t/%s/%s" % (name, key)]
            assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32)), (name, key)
        dense = g["t/%s/cls_gt" % name].astype(F32)
        assert np.array_equal(t.cls_dense.cpu().numpy().view(np.int32), dense.view(np.int32)), name
        # dense and compact agree with each other, and with the count
        cid = t.cls_id.cpu().numpy()
        d3 = dense.reshape(N, K, -1)
        want_id = np.where(d3[:, 0] == -1, -1, (d3.argmax(axis=1) + 1) * (d3.max(axis=1) == 1))
        assert np.array_equal(cid, want_id), name
        state = t.state.cpu().numpy()
        assert state[0] == int((dense * (dense != -1)).sum()) == int((cid >= 1).sum()), name
        cen = g["t/%s/centerness" % name]
        assert state[1] == int(np.logical_and(cen != -1, cen > 0).sum()), name
        # the compact call alone writes the same bits
        t2 = _run_target(ops, c, dense=False)
        assert t2.cls_dense is None and torch.equal(t2.cls_id, t.cls_id) and torch.equal(t2.state, t.state)
        assert torch.equal(_bits(t2.centerness), _bits(t.centerness)) and torch.equal(t2.offset, t.offset)
    assert np.isnan(g["t/degenerate/centerness"]).any()


def _levels(c, flat, C):
    """the concatenated (N, C, HW) array as per-level (N, C, H_l, W_l) device tensors"""
    shapes = [(flat.shape[0], C, a, b) for a, b in fr.level_sizes(c["case"]["data_size"], c["case"]["strides"])]
    return [_dev(v) for v in fr.split_levels(flat, c["hws"], shapes)]


def _targets(ops, c):
    return _run_target(ops, c["case"], dense=False)


def _cat(levels):
    import torch
    return torch.cat([v.reshape(v.shape[0], v.shape[1], -1) for v in levels], dim=2).cpu().numpy()


@pytest.mark.gpu
def test_hip_losses_margin_zero_patterns_and_level_forms(ops):
    import torch
    kg_ref, ks_ref = k_ref()
    kg_gpu = ks_gpu = 0.0
    for name, c, r32, truth in loss_refs():
        tg = _targets(ops, c)
        kw = dict(alpha=c["alpha"], gamma=c["gamma"])
        K = c["case"]["K"]
        lv = [_levels(c, c["cls"], K), _levels(c, c["ctr"], 1), _levels(c, c["off"], 4)]
        one = [[_dev(c["cls"])], [_dev(c["ctr"])], [_dev(c["off"])]]
        l5 = ops.fcos_loss_forward(*lv, tg, **kw)
        l1 = ops.fcos_loss_forward(*one, tg, **kw)
        assert torch.equal(_bits(l5), _bits(l1)), name                   # L = 5 and L = 1: the same bits
        g5 = ops.fcos_loss_backward(*lv, tg, **kw)
        g1 = ops.fcos_loss_backward(*one, tg, **kw)
        got = dict(losses=l5.cpu().numpy())
        for key, a, b in zip(("d_cls", "d_ctr", "d_off"), g5, g1):
            assert [tuple(x.shape) for x in a] == [tuple(x.shape) for x in lv[("d_cls", "d_ctr", "d_off").index(key)]]
            got[key] = _cat(a)
            assert np.array_equal(got[key].view(np.int32), b[0].cpu().numpy().view(np.int32)), (name, key)
            # masks and zero patterns are exactly the truth's; ignored and padded locations hold exact zeros
            assert _same_zeros(got, truth, key, r32), (name, key)
        ign = c["tg"]["cls_id"] < 0
        assert ign.any() or "pad" not in name
        assert not got["d_cls"][np.broadcast_to(ign[:, None, :], got["d_cls"].shape)].any()
        kg, ks = _k(got, truth)
        print("%s: gradients k_gpu %.3f  scalars k_gpu %.3f" % (name, kg, ks))
        kg_gpu, ks_gpu = max(kg_gpu, kg), max(ks_gpu, ks)
    print("fcos margins: gradients k_ref %.3f k_gpu %.3f (bound %.3f); scalars k_ref %.3f k_gpu %.3f (bound %.3f)"
          % (kg_ref, kg_gpu, 2 * kg_ref + 2, ks_ref, ks_gpu, 2 * ks_ref + 2))
    assert kg_gpu <= 2 * kg_ref + 2
    assert ks_gpu <= 2 * ks_ref + 2


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0])
def test_hip_gamma_variants_match_the_restatement(ops, gamma):
    name, c = loss_cases()[1]
    tg = _targets(ops, c)
    K = c["case"]["K"]
    lv = [_levels(c, c["cls"], K), _levels(c, c["ctr"], 1), _levels(c, c["off"], 4)]
    truth = fr.losses_truth(c["cls"], c["ctr"], c["off"], c["tg"], alpha=0.25, gamma=gamma)
    r32 = fr.losses_f32(c["cls"], c["ctr"], c["off"], c["tg"], alpha=0.25, gamma=gamma)
    got = dict(losses=ops.fcos_loss_forward(*lv, tg, alpha=0.25, gamma=gamma).cpu().numpy())
    for key, a in zip(("d_cls", "d_ctr", "d_off"), ops.fcos_loss_backward(*lv, tg, alpha=0.25, gamma=gamma)):
        got[key] = _cat(a)
    (kg, ks), (kg_ref, ks_ref) = _k(got, truth), _k(r32, truth)
    print("gamma %g: gradients k_ref %.3f k_gpu %.3f; scalars k_ref %.3f k_gpu %.3f" % (gamma, kg_ref, kg, ks_ref, ks))
    assert kg <= 2 * kg_ref + 2 and ks <= 2 * ks_ref + 2


def _chain(ops, c, lv, bufs=None):
    b = bufs or {}
    tg = ops.fcos_target(b["gt"], b["info"], c["case"]["data_size"], c["case"]["strides"], c["case"]["K"],
                         centerness=b.get("centerness"), offset=b.get("offset"), cls_id=b.get("cls_id"),
                         state=b.get("state"), workspace=b.get("ws_t"))
    kw = dict(alpha=c["alpha"], gamma=c["gamma"])
    losses = ops.fcos_loss_forward(*lv, tg, losses=b.get("losses"), workspace=b.get("ws_l"), **kw)
    grads = ops.fcos_loss_backward(*lv, tg, d_cls=b.get("d_cls"), d_ctr=b.get("d_ctr"), d_off=b.get("d_off"), **kw)
    return tg, losses, grads


def _flat(tg, losses, grads):
    return [tg.centerness, tg.offset, tg.cls_id, tg.state, losses] + [x for g in grads for x in g]


@pytest.mark.gpu
def test_hip_chain_repeats_and_replays_with_equal_bits(ops):
    import torch
    name, c = loss_cases()[4]                                     # several workgroups per image
    K = c["case"]["K"]
    lv = [_levels(c, c["cls"], K), _levels(c, c["ctr"], 1), _levels(c, c["off"], 4)]
    N, HW = c["tg"]["centerness"].shape
    b = dict(gt=_dev(c["case"]["gt_bbox"]), info=_dev(c["case"]["im_info"]))
    first = [t.clone() for t in _flat(*_chain(ops, c, lv, b))]
    second = _flat(*_chain(ops, c, lv, b))
    for x, y in zip(first, second):
        assert torch.equal(_bits(x), _bits(y))
    # the chain target -> forward -> backward as ONE graph, into buffers allocated beforehand
    b.update(centerness=torch.empty(N, HW, device="cuda"), offset=torch.empty(N, 4, HW, device="cuda"),
             cls_id=torch.empty(N, HW, device="cuda", dtype=torch.int32),
             state=torch.empty(4, device="cuda", dtype=torch.int32), losses=torch.empty(3, device="cuda"),
             ws_t=torch.empty(ops.fcos_target_workspace_bytes(N, HW), device="cuda", dtype=torch.uint8),
             ws_l=torch.empty(ops.fcos_loss_workspace_bytes(N, K, HW), device="cuda", dtype=torch.uint8),
             d_cls=[torch.empty_like(t) for t in lv[0]], d_ctr=[torch.empty_like(t) for t in lv[1]],
             d_off=[torch.empty_like(t) for t in lv[2]])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _chain(ops, c, lv, b)                                     # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _flat(*_chain(ops, c, lv, b))
    for _ in range(2):
        for t in out:
            t.zero_() if t.dtype == torch.int32 else t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip(first, out):
            assert torch.equal(_bits(x), _bits(y))


def _carve(arena, off, like, skew):
    """a tensor of like's shape inside the sentinel arena, 16-byte aligned plus `skew` bytes, guards around it"""
    n = like.numel() * 4
    start = (off + 4096 + 255) // 256 * 256 + skew
    view = arena[start:start + n].view(like.dtype).reshape(like.shape)
    return view, start, start + n


@pytest.mark.gpu
@pytest.mark.parametrize("skew", [0, 4])
def test_hip_red_zones_and_pointers_off_their_16_byte_boundary(ops, skew):
    """every output and workspace sits in one arena filled with a sentinel, 4 KB guards around each; with skew = 4
    every pointer -- inputs included -- is 4 bytes past a 16-byte boundary.  The results equal the plain run's bits
    and no guard byte changes."""
    import torch
    name, c = loss_cases()[0]                                     # K = 80, HW = 129: rows on every 16-byte phase
    K = c["case"]["K"]
    plain_lv = [_levels(c, c["cls"], K), _levels(c, c["ctr"], 1), _levels(c, c["off"], 4)]
    plain_b = dict(gt=_dev(c["case"]["gt_bbox"]), info=_dev(c["case"]["im_info"]))
    tg0 = ops.fcos_target(plain_b["gt"], plain_b["info"], c["case"]["data_size"], c["case"]["strides"], K, dense=True)
    kw = dict(alpha=c["alpha"], gamma=c["gamma"])
    want = [tg0.centerness, tg0.offset, tg0.cls_id, tg0.state, tg0.cls_dense,
            ops.fcos_loss_forward(*plain_lv, tg0, **kw)] + [x for g in ops.fcos_loss_backward(*plain_lv, tg0, **kw) for x in g]
    N, HW = c["tg"]["centerness"].shape
    arena = torch.full((8 << 20,), 0xA5, dtype=torch.uint8, device="cuda")
    spans, off = [], 0

    def carve(like):
        nonlocal off
        v, s, e = _carve(arena, off, like, skew)
        spans.append((s, e))
        off = e
        return v

    def put(t):
        v = carve(t)
        v.copy_(t)
        return v
    lv = [[put(t) for t in lst] for lst in plain_lv]
    gt, info = put(plain_b["gt"]), put(plain_b["info"])
    f, i32, u8 = torch.float32, torch.int32, torch.uint8
    E = lambda shape, dt=f: carve(torch.empty(shape, dtype=dt, device="meta"))
    ws_t = carve(torch.empty((ops.fcos_target_workspace_bytes(N, HW) + 3) // 4, dtype=i32, device="meta")).view(u8)
    ws_l = carve(torch.empty((ops.fcos_loss_workspace_bytes(N, K, HW) + 3) // 4, dtype=i32, device="meta")).view(u8)
    tg = ops.fcos_target(gt, info, c["case"]["data_size"], c["case"]["strides"], K, centerness=E((N, HW)),
                         offset=E((N, 4, HW)), cls_id=E((N, HW), i32), state=E((4,), i32), cls_dense=E((N, K * HW)),
                         workspace=ws_t)
    losses = ops.fcos_loss_forward(*lv, tg, losses=E((3,)), workspace=ws_l, **kw)
    grads = ops.fcos_loss_backward(*lv, tg, d_cls=[E(t.shape) for t in lv[0]], d_ctr=[E(t.shape) for t in lv[1]],
                                   d_off=[E(t.shape) for t in lv[2]], **kw)
    torch.cuda.synchronize()
    got = [tg.centerness, tg.offset, tg.cls_id, tg.state, tg.cls_dense, losses] + [x for g in grads for x in g]
    for x, y in zip(want, got):
        assert y.data_ptr() % 16 == skew and torch.equal(_bits(x), _bits(y))
    keep = torch.ones(arena.numel(), dtype=torch.bool, device="cuda")
    for s, e in spans:
        keep[s:e] = False
    assert bool((arena[keep] == 0xA5).all()), "a store outside the buffers the library was given"


@pytest.mark.gpu
def test_empty_problem_leaves_zero_normalisers(ops):
    import torch
    gt, info = torch.zeros(2, 1, 5, device="cuda"), torch.ones(2, 3, device="cuda")
    state = torch.full((4,), 7, device="cuda", dtype=torch.int32)
    t = ops.fcos_target(gt, info, (0, 8), (8,), 3, state=state)        # HW = 0: nothing is launched
    assert t.centerness.shape == (2, 0) and t.state is state and not state.any()
    lv = [[torch.empty(2, 3, 0, 1, device="cuda")], [torch.empty(2, 1, 0, 1, device="cuda")],
          [torch.empty(2, 4, 0, 1, device="cuda")]]
    assert not ops.fcos_loss_forward(*lv, t).any()


@pytest.mark.gpu
def test_autograd_function_returns_the_raw_gradients(ops):
    import torch
    name, c = loss_cases()[3]
    K = c["case"]["K"]
    lv = [_levels(c, c["cls"], K), _levels(c, c["ctr"], 1), _levels(c, c["off"], 4)]
    tg = _targets(ops, c)
    kw = dict(alpha=c["alpha"], gamma=c["gamma"])
    req = [[t.clone().requires_grad_(True) for t in lst] for lst in lv]
    losses = ops.fcos_loss(*req, tg, **kw)
    assert torch.equal(losses, ops.fcos_loss_forward(*lv, tg, **kw))
    (losses.sum() * 3.0).backward()          # the incoming gradient is ignored, as the reference's loss nodes do
    want = ops.fcos_loss_backward(*lv, tg, **kw)
    for a, b in zip(req, want):
        for x, y in zip(a, b):
            assert torch.equal(_bits(x.grad), _bits(y))
