"""RetinaNet anchor targets on the device (sd_retina_anchor_target) against the loader's own
PyramidAnchorTarget2D (models/retinanet/input.py:33-199).

tests/golden/retina_target.npz was produced by the reference's classes (loaded from the reference
files, its compiled Cython IoU) on the seeded cases of tests/retinacases.py.
  CPU: the hand case of the fixture is the answer worked on paper; the quirk cases are in the fixture;
       argument validation of the C entry point.
  GPU: labels, targets, weights and fg_count equal the fixture bit for bit in both layouts, eagerly
       and under graph capture and replay.
"""
import ctypes
import hashlib
import os

import numpy as np
import pytest

from simpledet_amd import _lib

from . import retinacases

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retina_target.npz"))


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).digest()


def _param_struct(cfg):
    """sd_rpn_target_param without importing torch (simpledet_amd.ops needs it)"""
    class P(ctypes.Structure):
        _fields_ = [("nlvl", ctypes.c_int), ("stride", ctypes.c_int * 8), ("short_side", ctypes.c_int * 8),
                    ("long_side", ctypes.c_int * 8), ("n_scales", ctypes.c_int), ("n_aspects", ctypes.c_int),
                    ("scales", ctypes.c_double * 16), ("aspects", ctypes.c_double * 16),
                    ("allowed_border", ctypes.c_int), ("pos_thr", ctypes.c_float), ("neg_thr", ctypes.c_float),
                    ("min_pos_thr", ctypes.c_float), ("image_anchor", ctypes.c_int),
                    ("pos_fraction", ctypes.c_double)]
    p = P()
    p.nlvl, p.n_scales, p.n_aspects = len(cfg["stride"]), len(cfg["scales"]), len(cfg["aspects"])
    for i in range(p.nlvl):
        p.stride[i], p.short_side[i], p.long_side[i] = cfg["stride"][i], cfg["short"][i], cfg["long"][i]
    for i, v in enumerate(cfg["scales"]):
        p.scales[i] = v
    for i, v in enumerate(cfg["aspects"]):
        p.aspects[i] = v
    p.allowed_border, p.pos_thr, p.neg_thr, p.min_pos_thr = cfg["allowed_border"], cfg["pos_thr"], cfg["neg_thr"], \
        cfg["min_pos_thr"]
    return p


# ------------------------------------------------------------------------------------------ CPU --
def test_hand_case_known_answer():
    """One level, stride 16, one 32 x 32 anchor per cell: base anchor [-8, -8, 23, 23], cells (y, x) of a
    2 x 3 grid.  The gt box [8, 8, 39, 39] class 3 IS the anchor of cell (1, 1): IoU 1 -> label 3,
    weight 1.  Its x / y neighbours share 16 x 32 of 32 x 32: IoU 512 / 1536 = 1/3 < 0.4 -> 0; the
    diagonal ones 256 / 1792 -> 0.  Every anchor (all are valid) is encoded against the box: centre
    offsets of +16 / 0 / -16 pixels over a 32-pixel anchor, log(32 / 32) = 0."""
    k = "hand/0/"
    np.testing.assert_array_equal(GOLD[k + "label_flat"], [0, 0, 0, 0, 3, 0])
    np.testing.assert_array_equal(GOLD[k + "label"], [0, 0, 0, 0, 3, 0])  # A = 1: the same order
    want = np.float32([[.5, .5, 0, 0], [0, .5, 0, 0], [-.5, .5, 0, 0], [.5, 0, 0, 0], [0, 0, 0, 0], [-.5, 0, 0, 0]])
    np.testing.assert_array_equal(GOLD[k + "target_flat"], want)
    np.testing.assert_array_equal(GOLD[k + "target"], want.T)             # (4A, fh * fw)
    w = np.zeros((6, 4), np.float32)
    w[4] = 1
    np.testing.assert_array_equal(GOLD[k + "weight_flat"], w)
    assert float(GOLD[k + "fg_count"][0]) == 1.0
    # the indexing helper the GPU test relies on
    cfg = retinacases.CASES["hand"]["cfg"]
    im_info = retinacases.inputs(retinacases.CASES["hand"])[0][0]
    np.testing.assert_array_equal(retinacases.to_flat(cfg, im_info, GOLD[k + "target"], 4), want)


def test_tie_case_last_gt_gives_the_class_first_gives_the_target():
    """Anchors [-8,..], [8,..], [24,..] (32 wide), gt 0 = [0, 31] class 5, gt 1 = [16, 47] class 9: every
    anchor-gt pair that overlaps shares 24 of 32 columns (IoU 0.6 < pos_thr 0.9), so the middle anchor
    ties BOTH per-gt maxima: np.where's last pair (gt 1) gives class 9, argmax (first maximum, gt 0)
    gives the target: (15.5 - 23.5) / 32 = -0.25."""
    k = "hand_tie/0/"
    np.testing.assert_array_equal(GOLD[k + "label_flat"], [5, 9, 9])
    np.testing.assert_array_equal(GOLD[k + "target_flat"][:, 0], np.float32([0.25, -0.25, -0.25]))
    assert float(GOLD[k + "fg_count"][0]) == 3.0


def test_quirks_are_in_the_fixture():
    # a gt nothing overlaps, min_pos_thr = 0: every valid zero-overlap anchor takes its class (7)
    lab = GOLD["cfg_zero_overlap_gt/0/label"]
    assert (lab == 7).sum() > 150000 and float(GOLD["cfg_zero_overlap_gt/0/fg_count"][0]) == (lab > 0).sum()
    # duplicated boxes: anchors at a per-gt maximum below pos_thr take the LAST copy's class (7, never 4);
    # anchors at or above pos_thr take the FIRST copy's (5, never 8: arg-max is the first maximum)
    lab = GOLD["cfg_duplicate_gt_holes/0/label"]
    assert (lab == 7).sum() > 0 and (lab == 4).sum() == 0 and (lab == 5).sum() > 0 and (lab == 8).sum() == 0
    # no gt: 0 on every valid anchor, fg_count is max(1, 0)
    assert not GOLD["cfg_nogt/0/label"].any() and float(GOLD["cfg_nogt/0/fg_count"][0]) == 1.0
    # allowed_border = 0 leaves invalid anchors
    assert (GOLD["cfg_thr_border0/0/label"] == -1).sum() > 20000


def _call(cfg=retinacases.HAND, *, B=1, M=4, layout=1, ws=None, wsb=0, ptr=1, aligned=True, param=True):
    p = ctypes.c_void_p(256) if ptr else None  # never dereferenced: every case fails validation first
    out = p if aligned else ctypes.c_void_p(260)
    return _lib.lib().call("sd_retina_anchor_target", p, p, B, M, ctypes.byref(_param_struct(cfg)) if param else None,
                           p, out, out, p, layout, ws, ctypes.c_size_t(wsb), None)


def test_rejects_bad_arguments_and_small_workspace():
    with pytest.raises(_lib.SimpleDetOpsError, match="param is null"):
        _call(param=False)
    with pytest.raises(_lib.SimpleDetOpsError, match="bad B / M"):
        _call(B=-1)
    with pytest.raises(_lib.SimpleDetOpsError, match="bad B / M"):
        _call(M=-1)
    with pytest.raises(_lib.SimpleDetOpsError, match="layout must be"):
        _call(layout=2)
    with pytest.raises(_lib.SimpleDetOpsError, match="too many gt boxes"):
        _call(M=3277)
    with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
        _call(ptr=0)
    with pytest.raises(_lib.SimpleDetOpsError, match="16-B aligned"):
        _call(aligned=False)
    with pytest.raises(_lib.SimpleDetOpsError, match="scales x aspects"):
        _call(dict(retinacases.HAND, scales=tuple(range(1, 7)), aspects=(0.5, 1.0, 2.0)))
    with pytest.raises(_lib.SimpleDetOpsError, match="too many anchors"):
        _call(dict(retinacases.HAND, short=(20000,), long=(20000,)))
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
        _call(ws=ctypes.c_void_p(256), wsb=64)
    assert e.value.code == -4
    assert _call(B=0, ptr=0) == 0   # accepted without touching the device
    l = _lib.lib()
    l.cdll.sd_retina_target_workspace_bytes.restype = ctypes.c_size_t
    n = int(l.cdll.sd_retina_target_workspace_bytes(ctypes.byref(_param_struct(retinacases.RETINA)), 2, 100))
    assert 2 * 200700 * 9 <= n < 2 * 200700 * 9 + (1 << 16)   # max / arg-max / flag per anchor


# ------------------------------------------------------------------------------------------ GPU --
def _check(name, i, layout, cls, tgt, wgt, fg):
    k = "%s/%d/" % (name, i)
    sfx = "" if layout == 1 else "_flat"
    cls, tgt, wgt = cls.cpu().numpy(), tgt.cpu().numpy(), wgt.cpu().numpy()
    np.testing.assert_array_equal(cls, GOLD[k + "label" + sfx].astype(np.float32), err_msg=name + " labels")
    assert float(fg) == float(GOLD[k + "fg_count"][0]), name + " fg_count"
    if layout == 0:  # reg_weight = 1 exactly where label >= 1 (:70)
        np.testing.assert_array_equal(wgt, np.repeat((cls >= 1).astype(np.float32)[:, None], 4, 1), err_msg=name)
    if k + "target" in GOLD.files:
        np.testing.assert_array_equal(tgt, GOLD[k + "target" + sfx], err_msg=name + " targets")
        np.testing.assert_array_equal(wgt, GOLD[k + "weight" + sfx], err_msg=name + " weights")
    else:
        if layout == 0:  # a readable diff first: every 53rd row is stored in full
            np.testing.assert_array_equal(tgt[::53], GOLD[k + "target_flat_sample"], err_msg=name + " target rows")
        assert _sha(tgt) == bytes(GOLD[k + "target" + sfx + "_sha256"]), name + " targets (sha-256 of the bytes)"
        assert _sha(wgt) == bytes(GOLD[k + "weight" + sfx + "_sha256"]), name + " weights (sha-256 of the bytes)"


def _param(ops, cfg):
    return ops.rpn_target_param(cfg["stride"], cfg["short"], cfg["long"], cfg["scales"], cfg["aspects"],
                                cfg["allowed_border"], cfg["pos_thr"], cfg["neg_thr"], cfg["min_pos_thr"])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 0])
@pytest.mark.parametrize("name", sorted(retinacases.CASES))
def test_hip_reproduces_reference(ops, name, layout):
    import torch
    case = retinacases.CASES[name]
    p = _param(ops, case["cfg"])
    for i, (im_info, gt) in enumerate(retinacases.inputs(case)):
        cls, tgt, wgt, fg = ops.retina_anchor_target(torch.from_numpy(im_info[None]).cuda(),
                                                     torch.from_numpy(gt[None]).cuda(), p, layout=layout)
        _check(name, i, layout, cls[0], tgt[0], wgt[0], fg[0])


@pytest.mark.gpu
def test_hip_batch_of_two_orientations_and_layout_permutation(ops):
    """B = 2 with a landscape and a padded-hole image in one call equals the fixtures image by image,
    and layout 0 is layout 1 re-indexed."""
    import torch
    names = ["cfg_landscape", "cfg_duplicate_gt_holes"]
    ins = [retinacases.inputs(retinacases.CASES[n])[0] for n in names]
    im = torch.from_numpy(np.stack([x[0] for x in ins])).cuda()
    gt = torch.from_numpy(np.stack([x[1] for x in ins])).cuda()
    p = _param(ops, retinacases.RETINA)
    out1 = ops.retina_anchor_target(im, gt, p, layout=1)
    out0 = ops.retina_anchor_target(im, gt, p, layout=0)
    for b, n in enumerate(names):
        _check(n, 0, 1, out1[0][b], out1[1][b], out1[2][b], out1[3][b])
        _check(n, 0, 0, out0[0][b], out0[1][b], out0[2][b], out0[3][b])
        np.testing.assert_array_equal(retinacases.to_flat(retinacases.RETINA, ins[b][0], out1[1][b].cpu().numpy(), 4),
                                      out0[1][b].cpu().numpy())
        np.testing.assert_array_equal(retinacases.to_flat(retinacases.RETINA, ins[b][0], out1[0][b].cpu().numpy(), 1),
                                      out0[0][b].cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [1, 0])
def test_hip_graph_capture_and_replay(ops, layout):
    """the same bits come out of a captured graph, replayed twice over poisoned outputs"""
    import torch
    name = "cfg_portrait"
    im_info, gt = retinacases.inputs(retinacases.CASES[name])[0]
    im, g = torch.from_numpy(im_info[None]).cuda(), torch.from_numpy(gt[None]).cuda()
    p = _param(ops, retinacases.RETINA)
    B, M = 1, gt.shape[0]
    ws = torch.empty(int(_lib.lib().cdll.sd_retina_target_workspace_bytes(ctypes.byref(p), B, M)), dtype=torch.uint8,
                     device="cuda")
    ops.retina_anchor_target(im, g, p, layout=layout, workspace=ws)   # warm-up outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            out = ops.retina_anchor_target(im, g, p, layout=layout, workspace=ws)
    for _ in range(2):
        for t in out:
            t.fill_(float("nan"))
        ws.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        _check(name, 0, layout, out[0][0], out[1][0], out[2][0], out[3][0])
