"""_contrib_Proposal_v2 (TridentNet) and _contrib_Proposal (simpledet_amd/csrc/nms.hip, sd_proposal_v2 /
sd_proposal): argument validation and the hand-worked restatement without a GPU, and bit-exact
forwards against the numpy restatement of the .cu (tests/proposal_ref.py) on the GPU, including
the cut inside a long run of rows filtered to -1 on both top-k paths, graph capture and replay, and
the TridentNet Proposal_v2 -> ProposalTarget_v2 chain.  The restatement itself is held to the
reference's .cu run through the MXNet stand-in and to its Python twins (tests/golden/proposal_ref.npz,
made by tests/golden/make_golden_proposal.py)."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

from simpledet_amd import _lib

from . import proposal_ref as pr

f32 = np.float32
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "proposal_ref.npz")


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32)


def _call_v2(*, B=1, A=15, H=50, W=75, pre=12000, post=500, ws=None, wsb=0, fs=1):
    p = ctypes.c_void_p(16)  # never dereferenced: every case fails validation first
    sc = (ctypes.c_float * 5)(2, 4, 8, 16, 32)
    ra = (ctypes.c_float * 3)(0.5, 1, 2)
    return _lib.lib().call("sd_proposal_v2", p, p, p, p, p, p, B, A, H, W, pre, post, 0.7, 0, sc,
                           5, ra, 3, 16, fs, 0, ws, ctypes.c_size_t(wsb), None)


def _call_v1(*, B=1, A=15, H=50, W=75, pre=12000, post=500, ws=None, wsb=0, is_train=1):
    p = ctypes.c_void_p(16)
    sc = (ctypes.c_float * 5)(2, 4, 8, 16, 32)
    ra = (ctypes.c_float * 3)(0.5, 1, 2)
    return _lib.lib().call("sd_proposal", p, p, p, p, p, B, A, H, W, pre, post, 0.7, 0, sc, 5, ra,
                           3, 16, is_train, 0, ws, ctypes.c_size_t(wsb), None)


# ------------------------------------------------------------------------------------------------
# CPU: validation of the C entry points (all of these fail before any launch)
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", [_call_v2, _call_v1])
def test_refusals(call):
    # post > min(pre, count): the reference writes image i at stride min(post, pre)
    with pytest.raises(_lib.SimpleDetOpsError, match="rpn_post_nms_top_n=501 > min") as e:
        call(pre=500, post=501)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="rpn_post_nms_top_n=16 > min") as e:
        call(H=1, W=1, pre=-1, post=16)  # count = 15
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="exceeds 16384") as e:
        call(pre=16385, post=300)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="too many anchors") as e:
        call(H=1100, W=1100, pre=6000, post=300)  # 15 * 1100^2 >= 2^24
    assert e.value.code == -1  # SD_ERR_INVALID_ARG
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
        call(ws=ctypes.c_void_p(256), wsb=1024)
    assert e.value.code == -4  # SD_ERR_WORKSPACE


def test_v1_test_mode_keeps_post_past_pre():
    """proposal.cu:453-455: in test mode post stays as given (stride post, zero tail), so post > pre
    is not refused; the call gets as far as the workspace check."""
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
        _call_v1(pre=500, post=501, is_train=0)


def test_workspace_holds_the_tie_histograms():
    """v1 / v2 add B x G x 256 ints (G = ceil(count / 2048) chunks, at most 128) to Proposal_v3's
    layout, which is unchanged; a v3-sized workspace is too small for them."""
    l = _lib.lib().cdll
    for name in ("sd_proposal_v2_workspace_bytes", "sd_proposal_workspace_bytes",
                 "sd_proposal_v3_workspace_bytes"):
        getattr(l, name).restype = ctypes.c_size_t
    B, count = 6, 15 * 50 * 75
    G = min(128, (count + 2047) // 2048)
    a = l.sd_proposal_v2_workspace_bytes(B, 15, 50, 75, 12000)
    v3 = l.sd_proposal_v3_workspace_bytes(B, 15, 50, 75, 12000)
    assert a == l.sd_proposal_workspace_bytes(B, 15, 50, 75, 12000)
    assert a - v3 == (B * G * 1024 + 255) // 256 * 256
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
        _call_v2(B=B, ws=ctypes.c_void_p(256), wsb=v3)


def test_anchors_round_like_proposal_v2():
    """floor(x + 0.5f), not v3's rintf: stride 9, ratio 0.5 gives size_ratios 162, new_w 13 and
    13 * 0.5 = 6.5, which rounds to 7 here (rintf: 6)."""
    a = pr.anchors_v12(16, (2., 4., 8., 16., 32.), (0.5, 1., 2.))
    assert a.shape == (15, 4)
    np.testing.assert_array_equal(a[0], f32([-15.0, -4.0, 30.0, 19.0]))  # 46 x 24
    np.testing.assert_array_equal(a[5], f32([-8.0, -8.0, 23.0, 23.0]))    # ratio 1, scale 2
    b = pr.anchors_v12(9, (1.,), (0.5,))[0]
    assert b[2] - b[0] + 1 == 13 and b[3] - b[1] + 1 == 7
    c = pr.anchors_v12(3, (1.,), (2.,))[0]  # size 9, /2 -> floor 4, sqrt 2 -> w 2, 2*2 = 4
    assert c[2] - c[0] + 1 == 2 and c[3] - c[1] + 1 == 4


def _grid(A, H, W, score, deltas):
    cls = np.zeros((2 * A, H, W), f32)
    cls[A:] = np.asarray(score, f32).reshape(A, H, W)
    bbox = np.zeros((4 * A, H, W), f32)
    d = np.asarray(deltas, f32).reshape(H, W, A, 4)
    for a in range(A):
        for j in range(4):
            bbox[4 * a + j] = d[:, :, a, j]
    return cls, bbox


# hand-worked 2x3 grid, one 16x16 anchor (0, 0, 15, 15) per cell, iou_loss deltas move the corners;
# im_info (32, 40, 2): real_h = 2, real_w = 2, min_size = 2 * 2 = 4; valid range (10, 15): area in
# [100, 225]
KA_SCORE = [[0.9, 0.8, 0.95], [0.7, 0.6, 0.5]]
KA_DELTA = [[[0, 0, -4, -4], [0, 0, -14, 0], [0, 0, 0, 0]],
            [[0, 0, -7, -7], [0, 0, 0, 0], [0, 0, 0, 0]]]
KA_BOXES = [[0, 0, 11, 11],      # 12 x 12 = 144: kept, score 0.9
            [14, -2, 19, 17],    # (16,0,17,15): width 2 < 4 -> grown by 2 per side, -1
            [32, 0, 39, 15],     # w = 2 >= real_w: -1 (clipped to x <= 39, area 128 in range)
            [0, 16, 8, 24],      # 9 x 9 = 81 < 100: -1 (scale filter, below)
            [16, 16, 31, 31],    # 256 > 225: -1 (scale filter, above)
            [32, 16, 39, 31]]    # past the unpadded image: -1
KA_SC = [0.9, -1, -1, -1, -1, -1]


def test_known_answer_filters():
    cls, bbox = _grid(1, 2, 3, KA_SCORE, KA_DELTA)
    kw = dict(feature_stride=16, scales=(1.,), ratios=(1.,), rpn_min_size=2, iou_loss=True)
    boxes, sc = pr.decode(cls, bbox, f32([32, 40, 2]), valid_range=(10, 15), filter_scales=True,
                          **kw)
    np.testing.assert_array_equal(boxes, f32(KA_BOXES))
    np.testing.assert_array_equal(sc, f32(KA_SC))
    # without filter_scales rows 3 and 4 keep their scores (and v1 has no scale filter)
    _, sc1 = pr.decode(cls, bbox, f32([32, 40, 2]), **kw)
    np.testing.assert_array_equal(sc1, f32([0.9, -1, -1, 0.7, 0.6, -1]))
    # the whole op: the -1 rows follow in row order and are emitted (nothing overlaps > 0.7)
    out, score, src = pr.proposal_image(cls, bbox, f32([32, 40, 2]), 6, 6, 0.7, 2, (1.,), (1.,), 16,
                                        True, (10, 15), True)
    np.testing.assert_array_equal(src, [0, 1, 2, 3, 4, 5])
    np.testing.assert_array_equal(out, f32(KA_BOXES))
    np.testing.assert_array_equal(score, f32(KA_SC))


# 1x3 grid, im_info (16, 48, 1): box 1 has IoU exactly 0.5 with box 0 (72 / 144) and is kept by
# the strict > ; box 2 equals box 0 and is suppressed
KB_SCORE = [[0.9, 0.8, 0.7]]
KB_DELTA = [[[0, 0, -4, -4], [-16, 0, -20, -10], [-32, 0, -36, -4]]]


def _kb():
    return _grid(1, 1, 3, KB_SCORE, KB_DELTA)


def test_known_answer_nms_at_threshold_and_v1_padding():
    cls, bbox = _kb()
    args = (f32([16, 48, 1]), 3, 3, 0.5, 0, (1.,), (1.,), 16, True)
    out, score, src = pr.proposal_image(cls, bbox, *args, None, False, True)
    np.testing.assert_array_equal(src, [0, 1, 0])  # is_train: cyclic
    np.testing.assert_array_equal(out, f32([[0, 0, 11, 11], [0, 0, 11, 5], [0, 0, 11, 11]]))
    np.testing.assert_array_equal(score, f32([0.9, 0.8, 0.9]))
    out, score, src = pr.proposal_image(cls, bbox, *args, None, False, False)
    np.testing.assert_array_equal(src, [0, 1, -1])  # test / v2: zeros
    np.testing.assert_array_equal(out[2], f32([0, 0, 0, 0]))
    assert score[2] == 0
    b = f32([[0, 0, 11, 11], [0, 0, 11, 5]])
    assert pr.iou_row(b[0], b[1:])[0] == f32(0.5)


def test_known_answer_bbox_pred_has_no_clamp():
    """dw = 5 is past v3's clamp (4.1352): the v1/v2 decode uses it as it is."""
    cls, bbox = _grid(1, 1, 1, [[0.9]], [[[0.5, 0, 5, 0]]])
    boxes, sc = pr.decode(cls, bbox, f32([4000, 4000, 1]), 16, (1.,), (1.,), 0)
    pw = np.exp(np.float64(5)).astype(f32) * f32(16)
    assert boxes[0, 0] == f32(0)  # 15.5 - 0.5 * (pw - 1) < 0 -> clipped
    assert boxes[0, 2] == f32(15.5) + f32(0.5) * (pw - f32(1))
    assert boxes[0, 2] > 1000 and boxes[0, 1] == 0 and boxes[0, 3] == 15 and sc[0] == f32(0.9)


def test_sort_key_orders_nan_by_bits():
    s = f32([0.5, np.nan, -np.nan, np.inf, -np.inf, -0.0, 0.0, -1.0])
    order = np.argsort(pr.sort_key(s), kind="stable")
    np.testing.assert_array_equal(order, [1, 3, 0, 5, 6, 7, 4, 2])


# ------------------------------------------------------------------------------------------------
# GPU: bit-exact against the restatement
# ------------------------------------------------------------------------------------------------
def _t(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check_v2(cls, bbox, im, vr, **kw):
    from simpledet_amd import ops
    o, s = ops.proposal_v2(_t(cls), _t(bbox), _t(im), _t(vr), **kw)
    wo, ws = pr.proposal_v2(cls, bbox, im, vr, **kw)
    o, s = o.cpu().numpy(), s.cpu().numpy()
    assert o.shape == wo.shape and s.shape == ws.shape
    np.testing.assert_array_equal(_bits(s), _bits(ws))
    np.testing.assert_array_equal(_bits(o), _bits(wo))
    return o, s


def _check_v1(cls, bbox, im, **kw):
    from simpledet_amd import ops
    o, s = ops.proposal(_t(cls), _t(bbox), _t(im), **kw)
    wo, ws = pr.proposal(cls, bbox, im, **kw)
    o, s = o.cpu().numpy(), s.cpu().numpy()
    assert o.shape == wo.shape and s.shape == ws.shape
    np.testing.assert_array_equal(_bits(s), _bits(ws))
    np.testing.assert_array_equal(_bits(o), _bits(wo))
    return o, s


def _trident(seed, B=6, H=50, W=75, **kw):
    cls, bbox, im = pr.rpn_inputs(seed, B, 15, H, W, **kw)
    vr = np.asarray([pr.TRIDENT_RANGES[i % 3] for i in range(B)], f32)
    return cls, bbox, im, vr


@pytest.fixture
def topk_mode():
    """topk_mode(m): the rest of the test runs under proposal_topk = m"""
    from simpledet_amd._lib import lib
    with contextlib.ExitStack() as stack:
        yield lambda m: stack.enter_context(lib().tuned(proposal_topk=m))


@pytest.mark.gpu
@pytest.mark.parametrize("post,filter_scales", [(500, True), (500, False), (300, True)])
def test_tridentnet_train_and_test_shapes(post, filter_scales):
    """train: pre 12000 / post 500; test: pre 6000 / post 300 (config/tridentnet_*: RPN test)."""
    cls, bbox, im, vr = _trident(1)
    pre = 12000 if post == 500 else 6000
    _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=pre, rpn_post_nms_top_n=post,
              filter_scales=filter_scales, **pr.TRIDENT)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_cut_inside_a_long_minus_one_run(topk_mode, mode):
    """A narrow valid range filters all but a few thousand rows: the top-12000 cut falls inside a
    run of > 40000 rows tied at -1, on the single- (1) and the multi-workgroup (2) select."""
    topk_mode(mode)
    cls, bbox, im, vr = _trident(2, B=2)
    vr[:] = f32([[40, 60], [100, 130]])
    boxes, sc = pr.decode(cls[0], bbox[0], im[0], 16, pr.TRIDENT["scales"], pr.TRIDENT["ratios"], 0,
                          False, vr[0], True)
    n_tied = int((sc == -1).sum())
    assert n_tied > 40000 and (sc != -1).sum() < 12000
    _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=12000, rpn_post_nms_top_n=500,
              filter_scales=True, **pr.TRIDENT)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_ties_on_real_scores_straddle_the_cut(topk_mode, mode):
    topk_mode(mode)
    cls, bbox, im, vr = _trident(3, B=2, ties=0.6)
    _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
              filter_scales=False, **pr.TRIDENT)


@pytest.mark.gpu
def test_every_row_filtered():
    cls, bbox, im, vr = _trident(4, B=2)
    vr[:] = f32([[5000, 6000], [0, 1]])
    _, s = _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=300,
                     filter_scales=True, **pr.TRIDENT)
    assert (s == -1).all()


@pytest.mark.gpu
def test_padded_images():
    """im_info below H*stride: the anchors past the unpadded image score -1; an image taller than
    H*stride marks none (the reference aborts there)."""
    cls, bbox, im, vr = _trident(5, B=3)
    im[0, :2] = (600, 1000)
    im[1, :2] = (803, 1199)
    im[2, :2] = (900, 1300)  # > 50*16 x 75*16
    _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=12000, rpn_post_nms_top_n=500,
              filter_scales=True, **pr.TRIDENT)
    _check_v1(cls, bbox, im, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, is_train=False,
              **pr.TRIDENT)


@pytest.mark.gpu
def test_min_size_with_scale():
    cls, bbox, im, vr = _trident(6, B=2, H=38, W=50, delta_scale=0.8)
    im[:, 2] = (1.5, 0.75)
    kw = dict(pr.TRIDENT, rpn_min_size=16)
    _, s = _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
                     filter_scales=True, **kw)
    _check_v1(cls, bbox, im, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, is_train=True, **kw)


@pytest.mark.gpu
def test_nan_rule():
    cls, bbox, im, vr = _trident(7, B=2, H=20, W=30)
    rs = np.random.RandomState(7)
    fg = cls[:, 15:]
    fg.reshape(-1)[rs.choice(fg.size, 50, replace=False)] = np.nan
    fg.reshape(-1)[rs.choice(fg.size, 20, replace=False)] = -np.nan
    bbox.reshape(-1)[rs.choice(bbox.size, 200, replace=False)] = np.nan
    bbox.reshape(-1)[rs.choice(bbox.size, 50, replace=False)] = np.inf
    _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=3000, rpn_post_nms_top_n=300,
              filter_scales=True, **pr.TRIDENT)
    _check_v1(cls, bbox, im, rpn_pre_nms_top_n=3000, rpn_post_nms_top_n=300, is_train=True,
              **pr.TRIDENT)


@pytest.mark.gpu
def test_iou_loss():
    cls, bbox, im, vr = _trident(8, B=2, H=30, W=40, delta_scale=8.0)
    _check_v2(cls, bbox, im, vr, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
              filter_scales=True, iou_loss=True, **pr.TRIDENT)
    _check_v1(cls, bbox, im, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, is_train=True,
              iou_loss=True, **pr.TRIDENT)


@pytest.mark.gpu
@pytest.mark.parametrize("is_train", [True, False])
def test_v1_padding(is_train):
    """Few boxes survive NMS (a tiny image clips every box to a few pixels): the tail is the kept
    boxes repeated (is_train) or zeros."""
    cls, bbox, im = pr.rpn_inputs(9, 2, 9, 20, 30)
    im[:, :2] = (40, 60)
    o, s = _check_v1(cls, bbox, im, rpn_pre_nms_top_n=2000, rpn_post_nms_top_n=1000,
                     is_train=is_train, threshold=0.5, rpn_min_size=0, scales=(8., 16., 32.))
    assert (s[:, -1, 0] != 0).all() == is_train


@pytest.mark.gpu
def test_known_answer_cases_on_device():
    from simpledet_amd import ops
    cls, bbox = _grid(1, 2, 3, KA_SCORE, KA_DELTA)
    o, s = ops.proposal_v2(_t(cls[None]), _t(bbox[None]), _t(f32([[32, 40, 2]])), _t(f32([[10, 15]])),
                           6, 6, 0.7, 2, (1.,), (1.,), 16, True, True)
    np.testing.assert_array_equal(o.cpu().numpy()[0], f32(KA_BOXES))
    np.testing.assert_array_equal(s.cpu().numpy()[0, :, 0], f32(KA_SC))
    cls, bbox = _kb()
    o, s = ops.proposal(_t(cls[None]), _t(bbox[None]), _t(f32([[16, 48, 1]])), 3, 3, 0.5, 0, (1.,),
                        (1.,), 16, True, True)
    np.testing.assert_array_equal(s.cpu().numpy()[0, :, 0], f32([0.9, 0.8, 0.9]))


@pytest.mark.gpu
def test_v1_test_mode_post_past_pre_zero_pads():
    cls, bbox, im = pr.rpn_inputs(12, 2, 15, 4, 5)  # count = 300
    o, s = _check_v1(cls, bbox, im, rpn_pre_nms_top_n=200, rpn_post_nms_top_n=400, is_train=False,
                     **pr.TRIDENT)
    assert o.shape == (2, 400, 4) and (s[:, 200:] == 0).all()


# ------------------------------------------------------------------------------------------------
# the restatement against the reference's .cu run through the stand-in, and its Python twins
# ------------------------------------------------------------------------------------------------
def _golden():
    from .golden import make_golden_proposal as g
    return g, np.load(GOLDEN)


def _restate(g, name):
    op, cls, bbox, im, vr, p = g.case_inputs(name)
    if op == "v2":
        return (cls, bbox, im, vr, p), pr.proposal_v2(cls, bbox, im, vr, **p)
    return (cls, bbox, im, None, p), pr.proposal(cls, bbox, im, **p)


def _golden_equal(got_o, got_s, ref_o, ref_s):
    """scores and order bit-equal; boxes within the 1-ulp expf of the stand-in's emulation"""
    assert got_o.shape == ref_o.shape and got_s.shape == ref_s.shape
    np.testing.assert_array_equal(_bits(got_s), _bits(ref_s))
    np.testing.assert_allclose(got_o, ref_o, rtol=2.5e-7, atol=0)


def test_restatement_matches_reference_run():
    g, z = _golden()
    names = sorted(k[:-4] for k in z.files if k.endswith("/out"))
    assert set(names) == set(g.CASES)
    straddle = 0
    for name in names:
        (cls, bbox, im, vr, p), (wo, ws) = _restate(g, name)
        _golden_equal(wo, ws, z[name + "/out"], z[name + "/score"])
        if name == "trident_ranges":  # the -1 run straddles pre in at least one image
            for b in range(cls.shape[0]):
                _, sc = pr.decode(cls[b], bbox[b], im[b], 16, p["scales"], p["ratios"], 0, False,
                                  vr[b], True)
                straddle += (sc != -1).sum() < p["rpn_pre_nms_top_n"] <= len(sc)
    assert straddle >= 1
    af = z["all_filtered/score"]  # every emitted row scores -1, the tail is zero padding
    assert (af == -1).any() and ((af == -1) | (af == 0)).all()
    v1t, v1e = z["v1_train/score"], z["v1_test/score"]
    assert (v1e[:, -1] == 0).all() and (v1t[:, -1] != 0).all()


def test_restatement_matches_python_twins():
    """unfiltered path: nonlinear_pred + clip_boxes + nms (ovr <= thresh kept) of the reference; the
    twin runs in float64, so rows must agree and boxes within float32 rounding of the decode."""
    g, z = _golden()
    t = g.TWIN
    cls, bbox, im = g.twin_inputs()
    _, _, src = pr.proposal_image(cls[0], bbox[0], im[0], t["pre"], t["post"], t["thr"], 0,
                                  t["scales"], t["ratios"], t["stride"])
    out, score, _ = pr.proposal_image(cls[0], bbox[0], im[0], t["pre"], t["post"], t["thr"], 0,
                                      t["scales"], t["ratios"], t["stride"])
    n = len(z["twin/rows"])
    assert n == t["post"] and (src >= 0).all()
    np.testing.assert_array_equal(src, z["twin/rows"])
    np.testing.assert_allclose(out, z["twin/boxes"], rtol=0, atol=1e-3)
    np.testing.assert_array_equal(score, z["twin/score"].astype(f32))


@pytest.mark.gpu
def test_reference_run_fixture_on_device():
    from simpledet_amd import ops
    g, z = _golden()
    for name in g.CASES:
        op, cls, bbox, im, vr, p = g.case_inputs(name)
        if op == "v2":
            o, s = ops.proposal_v2(_t(cls), _t(bbox), _t(im), _t(vr), **p)
        else:
            o, s = ops.proposal(_t(cls), _t(bbox), _t(im), **p)
        _golden_equal(o.cpu().numpy(), s.cpu().numpy(), z[name + "/out"], z[name + "/score"])
    t = g.TWIN
    cls, bbox, im = g.twin_inputs()
    o, s = ops.proposal(_t(cls), _t(bbox), _t(im), t["pre"], t["post"], t["thr"], 0, t["scales"],
                        t["ratios"], t["stride"], is_train=False)
    np.testing.assert_allclose(o.cpu().numpy()[0], z["twin/boxes"], rtol=0, atol=1e-3)


@pytest.mark.gpu
def test_graph_capture_and_side_stream():
    """Two replays of a captured graph at the TridentNet train shape (multi-workgroup select, 128 KB
    LDS sort): the top-k counters must be zeroed in every replay."""
    import torch
    from simpledet_amd import ops
    cls, bbox, im, vr = _trident(10)
    vr[:3] = f32([[40, 60], [100, 130], [20, 30]])  # images 0-2: the cut inside the -1 run
    tc, tb, ti, tv = _t(cls), _t(bbox), _t(im), _t(vr)
    kw = dict(rpn_pre_nms_top_n=12000, rpn_post_nms_top_n=500, filter_scales=True, **pr.TRIDENT)
    wo, ws = pr.proposal_v2(cls, bbox, im, vr, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eo, es = ops.proposal_v2(tc, tb, ti, tv, **kw)  # warm-up (kernel attributes) off-graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_bits(eo.cpu().numpy()), _bits(wo))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o, s = ops.proposal_v2(tc, tb, ti, tv, **kw)
    for _ in range(2):
        o.zero_()
        s.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_bits(o.cpu().numpy()), _bits(wo))
        np.testing.assert_array_equal(_bits(s.cpu().numpy()), _bits(ws))


@pytest.mark.gpu
def test_tridentnet_chain_proposal_v2_to_proposal_target_v2(oracle):
    """Proposal_v2 -> ProposalTarget_v2 (filter_scales) captured as one graph, equal to the
    restatement -> oracle.proposal_target_v2."""
    import torch
    from simpledet_amd import ops
    B = 3
    cls, bbox, im, vr = _trident(11, B=B)
    rs = np.random.RandomState(11)
    M = 20
    xy = rs.uniform(0, 900, (B, M, 2)).astype(f32)
    wh = rs.uniform(8, 300, (B, M, 2)).astype(f32)
    gt = np.concatenate([xy, np.minimum(xy + wh, f32(799)), rs.randint(1, 81, (B, M, 1))], 2).astype(f32)
    kw = dict(rpn_pre_nms_top_n=12000, rpn_post_nms_top_n=500, filter_scales=True, **pr.TRIDENT)
    tc, tb, ti, tv, tg = _t(cls), _t(bbox), _t(im), _t(vr), _t(gt)
    rng0 = ops.glibc_rand_state(1)
    rng = rng0.clone()

    def step():
        rois, _ = ops.proposal_v2(tc, tb, ti, tv, **kw)
        return ops.proposal_target(rois, tg, 81, B, 128, rng_state=rng, valid_ranges=tv,
                                   filter_scales=True)
    step()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        got = step()
    wo, _ = pr.proposal_v2(cls, bbox, im, vr, **kw)
    p = oracle.make_pt_param(81, B, 128)
    want = oracle.proposal_target(wo, gt, p, rng=oracle.GlibcRand(1), valid_ranges=vr,
                                  filter_scales=True)
    assert want[-1] == 0
    for _ in range(2):
        rng.copy_(rng0)
        g.replay()
        torch.cuda.synchronize()
        for k, (gx, wx) in enumerate(zip(got, want[:5])):
            if k == 2:  # bbox_target: device logf, the bar of tests/test_train_chain.py
                np.testing.assert_allclose(gx.cpu().numpy(), wx, rtol=2e-6, atol=2e-6)
            else:
                np.testing.assert_array_equal(_bits(gx.cpu().numpy()), _bits(wx))
