"""_contrib_GenProposalRetina (simpledet_amd/csrc/gen_proposal_retina.hip): argument validation
without a GPU, and bit-exact forward against the numpy restatement of the .cu (tests/retina_ref.py)
on the GPU, including graph capture and the RetinaNet test chain."""
import ctypes
import os

import numpy as np
import pytest

from simpledet_amd import _lib

from . import retina_ref

STRIDES = (8, 16, 32, 64, 128)
SHAPES_800 = ((100, 167), (50, 84), (25, 42), (13, 21), (7, 11))  # P3-P7 of an 800x1333 image
SCALES = (4 * 2 ** 0, 4 * 2 ** (1.0 / 3.0), 4 * 2 ** (2.0 / 3.0))
RATIOS = (0.5, 1.0, 2.0)
A = 9
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "retina_decode.npz")


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _call(*, B=1, AK=720, H=4, W=5, A_=9, pre=100, min_size=0, thresh=0.05, iou=0, one_hot=1, bwa=0,
          ws=None, wsb=0, ptr=1):
    p = ctypes.c_void_p(16) if ptr else None  # never dereferenced: every case fails validation first
    f4 = (ctypes.c_float * 4)(0, 0, 0, 0)
    return _lib.lib().call("sd_gen_proposal_retina", p, p, p, p, p, p, B, AK, H, W, A_, pre, min_size,
                           float(thresh), f4, f4, iou, one_hot, bwa, ws, ctypes.c_size_t(wsb), None)


# ------------------------------------------------------------------------------------------------
# CPU: validation of the C entry point (no GPU needed: all of these fail before any launch)
# ------------------------------------------------------------------------------------------------
def test_refuses_reference_out_of_bounds_cases():
    with pytest.raises(_lib.SimpleDetOpsError, match="iou_loss needs one class") as e:
        _call(iou=1)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    with pytest.raises(_lib.SimpleDetOpsError, match="batch_wise_anchor") as e:
        _call(B=2, bwa=1)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED


def test_rejects_bad_arguments_and_small_workspace():
    with pytest.raises(_lib.SimpleDetOpsError, match="multiple of num_anchors"):
        _call(AK=721)
    with pytest.raises(_lib.SimpleDetOpsError, match="rpn_pre_nms_top_n must be > 0"):
        _call(pre=0)
    with pytest.raises(_lib.SimpleDetOpsError, match="thresh is NaN"):
        _call(thresh=float("nan"))
    with pytest.raises(_lib.SimpleDetOpsError, match="exceeds 16384"):
        _call(H=100, W=100, pre=20000)
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small") as e:
        _call(ws=ctypes.c_void_p(256), wsb=1024)
    assert e.value.code == -4
    # B = 0 is accepted without touching the device
    assert _call(B=0, ptr=0) == 0


def test_row_limit_is_enforced():
    # 2^28 rows per image is the stated limit: 720 channels x 611 x 611 = 268.8 M > 2^28
    with pytest.raises(_lib.SimpleDetOpsError, match="exceed the limit") as e:
        _call(H=611, W=611)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    # the largest reference level fits: P3 of a 1280x1280 NAS-FPN image, 160*160*720 = 18.4 M rows
    l = _lib.lib()
    l.cdll.sd_gen_proposal_retina_workspace_bytes.restype = ctypes.c_size_t
    n = int(l.cdll.sd_gen_proposal_retina_workspace_bytes(1, 720, 160, 160))
    assert 160 * 160 * 720 * 4 <= n < 160 * 160 * 720 * 4 + (1 << 20)
    with pytest.raises(_lib.SimpleDetOpsError, match="workspace too small"):
        _call(H=160, W=160, ws=ctypes.c_void_p(256), wsb=n // 2)


def test_known_answer_restatement():
    """H = W = 1, A = 1, K = 2: channels are (anchor 0, class 0), (anchor 0, class 1); rows 0, 1."""
    cls = np.array([0.3, 0.7], np.float32).reshape(1, 2, 1, 1)
    deltas = np.zeros((1, 4, 1, 1), np.float32)
    info = np.array([[100, 200, 1]], np.float32)
    anchors = np.array([[10, 20, 29, 59]], np.float32)
    out, score = retina_ref.gen_proposal_retina(cls, deltas, info, anchors, 1, rpn_pre_nms_top_n=3,
                                                rpn_min_size=0, thresh=0.05)
    # zero deltas decode to the anchor itself; order: class 1 (0.7) then class 0 (0.3), then padding
    np.testing.assert_array_equal(out[0], [[10, 20, 29, 59], [10, 20, 29, 59], [0, 0, 0, 0]])
    np.testing.assert_array_equal(score[0], np.float32([[0, 0, 0.7], [0, 0.3, 0], [0, 0, 0]]))
    _, s1 = retina_ref.gen_proposal_retina(cls, deltas, info, anchors, 1, rpn_pre_nms_top_n=3,
                                           rpn_min_size=0, thresh=0.05, output_one_hot=False)
    np.testing.assert_array_equal(s1[0], np.float32([[0.7], [0.3], [0]]))
    # thresh 0.5 zeroes row 0 (score and box); min size 25 zeroes both (box width 20 < 25)
    out, score = retina_ref.gen_proposal_retina(cls, deltas, info, anchors, 1, rpn_pre_nms_top_n=2,
                                                rpn_min_size=0, thresh=0.5)
    np.testing.assert_array_equal(score[0], np.float32([[0, 0, 0.7], [0, 0, 0]]))
    np.testing.assert_array_equal(out[0, 1], [0, 0, 0, 0])
    out, score = retina_ref.gen_proposal_retina(cls, deltas, info, anchors, 1, rpn_pre_nms_top_n=2,
                                                rpn_min_size=25, thresh=0.0)
    assert not out.any() and not score.any()
    # a delta of log(2) on w doubles the width about the centre 19.5: 40 wide -> x 0 .. 39
    deltas[0, 2] = np.float32(np.log(2.0))
    out, _ = retina_ref.gen_proposal_retina(cls, deltas, info, anchors, 1, rpn_pre_nms_top_n=1,
                                            rpn_min_size=0, thresh=0.0)
    np.testing.assert_allclose(out[0, 0], [0.0, 20, 39, 59], rtol=0, atol=1e-4)


def test_restatement_matches_decode_retina_fixture():
    """The reference's own Python twin (models/retinanet/decode_retina.py) on seeded 5-level inputs
    with continuous scores selects the same (anchor, class, y, x) per level, with the same scores and
    labels; boxes agree within the stated tolerance (the twin decodes in float64 / float32 numpy)."""
    g = np.load(GOLDEN)
    assert bool(g["anchors_equal_gen_anchor"])
    _check_against_fixture(g, lambda lvl, cls, dl, info, anc: retina_ref.gen_proposal_retina(
        cls, dl, info, anc, A, rpn_pre_nms_top_n=int(g["top_n"]), rpn_min_size=0,
        thresh=float(g["thresh"][lvl])))


def _check_against_fixture(g, run):
    top_n = int(g["top_n"])
    want_boxes, want_scores = g["boxes"][0], g["scores"][0]
    info = g["im_info"]
    row0 = 0
    for lvl, s in enumerate(g["strides"]):
        cls, dl = g["cls_%d" % s], g["bbox_%d" % s]
        anc = g["anchors_%d" % s]
        out, score = run(lvl, cls, dl, info, anc)
        out, score = np.asarray(out)[0], np.asarray(score)[0]
        n = int(g["count_%d" % s])
        # the twin's per-level rows come in argpartition order: compare as sets keyed by (label, score)
        wl = want_scores[row0:row0 + n].argmax(1)
        ws = want_scores[row0:row0 + n].max(1)
        wb = want_boxes[row0:row0 + n]
        gl = score[:n].argmax(1)
        gs = score[:n].max(1)
        assert not score[n:].any() and not out[n:].any()
        ko = np.lexsort((wl, -ws))
        kg = np.lexsort((gl, -gs))
        np.testing.assert_array_equal(gl[kg], wl[ko])
        np.testing.assert_array_equal(gs[kg], ws[ko].astype(np.float32))
        np.testing.assert_allclose(out[:n][kg], wb[ko], rtol=0, atol=float(g["box_atol"]))
        row0 += top_n


# ------------------------------------------------------------------------------------------------
# GPU
# ------------------------------------------------------------------------------------------------
def _level(rs, B, H, W, K=80, mu=-4.595, box_sd=0.2):
    cls = (1.0 / (1.0 + np.exp(-rs.normal(mu, 1.0, (B, A * K, H, W))))).astype(np.float32)
    dl = (rs.standard_normal((B, 4 * A, H, W)) * box_sd).astype(np.float32)
    return cls, dl


def _anchors(H, W, s):
    from oracle import pyoracle as orc
    return orc.gen_anchor(H, W, s, SCALES, RATIOS)


def _check(cls, dl, info, anc, num_anchors=A, **kw):
    import torch
    from simpledet_amd import ops
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    o, s = ops.gen_proposal_retina(t(cls), t(dl), t(info), t(anc), num_anchors=num_anchors, **kw)
    wo, ws = retina_ref.gen_proposal_retina(cls, dl, info, anc, num_anchors, **kw)
    o, s = o.cpu().numpy(), s.cpu().numpy()
    assert o.shape == wo.shape and s.shape == ws.shape
    np.testing.assert_array_equal(_bits(o), _bits(wo))
    np.testing.assert_array_equal(_bits(s), _bits(ws))
    return o, s


def _info(B, h=800, w=1333, scale=1.0):
    return np.tile(np.array([[h, w, scale]], np.float32), (B, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 2])
def test_five_levels_800x1333_bit_exact(B):
    rs = np.random.RandomState(10 + B)
    info = _info(B)
    for (H, W), s in zip(SHAPES_800, STRIDES):
        cls, dl = _level(rs, B, H, W)
        _, sc = _check(cls, dl, info, _anchors(H, W, s), rpn_pre_nms_top_n=1000, rpn_min_size=0,
                       thresh=0.0 if s == 128 else 0.05)
        assert (sc.max(2) > 0).sum() == B * 1000


@pytest.mark.gpu
@pytest.mark.parametrize("thresh", [0.05, 0.0, -0.1])
def test_thresholds_with_exact_zeros(thresh):
    rs = np.random.RandomState(3)
    H, W = 25, 42
    cls, dl = _level(rs, 2, H, W, mu=-1.0)
    cls = cls * np.where(rs.rand(*cls.shape) < 0.5, 1, -1).astype(np.float32)  # negative scores too
    cls.reshape(-1)[rs.choice(cls.size, 5000, replace=False)] = 0.0
    cls.reshape(-1)[rs.choice(cls.size, 5000, replace=False)] = -0.0
    for pre in (1000, 16384):
        _check(cls, dl, _info(2), _anchors(H, W, 32), rpn_pre_nms_top_n=pre, rpn_min_size=0,
               thresh=thresh)


@pytest.mark.gpu
def test_min_size_scale_mean_std():
    rs = np.random.RandomState(4)
    H, W = 50, 84
    cls, dl = _level(rs, 2, H, W, box_sd=1.0)
    info = np.array([[600, 1000, 1.5], [640, 660, 0.75]], np.float32)
    o, _ = _check(cls, dl, info, _anchors(H, W, 16), rpn_pre_nms_top_n=2000, rpn_min_size=16,
                  thresh=0.05, anchor_mean=(0.01, -0.02, 0.05, -0.05), anchor_std=(0.1, 0.1, 0.2, 0.2))
    assert o.any()


@pytest.mark.gpu
def test_one_hot_off_and_padding_rows():
    rs = np.random.RandomState(5)
    H, W = 7, 11
    cls, dl = _level(rs, 2, H, W, mu=0.0)
    anc = _anchors(H, W, 128)
    _, s = _check(cls, dl, _info(2), anc, rpn_pre_nms_top_n=1000, rpn_min_size=0, thresh=0.05,
                  output_one_hot=False)
    assert s.shape == (2, 1000, 1)
    cls2, dl2 = _level(rs, 2, H, W, K=2, mu=0.0)  # 1386 rows: rpn_pre_nms_top_n > count
    o, s = _check(cls2, dl2, _info(2), anc, rpn_pre_nms_top_n=H * W * A * 2 + 37, rpn_min_size=0,
                  thresh=0.0)
    assert o[:, :H * W * A * 2].any() and not o[:, H * W * A * 2:].any()


@pytest.mark.gpu
def test_every_row_filtered():
    rs = np.random.RandomState(6)
    H, W = 13, 21
    cls, dl = _level(rs, 1, H, W)
    o, s = _check(cls, dl, _info(1), _anchors(H, W, 64), rpn_pre_nms_top_n=1000, rpn_min_size=0,
                  thresh=1.0)
    assert not o.any() and not s.any()


@pytest.mark.gpu
def test_quantised_ties_straddle_the_cut_off():
    rs = np.random.RandomState(7)
    for (H, W), s in (((100, 167), 8), ((25, 42), 32), ((7, 11), 128)):
        cls, dl = _level(rs, 1, H, W, mu=-2.0)
        cls = np.floor(cls * 64) / np.float32(64)
        _check(cls, dl, _info(1), _anchors(H, W, s), rpn_pre_nms_top_n=1000, rpn_min_size=0,
               thresh=0.05)


@pytest.mark.gpu
def test_nan_scores_count_as_filtered():
    rs = np.random.RandomState(8)
    H, W = 25, 42
    cls, dl = _level(rs, 1, H, W, mu=-2.0)
    nan_at = rs.choice(cls.size, 20000, replace=False)
    cls.reshape(-1)[nan_at] = np.nan
    for thresh in (0.05, -0.1):
        o, s = _check(cls, dl, _info(1), _anchors(H, W, 32), rpn_pre_nms_top_n=1000, rpn_min_size=0,
                      thresh=thresh)
        assert np.isfinite(s).all() and np.isfinite(o).all()
    # the finite rows are exactly the op's selection on the same input with NaN replaced by 0
    c0 = np.nan_to_num(cls, nan=0.0)
    o0, s0 = _check(c0, dl, _info(1), _anchors(H, W, 32), rpn_pre_nms_top_n=1000, rpn_min_size=0,
                    thresh=0.05)
    o1, s1 = _check(cls, dl, _info(1), _anchors(H, W, 32), rpn_pre_nms_top_n=1000, rpn_min_size=0,
                    thresh=0.05)
    np.testing.assert_array_equal(o0, o1)
    np.testing.assert_array_equal(s0, s1)


@pytest.mark.gpu
def test_iou_loss_one_class_and_batch_wise_anchor():
    rs = np.random.RandomState(9)
    H, W = 20, 30
    cls, dl = _level(rs, 2, H, W, K=1, mu=-1.0, box_sd=3.0)
    anc = _anchors(H, W, 16)
    _check(cls, dl, _info(2), anc, rpn_pre_nms_top_n=500, rpn_min_size=4, thresh=0.05, iou_loss=True)
    banc = np.stack([anc, anc + np.float32(3.0)])
    _check(cls, dl, _info(2), banc, rpn_pre_nms_top_n=500, rpn_min_size=4, thresh=0.05,
           batch_wise_anchor=True)
    cls80, dl80 = _level(rs, 1, H, W)
    _check(cls80, dl80, _info(1), anc[None], rpn_pre_nms_top_n=500, rpn_min_size=0, thresh=0.05,
           batch_wise_anchor=True)


@pytest.mark.gpu
def test_decode_retina_fixture_on_device():
    import torch
    from simpledet_amd import ops
    g = np.load(GOLDEN)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731

    def run(lvl, cls, dl, info, anc):
        H, W = cls.shape[2:]
        ga = ops.gen_anchor(H, W, int(g["strides"][lvl]), SCALES, RATIOS)
        np.testing.assert_array_equal(ga.cpu().numpy(), anc)
        o, s = ops.gen_proposal_retina(t(cls), t(dl), t(info), ga, num_anchors=A,
                                       rpn_pre_nms_top_n=int(g["top_n"]), rpn_min_size=0,
                                       thresh=float(g["thresh"][lvl]))
        return o.cpu().numpy(), s.cpu().numpy()
    _check_against_fixture(g, run)


def _five_levels(ops, torch, cls_l, dl_l, info, anchors):
    outs = []
    for (cls, dl, anc, s) in zip(cls_l, dl_l, anchors, STRIDES):
        outs.append(ops.gen_proposal_retina(cls, dl, info, anc, num_anchors=A, rpn_pre_nms_top_n=1000,
                                            rpn_min_size=0, thresh=0.0 if s == 128 else 0.05))
    return outs


@pytest.mark.gpu
def test_graph_capture_and_side_stream():
    import torch
    from simpledet_amd import ops
    rs = np.random.RandomState(11)
    shapes = ((50, 84), (25, 42), (13, 21), (7, 11), (4, 6))
    lv = [_level(rs, 1, H, W) for H, W in shapes]
    cls_l = [torch.from_numpy(c).cuda() for c, _ in lv]
    dl_l = [torch.from_numpy(d).cuda() for _, d in lv]
    info = torch.from_numpy(_info(1, 512, 672)).cuda()
    anchors = [ops.gen_anchor(H, W, s, SCALES, RATIOS) for (H, W), s in zip(shapes, STRIDES)]
    eager = [(o.cpu().numpy(), s.cpu().numpy()) for o, s in _five_levels(ops, torch, cls_l, dl_l, info, anchors)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = [(o.cpu().numpy(), s.cpu().numpy()) for o, s in _five_levels(ops, torch, cls_l, dl_l, info, anchors)]
    torch.cuda.current_stream().wait_stream(side)
    for (a, b), (c, d) in zip(eager, got):
        np.testing.assert_array_equal(_bits(a), _bits(c))
        np.testing.assert_array_equal(_bits(b), _bits(d))
    g = torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _five_levels(ops, torch, cls_l, dl_l, info, anchors)  # warm-up (kernel attributes) off-graph
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        cap = _five_levels(ops, torch, cls_l, dl_l, info, anchors)
    for _ in range(2):
        for o, s in cap:
            o.zero_()
            s.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        for (a, b), (o, s) in zip(eager, cap):
            np.testing.assert_array_equal(_bits(a), _bits(o.cpu().numpy()))
            np.testing.assert_array_equal(_bits(b), _bits(s.cpu().numpy()))


@pytest.mark.gpu
def test_retinanet_test_chain(oracle):
    """GenAnchor -> GenProposalRetina x5 -> cat -> det_filter(bbox_classes=1) -> hard NMS 0.5 per
    class, against the restatement + the CPU oracle."""
    import torch
    from simpledet_amd import ops
    rs = np.random.RandomState(12)
    shapes = ((40, 60), (20, 30), (10, 15), (5, 8), (3, 4))
    lv = [_level(rs, 1, H, W) for H, W in shapes]
    info = _info(1, 320, 480)
    anchors = ops.gen_anchor_levels(shapes, STRIDES, SCALES, RATIOS)
    outs = [ops.gen_proposal_retina(torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda(),
                                    torch.from_numpy(info).cuda(), a, num_anchors=A,
                                    rpn_pre_nms_top_n=1000, rpn_min_size=0,
                                    thresh=0.0 if s == 128 else 0.05)
            for (c, d), a, s in zip(lv, anchors, STRIDES)]
    box = torch.cat([o for o, _ in outs], 1)
    score = torch.cat([s for _, s in outs], 1)[:, :, 1:].contiguous()
    dets, counts = ops.det_filter(box, score, 0.05)
    od, oi, oc = ops.soft_nms_batched(dets, counts, 0.5, 0.5, 0.001, 0)
    wbox, wscore = [], []
    for (c, d), (H, W), s in zip(lv, shapes, STRIDES):
        wo, ws = retina_ref.gen_proposal_retina(c, d, info, oracle.gen_anchor(H, W, s, SCALES, RATIOS), A,
                                                rpn_pre_nms_top_n=1000, rpn_min_size=0,
                                                thresh=0.0 if s == 128 else 0.05)
        wbox.append(wo)
        wscore.append(ws)
    wbox = np.concatenate(wbox, 1)
    wscore = np.ascontiguousarray(np.concatenate(wscore, 1)[:, :, 1:])
    wd, wc = oracle.det_filter(wbox, wscore, 0.05)
    np.testing.assert_array_equal(counts.cpu().numpy(), wc)
    od, oi, oc = od.cpu().numpy(), oi.cpu().numpy(), oc.cpu().numpy()
    assert wc.sum() > 100
    for p in range(len(wc)):
        wb, wi = oracle.soft_nms(wd[p, :wc[p]], 0.5, 0.5, 0.001, 0)
        assert oc[p] == len(wi)
        np.testing.assert_array_equal(od[p, :oc[p]], wb)
        np.testing.assert_array_equal(oi[p, :oc[p]], wi)
