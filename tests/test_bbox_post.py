"""BboxPostProcessing (models/maskrcnn/bbox_post_processing.py) and the numpy hard NMS (operator_py/nms.py)
on the device, pinned to what the reference's own Python computed (tests/golden/bbox_post.npz, written by
tests/golden/make_golden_bbox_post.py from inputs that tests/bbox_post_cases.py regenerates here).

Every result is a selection and a copy of input floats, so every comparison is exact.

CPU: fixture integrity, the restatement tests/bbox_post_ref.py equals the fixture on every case (which
licenses it for ties, NaNs and fuzzing, where the reference's unstable sort has no single answer), and the
tie rule on the restatement.  GPU: the operator, the batched primitive, det_filter -> hard_nms_batched,
ties, NaNs, a fuzz, red zones, limits, HIP-graph replay and the Mask R-CNN test chain."""
import hashlib
import os

import numpy as np
import pytest

from . import bbox_post_cases as cases
from . import bbox_post_ref as ref

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bbox_post.npz")


@pytest.fixture(scope="module")
def golden():
    return np.load(GOLDEN)


_inputs = {}


def inputs(name):
    if name not in _inputs:
        _inputs[name] = cases.case(name)
    return _inputs[name]


def sha256(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def fixture_kept(golden, name):
    """[[rows of (image b, class c)]] from the flat fixture arrays"""
    counts, flat = golden[name + "/kept_counts"], golden[name + "/kept_rows"].astype(np.int64)
    out, at = [], 0
    for b in range(counts.shape[0]):
        out.append([])
        for c in range(counts.shape[1]):
            out[b].append(flat[at:at + counts[b, c]])
            at += counts[b, c]
    assert at == len(flat)
    return out


# ------------------------------------------------------------------------------------------ CPU ----
@pytest.mark.parametrize("name", cases.CASES)
def test_fixture_inputs_regenerate(golden, name):
    score, bbox, par = inputs(name)
    assert sha256(score, bbox) == str(golden[name + "/inputs_sha256"])
    assert list(golden[name + "/param"]) == [par["max_det_per_image"], par["min_det_score"], par["nms_thr"]]
    assert golden[name + "/post_score"].shape == (score.shape[0], par["max_det_per_image"], 1)


def test_fixture_covers_what_it_claims(golden):
    """padding, overflow of max_det, an empty class, and thousands of candidates are all in the fixture"""
    assert (golden["edges/post_cls"] == -1).sum() == 100 - 9 and (golden["edges_top/post_cls"] >= 0).all()
    assert golden["edges/kept_counts"].tolist() == [[2, 4, 2, 0, 1]]
    assert golden["edges_ulp/kept_counts"].tolist() == [[1, 4, 2, 0, 1]]   # IoU 0.5 is one ulp over the threshold
    assert int(golden["mask_r50_low/candidates"]) > 20000 and int(golden["r2000/candidates"]) > 10000
    assert golden["shared/kept_counts"].shape == (2, 10)


@pytest.mark.parametrize("name", cases.CASES)
def test_restatement_equals_the_reference_run(golden, name):
    score, bbox, par = inputs(name)
    ps, pb, pc, kept = ref.bbox_post(score, bbox, **par)
    assert np.array_equal(ps, golden[name + "/post_score"])
    assert np.array_equal(pb, golden[name + "/post_bbox"])
    assert np.array_equal(pc, golden[name + "/post_cls"])
    want = fixture_kept(golden, name)
    for b in range(score.shape[0]):
        for c in range(score.shape[2] - 1):
            assert np.array_equal(kept[b][c], want[b][c]), (b, c)


def test_tie_rule_of_the_restatement():
    """equal scores: the later row first -- in the NMS and in the image top-k"""
    dets = np.array([[0, 0, 9, 9, .5], [0, 0, 9, 9, .5], [50, 50, 59, 59, .5], [0, 0, 9, 9, .7]], F)
    assert ref.hard_nms(dets, 0.5).tolist() == [3, 2]          # row 3 kills rows 0 and 1; row 2 before them anyway
    assert ref.hard_nms(dets[:3], 0.5).tolist() == [2, 1]      # of the identical pair the later row survives
    score = np.zeros((1, 3, 3), F)
    score[0, 0, 1] = score[0, 1, 2] = score[0, 2, 1] = .5
    bbox = np.array([[[0, 0, 9, 9]], [[20, 0, 29, 9]], [[40, 0, 49, 9]]], F).reshape(1, 3, 4)
    ps, pb, pc, _ = ref.bbox_post(score, bbox, 2, 0.25, 0.5)
    # stacked list: class 0 -> rows [2, 0] (later row first), class 1 -> [1]; all equal: last entry first
    assert pc[0, :, 0].tolist() == [1, 0] and pb[0, :, 0].tolist() == [20, 0]
    nan = np.array([[0, 0, 9, 9, np.nan], [30, 0, 39, 9, 1.0], [60, 0, 69, 9, np.nan]], F)
    assert ref.hard_nms(nan, 0.5).tolist() == [2, 0, 1]        # NaN scores first, the later row first


# ------------------------------------------------------------------------------------------ GPU ----
def T(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.cpu().numpy()


def same(a, b):
    """bit equality (NaN payloads included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def run_op(ops, score, bbox, par, **kw):
    return [N(x) for x in ops.bbox_post_processing(T(score), T(bbox), **par, **kw)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.CASES)
def test_operator_equals_the_reference_run(ops, golden, name):
    score, bbox, par = inputs(name)
    ps, pb, pc = run_op(ops, score, bbox, par)
    assert same(ps, golden[name + "/post_score"])
    assert same(pb, golden[name + "/post_bbox"])
    assert same(pc, golden[name + "/post_cls"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", cases.CASES)
def test_hard_nms_batched_equals_the_reference_run(ops, golden, name):
    """det_filter -> hard_nms_batched: the twin's kept rows of every (image, class), their order, out_inds --
    which is also the fused operator's result before the top-k (the fixture ties the two together)."""
    import torch
    score, bbox, par = inputs(name)
    B, R, K = score.shape
    dets, counts = ops.det_filter(T(bbox), T(score), par["min_det_score"])
    od, oi, oc = [N(x) for x in ops.hard_nms_batched(dets, counts, par["nms_thr"])]
    dets, counts = N(dets), N(counts)
    want = fixture_kept(golden, name)
    for b in range(B):
        for c in range(K - 1):
            q = b * K + c + 1
            n = oc[q]
            # det_filter keeps row order: candidate i of the problem is image row valid[i]
            valid = np.flatnonzero(score[b, :, c + 1] > F(par["min_det_score"]))
            assert counts[q] == len(valid)
            assert np.array_equal(valid[oi[q, :n]], want[b][c]), (b, c)
            assert same(od[q, :n], dets[q][oi[q, :n]])
    # the convenience wrapper is the same composition
    md, mi, mc = ops.multiclass_nms(T(score), T(bbox), par["min_det_score"], par["nms_thr"], skip_background=True)
    assert same(N(mc), oc.reshape(B, K)[:, 1:]) and tuple(md.shape) == (B, K - 1, R, 5)
    torch.cuda.synchronize()


def _check_against_restatement(ops, score, bbox, par):
    ps, pb, pc = run_op(ops, score, bbox, par)
    ws, wb, wc, _ = ref.bbox_post(score, bbox, **par)
    assert same(ps, ws) and same(pb, wb) and same(pc, wc)


@pytest.mark.gpu
def test_equal_scores_follow_the_documented_tie_rule(ops):
    rs = np.random.RandomState(5)
    score, bbox, par = cases.case("shared")
    score = score.copy()
    # duplicated scores: quantise so that every image holds many equal scores over the threshold
    score[:, :, 1:] = np.round(score[:, :, 1:] * 16) / 16
    assert len(np.unique(score[0, :, 1:][score[0, :, 1:] > 0.05])) < 20
    _check_against_restatement(ops, score, bbox, par)
    # all equal
    score[:, :, 1:] = 0.5
    _check_against_restatement(ops, score, bbox, par)
    # class-specific boxes, duplicates, more than one chunk of 64 per class
    s2, b2 = cases.random_inputs(7, 1, 700, 5, True, 2.0)
    s2[:, :, 1:] = rs.randint(0, 6, s2[:, :, 1:].shape) / 8.0
    _check_against_restatement(ops, s2, b2, dict(max_det_per_image=128, min_det_score=0.2, nms_thr=0.5))
    # the primitive on ties, NaN scores included
    dets = np.concatenate([b2[0, :, 4:8], s2[0, :, 1:2]], 1).astype(F)
    dets[::50, 4] = np.nan
    od, oi, oc = [N(x) for x in ops.hard_nms_batched(T(dets[None]), None, 0.5)]
    want = ref.hard_nms(dets, 0.5)
    assert oc[0] == len(want) and np.array_equal(oi[0, :oc[0]], want) and same(od[0, :oc[0]], dets[want])


@pytest.mark.gpu
def test_nan_scores_and_nan_coordinates(ops):
    score, bbox, par = cases.case("shared")
    score, bbox = score.copy(), bbox.copy()
    rs = np.random.RandomState(9)
    score[rs.rand(*score.shape) < 0.05] = np.nan      # fail `> min_det_score`
    bbox[rs.rand(*bbox.shape) < 0.02] = np.nan        # a NaN overlap suppresses
    bbox[0, 3, 2] = np.inf
    bbox[1, 5, 0] = -np.inf
    _check_against_restatement(ops, score, bbox, par)
    s2, b2 = cases.random_inputs(11, 1, 400, 7, True, 0.05)
    b2[rs.rand(*b2.shape) < 0.01] = np.nan
    _check_against_restatement(ops, s2, b2, dict(max_det_per_image=100, min_det_score=0.05, nms_thr=0.5))


@pytest.mark.gpu
def test_fuzz_against_the_restatement(ops):
    rs = np.random.RandomState(2024)
    for it in range(24):
        R = int(rs.randint(0, 1501)) if it else 0
        K = int(rs.choice([2, 21, 81]))
        specific = bool(rs.randint(2))
        thr = float(rs.choice([0.3, 0.5, 0.7]))
        B = int(rs.randint(1, 3))
        score, bbox = cases.random_inputs(1000 + it, B, R, K, specific, 0.02)
        par = dict(max_det_per_image=int(rs.choice([1, 37, 100, 300])), min_det_score=0.02, nms_thr=thr)
        _check_against_restatement(ops, score, bbox, par)


@pytest.mark.gpu
def test_empty_shapes_produce_the_padding(ops):
    import torch
    for B, R, K in ((0, 10, 5), (2, 0, 5), (2, 10, 1)):
        score = torch.full((B, R, K), 0.9, device="cuda")
        bbox = torch.zeros((B, R, 4), device="cuda")
        ps, pb, pc = ops.bbox_post_processing(score, bbox, 7, 0.05, 0.5)
        assert tuple(ps.shape) == (B, 7, 1) and tuple(pb.shape) == (B, 7, 4)
        assert not N(ps).any() and not N(pb).any() and (N(pc) == -1).all()
    score, bbox, par = cases.case("edges")
    ps, pb, pc = run_op(ops, score, bbox, dict(par, min_det_score=0.99))   # no row over the threshold
    assert not ps.any() and not pb.any() and (pc == -1).all()
    od, oi, oc = ops.hard_nms_batched(torch.zeros((3, 0, 5), device="cuda"), None, 0.5)
    assert N(oc).tolist() == [0, 0, 0]


@pytest.mark.gpu
def test_limits_are_refused(ops):
    import torch
    from simpledet_amd._lib import SD_ERR_UNSUPPORTED, SimpleDetOpsError

    def refused(fn):
        with pytest.raises(SimpleDetOpsError) as e:
            fn()
        assert e.value.code == SD_ERR_UNSUPPORTED

    z = lambda *s: torch.zeros(s, device="cuda")
    refused(lambda: ops.bbox_post_processing(z(1, 4097, 3), z(1, 4097, 4), 10))
    refused(lambda: ops.bbox_post_processing(z(1, 8, 257), z(1, 8, 4), 10))
    refused(lambda: ops.bbox_post_processing(z(1, 8, 3), z(1, 8, 4), 1025))
    refused(lambda: ops.bbox_post_processing(z(1, 8, 3), z(1, 8, 8), 10))      # neither (R,4) nor (R,4K)
    refused(lambda: ops.hard_nms_batched(z(1, 4097, 5), None, 0.5))
    # the limits themselves are taken
    score, bbox = cases.random_inputs(3, 1, 4096, 3, False, 0.3)
    _check_against_restatement(ops, score, bbox, dict(max_det_per_image=1024, min_det_score=0.3, nms_thr=0.5))
    score, bbox = cases.random_inputs(4, 1, 64, 256, False, 0.01)
    _check_against_restatement(ops, score, bbox, dict(max_det_per_image=1024, min_det_score=0.01, nms_thr=0.7))


PAGE = 2 << 20
GUARD = 4096
SENTINEL = 0xA5


def _flush_end(a):
    """numpy array -> device tensor whose last byte is the last byte of its own 2 MB-granular allocation"""
    import torch
    a = np.ascontiguousarray(a)
    total = max(PAGE, (a.nbytes + PAGE - 1) // PAGE * PAGE)
    raw = torch.empty(total, dtype=torch.uint8, device="cuda")
    view = raw[total - a.nbytes:].view(torch.from_numpy(a).dtype).reshape(a.shape)
    view.copy_(torch.from_numpy(a))
    return view, raw


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "shared", "mask_r50_low", "r2000"])
def test_red_zones_stay_untouched(ops, golden, name):
    """outputs and workspace carved from a sentinel-filled arena with guards around each; inputs flush against
    the end of their allocation"""
    import torch
    score, bbox, par = inputs(name)
    B, R, K = score.shape
    top = par["max_det_per_image"]
    wsb = ops.bbox_post_processing_workspace_bytes(B, R, K, bbox.shape[2] // 4, top)
    sizes = [B * top * 4, B * top * 16, B * top * 4, wsb]
    arena = torch.full((sum((s + 255) // 256 * 256 + 2 * GUARD for s in sizes) + GUARD,), SENTINEL,
                       dtype=torch.uint8, device="cuda")
    spans, off = [], 0
    for s in sizes:
        start = (off + GUARD + 255) // 256 * 256
        spans.append((start, start + s))
        off = start + s
    carve = lambda i, shape: arena[spans[i][0]:spans[i][1]].view(torch.float32).reshape(shape)
    out = (carve(0, (B, top, 1)), carve(1, (B, top, 4)), carve(2, (B, top, 1)))
    ws = arena[spans[3][0]:spans[3][1]]
    ts, keep1 = _flush_end(score)
    tb, keep2 = _flush_end(bbox)
    ops.bbox_post_processing(ts, tb, workspace=ws, out=out, **par)
    torch.cuda.synchronize()
    host = N(arena)
    mask = np.ones(len(host), bool)
    for a, b in spans:
        mask[a:b] = False
    bad = np.flatnonzero(mask & (host != SENTINEL))
    assert len(bad) == 0, "stores outside the buffers at arena offsets %s" % bad[:8]
    assert same(N(out[0]), golden[name + "/post_score"]) and same(N(out[1]), golden[name + "/post_bbox"])
    assert same(N(out[2]), golden[name + "/post_cls"])
    # the primitive with its inputs flush against the end of their allocations
    dets, counts = ops.det_filter(tb, ts, par["min_det_score"])
    td, keep3 = _flush_end(N(dets))
    tc, keep4 = _flush_end(N(counts))
    od, oi, oc = ops.hard_nms_batched(td, tc, par["nms_thr"])
    torch.cuda.synchronize()
    assert int(N(oc).sum()) == int(golden[name + "/kept_counts"].sum()) + int(N(oc).reshape(B, K)[:, 0].sum())


@pytest.mark.gpu
def test_graph_capture_and_replay_on_fresh_inputs(ops):
    import torch
    sets = [cases.random_inputs(500 + i, 2, 1000, 81, True, 0.05) for i in range(4)]
    par = dict(max_det_per_image=100, min_det_score=0.05, nms_thr=0.5)
    ts, tb = T(sets[0][0]), T(sets[0][1])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.bbox_post_processing(ts, tb, **par)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = ops.bbox_post_processing(ts, tb, **par)
    for score, bbox in sets[1:]:
        ts.copy_(T(score))
        tb.copy_(T(bbox))
        graph.replay()
        torch.cuda.synchronize()
        got = [N(x).copy() for x in g_out]
        eager = run_op(ops, score, bbox, par)
        assert all(same(g, e) for g, e in zip(got, eager))
        want = ref.bbox_post(score, bbox, **par)[:3]
        assert all(same(g, w) for g, w in zip(got, want))


@pytest.mark.gpu
def test_maskrcnn_test_chain_stage_by_stage(ops, oracle):
    """fused RoIAlign 7x7 -> decode_bbox -> bbox_post_processing -> fused RoIAlign 14x14 on post_bbox_xyxy, one
    HIP graph, against the CPU chain (oracle RoIAlign / decode, the restatement in between)."""
    import torch
    from simpledet_amd import synth
    B, R, K, C = 1, 300, 21, 16
    strides = list(synth.FPN_STRIDES)[:4]
    feats = synth.feature_maps(3, batch=B, channels=C)[:4]
    rois = synth.random_rois(3, B, R, degenerate=False)
    rs = np.random.RandomState(3)
    deltas = (rs.standard_normal((B, R, 4 * K)) * 0.5).astype(F)
    score, _ = cases.random_inputs(77, B, R, K, True, 0.05)
    info = np.array([[800, 1333, 1.0]] * B, F)
    tf, tr, td, tsc, ti = [T(f) for f in feats], T(rois), T(deltas), T(score), T(info)

    def chain():
        return ops.maskrcnn_test_chain(tf, tr, tsc, td, ti, strides, 100, 0.7, 0.5)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [N(x).copy() for x in chain()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        g_out = chain()
    graph.replay()
    torch.cuda.synchronize()
    got = [N(x) for x in g_out]
    assert all(same(g, e) for g, e in zip(got, eager))
    roi_feat, boxes, ps, pb, pc, mask_feat = got
    w_feat = oracle.fpn_roi_align_fwd(feats, rois, strides, (7, 7), nthreads=4)[0]
    assert same(roi_feat, w_feat)
    w_boxes = oracle.decode_bbox(rois, deltas, info, class_agnostic=False)
    assert same(boxes, w_boxes)
    ws, wb, wc, _ = ref.bbox_post(score, w_boxes, 100, 0.7, 0.5)
    assert same(ps, ws) and same(pb, wb) and same(pc, wc)
    assert (wc == -1).any() and (wc >= 0).any()   # padded rows (all-zero boxes) go through the mask extractor too
    w_mask = oracle.fpn_roi_align_fwd(feats, wb, strides, (14, 14), nthreads=4)[0]
    assert same(mask_feat, w_mask)
