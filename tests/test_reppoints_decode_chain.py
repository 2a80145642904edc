"""The RepPoints test path from head outputs to final detections on the device: reppoints_decode feeds
bbox_post_processing (the `(B, R, K)` scores with the background in column 0 and `(B, R, 4)` boxes it takes) and
det_filter -> hard_nms_batched (detection_test.py's do_nms for nms.type = "nms").  Both chains must give what the
same calls give when fed the float32 restatement's outputs (tests/reppoints_decode_ref.py), and the whole chain must
capture as ONE graph: a host read or synchronisation inside would end the capture with an error."""
import numpy as np
import pytest

from . import reppoints_decode_ref as dr

MIN_SCORE, NMS_THR, MAX_DET = 0.05, 0.5, 100


def _case():
    return dict(dr.cases())["five_levels"]


def _decode(ops, c, dev):
    return ops.reppoints_decode(dev["cls"], dev["pts"], dev["im_info"], c["strides"], c["ks"], transform=c["transform"],
                                moment_transfer=dev["mt"])


def _upload(c):
    import torch
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return dict(cls=[cu(x) for x in c["cls"]], pts=[cu(x) for x in c["pts"]], im_info=cu(c["im_info"]), mt=cu(c["mt"]))


def _post(ops, score, box):
    return ops.bbox_post_processing(score, box, max_det_per_image=MAX_DET, min_det_score=MIN_SCORE, nms_thr=NMS_THR)


def _nms(ops, score, box):
    return ops.hard_nms_batched(*ops.det_filter(box, score, MIN_SCORE), NMS_THR)


def _kept(out):
    """(dets, inds) rows below each problem's count; the rows past it are unspecified"""
    import torch
    od, oi, oc = out
    live = torch.arange(od.shape[1], device=od.device)[None, :] < oc[:, None]
    return od[live].view(torch.int32), oi[live], oc


@pytest.mark.gpu
def test_decode_feeds_post_processing_and_nms(ops):
    import torch
    c = _case()
    want = dr.run(c)
    score, box = _decode(ops, c, _upload(c))
    ref_score, ref_box = torch.from_numpy(want["cls_score"]).cuda(), torch.from_numpy(want["bbox_xyxy"]).cuda()
    N, R, K = ref_score.shape
    assert score.shape == (N, R, K) and box.shape == (N, R, 4) and R <= 4096 and K == 81
    got, ref = _post(ops, score, box), _post(ops, ref_score, ref_box)
    for g, w in zip(got, ref):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32))
    assert bool((got[2][:, :K - 1] >= 0).all())             # every class keeps a row: the chain was not fed padding
    g, w = _kept(_nms(ops, score, box)), _kept(_nms(ops, ref_score, ref_box))
    for a, b in zip(g, w):
        assert torch.equal(a, b)
    counts = g[2].view(N, K)
    assert not counts[:, 0].any() and bool((counts[:, 1:] > 0).all())       # background: no row passes the threshold


@pytest.mark.gpu
def test_the_chain_captures_as_one_graph(ops):
    import torch
    c = _case()
    dev = _upload(c)
    eager = [t.clone() for t in _post(ops, *_decode(ops, c, dev))]
    eager_nms = [t.clone() for t in _kept(_nms(ops, *_decode(ops, c, dev)))]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _post(ops, *_decode(ops, c, dev))                    # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                            # a host synchronisation in here raises
        score, box = _decode(ops, c, dev)
        post = _post(ops, score, box)
        nms = _nms(ops, score, box)
    for _ in range(2):
        for t in (score, box) + tuple(post):
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for g, w in zip(post, eager):
            assert torch.equal(g.view(torch.int32), w.view(torch.int32))
        for g, w in zip(_kept(nms), eager_nms):
            assert torch.equal(g, w)
