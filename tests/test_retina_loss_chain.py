"""The RetinaNet train head as one captured graph: retina_anchor_target (loader layout) -> focal-loss backward
on `out` -> BBoxNorm backward, the labels staying on the device.  Inputs are the reference fixture's im_info
and gt boxes (tests/retinacases.py); the labels must equal the fixture and the gradients the separately
called ops, bit for bit."""
import ctypes
import os

import numpy as np
import pytest

from . import focal_ref as fr
from . import retinacases

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retina_target.npz"))


@pytest.mark.gpu
def test_target_focal_bbox_chain_as_one_graph(ops):
    import torch
    from simpledet_amd._lib import lib
    names = ["cfg_landscape", "cfg_duplicate_gt_holes"]
    ins = [retinacases.inputs(retinacases.CASES[n])[0] for n in names]
    im = torch.from_numpy(np.stack([x[0] for x in ins])).cuda()
    gt = torch.from_numpy(np.stack([x[1] for x in ins])).cuda()
    cfg = retinacases.RETINA
    p = ops.rpn_target_param(cfg["stride"], cfg["short"], cfg["long"], cfg["scales"], cfg["aspects"],
                             cfg["allowed_border"], cfg["pos_thr"], cfg["neg_thr"], cfg["min_pos_thr"])
    B, K, A = 2, 80, 9
    N = GOLD["cfg_landscape/0/label"].size
    rs = np.random.RandomState(11)
    out = torch.from_numpy(fr.sigmoid_f32(fr.logits(rs, (B, N, K)))).cuda()
    gout = torch.from_numpy(rs.standard_normal((B, 4 * A, N // A)).astype(np.float32)).cuda()
    tws = torch.empty(int(lib().cdll.sd_retina_target_workspace_bytes(ctypes.byref(p), B, gt.shape[1])),
                      dtype=torch.uint8, device="cuda")
    ws = [torch.empty(ops.focal_loss_workspace_bytes(), dtype=torch.uint8, device="cuda") for _ in range(2)]
    kw = dict(alpha=0.25, gamma=2.0, grad_scale=1.0, normalization="valid")

    def chain():
        cls, tgt, wgt, fg = ops.retina_anchor_target(im, gt, p, layout=1, workspace=tws)
        return cls, fg, ops.focal_loss_backward(out, cls, workspace=ws[0], **kw), \
            ops.bbox_norm_backward(gout, cls, workspace=ws[1])
    chain()                                  # warm-up outside the capture
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cls, fg, gcls, gbox = chain()
    for t in (cls, fg, gcls, gbox):
        t.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for b, n in enumerate(names):
        np.testing.assert_array_equal(cls[b].cpu().numpy(), GOLD[n + "/0/label"].astype(np.float32))
        assert float(fg[b]) == float(GOLD[n + "/0/fg_count"][0])
    want_label = torch.from_numpy(np.stack([GOLD[n + "/0/label"].astype(np.float32) for n in names])).cuda()
    want_cls = ops.focal_loss_backward(out, want_label, **kw)
    want_box = ops.bbox_norm_backward(gout, want_label)
    assert torch.equal(gcls.view(torch.int32), want_cls.view(torch.int32))
    assert torch.equal(gbox.view(torch.int32), want_box.view(torch.int32))
    count = fr.label_count(want_label.cpu().numpy())
    assert count == sum(int((GOLD[n + "/0/label"] >= 1).sum()) for n in names)
    np.testing.assert_array_equal(gbox.cpu().numpy(), gout.cpu().numpy() / np.float32(count + 1))
