"""Vectorised numpy restatement of _contrib_GenProposalRetina, generate_proposal_retina.cu:301-468
(the spec; the .cc file is a stale RPN-style copy).  float32 arithmetic in the .cu's operation order
without FMA, exp as float32(exp(float64)), so it is bit-exact against the device op.

Per image: row i = (h*W + w)*AK + c with channel c = anchor*K + class (ProposalGridKernel :66-94),
BBoxPredKernel (:96-159) or IoUPredKernel (:161-209), FilterBoxKernel (:211-233: the whole row is
zeroed), a stable descending sort of (filtered ? 0 : score) and the first pre rows written by
PrepareOutput (:275-297) with the score in column min(out_channel-1, class+1).  NaN scores count
as filtered (the reference's thrust order is undefined for them)."""
import numpy as np

f32 = np.float32


def decode_level(cls_prob, bbox_pred, im_info, anchors, num_anchors, rpn_min_size=16, thresh=0.,
                 anchor_mean=(0.,) * 4, anchor_std=(1.,) * 4, iou_loss=False):
    """One image: cls_prob (AK,H,W), bbox_pred (4A,H,W), im_info (3,), anchors (H*W*A,4) ->
    boxes (count,4), scores (count,), keep (count,) bool, classes (count,), all in row order."""
    AK, H, W = cls_prob.shape
    A = int(num_anchors)
    K = AK // A
    c = np.arange(AK)
    an = c // K
    sc = cls_prob.reshape(AK, H * W).T.reshape(-1).astype(f32)           # (HW*AK,) row order
    anc = anchors.reshape(H * W, A, 4)[:, an, :].reshape(-1, 4).astype(f32)
    d = bbox_pred.reshape(A, 4, H * W)[an].transpose(2, 0, 1).reshape(-1, 4).astype(f32)
    x1, y1, x2, y2 = (anc[:, j] for j in range(4))
    with np.errstate(all="ignore"):
        if iou_loss:
            px1, py1, px2, py2 = x1 + d[:, 0], y1 + d[:, 1], x2 + d[:, 2], y2 + d[:, 3]
        else:
            mean = np.asarray(anchor_mean, f32)
            std = np.asarray(anchor_std, f32)
            width = x2 - x1 + f32(1)
            height = y2 - y1 + f32(1)
            ctr_x = x1 + f32(0.5) * (width - f32(1))
            ctr_y = y1 + f32(0.5) * (height - f32(1))
            dx = d[:, 0] * std[0] + mean[0]
            dy = d[:, 1] * std[1] + mean[1]
            dw = d[:, 2] * std[2] + mean[2]
            dh = d[:, 3] * std[3] + mean[3]
            pcx = dx * width + ctr_x
            pcy = dy * height + ctr_y
            pw = np.exp(dw.astype(np.float64)).astype(f32) * width
            ph = np.exp(dh.astype(np.float64)).astype(f32) * height
            px1 = pcx - f32(0.5) * (pw - f32(1))
            py1 = pcy - f32(0.5) * (ph - f32(1))
            px2 = pcx + f32(0.5) * (pw - f32(1))
            py2 = pcy + f32(0.5) * (ph - f32(1))
        im_h, im_w, scale = (f32(v) for v in im_info)
        clip = lambda v, hi: np.fmax(np.fmin(v, hi - f32(1)), f32(0))  # noqa: E731  CUDA fminf/fmaxf
        boxes = np.stack([clip(px1, im_w), clip(py1, im_h), clip(px2, im_w), clip(py2, im_h)], 1)
        iw = boxes[:, 2] - boxes[:, 0] + f32(1)
        ih = boxes[:, 3] - boxes[:, 1] + f32(1)
        min_size = f32(rpn_min_size) * scale
        keep = ~((iw < min_size) | (ih < min_size) | ~(sc > f32(thresh)))  # NaN score: filtered
    classes = np.tile(c % K, H * W)
    return boxes.astype(f32), sc, keep, classes


def gen_proposal_retina(cls_prob, bbox_pred, im_info, anchors, num_anchors, rpn_pre_nms_top_n=6000,
                        rpn_min_size=16, thresh=0., anchor_mean=(0.,) * 4, anchor_std=(1.,) * 4,
                        iou_loss=False, output_one_hot=True, batch_wise_anchor=False):
    """(B,AK,H,W), (B,4A,H,W), (B,3), anchors -> out (B,top_n,4), score (B,top_n,oc) float32."""
    B, AK, H, W = cls_prob.shape
    K = AK // int(num_anchors)
    count = AK * H * W
    top_n = int(rpn_pre_nms_top_n)
    pre = min(top_n, count)
    oc = K + 1 if output_one_hot else 1
    out = np.zeros((B, top_n, 4), f32)
    score = np.zeros((B, top_n, oc), f32)
    for n in range(B):
        anc = anchors[n] if batch_wise_anchor else anchors
        boxes, sc, keep, classes = decode_level(cls_prob[n], bbox_pred[n], im_info[n], anc, num_anchors,
                                                rpn_min_size, thresh, anchor_mean, anchor_std, iou_loss)
        eff = np.where(keep, sc, f32(0))
        order = np.argsort(-eff, kind="stable")[:pre]   # thrust::stable_sort_by_key(greater)
        k = keep[order]
        out[n, :pre] = np.where(k[:, None], boxes[order], f32(0))
        cols = np.minimum(oc - 1, classes[order] + 1)
        score[n, np.arange(pre), cols] = np.where(k, sc[order], f32(0))
    return out, score


def selected_rows(cls_prob, bbox_pred, im_info, anchors, num_anchors, **kw):
    """The row indices (in output order) that one image's op selects, for cross-checks."""
    pre = min(int(kw.pop("rpn_pre_nms_top_n", 6000)), cls_prob[0].size)
    boxes, sc, keep, classes = decode_level(cls_prob[0], bbox_pred[0], im_info[0], anchors,
                                            num_anchors, **kw)
    eff = np.where(keep, sc, f32(0))
    return np.argsort(-eff, kind="stable")[:pre], keep
