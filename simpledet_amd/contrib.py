"""The reference's operator names for the PyTorch-ROCm harness (autograd enabled).

Each function mirrors the symbol constructor of the same name in the reference graph
(`mx.sym.contrib.ROIAlign_v2`, `mx.sym.ROIPooling_v1`, `mx.sym.ProposalTarget`,
`mx.sym.contrib.GenAnchor`, `mx.sym.contrib.NMS`, `mx.sym.contrib.DeformableConvolution`, mxnext's
`X.roi_align`): same argument names and meaning, same visible outputs.  Forward and backward both
go through the HIP C ABI (simpledet_amd.ops); there is no CPU path.
"""
import os

import torch

from . import ops


class _ROIAlignV2(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, rois, pooled_size, spatial_scale):
        out, mx, my = ops.roi_align_v2_forward(data, rois, pooled_size, spatial_scale)
        ctx.save_for_backward(rois, mx, my)
        ctx.data_shape, ctx.scale = tuple(data.shape), spatial_scale
        return out

    @staticmethod
    def backward(ctx, dy):
        rois, mx, my = ctx.saved_tensors
        dx, _ = ops.roi_align_v2_backward(dy.contiguous(), rois, mx, my, ctx.data_shape, ctx.scale,
                                          req_rois="null")
        return dx, None, None, None


def ROIAlign_v2(data, rois, pooled_size, spatial_scale):
    """mx.sym.contrib.ROIAlign_v2: data (B,C,H,W), rois (B,R,4) -> (B,R,C,ph,pw) (1 visible
    output; maxidx_x / maxidx_y are kept for the backward, roi_align_v2.cc:175-186)."""
    return _ROIAlignV2.apply(data, rois, pooled_size, spatial_scale)


def roi_align(data, rois, out_size, stride):
    """mxnext X.roi_align(feat, rois, out_size, stride) (symbol/builder.py:885-891)."""
    return ROIAlign_v2(data, rois, (out_size, out_size), 1.0 / stride)


class _FPNRoIAlign(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rois, rcnn_stride, pooled_size, scale0, lvl0, *feats):
        ph, pw = (pooled_size, pooled_size) if isinstance(pooled_size, int) else tuple(pooled_size)
        ctx.packed = (ph, pw) in ((7, 7), (14, 14)) and rois.shape[1] <= 8192
        if ctx.packed:  # one-byte arg-max between forward and backward
            out, am = ops.fpn_roi_align_forward_packed(list(feats), rois, rcnn_stride, (ph, pw),
                                                       scale0, lvl0)
            ctx.save_for_backward(rois, am[0], am[1])
        else:
            out, mx, my = ops.fpn_roi_align_forward(list(feats), rois, rcnn_stride, (ph, pw), scale0,
                                                    lvl0)
            ctx.save_for_backward(rois, mx, my)
        ctx.meta = ([tuple(f.shape) for f in feats], list(rcnn_stride), scale0, lvl0)
        return out

    @staticmethod
    def backward(ctx, dy):
        shapes, strides, scale0, lvl0 = ctx.meta
        if ctx.packed:
            rois, am, co = ctx.saved_tensors
            d = ops.fpn_roi_align_backward_packed(dy.contiguous(), rois, (am, co), shapes, strides,
                                                  scale0, lvl0)
        else:
            rois, mx, my = ctx.saved_tensors
            d = ops.fpn_roi_align_backward(dy.contiguous(), rois, mx, my, shapes, strides, scale0,
                                           lvl0)
        return (None, None, None, None, None) + tuple(d)


def fpn_roi_align(feats, rois, rcnn_stride, pooled_size=(7, 7), roi_canonical_scale=224,
                  roi_canonical_level=4):
    """FPNRoiAlign.get_roi_feature (models/FPN/builder.py:567-610) as ONE op:
    fpn_roi_assign -> per-level ROIAlign_v2 -> add_n.  feats: list of (B,C,H_l,W_l)."""
    return _FPNRoIAlign.apply(rois, tuple(rcnn_stride), pooled_size, roi_canonical_scale,
                              roi_canonical_level, *feats)


class _ROIPoolingV1(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, rois, pooled_size, spatial_scale):
        out, idx = ops.roi_pool_v1_forward(data, rois, pooled_size, spatial_scale)
        ctx.save_for_backward(rois, idx)
        ctx.data_shape, ctx.scale = tuple(data.shape), spatial_scale
        return out

    @staticmethod
    def backward(ctx, dy):
        rois, idx = ctx.saved_tensors
        dx, _ = ops.roi_pool_v1_backward(dy.contiguous(), rois, idx, ctx.data_shape, ctx.scale,
                                         req_rois="null")
        return dx, None, None, None


def ROIPooling_v1(data, rois, pooled_size, spatial_scale):
    """mx.sym.ROIPooling_v1: data (B,C,H,W), rois (K,5) -> (K,C,ph,pw)."""
    return _ROIPoolingV1.apply(data, rois, pooled_size, spatial_scale)


class _DeformConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, offset, weight, bias, pad, stride, dilate, dg, num_group, will_backward):
        ctx.save_for_backward(data, offset, weight)
        ctx.cfg = (pad, stride, dilate, dg, num_group, bias is not None)
        # the col matrix stays alive for the backward (which then skips its own im2col): 620 MB per
        # layer at (16,256,50,84) -- only when a backward can follow (will_backward: grad mode on and
        # some input requires a gradient, decided by the caller: in here grad mode is always off).
        # Inference and SIMPLEDET_AMD_DCN_CACHE_COL=0 (process-wide) take the col-free fused kernel; the
        # backward then recomputes col.
        keep = will_backward and os.environ.get("SIMPLEDET_AMD_DCN_CACHE_COL", "1") != "0"
        if keep:
            y, ctx.fwd_ws = ops.deform_conv_forward(data, offset, weight, pad, stride, dilate, dg, keep_col=True,
                                                    bias=bias, num_group=num_group)
        else:
            y, ctx.fwd_ws = ops.deform_conv_forward(data, offset, weight, pad, stride, dilate, dg, bias=bias,
                                                    num_group=num_group), None
        return y

    @staticmethod
    def backward(ctx, dy):
        data, offset, weight = ctx.saved_tensors
        pad, stride, dilate, dg, num_group, has_bias = ctx.cfg
        need = ctx.needs_input_grad
        req = tuple("write" if n else "null" for n in need[:3])
        if has_bias:
            req = req + ("write" if need[3] else "null",)
        g = ops.deform_conv_backward(dy.contiguous(), data, offset, weight, pad, stride, dilate, dg, req=req,
                                     fwd_ws=ctx.fwd_ws, num_group=num_group, bias=has_bias)
        ctx.fwd_ws = None
        return (g[0] if need[0] else None, g[1] if need[1] else None, g[2] if need[2] else None,
                g[3] if has_bias and need[3] else None, None, None, None, None, None, None)


def DeformableConvolution(data, offset, weight, *, bias=None, kernel=(3, 3), stride=(1, 1), dilate=(1, 1),
                          pad=(0, 0), num_filter=None, num_group=1, num_deformable_group=1,
                          no_bias=False):
    """mx.sym.contrib.DeformableConvolution with upstream's parameter set (no_bias defaults to False
    there): models/dcn/builder.py:14-17 (no_bias=True, 4 deformable groups), models/RepPoints/builder.py:
    215-245 (bias), models/sepc/sepc_dconv.py:12-16 (num_group / bias passed through).  Everything behind the
    three tensors is keyword-only: a positional `kernel` must not land in `bias`."""
    if no_bias:
        if bias is not None:
            raise ValueError("no_bias=True but a bias was given")
    elif bias is None:
        raise ValueError("no_bias=False needs a bias (F,)")
    k, s, d, p = [v if isinstance(v, (tuple, list)) else (v, v) for v in (kernel, stride, dilate, pad)]
    if tuple(weight.shape[2:]) != tuple(k) or (num_filter is not None and weight.shape[0] != num_filter):
        raise ValueError("weight shape %s does not match kernel/num_filter" % (tuple(weight.shape),))
    if s[0] != s[1] or d[0] != d[1] or p[0] != p[1]:
        raise ValueError("square stride/dilate/pad only")
    will_backward = torch.is_grad_enabled() and any(t is not None and t.requires_grad
                                                    for t in (data, offset, weight, bias))
    return _DeformConv.apply(data, offset, weight, bias, p[0], s[0], d[0], num_deformable_group, int(num_group),
                             will_backward)


def ProposalTarget(rois, gt_boxes, num_classes, batch_images, image_rois, fg_thresh, bg_thresh_hi,
                   bg_thresh_lo, fg_fraction=0.25, proposal_without_gt=False, class_agnostic=False,
                   output_iou=False, bbox_mean=(0., 0., 0., 0.), bbox_std=(.1, .1, .2, .2),
                   bbox_weight=(1., 1., 1., 1.), rng_state=None):
    """mx.sym.ProposalTarget: 4 visible outputs (5 with output_iou, proposal_target-inl.h:297-303);
    no gradient flows to rois / gt_boxes (:272-276)."""
    with torch.no_grad():
        res = ops.proposal_target(rois, gt_boxes, num_classes, batch_images, image_rois, fg_fraction,
                                  fg_thresh, bg_thresh_hi, bg_thresh_lo, proposal_without_gt,
                                  class_agnostic, bbox_mean, bbox_std, bbox_weight, rng_state)
    return res if output_iou else res[:4]


def GenAnchor(cls_prob, feature_stride=16, scales=(4.0, 8.0, 16.0, 32.0), ratios=(0.5, 1.0, 2.0)):
    """mx.sym.contrib.GenAnchor: only the (H, W) of cls_prob is used."""
    return ops.gen_anchor(cls_prob.shape[2], cls_prob.shape[3], feature_stride, scales, ratios,
                          device=cls_prob.device)


def NMS(rois, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300, threshold=0.7, output_score=False,
        already_sorted=False):
    """mx.sym.contrib.NMS: output (B,post,4) [, score (B,post,1) with output_score]."""
    with torch.no_grad():
        out, score = ops.nms(rois, rpn_pre_nms_top_n, rpn_post_nms_top_n, threshold, already_sorted)
    return (out, score) if output_score else out


def Proposal_v3(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
                threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.), ratios=(0.5, 1., 2.),
                feature_stride=16, output_score=False, iou_loss=False, is_train=False):
    """mx.sym.contrib.Proposal_v3 as models/FPN/builder.py:275-287 calls it."""
    if iou_loss:
        raise ValueError("Proposal_v3: iou_loss=True is not supported")
    with torch.no_grad():
        out, score = ops.proposal_v3(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n,
                                     rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                                     feature_stride, is_train)
    return (out, score) if output_score else out


def Proposal_v2(cls_prob, bbox_pred, im_info, valid_ranges, rpn_pre_nms_top_n=6000,
                rpn_post_nms_top_n=300, threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.),
                ratios=(0.5, 1., 2.), feature_stride=16, output_score=False, iou_loss=False,
                workspace=256, filter_scales=False):
    """mx.sym.contrib.Proposal_v2 as models/tridentnet/builder.py:239-255 calls it.
    workspace (MB) is the reference's temp-space size and is ignored (the op sizes its own)."""
    with torch.no_grad():
        out, score = ops.proposal_v2(cls_prob, bbox_pred, im_info, valid_ranges, rpn_pre_nms_top_n,
                                     rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                                     feature_stride, filter_scales, iou_loss)
    return (out, score) if output_score else out


def Proposal(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n=6000, rpn_post_nms_top_n=300,
             threshold=0.7, rpn_min_size=16, scales=(4., 8., 16., 32.), ratios=(0.5, 1., 2.),
             feature_stride=16, output_score=False, iou_loss=False, workspace=256, is_train=False):
    """mx.sym.contrib.Proposal (X.proposal, symbol/builder.py:241).  workspace (MB) is ignored."""
    with torch.no_grad():
        out, score = ops.proposal(cls_prob, bbox_pred, im_info, rpn_pre_nms_top_n,
                                  rpn_post_nms_top_n, threshold, rpn_min_size, scales, ratios,
                                  feature_stride, is_train, iou_loss)
    return (out, score) if output_score else out


def GenProposalRetina(cls_prob, bbox_pred, im_info, anchors, num_anchors, rpn_pre_nms_top_n=6000,
                      rpn_min_size=16, thresh=0., anchor_mean=(0.,) * 4, anchor_std=(1.,) * 4,
                      iou_loss=False, output_one_hot=True, batch_wise_anchor=False, feature_stride=16,
                      workspace=256):
    """mx.sym.contrib.GenProposalRetina as models/retinanet/builder.py:358-389 calls it: (out, score).
    workspace (MB) is the reference's temp-space size and is ignored (the op sizes its own)."""
    with torch.no_grad():
        return ops.gen_proposal_retina(cls_prob, bbox_pred, im_info, anchors, num_anchors=num_anchors,
                                       rpn_pre_nms_top_n=rpn_pre_nms_top_n, rpn_min_size=rpn_min_size,
                                       thresh=thresh, anchor_mean=anchor_mean, anchor_std=anchor_std,
                                       iou_loss=iou_loss, output_one_hot=output_one_hot,
                                       batch_wise_anchor=batch_wise_anchor,
                                       feature_stride=feature_stride)


def get_top_proposal(bbox, score, top_n):
    """mxnext.tvm.get_top_proposal / models/FPN/get_top_proposal.py."""
    with torch.no_grad():
        return ops.get_top_proposal(bbox, score, top_n)


def DecodeBBox(rois, bbox_pred, im_info, bbox_mean=(0., 0., 0., 0.), bbox_std=(.1, .1, .2, .2),
               class_agnostic=True, bbox_decode_type="xywh"):
    """mx.sym.contrib.DecodeBBox / X.decode_bbox (symbol/builder.py:384-392)."""
    with torch.no_grad():
        return ops.decode_bbox(rois, bbox_pred, im_info, bbox_mean, bbox_std, class_agnostic,
                               bbox_decode_type)


class _FocalLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, label, alpha, gamma, grad_scale, normalization, out_grad):
        out = ops.focal_loss_forward(data.contiguous())
        ctx.save_for_backward(out, label)
        ctx.cfg = (alpha, gamma, grad_scale, normalization, out_grad)
        ctx.mark_non_differentiable(label)
        return out

    @staticmethod
    def backward(ctx, dy):
        out, label = ctx.saved_tensors
        alpha, gamma, grad_scale, normalization, out_grad = ctx.cfg
        g = ops.focal_loss_backward(out, label, dy.contiguous() if out_grad else None, alpha=alpha, gamma=gamma,
                                    grad_scale=grad_scale, normalization=normalization)
        return g, None, None, None, None, None, None


def focal_loss(data, label, alpha=0.25, gamma=2.0, grad_scale=1.0, normalization="null", out_grad=False):
    """mx.sym.contrib.FocalLoss / X.focal_loss (models/retinanet/builder.py:289-297): data (B,nbox,nclass),
    label (B,nbox) -> sigmoid(data).  The backward is the reference's (focal_loss-inl.h:186-230), NOT the
    derivative of the sigmoid: it is the focal-loss gradient itself, and the head gradient enters only with
    out_grad=True.  Defaults: focal_loss-inl.h:52-79."""
    return _FocalLoss.apply(data, label, float(alpha), float(gamma), float(grad_scale), normalization,
                            bool(out_grad))


class _BBoxNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, label):
        ctx.save_for_backward(label)
        return data.clone()

    @staticmethod
    def backward(ctx, dy):
        (label,) = ctx.saved_tensors
        return ops.bbox_norm_backward(dy.contiguous(), label), None


def bbox_norm(data, label):
    """mx.sym.contrib.BBoxNorm / X.bbox_norm (models/retinanet/builder.py:320-324): the identity forward;
    the backward divides the head gradient by max(1, #(label >= 1) over the batch + 1)
    (bbox_norm-inl.h:116-126)."""
    return _BBoxNorm.apply(data, label)


class _SigmoidCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, data, label, grad_scale):
        data = data.contiguous()
        out, _, _ = ops.sigmoid_cross_entropy_forward(data, label.contiguous())
        ctx.save_for_backward(data, label)
        ctx.grad_scale = grad_scale
        return out

    @staticmethod
    def backward(ctx, _dy):
        data, label = ctx.saved_tensors
        return ops.sigmoid_cross_entropy_backward(data, label.contiguous(), ctx.grad_scale)[0], None, None


def sigmoid_cross_entropy(data, label, grad_scale=1.0):
    """mx.sym.contrib.SigmoidCrossEntropy (models/maskrcnn/builder.py:307-312): data / label (n, ...) -> out (n,),
    the mean loss of every row over its labels != -1.  A loss operator: the backward IGNORES the incoming
    gradient, as the reference's does (sigmoid_cross_entropy-inl.h:94-119 never reads out_grad), and grad_scale
    scales the gradient only, not `out`.  The reference's `normalization` parameter is never used and has no
    counterpart here."""
    return _SigmoidCrossEntropy.apply(data, label, float(grad_scale))


class _MaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, cls, target, grad_scale):
        logits = logits.contiguous()
        out, _ = ops.mask_loss_forward(logits, cls.contiguous(), target.contiguous())
        ctx.save_for_backward(logits, cls, target)
        ctx.grad_scale = grad_scale
        return out

    @staticmethod
    def backward(ctx, _dy):
        logits, cls, target = ctx.saved_tensors
        return (ops.mask_loss_backward(logits, cls.contiguous(), target.contiguous(), ctx.grad_scale), None, None,
                None)


def mask_loss(logits, cls, target, grad_scale=1.0):
    """MaskFasterRcnnHead.get_loss (models/maskrcnn/builder.py:278-313) as one op: logits (R, K, h, w), cls (R,)
    float class of every RoI (mask_label), target (R, h, w) in {-1 ignore, 0, 1} -> the (1,) mask loss.  The
    backward writes the dense (R, K, h, w) gradient once and IGNORES the incoming gradient, as the reference's
    loss operator does; grad_scale scales the gradient only."""
    return _MaskLoss.apply(logits, cls, target, float(grad_scale))


class _MsrcnnMaskLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, cls, target, grad_scale):
        logits = logits.contiguous()
        out, _, prob = ops.msrcnn_mask_loss_forward(logits, cls.contiguous(), target.contiguous())
        ctx.save_for_backward(logits, cls, target)
        ctx.grad_scale = grad_scale
        ctx.set_materialize_grads(False)      # no gradient into prob: d_prob stays None, not a tensor of zeros
        return out, prob

    @staticmethod
    def backward(ctx, _dy, d_prob):
        logits, cls, target = ctx.saved_tensors
        if d_prob is not None:
            d_prob = d_prob.contiguous()
        return (ops.msrcnn_mask_loss_backward(logits, cls.contiguous(), target.contiguous(), d_prob, ctx.grad_scale),
                None, None, None)


def msrcnn_mask_loss(logits, cls, target, grad_scale=1.0):
    """Mask Scoring R-CNN's MaskFasterRcnnHead.get_loss (models/msrcnn/builder.py:383-424) as one op: logits
    (R, K, h, w), cls (R,) float, target (R, h, w) -> (mask loss (1,), mask_pred_prob (R, h, w)).  The loss output
    IGNORES its incoming gradient, as the reference's loss operator does (grad_scale scales the gradient only); prob
    is an ordinary differentiable output: what flows into it is added, through the sigmoid, to the selected plane's
    gradient in the same single pass that writes the dense (R, K, h, w) gradient."""
    return _MsrcnnMaskLoss.apply(logits, cls, target, float(grad_scale))


class _MaskIoULoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, iou_pred, prob, target, ratio, cls, grad_scale):
        iou_pred = iou_pred.contiguous()
        cls = cls.contiguous()
        iou_target, weight, loss, weight_sum = ops.maskiou_loss_forward(
            iou_pred, prob.contiguous(), target.contiguous(), ratio.contiguous(), cls)
        ctx.save_for_backward(iou_pred, cls, iou_target, weight, weight_sum)
        ctx.grad_scale = grad_scale
        ctx.mark_non_differentiable(iou_target, weight)
        return loss, iou_target, weight

    @staticmethod
    def backward(ctx, _dy, _dt, _dw):
        iou_pred, cls, iou_target, weight, weight_sum = ctx.saved_tensors
        return (ops.maskiou_loss_backward(iou_pred, cls, iou_target, weight, weight_sum, ctx.grad_scale),
                None, None, None, None, None)


def maskiou_loss(iou_pred, prob, target, ratio, cls, grad_scale=1.0, return_target=False):
    """MaskIoUConvHead.get_loss behind its tower (models/msrcnn/builder.py:146-167) as one op: iou_pred (R, K), prob
    and target (R, h, w), ratio (R,), cls (R,) float -> the (1,) MaskIoU loss; with return_target=True also
    (iou_target, weight), maskiou_compute.py's outputs.  Gradient flows to iou_pred alone (the reference BlockGrads
    the target and the weight) and IGNORES the incoming gradient, as MakeLoss does."""
    loss, iou_target, weight = _MaskIoULoss.apply(iou_pred, prob, target, ratio, cls, float(grad_scale))
    return (loss, iou_target, weight) if return_target else loss


def reppoints_head_loss(pts_init, pts_refine, gt_bbox, moment_transfer, strides, transform="moment", scale=4,
                        target_scale=4, num_pos=1, pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.0):
    """The box branches of RepPointsHead.get_loss (models/RepPoints/builder.py:311-484) on lists of per-level point
    maps (N, 2 * num_points, H_l, W_l): both assigners on the (gradient-blocked) init maps, then the two box losses.
    Returns (pts_init_loss, pts_refine_loss, targets): the losses (N, P, 4) with autograd into the maps and
    moment_transfer (the incoming gradient is IGNORED, as the reference's MakeLoss does: the head gradient is 0.5 /
    1.0 over the BBoxNorm denominators), and the RepPointsTargets whose label_refine feeds focal_loss."""
    targets = ops.reppoints_target([t.detach().contiguous() for t in pts_init], gt_bbox.contiguous(), strides,
                                   transform=transform, moment_transfer=None if moment_transfer is None else moment_transfer.detach(),
                                   target_scale=target_scale, num_pos=num_pos, pos_iou_thr=pos_iou_thr,
                                   neg_iou_thr=neg_iou_thr, min_pos_iou=min_pos_iou)
    loss_init, loss_refine = ops.reppoints_box_loss(pts_init, pts_refine, targets, strides, transform=transform,
                                                    moment_transfer=moment_transfer, scale=scale)
    return loss_init, loss_refine, targets
