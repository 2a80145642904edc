"""ProposalTarget and DecodeBBox pinned to THE REFERENCE'S OWN float64 PYTHON TWINS.

tests/golden/make_golden_py_twins.py ran, from the reference files where they lie,
operator_py/bbox_target.py (_sample_proposal / _expand_bbox_targets / BboxTargetOperator.forward),
operator_py/detectron_bbox_utils.py bbox_transform_inv and operator_py/bbox_transform.py
(bbox_overlaps_py, nonlinear_transform, nonlinear_pred, clip_boxes) and stored what they computed in
tests/golden/py_twins.npz.  Unlike tests/test_ref_pins.py, whose fixtures come from the reference's
C++ compiled against this repository's own MXNet stand-ins, nothing here passed through code of ours:
a misreading shared by the oracle and the kernels (the +1 box convention, >= at fg_thresh, the first
maximum winning an IoU tie, the class slot, the -1 in the decoded x2) fails these tests.

  CPU  (-m "not gpu"): the C oracle reproduces every fixture.
  GPU  (-m gpu): ops.proposal_target (with and without return_index), ops.proposal_target with a
       valid_ranges that admits every box (ProposalTarget_v2: "= ProposalTarget plus valid_ranges",
       include/simpledet_ops.h), the sampling outputs of ops.proposal_mask_target (the v2 sampling
       plus masks, same header) and ops.decode_bbox reproduce the same fixtures through the C ABI.

The cases avoid every place where the twin and the C++ op differ: no subsampling
(#fg <= fg_per_img and #fg + #bg == image_rois, so the RNGs never draw; npr.choice still permutes,
so fg and bg blocks are compared as sets keyed by the op's kept index), image_rois * fg_fraction
integral, all-zero padded proposals, mean 0 and power-of-two stds.  The baseline case (synth inputs,
2000 proposals, 512 rois) does subsample: there every kept fg row must be twin-fg, every kept bg row
twin-bg, and every output row must equal the twin's facts for that proposal.

The targets are pinned to nonlinear_transform (bbox_transform.py, the formula of
proposal_target.cc:204-227); the BboxTarget op's own encoding, bbox_transform_inv, places centres
half a pixel further right, which cancels in gt - roi: the fixture holds both and a test shows they
agree, and BboxTargetOperator.forward's rows are matched on top.

Bars (each rejects a half-pixel slip, which moves a target by >= 0.5 / w / std >= 4e-3 at the
widths used here, an IoU by > 1e-3, a box by 0.5):
  labels, kept sets, weights, roi_output   exact (integers and copied floats)
  match_gt_iou    <= 1e-6: fp32 division in the op, the twin's float32 quotient stored as float64
  targets, dyadic cases (edges, agnostic)   <= 4e-6 max(1, |want|): integer boxes, so the only
                  rounding is the op's fp32 division and logf (<= 1 ulp each, 2 ulp ~ 2.4e-7 rel)
                  against the twin's float64, times 1 / std <= 8 -- a 4x margin
  targets, random cases (random, baseline)  <= 1e-4 absolute: centres of fp32 coordinates up to
                  ~1333 round by <= 3e-5 in fp32 (half an ulp of 1024..2048), divided by widths
                  >= 8 and std 1/8: <= 6e-5
  decoded boxes   <= 1e-3 absolute: the op decodes in fp32 (exp in double) against float64, boxes
                  of <= 4000 px (ulp 2.4e-4); the precedent is tests/golden/make_golden_retina.py
"""
import hashlib
import os

import numpy as np
import pytest

from simpledet_amd import synth

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
Z = np.load(os.path.join(GOLD, "py_twins.npz"))
STD = tuple(float(s) for s in Z["std"])
PT_CASES = ("edges", "agnostic", "random", "baseline")
DEC_CASES = ("dec_cls", "dec_agnostic", "dec_clip")
DYADIC = ("edges", "agnostic")
IOU_BAR = 1e-6
BOX_BAR = 1e-3
EVERYTHING = np.array([[0.0, 1e6]] * 2, np.float32)  # valid_ranges admitting every box


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pt_inputs(name):
    if name == "baseline":
        rois, gt = synth.proposal_target_inputs(0, 2, 2000, 100)
        h = hashlib.sha256(np.ascontiguousarray(rois).tobytes() + np.ascontiguousarray(gt).tobytes())
        assert h.hexdigest() == str(Z["baseline/inputs_sha256"]), "synth inputs changed"
        return rois, gt
    return Z[name + "/rois"], Z[name + "/gt"]


def pt_param(name):
    K, S, frac = Z[name + "/param"]
    return dict(num_classes=int(K), image_rois=int(S), fg_fraction=float(frac), fg_thresh=0.5,
                bg_thresh_hi=0.5, bg_thresh_lo=0.0, class_agnostic=name == "agnostic",
                bbox_mean=(0.0, 0.0, 0.0, 0.0), bbox_std=STD, bbox_weight=(1.0, 1.0, 1.0, 1.0))


def polys_for(gt):
    """One rectangle polygon per gt box, -1 rows for padding: [cls, 1, 8, x1,y1, x2,y1, x2,y2, x1,y2]."""
    B, M, _ = gt.shape
    p = -np.ones((B, M, 11), np.float32)
    for b in range(B):
        for m in range(M):
            x1, y1, x2, y2, c = gt[b, m]
            if c != -1:
                p[b, m] = [c, 1, 8, x1, y1, x2, y1, x2, y2, x1, y2]
    return p


def candidates(rois, gt, b):
    """The op's kept-roi list: non-padded proposals, then the valid gt boxes (-inl.h:155-185)."""
    return np.concatenate([rois[b][rois[b, :, 3] != 0], gt[b][gt[b, :, 4] != -1][:, :4]], 0)


def check_pt(name, ro, lb, bt, bw, iou, kept):
    """Every output of ProposalTarget against the twin's per-row facts and forward rows."""
    rois, gt = pt_inputs(name)
    P = pt_param(name)
    S, K = P["image_rois"], P["num_classes"]
    fg_per = int(S * P["fg_fraction"])
    bar_abs, bar_rel = (0.0, 4e-6) if name in DYADIC else (1e-4, 0.0)
    for b in range(rois.shape[0]):
        n = int(Z[name + "/count"][b])
        cand = candidates(rois, gt, b)
        assert len(cand) == n
        member = Z[name + "/member"][b, :n]
        n_fg = int((member == 1).sum())
        fg_this = min(fg_per, n_fg)
        k = kept[b]
        assert k.min() >= 0 and k.max() < n and len(set(k.tolist())) == S, (name, b, k)
        # kept sets: fg block then bg block, each from the twin's own lists
        assert np.all(member[k[:fg_this]] == 1), "%s img %d: a kept fg row is not twin-fg" % (name, b)
        assert np.all(member[k[fg_this:]] == 0), "%s img %d: a kept bg row is not twin-bg" % (name, b)
        if name != "baseline":
            assert sorted(k[:fg_this]) == sorted(np.nonzero(member == 1)[0].tolist())
            assert sorted(k[fg_this:]) == sorted(np.nonzero(member == 0)[0].tolist())
        np.testing.assert_array_equal(ro[b], cand[k], err_msg="%s img %d: roi_output" % (name, b))
        want_lb = np.where(np.arange(S) < fg_this, Z[name + "/cls"][b, k], 0).astype(np.float32)
        np.testing.assert_array_equal(lb[b], want_lb, err_msg="%s img %d: labels" % (name, b))
        d = np.abs(iou[b].astype(np.float64) - Z[name + "/iou"][b, k])
        assert d.max() <= IOU_BAR, "%s img %d: match_gt_iou off by %g" % (name, b, d.max())
        # targets / weights: the four targets in slot 4 * cls (1 when class-agnostic), zeros elsewhere
        want_t = np.zeros((S, 4 * K))
        want_w = np.zeros((S, 4 * K), np.float32)
        for i in range(fg_this):
            c = 1 if P["class_agnostic"] else int(want_lb[i])
            want_t[i, 4 * c:4 * c + 4] = Z[name + "/tgt"][b, k[i]]
            want_w[i, 4 * c:4 * c + 4] = 1
        np.testing.assert_array_equal(bw[b], want_w, err_msg="%s img %d: weights" % (name, b))
        np.testing.assert_array_equal(bt[b] != 0, want_t != 0, err_msg="%s img %d: target slots" % (name, b))
        err = np.abs(bt[b] - want_t)
        lim = bar_abs + bar_rel * np.maximum(1.0, np.abs(want_t))
        i, j = np.unravel_index(np.argmax(err - lim), err.shape)
        assert np.all(err <= lim), "%s img %d row %d col %d: target %r, twin %r" % (
            name, b, i, j, bt[b, i, j], want_t[i, j])
        if name != "baseline":
            check_forward_rows(name, b, ro[b], lb[b], bt[b], bw[b], K)


def check_forward_rows(name, b, ro, lb, bt, bw, K):
    """BboxTargetOperator.forward's output rows as a multiset: roi, label, class slot, weights, dw/dh."""
    def rows(roi, lab, slot, w, dwdh):
        r = [tuple(roi[i].tolist()) + (float(lab[i]), int(slot[i])) + tuple(w[i].tolist())
             for i in range(len(lab))]
        order = sorted(range(len(r)), key=lambda i: r[i])
        return [r[i] for i in order], dwdh[order]

    slot = np.full(len(lb), -1)
    w4 = np.zeros((len(lb), 4), np.float32)
    dwdh = np.zeros((len(lb), 2))
    for i in range(len(lb)):
        nz = np.nonzero(bw[i])[0]
        if len(nz):
            slot[i] = nz[0] // 4
            w4[i] = bw[i, nz]
            dwdh[i] = bt[i, 4 * slot[i] + 2:4 * slot[i] + 4]
    got, got_dwdh = rows(ro, lb, slot, w4, dwdh)
    want, want_dwdh = rows(Z[name + "/fwd_roi"][b], Z[name + "/fwd_label"][b], Z[name + "/fwd_slot"][b],
                           Z[name + "/fwd_w"][b], Z[name + "/fwd_tgt"][b][:, 2:])
    assert got == want, "%s img %d: rows differ from BboxTargetOperator.forward's" % (name, b)
    err = np.abs(got_dwdh - want_dwdh)
    assert np.all(err <= 4e-6 * np.maximum(1.0, np.abs(want_dwdh))), err.max()


# ---------------------------------------------------------------------------- fixture sanity ---
def test_fixture_cases_avoid_the_twin_differences():
    """No subsampling, integral fg_per_img, power-of-two stds: the twin's RNG and rounding never act."""
    assert all(np.log2(s) == int(np.log2(s)) for s in STD)
    for name in PT_CASES:
        P = pt_param(name)
        S, frac = P["image_rois"], P["fg_fraction"]
        assert S * frac == int(S * frac)
        m = Z[name + "/member"]
        if name != "baseline":
            assert np.all(Z[name + "/count"] == S)
            assert np.all((m == 1).sum(1) <= S * frac) and np.all((m >= 0).sum(1) == S)
        rois, gt = pt_inputs(name)
        pad = rois[:, :, 3] <= 0
        assert np.all(rois[pad] == 0), "padded proposals must be all zeros"
        iou = Z[name + "/iou"][m >= 0]
        if name not in DYADIC:
            assert np.abs(iou - 0.5).min() > 1e-6


def test_edges_case_holds_the_edges():
    """The hand-built case really contains what its comments claim (read from the twin's output)."""
    iou, cls, m = Z["edges/iou"][0], Z["edges/cls"][0], Z["edges/member"][0]
    assert np.sum((iou == 0.5) & (m == 1)) == 3           # IoU exactly 0.5 -> fg
    assert np.sum((iou == 0.0) & (m == 0)) >= 4           # IoU exactly 0 -> bg at bg_thresh_lo = 0
    assert cls[1] == 80 and abs(iou[1] - 90 / 110) < 1e-7  # the tie: first gt (class 80) wins
    assert cls[2] == 7 and m[2] == 1                     # the one-pixel gt's class
    assert (m == 1).sum() == 8 == int(16 * 0.5)          # #fg == fg_per_img
    assert np.all(Z["edges/member"][1, :14] == 0) and np.all(Z["edges/member"][1, 14:16] == 1)
    assert set(Z["agnostic/fwd_label"][0][Z["agnostic/fwd_slot"][0] >= 0]) == {3.0, 7.0, 80.0}
    assert np.all(Z["agnostic/fwd_slot"][Z["agnostic/fwd_slot"] >= 0] == 1)


@pytest.mark.parametrize("name", PT_CASES)
def test_twin_encodings_agree(name):
    """bbox_transform_inv (the BboxTarget op's, centre x1 + w / 2) and nonlinear_transform (the
    formula of proposal_target.cc, centre x1 + (w - 1) / 2): the half pixels cancel in gt - roi, so
    the two twins agree on all four targets.  bbox_transform_inv computes in float32 when handed
    float32 boxes, as the op hands them, so the targets' bars apply."""
    rois, gt = pt_inputs(name)
    bar_abs, bar_rel = (0.0, 4e-6) if name in DYADIC else (1e-4, 0.0)
    for b in range(rois.shape[0]):
        n = int(Z[name + "/count"][b])
        t, ti = Z[name + "/tgt"][b, :n].astype(np.float64), Z[name + "/tgt_inv"][b, :n].astype(np.float64)
        assert np.all(np.abs(ti - t) <= bar_abs + bar_rel * np.maximum(1.0, np.abs(t))), np.abs(ti - t).max()


# --------------------------------------------------------------------------------- CPU oracle ---
def _oracle_pt(oracle, name, variant):
    rois, gt = pt_inputs(name)
    P = pt_param(name)
    p = oracle.make_pt_param(P["num_classes"], rois.shape[0], P["image_rois"], P["fg_fraction"],
                             P["fg_thresh"], P["bg_thresh_hi"], P["bg_thresh_lo"],
                             class_agnostic=P["class_agnostic"], bbox_mean=P["bbox_mean"],
                             bbox_std=P["bbox_std"], bbox_weight=P["bbox_weight"])
    if variant == "v1":
        ro, lb, bt, bw, iou, kept, rc = oracle.proposal_target(rois, gt, p, rng=oracle.GlibcRand(1))
        assert rc == 0
    elif variant == "v2":
        ro, lb, bt, bw, iou, kept, rc = oracle.proposal_target(
            rois, gt, p, rng=oracle.GlibcRand(1), valid_ranges=EVERYTHING, filter_scales=True)
        assert rc == 0
    else:
        ro, lb, bt, bw, iou, _, kept = oracle.proposal_mask_target(
            rois, gt, polys_for(gt), p, mask_size=7, rng=oracle.GlibcRand(1))
    return ro, lb, bt, bw, iou, kept


@pytest.mark.parametrize("variant", ["v1", "v2", "mask"])
@pytest.mark.parametrize("name", PT_CASES)
def test_oracle_proposal_target_matches_twin(oracle, name, variant):
    check_pt(name, *_oracle_pt(oracle, name, variant))


def check_decode(name, got, oracle_out=None):
    want = Z[name + "/boxes"].astype(np.float64)
    err = np.abs(got.astype(np.float64) - want)
    if name != "dec_clip":
        assert err.max() <= BOX_BAR, "%s: max |box - twin| %g" % (name, err.max())
        return
    # nonlinear_pred clips dw, dh at log(1000 / 16); decodebbox.cc does not.  The op follows the C++
    # (equal to the oracle, pinned to decodebbox.cc in test_ref_pins) and differs only on those rows.
    np.testing.assert_array_equal(got, oracle_out)
    R = got.shape[1]
    over = np.zeros(R, bool)
    over[0::4] = True
    row_err = err.max(axis=2)
    assert np.all(row_err[:, ~over] <= BOX_BAR), row_err[:, ~over].max()
    assert np.all(row_err[:, over] > 1.0), row_err[:, over].min()


@pytest.mark.parametrize("name", DEC_CASES)
def test_oracle_decode_bbox_matches_twin(oracle, name):
    out = oracle.decode_bbox(Z[name + "/rois"], Z[name + "/deltas"], Z[name + "/im_info"],
                             bbox_mean=(0, 0, 0, 0), bbox_std=STD,
                             class_agnostic=bool(Z[name + "/class_agnostic"]), xyxy=False)
    check_decode(name, out, out)


# ------------------------------------------------------------------------------------- HIP -----
def _hip_pt(ops, name, variant, return_index=True):
    rois, gt = pt_inputs(name)
    P = pt_param(name)
    B = rois.shape[0]
    kw = dict(P, rng_state=ops.glibc_rand_state(1))
    if variant == "mask":
        out = ops.proposal_mask_target(_t(rois), _t(gt), _t(polys_for(gt)), batch_images=B,
                                       mask_size=7, return_index=True, **kw)
        return [x.cpu().numpy() for x in out[:5] + out[6:]]
    if variant == "v2":
        kw.update(valid_ranges=_t(EVERYTHING), filter_scales=True)
    out = ops.proposal_target(_t(rois), _t(gt), batch_images=B, return_index=return_index, **kw)
    return [x.cpu().numpy() for x in out]


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["v1", "v2", "mask"])
@pytest.mark.parametrize("name", PT_CASES)
def test_hip_proposal_target_matches_twin(ops, name, variant):
    got = _hip_pt(ops, name, variant)
    check_pt(name, *got)
    if variant == "v1":   # the five outputs do not depend on whether the kept index is returned
        plain = _hip_pt(ops, name, variant, return_index=False)
        assert len(plain) == 5
        for a, b in zip(plain, got[:5]):
            np.testing.assert_array_equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", DEC_CASES)
def test_hip_decode_bbox_matches_twin(ops, oracle, name):
    agn = bool(Z[name + "/class_agnostic"])
    rois, deltas, im_info = Z[name + "/rois"], Z[name + "/deltas"], Z[name + "/im_info"]
    out = ops.decode_bbox(_t(rois), _t(deltas), _t(im_info), bbox_mean=(0.0, 0.0, 0.0, 0.0),
                          bbox_std=STD, class_agnostic=agn, bbox_decode_type="xywh").cpu().numpy()
    want = oracle.decode_bbox(rois, deltas, im_info, bbox_mean=(0, 0, 0, 0), bbox_std=STD,
                              class_agnostic=agn, xyxy=False)
    check_decode(name, out, want)
