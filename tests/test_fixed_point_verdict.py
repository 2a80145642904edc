"""The range verdict of the fixed-point backwards on crowded bands (csrc/common.h `fx_range_*`).

roi_align_bwd_packed4, roi_align_bwd_flt4_kernel and deform_col2im_chunk_kernel sum in LDS as 32-bit fixed point
and decide once per workgroup, from a sample of the gradients they streamed, whether the integer unit is fine
enough; if not they sum again with fp32 adds.  The verdict travelled as ONE int32, (sum of exponent margins << 12)
+ sample count.  Two ways it went wrong, restated in numpy by tests/fx_verdict.py:
  - packed4 restarted its trip index per chunk of RoIs, so it sampled every trip instead of the thinned ones its
    stride mask plans: past 4095 samples -- 316 RoIs of one image on one band at 7x7, 123 at 14x14 -- the count
    carried into the margins and a late outlier was under-corrected: fixed point kept with a unit far too coarse;
  - a first trip of zeros (gmax_used == 0) makes every margin ~140: the int32 wrapped, in all three kernels.
The CPU tests show that every GPU case below is one where the exact verdict and the wrapped one disagree (or, for
the controls, agree); the GPU tests hold the kernels to the oracle at test_fixed_point_precision's elementwise bar
    |got - want| <= 1e-4 * max(median |dY|, mass),   mass = the oracle's backward of |dY|,
and, where the exact verdict keeps fixed point, to bit-identical output over two launches.
"""
import numpy as np
import pytest

from simpledet_amd import synth

from . import fx_verdict as V
from .test_fixed_point_precision import _stats

STRIDES = list(synth.FPN_STRIDES)
SHAPES = [tuple(s) for s in synth.FPN_SHAPES]
OUTLIERS = [0, 8, 12, 16]   # log2 of the late outlier over the Gaussian's maximum; 0 = none


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ cases
def crowded_rois(seed, counts):
    """one image: counts = {level index: number of RoIs}, every RoI assigned to its level (sqrt(wh) in
    224 * 2^(l - 2) .. 2x that), spread uniformly over the image"""
    rs = np.random.RandomState(seed)
    boxes = []
    for l, n in sorted(counts.items()):
        lo = 224.0 * 2 ** (l - 2)
        s = rs.uniform(1.04 * lo, 1.9 * lo if l < 3 else min(1.9 * lo, 780.0), n)
        ar = rs.uniform(0.8, 1.25, n)
        w, h = np.minimum(s * np.sqrt(ar), synth.IMG_W - 2), np.minimum(s / np.sqrt(ar), synth.IMG_H - 2)
        x1, y1 = rs.uniform(0, synth.IMG_W - 1 - w), rs.uniform(0, synth.IMG_H - 1 - h)
        boxes.append(np.stack([x1, y1, x1 + w, y1 + h], 1))
    return np.concatenate(boxes).astype(np.float32)[None]


def _outlier(dy, rois_level, l, k, seed, base, pos=0):
    """2^k x base (the maximum before any outlier) at bin `pos` of the last RoI of level l (the last chunk of its
    band list), every channel"""
    if k:
        r = int(np.flatnonzero(rois_level[0] == l)[-1])
        sign = np.where(np.random.RandomState(seed).rand(dy.shape[2]) < 0.5, -1.0, 1.0).astype(np.float32)
        dy[0, r, :, pos // dy.shape[4], pos % dy.shape[4]] = sign * np.float32(2.0 ** k) * base
    return dy


def case_crowded(oracle, pooled, counts, k, seed, C=8, zero_first=0, lognormal=0.0):
    """rois (1,R,4), level (1,R), dY (1,R,C,P,P) Gaussian (x lognormal(sigma) when given); the first `zero_first`
    RoIs of every crowded level get dY = 0; the outlier goes into each crowded level's last RoI"""
    rois = crowded_rois(seed, counts)
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert all(int((level == l).sum()) == n for l, n in counts.items()), "a RoI left its level"
    rs = np.random.RandomState(seed + 1)
    P = pooled
    dy = rs.standard_normal((1, rois.shape[1], C, P, P)).astype(np.float32)
    if lognormal:
        dy *= np.exp(lognormal * rs.standard_normal(dy.shape)).astype(np.float32)
    base = np.float32(np.abs(dy).max())
    for l in counts:
        if zero_first:
            dy[0, np.flatnonzero(level[0] == l)[:zero_first]] = 0.0
        _outlier(dy, level, l, k, seed + 2, base)
    return rois, level, dy


def packed4_verdicts(rois, level, dy, pooled, mode):
    """numpy verdicts of every (level, band, channel) workgroup of the crowded levels: mode 'taps' (lists + tap
    tables, pre-pass pixel bound), 'lists0' (`roi_align_bwd_lists` = 0: band-summed bound of bwd_band_list),
    'flt' (MODE 2: float arg-max planes, one chunk, band-summed bound).  Returns [(verdicts at the bound and at
    the bound + one RoI's bins -- the device's 1-ulp reciprocal), ...]."""
    out = []
    for u in V.band_units(rois, level, SHAPES, STRIDES, pooled=pooled, taps=(mode == "taps")):
        if len(u["list"]) < 2:
            continue
        b = u["pixel"] if mode == "taps" else u["total"]
        for c in range(dy.shape[2]):
            g = dy[u["img"], u["list"], c].reshape(len(u["list"]), -1)
            vs = [V.packed4_verdict(g, bb, flt=(mode == "flt")) for bb in sorted({b, b + pooled})]
            out.append((u, c, b, vs))
    return out


def _differs(vs):
    return all(v["intended"] != v["head"] for v in vs)


def _mostly_differ(vv):
    """the wrapped verdict is wrong in at least half of the workgroups (per channel, gmax_used and hence the
    margins vary)"""
    return 2 * sum(_differs(x[3]) for x in vv) >= len(vv)


def _agrees(vs):
    return all(v["intended"] == v["head"] for v in vs)


def _fx_ok(b):
    return b <= 2048   # set_scale: a larger weight bound takes the float adds whatever the verdict


CROWD7 = {2: 330}                  # P4, one band: 330 RoIs of one image
CROWD14 = {2: 128, 3: 128}         # P4 and P5 at 14x14


# ------------------------------------------------------------------------------------------------ CPU: the cases reach the wrap
@pytest.mark.parametrize("k", OUTLIERS)
def test_crowded_7x7_cases_separate_the_verdicts(oracle, k):
    rois, level, dy = case_crowded(oracle, 7, CROWD7, k, 100 + k)
    for mode in ("taps", "lists0"):
        vv = [x for x in packed4_verdicts(rois, level, dy, 7, mode) if _fx_ok(x[2])]
        assert vv, mode
        # 13 samples per RoI: 4290 > 4095, the count carries into the margins
        assert all(x[3][0]["n_head"] == 13 * 330 for x in vv), mode
        assert all(x[3][0]["n"] < 4096 for x in vv), mode
        if k >= 8:   # the exact verdict refuses the unit, the wrapped one keeps it
            assert all(not v["intended"] for x in vv for v in x[3]), mode
            assert _mostly_differ(vv), mode
            assert all(x[3][0]["head_exact"] == x[3][0]["intended"] for x in vv), "not the wrap alone"
        else:
            assert any(v["intended"] for x in vv for v in x[3]), mode   # fixed point: determinism is tested
    # the float arg-max path thins its sampling correctly: the control
    vv = [x for x in packed4_verdicts(rois, level, dy, 7, "flt") if _fx_ok(x[2])]
    assert vv and all(_agrees(x[3]) for x in vv)


@pytest.mark.parametrize("k", OUTLIERS)
def test_crowded_14x14_cases_separate_the_verdicts(oracle, k):
    for half in (False, True):
        rois, level, dy = case_crowded(oracle, 14, CROWD14, k, 200 + k)
        if half:
            dy = (dy * np.float32(2.0 ** -4)).astype(np.float16).astype(np.float32)
        vv = [x for x in packed4_verdicts(rois, level, dy, 14, "taps") if _fx_ok(x[2])]
        assert len({x[0]["lvl"] for x in vv}) == 2
        # the first 512 items of each 16-RoI chunk: 8 chunks = 4096 samples
        assert all(x[3][0]["n_head"] == 4096 for x in vv)
        if k >= 8:
            assert _mostly_differ(vv), half


@pytest.mark.parametrize("pooled,nl", [(7, 315), (7, 316), (14, 122), (14, 123)])
def test_exact_boundary_cases(oracle, pooled, nl):
    """the count field holds 4095 samples: 315 RoIs x 13 at 7x7; at 14x14 the first trip of each 16-RoI chunk is
    sampled (512 items), so 122 RoIs (7 chunks + 490 items) stay below and 123 reach 4096.  (84 RoIs x 49 items
    would, had every item been sampled.)"""
    rois, level, dy = case_crowded(oracle, pooled, {2: nl}, 16, 300 + nl)
    vv = [x for x in packed4_verdicts(rois, level, dy, pooled, "taps") if _fx_ok(x[2])]
    assert vv
    wrap = nl in (316, 123)
    assert all((x[3][0]["n_head"] >= 4096) == wrap for x in vv)
    assert _mostly_differ(vv) if wrap else all(_agrees(x[3]) for x in vv)


def case_zero_first_packed4(oracle, k):
    # the first chunk (32 RoIs) receives no loss: gmax_used = 0, e_thr ~ -5, every margin ~130
    return case_crowded(oracle, 7, {2: 400}, k, 400 + k, zero_first=32)


@pytest.mark.parametrize("k", [0, 16])
def test_zero_first_chunk_packed4_case_separates_the_verdicts(oracle, k):
    rois, level, dy = case_zero_first_packed4(oracle, k)
    vv = [x for x in packed4_verdicts(rois, level, dy, 7, "taps") if _fx_ok(x[2])]
    assert vv and all(x[3][0]["gmax_used"] == 0.0 for x in vv)
    assert all(v["intended"] == (k == 0) for x in vv for v in x[3])
    # without the outlier the exact verdict keeps fixed point and the wrapped one refuses it (float adds: the
    # result is no longer a deterministic function of the inputs); with it both refuse
    assert all(_differs(x[3]) if k == 0 else _agrees(x[3]) for x in vv)


C4_SCALE = 2.0 ** 44   # a first trip of zeros wraps flt4's int32 only when 3072 samples x margin > 2^19


def case_zero_first_flt4(oracle):
    rs = np.random.RandomState(500)
    data = rs.standard_normal((1, 8, 50, 84)).astype(np.float32)
    rois = synth.random_rois(501, 1, 512)
    o, ax, ay = oracle.roi_align_v2_fwd(data, rois, (7, 7), 1 / 16.0, nthreads=4)
    dy = (rs.standard_normal(o.shape) * C4_SCALE).astype(np.float32)
    dy[:, :11] = 0.0   # units 0 .. 538 of every channel quad: the whole first trip
    return data, rois, ax, ay, dy


def test_zero_first_units_flt4_case_separates_the_verdicts(oracle):
    data, rois, ax, ay, dy = case_zero_first_flt4(oracle)
    bound = V.flt4_bound(rois[0], 50, 84, 1 / 16.0)
    for c in (0, 4):
        vs = [V.flt4_verdict(dy[0].reshape(512, 8, 49), c, b) for b in (bound, bound + 7)]
        assert vs[0]["gmax_used"] == 0.0
        assert all(v["intended"] and not v["head"] for v in vs), vs


COL_SCALE = 2.0 ** 24
COL_HW = (100, 168)    # 16800 pixels: channel 0 of tap 0 is sampled at every 4th of the first 16000


def case_zero_first_col2im():
    rs = np.random.RandomState(600)
    C, (H, W) = 8, COL_HW
    off = (rs.standard_normal((1, 18, H, W)) * 1.5).astype(np.float32)
    col = (rs.standard_normal((1, C * 9, H * W)) * COL_SCALE).astype(np.float32)
    col[0, 0:C * 9:9, :4 * 512] = 0.0   # tap 0 of every channel: the first trip (4 T pixels) of each workgroup
    return off, col


def test_zero_first_trip_col2im_case_separates_the_verdicts():
    off, col = case_zero_first_col2im()
    for c0 in (0, 4):
        tap0 = col[0, c0 * 9:(c0 + 4) * 9:9]
        gt = np.abs(col[0, c0 * 9:(c0 + 4) * 9]).max()
        # (the weight sum of the offsets above: a few x 9 taps -- every plausible bit count separates them)
        vs = [V.col2im_verdict(tap0, cb, gt) for cb in range(3, 8)]
        assert vs[0]["gmax_used"] == 0.0
        assert all(v["intended"] and not v["head"] for v in vs), vs


def test_verdict_restatement_without_wrap_is_the_exact_sum():
    """sanity of the restatement: below 4096 samples with small margins the packed int32 is exact"""
    g = np.random.RandomState(1).standard_normal((20, 49)).astype(np.float32)
    v = V.packed4_verdict(g, 64)
    assert v["n_head"] == v["n"] == 20 * 13 and v["intended"] == v["head"] == v["head_exact"]


# ------------------------------------------------------------------------------------------------ GPU
def _mass_bar(got, want, mass, dy):
    return _stats(got, want, mass, float(np.median(np.abs(dy))))


def _cat(arrs):
    return np.concatenate([np.asarray(a).ravel() for a in arrs])


def _run_fused(ops, oracle, rois, dy, pooled, modes, C=8, seed=0):
    """the crowded case through the product's backward in each mode -> {mode: (stats, deterministic)}"""
    import torch
    from simpledet_amd._lib import lib
    feats = synth.feature_maps(seed, batch=1, channels=C)
    shapes = [f.shape for f in feats]
    P = (pooled, pooled)
    fw = oracle.fpn_roi_align_fwd(feats, rois, STRIDES, P, nthreads=8)
    want = _cat(oracle.fpn_roi_align_bwd(dy, rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    mass = _cat(oracle.fpn_roi_align_bwd(np.abs(dy), rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    tf, tr, tdy = [_t(f) for f in feats], _t(rois), _t(dy)
    res = {}
    for mode in modes:
        if mode == "flt":
            _, mx, my = ops.fpn_roi_align_forward(tf, tr, STRIDES, P)
            run = lambda: ops.fpn_roi_align_backward(tdy, tr, mx, my, shapes, STRIDES)
        else:
            _, state = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, P)
            run = lambda: ops.fpn_roi_align_backward_packed(tdy, tr, state, shapes, STRIDES)
        with lib().tuned(roi_align_bwd_lists=0 if mode == "lists0" else 1):
            g1 = run()
            g2 = run()
        same = all(bool(torch.equal(a, b)) for a, b in zip(g1, g2))
        res[mode] = (_mass_bar(_cat([g.cpu().numpy() for g in g1]), want, mass, dy), same)
    return res


def _check(res, deterministic_modes):
    bad = {m: st for m, (st, _) in res.items() if not st["mass_bar"] <= 1e-4}
    assert not bad, {m: (st["mass_bar"], st["max_abs_err"]) for m, st in bad.items()}
    for m in deterministic_modes:
        assert res[m][1], "%s: two launches differ where the verdict keeps fixed point" % m


@pytest.mark.gpu
@pytest.mark.parametrize("k", OUTLIERS)
def test_crowded_band_7x7_against_the_oracle(ops, oracle, k):
    rois, level, dy = case_crowded(oracle, 7, CROWD7, k, 100 + k)
    res = _run_fused(ops, oracle, rois, dy, 7, ("taps", "lists0", "flt"))
    _check(res, ("taps",) if k == 0 else ())


@pytest.mark.gpu
@pytest.mark.parametrize("k", OUTLIERS)
def test_crowded_band_14x14_against_the_oracle(ops, oracle, k):
    rois, level, dy = case_crowded(oracle, 14, CROWD14, k, 200 + k)
    _check(_run_fused(ops, oracle, rois, dy, 14, ("taps",)), ("taps",) if k == 0 else ())


@pytest.mark.gpu
@pytest.mark.parametrize("k", OUTLIERS)
def test_crowded_band_14x14_fp16_io_against_the_oracle(ops, oracle, k):
    """fp16 gradients in and out: against the oracle's fp32 sums rounded to fp16, the mass bar plus one fp16 step
    of the reference"""
    import torch
    rois, level, dy = case_crowded(oracle, 14, CROWD14, k, 200 + k)
    dy16 = (dy * np.float32(2.0 ** -4)).astype(np.float16)
    feats16 = [f.astype(np.float16) for f in synth.feature_maps(0, batch=1, channels=8)]
    shapes = [f.shape for f in feats16]
    f32s = [f.astype(np.float32) for f in feats16]
    fw = oracle.fpn_roi_align_fwd(f32s, rois, STRIDES, (14, 14), nthreads=8)
    d32 = dy16.astype(np.float32)
    want = _cat(oracle.fpn_roi_align_bwd(d32, rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    mass = _cat(oracle.fpn_roi_align_bwd(np.abs(d32), rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    _, am = ops.fpn_roi_align_forward_packed_f16([_t(f) for f in feats16], _t(rois), STRIDES, (14, 14))
    g1 = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(rois), am, shapes, STRIDES)
    g2 = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(rois), am, shapes, STRIDES)
    got = _cat([g.cpu().numpy().astype(np.float32) for g in g1]).astype(np.float64)
    w16 = want.astype(np.float16).astype(np.float64)
    step = np.maximum(np.abs(w16) * 2.0 ** -10, 2.0 ** -24)
    excess = np.maximum(np.abs(got - w16) - step, 0.0)
    bar = float((excess / np.maximum(float(np.median(np.abs(d32))), mass)).max())
    assert bar <= 1e-4, bar
    if k == 0:
        assert all(bool(torch.equal(a, b)) for a, b in zip(g1, g2))


@pytest.mark.gpu
@pytest.mark.parametrize("pooled,nl", [(7, 315), (7, 316), (14, 122), (14, 123)])
def test_exact_boundary_against_the_oracle(ops, oracle, pooled, nl):
    rois, level, dy = case_crowded(oracle, pooled, {2: nl}, 16, 300 + nl)
    _check(_run_fused(ops, oracle, rois, dy, pooled, ("taps",)), ())


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 16])
def test_zero_first_chunk_packed4_against_the_oracle(ops, oracle, k):
    rois, level, dy = case_zero_first_packed4(oracle, k)
    _check(_run_fused(ops, oracle, rois, dy, 7, ("taps",)), ("taps",) if k == 0 else ())


@pytest.mark.gpu
def test_zero_first_units_flt4_against_the_oracle(ops, oracle):
    import torch
    data, rois, ax, ay, dy = case_zero_first_flt4(oracle)
    want = oracle.roi_align_v2_bwd(dy, ax, ay, data.shape)
    mass = oracle.roi_align_v2_bwd(np.abs(dy), ax, ay, data.shape)
    args = (_t(dy), _t(rois), _t(ax), _t(ay), data.shape, 1 / 16.0)
    g1 = ops.roi_align_v2_backward(*args)[0]
    g2 = ops.roi_align_v2_backward(*args)[0]
    st = _mass_bar(g1.cpu().numpy(), want, mass, dy)
    assert st["mass_bar"] <= 1e-4, st
    assert torch.equal(g1, g2), "two launches differ where the verdict keeps fixed point"


@pytest.mark.gpu
def test_zero_first_trip_col2im_against_the_oracle(ops, oracle):
    """the stand-alone deform_col2im (sd_deform_col2im_ws) on a col whose first trip of tap 0 is zero, and the
    layer backward on a dY whose first 4 T pixels are zero (so is every tap of dcol there)"""
    import torch
    off, col = case_zero_first_col2im()
    C, (H, W) = 8, COL_HW
    want = oracle.deform_col2im(col[0], off[0], (C, H, W), kernel=(3, 3), pad=1, stride=1, dil=1, dgroup=1)
    mass = oracle.deform_col2im(np.abs(col[0]), off[0], (C, H, W), kernel=(3, 3), pad=1, stride=1, dil=1, dgroup=1)
    g1 = ops.deform_col2im(_t(col), _t(off), (1, C, H, W), (3, 3), 1, 1, 1, 1)
    g2 = ops.deform_col2im(_t(col), _t(off), (1, C, H, W), (3, 3), 1, 1, 1, 1)
    st = _stats(g1.cpu().numpy()[0], want, mass, float(np.median(np.abs(col))))
    assert st["mass_bar"] <= 1e-4, st
    assert torch.equal(g1, g2), "stand-alone col2im: two launches differ"
    # layer backward
    rs = np.random.RandomState(601)
    F = 8
    x = rs.standard_normal((1, C, H, W)).astype(np.float32)
    w = (rs.standard_normal((F, C, 3, 3)) * 0.05).astype(np.float32)
    dy = (rs.standard_normal((1, F, H, W)) * COL_SCALE).astype(np.float32)
    dy.reshape(1, F, -1)[:, :, :4 * 512] = 0.0
    dcol = (w.reshape(F, -1).T.astype(np.float64) @ dy[0].reshape(F, -1).astype(np.float64)).astype(np.float32)
    want = oracle.deform_col2im(dcol, off[0], (C, H, W), kernel=(3, 3), pad=1, stride=1, dil=1, dgroup=1)
    mass = oracle.deform_col2im(np.abs(dcol), off[0], (C, H, W), kernel=(3, 3), pad=1, stride=1, dil=1, dgroup=1)
    run = lambda: ops.deform_conv_backward(_t(dy), _t(x), _t(off), _t(w), pad=1, stride=1, dilate=1,
                                           num_deformable_group=1)[0]
    d1, d2 = run(), run()
    st = _stats(d1.cpu().numpy()[0], want, mass, float(np.median(np.abs(dcol))))
    # (dcol comes out of the split-fp16 GEMM: test_dcn_col2im_heavy_tailed_loss_scaled's bar)
    assert st["mass_bar"] <= 1e-4 or st["max_abs_err"] <= 4e-6 * st["max_abs_want"], st
    assert torch.equal(d1, d2), "layer backward: two launches differ"
