"""_contrib_DeformablePSROIPooling and TSD's fused FPN extractor (simpledet_amd/csrc/deform_psroi.hip) against
the restatement of tests/deform_psroi_ref.py (DESIGN.md 4.15 is the spec).

  CPU: the restatement's backward against autograd on a float64 torch restatement of its forward (pins the
       signs of the d_trans formulas); known answers (a clamped sample with d_trans != 0, round(2.5) == 3,
       the bins the masked RoI (-1,-1,-1,-1) keeps on strides 4 / 8 / 16 / 32); argument validation of the
       four C entry points (all fail before any launch).
  GPU: top_count exact; out, d_data, d_trans within
           k = |got - truth| / (eps32 * T + tiny),   k_gpu <= 2 * k_ref + 2  per case and output,
       k_ref = the float32 restatement's own k against the float64 truth.  The random fixtures are drawn until,
       in float64, no sample lies within 1e-4 of a skip boundary and no level-rule argument within 1e-4 of a
       level boundary, so float32 and float64 take the same branches; the boundaries themselves are covered by
       cases made of exactly representable numbers, which must match bit for bit.
"""
import ctypes
import functools

import numpy as np
import pytest

from simpledet_amd import _lib

from . import deform_psroi_ref as dr

H, W, B, K = 13, 17, 2, 6
SCALE = 0.25
FSHAPES = ((16, 20), (8, 10), (4, 5), (2, 3))
FSTRIDES = (4, 8, 16, 32)


# ------------------------------------------------------------------------------------- fixtures --
def _rois(rs):
    j = lambda: rs.uniform(-0.4, 0.4)
    return np.float32([
        [0, 9 + j(), 7 + j(), 41 + j(), 37 + j()],          # interior
        [1, -21 + j(), -11 + j(), 22 + j(), 26 + j()],      # partly off the map
        [0, 200 + j(), 210 + j(), 240 + j(), 250 + j()],    # wholly off: count 0
        [1, 30 + j(), 22 + j(), 10 + j(), 5 + j()],         # degenerate: x2 < x1, y2 < y1
        [0, 4.5, 6.5, 30.5, 40.5],                          # .5 coordinates: round() half away from zero
        [1, 40 + j(), 30 + j(), 66 + j(), 50 + j()],        # at the border; its offsets push samples out
    ])


# name -> C, group, output_dim, P, S, num_classes (0: no_trans), part_size
SINGLE = {
    "C5-P7-S4-cls1": (5, 1, 5, 7, 4, 1, 0),
    "C8-P7-S4-cls2-part3": (8, 1, 8, 7, 4, 2, 3),
    "C8-G2-P3-S2-cls1": (8, 2, 2, 3, 2, 1, 3),
    "C8-G2-P7-S2-cls2-part3": (8, 2, 2, 7, 2, 2, 3),
    "C5-P3-S4-notrans": (5, 1, 5, 3, 4, 0, 0),
    "C8-P3-S2-cls2": (8, 1, 8, 3, 2, 2, 0),
    "C8-G2-P7-S4-notrans": (8, 2, 2, 7, 4, 0, 0),
}


@functools.lru_cache(maxsize=None)
def _single(name):
    """inputs, the float32 restatement and the float64 truth of one case, computed once"""
    C, G, OD, P, S, ncls, part = SINGLE[name]
    no_trans = ncls == 0
    prm = dr.params(SCALE, OD, G, P, part, S, 0.1, no_trans)
    pp = part or P
    for seed in range(100):
        rs = np.random.RandomState(1000 + seed)
        data = rs.standard_normal((B, C, H, W)).astype(np.float32)
        rois = _rois(rs)
        trans = rs.standard_normal((K, 2 * max(ncls, 1), pp, pp)).astype(np.float32)
        trans[5] *= 6.0
        dy = rs.standard_normal((K, OD, P, P)).astype(np.float32)
        info = {}
        truth = dr.forward(data, rois, trans, prm, np.float64, info)
        if info["skip_margin"] >= 1e-4:
            break
    assert info["skip_margin"] >= 1e-4, "no fixture met the condition"
    ref = dr.forward(data, rois, trans, prm, np.float32)
    assert np.array_equal(ref[1], truth[1]), "float32 and float64 keep different samples"
    bt = dr.backward(dy, data, rois, trans, prm, np.float64)
    br = dr.backward(dy, data, rois, trans, prm, np.float32)
    for a in (data, rois, trans, dy) + ref + truth + bt + br:
        a.setflags(write=False)
    return dict(prm=prm, data=data, rois=rois, trans=trans, dy=dy, ref=ref, truth=truth, bref=br, btruth=bt,
                no_trans=no_trans)


def _fused_rois(rs):
    """(B, 7, 4) in a 64 x 80 image; canonical scale 16 puts sizes < 8 on stride 4, 8-16 on 8, 16-32 on 16, the rest on 32"""
    out = np.zeros((B, 7, 4), np.float32)
    sizes = [(5, 6), (11, 12), (22, 25), (50, 44), (3, 30), (60, 9), (14, 40)]
    for b in range(B):
        for i, (w, h) in enumerate(sizes):
            x = rs.uniform(-4, 78 - w)
            y = rs.uniform(-4, 62 - h)
            out[b, i] = [x, y, x + w + rs.uniform(-0.4, 0.4), y + h + rs.uniform(-0.4, 0.4)]
    return out


@functools.lru_cache(maxsize=None)
def _fused(form):
    C, P = 5, 7
    for seed in range(100):
        rs = np.random.RandomState(2000 + seed)
        feats = tuple(rs.standard_normal((B, C) + s).astype(np.float32) for s in FSHAPES)
        rois = _fused_rois(rs)
        trans = rs.standard_normal((B * 7, 2, P, P) if form == "C" else (B * 7, 2)).astype(np.float32)
        dy = rs.standard_normal((B * 7, C, P, P)).astype(np.float32)
        info = {}
        truth = dr.tsd_forward(feats, rois, trans, FSTRIDES, P, form, scale0=16, dt=np.float64, info=info)
        target = dr.assign_levels(rois, FSTRIDES, 16, 4, np.float64)
        if info["skip_margin"] >= 1e-4 and info["level_margin"] >= 1e-4 and set(target.ravel()) == set(FSTRIDES):
            break
    assert info["skip_margin"] >= 1e-4 and info["level_margin"] >= 1e-4 and set(target.ravel()) == set(FSTRIDES)
    assert np.array_equal(target, dr.assign_levels(rois, FSTRIDES, 16, 4, np.float32))
    ref = dr.tsd_forward(feats, rois, trans, FSTRIDES, P, form, scale0=16, dt=np.float32)
    assert np.array_equal(ref[1], truth[1])
    assert (truth[1][:, 2:] > 0).any(), "the masked RoI keeps samples on strides 16 and 32"
    bt = dr.tsd_backward(dy, feats, rois, trans, FSTRIDES, P, form, scale0=16, dt=np.float64)
    br = dr.tsd_backward(dy, feats, rois, trans, FSTRIDES, P, form, scale0=16, dt=np.float32)
    return dict(feats=feats, rois=rois, trans=trans, dy=dy, ref=ref, truth=truth, bref=br, btruth=bt, P=P)


# ------------------------------------------------------------------------------------------ CPU --
def _torch_forward(data, rois, trans, prm):
    """float64 torch restatement of the forward, differentiable in data and trans (floor / ceil / the skip test
    are piecewise constant; the clamp is left out: the inputs of the test below clamp nothing)"""
    import torch
    P, S, std, scale = prm["pooled_size"], prm["sample_per_part"], prm["trans_std"], prm["spatial_scale"]
    part = prm["part_size"] or P
    Kn, OD = rois.shape[0], prm["output_dim"]
    ncls = trans.shape[1] // 2
    cpc = OD // ncls
    Hh, Ww = data.shape[2:]
    rnd = lambda v: float(np.sign(v) * np.floor(abs(v) + 0.5))
    rows = []
    for n in range(Kn):
        b = int(rois[n, 0])
        x1, y1, x2, y2 = [float(v) for v in rois[n, 1:]]
        rsw, rsh = rnd(x1) * scale - 0.5, rnd(y1) * scale - 0.5
        rw = max((rnd(x2) + 1) * scale - 0.5 - rsw, 0.1)
        rh = max((rnd(y2) + 1) * scale - 0.5 - rsh, 0.1)
        for ctop in range(OD):
            cls = ctop // cpc
            for ph in range(P):
                for pw in range(P):
                    part_h, part_w = int(np.floor(ph / P * part)), int(np.floor(pw / P * part))
                    ws = pw * rw / P + rsw + trans[n, 2 * cls, part_h, part_w] * std * rw
                    hs = ph * rh / P + rsh + trans[n, 2 * cls + 1, part_h, part_w] * std * rh
                    vals = []
                    for ih in range(S):
                        for iw in range(S):
                            w, h = ws + iw * rw / P / S, hs + ih * rh / P / S
                            wv, hv = float(w.detach()), float(h.detach())
                            if not (-0.5 <= wv <= Ww - 0.5 and -0.5 <= hv <= Hh - 0.5):
                                continue
                            x0, y0 = int(np.floor(wv)), int(np.floor(hv))
                            dx, dy = w - x0, h - y0
                            d = data[b, ctop]
                            vals.append((1 - dx) * (1 - dy) * d[y0, x0] + (1 - dx) * dy * d[y0 + 1, x0] +
                                        dx * (1 - dy) * d[y0, x0 + 1] + dx * dy * d[y0 + 1, x0 + 1])
                    rows.append(sum(vals) / len(vals) if vals else torch.zeros((), dtype=torch.float64))
    return torch.stack(rows).reshape(Kn, OD, P, P)


def test_restated_backward_is_the_gradient_of_the_restated_forward():
    import torch
    prm = dr.params(0.25, 4, 1, 3, 2, 2, 0.1, False)
    for seed in range(200):
        rs = np.random.RandomState(seed)
        data = rs.standard_normal((2, 4, 13, 17)).astype(np.float32)
        rois = np.float32([[0, 9, 7, 41, 33], [1, 12.5, 9.5, 50, 40], [0, 20, 16, 30, 28]])
        rois[:, 1:] += rs.uniform(-0.4, 0.4, (3, 4)).astype(np.float32)
        trans = (rs.standard_normal((3, 4, 2, 2)) * 0.5).astype(np.float32)
        info = {}
        dr.forward(data, rois, trans, prm, np.float64, info)
        if not info.get("clamped") and info["int_margin"] >= 1e-3 and info["skip_margin"] >= 1e-3:
            break
    assert not info.get("clamped") and info["int_margin"] >= 1e-3
    dy = rs.standard_normal((3, 4, 3, 3))
    td = torch.tensor(data, dtype=torch.float64, requires_grad=True)
    tt = torch.tensor(trans, dtype=torch.float64, requires_grad=True)
    out = _torch_forward(td, rois, tt, prm)
    want = dr.forward(data, rois, trans, prm, np.float64)
    np.testing.assert_allclose(out.detach().numpy(), want[0], rtol=1e-12, atol=1e-13)
    out.backward(torch.tensor(dy))
    dd, dt, _, _ = dr.backward(dy, data, rois, trans, prm, np.float64)
    assert np.abs(dt).min() > 0
    np.testing.assert_allclose(dd, td.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dt, tt.grad.numpy(), rtol=1e-9, atol=1e-12)


def _clamped_case():
    """One sample (P = S = 1, scale 1, trans_std 0.25) of RoI [0, 1, 0, 2] on data[y, x] = 10 y + x (4 x 4):
    roi_start_w = -0.5, roi_w = 1, trans_x = 1 -> w = -0.25: kept (>= -0.5) and clamped to 0, x0 = x1 = 0;
    roi_start_h = 0.5, roi_h = 2, trans_y = 0.5 -> h = 0.75: y0 = 0, y1 = 1, dy = 0.75.
    out = 0.25 * 0 + 0.75 * 10 = 7.5.  With dY = 2 (g = 2): the x terms cancel (both neighbours are pixel 0),
    gy = (U01 - U00) * trans_std * g * roi_h = 10 * 0.25 * 2 * 2 = 10: a gradient at a clamped sample."""
    data = (10.0 * np.arange(4)[:, None] + np.arange(4)[None, :]).astype(np.float32).reshape(1, 1, 4, 4)
    rois = np.float32([[0, 0, 1, 0, 2]])
    trans = np.float32([1.0, 0.5]).reshape(1, 2, 1, 1)
    return data, rois, trans, dr.params(1.0, 1, 1, 1, 0, 1, 0.25, False), np.float32([2]).reshape(1, 1, 1, 1)


def test_known_answer_d_trans_at_a_clamped_sample():
    data, rois, trans, prm, dy = _clamped_case()
    for dt in (np.float32, np.float64):
        info = {}
        out, cnt, _ = dr.forward(data, rois, trans, prm, dt, info)
        assert info["clamped"] and out.ravel().tolist() == [7.5] and cnt.ravel().tolist() == [1.0]
        dd, dtr, _, _ = dr.backward(dy, data, rois, trans, prm, dt)
        assert dtr.ravel().tolist() == [0.0, 10.0]
        want = np.zeros((4, 4))
        want[0, 0], want[1, 0] = 0.5, 1.5
        assert np.array_equal(dd[0, 0], want)


def test_round_is_half_away_from_zero():
    assert dr.c_round(np.float32(2.5)) == 3 and dr.c_round(np.float64(-2.5)) == -3 and np.round(2.5) == 2
    assert dr.c_round(np.float32(0.5)) == 1 and dr.c_round(np.float32(-0.49)) == 0
    data = np.random.RandomState(0).standard_normal((1, 1, 8, 8)).astype(np.float32)
    prm = dr.params(1.0, 1, 1, 2, 0, 2, 0.1, True)
    a = dr.forward(data, np.float32([[0, 2.5, 0.5, 4.5, 5]]), np.zeros((1, 2, 2, 2), np.float32), prm)[0]
    b = dr.forward(data, np.float32([[0, 3, 1, 5, 5]]), np.zeros((1, 2, 2, 2), np.float32), prm)[0]
    assert np.array_equal(a, b)


def test_masked_roi_bins_per_stride():
    """the config's levels (800 x 1333 padded to 32) in float32: strides 4 and 8 keep nothing, 16 keeps the bins
    with ph >= 4 and pw >= 4, 32 those with ph >= 2 and pw >= 2 -- all of them reading pixel (0, 0) alone"""
    for stride, lo in ((4, None), (8, None), (16, 4), (32, 2)):
        h, w = -(-800 // stride), -(-1344 // stride)
        bins, pixels = dr.quirk_bins(h, w, stride, 7, 4, np.float32)
        want = [] if lo is None else [(ph, pw) for ph in range(7) for pw in range(7) if ph >= lo and pw >= lo]
        assert bins == want, stride
        assert pixels == (set() if lo is None else {(0, 0)})
        assert dr.quirk_bins(h, w, stride, 7, 4, np.float64)[0] == want


def test_fixtures_meet_their_conditions_and_the_restatements_agree():
    """generating a fixture asserts its conditions (same samples kept, same levels in float32 and float64); the
    float32 restatement's k is finite everywhere, i.e. it is exactly zero wherever the truth has no term.  (k itself
    is not small: a coordinate up to ~20 pixels carries its ulp into dx / dy absolutely, which an element whose
    weights are tiny sees as a large multiple of eps32 * T.  The device evaluates the same float32 coordinates.)"""
    for name in SINGLE:
        c = _single(name)
        ks = [dr.k_of(c["ref"][0], c["truth"][0], c["truth"][2]), dr.k_of(c["bref"][0], c["btruth"][0], c["btruth"][2]),
              dr.k_of(c["bref"][1], c["btruth"][1], c["btruth"][3])]
        print(name, ["%.2f" % k for k in ks])
        assert np.isfinite(ks).all() and max(ks) < 1e6 and ks[0] > 0
        assert not c["truth"][1][2].any() and c["truth"][1][3].any() and c["truth"][1][1].min() < c["truth"][1][1].max()
        assert c["no_trans"] or c["truth"][1][5].min() < c["prm"]["sample_per_part"] ** 2     # offsets push samples out
    for form in "CR":
        c = _fused(form)
        ks = [dr.k_of(c["ref"][0], c["truth"][0], c["truth"][2]), dr.k_of(c["bref"][1], c["btruth"][1], c["btruth"][3])]
        ks += [dr.k_of(a, b, t) for a, b, t in zip(c["bref"][0], c["btruth"][0], c["btruth"][2])]
        print(form, ["%.2f" % k for k in ks])
        assert np.isfinite(ks).all() and max(ks) < 1e6


P256 = ctypes.c_void_p(256)    # never dereferenced: every case fails validation first


def _single_abi(name, *, ptr=P256, B=2, C=8, Hh=13, Ww=17, Kn=6, ncls=1, od=8, G=1, P=7, part=0, S=4, no_trans=0):
    tail = (B, C, Hh, Ww, Kn, ncls, 0.25, od, G, P, part, S, 0.1, no_trans, None)
    if name == "sd_deform_psroi_pool_fwd":
        return _lib.lib().call(name, ptr, ptr, ptr, ptr, ptr, *tail)
    return _lib.lib().call(name, ptr, ptr, ptr, ptr, ptr, ptr, ptr, ptr, 1, 1, 1, *tail)


@pytest.mark.parametrize("name", ["sd_deform_psroi_pool_fwd", "sd_deform_psroi_pool_bwd"])
def test_single_level_entry_points_reject_bad_arguments(name):
    E = _lib.SimpleDetOpsError
    with pytest.raises(E, match="null pointer"):
        _single_abi(name, ptr=None)
    with pytest.raises(E, match="output_dim \\* group_size\\^2"):
        _single_abi(name, C=9)
    with pytest.raises(E, match="output_dim \\* group_size\\^2"):
        _single_abi(name, G=2)
    with pytest.raises(E, match="not a multiple of num_classes"):
        _single_abi(name, ncls=3)
    with pytest.raises(E, match="pooled_size must be at least 1"):
        _single_abi(name, P=0)
    with pytest.raises(E, match="part_size must not be negative"):
        _single_abi(name, part=-1)
    with pytest.raises(E, match="sample_per_part must be at least 1"):
        _single_abi(name, S=0)
    with pytest.raises(E, match="negative dimension"):
        _single_abi(name, Kn=-1)
    with pytest.raises(E, match="do not fit in LDS") as e:
        _single_abi(name, P=14, S=8)
    assert e.value.code == _lib.SD_ERR_UNSUPPORTED
    if name.endswith("fwd"):   # no_trans: num_classes is not read; no RoI: nothing to do
        assert _single_abi(name, ncls=3, no_trans=1, Kn=0, ptr=None) == 0


# (num_classes, pooled_size, sample_per_part): 32 x 32 x 4 and 22..45 bins of one sample have a table the forward
# could hold, but not together with the backward's per-wave sums where U = num_classes * P^2 is large
SUPPORT_GRID = [(1, 7, 4), (2, 7, 4), (5, 7, 4), (6, 7, 4), (1, 14, 4), (1, 14, 8), (1, 32, 2), (1, 32, 1), (1, 45, 1),
                (1, 64, 1), (1, 65, 1), (2, 22, 1), (4, 22, 1), (1, 3, 21), (1, 3, 22), (1, 1, 64), (1, 1, 65), (9, 7, 3)]


def test_forward_backward_and_the_predicate_take_the_same_sets():
    """one supported set: sd_deform_psroi_pool_supported == 'the forward takes it' == 'the backward takes it', for the
    single-level and (one class) the fused entry points.  No RoI and no image: a taken set returns before any launch."""
    l = _lib.lib()
    seen = set()
    for ncls, P, S in SUPPORT_GRID:
        want = bool(l.cdll.sd_deform_psroi_pool_supported(ncls, P, S))
        seen.add(want)
        names = ["sd_deform_psroi_pool_fwd", "sd_deform_psroi_pool_bwd"]
        calls = [lambda n=n: _single_abi(n, ptr=None, B=0, Kn=0, ncls=ncls, od=ncls, C=ncls, P=P, S=S) for n in names]
        if ncls == 1:
            calls += [lambda n=n: _fused_abi(n, Bn=0, R=0, P=P, tpart=P, S=S)
                      for n in ("sd_fpn_deform_roi_pool_fwd", "sd_fpn_deform_roi_pool_bwd")]
        for call in calls:
            if want:
                assert call() == 0, (ncls, P, S)
            else:
                with pytest.raises(_lib.SimpleDetOpsError, match="do not fit in LDS") as e:
                    call()
                assert e.value.code == _lib.SD_ERR_UNSUPPORTED, (ncls, P, S)
    assert seen == {True, False}
    got = {c: bool(l.cdll.sd_deform_psroi_pool_supported(*c)) for c in SUPPORT_GRID}
    assert got[(1, 7, 4)] and got[(5, 7, 4)] and got[(1, 14, 4)] and not got[(1, 32, 2)] and not got[(1, 14, 8)]
    for bad in ((0, 7, 4), (1, 0, 4), (1, 7, 0), (-1, 7, 4), (1, 1 << 20, 1 << 20)):
        assert l.cdll.sd_deform_psroi_pool_supported(*bad) == 0


def _fused_abi(name, *, ptr=P256, lv=P256, nlvl=4, Bn=2, C=5, R=7, P=7, tpart=7, S=4, hs=(16, 8, 4, 2)):
    n = max(nlvl, 1)
    feats = (ctypes.c_void_p * n)(*[lv.value if lv else None] * n) if lv is not False else None
    ia = lambda v: (ctypes.c_int * n)(*(list(v) + [1] * n)[:n])
    geo = (ia(hs), ia((20, 10, 5, 3)), ia((4, 8, 16, 32)), nlvl)
    tail = (Bn, C, R, P, tpart, S, 0.1, 224.0, 4.0, None)
    if name == "sd_fpn_deform_roi_pool_fwd":
        return _lib.lib().call(name, feats, *geo, ptr, ptr, ptr, ptr, *tail)
    return _lib.lib().call(name, ptr, feats, feats, *geo, ptr, ptr, ptr, ptr, 1, 1, *tail)


@pytest.mark.parametrize("name", ["sd_fpn_deform_roi_pool_fwd", "sd_fpn_deform_roi_pool_bwd"])
def test_fused_entry_points_reject_bad_arguments(name):
    E = _lib.SimpleDetOpsError
    with pytest.raises(E, match="null pointer"):
        _fused_abi(name, ptr=None)
    with pytest.raises(E, match="null pointer"):
        _fused_abi(name, lv=False)
    with pytest.raises(E, match="null pointer"):
        _fused_abi(name, lv=None)
    for nlvl in (0, 6):
        with pytest.raises(E, match="nlvl=%d out of range" % nlvl):
            _fused_abi(name, nlvl=nlvl)
    with pytest.raises(E, match="pooled_size must be at least 1"):
        _fused_abi(name, P=0, tpart=0)
    with pytest.raises(E, match="sample_per_part must be at least 1"):
        _fused_abi(name, S=0)
    with pytest.raises(E, match="trans_part must be 1 or pooled_size"):
        _fused_abi(name, tpart=3)
    with pytest.raises(E, match="C must be at least 1"):
        _fused_abi(name, C=0)
    with pytest.raises(E, match="bad H/W/stride"):
        _fused_abi(name, hs=(16, 0, 4, 2))
    with pytest.raises(E, match="negative dimension"):
        _fused_abi(name, R=-1)


# ------------------------------------------------------------------------------------------ GPU --
SENT = 12345.0
GUARD = 64


class _Guarded:
    """a device array between two runs of sentinels; offset: its pointer sits 4 bytes off a 16-byte boundary"""

    def __init__(self, shape, fill=float("nan"), offset=False):
        import torch
        n = int(np.prod(shape))
        self.lo = GUARD + (1 if offset else 0)
        self.buf = torch.full((self.lo + n + GUARD,), SENT, dtype=torch.float32, device="cuda")
        self.t = self.buf[self.lo:self.lo + n].view(shape)
        if isinstance(fill, np.ndarray):
            self.t.copy_(torch.from_numpy(np.array(fill, np.float32)))
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (4 if offset else 0)

    def get(self):
        b = self.buf.cpu().numpy()
        n = self.t.numel()
        assert np.all(b[:self.lo] == SENT) and np.all(b[self.lo + n:] == SENT), "wrote outside the array"
        return b[self.lo:self.lo + n].reshape(tuple(self.t.shape)).copy()


def _cuda(a, offset=False):
    return _Guarded(a.shape, np.ascontiguousarray(a), offset).t


def _bound(name, what, got, truth, T, ref):
    k_ref, k_gpu = dr.k_of(ref, truth, T), dr.k_of(got, truth, T)
    print("%s %s: k_ref %.3f  k_gpu %.3f  bound %.3f" % (name, what, k_ref, k_gpu, 2 * k_ref + 2))
    assert k_gpu <= 2 * k_ref + 2, "%s %s: k_gpu %.3f > 2 * %.3f + 2" % (name, what, k_gpu, k_ref)


def _single_kw(c):
    p = c["prm"]
    return dict(spatial_scale=p["spatial_scale"], output_dim=p["output_dim"], group_size=p["group_size"],
                pooled_size=p["pooled_size"], part_size=p["part_size"], sample_per_part=p["sample_per_part"],
                trans_std=p["trans_std"], no_trans=p["no_trans"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SINGLE))
def test_hip_single_level(ops, name):
    import torch
    c = _single(name)
    offset = name in ("C5-P7-S4-cls1", "C8-G2-P7-S2-cls2-part3")
    kw = _single_kw(c)
    data, rois, dy = _cuda(c["data"], offset), _cuda(c["rois"], offset), _cuda(c["dy"], offset)
    trans = None if c["no_trans"] else _cuda(c["trans"], offset)
    shape = c["ref"][0].shape
    out, cnt = _Guarded(shape, offset=offset), _Guarded(shape, offset=offset)
    ops.deform_psroi_pool_forward(data, rois, trans, out=out.t, top_count=cnt.t, **kw)
    got_out, got_cnt = out.get(), cnt.get()
    assert np.array_equal(got_cnt, c["ref"][1]), name + ": top_count"
    assert not got_out[2].any() and not got_cnt[2].any(), "the RoI off the map pools nothing"
    _bound(name, "out", got_out, c["truth"][0], c["truth"][2], c["ref"][0])
    # backward: write, then add onto a base
    rs = np.random.RandomState(7)
    dd, dtr, Td, Tt = c["btruth"]
    g_d = _Guarded(c["data"].shape, offset=offset)
    g_t = None if c["no_trans"] else _Guarded(c["trans"].shape, offset=offset)
    bkw = dict(kw, d_data=g_d.t, d_trans=None if g_t is None else g_t.t)
    _, d_rois, _ = ops.deform_psroi_pool_backward(dy, data, rois, trans, cnt.t, **bkw)
    assert not d_rois.cpu().numpy().any()
    got_d = g_d.get()
    assert np.array_equal(got_d == 0, Td == 0), name + ": d_data is touched exactly where a tap lands"
    _bound(name, "d_data", got_d, dd, Td, c["bref"][0])
    if g_t is not None:
        first = g_t.get()
        _bound(name, "d_trans", first, dtr, Tt, c["bref"][1])
        assert not first[2].any(), "no gradient from the RoI off the map"
    base_d = rs.standard_normal(c["data"].shape).astype(np.float32)
    base_t = rs.standard_normal(c["trans"].shape).astype(np.float32)
    a_d = _Guarded(c["data"].shape, base_d, offset)
    a_t = None if c["no_trans"] else _Guarded(c["trans"].shape, base_t, offset)
    _, d_rois, _ = ops.deform_psroi_pool_backward(dy, data, rois, trans, cnt.t, req_data="add", req_rois="add",
                                                  req_trans="add", **dict(kw, d_data=a_d.t,
                                                                          d_trans=None if a_t is None else a_t.t))
    assert d_rois is None
    _bound(name, "d_data (add)", a_d.get(), base_d + dd, np.abs(base_d) + Td, base_d + c["bref"][0])
    if a_t is not None:
        _bound(name, "d_trans (add)", a_t.get(), base_t + dtr, np.abs(base_t) + Tt, base_t + c["bref"][1])
        # equal bits on a second call
        again = _Guarded(c["trans"].shape, offset=offset)
        ops.deform_psroi_pool_backward(dy, data, rois, trans, cnt.t, **dict(kw, d_trans=again.t))
        assert np.array_equal(again.get().view(np.int32), first.view(np.int32)), "d_trans is not reproducible"
    out2, cnt2 = ops.deform_psroi_pool_forward(data, rois, trans, **kw)
    assert np.array_equal(out2.cpu().numpy().view(np.int32), got_out.view(np.int32))
    assert np.array_equal(cnt2.cpu().numpy(), got_cnt)


def _exact_single():
    """scale 0.5, P = S = 2, trans_std 0.25, W = H = 8, integer data: RoI [0, 0, 15, 15] has roi_start -0.5,
    roi_w 8, sub-bin 2, so without offset its samples sit at -0.5 (kept, clamped), 1.5, 3.5, 5.5; trans 1 moves
    them by 2: 1.5 .. 7.5 = W - 0.5 (kept, clamped); trans 0.25 by 0.5: 0, 2, 4, 6 (on pixels); trans 2 by 4:
    the last two (7.5 + 2, ...) are skipped; trans -1: the first (-2.5) is skipped."""
    rs = np.random.RandomState(11)
    data = rs.randint(-8, 9, (1, 2, 8, 8)).astype(np.float32)
    rois = np.float32([[0, 0, 0, 15, 15]] * 5)
    tv = [0.0, 1.0, 0.25, 2.0, -1.0]
    trans = np.float32([[np.full((2, 2), t), np.full((2, 2), -t if t == 2.0 else t)] for t in tv])
    dy = rs.randint(-4, 5, (5, 2, 2, 2)).astype(np.float32) * 4
    return data, rois, trans, dr.params(0.5, 2, 1, 2, 0, 2, 0.25, False), dy


def test_exact_cases_restated_in_both_precisions():
    data, rois, trans, prm, dy = _exact_single()
    a, b = dr.forward(data, rois, trans, prm, np.float32), dr.forward(data, rois, trans, prm, np.float64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    cnt = a[1][:, 0]
    assert (cnt[0] == 4).all() and (cnt[1] == 4).all() and (cnt[2] == 4).all()     # -0.5 and W - 0.5 are kept
    assert cnt[3].tolist() == [[4, 2], [2, 1]] or cnt[3][0, 1] < 4                 # samples pushed past W - 0.5
    assert (cnt[4] < 4).any()
    x, y = dr.backward(dy, data, rois, trans, prm, np.float32), dr.backward(dy, data, rois, trans, prm, np.float64)
    assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


@pytest.mark.gpu
def test_hip_exact_branch_cases(ops):
    data, rois, trans, prm, dy = _exact_single()
    want = dr.forward(data, rois, trans, prm, np.float32)
    kw = _single_kw(dict(prm=prm))
    out, cnt = ops.deform_psroi_pool_forward(_cuda(data), _cuda(rois), _cuda(trans), **kw)
    assert np.array_equal(cnt.cpu().numpy(), want[1]) and np.array_equal(out.cpu().numpy(), want[0])
    dd, _, dt = ops.deform_psroi_pool_backward(_cuda(dy), _cuda(data), _cuda(rois), _cuda(trans), cnt, **kw)
    wd, wt, _, _ = dr.backward(dy, data, rois, trans, prm, np.float32)
    assert np.array_equal(dd.cpu().numpy(), wd) and np.array_equal(dt.cpu().numpy(), wt)
    # the clamped known answer of the CPU part
    data, rois, trans, prm, dy = _clamped_case()
    kw = _single_kw(dict(prm=prm))
    out, cnt = ops.deform_psroi_pool_forward(_cuda(data), _cuda(rois), _cuda(trans), **kw)
    assert out.item() == 7.5 and cnt.item() == 1.0
    _, _, dt = ops.deform_psroi_pool_backward(_cuda(dy), _cuda(data), _cuda(rois), _cuda(trans), cnt, **kw)
    assert dt.cpu().numpy().ravel().tolist() == [0.0, 10.0]


def _exact_fused():
    """P = 8, S = 2, integer data, RoIs [0, 0, 31, 31] and [4, 8, 19, 39] on stride 4 (scale 0.25: every
    coordinate is a multiple of 1/4 or 1/8), zero offsets, trans_std 0.25: the own level's values and every term of
    both gradients are exact, and strides 16 and 32 add feat[b, c, 0, 0] to the bins the masked RoI keeps there"""
    rs = np.random.RandomState(12)
    feats = tuple(rs.randint(-8, 9, (1, 3) + s).astype(np.float32) for s in FSHAPES)
    rois = np.float32([[[0, 0, 31, 31], [4, 8, 19, 39]]])
    trans = np.zeros((2, 2, 8, 8), np.float32)
    dy = rs.randint(-4, 5, (2, 3, 8, 8)).astype(np.float32) * 16
    return feats, rois, trans, dy


def test_exact_fused_case_restated_in_both_precisions():
    feats, rois, trans, dy = _exact_fused()
    a = dr.tsd_forward(feats, rois, trans, FSTRIDES, 8, "C", S=2, trans_std=0.25, dt=np.float32)
    b = dr.tsd_forward(feats, rois, trans, FSTRIDES, 8, "C", S=2, trans_std=0.25, dt=np.float64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    cnt = a[1]
    assert (cnt[:, 0] > 0).all() and not cnt[:, 1].any() and cnt[:, 2].any() and cnt[:, 3].any()
    for l, s in ((2, 16), (3, 32)):
        bins, pixels = dr.quirk_bins(FSHAPES[l][0], FSHAPES[l][1], s, 8, 2)
        assert pixels == {(0, 0)} and sorted(bins) == sorted(zip(*np.nonzero(cnt[0, l])))
    own = dr.forward(feats[0], np.float32([[0, 0, 0, 31, 31]]), trans[:1], dr.params(0.25, 3, 1, 8, 0, 2, 0.1, False))[0]
    extra = sum((cnt[0, l] > 0)[None] * feats[l][0, :, 0, 0][:, None, None] for l in (2, 3))
    assert np.array_equal(a[0][0], own[0] + extra)


@pytest.mark.gpu
def test_hip_exact_fused_quirk(ops):
    feats, rois, trans, dy = _exact_fused()
    want = dr.tsd_forward(feats, rois, trans, FSTRIDES, 8, "C", S=2, trans_std=0.25, dt=np.float32)
    tf = [_cuda(f) for f in feats]
    out, cnt = ops.fpn_deform_roi_pool_forward(tf, _cuda(rois), _cuda(trans), FSTRIDES, 8, sample_per_part=2, trans_std=0.25)
    assert np.array_equal(cnt.cpu().numpy(), want[1]) and np.array_equal(out.cpu().numpy(), want[0])
    dfs, dt = ops.fpn_deform_roi_pool_backward(_cuda(dy), tf, _cuda(rois), _cuda(trans), cnt, FSTRIDES, 8,
                                               sample_per_part=2, trans_std=0.25)
    wf, wt, _, _ = dr.tsd_backward(dy, feats, rois, trans, FSTRIDES, 8, "C", S=2, trans_std=0.25, dt=np.float32)
    for l in range(4):
        assert np.array_equal(dfs[l].cpu().numpy(), wf[l]), "level %d" % l
    assert wf[2][0, :, 0, 0].any() and wf[3][0, :, 0, 0].any()     # the corner pixel receives those bins' gradient
    assert np.array_equal(dt.cpu().numpy(), wt)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["C", "R"])
def test_hip_fused_extractor(ops, form):
    import torch
    c = _fused(form)
    P, nl = c["P"], len(FSTRIDES)
    offset = form == "R"
    feats = [_cuda(f, offset) for f in c["feats"]]
    rois, trans, dy = _cuda(c["rois"], offset), _cuda(c["trans"], offset), _cuda(c["dy"], offset)
    out, cnt = _Guarded(c["ref"][0].shape, offset=offset), _Guarded(c["ref"][1].shape, offset=offset)
    ops.fpn_deform_roi_pool_forward(feats, rois, trans, FSTRIDES, P, roi_canonical_scale=16, out=out.t,
                                    top_count=cnt.t)
    got_out, got_cnt = out.get(), cnt.get()
    assert np.array_equal(got_cnt, c["ref"][1]), "top_count"
    _bound(form, "out", got_out, c["truth"][0], c["truth"][2], c["ref"][0])
    dfs, dtr, Tfs, Ttr = c["btruth"]
    g_f = [_Guarded(f.shape, offset=offset) for f in c["feats"]]
    g_t = _Guarded(c["trans"].shape, offset=offset)
    ops.fpn_deform_roi_pool_backward(dy, feats, rois, trans, cnt.t, FSTRIDES, P, roi_canonical_scale=16,
                                     d_feats=[g.t for g in g_f], d_trans=g_t.t)
    got_f, got_t = [g.get() for g in g_f], g_t.get()
    for l in range(nl):
        assert np.array_equal(got_f[l] == 0, Tfs[l] == 0), "level %d: pixels touched" % l
        _bound(form, "d_feat[%d]" % l, got_f[l], dfs[l], Tfs[l], c["bref"][0][l])
    _bound(form, "d_trans", got_t, dtr, Ttr, c["bref"][1])
    # add requests
    rs = np.random.RandomState(8)
    base_f = [rs.standard_normal(f.shape).astype(np.float32) for f in c["feats"]]
    base_t = rs.standard_normal(c["trans"].shape).astype(np.float32)
    a_f = [_Guarded(b.shape, b, offset) for b in base_f]
    a_t = _Guarded(base_t.shape, base_t, offset)
    ops.fpn_deform_roi_pool_backward(dy, feats, rois, trans, cnt.t, FSTRIDES, P, roi_canonical_scale=16,
                                     req_data="add", req_trans="add", d_feats=[g.t for g in a_f], d_trans=a_t.t)
    for l in range(nl):
        _bound(form, "d_feat[%d] (add)" % l, a_f[l].get(), base_f[l] + dfs[l], np.abs(base_f[l]) + Tfs[l],
               base_f[l] + c["bref"][0][l])
    _bound(form, "d_trans (add)", a_t.get(), base_t + dtr, np.abs(base_t) + Ttr, base_t + c["bref"][1])
    # the same from eight calls of the device's own single-level operator on the reference's masked inputs
    comp, comp_t = None, torch.zeros_like(trans)
    comp_f = []
    for l, (s, (lr, lo, own)) in enumerate(zip(FSTRIDES, dr._masked_inputs(c["rois"], c["trans"], FSTRIDES, P, form,
                                                                           16, 4, np.float32))):
        kw = dict(spatial_scale=1.0 / s, output_dim=5, group_size=1, pooled_size=P, part_size=0, sample_per_part=4,
                  trans_std=0.1, no_trans=False)
        tlr, tlo = _cuda(lr), _cuda(lo)
        o, tc = ops.deform_psroi_pool_forward(feats[l], tlr, tlo, **kw)
        assert np.array_equal(tc[:, 0].cpu().numpy(), got_cnt[:, l])
        comp = o if comp is None else comp + o
        dd, _, dl = ops.deform_psroi_pool_backward(dy, feats[l], tlr, tlo, tc, **kw)
        comp_f.append(dd.cpu().numpy())
        if form == "R":
            dl = dl.sum((2, 3))
        m = torch.from_numpy(own).cuda().view((-1,) + (1,) * (dl.dim() - 1))
        comp_t = comp_t + torch.where(m, dl, torch.zeros_like(dl)).view(trans.shape)
    comp = comp.cpu().numpy()
    assert np.array_equal(comp, got_out), "the fused out differs from the eight-call composition"
    _bound(form, "out (composition)", comp, c["truth"][0], c["truth"][2], c["ref"][0])
    _bound(form, "out vs composition", got_out, comp.astype(np.float64), c["truth"][2], comp)
    for l in range(nl):
        _bound(form, "d_feat[%d] (composition)" % l, comp_f[l], dfs[l], Tfs[l], c["bref"][0][l])
    _bound(form, "d_trans (composition)", comp_t.cpu().numpy(), dtr, Ttr, c["bref"][1])


@pytest.mark.gpu
def test_hip_equal_bits_over_calls_and_graph_replay(ops):
    import torch
    c = _fused("C")
    P = c["P"]
    feats = [_cuda(f) for f in c["feats"]]
    rois, trans, dy = _cuda(c["rois"]), _cuda(c["trans"]), _cuda(c["dy"])
    s1 = _single("C8-P7-S4-cls2-part3")
    kw = _single_kw(s1)
    sd, sr, st, sdy = _cuda(s1["data"]), _cuda(s1["rois"]), _cuda(s1["trans"]), _cuda(s1["dy"])

    def run():
        out, cnt = ops.fpn_deform_roi_pool_forward(feats, rois, trans, FSTRIDES, P, roi_canonical_scale=16)
        _, dt = ops.fpn_deform_roi_pool_backward(dy, feats, rois, trans, cnt, FSTRIDES, P, roi_canonical_scale=16,
                                                 req_data="null")
        o1, c1 = ops.deform_psroi_pool_forward(sd, sr, st, **kw)
        dd, _, t1 = ops.deform_psroi_pool_backward(sdy, sd, sr, st, c1, **kw)
        return [out, cnt, dt, o1, c1, t1]

    eager = [t.clone() for t in run()]
    for e, g in zip(eager, run()):
        assert torch.equal(e.view(torch.int32), g.view(torch.int32))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(s):
        with torch.cuda.graph(graph, stream=s):
            cap = run()
    for _ in range(2):
        for t in cap:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for e, g in zip(eager, cap):
            assert torch.equal(e.view(torch.int32), g.view(torch.int32))


@pytest.mark.gpu
def test_hip_autograd_functions(ops):
    import torch
    s1 = _single("C5-P7-S4-cls1")
    kw = _single_kw(s1)
    data = _cuda(s1["data"]).clone().requires_grad_()
    trans = _cuda(s1["trans"]).clone().requires_grad_()
    rois, dy = _cuda(s1["rois"]), _cuda(s1["dy"])
    out = ops.deform_psroi_pool(data, rois, trans, **kw)
    raw, cnt = ops.deform_psroi_pool_forward(data.detach(), rois, trans.detach(), **kw)
    assert torch.equal(out.detach(), raw)
    out.backward(dy)
    _, _, wt = ops.deform_psroi_pool_backward(dy, data.detach(), rois, trans.detach(), cnt, **kw)
    assert torch.equal(trans.grad, wt) and data.grad is not None
    c = _fused("R")
    feats = [_cuda(f).clone().requires_grad_() for f in c["feats"]]
    tr = _cuda(c["trans"]).clone().requires_grad_()
    out = ops.fpn_deform_roi_pool(feats, _cuda(c["rois"]), tr, FSTRIDES, c["P"], roi_canonical_scale=16)
    out.backward(_cuda(c["dy"]))
    assert all(f.grad is not None for f in feats) and tuple(tr.grad.shape) == tuple(c["trans"].shape)
