"""The FPN level rule where one ulp of log2 decides the level (tests/fpn_level_cases.py has the inputs and why they
are the sensitive ones).  Everything else in the fused RoIAlign is IEEE add / multiply / divide / sqrt; the rule's
log2f is the one function whose device form (a hardware approximation) need not return the correctly rounded
bits, and floor() makes a last-bit difference a different pyramid level: another (C, 7, 7) output row, a gradient
scattered into another level.

  CPU: the inputs' own conditions; the RoIs against the fixture's hash; the oracle against the fixture
       (tests/golden/fpn_assign_thresholds.npz: the reference's own class, run by tests/golden/make_golden.py).
  GPU: sd_fpn_roi_assign on every row of both pyramids; every fused entry point that applies the rule in a kernel
       of its own (forward on its three kernel families, packed and fp16 forward, the three backwards, the unfused
       graph, TSD's extractor) on the +-16 ulp neighbourhood of every default-pyramid threshold.
"""
import functools
import os

import numpy as np
import pytest

from . import deform_psroi_ref as dr
from . import fpn_level_cases as cases
from .test_roi_align import _assert_bwd_close, _decode_packed, _fwd_path

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fpn_assign_thresholds.npz")
STRIDES = list(cases.PYRAMIDS["p2_p5"][0])
SHAPES = ((128, 128), (64, 64), (32, 32), (16, 16))        # a 512 x 512 image
C = 8


def _t(a):
    import torch
    return torch.from_numpy(np.array(a)).cuda()      # a copy: the shared arrays are read-only


@functools.lru_cache(maxsize=None)
def _gold():
    with np.load(GOLDEN) as g:
        return {k: g[k] for k in g.files}


# ------------------------------------------------------------------------------------------ CPU --
@pytest.mark.parametrize("name", sorted(cases.PYRAMIDS))
def test_sweep_conditions_hold(oracle, name):
    strides, scale0, lvl0, thr = cases.PYRAMIDS[name]
    rois = cases.rois(name)
    assert rois.shape == (1, len(thr) * (2 * cases.HALF + 1) + len(cases.SPECIAL), 4)
    _, level = oracle.fpn_roi_assign(rois, list(strides), scale0, lvl0)
    counts = cases.conditions(name, level)
    print(name, "areas whose level one ulp of log2f moves:", counts)
    assert all(counts[c] >= 1 for c, _ in thr if c in cases.SENSITIVE)
    assert all(counts[c] == 0 for c, _ in thr if c not in cases.SENSITIVE)
    # the neighbourhood the RoIAlign tests use holds every sensitive area
    for label, c, offs, r in cases.segments(name):
        if c is not None:
            s = cases.sensitive(cases.area_of(r), strides, scale0, lvl0)
            assert np.all(np.abs(offs[s]) <= cases.NEAR), (name, label, offs[s])


@pytest.mark.parametrize("name", sorted(cases.PYRAMIDS))
def test_rois_regenerate_to_the_fixture_hash(name):
    g = _gold()
    strides, scale0, lvl0, thr = cases.PYRAMIDS[name]
    assert int(g["half"]) == cases.HALF
    assert g[name + "/strides"].tolist() == list(strides)
    assert g[name + "/canonical"].tolist() == [scale0, lvl0]
    assert g[name + "/thresholds"].tolist() == [[c, w] for c, w in thr]
    assert str(g[name + "/rois_sha256"]) == cases.sha256(cases.rois(name))
    assert g[name + "/level"].dtype == np.int8 and g[name + "/level"].shape == (cases.rois(name).shape[1],)


@pytest.mark.parametrize("name", sorted(cases.PYRAMIDS))
def test_oracle_equals_the_reference_class_on_every_row(oracle, name):
    strides, scale0, lvl0, _ = cases.PYRAMIDS[name]
    want = _gold()[name + "/level"].astype(np.int32)
    rois = cases.rois(name)
    per, level = oracle.fpn_roi_assign(rois, list(strides), scale0, lvl0)
    bad = np.nonzero(level[0] != want)[0]
    assert not len(bad), "%s: oracle %s, reference %s at %s" % (name, level[0][bad], want[bad], cases.describe(name, bad))
    _assert_masked(per, rois, want, name)
    # what the special rows are there for
    sp = dict(zip([n for n, _ in cases.SPECIAL], want[-len(cases.SPECIAL):].tolist()))
    top = len(strides) - 1
    assert sp == dict(area_zero=0, area_negative=-1, area_inf=top, one_by_one=0, above_top=top, below_bottom=0)


def _assert_masked(per, rois, level, name):
    """per (nlvl, 1, n, 4): level l holds the RoIs assigned to it and zeros elsewhere"""
    for l in range(len(per)):
        m = level == l
        np.testing.assert_array_equal(per[l][0][m], rois[0][m], err_msg="%s level %d: own rows" % (name, l))
        assert np.all(per[l][0][~m] == 0), "%s level %d: rows of other levels are not zero" % (name, l)


# ------------------------------------------------------------------------------------------ GPU --
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(cases.PYRAMIDS))
def test_device_assign_equals_oracle_on_every_sweep_row(ops, oracle, name):
    """What the device returned at the sensitive rows is printed (pytest -s) before anything is asserted."""
    strides, scale0, lvl0, _ = cases.PYRAMIDS[name]
    rois = cases.rois(name)
    wper, want = oracle.fpn_roi_assign(rois, list(strides), scale0, lvl0)
    per, level = ops.fpn_roi_assign(_t(rois), list(strides), scale0, lvl0)
    got = level.cpu().numpy()
    at = 0
    for label, c, offs, r in cases.segments(name):
        if c is not None:
            s = np.nonzero(cases.sensitive(cases.area_of(r), strides, scale0, lvl0))[0]
            for i in s:
                print("%s %s %+d ulp (z = %r): device level %d, oracle %d"
                      % (name, label, offs[i], float(cases.z_of(cases.area_of(r[i]), scale0)), got[0, at + i],
                         want[0, at + i]))
        at += len(r)
    bad = np.nonzero(got[0] != want[0])[0]
    assert not len(bad), "%s: %d rows differ: %s" % (
        name, len(bad), ["%s: device %d oracle %d" % (d, g, w)
                         for d, g, w in zip(cases.describe(name, bad), got[0][bad], want[0][bad])])
    for l in range(len(strides)):
        np.testing.assert_array_equal(per[l].cpu().numpy(), wper[l], err_msg="%s: RoIs of level %d" % (name, l))


@functools.lru_cache(maxsize=None)
def _near():
    """the shared inputs and oracle results of the RoIAlign tests, computed once and left unchanged"""
    rois = cases.near_rois("p2_p5")
    assert rois.shape[1] == 3 * (2 * cases.NEAR + 1) + len(cases.SPECIAL) - 1 and np.isfinite(rois).all()
    rs = np.random.RandomState(77)
    feats = tuple(rs.standard_normal((1, C) + s).astype(np.float32) for s in SHAPES)
    dy = rs.standard_normal((1, rois.shape[1], C, 7, 7)).astype(np.float32)
    from oracle import pyoracle
    fwd = pyoracle.fpn_roi_align_fwd(feats, rois, STRIDES, (7, 7), nthreads=8)
    _, level = pyoracle.fpn_roi_assign(rois, STRIDES)
    assert set(level.ravel().tolist()) == {-1, 0, 1, 2, 3}
    bwd = tuple(pyoracle.fpn_roi_align_bwd(dy, rois, fwd[1], fwd[2], [f.shape for f in feats], STRIDES))
    for a in (rois, dy, level) + feats + tuple(fwd) + bwd:
        a.setflags(write=False)
    return dict(rois=rois, feats=feats, dy=dy, fwd=fwd, level=level, bwd=bwd, shapes=[f.shape for f in feats])


def _rows(which):
    """failure text: the RoIs (rows of near_rois) at which `which` (n,) is set"""
    return cases.describe("p2_p5", _near_index()[np.nonzero(which)[0]], cases.NEAR)


@functools.lru_cache(maxsize=None)
def _near_index():
    full = cases.rois("p2_p5", cases.NEAR)[0]
    return np.nonzero(np.isfinite(full).all(1))[0]


def _assert_rows_equal(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    differ = (got != want).reshape(got.shape[0], got.shape[1], -1).any(2)[0]
    assert not differ.any(), "%s differs at %s" % (what, _rows(differ))


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["band", "naive", "tiled"])
def test_fused_forward_bit_exact_at_the_thresholds(ops, variant):
    c = _near()
    tf, tr = [_t(f) for f in c["feats"]], _t(c["rois"])
    _fwd_path(variant)
    try:
        got = ops.fpn_roi_align_forward(tf, tr, STRIDES, (7, 7))
        outp, (am, con) = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, (7, 7))
    finally:
        _fwd_path("band")
    for g, w, what in zip(got, c["fwd"], ("output", "maxidx_x", "maxidx_y")):
        _assert_rows_equal(g.cpu().numpy(), w, "%s forward %s" % (variant, what))
    # the packed arg-max form: same output, and its codes decode to the oracle's float coordinates
    _assert_rows_equal(outp.cpu().numpy(), c["fwd"][0], "%s packed forward output" % variant)
    codes = ops.argmax_codes(am, (7, 7)).cpu().numpy()
    _assert_rows_equal(codes == 255, c["fwd"][1] == -1, "%s packed forward: bins that pooled nothing" % variant)
    dax, day = _decode_packed(codes, c["rois"], c["shapes"], STRIDES, c["level"])
    _assert_rows_equal(dax, c["fwd"][1], "%s packed forward: decoded x" % variant)
    _assert_rows_equal(day, c["fwd"][2], "%s packed forward: decoded y" % variant)


@pytest.mark.gpu
def test_fp16_forward_bit_exact_at_the_thresholds(ops, oracle):
    import torch
    c = _near()
    feats16 = [f.astype(np.float16) for f in c["feats"]]
    want = oracle.fpn_roi_align_fwd([f.astype(np.float32) for f in feats16], c["rois"], STRIDES, (7, 7), nthreads=8)
    tr = _t(c["rois"])
    out, (am, _) = ops.fpn_roi_align_forward_packed_f16([_t(f) for f in feats16], tr, STRIDES, (7, 7))
    assert out.dtype == torch.float16
    _assert_rows_equal(out.cpu().numpy(), want[0].astype(np.float16), "fp16 forward output")
    codes = ops.argmax_codes(am, (7, 7)).cpu().numpy()
    _assert_rows_equal(codes == 255, want[1] == -1, "fp16 forward: bins that pooled nothing")
    dax, day = _decode_packed(codes, c["rois"], c["shapes"], STRIDES, c["level"])
    _assert_rows_equal(dax, want[1], "fp16 forward: decoded x")
    _assert_rows_equal(day, want[2], "fp16 forward: decoded y")


def _assert_bwd(got, c, what):
    for l, (g, w) in enumerate(zip(got, c["bwd"])):
        g = g.cpu().numpy()
        _assert_bwd_close(g, w)
        # a RoI on the wrong level puts gradient where its true level's neighbours have none
        stray = (w == 0) & (g != 0)
        assert not stray.any(), "%s: level %d has gradient at %d pixels where the oracle has none" % (
            what, l, int(stray.sum()))


@pytest.mark.gpu
def test_fused_backwards_at_the_thresholds(ops):
    c = _near()
    # the oracle itself leaves most of every level untouched: the zero test below is not vacuous
    assert all((w == 0).mean() > 0.25 for w in c["bwd"])
    tf, tr, tdy = [_t(f) for f in c["feats"]], _t(c["rois"]), _t(c["dy"])
    _assert_bwd(ops.fpn_roi_align_backward(tdy, tr, _t(c["fwd"][1]), _t(c["fwd"][2]), c["shapes"], STRIDES), c,
                "float arg-max backward")
    out, st = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, (7, 7))
    _assert_rows_equal(out.cpu().numpy(), c["fwd"][0], "packed forward output")
    _assert_bwd(ops.fpn_roi_align_backward_packed(tdy, tr, st, c["shapes"], STRIDES), c, "packed backward")
    out, st = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, (7, 7), plan=True)
    assert len(st) == 3
    _assert_rows_equal(out.cpu().numpy(), c["fwd"][0], "planned packed forward output")
    _assert_bwd(ops.fpn_roi_align_backward_packed(tdy, tr, st, c["shapes"], STRIDES), c, "planned packed backward")


@pytest.mark.gpu
def test_unfused_graph_equals_the_fused_op_at_the_thresholds(ops):
    import torch
    c = _near()
    tf, tr = [_t(f) for f in c["feats"]], _t(c["rois"])
    per, level = ops.fpn_roi_assign(tr, STRIDES)
    np.testing.assert_array_equal(level.cpu().numpy(), c["level"])
    total = None
    for f, p, s in zip(tf, per, STRIDES):
        o, _, _ = ops.roi_align_v2_forward(f, p.contiguous(), (7, 7), 1.0 / s)
        total = o if total is None else total + o
    fused, _, _ = ops.fpn_roi_align_forward(tf, tr, STRIDES, (7, 7))
    assert torch.equal(fused, total), "differs at %s" % _rows((fused != total).flatten(2).any(2)[0].cpu().numpy())


TSD_P, TSD_S = 7, 2


@functools.lru_cache(maxsize=None)
def _tsd():
    """TSD's extractor with zero offsets on the same RoIs and maps: the float32 restatement, and the float64 truth
    of the same formulas on the float32 rule's levels (the level is what is under test; in float64 the rule itself
    would move the rows next to a threshold)"""
    c = _near()
    rois, feats = c["rois"], c["feats"]
    trans = np.zeros((rois.shape[1], 2, TSD_P, TSD_P), np.float32)
    ok = c["level"][0] >= 0                                    # (the NaN row's uint8 cast is whatever numpy makes of it)
    with np.errstate(invalid="ignore"):
        own = dr.assign_levels(rois, STRIDES)[0]
    assert np.array_equal(own[ok], np.array(STRIDES)[c["level"][0][ok]]), \
        "the restatement's level rule is not the oracle's"
    assert not np.isin(own[~ok], STRIDES).any()
    with np.errstate(invalid="ignore"):
        ref = dr.tsd_forward(feats, rois, trans, STRIDES, TSD_P, "C", S=TSD_S)
        masked = dr._masked_inputs(rois, trans, STRIDES, TSD_P, "C", 224, 4, np.float32)
    out = T = None
    cnts = []
    for f, s, (lr, lo, _) in zip(feats, STRIDES, masked):
        o, n, t = dr.forward(f, lr, lo, dr._tsd_prm(C, TSD_P, TSD_S, s, np.float64, 0.1), np.float64)
        out = o if out is None else out + o
        T = t if T is None else T + t
        cnts.append(n[:, 0])
    truth = (out, np.stack(cnts, 1), T)
    assert np.array_equal(ref[1], truth[1]), "float32 and float64 keep different samples"
    return dict(trans=trans, ref=ref, truth=truth)


@pytest.mark.gpu
def test_tsd_extractor_at_the_thresholds(ops):
    """tests/test_deform_psroi.py's rule: k = |got - truth| / (eps32 * T + tiny), k_gpu <= 2 * k_ref + 2.  A RoI
    pooled from another level is O(1) away, some 1e6 times the bound."""
    c, t = _near(), _tsd()
    out, cnt = ops.fpn_deform_roi_pool_forward([_t(f) for f in c["feats"]], _t(c["rois"]), _t(t["trans"]), STRIDES,
                                               TSD_P, sample_per_part=TSD_S)
    got_cnt, got = cnt.cpu().numpy(), out.cpu().numpy()
    differ = (got_cnt != t["ref"][1]).reshape(got_cnt.shape[0], -1).any(1)
    assert not differ.any(), "top_count differs at %s" % _rows(differ)
    k_ref, k_gpu = dr.k_of(t["ref"][0], t["truth"][0], t["truth"][2]), dr.k_of(got, t["truth"][0], t["truth"][2])
    print("tsd out: k_ref %.3f  k_gpu %.3f  bound %.3f" % (k_ref, k_gpu, 2 * k_ref + 2))
    if k_gpu > 2 * k_ref + 2:
        k = np.abs(got - t["truth"][0]) / (dr.EPS32 * t["truth"][2] + dr.TINY)
        worst = (k > 2 * k_ref + 2).reshape(k.shape[0], -1).any(1)
        raise AssertionError("k_gpu %.3f > 2 * %.3f + 2 at %s" % (k_gpu, k_ref, _rows(worst)))
