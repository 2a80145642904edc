"""The fp16 I/O entry points of the fused FPN RoIAlign and the two op-boundary casts, at odd plane offsets, cast tails
and the edges of fp16's value range.

The truth of every comparison is the CPU oracle in fp32 on the halves converted to float, rounded to fp16 by numpy
(round to nearest even, subnormals kept); fp16 results are compared by bits, so the sign of zero counts, and at NaN
positions only NaN-ness has to agree.  Device-against-device equalities (native against native=False, the fp16 entry
against the fp32 entry on converted maps) come on top of that, never instead.

  CPU: the geometries of tests/fp16_edges.py are not vacuous -- on the pyramids whose H W is odd every fp16 fill
       displacement 0..7 occurs on every level, displacement 7 meets band lengths of 8 k + 1 and 8 k + 2 halves (both
       corners of the LDS stride `((blen + 14) >> 3) * 8`), planes per fill 1, 2, 4 and 8 all meet odd displacements,
       the forward plans more than one band where R says so, the backward's bands have odd, 2 (mod 4) and 0 (mod 4)
       element counts, and the overflow / non-finite gradient cases hold what they are meant to hold.
  GPU: forward, backward (write and add) and the casts as the sections below say.
"""
import numpy as np
import pytest

from . import fp16_edges as E
from . import fx_verdict

STRIDES = E.STRIDES
NAMES = [g.name for g in E.GEOMS]
VALUE_GEOMS = ["b_c8_r300", "a_c3_r77_int"]      # C = 8 and C = 3, both on pyramids of odd H W
F16, F32 = np.float16, np.float32

_CACHE = {}


def reference(oracle, name, kind="normal"):
    """maps, RoIs and the oracle's forward of one geometry: computed once, shared, read-only"""
    key = (name, kind)
    if key not in _CACHE:
        g = E.BY_NAME[name]
        feats16 = E.make_feats16(g, kind)
        rois = E.make_rois(g)
        with np.errstate(all="ignore"):
            fw = oracle.fpn_roi_align_fwd([f.astype(F32) for f in feats16], rois, STRIDES, (g.pooled, g.pooled), nthreads=8)
            out16 = fw[0].astype(F16)
        for a in list(fw) + feats16 + [rois, out16]:
            a.setflags(write=False)
        _CACHE[key] = dict(geom=g, feats16=feats16, rois=rois, fw=fw, out16=out16, shapes=[f.shape for f in feats16])
    return _CACHE[key]


# ------------------------------------------------------------------------------------------------------ CPU --
def test_geometries_cover_the_parameters_asked_for():
    assert {g.C for g in E.GEOMS} == {1, 3, 6, 12, 8, 33}
    assert {g.B for g in E.GEOMS} == {1, 2, 3}
    assert {1, 7, 77} <= {g.R for g in E.GEOMS}
    assert {g.pooled for g in E.GEOMS} == {7, 14}
    assert any(g.round4 for g in E.GEOMS) and any(g.degenerate for g in E.GEOMS)
    for im in E.ODD_IMAGES:
        assert all((h * w) % 2 == 1 for h, w in E.shapes_of(im)), im
    assert any((h * w) % 8 == 4 or w % 4 == 0 for h, w in E.shapes_of(E.EVEN))
    # a few MB of device memory at most: maps (fp16 and fp32) and outputs (fp16, fp32, codes)
    for g in E.GEOMS:
        maps = g.B * g.C * sum(h * w for h, w in E.shapes_of(g.image))
        outs = g.B * g.R * g.C * g.pooled ** 2
        assert 6 * maps + 8 * outs < 8 << 20, g.name


def test_planes_per_fill_follow_the_launch_rule():
    """C = 1, 3, 6, 12, 8, 33 -> 1, 1, 2, 4, 8, 1 planes per fill wherever LDS holds that many (`P.g[l]`: the largest of
    1, 2, 4, 8 that divides C with g * bstride <= kBandBufFloats), fewer on the levels it does not"""
    nominal = {1: 1, 3: 1, 6: 2, 12: 4, 8: 8, 33: 1}
    seen = set()
    for g in E.GEOMS:
        shapes = E.shapes_of(g.image)
        plan = E.fwd_band_plan(shapes, g.C, g.R, g.pooled)
        gs = [p["g"] for p in plan]
        for p in plan:
            fits = [c for c in (1, 2, 4, 8) if g.C % c == 0 and c * p["bstride"] <= E.BAND_BUF_FLOATS]
            assert p["g"] == max(fits)
            assert p["g"] <= nominal[g.C]
        assert max(gs) == nominal[g.C], (g.name, gs)
        seen.add(max(gs))
    assert seen == {1, 2, 4, 8}


def test_every_fill_displacement_occurs_on_every_level_of_the_odd_pyramids():
    table = {}
    for g in E.GEOMS:
        for p in E.fwd_planes(g):
            table.setdefault((g.image, p["level"]), set()).add(p["disp"])
            table.setdefault((g.name, p["level"]), set()).add(p["disp"])
    for im in E.ODD_IMAGES:
        for l in range(4):
            assert table[im, l] == set(range(8)), (im, l, table[im, l])
    for g in E.GEOMS:   # eight planes of odd H W already take all eight
        if g.image in E.ODD_IMAGES and g.B * g.C >= 8:
            for l in range(4):
                assert table[g.name, l] == set(range(8)), (g.name, l)
    # what the suite had before: even displacements only
    for l, (h, w) in enumerate(((200, 334), (100, 167), (50, 84), (25, 42))):
        assert {(k * h * w) % 8 for k in range(64)} <= {0, 2, 4, 6}


def test_both_corners_of_the_fill_stride_and_every_fill_width_at_odd_displacements():
    planes = [(g.name, p) for g in E.GEOMS for p in E.fwd_planes(g)]
    for r in (1, 2):    # displacement 7 with blen = 8 k + r: the two cases ((blen + 14) >> 3) * 8 is sized for
        hit = [(n, p) for n, p in planes if p["disp"] == 7 and p["blen"] % 8 == r]
        assert hit, r
        for _, p in hit:   # (fwd_planes' bstride is the kernel's ((blen + 14) >> 3) * 8)
            if r == 1:     # the plane ends with the stride's last word
                assert 7 + p["blen"] == p["bstride"]
            else:          # one half in a word of its own: ceil(blen / 8) words would not hold it
                assert p["bstride"] - 8 < 7 + p["blen"] <= p["bstride"] and 7 + p["blen"] > ((p["blen"] + 7) >> 3) * 8
        if r == 2:   # ... and a plane behind it in the same fill, which a shorter stride would put on top of that half
            assert any(p["pos"] + 1 < p["g"] for _, p in hit)
    for gfill in (1, 2, 4, 8):
        assert any(p["g"] == gfill and p["disp"] % 2 == 1 for _, p in planes), gfill
        if gfill > 1:   # behind the first plane of a fill, where the consumer adds pos * (HW & 7) to the fill's shift
            assert any(p["g"] == gfill and p["pos"] > 0 and p["disp"] % 2 == 1 for _, p in planes), gfill


def test_forward_plans_more_than_one_band_where_the_item_count_says_so():
    """by_items = ceil(R POOL / levels / (0.8 cap)) with cap = kBandNP kBandWaves (64 / POOL) items per round"""
    for g in E.GEOMS:
        plan = E.fwd_band_plan(E.shapes_of(g.image), g.C, g.R, g.pooled)
        cap = E.BAND_NP * E.BAND_WAVES * (E.WAVE // g.pooled)
        many = (g.R * g.pooled // 4) * 5 > 4 * cap
        assert many == ((g.pooled == 7 and g.R >= 264) or (g.pooled == 14 and g.R >= 59)), g.name
        for p in plan:
            assert (p["nbands"] > 1) == many, (g.name, p)
    assert sum(E.BY_NAME[n].R == 300 for n in NAMES) >= 2


def test_backward_bands_have_odd_even_and_half2_element_counts():
    odd = two = four = 0
    for g in E.GEOMS:
        bands = E.bwd_bands(g)
        if g.image in E.ODD_IMAGES:
            assert all(b["count"] % 2 == 1 or b["band"] > 0 for b in bands)
            assert not any(b["half2"] for b in bands if b["count"] % 2)
        odd += sum(b["count"] % 2 == 1 for b in bands)
        two += sum(b["count"] % 4 == 2 for b in bands)
        four += sum(b["half2"] for b in bands)
    assert odd and two and four
    # the finest level of the 260 x 516 image is two bands, the first of odd length
    nb, rows, _ = fx_verdict.band_plan(E.shapes_of(E.ODD_B))
    assert nb[0] == 2 and (rows[0] * 129) % 2 == 1 and 65 * 129 * 4 > 27 * 1024
    # the even pyramid keeps the __half2 write-out covered on whole planes
    assert any(b["half2"] and b["level"] == 0 for b in E.bwd_bands(E.BY_NAME["e_c8_r77"]))
    assert any(b["count"] % 4 == 2 for b in E.bwd_bands(E.BY_NAME["e_c8_r77"]))


def test_every_level_has_rois_from_seven_rois_on(oracle):
    for g in E.GEOMS:
        if g.R >= 7:
            _, lvl = oracle.fpn_roi_assign(E.make_rois(g), STRIDES)
            assert set(range(4)) <= set(lvl.ravel().tolist()), g.name


@pytest.mark.parametrize("kind", ["subnormal", "max", "zeros", "nonfinite"])
@pytest.mark.parametrize("name", VALUE_GEOMS)
def test_forward_value_cases_hold_what_they_are_named_for(oracle, name, kind):
    ref = reference(oracle, name, kind)
    x = np.concatenate([f.ravel() for f in ref["feats16"]])
    o = ref["out16"].ravel()
    tiny = F16(2.0 ** -14)
    if kind == "subnormal":
        assert (np.abs(x[x != 0]) < tiny).mean() > 0.99
        assert ((np.abs(o) < tiny) & (o != 0)).mean() > 0.5
    elif kind == "max":
        assert (o == F16(65504)).sum() > 20 and np.isfinite(ref["fw"][0]).all()
        assert (ref["fw"][0] > 65504).any()      # sums of weights a rounding above 1: still 65504 after the rounding
        assert np.isfinite(o).all()
    elif kind == "zeros":
        assert (E.bits16(x) == 0x8000).sum() > 100 and (E.bits16(x) == 0).sum() > 100
        pooled = ref["fw"][1].ravel() != -1
        assert ((o == 0) & pooled).sum() > 20
        assert not (E.bits16(o) == 0x8000).any()   # add_n over the levels: -0 + 0 = +0
    else:
        assert np.isnan(x).sum() > 5 and (x == np.inf).sum() > 5 and (x == -np.inf).sum() > 5
        # a NaN sample never wins the maximum (value > maxval is false), +inf always does, and a bin whose every sample
        # is NaN keeps -FLT_MAX, which rounds to -inf: no NaN in the output, and outputs unlike the finite maps'
        clean = reference(oracle, name)["out16"].ravel()
        assert (o == np.inf).sum() > 5 and (E.bits16(o) != E.bits16(clean)).sum() > 20
        print("%s: %d +inf, %d -inf, %d NaN outputs" % (name, (o == np.inf).sum(), (o == -np.inf).sum(), np.isnan(o).sum()))


def test_overflow_case_straddles_the_largest_half(oracle):
    c = overflow_case(oracle)
    w, mass = c["want"], c["mass"]
    big = np.abs(w) > 32768
    over = np.abs(w) > 65520 + 1e-4 * mass
    under = big & (np.abs(w) < 65520 - 1e-4 * mass)
    assert np.isfinite(c["dy16"]).all() and float(np.abs(c["dy16"].astype(F32)).min()) >= 3e4
    assert (over & (w > 0)).sum() >= 20 and (over & (w < 0)).sum() >= 20 and under.sum() >= 20
    assert (big & ~over & ~under).sum() <= 0.01 * big.sum()


def test_nonfinite_gradient_case_has_no_zero_tap_weight(oracle):
    c = nonfinite_case(oracle)
    assert len(c["bins"]) >= 6
    for (b, r, ch, p, q), lv in zip(c["bins"], c["bin_levels"]):
        H, W = c["ref"]["shapes"][lv][2:]
        ax, ay = c["ref"]["fw"][1][b, r, ch, p, q], c["ref"]["fw"][2][b, r, ch, p, q]
        assert 0 < ax < W - 1 and 0 < ay < H - 1 and ax != np.floor(ax) and ay != np.floor(ay)
        al, be = F32(ay - np.floor(ay)), F32(ax - np.floor(ax))
        for wgt in ((1 - al) * (1 - be), (1 - al) * be, al * (1 - be), al * be):
            assert wgt > 0
    cls = _classes(np.concatenate([w.ravel() for w in c["want"]]))
    assert (cls == 1).sum() >= 4 and (cls == 2).sum() >= 4 and (cls == 3).sum() >= 4


# ------------------------------------------------------------------------------------------------------ GPU --
def _t(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).cuda()    # (a copy: the shared references are read-only)


def _dispatch():
    from simpledet_amd._lib import lib
    return (lib().cdll.sd_last_dispatch() or b"").decode()


def _half(t):
    return t.cpu().numpy()


def _check_forward(ops, oracle, name, kind):
    import torch
    from simpledet_amd._lib import lib
    ref = reference(oracle, name, kind)
    g = ref["geom"]
    pooled = (g.pooled, g.pooled)
    tf16, tr = [_t(f) for f in ref["feats16"]], _t(ref["rois"])
    out, (am, coords) = ops.fpn_roi_align_forward_packed_f16(tf16, tr, STRIDES, pooled)
    ran = _dispatch()
    assert "roi_align_fwd_band<%d,true,true>" % g.pooled in ran, ran
    assert out.dtype == torch.float16
    E.assert_same_half_bits(_half(out), ref["out16"], "%s %s: fp16 forward against the oracle" % (name, kind))
    codes = ops.argmax_codes(am, pooled)
    assert np.array_equal(codes.cpu().numpy() == 255, ref["fw"][1] == -1), "255 <-> maxidx_x == -1"
    # the same state as the fp32 entry on the converted maps
    o32, (am32, c32) = ops.fpn_roi_align_forward_packed([_t(f.astype(F32)) for f in ref["feats16"]], tr, STRIDES, pooled)
    assert torch.equal(codes, ops.argmax_codes(am32, pooled))
    lvl = ops.fpn_roi_assign(tr, STRIDES)[1].reshape(-1) >= 0
    assert torch.equal(coords.reshape(lvl.numel(), -1)[lvl].view(torch.int32), c32.reshape(lvl.numel(), -1)[lvl].view(torch.int32))
    with np.errstate(all="ignore"):
        E.assert_same_half_bits(_half(out), o32.cpu().numpy().astype(F16), "fp16 entry against the fp32 entry")
    # where the band-resident kernel is switched off: cast -> fp32 op -> cast, the same bits (both casts at odd n)
    with lib().tuned(roi_align_fwd_band=0):
        out_fb, (am_fb, _) = ops.fpn_roi_align_forward_packed_f16(tf16, tr, STRIDES, pooled)
        ran_fb = _dispatch()
    assert "true,true" not in ran_fb, ran_fb
    E.assert_same_half_bits(_half(out_fb), ref["out16"], "%s %s: cast fallback against the oracle" % (name, kind))
    E.assert_same_half_bits(_half(out_fb), _half(out), "cast fallback against the fp16 kernel")
    assert torch.equal(ops.argmax_codes(am_fb, pooled), codes)


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_forward_fp16_geometries(ops, oracle, name):
    _check_forward(ops, oracle, name, "normal")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["subnormal", "max", "zeros", "nonfinite"])
@pytest.mark.parametrize("name", VALUE_GEOMS)
def test_forward_fp16_value_edges(ops, oracle, name, kind):
    """subnormal halves in and out, +-65504, zeros of either sign, and +inf / -inf / NaN pixels: the last held to the
    same comparison (equal NaN mask, equal bits elsewhere)"""
    _check_forward(ops, oracle, name, kind)


# ---- backward ----
def _state(ops, ref):
    g = ref["geom"]
    return ops.fpn_roi_align_forward_packed_f16([_t(f) for f in ref["feats16"]], _t(ref["rois"]), STRIDES,
                                                (g.pooled, g.pooled))[1]


def _oracle_bwd(oracle, ref, d32, acc16=None):
    fw = ref["fw"]
    with np.errstate(all="ignore"):
        if acc16 is None:
            return oracle.fpn_roi_align_bwd(d32, ref["rois"], fw[1], fw[2], ref["shapes"], STRIDES, nthreads=8)
        return oracle.fpn_roi_align_bwd(d32, ref["rois"], fw[1], fw[2], ref["shapes"], STRIDES, req=3,
                                        dfeats=[np.ascontiguousarray(a.astype(F32)) for a in acc16], nthreads=8)


def _run_bwd(ops, ref, am, dy16, req, acc16, native=True):
    d = None if req == "write" else [_t(a) for a in acc16]
    res = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(ref["rois"]), am, ref["shapes"], STRIDES, req_data=req,
                                                d_feats=d, native=native)
    ran = _dispatch()
    if native:
        assert "roi_align_bwd_packed4<" in ran and ",true>" in ran, ran
    else:
        assert ",true>" not in ran, ran
    return [_half(x) for x in res]


def _accumulator(ref, scale, seed):
    rs = np.random.RandomState(seed)
    return [(rs.standard_normal(tuple(s)) * scale).astype(F16) for s in ref["shapes"]]


def _cat(arrs):
    return np.concatenate([np.asarray(a).ravel() for a in arrs])


def _normal_bar(got16, want32):
    """test_fpn_packed_backward_fp16_io's: 1e-4 + one fp16 step of the reference"""
    with np.errstate(all="ignore"):
        w16 = want32.astype(F16).astype(np.float64)
    err = np.abs(got16.astype(np.float64) - w16) - (1e-4 + E.half_step(w16))
    return float(err.max())


@pytest.mark.gpu
@pytest.mark.parametrize("req", ["write", "add"])
@pytest.mark.parametrize("name", NAMES)
def test_backward_fp16_geometries(ops, oracle, name, req):
    ref = reference(oracle, name)
    g = ref["geom"]
    am = _state(ops, ref)
    dy16 = np.random.RandomState(31).standard_normal((g.B, g.R, g.C, g.pooled, g.pooled)).astype(F16)
    acc16 = None if req == "write" else _accumulator(ref, 0.5, 32)
    want = _oracle_bwd(oracle, ref, dy16.astype(F32), acc16)
    got = _run_bwd(ops, ref, am, dy16, req, acc16)
    over = _normal_bar(_cat(got), _cat(want))
    print("%s %s: excess over 1e-4 + one fp16 step %.3g" % (name, req, over))
    assert over <= 0
    again = _run_bwd(ops, ref, am, dy16, req, acc16)
    casts = _run_bwd(ops, ref, am, dy16, req, acc16, native=False)
    for l, (a, b, c) in enumerate(zip(got, again, casts)):
        assert np.array_equal(E.bits16(a), E.bits16(b)), "level %d: two calls differ" % l
        assert np.array_equal(E.bits16(a), E.bits16(c)), "level %d: native against the casts around the fp32 kernel" % l


@pytest.mark.gpu
@pytest.mark.parametrize("req", ["write", "add"])
@pytest.mark.parametrize("name", VALUE_GEOMS)
def test_backward_fp16_subnormal_gradients(ops, oracle, name, req):
    """N(0,1) 2^-20 gradients: subnormal halves in, mostly subnormal halves out (a kernel that flushed them would be
    far outside the 2^-24 step floor)"""
    ref = reference(oracle, name)
    g = ref["geom"]
    am = _state(ops, ref)
    dy16 = (np.random.RandomState(33).standard_normal((g.B, g.R, g.C, g.pooled, g.pooled)) * 2.0 ** -20).astype(F16)
    d32 = dy16.astype(F32)
    assert (np.abs(d32[d32 != 0]) < 2.0 ** -14).mean() > 0.99
    acc16 = None if req == "write" else _accumulator(ref, 2.0 ** -19, 34)
    want = _cat(_oracle_bwd(oracle, ref, d32, acc16))
    mass = _cat(_oracle_bwd(oracle, ref, np.abs(d32)))
    assert ((np.abs(want) < 2.0 ** -14) & (want != 0)).mean() > 0.3
    res = {}
    for native in (True, False):
        got = res[native] = _cat(_run_bwd(ops, ref, am, dy16, req, acc16, native))
        bar = E.mass_bar(got, want, mass, d32)
        print("%s %s native=%s: mass bar %.3g" % (name, req, native, bar))
        assert bar <= 1e-4, bar
        assert ((np.abs(got.astype(F32)) < 2.0 ** -14) & (got != 0)).mean() > 0.3
    # gradients of one magnitude: fixed-point sums on both sides, one rounding each
    assert np.array_equal(E.bits16(res[True]), E.bits16(res[False])), "native against the casts around the fp32 kernel"


def overflow_case(oracle):
    """a pile of identical boxes on the 196 x 388 pyramid with gradients of +-(3..6) 10^4, one sign per channel: the
    fp32 sums run from 0 to far beyond 65504"""
    if "overflow" not in _CACHE:
        ref = reference(oracle, "a_c8_r7")
        g = ref["geom"]
        rois = np.tile(np.array([83.3, 41.7, 158.8, 111.9], F32), (g.B, g.R, 1))
        rois[:, 3:] = 0          # three copies and padding rows
        feats32 = [f.astype(F32) for f in ref["feats16"]]
        fw = oracle.fpn_roi_align_fwd(feats32, rois, STRIDES, (7, 7), nthreads=8)
        rs = np.random.RandomState(35)
        mag = rs.uniform(3e4, 6e4, fw[0].shape)
        sign = np.where(np.arange(g.C) % 2 == 0, 1.0, -1.0)[None, None, :, None, None]
        dy16 = (mag * sign).astype(F16)
        c = dict(geom=g, feats16=ref["feats16"], rois=rois, fw=fw, shapes=ref["shapes"], dy16=dy16)
        c["want"] = _cat(_oracle_bwd(oracle, c, dy16.astype(F32)))
        c["mass"] = _cat(_oracle_bwd(oracle, c, np.abs(dy16.astype(F32))))
        _CACHE["overflow"] = c
    return _CACHE["overflow"]


@pytest.mark.gpu
def test_backward_fp16_overflow_on_the_final_rounding(ops, oracle):
    """finite fp16 gradients whose fp32 sums pass 65504: inf of the sum's sign where the oracle's sum is beyond 65520
    (the rounding boundary) by more than the bar, finite and within the bar where it is below by more than the bar;
    by the kernel's fp16 instance and by the casts around the fp32 kernel"""
    c = overflow_case(oracle)
    am = _state(ops, c)
    w, mass = c["want"], c["mass"]
    over = np.abs(w) > 65520 + 1e-4 * mass
    under = np.abs(w) < 65520 - 1e-4 * mass
    for native in (True, False):
        got = _cat(_run_bwd(ops, c, am, c["dy16"], "write", None, native))
        assert np.array_equal(got[over].astype(F32), np.where(w[over] > 0, np.inf, -np.inf).astype(F32)), native
        assert np.isfinite(got[under]).all(), native
        bar = E.mass_bar(got[under], w[under], mass[under], c["dy16"].astype(F32))
        print("overflow native=%s: %d inf, mass bar of the finite ones %.3g" % (native, int(over.sum()), bar))
        assert bar <= 1e-4, (native, bar)


def _classes(a):
    """0 finite, 1 +inf, 2 -inf, 3 NaN"""
    a = np.asarray(a, F32)
    return np.where(np.isnan(a), 3, np.where(a == np.inf, 1, np.where(a == -np.inf, 2, 0)))


def nonfinite_case(oracle):
    """N(0,1) gradients with +inf, -inf and NaN in bins of RoIs that lie strictly inside their map and whose sample
    coordinates are not integers (no tap weight is zero: 0 * inf stays out of the picture)"""
    if "nonfinite" not in _CACHE:
        ref = reference(oracle, "b_c12_r77")
        g = ref["geom"]
        ax, ay = ref["fw"][1], ref["fw"][2]
        _, lvl = oracle.fpn_roi_assign(ref["rois"], STRIDES)
        dy16 = np.random.RandomState(36).standard_normal(ax.shape).astype(F16)
        bins, bin_levels = [], []
        vals = [np.inf, -np.inf, np.nan]
        for b in range(g.B):
            for r in range(g.R):
                lv = int(lvl[b, r])
                if lv < 0 or len(bins) >= 12:
                    continue
                H, W = ref["shapes"][lv][2:]
                x, y = ax[b, r], ay[b, r]
                inside = (x > 0) & (x < W - 1) & (y > 0) & (y < H - 1) & (x != np.floor(x)) & (y != np.floor(y))
                x1, y1, x2, y2 = ref["rois"][b, r] / STRIDES[lv]
                if inside.all() and x1 > 1 and y1 > 1 and x2 < W - 2 and y2 < H - 2:
                    k = len(bins)
                    pos = (b, r, k % g.C, (2 * k) % g.pooled, (3 * k + 1) % g.pooled)
                    dy16[pos] = vals[k % 3]
                    bins.append(pos)
                    bin_levels.append(lv)
        c = dict(ref=ref, dy16=dy16, bins=bins, bin_levels=bin_levels)
        c["want"] = _oracle_bwd(oracle, ref, dy16.astype(F32))
        _CACHE["nonfinite"] = c
    return _CACHE["nonfinite"]


@pytest.mark.gpu
def test_backward_fp16_nonfinite_gradients_reach_their_pixels(ops, oracle):
    """what a loss-scale overflow sends: every pixel the oracle makes +inf, -inf or NaN is of the same class on the
    device (native and native=False), every other pixel -- the rest of the bands that escaped to float adds included
    -- stays within the bar.  (No equal bits between runs are asked of the escaped bands.)"""
    c = nonfinite_case(oracle)
    ref = c["ref"]
    am = _state(ops, ref)
    want = _cat(c["want"])
    cw = _classes(want)
    fin = cw == 0
    for native in (True, False):
        got = _cat(_run_bwd(ops, ref, am, c["dy16"], "write", None, native))
        cg = _classes(got)
        assert np.array_equal(cw, cg), "native=%s: classes differ at %d pixels" % (native, int((cw != cg).sum()))
        over = _normal_bar(got[fin], want[fin])
        print("nonfinite native=%s: %d non-finite pixels, excess over the bar %.3g" % (native, int((~fin).sum()), over))
        assert over <= 0, native


# ---- the casts, called directly ----
NUM_CU = 256                               # kNumCU (csrc/common.h): both casts launch 8 kNumCU workgroups of 256
SWEEP = 8 * 256 * 8 * NUM_CU               # halves one grid-stride sweep of the half-to-float kernel converts


class Guarded:
    """a device tensor of n elements with four sentinels on either side (the pattern of tests/test_sigmoid_ce.py)"""
    SENT = -777.5     # (a half, too)

    def __init__(self, n, dtype, src=None):
        import torch
        self.n = n
        self.buf = torch.full((n + 8,), self.SENT, dtype=dtype, device="cuda")
        self.t = self.buf[4:4 + n]
        if src is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(src)))

    def check(self, what):
        g = self.buf.cpu().numpy()
        assert np.all(g[:4] == self.SENT) and np.all(g[4 + self.n:] == self.SENT), what + ": sentinel overwritten"
        return g[4:4 + self.n]


def _assert_same_float_bits(got, want, what):
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), what + ": NaN masks differ"
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~wn
    assert not bad.any(), "%s: %d floats differ, first at %d" % (what, int(bad.sum()), int(np.argmax(bad)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 8, 9, 15, 16391, 65536 + 3, SWEEP + 5])
def test_cast_f16_to_f32_every_pattern_and_every_tail(ops, n):
    """all 65,536 half bit patterns (from n = 65539 on), subnormals, infinities and NaNs included; n below one vector,
    one vector and a tail, and one full grid-stride sweep + a second trip + a tail"""
    import torch
    src = ((np.arange(n, dtype=np.int64) * 65521 + 0x03ff) % 65536).astype(np.uint16).view(F16)
    if n >= 65536:
        assert np.unique(E.bits16(src)).size == 65536
    dst = Guarded(n, torch.float32)
    assert dst.t.data_ptr() % 16 == 0
    ops.cast_f16_to_f32(_t(src), dst.t)
    _assert_same_float_bits(dst.check("cast_f16_to_f32 n=%d" % n), src.astype(F32), "cast_f16_to_f32 n=%d" % n)


def rne_probe_floats():
    """for every finite half h >= 0 the float midpoint to its successor (65536 after 65504) and that midpoint's two
    float neighbours, both signs: exhaustive for round-to-nearest-even; then the named values.  An odd count."""
    h = np.arange(0x0000, 0x7c00, dtype=np.uint16).view(F16).astype(np.float64)
    mid64 = (h + np.concatenate([h[1:], [65536.0]])) / 2
    mid = mid64.astype(F32)
    assert np.array_equal(mid.astype(np.float64), mid64)
    pos = np.concatenate([mid, np.nextafter(mid, F32(-np.inf)), np.nextafter(mid, F32(np.inf))])
    named = np.array([65504, 65519.99, 65520, 2.0 ** -24, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -23), 0.0, -0.0, np.inf,
                      -np.inf, np.nan], np.float64).astype(F32)
    x = np.concatenate([pos, -pos, named, -named[:6]])
    return x if x.size % 2 else np.concatenate([x, F32([1.0])])


@pytest.mark.gpu
def test_cast_f32_to_f16_rounds_to_nearest_even_everywhere(ops):
    import torch
    x = rne_probe_floats()
    assert x.size % 2 == 1 and x.size > 6 * 0x7c00
    with np.errstate(all="ignore"):
        want = x.astype(F16)
    assert np.isinf(want[x == F32(65520)]).all() and want[x == F32(65519.99)][0] == F16(65504)
    assert want[x == F32(2.0 ** -25)][0] == 0 and want[x == F32(2.0 ** -25 * (1 + 2.0 ** -23))][0] == F16(2.0 ** -24)
    dst = Guarded(x.size, torch.float16)
    ops.cast_f32_to_f16(_t(x), dst.t)
    E.assert_same_half_bits(dst.check("cast_f32_to_f16"), want, "cast_f32_to_f16 write")


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 9, 600001])
def test_cast_f32_to_f16_add_rounds_the_fp32_sum_once(ops, n):
    """req = add: (h.astype(f32) + x).astype(f16), at odd n, one of them beyond one grid-stride sweep of 524,288"""
    import torch
    rs = np.random.RandomState(37)
    h = rs.randint(0, 65536, n).astype(np.uint16).view(F16)            # any pattern: subnormals, -0, inf, NaN
    x = (rs.standard_normal(n) * np.exp2(rs.randint(-26, 17, n))).astype(F32)
    x[::7] = 0.0
    x[3::11] = -h[3::11].astype(F32)                                   # exact cancellation: +0
    with np.errstate(all="ignore"):
        want = (h.astype(F32) + x).astype(F16)
    dst = Guarded(n, torch.float16, h)
    ops.cast_f32_to_f16(_t(x), dst.t, req="add")
    E.assert_same_half_bits(dst.check("cast_f32_to_f16 add"), want, "cast_f32_to_f16 add n=%d" % n)


@pytest.mark.gpu
def test_cast_f16_to_f32_refuses_a_pointer_off_its_16_bytes(ops):
    import torch
    from simpledet_amd._lib import SimpleDetOpsError
    buf = torch.zeros(24, dtype=torch.float16, device="cuda")
    dst = torch.full((16,), 5.0, dtype=torch.float32, device="cuda")
    with pytest.raises(SimpleDetOpsError, match="16-byte aligned"):
        ops.cast_f16_to_f32(buf[1:17], dst)            # a view 2 bytes in: refused before any launch
    assert bool((dst == 5.0).all())
