"""The reordered workgroup of the fused backward (roi_align_bwd_packed4): raw items, early tables, the block decode
without divisions.

What a workgroup does between entry and exit was reordered and trimmed, nothing it computes was changed:
  - an item's loads are issued by every lane alike and stay untouched until the item is scattered; the last lane
    of a 7x7 RoI reads the gradients of bins 45..48 and lands only bin 48;
  - the first chunk's tap tables and items leave right behind the unit's header (the items take their RoI from
    the list in global memory), later chunks' tables with one wait;
  - the block -> (level, image, band, channel) decode multiplies by reciprocals and reads one record per level.
Both kinds of add (fixed point, float compare-and-swap) and the second attempt run through the same reordered loops.
Every case runs the packed forward with its plan, the backward, compares against the CPU oracle at the
project's elementwise 1e-4 and asks two launches for the same bits.  The shapes are the smallest at which each
piece can go wrong: one image-sized band of 24x40 .. 48x64 pixels, 8 channels unless the case is about channels.
"""
import numpy as np
import pytest

STRIDES = [4, 8, 16, 32]
f32 = np.float32


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shapes(B, C, img_h, img_w, strides=STRIDES):
    return [(B, C, img_h // s, img_w // s) for s in strides]


def p2_rois(rs, B, n, img_h, img_w, lo=20.0, hi=80.0):
    """B x n RoIs with sqrt(wh) in lo..hi px (< 112: FPN level P2), inside the image"""
    s = rs.uniform(lo, hi, (B, n))
    ar = rs.uniform(0.8, 1.25, (B, n))
    w, h = s * np.sqrt(ar), s / np.sqrt(ar)
    x1, y1 = rs.uniform(0, img_w - 1 - w), rs.uniform(0, img_h - 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 2).astype(f32)


def all_level_rois(rs, B, n, img_h, img_w):
    """square RoIs of the four FPN levels in turn (sqrt(wh) in 40..100, 120..200, 230..400, 450..500 px: the level
    rule changes at 112, 224 and 448); the image is at least 512 px either way"""
    lo = np.array([40.0, 120.0, 230.0, 450.0])[np.arange(n) % 4]
    hi = np.array([100.0, 200.0, 400.0, 500.0])[np.arange(n) % 4]
    s = rs.uniform(lo, hi, (B, n))
    x1, y1 = rs.uniform(0, img_w - 1 - s), rs.uniform(0, img_h - 1 - s)
    return np.stack([x1, y1, x1 + s, y1 + s], 2).astype(f32)


_ORACLE = {}


def reference(oracle, key, feats, rois, dy, pooled, strides=STRIDES):
    """the oracle's forward and backward, once per case"""
    if key not in _ORACLE:
        P = (pooled, pooled)
        fw = oracle.fpn_roi_align_fwd(feats, rois, strides, P, nthreads=8)
        want = oracle.fpn_roi_align_bwd(dy, rois, fw[1], fw[2], [f.shape for f in feats], strides, nthreads=8)
        _ORACLE[key] = (fw, want)
    return _ORACLE[key]


def compare(got, want, what):
    """elementwise 1e-4 where the oracle is finite, the same non-finite values elsewhere"""
    for l, (g, w) in enumerate(zip(got, want)):
        g = g.float().cpu().numpy() if hasattr(g, "cpu") else g
        fin = np.isfinite(w)
        np.testing.assert_array_equal(np.isfinite(g), fin, err_msg="%s level %d" % (what, l))
        if not fin.all():
            np.testing.assert_array_equal(g[~fin], w[~fin], err_msg="%s level %d" % (what, l))
        err = float(np.abs(g[fin] - w[fin]).max()) if fin.any() else 0.0
        print("%s level %d: max |got - oracle| = %.3g" % (what, l, err))
        assert err <= 1e-4, (what, l, err)


def run_planned(ops, oracle, key, feats, rois, dy, pooled, kernel=None, strides=STRIDES):
    """forward with its plan, backward twice: oracle and bit equality; -> the gradients"""
    import torch
    from simpledet_amd._lib import lib
    P = (pooled, pooled)
    fw, want = reference(oracle, key, feats, rois, dy, pooled, strides)
    tf, tr, tdy = [_t(f) for f in feats], _t(rois), _t(dy)
    out, state = ops.fpn_roi_align_forward_packed(tf, tr, strides, P, plan=True)
    assert np.array_equal(out.cpu().numpy(), fw[0])
    g1 = ops.fpn_roi_align_backward_packed(tdy, tr, state, [f.shape for f in feats], strides)
    name = (lib().cdll.sd_last_dispatch() or b"").decode()
    if kernel is None:
        kernel = "roi_align_bwd_packed4<%d,%d,512,%d,1>" % (pooled, pooled, 48 if pooled == 7 else 24)
    assert kernel in name, name
    g2 = ops.fpn_roi_align_backward_packed(tdy, tr, state, [f.shape for f in feats], strides)
    compare(g1, want, str(key))
    # (bit patterns: a NaN equals itself)
    assert all(bool(torch.equal(a.view(torch.int32), b.view(torch.int32))) for a, b in zip(g1, g2)), \
        "two launches differ: %s" % (key,)
    return g1


def one_band_case(pooled, n, img, seed, C=8, B=1):
    img_h, img_w = img
    rs = np.random.RandomState(seed)
    rois = p2_rois(rs, B, n, img_h, img_w)
    feats = [rs.standard_normal(s).astype(f32) for s in _shapes(B, C, img_h, img_w)]
    dy = rs.standard_normal((B, n, C, pooled, pooled)).astype(f32)
    return feats, rois, dy


# ------------------------------------------------------------------------------- item and chunk counts
# one band per level (P2 is 24x40 / 48x64 pixels), every RoI on P2: the P3..P5 units are empty bands; 39 RoIs are
# 507 lane items (one trip, not full), 40 are 520 (a second trip of 8 lanes), 47 / 48 / 49 and 97 the edges of the
# chunks of 48, 1 and 3 a band far below one chunk
@pytest.mark.gpu
@pytest.mark.parametrize("n,img", [(1, (96, 160)), (3, (96, 160)), (39, (96, 160)), (40, (128, 192)),
                                   (47, (128, 192)), (48, (192, 256)), (49, (192, 256)), (97, (192, 256))])
def test_item_and_chunk_counts_7x7(ops, oracle, n, img):
    feats, rois, dy = one_band_case(7, n, img, 700 + n)
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert (level == 0).all()
    run_planned(ops, oracle, ("count7", n), feats, rois, dy, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("n,img", [(1, (96, 160)), (24, (128, 192)), (25, (192, 256)), (49, (192, 256))])
def test_item_and_chunk_counts_14x14(ops, oracle, n, img):
    feats, rois, dy = one_band_case(14, n, img, 1400 + n)
    run_planned(ops, oracle, ("count14", n), feats, rois, dy, 14)


# ------------------------------------------------------------------------------- the tail lane
@pytest.mark.gpu
@pytest.mark.parametrize("bin_", [0, 44, 45, 46, 47, 48])
def test_tail_lane_lands_bin_48_only(ops, oracle, bin_):
    """dY is non-zero in ONE bin of every (RoI, channel).  The 13th lane of a 7x7 RoI holds the gradients of bins
    45..48 and owns bin 48: a gradient in 45, 46 or 47 must arrive once (through the 12th lane), one in 48 once
    (through the 13th), and nothing else anywhere."""
    n, img = 50, (128, 192)
    feats, rois, dy = one_band_case(7, n, img, 4800)
    keep = np.zeros((7, 7), bool)
    keep[bin_ // 7, bin_ % 7] = True
    dy = np.where(keep[None, None, None], dy, f32(0)).astype(f32)
    got = run_planned(ops, oracle, ("tail", bin_), feats, rois, dy, 7)
    assert float(got[0].abs().max()) > 0.0


# ------------------------------------------------------------------------------- the block decode
@pytest.mark.gpu
@pytest.mark.parametrize("C", [3, 8, 12, 24])
@pytest.mark.parametrize("B", [1, 3])
def test_block_decode_channels_images_levels_bands(ops, oracle, C, B):
    """512 x 640: P2 is 128 x 160 pixels = three bands, P3 one of 20 KB, P4 and P5 small; RoIs on every level.
    C = 3 and 12 take the block mapping without whole XCDs (divide by C), 8 and 24 the one with (divide by
    C / 8 = 1 and 3: a power of two and not)."""
    rs = np.random.RandomState(100 * C + B)
    rois = all_level_rois(rs, B, 60, 512, 640)
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert len(np.unique(level)) == 4
    feats = [rs.standard_normal(s).astype(f32) for s in _shapes(B, C, 512, 640)]
    dy = rs.standard_normal((B, 60, C, 7, 7)).astype(f32)
    run_planned(ops, oracle, ("decode", C, B), feats, rois, dy, 7)


@pytest.mark.gpu
def test_block_decode_one_level(ops, oracle):
    """a single level (stride 4) cut into three bands of a 96 x 128 map"""
    rs = np.random.RandomState(41)
    rois = p2_rois(rs, 2, 30, 384, 512, 20.0, 100.0)
    feats = [rs.standard_normal((2, 8, 96, 128)).astype(f32)]
    dy = rs.standard_normal((2, 30, 8, 7, 7)).astype(f32)
    run_planned(ops, oracle, ("one_level",), feats, rois, dy, 7, strides=[4])


@pytest.mark.gpu
def test_block_decode_a_level_without_rois(ops, oracle):
    """RoIs on P2, P4 and P5 only: the units of P3, in the middle of the launch order, are empty"""
    rs = np.random.RandomState(43)
    rois = all_level_rois(rs, 2, 80, 512, 640)
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    rois = np.stack([rois[b][level[b] != 1][:40] for b in range(2)])
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert set(np.unique(level)) == {0, 2, 3}
    feats = [rs.standard_normal(s).astype(f32) for s in _shapes(2, 8, 512, 640)]
    dy = rs.standard_normal((2, 40, 8, 7, 7)).astype(f32)
    run_planned(ops, oracle, ("no_p3",), feats, rois, dy, 7)


# ------------------------------------------------------------------------------- other instantiations and paths
@pytest.mark.gpu
@pytest.mark.parametrize("lists,mode", [(0, 0), (2, 0)])
def test_coordinate_table_mode(ops, oracle, lists, mode):
    """MODE 0: without the workspace lists (each workgroup builds its own) and with lists but no tap tables"""
    import torch
    from simpledet_amd._lib import lib
    feats, rois, dy = one_band_case(7, 49, (192, 256), 749)
    fw, want = reference(oracle, ("count7", 49), feats, rois, dy, 7)
    tf, tr, tdy = [_t(f) for f in feats], _t(rois), _t(dy)
    _, state = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, (7, 7))
    with lib().tuned(roi_align_bwd_lists=lists):
        g1 = ops.fpn_roi_align_backward_packed(tdy, tr, state, [f.shape for f in feats], STRIDES)
        name = (lib().cdll.sd_last_dispatch() or b"").decode()
        g2 = ops.fpn_roi_align_backward_packed(tdy, tr, state, [f.shape for f in feats], STRIDES)
    assert "roi_align_bwd_packed4<7,7,512,32,%d>" % mode in name, name
    compare(g1, want, "lists=%d" % lists)
    assert all(bool(torch.equal(a, b)) for a, b in zip(g1, g2))


@pytest.mark.gpu
def test_float_argmax_form(ops, oracle):
    """MODE 2: the reference's float arg-max planes, four levels so that the band kernel takes it"""
    import torch
    from simpledet_amd._lib import lib
    feats, rois, dy = one_band_case(7, 49, (192, 256), 749)
    fw, want = reference(oracle, ("count7", 49), feats, rois, dy, 7)
    tf, tr, tdy = [_t(f) for f in feats], _t(rois), _t(dy)
    out, mx, my = ops.fpn_roi_align_forward(tf, tr, STRIDES, (7, 7))
    shapes = [f.shape for f in feats]
    g1 = ops.fpn_roi_align_backward(tdy, tr, mx, my, shapes, STRIDES)
    name = (lib().cdll.sd_last_dispatch() or b"").decode()
    assert "roi_align_bwd_packed4<7,7,512,32,2>" in name, name
    g2 = ops.fpn_roi_align_backward(tdy, tr, mx, my, shapes, STRIDES)
    compare(g1, want, "float arg-max")
    assert all(bool(torch.equal(a, b)) for a, b in zip(g1, g2))


@pytest.mark.gpu
def test_req_add(ops, oracle):
    """req = add: the gradients are added to what the maps hold"""
    import torch
    feats, rois, dy = one_band_case(7, 49, (192, 256), 749)
    fw, want = reference(oracle, ("count7", 49), feats, rois, dy, 7)
    tf, tr, tdy = [_t(f) for f in feats], _t(rois), _t(dy)
    _, state = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, (7, 7), plan=True)
    base = [np.random.RandomState(5 + l).standard_normal(f.shape).astype(f32) for l, f in enumerate(feats)]
    runs = []
    for _ in range(2):
        d = [_t(b) for b in base]
        ops.fpn_roi_align_backward_packed(tdy, tr, state, [f.shape for f in feats], STRIDES, req_data="add", d_feats=d)
        runs.append(d)
    compare(runs[0], [b + w for b, w in zip(base, want)], "req=add")
    assert all(bool(torch.equal(a, b)) for a, b in zip(*runs))


@pytest.mark.gpu
def test_fp16_io(ops, oracle):
    """fp16 gradients in and out (the four halves of an item stay packed until it is scattered), 7x7 with its tail
    lane, 49 RoIs: against the oracle on the fp16-rounded inputs, within 1e-4 plus one fp16 step of the result"""
    import torch
    from simpledet_amd._lib import lib
    feats, rois, dy = one_band_case(7, 49, (192, 256), 749)
    feats16 = [f.astype(np.float16) for f in feats]
    dy16 = (dy * f32(2.0 ** -4)).astype(np.float16)
    shapes = [f.shape for f in feats]
    fw, want = reference(oracle, ("fp16",), [f.astype(f32) for f in feats16], rois, dy16.astype(f32), 7)
    _, am = ops.fpn_roi_align_forward_packed_f16([_t(f) for f in feats16], _t(rois), STRIDES, (7, 7))
    g1 = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(rois), am, shapes, STRIDES)
    assert "roi_align_bwd_packed4<7,7,512,48,1,true>" in (lib().cdll.sd_last_dispatch() or b"").decode()
    g2 = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(rois), am, shapes, STRIDES)
    for l, (g, w) in enumerate(zip(g1, want)):
        g = g.cpu().numpy().astype(np.float64)
        step = np.maximum(np.abs(w) * 2.0 ** -10, 2.0 ** -24)   # the result is rounded to fp16 once
        excess = float(np.maximum(np.abs(g - w) - step, 0.0).max())
        print("fp16 level %d: excess over one fp16 step %.3g" % (l, excess))
        assert excess <= 1e-4, (l, excess)
    assert all(bool(torch.equal(a, b)) for a, b in zip(g1, g2))


# ------------------------------------------------------------------------------- both kinds of add, second attempt
@pytest.mark.gpu
@pytest.mark.parametrize("value", [np.inf, np.nan])
def test_non_finite_gradient_takes_the_float_adds(ops, oracle, value):
    """One inf / NaN in dY: the workgroups that stream it sum with the float adds, and it reaches exactly the
    pixels the oracle sends it to.  It sits in the ONLY RoI of its level (P4), so those workgroups are 13 lanes of
    one wave and the order of their float adds is the wave's own: two launches give the same bits there too."""
    rs = np.random.RandomState(77)
    rois = p2_rois(rs, 1, 50, 256, 320, 40.0, 100.0)
    rois[0, 20] = [30.0, 20.0, 290.0, 240.0]   # sqrt(wh) = 239: P4
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert (level == 2).sum() == 1 and level[0, 20] == 2
    feats = [rs.standard_normal(s).astype(f32) for s in _shapes(1, 8, 256, 320)]
    dy = rs.standard_normal((1, 50, 8, 7, 7)).astype(f32)
    fw = oracle.fpn_roi_align_fwd(feats, rois, STRIDES, (7, 7), nthreads=8)
    assert fw[1][0, 20, 3, 6, 6] != -1
    dy[0, 20, 3, 6, 6] = value     # bin 48: the tail lane
    dy[0, 20, 5, 2, 3] = value
    got = run_planned(ops, oracle, ("nonfinite", str(value)), feats, rois, dy, 7)
    assert not bool(got[2].isfinite().all())


@pytest.mark.gpu
def test_late_outlier_takes_the_second_attempt(ops, oracle):
    """a gradient of 24 in the third chunk, above twice the first chunk's maximum (|N(0,1)| of 512 x 4 values stays
    below 5): the band is summed again with the exact maximum, still in fixed point"""
    feats, rois, dy = one_band_case(7, 120, (192, 256), 2400)
    assert float(np.abs(dy).max()) < 6.0
    dy[0, 110, :, 3, 3] = 24.0
    run_planned(ops, oracle, ("late_outlier",), feats, rois, dy, 7)


# ------------------------------------------------------------------------------- the side table
def axis_samples(start, end, stride, size, pooled):
    """the reference's sample loop along one axis (float32, the two double expressions kept) -> per bin the list
    of sample coordinates"""
    scale = f32(1.0) / f32(stride)
    rs, re = f32(start) * scale, f32(end) * scale
    b = f32(re - rs) / f32(pooled)
    out = []
    for p in range(pooled):
        lo = min(max(f32(f32(f32(p) * b) + rs), f32(0)), f32(size - 1))
        hi = min(max(f32(f32(f32(p + 1) * b) + rs), f32(0)), f32(size - 1))
        v = []
        if not hi <= lo:
            st = f32(np.float64(f32(hi - lo)) / 3.0)
            lim = np.float64(f32(hi - st)) + 0.01
            step = max(st, f32(0.01))
            x = f32(lo + st)
            while np.float64(x) <= lim:
                v.append(x)
                x = f32(x + step)
        out.append(v)
    return out


@pytest.mark.gpu
def test_side_table_third_candidate(ops, oracle):
    """needle RoIs whose bins are 0.03 px wide along x: the sample stride rounds to 0.01 px, a bin gets a third
    sample, and on a ramp that one wins -- the codes name candidate 2, which the scatter fetches from the side
    table in global memory.  One needle in the first chunk (taken from the global list word), one in the second."""
    img_h, img_w = 192, 256
    rs = np.random.RandomState(303)
    rois = p2_rois(rs, 1, 60, img_h, img_w)
    W = img_w // 4
    for r in (7, 53):
        for _ in range(4000):
            a = f32(rs.uniform(8.0, img_w - 16.0))
            b = f32(a + f32(0.03 * 7 * 4 * (1.0 + rs.uniform(-3e-4, 3e-4))))
            if sum(len(v) == 3 for v in axis_samples(a, b, 4, W, 7)) >= 3:
                break
        else:
            raise AssertionError("no needle found")
        rois[0, r] = [a, 40.0, b, 130.0]
    feats = []
    for (_, C, H, Wl) in _shapes(1, 8, img_h, img_w):
        g = np.arange(Wl, dtype=f32)[None, :] + np.arange(H, dtype=f32)[:, None]
        feats.append((g[None, None] * (1.0 + 0.125 * np.arange(C, dtype=f32))[None, :, None, None]).astype(f32))
    dy = rs.standard_normal((1, 60, 8, 7, 7)).astype(f32)
    run_planned(ops, oracle, ("needles",), feats, rois, dy, 7)
    _, state = ops.fpn_roi_align_forward_packed([_t(f) for f in feats], _t(rois), STRIDES, (7, 7))
    codes = ops.argmax_codes(state[0], (7, 7))[0].cpu().numpy().astype(np.int64)
    for r in (7, 53):
        assert ((codes[r] % 3) == 2).any(), "RoI %d names no third column candidate" % r
