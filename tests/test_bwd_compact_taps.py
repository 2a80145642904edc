"""The tap-table backward (roi_align_bwd_packed4, MODE 1) with two candidate entries per bin in LDS and the third
in a side table.

The channel workgroups stage the tap entries of their band's RoIs into LDS a chunk at a time: 48 RoIs at 7x7,
24 at 14x14, candidates 0 and 1 of every axis bin.  Candidate 2 -- the reference's sample loop makes a third
sample only where the sample stride rounds to 0.01 px -- lives in a side table in global memory and is fetched by
the bin whose arg-max code names it.  Checked here, against the CPU oracle at the elementwise 1e-4 of
tests/test_roi_align.py and for bit-identical output over two launches:
  - chunk edges: one chunk, exactly full, one RoI over, two full, two full plus one, all RoIs on one band;
  - third candidates: needle boxes whose width (height) puts the stride on 0.01 px, on a ramp so that the last
    sample wins, in the first chunk, in a later chunk and across a band edge, mixed with ordinary RoIs;
  - fp16 gradients in and out, once.
Everything is small: one image of 256 x 320 (256 x 512 where P2 has to take two bands), 8 channels (3 once: the
block mapping without whole XCDs).
"""
import numpy as np
import pytest

STRIDES = [4, 8, 16, 32]
f32 = np.float32


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _cat(arrs):
    return np.concatenate([np.asarray(a).ravel() for a in arrs])


def _shapes(C, img_h, img_w):
    return [(1, C, img_h // s, img_w // s) for s in STRIDES]


# ------------------------------------------------------------------------------------------------ inputs
def p2_rois(rs, n, img_h, img_w):
    """n ordinary RoIs of FPN level P2 (sqrt(wh) in 58..106 px), spread uniformly over the image"""
    s = rs.uniform(58.0, 106.0, n)
    ar = rs.uniform(0.8, 1.25, n)
    w, h = s * np.sqrt(ar), s / np.sqrt(ar)
    x1, y1 = rs.uniform(0, img_w - 1 - w), rs.uniform(0, img_h - 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h], 1).astype(f32)


def axis_samples(start, end, stride, size, pooled):
    """the reference's sample loop along one axis (the forward of oracle/roi_align_v2.c; float32, the two double
    expressions kept) -> per bin the list of sample coordinates"""
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


def needle_span(rs, lo, hi, pooled, size):
    """(start, end) on the image, start in lo..hi, whose P2 bins are 0.03 px wide: the sample stride rounds to
    0.01 px and at least three bins get a third sample (a rounding event: searched, a few tries)"""
    for _ in range(4000):
        a = f32(rs.uniform(lo, hi))
        b = f32(a + f32(0.03 * pooled * STRIDES[0] * (1.0 + rs.uniform(-3e-4, 3e-4))))
        if sum(len(v) == 3 for v in axis_samples(a, b, STRIDES[0], size, pooled)) >= 3:
            return a, b
    raise AssertionError("no needle found")


def ramp_feats(C, img_h, img_w):
    """x + y, a different slope per channel: the last sample of a bin wins on either axis"""
    out = []
    for (_, _, H, W) in _shapes(C, img_h, img_w):
        g = (np.arange(W, dtype=f32)[None, :] + np.arange(H, dtype=f32)[:, None])
        out.append((g[None, None] * (1.0 + 0.125 * np.arange(C, dtype=f32))[None, :, None, None]).astype(f32))
    return out


# ------------------------------------------------------------------------------------------------ the check
def run_backward(ops, oracle, feats, rois, dy, pooled, kernel):
    """the packed backward through the workspace path and the planned path (MODE 1 both) against the oracle;
    -> the forward's arg-max codes (R, C, P, P)"""
    import torch
    from simpledet_amd._lib import lib
    P = (pooled, pooled)
    shapes = [f.shape for f in feats]
    fw = oracle.fpn_roi_align_fwd(feats, rois, STRIDES, P, nthreads=8)
    want = _cat(oracle.fpn_roi_align_bwd(dy, rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    tf, tr, tdy = [_t(f) for f in feats], _t(rois), _t(dy)
    codes = None
    for plan in (False, True):
        out, state = ops.fpn_roi_align_forward_packed(tf, tr, STRIDES, P, plan=plan)
        assert np.array_equal(out.cpu().numpy(), fw[0])
        g1 = ops.fpn_roi_align_backward_packed(tdy, tr, state, shapes, STRIDES)
        assert kernel in (lib().cdll.sd_last_dispatch() or b"").decode()
        g2 = ops.fpn_roi_align_backward_packed(tdy, tr, state, shapes, STRIDES)
        err = float(np.abs(_cat([g.cpu().numpy() for g in g1]) - want).max())
        print("plan=%d max |got - oracle| = %.3g" % (plan, err))
        assert err <= 1e-4, (plan, err)
        assert all(bool(torch.equal(a, b)) for a, b in zip(g1, g2)), "two launches differ (plan=%d)" % plan
        codes = ops.argmax_codes(state[0], P)[0].cpu().numpy()
    return codes, fw


def chunk_case(ops, oracle, pooled, n, C):
    rs = np.random.RandomState(1000 * pooled + 10 * n + C)
    rois = p2_rois(rs, n, 256, 320)[None]
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert (level == 0).all(), "a RoI left P2"
    feats = [rs.standard_normal(s).astype(f32) for s in _shapes(C, 256, 320)]
    dy = rs.standard_normal((1, n, C, pooled, pooled)).astype(f32)
    tch = 48 if pooled == 7 else 24
    run_backward(ops, oracle, feats, rois, dy, pooled, "roi_align_bwd_packed4<%d,%d,512,%d,1>" % (pooled, pooled, tch))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [47, 48, 49, 96, 97])
def test_chunk_edges_7x7(ops, oracle, n):
    chunk_case(ops, oracle, 7, n, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [23, 24, 25, 49])
def test_chunk_edges_14x14(ops, oracle, n):
    chunk_case(ops, oracle, 14, n, 8)


@pytest.mark.gpu
def test_chunk_edge_three_channels(ops, oracle):
    """C = 3: the block -> (unit, channel) mapping without whole XCDs"""
    chunk_case(ops, oracle, 7, 49, 3)


def needle_case(pooled, img_h, img_w, slots, n, seed, y_edge=None):
    """n P2 RoIs; slots = {RoI index: 'w' | 'h'}: a needle thin along x (third COLUMN samples) or along y (third
    ROW samples) in place of the ordinary RoI.  y_edge: the needles cross / sit on that image row (a band edge
    of P2).  -> rois (1, n, 4), {index: (axis, per-bin sample lists)}"""
    rs = np.random.RandomState(seed)
    rois = p2_rois(rs, n, img_h, img_w)
    H, W = img_h // STRIDES[0], img_w // STRIDES[0]
    info = {}
    for r, axis in sorted(slots.items()):
        if axis == "w":
            a, b = needle_span(rs, 8.0, img_w - 16.0, pooled, W)
            y1 = rs.uniform(8.0, img_h - 110.0) if y_edge is None else y_edge - 30.0
            rois[r] = [a, y1, b, y1 + 90.0]
            info[r] = ("w", axis_samples(a, b, STRIDES[0], W, pooled))
        else:
            lo, hi = (8.0, img_h - 16.0) if y_edge is None else (y_edge - 0.9, y_edge - 0.3)
            a, b = needle_span(rs, lo, hi, pooled, H)
            x1 = rs.uniform(8.0, img_w - 110.0)
            rois[r] = [x1, a, x1 + 90.0, b]
            info[r] = ("h", axis_samples(a, b, STRIDES[0], H, pooled))
    return rois[None], info


def check_needles(ops, oracle, pooled, img_h, img_w, slots, n, seed, y_edge=None):
    C = 8
    rois, info = needle_case(pooled, img_h, img_w, slots, n, seed, y_edge)
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert (level == 0).all(), "a RoI left P2"
    feats = ramp_feats(C, img_h, img_w)
    dy = np.random.RandomState(seed + 1).standard_normal((1, n, C, pooled, pooled)).astype(f32)
    tch = 48 if pooled == 7 else 24
    codes, fw = run_backward(ops, oracle, feats, rois, dy, pooled,
                             "roi_align_bwd_packed4<%d,%d,512,%d,1>" % (pooled, pooled, tch))
    for r, (axis, samples) in info.items():
        third = [q for q, v in enumerate(samples) if len(v) == 3]
        assert len(third) >= 3
        # the oracle's own arg-max is the third sample of those bins ...
        am = fw[1][0, r] if axis == "w" else fw[2][0, r]          # (C, P, P) float coordinates
        for q in third:
            got = am[:, :, q] if axis == "w" else am[:, q, :]
            assert (got == samples[q][2]).all(), (r, axis, q)
        # ... and the forward's packed code names candidate 2 there
        c = codes[r].astype(np.int64)
        k = c % 3 if axis == "w" else c // 3
        for q in third:
            kk = k[:, :, q] if axis == "w" else k[:, q, :]
            assert (kk == 2).all(), (r, axis, q)


@pytest.mark.gpu
def test_third_candidate_in_the_first_and_a_later_chunk_7x7(ops, oracle):
    """list slots 5 / 20 (first chunk of 48) and 50 / 60 (second), one band: slot = RoI index"""
    check_needles(ops, oracle, 7, 256, 320, {5: "w", 20: "h", 50: "w", 60: "h"}, 64, 7)


@pytest.mark.gpu
def test_third_candidate_in_the_first_and_a_later_chunk_14x14(ops, oracle):
    """chunks of 24 at 14x14: slots 3 / 11 and 30 / 37"""
    check_needles(ops, oracle, 14, 256, 320, {3: "w", 11: "h", 30: "w", 37: "h"}, 40, 14)


@pytest.mark.gpu
def test_third_candidate_across_a_band_edge(ops, oracle):
    """256 x 512: P2 is 64 x 128 = 32 KB, two bands of 32 rows; image row 128 is map row 32.  The column needle
    runs over rows 24..47 of the map, the row needle's samples lie between rows 31 and 32: both bands read the
    side table, each for its own rows"""
    check_needles(ops, oracle, 7, 256, 512, {9: "w", 33: "h", 52: "w", 70: "h"}, 80, 21, y_edge=128.0)


@pytest.mark.gpu
def test_chunk_edge_14x14_fp16_io(ops, oracle):
    """fp16 gradients in and out, 25 RoIs (one chunk of 24 plus one): against the oracle on the fp16-rounded
    inputs, the bar of test_crowded_band_14x14_fp16_io_against_the_oracle (the mass bar plus one fp16 step of
    the reference)"""
    import torch
    n, C, P = 25, 8, (14, 14)
    rs = np.random.RandomState(1425)
    rois = p2_rois(rs, n, 256, 320)[None]
    feats16 = [rs.standard_normal(s).astype(np.float16) for s in _shapes(C, 256, 320)]
    dy16 = (rs.standard_normal((1, n, C, 14, 14)).astype(f32) * f32(2.0 ** -4)).astype(np.float16)
    shapes = [f.shape for f in feats16]
    f32s = [f.astype(f32) for f in feats16]
    d32 = dy16.astype(f32)
    fw = oracle.fpn_roi_align_fwd(f32s, rois, STRIDES, P, nthreads=8)
    want = _cat(oracle.fpn_roi_align_bwd(d32, rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    mass = _cat(oracle.fpn_roi_align_bwd(np.abs(d32), rois, fw[1], fw[2], shapes, STRIDES, nthreads=8))
    _, am = ops.fpn_roi_align_forward_packed_f16([_t(f) for f in feats16], _t(rois), STRIDES, P)
    g1 = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(rois), am, shapes, STRIDES)
    from simpledet_amd._lib import lib
    assert "roi_align_bwd_packed4<14,14,512,24,1,true>" in (lib().cdll.sd_last_dispatch() or b"").decode()
    g2 = ops.fpn_roi_align_backward_packed_f16(_t(dy16), _t(rois), am, shapes, STRIDES)
    got = _cat([g.cpu().numpy().astype(f32) for g in g1]).astype(np.float64)
    w16 = want.astype(np.float16).astype(np.float64)
    step = np.maximum(np.abs(w16) * 2.0 ** -10, 2.0 ** -24)
    excess = np.maximum(np.abs(got - w16) - step, 0.0)
    bar = float((excess / np.maximum(float(np.median(np.abs(d32))), mass)).max())
    print("fp16 bar %.3g" % bar)
    assert bar <= 1e-4, bar
    assert all(bool(torch.equal(a, b)) for a, b in zip(g1, g2))
