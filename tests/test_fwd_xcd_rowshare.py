"""The knob of the band-resident forward that changes where work runs, never what is computed:

  roi_align_fwd_xcd       0 shares of the cost prefix linear in blockIdx, 1 XCD-contiguous shares (band_xcd_slot),
                          2 the same with the unit table built in an order that interleaves the levels

(The second knob this file was written for, roi_align_fwd_rowshare -- rows of a bin's second y-sample that coincide
with a row of the first not read from LDS again -- was measured slower and is not in the library:
profiles/fwd_xcd_rowshare_ab.txt.  All fifteen GPU cases below passed with it at 0 and 1 before it was taken out; its
row-class inputs stay, they pin the sixteen tap reads of every instantiation whatever reads them.)

Every case runs the forward once per value on identical inputs, with the arg-max buffer, the coordinate table and
the plan buffer filled with a byte pattern before each run, and requires
  * `out` of EVERY value to equal the CPU oracle (oracle.pyoracle.fpn_roi_align_fwd) bit for bit, and
  * `out`, the arg-max, the coordinate table and the whole plan buffer to be byte-identical across the values.

Shapes: the smallest at which each mechanism can go wrong -- fewer units than XCDs, channel counts that are no
multiple of the grab of four (and below it), several bands with RoIs across their edges, a unit table longer than
one wave, and every way the rows of the two y-samples can coincide (one row, the integer row, neighbours, all four
apart, clipped at the border, the zero box), through each instantiation of the kernel.
"""
import ctypes

import numpy as np
import pytest

from . import fp16_edges as E

f32, f16 = np.float32, np.float16
PATTERN = 0xA5
XCD_VALUES = (0, 1, 2)
STRIDES4 = [4, 8, 16, 32]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rois(rs, B, R, img_h, img_w, smin, smax):
    """boxes of sqrt(area) in smin..smax px, aspect 1/2..2, anywhere in the image"""
    s = np.exp(rs.uniform(np.log(smin), np.log(smax), (B, R)))
    ar = np.exp(rs.uniform(np.log(0.5), np.log(2.0), (B, R)))
    w, h = np.minimum(s * np.sqrt(ar), img_w - 2), np.minimum(s / np.sqrt(ar), img_h - 2)
    x1, y1 = rs.uniform(0, img_w - 1 - w), rs.uniform(0, img_h - 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h], -1).astype(f32)


def _rois_all_levels(rs, B, R, img_h, img_w):
    """boxes of 8..600 px around centres anywhere in the image: every level of a four-level pyramid gets some, and
    the large ones reach past the (small) image on every side"""
    s = np.exp(rs.uniform(np.log(8.0), np.log(600.0), (B, R)))
    ar = np.exp(rs.uniform(np.log(0.5), np.log(2.0), (B, R)))
    w, h = s * np.sqrt(ar), s / np.sqrt(ar)
    cx, cy = rs.uniform(0, img_w - 1, (B, R)), rs.uniform(0, img_h - 1, (B, R))
    return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(f32)


def _feats(rs, B, C, img_h, img_w, strides):
    return [rs.standard_normal((B, C, img_h // s, img_w // s)).astype(f32) for s in strides]


def forward(ops, feats, rois, P, strides, mode, xcd):
    """one forward with the knob set -> every buffer it wrote (and the dispatch string).
    mode: "plan" packed arg-max with the backward's plan built in the same step, "f16" packed with fp16 features
    and output, "float" the drop-in ROIAlign_v2 (one level, two float arg-max planes)"""
    import torch
    from simpledet_amd._lib import lib
    from simpledet_amd.ops import _iarr, _p, _parr, _stream
    B, R = rois.shape[:2]
    C = feats[0].shape[1]
    with lib().tuned(roi_align_fwd_xcd=xcd):
        tr = _t(rois)
        if mode == "float":
            assert len(feats) == 1
            out, ax, ay = ops.roi_align_v2_forward(_t(feats[0]), tr, (P, P), 1.0 / strides[0])
            res = dict(out=out, ax=ax, ay=ay)
        else:
            tf = [_t(f.astype(f16) if mode == "f16" else f) for f in feats]
            hs, ws_ = _iarr([f.shape[2] for f in feats]), _iarr([f.shape[3] for f in feats])
            wsb = int(lib().cdll.sd_fpn_roi_align_workspace_bytes(B, R))
            work = torch.empty(wsb, device="cuda", dtype=torch.uint8)
            pat = lambda *shape: torch.full(shape, PATTERN, device="cuda", dtype=torch.uint8)
            out = torch.zeros((B, R, C, P, P), device="cuda", dtype=torch.float16 if mode == "f16" else torch.float32)
            amax = pat(B, R, C, ops.argmax_stride(P, P))
            coords = pat(B, R, 9 * 2 * P * 4).view(torch.float32)
            head = (_parr(tf), hs, ws_, _iarr(strides), len(tf), _p(tr), _p(out), _p(amax), _p(coords))
            tail = (B, C, R, P, P, 224.0, 4.0, _p(work), ctypes.c_size_t(wsb))
            res = dict(out=out, amax=amax, coords=coords)
            if mode == "f16":
                lib().call("sd_fpn_roi_align_fwd_packed_f16", *head, *tail, _stream())
            else:
                pb = int(lib().cdll.sd_fpn_roi_align_plan_bytes(hs, ws_, len(feats), B, R))
                plan = pat(pb)
                lib().call("sd_fpn_roi_align_fwd_packed_plan", *head, *tail, _p(plan), ctypes.c_size_t(pb), _stream())
                res["plan"] = plan
        res["dispatch"] = (lib().cdll.sd_last_dispatch() or b"").decode()
        torch.cuda.synchronize()
    return res


def same_bytes(a, b):
    import torch
    return bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def all_combinations(ops, oracle, feats, rois, P, strides, mode="plan"):
    """the oracle once, then every value of the knob: each equal to the oracle, all equal to one another"""
    kernel = "roi_align_fwd_band<%d,%s,%s>" % (P, "false" if mode == "float" else "true", "true" if mode == "f16" else "false")
    ref_in = [f.astype(f16).astype(f32) for f in feats] if mode == "f16" else feats
    want = oracle.fpn_roi_align_fwd(ref_in, rois, strides, (P, P), nthreads=8)
    first = None
    for xcd in XCD_VALUES:
        got = forward(ops, feats, rois, P, strides, mode, xcd)
        what = "roi_align_fwd_xcd = %d" % xcd
        assert kernel in got["dispatch"] and "[%s]" % what in got["dispatch"], got["dispatch"]
        out = got["out"].cpu().numpy()
        if mode == "f16":
            E.assert_same_half_bits(out, want[0].astype(f16), what + ": fp16 forward against the oracle")
        else:
            assert np.array_equal(out.view(np.uint32), want[0].view(np.uint32)), what + ": out differs from the oracle"
        if mode == "float":
            assert np.array_equal(got["ax"].cpu().numpy(), want[1]) and np.array_equal(got["ay"].cpu().numpy(), want[2]), what
        if first is None:
            first = got
            continue
        assert sorted(got) == sorted(first)
        for k in got:
            if k != "dispatch":
                assert same_bytes(got[k], first[k]), "%s differs between %s and roi_align_fwd_xcd = %d" % (k, what, XCD_VALUES[0])
    return first, want


# ------------------------------------------------------------------------------------------------- the cases
@pytest.mark.gpu
@pytest.mark.parametrize("C", [8, 6, 3, 1])
def test_four_small_levels(ops, oracle, C):
    """(32,40), (16,20), (8,10), (4,5), B = 2, R = 24: eight units at most, fewer workgroups with work than XCDs
    have blocks; C = 6, 3, 1: no multiple of the grab of four channels, and below it"""
    rs = np.random.RandomState(100 + C)
    feats = _feats(rs, 2, C, 128, 160, STRIDES4)
    assert [f.shape[2:] for f in feats] == [(32, 40), (16, 20), (8, 10), (4, 5)]
    rois = _rois_all_levels(rs, 2, 24, 128, 160)
    _, level = oracle.fpn_roi_assign(rois, STRIDES4)
    assert len(set(level.ravel().tolist())) == 4, "RoIs on every level"
    all_combinations(ops, oracle, feats, rois, 7, STRIDES4)


@pytest.mark.gpu
def test_several_bands_at_small_size(ops, oracle):
    """one level of 60 x 80, R = 300, C = 4: the launcher's item rule cuts the plane into five bands of twelve
    rows; the RoIs whose bin rows lie in two bands are written by two units"""
    rs = np.random.RandomState(7)
    feats = _feats(rs, 1, 4, 240, 320, [4])
    assert feats[0].shape[2:] == (60, 80)
    rois = _rois(rs, 1, 300, 240, 320, 16.0, 120.0)
    plan = E.fwd_band_plan([(60, 80)], 4, 300, 7, half=False)[0]
    assert plan["nbands"] == 5 and plan["owned"] == 12, plan
    y1, y2 = rois[0, :, 1] / 4.0, rois[0, :, 3] / 4.0
    assert (np.floor(y1 / 12) != np.floor(y2 / 12)).sum() >= 50, "RoIs across a band edge"
    all_combinations(ops, oracle, feats, rois, 7, [4])


def _units(shapes, B, C, R, P):
    return B * sum(p["nbands"] for p in E.fwd_band_plan(shapes, C, R, P, half=False))


@pytest.mark.gpu
@pytest.mark.parametrize("R", [64, 600])
def test_two_waves_of_the_unit_table(ops, oracle, R):
    """B = 8, four tiny levels, C = 4.  R = 64: one band per level, 32 units -- the order of roi_align_fwd_xcd = 2
    differs from the unit order at every place.  R = 600: the item rule makes three bands of a level (two of the
    four-row one: it stays whole at two), 72 units: the table, its order and the cost prefix span two waves"""
    rs = np.random.RandomState(200 + R)
    feats = _feats(rs, 8, 4, 128, 160, STRIDES4)
    shapes = [f.shape[2:] for f in feats]
    units = _units(shapes, 8, 4, R, 7)
    print("R = %d: %d units" % (R, units))
    assert units == (32 if R == 64 else 72)
    rois = _rois_all_levels(rs, 8, R, 128, 160)
    all_combinations(ops, oracle, feats, rois, 7, STRIDES4)


# ---- row classes: how the rows of a bin's two y-samples coincide
MAP_H, MAP_W, STRIDE = 64, 80, 4


def row_class_rois(P, seed):
    """RoIs on a 64 x 80 map (stride 4) whose bins are 0.5, 3.0 (integer origins), 2.5 and 3.9 px high on the map,
    six of each at different offsets and widths, then one box clipped at the bottom and right border and one zero
    box; coordinates in image pixels"""
    rs = np.random.RandomState(seed)
    boxes = []
    for bin_h in (0.5, 3.0, 2.5, 3.9):
        h = bin_h * P                                   # on the map
        for k in range(6):
            y1 = float(rs.randint(0, int(MAP_H - 1 - h))) if bin_h == 3.0 else rs.uniform(0.0, MAP_H - 1 - h)
            w = rs.uniform(3.0, 40.0)
            x1 = rs.uniform(0.0, MAP_W - 1 - w)
            boxes.append([x1 * STRIDE, y1 * STRIDE, (x1 + w) * STRIDE, (y1 + h) * STRIDE])
    boxes.append([(MAP_W - 20.0) * STRIDE, (MAP_H - 2.9 * P) * STRIDE, (MAP_W + 6.0) * STRIDE, (MAP_H + 5.0) * STRIDE])
    boxes.append([0.0, 0.0, 0.0, 0.0])
    return np.asarray(boxes, f32)[None]


def sample_rows(rois, P):
    """per (RoI, bin row): (low, high) rows of the first two y-samples, by the reference's float32 expressions;
    None where the bin has fewer than two samples"""
    scale = f32(1.0) / f32(STRIDE)
    res = []
    for box in rois[0]:
        a, e = f32(box[1]) * scale, f32(box[3]) * scale
        b = f32(e - a) / f32(P)
        for p in range(P):
            lo = min(max(f32(f32(f32(p) * b) + a), f32(0)), f32(MAP_H - 1))
            hi = min(max(f32(f32(f32(p + 1) * b) + a), f32(0)), f32(MAP_H - 1))
            if hi <= lo:
                res.append(None)
                continue
            st = f32(hi - lo) / f32(3.0)
            y0 = f32(lo + st)
            y1 = f32(y0 + max(st, f32(0.01)))
            rows = lambda y: (min(max(int(np.floor(y)), 0), MAP_H - 1), min(max(int(np.ceil(y)), 0), MAP_H - 1))
            res.append(rows(y0) + rows(y1))
    return res


def row_class_inputs(P, C, values, seed=5):
    rois = row_class_rois(P, seed)
    if values == "normal":
        feat = np.random.RandomState(seed + 1).standard_normal((1, C, MAP_H, MAP_W)).astype(f32)
    else:   # plane value = row * W + col (+ the channel): a tap from a wrong place is a wrong integer
        feat = (np.arange(MAP_H * MAP_W, dtype=f32).reshape(1, 1, MAP_H, MAP_W) + np.arange(C, dtype=f32).reshape(1, C, 1, 1))
    return [np.ascontiguousarray(feat, f32)], rois


@pytest.mark.parametrize("P", [7, 14])
def test_row_class_inputs_hold_every_class(P):
    """(no GPU) the RoIs above produce what they are meant to: the low row of sample 1 on sample 0's low row, on its
    high row and on neither; a bin whose sample sits on an integer row (low == high); bins without a second sample"""
    rows = sample_rows(row_class_rois(P, 5), P)
    have = [r for r in rows if r is not None]
    n_same = sum(r[2] == r[0] for r in have)
    n_next = sum(r[2] != r[0] and r[2] == r[1] for r in have)
    n_apart = sum(r[2] != r[0] and r[2] != r[1] for r in have)
    n_int = sum(r[0] == r[1] for r in have)
    n_hi_shared = sum(r[3] == r[1] for r in have)
    print("P = %d: %d bin rows, low row of sample 1 on low %d / on high %d / apart %d, integer rows %d, high rows shared %d,"
          " empty %d" % (P, len(rows), n_same, n_next, n_apart, n_int, n_hi_shared, len(rows) - len(have)))
    assert min(n_same, n_next, n_apart, n_int, n_hi_shared) >= P and len(rows) - len(have) >= P


@pytest.mark.gpu
@pytest.mark.parametrize("values", ["normal", "ramp"])
@pytest.mark.parametrize("P,mode", [(7, "plan"), (14, "plan"), (7, "float"), (7, "f16")])
def test_row_classes(ops, oracle, P, mode, values):
    feats, rois = row_class_inputs(P, 8, values)
    first, want = all_combinations(ops, oracle, feats, rois, P, [STRIDE], mode)
    # the zero box pools nothing, the clipped box pools something
    assert (want[1][0, -1] == -1).all() and (want[1][0, -2] != -1).any()
