"""The rois-only tables that no forward kernel reads -- the packed arg-max's coordinate table and the backward's
plan (band lists, tap tables, weight bounds) -- built as tasks in the tail of roi_align_fwd_band
(roi_align_plan_tail = 1, the default) instead of as blocks of the pre-pass launch (= 0).

Every case runs forward + backward twice in this process on identical inputs, once per value of the knob, with
the plan buffer, the coordinate table and the arg-max buffer filled with a byte pattern before each run (regions
nobody writes compare equal), and requires `out`, the arg-max, `coords`, the ENTIRE plan buffer and every
gradient to be byte-identical.  One case is checked against the CPU oracle as well (forward exact, backward
1e-4, the bars of tests/test_roi_align.py): equality with the twin alone would let both be wrong.

Shapes: the smallest at which each mechanism can go wrong -- more tasks than the 256 persistent workgroups, far
fewer, workgroups that made no band visit, units with empty lists, R on either side of a wave, several bands per
unit, 14 x 14, fp16, the float arg-max form (no such tasks), the task counter on a reused workspace, and the
forward alone (the coordinate table is an output of the op).  C = 8 throughout.

The rewritten spot of bwd_band_list (no address taken of the first sweep's box) has no host build; the plan
equality of these cases against the merged pre-pass -- same function, other launch -- and the oracle case are
its check.
"""
import ctypes
import re

import numpy as np
import pytest

STRIDES = [4, 8, 16, 32]
f32 = np.float32
C = 8
PATTERN = 0xA5
NWG = 256          # persistent workgroups of the band kernel: one per CU
KNOB = "roi_align_plan_tail"


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _shapes(B, img_h, img_w, strides):
    return [(B, C, img_h // s, img_w // s) for s in strides]


def _feats(rs, B, img_h, img_w, strides):
    return [rs.standard_normal(s).astype(f32) for s in _shapes(B, img_h, img_w, strides)]


def _rois(rs, B, R, img_h, img_w, smin, smax):
    """boxes of sqrt(area) in smin..smax px, aspect 1/2..2, anywhere in the image"""
    s = np.exp(rs.uniform(np.log(smin), np.log(smax), (B, R)))
    ar = np.exp(rs.uniform(np.log(0.5), np.log(2.0), (B, R)))
    w, h = np.minimum(s * np.sqrt(ar), img_w - 2), np.minimum(s / np.sqrt(ar), img_h - 2)
    x1, y1 = rs.uniform(0, img_w - 1 - w), rs.uniform(0, img_h - 1 - h)
    return np.stack([x1, y1, x1 + w, y1 + h], -1).astype(f32)


def task_counts(feat_hw, B, R, P, packed=True, plan=True):
    """(coordinate tasks, plan tasks) by the launcher's formulas: 1024 (RoI, coordinate) pairs per coordinate task;
    per (level, image, band) unit of the backward -- bands of at most 27 KB of a plane -- two tap-table tasks and,
    when some level's band has at most 10240 cells of 4 x 4 pixels (+ one border cell each way), one for the bound"""
    ncoord = -(-B * R * 6 * P // 1024) if packed else 0
    if not plan:
        return ncoord, 0
    units, pix = 0, False
    for H, W in feat_hw:
        nb = max(1, -(-H * W * 4 // (27 * 1024)))
        rows = -(-H // nb)
        nb = -(-H // rows)
        units += B * nb
        pix = pix or (((rows - 1) >> 2) + 2) * (((W - 1) >> 2) + 2) <= 10240
    return ncoord, units * (2 + (1 if pix else 0))


def parsed_counts(dispatch):
    m = re.search(r"tail tasks: (\d+) coordinate table \+ (\d+) backward plan", dispatch)
    return (int(m.group(1)), int(m.group(2))) if m else None


class Buffers:
    """workspace and plan buffer of one (B, R, level sizes): kept across the rounds of the counter-reset case"""

    def __init__(self, feats, R):
        import torch
        from simpledet_amd._lib import lib
        from simpledet_amd.ops import _iarr
        B = feats[0].shape[0]
        self.hs, self.ws_ = _iarr([f.shape[2] for f in feats]), _iarr([f.shape[3] for f in feats])
        self.wsb = int(lib().cdll.sd_fpn_roi_align_workspace_bytes(B, R))
        self.pb = int(lib().cdll.sd_fpn_roi_align_plan_bytes(self.hs, self.ws_, len(feats), B, R))
        self.work = torch.empty(self.wsb, device="cuda", dtype=torch.uint8)
        self.plan = torch.empty(self.pb, device="cuda", dtype=torch.uint8)


def step(ops, feats, rois, dy, P, strides, tail, mode="plan", bufs=None, backward=True):
    """forward (+ backward) with roi_align_plan_tail = tail -> every buffer the step wrote, and the forward's
    dispatch string.  mode: "plan" packed arg-max with the backward's plan, "noplan" packed without,
    "f16" packed with fp16 features / output / gradients, "float" the two float arg-max planes"""
    import torch
    from simpledet_amd._lib import lib
    from simpledet_amd.ops import _iarr, _p, _parr, _stream
    B, R = rois.shape[:2]
    tf = [_t(f.astype(np.float16) if mode == "f16" else f) for f in feats]
    tr = _t(rois)
    shapes = [f.shape for f in feats]
    bufs = bufs or Buffers(feats, R)
    S = ops.argmax_stride(P, P)
    pat = lambda *shape: torch.full(shape, PATTERN, device="cuda", dtype=torch.uint8)
    out = torch.zeros((B, R, C, P, P), device="cuda", dtype=torch.float16 if mode == "f16" else torch.float32)
    amax = pat(B, R, C, S)
    coords = pat(B, R, 9 * 2 * P * 4).view(torch.float32)
    bufs.plan.fill_(PATTERN)
    res = {"out": out}
    tail_args = (B, C, R, P, P, 224.0, 4.0, _p(bufs.work), ctypes.c_size_t(bufs.wsb))
    head = (_parr(tf), bufs.hs, bufs.ws_, _iarr(strides), len(tf), _p(tr), _p(out))
    with lib().tuned(**{KNOB: tail}):
        if mode == "float":
            ax, ay = torch.zeros_like(out), torch.zeros_like(out)
            lib().call("sd_fpn_roi_align_fwd", *head, _p(ax), _p(ay), *tail_args, _stream())
            res.update(ax=ax, ay=ay)
        elif mode == "plan":
            lib().call("sd_fpn_roi_align_fwd_packed_plan", *head, _p(amax), _p(coords), *tail_args,
                       _p(bufs.plan), ctypes.c_size_t(bufs.pb), _stream())
        else:
            lib().call("sd_fpn_roi_align_fwd_packed_f16" if mode == "f16" else "sd_fpn_roi_align_fwd_packed",
                       *head, _p(amax), _p(coords), *tail_args, _stream())
        res["dispatch"] = (lib().cdll.sd_last_dispatch() or b"").decode()
        if mode != "float":
            res.update(amax=amax, coords=coords)
        if mode == "plan":
            res["plan"] = bufs.plan.clone()
        if backward:
            tdy = _t(dy.astype(np.float16) if mode == "f16" else dy)
            if mode == "float":
                g = ops.fpn_roi_align_backward(tdy, tr, ax, ay, shapes, strides)
            elif mode == "f16":
                g = ops.fpn_roi_align_backward_packed_f16(tdy, tr, (amax, coords), shapes, strides)
            elif mode == "noplan":
                g = ops.fpn_roi_align_backward_packed(tdy, tr, (amax, coords), shapes, strides)
            else:
                g = [pat(*s, 4).view(torch.float32).reshape(s) for s in shapes]
                lib().call("sd_fpn_roi_align_bwd_packed_plan", _p(tdy), _p(tr), _p(amax), _p(coords), _parr(g),
                           bufs.hs, bufs.ws_, _iarr(strides), len(g), 1, B, C, R, P, P, 224.0, 4.0,
                           _p(bufs.plan), ctypes.c_size_t(bufs.pb), _stream())
                assert "roi_align_bwd_packed4" in (lib().cdll.sd_last_dispatch() or b"").decode()
            for i, t in enumerate(g):
                res["d_feat_%d" % i] = t
        torch.cuda.synchronize()
    return res


def same_bytes(a, b):
    import torch
    return bool(torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)))


def twins(ops, feats, rois, dy, P, strides, mode="plan", backward=True, bufs=None):
    """the step with the tables in the band kernel's tail and with the parent's pre-pass: byte-identical"""
    import torch
    new = step(ops, feats, rois, dy, P, strides, 1, mode, bufs, backward)
    old = step(ops, feats, rois, dy, P, strides, 0, mode, None, backward)
    assert "roi_align_fwd_band" in new["dispatch"] and "roi_align_fwd_band" in old["dispatch"]
    assert "tail tasks" not in old["dispatch"]
    if mode == "plan":
        assert "roi_prep_merged_kernel" in old["dispatch"] and "roi_fwd_prep_kernel" in new["dispatch"]
    assert (parsed_counts(new["dispatch"]) is None) == (mode == "float")
    assert sorted(new) == sorted(old)
    if mode == "plan":
        # a precondition on the INPUTS: the backward sums a band in fixed point -- bit-reproducibly -- only while the
        # band's weight bound (word 1 of its list in the plan) is at most 2048; a more crowded band takes float adds
        # in hardware order, and two runs of the same build differ in the last bits
        B, R = rois.shape[:2]
        units = task_counts(hw(feats), B, R, P)[1] // 3
        lists = old["plan"][:units * (R + 2) * 4].view(torch.int32).reshape(units, R + 2).cpu().numpy()
        print("weight bounds of the %d units: max %d" % (units, lists[:, 1].max()))
        assert lists[:, 1].max() <= 2048, "inputs too crowded for a bit-exact comparison of the gradients"
    for k in new:
        if k != "dispatch":
            assert same_bytes(new[k], old[k]), "%s differs between roi_align_plan_tail = 1 and 0" % k
    return new


def case(seed, B, R, img_h, img_w, strides=STRIDES, P=7, smin=8.0, smax=150.0):
    rs = np.random.RandomState(seed)
    feats = _feats(rs, B, img_h, img_w, strides)
    rois = _rois(rs, B, R, img_h, img_w, smin, smax)
    dy = rs.standard_normal((B, R, C, P, P)).astype(f32)
    return feats, rois, dy


def hw(feats):
    return [f.shape[2:] for f in feats]


# ----------------------------------------------------------------------------------------------- the cases
@pytest.mark.gpu
def test_more_tasks_than_workgroups(ops):
    """B = 8, R = 512, four levels of a 128 x 160 image: 168 coordinate tasks and 3 per backward unit, more than
    the 256 workgroups -- some draw a second number"""
    feats, rois, dy = case(1, 8, 512, 128, 160, smin=8.0, smax=20.0)
    # half small boxes on P2, half of 115..150 px on P3 (P4 and P5: empty lists): 512 small boxes, or uniform
    # boxes of every size, pile more weight on a pixel of these tiny maps than the backward's fixed point takes
    # (weight bound > 2048: float adds in hardware order, not reproducible bit for bit -- see twins())
    rois[:, ::2] = _rois(np.random.RandomState(101), 8, 256, 128, 160, 115.0, 150.0)
    want = task_counts(hw(feats), 8, 512, 7)
    assert want[0] == 168 and sum(want) > NWG, want
    new = twins(ops, feats, rois, dy, 7, STRIDES)
    assert parsed_counts(new["dispatch"]) == want


@pytest.mark.gpu
def test_far_fewer_tasks_than_workgroups(ops):
    feats, rois, dy = case(2, 1, 5, 128, 160)
    want = task_counts(hw(feats), 1, 5, 7)
    assert 0 < sum(want) < NWG // 8, want
    new = twins(ops, feats, rois, dy, 7, STRIDES)
    assert parsed_counts(new["dispatch"]) == want


@pytest.mark.gpu
def test_workgroups_without_a_band_visit(ops):
    """one level, a 16 x 20 map, three RoIs: one unit, almost every workgroup goes straight to the tail"""
    feats, rois, dy = case(3, 1, 3, 64, 80, strides=[4], smin=8.0, smax=40.0)
    assert hw(feats) == [(16, 20)]
    twins(ops, feats, rois, dy, 7, [4])


def samples_per_bin(start, end, stride, size, pooled):
    """iterations of the reference's sample loop along one axis, per bin (oracle/roi_align_v2.c: float32, the two
    double expressions kept)"""
    scale = f32(1.0) / f32(stride)
    a, e = f32(start) * scale, f32(end) * scale
    b = f32(e - a) / f32(pooled)
    out = []
    for p in range(pooled):
        lo = min(max(f32(f32(f32(p) * b) + a), f32(0)), f32(size - 1))
        hi = min(max(f32(f32(f32(p + 1) * b) + a), f32(0)), f32(size - 1))
        n = 0
        if not hi <= lo:
            st = f32(np.float64(f32(hi - lo)) / 3.0)
            lim = np.float64(f32(hi - st)) + 0.01
            x = f32(lo + st)
            while np.float64(x) <= lim:
                n += 1
                x = f32(x + max(st, f32(0.01)))
        out.append(n)
    return out


def thin_box(rs):
    """a box 0.2 px wide on the P2 map (0.84 px of the image): its bins are 0.03 px, the sample stride rounds to
    0.01 px and some bins get a third sample (a rounding event: searched, a few tries)"""
    for _ in range(4000):
        x1 = f32(rs.uniform(8.0, 300.0))
        x2 = f32(x1 + f32(0.84 * (1.0 + rs.uniform(-3e-4, 3e-4))))
        if sum(n == 3 for n in samples_per_bin(x1, x2, 4, 80, 7)) >= 3:
            return [x1, 50.0, x2, 120.0]
    raise AssertionError("no thin box found")


def awkward_rois(R, seed):
    """all on P2 of a 256 x 320 image (the other levels' units have empty lists), with a few zero boxes, a NaN box
    (no level: its rows of the coordinate table are never written) and a box 0.2 px wide on the map (bins that
    name the third candidate: the side table)"""
    rs = np.random.RandomState(seed)
    rois = _rois(rs, 1, R, 256, 320, 20.0, 100.0)
    rois[0, 3] = 0.0
    rois[0, 17] = 0.0
    rois[0, R - 1] = 0.0
    rois[0, 9] = np.nan
    rois[0, 30] = thin_box(rs)
    return rois


@pytest.mark.gpu
@pytest.mark.parametrize("R", [63, 65])
def test_empty_units_and_r_around_a_wave(ops, oracle, R):
    rs = np.random.RandomState(40 + R)
    feats = _feats(rs, 1, 256, 320, STRIDES)
    rois = awkward_rois(R, R)
    dy = rs.standard_normal((1, R, C, 7, 7)).astype(f32)
    _, level = oracle.fpn_roi_assign(rois, STRIDES)
    assert level[0, 9] < 0 and (np.delete(level[0], 9) == 0).all(), level
    new = twins(ops, feats, rois, dy, 7, STRIDES)
    if R != 65:
        return
    # ... and against the oracle: forward exact, backward 1e-4
    fw = oracle.fpn_roi_align_fwd(feats, rois, STRIDES, (7, 7), nthreads=8)
    assert np.array_equal(new["out"].cpu().numpy(), fw[0])
    codes = ops.argmax_codes(new["amax"], (7, 7)).cpu().numpy()
    check_table(codes, new["coords"].cpu().numpy(), fw[1], fw[2], 7)
    assert (codes[0, 30] % 3 == 2).any(), "the 0.2 px box names no third candidate"
    wd = oracle.fpn_roi_align_bwd(dy, rois, fw[1], fw[2], [f.shape for f in feats], STRIDES, nthreads=8)
    for i, w in enumerate(wd):
        err = float(np.abs(new["d_feat_%d" % i].cpu().numpy() - w).max())
        print("level %d max |got - oracle| = %.3g" % (i, err))
        assert err <= 1e-4, (i, err)


@pytest.mark.gpu
def test_multi_band_units(ops):
    """one level of 120 x 334 (P2's width): 157 KB of plane is six 27 KB bands of the backward and several of the
    forward; boxes of 20..200 px all over the image cross their edges"""
    feats, rois, dy = case(5, 1, 96, 480, 1336, strides=[4], smin=20.0, smax=200.0)
    assert hw(feats) == [(120, 334)]
    want = task_counts(hw(feats), 1, 96, 7)
    assert want[1] == 6 * 3, want
    rows = -(-120 // 6)
    y1, y2 = rois[0, :, 1] / 4.0, rois[0, :, 3] / 4.0
    assert ((np.floor(y1 / rows) != np.floor(y2 / rows)).sum()) >= 10, "RoIs across a band edge"
    new = twins(ops, feats, rois, dy, 7, [4])
    assert parsed_counts(new["dispatch"]) == want


@pytest.mark.gpu
def test_pooling_14x14(ops):
    feats, rois, dy = case(6, 2, 40, 256, 320, P=14)
    new = twins(ops, feats, rois, dy, 14, STRIDES)
    assert "roi_align_fwd_band<14,true,false>" in new["dispatch"]
    assert parsed_counts(new["dispatch"]) == task_counts(hw(feats), 2, 40, 14)


@pytest.mark.gpu
def test_fp16_io(ops):
    """the fp16 entry takes no plan: coordinate tasks only"""
    feats, rois, dy = case(7, 2, 40, 256, 320)
    new = twins(ops, feats, rois, dy * f32(2.0 ** -4), 7, STRIDES, mode="f16")
    assert "roi_align_fwd_band<7,true,true>" in new["dispatch"]
    assert parsed_counts(new["dispatch"]) == task_counts(hw(feats), 2, 40, 7, plan=False)


@pytest.mark.gpu
def test_float_argmax_has_no_tail_tasks(ops):
    """<7,false>: no coordinate table, and its entry takes no plan"""
    feats, rois, dy = case(8, 2, 40, 256, 320)
    new = twins(ops, feats, rois, dy, 7, STRIDES, mode="float")
    assert "roi_align_fwd_band<7,false,false>" in new["dispatch"]


@pytest.mark.gpu
def test_task_counter_is_reset_on_a_reused_workspace(ops):
    """two steps on the same workspace and plan buffer with different rois: a counter left at its last value
    would hand out no task in the second step, and the pattern would still be in its tables"""
    feats, rois_a, dy = case(9, 2, 65, 256, 320)
    rois_b = _rois(np.random.RandomState(10), 2, 65, 256, 320, 8.0, 150.0)
    bufs = Buffers(feats, 65)
    a = twins(ops, feats, rois_a, dy, 7, STRIDES, bufs=bufs)
    b = twins(ops, feats, rois_b, dy, 7, STRIDES, bufs=bufs)
    assert not same_bytes(a["plan"], b["plan"]) and not same_bytes(a["coords"], b["coords"])


def check_table(codes, coords, want_ax, want_ay, P):
    """the coordinate table, looked up with the arg-max codes, holds the oracle's float coordinates"""
    B, R = codes.shape[:2]
    code = codes.astype(np.int64)
    ok = code != 255
    pp, qq = np.meshgrid(np.arange(P), np.arange(P), indexing="ij")
    bi = np.arange(B)[:, None, None, None, None]
    ri = np.arange(R)[None, :, None, None, None]
    ty = coords[bi, ri, np.where(ok, pp * 3 + code // 3, 0)]
    tx = coords[bi, ri, 3 * P + np.where(ok, qq * 3 + code % 3, 0)]
    assert np.array_equal(ok, want_ax != -1)
    assert np.array_equal(np.where(ok, ty, f32(-1)), want_ay)
    assert np.array_equal(np.where(ok, tx, f32(-1)), want_ax)


@pytest.mark.gpu
def test_forward_alone_completes_the_coordinate_table(ops, oracle):
    """no plan, no backward: `coords` is an output of the op, whole when the launch is done"""
    feats, rois, dy = case(11, 2, 65, 256, 320)
    rois[1, 4] = np.nan
    new = twins(ops, feats, rois, dy, 7, STRIDES, mode="noplan", backward=False)
    assert parsed_counts(new["dispatch"]) == task_counts(hw(feats), 2, 65, 7, plan=False)
    fw = oracle.fpn_roi_align_fwd(feats, rois, STRIDES, (7, 7), nthreads=8)
    assert np.array_equal(new["out"].cpu().numpy(), fw[0])
    coords = new["coords"].cpu().numpy()
    check_table(ops.argmax_codes(new["amax"], (7, 7)).cpu().numpy(), coords, fw[1], fw[2], 7)
    # every word of every RoI that has a level is written; the NaN box's stay as they were
    words = coords.view(np.uint32).reshape(2, 65, -1)
    untouched = (words == 0xA5A5A5A5).all(-1)
    assert untouched[1, 4] and untouched.sum() == 1
    assert not (words[~untouched] == 0xA5A5A5A5).any()
