"""The knobs of the band-resident forward that decide WHERE and in what pieces the work is done, never what is computed:

  roi_align_fwd_staff        0 a workgroup starts where the midpoint of its share of the cost prefix falls,
                             1 whole workgroups per virtual unit (band_staffing, roi_align_common.h)
  roi_align_fwd_grab         channels a workgroup reserves at a time (rounded up to whole fills; 0: the launcher's choice)
  roi_align_fwd_tail         last per cent of a unit's channels handed out in smaller pieces ...
  roi_align_fwd_tail_planes  ... of this many planes

Every case runs the forward once per (staffing, reservation setting) on identical inputs, with the arg-max buffer, the
coordinate table and the plan buffer filled with a byte pattern before each run, and requires `out` of EVERY run to
equal the CPU oracle bit for bit and `out`, the arg-max, the coordinate table and the whole plan buffer to be
byte-identical across the runs.  The shapes are the smallest that reach each branch of the start-up; the device form of
band_staffing itself is held to the plain-integer restatement of tools/fwd_schedule_model.py on random vectors.
"""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

from . import fp16_edges as E

f32, f16 = np.float32, np.float16
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATTERN = 0xA5
KNOBS = ("roi_align_fwd_staff", "roi_align_fwd_grab", "roi_align_fwd_tail", "roi_align_fwd_tail_planes")
# (grab, tail, tail_planes): four channels, two, coarser and finer reservations, tails of whole fills, of part fills, of single planes
RESERVATIONS = ((4, 0, 8), (2, 0, 8), (8, 0, 8), (1, 0, 8), (4, 20, 4), (4, 50, 1), (16, 30, 2))
SETTINGS = tuple((staff,) + r for staff in (0, 1) for r in RESERVATIONS)
STRIDES4 = [4, 8, 16, 32]
_CACHE = {}


def tool(name):
    if name not in _CACHE:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _CACHE[name] = mod
    return _CACHE[name]


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _rois(rs, B, R, y_lo, y_hi, x_hi, smin, smax):
    """boxes of sqrt(area) in smin..smax px, aspect 1/2..2, whose top edge lies in y_lo..y_hi"""
    s = np.exp(rs.uniform(np.log(smin), np.log(smax), (B, R)))
    ar = np.exp(rs.uniform(np.log(0.5), np.log(2.0), (B, R)))
    w, h = s * np.sqrt(ar), s / np.sqrt(ar)
    x1, y1 = rs.uniform(0, x_hi - w), rs.uniform(y_lo, y_hi, (B, R))
    return np.stack([x1, y1, x1 + w, y1 + h], -1).astype(f32)


def _feats(rs, B, C, shapes):
    return [rs.standard_normal((B, C, h, w)).astype(f32) for h, w in shapes]


def forward(ops, feats, rois, P, strides, mode, setting):
    """one forward with the knobs set -> every buffer it wrote (and the dispatch string); mode "plan": packed arg-max
    with the backward's plan built in the same step, "f16": packed with fp16 features and output"""
    import torch
    from simpledet_amd._lib import lib
    from simpledet_amd.ops import _iarr, _p, _parr, _stream
    B, R = rois.shape[:2]
    C = feats[0].shape[1]
    with lib().tuned(**dict(zip(KNOBS, setting))):
        tr = _t(rois)
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


def every_setting(ops, oracle, feats, rois, P, strides, mode="plan"):
    """the oracle once, then every (staffing, reservations): each equal to the oracle, all equal to one another"""
    kernel = "roi_align_fwd_band<%d,true,%s>" % (P, "true" if mode == "f16" else "false")
    ref_in = [f.astype(f16).astype(f32) for f in feats] if mode == "f16" else feats
    want = oracle.fpn_roi_align_fwd(ref_in, rois, strides, (P, P), nthreads=8)
    first = None
    for setting in SETTINGS:
        got = forward(ops, feats, rois, P, strides, mode, setting)
        what = "[roi_align_fwd_staff = %d] [reservations: grab %d, tail %d %% in pieces of %d planes]" % setting
        assert kernel in got["dispatch"] and what in got["dispatch"], got["dispatch"]
        out = got["out"].cpu().numpy()
        if mode == "f16":
            E.assert_same_half_bits(out, want[0].astype(f16), what + ": fp16 forward against the oracle")
        else:
            assert np.array_equal(out.view(np.uint32), want[0].view(np.uint32)), what + ": out differs from the oracle"
        if first is None:
            first = got
            continue
        assert sorted(got) == sorted(first)
        for k in got:
            if k != "dispatch":
                assert same_bytes(got[k], first[k]), "%s differs between %s and the first setting" % (k, what)
    return want


def table(feats, rois, strides, P=7):
    """the kernel's virtual units for these inputs, by the restatement of tools/fwd_traffic_model.py (7x7, fp32)"""
    vus, units = tool("fwd_traffic_model").virtual_units(rois, [f.shape[2:] for f in feats], strides, feats[0].shape[1], P, xcd=1)
    return vus, units


# ------------------------------------------------------------------------------------------------- the cases
@pytest.mark.gpu
def test_one_unit(ops, oracle):
    """one level, one image, a map of one band, C = 8: one virtual unit of two reservations and 256 workgroups, all
    but two of them with nothing to take"""
    rs = np.random.RandomState(11)
    feats = _feats(rs, 1, 8, [(16, 20)])
    rois = _rois(rs, 1, 24, 0, 40, 76, 8.0, 24.0)
    vus, units = table(feats, rois, [4])
    assert units == 1 and len(vus) == 1
    every_setting(ops, oracle, feats, rois, 7, [4])


@pytest.mark.gpu
def test_seven_rounds_of_one_unit(ops, oracle):
    """R = 512 boxes on one band of one level, C = 8: the band's 3584 items are seven rounds of what a workgroup
    holds, seven virtual units of ONE unit; the level's other bands hold no item"""
    rs = np.random.RandomState(12)
    feats = _feats(rs, 1, 8, [(64, 80)])
    plan = E.fwd_band_plan([(64, 80)], 8, 512, 7, half=False)[0]
    assert plan["nbands"] == 8 and plan["owned"] == 8, plan
    rois = _rois(rs, 1, 512, 0.0, 6.0, 316, 8.0, 20.0)     # top edge in map rows 0 .. 1.5, at most 7 rows high
    vus, units = table(feats, rois, [4])
    assert units == 8 and [v["items"] for v in vus] == [576] * 6 + [128], [v["items"] for v in vus]
    assert len(set(id(v["unit"]) for v in vus)) == 1, "all rounds belong to the first band"
    every_setting(ops, oracle, feats, rois, 7, [4])


@pytest.mark.gpu
def test_twenty_four_images(ops, oracle):
    """B = 24 images, four levels at the benchmark's map sizes, C = 4, R = 8: 216 units, a third of them with items
    -- a unit table of four waves of which band_staffing sees two lanes' worth, units of one fill per reservation
    next to units of four-plane fills.  (Fewer virtual units than workgroups: the rule applies; the case below
    is the one where it does not.)"""
    from simpledet_amd import synth
    rs = np.random.RandomState(13)
    feats = _feats(rs, 24, 4, synth.FPN_SHAPES)
    rois = synth.random_rois(13, 24, 8)
    vus, units = table(feats, rois, STRIDES4)
    print("%d units, %d virtual units" % (units, len(vus)))
    assert units == 216 and 64 < len(vus) <= 216
    every_setting(ops, oracle, feats, rois, 7, STRIDES4)


@pytest.mark.gpu
def test_more_virtual_units_than_workgroups(ops, oracle):
    """B = 40 images of the same pyramid, R = 24: more than 256 virtual units, so band_staffing does not apply
    and roi_align_fwd_staff = 1 keeps the midpoint rule (the 24-image case above stays below 256)"""
    from simpledet_amd import synth
    rs = np.random.RandomState(14)
    feats = _feats(rs, 40, 4, synth.FPN_SHAPES)
    rois = synth.random_rois(14, 40, 24)
    vus, units = table(feats, rois, STRIDES4)
    print("%d units, %d virtual units" % (units, len(vus)))
    assert units == 360 and len(vus) > 256
    every_setting(ops, oracle, feats, rois, 7, STRIDES4)


@pytest.mark.gpu
def test_a_band_without_items(ops, oracle):
    """two levels of three bands, two images; every box of the fine level lies in its first or its last band: the
    band between holds no item and is no virtual unit"""
    rs = np.random.RandomState(15)
    feats = _feats(rs, 2, 8, [(60, 80), (30, 40)])
    plan = E.fwd_band_plan([(60, 80), (30, 40)], 8, 300, 7, half=False)
    assert plan[0]["nbands"] == 3 and plan[0]["owned"] == 20, plan
    small = np.concatenate([_rois(rs, 2, 100, 0.0, 20.0, 300, 10.0, 40.0), _rois(rs, 2, 100, 180.0, 200.0, 300, 10.0, 30.0)], 1)
    large = _rois(rs, 2, 100, 0.0, 60.0, 150, 120.0, 170.0)
    rois = np.ascontiguousarray(np.concatenate([small, large], 1))
    vus, units = table(feats, rois, [4, 8])
    per_unit = sorted(set((v["unit"]["level"], id(v["unit"])) for v in vus))
    assert units == 12 and len(per_unit) == 10, (units, len(per_unit))
    every_setting(ops, oracle, feats, rois, 7, [4, 8])


@pytest.mark.gpu
def test_short_last_reservation(ops, oracle):
    """C = 10 with reservations of four channels: three reservations, the last of two channels (and with grab 8 / 16
    one short reservation or none whole)"""
    rs = np.random.RandomState(16)
    feats = _feats(rs, 2, 10, [(32, 40), (16, 20)])
    rois = _rois(rs, 2, 48, 0.0, 80.0, 100, 10.0, 200.0)
    every_setting(ops, oracle, feats, rois, 7, [4, 8])


@pytest.mark.gpu
def test_fp16(ops, oracle):
    rs = np.random.RandomState(17)
    feats = _feats(rs, 2, 8, [(32, 40), (16, 20), (8, 10)])
    rois = _rois(rs, 2, 64, 0.0, 80.0, 100, 10.0, 300.0)
    every_setting(ops, oracle, feats, rois, 7, [4, 8, 16], mode="f16")


@pytest.mark.gpu
def test_14x14(ops, oracle):
    rs = np.random.RandomState(18)
    feats = _feats(rs, 2, 8, [(32, 40), (16, 20)])
    rois = _rois(rs, 2, 40, 0.0, 80.0, 100, 10.0, 200.0)
    every_setting(ops, oracle, feats, rois, 14, [4, 8])


@pytest.mark.gpu
def test_device_staffing_against_the_restatement(ops):
    """band_staffing as the kernel runs it -- one wave, lane = unit: the register form of up to 64 units, the one of
    up to 512, and beyond them the form that walks memory -- on random (n, t); all zero where it does not apply"""
    import torch
    from simpledet_amd._lib import lib
    from simpledet_amd.ops import _p, _stream
    model = tool("fwd_schedule_model")
    rs = np.random.RandomState(19)
    cases = []
    for it in range(120):
        nvu = (1, 2, 22, 63, 64, 65, 200, 512, 513, 700)[it % 10]
        nwg = int(rs.choice([256, 250, 1024])) if nvu <= 256 else 1024
        if it % 7 == 0:
            nwg = max(1, nvu - 1)                                  # does not apply
        n, t = rs.randint(1, 70, nvu), rs.randint(1, 5000, nvu)
        if it % 5 == 1:
            n[rs.rand(nvu) < 0.3] = 0
        if it % 5 == 2:
            n[:], t[:] = n[0], t[0]
        if it % 11 == 3:
            n, t = rs.randint(1, 5000, nvu), rs.randint(1, 200000, nvu)
        cases.append((n.astype(np.int32), t.astype(np.int32), nwg))
    outs = []
    for n, t, nwg in cases:
        m = torch.full((len(n),), -7, device="cuda", dtype=torch.int32)
        tn, tt = _t(n), _t(t)
        lib().call("sd_band_staffing_dev", _p(tn), _p(tt), len(n), nwg, 1500, _p(m), _stream())
        outs.append(m)
    torch.cuda.synchronize()
    applied = 0
    for (n, t, nwg), m in zip(cases, outs):
        want = model.staffing(n, t, nwg)
        applied += want is not None
        assert m.cpu().numpy().tolist() == (want if want is not None else [0] * len(n)), (len(n), nwg)
    assert 60 <= applied < len(cases)
