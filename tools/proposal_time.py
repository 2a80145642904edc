#!/usr/bin/env python
"""Proposal_v2 timing at the TridentNet train shape: B=6 image-branches, A=15 (scales 2-32, ratios
0.5/1/2), 50x75, stride 16, pre 12000, post 500, NMS 0.7, valid ranges (0,90) / (30,160) / (90,max)
(config/tridentnet_r50v2c4_c5_2x.py:25, models/tridentnet/builder.py:239-255).

Reported (median of device events around one eager call, launch gaps included): sd_proposal_v2
with filter_scales, the same with narrow ranges (40,60) / (100,130) / (20,30) so that the cut falls
inside the run of rows filtered to -1 ("tie"), the same shape with filter_scales=False, sd_proposal_v3,
their ratios, the number of rows filtered to -1 in image 0, and the numpy restatement's host time
(tests/proposal_ref.py) for the filtered case.  NSETS input sets are rotated between calls.

    python tools/proposal_time.py [--iters 50] [--sets 4] [--no-host]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simpledet_amd import ops  # noqa: E402
from tests import proposal_ref as pr  # noqa: E402

B, A, H, W = 6, 15, 50, 75
PRE, POST = 12000, 500
KW = dict(rpn_pre_nms_top_n=PRE, rpn_post_nms_top_n=POST, threshold=0.7, rpn_min_size=0,
          scales=pr.TRIDENT["scales"], ratios=pr.TRIDENT["ratios"], feature_stride=16)


def make_sets(nsets):
    sets = []
    for k in range(nsets):
        cls, bbox, im = pr.rpn_inputs(100 + k, B, A, H, W)
        vr = np.asarray([pr.TRIDENT_RANGES[i % 3] for i in range(B)], np.float32)
        sets.append(tuple(torch.from_numpy(x).cuda() for x in (cls, bbox, im, vr)))
    return sets


def event_time(fn, sets, iters):
    """fn(set) -> outputs; eager calls timed with device events, input sets rotated."""
    for s in sets:
        fn(s)  # warm-up (kernel attributes, allocator)
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for i in range(iters):
        s = sets[i % len(sets)]
        start.record()
        fn(s)
        end.record()
        end.synchronize()
        ts.append(start.elapsed_time(end) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--sets", type=int, default=4)
    ap.add_argument("--no-host", action="store_true")
    args = ap.parse_args()
    sets = make_sets(max(2, args.sets))
    ops.lib().cdll.sd_proposal_v2_workspace_bytes.restype = ctypes.c_size_t
    wsb = int(ops.lib().cdll.sd_proposal_v2_workspace_bytes(B, A, H, W, PRE))
    ws = torch.empty(wsb, device="cuda", dtype=torch.uint8)
    res = {"op": "proposal_v2", "shape": "B=%d A=%d %dx%d stride 16 pre %d post %d" % (B, A, H, W, PRE, POST),
           "device": torch.cuda.get_device_name(0)}
    res["filtered_us"] = event_time(
        lambda s: ops.proposal_v2(s[0], s[1], s[2], s[3], filter_scales=True, workspace=ws, **KW),
        sets, args.iters)
    narrow = []
    for s in sets:
        vr = torch.tensor([[40., 60.], [100., 130.], [20., 30.]] * (B // 3), device="cuda")
        narrow.append((s[0], s[1], s[2], vr))
    res["tie_us"] = event_time(
        lambda s: ops.proposal_v2(s[0], s[1], s[2], s[3], filter_scales=True, workspace=ws, **KW),
        narrow, args.iters)
    res["unfiltered_us"] = event_time(
        lambda s: ops.proposal_v2(s[0], s[1], s[2], s[3], filter_scales=False, workspace=ws, **KW),
        sets, args.iters)
    # Proposal_v3 through its C entry point with its own preallocated workspace, like the v2 legs
    l = ops.lib().cdll
    l.sd_proposal_v3_workspace_bytes.restype = ctypes.c_size_t
    wsb3 = int(l.sd_proposal_v3_workspace_bytes(B, A, H, W, PRE))
    ws3 = torch.empty(wsb3, device="cuda", dtype=torch.uint8)
    out3 = torch.empty((B, POST, 4), device="cuda")
    sc3 = torch.empty((B, POST, 1), device="cuda")
    sc_a, ra_a = ops._farr(KW["scales"]), ops._farr(KW["ratios"])

    def v3(s):
        ops.lib().call("sd_proposal_v3", ops._p(s[0]), ops._p(s[1]), ops._p(s[2]), ops._p(out3),
                       ops._p(sc3), B, A, H, W, PRE, POST, 0.7, 0, sc_a, len(KW["scales"]), ra_a,
                       len(KW["ratios"]), 16, 1, ops._p(ws3), ctypes.c_size_t(wsb3), ops._stream())
    res["v3_us"] = event_time(v3, sets, args.iters)
    res["filtered_over_unfiltered"] = round(res["filtered_us"] / res["unfiltered_us"], 3)
    res["tie_over_unfiltered"] = round(res["tie_us"] / res["unfiltered_us"], 3)
    res["unfiltered_over_v3"] = round(res["unfiltered_us"] / res["v3_us"], 3)
    s0 = [x.cpu().numpy() for x in sets[0]]
    _, sc = pr.decode(s0[0][0], s0[1][0], s0[2][0], 16, KW["scales"], KW["ratios"], 0, False,
                      s0[3][0], True)
    res["minus_one_rows_image0"] = int((sc == -1).sum())
    n0 = [x.cpu().numpy() for x in narrow[0]]
    _, sc = pr.decode(n0[0][0], n0[1][0], n0[2][0], 16, KW["scales"], KW["ratios"], 0, False,
                      n0[3][0], True)
    res["tie_minus_one_rows_image0"] = int((sc == -1).sum())
    if not args.no_host:
        t0 = time.perf_counter()
        pr.proposal_v2(*s0, filter_scales=True, **KW)
        res["numpy_host_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    for k in ("filtered_us", "tie_us", "unfiltered_us", "v3_us"):
        res[k] = round(res[k], 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
