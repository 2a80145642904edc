#!/usr/bin/env python
"""CPU model (numpy, no GPU) of WHEN the persistent workgroups of the band-resident RoIAlign forward finish, on the
benchmark's inputs: an event-driven replay of the kernel's scheduler on top of the plan, the item lists and the table
of virtual units that tools/fwd_traffic_model.py restates (imported, not copied).

  staffing       which virtual unit each of the 256 workgroups starts on: the midpoint rule (roi_align_fwd_staff = 0:
                 where the midpoint of its share of the cost prefix falls) or band_staffing (= 1, restated here as
                 `staffing`: the smallest T with sum_v ceil(n_v / floor((T - setup) / t_v)) <= nwg, spare workgroups one
                 at a time to the unit that finishes last)
  reservations   a workgroup takes a unit's channels from the unit's counter GR at a time, one reservation parked while
                 the current one is worked on; the last `tail` per cent of a unit in pieces of `tail_planes` planes
  moving on      a workgroup whose unit has run dry joins the unit with the most estimated work left, if that unit is
                 untouched or has >= 3 G channels left, and pays a set-up there; otherwise it is done
  cost           fill = k * (F0 + G * (F1 + items)) ticks, set-up S ticks per visit, HEAD ticks before the first visit,
                 EXIT ticks after the last (exact path, tail tasks): the refit of profiles/fwd_finish_clocks.txt

Output: the finish tick of every workgroup, their mean and maximum.

    python tools/fwd_schedule_model.py [--staff 0|1] [--grab N] [--tail PCT] [--tail-planes N] [--rank]
"""
import argparse
import heapq
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _traffic():
    spec = importlib.util.spec_from_file_location("fwd_traffic_model", os.path.join(ROOT, "tools", "fwd_traffic_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


T = _traffic()
band_plan, fpn_level, axis_samples, unit_order, xcd_slot, virtual_units = (
    T.band_plan, T.fpn_level, T.axis_samples, T.unit_order, T.xcd_slot, T.virtual_units)
NWG = T.NWG

# profiles/fwd_finish_clocks.txt (ticks): the refit of a visit, visit = S + fills * k * (F0 + G * (F1 + items)), the mean
# head in front of the first visit and the mean time between the end of the band work and the exit (exact path, tail
# tasks); LOOK, the search for the next unit, is not measured (no workgroup moves on at the benchmark's shape)
FIT = dict(k=10.45, F0=158.0, F1=18.0, S=18214.0, HEAD=9235.0, EXIT=11470.0, LOOK=1500.0)


# ---------------------------------------------------------------------------------------------- staffing
def need(n, t, D):
    return 0 if n <= 0 else -(-n // (D // t))


def staffing(n, t, nwg):
    """band_staffing (roi_align_common.h) in plain integers -> workgroups per unit, or None where the rule does not
    apply (more units than workgroups, no work, products past 2^30)"""
    n, t = [int(x) for x in n], [int(x) for x in t]
    nvu = len(n)
    live = [v for v in range(nvu) if n[v] > 0]
    if nvu <= 0 or nvu > nwg or nvu > (1 << 20) or not live:
        return None
    if any(t[v] <= 0 or n[v] * t[v] > (1 << 30) for v in live):
        return None
    lo, hi = max(t[v] for v in live), max(n[v] * t[v] for v in live)
    while lo < hi:
        mid = lo + (hi - lo) // 2
        if sum(need(n[v], t[v], mid) for v in range(nvu)) <= nwg:
            hi = mid
        else:
            lo = mid + 1
    m = [need(n[v], t[v], lo) for v in range(nvu)]
    spare = nwg - sum(m)
    while spare > 0:
        fin = [(-(-n[v] // m[v]) * t[v], -v) for v in live]
        v = -max(fin)[1]
        give = spare if m[v] >= n[v] else 1
        m[v] += give
        spare -= give
    return m


def makespan(n, t, m):
    """the latest finish, in cost units, of units staffed with m workgroups (inf where a unit with work has none)"""
    return max((float("inf") if m[v] <= 0 else -(-int(n[v]) // int(m[v])) * int(t[v])) for v in range(len(n)) if n[v] > 0)


def midpoint_starts(cost, nwg, xcd=1):
    """start unit of every workgroup by the kernel's midpoint rule on the prefix of `cost`"""
    start = np.concatenate([[0], np.cumsum(np.asarray(cost, np.int64))])
    out = []
    for wg in range(nwg):
        share = xcd_slot(wg, nwg) if xcd >= 1 else wg
        pos = int(start[-1]) * (2 * share + 1) // (2 * nwg)
        out.append(max(int((start[:-1] <= pos).sum()) - 1, 0))
    return out


def staffed_starts(m, nwg, xcd=1):
    pre = np.concatenate([[0], np.cumsum(m)])
    out = []
    for wg in range(nwg):
        share = xcd_slot(wg, nwg) if xcd >= 1 else wg
        out.append(max(int((pre[:-1] <= share).sum()) - 1, 0))
    return out


def unit_nt(vus, C, grab=T.GRAB):
    """the kernel's n_v (reservations) and t_v (cost units of one reservation) of every virtual unit"""
    n, t = [], []
    for v in vus:
        g = v["unit"]["g"]
        gr = -(-grab // g) * g
        n.append(-(-C // gr))
        t.append(gr * (T.FILL_COST // g + T.PLANE_COST + v["items"]))
    return n, t


# ---------------------------------------------------------------------------------------------- replay
def replay(vus, C, staff=0, grab=T.GRAB, tail=0, tail_planes=8, xcd=1, nwg=NWG, fit=FIT):
    """event-driven replay -> dict(finish=ticks per workgroup, mean, max, m=workgroups starting on each unit, visits)"""
    nvu = len(vus)
    G = [v["unit"]["g"] for v in vus]
    items = [v["items"] for v in vus]
    vcost = [T.FILL_COST // G[v] + T.PLANE_COST + items[v] for v in range(nvu)]
    n, t = unit_nt(vus, C, grab)
    m = staffing(n, t, nwg) if staff == 1 else None
    if m is not None:
        starts = staffed_starts(m, nwg, xcd)
    else:
        starts = midpoint_starts([T.SETUP_COST + vcost[v] * C for v in range(nvu)], nwg, xcd)
    ctr = [0] * nvu

    def fill_ticks(v, planes):
        return fit["k"] * (fit["F0"] + planes * (fit["F1"] + items[v]))

    def take(v, last):
        """one reservation from unit v's counter -> (first channel, channels); last = first channel of the previous one"""
        gr = -(-grab // G[v]) * G[v]
        size = min(tail_planes, G[v]) if last >= C - C * tail // 100 else gr
        k = ctr[v]
        ctr[v] += size
        return k, size

    def res_ticks(v, k, size):
        """time to work through channels [k, k + size) of unit v, clipped at C, in fills of G planes"""
        end = min(k + size, C)
        tot, c = 0.0, k
        while c < end:
            p = min(G[v], end - c)
            tot += fill_ticks(v, p)
            c += p
        return tot

    # events: (time, seq, wg, kind); state per workgroup
    finish = [0.0] * nwg
    visits = [0] * nwg
    ev = []
    seq = 0
    for wg in range(nwg):
        heapq.heappush(ev, (fit["HEAD"], seq, wg, "visit", starts[wg]))
        seq += 1
    parked = {}
    cur_unit = {}
    last_k = {}
    while ev:
        now, _, wg, kind, arg = heapq.heappop(ev)
        if kind == "visit":
            v = arg
            k, size = take(v, 0)
            last_k[wg] = k
            if k >= C:
                heapq.heappush(ev, (now, seq, wg, "look", None)); seq += 1
                continue
            visits[wg] += 1
            cur_unit[wg] = v
            # the tables are set up, the first fill lands, then the next reservation is parked
            k2, s2 = take(v, last_k[wg])
            last_k[wg] = k2
            parked[wg] = (k2, s2)
            heapq.heappush(ev, (now + fit["S"] + res_ticks(v, k, size), seq, wg, "next", None)); seq += 1
        elif kind == "next":
            v = cur_unit[wg]
            k, size = parked[wg]
            if k >= C:
                heapq.heappush(ev, (now, seq, wg, "look", None)); seq += 1
                continue
            k2, s2 = take(v, last_k[wg])
            last_k[wg] = k2
            parked[wg] = (k2, s2)
            heapq.heappush(ev, (now + res_ticks(v, k, size), seq, wg, "next", None)); seq += 1
        else:   # look for the unit with the most estimated work left
            best, bestval = -1, 0
            for v in range(nvu):
                done = ctr[v]
                if done < C and (done == 0 or C - done >= 3 * G[v]):
                    left = max((C - done) * vcost[v], 1)
                    if left > bestval:
                        best, bestval = v, left
            if best < 0:
                finish[wg] = now + fit["EXIT"]
            else:
                heapq.heappush(ev, (now + fit["LOOK"], seq, wg, "visit", best)); seq += 1
    f = np.asarray(finish)
    mcount = np.bincount(starts, minlength=nvu).tolist()
    return dict(finish=f, mean=float(f.mean()), max=float(f.max()), m=mcount, staffed=m is not None, visits=visits, n=n, t=t,
                items=items, G=G)


def benchmark_vus(C=256, xcd=1):
    rois, shapes, strides = T.benchmark_inputs()
    vus, _ = virtual_units(rois, shapes, strides, C, xcd=xcd)
    return vus


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--staff", type=int, default=0, choices=(0, 1))
    ap.add_argument("--grab", type=int, default=T.GRAB)
    ap.add_argument("--tail", type=int, default=0)
    ap.add_argument("--tail-planes", type=int, default=8)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--rank", action="store_true", help="rank a few reservation settings on top of --staff 1")
    a = ap.parse_args()
    vus = benchmark_vus(a.channels)
    if a.rank:
        rows = []
        for staff in (0, 1):
            for grab in (4, 8, 2, 1):
                for tail, planes in ((0, 8), (10, 8), (20, 8), (10, 4), (20, 4), (20, 2), (20, 1)):
                    r = replay(vus, a.channels, staff, grab, tail, planes)
                    rows.append((r["max"], r["mean"], staff, grab, tail, planes))
        for mx, mean, staff, grab, tail, planes in sorted(rows):
            print("staff %d grab %d tail %2d %% planes %d: finish mean %.0f max %.0f (max / mean %.3f)" % (
                staff, grab, tail, planes, mean, mx, mx / mean))
        return
    r = replay(vus, a.channels, a.staff, a.grab, a.tail, a.tail_planes)
    print("staff %d grab %d tail %d %% in pieces of %d planes: %d virtual units, staffed by band_staffing: %s" % (
        a.staff, a.grab, a.tail, a.tail_planes, len(vus), r["staffed"]))
    print("  items per unit     ", r["items"])
    print("  workgroups starting", r["m"])
    print("  finish ticks: mean %.0f max %.0f (max / mean %.3f)" % (r["mean"], r["max"], r["max"] / r["mean"]))


if __name__ == "__main__":
    main()
