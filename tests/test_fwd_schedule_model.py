"""tools/fwd_schedule_model.py -- the event-driven replay of the band-resident forward's scheduler -- against the
per-workgroup clocks it was written to explain, profiles/fwd_finish_clocks.txt, for today's policy (midpoint rule,
reservations of four channels, no tail pieces), no GPU:

  * the items of every virtual unit equal the measured ones, and so do the workgroups that start on each;
  * the mean and the maximum of the modelled finish ticks lie within the margin of the measured ones: twice the
    launch-to-launch spread of the measured maximum, 2 x 3600 = 7200 ticks (the profile states it);
  * with roi_align_fwd_staff = 1 the model's staffing is the plain-integer restatement of band_staffing, which is also
    what the kernel ran (part 2 of the profile).

What the model says about staffing = 1 and the reservation knobs is printed, not asserted: how those forecasts fared
on the GPU is in the tool's --rank output, the profile and DESIGN 4.1 (the staffing forecast did not hold).
"""
import importlib.util
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def model():
    if "m" not in _CACHE:
        spec = importlib.util.spec_from_file_location("fwd_schedule_model", os.path.join(ROOT, "tools", "fwd_schedule_model.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _CACHE["m"] = mod
        _CACHE["vus"] = mod.benchmark_vus()
    return _CACHE["m"]


def replay(**kw):
    key = tuple(sorted(kw.items()))
    if key not in _CACHE:
        m = model()
        _CACHE[key] = m.replay(_CACHE["vus"], 256, **kw)
    return _CACHE[key]


def profile():
    """-> per part (0: today's rule, 1: band_staffing) dict(m, items, mean, max, spread_max)"""
    if "profile" not in _CACHE:
        text = open(os.path.join(ROOT, "profiles", "fwd_finish_clocks.txt")).read()
        parts = re.split(r"^=+ part \d.*$", text, flags=re.M)
        assert len(parts) == 3
        margin = re.search(r"= 2 x (\d+) = (\d+) ticks", parts[0])
        res = []
        for p in parts[1:]:
            m = [int(x) for x in re.search(r"workgroups that start on each virtual unit: \[([^\]]*)\]", p).group(1).split(",")]
            first = p.split("== launch 2")[0] if "== launch 2" in p else p
            items = [int(x.group(2)) for x in re.finditer(r"^  vu +(\d+)  P\d +(\d+)  m", first, flags=re.M)]
            ex = np.asarray([(float(a), float(b)) for a, b in re.findall(r"^launch \d: exit mean (\d+) max (\d+);", p, flags=re.M)])
            assert len(ex) >= 3, "at least three launches"
            res.append(dict(m=m, items=items, mean=ex[:, 0].mean(), max=ex[:, 1].mean(), spread_max=np.ptp(ex[:, 1])))
        _CACHE["profile"] = (res, int(margin.group(1)), int(margin.group(2)))
    return _CACHE["profile"]


def test_the_margin_is_twice_the_spread_of_the_measured_maximum():
    parts, spread, margin = profile()
    assert spread == parts[0]["spread_max"] == 3600 and margin == 2 * spread == 7200


def test_items_and_staffing_of_todays_policy_equal_the_measured():
    parts, _, _ = profile()
    r = replay(staff=0)
    assert len(r["items"]) == 22
    assert r["items"] == parts[0]["items"]
    assert r["m"] == parts[0]["m"] and sum(r["m"]) == 256
    assert not r["staffed"]


def test_finish_of_todays_policy_within_the_margin():
    parts, _, margin = profile()
    r = replay(staff=0)
    print("finish ticks, model / measured: mean %.0f / %.0f (%+.0f), max %.0f / %.0f (%+.0f); margin %d" % (
        r["mean"], parts[0]["mean"], r["mean"] - parts[0]["mean"], r["max"], parts[0]["max"], r["max"] - parts[0]["max"], margin))
    assert abs(r["mean"] - parts[0]["mean"]) <= margin
    assert abs(r["max"] - parts[0]["max"]) <= margin


def test_staffing_numbers_are_the_restatements_and_the_kernels():
    parts, _, _ = profile()
    m = model()
    r = replay(staff=1)
    n, t = m.unit_nt(_CACHE["vus"], 256)
    assert r["staffed"] and r["m"] == m.staffing(n, t, 256) == parts[1]["m"]
    assert r["m"] == [13, 13, 13, 13, 13, 16, 13, 11, 11, 13, 13, 11, 13, 13, 11, 11, 13, 13, 9, 7, 7, 6]
    print("model, staffing = 1: finish mean %.0f max %.0f; measured %.0f / %.0f, of which 11.7 k are the search itself" % (
        r["mean"], r["max"], parts[1]["mean"], parts[1]["max"]))
