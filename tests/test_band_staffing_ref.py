"""sd_band_staffing_ref -- the host form of band_staffing (roi_align_common.h), the rule by which the band-resident
forward staffs its virtual units with whole workgroups under roi_align_fwd_staff = 1 -- against the plain-integer
restatement in tools/fwd_schedule_model.py, and its properties on random inputs (no GPU):

  * sum m = nwg;
  * m_v >= 1 for every unit with work (the rule only applies when nvu <= nwg);
  * the makespan max_v ceil(n_v / m_v) t_v is never above the midpoint rule's (workgroup slot s starts where
    (2 s + 1) / (2 nwg) of the prefix of n_v t_v falls; a unit with work that gets no workgroup there never ends);
  * the makespan is the least any staffing with sum m <= nwg reaches (brute force on small inputs);
  * m is all zero exactly where the restatement says the rule does not apply.
"""
import ctypes
import importlib.util
import itertools
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def model():
    if "m" not in _CACHE:
        spec = importlib.util.spec_from_file_location("fwd_schedule_model", os.path.join(ROOT, "tools", "fwd_schedule_model.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _CACHE["m"] = mod
    return _CACHE["m"]


def ref(n, t, nwg, setup=1500):
    from simpledet_amd._lib import lib
    n, t = np.ascontiguousarray(n, np.int32), np.ascontiguousarray(t, np.int32)
    m = np.full(len(n), -7, np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    lib().call("sd_band_staffing_ref", p(n), p(t), len(n), nwg, setup, p(m))
    return m.tolist()


def random_cases(seed, count):
    """(n, t, nwg): the kernel's ranges (a few dozen units, up to 64 reservations of a few thousand cost units, 256
    workgroups), then few workgroups, units without work, equal units, and products near the 2^30 limit"""
    rs = np.random.RandomState(seed)
    for it in range(count):
        kind = it % 6
        nvu = int(rs.randint(1, 48))
        nwg = int(rs.choice([256, 250, 64, 48, 300]))
        n = rs.randint(1, 70, nvu)
        t = rs.randint(1, 5000, nvu)
        if kind == 1:
            n[rs.rand(nvu) < 0.3] = 0
        elif kind == 2:
            t[:] = t[0]
            n[:] = n[0]
        elif kind == 3:
            n, t = rs.randint(1, 5000, nvu), rs.randint(1, 200000, nvu)
        elif kind == 4:
            nwg = int(rs.randint(1, nvu + 3))
        elif kind == 5:
            n, t = rs.randint(1, 4, nvu), rs.randint(1, 40, nvu)
        yield n.astype(np.int64), t.astype(np.int64), nwg


def midpoint_m(n, t, nwg):
    cost = n * t
    starts = model().midpoint_starts(cost, nwg, xcd=0)
    return np.bincount(starts, minlength=len(n))


def test_against_the_numpy_restatement():
    applied = fallback = 0
    for n, t, nwg in random_cases(0, 6000):
        want = model().staffing(n, t, nwg)
        got = ref(n, t, nwg)
        if want is None:
            fallback += 1
            assert got == [0] * len(n), (n, t, nwg, got)
        else:
            applied += 1
            assert got == want, (n.tolist(), t.tolist(), nwg, got, want)
    print("rule applied %d times, not applicable %d times" % (applied, fallback))
    assert applied > 3000 and fallback > 300


def test_setup_leaves_the_staffing_as_it_is():
    for n, t, nwg in itertools.islice(random_cases(1, 200), 200):
        assert ref(n, t, nwg, 0) == ref(n, t, nwg, 1500) == ref(n, t, nwg, 100000)


def test_properties():
    checked = 0
    for n, t, nwg in random_cases(2, 6000):
        m = np.asarray(ref(n, t, nwg))
        if len(n) > nwg or not (n > 0).any() or (n * t).max() > 1 << 30:
            assert not m.any()
            continue
        checked += 1
        assert m.sum() == nwg, (n, t, nwg, m)
        assert (m[n > 0] >= 1).all(), (n, t, nwg, m)
        ours, theirs = model().makespan(n, t, m), model().makespan(n, t, midpoint_m(n, t, nwg))
        assert ours <= theirs, (n.tolist(), t.tolist(), nwg, m.tolist(), ours, theirs)
    assert checked > 3000


def test_the_makespan_is_the_least_there_is():
    """every staffing of up to four units with up to nine workgroups, by brute force"""
    rs = np.random.RandomState(3)
    for _ in range(300):
        nvu = int(rs.randint(1, 5))
        nwg = int(rs.randint(nvu, 10))
        n, t = rs.randint(1, 12, nvu).astype(np.int64), rs.randint(1, 30, nvu).astype(np.int64)
        m = ref(n, t, nwg)
        best = min(model().makespan(n, t, c) for c in itertools.product(range(1, nwg + 1), repeat=nvu) if sum(c) <= nwg)
        assert model().makespan(n, t, m) == best, (n, t, nwg, m, best)


def test_the_benchmarks_units():
    """the benchmark's 22 units (profiles/fwd_finish_clocks.txt): the rule gives 13 13 13 13 13 16 13 11 11 13 13 11
    13 13 11 11 13 13 9 7 7 6, eight per cent under the midpoint rule's makespan in cost units"""
    vus = model().benchmark_vus()
    n, t = model().unit_nt(vus, 256)
    m = ref(n, t, 256)
    assert m == [13, 13, 13, 13, 13, 16, 13, 11, 11, 13, 13, 11, 13, 13, 11, 11, 13, 13, 9, 7, 7, 6]
    n, t = np.asarray(n), np.asarray(t)
    mid = np.bincount(model().midpoint_starts([1500 + x for x in (n * t).tolist()], 256, xcd=1), minlength=len(n))
    a, b = model().makespan(n, t, m), model().makespan(n, t, mid)
    print("makespan in cost units: staffed %d, midpoint %d (%.1f %%)" % (a, b, 100.0 * (a / b - 1)))
    assert a < 0.93 * b


def test_argument_checks():
    from simpledet_amd import _lib
    with pytest.raises(_lib.SimpleDetOpsError, match="null pointer"):
        _lib.lib().call("sd_band_staffing_ref", None, None, 3, 8, 0, None)
    assert _lib.lib().call("sd_band_staffing_ref", None, None, 0, 8, 0, None) == 0
