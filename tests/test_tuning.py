"""CPU-only checks of the kernel-variant knobs: the library's one list (SD_KNOBS, simpledet_amd/csrc/common.h)
against tests/golden/tuning_defaults.json, sd_set_tuning / sd_get_tuning / sd_tuning_key, and _Lib.tuned().
The knob entry points launch nothing, so none of this needs a device."""
import json
import os
import subprocess
import sys

import pytest

from simpledet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "tuning_defaults.json")))
A, B = "roi_align_bwd", "soft_nms_threads"      # two knobs whose defaults are neither 0 nor 1


def test_a_fresh_process_lists_the_golden_knobs_at_their_golden_defaults():
    """in a child process, so that nothing this session has set can show: the keys of sd_tuning_key are the golden
    keys, and every knob reads its golden default before anyone has set it"""
    code = ("import json; from simpledet_amd._lib import lib; l = lib(); "
            "print(json.dumps({k: l.get_tuning(k) for k in l.tuning_keys()}))")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert set(got) - set(GOLDEN) == set() and set(GOLDEN) - set(got) == set()
    assert got == GOLDEN


def test_the_key_list_ends_with_null():
    l = _lib.lib()
    keys = l.tuning_keys()
    assert len(keys) == len(set(keys)) == len(GOLDEN)
    key_at = l.entry("sd_tuning_key")
    assert key_at((len(keys),)) is None and key_at((-1,)) is None and key_at((1 << 30,)) is None


def test_set_then_get_round_trips():
    l = _lib.lib()
    before = l.get_tuning(B)
    try:
        for v in (64, -7, 2 ** 31 - 1, before):      # any integer is accepted; a launcher's read clamps
            l.set_tuning(B, v)
            assert l.get_tuning(B) == v
    finally:
        l.set_tuning(B, before)
    with pytest.raises(_lib.SimpleDetOpsError, match="unknown tuning key"):
        l.get_tuning("no_such_knob")


def test_tuned_restores_on_normal_exit_and_on_an_exception():
    l = _lib.lib()
    a, b = l.get_tuning(A), l.get_tuning(B)
    with l.tuned(**{A: a + 5, B: b + 5}):
        assert (l.get_tuning(A), l.get_tuning(B)) == (a + 5, b + 5)
    assert (l.get_tuning(A), l.get_tuning(B)) == (a, b)
    with pytest.raises(ZeroDivisionError):
        with l.tuned(**{A: a + 6}):
            assert l.get_tuning(A) == a + 6
            1 / 0
    assert l.get_tuning(A) == a


def test_tuned_nests_on_one_key():
    l = _lib.lib()
    a = l.get_tuning(A)
    with l.tuned(**{A: a + 1}):
        with l.tuned(**{A: a + 2}):
            assert l.get_tuning(A) == a + 2
        assert l.get_tuning(A) == a + 1              # the inner exit gives the outer value back
    assert l.get_tuning(A) == a


def test_tuned_with_an_unknown_key_changes_nothing():
    l = _lib.lib()
    a = l.get_tuning(A)
    entered = False
    with pytest.raises(_lib.SimpleDetOpsError, match="unknown tuning key"):
        with l.tuned(**{A: a + 3, "no_such_knob": 1}):
            entered = True
    assert not entered and l.get_tuning(A) == a
