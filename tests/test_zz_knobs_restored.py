"""Leak detector for the kernel-variant knobs (CPU only).

Every knob must read its golden default (tests/golden/tuning_defaults.json).  Alone this passes trivially.  Pytest
collects the files of a directory in name order and this one sorts last, so at the end of a full session it fails
if any test before it left a knob changed -- which would have run every later test on a variant that is not
shipped, and left the shipped path untested, without failing anything else.  Tests change knobs with
`with lib().tuned(...)`, which puts the previous values back."""
import json
import os

from simpledet_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_knob_reads_its_default():
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "tuning_defaults.json")))
    l = _lib.lib()
    assert {k: l.get_tuning(k) for k in l.tuning_keys()} == golden
