#!/usr/bin/env python
"""Run pytest with kernel-variant knobs set first: tools/pytest_tuned.py key=value [key=value ...] -- <pytest args>
The tests' `tuned()` blocks return to these values, not to the defaults, so the setting holds for the whole session;
tests/test_zz_knobs_restored.py compares against the defaults and fails under it by design (--deselect it)."""
import sys

import pytest

sys.path.insert(0, ".")
from simpledet_amd._lib import lib  # noqa: E402

i = sys.argv.index("--")
for kv in sys.argv[1:i]:
    k, v = kv.split("=")
    lib().set_tuning(k, int(v))
sys.exit(pytest.main(sys.argv[i + 1:]))
