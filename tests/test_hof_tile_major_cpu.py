"""COEVO_TASK_TILED on the host side: the task word that names a twin, and the constants lib.py mirrors from include/coevo.h."""
import os
import re

import pytest

from coevonet_amd import lib as L


def test_constants_mirror_the_header():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(here, "include", "coevo.h")).read()
    for name, value in (("COEVO_TASK_RESIDENT", L.TASK_RESIDENT), ("COEVO_TASK_TILED", L.TASK_TILED),
                        ("COEVO_TASK_TWIN_SHIFT", L.TASK_TWIN_SHIFT), ("COEVO_TASK_TWIN_UNIT", L.TASK_TWIN_UNIT)):
        assert int(re.search(rf"#define {name} (\d+)", text).group(1)) == value, name
    assert L.W2_FLOATS == 512 * 256 and L.W2_FLOATS % L.TASK_TWIN_UNIT == 0
    assert L.TASK_TILED & L.TASK_RESIDENT == 0 and L.TASK_TILED < 1 << L.TASK_TWIN_SHIFT


def test_task_word_names_the_twin_offset():
    for off in (0, L.TASK_TWIN_UNIT, 87 * L.W2_FLOATS, ((1 << 23) - 1) * L.TASK_TWIN_UNIT):
        word = L.task_tiled_flags(off)
        assert word & L.TASK_TILED and 0 < word < 1 << 31   # (coevo_fc_task.reserved is an int32)
        assert (word >> L.TASK_TWIN_SHIFT) * L.TASK_TWIN_UNIT == off
    for bad in (-L.TASK_TWIN_UNIT, 513, (1 << 23) * L.TASK_TWIN_UNIT):
        with pytest.raises(AssertionError):
            L.task_tiled_flags(bad)
