"""What the entry points answer to pictures that break a rule of their source format, without a GPU: the calls of
tests/golden/make_source_messages.py (every format value -1..21 against a wrong yuv_mode, a null plane, a row stride one
element short or exactly long enough, unequal pitches, addresses off the element size; widths 16 and 17) replayed on this
build.  Return code and sjpeg_hip_last_error() must be those recorded in tests/golden/source_messages.json with the
library as it was before the formats moved into one table (sjpeg_amd/csrc/source_layout.h), byte for byte.  Every call is
one that is refused before any device work -- the generator's docstring says how that is kept so."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_source_messages", os.path.join(GOLDEN, "make_source_messages.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "source_messages.json")) as _f:
    RECORDED = json.load(_f)


def test_every_format_is_recorded():
    assert sorted(RECORDED["cases"], key=int) == [str(f) for f in gen.FORMATS] == [str(f) for f in range(-1, 22)]
    assert all(rc != 0 for rc, _ in RECORDED["answers"])


@pytest.mark.parametrize("fmt", gen.FORMATS)
def test_answers_are_the_recorded_ones(fmt):
    want = RECORDED["cases"][str(fmt)]
    n = 0
    for label, call in gen.cases(fmt):
        assert n < len(want), (fmt, label, "a case that is not recorded")
        assert gen.answer(call) == RECORDED["answers"][want[n]], (fmt, label)
        n += 1
    assert n == len(want)
