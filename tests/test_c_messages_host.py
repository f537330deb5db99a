"""What the shaped ragged entries of the C layer answer to the calls they refuse on the host, without a GPU: the calls of
tests/golden/make_c_messages.py (every fault of each of the 62 entries alone, every pair of faults one call can hold,
each on every route of its entry) replayed on this build.  Return code and sjpeg_hip_last_error() must be those recorded
in tests/golden/c_messages.json with the library of the commit before each change to the entries
(sjpeg_amd/csrc/ragged_shaped.cc), byte for byte: there is no list of excepted cases.  Every call is one
that is refused before the engine is read -- the generator's docstring says how that is kept so."""
import importlib.util
import json
import os

import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_c_messages", os.path.join(GOLDEN, "make_c_messages.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

with open(os.path.join(GOLDEN, "c_messages.json")) as _f:
    RECORDED = json.load(_f)


def test_every_entry_is_recorded_and_refused():
    assert list(RECORDED["cases"]) == list(gen.ENTRIES) and len(gen.ENTRIES) == 62
    # (a refusal: an error code -- or the 0 bytes of sjpeg_hip_compose_ragged_bytes, whose rows alone hold such answers)
    answers = gen.recorded_answers(RECORDED)
    for entry, row in RECORDED["cases"].items():
        labels = [label for label, _ in gen.cases(entry)]
        codes = {answers[i][0] for i in gen.from_numbers(labels, gen.expand(row["answers"]))}
        assert codes == ({0} if entry == gen.BYTES_ENTRY else {gen.EINVAL}), entry


@pytest.mark.parametrize("entry", list(gen.ENTRIES))
def test_labels_are_unique_and_the_recorded_ones(entry):
    labels = [label for label, _ in gen.cases(entry)]
    assert len(set(labels)) == len(labels) == RECORDED["cases"][entry]["n"]
    assert gen.digest(labels) == RECORDED["cases"][entry]["labels"]
    # at least one case per entry per route
    want = {label for label, _ in gen.routes(entry)}
    assert want and {label.split("|")[1] for label in labels} == want
    assert all(label.split("|")[0] == entry for label in labels)


@pytest.mark.parametrize("entry", list(gen.ENTRIES))
def test_answers_are_the_recorded_ones(entry):
    numbers = gen.expand(RECORDED["cases"][entry]["answers"])
    labels = [label for label, _ in gen.cases(entry)]
    assert len(labels) == len(numbers), "the cases are not the recorded ones"
    answers, want = gen.recorded_answers(RECORDED), gen.from_numbers(labels, numbers)
    for n, (label, c) in enumerate(gen.cases(entry)):
        assert gen.answer(c) == answers[want[n]], label
