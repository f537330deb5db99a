"""Host-only (no GPU): what the Python binding answers to calls that break one of its argument rules, and the signatures of
its public names.  The table of tests/golden/make_python_messages.py -- every public call against a bad layout, an empty
list, pictures that are no CUDA tensor or of the wrong dtype, rank, channel count or strides, every wrapper where it is
refused and every ordered pair of nested wrappers, wrong lengths of the per-picture arguments, the targets, methods and
modes out of range, two faults at once, and the Engine methods' own length checks -- is replayed on this build.  The
exception's class and full text must be those recorded in tests/golden/python_messages.json with the binding as it was
before its entries were made to share one reader, one unwrap and launch step and one call builder, byte for byte.  The
one entry that may differ is named below with the answer it has now."""
import importlib.util
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_python_messages", os.path.join(GOLDEN, "make_python_messages.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

RECORDED = dict(zip(("cases", "signatures"), gen.recorded()))      # (it checks that the table is the recorded one)

# riskiness_images(layout="hwc") handed pictures on two devices to one engine; it now refuses them as the other calls do
CHANGED = {"riskiness_images|hwc|second_device": "SjpegError: riskiness_images: image 1 is on cuda:1, image 0 on cpu"}


def test_every_case_is_recorded():
    labels = [label for label, _, _ in gen.cases()]
    assert len(labels) == len(set(labels))
    assert labels == list(RECORDED["cases"]), "the table and tests/golden/python_messages.json list different cases"
    assert len(labels) > 1500


def test_answers_are_the_recorded_ones():
    wrong = []
    for label, call, guarded in gen.cases():
        got, want = gen.answer(call, guarded), CHANGED.get(label, RECORDED["cases"][label])
        if got != want:
            wrong.append((label, got, want))
    assert not wrong, "%d answers differ, the first: %r" % (len(wrong), wrong[:5])


def test_the_changed_answer_was_another():
    for label in CHANGED:
        assert RECORDED["cases"][label].startswith("ReachedEngine"), label


def test_no_recorded_case_ran_an_engine_method_to_the_library():
    """every Engine case is one of the binding's own refusals"""
    for label, want in RECORDED["cases"].items():
        if label.startswith("Engine."):
            assert want.startswith("SjpegError: "), (label, want)


def test_signatures():
    got = gen.signatures()
    assert list(got) == list(RECORDED["signatures"])
    wrong = [(k, got[k], v) for k, v in RECORDED["signatures"].items() if got[k] != v]
    assert not wrong, wrong
    for name in ("encode_images", "Engine.encode_ragged_full", "Engine.encode_ragged_sheet_packed", "Flattened.fit", "Reduced"):
        assert name in got
