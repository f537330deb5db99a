"""Generates tests/golden/reference_answers.json from the REAL reference (oracle/_ref/libsjpeg_ref.so): its answer
to every call the live tests of test_oracle.py / test_host.py make, recorded while those tests run against it
(so every recorded answer has just been compared with the oracle / the product).  Dev container only:

    make -C oracle ref && python tests/golden/make_reference_answers.py

Data only -- size and MD5 of the reference's outputs for the tests' seeded inputs, no reference code.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)

from oracle import orc, refso  # noqa: E402
import reference_answers  # noqa: E402
import test_host  # noqa: E402
import test_oracle  # noqa: E402

LIVE_TESTS = [getattr(test_oracle, n) for n in dir(test_oracle) if n.startswith("test_live_")] + \
             [test_host.test_live_jpeg_tools_vs_reference]


def main():
    if not refso.available():
        raise SystemExit("oracle/_ref/libsjpeg_ref.so is not built (make -C oracle ref)")
    rec = reference_answers.Recorder(refso.ref())
    o = orc.oracle()
    for t in LIVE_TESTS:
        if t is test_host.test_live_jpeg_tools_vs_reference:
            t(rec, None)
        else:
            t(o, rec)
        print("recorded", t.__name__)
    rec.save()
    print(f"{len(rec.answers)} answers -> {reference_answers.PATH} ({os.path.getsize(reference_answers.PATH)} bytes)")


if __name__ == "__main__":
    main()
