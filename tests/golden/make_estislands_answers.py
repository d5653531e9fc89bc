"""Generates tests/golden/ref_answers/tclap_estislands.json: what the reference's command-line library (TCLAP, driven by
oracle/tclap_ref.cpp, built by oracle/Makefile into oracle/_ref/tclap_ref where the reference's headers are present) prints and
returns for the estislands argument definitions (tools/estislands.cpp:27-30) on the command lines of tests/test_estislands.py.
Run it where that driver was built, after `make -C oracle`; the JSON is what travels.  It records a digest of the definitions
and command lines it was made from, which the tests check.

    python tests/golden/make_estislands_answers.py"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_estislands as te  # noqa: E402


def main():
    driver = os.path.join(ROOT, "oracle", "_ref", "tclap_ref")
    assert os.path.exists(driver), "oracle/_ref/tclap_ref is not built"
    message, spec = te.SPEC
    head = [driver, "estislands", message, str(len(spec))]
    for (flag, name, desc, typ, req) in spec:
        head += [flag, name, desc, typ, str(req)]
    answers = []
    for args in te.FAILING_LINES + te.PARSED_LINES:
        r = subprocess.run(head + ["--"] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        answers.append({"args": args, "returncode": r.returncode, "stdout": r.stdout, "stderr": r.stderr})
    out = os.path.join(HERE, "ref_answers", "tclap_estislands.json")
    with open(out, "w") as f:
        json.dump({"specs_sha256": te.specs_digest(), "answers": answers}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
