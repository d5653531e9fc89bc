"""Generates tests/golden/ref_answers/tclap_matealign.json: what the reference's command-line library (TCLAP, driven by
oracle/tclap_ref.cpp, built by oracle/Makefile into oracle/_ref/tclap_ref where the reference's headers are present) prints and
returns for the matealign argument definitions (tools/matealign.cpp:51-58) on the command lines of tests/test_matealign.py.
Run it where that driver was built, after `make -C oracle`; the JSON is what travels.  It records a digest of the definitions
and command lines it was made from, which the tests check.

    python tests/golden/make_matealign_answers.py"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from tests import test_matealign as tm  # noqa: E402


def main():
    driver = os.path.join(ROOT, "oracle", "_ref", "tclap_ref")
    assert os.path.exists(driver), "oracle/_ref/tclap_ref is not built"
    message, spec = tm.SPEC
    head = [driver, "matealign", message, str(len(spec))]
    for (flag, name, desc, typ, req) in spec:
        head += [flag, name, desc, typ, str(req)]
    answers = []
    for args in tm.FAILING_LINES + tm.PARSED_LINES:
        r = subprocess.run(head + ["--"] + args, capture_output=True, text=True, stdin=subprocess.DEVNULL)
        answers.append({"args": args, "returncode": r.returncode, "stdout": r.stdout, "stderr": r.stderr})
    out = os.path.join(HERE, "ref_answers", "tclap_matealign.json")
    with open(out, "w") as f:
        json.dump({"specs_sha256": tm.specs_digest(), "answers": answers}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
