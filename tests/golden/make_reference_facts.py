"""Generates tests/golden/reference_facts.json: what tests/test_integration_shim.py needs to know about the reference's
C# sources, so that the test runs without a checkout of the reference.

Recorded per entry of the test's tables: whether each declaration pattern of REF_DECLS matches its file, the 1-based
lines of each call-site text of REF_CALL_SITES, and a sha256 digest of the Console.Write* literals of each method of
CONSOLE_REF.  Names, line numbers and digests only: no source text of the reference is written.
Run from the repo root:  python tests/golden/make_reference_facts.py <reference checkout>/src
"""
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import test_integration_shim as T  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))


def main(src):
    def text(rel):
        return open(os.path.join(src, rel), encoding="utf-8-sig").read()
    facts = {"declarations": {}, "call_sites": {}, "console_literals_sha256": {}}
    for rel, pat in T.REF_DECLS:
        facts["declarations"][T.ref_key(rel, pat)] = bool(re.search(pat, text(rel)))
    for rel, snippet, _ in T.REF_CALL_SITES:
        facts["call_sites"][T.ref_key(rel, snippet)] = [i + 1 for i, ln in enumerate(text(rel).split("\n")) if snippet in ln]
    fun = T._strip_c_comments(text(os.path.join("STAN_Solver", "SolverFunctions.cs")))
    for name in T.CONSOLE_REF:
        facts["console_literals_sha256"][name] = T.literals_digest(T._console_literals(T._method_body(fun, name)))
    out = os.path.join(HERE, "reference_facts.json")
    with open(out, "w") as f:
        json.dump(facts, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
