#!/usr/bin/env python3
"""Record what the host entry points refuse, for tests/test_anchored_refusals_gpu.py and tests/test_retry_refusals_gpu.py
(a recording tool; needs the MI355X).

    python tools/record_refusals.py --commit <hash of the checkout> [--table anchored|retry] [--out FILE]

Runs the table of calls of the test module -- imported from there, so the tool and the test cannot drift -- on the
checkout it stands in, and writes per case the return code and the full text of gik_last_error() to
tests/golden/<table>_refusals_parent.json.  To record a parent commit, copy this file, the test module(s) and
tests/test_ws_layouts.py into a scratch checkout of it and run it there.

The table runs twice and has to give the same answers.  The file is refused (exit status 1, nothing written) if a case
did not do what its kind says: a refused call that returned 0 or left no message, a size that is not 0, a call that is
meant to run and did not return 0."""
import argparse
import importlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--commit", required=True, help="hash of the commit this checkout holds")
    p.add_argument("--table", choices=["anchored", "retry"], default="anchored")
    p.add_argument("--out", help="default: tests/golden/<table>_refusals_parent.json")
    a = p.parse_args()
    out = a.out or os.path.join(REPO, "tests", "golden", a.table + "_refusals_parent.json")
    table = importlib.import_module(f"test_{a.table}_refusals_gpu")
    from graphik_amd import build
    cases = table.cases()
    got = table.run(cases)
    refused = [name + ": two runs differ" for name, rec in table.run(cases).items() if rec != got[name]]
    for name, (kind, _) in cases.items():
        rec = got[name]
        if rec["rc"] != (-1 if kind == "call" else 0) or not rec["message"]:
            refused.append(f"{name}: not what a '{kind}' case does ({rec})")
    exports = sorted({name.split(":")[0] for name in cases})
    print(len(cases), "cases of", len(exports), "exports")
    if refused:
        print("refused:\n  " + "\n  ".join(refused))
        return 1
    doc = {"library": "parent commit " + a.commit, "library_source_digest": build.source_digest(), "exports": exports, "cases": got}
    with open(out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
