#!/usr/bin/env python3
"""Record what the anchored host entry points refuse, for tests/test_anchored_refusals_gpu.py (a recording tool; needs the
MI355X).

    python tools/record_refusals.py --commit <hash of the checkout> [--out tests/golden/anchored_refusals_parent.json]

Runs the table of refused calls of tests/test_anchored_refusals_gpu.py -- imported from there, so the tool and the test
cannot drift -- on the checkout it stands in, and writes per case the return code and the full text of gik_last_error().
To record a parent commit, copy this file, the test module and tests/test_ws_layouts.py into a scratch checkout of it and
run it there.

The table runs twice and has to give the same answers.  The file is refused (exit status 1, nothing written) if a case
was not refused: a call that returned 0 or left no message, a size that is not 0."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--commit", required=True, help="hash of the commit this checkout holds")
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "anchored_refusals_parent.json"))
    a = p.parse_args()
    import test_anchored_refusals_gpu as table
    from graphik_amd import build
    cases = table.cases()
    got = table.run(cases)
    refused = [name + ": two runs differ" for name, rec in table.run(cases).items() if rec != got[name]]
    for name, (kind, _) in cases.items():
        rec = got[name]
        if rec["rc"] != (0 if kind == "size" else -1) or not rec["message"]:
            refused.append(f"{name}: not refused ({rec})")
    exports = sorted({name.split(":")[0] for name in cases})
    print(len(cases), "cases of", len(exports), "exports")
    if refused:
        print("refused:\n  " + "\n  ".join(refused))
        return 1
    doc = {"library": "parent commit " + a.commit, "library_source_digest": build.source_digest(), "exports": exports, "cases": got}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
