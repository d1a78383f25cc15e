#!/usr/bin/env python3
"""Record gik_template_get_info and one solve per build word of the fixed-anchor solve, for
tests/test_anchored_build_words_gpu.py (a recording tool; needs the MI355X).

    python tools/anchored_build_words.py --commit <hash of the checkout> [--out tests/golden/anchored_build_words_parent.json]

Runs the state table of the test module -- imported from there, so the tool and the test cannot drift -- on the checkout
it stands in, and writes per state the template's whole info dict and the solve's points as int64 bit patterns, next to
the commit's hash and the library's source digest.  To record a parent commit, copy this file and the test module into
a scratch checkout of it and run it there.

Every state runs twice and has to give the same record.  The file is refused (exit status 1, nothing written) if a
state reports another `anchored` word than its table entry names, or if no goal of a state took an iteration."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--commit", required=True, help="hash of the commit this checkout holds")
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "anchored_build_words_parent.json"))
    a = p.parse_args()
    import torch
    import test_anchored_build_words_gpu as table
    from graphik_amd import build
    assert torch.cuda.is_available(), "recording needs the MI355X"
    states, refused = {}, []
    for name, (_, word) in table.STATES.items():
        rec = table.run(name)
        if table.run(name) != rec:
            refused.append(name + ": two runs differ")
        if rec["info"]["anchored"] != word:
            refused.append(f"{name}: anchored = {rec['info']['anchored']}, the table says {word}")
        if max(rec["iterations"]) < 1:
            refused.append(name + ": no goal took an iteration")
        print(name, rec["info"], "iterations", rec["iterations"], flush=True)
        states[name] = rec
    if refused:
        print("refused:\n  " + "\n  ".join(refused))
        return 1
    doc = {"library": "parent commit " + a.commit, "library_source_digest": build.source_digest(), "states": states}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
