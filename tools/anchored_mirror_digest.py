#!/usr/bin/env python3
"""Record what the numpy mirrors of the fixed-anchor pair geometry return, for tests/test_anchored_mirrors_parent.py
(a recording tool; CPU only, host-only problems).

    python tools/anchored_mirror_digest.py --commit <hash of the checkout> [--out tests/golden/anchored_mirrors_parent.json]

Runs the table of tests/test_anchored_mirrors_parent.py -- imported from there, so the tool and the test cannot drift --
on the checkout it stands in, and writes per entry the sha256 (over dtype, shape and bytes) of every returned array by
key, next to the commit's hash.  To record a parent commit, copy this file and the test module into a scratch checkout
of it and run it there.

Every entry runs twice and has to give the same hashes.  The file is refused (exit status 1, nothing written) if a
clearance entry holds no finite value or a hinge entry no active hinge: change that entry's seed in the table, not the
condition."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--commit", required=True, help="hash of the commit this checkout holds")
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "anchored_mirrors_parent.json"))
    a = p.parse_args()
    import test_anchored_mirrors_parent as table
    entries, refused = {}, []
    for name, run in table.ENTRIES.items():
        arrays = run()
        rec = {"sha": table.digest(arrays), "conditions": table.conditions(name, arrays)}
        if table.digest(run()) != rec["sha"]:
            refused.append(name + ": two runs differ")
        refused += [f"{name}: {key} == 0" for key, count in rec["conditions"].items() if count == 0]
        print(name, len(rec["sha"]), "keys", rec["conditions"], flush=True)
        entries[name] = rec
    if refused:
        print("refused:\n  " + "\n  ".join(refused))
        return 1
    doc = {"library": "parent commit " + a.commit,
           "hash": "sha256 over (dtype, shape) and the bytes of every returned array, by key", "entries": entries}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
