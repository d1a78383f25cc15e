#!/usr/bin/env python3
"""Record what the Python layer returns, for tests/test_python_layer_parity_gpu.py (a recording tool; needs the MI355X).

    python tools/python_layer_digest.py --commit <hash of the checkout> [--out tests/golden/python_layer_parent.json]

Runs the scenario table of tests/test_python_layer_parity_gpu.py -- the table is imported from there, so the tool and
the test cannot drift -- on the checkout it stands in, and writes per scenario the sha256 (over dtype, shape and
bytes) of every returned array by key, next to the commit's hash and the library's source digest.  To record a parent
commit, copy this file and the test module into a scratch checkout of it and run it there.

Every scenario runs twice and has to give the same hashes.  The file is refused (exit status 1, nothing written) if
a restart scenario improved no goal or a clearance scenario returned no finite clearance: change that scenario's seed
or iteration budget in the table, not the condition."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "tests")]


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--commit", required=True, help="hash of the commit this checkout holds")
    p.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "python_layer_parent.json"))
    a = p.parse_args()
    import torch
    import test_python_layer_parity_gpu as table
    from graphik_amd import build
    assert torch.cuda.is_available(), "recording needs the MI355X"
    scenarios, refused = {}, []
    for name, run in table.SCENARIOS.items():
        arrays = run()
        rec = {"sha": table.digest(arrays), "conditions": table.conditions(name, arrays)}
        if table.digest(run()) != rec["sha"]:
            refused.append(name + ": two runs differ")
        refused += [f"{name}: {key} == 0" for key, count in rec["conditions"].items() if count == 0]
        print(name, len(rec["sha"]), "keys", rec["conditions"], flush=True)
        scenarios[name] = rec
    if refused:
        print("refused:\n  " + "\n  ".join(refused))
        return 1
    doc = {"library": "parent commit " + a.commit, "library_source_digest": build.source_digest(),
           "hash": "sha256 over (dtype, shape) and the bytes of every returned array, by key; not hashed: "
                   + ", ".join(table.NOT_HASHED) + " and keys that begin with _",
           "scenarios": scenarios}
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
