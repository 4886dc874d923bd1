"""Writes tests/golden/module_trace_golden.json: the profiler records of every module call of tests/_module_trace_cases.py, taken from
the tree BEFORE a change to the Python layer (modules.py, ops.py, _tensors.py) that is meant to keep what it enqueues.  On the MI355X:

    python tests/golden/make_module_trace_golden.py                      # the golden; --commit names the commit it was taken from
    python tests/golden/make_module_trace_golden.py --hashes FILE        # instead: the sha256 of every tensor each case returns

The hashes (a training case: every parameter's .grad and every buffer afterwards too) depend on the torch build, so FILE is not
committed: write one before and one after the change on the same machine and compare the two.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "module_trace_golden.json")


def _commit():
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 else "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=GOLDEN)
    ap.add_argument("--hashes", default=None, metavar="FILE")
    a = ap.parse_args()
    import s3r
    from tests import _dispatch_cases as DC
    from tests import _module_trace_cases as MC
    lib = s3r.load_library()
    saved = s3r.modules.MAX_CHUNK
    records, hashes = {}, {}
    for c in MC.CASES:
        try:
            records[c.id], state, out = MC.trace(lib, c, lambda n: setattr(s3r.modules, "MAX_CHUNK", n))
        finally:
            s3r.modules.MAX_CHUNK = saved
        if a.hashes:
            hashes[c.id] = MC.hashes(c, state, out)
        print(f"{c.id}: {len(records[c.id])} records", flush=True)
    path = a.hashes or a.out
    with open(path, "w") as f:
        if a.hashes:
            json.dump(hashes, f, indent=0, sort_keys=True)
            f.write("\n")
        else:
            MC.dump_golden(dict(generated_at_commit=a.commit or _commit(), compute_units=DC.compute_units(), fields=list(MC.FIELDS),
                                cases={cid: MC.rows(r) for cid, r in records.items()}), f)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
