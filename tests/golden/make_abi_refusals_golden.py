"""Writes tests/golden/abi_refusals.json: what the C-ABI entry points answer to the refused calls of tests/_refusal_cases.py, taken
from the build BEFORE a change to the entry-point sources (csrc/s3r_api_*.hip, csrc/s3r_host.h) that is meant to keep them.

    python tests/golden/make_abi_refusals_golden.py          # no GPU needed: the calls are made where no device is visible

The calls run in a child process (tests/_refusal_cases.py); it also checks that every baseline passes all of its entry's checks.
--commit names the commit the library was built from.  Nothing is written when a case reached a launch (S3R_ERR_HIP).
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_refusals.json")


def _commit():
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 else "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    from tests import _refusal_cases as RC
    cases = RC.run_in_child(check_baseline=True)
    assert list(cases) == RC.CASE_IDS
    launched = [cid for cid, (rc, _) in cases.items() if rc == RC.ERR_HIP]
    if launched:
        sys.exit("not written: these cases were not refused, they reached a launch:\n  " + "\n  ".join(launched))
    with open(a.out, "w") as f:
        json.dump(dict(generated_at_commit=a.commit or _commit(), cases=cases), f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {a.out}: {len(cases)} cases ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
