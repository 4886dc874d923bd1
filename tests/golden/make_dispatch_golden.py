"""Writes tests/golden/dispatch_golden.json: what the forward dispatcher answers and records (tests/_dispatch_cases.py), taken from
the build BEFORE a change to csrc/s3r_conv_forward.hip or csrc/s3r_plan_*.hip that is meant to keep them.

    python tests/golden/make_dispatch_golden.py --part host          # sizes and scratch refusals: no GPU needed
    python tests/golden/make_dispatch_golden.py --part gpu           # profiler records: on the MI355X

Each part replaces its own keys of the file and keeps the other's.  --commit names the commit the library was built from.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "dispatch_golden.json")


def _commit():
    r = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True)
    return r.stdout.strip() if r.returncode == 0 else "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("host", "gpu"), required=True)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--out", default=GOLDEN)
    a = ap.parse_args()
    import s3r
    from tests import _dispatch_cases as DC
    lib = s3r.load_library()
    doc = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    doc["generated_at_commit"] = a.commit or doc.get("generated_at_commit") or _commit()
    if a.part == "host":
        doc["host"] = DC.host_part(lib)
    else:
        doc["compute_units"] = DC.compute_units()
        doc["gpu"] = DC.gpu_part(lib)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{a.part}: wrote {a.out} ({os.path.getsize(a.out)} bytes)")


if __name__ == "__main__":
    main()
