"""Kernel mutants on the GPU: every entry of tests/mutants/table.py, built by `make -C .../csrc mutants` into
build/mutants/<id>.so, must make one of its `kills` tests fail with an assertion.

One fresh child per mutant, one at a time, no retries:  timeout -k 10 180 python -m pytest -x -q -p no:cacheprovider <kills>
with S3R_LIB = the mutant's library (180 s: one interpreter start, one torch import, a few few-second tests).
  child exits 1 and its output names an AssertionError in a failed test of the kills   -> killed: the test passes
  child exits 0                                                                        -> survived: the test fails, naming the mutant
                                                                                          (an entry marked `equivalent` must survive)
  anything else (a signal, a time limit, a HIP error in the output)                    -> the test fails and a module-level flag fails
                                                                                          every remaining mutant test without a child:
                                                                                          nothing more goes to the GPU after an abnormal end
A control runs the stock library through the same runner and expects exit 0: the runner is not what fails."""
import os
import re
import runpy
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANTS = runpy.run_path(os.path.join(ROOT, "tests", "mutants", "table.py"))["MUTANTS"]
STOCK = os.path.join(ROOT, "stereo-3d-reconstruction_amd", "csrc", "libs3r_hip.so")
LIMIT_S = 180
HIP_ERROR = re.compile(r"illegal memory access|hipError(?!InvalidValue|NotSupported)\w+|HSA_STATUS_ERROR|Memory access fault|core dumped", re.I)

pytestmark = pytest.mark.gpu

_abnormal = []          # the first child that ended abnormally: (who, why)


def run_child(lib, kills):
    """-> (exit status, output) of one fresh pytest child on `lib`"""
    env = dict(os.environ, S3R_LIB=lib, PYTHONDONTWRITEBYTECODE="1")
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, "-m", "pytest", "-x", "-q", "-p", "no:cacheprovider", *kills]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    return r.returncode, r.stdout


def verdict(rc, out):
    """'killed' / 'survived' / 'abnormal: why'"""
    if HIP_ERROR.search(out):
        return "abnormal: a HIP error in the child's output"
    if rc == 0:
        return "survived"
    if rc == 1:
        failed = re.findall(r"^FAILED (\S+)", out, re.M)
        if failed and re.search(r"\bAssertionError\b|^E\s+assert ", out, re.M):
            return "killed"
        return "abnormal: exit 1 without an AssertionError in a failed test"
    return f"abnormal: exit status {rc}"


def _guard():
    if _abnormal:
        pytest.fail(f"not run: the child of {_abnormal[0][0]} ended abnormally ({_abnormal[0][1]}); nothing more goes to the GPU")


def _run(who, lib, kills):
    _guard()
    assert os.path.exists(lib), f"{os.path.relpath(lib, ROOT)} is not built: make -C stereo-3d-reconstruction_amd/csrc mutants"
    rc, out = run_child(lib, kills)
    v = verdict(rc, out)
    print(f"{who}: child exit {rc}: {v}")
    if os.environ.get("S3R_MUTANT_REPORT"):             # id, verdict, first failed test: the rows of docs/LAB_NOTES.md's table
        first = re.search(r"^FAILED (\S+)", out, re.M)
        with open(os.environ["S3R_MUTANT_REPORT"], "a") as f:
            f.write(f"{who}\t{v}\t{first.group(1) if first else '-'}\n")
    print(out[-3000:])
    if v.startswith("abnormal"):
        _abnormal.append((who, v))
        pytest.fail(f"{who}: {v}\n{out[-3000:]}")
    return v, out


def test_stock_library_passes_through_the_same_runner():
    v, out = _run("stock", STOCK, ["tests/test_exact_gpu.py::test_linear[p1-B1]",
                                   "tests/test_selection_gpu.py::test_metrics_on_signed_zero_subnormal_and_overflowing_values"])
    assert v == "survived", f"the stock library fails in the mutant runner:\n{out[-3000:]}"
    assert re.search(r"\b2 passed\b", out), out[-1000:]


@pytest.mark.parametrize("m", MUTANTS, ids=[m["id"] for m in MUTANTS])
def test_mutant_is_killed(m):
    v, out = _run(m["id"], os.path.join(ROOT, "build", "mutants", m["id"] + ".so"), m["kills"])
    if m.get("equivalent"):
        assert v == "survived", f"mutant {m['id']} is marked equivalent but a test fails on it: drop the mark\n{out[-3000:]}"
    else:
        assert v == "killed", f"mutant {m['id']} SURVIVED its kills {m['kills']}: {m['models']}\n{out[-1500:]}"
