"""The launch forms launch_conv_mfma takes by itself above one round of workgroups — the tail cut as one launch (conv_glds_dual_kernel)
and as two (the remainder a 64 x 64-tile launch with n_begin != 0, on the six-stage ring), and the 64 x 64 tile on both sides of the
ring's 384 workgroups — against the float64 reference BIT FOR BIT on integer lattices, and the profiler record's launch_form and
launches against tests/_launch_cases.py's restatement of the plan at THIS device's compute-unit count.

Every case goes through tests/_abi_bodies.py::conv_forward: s3r_conv_pack_weights + s3r_conv_forward with every argument in a
guarded allocation (tests/_guard.py), over NaN-filled and zero-filled scratch; guards intact, no poison left in the interior, the
output halo untouched, the same bits from both runs, then tests/test_exact_gpu.py's bit comparison with the reference.

That the forms under test are the ones that ran is asserted, never assumed: a case whose record differs from form(case, cus) fails,
whether the library stopped cutting (a constant of plan_tail_cut moved) or the restatement fell behind the kernel file.  On a device
with another compute-unit count other rows cut; the equality still holds, and test_every_form_is_reached fails — it does not skip —
if the table no longer reaches one of the four forms there (it then needs rows sized for that device).
"""
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _abi_bodies as AB
from tests import _launch_cases as LC
from tests import test_exact_gpu as XG

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib(s3r):
    return s3r.load_library()


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def run_case(s3r, lib, c):
    """the case guarded and twice, bit for bit against the reference; its two conv_mfma profiler records"""
    x, p, want = XG._data(c.data)
    s3r.profile_enable(16)
    try:
        got = AB.conv_forward(s3r, lib, c, x, p)
        rec = [r for r in s3r.profile_read(16) if r["family"] == "conv_mfma"]
    finally:
        s3r.profile_enable(0)
    XG.assert_bits(got.contiguous(), want, c.data, p, c.id)
    assert len(rec) == 2 and all(r["ran"] == "direct" for r in rec), (c.id, rec)
    return rec


@pytest.mark.parametrize("case", LC.CASES, ids=[c.id for c in LC.CASES])
def test_launch_form_is_exact_and_is_the_planned_one(s3r, lib, cus, case):
    rec = run_case(s3r, lib, case)
    want = LC.form(case, cus)
    got = [(r["launch_form"], r["launches"]) for r in rec]
    print(f"\n{case.id}: cus {cus} (launch_form, launches) {got} restated {want}")
    assert got == [want, want], (case.id, "launch_form, launches", got, "restated", want, "compute units", cus)


def test_every_form_is_reached(cus):
    kinds = {}
    for c in LC.CASES:
        kinds.setdefault(LC.kind(LC.form(c, cus)[0], c), []).append(c.id)
    missing = [k for k in ("one-launch", "two-launch", "ring", "two-stage") if not kinds.get(k)]
    assert not missing, (f"on {cus} compute units no row of tests/_launch_cases.py reaches", missing)
    # where a two-launch cut exists, its remainder is the ring on a sub-range
    assert any(LC.form(c, cus)[0] == LC.FORM_CUT | LC.FORM_RING for c in LC.CASES)


_CHILD = r"""
import json, sys
sys.path.insert(0, %r)
import s3r
from tests import _launch_cases as LC
from tests import test_launch_forms_gpu as T
lib = s3r.load_library()
out = {}
for c in LC.ONE_LAUNCH:
    out[c.id] = [(r["launch_form"], r["launches"]) for r in T.run_case(s3r, lib, c)]
json.dump(out, open(sys.argv[1], "w"))
"""


def test_one_launch_rows_as_two_launches(cus, tmp_path):
    """S3R_NO_DUAL (read once per process: a child): the same descriptors, guarded and bit for bit against the reference in the child
    exactly as above, with the bulk and the remainder as two launches wherever the two-launch cost model cuts as well"""
    out = tmp_path / "forms.json"
    env = dict(os.environ, S3R_NO_DUAL="1")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(out)], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    got = json.load(open(out))
    assert sorted(got) == sorted(c.id for c in LC.ONE_LAUNCH)
    two = 0
    for c in LC.ONE_LAUNCH:
        want = LC.form(c, cus, dual_built=False)
        assert [tuple(v) for v in got[c.id]] == [want, want], (c.id, got[c.id], "restated", want, "compute units", cus)
        assert not want[0] & LC.FORM_ONE_LAUNCH
        two += want[1] == 2
    if any(LC.form(c, cus)[0] & LC.FORM_ONE_LAUNCH for c in LC.ONE_LAUNCH):
        assert two, "no one-launch row cuts under the two-launch model on this device"
