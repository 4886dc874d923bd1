"""tests/golden/module_trace_golden.json: the ordered profiler records (s3r_profile_detail(1)) of one call of every network, partial
chain, read-out and training step of tests/_module_trace_cases.py — what the Python layer enqueues through the C-ABI, call by call.
Every field but `ms` is compared exactly, the doubles too: the library that computes them is the one the golden was taken from, and
JSON holds a double as its shortest exact decimal.

launch_conv_mfma plans a direct layer's launches against the device's compute-unit count: on a device with another count than
the file's, `launches` and `launch_form` of the direct conv_mfma records are left out, and the test says so."""
import json
import os

import pytest
import torch

from tests import _dispatch_cases as DC
from tests import _module_trace_cases as MC

pytestmark = pytest.mark.gpu
F_MFMA = 0


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "module_trace_golden.json")))


def test_the_golden_covers_every_case(golden):
    assert sorted(golden["cases"]) == sorted(MC.IDS) and tuple(golden["fields"]) == MC.FIELDS
    assert all(golden["cases"][i] for i in MC.IDS)
    assert max(len(r) for r in golden["cases"].values()) < MC.CAP


@pytest.mark.parametrize("cid", MC.IDS)
def test_module_trace(s3r, golden, monkeypatch, cid):
    same_device = golden["compute_units"] == DC.compute_units()
    got, _, _ = MC.trace(s3r.load_library(), MC.BY_ID[cid], lambda n: monkeypatch.setattr(s3r.modules, "MAX_CHUNK", n))
    want = [dict(zip(golden["fields"], row)) for row in golden["cases"][cid]]
    assert len(got) == len(want), (cid, len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        skip = ()
        if not same_device and w["family"] == F_MFMA and w["algo"] == 0:
            skip = ("launches", "launch_form")
            print(f"\n{cid} record {i}: another compute-unit count than the golden's {golden['compute_units']}: launches and launch_form not compared")
        for k in MC.FIELDS:
            assert k in skip or g[k] == w[k], (cid, i, k, g, w)
